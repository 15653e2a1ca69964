"""CPU: both forms of p3p_ransac_kernel (host pairs, device-resident frames) exist in the gfx950 code object of p3p.hip, use no scratch
memory -- the four poses of a lane's hypothesis are statically indexed slots and live in registers -- and have the occupancy the
design states: one wavefront per SIMD, i.e. one four-wavefront workgroup (one problem) per compute unit (read from the compiler's
resource remarks, the method of test_kernel_resources.py)."""
from test_kernel_resources import resources


def test_p3p_kernels_exist_and_do_not_spill():
    res = resources("p3p.hip")
    for k in ("p3p_ransac_kernelILb0", "p3p_ransac_kernelILb1"):
        hits = {n: v for n, v in res.items() if k in n}
        assert hits, f"{k}: no such kernel in p3p.hip ({sorted(res)})"
        for n, v in hits.items():
            assert v.get("ScratchSize") == 0, f"{n}: {v}"
            assert v.get("Occupancy") >= 1, f"{n}: {v}"
            assert v.get("LDS Size", 0) <= 1024, f"{n}: static LDS beside the dynamic pair planes: {v}"
