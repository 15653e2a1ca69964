"""CPU: both forms of sim3_ransac_kernel (host pairs, device-resident pairs) exist in the gfx950 code object of sim3.hip, use no scratch
memory -- the transform of a lane's hypothesis lives in registers -- and have the occupancy DESIGN.md section 3e states: three
wavefronts per SIMD by registers, i.e. up to three four-wavefront workgroups (problems) per compute unit while their pair planes fit
the LDS (read from the compiler's resource remarks, the method of test_kernel_resources.py)."""
from test_kernel_resources import resources


def test_sim3_kernels_exist_and_do_not_spill():
    res = resources("sim3.hip")
    for k in ("sim3_ransac_kernelILb0", "sim3_ransac_kernelILb1"):
        hits = {n: v for n, v in res.items() if k in n}
        assert hits, f"{k}: no such kernel in sim3.hip ({sorted(res)})"
        for n, v in hits.items():
            assert v.get("ScratchSize") == 0, f"{n}: {v}"
            assert v.get("VGPRs Spill", 0) == 0, f"{n}: {v}"
            assert v.get("Occupancy") == 3, f"{n}: {v}"
            assert v.get("LDS Size", 0) <= 1024, f"{n}: static LDS beside the dynamic pair planes: {v}"
