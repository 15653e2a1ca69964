"""CPU: the kernels of pgo.hip exist in the gfx950 code object, use no scratch memory and do not spill (read from the compiler's resource
remarks, the method of test_kernel_resources.py), and have exactly the occupancy by registers (wavefronts per SIMD) that the table of
DESIGN.md section 3f states: the linearisation 256 VGPRs and one wavefront per SIMD (its three work matrices per lane sit in 75 264 bytes
of dynamic LDS: two 64-lane workgroups per compute unit); the resident PCG 70 VGPRs and seven, so registers never limit its one
256-thread workgroup per compute unit -- the 150 KB of dynamic LDS do.  A change of the LDS / register trade of any kernel shows here."""
from test_kernel_resources import resources

# kernel: (wavefronts per SIMD by registers, VGPRs where DESIGN.md states them)
KERNELS = {"pgo_linearise_kernel": (1, 256), "pgo_assemble_kernel": (8, None), "pgo_damp_kernel": (8, None), "pgo_pcg_kernelILb1": (7, 70),
           "pgo_pcg_kernelILb0": (8, None), "pgo_update_kernel": (5, None), "pgo_cost_kernel": (4, None), "pgo_decide_kernel": (8, None),
           "pgo_commit_kernel": (8, None), "pgo_transform_points_kernel": (5, None)}


def test_pgo_kernels_exist_and_do_not_spill():
    res = resources("pgo.hip")
    for k, (occupancy, vgprs) in KERNELS.items():
        hits = {n: v for n, v in res.items() if k in n}
        assert len(hits) == 1, f"{k}: not exactly one such kernel in pgo.hip ({sorted(res)})"
        for n, v in hits.items():
            assert v.get("ScratchSize") == 0, f"{n}: {v}"
            assert v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0, f"{n}: {v}"
            assert v.get("Occupancy") == occupancy, f"{n}: {v}"
            assert vgprs is None or v.get("VGPRs") == vgprs, f"{n}: {v}"
            assert v.get("LDS Size", 0) <= 8192, f"{n}: static LDS beside the dynamic carve: {v}"
