"""CPU: the kernels of snk_triangulate_pairs / snk_triangulate_neighbours exist in the gfx950 code object of triangulate.hip and use no
scratch memory -- the 4 x 4 one-sided Jacobi of the per-pair thread is statically indexed and lives in registers (read from the
compiler's resource remarks, the method of test_kernel_resources.py)."""
from test_kernel_resources import resources


def test_triangulation_kernels_exist_and_do_not_spill():
    res = resources("triangulate.hip")
    for k in ("tri_pairs_kernel", "tri_commit_kernel"):
        hits = {n: v for n, v in res.items() if k in n}
        assert hits, f"{k}: no such kernel in triangulate.hip ({sorted(res)})"
        for n, v in hits.items():
            assert v.get("ScratchSize") == 0, f"{n}: {v}"
