"""CPU: every kernel of bow.hip exists exactly once in the gfx950 code object, uses no scratch memory, spills no register, and has the
occupancy the kernel table of DESIGN.md section 3g states (the compiler's resource remarks for this build: wavefronts per SIMD by
registers and static LDS; the method of test_kernel_resources.py)."""
from test_kernel_resources import resources

# kernel -> (wavefronts per SIMD, static LDS bytes) as DESIGN.md section 3g lists them
TABLE = {
    "bow_descent_kernel": (8, 0),
    "bow_finish_kernel": (6, 24640),
    "bow_db_store_kernel": (8, 0),
    "bow_db_score_kernel": (6, 24576),
    "bow_db_select_kernel": (8, 4096),
    "bow_match_kernel": (8, 10256),
}


def test_bow_kernels_exist_once_and_do_not_spill():
    res = resources("bow.hip")
    kernels = {n: v for n, v in res.items() if "Occupancy" in v}
    assert len(kernels) == len(TABLE), sorted(kernels)
    for k, (occupancy, lds) in TABLE.items():
        hits = {n: v for n, v in kernels.items() if k in n}
        assert len(hits) == 1, f"{k}: {sorted(hits)} in {sorted(res)}"
        (n, v), = hits.items()
        assert v.get("ScratchSize") == 0, f"{n}: {v}"
        assert v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0, f"{n}: {v}"
        assert v.get("Occupancy") == occupancy, f"{n}: {v}"
        assert v.get("LDS Size", 0) == lds, f"{n}: {v}"


def test_design_states_the_same_table():
    from pathlib import Path

    text = (Path(__file__).resolve().parent.parent / "DESIGN.md").read_text()
    sec = text[text.index("## 3g."):]
    for k, (occupancy, lds) in TABLE.items():
        row = next(line for line in sec.splitlines() if line.startswith(f"| `{k}`"))
        cells = [c.strip() for c in row.strip("|").split("|")]
        assert int(cells[-1]) == occupancy and int(cells[-2].replace(" ", "")) == lds, row
