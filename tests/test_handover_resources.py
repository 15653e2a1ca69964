"""CPU: ho_count_kernel and ho_fill_kernel -- the device stage behind snk_ba_set_problems_dev -- exist once each in the gfx950 code object
of ba_handover.hip, use no scratch memory and declare no static LDS: every byte a workgroup uses is in the dynamic carve that
handover_core.hpp states (pinned by tests/test_handover_core_cpu.py).  Read from the compiler's resource remarks, the method of
test_scene_resources.py.  The entry point is declared inside the header's Local-BA section, exported, and in the binding table."""
import re
import subprocess
from pathlib import Path

from test_kernel_resources import resources

ROOT = Path(__file__).resolve().parent.parent


def test_handover_kernels_exist_once_do_not_spill_and_keep_their_lds_in_the_carve():
    res = resources("ba_handover.hip")
    for k in ("ho_count_kernel", "ho_fill_kernel"):
        hits = {n: v for n, v in res.items() if k in n}
        assert len(hits) == 1, f"{k}: not exactly one such kernel in ba_handover.hip ({sorted(res)})"
        for n, v in hits.items():
            assert v.get("ScratchSize") == 0, f"{n}: {v}"
            assert v.get("LDS Size") == 0, f"{n}: static LDS beside the carve: {v}"
            # the carve, not the registers, bounds the workgroups of a compute unit: two at the limit are two wavefronts per SIMD
            assert v.get("Occupancy") >= 4, f"{n}: {v}"
    assert len([n for n in res if "ho_" in n and "kernel" in n]) == 2


def test_entry_point_is_declared_in_the_local_ba_section_exported_and_bound():
    from snake_slam_amd import _lib

    text = (ROOT / "include" / "snake_hip.h").read_text()
    start = text.index(" * Local bundle adjustment\n")
    end = text.index("Pose-graph optimisation of the loop corrector")
    section = re.sub(r"/\*.*?\*/", "", text[start:end], flags=re.S)
    declared = set(re.findall(r"SNK_API\s+[\w\s\*]+?\b(snk_\w+)\s*\(", section))
    assert {"snk_ba_set_problems", "snk_ba_set_problems_dev"} <= declared
    m = re.search(r"SNK_API int snk_ba_set_problems_dev\(snk_ba\* h, int n_q, const snk_scene_out\* out_dev,\s*const double K\[4\], double bf\);", text)
    assert m and start < m.start() < end
    # what the header has to say to a caller (the issue's list)
    doc = text[text.index("The same hand-over from DEVICE memory"):m.start()]
    for phrase in ("complete on the BA handle's stream", "takes the\n * whole batch off the point-major pass", "rpc == NULL", "NO problem set"):
        assert phrase in doc, phrase
    assert "snk_ba_set_problems_dev" in _lib.SIGNATURES and len(_lib.SIGNATURES["snk_ba_set_problems_dev"][1]) == 5
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert "snk_ba_set_problems_dev" in re.findall(r" T (\w+)", out)
