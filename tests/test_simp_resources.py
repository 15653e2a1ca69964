"""CPU: simp_stats_kernel and simp_decide_kernel exist once each in the gfx950 code object of simp.hip, use no scratch memory and declare
no static LDS: every byte a workgroup uses is in the dynamic carve that dispatch.hpp states, which at the limits (SNK_SIMP_MAX_FEAT
features, SNK_SIMP_MAX_NODES nodes) stays inside a compute unit's 160 KiB.  Read from the compiler's resource remarks, the method of
test_scene_resources.py; the carves through tests/cpp/simp_core_driver.cpp.  The library exports the four entry points that the header's
section declares, and the binding table lists them."""
import re
import subprocess
from pathlib import Path

from test_kernel_resources import resources
from test_simp_core_cpu import driver  # noqa: F401  (fixture)

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ["snk_simp_decide", "snk_simp_decide_batch_dev", "snk_simp_stats", "snk_simp_stats_batch_dev"]


def test_simp_kernels_exist_do_not_spill_and_keep_their_lds_in_the_carve(driver):  # noqa: F811
    res = resources("simp.hip")
    for k in ("simp_stats_kernel", "simp_decide_kernel"):
        hits = {n: v for n, v in res.items() if k in n}
        assert len(hits) == 1, f"{k}: not exactly one such kernel in simp.hip ({sorted(res)})"
        for n, v in hits.items():
            assert v.get("ScratchSize") == 0, f"{n}: {v}"
            assert v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0, f"{n}: {v}"
            assert v.get("LDS Size") == 0, f"{n}: static LDS beside the carve: {v}"
            # several workgroups of four wavefronts share a compute unit at small caps: the registers must allow them
            assert v.get("Occupancy") >= 4, f"{n}: {v}"
    assert len([n for n in res if "simp_" in n and "kernel" in n]) == 2
    line = subprocess.run([str(driver), "--consts"], capture_output=True, text=True, check=True).stdout.split()
    k = dict(zip(line[::2], map(int, line[1::2])))
    assert k["stats_carve_max"] <= 160 * 1024 and k["decide_carve_max"] <= 160 * 1024
    assert 8 * k["stats_carve_4096"] <= 160 * 1024  # eight workgroups per compute unit at feat_cap 4 096
    assert 16 * k["decide_carve_64"] <= 160 * 1024  # and sixteen at node_cap 64 (the wavefront slots allow eight)


def test_exported_symbols_match_the_header_section():
    from snake_slam_amd import _lib

    text = (ROOT / "include" / "snake_hip.h").read_text()
    start = text.index("Keyframe culling (snk-simp v1) (DESIGN.md section 3l)")
    end = text.index("Multi-GPU result gather")
    assert text.index("Bag-of-words place recognition") < start < end  # directly in front of the multi-GPU section
    assert text[start:end].count("/* ----") == 1  # no other section between the two titles
    section = re.sub(r"/\*.*?\*/", "", text[start:end], flags=re.S)
    declared = sorted(set(re.findall(r"SNK_API\s+[\w\s\*]+?\b(snk_\w+)\s*\(", section)))
    assert declared == ENTRIES
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("snk_simp_")) == ENTRIES
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert sorted(s for s in re.findall(r" T (\w+)", out) if "snk_simp" in s) == ENTRIES
    for name, value in (("SNK_SIMP_MAX_NODES", 256), ("SNK_SIMP_MAX_FEAT", 16384), ("SNK_SIMP_OK", 0), ("SNK_SIMP_SKIPPED", 1),
                        ("SNK_SIMP_FEAT_OVERFLOW", 2), ("SNK_SIMP_NODES_OVERFLOW", 3), ("SNK_SIMP_BAD_INDEX", 4), ("SNK_SIMP_NONE", 0),
                        ("SNK_SIMP_FACTOR", 1), ("SNK_SIMP_NO_CONN", 2), ("SNK_SIMP_ANGLE", 3), ("SNK_SIMP_MATCHES", 4), ("SNK_SIMP_REDUNDANCY", 5),
                        ("SNK_SIMP_LINK", 6), ("SNK_SIMP_KEEP_IMU_WEIGHTS", 7), ("SNK_SIMP_KEEP_TIME_GAP", 8), ("SNK_SIMP_KEEP_BRANCH", 9),
                        ("SNK_SIMP_KEEP_DISCONNECTED", 10), ("SNK_SIMP_KEEP_LINK", 11)):
        assert re.search(rf"#define {name} {value}\b", text), name


def test_python_mirror_states_the_same_layouts_and_values():
    import ctypes as C

    import simp_numpy as M
    from snake_slam_amd import simp as S

    assert S.STATS_DTYPE == M.STATS_DTYPE and S.VERDICT_DTYPE == M.VERDICT_DTYPE and S.STATS_DTYPE.itemsize == 28 and S.VERDICT_DTYPE.itemsize == 32
    assert C.sizeof(S.SimpParams) == M.PARAMS_DTYPE.itemsize == 48 and C.sizeof(S.SimpStatsParams) == 16
    assert C.sizeof(S.SimpMap) == 16 + 10 * 8 and C.sizeof(S.SimpGraph) == 8 + 9 * 8
    assert (S.OK, S.SKIPPED, S.FEAT_OVERFLOW, S.NODES_OVERFLOW, S.BAD_INDEX) == (M.OK, M.SKIPPED, M.FEAT_OVERFLOW, M.NODES_OVERFLOW, M.BAD_INDEX)
    assert (S.FACTOR, S.LINK, S.KEEP_IMU_WEIGHTS, S.KEEP_LINK) == (M.FACTOR, M.LINK, M.KEEP_IMU_WEIGHTS, M.KEEP_LINK)
    assert {k: v for k, v in S.KeyframeCuller.DEFAULTS.items() if k in M.PARAMS} == M.PARAMS
