"""CPU: lmap_select_kernel and lmap_gather_kernel exist once each in the gfx950 code object of localmap.hip, use no scratch memory and
declare no static LDS: every byte a workgroup uses is in the dynamic carve that dispatch.hpp states, which at the limits
(SNK_COVIS_MAX_KF keyframes, SNK_LMAP_MAX_LOCAL_KF x SNK_LMAP_MAX_NEIGHBOURS candidates; SNK_LMAP_MAX_PTS points) stays inside a compute
unit's 160 KiB and at the reference's sizes lets several workgroups share one (read from the compiler's resource remarks, the method of
test_covis_resources.py; the carves through tests/cpp/lmap_core_driver.cpp).  The library exports the four entry points that the
header's section declares, and the binding table lists them."""
import re
import subprocess
from pathlib import Path

from test_kernel_resources import resources
from test_localmap_core_cpu import driver  # noqa: F401  (fixture)

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ["snk_lmap_gather", "snk_lmap_gather_batch_dev", "snk_lmap_select", "snk_lmap_select_batch_dev"]


def test_localmap_kernels_exist_do_not_spill_and_keep_their_lds_in_the_carve(driver):  # noqa: F811
    res = resources("localmap.hip")
    for k in ("lmap_select_kernel", "lmap_gather_kernel"):
        hits = {n: v for n, v in res.items() if k in n}
        assert len(hits) == 1, f"{k}: not exactly one such kernel in localmap.hip ({sorted(res)})"
        for n, v in hits.items():
            assert v.get("ScratchSize") == 0, f"{n}: {v}"
            assert v.get("LDS Size") == 0, f"{n}: static LDS beside the carve: {v}"
            # four workgroups of four wavefronts on a compute unit are four wavefronts per SIMD: the registers must allow them
            assert v.get("Occupancy") >= 4, f"{n}: {v}"
    assert len([n for n in res if "lmap_" in n and "kernel" in n]) == 2
    line = subprocess.run([str(driver), "--consts"], capture_output=True, text=True, check=True).stdout.split()
    k = dict(zip(line[::2], map(int, line[1::2])))
    assert k["select_carve_max"] <= 160 * 1024 and k["gather_carve_max"] <= 160 * 1024
    assert 8 * k["select_carve_4096_64_5"] <= 160 * 1024  # 4096 keyframes, kf_cap 64, five neighbours
    assert 8 * k["gather_carve_64_2048"] <= 160 * 1024  # pts_cap 2048: the table is 16 KiB


def test_exported_symbols_match_the_header_section():
    from snake_slam_amd import _lib

    text = (ROOT / "include" / "snake_hip.h").read_text()
    start = text.index("Local map of fine tracking (snk-lmap v1)")
    assert text.index("Covisibility: connection lists") < start < text.index("Pose refinement (the step after")
    section = re.sub(r"/\*.*?\*/", "", text[start:text.index("Pose refinement (the step after")], flags=re.S)
    declared = sorted(set(re.findall(r"SNK_API\s+[\w\s\*]+?\b(snk_\w+)\s*\(", section)))
    assert declared == ENTRIES
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("snk_lmap_")) == ENTRIES
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert sorted(s for s in re.findall(r" T (\w+)", out) if "lmap" in s) == ENTRIES
    for name, value in (("SNK_LMAP_MAX_LOCAL_KF", 256), ("SNK_LMAP_MAX_PTS", 16384), ("SNK_LMAP_MAX_NEIGHBOURS", 16), ("SNK_LMAP_OK", 0),
                        ("SNK_LMAP_EMPTY", 1), ("SNK_LMAP_TRUNCATED", 2), ("SNK_LMAP_KF_OVERFLOW", 3), ("SNK_LMAP_PTS_OVERFLOW", 4),
                        ("SNK_LMAP_BAD_INDEX", 5)):
        assert re.search(rf"#define {name} {value}\b", text), name
