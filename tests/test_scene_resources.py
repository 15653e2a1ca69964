"""CPU: scene_window_kernel and scene_gather_kernel exist once each in the gfx950 code object of scene.hip, use no scratch memory and
declare no static LDS: every byte a workgroup uses is in the dynamic carve that dispatch.hpp states, which at the limits
(SNK_LMAP_MAX_PTS points, SNK_SCENE_MAX_IMG images) stays inside a compute unit's 160 KiB.  At the reference's sizes (a window of 36
keyframes, pt_cap 16 384, img_cap 512) the carve is the point table's 128.9 KiB: one workgroup of four wavefronts on a compute unit, which is
what DESIGN.md section 3k claims; the registers allow more, so a smaller pt_cap packs more (nine workgroups at pt_cap 2 048, img_cap 128).
Read from the compiler's resource remarks, the method of test_covis_resources.py; the carves through tests/cpp/scene_core_driver.cpp.
The library exports the four entry points that the header's section declares, and the binding table lists them."""
import re
import subprocess
from pathlib import Path

from test_kernel_resources import resources
from test_scene_core_cpu import driver  # noqa: F401  (fixture)

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ["snk_scene_gather", "snk_scene_gather_batch_dev", "snk_scene_window", "snk_scene_window_batch_dev"]


def test_scene_kernels_exist_do_not_spill_and_keep_their_lds_in_the_carve(driver):  # noqa: F811
    res = resources("scene.hip")
    for k in ("scene_window_kernel", "scene_gather_kernel"):
        hits = {n: v for n, v in res.items() if k in n}
        assert len(hits) == 1, f"{k}: not exactly one such kernel in scene.hip ({sorted(res)})"
        for n, v in hits.items():
            assert v.get("ScratchSize") == 0, f"{n}: {v}"
            assert v.get("LDS Size") == 0, f"{n}: static LDS beside the carve: {v}"
            # four workgroups of four wavefronts on a compute unit are four wavefronts per SIMD: the registers must allow them
            assert v.get("Occupancy") >= 4, f"{n}: {v}"
    assert len([n for n in res if "scene_" in n and "kernel" in n]) == 2
    line = subprocess.run([str(driver), "--consts"], capture_output=True, text=True, check=True).stdout.split()
    k = dict(zip(line[::2], map(int, line[1::2])))
    assert k["gather_carve_max"] <= 160 * 1024 and k["window_carve"] <= 160 * 1024
    assert 1 * k["gather_carve_ref"] <= 160 * 1024  # one workgroup per compute unit at pt_cap 16 384
    assert 9 * k["gather_carve_2048_128"] <= 160 * 1024


def test_exported_symbols_match_the_header_section():
    from snake_slam_amd import _lib

    text = (ROOT / "include" / "snake_hip.h").read_text()
    start = text.index("Local BA windows (snk-scene v1)")
    end = text.index("Local map of fine tracking (snk-lmap v1)")  # the section stands in front of snk-lmap's, whose own test reads up to the next one
    assert text.index("Covisibility: connection lists") < start < end < text.index("Pose refinement (the step after")
    section = re.sub(r"/\*.*?\*/", "", text[start:end], flags=re.S)
    declared = sorted(set(re.findall(r"SNK_API\s+[\w\s\*]+?\b(snk_\w+)\s*\(", section)))
    assert declared == ENTRIES
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("snk_scene_")) == ENTRIES
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert sorted(s for s in re.findall(r" T (\w+)", out) if "snk_scene" in s) == ENTRIES
    for name, value in (("SNK_SCENE_MAX_WINDOW", 64), ("SNK_SCENE_MAX_IMG", 4096), ("SNK_SCENE_MAX_OBS", 4194304), ("SNK_SCENE_OK", 0),
                        ("SNK_SCENE_SKIPPED", 1), ("SNK_SCENE_WINDOW_OVERFLOW", 2), ("SNK_SCENE_PTS_OVERFLOW", 3), ("SNK_SCENE_IMG_OVERFLOW", 4),
                        ("SNK_SCENE_OBS_OVERFLOW", 5), ("SNK_SCENE_BAD_INDEX", 6), ("SNK_SCENE_PT_CONST", 4)):
        assert re.search(rf"#define {name} {value}\b", text), name
