"""CPU: snake_slam_amd/csrc/covis_core.hpp and the covisibility part of dispatch.hpp compiled with plain g++ (no HIP) into
tests/cpp/covis_core_driver.cpp.  The per-set statements -- gate, count, emit rule, key and the cut by one counting pass per bit -- must
equal the restatement (tests/covis_numpy.py, a dictionary loop and a real sort) byte for byte, and the long-list threshold and the carve
formula are pinned."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import covis_numpy as M

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("covis_core") / "covis_core_driver"
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{ROOT / 'include'}", f"-I{ROOT / 'snake_slam_amd' / 'csrc'}",
           str(ROOT / "tests" / "cpp" / "covis_core_driver.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_driver(exe, d, m, cap, q=None, set_start=None, set_point=None, th=M.TH, th_depth=M.TH_DEPTH):
    vote = q is None
    start, point = (set_start, np.asarray(set_point).reshape(-1)) if vote else (m["feat_start"], m["feat_point"])
    n_sets = len(start) - 1 if vote else len(q)
    for name in M.MAP_KEYS:
        np.ascontiguousarray(m[name]).tofile(d / f"{name}.bin")
    np.ascontiguousarray(start, np.int32).tofile(d / "item_start.bin")
    np.ascontiguousarray(point, np.int32).tofile(d / "item_point.bin")
    if not vote:
        np.ascontiguousarray(m["feat_depth"], np.float32).tofile(d / "item_depth.bin")
        np.ascontiguousarray(q, np.int32).tofile(d / "q.bin")
    np.array([int(vote), len(m["kf_bad"]), len(m["pt_flags"]), len(m["obs"]), len(point), n_sets, th, cap], np.int32).tofile(d / "meta.bin")
    np.array([th_depth], np.float32).tofile(d / "th_depth.bin")
    r = subprocess.run([str(exe), str(d)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return np.fromfile(d / "conn.bin", M.CONN).reshape(n_sets, cap), np.fromfile(d / "res.bin", M.RESULT)


def same(got, want):
    return got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


@pytest.mark.parametrize("cap", [1, 4, 64, 256])
def test_core_statements_equal_the_restatement_on_the_edge_case(driver, tmp_path, cap):
    c = M.edge_case()
    assert same(run_driver(driver, tmp_path, c, cap, q=c["q"]), M.update(c, c["q"], cap=cap))
    assert same(run_driver(driver, tmp_path, c, cap, set_start=c["set_start"], set_point=c["set_point"]), M.vote(c, c["set_start"], c["set_point"], cap=cap))


@pytest.mark.parametrize("n_kf", [1, 2, 255, 256, 257])
def test_core_statements_at_every_keyframe_count(driver, tmp_path, n_kf):
    c = M.edge_case(n_kf)
    assert same(run_driver(driver, tmp_path, c, 64, q=c["q"]), M.update(c, c["q"], cap=64))
    assert same(run_driver(driver, tmp_path, c, 64, set_start=c["set_start"], set_point=c["set_point"]), M.vote(c, c["set_start"], c["set_point"], cap=64))


def test_core_statements_equal_the_restatement_on_a_structured_map(driver, tmp_path):
    m = M.make_map(21, 400, 8000)
    q = np.arange(400, dtype=np.int32)
    for cap, th in ((8, M.TH), (256, M.TH), (8, 1)):  # 8: most lists are cut; th = 1: every touched keyframe that is not bad
        want = M.update(m, q, th=th, cap=cap)
        assert same(run_driver(driver, tmp_path, m, cap, q=q, th=th), want)
    assert np.mean(want[1]["n_found"] > 8) > 0.9
    ss, sp = M.frames_of(m, 22, 50)
    assert same(run_driver(driver, tmp_path, m, 16, set_start=ss, set_point=sp), M.vote(m, ss, sp, cap=16))


def test_long_list_threshold_and_carve_are_pinned(driver):
    line = subprocess.run([str(driver), "--consts"], capture_output=True, text=True, check=True).stdout.split()
    k = dict(zip(line[::2], map(int, line[1::2])))
    assert k["long_min"] == M.LONG_MIN == 32 and k["long_min_env0"] == 0 and k["long_min_env7"] == 7
    assert k["threads"] == 256 and k["max_kf"] == M.MAX_KF == 32768 and k["max_cap"] == M.MAX_CAP == 4096
    assert k["sort_len_1000_64"] == 64 and k["sort_len_40_64"] == 64 and k["sort_len_max"] == 4096
    # a u32 counter per keyframe + the ids to sort + a queue entry per lane + 32 words
    assert k["carve_max"] == 32768 * 4 + 4096 * 4 + 256 * 4 + 128 <= 160 * 1024
    assert k["carve_4096_64"] == 4096 * 4 + 64 * 4 + 256 * 4 + 128
    assert k["carve_1_1"] == 4 * 4 + 4 * 4 + 256 * 4 + 128
