"""CPU: snake_slam_amd/csrc/simp_core.hpp and the culling part of dispatch.hpp compiled with plain g++ (no HIP) into
tests/cpp/simp_core_driver.cpp.  The whole-query loops over the statements the kernels share -- depth, ordered key, radix select,
redundancy test, node filter, edge weight, Prim step, verdict sequence -- must equal the restatement (tests/simp_numpy.py) on both
fixtures: integers and floats byte for byte, the angle within ANGLE_FLOOR, which this file measures and pins (the GPU tests allow ten
times that).  The limits and the carves are pinned."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import simp_numpy as M

ROOT = Path(__file__).resolve().parent.parent
MAP_FILES = ("kf_bad", "kf_pose", "feat_start", "feat_point", "feat_depth", "feat_octave", "obs_start", "obs", "pt_flags", "pt_pos")
GRAPH_FILES = ("kf_bad", "kf_pose", "kf_cull_factor", "kf_median_depth", "kf_prev", "kf_next", "kf_time", "conn_start", "conn_list")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("simp_core") / "simp_core_driver"
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", f"-I{ROOT / 'include'}", f"-I{ROOT / 'snake_slam_amd' / 'csrc'}",
           str(ROOT / "tests" / "cpp" / "simp_core_driver.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def fixtures():
    return M.require_coverage()


def run(driver, mode, d):
    p = subprocess.run([str(driver), mode, str(d)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr


def same_stats(got, want):
    """Byte for byte, except that a NaN redundancy equals a NaN redundancy (the sign of 0 / 0 is the platform's)."""
    for k in M.STATS_DTYPE.names:
        a, b = got[k], want[k]
        if k == "redundancy":
            nan = np.isnan(a) & np.isnan(b)
            a, b = np.where(nan, 0, a), np.where(nan, 0, b)
        assert a.tobytes() == b.tobytes(), (k, np.flatnonzero(a != b)[:5])


def test_stats_loops_equal_the_restatement(driver, fixtures, tmp_path):
    (t, queries, _), _, rows, _ = fixtures
    for name in MAP_FILES:
        t[name].tofile(tmp_path / f"{name}.bin")
    np.array(queries, np.int32).tofile(tmp_path / "q.bin")
    np.array([M.TH_DEPTH], np.float32).tofile(tmp_path / "th_depth.bin")
    for stereo in (0, 1):
        for cap in (256, 300):
            np.array([len(t["kf_bad"]), len(t["pt_flags"]), len(t["obs"]), len(t["feat_point"]), len(queries), 3, stereo, cap], np.int32).tofile(
                tmp_path / "meta.bin")
            run(driver, "stats", tmp_path)
            got = np.fromfile(tmp_path / "stats.bin", M.STATS_DTYPE)
            same_stats(got, M.stats_array([rows[(stereo, cap, q)] for q in queries]))


def test_select_finds_the_element_a_sort_by_the_bit_patterns_finds(driver, tmp_path):
    """Signed zeros, ties, negatives, subnormals and the extremes, 1 to 9 values: simp_key / simp_select against a sort by the bit patterns
    (and against np.sort where no zero of either sign is the median)."""
    rng = np.random.RandomState(4)
    pool = np.array([0.0, -0.0, 2.5, 2.5, -1.0, -0.0, 0.0, -3.0, 1e-45, -1e-45, 3.4e38, -3.4e38, 1.0, 1.0, 1.0], np.float32)
    for n in list(range(1, 10)) + [64, 257]:
        for _ in range(6):
            z = rng.choice(pool, n) if n < 10 else rng.choice(np.concatenate([pool, rng.randn(40).astype(np.float32)]), n)
            z.astype(np.float32).tofile(tmp_path / "z.bin")
            np.array([n], np.int32).tofile(tmp_path / "meta.bin")
            run(driver, "select", tmp_path)
            got = np.fromfile(tmp_path / "median.bin", np.float32)[0]
            want = sorted(z.tolist(), key=M.bits)[(n - 1) // 2]
            assert np.float32(got).tobytes() == np.float32(want).tobytes(), (z, got, want)
            assert got == np.sort(z)[(n - 1) // 2]


def write_graph(g, queries, st, params, times, node_cap, d):
    for name in GRAPH_FILES:
        g[name].tofile(d / f"{name}.bin")
    np.array(queries, np.int32).tofile(d / "q.bin")
    st.tofile(d / "stats.bin")
    M.params_record(params).tofile(d / "params.bin")
    np.array([len(g["kf_bad"]), len(g["conn_list"]), len(queries), node_cap, int(times)], np.int32).tofile(d / "meta.bin")


def test_decide_loops_equal_the_restatement(driver, fixtures, tmp_path):
    _, (g, queries, st, names), _, results = fixtures
    for pname, params, times in M.PARAM_SETS:
        write_graph(g, queries, st, params, times, M.MAX_NODES, tmp_path)
        run(driver, "decide", tmp_path)
        got = np.fromfile(tmp_path / "verdict.bin", M.VERDICT_DTYPE)
        want = M.verdict_array(results[pname])
        for k in M.VERDICT_DTYPE.names:
            if k == "value":
                continue
            assert got[k].tobytes() == want[k].tobytes(), (pname, k, [names[i] for i in np.flatnonzero(got[k] != want[k])[:5]])
        is_angle = want["reason"] == M.ANGLE
        assert got["value"][~is_angle].tobytes() == want["value"][~is_angle].tobytes(), pname
        assert is_angle.any() or pname != "no imu"
        assert np.abs(got["value"][is_angle] - want["value"][is_angle]).max(initial=0.0) <= M.ANGLE_FLOOR


def test_a_smaller_node_cap_overflows_earlier(driver, fixtures, tmp_path):
    _, (g, queries, st, names), _, _ = fixtures
    write_graph(g, queries, st, {}, True, 64, tmp_path)
    run(driver, "decide", tmp_path)
    got = np.fromfile(tmp_path / "verdict.bin", M.VERDICT_DTYPE)
    want = M.verdict_array([M.decide(g, q, st[i], {}, 64) for i, q in enumerate(queries)])
    assert got["status"].tobytes() == want["status"].tobytes() and got["reason"].tobytes() == want["reason"].tobytes()
    assert got["status"][names.index("64 nodes")] == M.OK and got["status"][names.index("65 nodes")] == M.NODES_OVERFLOW


def test_angle_floor_is_what_the_restatement_states(driver, fixtures, tmp_path):
    """The floor of the GPU tolerance: the g++ build's angle against the restatement's over every pair of the fixture for which an angle is
    computed, plus the same keyframes paired at random.  Printed; ANGLE_FLOOR must cover it and is not kept more than a quarter above it."""
    _, (g, queries, st, names), _, results = fixtures
    pairs = sorted({(q, r["other"]) for rows in results.values() for q, r in zip(queries, rows) if "angle" in r})
    rng = np.random.RandomState(2)
    live = np.flatnonzero(g["kf_median_depth"] > 0)
    pairs += [tuple(int(x) for x in rng.choice(live, 2, replace=False)) for _ in range(2000)]
    g["kf_pose"].tofile(tmp_path / "kf_pose.bin")
    g["kf_median_depth"].tofile(tmp_path / "kf_median_depth.bin")
    np.array(pairs, np.int32).tofile(tmp_path / "pairs.bin")
    np.array([len(g["kf_bad"]), len(pairs)], np.int32).tofile(tmp_path / "meta.bin")
    run(driver, "angles", tmp_path)
    got = np.fromfile(tmp_path / "angles.bin", np.float64)
    import math

    want = np.array([math.degrees(math.atan2(0.5 * float(np.linalg.norm(M.camera_position(g["kf_pose"][a]) - M.camera_position(g["kf_pose"][b]))),
                                             (float(g["kf_median_depth"][a]) + float(g["kf_median_depth"][b])) * 0.5) * 2.0) for a, b in pairs])
    floor = float(np.abs(got - want).max())
    print(f"angle floor: {floor:.3e} degrees over {len(pairs)} pairs (ANGLE_FLOOR {M.ANGLE_FLOOR:.3e})")
    assert floor <= M.ANGLE_FLOOR <= 1.25 * floor


def test_limits_and_carves_are_pinned(driver):
    line = subprocess.run([str(driver), "--consts"], capture_output=True, text=True, check=True).stdout.split()
    k = dict(zip(line[::2], map(int, line[1::2])))
    assert k["threads"] == 256 and k["max_nodes"] == M.MAX_NODES == 256 and k["max_feat"] == M.MAX_FEAT == 16384
    assert (k["long_min"], k["long_min_env0"], k["long_min_env7"]) == (32, 0, 7)
    # a key per feature, the queue (a feature per lane), 32 words
    assert k["stats_carve_max"] == 16384 * 4 + 256 * 4 + 32 * 4 and k["stats_carve_1"] == 4 * 4 + 256 * 4 + 32 * 4
    assert k["stats_carve_4096"] == 4096 * 4 + 256 * 4 + 32 * 4
    # the strict upper triangle, a sorted key and a keyframe per node, 32 words
    assert k["decide_carve_max"] == 32640 * 4 + 256 * 8 + 256 * 4 + 32 * 4 <= 160 * 1024
    assert k["decide_carve_1"] == 0 + 8 + 8 + 128 and k["decide_carve_16"] == 120 * 4 + 16 * 8 + 16 * 4 + 128
    assert k["decide_carve_64"] == 2016 * 4 + 64 * 8 + 64 * 4 + 128
