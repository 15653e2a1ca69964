"""GPU: snk_triangulate_pairs / snk_triangulate_neighbours ("snk-tri v1") against the numpy restatement of tests/tri_numpy.py.

Decision, branch, far_away, neighbour, output order, out_start and commit must be identical for every pair whose margin (smallest
relative distance of an evaluated gate to its threshold) is >= 1e-6; pairs below are borderline -- a float rounding of a cosine may
flip them -- and are left out of the decision comparison (at most 1 % of a case; tests/test_tri_numpy.py proves the restatement stays
inside that on these seeds).  out_start and commit are checked with the GPU's own decision for the borderline pairs fed to the
restatement's counting and commit pass.  Positions agree within tri_numpy.position_tolerance(): 10 x the measured disagreement of two
float64 CPU solutions of the same definition, relative to max(1, |x|) -- 9.0e-11; observed on an MI355X: 1.3e-12 at most."""
import ctypes as C

import numpy as np
import pytest

import tri_numpy as T

pytestmark = pytest.mark.gpu


def make_triangulator(c):
    from snake_slam_amd.tracking import Triangulator

    p = c["params"]
    return Triangulator(c["cam"], c["level_scale"], p["error_mono"], p["error_stereo"], p["th_depth"], mono=bool(p["mono"]))


def restate(c):
    return T.triangulate_neighbours(c["cam"], c["params"], c["kf1"], c["kf2s"], c["median_depth2s"], c["pairs"], c["level_scale"])


def check_against_restatement(c, res, pts, out_start):
    """Returns (largest position difference, number of borderline pairs)."""
    n_nb = len(c["kf2s"])
    assert len(out_start) == n_nb + 1 and out_start[0] == 0 and out_start[-1] == len(pts) and np.all(np.diff(out_start) >= 0)
    worst, borderline, total = 0.0, 0, 0
    entries, want_start = [], [0]
    for k in range(n_nb):
        got = pts[out_start[k]:out_start[k + 1]]
        j = 0
        for (a, b), (br, X, far, mg) in zip(c["pairs"][k], res[k]):
            total += 1
            hit = j < len(got) and got["feature1"][j] == a and got["feature2"][j] == b
            if mg < T.BORDERLINE:
                borderline += 1
            else:
                assert bool(hit) == (br != T.REJECT), f"neighbour {k}, pair ({a}, {b}): GPU {'kept' if hit else 'dropped'}, restatement branch {br}, margin {mg:.2e}"
                if hit:
                    assert got["branch"][j] == br and bool(got["far_away"][j]) == far, (k, a, b, got[j], br, far)
                    d = float(np.max(np.abs(got["pos"][j] - X) / np.maximum(1.0, np.abs(X))))
                    worst = max(worst, d)
            if hit:
                assert got["neighbour"][j] == k
                entries.append((k, int(a), int(b)))
                j += 1
        assert j == len(got), f"neighbour {k}: {len(got) - j} points that are not the pairs' survivors in pair order"
        want_start.append(len(entries))
    assert list(out_start) == want_start
    want_commit = T.commit_pass(entries, c["kf1"]["has_mp"], [k2["has_mp"] for k2 in c["kf2s"]])
    assert np.array_equal(pts["commit"].astype(bool), np.array(want_commit, bool))
    assert borderline <= T.BORDERLINE_CAP * total
    return worst, borderline


@pytest.mark.parametrize("seed,n_nb,mode", T.CASES)
def test_neighbours_against_the_restatement(seed, n_nb, mode):
    c = T.make_case(seed, n_nb, mode)
    res = restate(c)
    tri = make_triangulator(c)
    try:
        nnew, pts, out_start = tri.Process(c["kf1"], c["kf2s"], c["pairs"], c["median_depth2s"])
        again = tri.Process(c["kf1"], c["kf2s"], c["pairs"], c["median_depth2s"])
    finally:
        tri.close()
    worst, borderline = check_against_restatement(c, res, pts, out_start)
    print(f"case {seed}/{n_nb}/{mode}: {len(pts)} points, {nnew} committed, {borderline} borderline pairs, "
          f"largest position difference {worst:.3e} (tolerance {T.position_tolerance():.3e})")
    assert nnew == int(pts["commit"].sum()) and 0 < nnew < len(pts)
    assert worst <= T.position_tolerance()
    assert again[0] == nnew and again[1].tobytes() == pts.tobytes() and np.array_equal(again[2], out_start)  # deterministic


@pytest.mark.parametrize("seed,n_nb,mode", [T.CASES[0], T.CASES[3], T.CASES[6]])
def test_batched_call_equals_the_single_pair_calls(seed, n_nb, mode):
    c = T.make_case(seed, n_nb, mode)
    tri = make_triangulator(c)
    try:
        _, pts, out_start = tri.Process(c["kf1"], c["kf2s"], c["pairs"], c["median_depth2s"])
        singles = [tri.triangulate(c["kf1"], k2, p, m) for k2, p, m in zip(c["kf2s"], c["pairs"], c["median_depth2s"])]
    finally:
        tri.close()
    assert [len(s) for s in singles] == list(np.diff(out_start)) and any(len(s) == 0 for s in singles) and any(len(s) > 100 for s in singles)
    entries = []
    for k, s in enumerate(singles):
        got = pts[out_start[k]:out_start[k + 1]]
        for f in ("feature1", "feature2", "far_away", "branch", "pos"):
            assert np.array_equal(s[f], got[f]), (k, f)
        assert np.all(s["neighbour"] == 0) and np.all(got["neighbour"] == k)
        own = [(0, int(a), int(b)) for a, b in zip(s["feature1"], s["feature2"])]
        assert np.array_equal(s["commit"].astype(bool), np.array(T.commit_pass(own, c["kf1"]["has_mp"], [c["kf2s"][k]["has_mp"]]), bool))
        entries += [(k, a, b) for _, a, b in own]
    want = T.commit_pass(entries, c["kf1"]["has_mp"], [k2["has_mp"] for k2 in c["kf2s"]])
    assert np.array_equal(pts["commit"].astype(bool), np.array(want, bool))


def test_commit_conflicts_inside_one_chunk_and_across_chunks():
    """Every pair is the same good correspondence repeated, interleaved with pairs that share only one of its features: the ordered
    pass must keep exactly the first use of every feature, inside a 64-candidate chunk and across chunks."""
    c = T.make_case(21, 5, "mixed")
    res = restate(c)
    good = [(int(a), int(b)) for (a, b), r in zip(c["pairs"][0], res[0])
            if r[0] and r[3] >= T.BORDERLINE and not c["kf1"]["has_mp"][a] and not c["kf2s"][0]["has_mp"][b]]
    assert len(good) > 40
    rng = np.random.default_rng(5)
    pairs = np.array([good[i] for i in rng.integers(0, 40, 700)], np.int32)  # 40 distinct pairs, 700 entries: ~17 repeats each
    c["kf2s"], c["pairs"], c["median_depth2s"] = c["kf2s"][:1], [pairs], c["median_depth2s"][:1]
    tri = make_triangulator(c)
    try:
        nnew, pts, out_start = tri.Process(c["kf1"], c["kf2s"], c["pairs"], c["median_depth2s"])
    finally:
        tri.close()
    assert len(pts) == 700 and np.array_equal(pts["feature1"], pairs[:, 0]) and np.array_equal(pts["feature2"], pairs[:, 1])
    want = T.commit_pass([(0, int(a), int(b)) for a, b in pairs], c["kf1"]["has_mp"], [c["kf2s"][0]["has_mp"]])
    assert np.array_equal(pts["commit"].astype(bool), np.array(want, bool)) and nnew == sum(want) <= 40


def test_empty_inputs_launch_nothing_and_are_valid():
    c = T.make_case(11, 5, "mixed")
    tri = make_triangulator(c)
    try:
        nnew, pts, out_start = tri.Process(c["kf1"], [], [])
        assert nnew == 0 and len(pts) == 0 and list(out_start) == [0]
        nnew, pts, out_start = tri.Process(c["kf1"], c["kf2s"][:3], [np.zeros((0, 2), np.int32)] * 3, c["median_depth2s"][:3])
        assert nnew == 0 and len(pts) == 0 and list(out_start) == [0, 0, 0, 0]
        assert len(tri.triangulate(c["kf1"], c["kf2s"][0], [])) == 0
        # one neighbour of three without pairs
        prs = [c["pairs"][0], np.zeros((0, 2), np.int32), c["pairs"][3]]
        _, pts, out_start = tri.Process(c["kf1"], [c["kf2s"][0], c["kf2s"][1], c["kf2s"][3]], prs, c["median_depth2s"][[0, 1, 3]])
        assert out_start[1] == out_start[2] and out_start[1] > 0 and out_start[3] > out_start[2] and set(pts["neighbour"]) == {0, 2}
    finally:
        tri.close()


def test_bad_arguments_are_error_codes_not_faults():
    from snake_slam_amd import SnakeHipError, _lib
    from snake_slam_amd.tracking import TriView, _tri_view

    c = T.make_case(11, 5, "mixed")
    kf1, kf2 = c["kf1"], c["kf2s"][0]
    n1, n2 = len(kf1["kps"]), len(kf2["kps"])
    tri = make_triangulator(c)
    try:
        for bad, text in (([(n1, 0)], "keyframe-1 feature index"), ([(-1, 0)], "keyframe-1 feature index"), ([(0, n2)], "keyframe-2 feature index"),
                          ([(0, -5)], "keyframe-2 feature index")):
            with pytest.raises(SnakeHipError, match=text):
                tri.triangulate(kf1, kf2, bad)
            with pytest.raises(SnakeHipError, match=text):
                tri.Process(kf1, [c["kf2s"][1], kf2], [c["pairs"][1], bad], c["median_depth2s"][:2])
        for which, octave in ((0, T.N_LEVELS), (1, -1)):
            k = [dict(kf1), dict(kf2)]
            k[which]["kps"] = k[which]["kps"].copy()
            k[which]["kps"]["octave"][3] = octave
            with pytest.raises(SnakeHipError, match="octave outside"):
                tri.triangulate(k[0], k[1], [(3, 3)])
            assert len(tri.triangulate(k[0], k[1], [(4, 4)])) <= 1  # a bad octave nobody refers to is not read
        # NULL arrays with a non-zero count
        lib = _lib.load()
        v1, keep1 = _tri_view(kf1)
        v2, keep2 = _tri_view(kf2)
        pairs = np.zeros((4, 2), np.int32)
        out = np.zeros(4, T.NEW_POINT)
        n = C.c_int(7)
        args = lambda a, b, p, o: (tri._h, C.byref(tri._cam), C.byref(tri._params), C.byref(a), C.byref(b), 0.0, p, 4, tri._ls.ctypes.data, len(tri._ls), o, C.byref(n))
        null_kps = TriView.from_buffer_copy(v2)
        null_kps.kps = 0
        assert lib.snk_triangulate_pairs(*args(v1, null_kps, pairs.ctypes.data, out.ctypes.data)) == 1 and b"NULL array" in lib.snk_last_error()
        assert n.value == 0
        assert lib.snk_triangulate_pairs(*args(v1, v2, None, out.ctypes.data)) == 1 and b"NULL pairs" in lib.snk_last_error()
        assert lib.snk_triangulate_pairs(*args(v1, v2, pairs.ctypes.data, None)) == 1
        big = TriView.from_buffer_copy(v2)
        big.n = 65537
        assert lib.snk_triangulate_pairs(*args(v1, big, pairs.ctypes.data, out.ctypes.data)) == 1 and b"65536" in lib.snk_last_error()
        # the handle is as good as before
        assert len(tri.triangulate(kf1, kf2, c["pairs"][0])) > 100
    finally:
        tri.close()
