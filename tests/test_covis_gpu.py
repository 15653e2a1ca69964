"""GPU: snk_covis_update / snk_covis_vote and their _batch_dev forms ("snk-covis v1") against the restatement of
tests/covis_numpy.py -- every byte of every list and result, (-1, -1) where nothing may be written: the results are integers, so there is
nothing to tolerate.

The shapes are covis_numpy.edge_case (thresholds 14 / 15 / 16, ties, bad keyframes, duplicates, lists of 63 / 64 / 65 / 300 / 4096
observations around the long-list threshold of 32, lists cut at cap - 1 / cap / cap + 1 / 3 cap), one structured map of 1 025 keyframes,
a vote batch of 70 frames, SNK_COVIS_MAX_KF keyframes with a list longer than SNK_COVIS_MAX_CAP, the device forms' BAD_INDEX answers
and the host forms' argument errors; the long-list threshold is forced both ways in child processes (the switch is read once)."""
import ctypes as C
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import covis_numpy as M

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GUARD = 64  # int32 words behind conn and out that must keep their fill


@functools.lru_cache(maxsize=None)
def edge(n_kf=1025):
    return M.edge_case(n_kf)


@functools.lru_cache(maxsize=None)
def edge_want(cap, n_kf=1025):
    c = edge(n_kf)
    return M.update(c, c["q"], cap=cap), M.vote(c, c["set_start"], c["set_point"], cap=cap)


def graph(cap, th=M.TH):
    from snake_slam_amd.covis import CovisibilityGraph

    return CovisibilityGraph(th, M.TH_DEPTH, cap)


def host_update(g, m, q):
    return g.update(*(m[k] for k in M.MAP_KEYS + M.FEAT_KEYS), q)


def host_vote(g, m, set_start, set_point):
    return g.vote(*(m[k] for k in M.MAP_KEYS), set_start, set_point)


def to_dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_outputs(n, cap):
    import torch

    return (torch.full((n * cap * 2 + GUARD,), -1, dtype=torch.int32, device="cuda"),
            torch.full((n * 4 + GUARD,), -7, dtype=torch.int32, device="cuda"))


def read_outputs(conn, out, n, cap):
    """(conn, res) as records; the guard words behind both must be untouched."""
    c, o = conn.cpu().numpy(), out.cpu().numpy()
    assert np.all(c[n * cap * 2:] == -1) and np.all(o[n * 4:] == -7), "wrote behind conn / out"
    return c[:n * cap * 2].copy().view(M.CONN).reshape(n, cap), o[:n * 4].copy().view(M.RESULT).reshape(n)


def dev_update(g, m, q):
    import torch

    conn, out = dev_outputs(len(q), g.cap)
    d = [to_dev(m[k]) for k in M.MAP_KEYS + M.FEAT_KEYS] + [to_dev(np.asarray(q, np.int32))]
    torch.cuda.synchronize()
    g.update_dev(*d, conn, out)
    g.sync()
    return read_outputs(conn, out, len(q), g.cap)


def dev_vote(g, m, set_start, set_point):
    import torch

    n = len(set_start) - 1
    conn, out = dev_outputs(n, g.cap)
    d = [to_dev(m[k]) for k in M.MAP_KEYS] + [to_dev(np.asarray(set_start, np.int32)), to_dev(np.asarray(set_point, np.int32))]
    torch.cuda.synchronize()
    g.vote_dev(*d, conn, out)
    g.sync()
    return read_outputs(conn, out, n, g.cap)


def differing(got, want):
    rows = [s for s in range(len(want[1])) if got[1][s].tobytes() != want[1][s].tobytes() or got[0][s].tobytes() != want[0][s].tobytes()]
    return [(s, got[1][s], want[1][s], got[0][s][:4], want[0][s][:4]) for s in rows[:3]]


def same(got, want):
    return got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


@pytest.mark.parametrize("cap", [4, 64, 256])
def test_host_and_device_forms_equal_the_restatement_on_the_edge_case(cap):
    """cap 4 and 64 cut the lists built for them at cap - 1 / cap / cap + 1 / 3 cap, with equal weights across the cut."""
    c = edge()
    want_u, want_v = edge_want(cap)
    g = graph(cap)
    try:
        runs = [(host_update(g, c, c["q"]), host_vote(g, c, c["set_start"], c["set_point"]),
                 dev_update(g, c, c["q"]), dev_vote(g, c, c["set_start"], c["set_point"])) for _ in range(2)]
    finally:
        g.close()
    for hu, hv, du, dv in runs:
        assert same(hu, want_u), differing(hu, want_u)
        assert same(du, want_u), differing(du, want_u)
        assert same(hv, want_v), differing(hv, want_v)
        assert same(dv, want_v), differing(dv, want_v)
    w = c["what"]
    assert want_u[1]["status"][w["untouched"]] == M.UNCHANGED and tuple(want_u[1][w["only_bad"]]) == (0, 0, -1, M.OK)
    assert want_u[1]["n_found"][w[f"trunc{min(cap, 64)}_3"]] == 3 * min(cap, 64)


@pytest.mark.parametrize("n_kf", [1, 2, 255, 256, 257])
def test_every_keyframe_count(n_kf):
    c = edge(n_kf)
    want_u, want_v = edge_want(64, n_kf)
    g = graph(64)
    try:
        du, dv = dev_update(g, c, c["q"]), dev_vote(g, c, c["set_start"], c["set_point"])
        hu, hv = host_update(g, c, c["q"]), host_vote(g, c, c["set_start"], c["set_point"])
    finally:
        g.close()
    assert same(du, want_u) and same(hu, want_u), differing(du, want_u)
    assert same(dv, want_v) and same(hv, want_v), differing(dv, want_v)


def test_structured_map_of_1025_keyframes_every_keyframe_a_query():
    m = M.make_map(31, 1025, 20000)
    q = np.arange(1025, dtype=np.int32)
    want = M.update(m, q, cap=16)  # most lists hold more than 16 entries: the cut runs for them
    g = graph(16)
    try:
        dev, host = dev_update(g, m, q), host_update(g, m, q)
    finally:
        g.close()
    assert same(dev, want), differing(dev, want)
    assert same(host, want), differing(host, want)
    assert np.median(want[1]["n_found"]) > 16 and np.all(want[1]["status"] == M.OK)


def test_vote_batch_of_70_frames_ragged_and_padded():
    m = M.make_map(32, 300, 6000)
    ss, sp = M.frames_of(m, 33, 70)
    cut = ss.copy()
    for f in (0, 13, 69):  # empty frames: the set ends where it starts
        cut[f + 1:] -= ss[f + 1] - ss[f]
    sp_cut = np.concatenate([sp[ss[f]:ss[f + 1]] for f in range(70) if f not in (0, 13, 69)])
    ps, padded = M.frames_of(m, 33, 70, cap=320)
    want, want_cut = M.vote(m, ss, sp, cap=16), M.vote(m, cut, sp_cut, cap=16)
    g = graph(16)
    try:
        ragged, holes, pad = dev_vote(g, m, ss, sp), dev_vote(g, m, cut, sp_cut), dev_vote(g, m, ps, padded)
        host = host_vote(g, m, ps, padded)
    finally:
        g.close()
    assert same(ragged, want), differing(ragged, want)
    assert same(pad, want) and same(host, want)  # the -1 padding is skipped: a [batch][cap] array is a valid input
    assert same(holes, want_cut) and np.all(want_cut[1]["status"][[0, 13, 69]] == M.UNCHANGED)
    assert np.all(want[1]["n_found"] > 0) and np.all(want[1]["n_found"] > 16)  # every list is cut


def test_device_forms_answer_bad_index_per_set():
    """Each kind of bad index in turn, on copies of one small map; the sets it does not reach equal the restatement, the ones it
    reaches have status BAD_INDEX, no list and nothing written; the guard words behind conn and out keep their fill."""
    base = M.make_map(41, 40, 800, window=120)
    q = np.arange(40, dtype=np.int32)
    n_kf, n_pts, n_obs, n_feat = 40, 800, len(base["obs"]), len(base["feat_point"])
    first_feature = lambda kf: int(base["feat_start"][kf] + np.argmax(base["feat_point"][base["feat_start"][kf]:base["feat_start"][kf + 1]] >= 0))  # noqa: E731

    def edit(key, index, value):
        m = {k: v.copy() for k, v in base.items()}
        m[key][index] = value
        return m

    some_point = int(base["feat_point"][first_feature(12)])
    cases = [("query", base, np.where(q == 3, n_kf, np.where(q == 5, -1, q)).astype(np.int32)),
             ("feat_start past the array", edit("feat_start", n_kf, n_feat + 5), q),
             ("feat_start decreasing", edit("feat_start", 8, base["feat_start"][7] - 1), q),
             ("point id == n_points", edit("feat_point", first_feature(9), n_pts), q),
             ("point id -2", edit("feat_point", first_feature(10), -2), q),
             ("obs_start decreasing", edit("obs_start", some_point + 1, base["obs_start"][some_point] - 1), q),
             ("obs_start past the array", edit("obs_start", some_point + 1, n_obs + 3), q),
             ("observation keyframe == n_kf", edit("obs", (int(base["obs_start"][some_point]), 0), n_kf), q),
             ("observation keyframe -1", edit("obs", (int(base["obs_start"][some_point]), 0), -1), q)]
    g = graph(8)
    try:
        for name, m, qq in cases:
            want = M.update_checked(m, qq, cap=8)
            n_bad = int(np.sum(want[1]["status"] == M.BAD_INDEX))
            assert 0 < n_bad < 40, (name, n_bad)
            got = dev_update(g, m, qq)
            assert same(got, want), (name, differing(got, want))
        ss, sp = M.frames_of(base, 42, 12, n_matched=60)
        vote_cases = [("set_start decreasing", base, np.where(np.arange(13) == 4, ss[3] - 1, ss), sp),
                      ("set_start past the array", base, np.where(np.arange(13) == 12, len(sp) + 1, ss), sp),
                      ("point id == n_points", base, ss, np.where(np.arange(len(sp)) == ss[6], n_pts, sp)),
                      ("observation keyframe == n_kf", edit("obs", (int(base["obs_start"][some_point]), 0), n_kf), ss,
                       np.where(np.arange(len(sp)) == ss[2], some_point, sp))]
        for name, m, s_start, s_point in vote_cases:
            s_start, s_point = s_start.astype(np.int32), s_point.astype(np.int32)
            want = M.vote_checked(m, s_start, s_point, cap=8)
            n_bad = int(np.sum(want[1]["status"] == M.BAD_INDEX))
            assert 0 < n_bad < 12, (name, n_bad)
            got = dev_vote(g, m, s_start, s_point)
            assert same(got, want), (name, differing(got, want))
    finally:
        g.close()


def test_max_kf_with_touched_ids_at_both_ends_and_a_list_longer_than_max_cap():
    """SNK_COVIS_MAX_KF keyframes and SNK_COVIS_MAX_CAP entries: the largest carve.  5 000 points seen by every sixth keyframe and
    twenty seen by keyframes 0 and 32767: 5 001 touched keyframes, cut to the last 4 096; th = 1 lists them all in the connection form."""
    b = M.Builder(M.MAX_KF)
    me = 3
    for j in range(5000):
        b.see(me, [(j * 6) % M.MAX_KF], 1 + (j % 3))
    b.see(me, [0, M.MAX_KF - 1], 20)
    b.kf_bad[12] = 1
    m = b.tables()
    pts = m["feat_point"][m["feat_start"][me]:m["feat_start"][me + 1]]
    ss, sp = M.sets_of([pts.tolist()])
    q = np.array([me, 0], np.int32)
    want_u, want_v = M.update(m, q, th=1, cap=M.MAX_CAP), M.vote(m, ss, sp, cap=M.MAX_CAP)
    assert want_v[1]["n_found"][0] == 5001 and want_u[1]["n_found"][0] == 5000 and want_u[1]["status"][1] == M.UNCHANGED
    assert want_v[0][0][-2:].tolist() == [(20, M.MAX_KF - 1), (21, 0)] and want_v[1]["best_kf"][0] == 0
    g = graph(M.MAX_CAP, th=1)
    try:
        du, dv = dev_update(g, m, q), dev_vote(g, m, ss, sp)
        hu = host_update(g, m, q)
    finally:
        g.close()
    assert same(du, want_u) and same(hu, want_u), differing(du, want_u)
    assert same(dv, want_v), differing(dv, want_v)


CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import covis_numpy as M
from snake_slam_amd.covis import CovisibilityGraph
c = M.edge_case()
g = CovisibilityGraph(M.TH, M.TH_DEPTH, 64)
u = g.update(*(c[k] for k in M.MAP_KEYS + M.FEAT_KEYS), c["q"])
v = g.vote(*(c[k] for k in M.MAP_KEYS), c["set_start"], c["set_point"])
g.close()
open(sys.argv[2], "wb").write(u[0].tobytes() + u[1].tobytes() + v[0].tobytes() + v[1].tobytes())
"""


@pytest.mark.parametrize("long_min", [0, 1, 1000000])
def test_long_list_threshold_forced_both_ways(tmp_path, long_min):
    """SNK_COVIS_LONG_MIN is read once: a fresh child process per value.  0: a wavefront walks every list, one observation included;
    1 000 000: a lane walks every list alone, the 4096-entry one included.  The results do not depend on it."""
    out = tmp_path / "res.bin"
    env = dict(os.environ, SNK_COVIS_LONG_MIN=str(long_min), PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", CHILD, str(ROOT / "tests"), str(out)], capture_output=True, text=True, env=env, cwd=str(ROOT), timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    want_u, want_v = edge_want(64)
    assert out.read_bytes() == want_u[0].tobytes() + want_u[1].tobytes() + want_v[0].tobytes() + want_v[1].tobytes()


def test_argument_errors_are_codes_with_a_message_and_nothing_is_written():
    from snake_slam_amd import _lib
    from snake_slam_amd.covis import CovisMap, CovisParams

    lib = _lib.load()
    base = M.make_map(51, 12, 200, window=60)
    q = np.arange(12, dtype=np.int32)
    ss, sp = M.frames_of(base, 52, 3, n_matched=20)
    g = graph(8)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    try:
        def call(vote=False, par=None, n_kf=None, n=None, **kw):
            m = {k: (np.ascontiguousarray(kw[k]) if kw[k] is not None else None) if k in kw else base[k] for k in M.MAP_KEYS + M.FEAT_KEYS}
            qq, s_start, s_point = kw.get("q", q), kw.get("set_start", ss), kw.get("set_point", sp)
            cm = CovisMap(len(base["kf_bad"]) if n_kf is None else n_kf, len(base["pt_flags"]), len(base["obs"]), *(ptr(m[k]) for k in M.MAP_KEYS))
            par = par or CovisParams(M.TH, M.TH_DEPTH, 8)
            conn, res = M.empty_outputs(12, 8)
            res["status"] = -9
            out = None if kw.get("out", 1) is None else res.ctypes.data
            if vote:
                rc = lib.snk_covis_vote(g._h, C.byref(cm), 3 if n is None else n, ptr(s_start), ptr(s_point), C.byref(par), conn.ctypes.data, out)
            else:
                rc = lib.snk_covis_update(g._h, C.byref(cm), *(ptr(m[k]) for k in M.FEAT_KEYS), C.byref(par), 12 if n is None else n, ptr(qq),
                                          conn.ctypes.data, out)
            assert np.all(conn["kf"] == -1) and np.all(res["status"] == -9) or rc == 0
            return rc, lib.snk_last_error()

        i32 = lambda *a: np.array(a, np.int32)  # noqa: E731
        bumped = lambda key, i, v: {key: np.concatenate([base[key][:i], [v], base[key][i + 1:]]).astype(base[key].dtype)}  # noqa: E731
        obs_bad = base["obs"].copy()
        obs_bad[5, 0] = 12
        for kw, text in ((dict(par=CovisParams(0, M.TH_DEPTH, 8)), b"th < 1"), (dict(par=CovisParams(M.TH, M.TH_DEPTH, 0)), b"cap"),
                         (dict(par=CovisParams(M.TH, M.TH_DEPTH, M.MAX_CAP + 1)), b"cap"), (dict(n_kf=M.MAX_KF + 1), b"SNK_COVIS_MAX_KF"),
                         (dict(kf_bad=None), b"NULL"), (dict(obs_start=None), b"NULL"), (dict(obs=None), b"NULL"), (dict(pt_flags=None), b"NULL"),
                         (dict(feat_start=None), b"NULL"), (dict(feat_point=None), b"NULL"), (dict(feat_depth=None), b"NULL"), (dict(q=None), b"NULL"),
                         (dict(out=None), b"NULL"), (dict(n=-1), b"negative"), (bumped("obs_start", 0, 1), b"obs_start[0]"),
                         (bumped("obs_start", 7, int(base["obs_start"][6]) - 1), b"non-decreasing"), (bumped("obs_start", 200, len(base["obs"]) + 1), b"n_obs"),
                         (bumped("feat_start", 0, 1), b"begin at 0"), (bumped("feat_start", 4, int(base["feat_start"][3]) - 1), b"non-decreasing"),
                         (bumped("feat_point", 3, 200), b"point id"), (bumped("feat_point", 3, -2), b"point id"), (dict(obs=obs_bad), b"keyframe outside"),
                         (dict(q=i32(0, 1, 12, *range(3, 12))), b"query"), (dict(q=i32(0, 1, -1, *range(3, 12))), b"query")):
            rc, msg = call(**kw)
            assert rc == 1 and text in msg, (kw.keys(), rc, msg)
        for kw, text in ((dict(par=CovisParams(M.TH, M.TH_DEPTH, 0)), b"cap"), (dict(par=CovisParams(0, M.TH_DEPTH, 8)), b"th < 1"), (dict(set_start=None), b"NULL"), (dict(set_point=None), b"NULL"),
                         (dict(set_start=i32(0, 5, 4, 9)), b"non-decreasing"), (dict(set_start=i32(1, 5, 7, 9)), b"begin at 0"),
                         (dict(set_point=np.where(np.arange(len(sp)) == 2, 200, sp).astype(np.int32)), b"point id"), (dict(obs=obs_bad), b"keyframe outside")):
            rc, msg = call(vote=True, **kw)
            assert rc == 1 and text in msg, (kw.keys(), rc, msg)
        assert call(n=0, q=None)[0] == 0 and call(vote=True, n=0, set_start=None, set_point=None)[0] == 0  # n_q == 0 is valid
        # the handle is as good as before
        assert same(host_update(g, base, q), M.update(base, q, cap=8))
    finally:
        g.close()
