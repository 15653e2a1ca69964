"""GPU: snk_simp_stats / snk_simp_decide and their _batch_dev forms ("snk-simp v1") against the restatement of
tests/simp_numpy.py -- every byte of every record except the angle of an ANGLE verdict, which is within ten times the floor that
test_simp_core_cpu.py measures (no verdict of the fixture hinges on it: test_simp_numpy.py), and the sign of a NaN redundancy.

The shapes are simp_numpy.stats_fixture (keyframes of 0 / 1 / 2 / 3 / 256 / 257 features, feat_cap met and exceeded by one, lists of
3 / 4 / 32 / 33 / 300 observations around the walk threshold of 3 and the long-list threshold of 32, octaves at +1 and +2, the query
twice in a list, a depth equal to th_depth, stereo on and off, a bad query, no point that counts) and simp_numpy.decide_fixture (1, 2, 64,
65, 256 and 257 nodes, weights at and below min_matches_in_graph, one-sided and two-weight edges, equal weights, a disconnected second
graph, the thresholds met exactly, both IMU gates with and without the time tables); the device forms' BAD_INDEX answers and the host
forms' argument errors; the long-list threshold is forced both ways in child processes under SNK_DEBUG_POISON=1."""
import ctypes as C
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import simp_numpy as M

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GUARD = 64  # int32 words behind an output that must keep their fill
MAP_KEYS = ("kf_bad", "kf_pose", "feat_start", "feat_point", "feat_depth", "feat_octave", "obs_start", "obs", "pt_flags", "pt_pos")
GRAPH_KEYS = ("kf_bad", "kf_pose", "kf_cull_factor", "kf_median_depth", "kf_prev", "kf_next", "kf_time", "conn_start", "conn_list")


@functools.lru_cache(maxsize=None)
def fixtures():
    return M.require_coverage()


def culler(**kw):
    from snake_slam_amd.simp import KeyframeCuller

    return KeyframeCuller(dict(th_depth=M.TH_DEPTH, **kw))


def to_dev(a):
    import torch

    if a.dtype.fields:  # records travel as int32 words
        a = np.ascontiguousarray(a).view(np.int32).reshape(len(a), -1)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_out(n, words):
    import torch

    return torch.full((n * words + GUARD,), -7, dtype=torch.int32, device="cuda")


def read_out(out, n, words, dtype):
    o = out.cpu().numpy()
    assert np.all(o[n * words:] == -7), "wrote behind the output"
    return o[:n * words].copy().view(dtype).reshape(n)


def dev_stats(c, t, q):
    import torch

    d = {k: to_dev(t[k]) for k in MAP_KEYS}
    qd, out = to_dev(np.asarray(q, np.int32)), dev_out(len(q), 7)
    torch.cuda.synchronize()
    c.stats_dev(d, qd, out)
    c.sync()
    return read_out(out, len(q), 7, M.STATS_DTYPE)


def dev_decide(c, g, q, st):
    import torch

    d = {k: (to_dev(g[k]) if g.get(k) is not None else None) for k in GRAPH_KEYS}
    qd, sd, out = to_dev(np.asarray(q, np.int32)), to_dev(st), dev_out(len(q), 8)
    torch.cuda.synchronize()
    c.decide_dev(d, qd, sd, out)
    c.sync()
    return read_out(out, len(q), 8, M.VERDICT_DTYPE)


def check_stats(got, want, what=""):
    for k in M.STATS_DTYPE.names:
        a, b = got[k], want[k]
        if k == "redundancy":  # 0 / 0: NaN on both sides, the sign is the platform's
            nan = np.isnan(a) & np.isnan(b)
            a, b = np.where(nan, 0, a), np.where(nan, 0, b)
        assert a.tobytes() == b.tobytes(), (what, k, np.flatnonzero(a != b)[:5], a[a != b][:5], b[a != b][:5])


def check_verdicts(got, want, what=""):
    for k in M.VERDICT_DTYPE.names:
        if k != "value":
            assert got[k].tobytes() == want[k].tobytes(), (what, k, np.flatnonzero(got[k] != want[k])[:5], got[k][got[k] != want[k]][:5])
    is_angle = want["reason"] == M.ANGLE
    assert got["value"][~is_angle].tobytes() == want["value"][~is_angle].tobytes(), what
    diff = np.abs(got["value"][is_angle] - want["value"][is_angle])
    print(f"{what}: angle differences {diff}")
    assert np.all(diff <= M.ANGLE_BOUND), (what, diff)


@pytest.mark.parametrize("stereo,feat_cap", [(0, 256), (1, 256), (0, 300), (1, 300)])
def test_stats_host_and_device_forms_equal_the_restatement(stereo, feat_cap):
    (t, queries, names), _, rows, _ = fixtures()
    want = M.stats_array([rows[(stereo, feat_cap, q)] for q in queries])
    c = culler(stereo=stereo, feat_cap=feat_cap)
    try:
        runs = [(c.stats(t, queries), dev_stats(c, t, queries)) for _ in range(2)]
    finally:
        c.close()
    for host, dev in runs:
        check_stats(host, want, "host")
        check_stats(dev, want, "device")
    k257 = queries.index([k for k, v in names.items() if v == "257 features"][0])
    assert want["status"][k257] == (M.FEAT_OVERFLOW if feat_cap == 256 else M.OK)


def test_stats_min_obs_is_match_counts_argument():
    (t, queries, _), _, _, _ = fixtures()
    c = culler(stereo=1, feat_cap=300)
    try:
        for min_obs in (0, 1, 4, 33):
            want = M.stats_array([M.stats(t, q, min_obs, 1, M.TH_DEPTH, 300) for q in queries])
            check_stats(c.stats(t, queries, min_obs), want, f"min_obs {min_obs}")
    finally:
        c.close()


@pytest.mark.parametrize("pname", [p[0] for p in M.PARAM_SETS])
def test_decide_host_and_device_forms_equal_the_restatement(pname):
    _, (g, queries, st, names), _, results = fixtures()
    _, params, times = [p for p in M.PARAM_SETS if p[0] == pname][0]
    gg = g if times else M.without_times(g)
    want = M.verdict_array(results[pname])
    c = culler(**params)
    try:
        runs = [(c.decide(gg, queries, st), dev_decide(c, gg, queries, st)) for _ in range(2)]
    finally:
        c.close()
    for host, dev in runs:
        check_verdicts(host, want, "host")
        check_verdicts(dev, want, "device")


def test_decide_with_a_small_node_cap_and_other_thresholds():
    """node_cap 64: the 64-node graph fits, the 65-node one overflows; the carve is a sixteenth.  Other settings move every border."""
    _, (g, queries, st, names), _, _ = fixtures()
    for params, cap in (({}, 64), (dict(min_matches_in_graph=31, border_angle=30.0, border_redundancy=0.05, border_matches=300, th_map=29), 256),
                        (dict(min_matches_in_graph=-5, th_map=1000), 256)):
        want = M.verdict_array([M.decide(g, q, st[i], params, cap) for i, q in enumerate(queries)])
        c = culler(node_cap=cap, **params)
        try:
            check_verdicts(c.decide(g, queries, st), want, f"host {params} {cap}")
            check_verdicts(dev_decide(c, g, queries, st), want, f"device {params} {cap}")
        finally:
            c.close()
        if cap == 64:
            assert want["status"][names.index("64 nodes")] == M.OK and want["status"][names.index("65 nodes")] == M.NODES_OVERFLOW


def bad_row(dtype):
    r = np.zeros(1, dtype)
    r["status"] = M.BAD_INDEX
    if "median_depth" in dtype.names:
        r["median_depth"] = -1
    return r[0]


def test_stats_device_form_answers_bad_index_per_query():
    """Each kind of bad index in turn on copies of the fixture, placed where only the keyframe "the lists" reaches it: that query has
    status BAD_INDEX and nothing else, its neighbours equal the restatement; a bad entry in a list that is not walked is not seen."""
    (base, queries, names), _, rows, _ = fixtures()
    qk = [k for k, v in names.items() if v == "the lists"][0]
    assert qk == len(base["kf_bad"]) - 1
    n_kf, n_pts, n_obs, n_feat = len(base["kf_bad"]), len(base["pt_flags"]), len(base["obs"]), len(base["feat_point"])
    first = int(base["feat_start"][qk])
    point = lambda name: int(base["feat_point"][first + base["list_cases"].index(name)])  # noqa: E731
    p4, p33, p300, p3 = point("length 4, three qualify"), point("length 33"), point("length 300"), point("length 3")
    entry = lambda p, kf_is_q: int([o for o in range(base["obs_start"][p], base["obs_start"][p + 1]) if (base["obs"][o][0] == qk) == kf_is_q][0])  # noqa: E731

    def edit(key, index, value):
        m = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        m[key][index] = value
        return m

    q = np.array(queries, np.int32)
    at = queries.index(qk)
    want_ok = M.stats_array([rows[(1, 300, k)] for k in queries])
    want_bad = want_ok.copy()
    want_bad[at] = bad_row(M.STATS_DTYPE)
    q_out = q.copy()
    q_out[0], q_out[2] = n_kf, -1
    want_q = want_ok.copy()
    want_q[0] = want_q[2] = bad_row(M.STATS_DTYPE)
    cases = [("query", base, q_out, want_q),
             ("feat_start past the array", edit("feat_start", n_kf, n_feat + 5), q, want_bad),
             ("feat_start decreasing", edit("feat_start", n_kf, first - 1), q, want_bad),
             ("point id == n_points", edit("feat_point", first, n_pts), q, want_bad),
             ("point id -2", edit("feat_point", first + 1, -2), q, want_bad),
             ("obs_start decreasing", edit("obs_start", p4 + 1, base["obs_start"][p4] - 1), q, want_bad),
             ("obs_start past the array", edit("obs_start", p300 + 1, n_obs + 3), q, want_bad),
             ("observation keyframe == n_kf, a lane's walk", edit("obs", (entry(p4, False), 0), n_kf), q, want_bad),
             ("observation keyframe -1, a wavefront's walk", edit("obs", (entry(p300, False), 0), -1), q, want_bad),
             ("the query's own entry out of range", edit("obs", (entry(p33, True), 1), 1 << 20), q, want_bad),
             ("feature index == the keyframe's count", edit("obs", (entry(p33, False), 1), 8), q, want_bad),
             ("feature index -1", edit("obs", (entry(p4, False), 1), -1), q, want_bad),
             ("a list that is not walked is not checked", edit("obs", (entry(p3, False), 0), n_kf), q, want_ok)]
    c = culler(stereo=1, feat_cap=300)
    try:
        for name, m, qq, want in cases:
            check_stats(dev_stats(c, m, qq), want, name)
    finally:
        c.close()


def test_decide_device_form_answers_bad_index_per_query():
    _, (base, queries, st, names), _, results = fixtures()
    at = names.index("chain: one root edge of three nodes")
    qk = queries[at]
    n_kf, n_list = len(base["kf_bad"]), len(base["conn_list"])
    cs = base["conn_start"]

    def edit(key, index, value, field=None):
        m = {k: v.copy() for k, v in base.items()}
        if field:
            m[key][field][index] = value
        else:
            m[key][index] = value
        return m

    imu = dict(with_imu=1, gyro_weight=1.0, acc_weight=2.0)
    q = np.array(queries, np.int32)
    q_out = q.copy()
    q_out[1], q_out[3] = n_kf, -1
    for params, pname in (({}, "no imu"), (imu, "imu")):
        want_ok = M.verdict_array(results[pname])
        want_bad = want_ok.copy()
        want_bad[at] = bad_row(M.VERDICT_DTYPE)
        want_q = want_ok.copy()
        want_q[1] = want_q[3] = bad_row(M.VERDICT_DTYPE)
        reads_times = pname == "imu"
        cases = [("query", base, q_out, want_q),
                 ("conn_start decreasing", edit("conn_start", qk + 1, cs[qk] - 1), q, want_bad),
                 ("a node's conn_start past the array", edit("conn_start", qk + 2, n_list + 4), q, want_bad),
                 ("a connection of q == n_kf", edit("conn_list", int(cs[qk]), n_kf, "kf"), q, want_bad),
                 ("a connection of a node -1", edit("conn_list", int(cs[qk + 2]), -1, "kf"), q, want_bad),
                 ("kf_prev == n_kf", edit("kf_prev", qk, n_kf), q, want_bad if reads_times else want_ok),
                 ("kf_next -2", edit("kf_next", qk, -2), q, want_bad if reads_times else want_ok)]
        c = culler(**params)
        try:
            for name, m, qq, want in cases:
                check_verdicts(dev_decide(c, m, qq, st), want, f"{pname}: {name}")
        finally:
            c.close()


CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import simp_numpy as M
from snake_slam_amd.simp import KeyframeCuller
t, queries, _ = M.stats_fixture()
g, gq, st, _ = M.decide_fixture()
out = b""
for stereo in (0, 1):
    c = KeyframeCuller(dict(th_depth=M.TH_DEPTH, stereo=stereo, feat_cap=300))
    out += c.stats(t, queries).tobytes()
    c.close()
c = KeyframeCuller()
out += c.decide(g, gq, st).tobytes()
c.close()
open(sys.argv[2], "wb").write(out)
"""


@pytest.mark.parametrize("long_min", [None, 0, 1000000])
def test_long_list_threshold_forced_both_ways_on_poisoned_scratch(tmp_path, long_min):
    """SNK_SIMP_LONG_MIN is read once: a fresh child process per value.  Unset: lists above 32; 0: a wavefront walks every list longer than
    3; 1 000 000: a lane walks every list alone, the 300-entry ones included.  SNK_DEBUG_POISON=1 fills the staging buffers with 0xCD: every byte that comes
    back was written by a kernel.  The results do not depend on either."""
    (t, queries, _), (g, gq, st, _), rows, results = fixtures()
    out = tmp_path / "res.bin"
    env = dict(os.environ, SNK_DEBUG_POISON="1", PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("SNK_SIMP_LONG_MIN", None)
    if long_min is not None:
        env["SNK_SIMP_LONG_MIN"] = str(long_min)
    r = subprocess.run([sys.executable, "-c", CHILD, str(ROOT / "tests"), str(out)], capture_output=True, text=True, env=env, cwd=str(ROOT), timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    raw, n = out.read_bytes(), len(queries) * M.STATS_DTYPE.itemsize
    for stereo in (0, 1):
        got = np.frombuffer(raw[stereo * n:(stereo + 1) * n], M.STATS_DTYPE)
        check_stats(got, M.stats_array([rows[(stereo, 300, q)] for q in queries]), f"stereo {stereo}")
    check_verdicts(np.frombuffer(raw[2 * n:], M.VERDICT_DTYPE), M.verdict_array(results["no imu"]), "decide")


def test_argument_errors_are_codes_with_a_message_and_nothing_is_written():
    from snake_slam_amd import _lib, simp as S

    lib = _lib.load()
    (t, queries, _), (g, gq, st, _), rows, results = fixtures()
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    q = np.array(queries, np.int32)
    gqa = np.array(gq, np.int32)
    c = culler(stereo=1, feat_cap=300)
    try:
        def stats_call(par=None, n_kf=None, n=None, **kw):
            m = {k: kw[k] if k in kw else t[k] for k in MAP_KEYS}
            keep = {k: (None if v is None else np.ascontiguousarray(v)) for k, v in m.items()}
            cm = S.SimpMap(len(t["kf_bad"]) if n_kf is None else n_kf, len(t["pt_flags"]), len(t["obs"]), len(t["feat_point"]), *(ptr(keep[k]) for k in MAP_KEYS))
            par = par or S.SimpStatsParams(3, 1, M.TH_DEPTH, 300)
            res = np.zeros(len(q), M.STATS_DTYPE)
            res["status"] = -9
            qq = kw.get("q", q)
            rc = lib.snk_simp_stats(c._h, C.byref(cm), C.byref(par), len(q) if n is None else n, ptr(qq), None if kw.get("out", 1) is None else ptr(res))
            assert np.all(res["status"] == -9) or rc == 0
            return rc, lib.snk_last_error()

        def decide_call(par=None, n_kf=None, n=None, node_cap=256, **kw):
            m = {k: kw[k] if k in kw else g[k] for k in GRAPH_KEYS}
            keep = {k: (None if v is None else np.ascontiguousarray(v)) for k, v in m.items()}
            cg = S.SimpGraph(len(g["kf_bad"]) if n_kf is None else n_kf, len(g["conn_list"]), *(ptr(keep[k]) for k in GRAPH_KEYS))
            par = par or c._params()
            res = np.zeros(len(gqa), M.VERDICT_DTYPE)
            res["status"] = -9
            qq, ss = kw.get("q", gqa), kw.get("stats", st)
            rc = lib.snk_simp_decide(c._h, C.byref(cg), C.byref(par), node_cap, len(gqa) if n is None else n, ptr(qq), ptr(ss),
                                     None if kw.get("out", 1) is None else ptr(res))
            assert np.all(res["status"] == -9) or rc == 0
            return rc, lib.snk_last_error()

        def bumped(src, key, i, v, field=None):
            a = src[key].copy()
            if field:
                a[field][i] = v
            else:
                a[i] = v
            return {key: a}

        n_kf, n_pts, n_obs, n_feat = len(t["kf_bad"]), len(t["pt_flags"]), len(t["obs"]), len(t["feat_point"])
        with_point = int(np.argmax(t["feat_point"] >= 0))
        for kw, text in ([(dict([(k, None)]), b"NULL") for k in MAP_KEYS] +
                         [(dict(q=None), b"NULL"), (dict(out=None), b"NULL"), (dict(n=-1), b"negative"), (dict(n_kf=32769), b"SNK_COVIS_MAX_KF"),
                          (dict(par=S.SimpStatsParams(3, 1, M.TH_DEPTH, 0)), b"feat_cap"), (dict(par=S.SimpStatsParams(3, 1, M.TH_DEPTH, 16385)), b"feat_cap"),
                          (bumped(t, "feat_start", 0, 1), b"feat_start[0]"), (bumped(t, "feat_start", 4, int(t["feat_start"][3]) - 1), b"non-decreasing"),
                          (bumped(t, "feat_start", n_kf, n_feat + 1), b"n_feat"), (bumped(t, "obs_start", 0, 1), b"obs_start[0]"),
                          (bumped(t, "obs_start", 7, int(t["obs_start"][6]) - 1), b"non-decreasing"), (bumped(t, "obs_start", n_pts, n_obs + 1), b"n_obs"),
                          (bumped(t, "feat_point", with_point, n_pts), b"point id"), (bumped(t, "feat_point", with_point, -2), b"point id"),
                          (bumped(t, "obs", (5, 0), n_kf), b"keyframe outside"), (bumped(t, "obs", (5, 0), -1), b"keyframe outside"),
                          (bumped(t, "obs", (5, 1), 1 << 20), b"feature index"), (bumped(t, "obs", (5, 1), -1), b"feature index"),
                          (dict(q=np.where(np.arange(len(q)) == 2, n_kf, q).astype(np.int32)), b"query"),
                          (dict(q=np.where(np.arange(len(q)) == 2, -1, q).astype(np.int32)), b"query")]):
            rc, msg = stats_call(**kw)
            assert rc == 1 and text in msg, (list(kw), rc, msg)
        gk, n_list = len(g["kf_bad"]), len(g["conn_list"])
        for kw, text in ([(dict([(k, None)]), b"NULL") for k in GRAPH_KEYS if k not in ("kf_prev", "kf_next", "kf_time")] +
                         [(dict(kf_prev=None), b"all NULL or all present"), (dict(kf_next=None, kf_time=None), b"all NULL or all present"),
                          (dict(q=None), b"NULL"), (dict(stats=None), b"NULL"), (dict(out=None), b"NULL"), (dict(n=-1), b"negative"),
                          (dict(n_kf=32769), b"SNK_COVIS_MAX_KF"), (dict(node_cap=0), b"node_cap"), (dict(node_cap=257), b"node_cap"),
                          (bumped(g, "conn_start", 0, 1), b"conn_start[0]"), (bumped(g, "conn_start", 9, int(g["conn_start"][8]) - 1), b"non-decreasing"),
                          (bumped(g, "conn_start", gk, n_list + 1), b"n_list"), (bumped(g, "conn_list", 3, gk, "kf"), b"connection outside"),
                          (bumped(g, "conn_list", 3, -1, "kf"), b"connection outside"), (bumped(g, "kf_prev", 5, gk), b"kf_prev or kf_next"),
                          (bumped(g, "kf_next", 5, -2), b"kf_prev or kf_next"),
                          (dict(q=np.where(np.arange(len(gqa)) == 2, gk, gqa).astype(np.int32)), b"query")]):
            rc, msg = decide_call(**kw)
            assert rc == 1 and text in msg, (list(kw), rc, msg)
        assert stats_call(n=0, q=None, out=None)[0] == 0 and decide_call(n=0, q=None, stats=None, out=None)[0] == 0  # n_q == 0 is valid
        assert decide_call(kf_prev=None, kf_next=None, kf_time=None)[0] == 0  # all three absent is valid
        # the handle is as good as before
        check_stats(c.stats(t, queries), M.stats_array([rows[(1, 300, k)] for k in queries]))
        check_verdicts(c.decide(g, gq, st), M.verdict_array(results["no imu"]))
    finally:
        c.close()
