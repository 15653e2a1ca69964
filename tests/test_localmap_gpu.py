"""GPU: snk_lmap_select / snk_lmap_gather and their _batch_dev forms ("snk-lmap v1") against the restatement of
tests/localmap_numpy.py -- every list, every result word, every byte of every snk_lm_fine record, the -1 fill and 64 guard words behind
each output array: the results are integers and copied bytes, so there is nothing to tolerate.

The shapes are localmap_numpy.select_case (votes of 0 / 1 / 14 / 15 / 16 / 20 / 21 / 80 / 272 entries, one cut by its cap, twins under two
frame ids, connection lists of 0 / 3 / 5 / 9 entries, bad and repeated neighbours, kf_cap around n_local, three seeds) and gather_case
(candidate totals at the scan-chunk edges, duplicates, skips, own points of every kind, pts_cap 64 and SNK_LMAP_MAX_PTS met from both
sides, 40 ids on one slot, a probe chain that wraps, stage-1 statuses passed through) and long_range_case (a keyframe of 65 540
features between ordinary ones); then the device forms' BAD_INDEX answers, the host
forms' argument errors, a large call followed by a small one on one handle and the edge case in a child under SNK_DEBUG_POISON=1."""
import ctypes as C
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import localmap_numpy as M

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GUARD = 64  # int32 words behind every output array that must keep their fill
FILL = 0xA5  # the byte of records that nothing may write


@functools.lru_cache(maxsize=None)
def select_case(seed):
    return M.select_case(seed)


@functools.lru_cache(maxsize=None)
def gather_case(pts_cap):
    return M.gather_case(pts_cap)


@functools.lru_cache(maxsize=None)
def gather_want(pts_cap, fill):
    c = gather_case(pts_cap)
    return M.gather(c["m"], c["frame_id"], c["local_kf"], c["sel"], c["set_start"], c["set_point"], pts_cap, fill)


def builder(**params):
    from snake_slam_amd.localmap import LocalMapBuilder

    return LocalMapBuilder(params)


def to_dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        return torch.from_numpy(a.view(np.int64)).cuda()
    if a.dtype.fields:
        return torch.from_numpy(a.view(np.int32).reshape(a.shape + (-1,))).cuda()
    return torch.from_numpy(a).cuda()


def guarded(n_words, fill):
    import torch

    return torch.full((n_words + GUARD,), fill, dtype=torch.int32, device="cuda")


def take(t, n_words, fill, what):
    a = t.cpu().numpy()
    assert np.all(a[n_words:] == fill), f"wrote behind {what}"
    return a[:n_words].copy()


def host_select(b, c):
    return b.select(*(c[k] for k in M.SELECT_KEYS))


def dev_select(b, c):
    import torch

    n, cap = len(c["vote"]), b.kf_cap
    local, out = guarded(n * cap, -9), guarded(n * 5, -7)
    d = [to_dev(c[k]) for k in M.SELECT_KEYS]
    torch.cuda.synchronize()
    b.select_dev(*d, local[:n * cap].view(n, cap), out[:n * 5].view(n, 5))
    b.sync()
    return take(local, n * cap, -9, "local_kf").reshape(n, cap), take(out, n * 5, -7, "out").view(M.SELECT).reshape(n)


def host_gather(b, c, pts_cap):
    m = c["m"]
    return b.gather(*(m[k] for k in M.GATHER_KEYS), m, c["frame_id"], c["local_kf"], c["sel"], c["set_start"], c["set_point"], pts_cap)


def dev_gather(b, c, pts_cap):
    import torch

    m, n = c["m"], len(c["sel"])
    fill32 = int(np.array([FILL] * 4, np.uint8).view(np.int32)[0])
    lm, ids, n_pts, out = guarded(n * pts_cap * 24, fill32), guarded(n * pts_cap, -9), guarded(n, -9), guarded(n * 4, -7)
    d = [to_dev(m[k]) for k in M.GATHER_KEYS]
    pts = {k: to_dev(m[k]) for k in M.POINT_KEYS}
    rest = [to_dev(c[k]) for k in ("frame_id", "local_kf", "sel", "set_start", "set_point")]
    torch.cuda.synchronize()
    b.gather_dev(*d, pts, *rest, pts_cap, lm, ids[:n * pts_cap].view(n, pts_cap), n_pts, out)
    b.sync()
    return (take(lm, n * pts_cap * 24, fill32, "lm_pts").view(M.LM_FINE).reshape(n, pts_cap), take(ids, n * pts_cap, -9, "lm_point").reshape(n, pts_cap),
            take(n_pts, n, -9, "n_pts"), take(out, n * 4, -7, "out").view(M.GATHER).reshape(n))


def same(got, want):
    return len(got) == len(want) and all(np.asarray(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got, want))


def differing(got, want):
    res_g, res_w = got[-1], want[-1]
    rows = [s for s in range(len(res_w)) if any(np.asarray(g[s]).tobytes() != np.asarray(w[s]).tobytes() for g, w in zip(got, want))]
    return [(s, res_g[s], res_w[s]) for s in rows[:4]]


@pytest.mark.parametrize("cap_index", [0, 1, 2, 3])
@pytest.mark.parametrize("seed", M.SEEDS)
def test_select_host_and_device_forms_equal_the_restatement(seed, cap_index):
    """kf_cap = 256, then n_local + 1, n_local and n_local - 1 of the 80-entry vote: the last one is KF_OVERFLOW for that set."""
    c = select_case(seed)
    kf_cap = c["kf_caps"][cap_index]
    params = dict(kf_cap=kf_cap, seed=seed)
    want = M.select(*(c[k] for k in M.SELECT_KEYS), params)
    b = builder(**params)
    try:
        host, dev = host_select(b, c), dev_select(b, c)
    finally:
        b.close()
    assert same(dev, want), differing(dev, want)
    assert same(host, want), differing(host, want)
    assert want[1]["status"][c["cap_set"]] == (M.KF_OVERFLOW if cap_index == 3 else M.OK)
    assert want[1]["status"][c["truncated"]] == M.TRUNCATED and want[1]["status"][0] == M.EMPTY
    if cap_index in (1, 2):
        assert want[1]["n_local"][c["cap_set"]] == kf_cap - (cap_index == 1)


def test_select_parameters_other_than_the_reference_s():
    """n_direct 3, probabilities 2 / 7, 16 neighbours (SNK_LMAP_MAX_NEIGHBOURS), then no neighbours and no draws at all."""
    c = select_case(M.SEEDS[1])
    for params in (dict(n_direct=3, n_direct_prob=2, n_indirect_prob=7, n_neighbours=16, kf_cap=256, seed=5),
                   dict(n_direct=0, n_direct_prob=0, n_indirect_prob=0, n_neighbours=0, kf_cap=1, seed=5),
                   dict(n_direct=300, n_direct_prob=1, n_indirect_prob=1, n_neighbours=1, kf_cap=256, seed=6)):
        want = M.select(*(c[k] for k in M.SELECT_KEYS), params)
        b = builder(**params)
        try:
            host, dev = host_select(b, c), dev_select(b, c)
        finally:
            b.close()
        assert same(dev, want), (params, differing(dev, want))
        assert same(host, want), (params, differing(host, want))


@pytest.mark.parametrize("pts_cap", [64, M.MAX_PTS])
def test_gather_host_and_device_forms_equal_the_restatement(pts_cap):
    c = gather_case(pts_cap)
    b = builder(kf_cap=16)
    try:
        dev = dev_gather(b, c, pts_cap)
        host = host_gather(b, c, pts_cap)
    finally:
        b.close()
    want = gather_want(pts_cap, FILL)
    assert same(dev, want), differing(dev, want)
    want = gather_want(pts_cap, 0)
    assert same(host, want), differing(host, want)
    assert want[3]["status"][c["what"]["cap+1"]] == M.PTS_OVERFLOW and want[2][c["what"]["cap"]] == pts_cap


def test_gather_with_a_feature_range_longer_than_65535():
    """localmap_numpy.long_range_case: the high 16-bit halves of the range lengths and of their prefix sums are not 0."""
    c = M.long_range_case(64)
    b = builder(kf_cap=16)
    try:
        dev = dev_gather(b, c, 64)
        host = host_gather(b, c, 64)
    finally:
        b.close()
    m = c["m"]
    want = M.gather(m, c["frame_id"], c["local_kf"], c["sel"], c["set_start"], c["set_point"], 64, FILL)
    assert same(dev, want), differing(dev, want)
    want = M.gather(m, c["frame_id"], c["local_kf"], c["sel"], c["set_start"], c["set_point"], 64, 0)
    assert same(host, want), differing(host, want)


def test_select_then_gather_on_the_device_without_a_copy_between():
    """Stage 1's outputs go into stage 2 as they lie in HBM; features of the select case's 700 keyframes are drawn for it."""
    import torch

    c, g = select_case(M.SEEDS[2]), gather_case(64)
    n_kf, n_sets, n_points = c["n_kf"], len(c["vote"]), 3000
    rng = np.random.RandomState(3)
    lists = [rng.randint(-1, n_points, rng.randint(0, 30)).tolist() for _ in range(n_kf)]
    m = dict(g["m"], feat_start=M.csr(lists), feat_point=np.array([p for lst in lists for p in lst], np.int32))
    for k in ("pt_flags", "pt_last_seen") + M.POINT_KEYS:
        m[k] = m[k][:n_points]
    own = [rng.randint(-1, n_points, 12).tolist() for _ in range(n_sets)]
    ss, sp = M.csr(own), np.array([p for x in own for p in x], np.int32)
    params, pts_cap = dict(kf_cap=32, seed=M.SEEDS[2]), 2048
    local, sel = M.select(*(c[k] for k in M.SELECT_KEYS), params)
    want = M.gather(m, c["frame_id"], local, sel, ss, sp, pts_cap, FILL)
    assert M.TRUNCATED in sel["status"] and np.sum(sel["status"] == M.OK) > 6 and np.max(want[2]) > 300
    b = builder(**params)
    try:
        local_d, sel_d = torch.full((n_sets, 32), -5, dtype=torch.int32, device="cuda"), torch.full((n_sets, 5), -5, dtype=torch.int32, device="cuda")
        b.select_dev(*(to_dev(c[k]) for k in M.SELECT_KEYS), local_d, sel_d)
        chained = dict(c_local=local_d, c_sel=sel_d)
        fill32 = int(np.array([FILL] * 4, np.uint8).view(np.int32)[0])
        lm, ids, n_pts, out = guarded(n_sets * pts_cap * 24, fill32), guarded(n_sets * pts_cap, -9), guarded(n_sets, -9), guarded(n_sets * 4, -7)
        b.gather_dev(*(to_dev(m[k]) for k in M.GATHER_KEYS), {k: to_dev(m[k]) for k in M.POINT_KEYS}, to_dev(c["frame_id"]), chained["c_local"],
                     chained["c_sel"], to_dev(ss), to_dev(sp), pts_cap, lm, ids[:n_sets * pts_cap].view(n_sets, pts_cap), n_pts, out)
        b.sync()
    finally:
        b.close()
    got = (take(lm, n_sets * pts_cap * 24, fill32, "lm_pts").view(M.LM_FINE).reshape(n_sets, pts_cap), take(ids, n_sets * pts_cap, -9, "lm_point").reshape(n_sets, pts_cap),
           take(n_pts, n_sets, -9, "n_pts"), take(out, n_sets * 4, -7, "out").view(M.GATHER).reshape(n_sets))
    assert local_d.cpu().numpy().tobytes() == local.tobytes() and sel_d.cpu().numpy().tobytes() == sel.tobytes()
    assert same(got, want), differing(got, want)


def test_device_forms_answer_bad_index_per_set():
    """Each kind of bad index on a copy of the case: the sets it reaches have status BAD_INDEX and no list, the others equal the
    restatement (which applies the same checks), the guard words keep their fill."""
    c = select_case(M.SEEDS[0])
    params = dict(kf_cap=64, seed=1)
    n_kf, n_list = c["n_kf"], len(c["conn_list"])

    def edit(key, index, value, field=None):
        e = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
        if field:
            e[key][field][index] = value
        else:
            e[key][index] = value
        return e

    # a direct keyframe of the 15-entry vote that has connections
    direct = next(int(k) for k in c["conn"][3]["kf"][:15][::-1] if c["conn_start"][k + 1] > c["conn_start"][k])
    nb_slot = int(c["conn_start"][direct + 1]) - 1
    cases = [("voted keyframe == n_kf", edit("conn", (5, 2), n_kf, "kf")), ("voted keyframe -1", edit("conn", (6, 0), -1, "kf")),
             ("conn_start beyond the list", edit("conn_start", direct + 1, n_list + 4)),
             ("conn_start decreasing", edit("conn_start", direct + 1, int(c["conn_start"][direct]) - 1)),
             ("neighbour == n_kf", edit("conn_list", nb_slot, n_kf, "kf")), ("neighbour -3", edit("conn_list", nb_slot, -3, "kf")),
             ("vote n_conn above its cap", edit("vote", 4, c["vote_cap"] + 1, "n_conn")), ("vote status 7", edit("vote", 2, 7, "status"))]
    b = builder(**params)
    try:
        for name, e in cases:
            want = M.select(*(e[k] for k in M.SELECT_KEYS), params)
            n_bad = int(np.sum(want[1]["status"] == M.BAD_INDEX))
            assert 0 < n_bad < len(c["vote"]) - 2, (name, n_bad)
            got = dev_select(b, e)
            assert same(got, want), (name, differing(got, want))
        g = gather_case(64)
        m, w = g["m"], g["what"]
        n_points = len(m["pt_flags"])

        def gedit(**kw):
            e = dict(g, m=dict(m))
            for k, (i, v) in kw.items():
                tgt = e["m"] if k in m else e
                tgt[k] = tgt[k].copy()
                tgt[k][i] = v
            return e

        f2 = int(m["feat_start"][2])
        gcases = [("local keyframe == n_kf", gedit(local_kf=((w["mixed"], 1), 16))), ("local keyframe -1 inside n_local", gedit(local_kf=((w["last"], 0), -1))),
                  ("feat_start decreasing", gedit(feat_start=(3, f2 - 1))), ("feat_start beyond the array", gedit(feat_start=(15, len(m["feat_point"]) + 1))),
                  ("point id == n_points", gedit(feat_point=(f2 + 3, n_points))), ("point id -2", gedit(feat_point=(f2, -2))),
                  ("own point id == n_points", gedit(set_point=(int(g["set_start"][w["no_local"]]), n_points))),
                  ("set_start decreasing", gedit(set_start=(w["chunk64"] + 1, int(g["set_start"][w["chunk64"]]) - 1))),
                  ("n_local above kf_cap", gedit(sel=(w["chunk65"], (17, 0, 0, -1, M.OK))))]
        for name, e in gcases:
            want = M.gather(e["m"], e["frame_id"], e["local_kf"], e["sel"], e["set_start"], e["set_point"], 64, FILL)
            n_bad = int(np.sum(want[3]["status"] == M.BAD_INDEX))
            assert 1 < n_bad < len(g["sel"]) - 3, (name, n_bad)  # one set is BAD_INDEX by the status it passes through
            got = dev_gather(b, e, 64)
            assert same(got, want), (name, differing(got, want))
    finally:
        b.close()


def test_a_large_call_then_a_small_one_on_one_handle():
    """SNK_LMAP_MAX_PTS with 16 384 points placed, then pts_cap 64 on the same handle and once more: nothing of the first table, of
    the first call's records or of its staging shows in the second."""
    big, small = gather_case(M.MAX_PTS), gather_case(64)
    b = builder(kf_cap=16)
    try:
        d1, h1 = dev_gather(b, big, M.MAX_PTS), host_gather(b, big, M.MAX_PTS)
        d2, h2 = dev_gather(b, small, 64), host_gather(b, small, 64)
        h3 = host_gather(b, small, 64)
    finally:
        b.close()
    assert same(d1, gather_want(M.MAX_PTS, FILL)) and same(h1, gather_want(M.MAX_PTS, 0))
    assert same(d2, gather_want(64, FILL)), differing(d2, gather_want(64, FILL))
    assert same(h2, gather_want(64, 0)) and same(h3, gather_want(64, 0))


CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import localmap_numpy as M
from snake_slam_amd.localmap import LocalMapBuilder
c, g = M.select_case(M.SEEDS[1]), M.gather_case(64)
b = LocalMapBuilder(dict(kf_cap=c["kf_caps"][2], seed=M.SEEDS[1]))
s = b.select(*(c[k] for k in M.SELECT_KEYS))
m = g["m"]
r = b.gather(*(m[k] for k in M.GATHER_KEYS), m, g["frame_id"], g["local_kf"], g["sel"], g["set_start"], g["set_point"], 64)
b.close()
open(sys.argv[2], "wb").write(b"".join(a.tobytes() for a in s + r))
"""


def test_edge_case_on_poisoned_scratch(tmp_path):
    """SNK_DEBUG_POISON=1 fills fresh scratch and staging with 0xCD (read once: a child process): nothing may rely on zeros."""
    out = tmp_path / "res.bin"
    env = dict(os.environ, SNK_DEBUG_POISON="1", PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", CHILD, str(ROOT / "tests"), str(out)], capture_output=True, text=True, env=env, cwd=str(ROOT), timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    c = select_case(M.SEEDS[1])
    want = M.select(*(c[k] for k in M.SELECT_KEYS), dict(kf_cap=c["kf_caps"][2], seed=M.SEEDS[1])) + gather_want(64, 0)
    assert out.read_bytes() == b"".join(a.tobytes() for a in want)


def test_argument_errors_are_codes_with_a_message_and_nothing_is_written():
    from snake_slam_amd import _lib
    from snake_slam_amd.localmap import LmapMap, LmapParams, LmapPoints

    lib = _lib.load()
    c, g = select_case(M.SEEDS[0]), gather_case(64)
    m = g["m"]
    n_sets, n_gsets = len(c["vote"]), len(g["sel"])
    ptr = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data  # noqa: E731
    b = builder(kf_cap=64)
    try:
        def call_select(par=None, n=None, n_kf=None, vote_cap=None, out=1, local=1, **kw):
            a = {k: np.ascontiguousarray(kw[k]) if kw.get(k) is not None else (None if k in kw else c[k]) for k in M.SELECT_KEYS}
            par = par or LmapParams(15, 5, 5, 5, 64, 0)
            lk, res = np.full((n_sets, 64), -9, np.int32), np.full(n_sets * 5, -9, np.int32)
            rc = lib.snk_lmap_select(b._h, n_sets if n is None else n, ptr(a["conn"]), c["vote_cap"] if vote_cap is None else vote_cap, ptr(a["vote"]),
                                     c["n_kf"] if n_kf is None else n_kf, ptr(a["kf_bad"]), ptr(a["conn_start"]), ptr(a["conn_list"]), ptr(a["frame_id"]),
                                     C.byref(par), lk.ctypes.data if local else None, res.ctypes.data if out else None)
            assert rc == 0 or (np.all(lk == -9) and np.all(res == -9))
            return rc, lib.snk_last_error()

        def call_gather(n=None, kf_cap=16, pts_cap=64, n_kf=None, out=1, **kw):
            a = {k: np.ascontiguousarray(kw[k]) if kw.get(k) is not None else (None if k in kw else (m[k] if k in m else g[k]))
                 for k in M.GATHER_KEYS + M.POINT_KEYS + ("frame_id", "local_kf", "sel", "set_start", "set_point")}
            cm = LmapMap(len(m["feat_start"]) - 1 if n_kf is None else n_kf, len(m["pt_flags"]), kw.get("n_feat", len(m["feat_point"])),
                         *(ptr(a[k]) for k in M.GATHER_KEYS))
            cp = LmapPoints(*(ptr(a[k]) for k in M.POINT_KEYS))
            lm, ids = np.full(n_gsets * 64 * 24, -9, np.int32), np.full(n_gsets * 64, -9, np.int32)
            npts, res = np.full(n_gsets, -9, np.int32), np.full(n_gsets * 4, -9, np.int32)
            rc = lib.snk_lmap_gather(b._h, n_gsets if n is None else n, C.byref(cm), C.byref(cp), ptr(a["frame_id"]), ptr(a["local_kf"]), kf_cap, ptr(a["sel"]),
                                     ptr(a["set_start"]), ptr(a["set_point"]), pts_cap, lm.ctypes.data, ids.ctypes.data, npts.ctypes.data,
                                     res.ctypes.data if out else None)
            assert rc == 0 or all(np.all(x == -9) for x in (lm, ids, npts, res))
            return rc, lib.snk_last_error()

        def bumped(src, key, index, value, field=None):
            a = src[key].copy()
            if field:
                a[field][index] = value
            else:
                a[index] = value
            return {key: a}

        for kw, text in ((dict(par=LmapParams(-1, 5, 5, 5, 64, 0)), b"below 0"), (dict(par=LmapParams(15, -1, 5, 5, 64, 0)), b"below 0"),
                         (dict(par=LmapParams(15, 5, -1, 5, 64, 0)), b"below 0"), (dict(par=LmapParams(15, 5, 5, -1, 64, 0)), b"below 0"),
                         (dict(par=LmapParams(15, 5, 5, 17, 64, 0)), b"n_neighbours"), (dict(par=LmapParams(15, 5, 5, 5, 0, 0)), b"kf_cap"),
                         (dict(par=LmapParams(15, 5, 5, 5, M.MAX_LOCAL_KF + 1, 0)), b"kf_cap"), (dict(n_kf=M.MAX_KF + 1), b"SNK_COVIS_MAX_KF"),
                         (dict(n=-1), b"negative"), (dict(vote_cap=0), b"vote_cap"), (dict(conn=None), b"NULL"), (dict(vote=None), b"NULL"),
                         (dict(kf_bad=None), b"NULL"), (dict(conn_start=None), b"NULL"), (dict(conn_list=None), b"NULL"), (dict(frame_id=None), b"NULL"),
                         (dict(out=0), b"NULL"), (dict(local=0), b"NULL"), (bumped(c, "conn_start", 0, 1), b"begin at 0"),
                         (bumped(c, "conn_start", 9, int(c["conn_start"][8]) - 1), b"non-decreasing"), (bumped(c, "conn_list", 4, c["n_kf"], "kf"), b"connection's keyframe"),
                         (bumped(c, "conn_list", 4, -1, "kf"), b"connection's keyframe"), (bumped(c, "conn", (3, 1), c["n_kf"], "kf"), b"voted keyframe"),
                         (bumped(c, "vote", 3, c["vote_cap"] + 1, "n_conn"), b"vote record"), (bumped(c, "vote", 3, 9, "status"), b"vote record")):
            rc, msg = call_select(**kw)
            assert rc == 1 and text in msg, (kw.keys(), rc, msg)
        assert call_select(n=0, conn=None, vote=None, frame_id=None, out=0, local=0)[0] == 0  # n_sets == 0 is valid
        w = g["what"]
        for kw, text in ((dict(kf_cap=0), b"kf_cap"), (dict(kf_cap=M.MAX_LOCAL_KF + 1), b"kf_cap"), (dict(pts_cap=0), b"pts_cap"),
                         (dict(pts_cap=M.MAX_PTS + 1), b"pts_cap"), (dict(n_kf=M.MAX_KF + 1), b"SNK_COVIS_MAX_KF"), (dict(n=-1), b"negative"),
                         (dict(feat_start=None), b"NULL"), (dict(feat_point=None), b"NULL"), (dict(pt_flags=None), b"NULL"), (dict(pt_last_seen=None), b"NULL"),
                         (dict(pos=None), b"NULL"), (dict(normal=None), b"NULL"), (dict(desc=None), b"NULL"), (dict(ref_depth=None), b"NULL"),
                         (dict(ref_level=None), b"NULL"), (dict(frame_id=None), b"NULL"), (dict(local_kf=None), b"NULL"), (dict(sel=None), b"NULL"),
                         (dict(set_start=None), b"NULL"), (dict(set_point=None), b"NULL"), (dict(out=0), b"NULL"), (dict(n_feat=3), b"n_feat"),
                         (bumped(m, "feat_start", 0, 1), b"begin at 0"), (bumped(m, "feat_start", 3, int(m["feat_start"][2]) - 1), b"non-decreasing"),
                         (bumped(m, "feat_point", 2, len(m["pt_flags"])), b"point id"), (bumped(m, "feat_point", 2, -2), b"point id"),
                         (bumped(g, "set_start", 0, 1), b"begin at 0"), (bumped(g, "set_start", 2, int(g["set_start"][1]) - 1), b"non-decreasing"),
                         (bumped(g, "set_point", 1, len(m["pt_flags"])), b"point id"), (bumped(g, "local_kf", (w["mixed"], 0), 16), b"local keyframe"),
                         (bumped(g, "local_kf", (w["mixed"], 0), -1), b"local keyframe"), (bumped(g, "sel", w["mixed"], 17, "n_local"), b"stage-1 count"),
                         (bumped(g, "sel", w["mixed"], 6, "status"), b"stage-1 status")):
            rc, msg = call_gather(**kw)
            assert rc == 1 and text in msg, (kw.keys(), rc, msg)
        assert call_gather(n=0, frame_id=None, local_kf=None, sel=None, set_start=None, set_point=None, out=0)[0] == 0
        # the handle is as good as before
        assert same(host_gather(b, g, 64), gather_want(64, 0))
    finally:
        b.close()
