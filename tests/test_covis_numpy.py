"""CPU: the restatement of "snk-covis v1" (tests/covis_numpy.py, a dictionary loop written from Keyframe.cpp:89-171 and
TrackingFine.cpp:230-268) against an independent formulation -- the counts as a sparse matrix product G . O with the query's own column
removed, G[q, p] = number of gated features of q on p, O[p, k] = number of observations of p by k -- and the properties of the
semantics asserted directly on the hand-built edge case."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import covis_numpy as M


@functools.lru_cache(maxsize=None)
def edge():
    return M.edge_case()


def counts_by_product(m, connection, set_start=None, set_point=None):
    """[sets, n_kf] counts: G . O, for the connection form with the gate and without the diagonal."""
    n_kf, n_pts = len(m["kf_bad"]), len(m["pt_flags"])
    obs_point = np.repeat(np.arange(n_pts), np.diff(m["obs_start"]))
    O = sp.coo_matrix((np.ones(len(obs_point), np.int64), (obs_point, m["obs"][:, 0])), shape=(n_pts, n_kf)).tocsr()
    if connection:
        start, point = m["feat_start"], m["feat_point"]
        ok = point >= 0
        flags = m["pt_flags"][np.where(ok, point, 0)]
        ok &= (flags & M.PT_BAD) == 0
        ok &= ~((m["feat_depth"] > np.float32(M.TH_DEPTH)) | ((flags & M.PT_FAR) != 0))
    else:
        start, point = np.asarray(set_start), np.asarray(set_point).reshape(-1)
        ok = point >= 0
        ok &= (m["pt_flags"][np.where(ok, point, 0)] & M.PT_BAD) == 0
    row = np.repeat(np.arange(len(start) - 1), np.diff(start))
    G = sp.coo_matrix((np.ones(int(ok.sum()), np.int64), (row[ok], point[ok])), shape=(len(start) - 1, n_pts)).tocsr()
    counts = np.asarray((G @ O).todense())
    if connection:
        np.fill_diagonal(counts, 0)
    return counts


def list_from_counts(counts, kf_bad, th, connection):
    """The full ascending list [(weight, kf)] of one set from its row of counts, by sorting arrays."""
    ids = np.nonzero(counts)[0]
    if len(ids) == 0:
        return None
    if connection:
        ids = ids[kf_bad[ids] == 0]
        listed = ids[counts[ids] >= th]
        if len(listed) == 0 and len(ids):
            listed = ids[counts[ids] == counts[ids].max()][:1]  # ids ascend: the smallest among the largest
        ids = listed
    order = np.lexsort((ids, counts[ids]))
    return [(int(counts[k]), int(k)) for k in ids[order]]


def check_against_product(m, q, conn, res, cap, connection, set_start=None, set_point=None):
    counts = counts_by_product(m, connection, set_start, set_point)
    for s in range(len(res)):
        full = list_from_counts(counts[q[s]] if connection else counts[s], m["kf_bad"], M.TH, connection)
        if full is None:
            assert tuple(res[s]) == (0, 0, -1, M.UNCHANGED)
            continue
        kept = full[max(len(full) - cap, 0):]
        assert tuple(res[s]) == (len(full), len(kept), kept[-1][1] if kept else -1, M.OK), s
        assert [tuple(x) for x in conn[s][:len(kept)]] == kept, s
        assert np.all(conn[s][len(kept):]["kf"] == -1)


@pytest.mark.parametrize("cap", [4, 64, 256])
def test_restatement_equals_the_sparse_product_on_the_edge_case(cap):
    c = edge()
    conn, res = M.update(c, c["q"], cap=cap)
    check_against_product(c, c["q"], conn, res, cap, True)
    conn, res = M.vote(c, c["set_start"], c["set_point"], cap=cap)
    check_against_product(c, None, conn, res, cap, False, c["set_start"], c["set_point"])


def test_restatement_equals_the_sparse_product_on_a_structured_map():
    m = M.make_map(11, 300, 6000)
    q = np.arange(300, dtype=np.int32)
    conn, res = M.update(m, q, cap=32)
    check_against_product(m, q, conn, res, 32, True)
    # structured: the usual query lists several keyframes at or above the threshold, the fallback is the exception
    assert np.median(res["n_found"]) >= 5 and np.mean(res["n_found"] == 1) < 0.05
    assert np.all(conn["weight"][res["n_found"] > 1][:, 0] >= M.TH)
    ss, spts = M.frames_of(m, 12, 40)
    conn, res = M.vote(m, ss, spts, cap=32)
    check_against_product(m, None, conn, res, 32, False, ss, spts)


@pytest.mark.parametrize("n_kf", [1, 2, 255, 256, 257, 1025])
def test_every_keyframe_count_of_the_edge_case(n_kf):
    c = M.edge_case(n_kf)
    conn, res = M.update(c, c["q"], cap=64)
    check_against_product(c, c["q"], conn, res, 64, True)
    if n_kf == 1:
        assert np.all(res["status"] == M.UNCHANGED)  # only the query itself observes its points
    if n_kf == 2:
        assert tuple(res[0]) == (1, 1, 1, M.OK) and tuple(conn[0][0]) == (16, 1)
        assert tuple(res[1]) == (1, 1, 0, M.OK) and tuple(conn[1][0]) == (6, 0)  # 6 < th: the fallback; (1, 0, 0) lists 0 twice


def test_properties_of_the_edge_case():
    c = edge()
    w = c["what"]
    conn, res = M.update(c, c["q"], cap=256)
    lst = lambda name: [tuple(x) for x in conn[w[name]][:res[w[name]]["n_conn"]]]  # noqa: E731
    last = len(c["kf_bad"]) - 1
    # 14 is out, 15 and 16 are in; equal weights ascend by id; depth == th_depth and <= 0 count, just above / far / bad do not
    assert lst("thresholds") == [(15, 0), (15, 11), (15, 13), (15, 17), (15, last), (16, 12)]
    assert res[w["thresholds"]]["best_kf"] == 12
    assert lst("thresholds_again") == lst("thresholds")
    assert lst("fallback_tie") == [(7, 20)]  # 20 and 21 tied below th: the smallest id
    assert lst("bad_largest") == [(15, 32), (20, 31)] and c["kf_bad"][30] == 1
    assert tuple(res[w["only_bad"]]) == (0, 0, -1, M.OK)
    assert lst("bad_fallback") == [(4, 31)]
    assert tuple(res[w["untouched"]]) == tuple(res[w["no_features"]]) == (0, 0, -1, M.UNCHANGED)
    assert lst("duplicates") == [(16, 40), (16, 41)]
    long = dict((k, v) for v, k in lst("long_lists"))
    assert 0 not in long and last not in long and long[50] == 1 + 1 + 1 + 2 + 21  # ids 0 and n_kf - 1 have 8 < th; 50 is on every long list
    assert res[w["long_lists"]]["n_found"] == 200
    for cap in M.TRUNC_CAPS:
        conn_c, res_c = M.update(c, c["q"], cap=cap)
        for j, n in enumerate((cap - 1, cap, cap + 1, 3 * cap)):
            r = res_c[w[f"trunc{cap}_{j}"]]
            full = lst(f"trunc{cap}_{j}")
            assert r["n_found"] == n == len(full) and r["n_conn"] == min(n, cap)
            assert [tuple(x) for x in conn_c[w[f"trunc{cap}_{j}"]][:r["n_conn"]]] == full[-min(n, cap):]
        cut = lst(f"trunc{cap}_3")
        assert cut[-cap][0] == cut[-cap - 1][0]  # equal weights on both sides of the cut: the id decides
    vconn, vres = M.vote(c, c["set_start"], c["set_point"], cap=256)
    f = w["set_frame"]
    got = dict((k, v) for v, k in vconn[f][:vres[f]["n_conn"]])
    assert got[5] == 75 and got[13] == 15 and got[14] == 15 and got[15] == 15 and got[16] == 14  # no self exclusion, no gate, bad points skipped
    assert vres[f]["best_kf"] == 5
    assert tuple(vres[w["set_empty"]]) == tuple(vres[w["set_none"]]) == tuple(vres[w["set_only_bad_points"]]) == (0, 0, -1, M.UNCHANGED)
    assert vres[w["set_trunc4_1"]]["n_found"] == 4 and vres[w["set_long"]]["n_found"] == 202  # no threshold: 0 and n_kf - 1 beside the 200
    k = w["set_bad_keyframe"]
    assert [tuple(x) for x in vconn[k][:3]] == [(15, 32), (20, 31), (40, 30)] and vres[k]["best_kf"] == 30  # bad keyframes are kept
