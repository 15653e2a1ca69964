"""CPU: the restatement of "snk-lmap v1" (tests/localmap_numpy.py) against cases worked by hand from the reference's text
(Snake/Tracking/TrackingFine.cpp:272-356, Snake/Map/LocalMap.h:139-154), the integer draw rule against exact rational arithmetic, and
the case builders' own coverage assertions."""
from fractions import Fraction

import numpy as np
import pytest

import localmap_numpy as M


def votes(lists, cap=None):
    cap = cap or max(max((len(x) for x in lists), default=1), 1)
    conn = np.empty((len(lists), cap), M.CONN)
    conn["weight"] = conn["kf"] = -1
    vote = np.zeros(len(lists), M.VOTE)
    for s, lst in enumerate(lists):
        conn[s, :len(lst)] = [(i + 1, k) for i, k in enumerate(lst)]
        vote[s] = (len(lst), len(lst), lst[-1], M.VOTE_OK) if lst else (0, 0, -1, M.VOTE_UNCHANGED)
    return conn, vote


def graph(n_kf, lists):
    """lists: kf -> neighbour ids, ascending by weight."""
    ls = [lists.get(k, []) for k in range(n_kf)]
    return M.csr(ls), np.array([(10 + i, nb) for lst in ls for i, nb in enumerate(lst)], M.CONN).reshape(-1)


def test_mix_is_the_hash_of_the_p3p_sampler_and_the_draw_rule_is_exact():
    x = 0xDEADBEEF  # the five steps of p3p_mix by hand
    x ^= x >> 16
    x = x * 0x7FEB352D % 2 ** 32
    x ^= x >> 15
    x = x * 0x846CA68B % 2 ** 32
    x ^= x >> 16
    assert M.mix(0xDEADBEEF) == x and M.mix(0) == 0 and M.mix(2 ** 32 + 1) == M.mix(1) != 1
    assert M.key_of(0, 5) == M.mix(M.mix(0x9E3779B9)) ^ 5 and M.key_of(7 << 32, 0) == M.mix(M.mix(0x9E3779B9) ^ 7)
    assert M.draw(9, 3) == M.mix(M.mix(9) ^ 3)
    for k in (0, 1, 5):
        for n in (0, 1, k, k + 1, 7, 65, 32768):
            for h in (0, 1, 2 ** 31, 2 ** 32 - 1, (k << 32) // max(n, 1), max((k << 32) // max(n, 1) - 1, 0)):
                want = k > 0 if n == 0 else Fraction(h, 2 ** 32) < Fraction(k, n)  # sampleDouble(0, 1) < k / double(n); n = 0: inf
                assert M.accept(h, k, n) == want, (h, k, n)
    assert all(M.accept(h, 5, n) for n in range(6) for h in (0, 2 ** 32 - 1))  # n <= k always accepts


def test_direct_keyframes_from_the_back_and_the_reference_keyframe():
    n_kf = 40
    conn, vote = votes([[3], [5, 9, 2], list(range(20, 34)), list(range(20, 35)), []], cap=16)
    cs, cl = graph(n_kf, {})
    local, res = M.select(conn, vote, np.zeros(n_kf, np.uint8), cs, cl, np.arange(5), dict(kf_cap=16))
    assert local[0].tolist() == [3] + [-1] * 15 and tuple(res[0]) == (1, 1, 0, 3, M.OK)
    assert local[1].tolist()[:3] == [2, 9, 5] and tuple(res[1]) == (3, 3, 0, 2, M.OK)
    assert local[2].tolist()[:14] == list(range(33, 19, -1)) and tuple(res[2]) == (14, 14, 0, 33, M.OK)
    assert local[3].tolist()[:15] == list(range(34, 19, -1)) and tuple(res[3]) == (15, 15, 0, 34, M.OK)
    assert tuple(res[4]) == (0, 0, 0, -1, M.EMPTY) and np.all(local[4] == -1)


def test_walks_by_hand_with_draws_looked_up():
    """20 voted keyframes 100 .. 119 (R = 5: all five accepted, in order from the back); then 22 (R = 7): the draws decide."""
    n_kf = 200
    nbs = {119: [1, 2, 3, 4, 5, 6, 100, 7], 118: [7, 8], 104: [8, 9, 150]}  # 119's last five: 4 5 6 100 7; 100 is marked by the vote
    cs, cl = graph(n_kf, nbs)
    bad = np.zeros(n_kf, np.uint8)
    bad[5] = 1
    conn, vote = votes([list(range(100, 120)), list(range(100, 122))])
    fid = np.array([11, 12])
    par = dict(kf_cap=64, seed=77)
    local, res = M.select(conn, vote, bad, cs, cl, fid, par)
    # set 0: direct 119 .. 105, then 104 .. 100 accepted (n <= k); neighbours in list order: 119 -> 4, 6, 7 (5 bad, 100 marked),
    # 118 -> 8 (7 again), 104 -> 9, 150 (8 again): indirect = [4, 6, 7, 8, 9, 150], draws 5 .. 10 against 5 / 6
    key = M.key_of(77, 11)
    indirect = [4, 6, 7, 8, 9, 150]
    picked = [kf for j, kf in enumerate(indirect) if M.draw(key, 5 + j) * 6 < 5 << 32]
    assert local[0, :res[0]["n_local"]].tolist() == list(range(119, 99, -1)) + picked
    assert tuple(res[0]) == (20 + len(picked), 15, 6, 119, M.OK)
    # set 1: direct 121 .. 107; 106 .. 100 take draws 0 .. 6 against 5 / 7
    key = M.key_of(77, 12)
    acc = [M.draw(key, j) * 7 < 5 << 32 for j in range(7)]
    walk = list(range(106, 99, -1))
    first = [kf for kf, a in zip(walk, acc) if a]
    ind = [kf for kf, a in zip(walk, acc) if not a]
    loc = list(range(121, 106, -1)) + first
    marked = set(range(100, 122))
    for kf in loc:
        for nb in nbs.get(kf, [])[-5:]:
            if not bad[nb] and nb not in marked:
                ind.append(nb)
                marked.add(nb)
    loc += [kf for j, kf in enumerate(ind) if M.draw(key, 7 + j) * len(ind) < 5 << 32]
    assert local[1, :res[1]["n_local"]].tolist() == loc and tuple(res[1]) == (len(loc), 15, len(ind), 121, M.OK)


def test_statuses_of_stage_one():
    n_kf = 30
    cs, cl = graph(n_kf, {})
    bad = np.zeros(n_kf, np.uint8)
    conn, vote = votes([[1, 2, 3], [1, 2, 3], [1, 2, 30], [1, 2, 3], list(range(20))], cap=20)
    vote[1]["n_found"] = 9  # cut by its cap
    vote[3]["status"] = M.VOTE_BAD_INDEX
    local, res = M.select(conn, vote, bad, cs, cl, np.zeros(5, np.int32), dict(kf_cap=19))
    assert res["status"].tolist() == [M.OK, M.TRUNCATED, M.BAD_INDEX, M.BAD_INDEX, M.KF_OVERFLOW]
    assert np.all(local[1:] == -1) and all(tuple(r) == (0, 0, 0, -1, r["status"]) for r in res[1:])
    # a bad keyframe of the vote's list is kept
    bad[3] = 1
    assert M.select(conn, vote, bad, cs, cl, np.zeros(5, np.int32), dict(kf_cap=19))[0][0].tolist()[:3] == [3, 2, 1]


def test_gather_by_hand():
    n_points = 12
    m = dict(feat_start=M.csr([[0] * 4, [], [0] * 5]), feat_point=np.array([4, -1, 5, 4, 6, 5, 7, 8, 9], np.int32),
             pt_flags=np.zeros(n_points, np.uint8), pt_last_seen=np.full(n_points, -1, np.int32), **M.point_tables(n_points))
    m["pt_flags"][7] = M.PT_BAD
    m["pt_last_seen"][8] = 3
    sel = np.array([(3, 3, 0, 2, M.OK), (1, 1, 0, 0, M.OK), (0, 0, 0, -1, M.EMPTY), (0, 0, 0, -1, M.KF_OVERFLOW)], M.SELECT)
    local = np.array([[2, 1, 0], [0, -1, -1], [-1] * 3, [-1] * 3], np.int32)
    own = [[5, 10, 10, -1, 7], [], [9, 9], [1]]
    lm, ids, n_pts, res = M.gather(m, np.array([3, 3, 3, 3]), local, sel, M.csr(own), np.array([p for x in own for p in x]), 6, fill=0xEE)
    # set 0: keyframe 2 places 6 5 9 (7 bad, 8 seen in frame 3), keyframe 0 adds 4; own 5 clears its flag, 10 is new once
    assert ids[0].tolist() == [6, 5, 9, 4, 10, -1] and lm[0]["valid"][:5].tolist() == [1, 0, 1, 1, 0] and tuple(res[0]) == (5, 3, 1, M.OK)
    assert lm[0, 1]["pos"].tolist() == m["pos"][5].tolist() and lm[0, 1]["desc"].tolist() == m["desc"][5].tolist()
    assert lm[0, 4]["reference_depth"] == m["ref_depth"][10] and lm[0, 4]["reference_scale_level"] == m["ref_level"][10]
    assert np.all(lm[0, :5]["pad"] == 0) and np.all(lm[0, 5:].view(np.uint8) == 0xEE)
    assert ids[1].tolist() == [4, 5, -1, -1, -1, -1] and tuple(res[1]) == (2, 2, 0, M.OK)
    assert ids[2].tolist()[:2] == [9, -1] and tuple(res[2]) == (1, 0, 1, M.OK) and lm[2, 0]["valid"] == 0
    assert tuple(res[3]) == (0, 0, 0, M.KF_OVERFLOW) and n_pts.tolist() == [5, 2, 1, 0]
    # pts_cap 4 < 5 distinct points
    r4 = M.gather(m, np.array([3, 3, 3, 3]), local, sel, M.csr(own), np.array([p for x in own for p in x]), 4)
    assert tuple(r4[3][0]) == (0, 0, 0, M.PTS_OVERFLOW) and np.all(r4[1][0] == -1) and tuple(r4[3][1]) == (2, 2, 0, M.OK)


@pytest.mark.parametrize("seed", M.SEEDS)
def test_the_select_case_asserts_its_own_coverage(seed):
    c = M.select_case(seed)
    assert len(c["kf_caps"]) == 4 and c["kf_caps"][1] - 2 == c["kf_caps"][3]


@pytest.mark.parametrize("pts_cap", [64, M.MAX_PTS])
def test_the_edge_case_asserts_its_own_coverage(pts_cap):
    c = M.edge_case(pts_cap)
    g = c["gather"]
    assert {"mixed", "cap-1", "cap", "cap+1", "collisions", "no_local", "passed_truncated"} <= set(g["what"])
    assert M.table_slots(64) == 512 and len(g["same"]) == 40 and len(g["wrap"]) == 6


def test_the_generator_fails_when_a_situation_is_missing(monkeypatch):
    """The coverage assertions are live: with no neighbours asked for none is ever met, and the builder refuses."""
    monkeypatch.setattr(M, "PARAMS", dict(M.PARAMS, n_neighbours=0))
    with pytest.raises(AssertionError):
        M.select_case(0)
