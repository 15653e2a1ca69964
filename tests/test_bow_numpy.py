"""CPU: the numpy restatement of "snk-bow v1" (tests/bow_numpy.py) against brute-force definitions on tiny cases -- the descent
against an exhaustive strict-< scan per level, the score against the dense-vector L1 formula, the query against a literal transcription of
KeyframeDatabase.cpp:100-168 with an inverted list, MatchBoW against a literal transcription of LoopORBMatcher.cpp:121-215 -- and
answers worked out by hand on a two-level tree of three children."""
import numpy as np
import pytest

import bow_numpy as B


def popcount(x):
    return bin(int(x)).count("1")


def dist(a, b):
    return sum(popcount(int(x) ^ int(y)) for x, y in zip(a, b))


def descend_exhaustive(V, d):
    node, path = 0, [0]
    while V.child_count[node] > 0:
        best, best_child = None, None
        for c in V.kids(node):
            dc = dist(d, V.desc[c])
            if best is None or dc < best:  # strict <: the first child keeps a tie
                best, best_child = dc, int(c)
        node = best_child
        path.append(node)
    return path


@pytest.mark.parametrize("name", ["k4_L6", "irregular", "single_level", "twins_k4_L3"])
def test_descent_equals_the_exhaustive_scan(name):
    V = B.vocab(name)
    descs = np.concatenate([B.frame_descriptors(name, 40), B.tie_descriptors(name, 20) if name.startswith("twins") else B.frame_descriptors(name, 5, 3)])
    for d in descs:
        assert B.descend(V, d) == descend_exhaustive(V, d)


def test_twin_vocabulary_really_ties():
    V = B.vocab("twins_k4_L3")
    ties = 0
    for d in B.tie_descriptors():
        path = B.descend(V, d)
        for a, b in zip(path[:-1], path[1:]):
            ds = [dist(d, V.desc[c]) for c in V.kids(a)]
            ties += ds.count(min(ds)) > 1
            assert b == V.kids(a)[ds.index(min(ds))]
    assert ties >= 40  # equidistant children at several levels


def test_hand_vocabulary_known_answers():
    """Level 1: A = 0, B = low 64 bits, C = all ones (nodes 1-3); the children of X (nodes 4-6, 7-9, 10-12; words 0-8) are X, X ^ bit 62 of
    word 3, X ^ bits 62 and 63 of word 3.  Weights of the words: 1 2 3 1 1 1 4 .5 .25."""
    V = B.hand_vocab()
    assert V.L == 2 and V.n_words == 9
    z, f = 0, 0xFFFFFFFFFFFFFFFF
    descs = np.array([[z, z, z, z],                # A at distance 0; children 0, 1, 2 -> node 4, word 0
                      [z, z, z, 1 << 62],          # A; children 1, 0, 1 -> node 5, word 1
                      [z, z, z, 1 << 63],          # A; children 1, 2, 1: nodes 4 and 6 tie, the first wins -> node 4, word 0
                      [0xFFFFFFFF, z, z, z],       # A and B both at 32: A wins; children 32, 33, 34 -> node 4, word 0
                      [f, f, f, f],                # C -> node 10, word 6
                      [f, z, z, 3 << 62]], np.uint64)  # B at 2; children 2, 1, 0 -> node 9, word 5
    t = B.transform(V, descs, 1)
    assert t["word_of_feature"].tolist() == [0, 1, 0, 0, 6, 5]
    assert t["node_of_feature"].tolist() == [1, 1, 1, 1, 3, 2]
    assert t["words"].tolist() == [0, 1, 5, 6]
    assert np.allclose(t["values"], [0.3, 0.2, 0.1, 0.4], rtol=0, atol=1e-15)  # 3 * 1, 1 * 2, 1 * 1, 1 * 4 over 10
    assert t["node_id"].tolist() == [1, 2, 3] and t["node_start"].tolist() == [0, 4, 5, 6] and t["features"].tolist() == [0, 1, 2, 3, 5, 4]
    t0 = B.transform(V, descs, 0)
    assert t0["node_of_feature"].tolist() == [4, 5, 4, 4, 10, 9]
    assert t0["node_id"].tolist() == [4, 5, 9, 10] and t0["features"].tolist() == [0, 2, 3, 1, 5, 4]
    for up in (2, 3):  # L - levelsup <= 0: the root, no feature vector
        tr = B.transform(V, descs, up)
        assert tr["node_of_feature"].tolist() == [0] * 6 and len(tr["node_id"]) == 0 and tr["node_start"].tolist() == [0]
    assert abs(B.score((t["words"], t["values"]), (t["words"], t["values"])) - 1.0) < 1e-15
    # common words 0 and 6: (|.3 - .5| - .8) + (|.4 - .5| - .9) = -1.4 -> 0.7
    assert abs(B.score((t["words"], t["values"]), (np.array([0, 6]), np.array([0.5, 0.5]))) - 0.7) < 1e-15
    empty = B.transform(V, np.zeros((0, 4), np.uint64), 1)
    assert len(empty["words"]) == 0 and len(empty["node_id"]) == 0 and empty["node_start"].tolist() == [0]


def test_score_equals_the_dense_l1_formula():
    rng = np.random.default_rng(3)
    for _ in range(20):
        nw = 50
        a, b = np.zeros(nw), np.zeros(nw)
        ia, ib = rng.choice(nw, 12, replace=False), rng.choice(nw, 17, replace=False)
        a[ia], b[ib] = rng.random(12), rng.random(17)
        a, b = a / a.sum(), b / b.sum()
        sa, sb = (np.nonzero(a)[0], a[np.nonzero(a)[0]]), (np.nonzero(b)[0], b[np.nonzero(b)[0]])
        dense = 1.0 - 0.5 * np.abs(a - b).sum()  # for two L1-normalised vectors
        assert abs(B.score(sa, sb) - dense) < 1e-12
        assert 0.0 <= B.score(sa, sb) <= 1.0


def query_transcription(rows, n_words, q, exclude, swr, sr, ms, k):
    """KeyframeDatabase.cpp:100-168 with its inverted list; the tie order of std::sort is fixed as the definition fixes it"""
    inverse = [[] for _ in range(n_words)]
    for kf, (w, _) in rows.items():
        for x in w:
            inverse[int(x)].append(kf)
    loop_words, kfs = {}, []
    for x in q[0]:  # GetKeyframesWithSharingWords
        for kf in inverse[int(x)]:
            if kf not in loop_words:
                loop_words[kf] = 0
                kfs.append(kf)
            loop_words[kf] += 1
    kfs = [kf for kf in kfs if kf not in exclude]
    max_common = 0
    for kf in kfs:
        if loop_words[kf] > max_common:
            max_common = loop_words[kf]
    kfs = [kf for kf in kfs if not (np.float32(loop_words[kf]) < np.float32(swr) * np.float32(max_common))]
    best, sc = 0.0, {}
    for kf in kfs:
        a, b = dict(zip(q[0].tolist(), q[1].tolist())), dict(zip(rows[kf][0].tolist(), rows[kf][1].tolist()))
        s = 0.0
        for w in sorted(set(a) & set(b)):
            s += abs(a[w] - b[w]) - a[w] - b[w]
        sc[kf] = -0.5 * s
        best = max(best, sc[kf])
    kfs = [kf for kf in kfs if not (sc[kf] < float(np.float32(sr)) * best or sc[kf] < float(np.float32(ms)))]
    kfs.sort(key=lambda kf: (-sc[kf], kf))
    return kfs[:k], sc


def small_database(seed, n_kf=30):
    V = B.vocab("k4_L6")
    frames = B.place_keyframes("k4_L6", 5, n_kf // 5, 60, seed)
    rows = {}
    for i, d in enumerate(frames):
        t = B.transform(V, d, 4)
        rows[3 * i + 1] = (t["words"], t["values"])
    return V, rows


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_query_equals_the_transcription(seed):
    V, rows = small_database(seed)
    ids = sorted(rows)
    for qi in (ids[0], ids[7], ids[-1]):
        q = rows[qi]
        for exclude in ((), (qi,), tuple(ids[:10])):
            for (swr, sr, ms, k) in ((0.8, 0.75, 0.0, 10), (0.5, 0.3, 0.05, 3), (0.0, 0.0, 0.0, 64), (0.8, 0.75, 0.9, 10)):
                want, sc = query_transcription(rows, V.n_words, q, exclude, swr, sr, ms, k)
                got = B.query(rows, q, exclude, swr, sr, ms, k)
                assert got["ids"].tolist() == want
                assert np.allclose(got["scores"], [sc[i] for i in want], rtol=0, atol=1e-12)
    nothing = (np.array([], np.int32), np.array([]))
    assert len(B.query(rows, nothing)["ids"]) == 0  # maxCommon = 0: 0 < 0.8 * 0 is false, and still nobody is a candidate


def match_transcription(desc1, has1, bow1, desc2, has2, bow2, threshold, ratio):
    """LoopORBMatcher.cpp:121-215 line by line over dicts node -> feature list"""
    fv1 = {int(n): list(bow1[2][bow1[1][i]: bow1[1][i + 1]]) for i, n in enumerate(bow1[0])}
    fv2 = {int(n): list(bow2[2][bow2[1][i]: bow2[1][i + 1]]) for i, n in enumerate(bow2[0])}
    m12, matched2, n = [-1] * len(desc1), [False] * len(desc2), 0
    for node in sorted(fv1):
        if node not in fv2:
            continue
        for idx1 in fv1[node]:
            if not has1[idx1]:
                continue
            best1, best_idx2, best2 = 256, -1, 256
            for idx2 in fv2[node]:
                if matched2[idx2] or not has2[idx2]:
                    continue
                d = dist(desc1[idx1], desc2[idx2])
                if d < best1:
                    best2, best1, best_idx2 = best1, d, idx2
                elif d < best2:
                    best2 = d
            if best1 < threshold and np.float32(best1) < np.float32(ratio) * np.float32(best2):
                matched2[best_idx2] = True
                m12[idx1] = best_idx2
                n += 1
    return m12, n


CASES = [c for c in B.match_cases() if len(c[1]["desc1"]) <= 300]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_match_bow_equals_the_transcription(case):
    name, s, th, ratio = case
    want, n = match_transcription(s["desc1"], s["has1"], s["bow1"], s["desc2"], s["has2"], s["bow2"], th, ratio)
    got, k = B.match_bow(s["desc1"], s["has1"], s["bow1"], s["desc2"], s["has2"], s["bow2"], th, ratio)
    assert got.tolist() == want and k == n


def test_match_cases_exercise_what_they_name():
    by = {c[0]: c for c in B.match_cases()}
    run = lambda c: B.match_bow(c[1]["desc1"], c[1]["has1"], c[1]["bow1"], c[1]["desc2"], c[1]["has2"], c[1]["bow2"], c[2], c[3])
    assert run(by["list_0"])[1] == 0 and run(by["kf2_without_points"])[1] == 0
    assert run(by["list_70"])[1] >= 2 and run(by["list_17"])[1] >= 2
    assert run(by["duplicate_best"])[0].tolist() == [-1]  # best == second best: the ratio test rejects
    m = run(by["competing"])[0].tolist()
    assert m[0] == 1 and m[1] != 1  # the exact copy comes second and finds its partner taken
    assert run(by["threshold_equal"])[0].tolist() == [-1] and run(by["threshold_above"])[0].tolist() == [0]
    assert run(by["scene_k4_L6_2048"])[1] > 100


@pytest.mark.parametrize("n_kf", B.DB_SIZES)
def test_database_scenarios_keep_their_margin(n_kf):
    """The precondition of the GPU database test, checked where the seeds are chosen: no scored keyframe has a score within 1e-9 of
    `score_ratio * best` or of `min_score`, and no two scored keyframes with different rows have scores within 1e-9 of each other, so a
    difference of an ulp between two summation orders can change neither a candidate list nor its order."""
    rows = B.db_rows(n_kf)
    assert len(rows) == n_kf
    some = 0
    for name, q, exclude, swr, sr, ms, mc in B.db_queries(n_kf):
        res = B.query(rows, q, exclude, swr, sr, ms, mc)
        # a threshold of exactly 0 (score_ratio 0 and min_score 0) cuts nothing: every score is > 0 there, by more than the margin
        assert B.query_margin(res, rows) > 1e-9, (name, B.query_margin(res, rows))
        if name.startswith("no_common") or name.startswith("empty") or "min_score_above" in name:
            assert len(res["ids"]) == 0, name
        if name.startswith("own_row"):
            assert abs(res["scores"][0] - 1.0) < 1e-12
        some += len(res["ids"])
    assert some > 0 or n_kf == 0
    if n_kf >= 65:
        wide = [B.query(rows, q, e, a, b, c, d) for name, q, e, a, b, c, d in B.db_queries(n_kf) if name.endswith("wide_64")]
        assert max(len(w["ids"]) for w in wide) > 10  # the top-k really cuts / orders a long list
