"""GPU: the bag-of-words entry points (snk_bow_*, snk_match_loop_bow*) against the numpy restatement of "snk-bow v1"
(tests/bow_numpy.py).  Every integer output -- words, nodes, CSR offsets, feature lists, candidate ids and their order, common-word
counts, match12, pair lists -- must be bit-identical; bow values and scores must agree within 1e-12 absolute: a value or a score is a sum
of at most 2048 non-negative terms <= 1 in double, and two summation orders differ by at most about 2048 * 2 * 1.1e-16 = 4.5e-13.  The
largest difference observed is printed."""
import numpy as np
import pytest

import bow_numpy as B

pytestmark = pytest.mark.gpu

TOL = 1e-12
CAP = 2048


@pytest.fixture(scope="module")
def vocabs():
    from snake_slam_amd.bow import Vocabulary

    made = {}

    def get(name):
        if name not in made:
            made[name] = Vocabulary.from_arrays(B.vocab(name).arrays())
        return made[name]

    yield get
    for v in made.values():
        v.close()


def assert_transform_equal(got, want, where):
    for k in ("words", "node_id", "node_start", "features", "word_of_feature", "node_of_feature"):
        assert np.array_equal(got[k], want[k]), (where, k)
    worst = float(np.abs(got["values"] - want["values"]).max()) if len(want["values"]) else 0.0
    assert worst <= TOL, (where, worst)
    return worst


# ------------------------------------------------------------------------------------------------------------------------------------
# transform
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k10_L3", "k4_L6", "irregular", "single_level"])
def test_transform_equals_the_restatement(vocabs, name):
    V, G = B.vocab(name), vocabs(name)
    assert (G.size(), G.n_nodes, G.depth) == (V.n_words, len(V.child_count), V.L)
    worst = 0.0
    for n in B.FEATURE_COUNTS:
        descs = B.frame_descriptors(name, n)
        paths = [B.descend(V, d) for d in descs]
        for up in B.levelsups(V):
            worst = max(worst, assert_transform_equal(G.transform(descs, up), B.transform(V, descs, up, paths), (name, n, up)))
    print(f"{name}: largest difference of a bow value to the restatement {worst:.2e}")


def test_transform_ties_go_to_the_first_child(vocabs):
    V, G = B.vocab("twins_k4_L3"), vocabs("twins_k4_L3")
    descs = B.tie_descriptors()
    for up in (0, 1, 2):
        assert_transform_equal(G.transform(descs, up), B.transform(V, descs, up), ("ties", up))


@pytest.mark.parametrize("distinct", [False, True])
def test_transform_crowding(vocabs, distinct):
    for name in ("k10_L3", "irregular"):
        V, G = B.vocab(name), vocabs(name)
        descs = B.crowd_descriptors(name, distinct)
        got, want = G.transform(descs, 1), B.transform(V, descs, 1)
        assert len(want["words"]) == (len(descs) if distinct else 1)
        assert_transform_equal(got, want, (name, distinct))


def batch_frames(name, counts, cap=CAP):
    import torch

    desc = np.zeros((len(counts), cap, 4), np.uint64)
    rng = np.random.default_rng(1)
    desc[:] = rng.integers(0, 2 ** 64, desc.shape, dtype=np.uint64)  # what lies behind a frame's n must not matter
    sets = [B.frame_descriptors(name, n, seed=3 + i) for i, n in enumerate(counts)]
    for b, d in enumerate(sets):
        desc[b, : len(d)] = d
    return sets, torch.from_numpy(desc.view(np.int64)).cuda(), torch.tensor(counts, dtype=torch.int32).cuda()


def test_transform_batch_equals_the_per_frame_calls(vocabs):
    import torch

    from snake_slam_amd.bow import Vocabulary, desc_frames_dev

    name, counts = "irregular", [1000, 0, 17, 2048, 1]
    sets, desc_dev, n_dev = batch_frames(name, counts)
    st = torch.cuda.Stream()
    G = Vocabulary.from_arrays(B.vocab(name).arrays(), stream=st.cuda_stream)
    try:
        torch.cuda.synchronize()
        out = G.transform_batch_dev(desc_frames_dev(n_dev, desc_dev), 2)
        st.synchronize()
        host = {k: v.cpu().numpy() for k, v in out.items()}
        for b, d in enumerate(sets):
            one = G.transform(d, 2)
            nw, nn = int(host["n_words"][b]), int(host["n_nodes"][b])
            got = dict(words=host["words"][b, :nw], values=host["values"][b, :nw], node_id=host["node_id"][b, :nn].astype(np.uint32),
                       node_start=host["node_start"][b, : nn + 1], features=host["features"][b, : host["node_start"][b, nn]],
                       word_of_feature=host["word_of_feature"][b, : len(d)], node_of_feature=host["node_of_feature"][b, : len(d)])
            assert_transform_equal(got, one, ("batch", b))
            assert got["values"].tobytes() == one["values"].tobytes()  # the same kernels: the same bits
            assert (host["word_of_feature"][b, len(d):] == -1).all() and (host["node_of_feature"][b, len(d):] == 0).all()
            assert_transform_equal(got, B.transform(B.vocab(name), d, 2), ("batch vs restatement", b))
    finally:
        G.close()


def test_score_equals_the_restatement(vocabs):
    V, G = B.vocab("k4_L6"), vocabs("k4_L6")
    rows = B.db_rows(65)
    ids = sorted(rows)
    for a, b in ((0, 1), (0, 7), (3, 3), (10, 64)):
        assert abs(G.score(rows[ids[a]], rows[ids[b]]) - B.score(rows[ids[a]], rows[ids[b]])) <= TOL


# ------------------------------------------------------------------------------------------------------------------------------------
# database
# ------------------------------------------------------------------------------------------------------------------------------------
def check_query(db, rows, case):
    name, q, exclude, swr, sr, ms, mc = case
    want = B.query(rows, q, exclude, swr, sr, ms, mc)
    # the precondition, on the restatement alone: no scored keyframe within 1e-9 of a step-5 threshold, nor of another one's score
    # unless their rows are identical (the deliberate exact ties)
    assert B.query_margin(want, rows) > 1e-9, (name, B.query_margin(want, rows))
    ids, scores, common = db.query(q[0], q[1], exclude, swr, sr, ms, mc)
    assert ids.tolist() == want["ids"].tolist(), name
    assert common.tolist() == want["common"].tolist(), name
    worst = float(np.abs(scores - want["scores"]).max()) if len(ids) else 0.0
    assert worst <= TOL, (name, worst)
    return worst


@pytest.mark.parametrize("n_kf", B.DB_SIZES)
def test_database_queries_equal_the_restatement(vocabs, n_kf):
    from snake_slam_amd.bow import KeyframeDatabase

    rows = B.db_rows(n_kf)
    db = KeyframeDatabase(vocabs(B.DB_VOCAB), max_keyframes=max(n_kf, 1) + 4, max_words=64)
    try:
        for k in sorted(rows):
            db.add(k, *rows[k])
        worst = 0.0
        for case in B.db_queries(n_kf):
            worst = max(worst, check_query(db, rows, case))
        print(f"{n_kf} keyframes: largest score difference to the restatement {worst:.2e}")
    finally:
        db.close()


def test_database_remove_readd_ties_and_errors(vocabs):
    from snake_slam_amd import SnakeHipError
    from snake_slam_amd.bow import KeyframeDatabase

    rows = dict(B.db_rows(65))
    ids = sorted(rows)
    db = KeyframeDatabase(vocabs(B.DB_VOCAB), max_keyframes=70, max_words=64)
    try:
        for k in ids:
            db.add(k, *rows[k])
        q = B.db_fresh_query(65, 0)
        wide = ("wide", q, (), 0.0, 0.0, 0.0, 64)
        first = B.query(rows, q, (), 0.8, 0.75, 0.0, 10)["ids"]
        # remove the best candidates: they must be gone, the rest keeps its order
        for k in first[:2]:
            db.remove(int(k))
            del rows[int(k)]
        check_query(db, rows, ("after_remove", q, (), 0.8, 0.75, 0.0, 10))
        check_query(db, rows, wide)
        # errors are codes, and change nothing
        with pytest.raises(SnakeHipError):
            db.remove(int(first[0]))  # absent
        with pytest.raises(SnakeHipError):
            db.add(ids[-1], *rows[ids[-1]])  # twice
        with pytest.raises(SnakeHipError):
            db.add(10 ** 6, rows[ids[-1]][0][::-1], rows[ids[-1]][1])  # words not ascending
        check_query(db, rows, wide)
        # the removed id comes back with ANOTHER row (its slot is reused), and a second keyframe with an identical row under a lower id
        again = rows[ids[-1]]
        db.add(int(first[0]), *again)
        rows[int(first[0])] = again
        db.add(1, *again)  # ids are 5 i + 3: 1 is the lowest of all
        rows[1] = again
        res = B.query(rows, again, (), 0.8, 0.75, 0.0, 10)
        assert res["ids"][0] == 1 and len({float(s) for s in res["scores"][:3]}) == 1  # three identical rows: an exact tie, lowest id first
        check_query(db, rows, ("ties", again, (), 0.8, 0.75, 0.0, 10))
        check_query(db, rows, ("ties_top1", again, (), 0.8, 0.75, 0.0, 1))
        check_query(db, rows, ("ties_top2", again, (), 0.8, 0.75, 0.0, 2))
        check_query(db, rows, wide)
        # full: 65 - 2 + 2 = 65 stored of 70
        for k in range(5):
            db.add(2000 + k, *again)
            rows[2000 + k] = again
        with pytest.raises(SnakeHipError):
            db.add(3000, *again)
        check_query(db, rows, ("full", again, (1,), 0.8, 0.75, 0.0, 64))
    finally:
        db.close()


def test_batched_queries_equal_the_single_calls(vocabs):
    import torch

    from snake_slam_amd.bow import KeyframeDatabase, Vocabulary

    n_kf, Q, cap, ecap, mc = 300, 7, 64, 8, 10
    rows = B.db_rows(n_kf)
    ids = sorted(rows)
    queries = [B.db_fresh_query(n_kf, k) for k in (0, 50, 100, 299)] + [rows[ids[5]], B.db_unused_words(rows), (np.zeros(0, np.int32), np.zeros(0))]
    excludes = [(), tuple(ids[:8]), (), (ids[299],), (ids[5],), (), ()]
    words, values = np.full((Q, cap), -5, np.int32), np.full((Q, cap), np.nan)
    ex, n_ex = np.full((Q, ecap), -1, np.int32), np.zeros(Q, np.int32)
    for i, (q, e) in enumerate(zip(queries, excludes)):
        words[i, : len(q[0])], values[i, : len(q[0])] = q[0], q[1]
        ex[i, : len(e)], n_ex[i] = e, len(e)
    n_w = np.array([len(q[0]) for q in queries], np.int32)
    st = torch.cuda.Stream()
    G = Vocabulary.from_arrays(B.vocab(B.DB_VOCAB).arrays(), stream=st.cuda_stream)
    db = KeyframeDatabase(G, max_keyframes=n_kf, max_words=64)
    try:
        for k in ids:
            db.add(k, *rows[k])
        t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
        D = [t(words), t(values), t(n_w), t(ex), t(n_ex)]
        torch.cuda.synchronize()
        out = db.query_batch_dev(D[0], D[1], D[2], D[3], D[4], 0.8, 0.75, 0.0, mc)
        st.synchronize()
        got = {k: v.cpu().numpy() for k, v in out.items()}
        for i, (q, e) in enumerate(zip(queries, excludes)):
            one = db.query(q[0], q[1], e, 0.8, 0.75, 0.0, mc)
            k = int(got["n"][i])
            assert got["ids"][i, :k].tolist() == one[0].tolist() and got["common"][i, :k].tolist() == one[2].tolist(), i
            assert got["scores"][i, :k].tobytes() == one[1].tobytes(), i
            want = B.query(rows, q, e, 0.8, 0.75, 0.0, mc)
            assert B.query_margin(want, rows) > 1e-9
            assert one[0].tolist() == want["ids"].tolist(), i
        assert int(got["n"][0]) > 0 and int(got["n"][5]) == 0 and int(got["n"][6]) == 0
    finally:
        db.close()
        G.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# MatchBoW
# ------------------------------------------------------------------------------------------------------------------------------------
MATCH_CASES = B.match_cases()


@pytest.fixture(scope="module")
def matcher():
    from snake_slam_amd.bow import LoopMatcher

    m = LoopMatcher()
    yield m
    m.close()


@pytest.mark.parametrize("case", MATCH_CASES, ids=[c[0] for c in MATCH_CASES])
def test_match_bow_equals_the_restatement(matcher, case):
    name, s, th, ratio = case
    want, n = B.match_bow(s["desc1"], s["has1"], s["bow1"], s["desc2"], s["has2"], s["bow2"], th, ratio)
    got, k = matcher.match_bow(s["desc1"], s["has1"], s["bow1"], s["desc2"], s["has2"], s["bow2"], th, ratio)
    assert np.array_equal(got, want) and k == n, name


def test_match_bow_batch_equals_the_host_form(matcher):
    import torch

    from snake_slam_amd.bow import LoopMatcher, desc_frames_dev

    scenes = [c for c in MATCH_CASES if c[0] in ("scene_k10_L3_300", "list_70", "list_0", "scene_irregular_257", "competing")]
    Bn, cap1, cap2 = len(scenes), 320, 300
    A = {k: np.zeros((Bn, c, 4), np.uint64) for k, c in (("desc1", cap1), ("desc2", cap2))}
    H = {k: np.zeros((Bn, c), np.uint8) for k, c in (("has1", cap1), ("has2", cap2))}
    bow = {s: dict(node_id=np.zeros((Bn, c), np.int32), node_start=np.zeros((Bn, c + 1), np.int32), features=np.zeros((Bn, c), np.int32),
                   n_nodes=np.zeros(Bn, np.int32)) for s, c in (("1", cap1), ("2", cap2))}
    n = {"1": np.zeros(Bn, np.int32), "2": np.zeros(Bn, np.int32)}
    for b, (_, s, _, _) in enumerate(scenes):
        for side in "12":
            d = s["desc" + side]
            A["desc" + side][b, : len(d)], H["has" + side][b, : len(d)], n[side][b] = d, s["has" + side], len(d)
            nid, ns, ft = s["bow" + side]
            w = bow[side]
            w["node_id"][b, : len(nid)], w["node_start"][b, : len(ns)], w["features"][b, : len(ft)], w["n_nodes"][b] = nid, ns, ft, len(nid)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    st = torch.cuda.Stream()
    m = LoopMatcher(stream=st.cuda_stream)
    try:
        D = {k: t(v.view(np.int64)) for k, v in A.items()}
        Hd = {k: t(v) for k, v in H.items()}
        bd = {s: {k: t(v) for k, v in w.items()} for s, w in bow.items()}
        nd = {s: t(v) for s, v in n.items()}
        m12 = torch.full((Bn, cap1), -9, dtype=torch.int32, device="cuda")
        pairs, n_pairs = torch.full((Bn, cap1, 2), -9, dtype=torch.int32, device="cuda"), torch.full((Bn,), -9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        m.match_bow_batch_dev(desc_frames_dev(nd["1"], D["desc1"]), desc_frames_dev(nd["2"], D["desc2"]), Hd["has1"], Hd["has2"], bd["1"], bd["2"],
                              m12, pairs, n_pairs, 50, 0.75)
        st.synchronize()
        m12, pairs, n_pairs = m12.cpu().numpy(), pairs.cpu().numpy(), n_pairs.cpu().numpy()
        for b, (name, s, _, _) in enumerate(scenes):
            want, k = matcher.match_bow(s["desc1"], s["has1"], s["bow1"], s["desc2"], s["has2"], s["bow2"], 50, 0.75)
            assert np.array_equal(m12[b, : len(want)], want) and (m12[b, len(want):] == -1).all(), name
            f1 = np.nonzero(want >= 0)[0]
            assert n_pairs[b] == k and np.array_equal(pairs[b, :k, 0], f1) and np.array_equal(pairs[b, :k, 1], want[f1]), name
    finally:
        m.close()
