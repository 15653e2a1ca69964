"""An independent numpy restatement of "snk-bow v1"  and a seeded generator of synthetic vocabularies and scenes.

The restatement is written from the definitions, not from the kernels: descents by ``argmin`` over a node's children (numpy's argmin
returns the first minimum), bow vectors by ``np.unique``, the score over ``np.intersect1d``, the query as the seven steps of the
definition with numpy scalars of the stated types, MatchBoW by a stable sort of each feature's candidate distances.  The GPU tests, the
CPU build of bow_core.hpp and the brute-force transcriptions of tests/test_bow_numpy.py are all compared against it.
"""
from __future__ import annotations

import numpy as np

POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


def hamming(a, B):
    """distances of descriptor a [4] uint64 to the rows of B [m, 4] uint64"""
    x = np.bitwise_xor(np.asarray(a, np.uint64).reshape(1, 4), np.asarray(B, np.uint64).reshape(-1, 4))
    return POP8[np.ascontiguousarray(x).view(np.uint8)].sum(axis=1)


def flip_bits(rng, d, k):
    """descriptor d with k distinct random bits flipped"""
    bits = np.unpackbits(np.asarray(d, np.uint64).reshape(4).view(np.uint8))
    idx = rng.choice(256, size=int(k), replace=False)
    bits[idx] ^= 1
    return np.packbits(bits).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------------------------------
# vocabularies
# ------------------------------------------------------------------------------------------------------------------------------------
class Vocab:
    """Flat arrays as snk_bow_vocab_create takes them, numbered breadth first (parents before children, word ids in leaf order)."""

    def __init__(self, child_start, child_count, children, desc, word_id, weight):
        self.child_start = np.asarray(child_start, np.int32)
        self.child_count = np.asarray(child_count, np.int32)
        self.children = np.asarray(children, np.int32)
        self.desc = np.asarray(desc, np.uint64).reshape(-1, 4)
        self.word_id = np.asarray(word_id, np.int32)
        self.weight = np.asarray(weight, np.float64)
        n = len(self.child_start)
        self.depth_of = np.zeros(n, np.int64)
        for i in range(n):  # breadth-first numbering: a parent's depth is known before its children's
            self.depth_of[self.kids(i)] = self.depth_of[i] + 1
        self.L = int(self.depth_of[self.child_count == 0].max())
        self.n_words = int((self.child_count == 0).sum())
        self.word_weight = np.zeros(self.n_words)
        leaves = np.nonzero(self.child_count == 0)[0]
        self.word_weight[self.word_id[leaves]] = self.weight[leaves]

    def kids(self, i):
        return self.children[self.child_start[i]: self.child_start[i] + self.child_count[i]]

    def arrays(self) -> dict:
        return dict(child_start=self.child_start, child_count=self.child_count, children=self.children, desc=self.desc, word_id=self.word_id,
                    weight=self.weight)


def build_vocab(rng, n_children, twin_children=False) -> Vocab:
    """Breadth-first growth: ``n_children(depth, index)`` children for the node (0 = leaf).  A child is its parent's descriptor with
    96 >> depth (at least 6) bits flipped -- hierarchical bit flipping, so that descents are decided late --; with ``twin_children`` the
    second child of every node is a copy of the first and the last a copy of the one before it: exact ties at every level."""
    desc = [rng.integers(0, 2 ** 64, 4, dtype=np.uint64)]
    depth, counts, starts, children = [0], [], [], []
    i = 0
    while i < len(desc):
        k = int(n_children(depth[i], i))
        counts.append(k)
        starts.append(len(children))
        for c in range(k):
            children.append(len(desc))
            if twin_children and c in (1, k - 1) and c > 0:
                desc.append(desc[-1].copy())
            else:
                desc.append(flip_bits(rng, desc[i], max(6, 96 >> depth[i])))
            depth.append(depth[i] + 1)
        i += 1
    counts = np.array(counts, np.int32)
    word_id = np.full(len(desc), -1, np.int32)
    word_id[counts == 0] = np.arange(int((counts == 0).sum()), dtype=np.int32)
    weight = np.where(counts == 0, rng.uniform(0.5, 9.0, len(desc)), 0.0)
    return Vocab(starts, counts, children, np.array(desc), word_id, weight)


def vocab_regular(seed, k, L, twins=False) -> Vocab:
    return build_vocab(np.random.default_rng(seed), lambda d, i: k if d < L else 0, twins)


def vocab_irregular(seed) -> Vocab:
    """2-20 children (the root has 20: the stride past 16 lanes is taken at the first step; another node of 17), leaves at depths 1-5"""
    rng = np.random.default_rng(seed)

    def n_children(d, i):
        if i == 0:
            return 20
        if i == 2:
            return 17
        if i == 1 or d >= 5:
            return 0  # node 1: a leaf at depth 1
        if d >= 2 and rng.random() < 0.35:
            return 0
        return int(rng.integers(2, 8)) if d >= 2 else int(rng.integers(2, 21))

    return build_vocab(rng, n_children)


def hand_vocab() -> Vocab:
    """2 levels, 3 children each, descriptors chosen by hand (tests/test_bow_numpy.py derives the answers in its comments):
    level 1: A = 0...0, B = low 64 bits set, C = all 256 bits set; the children of X are X with 0, 1, 2 of the top bits of word 3 flipped."""
    z, f = np.uint64(0), np.uint64(0xFFFFFFFFFFFFFFFF)
    lvl1 = [np.array([z, z, z, z]), np.array([f, z, z, z]), np.array([f, f, f, f])]
    desc = [np.array([z, z, z, z])] + lvl1
    for p in lvl1:
        for t in (0, 1, 3):  # top bits of word 3: none, bit 62, bits 62 and 63
            d = p.copy()
            d[3] ^= np.uint64(t) << np.uint64(62)
            desc.append(d)
    counts = [3, 3, 3, 3] + [0] * 9
    starts = [0, 3, 6, 9] + [0] * 9
    children = list(range(1, 13))
    word_id = [-1] * 4 + list(range(9))
    weight = [0.0] * 4 + [1.0, 2.0, 3.0, 1.0, 1.0, 1.0, 4.0, 0.5, 0.25]
    return Vocab(starts, counts, children, np.array(desc), word_id, weight)


# ------------------------------------------------------------------------------------------------------------------------------------
# transform
# ------------------------------------------------------------------------------------------------------------------------------------
def descend(V: Vocab, d):
    """the path of descriptor d: node ids from the root to the leaf"""
    path, node = [0], 0
    while V.child_count[node] > 0:
        ch = V.kids(node)
        node = int(ch[int(np.argmin(hamming(d, V.desc[ch])))])  # argmin: the first child of minimal distance
        path.append(node)
    return path


def node_up(V: Vocab, path, levelsup):
    t = V.L - int(levelsup)
    return path[t] if 0 < t < len(path) else 0


def transform(V: Vocab, descs, levelsup, paths=None) -> dict:
    descs = np.asarray(descs, np.uint64).reshape(-1, 4)
    paths = [descend(V, d) for d in descs] if paths is None else paths
    wof = np.array([V.word_id[p[-1]] for p in paths], np.int32).reshape(-1)
    nof = np.array([node_up(V, p, levelsup) for p in paths], np.int32).reshape(-1)
    words, counts = np.unique(wof, return_counts=True)
    values = counts * V.word_weight[words] if len(words) else np.zeros(0)
    norm = float(values.sum())
    if norm > 0.0:
        values = values / norm
    else:
        words, values = np.zeros(0, np.int32), np.zeros(0)
    node_id = np.unique(nof[nof > 0])
    feats = [np.nonzero(nof == n)[0] for n in node_id]
    node_start = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int32)
    return dict(words=words.astype(np.int32), values=np.asarray(values, np.float64), node_id=node_id.astype(np.uint32), node_start=node_start,
                features=(np.concatenate(feats) if feats else np.zeros(0)).astype(np.int32), word_of_feature=wof, node_of_feature=nof)


def score(a, b) -> float:
    """L1 score of two bow vectors (words, values)"""
    _, ia, ib = np.intersect1d(a[0], b[0], assume_unique=True, return_indices=True)
    x, y = np.asarray(a[1], np.float64)[ia], np.asarray(b[1], np.float64)[ib]
    return float(-0.5 * np.sum(np.abs(x - y) - x - y))


# ------------------------------------------------------------------------------------------------------------------------------------
# database query
# ------------------------------------------------------------------------------------------------------------------------------------
def query(rows: dict, q, exclude=(), sharing_word_ratio=0.8, score_ratio=0.75, min_score=0.0, max_candidates=10) -> dict:
    """rows: {keyframe id: (words, values)} of the live keyframes.  Returns ids / scores / common of the candidates in order, and for
    the margin precondition of the GPU test: every scored keyframe's score (``scored``) and the two thresholds of step 5."""
    swr, sr, ms = np.float32(sharing_word_ratio), np.float32(score_ratio), np.float32(min_score)
    common = {k: len(np.intersect1d(q[0], r[0], assume_unique=True)) for k, r in rows.items() if k not in set(int(e) for e in exclude)}
    common = {k: c for k, c in common.items() if c >= 1}  # step 1
    empty = dict(ids=np.zeros(0, np.int32), scores=np.zeros(0), common=np.zeros(0, np.int32), scored={}, thresholds=(0.0, float(ms)))
    if not common:
        return empty
    max_common = max(common.values())  # step 2
    kept = [k for k, c in common.items() if not (np.float32(c) < swr * np.float32(max_common))]  # step 3, float
    scored = {k: score(q, rows[k]) for k in kept}  # step 4
    best = max([0.0] + list(scored.values()))
    t_ratio, t_min = float(sr) * best, float(ms)
    final = [k for k in kept if not (scored[k] < t_ratio or scored[k] < t_min)]  # step 5, double
    final.sort(key=lambda k: (-scored[k], k))  # step 6
    final = final[: int(max_candidates)]  # step 7
    return dict(ids=np.array(final, np.int32), scores=np.array([scored[k] for k in final], np.float64),
                common=np.array([common[k] for k in final], np.int32), scored=scored, thresholds=(t_ratio, t_min))


def query_margin(res: dict, rows: dict | None = None) -> float:
    """What keeps a candidate list independent of the summation order: the smallest distance of a scored keyframe's score to one of the
    step-5 thresholds, and -- the order of step 6 compares scores with each other -- the smallest difference between the scores of two
    scored keyframes, not counting keyframes whose rows are identical (given ``rows``): those tie exactly in any arithmetic, and the id
    decides.  inf when nothing was scored."""
    if not res["scored"]:
        return float("inf")
    keys = sorted(res["scored"], key=lambda k: res["scored"][k])
    s = np.array([res["scored"][k] for k in keys])
    margin = float(min(np.abs(s - res["thresholds"][0]).min(), np.abs(s - res["thresholds"][1]).min()))
    for a, b in zip(keys[:-1], keys[1:]):
        same = rows is not None and np.array_equal(rows[a][0], rows[b][0]) and np.array_equal(rows[a][1], rows[b][1])
        if not same:
            margin = min(margin, abs(res["scored"][b] - res["scored"][a]))
    return margin


# ------------------------------------------------------------------------------------------------------------------------------------
# MatchBoW
# ------------------------------------------------------------------------------------------------------------------------------------
def match_bow(desc1, has1, bow1, desc2, has2, bow2, threshold=50, ratio=0.75):
    """bow = (node_id, node_start, features).  Returns (match12, n)"""
    desc1, desc2 = np.asarray(desc1, np.uint64).reshape(-1, 4), np.asarray(desc2, np.uint64).reshape(-1, 4)
    m12 = np.full(len(desc1), -1, np.int32)
    matched = np.zeros(len(desc2), bool)
    has1, has2 = np.asarray(has1).astype(bool), np.asarray(has2).astype(bool)
    _, i1, i2 = np.intersect1d(np.asarray(bow1[0], np.int64), np.asarray(bow2[0], np.int64), assume_unique=True, return_indices=True)
    for a, b in zip(i1, i2):
        l1 = np.asarray(bow1[2])[bow1[1][a]: bow1[1][a + 1]]
        l2 = np.asarray(bow2[2])[bow2[1][b]: bow2[1][b + 1]]
        for f1 in l1:
            if not has1[f1]:
                continue
            cand = l2[has2[l2] & ~matched[l2]]
            if len(cand) == 0:
                continue
            dist = hamming(desc1[f1], desc2[cand])
            order = np.argsort(dist, kind="stable")
            d1 = int(dist[order[0]])
            d2 = int(dist[order[1]]) if len(cand) > 1 else 256
            if d1 < int(threshold) and np.float32(d1) < np.float32(ratio) * np.float32(d2):
                matched[cand[order[0]]] = True
                m12[f1] = cand[order[0]]
    return m12, int((m12 >= 0).sum())


# ------------------------------------------------------------------------------------------------------------------------------------
# scenes and the cases shared by the GPU tests and the CPU build of bow_core.hpp
# ------------------------------------------------------------------------------------------------------------------------------------
def leaf_descriptors(V: Vocab, rng, n, flips=4, pool=None):
    """n descriptors: a leaf's descriptor (drawn from ``pool`` of node ids, default all leaves) with ``flips`` bits flipped"""
    leaves = np.nonzero(V.child_count == 0)[0] if pool is None else np.asarray(pool)
    pick = rng.choice(leaves, size=int(n))
    return np.array([flip_bits(rng, V.desc[p], flips) for p in pick], np.uint64).reshape(-1, 4)


VOCABS = {"k10_L3": lambda: vocab_regular(11, 10, 3), "k4_L6": lambda: vocab_regular(12, 4, 6), "irregular": lambda: vocab_irregular(13),
          "single_level": lambda: vocab_regular(14, 12, 1), "twins_k4_L3": lambda: vocab_regular(15, 4, 3, True)}
_vocab_cache: dict = {}


def vocab(name) -> Vocab:
    if name not in _vocab_cache:
        _vocab_cache[name] = VOCABS[name]()
    return _vocab_cache[name]


FEATURE_COUNTS = (0, 1, 15, 16, 17, 63, 64, 65, 1000, 2048)


def levelsups(V: Vocab):
    return sorted({0, 2, 4, V.L, V.L + 1})


def frame_descriptors(name, n, seed=0):
    V = vocab(name)
    return leaf_descriptors(V, np.random.default_rng(1000 + 7 * n + seed), n, flips=5)


def tie_descriptors(name="twins_k4_L3", n=40):
    """descriptors of the twin vocabulary's duplicated children themselves: equidistant (distance 0 or a few bits) from two children at
    every level, so only the first-child rule decides"""
    V = vocab(name)
    rng = np.random.default_rng(77)
    twins = [int(V.kids(i)[1]) for i in range(len(V.child_count)) if V.child_count[i] > 1] + \
            [int(V.kids(i)[-1]) for i in range(len(V.child_count)) if V.child_count[i] > 1]
    pick = rng.choice(np.array(twins), size=n)
    out = V.desc[pick].copy()
    for i in range(0, n, 2):  # half of them moved off the node a little: still equidistant from both twins
        out[i] = flip_bits(rng, out[i], 3)
    return out


def crowd_descriptors(name, distinct: bool, n=64):
    """all features in one word / every feature in its own word (the leaves' own descriptors)"""
    V = vocab(name)
    leaves = np.nonzero(V.child_count == 0)[0]
    return V.desc[leaves[:n]].copy() if distinct else np.repeat(V.desc[leaves[5:6]], n, axis=0)


def place_keyframes(name, n_places, per_place, n_feat, seed, world=None):
    """keyframes of ``n_places`` places: a place owns a pool of leaves; its keyframes draw from the pool, so they share words.  Place p
    and its keyframe j depend on (seed, p, j) only, so asking for more keyframes per place leaves the earlier ones as they are.  With
    ``world`` the pools are drawn from that many leaves only, so keyframes of different places share a few words too."""
    V = vocab(name)
    leaves = np.nonzero(V.child_count == 0)[0]
    leaves = leaves if world is None else leaves[:: max(1, len(leaves) // world)][:world]
    out = []
    for p in range(n_places):
        pool = np.random.default_rng([seed, p]).choice(leaves, size=min(len(leaves), max(8, n_feat // 2)), replace=False)
        for j in range(per_place):
            out.append(leaf_descriptors(V, np.random.default_rng([seed, p, j]), n_feat, flips=3, pool=pool))
    return out


def match_scene(name, seed, n1, n2, levelsup, shared=0.7, missing=0.2, flips=6):
    """two keyframes of one place: keyframe 2 holds noisy copies of a share of keyframe 1's descriptors; some features have no point"""
    V = vocab(name)
    rng = np.random.default_rng(seed)
    d1 = leaf_descriptors(V, rng, n1, flips=3)
    d2 = leaf_descriptors(V, rng, n2, flips=3)
    k = min(int(shared * min(n1, n2)), n1, n2)
    if k:
        src = rng.choice(n1, size=k, replace=False)
        dst = rng.choice(n2, size=k, replace=False)
        for s, t in zip(src, dst):
            d2[t] = flip_bits(rng, d1[s], flips)
    has1 = (rng.random(n1) >= missing).astype(np.uint8)
    has2 = (rng.random(n2) >= missing).astype(np.uint8)
    t1, t2 = transform(V, d1, levelsup), transform(V, d2, levelsup)
    return dict(desc1=d1, desc2=d2, has1=has1, has2=has2, bow1=(t1["node_id"], t1["node_start"], t1["features"]),
                bow2=(t2["node_id"], t2["node_start"], t2["features"]))


def one_node_scene(d1, d2, has1, has2):
    """hand-made MatchBoW cases: every feature of either keyframe in node 7"""
    d1, d2 = np.asarray(d1, np.uint64).reshape(-1, 4), np.asarray(d2, np.uint64).reshape(-1, 4)
    mk = lambda n: (np.array([7], np.uint32), np.array([0, n], np.int32), np.arange(n, dtype=np.int32))
    return dict(desc1=d1, desc2=d2, has1=np.asarray(has1, np.uint8), has2=np.asarray(has2, np.uint8), bow1=mk(len(d1)), bow2=mk(len(d2)))


def match_cases():
    """(name, scene, threshold, ratio) of the MatchBoW tests"""
    rng = np.random.default_rng(5)
    base = rng.integers(0, 2 ** 62, (8, 4)).astype(np.uint64)
    near = lambda d, k, s: flip_bits(np.random.default_rng(s), d, k)
    cases = []
    for n_list in (0, 1, 17, 70):  # keyframe-2 lists of that length in one node (70: longer than a wavefront)
        d2 = np.array([near(base[0], 20 + (i * 7) % 30, i) for i in range(n_list)], np.uint64).reshape(-1, 4)
        d1 = np.array([near(base[0], 4, 100 + i) for i in range(max(n_list, 1))], np.uint64).reshape(-1, 4)
        if n_list:
            d2[n_list // 2] = near(d1[0], 2, 9)
            d2[n_list - 1] = near(d1[-1], 1, 10)
        cases.append((f"list_{n_list}", one_node_scene(d1, d2, np.ones(len(d1)), np.ones(len(d2))), 50, 0.75))
    d2 = np.array([near(base[1], 3, i) for i in range(9)])
    cases.append(("kf2_without_points", one_node_scene(d2[:4], d2, np.ones(4), np.zeros(9)), 50, 0.75))
    dup = np.array([near(base[2], 40, 1), near(base[2], 2, 2), near(base[2], 2, 2), near(base[2], 60, 3)])
    cases.append(("duplicate_best", one_node_scene(base[2:3], dup, [1], [1, 1, 1, 1]), 50, 0.75))  # second best == best: the ratio rejects
    comp2 = np.array([near(base[3], 90, 1), near(base[3], 1, 2), near(base[3], 100, 3)])
    comp1 = np.array([near(base[3], 2, 4), base[3], near(base[3], 3, 5)])
    cases.append(("competing", one_node_scene(comp1, comp2, [1, 1, 1], [1, 1, 1]), 50, 0.75))  # the first takes feature 1, the others see it matched
    exact = np.array([near(base[4], 12, 1), near(base[4], 120, 2)])
    cases.append(("threshold_equal", one_node_scene(base[4:5], exact, [1], [1, 1]), 12, 0.75))  # best == threshold: strict <
    cases.append(("threshold_above", one_node_scene(base[4:5], exact, [1], [1, 1]), 13, 0.75))
    for seed, (n1, n2, name, lv) in enumerate([(300, 280, "k10_L3", 1), (2048, 2048, "k4_L6", 4), (257, 190, "irregular", 2), (64, 65, "k4_L6", 5)]):
        cases.append((f"scene_{name}_{n1}", match_scene(name, 40 + seed, n1, n2, lv), 50, 0.75))
    return cases


# ------------------------------------------------------------------------------------------------------------------------------------
# database scenarios (tests/test_bow_gpu.py; their margins are checked on the CPU by tests/test_bow_numpy.py)
# ------------------------------------------------------------------------------------------------------------------------------------
DB_VOCAB, DB_LEVELSUP, DB_SIZES = "k4_L6", 4, (0, 1, 2, 65, 300)
_db_cache: dict = {}


def db_rows(n_kf):
    """{keyframe id: (words, values)} of n_kf keyframes of ceil(n_kf / 6) places, ids 5 i + 3; and the descriptor sets"""
    if n_kf not in _db_cache:
        V = vocab(DB_VOCAB)
        frames = place_keyframes(DB_VOCAB, (n_kf + 5) // 6, 6, 40, 902, world=40)[:n_kf]
        rows = {}
        for i, d in enumerate(frames):
            t = transform(V, d, DB_LEVELSUP)
            rows[5 * i + 3] = (t["words"], t["values"])
        _db_cache[n_kf] = rows
    return _db_cache[n_kf]


def db_fresh_query(n_kf, k):
    """the bow vector of a new view of the place of stored keyframe number k: other noise, other draws from the same pool"""
    V = vocab(DB_VOCAB)
    places = place_keyframes(DB_VOCAB, (max(n_kf, 1) + 5) // 6, 7, 40, 902, world=40)  # the same pools, a seventh keyframe per place
    t = transform(V, places[(k // 6) * 7 + 6], DB_LEVELSUP)
    return t["words"], t["values"]


def db_unused_words(rows, n=5):
    used = set()
    for w, _ in rows.values():
        used.update(int(x) for x in w)
    free = [w for w in range(vocab(DB_VOCAB).n_words) if w not in used][:n]
    return np.array(free, np.int32), np.full(len(free), 1.0 / max(len(free), 1))


def db_queries(n_kf):
    """(name, query, exclude, sharing_word_ratio, score_ratio, min_score, max_candidates) against db_rows(n_kf)"""
    rows = db_rows(n_kf)
    ids = sorted(rows)
    out = [("no_common_word", db_unused_words(rows), (), 0.8, 0.75, 0.0, 10),
           ("empty_query", (np.zeros(0, np.int32), np.zeros(0)), (), 0.8, 0.75, 0.0, 10)]
    for k in sorted({0, n_kf // 2, n_kf - 1} & set(range(n_kf))):
        q = db_fresh_query(n_kf, k)
        out.append((f"fresh_{k}_default", q, (), 0.8, 0.75, 0.0, 10))
        for mc in (1, 2, 10, 64):
            out.append((f"fresh_{k}_wide_{mc}", q, (), 0.0, 0.0, 0.0, mc))
        out.append((f"fresh_{k}_loose", q, (), 0.5, 0.4, 0.02, 64))
        best = query(rows, q, (), 0.8, 0.75, 0.0, 10)["ids"]
        out.append((f"fresh_{k}_exclude_best", q, tuple(best[:1]) + tuple(ids[:3]), 0.8, 0.75, 0.0, 10))
        out.append((f"fresh_{k}_min_score_above_all", q, (), 0.8, 0.75, 0.999, 10))
        out.append((f"own_row_{k}", rows[ids[k]], (), 0.8, 0.75, 0.0, 10))
    return out
