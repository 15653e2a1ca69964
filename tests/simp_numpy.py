"""Simplification::KeyFrameCullingGraph and Redundancy (reference Snake/Optimizer/Simplification.cpp:148-358, :75-146), Keyframe::MatchCount
and ComputeDepthRange (reference Snake/Map/Keyframe.cpp:68-77, :175-206) restated statement by statement as loops over Python lists and
dictionaries -- an id_map dictionary, an edge dictionary, a sort for the median, an O(n^2) Prim over Python lists -- so that it shares no
method with the kernels of snake_slam_amd/csrc/simp.hip or with simp_core.hpp.  Semantics "snk-simp v1" (DESIGN.md section 3l); the graph
rules are [DEFINED] there (saiga's WeightedUndirectedGraph is absent from the reference checkout).

``stats_fixture`` / ``decide_fixture`` generate the tables of the tests; ``require_coverage`` raises unless every property those tests are
about occurs in them.
"""
import math
import struct

import numpy as np

import scene_numpy

OK, SKIPPED, FEAT_OVERFLOW, NODES_OVERFLOW, BAD_INDEX = range(5)
NONE, FACTOR, NO_CONN, ANGLE, MATCHES, REDUNDANCY, LINK, KEEP_IMU_WEIGHTS, KEEP_TIME_GAP, KEEP_BRANCH, KEEP_DISCONNECTED, KEEP_LINK = range(12)
CULLS = (FACTOR, NO_CONN, ANGLE, MATCHES, REDUNDANCY, LINK)
PT_BAD = 1
MAX_NODES, MAX_FEAT = 256, 16384
STATS_DTYPE = np.dtype([("median_depth", "<f4"), ("n_depth", "<i4"), ("match_count", "<i4"), ("n_mps", "<i4"), ("n_redundant", "<i4"),
                        ("redundancy", "<f4"), ("status", "<i4")])
VERDICT_DTYPE = np.dtype([("reason", "<i4"), ("cull", "<i4"), ("value", "<f8"), ("n_nodes", "<i4"), ("n_root_edges", "<i4"),
                          ("weakest_link", "<i4"), ("status", "<i4")])
CONN_DTYPE = np.dtype([("weight", "<i4"), ("kf", "<i4")])
PARAMS = dict(min_matches_in_graph=20, border_angle=1.0, border_redundancy=0.8, border_matches=80, th_map=140, with_imu=0, gyro_weight=0.0,
              acc_weight=0.0, max_time_between_kf=0.5)
PARAMS_DTYPE = np.dtype([("min_matches_in_graph", "<i4"), ("border_angle", "<f4"), ("border_redundancy", "<f4"), ("border_matches", "<i4"),
                         ("th_map", "<i4"), ("with_imu", "<i4"), ("gyro_weight", "<f8"), ("acc_weight", "<f8"), ("max_time_between_kf", "<f4"),
                         ("pad", "<i4")])  # snk_simp_params, 48 bytes


def params_record(params=None):
    rec = np.zeros(1, PARAMS_DTYPE)
    for k, v in dict(PARAMS, **(params or {})).items():
        rec[k] = v
    return rec


# the largest |angle(g++ build of simp_core.hpp) - angle(this file)| in degrees over the pairs of decide_fixture() and 2 000 random pairs
# of its keyframes, measured by test_simp_core_cpu.py (which fails if it grows): 2.132e-14, kept as 2.2e-14.  Two correct evaluations of
# the same formula (the camera centres by R^T t in numpy against the spelled-out sums, numpy's norm).  The GPU is allowed 10 x that.
ANGLE_FLOOR = 2.2e-14
ANGLE_BOUND = 10 * ANGLE_FLOOR


def bits(z):
    """The place of a float32 in the total order of the bit patterns (-0 before +0)."""
    u = struct.unpack("<I", struct.pack("<f", z))[0]
    return (~u & 0xFFFFFFFF) if u >> 31 else (u | 0x80000000)


def rotation(pose):
    x, y, z, w = (float(v) for v in pose[:4])
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def depth_of(pose, p):
    """Keyframe.cpp:193-194 in the operation order DESIGN.md section 3l states: float(((r20 px + r21 py) + r22 pz) + tz)."""
    x, y, z, w = (float(v) for v in pose[:4])
    r20, r21, r22 = 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)
    return np.float32(((r20 * float(p[0]) + r21 * float(p[1])) + r22 * float(p[2])) + float(pose[6]))


def stats(t, q, min_obs=3, stereo=1, th_depth=40.0, feat_cap=MAX_FEAT):
    """One record of STATS_DTYPE as a dict."""
    none = dict(median_depth=np.float32(-1), n_depth=0, match_count=0, n_mps=0, n_redundant=0, redundancy=np.float32(0))
    if t["kf_bad"][q]:  # Simplification.cpp:93
        return dict(none, status=SKIPPED)
    fs, fp = t["feat_start"], t["feat_point"]
    if fs[q + 1] - fs[q] > feat_cap:
        return dict(none, status=FEAT_OVERFLOW)
    n_obs_of = lambda mp: int(t["obs_start"][mp + 1] - t["obs_start"][mp])  # noqa: E731
    # Keyframe.cpp:183-205
    depths = []
    for i in range(fs[q], fs[q + 1]):
        if fp[i] >= 0:
            depths.append(depth_of(t["kf_pose"][q], t["pt_pos"][fp[i]]))
    median = np.float32(-1)
    if depths:
        depths.sort(key=bits)
        median = depths[(len(depths) - 1) // 2]
    # Keyframe.cpp:68-77
    c = 0
    for i in range(fs[q], fs[q + 1]):
        mp = fp[i]
        if mp >= 0 and not t["pt_flags"][mp] & PT_BAD and n_obs_of(mp) >= min_obs:
            c += 1
    # Simplification.cpp:98-145
    th_obs, n_redundant, n_mps = 3, 0, 0
    for i in range(fs[q], fs[q + 1]):
        mp = fp[i]
        if mp < 0 or t["pt_flags"][mp] & PT_BAD:
            continue
        if stereo and t["feat_depth"][i] > np.float32(th_depth):
            continue
        n_mps += 1
        if n_obs_of(mp) > th_obs:
            scale_level = int(t["feat_octave"][i])
            n = 0
            for o in range(t["obs_start"][mp], t["obs_start"][mp + 1]):
                kfi, fi = int(t["obs"][o][0]), int(t["obs"][o][1])
                if kfi == q:
                    continue
                if int(t["feat_octave"][fs[kfi] + fi]) <= scale_level + 1:
                    n += 1
                    if n >= th_obs:
                        break
            if n >= th_obs:
                n_redundant += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        redundancy = np.float32(n_redundant) / np.float32(n_mps)
    return dict(median_depth=median, n_depth=len(depths), match_count=c, n_mps=n_mps, n_redundant=n_redundant, redundancy=redundancy, status=OK)


def stats_array(rows):
    out = np.zeros(len(rows), STATS_DTYPE)
    for i, r in enumerate(rows):
        for k in STATS_DTYPE.names:
            out[k][i] = r[k]
    return out


# ---- the graph: [DEFINED] rules -----------------------------------------------------------------------------------------------------------

class Graph:
    """WeightedUndirectedGraph as DESIGN.md section 3l defines it: the maximum of the weights given for a pair, no self edges, the maximum
    spanning tree by Prim from node 0."""

    def __init__(self, n):
        self.n, self.w = n, {}

    def add_edge(self, a, b, weight):
        if a == b:
            return
        key = (min(a, b), max(a, b))
        self.w[key] = max(self.w.get(key, weight), weight)

    def weight(self, a, b):
        return self.w.get((min(a, b), max(a, b)))

    def build_mst(self):
        """Tree edges as (parent, child, weight) in the order of joining; the nodes that cannot be reached stay outside."""
        in_tree = [False] * self.n
        best = [None] * self.n  # (weight, parent) of every outside node
        in_tree[0] = True
        for v in range(1, self.n):
            if self.weight(0, v) is not None:
                best[v] = (self.weight(0, v), 0)
        self.mst = []
        while True:
            pick = None
            for v in range(self.n):
                if in_tree[v] or best[v] is None:
                    continue
                if pick is None or best[v][0] > best[pick][0]:  # the largest weight; v ascends, so the smallest id among equals
                    pick = v
            if pick is None:
                break
            in_tree[pick] = True
            self.mst.append((best[pick][1], pick, best[pick][0]))
            for u in range(self.n):
                w = self.weight(pick, u)
                if in_tree[u] or w is None:
                    continue
                if best[u] is None or w > best[u][0] or (w == best[u][0] and pick < best[u][1]):
                    best[u] = (w, pick)
        self.complete = all(in_tree)
        return self.mst

    def mst_edges_for_node(self, v):
        return [(a, b, w) if a == v else (b, a, w) for a, b, w in self.mst if v in (a, b)]

    def weakest(self):
        """The smallest tree edge; None ("invalid") if a node stayed outside."""
        return min(w for _, _, w in self.mst) if self.complete and self.mst else (None if not self.complete else 0)


def connections(g, k):
    return [(int(w), int(x)) for w, x in g["conn_list"][g["conn_start"][k]:g["conn_start"][k + 1]].tolist()]


def camera_position(pose):
    return -rotation(pose).T @ np.asarray(pose[4:7], np.float64)


def add_connections(graph, id_map, frm, conns):
    """The lambda of Simplification.cpp:186-200."""
    if frm not in id_map:
        return
    id_from = id_map[frm]
    for w, kf in conns:
        if kf not in id_map:
            continue
        graph.add_edge(id_from, id_map[kf], w)


def decide(g, q, st, params=None, node_cap=MAX_NODES):
    """One record of VERDICT_DTYPE as a dict (plus "angle" where it was computed).  st: q's stats record."""
    P = dict(PARAMS, **(params or {}))
    none = dict(reason=NONE, cull=0, value=0.0, n_nodes=0, n_root_edges=0, weakest_link=0)
    verdict = lambda reason, value=0.0, **kw: dict(none, reason=reason, cull=int(reason in CULLS), value=float(value), status=OK, **kw)  # noqa: E731
    if g["kf_bad"][q]:
        return dict(none, status=SKIPPED)
    if st["status"] != OK:
        return dict(none, status=int(st["status"]))
    factor = np.float32(g["kf_cull_factor"][q])
    if factor > 3:  # :150
        return verdict(FACTOR)
    if P["with_imu"]:  # :158-179
        if P["gyro_weight"] == 0 or P["acc_weight"] == 0:
            return verdict(KEEP_IMU_WEIGHTS)
        if g.get("kf_time") is not None and g["kf_prev"][q] >= 0 and g["kf_next"][q] >= 0:
            delta = float(g["kf_time"][g["kf_next"][q]]) - float(g["kf_time"][g["kf_prev"][q]])
            if delta > float(np.float32(P["max_time_between_kf"])):
                return verdict(KEEP_TIME_GAP)
    # :222-246
    conns = [c for c in connections(g, q) if not c[0] < P["min_matches_in_graph"]]
    n = len(conns) + 1
    if n > node_cap:
        return dict(none, status=NODES_OVERFLOW)
    id_to_keyframe, id_map = [q], {q: 0}
    for _, kf in conns:
        id_map[kf] = len(id_to_keyframe)
        id_to_keyframe.append(kf)
    graph = Graph(n)
    add_connections(graph, id_map, q, conns)
    for _, kf in conns:
        add_connections(graph, id_map, kf, connections(g, kf))
    graph.build_mst()
    mst_edges = graph.mst_edges_for_node(0)
    if not mst_edges:  # :256
        return verdict(NO_CONN, n_nodes=n)
    if len(mst_edges) == 1:  # :287-310
        other = id_to_keyframe[mst_edges[0][1]]
        depth = (float(g["kf_median_depth"][q]) + float(g["kf_median_depth"][other])) * 0.5
        baseline = float(np.linalg.norm(camera_position(g["kf_pose"][q]) - camera_position(g["kf_pose"][other])))
        angle = math.degrees(math.atan2(0.5 * baseline, depth) * 2.0)
        kw = dict(n_nodes=n, n_root_edges=1, angle=angle, other=other)
        if angle < float(np.float32(P["border_angle"]) * factor):
            return verdict(ANGLE, angle, **kw)
        if np.float32(st["match_count"]) < np.float32(P["border_matches"]) * factor:
            return verdict(MATCHES, st["match_count"], **kw)
        if np.float32(st["redundancy"]) > np.float32(P["border_redundancy"]):
            return verdict(REDUNDANCY, np.float32(st["redundancy"]), **kw)
        return verdict(KEEP_BRANCH, **kw)
    # :316-357
    kfs, local_id_map = [], {}
    for _, to, _ in sorted(mst_edges, key=lambda e: e[1]):
        local_id_map[id_to_keyframe[to]] = len(kfs)
        kfs.append(id_to_keyframe[to])
    graph2 = Graph(len(kfs))
    for kf in kfs:
        add_connections(graph2, local_id_map, kf, connections(g, kf))
    graph2.build_mst()
    weakest = graph2.weakest()
    kw = dict(n_nodes=n, n_root_edges=len(mst_edges))
    if weakest is None:  # :342
        return verdict(KEEP_DISCONNECTED, **kw)
    if np.float32(weakest) * factor > np.float32(P["th_map"]):
        return verdict(LINK, weakest, weakest_link=weakest, **kw)
    return verdict(KEEP_LINK, weakest_link=weakest, **kw)


def verdict_array(rows):
    out = np.zeros(len(rows), VERDICT_DTYPE)
    for i, r in enumerate(rows):
        for k in VERDICT_DTYPE.names:
            out[k][i] = r[k]
    return out


# ---- the tables of the stats tests -----------------------------------------------------------------------------------------------------------

TH_DEPTH = 40.0


def stats_fixture(seed=11):
    """A scene_numpy.build_map map (120 keyframes) with hand-made keyframes and points appended.  Returns (tables, queries, names): names[k]
    says what keyframe k is there for."""
    t = scene_numpy.build_map(seed=seed, imu=False)
    rng = np.random.RandomState(seed + 1)
    n_kf0, n_pt0 = len(t["kf_bad"]), len(t["pt_flags"])
    feats = [[(int(t["feat_point"][f]), float(t["feat_depth"][f]), int(t["feat_octave"][f])) for f in range(t["feat_start"][k], t["feat_start"][k + 1])]
             for k in range(n_kf0)]
    lists = [[tuple(o) for o in t["obs"][t["obs_start"][p]:t["obs_start"][p + 1]].tolist()] for p in range(n_pt0)]
    flags, pos = t["pt_flags"].tolist(), t["pt_pos"].tolist()
    bad, poses, names = t["kf_bad"].tolist(), t["kf_pose"].tolist(), {}

    def new_kf(name, features, is_bad=0):
        quat = rng.randn(4)
        poses.append((quat / np.linalg.norm(quat)).tolist() + rng.randn(3).tolist())
        bad.append(is_bad)
        feats.append(list(features))
        names[len(feats) - 1] = name
        return len(feats) - 1

    def new_pt(p=None, fl=0, obs=()):
        pos.append(list(p) if p is not None else (rng.randn(3) * 5).tolist())
        flags.append(fl)
        lists.append(list(obs))
        return len(pos) - 1

    # observers: eight keyframes of 8 features each with octaves 0 .. 7 = the feature index
    obsv = [new_kf("observer", [(-1, 1.0, f) for f in range(8)]) for _ in range(8)]
    plain = lambda n: [new_pt() for _ in range(n)]  # noqa: E731
    new_kf("no features", [])
    new_kf("one feature", [(plain(1)[0], 5.0, 0)])
    same = new_pt()
    new_kf("two features, equal depths", [(same, 5.0, 0), (same, 6.0, 1)])
    new_kf("three features", [(p, 5.0, 2) for p in plain(3)])
    new_kf("four features, one without a point", [(p, 5.0, 2) for p in plain(3)] + [(-1, 5.0, 0)] + [(plain(1)[0], 2.0, 1)])
    new_kf("256 features", [(p, float(rng.uniform(1, 60)), int(rng.randint(0, 8))) for p in plain(256)])
    new_kf("257 features", [(p, float(rng.uniform(1, 60)), int(rng.randint(0, 8))) for p in plain(257)])
    new_kf("only bad points", [(new_pt(fl=PT_BAD), 5.0, 0) for _ in range(5)])
    new_kf("a bad query", [(plain(1)[0], 5.0, 0)], is_bad=1)
    # the lists: the query sees every point at octave 3, so an observer's feature 4 qualifies (+1) and its feature 5 does not (+2)
    q_oct, walked = 3, []
    qk = len(feats)  # the keyframe made below

    def listed(length, n_qualify, twice=False):
        """A list of `length` entries of which exactly n_qualify qualify; the query itself is in it once (twice: two times)."""
        entries = [(qk, len(walked) - 1)] * (2 if twice else 1)  # the feature appended just before
        others = length - len(entries)
        for j in range(others):
            entries.append((obsv[j % 8], 4 if j < n_qualify else 5))
        order = rng.permutation(len(entries))
        return [entries[i] for i in order]

    cases = [("length 3", 3, 2, False), ("length 4, three qualify", 4, 3, False), ("length 4, two qualify", 4, 2, False),
             ("length 5, q twice", 5, 3, True), ("length 32", 32, 3, False), ("length 33", 33, 32, False), ("length 33, two qualify", 33, 2, False),
             ("length 300", 300, 3, False), ("length 300, two qualify", 300, 2, False), ("length 300, all qualify", 300, 299, False)]
    case_names = []
    for name, length, nq, twice in cases:
        p = new_pt()
        walked.append((p, 5.0, q_oct))
        lists[p] = listed(length, nq, twice)
        case_names.append(name)
    walked.append((plain(1)[0], TH_DEPTH, q_oct))  # depth == th_depth counts
    walked.append((plain(1)[0], float(np.nextafter(np.float32(TH_DEPTH), np.float32(100))), q_oct))  # just above: skipped under stereo
    walked.append((new_pt(fl=PT_BAD), 5.0, q_oct))
    got = new_kf("the lists", walked)
    assert got == qk
    # every point's own keyframe observes it (the two sides of the map agree where nothing else is said)
    for k in range(n_kf0, len(feats)):
        for f, (p, _, _) in enumerate(feats[k]):
            if p >= 0 and (k, f) not in lists[p] and k != qk:
                lists[p].append((k, f))
    # negative depths: a point behind "three features"
    k3 = [k for k, v in names.items() if v == "three features"][0]
    R, tr = rotation(poses[k3]), np.array(poses[k3][4:])
    pos[feats[k3][0][0]] = (R.T @ (np.array([0.3, -0.2, -4.0]) - tr)).tolist()
    pos[feats[k3][1][0]] = (R.T @ (np.array([0.1, 0.2, -1.5]) - tr)).tolist()

    fs = np.concatenate([[0], np.cumsum([len(x) for x in feats])]).astype(np.int32)
    flat = [f for x in feats for f in x]
    os_ = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    out = dict(kf_bad=np.array(bad, np.uint8), kf_pose=np.array(poses, np.float64), feat_start=fs,
               feat_point=np.array([f[0] for f in flat], np.int32), feat_depth=np.array([f[1] for f in flat], np.float32),
               feat_octave=np.array([f[2] for f in flat], np.int32), obs_start=os_,
               obs=np.array([o for x in lists for o in x], np.int32).reshape(-1, 2), pt_flags=np.array(flags, np.uint8),
               pt_pos=np.array(pos, np.float64), list_cases=case_names)
    queries = [k for k in range(n_kf0, len(feats)) if names[k] != "observer"] + [3, 7, 12, 20, 31] + [int(k) for k in np.flatnonzero(t["kf_bad"])[:1]]
    return out, queries, names


STATS_PROPERTIES = ["no features", "one feature", "two features, equal depths", "three features", "even count", "256 features", "257 features",
                    "feat_cap met", "feat_cap exceeded", "negative depth", "a bad query", "n_mps == 0", "bad point has a depth",
                    "depth == th_depth", "depth above th_depth", "length 3 not walked", "length 4", "length 32", "length 33", "length 300",
                    "q twice in a list", "octave + 1", "octave + 2", "two qualify", "three qualify", "redundancy strictly inside (0, 1)"]


def stats_coverage(t, queries, names, feat_cap=256):
    seen, rows = set(), {}
    for stereo in (0, 1):
        for cap in (feat_cap, 300):
            for q in queries:
                rows[(stereo, cap, q)] = r = stats(t, q, 3, stereo, TH_DEPTH, cap)
                nf = int(t["feat_start"][q + 1] - t["feat_start"][q])
                if r["status"] == SKIPPED:
                    seen.add("a bad query")
                    continue
                if r["status"] == FEAT_OVERFLOW:
                    seen |= {"feat_cap exceeded"} if nf == cap + 1 else set()
                    continue
                seen |= {"feat_cap met"} if nf == cap else set()
                seen |= {names[q]} if names.get(q) in STATS_PROPERTIES else set()
                seen |= {"even count"} if r["n_depth"] > 0 and r["n_depth"] % 2 == 0 else set()
                seen |= {"n_mps == 0"} if r["n_mps"] == 0 and np.isnan(r["redundancy"]) else set()
                seen |= {"bad point has a depth"} if r["n_depth"] > r["n_mps"] and stereo == 0 else set()
                seen |= {"redundancy strictly inside (0, 1)"} if 0 < r["redundancy"] < 1 else set()
                for i in range(t["feat_start"][q], t["feat_start"][q + 1]):
                    p = t["feat_point"][i]
                    if p < 0:
                        continue
                    seen |= {"negative depth"} if depth_of(t["kf_pose"][q], t["pt_pos"][p]) < 0 else set()
                    if t["pt_flags"][p] & PT_BAD:
                        continue
                    seen |= {"depth == th_depth"} if t["feat_depth"][i] == np.float32(TH_DEPTH) else set()
                    seen |= {"depth above th_depth"} if stereo and t["feat_depth"][i] > np.float32(TH_DEPTH) else set()
                    lst = t["obs"][t["obs_start"][p]:t["obs_start"][p + 1]].tolist()
                    seen |= {"length 3 not walked"} if len(lst) == 3 else set()
                    seen |= {f"length {len(lst)}"} if len(lst) in (4, 32, 33, 300) else set()
                    if len(lst) > 3:
                        seen |= {"q twice in a list"} if sum(k == q for k, _ in lst) == 2 else set()
                        octs = [int(t["feat_octave"][t["feat_start"][k] + f]) - int(t["feat_octave"][i]) for k, f in lst if k != q]
                        seen |= {"octave + 1"} if 1 in octs else set()
                        seen |= {"octave + 2"} if 2 in octs else set()
                        nq = sum(o <= 1 for o in octs)
                        seen |= {"two qualify"} if nq == 2 else set()
                        seen |= {"three qualify"} if nq == 3 else set()
    return seen, rows


# ---- the tables of the decision tests ----------------------------------------------------------------------------------------------------------

class _Builder:
    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)
        self.bad, self.pose, self.factor, self.median, self.conn, self.prev, self.next, self.time = [], [], [], [], [], [], [], []

    def kf(self, factor=1.0, median=8.0, centre=None, bad=0, time=None):
        quat = self.rng.randn(4)
        quat /= np.linalg.norm(quat)
        c = np.asarray(centre if centre is not None else self.rng.randn(3) * 3, np.float64)
        self.pose.append(np.concatenate([quat, -rotation(quat) @ c]))
        self.bad.append(bad)
        self.factor.append(factor)
        self.median.append(median)
        self.conn.append([])
        self.prev.append(-1)
        self.next.append(-1)
        self.time.append(float(len(self.time)) if time is None else time)
        return len(self.bad) - 1

    def link(self, a, b, w, w_back=None, one_sided=False):
        self.conn[a].append((w, b))
        if not one_sided:
            self.conn[b].append((w if w_back is None else w_back, a))

    def tables(self):
        lists = [sorted(x) for x in self.conn]
        cs = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
        cl = np.zeros(int(cs[-1]), CONN_DTYPE)
        flat = [c for x in lists for c in x]
        cl["weight"], cl["kf"] = [c[0] for c in flat], [c[1] for c in flat]
        return dict(kf_bad=np.array(self.bad, np.uint8), kf_pose=np.array(self.pose, np.float64), kf_cull_factor=np.array(self.factor, np.float32),
                    kf_median_depth=np.array(self.median, np.float64), kf_prev=np.array(self.prev, np.int32), kf_next=np.array(self.next, np.int32),
                    kf_time=np.array(self.time, np.float64), conn_start=cs, conn_list=cl)


def decide_fixture(seed=5):
    """Hand-made connection tables, one small cluster of keyframes per case.  Returns (tables, queries, stats [n_q] STATS_DTYPE, names)."""
    B = _Builder(seed)
    rng = B.rng
    cases = []  # (name, q, match_count, redundancy)

    def case(name, q, match_count=200, redundancy=0.1):
        cases.append((name, q, match_count, redundancy))
        return q

    case("one node", B.kf())
    q = case("one below the threshold", B.kf())
    B.link(q, B.kf(), 19)
    # two nodes: a weight exactly min_matches_in_graph and one below; the four outcomes of a side branch
    for name, dist, mc, red in (("angle", 0.05, 200, 0.1), ("matches", 4.0, 79, 0.1), ("redundancy", 4.0, 80, 0.81), ("branch", 4.0, 80, 0.8)):
        c = rng.randn(3)
        q = case("two nodes: " + name, B.kf(centre=c, median=10.0), mc, red)
        B.link(q, B.kf(centre=c + np.array([dist, 0, 0]), median=6.0), 20)
        B.link(q, B.kf(), 19)
    q = case("two nodes: redundancy is NaN", B.kf(), 100, np.float32(np.nan))
    B.link(q, B.kf(centre=rng.randn(3) + 5), 30)
    q = case("two nodes: the cached median is -1", B.kf(median=-1.0), 100, 0.1)
    B.link(q, B.kf(median=-1.0, centre=rng.randn(3) + 5), 30)
    q = case("two nodes: a bad neighbour", B.kf(), 100, 0.1)
    B.link(q, B.kf(bad=1, centre=rng.randn(3) + 5), 30)
    q = case("cull factor scales the borders", B.kf(factor=2.5), 199, 0.1)  # 199 < 80 * 2.5
    B.link(q, B.kf(centre=rng.randn(3) + 9), 30)
    # large graphs: a star at q plus random edges among the neighbours, weights with ties
    for n in (64, 65, 256, 257):
        q = case(f"{n} nodes", B.kf(factor=float(rng.choice([1.0, 2.0]))))
        nb = [B.kf() for _ in range(n - 1)]
        for k in nb:
            B.link(q, k, int(rng.randint(20, 60)))
        for _ in range(3 * n):
            a, b = rng.choice(len(nb), 2, replace=False)
            B.link(nb[a], nb[b], int(rng.randint(15, 200)), int(rng.randint(15, 200)))
    # a chain: q - a - b - c, every neighbour also linked to q more weakly than along the chain: one tree edge at q
    q = case("chain: one root edge of three nodes", B.kf(), 50, 0.1)
    a, b, c = B.kf(centre=rng.randn(3) + 7), B.kf(), B.kf()
    B.link(q, a, 90), B.link(q, b, 40), B.link(q, c, 30), B.link(a, b, 100), B.link(b, c, 95)
    # an edge listed on one side only, and with two different weights
    q = case("one-sided and two-weight edges", B.kf(factor=2.0))
    a, b, c = B.kf(), B.kf(), B.kf()
    B.link(q, a, 100), B.link(q, b, 100), B.link(q, c, 100)
    B.link(a, b, 75, one_sided=True), B.link(b, c, 50, w_back=90)  # second tree: a-b 75, b-c 90 -> weakest 75, 150 > 140
    # the tie rule: everything equal
    q = case("all weights equal", B.kf())
    nb = [B.kf() for _ in range(4)]
    for i, k in enumerate(nb):
        B.link(q, k, 30)
        for k2 in nb[i + 1:]:
            B.link(k, k2, 30)
    # the neighbours' graph is disconnected / connected at the threshold
    q = case("second graph disconnected", B.kf())
    a, b, c = B.kf(), B.kf(), B.kf()
    B.link(q, a, 100), B.link(q, b, 90), B.link(q, c, 80), B.link(a, b, 60)
    for name, w in (("weakest * factor == th_map", 70), ("weakest * factor above th_map", 71)):
        q = case(name, B.kf(factor=2.0))
        a, b = B.kf(), B.kf()
        B.link(q, a, 100), B.link(q, b, 90), B.link(a, b, w)
    # a keyframe listed twice by q (the last id answers) and q in its own list
    q = case("listed twice, q in its own list", B.kf())
    a, b = B.kf(), B.kf()
    B.conn[q] += [(25, a), (45, a), (33, q), (50, b)]
    B.conn[a] += [(45, q), (70, b)]
    B.conn[b] += [(50, q)]
    q = case("listed twice", B.kf(), 50, 0.1)
    a, b = B.kf(centre=rng.randn(3) + 6), B.kf(centre=rng.randn(3) - 6)
    B.conn[q] += [(25, a), (45, a), (50, b)]
    B.conn[a] += [(45, q), (70, b)]
    B.conn[b] += [(50, q), (70, a)]
    # the cull factor at 3 and just above
    q = case("factor 3", B.kf(factor=3.0), 239, 0.1)
    B.link(q, B.kf(centre=rng.randn(3) + 9), 30)
    q = case("factor above 3", B.kf(factor=float(np.nextafter(np.float32(3), np.float32(4)))))
    B.link(q, B.kf(), 30)
    case("a bad query", B.kf(bad=1))
    q = case("stats overflowed", B.kf())
    # the time gate: previous and next 0.5 apart (go on), more than 0.5 apart (keep), no previous (go on)
    for name, gap, has_prev in (("time gap at the limit", 0.5, True), ("time gap above the limit", 0.5000001, True), ("no previous keyframe", 9.0, False)):
        q = case(name, B.kf())
        p, nx = B.kf(time=100.0), B.kf(time=100.0 + gap)
        B.prev[q], B.next[q] = (p if has_prev else -1), nx
        B.link(q, p, 40)
    g = B.tables()
    queries = [c[1] for c in cases]
    st = np.zeros(len(cases), STATS_DTYPE)
    for i, (name, q, mc, red) in enumerate(cases):
        st[i] = (8.0, 100, mc, 100, 10, red, FEAT_OVERFLOW if name == "stats overflowed" else (SKIPPED if g["kf_bad"][q] else OK))
    return g, queries, st, [c[0] for c in cases]


# the parameter sets of the decision tests: (name, params, with the time tables)
PARAM_SETS = [("no imu", {}, True), ("imu", dict(with_imu=1, gyro_weight=1.0, acc_weight=2.0), True),
              ("imu, no time tables", dict(with_imu=1, gyro_weight=1.0, acc_weight=2.0), False),
              ("imu, gyro weight 0", dict(with_imu=1, gyro_weight=0.0, acc_weight=2.0), True),
              ("imu, acc weight 0", dict(with_imu=1, gyro_weight=1.0, acc_weight=0.0), False)]


def without_times(g):
    return {k: (None if k in ("kf_prev", "kf_next", "kf_time") else v) for k, v in g.items()}


def decide_all(g, queries, st, node_cap=MAX_NODES):
    """{parameter set name: list of verdict dicts}."""
    return {name: [decide(g if times else without_times(g), q, st[i], params, node_cap) for i, q in enumerate(queries)]
            for name, params, times in PARAM_SETS}


DECIDE_PROPERTIES = ([f"reason {r}" for r in range(1, 12)] + [f"status {s}" for s in (OK, SKIPPED, FEAT_OVERFLOW, NODES_OVERFLOW)] +
                     ["1 node", "2 nodes", "64 nodes", "65 nodes", "256 nodes", "weight == min_matches_in_graph", "weight below min_matches_in_graph",
                      "one-sided edge", "two weights", "tie: root degree above 1", "weakest * factor == th_map", "factor == 3", "factor above 3",
                      "time gap at the limit", "imu without time tables", "NaN redundancy", "listed twice", "root edge count 1 with 4 nodes"])


def decide_coverage(g, queries, st, names):
    seen = set()
    results = decide_all(g, queries, st)
    for pname, rows in results.items():
        for i, (q, r) in enumerate(zip(queries, rows)):
            seen.add(f"status {r['status']}")
            if r["status"] != OK:
                continue
            seen.add(f"reason {r['reason']}")
            seen |= {f"{r['n_nodes']} node" + ("s" if r["n_nodes"] > 1 else "")} if r["n_nodes"] in (1, 2, 64, 65, 256) else set()
            conns = connections(g, q)
            if r["n_nodes"]:
                seen |= {"weight == min_matches_in_graph"} if any(w == 20 for w, _ in conns) else set()
                seen |= {"weight below min_matches_in_graph"} if any(w == 19 for w, _ in conns) else set()
                seen |= {"listed twice"} if len({k for _, k in conns}) < len(conns) else set()
                nodes = {k for w, k in conns if w >= 20}
                for a in nodes:
                    for w, b in connections(g, a):
                        if b in nodes and b != a:
                            back = [w2 for w2, k in connections(g, b) if k == a]
                            seen |= {"one-sided edge"} if not back else set()
                            seen |= {"two weights"} if back and back[0] != w else set()
            seen |= {"tie: root degree above 1"} if names[i] == "all weights equal" and r["n_root_edges"] > 1 else set()
            seen |= {"root edge count 1 with 4 nodes"} if r["n_root_edges"] == 1 and r["n_nodes"] == 4 else set()
            f = float(g["kf_cull_factor"][q])
            seen |= {"weakest * factor == th_map"} if r["reason"] == KEEP_LINK and r["weakest_link"] * f == 140 else set()
            seen |= {"factor == 3"} if f == 3.0 and r["reason"] != FACTOR else set()
            seen |= {"factor above 3"} if f > 3.0 and r["reason"] == FACTOR else set()
            seen |= {"time gap at the limit"} if pname == "imu" and names[i] == "time gap at the limit" and r["reason"] != KEEP_TIME_GAP else set()
            seen |= {"imu without time tables"} if pname == "imu, no time tables" and names[i] == "time gap above the limit" and r["reason"] != KEEP_TIME_GAP else set()
            seen |= {"NaN redundancy"} if np.isnan(st["redundancy"][i]) and r["reason"] == KEEP_BRANCH else set()
    return seen, results


def require_coverage():
    """Both fixtures, checked: raises on a property that does not occur.  Returns (stats fixture, decide fixture, stats rows, verdict rows)."""
    sf = stats_fixture()
    seen, srows = stats_coverage(*sf)
    missing = [p for p in STATS_PROPERTIES if p not in seen]
    df = decide_fixture()
    seen2, vrows = decide_coverage(*df)
    missing += [p for p in DECIDE_PROPERTIES if p not in seen2]
    if missing:
        raise AssertionError(f"the fixtures do not contain: {missing}")
    return sf, df, srows, vrows


def angle_margins(g, queries, results):
    """|angle - threshold| of every verdict that computed an angle: the distance at which a different atan2 could change it."""
    out = []
    for pname, params, _ in PARAM_SETS:
        P = dict(PARAMS, **params)
        for q, r in zip(queries, results[pname]):
            if "angle" in r:
                out.append(abs(r["angle"] - float(np.float32(P["border_angle"]) * np.float32(g["kf_cull_factor"][q]))))
    return out
