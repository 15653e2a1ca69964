"""Restatement of "snk-covis v1" (DESIGN.md section 3i): Keyframe::UpdateConnections (reference Snake/Map/Keyframe.cpp:89-171) and the
vote at the head of Tracking::UpdateLocalKeyFrames2 (reference Snake/Tracking/TrackingFine.cpp:230-268), written line by line from the
reference as a dictionary loop over the map tables, with the [DEFINED] rules: among equal largest counts the smallest id, the list
ascending by (weight, id), the LAST cap entries kept.  Also the case builders of the covisibility tests.

A map is a dict: kf_bad [n_kf] u8, obs_start [n_points + 1] i32, obs [n_obs, 2] i32 (kf, feature), pt_flags [n_points] u8 (1 = bad,
2 = far), feat_start [n_kf + 1] i32, feat_point [n_feat] i32 (-1: none), feat_depth [n_feat] f32.  The two sides are read as given."""
import numpy as np

MAX_KF, MAX_CAP = 32768, 4096
OK, UNCHANGED, BAD_INDEX = 0, 1, 2
PT_BAD, PT_FAR = 1, 2
LONG_MIN = 32  # dispatch.hpp COVIS_LONG_MIN (tests/test_covis_core_cpu.py pins it)
TH, TH_DEPTH = 15, 40.0

CONN = np.dtype([("weight", "<i4"), ("kf", "<i4")])
RESULT = np.dtype([("n_found", "<i4"), ("n_conn", "<i4"), ("best_kf", "<i4"), ("status", "<i4")])
MAP_KEYS = ("kf_bad", "obs_start", "obs", "pt_flags")
FEAT_KEYS = ("feat_start", "feat_point", "feat_depth")


def empty_outputs(n, cap):
    conn = np.empty((n, cap), CONN)
    conn["weight"] = conn["kf"] = -1  # "not written"
    res = np.zeros(n, RESULT)
    res["best_kf"] = -1
    return conn, res


def _store(pairs, status, cap, conn_row):
    """pairs: the full list, ascending.  The last cap entries, still ascending."""
    kept = pairs[max(len(pairs) - cap, 0):]
    for i, (w, k) in enumerate(kept):
        conn_row[i] = (w, k)
    return (len(pairs), len(kept), kept[-1][1] if kept else -1, status)


def update(m, q, th=TH, th_depth=TH_DEPTH, cap=256):
    """Keyframe::UpdateConnections for every q of the list, each against the same tables."""
    bad, os_, flags = m["kf_bad"].tolist(), m["obs_start"].tolist(), m["pt_flags"].tolist()
    obs_kf, fs, fp = m["obs"][:, 0].tolist(), m["feat_start"].tolist(), m["feat_point"].tolist()
    deeper = (m["feat_depth"].astype(np.float32) > np.float32(th_depth)).tolist()  # :111 on floats
    conn, res = empty_outputs(len(q), cap)
    for s, me in enumerate(np.asarray(q).tolist()):
        counter = {}
        for i in range(fs[me], fs[me + 1]):
            p = fp[i]
            if p < 0:  # :105
                continue
            if flags[p] & PT_BAD:  # :107
                continue
            if deeper[i] or flags[p] & PT_FAR:  # :111-115
                continue
            for o in range(os_[p], os_[p + 1]):  # :117
                k = obs_kf[o]
                if k == me:  # :119
                    continue
                counter[k] = counter.get(k, 0) + 1  # :120, weight 1
        if not counter:  # :125
            res[s] = (0, 0, -1, UNCHANGED)
            continue
        nmax, kmax, pairs = 0, None, []
        for k in sorted(counter):  # [DEFINED] ids ascending and a strict >: the smallest id among equal largest counts
            if bad[k]:  # :141
                continue
            if counter[k] > nmax:  # :142
                nmax, kmax = counter[k], k
            if counter[k] >= th:  # :147
                pairs.append((counter[k], k))
        if not pairs and kmax is not None:  # :154
            pairs.append((nmax, kmax))
        pairs.sort()  # [DEFINED] the full pair, KeyframeGraph.cpp:124
        res[s] = _store(pairs, OK, cap, conn[s])
    return conn, res


def vote(m, set_start, set_point, cap=256):
    """The vote of UpdateLocalKeyFrames2 for every set of point ids."""
    os_, flags, obs_kf = m["obs_start"].tolist(), m["pt_flags"].tolist(), m["obs"][:, 0].tolist()
    ss, sp = np.asarray(set_start).tolist(), np.asarray(set_point).reshape(-1).tolist()
    conn, res = empty_outputs(len(ss) - 1, cap)
    for s in range(len(ss) - 1):
        counter = {}
        for i in range(ss[s], ss[s + 1]):
            p = sp[i]
            if p < 0:  # :233
                continue
            if flags[p] & PT_BAD:  # :235
                continue
            for o in range(os_[p], os_[p + 1]):  # :241
                counter[obs_kf[o]] = counter.get(obs_kf[o], 0) + 1  # :244
        if not counter:  # :254
            res[s] = (0, 0, -1, UNCHANGED)
            continue
        pairs = sorted((c, k) for k, c in counter.items())  # :267
        res[s] = _store(pairs, OK, cap, conn[s])
    return conn, res


# ---- case builders ------------------------------------------------------------------------------------------------------------------
class Builder:
    """A map put together point by point and feature by feature; the two sides are independent."""

    def __init__(self, n_kf):
        self.n_kf = n_kf
        self.kf_bad = np.zeros(n_kf, np.uint8)
        self.lists, self.flags = [], []
        self.feats = [[] for _ in range(n_kf)]

    def point(self, observers, flags=0):
        self.lists.append([(int(k), len(self.lists) % 7) for k in observers])
        self.flags.append(flags)
        return len(self.lists) - 1

    def feature(self, kf, point, depth=10.0):
        self.feats[kf].append((point, depth))

    def see(self, kf, observers, n=1, depth=10.0, flags=0):
        """n new points, each observed by `observers`, each a feature of kf.  Returns their ids."""
        ids = [self.point(observers, flags) for _ in range(n)]
        for p in ids:
            self.feature(kf, p, depth)
        return ids

    def tables(self):
        obs = [o for lst in self.lists for o in lst]
        return dict(kf_bad=self.kf_bad.copy(), obs_start=np.concatenate([[0], np.cumsum([len(x) for x in self.lists])]).astype(np.int32),
                    obs=np.array(obs, np.int32).reshape(-1, 2), pt_flags=np.array(self.flags, np.uint8),
                    feat_start=np.concatenate([[0], np.cumsum([len(f) for f in self.feats])]).astype(np.int32),
                    feat_point=np.array([p for f in self.feats for p, _ in f], np.int32),
                    feat_depth=np.array([d for f in self.feats for _, d in f], np.float32))


def sets_of(lists):
    return np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32), np.array([p for x in lists for p in x], np.int32)


TRUNC_CAPS = (4, 64)
TRUNC_QUERIES = {4: (1, 2, 3, 4), 64: (43, 44, 45, 46)}  # n_found = cap - 1, cap, cap + 1, 3 cap under that cap


def edge_case(n_kf=1025):
    """The hand-built map.  Returns the tables plus q (the queries, one repeated), set_start / set_point (the vote's sets) and `what`:
    query or set name -> index.  th = TH, th_depth = TH_DEPTH.  n_kf < 255: the two-keyframe version of it."""
    K, b = n_kf, Builder(n_kf)
    just_above = float(np.nextafter(np.float32(TH_DEPTH), np.float32(np.inf)))
    if K < 255:
        other = K - 1
        b.see(0, [0, other], 16)  # K = 1: only the query itself -> UNCHANGED; K = 2: keyframe 1 with 16
        b.see(other, [other, 0, 0], 3)  # K = 2: keyframe 0 with 6 < th: the fallback
        c = b.tables()
        c["q"] = np.array([0, other, 0], np.int32)
        c["set_start"], c["set_point"] = sets_of([[0, 1, -1, 16, 17], [], [-1, -1]])
        c["what"] = {}
        return c
    q, what = [], {}

    def query(name, kf):
        what[name] = len(q)
        q.append(kf)
        return kf

    me = query("thresholds", 5)
    for kf, n in ((10, 14), (11, 15), (12, 16), (0, 15), (K - 1, 15)):  # 14 / 15 / 16, equal weights, ids 0 and n_kf - 1
        b.see(me, [kf, me], n)  # the query's own observation rides along and is not counted
    b.see(me, [13], 13), b.see(me, [13], 1, depth=TH_DEPTH), b.see(me, [13], 1, depth=-1.0)  # == th_depth and <= 0 count: 15
    b.see(me, [14], 14), b.see(me, [14], 1, depth=just_above)  # just above: 14
    b.see(me, [15], 14), b.see(me, [15], 1, flags=PT_FAR)  # far: 14
    b.see(me, [16], 14), b.see(me, [16], 1, flags=PT_BAD), b.see(me, [16], 1, flags=PT_BAD | PT_FAR)  # bad: 14
    b.see(me, [17], 14), b.see(me, [17], 1, depth=0.0)  # 15
    thresholds_points = [p for p, _ in b.feats[me]]

    me = query("fallback_tie", 6)
    b.see(me, [21, 20], 7), b.see(me, [22], 3)  # 20 and 21 tied at 7 < th: 20

    b.kf_bad[30] = 1
    me = query("bad_largest", 7)
    bad_kf_points = b.see(me, [30], 40) + b.see(me, [31], 20) + b.see(me, [32], 15)
    me = query("only_bad", 8)
    b.see(me, [30], 3)
    me = query("bad_fallback", 47)  # the bad keyframe holds the largest count below th: the fallback is the best of the others
    b.see(me, [30], 9), b.see(me, [31], 4), b.see(me, [32], 4)

    me = query("untouched", 9)
    b.feature(me, -1), b.see(me, [], 2), b.see(me, [me], 2), b.see(me, [11], 1, flags=PT_BAD)
    query("no_features", 33)

    me = query("duplicates", 34)
    b.see(me, [40, 40], 8)  # a point listing keyframe 40 twice: 16
    for p in b.see(me, [41], 8) + b.see(me, [42], 7):  # a keyframe holding a point in two features: 16 and 14
        b.feature(me, p)

    me = query("long_lists", 35)
    long_points = []
    for n in (63, 64, 65, 300, 4096):
        long_points += b.see(me, 50 + np.arange(n) % 200, 1)
    long_points += b.see(me, [0, K - 1] * 8, 1)

    trunc_sets = {}
    for cap in TRUNC_CAPS:
        for j, (kf, n) in enumerate(zip(TRUNC_QUERIES[cap], (cap - 1, cap, cap + 1, 3 * cap))):
            me = query(f"trunc{cap}_{j}", kf)
            group = list(range(60, 60 + n))
            pts = b.see(me, group, 15) + b.see(me, group[n // 3:], 1)  # 15 up to a third of the way, 16 beyond: equal weights across the cut
            trunc_sets[(cap, j)] = pts
    query("thresholds_again", 5)

    c = b.tables()
    c["q"], c["what"] = np.array(q, np.int32), what
    sets = [("frame", thresholds_points + [-1, -1]), ("empty", []), ("none", [-1] * 5), ("long", long_points),
            ("only_bad_points", [p for p, f in enumerate(b.flags) if f & PT_BAD]), ("bad_keyframe", bad_kf_points)]
    sets += [(f"trunc{cap}_{j}", pts) for (cap, j), pts in trunc_sets.items()]
    for i, (name, _) in enumerate(sets):
        what["set_" + name] = i
    c["set_start"], c["set_point"] = sets_of([pts for _, pts in sets])
    return c


def make_map(seed, n_kf, n_points, window=300, p_see=0.5, none_frac=0.1, bad_kf=0.03, bad_pt=0.03, far_pt=0.03, shuffle=True):
    """A structured map: keyframe k sees a sliding window of `window` consecutive points (each with probability p_see), so neighbouring
    keyframes share many points and most lists have several entries >= 15 -- a uniformly random map degenerates into the fallback for
    nearly every keyframe.  Depths are uniform in [0.5, 50): a fifth of the features is deeper than TH_DEPTH."""
    rng = np.random.default_rng(seed)
    stride = (n_points - window) / max(n_kf - 1, 1) if n_points > window else 0.0
    feats = []
    for k in range(n_kf):
        lo = int(k * stride)
        pts = np.arange(lo, min(lo + window, n_points))
        pts = pts[rng.random(len(pts)) < p_see]
        pts = np.concatenate([pts, np.full(int(len(pts) * none_frac), -1)])
        feats.append(rng.permutation(pts))
    feat_start = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int32)
    feat_point = np.concatenate(feats).astype(np.int32) if feats else np.zeros(0, np.int32)
    feat_kf = np.repeat(np.arange(n_kf), np.diff(feat_start))
    feat_idx = np.arange(len(feat_point)) - feat_start[feat_kf]
    has = feat_point >= 0
    pk = np.stack([feat_point[has], feat_kf[has], feat_idx[has]], 1)
    if shuffle:
        pk = pk[rng.permutation(len(pk))]  # list order is the order of insertion, not of the ids
    pk = pk[np.argsort(pk[:, 0], kind="stable")]
    obs_start = np.concatenate([[0], np.cumsum(np.bincount(pk[:, 0], minlength=n_points))]).astype(np.int32)
    flags = (rng.random(n_points) < bad_pt) * PT_BAD + (rng.random(n_points) < far_pt) * PT_FAR
    return dict(kf_bad=(rng.random(n_kf) < bad_kf).astype(np.uint8), obs_start=obs_start, obs=np.ascontiguousarray(pk[:, 1:], np.int32),
                pt_flags=flags.astype(np.uint8), feat_start=feat_start, feat_point=feat_point,
                feat_depth=rng.uniform(0.5, 50.0, len(feat_point)).astype(np.float32))


def frames_of(m, seed, n_frames, n_matched=300, cap=None):
    """Vote sets drawn from a map: frame f matched n_matched points around a random keyframe's window.  cap: pad every set to cap with
    -1 and return the padded [n_frames, cap] array too."""
    rng = np.random.default_rng(seed)
    n_kf = len(m["kf_bad"])
    lists = []
    for _ in range(n_frames):
        k = int(rng.integers(0, n_kf))
        pts = m["feat_point"][m["feat_start"][k]:m["feat_start"][k + 1]]
        lists.append(rng.permutation(pts)[:n_matched].tolist())
    if cap is None:
        return sets_of(lists)
    padded = np.full((n_frames, cap), -1, np.int32)
    for f, pts in enumerate(lists):
        padded[f, :min(len(pts), cap)] = pts[:cap]
    return (np.arange(n_frames + 1) * cap).astype(np.int32), padded


def bad_index_sets(m, q=None, set_start=None, set_point=None, th_depth=TH_DEPTH):
    """Which sets the device forms answer with BAD_INDEX: the query outside [0, n_kf); the set's range outside its array
    or decreasing; any of its point ids >= n_points or < -1; for a point that counts (the gate is applied first, a skipped point's list
    is not looked at), a list range outside obs or decreasing, or an observation's keyframe outside [0, n_kf)."""
    n_kf, n_pts, n_obs = len(m["kf_bad"]), len(m["pt_flags"]), len(m["obs"])
    connection = q is not None
    start = m["feat_start"] if connection else np.asarray(set_start)
    point = m["feat_point"] if connection else np.asarray(set_point).reshape(-1)
    n_sets = len(q) if connection else len(start) - 1
    bad = np.zeros(n_sets, bool)
    for s in range(n_sets):
        me = int(q[s]) if connection else s
        if connection and not 0 <= me < n_kf:
            bad[s] = True
            continue
        a, b = int(start[me]), int(start[me + 1])
        if a < 0 or b < a or b > len(point):
            bad[s] = True
            continue
        for i in range(a, b):
            p = int(point[i])
            if p < -1 or p >= n_pts:
                bad[s] = True
                break
            if p < 0 or m["pt_flags"][p] & PT_BAD:
                continue
            if connection and (m["feat_depth"][i] > np.float32(th_depth) or m["pt_flags"][p] & PT_FAR):
                continue
            oa, ob = int(m["obs_start"][p]), int(m["obs_start"][p + 1])
            if oa < 0 or ob < oa or ob > n_obs or np.any((m["obs"][oa:ob, 0] < 0) | (m["obs"][oa:ob, 0] >= n_kf)):
                bad[s] = True
                break
    return bad


def update_checked(m, q, th=TH, th_depth=TH_DEPTH, cap=256):
    """update() with the device forms' BAD_INDEX answers: the restatement runs for the other sets only."""
    q = np.asarray(q)
    bad = bad_index_sets(m, q=q, th_depth=th_depth)
    conn, res = empty_outputs(len(q), cap)
    conn[~bad], res[~bad] = update(m, q[~bad], th, th_depth, cap)
    res["status"][bad] = BAD_INDEX
    return conn, res


def vote_checked(m, set_start, set_point, cap=256):
    set_start, set_point = np.asarray(set_start), np.asarray(set_point).reshape(-1)
    bad = bad_index_sets(m, set_start=set_start, set_point=set_point)
    good = np.nonzero(~bad)[0]
    conn, res = empty_outputs(len(bad), cap)
    ss, sp = sets_of([set_point[set_start[s]:set_start[s + 1]].tolist() for s in good])
    conn[good], res[good] = vote(m, ss, sp, cap)
    res["status"][bad] = BAD_INDEX
    return conn, res
