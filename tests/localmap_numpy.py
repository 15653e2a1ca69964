"""Restatement of "snk-lmap v1" (DESIGN.md section 3j): the rest of Tracking::UpdateLocalKeyFrames2 behind the vote (reference
Snake/Tracking/TrackingFine.cpp:272-323) and Tracking::UpdateLocalPoints with LocalMap::addPoint (:328-356, Snake/Map/LocalMap.h:139-154),
written statement by statement from the reference with Python lists and dicts, plus the [DEFINED] integer draw rule and the hash of
lmap_core.hpp.  Also the case builders of the local-map tests: edge_case() asserts that every situation the tests name occurs in it.

All results are integers or copied bytes: the tests compare for equality."""
import numpy as np

MAX_KF, MAX_VOTE_CAP = 32768, 4096
MAX_LOCAL_KF, MAX_PTS, MAX_NEIGHBOURS, MAX_ORDER = 256, 16384, 16, 1 << 30
OK, EMPTY, TRUNCATED, KF_OVERFLOW, PTS_OVERFLOW, BAD_INDEX = range(6)
VOTE_OK, VOTE_UNCHANGED, VOTE_BAD_INDEX = 0, 1, 2
PT_BAD = 1
THREADS = 256  # dispatch.hpp LMAP_THREADS: a scan chunk

CONN = np.dtype([("weight", "<i4"), ("kf", "<i4")])
VOTE = np.dtype([("n_found", "<i4"), ("n_conn", "<i4"), ("best_kf", "<i4"), ("status", "<i4")])
SELECT = np.dtype([("n_local", "<i4"), ("n_direct", "<i4"), ("n_indirect", "<i4"), ("reference_kf", "<i4"), ("status", "<i4")])
GATHER = np.dtype([("n_pts", "<i4"), ("n_searchable", "<i4"), ("n_own_new", "<i4"), ("status", "<i4")])
LM_FINE = np.dtype([("pos", "<f8", 3), ("normal", "<f8", 3), ("desc", "<u8", 4), ("reference_depth", "<f4"), ("reference_scale_level", "<i4"),
                    ("valid", "u1"), ("pad", "u1", 7)])
POINT_KEYS = ("pos", "normal", "desc", "ref_depth", "ref_level")
PARAMS = dict(n_direct=15, n_direct_prob=5, n_indirect_prob=5, n_neighbours=5, kf_cap=64, seed=0)
M32 = 0xFFFFFFFF


# ---- the integer rules of lmap_core.hpp ---------------------------------------------------------------------------------------------
def mix(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def key_of(seed, frame_id):
    h = mix((seed & M32) ^ 0x9E3779B9)
    return mix(h ^ ((seed >> 32) & M32)) ^ (frame_id & M32)


def draw(key, c):
    return mix(mix(key) ^ (c & M32))


def accept(h, k, n):
    """Random::sampleDouble(0, 1) < k / double(n)"""
    return h * n < (k << 32)


def hash_of(point_id):
    return mix((point_id & M32) ^ 0x9E3779B9)


def table_slots(pts_cap):
    n = 2 * THREADS
    while n < 2 * pts_cap:
        n *= 2
    return n


def vote_status(status, n_found, n_conn, vote_cap):
    if status == VOTE_UNCHANGED:
        return EMPTY
    if status != VOTE_OK or n_found < 0 or n_conn < 0 or n_conn > vote_cap or n_conn > n_found:
        return BAD_INDEX
    if n_found > n_conn:
        return TRUNCATED
    return EMPTY if n_found == 0 else OK


# ---- stage 1 ---------------------------------------------------------------------------------------------------------------------------
def select(conn, vote, kf_bad, conn_start, conn_list, frame_id, params=None, trace=None):
    """TrackingFine.cpp:272-323 for every set, with the checks of the device form (a set with an index out of range: BAD_INDEX).
    Returns (local_kf [n_sets, kf_cap] with -1 past n_local, result [n_sets] SELECT).  trace: a list that receives a dict per set."""
    P = dict(PARAMS, **(params or {}))
    kf_cap, nn, seed = P["kf_cap"], P["n_neighbours"], P["seed"]
    bad_kf, cs = np.asarray(kf_bad).tolist(), np.asarray(conn_start).tolist()
    cl_kf = np.asarray(conn_list, CONN).reshape(-1)["kf"].tolist()
    n_kf, n_list = len(bad_kf), len(cl_kf)
    vote = np.asarray(vote, VOTE).reshape(-1)
    n_sets = len(vote)
    conn = np.asarray(conn, CONN).reshape(n_sets, -1)
    local_kf = np.full((n_sets, kf_cap), -1, np.int32)
    res = np.zeros(n_sets, SELECT)
    for s in range(n_sets):
        t = dict(acc1=0, rej1=0, acc2=0, rej2=0, nb_bad=0, nb_marked_vote=0, nb_again=0, nb_new=0, conn_sizes=set())
        if trace is not None:
            trace.append(t)

        def fail(status):
            res[s] = (0, 0, 0, -1, status)

        st = vote_status(int(vote[s]["status"]), int(vote[s]["n_found"]), int(vote[s]["n_conn"]), conn.shape[1])
        if st != OK:  # :254
            fail(st)
            continue
        count_keyframe = conn[s]["kf"][:vote[s]["n_found"]].tolist()  # ascending by (count, id): :267
        if any(k < 0 or k >= n_kf for k in count_keyframe):
            fail(BAD_INDEX)
            continue
        in_local_keyframes = set(count_keyframe)  # :246-250: every touched keyframe
        reference_kf = count_keyframe[-1]  # :268
        local_keyframes = []
        n_direct = min(P["n_direct"], len(count_keyframe))
        for _ in range(n_direct):  # :272-276
            local_keyframes.append(count_keyframe.pop())
        R = len(count_keyframe)  # :280: prob = n_direct_prob / R
        key = key_of(seed, int(frame_id[s]))
        indirect_neighbor, c = [], 0
        while count_keyframe:  # :282-295
            kf = count_keyframe[-1]
            if accept(draw(key, c), P["n_direct_prob"], R):
                local_keyframes.append(kf)
                t["acc1"] += 1
            else:
                indirect_neighbor.append(kf)
                t["rej1"] += 1
            c += 1
            count_keyframe.pop()
        if len(local_keyframes) > kf_cap:
            fail(KF_OVERFLOW)
            continue
        bad = False
        from_walk1 = len(indirect_neighbor)
        for kf in local_keyframes:  # :299-313
            a, b = cs[kf], cs[kf + 1]
            if a < 0 or b < a or b > n_list:
                bad = True
                continue
            t["conn_sizes"].add(b - a)
            for nb in cl_kf[b - min(nn, b - a):b]:  # GetBestCovisibilityKeyFrames(5): the last five, ascending (KeyframeGraph.cpp:62)
                if nb < 0 or nb >= n_kf:
                    bad = True
                    continue
                if bad_kf[nb]:  # :304
                    t["nb_bad"] += 1
                    continue
                if nb in in_local_keyframes:  # :306
                    t["nb_again" if nb in indirect_neighbor[from_walk1:] else "nb_marked_vote"] += 1
                    continue
                indirect_neighbor.append(nb)
                in_local_keyframes.add(nb)
                t["nb_new"] += 1
        if bad:
            fail(BAD_INDEX)
            continue
        n_ind = len(indirect_neighbor)  # :316: prob_ind = n_indirect_prob / n_ind
        for j, kf in enumerate(indirect_neighbor):  # :317-323
            if accept(draw(key, R + j), P["n_indirect_prob"], n_ind):
                local_keyframes.append(kf)
                t["acc2"] += 1
            else:
                t["rej2"] += 1
        if len(local_keyframes) > kf_cap:
            fail(KF_OVERFLOW)
            continue
        local_kf[s, :len(local_keyframes)] = local_keyframes
        res[s] = (len(local_keyframes), n_direct, n_ind, reference_kf, OK)
    return local_kf, res


# ---- stage 2 ---------------------------------------------------------------------------------------------------------------------------
def gather(m, frame_id, local_kf, sel, set_start, set_point, pts_cap, fill=0):
    """TrackingFine.cpp:328-356 with LocalMap::addPoint for every set, with the checks of the device form.  m: feat_start, feat_point,
    pt_flags, pt_last_seen and the POINT_KEYS tables.  Returns (lm_pts [n_sets, pts_cap] LM_FINE, lm_point, n_pts, result); records past
    n_pts hold the byte `fill` ("not written")."""
    fs, fp = np.asarray(m["feat_start"]).tolist(), np.asarray(m["feat_point"]).tolist()
    flags, last_seen = np.asarray(m["pt_flags"]).tolist(), np.asarray(m["pt_last_seen"]).tolist()
    n_kf, n_feat, n_points = len(fs) - 1, len(fp), len(flags)
    ss, sp = np.asarray(set_start).tolist(), np.asarray(set_point).reshape(-1).tolist()
    sel = np.asarray(sel, SELECT).reshape(-1)
    n_sets = len(sel)
    local_kf = np.asarray(local_kf).reshape(n_sets, -1)
    kf_cap = local_kf.shape[1]
    lm_pts = np.frombuffer(bytes([fill]) * (n_sets * pts_cap * LM_FINE.itemsize), LM_FINE).reshape(n_sets, pts_cap).copy()
    lm_point = np.full((n_sets, pts_cap), -1, np.int32)
    n_pts = np.zeros(n_sets, np.int32)
    res = np.zeros(n_sets, GATHER)
    for s in range(n_sets):
        status = int(sel[s]["status"])
        if status not in (OK, EMPTY):  # passed through
            res[s] = (0, 0, 0, status if status in (TRUNCATED, KF_OVERFLOW, PTS_OVERFLOW) else BAD_INDEX)
            continue
        n_local = 0 if status == EMPTY else int(sel[s]["n_local"])
        if n_local < 0 or n_local > kf_cap:
            res[s]["status"] = BAD_INDEX
            continue
        local_keyframes = local_kf[s, :n_local].tolist()
        bad, total = False, 0
        for kf in local_keyframes:
            if kf < 0 or kf >= n_kf:
                bad = True
            elif fs[kf] < 0 or fs[kf + 1] < fs[kf] or fs[kf + 1] > n_feat or fs[kf + 1] - fs[kf] > MAX_ORDER:
                bad = True
            else:
                total += fs[kf + 1] - fs[kf]
        if not (0 <= ss[s] <= ss[s + 1] <= len(sp)):
            bad = True
        elif total + ss[s + 1] - ss[s] > MAX_ORDER:
            bad = True
        if bad:
            res[s]["status"] = BAD_INDEX
            continue
        fid = int(frame_id[s])
        points, valid, lm_id = [], [], {}  # lm.points, their .valid, per_point_data

        def add_point(p):  # LocalMap.h:139-154
            if p not in lm_id:
                lm_id[p] = len(points)
                points.append(p)
                valid.append(True)  # LocalMap.h:44
            return lm_id[p]

        for kf in local_keyframes:  # :334
            for i in range(fs[kf], fs[kf + 1]):  # :336
                p = fp[i]
                if p < -1 or p >= n_points:
                    bad = True
                    continue
                if p < 0 or flags[p] & PT_BAD:  # :338
                    continue
                if last_seen[p] == fid:  # :339
                    continue
                add_point(p)  # :340
        from_keyframes = len(points)
        for i in range(ss[s], ss[s + 1]):  # :344
            p = sp[i]
            if p < -1 or p >= n_points:
                bad = True
                continue
            if p < 0 or flags[p] & PT_BAD:  # :346
                continue
            valid[add_point(p)] = False  # :351-353
        if bad or len(points) > pts_cap:
            res[s]["status"] = BAD_INDEX if bad else PTS_OVERFLOW
            continue
        n = len(points)
        rec = np.zeros(n, LM_FINE)
        rec["pos"], rec["normal"], rec["desc"] = m["pos"][points], m["normal"][points], m["desc"][points]
        rec["reference_depth"], rec["reference_scale_level"], rec["valid"] = m["ref_depth"][points], m["ref_level"][points], valid
        lm_pts[s, :n] = rec
        lm_point[s, :n] = points
        n_pts[s] = n
        res[s] = (n, int(np.sum(valid)), n - from_keyframes, OK)
    return lm_pts, lm_point, n_pts, res


# ---- case builders ------------------------------------------------------------------------------------------------------------------
SELECT_LENGTHS = (0, 1, 14, 15, 16, 20, 21, 15 + 65, 15 + 257)
SEEDS = (0, 0x123456789ABCDEF, 0xFFFFFFFFFFFFFFFF)


def csr(lists):
    return np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)


def select_case(seed=SEEDS[0]):
    """Votes of the SELECT_LENGTHS (ids spread over the map so that neighbours fall inside and outside them), one cut by its cap, one
    repeated under another frame id; connection lists of 0 / 3 / 5 / 9 entries; bad keyframes.  `kf_caps`: 256 and the three caps around
    the n_local of set `cap_set`.  Asserts that the situations the tests name occur."""
    n_kf, vote_cap = 700, 320
    rng = np.random.RandomState(5)
    kf_bad = np.zeros(n_kf, np.uint8)
    kf_bad[rng.choice(n_kf, 60, replace=False)] = 1
    lists = []
    for k in range(n_kf):
        size = (0, 3, 5, 9)[k % 4]
        nbs = rng.choice(n_kf // 4 if k % 3 == 0 else n_kf, size, replace=False)
        lists.append(sorted(zip(rng.randint(15, 80, size).tolist(), nbs.tolist())))  # ascending by (weight, kf)
    conn_start = csr(lists)
    conn_list = np.array([e for lst in lists for e in lst], CONN).reshape(-1)
    lengths = list(SELECT_LENGTHS) + [SELECT_LENGTHS[-2], 40, 30]
    n_sets = len(lengths)
    conn = np.empty((n_sets, vote_cap), CONN)
    conn["weight"] = conn["kf"] = -1
    vote = np.zeros(n_sets, VOTE)
    for s, n in enumerate(lengths):
        if n == 0:
            vote[s] = (0, 0, -1, VOTE_UNCHANGED)
            continue
        ids = rng.choice(n_kf, n, replace=False) if s != 9 else conn[7]["kf"][:n]
        pairs = sorted(zip(rng.randint(1, 9, n).tolist(), ids.tolist())) if s != 9 else list(zip(conn[7]["weight"][:n].tolist(), ids.tolist()))
        conn[s, :n] = pairs
        vote[s] = (n, n, pairs[-1][1], VOTE_OK)
    trunc = n_sets - 1  # 30 kept of 47 found
    vote[trunc]["n_found"] = 47
    frame_id = (100 + 3 * np.arange(n_sets)).astype(np.int32)
    c = dict(conn=conn, vote=vote, kf_bad=kf_bad, conn_start=conn_start, conn_list=conn_list, frame_id=frame_id, n_kf=n_kf, vote_cap=vote_cap,
             twins=(7, 9), truncated=trunc, cap_set=7)
    trace = []
    local, res = select(*(c[k] for k in SELECT_KEYS), dict(kf_cap=MAX_LOCAL_KF, seed=seed), trace)
    n0 = int(res[c["cap_set"]]["n_local"])
    c["kf_caps"] = (MAX_LOCAL_KF, n0 + 1, n0, n0 - 1)
    # ---- the coverage the tests rely on ----
    assert res["status"].tolist() == [EMPTY] + [OK] * (n_sets - 2) + [TRUNCATED]
    assert [int(r["n_direct"]) for r in res[:9]] == [0, 1, 14, 15, 15, 15, 15, 15, 15]
    for s in (4, 5):  # R <= 5: every draw of walk 1 accepts
        assert trace[s]["rej1"] == 0 and trace[s]["acc1"] == lengths[s] - 15
    ok = [t for t, r in zip(trace, res) if r["status"] == OK]
    for what in ("acc1", "rej1", "acc2", "rej2", "nb_bad", "nb_marked_vote", "nb_again", "nb_new"):
        assert sum(t[what] for t in ok) > 0, what
    assert set().union(*(t["conn_sizes"] for t in ok)) == {0, 3, 5, 9}
    assert any(0 < r["n_indirect"] <= 5 for r in res) and any(r["n_indirect"] >= 6 for r in res)
    a, b = c["twins"]
    assert conn[a].tobytes() == conn[b].tobytes() and frame_id[a] != frame_id[b] and local[a].tobytes() != local[b].tobytes()
    assert 17 < n0 < MAX_LOCAL_KF
    return c


SELECT_KEYS = ("conn", "vote", "kf_bad", "conn_start", "conn_list", "frame_id")


def colliding_ids(n_points, slots, want, first=2000):
    """`want` ids >= first that fall on one slot of a table of `slots`, and six whose chain starts in the last three slots."""
    by_slot = {}
    for p in range(first, n_points):
        by_slot.setdefault(hash_of(p) & (slots - 1), []).append(p)
    same = max(by_slot.values(), key=len)[:want]
    assert len(same) == want, "n_points too small for the collisions"
    wrap = (by_slot.get(slots - 1, []) + by_slot.get(slots - 2, []) + by_slot.get(slots - 3, []))[:6]
    assert len(wrap) == 6
    return same, wrap


def point_tables(n_points, seed=9):
    rng = np.random.RandomState(seed)
    return dict(pos=rng.standard_normal((n_points, 3)), normal=rng.standard_normal((n_points, 3)),
                desc=rng.randint(0, 2 ** 63, (n_points, 4)).astype(np.uint64) * np.uint64(2) + rng.randint(0, 2, (n_points, 4)).astype(np.uint64),
                ref_depth=rng.uniform(0.5, 40, n_points).astype(np.float32), ref_level=rng.randint(0, 8, n_points).astype(np.int32))


CHUNK_TOTALS = (63, 64, 65, 255, 256, 257, 1025)


def gather_case(pts_cap=64):
    """A hand-built map and sets for one pts_cap (64 or MAX_PTS): a keyframe without features, one whose features are all -1, bad
    points, the last-seen skip, a point shared by two keyframes, a point twice inside one; candidate totals at the scan-chunk edges; own
    points present / new / duplicated / -1 / bad; n_local = 0; distinct points at pts_cap - 1 / pts_cap / pts_cap + 1; 40 ids on one
    slot and a chain that wraps; stage-1 statuses passed through.  `what`: name -> set.  Asserts its own coverage."""
    n_points = 26000
    slots = table_slots(pts_cap)
    same, wrap = colliding_ids(n_points, table_slots(64), 40)
    feats = {0: [], 1: [-1] * 5, 2: [10, 11, 12, 13, 13, -1, 14, 15], 3: [14, 16, 10, 17]}
    for i, n in enumerate(CHUNK_TOTALS):  # 50 distinct points, every ninth feature empty
        feats[4 + i] = [-1 if j % 9 == 8 else 100 + (j * 7) % 50 for j in range(n)]
    base = 3000
    for i, n in enumerate((pts_cap - 1, pts_cap, pts_cap + 1)):
        feats[11 + i] = list(range(base, base + n))
    feats[14] = same + wrap + same[:3]
    n_kf = 16
    lists = [feats.get(k, []) for k in range(n_kf)]
    m = dict(feat_start=csr(lists), feat_point=np.array([p for lst in lists for p in lst], np.int32), pt_flags=np.zeros(n_points, np.uint8),
             pt_last_seen=np.full(n_points, -1, np.int32), **point_tables(n_points))
    m["pt_flags"][[11, 21]] = PT_BAD
    m["pt_last_seen"][12] = 7
    m["pt_last_seen"][100:105] = 8
    sets, what = [], {}

    def add(name, local, own, fid=1, status=OK, n_local=None):
        what[name] = len(sets)
        sets.append((local, own, fid, status, len(local) if n_local is None else n_local))

    own0 = [13, 300, 300, -1, 11, 16, 301, 21]
    add("mixed_seen", [0, 1, 2, 3], own0, fid=7)
    add("mixed", [0, 1, 2, 3], own0, fid=8)
    add("shared_reversed", [3, 2], [10])
    for i, n in enumerate(CHUNK_TOTALS):
        add(f"chunk{n}", [4 + i], [100, 400], fid=8 if n == 257 else 1)
    add("chunk127", [4, 5], [])
    add("chunk_all", [4, 5, 6, 7, 8, 9, 10, 0, 1], [401, 100])
    add("cap-1", [11], [])
    add("cap", [12], [])
    add("cap+1", [13], [])
    add("cap_by_own", [11], [base, 20])
    add("cap+1_by_own", [12], [base + 1, 20])
    add("empty_status", [], [20, 21, -1, 21, 20, 22], status=EMPTY, n_local=3)
    add("no_local", [], [22, 20])
    add("nothing", [], [])
    add("collisions", [14, 2], [same[5], wrap[0], 23])
    add("passed_truncated", [2], [20], status=TRUNCATED, n_local=0)
    add("passed_kf_overflow", [2], [20], status=KF_OVERFLOW, n_local=0)
    add("passed_bad_index", [2], [20], status=BAD_INDEX, n_local=0)
    add("last", [3, 2], [17, 15])
    kf_cap = 16
    local_kf = np.full((len(sets), kf_cap), -1, np.int32)
    sel = np.zeros(len(sets), SELECT)
    for s, (local, own, fid, status, n_local) in enumerate(sets):
        local_kf[s, :len(local)] = local
        sel[s] = (n_local, 0, 0, -1, status) if status != OK else (n_local, min(n_local, 15), 0, local[0] if local else -1, OK)
    c = dict(m=m, frame_id=np.array([x[2] for x in sets], np.int32), local_kf=local_kf, sel=sel, set_start=csr([x[1] for x in sets]),
             set_point=np.array([p for x in sets for p in x[1]], np.int32), pts_cap=pts_cap, what=what, same=same, wrap=wrap)
    # ---- the coverage the tests rely on ----
    lm, ids, n_pts, res = gather(m, c["frame_id"], local_kf, sel, c["set_start"], c["set_point"], pts_cap)
    w = what
    row = lambda name: ids[w[name], :n_pts[w[name]]].tolist()  # noqa: E731
    flag = lambda name: lm[w[name], :n_pts[w[name]]]["valid"].tolist()  # noqa: E731
    assert row("mixed_seen") == [10, 13, 14, 15, 16, 17, 300, 301] and flag("mixed_seen") == [1, 0, 1, 1, 0, 1, 0, 0]
    assert row("mixed") == [10, 12, 13, 14, 15, 16, 17, 300, 301] and tuple(res[w["mixed"]]) == (9, 5, 2, OK)
    assert row("shared_reversed") == [14, 16, 10, 17, 12, 13, 15] and flag("shared_reversed") == [1, 1, 0, 1, 1, 1, 1]
    for n in CHUNK_TOTALS:
        s = w[f"chunk{n}"]
        assert m["feat_start"][5 + CHUNK_TOTALS.index(n)] - m["feat_start"][4 + CHUNK_TOTALS.index(n)] == n and res[s]["status"] == OK
        seen = n == 257  # that set's frame id is 8: points 100 .. 104 were last seen in it, and the own point 100 is new
        assert n_pts[s] == len({p for p in feats[4 + CHUNK_TOTALS.index(n)] if p >= 0 and not (seen and p < 105)} | {100, 400})
        assert res[s]["n_own_new"] == (2 if seen else 1) and n_pts[s] > 40
    assert [int(res[w[k]]["status"]) for k in ("cap-1", "cap", "cap+1", "cap_by_own", "cap+1_by_own")] == [OK, OK, PTS_OVERFLOW, OK, PTS_OVERFLOW]
    assert [int(n_pts[w[k]]) for k in ("cap-1", "cap", "cap+1", "cap_by_own", "cap+1_by_own")] == [pts_cap - 1, pts_cap, 0, pts_cap, 0]
    assert row("empty_status") == [20, 22] and row("no_local") == [22, 20] and flag("no_local") == [0, 0] and n_pts[w["nothing"]] == 0
    assert [int(res[w[k]]["status"]) for k in ("passed_truncated", "passed_kf_overflow", "passed_bad_index")] == [TRUNCATED, KF_OVERFLOW, BAD_INDEX]
    if pts_cap == 64:
        assert len({hash_of(p) & (slots - 1) for p in same}) == 1 and all(hash_of(p) & (slots - 1) >= slots - 3 for p in wrap)
        assert res[w["collisions"]]["status"] == OK and n_pts[w["collisions"]] == 40 + 6 + 5 + 1 <= pts_cap
    return c


LONG_RANGE = 65540  # features of one keyframe: the smallest count at the tests' scale whose length and prefix have a high 16-bit half


def long_range_case(pts_cap=64):
    """Keyframe 2 has LONG_RANGE features, all -1 except three at either end; two ordinary keyframes stand in front of it and two behind,
    so that the keyframes behind it start at orders above 65 535 and its own last features win at such orders.  Asserts its coverage."""
    n_points = 64
    long_kf = [15, 20, 21] + [-1] * (LONG_RANGE - 6) + [22, 10, 23]
    lists = [[10, 11, 12, -1, 13], [12, 14, 15], long_kf, [23, 24, 11], [25, 20, -1, 26]]
    m = dict(feat_start=csr(lists), feat_point=np.array([p for lst in lists for p in lst], np.int32), pt_flags=np.zeros(n_points, np.uint8),
             pt_last_seen=np.full(n_points, -1, np.int32), **point_tables(n_points))
    sets = [([0, 1, 2, 3, 4], [21, 30, 24]), ([4, 3, 2, 1, 0], []), ([2], [22, 31]), ([2, 0], [])]
    kf_cap = 16
    local_kf = np.full((len(sets), kf_cap), -1, np.int32)
    sel = np.zeros(len(sets), SELECT)
    for s, (local, _) in enumerate(sets):
        local_kf[s, :len(local)] = local
        sel[s] = (len(local), len(local), 0, local[0], OK)
    c = dict(m=m, frame_id=np.ones(len(sets), np.int32), local_kf=local_kf, sel=sel, set_start=csr([x[1] for x in sets]),
             set_point=np.array([p for x in sets for p in x[1]], np.int32), pts_cap=pts_cap)
    lm, ids, n_pts, res = gather(m, c["frame_id"], local_kf, sel, c["set_start"], c["set_point"], pts_cap)
    assert len(long_kf) == LONG_RANGE and LONG_RANGE >> 16 == 1 and (res["status"] == OK).all()
    assert ids[0, :n_pts[0]].tolist() == [10, 11, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 30] and tuple(res[0]) == (14, 11, 1, OK)
    assert ids[1, :n_pts[1]].tolist() == [25, 20, 26, 23, 24, 11, 15, 21, 22, 10, 12, 14, 13]
    assert ids[2, :n_pts[2]].tolist() == [15, 20, 21, 22, 10, 23, 31] and ids[3, :n_pts[3]].tolist() == [15, 20, 21, 22, 10, 23, 11, 12, 13]
    return c


GATHER_KEYS = ("feat_start", "feat_point", "pt_flags", "pt_last_seen")


def edge_case(pts_cap=64, seed=SEEDS[0]):
    """Both halves; building them asserts their coverage."""
    return dict(select=select_case(seed), gather=gather_case(pts_cap))
