"""LocalBundleAdjustment::MakeLocalScene (reference Snake/Optimizer/LocalBundleAdjustment.cpp:94-346) restated statement by statement in
plain Python lists, dicts and marks -- the stamps of perKeyframeData / perPointData, no sorts beside the reference's own (:151), no hash
tables, no prefix sums -- so that it shares no method with the kernels of snake_slam_amd/csrc/scene.hip.  ``flatten`` models the order in
which snake_hip_reference.hpp:394 reads img.stereoPoints.  Semantics "snk-scene v1" (DESIGN.md section 3k).

``build_map`` generates the maps of the GPU tests and raises unless every property those tests are about occurs in them.
"""
import numpy as np

OK, SKIPPED, WINDOW_OVERFLOW, PTS_OVERFLOW, IMG_OVERFLOW, OBS_OVERFLOW, BAD_INDEX = range(7)
PT_BAD, PT_FAR, PT_CONST = 1, 2, 4
THREADS = 256  # a chunk of the kernels: 256 points, 256 observations
MAX_WINDOW, MAX_IMG, MAX_PTS, MAX_KF = 64, 4096, 16384, 32768
RPC_DTYPE = np.dtype([("img1", "<i4"), ("img2", "<i4"), ("rel_pose", "<f8", 7), ("weight_rotation", "<f8"), ("weight_translation", "<f8")])


def connections_of(t, k):
    """GetBestCovisibilityKeyFrames' store: keyframe k's connections ascending by (weight, kf), as keyframe slots."""
    return [int(x) for x in t["conn_list"]["kf"][t["conn_start"][k]:t["conn_start"][k + 1]]]


def window(t, q, n_neighbours=15, n_last=20, win_cap=36):
    """:77, :124-151.  Returns (keyframes, status)."""
    bad, prev = t["kf_bad"], t["kf_prev"]
    if bad[q]:  # :77
        return [], SKIPPED
    conns = connections_of(t, q)
    tmp = conns[len(conns) - min(n_neighbours, len(conns)):]  # :126, KeyframeGraph.cpp:62: a view of the back
    tmp.append(q)  # :127
    k, i = int(prev[q]), 0
    while k != -1 and i < n_last:  # :131-135
        tmp.append(k)
        k, i = int(prev[k]), i + 1
    local_for = {}  # perKeyframeData[..].mnBALocalForKF == currentOptimizationId
    keyframes = []
    for other in tmp:  # :139-149
        if local_for.get(other):
            continue
        local_for[other] = True
        if not bad[other]:
            keyframes.append(other)
    keyframes.sort()  # :151
    if len(keyframes) > win_cap:
        return [], WINDOW_OVERFLOW
    return keyframes, OK


def make_scene(t, keyframes, pt_cap, img_cap, obs_cap, gyro_weight=0.0, acc_weight=0.0):
    """:154-346 for the window `keyframes`.  Returns a dict: status, the counts and the arrays in the layout of snk_scene_out (one row)."""
    bad, fs, fp, flags = t["kf_bad"], t["feat_start"], t["feat_point"], t["pt_flags"]
    os_, obs = t["obs_start"], t["obs"]
    fail = lambda status: dict(status=status, n_window=0, n_img=0, n_pt=0, n_obs=0, n_rpc=0)  # noqa: E731
    local_kf = {k: True for k in keyframes}  # the stamps stage 1 left on the survivors; a bad candidate is no image either way
    # :154-167
    local_pt, map_points = {}, []
    for k in keyframes:
        for f in range(fs[k], fs[k + 1]):
            mp = int(fp[f])
            if mp < 0 or flags[mp] & PT_BAD:
                continue
            if not local_pt.get(mp):
                map_points.append(mp)
                local_pt[mp] = True
    if len(map_points) > pt_cap:
        return fail(PTS_OVERFLOW)
    # :170-184
    fixed_for, fixed = {}, []
    for mp in map_points:
        for o in range(os_[mp], os_[mp + 1]):
            kf = int(obs[o][0])
            if not local_kf.get(kf) and not fixed_for.get(kf):
                fixed_for[kf] = True
                if not bad[kf]:
                    fixed.append(kf)
    # :200-244
    images, id_in_scene, kfmapinv = [], {}, []
    for kf in keyframes:
        id_in_scene[kf] = len(images)
        images.append(dict(constant=0, pose=t["kf_pose"][kf], stereo=[]))
        kfmapinv.append(kf)
    for kf in fixed:
        if bad[kf]:
            continue
        id_in_scene[kf] = len(images)
        images.append(dict(constant=1, pose=t["kf_pose"][kf], stereo=[]))
        kfmapinv.append(kf)
    if len(images) > img_cap:
        return fail(IMG_OVERFLOW)
    # :246-293
    world, mpmapinv = [], []
    for mp in map_points:
        wpid = len(world)
        mpmapinv.append(mp)
        wp = dict(p=t["pt_pos"][mp], constant=1 if flags[mp] & PT_CONST else 0)
        world.append(wp)
        n_edges = 0
        for o in range(os_[mp], os_[mp + 1]):
            kf, fi = int(obs[o][0]), int(obs[o][1])
            if bad[kf]:
                continue
            n_edges += 1
            f = fs[kf] + fi
            weight = t["level_inv_sq_scale"][t["feat_octave"][f]]
            img = images[id_in_scene[kf]]
            if img["constant"] and wp["constant"]:
                continue
            img["stereo"].append(dict(wp=wpid, uv=t["feat_uv"][f], depth=t["feat_depth"][f], weight=weight, src=(kf, fi)))
        wp["valid"] = 1 if n_edges > 0 else 0
    # flatten (snake_hip_reference.hpp:394): image by image, inside an image in push order
    rec = [(i, ip) for i, img in enumerate(images) for ip in img["stereo"]]
    if len(rec) > obs_cap:
        return fail(OBS_OVERFLOW)
    # :295-346
    rpcs = []
    if t.get("kf_time") is not None and gyro_weight > 0:
        for i in range(1, len(keyframes)):
            a, b = keyframes[i - 1], keyframes[i]
            if t["kf_time"][a] != t["kf_imu_begin"][b] or t["kf_time"][b] != t["kf_imu_end"][b]:
                continue
            if not t["kf_preint_valid"][b]:
                continue
            dt = float(t["kf_time"][b]) - float(t["kf_time"][a])
            w_rot = float(gyro_weight) / dt
            w_tr = float(t["kf_rpc"]["weight_translation"][b]) * float(acc_weight) / dt
            if dt > 2:
                w_rot, w_tr = 0.0, 0.0
            rpcs.append((id_in_scene[a], id_in_scene[b], t["kf_rpc"]["rel_pose"][b], w_rot, w_tr))
    r = dict(status=OK, n_window=len(keyframes), n_img=len(images), n_pt=len(world), n_obs=len(rec), n_rpc=len(rpcs))
    r["img_kf"] = np.array(kfmapinv, np.int32).reshape(-1)
    r["pose"] = np.array([im["pose"] for im in images], np.float64).reshape(-1, 7)
    r["img_const"] = np.array([im["constant"] for im in images], np.uint8).reshape(-1)
    r["pt_id"] = np.array(mpmapinv, np.int32).reshape(-1)
    r["pt"] = np.array([w["p"] for w in world], np.float64).reshape(-1, 3)
    r["pt_const"] = np.array([w["constant"] for w in world], np.uint8).reshape(-1)
    r["pt_valid"] = np.array([w["valid"] for w in world], np.uint8).reshape(-1)
    r["obs_img"] = np.array([i for i, _ in rec], np.int32).reshape(-1)
    r["obs_pt"] = np.array([ip["wp"] for _, ip in rec], np.int32).reshape(-1)
    r["obs_uv"] = np.array([ip["uv"] for _, ip in rec], np.float32).reshape(-1, 2).astype(np.float64)
    r["obs_depth"] = np.array([ip["depth"] for _, ip in rec], np.float32).reshape(-1).astype(np.float64)
    r["obs_weight"] = np.array([ip["weight"] for _, ip in rec], np.float32).reshape(-1).astype(np.float64)
    r["obs_src"] = np.array([ip["src"] for _, ip in rec], np.int32).reshape(-1, 2)
    rp = np.zeros(len(rpcs), RPC_DTYPE)
    for i, (i1, i2, rel, w_rot, w_tr) in enumerate(rpcs):
        rp[i] = (i1, i2, rel, w_rot, w_tr)
    r["rpc"] = rp
    return r


def local_scene(t, q, n_neighbours=15, n_last=20, win_cap=36, pt_cap=MAX_PTS, img_cap=MAX_IMG, obs_cap=1 << 20, gyro_weight=0.0, acc_weight=0.0):
    """MakeLocalScene(q): (window keyframes, scene dict)."""
    kfs, status = window(t, q, n_neighbours, n_last, win_cap)
    if status != OK:
        return kfs, dict(status=status, n_window=0, n_img=0, n_pt=0, n_obs=0, n_rpc=0)
    return kfs, make_scene(t, kfs, pt_cap, img_cap, obs_cap, gyro_weight, acc_weight)


# ---- the maps of the GPU tests ------------------------------------------------------------------------------------------------------------

def build_map(seed=3, n_kf=120, feats=64, stride=24, band=200, n_levels=8, imu=True):
    """A map as the tables of snk_scene_map plus the connection store.  Keyframe k lists points of the band [k * stride, k * stride + band);
    the two sides of the map are written apart, as the entry points read them.  Keyframe 7 has no features, keyframe 5 no connections."""
    rng = np.random.RandomState(seed)
    n_points = n_kf * stride + band
    kf_bad = (rng.rand(n_kf) < 0.12).astype(np.uint8)
    kf_prev = np.arange(-1, n_kf - 1).astype(np.int32)
    for k in (40, 41, 77):  # chains that end early: 41 reaches -1 at once, 45 after four steps
        kf_prev[k] = -1
    kf_bad[[41, 45, 60, 100, 101]] = 0
    kf_bad[[43, 59, 98]] = 1  # bad keyframes in the chains of 45, 60 and 100
    kf_bad[50] = 1  # a bad query
    n_feat_of = np.full(n_kf, feats)
    n_feat_of[7] = 0
    feat_start = np.concatenate([[0], np.cumsum(n_feat_of)]).astype(np.int32)
    n_feat = int(feat_start[-1])
    feat_point = np.full(n_feat, -1, np.int32)
    for k in range(n_kf):
        a, b = feat_start[k], feat_start[k + 1]
        ids = k * stride + rng.randint(0, band, b - a)
        ids[rng.rand(b - a) < 0.2] = -1
        feat_point[a:b] = ids
        if b - a >= 8:  # a point listed twice in one keyframe
            feat_point[a + 5] = feat_point[a + 1] = k * stride + 3
    pt_flags = (rng.rand(n_points) < 0.06).astype(np.uint8) * PT_BAD
    pt_flags |= (rng.rand(n_points) < 0.15).astype(np.uint8) * PT_CONST
    pt_flags |= (rng.rand(n_points) < 0.1).astype(np.uint8) * PT_FAR
    lists = [[] for _ in range(n_points)]
    for k in range(n_kf):
        for f in range(feat_start[k], feat_start[k + 1]):
            if feat_point[f] >= 0:
                lists[feat_point[f]].append((k, f - feat_start[k]))
    bad_kfs = np.flatnonzero(kf_bad)
    for p in range(n_points):
        rng.shuffle(lists[p])  # the list order is the order of insertion, not of the ids
        if p % 37 == 5 and lists[p]:  # seen only by bad keyframes: still listed by the keyframes that list it
            lists[p] = [(int(bk), 0) for bk in bad_kfs[:2] if feat_start[bk + 1] > feat_start[bk]]
            pt_flags[p] &= ~np.uint8(PT_BAD)
        if p % 41 == 9 and lists[p]:  # seen from far away: fixed cameras outside every band
            far = (p // stride + 60) % n_kf
            if feat_start[far + 1] > feat_start[far]:
                lists[p].append((far, 2))
    obs_start = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    obs = np.array([o for x in lists for o in x], np.int32).reshape(-1, 2)
    conn_lists = []
    for k in range(n_kf):
        if k == 5:
            conn_lists.append([])
            continue
        others = sorted(set(int(x) for x in np.clip(k + rng.randint(-12, 13, rng.randint(3, 25)), 0, n_kf - 1)) - {k})
        w = rng.randint(15, 200, len(others))
        conn_lists.append(sorted(zip(w.tolist(), others)))
    conn_start = np.concatenate([[0], np.cumsum([len(x) for x in conn_lists])]).astype(np.int32)
    conn_list = np.zeros(int(conn_start[-1]), np.dtype([("weight", "<i4"), ("kf", "<i4")]))
    flat = [c for x in conn_lists for c in x]
    conn_list["weight"], conn_list["kf"] = [c[0] for c in flat], [c[1] for c in flat]
    quat = rng.randn(n_kf, 4)
    kf_pose = np.concatenate([quat / np.linalg.norm(quat, axis=1, keepdims=True), rng.randn(n_kf, 3)], axis=1)
    depth = rng.uniform(0.5, 30.0, n_feat).astype(np.float32)
    depth[rng.rand(n_feat) < 0.3] = -1.0
    depth[rng.rand(n_feat) < 0.05] = 0.0
    t = dict(kf_bad=kf_bad, kf_prev=kf_prev, kf_pose=kf_pose, feat_start=feat_start, feat_point=feat_point, feat_depth=depth,
             feat_uv=rng.uniform(0, 640, (n_feat, 2)).astype(np.float32), feat_octave=rng.randint(0, n_levels, n_feat).astype(np.int32),
             obs_start=obs_start, obs=obs, pt_flags=pt_flags, pt_pos=rng.randn(n_points, 3) * 5,
             level_inv_sq_scale=(1.0 / (np.float32(1.2) ** np.arange(n_levels, dtype=np.float32)) ** 2).astype(np.float32),
             conn_start=conn_start, conn_list=conn_list)
    if imu:
        time = np.cumsum(rng.choice([0.25, 0.5, 0.75], n_kf))
        time[90:] += 3.0  # dt > 2 between 89 and 90
        begin, end = np.concatenate([[0.0], time[:-1]]), time.copy()
        valid = np.ones(n_kf, np.uint8)
        begin[93], end[95], valid[97] = begin[93] + 0.125, end[95] - 0.125, 0
        rpc = np.zeros(n_kf, RPC_DTYPE)
        rpc["img1"], rpc["img2"] = -7, -9  # not read
        rpc["rel_pose"], rpc["weight_rotation"], rpc["weight_translation"] = rng.randn(n_kf, 7), rng.rand(n_kf), rng.uniform(0.1, 3.0, n_kf)
        t.update(kf_time=time, kf_imu_begin=begin, kf_imu_end=end, kf_preint_valid=valid, kf_rpc=rpc)
    return t


QUERIES = [100, 45, 41, 5, 50, 60, 7, 110, 20]

LONG_RANGE = 65540  # features of one keyframe: the smallest count at the tests' scale whose length and prefix have a high 16-bit half
LONG_QUERIES = [4, 2]


def long_range_map(seed=5, n_levels=8):
    """Keyframe 2 has LONG_RANGE features, all -1 except three at either end.  The window of query 4 is its chain 0 .. 4: two ordinary
    keyframes in front of the long one and two behind, which start at orders above 65 535; the window of query 2 ends with the long one.
    Keyframe 5 is outside both windows and sees two of the points: a fixed camera.  No connections, no IMU tables."""
    rng = np.random.RandomState(seed)
    lists = [[10, 11, 12, -1, 13], [12, 14, 15], [15, 20, 21] + [-1] * (LONG_RANGE - 6) + [22, 10, 23], [23, 24, 11], [25, 20, -1, 26], [22, 13]]
    n_kf, n_points = len(lists), 32
    feat_start = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    feat_point = np.array([p for x in lists for p in x], np.int32)
    n_feat = len(feat_point)
    seen = [[] for _ in range(n_points)]
    for k, x in enumerate(lists):
        for f, p in enumerate(x):
            if p >= 0:
                seen[p].append((k, f))
    pt_flags = np.zeros(n_points, np.uint8)
    pt_flags[[14, 22]] = PT_CONST
    quat = rng.randn(n_kf, 4)
    depth = rng.uniform(0.5, 30.0, n_feat).astype(np.float32)
    depth[::3] = -1.0
    t = dict(kf_bad=np.zeros(n_kf, np.uint8), kf_prev=np.array([-1, 0, 1, 2, 3, -1], np.int32),
             kf_pose=np.concatenate([quat / np.linalg.norm(quat, axis=1, keepdims=True), rng.randn(n_kf, 3)], axis=1),
             feat_start=feat_start, feat_point=feat_point, feat_depth=depth, feat_uv=rng.uniform(0, 640, (n_feat, 2)).astype(np.float32),
             feat_octave=rng.randint(0, n_levels, n_feat).astype(np.int32),
             obs_start=np.concatenate([[0], np.cumsum([len(x) for x in seen])]).astype(np.int32),
             obs=np.array([o for x in seen for o in x], np.int32).reshape(-1, 2), pt_flags=pt_flags, pt_pos=rng.randn(n_points, 3) * 5,
             level_inv_sq_scale=(1.0 / (np.float32(1.2) ** np.arange(n_levels, dtype=np.float32)) ** 2).astype(np.float32),
             conn_start=np.zeros(n_kf + 1, np.int32), conn_list=np.zeros(0, np.dtype([("weight", "<i4"), ("kf", "<i4")])))
    (w4, s4), (w2, s2) = (local_scene(t, q, pt_cap=64, img_cap=16, obs_cap=256) for q in LONG_QUERIES)
    assert w4 == [0, 1, 2, 3, 4] and w2 == [0, 1, 2] and s4["status"] == OK and s2["status"] == OK and LONG_RANGE >> 16 == 1
    assert s4["pt_id"].tolist() == [10, 11, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26] and s4["img_kf"].tolist() == [0, 1, 2, 3, 4, 5]
    assert s2["pt_id"].tolist() == [10, 11, 12, 13, 14, 15, 20, 21, 22, 23] and s2["img_kf"].tolist() == [0, 1, 2, 3, 5, 4]
    return t


def stream_chunks(t, scene):
    """(chunk of the walk, image or -1) of every observation of the scene's points: 256 points per chunk, 256 observations per sub-chunk."""
    image_of = {int(k): i for i, k in enumerate(scene["img_kf"])}
    out, chunk = [], 0
    for base in range(0, scene["n_pt"], THREADS):
        i = 0
        for p in scene["pt_id"][base:base + THREADS]:
            for o in range(t["obs_start"][p], t["obs_start"][p + 1]):
                out.append((chunk + i // THREADS, image_of.get(int(t["obs"][o][0]), -1)))
                i += 1
        chunk += (i + THREADS - 1) // THREADS
    return out


def coverage(t, queries=QUERIES, gyro_weight=2.0, acc_weight=0.5, **kw):
    """The restatement on `queries` and the set of properties that occurred; ``require_coverage`` raises on a missing one."""
    seen, results = set(), []
    bad = t["kf_bad"]
    for q in queries:
        kfs, sc = local_scene(t, q, gyro_weight=gyro_weight, acc_weight=acc_weight, **kw)
        results.append((kfs, sc))
        conns = connections_of(t, q)
        nb = conns[len(conns) - min(15, len(conns)):]
        chain, k = [], int(t["kf_prev"][q])
        while k != -1 and len(chain) < 20:
            chain.append(k)
            k = int(t["kf_prev"][k])
        if sc["status"] == SKIPPED:
            seen.add("bad query")
            continue
        seen |= {"no connections"} if not conns else set()
        seen |= {"neighbour in chain"} if set(nb) & set(chain) else set()
        seen |= {"bad neighbour"} if any(bad[x] for x in nb) else set()
        seen |= {"bad in chain"} if any(bad[x] for x in chain) else set()
        seen |= {"short chain"} if 0 < len(chain) < 20 else set()
        seen |= {"chain ends at once"} if not chain else set()
        if sc["status"] != OK:
            continue
        seen |= {"keyframe without features"} if any(t["feat_start"][x] == t["feat_start"][x + 1] for x in kfs) else set()
        for x in kfs:
            ids = [p for p in t["feat_point"][t["feat_start"][x]:t["feat_start"][x + 1]] if p >= 0 and not t["pt_flags"][p] & PT_BAD]
            seen |= {"point twice in a keyframe"} if len(ids) != len(set(ids)) else set()
        chunks = stream_chunks(t, sc)
        if chunks and chunks[-1][0] + 1 >= 5 and sc["n_pt"] > 2 * THREADS:
            seen.add("bases carry")
        per_image = {}
        for c, img in chunks:
            per_image.setdefault(img, set()).add(c)
        seen |= {"image in three chunks"} if any(len(v) >= 3 for i, v in per_image.items() if i >= 0) else set()
        for j, p in enumerate(sc["pt_id"]):
            lst = [tuple(o) for o in t["obs"][t["obs_start"][p]:t["obs_start"][p + 1]].tolist()]
            ks = [o[0] for o in lst if not bad[o[0]]]
            seen |= {"bad observer"} if any(bad[o[0]] for o in lst) else set()
            seen |= {"observed twice by a keyframe"} if len(ks) != len(set(ks)) else set()
            seen |= {"only bad observers"} if lst and not ks and not sc["pt_valid"][j] else set()
            if sc["pt_const"][j] and sc["pt_valid"][j] and any(k not in kfs for k in ks):
                seen.add("constant point at a fixed camera")
        seen |= {"depth <= 0"} if (sc["obs_depth"] <= 0).any() else set()
        seen |= {"every octave"} if len(set(sc["obs_weight"].tolist())) == len(t["level_inv_sq_scale"]) else set()
        if t.get("kf_time") is not None:
            for a, b in zip(kfs[:-1], kfs[1:]):
                gates = (t["kf_time"][a] == t["kf_imu_begin"][b], t["kf_time"][b] == t["kf_imu_end"][b], bool(t["kf_preint_valid"][b]))
                if all(gates):
                    seen.add("imu dt > 2" if t["kf_time"][b] - t["kf_time"][a] > 2 else "imu pass")
                for i, name in enumerate(("imu begin fails", "imu end fails", "imu invalid")):
                    if not gates[i] and all(gates[:i] + gates[i + 1:]):
                        seen.add(name)
    return seen, results


PROPERTIES = ["bad query", "no connections", "neighbour in chain", "bad neighbour", "bad in chain", "short chain", "chain ends at once",
              "keyframe without features", "point twice in a keyframe", "bases carry", "image in three chunks", "bad observer",
              "observed twice by a keyframe", "only bad observers", "constant point at a fixed camera", "depth <= 0", "every octave", "imu pass",
              "imu dt > 2", "imu begin fails", "imu end fails", "imu invalid"]


def require_coverage(t, queries=QUERIES, **kw):
    seen, results = coverage(t, queries, **kw)
    missing = [p for p in PROPERTIES if p not in seen]
    if missing:
        raise AssertionError(f"the generated map does not contain: {missing}")
    return results
