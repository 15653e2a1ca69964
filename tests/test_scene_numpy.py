"""CPU: the restatement of MakeLocalScene (tests/scene_numpy.py) on three maps small enough to work through with
LocalBundleAdjustment.cpp:94-346 beside them; the expected arrays are typed out below.  Feature f of a map has uv (f, f + 0.5), depth f + 1 and
octave f % 2, the levels weigh 1 and 0.25, so every record's values follow from its source (kf, feature)."""
import numpy as np

import scene_numpy as M


def tables(kf_bad, kf_prev, feats, flags, obs_lists, conns):
    """feats: per keyframe its point ids; obs_lists: per point its (kf, feature) list; conns: per keyframe its (weight, kf) list."""
    n_kf, n_feat = len(kf_bad), sum(len(f) for f in feats)
    conn_list = np.zeros(sum(len(c) for c in conns), np.dtype([("weight", "<i4"), ("kf", "<i4")]))
    flat = [x for c in conns for x in c]
    conn_list["weight"], conn_list["kf"] = [x[0] for x in flat], [x[1] for x in flat]
    return dict(kf_bad=np.array(kf_bad, np.uint8), kf_prev=np.array(kf_prev, np.int32), kf_pose=np.arange(n_kf * 7, dtype=np.float64).reshape(n_kf, 7),
                feat_start=np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int32),
                feat_point=np.array([p for f in feats for p in f], np.int32), feat_depth=np.arange(1, n_feat + 1, dtype=np.float32),
                feat_uv=np.stack([np.arange(n_feat), np.arange(n_feat) + 0.5], axis=1).astype(np.float32), feat_octave=(np.arange(n_feat) % 2).astype(np.int32),
                obs_start=np.concatenate([[0], np.cumsum([len(o) for o in obs_lists])]).astype(np.int32),
                obs=np.array([x for o in obs_lists for x in o], np.int32).reshape(-1, 2), pt_flags=np.array(flags, np.uint8),
                pt_pos=np.arange(len(flags) * 3, dtype=np.float64).reshape(-1, 3) * 0.5, level_inv_sq_scale=np.array([1.0, 0.25], np.float32),
                conn_start=np.concatenate([[0], np.cumsum([len(c) for c in conns])]).astype(np.int32), conn_list=conn_list)


def check(t, sc, img_kf, img_const, pt_id, pt_const, pt_valid, obs_img, obs_pt, obs_src):
    assert (sc["status"], sc["n_img"], sc["n_pt"], sc["n_obs"]) == (M.OK, len(img_kf), len(pt_id), len(obs_img))
    assert sc["img_kf"].tolist() == img_kf and sc["img_const"].tolist() == img_const
    assert sc["pt_id"].tolist() == pt_id and sc["pt_const"].tolist() == pt_const and sc["pt_valid"].tolist() == pt_valid
    assert sc["obs_img"].tolist() == obs_img and sc["obs_pt"].tolist() == obs_pt and sc["obs_src"].tolist() == [list(s) for s in obs_src]
    f = [int(t["feat_start"][k]) + i for k, i in obs_src]
    assert sc["obs_uv"].tolist() == [[float(x), x + 0.5] for x in f] and sc["obs_depth"].tolist() == [x + 1.0 for x in f]
    assert sc["obs_weight"].tolist() == [1.0 if x % 2 == 0 else 0.25 for x in f]
    assert np.array_equal(sc["pose"], t["kf_pose"][img_kf]) and np.array_equal(sc["pt"], t["pt_pos"][pt_id])
    assert sc["obs_uv"].dtype == sc["obs_depth"].dtype == sc["obs_weight"].dtype == np.float64


def test_a_chain_of_four_keyframes_and_the_image_major_order():
    t = tables([0, 0, 0, 0], [-1, 0, 1, 2], [[0, 1], [1, 2], [2, -1], [3, 1]], [0, 0, M.PT_CONST, 0],
               [[(0, 0)], [(3, 1), (0, 1), (1, 0)], [(1, 1), (2, 0)], [(3, 0)]], [[], [], [], [(20, 1)]])
    kfs, sc = M.local_scene(t, 3, n_neighbours=15, n_last=1)
    assert kfs == [1, 2, 3]  # the neighbour 1, the query, one step of the chain
    # points 1, 2 from keyframe 1, 3 from keyframe 3 (2 and 1 again are no new points); keyframe 0 sees point 1: the fixed camera
    check(t, sc, [1, 2, 3, 0], [0, 0, 0, 1], [1, 2, 3], [0, 1, 0], [1, 1, 1], [0, 0, 1, 2, 2, 3], [0, 1, 1, 0, 2, 0],
          [(1, 0), (1, 1), (2, 0), (3, 1), (3, 0), (0, 1)])
    assert M.local_scene(t, 3, n_last=1, win_cap=2)[1]["status"] == M.WINDOW_OVERFLOW
    assert M.local_scene(t, 3, n_last=1, obs_cap=5)[1]["status"] == M.OBS_OVERFLOW and M.local_scene(t, 3, n_last=1, obs_cap=6)[1]["status"] == M.OK
    assert M.local_scene(t, 3, n_last=1, img_cap=3)[1]["status"] == M.IMG_OVERFLOW and M.local_scene(t, 3, n_last=1, pt_cap=2)[1]["status"] == M.PTS_OVERFLOW
    assert M.local_scene(t, 0)[0] == [0] and M.local_scene(t, 3, n_last=20)[0] == [0, 1, 2, 3]


def test_bad_keyframes_constant_points_and_a_point_listed_twice():
    t = tables([0, 1, 0, 0, 0, 0], [-1, 0, 1, 2, 3, -1], [[0], [0], [1], [], [2, 2], [1, 2, 0]], [M.PT_CONST, M.PT_BAD, 0],
               [[(5, 2), (1, 0), (0, 0)], [(2, 0), (5, 0)], [(4, 0), (5, 1), (4, 1)]], [[], [], [], [], [(5, 1), (9, 0)], []])
    kfs, sc = M.local_scene(t, 4, n_neighbours=2, n_last=3)
    assert kfs == [0, 2, 3, 4]  # the bad neighbour 1 is dropped; the chain 3, 2, 1 spends its third step on the bad keyframe
    assert M.local_scene(t, 4, n_neighbours=2, n_last=4)[0] == [0, 2, 3, 4] and M.local_scene(t, 4, n_neighbours=0, n_last=2)[0] == [2, 3, 4]
    # point 1 is bad; point 2 stands twice in keyframe 4.  Keyframe 5 is the fixed camera; the bad keyframe 1 is none.  The constant point 0
    # loses its record at the constant image 4 but stays valid; point 2 is seen twice by keyframe 4
    check(t, sc, [0, 2, 3, 4, 5], [0, 0, 0, 0, 1], [0, 2], [1, 0], [1, 1], [0, 3, 3, 4], [0, 1, 1, 1], [(0, 0), (4, 0), (4, 1), (5, 1)])
    assert M.local_scene(t, 1)[1] == dict(status=M.SKIPPED, n_window=0, n_img=0, n_pt=0, n_obs=0, n_rpc=0)
    assert M.local_scene(t, 5)[0] == [5]  # no connections, the chain ends at once


def test_a_point_seen_only_by_a_bad_keyframe_and_the_imu_constraints():
    t = tables([0, 0, 1], [-1, 0, 1], [[0], [1], [0]], [0, 0], [[(2, 0)], [(1, 0)]], [[], [], []])
    rpc = np.zeros(3, M.RPC_DTYPE)
    rpc["rel_pose"], rpc["weight_translation"], rpc["img1"] = np.arange(21).reshape(3, 7), [0.0, 4.0, 0.0], 99
    t.update(kf_time=np.array([1.0, 1.5, 9.0]), kf_imu_begin=np.array([0.0, 1.0, 1.5]), kf_imu_end=np.array([1.0, 1.5, 9.0]),
             kf_preint_valid=np.array([1, 1, 1], np.uint8), kf_rpc=rpc)
    kfs, sc = M.local_scene(t, 1, gyro_weight=3.0, acc_weight=0.5)
    assert kfs == [0, 1]
    check(t, sc, [0, 1], [0, 0], [0, 1], [0, 0], [0, 1], [1], [1], [(1, 0)])  # point 0 is kept, without a record and not valid
    r = sc["rpc"][0]  # dt = 0.5: 3 / 0.5 and 4 * 0.5 / 0.5
    assert sc["n_rpc"] == 1 and (int(r["img1"]), int(r["img2"]), float(r["weight_rotation"]), float(r["weight_translation"])) == (0, 1, 6.0, 4.0)
    assert r["rel_pose"].tolist() == list(range(7, 14))
    assert M.local_scene(t, 1, gyro_weight=0.0, acc_weight=0.5)[1]["n_rpc"] == 0
    for key, value, n in (("kf_imu_begin", 1.25, 0), ("kf_imu_end", 1.25, 0), ("kf_preint_valid", 0, 0)):
        u = dict(t, **{key: t[key].copy()})
        u[key][1] = value
        assert M.local_scene(u, 1, gyro_weight=3.0, acc_weight=0.5)[1]["n_rpc"] == n
    u = dict(t, kf_time=np.array([1.0, 3.5, 9.0]), kf_imu_end=np.array([1.0, 3.5, 9.0]))
    assert M.local_scene(u, 1, gyro_weight=3.0, acc_weight=0.5)[1]["rpc"][["weight_rotation", "weight_translation"]].tolist() == [(0.0, 0.0)]  # dt = 2.5 > 2
    assert M.local_scene(t, 2)[1]["status"] == M.SKIPPED
