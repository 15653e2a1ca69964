"""GPU: the keyframe-rate chain covisibility update -> snk_scene_window -> snk_scene_gather -> snk_ba_set_problem -> snk_ba_solve on a map
made from synth.ba_scene (12 keyframes on an arc, 300 points): the connection store is what snk_covis_update emits, the window of the
last keyframe is a part of the map and the other observers become fixed cameras.  The arrays handed to the BA equal the restatement's
(tests/scene_numpy.py) byte for byte, and the solution is within the BA's bound (1e-5 RMSE, README) of the oracle's BA on the
restatement's scene."""
import numpy as np
import pytest

import scene_numpy as M
from test_ba_gpu import TOL, rmse

pytestmark = pytest.mark.gpu
N_LEVELS = 4


def map_of(scene):
    """The scene's observations as a map: keyframe k's features are its observations in order, a point's list is in the same order."""
    n_kf, n_pt = len(scene["pose"]), len(scene["pt"])
    levels = (1.0 / 1.44 ** np.arange(N_LEVELS)).astype(np.float32)
    by_kf = [np.flatnonzero(scene["obs_img"] == k) for k in range(n_kf)]
    feat_start = np.concatenate([[0], np.cumsum([len(x) for x in by_kf])]).astype(np.int32)
    order = np.concatenate(by_kf)
    index_in_kf = np.zeros(len(order), np.int32)
    for x in by_kf:
        index_in_kf[x] = np.arange(len(x))
    lists = [[] for _ in range(n_pt)]
    for o in range(len(order)):
        lists[scene["obs_pt"][o]].append((int(scene["obs_img"][o]), int(index_in_kf[o])))
    octave = np.rint(np.log(1.0 / scene["obs_weight"][order]) / np.log(1.44)).astype(np.int32)
    assert np.allclose(levels[octave], scene["obs_weight"][order], rtol=1e-6)
    return dict(kf_bad=np.zeros(n_kf, np.uint8), kf_prev=np.arange(-1, n_kf - 1).astype(np.int32), kf_pose=scene["pose"].copy(), feat_start=feat_start,
                feat_point=scene["obs_pt"][order].astype(np.int32), feat_depth=scene["obs_depth"][order].astype(np.float32),
                feat_uv=scene["obs_uv"][order].astype(np.float32), feat_octave=octave,
                obs_start=np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32),
                obs=np.array([o for x in lists for o in x], np.int32).reshape(-1, 2), pt_flags=np.zeros(n_pt, np.uint8), pt_pos=scene["pt"].copy(),
                level_inv_sq_scale=levels)


def test_covis_window_gather_and_ba_against_the_restatement_and_the_oracle(orc):
    from snake_slam_amd import scene as S, synth
    from snake_slam_amd.ba import BARec, lba_options
    from snake_slam_amd.covis import CovisibilityGraph

    src, _ = synth.ba_scene(n_kf=12, n_pt=300, obs_per_pt=5, seed=77)
    t = map_of(src)
    n_kf = 12
    g = CovisibilityGraph(th=15, th_depth=40.0, cap=16)
    conn, res = g.update(t["kf_bad"], t["obs_start"], t["obs"], t["pt_flags"], t["feat_start"], t["feat_point"], t["feat_depth"], np.arange(n_kf))
    g.close()
    assert (res["n_found"] == res["n_conn"]).all() and (res["n_conn"] > 0).all()
    t["conn_start"] = np.concatenate([[0], np.cumsum(res["n_conn"])]).astype(np.int32)
    t["conn_list"] = np.concatenate([conn[k, :res["n_conn"][k]] for k in range(n_kf)])
    params = dict(n_neighbours=3, n_last=4, win_cap=12)
    caps = dict(pt_cap=512, img_cap=16, obs_cap=2048)
    kfs, want = M.local_scene(t, n_kf - 1, **params, **caps)
    assert want["status"] == M.OK and 5 <= len(kfs) < want["n_img"] and want["img_const"].sum() >= 2  # a window and fixed cameras

    b = S.LocalSceneBuilder(params)
    win, wres = b.window([n_kf - 1], t["kf_bad"], t["kf_prev"], t["conn_start"], t["conn_list"])
    assert win[0, :len(kfs)].tolist() == kfs and int(wres[0]["n_window"]) == len(kfs)
    o = b.gather(t, win, wres, **caps)
    b.close()
    handed = S.ba_scene(o, 0, src["K"], src["bf"])
    for name in ("pose", "img_const", "pt", "pt_const", "obs_img", "obs_pt", "obs_uv", "obs_depth", "obs_weight"):
        assert np.ascontiguousarray(handed[name]).tobytes() == np.ascontiguousarray(want[name]).tobytes(), name
    assert o["img_kf"][0, :want["n_img"]].tolist() == want["img_kf"].tolist() and o["pt_id"][0, :want["n_pt"]].tolist() == want["pt_id"].tolist()
    assert handed["rpc"].size == 0

    ba = BARec(lba_options())
    ba.create(handed)
    ci, cf = ba.solve()
    pose, pt, _ = ba.state(0)
    ba.close()
    oracle_scene = dict({k: want[k] for k in ("pose", "img_const", "pt", "pt_const", "obs_img", "obs_pt", "obs_uv", "obs_depth", "obs_weight")},
                        K=src["K"], bf=src["bf"])
    wpose, wpt, wci, wcf, _ = orc.ba_solve(oracle_scene, orc.ba_options())
    assert abs(ci[0] - wci) <= 1e-9 * max(1.0, wci) and cf[0] < ci[0]
    assert rmse(pt, wpt) <= TOL and rmse(pose[:, 4:], wpose[:, 4:]) <= TOL and rmse(pose[:, :4], wpose[:, :4]) <= TOL
