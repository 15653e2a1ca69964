"""GPU: the device-resident chain vote -> select -> gather -> fine match on a synthetic scene of 40 keyframes and a batch of 8 frames:
snk_covis_vote_batch_dev, snk_lmap_select_batch_dev, snk_lmap_gather_batch_dev and snk_match_project_fine_batch_ro_dev on one stream, each
reading what the one before left in HBM, no host copy in between.  Expected, frame by frame and exactly: the matches, visible flags and
counts that the oracle's fine matcher returns on the local map that the restatements (tests/covis_numpy.py, tests/localmap_numpy.py)
assemble from the same tables."""
import numpy as np
import pytest

import covis_numpy as CM
import localmap_numpy as M
import track_helpers as T

pytestmark = pytest.mark.gpu
N_KF, BATCH, PER_FRAME, OBSERVERS = 40, 8, 180, 8
VOTE_CAP, KF_CAP, PTS_CAP = 64, 48, 2048


def scene(orc):
    """Eight tracking cases (a frame, its pose and the 180 world points it looks at); their points are the map's 1 440 points, point p
    observed by the keyframes p % 40 .. p % 40 + 7, so that keyframes up to seven apart share at least 36 points."""
    rng = np.random.default_rng(20240)
    cases = [T.make_tracking_case(orc, rng, n_clutter=150, m_pts=PER_FRAME) for _ in range(BATCH)]
    ls = cases[0][3]
    n_points = BATCH * PER_FRAME
    fine = np.concatenate([T.lm_fine(orc, rng, c[4], c[2], ls) for c in cases])
    b = CM.Builder(N_KF)
    for p in range(n_points):
        b.point([(p + k) % N_KF for k in range(OBSERVERS)], CM.PT_BAD if p % 97 == 5 else 0)
    for p in rng.permutation(n_points).tolist():  # a keyframe's features in no particular order, some of them without a point
        for k in range(OBSERVERS):
            b.feature((p + k) % N_KF, p)
            if p % 13 == 0:
                b.feature((p + k) % N_KF, -1)
    b.kf_bad[[7, 21]] = 1
    m = b.tables()
    m.update(pos=fine["pos"].copy(), normal=fine["normal"].copy(), desc=fine["desc"].copy(), ref_depth=fine["reference_depth"].copy(),
             ref_level=fine["reference_scale_level"].copy(), pt_last_seen=np.full(n_points, -1, np.int32))
    frame_id = (500 + np.arange(BATCH)).astype(np.int32)
    # mvpMapPoints of frame f after the coarse stage: a third of its own points, a few of the next frame's, holes between them
    own = []
    for f in range(BATCH):
        ids = f * PER_FRAME + rng.permutation(PER_FRAME)[:PER_FRAME // 3]
        other = ((f + 1) % BATCH) * PER_FRAME + rng.permutation(PER_FRAME)[:6]
        lst = np.concatenate([ids, other, np.full(20, -1)])
        own.append(rng.permutation(lst).astype(np.int32).tolist())
        m["pt_last_seen"][f * PER_FRAME + rng.permutation(PER_FRAME)[:25]] = frame_id[f]  # :339 skips them for this frame
    own[5] = [-1] * 9  # a frame that matched nothing: the vote is UNCHANGED, the local map empty
    set_start, set_point = M.csr(own), np.array([p for x in own for p in x], np.int32)
    conn, res = CM.update(m, np.arange(N_KF, dtype=np.int32), cap=N_KF)  # every keyframe's connections, ascending
    lists = [conn[k][:res[k]["n_conn"]].tolist() for k in range(N_KF)]
    m.update(conn_start=M.csr(lists), conn_list=np.array([e for lst in lists for e in lst], M.CONN).reshape(-1))
    return cases, m, frame_id, set_start, set_point


def test_vote_select_gather_fine_match_on_the_device_equal_the_oracle_on_the_restated_local_map(orc):
    import torch

    from snake_slam_amd.covis import CovisibilityGraph
    from snake_slam_amd.localmap import LocalMapBuilder
    from snake_slam_amd.tracking import SnakeORBMatcher, frames_dev
    from test_localmap_gpu import to_dev
    from test_track_gpu import _pack_frames_dev

    cases, m, frame_id, set_start, set_point = scene(orc)
    cam, ls = cases[0][1], cases[0][3]
    params = dict(kf_cap=KF_CAP, seed=99)
    # ---- expected: the restatements, then the oracle's matcher on the local map they assemble ----
    w_conn, w_vote = CM.vote(m, set_start, set_point, cap=VOTE_CAP)
    w_local, w_sel = M.select(w_conn, w_vote, m["kf_bad"], m["conn_start"], m["conn_list"], frame_id, params)
    w_lm, w_ids, w_n, w_res = M.gather(m, frame_id, w_local, w_sel, set_start, set_point, PTS_CAP)
    assert w_sel["status"].tolist() == [M.OK] * 5 + [M.EMPTY] + [M.OK] * 2 and np.all(w_res["status"] == M.OK)
    assert np.all(w_sel["n_local"][w_sel["status"] == M.OK] > 15) and np.all(w_sel["n_indirect"][w_sel["status"] == M.OK] > 0)
    assert w_n[5] == 0 and np.all(np.delete(w_n, 5) > 600) and np.all(w_res["n_own_new"][:5] > 0) and np.all(w_res["n_searchable"] < w_n + (w_n == 0))

    stream = torch.cuda.Stream()
    dev = torch.device("cuda", 0)
    cap = max(len(c[0]["kps"]) for c in cases) + 7
    D = _pack_frames_dev([c[0] for c in cases], cap)
    poses = torch.from_numpy(np.stack([c[2] for c in cases])).to(dev)
    t = {k: to_dev(m[k]) for k in CM.MAP_KEYS + ("feat_start", "feat_point", "pt_last_seen", "conn_start", "conn_list") + M.POINT_KEYS}
    d_fid, d_ss, d_sp = to_dev(frame_id), to_dev(set_start), to_dev(set_point)
    conn = torch.full((BATCH, VOTE_CAP, 2), -1, dtype=torch.int32, device=dev)
    vote = torch.full((BATCH, 4), -7, dtype=torch.int32, device=dev)
    local = torch.full((BATCH, KF_CAP), -7, dtype=torch.int32, device=dev)
    sel = torch.full((BATCH, 5), -7, dtype=torch.int32, device=dev)
    lm = torch.full((BATCH, PTS_CAP, 96), 0xA5, dtype=torch.uint8, device=dev)
    ids = torch.full((BATCH, PTS_CAP), -7, dtype=torch.int32, device=dev)
    n_pts = torch.full((BATCH,), -7, dtype=torch.int32, device=dev)
    gres = torch.full((BATCH, 4), -7, dtype=torch.int32, device=dev)
    mi = torch.full((BATCH, PTS_CAP), -7, dtype=torch.int32, device=dev)
    vis = torch.full((BATCH, PTS_CAP), 9, dtype=torch.uint8, device=dev)
    n_m = torch.full((BATCH,), -7, dtype=torch.int32, device=dev)
    fd = frames_dev(T.BOUNDS, D["n"], D["kps"], D["desc"], D["right_points"], D["taken"], D["cell_start"])
    torch.cuda.synchronize()
    # ---- the chain: three handles on ONE stream, nothing comes back before the end ----
    g = CovisibilityGraph(CM.TH, CM.TH_DEPTH, VOTE_CAP, stream=stream.cuda_stream)
    b = LocalMapBuilder(params, stream=stream.cuda_stream)
    matcher = SnakeORBMatcher(0, stream.cuda_stream)
    try:
        g.vote_dev(*(t[k] for k in CM.MAP_KEYS), d_ss, d_sp, conn, vote)
        b.select_dev(conn, vote, t["kf_bad"], t["conn_start"], t["conn_list"], d_fid, local, sel)
        b.gather_dev(t["feat_start"], t["feat_point"], t["pt_flags"], t["pt_last_seen"], t, d_fid, local, sel, d_ss, d_sp, PTS_CAP, lm, ids, n_pts, gres)
        matcher.fine_batch_dev(fd, cam, poses, lm, n_pts, 5.0, 0.8, ls, mi, vis, n_m, write_valid=False)
        matcher.sync()
    finally:
        g.close(), b.close(), matcher.close()
    assert local.cpu().numpy().tobytes() == w_local.tobytes() and sel.cpu().numpy().tobytes() == w_sel.tobytes()
    assert n_pts.cpu().numpy().tobytes() == w_n.tobytes() and ids.cpu().numpy().tobytes() == w_ids.tobytes() and gres.cpu().numpy().tobytes() == w_res.tobytes()
    got_lm = lm.cpu().numpy().view(M.LM_FINE).reshape(BATCH, PTS_CAP)
    mi, vis, n_m = mi.cpu().numpy(), vis.cpu().numpy(), n_m.cpu().numpy()
    total = 0
    for f, case in enumerate(cases):
        n = int(w_n[f])
        assert got_lm[f, :n].tobytes() == w_lm[f, :n].tobytes(), f
        wn, widx, wvis, wvalid = orc.match_fine(case[0], cam, case[2], w_lm[f, :n].astype(orc.LM_FINE), 5.0, 0.8, ls)
        assert n_m[f] == wn and np.array_equal(mi[f, :n], widx) and np.all(mi[f, n:] == -1), f
        assert np.array_equal(vis[f, :n], wvis), f
        total += int(wn)
    assert total > 300  # the frames do find their points in the assembled maps
