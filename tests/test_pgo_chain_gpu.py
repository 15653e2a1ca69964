"""GPU: the loop-correction chain from the geometric check to the corrected map (reference Snake/LoopClosing/LoopDetector.cpp:250-278,
355-372 and LoopClosingPGO.cpp:16-146, 231-260): snk_bf_knn2_batch_dev -> snk_bf_filter_batch_dev -> snk_sim3_ransac_pairs_batch_dev on one
stream (the keyframe pairs of test_sim3_chain_gpu.py), then corrected_pose_dev of the winning pair goes through
loop.corrected_source_sim3 into PoseGraph.set_pose, the graph is solved and the map points are transformed.  The test never computes
the corrected pose itself: what it hands to set_pose are the device's 7 doubles, inverted by the library's helper, with scale 1 in the
se3 form (LoopDetector.cpp:361) and the entry of scale_dev in the sim3 form.

The map around the loop is the test's own: keyframe 0 is the target at the pose the RANSAC was given, keyframe 7 the source, which the
map holds a known drift away from where the loop says it is (the pose of keyframe 1 that make_keyframes draws is a gauge: its world is
unrelated to the target's), the keyframes between them interpolate with 0.01 of noise.  Source and target are constant (the CorrectLoop
shape), edges reach 2 neighbours and are added out of order with one duplicate, so sort_edges has work to do.

Checks: the helper's output times the device's pose is the identity to 1e-14; the optimum is within pose_tolerance() of the
restatement's on the same graph (cost: the relative tolerance of test_pgo_gpu.py); target and source come back bit for bit as handed
in; the moved points equal numpy's to <= 1e-12 and points of constant keyframes or without one stay."""
import numpy as np
import pytest

import pgo_numpy as P
import sim3_numpy as S
from test_sim3_chain_gpu import B, CAP, make_keyframes

pytestmark = pytest.mark.gpu

N, PAIR = 8, 0
DRIFT = np.array([0.12, -0.08, 0.05, 0.02, -0.03, 0.06, 0.08])  # (upsilon, omega, sigma) between the map's source pose and the loop's


def ransac_on_one_stream(K, compute_scale):
    """the three device calls of test_sim3_chain_gpu.py; returns corrected_pose [B, 7], scale [B], inliers [B] as the device left them"""
    import torch

    from snake_slam_amd.loop import RegistrationRansac
    from snake_slam_amd.matcher import BruteForceMatcher
    from snake_slam_amd.tracking import frames_dev

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    kp = lambda a: t(a.view(np.uint8).reshape(B, CAP, 24))  # noqa: E731
    D = {k: t(K[k]) for k in ("n1", "n2", "n_pts1", "n_pts2", "frame_pt1", "frame_pt2", "poses1", "poses2")}
    D["desc1"], D["desc2"] = t(K["desc1"].view(np.int64)), t(K["desc2"].view(np.int64))
    D["pts1"], D["pts2"] = t(K["wp1"].view(np.uint8).reshape(B, CAP, 24)), t(K["wp2"].view(np.uint8).reshape(B, CAP, 24))
    zeros = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt, device="cuda")  # noqa: E731
    aux = dict(rp=zeros(B, CAP, dt=torch.float32), taken=zeros(B, CAP, dt=torch.uint8), cs=zeros(B, 2))
    D["kps1"], D["kps2"] = kp(K["kps1"]), kp(K["kps2"])
    fd = [frames_dev((0.0, 0.0, 752.0, 480.0), D["n" + s], D["kps" + s], D["desc" + s], aux["rp"], aux["taken"], aux["cs"]) for s in "12"]
    knn, pairs, n_pairs = zeros(B, CAP, 4), zeros(B, CAP, 2), zeros(B)
    T, scale, cpose = zeros(B, 7, dt=torch.float64), torch.ones(B, dtype=torch.float64, device="cuda"), zeros(B, 7, dt=torch.float64)
    inl, match12 = zeros(B), zeros(B, CAP)
    st = torch.cuda.Stream()
    bf = BruteForceMatcher(stream=st.cuda_stream)
    rs = RegistrationRansac(S.CAM, S.THRESHOLD, 300, compute_scale, 0x5EED0000ABCD, stream=st.cuda_stream)
    try:
        torch.cuda.synchronize()
        bf.knn2_batch_dev(D["desc1"], D["n1"], D["desc2"], D["n2"], knn)
        bf.filter_batch_dev(knn, D["n1"], 120, 0.9, pairs, n_pairs)
        rs.solve_pairs_batch_dev(fd[0], fd[1], pairs, n_pairs, D["pts1"], D["pts2"], D["frame_pt1"], D["frame_pt2"], D["n_pts1"], D["n_pts2"],
                                 D["poses1"], D["poses2"], T, scale, inl, match12, cpose)
        st.synchronize()
    finally:
        bf.close()
        rs.close()
    return cpose.cpu().numpy(), scale.cpu().numpy(), inl.cpu().numpy()


def map_around_the_loop(target, corrected, fix, seed=11):
    """poses [N, 8] of the map as it is: target first, the source last, DRIFT away from its corrected pose"""
    rng = np.random.default_rng(seed)
    sim3 = not fix
    d = DRIFT.copy()
    if not sim3:
        d[6] = 0.0
    source = P.mul(corrected[None], P.exp(d[None]))[0]
    x = P.log(P.mul(P.inv(target[None]), source[None]))[0]
    poses = P.mul(np.repeat(target[None], N, 0), P.exp(np.arange(N)[:, None] / (N - 1) * x[None]))
    poses[1:-1] = P.mul(poses[1:-1], P.exp(P._noise(rng, N - 2, sim3, 0.01)))
    poses[0], poses[-1] = target, source
    return poses


@pytest.mark.parametrize("fix", [1, 0], ids=["se3", "sim3"])
def test_corrected_pose_of_the_ransac_seeds_the_graph(fix):
    from snake_slam_amd.loop import PoseGraph, PoseGraphOptimizer, corrected_source_sim3

    K = make_keyframes(2026)
    cpose, scale, inliers = ransac_on_one_stream(K, compute_scale=not fix)
    assert inliers[PAIR] > 60, "the geometric check accepts the loop"
    # the hand-over: the device's 7 doubles and its scale, nothing recomputed here
    corrected = corrected_source_sim3(cpose[PAIR], 1.0 if fix else scale[PAIR])
    back = P.mul(np.concatenate([corrected[:7], [1.0]])[None], np.concatenate([cpose[PAIR], [1.0]])[None])
    assert P.pose_distance(back, np.array([[0, 0, 0, 1.0, 0, 0, 0, 1.0]])) <= 1e-14, "the se3 part of T_w_correctSource is tmpPose inverted"
    assert corrected[7] == (1.0 if fix else scale[PAIR]) and corrected[7] > 0
    print(f"pair {PAIR}: {inliers[PAIR]} inliers, scale {scale[PAIR]!r}")

    target = P.inv(np.concatenate([K["poses2"][PAIR], [1.0]])[None])[0]  # T_w_target: the pose the RANSAC was given, inverted
    poses = map_around_the_loop(target, corrected, fix)
    const = np.zeros(N, np.uint8)
    const[[0, N - 1]] = 1
    # ConstructPGO: edges in the order the covisibility lists give them, one pair twice; then sortEdges and SetPose
    pg = PoseGraph(poses, const, fix_scale=bool(fix))
    pairs = [(i, i + d) for d in (2, 1) for i in range(N - d)][::-1] + [(N - 1, 0), (3, 4)]
    for k, (i, j) in enumerate(pairs):
        pg.add_vertex_edge(i, j, 1.0 + 0.1 * (k % 4))
    pg.sort_edges()
    pg.set_pose(N - 1, corrected)
    edges = np.array([e[:2] for e in pg.edges], np.int32)
    assert len(edges) == (N - 1) + (N - 2) + 1 and np.array_equal(edges, np.array(sorted(map(tuple, edges)), np.int32))

    G = P.prepare(dict(name="chain", poses_measure=poses, poses_init=pg.poses, constant=const, edges=edges,
                       weights=np.array([e[2] for e in pg.edges]), measurements=None, fix_scale=int(fix)))
    want, info = P.optimise(G)
    o = PoseGraphOptimizer()
    try:
        o.create(pg)
        res = o.init_and_solve()
        got = o.poses()
        tol = P.pose_tolerance()
        d, dc = P.pose_distance(got, want), abs(res["cost_final"] - info["cost_final"])
        print(f"cost {res['cost_initial']:.6e} -> {res['cost_final']:.6e} (restatement {info['cost_final']:.6e}, difference {dc:.2e}), LM "
              f"{res['lm_iterations']} / {info['lm_iterations']}, pose difference {d:.2e}")
        assert abs(res["cost_initial"] - info["cost_initial"]) <= 1e-10 * info["cost_initial"]
        assert res["accepted_steps"] >= 1 and res["cost_final"] < res["cost_initial"]
        assert d <= tol
        assert dc <= tol * max(info["cost_final"], tol * info["cost_initial"])
        assert got[0].tobytes() == target.tobytes() and got[N - 1].tobytes() == corrected.tobytes(), "target and corrected source stay as handed in"
        assert P.pose_distance(got[1:-1], poses[1:-1]) > 1e-3, "the keyframes between them take up the drift"
        if fix:
            assert np.all(got[:, 7] == 1.0)
        # the map-point pass
        rng = np.random.default_rng(12)
        n = 200
        ref = rng.integers(-1, N, n).astype(np.int32)
        ref[:4] = [-1, 0, N - 1, 3]
        pos, nrm, dep = rng.standard_normal((n, 3)) * 5, rng.standard_normal((n, 3)), 1 + rng.random(n)
        gp, gn, gd = o.transform_points(ref, pos, nrm, dep)
        wp, wn, wd = P.transform_points(poses, got, const, ref, pos, nrm, dep)
        for a, b in ((gp, wp), (gn, wn), (gd, wd)):
            assert float(np.abs(a - b).max() / np.abs(b).max()) <= 1e-12
        still = (ref < 0) | (const[np.maximum(ref, 0)] == 1)
        assert still.sum() > 10 and np.array_equal(gp[still], pos[still]) and np.array_equal(gd[still], dep[still])
        assert np.abs(gp[~still] - pos[~still]).max() > 1e-3
    finally:
        o.close()
