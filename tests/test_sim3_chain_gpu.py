"""GPU: snk_sim3_ransac_pairs_batch_dev -- the device-resident registration RANSAC behind snk_bf_knn2_batch_dev and
snk_bf_filter_batch_dev (reference Snake/LoopClosing/LoopDetector.cpp:163-198, 222-226, 250-278) -- on a batch of 3 keyframe pairs
with cap = 256: the three calls run on one stream without a host round trip, and T, scale, inliers and match12 equal the host entry
snk_sim3_ransac run on the same pairs gathered on the host; corrected_pose equals the formula of DESIGN.md section 3e in numpy within
transform_tolerance(); entries whose feature lacks a point on either side are skipped; the keyframe pair with fewer than 3 usable
pairs leaves its outputs untouched, with 0 inliers."""
import numpy as np
import pytest

import sim3_numpy as S

pytestmark = pytest.mark.gpu

B, CAP = 3, 256


def make_keyframes(seed):
    """B keyframe pairs that see CAP physical points each.  Keyframe 1's map holds them in its world (wp1), keyframe 2's map in a
    world that has drifted: pose2 * wp2 = s R (pose1 * wp1) + t with a known (R, t, s = 1).  A feature shows one point; its
    descriptor is the point's with a few bits flipped, so the brute-force matcher finds most pairs; some features carry no point,
    some an index outside the point table, and some of keyframe 2's features show another point than their descriptor says."""
    from snake_slam_amd.matcher import KP64_DTYPE

    rng = np.random.default_rng(seed)
    out = dict(truth=[], poses1=np.zeros((B, 7)), poses2=np.zeros((B, 7)), wp1=np.zeros((B, CAP, 3)), wp2=np.zeros((B, CAP, 3)),
               kps1=np.zeros((B, CAP), KP64_DTYPE), kps2=np.zeros((B, CAP), KP64_DTYPE), desc1=np.zeros((B, CAP, 4), np.uint64),
               desc2=np.zeros((B, CAP, 4), np.uint64), frame_pt1=np.zeros((B, CAP), np.int32), frame_pt2=np.zeros((B, CAP), np.int32),
               n1=np.array([CAP, CAP - 9, CAP - 30], np.int32), n2=np.array([CAP - 5, CAP, CAP - 17], np.int32),
               n_pts1=np.array([CAP, CAP - 4, CAP - 8], np.int32), n_pts2=np.array([CAP - 6, CAP, CAP - 3], np.int32))
    for b in range(B):
        R, t, s = S.random_transform(rng, 1.0)
        out["truth"].append((R, t, s))
        for key in ("poses1", "poses2"):
            Rp, tp, _ = S.random_transform(rng, 1.0, angle=1.0, shift=5.0)
            out[key][b] = S.pose7(Rp.reshape(9), tp)
        P1 = S._random_points(rng, CAP)
        P2 = s * P1 @ R.T + t
        for P, pose, wp in ((P1, out["poses1"][b], "wp1"), (P2, out["poses2"][b], "wp2")):
            Rp = S.quat_to_R(pose[:4])
            out[wp][b] = (P - pose[4:]) @ Rp  # R^T (P - t)
        point_desc = rng.integers(0, 2**63, (CAP, 4), dtype=np.int64).astype(np.uint64)
        for side, P in (("1", P1), ("2", P2)):
            perm = rng.permutation(CAP)  # feature f shows point perm[f]
            shown = perm.copy()
            if side == "2":
                swap = rng.random(CAP) < 0.2  # the descriptor of one point at the place of another: a wrong pair for the RANSAC
                shown[swap] = rng.integers(0, CAP, int(swap.sum()))
            px = S.project(P[shown]) + 0.5 * rng.normal(size=(CAP, 2))
            out["kps" + side]["x"][b], out["kps" + side]["y"][b] = px[:, 0], px[:, 1]
            flips = np.zeros((CAP, 4), np.uint64)
            for _ in range(3):  # up to 12 of the 256 bits differ
                flips ^= np.left_shift(np.uint64(1), rng.integers(0, 64, (CAP, 4)).astype(np.uint64))
            out["desc" + side][b] = point_desc[perm] ^ flips
            fp = shown.astype(np.int32)
            fp[rng.random(CAP) < 0.1] = -1          # no map point
            fp[rng.random(CAP) < 0.03] = CAP + 7    # an index outside the point table
            out["frame_pt" + side][b] = fp
    out["frame_pt1"][1, 2:] = -1  # keyframe pair 1: at most two usable pairs
    return out


def gather(K, b, pairs, n_pairs):
    """The usable pairs of keyframe pair b as LoopDetector.cpp:163-198 gathers them, from the filter's output."""
    f1, f2 = pairs[b, : n_pairs[b], 0], pairs[b, : n_pairs[b], 1]
    v1, v2 = K["frame_pt1"][b, f1], K["frame_pt2"][b, f2]
    ok = (v1 >= 0) & (v1 < K["n_pts1"][b]) & (v2 >= 0) & (v2 < K["n_pts2"][b])
    f1, f2, v1, v2 = f1[ok], f2[ok], v1[ok], v2[ok]
    k1, k2 = K["kps1"][b, f1], K["kps2"][b, f2]
    return dict(points1=S.view_points(K["poses1"][b], K["wp1"][b, v1]), points2=S.view_points(K["poses2"][b], K["wp2"][b, v2]),
                ips1=np.stack([k1["x"], k1["y"]], 1), ips2=np.stack([k2["x"], k2["y"]], 1)), f1, v2, int((~ok).sum())


@pytest.mark.parametrize("iterations", [0, 300])
def test_knn2_filter_ransac_on_one_stream_equal_the_host_entry(iterations):
    import torch

    from snake_slam_amd.loop import RegistrationRansac
    from snake_slam_amd.matcher import BruteForceMatcher
    from snake_slam_amd.tracking import frames_dev

    K = make_keyframes(2026)
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
    T0, s0, cp0 = np.tile([0.0, 0.0, 0.0, 1.0, 0.5, -0.25, 0.125], (B, 1)), np.full(B, 0.75), np.tile([0.0, 0.0, 0.0, 1.0, 9.0, 8.0, 7.0], (B, 1))
    T, scale, cpose = t(T0), t(s0), t(cp0)
    inl, match12 = torch.full((B,), -7, dtype=torch.int32, device="cuda"), torch.full((B, CAP), -7, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    bf = BruteForceMatcher(stream=st.cuda_stream)
    rs = RegistrationRansac(S.CAM, S.THRESHOLD, iterations, False, 0x5EED0000ABCD, stream=st.cuda_stream)
    try:
        torch.cuda.synchronize()  # the inputs were uploaded on torch's default stream
        # LoopORBmatcher::MatchBruteforce(source, target, ..., 120, 0.9) and LoopDetector::solve, back to back on one stream
        bf.knn2_batch_dev(D["desc1"], D["n1"], D["desc2"], D["n2"], knn)
        bf.filter_batch_dev(knn, D["n1"], 120, 0.9, pairs, n_pairs)
        rs.solve_pairs_batch_dev(fd[0], fd[1], pairs, n_pairs, D["pts1"], D["pts2"], D["frame_pt1"], D["frame_pt2"], D["n_pts1"], D["n_pts2"],
                                 D["poses1"], D["poses2"], T, scale, inl, match12, cpose)
        st.synchronize()  # the one synchronisation of the chain: nothing above waited for the device or read a result
        pairs_h, n_pairs_h = pairs.cpu().numpy(), n_pairs.cpu().numpy()
        G = [gather(K, b, pairs_h, n_pairs_h) for b in range(B)]
        want = rs.solve_batch([dict(g[0], T=T0[b], scale=s0[b]) for b, g in enumerate(G)])
    finally:
        bf.close()
        rs.close()
    got_T, got_s, got_inl, got_m, got_cp = T.cpu().numpy(), scale.cpu().numpy(), inl.cpu().numpy(), match12.cpu().numpy(), cpose.cpu().numpy()
    assert n_pairs_h[0] > 100 and n_pairs_h[2] > 100
    for b in range(B):
        prob, f1, v2, skipped = G[b]
        w = want[b]
        print(f"pair {b}: {n_pairs_h[b]} filtered matches, {skipped} without a point on one side, {len(f1)} pairs, {w['inliers']} inliers")
        assert got_inl[b] == w["inliers"] and got_T[b].tobytes() == w["T"].tobytes() and got_s[b] == w["scale"], b
        m12 = np.full(CAP, -1, np.int32)
        m12[f1[w["mask"].astype(bool)]] = v2[w["mask"].astype(bool)]
        assert np.array_equal(got_m[b], m12), b
        if w["best"] >= 0:
            cp = S.corrected_pose(w["T"], w["scale"], K["poses2"][b])
            d = S.transform_distance(S.quat_to_R(got_cp[b, :4]), got_cp[b, 4:], 1.0, S.quat_to_R(cp[:4]), cp[4:], 1.0)
            assert d <= S.transform_tolerance(), (b, d)
        else:
            assert np.array_equal(got_cp[b], cp0[b])
    # entries without a point on either side were there to be skipped, and the true relative transform is found
    assert G[0][3] > 0 and G[2][3] > 0
    for b in (0, 2):
        R, tt, s = K["truth"][b]
        assert want[b]["inliers"] > 60
        # the map points are exact and only the keypoints carry noise, so a triplet of true pairs gives the true transform
        assert S.transform_distance(S.quat_to_R(got_T[b, :4]), got_T[b, 4:], got_s[b], R, tt, s) <= S.transform_tolerance()
    # fewer than 3 usable pairs: outputs untouched, 0 inliers, no match
    assert len(G[1][1]) < 3 and got_inl[1] == 0 and np.array_equal(got_T[1], T0[1]) and got_s[1] == s0[1] and np.array_equal(got_cp[1], cp0[1])
    assert (got_m[1] == -1).all()
