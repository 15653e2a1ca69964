"""GPU: snk_p3p_ransac_frame_batch_dev -- the device-resident P3P-RANSAC between snk_track_bf_matches_batch_dev and
snk_pose_refine_frame_batch_dev (reference Snake/Tracking/TrackingCoarse.cpp:373-452) -- against the host entry on the same pairs
(batches of 1, 64 and 1024 frames), the chain BF matches -> RANSAC -> refinement on scenes with 50 % wrong matches and a start pose
0.5 m / 15 degrees off, and MultiSequenceTracker(ransac=True) on the synthetic sequences."""
import ctypes as C

import numpy as np
import pytest

import p3p_numpy as P

pytestmark = pytest.mark.gpu

CAM = (P.FX, P.FY, P.CX, P.CY, 47.9)
POSE_REFINE_TOL = 1e-9  # the tolerance the pose refinement is specified by (tests/test_sequence_gpu.py, tests/test_pose_gpu.py)


def make_frames(B, cap, seed, wrong_share=0.5, noise_px=0.5):
    """B frames of up to `cap` features looking at `cap` world points each.  Feature f of frame b shows point perm[b][f]; half of the
    matches point at another point whose projection is at least 20 px away (a wrong brute-force match), a few features have no match
    and a few carry an index outside the point table."""
    from snake_slam_amd.matcher import KP64_DTYPE

    rng = np.random.default_rng(seed)
    n_feat = rng.integers(cap - 40, cap + 1, B).astype(np.int32)
    n_pts = rng.integers(cap - 20, cap + 1, B).astype(np.int32)
    n_feat[0], n_pts[0] = cap, cap
    poses = np.stack([P.random_pose(rng) for _ in range(B)])
    px = np.stack([rng.uniform(0, 752, (B, cap)), rng.uniform(0, 480, (B, cap))], -1)
    depth = np.exp(rng.uniform(np.log(0.5), np.log(40.0), (B, cap)))
    pc = np.stack([(px[..., 0] - P.CX) / P.FX * depth, (px[..., 1] - P.CY) / P.FY * depth, depth], -1)
    world = np.stack([(pc[b] - poses[b, 4:]) @ P.quat_to_R(poses[b, :4]) for b in range(B)])  # point table: point i = feature i's point
    kps = np.zeros((B, cap), KP64_DTYPE)
    kps["x"] = px[..., 0] + noise_px * rng.normal(size=(B, cap))
    kps["y"] = px[..., 1] + noise_px * rng.normal(size=(B, cap))
    kps["octave"] = rng.integers(0, 4, (B, cap))
    frame_pt = np.tile(np.arange(cap, dtype=np.int32), (B, 1))
    wrong = rng.random((B, cap)) < wrong_share
    other = rng.integers(0, cap, (B, cap)).astype(np.int32)
    far = np.linalg.norm(np.take_along_axis(px, other[..., None], 1) - px, axis=-1) >= 20.0
    wrong &= far
    frame_pt[wrong] = other[wrong]
    frame_pt[rng.random((B, cap)) < 0.05] = -1
    true_inlier = (frame_pt == np.arange(cap)) & (np.arange(cap) < n_feat[:, None]) & (frame_pt < n_pts[:, None])
    if B > 1:
        n_feat[1], frame_pt[1, 3:] = 3, -1  # a frame with fewer than four pairs
        true_inlier[1] = False
    return dict(B=B, cap=cap, n_feat=n_feat, n_pts=n_pts, poses=poses, kps=kps, world=world, frame_pt=frame_pt, true_inlier=true_inlier)


def to_dev(F, torch):
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    B, cap = F["B"], F["cap"]
    D = dict(n=t(F["n_feat"]), kps=t(F["kps"].view(np.uint8).reshape(B, cap, 24)), desc=torch.zeros((B, cap, 4), dtype=torch.int64, device=dev),
             rp=torch.full((B, cap), -1.0, dtype=torch.float32, device=dev), taken=torch.zeros((B, cap), dtype=torch.uint8, device=dev),
             cell_start=torch.zeros((B, 38 * 24 + 1), dtype=torch.int32, device=dev), depth=torch.full((B, cap), -1.0, dtype=torch.float32, device=dev),
             pts=t(F["world"].reshape(B, cap, 3).view(np.uint8).reshape(B, cap, 24)), n_pts=t(F["n_pts"]), frame_pt=t(F["frame_pt"]))
    return D


def frames_view(D):
    from snake_slam_amd.tracking import frames_dev

    return frames_dev((0.0, 0.0, 752.0, 480.0), D["n"], D["kps"], D["desc"], D["rp"], D["taken"], D["cell_start"])


def host_pairs(F, b):
    nf, npt = int(F["n_feat"][b]), int(F["n_pts"][b])
    fp = F["frame_pt"][b, :nf]
    f = np.nonzero((fp >= 0) & (fp < npt))[0]
    k = F["kps"][b, f]
    return f, F["world"][b, fp[f]], np.stack([(k["x"] - P.CX) / P.FX, (k["y"] - P.CY) / P.FY], 1)


@pytest.mark.parametrize("B", [1, 64, 1024])
def test_frame_batch_dev_equals_the_host_entry(B):
    import torch

    from snake_slam_amd.tracking import P3PRansac

    F = make_frames(B, 320, 100 + B)
    D = to_dev(F, torch)
    start = np.tile([0.0, 0.0, 0.0, 1.0, 0.5, -0.25, 0.125], (B, 1))
    poses = torch.from_numpy(start.copy()).cuda()
    inl = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    s = P3PRansac(250, P.THRESHOLD, 0x1234567800000000 + B)
    try:
        torch.cuda.synchronize()  # the tensors above were filled on torch's stream, the handle runs on its own
        s.solve_frame_batch_dev(frames_view(D), CAM, D["pts"], D["frame_pt"], D["n_pts"], poses, inl)
        torch.cuda.synchronize()
        pairs = [host_pairs(F, b) for b in range(B)]
        want = s.solve_batch([dict(wps=w, nips=q, pose=start[b]) for b, (f, w, q) in enumerate(pairs)])
    finally:
        s.close()
    got_pt, got_pose, got_inl = D["frame_pt"].cpu().numpy(), poses.cpu().numpy(), inl.cpu().numpy()
    cap = F["cap"]
    for b in range(B):
        f, _, _ = pairs[b]
        assert got_inl[b] == want[b]["inliers"], b
        assert got_pose[b].tobytes() == want[b]["pose"].tobytes(), b
        keep = np.zeros(cap, bool)
        keep[f[want[b]["mask"].astype(bool)]] = True
        nf = int(F["n_feat"][b])
        assert np.array_equal(got_pt[b, :nf], np.where(keep, F["frame_pt"][b], -1)[:nf]), b  # -1 exactly at the non-inliers
        assert np.array_equal(got_pt[b, nf:], F["frame_pt"][b, nf:]), b                      # beyond the frame's features: untouched
    if B > 1:
        assert got_inl[1] == 0 and np.array_equal(got_pose[1], start[1]) and (got_pt[1, :3] == -1).all()
    # sanity of the scene itself: the true inliers are found
    found = np.array([(got_pt[b] >= 0)[F["true_inlier"][b]].mean() for b in range(B) if F["true_inlier"][b].sum() >= 4])
    assert found.min() > 0.95


def rot_between(qa, qb):
    Ra, Rb = P.quat_to_R(qa), P.quat_to_R(qb)
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra @ Rb.T) - 1) / 2, -1, 1))))


def test_chain_bf_ransac_refine_survives_half_wrong_matches():
    """BF matches -> RANSAC -> RefinePoseWithMatches on 64 frames with 50 % wrong matches (each at least 20 px from the right place),
    0.5 px keypoint noise and a start pose 0.5 m / 15 degrees off: the final pose is within the pose refinement's own tolerance (1e-9)
    of the refinement over the true inliers alone.  The refinement WITHOUT RANSAC from the same start is measured and printed; the
    test asserts only that RANSAC is not worse."""
    import torch

    from snake_slam_amd import _lib
    from snake_slam_amd.tracking import P3PRansac, PoseRefinement

    B, cap = 64, 320
    F = make_frames(B, cap, 777)
    D = to_dev(F, torch)
    rng = np.random.default_rng(5)
    start = F["poses"].copy()
    for b in range(B):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        dq = np.concatenate([np.sin(np.radians(15) / 2) * ax, [np.cos(np.radians(15) / 2)]])
        Rn = P.quat_to_R(dq) @ P.quat_to_R(start[b, :4])
        sh = rng.normal(size=3)
        start[b] = P.pose7(Rn.reshape(9), start[b, 4:] + 0.5 * sh / np.linalg.norm(sh))
    ls = (np.float32(1.2) ** np.arange(4)).astype(np.float32)
    # the BF step's output: pairs (frame feature, reference feature) -> frame_pt through snk_track_bf_matches_batch_dev
    pairs = np.zeros((B, cap, 2), np.int32)
    n_pairs = np.zeros(B, np.int32)
    for b in range(B):
        f, _, _ = host_pairs(F, b)
        pairs[b, : len(f), 0], pairs[b, : len(f), 1], n_pairs[b] = f, F["frame_pt"][b, f], len(f)
    ref_has = np.zeros((B, cap), np.uint8)
    for b in range(B):
        ref_has[b, : F["n_pts"][b]] = 1
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    pairs_d, n_pairs_d, ref_has_d = t(pairs), t(n_pairs), t(ref_has)
    # one stream for the whole chain, as a tracker runs it: every step is ordered after the one before without a host round trip
    st = torch.cuda.Stream()
    ref, s = PoseRefinement(stream=st.cuda_stream), P3PRansac(250, P.THRESHOLD, 99, stream=st.cuda_stream)
    fd = frames_view(D)
    lib = _lib.load()

    def refine(frame_pt, poses):
        outl, inl = torch.zeros((B, cap), dtype=torch.uint8, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
        ref.refine_frame_batch_dev(fd, D["depth"], CAM, D["pts"], frame_pt, D["n_pts"], ls, poses, outl, inl)
        st.synchronize()
        return poses.cpu().numpy()

    try:
        torch.cuda.synchronize()  # the inputs were uploaded on torch's default stream
        with torch.cuda.stream(st):
            fp = torch.zeros((B, cap), dtype=torch.int32, device="cuda")
            _lib.check(lib.snk_track_bf_matches_batch_dev(ref._h, pairs_d.data_ptr(), n_pairs_d.data_ptr(), ref_has_d.data_ptr(), cap, B,
                                                          fp.data_ptr()), "snk_track_bf_matches_batch_dev")
            fp_plain = fp.clone()
            poses = t(start)
            inl = torch.zeros(B, dtype=torch.int32, device="cuda")
            s.solve_frame_batch_dev(fd, CAM, D["pts"], fp, D["n_pts"], poses, inl)
            with_ransac = refine(fp, poses)
            without = refine(fp_plain, t(start))
            only_true = t(np.where(F["true_inlier"], F["frame_pt"], -1).astype(np.int32))
            want = refine(only_true, t(F["poses"]))
    finally:
        ref.close()
        s.close()
    d_r, d_p = [], []
    for b in range(B):
        if F["true_inlier"][b].sum() < 4:
            continue
        Rw, tw = P.quat_to_R(want[b, :4]), want[b, 4:]
        d_r.append(P.pose_distance(P.quat_to_R(with_ransac[b, :4]), with_ransac[b, 4:], Rw, tw))
        d_p.append(P.pose_distance(P.quat_to_R(without[b, :4]), without[b, 4:], Rw, tw))
    d_r, d_p = np.array(d_r), np.array(d_p)
    print(f"distance to the true-inlier refinement: with RANSAC max {d_r.max():.2e}; without RANSAC median {np.median(d_p):.2e}, "
          f"max {d_p.max():.2e}, frames beyond 1e-9: {(d_p > POSE_REFINE_TOL).sum()} of {len(d_p)}")
    assert d_r.max() <= POSE_REFINE_TOL
    assert (d_r <= np.maximum(d_p, POSE_REFINE_TOL)).all()


def test_lockstep_tracker_with_ransac():
    """MultiSequenceTracker(ransac=True) on the synthetic sequences (the rig moves 0.05 baselines to the right per frame): the
    trajectory is no further from ground truth than with ransac=False; ransac=False is the chain as it was (no RANSAC handle, the
    same bits as the default construction)."""
    from snake_slam_amd import synth
    from snake_slam_amd.sequence import MultiSequenceTracker

    w, h, orb, cam = 640, 400, (800, 1.2, 4, 20, 7), (400.0, 400.0, 320.0, 200.0, 100.0)
    okw = dict(nfeatures=orb[0], scale_factor=orb[1], n_levels=orb[2], ini_th_fast=orb[3], min_th_fast=orb[4])
    S, T = 3, 4
    seqs = [list(synth.sequence_frames(10 + s, T, w, h, n_rects=300)) for s in range(S)]
    out = {}
    for name, kw in (("default", {}), ("off", dict(ransac=False)), ("on", dict(ransac=True))):
        mt = MultiSequenceTracker(cam, S, T, orb=okw, width=w, height=h, **kw)
        try:
            assert (mt.p3p is not None) == (name == "on")
            for t in range(T):
                mt.process([seqs[s][t][0] for s in range(S)], [seqs[s][t][1] for s in range(S)], float(t))
            out[name], _ = mt.results()
        finally:
            mt.close()
    step = 0.05 * cam[4] / cam[0]
    truth = np.stack([np.arange(T) * step, np.zeros(T), np.zeros(T)], 1)
    err = {k: float(np.sqrt(np.mean([((r[:, 1:4] - truth) ** 2).sum(1) for r in v]))) for k, v in out.items()}
    print(f"RMS distance to ground truth: ransac=False {err['off']:.4e} m, ransac=True {err['on']:.4e} m (step {step:.4f} m)")
    for s in range(S):
        assert np.array_equal(out["off"][s], out["default"][s])
    assert err["on"] <= err["off"]
