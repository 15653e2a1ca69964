"""GPU: the per-frame tracking chain composed from the C-ABI pieces the way TrackingCoarse / TrackingFine
compose them in the reference (TrackingCoarse.cpp:234-270, TrackingFine.cpp:149-158): projection matcher
with a perturbed pose prediction -> 2D-3D matches -> robust pose refinement.  The recovered pose must be
close to the pose the features were generated from; indices must be consistent across the components."""
import numpy as np
import pytest

import pose_helpers as PH
import track_helpers as T
from helpers import SEED

pytestmark = pytest.mark.gpu


def _chain(orc, seed, fine):
    from snake_slam_amd.tracking import PoseRefinement, SnakeORBMatcher, pose_observations

    rng = np.random.default_rng(SEED + seed)
    frame, cam, pose_true, ls, world, _ = T.make_tracking_case(orc, rng, n_clutter=400, m_pts=900, taken_frac=0.0)
    frame["taken"][:] = 0
    pose_pred = PH.perturb(rng, pose_true, rot=0.008, trans=0.04)
    m = SnakeORBMatcher()
    ref = PoseRefinement()
    try:
        if fine:
            pts = T.lm_fine(orc, rng, world, pose_pred, ls)
            n, idx, vis, valid = m.SearchByProjection2(frame, cam, pose_pred, pts, 5.0, 0.8, ls)
        else:
            pts = T.lm_coarse(orc, world)
            n, idx = m.SearchByProjectionFrameFrame2(frame, cam, pose_pred, pts, 15.0, 75, 0, ls)
        assert n > 150
        sel = np.nonzero(idx >= 0)[0]
        feat = idx[sel]
        assert len(set(feat.tolist())) == len(feat)
        depth = np.where(frame["right_points"][feat] > 0, cam[4] / np.maximum(frame["kps"]["x"][feat] - frame["right_points"][feat], 1e-3), -1.0)
        obs = pose_observations(frame["kps"][feat], depth, ls)
        pose, outl, inl = ref.refinePose(cam, pose_pred, world["pos"][sel], obs)
        # the same call through the oracle gives the same pose
        wpose, woutl, winl = orc.pose_refine(pose_pred, orc.Camera(*cam), world["pos"][sel], obs)
        assert np.allclose(pose, wpose, rtol=0, atol=1e-9) and inl == winl
        assert inl > 0.25 * len(sel)  # the synthetic features carry 3 px of noise: many matches exceed the 2.1 / 2.3 px gates

        def reproj(p):  # pixel positions of the visible world points under pose p
            R, t = T.quat_R(p[:4]), p[4:]
            pc = world["pos"][sel] @ R.T + t
            return np.stack([cam[0] * pc[:, 0] / pc[:, 2] + cam[2], cam[1] * pc[:, 1] / pc[:, 2] + cam[3]], 1)

        ref_px = reproj(pose_true)
        d0 = np.linalg.norm(reproj(pose_pred) - ref_px, axis=1).mean()
        d1 = np.linalg.norm(reproj(pose) - ref_px, axis=1).mean()
        assert d1 < 0.4 * d0 and d1 < 1.0, (d0, d1)  # rotation / translation trade off; the image-space distance is what counts
        # wrong matches (features up to 3 sigma = 9 px from the projection) are mostly flagged
        true_xy = np.stack([cam[0] * world["pc"][sel, 0] / world["pc"][sel, 2] + cam[2],
                            cam[1] * world["pc"][sel, 1] / world["pc"][sel, 2] + cam[3]], 1)
        err = np.hypot(frame["kps"]["x"][feat] - true_xy[:, 0], frame["kps"]["y"][feat] - true_xy[:, 1])
        far = err > 8.0 * ls[frame["kps"]["octave"][feat]]
        if far.sum() >= 5:
            assert outl[far].mean() > 0.8
    finally:
        m.close()
        ref.close()


@pytest.mark.parametrize("seed", [1, 2])
def test_coarse_match_then_refine(orc, seed):
    _chain(orc, seed, fine=False)


@pytest.mark.parametrize("seed", [3, 4])
def test_fine_match_then_refine(orc, seed):
    _chain(orc, seed, fine=True)


def test_device_resident_chain_coarse_refine_fine(orc):
    """A batch of frames through the device-resident chain -- coarse matcher, RefinePoseWithMatches, mvpMapPoints / outliers,
    fine matcher with the refined poses -- without a host round trip, against the same chain composed from the oracle's
    functions frame by frame (indices bit-exact, poses within 1e-9)."""
    import torch

    from snake_slam_amd.tracking import (LM_COARSE_DTYPE, LM_FINE_DTYPE, KP64_DTYPE, PoseRefinement, SnakeORBMatcher, frames_dev,
                                         pose_observations)

    rng = np.random.default_rng(SEED + 909)
    cases = [T.make_tracking_case(orc, rng, n_clutter=c, m_pts=mp, taken_frac=0.0) for c, mp in ((400, 900), (250, 500), (600, 1200), (50, 2))]
    cam, ls = cases[0][1], cases[0][3]
    B = len(cases)
    preds = [PH.perturb(rng, c[2], rot=0.006, trans=0.03) for c in cases]
    coarse = [T.lm_coarse(orc, c[4]) for c in cases]
    fine = [T.lm_fine(orc, rng, c[4], c[2], ls) for c in cases]
    cap = max(len(c[0]["kps"]) for c in cases) + 5
    mc = max(len(x) for x in coarse) + 3
    mf = max(len(x) for x in fine) + 3
    dev = torch.device("cuda", 0)
    kps = np.zeros((B, cap), KP64_DTYPE)
    desc = np.zeros((B, cap, 4), np.uint64)
    rp = np.full((B, cap), -1.0, np.float32)
    depth = np.full((B, cap), -1.0, np.float32)
    ncell = cases[0][0]["cols"] * cases[0][0]["rows"] + 1
    cs = np.zeros((B, ncell), np.int32)
    nf = np.zeros(B, np.int32)
    pc = np.zeros((B, mc), LM_COARSE_DTYPE)
    pf = np.zeros((B, mf), LM_FINE_DTYPE)
    ncp, nfp = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b, (frame, _, _, _, _, _) in enumerate(cases):
        k = len(frame["kps"])
        nf[b] = k
        kps[b, :k], desc[b, :k], rp[b, :k], cs[b] = frame["kps"], frame["desc"], frame["right_points"], frame["cell_start"]
        depth[b, :k] = np.where(frame["right_points"] > 0, cam[4] / np.maximum(frame["kps"]["x"] - frame["right_points"], 1e-3), -1.0)
        ncp[b], nfp[b] = len(coarse[b]), len(fine[b])
        pc[b, : ncp[b]], pf[b, : nfp[b]] = coarse[b], fine[b]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_kps = t(kps.view(np.uint8).reshape(B, cap, 24))
    d_desc, d_rp, d_depth, d_cs, d_n = t(desc.view(np.int64)), t(rp), t(depth), t(cs), t(nf)
    d_taken = torch.zeros((B, cap), dtype=torch.uint8, device=dev)
    d_pc, d_pf = t(pc.view(np.uint8).reshape(B, mc, 88)), t(pf.view(np.uint8).reshape(B, mf, 96))
    d_ncp, d_nfp = t(ncp), t(nfp)
    d_pose = t(np.stack(preds))
    mi_c = torch.zeros((B, mc), dtype=torch.int32, device=dev)
    mi_f = torch.zeros((B, mf), dtype=torch.int32, device=dev)
    n_c = torch.zeros(B, dtype=torch.int32, device=dev)
    n_f = torch.zeros(B, dtype=torch.int32, device=dev)
    vis = torch.zeros((B, mf), dtype=torch.uint8, device=dev)
    outl = torch.zeros((B, mc), dtype=torch.uint8, device=dev)
    inl = torch.zeros(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    m, ref = SnakeORBMatcher(), PoseRefinement()
    try:
        fd = frames_dev(T.BOUNDS, d_n, d_kps, d_desc, d_rp, d_taken, d_cs)
        m.coarse_batch_dev(fd, cam, d_pose, d_pc, d_ncp, 15.0, 75, 0, ls, mi_c, n_c)
        m.sync()
        # the refinement runs on its own handle / stream: same frames view, matches of the coarse pass
        ref.refine_matches_batch_dev(fd, d_depth, cam, d_pc, mi_c, d_ncp, ls, d_pose, outl, inl)
        ref.sync()
        m.mark_taken_batch_dev(mi_c, d_ncp, d_taken)
        m.fine_batch_dev(fd, cam, d_pose, d_pf, d_nfp, 5.0, 0.8, ls, mi_f, vis, n_f)
        m.sync()
    finally:
        m.close()
        ref.close()
    mi_c, mi_f, outl, inl, poses, n_f = mi_c.cpu().numpy(), mi_f.cpu().numpy(), outl.cpu().numpy(), inl.cpu().numpy(), d_pose.cpu().numpy(), n_f.cpu().numpy()
    for b, (frame, _, pose_true, _, world, _) in enumerate(cases):
        wn, widx = orc.match_coarse(frame, cam, preds[b], coarse[b], 15.0, 75, 0, ls)
        assert np.array_equal(mi_c[b, : ncp[b]], widx), b
        sel = np.nonzero(widx >= 0)[0]
        feat = widx[sel]
        obs = pose_observations(frame["kps"][feat], depth[b][feat], ls)
        if len(sel) >= 3:
            wpose, woutl, winl = orc.pose_refine(preds[b], orc.Camera(*cam), world["pos"][sel], obs)
        else:
            wpose, woutl, winl = preds[b], np.zeros(len(sel), np.uint8), 0
        assert np.allclose(poses[b], wpose, rtol=0, atol=1e-9) and inl[b] == winl, b
        assert np.array_equal(outl[b, sel], woutl) and not outl[b, : ncp[b]][widx < 0].any(), b
        f2 = dict(frame)
        f2["taken"] = frame["taken"].copy()
        f2["taken"][feat] = 1
        wn2, widx2, _, _ = orc.match_fine(f2, cam, wpose if len(sel) >= 3 else preds[b], fine[b], 5.0, 0.8, ls)
        # the fine matcher ran with the GPU's refined pose (equal to the oracle's within 1e-9): identical indices unless a
        # candidate sits within that of a gate, which these seeded cases do not have
        assert n_f[b] == wn2 and np.array_equal(mi_f[b, : nfp[b]], widx2), b
    assert inl[:3].min() > 20 and inl[3] == 0


@pytest.mark.skipif(__import__("os").environ.get("SNK_POSE_NO_RECURSE") == "1", reason="child run")
@pytest.mark.parametrize("switches", [{"SNK_POSE_LDS_MATCHES": "100"}, {"SNK_POSE_WAVES": "2"}, {"SNK_POSE_WAVES": "2", "SNK_POSE_LDS_MATCHES": "100"}],
                         ids=["small_carve", "two_waves", "two_waves_small_carve"])
def test_device_resident_chain_under_the_forms_large_batches_take(switches):
    """The chain's kernels pick their form by the batch: pose_kernel keeps the first `lds_matches` matches of a frame in LDS (sized so that
    several frames share a compute unit), reads the rest from global memory and runs two wavefronts per frame instead of four when there are
    more frames than two per CU.  The device-resident chain runs again in a child process with each of these forced on the small test batch
    (a carve of 100 matches, so that most matches of every frame take the global-memory tail; SNK_POSE_WAVES=2) -- same poses.  (The forms
    of the frame-resident matchers: test_zx_frontend_variants_gpu.py.)"""
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    r = subprocess.run([sys.executable, "-m", "pytest", str(Path(__file__).resolve()), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider",
                        "-k", "device_resident_chain_coarse_refine_fine"],
                       env=dict(os.environ, SNK_POSE_NO_RECURSE="1", **switches), capture_output=True, text=True,
                       cwd=str(root), timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-1000:])
    assert "1 passed" in r.stdout


def test_lockstep_glue_kernels_against_numpy():
    """snk_track_bf_matches_batch_dev / snk_track_backproject_batch_dev (the two glue steps of MultiSequenceTracker) on a ragged
    batch -- an empty frame, a frame without pairs, pairs whose reference feature has no point, out-of-range indices -- against
    plain numpy.  Integer work exact; the world points exact too (the kernel is compiled without floating-point contraction)."""
    import ctypes as C

    import torch

    from snake_slam_amd import _lib, synth
    from snake_slam_amd.matcher import KP64_DTYPE
    from snake_slam_amd.tracking import Camera, PoseRefinement, frames_dev

    rng = np.random.default_rng(SEED + 321)
    B, cap = 5, 300
    dev = torch.device("cuda:0")
    n = np.array([250, 0, 300, 17, 120], np.int32)
    n_pairs = np.array([100, 0, 0, 17, 300], np.int32)
    pairs = rng.integers(0, cap, (B, cap, 2)).astype(np.int32)
    for b in range(B):  # distinct queries per frame (one pair per query at most, as filterMatches produces them)
        pairs[b, :, 0] = rng.permutation(cap)
    pairs[0, 3] = (-1, 5)
    pairs[0, 4] = (7, cap + 3)
    has = (rng.random((B, cap)) < 0.6).astype(np.uint8)
    ref = PoseRefinement(device=0)
    lib = _lib.load()
    d_pairs, d_np, d_has = torch.from_numpy(pairs).to(dev), torch.from_numpy(n_pairs).to(dev), torch.from_numpy(has).to(dev)
    d_mi = torch.full((B, cap), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    _lib.check(lib.snk_track_bf_matches_batch_dev(ref._h, d_pairs.data_ptr(), d_np.data_ptr(), d_has.data_ptr(), cap, B, d_mi.data_ptr()), "bf_matches")
    ref.sync()
    want = np.full((B, cap), -1, np.int32)
    for b in range(B):
        for f, r in pairs[b, : n_pairs[b]]:  # (current feature, reference feature): frame.mvpMapPoints[f] = point of r
            if 0 <= f < cap and 0 <= r < cap and has[b, r]:
                want[b, f] = r
    assert np.array_equal(d_mi.cpu().numpy(), want) and (want >= 0).sum() > 100

    kps = np.zeros((B, cap), KP64_DTYPE)
    kps["x"], kps["y"] = rng.uniform(0, 752, (B, cap)), rng.uniform(0, 480, (B, cap))
    depth = np.where(rng.random((B, cap)) < 0.5, rng.uniform(0.5, 30.0, (B, cap)), -1000.0).astype(np.float32)
    poses = np.zeros((B, 7))
    for b in range(B):
        q = rng.normal(size=4)
        poses[b, :4] = q / np.linalg.norm(q)
        poses[b, 4:] = rng.normal(size=3)
    cam = (458.654, 457.296, 367.215, 248.375, 119.75)
    d_kps = torch.from_numpy(kps.view(np.uint8).reshape(B, cap, 24)).to(dev)
    d_n, d_depth, d_poses = torch.from_numpy(n).to(dev), torch.from_numpy(depth).to(dev), torch.from_numpy(poses).to(dev)
    d_desc = torch.zeros((B, cap, 4), dtype=torch.int64, device=dev)
    d_rp, d_tk = torch.zeros((B, cap), dtype=torch.float32, device=dev), torch.zeros((B, cap), dtype=torch.uint8, device=dev)
    d_cs = torch.zeros((B, 38 * 24 + 1), dtype=torch.int32, device=dev)
    fd = frames_dev((0.0, 0.0, 752.0, 480.0), d_n, d_kps, d_desc, d_rp, d_tk, d_cs)
    d_world = torch.full((B, cap, 3), 9.0, dtype=torch.float64, device=dev)
    d_h = torch.full((B, cap), 9, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    c = Camera(*cam)
    _lib.check(lib.snk_track_backproject_batch_dev(ref._h, C.byref(fd), d_depth.data_ptr(), C.byref(c), d_poses.data_ptr(), d_world.data_ptr(),
                                                   d_h.data_ptr()), "backproject")
    ref.sync()
    got_w, got_h = d_world.cpu().numpy(), d_h.cpu().numpy()
    for b in range(B):
        m = int(n[b])
        hb = depth[b, :m] > 0
        z = np.where(hb, depth[b, :m], 1.0).astype(np.float64)
        pc = np.stack([(kps["x"][b, :m] - cam[2]) / cam[0] * z, (kps["y"][b, :m] - cam[3]) / cam[1] * z, z], 1)
        R = synth.quat_to_R(poses[b, :4])
        p = pc - poses[b, 4:]
        # the kernel's expressions operation by operation (round 6: backproject_kernel is compiled without contraction, so the world
        # points -- the next frame's local map -- are exactly these doubles; a BLAS product would fuse multiply-adds)
        w = np.stack([(p[:, 0] * R[0, k] + p[:, 1] * R[1, k]) + p[:, 2] * R[2, k] for k in range(3)], 1)
        assert np.array_equal(got_h[b, :m], hb.astype(np.uint8)) and np.array_equal(got_w[b, :m], w)
        assert not got_h[b, m:].any() and not got_w[b, m:].any()   # beyond the frame's features: no point
    ref.close()


def frame_batch_case(cap, mcap, nf, npts):
    """Inputs of snk_pose_refine_frame_batch_dev for five frames of capacity cap with nf features and npts of mcap points each: an
    ordinary frame, one whose features share few points, an empty frame (nf[2] = 0), a frame with two pairs (features 5 and 200 of
    frame 3), and in frame 4 indices beyond the frame's point count and beyond the table."""
    from snake_slam_amd.tracking import KP64_DTYPE

    rng = np.random.default_rng(SEED + 4242)
    B = 5
    nf, npts = np.array(nf, np.int32), np.array(npts, np.int32)
    assert len(nf) == len(npts) == B and nf.max() <= cap and npts.max() <= mcap and nf[2] == 0 and nf[3] > 200 and nf[4] > 7
    kps = np.zeros((B, cap), KP64_DTYPE)
    depth = np.full((B, cap), -1.0, np.float32)
    pts = np.zeros((B, mcap, 3))
    frame_pt = np.full((B, cap), -1, np.int32)
    poses0 = np.zeros((B, 7))
    for b in range(B):
        pr = PH.make_problem(int(rng.integers(0, 1 << 30)), int(npts[b]), outlier_frac=0.2)
        poses0[b] = pr["pose0"]
        pts[b, : npts[b]] = pr["wps"]
        n = int(nf[b])
        if n == 0:
            continue
        # feature f observes point frame_pt[f]: a random subset of features, points drawn WITH replacement
        obs_of = pr["obs"]
        sel = rng.random(n) < (0.7 if b != 3 else 0.0)
        if b == 3:
            sel[[5, 200]] = True   # two pairs only: nothing to refine
        which = rng.integers(0, npts[b], n)
        frame_pt[b, :n] = np.where(sel, which, -1)
        kps["x"][b, :n], kps["y"][b, :n] = obs_of["x"][which], obs_of["y"][which]
        kps["octave"][b, :n] = rng.integers(0, 4, n)
        depth[b, :n] = np.where(obs_of["depth"][which] > 0, obs_of["depth"][which], -1.0)
        if b == 4:
            frame_pt[b, 7] = npts[b] + 3    # beyond the frame's points: ignored
            frame_pt[b, n - 1] = mcap + 50  # beyond the table: ignored
    ls = (np.float32(1.2) ** np.arange(4)).astype(np.float32)
    return dict(B=B, cap=cap, mcap=mcap, nf=nf, npts=npts, kps=kps, depth=depth, pts=pts, frame_pt=frame_pt, poses0=poses0, ls=ls)


def run_frame_batch(case):
    """The call on the device; returns (poses [B, 7], mvbOutlier [B, cap], inliers [B])."""
    import torch

    from snake_slam_amd.tracking import PoseRefinement, frames_dev

    B, cap, mcap = case["B"], case["cap"], case["mcap"]
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_kps, d_depth, d_n = t(case["kps"].view(np.uint8).reshape(B, cap, 24)), t(case["depth"]), t(case["nf"])
    d_desc = torch.zeros((B, cap, 4), dtype=torch.int64, device=dev)
    d_rp, d_tk = torch.zeros((B, cap), dtype=torch.float32, device=dev), torch.zeros((B, cap), dtype=torch.uint8, device=dev)
    d_cs = torch.zeros((B, 38 * 24 + 1), dtype=torch.int32, device=dev)
    d_pts, d_fp, d_np, d_pose = t(case["pts"].view(np.uint8).reshape(B, mcap, 24)), t(case["frame_pt"]), t(case["npts"]), t(case["poses0"])
    outl = torch.full((B, cap), 9, dtype=torch.uint8, device=dev)
    inl = torch.full((B,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ref = PoseRefinement()
    try:
        fd = frames_dev((0.0, 0.0, 752.0, 480.0), d_n, d_kps, d_desc, d_rp, d_tk, d_cs)
        ref.refine_frame_batch_dev(fd, d_depth, PH.CAM, d_pts, d_fp, d_np, case["ls"], d_pose, outl, inl)
        ref.sync()
    finally:
        ref.close()
    return d_pose.cpu().numpy(), outl.cpu().numpy(), inl.cpu().numpy()


def check_frame_batch(orc, case, got):
    """Against orc.pose_refine on the pairs gathered in feature order: mvbOutlier per feature identical, pose within 1e-9."""
    from snake_slam_amd.tracking import pose_observations

    cap, nf, npts, kps, depth, pts, frame_pt, poses0, ls = (case[k] for k in ("cap", "nf", "npts", "kps", "depth", "pts", "frame_pt", "poses0", "ls"))
    got_pose, got_outl, got_inl = got
    for b in range(case["B"]):
        n = int(nf[b])
        f = np.nonzero((frame_pt[b, :n] >= 0) & (frame_pt[b, :n] < npts[b]))[0]
        want_outl = np.zeros(cap, np.uint8)
        if len(f) < 3:
            assert np.array_equal(got_pose[b], poses0[b]) and got_inl[b] == 0 and not got_outl[b].any(), b
            continue
        obs = pose_observations(kps[b, f], depth[b, f], ls)
        wpose, woutl, winl = orc.pose_refine(poses0[b], orc.Camera(*PH.CAM), pts[b, frame_pt[b, f]], obs)
        want_outl[f] = woutl
        assert np.allclose(got_pose[b], wpose, rtol=0, atol=1e-9), b
        assert got_inl[b] == winl and np.array_equal(got_outl[b], want_outl), b
    assert len(set(frame_pt[0][frame_pt[0] >= 0].tolist())) < (frame_pt[0] >= 0).sum()  # the case did contain shared points


def test_refine_frame_batch_dev_walks_features_like_the_reference(orc):
    """snk_pose_refine_frame_batch_dev: `frame.mvpMapPoints` as indices, pairs in FEATURE order (PoseRefinement.cpp:37-57) -- what
    TrackBruteForce leaves behind (TrackingCoarse.cpp:373-377: several frame features may carry the point of one reference feature).
    A ragged batch: an ordinary frame, one whose features share few points, an empty frame, a frame with two pairs (pose untouched),
    indices beyond the frame's point count (ignored) -- against orc.pose_refine on the pairs gathered in feature order; mvbOutlier
    per feature identical, pose within 1e-9.  (The same at the capacities where the kernel form changes: test_pose_forms_gpu.py.)"""
    case = frame_batch_case(700, 500, [650, 400, 0, 300, 700], [500, 40, 10, 500, 480])
    check_frame_batch(orc, case, run_frame_batch(case))
