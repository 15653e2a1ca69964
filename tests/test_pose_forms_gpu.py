"""GPU: pose_kernel's forms at the launch shapes where the dispatch changes (snake_slam_amd/csrc/dispatch.hpp) against the oracle,
with test_pose_gpu.py's comparison: poses within 1e-9, outlier flags identical except within 1e-6 of the threshold.  Host entry: one
against four wavefronts at an average of 192 matches, and the two-problems-per-CU LDS carve of calls with more than 256 problems
(the tail of a large problem is read from global memory in every step).  Batched entries: row length 255 against 256.  The shapes come
from tests/forms.py; the form that keeps nothing in LDS runs once in a child process under SNK_POSE_NO_LDS."""
import numpy as np
import pytest

import form_children
import forms
import pose_helpers as PH
from helpers import SEED
from test_pose_gpu import compare
from test_tracking_chain_gpu import check_frame_batch, frame_batch_case, run_frame_batch

pytestmark = pytest.mark.gpu


def refine_all(prs):
    from snake_slam_amd.tracking import PoseRefinement

    ref = PoseRefinement()
    try:
        return ref.refine_batch(PH.CAM, [dict(pose=p["pose0"], wps=p["wps"], obs=p["obs"]) for p in prs])
    finally:
        ref.close()


@pytest.mark.parametrize("sizes,form", [((192, 192), "wave4_lds"), ((192, 191), "wave1")])
def test_host_entry_one_against_four_wavefronts(orc, sizes, form):
    forms.shape("pose_host", (sum(sizes), len(sizes), 0), form)
    prs = [PH.make_problem(50 + i, n, outlier_frac=0.2) for i, n in enumerate(sizes)]
    for got, pr in zip(refine_all(prs), prs):
        compare(orc, got, pr, orc.pose_options())


@pytest.fixture(scope="module")
def many_problems():
    """One problem of 1500 matches and 256 of 200 (eight distinct ones, repeated)."""
    small = [PH.make_problem(60 + i, 200, outlier_frac=0.2) for i in range(8)]
    return [PH.make_problem(59, 1500, outlier_frac=0.2)] + [small[i % 8] for i in range(256)]


@pytest.mark.parametrize("n_problems", [257, 256])
def test_host_entry_two_problems_per_cu_carve(orc, many_problems, tmp_path, n_problems):
    """257 problems: the carve is capped below the 1500 matches of the first problem, whose tail then comes from global memory in every
    step; 256 problems: no cap, the whole problem in LDS.  The carve is dispatch.hpp's, asked of the CPU driver."""
    prs = many_problems[:n_problems]
    forms.shape("pose_host", (sum(len(p["obs"]) for p in prs), n_problems, 0), "wave4_lds")
    carve = int(forms.ask(forms.build_driver(tmp_path), [("pose_host_carve", (1500, n_problems))])[0])
    assert (200 < carve < 1500) if n_problems == 257 else carve == 1500
    res = refine_all(prs)
    assert len(res) == n_problems
    for got, pr in zip(res, prs):
        compare(orc, got, pr, orc.pose_options())


@pytest.mark.parametrize("cap,form", [(255, "wave1"), (256, "wave4_lds")])
def test_frame_batch_at_the_stride_threshold(orc, cap, form):
    """snk_pose_refine_frame_batch_dev (row length = cap): test_tracking_chain_gpu.py's ragged batch scaled to cap 255 / 256."""
    forms.shape("pose_batch", (cap, 5, forms.N_CU, 0, 0), form)
    case = frame_batch_case(cap, 200, [240, 150, 0, 210, cap], [200, 40, 10, 200, 190])
    check_frame_batch(orc, case, run_frame_batch(case))


def matches_batch_case(pts_cap, cap=320):
    """snk_pose_refine_matches_batch_dev: per local-map point the index of its feature or -1, pairs in POINT order.  Five frames: full,
    few matches, no points, two matches (pose untouched), feature indices beyond the frame's capacity (ignored)."""
    from snake_slam_amd.tracking import KP64_DTYPE

    rng = np.random.default_rng(SEED + 255)
    B = 5
    npts = np.array([pts_cap, 120, 0, pts_cap - 1, pts_cap], np.int32)
    kps = np.zeros((B, cap), KP64_DTYPE)
    depth = np.full((B, cap), -1.0, np.float32)
    pts = np.zeros((B, pts_cap, 3))
    match_idx = np.full((B, pts_cap), -1, np.int32)
    poses0 = np.zeros((B, 7))
    for b in range(B):
        n = int(npts[b])
        pr = PH.make_problem(int(rng.integers(0, 1 << 30)), max(n, 3), outlier_frac=0.2)
        poses0[b] = pr["pose0"]
        if n == 0:
            continue
        pts[b, :n] = pr["wps"][:n]
        sel = rng.random(n) < (0.85 if b != 3 else 0.0)
        if b == 3:
            sel[[4, n - 1]] = True
        feat = rng.permutation(cap)[:n]   # a feature of its own for every point
        match_idx[b, :n] = np.where(sel, feat, -1)
        kps["x"][b, feat], kps["y"][b, feat] = pr["obs"]["x"][:n], pr["obs"]["y"][:n]
        kps["octave"][b] = rng.integers(0, 4, cap)
        depth[b, feat] = np.where(pr["obs"]["depth"][:n] > 0, pr["obs"]["depth"][:n], -1.0)
        if b == 4:
            match_idx[b, 3], match_idx[b, n - 1] = cap, cap + 77
    ls = (np.float32(1.2) ** np.arange(4)).astype(np.float32)
    return dict(B=B, cap=cap, pts_cap=pts_cap, npts=npts, kps=kps, depth=depth, pts=pts, match_idx=match_idx, poses0=poses0, ls=ls)


@pytest.mark.parametrize("pts_cap,form", [(255, "wave1"), (256, "wave4_lds")])
def test_matches_batch_at_the_stride_threshold(orc, pts_cap, form):
    import torch

    from snake_slam_amd.tracking import PoseRefinement, frames_dev, pose_observations

    forms.shape("pose_batch", (pts_cap, 5, forms.N_CU, 0, 0), form)
    c = matches_batch_case(pts_cap)
    B, cap = c["B"], c["cap"]
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_kps, d_depth, d_n = t(c["kps"].view(np.uint8).reshape(B, cap, 24)), t(c["depth"]), t(np.full(B, cap, np.int32))
    d_desc = torch.zeros((B, cap, 4), dtype=torch.int64, device=dev)
    d_rp, d_tk = torch.zeros((B, cap), dtype=torch.float32, device=dev), torch.zeros((B, cap), dtype=torch.uint8, device=dev)
    d_cs = torch.zeros((B, 38 * 24 + 1), dtype=torch.int32, device=dev)
    d_pts, d_mi, d_np, d_pose = t(c["pts"].view(np.uint8).reshape(B, pts_cap, 24)), t(c["match_idx"]), t(c["npts"]), t(c["poses0"])
    outl = torch.full((B, pts_cap), 9, dtype=torch.uint8, device=dev)
    inl = torch.full((B,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ref = PoseRefinement()
    try:
        fd = frames_dev((0.0, 0.0, 752.0, 480.0), d_n, d_kps, d_desc, d_rp, d_tk, d_cs)
        ref.refine_matches_batch_dev(fd, d_depth, PH.CAM, d_pts, d_mi, d_np, c["ls"], d_pose, outl, inl)
        ref.sync()
    finally:
        ref.close()
    got_pose, got_outl, got_inl = d_pose.cpu().numpy(), outl.cpu().numpy(), inl.cpu().numpy()
    refined = 0
    for b in range(B):
        n = int(c["npts"][b])
        mi = c["match_idx"][b, :n]
        p = np.nonzero((mi >= 0) & (mi < cap))[0]
        want_outl = np.zeros(pts_cap, np.uint8)
        if len(p) < 3:
            assert np.array_equal(got_pose[b], c["poses0"][b]) and got_inl[b] == 0 and not got_outl[b].any(), b
            continue
        obs = pose_observations(c["kps"][b, mi[p]], c["depth"][b, mi[p]], c["ls"])
        wpose, woutl, winl = orc.pose_refine(c["poses0"][b], orc.Camera(*PH.CAM), c["pts"][b, p], obs)
        want_outl[p] = woutl
        assert np.allclose(got_pose[b], wpose, rtol=0, atol=1e-9), b
        assert got_inl[b] == winl and np.array_equal(got_outl[b], want_outl), b
        refined += 1
    assert refined == 3


def test_global_memory_form_in_a_child_process(orc, tmp_path):
    """pose_kernel<4, false> (SNK_POSE_NO_LDS) is reached by no shape: one child process runs one problem of 300 matches through the
    host entry and one frame batch at cap = 256; compared here with the oracle."""
    forms.shape("pose_host", (300, 1, 1), "wave4_global")
    forms.shape("pose_batch", (256, 5, forms.N_CU, 0, 1), "wave4_global")
    out = tmp_path / "pose.npz"
    form_children.run_child("pose", out, SNK_POSE_NO_LDS="1")
    z = np.load(out)
    compare(orc, (z["pose"], z["outl"], int(z["inl"])), form_children.pose_problem(), orc.pose_options())
    check_frame_batch(orc, form_children.pose_batch_case(), (z["b_pose"], z["b_outl"], z["b_inl"]))
