"""GPU: the batched tracking chain (snk_feature_grid_batch_dev -> snk_match_project_coarse_batch_dev -> snk_match_mark_taken_batch_dev ->
snk_match_project_fine_batch_ro_dev / _dev) at the edges of its launch plan, bit for bit against the oracle, frame by frame: the edge of
64 points per wavefront by the size of the call alone, the last and first capacity of each LDS carve, every edge of the 1024-point chunk
walk, both forms of the separate resolution, device-side counts out of range, and the feature grid where its counting form ends.

Every launch shape is a row of tests/forms.py (forms.shape), and every launch names its plan on stderr under SNK_DEBUG: the line must
equal the row, so a test cannot pass on another kernel form than the one it was written for.  The plans that need a switch (read once per
process) run in two children (tests/form_children.py, kinds track_lds and track_wgs2); the parent builds the same seeded inputs."""
import os

import numpy as np
import pytest

import form_children as FC
import forms
import track_helpers as T
from helpers import SEED

pytestmark = pytest.mark.gpu
children = pytest.mark.skipif(os.environ.get("SNK_TRACK_NO_RECURSE") == "1", reason="child run")

N1 = forms.NCELL1
KEEP = ("mi_c", "mi_f", "vis", "n_c", "n_f", "taken")


@pytest.fixture(scope="module")
def matcher():
    from snake_slam_amd.tracking import SnakeORBMatcher

    m = SnakeORBMatcher(0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return forms.build_driver(tmp_path_factory.mktemp("dispatch"))


def plan_of(shape):
    return tuple(shape[:4])


def assert_chain_plans(stderr, launches):
    """One chain = three plan lines (coarse, fine_ro, fine); each names the shape and the form of its row of the table."""
    lines = forms.track_plan_lines(stderr)
    want = [(e, plan_of(s), f) for s, f in launches for e in ("coarse", "fine_ro", "fine")]
    assert [(e, s, f) for e, s, _, f in lines] == want, stderr[-2000:]
    return lines


def cross_chunk(lost):
    return [p for p in lost if p[2] >= 1024]


# ---- (a) the default dispatch at 64 points per wavefront: 512 frames, no switch ----
A_CAP = 333
A_FEATURES = [0, 1, 150, 300, A_CAP, 151, 299, A_CAP]


@pytest.fixture(scope="module")
def a_base(orc):
    """Two scenes of 2048 points; the eight small frames are thinned from them."""
    out = []
    for k in range(2):
        rng = np.random.default_rng(SEED + 910 + k)
        frame, cam, pose, ls, world, _ = T.make_tracking_case(orc, rng, n_clutter=0, m_pts=2048)
        # (rolled: the points behind the camera are the first of a scene, and the frames of 1, 63, 64 and 65 points take the first ones)
        out.append((frame, cam, pose, ls, np.roll(T.lm_coarse(orc, world), -128), np.roll(T.lm_fine(orc, rng, world, pose, ls), -128)))
    return out


def a_case(orc, a_base, points):
    rng = np.random.default_rng(SEED + 920)
    frames, poses, coarse, fine, copies = [], [], [], [], []
    for b, (n, m) in enumerate(zip(A_FEATURES, points)):
        frame, cam, pose, ls, pc, pf = a_base[b % 2]
        if 0 < m <= 65:   # few points: the features they want come first, so that the frames of 1, 63, 64 and 65 points have matches
            _, widx = orc.match_coarse(frame, cam, pose, pc[:max(m, 8)], 15.0, 75, 0, ls)
            wanted = np.unique(widx[widx >= 0])
            others = rng.permutation(np.setdiff1d(np.arange(len(frame["kps"])), wanted))
            frame = T.keep_features(orc, frame, np.concatenate([wanted, others])[:n])
        else:
            frame = T.thin_to(orc, rng, frame, n)
        pc, pf = pc[:m].copy(), pf[:m].copy()
        copies.append(T.add_conflicts(orc, frame, cam, pose, ls, pc, pf))
        frames.append(frame), poses.append(pose), coarse.append(pc), fine.append(pf)
    return frames, cam, poses, ls, coarse, fine, copies


@pytest.mark.parametrize("pts_cap,form,ppw,points", [
    (1024, "frame/1/fused", 64, [1024, 65, 64, 63, 1024, 1, 0, 1023]),
    (1023, "batch/0/lds", 63, [1023, 65, 64, 63, 1023, 1, 0, 1022]),
    (2048, "frame/2/lds", 64, [2048, 65, 64, 63, 2048, 1, 0, 1025])])   # <= 1024 points: the second workgroup of the frame returns at once
def test_default_dispatch_at_64_points_per_wavefront(orc, matcher, a_base, monkeypatch, capfd, pts_cap, form, ppw, points):
    """512 frames (eight distinct ones, tiled 64 times) x pts_cap points: 524 288 points select the frame kernels by size, 523 776 the
    batch kernels with 63 points per wavefront, 2048 points per frame two workgroups per frame and the separate resolution -- there
    the copies in the second chunk lose against originals that another workgroup matched."""
    shape = forms.shape("track_launch", (pts_cap, 512, A_CAP, N1, 0, 0, 0, 0), form)
    assert {0, 1, 63, 64, 65, pts_cap} <= set(points)
    frames, cam, poses, ls, coarse, fine, copies = a_case(orc, a_base, points)
    assert [len(f["kps"]) for f in frames] == A_FEATURES
    monkeypatch.setenv("SNK_DEBUG", "1")
    capfd.readouterr()
    res = T.run_chain_dev(matcher, frames, cam, poses, ls, coarse, fine, A_CAP, pts_cap, pts_cap, tile=64)
    lines = assert_chain_plans(capfd.readouterr().err, [(shape, form)])
    assert all(p == ppw for _, _, p, _ in lines)
    total, want = T.check_chain(orc, res, frames, cam, poses, ls, coarse, fine, tile=64)
    assert total > 150 and all((want[b][0] >= 0).sum() >= min(A_FEATURES[b], len(coarse[b]), 8) for b in range(8))
    for b, (cidx, fidx) in enumerate(want):
        lost = T.lost_copies(copies[b], cidx, fidx)
        if len(coarse[b]) >= 1000 and len(frames[b]["kps"]) >= 300:
            assert len(lost) >= 8, b                      # within a wavefront / across the wavefronts of a chunk
        if len(coarse[b]) >= 2048 and len(frames[b]["kps"]) >= 300:   # (frame 0 has the points and no feature to quarrel about)
            assert len(cross_chunk(lost)) >= 8, b         # across chunks, here also across workgroups


# ---- (b) the LDS limits, under SNK_TRACK_PPW=64 and one workgroup per frame; three chunks on two workgroups ----
def check_child_chain(orc, got, cap, stderr_lines=None):
    frames, cam, poses, ls, coarse, fine, copies = FC.track_lds_case(orc, cap)
    assert [len(c) for c in coarse] == FC.TRACK_LDS_POINTS and [len(f["kps"]) for f in frames].count(cap) == 3
    res = {k: got[f"{k}_{cap}"] for k in KEEP}
    pf = np.zeros(res["mi_f"].shape, [("valid", "u1")])
    pf["valid"] = got[f"valid_{cap}"]
    res["pf"] = pf
    total, want = T.check_chain(orc, res, frames, cam, poses, ls, coarse, fine)
    assert total > 1000
    for b, (cidx, fidx) in enumerate(want):
        if len(coarse[b]) > 1025:   # (1025 points: the one point of the second chunk could only copy point 0, which lies behind the camera)
            assert len(cross_chunk(T.lost_copies(copies[b], cidx, fidx))) >= 8, b
    full = [b for b, f in enumerate(frames) if len(f["kps"]) == cap]
    assert any((want[b][0] >= cap - 64).any() or (want[b][1] >= cap - 64).any() for b in full)   # matches among the last features of a full carve


@children
def test_lds_limits_of_the_frame_kernels_and_counts_out_of_range(orc, driver, tmp_path):
    """The last capacity at which the claims fit behind the frame (fused resolution), the first at which they do not, the last at which
    the frame fits and the first at which it does not: on the 40 x 26 grid 2203 / 2204 and 2347 / 2348.  The capacities are the
    driver's; the table's rows must be exactly those.  Frames with n == cap use the last bytes of each carve.  The same child then
    runs the chain at the first capacity with counts out of range: the results of the clamped counts, guard rows untouched."""
    rows = FC.track_lds_rows(1)
    fused_end, frame_end = forms.track_plan_edges(driver, 2049, 7, N1, 1, 64)
    caps = [fused_end, fused_end + 1, frame_end, frame_end + 1]
    assert [s[2] for s, _ in rows] == caps and caps[1] - caps[0] == 1 and caps[3] - caps[2] == 1
    plans = ["frame/1/fused", "frame/1/lds", "frame/1/lds", "batch/0/lds"]
    launches = [(forms.shape("track_launch", (2049, 7, c, N1, 0, 1, 0, 64), f), f) for c, f in zip(caps, plans)]
    assert launches == rows
    out = tmp_path / "track_lds.npz"
    r = FC.run_child("track_lds", out, SNK_TRACK_PPW="64", SNK_TRACK_FRAME_WGS="1", SNK_DEBUG="1")
    assert_chain_plans(r.stderr, launches + launches[:1])
    got = np.load(out)
    for cap in caps:
        check_child_chain(orc, got, cap)
    # counts out of range: frame 0 is full and reads n = cap + 9 and -5 points, frame 1 is empty and reads n = -3 and pts_cap + 7 points
    cap = caps[0]
    frames, cam, poses, ls, coarse, fine, _ = FC.track_lds_case(orc, cap)
    _, _, eff_c, eff_f = FC.track_bad_counts(frames, coarse, fine, cap, 2049)
    assert bool(got["guards_intact"])
    res = {k: got[f"{k}_bad"] for k in KEEP}
    pf = np.zeros(res["mi_f"].shape, [("valid", "u1")])
    pf["valid"] = got["valid_bad"]
    res["pf"] = pf
    T.check_chain(orc, res, frames, cam, poses, ls, eff_c, eff_f)


@children
def test_three_chunks_on_two_workgroups(orc, tmp_path):
    """SNK_TRACK_FRAME_WGS=2 at the fused form's last capacity: 2049 points are three chunks, workgroup 0 takes chunks 0 and 2, the
    resolution is the separate one."""
    (shape, form), = FC.track_lds_rows(2)
    forms.shape("track_launch", shape, "frame/2/lds")
    out = tmp_path / "track_wgs2.npz"
    r = FC.run_child("track_wgs2", out, SNK_TRACK_PPW="64", SNK_TRACK_FRAME_WGS="2", SNK_DEBUG="1")
    assert_chain_plans(r.stderr, [(shape, form)])
    check_child_chain(orc, np.load(out), shape[2])


# ---- (c) the two forms of the separate resolution ----
@pytest.fixture(scope="module")
def c_base(orc):
    """A frame of 32 769 features with 1200 points, and a scene for the two small frames."""
    full = T.make_tracking_case_exact(orc, SEED + 950, 32769, 1200)
    rng = np.random.default_rng(SEED + 951)
    small = T.make_tracking_case(orc, rng, n_clutter=300, m_pts=1200)
    return full, small, T.lm_fine(orc, np.random.default_rng(SEED + 952), full[4], full[2], full[3]), T.lm_fine(orc, rng, small[4], small[2], small[3])


@pytest.mark.parametrize("cap,form", [(32768, "batch/0/lds"), (32769, "batch/0/global")])
def test_resolution_with_claims_in_lds_and_in_global_memory(orc, matcher, c_base, monkeypatch, capfd, cap, form):
    """resolve_batch_kernel<true> at its largest capacity and resolve_batch_kernel<false> at its smallest: a full frame, one of 900
    features and an empty one, 1200 points each with copies."""
    shape = forms.shape("track_launch", (1200, 3, cap, N1, 0, 0, 0, 0), form)
    full, small, full_fine, small_fine = c_base
    rng = np.random.default_rng(SEED + 953)
    frames = [T.thin_to(orc, rng, full[0], cap), T.thin_to(orc, rng, small[0], 900), T.thin_to(orc, rng, small[0], 0)]
    assert [len(f["kps"]) for f in frames] == [cap, 900, 0]
    cam, ls = full[1], full[3]
    poses = [full[2], small[2], small[2]]
    coarse = [T.lm_coarse(orc, full[4]), T.lm_coarse(orc, small[4])[:1199], T.lm_coarse(orc, small[4])]
    fine = [full_fine.copy(), small_fine[:1199].copy(), small_fine.copy()]
    copies = [T.add_conflicts(orc, f, cam, p, ls, c, fi) for f, p, c, fi in zip(frames, poses, coarse, fine)]
    monkeypatch.setenv("SNK_DEBUG", "1")
    capfd.readouterr()
    res = T.run_chain_dev(matcher, frames, cam, poses, ls, coarse, fine, cap, 1200, 1200)
    assert_chain_plans(capfd.readouterr().err, [(shape, form)])
    total, want = T.check_chain(orc, res, frames, cam, poses, ls, coarse, fine)
    assert total > 300
    assert (want[0][0] >= cap // 2).sum() >= 10 and (want[0][1] >= cap // 2).sum() >= 10   # claims in the upper half of the full frame
    for b in (0, 1):
        lost = T.lost_copies(copies[b], *want[b])
        assert len(lost) >= 8 and len(cross_chunk(lost)) >= 2, b


# ---- (d) counts out of range in the default batch form of a small call (the frame form: in the first child above) ----
def test_counts_out_of_range_in_the_batch_form(orc, matcher, monkeypatch, capfd):
    """n_pts_dev = [-5, pts_cap + 7, ...], n = [cap + 9, -3, ...]: the results of the counts clamped to [0, cap], and no byte of the
    guard rows before and after match_idx, visible and n_matches changes (before the clamp, the -1 fill past n_pts of frame 0 began
    five entries before the frame's row)."""
    cap, pts_cap = 400, 300
    shape = forms.shape("track_launch", (pts_cap, 4, cap, N1, 0, 0, 0, 0), "batch/0/lds")
    rng = np.random.default_rng(SEED + 960)
    frame, cam, pose, ls, world, _ = T.make_tracking_case(orc, rng, n_clutter=200, m_pts=300)
    pc, pf = T.lm_coarse(orc, world), T.lm_fine(orc, rng, world, pose, ls)
    frames = [T.thin_to(orc, rng, frame, n) for n in (cap, 0, 200, 300)]
    poses = [pose] * 4
    coarse, fine = [pc, pc, pc[:150], pc], [pf, pf, pf[:150], pf]
    n_feat, n_pts, eff_c, eff_f = FC.track_bad_counts(frames, coarse, fine, cap, pts_cap)
    monkeypatch.setenv("SNK_DEBUG", "1")
    capfd.readouterr()
    bad = T.run_chain_dev(matcher, frames, cam, poses, ls, coarse, fine, cap, pts_cap, pts_cap, n_feat=n_feat, n_coarse=n_pts, n_fine=n_pts, guards=True,
                          expect_cleared=False)
    assert_chain_plans(capfd.readouterr().err, [(shape, "batch/0/lds")])
    clamp = lambda v, hi: [min(max(x, 0), hi) for x in v]
    good = T.run_chain_dev(matcher, frames, cam, poses, ls, coarse, fine, cap, pts_cap, pts_cap, n_feat=clamp(n_feat, cap), n_coarse=clamp(n_pts, pts_cap),
                           n_fine=clamp(n_pts, pts_cap), guards=True, expect_cleared=False)
    assert bad["guards_intact"] and good["guards_intact"]
    assert all(np.array_equal(bad[k], good[k]) for k in KEEP) and np.array_equal(bad["pf"], good["pf"])
    total, _ = T.check_chain(orc, bad, frames, cam, poses, ls, eff_c, eff_f)
    assert total > 100


# ---- (e) the feature grid where its counting form ends ----
def grid_inputs(orc, rng, bounds, cap, counts):
    """Keypoints of len(counts) frames: uniform over the bounds and a little beyond, some exactly on cell borders, 300 in one cell."""
    cols, rows = orc.grid_dims(bounds)
    B = len(counts)
    K = np.zeros((B, cap), orc.KP64)
    K["x"] = rng.uniform(bounds[0] - 30, bounds[2] + 30, (B, cap))
    K["y"] = rng.uniform(bounds[1] - 30, bounds[3] + 30, (B, cap))
    K["octave"] = rng.integers(0, 4, (B, cap))
    K["angle"] = rng.uniform(0, 360, (B, cap)).astype(np.float32)
    for b in range(B):
        k = min(cap // 4, 64)
        K["x"][b, :k] = bounds[0] + 20.0 * rng.integers(0, cols + 1, k)          # on a border between two columns, the outer ones included
        K["y"][b, k: 2 * k] = bounds[1] + 20.0 * rng.integers(0, rows + 1, k)
        if cap >= 1200:
            K["x"][b, 500:800] = bounds[0] + 20.0 * (cols // 2) + rng.uniform(0, 20, 300)   # 300 features in one cell
            K["y"][b, 500:800] = bounds[1] + 20.0 * (rows // 2) + rng.uniform(0, 20, 300)
    D = rng.integers(0, 2**64, size=(B, cap, 4), dtype=np.uint64)
    return K, D


def run_grid(orc, bounds, K, D, n_dev, capfd):
    """snk_feature_grid_batch_dev with every output between guard rows, checked against the oracle; returns the plan lines."""
    okh, odh, perm, cs, lines = grid_on_device(orc, bounds, K, D, n_dev, capfd)
    check_grid(orc, bounds, K, D, n_dev, okh, odh, perm, cs)
    return lines


def grid_on_device(orc, bounds, K, D, n_dev, capfd):
    import torch
    from snake_slam_amd.tracking import FeatureGrid

    B, cap = K.shape
    cols, rows = orc.grid_dims(bounds)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(a).to(dev)
    dk, dd, dn = t(K.view(np.uint8).reshape(B, cap, 24)), t(D.view(np.int64)), t(np.asarray(n_dev, np.int32))
    ok_w = torch.full((B + 2, cap, 24), T.GUARD_U8, dtype=torch.uint8, device=dev)
    od_w = torch.full((B + 2, cap, 4), T.GUARD_I32, dtype=torch.int64, device=dev)
    perm_w = torch.full((B + 2, cap), T.GUARD_I32, dtype=torch.int32, device=dev)
    cs_w = torch.full((B + 2, cols * rows + 1), T.GUARD_I32, dtype=torch.int32, device=dev)
    g = FeatureGrid(0)
    try:
        torch.cuda.synchronize()
        capfd.readouterr()
        g.create_batch_dev(bounds, dk, dd, dn, ok_w[1:-1], od_w[1:-1], perm_w[1:-1], cs_w[1:-1])
        g.sync()
    finally:
        g.close()
    lines = forms.grid_plan_lines(capfd.readouterr().err)
    okh = ok_w.cpu().numpy().view(orc.KP64).reshape(B + 2, cap)
    return okh, od_w.cpu().numpy().view(np.uint64), perm_w.cpu().numpy(), cs_w.cpu().numpy(), lines


def check_grid(orc, bounds, K, D, n_dev, okh, odh, perm, cs):
    """perm, cell_start and the reordered keypoints and descriptors of every frame equal the oracle's for the clamped count; nothing is
    written past the count, nor into the guard rows before the first and after the last frame."""
    B, cap = K.shape
    guard_k = np.full(24, T.GUARD_U8, np.uint8).view(orc.KP64)[0]
    for w, pattern in ((okh, guard_k), (odh, np.int64(T.GUARD_I32).astype(np.uint64)), (perm, T.GUARD_I32), (cs, T.GUARD_I32)):
        assert (w[0] == pattern).all() and (w[-1] == pattern).all()
    for b in range(B):
        n = min(max(int(n_dev[b]), 0), cap)
        wperm, wcs, _, _ = orc.feature_grid(K[b, :n], bounds)
        assert np.array_equal(perm[b + 1, :n], wperm) and np.array_equal(cs[b + 1], wcs), b
        wk, wd = np.zeros(n, orc.KP64), np.zeros((n, 4), np.uint64)
        wk[wperm], wd[wperm] = K[b, :n], D[b, :n]
        assert np.array_equal(okh[b + 1, :n], wk) and np.array_equal(odh[b + 1, :n], wd), b
        # past the count nothing is written
        assert (perm[b + 1, n:] == T.GUARD_I32).all() and (okh[b + 1, n:] == guard_k).all()


BIG_GRID = (0.0, 0.0, 2400.0, 2000.0)      # 120 x 100 cells
HUGE_GRID = (0.0, 0.0, 5080.0, 5160.0)     # 254 x 258 = 65 532 cells: the network only


def test_feature_grid_at_the_end_of_the_counting_form(orc, driver, monkeypatch, capfd):
    """grid_count_kernel with its LDS at the limit and grid_kernel right behind it, on the tracking grid and on one of 12 000 cells where
    the edge is at a small capacity; the capacities are the driver's.  Counts: the capacity itself, a negative and an oversized one."""
    monkeypatch.setenv("SNK_DEBUG", "1")
    rng = np.random.default_rng(SEED + 970)
    for bounds, ncell in ((T.BOUNDS, N1 - 1), (BIG_GRID, 12000)):
        assert orc.grid_dims(bounds)[0] * orc.grid_dims(bounds)[1] == ncell
        edge = forms.grid_form_edge(driver, ncell)
        for cap, form in ((edge, "count"), (edge + 1, "network")):
            forms.shape("grid_form", (cap, ncell, 0), form)
            counts = [cap, cap // 2, -4, cap + 11]
            K, D = grid_inputs(orc, rng, bounds, cap, counts)
            assert run_grid(orc, bounds, K, D, counts, capfd) == [((cap, ncell), 4, form)]


def test_feature_grid_network_at_its_largest_capacity_and_grid(orc, monkeypatch, capfd):
    """The bitonic network at the documented 16 384 features (n at and around the half where the sorted length doubles, 1 and 0), and on
    a grid of 65 532 cells with features in the first and in the last cell and a frame whose features all fall in the last cell."""
    monkeypatch.setenv("SNK_DEBUG", "1")
    rng = np.random.default_rng(SEED + 980)
    cap = forms.shape("grid_form", (16384, N1 - 1, 0), "network")[0]
    counts = [16384, 8193, 8192, 1, 0]
    K, D = grid_inputs(orc, rng, T.BOUNDS, cap, counts)
    assert run_grid(orc, T.BOUNDS, K, D, counts, capfd) == [((cap, N1 - 1), 5, "network")]
    cap, ncell, _ = forms.shape("grid_form", (400, 65532, 0), "network")
    cols, rows = orc.grid_dims(HUGE_GRID)
    assert cols * rows == ncell and (cols, rows) == (254, 258)
    counts = [400, 257, 400, -1]
    K, D = grid_inputs(orc, rng, HUGE_GRID, cap, counts)
    K["x"][0, 100:120], K["y"][0, 100:120] = rng.uniform(0, 20, 20), rng.uniform(0, 20, 20)                      # the first cell
    K["x"][0, 120:140], K["y"][0, 120:140] = rng.uniform(5060, 5080, 20), rng.uniform(5140, 5160, 20)            # the last cell
    K["x"][2], K["y"][2] = rng.uniform(5060, 5100, 400), rng.uniform(5140, 5200, 400)                            # every feature in (or clamped into) the last cell
    assert run_grid(orc, HUGE_GRID, K, D, counts, capfd) == [((cap, ncell), 4, "network")]
