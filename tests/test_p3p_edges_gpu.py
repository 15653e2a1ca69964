"""GPU: p3p_ransac_kernel past one group of 256 hypotheses and past one carve of LDS, on the 13 cases of p3p_numpy.edge_cases() (their
properties and seeds are checked on the CPU by tests/test_p3p_numpy.py): n = 63 / 64 / 65 noise-free with 513 iterations (every lane of
three groups ties, the third group holds one hypothesis), n = 255 / 256 / 257 with 256 / 257 / 512 iterations, 90 % wrong pairs with
1024 iterations (a winner beyond the first group, one in the last group, the best count reached in two groups), n = 1489 / 1490
(either side of the 64 KB of LDS a launch gets without asking) and n = 3072 (the maximum, 135 KB).

The comparison with the numpy restatement is the one of tests/test_p3p_gpu.py (p3p_numpy.check_device_against_restatement), with its
tolerance p3p_numpy.pose_tolerance().  Further: the plain entry against the debug entry, a batch that mixes the largest and the
smallest problems against each problem solved alone, the device-resident entry at cap = 257 / 1490 / 3072 against the host entry, and
the shapes the host refuses before a launch."""
import numpy as np
import pytest

import p3p_numpy as P
from test_p3p_chain_gpu import CAM, frames_view, host_pairs, make_frames

pytestmark = pytest.mark.gpu

EDGES = P.edge_cases()
BY_NAME = {c["name"]: c for c in EDGES}
N64 = next(c for c in EDGES if len(c["wps"]) == 64)


@pytest.fixture(scope="module")
def solver():
    from snake_slam_amd.tracking import P3PRansac

    s = P3PRansac(250, P.THRESHOLD, 0)
    yield s
    s.close()


def setup(solver, c, iterations=None):
    p = solver.params
    p.iterations, p.residual_threshold, p.seed = (c["iterations"] if iterations is None else iterations), c["threshold"], c["seed"]
    return dict(wps=c["wps"], nips=c["nips"])


def same_bytes(x, y):
    return (x["pose"].tobytes() == y["pose"].tobytes() and x["mask"].tobytes() == y["mask"].tobytes() and x["best"] == y["best"]
            and x["matches"].tobytes() == y["matches"].tobytes() and x["inliers"] == y["inliers"])


@pytest.mark.parametrize("c", EDGES, ids=[c["name"] for c in EDGES])
def test_edge_hypotheses_and_winner_match_the_restatement(solver, c):
    prob = setup(solver, c)
    out = solver.debug_hypotheses(**prob)
    want = P.ransac(c["wps"], c["nips"], c["iterations"], c["threshold"], c["seed"])
    P.check_device_against_restatement(c, want, *out)
    res = out[0]
    print(f"{c['name']}: winner {res['best']} with {res['inliers']} inliers, restatement {want['best']}")
    if c["property"] != "shape":  # ties and late winners: the seeds were chosen so that the decision is exact
        assert P.winner_is_exact(want) and res["best"] == want["best"]
        assert res["best"][0] >= (0 if c["property"] == "all_tie" else P.GROUP)
    # the plain entry runs the same launch without the debug arrays
    assert same_bytes(solver.solve_batch([prob])[0], res)


@pytest.mark.parametrize("iterations", [1, 256])
def test_one_hypothesis_and_one_full_group(solver, iterations):
    c = dict(N64, iterations=iterations)
    out = solver.debug_hypotheses(**setup(solver, c))
    assert len(out[1]) == iterations
    want = P.ransac(c["wps"], c["nips"], iterations, c["threshold"], c["seed"])
    P.check_device_against_restatement(c, want, *out)
    assert P.winner_is_exact(want) and out[0]["best"] == want["best"] and out[0]["best"][0] == 0 and out[0]["inliers"] == 64
    assert same_bytes(solver.solve_batch([dict(wps=c["wps"], nips=c["nips"])])[0], out[0])


def test_mixed_batch_equals_every_problem_solved_alone(solver):
    """[3072, 5, 0, 1490, 64] pairs in one launch (LDS carved for 3072) against each problem in a launch of its own, carved for its own
    size, under its own problem index."""
    big, mid = BY_NAME["n3072_o30_px1.0_it600_shape"], BY_NAME["n1490_o30_px1.0_it257_shape"]
    cases = [(big["wps"], big["nips"]), (big["wps"][:5], big["nips"][:5]), (big["wps"][:0], big["nips"][:0]), (mid["wps"], mid["nips"]),
             (N64["wps"], N64["nips"])]
    probs = [dict(wps=w, nips=q) for w, q in cases]
    seed = 0xABCDEF0123456789
    solver.params.iterations, solver.params.residual_threshold, solver.params.seed = 300, P.THRESHOLD, seed
    a = solver.solve_batch(probs)
    b = solver.solve_batch(probs)
    assert [r["inliers"] > 0 for r in a] == [True, True, False, True, True] and a[2]["best"] == (-1, -1)
    for i, (x, y) in enumerate(zip(a, b)):
        assert same_bytes(x, y), i
        alone = solver.solve_batch([probs[i]], first_problem=i)[0]
        assert same_bytes(x, alone), (i, x["best"], alone["best"])
        if len(cases[i][0]) >= 4:
            w = P.ransac(*cases[i], 300, P.THRESHOLD, seed, problem=i)
            print(f"problem {i}: winner {x['best']} with {x['inliers']} inliers, restatement {w['best']} with {w['inliers']}")
            if P.winner_is_exact(w):  # the winner of problem i comes from the triplets of problem index i
                assert x["best"] == w["best"] and x["inliers"] == w["inliers"] and np.array_equal(x["mask"], w["mask"])


def frames_to_dev(F, torch, pts_cap, stride):
    """The tensors of test_p3p_chain_gpu.to_dev with a point table of pts_cap records of `stride` bytes: the point in the first 24, the
    rest filled with bytes that are no zero."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    B, cap = F["B"], F["cap"]
    pts = np.full((B, pts_cap, stride), 0xA5, np.uint8)
    pts[:, :cap, :24] = F["world"].reshape(B, cap, 3).view(np.uint8).reshape(B, cap, 24)
    z = lambda *s, dt: torch.zeros(s, dtype=dt, device="cuda")  # noqa: E731
    return dict(n=t(F["n_feat"]), kps=t(F["kps"].view(np.uint8).reshape(B, cap, 24)), desc=z(B, cap, 4, dt=torch.int64),
                rp=z(B, cap, dt=torch.float32), taken=z(B, cap, dt=torch.uint8), cell_start=z(B, 38 * 24 + 1, dt=torch.int32),
                pts=t(pts), n_pts=t(F["n_pts"]), frame_pt=t(F["frame_pt"]))


@pytest.mark.parametrize("B,cap,pts_cap", [(3, 1490, 1527), (2, 3072, 3072), (5, 257, 257)])
def test_frame_batch_dev_equals_the_host_entry_at_the_lds_edges(B, cap, pts_cap):
    """The assertions of test_p3p_chain_gpu.test_frame_batch_dev_equals_the_host_entry with 300 iterations, point records of 88 bytes,
    frame 0 with exactly `cap` features and (B >= 3) frame 2 with exactly 256."""
    import torch

    from snake_slam_amd.tracking import P3PRansac

    F = make_frames(B, cap, 4000 + cap)
    if B >= 3:
        F["n_feat"][2] = 256
    assert F["n_feat"][0] == cap
    D = frames_to_dev(F, torch, pts_cap, 88)
    start = np.tile([0.0, 0.0, 0.0, 1.0, 0.5, -0.25, 0.125], (B, 1))
    poses = torch.from_numpy(start.copy()).cuda()
    inl = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    s = P3PRansac(300, P.THRESHOLD, 0x1234567800000000 + cap)
    try:
        torch.cuda.synchronize()  # the tensors above were filled on torch's stream, the handle runs on its own
        s.solve_frame_batch_dev(frames_view(D), CAM, D["pts"], D["frame_pt"], D["n_pts"], poses, inl)
        torch.cuda.synchronize()
        pairs = [host_pairs(F, b) for b in range(B)]
        want = s.solve_batch([dict(wps=w, nips=q, pose=start[b]) for b, (f, w, q) in enumerate(pairs)])
    finally:
        s.close()
    got_pt, got_pose, got_inl = D["frame_pt"].cpu().numpy(), poses.cpu().numpy(), inl.cpu().numpy()
    for b in range(B):
        f, _, _ = pairs[b]
        print(f"frame {b}: {F['n_feat'][b]} features, {len(f)} pairs, {want[b]['inliers']} inliers, winner {want[b]['best']}")
        assert got_inl[b] == want[b]["inliers"], b
        assert got_pose[b].tobytes() == want[b]["pose"].tobytes(), b
        keep = np.zeros(cap, bool)
        keep[f[want[b]["mask"].astype(bool)]] = True
        nf = int(F["n_feat"][b])
        assert np.array_equal(got_pt[b, :nf], np.where(keep, F["frame_pt"][b], -1)[:nf]), b  # -1 exactly at the non-inliers
        assert np.array_equal(got_pt[b, nf:], F["frame_pt"][b, nf:]), b                      # beyond the frame's features: untouched
    assert got_inl[1] == 0 and np.array_equal(got_pose[1], start[1]) and (got_pt[1, :3] == -1).all()
    assert len(pairs[0][0]) > 0.9 * cap and want[0]["inliers"] > 0.3 * cap


def test_oversized_and_invalid_shapes_are_refused_before_a_launch(solver):
    """One pair, one iteration, one feature more than the kernel is built for, a point record shorter than a point and a threshold of
    0: each is refused as an invalid argument (nothing is launched, no output is written) and the handle goes on working."""
    import torch

    from snake_slam_amd._lib import SnakeHipError
    from snake_slam_amd.tracking import P3PRansac

    c = BY_NAME["n3072_o30_px1.0_it600_shape"]
    prob = setup(solver, N64, 300)
    before = solver.solve_batch([prob])[0]
    big = dict(wps=np.concatenate([c["wps"], c["wps"][:1]]), nips=np.concatenate([c["nips"], c["nips"][:1]]))
    assert len(big["wps"]) == P.MAX_PAIRS + 1
    with pytest.raises(SnakeHipError, match="invalid argument.*3072"):
        solver.solve_batch([prob, big])
    with pytest.raises(SnakeHipError, match="invalid argument.*3072"):
        solver.debug_hypotheses(**big)
    solver.params.iterations = P.MAX_ITERATIONS + 1
    with pytest.raises(SnakeHipError, match=r"invalid argument.*2\^20"):
        solver.solve_batch([prob])
    solver.params.iterations = P.MAX_ITERATIONS  # the largest count the ABI admits passes the check: an empty batch launches nothing
    assert solver.solve_batch([]) == []
    solver.params.iterations, solver.params.residual_threshold = 300, 0.0
    with pytest.raises(SnakeHipError, match="invalid argument.*residual_threshold"):
        solver.solve_batch([prob])
    solver.params.residual_threshold = N64["threshold"]
    assert same_bytes(solver.solve_batch([prob])[0], before)
    # the device-resident entry: every buffer has the size the refused call names, so nothing depends on the refusal for its bounds
    s = P3PRansac(300, P.THRESHOLD, 1)
    try:
        for cap, stride, text in ((P.MAX_PAIRS + 1, 24, "3072"), (64, 20, "pts_stride")):
            F = make_frames(2, cap, 9)
            D = frames_to_dev(F, torch, cap, max(stride, 24))
            pts = D["pts"][:, :, :stride].contiguous()
            poses = torch.full((2, 7), 0.5, dtype=torch.float64, device="cuda")
            inl = torch.full((2,), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            with pytest.raises(SnakeHipError, match="invalid argument.*" + text):
                s.solve_frame_batch_dev(frames_view(D), CAM, pts, D["frame_pt"], D["n_pts"], poses, inl)
            s.params.iterations = P.MAX_ITERATIONS + 1
            with pytest.raises(SnakeHipError, match=r"invalid argument.*2\^20"):
                s.solve_frame_batch_dev(frames_view(D), CAM, D["pts"], D["frame_pt"], D["n_pts"], poses, inl)
            s.params.iterations = 300
            torch.cuda.synchronize()
            assert (poses.cpu().numpy() == 0.5).all() and (inl.cpu().numpy() == -7).all()
            assert np.array_equal(D["frame_pt"].cpu().numpy(), F["frame_pt"])
        s.params.seed = N64["seed"]
        assert same_bytes(s.solve_batch([prob])[0], before)
    finally:
        s.close()
