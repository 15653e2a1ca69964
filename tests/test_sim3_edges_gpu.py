"""GPU: sim3_ransac_kernel around the 1024 pairs it keeps in LDS and past one group of 256 hypotheses, on the 10 cases of
sim3_numpy.edge_cases() (their properties and seeds are checked on the CPU by tests/test_sim3_numpy.py): n = 1023 / 1024 / 1025 / 1280
with the scale estimated and not (no slab, an empty slab, a slab of one record, a slab of 256), a winner beyond the first group and a
best count reached in two groups of 1024 iterations.

The comparison with the numpy restatement is the one of tests/test_sim3_gpu.py (sim3_numpy.check_device_against_restatement), with
its tolerance sim3_numpy.transform_tolerance().  Further: a batch whose problems 0 and 2 each have a slab, against every problem solved
alone, and the device-resident entry with pairs_cap = 1030 and 2048 (compaction past entry 1024 into the slab, the iteration table
past 1024 pairs, 96 KB of LDS) against the host entry on the pairs gathered on the host."""
import numpy as np
import pytest

import sim3_numpy as S

pytestmark = pytest.mark.gpu

EDGES = S.edge_cases()
BY_N = {(len(c["P1"]), c["compute_scale"]): c for c in EDGES}


@pytest.fixture(scope="module")
def solver():
    from snake_slam_amd.loop import RegistrationRansac

    s = RegistrationRansac(S.CAM, S.THRESHOLD, 100, False, 0)
    yield s
    s.close()


def setup(solver, c, iterations=None):
    p = solver.params
    p.iterations, p.threshold, p.seed = (c["iterations"] if iterations is None else iterations), c["threshold"], c["seed"]
    p.compute_scale = int(c["compute_scale"])
    return dict(points1=c["P1"], points2=c["P2"], ips1=c["ip1"], ips2=c["ip2"])


def same_bytes(x, y):
    return (x["T"].tobytes() == y["T"].tobytes() and x["mask"].tobytes() == y["mask"].tobytes() and x["scale"] == y["scale"]
            and x["best"] == y["best"] and x["inliers"] == y["inliers"])


@pytest.mark.parametrize("c", EDGES, ids=[c["name"] for c in EDGES])
def test_edge_hypotheses_and_winner_match_the_restatement(solver, c):
    prob = setup(solver, c)
    out = solver.debug_hypotheses(**prob)
    want = S.ransac(c["P1"], c["P2"], c["ip1"], c["ip2"], c["iterations"], c["threshold"], c["compute_scale"], c["seed"])
    S.check_device_against_restatement(c, want, *out)
    res = out[0]
    print(f"{c['name']}: winner {res['best']} with {res['inliers']} inliers, restatement {want['best']}, groups at the best count "
          f"{S.groups_at_best(want)}")
    if c["property"] != "shape":  # a late winner, a tie across groups: the seeds were chosen so that the decision is exact
        assert S.winner_is_exact(want) and res["best"] == want["best"] and res["best"] >= S.GROUP
    # the plain entry runs the same launch without the debug arrays
    assert same_bytes(solver.solve_batch([prob])[0], res)


def with_true_pair_at(c, i):
    """The case's arrays with a true pair at index i (swapped with the first true pair, if a wrong one is there)."""
    order = np.arange(len(c["P1"]))
    if c["outlier"][i]:
        j = int(np.nonzero(~c["outlier"])[0][0])
        order[[i, j]] = order[[j, i]]
    return dict(points1=c["P1"][order], points2=c["P2"][order], ips1=c["ip1"][order], ips2=c["ip2"][order])


def batch_equals_alone(solver, probs, seed):
    """One launch of `probs` (300 iterations, the scale estimated) run twice, each problem against a launch of its own under its own
    problem index and -- where the restatement's decision is exact -- against the restatement with that problem index."""
    p = solver.params
    p.iterations, p.threshold, p.seed, p.compute_scale = 300, S.THRESHOLD, seed, 1
    a = solver.solve_batch(probs)
    b = solver.solve_batch(probs)
    for i, (x, y) in enumerate(zip(a, b)):
        assert same_bytes(x, y), i
        alone = solver.solve_batch([probs[i]], first_problem=i)[0]
        assert same_bytes(x, alone), (i, x["best"], alone["best"], x["inliers"], alone["inliers"])
        q = probs[i]
        w = S.ransac(q["points1"], q["points2"], q["ips1"], q["ips2"], 300, S.THRESHOLD, True, seed, problem=i)
        print(f"problem {i}: winner {x['best']} with {x['inliers']} inliers, restatement {w['best']} with {w['inliers']}")
        if S.winner_is_exact(w):  # the winner of problem i comes from the triplets of problem index i
            assert x["best"] == w["best"] and x["inliers"] == w["inliers"] and np.array_equal(x["mask"], w["mask"])
    return a


def problem(c, n=None):
    return {k: v[:n] for k, v in dict(points1=c["P1"], points2=c["P2"], ips1=c["ip1"], ips2=c["ip2"]).items()}


def test_mixed_batch_equals_every_problem_solved_alone(solver):
    """[1025, 200, 2048, 1024, 3] pairs in one launch: problems 0 and 2 have a slab each (of 1024 records a problem, as the largest
    needs), problems 1, 3 and 4 sit in planes carved for 1024 pairs.  Each equals the same problem in a launch of its own, carved for
    its own size, under its own problem index.  Pair 1024 -- the first record of a slab -- is a true pair in problems 0 and 2, so its
    mask bit shows whose record the workgroup read."""
    big = next(c for c in S.gpu_cases() if len(c["P1"]) == S.MAX_PAIRS)
    p1023, p1024 = BY_N[(1023, True)], BY_N[(1024, True)]
    assert big["compute_scale"]
    probs = [with_true_pair_at(BY_N[(1025, True)], 1024), problem(p1023, 200), with_true_pair_at(big, 1024), problem(p1024), problem(p1024, 3)]
    assert [len(q["points1"]) for q in probs] == [1025, 200, 2048, 1024, 3]
    a = batch_equals_alone(solver, probs, 0xABCDEF0123456789)
    assert a[0]["mask"][1024] == 1 and a[2]["mask"][1024] == 1 and a[0]["inliers"] > 600 and a[1]["inliers"] > 100 and a[2]["inliers"] > 1200


def test_slabs_of_workgroups_that_share_an_l2_stay_apart(solver):
    """[2048, 1280, 5, 5, 5, 5, 5, 5, 2048, 2048] pairs of four different scenes in one launch.  The mixed batch above cannot show a
    wrong slab base on this device: its five workgroups are dealt to five of the eight XCDs, whose L2s are not coherent with each other
    within a launch, so each would read back its own records from its own L2 whatever the address.  Workgroups b and b + 8 share an
    XCD; here 0 and 8, and 1 and 9, have slabs (80 KB for 2048 pairs, more than a compute unit's vector cache holds, so the scoring
    loop reads the records from the L2 again and again).  A workgroup that read another problem's records would count that scene's
    pairs under its own transform.  Ten problems instead of the five the other batches keep to: the six small ones cost nothing."""
    scenes = [S.make_case(n, 0.3, 1.0, True, 300, 7000 + i) for i, n in enumerate((2048, 1280, 2048, 2048))]
    order = [0, 1] + [None] * 6 + [2, 3]
    a = batch_equals_alone(solver, [problem(scenes[0], 5) if j is None else problem(scenes[j]) for j in order], 0x0123456789ABCDEF)
    for j, r in zip(order, a):
        if j is not None:
            true_pairs = ~scenes[j]["outlier"]
            assert r["inliers"] > 0.9 * true_pairs.sum() and r["mask"][S.LDS_PAIRS:].sum() > 0.9 * true_pairs[S.LDS_PAIRS:].sum(), j


# ------------------------------------------------------------------ the device-resident entry ------------
B = 3
USABLE = (1028, 700, 2)


def make_keyframes(cap, seed):
    """B keyframe pairs of `cap` features that see `cap` physical points each, as test_sim3_chain_gpu.make_keyframes lays them out
    (pose2 * wp2 = R (pose1 * wp1) + t, a fifth of keyframe 2's features show another point), and the pair list written directly:
    one entry per point in random order, n_pairs = cap for the first keyframe pair.  All but about USABLE[b] entries are made
    unusable in turn by a feature without a point, a point index outside the table, a point index beyond n_pts, or a feature index
    outside the frame."""
    from snake_slam_amd.matcher import KP64_DTYPE

    rng = np.random.default_rng(seed)
    K = dict(truth=[], cap=cap, poses1=np.zeros((B, 7)), poses2=np.zeros((B, 7)), wp1=np.zeros((B, cap, 3)), wp2=np.zeros((B, cap, 3)),
             kps1=np.zeros((B, cap), KP64_DTYPE), kps2=np.zeros((B, cap), KP64_DTYPE), frame_pt1=np.zeros((B, cap), np.int32),
             frame_pt2=np.zeros((B, cap), np.int32), n1=np.array([cap, cap - 9, cap - 30], np.int32), n2=np.array([cap - 5, cap, cap - 17], np.int32),
             n_pts1=np.array([cap, cap - 1, cap - 8], np.int32), n_pts2=np.array([cap - 1, cap, cap - 3], np.int32),
             pairs=np.full((B, cap, 2), -3, np.int32), n_pairs=np.array([cap, cap - 13, cap - 100], np.int32))
    for b in range(B):
        R, t, s = S.random_transform(rng, 1.0)
        K["truth"].append((R, t, s))
        for key in ("poses1", "poses2"):
            Rp, tp, _ = S.random_transform(rng, 1.0, angle=1.0, shift=5.0)
            K[key][b] = S.pose7(Rp.reshape(9), tp)
        P1 = S._random_points(rng, cap)
        P2 = s * P1 @ R.T + t
        for P, pose, wp in ((P1, K["poses1"][b], "wp1"), (P2, K["poses2"][b], "wp2")):
            K[wp][b] = (P - pose[4:]) @ S.quat_to_R(pose[:4])  # R^T (P - t)
        feat = {}
        for side, P in (("1", P1), ("2", P2)):
            perm = rng.permutation(cap)  # feature f belongs to point perm[f]
            shown = perm.copy()
            if side == "2":
                swap = rng.random(cap) < 0.2  # it shows another point: a wrong pair for the RANSAC
                shown[swap] = rng.integers(0, cap, int(swap.sum()))
            px = S.project(P[shown]) + 0.5 * rng.normal(size=(cap, 2))
            K["kps" + side]["x"][b], K["kps" + side]["y"][b] = px[:, 0], px[:, 1]
            K["frame_pt" + side][b] = shown
            feat[side] = np.argsort(perm)  # point -> feature
        ne = int(K["n_pairs"][b])
        pts = rng.permutation(cap)[:ne]
        pr = np.stack([feat["1"][pts], feat["2"][pts]], 1).astype(np.int32)
        for j, e in enumerate(rng.permutation(ne)[USABLE[b]:]):
            f1, f2 = pr[e]
            how = j % 6
            if how == 0:
                K["frame_pt1"][b, f1] = -1
            elif how == 1:
                K["frame_pt2"][b, f2] = -1
            elif how == 2:
                K["frame_pt1"][b, f1] = cap + 7
            elif how == 3:
                K["frame_pt2"][b, f2] = K["n_pts2"][b]
            elif how == 4:
                pr[e, 0] = (-1, cap)[j % 2]
            else:
                pr[e, 1] = (cap + 3, -2)[j % 2]
        K["pairs"][b, :ne] = pr
    return K


def gather(K, b):
    """The usable pairs of keyframe pair b as LoopDetector.cpp:163-198 gathers them from the pair list."""
    cap = K["cap"]
    pr = K["pairs"][b, : K["n_pairs"][b]]
    inside = (pr[:, 0] >= 0) & (pr[:, 0] < cap) & (pr[:, 1] >= 0) & (pr[:, 1] < cap)
    f1, f2 = pr[inside, 0], pr[inside, 1]
    v1, v2 = K["frame_pt1"][b, f1], K["frame_pt2"][b, f2]
    ok = (v1 >= 0) & (v1 < K["n_pts1"][b]) & (v2 >= 0) & (v2 < K["n_pts2"][b])
    f1, f2, v1, v2 = f1[ok], f2[ok], v1[ok], v2[ok]
    k1, k2 = K["kps1"][b, f1], K["kps2"][b, f2]
    return dict(points1=S.view_points(K["poses1"][b], K["wp1"][b, v1]), points2=S.view_points(K["poses2"][b], K["wp2"][b, v2]),
                ips1=np.stack([k1["x"], k1["y"]], 1), ips2=np.stack([k2["x"], k2["y"]], 1)), f1, v2


@pytest.fixture(scope="module", params=[1030, 2048])
def keyframes(request):
    K = make_keyframes(request.param, 3000 + request.param)
    return K, [gather(K, b) for b in range(B)]


@pytest.mark.parametrize("iterations", [0, 300])
def test_pairs_batch_dev_with_a_slab_equals_the_host_entry(keyframes, iterations):
    """The assertions of test_sim3_chain_gpu.py on a pair list written directly: T bytes, scale, inliers, match12, corrected_pose within
    transform_tolerance(), the keyframe pair with 2 usable pairs left untouched."""
    import torch

    from snake_slam_amd.loop import RegistrationRansac
    from snake_slam_amd.tracking import frames_dev

    K, G = keyframes
    cap = K["cap"]
    usable = [len(g[1]) for g in G]
    print(f"pairs_cap {cap}: {K['n_pairs'].tolist()} entries, {usable} usable")
    assert usable[0] > S.LDS_PAIRS and abs(usable[0] - USABLE[0]) <= 8 and abs(usable[1] - USABLE[1]) <= 8 and usable[2] == 2
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    D = {k: t(K[k]) for k in ("n1", "n2", "n_pts1", "n_pts2", "frame_pt1", "frame_pt2", "poses1", "poses2", "pairs", "n_pairs")}
    D["pts1"], D["pts2"] = t(K["wp1"].view(np.uint8).reshape(B, cap, 24)), t(K["wp2"].view(np.uint8).reshape(B, cap, 24))
    D["kps1"], D["kps2"] = t(K["kps1"].view(np.uint8).reshape(B, cap, 24)), t(K["kps2"].view(np.uint8).reshape(B, cap, 24))
    zeros = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt, device="cuda")  # noqa: E731
    aux = dict(desc=zeros(B, cap, 4, dt=torch.int64), rp=zeros(B, cap, dt=torch.float32), taken=zeros(B, cap, dt=torch.uint8), cs=zeros(B, 2))
    fd = [frames_dev((0.0, 0.0, 752.0, 480.0), D["n" + s], D["kps" + s], aux["desc"], aux["rp"], aux["taken"], aux["cs"]) for s in "12"]
    T0, s0, cp0 = np.tile([0.0, 0.0, 0.0, 1.0, 0.5, -0.25, 0.125], (B, 1)), np.full(B, 0.75), np.tile([0.0, 0.0, 0.0, 1.0, 9.0, 8.0, 7.0], (B, 1))
    T, scale, cpose = t(T0), t(s0), t(cp0)
    inl, match12 = torch.full((B,), -7, dtype=torch.int32, device="cuda"), torch.full((B, cap), -7, dtype=torch.int32, device="cuda")
    rs = RegistrationRansac(S.CAM, S.THRESHOLD, iterations, False, 0x5EED0000ABCD + cap)
    try:
        torch.cuda.synchronize()  # the inputs were uploaded on torch's stream, the handle runs on its own
        rs.solve_pairs_batch_dev(fd[0], fd[1], D["pairs"], D["n_pairs"], D["pts1"], D["pts2"], D["frame_pt1"], D["frame_pt2"], D["n_pts1"],
                                 D["n_pts2"], D["poses1"], D["poses2"], T, scale, inl, match12, cpose)
        torch.cuda.synchronize()
        want = rs.solve_batch([dict(g[0], T=T0[b], scale=s0[b]) for b, g in enumerate(G)])
    finally:
        rs.close()
    got_T, got_s, got_inl, got_m, got_cp = T.cpu().numpy(), scale.cpu().numpy(), inl.cpu().numpy(), match12.cpu().numpy(), cpose.cpu().numpy()
    for b in range(B):
        prob, f1, v2 = G[b]
        w = want[b]
        print(f"pair {b}: {len(f1)} pairs, {w['inliers']} inliers, winner {w['best']}")
        assert got_inl[b] == w["inliers"] and got_T[b].tobytes() == w["T"].tobytes() and got_s[b] == w["scale"], b
        m12 = np.full(cap, -1, np.int32)
        m12[f1[w["mask"].astype(bool)]] = v2[w["mask"].astype(bool)]
        assert np.array_equal(got_m[b], m12), b
        if w["best"] >= 0:
            cp = S.corrected_pose(w["T"], w["scale"], K["poses2"][b])
            d = S.transform_distance(S.quat_to_R(got_cp[b, :4]), got_cp[b, 4:], 1.0, S.quat_to_R(cp[:4]), cp[4:], 1.0)
            assert d <= S.transform_tolerance(), (b, d)
        else:
            assert np.array_equal(got_cp[b], cp0[b])
    for b in (0, 1):
        R, tt, s = K["truth"][b]
        assert want[b]["inliers"] > 0.6 * usable[b]
        assert want[b]["mask"][S.LDS_PAIRS:].any() == (b == 0)  # inliers among the pairs that live in the slab
        # the map points are exact and only the keypoints carry noise, so a triplet of true pairs gives the true transform
        assert S.transform_distance(S.quat_to_R(got_T[b, :4]), got_T[b, 4:], got_s[b], R, tt, s) <= S.transform_tolerance()
    # fewer than 3 usable pairs: outputs untouched, 0 inliers, no match
    assert got_inl[2] == 0 and np.array_equal(got_T[2], T0[2]) and got_s[2] == s0[2] and np.array_equal(got_cp[2], cp0[2])
    assert (got_m[2] == -1).all()
