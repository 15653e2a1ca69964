"""CPU: the numpy restatement of "snk-sim3 v1" (tests/sim3_numpy.py) against an independent closed form (Umeyama by
numpy.linalg.svd), against ground truth and against itself: the transform of random triplets agrees with the SVD form within the
recorded floor, noise-free scenes give back their transform, the iteration count is pinned, the case grid is the stated one with
seeds that qualify, and the restatement's own borderline share stays within the cap of the GPU test on every case that test uses.
The edge cases of tests/test_sim3_edges_gpu.py (sim3_numpy.edge_cases()) are held to the same with half the cap: their seeds are the
first that show the stated property, and the numbers of sim3.hip they are built on are read from the source."""
import re
from pathlib import Path

import numpy as np
import pytest

import sim3_numpy as S

CASES = S.gpu_cases()
EDGES = S.edge_cases()


@pytest.fixture(scope="module")
def runs():
    return {c["name"]: S.ransac(c["P1"], c["P2"], c["ip1"], c["ip2"], c["iterations"], c["threshold"], c["compute_scale"], c["seed"])
            for c in CASES}


def test_transform_tolerance_is_the_measured_floor():
    """transform_tolerance() = 10 x TRANSFORM_FLOOR, and TRANSFORM_FLOOR is what this test measures: the largest disagreement (largest
    entry of the rotation difference, translation difference relative to max(1, |t|), relative scale difference) between the
    restatement and Umeyama's SVD form over 20 000 random triplets (a random similarity plus 1 mm of noise, half with the scale
    estimated) that are not ill-conditioned by the borderline marks, and over the triplets of every valid hypothesis that is not
    borderline of edge_cases().  Measured 4.19e-6 on the former, 6.72e-8 on the latter, kept as 4.5e-6.  The figure is set
    by the few triplets whose two largest eigenvalues are just over 1e-6 apart (relative): Newton's root of the quartic carries
    eps / gap there and the adjugate column eps / gap^2; the median over the same triplets is printed."""
    floor = S.measure_transform_floor()
    edge = S.measure_case_floor(EDGES)
    print(f"restatement vs SVD form: {floor:.3e} on random triplets, {edge:.3e} on edge_cases()")
    assert 0.5 * S.TRANSFORM_FLOOR <= max(floor, edge) <= S.TRANSFORM_FLOOR
    assert S.transform_tolerance() == 10.0 * S.TRANSFORM_FLOOR


def test_well_conditioned_triplets_agree_with_the_svd_form_to_rounding():
    rng = np.random.default_rng(11)
    K = 2000
    A = S._random_points(rng, 3 * K).reshape(K, 3, 3)
    B = S._random_points(rng, 3 * K).reshape(K, 3, 3)  # unrelated triplets: a pure least-squares fit
    for cs in (True, False):
        q, R, t, s, valid, det = S.solve(A, B, cs, detail=True)
        keep = np.nonzero(valid & (det["flat"] > 1e-2) & (det["gap"] > 1e-2))[0]
        assert len(keep) > K // 2
        d = []
        for k in keep:
            Ru, tu, su = S.umeyama(A[k], B[k], cs)
            d.append(S.transform_distance(R[k], t[k], s[k], Ru, tu, su))
        print(f"compute_scale={cs}: median {np.median(d):.2e}, max {np.max(d):.2e} over {len(keep)} triplets")
        assert np.max(d) < 1e-9
        Rm = R[keep].reshape(-1, 3, 3)
        assert np.abs(Rm @ Rm.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.det(Rm) - 1).max() < 1e-12
        assert (q[keep, 3] >= 0).all() and np.abs(np.linalg.norm(q[keep], axis=1) - 1).max() < 1e-14


def test_degenerate_triplets_give_no_hypothesis():
    A = np.array([[[0, 0, 1.0], [1, 0, 1], [2, 0, 1]], [[0, 0, 1.0], [0, 0, 1], [1, 1, 2]], [[0, 0, 1.0], [1, 0, 1], [0, 1, 1]]])
    B = np.array([[[0, 0, 1.0], [1, 0, 1], [0, 1, 1]], [[0, 0, 1.0], [1, 0, 1], [0, 1, 1]], [[0, 0, 2.0], [1, 1, 3], [2, 2, 4]]])
    for cs in (True, False):
        assert not S.solve(A, B, cs)[4].any() and not S.solve(B, A, cs)[4].any()


def test_ransac_iterations_values():
    assert [S.ransac_iterations(n) for n in (14, 15, 16, 20, 150, 2048)] == [1, 1, 4, 13, 100, 100]
    assert S.ransac_iterations(0) == 1 and S.ransac_iterations(16, 0.999, 15, 3) == 3 and S.ransac_iterations(10**9) == 100


def test_case_grid_is_the_stated_one():
    assert sorted({len(c["P1"]) for c in CASES}) == [3, 4, 63, 64, 65, 200, 2048] and sum(len(c["P1"]) == 2048 for c in CASES) == 1
    small = [c for c in CASES if len(c["P1"]) <= 200]
    for n in (3, 4, 63, 64, 65, 200):
        mine = [c for c in small if len(c["P1"]) == n]
        assert sorted({c["outlier_share"] for c in mine}) == [0.0, 0.3, 0.6] and sorted({c["noise_px"] for c in mine}) == [0.0, 1.0]
        assert {c["compute_scale"] for c in mine} == {True, False} and {c["iterations"] for c in mine} == {1, 100, 300}
    for c in CASES:
        assert c["s"] == (0.8 if c["compute_scale"] else 1.0)
        good = ~c["outlier"]
        assert (c["P1"][:, 2] > 0).all() and (c["P2"][good, 2] > 0).all()


def test_case_seeds_are_the_first_that_qualify():
    for j, (g, seed) in enumerate(zip(S.case_grid(), S.CASE_SEEDS)):
        first = next(o for o in range(50) if S.case_ok(S.make_case(*g, 1000 * j + o)))
        assert seed == 1000 * j + first, (g, seed, first)


def test_borderline_share_is_within_the_cap(runs):
    for c in CASES:
        share = float(runs[c["name"]]["hyp"]["borderline"].mean())
        print(f"{c['name']}: borderline share {share:.4f}")
        assert share <= S.BORDERLINE_CAP, (c["name"], share)


def test_ground_truth_is_recovered_without_noise(runs):
    checked = 0
    for c in CASES:
        r = runs[c["name"]]
        assert r["inliers"] == int(r["mask"].sum())
        H = r["hyp"]
        if c["noise_px"] != 0.0 or r["best"] < 0 or c["outlier"][H["triplets"][r["best"]]].any():
            continue
        d = S.transform_distance(S.quat_to_R(r["T"][:4]), r["T"][4:], r["scale"], c["R"], c["t"], c["s"])
        assert d <= S.transform_tolerance(), (c["name"], d)
        assert r["mask"][~c["outlier"]].all(), c["name"]
        checked += 1
    shares = {(len(c["P1"]), c["outlier_share"]) for c in CASES if c["noise_px"] == 0.0}
    assert checked >= len([k for k in shares if k[1] <= 0.3 and k != (3, 0.3)])


def test_small_and_empty_inputs():
    c = CASES[-2]
    T0 = np.array([0, 0, 0, 1.0, 1, 2, 3])
    for n in (0, 1, 2):
        r = S.ransac(c["P1"][:n], c["P2"][:n], c["ip1"][:n], c["ip2"][:n], 100, 12.0, True, 1, T=T0, scale=0.5)
        assert r["inliers"] == 0 and r["best"] == -1 and np.array_equal(r["T"], T0) and r["scale"] == 0.5 and len(r["mask"]) == n


def test_corrected_pose_maps_world_points_like_the_sim3_chain():
    """DSim3(T, s)^-1 * DSim3(pose2, 1) maps p_w to (1 / s) R^T R2 p_w + R^T (t2 - t) / s; its .se3() (LoopDetector.cpp:278) keeps
    that rotation and translation and drops the factor 1 / s in front of the rotation."""
    rng = np.random.default_rng(5)
    R, t, s = S.random_transform(rng, 0.8)
    T = np.concatenate([S.pose7(R.reshape(9), t)[:4], t])
    R2, t2, _ = S.random_transform(rng, 1.0)
    pose2 = S.pose7(R2.reshape(9), t2)
    cp = S.corrected_pose(T, s, pose2)
    pw = rng.normal(size=(10, 3))
    want = pw @ R2.T @ R + ((t2 - t) @ R) / s
    assert np.abs(S.view_points(cp, pw) - want).max() < 1e-12


# ------------------------------------------------------------------ the edge cases ------------
def test_edge_grid_is_the_stated_one():
    got = [(len(c["P1"]), c["outlier_share"], c["noise_px"], c["compute_scale"], c["iterations"], c["property"]) for c in EDGES]
    assert got == S.edge_grid() and len({c["name"] for c in EDGES}) == len(EDGES) == 10
    assert [(g[0], g[3], g[4]) for g in got[:8]] == [(n, cs, 300) for n in (1023, 1024, 1025, 1280) for cs in (True, False)]
    assert got[8][0] <= 200 and got[8][1:3] == (0.9, 0.0) and got[8][4:] == (1024, "late") and got[9][4:] == (1024, "cross_tie")
    assert S.LDS_PAIRS == 1024 and S.MAX_PAIRS == 2048


def test_edge_seeds_are_the_first_that_qualify_and_borderline_share_is_at_most_half_the_cap():
    for j, (g, seed, c) in enumerate(zip(S.edge_grid(), S.EDGE_SEEDS, EDGES)):
        assert seed == S.first_edge_seed(j, g), (g, seed)
        r = S.ransac(c["P1"], c["P2"], c["ip1"], c["ip2"], c["iterations"], c["threshold"], c["compute_scale"], c["seed"])
        share = float(r["hyp"]["borderline"].mean())
        print(f"{c['name']}: borderline share {share:.4f}, winner {r['best']}, {r['inliers']} inliers, groups at the best count {S.groups_at_best(r)}")
        assert share <= 0.5 * S.BORDERLINE_CAP, (c["name"], share)
        if g[5] in ("late", "cross_tie"):
            assert r["best"] >= S.GROUP and S.winner_is_exact(r)
        if g[5] == "cross_tie":
            assert len(S.groups_at_best(r)) >= 2 and S.groups_at_best(r)[0] == r["best"] // S.GROUP


def test_pinned_limits_of_the_kernel():
    """The numbers the edge cases are built on, read from snake_slam_amd/csrc/sim3.hip: a moved carve fails here instead of leaving an
    edge untested."""
    src = (Path(__file__).resolve().parent.parent / "snake_slam_amd" / "csrc" / "sim3.hip").read_text()
    one = lambda pattern: (lambda m: (len(m) == 1 and m[0]) or pytest.fail(f"{pattern}: {m}"))(re.findall(pattern, src))  # noqa: E731
    assert int(one(r"constexpr int SIM3_MAX_PAIRS\s*=\s*(\d+);")) == S.MAX_PAIRS
    assert int(one(r"constexpr int SIM3_LDS_PAIRS\s*=\s*(\d+);")) == S.LDS_PAIRS
    assert int(one(r"for \(int k0 = 0; k0 < iterations; k0 \+= (\d+)\)")) == S.GROUP
    assert int(one(r"__launch_bounds__\((\d+)\) void sim3_ransac_kernel")) == S.GROUP
    per_pair, per_index = one(r"return \(size_t\)lds_pairs \* (\d+) \+ \(size_t\)idx_pairs \* (\d+);")
    assert (int(per_pair), int(per_index)) == (S.BYTES_PER_PAIR, 8)
    # the slab: ten doubles a pair, one slab_cap per problem
    assert len(re.findall(r"slab \+ \(size_t\)b \* \(size_t\)slab_cap \* 10", src)) == 1
    assert len(re.findall(r"\(size_t\)slab_cap \* 80 \+ 64", src)) == 2
    assert "pairs per problem outside [0, 2048]" in src and "pairs_cap outside [1, 2048]" in src
