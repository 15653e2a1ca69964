"""CPU: the numpy restatement of "snk-p3p v1" (tests/p3p_numpy.py) against ground truth and against itself -- the solver finds the
true pose, every solution fits its own three points, the sampler is a pure function with distinct indices and a pinned vector, the
restatement's own borderline share stays at most half the cap of the GPU test on every case that test uses, and pose_tolerance() is
the measured floor.  The edge cases of tests/test_p3p_edges_gpu.py (p3p_numpy.edge_cases()) are held to the same: their seeds are the
first that show the stated property, and the numbers of p3p.hip they are built on are read from the source."""
import re
from pathlib import Path

import numpy as np
import pytest

import p3p_numpy as P

CASES = P.gpu_cases()
EDGES = P.edge_cases()


@pytest.fixture(scope="module")
def hyps():
    return {c["name"]: P.hypotheses(c["wps"], c["nips"], c["iterations"], c["threshold"], c["seed"]) for c in CASES}


def test_case_grid_is_the_stated_one():
    assert sorted({len(c["wps"]) for c in CASES}) == [4, 30, 200, 1000]
    assert sorted({c["outlier_share"] for c in CASES}) == [0.0, 0.3, 0.6] and sorted({c["noise_px"] for c in CASES}) == [0.0, 1.0]
    assert len(CASES) == 24
    for c in CASES:
        depth = (c["wps"] @ P.quat_to_R(c["pose"][:4]).T + c["pose"][4:])[:, 2]
        assert depth.min() >= 0.5 - 1e-9 and depth.max() <= 40.0 + 1e-9


def test_sampling_is_distinct_and_a_pure_function_of_its_counters():
    for n in (4, 5, 30, 1000, 3072):
        a = P.triplets(1234567890123, 3, 2000, n)
        assert a.min() >= 0 and a.max() < n
        assert (a[:, 0] != a[:, 1]).all() and (a[:, 0] != a[:, 2]).all() and (a[:, 1] != a[:, 2]).all()
        assert np.array_equal(a, P.triplets(1234567890123, 3, 2000, n))
        assert np.array_equal(a[:100], P.triplets(1234567890123, 3, 100, n))          # hypothesis k does not depend on the count
        assert not np.array_equal(a, P.triplets(1234567890123, 4, 2000, n))           # the problem index enters
        assert not np.array_equal(a, P.triplets(1234567890123 + (1 << 40), 3, 2000, n))  # both halves of the seed enter
    # roughly uniform: every index of 30 is drawn
    assert len(np.unique(P.triplets(7, 0, 2000, 30))) == 30


def test_pinned_triplets_guard_the_hash():
    got = P.triplets(0x0123456789ABCDEF, 5, 6, 300)
    want = PINNED
    assert np.array_equal(got, want), got.tolist()


PINNED = np.array([[52, 233, 208], [66, 272, 112], [278, 160, 143], [155, 132, 129], [108, 74, 13], [32, 45, 208]], np.int32)


def test_ground_truth_pose_is_among_the_solutions_of_noise_free_triplets(hyps):
    n_checked = 0
    for c in CASES:
        if c["noise_px"] != 0.0:
            continue
        H = hyps[c["name"]]
        Rt, tt = P.quat_to_R(c["pose"][:4]), c["pose"][4:]
        clean = ~c["outlier"][H["triplets"]].any(1)
        for k in np.nonzero(clean & ~H["borderline"])[0]:
            d = [P.pose_distance(H["R"][k, s], H["t"][k, s], Rt, tt) for s in range(4) if H["valid"][k, s]]
            assert d and min(d) < 1e-8, (c["name"], int(k), d)
            n_checked += 1
    assert n_checked > 1000


def test_every_solution_reprojects_its_own_three_points(hyps):
    worst = 0.0
    for c in CASES:
        H = hyps[c["name"]]
        X, uv = c["wps"][H["triplets"]], c["nips"][H["triplets"]]
        pc = np.einsum("ksij,kpj->kspi", H["R"].reshape(-1, 4, 3, 3), X) + H["t"][:, :, None, :]
        with np.errstate(all="ignore"):
            err = np.abs(pc[..., :2] / pc[..., 2:] - uv[:, None])
        assert (pc[..., 2][H["valid"]] > 0).all()
        worst = max(worst, float(err[H["valid"]].max()))
    print(f"largest self-reprojection error {worst:.2e}")
    assert worst <= 1e-9


def test_rotations_are_rotations(hyps):
    for c in CASES:
        H = hyps[c["name"]]
        R = H["R"].reshape(-1, 4, 3, 3)[H["valid"]]
        assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-9 and np.abs(np.linalg.det(R) - 1).max() < 1e-9


def test_borderline_share_is_at_most_half_the_cap(hyps):
    for c in CASES:
        share = float(hyps[c["name"]]["borderline"].mean())
        print(f"{c['name']}: borderline share {share:.4f}")
        assert share <= 0.5 * P.BORDERLINE_CAP, (c["name"], share)


def test_ransac_recovers_the_pose_where_it_is_identifiable():
    for c in CASES:
        r = P.ransac(c["wps"], c["nips"], c["iterations"], c["threshold"], c["seed"])
        assert r["inliers"] == int(r["mask"].sum()) == len(r["matches"]) and np.array_equal(np.nonzero(r["mask"])[0], r["matches"])
        true_inl = ~c["outlier"]
        if c["noise_px"] == 0.0 and true_inl.sum() >= 4:
            assert r["mask"][true_inl].all(), c["name"]
            assert P.pose_distance(P.quat_to_R(r["pose"][:4]), r["pose"][4:], P.quat_to_R(c["pose"][:4]), c["pose"][4:]) < 1e-8, c["name"]


def test_small_and_empty_inputs():
    c = CASES[6]
    for n in (0, 1, 3):
        r = P.ransac(c["wps"][:n], c["nips"][:n], 250, c["threshold"], 1, pose=[0, 0, 0, 1, 1, 2, 3])
        assert r["inliers"] == 0 and r["best"] == (-1, -1) and np.array_equal(r["pose"], [0, 0, 0, 1, 1, 2, 3]) and len(r["mask"]) == n


def test_pose_tolerance_is_the_measured_floor():
    """pose_tolerance() = 10 x POSE_FLOOR, and POSE_FLOOR is what this test measures: the largest disagreement (largest entry of the
    rotation difference, translation difference relative to max(1, |t|)) between the closed form and the closed form polished by
    Gauss-Newton on its three points, over every solution of every hypothesis that is not borderline of the 24 cases of gpu_cases()
    and the 13 of edge_cases().  Measured 1.92e-12 on the former, 6.45e-13 on the latter, kept as 2.0e-12."""
    floor = P.measure_pose_floor(CASES)
    edge = P.measure_pose_floor(EDGES)
    print(f"closed form vs Gauss-Newton polish: {floor:.3e} on gpu_cases(), {edge:.3e} on edge_cases()")
    assert 0.5 * P.POSE_FLOOR <= max(floor, edge) <= P.POSE_FLOOR
    assert P.pose_tolerance() == 10.0 * P.POSE_FLOOR


# ------------------------------------------------------------------ the edge cases ------------
def test_edge_grid_is_the_stated_one():
    got = [(len(c["wps"]), c["outlier_share"], c["noise_px"], c["iterations"], c["property"]) for c in EDGES]
    assert got == P.edge_grid() and len({c["name"] for c in EDGES}) == len(EDGES) == 13
    assert [g[:4] for g in got[:6]] == [(63, 0.0, 0.0, 513), (64, 0.0, 0.0, 513), (65, 0.0, 0.0, 513), (255, 0.3, 1.0, 256),
                                        (256, 0.3, 1.0, 257), (257, 0.3, 1.0, 512)]
    for g, prop in zip(got[6:9], ("late", "last_group", "cross_tie")):
        assert g[0] <= 300 and 0.85 <= g[1] <= 0.9 and g[2:] == (0.0, 1024, prop)
    assert [g[:4] for g in got[9:]] == [(1489, 0.3, 1.0, 257), (1490, 0.3, 1.0, 257), (3072, 0.3, 1.0, 600), (3072, 0.0, 0.0, 300)]
    # either side of what a launch gets without raising the kernel's limit, and the maximum
    lds = lambda n: P.LDS_BYTES_PER_PAIR * n + P.LDS_BYTES_FIXED  # noqa: E731
    assert lds(1489) <= P.LDS_DEFAULT_LIMIT < lds(1490) and P.MAX_PAIRS == 3072 and lds(P.MAX_PAIRS) == 135176


def test_edge_seeds_are_the_first_that_qualify_and_borderline_share_is_at_most_half_the_cap():
    for j, (g, seed, c) in enumerate(zip(P.edge_grid(), P.EDGE_SEEDS, EDGES)):
        assert seed == P.first_edge_seed(j, g), (g, seed)
        r = P.ransac(c["wps"], c["nips"], c["iterations"], c["threshold"], c["seed"])
        share = float(r["hyp"]["borderline"].mean())
        print(f"{c['name']}: borderline share {share:.4f}, winner {r['best']}, {r['inliers']} inliers, groups at the best count {P.groups_at_best(r)}")
        assert share <= 0.5 * P.BORDERLINE_CAP, (c["name"], share)
        k = r["best"][0]
        if g[4] == "all_tie":  # every hypothesis explains every pair; the first one wins, with its first solution that does
            assert k == 0 and r["inliers"] == g[0] and len(P.groups_at_best(r)) == -(-g[3] // P.GROUP) and P.winner_is_exact(r)
            assert r["slot"] == int(np.argmax(r["hyp"]["counts"][0] == g[0]))
        if g[4] in ("late", "last_group", "cross_tie"):
            assert k >= (3 * P.GROUP if g[4] == "last_group" else P.GROUP) and P.winner_is_exact(r)
        if g[4] == "cross_tie":
            assert len(P.groups_at_best(r)) >= 2 and P.groups_at_best(r)[0] == k // P.GROUP


def test_pinned_limits_of_the_kernel():
    """The numbers the edge cases are built on, read from snake_slam_amd/csrc/p3p.hip: a moved carve fails here instead of leaving an
    edge untested."""
    src = (Path(__file__).resolve().parent.parent / "snake_slam_amd" / "csrc" / "p3p.hip").read_text()
    one = lambda pattern: (lambda m: (len(m) == 1 and m[0]) or pytest.fail(f"{pattern}: {m}"))(re.findall(pattern, src))  # noqa: E731
    assert int(one(r"constexpr int P3P_MAX_PAIRS\s*=\s*(\d+);")) == P.MAX_PAIRS
    assert one(r"constexpr int P3P_MAX_ITERATIONS\s*=\s*([^;]+);").replace(" ", "") == "1<<20" and P.MAX_ITERATIONS == 1 << 20
    assert int(one(r"for \(int k0 = 0; k0 < iterations; k0 \+= (\d+)\)")) == P.GROUP
    assert int(one(r"__launch_bounds__\((\d+)\) void p3p_ransac_kernel")) == P.GROUP
    per_pair, fixed = one(r"size_t lds_bytes\(int pairs\)\s*\{\s*return \(size_t\)pairs \* (\d+) \+ (\d+);")
    assert (int(per_pair), int(fixed)) == (P.LDS_BYTES_PER_PAIR, P.LDS_BYTES_FIXED)
    # the scoring loop walks the pairs 64 at a time, the mask / list compaction 256 at a time
    assert len(re.findall(r"for \(int i0 = 0; i0 < n; i0 \+= 64\)", src)) == 1 and len(re.findall(r"for \(int i0 = 0; i0 < n; i0 \+= 256\)", src)) == 1
    assert "pairs per problem outside [0, 3072]" in src and "frames->cap above 3072 features" in src
