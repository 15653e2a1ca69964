"""GPU: snk_sim3_debug_hypotheses / snk_sim3_ransac against the numpy restatement of "snk-sim3 v1" (tests/sim3_numpy.py) on the 37 cases
of sim3_numpy.gpu_cases(): n in {3, 4, 63, 64, 65, 200} x 0 / 30 / 60 % wrong pairs x 0 / 1 px keypoint noise, every n with
compute_scale on (true scale 0.8) and off and with 1, 100 and 300 iterations (300 crosses a round of 256 hypotheses), and n = 2048 once.

Decisions are compared with a borderline rule, not bit for bit.  A hypothesis is borderline when its inlier count differs between
threshold (1 - g) and threshold (1 + g), g = 1e-6, when its triplet is ill-conditioned (|cross|^2 / (side^2 side^2) <= 1e-6 in
either point set) or when the two largest eigenvalues of N are within 1e-6 (relative); at most 2 % of a case's hypotheses may be
(asserted; a condition on the cases, which tests/test_sim3_numpy.py checks on the CPU).  Transforms agree within
sim3_numpy.transform_tolerance() = 4.5e-5 = 10 x the measured floor between the restatement and Umeyama's SVD form (4.19e-6,
tests/test_sim3_numpy.py::test_transform_tolerance_is_the_measured_floor; well-conditioned triplets agree to 1e-13).

The ground-truth check (0 px noise: the mask holds every true pair, the transform is the true one) applies where the restatement's
own winner is a triplet of true pairs."""
import numpy as np
import pytest

import sim3_numpy as S

pytestmark = pytest.mark.gpu

CASES = S.gpu_cases()


@pytest.fixture(scope="module")
def solver():
    from snake_slam_amd.loop import RegistrationRansac

    s = RegistrationRansac(S.CAM, S.THRESHOLD, 100, False, 0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def restated():
    return {c["name"]: S.ransac(c["P1"], c["P2"], c["ip1"], c["ip2"], c["iterations"], c["threshold"], c["compute_scale"], c["seed"])
            for c in CASES}


def setup(solver, c, iterations=None):
    p = solver.params
    p.iterations, p.threshold, p.seed = (c["iterations"] if iterations is None else iterations), c["threshold"], c["seed"]
    p.compute_scale = int(c["compute_scale"])
    return dict(points1=c["P1"], points2=c["P2"], ips1=c["ip1"], ips2=c["ip2"])


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_hypotheses_and_winner_match_the_restatement(solver, restated, c):
    """The comparison is sim3_numpy.check_device_against_restatement, shared with tests/test_sim3_edges_gpu.py."""
    S.check_device_against_restatement(c, restated[c["name"]], *solver.debug_hypotheses(**setup(solver, c)))


def test_ground_truth_check_applies_to_the_clean_and_30_percent_cases(restated):
    for c in CASES:
        if c["noise_px"] == 0.0 and c["outlier_share"] <= 0.3 and (~c["outlier"]).sum() >= 3:
            r = restated[c["name"]]
            assert r["best"] >= 0 and not c["outlier"][r["hyp"]["triplets"][r["best"]]].any(), c["name"]


def test_small_all_wrong_and_oversized_inputs_return_cleanly(solver):
    from snake_slam_amd._lib import SnakeHipError

    c = CASES[30]
    T0, s0 = [0.0, 0.0, 0.0, 1.0, 1.0, 2.0, 3.0], 0.5
    prob = setup(solver, c, 100)
    assert solver.solve_batch([]) == []
    for n in (0, 1, 2):
        r = solver.solve_batch([dict({k: v[:n] for k, v in prob.items()}, T=T0, scale=s0)])[0]
        assert r["inliers"] == 0 and r["best"] == -1 and np.array_equal(r["T"], T0) and r["scale"] == s0 and len(r["mask"]) == n
    res, tri, valid, Ts, sc, cnt = solver.debug_hypotheses(c["P1"][:2], c["P2"][:2], c["ip1"][:2], c["ip2"][:2], T=T0, scale=s0)
    assert res["inliers"] == 0 and not valid.any() and not cnt.any()
    # every pair wrong: whatever wins explains little more than its own three pairs, and the outputs stay consistent
    rng = np.random.default_rng(3)
    P2 = S._random_points(rng, 200)
    r = solver.solve_batch([dict(prob, points2=P2, ips2=S.project(P2), T=T0, scale=s0)])[0]
    w = S.ransac(c["P1"], P2, c["ip1"], S.project(P2), 100, c["threshold"], c["compute_scale"], c["seed"], T=T0, scale=s0)
    assert r["inliers"] == int(r["mask"].sum()) and r["inliers"] < 20
    assert r["inliers"] >= w["inliers"] - int((w["hyp"]["counts_hi"] - w["hyp"]["counts_lo"]).max())
    if r["best"] < 0:
        assert np.array_equal(r["T"], T0) and r["scale"] == s0
    # one pair more than the cap: refused with an error text, nothing launched, the handle stays usable
    big = {k: np.concatenate([v] * 11)[:2049] for k, v in prob.items()}
    with pytest.raises(SnakeHipError, match="2048"):
        solver.solve_batch([big])
    with pytest.raises(SnakeHipError, match="2048"):
        solver.debug_hypotheses(big["points1"], big["points2"], big["ips1"], big["ips2"])
    assert solver.solve_batch([prob])[0]["inliers"] > 0


@pytest.mark.parametrize("n", [14, 16, 20, 150])
def test_zero_iterations_use_the_table_count(solver, n):
    from snake_slam_amd.loop import ransac_iterations

    c = CASES[33]
    prob = {k: v[:n] for k, v in setup(solver, c, 0).items()}
    its = ransac_iterations(n, 0.999, 15, 100)
    assert its == S.ransac_iterations(n) == solver.ransac_iterations(n)
    a = solver.debug_hypotheses(**prob)
    assert len(a[1]) == its
    solver.params.iterations = its
    b = solver.debug_hypotheses(**prob)
    assert a[0]["T"].tobytes() == b[0]["T"].tobytes() and a[0]["best"] == b[0]["best"] and a[0]["mask"].tobytes() == b[0]["mask"].tobytes()
    for x, y in zip(a[1:], b[1:]):
        assert x.tobytes() == y.tobytes()
    solver.params.iterations = 0
    r = solver.solve_batch([prob])[0]
    assert r["T"].tobytes() == a[0]["T"].tobytes() and r["inliers"] == a[0]["inliers"]


def odd_batch(seed=4500):
    """three problems of 3, 0 and 65 pairs (Sim3, 30 % wrong pairs, 1 px noise, 100 iterations): 68 pairs in all, so the mask ends off
    a 16-byte boundary and begins on the padding behind three result records (stage.hpp); one problem is empty, and 65 crosses the
    64 / 65 case.  Shared with the sim3 seam of tests/backend_cases.py."""
    return [S.make_case(n, 0.3, 1.0, True, 100, seed + i) for i, n in enumerate((3, 0, 65))]


def test_batch_whose_parts_end_off_a_16_byte_boundary(solver):
    """The winner's part of sim3_numpy.check_device_against_restatement, against the restatement under the problem's index; the empty
    problem by what the header says of n < 3: T and scale as they came in, no inlier, no winner."""
    cs, seed, T0, s0 = odd_batch(), 0xABCDEF0123456789, [0.0, 0.0, 0.0, 1.0, 1.0, 2.0, 3.0], 0.5
    probs = [dict(setup(solver, c, 100), T=T0, scale=s0) for c in cs]
    solver.params.seed = seed
    res = solver.solve_batch(probs)
    for i, (r, c) in enumerate(zip(res, cs)):
        n = len(c["P1"])
        assert len(r["mask"]) == n and r["inliers"] == int(r["mask"].sum())
        if n == 0:
            assert r["inliers"] == 0 and r["best"] == -1 and np.array_equal(r["T"], T0) and r["scale"] == s0
            continue
        w = S.ransac(c["P1"], c["P2"], c["ip1"], c["ip2"], 100, c["threshold"], True, seed, problem=i, T=T0, scale=s0)
        H, kb = w["hyp"], w["best"]
        if S.winner_is_exact(w):
            assert r["best"] == kb and r["inliers"] == w["inliers"] and np.array_equal(r["mask"], w["mask"]), (i, r["best"], kb)
            assert S.device_distance(r["T"], r["scale"], H["R"][kb], H["t"][kb], H["s"][kb]) <= S.transform_tolerance()
        elif kb >= 0:
            assert r["inliers"] >= H["counts_lo"][kb]
        else:
            assert r["best"] == -1 or H["borderline"][r["best"]]
        if r["best"] < 0:
            assert r["inliers"] == 0 and np.array_equal(r["T"], T0) and r["scale"] == s0


def test_batch_uses_the_problem_index_and_two_runs_give_identical_bytes(solver):
    sel = [c for c in CASES if c["compute_scale"] and len(c["P1"]) >= 63]
    probs = [setup(solver, c, 300) for c in sel]
    seed = 0xABCDEF0123456789
    solver.params.seed = seed
    a = solver.solve_batch(probs)
    b = solver.solve_batch(probs)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x["T"].tobytes() == y["T"].tobytes() and x["mask"].tobytes() == y["mask"].tobytes()
        assert x["scale"] == y["scale"] and x["best"] == y["best"] and x["inliers"] == y["inliers"]
        c = sel[i]
        w = S.ransac(c["P1"], c["P2"], c["ip1"], c["ip2"], 300, c["threshold"], True, seed, problem=i)
        if x["best"] == w["best"]:
            assert x["inliers"] == w["inliers"] or w["hyp"]["borderline"][w["best"]]
        H, kb = w["hyp"], w["best"]
        spread = H["counts_hi"] - H["counts_lo"]
        if not H["borderline"][kb] and all(H["counts"][kb] - H["counts"][h] > spread[h] for h in np.nonzero(H["borderline"])[0]):
            assert x["best"] == kb, (i, x["best"], kb)  # the winner of problem i comes from the triplets of problem index i
    r1 = solver.debug_hypotheses(**probs[3])
    r2 = solver.debug_hypotheses(**probs[3])
    for x, y in zip(r1[1:], r2[1:]):
        assert x.tobytes() == y.tobytes()
