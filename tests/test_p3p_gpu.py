"""GPU: snk_p3p_debug_hypotheses / snk_p3p_ransac against the numpy restatement of "snk-p3p v1" (tests/p3p_numpy.py) on 24 cases
(n in {4, 30, 200, 1000} x 0 / 30 / 60 % wrong pairs x 0 / 1 px keypoint noise).

Decisions are compared with a borderline rule, not bit for bit.  A hypothesis is borderline when its inlier count differs between
threshold (1 - g) and threshold (1 + g), g = 1e-6, when its triplet is ill-conditioned by p3p_numpy.ill_conditioned, or when the
restatement's two formulations disagree on the number of solutions; at most 2 % of a case's hypotheses may be (asserted).  Poses pair
up within p3p_numpy.pose_tolerance() = 2.0e-11 = 10 x the measured floor between the closed form and its Gauss-Newton polish
(1.92e-12, tests/test_p3p_numpy.py::test_pose_tolerance_is_the_measured_floor).

The ground-truth check (0 px noise: the mask holds every true inlier, the pose is the true one) applies where the pose is identifiable:
at least 4 true inliers.  With n = 4 and 30 / 60 % wrong pairs 3 / 2 true inliers are left, every hypothesis through a wrong pair fits
its own three points just as well, and no rule can prefer the true pose."""
import numpy as np
import pytest

import p3p_numpy as P

pytestmark = pytest.mark.gpu

CASES = P.gpu_cases()


@pytest.fixture(scope="module")
def solver():
    from snake_slam_amd.tracking import P3PRansac

    s = P3PRansac(250, P.THRESHOLD, 0)
    yield s
    s.close()


def run(solver, c, debug=True):
    solver.params.iterations, solver.params.residual_threshold, solver.params.seed = c["iterations"], c["threshold"], c["seed"]
    if debug:
        return solver.debug_hypotheses(c["wps"], c["nips"])
    return solver.solve_batch([dict(wps=c["wps"], nips=c["nips"])])[0]


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_hypotheses_and_winner_match_the_restatement(solver, c):
    """The comparison is p3p_numpy.check_device_against_restatement, shared with tests/test_p3p_edges_gpu.py."""
    want = P.ransac(c["wps"], c["nips"], c["iterations"], c["threshold"], c["seed"])
    P.check_device_against_restatement(c, want, *run(solver, c))


def test_small_all_outlier_and_empty_inputs_return_cleanly(solver):
    c = CASES[12]
    solver.params.iterations, solver.params.residual_threshold, solver.params.seed = 250, c["threshold"], 5
    start = [0.0, 0.0, 0.0, 1.0, 1.0, 2.0, 3.0]
    assert solver.solve_batch([]) == []
    for n in (0, 1, 3):
        r = solver.solve_batch([dict(wps=c["wps"][:n], nips=c["nips"][:n], pose=start)])[0]
        assert r["inliers"] == 0 and r["best"] == (-1, -1) and np.array_equal(r["pose"], start) and not r["mask"].any()
    res, tri, ns, poses, cnt = solver.debug_hypotheses(c["wps"][:3], c["nips"][:3], pose=start)
    assert res["inliers"] == 0 and not ns.any() and not cnt.any()
    # every pair wrong: whatever wins explains little more than its own three points, and the outputs stay consistent
    rng = np.random.default_rng(3)
    nips = np.stack([(rng.uniform(0, 752, 200) - P.CX) / P.FX, (rng.uniform(0, 480, 200) - P.CY) / P.FY], 1)
    r = solver.solve_batch([dict(wps=c["wps"], nips=nips, pose=start)])[0]
    w = P.ransac(c["wps"], nips, 250, c["threshold"], 5, pose=start)
    assert r["inliers"] == int(r["mask"].sum()) == len(r["matches"]) and r["inliers"] < 20
    assert r["inliers"] >= w["inliers"] - int((w["hyp"]["counts_hi"] - w["hyp"]["counts_lo"]).max()) if w["hyp"] is not None else True
    solver.params.iterations = 0
    r = solver.solve_batch([dict(wps=c["wps"], nips=c["nips"], pose=start)])[0]
    assert r["inliers"] == 0 and r["best"] == (-1, -1) and np.array_equal(r["pose"], start)


def odd_batch(seed=4400):
    """three problems of 5, 0 and 33 pairs (30 % wrong pairs, 1 px noise): 38 pairs in all, so the world points (24 bytes a pair), the
    match list and the mask end off a 16-byte boundary and the parts behind them begin on padding (stage.hpp); one problem is empty.
    Shared with the p3p seam of tests/backend_cases.py."""
    return [P.make_case(n, 0.3, 1.0, seed + i) for i, n in enumerate((5, 0, 33))]


def test_batch_whose_parts_end_off_a_16_byte_boundary(solver):
    """The winner's part of p3p_numpy.check_device_against_restatement, against the restatement under the problem's index; the empty
    problem by what the header says of n < 4: the pose as it came in, no inlier, no winner."""
    cs, seed, start = odd_batch(), 0xABCDEF0123456789, [0.0, 0.0, 0.0, 1.0, 1.0, 2.0, 3.0]
    solver.params.iterations, solver.params.residual_threshold, solver.params.seed = 250, P.THRESHOLD, seed
    res = solver.solve_batch([dict(wps=c["wps"], nips=c["nips"], pose=start) for c in cs])
    for i, (r, c) in enumerate(zip(res, cs)):
        n = len(c["wps"])
        assert len(r["mask"]) == n and r["inliers"] == int(r["mask"].sum()) == len(r["matches"])
        assert np.array_equal(r["matches"], np.nonzero(r["mask"])[0])
        if n == 0:
            assert r["inliers"] == 0 and r["best"] == (-1, -1) and np.array_equal(r["pose"], start)
            continue
        w = P.ransac(c["wps"], c["nips"], 250, P.THRESHOLD, seed, problem=i, pose=start)
        H, (kb, _) = w["hyp"], w["best"]
        if P.winner_is_exact(w):
            assert r["best"] == w["best"] and r["inliers"] == w["inliers"], (i, r["best"], w["best"])
            assert np.array_equal(r["mask"], w["mask"]) and np.array_equal(r["matches"], w["matches"])
            assert P.device_pose_distance(r["pose"], H["R"][kb, w["slot"]], H["t"][kb, w["slot"]]) <= P.pose_tolerance()
        elif kb >= 0:
            assert r["inliers"] >= H["counts_lo"][kb, w["slot"]]


def test_batch_uses_the_problem_index_and_two_runs_give_identical_bytes(solver):
    probs = [dict(wps=c["wps"], nips=c["nips"]) for c in CASES[6:]]
    solver.params.iterations, solver.params.residual_threshold, solver.params.seed = 250, P.THRESHOLD, 0xABCDEF0123456789
    a = solver.solve_batch(probs)
    b = solver.solve_batch(probs)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x["pose"].tobytes() == y["pose"].tobytes() and x["mask"].tobytes() == y["mask"].tobytes()
        assert x["matches"].tobytes() == y["matches"].tobytes() and x["best"] == y["best"] and x["inliers"] == y["inliers"]
        w = P.ransac(probs[i]["wps"], probs[i]["nips"], 250, P.THRESHOLD, 0xABCDEF0123456789, problem=i)
        assert np.array_equal(P.triplets(0xABCDEF0123456789, i, 250, len(probs[i]["wps"])), w["hyp"]["triplets"])
        if x["best"] == w["best"]:
            assert x["inliers"] == w["inliers"] or w["hyp"]["borderline"][w["best"][0]]
    r1 = solver.debug_hypotheses(probs[3]["wps"], probs[3]["nips"])
    r2 = solver.debug_hypotheses(probs[3]["wps"], probs[3]["nips"])
    for x, y in zip(r1[1:], r2[1:]):
        assert x.tobytes() == y.tobytes()
