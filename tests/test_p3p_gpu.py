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


def pose_dist(p7, R, t):
    return P.pose_distance(P.quat_to_R(p7[:4]), p7[4:], R, t)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_hypotheses_and_winner_match_the_restatement(solver, c):
    res, tri, ns, poses, cnt = run(solver, c)
    want = P.ransac(c["wps"], c["nips"], c["iterations"], c["threshold"], c["seed"])
    H = want["hyp"]
    assert np.array_equal(tri, H["triplets"])
    border = H["borderline"]
    print(f"{c['name']}: borderline share {border.mean():.4f}")
    assert border.mean() <= P.BORDERLINE_CAP
    ok = ~border
    assert np.array_equal(ns[ok], H["valid"].sum(1)[ok])
    worst = 0.0
    for k in np.nonzero(ok)[0]:
        slots = np.nonzero(H["valid"][k])[0]
        for j, s in enumerate(slots):
            worst = max(worst, pose_dist(poses[k, j], H["R"][k, s], H["t"][k, s]))
            assert cnt[k, j] == H["counts"][k, s], (int(k), j, cnt[k].tolist(), H["counts"][k].tolist())
    print(f"{c['name']}: largest pose difference to the restatement {worst:.2e}")
    assert worst <= P.pose_tolerance()
    # the winner
    assert res["inliers"] == int(res["mask"].sum()) == len(res["matches"])
    assert np.array_equal(np.nonzero(res["mask"])[0], res["matches"])
    kb, sb = want["best"]
    top = H["counts"].max(1)
    spread = (H["counts_hi"] - H["counts_lo"]).max(1)
    exact = kb >= 0 and not border[kb] and all(top[kb] - top[h] > spread[h] for h in np.nonzero(border)[0])
    if exact:
        assert res["best"] == want["best"] and res["inliers"] == want["inliers"]
        assert np.array_equal(res["mask"], want["mask"]) and np.array_equal(res["matches"], want["matches"])
        assert pose_dist(res["pose"], H["R"][kb, want["slot"]], H["t"][kb, want["slot"]]) <= P.pose_tolerance()
    elif kb >= 0:
        assert res["inliers"] >= H["counts_lo"][kb, want["slot"]]
    if res["best"][0] >= 0:
        Rg, tg = P.quat_to_R(res["pose"][:4]).reshape(9), res["pose"][4:]
        lo = P.inlier_mask(Rg, tg, c["wps"], c["nips"], c["threshold"] * (1 - P.BORDERLINE))
        hi = P.inlier_mask(Rg, tg, c["wps"], c["nips"], c["threshold"] * (1 + P.BORDERLINE))
        m = res["mask"].astype(bool)
        assert (m[lo]).all() and not (m[~hi]).any()
    true_inl = ~c["outlier"]
    if c["noise_px"] == 0.0 and true_inl.sum() >= 4:
        assert res["mask"][true_inl].all()
        assert pose_dist(res["pose"], P.quat_to_R(c["pose"][:4]), c["pose"][4:]) <= P.pose_tolerance()


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
