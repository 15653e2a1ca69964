"""CPU: the numpy restatement of snk-pgo v1 against itself and against an independent minimiser.

exp(log(T)) = T and the exact Jacobians against central differences for se3 and sim3, with angles near 0, on both sides of the
series thresholds and sigma near 0; the LM optimum against scipy.optimize.least_squares on the same residual, parametrised
independently (an additive tangent vector per free vertex around the START pose, not the right perturbation of the current one),
which is where the floor behind pose_tolerance() is measured."""
import numpy as np
import pytest

import pgo_numpy as P


def _tangents(sim3):
    rng = np.random.default_rng(77)
    xs = []
    for theta in (0.0, 1e-9, 1e-5, 0.999 * P.TH_THETA, 1.001 * P.TH_THETA, 0.1, 0.3, 1.0, 2.5):
        for sigma in ((0.0, 1e-12, 0.5 * P.TH_SIGMA, 2 * P.TH_SIGMA, -1e-4, 0.05, -0.3) if sim3 else (0.0,)):
            d = rng.standard_normal(3)
            xs.append(np.concatenate([rng.standard_normal(3), theta * d / np.linalg.norm(d), [sigma]]))
    return np.array(xs)


@pytest.mark.parametrize("sim3", [False, True], ids=["se3", "sim3"])
def test_exp_log_round_trip(sim3):
    x = _tangents(sim3)
    T = P.exp(x)
    assert np.abs(np.linalg.norm(T[:, :4], axis=1) - 1).max() < 1e-15
    assert np.abs(P.log(T) - x).max() < 1e-11
    assert P.pose_distance(P.exp(P.log(T)), T) < 1e-12
    # against the matrix exponential of the 4 x 4 generator
    from scipy.linalg import expm

    for xi, Ti in zip(x, T):
        M = np.zeros((4, 4))
        M[:3, :3] = P.skew(xi[3:6]) + xi[6] * np.eye(3)
        M[:3, 3] = xi[:3]
        E = expm(M)
        assert np.abs(E[:3, :3] - Ti[7] * P.quat_R(Ti[:4])).max() < 1e-12 and np.abs(E[:3, 3] - Ti[4:7]).max() < 1e-12


def test_w_coefficients_are_continuous_across_the_thresholds():
    for sigma in (0.0, 1e-9, 0.2, -0.4):
        a = np.array(P.w_coeffs(0.9999999 * P.TH_THETA, sigma))
        b = np.array(P.w_coeffs(1.0000001 * P.TH_THETA, sigma))
        assert np.abs(a - b).max() < 1e-9
    for theta in (0.0, 1e-3, 0.5):
        a = np.array(P.w_coeffs(theta, 0.999 * P.TH_SIGMA))
        b = np.array(P.w_coeffs(theta, 1.001 * P.TH_SIGMA))
        assert np.abs(a - b).max() < 1e-10


@pytest.mark.parametrize("sim3", [False, True], ids=["se3", "sim3"])
def test_jacobians_against_central_differences(sim3):
    rng = np.random.default_rng(5)
    x = _tangents(sim3)
    x[:, :3] *= 0.1
    x = x[np.linalg.norm(x, axis=1) < 0.6]  # the residuals the series is meant for
    E = len(x)
    D = 7 if sim3 else 6
    n = 2 * E
    poses = P.exp(np.concatenate([rng.standard_normal((n, 3)), 0.5 * rng.standard_normal((n, 3)),
                                  0.2 * rng.standard_normal((n, 1)) * sim3], -1))
    edges = np.stack([np.arange(E), np.arange(E) + E], -1)
    w = 0.5 + rng.random(E)
    # measurements such that the residual is exactly the tangent wanted: M = T_i^-1 T_j exp(x)^-1
    meas = P.mul(P.measurements_from(poses, edges), P.inv(P.exp(x)))
    r, Ji, Jj = P.edge_terms(poses, edges, w, meas, not sim3)
    assert np.abs(r[:, :D] - w[:, None] * x[:, :D]).max() < 1e-10
    h = 1e-6
    for side, J in ((0, Ji), (1, Jj)):
        for a in range(D):
            d = np.zeros((n, 7))
            d[edges[:, side], a] = h
            rp = P.edge_terms(P.mul(poses, P.exp(d)), edges, w, meas, not sim3, jacobians=False)
            rm = P.edge_terms(P.mul(poses, P.exp(-d)), edges, w, meas, not sim3, jacobians=False)
            assert np.abs((rp - rm) / (2 * h) - J[:, :, a]).max() < 2e-8, (side, a)


def _least_squares(G):
    from scipy.optimize import least_squares

    G = P.prepare(G)
    fv = np.nonzero(G["row"] >= 0)[0]
    D = 6 if G["fix_scale"] else 7
    if len(fv) == 0:
        return G["start"].copy()

    def poses_of(z):
        d = np.zeros((len(fv), 7))
        d[:, :D] = z.reshape(-1, D)
        p = G["start"].copy()
        p[fv] = P.mul(P.exp(d), G["start"][fv])  # a left, additive chart around the start: not the solver's parametrisation
        return p

    def fun(z):
        return P.edge_terms(poses_of(z), G["edges"], G["weights"], G["meas"], G["fix_scale"], jacobians=False)[:, :D].ravel()

    res = least_squares(fun, np.zeros(len(fv) * D), x_scale=1.0, xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=400)
    p = poses_of(res.x)
    p[:, :4] /= np.linalg.norm(p[:, :4], axis=1)[:, None]
    return p


@pytest.mark.parametrize("fix_scale", [1, 0], ids=["se3", "sim3"])
def test_lm_optimum_against_least_squares(fix_scale):
    worst = 0.0
    for G in P.reference_graphs(fix_scale):
        poses, info = P.optimise(G)
        want = _least_squares(G)
        d = P.pose_distance(poses, want)
        worst = max(worst, d)
        print(f"{G['name']} fix_scale={fix_scale}: cost {info['cost_initial']:.3e} -> {info['cost_final']:.3e} in {info['lm_iterations']} iterations, "
              f"pose difference to least_squares {d:.2e}")
        Gp = P.prepare(G)
        assert info["cost_final"] <= info["cost_initial"]
        assert abs(info["cost_final"] - P.cost(Gp, want)) <= 1e-9 * max(1.0, info["cost_final"])
        r0 = P.edge_terms(Gp["start"], Gp["edges"], Gp["weights"], Gp["meas"], fix_scale, jacobians=False)
        assert np.linalg.norm(r0, axis=1).max() < 0.35, "the generators keep the residuals in the range the series is meant for"
    print(f"floor fix_scale={fix_scale}: {worst:.3e}")
    assert worst <= P.POSE_FLOOR * 1.0000001, "pose_tolerance() is 10 x the measured floor: re-measure POSE_FLOOR"


def test_degenerate_graphs():
    G = P.ring(6, 1, 1, 1)
    G["constant"][:] = 1
    poses, info = P.optimise(G)
    assert info["lm_iterations"] == 0 and np.array_equal(poses, G["poses_init"])
    G = P.ring(6, 1, 1, 0)
    G["edges"], G["weights"], G["measurements"] = np.zeros((0, 2), np.int32), None, None
    poses, info = P.optimise(G)
    assert info["lm_iterations"] == 0 and info["cost_initial"] == 0.0 and np.array_equal(poses, G["poses_init"])


def test_transform_points_moves_by_after_times_before_inverse():
    rng = np.random.default_rng(3)
    before = P.exp(0.3 * rng.standard_normal((4, 7)))
    after = P.mul(before, P.exp(0.1 * rng.standard_normal((4, 7))))
    const = np.array([0, 1, 0, 0], np.uint8)
    ref = np.array([0, 1, -1, 3])
    local = rng.standard_normal((4, 3))
    pos = before[ref, 7:8] * np.einsum("kab,kb->ka", P.quat_R(before[ref, :4]), local) + before[ref, 4:7]
    out, _, depth = P.transform_points(before, after, const, ref, pos, None, np.ones(4))
    want = after[ref, 7:8] * np.einsum("kab,kb->ka", P.quat_R(after[ref, :4]), local) + after[ref, 4:7]
    assert np.abs(out[[0, 3]] - want[[0, 3]]).max() < 1e-12 and np.array_equal(out[[1, 2]], pos[[1, 2]])
    assert np.allclose(depth[[0, 3]], (after[:, 7] / before[:, 7])[[0, 3]], rtol=1e-14) and np.array_equal(depth[[1, 2]], [1.0, 1.0])
