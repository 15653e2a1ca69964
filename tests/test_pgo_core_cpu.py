"""CPU: pgo_core.hpp -- the per-edge statements the kernels run -- built with plain g++ and compared with the numpy restatement on a few
hundred random edges of both kinds: residuals, both Jacobians, the block products and the update agree to <= 1e-12 relative (relative
to the largest entry of the quantity over the batch).  The edges include rotation angles and sigma on both sides of the series thresholds
and at zero."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pgo_numpy as P

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pgo_core") / "pgo_core_driver"
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", f"-I{ROOT / 'snake_slam_amd' / 'csrc'}",
           str(ROOT / "tests" / "cpp" / "pgo_core_driver.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def edges_with_thresholds(sim3, n=300, seed=11):
    """(Ti, Tj, M, w): random poses; the residual tangent of edge e is x[e], whose angle / sigma walk over the thresholds"""
    rng = np.random.default_rng(seed)
    x = 0.1 * rng.standard_normal((n, 7))
    thetas = [0.0, 1e-12, 1e-6, 0.999 * P.TH_THETA, 1.001 * P.TH_THETA, 0.4999 * P.TH_THETA, 0.3]
    sigmas = [0.0, 1e-13, 0.999 * P.TH_SIGMA, 1.001 * P.TH_SIGMA, -1e-5, 0.2]
    for e in range(min(n, 84)):
        d = rng.standard_normal(3)
        x[e, 3:6] = thetas[e % 7] * d / np.linalg.norm(d)
        x[e, 6] = sigmas[(e // 7) % 6]
    if not sim3:
        x[:, 6] = 0.0
    mk = lambda: P.exp(np.concatenate([rng.standard_normal((n, 3)), 0.8 * rng.standard_normal((n, 3)), 0.2 * sim3 * rng.standard_normal((n, 1))], -1))
    Ti, Tj = mk(), mk()
    M = P.mul(P.mul(P.inv(Ti), Tj), P.inv(P.exp(x)))
    return Ti, Tj, M, 0.5 + rng.random(n)


@pytest.mark.parametrize("sim3", [False, True], ids=["se3", "sim3"])
def test_cpu_build_of_the_core_equals_the_restatement(driver, tmp_path, sim3):
    Ti, Tj, M, w = edges_with_thresholds(sim3)
    n, D = len(w), 7 if sim3 else 6
    for name, a in (("Ti", Ti), ("Tj", Tj), ("M", M), ("w", w), ("params", np.array([float(n), float(D)]))):
        np.ascontiguousarray(a, np.float64).tofile(tmp_path / f"{name}.bin")
    r = subprocess.run([str(driver), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = {k: np.fromfile(tmp_path / f"out_{k}.bin", np.float64) for k in ("r", "Ji", "Jj", "Hii", "Hij", "Hjj", "gi", "gj", "retract")}
    poses = np.concatenate([Ti, Tj])
    edges = np.stack([np.arange(n), np.arange(n) + n], -1)
    rr, Ji, Jj = P.edge_terms(poses, edges, w, M, not sim3)
    T = lambda A: np.swapaxes(A, 1, 2)
    want = dict(r=rr, Ji=Ji, Jj=Jj, Hii=T(Ji) @ Ji, Hij=T(Ji) @ Jj, Hjj=T(Jj) @ Jj, gi=np.einsum("eka,ek->ea", Ji, rr),
                gj=np.einsum("eka,ek->ea", Jj, rr), retract=P.retract(Ti, rr))
    for k, v in want.items():
        rel = np.abs(got[k] - v.ravel()).max() / np.abs(v).max()
        print(f"{k}: {rel:.2e}")
        assert rel <= 1e-12, k
