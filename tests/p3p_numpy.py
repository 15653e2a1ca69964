"""Numpy restatement of "snk-p3p v1" (DESIGN.md section 3d): the sampler, the minimal solver, the scoring and the winner rule of
the P3P-RANSAC step of Tracking::TrackBruteForce (reference Snake/Tracking/TrackingCoarse.cpp:403-440), written from the text and
vectorised over the hypotheses.  The solver repeats the statements of snake_slam_amd/csrc/p3p_core.hpp in the same order (every
operation is an IEEE + - * / or sqrt); the per-point test is written with separate products and sums where the kernel uses fma(),
which is what the borderline band below is for.

Also here: the case generators of the tests, the three borderline marks and `pose_tolerance()`.
"""
from __future__ import annotations

import numpy as np

SLOTS = 4
CUBIC_STEPS = 100
NEWTON_STEPS = 3
DRAW_LIMIT = 32
BORDERLINE = 1e-6   # g: relative band on the threshold (the value tri_numpy.BORDERLINE uses)
BORDERLINE_CAP = 0.02  # share of a case's hypotheses that may be borderline (the issue's figure; tests assert half of it here)
M32 = 0xFFFFFFFF


# ------------------------------------------------------------------ sampling ------------
def mix(x):
    x = np.asarray(x, np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    x = x ^ (x >> np.uint64(16))
    return x


def problem_key(seed: int, problem: int):
    h = mix((seed & M32) ^ 0x9E3779B9)
    h = mix(int(h) ^ ((seed >> 32) & M32))
    return int(mix(int(h) ^ (problem & M32)))


def draw_index(key, k, c, n):
    h = mix(mix(np.uint64(key) ^ np.asarray(k, np.uint64)) ^ np.asarray(c, np.uint64))
    return ((h * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def triplets(seed: int, problem: int, iterations: int, n: int) -> np.ndarray:
    """[iterations, 3] distinct indices in [0, n), n >= 4."""
    key = problem_key(seed, problem)
    k = np.arange(iterations, dtype=np.uint64)
    c = np.zeros(iterations, np.uint64)
    i0 = draw_index(key, k, c, n)
    c += 1
    i1 = draw_index(key, k, c, n)
    c += 1
    while True:
        again = (i1 == i0) & (c < DRAW_LIMIT)
        if not again.any():
            break
        i1 = np.where(again, draw_index(key, k, c, n), i1)
        c = c + again.astype(np.uint64)
    i1 = np.where(i1 == i0, (i0 + 1) % n, i1)
    i2 = draw_index(key, k, c, n)
    c += 1
    while True:
        again = ((i2 == i0) | (i2 == i1)) & (c < DRAW_LIMIT)
        if not again.any():
            break
        i2 = np.where(again, draw_index(key, k, c, n), i2)
        c = c + again.astype(np.uint64)
    while True:
        again = (i2 == i0) | (i2 == i1)
        if not again.any():
            break
        i2 = np.where(again, (i2 + 1) % n, i2)
    return np.stack([i0, i1, i2], 1).astype(np.int32)


# ------------------------------------------------------------------ the minimal solver ------------
def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _det_cols(A, B, pick):
    c = [[(B[i][j] if (pick >> j) & 1 else A[i][j]) for i in range(3)] for j in range(3)]
    return _dot(c[0], _cross(c[1], c[2]))


def _sel3(i, a0, a1, a2):
    return np.where(i == 0, a0, np.where(i == 1, a1, a2))


def _pos_finite(x):
    return (x > 0.0) & (x < np.inf)


def solve(X, uv, detail=False):
    """X [K, 3, 3] world points, uv [K, 3, 2] normalised image points of K triplets.
    Returns R [K, 4, 9], t [K, 4, 3], valid [K, 4] bool (slot = 2 * line + root).  With detail: also a dict of the quantities the
    conditioning measure reads."""
    X = np.asarray(X, np.float64)
    uv = np.asarray(uv, np.float64)
    K = len(X)
    with np.errstate(all="ignore"):
        y = []
        for i in range(3):
            nrm = np.sqrt((uv[:, i, 0] * uv[:, i, 0] + uv[:, i, 1] * uv[:, i, 1]) + 1.0)
            y.append([uv[:, i, 0] / nrm, uv[:, i, 1] / nrm, 1.0 / nrm])
        b12, b13, b23 = _dot(y[0], y[1]), _dot(y[0], y[2]), _dot(y[1], y[2])
        X0 = [X[:, 0, j] for j in range(3)]
        d1 = [X[:, 1, j] - X[:, 0, j] for j in range(3)]
        d2 = [X[:, 2, j] - X[:, 0, j] for j in range(3)]
        d12 = [X[:, 2, j] - X[:, 1, j] for j in range(3)]
        a12, a13, a23 = _dot(d1, d1), _dot(d2, d2), _dot(d12, d12)
        cx = _cross(d1, d2)
        det = _dot(cx, cx)
        alive = (a12 > 0.0) & (a13 > 0.0) & (a23 > 0.0)
        alive &= det > 1e-18 * (a12 * a13)
        z = np.zeros(K)
        D1 = [[a23, -(a23 * b12), z], [-(a23 * b12), a23 - a12, a12 * b23], [z, a12 * b23, -a12]]
        D2 = [[a23, z, -(a23 * b13)], [z, -a13, a13 * b23], [-(a23 * b13), a13 * b23, a23 - a13]]
        c0 = _det_cols(D1, D2, 0)
        c1 = (_det_cols(D1, D2, 1) + _det_cols(D1, D2, 2)) + _det_cols(D1, D2, 4)
        c2 = (_det_cols(D1, D2, 6) + _det_cols(D1, D2, 5)) + _det_cols(D1, D2, 3)
        c3 = _det_cols(D1, D2, 7)
        swap = np.abs(c3) < np.abs(c0)
        D1, D2 = ([[np.where(swap, D2[i][j], D1[i][j]) for j in range(3)] for i in range(3)],
                  [[np.where(swap, D1[i][j], D2[i][j]) for j in range(3)] for i in range(3)])
        c0, c3 = np.where(swap, c3, c0), np.where(swap, c0, c3)
        c1, c2 = np.where(swap, c2, c1), np.where(swap, c1, c2)
        alive &= np.abs(c3) > 0.0
        pb, pc, pd = c2 / c3, c1 / c3, c0 / c3
        bound = 1.0 + np.fmax(np.abs(pb), np.fmax(np.abs(pc), np.abs(pd)))
        lo, hi, g = -bound, bound.copy(), -pb / 3.0
        run = np.ones(K, bool)
        df_last = np.full(K, np.nan)
        for _ in range(CUBIC_STEPS):
            f = ((g + pb) * g + pc) * g + pd
            up = f > 0.0
            hi = np.where(run & up, g, hi)
            lo = np.where(run & ~up, g, lo)
            df = (3.0 * g + 2.0 * pb) * g + pc
            df_last = np.where(run, df, df_last)
            gn = g - f / df
            gn = np.where((gn > lo) & (gn < hi), gn, 0.5 * (lo + hi))
            run &= gn != g
            g = np.where(run, gn, g)
            if not run.any():
                break
        use2 = np.abs(g) <= 1.0
        D0 = [[D1[i][j] + g * D2[i][j] for j in range(3)] for i in range(3)]
        Q = [[np.where(use2, D2[i][j], D1[i][j]) for j in range(3)] for i in range(3)]
        B = [[None] * 3 for _ in range(3)]
        B[0][0] = -(D0[1][1] * D0[2][2] - D0[1][2] * D0[1][2])
        B[0][1] = -(D0[0][2] * D0[1][2] - D0[0][1] * D0[2][2])
        B[0][2] = -(D0[0][1] * D0[1][2] - D0[0][2] * D0[1][1])
        B[1][1] = -(D0[0][0] * D0[2][2] - D0[0][2] * D0[0][2])
        B[1][2] = -(D0[0][1] * D0[0][2] - D0[0][0] * D0[1][2])
        B[2][2] = -(D0[0][0] * D0[1][1] - D0[0][1] * D0[0][1])
        B[1][0], B[2][0], B[2][1] = B[0][1], B[0][2], B[1][2]
        bi = np.zeros(K, np.int64)
        bmax = B[0][0].copy()
        for i in (1, 2):
            up = B[i][i] > bmax
            bmax = np.where(up, B[i][i], bmax)
            bi = np.where(up, i, bi)
        alive &= bmax > 0.0
        beta = np.sqrt(bmax)
        p = [_sel3(bi, B[0][j], B[1][j], B[2][j]) / beta for j in range(3)]
        N = [[D0[0][0], D0[0][1] - p[2], D0[0][2] + p[1]],
             [D0[1][0] + p[2], D0[1][1], D0[1][2] - p[0]],
             [D0[2][0] - p[1], D0[2][1] + p[0], D0[2][2]]]
        br, bc, nmax = np.zeros(K, np.int64), np.zeros(K, np.int64), np.full(K, -1.0)
        for i in range(3):
            for j in range(3):
                v = np.abs(N[i][j])
                up = v > nmax
                nmax = np.where(up, v, nmax)
                br = np.where(up, i, br)
                bc = np.where(up, j, bc)
        alive &= nmax > 0.0
        line = [[_sel3(br, N[0][j], N[1][j], N[2][j]) for j in range(3)], [_sel3(bc, N[j][0], N[j][1], N[j][2]) for j in range(3)]]
        r1, r2 = _cross(d2, cx), _cross(cx, d1)
        r1 = [r1[j] / det for j in range(3)]
        r2 = [r2[j] / det for j in range(3)]
        r3 = [cx[j] / det for j in range(3)]
        asum = (a12 + a13) + a23
        R = np.zeros((K, SLOTS, 9))
        t = np.zeros((K, SLOTS, 3))
        valid = np.zeros((K, SLOTS), bool)
        disc_rel = np.full((K, 2), np.inf)
        for l in range(2):
            w0, w1, w2 = line[l]
            ia = np.zeros(K, np.int64)
            wm = np.abs(w0)
            for i, w in ((1, w1), (2, w2)):
                up = np.abs(w) > wm
                wm = np.where(up, np.abs(w), wm)
                ia = np.where(up, i, ia)
            ib = np.where(ia == 2, 0, ia + 1)
            ic = np.where(ia == 0, 2, ia - 1)
            wa = _sel3(ia, w0, w1, w2)
            sb = -_sel3(ib, w0, w1, w2) / wa
            sc = -_sel3(ic, w0, w1, w2) / wa
            gv = [np.where(ia == j, sb, np.where(ib == j, 1.0, 0.0)) for j in range(3)]
            hv = [np.where(ia == j, sc, np.where(ic == j, 1.0, 0.0)) for j in range(3)]
            Qg = [_dot(Q[i], gv) for i in range(3)]
            Qh = [_dot(Q[i], hv) for i in range(3)]
            qa, qb, qc = _dot(gv, Qg), _dot(gv, Qh), _dot(hv, Qh)
            disc = qb * qb - qa * qc
            disc_rel[:, l] = np.abs(disc) / (qb * qb + np.abs(qa * qc) + 1e-300)
            ok_l = alive & (disc >= 0.0)
            sq = np.sqrt(disc)
            qq = -(qb + np.where(qb >= 0.0, sq, -sq))
            for r in range(2):
                s = 2 * l + r
                tau = qq / qa if r == 0 else qc / qq
                ok = ok_l & _pos_finite(tau)
                lam = [tau * gv[j] + hv[j] for j in range(3)]
                ok &= (lam[0] > 0.0) & (lam[1] > 0.0) & (lam[2] > 0.0)
                den = 2.0 * _dot(lam, lam) - 2.0 * ((b12 * (lam[0] * lam[1]) + b13 * (lam[0] * lam[2])) + b23 * (lam[1] * lam[2]))
                ok &= den > 0.0
                rho = np.sqrt(asum / den)
                lam = [rho * lam[j] for j in range(3)]
                going = np.ones(K, bool)
                for _ in range(NEWTON_STEPS):
                    l0, l1, l2 = lam
                    e12 = ((l0 * l0 + l1 * l1) - 2.0 * b12 * (l0 * l1)) - a12
                    e13 = ((l0 * l0 + l2 * l2) - 2.0 * b13 * (l0 * l2)) - a13
                    e23 = ((l1 * l1 + l2 * l2) - 2.0 * b23 * (l1 * l2)) - a23
                    j00, j01 = 2.0 * (l0 - b12 * l1), 2.0 * (l1 - b12 * l0)
                    j10, j12 = 2.0 * (l0 - b13 * l2), 2.0 * (l2 - b13 * l0)
                    j21, j22 = 2.0 * (l1 - b23 * l2), 2.0 * (l2 - b23 * l1)
                    dj = -(j00 * (j12 * j21)) - j01 * (j10 * j22)
                    going &= np.abs(dj) > 0.0
                    x0 = (-(j12 * j21) * e12 - (j01 * j22) * e13) + (j01 * j12) * e23
                    x1 = (-(j10 * j22) * e12 + (j00 * j22) * e13) - (j00 * j12) * e23
                    x2 = ((j10 * j21) * e12 - (j00 * j21) * e13) - (j01 * j10) * e23
                    lam = [np.where(going, l0 - x0 / dj, l0), np.where(going, l1 - x1 / dj, l1), np.where(going, l2 - x2 / dj, l2)]
                ok &= _pos_finite(lam[0]) & _pos_finite(lam[1]) & _pos_finite(lam[2])
                Y0 = [lam[0] * y[0][j] for j in range(3)]
                e1 = [lam[1] * y[1][j] - Y0[j] for j in range(3)]
                e2 = [lam[2] * y[2][j] - Y0[j] for j in range(3)]
                e3 = _cross(e1, e2)
                for i in range(3):
                    for j in range(3):
                        R[:, s, 3 * i + j] = (e1[i] * r1[j] + e2[i] * r2[j]) + e3[i] * r3[j]
                    t[:, s, i] = Y0[i] - ((R[:, s, 3 * i] * X0[0] + R[:, s, 3 * i + 1] * X0[1]) + R[:, s, 3 * i + 2] * X0[2])
                valid[:, s] = ok
        R[~valid] = 0.0
        t[~valid] = 0.0
        if not detail:
            return R, t, valid
        # what the conditioning measure reads: how flat the world triangle is, how close the bearings are, how close each quadratic
        # is to a double root, and the slope of the cubic at the root it stopped on (relative to the size of its terms)
        flat = det / (a12 * a13)
        cubic = np.abs(df_last) / (3.0 * g * g + np.abs(2.0 * pb * g) + np.abs(pc) + 1e-300)
        return R, t, valid, dict(flat=flat, cosines=np.stack([b12, b13, b23], 1), disc_rel=disc_rel, cubic=cubic, alive=alive)


def pose7(R, t):
    """(R [9], t [3]) -> qx qy qz qw tx ty tz as p3p_pose7 does."""
    R = np.asarray(R, np.float64)
    tr = (R[0] + R[4]) + R[8]
    if tr > 0.0:
        s = 2.0 * np.sqrt(tr + 1.0)
        w, x, y, z = 0.25 * s, (R[7] - R[5]) / s, (R[2] - R[6]) / s, (R[3] - R[1]) / s
    elif R[0] > R[4] and R[0] > R[8]:
        s = 2.0 * np.sqrt(((1.0 + R[0]) - R[4]) - R[8])
        w, x, y, z = (R[7] - R[5]) / s, 0.25 * s, (R[1] + R[3]) / s, (R[2] + R[6]) / s
    elif R[4] > R[8]:
        s = 2.0 * np.sqrt(((1.0 + R[4]) - R[0]) - R[8])
        w, x, y, z = (R[2] - R[6]) / s, (R[1] + R[3]) / s, 0.25 * s, (R[5] + R[7]) / s
    else:
        s = 2.0 * np.sqrt(((1.0 + R[8]) - R[0]) - R[4])
        w, x, y, z = (R[3] - R[1]) / s, (R[2] + R[6]) / s, (R[5] + R[7]) / s, 0.25 * s
    nq = np.sqrt(((x * x + y * y) + z * z) + w * w)
    sg = -nq if w < 0.0 else nq
    return np.array([x / sg, y / sg, z / sg, w / sg, t[0], t[1], t[2]])


def quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


# ------------------------------------------------------------------ scoring and the winner ------------
def inlier_mask(R, t, wps, nips, threshold):
    """R [..., 9], t [..., 3] -> bool [..., n]: z_c > 0 and (x - u z)^2 + (y - v z)^2 < threshold z^2."""
    R = np.asarray(R, np.float64)
    t = np.asarray(t, np.float64)
    Xw, Yw, Zw = wps[:, 0], wps[:, 1], wps[:, 2]
    r = lambda j: R[..., j, None]  # noqa: E731
    x = r(0) * Xw + r(1) * Yw + r(2) * Zw + t[..., 0, None]
    y = r(3) * Xw + r(4) * Yw + r(5) * Zw + t[..., 1, None]
    z = r(6) * Xw + r(7) * Yw + r(8) * Zw + t[..., 2, None]
    ex, ey = x - nips[:, 0] * z, y - nips[:, 1] * z
    return (z > 0.0) & (ex * ex + ey * ey < threshold * (z * z))


def hypotheses(wps, nips, iterations, threshold, seed, problem=0):
    """Everything snk_p3p_debug_hypotheses lays open, plus the borderline marks.  Returns a dict:
    triplets [K, 3], R [K, 4, 9], t [K, 4, 3], valid [K, 4], counts / counts_lo / counts_hi [K, 4] (threshold, threshold (1 - g),
    threshold (1 + g); -1 in empty slots), borderline [K] bool."""
    wps = np.ascontiguousarray(wps, np.float64).reshape(-1, 3)
    nips = np.ascontiguousarray(nips, np.float64).reshape(-1, 2)
    n = len(wps)
    tri = triplets(seed, problem, iterations, n)
    X, uv = wps[tri], nips[tri]
    R, t, valid, det = solve(X, uv, detail=True)
    cnt = {}
    for name, th in (("counts", threshold), ("counts_lo", threshold * (1.0 - BORDERLINE)), ("counts_hi", threshold * (1.0 + BORDERLINE))):
        c = inlier_mask(R, t, wps, nips, th).sum(-1)
        cnt[name] = np.where(valid, c, -1).astype(np.int64)
    border = (cnt["counts_lo"] != cnt["counts_hi"]).any(1)
    border |= ill_conditioned(det)
    # the second f64 formulation: the same triplet with its points rotated by one place
    _, _, valid2 = solve(X[:, [1, 2, 0]], uv[:, [1, 2, 0]])
    border |= valid.sum(1) != valid2.sum(1)
    return dict(triplets=tri, R=R, t=t, valid=valid, borderline=border, detail=det, **cnt)


# conditioning thresholds, chosen from the geometry and the number format, not from any device result: a world triangle whose
# sin^2 of an angle is below 1e-6 (points within 1e-3 rad of a line), a quadratic or the cubic within 1e-6 (relative) of a double
# root -- sqrt(1e-6) = 1e-3 relative movement of the roots per 1e-6 relative perturbation of the coefficients is where
# a root-discard branch can move under roundings that are amplified by the earlier steps
FLAT_MIN = 1e-6
DOUBLE_ROOT_MIN = 1e-6


def ill_conditioned(det):
    with np.errstate(all="ignore"):
        bad = ~(det["flat"] > FLAT_MIN)
        bad |= ~(det["disc_rel"] > DOUBLE_ROOT_MIN).all(1)
        bad |= ~(det["cubic"] > DOUBLE_ROOT_MIN)
    return bad & det["alive"]


def ransac(wps, nips, iterations, threshold, seed, problem=0, pose=None):
    """The whole call: returns a dict with pose [7], inliers, mask [n] uint8, matches (ascending), best (k, solution) and `hyp`
    (the dict of hypotheses(), None for n < 4)."""
    wps = np.ascontiguousarray(wps, np.float64).reshape(-1, 3)
    nips = np.ascontiguousarray(nips, np.float64).reshape(-1, 2)
    n = len(wps)
    pose = np.array([0, 0, 0, 1.0, 0, 0, 0]) if pose is None else np.asarray(pose, np.float64).copy()
    none = dict(pose=pose, inliers=0, mask=np.zeros(n, np.uint8), matches=np.zeros(0, np.int32), best=(-1, -1), hyp=None)
    if n < 4 or iterations == 0:
        return none
    H = hypotheses(wps, nips, iterations, threshold, seed, problem)
    c = H["counts"]
    if c.max() <= 0:
        return dict(none, hyp=H)
    # largest count; ties to the smaller k, then the smaller slot: the first maximum in row-major order
    k, s = np.unravel_index(np.argmax(c), c.shape)
    mask = inlier_mask(H["R"][k, s], H["t"][k, s], wps, nips, threshold)
    sol = int(H["valid"][k, :s].sum())
    return dict(pose=pose7(H["R"][k, s], H["t"][k, s]), inliers=int(mask.sum()), mask=mask.astype(np.uint8),
                matches=np.nonzero(mask)[0].astype(np.int32), best=(int(k), sol), slot=int(s), hyp=H)


# ------------------------------------------------------------------ Gauss-Newton polish and the tolerance ------------
def polish(R, t, X, uv, steps=5):
    """Gauss-Newton on the six residuals of the pose's own three points in the normalised plane (left-multiplied se(3) update)."""
    R = np.asarray(R, np.float64).reshape(3, 3).copy()
    t = np.asarray(t, np.float64).copy()
    for _ in range(steps):
        J, r = np.zeros((6, 6)), np.zeros(6)
        for i in range(3):
            p = R @ X[i] + t
            iz = 1.0 / p[2]
            r[2 * i: 2 * i + 2] = [p[0] * iz - uv[i, 0], p[1] * iz - uv[i, 1]]
            dp = np.array([[iz, 0, -p[0] * iz * iz], [0, iz, -p[1] * iz * iz]])
            px = np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])
            J[2 * i: 2 * i + 2] = dp @ np.hstack([-px, np.eye(3)])
        try:
            d = np.linalg.solve(J, -r)
        except np.linalg.LinAlgError:
            break
        w, v = d[:3], d[3:]
        th = np.linalg.norm(w)
        Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        dR = np.eye(3) + Kx + 0.5 * Kx @ Kx if th < 1e-8 else np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th**2 * Kx @ Kx
        R, t = dR @ R, dR @ t + v
    return R, t


def pose_distance(Ra, ta, Rb, tb):
    """Largest entry of R_a - R_b, and |t_a - t_b| relative to max(1, |t|): the figure pose_tolerance() bounds."""
    Ra, Rb = np.asarray(Ra).reshape(3, 3), np.asarray(Rb).reshape(3, 3)
    return max(float(np.abs(Ra - Rb).max()), float(np.linalg.norm(ta - tb) / max(1.0, np.linalg.norm(tb))))


def measure_pose_floor(cases=None):
    """The largest disagreement between the closed form and its Gauss-Newton polish over every solution of every hypothesis that is
    not borderline, over the given cases (default: every case of gpu_cases())."""
    worst = 0.0
    for c in cases if cases is not None else gpu_cases():
        H = hypotheses(c["wps"], c["nips"], c["iterations"], c["threshold"], c["seed"])
        tri = H["triplets"]
        for k in np.nonzero(~H["borderline"])[0]:
            for s in np.nonzero(H["valid"][k])[0]:
                Rp, tp = polish(H["R"][k, s], H["t"][k, s], c["wps"][tri[k]], c["nips"][tri[k]])
                worst = max(worst, pose_distance(H["R"][k, s], H["t"][k, s], Rp, tp))
    return worst


# measured by tests/test_p3p_numpy.py::test_pose_tolerance_is_the_measured_floor on the cases of gpu_cases(): see its docstring
POSE_FLOOR = 2.0e-12


def pose_tolerance() -> float:
    """10 x the measured floor between the closed form and its polish (relative to max(1, |t|))."""
    return 10.0 * POSE_FLOOR


# ------------------------------------------------------------------ cases ------------
FX, FY, CX, CY = 458.654, 457.296, 367.215, 248.375
THRESHOLD = (2 * 2.1 / FX) ** 2  # TrackingCoarse.cpp:412-413 with reprojectionErrorThresholdMono = 2.1


def random_pose(rng, angle=0.3, shift=1.0):
    w = rng.normal(size=3)
    w *= rng.uniform(0, angle) / np.linalg.norm(w)
    q = np.concatenate([np.sin(np.linalg.norm(w) / 2) * w / np.linalg.norm(w), [np.cos(np.linalg.norm(w) / 2)]])
    return np.concatenate([q, rng.uniform(-shift, shift, 3)])


def make_case(n, outlier_share, noise_px, seed, iterations=250):
    """n pairs seen by a camera at a random pose: stereo-like depths 0.5 .. 40 m over a 752 x 480 image, keypoint noise in
    pixels, a share of pairs whose image point is replaced by a random one (a wrong brute-force match)."""
    rng = np.random.default_rng(seed)
    pose = random_pose(rng)
    R, t = quat_to_R(pose[:4]), pose[4:]
    px = np.stack([rng.uniform(0, 752, n), rng.uniform(0, 480, n)], 1)
    depth = np.exp(rng.uniform(np.log(0.5), np.log(40.0), n))
    pc = np.stack([(px[:, 0] - CX) / FX * depth, (px[:, 1] - CY) / FY * depth, depth], 1)
    wps = (pc - t) @ R  # R^T (p_c - t)
    obs = px + noise_px * rng.normal(size=(n, 2))
    n_out = int(round(outlier_share * n))
    outl = np.zeros(n, bool)
    if n_out:
        outl[rng.choice(n, n_out, replace=False)] = True
        obs[outl] = np.stack([rng.uniform(0, 752, n_out), rng.uniform(0, 480, n_out)], 1)
    nips = np.stack([(obs[:, 0] - CX) / FX, (obs[:, 1] - CY) / FY], 1)
    return dict(name=f"n{n}_o{int(outlier_share * 100)}_px{noise_px}", wps=np.ascontiguousarray(wps), nips=np.ascontiguousarray(nips),
                pose=pose, outlier=outl, noise_px=noise_px, outlier_share=outlier_share, iterations=iterations, threshold=THRESHOLD,
                seed=0x5EED0000 + seed, px=obs)


def gpu_cases():
    """n in {4, 30, 200, 1000} x outlier share {0, 30, 60 %} x keypoint noise {0, 1 px}."""
    out = []
    for a, n in enumerate((4, 30, 200, 1000)):
        for b, share in enumerate((0.0, 0.3, 0.6)):
            for c, noise in enumerate((0.0, 1.0)):
                out.append(make_case(n, share, noise, 1000 + 100 * a + 10 * b + c))
    return out


# ------------------------------------------------------------------ edge cases ------------
# the numbers of snake_slam_amd/csrc/p3p.hip the table below is built on (tests/test_p3p_numpy.py::test_pinned_limits_of_the_kernel
# reads them from the source): pairs per problem, iterations per call, hypotheses per pass of the kernel's loop, bytes of LDS a pair and
# per launch, and what a launch may ask for before the kernel's limit has to be raised
MAX_PAIRS = 3072
MAX_ITERATIONS = 1 << 20
GROUP = 256
LDS_BYTES_PER_PAIR, LDS_BYTES_FIXED = 44, 8
LDS_DEFAULT_LIMIT = 65536


def winner_is_exact(want) -> bool:
    """True where the restatement decides the winner beyond rounding: it has one, the winning hypothesis is not borderline, and no
    borderline hypothesis comes within its own count spread of the best count."""
    H = want["hyp"]
    kb = want["best"][0]
    if H is None or kb < 0 or H["borderline"][kb]:
        return False
    top = H["counts"].max(1)
    spread = (H["counts_hi"] - H["counts_lo"]).max(1)
    return all(top[kb] - top[h] > spread[h] for h in np.nonzero(H["borderline"])[0])


def groups_at_best(want):
    """The groups of GROUP hypotheses (k // GROUP) that hold a hypothesis with the best count."""
    top = want["hyp"]["counts"].max(1)
    return sorted({int(k) // GROUP for k in np.nonzero(top == top.max())[0]})


# property name -> what the restatement's run `r` of case `c` has to show, beyond a borderline share of at most half the cap
EDGE_PROPERTIES = {
    # nothing more: the shape is the point
    "shape": lambda c, r: True,
    # every hypothesis reaches n, so every lane of every group ties and the first hypothesis has to win
    "all_tie": lambda c, r: bool((r["hyp"]["counts"].max(1) == len(c["wps"])).all()) and r["best"][0] == 0 and winner_is_exact(r),
    # the winner lies beyond the first group / in the last group of 1024 iterations
    "late": lambda c, r: r["best"][0] >= GROUP and winner_is_exact(r),
    "last_group": lambda c, r: r["best"][0] >= 3 * GROUP and winner_is_exact(r),
    # the best count is reached in two different groups, the first of them not group 0: the running best has to keep the earlier one
    "cross_tie": lambda c, r: len(groups_at_best(r)) >= 2 and r["best"][0] >= GROUP and winner_is_exact(r),
}


def edge_grid():
    """(n, wrong share, noise in px, iterations, property) of the edge cases: the strides of the scoring loop (64) and of the mask / list
    compaction (256) with one, two and three groups of hypotheses, winners and ties beyond the first group, either side of the 64 KB
    of LDS a launch gets without asking (1489 / 1490 pairs), and the maximum."""
    out = [(n, 0.0, 0.0, 2 * GROUP + 1, "all_tie") for n in (63, 64, 65)]
    out += [(255, 0.3, 1.0, GROUP, "shape"), (256, 0.3, 1.0, GROUP + 1, "shape"), (257, 0.3, 1.0, 2 * GROUP, "shape")]
    out += [(200, 0.9, 0.0, 4 * GROUP, "late"), (65, 0.9, 0.0, 4 * GROUP, "last_group"), (257, 0.9, 0.0, 4 * GROUP, "cross_tie")]
    out += [(1489, 0.3, 1.0, GROUP + 1, "shape"), (1490, 0.3, 1.0, GROUP + 1, "shape")]
    out += [(MAX_PAIRS, 0.3, 1.0, 600, "shape"), (MAX_PAIRS, 0.0, 0.0, 300, "all_tie")]
    return out


def edge_ok(c, prop, r=None):
    r = r if r is not None else ransac(c["wps"], c["nips"], c["iterations"], c["threshold"], c["seed"])
    return float(r["hyp"]["borderline"].mean()) <= 0.5 * BORDERLINE_CAP and bool(EDGE_PROPERTIES[prop](c, r))


def make_edge_case(g, seed):
    n, share, noise, iterations, prop = g
    c = make_case(n, share, noise, seed, iterations)
    c["name"] += f"_it{iterations}_{prop}"
    c["property"] = prop
    return c


def first_edge_seed(j, g, limit=200):
    """The first generator seed of 5000 + 100 j + 0, 1, 2, ... whose case satisfies the property of entry j of edge_grid()."""
    return next(5000 + 100 * j + o for o in range(limit) if edge_ok(make_edge_case(g, 5000 + 100 * j + o), g[4]))


# the generator seed of every entry of edge_grid(), found by first_edge_seed on the CPU
# (tests/test_p3p_numpy.py::test_edge_seeds_are_the_first_that_qualify fails when this table is stale)
EDGE_SEEDS = [5000 + 100 * j + o for j, o in enumerate([1, 0, 1, 0, 0, 0, 0, 3, 6, 0, 0, 0, 0])]


def edge_cases():
    return [make_edge_case(g, seed) for g, seed in zip(edge_grid(), EDGE_SEEDS)]


# ------------------------------------------------------------------ the comparison of the GPU tests ------------
def device_pose_distance(p7, R, t):
    return pose_distance(quat_to_R(p7[:4]), p7[4:], R, t)


def check_device_against_restatement(c, want, res, tri, ns, poses, cnt):
    """What tests/test_p3p_gpu.py and tests/test_p3p_edges_gpu.py assert of one snk_p3p_debug_hypotheses call (`res, tri, ns, poses,
    cnt` as P3PRansac.debug_hypotheses returns them) on case `c`, against `want` = ransac() of the same case: triplets equal; solution
    counts and inlier counts equal on the hypotheses that are not borderline, poses within pose_tolerance(); winner, mask and ascending
    list exact where winner_is_exact(want); the mask consistent with the returned pose; ground truth on the noise-free cases."""
    H = want["hyp"]
    assert np.array_equal(tri, H["triplets"])
    border = H["borderline"]
    print(f"{c['name']}: borderline share {border.mean():.4f}")
    assert border.mean() <= BORDERLINE_CAP
    ok = ~border
    assert np.array_equal(ns[ok], H["valid"].sum(1)[ok])
    worst = 0.0
    for k in np.nonzero(ok)[0]:
        slots = np.nonzero(H["valid"][k])[0]
        for j, s in enumerate(slots):
            worst = max(worst, device_pose_distance(poses[k, j], H["R"][k, s], H["t"][k, s]))
            assert cnt[k, j] == H["counts"][k, s], (int(k), j, cnt[k].tolist(), H["counts"][k].tolist())
    print(f"{c['name']}: largest pose difference to the restatement {worst:.2e}")
    assert worst <= pose_tolerance()
    # the winner
    assert res["inliers"] == int(res["mask"].sum()) == len(res["matches"])
    assert np.array_equal(np.nonzero(res["mask"])[0], res["matches"])
    kb, sb = want["best"]
    if winner_is_exact(want):
        assert res["best"] == want["best"] and res["inliers"] == want["inliers"]
        assert np.array_equal(res["mask"], want["mask"]) and np.array_equal(res["matches"], want["matches"])
        assert device_pose_distance(res["pose"], H["R"][kb, want["slot"]], H["t"][kb, want["slot"]]) <= pose_tolerance()
    elif kb >= 0:
        assert res["inliers"] >= H["counts_lo"][kb, want["slot"]]
    if res["best"][0] >= 0:
        Rg, tg = quat_to_R(res["pose"][:4]).reshape(9), res["pose"][4:]
        lo = inlier_mask(Rg, tg, c["wps"], c["nips"], c["threshold"] * (1 - BORDERLINE))
        hi = inlier_mask(Rg, tg, c["wps"], c["nips"], c["threshold"] * (1 + BORDERLINE))
        m = res["mask"].astype(bool)
        assert (m[lo]).all() and not (m[~hi]).any()
    true_inl = ~c["outlier"]
    if c["noise_px"] == 0.0 and true_inl.sum() >= 4:
        assert res["mask"][true_inl].all()
        assert device_pose_distance(res["pose"], quat_to_R(c["pose"][:4]), c["pose"][4:]) <= pose_tolerance()
