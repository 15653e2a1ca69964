"""numpy restatement of "snk-pgo v1" (DESIGN.md section 3f): pose-graph optimisation over SE3 / Sim3 vertices.

Poses are rows of 8 doubles ``qx qy qz qw tx ty tz s`` acting as ``x -> s R x + t``.  Tangent vectors are 7 wide, translation
first, then rotation, then sigma = log s; the se3 form uses the first 6 entries and s = 1.  Every function works on a batch (leading
axes) so that the graphs of the GPU tests are linearised in one pass.  The linear solve is scipy's sparse direct solver; everything
else is the text the device runs: the same branches, thresholds and series orders as pgo_core.hpp.
"""
import numpy as np

TH_THETA = 1e-2   # below: series in theta for W's coefficients, the quaternion of exp and the angle of log
TH_SIGMA = 1e-8   # below: (e^sigma - 1) / sigma = 1 + sigma / 2
G_TERMS = 30      # terms of g_n(sigma) = int_0^1 tau^n e^(tau sigma) dtau = sum_k sigma^k / (k! (n + k + 1))
BERNOULLI_ORDER = 10
# B_n / n!, n = 0..10 (B_1 = -1/2)
JR_COEFF = [1.0, -0.5, 1.0 / 12.0, 0.0, -1.0 / 720.0, 0.0, 1.0 / 30240.0, 0.0, -1.0 / 1209600.0, 0.0, 1.0 / 47900160.0]
LAMBDA_INIT, MAX_ITERATIONS, MIN_CHI2_DELTA = 1e-4, 50, 1e-10


# ---- quaternions and similarity transforms ----
def qmul(a, b):
    ax, ay, az, aw = np.moveaxis(a, -1, 0)
    bx, by, bz, bw = np.moveaxis(b, -1, 0)
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], -1)


def quat_R(q):
    x, y, z, w = np.moveaxis(q, -1, 0)
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)
    return R.reshape(q.shape[:-1] + (3, 3))


def mul(A, B):
    """A . B"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    R = quat_R(A[..., :4])
    t = A[..., 7:8] * np.einsum("...ab,...b->...a", R, B[..., 4:7]) + A[..., 4:7]
    return np.concatenate([qmul(A[..., :4], B[..., :4]), t, A[..., 7:8] * B[..., 7:8]], -1)


def inv(A):
    A = np.asarray(A, np.float64)
    qi = A[..., :4] * np.array([-1.0, -1.0, -1.0, 1.0])
    si = 1.0 / A[..., 7:8]
    t = -si * np.einsum("...ab,...b->...a", quat_R(qi), A[..., 4:7])
    return np.concatenate([qi, t, si], -1)


def skew(v):
    x, y, z = np.moveaxis(v, -1, 0)
    o = np.zeros_like(x)
    return np.stack([o, -z, y, z, o, -x, -y, x, o], -1).reshape(v.shape[:-1] + (3, 3))


def _g(n, sigma):
    s, term, fact = np.zeros_like(sigma), np.ones_like(sigma), 1.0
    for k in range(G_TERMS):
        if k:
            term = term * sigma
            fact *= k
        s = s + term / (fact * (n + k + 1))
    return s


def w_coeffs(theta, sigma):
    """W = C I + A [w]x + B [w]x^2 = int_0^1 e^(tau sigma) exp(tau [w]x) dtau, exact; series in theta below TH_THETA."""
    theta, sigma = np.asarray(theta, np.float64), np.asarray(sigma, np.float64)
    small_s = np.abs(sigma) < TH_SIGMA
    ss = np.where(small_s, 1.0, sigma)
    C = np.where(small_s, 1.0 + 0.5 * sigma, np.expm1(ss) / ss)
    small_t = theta < TH_THETA
    th = np.where(small_t, 1.0, theta)
    # (e^z - 1) / z at z = sigma + i theta with e^z - 1 = P + i Q
    sh = np.sin(0.5 * th)
    P = np.expm1(sigma) * np.cos(th) - 2.0 * sh * sh
    Q = np.exp(sigma) * np.sin(th)
    c = sigma * sigma + th * th
    A = (Q * sigma - P * th) / (th * c)
    B = (C - (P * sigma + Q * th) / c) / (th * th)
    if np.any(small_t):
        t2 = theta * theta
        As = _g(1, sigma) - t2 * (_g(3, sigma) / 6.0 - t2 * (_g(5, sigma) / 120.0))
        Bs = _g(2, sigma) / 2.0 - t2 * (_g(4, sigma) / 24.0 - t2 * (_g(6, sigma) / 720.0))
        A, B = np.where(small_t, As, A), np.where(small_t, Bs, B)
    return A, B, C


def w_matrix(omega, sigma):
    theta = np.sqrt((omega * omega).sum(-1))
    A, B, C = w_coeffs(theta, sigma)
    K = skew(omega)
    return C[..., None, None] * np.eye(3) + A[..., None, None] * K + B[..., None, None] * (K @ K)


def exp(x):
    """x [..., 7] (upsilon, omega, sigma) -> pose [..., 8]"""
    x = np.asarray(x, np.float64)
    ups, om, sg = x[..., :3], x[..., 3:6], x[..., 6]
    t2 = (om * om).sum(-1)
    theta = np.sqrt(t2)
    small = theta < TH_THETA
    th = np.where(small, 1.0, theta)
    k = np.where(small, 0.5 - t2 * (1.0 / 48.0 - t2 * (1.0 / 3840.0 - t2 / 645120.0)), np.sin(0.5 * th) / th)
    q = np.concatenate([om * k[..., None], np.cos(0.5 * theta)[..., None]], -1)
    t = np.einsum("...ab,...b->...a", w_matrix(om, sg), ups)
    return np.concatenate([q, t, np.exp(sg)[..., None]], -1)


def inv3(M):
    """adjugate inverse of a 3 x 3 (the order of pgo_core.hpp)"""
    a, b, c, d, e, f, g, h, i = np.moveaxis(M.reshape(M.shape[:-2] + (9,)), -1, 0)
    A, Bc, Cc = e * i - f * h, c * h - b * i, b * f - c * e
    det = a * A + d * Bc + g * Cc
    out = np.stack([A, Bc, Cc, f * g - d * i, a * i - c * g, c * d - a * f, d * h - e * g, b * g - a * h, a * e - b * d], -1)
    return (out / det[..., None]).reshape(M.shape)


def log(T):
    """pose [..., 8] -> x [..., 7]"""
    T = np.asarray(T, np.float64)
    q = T[..., :4] * np.where(T[..., 3:4] < 0, -1.0, 1.0)
    v, w = q[..., :3], q[..., 3]
    n2 = (v * v).sum(-1)
    n = np.sqrt(n2)
    small = n < 0.5 * TH_THETA
    ns = np.where(small, 1.0, n)
    x2 = n2 / (w * w)
    k = np.where(small, (2.0 / w) * (1.0 - x2 * (1.0 / 3.0 - x2 * (1.0 / 5.0 - x2 / 7.0))), 2.0 * np.arctan2(ns, w) / ns)
    om = v * k[..., None]
    sg = np.log(T[..., 7])
    ups = np.einsum("...ab,...b->...a", inv3(w_matrix(om, sg)), T[..., 4:7])
    return np.concatenate([ups, om, sg[..., None]], -1)


def ad(x):
    x = np.asarray(x, np.float64)
    M = np.zeros(x.shape[:-1] + (7, 7))
    K = skew(x[..., 3:6])
    M[..., :3, :3] = K + x[..., 6, None, None] * np.eye(3)
    M[..., :3, 3:6] = skew(x[..., :3])
    M[..., :3, 6] = -x[..., :3]
    M[..., 3:6, 3:6] = K
    return M


def Ad(T):
    T = np.asarray(T, np.float64)
    R = quat_R(T[..., :4])
    M = np.zeros(T.shape[:-1] + (7, 7))
    M[..., :3, :3] = T[..., 7, None, None] * R
    M[..., :3, 3:6] = skew(T[..., 4:7]) @ R
    M[..., :3, 6] = -T[..., 4:7]
    M[..., 3:6, 3:6] = R
    M[..., 6, 6] = 1.0
    return M


def jr_inv(x):
    """sum_{n = 0..10} B_n / n! (-ad_x)^n"""
    N = -ad(x)
    P = np.broadcast_to(np.eye(7), N.shape).copy()
    S = P * JR_COEFF[0]
    for n in range(1, BERNOULLI_ORDER + 1):
        P = P @ N
        if JR_COEFF[n] != 0.0:
            S = S + JR_COEFF[n] * P
    return S


# ---- the graph ----
def measurements_from(poses, edges):
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    return mul(inv(poses[edges[:, 0]]), poses[edges[:, 1]])


def edge_terms(poses, edges, weights, meas, fix_scale, jacobians=True):
    """r [E, 7] and, optionally, J_i, J_j [E, 7, 7]; the se3 form leaves row / column 6 zero"""
    Ti, Tj = poses[edges[:, 0]], poses[edges[:, 1]]
    x = log(mul(inv(meas), mul(inv(Ti), Tj)))
    w = weights[:, None]
    D = 6 if fix_scale else 7
    r = w * x
    r[:, D:] = 0.0
    if not jacobians:
        return r
    S = jr_inv(x)
    Jj = w[..., None] * S
    Ji = -(Jj @ Ad(mul(inv(Tj), Ti)))
    Jj[:, D:, :], Jj[:, :, D:], Ji[:, D:, :], Ji[:, :, D:] = 0.0, 0.0, 0.0, 0.0
    return r, Ji, Jj


def cost(G, poses):
    if len(G["edges"]) == 0:
        return 0.0
    r = edge_terms(poses, G["edges"], G["weights"], G["meas"], G["fix_scale"], jacobians=False)
    return float((r * r).sum(-1).sum())


def prepare(G):
    """fill in the defaults of snk_pgo_set_graph: weights 1, measurements from poses_measure, start at poses_measure"""
    G = dict(G)
    G["edges"] = np.asarray(G["edges"], np.int32).reshape(-1, 2)
    E = len(G["edges"])
    G["poses_measure"] = np.asarray(G["poses_measure"], np.float64).reshape(-1, 8)
    G["constant"] = np.asarray(G["constant"], np.uint8)
    G["weights"] = np.ones(E) if G.get("weights") is None else np.asarray(G["weights"], np.float64)
    G["meas"] = measurements_from(G["poses_measure"], G["edges"]) if G.get("measurements") is None else np.asarray(G["measurements"], np.float64)
    G["start"] = G["poses_measure"].copy() if G.get("poses_init") is None else np.asarray(G["poses_init"], np.float64).reshape(-1, 8)
    n = len(G["poses_measure"])
    deg = np.bincount(G["edges"].ravel(), minlength=n) if E else np.zeros(n, np.int64)
    G["row"] = np.full(n, -1, np.int64)
    free = (G["constant"] == 0) & (deg > 0)
    G["row"][free] = np.arange(int(free.sum()))
    return G


def linearise(G, poses):
    """residuals [E, 7], gradient J^T r [n, 7], diagonal blocks [n, 49], off-diagonal J_i^T J_j [E, 7, 7] (all vertices, constants included)"""
    n, E = len(poses), len(G["edges"])
    grad, diag = np.zeros((n, 7)), np.zeros((n, 7, 7))
    if E == 0:
        return np.zeros((0, 7)), grad, diag.reshape(n, 49), np.zeros((0, 7, 7))
    r, Ji, Jj = edge_terms(poses, G["edges"], G["weights"], G["meas"], G["fix_scale"])
    Hii, Hjj, Hij = np.swapaxes(Ji, 1, 2) @ Ji, np.swapaxes(Jj, 1, 2) @ Jj, np.swapaxes(Ji, 1, 2) @ Jj
    gi, gj = np.einsum("eka,ek->ea", Ji, r), np.einsum("eka,ek->ea", Jj, r)
    for e in range(E):  # edge order, the order of the device's incident-edge lists
        i, j = G["edges"][e]
        diag[i] += Hii[e]
        diag[j] += Hjj[e]
        grad[i] += gi[e]
        grad[j] += gj[e]
    return r, grad, diag.reshape(n, 49), Hij


def retract(poses, delta):
    out = mul(poses, exp(delta))
    out[:, :4] /= np.sqrt((out[:, :4] ** 2).sum(-1))[:, None]
    return out


def solve_step(G, grad, diag, Hij, lam):
    """(H + lam clamp(diag H, 1e-6, 1e32)) delta = -g over the free rows, scipy's sparse direct solver"""
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve

    row, n = G["row"], len(G["row"])
    D = 6 if G["fix_scale"] else 7
    nr = int((row >= 0).sum())
    delta = np.zeros((n, 7))
    if nr == 0:
        return delta
    fv = np.nonzero(row >= 0)[0]
    Dg = diag.reshape(n, 7, 7)[fv][:, :D, :D].copy()
    idx = np.arange(D)
    Dg[:, idx, idx] += lam * np.clip(Dg[:, idx, idx], 1e-6, 1e32)
    a, b = np.meshgrid(idx, idx, indexing="ij")
    rows = [(np.arange(nr)[:, None, None] * D + a).ravel()]
    cols = [(np.arange(nr)[:, None, None] * D + b).ravel()]
    vals = [Dg.ravel()]
    ri, rj = row[G["edges"][:, 0]], row[G["edges"][:, 1]]
    both = (ri >= 0) & (rj >= 0)
    if both.any():
        Hb = Hij[both][:, :D, :D]
        R_, C_ = (ri[both][:, None, None] * D + a), (rj[both][:, None, None] * D + b)
        rows += [R_.ravel(), C_.ravel()]
        cols += [C_.ravel(), R_.ravel()]
        vals += [Hb.ravel(), Hb.ravel()]
    A = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(nr * D, nr * D))
    x = spsolve(A, -grad[fv][:, :D].ravel()).reshape(nr, D)
    delta[fv, :D] = x
    return delta


def optimise(G, max_iterations=MAX_ITERATIONS, min_chi2_delta=MIN_CHI2_DELTA, lambda_init=LAMBDA_INIT):
    """the LM loop of snk-pgo v1; returns (poses, dict(cost_initial, cost_final, lm_iterations, accepted_steps))"""
    G = prepare(G) if "row" not in G else G
    poses = G["start"].copy()
    c = cost(G, poses)
    info = dict(cost_initial=c, cost_final=c, lm_iterations=0, accepted_steps=0)
    if not (G["row"] >= 0).any():
        return poses, info
    lam, v, lin = lambda_init, 2.0, None
    for _ in range(max_iterations):
        if lin is None:
            lin = linearise(G, poses)
        delta = solve_step(G, lin[1], lin[2], lin[3], lam)
        trial = poses.copy()
        fv = G["row"] >= 0
        trial[fv] = retract(poses[fv], delta[fv])
        c_new = cost(G, trial)
        info["lm_iterations"] += 1
        if c_new < c:
            dec, poses, c, lam, v, lin = c - c_new, trial, c_new, lam * (1.0 / 3.0), 2.0, None
            info["accepted_steps"] += 1
            if dec < min_chi2_delta:
                break
        else:
            lam, v = lam * v, v * 2.0
    info["cost_final"] = c
    return poses, info


def pose_distance(a, b):
    """largest absolute difference over the 8 entries, quaternion signs aligned"""
    a, b = np.asarray(a, np.float64).reshape(-1, 8).copy(), np.asarray(b, np.float64).reshape(-1, 8)
    if len(a) == 0:
        return 0.0
    sgn = np.where((a[:, :4] * b[:, :4]).sum(-1) < 0, -1.0, 1.0)
    a[:, :4] *= sgn[:, None]
    return float(np.abs(a - b).max())


def pose_tolerance():
    """10 x the largest pose_distance between optimise() and scipy.optimize.least_squares (x_scale 1, xtol = ftol = gtol = 1e-15) on the
    same residual over reference_graphs(), both forms (tests/test_pgo_numpy.py prints and re-checks the floor)."""
    return 10 * POSE_FLOOR


POSE_FLOOR = 2.82e-7  # measured: 1.08e-7 (se3) and 2.813e-7 (sim3), both on ring40x3; line3 4e-11, loop8 6e-9, hub70 3e-8


def transform_points(before, after, constant, ref, pos, normal=None, depth=None):
    """the map-point pass of OptimizeEssentialGraph: point k moves by after[ref] . before[ref]^-1 unless ref < 0 or the vertex is constant"""
    pos = np.array(pos, np.float64)
    normal = None if normal is None else np.array(normal, np.float64)
    depth = None if depth is None else np.array(depth, np.float64)
    ref = np.asarray(ref, np.int64)
    m = (ref >= 0) & (np.asarray(constant)[np.maximum(ref, 0)] == 0)
    T = mul(after[ref[m]], inv(before[ref[m]]))
    R = quat_R(T[:, :4])
    pos[m] = T[:, 7:8] * np.einsum("kab,kb->ka", R, pos[m]) + T[:, 4:7]
    if normal is not None:
        normal[m] = np.einsum("kab,kb->ka", R, normal[m])
    if depth is not None:
        depth[m] = depth[m] * T[:, 7]
    return pos, normal, depth


# ---- graph generators (seeded; ground-truth trajectory + noise, residuals below about 0.3 in norm) ----
def _trajectory(n, rng, sim3, radius=None):
    radius = max(2.0, 0.15 * n) if radius is None else radius
    a = 2 * np.pi * np.arange(n) / max(n, 1)
    x = np.zeros((n, 7))
    x[:, 3:6] = np.stack([0.1 * np.sin(3 * a), 0.1 * np.cos(2 * a), a], -1)
    T = exp(x)
    T[:, 4:7] = np.stack([radius * np.cos(a), radius * np.sin(a), 0.2 * np.sin(2 * a)], -1) + 0.02 * rng.standard_normal((n, 3))
    if sim3:
        T[:, 7] = np.exp(0.05 * np.sin(a) + 0.01 * rng.standard_normal(n))
    return T


def _noise(rng, m, sim3, sd):
    x = sd * rng.standard_normal((m, 7))
    if not sim3:
        x[:, 6] = 0.0
    return x


def ring_edges(n, k):
    """vertex i to i + 1 .. i + k (mod n): i < j, unique, sorted"""
    e = {(min(i, (i + d) % n), max(i, (i + d) % n)) for i in range(n) for d in range(1, k + 1) if (i + d) % n != i}
    return np.array(sorted(e), np.int32).reshape(-1, 2)


def ring(n, k, seed, fix_scale, n_const=1, meas_sd=0.01, init_sd=0.02, weights=True):
    rng = np.random.default_rng(seed)
    sim3 = not fix_scale
    gt = _trajectory(n, rng, sim3)
    edges = ring_edges(n, k)
    meas = mul(measurements_from(gt, edges), exp(_noise(rng, len(edges), sim3, meas_sd)))
    init = mul(gt, exp(_noise(rng, n, sim3, init_sd)))
    const = np.zeros(n, np.uint8)
    const[:n_const] = 1
    init[const == 1] = gt[const == 1]
    w = 0.5 + rng.random(len(edges)) if weights else None
    return dict(name=f"ring{n}x{k}", poses_measure=gt, poses_init=init, constant=const, edges=edges, weights=w, measurements=meas,
                fix_scale=int(fix_scale))


def correct_loop(n, seed, fix_scale, k=1):
    """the CorrectLoop shape: a drifted ring measured as it is, a loop edge between source (n - 1) and target (0), both constant, the
    source moved to its corrected pose by set_pose -- measurements come from poses_measure, the loop edge's from the correction"""
    rng = np.random.default_rng(seed)
    sim3 = not fix_scale
    gt = _trajectory(n, rng, sim3)
    d = np.array([0.12, -0.08, 0.05, 0.02, -0.03, 0.06, 0.08 if sim3 else 0.0])
    corrected = mul(gt[n - 1], exp(d[None])[0])
    e = {(i, i + d_) for i in range(n) for d_ in range(1, k + 1) if i + d_ < n} | {(0, n - 1)}
    edges = np.array(sorted(e), np.int32)
    meas = measurements_from(gt, edges)
    loop = int(np.nonzero((edges == (0, n - 1)).all(1))[0][0])
    meas[loop] = mul(inv(gt[0]), corrected)
    init = gt.copy()
    init[n - 1] = corrected
    const = np.zeros(n, np.uint8)
    const[[0, n - 1]] = 1
    return dict(name=f"loop{n}", poses_measure=gt, poses_init=init, constant=const, edges=edges, weights=None, measurements=meas,
                fix_scale=int(fix_scale))


def line3(seed, fix_scale):
    rng = np.random.default_rng(seed)
    sim3 = not fix_scale
    gt = np.zeros((3, 8))
    gt[:, 3], gt[:, 7], gt[:, 4] = 1.0, 1.0, [0.0, 1.0, 2.0]
    init = mul(gt, exp(_noise(rng, 3, sim3, 0.05)))
    init[0] = gt[0]
    return dict(name="line3", poses_measure=gt, poses_init=init, constant=np.array([1, 0, 0], np.uint8),
                edges=np.array([[0, 1], [1, 2]], np.int32), weights=np.array([1.0, 2.0]), measurements=None, fix_scale=int(fix_scale))


def hub(m, seed, fix_scale):
    """vertex 0 with m neighbours (a degree above the wavefront width), the neighbours chained; vertex 1 constant"""
    rng = np.random.default_rng(seed)
    sim3 = not fix_scale
    gt = _trajectory(m + 1, rng, sim3, radius=2.0)
    gt[0, 4:7] = 0.0
    e = {(0, j) for j in range(1, m + 1)} | {(j, j + 1) for j in range(1, m)}
    edges = np.array(sorted(e), np.int32)
    meas = mul(measurements_from(gt, edges), exp(_noise(rng, len(edges), sim3, 0.01)))
    init = mul(gt, exp(_noise(rng, m + 1, sim3, 0.02)))
    const = np.zeros(m + 1, np.uint8)
    const[1] = 1
    init[1] = gt[1]
    return dict(name=f"hub{m}", poses_measure=gt, poses_init=init, constant=const, edges=edges, weights=None, measurements=meas,
                fix_scale=int(fix_scale))


def with_isolated(G, seed):
    """G plus one free vertex without edges (appended, so that the edges stay valid)"""
    rng = np.random.default_rng(seed)
    G = dict(G)
    extra = exp(_noise(rng, 1, not G["fix_scale"], 0.3))
    G["poses_measure"] = np.concatenate([G["poses_measure"], extra])
    G["poses_init"] = np.concatenate([G["poses_init"], extra])
    G["constant"] = np.concatenate([G["constant"], [0]]).astype(np.uint8)
    G["name"] += "+isolated"
    return G


def reference_graphs(fix_scale):
    """the small graphs of the GPU test; the floor behind pose_tolerance() is measured over them"""
    gs = [line3(1, fix_scale), correct_loop(8, 2, fix_scale), ring(40, 3, 3, fix_scale), hub(70, 4, fix_scale),
          with_isolated(ring(12, 2, 5, fix_scale), 6)]
    return gs
