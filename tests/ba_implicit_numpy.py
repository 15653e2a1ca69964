"""Vectorised numpy restatement of ONE snk-ba v1 LM iteration with the reduced camera system solved in implicit form (test helper).

It follows the oracle (oracle/ba_oracle.c, orc_ba_solve): the same observation model, Jacobians, Huber IRLS weights, damping with
lambda_init, block-Jacobi PCG from x0 = 0 with the same stop rule, back-substitution, SE(3) update, trial cost and accept / reject.
The Schur complement S is never formed: S p = U p + (constraint cross blocks) p - W V^-1 W^T p is evaluated from the per-observation
W blocks with sparse index arithmetic (np.bincount, einsum), so a 10 000-keyframe map (720 k observations) takes seconds.  The one
piece taken from the oracle is the residual / Jacobian of a relative pose constraint (oracle.ba_rpc_linearize: one small function
per constraint; the normal equations they enter are restated here)."""
import numpy as np


def _quat_R(q):
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def _segsum(idx, vals, n):
    """sum of vals[k] into row idx[k] of an (n, ...) array."""
    flat = vals.reshape(len(vals), int(np.prod(vals.shape[1:])))
    out = np.empty((n, flat.shape[1]))
    for j in range(flat.shape[1]):
        out[:, j] = np.bincount(idx, weights=flat[:, j], minlength=n)
    return out.reshape((n,) + vals.shape[1:])


def _clamp(v):
    return np.clip(v, 1e-6, 1e32)


def _observations(sc, outlier):
    n_img, n_pt = len(sc["pose"]), len(sc["pt"])
    i = np.asarray(sc["obs_img"], np.int64)
    p = np.asarray(sc["obs_pt"], np.int64)
    ok = (i >= 0) & (i < n_img) & (p >= 0) & (p < n_pt)
    ic, pc = np.asarray(sc["img_const"]).astype(bool), np.asarray(sc["pt_const"]).astype(bool)
    ok[ok] &= ~(ic[i[ok]] & pc[p[ok]])
    if outlier is not None:
        ok &= ~np.asarray(outlier).astype(bool)
    return np.nonzero(ok)[0]


def _linearize(sc, pose, pt, obs, huber_mono, huber_stereo, jac=True):
    """rho per observation of `obs` and (jac) the IRLS-scaled r (n,3), Jc (n,3,6), Jp (n,3,3); rows of inactive ones are zero."""
    i, p = np.asarray(sc["obs_img"])[obs], np.asarray(sc["obs_pt"])[obs]
    R = _quat_R(pose[i, :4])
    Xc = np.einsum("nij,nj->ni", R, pt[p]) + pose[i, 4:]
    X, Y, Z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    front = Z > 0
    iz = np.where(front, 1.0 / np.where(front, Z, 1.0), 0.0)
    iz2 = iz * iz
    fx, fy, cx, cy = sc["K"]
    bf = float(sc["bf"])
    uv, d, w = np.asarray(sc["obs_uv"])[obs], np.asarray(sc["obs_depth"])[obs], np.asarray(sc["obs_weight"])[obs]
    st = d > 0
    r = np.zeros((len(obs), 3))
    r[:, 0] = w * (fx * X * iz + cx - uv[:, 0])
    r[:, 1] = w * (fy * Y * iz + cy - uv[:, 1])
    r[:, 2] = np.where(st, w * ((fx * X * iz + cx - bf * iz) - (uv[:, 0] - bf / np.where(st, d, 1.0))), 0.0)
    r[~front] = 0.0
    s = (r * r).sum(1)
    delta = np.where(st, huber_stereo, huber_mono)
    big = s > delta * delta
    rho = np.where(big, 2 * delta * np.sqrt(s) - delta * delta, s)
    rho[~front] = 0.0
    if not jac:
        return rho
    sw = np.where(big, np.sqrt(delta / np.sqrt(np.where(big, s, 1.0))), 1.0)
    sw[~front] = 0.0
    m = np.zeros((len(obs), 3, 3))  # rows m_k = w * d proj_k / d Xc
    m[:, 0, 0], m[:, 0, 2] = fx * iz, -fx * X * iz2
    m[:, 1, 1], m[:, 1, 2] = fy * iz, -fy * Y * iz2
    m[:, 2, 0], m[:, 2, 2] = fx * iz, -fx * X * iz2 + bf * iz2
    m[~st, 2, :] = 0.0
    m *= (w * sw)[:, None, None]
    Jc = np.concatenate([m, np.cross(Xc[:, None, :], m)], axis=2)  # [m_k | Xc x m_k]
    Jp = np.einsum("nki,nij->nkj", m, R)
    return rho, r * sw[:, None], Jc, Jp


def _rpcs(sc, pose, cam):
    """valid constraints: list of (c1, c2, r, J1, w)"""
    from oracle import oracle

    rp = sc.get("rpc")
    if rp is None or len(rp) == 0:
        return []
    ic = np.asarray(sc["img_const"]).astype(bool)
    out = []
    for q in rp:
        a, b = int(q["img1"]), int(q["img2"])
        if a < 0 or b < 0 or a >= len(pose) or b >= len(pose) or a == b or (ic[a] and ic[b]):
            continue
        r, J1 = oracle.ba_rpc_linearize(pose[a], pose[b], q)
        wv = np.array([q["weight_translation"]] * 3 + [q["weight_rotation"]] * 3, np.float64)
        out.append((cam[a], cam[b], r, J1, wv))
    return out


def total_cost(sc, pose, pt, outlier=None, huber_mono=2.1, huber_stereo=2.3):
    obs = _observations(sc, outlier)
    c = float(_linearize(sc, pose, pt, obs, huber_mono, huber_stereo, jac=False).sum())
    cam = np.full(len(pose), -1)
    for (_, _, r, _, _) in _rpcs(sc, pose, cam):
        c += float(r @ r)
    return c


def _inv_spd6(D):
    """block-Jacobi preconditioner blocks: Cholesky inverse, 1 / clamp(diag) where a block is not positive definite (the oracle's rule)"""
    out = np.zeros_like(D)
    for k in range(len(D)):
        try:
            L = np.linalg.cholesky(D[k])
            Li = np.linalg.inv(L)
            out[k] = Li.T @ Li
        except np.linalg.LinAlgError:
            out[k] = np.diag(1.0 / _clamp(np.diag(D[k])))
    return out


def _se3_update(pose, d):
    """exp(d) * pose, d = (translation, rotation), the oracle's closed form (orc_se3_update)."""
    w, v = d[:, 3:], d[:, :3]
    th2 = (w * w).sum(1)
    th = np.sqrt(th2)
    small = th < 1e-8
    ths = np.where(small, 1.0, th)
    B = np.where(small, 0.5 - th2 / 24.0, (1.0 - np.cos(ths)) / np.where(small, 1.0, th2))
    Cc = np.where(small, 1.0 / 6.0 - th2 / 120.0, (ths - np.sin(ths)) / (np.where(small, 1.0, th2) * ths))
    h = np.where(small, 0.5 - th2 / 48.0, np.sin(0.5 * ths) / ths)
    qd = np.concatenate([h[:, None] * w, np.where(small, 1.0 - th2 / 8.0, np.cos(0.5 * ths))[:, None]], 1)
    c1 = np.cross(w, v)
    c2 = np.cross(w, c1)
    td = v + B[:, None] * c1 + Cc[:, None] * c2
    Rd = _quat_R(qd)
    a, b = qd, pose[:, :4]
    ax, ay, az, aw = a.T
    bx, by, bz, bw = b.T
    q = np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                  aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], 1)
    q /= np.sqrt((q * q).sum(1))[:, None]
    t = np.einsum("nij,nj->ni", Rd, pose[:, 4:]) + td
    return np.concatenate([q, t], 1)


def lm_iteration(sc, max_pcg=40, pcg_tol=1e-10, huber_mono=2.1, huber_stereo=2.3, lambda_init=0.0, outlier=None):
    """One LM iteration from the scene's state.  Returns (pose, pt, cost_initial, cost_final, pcg_iterations)."""
    pose = np.asarray(sc["pose"], np.float64).copy()
    pt = np.asarray(sc["pt"], np.float64).copy()
    n_img, n_pt = len(pose), len(pt)
    ic, pc = np.asarray(sc["img_const"]).astype(bool), np.asarray(sc["pt_const"]).astype(bool)
    cam = np.full(n_img, -1, np.int64)
    cam[~ic] = np.arange(int((~ic).sum()))
    nfc = int((~ic).sum())
    lam = lambda_init if lambda_init > 0 else 1e-4
    obs = _observations(sc, outlier)
    rho, r, Jc, Jp = _linearize(sc, pose, pt, obs, huber_mono, huber_stereo)
    rpcs = _rpcs(sc, pose, cam)
    cost = float(rho.sum()) + sum(float(q[2] @ q[2]) for q in rpcs)
    oc = cam[np.asarray(sc["obs_img"])[obs]]
    op = np.asarray(sc["obs_pt"], np.int64)[obs]
    # normal equations
    hc = oc >= 0
    U = _segsum(oc[hc], np.einsum("nka,nkb->nab", Jc[hc], Jc[hc]), nfc)
    bc = -_segsum(oc[hc], np.einsum("nka,nk->na", Jc[hc], r[hc]), nfc)
    hp = ~pc[op]
    V = _segsum(op[hp], np.einsum("nka,nkb->nab", Jp[hp], Jp[hp]), n_pt)
    bp = -_segsum(op[hp], np.einsum("nka,nk->na", Jp[hp], r[hp]), n_pt)
    used = hc & hp
    Wc, Wp, Wm = oc[used], op[used], np.einsum("nka,nkb->nab", Jc[used], Jp[used])  # W_o = Jc^T Jp (6 x 3)
    cross = []
    for c1, c2, rr, J1, wv in rpcs:
        if c1 >= 0:
            U[c1] += J1.T @ J1
            bc[c1] -= J1.T @ rr
        if c2 >= 0:
            U[c2] += np.diag(wv * wv)
            bc[c2] -= wv * rr
        if c1 >= 0 and c2 >= 0:
            cross.append((c1, c2, J1.T * wv[None, :]))  # H12 = J1^T W
    # damping, V^-1
    k6, k3 = np.arange(6), np.arange(3)
    U[:, k6, k6] += lam * _clamp(U[:, k6, k6])
    V[:, k3, k3] += np.where(pc[:, None], 0.0, lam * _clamp(V[:, k3, k3]))
    det = np.linalg.det(V)
    Vi = np.zeros_like(V)
    inv = ~pc & (det != 0.0)
    Vi[inv] = np.linalg.inv(V[inv])
    # reduced right-hand side and the preconditioner's blocks D_c = U_c - sum W V^-1 W^T
    Y = np.einsum("nab,nbc->nac", Wm, Vi[Wp])
    rhs = bc - _segsum(Wc, np.einsum("nab,nb->na", Y, bp[Wp]), nfc)
    D = U - _segsum(Wc, np.einsum("nab,ncb->nac", Y, Wm), nfc)
    Minv = _inv_spd6(D)

    def S_mul(p):  # implicit S p
        y = np.einsum("nab,nb->na", Vi, _segsum(Wp, np.einsum("nab,na->nb", Wm, p[Wc]), n_pt))
        q = np.einsum("nab,nb->na", U, p) - _segsum(Wc, np.einsum("nab,nb->na", Wm, y[Wp]), nfc)
        for c1, c2, H in cross:
            q[c1] += H @ p[c2]
            q[c2] += H.T @ p[c1]
        return q

    # block-Jacobi PCG, x0 = 0, stop when |r|^2 <= tol^2 |rhs|^2 or after max_pcg iterations
    x = np.zeros((nfc, 6))
    res = rhs.copy()
    z = np.einsum("nab,nb->na", Minv, res)
    p = z.copy()
    rz = float((res * z).sum())
    stop2 = pcg_tol * pcg_tol * float((rhs * rhs).sum())
    its = 0
    for _ in range(max_pcg if nfc > 0 else 0):
        if float((res * res).sum()) <= stop2:
            break
        Ap = S_mul(p)
        pAp = float((p * Ap).sum())
        if pAp <= 0.0:
            break
        alpha = rz / pAp
        x += alpha * p
        res -= alpha * Ap
        z = np.einsum("nab,nb->na", Minv, res)
        rz_new = float((res * z).sum())
        p = z + (rz_new / rz) * p
        rz = rz_new
        its += 1
    # back-substitution, trial state, accept / reject
    g = bp - _segsum(Wp, np.einsum("nab,na->nb", Wm, x[Wc]), n_pt)
    dpt = np.where(pc[:, None], 0.0, np.einsum("nab,nb->na", Vi, g))
    pose_new = pose.copy()
    if nfc:
        pose_new[~ic] = _se3_update(pose[~ic], x[cam[~ic]])
    pt_new = pt + dpt
    cost_new = total_cost(sc, pose_new, pt_new, outlier, huber_mono, huber_stereo)
    if cost_new < cost:
        return pose_new, pt_new, cost, cost_new, its
    return pose, pt, cost, cost, its
