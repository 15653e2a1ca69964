"""Independent float64 numpy restatement of "snk-tri v1" (DESIGN.md section 3b): the geometric loop of Triangulator::triangulate
(reference Snake/LocalMapping/Triangulator.cpp:127-291) pair by pair in a Python loop, np.linalg.svd for the homogeneous system, the
reference's float roundings mirrored with np.float32, and the first-wins commit rule of Triangulator::Process (:61-70).

For every pair it returns the decision, the branch taken, the point and a MARGIN: the smallest relative distance of any gate it
evaluated to that gate's threshold.  A pair whose margin is below BORDERLINE may legitimately be decided differently by another correct
implementation (one float rounding of a cosine); the tests leave those out of the decision comparison and cap their share.

Also here: the synthetic cases of the triangulation tests (make_case), built on the geometry of track_helpers.make_triangulation_case
(same intrinsics, bf, image bounds, pose and depth distributions) but keeping the correspondences, with several neighbours, stereo
depths, a far subset and conflicting pairs."""
import numpy as np

from track_helpers import BF, BOUNDS, K_EUROC, quat_R

KP64 = np.dtype([("x", "<f8"), ("y", "<f8"), ("angle", "<f4"), ("octave", "<i4")])
NEW_POINT = np.dtype([("feature1", "<i4"), ("feature2", "<i4"), ("neighbour", "<i4"), ("far_away", "u1"), ("commit", "u1"),
                      ("branch", "u1"), ("pad", "u1"), ("pos", "<f8", 3)])
REJECT, TRIANGULATED, STEREO1, STEREO2 = 0, 1, 2, 3

BORDERLINE = 1e-6       # margin below which a pair's decision is not compared
BORDERLINE_CAP = 0.01   # at most this share of a case may be borderline

# The floor of what two correct float64 solutions of TriangulateHomogeneous disagree by on the inputs of the GPU tests: the largest
# relative difference (max over coordinates of |a - b| / max(1, |a|)) between the SVD of A and eigh of A^T A over every pair of every
# case in CASES that takes the triangulation branch.  Produced by
#     python tests/tri_numpy.py --floor
# which prints the value stored here.  The position tolerance of the GPU tests is 10 x this floor, and never looser than the
# project's BA bound of 1e-5.
POSITION_FLOOR = 8.984e-12
BA_BOUND = 1e-5


def position_tolerance():
    return min(10.0 * POSITION_FLOOR, BA_BOUND)


class Margin:
    """Smallest relative distance of the compared pairs of values seen so far."""

    def __init__(self):
        self.value = np.inf

    def see(self, a, b, scale=None):
        a, b = float(a), float(b)
        s = max(abs(a), abs(b)) if scale is None else float(scale)
        self.value = min(self.value, abs(a - b) / s if s > 0 else 0.0)

    def lt(self, a, b, scale=None):
        self.see(a, b, scale)
        return a < b

    def gt(self, a, b, scale=None):
        self.see(a, b, scale)
        return a > b


def pose_parts(pose):
    """R, t of the world -> camera pose (qx qy qz qw tx ty tz) and the camera centre pose.inverse().translation()."""
    pose = np.asarray(pose, np.float64)
    R, t = quat_R(pose[:4]), pose[4:]
    return R, t, -R.T @ t


def homogeneous_rows(R1, t1, R2, t2, p1, p2):
    rows = []
    for (R, t), (x, y) in (((R1, t1), p1), ((R2, t2), p2)):
        P = np.hstack([R, t[:, None]])
        rows += [x * P[2] - P[0], y * P[2] - P[1]]
    A = np.array(rows)
    return A / np.linalg.norm(A, axis=1, keepdims=True)


def triangulate_homogeneous(R1, t1, R2, t2, p1, p2, method="svd"):
    """TriangulateHomogeneous<double, true> [DEFINED]: unit rows, smallest right singular vector, dehomogenised."""
    A = homogeneous_rows(R1, t1, R2, t2, p1, p2)
    if method == "svd":
        v = np.linalg.svd(A)[2][-1]
    else:
        v = np.linalg.eigh(A.T @ A)[1][:, 0]
    return v[:3] / v[3]


def _reprojection_rejects(mg, cam, chi2, ls, kp, ur, stereo, xc):
    fx, fy, cx, cy, bf = cam
    s = np.float32(ls[kp["octave"]])
    sigma2 = np.float32(s * s)
    u, v = fx * xc[0] / xc[2] + cx, fy * xc[1] / xc[2] + cy
    e2 = (u - kp["x"]) ** 2 + (v - kp["y"]) ** 2
    if stereo:
        e2 += ((u - bf / xc[2]) - float(ur)) ** 2
    return mg.gt(e2, float(np.float32(chi2 * sigma2)))


def tri_pair(cam, params, kf1, kf2, idx1, idx2, ls, why=None):
    """One pass of the loop body of :174-291.  Returns (branch, pos or None, far_away, margin); `why` (a list) receives the name of
    the gate that rejected the pair."""
    why = [] if why is None else why
    fx, fy, cx, cy, bf = cam
    mg = Margin()
    R1, t1, c1 = pose_parts(kf1["pose"])
    R2, t2, c2 = pose_parts(kf2["pose"])
    chi2_mono = np.float32(params["error_mono"]) * np.float32(params["error_mono"])
    chi2_stereo = np.float32(params["error_stereo"]) * np.float32(params["error_stereo"])
    ratio_factor = np.float32(1.5) * np.float32(params["scale_factor"])
    baseline = bf / fx
    kp1, kp2 = kf1["kps"][idx1], kf2["kps"][idx2]
    ur1, ur2 = np.float32(kf1["right_points"][idx1]), np.float32(kf2["right_points"][idx2])
    st1, st2 = bool(ur1 >= 0), bool(ur2 >= 0)
    d1, d2 = float(np.float32(kf1["depth"][idx1])), float(np.float32(kf2["depth"][idx2]))
    xn1 = np.array([(kp1["x"] - cx) / fx, (kp1["y"] - cy) / fy, 1.0])
    xn2 = np.array([(kp2["x"] - cx) / fx, (kp2["y"] - cy) / fy, 1.0])
    ray1, ray2 = R1.T @ xn1, R2.T @ xn2
    cos_rays = np.float32(ray1 @ ray2 / (np.linalg.norm(ray1) * np.linalg.norm(ray2)))
    cos_stereo1 = cos_stereo2 = np.float32(cos_rays + np.float32(1))
    if st1:
        cos_stereo1 = np.float32(np.cos(2 * np.arctan2(baseline / 2, d1)))
    elif st2:
        cos_stereo2 = np.float32(np.cos(2 * np.arctan2(baseline / 2, d2)))
    cos_stereo = min(cos_stereo1, cos_stereo2)
    th_parall = np.float32(0.9998)
    far_away = False
    if mg.lt(cos_rays, cos_stereo, 1.0) and mg.gt(cos_rays, 0.0, 1.0) and (st1 or st2 or mg.lt(cos_rays, th_parall, 1.0)):
        X = triangulate_homogeneous(R1, t1, R2, t2, xn1[:2], xn2[:2])
        branch = TRIANGULATED
    elif st1 and mg.lt(cos_stereo1, cos_stereo2, 1.0):
        X = R1.T @ (xn1 * d1 - t1)
        far_away = mg.gt(d1, params["th_depth"])
        branch = STEREO1
    elif st2 and mg.lt(cos_stereo2, cos_stereo1, 1.0):
        X = R2.T @ (xn2 * d2 - t2)
        far_away = mg.gt(d2, params["th_depth"])
        branch = STEREO2
    else:
        why.append("parallax")
        return REJECT, None, False, mg.value
    xc1, xc2 = R1 @ X + t1, R2 @ X + t2
    if not mg.gt(xc1[2], 0.0, np.linalg.norm(xc1)) or not mg.gt(xc2[2], 0.0, np.linalg.norm(xc2)):
        why.append("behind")
        return REJECT, None, False, mg.value
    if _reprojection_rejects(mg, cam, chi2_stereo if st1 else chi2_mono, ls, kp1, ur1, st1, xc1):
        why.append("chi2_stereo_1" if st1 else "chi2_mono_1")
        return REJECT, None, False, mg.value
    if _reprojection_rejects(mg, cam, chi2_stereo if st2 else chi2_mono, ls, kp2, ur2, st2, xc2):
        why.append("chi2_stereo_2" if st2 else "chi2_mono_2")
        return REJECT, None, False, mg.value
    dist1, dist2 = np.linalg.norm(c1 - X), np.linalg.norm(c2 - X)
    if dist1 == 0 or dist2 == 0:
        why.append("zero_distance")
        return REJECT, None, False, mg.value
    ratio_dist = dist2 / dist1
    ratio_octave = np.float32(np.float32(ls[kp1["octave"]]) / np.float32(ls[kp2["octave"]]))
    if mg.lt(ratio_dist * float(ratio_factor), float(ratio_octave)):
        why.append("scale_low")
        return REJECT, None, False, mg.value
    if mg.gt(ratio_dist, float(np.float32(ratio_octave * ratio_factor))):
        why.append("scale_high")
        return REJECT, None, False, mg.value
    return branch, X, bool(far_away), mg.value


def neighbour_skipped(cam, params, kf1, kf2, median_depth2):
    """The baseline gate of :140-157.  Returns (skipped, margin)."""
    mg = Margin()
    c1, c2 = pose_parts(kf1["pose"])[2], pose_parts(kf2["pose"])[2]
    baseline = np.linalg.norm(c1 - c2)
    if params["mono"]:
        ratio = np.float32(baseline / float(np.float32(median_depth2)))
        return mg.lt(float(ratio), 0.01), mg.value
    return mg.lt(baseline, cam[4] / cam[0]), mg.value


def commit_pass(entries, has1, has2s):
    """entries: (neighbour, feature1, feature2) in visiting order.  The test of :67 against a map that the kept entries edit."""
    used1 = np.asarray(has1).astype(bool).copy()
    used2 = [np.asarray(h).astype(bool).copy() for h in has2s]
    out = []
    for nb, a, b in entries:
        keep = not used1[a] and not used2[nb][b]
        if keep:
            used1[a] = used2[nb][b] = True
        out.append(keep)
    return out


def triangulate_neighbours(cam, params, kf1, kf2s, median_depth2s, pairs, ls):
    """pairs: one (n, 2) array per neighbour.  Returns one list per neighbour of (branch, pos, far_away, margin) per pair."""
    res = []
    for k, kf2 in enumerate(kf2s):
        skipped, m0 = neighbour_skipped(cam, params, kf1, kf2, median_depth2s[k])
        rows = []
        for a, b in np.asarray(pairs[k]).reshape(-1, 2):
            if skipped:
                rows.append((REJECT, None, False, m0))
            else:
                br, X, far, mg = tri_pair(cam, params, kf1, kf2, int(a), int(b), ls)
                rows.append((br, X, far, min(mg, m0)))
        res.append(rows)
    return res


# ------------------------------------------------------------------------------------------------ cases
PARAMS = dict(error_mono=2.1, error_stereo=2.3, th_depth=35.0, scale_factor=1.2, mono=0)
N_LEVELS = 8
# the neighbours' translations: baselines on both sides of bf / fx = 0.104 m (and, in mono mode, of 1 % of the median depth); the ones
# along the optical axis leave the central points with less parallax than a stereo depth has, which is what the stereo fallbacks are for
NEIGHBOUR_OFFSETS = ((0.6, 0, 0), (0.03, 0, 0.5), (0.05, 0, 0), (0.3, 0, 0), (0.02, 0, 0), (-0.9, 0, 0), (0, 0.02, -0.4), (0.08, 0, 0),
                     (-0.25, 0, 0), (1.2, 0, 0))
# (seed, neighbours, mode); mode: "mixed" = half the features have a stereo depth, "mono", "stereo" = all of them
CASES = [(11, 5, "mixed"), (12, 10, "mixed"), (13, 10, "mixed"), (14, 5, "mono"), (15, 10, "mono"), (16, 5, "stereo"), (17, 10, "stereo")]


def make_case(seed, n_neighbours, mode, m_pts=400, n_clutter=100):
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = K_EUROC
    cam = (fx, fy, cx, cy, BF)
    ls = (np.float32(1.2) ** np.arange(N_LEVELS)).astype(np.float32)
    params = dict(PARAMS, mono=1 if mode == "mono" else 0)
    stereo_frac = {"mixed": 0.5, "mono": 0.0, "stereo": 1.0}[mode]

    def pose(offset):
        q = rng.normal(size=4) * 0.02 + np.array([0, 0, 0, 1.0])
        q /= np.linalg.norm(q)
        return np.concatenate([q, rng.normal(size=3) * 0.01 + np.asarray(offset, np.float64)])

    pose1 = pose((0, 0, 0))
    R1, t1 = quat_R(pose1[:4]), pose1[4:]
    pc1 = np.stack([rng.uniform(-3, 3, m_pts), rng.uniform(-2, 2, m_pts), rng.uniform(3, 9, m_pts)], 1)
    far = rng.random(m_pts) < 0.08  # the far subset at 40-80 m: little parallax, so the stereo fallbacks run
    zf = rng.uniform(40, 80, m_pts)
    pc1[far] = pc1[far] * (zf[far] / pc1[far, 2])[:, None]
    pw = (pc1 - t1) @ R1
    p_oct = rng.integers(0, N_LEVELS, m_pts)

    def view(pose_k):
        """Features of the points this keyframe sees (in a random order, with clutter) and point -> feature."""
        R, t = quat_R(pose_k[:4]), pose_k[4:]
        pc = pw @ R.T + t
        u = fx * pc[:, 0] / pc[:, 2] + cx + rng.normal(0, 0.3, m_pts)
        v = fy * pc[:, 1] / pc[:, 2] + cy + rng.normal(0, 0.3, m_pts)
        seen = (pc[:, 2] > 0.5) & (u >= BOUNDS[0]) & (u < BOUNDS[2]) & (v >= BOUNDS[1]) & (v < BOUNDS[3])
        ids = np.nonzero(seen)[0]
        n = len(ids) + n_clutter
        kps = np.zeros(n, KP64)
        kps["x"] = np.concatenate([u[ids], rng.uniform(BOUNDS[0], BOUNDS[2], n_clutter)])
        kps["y"] = np.concatenate([v[ids], rng.uniform(BOUNDS[1], BOUNDS[3], n_clutter)])
        # mostly the point's level (+-1), some anything: the scale-consistency gate is hit from both sides
        octv = np.clip(p_oct[ids] + rng.integers(-1, 2, len(ids)), 0, N_LEVELS - 1)
        anyo = rng.random(len(ids)) < 0.15
        octv[anyo] = rng.integers(0, N_LEVELS, int(anyo.sum()))
        kps["octave"] = np.concatenate([octv, rng.integers(0, N_LEVELS, n_clutter)])
        kps["angle"] = rng.uniform(0, 360, n).astype(np.float32)
        z = np.concatenate([pc[ids, 2], rng.uniform(3, 60, n_clutter)])
        depth = (z * (1 + rng.normal(0, 0.02, n))).astype(np.float32)
        st = rng.random(n) < stereo_frac
        right = np.where(st, (kps["x"] - BF / depth.astype(np.float64)), -1.0).astype(np.float32)
        depth = np.where(st, depth, np.float32(-1)).astype(np.float32)
        order = rng.permutation(n)
        feat_of_point = np.full(m_pts, -1)
        inv = np.empty(n, int)
        inv[order] = np.arange(n)
        feat_of_point[ids] = inv[: len(ids)]
        has = (rng.random(n) < 0.3).astype(np.uint8)
        return dict(kps=kps[order], right_points=right[order], depth=depth[order], has_mp=has, pose=pose_k,
                    median_depth=np.float32(np.median(pc[seen, 2]))), feat_of_point

    kf1, f1 = view(pose1)
    kf2s, pairs = [], []
    for k in range(n_neighbours):
        kf2, f2 = view(pose(NEIGHBOUR_OFFSETS[k]))
        both = np.nonzero((f1 >= 0) & (f2 >= 0))[0]
        both = both[rng.random(len(both)) < 0.8]
        true = np.stack([f1[both], f2[both]], 1)
        n_wrong = len(true) // 5  # ~20 % random wrong pairs
        wrong = np.stack([rng.integers(0, len(kf1["kps"]), n_wrong), rng.integers(0, len(kf2["kps"]), n_wrong)], 1)
        # repeated idx1 / idx2: the commit pass has conflicts inside a neighbour (and idx1 repeats between neighbours anyway)
        rep = true[rng.integers(0, len(true), len(true) // 10)].copy()
        half = len(rep) // 2
        rep[:half, 1] = rng.integers(0, len(kf2["kps"]), half)
        rep[half:, 0] = rng.integers(0, len(kf1["kps"]), len(rep) - half)
        dup = true[rng.integers(0, len(true), len(true) // 20)]  # exact repeats
        p = np.concatenate([true, wrong, rep, dup])
        pairs.append(np.ascontiguousarray(p[rng.permutation(len(p))], np.int32))
        kf2s.append(kf2)
    median2 = np.array([k["median_depth"] for k in kf2s], np.float32)
    return dict(cam=cam, params=params, kf1=kf1, kf2s=kf2s, median_depth2s=median2, pairs=pairs, level_scale=ls, world=pw)


def measure_floor():
    """See POSITION_FLOOR."""
    worst = 0.0
    for seed, n_nb, mode in CASES:
        c = make_case(seed, n_nb, mode)
        res = triangulate_neighbours(c["cam"], c["params"], c["kf1"], c["kf2s"], c["median_depth2s"], c["pairs"], c["level_scale"])
        fx, fy, cx, cy, _ = c["cam"]
        R1, t1, _ = pose_parts(c["kf1"]["pose"])
        for k, rows in enumerate(res):
            R2, t2, _ = pose_parts(c["kf2s"][k]["pose"])
            for (a, b), (br, X, _, _) in zip(c["pairs"][k], rows):
                if br != TRIANGULATED:
                    continue
                k1, k2 = c["kf1"]["kps"][a], c["kf2s"][k]["kps"][b]
                p1 = ((k1["x"] - cx) / fx, (k1["y"] - cy) / fy)
                p2 = ((k2["x"] - cx) / fx, (k2["y"] - cy) / fy)
                Y = triangulate_homogeneous(R1, t1, R2, t2, p1, p2, "eigh")
                worst = max(worst, float(np.max(np.abs(X - Y) / np.maximum(1.0, np.abs(X)))))
    return worst


if __name__ == "__main__":
    import sys

    if "--floor" in sys.argv:
        print(f"POSITION_FLOOR = {measure_floor():.3e}")
