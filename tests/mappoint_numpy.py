"""numpy restatement of "snk-mp v1" (DESIGN.md section 3h): MapPoint::ComputeDistinctiveDescriptors, UpdateNormal and UpdateDepth
(reference Snake/Map/MapPoint.cpp:60-81, :120-135, :154-166) for a list of points, written from the definition:

* the median of a row of the distance matrix is taken from the row actually SORTED (element (N - 1) // 2), so the kernels' selection by
  halving is checked against the literal rule;
* every fp64 expression has the order of snake_slam_amd/csrc/mappoint_core.hpp and is evaluated one IEEE operation at a time
  (numpy elementwise operations and Python floats do not contract), so the doubles are compared bit for bit;
* the normal is summed one observation after the other, in list order.
"""
import math

import numpy as np

MAX_OBS = 4096
MEDIAN, SUM = 0, 1
DESCRIPTOR, NORMAL, DEPTH = 1, 2, 4
ALL = DESCRIPTOR | NORMAL | DEPTH
OK, BAD_INDEX, TOO_MANY = 0, 1, 2
PACKED_MAX_K = 32  # dispatch.hpp MP_PACKED_MAX_K: the last k of the packed form (tests/test_mappoint_core_cpu.py pins it)
CHUNK_POINTS = 64  # dispatch.hpp MP_CHUNK_POINTS

RESULT = np.dtype([("best", "<i4"), ("n_valid", "<i4"), ("ref_level", "<i4"), ("status", "<i4"), ("normal", "<f8", 3), ("ref_depth", "<f8"),
                   ("desc", "<u8", 4)])
assert RESULT.itemsize == 80


def hamming_matrix(desc):
    """[n, n] Hamming distances of [n, 4] uint64 descriptors (exact: bit products summed in float32 stay below 2^24)."""
    bits = np.unpackbits(np.ascontiguousarray(desc, "<u8").view(np.uint8).reshape(len(desc), 32), axis=1).astype(np.float32)
    ones = bits.sum(1)
    return (ones[:, None] + ones[None, :] - 2.0 * (bits @ bits.T)).astype(np.int32)


def centre(pose):
    """C = -R^T t of poses [..., 7] (qx qy qz qw tx ty tz, world -> camera), expression order of mp_centre."""
    pose = np.asarray(pose, np.float64)
    x, y, z, w, tx, ty, tz = (pose[..., i] for i in range(7))
    r00, r01, r02 = 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)
    r10, r11, r12 = 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)
    r20, r21, r22 = 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)
    return np.stack([-((r00 * tx + r10 * ty) + r20 * tz), -((r01 * tx + r11 * ty) + r21 * tz), -((r02 * tx + r12 * ty) + r22 * tz)], -1)


def unit(v):
    """(u, s) of mp_unit for one vector: u = s > 0 ? v / sqrt(s) : v, component by component."""
    x, y, z = (float(a) for a in v)
    s = (x * x + y * y) + z * z
    if s > 0:
        r = math.sqrt(s)
        return (x / r, y / r, z / r), s
    return (x, y, z), s


def best_descriptor(desc, valid, rule=MEDIAN):
    """(best, N): best as an index into the full list, -1 without a valid observation."""
    vi = np.flatnonzero(np.asarray(valid) != 0)
    N = len(vi)
    if N == 0:
        return -1, 0
    D = hamming_matrix(np.asarray(desc)[vi])
    m = D.sum(1, dtype=np.int64) if rule == SUM else np.sort(D, axis=1)[:, (N - 1) // 2]
    return int(vi[int(np.argmin(m))]), N  # argmin: the first smallest


def normal(pose, valid, position):
    acc = [0.0, 0.0, 0.0]
    C = centre(pose).reshape(-1, 3)
    p = [float(a) for a in position]
    for j in np.flatnonzero(np.asarray(valid) != 0):
        u, _ = unit((C[j, 0] - p[0], C[j, 1] - p[1], C[j, 2] - p[2]))
        acc = [acc[0] + u[0], acc[1] + u[1], acc[2] + u[2]]
    return unit(acc)[0]


def ref_depth(pose, position):
    C = centre(pose)
    p = [float(a) for a in position]
    return math.sqrt(unit((p[0] - C[0], p[1] - C[1], p[2] - C[2]))[1])


def refresh(case, rule=MEDIAN, what=ALL):
    """The host call shape: case = dict(obs_start [n + 1], desc [n_obs, 4] uint64, pose [n_obs, 7], octave [n_obs], valid [n_obs],
    position [n, 3], ref_obs [n]).  Returns RESULT records."""
    start = np.asarray(case["obs_start"])
    out = np.zeros(len(start) - 1, RESULT)
    out["best"], out["ref_level"] = -1, -1
    for p in range(len(out)):
        a, b = int(start[p]), int(start[p + 1])
        valid = case["valid"][a:b]
        out["n_valid"][p] = int(np.count_nonzero(valid))
        if what & DESCRIPTOR:
            best, _ = best_descriptor(case["desc"][a:b], valid, rule)
            if best >= 0:
                out["best"][p], out["desc"][p] = best, case["desc"][a + best]
        if what & NORMAL:
            out["normal"][p] = normal(case["pose"][a:b], valid, case["position"][p])
        r = int(case["ref_obs"][p])
        if (what & DEPTH) and r >= 0:
            out["ref_depth"][p] = ref_depth(case["pose"][a + r], case["position"][p])
            out["ref_level"][p] = case["octave"][a + r]
    return out


def untouched(status):
    r = np.zeros((), RESULT)
    r["best"], r["ref_level"], r["status"] = -1, -1, status
    return r


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def random_pose(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.concatenate([q, rng.uniform(-5, 5, (n, 3))], 1)


def descriptors(rng, n, near_tie):
    """near_tie: one base pattern with <= 8 flipped bits each, so that many rows of a point share a median and first-wins decides."""
    if not near_tie:
        return rng.integers(0, 2**64, (n, 4), dtype=np.uint64)
    base = rng.integers(0, 2**64, 4, dtype=np.uint64)
    out = np.tile(base, (n, 1))
    for i in range(n):
        for b in rng.integers(0, 256, int(rng.integers(0, 9))):
            out[i, b // 64] ^= np.uint64(1) << np.uint64(b % 64)
    return out


def make_case(seed, ks, near_tie=False, invalid_frac=0.0):
    """Points with the observation counts `ks`; every point's descriptors are drawn on their own."""
    rng = np.random.default_rng(seed)
    ks = [int(k) for k in ks]
    start = np.concatenate([[0], np.cumsum(ks)]).astype(np.int32)
    n_obs = int(start[-1])
    desc = np.concatenate([descriptors(rng, k, near_tie) for k in ks] + [np.zeros((0, 4), np.uint64)])
    valid = (rng.random(n_obs) >= invalid_frac).astype(np.uint8)
    ref = np.array([int(rng.integers(-1, k)) if k else -1 for k in ks], np.int32)
    return dict(obs_start=start, desc=desc, pose=random_pose(rng, n_obs), octave=rng.integers(0, 8, n_obs).astype(np.int32), valid=valid,
                position=rng.uniform(-3, 3, (len(ks), 3)), ref_obs=ref)


def point_slice(case, p):
    return slice(int(case["obs_start"][p]), int(case["obs_start"][p + 1]))


EDGE_KS = [0, 1, 2, 3, 4, 31, 32, 33, 63, 64, 65, PACKED_MAX_K - 1, PACKED_MAX_K, PACKED_MAX_K + 1]


def edge_case(seed, near_tie):
    """The k of the issue (threshold - 1 / exact / + 1 and SNK_MP_MAX_OBS included), invalid observations at the first, the last and an
    interior position, a point without a valid one, a tie between two identical descriptors, ref_obs -1 / first / last; then a run of
    k = 5 points longer than one workgroup chunk followed by one k = 64 point."""
    ks = EDGE_KS + [6, 7, 9, 12, 5, 40, MAX_OBS] + [5] * (2 * CHUNK_POINTS + 9) + [64]
    c = make_case(seed, ks, near_tie)
    s = lambda p: point_slice(c, p)
    base = len(EDGE_KS)
    c["valid"][s(base)][0] = 0          # k = 6: the first
    c["valid"][s(base + 1)][-1] = 0     # k = 7: the last
    c["valid"][s(base + 2)][4] = 0      # k = 9: an interior one
    c["valid"][s(base + 3)][:] = 0      # k = 12: none valid
    c["valid"][s(base + 5)][[0, 17, 39]] = 0  # k = 40 (wide): first, interior, last
    c["valid"][s(base + 6)][[0, 1000, MAX_OBS - 1]] = 0
    d = c["desc"][s(8)]                 # k = 63: observations 7 and 40 identical, and closest to all the others
    d[40] = d[7]
    d = c["desc"][s(5)]                 # k = 31: 3 and 20
    d[20] = d[3]
    c["ref_obs"][[1, 2, 3]] = [0, -1, 2]          # k = 1: first (= last); k = 2: none; k = 3: last
    c["ref_obs"][[9, 10]] = [0, 64]               # k = 64: first; k = 65: last
    c["ref_obs"][base + 6] = MAX_OBS - 1
    c["ref_obs"][base + 3] = 5                    # the reference observation of the all-invalid point is still read
    return c
