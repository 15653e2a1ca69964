"""CPU: the numpy restatement of "snk-tri v1" (tests/tri_numpy.py) checked on its own -- noise-free correspondences give back the
true points, every gate of Triangulator.cpp:174-291 is hit by a constructed pair, the commit rule of :61-70 on a hand-made conflict
list, and the share of borderline pairs stays under the cap on every case the GPU tests use."""
import numpy as np
import pytest

import tri_numpy as T
from track_helpers import BF, K_EUROC

CAM = (*K_EUROC, BF)
LS = (np.float32(1.2) ** np.arange(T.N_LEVELS)).astype(np.float32)
IDENTITY = np.array([0, 0, 0, 1.0, 0, 0, 0])


def project(pose, X):
    R, t, _ = T.pose_parts(pose)
    xc = R @ np.asarray(X, np.float64) + t
    return CAM[0] * xc[0] / xc[2] + CAM[2], CAM[1] * xc[1] / xc[2] + CAM[3], xc[2]


def one_feature(pose, X, octave=0, stereo_depth=None, du=0.0, dv=0.0, dur=0.0):
    """A keyframe with the single feature that observes X (optionally displaced), mono or with a stereo depth."""
    u, v, z = project(pose, X)
    kps = np.zeros(1, T.KP64)
    kps["x"], kps["y"], kps["octave"] = u + du, v + dv, octave
    if stereo_depth is None:
        rp, dp = np.float32(-1), np.float32(-1)
    else:
        dp = np.float32(stereo_depth)
        rp = np.float32(u + du - BF / float(dp) + dur)
    return dict(kps=kps, right_points=np.array([rp], np.float32), depth=np.array([dp], np.float32), has_mp=np.zeros(1, np.uint8),
                pose=np.asarray(pose, np.float64))


SIDE = np.array([0, 0, 0, 1.0, -0.6, 0, 0])     # camera 0.6 m to the right
FORWARD = np.array([0, 0, 0, 1.0, 0, 0, -0.5])  # camera 0.5 m ahead: no parallax on the optical axis
X_NEAR = np.array([0.5, 0.2, 6.0])
X_AXIS = np.array([0.0, 0.0, 6.0])


def run(kf1, kf2):
    why = []
    br, X, far, mg = T.tri_pair(CAM, T.PARAMS, kf1, kf2, 0, 0, LS, why)
    return br, X, far, (why[0] if why else None)


def test_noise_free_correspondences_reproduce_the_points():
    rng = np.random.default_rng(0)
    for pose2 in (SIDE, np.array([0.01, -0.02, 0.005, 1.0, 0.3, 0.1, 0.05])):
        pose2 = pose2.copy()
        pose2[:4] /= np.linalg.norm(pose2[:4])
        for _ in range(50):
            X = np.array([rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(3, 9)])
            br, Y, far, why = run(one_feature(IDENTITY, X), one_feature(pose2, X))
            assert br == T.TRIANGULATED and not far, why
            assert np.max(np.abs(Y - X)) < 1e-9


def test_each_gate_is_hit_by_a_constructed_pair():
    # the pair as it should be: triangulated, mono and stereo
    assert run(one_feature(IDENTITY, X_NEAR), one_feature(SIDE, X_NEAR))[0] == T.TRIANGULATED
    assert run(one_feature(IDENTITY, X_NEAR, stereo_depth=6.0), one_feature(SIDE, X_NEAR, stereo_depth=6.0))[0] == T.TRIANGULATED
    # rays that meet behind the cameras: the second view's feature moved the wrong way by more than the disparity
    u1, _, _ = project(IDENTITY, X_NEAR)
    u2, _, _ = project(SIDE, X_NEAR)
    assert run(one_feature(IDENTITY, X_NEAR), one_feature(SIDE, X_NEAR, du=2 * (u1 - u2)))[3] == "behind"
    # chi-square, mono: 6 px off the epipolar line leaves 3 px in each view, 9 > 2.1^2
    assert run(one_feature(IDENTITY, X_NEAR), one_feature(SIDE, X_NEAR, dv=6.0))[3] in ("chi2_mono_1", "chi2_mono_2")
    # chi-square, stereo: the right coordinate 3 px off in keyframe 1 / keyframe 2, 9 > 2.3^2
    assert run(one_feature(IDENTITY, X_NEAR, stereo_depth=6.0, dur=3.0), one_feature(SIDE, X_NEAR))[3] == "chi2_stereo_1"
    assert run(one_feature(IDENTITY, X_NEAR), one_feature(SIDE, X_NEAR, stereo_depth=6.0, dur=3.0))[3] == "chi2_stereo_2"
    # scale consistency from both sides: the distances are equal, the octaves seven levels apart
    assert run(one_feature(IDENTITY, X_NEAR, octave=7), one_feature(SIDE, X_NEAR, octave=0))[3] == "scale_low"
    assert run(one_feature(IDENTITY, X_NEAR, octave=0), one_feature(SIDE, X_NEAR, octave=7))[3] == "scale_high"
    # no parallax (forward motion, point on the axis): the stereo depth of keyframe 1, then of keyframe 2, makes the point
    br, X, far, _ = run(one_feature(IDENTITY, X_AXIS, stereo_depth=6.0), one_feature(FORWARD, X_AXIS))
    assert br == T.STEREO1 and not far and np.allclose(X, X_AXIS, atol=1e-5)
    br, X, far, _ = run(one_feature(IDENTITY, X_AXIS), one_feature(FORWARD, X_AXIS, stereo_depth=5.5))
    assert br == T.STEREO2 and not far and np.allclose(X, X_AXIS, atol=1e-5)
    # the same beyond th_depth: far_away
    Xf = np.array([0.0, 0.0, 50.0])
    br, X, far, _ = run(one_feature(IDENTITY, Xf, stereo_depth=50.0), one_feature(FORWARD, Xf))
    assert br == T.STEREO1 and far
    br, X, far, _ = run(one_feature(IDENTITY, Xf), one_feature(FORWARD, Xf, stereo_depth=49.5))
    assert br == T.STEREO2 and far
    # and without any stereo depth: the `else -> continue`
    assert run(one_feature(IDENTITY, X_AXIS), one_feature(FORWARD, X_AXIS))[3] == "parallax"


def test_baseline_gate_per_neighbour():
    kf = lambda tx: dict(pose=np.array([0, 0, 0, 1.0, tx, 0, 0]))
    stereo, mono = dict(T.PARAMS, mono=0), dict(T.PARAMS, mono=1)
    b = BF / K_EUROC[0]
    assert T.neighbour_skipped(CAM, stereo, kf(0), kf(0.9 * b), 6.0)[0] and not T.neighbour_skipped(CAM, stereo, kf(0), kf(1.1 * b), 6.0)[0]
    assert T.neighbour_skipped(CAM, mono, kf(0), kf(0.05), 6.0)[0] and not T.neighbour_skipped(CAM, mono, kf(0), kf(0.07), 6.0)[0]


def test_commit_rule_on_a_hand_made_conflict_list():
    has1 = [0, 0, 1, 0, 0]
    has2s = [[0, 0, 0, 1], [0, 0, 0, 0]]
    entries = [(0, 0, 0),  # kept
               (0, 0, 1),  # feature 0 of keyframe 1 was used by the entry above
               (0, 1, 0),  # feature 0 of neighbour 0 was used
               (0, 2, 2),  # keyframe-1 feature 2 already had a point
               (0, 3, 3),  # neighbour-0 feature 3 already had a point
               (0, 3, 1),  # kept: the entry above was NOT kept, so feature 3 is still free
               (1, 3, 0),  # feature 3 of keyframe 1 is used now (by a point of neighbour 0)
               (1, 4, 1),  # kept: feature 1 of neighbour 1 is another feature than feature 1 of neighbour 0
               (1, 1, 1),  # feature 1 of neighbour 1 was used
               (1, 1, 2)]  # kept
    assert T.commit_pass(entries, has1, has2s) == [True, False, False, False, False, True, False, True, False, True]


@pytest.mark.parametrize("seed,n_nb,mode", T.CASES)
def test_borderline_pairs_stay_under_the_cap(seed, n_nb, mode):
    """What the GPU test leaves out of the decision comparison is at most 1 % of a case; the cases are what they say they are."""
    c = T.make_case(seed, n_nb, mode)
    res = T.triangulate_neighbours(c["cam"], c["params"], c["kf1"], c["kf2s"], c["median_depth2s"], c["pairs"], c["level_scale"])
    rows = [r for rs in res for r in rs]
    borderline = sum(r[3] < T.BORDERLINE for r in rows)
    print(f"case {seed}/{n_nb}/{mode}: {len(rows)} pairs, {borderline} borderline")
    assert len(rows) > 1500 and borderline <= T.BORDERLINE_CAP * len(rows)
    skipped = [T.neighbour_skipped(c["cam"], c["params"], c["kf1"], k2, m)[0] for k2, m in zip(c["kf2s"], c["median_depth2s"])]
    assert any(skipped) and not all(skipped)
    branches = np.bincount([r[0] for r in rows], minlength=4)
    assert branches[T.REJECT] > 100 and branches[T.TRIANGULATED] > 100
    if mode == "mono":
        assert branches[T.STEREO1] == branches[T.STEREO2] == 0
    else:
        assert branches[T.STEREO1] > 10 and any(r[2] for r in rows)
    if mode == "mixed":
        assert branches[T.STEREO2] > 5
    # conflicts for the commit pass: repeated features among the accepted entries
    ent = [(k, int(a), int(b)) for k, rs in enumerate(res) for (a, b), r in zip(c["pairs"][k], rs) if r[0]]
    kept = T.commit_pass(ent, c["kf1"]["has_mp"], [k2["has_mp"] for k2 in c["kf2s"]])
    assert 0 < sum(kept) < len(kept)


def test_position_floor_constant_is_the_measured_one():
    """POSITION_FLOOR is a measurement (SVD of A against eigh of A^T A on the test inputs), not a choice: the same order of magnitude
    must come out again."""
    got = T.measure_floor()
    print(f"measured floor {got:.3e}, stored {T.POSITION_FLOOR:.3e}, tolerance {T.position_tolerance():.3e}")
    assert T.POSITION_FLOOR / 10 <= got <= T.POSITION_FLOOR * 10
    assert T.position_tolerance() <= T.BA_BOUND
