"""CPU: self-checks of the numpy restatement of "snk-mp v1" (tests/mappoint_numpy.py) -- the checker of the GPU tests has to be right
about the corners of the definition before anything is compared with it."""
import numpy as np

import mappoint_numpy as M


def one_point(desc, valid=None, pose=None, position=(0.0, 0.0, 0.0), ref=-1, octave=None):
    k = len(desc)
    return dict(obs_start=np.array([0, k], np.int32), desc=np.asarray(desc, np.uint64).reshape(k, 4),
                pose=np.tile([0, 0, 0, 1, 0, 0, 0], (k, 1)).astype(np.float64) if pose is None else np.asarray(pose, np.float64).reshape(k, 7),
                octave=np.zeros(k, np.int32) if octave is None else np.asarray(octave, np.int32),
                valid=np.ones(k, np.uint8) if valid is None else np.asarray(valid, np.uint8), position=np.array([position], np.float64),
                ref_obs=np.array([ref], np.int32))


def bits(*positions):
    d = np.zeros(4, np.uint64)
    for b in positions:
        d[b // 64] |= np.uint64(1) << np.uint64(b % 64)
    return d


def test_hamming_matrix_is_the_popcount_of_the_xor():
    rng = np.random.default_rng(1)
    d = rng.integers(0, 2**64, (40, 4), dtype=np.uint64)
    want = np.array([[sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a, b)) for b in d] for a in d])
    assert np.array_equal(M.hamming_matrix(d), want)
    full = np.array([[0] * 4, [2**64 - 1] * 4], np.uint64)
    assert M.hamming_matrix(full)[0, 1] == 256


def test_single_valid_observation_is_the_best():
    rng = np.random.default_rng(2)
    d = rng.integers(0, 2**64, (5, 4), dtype=np.uint64)
    for i in range(5):
        valid = np.zeros(5, np.uint8)
        valid[i] = 1
        r = M.refresh(one_point(d, valid))[0]
        assert r["best"] == i and r["n_valid"] == 1 and np.array_equal(r["desc"], d[i])


def test_two_observations_have_median_zero_so_the_first_valid_wins():
    rng = np.random.default_rng(3)
    d = rng.integers(0, 2**64, (4, 4), dtype=np.uint64)
    assert M.refresh(one_point(d[:2]))[0]["best"] == 0
    assert M.refresh(one_point(d, [0, 1, 0, 1]))[0]["best"] == 1  # reported as an index into the full list
    assert M.refresh(one_point(d, [0, 0, 0, 0]))[0]["best"] == -1 and M.refresh(one_point(d, [0, 0, 0, 0]))[0]["n_valid"] == 0


def test_duplicate_descriptors_the_first_wins():
    rng = np.random.default_rng(4)
    d = rng.integers(0, 2**64, (9, 4), dtype=np.uint64)
    centre = d[0].copy()
    for i in range(9):  # everything within a few bits of one pattern, 3 and 6 exactly on it
        d[i] = centre ^ bits(i, 100 + i, 200 + i)
    d[3] = centre
    d[6] = centre
    for rule in (M.MEDIAN, M.SUM):
        assert M.refresh(one_point(d), rule)[0]["best"] == 3
        assert M.refresh(one_point(d, [1, 1, 1, 0, 1, 1, 1, 1, 1]), rule)[0]["best"] == 6


def test_sum_and_median_disagree_on_a_constructed_case():
    """Five observations: A sits 10 bits from B and C and 250 from the outliers D = E; B and C sit 10 from A, 20 from each other and 240
    from D, E.  Row medians (element 2 of 5): A 10, B 20, C 20, D 240 -> A; row sums: A 520, B 510, C 510, D 730 -> B."""
    z = bits()
    A = z
    B = bits(*range(0, 10))
    Cc = bits(*range(10, 20))
    D = bits(*range(0, 130), *range(136, 256))     # 250 from A
    E = D.copy()
    d = np.array([A, B, Cc, D, E])
    H = M.hamming_matrix(d)
    assert H[0, 1] == 10 and H[0, 2] == 10 and H[1, 2] == 20 and H[0, 3] == 250
    med = M.refresh(one_point(d), M.MEDIAN)[0]["best"]
    sm = M.refresh(one_point(d), M.SUM)[0]["best"]
    rows = np.sort(H, 1)[:, 2]
    assert med == int(np.argmin(rows)) == 0 and sm == int(np.argmin(H.sum(1))) and sm != med


def test_zero_length_view_vector_follows_the_s_rule():
    # camera centre of the identity pose with t = -p is p itself: v = 0, s = 0, u = v; the normal of that single observation is (0, 0, 0)
    p = (1.0, 2.0, 3.0)
    pose = [[0, 0, 0, 1, -1.0, -2.0, -3.0]]
    r = M.refresh(one_point(np.zeros((1, 4), np.uint64), pose=pose, position=p, ref=0))[0]
    assert np.all(r["normal"] == 0) and r["ref_depth"] == 0.0
    # with a second observation one unit along x the normal is exactly that direction
    pose2 = pose + [[0, 0, 0, 1, -2.0, -2.0, -3.0]]
    r = M.refresh(one_point(np.zeros((2, 4), np.uint64), pose=pose2, position=p, ref=1))[0]
    assert list(r["normal"]) == [1.0, 0.0, 0.0] and r["ref_depth"] == 1.0
    assert M.unit((0.0, 0.0, 0.0)) == ((0.0, 0.0, 0.0), 0.0)


def test_centre_is_minus_rt_t():
    rng = np.random.default_rng(5)
    pose = M.random_pose(rng, 6)
    C = M.centre(pose)
    for q, c in zip(pose, C):
        x, y, z, w = q[:4]
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        assert np.allclose(R @ c + q[4:], 0, atol=1e-12)  # the centre maps to the camera's origin


def test_what_masks_and_untouched_values():
    c = M.make_case(6, [4, 0, 7])
    full = M.refresh(c)
    for what, keep in ((M.DESCRIPTOR, ("best", "desc")), (M.NORMAL, ("normal",)), (M.DEPTH, ("ref_depth", "ref_level"))):
        r = M.refresh(c, what=what)
        blank = M.untouched(0)
        for f in ("best", "desc", "normal", "ref_depth", "ref_level"):
            for p in range(3):
                assert np.array_equal(r[f][p], full[f][p] if f in keep else blank[f]), (what, f, p)
        assert np.array_equal(r["n_valid"], full["n_valid"])
    assert full["best"][1] == -1 and full["n_valid"][1] == 0 and np.all(full["normal"][1] == 0)


def test_edge_case_holds_what_the_gpu_test_needs():
    c = M.edge_case(7, True)
    ks = np.diff(c["obs_start"])
    for k in (0, 1, 2, 3, 4, 31, 32, 33, 63, 64, 65, M.PACKED_MAX_K - 1, M.PACKED_MAX_K, M.PACKED_MAX_K + 1, M.MAX_OBS):
        assert k in ks
    run = np.flatnonzero(ks == 5)
    assert len(run) > 2 * M.CHUNK_POINTS and ks[run[-1] + 1] == 64
    assert set(c["ref_obs"][[1, 2, 3]]) == {0, -1, 2}
