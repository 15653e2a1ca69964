"""CPU: the restatement of keyframe culling (tests/simp_numpy.py) against what is independent of it -- its spanning tree against scipy's on
negated weights, its median against np.sort -- and the fixtures of the GPU tests against the list of properties those tests are about:
every reason code, every status and every edge named in STATS_PROPERTIES / DECIDE_PROPERTIES occurs, and no verdict of the fixture hinges
on an angle within the GPU's angle bound of its threshold, so that the GPU tests compare every verdict without exclusions."""
import numpy as np
import pytest

import simp_numpy as M


@pytest.fixture(scope="module")
def fixtures():
    return M.require_coverage()


def random_graph(rng, n, n_weights, p=0.4):
    g = M.Graph(n)
    for a in range(n):
        for b in range(a + 1, n):
            if rng.rand() < p or b == a + 1:  # the path keeps it connected
                g.add_edge(a, b, int(rng.randint(1, n_weights + 1)))
    return g


def scipy_tree(g):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import minimum_spanning_tree

    rows, cols, vals = zip(*[(a, b, -w) for (a, b), w in g.w.items()])
    t = minimum_spanning_tree(csr_matrix((vals, (rows, cols)), shape=(g.n, g.n))).tocoo()
    return [(int(a), int(b), int(-w)) for a, b, w in zip(t.row, t.col, t.data)]


def test_tree_equals_scipy_on_graphs_with_ties():
    rng = np.random.RandomState(8)
    for trial in range(60):
        n = int(rng.randint(2, 40))
        g = random_graph(rng, n, n_weights=int(rng.choice([1, 3, 10])))
        mine, ref = g.build_mst(), scipy_tree(g)
        assert len(mine) == len(ref) == n - 1 and g.complete
        assert sum(w for _, _, w in mine) == sum(w for _, _, w in ref)
        assert g.weakest() == min(w for _, _, w in ref)  # the bottleneck of every maximum tree is the same: no tie rule shows in it


def test_root_degree_equals_scipy_on_graphs_with_distinct_weights():
    rng = np.random.RandomState(9)
    for trial in range(60):
        n = int(rng.randint(2, 40))
        g = random_graph(rng, n, n_weights=1)
        for i, key in enumerate(rng.permutation(len(g.w))):
            g.w[list(g.w)[key]] = i + 1  # a permutation: the tree is unique
        g.build_mst()
        ref = scipy_tree(g)
        assert sorted((min(a, b), max(a, b)) for a, b, _ in g.mst) == sorted((min(a, b), max(a, b)) for a, b, _ in ref)
        assert len(g.mst_edges_for_node(0)) == sum(0 in (a, b) for a, b, _ in ref)


def test_the_tie_rule_and_the_forest():
    g = M.Graph(5)
    for a, b in ((0, 1), (0, 2), (1, 2), (3, 4)):
        g.add_edge(a, b, 7)
    g.add_edge(1, 2, 5)  # the maximum of the weights given stays
    g.add_edge(2, 2, 99)  # no self edges
    assert g.build_mst() == [(0, 1, 7), (0, 2, 7)] and not g.complete and g.weakest() is None  # the smaller parent among equals; 3, 4 outside
    assert g.weight(1, 2) == 7 and g.weight(2, 2) is None


def test_median_equals_np_sort(fixtures):
    (t, queries, _), _, rows, _ = fixtures
    n = 0
    for q in queries:
        r = rows[(0, 300, q)]
        if r["status"] != M.OK or r["n_depth"] == 0:
            continue
        z = np.array([M.depth_of(t["kf_pose"][q], t["pt_pos"][p]) for p in t["feat_point"][t["feat_start"][q]:t["feat_start"][q + 1]] if p >= 0], np.float32)
        assert len(z) == r["n_depth"] and r["median_depth"] == np.sort(z)[(len(z) - 1) // 2]
        # row 3 of the rotation and the translation, by numpy: the stated operation order agrees with it to rounding
        zn = (M.rotation(t["kf_pose"][q]) @ t["pt_pos"][t["feat_point"][t["feat_start"][q]:t["feat_start"][q + 1]]].T)[2] + t["kf_pose"][q][6]
        assert np.allclose(np.sort(zn[t["feat_point"][t["feat_start"][q]:t["feat_start"][q + 1]] >= 0]), np.sort(z), rtol=1e-5, atol=1e-5)
        n += 1
    assert n >= 10


def test_fixtures_reach_every_reason_status_and_edge(fixtures):
    sf, df, srows, vrows = fixtures
    seen, _ = M.stats_coverage(*sf)
    assert [p for p in M.STATS_PROPERTIES if p not in seen] == []
    seen, _ = M.decide_coverage(*df)
    assert [p for p in M.DECIDE_PROPERTIES if p not in seen] == []
    reasons = {r["reason"] for rows in vrows.values() for r in rows if r["status"] == M.OK}
    assert reasons == set(range(1, 12))
    assert {r["status"] for rows in vrows.values() for r in rows} == {M.OK, M.SKIPPED, M.FEAT_OVERFLOW, M.NODES_OVERFLOW}
    assert {r["status"] for r in srows.values()} == {M.OK, M.SKIPPED, M.FEAT_OVERFLOW}  # BAD_INDEX: the device forms' own test
    assert all(r["cull"] == int(r["reason"] in M.CULLS) for rows in vrows.values() for r in rows)


def test_no_verdict_of_the_fixture_hinges_on_the_angle(fixtures):
    _, (g, queries, st, names), _, vrows = fixtures
    margins = M.angle_margins(g, queries, vrows)
    assert len(margins) >= 20 and min(margins) > 1e6 * M.ANGLE_BOUND, min(margins)
    assert M.ANGLE_BOUND == 10 * M.ANGLE_FLOOR
