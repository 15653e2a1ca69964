"""GPU: snk_pgo_* (pgo.hip) against the numpy restatement of snk-pgo v1 (tests/pgo_numpy.py) on the smallest graphs at which each part
can go wrong, in the se3 and the sim3 form: the linearisation at the start state (<= 1e-10 relative), the optimum within
pose_tolerance() (10 x the floor measured against scipy.optimize.least_squares, tests/test_pgo_numpy.py), constant and isolated vertices
bit for bit, determinism, the resident (one cooperative launch) and the multi-launch PCG on the same graph, the map-point pass and the
argument checks of snk_pgo_set_graph.

Cost tolerance: |cost_final - restatement's| <= pose_tolerance() x max(restatement's cost_final, pose_tolerance() x cost_initial), the
relative tolerance that matches the pose check: the cost is stationary at the optimum, so pose differences d move it by about |H| d^2,
far less than the fraction d of the cost.  The floor serves the graphs whose optimum is zero (line3: 1.9e-21), where a relative figure
means nothing: there the cost is |J dx|^2, second order in the pose difference, hence pose_tolerance()^2 of the cost scale."""
import functools

import numpy as np
import pytest

import pgo_numpy as P

pytestmark = pytest.mark.gpu

BUILDERS = {
    "line3": lambda f: P.line3(1, f),
    "loop8": lambda f: P.correct_loop(8, 2, f),
    "ring40x3": lambda f: P.ring(40, 3, 3, f),
    "hub70": lambda f: P.hub(70, 4, f),
    "isolated": lambda f: P.with_isolated(P.ring(12, 2, 5, f), 6),
    "ring300x6": lambda f: P.ring(300, 6, 7, f),
}
BIG = {"ring4000x8": lambda f: P.ring(4000, 8, 9, f)}
ROWS_300 = "100"  # SNK_PGO_ROWS_PER_WG for ring300x6: 299 free rows over at least 3 workgroups (12: LDS holds 26 rows of this degree); neighbours 1..6 cross every boundary


@functools.lru_cache(maxsize=None)
def graph(name, fix):
    return P.prepare((BUILDERS.get(name) or BIG[name])(fix))


@functools.lru_cache(maxsize=None)
def reference(name, fix, max_iterations=P.MAX_ITERATIONS):
    return P.optimise(graph(name, fix), max_iterations=max_iterations)


def make(G, **opt):
    from snake_slam_amd.loop import PoseGraphOptimizer, pgo_options

    o = PoseGraphOptimizer(pgo_options(**opt))
    o.set_graph(G["poses_measure"], G["constant"], G["edges"], G.get("weights"), G.get("measurements"), G.get("poses_init"), G["fix_scale"])
    return o


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if b.size else 0.0


def check_solution(G, poses, res, want, info):
    tol = P.pose_tolerance()
    d = P.pose_distance(poses, want)
    print(f"{G['name']} fix_scale={G['fix_scale']}: cost {res['cost_initial']:.6e} -> {res['cost_final']:.6e} (restatement {info['cost_final']:.6e}), "
          f"LM {res['lm_iterations']} / {info['lm_iterations']}, PCG iterations {res['pcg_iterations_total']}, form {res['pcg_form']} on "
          f"{res['workgroups']} workgroups, pose difference {d:.2e}")
    assert res["cost_final"] <= res["cost_initial"]
    assert d <= tol
    dc = abs(res["cost_final"] - info["cost_final"])
    print(f"  cost difference {dc:.2e} = {dc / max(info['cost_final'], 1e-300):.2e} of cost_final; most PCG iterations in one solve {res['pcg_iterations_max']}")
    assert dc <= tol * max(info["cost_final"], tol * info["cost_initial"])
    const = G["constant"] == 1
    assert np.array_equal(poses[const].view(np.uint64), G["start"][const].view(np.uint64)), "constant vertices are bit-identical to their input"
    assert np.abs(np.linalg.norm(poses[:, :4], axis=1) - 1.0).max() <= 1e-14
    if G["fix_scale"]:
        assert np.all(poses[:, 7] == 1.0)


@pytest.mark.parametrize("fix", [1, 0], ids=["se3", "sim3"])
@pytest.mark.parametrize("name", list(BUILDERS))
def test_linearisation_and_optimum(name, fix, monkeypatch):
    G = graph(name, fix)
    if name == "ring300x6":
        monkeypatch.setenv("SNK_PGO_ROWS_PER_WG", ROWS_300)
    if not fix:
        assert np.any(G["start"][:, 7] != 1.0), "the sim3 form carries scales other than 1"
    o = make(G)
    try:
        r, g, d = o.debug_linearisation()
        wr, wg, wd, _ = P.linearise(G, G["start"])
        for what, a, b in (("residuals", r, wr), ("gradient", g, wg), ("diagonal blocks", d, wd)):
            print(f"{name} {what}: {rel(a, b):.2e}")
            assert rel(a, b) <= 1e-10, what
        c0 = P.cost(G, G["start"])
        assert abs(o.cost() - c0) <= 1e-10 * c0
        res = o.solve()
        assert abs(res["cost_initial"] - c0) <= 1e-10 * c0
        poses = o.poses()
        want, info = reference(name, fix)
        check_solution(G, poses, res, want, info)
        assert abs(o.cost() - res["cost_final"]) <= 1e-12 * max(res["cost_final"], 1e-300) or o.cost() == res["cost_final"]
        assert res["pcg_form"] == 1, "small graphs take the resident PCG"
        assert res["pcg_iterations_max"] < o.options.max_pcg_iterations, "every solve stops on pcg_tol, not at the cap"
        if name == "ring300x6":
            assert res["workgroups"] >= 3
        if name == "isolated":
            assert np.array_equal(poses[-1].view(np.uint64), G["start"][-1].view(np.uint64)), "a free vertex without edges keeps its pose"
        if name == "loop8":
            assert G["constant"].sum() == 2 and not np.array_equal(G["start"][7], G["poses_measure"][7])
        # the same input again: identical bytes
        o.set_graph(G["poses_measure"], G["constant"], G["edges"], G["weights"], G["meas"], G["start"], G["fix_scale"])
        res2 = o.solve()
        assert res2 == res and o.poses().tobytes() == poses.tobytes()
    finally:
        o.close()


@pytest.mark.parametrize("fix", [1, 0], ids=["se3", "sim3"])
def test_multi_launch_fallback_agrees_with_the_resident_form(fix, monkeypatch):
    G = graph("ring300x6", fix)
    monkeypatch.setenv("SNK_PGO_ROWS_PER_WG", ROWS_300)
    a = make(G)
    monkeypatch.setenv("SNK_PGO_PCG_LAUNCHES", "1")
    b = make(G)
    try:
        rb = b.solve()
        pb = b.poses()
        monkeypatch.delenv("SNK_PGO_PCG_LAUNCHES")
        ra = a.solve()
        pa = a.poses()
        assert ra["pcg_form"] == 1 and rb["pcg_form"] == 2 and rb["workgroups"] >= 3
        want, info = reference("ring300x6", fix)
        check_solution(G, pb, rb, want, info)
        d = P.pose_distance(pa, pb)
        print(f"resident against multi-launch: {d:.2e}; PCG iterations {ra['pcg_iterations_total']} / {rb['pcg_iterations_total']}")
        assert d <= P.pose_tolerance()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("fix", [1, 0], ids=["se3", "sim3"])
def test_degenerate_graphs(fix):
    G = graph("ring40x3", fix)
    const = np.ones(len(G["constant"]), np.uint8)
    o = make(dict(G, constant=const))
    try:
        res = o.solve()
        assert res["lm_iterations"] == 0 and res["pcg_form"] == 0 and res["cost_final"] == res["cost_initial"] > 0
        assert o.poses().tobytes() == G["start"].tobytes(), "an all-constant graph leaves the poses untouched"
        o.set_graph(G["poses_measure"], G["constant"], np.zeros((0, 2), np.int32), None, None, G["start"], fix)
        res = o.solve()
        assert res["lm_iterations"] == 0 and res["cost_initial"] == 0.0 and o.poses().tobytes() == G["start"].tobytes()
        o.set_graph(np.zeros((0, 8)), np.zeros(0, np.uint8), np.zeros((0, 2), np.int32), None, None, None, fix)
        assert o.solve()["lm_iterations"] == 0 and o.poses().shape == (0, 8)
        # gauge freedom: every vertex free, the undamped system is singular -- the cost goes down and the poses stay finite
        free = np.zeros(len(G["constant"]), np.uint8)
        o.set_graph(G["poses_measure"], free, G["edges"], G["weights"], G["meas"], G["start"], fix)
        res = o.solve()
        assert res["cost_final"] < res["cost_initial"] and np.isfinite(o.poses()).all() and res["accepted_steps"] >= 1
    finally:
        o.close()


@pytest.mark.parametrize("fix", [1, 0], ids=["se3", "sim3"])
@pytest.mark.parametrize("rows", [None, "1"], ids=["resident", "launches"])
def test_map_sized_graph_after_two_iterations(fix, rows, monkeypatch):
    """4 000 vertices x 8 neighbours, max_iterations = 2, default options otherwise: the path a full-size map takes (one workgroup per
    compute unit), and with one row per workgroup (4 000 workgroups) more than the device holds at once, i.e. the multi-launch form.

    The state after two LM iterations is not an optimum: it is two linear solves, so this case compares the PCG at its default pcg_tol
    with the restatement's direct solve, within pose_tolerance().  No solve may end at the cap."""
    name = "ring4000x8"
    G = graph(name, fix)
    if rows:
        monkeypatch.setenv("SNK_PGO_ROWS_PER_WG", rows)
    o = make(G, max_iterations=2)
    try:
        res = o.solve()
        want, info = reference(name, fix, 2)
        check_solution(G, o.poses(), res, want, info)
        assert res["lm_iterations"] == info["lm_iterations"] == 2
        assert res["pcg_form"] == (2 if rows else 1), res
        assert 0 < res["pcg_iterations_max"] < o.options.max_pcg_iterations, "every solve stops on pcg_tol, not at the cap"
    finally:
        o.close()


def test_transform_points():
    G = graph("loop8", 0)
    o = make(G)
    try:
        o.solve()
        after = o.poses()
        rng = np.random.default_rng(8)
        n = 1000
        ref = rng.integers(-1, 8, n).astype(np.int32)
        ref[:3] = [-1, 0, 3]  # no reference, a constant vertex, a free one
        assert np.any(np.abs(after[ref[ref >= 0], 7] / G["poses_measure"][ref[ref >= 0], 7] - 1) > 1e-6), "a scaled vertex is among the references"
        pos, nrm, dep = rng.standard_normal((n, 3)) * 5, rng.standard_normal((n, 3)), 1 + rng.random(n)
        gp, gn, gd = o.transform_points(ref, pos, nrm, dep)
        wp, wn, wd = P.transform_points(G["poses_measure"], after, G["constant"], ref, pos, nrm, dep)
        for a, b in ((gp, wp), (gn, wn), (gd, wd)):
            assert rel(a, b) <= 1e-12
        still = (ref < 0) | (G["constant"][np.maximum(ref, 0)] == 1)
        assert still.sum() > 10 and np.array_equal(gp[still], pos[still]) and np.array_equal(gn[still], nrm[still]) and np.array_equal(gd[still], dep[still])
        gp2, _, _ = o.transform_points(ref, pos)
        assert np.array_equal(gp2, gp)
    finally:
        o.close()


def test_set_graph_refuses_bad_input_and_leaves_the_handle_usable():
    from snake_slam_amd import SnakeHipError

    G = graph("loop8", 1)
    o = make(G)
    try:
        E = G["edges"]
        scaled = G["poses_measure"].copy()
        scaled[2, 7] = 1.5
        bad = [
            ("i >= j", dict(edges=np.concatenate([E, [[5, 5]]]))),
            ("i > j", dict(edges=np.concatenate([E[:-1], [[7, 6]]]))),
            ("duplicate", dict(edges=np.concatenate([E[:1], E]))),
            ("unsorted", dict(edges=E[::-1])),
            ("out of range", dict(edges=np.concatenate([E, [[7, 8]]]))),
            ("negative index", dict(edges=np.concatenate([[[-1, 2]], E]))),
            ("scale with fix_scale", dict(poses_measure=scaled)),
        ]
        for what, ch in bad:
            g = dict(G, weights=None, measurements=None, **ch)
            with pytest.raises(SnakeHipError, match="invalid argument"):
                o.set_graph(g["poses_measure"], g["constant"], g["edges"], None, None, None, 1)
            assert o.poses().shape == (8, 8)  # a refused call changes nothing: the handle keeps the graph it had
            o.set_graph(G["poses_measure"], G["constant"], G["edges"], G["weights"], G["meas"], G["start"], 1)
            res = o.solve()
            assert P.pose_distance(o.poses(), reference("loop8", 1)[0]) <= P.pose_tolerance(), what
        neg = G["poses_measure"].copy()
        neg[1, 7] = -1.0
        with pytest.raises(SnakeHipError, match="scale"):
            o.set_graph(neg, G["constant"], E, None, None, None, 0)
    finally:
        o.close()
