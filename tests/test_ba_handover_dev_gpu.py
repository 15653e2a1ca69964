"""GPU: snk_ba_set_problems_dev against snk_ba_set_problems.  Every case loads the same problems twice -- from host copies of the rows, and
from device tensors on a fresh handle of the same options (tests/handover_cases.py) -- and requires the same BYTES from every entry
point: cost_initial / cost_final, get_state, residuals, pcg_form, and after solve_local_scene the outlier flags and n_marked.  Both loads
feed the same lists to the same kernels, so a difference is a list difference, not a tolerance question.  The workgroup size T of the device
stage's chunks is handover_numpy.THREADS (HO_THREADS, pinned by tests/test_handover_core_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import handover_cases as HC
import handover_numpy as M

pytestmark = pytest.mark.gpu
T = M.THREADS


def _spread(s, n_obs, seed):
    """n_obs observations of the scene in a shuffled order: point 0's are in the first, the second and the third chunk (where there are
    as many), and two observations of one point stand side by side at 10 and 11."""
    rng = np.random.RandomState(seed)
    pt = np.asarray(s["obs_pt"])
    order = rng.permutation(len(pt)).tolist()
    of0, of1 = np.flatnonzero(pt == 0).tolist(), np.flatnonzero(pt == 1).tolist()
    for o in of0[:3] + of1[:2]:
        order.remove(o)
    order = order[:max(n_obs - 5, 0)]
    for at, o in ((3, of0[0]), (10, of1[0]), (11, of1[1]), (T + 7, of0[1]), (2 * T + 9, of0[2])):
        order.insert(min(at, len(order)), o)
    return HC.take_obs(s, order[:n_obs])


def test_chunk_edges():
    s, _ = HC.scene(n_kf=6, n_pt=200, obs_per_pt=4, seed=3)  # 800 observations
    sizes = (0, 1, T - 1, T, T + 1, 3 * T + 5)
    rows = [_spread(s, n, 10 + k) for k, n in enumerate(sizes)]
    assert [len(r["obs_img"]) for r in rows] == list(sizes)
    big = rows[-1]["obs_pt"]
    assert {int(x) // T for x in np.flatnonzero(big == 0)} >= {0, 1, 2} and big[10] == big[11]
    want, got, _ = HC.both_ways(rows, local_scene_of=(2, 5))
    HC.assert_same(want, got)
    for k in (4, 5):  # ... and alone, the single-problem shape
        want, got, _ = HC.both_ways(rows[k:k + 1])
        HC.assert_same(want, got)


def test_observations_that_do_not_count_are_scattered_through_the_row():
    s, _ = HC.scene(n_kf=5, n_pt=160, obs_per_pt=4, seed=4)
    rng = np.random.RandomState(2)
    s = HC.take_obs(s, rng.permutation(len(s["obs_img"])))
    s["pt_const"] = (rng.rand(160) < 0.3).astype(np.uint8)
    assert s["img_const"][0] == 1
    n = len(s["obs_img"])
    bad = rng.choice(n, 60, replace=False)
    s["obs_img"], s["obs_pt"] = s["obs_img"].copy(), s["obs_pt"].copy()
    s["obs_img"][bad[:15]], s["obs_img"][bad[15:30]] = -1, 5
    s["obs_pt"][bad[30:45]], s["obs_pt"][bad[45:]] = -1, 160
    w = M.fill(s["img_const"], s["pt_const"], s["obs_img"], s["obs_pt"])
    both_const = (s["img_const"][np.clip(s["obs_img"], 0, 4)] & s["pt_const"][np.clip(s["obs_pt"], 0, 159)]).astype(bool)
    assert w["no"] < n - 60 and both_const.sum() > 5 and n > 2 * T
    want, got, _ = HC.both_ways([s])
    HC.assert_same(want, got)
    res = np.frombuffer(dict(got)["residuals0"], np.float64)
    assert (res[w["valid"] == 0] == 0).all() and (res[w["valid"] == 1] > 0).any()


@pytest.mark.parametrize("n", [3, 17, 64])
def test_unequal_rows_in_one_batch_with_caps_far_above_the_counts(n):
    rows = HC.unequal_batch(n)
    want, got, o = HC.both_ways(rows, dict(pt_cap=100, img_cap=16, obs_cap=700), local_scene_of=(0, n - 1))
    assert o["result"]["status"][1] == 1 and o["result"]["n_obs"][1] == 0 and o["result"]["n_pt"][0] == 1
    HC.assert_same(want, got)


@pytest.mark.parametrize("nine", [False, True])
def test_256_windows_with_and_without_work_items_of_up_to_128_points(nine):
    """At most 8 free observations per point in every window: the hand-over cuts work items of up to 128 points; one point with 9 in one
    window: it does not.  Either way the decision (made from the device stage's record) and every list behind it equal the host's."""
    rows = [HC.scene(n_kf=4, n_pt=int(26 + b % 9), obs_per_pt=3, seed=500 + b)[0] for b in range(256)]
    if nine:
        s, _ = HC.scene(n_kf=10, n_pt=30, obs_per_pt=3, seed=77)
        seen = set(s["obs_img"][s["obs_pt"] == 0].tolist())
        like = int(np.flatnonzero(s["obs_pt"] == 0)[0])
        for img in range(1, 10):
            if img not in seen:
                s = HC.add_obs(s, like, img)
        assert int((s["img_const"][s["obs_img"][s["obs_pt"] == 0]] == 0).sum()) == 9
        rows[41] = s
    assert max(M.fill(r["img_const"], r["pt_const"], r["obs_img"], r["obs_pt"])["k_over8"] for r in rows) == int(nine)
    want, got, _ = HC.both_ways(rows, local_scene_of=(41,))
    HC.assert_same(want, got)


def test_a_camera_twice_on_a_point():
    rows = [HC.scene(n_kf=5, n_pt=40, obs_per_pt=3, seed=20 + b)[0] for b in range(3)]
    s = rows[1]
    like = int(np.flatnonzero(s["img_const"][s["obs_img"]] == 0)[5])
    rows[1] = HC.add_obs(s, like, int(s["obs_img"][like]))
    assert M.fill(rows[1]["img_const"], rows[1]["pt_const"], rows[1]["obs_img"], rows[1]["obs_pt"])["dup"] == 1
    want, got, _ = HC.both_ways(rows, local_scene_of=(1,))
    HC.assert_same(want, got)


def test_relative_pose_constraints():
    rows = HC.constraint_batch()
    want, got, o = HC.both_ways(rows, local_scene_of=(0, 2))
    assert o["result"]["n_rpc"].tolist() == [5, 0, 6]
    HC.assert_same(want, got)
    # the constraints count: without them the costs differ
    bare, _, _ = HC.both_ways([{k: v for k, v in r.items() if k != "rpc"} for r in rows], local_scene_of=())
    assert dict(bare)["cost_initial"] != dict(want)["cost_initial"]


def test_implicit_schur_form_takes_one_problem():
    from snake_slam_amd._lib import SnakeHipError

    s, _ = HC.scene(n_kf=6, n_pt=60, obs_per_pt=4, seed=9)
    want, got, o = HC.both_ways([s], explicit_schur=False)
    assert dict(got)["pcg_form"].startswith(b"('implicit")
    HC.assert_same(want, got)
    two = M.pad_rows([s, s])
    with pytest.raises(SnakeHipError, match="implicit Schur form takes one problem"):
        HC.load_dev(two, explicit_schur=False)
    ba, keep = HC.load_dev(o, explicit_schur=False)
    ba.solve()
    with pytest.raises(SnakeHipError, match="implicit Schur form takes one problem"):
        HC.load_dev(two, ba=ba)
    with pytest.raises(SnakeHipError, match="no problem set"):
        ba.solve()
    ba.close()


@pytest.mark.parametrize("n_pt", [M.MAX_PTS, M.MAX_PTS + 1])
def test_points_at_the_carve_limit_and_one_past_it(n_pt):
    """MAX_PTS points, two observations each: the kernels take the row.  One more: the batch is staged through the host builder."""
    s, _ = HC.scene(n_kf=4, n_pt=n_pt, obs_per_pt=2, seed=11)
    assert len(s["obs_img"]) == 2 * n_pt
    want, got, _ = HC.both_ways([s], dict(pt_cap=M.MAX_PTS + 1, img_cap=4, obs_cap=2 * M.MAX_PTS + 2))
    HC.assert_same(want, got)


def test_a_point_with_more_observations_than_the_kernels_walk_is_staged():
    s, _ = HC.scene(n_kf=5, n_pt=20, obs_per_pt=3, seed=12)
    like = int(np.flatnonzero((s["obs_pt"] == 3) & (s["img_const"][s["obs_img"]] == 0))[0])
    extra = {k: np.repeat(np.asarray(s[k])[like:like + 1], M.MAX_RUN, axis=0) for k in ("obs_img", "obs_pt", "obs_uv", "obs_depth", "obs_weight")}
    s = dict(s, **{k: np.concatenate([np.asarray(s[k]), v]) for k, v in extra.items()})
    assert M.fill(s["img_const"], s["pt_const"], s["obs_img"], s["obs_pt"])["long_run"] == 1
    want, got, _ = HC.both_ways([s, HC.scene(seed=13)[0]])
    HC.assert_same(want, got)


def test_refusals_leave_no_problem_set_and_the_handle_usable():
    from snake_slam_amd import _lib
    from snake_slam_amd._lib import SnakeHipError
    from snake_slam_amd.ba import BARec, lba_options

    rows = HC.unequal_batch(3)
    o = M.pad_rows(rows, dict(pt_cap=64, img_cap=8, obs_cap=256))
    host = HC.load_host(o)
    want = HC.collect(host, 3)
    host.close()
    ba, good = HC.load_dev(o)
    ba.solve()

    def refused(d, msg):
        with pytest.raises(SnakeHipError, match=msg) as e:
            ba.create_dev(d, HC.K, HC.BF)
        assert "failed with status 1:" in str(e.value)  # SNK_ERR_INVALID_ARG
        assert ba._scenes == []
        ci = np.zeros(3)
        assert ba._lib.snk_ba_solve(ba._h, 1, C.c_void_p(ci.ctypes.data), None) != 0
        assert "no problem set" in ba._lib.snk_last_error().decode()
        ba.create_dev(good, HC.K, HC.BF)  # a following valid call works
        ba.solve()

    assert _lib.load().snk_ba_set_problems_dev(ba._h, 3, None, (C.c_double * 4)(*HC.K), HC.BF) == 1
    for name in ("pose", "img_const", "pt", "pt_const", "obs_img", "obs_pt", "obs_uv", "obs_depth", "obs_weight", "result"):
        if name == "result":
            continue  # (the binding reads its shape; the C check is the same line as the arrays')
        refused(dict(good, **{name: None}), "NULL row arrays")
    for cap in ("win_cap", "pt_cap", "img_cap", "obs_cap"):
        refused(dict(good, **{cap: 0}), "a cap of the rows is outside its range")
    refused(dict(good, pt_cap=16385), "a cap of the rows is outside its range")
    for field, value, msg in ((3, 257, "exceeds the row's cap"), (3, -1, "negative problem size"), (1, 9, "exceeds the row's cap"),
                              (4, 5, "exceeds the row's cap")):
        res = good["result"].clone()
        res[2, field] = value
        refused(dict(good, result=res), msg)
    with pytest.raises(SnakeHipError, match="count must be"):
        ba.create_dev(dict(good, result=good["result"][:0]), HC.K, HC.BF)
    # obs_src, img_kf, pt_id, pt_valid and rpc may be absent
    ba.create_dev({k: v for k, v in good.items() if k not in ("obs_src", "img_kf", "pt_id", "pt_valid", "rpc")}, HC.K, HC.BF)
    HC.assert_same(want, HC.collect(ba, 3))
    ba.close()
    fresh = BARec(lba_options())
    with pytest.raises(SnakeHipError, match="NULL row arrays"):
        fresh.create_dev(dict(good, pose=None), HC.K, HC.BF)
    fresh.close()


def test_child_process_checks_every_array_on_poisoned_scratch_and_hands_over_twice(tmp_path):
    from handover_children import run_child

    out = tmp_path / "child.npz"
    run_child(out, SNK_BA_CHECK_LISTS="1", SNK_DEBUG_POISON="1")
    got = np.load(out)
    o17, orpc = M.pad_rows(HC.unequal_batch(17), dict(pt_cap=100, img_cap=16, obs_cap=700)), M.pad_rows(HC.constraint_batch())
    for prefix, o, n in (("first", o17, 17), ("rpc", orpc, 3), ("again", o17, 17)):
        ba = HC.load_host(o)
        want = HC.collect(ba, n)
        ba.close()
        for k, b in want:
            assert got[f"{prefix}_{k}"].tobytes() == b, (prefix, k)
