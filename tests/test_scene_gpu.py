"""GPU: snk_scene_window / snk_scene_gather and their _batch_dev forms ("snk-scene v1") against the restatement of
tests/scene_numpy.py -- every window, every result word, every byte of every output row up to its count, the -1 fill of pt_id, the fill
pattern behind every count and a guard row on either side of every device array: the results are integers and copied or singly rounded
values, so there is nothing to tolerate.

The map is scene_numpy.build_map (120 keyframes, 64 features each, 3 080 points), whose builder raises unless it holds every property
listed in scene_numpy.PROPERTIES, and scene_numpy.long_range_map (a window keyframe of 65 540 features); then every overflow status met at its cap and one above, the device forms' BAD_INDEX answers with the
other sets of the batch unharmed, the table limits (32 768 keyframe slots, pt_cap 16 384, img_cap 4 096), two runs of one batch byte for
byte, and two batches of different sizes on one handle in a child under SNK_DEBUG_POISON=1."""
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import scene_numpy as M

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FILL = 0xA5  # the byte of rows that nothing may write
GYRO, ACC = 2.0, 0.5
CAPS = dict(win_cap=36, pt_cap=1024, img_cap=128, obs_cap=4096)
COUNT_OF = dict(img_kf="n_img", pose="n_img", img_const="n_img", pt_id="n_pt", pt="n_pt", pt_const="n_pt", pt_valid="n_pt", obs_img="n_obs",
                obs_pt="n_obs", obs_uv="n_obs", obs_depth="n_obs", obs_weight="n_obs", obs_src="n_obs", rpc="n_rpc")


@functools.lru_cache(maxsize=None)
def the_map():
    t = M.build_map()
    M.require_coverage(t, gyro_weight=GYRO, acc_weight=ACC)
    return t


def want(t, queries, caps, **params):
    return [M.local_scene(t, q, win_cap=caps["win_cap"], pt_cap=caps["pt_cap"], img_cap=caps["img_cap"], obs_cap=caps["obs_cap"],
                          gyro_weight=GYRO, acc_weight=ACC, **params) for q in queries]


def builder(caps, **params):
    from snake_slam_amd.scene import LocalSceneBuilder

    p = dict(win_cap=caps["win_cap"], gyro_weight=GYRO, acc_weight=ACC)
    p.update(params)
    return LocalSceneBuilder(p)


def check_window(win, res, expected, win_cap):
    for s, (kfs, sc) in enumerate(expected):
        st = sc["status"] if sc["status"] in (M.SKIPPED, M.WINDOW_OVERFLOW) else M.OK
        assert (int(res[s]["n_window"]), int(res[s]["status"])) == (len(kfs) if st == M.OK else 0, st), s
        row = np.full(win_cap, -1, np.int32)
        if st == M.OK:
            row[:len(kfs)] = kfs
        assert np.array_equal(win[s], row), s


def check_rows(o, expected):
    """Every row up to its count equals the restatement byte for byte; behind it the fill stands (pt_id: -1)."""
    for s, (_, sc) in enumerate(expected):
        got = tuple(int(o["result"][s][k]) for k in ("n_window", "n_img", "n_pt", "n_obs", "n_rpc", "status"))
        assert got == tuple(sc[k] for k in ("n_window", "n_img", "n_pt", "n_obs", "n_rpc", "status")), (s, got)
        for name, count in COUNT_OF.items():
            n = sc[count]
            row = np.ascontiguousarray(o[name][s])
            if n:
                assert row[:n].tobytes() == np.ascontiguousarray(sc[name]).tobytes(), (s, name)
            rest = row[n:]
            if name == "pt_id":
                assert (rest == -1).all(), (s, name)
            else:
                assert (rest.view(np.uint8) == FILL).all(), (s, name, "written behind its count")


def run_host(t, queries, caps, **params):
    from snake_slam_amd import scene as S

    b = builder(caps, **params)
    win, res = b.window(queries, t["kf_bad"], t["kf_prev"], t["conn_start"], t["conn_list"])
    o = S.host_outputs(len(queries), fill=FILL, **caps)
    b.gather(t, win, res, caps["pt_cap"], caps["img_cap"], caps["obs_cap"], out=o)
    return win, res, o


def to_dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype.fields:
        return torch.from_numpy(a.view(np.uint8).reshape(a.shape + (-1,))).cuda()
    return torch.from_numpy(a).cuda()


def dev_tables(t):
    from snake_slam_amd import scene as S

    d = {n: to_dev(np.ascontiguousarray(t[n], dt)) for n, dt, _ in S.MAP_TABLES if t.get(n) is not None}
    d["conn_start"] = to_dev(t["conn_start"])
    d["conn_list"] = to_dev(np.stack([t["conn_list"]["weight"], t["conn_list"]["kf"]], axis=1).astype(np.int32).reshape(-1, 2))
    return d


def run_dev(t, queries, caps, b=None, d=None, window_edit=None, **params):
    """The device forms on tensors with a guard row of the fill pattern before and behind every array.  Returns numpy copies and the
    whole tensors' bytes."""
    import torch
    from snake_slam_amd import scene as S

    b = b or builder(caps, **params)
    d = d or dev_tables(t)
    n = len(queries)
    q = to_dev(np.asarray(queries, np.int32))

    def alloc(shape, np_dtype):
        item = np.dtype(np_dtype).itemsize
        whole = torch.full((n + 2,) + shape + (item,), FILL, dtype=torch.uint8, device="cuda")
        return whole, whole[1:n + 1]

    whole = {}
    whole["window_kf"], win = alloc((caps["win_cap"],), np.int32)
    whole["win"], wres = alloc((), S.WINDOW_DTYPE)
    o = dict(caps)
    for name, dt, cap, tail in S.OUT_ROWS:
        whole[name], o[name] = alloc((caps[cap],) + tail, dt)
    whole["result"], o["result"] = alloc((), S.RESULT_DTYPE)
    b.window_dev(q, d["kf_bad"], d["kf_prev"], d["conn_start"], d["conn_list"], win, wres)
    if window_edit is not None:
        b.sync()
        window_edit(win.view(torch.int32).reshape(n, caps["win_cap"]))
    b.gather_dev(d, win, wres, o)
    b.sync()
    for name, w in whole.items():
        w = w.cpu().numpy()
        assert (w[0] == FILL).all() and (w[-1] == FILL).all(), (name, "a guard row was written")
    host = dict(caps)
    for name, dt, cap, tail in S.OUT_ROWS:
        host[name] = np.ascontiguousarray(o[name].cpu().numpy()).view(dt).reshape((n, caps[cap]) + tail)
    host["result"] = np.ascontiguousarray(o["result"].cpu().numpy()).view(S.RESULT_DTYPE).reshape(n)
    win_h = np.ascontiguousarray(win.cpu().numpy()).view(np.int32).reshape(n, caps["win_cap"])
    wres_h = np.ascontiguousarray(wres.cpu().numpy()).view(S.WINDOW_DTYPE).reshape(n)
    return win_h, wres_h, host, b"".join(whole[k].cpu().numpy().tobytes() for k in sorted(whole))


def test_host_forms_equal_the_restatement_byte_for_byte():
    t = the_map()
    expected = want(t, M.QUERIES, CAPS)
    assert {sc["status"] for _, sc in expected} == {M.OK, M.SKIPPED}
    win, res, o = run_host(t, M.QUERIES, CAPS)
    check_window(win, res, expected, CAPS["win_cap"])
    check_rows(o, expected)


def test_device_forms_equal_the_restatement_and_two_runs_give_the_same_bytes():
    t = the_map()
    expected = want(t, M.QUERIES, CAPS)
    b, d = builder(CAPS), dev_tables(t)
    win, res, o, bytes_1 = run_dev(t, M.QUERIES, CAPS, b, d)
    check_window(win, res, expected, CAPS["win_cap"])
    check_rows(o, expected)
    _, _, _, bytes_2 = run_dev(t, M.QUERIES, CAPS, b, d)
    assert bytes_1 == bytes_2  # no result depends on the order in which atomics land


def test_gather_with_a_feature_range_longer_than_65535():
    """scene_numpy.long_range_map: the high 16-bit halves of the range lengths and of their prefix sums are not 0."""
    t = M.long_range_map()
    expected = want(t, M.LONG_QUERIES, CAPS)
    assert all(sc["status"] == M.OK for _, sc in expected)
    win, res, o, _ = run_dev(t, M.LONG_QUERIES, CAPS)
    check_window(win, res, expected, CAPS["win_cap"])
    check_rows(o, expected)
    win, res, o = run_host(t, M.LONG_QUERIES, CAPS)
    check_window(win, res, expected, CAPS["win_cap"])
    check_rows(o, expected)


def test_without_imu_tables_or_gyro_weight_no_constraints_are_emitted():
    t = the_map()
    bare = {k: v for k, v in t.items() if not k.startswith("kf_time") and k not in ("kf_imu_begin", "kf_imu_end", "kf_preint_valid", "kf_rpc")}
    expected = [M.local_scene(bare, q, win_cap=36, pt_cap=1024, img_cap=128, obs_cap=4096) for q in M.QUERIES[:2]]
    _, _, o = run_host(bare, M.QUERIES[:2], CAPS)
    check_rows(o, expected)
    _, _, o = run_host(t, M.QUERIES[:2], CAPS, gyro_weight=0.0)
    check_rows(o, expected)
    assert all(sc["n_rpc"] == 0 for _, sc in expected)


@pytest.mark.parametrize("form", ["host", "dev"])
def test_every_overflow_status_at_its_cap_and_one_above(form):
    t = the_map()
    q = M.QUERIES[0]
    _, full = want(t, [q], CAPS)[0]
    run = run_host if form == "host" else run_dev
    for cap, count, status in (("win_cap", "n_window", M.WINDOW_OVERFLOW), ("pt_cap", "n_pt", M.PTS_OVERFLOW), ("img_cap", "n_img", M.IMG_OVERFLOW),
                               ("obs_cap", "n_obs", M.OBS_OVERFLOW)):
        for delta in (0, -1):
            caps = dict(CAPS, **{cap: full[count] + delta})
            expected = want(t, [q, M.QUERIES[3]], caps)
            assert expected[0][1]["status"] == (M.OK if delta == 0 else status) and expected[1][1]["status"] == M.OK
            out = run(t, [q, M.QUERIES[3]], caps)
            check_window(out[0], out[1], expected, caps["win_cap"])
            check_rows(out[2], expected)


def corrupted(t, kind):
    """A copy of the map with one bad index that only the window of keyframe 100 reaches."""
    t = {k: np.array(v, copy=True) for k, v in t.items()}
    n_kf, n_points = len(t["kf_bad"]), len(t["pt_flags"])
    f = next(f for f in range(t["feat_start"][100] + 10, t["feat_start"][101]) if t["feat_point"][f] >= 0 and not t["pt_flags"][t["feat_point"][f]] & M.PT_BAD
             and t["feat_point"][f] % 37 != 5 and t["feat_point"][f] % 41 != 9 and t["obs_start"][t["feat_point"][f] + 1] > t["obs_start"][t["feat_point"][f]])
    p = int(t["feat_point"][f])
    o = int(t["obs_start"][p])
    if kind == "point id":
        t["feat_point"][f] = n_points + 5
    elif kind == "observation keyframe":
        t["obs"][o][0] = n_kf
    elif kind == "observation feature":
        t["obs"][o][1] = 64
    elif kind == "octave":
        t["feat_octave"][t["feat_start"][t["obs"][o][0]] + t["obs"][o][1]] = len(t["level_inv_sq_scale"])
    elif kind == "obs_start":
        t["obs_start"][p + 1] = t["obs_start"][p] - 1
    elif kind == "kf_prev":
        t["kf_prev"][100] = n_kf + 3
    elif kind == "conn_start":
        t["conn_start"][101] = t["conn_start"][100] - 1
    elif kind == "connection":
        t["conn_list"]["kf"][t["conn_start"][101] - 1] = -2
    return t


@pytest.mark.parametrize("kind", ["point id", "observation keyframe", "observation feature", "octave", "obs_start", "kf_prev", "conn_start", "connection",
                                  "window order", "query"])
def test_device_forms_answer_a_bad_index_for_that_set_alone(kind):
    t = the_map()
    queries = [20, 100, 5]
    expected = want(t, queries, CAPS)
    edit = None
    if kind == "window order":
        def edit(win):
            win[1, 0], win[1, 1] = win[1, 1].clone(), win[1, 0].clone()
    sent = [20, len(t["kf_bad"]), 5] if kind == "query" else queries
    win, res, o, _ = run_dev(corrupted(t, kind), sent, CAPS, window_edit=edit)
    stage_1 = kind in ("kf_prev", "conn_start", "connection", "query")
    assert int(res[1]["status"]) == (M.BAD_INDEX if stage_1 else M.OK)
    expected[1] = ([], dict(status=M.BAD_INDEX, n_window=0, n_img=0, n_pt=0, n_obs=0, n_rpc=0))
    check_rows(o, expected)
    if stage_1:
        assert (win[1] == -1).all() and int(res[1]["n_window"]) == 0
    check_window(win[[0, 2]], res[[0, 2]], [expected[0], expected[2]], CAPS["win_cap"])


def test_host_forms_refuse_a_bad_index_before_any_launch():
    from snake_slam_amd import _lib, scene as S

    t = the_map()
    b = builder(CAPS)
    win, res = b.window([20, 100], t["kf_bad"], t["kf_prev"], t["conn_start"], t["conn_list"])
    for kind in ("point id", "observation keyframe", "observation feature", "octave", "obs_start"):
        o = S.host_outputs(2, fill=FILL, **CAPS)
        with pytest.raises(_lib.SnakeHipError):
            b.gather(corrupted(t, kind), win, res, CAPS["pt_cap"], CAPS["img_cap"], CAPS["obs_cap"], out=o)
        assert all((o[n].view(np.uint8) == FILL).all() for n in COUNT_OF)
    for kind in ("kf_prev", "conn_start", "connection"):
        c = corrupted(t, kind)
        with pytest.raises(_lib.SnakeHipError):
            b.window([20, 100], c["kf_bad"], c["kf_prev"], c["conn_start"], c["conn_list"])
    with pytest.raises(_lib.SnakeHipError):
        builder(CAPS, n_neighbours=44).window([20], t["kf_bad"], t["kf_prev"], t["conn_start"], t["conn_list"])


def padded(t, n_kf):
    """The same map in n_kf keyframe slots: the new ones have no features, no connections and no predecessor."""
    t = dict(t)
    extra = n_kf - len(t["kf_bad"])
    t["kf_bad"] = np.concatenate([t["kf_bad"], np.zeros(extra, np.uint8)])
    t["kf_prev"] = np.concatenate([t["kf_prev"], np.full(extra, -1, np.int32)])
    t["kf_prev"][-1] = 100  # the last slot is a keyframe behind 100
    t["kf_pose"] = np.concatenate([t["kf_pose"], np.zeros((extra, 7))])
    for k in ("feat_start", "conn_start"):
        t[k] = np.concatenate([t[k], np.full(extra, t[k][-1], np.int32)])
    for k in ("kf_time", "kf_imu_begin", "kf_imu_end", "kf_preint_valid", "kf_rpc"):
        t[k] = np.concatenate([t[k], np.zeros(extra, t[k].dtype)])
    return t


@pytest.mark.parametrize("form", ["host", "dev"])
def test_the_table_limits(form):
    t = padded(the_map(), M.MAX_KF)
    caps = dict(win_cap=M.MAX_WINDOW, pt_cap=M.MAX_PTS, img_cap=M.MAX_IMG, obs_cap=16384)
    queries = [M.MAX_KF - 1, 100]
    expected = want(t, queries, caps, n_neighbours=20, n_last=43)
    assert expected[0][1]["status"] == M.OK and expected[0][0][-1] == M.MAX_KF - 1
    out = (run_host if form == "host" else run_dev)(t, queries, caps, n_neighbours=20, n_last=43)
    check_window(out[0], out[1], expected, caps["win_cap"])
    check_rows(out[2], expected)


CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import test_scene_gpu as T
t = T.the_map()
b = T.builder(T.CAPS)
from snake_slam_amd import scene as S
for queries in (T.M.QUERIES, T.M.QUERIES[2:5], T.M.QUERIES):  # a large batch, a small one, the large one again: nothing stale is read
    expected = T.want(t, queries, T.CAPS)
    win, res = b.window(queries, t["kf_bad"], t["kf_prev"], t["conn_start"], t["conn_list"])
    o = S.host_outputs(len(queries), fill=T.FILL, **T.CAPS)
    b.gather(t, win, res, T.CAPS["pt_cap"], T.CAPS["img_cap"], T.CAPS["obs_cap"], out=o)
    T.check_window(win, res, expected, T.CAPS["win_cap"])
    T.check_rows(o, expected)
d = T.dev_tables(t)
for queries in (T.M.QUERIES, T.M.QUERIES[2:5]):
    expected = T.want(t, queries, T.CAPS)
    win, res, o, _ = T.run_dev(t, queries, T.CAPS, b, d)
    T.check_window(win, res, expected, T.CAPS["win_cap"])
    T.check_rows(o, expected)
print("child ok")
"""


def test_two_batch_sizes_on_one_handle_under_poison():
    """SNK_DEBUG_POISON=1 fills fresh scratch and staging with 0xCD (read once: a child process): nothing may rely on zeros, nothing behind
    a count is written, nothing stale is read."""
    env = dict(os.environ, SNK_DEBUG_POISON="1", PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", CHILD, str(ROOT / "tests")], capture_output=True, text=True, env=env, cwd=str(ROOT), timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stderr[-3000:]
