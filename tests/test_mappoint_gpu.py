"""GPU: snk_mappoint_refresh / snk_mappoint_refresh_batch_dev ("snk-mp v1") against the numpy restatement of
tests/mappoint_numpy.py -- bit-identical in every field, the doubles included: the restatement sorts every row of the distance matrix
and evaluates the fp64 expressions one IEEE operation at a time in the order of mappoint_core.hpp, the kernels select by halving and
sum the normal in list order, so there is nothing to tolerate.

The shapes are mappoint_numpy.edge_case: k in {0, 1, 2, 3, 4, 31, 32, 33, 63, 64, 65} (31 / 32 / 33 is also the packed / wide threshold
-1 / exact / +1), SNK_MP_MAX_OBS, invalid observations first / last / interior / all, two identical descriptors, ref_obs -1 / first /
last, and a run of 137 points of k = 5 (more than two 64-point chunks, 12 to a wavefront so the 13th opens the next) before a k = 64
point; half of the cases draw the descriptors as one pattern with <= 8 flipped bits so that rows share a median."""
import ctypes as C
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import mappoint_numpy as M

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
ARGS = ("obs_start", "desc", "pose", "octave", "valid", "position", "ref_obs")


@functools.lru_cache(maxsize=None)
def edge(near_tie):
    return M.edge_case(70 + int(near_tie), bool(near_tie))


@functools.lru_cache(maxsize=None)
def edge_want(near_tie, rule):
    return M.refresh(edge(near_tie), rule)


@functools.lru_cache(maxsize=None)
def small(near_tie):
    """Every k up to two past the packed form's last, then a run that straddles wavefronts and a chunk, then wide points."""
    return M.make_case(80 + int(near_tie), list(range(0, M.PACKED_MAX_K + 3)) + [5] * 70 + [64, 100, 7], bool(near_tie), invalid_frac=0.1)


def run(ref, case, what=M.ALL):
    return ref.refresh(*(case[k] for k in ARGS), what=what)


def differing(got, want):
    return [(p, got[p], want[p]) for p in range(len(want)) if got[p].tobytes() != want[p].tobytes()][:3]


@pytest.mark.parametrize("rule", [M.MEDIAN, M.SUM])
@pytest.mark.parametrize("near_tie", [False, True])
def test_host_form_equals_the_restatement(near_tie, rule):
    from snake_slam_amd.mappoint import MapPointRefresher

    c, want = edge(near_tie), edge_want(near_tie, rule)
    r = MapPointRefresher(rule)
    try:
        got = run(r, c)
        again = run(r, c)
    finally:
        r.close()
    assert got.tobytes() == want.tobytes(), differing(got, want)
    assert again.tobytes() == got.tobytes()
    ks = np.diff(c["obs_start"])
    assert np.all(got["status"] == 0) and np.array_equal(got["best"] >= 0, got["n_valid"] > 0) and np.all(got["n_valid"] <= ks)
    tie = got[8]  # k = 63, observations 7 and 40 identical
    assert tie["best"] != 40


@pytest.mark.parametrize("what", [M.DESCRIPTOR, M.NORMAL, M.DEPTH])
def test_single_part_masks(what):
    from snake_slam_amd.mappoint import MapPointRefresher

    c = small(True)
    r = MapPointRefresher(M.MEDIAN)
    try:
        got = run(r, c, what)
    finally:
        r.close()
    want = M.refresh(c, M.MEDIAN, what)
    assert got.tobytes() == want.tobytes(), differing(got, want)


def test_reference_method_names_and_empty_call():
    from snake_slam_amd.mappoint import MapPointRefresher

    c = small(False)
    want = M.refresh(c, M.SUM)
    r = MapPointRefresher(M.SUM)
    try:
        best, desc = r.ComputeDistinctiveDescriptors(c["obs_start"], c["desc"], c["valid"])
        nrm = r.UpdateNormal(c["obs_start"], c["pose"], c["valid"], c["position"])
        dep, lvl = r.UpdateDepth(c["obs_start"], c["pose"], c["octave"], c["position"], c["ref_obs"])
        none = r.refresh(np.zeros(1, np.int32), np.zeros((0, 4), np.uint64), np.zeros((0, 7)), [], [], np.zeros((0, 3)), [])
    finally:
        r.close()
    assert np.array_equal(best, want["best"]) and np.array_equal(desc, want["desc"]) and nrm.tobytes() == want["normal"].tobytes()
    assert dep.tobytes() == want["ref_depth"].tobytes() and np.array_equal(lvl, want["ref_level"]) and len(none) == 0


CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import mappoint_numpy as M
from snake_slam_amd.mappoint import MapPointRefresher
kind, tie, out = sys.argv[2], int(sys.argv[3]), sys.argv[4]
c = M.edge_case(70 + tie, bool(tie)) if kind == "edge" else M.make_case(80 + tie, list(range(0, M.PACKED_MAX_K + 3)) + [5] * 70 + [64, 100, 7], bool(tie), invalid_frac=0.1)
res = []
for rule in (M.MEDIAN, M.SUM):
    r = MapPointRefresher(rule)
    res.append(r.refresh(*(c[k] for k in %r)))
    r.close()
np.concatenate(res).tofile(out)
""" % (ARGS,)


@pytest.mark.parametrize("form,kind,near_tie", [("wide", "edge", True), ("packed", "small", True), ("wide", "small", False)])
def test_each_form_forced_over_the_k_it_accepts(tmp_path, form, kind, near_tie):
    """SNK_MP_FORM is read once: a fresh child process per value.  wide takes every k from 1 to SNK_MP_MAX_OBS (the edge case), packed every
    k up to 32 (beyond it the wide form runs, as without the switch); the results do not depend on the form."""
    out = tmp_path / "res.bin"
    env = dict(os.environ, SNK_MP_FORM=form, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", CHILD, str(ROOT / "tests"), kind, str(int(near_tie)), str(out)], capture_output=True, text=True, env=env,
                       cwd=str(ROOT), timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.fromfile(out, M.RESULT)
    if kind == "edge":
        want = np.concatenate([edge_want(near_tie, M.MEDIAN), edge_want(near_tie, M.SUM)])
    else:
        want = np.concatenate([M.refresh(small(near_tie), M.MEDIAN), M.refresh(small(near_tie), M.SUM)])
    assert got.tobytes() == want.tobytes(), differing(got, want)


def test_device_form_equals_the_host_form_and_reports_bad_indices():
    """A synthetic keyframe batch (3 slots, cap 128, n = 128 / 77 / 100).  Points of k up to 70 observe random in-range features; three
    more are broken on purpose -- a feature == n[slot] (inside cap, outside n), a kf_slot == batch, k = SNK_MP_MAX_OBS + 1 -- and one has
    its out-of-range pair on an INVALID observation, which is never read and so is no error.  The broken points sit between good ones."""
    import torch

    from snake_slam_amd.mappoint import RESULT_DTYPE, MapPointRefresher
    from snake_slam_amd.matcher import KP64_DTYPE
    from snake_slam_amd.tracking import frames_dev

    rng = np.random.default_rng(91)
    B, CAP = 3, 128
    n = np.array([128, 77, 100], np.int32)
    desc = M.descriptors(rng, B * CAP, True).reshape(B, CAP, 4)
    kps = np.zeros((B, CAP), KP64_DTYPE)
    kps["octave"] = rng.integers(0, 8, (B, CAP))
    poses = M.random_pose(rng, B)
    ks = [3, 0, 8, 33, 5, 1, 32, 70, 12, 2, 6, 40, 9] + [5] * 70 + [M.MAX_OBS + 1, 4, 31]
    BAD_FEATURE, BAD_SLOT, INVALID_BAD, TOO_MANY = 2, 7, 10, len(ks) - 3
    start = np.concatenate([[0], np.cumsum(ks)]).astype(np.int32)
    slot = rng.integers(0, B, start[-1]).astype(np.int32)
    obs = np.stack([slot, (rng.random(start[-1]) * n[slot]).astype(np.int32)], 1)
    valid = (rng.random(start[-1]) >= 0.1).astype(np.uint8)
    ref = np.array([int(rng.integers(-1, k)) if k else -1 for k in ks], np.int32)
    position = rng.uniform(-3, 3, (len(ks), 3))
    obs[start[BAD_FEATURE] + 5] = (1, 77)
    valid[start[BAD_FEATURE] + 5] = 1
    obs[start[BAD_SLOT] + 69] = (B, 0)
    valid[start[BAD_SLOT] + 69] = 1
    obs[start[INVALID_BAD] + 2] = (-1, 1 << 30)
    valid[start[INVALID_BAD] + 2] = 0
    ref[INVALID_BAD] = 0
    ref[TOO_MANY] = -1

    # the gathered copy of the good points for the host form
    good = [p for p in range(len(ks)) if p not in (BAD_FEATURE, BAD_SLOT, TOO_MANY)]
    sel = np.concatenate([np.arange(start[p], start[p + 1]) for p in good]).astype(np.int64)
    o = obs[sel].copy()
    assert np.count_nonzero(o[:, 0] < 0) == 1
    o[o[:, 0] < 0] = 0  # the invalid observation's pair is not read: any in-range stand-in
    host = dict(obs_start=np.concatenate([[0], np.cumsum([ks[p] for p in good])]).astype(np.int32), desc=desc[o[:, 0], o[:, 1]],
                pose=poses[o[:, 0]], octave=kps["octave"][o[:, 0], o[:, 1]].astype(np.int32), valid=valid[sel], position=position[good], ref_obs=ref[good])

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    d = dict(n=t(n), kps=t(kps.view(np.uint8).reshape(B, CAP, 24)), desc=t(desc.view(np.int64)), poses=t(poses), start=t(start), obs=t(obs),
             valid=t(valid), position=t(position), ref=t(ref))
    aux = (torch.zeros((B, CAP), dtype=torch.float32, device="cuda"), torch.zeros((B, CAP), dtype=torch.uint8, device="cuda"),
           torch.zeros((B, 2), dtype=torch.int32, device="cuda"))
    fd = frames_dev((0.0, 0.0, 752.0, 480.0), d["n"], d["kps"], d["desc"], *aux)
    for rule in (M.MEDIAN, M.SUM):
        out = torch.full((len(ks), 80), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        r = MapPointRefresher(rule)
        try:
            r.refresh_batch_dev(fd, d["poses"], d["start"], d["obs"], d["valid"], d["position"], d["ref"], out)
            r.sync()
            got = out.cpu().numpy().view(RESULT_DTYPE).reshape(-1)
            host_res = run(r, host)
        finally:
            r.close()
        want = np.zeros(len(ks), M.RESULT)
        want[good] = host_res
        want[BAD_FEATURE] = want[BAD_SLOT] = M.untouched(M.BAD_INDEX)
        want[TOO_MANY] = M.untouched(M.TOO_MANY)
        assert got.tobytes() == want.tobytes(), differing(got, want)
        assert host_res.tobytes() == M.refresh(host, rule).tobytes()
        assert got["best"][INVALID_BAD] >= 0 and got["status"][INVALID_BAD] == 0


def test_argument_errors_are_codes_with_a_message():
    from snake_slam_amd import _lib
    from snake_slam_amd.mappoint import MapPointRefresher, MpParams

    lib = _lib.load()
    c = M.make_case(95, [3, 5, 2])
    r = MapPointRefresher()
    try:
        def call(par=None, n=3, **kw):
            a = {k: np.ascontiguousarray(kw.get(k, c[k])) if kw.get(k, c[k]) is not None else None for k in ARGS}
            a["obs_start"] = None if a["obs_start"] is None else a["obs_start"].astype(np.int32)
            out = np.zeros(max(len(c["ref_obs"]), 1), M.RESULT)
            ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
            par = par or MpParams(M.MEDIAN, M.ALL)
            rc = lib.snk_mappoint_refresh(r._h, C.byref(par), n, *(ptr(a[k]) for k in ARGS), None if kw.get("out", 1) is None else out.ctypes.data)
            return rc, lib.snk_last_error()

        for kw, text in ((dict(obs_start=np.array([0, 3, 2, 10])), b"non-decreasing"), (dict(obs_start=np.array([1, 3, 8, 10])), b"obs_start[0]"),
                         (dict(ref_obs=np.array([3, 0, 0], np.int32)), b"ref_obs"), (dict(ref_obs=np.array([0, -2, 0], np.int32)), b"ref_obs"),
                         (dict(obs_start=np.array([0, 3, 8, 8 + M.MAX_OBS + 1])), b"SNK_MP_MAX_OBS"), (dict(desc=None), b"NULL"), (dict(valid=None), b"NULL"),
                         (dict(position=None), b"NULL"), (dict(obs_start=None), b"NULL"), (dict(out=None), b"NULL"), (dict(par=MpParams(2, M.ALL)), b"rule"),
                         (dict(par=MpParams(M.MEDIAN, 8)), b"what"), (dict(n=-1), b"negative")):
            rc, msg = call(**kw)
            assert rc == 1 and text in msg, (kw, rc, msg)
        assert lib.snk_mappoint_refresh(r._h, None, 0, None, None, None, None, None, None, None, None) == 1
        assert lib.snk_mappoint_refresh(r._h, C.byref(MpParams(M.MEDIAN, M.ALL)), 0, None, None, None, None, None, None, None, None) == 0
        # the handle is as good as before
        assert run(r, c).tobytes() == M.refresh(c).tobytes()
    finally:
        r.close()
