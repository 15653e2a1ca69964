"""GPU: global BA (FullBA) at map scale, where the form of the reduced-camera-system PCG changes with the size of the system.

n6 = 6 x free keyframes.  The hand-over picks (csrc/ba.hip, ba_plan_pcg, called by snk_ba_set_problems):
* pcgl_persist_reg (rows of S in registers) up to n6 = 2048 -- pinned by test_ba_gpu.py's boundary sizes;
* pcgl_persist1 (one grid barrier, rows of S streamed) up to n6 * 24 <= 150 KB (n6 <= 6400); its preconditioner rows sit in
  registers up to n6 = 16 * 256 = 4096 and are read from memory above;
* pcgl_persist (two grid barriers) up to n6 * 8 <= 150 KB (n6 <= 19200);
* the multi-launch pcgl_* sequence beyond that (and after a refused cooperative launch).
The one-launch forms run min(CUs, max(16, ceil(n6 / 12))) workgroups: more than 12 rows per workgroup from n6 > 12 CUs on.

Every case is compared with the CPU oracle at bounds far tighter than the 1e-5 specification: the legitimate difference is the
summation order alone, and a wrong preconditioner entry or a dropped partial sum moves the result by far more than that (see
TOL_SCENE below for the measured spread).  Child processes (forced workgroup counts and forms) get the scene and the oracle's result
as an .npz; after a child that ends on a signal or a time limit no later GPU work of this module is started."""
import functools
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

# Bounds against the oracle, per scene: (pose RMSE, point RMSE, final cost relative).  Two spreads are recorded per scene: the oracle
# against its own reversed-order sums (oracle.ba_solve(..., sum_order=1): what a legitimate change of a summation order can do) and
# HIP against the oracle on the MI355X (256 CUs; largest over every form and workgroup count the scene runs here).  FullBA(2) with
# PCG 40; 3202 keyframes FullBA(1) with PCG 20.  Each bound is 10-20x the larger of the two:
#   keyframes   reordered oracle: pose / point / cost   HIP: pose / point / cost   ->  bound
#   513         7.7e-13 / 1.5e-12 / 2.8e-14             6.7e-13 / 1.4e-12 / 2.9e-15    default: 2e-11 / 5e-11 / 1e-12
#   514         7.1e-13 / 1.6e-12 / 2.6e-14             9.6e-13 / 1.3e-12 / 3.3e-15    default
#   684         7.4e-13 / 2.2e-12 / 5.0e-14             1.1e-12 / 1.5e-12 / 4.4e-14    default
#   1068        8.3e-13 / 2.3e-12 / 5.5e-14             7.8e-13 / 2.3e-12 / 3.6e-14    default
#   3202        1.1e-12 / 8.0e-13 / 1.5e-16             9.3e-13 / 7.3e-13 / 2.9e-14    default
#   683         2.8e-12 / 9.6e-12 / 9.7e-15             1.0e-12 / 1.9e-12 / 3.6e-15    5e-11 / 1e-10 / 1e-12
#   343         3.9e-12 / 9.6e-11 / 2.0e-13             4.6e-12 / 1.1e-10 / 2.5e-13    5e-11 / 2e-9 / 5e-12   (pcgl_persist1 forced)
#   1067        4.9e-11 / 2.8e-10 / 2.9e-13             6.5e-11 / 2.5e-10 / 5.8e-13    1e-9 / 5e-9 / 1e-11
# 683, 343 and 1067 are less well conditioned (their truncated PCG amplifies rounding more): the looser bounds follow the scene, not
# the kernel.  Initial cost: measured <= 9e-15 relative, bound 1e-12.  A relative 1e-9 on one row of A p in pcgl_persist moves the
# 1068-keyframe result by 1.3e-10 (pose) / 4.6e-10 (points) / 3.6e-12 (cost), 4-9x over its bounds.  The specification (1e-5,
# test_ba_gpu.py) is unchanged.
TOL_DEFAULT = (2e-11, 5e-11, 1e-12)
TOL_SCENE = {683: (5e-11, 1e-10, 1e-12), 343: (5e-11, 2e-9, 5e-12), 1067: (1e-9, 5e-9, 1e-11)}
TOL_COST_INITIAL = 1e-12

_STOP = {"reason": None}  # set when a child ended on a signal or a time limit: every later GPU step of the module is skipped


def _check_stop():
    if _STOP["reason"]:
        pytest.skip(_STOP["reason"])


def _rmse(a, b):
    return float(np.sqrt(((np.asarray(a) - np.asarray(b)) ** 2).sum(axis=-1).mean())) if len(a) else 0.0


@functools.lru_cache(maxsize=None)
def _cus():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@functools.lru_cache(maxsize=2)
def _scene(n_kf):
    from snake_slam_amd import synth

    return synth.ba_scene(n_kf=n_kf, n_pt=12 * n_kf, obs_per_pt=6, seed=900 + n_kf, n_fixed=1)[0]


@functools.lru_cache(maxsize=4)
def _oracle(n_kf, iterations, pcg):
    from oracle import oracle

    oracle.build()
    pose, pt, ci, cf, its = oracle.ba_solve(_scene(n_kf), oracle.ba_options(iterations, pcg))
    return dict(pose=pose, pt=pt, ci=ci, cf=cf, pcg=its)


def _solve(sc, iterations, pcg, ba=None):
    """FullBA on the scene; returns (result dict, pcg form after the hand-over, form after the solve)."""
    from snake_slam_amd.ba import BARec, gba_options

    own = ba is None
    ba = ba or BARec(gba_options(max_iterations=iterations, max_pcg_iterations=pcg))
    ba.create(sc)
    form = ba.pcg_form()
    ci, cf = ba.solve(iterations)
    pose, pt, its = ba.state(0)
    after = ba.pcg_form()
    if own:
        ba.close()
    return dict(pose=pose, pt=pt, ci=ci[0], cf=cf[0], pcg=its), form, after


def _spread(got, want):
    return dict(pose_q=_rmse(got["pose"][:, :4], want["pose"][:, :4]), pose_t=_rmse(got["pose"][:, 4:], want["pose"][:, 4:]),
                pt=_rmse(got["pt"], want["pt"]), ci=abs(got["ci"] - want["ci"]) / want["ci"], cf=abs(got["cf"] - want["cf"]) / want["cf"],
                pcg=int(got["pcg"]), pcg_oracle=int(want["pcg"]))


def _assert_close(got, want, iterations, what):
    s = _spread(got, want)
    print(f"[spread] {what}: {json.dumps(s)}")
    tol_pose, tol_pt, tol_cf = TOL_SCENE.get(len(got["pose"]), TOL_DEFAULT)
    assert s["ci"] <= TOL_COST_INITIAL, (what, s)
    assert s["cf"] <= tol_cf, (what, s)
    assert s["pose_q"] <= tol_pose and s["pose_t"] <= tol_pose, (what, s)
    assert s["pt"] <= tol_pt, (what, s)
    assert abs(s["pcg"] - s["pcg_oracle"]) <= iterations, (what, s)  # within one PCG iteration per LM iteration
    assert got["cf"] < got["ci"], (what, s)
    return s


def _persist_wgs(n6):
    return min(_cus(), max(16, -(-n6 // 12)))


def _natural_cases():
    cus = _cus()
    return [  # (keyframes, expected form); n6 = 6 (keyframes - 1)
        (2 * cus + 1, "persist1"),  # n6 = 12 CUs: 12 rows per workgroup
        (2 * cus + 2, "persist1"),  # n6 = 12 CUs + 6: 13 rows per workgroup
        (683, "persist1"),          # n6 = 4092: preconditioner rows in registers
        (684, "persist1"),          # n6 = 4098: ... read from memory
        (1067, "persist1"),         # n6 = 6396: the largest one-barrier system
        (1068, "persist"),          # n6 = 6402: the two-barrier form
    ]


@pytest.mark.parametrize("case", range(6), ids=["12cus", "12cus+6", "n6-4092", "n6-4098", "n6-6396", "n6-6402"])
def test_global_ba_natural_form_boundaries(orc, case):
    """FullBA(2) at the sizes where the form chosen by the hand-over, or the code inside it, changes: the workgroups' rows go from 12
    to 13 (n6 = 12 CUs, 12 CUs + 6), pcgl_persist1's preconditioner moves from registers to memory (n6 = 4092, 4098), pcgl_persist1
    gives way to pcgl_persist (n6 = 6396, 6402).  The form and its workgroup count are read back, not inferred from the size."""
    _check_stop()
    n_kf, form = _natural_cases()[case]
    n6 = 6 * (n_kf - 1)
    if case < 2 and 12 * _cus() <= 2048:
        pytest.skip(f"{_cus()} compute units: n6 = 12 CUs is a pcgl_persist_reg size on this device (test_ba_gpu.py covers those)")
    got, chosen, _ = _solve(_scene(n_kf), 2, 40)
    assert chosen == (form, _persist_wgs(n6)), (n_kf, chosen)
    _assert_close(got, _oracle(n_kf, 2, 40), 2, f"{n_kf} keyframes ({form})")


def test_global_ba_multi_launch_at_natural_size(orc):
    """n6 = 19206 (3202 keyframes): pcgl_persist's direction no longer fits 150 KB of LDS, the multi-launch PCG is chosen by size.
    FullBA(1) with PCG 20 bounds the oracle's dense PCG (S is 19206 x 19206 doubles, 2.9 GB on both sides)."""
    _check_stop()
    n_kf = 3202
    got, chosen, _ = _solve(_scene(n_kf), 1, 20)
    assert chosen == ("launches", 0), chosen
    _assert_close(got, _oracle(n_kf, 1, 20), 1, "3202 keyframes (launches)")


# ---- child processes: forced workgroup counts and forms ----

def _child(args):
    """Runs in a child process: python -c '...' <scene.npz> <oracle.npz> <out.json> <iterations> <pcg>."""
    scene_f, oracle_f, out_f, iterations, pcg = args[0], args[1], args[2], int(args[3]), int(args[4])
    with np.load(scene_f) as z:
        sc = {k: z[k] for k in z.files}
    with np.load(oracle_f) as z:
        want = {k: z[k][()] if z[k].ndim == 0 else z[k] for k in z.files}
    got, form, after = _solve(sc, iterations, pcg)
    s = _assert_close(got, want, iterations, f"{sc['pose'].shape[0]} keyframes, {form}")
    Path(out_f).write_text(json.dumps(dict(spread=s, form=list(form), after=list(after))))


def _run_child(tmp_path, n_kf, env, iterations=2, pcg=40, timeout=300):
    _check_stop()
    tag = f"{n_kf}_" + "_".join(f"{k}{v}" for k, v in sorted(env.items()))
    scene_f, oracle_f, out_f = tmp_path / f"scene_{n_kf}.npz", tmp_path / f"oracle_{n_kf}.npz", tmp_path / f"out_{tag}.json"
    if not scene_f.exists():
        np.savez(scene_f, **{k: np.asarray(v) for k, v in _scene(n_kf).items()})
        np.savez(oracle_f, **_oracle(n_kf, iterations, pcg))
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import test_ba_map_scale_gpu as m; m._child(sys.argv[2:])")
    cmd = [sys.executable, "-c", code, str(ROOT / "tests"), str(scene_f), str(oracle_f), str(out_f), str(iterations), str(pcg)]
    try:
        r = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=str(ROOT), **env), capture_output=True, text=True, cwd=str(ROOT),
                           timeout=timeout)
    except subprocess.TimeoutExpired:
        _STOP["reason"] = f"an earlier child ({n_kf} keyframes, {env}) ran into its {timeout} s time limit"
        raise
    if r.returncode < 0 or r.returncode in (134, 137, 139):
        _STOP["reason"] = f"an earlier child ({n_kf} keyframes, {env}) ended with status {r.returncode}"
    assert r.returncode == 0, f"{n_kf} keyframes {env}: status {r.returncode}\n--- child stdout (tail) ---\n{r.stdout[-3000:]}\n" \
                              f"--- child stderr (tail) ---\n{r.stderr[-3000:]}"
    res = json.loads(out_f.read_text())
    print(f"[spread] {n_kf} keyframes {env}: {json.dumps(res['spread'])}")
    return tuple(res["form"]), tuple(res["after"])


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("map_scale")


@pytest.mark.parametrize("which", ["1", "8", "9", "63", "cus-1", "cus"])
def test_persistent_pcg_workgroup_sweep(orc, scene_dir, which):
    """SNK_BA_PERSIST_WGS: one workgroup alone, full and partial groups of eight (the grid barrier groups the workgroups by
    blockIdx & 7), a partial last group, one fewer than the CUs and all of them -- on 343 keyframes (the switch forces
    pcgl_persist1 there) and 1068 keyframes (pcgl_persist, the two-barrier form, chosen by size)."""
    wgs = _cus() - 1 if which == "cus-1" else _cus() if which == "cus" else int(which)
    env = {"SNK_BA_PERSIST_WGS": str(wgs)}
    assert _run_child(scene_dir, 343, env)[0] == ("persist1", wgs)
    assert _run_child(scene_dir, 1068, env)[0] == ("persist", wgs)


@pytest.mark.parametrize("env, form, after", [
    ({"SNK_BA_PCGL_LAUNCHES": "1"}, "launches", "launches"),
    ({"SNK_BA_PERSIST_FAIL": "1"}, "persist", "launches"),  # the runtime refuses the cooperative launch: multi-launch in the same solve
], ids=["launches", "persist-fail"])
def test_forced_pcg_forms_at_large_size(orc, scene_dir, env, form, after):
    """The multi-launch PCG on 1068 keyframes, chosen by switch and reached through a refused cooperative launch."""
    got, done = _run_child(scene_dir, 1068, env)
    assert got == (form, _persist_wgs(6 * 1067) if form == "persist" else 0) and done == (after, 0), (got, done)


@pytest.mark.parametrize("n_kf", [684, 1068])
def test_persistent_pcg_is_deterministic_across_hand_overs(n_kf):
    """pcgl_persist1 (684 keyframes) and pcgl_persist (1068) sum in a fixed order: the same scene solved three times on one handle
    (handed over again, handed over again, reset) and once on a fresh handle gives bit-identical results.  A difference is a barrier
    or flag-reset defect (the grid barrier's flags are zeroed by pcgl_init before every PCG)."""
    _check_stop()
    from snake_slam_amd.ba import BARec, gba_options

    sc = _scene(n_kf)
    ba = BARec(gba_options(max_iterations=2, max_pcg_iterations=40))
    runs = [_solve(sc, 2, 40, ba)[0], _solve(sc, 2, 40, ba)[0]]
    ba.reset()
    ci, cf = ba.solve(2)
    pose, pt, its = ba.state(0)
    runs.append(dict(pose=pose, pt=pt, ci=ci[0], cf=cf[0], pcg=its))
    ba.close()
    runs.append(_solve(sc, 2, 40)[0])
    for k, r in enumerate(runs[1:], 1):
        for f in ("pose", "pt", "ci", "cf", "pcg"):
            assert np.array_equal(r[f], runs[0][f]), f"run {k}: {f} differs from the first solve"


def test_failed_hand_over_with_host_threads_per_pass():
    """test_ba_gpu.py's failed hand-over cases with the threaded list builder forced and its threads created per pass."""
    _check_stop()
    env = {"SNK_BA_HOST_THREADS": "4", "SNK_BA_NO_HOST_POOL": "1"}
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", str(ROOT / "tests" / "test_ba_gpu.py"), "-m", "gpu", "-q", "-rf", "--tb=short",
                            "-p", "no:cacheprovider", "-k", "failed_hand_over"], env=dict(os.environ, **env), capture_output=True, text=True,
                           cwd=str(ROOT), timeout=300)
    except subprocess.TimeoutExpired:
        _STOP["reason"] = "the host-thread hand-over child ran into its time limit"
        raise
    if r.returncode < 0 or r.returncode in (134, 137, 139):
        _STOP["reason"] = f"the host-thread hand-over child ended with status {r.returncode}"
    assert r.returncode == 0, f"{env}\n--- child stdout (tail) ---\n{r.stdout[-6000:]}\n--- child stderr (tail) ---\n{r.stderr[-1500:]}"
    assert "4 passed" in r.stdout
