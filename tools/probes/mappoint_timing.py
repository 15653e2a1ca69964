"""Timing probe of the map-point refresh (does not touch bench.py): the device-resident form at a map-scale shape -- `--points` points
with k drawn from 2 .. 30 (mean about 8) plus `--wide-points` points of `--wide-k` observations, over `--keyframes` keyframe slots of
1000 features.

Prints one JSON line with the time per call of snk_mappoint_refresh_batch_dev (median and minimum of `--reps` calls after three
warm-ups, events on the handle's stream) for the whole list, for the small points alone, for the wide points alone and for the whole list
with only the normal selected; then the numpy restatement's time on this host for a sample of the points, extrapolated to the list.
The form is chosen per point by its k; SNK_MP_FORM=wide (read once per process) puts every point on the wide form: run the probe a second
time under it for the per-form figure.  Kernel statistics: `rocprofv3 --kernel-trace --stats -- python tools/probes/mappoint_timing.py`.
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--wide-points", type=int, default=100)
    ap.add_argument("--wide-k", type=int, default=1000)
    ap.add_argument("--keyframes", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--numpy-sample", type=int, default=1000, help="small points (and 2 wide ones) the numpy loop is timed on")
    a = ap.parse_args()
    import torch

    import mappoint_numpy as M
    from snake_slam_amd.mappoint import RESULT_DTYPE, MapPointRefresher
    from snake_slam_amd.matcher import KP64_DTYPE
    from snake_slam_amd.tracking import frames_dev

    rng = np.random.default_rng(5)
    B, CAP = a.keyframes, 1000
    ks_small = np.clip(2 + rng.poisson(6.0, a.points), 2, 30)
    ks = np.concatenate([ks_small, np.full(a.wide_points, a.wide_k)]).astype(np.int64)
    perm = rng.permutation(len(ks))  # the wide points lie anywhere in the list
    ks = ks[perm]
    start = np.concatenate([[0], np.cumsum(ks)]).astype(np.int32)
    n_obs = int(start[-1])
    obs = np.stack([rng.integers(0, B, n_obs), rng.integers(0, CAP, n_obs)], 1).astype(np.int32)
    valid = (rng.random(n_obs) >= 0.02).astype(np.uint8)
    desc = rng.integers(0, 2**63, (B, CAP, 4), dtype=np.int64)
    kps = np.zeros((B, CAP), KP64_DTYPE)
    kps["octave"] = rng.integers(0, 8, (B, CAP))
    poses = M.random_pose(rng, B)
    position = rng.uniform(-3, 3, (len(ks), 3))
    ref = (rng.random(len(ks)) * ks).astype(np.int32)

    def sub(mask):
        """the points of `mask` as a list of their own"""
        idx = np.flatnonzero(mask)
        sel = np.concatenate([np.arange(start[p], start[p + 1]) for p in idx]) if len(idx) else np.zeros(0, np.int64)
        return dict(start=np.concatenate([[0], np.cumsum(ks[idx])]).astype(np.int32), obs=obs[sel], valid=valid[sel], position=position[idx], ref=ref[idx])

    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt, device="cuda")  # noqa: E731
    # the view holds addresses only: the tensors stay alive in `frame`
    frame = (t(np.full(B, CAP, np.int32)), t(kps.view(np.uint8).reshape(B, CAP, 24)), t(desc), z(1, dt=torch.float32), z(1, dt=torch.uint8), z(1))
    fd = frames_dev((0.0, 0.0, 752.0, 480.0), *frame)
    d_poses = t(poses)
    lists = dict(all=dict(start=start, obs=obs, valid=valid, position=position, ref=ref), small=sub(ks <= 30), wide=sub(ks > 30))
    dev = {name: {k: t(v) for k, v in L.items()} for name, L in lists.items()}
    outs = {name: z(len(L["ref"]), 80, dt=torch.uint8) for name, L in lists.items()}
    stream = torch.cuda.Stream()
    r = MapPointRefresher(M.MEDIAN, stream=stream.cuda_stream)
    out = dict(points=int(a.points), wide_points=int(a.wide_points), wide_k=int(a.wide_k), mean_k_small=float(ks_small.mean()), observations=n_obs,
               keyframes=B, form_env=os.environ.get("SNK_MP_FORM", ""))
    torch.cuda.synchronize()  # the inputs were uploaded on torch's default stream
    with torch.cuda.stream(stream):
        for name, which, what in (("all", "all", M.ALL), ("small_points", "small", M.ALL), ("wide_points", "wide", M.ALL), ("all_normal_only", "all", M.NORMAL)):
            D = dev[which]
            if len(lists[which]["ref"]) == 0:
                continue
            times = []
            for rep in range(a.reps + 3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                r.refresh_batch_dev(fd, d_poses, D["start"], D["obs"], D["valid"], D["position"], D["ref"], outs[which], what)
                e1.record(stream)
                e1.synchronize()
                if rep >= 3:
                    times.append(e0.elapsed_time(e1))
            out[name + "_ms_median"], out[name + "_ms_min"] = float(np.median(times)), float(np.min(times))
    r.sync()
    got = outs["small"].cpu().numpy().view(RESULT_DTYPE).reshape(-1)
    got_wide = outs["wide"].cpu().numpy().view(RESULT_DTYPE).reshape(-1)
    r.close()
    assert np.all(got["status"] == 0) and np.all(got_wide["status"] == 0)

    # the same loop in numpy on this host, on a sample, checked against the device's results on the way
    def host_case(L, count):
        e = int(L["start"][count])
        o = L["obs"][:e]
        return dict(obs_start=L["start"][:count + 1], desc=desc.view(np.uint64)[o[:, 0], o[:, 1]], pose=poses[o[:, 0]],
                    octave=kps["octave"][o[:, 0], o[:, 1]].astype(np.int32), valid=L["valid"][:e], position=L["position"][:count], ref_obs=L["ref"][:count])

    ns = min(a.numpy_sample, len(lists["small"]["ref"]))
    t0 = time.perf_counter()
    want = M.refresh(host_case(lists["small"], ns))
    out["numpy_ms_per_small_point"] = (time.perf_counter() - t0) / max(ns, 1) * 1e3
    assert want.tobytes() == got[:ns].tobytes()
    nw = min(2, len(lists["wide"]["ref"]))
    if nw:
        t0 = time.perf_counter()
        want = M.refresh(host_case(lists["wide"], nw))
        out["numpy_ms_per_wide_point"] = (time.perf_counter() - t0) / nw * 1e3
        assert want.tobytes() == got_wide[:nw].tobytes()
    out["numpy_ms_extrapolated"] = out["numpy_ms_per_small_point"] * a.points + out.get("numpy_ms_per_wide_point", 0.0) * a.wide_points
    print(json.dumps(out))


if __name__ == "__main__":
    main()
