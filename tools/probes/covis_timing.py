"""Timing probe of the covisibility kernels (does not touch bench.py): the device-resident forms at a map-scale shape -- `--queries`
UpdateConnections queries on a structured map of `--keyframes` keyframes whose points have about eight observations each
(covis_numpy.make_map: a sliding window of points per keyframe), and `--frames` local-keyframe votes of `--matched` matched points.

Prints one JSON line with the time per call of snk_covis_update_batch_dev and snk_covis_vote_batch_dev (median and minimum of `--reps`
calls after three warm-ups, events on the handle's stream), the list lengths, and the restatement's time on this host for a sample of
the sets, extrapolated to the call.  SNK_COVIS_LONG_MIN=<n> (read once per process) moves the length from which a wavefront walks a
list: run the probe again under it for an A/B.  Kernel statistics: `rocprofv3 --kernel-trace --stats -- python tools/probes/covis_timing.py`.
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
    ap.add_argument("--keyframes", type=int, default=10000)
    ap.add_argument("--points", type=int, default=400000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--matched", type=int, default=300)
    ap.add_argument("--cap", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--numpy-sample", type=int, default=50, help="sets the restatement is timed on (and the device's results checked against)")
    a = ap.parse_args()
    import torch

    import covis_numpy as M
    from snake_slam_amd.covis import CovisibilityGraph

    rng = np.random.default_rng(7)
    m = M.make_map(7, a.keyframes, a.points, window=600, p_see=0.55)
    q = rng.integers(0, a.keyframes, a.queries).astype(np.int32)
    ss, padded = M.frames_of(m, 8, a.frames, n_matched=a.matched, cap=a.matched)  # the padded [frames][matched] form of the tracking chain
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    d_map = [t(m[k]) for k in M.MAP_KEYS]
    d_feat = [t(m[k]) for k in M.FEAT_KEYS]
    d_q, d_ss, d_sp = t(q), t(ss), t(padded)
    conn_u = torch.full((a.queries, a.cap, 2), -1, dtype=torch.int32, device="cuda")
    out_u = torch.zeros((a.queries, 4), dtype=torch.int32, device="cuda")
    conn_v = torch.full((a.frames, a.cap, 2), -1, dtype=torch.int32, device="cuda")
    out_v = torch.zeros((a.frames, 4), dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    g = CovisibilityGraph(M.TH, M.TH_DEPTH, a.cap, stream=stream.cuda_stream)
    out = dict(keyframes=a.keyframes, points=a.points, observations=len(m["obs"]), mean_obs=float(np.diff(m["obs_start"]).mean()),
               mean_features=float(np.diff(m["feat_start"]).mean()), queries=a.queries, frames=a.frames, matched=a.matched, cap=a.cap,
               long_min_env=os.environ.get("SNK_COVIS_LONG_MIN", ""))
    torch.cuda.synchronize()  # the inputs were uploaded on torch's default stream
    calls = dict(update=lambda: g.update_dev(*d_map, *d_feat, d_q, conn_u, out_u), vote=lambda: g.vote_dev(*d_map, d_ss, d_sp, conn_v, out_v))
    with torch.cuda.stream(stream):
        for name, call in calls.items():
            times = []
            for rep in range(a.reps + 3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call()
                e1.record(stream)
                e1.synchronize()
                if rep >= 3:
                    times.append(e0.elapsed_time(e1))
            out[name + "_ms_median"], out[name + "_ms_min"] = float(np.median(times)), float(np.min(times))
    g.sync()
    res_u, res_v = out_u.cpu().numpy().view(M.RESULT).reshape(-1), out_v.cpu().numpy().view(M.RESULT).reshape(-1)
    got_u, got_v = conn_u.cpu().numpy().view(M.CONN).reshape(a.queries, a.cap), conn_v.cpu().numpy().view(M.CONN).reshape(a.frames, a.cap)
    g.close()
    assert np.all(res_u["status"] == 0) and np.all(res_v["status"] == 0)
    out["update_n_found_median"], out["vote_n_found_median"] = float(np.median(res_u["n_found"])), float(np.median(res_v["n_found"]))

    # the same loops on this host, on a sample, checked against the device's results on the way
    ns = min(a.numpy_sample, a.queries, a.frames)
    t0 = time.perf_counter()
    want = M.update(m, q[:ns], cap=a.cap)
    out["numpy_update_ms_extrapolated"] = (time.perf_counter() - t0) / ns * 1e3 * a.queries
    assert want[0].tobytes() == got_u[:ns].tobytes() and want[1].tobytes() == res_u[:ns].tobytes()
    t0 = time.perf_counter()
    want = M.vote(m, ss[:ns + 1], padded, cap=a.cap)
    out["numpy_vote_ms_extrapolated"] = (time.perf_counter() - t0) / ns * 1e3 * a.frames
    assert want[0].tobytes() == got_v[:ns].tobytes() and want[1].tobytes() == res_v[:ns].tobytes()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
