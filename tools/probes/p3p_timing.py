"""Timing probe of the P3P-RANSAC (does not touch bench.py): 1024 frames x 300 pairs x 250 iterations.

Prints one JSON line with (a) the time per batch of snk_p3p_ransac_frame_batch_dev (median of `--reps` batches after warm-up, events
on the handle's stream), (b) the lockstep step time of MultiSequenceTracker with and without ransac (median step over `--steps`
steps, wall clock around a synchronised run), (c) the numpy restatement's time per frame on this host (extrapolated to the batch).
Kernel statistics: run it under `rocprofv3 --kernel-trace --stats -- python tools/probes/p3p_timing.py --no-tracker`.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--pairs", type=int, default=300)
    ap.add_argument("--iterations", type=int, default=250)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--sequences", type=int, default=64)
    ap.add_argument("--no-tracker", action="store_true")
    a = ap.parse_args()
    import torch

    import p3p_numpy as P
    from snake_slam_amd import synth
    from snake_slam_amd.sequence import MultiSequenceTracker
    from snake_slam_amd.tracking import P3PRansac
    from test_p3p_chain_gpu import CAM, frames_view, host_pairs, make_frames, to_dev

    out = dict(frames=a.frames, pairs=a.pairs, iterations=a.iterations)
    F = make_frames(a.frames, a.pairs, 1)
    D = to_dev(F, torch)
    fp0 = D["frame_pt"].clone()
    poses = torch.zeros((a.frames, 7), dtype=torch.float64, device="cuda")
    inl = torch.zeros(a.frames, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    s = P3PRansac(a.iterations, P.THRESHOLD, 1, stream=stream.cuda_stream)
    fd = frames_view(D)
    times = []
    torch.cuda.synchronize()  # the inputs were uploaded on torch's default stream
    with torch.cuda.stream(stream):
        for r in range(a.reps + 3):
            D["frame_pt"].copy_(fp0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            s.solve_frame_batch_dev(fd, CAM, D["pts"], D["frame_pt"], D["n_pts"], poses, inl)
            e1.record(stream)
            e1.synchronize()
            if r >= 3:
                times.append(e0.elapsed_time(e1))
    s.close()
    out["p3p_batch_ms_median"], out["p3p_batch_ms_min"] = float(np.median(times)), float(np.min(times))
    out["mean_inliers"] = float(inl.float().mean())
    t0 = time.perf_counter()
    nf = 4
    for b in range(nf):
        _, w, q = host_pairs(F, b)
        P.ransac(w, q, a.iterations, P.THRESHOLD, 1, problem=b)
    out["numpy_ms_per_frame"] = (time.perf_counter() - t0) / nf * 1e3
    out["numpy_ms_per_batch_extrapolated"] = out["numpy_ms_per_frame"] * a.frames
    if not a.no_tracker:
        w, h, orb, cam = 640, 400, dict(nfeatures=800, scale_factor=1.2, n_levels=4, ini_th_fast=20, min_th_fast=7), (400.0, 400.0, 320.0, 200.0, 100.0)
        S, T = a.sequences, a.steps + 2
        base = [list(synth.sequence_frames(10 + k, T, w, h, n_rects=300)) for k in range(4)]
        for name, flag in (("step_ms_ransac_off", False), ("step_ms_ransac_on", True)):
            mt = MultiSequenceTracker(cam, S, T, orb=orb, width=w, height=h, ransac=flag)
            staged = [mt.stage([base[k % 4][t][0] for k in range(S)], [base[k % 4][t][1] for k in range(S)]) for t in range(T)]
            for t in range(2):
                mt.process_staged(staged[t], float(t))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(2, T):
                mt.process_staged(staged[t], float(t))
            torch.cuda.synchronize()
            out[name] = (time.perf_counter() - t0) / (T - 2) * 1e3
            mt.close()
        out["sequences"] = S
    print(json.dumps(out))


if __name__ == "__main__":
    main()
