"""Timing probe of the two BA hand-overs (does not touch bench.py): `--windows` windows of the benchmark shape (20 keyframes x 2000 points
x 8 observations; `--distinct` different scenes, repeated) are loaded into ONE handle, in one process,
  * through snk_ba_set_problems from host arrays -- the yardstick, and
  * through snk_ba_set_problems_dev from device rows that hold the same data.
Each timing is the wall time of the call plus the wait for the handle's stream (snk_ba_sync), bracketed by synchronisation: median, minimum
and maximum of `--reps` repeats after `--warmups` warm-ups, the two forms alternating.  A solve after each form's last load gives the costs,
which must be the same bytes.  Prints one JSON line.  Then a child process repeats one load of each form under SNK_BA_PROFILE_CREATE=1
(read once per process) and its [snk_ba_set_problems] lines follow: the host sections, the device stage and the read-back, and the bytes
that crossed the bus in each direction."""
import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--keyframes", type=int, default=20)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--obs-per-point", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--profile-child", action="store_true")
    a = ap.parse_args()
    import torch

    import handover_numpy as M
    from snake_slam_amd import synth
    from snake_slam_amd.ba import BARec, lba_options

    base = [synth.ba_scene(n_kf=a.keyframes, n_pt=a.points, obs_per_pt=a.obs_per_point, seed=900 + k)[0] for k in range(a.distinct)]
    scenes = [base[b % a.distinct] for b in range(a.windows)]
    K, bf = base[0]["K"], base[0]["bf"]
    o = M.pad_rows(scenes)
    host = [M.row_scene(o, s, K, bf) for s in range(a.windows)]
    dev = M.rows_to_device(o)
    torch.cuda.synchronize()
    ba = BARec(lba_options())

    def load(form):
        ba.sync()
        t0 = time.perf_counter()
        if form == "host":
            ba.create(host)
        else:
            ba.create_dev(dev, K, bf)
        call = ba.last_set_problems_ms
        ba.sync()
        return (time.perf_counter() - t0) * 1e3 - (ba.last_pack_ms if form == "host" else 0.0), call

    if a.profile_child:
        for form in ("host", "dev", "host", "dev"):  # the second pair: buffers and pinned lists at their sizes
            print(f"[probe] {form}", file=sys.stderr, flush=True)
            load(form)
        ba.close()
        return
    times = {"host": [], "dev": []}
    for r in range(a.warmups + a.reps):
        for form in ("host", "dev"):
            t = load(form)
            if r >= a.warmups:
                times[form].append(t)
    costs = {}
    for form in ("host", "dev"):
        load(form)
        costs[form] = np.concatenate(ba.solve()).tobytes()
    ba.close()
    n_obs = int(o["result"]["n_obs"].sum())
    out = dict(windows=a.windows, observations=n_obs, same_costs=costs["host"] == costs["dev"], reps=a.reps)
    for form in ("host", "dev"):
        total = np.array([t[0] for t in times[form]])
        call = np.array([t[1] for t in times[form]])
        out[form] = dict(median_ms=round(float(np.median(total)), 3), min_ms=round(float(total.min()), 3), max_ms=round(float(total.max()), 3),
                         call_median_ms=round(float(np.median(call)), 3))
    out["dev_faster"] = bool(out["dev"]["max_ms"] < out["host"]["min_ms"])  # only if the ranges do not overlap
    print(json.dumps(out), flush=True)
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--profile-child"] + [x for x in sys.argv[1:]],
                       env=dict(os.environ, SNK_BA_PROFILE_CREATE="1"), capture_output=True, text=True, timeout=900)
    print(r.stderr[-6000:] if r.returncode == 0 else f"profile child failed: {r.stderr[-2000:]}", flush=True)


if __name__ == "__main__":
    main()
