"""FullBA(4) (PCG 40; GlobalBundleAdjustment.cpp:32-43) in the explicit and the implicit Schur form at map sizes: wall time per solve
(after one warm-up solve, snk_ba_reset in between, synchronised; global BA with a one-launch PCG never records a graph, so every
timed solve runs the form the handle reports), the PCG form before and after the timed solves and the device bytes one handle holds after its hand-over
(torch.cuda.mem_get_info before / after).  Every measurement runs in a child process of its own under a time limit; the run stops at
the first child that fails.  Writes profiles/r07/gba_implicit_time.json.

    python tools/gba_implicit_time.py [--sizes 300,1068,3202,10000] [--reps 3] [--out profiles/r07/gba_implicit_time.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
EXPLICIT_MAX_KF = 3202  # the dense S of 10 000 keyframes would be 28.8 GB


def child(n_kf, explicit, reps):
    import numpy as np
    import torch

    sys.path.insert(0, str(ROOT))
    from snake_slam_amd import synth
    from snake_slam_amd.ba import BARec, gba_options

    sc = synth.ba_scene(n_kf=n_kf, n_pt=12 * n_kf, obs_per_pt=6, seed=900 + n_kf, n_fixed=1)[0]
    torch.cuda.init()
    free0 = torch.cuda.mem_get_info(0)[0]
    ba = BARec(gba_options(max_iterations=4, max_pcg_iterations=40), explicit_schur=explicit)
    t0 = time.perf_counter()
    ba.create(sc)
    ba.sync()
    handover_ms = (time.perf_counter() - t0) * 1e3
    dev_bytes = free0 - torch.cuda.mem_get_info(0)[0]
    form = ba.pcg_form()
    ci, cf = ba.solve(4)  # warm-up (and the plain-launch first solve)
    times = []
    for _ in range(reps):
        ba.reset()
        ba.sync()
        t0 = time.perf_counter()
        ci, cf = ba.solve(4)
        times.append((time.perf_counter() - t0) * 1e3)
    _, _, pcg = ba.state(0)
    form_after = ba.pcg_form()  # a refused cooperative launch would show here
    ba.close()
    return dict(keyframes=n_kf, points=12 * n_kf, observations=int(len(sc["obs_img"])), form="explicit" if explicit else "implicit",
                pcg_form=list(form), pcg_form_after=list(form_after), handover_ms=round(handover_ms, 2), device_bytes=int(dev_bytes), fullba4_ms=[round(t, 3) for t in times],
                fullba4_ms_median=round(float(np.median(times)), 3), cost_initial=float(ci[0]), cost_final=float(cf[0]), pcg_iterations=int(pcg))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="300,1068,3202,10000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r07" / "gba_implicit_time.json"))
    ap.add_argument("--child", nargs=3, metavar=("N_KF", "EXPLICIT", "REPS"))
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(int(a.child[0]), a.child[1] == "1", int(a.child[2]))), flush=True)
        return 0
    rows = []
    for n in [int(s) for s in a.sizes.split(",")]:
        for explicit in ((True, False) if n <= EXPLICIT_MAX_KF else (False,)):
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, str(Path(__file__).resolve()), "--child", str(n),
                   "1" if explicit else "0", str(a.reps)]
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(ROOT), env=dict(os.environ, PYTHONPATH=str(ROOT)))
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                print(f"[gba_implicit_time] {n} keyframes explicit={explicit}: status {r.returncode}\n{r.stderr[-2000:]}", file=sys.stderr)
                rows.append(dict(keyframes=n, form="explicit" if explicit else "implicit", failed=r.returncode))
                Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                Path(a.out).write_text(json.dumps(rows, indent=1) + "\n")
                return 1
            rows.append(json.loads(line[0][len("RESULT "):]))
            print(json.dumps(rows[-1]), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rows, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
