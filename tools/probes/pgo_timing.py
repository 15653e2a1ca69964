"""Times snk_pgo_solve on rings of 300, 1 000 and 5 000 vertices with 10 neighbours each (se3 and sim3), beside the scipy sparse direct
restatement (tests/pgo_numpy.py) on the same host.  The parent process starts ONE child that opens the GPU and waits for it with a time
limit; nothing is claimed in advance -- whoever runs it writes the numbers into profiles/NOTES.md.

    python tools/probes/pgo_timing.py [--limit SECONDS] [--no-cpu]
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]


def child(cpu: bool) -> None:
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
    import pgo_numpy as P
    from snake_slam_amd.loop import PoseGraphOptimizer

    for n in (300, 1000, 5000):
        for fix in (1, 0):
            G = P.prepare(P.ring(n, 10, 100 + n, fix))
            o = PoseGraphOptimizer()
            try:
                times = []
                for _ in range(4):  # the first call pays allocations
                    o.set_graph(G["poses_measure"], G["constant"], G["edges"], G["weights"], G["meas"], G["start"], fix)
                    t = time.perf_counter()
                    res = o.solve()
                    times.append(time.perf_counter() - t)
                line = dict(vertices=n, edges=int(len(G["edges"])), fix_scale=fix, gpu_ms=round(1e3 * sorted(times[1:])[1], 3), **res)
            finally:
                o.close()
            if cpu:
                t = time.perf_counter()
                _, info = P.optimise(G)
                line.update(cpu_ms=round(1e3 * (time.perf_counter() - t), 1), cpu_lm_iterations=info["lm_iterations"], cpu_cost_final=info["cost_final"])
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--limit", type=float, default=240.0)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(not a.no_cpu)
    else:
        r = subprocess.run([sys.executable, __file__, "--child"] + (["--no-cpu"] if a.no_cpu else []), timeout=a.limit)
        sys.exit(r.returncode)
