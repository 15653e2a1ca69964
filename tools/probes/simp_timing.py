"""Timing probe of the keyframe-culling kernels (does not touch bench.py): the device forms snk_simp_stats_batch_dev and
snk_simp_decide_batch_dev for `--queries` keyframes and for a single one on a structured map of `--keyframes` keyframes
(covis_numpy.make_map, the map of tools/probes/scene_timing.py) with the tables snk-simp v1 adds (poses, octaves, positions, cull
factors).  The connection store is what snk_covis_update_batch_dev emits for every keyframe, packed into start / list arrays on the host
once; the cached medians are stage 1's for every keyframe.

Prints one JSON line with the time per call (median, minimum and maximum of `--reps` calls after three warm-ups, events on the handle's
stream), the graphs' sizes, the reasons and statuses, and the time of the restatement's loops (tests/simp_numpy.py) on this host for a
sample of the queries, per query; the sample is compared with the device's results on the way.
Kernel statistics: `rocprofv3 --kernel-trace --stats -- python tools/probes/simp_timing.py`.
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
    ap.add_argument("--keyframes", type=int, default=10000)
    ap.add_argument("--points", type=int, default=400000)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--conn-cap", type=int, default=64)
    ap.add_argument("--feat-cap", type=int, default=1024)
    ap.add_argument("--node-cap", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--numpy-sample", type=int, default=8)
    a = ap.parse_args()
    import torch

    import covis_numpy as CM
    import simp_numpy as M
    from snake_slam_amd import simp as S
    from snake_slam_amd.covis import CovisibilityGraph

    m = CM.make_map(7, a.keyframes, a.points, window=600, p_see=0.55)
    rng = np.random.RandomState(11)
    n_kf, n_feat = a.keyframes, len(m["feat_point"])
    quat = rng.randn(n_kf, 4)
    m.update(kf_pose=np.concatenate([quat / np.linalg.norm(quat, axis=1, keepdims=True), rng.randn(n_kf, 3)], axis=1),
             feat_octave=rng.randint(0, 8, n_feat).astype(np.int32), pt_pos=rng.randn(a.points, 3) + np.array([0, 0, 8.0]),
             kf_cull_factor=rng.choice([1.0, 1.5, 2.5], n_kf).astype(np.float32))

    def t(x):
        x = np.ascontiguousarray(x)
        return torch.from_numpy(x.view(np.int32).reshape(len(x), -1) if x.dtype.fields else x).cuda()

    stream = torch.cuda.Stream()
    g = CovisibilityGraph(CM.TH, CM.TH_DEPTH, a.conn_cap, stream=stream.cuda_stream)
    conn_u = torch.full((n_kf, a.conn_cap, 2), -1, dtype=torch.int32, device="cuda")
    out_u = torch.zeros((n_kf, 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g.update_dev(*[t(m[k]) for k in CM.MAP_KEYS], *[t(m[k]) for k in CM.FEAT_KEYS], t(np.arange(n_kf, dtype=np.int32)), conn_u, out_u)
    g.sync()
    g.close()
    n_conn = out_u.cpu().numpy()[:, 1]
    rows = conn_u.cpu().numpy()
    m["conn_start"] = np.concatenate([[0], np.cumsum(n_conn)]).astype(np.int32)
    m["conn_list"] = np.ascontiguousarray(np.concatenate([rows[k, :n_conn[k]] for k in range(n_kf)]).astype(np.int32)).view(M.CONN_DTYPE).reshape(-1)

    params = dict(stereo=1, th_depth=CM.TH_DEPTH, feat_cap=a.feat_cap, node_cap=a.node_cap)
    c = S.KeyframeCuller(params, stream=stream.cuda_stream)
    d = {n: t(np.ascontiguousarray(m[n], dt)) for n, dt, _ in S.MAP_TABLES}
    # the cache: stage 1 for every keyframe, once
    all_q, all_st = t(np.arange(n_kf, dtype=np.int32)), torch.zeros((n_kf, 7), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    c.stats_dev(d, all_q, all_st)
    c.sync()
    st_all = all_st.cpu().numpy().view(M.STATS_DTYPE).reshape(-1)
    m["kf_median_depth"] = np.where((st_all["status"] == M.OK) & (st_all["n_depth"] > 0), st_all["median_depth"].astype(np.float64), -1.0)
    gd = dict(kf_bad=d["kf_bad"], kf_pose=d["kf_pose"], kf_cull_factor=t(m["kf_cull_factor"]), kf_median_depth=t(m["kf_median_depth"]), kf_prev=None,
              kf_next=None, kf_time=None, conn_start=t(m["conn_start"]), conn_list=t(m["conn_list"]))
    queries = np.linspace(40, n_kf - 1, a.queries).astype(np.int32)

    out = dict(keyframes=n_kf, points=a.points, queries=a.queries, connections_mean=float(n_conn.mean()),
               mean_features=float(np.diff(m["feat_start"]).mean()), mean_list=float(np.diff(m["obs_start"]).mean()), **params)
    kept = {}
    with torch.cuda.stream(stream):
        for label, qs in (("batch", queries), ("single", queries[len(queries) // 2:len(queries) // 2 + 1])):
            d_q = t(qs)
            st, vd = torch.zeros((len(qs), 7), dtype=torch.int32, device="cuda"), torch.zeros((len(qs), 8), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            calls = dict(stats=lambda: c.stats_dev(d, d_q, st), decide=lambda: c.decide_dev(gd, d_q, st, vd))
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
                out[f"{label}_{name}_ms_median"], out[f"{label}_{name}_ms_min"], out[f"{label}_{name}_ms_max"] = (
                    float(np.median(times)), float(np.min(times)), float(np.max(times)))
            kept[label] = (st, vd)
    c.sync()
    c.close()
    st, vd = (x.cpu().numpy() for x in kept["batch"])
    st, vd = st.view(M.STATS_DTYPE).reshape(-1), vd.view(M.VERDICT_DTYPE).reshape(-1)
    out["stats_status_counts"] = np.bincount(st["status"], minlength=5).tolist()
    out["verdict_status_counts"] = np.bincount(vd["status"], minlength=5).tolist()
    out["reason_counts"] = np.bincount(vd["reason"], minlength=12).tolist()
    ok = vd["status"] == M.OK
    out["n_nodes_median"], out["n_nodes_max"] = (float(np.median(vd["n_nodes"][ok])), int(vd["n_nodes"][ok].max())) if ok.any() else (0.0, 0)
    out["n_depth_median"] = float(np.median(st["n_depth"][st["status"] == M.OK])) if (st["status"] == M.OK).any() else 0.0

    # the same loops on this host, on a sample, checked against the device's results on the way
    ns = min(a.numpy_sample, a.queries)
    graph = dict(m, kf_prev=None, kf_next=None, kf_time=None)
    t_stats = t_decide = 0.0
    for s in range(ns):
        q = int(queries[s])
        t0 = time.perf_counter()
        ws = M.stats(m, q, 3, 1, CM.TH_DEPTH, a.feat_cap)
        t1 = time.perf_counter()
        wv = M.decide(graph, q, M.stats_array([ws])[0], {}, a.node_cap)
        t2 = time.perf_counter()
        t_stats, t_decide = t_stats + (t1 - t0), t_decide + (t2 - t1)
        assert all(st[k][s] == ws[k] or (np.isnan(st[k][s]) and np.isnan(ws[k])) for k in M.STATS_DTYPE.names), (s, st[s], ws)
        assert all(vd[k][s] == wv[k] for k in ("reason", "cull", "n_nodes", "n_root_edges", "weakest_link", "status")), (s, vd[s], wv)
    out["numpy_stats_ms_per_query"], out["numpy_decide_ms_per_query"] = t_stats / ns * 1e3, t_decide / ns * 1e3
    print(json.dumps(out))


if __name__ == "__main__":
    main()
