"""Timing probe of the local-BA-window kernels (does not touch bench.py): the device-resident chain window -> gather for `--queries`
keyframes on a structured map of `--keyframes` keyframes (covis_numpy.make_map, the map of tools/probes/localmap_timing.py) with the
tables snk-scene v1 adds (previous keyframe = the slot before, poses, pixels, octaves, positions, IMU stamps).  The connection store is
what snk_covis_update_batch_dev emits for every keyframe, packed into start / list arrays on the host once.

Prints one JSON line with the time per call of snk_scene_window_batch_dev and snk_scene_gather_batch_dev for the batch and for a single
query (median and minimum of `--reps` calls after three warm-ups, events on the handle's stream), the sizes of the scenes, the statuses,
and the time of the restatement's loops (tests/scene_numpy.py) on this host for a sample of the queries, per query and extrapolated to the
batch; the sample is compared with the device's results on the way.
Kernel statistics: `rocprofv3 --kernel-trace --stats -- python tools/probes/scene_timing.py`.
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
    ap.add_argument("--win-cap", type=int, default=36)
    ap.add_argument("--pt-cap", type=int, default=16384)
    ap.add_argument("--img-cap", type=int, default=512)
    ap.add_argument("--obs-cap", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--numpy-sample", type=int, default=8)
    a = ap.parse_args()
    import torch

    import covis_numpy as CM
    import scene_numpy as M
    from snake_slam_amd import scene as S
    from snake_slam_amd.covis import CovisibilityGraph

    m = CM.make_map(7, a.keyframes, a.points, window=600, p_see=0.55)
    rng = np.random.RandomState(11)
    n_kf, n_feat, n_levels = a.keyframes, len(m["feat_point"]), 8
    quat = rng.randn(n_kf, 4)
    stamps = np.cumsum(rng.choice([0.25, 0.5], n_kf))
    rpc = np.zeros(n_kf, M.RPC_DTYPE)
    rpc["rel_pose"], rpc["weight_translation"] = rng.randn(n_kf, 7), rng.uniform(0.1, 3.0, n_kf)
    m.update(kf_prev=np.arange(-1, n_kf - 1).astype(np.int32), kf_pose=np.concatenate([quat / np.linalg.norm(quat, axis=1, keepdims=True), rng.randn(n_kf, 3)], axis=1),
             feat_uv=rng.uniform(0, 640, (n_feat, 2)).astype(np.float32), feat_octave=rng.randint(0, n_levels, n_feat).astype(np.int32),
             pt_pos=rng.randn(a.points, 3), level_inv_sq_scale=(1.0 / 1.44 ** np.arange(n_levels)).astype(np.float32), kf_time=stamps,
             kf_imu_begin=np.concatenate([[0.0], stamps[:-1]]), kf_imu_end=stamps.copy(), kf_preint_valid=np.ones(n_kf, np.uint8), kf_rpc=rpc)
    m["pt_flags"] = m["pt_flags"] | (rng.rand(a.points) < 0.05).astype(np.uint8) * M.PT_CONST

    def t(x):
        x = np.ascontiguousarray(x)
        return torch.from_numpy(x.view(np.uint8).reshape(x.shape + (-1,)) if x.dtype.fields else x).cuda()

    stream = torch.cuda.Stream()
    # ---- the connection store: every keyframe's list from the device, packed on the host ----
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
    m["conn_list"] = np.ascontiguousarray(np.concatenate([rows[k, :n_conn[k]] for k in range(n_kf)]).astype(np.int32)).view(CM.CONN).reshape(-1)

    gyro, acc = 2.0, 0.5
    b = S.LocalSceneBuilder(dict(win_cap=a.win_cap, gyro_weight=gyro, acc_weight=acc), stream=stream.cuda_stream)
    d = {n: t(np.ascontiguousarray(m[n], dt)) for n, dt, _ in S.MAP_TABLES}
    d_cs, d_cl = t(m["conn_start"]), t(m["conn_list"].view(np.int32).reshape(-1, 2))
    queries = np.linspace(40, n_kf - 1, a.queries).astype(np.int32)
    caps = dict(win_cap=a.win_cap, pt_cap=a.pt_cap, img_cap=a.img_cap, obs_cap=a.obs_cap)

    def buffers(n):
        o = dict(caps)
        for name, dt, cap, tail in S.OUT_ROWS:
            o[name] = torch.zeros((n, caps[cap]) + tail + (np.dtype(dt).itemsize,), dtype=torch.uint8, device="cuda")
        o["result"] = torch.zeros((n, 6), dtype=torch.int32, device="cuda")
        return torch.full((n, a.win_cap), -1, dtype=torch.int32, device="cuda"), torch.zeros((n, 2), dtype=torch.int32, device="cuda"), o

    out = dict(keyframes=n_kf, points=a.points, queries=a.queries, connections_mean=float(n_conn.mean()),
               mean_features=float(np.diff(m["feat_start"]).mean()), **caps)
    kept = {}
    with torch.cuda.stream(stream):
        for label, qs in (("batch", queries), ("single", queries[len(queries) // 2:len(queries) // 2 + 1])):
            d_q = t(qs)
            win, wres, o = buffers(len(qs))
            torch.cuda.synchronize()
            calls = dict(window=lambda: b.window_dev(d_q, d["kf_bad"], d["kf_prev"], d_cs, d_cl, win, wres), gather=lambda: b.gather_dev(d, win, wres, o))
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
                out[f"{label}_{name}_ms_median"], out[f"{label}_{name}_ms_min"] = float(np.median(times)), float(np.min(times))
            kept[label] = (win, wres, o)
    b.sync()
    b.close()
    win, wres, o = kept["batch"]
    res = o["result"].cpu().numpy().view(S.RESULT_DTYPE).reshape(-1)
    out["window_status_counts"] = np.bincount(wres.cpu().numpy()[:, 1], minlength=7).tolist()
    out["gather_status_counts"] = np.bincount(res["status"], minlength=7).tolist()
    ok = res["status"] == M.OK
    for k in ("n_window", "n_img", "n_pt", "n_obs", "n_rpc"):
        out[k + "_median"], out[k + "_max"] = (float(np.median(res[k][ok])), int(res[k][ok].max())) if ok.any() else (0.0, 0)

    # the same loops on this host, on a sample, checked against the device's results on the way
    ns = min(a.numpy_sample, a.queries)
    t_win = t_scene = 0.0
    for s in range(ns):
        t0 = time.perf_counter()
        kfs, status = M.window(m, int(queries[s]), win_cap=a.win_cap)
        t1 = time.perf_counter()
        sc = M.make_scene(m, kfs, a.pt_cap, a.img_cap, a.obs_cap, gyro, acc) if status == M.OK else dict(status=status, n_pt=0, n_obs=0)
        t2 = time.perf_counter()
        t_win, t_scene = t_win + (t1 - t0), t_scene + (t2 - t1)
        assert int(res[s]["status"]) == sc["status"], (s, int(res[s]["status"]), sc["status"])
        if sc["status"] == M.OK:
            assert win[s].cpu().numpy()[:len(kfs)].tolist() == kfs
            assert o["pt_id"][s].cpu().numpy().view(np.int32).reshape(-1)[:sc["n_pt"]].tobytes() == sc["pt_id"].tobytes()
            for name in ("obs_img", "obs_pt", "obs_uv", "obs_weight", "obs_src"):
                n_bytes = sc["n_obs"] * sc[name][:1].nbytes
                assert o[name][s].cpu().numpy().reshape(-1)[:n_bytes].tobytes() == sc[name].tobytes(), (s, name)
    out["numpy_window_ms_per_query"], out["numpy_scene_ms_per_query"] = t_win / ns * 1e3, t_scene / ns * 1e3
    out["numpy_window_ms_extrapolated"], out["numpy_scene_ms_extrapolated"] = t_win / ns * 1e3 * a.queries, t_scene / ns * 1e3 * a.queries
    print(json.dumps(out))


if __name__ == "__main__":
    main()
