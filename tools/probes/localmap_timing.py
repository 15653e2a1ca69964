"""Timing probe of the local-map kernels (does not touch bench.py): the device-resident chain vote -> select -> gather for `--frames`
frames on a structured map of `--keyframes` keyframes (covis_numpy.make_map, the map of tools/probes/covis_timing.py).  The connection
store is what snk_covis_update_batch_dev emits for every keyframe, packed into start / list arrays on the host once.

Prints one JSON line with the time per call of snk_lmap_select_batch_dev and snk_lmap_gather_batch_dev (median and minimum of `--reps`
calls after three warm-ups, events on the handles' stream), the sizes of the lists and maps, the statuses, and the restatement's time
on this host for a sample of the frames, extrapolated to the call; the sample is compared with the device's results on the way.
Kernel statistics: `rocprofv3 --kernel-trace --stats -- python tools/probes/localmap_timing.py`.
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
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--matched", type=int, default=300)
    ap.add_argument("--vote-cap", type=int, default=512)
    ap.add_argument("--conn-cap", type=int, default=64)
    ap.add_argument("--kf-cap", type=int, default=64)
    ap.add_argument("--pts-cap", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--numpy-sample", type=int, default=16)
    a = ap.parse_args()
    import torch

    import covis_numpy as CM
    import localmap_numpy as M
    from snake_slam_amd.covis import CovisibilityGraph
    from snake_slam_amd.localmap import LocalMapBuilder

    m = CM.make_map(7, a.keyframes, a.points, window=600, p_see=0.55)
    ss, padded = CM.frames_of(m, 8, a.frames, n_matched=a.matched, cap=a.matched)
    m.update(M.point_tables(a.points), pt_last_seen=np.full(a.points, -1, np.int32))
    frame_id = np.arange(a.frames, dtype=np.int32)

    def t(x):
        x = np.ascontiguousarray(x)
        return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda()

    stream = torch.cuda.Stream()
    d_map = [t(m[k]) for k in CM.MAP_KEYS]
    d_feat = [t(m[k]) for k in CM.FEAT_KEYS]
    # ---- the connection store: every keyframe's list from the device, packed on the host ----
    g = CovisibilityGraph(CM.TH, CM.TH_DEPTH, a.conn_cap, stream=stream.cuda_stream)
    conn_u = torch.full((a.keyframes, a.conn_cap, 2), -1, dtype=torch.int32, device="cuda")
    out_u = torch.zeros((a.keyframes, 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g.update_dev(*d_map, *d_feat, t(np.arange(a.keyframes, dtype=np.int32)), conn_u, out_u)
    g.sync()
    n_conn = out_u.cpu().numpy()[:, 1]
    rows = conn_u.cpu().numpy()
    conn_start = np.concatenate([[0], np.cumsum(n_conn)]).astype(np.int32)
    conn_list = np.concatenate([rows[k, :n_conn[k]] for k in range(a.keyframes)]).astype(np.int32)
    # ---- the votes ----
    g.cap = a.vote_cap
    d_ss, d_sp = t(ss), t(padded)
    conn = torch.full((a.frames, a.vote_cap, 2), -1, dtype=torch.int32, device="cuda")
    vote = torch.zeros((a.frames, 4), dtype=torch.int32, device="cuda")
    g.vote_dev(*d_map, d_ss, d_sp, conn, vote)
    g.sync()
    g.close()

    params = dict(kf_cap=a.kf_cap, seed=1)
    b = LocalMapBuilder(params, stream=stream.cuda_stream)
    d_cs, d_cl, d_fid = t(conn_start), t(conn_list), t(frame_id)
    d_pts = {k: t(m[k]) for k in M.POINT_KEYS}
    d_ls = t(m["pt_last_seen"])
    local = torch.full((a.frames, a.kf_cap), -1, dtype=torch.int32, device="cuda")
    sel = torch.zeros((a.frames, 5), dtype=torch.int32, device="cuda")
    lm = torch.zeros((a.frames, a.pts_cap, 96), dtype=torch.uint8, device="cuda")
    ids = torch.zeros((a.frames, a.pts_cap), dtype=torch.int32, device="cuda")
    n_pts = torch.zeros(a.frames, dtype=torch.int32, device="cuda")
    gres = torch.zeros((a.frames, 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    calls = dict(select=lambda: b.select_dev(conn, vote, d_map[0], d_cs, d_cl, d_fid, local, sel),
                 gather=lambda: b.gather_dev(d_feat[0], d_feat[1], d_map[3], d_ls, d_pts, d_fid, local, sel, d_ss, d_sp, a.pts_cap, lm, ids, n_pts, gres))
    out = dict(keyframes=a.keyframes, points=a.points, frames=a.frames, matched=a.matched, vote_cap=a.vote_cap, kf_cap=a.kf_cap, pts_cap=a.pts_cap,
               connections_mean=float(n_conn.mean()), mean_features=float(np.diff(m["feat_start"]).mean()))
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
    b.sync()
    b.close()
    r_sel, r_g = sel.cpu().numpy().view(M.SELECT).reshape(-1), gres.cpu().numpy().view(M.GATHER).reshape(-1)
    r_vote = vote.cpu().numpy().view(M.VOTE).reshape(-1)
    out["vote_n_found_median"] = float(np.median(r_vote["n_found"]))
    out["select_status_counts"] = np.bincount(r_sel["status"], minlength=6).tolist()
    out["gather_status_counts"] = np.bincount(r_g["status"], minlength=6).tolist()
    ok = r_g["status"] == M.OK
    out["n_local_median"] = float(np.median(r_sel["n_local"][r_sel["status"] == M.OK])) if np.any(r_sel["status"] == M.OK) else 0.0
    out["n_pts_median"], out["n_pts_max"] = (float(np.median(r_g["n_pts"][ok])), int(r_g["n_pts"][ok].max())) if ok.any() else (0.0, 0)

    # the same loops on this host, on a sample, checked against the device's results on the way
    ns = min(a.numpy_sample, a.frames)
    h_conn, h_vote = conn.cpu().numpy().view(M.CONN).reshape(a.frames, a.vote_cap)[:ns], r_vote[:ns]
    t0 = time.perf_counter()
    w_local, w_sel = M.select(h_conn, h_vote, m["kf_bad"], conn_start, conn_list.view(M.CONN).reshape(-1), frame_id[:ns], params)
    out["numpy_select_ms_extrapolated"] = (time.perf_counter() - t0) / ns * 1e3 * a.frames
    assert w_local.tobytes() == local[:ns].cpu().numpy().tobytes() and w_sel.tobytes() == r_sel[:ns].tobytes()
    t0 = time.perf_counter()
    w = M.gather(m, frame_id[:ns], w_local, w_sel, ss[:ns + 1], padded, a.pts_cap)
    out["numpy_gather_ms_extrapolated"] = (time.perf_counter() - t0) / ns * 1e3 * a.frames
    assert w[1].tobytes() == ids[:ns].cpu().numpy().tobytes() and w[3].tobytes() == r_g[:ns].tobytes()
    got_lm = lm[:ns].cpu().numpy().reshape(ns, a.pts_cap, 96)
    for s in range(ns):
        assert got_lm[s, :w[2][s]].tobytes() == w[0][s, :w[2][s]].tobytes()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
