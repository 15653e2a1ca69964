"""Timing probe of the bag-of-words place recognition (does not touch bench.py): synthetic k = 10, L = 6 vocabulary.

Prints one JSON line with the time (median of `--reps` after warm-up, events on the handles' stream) of (a) the transform of 1024
frames x 1000 features, (b) one query and 64 batched queries against 1 000 and 10 000 keyframes, (c) MatchBoW for 64 keyframe pairs;
and beside (a) the time of the CPU build of bow_core.hpp (tests/cpp/bow_core_driver.cpp, plain g++ -O2, one thread) on the same host,
extrapolated from `--cpu-frames` frames -- the only baseline there is.  Kernel statistics: run it under `rocprofv3 --kernel-trace
--stats -- python tools/probes/bow_timing.py`.
"""
import argparse
import json
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]


def big_vocab(rng, k=10, L=6):
    """a regular tree as flat arrays, vectorised: a child is its parent with about 96 >> depth (at least 6) random bits flipped"""
    counts = [k ** d for d in range(L + 1)]
    n = sum(counts)
    desc = np.zeros((n, 4), np.uint64)
    desc[0] = rng.integers(0, 2 ** 64, 4, dtype=np.uint64)
    first, start = 0, 1
    for d in range(L):
        kids = np.repeat(desc[first: first + counts[d]], k, axis=0)
        rows = np.arange(len(kids))
        for _ in range(max(6, 96 >> d)):  # bits drawn with replacement: a few cancel, which does not matter here
            kids[rows, rng.integers(0, 4, len(kids))] ^= np.left_shift(np.uint64(1), rng.integers(0, 64, len(kids)).astype(np.uint64))
        desc[start: start + counts[d + 1]] = kids
        first, start = start, start + counts[d + 1]
    inner = n - counts[L]
    child_count = np.where(np.arange(n) < inner, k, 0).astype(np.int32)
    child_start = np.minimum(np.arange(n) * k, n - 1).astype(np.int32)
    word_id = np.where(np.arange(n) < inner, -1, np.arange(n) - inner).astype(np.int32)
    weight = np.where(np.arange(n) < inner, 0.0, rng.uniform(0.5, 9.0, n))
    return dict(child_start=child_start, child_count=child_count, children=np.arange(1, n, dtype=np.int32), desc=desc,
                word_id=word_id, weight=weight), inner


def timed(torch, stream, fn, reps):
    times = []
    for r in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        if r >= 3:
            times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(np.min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu-frames", type=int, default=4)
    a = ap.parse_args()
    import torch

    from snake_slam_amd.bow import KeyframeDatabase, LoopMatcher, Vocabulary, desc_frames_dev

    rng = np.random.default_rng(1)
    arrays, inner = big_vocab(rng)
    leaves = arrays["desc"][inner:]
    stream = torch.cuda.Stream()
    G = Vocabulary.from_arrays(arrays, stream=stream.cuda_stream)
    lm = LoopMatcher(stream=stream.cuda_stream)
    out = dict(vocabulary_words=G.size(), frames=a.frames, features=a.features)

    # frames of "places": a place owns 600 leaves, a frame draws its features from them and flips 3 bits
    n_places = max(a.frames // 8, 1)
    pools = rng.integers(0, len(leaves), (n_places, 600))
    pick = np.take_along_axis(pools[np.arange(a.frames) % n_places], rng.integers(0, 600, (a.frames, a.features)), axis=1)
    desc = leaves[pick].copy()
    for _ in range(3):
        desc[..., rng.integers(0, 4)] ^= np.left_shift(np.uint64(1), rng.integers(0, 64, desc.shape[:2]).astype(np.uint64))
    desc_dev = torch.from_numpy(desc.view(np.int64)).cuda()
    n_dev = torch.full((a.frames,), a.features, dtype=torch.int32, device="cuda")
    frames = desc_frames_dev(n_dev, desc_dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        t = G.transform_batch_dev(frames, 4)
        out["transform_ms_median"], out["transform_ms_min"] = timed(torch, stream, lambda: G.transform_batch_dev(frames, 4, t), a.reps)
        for n_kf in (1000, 10000):
            db = KeyframeDatabase(G, max_keyframes=n_kf, max_words=a.features)
            rows = np.arange(n_kf) % a.frames
            for lo in range(0, n_kf, a.frames):
                sel = torch.from_numpy(rows[lo: lo + a.frames]).cuda()
                db.add_batch_dev(np.arange(lo, lo + len(sel)), t["words"][sel].contiguous(), t["values"][sel].contiguous(), t["n_words"][sel].contiguous())
            for q in (1, 64):
                w, v, nw = t["words"][:q].contiguous(), t["values"][:q].contiguous(), t["n_words"][:q].contiguous()
                res = db.query_batch_dev(w, v, nw, max_candidates=10)
                key = f"query_{q}_of_{n_kf}_ms"
                out[key + "_median"], out[key + "_min"] = timed(torch, stream, lambda: db.query_batch_dev(w, v, nw, max_candidates=10, out=res), a.reps)
            stream.synchronize()
            out[f"candidates_of_{n_kf}"] = float(res["n"].float().mean())
            db.close()
        # MatchBoW: 64 pairs of frames of the same place
        P = 64
        i1, i2 = np.arange(P), (np.arange(P) + n_places) % a.frames
        sub = lambda x, i: {k: x[k][torch.from_numpy(i).cuda()].contiguous() for k in ("node_id", "node_start", "features", "n_nodes")}  # noqa: E731
        d1, d2 = desc_dev[torch.from_numpy(i1).cuda()].contiguous(), desc_dev[torch.from_numpy(i2).cuda()].contiguous()
        n64 = n_dev[:P].contiguous()
        has = torch.ones((P, a.features), dtype=torch.uint8, device="cuda")
        m12 = torch.zeros((P, a.features), dtype=torch.int32, device="cuda")
        pairs, n_pairs = torch.zeros((P, a.features, 2), dtype=torch.int32, device="cuda"), torch.zeros(P, dtype=torch.int32, device="cuda")
        b1, b2 = sub(t, i1), sub(t, i2)
        f1, f2 = desc_frames_dev(n64, d1), desc_frames_dev(n64, d2)
        torch.cuda.synchronize()
        out["match_bow_64_ms_median"], out["match_bow_64_ms_min"] = timed(
            torch, stream, lambda: lm.match_bow_batch_dev(f1, f2, has, has, b1, b2, m12, pairs, n_pairs, 50, 0.75), a.reps)
        out["mean_matches"] = float(n_pairs.float().mean())
    lm.close()
    G.close()

    # the CPU build of bow_core.hpp, one thread, on --cpu-frames frames
    with tempfile.TemporaryDirectory() as tmp:
        d = Path(tmp)
        exe = d / "bow_core_driver"
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", f"-I{ROOT / 'snake_slam_amd' / 'csrc'}",
                        str(ROOT / "tests" / "cpp" / "bow_core_driver.cpp"), "-o", str(exe)], check=True)
        for k, dt in (("child_start", np.int32), ("child_count", np.int32), ("children", np.int32), ("desc", np.uint64), ("weight", np.float64)):
            np.ascontiguousarray(arrays[k], dt).tofile(d / f"v_{k}.bin")
        arrays["word_id"].tofile(d / "v_word.bin")
        desc[: a.cpu_frames].tofile(d / "desc.bin")
        r = subprocess.run([str(exe), str(d), "time", "4", "3"], capture_output=True, text=True, check=True)
        out["cpu_descent_ms_per_frame"] = float(r.stdout.strip()) / a.cpu_frames * 1e3
        out["cpu_descent_ms_per_batch_extrapolated"] = out["cpu_descent_ms_per_frame"] * a.frames
    print(json.dumps(out))


if __name__ == "__main__":
    main()
