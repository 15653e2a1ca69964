"""Inputs of tests/test_knn2_wide_gpu.py, seeded, and the child process that runs them: SNK_BF_MFMA_WIDE is read once per process, so
`python knn2_wide_cases.py OUT.npz [case ...]` runs the named cases (default: all) on the device under whatever the environment
forces and writes what came back; the test builds the same inputs and compares with the oracle.

Q = 64 queries per wavefront, W = 256 per workgroup, T = 32 trains per tile of bf_knn2_mfma_kernel<2, .>; SHORT_NT = 8192 is the train
capacity up to which the kernel runs on 13-bit keys (snake_slam_amd/csrc/dispatch.hpp)."""
import sys
from pathlib import Path

import numpy as np

TESTS = Path(__file__).resolve().parent
for p in (str(TESTS.parent), str(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)

import forms  # noqa: E402
from helpers import SEED, rand_desc  # noqa: E402

Q, W, T, SHORT_NT = 64, 256, 32, 8192
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
EDGE_NQ, EDGE_NT = [Q - 1, Q, Q + 1, W - 1, W, W + 1], [T - 1, T, T + 1, 2 * T + 1]
BATCH_NQ = [W + 1, 0, 1, Q - 1, Q, Q + 1, W - 1, W, 400]          # W + 1: one query in the second workgroup; 400 -> W + 1 (clamped)
BATCH_NT = [2 * T + 1, 2 * T, 0, 1, T - 1, T, T + 1, 2 * T - 1, 1000]  # 1000 -> 2 T + 1 (clamped)
TIE_ROWS = {"tiles": (5, 70), "halves": (33, 38), "three": (2, 36, 67)}  # duplicates: two tiles; rows 1 and 6 of tile 1 (lane halves 0 / 1)


def flip(d, bits):
    d = d.copy()
    for b in bits:
        d[b >> 6] ^= np.uint64(1) << np.uint64(b & 63)
    return d


def host_edges():
    rng = np.random.default_rng(SEED + 6401)
    out = {}
    for nq in EDGE_NQ:
        for nt in EDGE_NT:
            q, t = rand_desc(rng, nq), rand_desc(rng, nt)
            t[nt - 1], q[0], q[nq - 1] = t[0], t[0], t[min(3, nt - 1)]  # ties decided by the index, at both ends of the query range
            out[f"edge_{nq}_{nt}"] = ("host", q, t)
    return out


def batch_edges():
    rng = np.random.default_rng(SEED + 6402)
    B, capq, capt = 9, W + 1, 2 * T + 1
    q, t = rand_desc(rng, B * capq).reshape(B, capq, 4), rand_desc(rng, B * capt).reshape(B, capt, 4)
    t[:, capt - 1], t[:, 5], q[:, 0], q[:, capq - 1] = t[:, 0], t[:, 1], t[:, 0], t[:, 3]
    return {"batch_edges": ("batch", q, np.array(BATCH_NQ), t, np.array(BATCH_NT))}


def ties():
    """Every group of TIE_ROWS holds one descriptor; queries 1 - 4 bits away from it stand in the first and the second query block of
    the first wavefront and in the second wavefront; everything else is random (distance ~128)."""
    rng = np.random.default_rng(SEED + 6403)
    nq, nt = 140, 100
    q, t = rand_desc(rng, nq), rand_desc(rng, nt)
    for k, rows in enumerate(TIE_ROWS.values()):
        d = rand_desc(rng, 1)[0]
        for r in rows:
            t[r] = d
        for i, row in enumerate((3 + k, 40 + k, 70 + k, 130 + k)):
            q[row] = flip(d, [7 * i + 11 * k + 1 + 60 * m for m in range(i + 1)])
    return {"ties": ("host", q, t)}


def d255(finite_row):
    nq, nt = 70, 70
    q, t = np.zeros((nq, 4), np.uint64), np.full((nt, 4), ONES)
    t[finite_row, 2] ^= np.uint64(1) << np.uint64(17)
    return ("host", q, t)


def last_index(nt, nq=Q + 1):
    """The nearest neighbour of every query (distance 1) at the last index nt - 1 and an equal duplicate at index 0."""
    rng = np.random.default_rng(SEED + 6404 + nt)
    t = rand_desc(rng, nt)
    base = rand_desc(rng, 1)[0]
    t[0] = t[nt - 1] = base
    q = np.stack([flip(base, [(3 * i + 1) % 256]) for i in range(nq)])
    return ("host", q, t)


def agree():
    rng = np.random.default_rng(SEED + 6405)
    B, cap = 5, 300
    q, t = rand_desc(rng, B * cap).reshape(B, cap, 4), rand_desc(rng, B * cap).reshape(B, cap, 4)
    t[:, 299], t[:, 150], q[:, 7], q[:, 290] = t[:, 0], t[:, 0], t[:, 0], t[:, 4]
    return {"agree": ("batch", q, np.array([300, 299, 257, 300, 64]), t, np.array([300, 300, 33, 1, 257]))}


def cases(names=None):
    """name -> ("host", q, t) or ("batch", q, nq, t, nt); the large train sets only when they are asked for."""
    makers = {"edges": lambda: {**host_edges(), **batch_edges()}, "ties": ties,
              "d255": lambda: {"d255_37": d255(37), "d255_69": d255(69)},
              "index_field": lambda: {"index_field": last_index(forms.NT_MAX)},
              "key_width": lambda: {"keys_8192": last_index(SHORT_NT), "keys_8193": last_index(SHORT_NT + 1)},
              "agree": agree}
    out = {}
    for n in names or list(makers):
        out.update(makers[n]())
    return out


def main(out, names):
    import torch

    from helpers import knn_to_array
    from snake_slam_amd.matcher import BruteForceMatcher

    dev = torch.device("cuda:0")
    bf = BruteForceMatcher(0)
    res = {}
    try:
        for name, c in cases(names).items():
            if c[0] == "host":
                bf.matchKnn2(c[1], c[2])
                res[name] = knn_to_array(bf.knn)
            else:
                _, q, nq, t, nt = c
                qd, td = torch.from_numpy(q.view(np.int64)).to(dev), torch.from_numpy(t.view(np.int64)).to(dev)
                nqd, ntd = torch.from_numpy(nq.astype(np.int32)).to(dev), torch.from_numpy(nt.astype(np.int32)).to(dev)
                o = torch.full((q.shape[0], q.shape[1], 4), -7, dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                bf.knn2_batch_dev(qd, nqd, td, ntd, o)
                bf.sync()
                res[name] = o.cpu().numpy()
    finally:
        bf.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
