"""Kernel time of snk_bf_knn2_batch_dev at 1000 x 1000 descriptors per frame for a list of batch sizes (GPU box).  The form is chosen
by the environment, read once per process: SNK_HIP_LIB (another build of the library), SNK_BF_MFMA_WIDE=0 / 1, SNK_BF_MFMA_NO_SHORT=1,
SNK_BF_NO_MFMA=1 -- so one process per row of a table:
    SNK_BF_MFMA_WIDE=1 python tools/probes/knn2_batch_timing.py wide_13bit 1,8,64,128,256,1024
prints one JSON line: per batch size the five per-launch times in microseconds (sorted; each from stream events around 20 - 100 launches),
a hash of the output -- equal hashes across rows = identical outputs -- and, up to 8 frames, whether every row equals the oracle."""
import hashlib
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import oracle  # noqa: E402
from snake_slam_amd.matcher import BruteForceMatcher  # noqa: E402


def main(tag, batches):
    oracle.build()
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream()  # the handle's stream: the events below are recorded on it
    torch.cuda.set_stream(st)
    bf = BruteForceMatcher(0, st.cuda_stream)
    rng = np.random.default_rng(5)
    res = {"tag": tag, "lib": "variant" if os.environ.get("SNK_HIP_LIB") else "tree", "wide": os.environ.get("SNK_BF_MFMA_WIDE", ""),
           "no_short": os.environ.get("SNK_BF_MFMA_NO_SHORT", "")}
    for B in batches:
        q = rng.integers(0, 2**63, size=(B, 1000, 4), dtype=np.int64)
        t = rng.integers(0, 2**63, size=(B, 1000, 4), dtype=np.int64)
        t[:, 500] = t[:, 3]
        t[:, 999] = t[:, 3]
        q[:, 7] = t[:, 3]
        qd, td = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev)
        nqh, nth = rng.integers(900, 1001, B).astype(np.int32), rng.integers(900, 1001, B).astype(np.int32)
        nq, nt = torch.from_numpy(nqh).to(dev), torch.from_numpy(nth).to(dev)
        out = torch.full((B, 1000, 4), -7, dtype=torch.int32, device=dev)
        for _ in range(3):
            bf.knn2_batch_dev(qd, nq, td, nt, out)
        torch.cuda.synchronize()
        n = 20 if B >= 256 else 100
        ts = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                bf.knn2_batch_dev(qd, nq, td, nt, out)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / n * 1000)
        o = out.cpu().numpy()
        ok = None
        if B <= 8:
            ok = True
            for b in range(B):
                w = oracle.bf_knn2(q[b, :nqh[b]].view(np.uint64), t[b, :nth[b]].view(np.uint64))
                w = np.stack([w["idx1"], w["dist1"], w["idx2"], w["dist2"]], axis=1)
                ok = ok and bool(np.array_equal(o[b, :nqh[b]], w)) and bool((o[b, nqh[b]:] == -7).all())
        res[str(B)] = {"us": [round(x, 2) for x in sorted(ts)], "sha": hashlib.sha1(o.tobytes()).hexdigest()[:12], "oracle_equal": ok}
    bf.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main(sys.argv[1], [int(x) for x in sys.argv[2].split(",")])
