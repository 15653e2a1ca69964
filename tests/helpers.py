"""Shared test helpers: seeded inputs and an independent numpy Hamming implementation."""
import numpy as np

SEED = 363456635  # the reference's randomSeed (reference configs/euroc.ini:3)


def rand_desc(rng, n):
    return rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)


def np_hamming_matrix(q, t):
    """Independent of the oracle: bit-unpack and count."""
    qb = np.unpackbits(np.ascontiguousarray(q).view(np.uint8).reshape(q.shape[0], 32), axis=1).astype(np.int16)
    tb = np.unpackbits(np.ascontiguousarray(t).view(np.uint8).reshape(t.shape[0], 32), axis=1).astype(np.int16)
    return (qb[:, None, :] != tb[None, :, :]).sum(axis=2).astype(np.int32)


def np_knn2(q, t):
    """Two lexicographically smallest (dist, idx) per query — the definition the scan implements."""
    nq, nt = q.shape[0], t.shape[0]
    out = np.zeros((nq, 4), np.int32)
    out[:, 0] = -1
    out[:, 1] = 256
    out[:, 2] = -1
    out[:, 3] = 256
    if nt == 0 or nq == 0:
        return out
    d = np_hamming_matrix(q, t)
    key = d.astype(np.int64) * (1 << 24) + np.arange(nt)[None, :]
    order = np.argsort(key, axis=1, kind="stable")
    out[:, 0] = order[:, 0]
    out[:, 1] = d[np.arange(nq), order[:, 0]]
    if nt > 1:
        out[:, 2] = order[:, 1]
        out[:, 3] = d[np.arange(nq), order[:, 1]]
    return out


def np_knn2_snake(q, t):
    """Snake's kNN-2, numpy only and independent of the oracle: per query the two lexicographically smallest (dist, idx) over the train
    rows with dist < 256 -- distance 256 is 'infinite' on the Snake side and never a neighbour (-1, 256).  One query at a time, so a
    train set of 2^20 rows costs nt x 4 words of scratch and no nq x nt table.  Rows are (idx1, dist1, idx2, dist2) like knn_to_array."""
    q = np.ascontiguousarray(q, np.uint64).reshape(-1, 4)
    t = np.ascontiguousarray(t, np.uint64).reshape(-1, 4)
    nt = t.shape[0]
    out = np.empty((q.shape[0], 4), np.int32)
    out[:, 0::2], out[:, 1::2] = -1, 256
    idx = np.arange(nt, dtype=np.int64)
    for i in range(q.shape[0] if nt else 0):
        d = np.bitwise_count(t ^ q[i]).sum(axis=1, dtype=np.int64)
        key = np.where(d < 256, (d << 32) | idx, np.int64(1) << 62)
        for k in (0, 1)[: min(2, nt)]:
            j = int(np.argmin(key))
            if key[j] < (np.int64(1) << 62):
                out[i, 2 * k], out[i, 2 * k + 1] = j, d[j]
            key[j] = np.int64(1) << 62
    return out


def knn_to_array(knn):
    return np.stack([knn["idx1"], knn["dist1"], knn["idx2"], knn["dist2"]], axis=1).astype(np.int32)


def make_stereo_case(rng, nl, nr, n_levels=4, height=480, width=752, bf=47.9, dup_frac=0.6):
    """Random rectified keypoints; a fraction of the right set are noisy copies of left ones at a
    plausible disparity so that matches, ties and rejections all occur."""
    from oracle.oracle import KP64

    left = np.zeros(nl, KP64)
    left["x"] = rng.uniform(20, width - 20, nl)
    left["y"] = rng.uniform(20, height - 20, nl)
    left["angle"] = rng.uniform(0, 360, nl).astype(np.float32)
    left["octave"] = rng.integers(0, n_levels, nl)
    dl = rand_desc(rng, nl)
    right = np.zeros(nr, KP64)
    right["x"] = rng.uniform(20, width - 20, nr)
    right["y"] = rng.uniform(20, height - 20, nr)
    right["angle"] = rng.uniform(0, 360, nr).astype(np.float32)
    right["octave"] = rng.integers(0, n_levels, nr)
    dr = rand_desc(rng, nr)
    ncopy = int(min(nl, nr) * dup_frac)
    src = rng.permutation(nl)[:ncopy]
    dst = rng.permutation(nr)[:ncopy]
    for s, d in zip(src, dst):
        right["x"][d] = left["x"][s] - rng.uniform(-2, bf * 0.55)
        right["y"][d] = left["y"][s] + rng.uniform(-3, 3)
        right["angle"][d] = np.float32((left["angle"][s] + rng.uniform(-30, 30)) % 360)
        right["octave"][d] = np.clip(left["octave"][s] + rng.integers(-2, 3), 0, n_levels - 1)
        flip = rng.integers(0, 90)
        bits = rng.permutation(256)[:flip]
        desc = dl[s].copy()
        for b in bits:
            desc[b >> 6] ^= np.uint64(1) << np.uint64(b & 63)
        dr[d] = desc
    # exact duplicates on the right to force distance ties
    for _ in range(max(1, nr // 20)):
        a, b = rng.integers(0, nr, 2)
        dr[b] = dr[a]
        right["y"][b] = right["y"][a] + rng.integers(-1, 2)
    level_scale = (np.float32(1.2) ** np.arange(n_levels)).astype(np.float32)
    return left, dl, right, dr, bf, level_scale


def stereo_prefill(B, capl):
    """Caller-owned right_points / depth with a value of its own in every entry: the public batched entry writes matched entries only."""
    i = np.arange(B * capl, dtype=np.float32).reshape(B, capl)
    return -2000.0 - (i % 251), -3000.0 - (i % 241)


def stereo_batch_dev(st, frames, capl, capr, bf, level_scale, relaxed=True):
    """frames: one (left, dl, right, dr) per batch entry, counts = lengths.  Runs snk_stereo_match_batch_dev on the padded batch with
    stereo_prefill's right_points / depth and returns (right_points [B, capl], depth [B, capl], n_matches [B]) as numpy arrays."""
    import torch

    from oracle.oracle import KP64

    B = len(frames)
    L, R = np.zeros((B, capl), KP64), np.zeros((B, capr), KP64)
    DL, DR = np.zeros((B, capl, 4), np.uint64), np.zeros((B, capr, 4), np.uint64)
    nl, nr = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b, (l, dl, r, dr) in enumerate(frames):
        nl[b], nr[b] = len(l), len(r)
        assert nl[b] <= capl and nr[b] <= capr
        L[b, : nl[b]], DL[b, : nl[b]], R[b, : nr[b]], DR[b, : nr[b]] = l, dl, r, dr
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rp0, dp0 = stereo_prefill(B, capl)
    rp, dp = t(rp0), t(dp0)
    nm = torch.full((B,), -1, dtype=torch.int32, device=dev)
    Ld, Rd = t(L.view(np.uint8).reshape(B, capl, 24)), t(R.view(np.uint8).reshape(B, capr, 24))
    DLd, DRd, nld, nrd = t(DL.view(np.int64)), t(DR.view(np.int64)), t(nl), t(nr)
    torch.cuda.synchronize()
    st.match_batch_dev(Ld, DLd, nld, Rd, DRd, nrd, bf, level_scale, relaxed, rp, dp, nm)
    st.sync()
    return rp.cpu().numpy(), dp.cpu().numpy(), nm.cpu().numpy()


def check_stereo_batch(orc, got, frames, capl, bf, level_scale, relaxed=True):
    """Every frame against orc.stereo_match started from the same caller-owned values, bit for bit; entries past nl[b] untouched.
    Returns the matches per frame."""
    rp, dp, nm = got
    rp0, dp0 = stereo_prefill(len(frames), capl)
    for b, (l, dl, r, dr) in enumerate(frames):
        n = len(l)
        wn, wrp, wdp = orc.stereo_match(l, dl, r, dr, bf, level_scale, relaxed, rp0[b, :n], dp0[b, :n])
        assert nm[b] == wn, f"frame {b}: {nm[b]} matches, the oracle has {wn}"
        assert np.array_equal(rp[b, :n], wrp) and np.array_equal(dp[b, :n], wdp), f"frame {b}"
        assert np.array_equal(rp[b, n:], rp0[b, n:]) and np.array_equal(dp[b, n:], dp0[b, n:]), f"frame {b}: entries past nl were written"
    return nm
