"""GPU: distribute_kernel / distribute_large_kernel at the candidate counts where their code changes path, bit for bit against the
oracle: the selection per (image, level) with orc.distribute, keypoints and descriptors with orc.orb_detect, per-frame call
(snk_orb_detect: one launch with the full LDS carve) against the batched call (2048-candidate carve + overflow queue).

The images are isolated bright pixels on a dark ground, one FAST corner each with a score of its own, so level 0 of a 320 x 240 image
holds EXACTLY the wanted number of candidates (asserted with the oracle on the CPU before anything runs on the device):
  0, 1, 2               nothing to sort, a single node
  511, 512, 513         one candidate per thread of the 512-thread workgroup: the strided loops' second trip
  2047, 2048, 2049      four per thread, the register-array forms and the 2048-candidate carve; 2049 overflows it: the batched call
                        queues the level for distribute_large_kernel (bitonic sort, sorted node list)
Level 1 (scale 1.2) holds whatever the down-scaled dots give, a different count per image."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 320, 240
PARAMS = (500, 1.2, 2, 20, 7)  # nfeatures, scale, levels, ini / min FAST threshold: 273 features on level 0, 227 on level 1
COUNTS = [0, 1, 2, 511, 512, 513, 2047, 2048, 2049]
MORE_COUNTS = [3, 64, 300, 777, 1024, 1500, 1900, 2500]  # fills the batch of 17 (the XCD-mapped grids start at 16 images)


def dot_image(n, seed=0, pairs=False):
    """n isolated bright pixels on a 4-pixel lattice inside the FAST cells (a pixel 4 away is on nobody's radius-3 circle): n
    candidates on level 0.  pairs: the dots come as horizontal neighbours on the lattice, far from the other pairs, so a quadtree node
    with two points splits into two children and not four."""
    rng = np.random.default_rng(1000 * n + seed)
    img = np.full((H, W), 10, np.uint8)
    xs, ys = np.arange(24, W - 24, 4), np.arange(24, H - 24, 4)
    if pairs:
        cx, cy = np.meshgrid(xs[1:-2:5], ys[1:-1:4])
        sites = np.stack([cx.ravel(), cy.ravel()], 1)
        pick = sites[rng.permutation(len(sites))[: n // 2]]
        pts = np.concatenate([pick, pick + np.array([4, 0])])
    else:
        cx, cy = np.meshgrid(xs, ys)
        sites = np.stack([cx.ravel(), cy.ravel()], 1)
        pts = sites[rng.permutation(len(sites))[:n]]
    assert len(pts) == n
    img[pts[:, 1], pts[:, 0]] = rng.integers(60, 256, n).astype(np.uint8)
    return img


def careful_rounds(orc, cand, w, h, N):
    """Rounds of the careful phase (split the fullest nodes first until N nodes exist) that the sorted-key formulation of the
    distribution takes on these candidates: a restatement on the oracle's keys of steps 4 to 6 of distribute_body."""
    Wb, Hb = w - 32, h - 32
    keys = sorted(orc.point_key(int(c["x"]) - 16, int(c["y"]) - 16, Wb, Hb) for c in cand)
    n = len(keys)
    if n < 2:
        return 0

    def lcp_of(a, b):  # equal leading digits, -1: another root
        d = a ^ b
        return -1 if d >> 32 else 15 - ((d.bit_length() - 1) >> 1)

    lcp = [-1] + [lcp_of(keys[i - 1], keys[i]) for i in range(1, n)] + [-1]
    D, careful, size, prev = 16, False, 0, None
    for d in range(1, 17):
        heads = 1 + sum(1 for i in range(1, n) if lcp[i] < d)
        singles = sum(1 for i in range(n) if max(lcp[i], lcp[i + 1]) < d)
        multi = heads - singles
        if prev is None:
            prev = 1 + sum(1 for i in range(1, n) if lcp[i] < 0)
        if heads >= N or heads == prev:
            D, size = d, heads
            break
        if heads + 3 * multi > N:
            D, careful, size = d, True, heads
            break
        prev, size = heads, heads
    if not careful:
        return 0
    fd, rounds = [D] * n, 0
    for dd in range(D, 16):
        rounds += 1
        nodes = []  # (count, position, new nodes)
        for i in range(n):
            if fd[i] == dd and lcp[i] < dd:
                e = i + 1
                while e < n and lcp[e] >= dd:
                    e += 1
                if e - i > 1:
                    nodes.append((e - i, i, sum(1 for j in range(i + 1, e) if lcp[j] == dd)))
        if not nodes:
            break
        add = 0
        for cnt, i, delta in sorted(nodes, key=lambda t: (-t[0], t[1])):
            if size + add >= N:
                break
            add += delta
            for e in range(i, i + cnt):
                fd[e] = dd + 1
        size += add
        if size >= N or add == 0:
            break
    return rounds


def level0_candidates(orc, img):
    p = orc.orb_params(*PARAMS)
    levels, L = orc.pyramid(p, img)
    return orc.candidates(levels[0], p.ini_th, p.min_th, 8192), L


@pytest.fixture(scope="module")
def cases(orc):
    """Images by level-0 candidate count, with the oracle's keypoints and descriptors (computed once, read by every test)."""
    out = {}
    for n in COUNTS + MORE_COUNTS:
        img = dot_image(n)
        cand, _ = level0_candidates(orc, img)
        assert len(cand) == n, f"the image for {n} candidates holds {len(cand)}"
        out[n] = (img, *orc.orb_detect(orc.orb_params(*PARAMS), img))
    return out


def run_batch(imgs, queued=None):
    """The batched call on imgs; queued (a list): receives the (image, level) pairs the call handed to distribute_large_kernel."""
    import torch
    from snake_slam_amd.orb import DEBUG_DIST_QUEUE, ORBExtractor, KEYPOINT_DTYPE

    B = len(imgs)
    ext = ORBExtractor(*PARAMS)
    try:
        cap = ext.configure(W, H, B)
        dev = torch.device("cuda:0")
        d_img = torch.from_numpy(np.stack(imgs)).to(dev)
        d_kps = torch.zeros((B, cap, 24), dtype=torch.uint8, device=dev)
        d_desc = torch.zeros((B, cap, 4), dtype=torch.int64, device=dev)
        d_n = torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ext.detect_batch_dev(d_img, d_kps, d_desc, d_n)
        ext.sync()
        n = d_n.cpu().numpy()
        kps = d_kps.cpu().numpy().view(KEYPOINT_DTYPE).reshape(B, cap)
        desc = d_desc.cpu().numpy().view(np.uint64).reshape(B, cap, 4)
        if queued is not None:
            q = ext.debug_fetch(DEBUG_DIST_QUEUE, 0, 0, np.int32)
            queued.extend(sorted(divmod(int(v), 16) for v in q[1 : 1 + int(q[0])]))
        return [(kps[i, : n[i]], desc[i, : n[i]]) for i in range(B)]
    finally:
        ext.close()


def assert_same(got, want, what):
    from snake_slam_amd.orb import KEYPOINT_DTYPE

    (gk, gd), (wk, wd) = got, want
    assert len(gk) == len(wk), f"{what}: {len(gk)} keypoints, the oracle has {len(wk)}"
    assert np.array_equal(gk, wk.astype(KEYPOINT_DTYPE)), f"{what}: keypoints differ"
    assert np.array_equal(gd, wd), f"{what}: descriptors differ"


@pytest.mark.parametrize("n", COUNTS)
def test_per_frame_call_at_the_boundary_counts(orc, cases, n):
    """snk_orb_detect: pyramid, candidates and the selection of every level against the oracle's stages, then the keypoints."""
    from snake_slam_amd.orb import ORBExtractor
    from test_orb_gpu import stage_check

    img, wk, wd = cases[n]
    ext = ORBExtractor(*PARAMS)
    try:
        kps, desc = ext.Detect(img)
        stage_check(ext, orc, img, orc.orb_params(*PARAMS))
        assert len(kps) == len(wk)
        for f in ("octave", "x", "y", "size", "response", "angle"):
            assert np.array_equal(kps[f], wk[f]), f"keypoint field {f} differs"
        assert np.array_equal(desc, wd), "descriptors differ"
    finally:
        ext.close()


def test_batched_call_with_the_overflow_queue(orc, cases):
    """More than 128 (image, level) problems: the 2048-candidate carve, the level with 2049 goes through the queue to
    distribute_large_kernel.  Every image comes out as the per-frame call and the oracle have it."""
    imgs = [cases[n][0] for n in COUNTS]
    B = 72  # 144 problems
    queued = []
    got = run_batch([imgs[i % len(imgs)] for i in range(B)], queued)
    assert queued == [(i, 0) for i in range(B) if COUNTS[i % len(COUNTS)] == 2049], "level 0 of the 2049-candidate images, nothing else, is queued"
    for i in range(B):
        n = COUNTS[i % len(COUNTS)]
        assert_same(got[i], cases[n][1:], f"image {i} ({n} candidates)")


def test_batch_of_17_with_a_count_of_its_own_per_image(orc, cases):
    """17 images cross the threshold of the XCD-mapped grids (16); full-carve launch (34 problems), a different count in every image."""
    counts = COUNTS + MORE_COUNTS
    assert len(counts) == 17 and len(set(counts)) == 17
    queued = []
    got = run_batch([cases[n][0] for n in counts], queued)
    assert queued == [], "the full-carve launch queues nothing"
    for i, n in enumerate(counts):
        assert_same(got[i], cases[n][1:], f"image {i} ({n} candidates)")


def test_harris_ranks_with_the_overflow_queue(orc, cases):
    """"orb.response" = 1: the Harris ranks ride behind the 2048-candidate carve (two-tier launch at every batch size) and in global
    scratch for the queued level."""
    from snake_slam_amd import _lib

    counts = [2, 513, 2047, 2048, 2049]
    _lib.set_definition("orb.response", 1)
    orc.set_definition("orb.response", 1)
    try:
        want = [orc.orb_detect(orc.orb_params(*PARAMS), cases[n][0]) for n in counts]
        queued = []
        got = run_batch([cases[n][0] for n in counts], queued)
    finally:
        _lib.set_definition("orb.response", 0)
        orc.set_definition("orb.response", 0)
    assert queued == [(counts.index(2049), 0)]
    for i, n in enumerate(counts):
        assert_same(got[i], want[i], f"image {i} ({n} candidates, Harris)")


def test_careful_phase_past_its_first_round(orc):
    """Dots in pairs: a node with two points gives two children where the replay's bound counts four, so the first careful round
    splits every node and still has fewer than N (the restatement above counts the rounds; asserted before the device runs)."""
    from test_orb_gpu import check_image

    img = dot_image(280, pairs=True)
    cand, L = level0_candidates(orc, img)
    assert len(cand) == 280
    assert careful_rounds(orc, cand, W, H, L.nfeat[0]) >= 2
    check_image(orc, img, PARAMS[0], PARAMS[2], PARAMS[1], PARAMS[3], PARAMS[4])
    got = run_batch([img] * 3)
    want = orc.orb_detect(orc.orb_params(*PARAMS), img)
    for i in range(3):
        assert_same(got[i], want, f"image {i}")


def test_loop_form_of_the_keys_gives_the_same():
    """SNK_ORB_DIST_KEY_LOOP=1 (read once per process): the tests above again in a child process whose distribute kernels compute the
    subdivision keys by the loop form of orb_keys.hpp instead of reading the tables."""
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    r = subprocess.run([sys.executable, "-m", "pytest", str(Path(__file__).resolve()), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider",
                        "-k", "not loop_form_of_the_keys"],
                       env=dict(os.environ, SNK_ORB_DIST_KEY_LOOP="1"), capture_output=True, text=True, cwd=str(root), timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-1000:])
    assert "13 passed" in r.stdout
