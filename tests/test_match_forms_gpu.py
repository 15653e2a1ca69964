"""GPU: every kernel form of the matchers at the launch shape where the dispatch changes (snake_slam_amd/csrc/dispatch.hpp), bit
for bit: kNN-2 against a numpy-only restatement (helpers.np_knn2_snake) AND the oracle, the ratio filter and the stereo matcher against
the oracle.  The shapes come from tests/forms.py, which the CPU test test_cpp_dispatch.py pins to their forms; the two forms that
only an environment switch selects run once each in a child process (form_children.py)."""
import numpy as np
import pytest

import form_children
import forms
from helpers import SEED, check_stereo_batch, knn_to_array, make_stereo_case, np_knn2_snake, rand_desc, stereo_batch_dev

pytestmark = pytest.mark.gpu
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def bf():
    from snake_slam_amd.matcher import BruteForceMatcher

    m = BruteForceMatcher(0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def st():
    from snake_slam_amd.matcher import StereoMatcher

    m = StereoMatcher(0)
    yield m
    m.close()


# ------------------------------------------------------------------------------------------------ kNN-2
def knn_batch(bf, q, nq, t, nt):
    """snk_bf_knn2_batch_dev on q [B, capq, 4] / t [B, capt, 4] uint64 with counts nq / nt; the output starts as -7 everywhere."""
    import torch

    dev = torch.device("cuda:0")
    B, capq = q.shape[:2]
    qd, td = torch.from_numpy(q.view(np.int64)).to(dev), torch.from_numpy(t.view(np.int64)).to(dev)
    nqd, ntd = torch.from_numpy(nq.astype(np.int32)).to(dev), torch.from_numpy(nt.astype(np.int32)).to(dev)
    out = torch.full((B, capq, 4), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    bf.knn2_batch_dev(qd, nqd, td, ntd, out)
    bf.sync()
    return out.cpu().numpy()


def check_knn_batch(orc, out, q, nq, t, nt):
    capq, capt = q.shape[1], t.shape[1]
    for b in range(q.shape[0]):
        n, m = min(int(nq[b]), capq), min(int(nt[b]), capt)  # a count above the capacity is clamped
        want = np_knn2_snake(q[b, :n], t[b, :m])
        assert np.array_equal(out[b, :n], want), f"batch entry {b} (nq {nq[b]}, nt {nt[b]}) differs from numpy"
        assert np.array_equal(want, knn_to_array(orc.bf_knn2(q[b, :n], t[b, :m]))), f"batch entry {b}: numpy and the oracle differ"
        assert (out[b, n:] == -7).all(), f"batch entry {b}: rows past nq were written"


def with_ties(rng, q, t):
    """Duplicate train rows and queries equal to a train row, so that ties are decided by the index."""
    nt = t.shape[1]
    for b in range(q.shape[0]):
        if nt > 8:
            t[b, nt // 2], t[b, nt - 1], t[b, 5] = t[b, 0], t[b, 3], t[b, 1]
        elif nt > 1:
            t[b, nt - 1] = t[b, 0]
        q[b, 0], q[b, q.shape[1] - 1] = t[b, 0], t[b, min(3, nt - 1)]
    return q, t


@pytest.mark.parametrize("form", ["vector4", "vector1"])
def test_knn2_four_queries_per_wave_at_its_threshold(bf, orc, form):
    """B x nq_cap = 64 x 256 = 16384 exactly with nt_cap = 23 < 24: bf_knn2_kernel<4>; 64 x 255 = 16320: bf_knn2_kernel<1>.  The
    counts leave the last group of four queries partly filled (the kernel re-reads query nq - 1 for the empty slots), the train sets
    hold 0, 1, 2 or all 23 rows with duplicates."""
    capq, capt, B, _ = forms.shape("knn2", (256 if form == "vector4" else 255, 23, 64, 0), form)
    rng = np.random.default_rng(SEED + capq)
    NQ, NT = [0, 1, 3, 4, 5, 255, 256], [0, 1, 2, 23]
    nq = np.array([NQ[b % 7] for b in range(B)])            # 256 with a capacity of 255: clamped
    nt = np.array([NT[(b // 7) % 4] for b in range(B)])     # every (nq, nt) combination within the first 28 entries
    q, t = with_ties(rng, rand_desc(rng, B * capq).reshape(B, capq, 4), rand_desc(rng, B * capt).reshape(B, capt, 4))
    # distance 255 against 256 in this kernel too: all-zero queries, all-one trains, the last train row with 255 bits set
    assert nq[27] >= capq and nt[27] == capt
    q[27], t[27] = 0, ONES
    t[27, capt - 1, 1] ^= np.uint64(1) << np.uint64(40)
    out = knn_batch(bf, q, nq, t, nt)
    assert out[27].tolist() == [[capt - 1, 255, -1, 256]] * capq
    check_knn_batch(orc, out, q, nq, t, nt)


def test_knn2_four_queries_per_wave_many_trains(bf, orc):
    """The other side of the ||: nq_cap = 15 < 24 with 1000 trains and 1100 x 15 = 16500 queries -- the 64-lane strided scan (j += 64)
    and the xor-shuffle merge of bf_knn2_kernel<4> do real work."""
    capq, capt, B, _ = forms.shape("knn2", (15, 1000, 1100, 0), "vector4")
    rng = np.random.default_rng(SEED + 15)
    nq = rng.integers(0, capq + 1, B)
    nt = rng.choice([0, 1, 2, 63, 64, 65, 127, 128, 129, 999, 1000], B)
    nq[:4], nt[:4] = [15, 13, 1, 15], [1000, 1000, 1000, 65]
    base = rand_desc(rng, 3)
    q, t = with_ties(rng, rand_desc(rng, B * capq).reshape(B, capq, 4), rand_desc(rng, B * capt).reshape(B, capt, 4))
    t[1], q[1] = base[rng.integers(0, 3, capt)], base[rng.integers(0, 3, capq)]  # three distinct descriptors: almost everything ties
    check_knn_batch(orc, knn_batch(bf, q, nq, t, nt), q, nq, t, nt)


@pytest.mark.parametrize("nq,nt", [(23, 24), (24, 23), (24, 24), (24, 25)])
def test_knn2_host_entry_at_the_matrix_core_boundary(bf, orc, nq, nt):
    forms.shape("knn2", (nq, nt, 1, 0), "mfma" if nq >= 24 and nt >= 24 else "vector1")
    rng = np.random.default_rng(SEED + 100 * nq + nt)
    q, t = with_ties(rng, rand_desc(rng, nq)[None], rand_desc(rng, nt)[None])
    bf.matchKnn2(q[0], t[0])
    got = knn_to_array(bf.knn)
    assert np.array_equal(got, np_knn2_snake(q[0], t[0])) and np.array_equal(got, knn_to_array(orc.bf_knn2(q[0], t[0])))


def test_knn2_matrix_core_batch_with_ragged_counts(bf, orc):
    """bf_knn2_mfma_kernel, nq_cap = 129 (the second workgroup in x has ONE live query), nt_cap = 65 (the third tile has one row):
    counts on both sides of a query block and a train tile, and one count above its capacity on either side (clamped)."""
    capq, capt, B, _ = forms.shape("knn2", (129, 65, 9, 0), "mfma")
    rng = np.random.default_rng(SEED + 129)
    nq = np.array([129, 0, 1, 31, 32, 33, 127, 128, 200])   # 200 -> 129
    nt = np.array([64, 63, 1000, 0, 1, 33, 23, 31, 32])     # 1000 -> 65
    assert sorted(np.minimum(nt, capt).tolist()) == [0, 1, 23, 31, 32, 33, 63, 64, 65]
    q, t = with_ties(rng, rand_desc(rng, B * capq).reshape(B, capq, 4), rand_desc(rng, B * capt).reshape(B, capt, 4))
    check_knn_batch(orc, knn_batch(bf, q, nq, t, nt), q, nq, t, nt)


@pytest.mark.parametrize("nq", [8, 40])
@pytest.mark.parametrize("finite_row", [37, 69])
def test_knn2_distance_255_against_256(bf, orc, nq, finite_row):
    """All-zero queries against a train set of all-one rows (distance 256: never a neighbour) and ONE row with 255 bits set, in the
    middle of the set and as its last row: that row is the only neighbour, the second stays (-1, 256).  nq = 8: vector kernel,
    nq = 40: matrix cores."""
    _, nt, _, _ = forms.shape("knn2", (nq, 70, 1, 0), "mfma" if nq == 40 else "vector1")
    q = np.zeros((nq, 4), np.uint64)
    t = np.full((nt, 4), ONES)
    t[finite_row, 2] ^= np.uint64(1) << np.uint64(17)
    bf.matchKnn2(q, t)
    got = knn_to_array(bf.knn)
    assert got.tolist() == [[finite_row, 255, -1, 256]] * nq
    assert np.array_equal(got, np_knn2_snake(q, t)) and np.array_equal(got, knn_to_array(orc.bf_knn2(q, t)))


@pytest.fixture(scope="module")
def largest_train_set(orc):
    """nt = 2^20 - 2, the documented maximum: the nearest neighbour of every query (distance 1) at the last index 2^20 - 3 and an equal
    duplicate at index 0.  The references are computed once, for the 32 queries; the vector case uses the first three."""
    rng = np.random.default_rng(SEED + 20)
    t = rand_desc(rng, forms.NT_MAX)
    base = rand_desc(rng, 1)[0]
    t[0] = t[forms.NT_MAX - 1] = base
    q = np.tile(base, (32, 1))
    for i in range(32):
        q[i, i & 3] ^= np.uint64(1) << np.uint64(2 * i + 1)
    want = np_knn2_snake(q, t)
    assert np.array_equal(want, knn_to_array(orc.bf_knn2(q, t)))
    assert (want[:, 0] == 0).all() and (want[:, 2] == forms.NT_MAX - 1).all() and (want[:, [1, 3]] == 1).all()  # index 0 wins, the last index second
    return q, t, want


@pytest.mark.parametrize("nq", [3, 32])
def test_knn2_index_field_at_the_largest_train_set(bf, largest_train_set, nq):
    forms.shape("knn2", (nq, forms.NT_MAX, 1, 0), "mfma" if nq == 32 else "vector1")
    q, t, want = largest_train_set
    bf.matchKnn2(q[:nq], t)
    assert np.array_equal(knn_to_array(bf.knn), want[:nq])


def test_knn2_train_set_past_the_index_field_is_refused(bf):
    import torch

    from snake_slam_amd import _lib

    lib = _lib.load()
    q, t, out = np.zeros((1, 4), np.uint64), np.zeros((1, 4), np.uint64), np.zeros((1, 4), np.int32)
    p = lambda a: a.ctypes.data
    assert lib.snk_bf_knn2(bf._h, p(q), 1, p(t), forms.NT_MAX + 1, p(out)) == 1  # SNK_ERR_INVALID_ARG, before anything is read
    d = torch.zeros(8, dtype=torch.int64, device="cuda:0")
    assert lib.snk_bf_knn2_batch_dev(bf._h, d.data_ptr(), d.data_ptr(), 1, d.data_ptr(), d.data_ptr(), forms.NT_MAX + 1, 1, d.data_ptr()) == 1
    assert lib.snk_bf_knn2_batch_dev(bf._h, d.data_ptr(), d.data_ptr(), 1, d.data_ptr(), d.data_ptr(), forms.NT_MAX, 0, d.data_ptr()) == 0


# ------------------------------------------------------------------------------------------------ ratio filter
FILTER_NQ = [255, 256, 257, 1025]  # bf_filter_kernel walks a frame in steps of 256
FILTER_KINDS = ["all", "none", "ends", "no_neighbour"]


def filter_table(orc, nq, kind):
    """kNN table for filterMatches(60, 0.8) and the pairs it must give: every row passes / none / only row 0 and the last row / every row
    would pass by its distances but two thirds have idx1 = -1 with dist1 = 0 ("no neighbour": dropped)."""
    k = np.zeros(nq, orc.KNN2)
    k["idx1"], k["idx2"] = (np.arange(nq) * 7 + 3) % nq, (np.arange(nq) * 5 + 1) % nq
    k["dist1"], k["dist2"] = 10, 100
    keep = np.ones(nq, bool)
    if kind == "none":
        keep[:] = False
    elif kind == "ends":
        keep[1:-1] = False
    k["dist1"][~keep] = 61
    if kind == "no_neighbour":
        keep = np.arange(nq) % 3 == 1
        k["idx1"][~keep], k["dist1"][~keep] = -1, 0
    rows = np.nonzero(keep)[0]
    return k, np.stack([rows, k["idx1"][rows]], 1).astype(np.int32)


@pytest.mark.parametrize("nq", FILTER_NQ)
def test_filter_host_entry_at_the_block_boundaries(bf, orc, nq):
    for kind in FILTER_KINDS:
        k, want = filter_table(orc, nq, kind)
        assert np.array_equal(orc.bf_filter(k, 60, 0.8), want), kind
        bf.knn = k
        assert bf.filterMatches(60, 0.8) == len(want), kind
        assert np.array_equal(bf.matches, want), kind


def test_filter_batched_entry_at_the_block_boundaries(bf, orc):
    import torch

    cap, B = max(FILTER_NQ), len(FILTER_NQ) * len(FILTER_KINDS)
    knn = np.full((B, cap, 4), 9, np.int32)  # rows past nq[b] would all pass
    knn[:, :, 1], knn[:, :, 3] = 10, 100
    nq, want = np.zeros(B, np.int32), []
    for b in range(B):
        nq[b] = FILTER_NQ[b % 4]
        k, w = filter_table(orc, int(nq[b]), FILTER_KINDS[b // 4])
        knn[b, : nq[b]] = knn_to_array(k)
        assert np.array_equal(orc.bf_filter(k, 60, 0.8), w)
        want.append(w)
    dev = torch.device("cuda:0")
    pairs = torch.full((B, cap, 2), -7, dtype=torch.int32, device=dev)
    npairs = torch.full((B,), -7, dtype=torch.int32, device=dev)
    kd, nd = torch.from_numpy(knn).to(dev), torch.from_numpy(nq).to(dev)
    torch.cuda.synchronize()
    bf.filter_batch_dev(kd, nd, 60, 0.8, pairs, npairs)
    bf.sync()
    pairs, npairs = pairs.cpu().numpy(), npairs.cpu().numpy()
    for b in range(B):
        assert npairs[b] == len(want[b]), b
        assert np.array_equal(pairs[b, : npairs[b]], want[b]), b
        assert (pairs[b, npairs[b]:] == -7).all(), b


# ------------------------------------------------------------------------------------------------ stereo
NL = 300  # left keypoints of a frame: enough for a few dozen matches, short on the oracle's side


def stereo_frames(rng, nrs, nl=NL, **kw):
    out = []
    for nr in nrs:
        left, dl, right, dr, bfv, ls = make_stereo_case(rng, nl if nr else 7, max(nr, 1), **kw)
        out.append((left, dl, right[:nr], dr[:nr]))
    return out, bfv, ls


@pytest.mark.parametrize("capr,B,form", [(2560, 8, "frame"), (2561, 8, "count16"), (2560, 7, "count16"), (8192, 2, "count16"),
                                         (8193, 2, "unindexed")])
def test_stereo_batched_entry_at_its_capacity_edges(st, orc, capr, B, form):
    """nr_cap on both sides of ST_FRAME_MAX = 2560 (frame form at a batch of 8, where 2049 right keypoints leave the third per-thread
    slot of its 1024 threads partly used) and of ST_SORT_MAX = 8192 (past it: the unindexed kernel, which no other test runs through
    the batched entry), and the batch threshold of 8.  One frame is full; right_points / depth are the caller's outside the matches."""
    forms.shape("stereo_batch", (capr, B, 0, 0), form)
    rng = np.random.default_rng(SEED + capr + B)
    nrs = ([capr, 2049, 0, 1, 650, 1025, 300, 2048] if B >= 7 else [capr, 333])[:B]
    frames, bfv, ls = stereo_frames(rng, nrs)
    nm = check_stereo_batch(orc, stereo_batch_dev(st, frames, NL + 5, capr, bfv, ls), frames, NL + 5, bfv, ls)
    assert nm[0] > 0 and nm.sum() > 20


def matched_pairs(left, dl, right, dr):
    """(left index, right index) of the noisy copies make_stereo_case planted: descriptors within 90 bits."""
    pairs = []
    for j in range(len(right)):
        d = np.bitwise_count(dl ^ dr[j]).sum(axis=1)
        i = int(np.argmin(d))
        if d[i] < 90:
            pairs.append((i, j))
    return pairs


def shift_pairs(rng, frame, amount):
    """Shift a third of the right keypoints by up to +-amount rows and the left keypoint each was copied from by the same."""
    left, dl, right, dr = frame
    sh = np.where(np.arange(len(right)) % 3 == 0, rng.integers(-amount, amount, len(right)) * 1.0, 0.0)
    moved = set()
    for i, j in matched_pairs(left, dl, right, dr):
        if sh[j] and i not in moved:
            left["y"][i] += sh[j]
            moved.add(i)
    right["y"] += sh


def test_stereo_frame_form_with_rows_beyond_its_buckets(st, orc):
    """stereo_frame_kernel buckets right keypoints by row - first row, clamped to ST_ROWS - 1 = 2047: frames whose right rows span
    ~6000, so that every row of the image proper lands in the clamped last bucket together with everything below it; a frame 5000
    rows above the image on both sides (every index row clamps to 0) and one with the right side only; every right keypoint on one row."""
    capr, B, _, _ = forms.shape("stereo_batch", (400, 8, 0, 0), "frame")
    capl = 420
    rng = np.random.default_rng(SEED + 2047)
    frames, bfv, ls = stereo_frames(rng, [400, 380, 380, 400, 333, 400, 64, 400], nl=400)
    for b in (0, 1, 5, 7):
        shift_pairs(rng, frames[b], 3000)
    for a in (frames[2][0], frames[2][2], frames[3][2]):
        a["y"] -= 5000.0
    frames[4][2]["y"][:] = 211.0
    rows0 = np.floor(frames[0][2]["y"] + 0.5)
    assert rows0.max() - rows0.min() > 2 * 2048
    got = stereo_batch_dev(st, frames, capl, capr, bfv, ls)
    nm = check_stereo_batch(orc, got, frames, capl, bfv, ls)
    # the case decides something: matches among the left keypoints whose band lies in the clamped bucket, and in the frame above the image
    hit = got[0][0, :400] > -1000.0
    assert (hit & (np.floor(frames[0][0]["y"] + 0.5) - rows0.min() > 2048)).sum() > 10
    assert nm[2] > 10 and nm[3] == 0 and nm[4] > 0


def count_index_cases(rng):
    """Right rows spanning exactly ST_COUNT_ROWS = 4096 (rows 0 .. 4095: the counting index with its table full), exactly 4097 (the
    network inside the same launch), and 2000 right keypoints on one row (the rank-within-row loop)."""
    frames, bfv, ls = stereo_frames(rng, [400, 400, 2000], height=4096)
    for b, last in ((0, 4095.0), (1, 4096.0)):
        right = frames[b][2]
        right["y"][:2] = [0.0, last]
        rows = np.floor(right["y"] + 0.5)
        assert rows.min() == 0 and rows.max() == last
    frames[2][2]["y"][:] = 2040.0
    frames[2][0]["y"][::2] = 2040.0 + rng.integers(-2, 3, len(frames[2][0]["y"][::2]))
    return frames, bfv, ls


def test_stereo_counting_index_at_the_end_of_its_table(st, orc):
    rng = np.random.default_rng(SEED + 4096)
    frames, bfv, ls = count_index_cases(rng)
    for b, (left, dl, right, dr) in enumerate(frames):  # host entry
        forms.shape("stereo_host", (len(right), 0), "count16")
        n, rp, dp = st.StereoMatching(left, dl, right, dr, bfv, ls, True)
        wn, wrp, wdp = orc.stereo_match(left, dl, right, dr, bfv, ls, True)
        assert n == wn and np.array_equal(rp, wrp) and np.array_equal(dp, wdp), b
        assert n > 0, b
    capr, B, _, _ = forms.shape("stereo_batch", (2000, 3, 0, 0), "count16")
    check_stereo_batch(orc, stereo_batch_dev(st, frames, NL + 1, capr, bfv, ls), frames, NL + 1, bfv, ls)


def test_stereo_sort_network_form_at_a_batch_of_eight(orc, tmp_path):
    """stereo_sort_kernel + stereo_kernel16 for B >= 8 is reached by no shape: the frame form takes every nr_cap <= 2560 and the counting
    index the rest.  One child process with SNK_STEREO_NO_FRAME_KERNEL and SNK_STEREO_SORT_NETWORK set (the second alone leaves the
    frame form in place, see tests/forms.py) runs B = 8, nr_cap = 400 and writes its results; compared here with the oracle."""
    capr, B, _, _ = forms.shape("stereo_batch", (400, 8, 1, 1), "sort16")
    out = tmp_path / "stereo.npz"
    form_children.run_child("stereo", out, SNK_STEREO_NO_FRAME_KERNEL="1", SNK_STEREO_SORT_NETWORK="1")
    frames, capl, bfv, ls = form_children.stereo_case(B)
    z = np.load(out)
    nm = check_stereo_batch(orc, (z["rp"], z["dp"], z["nm"]), frames, capl, bfv, ls)
    assert nm.sum() > 50
