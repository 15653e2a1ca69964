"""GPU: rectify / undistort kernel vs the oracle — bit-exact fp64 (fixed operation order)."""
import numpy as np
import pytest

from test_oracle_preprocess import EUROC_D, EUROC_K, make_kps

pytestmark = pytest.mark.gpu


def test_rectify_parity(orc):
    from snake_slam_amd.matcher import Preprocess, Rectification

    pp = Preprocess(0)
    a = 0.013
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    for n, D, Rm, Kd in [(1000, EUROC_D, R, (435.2, 435.2, 367.4, 252.2)), (257, None, None, None), (0, EUROC_D, None, None),
                         (64, (0.1, -0.05, 0.01, 0.02, 0.003, 0.0001, 0.001, -0.002), R, None)]:
        k = make_kps(orc, n, n)
        ro = orc.rectification(EUROC_K, D, Rm, Kd)
        rg = Rectification.make(EUROC_K, D, Rm, Kd)
        want, wn = orc.rectify(ro, k)
        got, gn = pp.rectify(rg, k)
        for f in ("x", "y", "angle", "octave"):
            assert np.array_equal(got[f], want[f]), f
        assert np.array_equal(gn, wn)
    pp.close()


def test_rgbd_stereo_parity(orc):
    """Preprocess::ComputeStereoFromRGBD (Preprocess.cpp:79-120) on the device against the oracle, bit for bit (fp64 geometry, float
    stores): host call and batched device form, with a distorted depth camera; and the reference's aborts reported, not executed."""
    import torch

    from oracle.oracle import KP64
    from snake_slam_amd._lib import SnakeHipError
    from snake_slam_amd.matcher import Preprocess, RgbdModel

    rng = np.random.default_rng(2026)
    w, h = 640, 480
    K, Kd = (525.0, 525.0, 319.5, 239.5), (570.3, 570.3, 320.0, 240.0)
    Dd = (0.05, -0.1, 0.0, 0.0, 0.0, 0.0, 1e-3, -5e-4)
    model = RgbdModel.make(K, Dd, Kd, 40.0)
    pre = Preprocess(0)
    try:
        for n in (0, 1, 777, 2000):
            und = np.zeros(n, KP64)
            und["x"], und["y"] = rng.uniform(40, w - 40, n), rng.uniform(40, h - 40, n)
            img = np.where(rng.random((h, w)) < 0.3, 0.0, rng.uniform(0.3, 19.9, (h, w))).astype(np.float32)
            got = pre.ComputeStereoFromRGBD(model, und, img)
            want = orc.rgbd_stereo(und, K, Dd, Kd, 40.0, img)
            assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
            if n > 100:
                assert 0 < got[0] < n and (got[2] == -1).any()
        # the reference aborts: outside the depth image / depth >= 20
        und = np.zeros(5, KP64)
        und["x"], und["y"] = [100, 200, 5000, 300, 9000], [100, 100, 100, 100, 100]
        img = np.full((h, w), 1.0, np.float32)
        assert orc.rgbd_stereo(und, K, Dd, Kd, 40.0, img)[0] == -3
        with pytest.raises(SnakeHipError):
            pre.ComputeStereoFromRGBD(model, und, img)
        und["x"][2], und["x"][4] = 150, 160
        img[:, :] = 20.0
        assert orc.rgbd_stereo(und, K, Dd, Kd, 40.0, img)[0] == -1
        with pytest.raises(SnakeHipError):
            pre.ComputeStereoFromRGBD(model, und, img)
        # batched, device resident: ragged counts, one frame with an offending keypoint
        B, cap = 4, 900
        dev = torch.device("cuda:0")
        U = np.zeros((B, cap), KP64)
        nn = np.array([900, 0, 333, 512], np.int32)
        imgs = np.where(rng.random((B, h, w)) < 0.3, 0.0, rng.uniform(0.3, 19.9, (B, h, w))).astype(np.float32)
        for b in range(B):
            U["x"][b, : nn[b]], U["y"][b, : nn[b]] = rng.uniform(40, w - 40, nn[b]), rng.uniform(40, h - 40, nn[b])
        U["x"][3, 17] = -500.0
        t = lambda a: torch.from_numpy(a).to(dev)
        rp = torch.full((B, cap), -1000.0, dtype=torch.float32, device=dev)
        dp = torch.full((B, cap), -1000.0, dtype=torch.float32, device=dev)
        nm, stt = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        pre.rgbd_batch_dev(model, t(U.view(np.uint8).reshape(B, cap, 24)), t(nn), t(imgs), rp, dp, nm, stt)
        pre.sync()
        for b in range(B):
            want = orc.rgbd_stereo(U[b, : nn[b]], K, Dd, Kd, 40.0, imgs[b])
            if b == 3:
                assert want[0] == -18 and int(stt[b]) == 18
                continue
            assert int(stt[b]) == 0x7FFFFFFF and int(nm[b]) == want[0]
            assert np.array_equal(rp[b, : nn[b]].cpu().numpy(), want[1]) and np.array_equal(dp[b, : nn[b]].cpu().numpy(), want[2])
            assert (rp[b, nn[b]:] == -1000).all()
    finally:
        pre.close()


@pytest.mark.parametrize("with_normalized", [True, False])
def test_rectify_batch_dev_parity(orc, with_normalized):
    """snk_rectify_batch_dev -- the first call of the batched matching step -- per frame against orc.rectify, bit for bit, under the
    four rectifications of test_rectify_parity: counts 257 (= cap: the second block has one live thread), 0, 1, 256 and 300 (clamped
    to cap); `out` and the optional `normalized` start as a pattern that must survive past n[b]."""
    import torch

    from oracle.oracle import KP64
    from snake_slam_amd.matcher import Preprocess, Rectification

    B, cap = 5, 257
    n = np.array([257, 0, 1, 256, 300], np.int32)
    a = 0.013
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    dev = torch.device("cuda:0")
    k = make_kps(orc, B * cap, 31).reshape(B, cap)
    d_k, d_n = torch.from_numpy(k.view(np.uint8).reshape(B, cap, 24)).to(dev), torch.from_numpy(n).to(dev)
    pat_out = (np.arange(B * cap * 24) % 251).astype(np.uint8).reshape(B, cap, 24)
    pat_norm = -7.0 - np.arange(B * cap * 2, dtype=np.float64).reshape(B, cap, 2)
    pp = Preprocess(0)
    try:
        for D, Rm, Kd in [(EUROC_D, R, (435.2, 435.2, 367.4, 252.2)), (None, None, None), (EUROC_D, None, None),
                          ((0.1, -0.05, 0.01, 0.02, 0.003, 0.0001, 0.001, -0.002), R, None)]:
            ro, rg = orc.rectification(EUROC_K, D, Rm, Kd), Rectification.make(EUROC_K, D, Rm, Kd)
            d_out = torch.from_numpy(pat_out).to(dev)
            d_norm = torch.from_numpy(pat_norm).to(dev) if with_normalized else None
            torch.cuda.synchronize()
            pp.rectify_batch_dev(rg, d_k, d_n, d_out, d_norm)
            pp.sync()
            out = d_out.cpu().numpy()
            for b in range(B):
                m = min(int(n[b]), cap)
                want, wn = orc.rectify(ro, k[b, :m])
                got = out[b, :m].copy().view(KP64).reshape(m)
                for f in ("x", "y", "angle", "octave"):
                    assert np.array_equal(got[f], want[f]), (b, f)
                assert np.array_equal(out[b, m:], pat_out[b, m:]), f"frame {b}: out was written past n"
                if with_normalized:
                    norm = d_norm[b].cpu().numpy()
                    assert np.array_equal(norm[:m], wn) and np.array_equal(norm[m:], pat_norm[b, m:]), b
    finally:
        pp.close()


def rgbd_pitch_case():
    """K_depth = K = (512, 512, 320, 240) and no distortion: every operation from an undistorted keypoint to its depth pixel is exact
    for the coordinates below, so the pixel is known by hand -- (int)(x + 0.5).  x = -0.5 -> column 0, x = w - 1.5 + 2^-20 -> column
    w - 1, x = w - 0.5 -> column w: outside; the same for y.  The depth image holds a value of its own in every pixel."""
    from oracle.oracle import KP64

    w, h = 640, 480
    K = (512.0, 512.0, 320.0, 240.0)
    rng = np.random.default_rng(2027)
    img = (0.5 + (np.arange(h * w) % 9973) / 1000.0).astype(np.float32).reshape(h, w)  # 0.5 .. 10.5, neighbours differ
    img[rng.random((h, w)) < 0.1] = 0.0
    img[0, 0] = img[0, w - 1] = img[h - 1, 0] = img[h - 1, w - 1] = 1.25
    und = np.zeros(40, KP64)
    und["x"], und["y"] = rng.uniform(5, w - 5, 40), rng.uniform(5, h - 5, 40)
    edge = 2.0 ** -20
    und["x"][:4], und["y"][:4] = [-0.5, w - 1.5 + edge, -0.5, w - 1.5 + edge], [-0.5, -0.5, h - 1.5 + edge, h - 1.5 + edge]
    pixel = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)]  # (column, row) of the first four keypoints
    return w, h, K, img, und, pixel


def rgbd_host_pitched(pre, model, und, padded, w, h):
    """snk_rgbd_stereo on the [:, :w] part of `padded`, pitch = its row length; returns (status code, n_matches, right_points, depth)."""
    import ctypes as C

    from snake_slam_amd import _lib

    rp, dp = np.full(len(und), -5.0, np.float32), np.full(len(und), -5.0, np.float32)
    nm = C.c_int(0)
    rc = _lib.load().snk_rgbd_stereo(pre._h, C.byref(model), und.ctypes.data, len(und), padded.ctypes.data, w, h, padded.shape[1],
                                     rp.ctypes.data, dp.ctypes.data, C.byref(nm))
    return rc, nm.value, rp, dp


def test_rgbd_stereo_with_a_row_pitch(orc):
    """The depth image inside a larger allocation: the host entry with pitch_floats = width + 13 (the Python wrapper only ever passes
    pitch == width), the batched entry with a [:, :h, :w] view whose row pitch and image stride both exceed the image.  The padding
    holds 25.0, a depth on which the reference aborts: reading it instead of the image shows as a status."""
    import torch

    from snake_slam_amd.matcher import Preprocess, RgbdModel

    w, h, K, img, und, pixel = rgbd_pitch_case()
    bf_ = 40.0
    model = RgbdModel.make(K, None, K, bf_)
    pre = Preprocess(0)
    try:
        padded = np.full((h, w + 13), 25.0, np.float32)
        padded[:, :w] = img
        rc, nm, rp, dp = rgbd_host_pitched(pre, model, und, padded, w, h)
        wn, wrp, wdp = orc.rgbd_stereo(und, K, np.zeros(8), K, bf_, img)
        assert rc == 0 and nm == wn > 20 and np.array_equal(rp, wrp) and np.array_equal(dp, wdp)
        for i, (x, y) in enumerate(pixel):   # the pixels known by hand
            assert dp[i] == img[y, x] == np.float32(1.25) and rp[i] == np.float32(und["x"][i] - bf_ / 1.25)
        # one step further is outside the image: status = index + 1 of the LOWEST offending keypoint, outputs untouched
        for field, value, first, second in (("x", w - 0.5, 7, 3), ("y", h - 0.5, 9, 2), ("x", w - 0.5, 0, 39)):
            bad = und.copy()
            bad[field][[first, second]] = value
            rc, nm, rp, dp = rgbd_host_pitched(pre, model, bad, padded, w, h)
            assert rc == 1 and nm == -(min(first, second) + 1) and (rp == -5.0).all() and (dp == -5.0).all(), (field, first, second)
            assert orc.rgbd_stereo(bad, K, np.zeros(8), K, bf_, img)[0] == -(min(first, second) + 1)
        # batched: three images inside one allocation [3, h + 5, w + 13]
        B, cap = 3, 48
        dev = torch.device("cuda:0")
        big = np.full((B, h + 5, w + 13), 25.0, np.float32)
        imgs = np.stack([img, np.roll(img, 7, axis=1), img[::-1].copy()])
        big[:, :h, :w] = imgs
        U = np.zeros((B, cap), und.dtype)
        nn = np.array([40, 40, 33], np.int32)
        U[0, :40], U[1, :40], U[2, :33] = und, und, und[:33]
        U["x"][1, 11], U["y"][1, 30], U["x"][1, 5] = w - 0.5, h - 0.5, w - 0.5   # frame 1 offends at 5, 11 and 30: 5 wins
        view = torch.from_numpy(big).to(dev)[:, :h, :w]
        assert view.stride(1) == w + 13 and view.stride(0) == (h + 5) * (w + 13)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        rpd = torch.full((B, cap), -1000.0, dtype=torch.float32, device=dev)
        dpd = torch.full((B, cap), -1000.0, dtype=torch.float32, device=dev)
        nmd, stt = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        pre.rgbd_batch_dev(model, t(U.view(np.uint8).reshape(B, cap, 24)), t(nn), view, rpd, dpd, nmd, stt)
        pre.sync()
        rpd, dpd, nmd, stt = rpd.cpu().numpy(), dpd.cpu().numpy(), nmd.cpu().numpy(), stt.cpu().numpy()
        for b in range(B):
            want = orc.rgbd_stereo(U[b, : nn[b]], K, np.zeros(8), K, bf_, imgs[b])
            if b == 1:
                assert want[0] == -6 and stt[b] == 6
                continue
            assert stt[b] == 0x7FFFFFFF and nmd[b] == want[0] > 15
            assert np.array_equal(rpd[b, : nn[b]], want[1]) and np.array_equal(dpd[b, : nn[b]], want[2])
            assert (rpd[b, nn[b]:] == -1000).all() and (dpd[b, nn[b]:] == -1000).all()
    finally:
        pre.close()
