"""Tiny BA batches laid out as the device rows snk_ba_set_problems_dev takes, and the comparison every case of
tests/test_ba_handover_dev_gpu.py makes: the same problems loaded through snk_ba_set_problems from host copies of the rows and through
snk_ba_set_problems_dev from device tensors, on fresh handles of the same options.  Both loads feed the same lists to the same kernels, so
every output must be the same bytes.  Shared with the child process of tests/handover_children.py."""
import numpy as np

import handover_numpy as M

CHI2_MONO, CHI2_STEREO = 5.991, 7.815  # the reference's thresholds
K = (458.654, 457.296, 367.215, 248.375)
BF = 47.9


def scene(n_kf=4, n_pt=30, obs_per_pt=3, seed=1, **kw):
    from snake_slam_amd import synth

    s, gt = synth.ba_scene(n_kf=n_kf, n_pt=n_pt, obs_per_pt=obs_per_pt, seed=seed, **kw)
    assert tuple(s["K"]) == K and s["bf"] == BF
    return s, gt


def take_obs(s, idx):
    """The scene with the observations ``idx`` (in that order) only."""
    idx = np.asarray(idx, np.int64)
    return dict(s, **{k: np.asarray(s[k])[idx] for k in ("obs_img", "obs_pt", "obs_uv", "obs_depth", "obs_weight")})


def add_obs(s, like, img):
    """The scene with a copy of observation ``like`` appended, seen by image ``img``."""
    out = dict(s)
    for k in ("obs_img", "obs_pt", "obs_uv", "obs_depth", "obs_weight"):
        a = np.asarray(s[k])
        out[k] = np.concatenate([a, a[like:like + 1]])
    out["obs_img"] = out["obs_img"].copy()
    out["obs_img"][-1] = img
    return out


def unequal_batch(n, seed=0):
    """n unequal tiny windows; row 1 is an empty row (its query was skipped), row 2 has every camera constant, row 0 a single point."""
    rng = np.random.RandomState(seed)
    rows = []
    for b in range(n):
        s, _ = scene(n_kf=int(rng.randint(3, 7)), n_pt=int(rng.randint(8, 41)), obs_per_pt=int(rng.randint(2, 4)), seed=100 + seed * 1000 + b)
        rows.append(s)
    rows[0] = scene(n_kf=3, n_pt=1, obs_per_pt=3, seed=7)[0]
    rows[1] = None
    rows[2] = dict(rows[2], img_const=np.ones(len(rows[2]["pose"]), np.uint8))
    return rows


def constraint_batch():
    """Three windows with relative pose constraints: one between two constant images (the first two cameras are fixed), one that names an
    image out of range; a row without constraints between them."""
    from snake_slam_amd import synth

    rows = []
    for b, n_kf in enumerate((5, 4, 6)):
        s, gt = scene(n_kf=n_kf, n_pt=25, obs_per_pt=3, seed=300 + b, n_fixed=2)
        if b != 1:
            synth.ba_add_rpcs(s, gt, seed=b)
            assert s["img_const"][0] and s["img_const"][1] and s["rpc"][0]["img1"] == 0 and s["rpc"][0]["img2"] == 1
            bad = s["rpc"][-1:].copy()
            bad["img2"] = n_kf
            s["rpc"] = np.concatenate([s["rpc"], bad])
        rows.append(s)
    return rows


def collect(ba, n, local_scene_of=(0,)):
    """Everything the entry points answer for the loaded problems, as a list of (name, bytes)."""
    out = [("pcg_form", repr(ba.pcg_form()).encode())]
    ci, cf = ba.initAndSolve()
    out += [("cost_initial", ci.tobytes()), ("cost_final", cf.tobytes())]
    for p in range(n):
        pose, pt, it = ba.state(p)
        out += [(f"pose{p}", pose.tobytes()), (f"pt{p}", pt.tobytes()), (f"pcg{p}", bytes([it & 255])), (f"residuals{p}", ba.residuals(p).tobytes())]
    for p in local_scene_of:
        ba.reset()
        marked, c0, c1, pose, pt, flags = ba.solve_local_scene(CHI2_MONO, CHI2_STEREO, problem=p)
        out += [(f"marked{p}", repr(marked).encode()), (f"ls_cost{p}", np.array([c0, c1]).tobytes()), (f"ls_pose{p}", pose.tobytes()),
                (f"ls_pt{p}", pt.tobytes()), (f"flags{p}", flags.tobytes())]
    return out


def load_host(o, explicit_schur=True):
    from snake_slam_amd.ba import BARec, lba_options

    ba = BARec(lba_options(), explicit_schur=explicit_schur)
    ba.create([M.row_scene(o, s, K, BF) for s in range(len(o["result"]))])
    return ba


def load_dev(o, explicit_schur=True, ba=None):
    """-> (handle, the device rows: alive until the caller drops them)."""
    import torch
    from snake_slam_amd.ba import BARec, lba_options

    d = M.rows_to_device(o)
    torch.cuda.synchronize()  # the rows' producer (the copies above) is complete before the BA handle's stream reads them
    ba = ba or BARec(lba_options(), explicit_schur=explicit_schur)
    ba.create_dev(d, K, BF)
    return ba, d


def both_ways(rows, caps=None, local_scene_of=(0,), explicit_schur=True):
    """Loads ``rows`` both ways and returns (host results, device results, the padded rows)."""
    o = M.pad_rows(rows, caps)
    n = len(rows)
    ba = load_host(o, explicit_schur)
    want = collect(ba, n, local_scene_of)
    ba.close()
    ba, keep = load_dev(o, explicit_schur)
    got = collect(ba, n, local_scene_of)
    ba.close()
    del keep
    return want, got, o


def assert_same(want, got):
    assert [k for k, _ in want] == [k for k, _ in got]
    for (k, a), (_, b) in zip(want, got):
        assert a == b, f"{k} differs between the hand-over from host arrays and the one from device rows"
