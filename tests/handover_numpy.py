"""The fill pass of the BA hand-over restated in numpy, independently of snake_slam_amd/csrc/handover_core.hpp: which observations of a
problem count, the free-camera index of every image, the stable order by point, and the two flags (a free camera twice on a point; a point
with more than eight observations by free cameras).  tests/test_handover_core_cpu.py holds the C++ statements to it; the GPU tests use
``pad_rows`` to lay scenes out as the rows snk_ba_set_problems_dev takes."""
import numpy as np

THREADS = 256     # HO_THREADS: a chunk of the fill kernel
MAX_PTS = 8192    # HO_MAX_PTS
MAX_RUN = 1024    # HO_MAX_RUN
DUP_MAX_CAMS = 512


def fill(img_const, pt_const, obs_img, obs_pt):
    """-> dict(nfc, no, k_over8, dup, long_run, cam_idx [n_img], pt_start [n_pt + 1], valid [n_obs], order [no], o_cam [no])."""
    img_const = np.asarray(img_const).astype(bool)
    pt_const = np.asarray(pt_const).astype(bool)
    obs_img = np.asarray(obs_img, np.int64)
    obs_pt = np.asarray(obs_pt, np.int64)
    n_img, n_pt = len(img_const), len(pt_const)
    in_range = (obs_img >= 0) & (obs_img < n_img) & (obs_pt >= 0) & (obs_pt < n_pt)
    i = np.where(in_range, obs_img, 0)
    p = np.where(in_range, obs_pt, 0)
    ic = img_const[i] if n_img else np.zeros(len(i), bool)
    pc = pt_const[p] if n_pt else np.zeros(len(p), bool)
    valid = in_range & ~(ic & pc)
    cam_idx = np.where(img_const, -1, np.cumsum(~img_const) - 1).astype(np.int32)
    nfc = int((~img_const).sum())
    order = np.flatnonzero(valid)
    order = order[np.argsort(obs_pt[order], kind="stable")]
    counts = np.bincount(obs_pt[valid], minlength=n_pt) if n_pt else np.zeros(0, np.int64)
    pt_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    free = in_range & ~ic
    k_over8 = bool(n_pt and (np.bincount(obs_pt[free], minlength=n_pt) > 8).any())
    o_cam = cam_idx[obs_img[order]] if len(order) else np.zeros(0, np.int32)
    dup = False
    if nfc <= DUP_MAX_CAMS and len(order):
        seen = set()
        for pp, c in zip(obs_pt[order].tolist(), o_cam.tolist()):
            if c >= 0:
                dup = dup or (pp, c) in seen
                seen.add((pp, c))
    return dict(nfc=nfc, no=len(order), k_over8=int(k_over8), dup=int(dup), long_run=int(bool(len(counts) and counts.max() > MAX_RUN)), cam_idx=cam_idx,
                pt_start=pt_start, valid=valid.astype(np.int32), order=order.astype(np.int32), o_cam=o_cam.astype(np.int32))


def pad_rows(scenes, caps=None, statuses=None, win_cap=4):
    """Scene dicts (synth.ba_scene, ba_add_rpcs; None: an empty row) as the rows of snk_scene_out, numpy, padded to the caps with a pattern
    that is no valid value.  caps: dict(pt_cap, img_cap, obs_cap) or None for the largest count of each (at least 1)."""
    from snake_slam_amd.ba import BA_RPC_DTYPE
    from snake_slam_amd.scene import OK, SKIPPED, host_outputs

    n = len(scenes)
    count = lambda s, k: 0 if s is None else len(s[k])  # noqa: E731
    caps = dict(caps or {})
    caps.setdefault("img_cap", max([count(s, "pose") for s in scenes] + [1]))
    caps.setdefault("pt_cap", max([count(s, "pt") for s in scenes] + [1]))
    caps.setdefault("obs_cap", max([count(s, "obs_img") for s in scenes] + [1]))
    win_cap = max([win_cap] + [len(s.get("rpc", ())) for s in scenes if s is not None])
    o = host_outputs(n, win_cap, caps["pt_cap"], caps["img_cap"], caps["obs_cap"], fill=0xA5)
    for s, sc in enumerate(scenes):
        st = OK if sc is not None else SKIPPED
        if statuses is not None:
            st = statuses[s]
        if sc is None or st != OK:
            o["result"][s] = (0, 0, 0, 0, 0, st)
            continue
        ni, npt, no = len(sc["pose"]), len(sc["pt"]), len(sc["obs_img"])
        rpc = np.ascontiguousarray(sc.get("rpc", np.zeros(0, BA_RPC_DTYPE)), BA_RPC_DTYPE)
        for k, m in (("pose", ni), ("img_const", ni), ("pt", npt), ("pt_const", npt), ("obs_img", no), ("obs_pt", no), ("obs_uv", no), ("obs_depth", no),
                     ("obs_weight", no)):
            o[k][s, :m] = np.asarray(sc[k]).reshape((m,) + o[k].shape[2:])
        o["rpc"][s, :len(rpc)] = rpc
        o["result"][s] = (0, ni, npt, no, len(rpc), st)
    return o


def rows_to_device(o, device="cuda"):
    """The dict of ``pad_rows`` as device tensors (rpc as bytes, result [n, 6] int32)."""
    import torch

    d = dict(win_cap=o["win_cap"], pt_cap=o["pt_cap"], img_cap=o["img_cap"], obs_cap=o["obs_cap"])
    for k, v in o.items():
        if isinstance(v, np.ndarray):
            a = np.ascontiguousarray(v)
            if k == "rpc":
                a = a.view(np.uint8).reshape(a.shape[0], a.shape[1], 80)
            elif k == "result":
                a = a.view(np.int32).reshape(-1, 6)
            d[k] = torch.from_numpy(a.copy()).to(device)
    return d


def row_scene(o, s, K, bf):
    """Row s of ``pad_rows`` as the scene dict BARec.create takes (an empty scene for a row that is not OK)."""
    r = o["result"][s]
    ni, npt, no, nr = (int(r["n_img"]), int(r["n_pt"]), int(r["n_obs"]), int(r["n_rpc"])) if int(r["status"]) == 0 else (0, 0, 0, 0)
    return dict(pose=o["pose"][s, :ni].copy(), img_const=o["img_const"][s, :ni].copy(), pt=o["pt"][s, :npt].copy(), pt_const=o["pt_const"][s, :npt].copy(),
                obs_img=o["obs_img"][s, :no].copy(), obs_pt=o["obs_pt"][s, :no].copy(), obs_uv=o["obs_uv"][s, :no].copy(),
                obs_depth=o["obs_depth"][s, :no].copy(), obs_weight=o["obs_weight"][s, :no].copy(), rpc=o["rpc"][s, :nr].copy(), K=list(K), bf=float(bf))
