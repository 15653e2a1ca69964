"""Host-side mirror of the local-BA-window entry points over the C ABI.

``LocalSceneBuilder`` runs ``LocalBundleAdjustment::MakeLocalScene`` (reference Snake/Optimizer/LocalBundleAdjustment.cpp:94-346) for many
keyframes per call, semantics "snk-scene v1" (DESIGN.md section 3k): ``window`` picks the keyframes (:124-151), ``gather`` builds the
points, the images, the observation records and the IMU constraints (:154-346), laid out as ``snk_ba_problem`` takes them, plus the inverse
maps ``img_kf`` / ``pt_id`` / ``obs_src`` that ``UpdateLocalScene`` needs.  ``ba_problem`` / ``ba_scene`` point a BA problem at one row.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .ba import BA_RPC_DTYPE, BaProblem
from .covis import CONN_DTYPE
from .matcher import _Handle, _ptr

MAX_WINDOW = 64
MAX_IMG = 4096
MAX_OBS = 1 << 22
OK, SKIPPED, WINDOW_OVERFLOW, PTS_OVERFLOW, IMG_OVERFLOW, OBS_OVERFLOW, BAD_INDEX = range(7)
PT_BAD, PT_CONST = 1, 4

WINDOW_DTYPE = np.dtype([("n_window", "<i4"), ("status", "<i4")])
RESULT_DTYPE = np.dtype([("n_window", "<i4"), ("n_img", "<i4"), ("n_pt", "<i4"), ("n_obs", "<i4"), ("n_rpc", "<i4"), ("status", "<i4")])

# the tables of snk_scene_map in the struct's order: (name, dtype, trailing shape); the last five are the optional IMU tables
MAP_TABLES = (("kf_bad", np.uint8, ()), ("kf_prev", np.int32, ()), ("kf_pose", np.float64, (7,)), ("feat_start", np.int32, ()),
              ("feat_point", np.int32, ()), ("feat_depth", np.float32, ()), ("feat_uv", np.float32, (2,)), ("feat_octave", np.int32, ()),
              ("obs_start", np.int32, ()), ("obs", np.int32, (2,)), ("pt_flags", np.uint8, ()), ("pt_pos", np.float64, (3,)),
              ("level_inv_sq_scale", np.float32, ()), ("kf_time", np.float64, ()), ("kf_imu_begin", np.float64, ()),
              ("kf_imu_end", np.float64, ()), ("kf_preint_valid", np.uint8, ()), ("kf_rpc", BA_RPC_DTYPE, ()))
IMU_TABLES = ("kf_time", "kf_imu_begin", "kf_imu_end", "kf_preint_valid", "kf_rpc")
# the rows of snk_scene_out in the struct's order: (name, dtype, which cap, trailing shape)
OUT_ROWS = (("img_kf", np.int32, "img_cap", ()), ("pose", np.float64, "img_cap", (7,)), ("img_const", np.uint8, "img_cap", ()),
            ("pt_id", np.int32, "pt_cap", ()), ("pt", np.float64, "pt_cap", (3,)), ("pt_const", np.uint8, "pt_cap", ()),
            ("pt_valid", np.uint8, "pt_cap", ()), ("obs_img", np.int32, "obs_cap", ()), ("obs_pt", np.int32, "obs_cap", ()),
            ("obs_uv", np.float64, "obs_cap", (2,)), ("obs_depth", np.float64, "obs_cap", ()), ("obs_weight", np.float64, "obs_cap", ()),
            ("obs_src", np.int32, "obs_cap", (2,)), ("rpc", BA_RPC_DTYPE, "win_cap", ()))


class SceneMap(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_kf", "n_points", "n_obs", "n_feat", "n_levels")] + [(n, C.c_void_p) for n, _, _ in MAP_TABLES]


class SceneParams(C.Structure):
    _fields_ = [("n_neighbours", C.c_int32), ("n_last", C.c_int32), ("gyro_weight", C.c_double), ("acc_weight", C.c_double)]


class SceneOut(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("win_cap", "pt_cap", "img_cap", "obs_cap")] + [(n, C.c_void_p) for n, _, _, _ in OUT_ROWS] + [
        ("result", C.c_void_p)]


def host_map(tables: dict):
    """The tables as contiguous numpy arrays of the ABI's dtypes (the IMU tables: all or none) and the snk_scene_map over them."""
    a = {}
    for name, dt, tail in MAP_TABLES:
        if name in IMU_TABLES and tables.get(name) is None:
            continue
        a[name] = np.ascontiguousarray(tables[name], dt).reshape((-1,) + tail)
    if 0 < sum(n in a for n in IMU_TABLES) < len(IMU_TABLES):
        raise ValueError("the IMU tables are either all absent or all present")
    n_kf, n_points = len(a["kf_bad"]), len(a["pt_flags"])
    if (len(a["feat_start"]) != n_kf + 1 or len(a["obs_start"]) != n_points + 1 or len(a["kf_prev"]) != n_kf or len(a["kf_pose"]) != n_kf
            or len(a["pt_pos"]) != n_points or any(len(a[n]) != len(a["feat_point"]) for n in ("feat_depth", "feat_uv", "feat_octave"))
            or any(len(a[n]) != n_kf for n in IMU_TABLES if n in a)):
        raise ValueError("array lengths")
    m = SceneMap(n_kf, n_points, len(a["obs"]), len(a["feat_point"]), len(a["level_inv_sq_scale"]),
                 *[_ptr(a[n]) if n in a else None for n, _, _ in MAP_TABLES])
    return m, a


def device_map(t: dict) -> SceneMap:
    """snk_scene_map over device tensors of the same names and dtypes (kf_rpc: [n_kf, 80] uint8 or any tensor of that size)."""
    return SceneMap(int(t["kf_bad"].shape[0]), int(t["pt_flags"].shape[0]), int(t["obs"].shape[0]), int(t["feat_point"].shape[0]),
                    int(t["level_inv_sq_scale"].shape[0]), *[t[n].data_ptr() if t.get(n) is not None else None for n, _, _ in MAP_TABLES])


def host_outputs(n_q: int, win_cap: int, pt_cap: int, img_cap: int, obs_cap: int, fill=None) -> dict:
    """The output rows of snk_scene_gather as numpy arrays (zeros, pt_id -1; ``fill``: a byte pattern instead) plus the caps."""
    caps = dict(win_cap=int(win_cap), pt_cap=int(pt_cap), img_cap=int(img_cap), obs_cap=int(obs_cap))
    o = dict(caps)
    for name, dt, cap, tail in OUT_ROWS:
        o[name] = np.zeros((n_q, caps[cap]) + tail, dt)
        if fill is not None:
            o[name].view(np.uint8)[...] = fill
        elif name == "pt_id":
            o[name][...] = -1
    o["result"] = np.zeros(n_q, RESULT_DTYPE)
    return o


def out_struct(o: dict) -> SceneOut:
    """snk_scene_out over numpy arrays or device tensors named as OUT_ROWS, ``result`` and the four caps."""
    def ptr(x):
        return None if x is None else (x.data_ptr() if hasattr(x, "data_ptr") else _ptr(x))

    return SceneOut(o["win_cap"], o["pt_cap"], o["img_cap"], o["obs_cap"], *[ptr(o.get(n)) for n, _, _, _ in OUT_ROWS], ptr(o["result"]))


def ba_scene(o: dict, s: int, K, bf: float) -> dict:
    """Row ``s`` of host outputs as the scene dict that ``BARec.create`` takes: views, nothing is copied."""
    r = o["result"][s]
    if r["status"] != OK:
        raise ValueError(f"query {s} has status {int(r['status'])}")
    ni, npt, no, nr = int(r["n_img"]), int(r["n_pt"]), int(r["n_obs"]), int(r["n_rpc"])
    return dict(pose=o["pose"][s, :ni], img_const=o["img_const"][s, :ni], pt=o["pt"][s, :npt], pt_const=o["pt_const"][s, :npt],
                obs_img=o["obs_img"][s, :no], obs_pt=o["obs_pt"][s, :no], obs_uv=o["obs_uv"][s, :no], obs_depth=o["obs_depth"][s, :no],
                obs_weight=o["obs_weight"][s, :no], rpc=o["rpc"][s, :nr], K=list(K), bf=float(bf))


def ba_problem(o: dict, s: int, K, bf: float) -> BaProblem:
    """A snk_ba_problem that points at row ``s`` of host outputs (which must stay alive while it is used)."""
    sc = ba_scene(o, s, K, bf)
    P = BaProblem()
    P.n_img, P.n_pt, P.n_obs = len(sc["pose"]), len(sc["pt"]), len(sc["obs_img"])
    for k in ("pose", "img_const", "pt", "pt_const", "obs_img", "obs_pt", "obs_uv", "obs_depth", "obs_weight"):
        setattr(P, k, sc[k].ctypes.data if sc[k].size else 0)
    P.K[:] = list(K)
    P.bf = float(bf)
    P.n_rpc, P.pad, P.rpc = len(sc["rpc"]), 0, (sc["rpc"].ctypes.data if len(sc["rpc"]) else 0)
    return P


class LocalSceneBuilder(_Handle):
    """``params``: a dict or keywords n_neighbours (15), n_last (20), win_cap (36), gyro_weight (0), acc_weight (0):
    LocalBundleAdjustment.cpp:126, :132, :296."""

    def __init__(self, params: dict | None = None, device: int = 0, stream: int | None = None, **kw):
        super().__init__(device, stream)
        p = dict(n_neighbours=15, n_last=20, win_cap=36, gyro_weight=0.0, acc_weight=0.0)
        p.update(params or {})
        p.update(kw)
        self.params = p
        self.win_cap = int(p["win_cap"])

    def _params(self):
        p = self.params
        return SceneParams(int(p["n_neighbours"]), int(p["n_last"]), float(p["gyro_weight"]), float(p["acc_weight"]))

    def window(self, q, kf_bad, kf_prev, conn_start, conn_list):
        """snk_scene_window.  q [n_q]; kf_bad [n_kf] uint8; kf_prev [n_kf] int32; conn_start [n_kf + 1], conn_list CONN_DTYPE ascending by
        (weight, kf).  Returns (window_kf [n_q, win_cap] int32, -1 past n_window; result [n_q] WINDOW_DTYPE)."""
        qq = np.ascontiguousarray(q, np.int32).reshape(-1)
        bad = np.ascontiguousarray(kf_bad, np.uint8).reshape(-1)
        prev = np.ascontiguousarray(kf_prev, np.int32).reshape(-1)
        cs = np.ascontiguousarray(conn_start, np.int32).reshape(-1)
        cl = np.ascontiguousarray(conn_list, CONN_DTYPE).reshape(-1)
        if len(cs) != len(bad) + 1 or len(prev) != len(bad) or len(cl) < max(int(cs[-1]), 0):
            raise ValueError("array lengths")
        win = np.full((len(qq), max(self.win_cap, 1)), -1, np.int32)
        res = np.zeros(len(qq), WINDOW_DTYPE)
        par = self._params()
        _lib.check(self._lib.snk_scene_window(self._h, len(qq), _ptr(qq), len(bad), _ptr(bad), _ptr(prev), _ptr(cs), _ptr(cl), C.byref(par), self.win_cap,
                                              _ptr(win), _ptr(res)), "snk_scene_window")
        return win, res

    def gather(self, tables: dict, window_kf, win, pt_cap: int, img_cap: int, obs_cap: int, out: dict | None = None):
        """snk_scene_gather.  tables: the arrays of MAP_TABLES by name; window_kf, win: what ``window`` returned.  Returns the dict of
        ``host_outputs`` (or fills ``out``): rows past a query's counts keep what they held."""
        cmap, keep = host_map(tables)
        wr = np.ascontiguousarray(win, WINDOW_DTYPE).reshape(-1)
        wk = np.ascontiguousarray(window_kf, np.int32).reshape(len(wr), -1) if len(wr) else np.zeros((0, self.win_cap), np.int32)
        if len(wr) and wk.shape[1] != self.win_cap:
            raise ValueError("window_kf must have win_cap columns")
        o = out if out is not None else host_outputs(len(wr), self.win_cap, pt_cap, img_cap, obs_cap)
        cout, par = out_struct(o), self._params()
        _lib.check(self._lib.snk_scene_gather(self._h, len(wr), C.byref(cmap), _ptr(wk), _ptr(wr), C.byref(par), C.byref(cout)), "snk_scene_gather")
        del keep
        return o

    def window_dev(self, q, kf_bad, kf_prev, conn_start, conn_list, window_kf, out):
        """snk_scene_window_batch_dev: device tensors (conn_list [n_list, 2] int32, window_kf [n_q, win_cap] int32, out [n_q, 2] int32).
        Asynchronous on the handle's stream; a query with an index out of range has status BAD_INDEX."""
        par = self._params()
        _lib.check(self._lib.snk_scene_window_batch_dev(self._h, int(q.shape[0]), q.data_ptr(), int(kf_bad.shape[0]), kf_bad.data_ptr(), kf_prev.data_ptr(),
                                                        conn_start.data_ptr(), int(conn_list.shape[0]), conn_list.data_ptr(), C.byref(par),
                                                        int(window_kf.shape[1]), window_kf.data_ptr(), out.data_ptr()), "snk_scene_window_batch_dev")

    def gather_dev(self, tables: dict, window_kf, win, out: dict):
        """snk_scene_gather_batch_dev: ``tables`` and ``out`` hold device tensors (out: the rows of OUT_ROWS, result [n_q, 6] int32 and the
        four caps; rpc [n_q, win_cap, 80] uint8)."""
        cmap, cout, par = device_map(tables), out_struct(out), self._params()
        _lib.check(self._lib.snk_scene_gather_batch_dev(self._h, int(win.shape[0]), C.byref(cmap), window_kf.data_ptr(), win.data_ptr(), C.byref(par),
                                                        C.byref(cout)), "snk_scene_gather_batch_dev")
