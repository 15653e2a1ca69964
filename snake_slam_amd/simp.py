"""Host-side mirror of the keyframe-culling entry points over the C ABI.

``KeyframeCuller`` runs ``Simplification::KeyFrameCullingGraph`` and ``Redundancy`` (reference Snake/Optimizer/Simplification.cpp:148-358,
:75-146), ``Keyframe::MatchCount`` and ``ComputeDepthRange`` (reference Snake/Map/Keyframe.cpp:68-77, :175-206) for many keyframes per
call, semantics "snk-simp v1" (DESIGN.md section 3l): ``stats`` computes the per-keyframe statistics from the map tables, ``decide`` the
verdicts from the connection lists, ``process`` does what ``Simplification::Process`` does around the decision.  Applying a verdict
(EraseKeyframe, the re-queue of the three best covisible keyframes) stays with the caller.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .covis import CONN_DTYPE, OK as COVIS_OK
from .matcher import _Handle, _ptr

MAX_NODES = 256
MAX_FEAT = 16384
OK, SKIPPED, FEAT_OVERFLOW, NODES_OVERFLOW, BAD_INDEX = range(5)
NONE, FACTOR, NO_CONN, ANGLE, MATCHES, REDUNDANCY, LINK, KEEP_IMU_WEIGHTS, KEEP_TIME_GAP, KEEP_BRANCH, KEEP_DISCONNECTED, KEEP_LINK = range(12)
REASON_NAMES = ("", "Factor", "No Conn.", "Angle", "Matches", "Redu.", "Link", "", "", "", "", "")  # the reference's strings (:152 .. :353)

STATS_DTYPE = np.dtype([("median_depth", "<f4"), ("n_depth", "<i4"), ("match_count", "<i4"), ("n_mps", "<i4"), ("n_redundant", "<i4"),
                        ("redundancy", "<f4"), ("status", "<i4")])
VERDICT_DTYPE = np.dtype([("reason", "<i4"), ("cull", "<i4"), ("value", "<f8"), ("n_nodes", "<i4"), ("n_root_edges", "<i4"),
                          ("weakest_link", "<i4"), ("status", "<i4")])

# the tables of snk_simp_map / snk_simp_graph in the structs' order: (name, dtype, trailing shape)
MAP_TABLES = (("kf_bad", np.uint8, ()), ("kf_pose", np.float64, (7,)), ("feat_start", np.int32, ()), ("feat_point", np.int32, ()),
              ("feat_depth", np.float32, ()), ("feat_octave", np.int32, ()), ("obs_start", np.int32, ()), ("obs", np.int32, (2,)),
              ("pt_flags", np.uint8, ()), ("pt_pos", np.float64, (3,)))
GRAPH_TABLES = (("kf_bad", np.uint8, ()), ("kf_pose", np.float64, (7,)), ("kf_cull_factor", np.float32, ()), ("kf_median_depth", np.float64, ()),
                ("kf_prev", np.int32, ()), ("kf_next", np.int32, ()), ("kf_time", np.float64, ()), ("conn_start", np.int32, ()),
                ("conn_list", CONN_DTYPE, ()))
TIME_TABLES = ("kf_prev", "kf_next", "kf_time")


class SimpMap(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_kf", "n_points", "n_obs", "n_feat")] + [(n, C.c_void_p) for n, _, _ in MAP_TABLES]


class SimpStatsParams(C.Structure):
    _fields_ = [("min_obs", C.c_int32), ("stereo", C.c_int32), ("th_depth", C.c_float), ("feat_cap", C.c_int32)]


class SimpGraph(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("n_list", C.c_int32)] + [(n, C.c_void_p) for n, _, _ in GRAPH_TABLES]


class SimpParams(C.Structure):
    _fields_ = [("min_matches_in_graph", C.c_int32), ("border_angle", C.c_float), ("border_redundancy", C.c_float), ("border_matches", C.c_int32),
                ("th_map", C.c_int32), ("with_imu", C.c_int32), ("gyro_weight", C.c_double), ("acc_weight", C.c_double),
                ("max_time_between_kf", C.c_float)]


def host_map(tables: dict):
    """The tables as contiguous numpy arrays of the ABI's dtypes and the snk_simp_map over them."""
    a = {name: np.ascontiguousarray(tables[name], dt).reshape((-1,) + tail) for name, dt, tail in MAP_TABLES}
    n_kf, n_points, n_feat = len(a["kf_bad"]), len(a["pt_flags"]), len(a["feat_point"])
    if (len(a["feat_start"]) != n_kf + 1 or len(a["obs_start"]) != n_points + 1 or len(a["kf_pose"]) != n_kf or len(a["pt_pos"]) != n_points
            or len(a["feat_depth"]) != n_feat or len(a["feat_octave"]) != n_feat):
        raise ValueError("array lengths")
    return SimpMap(n_kf, n_points, len(a["obs"]), n_feat, *[_ptr(a[n]) for n, _, _ in MAP_TABLES]), a


def device_map(t: dict) -> SimpMap:
    """snk_simp_map over device tensors of the same names and dtypes (obs [n_obs, 2] int32)."""
    return SimpMap(int(t["kf_bad"].shape[0]), int(t["pt_flags"].shape[0]), int(t["obs"].shape[0]), int(t["feat_point"].shape[0]),
                   *[t[n].data_ptr() for n, _, _ in MAP_TABLES])


def host_graph(tables: dict):
    """The keyframe side as contiguous numpy arrays (the time tables: all or none) and the snk_simp_graph over them."""
    a = {}
    for name, dt, tail in GRAPH_TABLES:
        if name in TIME_TABLES and tables.get(name) is None:
            continue
        a[name] = np.ascontiguousarray(tables[name], dt).reshape((-1,) + tail)
    if 0 < sum(n in a for n in TIME_TABLES) < len(TIME_TABLES):
        raise ValueError("kf_prev, kf_next and kf_time are either all absent or all present")
    n_kf = len(a["kf_bad"])
    if len(a["conn_start"]) != n_kf + 1 or any(len(a[n]) != n_kf for n in a if n.startswith("kf_")) or len(a["conn_list"]) < max(int(a["conn_start"][-1]), 0):
        raise ValueError("array lengths")
    return SimpGraph(n_kf, len(a["conn_list"]), *[_ptr(a[n]) if n in a else None for n, _, _ in GRAPH_TABLES]), a


def device_graph(t: dict) -> SimpGraph:
    """snk_simp_graph over device tensors (conn_list [n_list, 2] int32; the time tables None or all present)."""
    return SimpGraph(int(t["kf_bad"].shape[0]), int(t["conn_list"].shape[0]),
                     *[t[n].data_ptr() if t.get(n) is not None else None for n, _, _ in GRAPH_TABLES])


class KeyframeCuller(_Handle):
    """``params``: a dict or keywords -- min_matches_in_graph (20), border_angle (1.0), border_redundancy (0.8), border_matches (80),
    th_map (140), with_imu (0), gyro_weight, acc_weight, max_time_between_kf (0.5): the settings Simplification.cpp reads; stereo (1),
    th_depth (40.0): Simplification.cpp:107-109; feat_cap (4096), node_cap (256): the sizes of the kernels' LDS."""

    DEFAULTS = dict(min_matches_in_graph=20, border_angle=1.0, border_redundancy=0.8, border_matches=80, th_map=140, with_imu=0, gyro_weight=0.0,
                    acc_weight=0.0, max_time_between_kf=0.5, stereo=1, th_depth=40.0, feat_cap=4096, node_cap=MAX_NODES)

    def __init__(self, params: dict | None = None, device: int = 0, stream: int | None = None, **kw):
        super().__init__(device, stream)
        p = dict(self.DEFAULTS)
        p.update(params or {})
        p.update(kw)
        unknown = set(p) - set(self.DEFAULTS)
        if unknown:
            raise ValueError(f"unknown parameters: {sorted(unknown)}")
        self.params = p

    def _stats_params(self, min_obs):
        p = self.params
        return SimpStatsParams(int(min_obs), int(p["stereo"]), float(p["th_depth"]), int(p["feat_cap"]))

    def _params(self):
        p = self.params
        return SimpParams(int(p["min_matches_in_graph"]), float(p["border_angle"]), float(p["border_redundancy"]), int(p["border_matches"]),
                          int(p["th_map"]), int(p["with_imu"]), float(p["gyro_weight"]), float(p["acc_weight"]), float(p["max_time_between_kf"]))

    # ---- stage 1 ----
    def stats(self, tables: dict, q, min_obs: int = 3, out=None):
        """snk_simp_stats.  tables: the arrays of MAP_TABLES by name; q: the query keyframes.  Returns [n_q] STATS_DTYPE."""
        cmap, keep = host_map(tables)
        qq = np.ascontiguousarray(q, np.int32).reshape(-1)
        res = out if out is not None else np.zeros(len(qq), STATS_DTYPE)
        par = self._stats_params(min_obs)
        _lib.check(self._lib.snk_simp_stats(self._h, C.byref(cmap), C.byref(par), len(qq), _ptr(qq), _ptr(res)), "snk_simp_stats")
        del keep
        return res

    def stats_dev(self, tables: dict, q, out, min_obs: int = 3):
        """snk_simp_stats_batch_dev: ``tables`` holds device tensors, q [n_q] int32, out [n_q, 7] int32 (the records of STATS_DTYPE).
        Asynchronous on the handle's stream; a query with an index out of range has status BAD_INDEX."""
        cmap, par = device_map(tables), self._stats_params(min_obs)
        _lib.check(self._lib.snk_simp_stats_batch_dev(self._h, C.byref(cmap), C.byref(par), int(q.shape[0]), q.data_ptr(), out.data_ptr()),
                   "snk_simp_stats_batch_dev")

    # ---- stage 2 ----
    def decide(self, graph: dict, q, stats, out=None):
        """snk_simp_decide.  graph: the arrays of GRAPH_TABLES by name (kf_median_depth already filled, see ``fill_median``); stats: the
        same queries' records of ``stats`` with min_obs = 3.  Returns [n_q] VERDICT_DTYPE."""
        cg, keep = host_graph(graph)
        qq = np.ascontiguousarray(q, np.int32).reshape(-1)
        st = np.ascontiguousarray(stats, STATS_DTYPE).reshape(-1)
        if len(st) != len(qq):
            raise ValueError("one stats record per query")
        res = out if out is not None else np.zeros(len(qq), VERDICT_DTYPE)
        par = self._params()
        _lib.check(self._lib.snk_simp_decide(self._h, C.byref(cg), C.byref(par), int(self.params["node_cap"]), len(qq), _ptr(qq), _ptr(st), _ptr(res)),
                   "snk_simp_decide")
        del keep
        return res

    def decide_dev(self, graph: dict, q, stats, out):
        """snk_simp_decide_batch_dev: device tensors; stats [n_q, 7] int32 as ``stats_dev`` left it, out [n_q, 8] int32 (the records of
        VERDICT_DTYPE).  Asynchronous."""
        cg, par = device_graph(graph), self._params()
        _lib.check(self._lib.snk_simp_decide_batch_dev(self._h, C.byref(cg), C.byref(par), int(self.params["node_cap"]), int(q.shape[0]), q.data_ptr(),
                                                       stats.data_ptr(), out.data_ptr()), "snk_simp_decide_batch_dev")

    # ---- Simplification::Process around the decision ----
    @staticmethod
    def fill_median(kf_median_depth, kf_bad, kf, stats):
        """The lazy rule of Keyframe.cpp:177, :199-202: entries <= 0 of live keyframes take stage 1's median where it saw a depth."""
        med = np.array(kf_median_depth, np.float64)
        for k, s in zip(np.asarray(kf).tolist(), stats):
            if med[k] <= 0 and not kf_bad[k] and s["status"] == OK and s["n_depth"] > 0:
                med[k] = np.float64(s["median_depth"])
        return med

    def process(self, q, tables: dict, graph: dict, covis):
        """What Simplification::Process does around the decision (Simplification.cpp:27-72, :203-208), for the keyframes ``q`` of one call:
        UpdateConnections of every q through ``covis`` (a CovisibilityGraph) -- a list that comes back OK replaces q's list in the
        connection store, UNCHANGED keeps it (Keyframe.cpp:125-129); adding q to the other keyframes' lists stays with the caller -- then
        stage 1 for q and for every live keyframe whose cached median is <= 0, the fill of the cache, and stage 2.  Every query sees the
        same tables.  Returns a dict: verdict [n_q], stats [n_q], kf_median_depth, conn_start, conn_list (the updated store)."""
        qq = np.ascontiguousarray(q, np.int32).reshape(-1)
        bad = np.ascontiguousarray(tables["kf_bad"], np.uint8)
        n_kf = len(bad)
        conn, res = covis.update(tables["kf_bad"], tables["obs_start"], tables["obs"], tables["pt_flags"], tables["feat_start"], tables["feat_point"],
                                 tables["feat_depth"], qq)
        cs, cl = np.asarray(graph["conn_start"], np.int64), np.ascontiguousarray(graph["conn_list"], CONN_DTYPE)
        lists = [cl[cs[k]:cs[k + 1]] for k in range(n_kf)]
        for i, k in enumerate(qq.tolist()):
            if res["status"][i] == COVIS_OK:
                lists[k] = conn[i, :res["n_conn"][i]]
        new_start = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
        new_list = np.concatenate(lists) if n_kf else np.zeros(0, CONN_DTYPE)
        cached = np.asarray(graph["kf_median_depth"], np.float64)
        stale = np.flatnonzero((cached <= 0) & (bad == 0)).astype(np.int32)
        todo = np.concatenate([qq, stale])
        st = self.stats(tables, todo, 3)
        median = self.fill_median(cached, bad, todo, st)
        g = dict(graph, kf_median_depth=median, conn_start=new_start, conn_list=new_list)
        verdict = self.decide(g, qq, st[:len(qq)])
        return dict(verdict=verdict, stats=st[:len(qq)], kf_median_depth=median, conn_start=new_start, conn_list=new_list)
