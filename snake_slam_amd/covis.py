"""Host-side mirror of the covisibility entry points over the C ABI.

``CovisibilityGraph`` runs ``Keyframe::UpdateConnections`` (reference Snake/Map/Keyframe.cpp:89-171) for many query keyframes per call
and the vote at the head of ``Tracking::UpdateLocalKeyFrames2`` (reference Snake/Tracking/TrackingFine.cpp:230-268) for many frames
per call, semantics "snk-covis v1" (DESIGN.md section 3i), from the map given as tables: per keyframe a bad flag, per point its
observation list as (kf, feature) pairs and two flag bits, per keyframe its features as point ids and depths.  The lists come back
ascending by (weight, kf); applying them (AddConnection, parent / child, the local-map assembly) stays with the caller.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .matcher import _Handle, _ptr

MAX_KF = 32768
MAX_CAP = 4096
OK, UNCHANGED, BAD_INDEX = 0, 1, 2
PT_BAD, PT_FAR = 1, 2

CONN_DTYPE = np.dtype([("weight", "<i4"), ("kf", "<i4")])
RESULT_DTYPE = np.dtype([("n_found", "<i4"), ("n_conn", "<i4"), ("best_kf", "<i4"), ("status", "<i4")])


class CovisMap(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("n_points", C.c_int32), ("n_obs", C.c_int32), ("kf_bad", C.c_void_p), ("obs_start", C.c_void_p),
                ("obs", C.c_void_p), ("pt_flags", C.c_void_p)]


class CovisParams(C.Structure):
    _fields_ = [("th", C.c_int32), ("th_depth", C.c_float), ("cap", C.c_int32)]


def _host_map(kf_bad, obs_start, obs, pt_flags):
    bad = np.ascontiguousarray(kf_bad, np.uint8).reshape(-1)
    start = np.ascontiguousarray(obs_start, np.int32).reshape(-1)
    o = np.ascontiguousarray(obs, np.int32).reshape(-1, 2)
    flags = np.ascontiguousarray(pt_flags, np.uint8).reshape(-1)
    if len(start) != len(flags) + 1:
        raise ValueError("obs_start must have n_points + 1 entries")
    keep = (bad, start, o, flags)
    return CovisMap(len(bad), len(flags), len(o), _ptr(bad), _ptr(start), _ptr(o), _ptr(flags)), keep


def _dev_map(kf_bad, obs_start, obs, pt_flags):
    return CovisMap(int(kf_bad.shape[0]), int(pt_flags.shape[0]), int(obs.shape[0]), kf_bad.data_ptr(), obs_start.data_ptr(), obs.data_ptr(),
                    pt_flags.data_ptr())


class CovisibilityGraph(_Handle):
    """``th`` / ``th_depth``: Keyframe.cpp:135 / :111; ``cap``: entries of a list kept per set (the LAST cap of it)."""

    def __init__(self, th: int = 15, th_depth: float = 40.0, cap: int = 256, device: int = 0, stream: int | None = None):
        super().__init__(device, stream)
        self.th, self.th_depth, self.cap = int(th), float(th_depth), int(cap)

    def _params(self):
        return CovisParams(self.th, self.th_depth, self.cap)

    def _outputs(self, n):
        conn = np.empty((max(n, 0), max(self.cap, 1)), CONN_DTYPE)
        conn["weight"] = conn["kf"] = -1
        return conn, np.zeros(max(n, 0), RESULT_DTYPE)

    def update(self, kf_bad, obs_start, obs, pt_flags, feat_start, feat_point, feat_depth, q):
        """snk_covis_update.  kf_bad [n_kf] uint8; obs_start [n_points + 1], obs [n_obs, 2] (kf, feature), pt_flags [n_points]
        (PT_BAD | PT_FAR); feat_start [n_kf + 1], feat_point [n_feat] (-1: none), feat_depth [n_feat] float32; q: the query
        keyframes.  Returns (conn [n_q, cap] CONN_DTYPE, result [n_q] RESULT_DTYPE); conn[s, :n_conn] is the list's tail, ascending,
        the entries behind it are (-1, -1)."""
        cmap, keep = _host_map(kf_bad, obs_start, obs, pt_flags)
        fs = np.ascontiguousarray(feat_start, np.int32).reshape(-1)
        fp = np.ascontiguousarray(feat_point, np.int32).reshape(-1)
        fd = np.ascontiguousarray(feat_depth, np.float32).reshape(-1)
        qq = np.ascontiguousarray(q, np.int32).reshape(-1)
        if len(fs) != cmap.n_kf + 1 or len(fp) != len(fd) or (len(fs) and len(fp) < max(int(fs[-1]), 0)):
            raise ValueError("array lengths")
        conn, res = self._outputs(len(qq))
        par = self._params()
        _lib.check(self._lib.snk_covis_update(self._h, C.byref(cmap), _ptr(fs), _ptr(fp), _ptr(fd), C.byref(par), len(qq), _ptr(qq), _ptr(conn),
                                              _ptr(res)), "snk_covis_update")
        del keep
        return conn, res

    def vote(self, kf_bad, obs_start, obs, pt_flags, set_start, set_point):
        """snk_covis_vote.  Set s is the point ids set_point[set_start[s] : set_start[s + 1]] (-1: none; a padded [batch, cap] array with
        set_start = arange(batch + 1) * cap is fine).  Returns (conn, result) as update does; best_kf is the reference keyframe."""
        cmap, keep = _host_map(kf_bad, obs_start, obs, pt_flags)
        ss = np.ascontiguousarray(set_start, np.int32).reshape(-1)
        sp = np.ascontiguousarray(set_point, np.int32).reshape(-1)
        if len(ss) < 1 or len(sp) < max(int(ss[-1]), 0):
            raise ValueError("array lengths")
        conn, res = self._outputs(len(ss) - 1)
        par = self._params()
        _lib.check(self._lib.snk_covis_vote(self._h, C.byref(cmap), len(ss) - 1, _ptr(ss), _ptr(sp), C.byref(par), _ptr(conn), _ptr(res)),
                   "snk_covis_vote")
        del keep
        return conn, res

    def update_dev(self, kf_bad, obs_start, obs, pt_flags, feat_start, feat_point, feat_depth, q, conn, out):
        """snk_covis_update_batch_dev: device tensors of the dtypes above (conn [n_q, cap, 2] int32, out [n_q, 4] int32).  Asynchronous
        on the handle's stream; a set with an index out of range has status BAD_INDEX."""
        cmap, par = _dev_map(kf_bad, obs_start, obs, pt_flags), self._params()
        _lib.check(self._lib.snk_covis_update_batch_dev(self._h, C.byref(cmap), feat_start.data_ptr(), int(feat_point.shape[0]), feat_point.data_ptr(),
                                                        feat_depth.data_ptr(), C.byref(par), int(q.shape[0]), q.data_ptr(), conn.data_ptr(),
                                                        out.data_ptr()), "snk_covis_update_batch_dev")

    def vote_dev(self, kf_bad, obs_start, obs, pt_flags, set_start, set_point, conn, out):
        """snk_covis_vote_batch_dev: set_start [n_sets + 1], set_point [n] (any shape, its element count is what the starts are checked
        against), conn [n_sets, cap, 2] int32, out [n_sets, 4] int32."""
        cmap, par = _dev_map(kf_bad, obs_start, obs, pt_flags), self._params()
        _lib.check(self._lib.snk_covis_vote_batch_dev(self._h, C.byref(cmap), int(set_start.shape[0]) - 1, set_start.data_ptr(), int(set_point.numel()),
                                                      set_point.data_ptr(), C.byref(par), conn.data_ptr(), out.data_ptr()),
                   "snk_covis_vote_batch_dev")

