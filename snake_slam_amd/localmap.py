"""Host-side mirror of the local-map entry points over the C ABI.

``LocalMapBuilder`` assembles the local map of fine tracking for many frames per call, semantics "snk-lmap v1" (DESIGN.md section 3j):
``select`` is the rest of ``Tracking::UpdateLocalKeyFrames2`` behind the vote (reference Snake/Tracking/TrackingFine.cpp:272-323) -- the
direct keyframes, the draws, the neighbours --, ``gather`` is ``Tracking::UpdateLocalPoints`` with ``LocalMap::addPoint`` (:328-356,
Snake/Map/LocalMap.h:139-154).  Inputs are the tables the covisibility calls leave (``covis.py``); the outputs of ``gather_dev`` plug into
``snk_match_project_fine_batch_dev`` / ``_ro_dev`` without leaving the device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .covis import CONN_DTYPE, RESULT_DTYPE
from .matcher import _Handle, _ptr

MAX_LOCAL_KF = 256
MAX_PTS = 16384
MAX_NEIGHBOURS = 16
OK, EMPTY, TRUNCATED, KF_OVERFLOW, PTS_OVERFLOW, BAD_INDEX = range(6)

SELECT_DTYPE = np.dtype([("n_local", "<i4"), ("n_direct", "<i4"), ("n_indirect", "<i4"), ("reference_kf", "<i4"), ("status", "<i4")])
GATHER_DTYPE = np.dtype([("n_pts", "<i4"), ("n_searchable", "<i4"), ("n_own_new", "<i4"), ("status", "<i4")])
LM_FINE_DTYPE = np.dtype([("pos", "<f8", 3), ("normal", "<f8", 3), ("desc", "<u8", 4), ("reference_depth", "<f4"), ("reference_scale_level", "<i4"),
                          ("valid", "u1"), ("pad", "u1", 7)])
assert LM_FINE_DTYPE.itemsize == 96


class LmapParams(C.Structure):
    _fields_ = [("n_direct", C.c_int32), ("n_direct_prob", C.c_int32), ("n_indirect_prob", C.c_int32), ("n_neighbours", C.c_int32),
                ("kf_cap", C.c_int32), ("seed", C.c_uint64)]


class LmapMap(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("n_points", C.c_int32), ("n_feat", C.c_int32), ("feat_start", C.c_void_p), ("feat_point", C.c_void_p),
                ("pt_flags", C.c_void_p), ("pt_last_seen", C.c_void_p)]


class LmapPoints(C.Structure):
    _fields_ = [("pos", C.c_void_p), ("normal", C.c_void_p), ("desc", C.c_void_p), ("ref_depth", C.c_void_p), ("ref_level", C.c_void_p)]


class LocalMapBuilder(_Handle):
    """``params``: a dict or keywords n_direct (15), n_direct_prob (5), n_indirect_prob (5), n_neighbours (5), kf_cap (64), seed (0):
    TrackingFine.cpp:223-225, :301."""

    def __init__(self, params: dict | None = None, device: int = 0, stream: int | None = None, **kw):
        super().__init__(device, stream)
        p = dict(n_direct=15, n_direct_prob=5, n_indirect_prob=5, n_neighbours=5, kf_cap=64, seed=0)
        p.update(params or {})
        p.update(kw)
        self.params = p
        self.kf_cap = int(p["kf_cap"])

    def _params(self):
        p = self.params
        return LmapParams(int(p["n_direct"]), int(p["n_direct_prob"]), int(p["n_indirect_prob"]), int(p["n_neighbours"]), int(p["kf_cap"]),
                          int(p["seed"]) & 0xFFFFFFFFFFFFFFFF)

    def select(self, conn, vote, kf_bad, conn_start, conn_list, frame_id):
        """snk_lmap_select.  conn [n_sets, vote_cap] CONN_DTYPE and vote [n_sets] RESULT_DTYPE as CovisibilityGraph.vote returns them;
        kf_bad [n_kf] uint8; conn_start [n_kf + 1], conn_list [conn_start[-1]] CONN_DTYPE: every keyframe's connections ascending by
        (weight, kf); frame_id [n_sets].  Returns (local_kf [n_sets, kf_cap] int32 with -1 past n_local, result [n_sets] SELECT_DTYPE)."""
        cn = np.ascontiguousarray(conn, CONN_DTYPE)
        vt = np.ascontiguousarray(vote, RESULT_DTYPE).reshape(-1)
        n = len(vt)
        cn = cn.reshape(n, -1) if n else cn.reshape(0, max(cn.shape[-1] if cn.ndim > 1 else 1, 1))
        bad = np.ascontiguousarray(kf_bad, np.uint8).reshape(-1)
        cs = np.ascontiguousarray(conn_start, np.int32).reshape(-1)
        cl = np.ascontiguousarray(conn_list, CONN_DTYPE).reshape(-1)
        fid = np.ascontiguousarray(frame_id, np.int32).reshape(-1)
        if len(cs) != len(bad) + 1 or len(fid) != n or len(cl) < max(int(cs[-1]), 0):
            raise ValueError("array lengths")
        local = np.full((n, max(self.kf_cap, 1)), -1, np.int32)
        res = np.zeros(n, SELECT_DTYPE)
        par = self._params()
        _lib.check(self._lib.snk_lmap_select(self._h, n, _ptr(cn), cn.shape[1], _ptr(vt), len(bad), _ptr(bad), _ptr(cs), _ptr(cl), _ptr(fid), C.byref(par),
                                             _ptr(local), _ptr(res)), "snk_lmap_select")
        return local, res

    def gather(self, feat_start, feat_point, pt_flags, pt_last_seen, points, frame_id, local_kf, sel, set_start, set_point, pts_cap):
        """snk_lmap_gather.  feat_start [n_kf + 1], feat_point [n_feat], pt_flags [n_points] uint8, pt_last_seen [n_points] int32; points:
        a dict pos [n, 3] / normal [n, 3] float64, desc [n, 4] uint64, ref_depth [n] float32, ref_level [n] int32; local_kf, sel: what
        select returned; set_start / set_point: the vote's sets.  Returns (lm_pts [n_sets, pts_cap] LM_FINE_DTYPE, zero past n_pts;
        lm_point [n_sets, pts_cap] int32, -1 past n_pts; n_pts [n_sets] int32; result [n_sets] GATHER_DTYPE)."""
        fs = np.ascontiguousarray(feat_start, np.int32).reshape(-1)
        fp = np.ascontiguousarray(feat_point, np.int32).reshape(-1)
        fl = np.ascontiguousarray(pt_flags, np.uint8).reshape(-1)
        ls = np.ascontiguousarray(pt_last_seen, np.int32).reshape(-1)
        pos = np.ascontiguousarray(points["pos"], np.float64).reshape(-1, 3)
        nrm = np.ascontiguousarray(points["normal"], np.float64).reshape(-1, 3)
        dsc = np.ascontiguousarray(points["desc"], np.uint64).reshape(-1, 4)
        dep = np.ascontiguousarray(points["ref_depth"], np.float32).reshape(-1)
        lvl = np.ascontiguousarray(points["ref_level"], np.int32).reshape(-1)
        fid = np.ascontiguousarray(frame_id, np.int32).reshape(-1)
        sl = np.ascontiguousarray(sel, SELECT_DTYPE).reshape(-1)
        n = len(sl)
        lk = np.ascontiguousarray(local_kf, np.int32).reshape(n, -1) if n else np.zeros((0, self.kf_cap), np.int32)
        ss = np.ascontiguousarray(set_start, np.int32).reshape(-1)
        sp = np.ascontiguousarray(set_point, np.int32).reshape(-1)
        n_pts_all = len(fl)
        if (len(ls) != n_pts_all or any(len(a) != n_pts_all for a in (pos, nrm, dsc, dep, lvl)) or len(fid) != n or len(ss) != n + 1
                or len(sp) < max(int(ss[-1]), 0)):
            raise ValueError("array lengths")
        cap = max(int(pts_cap), 1)
        lm = np.zeros((n, cap), LM_FINE_DTYPE)
        ids = np.full((n, cap), -1, np.int32)
        n_pts = np.zeros(n, np.int32)
        res = np.zeros(n, GATHER_DTYPE)
        cmap = LmapMap(len(fs) - 1, n_pts_all, len(fp), _ptr(fs), _ptr(fp), _ptr(fl), _ptr(ls))
        cpts = LmapPoints(_ptr(pos), _ptr(nrm), _ptr(dsc), _ptr(dep), _ptr(lvl))
        _lib.check(self._lib.snk_lmap_gather(self._h, n, C.byref(cmap), C.byref(cpts), _ptr(fid), _ptr(lk), lk.shape[1], _ptr(sl), _ptr(ss), _ptr(sp),
                                             int(pts_cap), _ptr(lm), _ptr(ids), _ptr(n_pts), _ptr(res)), "snk_lmap_gather")
        return lm, ids, n_pts, res

    def select_dev(self, conn, vote, kf_bad, conn_start, conn_list, frame_id, local_kf, out):
        """snk_lmap_select_batch_dev: device tensors.  conn [n_sets, vote_cap, 2] int32 and vote [n_sets, 4] int32 as vote_dev leaves them,
        conn_list [n_list, 2] int32, local_kf [n_sets, kf_cap] int32, out [n_sets, 5] int32.  Asynchronous on the handle's stream; a
        set with an index out of range has status BAD_INDEX."""
        par = self._params()
        _lib.check(self._lib.snk_lmap_select_batch_dev(self._h, int(vote.shape[0]), conn.data_ptr(), int(conn.shape[1]), vote.data_ptr(),
                                                       int(kf_bad.shape[0]), kf_bad.data_ptr(), conn_start.data_ptr(), int(conn_list.shape[0]),
                                                       conn_list.data_ptr(), frame_id.data_ptr(), C.byref(par), local_kf.data_ptr(), out.data_ptr()),
                   "snk_lmap_select_batch_dev")

    def gather_dev(self, feat_start, feat_point, pt_flags, pt_last_seen, points, frame_id, local_kf, sel, set_start, set_point, pts_cap, lm_pts,
                   lm_point, n_pts, out):
        """snk_lmap_gather_batch_dev: device tensors of the dtypes above (points: a dict of tensors; sel [n_sets, 5] int32; lm_pts
        [n_sets, pts_cap, 96] uint8 or any tensor of that size; lm_point [n_sets, pts_cap] int32; n_pts [n_sets] int32; out [n_sets, 4]
        int32)."""
        cmap = LmapMap(int(feat_start.shape[0]) - 1, int(pt_flags.shape[0]), int(feat_point.shape[0]), feat_start.data_ptr(), feat_point.data_ptr(),
                       pt_flags.data_ptr(), pt_last_seen.data_ptr())
        cpts = LmapPoints(*(points[k].data_ptr() for k in ("pos", "normal", "desc", "ref_depth", "ref_level")))
        _lib.check(self._lib.snk_lmap_gather_batch_dev(self._h, int(sel.shape[0]), C.byref(cmap), C.byref(cpts), frame_id.data_ptr(), local_kf.data_ptr(),
                                                       int(local_kf.shape[1]), sel.data_ptr(), set_start.data_ptr(), int(set_point.numel()),
                                                       set_point.data_ptr(), int(pts_cap), lm_pts.data_ptr(), lm_point.data_ptr(), n_pts.data_ptr(),
                                                       out.data_ptr()), "snk_lmap_gather_batch_dev")
