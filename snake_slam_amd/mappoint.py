"""Host-side mirror of the map-point refresh over the C ABI.

``MapPointRefresher`` runs ``MapPoint::ComputeDistinctiveDescriptors``, ``UpdateNormal`` and ``UpdateDepth`` (reference
Snake/Map/MapPoint.cpp:60-81, :120-135, :154-166) for many points per call, semantics "snk-mp v1" (DESIGN.md section 3h): the
descriptor is the first valid observation whose row of Hamming distances has the smallest median (or sum), the normal is the
normalised sum of the unit vectors towards the observing cameras in list order, the reference depth is the distance to the reference
keyframe's centre.  The list surgery around it (AddObservation, Replace, SetBadFlag) stays with the caller.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .matcher import _Handle, _as_desc, _ptr
from .tracking import FramesDev

MAX_OBS = 4096
MEDIAN, SUM = 0, 1
DESCRIPTOR, NORMAL, DEPTH = 1, 2, 4
ALL = DESCRIPTOR | NORMAL | DEPTH
OK, BAD_INDEX, TOO_MANY = 0, 1, 2

RESULT_DTYPE = np.dtype([("best", "<i4"), ("n_valid", "<i4"), ("ref_level", "<i4"), ("status", "<i4"), ("normal", "<f8", 3),
                         ("ref_depth", "<f8"), ("desc", "<u8", 4)])


class MpParams(C.Structure):
    _fields_ = [("rule", C.c_int32), ("what", C.c_int32)]


class MapPointRefresher(_Handle):
    """``rule``: MEDIAN (the ORB-SLAM rule, default) or SUM."""

    def __init__(self, rule: int = MEDIAN, device: int = 0, stream: int | None = None):
        super().__init__(device, stream)
        self.rule = int(rule)

    def refresh(self, obs_start, desc, cam_pose, octave, valid, position, ref_obs, what: int = ALL) -> np.ndarray:
        """snk_mappoint_refresh.  Point p owns the observations obs_start[p] .. obs_start[p + 1] - 1 in list order; per observation
        desc [n_obs, 4] uint64 (or [n_obs, 32] uint8), cam_pose [n_obs, 7] (qx qy qz qw tx ty tz), octave [n_obs], valid [n_obs];
        per point position [n, 3] and ref_obs [n] (index into the point's list, -1: no UpdateDepth).  Returns RESULT_DTYPE records."""
        start = np.ascontiguousarray(obs_start, np.int32).reshape(-1)
        n = len(start) - 1
        n_obs = int(start[-1]) if n >= 0 else 0
        d = _as_desc(desc) if n_obs > 0 else np.zeros((0, 4), np.uint64)
        pose = np.ascontiguousarray(cam_pose, np.float64).reshape(-1, 7)
        octv = np.ascontiguousarray(octave, np.int32).reshape(-1)
        val = np.ascontiguousarray(valid, np.uint8).reshape(-1)
        pos = np.ascontiguousarray(position, np.float64).reshape(-1, 3)
        ref = np.ascontiguousarray(ref_obs, np.int32).reshape(-1)
        if n < 0 or len(pos) != n or len(ref) != n or min(len(d), len(pose), len(octv), len(val)) < max(n_obs, 0):
            raise ValueError("array lengths")
        out = np.zeros(max(n, 0), RESULT_DTYPE)
        par = MpParams(self.rule, int(what))
        _lib.check(self._lib.snk_mappoint_refresh(self._h, C.byref(par), n, _ptr(start), _ptr(d), _ptr(pose), _ptr(octv), _ptr(val), _ptr(pos),
                                                  _ptr(ref), _ptr(out)), "snk_mappoint_refresh")
        return out

    # the reference's method names, over the same gathered lists
    def ComputeDistinctiveDescriptors(self, obs_start, desc, valid):
        """(best [n], descriptor [n, 4]) -- best = -1 leaves the point's descriptor as it was (MapPoint.cpp:75)."""
        n_obs, n = len(np.asarray(valid).reshape(-1)), len(np.asarray(obs_start).reshape(-1)) - 1
        r = self.refresh(obs_start, desc, np.zeros((n_obs, 7)), np.zeros(n_obs, np.int32), valid, np.zeros((n, 3)), np.full(n, -1, np.int32),
                         DESCRIPTOR)
        return r["best"], r["desc"]

    def UpdateNormal(self, obs_start, cam_pose, valid, position):
        n_obs = len(np.asarray(valid).reshape(-1))
        n = len(np.asarray(obs_start).reshape(-1)) - 1
        return self.refresh(obs_start, np.zeros((n_obs, 4), np.uint64), cam_pose, np.zeros(n_obs, np.int32), valid, position,
                            np.full(n, -1, np.int32), NORMAL)["normal"]

    def UpdateDepth(self, obs_start, cam_pose, octave, position, ref_obs):
        """(reference_depth [n], reference_scale_level [n])"""
        n_obs = len(np.asarray(octave).reshape(-1))
        r = self.refresh(obs_start, np.zeros((n_obs, 4), np.uint64), cam_pose, octave, np.ones(n_obs, np.uint8), position, ref_obs, DEPTH)
        return r["ref_depth"], r["ref_level"]

    def refresh_batch_dev(self, frames: FramesDev, poses, obs_start, obs, valid, position, ref_obs, out, what: int = ALL):
        """snk_mappoint_refresh_batch_dev: device tensors.  frames: the keyframe slots (n, kps, desc are read), poses [batch, 7]
        float64, obs_start [n + 1] int32, obs [n_obs, 2] int32 (kf_slot, feature), valid [n_obs] uint8, position [n, 3] float64,
        ref_obs [n] int32, out [n, 80] uint8 (RESULT_DTYPE records).  Asynchronous on the handle's stream; a point with an index out
        of range has status BAD_INDEX, one with more than MAX_OBS observations TOO_MANY."""
        par = MpParams(self.rule, int(what))
        _lib.check(self._lib.snk_mappoint_refresh_batch_dev(
            self._h, C.byref(par), C.byref(frames), poses.data_ptr(), int(position.shape[0]), obs_start.data_ptr(), int(obs.shape[0]),
            obs.data_ptr(), valid.data_ptr(), position.data_ptr(), ref_obs.data_ptr(), out.data_ptr()), "snk_mappoint_refresh_batch_dev")
