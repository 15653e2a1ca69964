"""Host-side mirror of the loop detector's geometric check over the C ABI.

``RegistrationRansac`` mirrors the solver member of ``Snake::LoopDetector`` as ``LoopDetector::solve`` uses it (reference
Snake/LoopClosing/LoopDetector.cpp:148-206), semantics "snk-sim3 v1" (DESIGN.md section 3e): a 3-point registration RANSAC between the
view-space map points of two keyframes, scored by the reprojection error in both images.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .matcher import _Handle, _ptr
from .tracking import Camera, FramesDev

MAX_PAIRS = 2048


class Sim3Params(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("compute_scale", C.c_int32), ("threshold", C.c_double), ("seed", C.c_uint64),
                ("probability", C.c_double), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32)]


class Sim3Problem(C.Structure):
    _fields_ = [("n", C.c_int32), ("inliers", C.c_int32), ("points1", C.c_void_p), ("points2", C.c_void_p), ("ips1", C.c_void_p),
                ("ips2", C.c_void_p), ("inlier_mask", C.c_void_p), ("cam", Camera), ("T", C.c_double * 7), ("scale", C.c_double),
                ("best_iteration", C.c_int32), ("pad", C.c_int32)]


def ransac_iterations(n: int, probability: float = 0.999, min_inliers: int = 15, max_iterations: int = 100) -> int:
    """``RansacIterationsFromProbability(N, 0.999, 15, 100)`` of LoopDetector.cpp:203 (snk_ransac_iterations)."""
    return int(_lib.load().snk_ransac_iterations(int(n), float(probability), int(min_inliers), int(max_iterations)))


class RegistrationRansac(_Handle):
    """The solver of LoopDetector.cpp:152-205.  ``threshold`` is in squared pixels (12 at :156); ``iterations`` > 0 forces the
    count, 0 uses ``ransac_iterations(n, probability, min_inliers, max_iterations)`` per problem (:203); ``compute_scale`` is true
    for mono input only (:231); ``seed`` feeds the counter-based sampler."""

    ransac_iterations = staticmethod(ransac_iterations)

    def __init__(self, cam, threshold: float = 12.0, iterations: int = 0, compute_scale: bool = False, seed: int = 0,
                 probability: float = 0.999, min_inliers: int = 15, max_iterations: int = 100, device: int = 0, stream: int | None = None):
        super().__init__(device, stream)
        self.cam = tuple(float(v) for v in cam)[:4]
        self.params = Sim3Params(int(iterations), int(bool(compute_scale)), float(threshold), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                 float(probability), int(min_inliers), int(max_iterations))

    def _problems(self, problems):
        probs = (Sim3Problem * max(len(problems), 1))()
        keep = []
        for P, f in zip(probs, problems):
            a = [np.ascontiguousarray(f[k], np.float64).reshape(-1, w) for k, w in (("points1", 3), ("points2", 3), ("ips1", 2), ("ips2", 2))]
            if len({len(x) for x in a}) != 1:
                raise ValueError("points1 / points2 / ips1 / ips2 length mismatch")
            mask = np.zeros(max(len(a[0]), 1), np.uint8)
            keep.append((a, mask))
            P.n = len(a[0])
            P.points1, P.points2, P.ips1, P.ips2 = ((x.ctypes.data if x.size else 0) for x in a)
            P.inlier_mask = mask.ctypes.data
            P.cam = Camera(*self.cam, 0.0)
            T = f.get("T")
            P.T[:] = [float(v) for v in (T if T is not None else (0, 0, 0, 1, 0, 0, 0))]
            P.scale = float(f.get("scale", 1.0))
        return probs, keep

    @staticmethod
    def _result(P, k):
        return dict(T=np.array(P.T[:]), scale=float(P.scale), inliers=int(P.inliers), mask=k[1][: P.n].copy(), best=int(P.best_iteration))

    def solve_batch(self, problems):
        """problems: list of dict(points1 [n, 3], points2 [n, 3], ips1 [n, 2], ips2 [n, 2], optional T [7] and scale).  One launch;
        returns one dict per problem: T (qx qy qz qw tx ty tz), scale, inliers, mask [n] uint8, best (the winning hypothesis)."""
        probs, keep = self._problems(problems)
        _lib.check(self._lib.snk_sim3_ransac(self._h, C.byref(self.params), probs, len(problems)), "snk_sim3_ransac")
        return [self._result(P, k) for P, k in zip(probs, keep)]

    def solve(self, points1, points2, ips1, ips2):
        """``auto [T, scale, nInliers] = solver.solve(its, compute_scale)``: returns (T, scale, inliers, vbInliers)."""
        r = self.solve_batch([dict(points1=points1, points2=points2, ips1=ips1, ips2=ips2)])[0]
        return r["T"], r["scale"], r["inliers"], r["mask"]

    def debug_hypotheses(self, points1, points2, ips1, ips2, T=None, scale=1.0):
        """snk_sim3_debug_hypotheses: (result dict as solve_batch, triplets [K, 3], valid [K], T [K, 7], scale [K], counts [K])."""
        probs, keep = self._problems([dict(points1=points1, points2=points2, ips1=ips1, ips2=ips2, T=T, scale=scale)])
        p = self.params
        K = int(p.iterations) if p.iterations > 0 else ransac_iterations(probs[0].n, p.probability, p.min_inliers, p.max_iterations)
        tri, valid, cnt = np.zeros((K, 3), np.int32), np.zeros(K, np.int32), np.zeros(K, np.int32)
        Ts, sc = np.zeros((K, 7), np.float64), np.zeros(K, np.float64)
        _lib.check(self._lib.snk_sim3_debug_hypotheses(self._h, C.byref(p), probs, _ptr(tri), _ptr(valid), _ptr(Ts), _ptr(sc), _ptr(cnt)),
                   "snk_sim3_debug_hypotheses")
        return self._result(probs[0], keep[0]), tri, valid, Ts, sc, cnt

    def solve_pairs_batch_dev(self, frames1: FramesDev, frames2: FramesDev, pairs, n_pairs, pts1, pts2, frame_pt1, frame_pt2, n_pts1,
                              n_pts2, poses1, poses2, T, scale, inliers, match12, corrected_pose):
        """Device-resident form behind snk_bf_knn2_batch_dev / snk_bf_filter_batch_dev (keyframe 1 = query set): pairs [B, cap, 2]
        int32 and n_pairs [B] int32 as the filter leaves them, pts1 / pts2 [B, m_cap, stride] uint8 point tables, frame_pt1 / frame_pt2
        [B, cap] int32 (-1 = no point), n_pts1 / n_pts2 [B] int32, poses1 / poses2 [B, 7] float64 in; T [B, 7], scale [B] float64,
        inliers [B] int32, match12 [B, frames1.cap] int32, corrected_pose [B, 7] float64 out.  Asynchronous on the handle's stream."""
        c = Camera(*self.cam, 0.0)
        _lib.check(self._lib.snk_sim3_ransac_pairs_batch_dev(
            self._h, C.byref(frames1), C.byref(frames2), C.byref(c), C.byref(self.params), pairs.data_ptr(), n_pairs.data_ptr(),
            int(pairs.shape[1]), pts1.data_ptr(), pts2.data_ptr(), int(pts1.shape[2]), frame_pt1.data_ptr(), frame_pt2.data_ptr(),
            n_pts1.data_ptr(), n_pts2.data_ptr(), int(pts1.shape[1]), poses1.data_ptr(), poses2.data_ptr(), T.data_ptr(), scale.data_ptr(),
            inliers.data_ptr(), match12.data_ptr(), corrected_pose.data_ptr()), "snk_sim3_ransac_pairs_batch_dev")
