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

    def solve_batch(self, problems, first_problem: int = 0):
        """problems: list of dict(points1 [n, 3], points2 [n, 3], ips1 [n, 2], ips2 [n, 2], optional T [7] and scale).  One launch;
        returns one dict per problem: T (qx qy qz qw tx ty tz), scale, inliers, mask [n] uint8, best (the winning hypothesis).  The
        sampler draws problem i of a call from (seed, i); ``first_problem`` = j gives the problems the indices j, j + 1, ... by putting
        j empty problems in front, so that a problem solved on its own repeats what it gave as entry j of a batch."""
        empty = dict(points1=np.zeros((0, 3)), points2=np.zeros((0, 3)), ips1=np.zeros((0, 2)), ips2=np.zeros((0, 2)))
        probs, keep = self._problems([empty] * int(first_problem) + list(problems))
        _lib.check(self._lib.snk_sim3_ransac(self._h, C.byref(self.params), probs, len(keep)), "snk_sim3_ransac")
        return [self._result(P, k) for P, k in zip(probs, keep)][int(first_problem):]

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


# ---- pose-graph optimisation of the loop corrector (snk-pgo v1) ----
class PgoOptions(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("max_pcg_iterations", C.c_int32), ("pcg_tol", C.c_double), ("min_chi2_delta", C.c_double),
                ("lambda_init", C.c_double)]


class PgoResult(C.Structure):
    _fields_ = [("cost_initial", C.c_double), ("cost_final", C.c_double), ("lm_iterations", C.c_int32), ("pcg_iterations_total", C.c_int32),
                ("accepted_steps", C.c_int32), ("pcg_form", C.c_int32), ("workgroups", C.c_int32), ("pcg_iterations_max", C.c_int32)]


def pgo_options(max_iterations: int = 50, max_pcg_iterations: int = 10000, pcg_tol: float = 1e-20, min_chi2_delta: float = 1e-10,
                lambda_init: float = 1e-4) -> PgoOptions:
    """The options of LoopClosingPGO.cpp:125-126 plus the [DEFINED] ones of snk-pgo v1."""
    return PgoOptions(int(max_iterations), int(max_pcg_iterations), float(pcg_tol), float(min_chi2_delta), float(lambda_init))


def corrected_source_sim3(corrected_pose, scale: float = 1.0) -> np.ndarray:
    """The hand-over from the geometric check: ``corrected_pose`` is one row of ``corrected_pose_dev`` of
    snk_sim3_ransac_pairs_batch_dev (tmpPose of LoopDetector.cpp:278, an SE3 world -> camera, qx qy qz qw tx ty tz) and ``scale`` the
    scale that goes with it (1 for stereo / RGB-D, LoopDetector.cpp:361; the entry of ``scale_dev`` otherwise).  Returns
    ``T_w_correctSource`` as ``PoseGraph.set_pose`` takes it: ``T_w_corrected_source.se3() = tmpPose.inverse()`` with that scale
    (:355-361), 8 doubles.  The quaternion is used as it is (no normalisation), like everywhere behind this ABI."""
    c = np.asarray(corrected_pose, np.float64).reshape(7)
    x, y, z, w = c[:4]
    R = np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)],
                  [2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)],
                  [2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]])
    return np.concatenate([[-x, -y, -z, w], -(R.T @ c[4:]), [float(scale)]])


class PoseGraph:
    """The graph ``LoopClosing::ConstructPGO`` builds (LoopClosingPGO.cpp:16-118).  ``poses`` [n, 8] (qx qy qz qw tx ty tz s, T_w_i) are the
    poses the edges are measured at; ``add_vertex_edge`` records T_i_j = T_w_i^-1 T_w_j from them (:105), ``set_pose`` then moves a vertex
    (:114) without touching the edges already added, ``sort_edges`` orders them (:90,99,108)."""

    def __init__(self, poses, constant=None, fix_scale: bool = True):
        self.poses_measure = np.array(poses, np.float64).reshape(-1, 8)
        self.poses = self.poses_measure.copy()
        n = len(self.poses)
        self.constant = np.zeros(n, np.uint8) if constant is None else np.array(constant, np.uint8).reshape(n)
        self.fix_scale = bool(fix_scale)
        self.edges: list[tuple[int, int, float]] = []

    def add_vertex_edge(self, i: int, j: int, weight: float = 1.0):
        i, j = (int(i), int(j)) if i < j else (int(j), int(i))
        self.edges.append((i, j, float(weight)))

    def sort_edges(self):
        """sorted by (i, j); of several edges between the same pair the first one added stays"""
        seen, out = set(), []
        for e in sorted(self.edges, key=lambda e: e[:2]):
            if e[:2] not in seen:
                seen.add(e[:2])
                out.append(e)
        self.edges = out

    def set_pose(self, i: int, sim3):
        self.poses[int(i)] = np.asarray(sim3, np.float64).reshape(8)


class PoseGraphOptimizer:
    """``PGORec`` / ``PGOSim3Rec`` as OptimizeEssentialGraph uses them (LoopClosingPGO.cpp:134-146): create(pg), init_and_solve(), then the
    optimised poses and the map-point pass (:231-260)."""

    def __init__(self, options: PgoOptions | None = None, device: int = 0, stream: int | None = None):
        self._lib = _lib.load()
        self.options = options or pgo_options()
        self._h = C.c_void_p()
        _lib.check(self._lib.snk_pgo_create(C.byref(self.options), int(device), C.c_void_p(stream or 0), C.byref(self._h)), "snk_pgo_create")
        self.n = 0
        self.result = None

    def close(self):
        if self._h:
            self._lib.snk_pgo_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def set_graph(self, poses_measure, constant, edges, weights=None, measurements=None, poses_init=None, fix_scale=True):
        """snk_pgo_set_graph with numpy arrays"""
        pm = np.ascontiguousarray(poses_measure, np.float64).reshape(-1, 8)
        n = len(pm)
        pi = None if poses_init is None else np.ascontiguousarray(poses_init, np.float64).reshape(n, 8)
        cs = np.ascontiguousarray(constant, np.uint8).reshape(n)
        ed = np.ascontiguousarray(edges, np.int32).reshape(-1, 2)
        w = None if weights is None else np.ascontiguousarray(weights, np.float64).reshape(len(ed))
        ms = None if measurements is None else np.ascontiguousarray(measurements, np.float64).reshape(len(ed), 8)
        p = lambda a: None if a is None else a.ctypes.data
        _lib.check(self._lib.snk_pgo_set_graph(self._h, n, p(pm), p(pi), p(cs), len(ed), p(ed), p(w), p(ms), int(bool(fix_scale))), "snk_pgo_set_graph")
        self.n, self.n_edges = n, len(ed)

    def create(self, pg: PoseGraph):
        ed = np.array([e[:2] for e in pg.edges], np.int32).reshape(-1, 2)
        w = np.array([e[2] for e in pg.edges], np.float64)
        self.set_graph(pg.poses_measure, pg.constant, ed, w, None, pg.poses, pg.fix_scale)

    def solve(self) -> dict:
        r = PgoResult()
        _lib.check(self._lib.snk_pgo_solve(self._h, C.byref(r)), "snk_pgo_solve")
        self.result = {k: getattr(r, k) for k, _ in PgoResult._fields_}
        return self.result

    init_and_solve = solve

    def poses(self) -> np.ndarray:
        out = np.zeros((self.n, 8), np.float64)
        _lib.check(self._lib.snk_pgo_get_poses(self._h, out.ctypes.data), "snk_pgo_get_poses")
        return out

    def cost(self) -> float:
        c = C.c_double(0.0)
        _lib.check(self._lib.snk_pgo_cost(self._h, C.byref(c)), "snk_pgo_cost")
        return float(c.value)

    def debug_linearisation(self):
        """(residuals [E, 7], gradient [n, 7], diag [n, 49]) at the current state"""
        r, g, d = np.zeros((self.n_edges, 7)), np.zeros((self.n, 7)), np.zeros((self.n, 49))
        _lib.check(self._lib.snk_pgo_debug_linearisation(self._h, r.ctypes.data, g.ctypes.data, d.ctypes.data), "snk_pgo_debug_linearisation")
        return r, g, d

    def transform_points(self, ref_vertex, positions, normals=None, reference_depth=None):
        """The map-point pass: returns (positions, normals, reference_depth) moved by T_w_i^after (T_w_i^before)^-1 of their reference vertex."""
        ref = np.ascontiguousarray(ref_vertex, np.int32)
        pos = np.array(positions, np.float64).reshape(len(ref), 3)
        nrm = None if normals is None else np.array(normals, np.float64).reshape(len(ref), 3)
        dep = None if reference_depth is None else np.array(reference_depth, np.float64).reshape(len(ref))
        p = lambda a: None if a is None else a.ctypes.data
        _lib.check(self._lib.snk_pgo_transform_points(self._h, len(ref), p(ref), p(pos), p(nrm), p(dep)), "snk_pgo_transform_points")
        return pos, nrm, dep
