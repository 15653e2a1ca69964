"""One table of back-end "seams" for the tests that run the library the way an integrator does -- on dirty scratch, on one shared handle,
beside other threads, on a caller's stream (tests/test_backend_scratch_gpu.py, tests/test_backend_handles_gpu.py,
tests/test_zz_backend_threads_gpu.py; the CPU side is tests/test_backend_cases.py).

A seam is (name, make(device, stream) -> handles, run(handles, k) -> bytes): `run` makes the module's calls on case k % 3 and returns every
output concatenated as bytes.  The cases come from the makers the parity suites already use, at small sizes; each parity suite pins its
module to the numpy restatement, so a seam's result on a fresh handle of its own ("solo") is the ground truth of everything here and is
compared byte for byte: the kernels are deterministic.

`handles` is a dict: "objs" (everything with close(), in closing order), "matchers" (the wrappers that own a snk_matcher: what share_handle
points at one handle), "st" (the torch stream every call of the seam is enqueued on) and whatever the seam keeps between calls."""
import contextlib
import functools

import numpy as np

import bow_numpy as BW
import covis_numpy as CV
import localmap_numpy as LM
import mappoint_numpy as MP
import p3p_numpy as P3
import pgo_numpy as PG
import scene_numpy as SN
import sim3_numpy as S3
import tri_numpy as TR
from helpers import SEED, make_stereo_case, rand_desc

COVIS_CAP = 16
MAPPOINT_KS = list(range(0, 35)) + [5] * 70 + [64, 100]  # every k around the packed form's last (32), a run across chunks, two wide points


def i32(*v):
    return np.asarray(v, np.int32).tobytes()


def cat(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


# ------------------------------------------------------------------------------------------------------------------------------------
# cases (host side, cached: a reference is computed once and shared)
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def p3p_cases():
    """case k: three problems of n = 30 / 200 / 1000 pairs (one outlier share each, 1 px noise)"""
    by_n = {n: [c for c in P3.gpu_cases() if len(c["wps"]) == n and c["noise_px"] == 1.0] for n in (30, 200, 1000)}
    return [by_n[n] for n in (30, 200, 1000)]


@functools.lru_cache(maxsize=None)
def p3p_odd_batch(k):
    """5, 0 and 33 pairs in one call (tests/test_p3p_gpu.py): the parts of the staged blocks end off a 16-byte boundary"""
    from test_p3p_gpu import odd_batch

    return odd_batch(4400 + 10 * k)


@functools.lru_cache(maxsize=None)
def p3p_frames(k):
    from test_p3p_chain_gpu import make_frames

    return make_frames(3, 320, 100 + k)


@functools.lru_cache(maxsize=None)
def sim3_cases():
    """three of sim3_numpy.gpu_cases(): n = 64, 65 and 200 with 30 % wrong pairs and 1 px noise"""
    cs = S3.gpu_cases()
    return [next(c for c in cs if len(c["P1"]) == n and c["outlier_share"] == 0.3 and c["noise_px"] == 1.0) for n in (64, 65, 200)]


@functools.lru_cache(maxsize=None)
def sim3_odd_batch(k):
    """3, 0 and 65 pairs in one call (tests/test_sim3_gpu.py)"""
    from test_sim3_gpu import odd_batch

    return odd_batch(4500 + 10 * k)


@functools.lru_cache(maxsize=None)
def sim3_keyframes():
    from test_sim3_chain_gpu import make_keyframes

    return make_keyframes(2026)


@functools.lru_cache(maxsize=None)
def tri_case(k):
    return TR.make_case(*(TR.CASES[0], TR.CASES[3], TR.CASES[5])[k])  # (11, 5, "mixed"), (14, 5, "mono"), (16, 5, "stereo")


@functools.lru_cache(maxsize=None)
def mappoint_case(k):
    return MP.make_case(80 + k, MAPPOINT_KS, bool(k % 2), invalid_frac=0.1)


@functools.lru_cache(maxsize=None)
def mappoint_frames(k):
    """The frames-on-device setup of tests/test_mappoint_gpu.py (3 keyframe slots, cap 128, n = 128 / 77 / 100) without its broken
    points, and the gathered copy for the host form / the restatement."""
    from snake_slam_amd.matcher import KP64_DTYPE

    rng = np.random.default_rng(91 + k)
    B, CAP = 3, 128
    n = np.array([128, 77, 100], np.int32)
    desc = MP.descriptors(rng, B * CAP, True).reshape(B, CAP, 4)
    kps = np.zeros((B, CAP), KP64_DTYPE)
    kps["octave"] = rng.integers(0, 8, (B, CAP))
    poses = MP.random_pose(rng, B)
    ks = [3, 0, 8, 33, 5, 1, 32, 70, 12, 2, 6, 40, 9] + [5] * 70 + [4, 31, 100]
    start = np.concatenate([[0], np.cumsum(ks)]).astype(np.int32)
    slot = rng.integers(0, B, start[-1]).astype(np.int32)
    obs = np.stack([slot, (rng.random(start[-1]) * n[slot]).astype(np.int32)], 1)
    valid = (rng.random(start[-1]) >= 0.1).astype(np.uint8)
    ref = np.array([int(rng.integers(-1, kk)) if kk else -1 for kk in ks], np.int32)
    position = rng.uniform(-3, 3, (len(ks), 3))
    host = dict(obs_start=start, desc=desc[obs[:, 0], obs[:, 1]], pose=poses[obs[:, 0]], octave=kps["octave"][obs[:, 0], obs[:, 1]].astype(np.int32),
                valid=valid, position=position, ref_obs=ref)
    return dict(B=B, CAP=CAP, n=n, desc=desc, kps=kps, poses=poses, start=start, obs=obs, valid=valid, ref=ref, position=position, host=host)


@functools.lru_cache(maxsize=None)
def covis_case(k):
    m = CV.make_map(31 + k, 300, 6000)
    set_start, set_point = CV.frames_of(m, 41 + k, 12)
    q = np.random.default_rng(51 + k).permutation(300)[:40].astype(np.int32)
    return dict(m=m, q=q, set_start=np.asarray(set_start, np.int32), set_point=np.asarray(set_point, np.int32))


# the local map at kf_cap 4 / pts_cap 64: three votes of localmap_numpy.select_case and three sets of gather_case(64) with at most four
# local keyframes per case (the two halves of edge_case have maps of their own: gather does not read what select wrote)
LMAP_PARAMS = dict(n_direct=2, n_direct_prob=1, n_indirect_prob=1, n_neighbours=2, kf_cap=4, seed=0)
LMAP_PTS_CAP = 64
LMAP_SELECT_SETS = ((1, 4, 8), (2, 5, 9), (3, 7, 11))  # case 0 ends on a KF_OVERFLOW, case 2 on the truncated vote
LMAP_GATHER_SETS = (("mixed_seen", "cap", "collisions"), ("mixed", "cap+1", "chunk257"), ("shared_reversed", "cap_by_own", "empty_status"))


def _lmap_gather_sets(g, sets):
    """the sets `sets` of a localmap_numpy.gather_case as a case of their own, local_kf cut to kf_cap columns"""
    cap = LMAP_PARAMS["kf_cap"]
    assert np.all(g["local_kf"][sets][:, cap:] == -1)
    own = [g["set_point"][g["set_start"][s]:g["set_start"][s + 1]] for s in sets]
    return dict(m=g["m"], frame_id=g["frame_id"][sets], local_kf=np.ascontiguousarray(g["local_kf"][sets][:, :cap]), sel=g["sel"][sets],
                set_start=LM.csr(own), set_point=np.concatenate(own).astype(np.int32))


@functools.lru_cache(maxsize=None)
def lmap_case(k):
    e = LM.edge_case(LMAP_PTS_CAP)
    s, g = e["select"], e["gather"]
    rows = list(LMAP_SELECT_SETS[k])
    select = dict(s, conn=s["conn"][rows], vote=s["vote"][rows], frame_id=s["frame_id"][rows])
    return dict(select=select, gather=_lmap_gather_sets(g, [g["what"][n] for n in LMAP_GATHER_SETS[k]]))


# local BA windows at win_cap 4 / pt_cap 64 / obs_cap 256: scene_numpy.build_map with 16 features a keyframe, three of its QUERIES per case
SCENE_PARAMS = dict(n_neighbours=2, n_last=1, win_cap=4, gyro_weight=2.0, acc_weight=0.5)
SCENE_CAPS = dict(win_cap=4, pt_cap=64, img_cap=16, obs_cap=256)


@functools.lru_cache(maxsize=None)
def scene_map():
    return SN.build_map(feats=16)


def scene_queries(k):
    return SN.QUERIES[k::3]  # (100, 5, 7), (45, 50, 110), (41, 60, 20): 50 is a bad query


BOW_FRAME_COUNTS = (257, 65, 1000)
BOW_MATCH_NAMES = ("scene_k10_L3_300", "list_70", "scene_irregular_257")


@functools.lru_cache(maxsize=None)
def bow_match_cases():
    cs = {c[0]: c for c in BW.match_cases()}
    return [cs[n] for n in BOW_MATCH_NAMES]


@functools.lru_cache(maxsize=None)
def pgo_graph(k, fix):
    return PG.prepare((lambda f: PG.ring(40, 3, 3, f), lambda f: PG.hub(70, 4, f), lambda f: PG.correct_loop(8, 2, f))[k](fix))


@functools.lru_cache(maxsize=None)
def front_cases():
    """the front-end seams' inputs as tests/test_zz_threads_gpu.py draws them"""
    import track_helpers as T
    from oracle import oracle as orc

    orc.build()
    rng = np.random.default_rng(SEED + 4242)
    stereo = [make_stereo_case(rng, 300, 280) for _ in range(3)]
    bf_sets = [(rand_desc(rng, 257), rand_desc(rng, 301)) for _ in range(3)]
    track, fine = [], []
    for i in range(3):
        frame, cam, pose, ls, world, _ = T.make_tracking_case(orc, rng, n_clutter=300, m_pts=250)
        skip = (rng.random(len(world["pos"])) < 0.1).astype(np.uint8)
        track.append((frame, cam, pose, ls, T.lm_coarse(orc, world), (world["pos"], world["desc"], skip)))
        # the fine matcher's 251 records: the 250 points and the first once more (both want the same feature); a generator of their own,
        # so that the cases above stay what they were
        f = T.lm_fine(orc, np.random.default_rng(SEED + 4343 + i), world, pose, ls)
        fine.append(np.concatenate([f, f[:1]]))
    # 301 raw keypoints for rectify: a snk_keypoint has 24 bytes, so the array ends off a 16-byte boundary
    from test_oracle_preprocess import make_kps

    rect = [make_kps(orc, 301, 700 + i) for i in range(3)]
    return dict(stereo=stereo, bf=bf_sets, track=track, fine=fine, rect=rect)


@functools.lru_cache(maxsize=None)
def pose_case(k):
    import pose_helpers as PH

    return PH.make_problem(77 + k, 300, outlier_frac=0.2)


@functools.lru_cache(maxsize=None)
def pose_odd_batch(k):
    """1, 0, 37 and 299 matches in one call (tests/test_pose_gpu.py): 337 in all, an odd total, one problem empty"""
    import pose_helpers as PH

    return [PH.make_problem(150 + 10 * k + i, n, outlier_frac=0.2) for i, n in enumerate((1, 0, 37, 299))]


# ------------------------------------------------------------------------------------------------------------------------------------
# plumbing
# ------------------------------------------------------------------------------------------------------------------------------------
def _stream(device, stream):
    import torch

    return stream if stream is not None else torch.cuda.Stream(device=device)


@contextlib.contextmanager
def on(H):
    """torch's current device and stream = the seam's: uploads, resets and read-backs are ordered with the library's calls"""
    import torch

    with torch.cuda.device(H["device"]), torch.cuda.stream(H["st"]):
        yield


def _base(device, stream, objs, matchers=None, **more):
    return dict(device=device, st=stream, objs=list(objs), matchers=list(objs if matchers is None else matchers), **more)


def _up(H, a):
    """upload on the seam's stream (call under on(H))"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", H["device"]))


def close_handles(H):
    for o in H["objs"]:
        o.close()


def share_handle(owner, adopters):
    """Point several wrapper objects at ONE snk_matcher: each adopter's own handle is destroyed and its _h becomes the owner's.  Only the
    owner closes it -- call release_adopters first."""
    for a in adopters:
        if a is owner:
            continue
        a.close()
        a._h = owner._h


def release_adopters(owner, adopters):
    for a in adopters:
        if a is not owner:
            a._h = None


# ------------------------------------------------------------------------------------------------------------------------------------
# seams
# ------------------------------------------------------------------------------------------------------------------------------------
def make_p3p(device=0, stream=None):
    from snake_slam_amd.tracking import P3PRansac

    st = _stream(device, stream)
    s = P3PRansac(250, P3.THRESHOLD, 0x1234567800000000, device, st.cuda_stream)
    return _base(device, st, [s], dev={})


def _p3p_dev(H, k):
    import torch

    if k not in H["dev"]:
        F = p3p_frames(k)
        B, cap = F["B"], F["cap"]
        dv = torch.device("cuda", H["device"])
        D = dict(n=_up(H, F["n_feat"]), kps=_up(H, F["kps"].view(np.uint8).reshape(B, cap, 24)), desc=torch.zeros((B, cap, 4), dtype=torch.int64, device=dv),
                 rp=torch.full((B, cap), -1.0, dtype=torch.float32, device=dv), taken=torch.zeros((B, cap), dtype=torch.uint8, device=dv),
                 cell_start=torch.zeros((B, 38 * 24 + 1), dtype=torch.int32, device=dv), pts=_up(H, F["world"].reshape(B, cap, 3).view(np.uint8).reshape(B, cap, 24)),
                 n_pts=_up(H, F["n_pts"]), frame_pt0=_up(H, F["frame_pt"]), frame_pt=_up(H, F["frame_pt"]),
                 poses0=_up(H, np.tile([0.0, 0.0, 0.0, 1.0, 0.5, -0.25, 0.125], (B, 1))), poses=torch.zeros((B, 7), dtype=torch.float64, device=dv),
                 inl=torch.zeros(B, dtype=torch.int32, device=dv))
        H["dev"][k] = D
    return H["dev"][k]


P3P_CAM = (P3.FX, P3.FY, P3.CX, P3.CY, 47.9)


def p3p_dev_call(H, k):
    """the device entry alone on the seam's stream; returns the output tensors (no synchronisation)"""
    from test_p3p_chain_gpu import frames_view

    D = _p3p_dev(H, k)
    D["frame_pt"].copy_(D["frame_pt0"])
    D["poses"].copy_(D["poses0"])
    D["inl"].fill_(-7)
    H["objs"][0].solve_frame_batch_dev(frames_view(D), P3P_CAM, D["pts"], D["frame_pt"], D["n_pts"], D["poses"], D["inl"])
    return D["frame_pt"], D["poses"], D["inl"]


def run_p3p(H, k):
    k %= 3
    s = H["objs"][0]
    res = s.solve_batch([dict(wps=c["wps"], nips=c["nips"]) for c in p3p_cases()[k]])
    start = [0.0, 0.0, 0.0, 1.0, 1.0, 2.0, 3.0]
    odd = s.solve_batch([dict(wps=c["wps"], nips=c["nips"], pose=start) for c in p3p_odd_batch(k)])
    assert odd[1]["inliers"] == 0 and odd[1]["best"] == (-1, -1) and np.array_equal(odd[1]["pose"], start)  # n = 0: the pose as it came in
    out = b"".join(cat(r["pose"], r["mask"], r["matches"]) + i32(r["inliers"], *r["best"]) for r in res + odd)
    with on(H):
        got = p3p_dev_call(H, k)
        out += cat(*(t.cpu().numpy() for t in got))
    return out


def make_sim3(device=0, stream=None):
    import torch

    from snake_slam_amd.loop import RegistrationRansac
    from snake_slam_amd.matcher import BruteForceMatcher
    from snake_slam_amd.tracking import frames_dev

    st = _stream(device, stream)
    rs = RegistrationRansac(S3.CAM, S3.THRESHOLD, 0, False, 0x5EED0000ABCD, device=device, stream=st.cuda_stream)
    H = _base(device, st, [rs])
    K = sim3_keyframes()
    B, CAP = K["desc1"].shape[:2]
    with on(H):
        dv = torch.device("cuda", device)
        D = {key: _up(H, K[key]) for key in ("n1", "n2", "n_pts1", "n_pts2", "frame_pt1", "frame_pt2", "poses1", "poses2")}
        D["desc1"], D["desc2"] = _up(H, K["desc1"].view(np.int64)), _up(H, K["desc2"].view(np.int64))
        D["pts1"], D["pts2"] = _up(H, K["wp1"].view(np.uint8).reshape(B, CAP, 24)), _up(H, K["wp2"].view(np.uint8).reshape(B, CAP, 24))
        D["kps1"], D["kps2"] = _up(H, K["kps1"].view(np.uint8).reshape(B, CAP, 24)), _up(H, K["kps2"].view(np.uint8).reshape(B, CAP, 24))
        z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt, device=dv)  # noqa: E731
        D["aux"] = (z(B, CAP, dt=torch.float32), z(B, CAP, dt=torch.uint8), z(B, 2))
        D["fd"] = [frames_dev((0.0, 0.0, 752.0, 480.0), D["n" + s], D["kps" + s], D["desc" + s], *D["aux"]) for s in "12"]
        knn, D["pairs"], D["n_pairs"] = z(B, CAP, 4), z(B, CAP, 2), z(B)
        # the pairs come from the matcher once, on a handle of its own: LoopORBmatcher::MatchBruteforce(source, target, ..., 120, 0.9)
        bf = BruteForceMatcher(device, st.cuda_stream)
        try:
            bf.knn2_batch_dev(D["desc1"], D["n1"], D["desc2"], D["n2"], knn)
            bf.filter_batch_dev(knn, D["n1"], 120, 0.9, D["pairs"], D["n_pairs"])
            st.synchronize()
        finally:
            bf.close()
        D["T0"] = _up(H, np.tile([0.0, 0.0, 0.0, 1.0, 0.5, -0.25, 0.125], (B, 1)))
        D["out"] = dict(T=z(B, 7, dt=torch.float64), scale=z(B, dt=torch.float64), cpose=z(B, 7, dt=torch.float64), inl=z(B), match12=z(B, CAP))
    H["D"] = D
    return H


def sim3_dev_call(H, k, compute_scale, max_iterations):
    """snk_sim3_ransac_pairs_batch_dev with iterations = 0 (the count comes from the handle's iteration table); returns the outputs"""
    rs, D = H["objs"][0], H["D"]
    p, o = rs.params, D["out"]
    p.iterations, p.compute_scale, p.max_iterations, p.seed = 0, int(compute_scale), int(max_iterations), 0x5EED0000ABCD + k
    o["T"].copy_(D["T0"])
    o["scale"].fill_(0.75)
    o["cpose"].copy_(D["T0"])
    o["inl"].fill_(-7)
    o["match12"].fill_(-7)
    rs.solve_pairs_batch_dev(D["fd"][0], D["fd"][1], D["pairs"], D["n_pairs"], D["pts1"], D["pts2"], D["frame_pt1"], D["frame_pt2"], D["n_pts1"],
                             D["n_pts2"], D["poses1"], D["poses2"], o["T"], o["scale"], o["inl"], o["match12"], o["cpose"])
    return [o[key] for key in ("T", "scale", "inl", "match12", "cpose")]


def run_sim3(H, k):
    k %= 3
    rs = H["objs"][0]
    c = sim3_cases()[k]
    out = b""
    for cs in (False, True):
        p = rs.params
        p.iterations, p.compute_scale, p.max_iterations, p.seed = int(c["iterations"]), int(cs), 100, int(c["seed"])
        r = rs.solve_batch([dict(points1=c["P1"], points2=c["P2"], ips1=c["ip1"], ips2=c["ip2"])])[0]
        out += cat(r["T"], r["mask"]) + np.float64(r["scale"]).tobytes() + i32(r["inliers"], r["best"])
        with on(H):
            # 100 then 60 + k: the iteration table is refilled when a parameter it depends on changes
            for max_it in (100, 60 + k):
                out += cat(*(t.cpu().numpy() for t in sim3_dev_call(H, k, cs, max_it)))
    p, T0, s0 = rs.params, [0.0, 0.0, 0.0, 1.0, 1.0, 2.0, 3.0], 0.5
    p.iterations, p.compute_scale, p.max_iterations, p.seed = 100, 1, 100, 0x5EED0000ABCD + k
    odd = rs.solve_batch([dict(points1=c["P1"], points2=c["P2"], ips1=c["ip1"], ips2=c["ip2"], T=T0, scale=s0) for c in sim3_odd_batch(k)])
    assert odd[1]["inliers"] == 0 and odd[1]["best"] == -1 and np.array_equal(odd[1]["T"], T0) and odd[1]["scale"] == s0  # n = 0: as it came in
    return out + b"".join(cat(r["T"], r["mask"]) + np.float64(r["scale"]).tobytes() + i32(r["inliers"], r["best"]) for r in odd)


def make_tri(device=0, stream=None):
    from snake_slam_amd.tracking import Triangulator

    st = _stream(device, stream)
    objs = []
    for k in range(3):
        c = tri_case(k)
        p = c["params"]
        objs.append(Triangulator(c["cam"], c["level_scale"], p["error_mono"], p["error_stereo"], p["th_depth"], mono=bool(p["mono"]), device=device,
                                 stream=st.cuda_stream))
    return _base(device, st, objs)


def run_tri(H, k):
    k %= 3
    c = tri_case(k)
    nnew, pts, out_start = H["objs"][k].Process(c["kf1"], c["kf2s"], c["pairs"], c["median_depth2s"])
    return i32(nnew) + cat(pts, out_start)


MP_ARGS = ("obs_start", "desc", "pose", "octave", "valid", "position", "ref_obs")


def make_mappoint(device=0, stream=None):
    from snake_slam_amd.mappoint import MapPointRefresher

    st = _stream(device, stream)
    return _base(device, st, [MapPointRefresher(MP.MEDIAN, device, st.cuda_stream)], dev={})


def _mappoint_dev(H, k):
    import torch

    from snake_slam_amd.tracking import frames_dev

    if k not in H["dev"]:
        F = mappoint_frames(k)
        B, CAP = F["B"], F["CAP"]
        dv = torch.device("cuda", H["device"])
        d = dict(n=_up(H, F["n"]), kps=_up(H, F["kps"].view(np.uint8).reshape(B, CAP, 24)), desc=_up(H, F["desc"].view(np.int64)), poses=_up(H, F["poses"]),
                 start=_up(H, F["start"]), obs=_up(H, F["obs"]), valid=_up(H, F["valid"]), position=_up(H, F["position"]), ref=_up(H, F["ref"]),
                 aux=(torch.zeros((B, CAP), dtype=torch.float32, device=dv), torch.zeros((B, CAP), dtype=torch.uint8, device=dv),
                      torch.zeros((B, 2), dtype=torch.int32, device=dv)), out=torch.zeros((len(F["ref"]), 80), dtype=torch.uint8, device=dv))
        d["fd"] = frames_dev((0.0, 0.0, 752.0, 480.0), d["n"], d["kps"], d["desc"], *d["aux"])
        H["dev"][k] = d
    return H["dev"][k]


def mappoint_dev_call(H, k, rule):
    r, d = H["objs"][0], _mappoint_dev(H, k)
    r.rule = rule
    d["out"].fill_(0xEE)
    r.refresh_batch_dev(d["fd"], d["poses"], d["start"], d["obs"], d["valid"], d["position"], d["ref"], d["out"])
    return [d["out"]]


def run_mappoint(H, k):
    k %= 3
    r, c = H["objs"][0], mappoint_case(k)
    out = b""
    for rule in (MP.MEDIAN, MP.SUM):
        r.rule = rule
        out += r.refresh(*(c[a] for a in MP_ARGS)).tobytes()
        with on(H):
            out += cat(mappoint_dev_call(H, k, rule)[0].cpu().numpy())
    return out


def make_covis(device=0, stream=None):
    from snake_slam_amd.covis import CovisibilityGraph

    st = _stream(device, stream)
    return _base(device, st, [CovisibilityGraph(CV.TH, CV.TH_DEPTH, COVIS_CAP, device, st.cuda_stream)], dev={})


def _covis_dev(H, k):
    import torch

    if k not in H["dev"]:
        c = covis_case(k)
        dv = torch.device("cuda", H["device"])
        nq, ns = len(c["q"]), len(c["set_start"]) - 1
        H["dev"][k] = dict(map=[_up(H, c["m"][a]) for a in CV.MAP_KEYS], feat=[_up(H, c["m"][a]) for a in CV.FEAT_KEYS], q=_up(H, c["q"]),
                           set_start=_up(H, c["set_start"]), set_point=_up(H, c["set_point"]),
                           u_conn=torch.zeros((nq, COVIS_CAP, 2), dtype=torch.int32, device=dv), u_out=torch.zeros((nq, 4), dtype=torch.int32, device=dv),
                           v_conn=torch.zeros((ns, COVIS_CAP, 2), dtype=torch.int32, device=dv), v_out=torch.zeros((ns, 4), dtype=torch.int32, device=dv))
    return H["dev"][k]


def covis_dev_call(H, k, which):
    g, d = H["objs"][0], _covis_dev(H, k)
    conn, out = d[which[0] + "_conn"], d[which[0] + "_out"]
    conn.fill_(-1)
    out.fill_(-7)
    if which == "update":
        g.update_dev(*d["map"], *d["feat"], d["q"], conn, out)
    else:
        g.vote_dev(*d["map"], d["set_start"], d["set_point"], conn, out)
    return [conn, out]


def run_covis(H, k):
    k %= 3
    g, c = H["objs"][0], covis_case(k)
    m = c["m"]
    out = cat(*g.update(*(m[a] for a in CV.MAP_KEYS + CV.FEAT_KEYS), c["q"]))
    out += cat(*g.vote(*(m[a] for a in CV.MAP_KEYS), c["set_start"], c["set_point"]))
    with on(H):
        for which in ("update", "vote"):
            out += cat(*(t.cpu().numpy() for t in covis_dev_call(H, k, which)))
    return out


def make_lmap(device=0, stream=None):
    from snake_slam_amd.localmap import LocalMapBuilder

    st = _stream(device, stream)
    return _base(device, st, [LocalMapBuilder(LMAP_PARAMS, device, st.cuda_stream)])


def lmap_gather_bytes(b, g, pts_cap=LMAP_PTS_CAP):
    m = g["m"]
    return cat(*b.gather(*(m[a] for a in LM.GATHER_KEYS), m, g["frame_id"], g["local_kf"], g["sel"], g["set_start"], g["set_point"], pts_cap))


def run_lmap(H, k):
    """select, then gather"""
    b, c = H["objs"][0], lmap_case(k % 3)
    return cat(*b.select(*(c["select"][a] for a in LM.SELECT_KEYS))) + lmap_gather_bytes(b, c["gather"])


def make_scene(device=0, stream=None):
    from snake_slam_amd.scene import LocalSceneBuilder

    st = _stream(device, stream)
    return _base(device, st, [LocalSceneBuilder(SCENE_PARAMS, device, st.cuda_stream)])


def scene_bytes(b, t, queries):
    """window, then gather into zeroed rows (pt_id: -1)"""
    from snake_slam_amd import scene as S

    win, res = b.window(queries, t["kf_bad"], t["kf_prev"], t["conn_start"], t["conn_list"])
    o = b.gather(t, win, res, SCENE_CAPS["pt_cap"], SCENE_CAPS["img_cap"], SCENE_CAPS["obs_cap"], out=S.host_outputs(len(queries), **SCENE_CAPS))
    return cat(win, res, *(o[row[0]] for row in S.OUT_ROWS), o["result"])


def run_scene(H, k):
    return scene_bytes(H["objs"][0], scene_map(), scene_queries(k % 3))


BOW_CAP = 1024  # the device batch's feature capacity: above every count of BOW_FRAME_COUNTS
BOW_QCAP, BOW_Q = 64, 4


def make_bow(device=0, stream=None):
    import torch

    from snake_slam_amd.bow import KeyframeDatabase, LoopMatcher, Vocabulary

    st = _stream(device, stream)
    v_irr = Vocabulary.from_arrays(BW.vocab("irregular").arrays(), device, st.cuda_stream)
    v_db = Vocabulary.from_arrays(BW.vocab(BW.DB_VOCAB).arrays(), device, st.cuda_stream)
    db = KeyframeDatabase(v_db, max_keyframes=70, max_words=64)
    lm = LoopMatcher(device, st.cuda_stream)
    H = _base(device, st, [lm, db, v_db, v_irr], matchers=[lm], v_irr=v_irr, v_db=v_db, db=db, lm=lm, dev={})
    with torch.cuda.device(device):
        rows = BW.db_rows(65)
        for kf in sorted(rows):
            db.add(kf, *rows[kf])
    return H


def _bow_dev(H, k):
    import torch

    from snake_slam_amd.bow import desc_frames_dev

    if k not in H["dev"]:
        dv = torch.device("cuda", H["device"])
        # transform: the three frames as one batch, frame k first; what lies behind a frame's n must not matter
        counts = [BOW_FRAME_COUNTS[(k + i) % 3] for i in range(3)]
        desc = np.random.default_rng(1 + k).integers(0, 2 ** 64, (3, BOW_CAP, 4), dtype=np.uint64)
        for b, n in enumerate(counts):
            desc[b, :n] = BW.frame_descriptors("irregular", n)
        d = dict(desc=_up(H, desc.view(np.int64)), n=_up(H, np.asarray(counts, np.int32)))
        d["frames"] = desc_frames_dev(d["n"], d["desc"])
        i32t = dict(dtype=torch.int32, device=dv)
        d["t_out"] = dict(words=torch.zeros((3, BOW_CAP), **i32t), values=torch.zeros((3, BOW_CAP), dtype=torch.float64, device=dv),
                          n_words=torch.zeros(3, **i32t), node_id=torch.zeros((3, BOW_CAP), **i32t), node_start=torch.zeros((3, BOW_CAP + 1), **i32t),
                          features=torch.zeros((3, BOW_CAP), **i32t), n_nodes=torch.zeros(3, **i32t), word_of_feature=torch.zeros((3, BOW_CAP), **i32t),
                          node_of_feature=torch.zeros((3, BOW_CAP), **i32t))
        # queries: fresh views of four stored places
        qs = [BW.db_fresh_query(65, (k + 16 * i) % 65) for i in range(BOW_Q)]
        words, values = np.full((BOW_Q, BOW_QCAP), -5, np.int32), np.full((BOW_Q, BOW_QCAP), np.nan)
        for i, q in enumerate(qs):
            words[i, : len(q[0])], values[i, : len(q[0])] = q[0], q[1]
        d["q"] = (_up(H, words), _up(H, values), _up(H, np.asarray([len(q[0]) for q in qs], np.int32)))
        d["q_out"] = dict(ids=torch.zeros((BOW_Q, 10), **i32t), scores=torch.zeros((BOW_Q, 10), dtype=torch.float64, device=dv),
                          common=torch.zeros((BOW_Q, 10), **i32t), n=torch.zeros(BOW_Q, **i32t))
        # MatchBoW: the seam's three scenes as one batch, scene k first
        scenes = [bow_match_cases()[(k + i) % 3][1] for i in range(3)]
        cap1, cap2 = 320, 300
        A = {key: np.zeros((3, c, 4), np.uint64) for key, c in (("desc1", cap1), ("desc2", cap2))}
        Hs = {key: np.zeros((3, c), np.uint8) for key, c in (("has1", cap1), ("has2", cap2))}
        bow = {s: dict(node_id=np.zeros((3, c), np.int32), node_start=np.zeros((3, c + 1), np.int32), features=np.zeros((3, c), np.int32),
                       n_nodes=np.zeros(3, np.int32)) for s, c in (("1", cap1), ("2", cap2))}
        n = {"1": np.zeros(3, np.int32), "2": np.zeros(3, np.int32)}
        for b, s in enumerate(scenes):
            for side in "12":
                dd = s["desc" + side]
                A["desc" + side][b, : len(dd)], Hs["has" + side][b, : len(dd)], n[side][b] = dd, s["has" + side], len(dd)
                nid, ns, ft = s["bow" + side]
                w = bow[side]
                w["node_id"][b, : len(nid)], w["node_start"][b, : len(ns)], w["features"][b, : len(ft)], w["n_nodes"][b] = nid, ns, ft, len(nid)
        d["m_desc"] = {key: _up(H, v.view(np.int64)) for key, v in A.items()}
        d["m_has"] = {key: _up(H, v) for key, v in Hs.items()}
        d["m_bow"] = {s: {key: _up(H, v) for key, v in w.items()} for s, w in bow.items()}
        d["m_n"] = {s: _up(H, v) for s, v in n.items()}
        d["m_frames"] = [desc_frames_dev(d["m_n"][s], d["m_desc"]["desc" + s]) for s in "12"]
        d["m_out"] = (torch.zeros((3, cap1), **i32t), torch.zeros((3, cap1, 2), **i32t), torch.zeros(3, **i32t))
        H["dev"][k] = d
    return H["dev"][k]


BOW_T_KEYS = ("words", "values", "n_words", "node_id", "node_start", "features", "n_nodes", "word_of_feature", "node_of_feature")


def bow_dev_call(H, k, which):
    d = _bow_dev(H, k)
    if which == "transform":
        for t in d["t_out"].values():
            t.fill_(-9)
        H["v_irr"].transform_batch_dev(d["frames"], 2, d["t_out"])
        n_w, n_n = d["t_out"]["n_words"], d["t_out"]["n_nodes"]
        return [d["t_out"][key] for key in BOW_T_KEYS], (n_w, n_n)
    if which == "query":
        for t in d["q_out"].values():
            t.fill_(-9)
        H["db"].query_batch_dev(*d["q"], None, None, 0.8, 0.75, 0.0, 10, d["q_out"])
        return [d["q_out"][key] for key in ("ids", "scores", "common", "n")], None
    for t in d["m_out"]:
        t.fill_(-9)
    H["lm"].match_bow_batch_dev(d["m_frames"][0], d["m_frames"][1], d["m_has"]["has1"], d["m_has"]["has2"], d["m_bow"]["1"], d["m_bow"]["2"],
                                *d["m_out"], 50, 0.75)
    return list(d["m_out"]), None


def bow_dev_bytes(which, tensors):
    """The defined part of a device entry's outputs: rows are specified up to their counts (n_words / n_nodes / n / n_pairs)."""
    a = [t.cpu().numpy() for t in tensors]
    if which == "transform":
        o = dict(zip(BOW_T_KEYS, a))
        out = cat(o["n_words"], o["n_nodes"], o["word_of_feature"], o["node_of_feature"])
        for b in range(len(o["n_words"])):
            nw, nn = int(o["n_words"][b]), int(o["n_nodes"][b])
            out += cat(o["words"][b, :nw], o["values"][b, :nw], o["node_id"][b, :nn], o["node_start"][b, : nn + 1], o["features"][b, : o["node_start"][b, nn]])
        return out
    if which == "query":
        ids, scores, common, n = a
        return cat(n) + b"".join(cat(ids[i, : n[i]], scores[i, : n[i]], common[i, : n[i]]) for i in range(len(n)))
    m12, pairs, n_pairs = a
    return cat(m12, n_pairs) + b"".join(cat(pairs[b, : n_pairs[b]]) for b in range(len(n_pairs)))


def run_bow_match(H, k):
    """the part of the bow seam that runs on a snk_matcher"""
    k %= 3
    _, s, th, ratio = bow_match_cases()[k]
    m12, n = H["lm"].match_bow(s["desc1"], s["has1"], s["bow1"], s["desc2"], s["has2"], s["bow2"], th, ratio)
    out = cat(m12) + i32(n)
    with on(H):
        out += bow_dev_bytes("match", bow_dev_call(H, k, "match")[0])
    return out


def run_bow(H, k):
    k %= 3
    import torch

    with torch.cuda.device(H["device"]):
        t = H["v_irr"].transform(BW.frame_descriptors("irregular", BOW_FRAME_COUNTS[k]), 2)
        out = cat(*(t[key] for key in ("words", "values", "node_id", "node_start", "features", "word_of_feature", "node_of_feature")))
        rows = BW.db_rows(65)
        ids = sorted(rows)
        db = H["db"]
        db.add(9000 + k, *rows[ids[k]])  # a twin of a stored row: an exact tie, lowest id first
        q = BW.db_fresh_query(65, 20 * k)
        out += cat(*db.query(q[0], q[1], (), 0.8, 0.75, 0.0, 10)) + cat(*db.query(rows[ids[k]][0], rows[ids[k]][1], (ids[0],), 0.0, 0.0, 0.0, 64))
        db.remove(9000 + k)
        out += np.float64(H["v_db"].score(rows[ids[k]], rows[ids[k + 7]])).tobytes()
    with on(H):
        for which in ("transform", "query"):
            out += bow_dev_bytes(which, bow_dev_call(H, k, which)[0])
    return out + run_bow_match(H, k)


def make_pgo(device=0, stream=None):
    from snake_slam_amd.loop import PoseGraphOptimizer

    st = _stream(device, stream)
    return _base(device, st, [PoseGraphOptimizer(None, device, st.cuda_stream)], matchers=[], pcg_form=[], poses=[])


def run_pgo(H, k):
    """Also appends every solve's pcg_form to H["pcg_form"] and its poses to H["poses"]."""
    k %= 3
    o = H["objs"][0]
    out = b""
    for fix in (1, 0):
        G = pgo_graph(k, fix)
        o.set_graph(G["poses_measure"], G["constant"], G["edges"], G["weights"], G["meas"], G["start"], G["fix_scale"])
        res = o.solve()
        poses = o.poses()
        rng = np.random.default_rng(600 + k)
        n = len(poses)
        ref = rng.integers(-1, n, 200).astype(np.int32)
        pos, nrm, dep = o.transform_points(ref, rng.uniform(-5, 5, (200, 3)), rng.normal(size=(200, 3)), rng.uniform(0.5, 20, 200))
        H["pcg_form"].append(int(res["pcg_form"]))
        H["poses"].append(poses)
        out += cat(poses, pos, nrm, dep) + np.float64([res["cost_initial"], res["cost_final"]]).tobytes() + i32(res["lm_iterations"], res["accepted_steps"])
    return out


def make_knn2(device=0, stream=None):
    from snake_slam_amd.matcher import BruteForceMatcher

    st = _stream(device, stream)
    return _base(device, st, [BruteForceMatcher(device, st.cuda_stream)])


def knn2_match(H, k):
    q, t = front_cases()["bf"][k % 3]
    H["objs"][0].matchKnn2(q, t)


def knn2_filter(H, k):
    m = H["objs"][0]
    n = m.filterMatches(90, 0.9)
    return cat(m.knn, m.matches) + i32(n)


def run_knn2(H, k):
    knn2_match(H, k)
    return knn2_filter(H, k)


def make_stereo(device=0, stream=None):
    from snake_slam_amd.matcher import Preprocess

    st = _stream(device, stream)
    return _base(device, st, [Preprocess(device, st.cuda_stream)])


def stereo_rect():
    """EuRoC cam0 with its distortion, as Preprocess::undistortKeypoints has it"""
    from snake_slam_amd.matcher import Rectification
    from test_oracle_preprocess import EUROC_D, EUROC_K

    return Rectification.make(EUROC_K, EUROC_D)


def run_stereo(H, k):
    left, dl, right, dr, bf, ls = front_cases()["stereo"][k % 3]
    pp = H["objs"][0]
    n, rp, dp = pp.StereoMatching(left, dl, right, dr, bf, ls, True)
    # undistortKeypoints on the same handle, with and without the normalized points
    und, norm = pp.rectify(stereo_rect(), front_cases()["rect"][k % 3], True)
    und2, none = pp.rectify(stereo_rect(), front_cases()["rect"][k % 3], False)
    assert none is None
    return i32(n) + cat(rp, dp, und, norm, und2)


def make_track(device=0, stream=None):
    from snake_slam_amd.tracking import SnakeORBMatcher

    st = _stream(device, stream)
    return _base(device, st, [SnakeORBMatcher(device, st.cuda_stream)])


def track_bind(H, k):
    H["objs"][0].bind_frame(front_cases()["track"][k % 3][0])


def track_search(H, k):
    """on the BOUND frame (frame = None): the coarse matcher, then the keyframe matcher -- which leaves its match count in the handle's
    counter buffer, the one the map-point refresh counts its wide points in"""
    from snake_slam_amd.tracking import FeatureGrid

    frame, cam, pose, ls, pts, (pos, desc, skip) = front_cases()["track"][k % 3]
    m = H["objs"][0]
    n, idx = m.SearchByProjectionFrameFrame2(None, cam, pose, pts, 15.0, 75, 0, ls)
    n_kf, idx_kf = m.SearchByProjectionFrameToKeyframe(None, cam, pose, pos, desc, skip, 15.0, 100)
    # the frame's grid (snk_feature_grid, from the keypoints in reverse order) and the fine matcher, on the seam's handle too
    perm, cell_start, _, _ = FeatureGrid.create(m, frame["bounds"], frame["kps"][::-1])
    n_f, idx_f, vis, valid = m.SearchByProjection2(None, cam, pose, front_cases()["fine"][k % 3], 5.0, 0.8, ls)
    return i32(n, n_kf, n_f) + cat(idx, idx_kf, perm, cell_start, idx_f, vis, valid)


def run_track(H, k):
    track_bind(H, k)
    return track_search(H, k)


def make_pose(device=0, stream=None):
    from snake_slam_amd.tracking import PoseRefinement

    st = _stream(device, stream)
    return _base(device, st, [PoseRefinement(device=device, stream=st.cuda_stream)])


def run_pose(H, k):
    import pose_helpers as PH

    pr = pose_case(k % 3)
    pose, outl, inl = H["objs"][0].refinePose(PH.CAM, pr["pose0"], pr["wps"], pr["obs"])
    odd = H["objs"][0].refine_batch(PH.CAM, [dict(pose=p["pose0"], wps=p["wps"], obs=p["obs"]) for p in pose_odd_batch(k % 3)])
    assert odd[1][2] == 0 and len(odd[1][1]) == 0  # n = 0: no inlier, no flag
    return cat(pose, outl) + i32(inl) + b"".join(cat(p, o) + i32(n) for p, o, n in odd)


SEAMS = {"p3p": (make_p3p, run_p3p), "sim3": (make_sim3, run_sim3), "tri": (make_tri, run_tri), "mappoint": (make_mappoint, run_mappoint),
         "covis": (make_covis, run_covis), "bow": (make_bow, run_bow), "pgo": (make_pgo, run_pgo), "knn2": (make_knn2, run_knn2),
         "stereo": (make_stereo, run_stereo), "track": (make_track, run_track), "pose": (make_pose, run_pose), "lmap": (make_lmap, run_lmap),
         "scene": (make_scene, run_scene)}
# what runs on a snk_matcher (bow: its MatchBoW part, the vocabulary and the database have handles of their own)
MATCHER_SEAMS = ("knn2", "stereo", "track", "pose", "p3p", "sim3", "tri", "mappoint", "covis", "bow", "lmap", "scene")
# the poison children: four groups, torch's import paid four times
GROUPS = {"front": ("knn2", "stereo", "track", "pose", "tri"), "ransac": ("p3p", "sim3", "mappoint", "covis"), "loop": ("bow", "pgo"),
          "map": ("lmap", "scene")}


def run_on_matcher(name):
    return run_bow_match if name == "bow" else SEAMS[name][1]


def solo(name, device=0, ks=(0, 1, 2)):
    """the seam on fresh handles of its own: [bytes of case k for k in ks]"""
    make, run = SEAMS[name]
    H = make(device, None)
    try:
        return [run(H, k) for k in ks]
    finally:
        close_handles(H)


_solo_cache: dict = {}


def solo_bytes(name, run=None):
    """the unpoisoned solo result on device 0, computed once per process and left unchanged"""
    key = (name, run)
    if key not in _solo_cache:
        if run is None:
            _solo_cache[key] = solo(name)
        else:
            H = SEAMS[name][0](0, None)
            try:
                _solo_cache[key] = [run(H, k) for k in range(3)]
            finally:
                close_handles(H)
    return _solo_cache[key]


# ------------------------------------------------------------------------------------------------------------------------------------
# growth: the smallest calls that need more scratch than a snk_matcher HOLDS after create -- scratch_capacity(MATCHER_*_BYTES) of
# dispatch.hpp, a quarter more than the nominal sizes -- so that the device block AND both pinned blocks are freed and reallocated
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def matcher_constants():
    """MATCHER_*_BYTES and what a buffer created with each holds, asked of the compiled dispatch.hpp (tests/cpp/dispatch_driver.cpp)"""
    import tempfile

    import forms

    names = ("MATCHER_SCRATCH_BYTES", "MATCHER_H_IN_BYTES", "MATCHER_H_RES_BYTES")
    with tempfile.TemporaryDirectory() as d:
        exe = forms.build_driver(d)
        out = dict(zip(names, map(int, forms.ask(exe, [("const", (n,)) for n in names]))))
        caps = forms.ask(exe, [("capacity", (out[n],)) for n in names])
    out.update(dev_capacity=int(caps[0]), h_in_capacity=int(caps[1]), h_res_capacity=int(caps[2]))
    return out


def align16(n):
    return (n + 15) & ~15


P3P_PAIR_BYTES, SIM3_PAIR_BYTES = 24 + 16, 24 + 24 + 16 + 16  # what a pair takes of the input block (p3p.hip / sim3.hip ransac_host)
P3P_PAIR_RESULT_BYTES = 4 + 1                                  # and of the result block: a list entry and a mask byte (sim3: the mask byte)
SIM3_RESULT_BYTES = 72                                         # Sim3Result, one per problem in front of the mask bytes
MP_RESULT_BYTES, COVIS_CONN_BYTES, COVIS_RESULT_BYTES, KNN2_BYTES = 80, 8, 16, 16
GROWTH_ITERATIONS = 8  # keeps the large calls far below a second of device time
GROWTH_COVIS_CAP = 256
GROWTH_SET_CAP = 512   # entries per padded vote set of the large covis call
GROWTH_KNN2_TRAIN = 4096
LMAP_POINT_BYTES = 1 + 4 + 24 + 24 + 32 + 4 + 4                        # a map point in snk_lmap_gather's input block: flags, last_seen and the five tables of snk_lmap_points
LMAP_SET_RESULT_BYTES = LMAP_PTS_CAP * (96 + 4) + 4 + 16               # a set in its result block: the records, the ids, n_pts, the result
SCENE_POINT_BYTES = 4 + 1 + 24                                         # a map point in snk_scene_gather's input block: obs_start, flags, position
SCENE_ROW_BYTES = dict(img_cap=(4, 56, 1), pt_cap=(4, 24, 1, 1), obs_cap=(4, 4, 16, 8, 8, 8), win_cap=(80,))  # an item of every row output of snk_scene_out, by its cap
SCENE_QUERY_RESULT_BYTES = sum(SCENE_CAPS[cap] * sum(items) for cap, items in SCENE_ROW_BYTES.items()) + 24  # a query in its result block
POSE_MATCHES, POSE_MATCH_BYTES, POSE_RESULT_BYTES = 300, 24 + 32, 56 + 4  # pose_case: matches per problem; a match in the input block; a
#                                                                           problem in the result block behind the outlier bytes


def growth_sizes():
    """The smallest counts with which the call asks for more than the handle's buffers hold:
    p3p -- problems of the largest pair count: the input block past `q` (with it past `h_in`; the result block is then past `h_res`);
    sim3 -- problems of the largest pair count: the result block (a record and the mask bytes) past `h_res` (the input is then past `q` and `h_in`, the slabs past `aux2`);
    mappoint -- points of one observation: the result block past `out` (with it past `h_res`; the input is then past `q` and `h_in`);
    covis -- padded vote sets: the set array alone past `q` / `h_in` and the lists past `out` / `h_res`;
    knn2 -- queries: the result block past `out` / `h_res` (query + train is then past `q` / `h_in`);
    pose -- problems of pose_case(0): the result block (an outlier byte per match, a pose and a count per problem) past `h_res` (the
    input is then past `q` / `h_in`);
    lmap -- sets of gather: the result block past `out` / `h_res`, and map points (behind the case's own, seen by nobody): the point tables
    past `q` / `h_in`;
    scene -- queries of gather and map points in the same way."""
    c = matcher_constants()
    dev, h_res = c["dev_capacity"], c["h_res_capacity"]
    return dict(p3p_problems=dev // (P3P_PAIR_BYTES * P3.MAX_PAIRS) + 1,
                sim3_problems=h_res // (S3.MAX_PAIRS + SIM3_RESULT_BYTES) + 1,
                mappoint_points=dev // MP_RESULT_BYTES + 1,
                covis_sets=max(dev // (GROWTH_SET_CAP * 4), dev // (GROWTH_COVIS_CAP * COVIS_CONN_BYTES + COVIS_RESULT_BYTES)) + 1,
                knn2_queries=dev // KNN2_BYTES + 1,
                pose_problems=h_res // (POSE_MATCHES + POSE_RESULT_BYTES) + 1,
                lmap_sets=dev // LMAP_SET_RESULT_BYTES + 1, lmap_points=dev // LMAP_POINT_BYTES + 1,
                scene_queries=dev // SCENE_QUERY_RESULT_BYTES + 1, scene_points=dev // SCENE_POINT_BYTES + 1)


def growth_requests(name):
    """{buffer: bytes the large call asks of it}, by the layout of the host entry (p3p.hip / sim3.hip ransac_host, snk_mappoint_refresh,
    covis.hip run_host, snk_bf_knn2, snk_lmap_gather, snk_scene_gather: stage.hpp pads every part to 16 bytes) -- at least: the per-problem records of the RANSACs come on top.  Every buffer named here must
    be reallocated by the call."""
    g = growth_sizes()
    if name == "p3p":
        total = g["p3p_problems"] * P3.MAX_PAIRS
        return dict(q=total * P3P_PAIR_BYTES, h_in=total * P3P_PAIR_BYTES, h_res=total * P3P_PAIR_RESULT_BYTES)
    if name == "sim3":
        total = g["sim3_problems"] * S3.MAX_PAIRS
        return dict(q=total * SIM3_PAIR_BYTES, h_in=total * SIM3_PAIR_BYTES, h_res=total + g["sim3_problems"] * SIM3_RESULT_BYTES,
                    aux2=g["sim3_problems"] * (S3.MAX_PAIRS - S3.LDS_PAIRS) * S3.BYTES_PER_PAIR)
    if name == "mappoint":
        n = g["mappoint_points"]  # one observation each: obs_start | ref_obs | position | valid | octave | cam_pose | desc
        bytes_in = align16((n + 1) * 4) + align16(n * 4) + align16(n * 24) + align16(n) + align16(n * 4) + align16(n * 56) + align16(n * 32)
        return dict(q=bytes_in, h_in=bytes_in, out=n * MP_RESULT_BYTES, h_res=n * MP_RESULT_BYTES)
    if name == "covis":
        n = g["covis_sets"]
        out = align16(n * GROWTH_COVIS_CAP * COVIS_CONN_BYTES) + n * COVIS_RESULT_BYTES
        return dict(q=n * GROWTH_SET_CAP * 4, h_in=n * GROWTH_SET_CAP * 4, out=out, h_res=out)
    if name == "knn2":
        n = g["knn2_queries"]
        return dict(q=(n + GROWTH_KNN2_TRAIN) * 32, h_in=(n + GROWTH_KNN2_TRAIN) * 32, out=n * KNN2_BYTES, h_res=n * KNN2_BYTES)
    if name == "pose":
        n = g["pose_problems"]
        return dict(q=n * POSE_MATCHES * POSE_MATCH_BYTES, h_in=n * POSE_MATCHES * POSE_MATCH_BYTES, h_res=n * (POSE_MATCHES + POSE_RESULT_BYTES))
    if name == "lmap":
        n, pts = g["lmap_sets"], g["lmap_points"]  # the point parts: pt_flags | pt_last_seen | pos | normal | desc | ref_depth | ref_level
        bytes_in = sum(align16(pts * b) for b in (1, 4, 24, 24, 32, 4, 4))
        out = align16(n * LMAP_PTS_CAP * 96) + align16(n * LMAP_PTS_CAP * 4) + align16(n * 4) + n * 16  # lm_pts | lm_point | n_pts | result
        return dict(q=bytes_in, h_in=bytes_in, out=out, h_res=out)
    if name == "scene":
        n, pts = g["scene_queries"], g["scene_points"]  # the point parts: obs_start | pt_flags | pt_pos
        bytes_in = align16((pts + 1) * 4) + align16(pts) + align16(pts * 24)
        out = sum(align16(n * SCENE_CAPS[cap] * b) for cap, items in SCENE_ROW_BYTES.items() for b in items) + align16(n * 24)  # the rows | result
        return dict(q=bytes_in, h_in=bytes_in, out=out, h_res=out)
    raise KeyError(name)


def growth_capacity(buffer):
    c = matcher_constants()
    return c["h_in_capacity"] if buffer == "h_in" else c["h_res_capacity"] if buffer == "h_res" else c["dev_capacity"]


@functools.lru_cache(maxsize=None)
def growth_case(name):
    g = growth_sizes()
    if name == "p3p":
        c = P3.make_case(P3.MAX_PAIRS, 0.3, 1.0, 4301)
        return [dict(wps=c["wps"], nips=c["nips"])] * g["p3p_problems"]
    if name == "sim3":
        c = S3.make_case(S3.MAX_PAIRS, 0.3, 1.0, False, GROWTH_ITERATIONS, 4302)
        return [dict(points1=c["P1"], points2=c["P2"], ips1=c["ip1"], ips2=c["ip2"])] * g["sim3_problems"]
    if name == "mappoint":
        # the points of a small case of single observations, repeated: the generator draws point by point
        n, rep = g["mappoint_points"], 1024
        c = MP.make_case(4303, [1] * rep, False, invalid_frac=0.1)
        t = lambda a: np.ascontiguousarray(np.concatenate([a] * (n // rep + 1))[:n])  # noqa: E731
        return dict(obs_start=np.arange(n + 1, dtype=np.int32), desc=t(c["desc"]), pose=t(c["pose"]), octave=t(c["octave"]), valid=t(c["valid"]),
                    position=t(c["position"]), ref_obs=t(c["ref_obs"]))
    if name == "covis":
        m = covis_case(0)["m"]
        return CV.frames_of(m, 4304, g["covis_sets"], cap=GROWTH_SET_CAP)
    if name == "knn2":
        rng = np.random.default_rng(4305)
        return rand_desc(rng, g["knn2_queries"]), rand_desc(rng, GROWTH_KNN2_TRAIN)
    if name == "pose":
        pr = pose_case(0)
        return [dict(pose=pr["pose0"], wps=pr["wps"], obs=pr["obs"])] * g["pose_problems"]
    if name == "lmap":
        # the three sets of case 0 in turn; the point tables go on behind the case's own points with zeros
        gc = LM.edge_case(LMAP_PTS_CAP)["gather"]
        sets = [gc["what"][n] for n in LMAP_GATHER_SETS[0]]
        c = _lmap_gather_sets(gc, [sets[i % 3] for i in range(g["lmap_sets"])])
        m = dict(c["m"])
        for key in ("pt_flags", "pt_last_seen") + LM.POINT_KEYS:
            m[key] = np.concatenate([m[key], np.zeros((g["lmap_points"] - len(m[key]),) + m[key].shape[1:], m[key].dtype)])
        return dict(c, m=m)
    if name == "scene":
        # the queries of case 0 in turn; points without observations behind the map's own
        t = dict(scene_map())
        more = g["scene_points"] - len(t["pt_flags"])
        t["obs_start"] = np.concatenate([t["obs_start"], np.full(more, t["obs_start"][-1], np.int32)])
        t["pt_flags"] = np.concatenate([t["pt_flags"], np.zeros(more, np.uint8)])
        t["pt_pos"] = np.concatenate([t["pt_pos"], np.zeros((more, 3))])
        q = scene_queries(0)
        return t, [q[i % 3] for i in range(g["scene_queries"])]
    raise KeyError(name)


def growth_call(name, H):
    """the large call on the seam's handle; the wrapper's parameters are put back afterwards"""
    o, c = H["objs"][0], growth_case(name)
    if name == "p3p":
        o.params.iterations = GROWTH_ITERATIONS
        try:
            res = o.solve_batch(c)
        finally:
            o.params.iterations = 250
        return b"".join(cat(r["pose"], r["mask"], r["matches"]) + i32(r["inliers"], *r["best"]) for r in res)
    if name == "sim3":
        p = o.params
        p.iterations, p.compute_scale, p.seed = GROWTH_ITERATIONS, 0, 4302
        res = o.solve_batch(c)
        return b"".join(cat(r["T"], r["mask"]) + np.float64(r["scale"]).tobytes() + i32(r["inliers"], r["best"]) for r in res)
    if name == "mappoint":
        o.rule = MP.MEDIAN
        return o.refresh(*(c[a] for a in MP_ARGS)).tobytes()
    if name == "covis":
        m = covis_case(0)["m"]
        o.cap = GROWTH_COVIS_CAP
        try:
            return cat(*o.vote(*(m[a] for a in CV.MAP_KEYS), c[0], c[1]))
        finally:
            o.cap = COVIS_CAP
    if name == "knn2":
        o.matchKnn2(*c)
        return cat(o.knn)
    if name == "pose":
        import pose_helpers as PH

        return b"".join(cat(pose, outl) + i32(inl) for pose, outl, inl in o.refine_batch(PH.CAM, c))
    if name == "lmap":
        return lmap_gather_bytes(o, c)
    if name == "scene":
        return scene_bytes(o, *c)
    raise KeyError(name)


# No growth case: bow (MatchBoW takes at most 2048 features a keyframe, 66 KB a side: it cannot outgrow a buffer); tri and stereo (their
# inputs are whole keyframes / images, and one past 5 MiB of scratch has some 90 000 keypoints, beyond what the stereo row index holds);
# track (82 000 local-map points would do it; not built: the seam rebinds its frame in every run, which the bound-frame check needs kept)
GROWTH_SEAMS = ("p3p", "sim3", "mappoint", "covis", "knn2", "pose", "lmap", "scene")


# ------------------------------------------------------------------------------------------------------------------------------------
# the *_dev / *_batch_dev entries on their own: (seam, inputs(H, k) -> the device tensors the entry reads, call(H, k) -> the tensors it
# wrote, to_bytes(tensors)).  call only enqueues on the seam's stream (call it under on(H)); inputs allocates everything the call uses.
# ------------------------------------------------------------------------------------------------------------------------------------
def _plain(tensors):
    return cat(*(t.cpu().numpy() for t in tensors))


def _flat(v):
    if isinstance(v, dict):
        v = list(v.values())
    return [t for x in v for t in _flat(x)] if isinstance(v, (list, tuple)) else [v]


def _tensors(d, keys):
    return [t for key in keys for t in _flat(d[key])]


def _sim3_entry(cs):
    keys = ("n1", "n2", "n_pts1", "n_pts2", "frame_pt1", "frame_pt2", "poses1", "poses2", "pts1", "pts2", "kps1", "kps2", "pairs", "n_pairs", "T0")
    return ("sim3", lambda H, k: _tensors(H["D"], keys), lambda H, k: sim3_dev_call(H, k, cs, 100), _plain)


def _bow_entry(which, keys):
    return ("bow", lambda H, k: _tensors(_bow_dev(H, k), keys), lambda H, k: bow_dev_call(H, k, which)[0], lambda t: bow_dev_bytes(which, t))


DEV_ENTRIES = {
    "p3p_frame_batch": ("p3p", lambda H, k: _tensors(_p3p_dev(H, k), ("n", "kps", "pts", "n_pts", "frame_pt0", "poses0")), p3p_dev_call, _plain),
    "sim3_pairs_batch_se3": _sim3_entry(False),
    "sim3_pairs_batch_sim3": _sim3_entry(True),
    "mappoint_refresh_batch": ("mappoint", lambda H, k: _tensors(_mappoint_dev(H, k), ("n", "kps", "desc", "poses", "start", "obs", "valid", "position", "ref")),
                               lambda H, k: mappoint_dev_call(H, k, MP.MEDIAN), _plain),
    "covis_update": ("covis", lambda H, k: _tensors(_covis_dev(H, k), ("map", "feat", "q")), lambda H, k: covis_dev_call(H, k, "update"), _plain),
    "covis_vote": ("covis", lambda H, k: _tensors(_covis_dev(H, k), ("map", "set_start", "set_point")), lambda H, k: covis_dev_call(H, k, "vote"), _plain),
    "bow_transform_batch": _bow_entry("transform", ("desc", "n")),
    "bow_query_batch": _bow_entry("query", ("q",)),
    "bow_match_batch": _bow_entry("match", ("m_desc", "m_has", "m_bow", "m_n")),
}


def own_stream_cycle(device=0):
    """create -> one small host call -> close of every matcher-handle wrapper of the back end and of the pose-graph optimiser WITHOUT a
    caller's stream: the handle creates and destroys a stream of its own (the seams above always bring one)"""
    from snake_slam_amd.bow import LoopMatcher
    from snake_slam_amd.covis import CovisibilityGraph
    from snake_slam_amd.loop import PoseGraphOptimizer, RegistrationRansac
    from snake_slam_amd.mappoint import MapPointRefresher
    from snake_slam_amd.tracking import P3PRansac, Triangulator

    def use(obj, call):
        try:
            call(obj)
        finally:
            obj.close()

    c = p3p_cases()[0][0]
    use(P3PRansac(GROWTH_ITERATIONS, P3.THRESHOLD, 1, device), lambda o: o.solve_batch([dict(wps=c["wps"], nips=c["nips"])]))
    s = sim3_cases()[0]
    use(RegistrationRansac(S3.CAM, S3.THRESHOLD, GROWTH_ITERATIONS, False, 1, device=device),
        lambda o: o.solve_batch([dict(points1=s["P1"], points2=s["P2"], ips1=s["ip1"], ips2=s["ip2"])]))
    t = tri_case(0)
    p = t["params"]
    use(Triangulator(t["cam"], t["level_scale"], p["error_mono"], p["error_stereo"], p["th_depth"], mono=bool(p["mono"]), device=device),
        lambda o: o.Process(t["kf1"], t["kf2s"], t["pairs"], t["median_depth2s"]))
    m = mappoint_case(0)
    use(MapPointRefresher(MP.MEDIAN, device), lambda o: o.refresh(*(m[a] for a in MP_ARGS)))
    v = covis_case(0)
    use(CovisibilityGraph(CV.TH, CV.TH_DEPTH, COVIS_CAP, device), lambda o: o.update(*(v["m"][a] for a in CV.MAP_KEYS + CV.FEAT_KEYS), v["q"]))
    _, b, th, ratio = bow_match_cases()[1]
    use(LoopMatcher(device), lambda o: o.match_bow(b["desc1"], b["has1"], b["bow1"], b["desc2"], b["has2"], b["bow2"], th, ratio))
    G = pgo_graph(2, 1)

    def pgo(o):
        o.set_graph(G["poses_measure"], G["constant"], G["edges"], G["weights"], G["meas"], G["start"], G["fix_scale"])
        o.solve()

    use(PoseGraphOptimizer(None, device), pgo)
