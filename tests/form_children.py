"""The two kernel forms that no launch shape selects -- pose_kernel<4, false> (SNK_POSE_NO_LDS) and the stereo row index by the bitonic
network at a batch of 8 or more (SNK_STEREO_NO_FRAME_KERNEL + SNK_STEREO_SORT_NETWORK) -- read their switch once per process, so each
runs in a child: `python form_children.py pose|stereo OUT.npz` builds the seeded inputs below, runs them on the device and writes what
came back.  The parent test (test_pose_forms_gpu.py, test_match_forms_gpu.py) builds the same inputs and compares with the oracle.

`python form_children.py track_lds|track_wgs2 OUT.npz`: the batched projection matchers at the capacities where their LDS carve ends,
which need SNK_TRACK_PPW / SNK_TRACK_FRAME_WGS (test_track_forms_gpu.py); the launches are the rows of tests/forms.py with 2049 points."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

TESTS = Path(__file__).resolve().parent
for p in (str(TESTS.parent), str(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)

POSE_BATCH = dict(cap=256, mcap=200, nf=[240, 150, 0, 210, 256], npts=[200, 40, 10, 200, 190])  # stride 256: the four-wavefront forms


def stereo_case(B):
    """B frames of up to 400 right keypoints: (frames, capl, bf, level scales)."""
    from helpers import SEED, make_stereo_case

    rng = np.random.default_rng(SEED + 816)
    frames = []
    for nr in ([400, 1, 333, 0, 400, 65, 399, 256] * 2)[:B]:
        left, dl, right, dr, bfv, ls = make_stereo_case(rng, 300 if nr else 5, max(nr, 1))
        frames.append((left, dl, right[:nr], dr[:nr]))
    return frames, 310, bfv, ls


def pose_problem():
    import pose_helpers as PH

    return PH.make_problem(77, 300, outlier_frac=0.2)


def pose_batch_case():
    from test_tracking_chain_gpu import frame_batch_case

    return frame_batch_case(**POSE_BATCH)


TRACK_LDS_POINTS = [2049, 1024, 1025, 2048, 1023, 1, 0]   # of pts_cap 2049: a last chunk of one point, full and nearly full chunks, none


def track_lds_rows(frame_wgs):
    """The rows of the table with 2049 points per frame and that many workgroups per frame, in table order: [(shape, form)]."""
    import forms

    return [(s, f) for e, s, f in forms.FORMS if e == "track_launch" and s[0] == 2049 and s[5] == frame_wgs]


_track_base = []


def track_lds_case(orc, cap):
    """Seven frames at the capacity `cap`: three hold exactly cap features, one none (with points present), the others a part; the
    points carry copies that want the feature of their original.  (frames, cam, poses, level scales, coarse, fine, copies per frame)"""
    import track_helpers as T
    from helpers import SEED

    if not _track_base:   # three scenes of 2049 points and more features than any capacity asked for; the frames are thinned from them
        for k in range(3):
            rng = np.random.default_rng(SEED + 930 + k)
            frame, cam, pose, ls, world, _ = T.make_tracking_case(orc, rng, n_clutter=500, m_pts=2049)
            # (rolled: the points behind the camera are the first of a scene, and the frame of one point takes the first one)
            _track_base.append((frame, cam, pose, ls, np.roll(T.lm_coarse(orc, world), -128), np.roll(T.lm_fine(orc, rng, world, pose, ls), -128)))
    rng = np.random.default_rng(SEED + 940)
    n_feat = [cap, 0, 900, cap, cap, 901, cap // 2]
    frames, poses, coarse, fine, copies = [], [], [], [], []
    for b, (n, m) in enumerate(zip(n_feat, TRACK_LDS_POINTS)):
        frame, cam, pose, ls, pc, pf = _track_base[b % 3]
        frame = T.thin_to(orc, rng, frame, n)
        pc, pf = pc[:m].copy(), pf[:m].copy()
        copies.append(T.add_conflicts(orc, frame, cam, pose, ls, pc, pf))
        frames.append(frame), poses.append(pose), coarse.append(pc), fine.append(pf)
    return frames, cam, poses, ls, coarse, fine, copies


def track_bad_counts(frames, coarse, fine, cap, pts_cap):
    """Device-side counts out of range for a chain whose frame 0 is full and frame 1 empty: (n_feat, n_pts) as the device reads them, and
    the frames / points that the clamped counts describe (a row's records past its points are zeros)."""
    n_feat = [len(f["kps"]) for f in frames]
    n_pts = [len(p) for p in coarse]
    assert n_feat[0] == cap and n_feat[1] == 0 and n_pts[2] < pts_cap
    n_feat[0], n_feat[1] = cap + 9, -3
    n_pts[0], n_pts[1], n_pts[2] = -5, pts_cap + 7, pts_cap + 7
    grow = lambda a, m: np.concatenate([a, np.zeros(m - len(a), a.dtype)])[:m]
    eff_c = [coarse[0][:0], grow(coarse[1], pts_cap), grow(coarse[2], pts_cap)] + list(coarse[3:])
    eff_f = [fine[0][:0], grow(fine[1], pts_cap), grow(fine[2], pts_cap)] + list(fine[3:])
    return n_feat, n_pts, eff_c, eff_f


def _track_child(kind, out):
    import track_helpers as T
    from oracle import oracle as orc
    from snake_slam_amd.tracking import SnakeORBMatcher

    keep = ("mi_c", "mi_f", "vis", "n_c", "n_f", "taken")
    save = {}
    matcher = SnakeORBMatcher(0)
    try:
        for shape, _ in track_lds_rows(1 if kind == "track_lds" else 2):
            pts_cap, cap = shape[0], shape[2]
            frames, cam, poses, ls, coarse, fine, _ = track_lds_case(orc, cap)
            res = T.run_chain_dev(matcher, frames, cam, poses, ls, coarse, fine, cap, pts_cap, pts_cap)
            save.update({f"{k}_{cap}": res[k] for k in keep})
            save[f"valid_{cap}"] = res["pf"]["valid"]
        if kind == "track_lds":   # counts out of range at the first capacity (the fused resolution at the end of its carve), between guard rows
            shape = track_lds_rows(1)[0][0]
            pts_cap, cap = shape[0], shape[2]
            frames, cam, poses, ls, coarse, fine, _ = track_lds_case(orc, cap)
            n_feat, n_pts, _, _ = track_bad_counts(frames, coarse, fine, cap, pts_cap)
            res = T.run_chain_dev(matcher, frames, cam, poses, ls, coarse, fine, cap, pts_cap, pts_cap, n_feat=n_feat, n_coarse=n_pts, n_fine=n_pts,
                                  guards=True, expect_cleared=False)
            save.update({f"{k}_bad": res[k] for k in keep})
            save["valid_bad"], save["guards_intact"] = res["pf"]["valid"], np.array(res["guards_intact"])
    finally:
        matcher.close()
    np.savez(out, **save)


def main(kind, out):
    if kind in ("track_lds", "track_wgs2"):
        _track_child(kind, out)
    elif kind == "stereo":
        from helpers import stereo_batch_dev
        from snake_slam_amd.matcher import StereoMatcher

        frames, capl, bfv, ls = stereo_case(8)
        st = StereoMatcher(0)
        try:
            rp, dp, nm = stereo_batch_dev(st, frames, capl, 400, bfv, ls)
        finally:
            st.close()
        np.savez(out, rp=rp, dp=dp, nm=nm)
    elif kind == "pose":
        import pose_helpers as PH
        from snake_slam_amd.tracking import PoseRefinement
        from test_tracking_chain_gpu import run_frame_batch

        pr = pose_problem()
        ref = PoseRefinement()
        try:
            pose, outl, inl = ref.refinePose(PH.CAM, pr["pose0"], pr["wps"], pr["obs"])
        finally:
            ref.close()
        b_pose, b_outl, b_inl = run_frame_batch(pose_batch_case())
        np.savez(out, pose=pose, outl=outl, inl=inl, b_pose=b_pose, b_outl=b_outl, b_inl=b_inl)
    else:
        raise SystemExit(f"form_children.py: unknown kind {kind!r}")


def run_child(kind, out, **switches):
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), kind, str(out)], env=dict(os.environ, **switches), capture_output=True,
                       text=True, cwd=str(TESTS.parent), timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return r


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
