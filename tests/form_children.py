"""The two kernel forms that no launch shape selects -- pose_kernel<4, false> (SNK_POSE_NO_LDS) and the stereo row index by the bitonic
network at a batch of 8 or more (SNK_STEREO_NO_FRAME_KERNEL + SNK_STEREO_SORT_NETWORK) -- read their switch once per process, so each
runs in a child: `python form_children.py pose|stereo OUT.npz` builds the seeded inputs below, runs them on the device and writes what
came back.  The parent test (test_pose_forms_gpu.py, test_match_forms_gpu.py) builds the same inputs and compares with the oracle."""
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


def main(kind, out):
    if kind == "stereo":
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


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
