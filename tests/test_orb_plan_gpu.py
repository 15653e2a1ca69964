"""GPU: the launch plan of the ORB extractor is observed, not trusted.  Under SNK_DEBUG every launch chain (run_part) prints its plan; the
forms on those lines must be the ones dispatch.hpp gives for the same configuration (asked of the CPU driver), the rows of tests/forms.py
these shapes are pinned to, and the keypoints and descriptors of the same run must equal the oracle's."""
import os
import subprocess
import sys

import numpy as np
import pytest

import forms

pytestmark = pytest.mark.gpu

CHILD = r"""
import sys
import numpy as np
import torch
from snake_slam_amd import synth
from snake_slam_amd.orb import ORBExtractor, KEYPOINT_DTYPE

out, nfeat1, w2, h2, nfeat2, levels, B = sys.argv[1], *map(int, sys.argv[2:8])
ext = ORBExtractor(nfeat1, 1.2, levels, 20, 7)
kps, desc = ext.Detect(synth.stereo_frame(0)[0])                       # snk_orb_detect: one 752 x 480 image
ext.close()
imgs = np.stack([synth.stereo_frame(500 + i, w2, h2, n_rects=40)[0] for i in range(B)])
ext = ORBExtractor(nfeat2, 1.2, levels, 20, 7)
cap = ext.configure(w2, h2, B)
dev = torch.device("cuda:0")
d_img = torch.from_numpy(imgs).to(dev)
d_kps = torch.zeros((B, cap, 24), dtype=torch.uint8, device=dev)
d_desc = torch.zeros((B, cap, 4), dtype=torch.int64, device=dev)
d_n = torch.zeros(B, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
ext.detect_batch_dev(d_img, d_kps, d_desc, d_n)                        # snk_orb_detect_batch_dev
ext.sync()
np.savez(out, kps=kps, desc=desc, n=d_n.cpu().numpy(), bkps=d_kps.cpu().numpy().view(KEYPOINT_DTYPE).reshape(B, cap), bdesc=d_desc.cpu().numpy().view(np.uint64))
ext.close()
"""


def test_plan_lines_name_the_forms_that_ran(orc, tmp_path):
    from snake_slam_amd import synth
    from snake_slam_amd.orb import KEYPOINT_DTYPE

    switches = forms.orb_env_switches(os.environ)
    single, batch = forms.orb(), forms.orb(w=160, h=120, nfeat=500, batch=16)
    if not switches:   # the default path: both shapes are rows of the table
        single = forms.shape("orb_plan", single, "8+,8+,8+,8;1/3;none;one_full;dma")
        batch = forms.shape("orb_plan", batch, "8+,8+,8+,8;1/4;none;one_full;dma")
    F = dict(zip(forms.ORB_FIELDS, batch))
    out = tmp_path / "plan_run.npz"
    r = subprocess.run([sys.executable, "-c", CHILD, str(out), str(single[2]), str(F["w"]), str(F["h"]), str(F["nfeat"]), str(F["levels"]), str(F["batch"])],
                       env=dict(os.environ, SNK_DEBUG="1"), capture_output=True, text=True, cwd=str(forms.ROOT), timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = forms.orb_plan_lines(r.stderr)
    print(r.stderr)
    assert [sh for sh, _ in lines] == [single[:-1], batch[:-1]]   # one line per launch chain, with the configuration it ran
    want = forms.ask(forms.build_driver(tmp_path), [("orb_plan", sh + (switches,)) for sh, _ in lines])
    assert [f for _, f in lines] == want
    if not switches:
        assert want == ["8+,8+,8+,8;1/3;none;one_full;dma", "8+,8+,8+,8;1/4;none;one_full;dma"]
    # what those plans computed
    got = np.load(out)
    wk, wd = orc.orb_detect(orc.orb_params(single[2], 1.2, single[3], 20, 7), synth.stereo_frame(0)[0])
    assert len(wk) >= 1000 and np.array_equal(got["kps"], wk.astype(KEYPOINT_DTYPE)) and np.array_equal(got["desc"], wd)
    p = orc.orb_params(F["nfeat"], 1.2, F["levels"], 20, 7)
    total = 0
    for i in range(F["batch"]):
        wk, wd = orc.orb_detect(p, synth.stereo_frame(500 + i, F["w"], F["h"], n_rects=40)[0])
        n = int(got["n"][i])
        assert n == len(wk), f"image {i}"
        assert np.array_equal(got["bkps"][i, :n], wk.astype(KEYPOINT_DTYPE)) and np.array_equal(got["bdesc"][i, :n], wd), f"image {i}"
        total += n
    assert total > 16 * 50
