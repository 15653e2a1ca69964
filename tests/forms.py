"""The launch shapes of the kernel-form tests and the form each was written for: one table, read by the CPU test
(tests/test_cpp_dispatch.py asserts every row against snake_slam_amd/csrc/dispatch.hpp, built with plain g++) and by the GPU tests
(test_match_forms_gpu.py, test_pose_forms_gpu.py take their shapes from it through `shape` / `shapes`).  A threshold that moves in
dispatch.hpp fails the CPU test; a GPU test cannot use a shape that the table does not pin to a form.

A row is (entry, shape, form).  entry names a function of dispatch.hpp, shape is its argument tuple (switches as 0 / 1):
  knn2          (nq_cap, nt_cap, batch, no_mfma)             the host entry calls it with (nq, max(nt, 1), 1, .)
  stereo_host   (nr, sort_network)
  stereo_batch  (nr_cap, batch, no_frame_kernel, sort_network)
  pose_host     (total matches, n_problems, no_lds)
  pose_batch    (stride, batch, n_cu, waves_env, no_lds)     stride = cap (frame form) or pts_cap (matches form)
  ba_lm         ba(...): the fields of BaShape, `recording`, and the switches as one string -- the five forms of an LM iteration of
                the BA solver, "linearisation/camera pass/Schur complement/PCG/update and cost"
  orb_band      (n_strips, h, batch, bh_env)                 a level pass of the extractor: rows per band of level_kernel
  orb_fast      (quads, cpw)                                 fast_kernel<NQ, LOOP>
  orb_harris    (total_cells, harris, per_cell)              harris: "orb.response" = 1
  orb_dist      (n_levels, batch, level_cap, harris)
  orb_desc      (switches,)                                  the extractor's switches as one string ("NAME=VALUE,..." without SNK_ORB_)
  orb_sched     (batch, parts, stagger, split_min_batch, one_stream)   parts / stagger: the handle's (snk_orb_set_chains / _set_stagger)
  orb_plan      orb(...): an extractor's configuration, a launch chain and the switches -- "levels;cpw/quads;harris;dist;desc", the
                fields of run_part's plan line (a level: rows per band, "r" resize_kernel first, "t" tiny, "u" unaligned, "+" also
                writes level l + 1, "-" no pixels)
  track_form    (pts_cap, batch, cap, ncell1, no_frame_lds, ppw_env)   a batched projection matcher
  track_launch  (pts_cap, batch, cap, ncell1, no_frame_lds, frame_wgs, no_fused_resolve, ppw_env)   the whole plan of a batched projection
                matcher, "form/workgroups per frame/resolution" as its plan line names them (tests/test_track_forms_gpu.py)
  grid_form     (cap, ncell, network_env)                    the feature grid: counting form or bitonic network
"""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
NT_MAX = (1 << 20) - 2  # documented maximum of the train set: the index field of the packed key holds 20 bits, all ones = "none"
NCELL1 = 40 * 26 + 1    # cells + 1 of the 20-pixel grid over track_helpers.BOUNDS
N_CU = 256              # compute units of an MI355X; no row below is within reach of the batch > 2 * n_cu rule except the one that names it

# ---- bundle adjustment: a shape is BaShape's fields in this order, then `recording`, then the switches ("NAME=VALUE,..." without SNK_BA_)
BA_FIELDS = ("B", "imp", "n6", "nfc", "np", "ni", "wv", "rpc", "items", "set_ok", "small", "k", "run", "wave_ok", "sums_ok", "blk", "pwgs", "pone",
             "prows", "rec")
# every switch of BaSwitches (dispatch.hpp), as the environment names it
BA_SWITCHES = ["PCG_GENERAL", "NO_POINT_WAVE", "NO_SCHUR_SET", "SCHUR_SET_MIN_ITEMS", "NO_SCHUR_MFMA", "NO_SCHUR_FUSED", "FUSED_K10", "CAM_SUMS",
               "CAM_GRID_2D", "NO_SCHUR_WIDE", "PCG_LDS", "NO_UPDATE_COST", "FLAT_BARRIER", "PCG_TIMING", "PCGL_LAUNCHES", "PERSIST_TWO_BARRIERS",
               "PERSIST_STREAM", "PERSIST_WGS", "PERSIST_REG_ROWS", "PERSIST_FAIL", "GRAPH_CHAINS", "NO_GRAPH", "GRAPH_FIRST", "LOCAL_SYNC"]


def ba(sw="", **kw):
    """A BA shape.  Defaults: one window of 3 free cameras and 10 points as the hand-over describes it (no point-major lists for a
    single small window, point_wave's lists built); n6 = 6 * nfc unless given."""
    d = dict(B=1, imp=0, nfc=3, np=10, ni=4, wv=10, rpc=0, items=0, set_ok=0, small=1, k=3, run=4, wave_ok=1, sums_ok=1, blk=1, pwgs=0, pone=0,
             prows=0, rec=0)
    d.update(kw)
    d.setdefault("n6", 6 * d["nfc"])
    return tuple(d[f] for f in BA_FIELDS) + (sw,)


SETS = dict(set_ok=1, items=2)   # what a hand-over of >= 8 windows adds: the point-major work items
SETS_ON = "SCHUR_SET_MIN_ITEMS=1"
GLOBAL = dict(nfc=299, np=9000, ni=300, wv=9000)  # a 300-keyframe global scene: the multi-workgroup PCG

# ---- ORB extractor: a configuration (OrbParams' fields the geometry depends on), a launch chain, the switches
ORB_FIELDS = ("w", "h", "nfeat", "levels", "scale", "cap", "batch", "aligned", "harris", "stages")
# every switch of OrbSwitches (dispatch.hpp), as the environment names it
ORB_SWITCHES = ["BALANCED_STRIPS", "FAST_SURV_CAP", "PARTS", "STAGGER", "BLUR_IN_DESCRIBE", "BLUR_TILED", "DESC_NO_DMA", "DESC_FAKE", "UNFUSED",
                "LEVEL_BH", "FAST_CPW", "FAST_STOP", "FAST_LDS_WG", "DIST_TIMING", "DIST_KEY_LOOP", "HARRIS_PER_CELL", "ONE_STREAM"]
TRACK_SWITCHES = ["NO_FRAME_LDS", "FRAME_WGS", "NO_FUSED_RESOLVE", "PPW"]


def orb(sw="", **kw):
    """An extractor launch chain.  Defaults: one aligned 752 x 480 image, 1000 features on 4 levels of 1.2 (the EuRoC configuration), FAST
    score as the response, both halves of the chain."""
    d = dict(w=752, h=480, nfeat=1000, levels=4, scale=1.2, cap=0, batch=1, aligned=1, harris=0, stages=3)
    d.update(kw)
    return tuple(d[f] for f in ORB_FIELDS) + (sw,)


KITTI = dict(w=1241, h=376, nfeat=2000, levels=8)

FORMS = [
    # ---- kNN-2: vector4 needs batch * nq_cap >= 16384 AND (nq_cap < 24 OR nt_cap < 24)
    ("knn2", (256, 23, 64, 0), "vector4"),        # 16384 exactly
    ("knn2", (255, 23, 64, 0), "vector1"),        # 16320
    ("knn2", (15, 1000, 1100, 0), "vector4"),     # the other side of the ||: few queries, many trains
    ("knn2", (23, 24, 1, 0), "vector1"),
    ("knn2", (24, 23, 1, 0), "vector1"),
    ("knn2", (24, 24, 1, 0), "mfma"),
    ("knn2", (24, 25, 1, 0), "mfma"),
    ("knn2", (129, 65, 9, 0), "mfma"),
    ("knn2", (8, 70, 1, 0), "vector1"),           # distance 255 against 256
    ("knn2", (40, 70, 1, 0), "mfma"),
    ("knn2", (3, NT_MAX, 1, 0), "vector1"),       # index field
    ("knn2", (32, NT_MAX, 1, 0), "mfma"),
    ("knn2", (1000, 1000, 24, 0), "mfma"),        # test_match_gpu.py::test_bf_batch_dev_parity
    # ---- stereo, batched entry
    ("stereo_batch", (2560, 8, 0, 0), "frame"),
    ("stereo_batch", (2561, 8, 0, 0), "count16"),
    ("stereo_batch", (2560, 7, 0, 0), "count16"),
    ("stereo_batch", (8192, 2, 0, 0), "count16"),
    ("stereo_batch", (8193, 2, 0, 0), "unindexed"),
    ("stereo_batch", (400, 8, 0, 0), "frame"),    # rows beyond the frame form's 2048 buckets
    ("stereo_batch", (2000, 3, 0, 0), "count16"),  # the counting index at the end of its table
    ("stereo_batch", (400, 8, 0, 1), "frame"),    # SNK_STEREO_SORT_NETWORK alone does not displace the frame form ...
    ("stereo_batch", (400, 8, 1, 1), "sort16"),   # ... together with SNK_STEREO_NO_FRAME_KERNEL it selects the network
    # ---- stereo, host entry
    ("stereo_host", (400, 0), "count16"),
    ("stereo_host", (2000, 0), "count16"),
    ("stereo_host", (8192, 0), "count16"),
    ("stereo_host", (9000, 0), "unindexed"),      # test_match_gpu.py::test_stereo_parity
    # ---- pose, host entry: four wavefronts from 192 matches per problem on average
    ("pose_host", (192 + 192, 2, 0), "wave4_lds"),
    ("pose_host", (192 + 191, 2, 0), "wave1"),
    ("pose_host", (1500 + 256 * 200, 257, 0), "wave4_lds"),  # more than 256 problems: the two-per-CU carve
    ("pose_host", (1500 + 255 * 200, 256, 0), "wave4_lds"),
    ("pose_host", (300, 1, 1), "wave4_global"),   # SNK_POSE_NO_LDS
    # ---- pose, batched entries
    ("pose_batch", (255, 5, N_CU, 0, 0), "wave1"),
    ("pose_batch", (256, 5, N_CU, 0, 0), "wave4_lds"),
    ("pose_batch", (700, 5, N_CU, 0, 0), "wave4_lds"),       # test_tracking_chain_gpu.py, the frame form at cap 700
    ("pose_batch", (256, 2 * N_CU + 1, N_CU, 0, 0), "wave2_lds"),
    ("pose_batch", (256, 2 * N_CU, N_CU, 0, 0), "wave4_lds"),
    ("pose_batch", (256, 5, N_CU, 0, 1), "wave4_global"),    # SNK_POSE_NO_LDS
    # ---- BA, the default path of the five scenes of test_ba_gpu.py::test_lm_plan_lines_name_the_forms_that_ran
    # (the shapes are what the hand-over reports for those scenes: the plan lines of a run under SNK_DEBUG=1)
    ("ba_lm", ba(nfc=2, ni=3, wv=1, k=0, run=0), "point_wave/cam256/pass4/small/update_wave"),                      # one window of 3 keyframes x 10 points
    ("ba_lm", ba(nfc=19, np=400, ni=20, wv=34, k=0, run=0), "point_wave/cam256/pass4/small/update_wave"),           # one window of 20 keyframes
    ("ba_lm", ba(B=16, nfc=2, ni=3, wv=1, set_ok=1, items=3, k=2, run=2), "point_wave/cam64_xcd/pass1/small/update_wave"),   # 16 windows: 48 work items < 256
    ("ba_lm", ba(B=256, nfc=2, ni=3, wv=1, set_ok=1, items=3, k=2, run=2, blk=0), "fused3/cam64_xcd/in_fused/small/update_cost"),  # 256 windows: the point-major pass, no block lists
    ("ba_lm", ba(nfc=29, np=900, ni=30, wv=75, k=0, run=0, pwgs=22, pone=2, prows=8), "point_wave/cam256/pass4/persist_reg8/update_wave"),  # "large": 30 keyframes
    # ---- BA, the other forms a shape selects
    ("ba_lm", ba(B=256, k=9, run=10, **SETS), "point_wave/cam64_xcd/mfma43/small/update_cost"),   # points with 9-10 free observations
    ("ba_lm", ba(wave_ok=0), "point_pass/cam256/pass4/small/update_point"),                       # a point with > 64 observations
    ("ba_lm", ba(nfc=0), "point_wave/none/none/none/update_wave"),                                # every camera constant
    ("ba_lm", ba(nfc=22), "point_wave/cam256/pass4/solve_global/update_wave"),                    # S leaves the registers, not yet LDS-resident
    ("ba_lm", ba(nfc=100), "point_wave/cam256/pass1/launches/update_wave"),                       # 10 000 blocks > 8192; no cooperative launch
    ("ba_lm", ba(pwgs=113, pone=2, prows=16, **GLOBAL), "point_wave/cam256/pass1/persist_reg16/update_wave"),
    ("ba_lm", ba(pwgs=150, pone=1, **GLOBAL), "point_wave/cam256/pass1/persist1/update_wave"),
    ("ba_lm", ba(pwgs=150, pone=0, **GLOBAL), "point_wave/cam256/pass1/persist/update_wave"),
    ("ba_lm", ba(B=2, pwgs=150, pone=1, **GLOBAL), "point_wave/cam256/pass1/launches/update_wave"),  # a batch of large problems
    ("ba_lm", ba(imp=1, pwgs=40, **GLOBAL), "point_wave/cam256/none/imp_persist/update_wave"),
    ("ba_lm", ba(imp=1, pwgs=0, **GLOBAL), "point_wave/cam256/none/imp_launches/update_wave"),
    ("ba_lm", ba(imp=1, pwgs=40, rec=1, **GLOBAL), "point_wave/cam256/none/imp_launches/update_wave"),  # a cooperative launch is no graph node
    # ---- BA, the switches of tests/test_zy_ba_variants_gpu.py on a shape that otherwise takes the default
    ("ba_lm", ba(SETS_ON, **SETS), "fused3/cam256/in_fused/small/update_cost"),
    ("ba_lm", ba("NO_SCHUR_SET", B=256, **SETS), "point_wave/cam64_xcd/pass1/small/update_wave"),
    ("ba_lm", ba("NO_POINT_WAVE", B=256, **SETS), "point_pass/cam64_xcd/pass1/small/update_point"),
    ("ba_lm", ba("PCG_GENERAL"), "point_wave/cam256/pass4/solve_lds/update_wave"),
    ("ba_lm", ba(SETS_ON + ",FUSED_K10", k=9, run=10, **SETS), "fused4/cam256/in_fused/small/update_cost"),
    ("ba_lm", ba(SETS_ON + ",NO_SCHUR_FUSED", **SETS), "point_wave/cam256/mfma32/small/update_cost"),
    ("ba_lm", ba(SETS_ON + ",NO_SCHUR_FUSED", run=14, **SETS), "point_wave/cam256/mfma33/small/update_cost"),  # 14 * 9 + 3 > 128: three tiles
    ("ba_lm", ba(SETS_ON + ",NO_SCHUR_FUSED", k=9, run=10, **SETS), "point_wave/cam256/mfma43/small/update_cost"),
    ("ba_lm", ba(SETS_ON + ",NO_SCHUR_MFMA", **SETS), "point_wave/cam256/set42/small/update_cost"),
    ("ba_lm", ba(SETS_ON + ",NO_SCHUR_MFMA", small=0, **SETS), "point_wave/cam256/set63/small/update_cost"),
    ("ba_lm", ba(SETS_ON + ",CAM_SUMS", **SETS), "fused3_sums/cam_sum/in_fused/small/update_cost"),
    ("ba_lm", ba(SETS_ON + ",CAM_SUMS", sums_ok=0, **SETS), "fused3/cam256/in_fused/small/update_cost"),  # a constant point seen by a free camera
    ("ba_lm", ba("CAM_GRID_2D", B=16), "point_wave/cam64_2d/pass1/small/update_wave"),
    ("ba_lm", ba("PCG_LDS"), "point_wave/cam256/pass4/solve_lds/update_wave"),
    ("ba_lm", ba("NO_SCHUR_WIDE,NO_SCHUR_SET"), "point_wave/cam256/pass1/small/update_wave"),
    ("ba_lm", ba("NO_UPDATE_COST", B=256, **SETS), "fused3/cam64_xcd/in_fused/small/update_wave"),
    ("ba_lm", ba("GRAPH_CHAINS=2,GRAPH_FIRST", B=256, rec=1, **SETS), "fused3/cam64_xcd/in_fused/small/update_cost"),
    # ---- ORB, level passes: 64 rows per band from 2048 strips x bands on, else 22 from 2048 on, else 8
    ("orb_band", (4, 480, 64, 0), "bh64"),        # 4 * 64 * ceil(480 / 64) = 2048 exactly
    ("orb_band", (4, 480, 24, 0), "bh22"),        # 96 * 8 = 768 < 2048 <= 96 * 22 = 2112
    ("orb_band", (4, 480, 1, 0), "bh8"),          # a per-frame call
    ("orb_band", (4, 480, 1, 22), "bh22"),        # SNK_ORB_LEVEL_BH
    # ---- ORB, FAST: the compile-time tile pitches of the layout and one cell per wavefront or a loop over cpw cells
    ("orb_fast", (3, 1), "single3"), ("orb_fast", (4, 1), "single4"), ("orb_fast", (0, 1), "single0"),
    ("orb_fast", (3, 8), "loop3"), ("orb_fast", (4, 2), "loop4"), ("orb_fast", (0, 8), "loop0"),
    ("orb_harris", (828, 0, 0), "none"), ("orb_harris", (828, 1, 0), "dense"), ("orb_harris", (0, 1, 0), "none"), ("orb_harris", (828, 1, 1), "per_cell"),
    # ---- ORB, distribution: one launch at the full carve up to 128 (image, level) workgroups
    ("orb_dist", (4, 32, 8192, 0), "one_full"),      # 128
    ("orb_dist", (3, 43, 8192, 0), "small_drain"),   # 129
    ("orb_dist", (4, 1, 8192, 1), "small_drain"),    # the Harris ranks do not fit beside the full carve
    ("orb_dist", (4, 1, 2048, 0), "one_small"),      # level_cap <= 2048: the small carve holds every level
    ("orb_dist", (4, 2048, 1024, 1), "one_small"),
    ("orb_dist", (4, 1, 4096, 0), "one_full"),
    # ---- ORB, descriptors
    ("orb_desc", ("",), "dma"),
    ("orb_desc", ("BLUR_IN_DESCRIBE",), "blur_in"),
    ("orb_desc", ("DESC_NO_DMA",), "registers"),
    ("orb_desc", ("BLUR_TILED",), "dma_tiled"),
    ("orb_desc", ("BLUR_TILED,DESC_NO_DMA",), "registers"),   # the tiled planes need the DMA path: row-major
    ("orb_desc", ("BLUR_TILED,DESC_FAKE=1",), "dma"),
    # ---- ORB, launch chains of a batch
    ("orb_sched", (2048, 1, 0, 8, 0), "one_chain"),
    ("orb_sched", (2048, 2, 0, 8, 0), "chains"),
    ("orb_sched", (7, 2, 0, 8, 0), "one_chain"),     # below split_min_batch
    ("orb_sched", (64, 1, 4, 8, 0), "staggered"),
    ("orb_sched", (8, 1, 5, 8, 0), "one_chain"),     # fewer than two images per part
    ("orb_sched", (2048, 2, 4, 8, 1), "one_chain"),  # SNK_ORB_ONE_STREAM
    # ---- ORB, whole chains: the two calls of tests/test_orb_plan_gpu.py, the benchmark's batch, and the paths a configuration selects
    ("orb_plan", orb(), "8+,8+,8+,8;1/3;none;one_full;dma"),                                          # snk_orb_detect on one 752 x 480 image
    ("orb_plan", orb(w=160, h=120, nfeat=500, batch=16), "8+,8+,8+,8;1/4;none;one_full;dma"),         # 16 images of 160 x 120: 40-pixel cells on level 2, 64 workgroups
    ("orb_plan", orb(batch=2048), "64+,64+,64+,64;8/3;none;small_drain;dma"),
    ("orb_plan", orb(batch=2048, aligned=0), "64u+,64+,64+,64;8/3;none;small_drain;dma"),
    ("orb_plan", orb(batch=64, harris=1, **KITTI), "64+,22+,22+,22+,8+,8+,8+,8;2/3;dense;small_drain;dma"),   # 7 * 64 strips x 6 bands = 2688 on level 0
    ("orb_plan", orb(scale=2.5), "8,r8,r8,r8;1/4;none;one_full;dma"),                                 # scale factor > 2: stand-alone resize_kernel
    ("orb_plan", orb("UNFUSED"), "8,r8,r8,r8;1/3;none;one_full;dma"),
    ("orb_plan", orb(w=40, h=40, nfeat=500, levels=16), "8+,8+,8+,8+,8+,8+,8+,8+,8+,8+,t,rt,rt,rt,rt,rt;0/0;none;one_full;dma"),  # tiny levels, no cells
    ("orb_plan", orb(w=40, h=40, nfeat=500, levels=16, scale=2.0), "8+,8+,8+,t,rt,rt,rt,-,-,-,-,-,-,-,-,-;0/0;none;one_full;dma"),  # 40, 20, 10, 5, 2, 1, 1, then levels scaled to nothing
    # ---- projection matchers, batched: the frame in LDS from 64 points per wavefront on (8192 * 64 points in the call)
    ("track_form", (512, 1024, 1000, 2401, 0, 0), "frame"),   # 524288 points
    ("track_form", (512, 1023, 1000, 2401, 0, 0), "batch"),
    ("track_form", (10000, 1024, 2258, 2401, 0, 0), "frame"),  # 147428 bytes of LDS ...
    ("track_form", (10000, 1024, 2259, 2401, 0, 0), "batch"),  # ... 147492 > 144 KB = 147456
    ("track_form", (512, 1024, 1000, 2401, 1, 0), "batch"),   # SNK_TRACK_NO_FRAME_LDS
    ("track_form", (512, 8, 1000, 2401, 0, 64), "frame"),     # SNK_TRACK_PPW=64
    # ---- the whole plan, on the 40 x 26 grid of track_helpers.BOUNDS.  512 frames: the edge of 64 points per wavefront by size alone
    ("track_launch", (1024, 512, 333, NCELL1, 0, 0, 0, 0), "frame/1/fused"),   # 524288 points, one chunk
    ("track_launch", (1023, 512, 333, NCELL1, 0, 0, 0, 0), "batch/0/lds"),     # 523776 points: 63 per wavefront
    ("track_launch", (2048, 512, 333, NCELL1, 0, 0, 0, 0), "frame/2/lds"),     # two chunks, two workgroups per frame: no fused resolution
    # the LDS limits (SNK_TRACK_PPW=64, one workgroup per frame): frame + claims end at 147452 of 147456 bytes, frame alone at 147412
    ("track_launch", (2049, 7, 2203, NCELL1, 0, 1, 0, 64), "frame/1/fused"),
    ("track_launch", (2049, 7, 2204, NCELL1, 0, 1, 0, 64), "frame/1/lds"),
    ("track_launch", (2049, 7, 2347, NCELL1, 0, 1, 0, 64), "frame/1/lds"),
    ("track_launch", (2049, 7, 2348, NCELL1, 0, 1, 0, 64), "batch/0/lds"),
    ("track_launch", (2049, 7, 2203, NCELL1, 0, 2, 0, 64), "frame/2/lds"),     # three chunks on two workgroups
    # the separate resolution: claims in LDS up to 32768 features
    ("track_launch", (1200, 3, 32768, NCELL1, 0, 0, 0, 0), "batch/0/lds"),
    ("track_launch", (1200, 3, 32769, NCELL1, 0, 0, 0, 0), "batch/0/global"),
    ("track_launch", (300, 4, 400, NCELL1, 0, 0, 0, 0), "batch/0/lds"),       # counts out of range in the default form of a small call
    # ---- feature grid: the counting form while 2 (ncell + 1) + 2 cap ints fit 96 KB
    ("grid_form", (11247, NCELL1 - 1, 0), "count"),   # 98304 bytes exactly
    ("grid_form", (11248, NCELL1 - 1, 0), "network"),
    ("grid_form", (16384, NCELL1 - 1, 0), "network"),  # the documented maximum
    ("grid_form", (287, 12000, 0), "count"),          # 120 x 100 cells
    ("grid_form", (288, 12000, 0), "network"),
    ("grid_form", (400, 65532, 0), "network"),        # 254 x 258 cells: the largest grid but two
    ("grid_form", (1100, NCELL1 - 1, 1), "network"),  # SNK_GRID_NETWORK (tests/test_zx_frontend_variants_gpu.py)
]

# the values of the enums of dispatch.hpp (the CPU test reads the header and compares)
ENUMS = {"Knn2Form": ["vector1", "vector4", "mfma"], "StereoForm": ["frame", "count16", "sort16", "unindexed"],
         "PoseForm": ["wave1", "wave2_lds", "wave4_lds", "wave4_global"],
         "BaLinForm": ["fused3", "fused3_sums", "fused4", "point_wave", "point_pass"],
         "BaCamForm": ["none", "cam_sum", "cam64_xcd", "cam64_2d", "cam256"],
         "BaSchurForm": ["none", "in_fused", "mfma32", "mfma33", "mfma43", "set42", "set63", "pass4", "pass1"],
         "BaPcgForm": ["none", "small", "solve_lds", "solve_global", "persist_reg16", "persist_reg8", "persist1", "persist", "launches", "imp_persist",
                       "imp_launches"],
         "BaUpdateForm": ["update_cost", "update_wave", "update_point"],
         "OrbBandForm": ["bh64", "bh22", "bh8"], "OrbFastForm": ["single0", "single3", "single4", "loop0", "loop3", "loop4"],
         "OrbHarrisForm": ["none", "per_cell", "dense"], "OrbDistForm": ["one_full", "one_small", "small_drain"],
         "OrbDescForm": ["registers", "blur_in", "dma", "dma_tiled"], "OrbSchedule": ["one_chain", "chains", "staggered"],
         "TrackForm": ["frame", "batch"], "TrackResolve": ["fused", "lds", "global"], "GridForm": ["count", "network"]}
# the enum of an entry's form; an entry whose form is "a/b/..." names one enum per part
ENUM_OF = {"knn2": "Knn2Form", "stereo_host": "StereoForm", "stereo_batch": "StereoForm", "pose_host": "PoseForm", "pose_batch": "PoseForm",
           "ba_lm": ("BaLinForm", "BaCamForm", "BaSchurForm", "BaPcgForm", "BaUpdateForm"),
           "orb_band": "OrbBandForm", "orb_fast": "OrbFastForm", "orb_harris": "OrbHarrisForm", "orb_dist": "OrbDistForm", "orb_desc": "OrbDescForm",
           "orb_sched": "OrbSchedule", "orb_plan": (None, None, "OrbHarrisForm", "OrbDistForm", "OrbDescForm"), "track_form": "TrackForm",
           "track_launch": ("TrackForm", None, "TrackResolve"), "grid_form": "GridForm"}
# forms that no shape selects (test_match_forms_gpu.py / test_pose_forms_gpu.py run each once in a child process under its switch;
# the BA forms: the rows of tests/test_zy_ba_variants_gpu.py)
ENV_ONLY = {("PoseForm", "wave4_global"), ("StereoForm", "sort16"),
            ("BaLinForm", "fused3_sums"), ("BaLinForm", "fused4"), ("BaCamForm", "cam_sum"), ("BaCamForm", "cam64_2d"), ("BaSchurForm", "mfma32"),
            ("BaSchurForm", "mfma33"), ("BaSchurForm", "set42"), ("BaSchurForm", "set63"), ("BaPcgForm", "solve_lds"),
            # the extractor: tests/test_zx_frontend_variants_gpu.py and test_orb_gpu.py run each under its switch
            ("OrbHarrisForm", "per_cell"), ("OrbDescForm", "registers"), ("OrbDescForm", "blur_in"), ("OrbDescForm", "dma_tiled")}


def parts(entry, form):
    """(enum, value) for every part of an entry's form."""
    enums = ENUM_OF[entry]
    if isinstance(enums, str):
        return [(enums, form)]
    # "a/b/..." names one enum per part; the extractor's "levels;cpw/quads;a;b;c" has two parts that are no enum (None), and so has the
    # workgroup count of "form/wgs/resolve"
    return [(e, v) for e, v in zip(enums, form.split(";" if entry == "orb_plan" else "/"), strict=True) if e is not None]


def ba_env_switches(environ):
    """The BA switches of an environment as the `switches` argument of the driver's ba_* entries."""
    sw = [f"{n}={environ['SNK_BA_' + n] or 0}" for n in BA_SWITCHES if "SNK_BA_" + n in environ]
    return ",".join(sw + (["DEBUG"] if "SNK_DEBUG" in environ else []))


def ba_plan_lines(stderr):
    """The plan lines of enqueue_lm under SNK_DEBUG ("snake_hip: ba lm B=... lin=... chains=n"), each as (driver query for ba_lm
    without the switches, "lin/cam/schur/pcg/update")."""
    out = []
    for ln in stderr.splitlines():
        if not ln.startswith("snake_hip: ba lm "):
            continue
        kv = dict(re.findall(r"(\w+)=(\S+)", ln))
        out.append((tuple(int(kv[f]) for f in BA_FIELDS), "/".join(kv[k] for k in ("lin", "cam", "schur", "pcg", "update"))))
    return out


def orb_env_switches(environ):
    """The extractor's switches of an environment as the `switches` argument of the driver's orb_* entries."""
    return ",".join(f"{n}={environ['SNK_ORB_' + n] or 0}" for n in ORB_SWITCHES if "SNK_ORB_" + n in environ)


def orb_plan_lines(stderr):
    """The plan lines of run_part under SNK_DEBUG ("snake_hip: orb plan w=... desc=..."), each as (driver query for orb_plan without the
    switches, "levels;cpw/quads;harris;dist;desc")."""
    import numpy as np

    out = []
    for ln in stderr.splitlines():
        if not ln.startswith("snake_hip: orb plan "):
            continue
        kv = dict(re.findall(r"(\w+)=(\S+)", ln))
        # the scale factor is printed with nine digits (the float itself): back to its shortest decimal, 1.20000005 -> 1.2
        out.append((tuple(float(str(np.float32(kv[f]))) if f == "scale" else int(kv[f]) for f in ORB_FIELDS),
                    ";".join(kv[k] for k in ("level", "fast", "harris_form", "dist", "desc"))))
    return out


TRACK_LAUNCH_FIELDS = ("pts_cap", "batch", "cap", "ncell1")


def track_plan_lines(stderr):
    """The plan lines of the batched projection matchers under SNK_DEBUG ("snake_hip: track plan entry=... resolve=..."), each as
    (entry, (pts_cap, batch, cap, ncell1), ppw, "form/wgs/resolve")."""
    out = []
    for ln in stderr.splitlines():
        if not ln.startswith("snake_hip: track plan "):
            continue
        kv = dict(re.findall(r"(\w+)=(\S+)", ln))
        out.append((kv["entry"], tuple(int(kv[f]) for f in TRACK_LAUNCH_FIELDS), int(kv["ppw"]), "/".join(kv[k] for k in ("form", "wgs", "resolve"))))
    return out


def grid_plan_lines(stderr):
    """The plan lines of the feature grid under SNK_DEBUG ("snake_hip: grid plan cap=... form=..."), each as ((cap, ncell), batch, form)."""
    out = []
    for ln in stderr.splitlines():
        if not ln.startswith("snake_hip: grid plan "):
            continue
        kv = dict(re.findall(r"(\w+)=(\S+)", ln))
        out.append(((int(kv["cap"]), int(kv["ncell"])), int(kv["batch"]), kv["form"]))
    return out


def shapes(entry, form):
    """Every shape of the table that `entry` maps to `form`, in table order."""
    return [s for e, s, f in FORMS if e == entry and f == form]


def shape(entry, wanted, form):
    """`wanted` if the table pins it to `form` -- the GPU tests pass every launch shape through here."""
    assert (entry, tuple(wanted), form) in FORMS, f"{entry}{tuple(wanted)} -> {form} is not a row of tests/forms.py"
    return tuple(wanted)


def track_plan_edges(exe, pts_cap, batch, ncell1, frame_wgs, ppw_env, caps=range(1, 4001)):
    """(last capacity with the fused resolution, last capacity of the frame form) of a batched matcher's plan, found by asking the
    driver for every capacity of `caps`; each form must hold one unbroken range of capacities."""
    plans = ask(exe, [("track_launch", (pts_cap, batch, c, ncell1, 0, frame_wgs, 0, ppw_env)) for c in caps])
    kinds = [("fused" if p.endswith("/fused") else p.split("/")[0]) for p in plans]
    n_fused, n_frame = kinds.count("fused"), kinds.count("frame")
    assert kinds == ["fused"] * n_fused + ["frame"] * n_frame + ["batch"] * (len(kinds) - n_fused - n_frame) and n_fused and n_frame and kinds[-1] == "batch"
    return caps[n_fused - 1], caps[n_fused + n_frame - 1]


def grid_form_edge(exe, ncell, caps=range(1, 16385)):
    """The last capacity at which a grid of ncell cells takes the counting form."""
    got = ask(exe, [("grid_form", (c, ncell, 0)) for c in caps])
    n = got.count("count")
    assert got == ["count"] * n + ["network"] * (len(got) - n) and 0 < n < len(got)
    return caps[n - 1]


def build_driver(directory):
    """tests/cpp/dispatch_driver.cpp, plain g++ with -Wall -Werror; returns the executable."""
    exe = Path(directory) / "dispatch_driver"
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{ROOT / 'snake_slam_amd' / 'csrc'}", str(ROOT / "tests" / "cpp" / "dispatch_driver.cpp"),
           "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def ask(exe, queries):
    """One answer per (entry, args) query: the form's name, or the integer for the carve functions and `const`."""
    r = subprocess.run([str(exe)] + [":".join([e] + [str(a) for a in args]) for e, args in queries], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split()
    assert len(out) == len(queries)
    return out
