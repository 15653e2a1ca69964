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
"""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
NT_MAX = (1 << 20) - 2  # documented maximum of the train set: the index field of the packed key holds 20 bits, all ones = "none"
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
]

# the values of the enums of dispatch.hpp (the CPU test reads the header and compares)
ENUMS = {"Knn2Form": ["vector1", "vector4", "mfma"], "StereoForm": ["frame", "count16", "sort16", "unindexed"],
         "PoseForm": ["wave1", "wave2_lds", "wave4_lds", "wave4_global"],
         "BaLinForm": ["fused3", "fused3_sums", "fused4", "point_wave", "point_pass"],
         "BaCamForm": ["none", "cam_sum", "cam64_xcd", "cam64_2d", "cam256"],
         "BaSchurForm": ["none", "in_fused", "mfma32", "mfma33", "mfma43", "set42", "set63", "pass4", "pass1"],
         "BaPcgForm": ["none", "small", "solve_lds", "solve_global", "persist_reg16", "persist_reg8", "persist1", "persist", "launches", "imp_persist",
                       "imp_launches"],
         "BaUpdateForm": ["update_cost", "update_wave", "update_point"]}
# the enum of an entry's form; an entry whose form is "a/b/..." names one enum per part
ENUM_OF = {"knn2": "Knn2Form", "stereo_host": "StereoForm", "stereo_batch": "StereoForm", "pose_host": "PoseForm", "pose_batch": "PoseForm",
           "ba_lm": ("BaLinForm", "BaCamForm", "BaSchurForm", "BaPcgForm", "BaUpdateForm")}
# forms that no shape selects (test_match_forms_gpu.py / test_pose_forms_gpu.py run each once in a child process under its switch;
# the BA forms: the rows of tests/test_zy_ba_variants_gpu.py)
ENV_ONLY = {("PoseForm", "wave4_global"), ("StereoForm", "sort16"),
            ("BaLinForm", "fused3_sums"), ("BaLinForm", "fused4"), ("BaCamForm", "cam_sum"), ("BaCamForm", "cam64_2d"), ("BaSchurForm", "mfma32"),
            ("BaSchurForm", "mfma33"), ("BaSchurForm", "set42"), ("BaSchurForm", "set63"), ("BaPcgForm", "solve_lds")}


def parts(entry, form):
    """(enum, value) for every part of an entry's form."""
    enums = ENUM_OF[entry]
    return [(enums, form)] if isinstance(enums, str) else list(zip(enums, form.split("/"), strict=True))


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


def shapes(entry, form):
    """Every shape of the table that `entry` maps to `form`, in table order."""
    return [s for e, s, f in FORMS if e == entry and f == form]


def shape(entry, wanted, form):
    """`wanted` if the table pins it to `form` -- the GPU tests pass every launch shape through here."""
    assert (entry, tuple(wanted), form) in FORMS, f"{entry}{tuple(wanted)} -> {form} is not a row of tests/forms.py"
    return tuple(wanted)


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
