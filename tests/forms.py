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
"""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
NT_MAX = (1 << 20) - 2  # documented maximum of the train set: the index field of the packed key holds 20 bits, all ones = "none"
N_CU = 256              # compute units of an MI355X; no row below is within reach of the batch > 2 * n_cu rule except the one that names it

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
]

# the values of the enums of dispatch.hpp (the CPU test reads the header and compares)
ENUMS = {"Knn2Form": ["vector1", "vector4", "mfma"], "StereoForm": ["frame", "count16", "sort16", "unindexed"],
         "PoseForm": ["wave1", "wave2_lds", "wave4_lds", "wave4_global"]}
ENUM_OF = {"knn2": "Knn2Form", "stereo_host": "StereoForm", "stereo_batch": "StereoForm", "pose_host": "PoseForm", "pose_batch": "PoseForm"}
# forms that no shape selects (test_match_forms_gpu.py / test_pose_forms_gpu.py run each once in a child process under its switch)
ENV_ONLY = {("PoseForm", "wave4_global"), ("StereoForm", "sort16")}


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
