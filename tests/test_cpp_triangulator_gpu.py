"""GPU: snake_hip::Triangulator of the C++ adaptor header (snake_slam_amd/cpp/snake_hip.hpp) built into a small driver
(tests/cpp/triangulator_driver.cpp, plain g++) and EXECUTED on a synthetic case: Process over ten neighbours and triangulate per
keyframe pair must return, byte for byte, what the Python mirror returns from the same library, and agree with the numpy restatement."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import tri_numpy as T
from test_triangulate_gpu import check_against_restatement, make_triangulator, restate

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def build_driver(out_dir: Path) -> Path:
    lib = ROOT / "snake_slam_amd" / "lib"
    exe = out_dir / "triangulator_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", f"-I{ROOT / 'snake_slam_amd' / 'cpp'}",
           str(ROOT / "tests" / "cpp" / "triangulator_driver.cpp"), f"-L{lib}", "-lsnake_hip", "-L/opt/rocm/lib", "-lamdhip64",
           f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_cpp_triangulator_equals_the_python_mirror(tmp_path):
    seed, n_nb, mode = T.CASES[1]
    c = T.make_case(seed, n_nb, mode)
    put = lambda name, a: np.ascontiguousarray(a).tofile(tmp_path / f"{name}.bin")
    put("cam", np.array([*c["cam"], c["params"]["th_depth"]], np.float64))
    put("ls", c["level_scale"])
    put("meta", np.array([n_nb, c["params"]["mono"]], np.int32))
    for tag, kf in [("kf1", c["kf1"])] + [(f"kf2_{k}", k2) for k, k2 in enumerate(c["kf2s"])]:
        put(tag + "_kps", kf["kps"]), put(tag + "_rp", kf["right_points"]), put(tag + "_depth", kf["depth"]), put(tag + "_has", kf["has_mp"])
        put(tag + "_pose", np.concatenate([kf["pose"], [float(kf["median_depth"])]]))
    for k, p in enumerate(c["pairs"]):
        put(f"pairs_{k}", p)
    exe = build_driver(tmp_path)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    pts = np.fromfile(tmp_path / "out_points.bin", T.NEW_POINT)
    counts = np.fromfile(tmp_path / "out_counts.bin", np.int32)
    singles = np.fromfile(tmp_path / "out_singles.bin", T.NEW_POINT)
    tri = make_triangulator(c)
    try:
        nnew, want, out_start = tri.Process(c["kf1"], c["kf2s"], c["pairs"], c["median_depth2s"])
        want_singles = np.concatenate([tri.triangulate(c["kf1"], k2, p, m) for k2, p, m in zip(c["kf2s"], c["pairs"], c["median_depth2s"])])
    finally:
        tri.close()
    assert counts[0] == nnew > 0 and list(counts[1:]) == list(np.diff(out_start))
    assert pts.tobytes() == want.tobytes() and singles.tobytes() == want_singles.tobytes()
    worst, _ = check_against_restatement(c, restate(c), pts, out_start)
    assert worst <= T.position_tolerance()
