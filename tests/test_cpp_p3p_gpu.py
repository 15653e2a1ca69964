"""GPU: snake_hip::P3PRansac of the C++ adaptor header (snake_slam_amd/cpp/snake_hip.hpp) built into a small driver
(tests/cpp/p3p_driver.cpp, plain g++) and EXECUTED: `solve(wps, ips, pose, inlierMatches, inlierMask)` must return, byte for byte,
what the Python mirror returns from the same library."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import p3p_numpy as P

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def build_driver(out_dir: Path) -> Path:
    lib = ROOT / "snake_slam_amd" / "lib"
    exe = out_dir / "p3p_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", f"-I{ROOT / 'snake_slam_amd' / 'cpp'}",
           str(ROOT / "tests" / "cpp" / "p3p_driver.cpp"), f"-L{lib}", "-lsnake_hip", "-L/opt/rocm/lib", "-lamdhip64",
           f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_cpp_p3p_solve_equals_the_python_mirror(tmp_path):
    from snake_slam_amd.tracking import P3PRansac

    c = P.make_case(200, 0.3, 1.0, 4242)
    seed = 123456789
    c["wps"].tofile(tmp_path / "wps.bin")
    c["nips"].tofile(tmp_path / "nips.bin")
    np.array([250.0, c["threshold"], float(seed)]).tofile(tmp_path / "params.bin")
    exe = build_driver(tmp_path)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    s = P3PRansac(250, c["threshold"], seed)
    try:
        inliers, pose, matches, mask = s.solve(c["wps"], c["nips"])
        best = s.solve_batch([dict(wps=c["wps"], nips=c["nips"])])[0]["best"]
    finally:
        s.close()
    meta = np.fromfile(tmp_path / "out_meta.bin", np.int32)
    assert list(meta) == [inliers, *best] and inliers > 100
    assert np.fromfile(tmp_path / "out_pose.bin", np.float64).tobytes() == pose.tobytes()
    assert np.fromfile(tmp_path / "out_mask.bin", np.uint8).tobytes() == mask.tobytes()
    assert np.fromfile(tmp_path / "out_matches.bin", np.int32).tobytes() == matches.tobytes()
