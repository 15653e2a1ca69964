"""GPU: snake_hip::RegistrationRansac of the C++ adaptor header (snake_slam_amd/cpp/snake_hip.hpp) built into a small driver
(tests/cpp/sim3_driver.cpp, plain g++) and EXECUTED: filled and called as LoopDetector::solve does, `solver.solve(its, compute_scale)`
must return, byte for byte, what the Python mirror returns from the same library."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sim3_numpy as S

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def build_driver(out_dir: Path) -> Path:
    lib = ROOT / "snake_slam_amd" / "lib"
    exe = out_dir / "sim3_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", f"-I{ROOT / 'snake_slam_amd' / 'cpp'}",
           str(ROOT / "tests" / "cpp" / "sim3_driver.cpp"), f"-L{lib}", "-lsnake_hip", "-L/opt/rocm/lib", "-lamdhip64",
           f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_cpp_sim3_solve_equals_the_python_mirror(tmp_path):
    from snake_slam_amd.loop import RegistrationRansac

    c = S.make_case(200, 0.3, 1.0, True, 0, 4242)
    seed = 123456789
    for name, key in (("p1", "P1"), ("p2", "P2"), ("ip1", "ip1"), ("ip2", "ip2")):
        c[key].tofile(tmp_path / f"{name}.bin")
    np.array([0.0, 1.0, c["threshold"], float(seed), *S.CAM]).tofile(tmp_path / "params.bin")
    exe = build_driver(tmp_path)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    s = RegistrationRansac(S.CAM, c["threshold"], 0, True, seed)
    try:
        res = s.solve_batch([dict(points1=c["P1"], points2=c["P2"], ips1=c["ip1"], ips2=c["ip2"])])[0]
    finally:
        s.close()
    meta = np.fromfile(tmp_path / "out_meta.bin", np.int32)
    assert list(meta) == [res["inliers"], res["best"], S.ransac_iterations(200)] and res["inliers"] > 100
    assert np.fromfile(tmp_path / "out_T.bin", np.float64).tobytes() == np.concatenate([res["T"], [res["scale"]]]).tobytes()
    assert np.fromfile(tmp_path / "out_mask.bin", np.uint8).tobytes() == res["mask"].tobytes()
