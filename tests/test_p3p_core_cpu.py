"""CPU: p3p_core.hpp -- the statements the kernel runs -- built with plain g++ (no contraction) and executed on the cases of the GPU
test: the sampler's triplets equal the numpy restatement's exactly, and so do the slot masks and the poses, bit for bit (both are
sequences of the same IEEE + - * / and sqrt).  This is the claim "two implementations of one text" checked without a GPU."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import p3p_numpy as P

ROOT = Path(__file__).resolve().parent.parent
CASES = P.gpu_cases()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("p3p_core") / "p3p_core_driver"
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", f"-I{ROOT / 'snake_slam_amd' / 'csrc'}",
           str(ROOT / "tests" / "cpp" / "p3p_core_driver.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("c", CASES[::3], ids=[c["name"] for c in CASES[::3]])
def test_cpu_build_of_the_core_equals_the_restatement(driver, tmp_path, c):
    seed, problem = c["seed"] & 0xFFFFFFFF, 3  # a seed a double carries exactly
    c["wps"].tofile(tmp_path / "wps.bin")
    c["nips"].tofile(tmp_path / "nips.bin")
    np.array([250.0, float(seed), float(problem)]).tofile(tmp_path / "params.bin")
    r = subprocess.run([str(driver), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    tri = np.fromfile(tmp_path / "out_tri.bin", np.int32).reshape(-1, 3)
    valid = np.fromfile(tmp_path / "out_valid.bin", np.int32)
    poses = np.fromfile(tmp_path / "out_poses.bin", np.float64).reshape(-1, 4, 12)
    want_tri = P.triplets(seed, problem, 250, len(c["wps"]))
    assert np.array_equal(tri, want_tri)
    R, t, v = P.solve(c["wps"][want_tri], c["nips"][want_tri])
    assert np.array_equal(valid, (v * (1 << np.arange(4))).sum(1))
    assert np.array_equal(poses[..., :9], R) and np.array_equal(poses[..., 9:], t)
