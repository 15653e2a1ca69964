"""CPU: sim3_core.hpp -- the statements the kernel runs -- built with plain g++ (no contraction) and executed on cases of the GPU
test: the sampler's triplets and the valid flags equal the numpy restatement's exactly, the transforms agree within
transform_tolerance() (both are sequences of the same IEEE + - * / and sqrt: the difference observed is printed), the inlier counts
are identical outside borderline hypotheses (the header's per-pair test uses fma), and the iteration count equals the restatement's
for every n up to the cap.  This is the claim "two implementations of one text" checked without a GPU."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sim3_numpy as S

ROOT = Path(__file__).resolve().parent.parent
CASES = S.gpu_cases()[1::3]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sim3_core") / "sim3_core_driver"
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", f"-I{ROOT / 'snake_slam_amd' / 'csrc'}",
           str(ROOT / "tests" / "cpp" / "sim3_core_driver.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_cpu_build_of_the_core_equals_the_restatement(driver, tmp_path, c):
    seed, problem, its = c["seed"] & 0xFFFFFFFF, 3, max(c["iterations"], 100)  # a seed a double carries exactly
    for name, key in (("p1", "P1"), ("p2", "P2"), ("ip1", "ip1"), ("ip2", "ip2")):
        c[key].tofile(tmp_path / f"{name}.bin")
    np.array([float(its), float(seed), float(problem), float(c["compute_scale"]), c["threshold"], *S.CAM]).tofile(tmp_path / "params.bin")
    r = subprocess.run([str(driver), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    tri = np.fromfile(tmp_path / "out_tri.bin", np.int32).reshape(-1, 3)
    valid = np.fromfile(tmp_path / "out_valid.bin", np.int32)
    T = np.fromfile(tmp_path / "out_T.bin", np.float64).reshape(-1, 8)
    counts = np.fromfile(tmp_path / "out_counts.bin", np.int32)
    H = S.hypotheses(c["P1"], c["P2"], c["ip1"], c["ip2"], its, c["threshold"], c["compute_scale"], seed, problem)
    assert np.array_equal(tri, H["triplets"])
    assert np.array_equal(valid.astype(bool), H["valid"])
    worst = 0.0
    for k in np.nonzero(H["valid"])[0]:
        worst = max(worst, S.transform_distance(S.quat_to_R(T[k, :4]), T[k, 4:7], T[k, 7], H["R"][k], H["t"][k], H["s"][k]))
    print(f"{c['name']}: largest transform difference to the restatement {worst:.2e}")
    assert worst <= S.transform_tolerance()
    ok = ~H["borderline"]
    assert np.array_equal(counts[ok], H["counts"][ok])
    its_all = np.fromfile(tmp_path / "out_its.bin", np.int32)
    assert np.array_equal(its_all, [S.ransac_iterations(n) for n in range(2049)])
