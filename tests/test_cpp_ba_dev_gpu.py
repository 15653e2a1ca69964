"""GPU: snake_hip::BARec::createDev of the C++ adaptor header (snake_slam_amd/cpp/snake_hip.hpp) built into a small driver
(tests/cpp/ba_dev_driver.cpp, plain g++ against the HIP runtime's C API) and EXECUTED on three unequal windows laid out as device rows, one
of them an empty row: the costs and the states it dumps must equal, byte for byte, what snk_ba_set_problems gives for the same rows."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import handover_cases as HC
import handover_numpy as M

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def build_driver(out_dir: Path) -> Path:
    lib = ROOT / "snake_slam_amd" / "lib"
    exe = out_dir / "ba_dev_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{ROOT / 'include'}", f"-I{ROOT / 'snake_slam_amd' / 'cpp'}",
           "-isystem", "/opt/rocm/include", str(ROOT / "tests" / "cpp" / "ba_dev_driver.cpp"), f"-L{lib}", "-lsnake_hip", "-L/opt/rocm/lib", "-lamdhip64",
           f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_cpp_create_dev_equals_the_hand_over_from_host_arrays(tmp_path):
    rows = HC.unequal_batch(3, seed=4)
    o = M.pad_rows(rows, dict(pt_cap=64, img_cap=8, obs_cap=256))
    for name in ("pose", "img_const", "pt", "pt_const", "obs_img", "obs_pt", "obs_uv", "obs_depth", "obs_weight", "rpc", "result"):
        np.ascontiguousarray(o[name]).tofile(tmp_path / f"{name}.bin")
    np.array([3, o["win_cap"], o["pt_cap"], o["img_cap"], o["obs_cap"]], np.int32).tofile(tmp_path / "meta.bin")
    np.array(list(HC.K) + [HC.BF], np.float64).tofile(tmp_path / "kbf.bin")
    exe = build_driver(tmp_path)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    ba = HC.load_host(o)
    ci, cf = ba.initAndSolve()
    states = [ba.state(p) for p in range(3)]
    ba.close()
    cost = np.fromfile(tmp_path / "out_cost.bin", np.float64).reshape(3, 2)
    assert cost[:, 0].tobytes() == ci.tobytes() and cost[:, 1].tobytes() == cf.tobytes()
    assert np.fromfile(tmp_path / "out_pose.bin", np.float64).tobytes() == b"".join(s[0].tobytes() for s in states)
    assert np.fromfile(tmp_path / "out_pt.bin", np.float64).tobytes() == b"".join(s[1].tobytes() for s in states)
