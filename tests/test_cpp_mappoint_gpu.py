"""GPU: snake_hip::MapPointRefresher of the C++ adaptor header (snake_slam_amd/cpp/snake_hip.hpp) built into a small driver
(tests/cpp/mappoint_driver.cpp, plain g++) and EXECUTED against mock Keyframe / MapPoint structs: Refresh and the three methods with the
reference's names must return, byte for byte, what the Python mirror returns from the same library for the gathered lists, and that
is the numpy restatement."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mappoint_numpy as M

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def build_driver(out_dir: Path) -> Path:
    lib = ROOT / "snake_slam_amd" / "lib"
    exe = out_dir / "mappoint_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", f"-I{ROOT / 'snake_slam_amd' / 'cpp'}",
           str(ROOT / "tests" / "cpp" / "mappoint_driver.cpp"), f"-L{lib}", "-lsnake_hip", "-L/opt/rocm/lib", "-lamdhip64",
           f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_cpp_mappoint_refresher_equals_the_python_mirror(tmp_path):
    from snake_slam_amd.mappoint import MapPointRefresher

    rng = np.random.default_rng(17)
    NK, CAP, rule = 40, 16, M.MEDIAN
    ks = [0, 1, 2, 5, 9, 31, 32, 33, 40] + [int(k) for k in rng.integers(2, 12, 80)]
    kf_pose = M.random_pose(rng, NK)
    kf_desc = M.descriptors(rng, NK * CAP, True).reshape(NK, CAP, 4)
    kf_oct = rng.integers(0, 8, (NK, CAP)).astype(np.int32)
    kf_bad = (rng.random(NK) < 0.1).astype(np.uint8)
    start = np.concatenate([[0], np.cumsum(ks)]).astype(np.int32)
    obs = np.concatenate([np.stack([rng.permutation(NK)[:k], rng.integers(0, CAP, k)], 1) for k in ks]).astype(np.int32)  # distinct keyframes per point
    position = rng.uniform(-3, 3, (len(ks), 3))
    ref_obs = np.array([int(rng.integers(-1, k)) if k else -1 for k in ks], np.int32)
    ref_kf = np.array([obs[start[p] + r, 0] if r >= 0 else -1 for p, r in enumerate(ref_obs)], np.int32)
    for name, a in (("meta", np.array([NK, CAP, rule], np.int32)), ("kf_pose", kf_pose), ("kf_desc", kf_desc), ("kf_octave", kf_oct), ("kf_bad", kf_bad),
                    ("obs_start", start), ("obs", obs), ("position", position), ("ref_kf", ref_kf)):
        np.ascontiguousarray(a).tofile(tmp_path / f"{name}.bin")
    exe = build_driver(tmp_path)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert np.array_equal(np.fromfile(tmp_path / "out_ref_obs.bin", np.int32), ref_obs)
    case = dict(obs_start=start, desc=kf_desc[obs[:, 0], obs[:, 1]], pose=kf_pose[obs[:, 0]], octave=kf_oct[obs[:, 0], obs[:, 1]],
                valid=(1 - kf_bad[obs[:, 0]]).astype(np.uint8), position=position, ref_obs=ref_obs)
    mirror = MapPointRefresher(rule)
    try:
        for name, what in (("all", M.ALL), ("desc", M.DESCRIPTOR), ("normal", M.NORMAL), ("depth", M.DEPTH)):
            want = mirror.refresh(*(case[k] for k in ("obs_start", "desc", "pose", "octave", "valid", "position", "ref_obs")), what=what)
            got = np.fromfile(tmp_path / f"out_{name}.bin", M.RESULT)
            assert got.tobytes() == want.tobytes(), name
            assert want.tobytes() == M.refresh(case, rule, what).tobytes(), name
    finally:
        mirror.close()
