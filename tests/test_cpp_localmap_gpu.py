"""GPU: snake_hip::LocalMapBuilder of the C++ adaptor header (snake_slam_amd/cpp/snake_hip.hpp) built into a small driver
(tests/cpp/localmap_driver.cpp, plain g++) and EXECUTED on the edge case: the local keyframes, the records, the point ids and the result
words it dumps must equal, byte for byte, the restatement's (tests/localmap_numpy.py)."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import localmap_numpy as M

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def build_driver(out_dir: Path) -> Path:
    lib = ROOT / "snake_slam_amd" / "lib"
    exe = out_dir / "localmap_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", f"-I{ROOT / 'snake_slam_amd' / 'cpp'}",
           str(ROOT / "tests" / "cpp" / "localmap_driver.cpp"), f"-L{lib}", "-lsnake_hip", "-L/opt/rocm/lib", "-lamdhip64",
           f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_cpp_local_map_builder_equals_the_restatement(tmp_path):
    seed, pts_cap = M.SEEDS[1], 64
    e = M.edge_case(pts_cap, seed)
    c, g = e["select"], e["gather"]
    kf_cap = g["local_kf"].shape[1]  # one builder for both stages: the gather case's lists are 16 wide
    params = dict(kf_cap=kf_cap, seed=seed)
    for name in M.SELECT_KEYS:
        np.ascontiguousarray(c[name]).tofile(tmp_path / f"{name}.bin")
    for name in M.GATHER_KEYS + M.POINT_KEYS:
        np.ascontiguousarray(g["m"][name]).tofile(tmp_path / f"{name}.bin")
    for name, key in (("g_frame_id", "frame_id"), ("g_local_kf", "local_kf"), ("g_sel", "sel"), ("set_start", "set_start"), ("set_point", "set_point")):
        np.ascontiguousarray(g[key]).tofile(tmp_path / f"{name}.bin")
    p = dict(M.PARAMS, **params)
    np.array([len(c["vote"]), c["vote_cap"], c["n_kf"], p["n_direct"], p["n_direct_prob"], p["n_indirect_prob"], p["n_neighbours"], kf_cap, pts_cap,
              len(g["sel"])], np.int32).tofile(tmp_path / "meta.bin")
    np.array([seed], np.uint64).tofile(tmp_path / "seed.bin")
    exe = build_driver(tmp_path)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    local, sel = M.select(*(c[k] for k in M.SELECT_KEYS), params)
    assert M.KF_OVERFLOW in sel["status"] and M.OK in sel["status"]  # 16 local keyframes do not hold the long votes
    assert np.fromfile(tmp_path / "out_local_kf.bin", np.int32).tobytes() == local.tobytes()
    assert np.fromfile(tmp_path / "out_sel.bin", M.SELECT).tobytes() == sel.tobytes()
    lm, ids, n_pts, res = M.gather(g["m"], g["frame_id"], g["local_kf"], g["sel"], g["set_start"], g["set_point"], pts_cap)
    assert np.fromfile(tmp_path / "out_counts.bin", np.int32).tobytes() == n_pts.tobytes()
    assert np.fromfile(tmp_path / "out_res.bin", M.GATHER).tobytes() == res.tobytes()
    assert np.fromfile(tmp_path / "out_ids.bin", np.int32).tobytes() == b"".join(ids[s, :n].tobytes() for s, n in enumerate(n_pts))
    assert np.fromfile(tmp_path / "out_lm.bin", M.LM_FINE).tobytes() == b"".join(lm[s, :n].tobytes() for s, n in enumerate(n_pts))
