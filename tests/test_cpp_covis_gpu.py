"""GPU: snake_hip::CovisibilityGraph of the C++ adaptor header (snake_slam_amd/cpp/snake_hip.hpp) built into a small driver
(tests/cpp/covis_driver.cpp, plain g++) and EXECUTED against mock Keyframe / MapPoint structs joined by pointers: UpdateConnections,
VoteLocalKeyframes and the two list helpers must return, byte for byte, what the Python mirror returns from the same library on the
edge case, and that is the restatement."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import covis_numpy as M

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def build_driver(out_dir: Path) -> Path:
    lib = ROOT / "snake_slam_amd" / "lib"
    exe = out_dir / "covis_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", f"-I{ROOT / 'snake_slam_amd' / 'cpp'}",
           str(ROOT / "tests" / "cpp" / "covis_driver.cpp"), f"-L{lib}", "-lsnake_hip", "-L/opt/rocm/lib", "-lamdhip64",
           f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_cpp_covisibility_graph_equals_the_python_mirror(tmp_path):
    from snake_slam_amd.covis import CovisibilityGraph

    c, cap = M.edge_case(), 64
    for name in M.MAP_KEYS + M.FEAT_KEYS + ("q", "set_start", "set_point"):
        np.ascontiguousarray(c[name]).tofile(tmp_path / f"{name}.bin")
    np.array([len(c["kf_bad"]), len(c["pt_flags"]), M.TH, cap], np.int32).tofile(tmp_path / "meta.bin")
    np.array([M.TH_DEPTH], np.float32).tofile(tmp_path / "th_depth.bin")
    exe = build_driver(tmp_path)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    g = CovisibilityGraph(M.TH, M.TH_DEPTH, cap)
    try:
        mirror = dict(update=g.update(*(c[k] for k in M.MAP_KEYS + M.FEAT_KEYS), c["q"]),
                      vote=g.vote(*(c[k] for k in M.MAP_KEYS), c["set_start"], c["set_point"]))
    finally:
        g.close()
    want = dict(update=M.update(c, c["q"], cap=cap), vote=M.vote(c, c["set_start"], c["set_point"], cap=cap))
    for op in ("update", "vote"):
        conn, res = mirror[op]
        assert np.fromfile(tmp_path / f"{op}_conn.bin", M.CONN).tobytes() == conn.tobytes() == want[op][0].tobytes(), op
        assert np.fromfile(tmp_path / f"{op}_res.bin", M.RESULT).tobytes() == res.tobytes() == want[op][1].tobytes(), op
        best = np.fromfile(tmp_path / f"{op}_best5.bin", np.int32).reshape(-1, 5)
        w16 = np.fromfile(tmp_path / f"{op}_w16.bin", np.int32)
        for s in range(len(res)):
            kept = conn[s][:res[s]["n_conn"]]
            b = kept["kf"][-5:]  # GetBestCovisibilityKeyFrames(5), KeyframeGraph.cpp:62: the last five, the best last
            assert np.array_equal(best[s][:len(b)], b) and np.all(best[s][len(b):] == -1), (op, s)
            assert w16[s] == np.count_nonzero(kept["weight"] >= 16), (op, s)  # GetCovisiblesByWeight(16), :148-172
