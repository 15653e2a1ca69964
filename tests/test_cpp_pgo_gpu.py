"""GPU: snake_hip::PoseGraph / PGORec / PGOSim3Rec / TransformMapPoints of the C++ adaptor header built into a small driver
(tests/cpp/pgo_driver.cpp, plain g++) and EXECUTED on the CorrectLoop-shaped ring of 8: edges added unsorted and twice, sortEdges,
SetPose of the source, create, initAndSolve -- the poses must equal the Python mirror's byte for byte (the same library, the same input)
and lie within pose_tolerance() of the restatement's optimum."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pgo_numpy as P

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def build_driver(out_dir: Path) -> Path:
    lib = ROOT / "snake_slam_amd" / "lib"
    exe = out_dir / "pgo_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", f"-I{ROOT / 'snake_slam_amd' / 'cpp'}",
           str(ROOT / "tests" / "cpp" / "pgo_driver.cpp"), f"-L{lib}", "-lsnake_hip", "-L/opt/rocm/lib", "-lamdhip64",
           f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("fix", [1, 0], ids=["PGORec", "PGOSim3Rec"])
def test_cpp_pose_graph_equals_the_python_mirror(tmp_path, fix):
    from snake_slam_amd.loop import PoseGraph, PoseGraphOptimizer

    G = P.correct_loop(8, 2, fix)  # its measurements are those of poses_measure except the loop edge's -- here the loop edge is measured too
    gt, n = G["poses_measure"], 8
    edges = [(i, i + 1, 1.0 + 0.1 * i) for i in range(n - 1)] + [(n - 1, 0, 2.0)]
    added = edges[::-1] + edges[:3]  # unsorted, three of them twice
    rng = np.random.default_rng(4)
    pts = np.concatenate([rng.integers(-1, n, (50, 1)).astype(np.float64), rng.standard_normal((50, 3))], 1)
    gt.tofile(tmp_path / "poses.bin")
    G["constant"].astype(np.float64).tofile(tmp_path / "constant.bin")
    np.array(added, np.float64).tofile(tmp_path / "edges.bin")
    np.concatenate([[n - 1.0], G["poses_init"][n - 1]]).tofile(tmp_path / "set_pose.bin")
    np.array([float(fix)]).tofile(tmp_path / "params.bin")
    pts.tofile(tmp_path / "points.bin")
    exe = build_driver(tmp_path)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)

    pg = PoseGraph(gt, G["constant"], bool(fix))
    for i, j, w in added:
        pg.add_vertex_edge(i, j, w)
    pg.sort_edges()
    pg.set_pose(n - 1, G["poses_init"][n - 1])
    assert [e[:2] for e in pg.edges] == sorted({(min(i, j), max(i, j)) for i, j, _ in edges})
    o = PoseGraphOptimizer()
    try:
        o.create(pg)
        res = o.init_and_solve()
        poses = o.poses()
        pos, _, dep = o.transform_points(pts[:, 0].astype(np.int32), pts[:, 1:], None, np.full(50, 2.0))
    finally:
        o.close()
    assert np.fromfile(tmp_path / "out_poses.bin", np.float64).tobytes() == poses.tobytes()
    out = np.fromfile(tmp_path / "out_result.bin", np.float64)
    assert list(out) == [res["cost_initial"], res["cost_final"], res["lm_iterations"], res["pcg_iterations_total"], res["accepted_steps"]]
    assert np.fromfile(tmp_path / "out_points.bin", np.float64).tobytes() == np.concatenate([pos, dep[:, None]], 1).tobytes()
    ed = np.array([e[:2] for e in pg.edges], np.int32)
    want, info = P.optimise(dict(poses_measure=gt, poses_init=pg.poses, constant=G["constant"], edges=ed, weights=np.array([e[2] for e in pg.edges]),
                                 measurements=None, fix_scale=fix))
    assert res["cost_final"] < res["cost_initial"] and P.pose_distance(poses, want) <= P.pose_tolerance()
