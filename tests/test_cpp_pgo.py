"""CPU: snake_hip::PoseGraph / PGORec / PGOSim3Rec / TransformMapPoints of the C++ adaptor header compile as C++17 (plain g++, -Wall
-Werror) and link into the driver of tests/test_cpp_pgo_gpu.py; without inputs the driver fails cleanly (exception text, status 1); and
include/snake_hip.h with the snk_pgo_* declarations stays plain C99."""
import subprocess
from pathlib import Path

from test_cpp_pgo_gpu import build_driver

ROOT = Path(__file__).resolve().parent.parent


def test_pgo_driver_compiles_and_fails_cleanly_without_inputs(tmp_path):
    exe = build_driver(tmp_path)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 1 and "pgo_driver: missing input" in r.stderr


def test_header_with_the_pgo_entries_is_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "snake_hip.h"\n'
                   "int use(snk_pgo* h, const double (*p)[8], const uint8_t* c, const int32_t (*e)[2], double (*out)[8])\n{\n"
                   "    snk_pgo_options o = {50, 2000, 1e-10, 1e-10, 1e-4};\n    snk_pgo_result r;\n    (void)o;\n"
                   "    return snk_pgo_set_graph(h, 3, p, 0, c, 2, e, 0, 0, 1) + snk_pgo_solve(h, &r) + snk_pgo_get_poses(h, out);\n}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT / 'include'}", "-c", str(src), "-o",
                        str(tmp_path / "use.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
