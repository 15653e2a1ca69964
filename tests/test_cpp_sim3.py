"""CPU: snake_hip::RegistrationRansac of the C++ adaptor header compiles as C++17 (plain g++, -Wall -Werror) and links into the driver of
tests/test_cpp_sim3_gpu.py; without inputs the driver fails cleanly (exception text, status 1) instead of crashing; and
include/snake_hip.h with the snk_sim3_* declarations stays plain C99."""
import subprocess
from pathlib import Path

from test_cpp_sim3_gpu import build_driver

ROOT = Path(__file__).resolve().parent.parent


def test_sim3_driver_compiles_and_fails_cleanly_without_inputs(tmp_path):
    exe = build_driver(tmp_path)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 1 and "sim3_driver: missing input" in r.stderr


def test_header_with_the_sim3_entries_is_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "snake_hip.h"\n'
                   "int use(snk_matcher* m, snk_sim3_problem* p)\n{\n"
                   "    snk_sim3_params q = {0, 1, 12.0, 0, 0.999, 15, 100};\n"
                   "    return snk_sim3_ransac(m, &q, p, 1) + snk_ransac_iterations(p->n, q.probability, q.min_inliers, q.max_iterations);\n}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT / 'include'}", "-c", str(src), "-o",
                        str(tmp_path / "use.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
