"""CPU: the covisibility block keeps include/snake_hip.h C99 (the structs, the limits and the four entry points are usable from a C
translation unit), and snake_hip::CovisibilityGraph of the C++ adaptor header compiles (plain g++, -Wall -Werror) against the mock
Keyframe / MapPoint structs of tests/cpp/covis_driver.cpp and links into the driver of tests/test_cpp_covis_gpu.py; without inputs the
driver fails cleanly (exception text, status 1) instead of crashing."""
import subprocess
from pathlib import Path

from test_cpp_covis_gpu import build_driver

ROOT = Path(__file__).resolve().parent.parent

C99_USER = r"""
#include "snake_hip.h"
#if SNK_COVIS_MAX_KF != 32768 || SNK_COVIS_MAX_CAP != 4096 || SNK_COVIS_OK != 0 || SNK_COVIS_UNCHANGED != 1 || SNK_COVIS_BAD_INDEX != 2
#error "snk-covis constants"
#endif
typedef char conn_is_two_ints[sizeof(snk_covis_conn) == 8 ? 1 : -1];
typedef char result_is_four_ints[sizeof(snk_covis_result) == 16 ? 1 : -1];
int use(snk_matcher* m, const snk_covis_map* map, const int32_t* start, const int32_t* point, const float* depth, const int32_t* q,
        snk_covis_conn* conn, snk_covis_result* out)
{
    snk_covis_params par;
    par.th = 15;
    par.th_depth = 40.0f;
    par.cap = 64;
    return snk_covis_update(m, map, start, point, depth, &par, 1, q, conn, out) + snk_covis_update_batch_dev(m, map, start, 0, point, depth, &par, 1, q, conn, out) +
           snk_covis_vote(m, map, 1, start, point, &par, conn, out) + snk_covis_vote_batch_dev(m, map, 1, start, 0, point, &par, conn, out);
}
"""


def test_header_stays_c99_with_the_covisibility_block(tmp_path):
    src = tmp_path / "use_covis.c"
    src.write_text(C99_USER)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{ROOT / 'include'}", "-c", str(src), "-o", str(tmp_path / "use_covis.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_covis_driver_compiles_and_fails_cleanly_without_inputs(tmp_path):
    exe = build_driver(tmp_path)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 1 and "covis_driver: missing input" in r.stderr
