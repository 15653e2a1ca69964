"""CPU: snake_hip::ORBVocabulary / KeyframeDatabase / LoopORBmatcher of the C++ adaptor header compile as C++17 (plain g++, -Wall
-Werror) and link into the driver of tests/test_cpp_bow_gpu.py; without inputs the driver fails cleanly (exception text, status 1)
instead of crashing; and include/snake_hip.h with the snk_bow_* declarations stays plain C99."""
import subprocess
from pathlib import Path

from test_cpp_bow_gpu import build_driver

ROOT = Path(__file__).resolve().parent.parent


def test_bow_driver_compiles_and_fails_cleanly_without_inputs(tmp_path):
    exe = build_driver(tmp_path)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 1 and "bow_driver: missing input" in r.stderr


def test_header_with_the_bow_entries_is_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "snake_hip.h"\n'
                   "typedef char cap_is_2048[SNK_BOW_MAX_FEATURES == 2048 && SNK_BOW_MAX_CANDIDATES == 64 && SNK_BOW_MAX_DEPTH == 16 ? 1 : -1];\n"
                   "int use(snk_bow_vocab* v, snk_bow_db* db, snk_matcher* m, const snk_bow_features* f, const uint64_t (*d)[4], const uint8_t* h)\n{\n"
                   "    int32_t ids[4] = {0, 0, 0, 0}, m12[8];\n    double s[4] = {0.0, 0.0, 0.0, 0.0}, score = 0.0;\n    int n = 0;\n"
                   "    return snk_bow_db_query(db, ids, s, 0, ids, 0, 0.8f, 0.75f, 0.0f, 4, ids, s, ids, &n) + snk_bow_score(v, ids, s, 0, ids, s, 0, &score)\n"
                   "           + snk_match_loop_bow(m, d, h, 8, f, d, h, 8, f, 50, 0.75f, m12, &n);\n}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT / 'include'}", "-c", str(src), "-o",
                        str(tmp_path / "use.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
