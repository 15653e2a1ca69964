"""GPU: snake_hip::ORBVocabulary, KeyframeDatabase and LoopORBmatcher of the C++ adaptor header built into a small driver
(tests/cpp/bow_driver.cpp, plain g++) and EXECUTED as the loop closer uses them: transform of three keyframes, Add, score,
DetectLoopCandidates / DetectRelocalizationCandidates, Remove, MatchBoW must return, byte for byte, what the Python mirror returns from
the same library (the float scores of the reference's signature are the doubles rounded to float)."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bow_numpy as B

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def build_driver(out_dir: Path) -> Path:
    lib = ROOT / "snake_slam_amd" / "lib"
    exe = out_dir / "bow_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", f"-I{ROOT / 'snake_slam_amd' / 'cpp'}",
           str(ROOT / "tests" / "cpp" / "bow_driver.cpp"), f"-L{lib}", "-lsnake_hip", "-L/opt/rocm/lib", "-lamdhip64",
           f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def write_inputs(d: Path):
    V = B.vocab("k4_L6")
    a = V.arrays()
    for k, dt in (("child_start", np.int32), ("child_count", np.int32), ("children", np.int32), ("desc", np.uint64), ("weight", np.float64)):
        np.ascontiguousarray(a[k], dt).tofile(d / f"v_{k}.bin")
    np.ascontiguousarray(a["word_id"], np.int32).tofile(d / "v_word.bin")
    s = B.match_scene("k4_L6", 91, 200, 180, 4)
    third = B.leaf_descriptors(V, np.random.default_rng(92), 150, flips=3)
    descs = [s["desc1"], s["desc2"], third]
    for i, x in enumerate(descs):
        np.ascontiguousarray(x, np.uint64).tofile(d / f"desc{i}.bin")
    s["has1"].tofile(d / "has0.bin")
    s["has2"].tofile(d / "has1.bin")
    return V, s, descs


def test_cpp_bow_equals_the_python_mirror(tmp_path):
    from snake_slam_amd.bow import KeyframeDatabase, LoopMatcher, Vocabulary

    V, s, descs = write_inputs(tmp_path)
    exe = build_driver(tmp_path)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    G = Vocabulary.from_arrays(V.arrays())
    db = KeyframeDatabase(G, 16, 512)
    m = LoopMatcher()
    try:
        T = [G.transform(x, 4) for x in descs]
        for i, t in enumerate(T):
            for name, key, dt in (("words", "words", np.int32), ("values", "values", np.float64), ("nodes", "node_id", np.uint32),
                                  ("ns", "node_start", np.int32), ("ft", "features", np.int32)):
                assert np.fromfile(tmp_path / f"out_{name}{i}.bin", dt).tobytes() == t[key].tobytes(), (i, name)
            db.add(10 + i, t["words"], t["values"])
        bv = [(t["words"], t["values"]) for t in T]
        assert np.fromfile(tmp_path / "out_score.bin", np.float64)[0] == G.score(bv[0], bv[1])
        loop = db.detect_loop_candidates(bv[0], [10], 0.01, 5)
        reloc = db.detect_relocalization_candidates(bv[0], 0.5, 5)
        flat = lambda c: np.array([[i, np.float32(x).view(np.int32)] for i, x in c], np.int32).reshape(-1)  # noqa: E731
        assert np.array_equal(np.fromfile(tmp_path / "out_loop.bin", np.int32), flat(loop))
        assert np.array_equal(np.fromfile(tmp_path / "out_reloc.bin", np.int32), flat(reloc))
        assert reloc[0][0] == 10 and 10 not in [i for i, _ in loop] and len(loop) >= 1
        bow = lambda t: (t["node_id"], t["node_start"], t["features"])  # noqa: E731
        m12, n = m.match_bow(descs[0], s["has1"], bow(T[0]), descs[1], s["has2"], bow(T[1]), 50, 0.75)
        assert np.array_equal(np.fromfile(tmp_path / "out_m12.bin", np.int32), m12) and n > 20
        assert np.fromfile(tmp_path / "out_meta.bin", np.int32).tolist() == [V.n_words, n, len(loop), len(reloc)]
    finally:
        m.close()
        db.close()
        G.close()
