"""CPU: bow_core.hpp -- the statements the kernels run -- built with plain g++ (-ffp-contract=off -Wall -Werror) through
tests/cpp/bow_core_driver.cpp and executed on the cases of the GPU test: the word and the feature-vector node of every descriptor and
every MatchBoW decision equal the numpy restatement's exactly.  The same driver, built once more with -fsanitize=address,undefined as a
stand-alone program, runs the smallest and the irregular case clean; and bow_validate (through the driver) refuses unsound trees."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bow_numpy as B

ROOT = Path(__file__).resolve().parent.parent


def build(tmp, flags=(), name="bow_core_driver"):
    exe = tmp / name
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", *flags, f"-I{ROOT / 'snake_slam_amd' / 'csrc'}",
           str(ROOT / "tests" / "cpp" / "bow_core_driver.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("bow_core"))


@pytest.fixture(scope="module")
def driver_sanitized(tmp_path_factory):
    return build(tmp_path_factory.mktemp("bow_core_san"), ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"), "bow_core_driver_san")


def write_vocab(d: Path, arrays: dict):
    for k, dt in (("child_start", np.int32), ("child_count", np.int32), ("children", np.int32), ("desc", np.uint64), ("weight", np.float64)):
        np.ascontiguousarray(arrays[k], dt).tofile(d / f"v_{k}.bin")
    np.ascontiguousarray(arrays["word_id"], np.int32).tofile(d / "v_word.bin")


def case_descriptors(name):
    """every descriptor the GPU transform test feeds this vocabulary (a descriptor's word and node do not depend on its frame)"""
    sets = [B.frame_descriptors(name, n) for n in B.FEATURE_COUNTS if n]
    sets += [B.crowd_descriptors(name, True), B.crowd_descriptors(name, False)]
    if name.startswith("twins"):
        sets.append(B.tie_descriptors(name))
    return np.concatenate(sets)


def run_transform(exe, d: Path, V, descs, levelsup):
    write_vocab(d, V.arrays())
    np.ascontiguousarray(descs, np.uint64).tofile(d / "desc.bin")
    r = subprocess.run([str(exe), str(d), "transform", str(levelsup)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return np.fromfile(d / "out_word.bin", np.int32), np.fromfile(d / "out_node.bin", np.int32)


@pytest.mark.parametrize("name", list(B.VOCABS))
def test_words_and_nodes_equal_the_restatement(driver, tmp_path, name):
    V = B.vocab(name)
    descs = case_descriptors(name)
    paths = [B.descend(V, d) for d in descs]
    for up in B.levelsups(V):
        word, node = run_transform(driver, tmp_path, V, descs, up)
        assert np.array_equal(word, [V.word_id[p[-1]] for p in paths])
        assert np.array_equal(node, [B.node_up(V, p, up) for p in paths])


def write_scene(d: Path, s):
    for k in ("1", "2"):
        np.ascontiguousarray(s["desc" + k], np.uint64).tofile(d / f"desc{k}.bin")
        np.ascontiguousarray(s["has" + k], np.uint8).tofile(d / f"has{k}.bin")
        nid, ns, ft = s["bow" + k]
        np.ascontiguousarray(nid, np.int32).tofile(d / f"nid{k}.bin")
        np.ascontiguousarray(ns, np.int32).tofile(d / f"ns{k}.bin")
        np.ascontiguousarray(ft, np.int32).tofile(d / f"ft{k}.bin")


MATCH_CASES = B.match_cases()


@pytest.mark.parametrize("case", MATCH_CASES, ids=[c[0] for c in MATCH_CASES])
def test_match_decisions_equal_the_restatement(driver, tmp_path, case):
    name, s, th, ratio = case
    write_vocab(tmp_path, B.hand_vocab().arrays())
    write_scene(tmp_path, s)
    r = subprocess.run([str(driver), str(tmp_path), "match", str(th), repr(float(ratio))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    want, _ = B.match_bow(s["desc1"], s["has1"], s["bow1"], s["desc2"], s["has2"], s["bow2"], th, ratio)
    assert np.array_equal(np.fromfile(tmp_path / "out_m12.bin", np.int32), want)


def test_sanitized_build_runs_the_smallest_and_the_irregular_case(driver_sanitized, tmp_path):
    for name, n in (("single_level", 1), ("irregular", 300)):
        V = B.vocab(name)
        descs = B.frame_descriptors(name, n)
        word, node = run_transform(driver_sanitized, tmp_path, V, descs, 2)
        t = B.transform(V, descs, 2)
        assert np.array_equal(word, t["word_of_feature"]) and np.array_equal(node, t["node_of_feature"])
    name, s, th, ratio = next(c for c in MATCH_CASES if c[0] == "scene_irregular_257")
    write_scene(tmp_path, s)
    r = subprocess.run([str(driver_sanitized), str(tmp_path), "match", str(th), repr(float(ratio))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    want, _ = B.match_bow(s["desc1"], s["has1"], s["bow1"], s["desc2"], s["has2"], s["bow2"], th, ratio)
    assert np.array_equal(np.fromfile(tmp_path / "out_m12.bin", np.int32), want)


def test_sanitized_build_refuses_unsound_trees(driver_sanitized, tmp_path):
    a = B.hand_vocab().arrays()
    np.zeros((1, 4), np.uint64).tofile(tmp_path / "desc.bin")
    bad = dict(a, children=np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 1], np.int32))  # node 1 twice, node 12 never
    write_vocab(tmp_path, bad)
    r = subprocess.run([str(driver_sanitized), str(tmp_path), "transform", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "invalid vocabulary" in r.stderr, (r.returncode, r.stderr)
