"""CPU: snake_slam_amd/csrc/mappoint_core.hpp and the map-point part of dispatch.hpp compiled with plain g++ (no HIP) into
tests/cpp/mappoint_core_driver.cpp.  The per-point statements -- the selection by nine halvings (the packed kernel's) and by three
eight-way passes (the wide kernel's), first-wins, the fp64 expressions of the normal and the reference depth -- must equal the numpy
restatement (tests/mappoint_numpy.py: rows actually sorted) bit for bit, and the form each k selects is pinned."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mappoint_numpy as M

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mp_core") / "mappoint_core_driver"
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", f"-I{ROOT / 'include'}", f"-I{ROOT / 'snake_slam_amd' / 'csrc'}",
           str(ROOT / "tests" / "cpp" / "mappoint_core_driver.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_driver(exe, d, case, rule, what, eight_way=0):
    for name, a in case.items():
        np.ascontiguousarray(a).tofile(d / f"{name}.bin")
    np.array([rule, what, eight_way], np.int32).tofile(d / "meta.bin")
    r = subprocess.run([str(exe), str(d)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return np.fromfile(d / "out.bin", M.RESULT)


@pytest.mark.parametrize("near_tie", [False, True])
@pytest.mark.parametrize("rule", [M.MEDIAN, M.SUM])
def test_core_statements_equal_the_restatement_bit_for_bit(driver, tmp_path, rule, near_tie):
    ks = [0, 1, 2, 3, 4, 5, 8, 17, 31, 32, 33, 64, 65, 130, 300]
    c = M.make_case(40 + rule, ks, near_tie, invalid_frac=0.15)
    c["valid"][M.point_slice(c, 6)][:] = 0  # a point without a valid observation
    c["pose"][c["obs_start"][7]] = [0, 0, 0, 1, *(-c["position"][7])]  # a camera centre on the point: s = 0
    got = run_driver(driver, tmp_path, c, rule, M.ALL)
    want = M.refresh(c, rule)
    assert got.tobytes() == want.tobytes(), [(p, got[p], want[p]) for p in range(len(ks)) if got[p].tobytes() != want[p].tobytes()][:3]
    # the wide kernel's three eight-way passes select the element the nine halvings select
    assert run_driver(driver, tmp_path, c, rule, M.ALL, eight_way=1).tobytes() == want.tobytes()
    assert got["best"][6] == -1 and got["n_valid"][6] == 0 and (got["best"][1:] >= 0).sum() >= len(ks) - 3


@pytest.mark.parametrize("what", [M.DESCRIPTOR, M.NORMAL, M.DEPTH])
def test_core_what_masks(driver, tmp_path, what):
    c = M.make_case(50, [3, 9, 0, 40], True)
    assert run_driver(driver, tmp_path, c, M.MEDIAN, what).tobytes() == M.refresh(c, M.MEDIAN, what).tobytes()


def test_both_selections_return_the_element_of_the_sorted_row_for_every_rank(driver):
    r = subprocess.run([str(driver), "--select"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) > 50000


def test_forms_are_pinned(driver):
    ks = [0, 1, 2, 30, 31, 32, 33, 63, 64, 65, 1000, 4096]
    out = lambda env: subprocess.run([str(driver), "--forms", str(env), *map(str, ks)], capture_output=True, text=True, check=True).stdout.split("\n")
    for env in (0, 1):  # unset, SNK_MP_FORM=packed: the packed form up to MP_PACKED_MAX_K, the wide form beyond
        lines = out(env)
        assert lines[:len(ks)] == [f"{k} {'packed' if k <= 32 else 'wide'}" for k in ks]
    lines = out(2)  # SNK_MP_FORM=wide
    assert lines[:len(ks)] == [f"{k} wide" for k in ks]
    consts = dict(zip(lines[len(ks)].split()[::2], map(int, lines[len(ks)].split()[1::2])))
    assert consts["packed_max_k"] == M.PACKED_MAX_K == 32 and consts["chunk_points"] == M.CHUNK_POINTS == 64
    assert consts["packed_rows_max"] == 64 * 32
    # descriptors (32 B a row) + flags + the slot map + four ints a point; 128 KB of descriptors + flags + keys for the largest point
    assert consts["packed_carve_max"] == 2048 * 32 + 2048 + 64 * 64 * 2 + 64 * 16 + 16 <= 160 * 1024
    assert consts["wide_carve_max"] == 4096 * 32 + 4096 + 16 * 8 + 16 <= 160 * 1024
