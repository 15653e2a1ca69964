"""CPU: snake_slam_amd/csrc/lmap_core.hpp and the local-map part of dispatch.hpp compiled with plain g++ (no HIP) into
tests/cpp/lmap_core_driver.cpp.  The draw, the accept rule, the hash, the skip rules and the reading of a vote record must equal the
Python mirror (tests/localmap_numpy.py) on a few thousand rows, the edges n = 0, 1, k, k + 1 and h = 0, 2^32 - 1 included; the limits,
the table sizes and the carve formulas are pinned."""
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import localmap_numpy as M

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("lmap_core") / "lmap_core_driver"
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{ROOT / 'include'}", f"-I{ROOT / 'snake_slam_amd' / 'csrc'}",
           str(ROOT / "tests" / "cpp" / "lmap_core_driver.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def rows():
    rng = np.random.RandomState(17)
    n = 4000
    r = np.zeros((n, 15), np.int64)
    r[:, 0] = rng.randint(0, 2 ** 62, n) * 4 + rng.randint(0, 4, n)  # seed: all 64 bits (wraps into the sign)
    r[:, 1] = rng.randint(-2 ** 31, 2 ** 31, n)  # frame id
    r[:, 2] = rng.randint(0, 2 ** 32, n)  # draw number
    r[:, 3] = rng.randint(0, 9, n)  # k
    r[:, 4] = rng.randint(0, 40, n)  # n
    r[:, 5] = rng.randint(0, 2 ** 32, n)  # h
    r[:, 6] = rng.randint(-1, 2 ** 31, n)  # point id
    r[:, 7] = rng.randint(0, 4, n)  # flags
    r[:, 8] = np.where(rng.randint(0, 3, n) == 0, r[:, 1], rng.randint(-2 ** 31, 2 ** 31, n))  # last seen: a third in this frame
    r[:, 9] = rng.randint(0, 2, n) * rng.randint(1, 256, n)  # kf_bad: any non-zero byte
    r[:, 10] = rng.randint(0, 2, n)
    r[:, 11] = rng.randint(0, 4, n)  # vote status, 3 unknown
    r[:, 12] = rng.randint(-1, 12, n)
    r[:, 13] = rng.randint(-1, 12, n)
    r[:, 14] = rng.randint(1, 12, n)
    # the edges of the accept rule: n = 0, 1, k, k + 1 and h = 0, 2^32 - 1, around the threshold too
    edges = []
    for k, h in itertools.product((0, 1, 5, 8), (0, 1, 2 ** 32 - 1, 2 ** 31, 2 ** 31 - 1)):
        for nn in (0, 1, k, k + 1, 2 * k, 2 * k + 1, 32768):
            edges.append((k, nn, h))
    for k, nn in ((5, 7), (5, 65), (3, 257), (1, 3)):  # h just below / at / above k * 2^32 / n
        t = (k << 32) // nn
        edges += [(k, nn, t - 1), (k, nn, t), (k, nn, t + 1)]
    for i, (k, nn, h) in enumerate(edges):
        r[i, 3], r[i, 4], r[i, 5] = k, nn, h
    r[:40, 0] = [0, 1, 2 ** 32 - 1, 2 ** 32, -1] * 8  # seeds whose halves are 0 / all ones
    r[40:60, 6] = [-1, 0, 1, 2 ** 31 - 1] * 5
    return r


def test_core_statements_equal_the_python_mirror(driver, tmp_path):
    r = rows()
    r.tofile(tmp_path / "rows.bin")
    p = subprocess.run([str(driver), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    got = np.fromfile(tmp_path / "out.bin", np.int64).reshape(len(r), 9)
    want = np.zeros_like(got)
    for i, (seed, fid, c, k, n, h, pid, flags, seen, bad, marked, vs, nf, nc, vc) in enumerate(r.tolist()):
        key = M.key_of(seed & (2 ** 64 - 1), fid)
        d = M.draw(key, c)
        want[i] = (key, d, M.accept(d, k, n), M.accept(h, k, n), M.hash_of(pid), pid < 0 or bool(flags & M.PT_BAD) or seen == fid,
                   pid < 0 or bool(flags & M.PT_BAD), bad == 0 and not marked, M.vote_status(vs, nf, nc, vc))
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    # n <= k always accepts (k > 0), k = 0 never does; the rule is the real-number comparison h / 2^32 < k / n
    for i, (k, n, h) in enumerate(r[:, 3:6].tolist()):
        assert got[i, 3] == (k > 0 and (n == 0 or h * n < k * 2 ** 32)), (k, n, h)
        if 0 < k and n <= k:
            assert got[i, 3] == 1
    assert 0.2 < got[:, 2].mean() < 0.8 and len(set(got[:, 1].tolist())) > 3990 and len(set((got[:, 4] & 511).tolist())) == 512


def test_limits_table_sizes_and_carves_are_pinned(driver):
    line = subprocess.run([str(driver), "--consts"], capture_output=True, text=True, check=True).stdout.split()
    k = dict(zip(line[::2], map(int, line[1::2])))
    assert k["threads"] == M.THREADS == 256 and k["max_local_kf"] == M.MAX_LOCAL_KF == 256 and k["max_pts"] == M.MAX_PTS == 16384
    assert k["max_neighbours"] == M.MAX_NEIGHBOURS == 16 and k["max_order"] == M.MAX_ORDER == 2 ** 30
    # load at most 0.5 and room for a claim per lane in flight
    assert [k[f"slots_{n}"] for n in (1, 64, 256, 257)] == [M.table_slots(n) for n in (1, 64, 256, 257)] == [512, 512, 512, 1024]
    assert k["slots_max"] == M.table_slots(M.MAX_PTS) == 32768
    assert k["sort_len_64_5"] == 512 and k["sort_len_max"] == 4096
    # a bit per keyframe (+ a word), the local list, a key and a first per slot, 32 words
    assert k["select_carve_max"] == (1024 + 1) * 4 + 256 * 4 + 4096 * 8 + 128 <= 160 * 1024
    assert k["select_carve_4096_64_5"] == (128 + 1) * 4 + 64 * 4 + 512 * 8 + 128
    # the table, the prefix sums and starts of the local keyframes, 32 words
    assert k["gather_carve_max"] == 32768 * 4 + (2 * 256 + 1) * 4 + 128 <= 160 * 1024
    assert k["gather_carve_64_2048"] == 4096 * 4 + (2 * 64 + 1) * 4 + 128
