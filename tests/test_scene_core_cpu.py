"""CPU: snake_slam_amd/csrc/scene_core.hpp and the scene part of dispatch.hpp compiled with plain g++ (no HIP) into
tests/cpp/scene_core_driver.cpp.  The number of neighbours taken, the survival of a candidate, the skip rules, the reading of a stage-1
record and the IMU gate must equal the restatement's statements (tests/scene_numpy.py) on a few thousand rows; the two weights must equal
Python's IEEE doubles bit for bit (gyro / dt and (w * acc) / dt, 0 behind dt > 2); the limits, the table sizes and the carves are pinned."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import scene_numpy as M

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("scene_core") / "scene_core_driver"
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{ROOT / 'include'}", f"-I{ROOT / 'snake_slam_amd' / 'csrc'}",
           str(ROOT / "tests" / "cpp" / "scene_core_driver.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_core_statements_equal_the_restatement(driver, tmp_path):
    rng = np.random.RandomState(23)
    n = 4000
    rows = np.zeros((n, 8))
    rows[:, 0] = rng.uniform(0, 1000, n)
    rows[:, 1] = rows[:, 0] + rng.choice([0.1, 1 / 3, 0.5, 2.0, 2.0000001, 2.5, 1e-3, 7.0], n) * rng.uniform(0.5, 1.0, n) ** rng.randint(0, 2, n)
    rows[:, 2] = np.where(rng.rand(n) < 0.7, rows[:, 0], np.nextafter(rows[:, 0], np.inf))
    rows[:, 3] = np.where(rng.rand(n) < 0.7, rows[:, 1], np.nextafter(rows[:, 1], -np.inf))
    rows[:, 4] = rng.randint(0, 2, n) * rng.randint(1, 256, n)
    rows[:, 5], rows[:, 6], rows[:, 7] = rng.uniform(0.01, 50, n), rng.uniform(0.01, 50, n), rng.uniform(0.0, 9, n)
    rows[:8, 0], rows[:8, 1] = 10.0, [12.0, np.nextafter(12.0, 13), np.nextafter(12.0, 11), 10.5, 13.0, 12.0, 12.0, 12.0]  # dt around 2
    flags = np.zeros((n, 10), np.int64)
    flags[:, 0], flags[:, 1] = rng.randint(0, 20, n), rng.randint(0, 40, n)
    flags[:, 2] = rng.randint(0, 2, n) * rng.randint(1, 256, n)
    flags[:, 3], flags[:, 4], flags[:, 5], flags[:, 6] = rng.randint(0, 2, n), rng.randint(-1, 50, n), rng.randint(0, 8, n), rng.randint(0, 2, n)
    flags[:, 7], flags[:, 8], flags[:, 9] = rng.randint(-1, 9, n), rng.randint(-2, 70, n), rng.randint(1, 65, n)
    rows.tofile(tmp_path / "rows.bin")
    flags.tofile(tmp_path / "flags.bin")
    p = subprocess.run([str(driver), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    got = np.fromfile(tmp_path / "out.bin", np.float64).reshape(n, 3)
    got_flags = np.fromfile(tmp_path / "out_flags.bin", np.int64).reshape(n, 6)
    want = np.zeros_like(got)
    for i, (ta, tb, begin, end, valid, gyro, acc, w) in enumerate(rows.tolist()):
        dt = tb - ta  # scene_numpy.make_scene, :331-339
        w_rot, w_tr = gyro / dt, w * acc / dt
        if dt > 2:
            w_rot, w_tr = 0.0, 0.0
        want[i] = (not (ta != begin or tb != end) and bool(valid), w_rot, w_tr)
    assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:5]
    assert 0.2 < got[:, 0].mean() < 0.8 and (got[:, 1] == 0).any() and (got[:, 1] > 0).any()
    for i, (nn, size, bad, earlier, pid, fl, img_const, status, n_window, win_cap) in enumerate(flags.tolist()):
        pt_const = bool(fl & M.PT_CONST)
        if status in (M.SKIPPED, M.WINDOW_OVERFLOW, M.BAD_INDEX):
            ws = status
        else:
            ws = M.OK if status == M.OK and 0 <= n_window <= min(win_cap, M.MAX_WINDOW) else M.BAD_INDEX
        want_flags = (min(nn, size), bad == 0 and not earlier, pid < 0 or bool(fl & M.PT_BAD), pt_const, bad != 0 or (bool(img_const) and pt_const), ws)
        assert tuple(got_flags[i].tolist()) == tuple(int(x) for x in want_flags), (i, flags[i])


def test_limits_table_sizes_and_carves_are_pinned(driver):
    line = subprocess.run([str(driver), "--consts"], capture_output=True, text=True, check=True).stdout.split()
    k = dict(zip(line[::2], map(int, line[1::2])))
    assert k["threads"] == M.THREADS == 256 and k["win_threads"] == 64 and k["max_window"] == M.MAX_WINDOW == 64 and k["max_img"] == M.MAX_IMG == 4096
    assert k["max_obs"] == 1 << 22 and k["max_walk"] == 1 << 30
    # load at most 0.5 and room for a claim per lane in flight
    assert (k["img_slots_1"], k["img_slots_512"], k["img_slots_max"], k["sort_len_512"], k["sort_len_max"]) == (512, 1024, 8192, 512, 4096)
    assert k["window_carve"] == (64 + 4) * 4
    # the point table of snk-lmap v1 and the window's prefix sums and starts
    assert k["points_carve_max"] == 32768 * 4 + (2 * 64 + 1) * 4
    # a key and a value per slot, the sort keys, a base per image, the four arrays of a chunk
    assert k["obs_carve_max"] == 8192 * 8 + 4096 * 4 + 4096 * 4 + (4 * 256 + 1) * 4
    # the window and 32 words, then the larger phase: one carve used twice
    assert k["gather_carve_max"] == (64 + 32) * 4 + k["points_carve_max"] <= 160 * 1024
    assert k["gather_carve_ref"] == k["gather_carve_max"] and k["gather_carve_2048_128"] == (64 + 32) * 4 + 4096 * 4 + (2 * 64 + 1) * 4
