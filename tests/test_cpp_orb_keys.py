"""CPU: orb_keys.hpp -- the subdivision keys of the quadtree distribution -- built with plain g++.  The driver checks the table form
(two table entries and a bit-interleave, what distribute_kernel computes) against the header's loop form for every pixel of every size;
this test compares a seeded sample of the table-form keys with the oracle's orc_point_key."""
import subprocess
from pathlib import Path

import pytest

from oracle import oracle as orc

ROOT = Path(__file__).resolve().parent.parent
# W x H of a level without its border: the four EuRoC levels, KITTI level 0 (more than one root), taller than wide, the degenerate
# cases, and both sides of a power of two
SIZES = [(720, 448), (595, 368), (490, 301), (403, 246), (1209, 344), (88, 168), (1, 1), (2, 3), (3, 2), (1, 40), (40, 1), (256, 256),
         (257, 255)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("orb_keys") / "orb_keys_driver"
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{ROOT / 'snake_slam_amd' / 'csrc'}", str(ROOT / "tests" / "cpp" / "orb_keys_driver.cpp"),
           "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def sample(driver):
    r = subprocess.run([str(driver)] + [str(v) for s in SIZES for v in s], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr  # tables == loop form at every (x, y) of every size
    rows = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert all(len(row) == 5 for row in rows)
    return rows


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_table_keys_equal_the_oracle(sample, size):
    W, H = size
    rows = [r for r in sample if (r[0], r[1]) == size]
    assert len(rows) == min(64, W * H)
    for _, _, x, y, key in rows:
        assert key == orc.point_key(x, y, W, H), f"{W} x {H}: key of ({x}, {y})"
    if W * H >= 64:
        assert {(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)} <= {(r[2], r[3]) for r in rows}
