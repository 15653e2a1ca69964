"""CPU: snake_slam_amd/csrc/handover_core.hpp compiled with plain g++ (no HIP) into tests/cpp/handover_core_driver.cpp.  The driver builds
every problem twice -- the way the host builder's fill pass does and the way the kernels behind snk_ba_set_problems_dev walk it (chunks of
256 observations ranked by ho_chunk_rank, one cursor writer per point and chunk, the dup rule on the sorted runs) -- and fails if the two
differ; what it writes must equal the numpy restatement (tests/handover_numpy.py): the valid mask, the stable order by point, the
free-camera indices, dup and k > 8.  The plan is pinned: the carves stay inside 160 KiB at the limit, and the take / stage decision flips
between the limit and the limit + 1."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import handover_numpy as M

ROOT = Path(__file__).resolve().parent.parent


def build(out: Path, extra=()):
    exe = out / "handover_core_driver"
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", *extra, f"-I{ROOT / 'include'}", f"-I{ROOT / 'snake_slam_amd' / 'csrc'}",
           str(ROOT / "tests" / "cpp" / "handover_core_driver.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("handover_core"))


def problems():
    rng = np.random.RandomState(5)
    P = []

    def add(img_const, pt_const, obs_img, obs_pt):
        P.append((np.asarray(img_const, np.int32), np.asarray(pt_const, np.int32), np.asarray(obs_img, np.int32), np.asarray(obs_pt, np.int32)))

    add([0, 1, 0], [0, 1], [], [])                                        # no observations
    add([], [], [], [])                                                   # nothing at all
    add([1, 1], [1, 1, 1], [0, 1, 0, 1], [0, 1, 2, 0])                    # all invalid: every pair is constant
    add([0, 0], [0, 0], [-1, 2, 0, 1], [0, 1, -1, 2])                     # all invalid: index -1 and index == n
    add([0, 1, 0], [0, 1, 0], [0, 1, 2, -1, 3, 1, 1, 0, 2], [0, 1, 2, 0, 0, 1, 1, 3, -1])  # both-constant pairs and bad indices in the middle
    n = 3 * M.THREADS + 5
    add([0] * 7 + [1] * 3, [0], rng.randint(0, 10, n), np.zeros(n))      # one point holds every observation, over three chunks
    add([0, 0, 1], [0, 0, 0], [0, 1, 2, 0, 1], [0, 0, 0, 1, 0])           # camera 1 twice on point 0
    add([0, 0, 1], [0, 0, 0], [2, 2, 0, 1], [0, 0, 0, 0])                 # a CONSTANT camera twice on a point: no dup
    add([0] * 9 + [1], [0, 0], list(range(8)) + [9] + list(range(9)), [0] * 9 + [1] * 9)   # exactly 8 free (+1 constant) and exactly 9
    add([0] * 8 + [1], [0, 0], list(range(8)) + [8, 8], [0] * 8 + [0, 1])                  # exactly 8 free: k > 8 stays off
    add([0] * 3, [0, 0], [0] * (M.MAX_RUN + 1) + [1] * M.MAX_RUN, [0] * (M.MAX_RUN + 1) + [1] * M.MAX_RUN)  # a run of MAX_RUN + 1 and one of MAX_RUN
    add([0] * 2, [0], [0] * M.MAX_RUN, [0] * M.MAX_RUN)                   # a run of exactly MAX_RUN
    add([0] * 600, [0] * 3, rng.randint(0, 600, 40), rng.randint(0, 3, 40))  # more than 512 free cameras: the dup rule is off
    add(np.r_[[0] * 513], [0], [7, 7], [0, 0])                             # ... even where a camera is there twice
    add(np.r_[[0] * 512], [0], [7, 7], [0, 0])                             # 512: on
    for n_img, n_pt, n_obs in ((1, 1, 1), (5, 40, 255), (5, 40, 256), (5, 40, 257), (12, 300, 1500), (40, 7, 2000), (3, 2000, 700), (64, 64, 4096)):
        oi, op = rng.randint(-1, n_img + 1, n_obs), rng.randint(-1, n_pt + 1, n_obs)
        add(rng.rand(n_img) < 0.3, rng.rand(n_pt) < 0.2, oi, op)
    return P


def test_core_statements_equal_the_restatement(driver, tmp_path):
    P = problems()
    blob = [np.array([len(P)], np.int32)]
    for ic, pc, oi, op in P:
        blob += [np.array([len(ic), len(pc), len(oi)], np.int32), ic, pc, oi, op]
    np.concatenate(blob).astype(np.int32).tofile(tmp_path / "in.bin")
    r = subprocess.run([str(driver), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(tmp_path / "out.bin", np.int32)
    at = 0
    seen = dict(dup=0, k_over8=0, long_run=0, partial=0)
    for k, (ic, pc, oi, op) in enumerate(P):
        w = M.fill(ic, pc, oi, op)
        head = got[at:at + 5].tolist()
        at += 5
        assert head == [w["nfc"], w["no"], w["k_over8"], w["dup"], w["long_run"]], (k, head)
        for name, n in (("cam_idx", len(ic)), ("pt_start", len(pc) + 1), ("valid", len(oi)), ("order", w["no"]), ("o_cam", w["no"])):
            assert got[at:at + n].tolist() == w[name].tolist(), (k, name)
            at += n
        for f in ("dup", "k_over8", "long_run"):
            seen[f] += w[f]
        seen["partial"] += 0 < w["no"] < len(oi)
    assert at == len(got)
    assert seen["dup"] >= 2 and seen["k_over8"] >= 2 and seen["long_run"] == 1 and seen["partial"] >= 5
    # the edge problems say what they were written for
    flags = [M.fill(*p) for p in P]
    assert [f["no"] for f in flags[:4]] == [0, 0, 0, 0]
    assert flags[6]["dup"] == 1 and flags[7]["dup"] == 0
    assert flags[8]["k_over8"] == 1 and flags[9]["k_over8"] == 0
    assert flags[10]["long_run"] == 1 and flags[11]["long_run"] == 0
    assert flags[13]["dup"] == 0 and flags[14]["dup"] == 1


def test_the_plan_is_pinned(driver):
    line = subprocess.run([str(driver), "--consts"], capture_output=True, text=True, check=True).stdout.split()
    k = dict(zip(line[::2], map(int, line[1::2])))
    assert k["threads"] == M.THREADS == 256 and k["max_pts"] == M.MAX_PTS == 8192 and k["max_run"] == M.MAX_RUN == 1024
    assert k["dup_max_cams"] == M.DUP_MAX_CAMS == 512 and k["big_max_free"] == 8
    # two words per point beside the scan's words; a word per point beside a chunk's keys
    assert k["count_carve_max"] == 16 * 4 + 8192 * 8 and k["fill_carve_max"] == 16 * 4 + 256 * 4 + 8192 * 4
    assert k["carve_max"] == max(k["count_carve_max"], k["fill_carve_max"]) <= 160 * 1024
    assert 2 * k["count_carve_max"] <= 160 * 1024  # two workgroups of the count kernel on a compute unit at the limit
    assert k["count_carve_1000"] == 64 + 8000 and k["fill_carve_1000"] == 64 + 1024 + 4000
    assert (k["takes_at_limit"], k["takes_past_limit"]) == (1, 0) and (k["run_at_limit"], k["run_past_limit"]) == (1, 0)
    assert (k["dup_words_512"], k["dup_words_513"], k["dup_words_65"]) == (8, 0, 2)
    # the limit + 1 is a row snk_ba_set_problems_dev accepts (pt_cap may be 16 384): the staged path is reachable
    text = (ROOT / "include" / "snake_hip.h").read_text()
    assert "#define SNK_LMAP_MAX_PTS 16384" in text and k["max_pts"] + 1 <= 16384


def test_driver_is_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = build(tmp_path, extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    rng = np.random.RandomState(9)
    ic, pc = (rng.rand(9) < 0.3).astype(np.int32), (rng.rand(50) < 0.2).astype(np.int32)
    oi, op = rng.randint(-1, 10, 700).astype(np.int32), rng.randint(-1, 51, 700).astype(np.int32)
    np.concatenate([np.array([1, 9, 50, 700], np.int32), ic, pc, oi, op]).tofile(tmp_path / "in.bin")
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    w = M.fill(ic, pc, oi, op)
    got = np.fromfile(tmp_path / "out.bin", np.int32)
    assert got[:5].tolist() == [w["nfc"], w["no"], w["k_over8"], w["dup"], w["long_run"]] and got[-w["no"]:].tolist() == w["o_cam"].tolist()
