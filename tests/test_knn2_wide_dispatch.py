"""CPU: the choices inside Knn2Form::mfma (snake_slam_amd/csrc/dispatch.hpp) -- one or two query blocks per wavefront
(knn2_mfma_wide) and 13- or 20-bit keys (knn2_mfma_short) -- built with plain g++ from a driver of their own, and knn2_form still as
tests/forms.py has it."""
import subprocess

import pytest

import forms


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = tmp_path_factory.mktemp("knn2_wide") / "knn2_wide_driver"
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{forms.ROOT / 'snake_slam_amd' / 'csrc'}",
           str(forms.ROOT / "tests" / "cpp" / "knn2_wide_driver.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(queries):
        r = subprocess.run([str(exe)] + [":".join([e] + [str(a) for a in args]) for e, args in queries], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        out = r.stdout.split()
        assert len(out) == len(queries)
        return out

    return run


def test_wide_form_from_its_threshold_on(ask):
    """Wide from BF_MFMA_WIDE_MIN_WGS workgroups of 256 queries on.  Measured with 1000 queries per frame: narrow ahead at 1 and 8
    frames, the two equal at 64 (256 workgroups), wide ahead at 128 (512 workgroups), 256 and 1024; nothing between 256 and 512
    workgroups was measured.  The bench batch is wide, one frame per call narrow."""
    wgs = int(ask([("const", ("BF_MFMA_WIDE_MIN_WGS",))])[0])
    assert wgs == 512
    q = [("wide", (1000, 1000, 1024, -1)), ("wide", (1000, 1000, 1, -1)), ("wide", (1000, 1000, 64, -1)), ("wide", (1000, 1000, 256, -1)),
         ("wide", (1000, 1000, wgs // 4, -1)), ("wide", (1000, 1000, wgs // 4 - 1, -1)),      # ceil(1000 / 256) = 4 workgroups per frame
         ("wide", (256, 1000, wgs, -1)), ("wide", (256, 1000, wgs - 1, -1)), ("wide", (257, 1000, wgs // 2, -1)),
         ("wide", (24, 24, wgs, -1)), ("wide", (1 << 30, 24, 4096, -1)),                         # batch * workgroups past 2^31
         ("wide", (1000, 1000, 1, 1)), ("wide", (24, 24, 1, 1)), ("wide", (1000, 1000, 1024, 0))]  # SNK_BF_MFMA_WIDE forces either
    assert ask(q) == ["1", "0", "0", "1", "1", "0", "1", "0", "1", "1", "1", "1", "1", "0"]


def test_short_keys_up_to_their_index_field(ask):
    nt = int(ask([("const", ("BF_MFMA_SHORT_NT",))])[0])
    assert nt == 8192
    q = [("short", (24, 1)), ("short", (1000, 1)), ("short", (nt, 1)), ("short", (nt + 1, 1)), ("short", (forms.NT_MAX, 1)), ("short", (1000, 0))]
    assert ask(q) == ["1", "1", "1", "0", "0", "0"]


def test_knn2_form_is_what_the_table_says(ask):
    rows = [(s, f) for e, s, f in forms.FORMS if e == "knn2"]
    assert len(rows) >= 13
    assert ask([("knn2", s) for s, _ in rows]) == [f for _, f in rows]
