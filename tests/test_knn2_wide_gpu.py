"""GPU: the wide form of the matrix-core kNN-2 kernel (two query blocks per wavefront, 256 queries per workgroup), forced by
SNK_BF_MFMA_WIDE=1 in ONE child process (the switch is read once) that runs every case of tests/knn2_wide_cases.py; every field of
every snk_knn2 row is compared with the oracle's bf_knn2 here.  A second child under SNK_BF_MFMA_WIDE=0 runs the narrow form on one
case: the two forms agree with each other and with the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

import forms
import knn2_wide_cases as KC
from helpers import knn_to_array

pytestmark = pytest.mark.gpu


def run_child(out, names, **switches):
    env = {k: v for k, v in os.environ.items() if k not in ("SNK_BF_MFMA_WIDE", "SNK_BF_MFMA_NO_SHORT", "SNK_BF_NO_MFMA")}
    r = subprocess.run([sys.executable, str(KC.TESTS / "knn2_wide_cases.py"), str(out)] + list(names), env=dict(env, **switches),
                       capture_output=True, text=True, cwd=str(KC.TESTS.parent), timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return np.load(out)


@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    return run_child(tmp_path_factory.mktemp("knn2_wide") / "wide.npz", [], SNK_BF_MFMA_WIDE="1")


@pytest.fixture(scope="module")
def want(orc):
    """The oracle's answer to every case, once: rows past a frame's count keep the -7 the output starts with."""
    out = {}
    for name, c in KC.cases().items():
        if c[0] == "host":
            out[name] = knn_to_array(orc.bf_knn2(c[1], c[2]))
            continue
        _, q, nq, t, nt = c
        w = np.full((q.shape[0], q.shape[1], 4), -7, np.int32)
        for b in range(q.shape[0]):
            n, m = min(int(nq[b]), q.shape[1]), min(int(nt[b]), t.shape[1])  # a count above the capacity is clamped
            w[b, :n] = knn_to_array(orc.bf_knn2(q[b, :n], t[b, :m]))
        out[name] = w
    return out


def check(want, got, name):
    assert got.shape == want[name].shape and np.array_equal(got, want[name]), name


def test_block_edges_host_entry(wide, want):
    """nq on both sides of a wavefront's 64 and a workgroup's 256 queries, nt on both sides of a tile and with a third, one-row tile."""
    cs = KC.host_edges()
    assert len(cs) == len(KC.EDGE_NQ) * len(KC.EDGE_NT) == 24
    for name in cs:
        check(want, wide[name], name)


def test_block_edges_batched_entry(wide, want):
    """nq_cap = 257, nt_cap = 65, nine frames: no queries, no trains, one query in the second workgroup, counts above both capacities."""
    (name, c), = KC.batch_edges().items()
    assert 0 in c[2] and 0 in c[4] and c[2][0] == KC.W + 1 and c[2][8] > KC.W + 1 and c[4][8] > 2 * KC.T + 1
    check(want, wide[name], name)


def tie_rows(got):
    for k, rows in enumerate(KC.TIE_ROWS.values()):
        for i, row in enumerate((3 + k, 40 + k, 70 + k, 130 + k)):  # both places are duplicates, the lower indices, at the same distance
            assert got[row].tolist() == [rows[0], i + 1, rows[1], i + 1], (rows, row)


def test_ties_go_to_the_lower_index(wide, want):
    check(want, wide["ties"], "ties")
    tie_rows(wide["ties"])


@pytest.mark.parametrize("finite_row", [37, 69])
def test_distance_255_against_256(wide, want, finite_row):
    """All-zero queries in both query blocks of a wavefront (rows 0 - 63) and in the next; all-one trains are their complement (256:
    never a neighbour) but for one row at 255."""
    got = wide[f"d255_{finite_row}"]
    assert got.tolist() == [[finite_row, 255, -1, 256]] * 70
    check(want, got, f"d255_{finite_row}")


def test_index_field_at_the_largest_train_set(wide, want):
    got = wide["index_field"]
    assert got.shape[0] == KC.Q + 1 and (got == [0, 1, forms.NT_MAX - 1, 1]).all()
    check(want, got, "index_field")


@pytest.mark.parametrize("nt", [KC.SHORT_NT, KC.SHORT_NT + 1])
def test_last_index_on_both_sides_of_the_key_width(wide, want, nt):
    """8192 trains: 13-bit keys with the index field full; 8193: the 20-bit keys."""
    got = wide[f"keys_{nt}"]
    assert (got == [0, 1, nt - 1, 1]).all()
    check(want, got, f"keys_{nt}")


def test_narrow_and_wide_agree(wide, want, tmp_path):
    narrow = run_child(tmp_path / "narrow.npz", ["agree"], SNK_BF_MFMA_WIDE="0")["agree"]
    assert np.array_equal(narrow, wide["agree"])
    check(want, narrow, "agree")


@pytest.mark.parametrize("form", ["1", "0"], ids=["wide", "narrow"])
def test_every_case_on_20_bit_keys(wide, want, tmp_path, form):
    """bf_knn2_mfma_kernel<2, false> and <1, false> -- what a train capacity above 8192 runs -- forced by SNK_BF_MFMA_NO_SHORT=1 on the
    small cases as well (block edges on both entries, ragged / zero / clamped counts, ties, 255 against 256, both sides of the key
    width, the agreement case): equal to the oracle and to what the 13-bit keys gave."""
    names = ["edges", "ties", "d255", "key_width", "agree"]
    got = run_child(tmp_path / "long.npz", names, SNK_BF_MFMA_WIDE=form, SNK_BF_MFMA_NO_SHORT="1")
    assert sorted(got.files) == sorted(KC.cases(names))
    for name in got.files:
        check(want, got[name], name)
        assert np.array_equal(got[name], wide[name]), name
    tie_rows(got["ties"])
