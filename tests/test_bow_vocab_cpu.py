"""CPU: snk_bow_vocab_create validates a vocabulary on the host before it touches a device -- a cycle, an orphan node, a leaf without a
word id, a duplicated word id, depth 17 and a NaN weight are refused with SNK_ERR_INVALID_ARG and a reason, while a sound tree gets past
the validation (and then needs a device) --, the host-only entry points check their arguments, and the text format of the public ORB
vocabulary (an assumed layout) survives a round trip of a file this test writes."""
import ctypes as C

import numpy as np
import pytest

import bow_numpy as B

INVALID_ARG = 1


def create(arrays):
    from snake_slam_amd import _lib

    lib = _lib.load()
    a = {k: np.ascontiguousarray(arrays[k], t) for k, t in (("child_start", np.int32), ("child_count", np.int32), ("children", np.int32),
                                                             ("desc", np.uint64), ("word_id", np.int32), ("weight", np.float64))}
    h = C.c_void_p()
    p = lambda x: x.ctypes.data if x.size else None
    rc = lib.snk_bow_vocab_create(len(a["child_start"]), p(a["child_start"]), p(a["child_count"]), p(a["children"]), len(a["children"]),
                                  p(a["desc"]), p(a["word_id"]), p(a["weight"]), 0, None, C.byref(h))
    text = lib.snk_last_error().decode()
    if rc == 0:
        lib.snk_bow_vocab_destroy(h)
    return rc, text


def chain(depth):
    """root -> one child -> ... -> one leaf at `depth`"""
    n = depth + 1
    return dict(child_start=np.arange(n), child_count=np.array([1] * depth + [0]), children=np.arange(1, n), desc=np.zeros((n, 4), np.uint64),
                word_id=np.array([-1] * depth + [0]), weight=np.array([0.0] * depth + [1.0]))


def test_a_sound_tree_passes_the_validation():
    for arrays in (B.hand_vocab().arrays(), B.vocab("irregular").arrays(), chain(16)):
        rc, text = create(arrays)
        assert rc != INVALID_ARG, text  # SNK_OK on a GPU, SNK_ERR_NO_DEVICE without one


def broken():
    h = B.hand_vocab().arrays()
    out = {}
    # nodes 4 and 5 are each other's only child, unreachable from the root; node 1 keeps one child so that children == nodes - 1
    c = dict(h, child_count=h["child_count"].copy(), child_start=h["child_start"].copy(), children=h["children"].copy(), word_id=h["word_id"].copy())
    c["child_count"][[1, 4, 5]] = 1
    c["child_start"][[1, 4, 5]] = [3, 4, 5]
    c["children"][3:6] = [6, 5, 4]
    c["word_id"][[4, 5]] = -1
    c["word_id"][6:] = np.arange(7)
    out["cycle"] = (c, "cycle")
    o = dict(h, children=h["children"].copy())
    o["children"][11] = 11  # node 11 twice, node 12 an orphan
    out["orphan"] = (o, "child of two nodes")
    w = dict(h, word_id=h["word_id"].copy())
    w["word_id"][6] = -1
    out["leaf_without_word"] = (w, "leaf without a word id")
    d = dict(h, word_id=h["word_id"].copy())
    d["word_id"][6] = 1
    out["duplicate_word"] = (d, "used twice")
    out["depth_17"] = (chain(17), "depth above 16")
    n = dict(h, weight=h["weight"].copy())
    n["weight"][7] = np.nan
    out["nan_weight"] = (n, "weight")
    m = dict(h, weight=h["weight"].copy())
    m["weight"][7] = -1.0
    out["negative_weight"] = (m, "weight")
    return out


BROKEN = broken()


@pytest.mark.parametrize("name", list(BROKEN))
def test_validation_refuses(name):
    arrays, reason = BROKEN[name]
    rc, text = create(arrays)
    assert rc == INVALID_ARG and reason in text, (rc, text)


def test_orphan_without_a_double_parent_is_refused_too():
    h = B.hand_vocab().arrays()
    o = dict(h, child_count=h["child_count"].copy())
    o["child_count"][3] = 2  # node 12 is in children[] but in nobody's list
    rc, text = create(o)
    assert rc == INVALID_ARG and "orphan" in text, (rc, text)


def test_null_handles_are_error_codes():
    from snake_slam_amd import _lib

    lib = _lib.load()
    s, n = C.c_double(0), C.c_int(0)
    assert lib.snk_bow_vocab_size(None, None, None, None) == INVALID_ARG
    assert lib.snk_bow_score(None, None, None, 0, None, None, 0, C.byref(s)) == INVALID_ARG
    assert lib.snk_bow_db_create(None, 10, 10, C.byref(C.c_void_p())) == INVALID_ARG
    assert lib.snk_bow_db_add(None, 0, None, None, 0) == INVALID_ARG and lib.snk_bow_db_remove(None, 0) == INVALID_ARG
    assert lib.snk_bow_db_query(None, None, None, 0, None, 0, 0.8, 0.75, 0.0, 10, None, None, None, C.byref(n)) == INVALID_ARG
    assert lib.snk_bow_vocab_destroy(None) == 0 and lib.snk_bow_db_destroy(None) == 0


@pytest.mark.parametrize("name", ["k10_L3", "irregular", "single_level"])
def test_dbow2_text_round_trip(tmp_path, name):
    from snake_slam_amd.bow import Vocabulary

    V = B.vocab(name)
    path = tmp_path / "voc.txt"
    Vocabulary.save_dbow2_text(path, V.arrays(), header=(10, V.L, 0, 0))
    first = path.read_text().splitlines()
    assert first[0] == f"10 {V.L} 0 0" and len(first) == len(V.child_count) and len(first[1].split()) == 35
    back = Vocabulary.load_dbow2_text(path)
    assert back["header"] == (10, V.L, 0, 0)
    for k, v in V.arrays().items():
        if k == "desc":  # the root has no line in the file: its descriptor, which no descent reads, comes back as zeros
            assert np.array_equal(back[k][1:], v[1:]) and not back[k][0].any()
        else:
            assert np.array_equal(back[k], v), k
    assert back["weight"].dtype == np.float64 and np.array_equal(back["weight"], V.weight)  # repr round trip: exact
    again = tmp_path / "voc2.txt"
    Vocabulary.save_dbow2_text(again, back)
    assert again.read_text() == path.read_text()
