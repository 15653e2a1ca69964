"""Host-side mirror of the reference's bag-of-words place recognition over the C ABI, semantics "snk-bow v1" (DESIGN.md section 3g).

* ``Vocabulary`` mirrors ``ORBVocabulary`` as Snake uses it: ``transform`` (reference Snake/Map/Frame.cpp:38-40), ``score``
  (Snake/LoopClosing/LoopDetector.cpp:73), ``size``.
* ``KeyframeDatabase`` mirrors ``Snake::KeyframeDatabase`` (Snake/LoopClosing/KeyframeDatabase.cpp:20-168).
* ``match_bow`` mirrors ``LoopORBmatcher::MatchBoW`` (Snake/LoopClosing/LoopORBMatcher.cpp:121-215).

Everything runs in the HIP library; numpy only carries host buffers and the ``*_dev`` forms take torch tensors that stay in HBM.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .matcher import _Handle, _as_desc, _ptr
from .tracking import FramesDev, bow_features

MAX_FEATURES = 2048
MAX_CANDIDATES = 64
MAX_DEPTH = 16
SHARING_WORD_RATIO = 0.8  # KeyframeDatabase.cpp:71,89
SCORE_RATIO = 0.75


def desc_frames_dev(n, desc) -> FramesDev:
    """A snk_frames_dev that carries only what the bag-of-words entry points read: n [B] int32 and desc [B, cap, 4] int64 (torch
    tensors on the device; they must outlive the calls that use the view)."""
    f = FramesDev()
    f.batch, f.cap = int(desc.shape[0]), int(desc.shape[1])
    f.n, f.desc = n.data_ptr(), desc.data_ptr()
    return f


class Vocabulary:
    """A vocabulary tree in flat arrays (include/snake_hip.h, snk_bow_vocab_create).  ``desc`` is [n_nodes, 4] uint64 or [n_nodes, 32]
    uint8; node 0 is the root."""

    def __init__(self, child_start, child_count, children, desc, word_id, weight, device: int = 0, stream: int | None = None):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.arrays = dict(child_start=np.ascontiguousarray(child_start, np.int32), child_count=np.ascontiguousarray(child_count, np.int32),
                           children=np.ascontiguousarray(children, np.int32), desc=_as_desc(desc),
                           word_id=np.ascontiguousarray(word_id, np.int32), weight=np.ascontiguousarray(weight, np.float64))
        a = self.arrays
        n = len(a["child_start"])
        if not (len(a["child_count"]) == len(a["desc"]) == len(a["word_id"]) == len(a["weight"]) == n):
            raise ValueError("per-node arrays differ in length")
        _lib.check(self._lib.snk_bow_vocab_create(n, _ptr(a["child_start"]), _ptr(a["child_count"]), _ptr(a["children"]), len(a["children"]),
                                                  _ptr(a["desc"]), _ptr(a["word_id"]), _ptr(a["weight"]), int(device),
                                                  C.c_void_p(stream or 0), C.byref(self._h)), "snk_bow_vocab_create")
        w, nn, d = C.c_int(0), C.c_int(0), C.c_int(0)
        _lib.check(self._lib.snk_bow_vocab_size(self._h, C.byref(w), C.byref(nn), C.byref(d)), "snk_bow_vocab_size")
        self.n_words, self.n_nodes, self.depth = int(w.value), int(nn.value), int(d.value)

    @classmethod
    def from_arrays(cls, arrays: dict, device: int = 0, stream: int | None = None) -> "Vocabulary":
        return cls(arrays["child_start"], arrays["child_count"], arrays["children"], arrays["desc"], arrays["word_id"], arrays["weight"],
                   device, stream)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.snk_bow_vocab_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self) -> int:
        """``vocabulary.size()``: the number of words"""
        return self.n_words

    def transform(self, descriptors, levelsup: int = 4) -> dict:
        """``vocabulary.transform(descriptors, bow_vec, bow_feature_vec, levelsup)``: dict(words, values -- bow_vec --, node_id,
        node_start, features -- bow_feature_vec as snk_bow_features takes it --, word_of_feature, node_of_feature)."""
        d = _as_desc(descriptors) if len(descriptors) else np.zeros((0, 4), np.uint64)
        n, cap = len(d), max(len(d), 1)
        words, values = np.zeros(cap, np.int32), np.zeros(cap, np.float64)
        node_id, node_start, features = np.zeros(cap, np.uint32), np.zeros(cap + 1, np.int32), np.zeros(cap, np.int32)
        wof, nof = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        nw, nn = C.c_int(0), C.c_int(0)
        _lib.check(self._lib.snk_bow_transform(self._h, _ptr(d), n, int(levelsup), _ptr(words), _ptr(values), C.byref(nw), _ptr(node_id),
                                               _ptr(node_start), _ptr(features), C.byref(nn), _ptr(wof), _ptr(nof)), "snk_bow_transform")
        nw, nn = int(nw.value), int(nn.value)
        return dict(words=words[:nw].copy(), values=values[:nw].copy(), node_id=node_id[:nn].copy(), node_start=node_start[: nn + 1].copy(),
                    features=features[: int(node_start[nn])].copy(), word_of_feature=wof[:n].copy(), node_of_feature=nof[:n].copy())

    def transform_batch_dev(self, frames: FramesDev, levelsup: int = 4, out: dict | None = None) -> dict:
        """The transform of every frame of a device-resident batch.  Returns (or fills) a dict of torch tensors on the device: words,
        node_id, features, word_of_feature, node_of_feature [B, cap] int32, values [B, cap] float64, node_start [B, cap + 1] int32,
        n_words, n_nodes [B] int32.  Asynchronous on the vocabulary's stream."""
        import torch

        B, cap = int(frames.batch), int(frames.cap)
        if out is None:
            dev = torch.device("cuda", torch.cuda.current_device())
            i32 = dict(dtype=torch.int32, device=dev)
            out = dict(words=torch.zeros((B, cap), **i32), values=torch.zeros((B, cap), dtype=torch.float64, device=dev),
                       n_words=torch.zeros(B, **i32), node_id=torch.zeros((B, cap), **i32), node_start=torch.zeros((B, cap + 1), **i32),
                       features=torch.zeros((B, cap), **i32), n_nodes=torch.zeros(B, **i32), word_of_feature=torch.zeros((B, cap), **i32),
                       node_of_feature=torch.zeros((B, cap), **i32))
        _lib.check(self._lib.snk_bow_transform_batch_dev(
            self._h, C.byref(frames), int(levelsup), out["words"].data_ptr(), out["values"].data_ptr(), out["n_words"].data_ptr(),
            out["node_id"].data_ptr(), out["node_start"].data_ptr(), out["features"].data_ptr(), out["n_nodes"].data_ptr(),
            out["word_of_feature"].data_ptr(), out["node_of_feature"].data_ptr()), "snk_bow_transform_batch_dev")
        return out

    def score(self, a, b) -> float:
        """``vocabulary.score(a, b)``: a, b = (words, values) of two bow_vecs"""
        wa, va = np.ascontiguousarray(a[0], np.int32), np.ascontiguousarray(a[1], np.float64)
        wb, vb = np.ascontiguousarray(b[0], np.int32), np.ascontiguousarray(b[1], np.float64)
        s = C.c_double(0.0)
        _lib.check(self._lib.snk_bow_score(self._h, _ptr(wa), _ptr(va), len(wa), _ptr(wb), _ptr(vb), len(wb), C.byref(s)), "snk_bow_score")
        return float(s.value)

    # ---- the text format of the publicly distributed ORB vocabulary (DBoW2's saveToTextFile), an ASSUMED layout ----
    @staticmethod
    def load_dbow2_text(path) -> dict:
        """Reads ``k L scoring weighting`` then one line per non-root node, ``parent is_leaf b0 .. b31 weight``: node ids in line order
        (the first line is node 1), word ids in the order the leaves appear.  Returns the arrays ``from_arrays`` takes plus
        ``header``.  The layout is assumed from DBoW2's published writer; no file of the reference pins it."""
        with open(path) as f:
            head = f.readline().split()
            if len(head) != 4:
                raise ValueError("vocabulary text: the first line must be `k L scoring weighting`")
            rows = [line.split() for line in f if line.strip()]
        n = len(rows) + 1
        parent, leaf = np.zeros(n, np.int64), np.zeros(n, bool)
        desc, weight = np.zeros((n, 32), np.uint8), np.zeros(n, np.float64)
        for i, r in enumerate(rows, start=1):
            if len(r) != 35:
                raise ValueError(f"vocabulary text: line {i + 1} has {len(r)} fields, not 35")
            parent[i], leaf[i] = int(r[0]), int(r[1]) != 0
            desc[i] = [int(v) for v in r[2:34]]
            weight[i] = float(r[34])
            if not 0 <= parent[i] < n:
                raise ValueError(f"vocabulary text: line {i + 1}: parent {parent[i]} outside the file")
        order = np.argsort(parent[1:], kind="stable") + 1  # children grouped by parent, in line order inside a group
        child_count = np.bincount(parent[1:], minlength=n).astype(np.int32)
        child_start = (np.cumsum(child_count) - child_count).astype(np.int32)
        word_id = np.full(n, -1, np.int32)
        is_leaf = child_count == 0
        if n > 1 and not np.array_equal(is_leaf[1:], leaf[1:]):
            raise ValueError("vocabulary text: the is_leaf column disagrees with the parent column")
        word_id[is_leaf] = np.arange(int(is_leaf.sum()), dtype=np.int32)
        weight[~is_leaf] = 0.0
        return dict(child_start=child_start, child_count=child_count, children=order.astype(np.int32), desc=desc.view("<u8").reshape(n, 4),
                    word_id=word_id, weight=weight, header=(int(head[0]), int(head[1]), int(head[2]), int(head[3])))

    @staticmethod
    def save_dbow2_text(path, arrays: dict, header=None) -> None:
        """Writes the arrays in that layout.  The file numbers nodes in line order, so the tree must already be numbered with every
        parent before its children and the word ids in order of leaf appearance (what ``load_dbow2_text`` returns)."""
        cs, cc, ch = (np.asarray(arrays[k]) for k in ("child_start", "child_count", "children"))
        n = len(cs)
        parent = np.zeros(n, np.int64)
        for i in range(n):
            parent[ch[cs[i]: cs[i] + cc[i]]] = i
        leaves = np.nonzero(cc == 0)[0]
        if not np.array_equal(np.asarray(arrays["word_id"])[leaves], np.arange(len(leaves))):
            raise ValueError("save_dbow2_text: word ids must follow the order of the leaves")
        desc = np.ascontiguousarray(arrays["desc"], np.uint64).view(np.uint8).reshape(n, 32)
        if header is None:
            header = arrays.get("header", (int(cc.max()) if n else 0, 0, 0, 0))
        with open(path, "w") as f:
            f.write(" ".join(str(int(v)) for v in header) + "\n")
            for i in range(1, n):
                f.write(f"{parent[i]} {int(cc[i] == 0)} " + " ".join(str(int(b)) for b in desc[i]) + f" {float(arrays['weight'][i])!r}\n")


class KeyframeDatabase:
    """``KeyframeDatabase`` of the loop closer: one device-resident row (bow_vec) per keyframe."""

    def __init__(self, vocabulary: Vocabulary, max_keyframes: int = 10000, max_words: int = MAX_FEATURES):
        self._lib = _lib.load()
        self.vocabulary = vocabulary  # keeps the handle alive: the database works on its stream
        self._h = C.c_void_p()
        _lib.check(self._lib.snk_bow_db_create(vocabulary._h, int(max_keyframes), int(max_words), C.byref(self._h)), "snk_bow_db_create")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.snk_bow_db_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, kf_id: int, words, values) -> None:
        w, v = np.ascontiguousarray(words, np.int32), np.ascontiguousarray(values, np.float64)
        if len(w) != len(v):
            raise ValueError("words / values length mismatch")
        _lib.check(self._lib.snk_bow_db_add(self._h, int(kf_id), _ptr(w), _ptr(v), len(w)), "snk_bow_db_add")

    def add_batch_dev(self, kf_ids, words, values, n_words) -> None:
        """rows straight from ``Vocabulary.transform_batch_dev``: kf_ids [B] on the host, the rest torch tensors on the device"""
        ids = np.ascontiguousarray(kf_ids, np.int32)
        _lib.check(self._lib.snk_bow_db_add_batch_dev(self._h, _ptr(ids), len(ids), words.data_ptr(), values.data_ptr(), n_words.data_ptr(),
                                                      int(words.shape[1])), "snk_bow_db_add_batch_dev")

    def remove(self, kf_id: int) -> None:
        _lib.check(self._lib.snk_bow_db_remove(self._h, int(kf_id)), "snk_bow_db_remove")

    def query(self, words, values, exclude=(), sharing_word_ratio=SHARING_WORD_RATIO, score_ratio=SCORE_RATIO, min_score=0.0,
              max_candidates=10):
        """(ids, scores, common-word counts) of the candidates, best first"""
        w, v = np.ascontiguousarray(words, np.int32), np.ascontiguousarray(values, np.float64)
        ex = np.ascontiguousarray(exclude, np.int32).reshape(-1)
        k = int(max_candidates)
        ids, sc, cm = np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.float64), np.zeros(max(k, 1), np.int32)
        n = C.c_int(0)
        _lib.check(self._lib.snk_bow_db_query(self._h, _ptr(w), _ptr(v), len(w), _ptr(ex), len(ex), float(sharing_word_ratio), float(score_ratio),
                                              float(min_score), k, _ptr(ids), _ptr(sc), _ptr(cm), C.byref(n)), "snk_bow_db_query")
        return ids[: n.value].copy(), sc[: n.value].copy(), cm[: n.value].copy()

    def detect_loop_candidates(self, bow_vec, connected, min_score: float, max_candidates: int):
        """``DetectLoopCandidates(bv, connected_keyframes, minScore, max_candidates)``: [(keyframe id, score)]"""
        ids, sc, _ = self.query(bow_vec[0], bow_vec[1], connected, SHARING_WORD_RATIO, SCORE_RATIO, min_score, max_candidates)
        return list(zip(ids.tolist(), sc.tolist()))

    def detect_relocalization_candidates(self, bow_vec, min_score: float, max_candidates: int):
        """``DetectRelocalizationCandidates(bv, minScore, max_candidates)``: the reference passes 0 for the score floor (:89)"""
        ids, sc, _ = self.query(bow_vec[0], bow_vec[1], (), SHARING_WORD_RATIO, SCORE_RATIO, 0.0, max_candidates)
        return list(zip(ids.tolist(), sc.tolist()))

    def query_batch_dev(self, words, values, n_words, exclude=None, n_exclude=None, sharing_word_ratio=SHARING_WORD_RATIO,
                        score_ratio=SCORE_RATIO, min_score=0.0, max_candidates=10, out: dict | None = None) -> dict:
        """Q queries in one launch pair; all arguments torch tensors on the device (words / values [Q, cap], n_words [Q], exclude
        [Q, e_cap] int32 with n_exclude [Q], or None).  Returns device tensors ids, common [Q, max_candidates] int32, scores
        [Q, max_candidates] float64, n [Q] int32."""
        import torch

        Q, k = int(words.shape[0]), int(max_candidates)
        if out is None:
            out = dict(ids=torch.zeros((Q, k), dtype=torch.int32, device=words.device), scores=torch.zeros((Q, k), dtype=torch.float64, device=words.device),
                       common=torch.zeros((Q, k), dtype=torch.int32, device=words.device), n=torch.zeros(Q, dtype=torch.int32, device=words.device))
        _lib.check(self._lib.snk_bow_db_query_batch_dev(
            self._h, Q, words.data_ptr(), values.data_ptr(), n_words.data_ptr(), int(words.shape[1]),
            exclude.data_ptr() if exclude is not None else None, n_exclude.data_ptr() if exclude is not None else None,
            int(exclude.shape[1]) if exclude is not None else 0, float(sharing_word_ratio), float(score_ratio), float(min_score), k,
            out["ids"].data_ptr(), out["scores"].data_ptr(), out["common"].data_ptr(), out["n"].data_ptr()), "snk_bow_db_query_batch_dev")
        return out

    def detect_loop_candidates_batch_dev(self, words, values, n_words, connected, n_connected, min_score: float, max_candidates: int) -> dict:
        return self.query_batch_dev(words, values, n_words, connected, n_connected, SHARING_WORD_RATIO, SCORE_RATIO, min_score, max_candidates)

    def detect_relocalization_candidates_batch_dev(self, words, values, n_words, max_candidates: int) -> dict:
        return self.query_batch_dev(words, values, n_words, None, None, SHARING_WORD_RATIO, SCORE_RATIO, 0.0, max_candidates)


class LoopMatcher(_Handle):
    """``LoopORBmatcher``: MatchBoW on a matcher handle."""

    def match_bow(self, desc1, has_mp1, bow1, desc2, has_mp2, bow2, threshold: int = 50, ratio: float = 0.75):
        """``MatchBoW(kf1, kf2, matches, threshold, ratio)``; bow = (node_id, node_start, features).  Returns (match12 [n1] int32 -- the
        feature of keyframe 2 or -1 --, the number of matches)."""
        d1 = _as_desc(desc1) if len(desc1) else np.zeros((0, 4), np.uint64)
        d2 = _as_desc(desc2) if len(desc2) else np.zeros((0, 4), np.uint64)
        h1, h2 = np.ascontiguousarray(has_mp1, np.uint8), np.ascontiguousarray(has_mp2, np.uint8)
        if len(h1) != len(d1) or len(h2) != len(d2):
            raise ValueError("has_mp / descriptor length mismatch")
        b1, keep1 = bow_features(bow1)
        b2, keep2 = bow_features(bow2)
        m12 = np.full(max(len(d1), 1), -1, np.int32)
        n = C.c_int(0)
        _lib.check(self._lib.snk_match_loop_bow(self._h, _ptr(d1), _ptr(h1), len(d1), C.byref(b1), _ptr(d2), _ptr(h2), len(d2), C.byref(b2),
                                                int(threshold), float(ratio), _ptr(m12), C.byref(n)), "snk_match_loop_bow")
        return m12[: len(d1)].copy(), int(n.value)

    def match_bow_batch_dev(self, frames1: FramesDev, frames2: FramesDev, has_mp1, has_mp2, bow1: dict, bow2: dict, match12, pairs, n_pairs,
                            threshold: int = 50, ratio: float = 0.75) -> None:
        """Every keyframe pair of a device-resident batch; bow1 / bow2 are the dicts ``transform_batch_dev`` returns, has_mp [B, cap]
        uint8; out: match12 [B, cap1] int32, pairs [B, cap1, 2] int32, n_pairs [B] int32 (what ``solve_pairs_batch_dev`` takes)."""
        _lib.check(self._lib.snk_match_loop_bow_batch_dev(
            self._h, C.byref(frames1), C.byref(frames2), has_mp1.data_ptr(), has_mp2.data_ptr(), bow1["node_id"].data_ptr(),
            bow1["node_start"].data_ptr(), bow1["features"].data_ptr(), bow1["n_nodes"].data_ptr(), bow2["node_id"].data_ptr(),
            bow2["node_start"].data_ptr(), bow2["features"].data_ptr(), bow2["n_nodes"].data_ptr(), int(threshold), float(ratio),
            match12.data_ptr(), pairs.data_ptr(), n_pairs.data_ptr()), "snk_match_loop_bow_batch_dev")


def match_bow(desc1, has_mp1, bow1, desc2, has_mp2, bow2, threshold: int = 50, ratio: float = 0.75, device: int = 0):
    """One MatchBoW call on a handle of its own."""
    m = LoopMatcher(device)
    try:
        return m.match_bow(desc1, has_mp1, bow1, desc2, has_mp2, bow2, threshold, ratio)
    finally:
        m.close()
