"""GPU: the back-end entry points outside a fresh handle that one module has to itself (tests/backend_cases.py has the seams).

* poison: every seam with SNK_DEBUG_POISON=1 -- fresh device scratch and fresh pinned staging memory filled with 0xCD -- in four child
  processes (the switch is read once);
* one handle: the seams that run on a snk_matcher, all on ONE handle, interleaved in the reference's frame order and in a seeded
  shuffle, and the three pieces of state a handle keeps between calls ("One handle, many entry points");
* growth: a small call, a call that needs more scratch than the handle's buffers hold after create (they are freed and reallocated;
  the library's allocation count confirms it), the small call again -- on one handle.

Everything is compared byte for byte with the seam's result on fresh handles of its own, which the parity suites pin to the numpy
restatements: the kernels are deterministic, so there is no tolerance."""
import numpy as np
import pytest

import backend_cases as BC
from helpers import SEED

pytestmark = pytest.mark.gpu

# Tracking's order inside a frame, then relocalisation, local mapping and loop closing (reference System: Preprocess -> TrackingCoarse /
# TrackingFine, whose local map is lmap -> TrackBruteForce -> LocalMapping, whose local BA window is scene -> LoopClosing)
FRAME_ORDER = ("stereo", "track", "pose", "lmap", "knn2", "p3p", "tri", "mappoint", "covis", "scene", "bow", "sim3")


def where(got, want):
    if len(got) != len(want):
        return f"{len(got)} bytes, {len(want)} expected"
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    d = np.nonzero(a != b)[0]
    return f"{len(d)} of {len(a)} bytes differ, the first at {d[0]}" if len(d) else "equal"


@pytest.mark.parametrize("group", list(BC.GROUPS))
def test_poisoned_scratch_changes_nothing(tmp_path, group):
    from backend_children import run_child

    want = {name: BC.solo_bytes(name) for name in BC.GROUPS[group]}
    out = tmp_path / "poison.npz"
    run_child(group, out, SNK_DEBUG_POISON="1")
    got = np.load(out)
    for name in BC.GROUPS[group]:
        for k in range(3):
            assert got[f"{name}_{k}"].tobytes() == want[name][k], (name, k, where(got[f"{name}_{k}"].tobytes(), want[name][k]))


class OneHandle:
    """every matcher seam's wrappers on the snk_matcher of the knn2 seam's BruteForceMatcher, all on one stream"""

    def __enter__(self):
        import torch

        self.st = torch.cuda.Stream()
        self.H = {name: BC.SEAMS[name][0](0, self.st) for name in BC.MATCHER_SEAMS}
        self.owner = self.H["knn2"]["objs"][0]
        self.adopters = [o for name in BC.MATCHER_SEAMS for o in self.H[name]["matchers"]]
        BC.share_handle(self.owner, self.adopters)
        assert len({o._h.value for o in self.adopters}) == 1
        return self

    def run(self, name, k):
        return BC.run_on_matcher(name)(self.H[name], k)

    def want(self, name, k):
        return BC.solo_bytes("bow", BC.run_bow_match)[k] if name == "bow" else BC.solo_bytes(name)[k]

    def __exit__(self, *exc):
        BC.release_adopters(self.owner, self.adopters)
        for H in self.H.values():
            BC.close_handles(H)  # the adopters' close() is a no-op: their _h is None
        return False


@pytest.mark.parametrize("order", ["frame", "shuffled"])
def test_every_matcher_seam_on_one_handle(order):
    assert sorted(FRAME_ORDER) == sorted(BC.MATCHER_SEAMS)
    names = list(FRAME_ORDER)
    if order == "shuffled":
        names = [names[i] for i in np.random.default_rng(SEED + 77).permutation(len(names))]
        assert names != list(FRAME_ORDER)
    with OneHandle() as one:
        got = [(name, k, one.run(name, k)) for k in range(3) for name in names]
        for name, k, b in got:
            assert b == one.want(name, k), (order, name, k, where(b, one.want(name, k)))


def test_handle_state_survives_the_calls_in_between():
    """The three pieces of state a snk_matcher keeps between calls, each with other entry points called in between: the kNN-2 result
    filterMatches works on (it lives with the caller: the call takes it as an argument), the frame bound by snk_match_bind_frame (it has
    a buffer of its own, which no other entry point touches) and the Sim3 iteration table (keyed by the parameters it was filled under)."""
    from snake_slam_amd import SnakeHipError

    others = ("p3p", "covis", "stereo", "mappoint", "bow", "tri", "pose")
    with OneHandle() as one:
        for k in range(3):
            BC.knn2_match(one.H["knn2"], k)
            BC.track_bind(one.H["track"], k)
            for name in others + ("sim3",):
                assert one.run(name, k) == one.want(name, k), (name, k)
            got = BC.track_search(one.H["track"], k)
            assert got == one.want("track", k), ("bound frame", k, where(got, one.want("track", k)))
            got = BC.knn2_filter(one.H["knn2"], k)
            assert got == one.want("knn2", k), ("filterMatches", k, where(got, one.want("knn2", k)))
        # the iteration table: 100, then 61 (refilled), then 100 again, other entry points in between -- each equals a handle that was
        # only ever called with that parameter
        H = one.H["sim3"]
        table = []
        for max_it in (100, 61, 100):
            with BC.on(H):
                table.append(BC.cat(*(t.cpu().numpy() for t in BC.sim3_dev_call(H, 0, False, max_it))))
            one.run("p3p", 1), one.run("covis", 2)
        for max_it, got in zip((100, 61), table):
            F = BC.make_sim3(0, None)
            try:
                with BC.on(F):
                    fresh = BC.cat(*(t.cpu().numpy() for t in BC.sim3_dev_call(F, 0, False, max_it)))
            finally:
                BC.close_handles(F)
            assert got == fresh, ("iteration table", max_it, where(got, fresh))
        assert table[2] == table[0]
        # no frame bound: an error code, not a result from whatever the buffer holds
        one.H["track"]["objs"][0].bind_frame(None)
        with pytest.raises(SnakeHipError, match="no frame is bound"):
            BC.track_search(one.H["track"], 0)
        assert one.run("track", 0) == one.want("track", 0)


@pytest.mark.parametrize("name", BC.GROWTH_SEAMS)
def test_small_large_small_on_one_handle(name):
    """The large call asks for more than the handle's buffers hold (scratch_capacity of the create-time sizes), so DevBuf::reserve /
    HostBuf::reserve free and reallocate the device block(s) and both pinned blocks of the seam (backend_cases.growth_requests names
    them); the library's allocation count moves by exactly that many, and not at all in the small call after it.  Nothing may keep a
    pointer from before, and a frame bound before the growth is still there after it."""
    from snake_slam_amd import _lib

    allocations = _lib.load().snk_debug_buffer_allocations
    grown = BC.growth_requests(name)
    assert all(need > BC.growth_capacity(buf) for buf, need in grown.items())
    make, run = BC.SEAMS[name]
    H, T = make(0, None), BC.make_track(0, None)
    trk = T["objs"][0]
    BC.share_handle(H["objs"][0], [trk])
    try:
        BC.track_bind(T, 1)
        before = BC.track_search(T, 1)
        first = run(H, 0)
        a0 = allocations()
        large = BC.growth_call(name, H)
        a1 = allocations()
        after = BC.track_search(T, 1)
        third = run(H, 0)
        a2 = allocations()
    finally:
        BC.release_adopters(H["objs"][0], [trk])
        BC.close_handles(H)
    F = make(0, None)
    try:
        fresh = BC.growth_call(name, F)
    finally:
        BC.close_handles(F)
    assert a1 - a0 == len(grown), (name, "buffers reallocated by the large call", a1 - a0, sorted(grown))
    assert a2 == a1, (name, "the small calls after it allocate nothing")
    assert first == BC.solo_bytes(name)[0] and third == first, (name, where(third, first))
    assert large == fresh, (name, where(large, fresh))
    assert before == BC.solo_bytes("track")[1] and after == before, (name, "the bound frame", where(after, before))
