"""GPU: the life of the back-end handles (tests/backend_cases.py has the seams): created, used and destroyed in a loop without losing
device or pinned memory; on a second device (five modules raise their kernels' LDS limit per device and kernel); and on a caller's
stream behind work that is still running, without a host synchronisation before the call."""
import gc
import os

import numpy as np
import pytest

import backend_cases as BC

pytestmark = pytest.mark.gpu

LEAK_BOUND = 8 << 20  # the project's bound (tests/test_leaks_gpu.py)
LEAK_SEAMS = ("tri", "p3p", "sim3", "mappoint", "covis", "bow", "pgo")  # bow: LoopMatcher, two vocabularies and a database


def rss_bytes():
    with open("/proc/self/statm") as f:
        return int(f.read().split()[1]) * os.sysconf("SC_PAGE_SIZE")


def test_backend_handles_release_their_memory(monkeypatch):
    import torch

    # one caller's stream for every cycle: torch's caching allocator keeps a pool per stream, and a fresh stream per cycle would grow
    # the cache (the seams' device tensors), which is torch's memory, not the library's
    st = torch.cuda.Stream()

    def cycle():
        for name in LEAK_SEAMS:
            make, run = BC.SEAMS[name]
            H = make(0, st)
            try:
                run(H, 0)
            finally:
                BC.close_handles(H)
        # the pose-graph optimiser once more with the rows spread over several workgroups (39 free rows, 10 per workgroup)
        monkeypatch.setenv("SNK_PGO_ROWS_PER_WG", "10")
        H = BC.make_pgo(0, st)
        try:
            BC.run_pgo(H, 0)
        finally:
            BC.close_handles(H)
            monkeypatch.delenv("SNK_PGO_ROWS_PER_WG")
        BC.own_stream_cycle()  # and every handle type on a stream of its own, which it creates and destroys

    from snake_slam_amd import _lib

    live = _lib.load().snk_debug_live_buffers
    gc.collect()  # a wrapper an earlier test left to the collector closes its handle now, not in the middle of the count
    live_start = live()  # what handles of other tests (module fixtures) hold
    cycle()
    torch.cuda.synchronize()
    live0 = live()
    free0, rss0, held0 = torch.cuda.mem_get_info()[0], rss_bytes(), torch.cuda.memory_reserved()
    for _ in range(20):
        cycle()
    torch.cuda.synchronize()
    free1, rss1, held1 = torch.cuda.mem_get_info()[0], rss_bytes(), torch.cuda.memory_reserved()
    print(f"20 cycles: device memory {free0 - free1} bytes (torch's cache grew by {held1 - held0}), host RSS {rss1 - rss0} bytes")
    assert free0 - free1 < LEAK_BOUND, (free0 - free1) >> 20
    assert rss1 - rss0 < LEAK_BOUND, (rss1 - rss0) >> 20
    # the runtime's free-memory figure moves in large steps: a forgotten buffer of a kilobyte (the Sim3 iteration table) never shows in it.
    # Every buffer a handle allocates is counted by the library; all of them are released when the handle is destroyed, so the count is
    # back where it was after every cycle -- exactly.
    assert live0 == live_start and live() == live_start, (live_start, live0, live())


def test_lds_opt_ins_on_a_second_device():
    """p3p, sim3, mappoint (its k = 100 points take the wide form), covis and the resident PGO ask for more than 64 KB of LDS through
    set_max_lds_once, keyed by (device, kernel): device 1 first, then 0, then 1 again."""
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    for name in ("p3p", "sim3", "mappoint", "covis", "pgo"):
        want = BC.solo_bytes(name)
        for device in (1, 0, 1):
            assert BC.solo(name, device) == want, (name, device)


@pytest.mark.parametrize("entry", list(BC.DEV_ENTRIES))
def test_dev_entries_only_enqueue_on_the_callers_stream(entry):
    """The handle lives on the caller's stream; behind some ten milliseconds of unrelated work on that stream the inputs are overwritten
    (with zeros, not random bytes: zeros are in range for every count and index, so a call that ran early would read an empty batch,
    not a wild one), the real inputs are copied back in from a staging copy, and the entry is called at once -- no synchronisation
    between.  An event recorded behind that work must still be pending when the call returns: the entry was enqueued behind running
    work and did not wait for the stream (a handle's first call may: the Sim3 entry synchronises once to fill its iteration table, so
    every entry is called once, with the same parameters, before the work is queued).  The outputs are cloned on the stream; only then
    the host waits."""
    import torch

    name, inputs, call, to_bytes = BC.DEV_ENTRIES[entry]
    make = BC.SEAMS[name][0]
    k = 1
    F = make(0, None)  # the same call on a fresh handle, the host waiting before and after
    try:
        with BC.on(F):
            inputs(F, k)
            F["st"].synchronize()
            want = to_bytes(call(F, k))
    finally:
        BC.close_handles(F)
    st = torch.cuda.Stream()
    H = make(0, st)
    try:
        with BC.on(H):
            ins = inputs(H, k)  # every tensor allocated up front and kept alive (the caching allocator)
            staging = [t.clone() for t in ins]
            a = torch.randn((4096, 4096), device="cuda")
            b = torch.empty_like(a)
            call(H, k)  # the handle's one-time work (kernel attributes, the iteration table) is done
            st.synchronize()
            behind = torch.cuda.Event()
            for t in ins:
                t.zero_()
            for _ in range(16):
                torch.matmul(a, a, out=b)
            for t, s in zip(ins, staging):
                t.copy_(s)
            behind.record(st)
            outs = [t.clone() for t in call(H, k)]
            pending = not behind.query()
            st.synchronize()
            got = to_bytes(outs)
    finally:
        BC.close_handles(H)
    assert pending, f"{entry}: the stream had drained before the call returned -- the entry waited for it, or the work in front was too short"
    assert got == want, entry
