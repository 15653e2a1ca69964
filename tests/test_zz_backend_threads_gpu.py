"""GPU: the reference runs LocalMapping, LoopClosing and relocalisation on threads of their own beside Tracking and the bundle
adjustments.  Five threads, each with its own handles and streams, run their chain of back-end seams (tests/backend_cases.py)
concurrently: local mapping (triangulation -> map-point refresh -> covisibility), loop closing (bag of words -> Sim3 RANSAC -> pose-graph
optimisation), relocalisation (kNN-2 -> P3P RANSAC -> pose refinement), local BA and global BA -- the last one a cooperative launch
(the persistent PCG) beside the pose-graph optimiser's resident PCG, another one.  Every result must equal the result of the same call
made alone, and every PGO solve must have run resident: a cooperative launch refused under contention downgrades the handle to the
multi-launch form silently and for good (pgo.hip, launch_pcg)."""
import os
import threading

import numpy as np
import pytest

import backend_cases as BC

pytestmark = pytest.mark.gpu

# named test_zz_*: collected last, like tests/test_zz_threads_gpu.py
ROUNDS = int(os.environ.get("SNK_THREAD_ROUNDS", "6"))
CHAINS = {"local mapping": ("tri", "mappoint", "covis"), "loop closing": ("bow", "sim3", "pgo"), "relocalisation": ("knn2", "p3p", "pose")}


def test_backend_seams_run_concurrently_on_their_own_handles():
    from snake_slam_amd import synth
    from snake_slam_amd.ba import BARec, lba_options

    scenes = [synth.ba_scene(n_kf=8, n_pt=150, obs_per_pt=4, seed=900 + i)[0] for i in range(3)]

    def run_ba_one_call(ba, k):
        ba.create(scenes[k % 3])
        n, ci, cf, pose, pt, flags = ba.solve_local_scene(4.41, 5.29)
        return bytes([n & 255]) + np.float64(ci).tobytes() + np.float64(cf).tobytes() + pose.tobytes() + pt.tobytes() + flags.tobytes()

    def run_gba(gba, k):
        # the PCG of every LM iteration is ONE cooperative launch (pcgl_persist, grid barriers inside)
        gba.reset()
        ci, cf = gba.initAndSolve()
        pose, pt, it = gba.state(0)
        return ci.tobytes() + cf.tobytes() + pose.tobytes() + pt.tobytes() + bytes([it & 255])

    def run_chain(names):
        def run(Hs, k):
            return [BC.SEAMS[name][1](H, k) for name, H in zip(names, Hs)]
        return run

    want_seam = {name: BC.solo_bytes(name) for names in CHAINS.values() for name in names}
    ba = BARec(lba_options())
    gba = BARec(lba_options(max_iterations=2, max_pcg_iterations=25))
    gba.create(synth.ba_scene(n_kf=60, n_pt=900, obs_per_pt=6, seed=77, n_fixed=1)[0])  # 354 x 354 reduced system: beyond one workgroup's LDS
    gba.initAndSolve()
    chains = {title: [BC.SEAMS[name][0](0, None) for name in names] for title, names in CHAINS.items()}
    workers = [(title, run_chain(CHAINS[title]), chains[title]) for title in CHAINS] + [("local BA", run_ba_one_call, ba), ("global BA", run_gba, gba)]
    try:
        want = {"local BA": [run_ba_one_call(ba, k) for k in range(3)], "global BA": [run_gba(gba, k) for k in range(3)]}
        errors, got = [], {title: [None] * ROUNDS for title, _, _ in workers}
        start = threading.Barrier(len(workers))

        def worker(title, fn, h):
            try:
                start.wait()
                for k in range(ROUNDS):
                    got[title][k] = fn(h, k)
            except Exception as e:  # noqa: BLE001
                errors.append((title, repr(e)))

        threads = [threading.Thread(target=worker, args=w) for w in workers]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in threads), "a seam hung"
        assert errors == []
        pgo = chains["loop closing"][2]
        assert pgo["pcg_form"] == [1] * (2 * ROUNDS), "a PGO solve left the resident (cooperative) form under contention"
        for title, _, _ in workers:
            for k in range(ROUNDS):
                if title in CHAINS:
                    for name, b in zip(CHAINS[title], got[title][k]):
                        assert b == want_seam[name][k % 3], (title, name, k)
                else:
                    assert got[title][k] == want[title][k % 3], (title, k)
    finally:
        ba.close(), gba.close()
        for Hs in chains.values():
            for H in Hs:
                BC.close_handles(H)
