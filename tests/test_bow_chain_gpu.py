"""GPU: the place-recognition chain on one stream with no host copy in between -- descriptors -> snk_bow_transform_batch_dev ->
snk_bow_db_add_batch_dev -> snk_bow_db_query_batch_dev -> snk_match_loop_bow_batch_dev -> snk_sim3_ransac_pairs_batch_dev (reference
Snake/Map/Frame.cpp:38-40, KeyframeDatabase.cpp:20-168, LoopDetector.cpp:69-87, 225, 148-206) -- on four synthetic keyframe pairs with
cap = 256: the pairs handed over equal the host-form results, every source keyframe finds its target as the first candidate, the
RANSAC recovers the planted transform under the tolerance of tests/test_sim3_chain_gpu.py, and the batched transform's feature vectors
give, through the existing snk_match_triangulation_bow, the pairs the host-built (restatement) vectors give."""
import numpy as np
import pytest

import bow_numpy as B
import sim3_numpy as S

pytestmark = pytest.mark.gpu

NB, CAP, VOCAB, LEVELSUP = 4, 256, "k4_L6", 4


def make_keyframes(seed):
    """NB keyframe pairs that see CAP physical points each, as tests/test_sim3_chain_gpu.py builds them: pose2 * wp2 = R (pose1 * wp1) + t
    with a known (R, t); a feature shows one point, its descriptor is the point's -- a vocabulary leaf with a few bits flipped, so that
    the two views of a point mostly fall into the same node -- with a few more bits flipped; some features carry no point."""
    from snake_slam_amd.matcher import KP64_DTYPE

    rng = np.random.default_rng(seed)
    V = B.vocab(VOCAB)
    out = dict(truth=[], poses1=np.zeros((NB, 7)), poses2=np.zeros((NB, 7)), wp1=np.zeros((NB, CAP, 3)), wp2=np.zeros((NB, CAP, 3)),
               kps1=np.zeros((NB, CAP), KP64_DTYPE), kps2=np.zeros((NB, CAP), KP64_DTYPE), desc1=np.zeros((NB, CAP, 4), np.uint64),
               desc2=np.zeros((NB, CAP, 4), np.uint64), frame_pt1=np.zeros((NB, CAP), np.int32), frame_pt2=np.zeros((NB, CAP), np.int32),
               n1=np.array([CAP, CAP - 9, CAP - 30, CAP - 1], np.int32), n2=np.array([CAP - 5, CAP, CAP - 17, CAP], np.int32),
               n_pts1=np.full(NB, CAP, np.int32), n_pts2=np.full(NB, CAP, np.int32))
    for b in range(NB):
        R, t, s = S.random_transform(rng, 1.0)
        out["truth"].append((R, t, s))
        for key in ("poses1", "poses2"):
            Rp, tp, _ = S.random_transform(rng, 1.0, angle=1.0, shift=5.0)
            out[key][b] = S.pose7(Rp.reshape(9), tp)
        P1 = S._random_points(rng, CAP)
        P2 = s * P1 @ R.T + t
        for P, pose, wp in ((P1, out["poses1"][b], "wp1"), (P2, out["poses2"][b], "wp2")):
            out[wp][b] = (P - pose[4:]) @ S.quat_to_R(pose[:4])
        point_desc = B.leaf_descriptors(V, rng, CAP, flips=2)
        for side, P in (("1", P1), ("2", P2)):
            perm = rng.permutation(CAP)  # feature f shows point perm[f]
            px = S.project(P[perm]) + 0.5 * rng.normal(size=(CAP, 2))
            out["kps" + side]["x"][b], out["kps" + side]["y"][b] = px[:, 0], px[:, 1]
            out["desc" + side][b] = np.array([B.flip_bits(rng, d, 3) for d in point_desc[perm]], np.uint64).reshape(CAP, 4)
            fp = perm.astype(np.int32)
            fp[rng.random(CAP) < 0.1] = -1  # no map point
            out["frame_pt" + side][b] = fp
    return out


def test_transform_database_matchbow_ransac_on_one_stream():
    import torch

    from snake_slam_amd.bow import KeyframeDatabase, LoopMatcher, Vocabulary, desc_frames_dev
    from snake_slam_amd.loop import RegistrationRansac
    from snake_slam_amd.tracking import MappingORBMatcher, frames_dev

    K, V = make_keyframes(515), B.vocab(VOCAB)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    kp = lambda a: t(a.view(np.uint8).reshape(NB, CAP, 24))  # noqa: E731
    D = {k: t(K[k]) for k in ("n1", "n2", "n_pts1", "n_pts2", "frame_pt1", "frame_pt2", "poses1", "poses2")}
    D["desc1"], D["desc2"] = t(K["desc1"].view(np.int64)), t(K["desc2"].view(np.int64))
    D["pts1"], D["pts2"] = t(K["wp1"].view(np.uint8).reshape(NB, CAP, 24)), t(K["wp2"].view(np.uint8).reshape(NB, CAP, 24))
    D["has1"], D["has2"] = (D["frame_pt1"] >= 0).to(torch.uint8), (D["frame_pt2"] >= 0).to(torch.uint8)
    zeros = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt, device="cuda")  # noqa: E731
    aux = dict(rp=zeros(NB, CAP, dt=torch.float32), taken=zeros(NB, CAP, dt=torch.uint8), cs=zeros(NB, 2))
    D["kps1"], D["kps2"] = kp(K["kps1"]), kp(K["kps2"])
    fd = [frames_dev((0.0, 0.0, 752.0, 480.0), D["n" + s], D["kps" + s], D["desc" + s], aux["rp"], aux["taken"], aux["cs"]) for s in "12"]
    m12, pairs, n_pairs = zeros(NB, CAP), zeros(NB, CAP, 2), zeros(NB)
    T, scale, cpose = t(np.tile([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], (NB, 1))), t(np.ones(NB)), t(np.zeros((NB, 7)))
    inl, match12 = zeros(NB), zeros(NB, CAP)
    target_ids = [100, 101, 102, 103]
    st = torch.cuda.Stream()
    G = Vocabulary.from_arrays(V.arrays(), stream=st.cuda_stream)
    db = KeyframeDatabase(G, max_keyframes=16, max_words=CAP)
    lm = LoopMatcher(stream=st.cuda_stream)
    rs = RegistrationRansac(S.CAM, S.THRESHOLD, 300, False, 0x5EED0000B0B0, stream=st.cuda_stream)
    tri = MappingORBMatcher()
    try:
        torch.cuda.synchronize()  # the inputs were uploaded on torch's default stream
        t2 = G.transform_batch_dev(desc_frames_dev(D["n2"], D["desc2"]), LEVELSUP)            # Frame::computeBoW of the targets
        db.add_batch_dev(target_ids, t2["words"], t2["values"], t2["n_words"])                # KeyframeDatabase::Add
        t1 = G.transform_batch_dev(desc_frames_dev(D["n1"], D["desc1"]), LEVELSUP)            # ... of the sources
        cand = db.query_batch_dev(t1["words"], t1["values"], t1["n_words"], max_candidates=4)  # DetectLoopCandidates
        lm.match_bow_batch_dev(fd[0], fd[1], D["has1"], D["has2"], t1, t2, m12, pairs, n_pairs, 50, 0.75)  # MatchBoW
        rs.solve_pairs_batch_dev(fd[0], fd[1], pairs, n_pairs, D["pts1"], D["pts2"], D["frame_pt1"], D["frame_pt2"], D["n_pts1"], D["n_pts2"],
                                 D["poses1"], D["poses2"], T, scale, inl, match12, cpose)      # LoopDetector::solve
        st.synchronize()  # the one synchronisation of the chain: nothing above read a result
        H = {k: v.cpu().numpy() for k, v in dict(pairs=pairs, n_pairs=n_pairs, m12=m12, ids=cand["ids"], n_cand=cand["n"], T=T, scale=scale,
                                                 inl=inl).items()}
        h1, h2 = ({k: v.cpu().numpy() for k, v in x.items()} for x in (t1, t2))
        has1, has2 = (K["frame_pt1"] >= 0).astype(np.uint8), (K["frame_pt2"] >= 0).astype(np.uint8)
        E = np.array([0.0, -1.0, 0.02, 1.0, 0.0, -0.3, -0.02, 0.3, 0.0])  # some essential matrix: the gate is the same for both inputs
        for b in range(NB):
            n1, n2 = int(K["n1"][b]), int(K["n2"][b])
            r1, r2 = B.transform(V, K["desc1"][b, :n1], LEVELSUP), B.transform(V, K["desc2"][b, :n2], LEVELSUP)
            bow = lambda r: (r["node_id"], r["node_start"], r["features"])  # noqa: E731
            dev_bow = lambda h: (h["node_id"][b, : h["n_nodes"][b]], h["node_start"][b, : h["n_nodes"][b] + 1],  # noqa: E731
                                 h["features"][b, : h["node_start"][b, h["n_nodes"][b]]])
            for got, want in ((dev_bow(h1), bow(r1)), (dev_bow(h2), bow(r2))):
                assert all(np.array_equal(x, y) for x, y in zip(got, want)), b
            # the pairs handed to the RANSAC equal the host form on host-built vectors
            want12, k = lm.match_bow(K["desc1"][b, :n1], has1[b, :n1], bow(r1), K["desc2"][b, :n2], has2[b, :n2], bow(r2), 50, 0.75)
            f1 = np.nonzero(want12 >= 0)[0]
            assert H["n_pairs"][b] == k and k > 60, (b, k)
            assert np.array_equal(H["pairs"][b, :k, 0], f1) and np.array_equal(H["pairs"][b, :k, 1], want12[f1]), b
            assert np.array_equal(H["m12"][b, :n1], want12) and (H["m12"][b, n1:] == -1).all(), b
            assert np.array_equal(want12, B.match_bow(K["desc1"][b, :n1], has1[b, :n1], bow(r1), K["desc2"][b, :n2], has2[b, :n2], bow(r2))[0]), b
            # the source finds its target first
            assert H["n_cand"][b] >= 1 and H["ids"][b, 0] == target_ids[b], (b, H["ids"][b])
            # the planted transform: map points are exact, only keypoints carry noise (the tolerance of test_sim3_chain_gpu.py)
            R, tt, s = K["truth"][b]
            assert H["inl"][b] > 40, (b, H["inl"][b])
            assert S.transform_distance(S.quat_to_R(H["T"][b, :4]), H["T"][b, 4:], H["scale"][b], R, tt, s) <= S.transform_tolerance(), b
            # snk_match_triangulation_bow on the batched transform's vectors and on the host-built ones
            np1, np2 = rng_points(n1, 1), rng_points(n2, 2)
            a = tri.SearchForTriangulation2((*S.CAM, 0.0), E, np1, K["desc1"][b, :n1], 1 - has1[b, :n1], dev_bow(h1), np2, K["desc2"][b, :n2],
                                            1 - has2[b, :n2], dev_bow(h2), 1e6, 50)
            c = tri.SearchForTriangulation2((*S.CAM, 0.0), E, np1, K["desc1"][b, :n1], 1 - has1[b, :n1], bow(r1), np2, K["desc2"][b, :n2],
                                            1 - has2[b, :n2], bow(r2), 1e6, 50)
            assert a == c and a[0] > 0, (b, a[0], c[0])
    finally:
        tri.close()
        rs.close()
        lm.close()
        db.close()
        G.close()


def rng_points(n, seed):
    return np.random.default_rng(seed).uniform(-0.5, 0.5, (n, 2))
