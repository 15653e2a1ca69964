"""CPU: the seam table of tests/backend_cases.py.  The GPU tests built on it compare bytes with bytes, so this file makes sure the bytes
are worth comparing: for every seam with a bit-exact restatement (mappoint, covis, the bag-of-words integers, the triangulation
decisions) the restatement of case 0 exists and is not trivial -- a list is cut at the cap, a point takes the wide form, a pair is
committed and another rejected, words and matches are found.  The growth cases are the smallest that outgrow what a handle's buffers
hold after create (scratch_capacity of the sizes of dispatch.hpp), computed from the compiled header."""
import numpy as np

import backend_cases as BC
import bow_numpy as BW
import covis_numpy as CV
import localmap_numpy as LM
import mappoint_numpy as MP
import p3p_numpy as P3
import scene_numpy as SN
import sim3_numpy as S3
import tri_numpy as TR


def test_the_table_names_every_seam_once():
    assert set(BC.SEAMS) == {"p3p", "sim3", "tri", "mappoint", "covis", "bow", "pgo", "knn2", "stereo", "track", "pose", "lmap", "scene"}
    assert set(BC.MATCHER_SEAMS) == set(BC.SEAMS) - {"pgo"}
    grouped = [s for g in BC.GROUPS.values() for s in g]
    assert sorted(grouped) == sorted(BC.SEAMS) and len(BC.GROUPS) <= 4 and BC.GROUPS["map"] == ("lmap", "scene")


def test_mappoint_case_takes_both_forms_under_both_rules():
    c = BC.mappoint_case(0)
    ks = np.diff(c["obs_start"])
    assert (ks > MP.PACKED_MAX_K).sum() >= 2 and (ks <= MP.PACKED_MAX_K).sum() > MP.CHUNK_POINTS and ks.max() == 100
    med, tot = MP.refresh(c, MP.MEDIAN), MP.refresh(c, MP.SUM)
    wide = np.nonzero(ks > MP.PACKED_MAX_K)[0]
    assert np.all(med["best"][wide] >= 0) and np.all(med["n_valid"][wide] > MP.PACKED_MAX_K // 2)
    assert med.tobytes() != tot.tobytes(), "the two rules pick different descriptors somewhere"
    assert np.any(med["best"] < 0) and np.any(med["ref_level"] >= 0) and np.any(np.abs(med["normal"]).sum(1) > 0)
    # the device form's gathered copy restates to something with wide points too
    h = BC.mappoint_frames(0)["host"]
    r = MP.refresh(h)
    assert np.diff(h["obs_start"]).max() == 100 and np.all(r["status"] == 0) and np.count_nonzero(r["best"] >= 0) > 70


def test_covis_case_cuts_a_list_at_the_cap():
    c = BC.covis_case(0)
    conn_u, res_u = CV.update(c["m"], c["q"], cap=BC.COVIS_CAP)
    conn_v, res_v = CV.vote(c["m"], c["set_start"], c["set_point"], cap=BC.COVIS_CAP)
    for conn, res in ((conn_u, res_u), (conn_v, res_v)):
        assert np.any(res["n_found"] > BC.COVIS_CAP), "at least one list is cut"
        assert np.any(res["n_conn"] == BC.COVIS_CAP) and np.all(res["status"] != CV.BAD_INDEX)
        assert np.any(conn["kf"] >= 0)
    assert np.any(res_u["n_found"] < BC.COVIS_CAP), "and one is not"


def test_lmap_cases_select_and_gather_at_their_small_caps():
    """kf_cap 4 and pts_cap 64: lists are built, one overflows its four keyframes, a vote is passed through as truncated; points are kept at
    the cap, refused above it, found on one table slot."""
    statuses, points = [], []
    for k in range(3):
        c = BC.lmap_case(k)
        s, g = c["select"], c["gather"]
        assert len(s["vote"]) == len(g["sel"]) == 3 and g["local_kf"].shape == (3, BC.LMAP_PARAMS["kf_cap"])
        local, res = LM.select(*(s[a] for a in LM.SELECT_KEYS), BC.LMAP_PARAMS)
        assert local.shape == (3, 4) and np.all((local >= 0).sum(1) == res["n_local"])
        statuses += res["status"].tolist()
        _, ids, n_pts, gres = LM.gather(g["m"], g["frame_id"], g["local_kf"], g["sel"], g["set_start"], g["set_point"], BC.LMAP_PTS_CAP)
        assert np.all((ids >= 0).sum(1) == n_pts)
        statuses += gres["status"].tolist()
        points += n_pts.tolist()
    assert {LM.OK, LM.KF_OVERFLOW, LM.TRUNCATED, LM.PTS_OVERFLOW} <= set(statuses) and statuses.count(LM.OK) >= 12
    assert BC.LMAP_PTS_CAP in points and max(points) == BC.LMAP_PTS_CAP and 0 < min(p for p in points if p) < 10


def test_scene_cases_fit_their_small_caps():
    """win_cap 4, pt_cap 64, obs_cap 256: every query but the bad one gives a scene with fixed cameras, records and, somewhere, constraints"""
    t, p, caps = BC.scene_map(), BC.SCENE_PARAMS, BC.SCENE_CAPS
    got = [SN.local_scene(t, q, p["n_neighbours"], p["n_last"], caps["win_cap"], caps["pt_cap"], caps["img_cap"], caps["obs_cap"], p["gyro_weight"],
                          p["acc_weight"])[1] for k in range(3) for q in BC.scene_queries(k)]
    assert sorted(q for k in range(3) for q in BC.scene_queries(k)) == sorted(SN.QUERIES) and len(got) == 9
    assert [s["status"] for s in got].count(SN.OK) == 8 and [s["status"] for s in got].count(SN.SKIPPED) == 1
    ok = [s for s in got if s["status"] == SN.OK]
    assert all(s["n_img"] > s["n_window"] >= 2 and s["n_pt"] > 16 and s["n_obs"] > s["n_pt"] for s in ok)
    assert max(s["n_window"] for s in ok) == caps["win_cap"] and any(s["n_rpc"] for s in ok) and any(not s["n_rpc"] for s in ok)


def test_tri_case_commits_a_pair_and_rejects_another():
    c = BC.tri_case(0)
    res = TR.triangulate_neighbours(c["cam"], c["params"], c["kf1"], c["kf2s"], c["median_depth2s"], c["pairs"], c["level_scale"])
    entries, rejected = [], 0
    for k, pairs in enumerate(c["pairs"]):
        for (a, b), (br, _, _, _) in zip(pairs, res[k]):
            if br == TR.REJECT:
                rejected += 1
            else:
                entries.append((k, int(a), int(b)))
    commit = TR.commit_pass(entries, c["kf1"]["has_mp"], [k2["has_mp"] for k2 in c["kf2s"]])
    assert rejected > 0 and 0 < sum(bool(x) for x in commit) < len(entries)


def test_bow_cases_have_words_candidates_and_matches():
    V = BW.vocab("irregular")
    t = BW.transform(V, BW.frame_descriptors("irregular", BC.BOW_FRAME_COUNTS[0]), 2)
    assert len(t["words"]) > 10 and len(t["node_id"]) > 1 and len(t["features"]) > 200
    rows = BW.db_rows(65)
    q = BW.db_fresh_query(65, 0)
    assert len(BW.query(rows, q, (), 0.8, 0.75, 0.0, 10)["ids"]) > 0
    _, s, th, ratio = BC.bow_match_cases()[0]
    m12, n = BW.match_bow(s["desc1"], s["has1"], s["bow1"], s["desc2"], s["has2"], s["bow2"], th, ratio)
    assert 0 < n < len(m12) and np.count_nonzero(m12 >= 0) == n
    assert max(BC.BOW_FRAME_COUNTS) <= BC.BOW_CAP


def test_track_case_leaves_a_count_behind(orc):
    """the keyframe matcher's match count stays in the handle's counter buffer: not zero, so the next entry that counts there starts dirty"""
    frame, cam, pose, ls, pts, (pos, desc, skip) = BC.front_cases()["track"][0]
    n, idx = orc.match_coarse(frame, cam, pose, pts, 15.0, 75, 0, ls)
    n_kf, idx_kf = orc.match_keyframe(frame, cam, pose, pos, desc, skip, 15.0, 100)
    assert n > 50 and n_kf > 50 and 0 < skip.sum() < len(skip) and np.count_nonzero(np.asarray(idx_kf) >= 0) == n_kf


def test_ransac_cases_are_the_suites_own():
    assert [[len(c["wps"]) for c in cs] for cs in BC.p3p_cases()] == [[30] * 3, [200] * 3, [1000] * 3]
    assert [len(c["P1"]) for c in BC.sim3_cases()] == [64, 65, 200]


def test_growth_cases_are_the_smallest_that_outgrow_what_a_handle_holds():
    """A buffer created with MATCHER_*_BYTES holds scratch_capacity() of it (a quarter more): the growth cases are sized against that,
    every buffer a case names is asked for more than it holds, and one problem / point / set / query fewer would leave the deciding
    buffer as it is."""
    c, g = BC.matcher_constants(), BC.growth_sizes()
    dev, h_in, h_res = c["dev_capacity"], c["h_in_capacity"], c["h_res_capacity"]
    assert (dev, h_in, h_res) == tuple(n + n // 4 + 256 for n in (c["MATCHER_SCRATCH_BYTES"], c["MATCHER_H_IN_BYTES"], c["MATCHER_H_RES_BYTES"]))
    assert h_res < h_in < dev
    for name in BC.GROWTH_SEAMS:
        need = BC.growth_requests(name)
        assert {"q", "h_in", "h_res"} <= set(need), name  # a device block and both pinned blocks, for every seam
        for buf, n in need.items():
            assert n > BC.growth_capacity(buf), (name, buf, n)
    # the smallest: with one fewer, the buffer that decides the count still fits (P3P's per-problem record is below 256 bytes)
    assert (g["p3p_problems"] - 1) * (P3.MAX_PAIRS * BC.P3P_PAIR_BYTES + 256) + 64 <= dev
    assert (g["sim3_problems"] - 1) * (S3.MAX_PAIRS + BC.SIM3_RESULT_BYTES) <= h_res
    assert (g["mappoint_points"] - 1) * BC.MP_RESULT_BYTES <= dev
    n = g["covis_sets"] - 1
    assert n * BC.GROWTH_SET_CAP * 4 <= dev or n * (BC.GROWTH_COVIS_CAP * BC.COVIS_CONN_BYTES + BC.COVIS_RESULT_BYTES) <= dev
    assert (g["knn2_queries"] - 1) * BC.KNN2_BYTES <= dev
    assert (g["pose_problems"] - 1) * (BC.POSE_MATCHES + BC.POSE_RESULT_BYTES) <= h_res and len(BC.pose_case(0)["obs"]) == BC.POSE_MATCHES
    assert len(BC.growth_case("pose")) == g["pose_problems"]
    # and the cases have those sizes
    assert len(BC.growth_case("p3p")) == g["p3p_problems"] and len(BC.growth_case("p3p")[0]["wps"]) == P3.MAX_PAIRS
    assert len(BC.growth_case("sim3")) == g["sim3_problems"] and len(BC.growth_case("sim3")[0]["points1"]) == S3.MAX_PAIRS
    mp = BC.growth_case("mappoint")
    assert len(mp["ref_obs"]) == g["mappoint_points"] == len(mp["desc"]) == len(mp["pose"]) == len(mp["valid"]) and np.all(np.diff(mp["obs_start"]) == 1)
    start, sets = BC.growth_case("covis")
    assert len(start) - 1 == g["covis_sets"] and sets.shape == (g["covis_sets"], BC.GROWTH_SET_CAP) and np.any(sets >= 0)
    q, t = BC.growth_case("knn2")
    assert len(q) == g["knn2_queries"] and len(t) == BC.GROWTH_KNN2_TRAIN
    # the map seams: one set / query fewer leaves `out`, one map point fewer leaves `q` as it is (48 / 240 bytes: the padding of the parts)
    assert (g["lmap_sets"] - 1) * BC.LMAP_SET_RESULT_BYTES + 48 <= dev and (g["lmap_points"] - 1) * BC.LMAP_POINT_BYTES <= dev
    assert (g["scene_queries"] - 1) * BC.SCENE_QUERY_RESULT_BYTES + 240 <= dev and (g["scene_points"] - 1) * BC.SCENE_POINT_BYTES <= dev
    lm = BC.growth_case("lmap")
    assert len(lm["sel"]) == len(lm["frame_id"]) == len(lm["set_start"]) - 1 == g["lmap_sets"] and lm["local_kf"].shape == (g["lmap_sets"], 4)
    assert all(len(lm["m"][key]) == g["lmap_points"] for key in ("pt_flags", "pt_last_seen") + LM.POINT_KEYS)
    t, queries = BC.growth_case("scene")
    assert len(queries) == g["scene_queries"] and len(t["pt_flags"]) == len(t["pt_pos"]) == len(t["obs_start"]) - 1 == g["scene_points"]
    assert t["obs_start"][-1] == len(t["obs"]) and np.all(np.diff(t["obs_start"]) >= 0)
