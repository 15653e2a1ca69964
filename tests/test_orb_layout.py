"""CPU: the ORB extractor's geometry (snake_slam_amd/csrc/orb_layout.hpp, built with plain g++ through tests/cpp/dispatch_driver.cpp).

Level sizes, scales and feature quotas are compared with the oracle's own restatement of the ORB-SLAM2 constructor arithmetic.  The strips
of the streaming pass and fast_kernel's LDS slice have no second definition: their expected numbers were produced once by the
compute_layout of orb.hip as it stood before the arithmetic moved into the header (copied unchanged into a stand-alone program), so a
change of the geometry shows here without a GPU."""
import numpy as np
import pytest

import forms

# (w, h, nfeatures, n_levels, scale_factor)
EUROC = (752, 480, 1000, 4, 1.2)
KITTI8 = (1241, 376, 2000, 8, 1.2)
SMALL = (40, 40, 500, 16, 1.2)     # tiny levels (below 8 x 8) from level 10 on
NOTHING = (40, 40, 500, 16, 2.0)   # levels scaled to nothing from level 7 on
UNFUSED = (752, 480, 1000, 4, 2.5)  # scale factor > 2: the stand-alone down-scale

GEOM = ("w", "h", "scale", "nfeat", "pitch", "strip_stride", "n_strips", "store_end", "n_bands", "ncols", "nrows", "wcell", "hcell", "slot_cap", "nroots")
SLICE = ("tile_pitch_dw", "s_pitch", "off_s", "off_surv", "off_list", "off_cnt", "lds_wave", "surv_cap", "quads", "cells", "slots", "units", "list_fits",
         "fast_fits")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return forms.build_driver(tmp_path_factory.mktemp("orb_layout"))


def geom(driver, cfg, sw=""):
    w, h, nfeat, levels, scale = cfg
    out, = forms.ask(driver, [("orb_geom", (w, h, nfeat, levels, scale, 0, sw))])
    return [dict(zip(GEOM, (float(v) if k == "scale" else int(v) for k, v in zip(GEOM, lv.split(","))))) for lv in out.split(";")]


def fast_slice(driver, cfg, sw=""):
    w, h, nfeat, levels, scale = cfg
    out, = forms.ask(driver, [("orb_slice", (w, h, nfeat, levels, scale, 0, sw))])
    return dict(zip(SLICE, map(int, out.split(","))))


@pytest.mark.parametrize("cfg", [EUROC, KITTI8, SMALL, NOTHING, UNFUSED], ids=["euroc", "kitti8", "small16", "nothing16", "scale2.5"])
def test_levels_equal_the_oracle(orc, driver, cfg):
    w, h, nfeat, levels, scale = cfg
    L = orc.orb_layout(orc.orb_params(nfeat, scale, levels, 20, 7), w, h)
    G = geom(driver, cfg)
    assert L.n_levels == len(G) == levels
    for l, g in enumerate(G):
        assert (g["w"], g["h"], g["nfeat"]) == (L.w[l], L.h[l], L.nfeat[l]), l
        assert np.float32(g["scale"]) == np.float32(L.scale[l]), l   # printed with nine digits: the float itself
    if cfg is SMALL:
        assert min(g["w"] for g in G) == 3 and sum(g["w"] < 8 for g in G) == 6
    if cfg is NOTHING:
        assert [g["w"] for g in G] == [40, 20, 10, 5, 2, 1, 1] + [0] * 9
        assert all((g["n_strips"], g["n_bands"], g["strip_stride"]) == (0, 0, 4) for g in G[7:])


# (pitch, strip_stride, n_strips, store_end, n_bands) per level
EUROC_STRIPS = [(768, 192, 4, 768, 8), (640, 192, 3, 627, 7), (576, 192, 3, 576, 6), (448, 192, 2, 435, 5)]
EUROC_BALANCED = [(768, 188, 4, 752, 8), (640, 212, 3, 627, 7), (576, 176, 3, 522, 6), (448, 220, 2, 435, 5)]
KITTI_STRIPS = [(1280, 192, 7, 1280, 6), (1088, 192, 6, 1088, 5), (896, 192, 5, 896, 5), (768, 192, 4, 768, 4), (640, 192, 3, 598, 3), (512, 192, 3, 512, 3),
                (448, 192, 2, 416, 2), (384, 192, 2, 384, 2)]
KITTI_BALANCED = [(1280, 208, 6, 1241, 6), (1088, 208, 5, 1034, 5), (896, 216, 4, 862, 5), (768, 240, 3, 718, 4), (640, 200, 3, 598, 3), (512, 168, 3, 499, 3),
                  (448, 208, 2, 416, 2), (384, 176, 2, 346, 2)]
UNFUSED_STRIPS = [(768, 192, 4, 768, 8), (320, 192, 2, 320, 3), (128, 120, 1, 120, 2), (64, 48, 1, 48, 1)]


@pytest.mark.parametrize("cfg,sw,want", [(EUROC, "", EUROC_STRIPS), (EUROC, "BALANCED_STRIPS", EUROC_BALANCED), (KITTI8, "", KITTI_STRIPS),
                                         (KITTI8, "BALANCED_STRIPS", KITTI_BALANCED), (UNFUSED, "", UNFUSED_STRIPS)],
                         ids=["euroc", "euroc-balanced", "kitti8", "kitti8-balanced", "scale2.5"])
def test_strips_as_before_the_move(driver, cfg, sw, want):
    G = geom(driver, cfg, sw)
    assert [(g["pitch"], g["strip_stride"], g["n_strips"], g["store_end"], g["n_bands"]) for g in G] == want
    for g in G:
        last = g["w"] - (g["n_strips"] - 1) * g["strip_stride"]
        assert 0 < last <= 244 and g["strip_stride"] % 4 == 0 and g["store_end"] <= g["pitch"]   # what a wavefront's 61 output lanes cover
        if sw:   # equal strips, nothing stored past the row
            assert g["store_end"] == g["w"] and g["strip_stride"] * g["n_strips"] - g["w"] < 4 * g["n_strips"]
        else:
            assert g["strip_stride"] % 64 == 0 or g["n_strips"] == 1


def test_cells_and_slots_as_before_the_move(driver):
    G = geom(driver, EUROC)
    assert [(g["ncols"], g["nrows"], g["wcell"], g["hcell"], g["slot_cap"], g["nroots"]) for g in G] == \
        [(24, 14, 30, 32, 325, 2), (19, 12, 32, 31, 271, 2), (16, 10, 31, 31, 227, 2), (13, 8, 31, 31, 189, 2)]
    G = geom(driver, KITTI8)
    assert [(g["ncols"], g["nrows"], g["wcell"], g["hcell"], g["slot_cap"], g["nroots"]) for g in G] == \
        [(40, 11, 31, 32, 437, 4), (33, 9, 31, 32, 365, 4), (27, 7, 31, 33, 305, 4), (22, 6, 32, 31, 254, 4), (18, 4, 32, 38, 212, 4), (15, 3, 32, 40, 178, 4),
         (12, 3, 32, 32, 148, 4), (10, 2, 32, 37, 125, 4)]
    G = geom(driver, UNFUSED)
    assert [(g["ncols"], g["nrows"], g["wcell"], g["hcell"]) for g in G] == [(24, 14, 30, 32), (8, 5, 34, 32), (2, 1, 44, 45), (0, 0, 1, 1)]


FAST_SLICES = {
    (EUROC, ""): (12, 40, 1824, 3200, 0, 4224, 4240, 512, 3, 828, 1012, 81),
    (KITTI8, ""): (12, 40, 2208, 3904, 0, 5184, 5200, 640, 3, 1231, 2024, 139),
    (UNFUSED, ""): (16, 64, 3264, 6288, 0, 8336, 8352, 1024, 4, 378, 1012, 41),
    (SMALL, ""): (12, 40, 336, 480, 0, 992, 1008, 256, 3, 0, 548, 16),
    (EUROC, "FAST_SURV_CAP=100"): (12, 40, 1824, 3200, 0, 3456, 3472, 128, 3, 828, 1012, 81),   # at least 128
    (EUROC, "FAST_SURV_CAP=300"): (12, 40, 1824, 3200, 0, 3808, 3824, 300, 3, 828, 1012, 81),
}


@pytest.mark.parametrize("cfg,sw", list(FAST_SLICES), ids=[f"{c[0]}x{c[1]}-{c[3]}-{c[4]}{'-' + s if s else ''}" for c, s in FAST_SLICES])
def test_fast_slice_as_before_the_move(driver, cfg, sw):
    S = fast_slice(driver, cfg, sw)
    assert tuple(S[k] for k in SLICE[:12]) == FAST_SLICES[(cfg, sw)]
    # the invariants snk_orb_configure refuses a shape on: the corner list aliases the image tile, four slices fit a workgroup's LDS
    cells = [g for g in geom(driver, cfg) if g["ncols"] > 0]
    mw, mh = max([g["wcell"] for g in cells] + [1]), max([g["hcell"] for g in cells] + [1])
    list_b, tile_b = (((mw + 1) // 2) * ((mh + 1) // 2) * 4 + 15) & ~15, S["off_s"]
    assert list_b <= tile_b and S["list_fits"] == 1
    assert 4 * S["lds_wave"] <= 160 * 1024 and S["fast_fits"] == 1
    assert S["off_surv"] > S["off_s"] and S["off_cnt"] >= S["off_surv"] + 2 * S["surv_cap"] and S["lds_wave"] == S["off_cnt"] + 16
