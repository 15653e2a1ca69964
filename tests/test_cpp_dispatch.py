"""CPU: dispatch.hpp -- the one definition of which kernel form a launch shape selects -- built with plain g++.  Every row of the
table the GPU tests take their shapes from (tests/forms.py) is asserted against it, so a threshold that moves, or a shape that drifts
away from the form it was written for, fails here without a GPU."""
import re

import pytest

import forms
from forms import ENUM_OF, ENUMS, ENV_ONLY, FORMS

SWITCH_ARGS = {"knn2": [3], "stereo_host": [1], "stereo_batch": [2, 3], "pose_host": [2], "pose_batch": [3, 4]}  # environment switches in a shape


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return forms.build_driver(tmp_path_factory.mktemp("dispatch"))


@pytest.fixture(scope="module")
def answers(driver):
    return dict(zip([(e, s) for e, s, _ in FORMS], forms.ask(driver, [(e, s) for e, s, _ in FORMS])))


@pytest.mark.parametrize("entry,shape,form", FORMS, ids=[f"{e}{s}".replace(" ", "") for e, s, _ in FORMS])
def test_every_row_of_the_table(answers, entry, shape, form):
    assert form in ENUMS[ENUM_OF[entry]]
    assert answers[(entry, shape)] == form


def test_the_table_names_every_form():
    header = (forms.ROOT / "snake_slam_amd" / "csrc" / "dispatch.hpp").read_text()
    for enum, values in ENUMS.items():
        m = re.search(r"enum class %s\s*\{([^}]*)\}" % enum, header)
        assert m and [v.strip() for v in m.group(1).split(",")] == values, f"tests/forms.py does not list {enum} as dispatch.hpp has it"
        named = {f for e, sh, f in FORMS if ENUM_OF[e] == enum and not any(sh[i] for i in SWITCH_ARGS[e])}  # selected by shape alone
        for v in values:
            if (enum, v) not in ENV_ONLY:
                assert v in named, f"no shape of the table selects {enum}::{v}"
    assert len(set((e, s) for e, s, _ in FORMS)) == len(FORMS)


def test_thresholds_from_both_sides(driver):
    """The neighbours of every threshold, computed from the header's own constants: the forms change exactly there."""
    names = ["BF_MFMA_MIN", "BF_WIDE_MIN_WORK", "ST_SORT_MAX", "ST_FRAME_MAX", "ST_FRAME_BATCH", "POSE_HOST_WAVE4_MEAN", "POSE_BATCH_WAVE4_MIN"]
    c = dict(zip(names, map(int, forms.ask(driver, [("const", (n,)) for n in names]))))
    assert c == {"BF_MFMA_MIN": 24, "BF_WIDE_MIN_WORK": 16384, "ST_SORT_MAX": 8192, "ST_FRAME_MAX": 2560, "ST_FRAME_BATCH": 8,
                 "POSE_HOST_WAVE4_MEAN": 192, "POSE_BATCH_WAVE4_MIN": 256}
    q = [("knn2", (24, 24, 1, 1)), ("knn2", (24, 24, 16384, 1)),                               # SNK_BF_NO_MFMA: the vector kernels
         ("knn2", (1, 1, 16383, 0)), ("knn2", (1, 1, 16384, 0)),
         ("knn2", (1 << 20, 23, 4096, 0)),                                                      # batch * nq_cap past 2^31
         ("stereo_batch", (2560, 8, 1, 0)), ("stereo_batch", (1, 1 << 20, 0, 0)), ("stereo_host", (8193, 1)), ("stereo_host", (8192, 1)),
         ("pose_host", (0, 1, 0)), ("pose_host", (192 * 1000, 1000, 0)), ("pose_host", (192 * 1000 - 1, 1000, 0)),
         ("pose_batch", (256, 1000, N := forms.N_CU, 4, 0)), ("pose_batch", (256, 1, N, 2, 0)), ("pose_batch", (255, 1000, N, 2, 0)),
         ("pose_batch", (256, 1000, N, 2, 1))]
    want = ["vector1", "vector4", "vector1", "vector4", "vector4", "count16", "frame", "unindexed", "sort16", "wave1", "wave4_lds", "wave1",
            "wave4_lds", "wave2_lds", "wave1", "wave4_global"]
    assert forms.ask(driver, q) == want


def test_lds_carves(driver):
    """pose_host_carve / pose_batch_carve: the largest problem, capped so that two problems (four frames in the two-wavefront form) share
    a compute unit once there are more than 256, and to what a workgroup can have at all; SNK_POSE_LDS_MATCHES overrides."""
    slots = int(forms.ask(driver, [("const", ("POSE_SLOTS_PER_WAVE",))])[0])
    static4, static2 = (4 * slots * 28 + 28) * 8, (2 * slots * 28 + 28) * 8   # s_part + s_tot of pose_kernel<4, .> / <2, .>
    two_per_cu, four_per_cu = (80 * 1024 - static4 - 256) // 56, (40 * 1024 - static2 - 512) // 56
    dyn_max = (160 * 1024 - static4 - 2048) // 56
    assert two_per_cu * 56 + static4 <= 80 * 1024 and four_per_cu * 56 + static2 <= 40 * 1024 and dyn_max * 56 + static4 <= 160 * 1024
    q = [("pose_host_carve", (1500, 256)), ("pose_host_carve", (1500, 257)), ("pose_host_carve", (900, 257)), ("pose_host_carve", (9000, 1)),
         ("pose_batch_carve", (700, 5, 0, 0)), ("pose_batch_carve", (1500, 257, 0, 0)), ("pose_batch_carve", (1500, 256, 0, 0)),
         ("pose_batch_carve", (1500, 257, 100, 0)), ("pose_batch_carve", (50, 5, 100, 0)), ("pose_batch_carve", (9000, 5, 0, 0)),
         ("pose_batch_carve", (1500, 1000, 0, 1)), ("pose_batch_carve", (300, 1000, 0, 1)), ("pose_batch_carve", (1500, 5, 100, 1)),
         ("pose_batch_carve", (9000, 5, 8000, 1))]
    want = [1500, two_per_cu, 900, dyn_max, 700, two_per_cu, 1500, 100, 50, dyn_max, four_per_cu, 300, 100, dyn_max]
    assert [int(v) for v in forms.ask(driver, q)] == want
