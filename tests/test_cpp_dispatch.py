"""CPU: dispatch.hpp -- the one definition of which kernel form a launch shape selects -- built with plain g++.  Every row of the
table the GPU tests take their shapes from (tests/forms.py) is asserted against it, so a threshold that moves, or a shape that drifts
away from the form it was written for, fails here without a GPU."""
import re

import pytest

import forms
from forms import ENUM_OF, ENUMS, ENV_ONLY, FORMS

SWITCH_ARGS = {"knn2": [3], "stereo_host": [1], "stereo_batch": [2, 3], "pose_host": [2], "pose_batch": [3, 4],
               "ba_lm": [len(forms.BA_FIELDS)], "orb_band": [3], "orb_fast": [], "orb_harris": [2], "orb_dist": [], "orb_desc": [0], "orb_sched": [4],
               "orb_plan": [len(forms.ORB_FIELDS)], "track_form": [4, 5], "track_launch": [4, 5, 6, 7], "grid_form": [2]}  # environment switches in a shape


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return forms.build_driver(tmp_path_factory.mktemp("dispatch"))


@pytest.fixture(scope="module")
def answers(driver):
    return dict(zip([(e, s) for e, s, _ in FORMS], forms.ask(driver, [(e, s) for e, s, _ in FORMS])))


@pytest.mark.parametrize("entry,shape,form", FORMS, ids=[f"{e}{s}".replace(" ", "") for e, s, _ in FORMS])
def test_every_row_of_the_table(answers, entry, shape, form):
    assert all(value in ENUMS[enum] for enum, value in forms.parts(entry, form))
    assert answers[(entry, shape)] == form


def test_the_table_names_every_form():
    header = (forms.ROOT / "snake_slam_amd" / "csrc" / "dispatch.hpp").read_text()
    for enum, values in ENUMS.items():
        m = re.search(r"enum class %s\s*\{([^}]*)\}" % enum, header)
        assert m and [v.strip() for v in m.group(1).split(",")] == values, f"tests/forms.py does not list {enum} as dispatch.hpp has it"
        named = {v for e, sh, f in FORMS if not any(sh[i] for i in SWITCH_ARGS[e]) for en, v in forms.parts(e, f) if en == enum}  # selected by shape alone
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


BA_CONSTANTS = {"BA_SET_MIN_ITEMS": 256, "BA_FUSED3_MAX_K": 8, "BA_CAM64_MIN_BATCH": 16, "BA_SCHUR_WIDE_BATCH_END": 16, "BA_SCHUR_WIDE_MAX_BLOCKS": 8192,
                "BA_PCG_SMALL_MAX_N6": 128, "BA_PCG_LDS_MAX": 158 * 1024, "BA_PERSIST_LDS_MAX": 150 * 1024, "PREG_MAX_N6": 2048,
                "BA_PREG_ROWS16_ABOVE_N6": 512, "BA_SPLIT_COPY_MAX_BATCH": 4, "BA_SPLIT_COPY_MIN_POINTS": 4096, "BA_GRAPH_CHAINS": 1,
                "BA_GRAPH_CHAINS_MIN_BATCH": 128, "BA_GRAPH_CHAIN_MIN": 64, "SUM_NB": 4, "PERSIST_WGS_MAX": 1024}


def test_ba_constants(driver):
    names = list(BA_CONSTANTS)
    assert dict(zip(names, map(int, forms.ask(driver, [("const", (n,)) for n in names])))) == BA_CONSTANTS


def test_ba_thresholds_from_both_sides(driver):
    """Both neighbours of every threshold of ba_lm_plan: the form of a stage changes exactly there."""
    ba, SETS = forms.ba, forms.SETS
    stage = {"lin": 0, "cam": 1, "schur": 2, "pcg": 3, "update": 4}
    cases = [  # (shape, stage, form)
        # 256 work items in the call: max_set_items * B
        (ba(B=128, set_ok=1, items=2), "lin", "fused3"), (ba(B=127, set_ok=1, items=2), "lin", "point_wave"),
        (ba(B=85, set_ok=1, items=3), "update", "update_wave"), (ba(B=86, set_ok=1, items=3), "update", "update_cost"),
        (ba(B=128, set_ok=0, items=2), "lin", "point_wave"),
        # set_k_max <= 8: three tile rows
        (ba(B=256, k=8, run=10, **SETS), "lin", "fused3"), (ba(B=256, k=9, run=10, **SETS), "lin", "point_wave"),
        (ba(B=256, k=9, run=10, **SETS), "schur", "mfma43"),
        (ba("NO_SCHUR_FUSED", B=256, k=8, run=10, **SETS), "schur", "mfma32"), (ba("NO_SCHUR_FUSED", B=256, k=9, run=10, **SETS), "schur", "mfma43"),
        (ba("CAM_SUMS,FUSED_K10", B=256, k=9, run=10, **SETS), "lin", "fused4"), (ba("CAM_SUMS,FUSED_K10", B=256, k=9, run=10, **SETS), "cam", "cam64_xcd"),
        # set_run_max * 9 + 3 <= 128: two register tiles up to 13 rows
        (ba("NO_SCHUR_FUSED", B=256, run=13, **SETS), "schur", "mfma32"), (ba("NO_SCHUR_FUSED", B=256, run=14, **SETS), "schur", "mfma33"),
        # B >= 16: a wavefront per camera
        (ba(B=15), "cam", "cam256"), (ba(B=16), "cam", "cam64_xcd"),
        # B < 16 and nb * B <= 8192: a workgroup per block
        (ba(B=15, nfc=3), "schur", "pass4"), (ba(B=16, nfc=3), "schur", "pass1"),
        (ba(B=2, nfc=64, pwgs=0), "schur", "pass4"), (ba(B=2, nfc=65, pwgs=0), "schur", "pass1"),   # 2 * 4096 = 8192, 2 * 4225
        (ba(B=1, nfc=90), "schur", "pass4"), (ba(B=1, nfc=91), "schur", "pass1"),                   # 8100, 8281
        # max_n6 <= 128, and the 21 / 22 / 23 free-camera window of the per-problem PCG
        (ba(nfc=21), "pcg", "small"), (ba(nfc=22), "pcg", "solve_global"), (ba(nfc=23), "pcg", "launches"),
        (ba(nfc=21, n6=128), "pcg", "small"), (ba(nfc=21, n6=129), "pcg", "solve_lds"),   # (the hand-over gives n6 = 6 nfc: 126 and 132 are the real neighbours)
        (ba("PCG_LDS", nfc=21), "pcg", "solve_lds"), (ba("PCG_GENERAL", nfc=21), "pcg", "solve_lds"), (ba("PCG_LDS", nfc=22), "pcg", "solve_global"),
        # the cooperative forms as ba_plan_pcg left them; recorded sequences and batches take the launches
        (ba(nfc=23, pwgs=18, pone=2, prows=8), "pcg", "persist_reg8"), (ba(nfc=23, pwgs=9, pone=2, prows=16), "pcg", "persist_reg16"),
        (ba(nfc=23, pwgs=18, pone=2, prows=8, rec=1), "pcg", "launches"), (ba(B=2, nfc=23, pwgs=18, pone=2, prows=8), "pcg", "launches"),
        # B <= 4 and max_np >= 4096: the copy of the accepted state on its own workgroups -- see the numbers below
    ]
    got = forms.ask(driver, [("ba_lm", sh) for sh, _, _ in cases])
    for (sh, st, want), g in zip(cases, got):
        assert g.split("/")[stage[st]] == want, (sh, st, g)
    # the derived numbers: use_set, nsx, nbs, nbx, pcg_lds, zero_rows, split_copy, no_block_lists, chains
    nums = lambda *shapes: [tuple(int(x) for x in a.split(",")) for a in forms.ask(driver, [("ba_lm_nums", sh) for sh in shapes])]
    a, b, c, d = nums(ba(B=4, np=4096), ba(B=4, np=4095), ba(B=5, np=4096), ba(B=1, np=1 << 20))
    assert (a[6], b[6], c[6], d[6]) == (1, 0, 0, 1)
    # nsx = ceil(items / 4); nbx = ceil(nfc^2 / 4); nbs = ceil(nfc^2 / 16); the LDS of pcg_small, pcg_solve<false>, pcg_solve<true>
    a, b, c = nums(ba(B=256, nfc=5, set_ok=1, items=9), ba(nfc=22), ba("PCG_LDS", nfc=21))
    assert a[:4] == (1, 3, 2, 7) and a[4] == (30 * 9 + 5 * 72) * 8 + 8192 and a[5] == 1
    assert b[4] == 132 * 72 + 22 * 288 and c[4] == 126 * 72 + 21 * 288 + 126 * 126 * 8 + 1024 + 8192 <= 158 * 1024
    # the LDS of the cooperative forms: 2, 3 and 1 vectors of n6 doubles
    a, b, c = nums(ba(nfc=23, pwgs=18, pone=2, prows=8), ba(nfc=23, pwgs=18, pone=1), ba(nfc=23, pwgs=18, pone=0))
    assert (a[4], b[4], c[4]) == (138 * 16, 138 * 24, 138 * 8)
    # the block-major pass without its lists is an internal error, as a value; NO_POINT_WAVE clears zero_rows
    a, b, c = nums(ba(blk=0), ba(B=256, blk=0, **SETS), ba("NO_POINT_WAVE"))
    assert (a[7], b[7], c[7]) == (1, 0, 0) and (a[5], c[5]) == (1, 0)
    a, = nums(ba(imp=1, blk=0, pwgs=8))
    assert a[7] == 0


def test_ba_pcg_sizes_chains_and_persistent_forms(driver):
    """ba_pcg_is_large, ba_graph_chains, the register-row rule and what ba_plan_pcg makes of the runtime's answers."""
    ask = lambda *q: forms.ask(driver, list(q))
    assert ask(("ba_pcg_large", (126, 21, 0)), ("ba_pcg_large", (132, 22, 0)), ("ba_pcg_large", (138, 23, 0)), ("ba_pcg_large", (1794, 299, 1))) == \
        ["0", "0", "1", "0"]
    # chains: recorded sequences of >= 128 per-problem windows only; SNK_BA_GRAPH_CHAINS at most one chain per 64 windows
    assert ask(("ba_chains", (256, 1, 0, 0)), ("ba_chains", (256, 1, 0, 2)), ("ba_chains", (256, 0, 0, 2)), ("ba_chains", (127, 1, 0, 2)),
               ("ba_chains", (128, 1, 0, 2)), ("ba_chains", (128, 1, 0, 4)), ("ba_chains", (256, 1, 1, 2))) == ["1", "2", "1", "1", "2", "2", "1"]
    assert [int(a.split(",")[8]) for a in ask(("ba_lm_nums", forms.ba("GRAPH_CHAINS=2", B=256, rec=1)), ("ba_lm_nums", forms.ba("GRAPH_CHAINS=2", B=256)))] == [2, 1]
    # 16 register rows above 512 unknowns; SNK_BA_PERSIST_REG_ROWS forces 8 or 16 and nothing else
    assert ask(("ba_reg_rows", (512, "")), ("ba_reg_rows", (513, "")), ("ba_reg_rows", (100, "PERSIST_REG_ROWS=16")),
               ("ba_reg_rows", (1000, "PERSIST_REG_ROWS=8")), ("ba_reg_rows", (1000, "PERSIST_REG_ROWS=12"))) == ["8", "16", "16", "8", "16"]
    # count, n6, nfc, cooperative launch, CUs, resident workgroups per CU of pcgl_persist / pcgl_persist1 / pcgl_persist_reg
    q = [(1, 1794, 299, 1, 256, 1, 1, 1, ""),                       # FullBA on 300 keyframes: 113 workgroups of 16 rows in registers
         (1, 174, 29, 1, 256, 1, 1, 1, ""),                         # 30 keyframes: 22 workgroups of 8 rows
         (1, 2048, 342, 1, 256, 1, 1, 1, ""), (1, 2052, 342, 1, 256, 1, 1, 1, ""),   # PREG_MAX_N6: beyond, pcgl_persist1 with n6 / 12 workgroups
         (1, 1794, 299, 1, 256, 1, 1, 1, "PERSIST_STREAM"), (1, 1794, 299, 1, 256, 1, 1, 1, "PERSIST_TWO_BARRIERS"),
         (1, 1794, 299, 1, 256, 1, 1, 1, "PERSIST_WGS=32"), (1, 1794, 299, 1, 256, 1, 1, 1, "PCGL_LAUNCHES"),
         (2, 1794, 299, 1, 256, 1, 1, 1, ""), (1, 1794, 299, 0, 256, 1, 1, 1, ""), (1, 1794, 299, 1, 256, 0, 1, 1, ""),
         (1, 1794, 299, 1, 256, 1, 0, 1, ""), (1, 1794, 299, 1, 256, 1, 1, 0, ""), (1, 1794, 299, 1, 64, 1, 1, 1, ""),
         (1, 6402, 1067, 1, 256, 1, 1, 1, ""), (1, 19206, 3201, 1, 256, 1, 1, 1, "")]   # 3 n6 doubles past 150 KB: two barriers; n6 doubles past it: none
    want = ["113,2,16", "22,2,8", "128,2,16", "171,1,0", "150,1,0", "150,0,0", "32,1,0", "0,0,0", "0,0,0", "0,0,0", "0,0,0", "150,0,0", "150,1,0",
            "64,1,0", "256,0,0", "0,0,0"]
    assert ask(*[("ba_persist", a) for a in q]) == want
    # implicit form: a point per thread or a camera per wavefront, at least 16 workgroups, at most one per CU
    assert ask(("ba_persist_imp", (9000, 299, 1, 256, 2, "")), ("ba_persist_imp", (100, 10, 1, 256, 2, "")), ("ba_persist_imp", (10**6, 299, 1, 256, 2, "")),
               ("ba_persist_imp", (9000, 299, 1, 256, 2, "PCGL_LAUNCHES")), ("ba_persist_imp", (9000, 0, 1, 256, 2, "")),
               ("ba_persist_imp", (9000, 299, 1, 256, 2, "PERSIST_WGS=600"))) == ["75,0,0", "16,0,0", "256,0,0", "0,0,0", "0,0,0", "512,0,0"]
    # graph or plain launches: cooperative forms, SNK_BA_NO_GRAPH and zero iterations are always plain
    assert ask(("ba_plain", forms.ba(nfc=23, pwgs=18, pone=2, prows=8)[:19] + (5, "")), ("ba_plain", forms.ba()[:19] + (5, "")),
               ("ba_plain", forms.ba()[:19] + (0, "")), ("ba_plain", forms.ba()[:19] + (5, "NO_GRAPH")),
               ("ba_plain", forms.ba(nfc=23, pwgs=0)[:19] + (5, "")), ("ba_plain", forms.ba(imp=1, pwgs=8)[:19] + (5, ""))) == ["1", "0", "1", "1", "0", "1"]
    assert ask(("ba_sets", forms.ba(B=128, set_ok=1, items=2)[:19] + ("",)), ("ba_sets", forms.ba(B=127, set_ok=1, items=2)[:19] + ("",)),
               ("ba_sets", forms.ba(B=1, set_ok=1, items=1)[:19] + ("SCHUR_SET_MIN_ITEMS=1",)), ("ba_sets", forms.ba(B=128, nfc=0, set_ok=1, items=2)[:19] + ("",))) == \
        ["1", "0", "1", "0"]


def test_ba_switch_lists_agree():
    """BaSwitches (dispatch.hpp), its reader (ba_types.hpp), the driver's parser, tests/forms.py and the README name the same switches;
    ba.hip reads none itself but SNK_DEBUG, and the hand-over none of the solver's path switches."""
    csrc = forms.ROOT / "snake_slam_amd" / "csrc"
    struct = re.search(r"struct BaSwitches\s*\{(.*?)\n\};", (csrc / "dispatch.hpp").read_text(), re.S).group(1)
    fields = re.findall(r"^\s+(?:bool|int|long long) \w+\s*=[^;]*;\s*// (\w+)", struct, re.M)
    assert fields == forms.BA_SWITCHES + ["SNK_DEBUG"]
    reader = (csrc / "ba_types.hpp").read_text()
    assert sorted(set(re.findall(r'"SNK_BA_(\w+)"', reader))) == sorted(forms.BA_SWITCHES) and '"SNK_DEBUG"' in reader
    driver = (forms.ROOT / "tests" / "cpp" / "dispatch_driver.cpp").read_text()
    assert sorted(re.findall(r'k == "(\w+)"', driver)) == sorted(forms.BA_SWITCHES + ["DEBUG"])
    readme = (forms.ROOT / "README.md").read_text()
    assert all(f"SNK_BA_{n}" in readme for n in forms.BA_SWITCHES)
    assert re.findall(r'getenv\("(\w+)"\)', (csrc / "ba.hip").read_text()) == ["SNK_DEBUG"]
    handover = set(re.findall(r'"SNK_BA_(\w+)"', (csrc / "ba_handover.hip").read_text()))
    assert handover == {"NO_BIG_ITEMS", "SCHUR_SET_MIN_ITEMS", "PROFILE_CREATE", "HOST_THREADS", "NO_HOST_POOL", "FILL_CHUNKS", "HOST_ENTRIES",
                        "BECNT_BUDGET", "CHECK_LISTS"}


ORB_CONSTANTS = {"ORB_BAND_MIN_WAVES": 2048, "ORB_WAVE_SLOTS": 8192, "ORB_FAST_CPW_DEFAULT": 8, "ORB_FAST_MIN_ROUNDS": 4, "ORB_XCD_MIN_BATCH": 16,
                 "ORB_DIST_ONE_MAX_WGS": 128, "ORB_DIST_LARGE_WGS": 256, "ORB_DIST_SMALL_CAP": 2048,
                 # 19 bytes per candidate + 16; the 2048-candidate carve with the Harris ranks (4 bytes each + 16) is the smaller one
                 "ORB_DIST_LDS_MAX": 8192 * 19 + 16, "ORB_DIST_LARGE_LDS_MAX": 8192 * 19 + 16,
                 "TRACK_FRAME_LDS_MAX": 144 * 1024, "TRACK_PPW_POINTS": 8192}


def test_orb_and_track_constants(driver):
    names = list(ORB_CONSTANTS)
    assert dict(zip(names, map(int, forms.ask(driver, [("const", (n,)) for n in names])))) == ORB_CONSTANTS
    assert 2048 * 19 + 16 + 4 * 2048 + 16 < 8192 * 19 + 16 <= 160 * 1024


MATCHER_CONSTANTS = {"MATCHER_SCRATCH_BYTES": 4 << 20, "MATCHER_H_IN_BYTES": 1 << 20, "MATCHER_H_RES_BYTES": 256 << 10}


def test_matcher_scratch_constants(driver):
    """What snk_matcher_create pre-sizes; tests/backend_cases.py computes its growth cases from the same header."""
    import backend_cases

    names = list(MATCHER_CONSTANTS)
    assert dict(zip(names, map(int, forms.ask(driver, [("const", (n,)) for n in names])))) == MATCHER_CONSTANTS
    got = backend_cases.matcher_constants()
    assert {n: got[n] for n in names} == MATCHER_CONSTANTS
    # a buffer holds a quarter more than it was asked for, plus 256 bytes (DevBuf / HostBuf::reserve use the same function)
    assert [int(a) for a in forms.ask(driver, [("capacity", (n,)) for n in (0, 1000, 4 << 20)])] == [256, 1506, (5 << 20) + 256]
    assert got["dev_capacity"] == (5 << 20) + 256 and got["h_in_capacity"] == 1310976 and got["h_res_capacity"] == 327936
    common = (forms.ROOT / "snake_slam_amd" / "csrc" / "common.hpp").read_text()
    assert common.count("size_t want = scratch_capacity(n);") == 2
    src = (forms.ROOT / "snake_slam_amd" / "csrc" / "matcher.hip").read_text()
    assert all(re.search(r"reserve\(%s\)" % n, src) for n in names), "snk_matcher_create sizes its buffers by the header's constants"


def test_orb_thresholds_from_both_sides(driver):
    """Both neighbours of every threshold of orb_plan's parts."""
    ask = lambda *q: forms.ask(driver, list(q))
    # rows per band: strips * ceil(h / bh) = 2047 and 2048, for 64 and for 22 rows (23 * 89 = 2047, 2048 = 2 * 1024; 1 strip x 2047 / 2048 images)
    assert ask(("orb_band", (1, 64, 2047, 0)), ("orb_band", (1, 64, 2048, 0)), ("orb_band", (89, 23 * 64, 1, 0)), ("orb_band", (2, 1024 * 64, 1, 0)),
               ("orb_band", (89, 23 * 22, 1, 0)), ("orb_band", (127, 16 * 22, 1, 0)), ("orb_band", (128, 16 * 22, 1, 0)), ("orb_band", (1, 22, 2047, 0)),
               ("orb_band", (1, 65, 1024, 0)),                                   # ceil: 65 rows are two bands of 64
               ("orb_band", (1, 64, 2048, 8)), ("orb_band", (1, 22, 1, 64)), ("orb_band", (1, 64, 2048, 23))) == \
        ["bh22", "bh64", "bh22", "bh64", "bh8", "bh8", "bh22", "bh8", "bh64", "bh8", "bh64", "bh64"]
    # cells per wavefront: halved while cell_waves / cpw < 32768 (four rounds of 8192 wavefront slots)
    assert [int(a) for a in ask(("orb_cpw", (32768 * 8, 1, 0)), ("orb_cpw", (32768 * 8 - 1, 1, 0)),       # / 8 = 32768 and 32767
                                ("orb_cpw", (32768 * 4, 1, 0)), ("orb_cpw", (32768 * 4 - 1, 1, 0)),
                                ("orb_cpw", (32768 * 2, 1, 0)), ("orb_cpw", (32768 * 2 - 1, 1, 0)),
                                ("orb_cpw", (828, 2048, 0)), ("orb_cpw", (828, 1, 0)), ("orb_cpw", (1 << 20, 1 << 15, 0)),   # past 2^31 cells
                                ("orb_cpw", (828, 1, 64)), ("orb_cpw", (828, 2048, 1)), ("orb_cpw", (828, 2048, 65)))] == \
        [8, 4, 4, 2, 2, 1, 8, 1, 8, 64, 1, 8]
    # one distribute launch: n_levels * batch = 128 and 129; never under Harris; the small carve alone when it holds level_cap
    assert ask(("orb_dist", (8, 16, 8192, 0)), ("orb_dist", (1, 129, 8192, 0)), ("orb_dist", (8, 16, 8192, 1)), ("orb_dist", (1, 1, 4096, 1)),
               ("orb_dist", (1, 1, 2048, 0)), ("orb_dist", (1, 1, 2048, 1)), ("orb_dist", (16, 65535, 256, 0)), ("orb_dist", (16, 65535, 8192, 0))) == \
        ["one_full", "small_drain", "small_drain", "small_drain", "one_small", "one_small", "one_small", "small_drain"]
    # the carve and its capacity, the drain launch's workers, the queue counter's fill: fast_gx, fast_lds, harris_gx, lds_cap, dist_lds,
    # large_workers, queue_memset, desc_gx, desc_nb, dfake, blur_mode; then n_bands.gx per level
    nums = lambda *shapes: [([int(x) for x in a.split(";")[0].split(",")], a.split(";")[1]) for a in forms.ask(driver, [("orb_plan_nums", sh) for sh in shapes])]
    orb = forms.orb
    carve = lambda cap: cap * 19 + 16
    (a, al), (b, _), (c, _), (d, _), (e, _), (f, _) = nums(orb(), orb(batch=33), orb(harris=1), orb(cap=1024, harris=1), orb(stages=1), orb(stages=2))
    assert a[3:7] == [8192, carve(8192), 4, 0] and b[3:7] == [2048, carve(2048), 132, 0]
    assert c[3:5] == [2048, carve(2048) + 4 * 2048 + 16] and d[3:5] == [1024, carve(1024) + 4 * 1024 + 16]
    assert (a[6], e[6], f[6]) == (0, 1, 1)                       # fast_kernel resets the counter only when the whole chain is one call's
    assert nums(orb(batch=300))[0][0][5] == 256
    # one image of 752 x 480: 828 cells, one per wavefront, four wavefronts of 4240 bytes; bands of 8 rows, strips x bands / 4 workgroups
    assert a[0:2] == [207, 4 * 4240] and al == "60.60,50.38,42.32,35.18" and a[7:9] == [ceil_div(325, 16), 1]
    g, h, i = nums(orb(batch=2048), orb("FAST_LDS_WG=65536"), orb("FAST_LDS_WG=999999"))
    assert g[0][0] == ceil_div(828, 32) and g[1] == "8.8,7.6,6.5,5.3" and g[0][8] == 2048 and (h[0][1], i[0][1]) == (65536, 160 * 1024)
    assert nums(orb(batch=17))[0][0][8] == 24 and nums(orb(batch=15))[0][0][8] == 15                   # describe_kernel's image slots: eights from 16 on
    assert [n[0][10] for n in nums(orb("BLUR_IN_DESCRIBE"), orb("BLUR_TILED"), orb("BLUR_TILED,DESC_NO_DMA"), orb("BLUR_TILED,DESC_FAKE=0"), orb("DESC_FAKE=2"))] == \
        [1, 2, 0, 0, 0]
    assert nums(orb("DESC_FAKE=2"))[0][0][9] == 2
    # Harris: 16 cells per wavefront, or one
    assert nums(orb(harris=1))[0][0][2] == ceil_div(ceil_div(828, 16), 4) and nums(orb("HARRIS_PER_CELL", harris=1))[0][0][2] == 207
    # XCD-aware grids: batch 15 and 16
    assert ask(("orb_xcd", (207, 15)), ("orb_xcd", (207, 16)), ("orb_xcd", (207, 17)), ("orb_xcd", (3, 1))) == ["207,15", "1656,2", "1656,3", "3,1"]
    # launch chains: split_min_batch, two images per staggered part, parts capped by the batch
    assert ask(("orb_sched", (8, 2, 0, 8, 0)), ("orb_sched", (7, 2, 0, 8, 0)), ("orb_sched", (8, 1, 4, 8, 0)), ("orb_sched", (9, 1, 5, 8, 0)),
               ("orb_sched", (10, 1, 5, 8, 0)), ("orb_sched", (10, 3, 5, 8, 0)), ("orb_sched", (9, 3, 5, 8, 0)), ("orb_sched", (2, 4, 0, 1, 0)),
               ("orb_sched", (1, 4, 0, 1, 0)), ("orb_sched", (64, 4, 4, 8, 1))) == \
        ["chains", "one_chain", "staggered", "one_chain", "staggered", "staggered", "chains", "chains", "one_chain", "one_chain"]
    assert ask(("orb_sched_n", (8, 2, 0, 8, 0)), ("orb_sched_n", (10, 3, 5, 8, 0)), ("orb_sched_n", (9, 3, 5, 8, 0)), ("orb_sched_n", (2, 4, 0, 1, 0)),
               ("orb_sched_n", (7, 2, 0, 8, 0))) == ["2", "5", "3", "2", "1"]


def ceil_div(a, b):
    return -(-a // b)


def frame_lds(cap, ncell1):
    """LDS of a frame: keypoints, descriptors, right points, taken flags (each padded to 16 bytes), cell starts, 64 bytes of slack."""
    up = lambda v: (v + 15) & ~15
    return up(cap * 24) + cap * 32 + up(cap * 4) + up(cap) + ncell1 * 4 + 64


def test_track_thresholds_from_both_sides(driver):
    ask = lambda *q: [int(a) for a in forms.ask(driver, list(q))]
    # workgroups per frame: ceil(1024 / batch), at most one per chunk, at least one; SNK_TRACK_FRAME_WGS
    assert ask(("track_wgs", (10, 1, 0)), ("track_wgs", (10, 1024, 0)), ("track_wgs", (10, 1025, 0)), ("track_wgs", (10, 512, 0)), ("track_wgs", (10, 511, 0)),
               ("track_wgs", (10, 103, 0)), ("track_wgs", (1, 1, 0)), ("track_wgs", (10, 1024, 3)), ("track_wgs", (2, 1024, 3)), ("track_wgs", (10, 0, 0))) == \
        [10, 1, 1, 2, 3, 10, 1, 3, 2, 10]
    # the claims behind the frame: the last capacity at which frame + claims fit 144 KB, and the next
    M = 144 * 1024
    cap = max(c for c in range(1, 4000) if ((frame_lds(c, 2401) + 15) & ~15) + 4 * c <= M)
    f0, f1 = frame_lds(cap, 2401), frame_lds(cap + 1, 2401)
    assert ask(("track_lds", (cap, 2401)), ("track_lds", (cap + 1, 2401)), ("track_lds", (1000, 2401))) == [f0, f1, 24000 + 32000 + 4000 + 1008 + 9604 + 64]
    assert ask(("track_claim", (1, f0, cap, 0)), ("track_claim", (1, f1, cap + 1, 0)), ("track_claim", (2, f0, cap, 0)), ("track_claim", (1, f0, cap, 1)),
               ("track_claim", (1, M - 4 * 2116, 2116, 0)), ("track_claim", (1, M - 4 * 2116 + 1, 2116, 0)), ("track_claim", (1, 100, 10, 0))) == \
        [(f0 + 15) & ~15, -1, -1, -1, M - 4 * 2116, -1, 112]   # (4 * 2116 is a multiple of 16: the claims end on the last byte)
    # points per wavefront: a point per 8192 of the call, 1 .. 64; SNK_TRACK_PPW
    assert ask(("track_ppw", (8191, 0)), ("track_ppw", (8192, 0)), ("track_ppw", (16383, 0)), ("track_ppw", (16384, 0)), ("track_ppw", (0, 0)),
               ("track_ppw", (64 * 8192 - 1, 0)), ("track_ppw", (64 * 8192, 0)), ("track_ppw", (1 << 40, 0)), ("track_ppw", (100, 64)), ("track_ppw", (1 << 40, 1)),
               ("track_ppw", (8192 * 5, 65))) == [1, 1, 1, 2, 1, 63, 64, 64, 64, 1, 5]
    # a whole launch: ppw, wgs, claim_off, lds -- the frame form resolves in the kernel with one workgroup per frame
    plan = lambda *a: [int(x) for x in forms.ask(driver, [("track_plan", a)])[0].split(",")]
    fl = frame_lds(1000, 2401)
    assert plan(10000, 1024, 1000, 2401, 0, 0, 0, 0) == [64, 1, (fl + 15) & ~15, ((fl + 15) & ~15) + 4000]
    assert plan(10000, 512, 1000, 2401, 0, 0, 0, 0) == [64, 2, -1, fl]
    assert plan(10000, 1024, 1000, 2401, 0, 0, 1, 0) == [64, 1, -1, fl]        # SNK_TRACK_NO_FUSED_RESOLVE
    assert plan(10000, 1024, 1000, 2401, 0, 4, 0, 0) == [64, 4, -1, fl]        # SNK_TRACK_FRAME_WGS
    assert plan(10000, 1024, 1000, 2401, 1, 0, 0, 0) == [64, 0, -1, 0]         # SNK_TRACK_NO_FRAME_LDS: coarse_batch_kernel / fine_batch_kernel
    assert plan(100, 8, 1000, 2401, 0, 0, 0, 0) == [1, 0, -1, 0]


def test_track_launch_and_grid_thresholds_from_both_sides(driver):
    """The resolution of a batched matcher and the form of the feature grid: both neighbours of every threshold, and the capacities at
    which the plan of the 40 x 26 grid changes, found by asking for every capacity (tests/test_track_forms_gpu.py runs there)."""
    ask = lambda *q: forms.ask(driver, list(q))
    names = ["TRACK_RESOLVE_LDS_FEATURES", "TRACK_CHUNK_POINTS", "GRID_MAX_FEATURES", "GRID_COUNT_LDS_MAX"]
    assert dict(zip(names, map(int, ask(*[("const", (n,)) for n in names])))) == \
        {"TRACK_RESOLVE_LDS_FEATURES": 32768, "TRACK_CHUNK_POINTS": 1024, "GRID_MAX_FEATURES": 16384, "GRID_COUNT_LDS_MAX": 96 * 1024}
    assert ask(("track_resolve_lds", (32768,)), ("track_resolve_lds", (32769,)), ("track_resolve_lds", (1,)), ("track_resolve_lds", ((1 << 20) - 2,))) == \
        ["1", "0", "1", "0"]
    N1 = forms.NCELL1
    launch = lambda *a: ask(("track_launch", a))[0]
    # fused only with one workgroup per frame and the claims behind the frame; the separate resolution by the capacity alone
    assert launch(10000, 1024, 1000, 2401, 0, 0, 0, 0) == "frame/1/fused" and launch(10000, 1024, 1000, 2401, 0, 0, 1, 0) == "frame/1/lds"
    assert launch(10000, 512, 1000, 2401, 0, 0, 0, 0) == "frame/2/lds" and launch(10000, 1024, 1000, 2401, 1, 0, 0, 0) == "batch/0/lds"
    assert launch(100, 8, 32768, N1, 0, 0, 0, 64) == "batch/0/lds" and launch(100, 8, 32769, N1, 0, 0, 0, 64) == "batch/0/global"
    assert launch(2049, 7, 2203, N1, 0, 0, 0, 64) == "frame/3/lds"   # seven frames: a workgroup per chunk unless SNK_TRACK_FRAME_WGS says otherwise
    fused_end, frame_end = forms.track_plan_edges(driver, 2049, 7, N1, 1, 64)
    assert (fused_end, frame_end) == (2203, 2347)
    up = lambda v: (v + 15) & ~15
    assert up(frame_lds(2203, N1)) + 4 * 2203 == 147452 and up(frame_lds(2204, N1)) + 4 * 2204 == 147504 > 144 * 1024
    assert frame_lds(2347, N1) == 147412 and frame_lds(2348, N1) == 147460 > 144 * 1024
    # the grid: 2 (ncell + 1) + 2 cap ints in 96 KB; SNK_GRID_NETWORK
    lds = lambda n, c: int(ask(("grid_lds", (n, c)))[0])
    assert lds(11247, 1040) == 96 * 1024 and lds(11248, 1040) == 96 * 1024 + 8 and lds(0, 0) == 8 and lds(16384, 65534) == (2 * 65535 + 2 * 16384) * 4
    assert ask(("grid_form", (11247, 1040, 0)), ("grid_form", (11248, 1040, 0)), ("grid_form", (11247, 1040, 1)), ("grid_form", (1, 12286, 0)),
               ("grid_form", (1, 12287, 0)), ("grid_form", (0, 12287, 0)), ("grid_form", (16384, 1, 0)), ("grid_form", (1, 65534, 0))) == \
        ["count", "network", "network", "count", "network", "count", "network", "network"]
    assert forms.grid_form_edge(driver, 1040) == 11247 and forms.grid_form_edge(driver, 12000) == 287
    # no copy of a threshold is left in track.hip's code (its messages and comments may name the numbers)
    track = re.sub(r'"[^"\n]*"|//[^\n]*', "", (forms.ROOT / "snake_slam_amd" / "csrc" / "track.hip").read_text())
    assert not re.search(r"\b(32768|16384|96 \* 1024|98304)\b", track) and "grid_form(" in track and "track_resolve_in_lds(" in track


def test_orb_and_track_switch_lists_agree():
    """OrbSwitches (dispatch.hpp), its reader (orb.hip), the driver's parser, tests/forms.py and the README name the same switches; orb.hip
    reads the environment only there and for SNK_DEBUG, track.hip only in track_switches() (and SNK_GRID_NETWORK of the feature grid)."""
    csrc = forms.ROOT / "snake_slam_amd" / "csrc"
    header = (csrc / "dispatch.hpp").read_text()
    struct = re.search(r"struct OrbSwitches\s*\{(.*?)\n\};", header, re.S).group(1)
    fields = re.findall(r"^\s+(?:bool|int|size_t) \w+\s*=[^;]*;\s*// (\w+)", struct, re.M)
    assert fields == forms.ORB_SWITCHES
    orb = (csrc / "orb.hip").read_text()
    reader = re.search(r"static const OrbSwitches& orb_switches\(\)\n\{(.*?)\n\}\n", orb, re.S).group(1)
    assert sorted(set(re.findall(r'"SNK_ORB_(\w+)"', reader))) == sorted(forms.ORB_SWITCHES)
    assert re.findall(r'getenv\((\w+|"\w+")\)', orb.replace(reader, "")) == ['"SNK_DEBUG"']
    driver = (forms.ROOT / "tests" / "cpp" / "dispatch_driver.cpp").read_text()
    assert sorted(re.findall(r'is\("(\w+)"\)', driver)) == sorted(forms.ORB_SWITCHES)
    readme = (forms.ROOT / "README.md").read_text()
    assert all(f"SNK_ORB_{n}" in readme for n in forms.ORB_SWITCHES) and all(f"SNK_TRACK_{n}" in readme for n in forms.TRACK_SWITCHES)
    struct = re.search(r"struct TrackSwitches\s*\{(.*?)\n\};", header, re.S).group(1)
    assert re.findall(r"// SNK_TRACK_(\w+)", struct) == forms.TRACK_SWITCHES
    track = (csrc / "track.hip").read_text()
    reader = re.search(r"const TrackSwitches& track_switches\(\)\n\{(.*?)\n\}\n", track, re.S).group(1)
    assert sorted(re.findall(r'"SNK_TRACK_(\w+)"', reader)) == sorted(forms.TRACK_SWITCHES)
    assert re.findall(r'getenv\((\w+|"\w+")\)', track.replace(reader, "")) == ['"SNK_GRID_NETWORK"']
