// Which kernel form a launch shape selects: the ONE place where the thresholds of matcher.hip, pose.hip, mappoint.hip, covis.hip, localmap.hip, scene.hip, simp.hip, ba.hip,
// orb.hip (the extractor's whole launch plan, over the geometry of orb_layout.hpp) and track.hip (the projection matchers) live.
// Host-only and free of HIP includes, so that tests/cpp/dispatch_driver.cpp builds it with plain g++ and tests/forms.py can pin every
// shape of the GPU tests to the form it was written for.  launch_knn2, snk_stereo_match, stereo_match_batch_dev_impl, snk_pose_refine,
// refine_batch_impl, the BA solver (ba_plan_pcg, enqueue_lm), the extractor (snk_orb_configure, run_part, run_pipeline) and the batched
// projection matchers call these functions and keep no copy of the conditions; the environment switches are read there and passed in.
// The workgroup-level blocks that the map-side kernels share (sort, long scan, first-appearance table, list walk, reduction): wg.hpp.
#pragma once
#include <cstddef>

#include "handover_core.hpp"  // the BA hand-over from device rows: which problems its kernels take, their carves (HO_*, ho_*)
#include "orb_layout.hpp"

#ifndef SNK_POSE_RED_STEPS  // DPP steps of pose_kernel's 27 sums before they meet in LDS: 4 = rows of 16 lanes, 2 = quads (pose.hip)
#define SNK_POSE_RED_STEPS 2
#endif

namespace snk
{
// ---- the matcher handle's scratch as snk_matcher_create sizes it (matcher.hip): a call that needs more grows a buffer once -----------
constexpr size_t MATCHER_SCRATCH_BYTES = 4u << 20;    // q, t, out, aux, aux2, view: any per-frame call up to ~40 000 features / map points
constexpr size_t MATCHER_H_IN_BYTES    = 1u << 20;    // pinned input staging: 10 000 local-map points of the fine matcher
constexpr size_t MATCHER_H_RES_BYTES   = 256u << 10;  // pinned result staging
// What DevBuf::reserve(n) / HostBuf::reserve(n) allocate (common.hpp): a quarter more than asked for, so that a slowly growing call does
// not reallocate every time.  A buffer sized at create holds scratch_capacity(MATCHER_*_BYTES); only a call that asks for more than that
// frees and reallocates it.
constexpr size_t scratch_capacity(size_t n) { return n + n / 4 + 256; }

// ---- brute-force kNN-2 (launch_knn2) ----------------------------------------------------------------------------------------------
constexpr int BF_MFMA_MIN      = 24;     // matrix-core kernel once a query block (32) and a train tile (32) are mostly full
constexpr int BF_WIDE_MIN_WORK = 16384;  // batch * nq_cap from which a wavefront takes four queries (enough work for 256 CUs)

enum class Knn2Form { vector1, vector4, mfma };

inline Knn2Form knn2_form(int nq_cap, int nt_cap, int batch, bool no_mfma)
{
    if (!no_mfma && nq_cap >= BF_MFMA_MIN && nt_cap >= BF_MFMA_MIN) return Knn2Form::mfma;
    return (long long)batch * nq_cap >= BF_WIDE_MIN_WORK ? Knn2Form::vector4 : Knn2Form::vector1;
}

// Inside Knn2Form::mfma: two query blocks (64 queries) per wavefront -- the wide form, 256 queries per workgroup -- instead of one.
// It halves the LDS reads, the train expansion and the barriers per query, and the number of workgroups with them; so it is
// taken from BF_MFMA_WIDE_MIN_WGS wide workgroups on: with 1000 queries per frame it equals the narrow form at 64 frames (256 wide
// workgroups) and is ahead at 128 (512), the first measured point where it wins (profiles/NOTES.md, r08).
// wide_env: SNK_BF_MFMA_WIDE (0 / 1 force a form, -1 = unset).
constexpr int BF_MFMA_WIDE_MIN_WGS = 512;

constexpr bool knn2_mfma_wide(int nq_cap, int /*nt_cap*/, int batch, int wide_env)
{
    return wide_env >= 0 ? wide_env != 0 : (long long)batch * ((nq_cap + 255) / 256) >= BF_MFMA_WIDE_MIN_WGS;
}

// Inside Knn2Form::mfma: keys of distance << 13 | index, which the matrix pipe forms whole (matcher.hip), while every train index
// fits 13 bits; 20-bit keys formed by the vector ALU beyond.  allowed: false under SNK_BF_MFMA_NO_SHORT.
constexpr int BF_MFMA_SHORT_NT = 8192;

constexpr bool knn2_mfma_short(int nt_cap, bool allowed) { return allowed && nt_cap <= BF_MFMA_SHORT_NT; }

// ---- stereo matcher (snk_stereo_match, stereo_match_batch_dev_impl) ---------------------------------------------------------------
constexpr int ST_SORT_MAX     = 8192;  // right keypoints per image the in-LDS row index handles
constexpr int ST_FRAME_MAX    = 2560;  // right keypoints per frame stereo_frame_kernel keeps in LDS
constexpr int ST_FRAME_BATCH  = 8;     // frames from which one workgroup per frame fills the chip
constexpr int ST_COUNT_ROWS   = 4096;  // row span the counting index covers; a wider frame runs the network inside the same launch

// frame: stereo_frame_kernel;  count16 / sort16: row index by stereo_count_kernel / stereo_sort_kernel, then stereo_kernel16;
// unindexed: stereo_kernel over every right keypoint
enum class StereoForm { frame, count16, sort16, unindexed };

inline StereoForm stereo_host_form(int nr, bool sort_network)
{
    if (nr > ST_SORT_MAX) return StereoForm::unindexed;
    return sort_network ? StereoForm::sort16 : StereoForm::count16;
}

inline StereoForm stereo_batch_form(int nr_cap, int batch, bool no_frame_kernel, bool sort_network)
{
    if (!no_frame_kernel && nr_cap <= ST_FRAME_MAX && batch >= ST_FRAME_BATCH) return StereoForm::frame;
    return stereo_host_form(nr_cap, sort_network);
}

// ---- pose refinement (snk_pose_refine, refine_batch_impl) -------------------------------------------------------------------------
constexpr int POSE_SLOTS_PER_WAVE   = 64 >> SNK_POSE_RED_STEPS;
constexpr int POSE_HOST_WAVE4_MEAN  = 192;  // matches per problem on average from which the host entry runs four wavefronts
constexpr int POSE_BATCH_WAVE4_MIN  = 256;  // row length of the batched entry from which a frame gets more than one wavefront
constexpr int POSE_TWO_PER_CU_BATCH = 256;  // more problems than this: the carve is sized so that two share a compute unit
constexpr int POSE_MATCH_BYTES      = 56;   // a match in LDS: seven doubles

enum class PoseForm { wave1, wave2_lds, wave4_lds, wave4_global };

// dynamic LDS a workgroup can have beside pose_kernel's static part
constexpr int pose_dyn_max() { return 160 * 1024 - (4 * POSE_SLOTS_PER_WAVE * 28 + 28) * 8 - 2048; }
// matches of a problem in LDS so that carve + static LDS <= 80 KB: two problems per compute unit
constexpr int pose_two_per_cu() { return (80 * 1024 - (4 * POSE_SLOTS_PER_WAVE * 28 + 28) * 8 - 256) / POSE_MATCH_BYTES; }
// the same for the two-wavefront form: four frames per compute unit
constexpr int pose_four_per_cu() { return (160 * 1024 / 4 - (2 * POSE_SLOTS_PER_WAVE * 28 + 28) * 8 - 512) / POSE_MATCH_BYTES; }

inline PoseForm pose_host_form(size_t total, int n_problems, bool no_lds)
{
    if (total < (size_t)n_problems * POSE_HOST_WAVE4_MEAN) return PoseForm::wave1;
    return no_lds ? PoseForm::wave4_global : PoseForm::wave4_lds;
}

// LDS carve of the host entry's four-wavefront form, in matches: the largest problem, capped to two problems per CU in a large call
inline int pose_host_carve(int n_max, int n_problems)
{
    int lds_matches = n_max;
    if (n_problems > POSE_TWO_PER_CU_BATCH && lds_matches > pose_two_per_cu()) lds_matches = pose_two_per_cu();
    if ((size_t)lds_matches * POSE_MATCH_BYTES > (size_t)pose_dyn_max()) lds_matches = pose_dyn_max() / POSE_MATCH_BYTES;
    return lds_matches;
}

// n_cu: compute units of the device; waves_env: SNK_POSE_WAVES (2 or 4 force a form, 0 = unset)
inline bool pose_batch_two_waves(int batch, int n_cu, int waves_env) { return waves_env == 2 || (waves_env != 4 && batch > 2 * n_cu); }

inline PoseForm pose_batch_form(int stride, int batch, int n_cu, int waves_env, bool no_lds)
{
    if (stride < POSE_BATCH_WAVE4_MIN) return PoseForm::wave1;
    if (no_lds) return PoseForm::wave4_global;
    return pose_batch_two_waves(batch, n_cu, waves_env) ? PoseForm::wave2_lds : PoseForm::wave4_lds;
}

// LDS carve of the batched entry, in matches.  lds_env: SNK_POSE_LDS_MATCHES (0 = unset); two_waves: the launch is wave2_lds
inline int pose_batch_carve(int stride, int batch, int lds_env, bool two_waves)
{
    int lds_matches = stride;
    if (two_waves)
    {
        const int lm = lds_env > 0 ? lds_env : pose_four_per_cu();
        lds_matches  = lm < stride ? lm : stride;
    }
    else if (lds_env > 0) lds_matches = lds_env < stride ? lds_env : stride;
    else if (batch > POSE_TWO_PER_CU_BATCH && lds_matches > pose_two_per_cu()) lds_matches = pose_two_per_cu();
    if ((size_t)lds_matches * POSE_MATCH_BYTES > (size_t)pose_dyn_max()) lds_matches = pose_dyn_max() / POSE_MATCH_BYTES;
    return lds_matches;
}

// ---- map-point refresh (mappoint.hip: snk_mappoint_refresh, snk_mappoint_refresh_batch_dev) ----------------------------------------
// packed: mp_packed_kernel, a lane per observation row, the points of a 64-point chunk packed into wavefronts (no point straddles
// one), the row of distances in registers;  wide: mp_wide_kernel, a workgroup per point, rows strided over its lanes.
constexpr int MP_PACKED_MAX_K   = 32;    // observations up to which a point's rows share a wavefront: 16 registers hold its row of distances
constexpr int MP_CHUNK_POINTS   = 64;    // points per workgroup of the packed form: one lane of its first wavefront plans each
constexpr int MP_CHUNK_SLOTS    = 64;    // wavefront-sized row groups a chunk can need: a closed group holds more than 64 - 32 rows
constexpr int MP_PACKED_THREADS = 256;
constexpr int MP_WIDE_THREADS   = 1024;
constexpr int MP_WIDE_MAX_WGS   = 1024;  // the wide form's workgroups walk the list of wide points
constexpr int MP_WIDE_MAX_K     = 4096;  // = SNK_MP_MAX_OBS

enum class MpForm { packed, wide };

// form_env: SNK_MP_FORM (0 = unset, 1 = "packed": the default rule, 2 = "wide": every point on a workgroup of its own)
constexpr MpForm mp_form(int k, int form_env) { return form_env != 2 && k <= MP_PACKED_MAX_K ? MpForm::packed : MpForm::wide; }

// LDS carve of a packed workgroup whose chunk has at most `rows` packed rows: descriptors (32 B), a flag byte per row, the
// row -> (point, observation) map of the chunk's slots, four ints per point and the slot count
constexpr size_t mp_packed_carve(int rows)
{
    return (size_t)rows * 32 + (size_t)((rows + 15) & ~15) + (size_t)MP_CHUNK_SLOTS * 64 * 2 + (size_t)MP_CHUNK_POINTS * 16 + 16;
}
// ... of a wide workgroup for points of at most k_cap observations: descriptors (the unit vectors of the normal use the same bytes
// before them, 24 B each), a flag byte per observation, a key per wavefront and two ints
constexpr size_t mp_wide_carve(int k_cap) { return (size_t)k_cap * 32 + (size_t)((k_cap + 15) & ~15) + (size_t)(MP_WIDE_THREADS / 64) * 8 + 16; }
// the device-resident entry cannot look at the lists: the largest chunk and the largest point
constexpr int mp_packed_rows_max() { return MP_CHUNK_POINTS * MP_PACKED_MAX_K; }

// ---- covisibility (covis.hip: snk_covis_update, snk_covis_vote and their _batch_dev forms) ------------------------------------------
// covis_kernel: a workgroup per set.  A lane takes a feature; a list of at most covis_long_min observations it walks itself, a longer
// one it queues in LDS and a wavefront walks it, a lane per observation.
constexpr int COVIS_THREADS  = 256;  // four wavefronts: several workgroups share a compute unit at the usual few thousand keyframes
constexpr int COVIS_LONG_MIN = 32;   // observations above which a list is walked by a wavefront (a lane alone would hold its 63 neighbours up)
constexpr int COVIS_MISC     = 32;   // u32 words of flags, sums, the fallback key and the per-wavefront partial counts

// long_env: SNK_COVIS_LONG_MIN (< 0 = unset; n >= 0: lists longer than n observations are queued -- 0 queues every list)
constexpr int covis_long_min(int long_env) { return long_env >= 0 ? long_env : COVIS_LONG_MIN; }
// ids the in-LDS sort holds: the entries kept (at most cap, at most n_kf) rounded up to a power of two, at least four
constexpr int covis_sort_len(int n_kf, int cap)
{
    int n = 4;
    while (n < cap && n < n_kf) n <<= 1;
    return n;
}
// LDS carve of a workgroup: a u32 counter per keyframe, the ids to sort, the queue of long lists (a point id per lane), the words above
constexpr size_t covis_carve(int n_kf, int cap)
{
    return (size_t)((n_kf + 3) & ~3) * 4 + (size_t)covis_sort_len(n_kf, cap) * 4 + (size_t)COVIS_THREADS * 4 + (size_t)COVIS_MISC * 4;
}

// ---- local map of fine tracking (localmap.hip: snk_lmap_select, snk_lmap_gather and their _batch_dev forms) --------------------------
// One form each.  lmap_select_kernel: a workgroup per set; the marks are a bit per keyframe, the neighbour candidates (a slot per local
// keyframe and neighbour rank) are sorted by kf << bits | slot.  lmap_gather_kernel: a workgroup per set; an open-addressing table of
// four-byte slots (candidate order + 1, bit 31 = "also an own point") over the point ids.
constexpr int LMAP_THREADS = 256;  // four wavefronts; a scan chunk is one candidate per lane
constexpr int LMAP_MISC    = 32;   // u32 words of flags, counts and the per-wavefront partial sums (two banks)

constexpr int lmap_pow2_at_least(int n, int least)
{
    int p = least;
    while (p < n) p <<= 1;
    return p;
}
// keys the neighbour sort holds: a slot per (local keyframe, neighbour rank), rounded up to a power of two
constexpr int lmap_sort_len(int kf_cap, int n_neighbours) { return lmap_pow2_at_least(kf_cap * n_neighbours, 4); }
// slots of the point table: load at most 0.5 at pts_cap, and room for the claims in flight when the count passes pts_cap (one per lane)
constexpr int lmap_table_slots(int pts_cap) { return lmap_pow2_at_least(2 * pts_cap, 2 * LMAP_THREADS); }
// LDS carve of lmap_select_kernel: the marks, the local list, the sort keys, the neighbour firsts by slot, the words above
constexpr size_t lmap_select_carve(int n_kf, int kf_cap, int n_neighbours)
{
    return (size_t)((n_kf + 31) / 32 + 1) * 4 + (size_t)kf_cap * 4 + (size_t)lmap_sort_len(kf_cap, n_neighbours) * 8 + (size_t)LMAP_MISC * 4;
}
// LDS carve of lmap_gather_kernel: the table, the prefix sums of the feature ranges (kf_cap + 1), their starts (kf_cap), the words above
constexpr size_t lmap_gather_carve(int kf_cap, int pts_cap)
{
    return (size_t)lmap_table_slots(pts_cap) * 4 + (size_t)(2 * kf_cap + 1) * 4 + (size_t)LMAP_MISC * 4;
}

// ---- local BA windows (scene.hip: snk_scene_window, snk_scene_gather and their _batch_dev forms) -------------------------------------
// One form each, a workgroup per query.  scene_window_kernel: one wavefront, a lane per candidate.  scene_gather_kernel: four wavefronts;
// its carve is used twice: first the first-appearance table of wg.hpp (four-byte slots, as lmap_gather_kernel), then, the point list being in the pt_id row,
// the fixed-camera table (a key and a value per slot), the sort keys of the fixed cameras, a base per image and the words of a chunk.
constexpr int SCENE_WIN_THREADS = 64;   // one wavefront: a lane per candidate (SCENE_MAX_WINDOW)
constexpr int SCENE_THREADS     = 256;  // four wavefronts; a chunk is one point or one observation per lane
constexpr int SCENE_MISC        = 32;   // u32 words of flags, counts and the per-wavefront partial sums (two banks)
constexpr int SCENE_WIN_SLOTS   = 64;   // window keyframes kept in LDS (SCENE_MAX_WINDOW)

constexpr size_t scene_window_carve() { return (size_t)(SCENE_WIN_SLOTS + 4) * 4; }
// slots of the fixed-camera table: load at most 0.5 at img_cap, room for a claim per lane in flight
constexpr int scene_img_slots(int img_cap) { return lmap_pow2_at_least(2 * img_cap, 2 * SCENE_THREADS); }
constexpr int scene_sort_len(int img_cap) { return lmap_pow2_at_least(img_cap, 4); }
// phase 1: the point table, the prefix sums (65) and the starts (64) of the window's feature ranges
constexpr size_t scene_points_carve(int pt_cap) { return (size_t)lmap_table_slots(pt_cap) * 4 + (size_t)(2 * SCENE_WIN_SLOTS + 1) * 4; }
// phase 2: key and value per slot, the sort keys, a base per image, per chunk: the points' stream starts (257), their observation starts,
// their ids and constant flags packed (256), the images of a chunk's records (256)
constexpr size_t scene_obs_carve(int img_cap)
{
    return (size_t)scene_img_slots(img_cap) * 8 + (size_t)scene_sort_len(img_cap) * 4 + (size_t)img_cap * 4 + (size_t)(4 * SCENE_THREADS + 1) * 4;
}
// LDS carve of scene_gather_kernel: the window keyframes and the words above, then the larger of the two phases
constexpr size_t scene_gather_carve(int pt_cap, int img_cap)
{
    const size_t a = scene_points_carve(pt_cap), b = scene_obs_carve(img_cap);
    return (size_t)(SCENE_WIN_SLOTS + SCENE_MISC) * 4 + (a > b ? a : b);
}

// ---- keyframe culling (simp.hip: snk_simp_stats, snk_simp_decide and their _batch_dev forms) ------------------------------------------
// One form each, a workgroup of four wavefronts per query.  simp_stats_kernel: a lane per feature, a list of at most simp_long_min
// observations is walked by its lane, a longer one by a wavefront (walk_lists of wg.hpp, as covis_kernel); the depths stay in LDS for the radix select.
// simp_decide_kernel: a lane per node, the strict upper triangle of the weight matrix in LDS.
constexpr int SIMP_THREADS  = 256;
constexpr int SIMP_LONG_MIN = 32;  // observations above which a list is walked by a wavefront
constexpr int SIMP_MISC     = 32;  // u32 words of flags, counts and the partial results of the reductions (two banks of four u64)
// long_env: SNK_SIMP_LONG_MIN (< 0 = unset; n >= 0: lists longer than n observations are queued -- 0 queues every walked list)
constexpr int simp_long_min(int long_env) { return long_env >= 0 ? long_env : SIMP_LONG_MIN; }
// LDS carve of simp_stats_kernel: a key per feature, the queue of long lists (a feature per lane and round), the words above
constexpr size_t simp_stats_carve(int feat_cap) { return (size_t)((feat_cap + 3) & ~3) * 4 + (size_t)SIMP_THREADS * 4 + (size_t)SIMP_MISC * 4; }
// LDS carve of simp_decide_kernel: the triangle (an even number of words), the sorted node keys, the nodes' keyframes, the words above
constexpr size_t simp_decide_carve(int max_nodes)
{
    return (size_t)((max_nodes * (max_nodes - 1) / 2 + 1) & ~1) * 4 + (size_t)max_nodes * 8 + (size_t)((max_nodes + 1) & ~1) * 4 + (size_t)SIMP_MISC * 4;
}

// ---- bundle adjustment (ba.hip: ba_plan_pcg, enqueue_lm, snk_ba_solve_async, snk_ba_pcg_form; the hand-over asks ba_sets_will_run) --
constexpr int BA_SET_MIN_ITEMS = 256;  // a single small window has too few work items to fill the chip, the block-major pass is quicker there

// Every SNK_BA_* switch that selects a code path of the solver, and SNK_DEBUG.  ba.hip fills one per process (ba_switches()); the
// hand-over's own host-side switches stay in ba_handover.hip.  Integer fields: 0 = unset where not said otherwise.
struct BaSwitches
{
    bool pcg_general          = false;  // PCG_GENERAL: the 256-thread PCG loop for every size (A/B against the replicated one)
    bool no_point_wave        = false;  // NO_POINT_WAVE: thread-per-point linearisation, update and cost
    bool no_schur_set         = false;  // NO_SCHUR_SET: never the point-major Schur pass
    long long set_min_items   = BA_SET_MIN_ITEMS;  // SCHUR_SET_MIN_ITEMS: work items of a call from which the point-major pass runs
    bool no_schur_mfma        = false;  // NO_SCHUR_MFMA: A/B: the vector-ALU form (schur_set)
    bool no_schur_fused       = false;  // NO_SCHUR_FUSED: A/B: point_wave + schur_mfma through W in HBM
    bool fused_k10            = false;  // FUSED_K10: schur_fused<4> also where points have 9-10 free observations (tests)
    bool cam_sums             = false;  // CAM_SUMS: schur_fused<3, true> + cam_sum instead of cam_pass
    bool cam_grid_2d          = false;  // CAM_GRID_2D: A/B: the round-1..4 grid (cameras of a window over all XCDs)
    bool no_schur_wide        = false;  // NO_SCHUR_WIDE: A/B: schur_pass<1> also for single windows
    bool pcg_lds              = false;  // PCG_LDS: A/B: S in LDS (pcg_solve<true>) also for local-BA sizes
    bool no_update_cost       = false;  // NO_UPDATE_COST: A/B: update_wave + cost_wave
    bool flat_barrier         = false;  // FLAT_BARRIER: every workgroup polls every flag (the round-5 grid barrier)
    bool pcg_timing           = false;  // PCG_TIMING (diagnostic): pcgl_persist_reg's cycles per phase on stderr
    bool pcgl_launches        = false;  // PCGL_LAUNCHES: the multi-launch PCG instead of the one cooperative launch
    bool persist_two_barriers = false;  // PERSIST_TWO_BARRIERS: A/B: pcgl_persist (the round-5 form) instead of pcgl_persist1
    bool persist_stream       = false;  // PERSIST_STREAM: pcgl_persist1 streams its rows of S instead of pcgl_persist_reg's registers
    int persist_wgs           = -1;     // PERSIST_WGS: workgroups of the cooperative launch (-1: unset; <= 0: by the problem's size)
    int persist_reg_rows      = 0;      // PERSIST_REG_ROWS: 8 or 16 rows of S per workgroup of pcgl_persist_reg (0: by the size)
    bool persist_fail         = false;  // PERSIST_FAIL (tests): the runtime refuses the cooperative launch
    int graph_chains          = 0;      // GRAPH_CHAINS: chains a recorded batch sequence is split into (0: BA_GRAPH_CHAINS)
    bool no_graph             = false;  // NO_GRAPH: plain launches always
    bool graph_first          = false;  // GRAPH_FIRST: the graph already at the first solve of a problem set
    bool local_sync           = false;  // LOCAL_SYNC: A/B: snk_ba_solve_local_scene decides about the extra iteration on the host
    bool debug                = false;  // SNK_DEBUG: which forms a solve enqueued, on stderr

    // a switch that takes the point-major pass off its default kernels (schur_fused + update_cost): the hand-over then keeps work
    // items of <= 64 points, the only ones the alternative kernels walk (SET_CHUNK_BIG in ba_types.hpp)
    bool any_alt_path() const { return no_schur_fused || no_schur_mfma || no_update_cost || fused_k10 || no_schur_set || no_point_wave; }
};

// The totals of a problem set that the decisions depend on (fields of ba::Handle and of its PCG plan).
struct BaShape
{
    int count = 0;  // problems of the set
    bool implicit = false;
    int max_n6 = 0, max_nfc = 0, max_np = 0, max_ni = 0, max_wv = 0, max_rpc = 0, max_set_items = 0;
    bool set_ok = false, set_small = false;
    int set_k_max = 0, set_run_max = 0;
    bool point_wave_ok = false, cam_sums_ok = false, blk_built = true;
    int persist_wgs = 0, persist_one = 0, persist_rows = 0;  // ba_plan_pcg's answer (BaPersist); a refused cooperative launch zeroes persist_wgs
};

// points with 9 or 10 free observations need a fourth tile row: 260 registers, one wavefront per SIMD -- there the linearisation
// stays in point_wave and schur_mfma<4> reads W (measured on the 300-keyframe global BA: 14.7 vs 15.5 ms)
constexpr int BA_FUSED3_MAX_K           = 8;
constexpr int BA_CAM64_MIN_BATCH        = 16;    // windows from which a camera gets one wavefront (cam_pass<64>), not a workgroup of four
constexpr int BA_SCHUR_WIDE_BATCH_END   = 16;    // fewer windows than this and ...
constexpr int BA_SCHUR_WIDE_MAX_BLOCKS  = 8192;  // ... at most this many camera-pair blocks: a workgroup per block (schur_pass<4>)
constexpr int BA_PCG_SMALL_MAX_N6       = 128;   // unknowns up to which pcg_small keeps its quarter of S in registers
constexpr int BA_PCG_LDS_MAX            = 158 * 1024;  // LDS of pcg_solve / pcg_small: S (and the vectors) of the largest problem fit -> one workgroup per problem
constexpr int BA_PERSIST_LDS_MAX        = 150 * 1024;  // LDS of the persistent PCG forms (p; r, z, p in the one-barrier form)
constexpr int PREG_MAX_N6               = 2048;  // pcgl_persist_reg: 8 rows x 2048 columns of S in a workgroup's registers
// 16 rows per workgroup above 512 unknowns (the barrier and the exchange of A p grow with the workgroups: 225 against 113 for 300
// keyframes: 9.4 -> 7.1 us per PCG iteration; 90 against 45 for 120 keyframes: 6.45 -> 5.7), 8 below
constexpr int BA_PREG_ROWS16_ABOVE_N6   = 512;
constexpr int BA_SPLIT_COPY_MAX_BATCH   = 4;     // big problems in small numbers: the copy of the accepted state on its own workgroups
constexpr int BA_SPLIT_COPY_MIN_POINTS  = 4096;
constexpr int BA_GRAPH_CHAINS           = 1;     // chains a recorded batch sequence is split into by default (measured +1 % with 2, -6 % with 4)
constexpr int BA_GRAPH_CHAINS_MIN_BATCH = 128;   // windows from which a recorded sequence may be split at all ...
constexpr int BA_GRAPH_CHAIN_MIN        = 64;    // ... into chains of at least this many
constexpr int SUM_NB          = 4;  // schur_sum, measured per 1024 windows: 1 block per wavefront 118 us, 4: 90 us, 8: 151 us (profiles/r05/r05Q_, r05R_)
constexpr int PERSIST_WGS_MAX = 1024;
constexpr int PERSIST_THREADS = 256;
constexpr int PERSIST_CAMS    = PERSIST_THREADS / 6;  // 42 cameras (252 elements) per workgroup in the update phase
constexpr int IMP_THREADS     = 256;
constexpr int PERSIST_MIN_WGS = 16;  // the fewest workgroups a cooperative PCG launch asks for
constexpr int PERSIST_ROWS_PER_WG = 12;  // pcgl_persist / pcgl_persist1: a dozen rows of S per workgroup (FullBA(4), n6 = 1794: 5.0 / 4.6 / 5.9 / 5.0 ms with 256 / 128 / 64 / 32)

constexpr int ba_ceil_div(int a, int b) { return (a + b - 1) / b; }
constexpr int ba_max(int a, int b) { return a > b ? a : b; }
constexpr int ba_min(int a, int b) { return a < b ? a : b; }

// Will the LM sequence of this problem set run the point-major kernels (schur_fused / schur_mfma + update_cost over the camera-set work
// items)?  The hand-over asks too, because the camera-pair block entries are only read by the block-major pass (schur_pass) -- building
// them for a 1024-window batch that never runs it was 1.4 ms of device time behind every hand-over (block_entries_count 0.40 +
// block_entries_fill 1.03 ms, round 6 trace).
inline bool ba_sets_will_run(const BaShape& s, const BaSwitches& sw)
{
    return s.max_nfc > 0 && s.point_wave_ok && !sw.no_point_wave && s.set_ok && !sw.no_schur_set && (long long)s.max_set_items * s.count >= sw.set_min_items;
}

// LDS of the per-problem PCG without S: nine n6-vectors and the preconditioner blocks
constexpr size_t ba_pcg_vec_lds(int max_n6, int max_nfc) { return (size_t)max_n6 * 9 * 8 + (size_t)max_nfc * 36 * 8; }
// S (and the vectors) of the largest problem fit one workgroup's LDS -> one workgroup per problem; otherwise the multi-workgroup
// PCG (measured: 120 keyframes 38 ms -> 9 ms, 600 keyframes 21 ms)
constexpr bool ba_pcg_is_large(int max_n6, int max_nfc, bool implicit)
{
    return !implicit && ba_pcg_vec_lds(max_n6, max_nfc) + (size_t)max_n6 * max_n6 * 8 > (size_t)BA_PCG_LDS_MAX;
}

// A recorded sequence of a big batch may be split into chains over disjoint ranges of the windows (enqueue_lm).
inline int ba_graph_chains(int count, bool recording, bool pcg_large, int chains_env)
{
    if (!recording || pcg_large || count < BA_GRAPH_CHAINS_MIN_BATCH) return 1;
    return chains_env > 0 ? ba_min(chains_env, count / BA_GRAPH_CHAIN_MIN) : BA_GRAPH_CHAINS;
}

// ---- the cooperative (one-launch) PCG forms: what ba_plan_pcg asks the runtime, and what it makes of the answers --------------------
struct BaPersist
{
    int wgs = 0, one = 0, rows = 0;  // workgroups (0: multi-launch); 0 pcgl_persist, 1 pcgl_persist1, 2 pcgl_persist_reg<rows>
};
// SNK_BA_PERSIST_WGS or `natural`, at most one per compute unit and PERSIST_WGS_MAX: the barrier's cost grows with the participants
// (measured 7.0 ms per FullBA(4) with 256, 10.4 with 512)
inline int ba_persist_wgs_wanted(int natural, int n_cu, const BaSwitches& sw)
{
    return ba_min(PERSIST_WGS_MAX, sw.persist_wgs > 0 ? sw.persist_wgs : ba_min(n_cu, ba_max(PERSIST_MIN_WGS, natural)));
}
inline bool ba_persist_tried(int count, const BaSwitches& sw) { return count == 1 && !sw.pcgl_launches; }
// p in LDS; partial-sum slots
inline bool ba_persist_fits(int max_n6, int max_nfc) { return (size_t)max_n6 * 8 <= (size_t)BA_PERSIST_LDS_MAX && ba_ceil_div(max_nfc, PERSIST_CAMS) <= PERSIST_WGS_MAX; }
// the one-barrier form needs 3 n6 doubles of LDS
inline bool ba_persist1_fits(int max_n6, const BaSwitches& sw) { return (size_t)max_n6 * 24 <= (size_t)BA_PERSIST_LDS_MAX && !sw.persist_two_barriers; }
// the register-row rule of pcgl_persist_reg
inline int ba_persist_reg_rows(int max_n6, const BaSwitches& sw)
{
    return sw.persist_reg_rows == 8 || sw.persist_reg_rows == 16 ? sw.persist_reg_rows : (max_n6 > BA_PREG_ROWS16_ABOVE_N6 ? 16 : 8);
}
inline bool ba_persist_reg_fits(int max_n6, const BaSwitches& sw)
{
    return max_n6 <= PREG_MAX_N6 && !sw.persist_stream && sw.persist_wgs < 0 &&
           ba_ceil_div(ba_max(max_n6, 1), ba_persist_reg_rows(max_n6, sw)) <= PERSIST_WGS_MAX;
}
// The dense form.  coop: cooperative launch is available; res_*: resident workgroups per compute unit the runtime reports for
// pcgl_persist (n6 doubles of LDS), pcgl_persist1 (3 n6) and pcgl_persist_reg<rows> (2 n6) -- 0: refused or not asked.  All
// workgroups must be resident at once (grid barriers inside).
inline BaPersist ba_persist_dense(int count, int max_n6, int max_nfc, bool coop, int n_cu, int res_persist, int res_persist1, int res_reg,
                                  const BaSwitches& sw)
{
    BaPersist P;
    if (!ba_persist_tried(count, sw) || !coop || !ba_persist_fits(max_n6, max_nfc) || res_persist < 1) return P;
    const int wgs = ba_persist_wgs_wanted(ba_ceil_div(max_n6, PERSIST_ROWS_PER_WG), n_cu, sw);
    if (wgs < 1) return P;
    P.wgs = ba_min(wgs, res_persist * n_cu);
    if (ba_persist1_fits(max_n6, sw) && res_persist1 >= 1 && res_persist1 * n_cu >= P.wgs) P.one = 1;
    // ... and with S in registers when the system is small enough (one workgroup per 8 or 16 rows)
    const int rows = ba_persist_reg_rows(max_n6, sw), wgs_reg = ba_ceil_div(ba_max(max_n6, 1), rows);
    if (P.one == 1 && ba_persist_reg_fits(max_n6, sw) && res_reg >= 1 && res_reg * n_cu >= wgs_reg) P.one = 2, P.rows = rows, P.wgs = wgs_reg;
    return P;
}
// The implicit form (imp_persist): enough workgroups for a point per thread or a camera per wavefront
inline BaPersist ba_persist_implicit(int max_np, int max_nfc, bool coop, int n_cu, int res_imp, const BaSwitches& sw)
{
    BaPersist P;
    if (sw.pcgl_launches || max_nfc <= 0 || !coop || res_imp < 1) return P;
    const int want = ba_max(ba_ceil_div(max_np, IMP_THREADS), ba_ceil_div(max_nfc, IMP_THREADS / 64));
    P.wgs = ba_min(ba_persist_wgs_wanted(want, n_cu, sw), res_imp * n_cu);
    return P;
}

// ---- one LM iteration: a kernel form per stage ---------------------------------------------------------------------------------------
// linearisation: schur_fused<3, false> | <3, true> | <4, false> (with the Schur products), point_wave, point_pass<0>
enum class BaLinForm { fused3, fused3_sums, fused4, point_wave, point_pass };
// camera pass: none without free cameras; cam_sum, cam_pass<64> on the per-XCD grid | the 2-D grid, cam_pass<256>
enum class BaCamForm { none, cam_sum, cam64_xcd, cam64_2d, cam256 };
// Schur complement: none (implicit form, no free cameras), inside schur_fused, schur_mfma<3, 2> | <3, 3> | <4, 3>, schur_set<4, 2> | <6, 3>
// (each followed by schur_sum), schur_pass<4> | <1>
enum class BaSchurForm { none, in_fused, mfma32, mfma33, mfma43, set42, set63, pass4, pass1 };
// PCG: none without free cameras; pcg_small, pcg_solve<true> | <false>, pcgl_persist_reg<16> | <8>, pcgl_persist1, pcgl_persist, the
// dense multi-launch sequence (pcgl_*), imp_persist, the implicit multi-launch sequence (imp_*)
enum class BaPcgForm { none, small, solve_lds, solve_global, persist_reg16, persist_reg8, persist1, persist, launches, imp_persist, imp_launches };
// update and cost: update_pass + update_cost, update_wave + cost_wave, update_pass + point_pass<1>
enum class BaUpdateForm { update_cost, update_wave, update_point };

// the names of the forms, in the order of the enums: the plan line of enqueue_lm (SNK_DEBUG) and tests/cpp/dispatch_driver.cpp print them
inline const char* ba_name(BaLinForm f)
{
    static const char* const n[] = {"fused3", "fused3_sums", "fused4", "point_wave", "point_pass"};
    return n[(int)f];
}
inline const char* ba_name(BaCamForm f)
{
    static const char* const n[] = {"none", "cam_sum", "cam64_xcd", "cam64_2d", "cam256"};
    return n[(int)f];
}
inline const char* ba_name(BaSchurForm f)
{
    static const char* const n[] = {"none", "in_fused", "mfma32", "mfma33", "mfma43", "set42", "set63", "pass4", "pass1"};
    return n[(int)f];
}
inline const char* ba_name(BaPcgForm f)
{
    static const char* const n[] = {"none", "small", "solve_lds", "solve_global", "persist_reg16", "persist_reg8", "persist1", "persist", "launches",
                                    "imp_persist", "imp_launches"};
    return n[(int)f];
}
inline const char* ba_name(BaUpdateForm f)
{
    static const char* const n[] = {"update_cost", "update_wave", "update_point"};
    return n[(int)f];
}

inline bool ba_pcg_is_cooperative(BaPcgForm f)
{
    return f == BaPcgForm::persist_reg16 || f == BaPcgForm::persist_reg8 || f == BaPcgForm::persist1 || f == BaPcgForm::persist || f == BaPcgForm::imp_persist;
}

// The PCG form of a problem set (with free cameras) and its dynamic LDS.  recording: the sequence becomes graph nodes, and a
// cooperative launch is not a graph node.
inline BaPcgForm ba_pcg_form(const BaShape& s, const BaSwitches& sw, bool recording, size_t* lds = nullptr)
{
    size_t bytes  = 0;
    BaPcgForm f   = BaPcgForm::launches;
    const bool co = s.persist_wgs > 0 && !recording;
    if (s.implicit)
        f = co ? BaPcgForm::imp_persist : BaPcgForm::imp_launches;
    else if (!ba_pcg_is_large(s.max_n6, s.max_nfc, false))
    {
        bytes = ba_pcg_vec_lds(s.max_n6, s.max_nfc);
        // + 128 doubles read padding behind S (rows lane and lane + 64 are read unmasked) + [2][4][128] partial products
        const size_t with_s = bytes + (size_t)s.max_n6 * s.max_n6 * 8 + 1024 + 8192;
        if (s.max_n6 <= BA_PCG_SMALL_MAX_N6 && !sw.pcg_general && !sw.pcg_lds)
            f = BaPcgForm::small, bytes = ((size_t)s.max_n6 * 9 + (size_t)s.max_nfc * 72) * 8 + 8192;
        else if (with_s <= (size_t)BA_PCG_LDS_MAX)
            f = BaPcgForm::solve_lds, bytes = with_s;
        else
            f = BaPcgForm::solve_global;
    }
    else if (co && s.count == 1)
    {
        if (s.persist_one == 2) f = s.persist_rows == 16 ? BaPcgForm::persist_reg16 : BaPcgForm::persist_reg8, bytes = (size_t)s.max_n6 * 16;
        else if (s.persist_one) f = BaPcgForm::persist1, bytes = (size_t)s.max_n6 * 24;
        else f = BaPcgForm::persist, bytes = (size_t)s.max_n6 * 8;
    }
    if (lds) *lds = bytes;
    return f;
}

// "Graph or plain launches" of snk_ba_solve_async.  A cooperative launch is not a graph node: scenes solved by a one-launch PCG (global
// BA, dense or implicit) always take plain launches -- seven per LM iteration there, against milliseconds of work.  Otherwise the first
// solve with an iteration count after a hand-over uses plain launches and a repeat builds the graph (plain_runs: plain solves so far).
inline bool ba_solve_plain(const BaShape& s, const BaSwitches& sw, int iterations)
{
    return sw.no_graph || iterations == 0 || ba_pcg_is_cooperative(ba_pcg_form(s, sw, false));  // (the implicit form takes one problem)
}
inline bool ba_first_solve_plain(const BaSwitches& sw, int plain_runs) { return !sw.graph_first && plain_runs == 0; }

struct BaLmPlan
{
    BaLinForm lin       = BaLinForm::point_pass;
    BaCamForm cam       = BaCamForm::none;
    BaSchurForm schur   = BaSchurForm::none;
    BaPcgForm pcg       = BaPcgForm::none;
    BaUpdateForm update = BaUpdateForm::update_point;
    bool use_set    = false;  // the point-major kernels run (the whole batch decides, not the range of a chain: the hand-over left out the block entries on the same answer)
    bool zero_rows  = false;  // point_wave linearises: inactive observations have zero W rows (the implicit PCG's and schur_pass's flag)
    bool split_copy = false;  // accept_copy behind accept_pass
    bool no_block_lists = false;  // internal error: the block-major pass was chosen but the hand-over did not build its lists
    int n_chain = 1;
    int nsx = 0;   // work-item groups of the point-major kernels: four items per workgroup
    int nbx = 0;   // schur_pass<1>: a block per wavefront
    int nbs = 0;   // schur_sum: SUM_NB blocks per wavefront
    size_t pcg_lds = 0;
};

// Re-planning after a refused cooperative launch: the shape with persist_wgs = 0.
inline void ba_plan_pcg_stage(BaLmPlan& P, const BaShape& s, const BaSwitches& sw, bool recording)
{
    P.pcg = s.max_nfc > 0 ? ba_pcg_form(s, sw, recording, &P.pcg_lds) : BaPcgForm::none;
}

// The thresholds on the batch see B, the windows of one launch: the whole set, or the first chain's share of it (every chain of a
// split sequence has >= BA_GRAPH_CHAIN_MIN - 7 windows, beyond all of them).
inline BaLmPlan ba_lm_plan(const BaShape& s, const BaSwitches& sw, bool recording)
{
    BaLmPlan P;
    const bool large = ba_pcg_is_large(s.max_n6, s.max_nfc, s.implicit);
    P.n_chain        = ba_graph_chains(s.count, recording, large, sw.graph_chains);
    const int B      = P.n_chain == 1 ? s.count : ((int)((long long)s.count / P.n_chain) & ~7);
    P.use_set        = !s.implicit && ba_sets_will_run(s, sw);
    P.no_block_lists = !P.use_set && !s.blk_built && !s.implicit;
    P.zero_rows           = s.point_wave_ok && !sw.no_point_wave;
    P.nsx            = ba_ceil_div(ba_max(s.max_set_items, 1), 4);
    P.nbx            = ba_ceil_div(s.max_nfc * s.max_nfc, 4);
    P.nbs            = ba_ceil_div(s.max_nfc * s.max_nfc, 4 * SUM_NB);
    P.split_copy     = B <= BA_SPLIT_COPY_MAX_BATCH && s.max_np >= BA_SPLIT_COPY_MIN_POINTS;

    const bool k8    = s.set_k_max <= BA_FUSED3_MAX_K;
    const bool fused = P.use_set && !sw.no_schur_mfma && !sw.no_schur_fused && (k8 || sw.fused_k10);
    // the camera pass as per-item partial sums out of schur_fused<3, true> + cam_sum instead of cam_pass.  Built because cam_pass
    // linearises every observation a second time (294 us per 1024 windows); measured: schur_fused 1127 -> 1437 us for the five passes
    // through the contribution buffer, cam_sum 29 us -- 46 us SLOWER per LM iteration (profiles/r03/r03aa_*).  Kept selectable and
    // tested, not the default.
    const bool cam_sums = fused && k8 && s.cam_sums_ok && sw.cam_sums;
    if (fused) P.lin = cam_sums ? BaLinForm::fused3_sums : k8 ? BaLinForm::fused3 : BaLinForm::fused4;
    else P.lin = P.zero_rows ? BaLinForm::point_wave : BaLinForm::point_pass;

    if (P.use_set && !sw.no_update_cost) P.update = BaUpdateForm::update_cost;
    else P.update = P.zero_rows ? BaUpdateForm::update_wave : BaUpdateForm::update_point;

    if (s.max_nfc <= 0) return P;
    if (cam_sums) P.cam = BaCamForm::cam_sum;
    else if (B >= BA_CAM64_MIN_BATCH) P.cam = sw.cam_grid_2d ? BaCamForm::cam64_2d : BaCamForm::cam64_xcd;
    else P.cam = BaCamForm::cam256;

    if (s.implicit) P.schur = BaSchurForm::none;  // no S: the implicit PCG works from W, V^-1 and U
    else if (fused) P.schur = BaSchurForm::in_fused;
    else if (P.use_set)
    {
        const bool q2 = s.set_run_max * 9 + 3 <= 2 * 64;  // the rows of a point's run fit two register tiles
        if (!sw.no_schur_mfma) P.schur = !k8 ? BaSchurForm::mfma43 : q2 ? BaSchurForm::mfma32 : BaSchurForm::mfma33;
        else P.schur = s.set_small ? BaSchurForm::set42 : BaSchurForm::set63;
    }
    else
    {
        const long long nb = (long long)s.max_nfc * s.max_nfc;
        P.schur = B < BA_SCHUR_WIDE_BATCH_END && nb * B <= BA_SCHUR_WIDE_MAX_BLOCKS && !sw.no_schur_wide ? BaSchurForm::pass4 : BaSchurForm::pass1;
    }
    ba_plan_pcg_stage(P, s, sw, recording);
    return P;
}

// ---- ORB extractor (orb.hip: snk_orb_configure, run_part, run_pipeline; the geometry is orb_layout.hpp's) ----------------------------
// Every SNK_ORB_* switch.  orb.hip fills one per process (orb_switches()); SNK_DEBUG is read per call.
struct OrbSwitches
{
    bool balanced_strips  = false;  // BALANCED_STRIPS: the round-1..4 strip layout (equal strips of a multiple of 4 columns)
    int fast_surv_cap     = 0;      // FAST_SURV_CAP: quick-test survivors kept at a time, at least 128 (0: by the cell size; tests force the spill path)
    int parts             = 1;      // PARTS: launch chains per batch a handle starts with, 1..4
    int stagger           = 0;      // STAGGER: parts of the staggered schedule a handle starts with, 2..16 (0: off)
    bool blur_in_describe = false;  // BLUR_IN_DESCRIBE: experiment (round 5): no blurred plane, describe_kernel<true> blurs its patch
    bool blur_tiled       = false;  // BLUR_TILED: experiment (round 6): blurred planes tiled 32 x 4, see orb_blur_mode
    bool desc_no_dma      = false;  // DESC_NO_DMA: A/B: describe_kernel's register path instead of the patch by LDS-DMA
    bool desc_fake_on     = false;  // DESC_FAKE: timing experiments: describe_kernel leaves out a phase ...
    int desc_fake         = 0;      // ... this one (the variable's value)
    bool unfused          = false;  // UNFUSED: A/B: stand-alone resize_kernel + blur-only passes
    int level_bh          = 0;      // LEVEL_BH: A/B, tests: 64 / 22 / 8 rows per band of level_kernel (anything else: by the launch size)
    int fast_cpw          = 0;      // FAST_CPW: FAST cells per wavefront, 1..64 (anything else: by the launch size)
    int fast_stop         = 0;      // FAST_STOP: timing experiments: fast_kernel returns after a phase
    size_t fast_lds_wg    = 0;      // FAST_LDS_WG: experiment (round 4): fast_kernel asks for at least this much LDS per workgroup
    bool dist_timing      = false;  // DIST_TIMING (diagnostic): distribute_kernel's cycles per phase and level on stderr
    bool dist_key_loop    = false;  // DIST_KEY_LOOP: A/B: subdivision keys by the loop form, not from the tables
    bool harris_per_cell  = false;  // HARRIS_PER_CELL: A/B: harris_kernel, one wavefront per cell (round 5), instead of harris_dense_kernel
    bool one_stream       = false;  // ONE_STREAM: every batch as one launch chain, whatever the handle's schedule
};

// Layout of the blurred planes for this process (level_kernel writes it, describe_kernel reads it -- both ask here): 0 = row-major (the
// default), 2 = tiled 32 x 4 (SNK_ORB_BLUR_TILED=1, an experiment of round 6: built, bit-exact, MEASURED SLOWER -- describe_kernel
// 1.39 -> 1.32 ms, but level_kernel's stores, 16-byte pieces of 47 lines per row instead of two whole lines, cost 1.50 -> 1.74 ms:
// 191.6 -> 187.9 k frames/s, profiles/r06/r06p_ab_blur_tiled_negative.txt), 1 = no blurred plane (SNK_ORB_BLUR_IN_DESCRIBE=1).
inline int orb_blur_mode(const OrbSwitches& sw)
{
    return sw.blur_in_describe ? 1 : (sw.blur_tiled && !sw.desc_no_dma && !sw.desc_fake_on) ? 2 : 0;
}

constexpr int ORB_WAVE_SLOTS       = 8192;  // wavefront slots of the chip: 256 CUs x 32
constexpr int ORB_BAND_MIN_WAVES   = 2048;  // strips x bands of a level pass from which the next taller band is taken
constexpr int ORB_FAST_CPW_DEFAULT = 8;     // FAST cells per wavefront for big launches (measured in DESIGN.md section 5)
constexpr int ORB_FAST_MIN_ROUNDS  = 4;     // ... that still give every wavefront slot of the chip this many wavefronts
constexpr int ORB_XCD_MIN_BATCH    = 16;    // images from which a grid keeps an image's workgroups on one XCD (xcd_image_map)
constexpr int ORB_DIST_ONE_MAX_WGS = 128;   // (image, level) workgroups up to which each takes the full-budget carve at once
constexpr int ORB_DIST_LARGE_WGS   = 256;   // workgroups of the drain launch, at most
constexpr int ORB_HARRIS_NC        = 16;    // cells whose candidates harris_dense_kernel packs into a wavefront
constexpr int ORB_DESC_KPW         = 4;     // keypoints per wavefront of describe_kernel

// level_kernel<., BH>: rows per band
enum class OrbBandForm { bh64, bh22, bh8 };
// fast_kernel<NQ, LOOP>: one cell per wavefront | a loop over cpw cells; 0 / 3 / 4: tile pitches from the layout | of 3 / 4 quads
enum class OrbFastForm { single0, single3, single4, loop0, loop3, loop4 };
// Harris response ("orb.response" = 1): harris_kernel | harris_dense_kernel
enum class OrbHarrisForm { none, per_cell, dense };
// distribute_kernel at the full carve alone | at the small carve alone (level_cap <= 2048) | at the small carve, then distribute_large_kernel
enum class OrbDistForm { one_full, one_small, small_drain };
// describe_kernel<BLUR_IN, DMA, TILED>: <0,0,0> | <1,0,0> | <0,1,0> | <0,1,1>
enum class OrbDescForm { registers, blur_in, dma, dma_tiled };
// run_pipeline: one launch chain | `n` chains on as many streams | `n` parts, front halves on one stream and back halves on a second
enum class OrbSchedule { one_chain, chains, staggered };

inline const char* orb_name(OrbBandForm f)
{
    static const char* const n[] = {"bh64", "bh22", "bh8"};
    return n[(int)f];
}
inline const char* orb_name(OrbFastForm f)
{
    static const char* const n[] = {"single0", "single3", "single4", "loop0", "loop3", "loop4"};
    return n[(int)f];
}
inline const char* orb_name(OrbHarrisForm f)
{
    static const char* const n[] = {"none", "per_cell", "dense"};
    return n[(int)f];
}
inline const char* orb_name(OrbDistForm f)
{
    static const char* const n[] = {"one_full", "one_small", "small_drain"};
    return n[(int)f];
}
inline const char* orb_name(OrbDescForm f)
{
    static const char* const n[] = {"registers", "blur_in", "dma", "dma_tiled"};
    return n[(int)f];
}
inline const char* orb_name(OrbSchedule f)
{
    static const char* const n[] = {"one_chain", "chains", "staggered"};
    return n[(int)f];
}

// XCD-aware grids (orb.hip, xcd_image_map): from 16 images on, grid.x = 8 * gx and eight images share a grid row
inline void orb_xcd_grid(int gx, int batch, int& x, int& y)
{
    x = batch >= ORB_XCD_MIN_BATCH ? 8 * gx : gx;
    y = batch >= ORB_XCD_MIN_BATCH ? (batch + 7) / 8 : batch;
}

// Rows per band of a level pass: 64 when the launch fills the chip's 8192 wavefront slots anyway, else 22, else 8 (per-frame calls: a
// wavefront walks its band row by row behind a chain of load latencies).  bh_env: SNK_ORB_LEVEL_BH.
inline OrbBandForm orb_band_form(int n_strips, int h, int batch, int bh_env)
{
    if (bh_env == 64) return OrbBandForm::bh64;
    if (bh_env == 22) return OrbBandForm::bh22;
    if (bh_env == 8) return OrbBandForm::bh8;
    const long long strips = (long long)n_strips * batch;
    return strips * orb::cdiv(h, 64) >= ORB_BAND_MIN_WAVES ? OrbBandForm::bh64 : strips * orb::cdiv(h, 22) >= ORB_BAND_MIN_WAVES ? OrbBandForm::bh22 : OrbBandForm::bh8;
}
constexpr int orb_band_rows(OrbBandForm f) { return f == OrbBandForm::bh64 ? 64 : f == OrbBandForm::bh22 ? 22 : 8; }

// FAST cells per wavefront: 1 for small launches (keep the chip filled), more once there are plenty of workgroups -- at least four
// rounds of the chip's wavefront slots.  cpw_env: SNK_ORB_FAST_CPW, forced whatever the launch size (tests, measurements).
inline int orb_fast_cpw(int total_cells, int batch, int cpw_env)
{
    if (cpw_env >= 1 && cpw_env <= 64) return cpw_env;
    const long long cell_waves = (long long)total_cells * batch;
    int cpw = ORB_FAST_CPW_DEFAULT;
    while (cpw > 1 && cell_waves / cpw < (long long)ORB_WAVE_SLOTS * ORB_FAST_MIN_ROUNDS) cpw >>= 1;
    return cpw;
}
inline OrbFastForm orb_fast_form(int quads, bool loop)
{
    const int q = quads == 3 ? 1 : quads == 4 ? 2 : 0;
    return (OrbFastForm)((loop ? 3 : 0) + q);
}

// harris: "orb.response" = 1; per_cell: SNK_ORB_HARRIS_PER_CELL
inline OrbHarrisForm orb_harris_form(int total_cells, bool harris, bool per_cell)
{
    return !harris || total_cells <= 0 ? OrbHarrisForm::none : per_cell ? OrbHarrisForm::per_cell : OrbHarrisForm::dense;
}

// A launch of a few (image, level) workgroups (the per-frame calls) gives every workgroup the full-budget carve at once: nothing can
// be queued, the drain launch is skipped (one launch less in the per-frame chain; the carve only limits workgroups per CU, and these
// launches do not fill the chip).  Not under "orb.response" = 1: the Harris ranks do not fit beside the full carve.
inline OrbDistForm orb_dist_form(int n_levels, int batch, int level_cap, bool harris)
{
    if (orb::dist_small_cap(level_cap) >= level_cap) return OrbDistForm::one_small;
    return !harris && (long long)n_levels * batch <= ORB_DIST_ONE_MAX_WGS ? OrbDistForm::one_full : OrbDistForm::small_drain;
}

// round 6: the blurred patch by LDS-DMA (describe_kernel<false, true>; same-box A/B 1.457 -> 1.398 ms per 2048 images,
// profiles/r06/r06c_ab_describe_lds_dma.txt)
inline OrbDescForm orb_desc_form(const OrbSwitches& sw)
{
    if (sw.blur_in_describe) return OrbDescForm::blur_in;
    if (sw.desc_no_dma) return OrbDescForm::registers;
    return orb_blur_mode(sw) == 2 ? OrbDescForm::dma_tiled : OrbDescForm::dma;
}

// Launch chains of a batch: one by default.  Two half-batch chains on two streams (snk_orb_set_chains) overlap the tails of one chain's
// launches with the other's kernels: 186.0 / 192.1 / 192.9 / 188.4 k frames/s with 1 / 2 / 3 / 4 chains in one run, 187.6 k with 2 in
// the next (profiles/r05/r05o_chains.txt, r05p_bench_two_chains_by_default.txt) -- the chains start together and mostly run the same
// stage at the same time, so the gain is the tails only and a kernel's duration is then measured under a concurrent copy of itself.
// Tried as the default for big batches in round 5 and taken back.  Per-frame launches never split (and never create the extra streams).
// parts, stagger: the handle's (snk_orb_set_chains, snk_orb_set_stagger; SNK_ORB_PARTS, SNK_ORB_STAGGER at its creation).
// n: chains, or parts of the staggered schedule.
inline OrbSchedule orb_schedule(int batch, int parts, int stagger, int split_min_batch, bool one_stream, int& n)
{
    n = 1;
    const bool stag = stagger >= 2 && batch >= 2 * stagger;
    if (one_stream || batch < split_min_batch || !(parts > 1 || stag)) return OrbSchedule::one_chain;
    if (stag) return n = stagger, OrbSchedule::staggered;
    n = parts < batch ? parts : batch;
    return n > 1 ? OrbSchedule::chains : OrbSchedule::one_chain;
}

struct OrbLevelPlan
{
    bool skipped      = true;   // a level scaled down to nothing (small image, many levels): no pixels, no cells
    bool resize_first = false;  // stand-alone resize_kernel from level l - 1 (no in-stream down-scale there)
    bool tiny         = false;  // below 8 x 8: only down-scaled, never blurred (outside the domain of the streaming pass's reflect-101 halo)
    OrbBandForm band  = OrbBandForm::bh8;
    bool aligned      = true;   // level_kernel<true, .>; false: level 0 of an input whose base / pitch is not a multiple of 4
    int n_bands = 0, gx = 0;
    bool make_next    = false;  // the pass also writes level l + 1
};
struct OrbPlan
{
    int n_levels = 0, blur_mode = 0;
    OrbLevelPlan lv[orb::MAX_LEVELS];
    bool fast_run     = false;  // the layout has FAST cells
    OrbFastForm fast  = OrbFastForm::single0;
    int fast_cpw = 1, fast_quads = 0, fast_gx = 0;
    size_t fast_lds   = 0;
    OrbHarrisForm harris = OrbHarrisForm::none;
    int harris_gx     = 0;
    OrbDistForm dist  = OrbDistForm::one_small;
    int dist_lds_cap  = 0;      // candidates of a level the first launch's carve holds
    size_t dist_lds = 0, dist_large_lds = 0;
    int large_workers = 0;
    // the queue's counter: reset by fast_kernel when the call enqueues the whole chain on one stream (the usual case: one launch less
    // per frame); the split schedules (front and back halves on different streams, chain slots shared by parts) keep the fill
    bool queue_memset = true;
    OrbDescForm desc  = OrbDescForm::dma;
    int desc_gx = 0, desc_nb = 0, dfake = 0;
};

// A level in the plan line of run_part (SNK_DEBUG) and of tests/cpp/dispatch_driver.cpp: "-" skipped, else "r" (resize_kernel first) and
// "t" (tiny) or the rows per band, "u" (unaligned) and "+" (the pass also writes level l + 1) -- "64+", "r22u", "rt"
inline void orb_level_token(const OrbLevelPlan& p, char out[8])
{
    int n = 0;
    if (p.skipped) out[n++] = '-';
    else
    {
        if (p.resize_first) out[n++] = 'r';
        if (p.tiny) out[n++] = 't';
        else
        {
            const int bh = orb_band_rows(p.band);
            if (bh >= 10) out[n++] = (char)('0' + bh / 10);
            out[n++] = (char)('0' + bh % 10);
            if (!p.aligned) out[n++] = 'u';
            if (p.make_next) out[n++] = '+';
        }
    }
    out[n] = 0;
}

// One launch chain over `batch` images.  aligned0: base, pitch and stride of the caller's images are multiples of 4; harris:
// "orb.response" = 1; stages: 1 = the front half (pyramid / blur passes + FAST cells), 2 = the back half (distribution + descriptors),
// 3 = both.
inline OrbPlan orb_plan(const Layout& L, int batch, bool aligned0, bool harris, int stages, float scale_factor, const OrbSwitches& sw)
{
    OrbPlan P;
    P.n_levels  = L.n_levels;
    P.blur_mode = orb_blur_mode(sw);
    const bool fused_ok = scale_factor <= 2.0f && !sw.unfused;  // the in-stream down-scale reaches 3 * scale + 1 columns right
    const auto tiny     = [&](int l) { return L.lv[l].w < 8 || L.lv[l].h < 8; };
    for (int l = 0; l < L.n_levels; ++l)
    {
        const LevelInfo& lv = L.lv[l];
        OrbLevelPlan& p     = P.lv[l];
        if (lv.w <= 0 || lv.h <= 0) continue;
        p.skipped      = false;
        p.resize_first = l > 0 && (!fused_ok || tiny(l - 1));
        p.tiny         = tiny(l);
        if (p.tiny) continue;
        p.band      = orb_band_form(lv.n_strips, lv.h, batch, sw.level_bh);
        p.n_bands   = orb::cdiv(lv.h, orb_band_rows(p.band));
        p.gx        = orb::cdiv(lv.n_strips * p.n_bands, 4);
        p.aligned   = l > 0 || aligned0;
        p.make_next = fused_ok && l + 1 < L.n_levels && L.lv[l + 1].w > 0 && L.lv[l + 1].h > 0;
    }
    P.fast_run = L.total_cells > 0;
    if (P.fast_run)
    {
        P.fast_cpw   = orb_fast_cpw(L.total_cells, batch, sw.fast_cpw);
        P.fast_quads = orb::fast_quads(L);
        P.fast       = orb_fast_form(P.fast_quads, P.fast_cpw > 1);
        P.fast_gx    = orb::cdiv(L.total_cells, 4 * P.fast_cpw);
        // occupancy shaping (experiment, round 4): a workgroup that asks for at least SNK_ORB_FAST_LDS_WG bytes of LDS caps how many
        // FAST workgroups a CU holds, so that back-half workgroups of another stream (staggered schedule) find room beside them
        const size_t own = (size_t)4 * L.f_lds_wave, asked = sw.fast_lds_wg < (size_t)orb::LDS_BYTES ? sw.fast_lds_wg : (size_t)orb::LDS_BYTES;
        P.fast_lds       = own > asked ? own : asked;
    }
    P.harris = orb_harris_form(L.total_cells, harris, sw.harris_per_cell);
    if (P.harris == OrbHarrisForm::per_cell) P.harris_gx = orb::cdiv(L.total_cells, 4);
    if (P.harris == OrbHarrisForm::dense) P.harris_gx = orb::cdiv(orb::cdiv(L.total_cells, ORB_HARRIS_NC), 4);
    P.queue_memset = stages != 3 || !P.fast_run;
    P.dist         = orb_dist_form(L.n_levels, batch, L.level_cap, harris);
    const int small_cap = orb::dist_small_cap(L.level_cap);
    P.dist_lds_cap   = P.dist == OrbDistForm::one_full ? L.level_cap : small_cap;
    P.dist_lds       = P.dist == OrbDistForm::one_full ? orb::dist_lds_bytes((size_t)L.level_cap)
                                                       : orb::dist_lds_bytes((size_t)small_cap) + (harris ? orb::dist_harris_bytes((size_t)small_cap) : 0);
    P.dist_large_lds = orb::dist_lds_bytes((size_t)L.level_cap);
    P.large_workers  = L.n_levels * batch < ORB_DIST_LARGE_WGS ? L.n_levels * batch : ORB_DIST_LARGE_WGS;
    int max_slot = 1;
    for (int l = 0; l < L.n_levels; ++l) max_slot = L.lv[l].slot_cap > max_slot ? L.lv[l].slot_cap : max_slot;
    P.desc    = orb_desc_form(sw);
    P.desc_gx = orb::cdiv(max_slot, 4 * ORB_DESC_KPW);
    P.desc_nb = batch >= ORB_XCD_MIN_BATCH ? 8 * orb::cdiv(batch, 8) : batch;
    P.dfake   = sw.desc_fake;
    return P;
}

// ---- projection matchers (track.hip: snk_match_project_coarse_batch_dev, fine_batch_impl and the host entries) -----------------------
struct TrackSwitches
{
    bool no_frame_lds     = false;  // SNK_TRACK_NO_FRAME_LDS: A/B: the batched matchers with global-memory gathers
    int frame_wgs         = 0;      // SNK_TRACK_FRAME_WGS: A/B, tests: workgroups per frame of the frame-resident matchers (0: by the batch)
    bool no_fused_resolve = false;  // SNK_TRACK_NO_FUSED_RESOLVE: A/B, tests: always the separate resolution
    int ppw               = 0;      // SNK_TRACK_PPW: tests: points per wavefront, 1..64 (anything else: by the number of points)
};

constexpr int TRACK_FRAME_LDS_MAX = 144 * 1024;  // LDS carve of the frame-resident matchers (one workgroup per CU above 80 KB)
constexpr int TRACK_CHUNK_POINTS  = 1024;        // points of the local map a workgroup of the frame-resident matchers takes at a time
constexpr int TRACK_PPW_POINTS    = 8192;        // points of a call per point of a wavefront

// LDS of a frame of `cap` features over a grid of ncell1 - 1 cells: keypoints (24 B), descriptors (32 B), right points, taken flags, cell starts
constexpr size_t track_frame_lds(int cap, int ncell1)
{
    return (((size_t)cap * 24 + 15) & ~(size_t)15) + (size_t)cap * 32 + (((size_t)cap * 4 + 15) & ~(size_t)15) + (((size_t)cap + 15) & ~(size_t)15) +
           (size_t)ncell1 * 4 + 64;
}

// Points per wavefront of the projection matchers: a wavefront does the per-point geometry for `ppw` points at once and, with
// PJ_GROUP = 1, every lane then scans its own point's window.  Many points per wavefront fill the lanes (throughput of the
// batched forms), few spread a single frame's points over the chip: for the host calls (one frame, the reference's call
// pattern) ONE point per wavefront is the lowest latency -- measured on MI355X with the frame bound (tools/latency_track.py,
// profiles/r03/r03b_latency_track.log): SearchByProjectionFrameFrame2 with 1500 points 0.089 / 0.097 / 0.104 / 0.113 ms and
// SearchByProjection2 with 10 000 points 0.785 / 0.797 / 0.800 / 0.907 ms at 1 / 4 / 16 / 64 points per wavefront -- a lane's
// serial window scan is the critical path either way, and more wavefronts only add parallel scans.
inline int track_points_per_wave(long long total_points, int ppw_env)
{
    if (ppw_env >= 1 && ppw_env <= 64) return ppw_env;
    const long long want = total_points / TRACK_PPW_POINTS;
    return (int)(want < 1 ? 1 : (want > 64 ? 64 : want));
}

// Workgroups per frame of the frame-resident matchers: every workgroup stages the frame in LDS once and then walks its share of the
// local map's 1024-point chunks, so as few as keep the chip's 512 workgroup slots (two 65 KB frames per CU) filled about twice.
// Measured on the tracking leg of bench.py (1024 frames x 10 000 points, profiles/r04/r04g_track_wgs.log): 10 workgroups per frame
// (one per chunk, the round-3 form) 537 k frames/s, 5: 582 k, 3: 595 k, 2: 610 k, 1: 611 k.  forced: SNK_TRACK_FRAME_WGS.
inline int track_frame_wgs(int chunks, int batch, int forced)
{
    int wgs = batch > 0 ? (1024 + batch - 1) / batch : chunks;
    if (forced >= 1) wgs = forced;
    return wgs < 1 ? 1 : (wgs > chunks ? chunks : wgs);
}

// Byte offset of the claims inside the LDS carve of a frame-resident matcher that resolves its matches itself, -1 = separate resolution
// (several workgroups per frame, or the claims do not fit behind the frame).  off: SNK_TRACK_NO_FUSED_RESOLVE.
inline int track_fused_claim_offset(int wgs, size_t flds, int cap, bool off)
{
    const size_t at = (flds + 15) & ~(size_t)15;
    return (off || wgs != 1 || at + (size_t)cap * 4 > (size_t)TRACK_FRAME_LDS_MAX) ? -1 : (int)at;
}

// A batched projection matcher over `batch` frames of `cap` features (a grid of ncell1 - 1 cells) and pts_cap points each
// frame: coarse_frame_kernel / fine_frame_kernel, the frame in LDS;  batch: coarse_batch_kernel / fine_batch_kernel, global-memory gathers
enum class TrackForm { frame, batch };
inline const char* track_name(TrackForm f) { return f == TrackForm::frame ? "frame" : "batch"; }

struct TrackBatchPlan
{
    TrackForm form = TrackForm::batch;
    int ppw        = 1;
    int wgs        = 0;   // frame: workgroups per frame
    int claim_off  = -1;  // frame: >= 0: the kernel resolves its matches itself
    size_t lds     = 0;   // frame: the frame, and the claims behind it
};
inline TrackBatchPlan track_batch_plan(int pts_cap, int batch, int cap, int ncell1, const TrackSwitches& sw)
{
    TrackBatchPlan P;
    P.ppw             = track_points_per_wave((long long)pts_cap * batch, sw.ppw);
    const size_t flds = track_frame_lds(cap, ncell1);
    if (P.ppw != 64 || flds > (size_t)TRACK_FRAME_LDS_MAX || sw.no_frame_lds) return P;
    P.form      = TrackForm::frame;
    P.wgs       = track_frame_wgs((pts_cap + TRACK_CHUNK_POINTS - 1) / TRACK_CHUNK_POINTS, batch, sw.frame_wgs);
    P.claim_off = track_fused_claim_offset(P.wgs, flds, cap, sw.no_fused_resolve);
    P.lds       = P.claim_off >= 0 ? (size_t)P.claim_off + (size_t)cap * 4 : flds;
    return P;
}

// The separate resolution (resolve_batch_kernel) keeps the claims of a frame's features in LDS up to this capacity (128 KB of ints,
// 1024 threads per frame) and in global memory beyond it.
constexpr int TRACK_RESOLVE_LDS_FEATURES = 32768;
inline bool track_resolve_in_lds(int cap) { return cap <= TRACK_RESOLVE_LDS_FEATURES; }

// Where a batched matcher's claims are resolved: fused = in the frame kernel itself; lds / global: resolve_batch_kernel<true / false>
enum class TrackResolve { fused, lds, global };
inline const char* track_name(TrackResolve r) { return r == TrackResolve::fused ? "fused" : (r == TrackResolve::lds ? "lds" : "global"); }
inline TrackResolve track_resolve_form(const TrackBatchPlan& P, int cap)
{
    if (P.form == TrackForm::frame && P.claim_off >= 0) return TrackResolve::fused;
    return track_resolve_in_lds(cap) ? TrackResolve::lds : TrackResolve::global;
}

// ---- feature grid (track.hip: snk_feature_grid, snk_feature_grid_batch_dev) -----------------------------------------------------------
constexpr int GRID_MAX_FEATURES  = 16384;      // features of a frame: the bitonic network sorts (cell << 16 | index) keys in 64 KB of LDS
constexpr int GRID_COUNT_LDS_MAX = 96 * 1024;  // LDS carve of the counting form

// LDS of grid_count_kernel: counts / starts and the fill cursors of ncell + 1 cells, the cell and the segment slot of n features
constexpr size_t grid_count_lds(int n, int ncell) { return ((size_t)2 * ((size_t)ncell + 1) + (size_t)2 * (size_t)n) * 4; }

// count: grid_count_kernel (histogram, scan, rank inside the cell: five barriers);  network: grid_kernel (bitonic sort), where the
// counting form's LDS does not fit.  network_env: SNK_GRID_NETWORK (A/B, tests: the network also where the counting form fits)
enum class GridForm { count, network };
inline const char* grid_name(GridForm f) { return f == GridForm::count ? "count" : "network"; }
inline GridForm grid_form(int cap, int ncell, bool network_env)
{
    return (grid_count_lds(cap, ncell) <= (size_t)GRID_COUNT_LDS_MAX && !network_env) ? GridForm::count : GridForm::network;
}
}  // namespace snk
