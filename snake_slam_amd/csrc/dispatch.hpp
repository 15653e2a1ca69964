// Which kernel form a launch shape selects: the ONE place where the thresholds of matcher.hip and pose.hip live.  Host-only and free
// of HIP includes, so that tests/cpp/dispatch_driver.cpp builds it with plain g++ and tests/forms.py can pin every shape of the GPU
// tests to the form it was written for.  launch_knn2, snk_stereo_match, stereo_match_batch_dev_impl, snk_pose_refine and
// refine_batch_impl call these functions and keep no copy of the conditions; the environment switches are read there and passed in.
#pragma once
#include <cstddef>

#ifndef SNK_POSE_RED_STEPS  // DPP steps of pose_kernel's 27 sums before they meet in LDS: 4 = rows of 16 lanes, 2 = quads (pose.hip)
#define SNK_POSE_RED_STEPS 2
#endif

namespace snk
{
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
}  // namespace snk
