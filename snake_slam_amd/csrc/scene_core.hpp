// "snk-scene v1": the per-item statements of LocalBundleAdjustment::MakeLocalScene (reference Snake/Optimizer/LocalBundleAdjustment.cpp:94-346)
// as functions of plain values, so that the kernels (scene.hip) and a CPU build (tests/cpp/scene_core_driver.cpp, a debugger) run the same
// statements.  DESIGN.md section 3k.
//
//   candidates  the last min(n_neighbours, size) connections, the query, then previousKF at most n_last times (:124-135); a bad keyframe
//               of the chain counts as a step and is walked through
//   window      a candidate survives iff it is not bad (:145) and no earlier candidate is the same keyframe (:142); ascending slot (:151)
//   point       skipped iff -1 or bad (:158)
//   record      skipped iff its keyframe is bad (:261) or image and point are both constant (:286)
//   constraint  emitted iff time[a] == imu_begin[b], time[b] == imu_end[b] (:304) and preint_valid[b] (:309); dt = time[b] - time[a],
//               weight_rotation = gyro / dt, weight_translation = (w * acc) / dt, both 0 when dt > 2 (:331-339): IEEE fp64, in that order
#pragma once
#include <cstdint>

#include "lmap_core.hpp"

namespace snk
{
constexpr int SCENE_MAX_WINDOW = 64;       // n_neighbours + 1 + n_last at most: the candidates are one wavefront
constexpr int SCENE_MAX_IMG    = 4096;     // [DEFINED] img_cap at most: 8 192 two-word slots, 4 096 sort keys and 4 096 bases in LDS
constexpr int SCENE_MAX_OBS    = 1 << 22;  // [DEFINED] obs_cap at most
constexpr int SCENE_MAX_WALK   = 1 << 30;  // [DEFINED] observations of a set's points (the walk's ordinals) at most
enum { SCENE_OK = 0, SCENE_SKIPPED = 1, SCENE_WINDOW_OVERFLOW = 2, SCENE_PTS_OVERFLOW = 3, SCENE_IMG_OVERFLOW = 4, SCENE_OBS_OVERFLOW = 5, SCENE_BAD_INDEX = 6 };
enum { SCENE_PT_BAD = 1, SCENE_PT_CONST = 4 };  // SNK_COVIS_PT_BAD, SNK_SCENE_PT_CONST

struct SceneWindowResult
{
    int32_t n_window, status;
};
struct SceneResult
{
    int32_t n_window, n_img, n_pt, n_obs, n_rpc, status;
};
SNK_LMAP_HD SceneWindowResult scene_no_window(int status) { return SceneWindowResult{0, status}; }
SNK_LMAP_HD SceneResult scene_no_scene(int status) { return SceneResult{0, 0, 0, 0, 0, status}; }

// candidates of a query with `size` connections whose chain has `chain` keyframes (already cut at n_last)
SNK_LMAP_HD int scene_n_neighbours_taken(int n_neighbours, int size) { return n_neighbours < size ? n_neighbours : size; }
// :142-145, `earlier` = an earlier candidate is the same keyframe
SNK_LMAP_HD bool scene_candidate_survives(unsigned kf_bad, bool earlier) { return kf_bad == 0 && !earlier; }
// :158, p >= -1
SNK_LMAP_HD bool scene_point_skipped(int p, unsigned flags) { return p < 0 || (flags & SCENE_PT_BAD) != 0; }
SNK_LMAP_HD bool scene_point_constant(unsigned flags) { return (flags & SCENE_PT_CONST) != 0; }
// :261, :286
SNK_LMAP_HD bool scene_record_skipped(unsigned kf_bad, bool img_const, bool pt_const) { return kf_bad != 0 || (img_const && pt_const); }
// what stage 2 makes of a stage-1 record: SCENE_OK = build the scene of n_window keyframes
SNK_LMAP_HD int scene_window_status(int status, int n_window, int win_cap)
{
    if (status == SCENE_SKIPPED || status == SCENE_WINDOW_OVERFLOW || status == SCENE_BAD_INDEX) return status;
    if (status != SCENE_OK || n_window < 0 || n_window > win_cap || n_window > SCENE_MAX_WINDOW) return SCENE_BAD_INDEX;
    return SCENE_OK;
}
// :304, :309
SNK_LMAP_HD bool scene_rpc_emitted(double time_a, double time_b, double imu_begin_b, double imu_end_b, unsigned preint_valid_b)
{
    return time_a == imu_begin_b && time_b == imu_end_b && preint_valid_b != 0;
}
// :331-339.  Two divisions and one product, each rounded once
SNK_LMAP_HD void scene_rpc_weights(double time_a, double time_b, double gyro_weight, double acc_weight, double weight_translation_in, double& weight_rotation,
                                   double& weight_translation)
{
    const double dt    = time_b - time_a;
    const double prod  = weight_translation_in * acc_weight;
    weight_rotation    = gyro_weight / dt;
    weight_translation = prod / dt;
    if (dt > 2)
    {
        weight_rotation    = 0;
        weight_translation = 0;
    }
}
}  // namespace snk
