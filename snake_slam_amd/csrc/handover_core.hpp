// The statements the host builder of the BA hand-over (fill_problem / size_pass in ba_handover.hip) and the device stage behind
// snk_ba_set_problems_dev (ho_count_kernel / ho_fill_kernel there) share, as functions of plain values, and the plan of that device stage:
// which problems its kernels take and the LDS carve they ask for.  Free of HIP includes: tests/cpp/handover_core_driver.cpp builds it with
// plain g++ and walks a problem the way the kernels do.  DESIGN.md section 4.
//
//   valid       an observation counts iff image and point index are in range and image and point are not both constant
//               (reference LocalBundleAdjustment.cpp:286)
//   free camera index of image i = the number of images before it that are not constant, -1 for a constant image
//   order       stable counting sort by point: caller order inside a point
//   dup         a free camera appears twice on one point (looked at only up to HO_DUP_MAX_CAMS free cameras: the device builder of the
//               camera-pair block entries, which is what the flag switches off, takes no more)
//   k > 8       a point has more than eight observations by free cameras (in-range indices; work items of up to 128 points are then off)
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SNK_HO_HD __host__ __device__ inline __attribute__((always_inline))  // (dispatch.hpp is read before the HIP headers in places)
#else
#define SNK_HO_HD inline
#endif

namespace snk
{
// ---- the plan -----------------------------------------------------------------------------------------------------------------------
// One workgroup of HO_THREADS lanes per problem, twice: ho_count_kernel (values, free-camera indices, the histogram by point and its
// prefix sums) and, once the host has placed every problem's observations, ho_fill_kernel (the sorted observation arrays, dup).
// Both keep a word (the count kernel two) per point in LDS, so a batch is taken iff every problem has at most HO_MAX_PTS points; and iff
// no point of it holds more than HO_MAX_RUN valid observations, which the count kernel reports: the dup rule walks a point's run per
// observation.  Any other batch is staged through the host builder as a whole.  HO_MAX_PTS is half of snk-scene v1's pt_cap limit: two
// workgroups of the count kernel per compute unit at the limit (64 KiB each), and windows above it exist to be staged.
constexpr int HO_THREADS      = 256;   // a chunk of the fill kernel: one observation per lane, in caller order
constexpr int HO_MAX_PTS      = 8192;  // points of a problem the kernels take
constexpr int HO_MAX_RUN      = 1024;  // valid observations of one point the kernels take
constexpr int HO_MISC         = 16;    // u32 words: the two banks of block_scan's partial sums (8), the flags
constexpr int HO_DUP_MAX_CAMS = 512;   // BE_MAX_CAMS of ba_handover.hip
constexpr int HO_BIG_MAX_FREE = 8;     // free observations of a point the work items of up to 128 points allow

constexpr size_t ho_count_carve(int n_pt) { return (size_t)HO_MISC * 4 + (size_t)n_pt * 8; }                        // valid and free counts per point
constexpr size_t ho_fill_carve(int n_pt) { return (size_t)HO_MISC * 4 + (size_t)HO_THREADS * 4 + (size_t)n_pt * 4; }  // a chunk's keys, a cursor per point
constexpr size_t ho_carve_max() { return ho_count_carve(HO_MAX_PTS) > ho_fill_carve(HO_MAX_PTS) ? ho_count_carve(HO_MAX_PTS) : ho_fill_carve(HO_MAX_PTS); }
constexpr bool ho_kernels_take(int n_pt) { return n_pt <= HO_MAX_PTS; }
constexpr bool ho_run_taken(int run) { return run <= HO_MAX_RUN; }

// What the host tells the kernels about problem b (row b of the caller's arrays) and what they answer
struct HoPlace
{
    int32_t n_img, n_pt, n_obs;
    int32_t img_at, pt_at, ps_at, orig_at;  // the problem's place in the shared lists (PreProb::*_at)
    int32_t obs_at;                         // known after the count kernel: ho_fill_kernel reads it
};
struct HoOut
{
    int32_t nfc, no;            // free cameras, valid observations           (ho_count_kernel)
    int32_t k_over8, long_run;  // the rules above; a point with more than HO_MAX_RUN valid observations
    int32_t dup;                // (ho_fill_kernel)
};

// ---- the rules ----------------------------------------------------------------------------------------------------------------------
SNK_HO_HD bool ho_in_range(int i, int p, int n_img, int n_pt) { return i >= 0 && i < n_img && p >= 0 && p < n_pt; }
SNK_HO_HD bool ho_obs_valid(int i, int p, int n_img, int n_pt, const uint8_t* img_const, const uint8_t* pt_const)
{
    return ho_in_range(i, p, n_img, n_pt) && !(img_const[i] && pt_const[p]);
}
// the observations the k > 8 rule counts
SNK_HO_HD bool ho_obs_by_free_camera(int i, int p, int n_img, int n_pt, const uint8_t* img_const)
{
    return ho_in_range(i, p, n_img, n_pt) && !img_const[i];
}
SNK_HO_HD int ho_cam_index(bool is_const, int free_before) { return is_const ? -1 : free_before; }
SNK_HO_HD bool ho_k_over8(int free_obs_of_point) { return free_obs_of_point > HO_BIG_MAX_FREE; }
// 64-bit words of "cameras seen" per point the host keeps; 0: the dup rule is off
SNK_HO_HD int ho_dup_words(int nfc) { return nfc <= HO_DUP_MAX_CAMS ? (nfc + 63) >> 6 : 0; }
// the same rule on the sorted observations: the camera of observation s stands earlier in its point's run [run_begin, s)
SNK_HO_HD bool ho_cam_seen_before(const int* o_cam, int run_begin, int s)
{
    const int c = o_cam[s];
    if (c < 0) return false;
    for (int j = run_begin; j < s; ++j)
        if (o_cam[j] == c) return true;
    return false;
}

// The order inside a chunk of the fill kernel.  keys[t] = the point of the chunk's t-th observation, -1 for one that is not valid;
// n4 * 4 keys, read four at a time.  before = the observations of the same point in front of t, total = all of them in the chunk: the
// observation goes to cursor[point] + before, and the one with before + 1 == total advances the cursor by total.
struct alignas(16) HoKey4
{
    int32_t x, y, z, w;
};
SNK_HO_HD void ho_chunk_rank(const int32_t* keys, int n4, int t, int& before, int& total)
{
    const int32_t key = keys[t];
    const HoKey4* k4  = reinterpret_cast<const HoKey4*>(keys);
    before = 0, total = 0;
    for (int q = 0; q < n4; ++q)
    {
        const HoKey4 k = k4[q];
        const int j    = 4 * q;
        const int e0 = k.x == key, e1 = k.y == key, e2 = k.z == key, e3 = k.w == key;
        total += e0 + e1 + e2 + e3;
        before += (j < t ? e0 : 0) + (j + 1 < t ? e1 : 0) + (j + 2 < t ? e2 : 0) + (j + 3 < t ? e3 : 0);
    }
}
}  // namespace snk
