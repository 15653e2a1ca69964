// "snk-lmap v1": the per-item statements of the fine-tracking local map -- the rest of Tracking::UpdateLocalKeyFrames2 (reference
// Snake/Tracking/TrackingFine.cpp:272-323) and Tracking::UpdateLocalPoints with LocalMap::addPoint (:328-356, Snake/Map/LocalMap.h:139-154)
// -- as functions of plain values, so that the kernels (localmap.hip) and a CPU build (tests/cpp/lmap_core_driver.cpp, a debugger) run the
// same statements.  DESIGN.md section 3j.
//
//   draw        [DEFINED] Saiga::Random is absent.  key = mix(mix(seed lo ^ golden) ^ seed hi) ^ frame_id; draw number c is
//               h = mix(mix(key) ^ c).  Integers only, every draw a function of its position.
//   accept      "sampleDouble(0, 1) < k / double(n)" [DEFINED] as (u64)h * n < (u64)k << 32: n <= k always accepts (prob >= 1 and the inf
//               of an empty list, which the reference never evaluates), k = 0 never does                                  :280-285, :316-319
//   vote        UNCHANGED (or an empty list): EMPTY (:254).  n_found > n_conn: TRUNCATED.  Any other status or a count outside its
//               range: BAD_INDEX
//   neighbour   appended iff not bad (:304) and not marked (:306)
//   skip        a keyframe's feature: point -1, bad, or lastFrameSeen == frame id (:338-339).  An own point: -1 or bad (:346)
//   hash        slot = mix(id ^ golden) & (slots - 1); linear probing
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SNK_LMAP_HD __host__ __device__ __forceinline__
#else
#define SNK_LMAP_HD inline
#endif

namespace snk
{
constexpr int LMAP_MAX_LOCAL_KF   = 256;    // local keyframes per set: the prefix sum of their feature ranges is one pass of a workgroup
constexpr int LMAP_MAX_PTS        = 16384;  // local-map points per set (the reference reserves 10 000): 32 768 four-byte slots in LDS
constexpr int LMAP_MAX_NEIGHBOURS = 16;     // [DEFINED] n_neighbours at most: kf_cap * n_neighbours candidates are sorted in LDS
constexpr int LMAP_MAX_ORDER      = 1 << 30;  // [DEFINED] candidates of a set (features of its local keyframes + own points) at most
enum { LMAP_OK = 0, LMAP_EMPTY = 1, LMAP_TRUNCATED = 2, LMAP_KF_OVERFLOW = 3, LMAP_PTS_OVERFLOW = 4, LMAP_BAD_INDEX = 5 };
enum { LMAP_PT_BAD = 1 };                       // SNK_COVIS_PT_BAD
enum { LMAP_VOTE_OK = 0, LMAP_VOTE_UNCHANGED = 1 };  // SNK_COVIS_OK, SNK_COVIS_UNCHANGED

SNK_LMAP_HD uint32_t lmap_mix(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

SNK_LMAP_HD uint32_t lmap_key(uint64_t seed, int32_t frame_id)
{
    const uint32_t h = lmap_mix((uint32_t)seed ^ 0x9e3779b9u);
    return lmap_mix(h ^ (uint32_t)(seed >> 32)) ^ (uint32_t)frame_id;
}

SNK_LMAP_HD uint32_t lmap_draw(uint32_t key, uint32_t c) { return lmap_mix(lmap_mix(key) ^ c); }

// Random::sampleDouble(0, 1) < k / double(n)
SNK_LMAP_HD bool lmap_accept(uint32_t h, int k, int n) { return (uint64_t)h * (uint64_t)(uint32_t)n < ((uint64_t)(uint32_t)k << 32); }

SNK_LMAP_HD uint32_t lmap_hash(int32_t id) { return lmap_mix((uint32_t)id ^ 0x9e3779b9u); }

// what the vote's record says about the set: LMAP_OK = walk the list of n_found entries
SNK_LMAP_HD int lmap_vote_status(int status, int n_found, int n_conn, int vote_cap)
{
    if (status == LMAP_VOTE_UNCHANGED) return LMAP_EMPTY;
    if (status != LMAP_VOTE_OK || n_found < 0 || n_conn < 0 || n_conn > vote_cap || n_conn > n_found) return LMAP_BAD_INDEX;
    if (n_found > n_conn) return LMAP_TRUNCATED;
    return n_found == 0 ? LMAP_EMPTY : LMAP_OK;
}

// TrackingFine.cpp:304-306
SNK_LMAP_HD bool lmap_neighbour_listed(unsigned kf_bad, bool marked) { return kf_bad == 0 && !marked; }
// :338-339, p >= -1
SNK_LMAP_HD bool lmap_kf_point_skipped(int p, unsigned flags, int last_seen, int frame_id)
{
    return p < 0 || (flags & LMAP_PT_BAD) != 0 || last_seen == frame_id;
}
// :346
SNK_LMAP_HD bool lmap_own_point_skipped(int p, unsigned flags) { return p < 0 || (flags & LMAP_PT_BAD) != 0; }

struct LmapSelectResult
{
    int32_t n_local, n_direct, n_indirect, reference_kf, status;
};
struct LmapGatherResult
{
    int32_t n_pts, n_searchable, n_own_new, status;
};
SNK_LMAP_HD LmapSelectResult lmap_no_list(int status) { return LmapSelectResult{0, 0, 0, -1, status}; }
SNK_LMAP_HD LmapGatherResult lmap_no_points(int status) { return LmapGatherResult{0, 0, 0, status}; }
}  // namespace snk
