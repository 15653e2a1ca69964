// "snk-covis v1": the covisibility list of ONE set -- Keyframe::UpdateConnections (reference Snake/Map/Keyframe.cpp:89-171) for a query
// keyframe, the vote at the head of Tracking::UpdateLocalKeyFrames2 (reference Snake/Tracking/TrackingFine.cpp:230-268) for a frame's
// matched points -- as functions of plain values, so that the kernel (covis.hip) and a CPU build (tests/cpp/covis_core_driver.cpp, a
// debugger) run the same statements.  DESIGN.md section 3i.
//
//   gate        a feature counts iff its point id is >= 0, bit 0 of the point's flags (bad) is clear and, in the connection form only,
//               bit 1 (far stereo point) is clear and depth <= th_depth (equality counts, a depth <= 0 counts)      Keyframe.cpp:105-115
//   count       count[k] += 1 for every observation (k, .) of a counting feature's point, k != q in the connection form; duplicates count
//               as often as they occur; bad keyframes are counted                                                    :117-121, :241-251
//   list        connection form: the touched keyframes that are not bad with count >= th; if none, the one with the largest count,
//               [DEFINED] the smallest id among equals.  vote form: every touched keyframe                           :139-158, :259-264
//   order       [DEFINED] ascending by the key count << 32 | id (KeyframeGraph.cpp:124 sorts the full pair, the id stands for the pointer)
//   cut         n_found > cap: the last cap entries of that order, i.e. the keys >= the cap-th largest key
#pragma once
#include <algorithm>
#include <cstdint>

#if defined(__HIPCC__)
#define SNK_COVIS_HD __host__ __device__ __forceinline__
#else
#define SNK_COVIS_HD inline
#endif

namespace snk
{
constexpr int COVIS_MAX_KF  = 32768;  // a u32 counter per keyframe: 128 KiB of a compute unit's 160 KiB LDS
constexpr int COVIS_MAX_CAP = 4096;   // list entries kept per set: 16 KiB of ids to sort beside the counters
enum { COVIS_OK = 0, COVIS_UNCHANGED = 1, COVIS_BAD_INDEX = 2 };
enum { COVIS_PT_BAD = 1, COVIS_PT_FAR = 2 };

// does a feature with a point (id >= 0) count?  Keyframe.cpp:107,111 / TrackingFine.cpp:235
template <bool GATE>
SNK_COVIS_HD bool covis_gate(unsigned flags, float depth, float th_depth)
{
    if (flags & COVIS_PT_BAD) return false;
    if (GATE && (depth > th_depth || (flags & COVIS_PT_FAR))) return false;
    return true;
}

// does an observation by keyframe k count for query q?  Keyframe.cpp:119
template <bool SELF_EXCLUDED>
SNK_COVIS_HD bool covis_counts(int k, int q)
{
    return !(SELF_EXCLUDED && k == q);
}

// may a touched keyframe be listed?  Keyframe.cpp:141
template <bool BAD_FILTER>
SNK_COVIS_HD bool covis_listable(unsigned kf_bad)
{
    return !(BAD_FILTER && kf_bad != 0);
}

// the count from which a listable keyframe is listed: th of Keyframe.cpp:147, or every touched one
template <bool THRESHOLD>
SNK_COVIS_HD uint32_t covis_min_count(int th)
{
    return THRESHOLD ? (uint32_t)th : 1u;
}

// the order of the list: ascending in this key, no two entries equal
SNK_COVIS_HD uint64_t covis_key(uint32_t weight, uint32_t id) { return (uint64_t)weight << 32 | id; }
// the fallback of Keyframe.cpp:154-158: the largest of these keys is the largest count and, among equals, the smallest id
SNK_COVIS_HD uint64_t covis_max_key(uint32_t weight, uint32_t id) { return (uint64_t)weight << 32 | (0xFFFFFFFFu - id); }
SNK_COVIS_HD uint32_t covis_max_key_id(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)key; }

SNK_COVIS_HD int covis_bits(uint32_t v)
{
    int n = 0;
    while (v) n += 1, v >>= 1;
    return n;
}

// The keep-th largest key of a list of distinct keys without sorting it: the largest T with #{key >= T} >= keep, built bit by bit from
// the top.  count_ge(T) counts the list; max_weight bounds the weights and the ids are < n_kf, so only the bits a key can have are
// tried: bits(max_weight) + bits(n_kf - 1) counting passes.  Requires 1 <= keep <= length of the list.
template <typename CountGE>
SNK_COVIS_HD uint64_t covis_cut(CountGE count_ge, int keep, uint32_t max_weight, int n_kf)
{
    uint64_t T = 0;
    for (int bit = 32 + covis_bits(max_weight) - 1; bit >= 32; --bit)
    {
        const uint64_t cand = T | (1ull << bit);
        if (count_ge(cand) >= keep) T = cand;
    }
    for (int bit = covis_bits((uint32_t)(n_kf - 1)) - 1; bit >= 0; --bit)
    {
        const uint64_t cand = T | (1ull << bit);
        if (count_ge(cand) >= keep) T = cand;
    }
    return T;
}

struct CovisConn
{
    int32_t weight, kf;
};
struct CovisResult
{
    int32_t n_found, n_conn, best_kf, status;
};

SNK_COVIS_HD CovisResult covis_no_list(int status) { return CovisResult{0, 0, -1, status}; }

// ---- the whole set on one thread: what the kernel computes, spelled as loops (host builds only use this) ---------------------------
// count: n_kf zeroed counters, left dirty; conn: room for min(cap, n_kf) entries.  Returns the result and writes conn[0 .. n_conn).  The caller has checked every index.
template <bool GATE, bool SELF_EXCLUDED, bool BAD_FILTER, bool THRESHOLD>
inline CovisResult covis_set(int n_kf, const uint8_t* kf_bad, const int32_t* obs_start, const int32_t (*obs)[2], const uint8_t* pt_flags,
                             int first, int last, const int32_t* item_point, const float* item_depth, int q, int th, float th_depth, int cap,
                             uint32_t* count, CovisConn* conn)
{
    for (int i = first; i < last; ++i)
    {
        const int p = item_point[i];
        if (p < 0) continue;
        if (!covis_gate<GATE>(pt_flags[p], GATE ? item_depth[i] : 0.0f, th_depth)) continue;
        for (int o = obs_start[p]; o < obs_start[p + 1]; ++o)
            if (covis_counts<SELF_EXCLUDED>(obs[o][0], q)) count[obs[o][0]] += 1;
    }
    const uint32_t min_count = covis_min_count<THRESHOLD>(th);
    int touched = 0, n_found = 0;
    uint64_t max_key = 0;
    for (int k = 0; k < n_kf; ++k)
    {
        const uint32_t c = count[k];
        if (c == 0) continue;
        touched += 1;
        const bool listable = covis_listable<BAD_FILTER>(kf_bad[k]);
        if (listable)
        {
            const uint64_t mk = covis_max_key(c, (uint32_t)k);
            max_key           = mk > max_key ? mk : max_key;
        }
        if (listable && c >= min_count) n_found += 1;
        else count[k] = 0;  // from here on: listed <=> count > 0
    }
    if (touched == 0) return covis_no_list(COVIS_UNCHANGED);
    if (n_found == 0)
    {
        if (max_key == 0) return covis_no_list(COVIS_OK);  // only bad keyframes touched: the connections are cleared
        conn[0] = CovisConn{(int32_t)(max_key >> 32), (int32_t)covis_max_key_id(max_key)};
        return CovisResult{1, 1, conn[0].kf, COVIS_OK};
    }
    uint64_t cut = 0;
    if (n_found > cap)
        cut = covis_cut(
            [&](uint64_t T) {
                int n = 0;
                for (int k = 0; k < n_kf; ++k) n += count[k] > 0 && covis_key(count[k], (uint32_t)k) >= T ? 1 : 0;
                return n;
            },
            cap, (uint32_t)(max_key >> 32), n_kf);
    int n = 0;
    for (int k = 0; k < n_kf; ++k)
        if (count[k] > 0 && covis_key(count[k], (uint32_t)k) >= cut) conn[n++] = CovisConn{(int32_t)count[k], k};
    std::sort(conn, conn + n, [](const CovisConn& a, const CovisConn& b) {
        return covis_key((uint32_t)a.weight, (uint32_t)a.kf) < covis_key((uint32_t)b.weight, (uint32_t)b.kf);
    });
    return CovisResult{n_found, n, conn[n - 1].kf, COVIS_OK};
}
}  // namespace snk
