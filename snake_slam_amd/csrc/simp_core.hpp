// "snk-simp v1": the culling decision for ONE keyframe -- Simplification::KeyFrameCullingGraph and Redundancy (reference
// Snake/Optimizer/Simplification.cpp:148-358, :75-146), Keyframe::MatchCount and ComputeDepthRange (reference Snake/Map/Keyframe.cpp:68-77,
// :175-206) -- as functions of plain values, so that the kernels (simp.hip) and a CPU build (tests/cpp/simp_core_driver.cpp, a debugger)
// run the same statements.  DESIGN.md section 3l.  saiga's WeightedUndirectedGraph is absent from the reference checkout: the graph
// rules (edge weight, spanning tree, weakest link) are [DEFINED] here.
//
//   depth       z = (float)(((r20 px + r21 py) + r22 pz) + tz) in double, r2. the third row of R(q) as mappoint_core.hpp spells it;
//               no contraction (the translation unit and the CPU driver are built with -ffp-contract=off)            Keyframe.cpp:193-194
//   median      element (n - 1) / 2 of the ascending order, [DEFINED] the total order of the IEEE bit patterns (-0 before +0), found by
//               a radix select on simp_key: no sort.  n = 0: -1                                                       :199-205, Keyframe.h:125
//   matches     features with a point that is not bad and a list of at least min_obs entries                          :68-77
//   redundancy  over the features with a point that is not bad, stereo: depth <= th_depth only; n_mps += 1; a list longer than 3 is
//               walked, entries of q skipped, those with octave <= octave_i + 1 counted; 3 or more: n_redundant += 1 (the early stop of
//               :131 cannot change that)                                                                              Simplification.cpp:98-145
//   nodes       id 0 = q, then q's connections with weight >= min_matches_in_graph in list order; a keyframe listed twice (or q in
//               its own list) answers to its LAST id, as id_map of :231-239 does                                      :222-239
//   edges       [DEFINED] undirected, the maximum of the weights given for a pair, self edges dropped                 :242-246
//   tree        [DEFINED] the MAXIMUM spanning tree by Prim from id 0: best (weight, parent) per outside node, the smaller parent among
//               equal weights; joins the largest weight, the smallest id among equals; unreachable nodes stay outside
//   verdict     the sequence of :150-357, simp_pre / simp_branch / simp_link
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "mappoint_core.hpp"

#if defined(__HIPCC__)
#define SNK_SIMP_HD __host__ __device__ __forceinline__
#else
#define SNK_SIMP_HD inline
#endif

namespace snk
{
constexpr int SIMP_MAX_NODES = 256;    // local graph: q and its connections above the threshold; one lane per node
constexpr int SIMP_MAX_FEAT  = 16384;  // feat_cap at most: a float per feature in LDS
enum { SIMP_OK = 0, SIMP_SKIPPED = 1, SIMP_FEAT_OVERFLOW = 2, SIMP_NODES_OVERFLOW = 3, SIMP_BAD_INDEX = 4 };
enum
{
    SIMP_NONE = 0,
    SIMP_FACTOR = 1,
    SIMP_NO_CONN = 2,
    SIMP_ANGLE = 3,
    SIMP_MATCHES = 4,
    SIMP_REDUNDANCY = 5,
    SIMP_LINK = 6,
    SIMP_KEEP_IMU_WEIGHTS = 7,
    SIMP_KEEP_TIME_GAP = 8,
    SIMP_KEEP_BRANCH = 9,
    SIMP_KEEP_DISCONNECTED = 10,
    SIMP_KEEP_LINK = 11
};
constexpr int SIMP_PT_BAD       = 1;           // pt_flags bit 0 (SNK_COVIS_PT_BAD)
constexpr int32_t SIMP_NO_EDGE  = INT32_MIN;   // a pair without an edge; [DEFINED] a weight of INT32_MIN is no edge either
constexpr uint32_t SIMP_KEY_PAD = 0xFFFFFFFFu; // the key of a slot without a depth: above every finite float's key

struct SimpStats
{
    float median_depth;
    int32_t n_depth, match_count, n_mps, n_redundant;
    float redundancy;
    int32_t status;
};
struct SimpVerdict
{
    int32_t reason, cull;
    double value;
    int32_t n_nodes, n_root_edges, weakest_link, status;
};
struct SimpConn
{
    int32_t weight, kf;
};
struct SimpParams
{
    int32_t min_matches_in_graph;
    float border_angle, border_redundancy;
    int32_t border_matches, th_map, with_imu;
    double gyro_weight, acc_weight;
    float max_time_between_kf;
};

SNK_SIMP_HD SimpStats simp_no_stats(int status) { return SimpStats{-1.0f, 0, 0, 0, 0, 0.0f, status}; }
SNK_SIMP_HD SimpVerdict simp_no_verdict(int status) { return SimpVerdict{SIMP_NONE, 0, 0.0, 0, 0, 0, status}; }
SNK_SIMP_HD SimpVerdict simp_verdict(int reason, double value, int n_nodes, int n_root, int weakest)
{
    return SimpVerdict{reason, reason >= SIMP_FACTOR && reason <= SIMP_LINK ? 1 : 0, value, n_nodes, n_root, weakest, SIMP_OK};
}

// ---- stage 1 -------------------------------------------------------------------------------------------------------------------------
// z of point p in the camera of `pose` (qx qy qz qw tx ty tz, world -> camera)  Keyframe.cpp:193-194
SNK_SIMP_HD float simp_depth(const double* pose, const double* p)
{
    const double x = pose[0], y = pose[1], z = pose[2], w = pose[3];
    const double r20 = 2 * (x * z - y * w), r21 = 2 * (y * z + x * w), r22 = 1 - 2 * (x * x + y * y);
    return (float)(((r20 * p[0] + r21 * p[1]) + r22 * p[2]) + pose[6]);
}

// ascending in the key <=> ascending in the total order of the bit patterns; no finite float has the key SIMP_KEY_PAD
SNK_SIMP_HD uint32_t simp_key(float v)
{
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
SNK_SIMP_HD float simp_unkey(uint32_t k)
{
    const uint32_t u = (k >> 31) ? (k & 0x7FFFFFFFu) : ~k;
    float v;
    memcpy(&v, &u, 4);
    return v;
}
SNK_SIMP_HD int simp_median_rank(int n) { return (n - 1) / 2; }

// The element of 0-based rank `rank` of the ascending keys without sorting them: the largest T with #{key < T} <= rank, built bit by
// bit from the top, a counting pass per bit.  count_lt(T) counts the list.  Requires 0 <= rank < length.
template <typename CountLT>
SNK_SIMP_HD uint32_t simp_select(CountLT count_lt, int rank)
{
    uint32_t T = 0;
#if defined(__clang__)
#pragma unroll 1
#endif
    for (int bit = 31; bit >= 0; --bit)
    {
        const uint32_t cand = T | (1u << bit);
        if (count_lt(cand) <= rank) T = cand;
    }
    return T;
}

// Keyframe.cpp:74
SNK_SIMP_HD bool simp_matches(unsigned flags, int list_len, int min_obs) { return !(flags & SIMP_PT_BAD) && list_len >= min_obs; }
// Simplification.cpp:105-113: does the feature's point enter n_mps?
SNK_SIMP_HD bool simp_point_counts(unsigned flags, int stereo, float depth, float th_depth)
{
    if (flags & SIMP_PT_BAD) return false;
    if (stereo && depth > th_depth) return false;
    return true;
}
SNK_SIMP_HD bool simp_list_walked(int list_len) { return list_len > 3; }  // :117
// :125-128: does the observation (k, octave_k) of a point seen by q at octave_i qualify?
SNK_SIMP_HD bool simp_obs_qualifies(int k, int q, int octave_k, int octave_i) { return k != q && octave_k <= octave_i + 1; }
SNK_SIMP_HD bool simp_redundant(int qualifying) { return qualifying >= 3; }  // :131-137
SNK_SIMP_HD float simp_redundancy(int n_redundant, int n_mps) { return (float)n_redundant / (float)n_mps; }  // :145; 0 / 0 = NaN

// ---- stage 2 -------------------------------------------------------------------------------------------------------------------------
SNK_SIMP_HD bool simp_is_node(int weight, int min_matches_in_graph) { return weight >= min_matches_in_graph; }  // :223-225

// the strict upper triangle, independent of the node count: pair (a, b), a != b
SNK_SIMP_HD int simp_tri(int a, int b)
{
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    return hi * (hi - 1) / 2 + lo;
}
SNK_SIMP_HD int32_t simp_edge_weight(int32_t stored, int32_t given) { return given > stored ? given : stored; }

// the node table sorted by kf << 32 | id: the LAST id of keyframe kf, -1 if it is no node
SNK_SIMP_HD uint64_t simp_node_key(int kf, int id) { return (uint64_t)(uint32_t)kf << 32 | (uint32_t)id; }
template <typename U64>  // uint64_t or unsigned long long: the same 64 bits under two names
SNK_SIMP_HD int simp_node_find(const U64* sorted, int n, int kf)
{
    const uint64_t above = (uint64_t)(uint32_t)kf << 32 | 0xFFFFFFFFull;
    int lo = 0, hi = n;  // the first entry > above
    while (lo < hi)
    {
        const int mid = (lo + hi) >> 1;
        if (sorted[mid] <= above) lo = mid + 1;
        else hi = mid;
    }
    if (lo == 0 || (int)(sorted[lo - 1] >> 32) != kf) return -1;
    return (int)(uint32_t)sorted[lo - 1];
}

// Prim.  The candidate of an outside node is (weight, parent); the key of the join is weight (order-preserving, unsigned) << 32 | ~id:
// its maximum over the outside nodes is the largest weight and, among equals, the smallest id; 0 = no candidate.
SNK_SIMP_HD uint64_t simp_prim_key(int32_t weight, int id)
{
    return weight == SIMP_NO_EDGE ? 0ull : ((uint64_t)((uint32_t)weight ^ 0x80000000u) << 32 | (uint32_t)~(uint32_t)id);
}
SNK_SIMP_HD int simp_prim_key_id(uint64_t key) { return (int)~(uint32_t)key; }
SNK_SIMP_HD int32_t simp_prim_key_weight(uint64_t key) { return (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u); }
// node v joined the tree: does its edge of weight w replace an outside node's candidate (best_w, parent)?
SNK_SIMP_HD bool simp_prim_better(int32_t w, int v, int32_t best_w, int parent)
{
    return w != SIMP_NO_EDGE && (best_w == SIMP_NO_EDGE || w > best_w || (w == best_w && v < parent));
}

// :150-179, before the graph: SIMP_NONE = go on.  prev / next: -1 = none or no time tables; dt = time[next] - time[prev]
SNK_SIMP_HD int simp_pre(float cull_factor, const SimpParams& P, bool have_times, int prev, int next, double dt)
{
    if (cull_factor > 3) return SIMP_FACTOR;
    if (P.with_imu)
    {
        if (P.gyro_weight == 0 || P.acc_weight == 0) return SIMP_KEEP_IMU_WEIGHTS;
        if (have_times && prev >= 0 && next >= 0 && dt > (double)P.max_time_between_kf) return SIMP_KEEP_TIME_GAP;
    }
    return SIMP_NONE;
}

// :276-280: the angle under which q and o see the scene, in degrees
SNK_SIMP_HD double simp_angle(double median_q, double median_o, const double* pose_q, const double* pose_o)
{
    double cq[3], co[3];
    mp_centre(pose_q, cq);
    mp_centre(pose_o, co);
    const double dx = cq[0] - co[0], dy = cq[1] - co[1], dz = cq[2] - co[2];
    const double baseline = sqrt((dx * dx + dy * dy) + dz * dz);
    const double depth    = (median_q + median_o) * 0.5;
    return (atan2(0.5 * baseline, depth) * 2.0) * (180.0 / 3.14159265358979323846);
}

// :287-310: one tree edge at the root
SNK_SIMP_HD int simp_branch(double angle, int match_count, float redundancy, float cull_factor, const SimpParams& P, double* value)
{
    if (angle < (double)(P.border_angle * cull_factor)) return *value = angle, SIMP_ANGLE;
    if ((float)match_count < (float)P.border_matches * cull_factor) return *value = (double)match_count, SIMP_MATCHES;
    if (redundancy > P.border_redundancy) return *value = (double)redundancy, SIMP_REDUNDANCY;
    return *value = 0.0, SIMP_KEEP_BRANCH;
}

// :341-357: the tree of the root's neighbours without the root
SNK_SIMP_HD int simp_link(bool connected, int weakest, float cull_factor, int th_map, double* value)
{
    if (!connected) return *value = 0.0, SIMP_KEEP_DISCONNECTED;
    if ((float)weakest * cull_factor > (float)th_map) return *value = (double)weakest, SIMP_LINK;
    return *value = 0.0, SIMP_KEEP_LINK;
}

// ---- the whole query on one thread: what the kernels compute, spelled as loops (host builds only use this) ----------------------------
struct SimpMapView
{
    int n_kf, n_points, n_obs, n_feat;
    const uint8_t* kf_bad;
    const double* kf_pose;
    const int32_t *feat_start, *feat_point;
    const float* feat_depth;
    const int32_t *feat_octave, *obs_start;
    const int32_t (*obs)[2];
    const uint8_t* pt_flags;
    const double* pt_pos;
};
struct SimpGraphView
{
    int n_kf, n_list;
    const uint8_t* kf_bad;
    const double* kf_pose;
    const float* kf_cull_factor;
    const double* kf_median_depth;
    const int32_t *kf_prev, *kf_next;
    const double* kf_time;
    const int32_t* conn_start;
    const SimpConn* conn_list;
};

// keys: room for feat_cap words.  The caller has checked every index.
inline SimpStats simp_stats_one(const SimpMapView& M, int q, int min_obs, int stereo, float th_depth, int feat_cap, uint32_t* keys)
{
    if (M.kf_bad[q]) return simp_no_stats(SIMP_SKIPPED);
    const int first = M.feat_start[q], last = M.feat_start[q + 1];
    if (last - first > feat_cap) return simp_no_stats(SIMP_FEAT_OVERFLOW);
    SimpStats s = simp_no_stats(SIMP_OK);
    for (int i = first; i < last; ++i)
    {
        const int p = M.feat_point[i];
        if (p < 0) continue;
        keys[s.n_depth++] = simp_key(simp_depth(M.kf_pose + 7 * (size_t)q, M.pt_pos + 3 * (size_t)p));
        const int a = M.obs_start[p], b = M.obs_start[p + 1];
        s.match_count += simp_matches(M.pt_flags[p], b - a, min_obs) ? 1 : 0;
        if (!simp_point_counts(M.pt_flags[p], stereo, M.feat_depth[i], th_depth)) continue;
        s.n_mps += 1;
        if (!simp_list_walked(b - a)) continue;
        int n = 0;
        for (int o = a; o < b; ++o)
            n += simp_obs_qualifies(M.obs[o][0], q, M.feat_octave[M.feat_start[M.obs[o][0]] + M.obs[o][1]], M.feat_octave[i]) ? 1 : 0;
        s.n_redundant += simp_redundant(n) ? 1 : 0;
    }
    if (s.n_depth > 0)
    {
        const int n = s.n_depth;
        s.median_depth = simp_unkey(simp_select(
            [&](uint32_t T) {
                int c = 0;
                for (int i = 0; i < n; ++i) c += keys[i] < T ? 1 : 0;
                return c;
            },
            simp_median_rank(n)));
    }
    s.redundancy = simp_redundancy(s.n_redundant, s.n_mps);
    return s;
}

// Prim over the nodes with member[v] != 0 from `root`; tri: the weights.  parent[v] = the tree parent (-1: outside or root).  Returns the
// number of nodes joined beside the root; *weakest = the smallest tree edge (0 without an edge).
inline int simp_prim(int n, const uint8_t* member, int root, const int32_t* tri, int* parent, int* weakest)
{
    int32_t best_w[SIMP_MAX_NODES];
    int cand[SIMP_MAX_NODES];
    uint8_t in_tree[SIMP_MAX_NODES];
    for (int v = 0; v < n; ++v)
    {
        in_tree[v] = v == root;
        parent[v]  = -1;
        cand[v]    = root;
        best_w[v]  = member[v] && v != root ? tri[simp_tri(root, v)] : SIMP_NO_EDGE;
    }
    int joined = 0, weak = 0;
    for (;;)
    {
        uint64_t key = 0;
        for (int v = 0; v < n; ++v)
            if (member[v] && !in_tree[v])
            {
                const uint64_t k = simp_prim_key(best_w[v], v);
                key              = k > key ? k : key;
            }
        if (key == 0) break;
        const int v     = simp_prim_key_id(key);
        const int32_t w = simp_prim_key_weight(key);
        in_tree[v]      = 1;
        parent[v]       = cand[v];
        weak            = joined == 0 || w < weak ? w : weak;
        joined += 1;
        for (int u = 0; u < n; ++u)
            if (member[u] && !in_tree[u] && simp_prim_better(tri[simp_tri(v, u)], v, best_w[u], cand[u])) best_w[u] = tri[simp_tri(v, u)], cand[u] = v;
    }
    *weakest = weak;
    return joined;
}

// node_kf: room for node_cap ids; sorted: node_cap keys; tri: simp_tri(node_cap - 1, node_cap - 2) + 1 words.  `stats` is q's record.
inline SimpVerdict simp_decide_one(const SimpGraphView& G, const SimpParams& P, int q, const SimpStats& stats, int node_cap, int* node_kf,
                                   uint64_t* sorted, int32_t* tri)
{
    if (G.kf_bad[q]) return simp_no_verdict(SIMP_SKIPPED);
    if (stats.status != SIMP_OK) return simp_no_verdict(stats.status);
    const float factor = G.kf_cull_factor[q];
    const bool times   = G.kf_time != nullptr;
    const int prev = times ? G.kf_prev[q] : -1, next = times ? G.kf_next[q] : -1;
    const int pre = simp_pre(factor, P, times, prev, next, prev >= 0 && next >= 0 ? G.kf_time[next] - G.kf_time[prev] : 0.0);
    if (pre != SIMP_NONE) return simp_verdict(pre, 0.0, 0, 0, 0);
    // nodes
    int n      = 1;
    node_kf[0] = q;
    for (int c = G.conn_start[q]; c < G.conn_start[q + 1]; ++c)
        if (simp_is_node(G.conn_list[c].weight, P.min_matches_in_graph))
        {
            if (n < node_cap) node_kf[n] = G.conn_list[c].kf;
            n += 1;
        }
    if (n > node_cap) return simp_no_verdict(SIMP_NODES_OVERFLOW);
    for (int i = 0; i < n; ++i)  // a rank sort: the keys are distinct
    {
        const uint64_t k = simp_node_key(node_kf[i], i);
        int r            = 0;
        for (int j = 0; j < n; ++j) r += simp_node_key(node_kf[j], j) < k ? 1 : 0;
        sorted[r] = k;
    }
    // edges
    for (int i = 0; i < n * (n - 1) / 2; ++i) tri[i] = SIMP_NO_EDGE;
    for (int l = 0; l < n; ++l)
    {
        const int owner = node_kf[l], from = simp_node_find(sorted, n, owner);
        for (int c = G.conn_start[owner]; c < G.conn_start[owner + 1]; ++c)
        {
            if (l == 0 && !simp_is_node(G.conn_list[c].weight, P.min_matches_in_graph)) continue;
            const int to = simp_node_find(sorted, n, G.conn_list[c].kf);
            if (to < 0 || to == from) continue;
            tri[simp_tri(from, to)] = simp_edge_weight(tri[simp_tri(from, to)], G.conn_list[c].weight);
        }
    }
    uint8_t member[SIMP_MAX_NODES];
    int parent[SIMP_MAX_NODES];
    for (int v = 0; v < n; ++v) member[v] = 1;
    int weakest = 0;
    simp_prim(n, member, 0, tri, parent, &weakest);
    int n_root = 0, o = -1, first = -1;
    for (int v = 1; v < n; ++v)
    {
        member[v] = parent[v] == 0;
        if (member[v]) n_root += 1, o = v, first = first < 0 ? v : first;
    }
    member[0] = 0;
    if (n_root == 0) return simp_verdict(SIMP_NO_CONN, 0.0, n, 0, 0);
    double value = 0.0;
    if (n_root == 1)
    {
        const int ko       = node_kf[o];
        const double angle = simp_angle(G.kf_median_depth[q], G.kf_median_depth[ko], G.kf_pose + 7 * (size_t)q, G.kf_pose + 7 * (size_t)ko);
        const int reason   = simp_branch(angle, stats.match_count, stats.redundancy, factor, P, &value);
        return simp_verdict(reason, value, n, 1, 0);
    }
    const int joined = simp_prim(n, member, first, tri, parent, &weakest);
    const bool connected = joined == n_root - 1;
    const int reason     = simp_link(connected, weakest, factor, P.th_map, &value);
    return simp_verdict(reason, value, n, n_root, connected ? weakest : 0);
}
}  // namespace snk
