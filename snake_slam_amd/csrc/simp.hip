// Keyframe culling for gfx950 ("snk-simp v1") — replaces, for many keyframes per call,
//   Simplification::KeyFrameCullingGraph, Redundancy   (reference Snake/Optimizer/Simplification.cpp:148-358, :75-146)
//   Keyframe::MatchCount, ComputeDepthRange            (reference Snake/Map/Keyframe.cpp:68-77, :175-206)
// The per-query statements are simp_core.hpp's; the long-list threshold and the carves are dispatch.hpp's.
//
// Mapping to the hardware.  Both kernels: a workgroup of four wavefronts per query, every byte of LDS in the dynamic carve, no scratch.
// simp_stats_kernel: a lane takes a feature, computes its depth key into LDS and reads its point's list bounds; the lists are walked by
// walk_lists (wg.hpp: a short one by its lane, a long one by a wavefront).  The early stop at three qualifying observations is a
// count >= 3.  The counts are integer sums, the median is a radix select on the ordered key (a counting pass per
// bit): nothing depends on the order in which lanes finish.
// simp_decide_kernel: the nodes are compacted in list order by a prefix sum, the node table is rank-sorted by keyframe so that a target's
// local id is a binary search, and every node's list is walked by a wavefront, a lane per entry, the weight going into the strict upper
// triangle of the weight matrix by an LDS atomic max (maxima commute).  Prim: a lane per node, one reduction per step on the key
// weight << 32 | ~id.  The second graph is the same matrix restricted to the root's tree neighbours.
// The host entries check every table and upload it; the device entries launch the same kernels, which check what the host could not
// see and answer SNK_SIMP_BAD_INDEX per query.
#include <cstddef>

#include "matcher_handle.hpp"

#include "dispatch.hpp"
#include "simp_core.hpp"
#include "wg.hpp"

namespace snk
{
namespace
{
using u8  = unsigned char;
using u32 = unsigned int;
using u64 = unsigned long long;

static_assert(sizeof(snk_simp_stats_result) == 28 && sizeof(SimpStats) == 28 && sizeof(snk_simp_verdict) == 32 && sizeof(SimpVerdict) == 32 &&
                  sizeof(snk_simp_params) == sizeof(SimpParams) && sizeof(SimpParams) == 48 && sizeof(SimpConn) == sizeof(snk_covis_conn),
              "snk-simp layouts");
static_assert(SIMP_MAX_NODES == SNK_SIMP_MAX_NODES && SIMP_MAX_FEAT == SNK_SIMP_MAX_FEAT && SIMP_PT_BAD == SNK_COVIS_PT_BAD, "snk-simp limits");
static_assert(SIMP_OK == SNK_SIMP_OK && SIMP_SKIPPED == SNK_SIMP_SKIPPED && SIMP_FEAT_OVERFLOW == SNK_SIMP_FEAT_OVERFLOW &&
                  SIMP_NODES_OVERFLOW == SNK_SIMP_NODES_OVERFLOW && SIMP_BAD_INDEX == SNK_SIMP_BAD_INDEX,
              "snk-simp status values");
static_assert(SIMP_NONE == SNK_SIMP_NONE && SIMP_FACTOR == SNK_SIMP_FACTOR && SIMP_NO_CONN == SNK_SIMP_NO_CONN && SIMP_ANGLE == SNK_SIMP_ANGLE &&
                  SIMP_MATCHES == SNK_SIMP_MATCHES && SIMP_REDUNDANCY == SNK_SIMP_REDUNDANCY && SIMP_LINK == SNK_SIMP_LINK &&
                  SIMP_KEEP_IMU_WEIGHTS == SNK_SIMP_KEEP_IMU_WEIGHTS && SIMP_KEEP_TIME_GAP == SNK_SIMP_KEEP_TIME_GAP &&
                  SIMP_KEEP_BRANCH == SNK_SIMP_KEEP_BRANCH && SIMP_KEEP_DISCONNECTED == SNK_SIMP_KEEP_DISCONNECTED && SIMP_KEEP_LINK == SNK_SIMP_KEEP_LINK,
              "snk-simp reasons");
static_assert(simp_stats_carve(SIMP_MAX_FEAT) <= (size_t)LDS_MAX_BYTES && simp_decide_carve(SIMP_MAX_NODES) <= (size_t)LDS_MAX_BYTES, "LDS carves");
static_assert(SIMP_THREADS == 256 && SIMP_THREADS == SIMP_MAX_NODES && SIMP_MISC >= 32, "a lane per node; the words of s_misc");

struct SimpStatsCall
{
    SimpMapView M;
    int n_q, min_obs, stereo, feat_cap, long_min;
    float th_depth;
    const int* q;
    SimpStats* out;
};
struct SimpDecideCall
{
    SimpGraphView G;
    SimpParams P;
    int n_q, node_cap;
    const int* q;
    const SimpStats* stats;
    SimpVerdict* out;
};

// words of s_misc: flags and sums, then two banks of four u64 (block_reduce), then two banks of four u32 (block_scan)
enum { W_BAD = 0, W_QUEUED = 1, W_NDEPTH = 2, W_MATCH = 3, W_NMPS = 4, W_NRED = 5, W_PART64 = 8, W_PART32 = 24 };

__global__ __launch_bounds__(SIMP_THREADS) void simp_stats_kernel(SimpStatsCall c)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u32* s_key   = reinterpret_cast<u32*>(smem);                         // [feat_cap rounded up to 4]
    int* s_queue = reinterpret_cast<int*>(s_key + ((c.feat_cap + 3) & ~3));  // [SIMP_THREADS] features whose lists a wavefront walks
    u32* s_misc  = reinterpret_cast<u32*>(s_queue + SIMP_THREADS);       // [SIMP_MISC]
    u64* s_part  = reinterpret_cast<u64*>(s_misc + W_PART64);
    const SimpMapView& M = c.M;
    const int tid = threadIdx.x, lane = tid & 63;
    const int set = blockIdx.x;

    if (tid < SIMP_MISC) s_misc[tid] = 0;
    // ---- the query (uniform) ----
    const int q = c.q[set];
    int status  = SIMP_OK, first = 0, last = 0;
    if (q < 0 || q >= M.n_kf) status = SIMP_BAD_INDEX;
    else if (M.kf_bad[q]) status = SIMP_SKIPPED;
    else
    {
        first = M.feat_start[q], last = M.feat_start[q + 1];
        if (first < 0 || last < first || last > M.n_feat) status = SIMP_BAD_INDEX;
        else if (last - first > c.feat_cap) status = SIMP_FEAT_OVERFLOW;
    }
    if (status != SIMP_OK)
    {
        if (tid == 0) c.out[set] = simp_no_stats(status);
        return;
    }
    __syncthreads();
    double pose[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) pose[j] = M.kf_pose[(size_t)q * 7 + j];
    const int2* obs = reinterpret_cast<const int2*>(M.obs);

    // the bounds of point p's list; false: outside obs
    auto list_of = [&](int p, int& a, int& b) {
        a = M.obs_start[p], b = M.obs_start[p + 1];
        return a >= 0 && b >= a && b <= M.n_obs;
    };
    // does observation o qualify for a feature of octave octave_i?  Checks the keyframe and the feature index before octave is read.
    auto qualifies = [&](int o, int octave_i) {
        const int2 e = obs[o];
        if (e.x < 0 || e.x >= M.n_kf) return s_misc[W_BAD] = 1, 0;
        const int fa = M.feat_start[e.x], fb = M.feat_start[e.x + 1];
        if (fa < 0 || fb < fa || fb > M.n_feat || e.y < 0 || e.y >= fb - fa) return s_misc[W_BAD] = 1, 0;
        return simp_obs_qualifies(e.x, q, M.feat_octave[fa + e.y], octave_i) ? 1 : 0;
    };

    int n_depth = 0, match = 0, n_mps = 0, n_red = 0;
    walk_lists<SIMP_THREADS>(
        first, last, c.long_min, s_queue, &s_misc[W_QUEUED],
        [&](int i, int& fi, int& a, int& b) {  // every feature: its depth key and counts; true: its list is walked
            const int p = M.feat_point[i];
            u32 key     = SIMP_KEY_PAD;
            bool walked = false;
            if (p < -1 || p >= M.n_points) s_misc[W_BAD] = 1;
            else if (p >= 0)
            {
                key = simp_key(simp_depth(pose, M.pt_pos + (size_t)p * 3));
                n_depth += 1;
                const unsigned flags = M.pt_flags[p];
                if (flags & SIMP_PT_BAD) {}
                else if (!list_of(p, a, b)) s_misc[W_BAD] = 1;
                else
                {
                    match += simp_matches(flags, b - a, c.min_obs) ? 1 : 0;
                    if (simp_point_counts(flags, c.stereo, M.feat_depth[i], c.th_depth))
                    {
                        n_mps += 1;
                        walked = simp_list_walked(b - a);
                    }
                }
            }
            s_key[i - first] = key;
            fi               = i;
            return walked;
        },
        [&](int fi, int a, int b) {
            const int octave_i = M.feat_octave[fi];
            int n              = 0;
            for (int o = a; o < b; ++o) n += qualifies(o, octave_i);
            n_red += simp_redundant(n) ? 1 : 0;
        },
        [&](int fi, int lane) {
            int la, lb;
            list_of(M.feat_point[fi], la, lb);  // checked when it was queued
            const int octave_i = M.feat_octave[fi];
            int n              = 0;
            for (int o = la + lane; o < lb; o += 64) n += qualifies(o, octave_i);
            n = wave_sum_xor(n);
            if (lane == 0) n_red += simp_redundant(n) ? 1 : 0;
        });
    n_depth = wave_sum_xor(n_depth);
    match   = wave_sum_xor(match);
    n_mps   = wave_sum_xor(n_mps);
    n_red   = wave_sum_xor(n_red);
    if (lane == 0)
    {
        atomicAdd(&s_misc[W_NDEPTH], (u32)n_depth);
        atomicAdd(&s_misc[W_MATCH], (u32)match);
        atomicAdd(&s_misc[W_NMPS], (u32)n_mps);
        atomicAdd(&s_misc[W_NRED], (u32)n_red);
    }
    __syncthreads();
    if (s_misc[W_BAD])  // uniform
    {
        if (tid == 0) c.out[set] = simp_no_stats(SIMP_BAD_INDEX);
        return;
    }
    SimpStats r   = simp_no_stats(SIMP_OK);
    r.n_depth     = (int)s_misc[W_NDEPTH];
    r.match_count = (int)s_misc[W_MATCH];
    r.n_mps       = (int)s_misc[W_NMPS];
    r.n_redundant = (int)s_misc[W_NRED];
    r.redundancy  = simp_redundancy(r.n_redundant, r.n_mps);
    if (r.n_depth > 0)  // uniform
    {
        const int n = last - first;
        int pass    = 0;
        r.median_depth = simp_unkey(simp_select(
            [&](u32 T) {
                int k = 0;
                for (int i = tid; i < n; i += SIMP_THREADS) k += s_key[i] < T ? 1 : 0;  // the pads are above every T the select can reach
                return (int)block_reduce<SIMP_THREADS>((u64)k, [](u64 a, u64 b) { return a + b; }, s_part, pass);
            },
            simp_median_rank(r.n_depth)));
    }
    if (tid == 0) c.out[set] = r;
}

// Prim over the nodes with `member` from `root`, a lane per node (v = threadIdx.x).  parent: this node's tree parent (-1: outside or the
// root).  Returns the number of nodes joined beside the root (uniform); weakest: the smallest tree edge (0 without one).
__device__ __forceinline__ int simp_prim_lanes(int n, bool member, int root, const int32_t* s_tri, u64* s_part, int& pass, int& parent, int& weakest)
{
    const int v  = threadIdx.x;
    bool outside = member && v != root;
    int cand     = root;
    int32_t best = outside ? s_tri[simp_tri(root, v)] : SIMP_NO_EDGE;
    parent       = -1;
    int joined = 0, weak = 0;
    for (int step = 1; step < n; ++step)  // uniform: at most n - 1 joins
    {
        const u64 key = block_reduce<SIMP_THREADS>(outside ? simp_prim_key(best, v) : 0ull, [](u64 a, u64 b) { return a > b ? a : b; }, s_part, pass);
        if (key == 0) break;
        const int j     = simp_prim_key_id(key);
        const int32_t w = simp_prim_key_weight(key);
        if (v == j) outside = false, parent = cand;
        else if (outside)
        {
            const int32_t w2 = s_tri[simp_tri(j, v)];
            if (simp_prim_better(w2, j, best, cand)) best = w2, cand = j;
        }
        weak = joined == 0 || w < weak ? w : weak;
        joined += 1;
    }
    weakest = weak;
    return joined;
}

__global__ __launch_bounds__(SIMP_THREADS) void simp_decide_kernel(SimpDecideCall c)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int cap    = c.node_cap;
    int32_t* s_tri   = reinterpret_cast<int32_t*>(smem);                                   // [cap (cap - 1) / 2 rounded up to 2]
    u64* s_sorted    = reinterpret_cast<u64*>(s_tri + ((cap * (cap - 1) / 2 + 1) & ~1));   // [cap]
    int* s_node      = reinterpret_cast<int*>(s_sorted + cap);                              // [cap rounded up to 2]
    u32* s_misc      = reinterpret_cast<u32*>(s_node + ((cap + 1) & ~1));                   // [SIMP_MISC]
    u64* s_part      = reinterpret_cast<u64*>(s_misc + W_PART64);
    const SimpGraphView& G = c.G;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int set = blockIdx.x;
    auto in_kf    = [&](int k) { return k >= 0 && k < G.n_kf; };
    auto range_of = [&](int k, int& a, int& b) {
        a = G.conn_start[k], b = G.conn_start[k + 1];
        return a >= 0 && b >= a && b <= G.n_list;
    };

    if (tid < SIMP_MISC) s_misc[tid] = 0;
    // ---- before the graph (uniform) ----
    const int q = c.q[set];
    SimpVerdict early = simp_no_verdict(SIMP_OK);
    bool done         = true;
    float factor      = 0.0f;
    int ca = 0, cb = 0;
    if (!in_kf(q)) early.status = SIMP_BAD_INDEX;
    else if (G.kf_bad[q]) early.status = SIMP_SKIPPED;
    else if (c.stats[set].status != SIMP_OK) early.status = c.stats[set].status;
    else
    {
        factor           = G.kf_cull_factor[q];
        const bool times = G.kf_time != nullptr;
        int prev = -1, next = -1;
        double dt    = 0.0;
        bool bad_idx = false;
        if (!(factor > 3) && c.P.with_imu && c.P.gyro_weight != 0 && c.P.acc_weight != 0 && times)  // the only path that reads them
        {
            prev = G.kf_prev[q], next = G.kf_next[q];
            if (prev < -1 || prev >= G.n_kf || next < -1 || next >= G.n_kf) bad_idx = true;
            else if (prev >= 0 && next >= 0) dt = G.kf_time[next] - G.kf_time[prev];
        }
        const int pre = bad_idx ? SIMP_NONE : simp_pre(factor, c.P, times, prev, next, dt);
        if (bad_idx) early.status = SIMP_BAD_INDEX;
        else if (pre != SIMP_NONE) early = simp_verdict(pre, 0.0, 0, 0, 0);
        else if (!range_of(q, ca, cb)) early.status = SIMP_BAD_INDEX;
        else done = false;
    }
    if (done)
    {
        if (tid == 0) c.out[set] = early;
        return;
    }
    __syncthreads();

    // ---- nodes: q, then its connections of weight >= min_matches_in_graph in list order ----
    int n = 1, pass32 = 0, pass = 0;
    if (tid == 0) s_node[0] = q;
    for (int base = ca; base < cb; base += SIMP_THREADS)  // uniform
    {
        const int e = base + tid;
        int take = 0, kf = -1;
        if (e < cb)
        {
            const SimpConn cn = G.conn_list[e];
            kf                = cn.kf;
            if (!in_kf(kf)) s_misc[W_BAD] = 1;
            else take = simp_is_node(cn.weight, c.P.min_matches_in_graph) ? 1 : 0;
        }
        int total;
        const int pos = block_scan<SIMP_THREADS>(take, total, s_misc + W_PART32, pass32);
        if (take && n + pos < cap) s_node[n + pos] = kf;
        n += total;
    }
    __syncthreads();
    if (s_misc[W_BAD] || n > cap)  // uniform
    {
        if (tid == 0) c.out[set] = simp_no_verdict(s_misc[W_BAD] ? SIMP_BAD_INDEX : SIMP_NODES_OVERFLOW);
        return;
    }
    // the node table sorted by (kf, id): a rank sort, the keys are distinct
    if (tid < n)
    {
        const u64 key = simp_node_key(s_node[tid], tid);
        int r         = 0;
        for (int j = 0; j < n; ++j) r += simp_node_key(s_node[j], j) < key ? 1 : 0;
        s_sorted[r] = key;
    }
    for (int i = tid; i < n * (n - 1) / 2; i += SIMP_THREADS) s_tri[i] = SIMP_NO_EDGE;
    __syncthreads();

    // ---- edges: q's filtered list, every other node's full list; a wavefront per list, a lane per entry ----
    for (int l = wave; l < n; l += SIMP_THREADS / 64)
    {
        const int owner = s_node[l], from = simp_node_find(s_sorted, n, owner);
        int la, lb;
        if (!range_of(owner, la, lb))
        {
            s_misc[W_BAD] = 1;
            continue;
        }
        for (int e = la + lane; e < lb; e += 64)
        {
            const SimpConn cn = G.conn_list[e];
            if (!in_kf(cn.kf))
            {
                s_misc[W_BAD] = 1;
                continue;
            }
            if (l == 0 && !simp_is_node(cn.weight, c.P.min_matches_in_graph)) continue;
            const int to = simp_node_find(s_sorted, n, cn.kf);
            if (to >= 0 && to != from) atomicMax(&s_tri[simp_tri(from, to)], cn.weight);
        }
    }
    __syncthreads();
    if (s_misc[W_BAD])  // uniform
    {
        if (tid == 0) c.out[set] = simp_no_verdict(SIMP_BAD_INDEX);
        return;
    }

    // ---- the tree from q, its edges at q ----
    int parent, weakest;
    simp_prim_lanes(n, tid < n, 0, s_tri, s_part, pass, parent, weakest);
    const bool at_root = tid < n && tid != 0 && parent == 0;
    const int n_root   = (int)block_reduce<SIMP_THREADS>((u64)(at_root ? 1 : 0), [](u64 a, u64 b) { return a + b; }, s_part, pass);
    if (n_root == 0)  // uniform
    {
        if (tid == 0) c.out[set] = simp_verdict(SIMP_NO_CONN, 0.0, n, 0, 0);
        return;
    }
    // the smallest neighbour id: ~id is largest
    const int first = (int)~(u32)block_reduce<SIMP_THREADS>(at_root ? (u64)(u32)~(u32)tid : 0ull, [](u64 a, u64 b) { return a > b ? a : b; }, s_part, pass);
    double value = 0.0;
    if (n_root == 1)  // uniform
    {
        if (tid == 0)
        {
            const int ko       = s_node[first];
            const double angle = simp_angle(G.kf_median_depth[q], G.kf_median_depth[ko], G.kf_pose + (size_t)q * 7, G.kf_pose + (size_t)ko * 7);
            const SimpStats st = c.stats[set];
            const int reason   = simp_branch(angle, st.match_count, st.redundancy, factor, c.P, &value);
            c.out[set]         = simp_verdict(reason, value, n, 1, 0);
        }
        return;
    }
    // ---- two or more: the tree of the neighbours alone ----
    const int joined     = simp_prim_lanes(n, at_root, first, s_tri, s_part, pass, parent, weakest);
    const bool connected = joined == n_root - 1;
    if (tid == 0)
    {
        const int reason = simp_link(connected, weakest, factor, c.P.th_map, &value);
        c.out[set]       = simp_verdict(reason, value, n, n_root, connected ? weakest : 0);
    }
}

int long_env()
{
    // SNK_SIMP_LONG_MIN=<n> (tests, A/B): read once
    static const int env = [] {
        const char* s = getenv("SNK_SIMP_LONG_MIN");
        if (!s || !*s) return -1;
        char* end    = nullptr;
        const long v = strtol(s, &end, 10);
        return (*end || v < 0 || v > 0x7FFFFFFFL) ? -1 : (int)v;
    }();
    return env;
}

int check_stats_scalars(const snk_simp_map* map, const snk_simp_stats_params* params, int n_q, const void* q, const void* out)
{
    SNK_REQUIRE(map != nullptr && params != nullptr, "keyframe culling: map or params is NULL");
    SNK_REQUIRE(map->n_kf >= 0 && map->n_points >= 0 && map->n_obs >= 0 && map->n_feat >= 0 && n_q >= 0, "keyframe culling: negative count");
    SNK_REQUIRE(map->n_kf <= SNK_COVIS_MAX_KF, "keyframe culling: n_kf above SNK_COVIS_MAX_KF (32768)");
    SNK_REQUIRE(params->feat_cap >= 1 && params->feat_cap <= SNK_SIMP_MAX_FEAT, "keyframe culling: feat_cap outside [1, SNK_SIMP_MAX_FEAT]");
    SNK_REQUIRE(map->n_kf == 0 || (map->kf_bad != nullptr && map->kf_pose != nullptr), "keyframe culling: NULL keyframe table with n_kf > 0");
    SNK_REQUIRE(map->feat_start != nullptr && map->obs_start != nullptr, "keyframe culling: NULL start array");
    SNK_REQUIRE(map->n_feat == 0 || (map->feat_point != nullptr && map->feat_depth != nullptr && map->feat_octave != nullptr),
                "keyframe culling: NULL feature table with n_feat > 0");
    SNK_REQUIRE(map->n_points == 0 || (map->pt_flags != nullptr && map->pt_pos != nullptr), "keyframe culling: NULL point table with n_points > 0");
    SNK_REQUIRE(map->n_obs == 0 || map->obs != nullptr, "keyframe culling: NULL obs with n_obs > 0");
    SNK_REQUIRE(n_q == 0 || (q != nullptr && out != nullptr), "keyframe culling: NULL array with n_q > 0");
    return SNK_OK;
}

int check_graph_scalars(const snk_simp_graph* g, const snk_simp_params* params, int node_cap, int n_q, const void* q, const void* stats, const void* out)
{
    SNK_REQUIRE(g != nullptr && params != nullptr, "keyframe culling: graph or params is NULL");
    SNK_REQUIRE(g->n_kf >= 0 && g->n_list >= 0 && n_q >= 0, "keyframe culling: negative count");
    SNK_REQUIRE(g->n_kf <= SNK_COVIS_MAX_KF, "keyframe culling: n_kf above SNK_COVIS_MAX_KF (32768)");
    SNK_REQUIRE(node_cap >= 1 && node_cap <= SNK_SIMP_MAX_NODES, "keyframe culling: node_cap outside [1, SNK_SIMP_MAX_NODES]");
    SNK_REQUIRE(g->n_kf == 0 || (g->kf_bad != nullptr && g->kf_pose != nullptr && g->kf_cull_factor != nullptr && g->kf_median_depth != nullptr),
                "keyframe culling: NULL keyframe table with n_kf > 0");
    const int n_time = (g->kf_prev != nullptr) + (g->kf_next != nullptr) + (g->kf_time != nullptr);
    SNK_REQUIRE(n_time == 0 || n_time == 3, "keyframe culling: kf_prev, kf_next and kf_time are all NULL or all present");
    SNK_REQUIRE(g->conn_start != nullptr, "keyframe culling: NULL conn_start");
    SNK_REQUIRE(g->n_list == 0 || g->conn_list != nullptr, "keyframe culling: NULL conn_list with n_list > 0");
    SNK_REQUIRE(n_q == 0 || (q != nullptr && stats != nullptr && out != nullptr), "keyframe culling: NULL array with n_q > 0");
    return SNK_OK;
}

SimpMapView map_view(const snk_simp_map* map)
{
    return SimpMapView{map->n_kf,      map->n_points,    map->n_obs,    map->n_feat, map->kf_bad,   map->kf_pose, map->feat_start,
                       map->feat_point, map->feat_depth, map->feat_octave, map->obs_start, map->obs, map->pt_flags, map->pt_pos};
}

SimpGraphView graph_view(const snk_simp_graph* g)
{
    return SimpGraphView{g->n_kf,   g->n_list,  g->kf_bad,  g->kf_pose,    g->kf_cull_factor, g->kf_median_depth,
                         g->kf_prev, g->kf_next, g->kf_time, g->conn_start, reinterpret_cast<const SimpConn*>(g->conn_list)};
}

SimpParams params_of(const snk_simp_params* p)
{
    return SimpParams{p->min_matches_in_graph, p->border_angle, p->border_redundancy, p->border_matches, p->th_map, p->with_imu,
                      p->gyro_weight,          p->acc_weight,   p->max_time_between_kf};
}

int launch_stats(snk_matcher* m, const SimpMapView& M, const snk_simp_stats_params* params, int n_q, const int* q, SimpStats* out)
{
    SimpStatsCall C{M, n_q, params->min_obs, params->stereo, params->feat_cap, simp_long_min(long_env()), params->th_depth, q, out};
    int rc;
    if ((rc = set_max_lds_once(reinterpret_cast<const void*>(simp_stats_kernel), (int)simp_stats_carve(SIMP_MAX_FEAT))) != SNK_OK) return rc;
    hipLaunchKernelGGL(simp_stats_kernel, dim3(n_q), dim3(SIMP_THREADS), simp_stats_carve(params->feat_cap), m->stream, C);
    SNK_LAUNCH_CHECK();
    return SNK_OK;
}

int launch_decide(snk_matcher* m, const SimpGraphView& G, const snk_simp_params* params, int node_cap, int n_q, const int* q, const SimpStats* stats,
                  SimpVerdict* out)
{
    SimpDecideCall C{G, params_of(params), n_q, node_cap, q, stats, out};
    int rc;
    if ((rc = set_max_lds_once(reinterpret_cast<const void*>(simp_decide_kernel), (int)simp_decide_carve(SIMP_MAX_NODES))) != SNK_OK) return rc;
    hipLaunchKernelGGL(simp_decide_kernel, dim3(n_q), dim3(SIMP_THREADS), simp_decide_carve(node_cap), m->stream, C);
    SNK_LAUNCH_CHECK();
    return SNK_OK;
}
}  // namespace
}  // namespace snk

using namespace snk;

extern "C" {
int snk_simp_stats(snk_matcher* m, const snk_simp_map* map, const snk_simp_stats_params* params, int n_q, const int32_t* q, snk_simp_stats_result* out)
{
    SNK_REQUIRE(m != nullptr, "NULL handle");
    int rc;
    if ((rc = check_stats_scalars(map, params, n_q, q, out)) != SNK_OK) return rc;
    // the host's look at the map: everything the kernel would otherwise have to refuse
    if ((rc = check_starts(map->feat_start, map->n_kf, "keyframe culling: feat_start[0] must be 0", "keyframe culling: feat_start must be non-decreasing")) != SNK_OK) return rc;
    SNK_REQUIRE(map->feat_start[map->n_kf] == map->n_feat, "keyframe culling: feat_start[n_kf] must be n_feat");
    if ((rc = check_starts(map->obs_start, map->n_points, "keyframe culling: obs_start[0] must be 0", "keyframe culling: obs_start must be non-decreasing")) != SNK_OK) return rc;
    SNK_REQUIRE(map->obs_start[map->n_points] == map->n_obs, "keyframe culling: obs_start[n_points] must be n_obs");
    for (int i = 0; i < map->n_feat; ++i)
        SNK_REQUIRE(map->feat_point[i] >= -1 && map->feat_point[i] < map->n_points, "keyframe culling: a point id outside [-1, n_points)");
    for (int o = 0; o < map->n_obs; ++o)
    {
        const int k = map->obs[o][0], f = map->obs[o][1];
        SNK_REQUIRE(k >= 0 && k < map->n_kf, "keyframe culling: an observation's keyframe outside [0, n_kf)");
        SNK_REQUIRE(f >= 0 && f < map->feat_start[k + 1] - map->feat_start[k], "keyframe culling: an observation's feature index outside its keyframe");
    }
    for (int i = 0; i < n_q; ++i) SNK_REQUIRE(q[i] >= 0 && q[i] < map->n_kf, "keyframe culling: a query outside [0, n_kf)");
    if (n_q == 0) return SNK_OK;

    const size_t n_kf = (size_t)map->n_kf, n_pts = (size_t)map->n_points, n_obs = (size_t)map->n_obs, n_feat = (size_t)map->n_feat, ns = (size_t)n_q;
    Block in, out_b;
    const int i_bad = in.add(map->kf_bad, n_kf), i_pose = in.add(map->kf_pose, n_kf * 56), i_fs = in.add(map->feat_start, (n_kf + 1) * 4),
              i_fp = in.add(map->feat_point, n_feat * 4), i_fd = in.add(map->feat_depth, n_feat * 4), i_fo = in.add(map->feat_octave, n_feat * 4),
              i_os = in.add(map->obs_start, (n_pts + 1) * 4), i_obs = in.add(map->obs, n_obs * 8), i_fl = in.add(map->pt_flags, n_pts),
              i_pos = in.add(map->pt_pos, n_pts * 24), i_q = in.add(q, ns * 4);
    const int o_res = out_b.add(nullptr, ns * sizeof(SimpStats));
    SNK_HIP_CHECK(hipSetDevice(m->device));
    if ((rc = stage_reserve(m, in.bytes, out_b.end())) != SNK_OK) return rc;
    if ((rc = stage_upload(m, in)) != SNK_OK) return rc;
    char *dev = m->q.as<char>(), *dout = m->out.as<char>(), *res = m->h_res.as<char>();
    SimpMapView M = map_view(map);
    M.kf_bad      = in.at<const u8>(dev, i_bad);
    M.kf_pose     = in.at<const double>(dev, i_pose);
    M.feat_start  = in.at<const int32_t>(dev, i_fs);
    M.feat_point  = in.at<const int32_t>(dev, i_fp);
    M.feat_depth  = in.at<const float>(dev, i_fd);
    M.feat_octave = in.at<const int32_t>(dev, i_fo);
    M.obs_start   = in.at<const int32_t>(dev, i_os);
    M.obs         = reinterpret_cast<const int32_t(*)[2]>(in.at<const int32_t>(dev, i_obs));
    M.pt_flags    = in.at<const u8>(dev, i_fl);
    M.pt_pos      = in.at<const double>(dev, i_pos);
    if ((rc = launch_stats(m, M, params, n_q, in.at<const int>(dev, i_q), out_b.at<SimpStats>(dout, o_res))) != SNK_OK) return rc;
    if ((rc = stage_download(m, 0, out_b.end())) != SNK_OK) return rc;
    memcpy(out, out_b.at<char>(res, o_res), ns * sizeof(SimpStats));
    return SNK_OK;
}

int snk_simp_stats_batch_dev(snk_matcher* m, const snk_simp_map* map_dev, const snk_simp_stats_params* params, int n_q, const int32_t* q_dev,
                             snk_simp_stats_result* out_dev)
{
    SNK_REQUIRE(m != nullptr, "NULL handle");
    int rc;
    if ((rc = check_stats_scalars(map_dev, params, n_q, q_dev, out_dev)) != SNK_OK) return rc;
    if (n_q == 0) return SNK_OK;
    SNK_HIP_CHECK(hipSetDevice(m->device));
    return launch_stats(m, map_view(map_dev), params, n_q, q_dev, reinterpret_cast<SimpStats*>(out_dev));
}

int snk_simp_decide(snk_matcher* m, const snk_simp_graph* graph, const snk_simp_params* params, int node_cap, int n_q, const int32_t* q,
                    const snk_simp_stats_result* stats, snk_simp_verdict* out)
{
    SNK_REQUIRE(m != nullptr, "NULL handle");
    int rc;
    if ((rc = check_graph_scalars(graph, params, node_cap, n_q, q, stats, out)) != SNK_OK) return rc;
    const snk_simp_graph* g = graph;
    if ((rc = check_starts(g->conn_start, g->n_kf, "keyframe culling: conn_start[0] must be 0", "keyframe culling: conn_start must be non-decreasing")) != SNK_OK) return rc;
    SNK_REQUIRE(g->conn_start[g->n_kf] == g->n_list, "keyframe culling: conn_start[n_kf] must be n_list");
    for (int e = 0; e < g->n_list; ++e) SNK_REQUIRE(g->conn_list[e].kf >= 0 && g->conn_list[e].kf < g->n_kf, "keyframe culling: a connection outside [0, n_kf)");
    if (g->kf_time)
        for (int k = 0; k < g->n_kf; ++k)
            SNK_REQUIRE(g->kf_prev[k] >= -1 && g->kf_prev[k] < g->n_kf && g->kf_next[k] >= -1 && g->kf_next[k] < g->n_kf,
                        "keyframe culling: kf_prev or kf_next outside [-1, n_kf)");
    for (int i = 0; i < n_q; ++i) SNK_REQUIRE(q[i] >= 0 && q[i] < g->n_kf, "keyframe culling: a query outside [0, n_kf)");
    if (n_q == 0) return SNK_OK;

    const size_t n_kf = (size_t)g->n_kf, n_list = (size_t)g->n_list, ns = (size_t)n_q, nt = g->kf_time ? n_kf : 0;
    Block in, out_b;
    const int i_bad = in.add(g->kf_bad, n_kf), i_pose = in.add(g->kf_pose, n_kf * 56), i_cf = in.add(g->kf_cull_factor, n_kf * 4),
              i_md = in.add(g->kf_median_depth, n_kf * 8), i_prev = in.add(g->kf_prev, nt * 4), i_next = in.add(g->kf_next, nt * 4),
              i_time = in.add(g->kf_time, nt * 8), i_cs = in.add(g->conn_start, (n_kf + 1) * 4), i_cl = in.add(g->conn_list, n_list * 8),
              i_q = in.add(q, ns * 4), i_st = in.add(stats, ns * sizeof(SimpStats));
    const int o_res = out_b.add(nullptr, ns * sizeof(SimpVerdict));
    SNK_HIP_CHECK(hipSetDevice(m->device));
    if ((rc = stage_reserve(m, in.bytes, out_b.end())) != SNK_OK) return rc;
    if ((rc = stage_upload(m, in)) != SNK_OK) return rc;
    char *dev = m->q.as<char>(), *dout = m->out.as<char>(), *res = m->h_res.as<char>();
    SimpGraphView G   = graph_view(g);
    G.kf_bad          = in.at<const u8>(dev, i_bad);
    G.kf_pose         = in.at<const double>(dev, i_pose);
    G.kf_cull_factor  = in.at<const float>(dev, i_cf);
    G.kf_median_depth = in.at<const double>(dev, i_md);
    G.kf_prev         = nt ? in.at<const int32_t>(dev, i_prev) : nullptr;
    G.kf_next         = nt ? in.at<const int32_t>(dev, i_next) : nullptr;
    G.kf_time         = nt ? in.at<const double>(dev, i_time) : nullptr;
    G.conn_start      = in.at<const int32_t>(dev, i_cs);
    G.conn_list       = in.at<const SimpConn>(dev, i_cl);
    if ((rc = launch_decide(m, G, params, node_cap, n_q, in.at<const int>(dev, i_q), in.at<const SimpStats>(dev, i_st), out_b.at<SimpVerdict>(dout, o_res))) != SNK_OK)
        return rc;
    if ((rc = stage_download(m, 0, out_b.end())) != SNK_OK) return rc;
    memcpy(out, out_b.at<char>(res, o_res), ns * sizeof(SimpVerdict));
    return SNK_OK;
}

int snk_simp_decide_batch_dev(snk_matcher* m, const snk_simp_graph* graph_dev, const snk_simp_params* params, int node_cap, int n_q, const int32_t* q_dev,
                              const snk_simp_stats_result* stats_dev, snk_simp_verdict* out_dev)
{
    SNK_REQUIRE(m != nullptr, "NULL handle");
    int rc;
    if ((rc = check_graph_scalars(graph_dev, params, node_cap, n_q, q_dev, stats_dev, out_dev)) != SNK_OK) return rc;
    if (n_q == 0) return SNK_OK;
    SNK_HIP_CHECK(hipSetDevice(m->device));
    return launch_decide(m, graph_view(graph_dev), params, node_cap, n_q, q_dev, reinterpret_cast<const SimpStats*>(stats_dev),
                         reinterpret_cast<SimpVerdict*>(out_dev));
}
}
