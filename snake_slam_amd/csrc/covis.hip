// Covisibility for gfx950 ("snk-covis v1") — replaces, for many sets per call,
//   Keyframe::UpdateConnections                      (reference Snake/Map/Keyframe.cpp:89-171)
//   the vote of Tracking::UpdateLocalKeyFrames2      (reference Snake/Tracking/TrackingFine.cpp:230-268)
// The per-set statements are covis_core.hpp's; the long-list threshold and the carve are dispatch.hpp's.
//
// Mapping to the hardware.  covis_kernel: a workgroup of four wavefronts per set (a query keyframe or a frame); the two forms are the
// template's four switches.  The counters are u32 [n_kf] in LDS.  Count: a lane takes a feature, applies the gate and reads its point's
// list bounds; the lists are walked by walk_lists (wg.hpp: a short one by its lane, a long one by a wavefront) with LDS atomic adds.
// Integer adds commute: the counters do not depend on the order in which atomics land.  Emit: one pass over the counters applies the
// bad flags, the threshold and the arg-max (an LDS atomic max of count << 32 | ~id) and zeroes every counter that is not listed, so the
// later passes test count > 0 only.  More than cap listed: covis_cut builds the cap-th largest key bit by bit, one counting pass per
// bit (block_reduce, one barrier a pass).  The ids kept (a power of two of them, padded) are sorted in LDS by block_sort on the key
// count << 32 | id, which has no ties, so the compaction order (an atomic slot counter) does not show in the result.  No step is
// quadratic.  No scratch; every byte of LDS is in the dynamic carve (covis_carve).  The host entries check every table and upload it;
// the device entries launch the same kernel, which checks what the host could not see and answers SNK_COVIS_BAD_INDEX per set.
#include <cstddef>

#include "matcher_handle.hpp"

#include "covis_core.hpp"
#include "dispatch.hpp"
#include "wg.hpp"

namespace snk
{
namespace
{
using u8  = unsigned char;
using u32 = unsigned int;
using u64 = unsigned long long;

static_assert(sizeof(snk_covis_conn) == 8 && sizeof(CovisConn) == 8 && sizeof(snk_covis_result) == 16 && sizeof(CovisResult) == 16, "snk-covis layouts");
static_assert(COVIS_MAX_KF == SNK_COVIS_MAX_KF && COVIS_MAX_CAP == SNK_COVIS_MAX_CAP, "snk-covis limits");
static_assert(COVIS_OK == SNK_COVIS_OK && COVIS_UNCHANGED == SNK_COVIS_UNCHANGED && COVIS_BAD_INDEX == SNK_COVIS_BAD_INDEX &&
                  COVIS_PT_BAD == SNK_COVIS_PT_BAD && COVIS_PT_FAR == SNK_COVIS_PT_FAR,
              "snk-covis constants");
static_assert(covis_carve(COVIS_MAX_KF, COVIS_MAX_CAP) <= (size_t)LDS_MAX_BYTES, "LDS carve");
static_assert(COVIS_THREADS == 256 && COVIS_MISC >= 8 + 2 * (COVIS_THREADS / 64), "covis_kernel's words");

struct CovisCall
{
    int n_kf, n_points, n_obs, n_items, n_sets;
    int th, cap, long_min;
    float th_depth;
    const u8* kf_bad;
    const int* obs_start;
    const int2* obs;
    const u8* pt_flags;
    const int* item_start;   // feat_start [n_kf + 1] (indexed by the query) or set_start [n_sets + 1]
    const int* item_point;   // [n_items]
    const float* item_depth; // [n_items], connection form only
    const int* q;            // [n_sets] query keyframes; nullptr: the set is its own index into item_start
    CovisConn* conn;         // [n_sets][cap]
    CovisResult* out;        // [n_sets]
};

// words of s_misc
enum { W_BAD = 0, W_QUEUED = 1, W_TOUCHED = 2, W_FOUND = 3, W_SLOT = 4, W_MAXKEY = 6, W_PART = 8 };

template <bool GATE, bool SELF_EXCLUDED, bool BAD_FILTER, bool THRESHOLD>
__global__ __launch_bounds__(COVIS_THREADS) void covis_kernel(CovisCall c)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int sort_len = covis_sort_len(c.n_kf, c.cap);
    u32* s_cnt   = reinterpret_cast<u32*>(smem);                    // [n_kf rounded up to 4]
    u32* s_ids   = s_cnt + ((c.n_kf + 3) & ~3);                     // [sort_len]
    int* s_queue = reinterpret_cast<int*>(s_ids + sort_len);        // [COVIS_THREADS] points whose lists a wavefront walks
    u32* s_misc  = reinterpret_cast<u32*>(s_queue + COVIS_THREADS);  // [COVIS_MISC]
    const int tid = threadIdx.x, lane = tid & 63;
    const int set = blockIdx.x;

    for (int k = tid; k < c.n_kf; k += COVIS_THREADS) s_cnt[k] = 0;
    if (tid < COVIS_MISC) s_misc[tid] = 0;

    // ---- the set's items (uniform) ----
    int q = -1, first = 0, last = 0;
    bool bad = false;
    if (c.q)
    {
        q = c.q[set];
        if (q < 0 || q >= c.n_kf) bad = true;
        else first = c.item_start[q], last = c.item_start[q + 1];
    }
    else first = c.item_start[set], last = c.item_start[set + 1];
    if (!bad && (first < 0 || last < first || last > c.n_items)) bad = true;
    if (bad)
    {
        if (tid == 0) c.out[set] = covis_no_list(COVIS_BAD_INDEX);
        return;
    }
    __syncthreads();

    // ---- count ----
    auto add = [&](int o) {
        const int k = c.obs[o].x;
        if (k < 0 || k >= c.n_kf) s_misc[W_BAD] = 1;
        else if (covis_counts<SELF_EXCLUDED>(k, q)) atomicAdd(&s_cnt[k], 1u);
    };
    // the bounds of point p's list; false: outside obs
    auto list_of = [&](int p, int& a, int& b) {
        a = c.obs_start[p], b = c.obs_start[p + 1];
        return a >= 0 && b >= a && b <= c.n_obs;
    };
    walk_lists<COVIS_THREADS>(
        first, last, c.long_min, s_queue, &s_misc[W_QUEUED],
        [&](int i, int& p, int& a, int& b) {
            p = c.item_point[i];
            if (p < -1 || p >= c.n_points) return s_misc[W_BAD] = 1, false;
            if (p < 0 || !covis_gate<GATE>(c.pt_flags[p], GATE ? c.item_depth[i] : 0.0f, c.th_depth)) return false;
            if (!list_of(p, a, b)) return s_misc[W_BAD] = 1, false;
            return true;
        },
        [&](int, int a, int b) {
            for (int o = a; o < b; ++o) add(o);
        },
        [&](int p, int lane) {
            int la, lb;
            list_of(p, la, lb);  // checked when it was queued
            for (int o = la + lane; o < lb; o += 64) add(o);
        });
    __syncthreads();
    if (s_misc[W_BAD])  // uniform
    {
        if (tid == 0) c.out[set] = covis_no_list(COVIS_BAD_INDEX);
        return;
    }

    // ---- emit: bad flags, threshold, arg-max; afterwards listed <=> counter > 0 ----
    const u32 min_count = covis_min_count<THRESHOLD>(c.th);
    {
        int touched = 0, found = 0;
        u64 max_key = 0;
        for (int k = tid; k < c.n_kf; k += COVIS_THREADS)
        {
            const u32 n = s_cnt[k];
            if (n == 0) continue;
            touched += 1;
            const bool listable = covis_listable<BAD_FILTER>(BAD_FILTER ? c.kf_bad[k] : 0);
            if (listable)
            {
                const u64 mk = covis_max_key(n, (u32)k);
                max_key      = mk > max_key ? mk : max_key;
            }
            if (listable && n >= min_count) found += 1;
            else s_cnt[k] = 0;
        }
        touched = wave_sum_xor(touched);
        found   = wave_sum_xor(found);
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1)
        {
            const u64 other = __shfl_xor(max_key, s);
            max_key         = other > max_key ? other : max_key;
        }
        if (lane == 0)
        {
            atomicAdd(&s_misc[W_TOUCHED], (u32)touched);
            atomicAdd(&s_misc[W_FOUND], (u32)found);
            atomicMax(reinterpret_cast<u64*>(&s_misc[W_MAXKEY]), max_key);
        }
    }
    __syncthreads();
    const int touched = (int)s_misc[W_TOUCHED], n_found = (int)s_misc[W_FOUND];
    const u64 max_key = *reinterpret_cast<const u64*>(&s_misc[W_MAXKEY]);
    CovisConn* conn   = c.conn + (size_t)set * (size_t)c.cap;
    if (touched == 0 || n_found == 0)  // uniform
    {
        if (tid == 0)
        {
            if (touched == 0) c.out[set] = covis_no_list(COVIS_UNCHANGED);
            else if (max_key == 0) c.out[set] = covis_no_list(COVIS_OK);  // only bad keyframes touched
            else
            {
                const int id = (int)covis_max_key_id(max_key);
                conn[0]      = CovisConn{(int)(max_key >> 32), id};
                c.out[set]   = CovisResult{1, 1, id, COVIS_OK};
            }
        }
        return;
    }

    // ---- more than cap listed: the cap-th largest key ----
    u64 cut = 0;
    if (n_found > c.cap)  // uniform
    {
        int pass = 0;
        cut      = covis_cut(
            [&](u64 T) {
                u32 n = 0;
                for (int k = tid; k < c.n_kf; k += COVIS_THREADS)
                {
                    const u32 w = s_cnt[k];
                    n += w > 0 && covis_key(w, (u32)k) >= T ? 1u : 0u;
                }
                return (int)block_reduce<COVIS_THREADS>(n, [](u32 x, u32 y) { return x + y; }, s_misc + W_PART, pass);
            },
            c.cap, (u32)(max_key >> 32), c.n_kf);
    }
    const int n_conn = n_found < c.cap ? n_found : c.cap;
    int P = 4;  // the network's length
    while (P < n_conn) P <<= 1;
    P = P < sort_len ? P : sort_len;  // n_conn <= min(cap, n_kf) <= sort_len
    for (int i = tid; i < P; i += COVIS_THREADS) s_ids[i] = 0xFFFFFFFFu;
    __syncthreads();
    for (int k = tid; k < c.n_kf; k += COVIS_THREADS)
    {
        const u32 w = s_cnt[k];
        if (w > 0 && covis_key(w, (u32)k) >= cut)
        {
            const u32 slot = atomicAdd(&s_misc[W_SLOT], 1u);
            if (slot < (u32)P) s_ids[slot] = (u32)k;  // exactly n_conn of them
        }
    }
    __syncthreads();
    auto key_of = [&](u32 id) { return id == 0xFFFFFFFFu ? ~0ull : covis_key(s_cnt[id], id); };
    block_sort<COVIS_THREADS>(s_ids, P, [&](u32 x, u32 y) { return key_of(x) < key_of(y); });
    for (int i = tid; i < n_conn; i += COVIS_THREADS)
    {
        const u32 id = s_ids[i];
        conn[i]      = CovisConn{(int)s_cnt[id], (int)id};
    }
    if (tid == 0) c.out[set] = CovisResult{n_found, n_conn, (int)s_ids[n_conn - 1], COVIS_OK};
}

int long_env()
{
    // SNK_COVIS_LONG_MIN=<n> (tests, A/B): read once
    static const int env = [] {
        const char* s = getenv("SNK_COVIS_LONG_MIN");
        if (!s || !*s) return -1;
        char* end    = nullptr;
        const long v = strtol(s, &end, 10);
        return (*end || v < 0 || v > 0x7FFFFFFFL) ? -1 : (int)v;
    }();
    return env;
}

int check_scalars(const snk_covis_map* map, const snk_covis_params* params)
{
    SNK_REQUIRE(map != nullptr && params != nullptr, "covisibility: map or params is NULL");
    SNK_REQUIRE(map->n_kf >= 0 && map->n_points >= 0 && map->n_obs >= 0, "covisibility: negative count");
    SNK_REQUIRE(map->n_kf <= SNK_COVIS_MAX_KF, "covisibility: n_kf above SNK_COVIS_MAX_KF (32768)");
    SNK_REQUIRE(params->cap >= 1 && params->cap <= SNK_COVIS_MAX_CAP, "covisibility: cap outside [1, SNK_COVIS_MAX_CAP]");
    SNK_REQUIRE(params->th >= 1, "covisibility: th < 1");
    SNK_REQUIRE(map->n_kf == 0 || map->kf_bad != nullptr, "covisibility: NULL kf_bad with n_kf > 0");
    SNK_REQUIRE(map->obs_start != nullptr, "covisibility: NULL obs_start");
    SNK_REQUIRE(map->n_points == 0 || map->pt_flags != nullptr, "covisibility: NULL pt_flags with n_points > 0");
    SNK_REQUIRE(map->n_obs == 0 || map->obs != nullptr, "covisibility: NULL obs with n_obs > 0");
    return SNK_OK;
}

// the host's look at the map: everything the kernel would otherwise have to refuse
int check_map(const snk_covis_map* map)
{
    int rc;
    if ((rc = check_starts(map->obs_start, map->n_points, "covisibility: obs_start[0] must be 0", "covisibility: obs_start must be non-decreasing")) != SNK_OK) return rc;
    SNK_REQUIRE(map->obs_start[map->n_points] == map->n_obs, "covisibility: obs_start[n_points] must be n_obs");
    for (int o = 0; o < map->n_obs; ++o) SNK_REQUIRE(map->obs[o][0] >= 0 && map->obs[o][0] < map->n_kf, "covisibility: an observation's keyframe outside [0, n_kf)");
    return SNK_OK;
}

int check_items(const int32_t* start, int n_starts, const int32_t* point, int n_points)
{
    int rc;
    if ((rc = check_starts(start, n_starts, "covisibility: a start array must begin at 0", "covisibility: a start array must be non-decreasing")) != SNK_OK) return rc;
    SNK_REQUIRE(start[n_starts] == 0 || point != nullptr, "covisibility: NULL point array with entries");
    for (int i = 0; i < start[n_starts]; ++i) SNK_REQUIRE(point[i] >= -1 && point[i] < n_points, "covisibility: a point id outside [-1, n_points)");
    return SNK_OK;
}

template <bool CONN>
int launch(snk_matcher* m, const CovisCall& C)
{
    auto kernel        = covis_kernel<CONN, CONN, CONN, CONN>;
    const size_t carve = covis_carve(C.n_kf, C.cap);
    int rc;
    if ((rc = set_max_lds_once(reinterpret_cast<const void*>(kernel), (int)covis_carve(COVIS_MAX_KF, COVIS_MAX_CAP))) != SNK_OK) return rc;
    hipLaunchKernelGGL(kernel, dim3(C.n_sets), dim3(COVIS_THREADS), carve, m->stream, C);
    SNK_LAUNCH_CHECK();
    return SNK_OK;
}

CovisCall make_call(const snk_covis_map* map, const snk_covis_params* params, int n_sets, int n_items)
{
    CovisCall C{};
    C.n_kf      = map->n_kf;
    C.n_points  = map->n_points;
    C.n_obs     = map->n_obs;
    C.n_items   = n_items;
    C.n_sets    = n_sets;
    C.th        = params->th;
    C.th_depth  = params->th_depth;
    C.cap       = params->cap;
    C.long_min  = covis_long_min(long_env());
    C.kf_bad    = map->kf_bad;
    C.obs_start = map->obs_start;
    C.obs       = reinterpret_cast<const int2*>(map->obs);
    C.pt_flags  = map->pt_flags;
    return C;
}

// The host entries: the tables go up as one block, the lists come back as one; conn[set] receives its n_conn entries only.
// items: feat_* of the connection form (n_starts = n_kf, q given) or set_* of the vote (n_starts = n_sets, q = nullptr)
template <bool CONN>
int run_host(snk_matcher* m, const snk_covis_map* map, const snk_covis_params* params, int n_starts, const int32_t* start, const int32_t* point,
             const float* depth, int n_sets, const int32_t* q, snk_covis_conn* conn, snk_covis_result* out)
{
    const size_t n_kf = (size_t)map->n_kf, n_pts = (size_t)map->n_points, n_obs = (size_t)map->n_obs, n_items = (size_t)start[n_starts],
                 ns = (size_t)n_sets, cap = (size_t)params->cap;
    // one upload (stage.hpp): kf_bad | pt_flags | obs_start | obs | start | point | depth | q, the last two empty in the vote
    Block in, out_b;
    const int i_bad = in.add(map->kf_bad, n_kf), i_flags = in.add(map->pt_flags, n_pts), i_ostart = in.add(map->obs_start, (n_pts + 1) * 4),
              i_obs = in.add(map->obs, n_obs * 8), i_start = in.add(start, ((size_t)n_starts + 1) * 4), i_point = in.add(point, n_items * 4),
              i_depth = in.add(depth, CONN ? n_items * 4 : 0), i_q = in.add(q, CONN ? ns * 4 : 0);
    const int o_conn = out_b.add(nullptr, ns * cap * sizeof(CovisConn)), o_res = out_b.add(nullptr, ns * sizeof(CovisResult));
    int rc;
    SNK_HIP_CHECK(hipSetDevice(m->device));
    if ((rc = stage_reserve(m, in.bytes, out_b.end())) != SNK_OK) return rc;
    if ((rc = stage_upload(m, in)) != SNK_OK) return rc;
    char *dev = m->q.as<char>(), *dout = m->out.as<char>(), *res = m->h_res.as<char>();
    CovisCall C  = make_call(map, params, n_sets, (int)n_items);
    C.kf_bad     = in.at<const u8>(dev, i_bad);
    C.pt_flags   = in.at<const u8>(dev, i_flags);
    C.obs_start  = in.at<const int>(dev, i_ostart);
    C.obs        = in.at<const int2>(dev, i_obs);
    C.item_start = in.at<const int>(dev, i_start);
    C.item_point = in.at<const int>(dev, i_point);
    C.item_depth = CONN ? in.at<const float>(dev, i_depth) : nullptr;
    C.q          = CONN ? in.at<const int>(dev, i_q) : nullptr;
    C.conn       = out_b.at<CovisConn>(dout, o_conn);
    C.out        = out_b.at<CovisResult>(dout, o_res);
    if ((rc = launch<CONN>(m, C)) != SNK_OK) return rc;
    if ((rc = stage_download(m, 0, out_b.end())) != SNK_OK) return rc;
    memcpy(out, out_b.at<char>(res, o_res), ns * sizeof(CovisResult));
    const CovisConn* lists = out_b.at<const CovisConn>(res, o_conn);
    for (size_t s = 0; s < ns; ++s)
        if (out[s].n_conn > 0) memcpy(conn + s * cap, lists + s * cap, (size_t)out[s].n_conn * sizeof(CovisConn));
    return SNK_OK;
}
}  // namespace
}  // namespace snk

using namespace snk;

extern "C" {
int snk_covis_update(snk_matcher* m, const snk_covis_map* map, const int32_t* feat_start, const int32_t* feat_point, const float* feat_depth,
                     const snk_covis_params* params, int n_q, const int32_t* q, snk_covis_conn* conn, snk_covis_result* out)
{
    SNK_REQUIRE(m != nullptr, "NULL handle");
    int rc;
    if ((rc = check_scalars(map, params)) != SNK_OK) return rc;
    SNK_REQUIRE(n_q >= 0, "covisibility: negative query count");
    SNK_REQUIRE(feat_start != nullptr, "covisibility: NULL feat_start");
    if ((rc = check_map(map)) != SNK_OK) return rc;
    if ((rc = check_items(feat_start, map->n_kf, feat_point, map->n_points)) != SNK_OK) return rc;
    SNK_REQUIRE(feat_start[map->n_kf] == 0 || feat_depth != nullptr, "covisibility: NULL feat_depth with features");
    if (n_q == 0) return SNK_OK;
    SNK_REQUIRE(q != nullptr && conn != nullptr && out != nullptr, "covisibility: NULL array with n_q > 0");
    for (int i = 0; i < n_q; ++i) SNK_REQUIRE(q[i] >= 0 && q[i] < map->n_kf, "covisibility: a query outside [0, n_kf)");
    return run_host<true>(m, map, params, map->n_kf, feat_start, feat_point, feat_depth, n_q, q, conn, out);
}

int snk_covis_update_batch_dev(snk_matcher* m, const snk_covis_map* map_dev, const int32_t* feat_start_dev, int n_feat, const int32_t* feat_point_dev,
                               const float* feat_depth_dev, const snk_covis_params* params, int n_q, const int32_t* q_dev, snk_covis_conn* conn_dev,
                               snk_covis_result* out_dev)
{
    SNK_REQUIRE(m != nullptr, "NULL handle");
    int rc;
    if ((rc = check_scalars(map_dev, params)) != SNK_OK) return rc;
    SNK_REQUIRE(n_q >= 0 && n_feat >= 0, "covisibility: negative count");
    SNK_REQUIRE(feat_start_dev != nullptr, "covisibility: NULL feat_start");
    SNK_REQUIRE(n_feat == 0 || (feat_point_dev != nullptr && feat_depth_dev != nullptr), "covisibility: NULL feature array with n_feat > 0");
    if (n_q == 0) return SNK_OK;
    SNK_REQUIRE(q_dev != nullptr && conn_dev != nullptr && out_dev != nullptr, "covisibility: NULL array with n_q > 0");
    SNK_HIP_CHECK(hipSetDevice(m->device));
    CovisCall C  = make_call(map_dev, params, n_q, n_feat);
    C.item_start = feat_start_dev;
    C.item_point = feat_point_dev;
    C.item_depth = feat_depth_dev;
    C.q          = q_dev;
    C.conn       = reinterpret_cast<CovisConn*>(conn_dev);
    C.out        = reinterpret_cast<CovisResult*>(out_dev);
    return launch<true>(m, C);
}

int snk_covis_vote(snk_matcher* m, const snk_covis_map* map, int n_sets, const int32_t* set_start, const int32_t* set_point,
                   const snk_covis_params* params, snk_covis_conn* conn, snk_covis_result* out)
{
    SNK_REQUIRE(m != nullptr, "NULL handle");
    int rc;
    if ((rc = check_scalars(map, params)) != SNK_OK) return rc;
    SNK_REQUIRE(n_sets >= 0, "covisibility: negative set count");
    if ((rc = check_map(map)) != SNK_OK) return rc;
    if (n_sets == 0) return SNK_OK;
    SNK_REQUIRE(set_start != nullptr && conn != nullptr && out != nullptr, "covisibility: NULL array with n_sets > 0");
    if ((rc = check_items(set_start, n_sets, set_point, map->n_points)) != SNK_OK) return rc;
    return run_host<false>(m, map, params, n_sets, set_start, set_point, nullptr, n_sets, nullptr, conn, out);
}

int snk_covis_vote_batch_dev(snk_matcher* m, const snk_covis_map* map_dev, int n_sets, const int32_t* set_start_dev, int n_set_points,
                             const int32_t* set_point_dev, const snk_covis_params* params, snk_covis_conn* conn_dev, snk_covis_result* out_dev)
{
    SNK_REQUIRE(m != nullptr, "NULL handle");
    int rc;
    if ((rc = check_scalars(map_dev, params)) != SNK_OK) return rc;
    SNK_REQUIRE(n_sets >= 0 && n_set_points >= 0, "covisibility: negative count");
    if (n_sets == 0) return SNK_OK;
    SNK_REQUIRE(set_start_dev != nullptr && conn_dev != nullptr && out_dev != nullptr, "covisibility: NULL array with n_sets > 0");
    SNK_REQUIRE(n_set_points == 0 || set_point_dev != nullptr, "covisibility: NULL set_point with n_set_points > 0");
    SNK_HIP_CHECK(hipSetDevice(m->device));
    CovisCall C  = make_call(map_dev, params, n_sets, n_set_points);
    C.item_start = set_start_dev;
    C.item_point = set_point_dev;
    C.conn       = reinterpret_cast<CovisConn*>(conn_dev);
    C.out        = reinterpret_cast<CovisResult*>(out_dev);
    return launch<false>(m, C);
}
}
