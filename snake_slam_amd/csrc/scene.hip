// Local BA windows for gfx950 ("snk-scene v1") — replaces, for many keyframes per call,
//   LocalBundleAdjustment::MakeLocalScene, the window  (reference Snake/Optimizer/LocalBundleAdjustment.cpp:124-151)   scene_window_kernel
//   ... the points, the images, the observations, the constraints (:154-346)                                           scene_gather_kernel
// The per-item statements are scene_core.hpp's; the carves and the table sizes are dispatch.hpp's.
//
// Mapping to the hardware.  A workgroup per query, every byte of LDS in the dynamic carve, no scratch.
//
// scene_window_kernel.  One wavefront, a lane per candidate (at most 64): the neighbours are copied from the back of the query's
// connections, lane 0 walks the previous-keyframe chain (at most n_last dependent loads), a lane compares its candidate with the
// earlier ones (:142) and ranks the survivors by counting the smaller ones (:151).
//
// scene_gather_kernel.  Four wavefronts, one carve used twice.
//   Points: the first-appearance table of wg.hpp over the concatenated feature ranges of the window, the id recovered through
//   feat_point, a slot of the same id taking a plain atomic minimum.  The point list goes to the pt_id row, which is this kernel's work
//   list from here on (and is -1 again if the query fails later).
//   The walk: the observation stream of the points in order.  256 points per chunk, block_scan_long over their list lengths; 256 stream
//   items per sub-chunk, a lane finds its point by last_at_most.  Its ordinal is the position in the stream.
//   Walk 1, fixed cameras: a keyframe that is neither bad nor in the window (binary search of the 64 window keyframes) goes into an
//   open-addressing table of (kf + 1, minimum ordinal): claim by compare-and-swap, atomic minimum.  The minima are distinct, so sorting
//   them (bitonic, LDS) and looking one up again is the order of first appearance; the slot's value becomes the image index.
//   Walk 2, counts: a record adds 1 to its image's counter; a scan over the images turns the counters into bases.
//   Walk 3, records: the images of a sub-chunk's records stand in LDS, a lane counts the equal ones before it (a compare loop, every
//   lane reads the same word), writes at base + rank, and then adds itself to the base for the next sub-chunk.  No result depends on
//   the order in which atomics land: the tables' contents as sets do not, and ranks never come from an atomic's return value.
// Every probe loop ends after `slots` steps, every search after log2 steps, the chain after n_last; no lane waits for another.
//
// The host entries lay the arrays of a call out as one block, inputs and outputs alike: stage.hpp, and matcher_handle.hpp for the copies.
#include <cstddef>

#include "matcher_handle.hpp"

#include "scene_core.hpp"
#include "dispatch.hpp"
#include "wg.hpp"

namespace snk
{
namespace
{
using u8  = unsigned char;
using u32 = unsigned int;
using u64 = unsigned long long;

static_assert(sizeof(snk_scene_window_result) == 8 && sizeof(SceneWindowResult) == 8 && sizeof(snk_scene_result) == 24 && sizeof(SceneResult) == 24 &&
                  sizeof(snk_ba_rpc) == 80 && sizeof(snk_covis_conn) == 8,
              "snk-scene layouts");
static_assert(SCENE_MAX_WINDOW == SNK_SCENE_MAX_WINDOW && SCENE_MAX_IMG == SNK_SCENE_MAX_IMG && SCENE_MAX_OBS == SNK_SCENE_MAX_OBS, "snk-scene limits");
static_assert(SCENE_OK == SNK_SCENE_OK && SCENE_SKIPPED == SNK_SCENE_SKIPPED && SCENE_WINDOW_OVERFLOW == SNK_SCENE_WINDOW_OVERFLOW &&
                  SCENE_PTS_OVERFLOW == SNK_SCENE_PTS_OVERFLOW && SCENE_IMG_OVERFLOW == SNK_SCENE_IMG_OVERFLOW && SCENE_OBS_OVERFLOW == SNK_SCENE_OBS_OVERFLOW &&
                  SCENE_BAD_INDEX == SNK_SCENE_BAD_INDEX && SCENE_PT_BAD == SNK_COVIS_PT_BAD && SCENE_PT_CONST == SNK_SCENE_PT_CONST,
              "snk-scene constants");
static_assert(scene_gather_carve(LMAP_MAX_PTS, SCENE_MAX_IMG) <= (size_t)LDS_MAX_BYTES && scene_window_carve() <= (size_t)LDS_MAX_BYTES, "LDS carves of scene.hip");
static_assert(SCENE_THREADS == 256 && SCENE_WIN_THREADS == 64 && SCENE_MAX_WINDOW <= SCENE_WIN_THREADS && SCENE_MAX_WINDOW <= SCENE_WIN_SLOTS && SCENE_MISC >= 16,
              "a lane per candidate; the words of s_misc");
static_assert(scene_img_slots(SCENE_MAX_IMG) >= SCENE_MAX_IMG + SCENE_THREADS && scene_img_slots(1) >= 1 + SCENE_THREADS && scene_sort_len(SCENE_MAX_IMG) >= SCENE_MAX_IMG,
              "room for the claims in flight");

// words of s_misc
enum { W_BAD = 0, W_FULL = 1, W_COUNT = 2, W_NFIX = 3, W_NRPC = 4, W_PART = 8 };

struct WindowCall
{
    int n_q, n_kf, n_list, n_neighbours, n_last, win_cap;
    const int* q;
    const u8* kf_bad;
    const int* kf_prev;
    const int* conn_start;
    const int2* conn_list;  // (weight, kf)
    int* window_kf;         // [n_q][win_cap]
    SceneWindowResult* out;
};

struct GatherCall
{
    int n_q, use_imu;
    double gyro_weight, acc_weight;
    snk_scene_map map;
    const int* window_kf;
    const SceneWindowResult* win;
    snk_scene_out out;
};

__global__ __launch_bounds__(SCENE_WIN_THREADS) void scene_window_kernel(WindowCall c)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* s_cand   = reinterpret_cast<int*>(smem);  // [SCENE_WIN_SLOTS] the candidates, then the survivors (-1: dropped)
    int* s_misc   = s_cand + SCENE_WIN_SLOTS;      // [4] chain length, chain flag
    const int tid = threadIdx.x;
    const int set = blockIdx.x;
    int* row      = c.window_kf + (size_t)set * (size_t)c.win_cap;

    auto finish = [&](int status) {  // uniform
        for (int i = tid; i < c.win_cap; i += SCENE_WIN_THREADS) row[i] = -1;
        if (tid == 0) c.out[set] = scene_no_window(status);
    };

    const int q = c.q[set];
    if (q < 0 || q >= c.n_kf)
    {
        finish(SCENE_BAD_INDEX);
        return;
    }
    if (c.kf_bad[q])  // :77
    {
        finish(SCENE_SKIPPED);
        return;
    }
    const int a = c.conn_start[q], b = c.conn_start[q + 1];
    if (a < 0 || b < a || b > c.n_list)
    {
        finish(SCENE_BAD_INDEX);
        return;
    }
    const int cnt = scene_n_neighbours_taken(c.n_neighbours, b - a);  // the last cnt entries, ascending (KeyframeGraph.cpp:62)
    bool bad = false;
    if (tid < cnt)
    {
        const int nb = c.conn_list[b - cnt + tid].y;
        if (nb < 0 || nb >= c.n_kf) bad = true;
        s_cand[tid] = nb;
    }
    if (tid == cnt) s_cand[cnt] = q;
    if (tid == 0)  // :131-135
    {
        int n = 0, k = c.kf_prev[q];
        bool chain_bad = false;
        for (int i = 0; i < c.n_last && k != -1; ++i)
        {
            if (k < -1 || k >= c.n_kf)
            {
                chain_bad = true;
                break;
            }
            s_cand[cnt + 1 + n] = k;
            n += 1;
            k = c.kf_prev[k];
        }
        s_misc[0] = n;
        s_misc[1] = chain_bad ? 1 : 0;
    }
    __syncthreads();
    if (__any(bad) || s_misc[1])  // uniform
    {
        finish(SCENE_BAD_INDEX);
        return;
    }
    const int n_cand = cnt + 1 + s_misc[0];  // <= SCENE_MAX_WINDOW: checked on the host
    int k            = -1;
    bool survives    = false;
    if (tid < n_cand)
    {
        k            = s_cand[tid];
        bool earlier = false;
        for (int j = 0; j < tid; ++j) earlier = earlier || s_cand[j] == k;
        survives = scene_candidate_survives(c.kf_bad[k], earlier);
    }
    __syncthreads();
    s_cand[tid] = survives ? k : -1;
    __syncthreads();
    const int n_window = __popcll(__ballot(survives));
    if (n_window > c.win_cap)
    {
        finish(SCENE_WINDOW_OVERFLOW);
        return;
    }
    if (survives)
    {
        int rank = 0;
        for (int j = 0; j < n_cand; ++j) rank += (s_cand[j] >= 0 && s_cand[j] < k) ? 1 : 0;
        row[rank] = k;
    }
    for (int i = n_window + tid; i < c.win_cap; i += SCENE_WIN_THREADS) row[i] = -1;
    if (tid == 0) c.out[set] = SceneWindowResult{n_window, SCENE_OK};
}

__global__ __launch_bounds__(SCENE_THREADS) void scene_gather_kernel(GatherCall c)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const snk_scene_map& M = c.map;
    const snk_scene_out& O = c.out;
    int* s_win  = reinterpret_cast<int*>(smem);                       // [SCENE_WIN_SLOTS] the window keyframes
    u32* s_misc = reinterpret_cast<u32*>(s_win + SCENE_WIN_SLOTS);    // [SCENE_MISC]
    u32* region = s_misc + SCENE_MISC;
    // phase 1
    const int n_slots = lmap_table_slots(O.pt_cap);
    u32* s_tab    = region;                                            // [n_slots] order + 1; 0 = free
    int* s_prefix = reinterpret_cast<int*>(s_tab + n_slots);           // [SCENE_WIN_SLOTS + 1] first order of a window keyframe's features
    int* s_fstart = s_prefix + SCENE_WIN_SLOTS + 1;                    // [SCENE_WIN_SLOTS] its feat_start
    // phase 2
    const int S     = scene_img_slots(O.img_cap);
    const u32 smask = (u32)S - 1u;
    u32* s_key    = region;                                            // [S] kf + 1; 0 = free
    u32* s_val    = s_key + S;                                         // [S] minimum ordinal, then the image index
    u32* s_sort   = s_val + S;                                         // [scene_sort_len(img_cap)]
    u32* s_base   = s_sort + scene_sort_len(O.img_cap);                // [img_cap] records of an image, then its running base
    int* s_pstart = reinterpret_cast<int*>(s_base + O.img_cap);        // [SCENE_THREADS + 1] a chunk's points: first stream item
    int* s_ostart = s_pstart + SCENE_THREADS + 1;                      // [SCENE_THREADS] obs_start
    int* s_pinfo  = s_ostart + SCENE_THREADS;                          // [SCENE_THREADS] point id
    int* s_cimg   = s_pinfo + SCENE_THREADS;                           // [SCENE_THREADS] a sub-chunk's records: image, -1 = none

    const int tid = threadIdx.x;
    const int set = blockIdx.x;
    int* ids      = O.pt_id + (size_t)set * (size_t)O.pt_cap;
    int pass      = 0;

    auto finish = [&](int status) {  // uniform
        for (int i = tid; i < O.pt_cap; i += SCENE_THREADS) ids[i] = -1;
        if (tid == 0) reinterpret_cast<SceneResult*>(O.result)[set] = scene_no_scene(status);
    };

    const SceneWindowResult wr = c.win[set];
    const int win_status       = scene_window_status(wr.status, wr.n_window, O.win_cap);
    if (win_status != SCENE_OK)
    {
        finish(win_status);
        return;
    }
    const int nw = wr.n_window;
    for (int i = tid; i < n_slots; i += SCENE_THREADS) s_tab[i] = 0;
    if (tid < SCENE_MISC) s_misc[tid] = 0;
    __syncthreads();

    // ---- the window: strictly ascending, in range; order numbers by a prefix sum over the feature ranges ----
    int len = 0;
    if (tid < nw)
    {
        const int* wrow = c.window_kf + (size_t)set * (size_t)O.win_cap;
        const int k     = wrow[tid];
        if (k < 0 || k >= M.n_kf || (tid > 0 && wrow[tid - 1] >= k)) s_misc[W_BAD] = 1;
        else
        {
            s_win[tid]  = k;
            const int a = M.feat_start[k], b = M.feat_start[k + 1];
            if (a < 0 || b < a || b > M.n_feat || b - a > LMAP_MAX_ORDER) s_misc[W_BAD] = 1;
            else len = b - a, s_fstart[tid] = a;
        }
    }
    long long T64;
    const long long ex = block_scan_long<SCENE_THREADS>(len, T64, s_misc + W_PART, pass);
    if (T64 > LMAP_MAX_ORDER || s_misc[W_BAD])  // uniform: the scans' barriers are behind the writes of W_BAD
    {
        finish(SCENE_BAD_INDEX);
        return;
    }
    const int T = (int)T64;
    if (tid < nw) s_prefix[tid] = (int)ex;
    if (tid == 0) s_prefix[nw] = T;
    __syncthreads();

    auto id_of = [&](int ord) {
        const int li = last_at_most(s_prefix, nw, ord);
        return M.feat_point[s_fstart[li] + (ord - s_prefix[li])];
    };
    auto load = [&](const u32* w) { return __atomic_load_n(w, __ATOMIC_RELAXED); };

    // ---- points (:154-167): build ----
    for (int li = 0; li < nw; ++li)  // uniform
    {
        const int a = s_fstart[li], first = s_prefix[li], n = s_prefix[li + 1] - first;
        for (int f = tid; f < n; f += SCENE_THREADS)
        {
            const int p = M.feat_point[a + f];
            if (p < -1 || p >= M.n_points) s_misc[W_BAD] = 1;
            else if (!scene_point_skipped(p, p >= 0 ? M.pt_flags[p] : 0))
            {
                u32 seen;
                const int slot = table_place(s_tab, n_slots, p, first + f, O.pt_cap, &s_misc[W_COUNT], &s_misc[W_FULL], seen, id_of);
                if (slot >= 0 && seen != 0) atomicMin(&s_tab[slot], (u32)(first + f) + 1u);
            }
        }
    }
    __syncthreads();
    if (s_misc[W_BAD] || s_misc[W_FULL])  // uniform; the range checks first
    {
        finish(s_misc[W_BAD] ? SCENE_BAD_INDEX : SCENE_PTS_OVERFLOW);
        return;
    }
    // ---- points: emit ----
    const int n_pt = table_emit<SCENE_THREADS>(
        s_tab, n_slots, T, O.pt_cap, s_misc + W_PART, pass, id_of, [&](int, int p) { return !scene_point_skipped(p, p >= 0 ? M.pt_flags[p] : 0); },
        [&](int, int p, int rank, u32) { ids[rank] = p; });
    __syncthreads();  // the table is read no more; the point list is in ids

    // ---- the carve again: the fixed-camera table, the bases ----
    for (int i = tid; i < S; i += SCENE_THREADS) s_key[i] = 0, s_val[i] = 0xFFFFFFFFu;
    for (int i = tid; i < O.img_cap; i += SCENE_THREADS) s_base[i] = 0;
    if (tid == 0) s_misc[W_COUNT] = 0;
    __syncthreads();

    auto window_index = [&](int kf) {  // the image of a window keyframe, -1: not in the window
        int lo = 0, hi = nw;
        while (lo < hi)
        {
            const int mid = (lo + hi) >> 1;
            if (s_win[mid] < kf) lo = mid + 1;
            else hi = mid;
        }
        return lo < nw && s_win[lo] == kf ? lo : -1;
    };
    auto image_of = [&](int kf) {  // after the sort: the image of a keyframe that is not bad
        const int w = window_index(kf);
        if (w >= 0) return w;
        u32 slot = lmap_hash(kf) & smask;
        for (int probe = 0; probe < S; ++probe, slot = (slot + 1) & smask)
        {
            const u32 key = s_key[slot];
            if (key == (u32)kf + 1u) return (int)s_val[slot];
            if (key == 0) break;  // cannot happen: walk 1 placed every such keyframe
        }
        return -1;
    };

    // The walk.  f(active, j, p, pos, ordinal) is called by every lane of the workgroup together (it may hold barriers): item `ordinal` of
    // the stream is observation `pos` of point p, the j-th of the list.  Returns false when a start is out of range or the stream too long.
    auto walk = [&](auto&& f) -> bool {
        long long walk_base = 0;
        for (int pbase = 0; pbase < n_pt; pbase += SCENE_THREADS)  // uniform
        {
            const int j = pbase + tid;
            int plen = 0, p = -1;
            bool bad = false;
            if (j < n_pt)
            {
                p           = ids[j];
                const int a = M.obs_start[p], b = M.obs_start[p + 1];
                if (a < 0 || b < a || b > M.n_obs || b - a > SCENE_MAX_WALK) bad = true;
                else plen = b - a, s_ostart[tid] = a;
            }
            s_pinfo[tid] = p;
            if (bad) s_misc[W_BAD] = 1;
            long long L;
            const long long ex = block_scan_long<SCENE_THREADS>(plen, L, s_misc + W_PART, pass);
            if (s_misc[W_BAD] || walk_base + L > SCENE_MAX_WALK) return false;  // uniform
            s_pstart[tid] = (int)ex;
            if (tid == 0) s_pstart[SCENE_THREADS] = (int)L;
            __syncthreads();
            for (int sbase = 0; sbase < (int)L; sbase += SCENE_THREADS)  // uniform
            {
                const int i       = sbase + tid;
                const bool active = i < (int)L;
                const int lo      = active ? last_at_most(s_pstart, SCENE_THREADS, i) : 0;
                f(active, pbase + lo, active ? s_pinfo[lo] : -1, active ? s_ostart[lo] + (i - s_pstart[lo]) : 0, (int)walk_base + i);
            }
            walk_base += L;
            __syncthreads();  // the chunk's words are written again
        }
        return true;
    };

    // ---- walk 1 (:170-184): the range checks, the fixed cameras with their minimum ordinals ----
    const int fixed_cap = O.img_cap - nw;
    const bool ok1      = walk([&](bool active, int, int, int pos, int ordinal) {
        if (!active) return;
        const int kf = M.obs[pos][0], fi = M.obs[pos][1];
        if (kf < 0 || kf >= M.n_kf)
        {
            s_misc[W_BAD] = 1;
            return;
        }
        const int fa = M.feat_start[kf], fb = M.feat_start[kf + 1];
        if (fa < 0 || fb < fa || fb > M.n_feat || fi < 0 || fi >= fb - fa)
        {
            s_misc[W_BAD] = 1;
            return;
        }
        const int oct = M.feat_octave[fa + fi];
        if (oct < 0 || oct >= M.n_levels)
        {
            s_misc[W_BAD] = 1;
            return;
        }
        if (M.kf_bad[kf] || window_index(kf) >= 0 || load(&s_misc[W_FULL])) return;
        u32 slot = lmap_hash(kf) & smask;
        for (int probe = 0; probe < S; ++probe, slot = (slot + 1) & smask)
        {
            u32 key = load(&s_key[slot]);
            if (key == 0)
            {
                key = atomicCAS(&s_key[slot], 0u, (u32)kf + 1u);
                if (key == 0)
                {
                    if ((int)atomicAdd(&s_misc[W_COUNT], 1u) + 1 > fixed_cap) s_misc[W_FULL] = 1;
                    key = (u32)kf + 1u;
                }
            }
            if (key == (u32)kf + 1u)
            {
                atomicMin(&s_val[slot], (u32)ordinal);
                return;
            }
        }
        s_misc[W_FULL] = 1;
    });
    __syncthreads();
    if (!ok1 || s_misc[W_BAD])  // uniform
    {
        finish(SCENE_BAD_INDEX);
        return;
    }
    if (nw > O.img_cap || s_misc[W_FULL])
    {
        finish(SCENE_IMG_OVERFLOW);
        return;
    }
    // ---- the order of the fixed cameras: their minimum ordinals (distinct) sorted ----
    for (int i = tid; i < S; i += SCENE_THREADS)
        if (s_key[i] != 0) s_sort[atomicAdd(&s_misc[W_NFIX], 1u)] = s_val[i];  // as a set; the sort follows
    __syncthreads();
    const int n_fixed = (int)s_misc[W_NFIX];
    const int n_img   = nw + n_fixed;
    const int Pn      = lmap_pow2_at_least(n_fixed, 4);  // <= scene_sort_len(img_cap)
    for (int i = n_fixed + tid; i < Pn; i += SCENE_THREADS) s_sort[i] = 0xFFFFFFFFu;
    __syncthreads();
    // The network of wg.hpp's block_sort in its `i ^ j` shape, kept inline: with every block of this kernel shared, the gather call of
    // tools/probes/scene_timing.py measured 0.9 % slower than before (profiles/NOTES.md); with this one inline it does not.
    for (int k2 = 2; k2 <= Pn; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1)
        {
            for (int i = tid; i < Pn; i += SCENE_THREADS)
            {
                const int l = i ^ j;
                if (l > i)
                {
                    const u32 x = s_sort[i], y = s_sort[l];
                    const bool up = (i & k2) == 0;
                    if ((x > y) == up) s_sort[i] = y, s_sort[l] = x;
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < S; i += SCENE_THREADS)
        if (s_key[i] != 0)
        {
            const u32 v = s_val[i];
            int lo = 0, hi = n_fixed;  // the first entry >= v is v itself
            while (lo < hi)
            {
                const int mid = (lo + hi) >> 1;
                if (s_sort[mid] < v) lo = mid + 1;
                else hi = mid;
            }
            s_val[i] = (u32)(nw + lo);
        }
    __syncthreads();

    // ---- walk 2: the records of every image ----
    walk([&](bool active, int, int p, int pos, int) {
        if (!active) return;
        const int kf = M.obs[pos][0];
        if (M.kf_bad[kf]) return;
        const int img = image_of(kf);
        if (img >= 0 && !scene_record_skipped(0, img >= nw, scene_point_constant(M.pt_flags[p]))) atomicAdd(&s_base[img], 1u);
    });
    __syncthreads();
    int n_obs = 0;
    for (int base = 0; base < n_img; base += SCENE_THREADS)  // uniform
    {
        const int i = base + tid;
        const int v = i < n_img ? (int)s_base[i] : 0;  // <= 2^30 in all
        int total;
        const int ex = block_scan<SCENE_THREADS>(v, total, s_misc + W_PART, pass);
        if (i < n_img) s_base[i] = (u32)(n_obs + ex);
        n_obs += total;
    }
    if (n_obs > O.obs_cap)
    {
        finish(SCENE_OBS_OVERFLOW);
        return;
    }
    __syncthreads();

    // ---- the scene is known to fit: images (:200-244), world points (:246-254), constraints (:295-346) ----
    {
        int* img_kf  = O.img_kf + (size_t)set * (size_t)O.img_cap;
        u64* pose    = reinterpret_cast<u64*>(O.pose) + (size_t)set * (size_t)O.img_cap * 7;
        u8* img_c    = O.img_const + (size_t)set * (size_t)O.img_cap;
        const u64* src = reinterpret_cast<const u64*>(M.kf_pose);
        auto image = [&](int idx, int kf, u8 constant) {
            img_kf[idx] = kf;
            img_c[idx]  = constant;
#pragma unroll
            for (int e = 0; e < 7; ++e) pose[(size_t)idx * 7 + e] = src[(size_t)kf * 7 + e];
        };
        if (tid < nw) image(tid, s_win[tid], 0);
        for (int i = tid; i < S; i += SCENE_THREADS)
            if (s_key[i] != 0) image((int)s_val[i], (int)s_key[i] - 1, 1);
    }
    u8* pt_valid = O.pt_valid + (size_t)set * (size_t)O.pt_cap;
    {
        u64* pt        = reinterpret_cast<u64*>(O.pt) + (size_t)set * (size_t)O.pt_cap * 3;
        u8* pt_c       = O.pt_const + (size_t)set * (size_t)O.pt_cap;
        const u64* src = reinterpret_cast<const u64*>(M.pt_pos);
        for (int j = tid; j < n_pt; j += SCENE_THREADS)
        {
            const int p = ids[j];
            pt[(size_t)j * 3 + 0] = src[(size_t)p * 3 + 0], pt[(size_t)j * 3 + 1] = src[(size_t)p * 3 + 1], pt[(size_t)j * 3 + 2] = src[(size_t)p * 3 + 2];
            pt_c[j]     = scene_point_constant(M.pt_flags[p]) ? 1 : 0;
            pt_valid[j] = 0;
        }
    }
    if (tid < 64)  // one wavefront: the pairs in order by a ballot
    {
        bool emit = false;
        int a = 0, b = 0;
        if (c.use_imu && tid >= 1 && tid < nw)
        {
            a = s_win[tid - 1], b = s_win[tid];
            emit = scene_rpc_emitted(M.kf_time[a], M.kf_time[b], M.kf_imu_begin[b], M.kf_imu_end[b], M.kf_preint_valid[b]);
        }
        const u64 votes = __ballot(emit);
        if (emit)
        {
            const int rank = __popcll(votes & ((1ull << tid) - 1ull));
            snk_ba_rpc* r  = O.rpc + (size_t)set * (size_t)O.win_cap + rank;
            r->img1 = tid - 1, r->img2 = tid;
#pragma unroll
            for (int e = 0; e < 7; ++e) r->rel_pose[e] = M.kf_rpc[b].rel_pose[e];
            double w_rot, w_tr;
            scene_rpc_weights(M.kf_time[a], M.kf_time[b], c.gyro_weight, c.acc_weight, M.kf_rpc[b].weight_translation, w_rot, w_tr);
            r->weight_rotation = w_rot, r->weight_translation = w_tr;
        }
        if (tid == 0) s_misc[W_NRPC] = (u32)__popcll(votes);
    }
    __syncthreads();  // pt_valid = 0 is behind; walk 3 sets the ones

    // ---- walk 3 (:258-291): the records, image by image, inside an image in the order of the walk ----
    {
        int* o_img    = O.obs_img + (size_t)set * (size_t)O.obs_cap;
        int* o_pt     = O.obs_pt + (size_t)set * (size_t)O.obs_cap;
        double* o_uv  = O.obs_uv + (size_t)set * (size_t)O.obs_cap * 2;
        double* o_dep = O.obs_depth + (size_t)set * (size_t)O.obs_cap;
        double* o_w   = O.obs_weight + (size_t)set * (size_t)O.obs_cap;
        int* o_src    = O.obs_src + (size_t)set * (size_t)O.obs_cap * 2;
        walk([&](bool active, int j, int p, int pos, int) {
            int img = -1, kf = -1, fi = 0;
            if (active)
            {
                kf = M.obs[pos][0], fi = M.obs[pos][1];
                if (!M.kf_bad[kf])
                {
                    pt_valid[j] = 1;  // nEdges > 0 (:263, :292): before the constant-constant skip
                    img         = image_of(kf);
                    if (img >= 0 && scene_record_skipped(0, img >= nw, scene_point_constant(M.pt_flags[p]))) img = -1;
                }
            }
            s_cimg[tid] = img;
            __syncthreads();
            int rank = 0;
            u32 base = 0;
            if (img >= 0)
            {
                for (int t = 0; t < tid; ++t) rank += s_cimg[t] == img ? 1 : 0;
                base = s_base[img];
            }
            __syncthreads();
            if (img >= 0)
            {
                atomicAdd(&s_base[img], 1u);  // the next sub-chunk's base; this one's was read behind the barrier
                const size_t at = (size_t)base + (size_t)rank;
                const int f     = M.feat_start[kf] + fi;
                o_img[at] = img, o_pt[at] = j;
                o_uv[at * 2 + 0] = (double)M.feat_uv[(size_t)f * 2 + 0], o_uv[at * 2 + 1] = (double)M.feat_uv[(size_t)f * 2 + 1];
                o_dep[at] = (double)M.feat_depth[f];
                o_w[at]   = (double)M.level_inv_sq_scale[M.feat_octave[f]];
                o_src[at * 2 + 0] = kf, o_src[at * 2 + 1] = fi;
            }
        });
    }
    for (int i = n_pt + tid; i < O.pt_cap; i += SCENE_THREADS) ids[i] = -1;
    if (tid == 0) reinterpret_cast<SceneResult*>(O.result)[set] = SceneResult{nw, n_img, n_pt, n_obs, (int)s_misc[W_NRPC], SCENE_OK};
}

int check_window_scalars(int n_q, int n_kf, const snk_scene_params* p, int win_cap)
{
    SNK_REQUIRE(p != nullptr, "scene: params is NULL");
    SNK_REQUIRE(n_q >= 0 && n_kf >= 0, "scene: negative count");
    SNK_REQUIRE(n_kf <= SNK_COVIS_MAX_KF, "scene: n_kf above SNK_COVIS_MAX_KF (32768)");
    SNK_REQUIRE(p->n_neighbours >= 0 && p->n_last >= 0, "scene: a parameter below 0");
    SNK_REQUIRE((long long)p->n_neighbours + 1 + (long long)p->n_last <= SNK_SCENE_MAX_WINDOW, "scene: n_neighbours + 1 + n_last above SNK_SCENE_MAX_WINDOW (64)");
    SNK_REQUIRE(win_cap >= 1 && win_cap <= SNK_SCENE_MAX_WINDOW, "scene: win_cap outside [1, SNK_SCENE_MAX_WINDOW]");
    return SNK_OK;
}

// a row output of snk_scene_gather: where the caller wants it, the rows' capacity in items, an item's bytes, and the count of the
// query's result that a row comes back up to (nullptr: the whole row)
struct SceneRow
{
    void* dst;
    size_t cap, item;
    int32_t SceneResult::*count;
};

bool has_imu(const snk_scene_map* map)
{
    return map->kf_time != nullptr;
}

int check_gather_scalars(int n_q, const snk_scene_map* map, const snk_scene_params* p, const snk_scene_out* o)
{
    SNK_REQUIRE(map != nullptr && p != nullptr && o != nullptr, "scene: map, params or out is NULL");
    SNK_REQUIRE(n_q >= 0 && map->n_kf >= 0 && map->n_points >= 0 && map->n_obs >= 0 && map->n_feat >= 0 && map->n_levels >= 0, "scene: negative count");
    SNK_REQUIRE(map->n_kf <= SNK_COVIS_MAX_KF, "scene: n_kf above SNK_COVIS_MAX_KF (32768)");
    SNK_REQUIRE(o->win_cap >= 1 && o->win_cap <= SNK_SCENE_MAX_WINDOW, "scene: win_cap outside [1, SNK_SCENE_MAX_WINDOW]");
    SNK_REQUIRE(o->pt_cap >= 1 && o->pt_cap <= SNK_LMAP_MAX_PTS, "scene: pt_cap outside [1, SNK_LMAP_MAX_PTS]");
    SNK_REQUIRE(o->img_cap >= 1 && o->img_cap <= SNK_SCENE_MAX_IMG, "scene: img_cap outside [1, SNK_SCENE_MAX_IMG]");
    SNK_REQUIRE(o->obs_cap >= 1 && o->obs_cap <= SNK_SCENE_MAX_OBS, "scene: obs_cap outside [1, SNK_SCENE_MAX_OBS]");
    SNK_REQUIRE(map->feat_start != nullptr && map->obs_start != nullptr, "scene: NULL feat_start or obs_start");
    SNK_REQUIRE(map->n_kf == 0 || (map->kf_bad != nullptr && map->kf_pose != nullptr), "scene: NULL kf_bad or kf_pose with n_kf > 0");
    SNK_REQUIRE(map->n_feat == 0 || (map->feat_point != nullptr && map->feat_depth != nullptr && map->feat_uv != nullptr && map->feat_octave != nullptr),
                "scene: NULL feature array with n_feat > 0");
    SNK_REQUIRE(map->n_obs == 0 || map->obs != nullptr, "scene: NULL obs with n_obs > 0");
    SNK_REQUIRE(map->n_points == 0 || (map->pt_flags != nullptr && map->pt_pos != nullptr), "scene: NULL pt_flags or pt_pos with n_points > 0");
    SNK_REQUIRE(map->n_levels == 0 || map->level_inv_sq_scale != nullptr, "scene: NULL level_inv_sq_scale with n_levels > 0");
    const int n_imu = (map->kf_time != nullptr) + (map->kf_imu_begin != nullptr) + (map->kf_imu_end != nullptr) + (map->kf_preint_valid != nullptr) +
                      (map->kf_rpc != nullptr);
    SNK_REQUIRE(n_imu == 0 || n_imu == 5, "scene: the IMU tables are either all NULL or all present");
    if (n_q == 0) return SNK_OK;
    SNK_REQUIRE(o->img_kf != nullptr && o->pose != nullptr && o->img_const != nullptr && o->pt_id != nullptr && o->pt != nullptr && o->pt_const != nullptr &&
                    o->pt_valid != nullptr && o->obs_img != nullptr && o->obs_pt != nullptr && o->obs_uv != nullptr && o->obs_depth != nullptr &&
                    o->obs_weight != nullptr && o->obs_src != nullptr && o->result != nullptr,
                "scene: NULL output with n_q > 0");
    SNK_REQUIRE(!(has_imu(map) && p->gyro_weight > 0) || o->rpc != nullptr, "scene: NULL rpc output where constraints are emitted");
    return SNK_OK;
}

int launch_window(snk_matcher* m, const WindowCall& C)
{
    hipLaunchKernelGGL(scene_window_kernel, dim3(C.n_q), dim3(SCENE_WIN_THREADS), scene_window_carve(), m->stream, C);
    SNK_LAUNCH_CHECK();
    return SNK_OK;
}

int launch_gather(snk_matcher* m, const GatherCall& C)
{
    int rc;
    if ((rc = set_max_lds_once(reinterpret_cast<const void*>(scene_gather_kernel), (int)scene_gather_carve(LMAP_MAX_PTS, SCENE_MAX_IMG))) != SNK_OK) return rc;
    hipLaunchKernelGGL(scene_gather_kernel, dim3(C.n_q), dim3(SCENE_THREADS), scene_gather_carve(C.out.pt_cap, C.out.img_cap), m->stream, C);
    SNK_LAUNCH_CHECK();
    return SNK_OK;
}

WindowCall window_call(int n_q, int n_kf, int n_list, const snk_scene_params* p, int win_cap)
{
    WindowCall C{};
    C.n_q = n_q, C.n_kf = n_kf, C.n_list = n_list, C.n_neighbours = p->n_neighbours, C.n_last = p->n_last, C.win_cap = win_cap;
    return C;
}

GatherCall gather_call(int n_q, const snk_scene_map* map, const snk_scene_params* p, const snk_scene_out* o)
{
    GatherCall C{};
    C.n_q = n_q, C.use_imu = has_imu(map) && p->gyro_weight > 0 ? 1 : 0;
    C.gyro_weight = p->gyro_weight, C.acc_weight = p->acc_weight;
    C.map = *map, C.out = *o;
    return C;
}
}  // namespace
}  // namespace snk

using namespace snk;

extern "C" {
int snk_scene_window(snk_matcher* m, int n_q, const int32_t* q, int n_kf, const uint8_t* kf_bad, const int32_t* kf_prev, const int32_t* conn_start,
                     const snk_covis_conn* conn_list, const snk_scene_params* params, int win_cap, int32_t* window_kf, snk_scene_window_result* out)
{
    SNK_REQUIRE(m != nullptr, "NULL handle");
    int rc;
    if ((rc = check_window_scalars(n_q, n_kf, params, win_cap)) != SNK_OK) return rc;
    SNK_REQUIRE(n_kf == 0 || (kf_bad != nullptr && kf_prev != nullptr), "scene: NULL kf_bad or kf_prev with n_kf > 0");
    SNK_REQUIRE(conn_start != nullptr, "scene: NULL conn_start");
    if ((rc = check_starts(conn_start, n_kf, "scene: conn_start must begin at 0", "scene: conn_start must be non-decreasing")) != SNK_OK) return rc;
    const int n_list = conn_start[n_kf];
    SNK_REQUIRE(n_list == 0 || conn_list != nullptr, "scene: NULL conn_list with connections");
    for (int i = 0; i < n_list; ++i) SNK_REQUIRE(conn_list[i].kf >= 0 && conn_list[i].kf < n_kf, "scene: a connection's keyframe outside [0, n_kf)");
    for (int i = 0; i < n_kf; ++i) SNK_REQUIRE(kf_prev[i] >= -1 && kf_prev[i] < n_kf, "scene: a kf_prev outside [-1, n_kf)");
    if (n_q == 0) return SNK_OK;
    SNK_REQUIRE(q != nullptr && window_kf != nullptr && out != nullptr, "scene: NULL array with n_q > 0");
    for (int s = 0; s < n_q; ++s) SNK_REQUIRE(q[s] >= 0 && q[s] < n_kf, "scene: a query outside [0, n_kf)");
    const size_t ns = (size_t)n_q, cap = (size_t)win_cap;
    Block in, out_b;
    const int i_q = in.add(q, ns * 4), i_bad = in.add(kf_bad, (size_t)n_kf), i_prev = in.add(kf_prev, (size_t)n_kf * 4),
              i_start = in.add(conn_start, ((size_t)n_kf + 1) * 4), i_list = in.add(conn_list, (size_t)n_list * sizeof(snk_covis_conn));
    const int o_win = out_b.add(nullptr, ns * cap * 4), o_res = out_b.add(nullptr, ns * sizeof(SceneWindowResult));
    SNK_HIP_CHECK(hipSetDevice(m->device));
    if ((rc = stage_reserve(m, in.bytes, out_b.end())) != SNK_OK) return rc;
    if ((rc = stage_upload(m, in)) != SNK_OK) return rc;
    char *dev = m->q.as<char>(), *dout = m->out.as<char>(), *res = m->h_res.as<char>();
    WindowCall C = window_call(n_q, n_kf, n_list, params, win_cap);
    C.q          = in.at<const int>(dev, i_q);
    C.kf_bad     = in.at<const u8>(dev, i_bad);
    C.kf_prev    = in.at<const int>(dev, i_prev);
    C.conn_start = in.at<const int>(dev, i_start);
    C.conn_list  = in.at<const int2>(dev, i_list);
    C.window_kf  = out_b.at<int>(dout, o_win);
    C.out        = out_b.at<SceneWindowResult>(dout, o_res);
    if ((rc = launch_window(m, C)) != SNK_OK) return rc;
    if ((rc = stage_download(m, 0, out_b.end())) != SNK_OK) return rc;
    memcpy(window_kf, out_b.at<char>(res, o_win), ns * cap * 4);
    memcpy(out, out_b.at<char>(res, o_res), ns * sizeof(SceneWindowResult));
    return SNK_OK;
}

int snk_scene_window_batch_dev(snk_matcher* m, int n_q, const int32_t* q_dev, int n_kf, const uint8_t* kf_bad_dev, const int32_t* kf_prev_dev,
                               const int32_t* conn_start_dev, int n_list, const snk_covis_conn* conn_list_dev, const snk_scene_params* params, int win_cap,
                               int32_t* window_kf_dev, snk_scene_window_result* out_dev)
{
    SNK_REQUIRE(m != nullptr, "NULL handle");
    int rc;
    if ((rc = check_window_scalars(n_q, n_kf, params, win_cap)) != SNK_OK) return rc;
    SNK_REQUIRE(n_list >= 0, "scene: negative count");
    SNK_REQUIRE(n_kf == 0 || (kf_bad_dev != nullptr && kf_prev_dev != nullptr), "scene: NULL kf_bad or kf_prev with n_kf > 0");
    SNK_REQUIRE(conn_start_dev != nullptr, "scene: NULL conn_start");
    SNK_REQUIRE(n_list == 0 || conn_list_dev != nullptr, "scene: NULL conn_list with connections");
    if (n_q == 0) return SNK_OK;
    SNK_REQUIRE(q_dev != nullptr && window_kf_dev != nullptr && out_dev != nullptr, "scene: NULL array with n_q > 0");
    SNK_HIP_CHECK(hipSetDevice(m->device));
    WindowCall C = window_call(n_q, n_kf, n_list, params, win_cap);
    C.q          = q_dev;
    C.kf_bad     = kf_bad_dev;
    C.kf_prev    = kf_prev_dev;
    C.conn_start = conn_start_dev;
    C.conn_list  = reinterpret_cast<const int2*>(conn_list_dev);
    C.window_kf  = window_kf_dev;
    C.out        = reinterpret_cast<SceneWindowResult*>(out_dev);
    return launch_window(m, C);
}

int snk_scene_gather(snk_matcher* m, int n_q, const snk_scene_map* map, const int32_t* window_kf, const snk_scene_window_result* win,
                     const snk_scene_params* params, const snk_scene_out* out)
{
    SNK_REQUIRE(m != nullptr, "NULL handle");
    int rc;
    if ((rc = check_gather_scalars(n_q, map, params, out)) != SNK_OK) return rc;
    if ((rc = check_starts(map->feat_start, map->n_kf, "scene: feat_start must begin at 0", "scene: feat_start must be non-decreasing")) != SNK_OK) return rc;
    SNK_REQUIRE(map->feat_start[map->n_kf] == map->n_feat, "scene: feat_start[n_kf] must be n_feat");
    if ((rc = check_starts(map->obs_start, map->n_points, "scene: obs_start must begin at 0", "scene: obs_start must be non-decreasing")) != SNK_OK) return rc;
    SNK_REQUIRE(map->obs_start[map->n_points] == map->n_obs, "scene: obs_start[n_points] must be n_obs");
    for (int i = 0; i < map->n_feat; ++i)
    {
        SNK_REQUIRE(map->feat_point[i] >= -1 && map->feat_point[i] < map->n_points, "scene: a point id outside [-1, n_points)");
        SNK_REQUIRE(map->feat_octave[i] >= 0 && map->feat_octave[i] < map->n_levels, "scene: an octave outside [0, n_levels)");
    }
    for (int i = 0; i < map->n_obs; ++i)
    {
        const int k = map->obs[i][0], f = map->obs[i][1];
        SNK_REQUIRE(k >= 0 && k < map->n_kf, "scene: an observation's keyframe outside [0, n_kf)");
        SNK_REQUIRE(f >= 0 && f < map->feat_start[k + 1] - map->feat_start[k], "scene: an observation's feature outside its keyframe's range");
    }
    if (n_q == 0) return SNK_OK;
    SNK_REQUIRE(window_kf != nullptr && win != nullptr, "scene: NULL array with n_q > 0");
    const size_t ns = (size_t)n_q, wc = (size_t)out->win_cap, pc = (size_t)out->pt_cap, ic = (size_t)out->img_cap, oc = (size_t)out->obs_cap;
    for (int s = 0; s < n_q; ++s)
    {
        SNK_REQUIRE(win[s].status >= SNK_SCENE_OK && win[s].status <= SNK_SCENE_BAD_INDEX, "scene: an unknown stage-1 status");
        if (win[s].status != SNK_SCENE_OK) continue;
        SNK_REQUIRE(win[s].n_window >= 0 && win[s].n_window <= out->win_cap, "scene: a stage-1 count outside [0, win_cap]");
        long long feats = 0;
        for (int i = 0; i < win[s].n_window; ++i)
        {
            const int k = window_kf[(size_t)s * wc + (size_t)i];
            SNK_REQUIRE(k >= 0 && k < map->n_kf, "scene: a window keyframe outside [0, n_kf)");
            SNK_REQUIRE(i == 0 || window_kf[(size_t)s * wc + (size_t)i - 1] < k, "scene: a window that is not strictly ascending");
            feats += map->feat_start[k + 1] - map->feat_start[k];
        }
        SNK_REQUIRE(feats <= LMAP_MAX_ORDER, "scene: more than 2^30 features in a window");
    }
    // a window walks every point once: its stream is at most n_obs
    SNK_REQUIRE(map->n_obs <= SCENE_MAX_WALK, "scene: more than 2^30 observations");
    const size_t nk = (size_t)map->n_kf, np = (size_t)map->n_points, nf = (size_t)map->n_feat, no = (size_t)map->n_obs;
    const bool imu = has_imu(map);
    Block in, out_b;
    const int i_bad = in.add(map->kf_bad, nk), i_pose = in.add(map->kf_pose, nk * 56), i_fs = in.add(map->feat_start, (nk + 1) * 4),
              i_fp = in.add(map->feat_point, nf * 4), i_fd = in.add(map->feat_depth, nf * 4), i_uv = in.add(map->feat_uv, nf * 8),
              i_oct = in.add(map->feat_octave, nf * 4), i_os = in.add(map->obs_start, (np + 1) * 4), i_obs = in.add(map->obs, no * 8),
              i_fl = in.add(map->pt_flags, np), i_pos = in.add(map->pt_pos, np * 24), i_lvl = in.add(map->level_inv_sq_scale, (size_t)map->n_levels * 4),
              i_t = in.add(map->kf_time, imu ? nk * 8 : 0), i_tb = in.add(map->kf_imu_begin, imu ? nk * 8 : 0), i_te = in.add(map->kf_imu_end, imu ? nk * 8 : 0),
              i_pv = in.add(map->kf_preint_valid, imu ? nk : 0), i_rpc = in.add(map->kf_rpc, imu ? nk * sizeof(snk_ba_rpc) : 0),
              i_win = in.add(window_kf, ns * wc * 4), i_wr = in.add(win, ns * sizeof(SceneWindowResult));
    // the outputs as one block, in the order of snk_scene_out: parts 0 .. 13 are the row outputs of `rows`, part 14 the results
    const SceneRow rows[14] = {{out->img_kf, ic, 4, &SceneResult::n_img},     {out->pose, ic, 56, &SceneResult::n_img},
                               {out->img_const, ic, 1, &SceneResult::n_img},  {out->pt_id, pc, 4, nullptr},
                               {out->pt, pc, 24, &SceneResult::n_pt},         {out->pt_const, pc, 1, &SceneResult::n_pt},
                               {out->pt_valid, pc, 1, &SceneResult::n_pt},    {out->obs_img, oc, 4, &SceneResult::n_obs},
                               {out->obs_pt, oc, 4, &SceneResult::n_obs},     {out->obs_uv, oc, 16, &SceneResult::n_obs},
                               {out->obs_depth, oc, 8, &SceneResult::n_obs},  {out->obs_weight, oc, 8, &SceneResult::n_obs},
                               {out->obs_src, oc, 8, &SceneResult::n_obs},    {out->rpc, wc, sizeof(snk_ba_rpc), &SceneResult::n_rpc}};
    for (const SceneRow& row : rows) out_b.add(nullptr, ns * row.cap * row.item);
    const int o_result = out_b.add(nullptr, ns * sizeof(SceneResult));
    SNK_HIP_CHECK(hipSetDevice(m->device));
    if ((rc = stage_reserve(m, in.bytes, out_b.bytes)) != SNK_OK) return rc;  // this block has always been asked for with its last part padded
    if ((rc = stage_upload(m, in)) != SNK_OK) return rc;
    char *dev = m->q.as<char>(), *dout = m->out.as<char>(), *res = m->h_res.as<char>();
    snk_scene_map dmap = *map;
    dmap.kf_bad = in.at<const uint8_t>(dev, i_bad), dmap.kf_prev = nullptr, dmap.kf_pose = in.at<const double>(dev, i_pose);
    dmap.feat_start = in.at<const int32_t>(dev, i_fs), dmap.feat_point = in.at<const int32_t>(dev, i_fp), dmap.feat_depth = in.at<const float>(dev, i_fd);
    dmap.feat_uv = in.at<const float>(dev, i_uv), dmap.feat_octave = in.at<const int32_t>(dev, i_oct), dmap.obs_start = in.at<const int32_t>(dev, i_os);
    dmap.obs = reinterpret_cast<const int32_t(*)[2]>(in.at<const int32_t>(dev, i_obs)), dmap.pt_flags = in.at<const uint8_t>(dev, i_fl);
    dmap.pt_pos = in.at<const double>(dev, i_pos), dmap.level_inv_sq_scale = in.at<const float>(dev, i_lvl);
    if (imu)
    {
        dmap.kf_time = in.at<const double>(dev, i_t), dmap.kf_imu_begin = in.at<const double>(dev, i_tb), dmap.kf_imu_end = in.at<const double>(dev, i_te);
        dmap.kf_preint_valid = in.at<const uint8_t>(dev, i_pv), dmap.kf_rpc = in.at<const snk_ba_rpc>(dev, i_rpc);
    }
    snk_scene_out dso = *out;
    dso.img_kf = out_b.at<int32_t>(dout, 0), dso.pose = out_b.at<double>(dout, 1), dso.img_const = out_b.at<uint8_t>(dout, 2);
    dso.pt_id = out_b.at<int32_t>(dout, 3), dso.pt = out_b.at<double>(dout, 4), dso.pt_const = out_b.at<uint8_t>(dout, 5);
    dso.pt_valid = out_b.at<uint8_t>(dout, 6), dso.obs_img = out_b.at<int32_t>(dout, 7), dso.obs_pt = out_b.at<int32_t>(dout, 8);
    dso.obs_uv = out_b.at<double>(dout, 9), dso.obs_depth = out_b.at<double>(dout, 10), dso.obs_weight = out_b.at<double>(dout, 11);
    dso.obs_src = out_b.at<int32_t>(dout, 12), dso.rpc = out_b.at<snk_ba_rpc>(dout, 13), dso.result = out_b.at<snk_scene_result>(dout, o_result);
    GatherCall C = gather_call(n_q, &dmap, params, &dso);
    C.window_kf  = in.at<const int>(dev, i_win);
    C.win        = in.at<const SceneWindowResult>(dev, i_wr);
    if ((rc = launch_gather(m, C)) != SNK_OK) return rc;
    if ((rc = stage_download(m, 0, out_b.bytes)) != SNK_OK) return rc;
    // a row comes back up to its count: the words behind it were never written
    const SceneResult* r = out_b.at<const SceneResult>(res, o_result);
    for (size_t s = 0; s < ns; ++s)
        for (int part = 0; part < 14; ++part)
        {
            const SceneRow& row = rows[part];
            const size_t at = s * row.cap * row.item;
            const int count = row.count ? r[s].*row.count : out->pt_cap;
            if (row.dst != nullptr && count > 0) memcpy(static_cast<char*>(row.dst) + at, out_b.at<char>(res, part) + at, (size_t)count * row.item);
        }
    memcpy(out->result, r, ns * sizeof(SceneResult));
    return SNK_OK;
}

int snk_scene_gather_batch_dev(snk_matcher* m, int n_q, const snk_scene_map* map_dev, const int32_t* window_kf_dev, const snk_scene_window_result* win_dev,
                               const snk_scene_params* params, const snk_scene_out* out_dev)
{
    SNK_REQUIRE(m != nullptr, "NULL handle");
    int rc;
    if ((rc = check_gather_scalars(n_q, map_dev, params, out_dev)) != SNK_OK) return rc;
    if (n_q == 0) return SNK_OK;
    SNK_REQUIRE(window_kf_dev != nullptr && win_dev != nullptr, "scene: NULL array with n_q > 0");
    SNK_HIP_CHECK(hipSetDevice(m->device));
    GatherCall C = gather_call(n_q, map_dev, params, out_dev);
    C.window_kf  = window_kf_dev;
    C.win        = reinterpret_cast<const SceneWindowResult*>(win_dev);
    return launch_gather(m, C);
}
}
