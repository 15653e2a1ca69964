// Local map of fine tracking for gfx950 ("snk-lmap v1") — replaces, for many frames per call,
//   the rest of Tracking::UpdateLocalKeyFrames2       (reference Snake/Tracking/TrackingFine.cpp:272-323)   lmap_select_kernel
//   Tracking::UpdateLocalPoints / LocalMap::addPoint  (:328-356, Snake/Map/LocalMap.h:139-154)              lmap_gather_kernel
// The per-item statements are lmap_core.hpp's; the carves and the table size are dispatch.hpp's.
//
// Mapping to the hardware.  Both kernels: a workgroup of four wavefronts per set (frame), every byte of LDS in the dynamic carve, no
// scratch.  Lists are built in order by prefix sums: a chunk is one item per lane, block_scan gives a lane its rank inside the chunk
// (six DPP additions per wavefront, four partial sums in LDS, one barrier), a running base carries over.
//
// lmap_select_kernel.  The marks of TrackingFine.cpp:246-250 are a bit per keyframe (atomic OR).  The direct keyframes are copied from
// the back of the vote's list.  Walk 1: a lane per remaining entry evaluates its own draw; accepted entries are ranked into the local
// list, the rejected ones are only counted (walk 2 recomputes their draws instead of storing up to n_kf of them).  Neighbours: a slot
// per (local keyframe, neighbour rank) in list order; a listable candidate becomes the key kf << bits | slot, the keys are sorted by
// block_sort (wg.hpp) and an entry whose predecessor has another keyframe is that keyframe's first appearance; the firsts go back to
// their slots, so that a scan over the slots restores the reference's order.  Walk 2 runs over the rejected entries and then over the
// slots, two scans per chunk (the position in `indirect`, the position in the local list).
//
// lmap_gather_kernel.  Every candidate has an order number: its position in the concatenated feature ranges of the local keyframes
// (block_scan_long over at most 256 ranges), the own points behind them.  The points are the first-appearance table of wg.hpp: four-byte
// slots holding order + 1, the id of a slot recovered through feat_point / set_point by a search of the prefix sums, so 32 768 slots
// are 128 KiB.  A slot of the same id takes an atomic minimum.  The own points come after a barrier: on a slot that a keyframe placed
// they set bit 31 ("valid is cleared"), otherwise they claim or take the minimum among themselves.  Emit (table_emit): winners write
// their 96-byte record (twelve 8-byte words) and their id.  No result depends on the order in which atomics land: the table's contents
// as a set (id -> minimum order, flag) do not, and nothing else is read from it.
//
// The host entries lay the arrays of a call out as one block, inputs and outputs alike: stage.hpp, and matcher_handle.hpp for the copies.
#include <cstddef>

#include "matcher_handle.hpp"

#include "lmap_core.hpp"
#include "dispatch.hpp"
#include "wg.hpp"

namespace snk
{
namespace
{
using u8  = unsigned char;
using u32 = unsigned int;
using u64 = unsigned long long;

static_assert(sizeof(snk_lmap_select_result) == 20 && sizeof(LmapSelectResult) == 20 && sizeof(snk_lmap_gather_result) == 16 && sizeof(LmapGatherResult) == 16 &&
                  sizeof(snk_lm_fine) == 96 && sizeof(snk_covis_conn) == 8 && sizeof(snk_covis_result) == 16,
              "snk-lmap layouts");
static_assert(offsetof(snk_lm_fine, desc) == 48 && offsetof(snk_lm_fine, reference_depth) == 80 && offsetof(snk_lm_fine, reference_scale_level) == 84 &&
                  offsetof(snk_lm_fine, valid) == 88,
              "snk_lm_fine as twelve words");
static_assert(LMAP_MAX_LOCAL_KF == SNK_LMAP_MAX_LOCAL_KF && LMAP_MAX_PTS == SNK_LMAP_MAX_PTS && LMAP_MAX_NEIGHBOURS == SNK_LMAP_MAX_NEIGHBOURS, "snk-lmap limits");
static_assert(LMAP_OK == SNK_LMAP_OK && LMAP_EMPTY == SNK_LMAP_EMPTY && LMAP_TRUNCATED == SNK_LMAP_TRUNCATED && LMAP_KF_OVERFLOW == SNK_LMAP_KF_OVERFLOW &&
                  LMAP_PTS_OVERFLOW == SNK_LMAP_PTS_OVERFLOW && LMAP_BAD_INDEX == SNK_LMAP_BAD_INDEX && LMAP_PT_BAD == SNK_COVIS_PT_BAD &&
                  LMAP_VOTE_OK == SNK_COVIS_OK && LMAP_VOTE_UNCHANGED == SNK_COVIS_UNCHANGED,
              "snk-lmap constants");
static_assert(lmap_select_carve(SNK_COVIS_MAX_KF, LMAP_MAX_LOCAL_KF, LMAP_MAX_NEIGHBOURS) <= (size_t)LDS_MAX_BYTES, "LDS carve of lmap_select_kernel");
static_assert(lmap_gather_carve(LMAP_MAX_LOCAL_KF, LMAP_MAX_PTS) <= (size_t)LDS_MAX_BYTES, "LDS carve of lmap_gather_kernel");
static_assert(LMAP_THREADS == 256 && LMAP_MAX_LOCAL_KF <= LMAP_THREADS && LMAP_MISC >= 16, "a lane per local keyframe; the words of s_misc");
// kf << bits | slot stays below the padding key
static_assert((long long)SNK_COVIS_MAX_KF * lmap_sort_len(LMAP_MAX_LOCAL_KF, LMAP_MAX_NEIGHBOURS) < 0xFFFFFFFFll, "neighbour sort key");
static_assert(lmap_table_slots(LMAP_MAX_PTS) >= LMAP_MAX_PTS + LMAP_THREADS && lmap_table_slots(1) >= 1 + LMAP_THREADS, "room for the claims in flight");

// words of s_misc
enum { W_BAD = 0, W_FULL = 1, W_COUNT = 2, W_NB = 3, W_SEARCH = 4, W_OWN = 5, W_PART = 8 };

struct SelectCall
{
    int n_sets, vote_cap, n_kf, n_list;
    int n_direct, n_direct_prob, n_indirect_prob, n_neighbours, kf_cap;
    u64 seed;
    const snk_covis_conn* conn;    // [n_sets][vote_cap]
    const snk_covis_result* vote;  // [n_sets]
    const u8* kf_bad;              // [n_kf]
    const int* conn_start;         // [n_kf + 1]
    const int2* conn_list;         // [n_list] (weight, kf)
    const int* frame_id;           // [n_sets]
    int* local_kf;                 // [n_sets][kf_cap]
    LmapSelectResult* out;         // [n_sets]
};

struct GatherCall
{
    int n_sets, n_kf, n_points, n_feat, n_set_points, kf_cap, pts_cap;
    const int* feat_start;
    const int* feat_point;
    const u8* pt_flags;
    const int* pt_last_seen;
    const int* frame_id;
    const int* local_kf;
    const LmapSelectResult* sel;
    const int* set_start;
    const int* set_point;
    const u64* pos;     // [n_points][3] doubles, copied as words
    const u64* normal;  // [n_points][3]
    const u64* desc;    // [n_points][4]
    const float* ref_depth;
    const int* ref_level;
    u64* lm_pts;  // [n_sets][pts_cap][12]
    int* lm_point;
    int* n_pts;
    LmapGatherResult* out;
};

__global__ __launch_bounds__(LMAP_THREADS) void lmap_select_kernel(SelectCall c)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int n_words = (c.n_kf + 31) / 32 + 1;
    const int P       = lmap_sort_len(c.kf_cap, c.n_neighbours);
    u32* s_mark  = reinterpret_cast<u32*>(smem);               // [n_words] a bit per keyframe
    int* s_local = reinterpret_cast<int*>(s_mark + n_words);   // [kf_cap]
    u32* s_keys  = reinterpret_cast<u32*>(s_local + c.kf_cap);  // [P]
    int* s_first = reinterpret_cast<int*>(s_keys + P);          // [P] by slot: the neighbour appended from it, or -1
    u32* s_misc  = reinterpret_cast<u32*>(s_first + P);         // [LMAP_MISC]
    const int tid = threadIdx.x;
    const int set = blockIdx.x;
    int* row      = c.local_kf + (size_t)set * (size_t)c.kf_cap;
    int pass      = 0;

    auto finish = [&](int status) {  // uniform
        for (int i = tid; i < c.kf_cap; i += LMAP_THREADS) row[i] = -1;
        if (tid == 0) c.out[set] = lmap_no_list(status);
    };

    const snk_covis_result v = c.vote[set];
    const int vote_status    = lmap_vote_status(v.status, v.n_found, v.n_conn, c.vote_cap);
    if (vote_status != LMAP_OK)
    {
        finish(vote_status);
        return;
    }
    const int L                = v.n_found;  // == n_conn <= vote_cap
    const snk_covis_conn* list = c.conn + (size_t)set * (size_t)c.vote_cap;

    for (int i = tid; i < n_words; i += LMAP_THREADS) s_mark[i] = 0;
    if (tid < LMAP_MISC) s_misc[tid] = 0;
    __syncthreads();

    // ---- the marks: every keyframe of the vote's list (:246-250) ----
    for (int i = tid; i < L; i += LMAP_THREADS)
    {
        const int k = list[i].kf;
        if (k < 0 || k >= c.n_kf) s_misc[W_BAD] = 1;
        else atomicOr(&s_mark[k >> 5], 1u << (k & 31));
    }
    __syncthreads();
    if (s_misc[W_BAD])  // uniform
    {
        finish(LMAP_BAD_INDEX);
        return;
    }

    // ---- direct (:272-276) ----
    const int nd = c.n_direct < L ? c.n_direct : L;
    const int R  = L - nd;
    if (nd > c.kf_cap)
    {
        finish(LMAP_KF_OVERFLOW);
        return;
    }
    for (int i = tid; i < nd; i += LMAP_THREADS) s_local[i] = list[L - 1 - i].kf;
    const u32 key = lmap_key(c.seed, c.frame_id[set]);

    // ---- walk 1 (:282-295): entry j from the back takes draw j; accepted -> local list, rejected -> counted ----
    int n_acc = 0, n_rej = 0;
    for (int base = 0; base < R; base += LMAP_THREADS)  // uniform
    {
        const int j    = base + tid;
        const bool in  = j < R;
        const bool acc = in && lmap_accept(lmap_draw(key, (u32)j), c.n_direct_prob, R);
        int total;
        const int ex = block_scan<LMAP_THREADS>(in ? (acc ? 1 : 0x10000) : 0, total, s_misc + W_PART, pass);
        if (acc)
        {
            const int pos = nd + n_acc + (ex & 0xFFFF);
            if (pos < c.kf_cap) s_local[pos] = list[L - 1 - nd - j].kf;
        }
        n_acc += total & 0xFFFF;
        n_rej += total >> 16;
    }
    const int n1 = nd + n_acc;
    if (n1 > c.kf_cap)
    {
        finish(LMAP_KF_OVERFLOW);
        return;
    }
    __syncthreads();

    // ---- neighbours (:299-313): a slot per (local keyframe, rank), the firsts by a sort on kf << bits | slot ----
    const int nn      = c.n_neighbours;
    const int n_slots = n1 * nn;
    const int Pn      = n_slots > 0 ? lmap_pow2_at_least(n_slots, 4) : 0;  // <= P
    int obits         = 0;
    while ((1 << obits) < P) obits += 1;
    const u32 omask = (1u << obits) - 1u;
    for (int o = tid; o < Pn; o += LMAP_THREADS)
    {
        u32 k32    = 0xFFFFFFFFu;
        s_first[o] = -1;
        if (o < n_slots)
        {
            const int li = o / nn, t = o - li * nn;
            const int k = s_local[li];
            const int a = c.conn_start[k], b = c.conn_start[k + 1];
            if (a < 0 || b < a || b > c.n_list) s_misc[W_BAD] = 1;
            else
            {
                const int cnt = nn < b - a ? nn : b - a;  // the last cnt entries, ascending (KeyframeGraph.cpp:62)
                if (t < cnt)
                {
                    const int nb = c.conn_list[b - cnt + t].y;
                    if (nb < 0 || nb >= c.n_kf) s_misc[W_BAD] = 1;
                    else if (lmap_neighbour_listed(c.kf_bad[nb], (s_mark[nb >> 5] >> (nb & 31)) & 1u)) k32 = (u32)nb << obits | (u32)o;
                }
            }
        }
        s_keys[o] = k32;
    }
    __syncthreads();
    if (s_misc[W_BAD])  // uniform
    {
        finish(LMAP_BAD_INDEX);
        return;
    }
    block_sort<LMAP_THREADS>(s_keys, Pn);
    for (int i = tid; i < Pn; i += LMAP_THREADS)
    {
        const u32 k32 = s_keys[i];
        if (k32 != 0xFFFFFFFFu && (i == 0 || (s_keys[i - 1] >> obits) != (k32 >> obits)))
        {
            s_first[k32 & omask] = (int)(k32 >> obits);
            atomicAdd(&s_misc[W_NB], 1u);
        }
    }
    __syncthreads();
    const int n_ind = n_rej + (int)s_misc[W_NB];

    // ---- walk 2 (:316-323): entry j of `indirect` takes draw R + j; first the rejected of walk 1, then the neighbours ----
    int n_loc = n1, j_base = 0;
    for (int base = 0; base < R; base += LMAP_THREADS)  // uniform
    {
        const int j    = base + tid;
        const bool rej = j < R && !lmap_accept(lmap_draw(key, (u32)j), c.n_direct_prob, R);
        int total, total2;
        const int ji    = j_base + block_scan<LMAP_THREADS>(rej ? 1 : 0, total, s_misc + W_PART, pass);
        const bool acc2 = rej && lmap_accept(lmap_draw(key, (u32)(R + ji)), c.n_indirect_prob, n_ind);
        const int pos   = n_loc + block_scan<LMAP_THREADS>(acc2 ? 1 : 0, total2, s_misc + W_PART, pass);
        if (acc2 && pos < c.kf_cap) s_local[pos] = list[L - 1 - nd - j].kf;
        j_base += total;
        n_loc += total2;
    }
    for (int base = 0; base < n_slots; base += LMAP_THREADS)  // uniform
    {
        const int o   = base + tid;
        const int nb  = o < n_slots ? s_first[o] : -1;
        int total, total2;
        const int ji    = j_base + block_scan<LMAP_THREADS>(nb >= 0 ? 1 : 0, total, s_misc + W_PART, pass);
        const bool acc2 = nb >= 0 && lmap_accept(lmap_draw(key, (u32)(R + ji)), c.n_indirect_prob, n_ind);
        const int pos   = n_loc + block_scan<LMAP_THREADS>(acc2 ? 1 : 0, total2, s_misc + W_PART, pass);
        if (acc2 && pos < c.kf_cap) s_local[pos] = nb;
        j_base += total;
        n_loc += total2;
    }
    if (n_loc > c.kf_cap)
    {
        finish(LMAP_KF_OVERFLOW);
        return;
    }
    __syncthreads();
    for (int i = tid; i < c.kf_cap; i += LMAP_THREADS) row[i] = i < n_loc ? s_local[i] : -1;
    if (tid == 0) c.out[set] = LmapSelectResult{n_loc, nd, n_ind, list[L - 1].kf, LMAP_OK};
}

__global__ __launch_bounds__(LMAP_THREADS) void lmap_gather_kernel(GatherCall c)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int n_slots = lmap_table_slots(c.pts_cap);
    u32* s_tab    = reinterpret_cast<u32*>(smem);                      // [n_slots] order + 1 | own bit; 0 = free
    int* s_prefix = reinterpret_cast<int*>(s_tab + n_slots);           // [kf_cap + 1] first order of a local keyframe's features
    int* s_fstart = s_prefix + c.kf_cap + 1;                           // [kf_cap] its feat_start
    u32* s_misc   = reinterpret_cast<u32*>(s_fstart + c.kf_cap);        // [LMAP_MISC]
    const int tid = threadIdx.x;
    const int set = blockIdx.x;
    int* ids      = c.lm_point + (size_t)set * (size_t)c.pts_cap;
    int pass      = 0;

    auto finish = [&](int status) {  // uniform
        for (int i = tid; i < c.pts_cap; i += LMAP_THREADS) ids[i] = -1;
        if (tid == 0) c.n_pts[set] = 0, c.out[set] = lmap_no_points(status);
    };

    const LmapSelectResult sel = c.sel[set];
    if (sel.status != LMAP_OK && sel.status != LMAP_EMPTY)  // passed through
    {
        finish(sel.status == LMAP_TRUNCATED || sel.status == LMAP_KF_OVERFLOW || sel.status == LMAP_PTS_OVERFLOW ? sel.status : LMAP_BAD_INDEX);
        return;
    }
    const int n_local = sel.status == LMAP_EMPTY ? 0 : sel.n_local;
    if (n_local < 0 || n_local > c.kf_cap)
    {
        finish(LMAP_BAD_INDEX);
        return;
    }
    for (int i = tid; i < n_slots; i += LMAP_THREADS) s_tab[i] = 0;
    if (tid < LMAP_MISC) s_misc[tid] = 0;
    __syncthreads();

    // ---- order numbers: a prefix sum over the feature ranges (a lane per local keyframe), the own points behind them ----
    int len = 0;
    if (tid < n_local)
    {
        const int k = c.local_kf[(size_t)set * (size_t)c.kf_cap + tid];
        if (k < 0 || k >= c.n_kf) s_misc[W_BAD] = 1;
        else
        {
            const int a = c.feat_start[k], b = c.feat_start[k + 1];
            if (a < 0 || b < a || b > c.n_feat || b - a > LMAP_MAX_ORDER) s_misc[W_BAD] = 1;
            else len = b - a, s_fstart[tid] = a;
        }
    }
    long long T64;
    const long long ex = block_scan_long<LMAP_THREADS>(len, T64, s_misc + W_PART, pass);
    const int own_a = c.set_start[set], own_b = c.set_start[set + 1];
    const bool own_ok = own_a >= 0 && own_b >= own_a && own_b <= c.n_set_points;
    const int n_own   = own_ok ? own_b - own_a : 0;
    if (!own_ok || T64 + n_own > LMAP_MAX_ORDER || s_misc[W_BAD])  // uniform: the scans' barriers are behind the writes of W_BAD
    {
        finish(LMAP_BAD_INDEX);
        return;
    }
    const int T = (int)T64;
    if (tid < n_local) s_prefix[tid] = (int)ex;
    if (tid == 0) s_prefix[n_local] = T;
    __syncthreads();
    const int fid = c.frame_id[set];

    // the id of candidate ord: an own point, or the feature ord - first order of the last local keyframe whose first order is <= ord
    auto id_of = [&](int ord) {
        if (ord >= T) return c.set_point[own_a + (ord - T)];
        const int li = last_at_most(s_prefix, n_local, ord);
        return c.feat_point[s_fstart[li] + (ord - s_prefix[li])];
    };
    // addPoint (LocalMap.h:139-154) for candidate (p, ord)
    auto insert = [&](int p, int ord, bool own) {
        u32 seen;
        const int slot = table_place(s_tab, n_slots, p, ord, c.pts_cap, &s_misc[W_COUNT], &s_misc[W_FULL], seen, id_of);
        if (slot < 0 || seen == 0) return;
        if (own && (int)(seen & 0x7FFFFFFFu) - 1 < T) atomicOr(&s_tab[slot], 0x80000000u);  // :353 on a point that a keyframe placed
        else atomicMin(&s_tab[slot], (u32)ord + 1u);                                        // no own bit on this slot, now or later
    };

    // ---- build: the local keyframes' features (:334-342) ----
    for (int li = 0; li < n_local; ++li)  // uniform
    {
        const int a = s_fstart[li], first = s_prefix[li], n = s_prefix[li + 1] - first;
        for (int f = tid; f < n; f += LMAP_THREADS)
        {
            const int p = c.feat_point[a + f];
            if (p < -1 || p >= c.n_points) s_misc[W_BAD] = 1;
            else if (p >= 0 && !lmap_kf_point_skipped(p, c.pt_flags[p], c.pt_last_seen[p], fid)) insert(p, first + f, false);
        }
    }
    __syncthreads();
    // ---- build: the frame's own points (:344-354), behind the barrier: bit 31 goes on slots that a keyframe placed ----
    for (int i = tid; i < n_own; i += LMAP_THREADS)
    {
        const int p = c.set_point[own_a + i];
        if (p < -1 || p >= c.n_points) s_misc[W_BAD] = 1;
        else if (p >= 0 && !lmap_own_point_skipped(p, c.pt_flags[p])) insert(p, T + i, true);
    }
    __syncthreads();
    if (s_misc[W_BAD] || s_misc[W_FULL])  // uniform
    {
        finish(s_misc[W_BAD] ? LMAP_BAD_INDEX : LMAP_PTS_OVERFLOW);
        return;
    }

    // ---- emit: the winners write their 96-byte record (twelve 8-byte words) and their id ----
    u64* recs = c.lm_pts + (size_t)set * (size_t)c.pts_cap * 12;
    int searchable = 0, own_new = 0;
    const int n_out = table_emit<LMAP_THREADS>(
        s_tab, n_slots, T + n_own, c.pts_cap, s_misc + W_PART, pass, id_of,
        [&](int ord, int p) {
            return ord < T ? !lmap_kf_point_skipped(p, p >= 0 ? c.pt_flags[p] : 0, p >= 0 ? c.pt_last_seen[p] : 0, fid)
                           : !lmap_own_point_skipped(p, p >= 0 ? c.pt_flags[p] : 0);
        },
        [&](int ord, int p, int rank, u32 w) {
            const bool valid = ord < T && (w >> 31) == 0;
            u64* r           = recs + (size_t)rank * 12;
            const u64* sp    = c.pos + (size_t)p * 3;
            const u64* sn    = c.normal + (size_t)p * 3;
            const u64* sd    = c.desc + (size_t)p * 4;
            r[0] = sp[0], r[1] = sp[1], r[2] = sp[2];
            r[3] = sn[0], r[4] = sn[1], r[5] = sn[2];
            r[6] = sd[0], r[7] = sd[1], r[8] = sd[2], r[9] = sd[3];
            r[10] = (u64)__float_as_uint(c.ref_depth[p]) | (u64)(u32)c.ref_level[p] << 32;
            r[11] = valid ? 1ull : 0ull;  // valid and the seven pad bytes
            ids[rank] = p;
            searchable += valid ? 1 : 0;
            own_new += ord >= T ? 1 : 0;
        });
    searchable = wave_sum_xor(searchable);
    own_new    = wave_sum_xor(own_new);
    if ((tid & 63) == 0)
    {
        atomicAdd(&s_misc[W_SEARCH], (u32)searchable);
        atomicAdd(&s_misc[W_OWN], (u32)own_new);
    }
    __syncthreads();
    for (int i = n_out + tid; i < c.pts_cap; i += LMAP_THREADS) ids[i] = -1;
    if (tid == 0) c.n_pts[set] = n_out, c.out[set] = LmapGatherResult{n_out, (int)s_misc[W_SEARCH], (int)s_misc[W_OWN], LMAP_OK};
}

int check_params(const snk_lmap_params* p)
{
    SNK_REQUIRE(p != nullptr, "local map: params is NULL");
    SNK_REQUIRE(p->n_direct >= 0 && p->n_direct_prob >= 0 && p->n_indirect_prob >= 0 && p->n_neighbours >= 0, "local map: a parameter below 0");
    SNK_REQUIRE(p->n_neighbours <= SNK_LMAP_MAX_NEIGHBOURS, "local map: n_neighbours above SNK_LMAP_MAX_NEIGHBOURS (16)");
    SNK_REQUIRE(p->kf_cap >= 1 && p->kf_cap <= SNK_LMAP_MAX_LOCAL_KF, "local map: kf_cap outside [1, SNK_LMAP_MAX_LOCAL_KF]");
    return SNK_OK;
}

int launch_select(snk_matcher* m, const SelectCall& C)
{
    int rc;
    if ((rc = set_max_lds_once(reinterpret_cast<const void*>(lmap_select_kernel),
                               (int)lmap_select_carve(SNK_COVIS_MAX_KF, LMAP_MAX_LOCAL_KF, LMAP_MAX_NEIGHBOURS))) != SNK_OK)
        return rc;
    hipLaunchKernelGGL(lmap_select_kernel, dim3(C.n_sets), dim3(LMAP_THREADS), lmap_select_carve(C.n_kf, C.kf_cap, C.n_neighbours), m->stream, C);
    SNK_LAUNCH_CHECK();
    return SNK_OK;
}

int launch_gather(snk_matcher* m, const GatherCall& C)
{
    int rc;
    if ((rc = set_max_lds_once(reinterpret_cast<const void*>(lmap_gather_kernel), (int)lmap_gather_carve(LMAP_MAX_LOCAL_KF, LMAP_MAX_PTS))) != SNK_OK) return rc;
    hipLaunchKernelGGL(lmap_gather_kernel, dim3(C.n_sets), dim3(LMAP_THREADS), lmap_gather_carve(C.kf_cap, C.pts_cap), m->stream, C);
    SNK_LAUNCH_CHECK();
    return SNK_OK;
}

SelectCall select_call(int n_sets, int vote_cap, int n_kf, int n_list, const snk_lmap_params* p)
{
    SelectCall C{};
    C.n_sets = n_sets, C.vote_cap = vote_cap, C.n_kf = n_kf, C.n_list = n_list;
    C.n_direct = p->n_direct, C.n_direct_prob = p->n_direct_prob, C.n_indirect_prob = p->n_indirect_prob, C.n_neighbours = p->n_neighbours;
    C.kf_cap = p->kf_cap, C.seed = p->seed;
    return C;
}

int check_select_scalars(int n_sets, int vote_cap, int n_kf, const snk_lmap_params* params)
{
    int rc;
    if ((rc = check_params(params)) != SNK_OK) return rc;
    SNK_REQUIRE(n_sets >= 0 && n_kf >= 0, "local map: negative count");
    SNK_REQUIRE(n_kf <= SNK_COVIS_MAX_KF, "local map: n_kf above SNK_COVIS_MAX_KF (32768)");
    SNK_REQUIRE(vote_cap >= 1 && vote_cap <= SNK_COVIS_MAX_CAP, "local map: vote_cap outside [1, SNK_COVIS_MAX_CAP]");
    return SNK_OK;
}

int check_gather_scalars(int n_sets, const snk_lmap_map* map, const snk_lmap_points* points, int kf_cap, int pts_cap)
{
    SNK_REQUIRE(map != nullptr && points != nullptr, "local map: map or points is NULL");
    SNK_REQUIRE(n_sets >= 0 && map->n_kf >= 0 && map->n_points >= 0 && map->n_feat >= 0, "local map: negative count");
    SNK_REQUIRE(map->n_kf <= SNK_COVIS_MAX_KF, "local map: n_kf above SNK_COVIS_MAX_KF (32768)");
    SNK_REQUIRE(kf_cap >= 1 && kf_cap <= SNK_LMAP_MAX_LOCAL_KF, "local map: kf_cap outside [1, SNK_LMAP_MAX_LOCAL_KF]");
    SNK_REQUIRE(pts_cap >= 1 && pts_cap <= SNK_LMAP_MAX_PTS, "local map: pts_cap outside [1, SNK_LMAP_MAX_PTS]");
    SNK_REQUIRE(map->feat_start != nullptr, "local map: NULL feat_start");
    SNK_REQUIRE(map->n_feat == 0 || map->feat_point != nullptr, "local map: NULL feat_point with n_feat > 0");
    SNK_REQUIRE(map->n_points == 0 || (map->pt_flags != nullptr && map->pt_last_seen != nullptr), "local map: NULL pt_flags or pt_last_seen with n_points > 0");
    SNK_REQUIRE(map->n_points == 0 || (points->pos != nullptr && points->normal != nullptr && points->desc != nullptr && points->ref_depth != nullptr &&
                                       points->ref_level != nullptr),
                "local map: NULL array in points with n_points > 0");
    return SNK_OK;
}

GatherCall gather_call(int n_sets, const snk_lmap_map* map, const snk_lmap_points* points, int n_set_points, int kf_cap, int pts_cap)
{
    GatherCall C{};
    C.n_sets = n_sets, C.n_kf = map->n_kf, C.n_points = map->n_points, C.n_feat = map->n_feat, C.n_set_points = n_set_points;
    C.kf_cap = kf_cap, C.pts_cap = pts_cap;
    C.feat_start = map->feat_start, C.feat_point = map->feat_point, C.pt_flags = map->pt_flags, C.pt_last_seen = map->pt_last_seen;
    C.pos = reinterpret_cast<const u64*>(points->pos), C.normal = reinterpret_cast<const u64*>(points->normal);
    C.desc = reinterpret_cast<const u64*>(points->desc), C.ref_depth = points->ref_depth, C.ref_level = points->ref_level;
    return C;
}
}  // namespace
}  // namespace snk

using namespace snk;

extern "C" {
int snk_lmap_select(snk_matcher* m, int n_sets, const snk_covis_conn* conn, int vote_cap, const snk_covis_result* vote, int n_kf, const uint8_t* kf_bad,
                    const int32_t* conn_start, const snk_covis_conn* conn_list, const int32_t* frame_id, const snk_lmap_params* params, int32_t* local_kf,
                    snk_lmap_select_result* out)
{
    SNK_REQUIRE(m != nullptr, "NULL handle");
    int rc;
    if ((rc = check_select_scalars(n_sets, vote_cap, n_kf, params)) != SNK_OK) return rc;
    SNK_REQUIRE(n_kf == 0 || kf_bad != nullptr, "local map: NULL kf_bad with n_kf > 0");
    SNK_REQUIRE(conn_start != nullptr, "local map: NULL conn_start");
    if ((rc = check_starts(conn_start, n_kf, "local map: conn_start must begin at 0", "local map: conn_start must be non-decreasing")) != SNK_OK) return rc;
    const int n_list = conn_start[n_kf];
    SNK_REQUIRE(n_list == 0 || conn_list != nullptr, "local map: NULL conn_list with connections");
    for (int i = 0; i < n_list; ++i) SNK_REQUIRE(conn_list[i].kf >= 0 && conn_list[i].kf < n_kf, "local map: a connection's keyframe outside [0, n_kf)");
    if (n_sets == 0) return SNK_OK;
    SNK_REQUIRE(conn != nullptr && vote != nullptr && frame_id != nullptr && local_kf != nullptr && out != nullptr, "local map: NULL array with n_sets > 0");
    for (int s = 0; s < n_sets; ++s)
    {
        const int st = lmap_vote_status(vote[s].status, vote[s].n_found, vote[s].n_conn, vote_cap);
        SNK_REQUIRE(st != LMAP_BAD_INDEX, "local map: a vote record with a count outside its range or an unknown status");
        if (st != LMAP_OK) continue;
        for (int i = 0; i < vote[s].n_conn; ++i)
        {
            const int k = conn[(size_t)s * (size_t)vote_cap + (size_t)i].kf;
            SNK_REQUIRE(k >= 0 && k < n_kf, "local map: a voted keyframe outside [0, n_kf)");
        }
    }
    const size_t ns = (size_t)n_sets, cap = (size_t)params->kf_cap;
    Block in, out_b;
    const int i_conn = in.add(conn, ns * (size_t)vote_cap * sizeof(snk_covis_conn)), i_vote = in.add(vote, ns * sizeof(snk_covis_result)),
              i_bad = in.add(kf_bad, (size_t)n_kf), i_start = in.add(conn_start, ((size_t)n_kf + 1) * 4),
              i_list = in.add(conn_list, (size_t)n_list * sizeof(snk_covis_conn)), i_fid = in.add(frame_id, ns * 4);
    const int o_kf = out_b.add(nullptr, ns * cap * 4), o_res = out_b.add(nullptr, ns * sizeof(LmapSelectResult));
    SNK_HIP_CHECK(hipSetDevice(m->device));
    if ((rc = stage_reserve(m, in.bytes, out_b.end())) != SNK_OK) return rc;
    if ((rc = stage_upload(m, in)) != SNK_OK) return rc;
    char *dev = m->q.as<char>(), *dout = m->out.as<char>(), *res = m->h_res.as<char>();
    SelectCall C = select_call(n_sets, vote_cap, n_kf, n_list, params);
    C.conn       = in.at<const snk_covis_conn>(dev, i_conn);
    C.vote       = in.at<const snk_covis_result>(dev, i_vote);
    C.kf_bad     = in.at<const u8>(dev, i_bad);
    C.conn_start = in.at<const int>(dev, i_start);
    C.conn_list  = in.at<const int2>(dev, i_list);
    C.frame_id   = in.at<const int>(dev, i_fid);
    C.local_kf   = out_b.at<int>(dout, o_kf);
    C.out        = out_b.at<LmapSelectResult>(dout, o_res);
    if ((rc = launch_select(m, C)) != SNK_OK) return rc;
    if ((rc = stage_download(m, 0, out_b.end())) != SNK_OK) return rc;
    memcpy(local_kf, out_b.at<char>(res, o_kf), ns * cap * 4);
    memcpy(out, out_b.at<char>(res, o_res), ns * sizeof(LmapSelectResult));
    return SNK_OK;
}

int snk_lmap_select_batch_dev(snk_matcher* m, int n_sets, const snk_covis_conn* conn_dev, int vote_cap, const snk_covis_result* vote_dev, int n_kf,
                              const uint8_t* kf_bad_dev, const int32_t* conn_start_dev, int n_list, const snk_covis_conn* conn_list_dev,
                              const int32_t* frame_id_dev, const snk_lmap_params* params, int32_t* local_kf_dev, snk_lmap_select_result* out_dev)
{
    SNK_REQUIRE(m != nullptr, "NULL handle");
    int rc;
    if ((rc = check_select_scalars(n_sets, vote_cap, n_kf, params)) != SNK_OK) return rc;
    SNK_REQUIRE(n_list >= 0, "local map: negative count");
    SNK_REQUIRE(n_kf == 0 || kf_bad_dev != nullptr, "local map: NULL kf_bad with n_kf > 0");
    SNK_REQUIRE(conn_start_dev != nullptr, "local map: NULL conn_start");
    SNK_REQUIRE(n_list == 0 || conn_list_dev != nullptr, "local map: NULL conn_list with connections");
    if (n_sets == 0) return SNK_OK;
    SNK_REQUIRE(conn_dev != nullptr && vote_dev != nullptr && frame_id_dev != nullptr && local_kf_dev != nullptr && out_dev != nullptr,
                "local map: NULL array with n_sets > 0");
    SNK_HIP_CHECK(hipSetDevice(m->device));
    SelectCall C = select_call(n_sets, vote_cap, n_kf, n_list, params);
    C.conn       = conn_dev;
    C.vote       = vote_dev;
    C.kf_bad     = kf_bad_dev;
    C.conn_start = conn_start_dev;
    C.conn_list  = reinterpret_cast<const int2*>(conn_list_dev);
    C.frame_id   = frame_id_dev;
    C.local_kf   = local_kf_dev;
    C.out        = reinterpret_cast<LmapSelectResult*>(out_dev);
    return launch_select(m, C);
}

int snk_lmap_gather(snk_matcher* m, int n_sets, const snk_lmap_map* map, const snk_lmap_points* points, const int32_t* frame_id, const int32_t* local_kf,
                    int kf_cap, const snk_lmap_select_result* sel, const int32_t* set_start, const int32_t* set_point, int pts_cap, snk_lm_fine* lm_pts,
                    int32_t* lm_point, int32_t* n_pts, snk_lmap_gather_result* out)
{
    SNK_REQUIRE(m != nullptr, "NULL handle");
    int rc;
    if ((rc = check_gather_scalars(n_sets, map, points, kf_cap, pts_cap)) != SNK_OK) return rc;
    if ((rc = check_starts(map->feat_start, map->n_kf, "local map: feat_start must begin at 0", "local map: feat_start must be non-decreasing")) != SNK_OK) return rc;
    SNK_REQUIRE(map->feat_start[map->n_kf] == map->n_feat, "local map: feat_start[n_kf] must be n_feat");
    for (int i = 0; i < map->n_feat; ++i)
        SNK_REQUIRE(map->feat_point[i] >= -1 && map->feat_point[i] < map->n_points, "local map: a point id outside [-1, n_points)");
    if (n_sets == 0) return SNK_OK;
    SNK_REQUIRE(frame_id != nullptr && local_kf != nullptr && sel != nullptr && set_start != nullptr && lm_pts != nullptr && lm_point != nullptr &&
                    n_pts != nullptr && out != nullptr,
                "local map: NULL array with n_sets > 0");
    if ((rc = check_starts(set_start, n_sets, "local map: set_start must begin at 0", "local map: set_start must be non-decreasing")) != SNK_OK) return rc;
    const int n_set_points = set_start[n_sets];
    SNK_REQUIRE(n_set_points == 0 || set_point != nullptr, "local map: NULL set_point with entries");
    for (int i = 0; i < n_set_points; ++i) SNK_REQUIRE(set_point[i] >= -1 && set_point[i] < map->n_points, "local map: a point id outside [-1, n_points)");
    for (int s = 0; s < n_sets; ++s)
    {
        SNK_REQUIRE(sel[s].status >= SNK_LMAP_OK && sel[s].status <= SNK_LMAP_BAD_INDEX, "local map: an unknown stage-1 status");
        if (sel[s].status != SNK_LMAP_OK) continue;
        SNK_REQUIRE(sel[s].n_local >= 0 && sel[s].n_local <= kf_cap, "local map: a stage-1 count outside [0, kf_cap]");
        long long candidates = set_start[s + 1] - set_start[s];
        for (int i = 0; i < sel[s].n_local; ++i)
        {
            const int k = local_kf[(size_t)s * (size_t)kf_cap + (size_t)i];
            SNK_REQUIRE(k >= 0 && k < map->n_kf, "local map: a local keyframe outside [0, n_kf)");
            candidates += map->feat_start[k + 1] - map->feat_start[k];
        }
        SNK_REQUIRE(candidates <= LMAP_MAX_ORDER, "local map: more than 2^30 candidates in a set");
    }
    const size_t ns = (size_t)n_sets, np = (size_t)map->n_points, cap = (size_t)pts_cap;
    Block in, out_b;
    const int i_fs = in.add(map->feat_start, ((size_t)map->n_kf + 1) * 4), i_fp = in.add(map->feat_point, (size_t)map->n_feat * 4),
              i_fl = in.add(map->pt_flags, np), i_ls = in.add(map->pt_last_seen, np * 4), i_fid = in.add(frame_id, ns * 4),
              i_lk = in.add(local_kf, ns * (size_t)kf_cap * 4), i_sel = in.add(sel, ns * sizeof(LmapSelectResult)), i_ss = in.add(set_start, (ns + 1) * 4),
              i_sp = in.add(set_point, (size_t)n_set_points * 4), i_pos = in.add(points->pos, np * 24), i_nrm = in.add(points->normal, np * 24),
              i_dsc = in.add(points->desc, np * 32), i_dep = in.add(points->ref_depth, np * 4), i_lvl = in.add(points->ref_level, np * 4);
    const size_t rec = sizeof(snk_lm_fine);
    const int o_pts = out_b.add(nullptr, ns * cap * rec), o_ids = out_b.add(nullptr, ns * cap * 4), o_n = out_b.add(nullptr, ns * 4),
              o_res = out_b.add(nullptr, ns * sizeof(LmapGatherResult));
    SNK_HIP_CHECK(hipSetDevice(m->device));
    if ((rc = stage_reserve(m, in.bytes, out_b.end())) != SNK_OK) return rc;
    if ((rc = stage_upload(m, in)) != SNK_OK) return rc;
    char *dev = m->q.as<char>(), *dout = m->out.as<char>(), *res = m->h_res.as<char>();
    snk_lmap_map dmap = *map;
    dmap.feat_start = in.at<const int32_t>(dev, i_fs), dmap.feat_point = in.at<const int32_t>(dev, i_fp), dmap.pt_flags = in.at<const uint8_t>(dev, i_fl);
    dmap.pt_last_seen = in.at<const int32_t>(dev, i_ls);
    const snk_lmap_points dpts{in.at<const double>(dev, i_pos), in.at<const double>(dev, i_nrm), in.at<const uint64_t>(dev, i_dsc), in.at<const float>(dev, i_dep),
                               in.at<const int32_t>(dev, i_lvl)};
    GatherCall C = gather_call(n_sets, &dmap, &dpts, n_set_points, kf_cap, pts_cap);
    C.frame_id   = in.at<const int>(dev, i_fid);
    C.local_kf   = in.at<const int>(dev, i_lk);
    C.sel        = in.at<const LmapSelectResult>(dev, i_sel);
    C.set_start  = in.at<const int>(dev, i_ss);
    C.set_point  = in.at<const int>(dev, i_sp);
    C.lm_pts     = out_b.at<u64>(dout, o_pts);
    C.lm_point   = out_b.at<int>(dout, o_ids);
    C.n_pts      = out_b.at<int>(dout, o_n);
    C.out        = out_b.at<LmapGatherResult>(dout, o_res);
    if ((rc = launch_gather(m, C)) != SNK_OK) return rc;
    // two steps: everything behind the records, then the records per set, n_pts of them: the words behind them were never written
    const size_t ids_at = out_b.parts[(size_t)o_ids].offset;
    if ((rc = stage_download(m, ids_at, out_b.end() - ids_at)) != SNK_OK) return rc;
    const int* got = out_b.at<const int>(res, o_n);
    for (size_t s = 0; s < ns; ++s)
        if (got[s] > 0)
            SNK_HIP_CHECK(hipMemcpyAsync(res + s * cap * rec, dout + s * cap * rec, (size_t)got[s] * rec, hipMemcpyDeviceToHost, m->stream));
    SNK_HIP_CHECK(hipStreamSynchronize(m->stream));
    for (size_t s = 0; s < ns; ++s)
        if (got[s] > 0) memcpy(lm_pts + s * cap, res + s * cap * rec, (size_t)got[s] * rec);
    memcpy(lm_point, out_b.at<char>(res, o_ids), ns * cap * 4);
    memcpy(n_pts, got, ns * 4);
    memcpy(out, out_b.at<char>(res, o_res), ns * sizeof(LmapGatherResult));
    return SNK_OK;
}

int snk_lmap_gather_batch_dev(snk_matcher* m, int n_sets, const snk_lmap_map* map_dev, const snk_lmap_points* points_dev, const int32_t* frame_id_dev,
                              const int32_t* local_kf_dev, int kf_cap, const snk_lmap_select_result* sel_dev, const int32_t* set_start_dev, int n_set_points,
                              const int32_t* set_point_dev, int pts_cap, snk_lm_fine* lm_pts_dev, int32_t* lm_point_dev, int32_t* n_pts_dev,
                              snk_lmap_gather_result* out_dev)
{
    SNK_REQUIRE(m != nullptr, "NULL handle");
    int rc;
    if ((rc = check_gather_scalars(n_sets, map_dev, points_dev, kf_cap, pts_cap)) != SNK_OK) return rc;
    SNK_REQUIRE(n_set_points >= 0, "local map: negative count");
    if (n_sets == 0) return SNK_OK;
    SNK_REQUIRE(frame_id_dev != nullptr && local_kf_dev != nullptr && sel_dev != nullptr && set_start_dev != nullptr && lm_pts_dev != nullptr &&
                    lm_point_dev != nullptr && n_pts_dev != nullptr && out_dev != nullptr,
                "local map: NULL array with n_sets > 0");
    SNK_REQUIRE(n_set_points == 0 || set_point_dev != nullptr, "local map: NULL set_point with n_set_points > 0");
    SNK_HIP_CHECK(hipSetDevice(m->device));
    GatherCall C = gather_call(n_sets, map_dev, points_dev, n_set_points, kf_cap, pts_cap);
    C.frame_id   = frame_id_dev;
    C.local_kf   = local_kf_dev;
    C.sel        = reinterpret_cast<const LmapSelectResult*>(sel_dev);
    C.set_start  = set_start_dev;
    C.set_point  = set_point_dev;
    C.lm_pts     = reinterpret_cast<u64*>(lm_pts_dev);
    C.lm_point   = lm_point_dev;
    C.n_pts      = n_pts_dev;
    C.out        = reinterpret_cast<LmapGatherResult*>(out_dev);
    return launch_gather(m, C);
}
}
