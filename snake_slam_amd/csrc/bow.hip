// Bag-of-words place recognition for gfx950, semantics "snk-bow v1" (the deciding statements are bow_core.hpp).
// Replaces, in the order of the loop: `vocabulary.transform(descriptors, bow_vec, bow_feature_vec, 4, threads)` of Frame::computeBoW
// (reference Snake/Map/Frame.cpp:38-40), KeyframeDatabase::Add / Remove / DetectLoopCandidates / DetectRelocalizationCandidates
// (Snake/LoopClosing/KeyframeDatabase.cpp:20-168), `vocabulary.score` (Snake/LoopClosing/LoopDetector.cpp:73) and
// LoopORBmatcher::MatchBoW (Snake/LoopClosing/LoopORBMatcher.cpp:121-215).
//
// Mapping to the hardware.
//   bow_descent_kernel   16 lanes (one DPP row) per feature, one child per lane, striding when a node has more than 16 children; four
//                        popcounts per child; the packed key (distance, child number) is reduced with four DPP moves inside the row, so
//                        the first child wins a tie.  The children of a node are contiguous in memory (repacked at create): k = 10 is
//                        one 320-byte run per step.  The loop runs exactly L times for every row (rows at a leaf idle), so the DPP
//                        moves never sit under divergent control flow.
//   bow_finish_kernel    one workgroup per frame: (word, feature) and (node, feature) keys sorted in LDS by block_sort (wg.hpp), run
//                        lengths by a workgroup scan, the L1 norm by a fixed-order reduction, the division.
//   bow_db_store_kernel  copies rows of a batched transform into the slots of the database.
//   bow_db_score_kernel  brute force instead of an inverted file: one wavefront per stored keyframe looks its words up by binary search
//                        in the query's word list (LDS, 24 KB) and yields the common-word count and the L1 score in one pass.
//   bow_db_select_kernel one workgroup per query: maxCommon, the two filters, and the ordered top-k by repeated arg-max.
//   bow_match_kernel     one workgroup per keyframe pair, one wavefront per common node: the keyframe-1 features of the node serially,
//                        the lanes over the node's keyframe-2 features with the `matched` flags in LDS; then the workgroup compacts
//                        match12 into the (f1, f2) pair list snk_sim3_ransac_pairs_batch_dev takes.
// No grid barriers, no cooperative launches, no atomics, no scratch (tests/test_bow_resources.py), every loop bounded by a validated
// or clamped count.  Everything is asynchronous on the handle's stream; the host forms synchronise once to hand the result over.
#include <algorithm>
#include <cstddef>
#include <unordered_map>
#include <vector>

#include "matcher_handle.hpp"
#include "bow_core.hpp"
#include "wg.hpp"

struct snk_bow_vocab : snk::HandleBase
{
    snk::DevBuf tree;  // every array of BowTree plus word_weight, one allocation
    snk::BowTree T{};
    const double* word_weight = nullptr;  // [n_words], device
    std::vector<double> host_word_weight;
    int n_nodes = 0, n_words = 0;
    snk::DevBuf in, out;  // host forms
    snk::HostBuf h_in, h_out;
};

struct snk_bow_db
{
    snk_bow_vocab* v = nullptr;
    int max_keyframes = 0, max_words = 0, hi = 0;  // hi: slots [0, hi) have been used
    snk::DevBuf rows_w, rows_v, meta, stage, scratch, qin, qout;  // meta: row_n | live | kf_id, each [max_keyframes]
    snk::HostBuf h_q;
    std::unordered_map<int, int> slot_of;
    std::vector<int> free_slots;
};

namespace snk
{
namespace
{
using u8  = unsigned char;
using u32 = unsigned int;
using u64 = uint64_t;

constexpr int FEAT_BITS = 11;  // a feature index < BOW_MAX_FEATURES = 2048
static_assert((1 << FEAT_BITS) == BOW_MAX_FEATURES, "key layout");
constexpr u64 KEY_NONE = ~0ull;

__device__ __forceinline__ int clampi(int v, int lo, int hi)
{
    return v < lo ? lo : (v > hi ? hi : v);
}

// minimum over the 16 lanes of a DPP row, in every lane of the row (every lane of these controls has a source lane)
__device__ __forceinline__ u32 row_min_u32(u32 v)
{
    v = min(v, (u32)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xf, 0xf, true));   // quad_perm [1,0,3,2]
    v = min(v, (u32)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xf, 0xf, true));   // quad_perm [2,3,0,1]
    v = min(v, (u32)__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xf, 0xf, true));  // row_half_mirror
    v = min(v, (u32)__builtin_amdgcn_mov_dpp((int)v, 0x140, 0xf, 0xf, true));  // row_mirror
    return v;
}

__device__ __forceinline__ u32 wave_min_u32(u32 v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, (u32)__shfl_xor((int)v, d, 64));
    return v;
}

// ------------------------------------------------------------------------------------------------------------------------------
// transform
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bow_descent_kernel(BowTree T, const u64* __restrict__ desc, const int* __restrict__ n_arr, int cap,
                                                          int levelsup, int* __restrict__ word_of, int* __restrict__ node_of)
{
    const int b = blockIdx.y, row = threadIdx.x >> 4, l16 = threadIdx.x & 15;
    const int f = blockIdx.x * 16 + row;
    const int n = clampi(n_arr[b], 0, cap);
    const size_t at = (size_t)b * cap + f;
    if (blockIdx.x * 16 >= n)  // the whole workgroup lies behind the frame's features
    {
        if (l16 == 0 && f < cap)
        {
            word_of[at] = -1;
            node_of[at] = 0;
        }
        return;
    }
    const bool live = f < n;
    u64 d[4]        = {0, 0, 0, 0};
    if (live)
    {
#pragma unroll
        for (int j = 0; j < 4; ++j) d[j] = desc[at * 4 + j];
    }
    const int target = bow_node_depth(T.depth, levelsup);
    int node = 0, up = 0;
    for (int depth = 1; depth <= T.depth; ++depth)  // the same trip count for every row: the DPP moves below are never divergent
    {
        const int cnt = live ? T.count[node] : 0, first = T.first[node];
        u32 key       = BOW_NO_CHILD;
        for (int c = l16; c < cnt; c += 16)
        {
            const u32 k = bow_child_key(bow_distance(d, T.slot_desc + (size_t)(first + c) * 4), c);
            key         = k < key ? k : key;
        }
        key = row_min_u32(key);
        if (key != BOW_NO_CHILD)
        {
            node = T.slot_node[first + (int)(key & 0xfffffu)];
            if (depth == target) up = node;
        }
    }
    if (l16 == 0 && f < cap)
    {
        word_of[at] = live ? T.word[node] : -1;
        node_of[at] = live ? up : 0;
    }
}

// ---- workgroup helpers of the finish and match kernels (256 threads) ----
// exclusive prefix of one int per thread over the workgroup, and the total
__device__ __forceinline__ int block_scan_excl(int v, int* s_wave, int& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_scan_incl_dpp(v);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = 0;
    total      = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w)
    {
        before += w < wave ? s_wave[w] : 0;
        total += s_wave[w];
    }
    __syncthreads();
    return before + incl - v;
}

// s_key[0 .. m) sorted: the runs of equal (key >> FEAT_BITS).  ids[r] = the run's id, s_hpos[r] = where it starts, s_hpos[runs] = m.
__device__ __forceinline__ int block_runs(const u64* s_key, int m, int* s_hpos, int* s_wave, int* __restrict__ ids)
{
    const int i0 = threadIdx.x * 8;  // eight consecutive positions per thread: 256 * 8 = BOW_MAX_FEATURES
    int heads    = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
    {
        const int i = i0 + j;
        heads += (i < m && (i == 0 || (s_key[i] >> FEAT_BITS) != (s_key[i - 1] >> FEAT_BITS))) ? 1 : 0;
    }
    int runs;
    int r = block_scan_excl(heads, s_wave, runs);
#pragma unroll
    for (int j = 0; j < 8; ++j)
    {
        const int i = i0 + j;
        if (i < m && (i == 0 || (s_key[i] >> FEAT_BITS) != (s_key[i - 1] >> FEAT_BITS)))
        {
            s_hpos[r] = i;  // r < runs <= m <= BOW_MAX_FEATURES
            ids[r]    = (int)(s_key[i] >> FEAT_BITS);
            ++r;
        }
    }
    if (threadIdx.x == 0) s_hpos[runs] = m;
    __syncthreads();
    return runs;
}

struct BowOut
{
    int* words;        // [B][cap]
    double* values;    // [B][cap]
    int* n_words;      // [B]
    int* node_id;      // [B][cap]
    int* node_start;   // [B][cap + 1]
    int* features;     // [B][cap]
    int* n_nodes;      // [B]
};

__global__ __launch_bounds__(256) void bow_finish_kernel(const int* __restrict__ n_arr, int cap, const int* __restrict__ word_of,
                                                         const int* __restrict__ node_of, const double* __restrict__ word_weight,
                                                         int n_vocab_words, BowOut O)
{
    __shared__ u64 s_key[BOW_MAX_FEATURES];
    __shared__ int s_hpos[BOW_MAX_FEATURES + 1];
    __shared__ int s_wave[4];
    __shared__ double s_sum[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = clampi(n_arr[b], 0, cap);  // cap <= BOW_MAX_FEATURES (checked by the host)
    int N       = 1;
    while (N < n) N <<= 1;
    const size_t base = (size_t)b * cap;

    // ---- bow_vec: distinct words ascending, count * weight, L1-normalised ----
    for (int i = tid; i < N; i += 256)
    {
        const int w = i < n ? word_of[base + i] : -1;
        s_key[i]    = (w >= 0 && w < n_vocab_words) ? (((u64)w << FEAT_BITS) | (u64)i) : KEY_NONE;
    }
    __syncthreads();
    block_sort<256>(s_key, N);
    int runs = block_runs(s_key, n, s_hpos, s_wave, O.words + base);
    double part = 0.0;
    for (int r = tid; r < runs; r += 256) part += (double)(s_hpos[r + 1] - s_hpos[r]) * word_weight[(int)(s_key[s_hpos[r]] >> FEAT_BITS)];
    part = wave_sum64_dpp(part);
    if (lane == 0) s_sum[wave] = part;
    __syncthreads();
    const double norm = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
    for (int r = tid; r < runs; r += 256)
        O.values[base + r] = (double)(s_hpos[r + 1] - s_hpos[r]) * word_weight[(int)(s_key[s_hpos[r]] >> FEAT_BITS)] / norm;
    if (tid == 0) O.n_words[b] = norm > 0.0 ? runs : 0;
    __syncthreads();

    // ---- bow_feature_vec: the features of every node != 0, nodes ascending, features ascending inside a node ----
    int mine = 0;
    for (int i = tid; i < N; i += 256)
    {
        const int w = i < n ? node_of[base + i] : 0;
        s_key[i]    = w > 0 ? (((u64)w << FEAT_BITS) | (u64)i) : KEY_NONE;
        mine += w > 0 ? 1 : 0;
    }
    int m;
    (void)block_scan_excl(mine, s_wave, m);  // m = features with a node; also the barrier behind the key writes
    block_sort<256>(s_key, N);
    runs = block_runs(s_key, m, s_hpos, s_wave, O.node_id + base);
    for (int r = tid; r <= runs; r += 256) O.node_start[(size_t)b * (cap + 1) + r] = s_hpos[r];
    for (int i = tid; i < m; i += 256) O.features[base + i] = (int)(s_key[i] & (u64)(BOW_MAX_FEATURES - 1));
    if (tid == 0) O.n_nodes[b] = runs;
}

// ------------------------------------------------------------------------------------------------------------------------------
// database
// ------------------------------------------------------------------------------------------------------------------------------
struct DbRows
{
    int* words;      // [max_keyframes][max_words]
    double* values;  // [max_keyframes][max_words]
    int *row_n, *live, *kf_id;  // [max_keyframes]
    int max_keyframes, max_words;
};

// ids_slots: count keyframe ids, then count slots (checked by the host: distinct, inside [0, max_keyframes))
__global__ __launch_bounds__(256) void bow_db_store_kernel(DbRows D, const int* __restrict__ ids_slots, int count, const int* __restrict__ words,
                                                           const double* __restrict__ values, const int* __restrict__ n_words, int cap)
{
    const int i = blockIdx.x, slot = ids_slots[count + i];
    if (slot < 0 || slot >= D.max_keyframes) return;
    const int n = clampi(n_words[i], 0, min(cap, D.max_words));
    for (int k = threadIdx.x; k < n; k += 256)
    {
        D.words[(size_t)slot * D.max_words + k]  = words[(size_t)i * cap + k];
        D.values[(size_t)slot * D.max_words + k] = values[(size_t)i * cap + k];
    }
    if (threadIdx.x == 0)
    {
        D.row_n[slot] = n;
        D.kf_id[slot] = ids_slots[i];
        D.live[slot]  = 1;
    }
}

struct DbQuery
{
    const int* words;      // [Q][cap]
    const double* values;  // [Q][cap]
    const int* n_words;    // [Q]
    int cap;
    const int* exclude;    // [Q][exclude_cap] keyframe ids, may be NULL
    const int* n_exclude;  // [Q]
    int exclude_cap;
    int* common;           // [Q][hi] scratch
    double* score;         // [Q][hi] scratch
    int hi;
};

__global__ __launch_bounds__(256) void bow_db_score_kernel(DbRows D, DbQuery Qy)
{
    __shared__ int s_w[BOW_MAX_FEATURES];
    __shared__ double s_v[BOW_MAX_FEATURES];
    const int q = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nq = clampi(Qy.n_words[q], 0, min(Qy.cap, BOW_MAX_FEATURES));
    for (int i = tid; i < nq; i += 256)
    {
        s_w[i] = Qy.words[(size_t)q * Qy.cap + i];
        s_v[i] = Qy.values[(size_t)q * Qy.cap + i];
    }
    __syncthreads();
    const int slot = blockIdx.x * 4 + wave;  // wavefront-uniform
    if (slot >= Qy.hi) return;
    int common = 0;
    double sum = 0.0;
    if (D.live[slot] != 0)
    {
        const int nr = clampi(D.row_n[slot], 0, D.max_words);
        for (int i = lane; i < nr; i += 64)
        {
            const int w = D.words[(size_t)slot * D.max_words + i];
            int lo = 0, hi = nq;  // first entry >= w; at most 12 halvings
            while (lo < hi)
            {
                const int mid = (lo + hi) >> 1;
                if (s_w[mid] < w)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            if (lo < nq && s_w[lo] == w)
            {
                ++common;
                sum += bow_score_term(s_v[lo], D.values[(size_t)slot * D.max_words + i]);
            }
        }
    }
    common = wave_sum_xor(common);
    sum    = wave_sum64_dpp(sum);
    if (lane == 0)
    {
        Qy.common[(size_t)q * Qy.hi + slot] = common;
        Qy.score[(size_t)q * Qy.hi + slot]  = -0.5 * sum;
    }
}

struct DbSelect
{
    float sharing_word_ratio, score_ratio, min_score;
    int max_candidates;
    int* out_ids;        // [Q][max_candidates]
    double* out_scores;  // [Q][max_candidates]
    int* out_common;     // [Q][max_candidates]
    int* n_out;          // [Q]
};

__global__ __launch_bounds__(256) void bow_db_select_kernel(DbRows D, DbQuery Qy, DbSelect S)
{
    __shared__ int s_i[256];
    __shared__ double s_d[256];
    __shared__ int s_slot[256];
    const int q = blockIdx.x, tid = threadIdx.x;
    int* common   = Qy.common + (size_t)q * Qy.hi;
    double* score = Qy.score + (size_t)q * Qy.hi;
    const int nex  = Qy.exclude != nullptr ? clampi(Qy.n_exclude[q], 0, Qy.exclude_cap) : 0;
    const int* ex  = Qy.exclude != nullptr ? Qy.exclude + (size_t)q * Qy.exclude_cap : nullptr;

    // 1-2: the keyframes with a common word that are not excluded (a removed one has common = 0 already); maxCommon
    int mx = 0;
    for (int s = tid; s < Qy.hi; s += 256)
    {
        int c = common[s];
        if (c > 0)
        {
            const int id = D.kf_id[s];
            for (int e = 0; e < nex; ++e)
                if (ex[e] == id) c = 0;
            common[s] = c;
        }
        mx = c > mx ? c : mx;
    }
    s_i[tid] = mx;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1)
    {
        if (tid < d) s_i[tid] = max(s_i[tid], s_i[tid + d]);
        __syncthreads();
    }
    const int max_common = s_i[0];
    __syncthreads();

    // 3-4: enough common words; the best score (starts at 0, KeyframeDatabase.cpp:142)
    double best = 0.0;
    for (int s = tid; s < Qy.hi; s += 256)
    {
        const int c = common[s];
        if (c > 0 && !bow_too_few_common(c, S.sharing_word_ratio, max_common)) best = score[s] > best ? score[s] : best;
    }
    s_d[tid] = best;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1)
    {
        if (tid < d) s_d[tid] = s_d[tid] > s_d[tid + d] ? s_d[tid] : s_d[tid + d];
        __syncthreads();
    }
    best = s_d[0];
    __syncthreads();

    // 5: the score filter; a dropped keyframe gets the score -1 (scores are >= 0)
    for (int s = tid; s < Qy.hi; s += 256)
    {
        const int c     = common[s];
        const bool keep = c > 0 && !bow_too_few_common(c, S.sharing_word_ratio, max_common) &&
                          !bow_score_too_low(score[s], S.score_ratio, best, S.min_score) && score[s] >= 0.0;
        if (!keep) score[s] = -1.0;
    }
    __syncthreads();

    // 6-7: the first max_candidates in (score descending, id ascending) order: each round takes the first one behind the previous
    double prev_score = 0.0;
    int prev_id = 0, count = 0;
    for (int r = 0; r < S.max_candidates; ++r)
    {
        double bs = -1.0;
        int bid = 0, bslot = -1;
        for (int s = tid; s < Qy.hi; s += 256)
        {
            const double sc = score[s];
            if (sc < 0.0) continue;
            const int id = D.kf_id[s];
            if (r > 0 && !bow_candidate_before(prev_score, prev_id, sc, id)) continue;  // taken in an earlier round
            if (bslot < 0 || bow_candidate_before(sc, id, bs, bid))
            {
                bs    = sc;
                bid   = id;
                bslot = s;
            }
        }
        s_d[tid]    = bs;
        s_i[tid]    = bid;
        s_slot[tid] = bslot;
        __syncthreads();
        for (int d = 128; d > 0; d >>= 1)
        {
            if (tid < d)
            {
                const int o = tid + d;
                if (s_slot[o] >= 0 && (s_slot[tid] < 0 || bow_candidate_before(s_d[o], s_i[o], s_d[tid], s_i[tid])))
                {
                    s_d[tid]    = s_d[o];
                    s_i[tid]    = s_i[o];
                    s_slot[tid] = s_slot[o];
                }
            }
            __syncthreads();
        }
        const int win = s_slot[0];
        prev_score    = s_d[0];
        prev_id       = s_i[0];
        __syncthreads();
        if (win < 0) break;  // uniform: every thread read the same s_slot[0]
        if (tid == 0)
        {
            S.out_ids[(size_t)q * S.max_candidates + r]    = prev_id;
            S.out_scores[(size_t)q * S.max_candidates + r] = prev_score;
            S.out_common[(size_t)q * S.max_candidates + r] = common[win];
        }
        ++count;
    }
    if (tid == 0) S.n_out[q] = count;
}

// ------------------------------------------------------------------------------------------------------------------------------
// MatchBoW
// ------------------------------------------------------------------------------------------------------------------------------
struct MatchSide
{
    const u64* desc;    // [B][cap][4]
    const int* n;       // [B]
    const u8* has_mp;   // [B][cap]
    const int* node_id; // [B][cap]
    const int* node_start;  // [B][cap + 1]
    const int* features;    // [B][cap]
    const int* n_nodes;     // [B]
    int cap;
};

__global__ __launch_bounds__(256) void bow_match_kernel(MatchSide A, MatchSide Bs, int threshold, float ratio, int* __restrict__ match12,
                                                        int* __restrict__ pairs, int* __restrict__ n_pairs)
{
    __shared__ int s_m12[BOW_MAX_FEATURES];
    __shared__ u8 s_matched[BOW_MAX_FEATURES];
    __shared__ int s_wave[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n1 = clampi(A.n[b], 0, A.cap), n2 = clampi(Bs.n[b], 0, Bs.cap);  // caps <= BOW_MAX_FEATURES (host)
    const int nn1 = clampi(A.n_nodes[b], 0, A.cap), nn2 = clampi(Bs.n_nodes[b], 0, Bs.cap);
    const size_t a0 = (size_t)b * A.cap, b0 = (size_t)b * Bs.cap;
    const int* ns1 = A.node_start + (size_t)b * (A.cap + 1);
    const int* ns2 = Bs.node_start + (size_t)b * (Bs.cap + 1);
    volatile u8* matched = s_matched;
    for (int i = tid; i < BOW_MAX_FEATURES; i += 256)
    {
        s_m12[i]   = -1;
        matched[i] = 0;
    }
    __syncthreads();

    for (int i = wave; i < nn1; i += 4)  // one wavefront per node of keyframe 1; everything below is wavefront-uniform but the lane loop
    {
        const int node = A.node_id[a0 + i];
        int lo = 0, hi = nn2;
        while (lo < hi)
        {
            const int mid = (lo + hi) >> 1;
            if (Bs.node_id[b0 + mid] < node)
                lo = mid + 1;
            else
                hi = mid;
        }
        if (lo >= nn2 || Bs.node_id[b0 + lo] != node) continue;
        const int p0 = clampi(ns1[i], 0, A.cap), p1 = clampi(ns1[i + 1], p0, A.cap);
        const int q0 = clampi(ns2[lo], 0, Bs.cap), q1 = clampi(ns2[lo + 1], q0, Bs.cap);
        for (int p = p0; p < p1; ++p)
        {
            const int f1 = A.features[a0 + p];
            if (f1 < 0 || f1 >= n1 || A.has_mp[a0 + f1] == 0) continue;
            u64 d1[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) d1[j] = A.desc[(a0 + f1) * 4 + j];
            u32 k1 = BOW_MATCH_NONE, k2 = BOW_MATCH_NONE;
            for (int qq = q0 + lane; qq < q1; qq += 64)
            {
                const int f2 = Bs.features[b0 + qq];
                if (f2 < 0 || f2 >= n2 || Bs.has_mp[b0 + f2] == 0 || matched[f2] != 0) continue;
                bow_match_update(bow_match_key(bow_distance(d1, Bs.desc + (b0 + f2) * 4), qq - q0), k1, k2);
            }
            const u32 K1 = wave_min_u32(k1);
            const u32 K2 = wave_min_u32(k1 == K1 ? k2 : k1);  // the second smallest key: keys are distinct, one lane owns K1
            if (K1 != BOW_MATCH_NONE && bow_match_accept(K1, K2, threshold, ratio))
            {
                const int f2 = Bs.features[b0 + q0 + (int)(K1 & 0xffffu)];
                if (lane == 0)
                {
                    matched[f2] = 1;  // f2 passed the range test when its key was made
                    s_m12[f1]   = f2;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // the next feature's scan must see the flag
        }
    }
    __syncthreads();

    // match12 and the pair list, ascending in f1
    const int i0 = tid * 8;
    int mine     = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) mine += (i0 + j < A.cap && s_m12[i0 + j] >= 0) ? 1 : 0;
    int total;
    int r = block_scan_excl(mine, s_wave, total);
#pragma unroll
    for (int j = 0; j < 8; ++j)
    {
        const int f1 = i0 + j;
        if (f1 >= A.cap) continue;
        match12[a0 + f1] = s_m12[f1];
        if (s_m12[f1] >= 0)
        {
            pairs[(a0 + r) * 2]     = f1;  // r < total <= cap
            pairs[(a0 + r) * 2 + 1] = s_m12[f1];
            ++r;
        }
    }
    if (tid == 0) n_pairs[b] = total;
}

// ------------------------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------------------------
int transform_launch(snk_bow_vocab* v, const u64* desc, const int* n_dev, int batch, int cap, int levelsup, BowOut O, int* word_of, int* node_of)
{
    hipLaunchKernelGGL(bow_descent_kernel, dim3(ceil_div(cap, 16), batch), dim3(256), 0, v->stream, v->T, desc, n_dev, cap, levelsup, word_of,
                       node_of);
    SNK_LAUNCH_CHECK();
    hipLaunchKernelGGL(bow_finish_kernel, dim3(batch), dim3(256), 0, v->stream, n_dev, cap, word_of, node_of, v->word_weight, v->n_words, O);
    SNK_LAUNCH_CHECK();
    return SNK_OK;
}

DbRows db_rows(snk_bow_db* db)
{
    DbRows D;
    D.words         = db->rows_w.as<int>();
    D.values        = db->rows_v.as<double>();
    D.row_n         = db->meta.as<int>();
    D.live          = D.row_n + db->max_keyframes;
    D.kf_id         = D.live + db->max_keyframes;
    D.max_keyframes = db->max_keyframes;
    D.max_words     = db->max_words;
    return D;
}

// takes slots for `count` new ids (refuses known ids and duplicates, changes nothing then) and uploads ids | slots
int db_take_slots(snk_bow_db* db, const int32_t* kf_ids, int count)
{
    std::vector<int> ids_slots((size_t)count * 2);
    {
        std::unordered_map<int, int> seen;
        size_t free_left = db->free_slots.size();
        int fresh        = db->hi;
        for (int i = 0; i < count; ++i)
        {
            SNK_REQUIRE(kf_ids[i] >= 0, "a keyframe id is negative");
            SNK_REQUIRE(db->slot_of.find(kf_ids[i]) == db->slot_of.end() && seen.emplace(kf_ids[i], i).second, "keyframe id already in the database");
            if (free_left > 0)
                --free_left;
            else
            {
                SNK_REQUIRE(fresh < db->max_keyframes, "the database is full (max_keyframes)");
                ++fresh;
            }
        }
    }
    for (int i = 0; i < count; ++i)
    {
        int slot;
        if (!db->free_slots.empty())
        {
            slot = db->free_slots.back();
            db->free_slots.pop_back();
        }
        else
            slot = db->hi++;
        db->slot_of[kf_ids[i]] = slot;
        ids_slots[i]           = kf_ids[i];
        ids_slots[count + i]   = slot;
    }
    int rc;
    if ((rc = db->stage.reserve(ids_slots.size() * sizeof(int))) != SNK_OK) return rc;
    SNK_HIP_CHECK(hipMemcpyAsync(db->stage.p, ids_slots.data(), ids_slots.size() * sizeof(int), hipMemcpyHostToDevice, db->v->stream));
    SNK_HIP_CHECK(hipStreamSynchronize(db->v->stream));  // ids_slots is pageable and dies with this scope
    return SNK_OK;
}

int db_query_launch(snk_bow_db* db, int n_queries, const int* words, const double* values, const int* n_words, int cap, const int* exclude,
                    const int* n_exclude, int exclude_cap, float sharing_word_ratio, float score_ratio, float min_score, int max_candidates,
                    int* out_ids, double* out_scores, int* out_common, int* n_out)
{
    const int hi = db->hi > 0 ? db->hi : 1;  // an empty database still runs the select kernel, over one slot that is not live
    int rc;
    const size_t o_score = align16((size_t)n_queries * hi * sizeof(int));
    if ((rc = db->scratch.reserve(o_score + (size_t)n_queries * hi * sizeof(double))) != SNK_OK) return rc;
    DbQuery Qy;
    Qy.words = words; Qy.values = values; Qy.n_words = n_words; Qy.cap = cap;
    Qy.exclude = exclude; Qy.n_exclude = n_exclude; Qy.exclude_cap = exclude_cap;
    Qy.common = db->scratch.as<int>();
    Qy.score  = reinterpret_cast<double*>(db->scratch.as<char>() + o_score);
    Qy.hi     = hi;
    DbSelect S{sharing_word_ratio, score_ratio, min_score, max_candidates, out_ids, out_scores, out_common, n_out};
    const DbRows D = db_rows(db);
    hipLaunchKernelGGL(bow_db_score_kernel, dim3(ceil_div(hi, 4), n_queries), dim3(256), 0, db->v->stream, D, Qy);
    SNK_LAUNCH_CHECK();
    hipLaunchKernelGGL(bow_db_select_kernel, dim3(n_queries), dim3(256), 0, db->v->stream, D, Qy, S);
    SNK_LAUNCH_CHECK();
    return SNK_OK;
}

int check_query_params(float sharing_word_ratio, float score_ratio, float min_score, int max_candidates)
{
    SNK_REQUIRE(sharing_word_ratio >= 0.0f && sharing_word_ratio <= 1.0f, "sharing_word_ratio outside [0, 1]");
    SNK_REQUIRE(score_ratio >= 0.0f && score_ratio <= 1.0f, "score_ratio outside [0, 1]");
    SNK_REQUIRE(min_score >= 0.0f && min_score < INFINITY, "min_score negative or not finite");  // also refuses NaN
    SNK_REQUIRE(max_candidates >= 1 && max_candidates <= BOW_MAX_CANDIDATES, "max_candidates outside [1, 64]");
    return SNK_OK;
}

int check_sparse(const int32_t* words, const double* values, int n, int n_vocab_words, int most)
{
    SNK_REQUIRE(n >= 0 && n <= most, "too many words");
    SNK_REQUIRE(n == 0 || (words != nullptr && values != nullptr), "NULL words / values with n > 0");
    for (int i = 0; i < n; ++i)
    {
        SNK_REQUIRE(words[i] >= 0 && words[i] < n_vocab_words && (i == 0 || words[i] > words[i - 1]), "words must be strictly ascending vocabulary words");
        SNK_REQUIRE(values[i] >= 0.0 && std::isfinite(values[i]), "a value is negative or not finite");
    }
    return SNK_OK;
}
}  // namespace
}  // namespace snk

using namespace snk;

extern "C" {
int snk_bow_vocab_create(int n_nodes, const int32_t* child_start, const int32_t* child_count, const int32_t* children, int n_children,
                         const uint64_t (*desc)[4], const int32_t* word_id, const double* weight, int device, void* stream, snk_bow_vocab** out)
{
    SNK_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    SNK_REQUIRE(n_nodes >= 1 && n_nodes < (1 << 30) && child_start && child_count && desc && word_id && weight, "NULL array or no nodes");
    SNK_REQUIRE(n_children == 0 || children != nullptr, "children is NULL");
    // the tree is validated before any device is touched: no kernel ever walks an unvalidated tree
    std::vector<int32_t> depth_of((size_t)n_nodes);
    int L = 0, n_words = 0;
    const char* why = bow_validate(n_nodes, child_start, child_count, children, n_children, word_id, weight, depth_of.data(), &L, &n_words);
    if (why != nullptr)
    {
        set_error("invalid argument: vocabulary: %s", why);
        return SNK_ERR_INVALID_ARG;
    }
    snk_bow_vocab* v = new snk_bow_vocab();
    int rc           = v->init(device, stream);
    if (rc != SNK_OK)
    {
        delete v;
        return rc;
    }
    // repack: the children of a node contiguous -- slot = position in children[] -- with their descriptors beside them
    const size_t nn = (size_t)n_nodes, ns = (size_t)(n_children > 0 ? n_children : 1), nw = (size_t)n_words;
    const size_t o_first = 0, o_count = align16(o_first + nn * 4), o_snode = align16(o_count + nn * 4), o_word = align16(o_snode + ns * 4),
                 o_sdesc = align16(o_word + nn * 4), o_weight = align16(o_sdesc + ns * 32), o_ww = align16(o_weight + nn * 8),
                 bytes = o_ww + nw * 8;
    std::vector<char> host(bytes, 0);
    int32_t* first = reinterpret_cast<int32_t*>(host.data() + o_first);
    int32_t* count = reinterpret_cast<int32_t*>(host.data() + o_count);
    int32_t* snode = reinterpret_cast<int32_t*>(host.data() + o_snode);
    int32_t* word  = reinterpret_cast<int32_t*>(host.data() + o_word);
    uint64_t* sdesc = reinterpret_cast<uint64_t*>(host.data() + o_sdesc);
    double* wt     = reinterpret_cast<double*>(host.data() + o_weight);
    double* ww     = reinterpret_cast<double*>(host.data() + o_ww);
    int slot       = 0;
    for (int i = 0; i < n_nodes; ++i)
    {
        first[i] = slot;
        count[i] = child_count[i];
        word[i]  = word_id[i];
        wt[i]    = child_count[i] == 0 ? weight[i] : 0.0;
        if (child_count[i] == 0) ww[word_id[i]] = weight[i];
        for (int c = 0; c < child_count[i]; ++c, ++slot)
        {
            const int ch = children[child_start[i] + c];
            snode[slot]  = ch;
            memcpy(sdesc + (size_t)slot * 4, desc[ch], 32);
        }
    }
    v->host_word_weight.assign(ww, ww + nw);
    if ((rc = v->tree.reserve(bytes)) != SNK_OK || (rc = copy_sync(v->tree.p, host.data(), bytes, hipMemcpyHostToDevice, v->stream)) != SNK_OK)
    {
        snk_bow_vocab_destroy(v);
        return rc;
    }
    char* d        = v->tree.as<char>();
    v->T.first     = reinterpret_cast<const int32_t*>(d + o_first);
    v->T.count     = reinterpret_cast<const int32_t*>(d + o_count);
    v->T.slot_node = reinterpret_cast<const int32_t*>(d + o_snode);
    v->T.slot_desc = reinterpret_cast<const uint64_t*>(d + o_sdesc);
    v->T.word      = reinterpret_cast<const int32_t*>(d + o_word);
    v->T.weight    = reinterpret_cast<const double*>(d + o_weight);
    v->T.depth     = L;
    v->word_weight = reinterpret_cast<const double*>(d + o_ww);
    v->n_nodes     = n_nodes;
    v->n_words     = n_words;
    *out           = v;
    return SNK_OK;
}

int snk_bow_vocab_destroy(snk_bow_vocab* v)
{
    if (!v) return SNK_OK;
    (void)hipSetDevice(v->device);
    if (v->stream) (void)hipStreamSynchronize(v->stream);
    v->tree.release();
    v->in.release();
    v->out.release();
    v->h_in.release();
    v->h_out.release();
    v->fini();
    delete v;
    return SNK_OK;
}

int snk_bow_vocab_size(const snk_bow_vocab* v, int* n_words, int* n_nodes, int* depth)
{
    SNK_REQUIRE(v != nullptr, "vocabulary is NULL");
    if (n_words) *n_words = v->n_words;
    if (n_nodes) *n_nodes = v->n_nodes;
    if (depth) *depth = v->T.depth;
    return SNK_OK;
}

int snk_bow_transform_batch_dev(snk_bow_vocab* v, const snk_frames_dev* frames, int levelsup, int32_t* words_dev, double* values_dev,
                                int32_t* n_words_dev, uint32_t* node_id_dev, int32_t* node_start_dev, int32_t* features_dev,
                                int32_t* n_nodes_dev, int32_t* word_of_feature_dev, int32_t* node_of_feature_dev)
{
    SNK_REQUIRE(v != nullptr && frames != nullptr, "NULL argument");
    SNK_REQUIRE(frames->batch >= 0 && frames->batch <= 65535, "batch outside [0, 65535]");
    SNK_REQUIRE(frames->cap >= 1 && frames->cap <= BOW_MAX_FEATURES, "cap outside [1, 2048]");
    SNK_REQUIRE(levelsup >= 0, "levelsup is negative");
    SNK_REQUIRE(frames->n && frames->desc, "frames without n / desc");
    SNK_REQUIRE(words_dev && values_dev && n_words_dev && node_id_dev && node_start_dev && features_dev && n_nodes_dev && word_of_feature_dev &&
                    node_of_feature_dev,
                "NULL device buffer");
    if (frames->batch == 0) return SNK_OK;
    SNK_HIP_CHECK(hipSetDevice(v->device));
    BowOut O{words_dev, values_dev, n_words_dev, reinterpret_cast<int*>(node_id_dev), node_start_dev, features_dev, n_nodes_dev};
    return transform_launch(v, reinterpret_cast<const u64*>(frames->desc), frames->n, frames->batch, frames->cap, levelsup, O, word_of_feature_dev,
                            node_of_feature_dev);
}

int snk_bow_transform(snk_bow_vocab* v, const uint64_t (*desc)[4], int n, int levelsup, int32_t* words, double* values, int* n_words,
                      uint32_t* node_id, int32_t* node_start, int32_t* features, int* n_nodes, int32_t* word_of_feature,
                      int32_t* node_of_feature)
{
    SNK_REQUIRE(v != nullptr, "vocabulary is NULL");
    SNK_REQUIRE(n >= 0 && n <= BOW_MAX_FEATURES, "n outside [0, 2048]");
    SNK_REQUIRE(levelsup >= 0, "levelsup is negative");
    SNK_REQUIRE(n == 0 || desc != nullptr, "desc is NULL");
    SNK_REQUIRE(n_words && n_nodes && node_start, "NULL count output");
    SNK_REQUIRE(n == 0 || (words && values && node_id && features && word_of_feature && node_of_feature), "NULL output array with n > 0");
    SNK_HIP_CHECK(hipSetDevice(v->device));
    const size_t cap = (size_t)(n > 0 ? n : 1);
    // in: n (a 16-byte header, the rest zero) | desc.  out: words | node_id | node_start | features | word_of | node_of | n_words, n_nodes | values
    // through the vocabulary's own buffers and stream
    Block in, out;
    const int head[4] = {n, 0, 0, 0};
    const int i_n = in.add(head, 16), i_desc = in.add(n > 0 ? desc : nullptr, cap * 32);
    const int r_w = out.add(nullptr, cap * 4), r_nid = out.add(nullptr, cap * 4), r_ns = out.add(nullptr, (cap + 1) * 4), r_ft = out.add(nullptr, cap * 4),
              r_wof = out.add(nullptr, cap * 4), r_nof = out.add(nullptr, cap * 4), r_cnt = out.add(nullptr, 8), r_val = out.add(nullptr, cap * 8);
    int rc;
    if ((rc = stage_reserve(v->in, in.bytes, v->h_in, in.bytes, v->out, out.end(), v->h_out, out.end())) != SNK_OK) return rc;
    if ((rc = stage_upload(in, v->h_in, v->in, v->stream)) != SNK_OK) return rc;
    char* di = v->in.as<char>();
    char* d  = v->out.as<char>();
    BowOut O{out.at<int>(d, r_w),  out.at<double>(d, r_val), out.at<int>(d, r_cnt), out.at<int>(d, r_nid),
             out.at<int>(d, r_ns), out.at<int>(d, r_ft),     out.at<int>(d, r_cnt) + 1};
    if ((rc = transform_launch(v, in.at<const u64>(di, i_desc), in.at<const int>(di, i_n), 1, (int)cap, levelsup, O, out.at<int>(d, r_wof),
                               out.at<int>(d, r_nof))) != SNK_OK)
        return rc;
    if ((rc = stage_download(v->h_out, 0, v->out, 0, out.end(), v->stream)) != SNK_OK) return rc;
    char* h       = v->h_out.as<char>();
    const int* ns = out.at<const int>(h, r_ns);
    const int nw = out.at<const int>(h, r_cnt)[0], nn = out.at<const int>(h, r_cnt)[1];
    if (nw < 0 || nw > n || nn < 0 || nn > n || ns[nn] < 0 || ns[nn] > n)
    {
        set_error("bow: device returned %d words / %d nodes for %d features", nw, nn, n);
        return SNK_ERR_HIP;
    }
    *n_words = nw;
    *n_nodes = nn;
    if (nw > 0)
    {
        memcpy(words, out.at<char>(h, r_w), (size_t)nw * 4);
        memcpy(values, out.at<char>(h, r_val), (size_t)nw * 8);
    }
    memcpy(node_start, ns, (size_t)(nn + 1) * 4);
    if (nn > 0) memcpy(node_id, out.at<char>(h, r_nid), (size_t)nn * 4);
    if (n > 0)
    {
        memcpy(features, out.at<char>(h, r_ft), (size_t)ns[nn] * 4);
        memcpy(word_of_feature, out.at<char>(h, r_wof), (size_t)n * 4);
        memcpy(node_of_feature, out.at<char>(h, r_nof), (size_t)n * 4);
    }
    return SNK_OK;
}

int snk_bow_score(const snk_bow_vocab* v, const int32_t* words_a, const double* values_a, int n_a, const int32_t* words_b,
                  const double* values_b, int n_b, double* score)
{
    SNK_REQUIRE(v != nullptr && score != nullptr, "NULL argument");
    int rc;
    if ((rc = check_sparse(words_a, values_a, n_a, v->n_words, 1 << 24)) != SNK_OK) return rc;
    if ((rc = check_sparse(words_b, values_b, n_b, v->n_words, 1 << 24)) != SNK_OK) return rc;
    // two sparse vectors that live on the host: a merge of at most a few thousand entries, no launch
    double sum = 0.0;
    for (int i = 0, j = 0; i < n_a && j < n_b;)
    {
        if (words_a[i] == words_b[j])
            sum += bow_score_term(values_a[i++], values_b[j++]);
        else if (words_a[i] < words_b[j])
            ++i;
        else
            ++j;
    }
    *score = -0.5 * sum;
    return SNK_OK;
}

int snk_bow_db_create(snk_bow_vocab* v, int max_keyframes, int max_words, snk_bow_db** out)
{
    SNK_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    SNK_REQUIRE(v != nullptr, "vocabulary is NULL");
    SNK_REQUIRE(max_keyframes >= 1 && max_keyframes <= (1 << 20), "max_keyframes outside [1, 2^20]");
    SNK_REQUIRE(max_words >= 1 && max_words <= BOW_MAX_FEATURES, "max_words outside [1, 2048]");
    SNK_HIP_CHECK(hipSetDevice(v->device));
    snk_bow_db* db    = new snk_bow_db();
    db->v             = v;
    db->max_keyframes = max_keyframes;
    db->max_words     = max_words;
    const size_t rows = (size_t)max_keyframes * (size_t)max_words;
    int rc;
    if ((rc = db->rows_w.reserve(rows * 4)) != SNK_OK || (rc = db->rows_v.reserve(rows * 8)) != SNK_OK ||
        (rc = db->meta.reserve((size_t)max_keyframes * 12)) != SNK_OK)
    {
        snk_bow_db_destroy(db);
        return rc;
    }
    if (hipMemsetAsync(db->meta.p, 0, (size_t)max_keyframes * 12, v->stream) != hipSuccess || hipStreamSynchronize(v->stream) != hipSuccess)
    {
        set_error("bow: clearing the database failed");
        snk_bow_db_destroy(db);
        return SNK_ERR_HIP;
    }
    *out = db;
    return SNK_OK;
}

int snk_bow_db_destroy(snk_bow_db* db)
{
    if (!db) return SNK_OK;
    (void)hipSetDevice(db->v->device);
    (void)hipStreamSynchronize(db->v->stream);
    for (DevBuf* b : {&db->rows_w, &db->rows_v, &db->meta, &db->stage, &db->scratch, &db->qin, &db->qout}) b->release();
    db->h_q.release();
    delete db;
    return SNK_OK;
}

int snk_bow_db_add_batch_dev(snk_bow_db* db, const int32_t* kf_ids, int count, const int32_t* words_dev, const double* values_dev,
                             const int32_t* n_words_dev, int cap)
{
    SNK_REQUIRE(db != nullptr, "database is NULL");
    SNK_REQUIRE(count >= 0 && count <= 65535 && (count == 0 || kf_ids != nullptr), "bad id array");
    SNK_REQUIRE(cap >= 1 && cap <= BOW_MAX_FEATURES, "cap outside [1, 2048]");
    SNK_REQUIRE(count == 0 || (words_dev && values_dev && n_words_dev), "NULL device input");
    if (count == 0) return SNK_OK;
    SNK_HIP_CHECK(hipSetDevice(db->v->device));
    int rc;
    if ((rc = db_take_slots(db, kf_ids, count)) != SNK_OK) return rc;
    hipLaunchKernelGGL(bow_db_store_kernel, dim3(count), dim3(256), 0, db->v->stream, db_rows(db), db->stage.as<int>(), count, words_dev,
                       values_dev, n_words_dev, cap);
    SNK_LAUNCH_CHECK();
    return SNK_OK;
}

int snk_bow_db_add(snk_bow_db* db, int kf_id, const int32_t* words, const double* values, int n)
{
    SNK_REQUIRE(db != nullptr, "database is NULL");
    int rc;
    if ((rc = check_sparse(words, values, n, db->v->n_words, db->max_words)) != SNK_OK) return rc;
    SNK_REQUIRE(kf_id >= 0 && db->slot_of.find(kf_id) == db->slot_of.end(), "keyframe id negative or already in the database");
    SNK_HIP_CHECK(hipSetDevice(db->v->device));
    const size_t cap = (size_t)(n > 0 ? n : 1), o_w = 16, o_v = align16(o_w + cap * 4), bytes = o_v + cap * 8;
    if ((rc = db->qin.reserve(bytes)) != SNK_OK) return rc;
    std::vector<char> host(bytes, 0);
    *reinterpret_cast<int*>(host.data()) = n;
    if (n > 0)
    {
        memcpy(host.data() + o_w, words, (size_t)n * 4);
        memcpy(host.data() + o_v, values, (size_t)n * 8);
    }
    if ((rc = copy_sync(db->qin.p, host.data(), bytes, hipMemcpyHostToDevice, db->v->stream)) != SNK_OK) return rc;
    const char* d = db->qin.as<char>();
    return snk_bow_db_add_batch_dev(db, &kf_id, 1, reinterpret_cast<const int32_t*>(d + o_w), reinterpret_cast<const double*>(d + o_v),
                                    reinterpret_cast<const int32_t*>(d), (int)cap);
}

int snk_bow_db_remove(snk_bow_db* db, int kf_id)
{
    SNK_REQUIRE(db != nullptr, "database is NULL");
    auto it = db->slot_of.find(kf_id);
    SNK_REQUIRE(it != db->slot_of.end(), "keyframe id not in the database");
    SNK_HIP_CHECK(hipSetDevice(db->v->device));
    const int slot = it->second;
    SNK_HIP_CHECK(hipMemsetAsync(db_rows(db).live + slot, 0, sizeof(int), db->v->stream));
    db->slot_of.erase(it);
    db->free_slots.push_back(slot);
    return SNK_OK;
}

int snk_bow_db_query_batch_dev(snk_bow_db* db, int n_queries, const int32_t* words_dev, const double* values_dev, const int32_t* n_words_dev,
                               int cap, const int32_t* exclude_ids_dev, const int32_t* n_exclude_dev, int exclude_cap, float sharing_word_ratio,
                               float score_ratio, float min_score, int max_candidates, int32_t* out_ids_dev, double* out_scores_dev,
                               int32_t* out_common_dev, int32_t* n_out_dev)
{
    SNK_REQUIRE(db != nullptr, "database is NULL");
    SNK_REQUIRE(n_queries >= 0 && n_queries <= 65535, "n_queries outside [0, 65535]");
    SNK_REQUIRE(cap >= 1 && cap <= BOW_MAX_FEATURES, "cap outside [1, 2048]");
    int rc;
    if ((rc = check_query_params(sharing_word_ratio, score_ratio, min_score, max_candidates)) != SNK_OK) return rc;
    SNK_REQUIRE(exclude_ids_dev == nullptr || (n_exclude_dev != nullptr && exclude_cap >= 1), "exclude list without counts / capacity");
    if (n_queries == 0) return SNK_OK;
    SNK_REQUIRE(words_dev && values_dev && n_words_dev && out_ids_dev && out_scores_dev && out_common_dev && n_out_dev, "NULL device buffer");
    SNK_HIP_CHECK(hipSetDevice(db->v->device));
    return db_query_launch(db, n_queries, words_dev, values_dev, n_words_dev, cap, exclude_ids_dev, n_exclude_dev, exclude_cap, sharing_word_ratio,
                           score_ratio, min_score, max_candidates, out_ids_dev, out_scores_dev, out_common_dev, n_out_dev);
}

int snk_bow_db_query(snk_bow_db* db, const int32_t* words, const double* values, int n, const int32_t* exclude_ids, int n_exclude,
                     float sharing_word_ratio, float score_ratio, float min_score, int max_candidates, int32_t* out_ids, double* out_scores,
                     int32_t* out_common, int* n_out)
{
    SNK_REQUIRE(db != nullptr && n_out != nullptr, "NULL argument");
    int rc;
    if ((rc = check_sparse(words, values, n, db->v->n_words, BOW_MAX_FEATURES)) != SNK_OK) return rc;
    if ((rc = check_query_params(sharing_word_ratio, score_ratio, min_score, max_candidates)) != SNK_OK) return rc;
    SNK_REQUIRE(n_exclude >= 0 && n_exclude <= (1 << 20) && (n_exclude == 0 || exclude_ids != nullptr), "bad exclude list");
    SNK_REQUIRE(out_ids && out_scores, "NULL output array");
    SNK_HIP_CHECK(hipSetDevice(db->v->device));
    const size_t cap = (size_t)(n > 0 ? n : 1), ecap = (size_t)(n_exclude > 0 ? n_exclude : 1), mc = (size_t)max_candidates;
    // in: n, n_exclude | words | exclude | values.  out: n_out | ids | common | scores
    const size_t i_w = 16, i_e = align16(i_w + cap * 4), i_v = align16(i_e + ecap * 4), in_b = i_v + cap * 8;
    const size_t o_id = 16, o_c = o_id + mc * 4, o_s = align16(o_c + mc * 4), out_b = o_s + mc * 8;
    if ((rc = db->qin.reserve(in_b)) != SNK_OK || (rc = db->qout.reserve(out_b)) != SNK_OK || (rc = db->h_q.reserve(in_b > out_b ? in_b : out_b)) != SNK_OK)
        return rc;
    char* h = db->h_q.as<char>();
    memset(h, 0, in_b);
    reinterpret_cast<int*>(h)[0] = n;
    reinterpret_cast<int*>(h)[1] = n_exclude;
    if (n > 0)
    {
        memcpy(h + i_w, words, (size_t)n * 4);
        memcpy(h + i_v, values, (size_t)n * 8);
    }
    if (n_exclude > 0) memcpy(h + i_e, exclude_ids, (size_t)n_exclude * 4);
    char* di = db->qin.as<char>();
    char* d  = db->qout.as<char>();
    SNK_HIP_CHECK(hipMemcpyAsync(di, h, in_b, hipMemcpyHostToDevice, db->v->stream));
    if ((rc = db_query_launch(db, 1, reinterpret_cast<const int*>(di + i_w), reinterpret_cast<const double*>(di + i_v), reinterpret_cast<const int*>(di),
                              (int)cap, reinterpret_cast<const int*>(di + i_e), reinterpret_cast<const int*>(di + 4), (int)ecap, sharing_word_ratio,
                              score_ratio, min_score, max_candidates, reinterpret_cast<int*>(d + o_id), reinterpret_cast<double*>(d + o_s),
                              reinterpret_cast<int*>(d + o_c), reinterpret_cast<int*>(d))) != SNK_OK)
        return rc;
    if ((rc = copy_sync(h, d, out_b, hipMemcpyDeviceToHost, db->v->stream)) != SNK_OK) return rc;
    const int k = *reinterpret_cast<const int*>(h);
    if (k < 0 || k > max_candidates)
    {
        set_error("bow: device returned %d candidates of at most %d", k, max_candidates);
        return SNK_ERR_HIP;
    }
    *n_out = k;
    memcpy(out_ids, h + o_id, (size_t)k * 4);
    memcpy(out_scores, h + o_s, (size_t)k * 8);
    if (out_common) memcpy(out_common, h + o_c, (size_t)k * 4);
    return SNK_OK;
}

int snk_match_loop_bow_batch_dev(snk_matcher* m, const snk_frames_dev* frames1, const snk_frames_dev* frames2, const uint8_t* has_mp1_dev,
                                 const uint8_t* has_mp2_dev, const uint32_t* node_id1_dev, const int32_t* node_start1_dev,
                                 const int32_t* features1_dev, const int32_t* n_nodes1_dev, const uint32_t* node_id2_dev,
                                 const int32_t* node_start2_dev, const int32_t* features2_dev, const int32_t* n_nodes2_dev, int threshold,
                                 float ratio, int32_t* match12_dev, int32_t* pairs_dev, int32_t* n_pairs_dev)
{
    SNK_REQUIRE(m != nullptr && frames1 != nullptr && frames2 != nullptr, "NULL argument");
    SNK_REQUIRE(frames1->batch >= 0 && frames1->batch == frames2->batch, "the two frame sets must have one batch size");
    SNK_REQUIRE(frames1->cap >= 1 && frames1->cap <= BOW_MAX_FEATURES && frames2->cap >= 1 && frames2->cap <= BOW_MAX_FEATURES,
                "cap outside [1, 2048]");
    SNK_REQUIRE(frames1->n && frames1->desc && frames2->n && frames2->desc, "frames without n / desc");
    SNK_REQUIRE(threshold >= 0 && threshold <= 256, "threshold outside [0, 256]");
    SNK_REQUIRE(ratio >= 0.0f && ratio < INFINITY, "ratio negative or not finite");
    SNK_REQUIRE(has_mp1_dev && has_mp2_dev && node_id1_dev && node_start1_dev && features1_dev && n_nodes1_dev && node_id2_dev &&
                    node_start2_dev && features2_dev && n_nodes2_dev && match12_dev && pairs_dev && n_pairs_dev,
                "NULL device buffer");
    if (frames1->batch == 0) return SNK_OK;
    SNK_HIP_CHECK(hipSetDevice(m->device));
    const MatchSide A{reinterpret_cast<const u64*>(frames1->desc), frames1->n, has_mp1_dev, reinterpret_cast<const int*>(node_id1_dev),
                      node_start1_dev, features1_dev, n_nodes1_dev, frames1->cap};
    const MatchSide B{reinterpret_cast<const u64*>(frames2->desc), frames2->n, has_mp2_dev, reinterpret_cast<const int*>(node_id2_dev),
                      node_start2_dev, features2_dev, n_nodes2_dev, frames2->cap};
    hipLaunchKernelGGL(bow_match_kernel, dim3(frames1->batch), dim3(256), 0, m->stream, A, B, threshold, ratio, match12_dev, pairs_dev,
                       n_pairs_dev);
    SNK_LAUNCH_CHECK();
    return SNK_OK;
}

int snk_match_loop_bow(snk_matcher* m, const uint64_t (*desc1)[4], const uint8_t* has_mp1, int n1, const snk_bow_features* bow1,
                       const uint64_t (*desc2)[4], const uint8_t* has_mp2, int n2, const snk_bow_features* bow2, int threshold, float ratio,
                       int32_t* match12, int* n_matches)
{
    SNK_REQUIRE(m != nullptr && bow1 != nullptr && bow2 != nullptr && n_matches != nullptr, "NULL argument");
    SNK_REQUIRE(n1 >= 0 && n1 <= BOW_MAX_FEATURES && n2 >= 0 && n2 <= BOW_MAX_FEATURES, "features per keyframe outside [0, 2048]");
    SNK_REQUIRE(n1 == 0 || (desc1 && has_mp1 && match12), "NULL keyframe-1 array");
    SNK_REQUIRE(n2 == 0 || (desc2 && has_mp2), "NULL keyframe-2 array");
    const snk_bow_features* bw[2] = {bow1, bow2};
    const int nf[2]               = {n1, n2};
    for (int s = 0; s < 2; ++s)
    {
        const snk_bow_features& f = *bw[s];
        SNK_REQUIRE(f.n_nodes >= 0 && f.n_nodes <= BOW_MAX_FEATURES, "n_nodes outside [0, 2048]");  // a node's list may be empty
        SNK_REQUIRE(f.n_nodes == 0 || (f.node_id && f.node_start), "NULL feature-vector array");
        for (int i = 0; i < f.n_nodes; ++i)
        {
            SNK_REQUIRE(i == 0 || f.node_id[i] > f.node_id[i - 1], "node ids must be strictly ascending");
            SNK_REQUIRE(f.node_id[i] < 0x7fffffffu, "node id too large");
            SNK_REQUIRE(f.node_start[i] >= 0 && f.node_start[i] <= f.node_start[i + 1] && f.node_start[i + 1] <= nf[s], "node_start must ascend inside [0, n]");
        }
        SNK_REQUIRE(f.n_nodes == 0 || f.node_start[f.n_nodes] == 0 || f.features != nullptr, "NULL feature list");  // every list may be empty
    }
    SNK_HIP_CHECK(hipSetDevice(m->device));
    // per side: n, n_nodes | desc | node_id | node_start | features | has_mp
    // (every array has `cap` entries and is filled as far as the keyframe has any: the parts have no source, the rest of the block is zero)
    enum { HEAD, DESC, NODE_ID, NODE_START, FEATURES, HAS_MP };
    Block in, out;
    int part[2][6];
    size_t cap[2];
    for (int s = 0; s < 2; ++s)
    {
        cap[s] = (size_t)std::max(std::max(nf[s], bw[s]->n_nodes), 1);
        const size_t bytes[6] = {8, cap[s] * 32, cap[s] * 4, (cap[s] + 1) * 4, cap[s] * 4, cap[s]};
        for (int k = 0; k < 6; ++k) part[s][k] = in.add(nullptr, bytes[k]);
    }
    // out: n_pairs | match12 | pairs (device only)
    const int r_cnt = out.add(nullptr, 4), r_match = out.add(nullptr, cap[0] * 4), r_pairs = out.add(nullptr, cap[0] * 8);
    int rc;
    if ((rc = stage_reserve(m, in.bytes, out.end())) != SNK_OK) return rc;
    char* h = m->h_in.as<char>();
    memset(h, 0, in.bytes);
    const uint64_t (*dsc[2])[4] = {desc1, desc2};
    const uint8_t* hmp[2]       = {has_mp1, has_mp2};
    for (int s = 0; s < 2; ++s)
    {
        const snk_bow_features& f = *bw[s];
        int* head                 = in.at<int>(h, part[s][HEAD]);
        head[0]                   = nf[s];
        head[1]                   = f.n_nodes;
        if (nf[s] > 0)
        {
            memcpy(in.at<char>(h, part[s][DESC]), dsc[s], (size_t)nf[s] * 32);
            memcpy(in.at<char>(h, part[s][HAS_MP]), hmp[s], (size_t)nf[s]);
        }
        if (f.n_nodes > 0)
        {
            memcpy(in.at<char>(h, part[s][NODE_ID]), f.node_id, (size_t)f.n_nodes * 4);
            memcpy(in.at<char>(h, part[s][NODE_START]), f.node_start, (size_t)(f.n_nodes + 1) * 4);
            if (f.node_start[f.n_nodes] > 0) memcpy(in.at<char>(h, part[s][FEATURES]), f.features, (size_t)f.node_start[f.n_nodes] * 4);
        }
    }
    if ((rc = stage_upload(m, in)) != SNK_OK) return rc;
    char* d = m->q.as<char>();
    char* o = m->out.as<char>();
    MatchSide S[2];
    for (int s = 0; s < 2; ++s)
        S[s] = MatchSide{in.at<const u64>(d, part[s][DESC]),       in.at<const int>(d, part[s][HEAD]),       in.at<const u8>(d, part[s][HAS_MP]),
                         in.at<const int>(d, part[s][NODE_ID]),    in.at<const int>(d, part[s][NODE_START]), in.at<const int>(d, part[s][FEATURES]),
                         in.at<const int>(d, part[s][HEAD]) + 1,   (int)cap[s]};
    hipLaunchKernelGGL(bow_match_kernel, dim3(1), dim3(256), 0, m->stream, S[0], S[1], threshold, ratio, out.at<int>(o, r_match),
                       out.at<int>(o, r_pairs), out.at<int>(o, r_cnt));
    SNK_LAUNCH_CHECK();
    const size_t back_b = out.parts[(size_t)r_pairs].offset;  // n_pairs | match12 come back
    if ((rc = stage_download(m, 0, back_b)) != SNK_OK) return rc;
    char* back  = m->h_res.as<char>();
    const int k = *out.at<const int>(back, r_cnt);
    if (k < 0 || k > n1)
    {
        set_error("bow: device returned %d matches for %d features", k, n1);
        return SNK_ERR_HIP;
    }
    *n_matches = k;
    if (n1 > 0) memcpy(match12, out.at<char>(back, r_match), (size_t)n1 * 4);
    return SNK_OK;
}
}
