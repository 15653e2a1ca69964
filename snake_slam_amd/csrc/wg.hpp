// Workgroup-level building blocks of the map-side kernels (covis.hip, localmap.hip, scene.hip, simp.hip, bow.hip) and of the two
// sort-network kernels of track.hip / matcher.hip: one definition per job, templates over the thread count.  Device code only.
// Every function is called by all THREADS lanes of the workgroup together unless it says "a lane".  block_scan, wave_scan_incl_dpp
// and wave_sum_xor are common.hpp's.
#pragma once
#include "common.hpp"
#include "lmap_core.hpp"  // lmap_hash

#if defined(__HIPCC__)
namespace snk
{
// Ascending bitonic network over keys[0 .. n_pow2) in LDS, n_pow2 a power of two; the caller pads with an element that sorts last.
// Contract: the caller has a barrier behind its writes of keys; every stage, the last included, ends with a barrier (n_pow2 < 2: no
// stage, nothing to order).  Pair-index shape: lane t takes the pair i = ((t & ~(j-1)) << 1) | (t & (j-1)) and i | j, so every lane of
// a stage is busy.  The `i ^ j` shape (a lane per element, the upper one idle) applies the same compare-exchanges in every stage, so
// the sorted array is the same bit for bit.  less(a, b): strict; without ties the result does not depend on anything else.
template <int THREADS, class T, class Less>
__device__ __forceinline__ void block_sort(T* keys, int n_pow2, Less less)
{
    for (int k = 2; k <= n_pow2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1)
        {
            for (int t = threadIdx.x; t < (n_pow2 >> 1); t += THREADS)
            {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const T x = keys[i], y = keys[l];
                if (less(y, x) == ((i & k) == 0)) keys[i] = y, keys[l] = x;
            }
            __syncthreads();
        }
}
template <int THREADS, class T>
__device__ __forceinline__ void block_sort(T* keys, int n_pow2)
{
    block_sort<THREADS>(keys, n_pow2, [](T a, T b) { return a < b; });
}

// Exclusive prefix and total of one length per lane, 0 <= len <= 2^30.  THREADS such lengths do not fit an int: the 16-bit halves are
// summed apart, two block_scans (s_part, pass: as block_scan's).  The second scan's barrier is behind the caller's earlier LDS writes.
template <int THREADS>
__device__ __forceinline__ long long block_scan_long(int len, long long& total, unsigned* s_part, int& pass)
{
    int tot_lo, tot_hi;
    const int ex_lo = block_scan<THREADS>(len & 0xFFFF, tot_lo, s_part, pass);
    const int ex_hi = block_scan<THREADS>(len >> 16, tot_hi, s_part, pass);
    total           = ((long long)tot_hi << 16) + tot_lo;
    return ((long long)ex_hi << 16) + ex_lo;
}
// A lane: the last of the n >= 1 non-decreasing entries of prefix that is <= x (prefix[0] <= x); log2 n steps.
__device__ __forceinline__ int last_at_most(const int* prefix, int n, int x)
{
    int lo = 0, hi = n;
    while (hi - lo > 1)
    {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// op over one value per lane, returned to every lane (T: u32 or u64).  part: two banks of THREADS / 64, aligned for T; pass: the
// caller's count of reductions, 0 at first.  ONE barrier: a bank is written again two passes later, behind the barrier of the pass between.
template <int THREADS, class T, class Op>
__device__ __forceinline__ T block_reduce(T v, Op op, T* part, int& pass)
{
    static_assert(THREADS == 256, "four wavefronts");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = op(v, __shfl_xor(v, s));
    T* bank = part + (pass & 1) * (THREADS / 64);
    pass += 1;
    if (lane == 0) bank[wave] = v;
    __syncthreads();
    return op(op(bank[0], bank[1]), op(bank[2], bank[3]));
}

// ---- the first-appearance table ----
// Candidates (id p, order number ord) arrive in any order; the table answers, per id, the smallest order.  s_tab: n_slots =
// lmap_table_slots(cap) four-byte slots, a power of two, zeroed by the caller; a slot holds order + 1 in bits 0-30 (0 = free), bit 31 is
// the caller's.  The id of a slot is id_of(order): a slot's id never changes, so equal ids meet in one slot whatever the order of the
// lanes, and the table's contents as a set do not depend on the order in which atomics land.

// A lane places its candidate: linear probing from lmap_hash(p), at most n_slots steps, none of which waits for another lane.
// Returns the slot, -1 if there is none (the full flag is or was set).  seen = 0: the slot was free and holds ord + 1 now, by one
// compare-and-swap; otherwise the word read from the slot of the same id, which the caller settles (an atomic minimum, its own bit).
// The count of claims sets *full once it passes cap; candidates then stop claiming (the table keeps room for the claims in flight).
template <class IdOf>
__device__ __forceinline__ int table_place(unsigned* s_tab, int n_slots, int p, int ord, int cap, unsigned* count, unsigned* full, unsigned& seen, IdOf id_of)
{
    seen = 0;
    if (__atomic_load_n(full, __ATOMIC_RELAXED)) return -1;
    const unsigned mask = (unsigned)n_slots - 1u;
    unsigned slot       = lmap_hash(p) & mask;
    for (int probe = 0; probe < n_slots; ++probe, slot = (slot + 1) & mask)
    {
        unsigned w = __atomic_load_n(&s_tab[slot], __ATOMIC_RELAXED);
        if (w == 0)
        {
            w = atomicCAS(&s_tab[slot], 0u, (unsigned)ord + 1u);
            if (w == 0)
            {
                if ((int)atomicAdd(count, 1u) + 1 > cap) *full = 1;
                return (int)slot;
            }
        }
        if (id_of((int)(w & 0x7FFFFFFFu) - 1) == p)
        {
            seen = w;
            return (int)slot;
        }
    }
    *full = 1;
    return -1;
}
// A lane, behind the barrier that ends the placing: the word of the slot of id p, 0 if it has none.
template <class IdOf>
__device__ __forceinline__ unsigned table_find(const unsigned* s_tab, int n_slots, int p, IdOf id_of)
{
    const unsigned mask = (unsigned)n_slots - 1u;
    unsigned slot       = lmap_hash(p) & mask;
    for (int probe = 0; probe < n_slots; ++probe, slot = (slot + 1) & mask)
    {
        const unsigned w = __atomic_load_n(&s_tab[slot], __ATOMIC_RELAXED);
        if (w == 0 || id_of((int)(w & 0x7FFFFFFFu) - 1) == p) return w;
    }
    return 0;
}
// The list of first appearances in order: candidates 0 .. n_cand chunk by chunk, a candidate per lane.  A candidate with live(ord, p)
// (every such one was placed) wins iff its slot holds its order; winners are ranked by block_scan and the ones below cap are handed
// to write(ord, p, rank, slot word).  Returns the number of winners.
template <int THREADS, class IdOf, class Live, class Write>
__device__ __forceinline__ int table_emit(const unsigned* s_tab, int n_slots, int n_cand, int cap, unsigned* s_part, int& pass, IdOf id_of, Live live, Write write)
{
    int n_out = 0;
    for (int base = 0; base < n_cand; base += THREADS)  // uniform
    {
        const int ord = base + (int)threadIdx.x;
        int p         = -1;
        unsigned w    = 0;
        if (ord < n_cand)
        {
            p = id_of(ord);
            if (live(ord, p)) w = table_find(s_tab, n_slots, p, id_of);
        }
        const bool win = (w & 0x7FFFFFFFu) == (unsigned)ord + 1u;  // w = 0 never is
        int total;
        const int rank = n_out + block_scan<THREADS>(win ? 1 : 0, total, s_part, pass);
        if (win && rank < cap) write(ord, p, rank, w);
        n_out += total;
    }
    return n_out;
}

// ---- lists of very different lengths ----
// Items first .. last in rounds of one per lane.  item(i, token, a, b) -> bool: does item i have a list [a, b) to walk, and under which
// token.  A list of at most long_min entries its lane walks itself, walk_short(token, a, b).  A longer one is queued in s_queue
// [THREADS] (at most one entry per lane and round), and after a barrier each wavefront takes queued tokens in turn, walk_long(token,
// lane), a lane per entry: a 4096-entry list costs 64 steps of one wavefront instead of 4096 of a lane.  *queued (zeroed by the caller)
// is a running total that nobody resets between rounds; the second barrier of a round makes the queue the next round's.
template <int THREADS, class Item, class WalkShort, class WalkLong>
__device__ __forceinline__ void walk_lists(int first, int last, int long_min, int* s_queue, unsigned* queued, Item item, WalkShort walk_short, WalkLong walk_long)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned queued_before = 0;
    for (int base = first; base < last; base += THREADS)  // uniform
    {
        const int i = base + tid;
        int token = 0, a = 0, b = 0;
        if (i < last && item(i, token, a, b))
        {
            if (b - a > long_min) s_queue[atomicAdd(queued, 1u) - queued_before] = token;
            else walk_short(token, a, b);
        }
        __syncthreads();
        const unsigned now = *queued;
        for (int e = wave; e < (int)(now - queued_before); e += THREADS / 64) walk_long(s_queue[e], lane);
        queued_before = now;
        __syncthreads();
    }
}
}  // namespace snk
#endif
