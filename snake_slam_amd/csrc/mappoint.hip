// Map-point refresh for gfx950 ("snk-mp v1") — replaces, for many points per call,
//   MapPoint::ComputeDistinctiveDescriptors   (reference Snake/Map/MapPoint.cpp:60-81)
//   MapPoint::UpdateNormal                    (reference Snake/Map/MapPoint.cpp:120-135)
//   MapPoint::UpdateDepth                     (reference Snake/Map/MapPoint.cpp:154-166)
// The per-point statements are mappoint_core.hpp's; which form a point takes is dispatch.hpp's mp_form.
//
// Mapping to the hardware.  mp_packed_kernel: a workgroup takes a chunk of 64 consecutive points; its first wavefront plans them, a
// lane per point: structural checks, the points without work answered at once, the wide ones appended to a list (one atomic per
// chunk), the others (k <= 32) packed greedily into wavefront-sized slots so that no point straddles a slot.  The descriptors of the
// chunk are staged once in LDS (32 B per row).  Then a lane is one observation row: it walks its point's descriptors out of LDS with
// v_bcnt, keeps the row of distances in 16 registers (two per register), finds the median by nine halvings of [0, 256] (no sort) and
// the point's best row by a segmented shuffle reduction of the key m << 16 | i.  The unit vectors of the normal are computed a lane
// each and summed by the point's first lane in list order (shuffles), so the sum has the sequential order of the definition.
// mp_wide_kernel: a workgroup of 1024 lanes per listed point, rows strided over the lanes; the unit vectors go through LDS and are
// summed by one lane in list order, then the descriptors are staged over them; the row of up to 4096 distances does not fit
// registers, so it is recomputed by each of three eight-way narrowing passes (mp_select8: the same element as the nine halvings); the
// key reduction runs through LDS.  No scratch; every byte of LDS is in the dynamic carve (mp_packed_carve / mp_wide_carve).  The
// device-resident entry makes no host round trip: the planner's list and its counter are read by the second launch on the device.
#include <cstddef>

#include "matcher_handle.hpp"

#include "dispatch.hpp"
#include "mappoint_core.hpp"

namespace snk
{
namespace
{
using u8  = unsigned char;
using u16 = unsigned short;
using u32 = unsigned int;
using u64 = uint64_t;

static_assert(sizeof(snk_mp_result) == 80 && offsetof(snk_mp_result, normal) == 16 && offsetof(snk_mp_result, desc) == 48, "snk_mp_result layout");
static_assert(MP_MAX_OBS == SNK_MP_MAX_OBS && MP_WIDE_MAX_K == SNK_MP_MAX_OBS, "SNK_MP_MAX_OBS");
static_assert(MP_RULE_MEDIAN == SNK_MP_MEDIAN && MP_RULE_SUM == SNK_MP_SUM && MP_DESCRIPTOR == SNK_MP_DESCRIPTOR && MP_NORMAL == SNK_MP_NORMAL &&
                  MP_DEPTH == SNK_MP_DEPTH && MP_BAD_INDEX == SNK_MP_BAD_INDEX && MP_TOO_MANY == SNK_MP_TOO_MANY,
              "snk-mp constants");
static_assert(MP_CHUNK_POINTS == 64 && MP_PACKED_MAX_K == 32 && MP_PACKED_THREADS == 256, "the packed kernel's plan: a lane per point, rows of 16 x 2 distances");
static_assert(mp_wide_carve(MP_WIDE_MAX_K) <= (size_t)LDS_MAX_BYTES && mp_packed_carve(mp_packed_rows_max()) <= (size_t)LDS_MAX_BYTES, "LDS carve");

struct MpCall
{
    int n_points, n_obs, rule, what, form_env;
    int rows_cap;  // packed rows a chunk's carve holds
    int k_cap;     // observations a wide workgroup's carve holds
    const int* obs_start;
    const u8* valid;
    const double* position;
    const int* ref_obs;
    snk_mp_result* out;
    int* wide_list;
    int* wide_count;
    // observations gathered by the host: [n_obs]
    const u64* desc;
    const double* pose;
    const int* octave;
    // observations as (kf_slot, feature) into a resident keyframe batch
    int batch, cap;
    const int* frame_n;
    const snk_kp64* kps;
    const u64* frame_desc;
    const double* frame_pose;
    const int2* obs;
};

struct MpObs
{
    const u64* desc;
    const double* pose;
    const int* octave;
};

// where observation o lives; false (and nothing read beyond the pair itself) when it points outside [0, batch) x [0, n[slot])
template <bool DEV>
__device__ __forceinline__ bool mp_locate(const MpCall& c, int o, MpObs& ob)
{
    if (DEV)
    {
        const int2 sf = c.obs[o];
        if (sf.x < 0 || sf.x >= c.batch) return false;
        int n = c.frame_n[sf.x];
        n     = n < c.cap ? n : c.cap;
        if (sf.y < 0 || sf.y >= n) return false;
        const size_t idx = (size_t)sf.x * (size_t)c.cap + (size_t)sf.y;
        ob.desc          = c.frame_desc + idx * 4;
        ob.pose          = c.frame_pose + (size_t)sf.x * 7;
        ob.octave        = &c.kps[idx].octave;
        return true;
    }
    ob.desc   = c.desc + (size_t)o * 4;
    ob.pose   = c.pose + (size_t)o * 7;
    ob.octave = c.octave + o;
    return true;
}

struct MpAnswer
{
    int best = -1, n_valid = 0, ref_level = -1, status = MP_OK;
    double normal[3] = {0, 0, 0};
    double ref_depth = 0;
};

// desc: the chosen descriptor (LDS) or nullptr
__device__ __forceinline__ void mp_write(snk_mp_result* out, const MpAnswer& a, const u64* desc)
{
    out->best      = a.best;
    out->n_valid   = a.n_valid;
    out->ref_level = a.ref_level;
    out->status    = a.status;
    out->normal[0] = a.normal[0];
    out->normal[1] = a.normal[1];
    out->normal[2] = a.normal[2];
    out->ref_depth = a.ref_depth;
#pragma unroll
    for (int w = 0; w < 4; ++w) out->desc[w] = desc ? desc[w] : 0ull;
}

__device__ __forceinline__ void mp_load_pose(const double* src, double* pose)
{
#pragma unroll
    for (int i = 0; i < 7; ++i) pose[i] = src[i];
}

// UpdateDepth for the point's reference observation (known to be in range)
template <bool DEV>
__device__ __forceinline__ void mp_depth(const MpCall& c, int o, const double* pos, MpAnswer& A)
{
    MpObs ob;
    if (!mp_locate<DEV>(c, o, ob)) return;
    double pose[7];
    mp_load_pose(ob.pose, pose);
    A.ref_depth = mp_ref_depth(pose, pos);
    A.ref_level = *ob.octave;
}

template <bool DEV>
__global__ __launch_bounds__(MP_PACKED_THREADS) void mp_packed_kernel(MpCall c)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* s_desc   = reinterpret_cast<u64*>(smem);                                  // [rows_cap][4]
    u8* s_flag    = reinterpret_cast<u8*>(smem) + (size_t)c.rows_cap * 32;         // [rows_cap]: 1 = valid, 2 = index out of range
    u16* s_map    = reinterpret_cast<u16*>(s_flag + ((c.rows_cap + 15) & ~15));    // [slots][64]: point of the chunk << 8 | observation
    int* s_row    = reinterpret_cast<int*>(s_map + MP_CHUNK_SLOTS * 64);           // [64] first row (slot * 64 + lane) of a point
    int* s_dense  = s_row + MP_CHUNK_POINTS;                                       // [64] its first row in s_desc / s_flag
    int* s_k      = s_dense + MP_CHUNK_POINTS;                                     // [64] its packed rows (0: not packed)
    int* s_a      = s_k + MP_CHUNK_POINTS;                                         // [64] obs_start
    int* s_nslots = s_a + MP_CHUNK_POINTS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int first = blockIdx.x * MP_CHUNK_POINTS;

    for (int w = tid; w < MP_CHUNK_SLOTS * 64 / 2; w += MP_PACKED_THREADS) reinterpret_cast<u32*>(s_map)[w] = 0xFFFFFFFFu;
    __syncthreads();

    if (wave == 0)
    {
        // ---- the plan: a lane per point of the chunk ----
        const int p   = first + lane;
        int a = 0, kp = 0;
        bool wide = false;
        if (p < c.n_points)
        {
            a             = c.obs_start[p];
            const int b   = c.obs_start[p + 1];
            const int k   = b - a;
            const int ref = c.ref_obs[p];
            MpAnswer A;
            if (a < 0 || b < a || b > c.n_obs) A.status = MP_BAD_INDEX;
            else if (k > MP_MAX_OBS) A.status = MP_TOO_MANY;
            else if (ref < -1 || ref >= k) A.status = MP_BAD_INDEX;
            if (A.status != MP_OK || k == 0) mp_write(c.out + p, A, nullptr);
            else if (mp_form(k, c.form_env) == MpForm::packed) kp = k;
            else wide = true;
        }
        const u64 wmask = __ballot(wide);
        if (wmask)  // uniform
        {
            int base = 0;
            if (lane == 0) base = atomicAdd(c.wide_count, __popcll(wmask));
            base = __builtin_amdgcn_readfirstlane(base);
            if (wide) c.wide_list[base + __popcll(wmask & ((1ull << lane) - 1ull))] = p;  // every point at most once: < n_points entries
        }
        // greedy packing in point order: a point that does not fit the open slot opens the next one
        int slot = 0, off = 0, dense = 0, my_row = 0, my_dense = 0;
#pragma unroll 1
        for (int q = 0; q < MP_CHUNK_POINTS; ++q)
        {
            const int kq = __builtin_amdgcn_readlane(kp, q);
            if (off + kq > 64) slot += 1, off = 0;
            if (lane == q) my_row = slot * 64 + off, my_dense = dense;
            off += kq;
            dense += kq;
        }
        if (my_dense + kp > c.rows_cap) kp = 0;  // cannot happen: rows_cap is the largest chunk's sum under the same mp_form
        s_row[lane]   = my_row;
        s_dense[lane] = my_dense;
        s_k[lane]     = kp;
        s_a[lane]     = a;
        if (lane == 0) *s_nslots = slot + (off > 0 ? 1 : 0);
        for (int i = 0; i < kp; ++i) s_map[my_row + i] = (u16)(lane << 8 | i);
    }
    __syncthreads();
    const int n_slots = *s_nslots;

    // ---- stage: flags and descriptors of the chunk's packed rows ----
    for (int r = tid; r < n_slots * 64; r += MP_PACKED_THREADS)
    {
        const u32 e = s_map[r];
        if (e == 0xFFFFu) continue;
        const int pl = e >> 8, i = e & 255;
        const int o = s_a[pl] + i, row = s_dense[pl] + i;
        const bool v = c.valid[o] != 0;
        int flag     = v ? 1 : 0;
        if (v || ((c.what & MP_DEPTH) && i == c.ref_obs[first + pl]))
        {
            MpObs ob;
            if (!mp_locate<DEV>(c, o, ob)) flag |= 2;
            else if (v && (c.what & MP_DESCRIPTOR))
            {
#pragma unroll
                for (int w = 0; w < 4; ++w) s_desc[(size_t)row * 4 + w] = ob.desc[w];
            }
        }
        s_flag[row] = (u8)flag;
    }
    __syncthreads();

    // ---- a lane per observation row ----
    for (int slot = wave; slot < n_slots; slot += MP_PACKED_THREADS / 64)
    {
        const u32 e     = s_map[slot * 64 + lane];
        const bool act  = e != 0xFFFFu;
        const int pl    = act ? (int)(e >> 8) : 0, i = act ? (int)(e & 255) : 0;
        const int k     = act ? s_k[pl] : 0;
        const int row0  = s_dense[pl];
        const int off   = lane - i;
        const int flag  = act ? s_flag[row0 + i] : 0;
        const bool vi   = (flag & 1) != 0;
        const u64 seg   = act ? ((1ull << k) - 1ull) << off : 0ull;  // k <= 32
        const bool bad  = (__ballot(act && (flag & 2)) & seg) != 0;
        const int N     = __popcll(__ballot(act && vi) & seg);
        const int p     = first + pl;
        const bool work = act && vi && !bad;
        int kmax        = k;
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) kmax = max(kmax, __shfl_xor(kmax, s));
        double pos[3] = {0, 0, 0};
        if (act)
        {
            pos[0] = c.position[(size_t)p * 3 + 0];
            pos[1] = c.position[(size_t)p * 3 + 1];
            pos[2] = c.position[(size_t)p * 3 + 2];
        }

        u32 key = 0xFFFFFFFFu;
        if (c.what & MP_DESCRIPTOR)  // uniform
        {
            u32 row[MP_PACKED_MAX_K / 2];
#pragma unroll
            for (int q = 0; q < MP_PACKED_MAX_K / 2; ++q) row[q] = 0xFFFFFFFFu;
            const u64* own = s_desc + (size_t)(row0 + i) * 4;
            u64 a0 = 0, a1 = 0, a2 = 0, a3 = 0;
            if (work) a0 = own[0], a1 = own[1], a2 = own[2], a3 = own[3];
            u32 sum = 0;
#pragma unroll
            for (int j = 0; j < MP_PACKED_MAX_K; ++j)
            {
                if (j >= kmax) break;  // uniform
                const int rj  = row0 + (j < k ? j : 0);
                const bool vj = work && j < k && (s_flag[rj] & 1);
                u32 d         = 0xFFFFu;
                if (vj)
                {
                    d = (u32)mp_hamming(a0, a1, a2, a3, s_desc + (size_t)rj * 4);
                    sum += d;
                }
                row[j >> 1] = (j & 1) ? ((row[j >> 1] & 0xFFFFu) | (d << 16)) : ((row[j >> 1] & 0xFFFF0000u) | d);
            }
            u32 m = sum;
            if (c.rule == MP_RULE_MEDIAN)
                m = (u32)mp_select(
                    [&](int v) {
                        int cnt = 0;
#pragma unroll
                        for (int q = 0; q < MP_PACKED_MAX_K / 2; ++q) cnt += ((row[q] & 0xFFFFu) <= (u32)v ? 1 : 0) + ((row[q] >> 16) <= (u32)v ? 1 : 0);
                        return cnt;
                    },
                    mp_rank(N));
            if (work) key = m << 16 | (u32)i;  // m <= 32 * 256
#pragma unroll
            for (int s = 1; s < MP_PACKED_MAX_K; s <<= 1)
            {
                const u32 other = __shfl_down(key, s);
                if (i + s < k) key = min(key, other);  // the source lane is a row of the same point
            }
        }

        double acc[3] = {0, 0, 0};
        if (c.what & MP_NORMAL)  // uniform
        {
            double u[3] = {0, 0, 0};
            if (work)
            {
                MpObs ob;
                if (mp_locate<DEV>(c, s_a[pl] + i, ob))
                {
                    double pose[7];
                    mp_load_pose(ob.pose, pose);
                    mp_view_dir(pose, pos, u);
                }
            }
            const int vflag = work ? 1 : 0;
#pragma unroll 1
            for (int j = 0; j < kmax; ++j)
            {
                const int src   = (off + j) & 63;
                const double ux = __shfl(u[0], src), uy = __shfl(u[1], src), uz = __shfl(u[2], src);
                const int vj    = __shfl(vflag, src);
                if (act && i == 0 && j < k && vj) acc[0] += ux, acc[1] += uy, acc[2] += uz;  // list order, one after the other
            }
        }

        if (act && i == 0)
        {
            MpAnswer A;
            const u64* chosen = nullptr;
            if (bad) A.status = MP_BAD_INDEX;
            else
            {
                A.n_valid = N;
                if ((c.what & MP_DESCRIPTOR) && N > 0)
                {
                    A.best = (int)(key & 0xFFFFu);
                    chosen = s_desc + (size_t)(row0 + A.best) * 4;
                }
                if (c.what & MP_NORMAL) mp_unit(acc, A.normal);
                const int ref = c.ref_obs[p];
                if ((c.what & MP_DEPTH) && ref >= 0) mp_depth<DEV>(c, s_a[pl] + ref, pos, A);
            }
            mp_write(c.out + p, A, chosen);
        }
    }
}

template <bool DEV>
__global__ __launch_bounds__(MP_WIDE_THREADS) void mp_wide_kernel(MpCall c)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* s_desc = reinterpret_cast<u64*>(smem);                             // [k_cap][4], after the normal
    double* s_u = reinterpret_cast<double*>(smem);                          // [k_cap][3], before the descriptors
    u8* s_flag  = reinterpret_cast<u8*>(smem) + (size_t)c.k_cap * 32;       // [k_cap]
    u64* s_key  = reinterpret_cast<u64*>(s_flag + ((c.k_cap + 15) & ~15));  // [wavefronts]
    int* s_int  = reinterpret_cast<int*>(s_key + MP_WIDE_THREADS / 64);     // [0] an index out of range, [1] N
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int count = *c.wide_count;
    count     = count < c.n_points ? count : c.n_points;
    for (int w = blockIdx.x; w < count; w += gridDim.x)
    {
        const int p = c.wide_list[w];
        if (p < 0 || p >= c.n_points) continue;  // uniform; the planner wrote it
        const int a = c.obs_start[p], k = c.obs_start[p + 1] - a, ref = c.ref_obs[p];
        if (k > c.k_cap || k < 1)  // uniform; cannot happen: k_cap is the largest listed point
        {
            if (tid == 0)
            {
                MpAnswer A;
                A.status = MP_TOO_MANY;
                mp_write(c.out + p, A, nullptr);
            }
            continue;
        }
        const double pos[3] = {c.position[(size_t)p * 3 + 0], c.position[(size_t)p * 3 + 1], c.position[(size_t)p * 3 + 2]};
        if (tid == 0) s_int[0] = 0;
        __syncthreads();
        for (int i = tid; i < k; i += MP_WIDE_THREADS)
        {
            const bool v = c.valid[a + i] != 0;
            int flag     = v ? 1 : 0;
            if (v || ((c.what & MP_DEPTH) && i == ref))
            {
                MpObs ob;
                if (!mp_locate<DEV>(c, a + i, ob)) flag |= 2, s_int[0] = 1;
                else if (v && (c.what & MP_NORMAL))
                {
                    double pose[7], u[3];
                    mp_load_pose(ob.pose, pose);
                    mp_view_dir(pose, pos, u);
                    s_u[(size_t)i * 3 + 0] = u[0];
                    s_u[(size_t)i * 3 + 1] = u[1];
                    s_u[(size_t)i * 3 + 2] = u[2];
                }
            }
            s_flag[i] = (u8)flag;
        }
        __syncthreads();
        const bool bad = s_int[0] != 0;
        MpAnswer A;  // thread 0's
        if (tid == 0)
        {
            if (bad) A.status = MP_BAD_INDEX;
            else
            {
                int N         = 0;
                double acc[3] = {0, 0, 0};
                const bool nr = (c.what & MP_NORMAL) != 0;
#pragma unroll 1
                for (int j = 0; j < k; ++j)  // list order, one after the other
                    if (s_flag[j] & 1)
                    {
                        N += 1;
                        if (nr) acc[0] += s_u[(size_t)j * 3 + 0], acc[1] += s_u[(size_t)j * 3 + 1], acc[2] += s_u[(size_t)j * 3 + 2];
                    }
                A.n_valid = N;
                if (nr) mp_unit(acc, A.normal);
                if ((c.what & MP_DEPTH) && ref >= 0) mp_depth<DEV>(c, a + ref, pos, A);
            }
            s_int[1] = A.n_valid;
        }
        __syncthreads();  // thread 0 is done with s_u
        const int N       = s_int[1];
        const bool select = !bad && (c.what & MP_DESCRIPTOR) && N > 0;  // uniform
        if (select)
        {
            for (int i = tid; i < k; i += MP_WIDE_THREADS)
                if (s_flag[i] & 1)
                {
                    MpObs ob;
                    if (mp_locate<DEV>(c, a + i, ob))
                    {
#pragma unroll
                        for (int q = 0; q < 4; ++q) s_desc[(size_t)i * 4 + q] = ob.desc[q];
                    }
                }
            __syncthreads();
            const int rank = mp_rank(N);
            u64 key        = ~0ull;
            for (int i = tid; i < k; i += MP_WIDE_THREADS)
            {
                if (!(s_flag[i] & 1)) continue;
                const u64 a0 = s_desc[(size_t)i * 4 + 0], a1 = s_desc[(size_t)i * 4 + 1], a2 = s_desc[(size_t)i * 4 + 2], a3 = s_desc[(size_t)i * 4 + 3];
                u64 m;
                if (c.rule == MP_RULE_SUM)
                {
                    m = 0;
#pragma unroll 1
                    for (int j = 0; j < k; ++j)
                        if (s_flag[j] & 1) m += (u64)mp_hamming(a0, a1, a2, a3, s_desc + (size_t)j * 4);
                }
                else
                    m = (u64)mp_select8(
                        [&](const int (&t)[7], int (&cnt)[7]) {
#pragma unroll
                            for (int q = 0; q < 7; ++q) cnt[q] = 0;
#pragma unroll 1
                            for (int j = 0; j < k; ++j)
                                if (s_flag[j] & 1)
                                {
                                    const int d = mp_hamming(a0, a1, a2, a3, s_desc + (size_t)j * 4);
#pragma unroll
                                    for (int q = 0; q < 7; ++q) cnt[q] += d <= t[q] ? 1 : 0;
                                }
                        },
                        rank);
                const u64 kk = m << 16 | (u64)i;
                key          = kk < key ? kk : key;
            }
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1)
            {
                const u64 other = __shfl_xor(key, s);
                key             = other < key ? other : key;
            }
            if (lane == 0) s_key[wave] = key;
            __syncthreads();
            if (tid == 0)
            {
                u64 best = s_key[0];
                for (int q = 1; q < MP_WIDE_THREADS / 64; ++q) best = s_key[q] < best ? s_key[q] : best;
                A.best = (int)(best & 0xFFFFull);
            }
        }
        if (tid == 0) mp_write(c.out + p, A, select ? s_desc + (size_t)A.best * 4 : nullptr);
        __syncthreads();  // the carve is the next point's
    }
}

int form_env()
{
    // SNK_MP_FORM=packed|wide (tests, A/B): read once
    static const int env = [] {
        const char* s = getenv("SNK_MP_FORM");
        if (!s) return 0;
        return strcmp(s, "wide") == 0 ? 2 : strcmp(s, "packed") == 0 ? 1 : 0;
    }();
    return env;
}

int check_params(const snk_mp_params* params)
{
    SNK_REQUIRE(params != nullptr, "map-point refresh: params is NULL");
    SNK_REQUIRE(params->rule == SNK_MP_MEDIAN || params->rule == SNK_MP_SUM, "map-point refresh: rule is neither SNK_MP_MEDIAN nor SNK_MP_SUM");
    SNK_REQUIRE((params->what & ~(SNK_MP_DESCRIPTOR | SNK_MP_NORMAL | SNK_MP_DEPTH)) == 0, "map-point refresh: unknown bit in `what`");
    return SNK_OK;
}

// the two launches; n_wide < 0: not known on the host
template <bool DEV>
int launch(snk_matcher* m, MpCall& C, int n_wide)
{
    int rc;
    if ((rc = m->aux.reserve((size_t)C.n_points * 4)) != SNK_OK) return rc;
    if ((rc = m->cnt.reserve(64)) != SNK_OK) return rc;
    C.wide_list  = m->aux.as<int>();
    C.wide_count = m->cnt.as<int>();
    C.form_env   = form_env();
    const void* packed = reinterpret_cast<const void*>(mp_packed_kernel<DEV>);
    const void* wide   = reinterpret_cast<const void*>(mp_wide_kernel<DEV>);
    if ((rc = set_max_lds_once(packed, (int)mp_packed_carve(mp_packed_rows_max()))) != SNK_OK) return rc;
    if ((rc = set_max_lds_once(wide, (int)mp_wide_carve(MP_WIDE_MAX_K))) != SNK_OK) return rc;
    SNK_HIP_CHECK(hipMemsetAsync(C.wide_count, 0, 4, m->stream));
    hipLaunchKernelGGL((mp_packed_kernel<DEV>), dim3(ceil_div(C.n_points, MP_CHUNK_POINTS)), dim3(MP_PACKED_THREADS), mp_packed_carve(C.rows_cap), m->stream, C);
    SNK_LAUNCH_CHECK();
    if (n_wide != 0)
    {
        const int want = n_wide < 0 ? C.n_points : n_wide;
        hipLaunchKernelGGL((mp_wide_kernel<DEV>), dim3(want < MP_WIDE_MAX_WGS ? want : MP_WIDE_MAX_WGS), dim3(MP_WIDE_THREADS), mp_wide_carve(C.k_cap), m->stream, C);
        SNK_LAUNCH_CHECK();
    }
    return SNK_OK;
}
}  // namespace
}  // namespace snk

using namespace snk;

extern "C" {
int snk_mappoint_refresh(snk_matcher* m, const snk_mp_params* params, int n_points, const int32_t* obs_start, const uint64_t (*desc)[4],
                         const double (*cam_pose)[7], const int32_t* octave, const uint8_t* valid, const double (*position)[3],
                         const int32_t* ref_obs, snk_mp_result* out)
{
    SNK_REQUIRE(m != nullptr, "NULL handle");
    int rc;
    if ((rc = check_params(params)) != SNK_OK) return rc;
    SNK_REQUIRE(n_points >= 0, "map-point refresh: negative point count");
    if (n_points == 0) return SNK_OK;
    SNK_REQUIRE(obs_start != nullptr && position != nullptr && ref_obs != nullptr && out != nullptr, "map-point refresh: NULL array with n_points > 0");
    SNK_REQUIRE(obs_start[0] == 0, "map-point refresh: obs_start[0] must be 0");
    const int fe = form_env();
    int rows_cap = 0, k_cap = 0, n_wide = 0, chunk_rows = 0;
    for (int p = 0; p < n_points; ++p)
    {
        SNK_REQUIRE(obs_start[p + 1] >= obs_start[p], "map-point refresh: obs_start must be non-decreasing");
        const int k = obs_start[p + 1] - obs_start[p];
        SNK_REQUIRE(k <= SNK_MP_MAX_OBS, "map-point refresh: a point has more than SNK_MP_MAX_OBS (4096) observations");
        SNK_REQUIRE(ref_obs[p] >= -1 && ref_obs[p] < k, "map-point refresh: ref_obs outside the point's observation list");
        if (p % MP_CHUNK_POINTS == 0) chunk_rows = 0;
        if (k > 0 && mp_form(k, fe) == MpForm::packed) chunk_rows += k, rows_cap = chunk_rows > rows_cap ? chunk_rows : rows_cap;
        else if (k > 0) n_wide += 1, k_cap = k > k_cap ? k : k_cap;
    }
    const size_t n_obs = (size_t)obs_start[n_points], np = (size_t)n_points;
    SNK_REQUIRE(n_obs == 0 || (desc != nullptr && cam_pose != nullptr && octave != nullptr && valid != nullptr), "map-point refresh: NULL observation array with observations");
    // one upload (stage.hpp): obs_start | ref_obs | position | valid | octave | cam_pose | desc
    Block in, out_b;
    const int i_start = in.add(obs_start, (np + 1) * 4), i_ref = in.add(ref_obs, np * 4), i_pos = in.add(position, np * 24), i_valid = in.add(valid, n_obs),
              i_oct = in.add(octave, n_obs * 4), i_pose = in.add(cam_pose, n_obs * 56), i_desc = in.add(desc, n_obs * 32);
    const int o_res = out_b.add(nullptr, np * sizeof(snk_mp_result));
    SNK_HIP_CHECK(hipSetDevice(m->device));
    if ((rc = stage_reserve(m, in.bytes, out_b.end())) != SNK_OK) return rc;
    if ((rc = stage_upload(m, in)) != SNK_OK) return rc;
    char* dev = m->q.as<char>();
    MpCall C{};
    C.n_points  = n_points;
    C.n_obs     = (int)n_obs;
    C.rule      = params->rule;
    C.what      = params->what;
    C.rows_cap  = rows_cap;
    C.k_cap     = k_cap;
    C.obs_start = in.at<const int>(dev, i_start);
    C.ref_obs   = in.at<const int>(dev, i_ref);
    C.position  = in.at<const double>(dev, i_pos);
    C.valid     = in.at<const u8>(dev, i_valid);
    C.octave    = in.at<const int>(dev, i_oct);
    C.pose      = in.at<const double>(dev, i_pose);
    C.desc      = in.at<const u64>(dev, i_desc);
    C.out       = out_b.at<snk_mp_result>(m->out.as<char>(), o_res);
    if ((rc = launch<false>(m, C, n_wide)) != SNK_OK) return rc;
    if ((rc = stage_download(m, 0, out_b.end())) != SNK_OK) return rc;
    memcpy(out, out_b.at<char>(m->h_res.as<char>(), o_res), np * sizeof(snk_mp_result));
    return SNK_OK;
}

int snk_mappoint_refresh_batch_dev(snk_matcher* m, const snk_mp_params* params, const snk_frames_dev* frames, const double* poses_dev,
                                   int n_points, const int32_t* obs_start_dev, int n_obs, const int32_t (*obs_dev)[2],
                                   const uint8_t* valid_dev, const double* position_dev, const int32_t* ref_obs_dev, snk_mp_result* out_dev)
{
    SNK_REQUIRE(m != nullptr, "NULL handle");
    int rc;
    if ((rc = check_params(params)) != SNK_OK) return rc;
    SNK_REQUIRE(n_points >= 0 && n_obs >= 0, "map-point refresh: negative count");
    if (n_points == 0) return SNK_OK;
    SNK_REQUIRE(frames != nullptr && frames->batch >= 0 && frames->cap >= 0, "map-point refresh: frames");
    SNK_REQUIRE(obs_start_dev != nullptr && position_dev != nullptr && ref_obs_dev != nullptr && out_dev != nullptr, "map-point refresh: NULL array with n_points > 0");
    SNK_REQUIRE(n_obs == 0 || (obs_dev != nullptr && valid_dev != nullptr), "map-point refresh: NULL observation array with n_obs > 0");
    SNK_REQUIRE(frames->batch == 0 || (frames->n != nullptr && frames->kps != nullptr && frames->desc != nullptr && poses_dev != nullptr),
                "map-point refresh: NULL keyframe array with batch > 0");
    SNK_HIP_CHECK(hipSetDevice(m->device));
    MpCall C{};
    C.n_points   = n_points;
    C.n_obs      = n_obs;
    C.rule       = params->rule;
    C.what       = params->what;
    C.rows_cap   = mp_packed_rows_max();  // the lists are not looked at on the host: the largest chunk, the largest point
    C.k_cap      = MP_WIDE_MAX_K;
    C.obs_start  = obs_start_dev;
    C.ref_obs    = ref_obs_dev;
    C.position   = position_dev;
    C.valid      = valid_dev;
    C.out        = out_dev;
    C.batch      = frames->batch;
    C.cap        = frames->cap;
    C.frame_n    = frames->n;
    C.kps        = frames->kps;
    C.frame_desc = reinterpret_cast<const u64*>(frames->desc);
    C.frame_pose = poses_dev;
    C.obs        = reinterpret_cast<const int2*>(obs_dev);
    return launch<true>(m, C, -1);
}
}
