// Scene hand-over of the bundle adjustment: snk_ba_set_problems turns the caller's scenes (snk_ba_problem: poses, points, observations
// in caller order, relative pose constraints) into the device lists every kernel of ba.hip walks, and leaves the handle ready to solve.
//
// One call is one HandOver object; its stages run in this order (snk_ba_set_problems at the end of the file):
//   check_arguments     every refusal of an argument, before anything is touched
//   reserve_lists       capacity of the pinned host lists from the totals of the call
//   size_pass           threaded: free cameras, valid observations, "more than 8 free observations on a point" per problem -> PreProb
//   place_problems      prefix sums: every problem's place in the shared lists (PreProb::*_at), the lists sized
//   fill_and_send       threaded, in chunks: values, free-camera indices, counting sort by point, the sorted observation arrays;
//                       batches send each chunk's ranges to the device as soon as they are written (copy_table_kernel)
//   build_problem_lists threaded: camera lists, point_wave work items, camera-set work items and their block lists, problem-local -> Built
//   merge_decide        serial: the Prob records, the running totals, where each problem's lists go (MergeAt), the constraints
//   merge_copy          threaded: the element copies with their relocations
//   publish_totals      the totals of the set into the handle
//   plan_block_entries  camera-pair block entries: on the device (offsets, counter budget) or by the host builder
//   upload_rest         the remaining lists into the upload table
//   reserve_work        the solver's work arrays, the PCG plan (ba_plan_pcg in ba.hip)
//   zero_and_launch     the zero entries, copy_table_kernel, then the lists the device derives: derive_obs_fields, derive_cam_items,
//                       gather_cam_records, gather_set_records, block_entries_count / _scan / _fill
//   check_lists         SNK_BA_CHECK_LISTS=1: the device-built lists against the host builder and the caller's arrays
//   report              SNK_BA_PROFILE_CREATE=1: the two [snk_ba_set_problems] lines
// snk_ba_set_problems_dev takes the scenes as device rows (snk_scene_out): dev_stage -- ho_count_kernel, a read-back, ho_fill_kernel, a
// read-back -- stands where size_pass, place_problems and fill_and_send do, dev_check compares it with them under SNK_BA_CHECK_LISTS=1,
// and build_problem_lists .. report run unchanged on a host shadow of the problems.  Batches the kernels do not take (handover_core.hpp)
// are copied down (RowsOnHost) and go through the stages above.
// A stage that fails returns the error code; the guard in snk_ba_set_problems then leaves the handle without a problem set.
#include "ba_types.hpp"

#include <atomic>
#include <chrono>
#include <unordered_map>

// This file is compiled with -ffp-contract=fast like ba.hip (snake_slam_amd/build.py): its kernels were part of that file.

namespace snk
{
using namespace ba;
namespace
{
// ---- scene lists built on the device -------------------------------------------------------------------------------------------
// The static per-camera observation records (what cam_pass streams) are a gather of the sorted observation arrays through the
// camera lists: 40 bytes per observation that neither the host loop nor the bus has to touch.
// Batches (round 6): three of the sorted observation arrays and the camera lists are functions of arrays that are on the device anyway --
// 13 of the 53 bytes per observation a hand-over used to carry over the bus (210 MB of a 1024-window batch's 1.07 GB).
//   o_pt[s]     = the point whose run [pt_start[p], pt_start[p + 1]) holds s (binary search),
//   o_cam[s]    = cam_idx[o_img[s]],   o_ptfree[s] = !pt_const[o_pt[s]]
__global__ __launch_bounds__(256) void derive_obs_fields(Arrays A, int* __restrict__ o_pt, int* __restrict__ o_cam, unsigned char* __restrict__ o_ptfree)
{
    const Prob pr = A.prob[blockIdx.y];
    const int s   = blockIdx.x * 256 + threadIdx.x;
    if (s >= pr.no) return;
    const int* ps = A.pt_start + pr.ptstart_off;
    int lo = 0, hi = pr.np;  // ps[lo] <= s < ps[hi]
    while (hi - lo > 1)
    {
        const int mid = (lo + hi) >> 1;
        if (ps[mid] <= s) lo = mid;
        else hi = mid;
    }
    const int go  = pr.obs_off + s;
    o_pt[go]      = lo;
    o_cam[go]     = A.cam_idx[pr.img_off + A.o_img[go]];
    o_ptfree[go]  = A.pt_const[pr.pt_off + lo] ? 0 : 1;
}
// cam_items of camera c = the observations s with o_cam[s] == c in ascending s (the host builder's order): one wavefront per (camera,
// problem) walks the observations 64 at a time and compacts by ballot.  cam_start comes from the host (nfc + 1 ints per problem).
__global__ __launch_bounds__(64) void derive_cam_items(Arrays A, const int* __restrict__ o_cam, int* __restrict__ cam_items)
{
    const Prob pr = A.prob[blockIdx.y];
    const int c   = blockIdx.x;
    if (c >= pr.nfc) return;
    const int lane = threadIdx.x;
    int at = pr.citem_off + A.cam_start[pr.camstart_off + c];
    for (int s0 = 0; s0 < pr.no; s0 += 64)
    {
        const int s    = s0 + lane;
        const bool hit = s < pr.no && o_cam[pr.obs_off + s] == c;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
        if (hit) cam_items[at + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] = s;
        at += __popcll(m);
    }
}

__global__ __launch_bounds__(256) void gather_cam_records(Arrays A, CamObs* __restrict__ out)
{
    const Prob pr = A.prob[blockIdx.y];
    const int n   = A.cam_start[pr.camstart_off + pr.nfc];
    const int k   = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int go = pr.obs_off + A.cam_items[pr.citem_off + k];
    const double2 uv = A.o_uv[go];
    CamObs rec;
    rec.u = uv.x; rec.v = uv.y; rec.depth = A.o_depth[go]; rec.weight = A.o_weight[go];
    rec.ptw = A.o_pt[go] | (A.o_ptfree[go] ? (int)0x80000000u : 0); rec.orig = A.o_orig[go];
    out[pr.citem_off + k] = rec;
}

// The static observation records in the order schur_fused / update_cost walk them (work item, point of the item, observation of
// the point) are a gather as well: 48 bytes per observation that the host loop wrote one by one and the bus carried (786 KB per
// benchmark window -- half of a batch's upload).  One workgroup per work item.
__global__ __launch_bounds__(256) void gather_set_records(Arrays A, SetObs* __restrict__ out)
{
    const Prob pr = A.prob[blockIdx.y];
    if ((int)blockIdx.x >= pr.n_set) return;
    const SetItem si = A.set_items[pr.set_off + blockIdx.x];
    const int n      = si.n_pts * si.run;
    for (int idx = threadIdx.x; idx < n; idx += 256)
    {
        const int q = idx / si.run, a = idx - q * si.run;
        const int go = pr.obs_off + A.set_pts[si.pts_off + q].y + a;
        const double2 uv = A.o_uv[go];
        SetObs rec;
        rec.u = uv.x; rec.v = uv.y; rec.depth = A.o_depth[go]; rec.weight = A.o_weight[go];
        rec.orig = A.o_orig[go]; rec.pk = set_pack(A.o_img[go], A.o_cam[go], A.o_ptfree[go]);
        out[(size_t)si.rec_off + idx] = rec;
    }
}

// The camera-pair block entries of schur_pass -- for every upper block (c1, c2) the co-observations (observation of c1,
// observation of c2, point) in ascending order -- built by three launches instead of a host loop over every pair of every
// point (half of a scene hand-over's host time, and 1.1 MB over the bus for a 20 x 2000 x 8 window).  Requirements (checked
// on the host, which keeps its own builder for the other scenes): <= BE_MAX_CAMS free cameras, no camera twice on a point.
// One wavefront per (camera c1, 64 items of its list): lane = one observation a of c1; the free cameras >= c1 in its point's
// run are a bit mask (BE_WORDS x 64 bits in registers); ballot(c2 in mask) ranks the lane inside the chunk for block (c1, c2).
// Order inside a block = list order of c1 = ascending observation index = ascending point: the host builder's order.
constexpr int BE_WORDS = 8, BE_MAX_CAMS = 64 * BE_WORDS;
static_assert(BE_MAX_CAMS == HO_DUP_MAX_CAMS, "the dup rule of handover_core.hpp covers the cameras the device builder takes");
__device__ inline void block_entry_item(const Arrays& A, const Prob& pr, int c1, int chunk, int lane, int& a, int& p, int& r0, int& r1,
                                        unsigned long long (&mask)[BE_WORDS])
{
    const int s0 = A.cam_start[pr.camstart_off + c1], s1 = A.cam_start[pr.camstart_off + c1 + 1];
    const int k  = s0 + chunk * 64 + lane;
    a = -1, p = 0, r0 = 0, r1 = 0;
#pragma unroll
    for (int w = 0; w < BE_WORDS; ++w) mask[w] = 0ull;
    if (k >= s1) return;
    const int s  = A.cam_items[pr.citem_off + k];
    const int go = pr.obs_off + s;
    if (!A.o_ptfree[go]) return;  // constant points produce no Schur products
    a  = s;
    p  = A.o_pt[go];
    r0 = A.pt_start[pr.ptstart_off + p], r1 = A.pt_start[pr.ptstart_off + p + 1];
    for (int c = r0; c < r1; ++c)
    {
        const int cc = A.o_cam[pr.obs_off + c];
        if (cc < c1) continue;
        const unsigned long long bit = 1ull << (cc & 63);
#pragma unroll
        for (int w = 0; w < BE_WORDS; ++w)
            if (w == (cc >> 6)) mask[w] |= bit;
    }
}

__global__ __launch_bounds__(64) void block_entries_count(Arrays A, int* __restrict__ cnt)
{
    const Prob pr = A.prob[blockIdx.y];
    const int w0  = blockIdx.x;
    if (pr.be_nch <= 0 || w0 >= pr.nfc * pr.be_nch) return;
    const int c1 = w0 / pr.be_nch, chunk = w0 - c1 * pr.be_nch, lane = threadIdx.x;
    int a, p, r0, r1;
    unsigned long long mask[BE_WORDS];
    block_entry_item(A, pr, c1, chunk, lane, a, p, r0, r1, mask);
    int* out = cnt + pr.becnt_off + (size_t)(c1 * pr.be_nch + chunk) * pr.nfc;
#pragma unroll
    for (int w = 0; w < BE_WORDS; ++w)
    {
        if (w * 64 >= pr.nfc) break;  // uniform
        int mine = 0;
        if (__builtin_amdgcn_ballot_w64(mask[w] != 0ull) != 0ull)  // uniform: most words of a big scene are empty
            for (int b = 0; b < 64; ++b)
            {
                const unsigned long long m = __builtin_amdgcn_ballot_w64((mask[w] >> b) & 1ull);
                if (lane == b) mine = __popcll(m);
            }
        if (w * 64 + lane < pr.nfc) out[w * 64 + lane] = mine;  // (cameras below c1 are in no mask: zeros)
    }
}

// per problem: chunk counts -> chunk bases (in place), block totals -> blk_start (exclusive scan over the nfc * nfc blocks)
constexpr int BE_SCAN_THREADS = 1024;
__global__ __launch_bounds__(BE_SCAN_THREADS) void block_entries_scan(Arrays A, int* __restrict__ cnt, int* __restrict__ blk_start)
{
    __shared__ int s_wave[BE_SCAN_THREADS / 64];
    __shared__ int s_run;
    const Prob pr = A.prob[blockIdx.x];
    const int nb = pr.nfc * pr.nfc, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_run = 0;
    __syncthreads();
    for (int base = 0; base < nb; base += BE_SCAN_THREADS)
    {
        const int blk = base + tid;
        int tot = 0;
        if (blk < nb && pr.be_nch > 0)
        {
            const int c1 = blk / pr.nfc, c2 = blk - c1 * pr.nfc;
            if (c2 >= c1)  // the lower blocks have no entries (and their counters were never written)
                for (int ch = 0; ch < pr.be_nch; ++ch)
                {
                    int* q = cnt + pr.becnt_off + (size_t)(c1 * pr.be_nch + ch) * pr.nfc + c2;
                    const int v = *q;
                    *q = tot;
                    tot += v;
                }
        }
        // inclusive scan: inside the wavefront by shuffles, then the wavefront totals
        int incl = tot;
        incl = wave_scan_incl_dpp(incl);
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int before = 0;
        for (int w = 0; w < wave; ++w) before += s_wave[w];
        const int run = s_run;
        if (blk < nb) blk_start[pr.blkstart_off + blk] = run + before + incl - tot;
        __syncthreads();
        if (tid == BE_SCAN_THREADS - 1) s_run = run + before + incl;
        __syncthreads();
    }
    if (tid == 0) blk_start[pr.blkstart_off + nb] = s_run;
}

__global__ __launch_bounds__(64) void block_entries_fill(Arrays A, const int* __restrict__ cnt, int4* __restrict__ blk_ent)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char be_smem[];
    const Prob pr = A.prob[blockIdx.y];
    const int w0  = blockIdx.x;
    if (pr.be_nch <= 0 || w0 >= pr.nfc * pr.be_nch) return;
    unsigned long long* s_ball = reinterpret_cast<unsigned long long*>(be_smem);  // [words * 64] ballots per camera c2
    const int nwords = (pr.nfc + 63) >> 6;
    int* s_base = reinterpret_cast<int*>(s_ball + nwords * 64);                     // [words * 64] first entry of (c1, chunk, c2)
    const int c1 = w0 / pr.be_nch, chunk = w0 - c1 * pr.be_nch, lane = threadIdx.x;
    int a, p, r0, r1;
    unsigned long long mask[BE_WORDS];
    block_entry_item(A, pr, c1, chunk, lane, a, p, r0, r1, mask);
    const int* cin = cnt + pr.becnt_off + (size_t)(c1 * pr.be_nch + chunk) * pr.nfc;
#pragma unroll
    for (int w = 0; w < BE_WORDS; ++w)
    {
        if (w * 64 >= pr.nfc) break;  // uniform
        unsigned long long mine = 0ull;
        if (__builtin_amdgcn_ballot_w64(mask[w] != 0ull) != 0ull)
            for (int b = 0; b < 64; ++b)
            {
                const unsigned long long m = __builtin_amdgcn_ballot_w64((mask[w] >> b) & 1ull);
                if (lane == b) mine = m;
            }
        const int c2 = w * 64 + lane;
        s_ball[c2] = mine;
        s_base[c2] = c2 >= c1 && c2 < pr.nfc ? A.blk_start[pr.blkstart_off + c1 * pr.nfc + c2] + cin[c2] : 0;
    }
    __syncthreads();
    if (a < 0) return;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int c = r0; c < r1; ++c)
    {
        const int cc = A.o_cam[pr.obs_off + c];
        if (cc < c1) continue;
        blk_ent[(size_t)pr.ent_off + s_base[cc] + __popcll(s_ball[cc] & below)] = make_int4(a, c, p, 0);
    }
}
__global__ __launch_bounds__(256) void copy_table_kernel(CopyTab T)
{
    const int e = blockIdx.y;
    const unsigned nb = T.bytes[e], nq = nb >> 4;
    const uint4* s4 = static_cast<const uint4*>(T.src[e]);  // both sides are at least 256-byte aligned (hipHostMalloc / hipMalloc)
    uint4* d4       = static_cast<uint4*>(T.dst[e]);
    if (s4 == nullptr)  // a buffer that starts as zeros
    {
        for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < nq; i += gridDim.x * 256u) d4[i] = make_uint4(0u, 0u, 0u, 0u);
        if (blockIdx.x == 0)
            for (unsigned i = (nq << 4) + threadIdx.x; i < nb; i += 256u) static_cast<unsigned char*>(T.dst[e])[i] = 0;
        return;
    }
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < nq; i += gridDim.x * 256u) d4[i] = s4[i];
    if (blockIdx.x == 0)
    {
        const unsigned char* sb = static_cast<const unsigned char*>(T.src[e]);
        unsigned char* db       = static_cast<unsigned char*>(T.dst[e]);
        for (unsigned i = (nq << 4) + threadIdx.x; i < nb; i += 256u) db[i] = sb[i];
    }
}
template <typename V>
int upload(DevBuf& b, const V& v, CopyTab& tab)
{
    using T = typename V::value_type;
    int rc  = b.reserve(std::max<size_t>(v.size(), 1) * sizeof(T));
    if (rc != SNK_OK) return rc;
    if (v.empty()) return SNK_OK;
    SNK_REQUIRE(tab.n < COPY_TAB_MAX && v.size() * sizeof(T) < (1ull << 32), "scene list too large for the upload table");
    tab.src[tab.n]   = v.data();
    tab.dst[tab.n]   = b.p;
    tab.bytes[tab.n] = (unsigned)(v.size() * sizeof(T));
    ++tab.n;
    return SNK_OK;
}

// ---- the device stage of snk_ba_set_problems_dev ---------------------------------------------------------------------------------
// The caller's rows are on the device (snk_scene_out): what size_pass, place_problems and fill_problem do on the host threads -- and the
// bus carries up afterwards -- is done by two kernels, one workgroup per problem, with the rules of handover_core.hpp.  The host reads
// back what its later stages need (camidx, pt_const, ptstart, the sorted o_cam, five ints per problem) and places the problems between
// the two launches.  Nothing is placed by the return value of an atomic: the histogram's LDS additions commute, and the order inside a
// point is the caller's by construction (chunks in order, ho_chunk_rank inside a chunk).
struct HoRows  // the rows of snk_scene_out that are read
{
    int img_cap, pt_cap, obs_cap;
    const double* pose;
    const uint8_t* img_const;
    const double* pt;
    const uint8_t* pt_const;
    const int* obs_img;
    const int* obs_pt;
    const double* obs_uv;
    const double* obs_depth;
    const double* obs_weight;
};

// values, free-camera indices, valid observations per point -> pt_start; HoOut::nfc / no / k_over8 / long_run
__global__ __launch_bounds__(HO_THREADS) void ho_count_kernel(HoRows R, const HoPlace* __restrict__ place, HoOut* __restrict__ out, double* __restrict__ d_pose,
                                                              double* __restrict__ d_pt, unsigned char* __restrict__ d_ptc, int* __restrict__ d_camidx,
                                                              int* __restrict__ d_ptstart)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ho_smem[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const HoPlace pl = place[b];
    unsigned* s_misc = reinterpret_cast<unsigned*>(ho_smem);  // [0, 8) block_scan, [8] k_over8, [9] long_run
    int* s_cnt  = reinterpret_cast<int*>(s_misc + HO_MISC);   // [n_pt] valid observations
    int* s_free = s_cnt + pl.n_pt;                             // [n_pt] observations by free cameras
    const size_t ri = (size_t)b * R.img_cap, rp = (size_t)b * R.pt_cap, ro = (size_t)b * R.obs_cap;
    const uint8_t* img_const = R.img_const + ri;
    const uint8_t* pt_const  = R.pt_const + rp;
    for (int k = tid; k < 7 * pl.n_img; k += HO_THREADS) d_pose[7 * (size_t)pl.img_at + k] = R.pose[7 * ri + k];
    for (int k = tid; k < 3 * pl.n_pt; k += HO_THREADS) d_pt[3 * (size_t)pl.pt_at + k] = R.pt[3 * rp + k];
    for (int p = tid; p < pl.n_pt; p += HO_THREADS)
    {
        d_ptc[(size_t)pl.pt_at + p] = pt_const[p] ? 1 : 0;
        s_cnt[p] = 0, s_free[p] = 0;
    }
    if (tid == 0) s_misc[8] = 0u, s_misc[9] = 0u;
    int pass = 0, nfc = 0;
    for (int i0 = 0; i0 < pl.n_img; i0 += HO_THREADS)  // (uniform trip count: every lane scans)
    {
        const int i    = i0 + tid;
        const int free = i < pl.n_img && !img_const[i] ? 1 : 0;
        int tot;
        const int before = block_scan<HO_THREADS>(free, tot, s_misc, pass);
        if (i < pl.n_img) d_camidx[(size_t)pl.img_at + i] = ho_cam_index(!free, nfc + before);
        nfc += tot;
    }
    __syncthreads();
    for (int o = tid; o < pl.n_obs; o += HO_THREADS)
    {
        const int i = R.obs_img[ro + o], p = R.obs_pt[ro + o];
        if (ho_obs_valid(i, p, pl.n_img, pl.n_pt, img_const, pt_const)) atomicAdd(&s_cnt[p], 1);
        if (ho_obs_by_free_camera(i, p, pl.n_img, pl.n_pt, img_const)) atomicAdd(&s_free[p], 1);
    }
    __syncthreads();
    int no = 0;
    for (int p0 = 0; p0 < pl.n_pt; p0 += HO_THREADS)
    {
        const int p = p0 + tid;
        const int v = p < pl.n_pt ? s_cnt[p] : 0;
        int tot;
        const int before = block_scan<HO_THREADS>(v, tot, s_misc, pass);
        if (p < pl.n_pt)
        {
            d_ptstart[(size_t)pl.ps_at + p] = no + before;
            if (ho_k_over8(s_free[p])) s_misc[8] = 1u;  // (every writer writes the same word)
            if (!ho_run_taken(v)) s_misc[9] = 1u;
        }
        no += tot;
    }
    __syncthreads();
    if (tid == 0)
    {
        d_ptstart[(size_t)pl.ps_at + pl.n_pt] = no;
        HoOut r;
        r.nfc = nfc, r.no = no, r.k_over8 = (int)s_misc[8], r.long_run = (int)s_misc[9], r.dup = 0;
        out[b] = r;
    }
}

// the sorted observation arrays (and o_cam, which the host's readback needs before the problem table exists); HoOut::dup
__global__ __launch_bounds__(HO_THREADS) void ho_fill_kernel(HoRows R, const HoPlace* __restrict__ place, HoOut* __restrict__ out, const int* __restrict__ d_camidx,
                                                             const int* __restrict__ d_ptstart, int* __restrict__ o_img, int* o_cam, double2* __restrict__ o_uv,
                                                             double* __restrict__ o_depth, double* __restrict__ o_weight, int* __restrict__ o_orig)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ho_smem[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const HoPlace pl = place[b];
    const HoOut cnt  = out[b];  // what ho_count_kernel left
    unsigned* s_misc = reinterpret_cast<unsigned*>(ho_smem);  // [0] dup
    int* s_keys = reinterpret_cast<int*>(s_misc + HO_MISC);   // [HO_THREADS] the chunk's points, -1: not valid
    int* s_cur  = s_keys + HO_THREADS;                        // [n_pt] next free slot of the point
    const size_t ri = (size_t)b * R.img_cap, rp = (size_t)b * R.pt_cap, ro = (size_t)b * R.obs_cap;
    const uint8_t* img_const = R.img_const + ri;
    const uint8_t* pt_const  = R.pt_const + rp;
    const int* cidx          = d_camidx + pl.img_at;
    for (int p = tid; p < pl.n_pt; p += HO_THREADS) s_cur[p] = d_ptstart[(size_t)pl.ps_at + p];
    if (tid == 0) s_misc[0] = 0u;
    __syncthreads();
    for (int c0 = 0; c0 < pl.n_obs; c0 += HO_THREADS)  // consecutive chunks in caller order
    {
        const int o = c0 + tid;
        int i = 0, p = 0;
        bool valid = false;
        if (o < pl.n_obs)
        {
            i = R.obs_img[ro + o], p = R.obs_pt[ro + o];
            valid = ho_obs_valid(i, p, pl.n_img, pl.n_pt, img_const, pt_const);
        }
        s_keys[tid] = valid ? p : -1;
        __syncthreads();
        int before = 0, total = 0, base = 0;
        if (valid)
        {
            ho_chunk_rank(s_keys, HO_THREADS / 4, tid, before, total);
            base = s_cur[p];
        }
        __syncthreads();  // every cursor of the chunk is read, every key compared
        if (valid)
        {
            if (before + 1 == total) s_cur[p] = base + total;  // the point's last observation of the chunk: one writer per cursor
            const size_t go = (size_t)pl.obs_at + base + before;
            if (base + before >= cnt.no) continue;  // (rows that changed between the two kernels: never outside the problem's range)
            o_img[go]    = i;
            o_cam[go]    = cidx[i];
            o_uv[go]     = make_double2(R.obs_uv[2 * (ro + o)], R.obs_uv[2 * (ro + o) + 1]);
            o_depth[go]  = R.obs_depth[ro + o];
            o_weight[go] = R.obs_weight[ro + o];
            o_orig[go]   = pl.orig_at + o;
        }
    }
    __threadfence_block();
    __syncthreads();  // s_cur[p] is now the END of point p's run; the workgroup's o_cam is written
    if (ho_dup_words(cnt.nfc) > 0)
        for (int s = tid; s < cnt.no; s += HO_THREADS)
        {
            int lo = -1, hi = pl.n_pt - 1;  // the smallest p with s_cur[p] > s: end(lo) <= s < end(hi)
            while (hi - lo > 1)
            {
                const int mid = (lo + hi) >> 1;
                if (s_cur[mid] <= s) lo = mid;
                else hi = mid;
            }
            const int begin = hi > 0 ? s_cur[hi - 1] : 0;
            if (ho_cam_seen_before(o_cam + pl.obs_at, begin, s)) s_misc[0] = 1u;
        }
    __syncthreads();
    if (tid == 0) out[b].dup = (int)s_misc[0];
}

// ---- what the stages hand to each other ----

// Written by size_pass (nfc, no, k_over8), place_problems (*_at) and fill_problem (dup); read by every later stage.
struct PreProb
{
    int nfc, no;  // free cameras, valid observations
    size_t img_at, pt_at, ps_at, obs_at;  // the problem's place in the shared lists (images, points, point starts, sorted observations)
    int orig_at;   // its first caller-order observation
    char dup;      // one camera twice on a point (device-built block entries are then off)
    char k_over8;  // a point with more than eight free observations (work items of up to 128 points are then off)
};

// The camera lists and the point-major lists of one problem with PROBLEM-LOCAL offsets.  Written by build_problem_lists on the host
// threads; merge_decide reads the sizes and flags, merge_copy appends the lists to the shared ones and relocates the offsets (positions in
// setpts / setpairs / cblkitems / ccitems, partial-sum, camera-partial and record indices) by the running totals.
struct Built
{
    std::vector<int> camstart, camitems;
    int be_nch          = 0;
    long long ent_bound = 0;
    bool ok = false, cam_sums_bad = false;
    std::vector<SetItem> items;
    std::vector<int2> ipts;
    std::vector<int> ipairs;
    int parts = 0, cparts = 0;
    long long recs = 0;
    int max_pairs = 0, max_run = 0, max_k = 0;
    std::vector<int> cblkstart, cblkitems, ccstart, ccitems;
    std::vector<int> wv;  // point_wave work items (first point of each, then n_pt); empty: a point has more than 64 observations
    bool wv_ok = false;
};

// Where merge_decide puts a problem's lists in the shared ones: the serial loop only takes the decisions and does the arithmetic of
// the running totals; the element copies (with their relocations) run on the host threads afterwards in merge_copy (the loop's push_back
// relocations were ~6 of a 1024-window hand-over's 23 ms of list time).
struct MergeAt
{
    size_t wvpt, camstart, camitems, ccstart, ccitems, setitems, setpts, setpairs, cblkstart, cblkitems;
    int base_parts, base_cparts;
    long long base_rec;
    bool set;
};

// Running totals of the set: merge_decide adds every problem to them, the later stages size the device buffers and launches by them.
struct Totals
{
    int img_off = 0, pt_off = 0, obs_off = 0, cam_off = 0, orig_off = 0, vec_off = 0;
    long long s_off = 0;
    int max_np = 0, max_nfc = 0, max_n6 = 0, max_ni = 0;
    int n_partials = 0, max_set_items = 0, max_set_pairs = 0, max_set_run = 0, max_set_k = 0;
    int n_cparts = 0;          // per (work item, free camera) partial sums of the camera pass
    long long n_setrec = 0;    // static observation records of the work items
    bool cam_sums_ok = true;   // no constant point is seen by a free camera (its observations are in no work item with pairs)
    bool set_ok = true;        // every problem can run the point-major Schur pass
    int max_rpc = 0, max_wv = 0;
    bool wave_ok = true;
    size_t blkrpc_logical = 0;   // entries of blk_rpc up to the current problem (materialised only for problems with constraints)
    bool dev_entries_ok = true;  // every problem can have its block entries built on the device
    int blkstart_total = 0, max_citems = 0;
    size_t n_wvpt = 0, n_camstart = 0, n_camitems = 0, n_ccstart = 0, n_ccitems = 0, n_setitems = 0, n_setpts = 0, n_setpairs = 0, n_cblkstart = 0,
           n_cblkitems = 0;
    // plan_block_entries
    bool dev_entries = false;
    long long ent_total = 0, becnt_total = 0;
    int max_be_waves = 0;
};

// Every environment switch of the hand-over's own (SNK_BA_*; the solver's path switches are BaSwitches in dispatch.hpp, read by
// ba_switches() in ba.hip, and the hand-over takes what it needs of them from there).  All but the last are read once per process,
// at the first hand-over.
struct Switches
{
    bool alt_paths;     // BaSwitches::any_alt_path() or NO_BIG_ITEMS: work items stay at <= 64 points
    bool sets_forced;   // SCHUR_SET_MIN_ITEMS is set: the point-major lists are built whatever the size of the call (tests)
    bool profile;       // PROFILE_CREATE: host-side cost of a hand-over on stderr, in microseconds
    int host_threads;   // HOST_THREADS: threads of the threaded passes (0: by the host's size)
    bool no_pool;       // NO_HOST_POOL: threads created and joined per pass (A/B)
    int fill_chunks;    // FILL_CHUNKS: chunks of the fill pass of a batch (A/B; 0: BA_FILL_CHUNKS)
    bool host_entries;  // HOST_ENTRIES: block entries by the host builder (A/B and tests)
    long long becnt_budget;  // BECNT_BUDGET: bytes of device counters beyond which the host builder takes over (tests force the fallback)
    bool check_lists;   // CHECK_LISTS: tests / fuzzers: device-built lists against the host builder
    bool sets_in_env_now;  // SCHUR_SET_MIN_ITEMS again, read at EVERY call: reserve_lists sizes the point-major lists by it
    static Switches read()
    {
        static const Switches once = []
        {
            Switches s{};
            s.alt_paths    = ba_switches().any_alt_path() || getenv("SNK_BA_NO_BIG_ITEMS");
            s.sets_forced  = getenv("SNK_BA_SCHUR_SET_MIN_ITEMS") != nullptr;
            s.profile      = getenv("SNK_BA_PROFILE_CREATE") != nullptr;
            s.host_threads = getenv("SNK_BA_HOST_THREADS") ? atoi(getenv("SNK_BA_HOST_THREADS")) : 0;
            s.no_pool      = getenv("SNK_BA_NO_HOST_POOL") != nullptr;
            s.fill_chunks  = getenv("SNK_BA_FILL_CHUNKS") ? atoi(getenv("SNK_BA_FILL_CHUNKS")) : 0;
            s.host_entries = getenv("SNK_BA_HOST_ENTRIES") != nullptr;
            s.becnt_budget = getenv("SNK_BA_BECNT_BUDGET") ? atoll(getenv("SNK_BA_BECNT_BUDGET")) : (64ll << 20);
            s.check_lists  = getenv("SNK_BA_CHECK_LISTS") != nullptr;
            return s;
        }();
        Switches s        = once;
        s.sets_in_env_now = getenv("SNK_BA_SCHUR_SET_MIN_ITEMS") != nullptr;
        return s;
    }
};

// Host time of the list building by section (SNK_BA_PROFILE_CREATE=1).  A lap timer: lap(s) adds the time since the previous lap to
// section s -- "what just ran belongs to s" -- so the serial loop of merge_decide charges its parts to the sections of the lists they
// place.  The sections are the fields of the second [snk_ba_set_problems] line (report); SEC_GROUPING and SEC_WORK_ITEMS are fields of
// that line that nothing is charged to since the point sets are built inside the threaded pass (charged to SEC_CAMERA_LISTS as a whole).
enum Section { SEC_VALUES_SORT, SEC_OBS_ARRAYS, SEC_WAVE_ITEMS, SEC_CAMERA_LISTS, SEC_BLOCK_ENTRIES, SEC_BLOCK_LISTS, SEC_CONSTRAINTS, SEC_REST,
               SEC_GROUPING, SEC_WORK_ITEMS, SEC_COUNT };
struct SectionTimer
{
    bool on = false;
    long long ns[SEC_COUNT] = {};
    std::chrono::steady_clock::time_point last;
    void start(bool enabled) { on = enabled, last = std::chrono::steady_clock::now(); }
    void lap(Section s)
    {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        ns[s] += (long long)std::chrono::duration_cast<std::chrono::nanoseconds>(now - last).count();
        last = now;
    }
    long long us(Section s) const { return ns[s] / 1000; }
};

// the one early return of the stages: a failed step's error code ends the stage
#define SNK_TRY(expr)                      \
    do                                     \
    {                                      \
        const int rc_ = (expr);            \
        if (rc_ != SNK_OK) return rc_;     \
    } while (0)

// Scratch of build_point_sets for one problem: the points grouped by camera set, then the work items cut from the groups and the
// partial sums they contribute to every camera-pair block and every free camera.
struct PointSets
{
    // camera set -> group: a hash of the signature finds the candidate, the stored signature confirms it (a std::map keyed by
    // the vectors themselves was 60 ns per point, a third of a batch hand-over's list time)
    std::unordered_multimap<unsigned long long, int> gid;
    std::vector<std::vector<int>> gpts;  // per group: its points
    std::vector<std::vector<int>> gsig;  // per group: free-camera index (or -1) of every observation of one of its points
    bool ok = false;                     // the problem can run the point-major pass
    std::vector<std::vector<int>> contrib;   // per camera-pair block: its partial sums in s_part
    std::vector<std::vector<int>> ccontrib;  // per free camera: its partial sums in cam_part
    std::vector<SetItem> items;
    std::vector<int2> ipts;
    std::vector<int> ipairs;
    int parts = 0, cparts = 0;
    long long recs = 0;  // static observation records of the work items (gathered on the device: gather_set_records)
    int find_group(const std::vector<int>& key)
    {
        unsigned long long hsh = 1469598103934665603ull;
        for (int v : key) hsh = (hsh ^ (unsigned long long)(unsigned)v) * 1099511628211ull;
        auto range = gid.equal_range(hsh);
        for (auto it = range.first; it != range.second; ++it)
            if (gsig[(size_t)it->second] == key) return it->second;
        gid.emplace(hsh, (int)gpts.size());
        gpts.emplace_back();
        gsig.push_back(key);
        return (int)gpts.size() - 1;
    }
};

struct RowsOnHost;

struct HandOver  // one snk_ba_set_problems or snk_ba_set_problems_dev call
{
    snk_ba* const h;
    // the caller's problems; snk_ba_set_problems_dev: a host shadow of the device rows (sizes, K, bf; img_const, pt_const and rpc point
    // at pinned read-backs; the pose, point and observation pointers are NULL), or the downloaded rows under SNK_BA_CHECK_LISTS
    const snk_ba_problem* problems;
    const int count;
    const bool dev;  // snk_ba_set_problems_dev: the values and the sorted observation arrays are written on the device (dev_stage)
    const bool imp;  // implicit Schur form (snk_ba_set_explicit_schur): one scene; nothing sized (free cameras)^2 is built or allocated
    BaLists& L;      // the handle's pinned lists, capacity kept from the previous set
    const Switches sw;
    SectionTimer sec;
    std::vector<PreProb> pre;
    std::vector<Built> built;
    std::vector<MergeAt> at;
    std::vector<long long> ent_bound;  // per problem: room for its block entries when the device builds them
    Totals tot;
    int n_threads = 1;  // of the threaded passes
    std::atomic<bool> worker_failed{false};
    // work items of up to 128 points: see SET_CHUNK_BIG.  Needs the default point-major kernels (sw.alt_paths: the A/B switches that select
    // the others) and at most 8 free observations per point in EVERY problem (else the batch runs point_wave + schur_mfma<4>), which is
    // known only after a look at all of them: size_pass counts them on the host threads (as a serial loop over every observation of the
    // batch in front of everything else it was ~20 of a 1024-window hand-over's 53 ms of list time)
    const bool want_big_items;
    bool big_items = false;
    // batches: the observation arrays (0.65 of a batch's GB) go over the bus WHILE the lists are built: the fill pass runs in
    // chunks of problems, every chunk's ranges of the arrays are sent as soon as they are written (the upload of a 1024-window batch is
    // ~15 ms of PCIe time that used to start when the last list was done), and build_problem_lists and the merge build the rest meanwhile
    const bool early_upload;
    // batches: the second and third copies of the poses / points (the reset state, the trial points) are device-to-device copies behind
    // the upload instead of two more trips over the bus (100 MB of a 1024-window hand-over's 1.1 GB); a single window keeps the one launch
    const bool dup_on_device;
    CopyTab tab{}, tab2{};  // the upload (host -> device, zero fills) and the device-to-device copies behind it
    std::chrono::steady_clock::time_point t_begin, t_lists, t_up, t_rs;
    long long bytes_up = 0, bytes_down = 0;    // over the bus, host -> device and device -> host (SNK_BA_PROFILE_CREATE)
    long long dev_stage_us = 0, readback_us = 0;  // snk_ba_set_problems_dev: the two kernels (with their waits), the copies down
    bool dev_long_run = false;                  // dev_stage met a point with more than HO_MAX_RUN observations: the batch is staged

    // device rows: every count derives o_pt / o_cam / o_ptfree / cam_items on the device and copies device-to-device
    HandOver(snk_ba* handle, const snk_ba_problem* p, int n, bool from_device = false)
        : h(handle), problems(p), count(n), dev(from_device), imp(handle->explicit_schur == 0), L(handle->lists), sw(Switches::read()),
          want_big_items(n >= 256 && !sw.alt_paths), early_upload(n >= 16 || from_device), dup_on_device(n >= 16 || from_device)
    {
    }

    int check_arguments();
    int reserve_lists();
    void pick_threads();
    int dev_stage(const snk_scene_out& rows, snk_ba_problem* shadow);
    int dev_check(const snk_scene_out& rows, RowsOnHost& host_rows, const std::vector<snk_scene_result>& rec);
    int later_stages();
    int host_hand_over();
    int size_pass();
    int place_problems();
    void fill_problem(int b);
    int send_chunk(int b0, int b1);
    int fill_and_send();
    void build_camera_lists(int b);
    void build_wave_items(int b);
    void group_points(int b, PointSets& S);
    void cut_work_items(int b, PointSets& S);
    void build_block_lists(int b, PointSets& S);
    int build_problem_lists();
    int merge_constraints(int b);
    int merge_decide();
    int merge_copy();
    int publish_totals();
    void host_block_entries(int b, pvec<int>& bs_out, pvec<int4>& ent_out) const;
    int plan_block_entries();
    int dup(DevBuf& dst, const DevBuf& src, size_t bytes);
    int upload_rest();
    int reserve_work();
    int zero(DevBuf& b, size_t bytes);
    int zero_and_launch();
    void bind_arrays();
    int launch_device_lists();
    int check_lists();
    int report();

    // body(b) for the problems lo <= b < hi, in runs of eight on n_threads host threads (the caller is one of them)
    template <typename Body>
    int threaded(int lo, int hi, Body&& body)
    {
        if (n_threads <= 1)
        {
            for (int b = lo; b < hi; ++b) body(b);
            return SNK_OK;
        }
        std::atomic<int> next{lo};
        // an exception in a worker (the vectors it grows: std::bad_alloc) must not reach std::terminate: it is caught, the remaining
        // work is abandoned and the caller turns worker_failed into an error code after the pass
        const std::function<void()> work = [&]()
        {
            try
            {
                for (;;)
                {
                    const int b0 = next.fetch_add(8);
                    if (b0 >= hi || worker_failed.load(std::memory_order_relaxed)) return;
                    for (int b = b0; b < std::min(b0 + 8, hi); ++b) body(b);
                }
            }
            catch (...)
            {
                worker_failed.store(true);
            }
        };
        if (!sw.no_pool)
            h->pool.run(n_threads - 1, work);
        else
        {
            std::vector<std::thread> pool;
            try
            {
                for (int t = 1; t < n_threads; ++t) pool.emplace_back(work);
            }
            catch (...)
            {
                worker_failed.store(true);  // thread creation failed: the threads that exist finish, this thread does the rest
            }
            work();
            for (auto& t : pool) t.join();
        }
        if (worker_failed.load())
        {
            set_error("snk_ba_set_problems: a list-building thread failed (out of host memory?)");
            return SNK_ERR_HIP;
        }
        return SNK_OK;
    }
};

// every refusal of an argument, in the order a caller met them before: the call as a whole, then problem by problem
int HandOver::check_arguments()
{
    SNK_REQUIRE(count >= 1 && count <= 65535 && problems != nullptr, "count must be 1..65535");
    SNK_REQUIRE(!imp || count == 1, "the implicit Schur form takes one problem (snk_ba_set_explicit_schur)");
    for (int b = 0; b < count; ++b)  // the packed observation records hold the image index in 15 bits (SetObs)
        SNK_REQUIRE(problems[b].n_img <= SET_MAX_IMG, "a problem has more than 32767 images");
    for (int b = 0; b < count; ++b)
    {
        const snk_ba_problem& P = problems[b];
        SNK_REQUIRE(P.n_img >= 0 && P.n_pt >= 0 && P.n_obs >= 0, "negative problem size");
        SNK_REQUIRE(P.n_img == 0 || (P.pose && P.img_const), "NULL pose arrays");
        SNK_REQUIRE(P.n_pt == 0 || (P.pt && P.pt_const), "NULL point arrays");
        SNK_REQUIRE(P.n_obs == 0 || (P.obs_img && P.obs_pt && P.obs_uv && P.obs_depth && P.obs_weight), "NULL observation arrays");
        SNK_REQUIRE(P.n_rpc >= 0 && (P.n_rpc == 0 || P.rpc != nullptr), "bad relative pose constraints");
    }
    return SNK_OK;
}

// capacity of the pinned lists (writes L; reads only the caller's sizes)
int HandOver::reserve_lists()
{
    t_begin = std::chrono::steady_clock::now();
    L.clear();
    L.probs.resize((size_t)count);
    // the big lists are sized by the totals of the call: growing a pinned vector re-pins and copies it every time it doubles
    size_t t_img = 0, t_pt = 0, t_obs = 0;
    for (int b = 0; b < count; ++b)
    {
        t_img += (size_t)std::max(problems[b].n_img, 0);
        t_pt += (size_t)std::max(problems[b].n_pt, 0);
        t_obs += (size_t)std::max(problems[b].n_obs, 0);
    }
    L.ptc.reserve(t_pt), L.camidx.reserve(t_img), L.ptstart.reserve(t_pt + (size_t)count), L.ocam.reserve(t_obs), L.camitems.reserve(t_obs);
    if (!dev)  // (device rows: the values and the other observation arrays never exist on the host)
    {
        L.pose.reserve(7 * t_img), L.pt.reserve(3 * t_pt);
        L.ouv2.reserve(2 * t_obs), L.odepth.reserve(t_obs), L.oweight.reserve(t_obs), L.optfree.reserve(t_obs), L.oimg.reserve(t_obs);
        L.oorig.reserve(t_obs), L.optidx.reserve(t_obs);
    }
    // ... and so are the lists of the point-major pass when they will be built (batches, big scenes): on a 300-keyframe
    // scene the doubling of setobs / cblkstart / cblkitems through fresh pinned allocations was 17 of the 26 ms of a
    // first hand-over (the same scene again on the handle, capacities kept: 8 ms)
    size_t t_blk = 0;
    bool sets_likely = count >= 8 || sw.sets_in_env_now;
    for (int b = 0; b < count; ++b)
    {
        size_t nfc = 0;
        if (problems[b].img_const)
            for (int i = 0; i < problems[b].n_img; ++i) nfc += problems[b].img_const[i] ? 0 : 1;
        t_blk += nfc * nfc + 1;
        sets_likely |= problems[b].n_pt >= 8000;
    }
    if (!imp) L.cblkstart.reserve(t_blk);
    if (sets_likely && !imp) L.setpts.reserve(t_pt), L.cblkitems.reserve(2 * t_obs), L.ccitems.reserve(t_obs);
    h->orig_off.assign((size_t)count, 0);
    h->orig_n.assign((size_t)count, 0);
    ent_bound.assign((size_t)count, 0);
    pre.resize((size_t)count), built.resize((size_t)count), at.resize((size_t)count);
    sec.start(sw.profile);
    return SNK_OK;
}

// ---- sizing pass + fill pass over the problems, on several host threads for batches ----
// The values, the free-camera indices, the counting sort by point and the eight sorted observation arrays of a problem depend on nothing
// but that problem, and they were half of a batch hand-over's list time on ONE core (1024 windows: 117 of 227 ms).  Pass 1 counts
// (valid observations, free cameras) per problem, a prefix sum gives every problem its place in the shared lists, pass 2 writes the
// places directly -- disjoint ranges, no locks.  The later stages only READ these lists.  Same contents as the serial
// builder : SNK_BA_CHECK_LISTS and the bit-identity tests of the variants suite cover it.
// size_pass writes PreProb::nfc / no / k_over8 and big_items.
void HandOver::pick_threads()
{
    if (count >= 16)
    {
        // up to 32 threads (round 6; 16 before): on the 256-thread hosts of the MI355X boxes a 1024-window hand-over builds its lists in 35
        // instead of 53 ms with 32, no faster with 64 (profiles/r06/r06i_ba_handover_threads_before.txt)
        n_threads = sw.host_threads > 0 ? sw.host_threads : (int)std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 32u);
        n_threads = std::min(n_threads, count / 8);
    }
    else if (sw.host_threads > 0 && count >= 2)
        n_threads = std::min(sw.host_threads, count);  // tests force the threaded form on small batches
}

int HandOver::size_pass()
{
    pick_threads();
    SNK_TRY(threaded(0, count, [&](int b)
    {
        const snk_ba_problem& P = problems[b];
        PreProb& q = pre[(size_t)b];
        q.nfc = 0;
        for (int i = 0; i < P.n_img; ++i) q.nfc += P.img_const[i] ? 0 : 1;
        int no = 0;
        for (int o = 0; o < P.n_obs; ++o)
            if (ho_obs_valid(P.obs_img[o], P.obs_pt[o], P.n_img, P.n_pt, P.img_const, P.pt_const)) ++no;  // handover_core.hpp
        q.no  = no;
        q.dup = 0;
        q.k_over8 = 0;
        if (want_big_items && P.n_pt > 0 && P.n_obs > 0)
        {
            // work items of up to 128 points need at most 8 free observations per point in EVERY problem
            std::vector<unsigned char> kfree((size_t)P.n_pt, 0);
            for (int o = 0; o < P.n_obs; ++o)
            {
                const int p = P.obs_pt[o];
                if (!ho_obs_by_free_camera(P.obs_img[o], p, P.n_img, P.n_pt, P.img_const)) continue;
                if (ho_k_over8(++kfree[(size_t)p])) q.k_over8 = 1;
            }
        }
    }));
    if (want_big_items)
    {
        big_items = true;
        for (int b = 0; b < count; ++b) big_items = big_items && !pre[(size_t)b].k_over8;
    }
    return SNK_OK;
}

// ---- snk_ba_set_problems_dev: size_pass, place_problems and fill_and_send on the device ----
// Reads the sizes of the shadow problems; writes d_pose .. d_oorig and d_ocam in full, PreProb, and what the later host stages read of L
// (camidx, ptc, ptstart, ocam); completes the shadow (img_const, pt_const, rpc).  Two launches, two waits: the problems' places in the
// observation arrays depend on the valid counts (obs_off advances by them in merge_decide), which the first kernel reports.
int HandOver::dev_stage(const snk_scene_out& rows, snk_ba_problem* shadow)
{
    using clk = std::chrono::steady_clock;
    auto us_since = [](clk::time_point a) { return (long long)std::chrono::duration_cast<std::chrono::microseconds>(clk::now() - a).count(); };
    hipStream_t st = h->stream;
    pick_threads();
    size_t a_img = 0, a_pt = 0, a_ps = 0;
    long long a_orig = 0;
    int max_np = 0, max_rpc = 0;
    L.hoplace.resize((size_t)count), L.hoout.resize((size_t)count);
    for (int b = 0; b < count; ++b)
    {
        const snk_ba_problem& P = problems[b];
        PreProb& q = pre[(size_t)b];
        q.img_at = a_img, q.pt_at = a_pt, q.ps_at = a_ps, q.obs_at = 0, q.orig_at = (int)a_orig;
        HoPlace& pl = L.hoplace[(size_t)b];
        pl.n_img = P.n_img, pl.n_pt = P.n_pt, pl.n_obs = P.n_obs;
        pl.img_at = (int)a_img, pl.pt_at = (int)a_pt, pl.ps_at = (int)a_ps, pl.orig_at = (int)a_orig, pl.obs_at = 0;
        a_img += (size_t)P.n_img, a_pt += (size_t)P.n_pt, a_ps += (size_t)P.n_pt + 1, a_orig += P.n_obs;
        SNK_REQUIRE(a_orig < (1ll << 31) && a_ps < ((size_t)1 << 31) && a_img * 7 < ((size_t)1 << 31), "scene list too large (observations)");
        max_np = std::max(max_np, P.n_pt), max_rpc = std::max(max_rpc, P.n_rpc);
    }
    HoRows R;
    R.img_cap = rows.img_cap, R.pt_cap = rows.pt_cap, R.obs_cap = rows.obs_cap;
    R.pose = rows.pose, R.img_const = rows.img_const, R.pt = rows.pt, R.pt_const = rows.pt_const;
    R.obs_img = rows.obs_img, R.obs_pt = rows.obs_pt, R.obs_uv = rows.obs_uv, R.obs_depth = rows.obs_depth, R.obs_weight = rows.obs_weight;
    SNK_TRY(h->d_pose.reserve(std::max<size_t>(a_img, 1) * 7 * sizeof(double)));
    SNK_TRY(h->d_pt.reserve(std::max<size_t>(a_pt, 1) * 3 * sizeof(double)));
    SNK_TRY(h->d_ptc.reserve(std::max<size_t>(a_pt, 1)));
    SNK_TRY(h->d_camidx.reserve(std::max<size_t>(a_img, 1) * sizeof(int)));
    SNK_TRY(h->d_ptstart.reserve(a_ps * sizeof(int)));
    SNK_TRY(h->d_hoplace.reserve((size_t)count * sizeof(HoPlace)));
    SNK_TRY(h->d_hoout.reserve((size_t)count * sizeof(HoOut)));
    SNK_TRY(set_max_lds_once(reinterpret_cast<const void*>(ho_count_kernel), (int)ho_count_carve(HO_MAX_PTS)));
    SNK_TRY(set_max_lds_once(reinterpret_cast<const void*>(ho_fill_kernel), (int)ho_fill_carve(HO_MAX_PTS)));
    auto t0 = clk::now();
    SNK_HIP_CHECK(hipMemcpyAsync(h->d_hoplace.p, L.hoplace.data(), (size_t)count * sizeof(HoPlace), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(ho_count_kernel, dim3(count), dim3(HO_THREADS), ho_count_carve(max_np), st, R, h->d_hoplace.as<const HoPlace>(), h->d_hoout.as<HoOut>(),
                       h->d_pose.as<double>(), h->d_pt.as<double>(), h->d_ptc.as<unsigned char>(), h->d_camidx.as<int>(), h->d_ptstart.as<int>());
    SNK_LAUNCH_CHECK();
    SNK_HIP_CHECK(hipStreamSynchronize(st));
    dev_stage_us += us_since(t0);
    // first readback: the counts, and the structure that depends on no placement
    t0 = clk::now();
    L.camidx.resize(a_img), L.ptc.resize(a_pt), L.ptstart.resize(a_ps), L.imgc.resize(std::max<size_t>(a_img, 1));
    SNK_HIP_CHECK(hipMemcpyAsync(L.hoout.data(), h->d_hoout.p, (size_t)count * sizeof(HoOut), hipMemcpyDeviceToHost, st));
    if (a_img) SNK_HIP_CHECK(hipMemcpyAsync(L.camidx.data(), h->d_camidx.p, a_img * sizeof(int), hipMemcpyDeviceToHost, st));
    if (a_pt) SNK_HIP_CHECK(hipMemcpyAsync(L.ptc.data(), h->d_ptc.p, a_pt, hipMemcpyDeviceToHost, st));
    SNK_HIP_CHECK(hipMemcpyAsync(L.ptstart.data(), h->d_ptstart.p, a_ps * sizeof(int), hipMemcpyDeviceToHost, st));
    L.rpcrows.resize((size_t)count * (size_t)std::max(max_rpc, 1));
    if (max_rpc > 0)  // the first n_rpc records of every row (the rows are win_cap apart)
        SNK_HIP_CHECK(hipMemcpy2DAsync(L.rpcrows.data(), (size_t)max_rpc * sizeof(snk_ba_rpc), rows.rpc, (size_t)rows.win_cap * sizeof(snk_ba_rpc),
                                       (size_t)max_rpc * sizeof(snk_ba_rpc), (size_t)count, hipMemcpyDeviceToHost, st));
    SNK_HIP_CHECK(hipStreamSynchronize(st));
    bytes_up += (long long)count * (long long)sizeof(HoPlace);
    bytes_down += (long long)count * (long long)sizeof(HoOut) + (long long)(a_img * 4 + a_pt + a_ps * 4) +
                  (long long)count * max_rpc * (long long)sizeof(snk_ba_rpc);
    readback_us += us_since(t0);
    size_t a_obs = 0;
    for (int b = 0; b < count; ++b)
    {
        const HoOut& r = L.hoout[(size_t)b];
        PreProb& q     = pre[(size_t)b];
        SNK_REQUIRE(r.nfc >= 0 && r.nfc <= problems[b].n_img && r.no >= 0 && r.no <= problems[b].n_obs, "the device stage of the hand-over answered a count out of range");
        if (r.long_run) dev_long_run = true;
        q.nfc = r.nfc, q.no = r.no, q.dup = 0;
        q.k_over8 = want_big_items && r.k_over8 ? 1 : 0;  // (size_pass looks only then)
        q.obs_at = a_obs;
        L.hoplace[(size_t)b].obs_at = (int)a_obs;
        a_obs += (size_t)r.no;
        SNK_REQUIRE(a_obs < ((size_t)1 << 31), "scene list too large (observations)");
    }
    if (dev_long_run) return SNK_OK;  // the caller stages the batch
    if (want_big_items)
    {
        big_items = true;
        for (int b = 0; b < count; ++b) big_items = big_items && !pre[(size_t)b].k_over8;
    }
    const size_t n_o = std::max<size_t>(a_obs, 1);
    SNK_TRY(h->d_oimg.reserve(n_o * sizeof(int)));
    SNK_TRY(h->d_ouv.reserve(n_o * 2 * sizeof(double)));
    SNK_TRY(h->d_odepth.reserve(n_o * sizeof(double)));
    SNK_TRY(h->d_oweight.reserve(n_o * sizeof(double)));
    SNK_TRY(h->d_oorig.reserve(n_o * sizeof(int)));
    SNK_TRY(h->d_ocam.reserve(n_o * sizeof(int)));
    SNK_TRY(h->d_optfree.reserve(n_o));
    SNK_TRY(h->d_optidx.reserve(n_o * sizeof(int)));
    t0 = clk::now();
    SNK_HIP_CHECK(hipMemcpyAsync(h->d_hoplace.p, L.hoplace.data(), (size_t)count * sizeof(HoPlace), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(ho_fill_kernel, dim3(count), dim3(HO_THREADS), ho_fill_carve(max_np), st, R, h->d_hoplace.as<const HoPlace>(), h->d_hoout.as<HoOut>(),
                       (const int*)h->d_camidx.as<int>(), (const int*)h->d_ptstart.as<int>(), h->d_oimg.as<int>(), h->d_ocam.as<int>(), h->d_ouv.as<double2>(),
                       h->d_odepth.as<double>(), h->d_oweight.as<double>(), h->d_oorig.as<int>());
    SNK_LAUNCH_CHECK();
    SNK_HIP_CHECK(hipStreamSynchronize(st));
    dev_stage_us += us_since(t0);
    // second readback: the sorted free-camera indices, dup
    t0 = clk::now();
    L.ocam.resize(a_obs);
    if (a_obs) SNK_HIP_CHECK(hipMemcpyAsync(L.ocam.data(), h->d_ocam.p, a_obs * sizeof(int), hipMemcpyDeviceToHost, st));
    SNK_HIP_CHECK(hipMemcpyAsync(L.hoout.data(), h->d_hoout.p, (size_t)count * sizeof(HoOut), hipMemcpyDeviceToHost, st));
    SNK_HIP_CHECK(hipStreamSynchronize(st));
    bytes_up += (long long)count * (long long)sizeof(HoPlace);
    bytes_down += (long long)count * (long long)sizeof(HoOut) + (long long)a_obs * 4;
    readback_us += us_since(t0);
    for (int b = 0; b < count; ++b)
    {
        PreProb& q = pre[(size_t)b];
        q.dup      = L.hoout[(size_t)b].dup ? 1 : 0;
        unsigned char* ic = L.imgc.data() + q.img_at;
        const int* cidx   = L.camidx.data() + q.img_at;
        for (int i = 0; i < problems[b].n_img; ++i) ic[i] = cidx[i] < 0 ? 1 : 0;
        shadow[b].img_const = ic;
        shadow[b].pt_const  = L.ptc.data() + q.pt_at;
        shadow[b].rpc       = problems[b].n_rpc > 0 ? L.rpcrows.data() + (size_t)b * (size_t)max_rpc : nullptr;
    }
    sec.lap(SEC_VALUES_SORT);
    return SNK_OK;
}

// The caller's rows [n_q][cap] copied down as tight rows of the largest count each: the staged hand-over of batches the kernels do not
// take, and SNK_BA_CHECK_LISTS.  Pinned, released with the object.
struct RowsOnHost
{
    HostBuf pose, imgc, pt, ptc, oimg, opt, ouv, odepth, oweight, rpc;
    std::vector<snk_ba_problem> problems;
    long long bytes = 0;
    ~RowsOnHost()
    {
        for (HostBuf* b : {&pose, &imgc, &pt, &ptc, &oimg, &opt, &ouv, &odepth, &oweight, &rpc}) b->release();
    }
    int fetch(const snk_scene_out& rows, const std::vector<snk_scene_result>& rec, const double K[4], double bf, hipStream_t st)
    {
        const size_t n = rec.size();
        int m_img = 0, m_pt = 0, m_obs = 0, m_rpc = 0;
        for (const snk_scene_result& r : rec)
            m_img = std::max(m_img, r.n_img), m_pt = std::max(m_pt, r.n_pt), m_obs = std::max(m_obs, r.n_obs), m_rpc = std::max(m_rpc, r.n_rpc);
        auto get = [&](HostBuf& dst, const void* src, size_t elem, int most, int cap) -> int
        {
            if (most == 0) return SNK_OK;
            int rc = dst.reserve(n * (size_t)most * elem);
            if (rc != SNK_OK) return rc;
            SNK_HIP_CHECK(hipMemcpy2DAsync(dst.p, (size_t)most * elem, src, (size_t)cap * elem, (size_t)most * elem, n, hipMemcpyDeviceToHost, st));
            bytes += (long long)(n * (size_t)most * elem);
            return SNK_OK;
        };
        int rc;
        if ((rc = get(pose, rows.pose, 56, m_img, rows.img_cap)) != SNK_OK) return rc;
        if ((rc = get(imgc, rows.img_const, 1, m_img, rows.img_cap)) != SNK_OK) return rc;
        if ((rc = get(pt, rows.pt, 24, m_pt, rows.pt_cap)) != SNK_OK) return rc;
        if ((rc = get(ptc, rows.pt_const, 1, m_pt, rows.pt_cap)) != SNK_OK) return rc;
        if ((rc = get(oimg, rows.obs_img, 4, m_obs, rows.obs_cap)) != SNK_OK) return rc;
        if ((rc = get(opt, rows.obs_pt, 4, m_obs, rows.obs_cap)) != SNK_OK) return rc;
        if ((rc = get(ouv, rows.obs_uv, 16, m_obs, rows.obs_cap)) != SNK_OK) return rc;
        if ((rc = get(odepth, rows.obs_depth, 8, m_obs, rows.obs_cap)) != SNK_OK) return rc;
        if ((rc = get(oweight, rows.obs_weight, 8, m_obs, rows.obs_cap)) != SNK_OK) return rc;
        if ((rc = get(rpc, rows.rpc, sizeof(snk_ba_rpc), m_rpc, rows.win_cap)) != SNK_OK) return rc;
        SNK_HIP_CHECK(hipStreamSynchronize(st));
        problems.assign(n, snk_ba_problem{});
        for (size_t b = 0; b < n; ++b)
        {
            snk_ba_problem& P = problems[b];
            P.n_img = rec[b].n_img, P.n_pt = rec[b].n_pt, P.n_obs = rec[b].n_obs, P.n_rpc = rec[b].n_rpc;
            // (a row without entries keeps a valid pointer where the batch has any: only its first `count` entries are ever read)
            P.pose       = reinterpret_cast<double(*)[7]>(pose.as<char>() + b * (size_t)m_img * 56);
            P.img_const  = imgc.as<uint8_t>() + b * (size_t)m_img;
            P.pt         = reinterpret_cast<double(*)[3]>(pt.as<char>() + b * (size_t)m_pt * 24);
            P.pt_const   = ptc.as<uint8_t>() + b * (size_t)m_pt;
            P.obs_img    = oimg.as<int32_t>() + b * (size_t)m_obs;
            P.obs_pt     = opt.as<int32_t>() + b * (size_t)m_obs;
            P.obs_uv     = reinterpret_cast<const double(*)[2]>(ouv.as<char>() + b * (size_t)m_obs * 16);
            P.obs_depth  = odepth.as<double>() + b * (size_t)m_obs;
            P.obs_weight = oweight.as<double>() + b * (size_t)m_obs;
            P.rpc        = P.n_rpc > 0 ? rpc.as<snk_ba_rpc>() + b * (size_t)m_rpc : nullptr;
            for (int k = 0; k < 4; ++k) P.K[k] = K[k];
            P.bf = bf;
        }
        return SNK_OK;
    }
};

// SNK_BA_CHECK_LISTS=1 on device rows: the rows come down, the host builder fills L from them, and every array the device stage wrote
// must equal the host's element for element.  L then holds what a host hand-over would, and `problems` the downloaded rows: the later
// stages and check_lists run as they do there.
int HandOver::dev_check(const snk_scene_out& rows, RowsOnHost& host_rows, const std::vector<snk_scene_result>& rec)
{
    hipStream_t st = h->stream;
    const std::vector<PreProb> dev_pre = pre;
    const bool dev_big = big_items;
    auto down = [&](auto& v, const DevBuf& src, size_t n) -> int
    {
        v.resize(n);
        if (n) SNK_HIP_CHECK(hipMemcpyAsync(v.data(), src.p, n * sizeof(v[0]), hipMemcpyDeviceToHost, st));
        return SNK_OK;
    };
    size_t a_img = L.camidx.size(), a_pt = L.ptc.size(), a_ps = L.ptstart.size(), a_obs = L.ocam.size();
    std::vector<double> g_pose, g_pt, g_uv, g_depth, g_weight;
    std::vector<unsigned char> g_ptc;
    std::vector<int> g_camidx, g_ptstart, g_oimg, g_ocam, g_oorig;
    SNK_TRY(down(g_pose, h->d_pose, 7 * a_img));
    SNK_TRY(down(g_pt, h->d_pt, 3 * a_pt));
    SNK_TRY(down(g_ptc, h->d_ptc, a_pt));
    SNK_TRY(down(g_camidx, h->d_camidx, a_img));
    SNK_TRY(down(g_ptstart, h->d_ptstart, a_ps));
    SNK_TRY(down(g_oimg, h->d_oimg, a_obs));
    SNK_TRY(down(g_ocam, h->d_ocam, a_obs));
    SNK_TRY(down(g_oorig, h->d_oorig, a_obs));
    SNK_TRY(down(g_uv, h->d_ouv, 2 * a_obs));
    SNK_TRY(down(g_depth, h->d_odepth, a_obs));
    SNK_TRY(down(g_weight, h->d_oweight, a_obs));
    SNK_TRY(host_rows.fetch(rows, rec, problems[0].K, problems[0].bf, st));  // (synchronises)
    problems = host_rows.problems.data();
    SNK_TRY(size_pass());
    SNK_TRY(place_problems());
    SNK_TRY(threaded(0, count, [&](int b) { fill_problem(b); }));
    SNK_REQUIRE(big_items == dev_big, "SNK_BA_CHECK_LISTS: the device stage's big-items decision differs from the host builder's");
    for (int b = 0; b < count; ++b)
    {
        const PreProb &d = dev_pre[(size_t)b], &w = pre[(size_t)b];
        SNK_REQUIRE(d.nfc == w.nfc && d.no == w.no && d.k_over8 == w.k_over8 && d.dup == w.dup,
                    "SNK_BA_CHECK_LISTS: the device stage's nfc / no / k_over8 / dup differ from the host builder's");
        SNK_REQUIRE(d.img_at == w.img_at && d.pt_at == w.pt_at && d.ps_at == w.ps_at && d.obs_at == w.obs_at && d.orig_at == w.orig_at,
                    "SNK_BA_CHECK_LISTS: the device stage's places differ from the host builder's");
    }
    auto same = [](const auto& g, const auto& l) { return g.size() == l.size() && (g.empty() || memcmp(g.data(), l.data(), g.size() * sizeof(g[0])) == 0); };
    SNK_REQUIRE(same(g_pose, L.pose), "SNK_BA_CHECK_LISTS: device-written pose differs from the host builder's");
    SNK_REQUIRE(same(g_pt, L.pt), "SNK_BA_CHECK_LISTS: device-written pt differs from the host builder's");
    SNK_REQUIRE(same(g_ptc, L.ptc), "SNK_BA_CHECK_LISTS: device-written pt_const differs from the host builder's");
    SNK_REQUIRE(same(g_camidx, L.camidx), "SNK_BA_CHECK_LISTS: device-written cam_idx differs from the host builder's");
    SNK_REQUIRE(same(g_ptstart, L.ptstart), "SNK_BA_CHECK_LISTS: device-written pt_start differs from the host builder's");
    SNK_REQUIRE(same(g_oimg, L.oimg), "SNK_BA_CHECK_LISTS: device-written o_img differs from the host builder's");
    SNK_REQUIRE(same(g_ocam, L.ocam), "SNK_BA_CHECK_LISTS: device-written o_cam differs from the host builder's");
    SNK_REQUIRE(same(g_oorig, L.oorig), "SNK_BA_CHECK_LISTS: device-written o_orig differs from the host builder's");
    SNK_REQUIRE(same(g_uv, L.ouv2), "SNK_BA_CHECK_LISTS: device-written o_uv differs from the host builder's");
    SNK_REQUIRE(same(g_depth, L.odepth), "SNK_BA_CHECK_LISTS: device-written o_depth differs from the host builder's");
    SNK_REQUIRE(same(g_weight, L.oweight), "SNK_BA_CHECK_LISTS: device-written o_weight differs from the host builder's");
    return SNK_OK;
}

// prefix sums over PreProb::no and the caller's sizes -> PreProb::*_at; the value and observation lists of L get their sizes
int HandOver::place_problems()
{
    size_t a_img = 0, a_pt = 0, a_ps = 0, a_obs = 0;
    long long a_orig = 0;
    for (int b = 0; b < count; ++b)
    {
        PreProb& q = pre[(size_t)b];
        q.img_at = a_img, q.pt_at = a_pt, q.ps_at = a_ps, q.obs_at = a_obs, q.orig_at = (int)a_orig;
        a_img += (size_t)problems[b].n_img, a_pt += (size_t)problems[b].n_pt, a_ps += (size_t)problems[b].n_pt + 1, a_obs += (size_t)q.no;
        a_orig += problems[b].n_obs;
        SNK_REQUIRE(a_orig < (1ll << 31) && a_obs < ((size_t)1 << 31), "scene list too large (observations)");
    }
    L.pose.resize(7 * a_img), L.pt.resize(3 * a_pt), L.ptc.resize(a_pt), L.camidx.resize(a_img), L.ptstart.resize(a_ps);
    L.oimg.resize(a_obs), L.ocam.resize(a_obs), L.optfree.resize(a_obs), L.ouv2.resize(2 * a_obs), L.odepth.resize(a_obs), L.oweight.resize(a_obs);
    L.oorig.resize(a_obs), L.optidx.resize(a_obs);
    return SNK_OK;
}

// One problem of the fill pass: reads PreProb::*_at, writes the problem's ranges of L.pose .. L.optidx in place and PreProb::dup
void HandOver::fill_problem(int b)
{
    const snk_ba_problem& P = problems[b];
    PreProb& q = pre[(size_t)b];
    // values
    if (P.n_img) memcpy(L.pose.data() + 7 * q.img_at, &P.pose[0][0], (size_t)P.n_img * 7 * sizeof(double));
    if (P.n_pt) memcpy(L.pt.data() + 3 * q.pt_at, &P.pt[0][0], (size_t)P.n_pt * 3 * sizeof(double));
    for (int p = 0; p < P.n_pt; ++p) L.ptc[q.pt_at + (size_t)p] = P.pt_const[p] ? 1 : 0;
    // free cameras
    int* cidx = L.camidx.data() + q.img_at;
    int nfc   = 0;
    for (int i = 0; i < P.n_img; ++i)
    {
        cidx[i] = ho_cam_index(P.img_const[i] != 0, nfc);
        nfc += P.img_const[i] ? 0 : 1;
    }
    // valid observations, counting sort by point (stable: caller order inside a point)
    int* pstart = L.ptstart.data() + q.ps_at;
    for (int p = 0; p <= P.n_pt; ++p) pstart[p] = 0;
    std::vector<char> valid((size_t)P.n_obs, 0);
    for (int o = 0; o < P.n_obs; ++o)
    {
        const int p = P.obs_pt[o];
        if (!ho_obs_valid(P.obs_img[o], p, P.n_img, P.n_pt, P.img_const, P.pt_const)) continue;
        valid[(size_t)o] = 1;
        pstart[p + 1]++;
    }
    for (int p = 0; p < P.n_pt; ++p) pstart[p + 1] += pstart[p];
    // the sorted observation arrays, written in ONE pass over the caller's order: position = next free slot of the point
    const size_t obs_at = q.obs_at;
    int* q_img = L.oimg.data() + obs_at, *q_cam = L.ocam.data() + obs_at, *q_orig = L.oorig.data() + obs_at, *q_pt = L.optidx.data() + obs_at;
    unsigned char* q_free = L.optfree.data() + obs_at;
    double *q_uv = L.ouv2.data() + 2 * obs_at, *q_d = L.odepth.data() + obs_at, *q_w = L.oweight.data() + obs_at;
    // free cameras seen so far per point (device-built block entries: no camera twice on a point)
    const int seen_words = ho_dup_words(nfc);
    std::vector<unsigned long long> seen((size_t)P.n_pt * (size_t)seen_words, 0ull);
    std::vector<int> fill(pstart, pstart + P.n_pt);
    for (int o = 0; o < P.n_obs; ++o)
    {
        if (!valid[(size_t)o]) continue;
        const int i = P.obs_img[o], p = P.obs_pt[o];
        const int sl = fill[(size_t)p]++;
        const int c  = cidx[i];
        if (c >= 0 && seen_words)
        {
            const unsigned long long bit = 1ull << (c & 63);
            unsigned long long& word     = seen[(size_t)p * (size_t)seen_words + (size_t)(c >> 6)];
            if (word & bit) q.dup = 1;
            word |= bit;
        }
        q_img[sl]  = i;
        q_cam[sl]  = c;
        q_free[sl] = P.pt_const[p] ? 0 : 1;
        q_uv[2 * sl]     = P.obs_uv[o][0];
        q_uv[2 * sl + 1] = P.obs_uv[o][1];
        q_d[sl]    = P.obs_depth[o];
        q_w[sl]    = P.obs_weight[o];
        q_orig[sl] = q.orig_at + o;
        q_pt[sl]   = p;
    }
}

// Sends the ranges of the arrays that the problems b0 <= b < b1 filled.  Range ends are rounded outwards to 16 bytes (the copy kernel
// moves 16-byte words): the few bytes of a neighbouring chunk that go along are either final already or sent again, later on the same
// stream, by their own chunk
int HandOver::send_chunk(int b0, int b1)
{
    CopyTab tabE;
    tabE.n = 0;
    auto part = [&](DevBuf& buf, const void* host, size_t elem, size_t e0, size_t e1, size_t total)
    {
        const size_t x0 = (e0 * elem) & ~(size_t)15, x1 = e1 >= total ? total * elem : std::min(total * elem, (e1 * elem + 15) & ~(size_t)15);
        if (x1 <= x0 || tabE.n >= COPY_TAB_MAX) return;
        tabE.src[tabE.n]   = static_cast<const char*>(host) + x0;
        tabE.dst[tabE.n]   = static_cast<char*>(buf.p) + x0;
        tabE.bytes[tabE.n] = (unsigned)(x1 - x0);
        ++tabE.n;
    };
    const size_t i0 = pre[(size_t)b0].img_at, p0 = pre[(size_t)b0].pt_at, s0 = pre[(size_t)b0].ps_at, o0 = pre[(size_t)b0].obs_at;
    const bool last = b1 >= count;
    const size_t i1 = last ? L.camidx.size() : pre[(size_t)b1].img_at, p1 = last ? L.ptc.size() : pre[(size_t)b1].pt_at,
                 s1 = last ? L.ptstart.size() : pre[(size_t)b1].ps_at, o1 = last ? L.oimg.size() : pre[(size_t)b1].obs_at;
    SNK_REQUIRE((o1 - o0 + 1) * 16 < (1ull << 32) && (p1 - p0 + 1) * 24 < (1ull << 32) && (i1 - i0 + 1) * 56 < (1ull << 32),
                "scene list too large for the upload table");
    part(h->d_pose, L.pose.data(), 56, i0, i1, L.camidx.size());
    part(h->d_camidx, L.camidx.data(), 4, i0, i1, L.camidx.size());
    part(h->d_pt, L.pt.data(), 24, p0, p1, L.ptc.size());
    part(h->d_ptc, L.ptc.data(), 1, p0, p1, L.ptc.size());
    part(h->d_ptstart, L.ptstart.data(), 4, s0, s1, L.ptstart.size());
    part(h->d_oimg, L.oimg.data(), 4, o0, o1, L.oimg.size());
    part(h->d_ouv, L.ouv2.data(), 16, o0, o1, L.oimg.size());
    part(h->d_odepth, L.odepth.data(), 8, o0, o1, L.oimg.size());
    part(h->d_oweight, L.oweight.data(), 8, o0, o1, L.oimg.size());
    part(h->d_oorig, L.oorig.data(), 4, o0, o1, L.oimg.size());
    if (tabE.n > 0)
    {
        unsigned big = 0;
        for (int e = 0; e < tabE.n; ++e) big = std::max(big, tabE.bytes[e]);
        for (int e = 0; e < tabE.n; ++e) bytes_up += tabE.bytes[e];
        const int gxe = (int)std::min(256u, std::max(16u, big >> 16));
        hipLaunchKernelGGL(copy_table_kernel, dim3(gxe, tabE.n), dim3(256), 0, h->stream, tabE);
        SNK_LAUNCH_CHECK();
    }
    return SNK_OK;
}

// The fill pass in chunks, each sent as soon as it is written (batches).  Everything sent here is final: the fill pass writes it in
// place and nothing later touches it.  o_cam, o_ptfree, o_pt and cam_items are derived on the device (derive_obs_fields,
// derive_cam_items): reserved, not sent.
int HandOver::fill_and_send()
{
    const int n_chunks = early_upload && count >= 64 ? (sw.fill_chunks > 0 ? std::min(sw.fill_chunks, count / 16) : BA_FILL_CHUNKS) : 1;
    if (early_upload)
    {
        auto room = [](DevBuf& buf, const auto& vec) { return buf.reserve(std::max<size_t>(vec.size(), 1) * sizeof(vec[0])); };
        SNK_TRY(room(h->d_pose, L.pose));
        SNK_TRY(room(h->d_pt, L.pt));
        SNK_TRY(room(h->d_ptc, L.ptc));
        SNK_TRY(room(h->d_camidx, L.camidx));
        SNK_TRY(room(h->d_ptstart, L.ptstart));
        SNK_TRY(room(h->d_oimg, L.oimg));
        SNK_TRY(room(h->d_ouv, L.ouv2));
        SNK_TRY(room(h->d_odepth, L.odepth));
        SNK_TRY(room(h->d_oweight, L.oweight));
        SNK_TRY(room(h->d_oorig, L.oorig));
        SNK_TRY(room(h->d_ocam, L.ocam));
        SNK_TRY(room(h->d_optfree, L.optfree));
        SNK_TRY(room(h->d_optidx, L.optidx));
    }
    for (int ck = 0; ck < n_chunks; ++ck)
    {
        const int b0 = (int)((long long)count * ck / n_chunks), b1 = (int)((long long)count * (ck + 1) / n_chunks);
        SNK_TRY(threaded(b0, b1, [&](int b) { fill_problem(b); }));
        if (early_upload) SNK_TRY(send_chunk(b0, b1));
    }
    sec.lap(SEC_VALUES_SORT);
    return SNK_OK;
}

// ---- the camera lists and the point-major lists of every problem, built with PROBLEM-LOCAL offsets on the host threads (Built) ----

// camera lists of problem b and the room its block entries need: reads the sorted observation arrays, writes Built::camstart / camitems /
// be_nch / ent_bound
void HandOver::build_camera_lists(int b)
{
    const snk_ba_problem& P = problems[b];
    const PreProb& pq       = pre[(size_t)b];
    Built& B                = built[(size_t)b];
    const int nfc = pq.nfc, no = pq.no;
    const int* const pstart = L.ptstart.data() + pq.ps_at;
    const int* const s_cam  = L.ocam.data() + pq.obs_at;
    {
        std::vector<int> cs((size_t)nfc + 1, 0);
        for (int s = 0; s < no; ++s)
            if (s_cam[(size_t)s] >= 0) cs[(size_t)s_cam[(size_t)s] + 1]++;
        for (int c = 0; c < nfc; ++c) cs[(size_t)c + 1] += cs[(size_t)c];
        std::vector<int> items((size_t)cs[(size_t)nfc]);
        std::vector<int> fill(cs.begin(), cs.end() - 1);
        for (int s = 0; s < no; ++s)
            if (s_cam[(size_t)s] >= 0) items[(size_t)fill[(size_t)s_cam[(size_t)s]]++] = s;
        B.camstart.assign(cs.begin(), cs.end());
        B.camitems.swap(items);
        int longest = 0;
        for (int c = 0; c < nfc; ++c) longest = std::max(longest, cs[(size_t)c + 1] - cs[(size_t)c]);
        B.be_nch = ceil_div(longest, 64);
        // (the same list as static records -- what cam_pass streams -- is gathered on the device: gather_cam_records)
    }
    {
        // room for the block entries when the device builds them: every pair of a point's run is the most there can be
        long long bound = 0;
        for (int p = 0; p < P.n_pt; ++p)
        {
            const long long run = pstart[(size_t)p + 1] - pstart[(size_t)p];
            bound += run * run;
        }
        B.ent_bound = bound;
    }
}

// point_wave work items of problem b: consecutive whole points with <= 64 observations in total (writes Built::wv / wv_ok)
void HandOver::build_wave_items(int b)
{
    const snk_ba_problem& P = problems[b];
    Built& B                = built[(size_t)b];
    const int* const pstart = L.ptstart.data() + pre[(size_t)b].ps_at;
    bool ok = true;
    std::vector<int>& wv = B.wv;
    int p = 0;
    while (p < P.n_pt && ok)
    {
        wv.push_back(p);
        int n = 0, q = p;
        while (q < P.n_pt && q - p < 64 && n + (pstart[(size_t)q + 1] - pstart[(size_t)q]) <= 64)
        {
            n += pstart[(size_t)q + 1] - pstart[(size_t)q];
            ++q;
        }
        if (q == p) ok = false;  // a point with more than 64 observations: point_pass handles the problem
        p = q;
    }
    if (ok) wv.push_back(P.n_pt);
    else wv.clear();
    B.wv_ok = ok;
}

// point-major Schur pass, first part: the points of problem b grouped by camera set (writes S.gpts / gsig / ok, Built::cam_sums_bad)
void HandOver::group_points(int b, PointSets& S)
{
    const snk_ba_problem& P = problems[b];
    const PreProb& pq       = pre[(size_t)b];
    Built& B                = built[(size_t)b];
    const int nfc           = pq.nfc;
    const int* const pstart = L.ptstart.data() + pq.ps_at;
    const int* const s_cam  = L.ocam.data() + pq.obs_at;
    std::vector<int> sig;
    // The point-major kernels (schur_fused / schur_mfma / update_cost) are only chosen when the launch has enough work
    // items (max_set_items * count >= SNK_BA_SCHUR_SET_MIN_ITEMS, default 256): for the reference's per-keyframe
    // call -- ONE window of a few thousand points -- their lists are never used, and building + uploading them
    // (0.8 MB of records alone) was a quarter of the 0.9 ms a scene hand-over cost.  Built for batches and for big
    // single scenes (global BA); forced when the threshold is lowered by the environment (tests).
    bool ok = !imp && nfc > 0 && (count >= 8 || P.n_pt >= 8000 || sw.sets_forced);
    // points that produce no Schur products (constant points, points seen by constant cameras only) still need their
    // linearisation (cost, V, b_p): they form groups of their own, keyed by their run length, with no pairs
    std::vector<int> plain_key;
    auto plain_group = [&](int p, int run)
    {
        // (a signature of `run` times -1 cannot be a set with free cameras: the plain group of that run length)
        plain_key.assign((size_t)run, -1);
        S.gpts[(size_t)S.find_group(plain_key)].push_back(p);
    };
    for (int p = 0; p < P.n_pt && ok; ++p)
    {
        const int a0 = pstart[(size_t)p], a1 = pstart[(size_t)p + 1];
        if (a1 - a0 > SET_MAX_RUN) ok = false;
        if (a1 == a0) continue;  // a point without observations: nothing to linearise (update_wave keeps it in place)
        if (P.pt_const[p])
        {
            for (int a = a0; a < a1; ++a)
                if (s_cam[(size_t)a] >= 0) B.cam_sums_bad = true;
            plain_group(p, a1 - a0);
            continue;
        }
        sig.clear();
        int k = 0;
        for (int a = a0; a < a1; ++a)
        {
            const int c = s_cam[(size_t)a];
            sig.push_back(c);
            if (c < 0) continue;
            ++k;
            for (int b = a0; b < a; ++b)
                if (s_cam[(size_t)b] == c) ok = false;  // one camera twice on a point: block-major pass only
        }
        if (k == 0)
        {
            plain_group(p, a1 - a0);
            continue;
        }
        if (k > SET_MAX_K || a1 - a0 > SET_MAX_RUN) ok = false;
        S.gpts[(size_t)S.find_group(sig)].push_back(p);
    }
    S.ok = ok;
}

// second part: every group cut into work items of equal size (SetItem, problem-local offsets), with the pair tables of its camera set
// and the partial sums the items contribute per block and per camera (reads S.gpts / gsig; writes the rest of S, Built::max_*)
void HandOver::cut_work_items(int b, PointSets& S)
{
    Built& B                = built[(size_t)b];
    const int nfc           = pre[(size_t)b].nfc;
    const int* const pstart = L.ptstart.data() + pre[(size_t)b].ps_at;
    S.contrib.resize(imp ? 0 : (size_t)nfc * nfc);
    S.ccontrib.resize((size_t)nfc);
    if (!S.ok) return;
    // groups in order of their first point (std::map order would do as well: any fixed order)
    for (size_t g = 0; g < S.gpts.size(); ++g)
    {
        const std::vector<int>& sig = S.gsig[g];
        const int pair_off = (int)((size_t)0 + S.ipairs.size());
        std::vector<int> blocks;
        for (size_t i = 0; i < sig.size(); ++i)
            for (size_t j = i; j < sig.size(); ++j)
            {
                if (sig[i] < 0 || sig[j] < 0) continue;
                const bool swapped = sig[i] > sig[j];
                const int ra = (int)(swapped ? j : i), rb = (int)(swapped ? i : j);
                S.ipairs.push_back(ra | (rb << 8));
                blocks.push_back(sig[(size_t)ra] * nfc + sig[(size_t)rb]);
            }
        const int npairs = (int)blocks.size();
        // matrix-core form (schur_mfma): the point's free rows ordered by camera index, so that every pair
        // (ra, rb) -- camera(ra) < camera(rb) -- lies in the upper triangle of Y W^T, and the slot of each
        const int aux_off = (int)((size_t)0 + S.ipairs.size());
        std::vector<int> fcams;  // the set's free cameras in ascending order (= the order of the k run positions)
        {
            std::vector<int> fpos;
            for (size_t i = 0; i < sig.size(); ++i)
                if (sig[i] >= 0) fpos.push_back((int)i);
            std::sort(fpos.begin(), fpos.end(), [&](int a, int b) { return sig[(size_t)a] < sig[(size_t)b]; });
            const int kf = (int)fpos.size();
            for (int v : fpos) S.ipairs.push_back(v);
            for (int v : fpos) fcams.push_back(sig[(size_t)v]);
            for (int i = 0; i < kf; ++i)
                for (int j = 0; j < kf; ++j)
                {
                    int slot = -1;
                    if (i <= j)
                        for (int q = 0; q < npairs; ++q)
                            if (S.ipairs[(size_t)(pair_off - (int)(size_t)0) + (size_t)q] == (fpos[(size_t)i] | (fpos[(size_t)j] << 8))) slot = q;
                    S.ipairs.push_back(slot);
                }
            B.max_k = std::max(B.max_k, kf);
        }
        const size_t chunk    = big_items ? SET_CHUNK_BIG : SET_CHUNK;
        const size_t n_in_set = S.gpts[g].size(), n_cuts = (n_in_set + chunk - 1) / chunk;
        size_t cut = (n_in_set + n_cuts - 1) / n_cuts;  // equal S.items: a launch ends with its longest item
        {
            // schur_fused linearises 64 / run points at a time: whole groups of that many per item where possible
            const size_t grp = std::min<size_t>(64 / std::max<size_t>(sig.size(), 1), 16);  // SF_GMAX
            cut = std::min<size_t>((cut + grp - 1) / grp * grp, big_items ? 128 : 64);
        }
        for (size_t q0 = 0; q0 < n_in_set; q0 += cut)
        {
            SetItem si;
            si.pts_off  = (int)((size_t)0 + S.ipts.size());
            si.n_pts    = (int)std::min<size_t>(cut, n_in_set - q0);
            si.pair_off = pair_off;
            si.npairs   = npairs;
            si.part_off = S.parts;
            si.run      = (int)sig.size();
            si.aux_off  = aux_off;
            si.nfree    = 0;
            si.rec_off  = (int)S.recs;
            for (int v : sig) si.nfree += v >= 0 ? 1 : 0;
            si.cpart_off = S.cparts;
            for (int f = 0; f < si.nfree; ++f) S.ccontrib[(size_t)fcams[(size_t)f]].push_back(S.cparts + f);
            S.cparts += si.nfree;
            for (int q = 0; q < si.n_pts; ++q)
            {
                const int pp = S.gpts[g][q0 + (size_t)q];
                S.ipts.push_back(make_int2(pp, pstart[(size_t)pp]));
            }
            S.recs += (long long)si.n_pts * si.run;
            if (S.recs >= (1ll << 31)) S.ok = false;  // (would not be addressable by rec_off: the block-major pass then)
            for (int q = 0; q < npairs; ++q) S.contrib[(size_t)blocks[(size_t)q]].push_back(S.parts + q);
            S.parts += npairs;
            S.items.push_back(si);
            B.max_pairs = std::max(B.max_pairs, npairs);
            B.max_run   = std::max(B.max_run, si.run);
        }
    }
}

// third part: the per-camera and per-block lists of the partial sums (fixed order), and the work items into Built
void HandOver::build_block_lists(int b, PointSets& S)
{
    Built& B        = built[(size_t)b];
    const int nfc   = pre[(size_t)b].nfc;
    const size_t nb = imp ? 0 : (size_t)nfc * nfc;
    const bool ok   = S.ok;
    {
        int crun = 0;
        for (int c = 0; c < nfc; ++c)
        {
            B.ccstart.push_back(crun);
            if (ok)
            {
                B.ccitems.insert(B.ccitems.end(), S.ccontrib[(size_t)c].begin(), S.ccontrib[(size_t)c].end());
                crun += (int)S.ccontrib[(size_t)c].size();
            }
        }
        B.ccstart.push_back(crun);
    }
    B.ok = ok;
    if (ok)
    {
        B.items.swap(S.items);
        B.ipts.swap(S.ipts);
        B.ipairs.swap(S.ipairs);
        B.parts  = S.parts;
        B.cparts = S.cparts;
        B.recs   = S.recs;
    }
    int run = 0;
    B.cblkstart.resize(nb + 1);
    int* cb = B.cblkstart.data();
    for (size_t k = 0; k < nb; ++k)
    {
        cb[k] = run;
        if (ok && !S.contrib[k].empty())
        {
            B.cblkitems.insert(B.cblkitems.end(), S.contrib[k].begin(), S.contrib[k].end());
            run += (int)S.contrib[k].size();
        }
    }
    cb[nb] = run;
}

int HandOver::build_problem_lists()
{
    SNK_TRY(threaded(0, count, [&](int b)
    {
        build_camera_lists(b);
        build_wave_items(b);
        PointSets S;
        group_points(b, S);
        cut_work_items(b, S);
        build_block_lists(b, S);
    }));
    sec.lap(SEC_CAMERA_LISTS);
    return SNK_OK;
}

// relative pose constraints of problem b (IMU scenes): valid ones, per-camera incidence, per-block chains.  Appends to L.rpcmeta /
// rpcnext / camrpcstart / camrpcitems / blkrpc, writes the constraint fields of the problem's Prob record
int HandOver::merge_constraints(int b)
{
    const snk_ba_problem& P = problems[b];
    Prob& pr                = L.probs[(size_t)b];
    const int nfc           = pr.nfc;
    const int* const cidx   = L.camidx.data() + pre[(size_t)b].img_at;
    pr.rpc_off    = (int)L.rpcmeta.size();
    pr.camrpc_off = (int)L.camrpcstart.size();
    std::vector<int> cs((size_t)nfc + 1, 0);
    std::vector<RpcMeta> mine;
    for (int k = 0; k < P.n_rpc; ++k)
    {
        const snk_ba_rpc& q = P.rpc[k];
        if (q.img1 < 0 || q.img2 < 0 || q.img1 >= P.n_img || q.img2 >= P.n_img || q.img1 == q.img2) continue;
        if (P.img_const[q.img1] && P.img_const[q.img2]) continue;
        SNK_REQUIRE(q.weight_rotation >= 0.0 && q.weight_translation >= 0.0, "negative constraint weight");
        RpcMeta m;
        m.img1 = q.img1; m.img2 = q.img2;
        m.c1 = cidx[(size_t)q.img1]; m.c2 = cidx[(size_t)q.img2];
        for (int t = 0; t < 7; ++t) m.rel[t] = q.rel_pose[t];
        m.w_rot = q.weight_rotation; m.w_trans = q.weight_translation;
        mine.push_back(m);
        if (m.c1 >= 0) cs[(size_t)m.c1 + 1]++;
        if (m.c2 >= 0) cs[(size_t)m.c2 + 1]++;
    }
    pr.n_rpc = (int)mine.size();
    tot.max_rpc  = std::max(tot.max_rpc, pr.n_rpc);
    for (int c = 0; c < nfc; ++c) cs[(size_t)c + 1] += cs[(size_t)c];
    const int item_base = (int)L.camrpcitems.size();
    std::vector<int> items((size_t)cs[(size_t)nfc]), fill(cs.begin(), cs.end() - 1);
    // the per-block chains are only read for problems that HAVE constraints: the others advance the offset and write nothing
    // (implicit form: no per-block chains -- its camera phase walks the per-camera lists)
    std::vector<int> brpc(mine.empty() || imp ? 0 : (size_t)nfc * nfc, 0), nxt(mine.size(), 0);
    for (int k = 0; k < (int)mine.size(); ++k)
    {
        const RpcMeta& m = mine[(size_t)k];
        if (m.c1 >= 0) items[(size_t)fill[(size_t)m.c1]++] = k * 2;
        if (m.c2 >= 0) items[(size_t)fill[(size_t)m.c2]++] = k * 2 + 1;
        if (m.c1 >= 0 && m.c2 >= 0 && !imp)
        {
            // the upper block (lo, hi) holds J(lo)^T J(hi): H12 when img1 is `lo`, its transpose otherwise
            const int lo = std::min(m.c1, m.c2), hi = std::max(m.c1, m.c2);
            const int code = 1 + (k * 2 + (m.c1 == lo ? 0 : 1));
            nxt[(size_t)k]                 = brpc[(size_t)lo * nfc + hi];
            brpc[(size_t)lo * nfc + hi] = code;
        }
    }
    for (int c = 0; c <= nfc; ++c) L.camrpcstart.push_back(item_base + cs[(size_t)c]);
    L.camrpcitems.insert(L.camrpcitems.end(), items.begin(), items.end());
    if (!mine.empty() && !imp)
    {
        L.blkrpc.resize(tot.blkrpc_logical, 0);  // zeros for the problems without constraints in front of this one
        L.blkrpc.insert(L.blkrpc.end(), brpc.begin(), brpc.end());
    }
    if (!imp) tot.blkrpc_logical += (size_t)nfc * nfc;
    L.rpcnext.insert(L.rpcnext.end(), nxt.begin(), nxt.end());
    L.rpcmeta.insert(L.rpcmeta.end(), mine.begin(), mine.end());
    return SNK_OK;
}

// The serial loop over the problems: reads PreProb and Built, writes the Prob records (L.probs), MergeAt, the running totals and the
// constraint lists; h->orig_off / orig_n
int HandOver::merge_decide()
{
    for (int b = 0; b < count; ++b)
    {
        const snk_ba_problem& P = problems[b];
        sec.lap(SEC_REST);
        Prob& pr = L.probs[(size_t)b];
        memset(&pr, 0, sizeof(pr));
        pr.ni = P.n_img;
        pr.np = P.n_pt;
        for (int k = 0; k < 4; ++k) pr.K[k] = P.K[k];
        pr.bf       = P.bf;
        pr.img_off  = tot.img_off;
        pr.pt_off   = tot.pt_off;
        pr.obs_off  = tot.obs_off;
        pr.cam_off  = tot.cam_off;
        pr.orig_off = tot.orig_off;
        pr.vec_off  = tot.vec_off;
        pr.s_off    = tot.s_off;
        h->orig_off[(size_t)b] = tot.orig_off;
        h->orig_n[(size_t)b]   = P.n_obs;
        // values, free-camera indices, counting sort and the sorted observation arrays: written by the fill pass
        const PreProb& pq = pre[(size_t)b];
        const int nfc     = pq.nfc;
        pr.nfc = nfc;
        pr.n6  = 6 * nfc;
        const int no = pq.no;
        pr.no        = no;
        pr.ptstart_off = (int)pq.ps_at;
        if (pq.dup) tot.dev_entries_ok = false;
        const Built& B = built[(size_t)b];
        MergeAt& M     = at[(size_t)b];
        // point_wave work items (Built::wv)
        pr.wv_off = (int)tot.n_wvpt;
        pr.n_wv   = 0;
        M.wvpt    = tot.n_wvpt;
        if (B.wv_ok)
        {
            pr.n_wv = (int)B.wv.size() - 1;
            tot.n_wvpt += B.wv.size();
            tot.max_wv = std::max(tot.max_wv, pr.n_wv);
        }
        else
            tot.wave_ok = false;
        sec.lap(SEC_WAVE_ITEMS);
        // camera lists (Built; positions and items are problem-local: appended as they are)
        pr.camstart_off = (int)tot.n_camstart;
        pr.citem_off    = (int)tot.n_camitems;
        M.camstart = tot.n_camstart, M.camitems = tot.n_camitems;
        tot.n_camstart += B.camstart.size();
        tot.n_camitems += B.camitems.size();
        tot.max_citems = std::max(tot.max_citems, (int)B.camitems.size());
        pr.be_nch  = B.be_nch;
        if (nfc > BE_MAX_CAMS) tot.dev_entries_ok = false;
        ent_bound[(size_t)b] = B.ent_bound;
        pr.blkstart_off = tot.blkstart_total;
        if (!imp) tot.blkstart_total += nfc * nfc + 1;
        sec.lap(SEC_CAMERA_LISTS);
        // point-major Schur pass (Built, problem-local offsets): append, relocating by the running totals
        pr.set_off  = (int)tot.n_setitems;
        pr.cblk_off = (int)tot.n_cblkstart;
        pr.n_set    = 0;
        {
            if (B.cam_sums_bad) tot.cam_sums_ok = false;
            tot.max_set_k     = std::max(tot.max_set_k, B.max_k);
            tot.max_set_pairs = std::max(tot.max_set_pairs, B.max_pairs);
            tot.max_set_run   = std::max(tot.max_set_run, B.max_run);
            pr.ccam_off = (int)tot.n_ccstart;
            M.ccstart = tot.n_ccstart, M.ccitems = tot.n_ccitems;  // ccstart entries + base_cc (= M.ccitems), ccitems entries + base_cparts
            tot.n_ccstart += B.ccstart.size();
            tot.n_ccitems += B.ccitems.size();
            M.base_parts = tot.n_partials, M.base_cparts = tot.n_cparts, M.base_rec = tot.n_setrec;
            // the batch's record / partial-sum counters are 32-bit on the device: a batch that would overflow them keeps the block-major pass
            // (what the serial builder of round 3 did), it is not an error
            const bool set_fits = tot.n_setrec + B.recs < (1ll << 31) && (long long)tot.n_partials + B.parts < (1ll << 31);
            M.set = B.ok && set_fits;
            M.setitems = tot.n_setitems, M.setpts = tot.n_setpts, M.setpairs = tot.n_setpairs;
            if (M.set)
            {
                tot.n_setitems += B.items.size();
                tot.n_setpts += B.ipts.size();
                tot.n_setpairs += B.ipairs.size();
                pr.n_set      = (int)B.items.size();
                tot.max_set_items = std::max(tot.max_set_items, pr.n_set);
            }
            else
                tot.set_ok = false;
            M.cblkstart = tot.n_cblkstart, M.cblkitems = tot.n_cblkitems;  // cblkstart entries + base_cb (= M.cblkitems), cblkitems entries + base_parts
            tot.n_cblkstart += B.cblkstart.size();
            tot.n_cblkitems += B.cblkitems.size();
            if (M.set)
            {
                tot.n_partials += B.parts;
                tot.n_cparts += B.cparts;
                tot.n_setrec += B.recs;
            }
        }
        sec.lap(SEC_BLOCK_LISTS);
        SNK_TRY(merge_constraints(b));
        sec.lap(SEC_CONSTRAINTS);
        tot.img_off += P.n_img;
        tot.pt_off += P.n_pt;
        tot.obs_off += no;
        tot.cam_off += nfc;
        tot.orig_off += P.n_obs;
        tot.vec_off += pr.n6;
        if (!imp) tot.s_off += (long long)pr.n6 * pr.n6;
        tot.max_np  = std::max(tot.max_np, P.n_pt);
        tot.max_ni  = std::max(tot.max_ni, P.n_img);
        tot.max_nfc = std::max(tot.max_nfc, nfc);
        tot.max_n6  = std::max(tot.max_n6, pr.n6);
    }
    return SNK_OK;
}

// ---- the element copies merge_decide left out: every problem's lists (Built) into its ranges (MergeAt) of the shared lists, relocated,
// on the host threads (disjoint ranges, no locks) ----
int HandOver::merge_copy()
{
    L.wvpt.resize(tot.n_wvpt), L.camstart.resize(tot.n_camstart), L.camitems.resize(tot.n_camitems), L.ccstart.resize(tot.n_ccstart), L.ccitems.resize(tot.n_ccitems);
    L.setitems.resize(tot.n_setitems), L.setpts.resize(tot.n_setpts), L.setpairs.resize(tot.n_setpairs), L.cblkstart.resize(tot.n_cblkstart), L.cblkitems.resize(tot.n_cblkitems);
    return threaded(0, count, [&](int b)
    {
        const Built& B   = built[(size_t)b];
        const MergeAt& M = at[(size_t)b];
        auto put = [](auto& dst, size_t pos, const auto& src)
        {
            if (!src.empty()) memcpy(dst.data() + pos, src.data(), src.size() * sizeof(src[0]));
        };
        if (B.wv_ok) put(L.wvpt, M.wvpt, B.wv);
        put(L.camstart, M.camstart, B.camstart);
        put(L.camitems, M.camitems, B.camitems);
        {
            int* d = L.ccstart.data() + M.ccstart;
            for (size_t k = 0; k < B.ccstart.size(); ++k) d[k] = B.ccstart[k] + (int)M.ccitems;
            d = L.ccitems.data() + M.ccitems;
            for (size_t k = 0; k < B.ccitems.size(); ++k) d[k] = B.ccitems[k] + M.base_cparts;
            d = L.cblkstart.data() + M.cblkstart;
            for (size_t k = 0; k < B.cblkstart.size(); ++k) d[k] = B.cblkstart[k] + (int)M.cblkitems;
            d = L.cblkitems.data() + M.cblkitems;
            for (size_t k = 0; k < B.cblkitems.size(); ++k) d[k] = B.cblkitems[k] + M.base_parts;
        }
        if (M.set)
        {
            SetItem* d = L.setitems.data() + M.setitems;
            for (size_t k = 0; k < B.items.size(); ++k)
            {
                SetItem si = B.items[k];
                si.pts_off += (int)M.setpts;
                si.pair_off += (int)M.setpairs;
                si.aux_off += (int)M.setpairs;
                si.part_off += M.base_parts;
                si.cpart_off += M.base_cparts;
                si.rec_off += (int)M.base_rec;
                d[k] = si;
            }
            put(L.setpts, M.setpts, B.ipts);
            put(L.setpairs, M.setpairs, B.ipairs);
        }
    });
}

// the totals of the set into the handle (ba_sets_will_run and ba_plan_pcg read them there)
int HandOver::publish_totals()
{
    h->count = count;
    h->tot_img = tot.img_off; h->tot_pt = tot.pt_off; h->tot_obs = tot.obs_off; h->tot_cam = tot.cam_off; h->tot_orig = tot.orig_off;
    h->tot_vec = tot.vec_off; h->tot_s = tot.s_off;
    h->max_np = tot.max_np; h->max_nfc = tot.max_nfc; h->max_n6 = tot.max_n6; h->max_ni = tot.max_ni;
    h->max_wv = tot.max_wv;
    h->max_rpc = tot.max_rpc;
    h->point_wave_ok = tot.wave_ok && tot.max_wv > 0;
    return SNK_OK;
}

// camera-pair blocks on the host: co-observations of every ordered pair (dense block grid, empty blocks allowed).  The
// builder for scenes the device kernels do not take (more than 512 free cameras, one camera twice on a point), and their checker.
void HandOver::host_block_entries(int b, pvec<int>& bs_out, pvec<int4>& ent_out) const
{
    const snk_ba_problem& P = problems[b];
    const Prob& pr          = L.probs[(size_t)b];
    const int nfc           = pr.nfc;
    const int* pstart       = L.ptstart.data() + pr.ptstart_off;
    const int* s_cam        = L.ocam.data() + pr.obs_off;
    const size_t nb = (size_t)nfc * nfc;
    std::vector<int> bs(nb + 1, 0);
    for (int p = 0; p < P.n_pt; ++p)
    {
        if (P.pt_const[p]) continue;
        for (int a = pstart[(size_t)p]; a < pstart[(size_t)p + 1]; ++a)
        {
            if (s_cam[(size_t)a] < 0) continue;
            for (int c = pstart[(size_t)p]; c < pstart[(size_t)p + 1]; ++c)  // upper blocks only: schur_pass never reads the others
                if (s_cam[(size_t)c] >= s_cam[(size_t)a]) bs[(size_t)s_cam[(size_t)a] * nfc + s_cam[(size_t)c] + 1]++;
        }
    }
    for (size_t k = 0; k < nb; ++k) bs[k + 1] += bs[k];
    const size_t ent_at = ent_out.size();
    ent_out.resize(ent_at + (size_t)bs[nb]);  // filled in place (no second copy of a megabyte of entries)
    int4* ent = ent_out.data() + ent_at;
    std::vector<int> fill(bs.begin(), bs.end() - 1);
    for (int p = 0; p < P.n_pt; ++p)
    {
        if (P.pt_const[p]) continue;
        for (int a = pstart[(size_t)p]; a < pstart[(size_t)p + 1]; ++a)
        {
            if (s_cam[(size_t)a] < 0) continue;
            for (int c = pstart[(size_t)p]; c < pstart[(size_t)p + 1]; ++c)
                if (s_cam[(size_t)c] >= s_cam[(size_t)a])
                {
                    int4 e;
                    e.x = a;
                    e.y = c;
                    e.z = p;
                    e.w = 0;
                    ent[(size_t)fill[(size_t)s_cam[(size_t)a] * nfc + s_cam[(size_t)c]]++] = e;
                }
        }
    }
    bs_out.insert(bs_out.end(), bs.begin(), bs.end());
}

// block entries: on the device when every problem qualifies, by the host builder otherwise.  Reads the Prob records, PreProb::dup (through
// tot.dev_entries_ok) and ent_bound; writes Prob::ent_off / becnt_off / be_nch, tot.dev_entries and its totals, h->probs
int HandOver::plan_block_entries()
{
    tot.dev_entries = tot.dev_entries_ok && !sw.host_entries && !imp;
    if (tot.dev_entries)
    {
        // The device builder counts into nfc x chunks x nfc ints per problem -- quadratic in the free cameras.  A global BA with
        // ~500 free cameras and one long camera list needs hundreds of megabytes of counters the host builder never allocates:
        // beyond a modest budget (64 MB; a batch of 1024 local windows needs 1.6 MB) the host builder takes over.
        long long cnt = 0;
        for (int b = 0; b < count; ++b) cnt += (long long)L.probs[(size_t)b].nfc * L.probs[(size_t)b].be_nch * L.probs[(size_t)b].nfc;
        if (cnt * (long long)sizeof(int) > sw.becnt_budget) tot.dev_entries = false;
    }
    if (tot.dev_entries)
    {
        for (int b = 0; b < count; ++b)
        {
            Prob& pr = L.probs[(size_t)b];
            SNK_REQUIRE(tot.ent_total + ent_bound[(size_t)b] < (1ll << 31), "scene list too large (block entries)");
            pr.ent_off   = (int)tot.ent_total;
            pr.becnt_off = (int)tot.becnt_total;
            tot.ent_total += ent_bound[(size_t)b];
            tot.becnt_total += (long long)pr.nfc * pr.be_nch * pr.nfc;
            SNK_REQUIRE(tot.becnt_total < (1ll << 31), "scene list too large (block entry counters)");
            tot.max_be_waves = std::max(tot.max_be_waves, pr.nfc * pr.be_nch);
        }
    }
    else if (!imp)
    {
        long long bound = 0;
        for (int b = 0; b < count; ++b) bound += ent_bound[(size_t)b];
        L.blkent.reserve((size_t)bound);  // one pinned allocation instead of a doubling chain
        L.blkstart.reserve((size_t)tot.blkstart_total);
        for (int b = 0; b < count; ++b)
        {
            L.probs[(size_t)b].be_nch  = 0;
            L.probs[(size_t)b].ent_off = (int)L.blkent.size();
            host_block_entries(b, L.blkstart, L.blkent);
        }
    }
    h->probs.assign(L.probs.begin(), L.probs.end());  // with the block-entry offsets
    sec.lap(SEC_BLOCK_ENTRIES);
    t_lists = std::chrono::steady_clock::now();
    return SNK_OK;
}

// a device-to-device copy behind the upload (tab2)
int HandOver::dup(DevBuf& dst, const DevBuf& src, size_t bytes)
{
    int rc2 = dst.reserve(std::max<size_t>(bytes, 1));
    if (rc2 != SNK_OK || bytes == 0) return rc2;
    SNK_REQUIRE(tab2.n < COPY_TAB_MAX && bytes < (1ull << 32), "scene list too large for the upload table");
    tab2.src[tab2.n] = src.p, tab2.dst[tab2.n] = dst.p, tab2.bytes[tab2.n] = (unsigned)bytes;
    ++tab2.n;
    return SNK_OK;
}

// The lists that are not on their way yet into the upload table (tab), their device buffers reserved; the buffers of the lists the
// device builds (cs_obs, set_obs, block entries) reserved
int HandOver::upload_rest()
{
    SNK_TRY(upload(h->d_prob, L.probs, tab));
    if (!early_upload) { SNK_TRY(upload(h->d_pose, L.pose, tab)); }
    if (!dup_on_device) { SNK_TRY(upload(h->d_pose0, L.pose, tab)); }
    else SNK_TRY(dup(h->d_pose0, h->d_pose, (size_t)tot.img_off * 7 * sizeof(double)));  // (by the totals: device rows leave L.pose empty)
    if (!early_upload) { SNK_TRY(upload(h->d_pt, L.pt, tab)); }
    if (!dup_on_device) { SNK_TRY(upload(h->d_pt0, L.pt, tab)); }
    else SNK_TRY(dup(h->d_pt0, h->d_pt, (size_t)tot.pt_off * 3 * sizeof(double)));
    if (!early_upload)
    {
        SNK_TRY(upload(h->d_ptc, L.ptc, tab));
        SNK_TRY(upload(h->d_camidx, L.camidx, tab));
        SNK_TRY(upload(h->d_ptstart, L.ptstart, tab));
        SNK_TRY(upload(h->d_oimg, L.oimg, tab));
        SNK_TRY(upload(h->d_ocam, L.ocam, tab));
        SNK_TRY(upload(h->d_optfree, L.optfree, tab));
        SNK_TRY(upload(h->d_ouv, L.ouv2, tab));
        SNK_TRY(upload(h->d_odepth, L.odepth, tab));
        SNK_TRY(upload(h->d_oweight, L.oweight, tab));
        SNK_TRY(upload(h->d_oorig, L.oorig, tab));
    }
    SNK_TRY(upload(h->d_camstart, L.camstart, tab));
    if (!early_upload) { SNK_TRY(upload(h->d_camitems, L.camitems, tab)); }
    else SNK_TRY(h->d_camitems.reserve(std::max<size_t>(L.camitems.size(), 1) * sizeof(int)));
    SNK_TRY(h->d_csobs.reserve(std::max<size_t>(L.camitems.size(), 1) * sizeof(CamObs)));  // gather_cam_records
    SNK_TRY(upload(h->d_setitems, L.setitems, tab));
    SNK_TRY(h->d_setobs.reserve((size_t)std::max<long long>(tot.n_setrec, 1) * sizeof(SetObs)));  // gather_set_records
    SNK_TRY(upload(h->d_setpts, L.setpts, tab));
    SNK_TRY(upload(h->d_setpairs, L.setpairs, tab));
    SNK_TRY(upload(h->d_cblkstart, L.cblkstart, tab));
    SNK_TRY(upload(h->d_cblkitems, L.cblkitems, tab));
    SNK_TRY(upload(h->d_ccstart, L.ccstart, tab));
    SNK_TRY(upload(h->d_ccitems, L.ccitems, tab));
    if (tot.dev_entries)
    {
        SNK_TRY(h->d_blkstart.reserve((size_t)std::max(tot.blkstart_total, 1) * sizeof(int)));
        SNK_TRY(h->d_blkent.reserve((size_t)std::max<long long>(tot.ent_total, 1) * sizeof(int4)));
        SNK_TRY(h->d_becnt.reserve((size_t)std::max<long long>(tot.becnt_total, 1) * sizeof(int)));
    }
    else
    {
        SNK_TRY(upload(h->d_blkstart, L.blkstart, tab));
        SNK_TRY(upload(h->d_blkent, L.blkent, tab));
    }
    if (!early_upload) { SNK_TRY(upload(h->d_optidx, L.optidx, tab)); }
    SNK_TRY(upload(h->d_wvpt, L.wvpt, tab));
    SNK_TRY(upload(h->d_rpcmeta, L.rpcmeta, tab));
    SNK_TRY(upload(h->d_rpcnext, L.rpcnext, tab));
    SNK_TRY(upload(h->d_camrpcstart, L.camrpcstart, tab));
    SNK_TRY(upload(h->d_camrpcitems, L.camrpcitems, tab));
    SNK_TRY(upload(h->d_blkrpc, L.blkrpc, tab));
    if (!dup_on_device) { SNK_TRY(upload(h->d_pt_new, L.pt, tab)); }  // points without observations stay put
    else SNK_TRY(dup(h->d_pt_new, h->d_pt, (size_t)tot.pt_off * 3 * sizeof(double)));
    t_up = std::chrono::steady_clock::now();
    return SNK_OK;
}

// the solver's work arrays, the kernel-choice facts of the set in the handle, the PCG plan
int HandOver::reserve_work()
{
    const size_t nobs = (size_t)std::max(tot.obs_off, 1), npt = (size_t)std::max(tot.pt_off, 1);
    SNK_TRY(h->d_state.reserve((size_t)count * sizeof(State)));
    SNK_TRY(h->d_pose_new.reserve((size_t)std::max(tot.img_off, 1) * 7 * 8));
    SNK_TRY(h->d_pt_new.reserve(npt * 3 * 8));
    SNK_TRY(h->d_outlier.reserve((size_t)std::max(tot.orig_off, 1)));
    SNK_TRY(h->d_chi2.reserve((size_t)std::max(tot.orig_off, 1) * 8));
    SNK_TRY(h->d_r.reserve(nobs * 4 * 8));
    SNK_TRY(h->d_W.reserve(nobs * 18 * 8));
    SNK_TRY(h->d_ptv.reserve(npt * 6 * 8));
    SNK_TRY(h->d_spart.reserve((size_t)std::max(tot.n_partials, 1) * 36 * 8));
    SNK_TRY(h->d_campart.reserve((size_t)std::max(tot.n_cparts, 1) * CS_TERMS * 8));
    h->cam_sums_ok = tot.cam_sums_ok;
    h->set_ok = tot.set_ok && tot.max_set_items > 0;
    h->max_set_items = tot.max_set_items;
    h->set_small     = tot.max_set_pairs * 6 <= 4 * 64 && tot.max_set_run * 9 + 3 <= 2 * 64;
    h->set_k_max     = tot.max_set_k;
    h->set_run_max   = tot.max_set_run;
    SNK_TRY(h->d_Vinv.reserve(npt * 6 * 8));
    SNK_TRY(h->d_bp.reserve(npt * 3 * 8));
    SNK_TRY(h->d_cost.reserve(npt * 8));
    SNK_TRY(h->d_cost_new.reserve(npt * 8));
    SNK_TRY(h->d_U.reserve((size_t)std::max(tot.cam_off, 1) * 36 * 8));
    SNK_TRY(h->d_S.reserve((size_t)std::max<long long>(tot.s_off, 1) * 8));
    SNK_TRY(h->d_rhs.reserve((size_t)std::max(tot.vec_off, 1) * 8));
    SNK_TRY(h->d_x.reserve((size_t)std::max(tot.vec_off, 1) * 8));
    SNK_TRY(h->d_rpcout.reserve(std::max<size_t>(L.rpcmeta.size(), 1) * RPC_STRIDE * 8));
    return ba_plan_pcg(h);
}

// a buffer that starts as zeros: an entry of the upload table with no source
int HandOver::zero(DevBuf& b, size_t bytes)
{
    SNK_REQUIRE(tab.n < COPY_TAB_MAX && bytes < (1ull << 32), "scene list too large for the upload table");
    tab.src[tab.n] = nullptr, tab.dst[tab.n] = b.p, tab.bytes[tab.n] = (unsigned)bytes;
    ++tab.n;
    return SNK_OK;
}

// ... and the buffers that start as zeros are entries of the same table (source NULL): nine fill launches of ~5 us each
// stood between the upload and the first kernel of the solve.  Then the one launch of the table (two for batches).
int HandOver::zero_and_launch()
{
    const size_t nobs = (size_t)std::max(tot.obs_off, 1), npt = (size_t)std::max(tot.pt_off, 1);
    hipStream_t st = h->stream;
    SNK_TRY(zero(h->d_outlier, (size_t)std::max(tot.orig_off, 1)));
    {
        // the state starts as begin_solve would leave it (the first solve of the scene then needs no launch for that)
        auto& states = L.states;
        State s0{};
        s0.lambda = make_opt(h->opt).lambda_init;
        s0.vfac   = 2.0;
        states.assign((size_t)count, s0);
        SNK_REQUIRE(tab.n < COPY_TAB_MAX, "scene list too large for the upload table");
        tab.src[tab.n] = states.data(), tab.dst[tab.n] = h->d_state.p, tab.bytes[tab.n] = (unsigned)(states.size() * sizeof(State));
        ++tab.n;
        h->state_fresh = true;
    }
    SNK_TRY(zero(h->d_r, nobs * 4 * 8));
    SNK_TRY(zero(h->d_x, (size_t)std::max(tot.vec_off, 1) * 8));
    // points without observations are in no work item of schur_fused: their cost, V^-1 and b_p are zero once and for all
    SNK_TRY(zero(h->d_cost, npt * 8));
    SNK_TRY(zero(h->d_cost_new, npt * 8));
    SNK_TRY(zero(h->d_Vinv, npt * 6 * 8));
    SNK_TRY(zero(h->d_bp, npt * 3 * 8));
    {
        // enough workgroups per array to keep the bus busy: one per 64 KB of the largest list, 16 .. 256
        unsigned big = 0;
        for (int e = 0; e < tab.n; ++e) big = std::max(big, tab.bytes[e]);
        for (int e = 0; e < tab.n; ++e) bytes_up += tab.src[e] ? tab.bytes[e] : 0;  // (tab2 is device to device)
        // (more workgroups per array do not shorten it: 16.3 / 18.3 / 17.1 / 15.2 us with one per 64 / 16 / 4 / 1 KB, r03ag)
        const int gx = (int)std::min(256u, std::max(16u, big >> 16));
        hipLaunchKernelGGL(copy_table_kernel, dim3(gx, tab.n), dim3(256), 0, st, tab);
        SNK_LAUNCH_CHECK();
        if (tab2.n > 0)
        {
            hipLaunchKernelGGL(copy_table_kernel, dim3(gx, tab2.n), dim3(256), 0, st, tab2);  // stream-ordered behind the upload
            SNK_LAUNCH_CHECK();
        }
    }
    bind_arrays();
    return launch_device_lists();
}

void HandOver::bind_arrays()
{
    Arrays& A   = h->arr;
    A.prob      = h->d_prob.as<Prob>();
    A.state     = h->d_state.as<State>();
    A.pose      = h->d_pose.as<double>();
    A.pose_new  = h->d_pose_new.as<double>();
    A.pt        = h->d_pt.as<double>();
    A.pt_new    = h->d_pt_new.as<double>();
    A.pt_const  = h->d_ptc.as<unsigned char>();
    A.cam_idx   = h->d_camidx.as<int>();
    A.pt_start  = h->d_ptstart.as<int>();
    A.o_img     = h->d_oimg.as<int>();
    A.o_cam     = h->d_ocam.as<int>();
    A.o_ptfree  = h->d_optfree.as<unsigned char>();
    A.o_uv      = h->d_ouv.as<double2>();
    A.o_depth   = h->d_odepth.as<double>();
    A.o_weight  = h->d_oweight.as<double>();
    A.o_orig    = h->d_oorig.as<int>();
    A.o_pt      = h->d_optidx.as<int>();
    A.wv_pt     = h->d_wvpt.as<int>();
    A.rpc_meta  = h->d_rpcmeta.as<RpcMeta>();
    A.rpc_out   = h->d_rpcout.as<double>();
    A.cam_rpc_start = h->d_camrpcstart.as<int>();
    A.cam_rpc_items = h->d_camrpcitems.as<int>();
    A.blk_rpc   = h->d_blkrpc.as<int>();
    A.rpc_next  = h->d_rpcnext.as<int>();
    A.outlier   = h->d_outlier.as<unsigned char>();
    A.o_r       = h->d_r.as<double>();
    A.o_W       = h->d_W.as<double>();
    A.ptv       = h->d_ptv.as<double>();
    A.cs_obs    = h->d_csobs.as<CamObs>();
    A.set_items = h->d_setitems.as<SetItem>();
    A.set_obs   = h->d_setobs.as<SetObs>();
    A.set_pts   = h->d_setpts.as<int2>();
    A.set_pairs = h->d_setpairs.as<int>();
    A.cc_start   = h->d_ccstart.as<int>();
    A.cc_items   = h->d_ccitems.as<int>();
    A.cam_part   = h->d_campart.as<double>();
    A.cblk_start = h->d_cblkstart.as<int>();
    A.cblk_items = h->d_cblkitems.as<int>();
    A.s_part    = h->d_spart.as<double>();
    A.Vinv      = h->d_Vinv.as<double>();
    A.bp        = h->d_bp.as<double>();
    A.cost_pt   = h->d_cost.as<double>();
    A.cost_pt_new = h->d_cost_new.as<double>();
    A.U         = h->d_U.as<double>();
    A.cam_start = h->d_camstart.as<int>();
    A.cam_items = h->d_camitems.as<int>();
    A.blk_start = h->d_blkstart.as<int>();
    A.blk_ent   = h->d_blkent.as<int4>();
    A.S         = h->d_S.as<double>();
    A.rhs       = h->d_rhs.as<double>();
    A.x         = h->d_x.as<double>();
    A.chi2      = h->d_chi2.as<double>();
}

// the lists the device builds from the uploaded ones (stream ordered behind copy_table_kernel)
int HandOver::launch_device_lists()
{
    const Arrays& A = h->arr;
    hipStream_t st  = h->stream;
    if (early_upload)
    {
        if (tot.obs_off > 0)
        {
            int max_no = 0;
            for (int b = 0; b < count; ++b) max_no = std::max(max_no, L.probs[(size_t)b].no);
            hipLaunchKernelGGL(derive_obs_fields, dim3(ceil_div(std::max(max_no, 1), 256), count), dim3(256), 0, st, A, h->d_optidx.as<int>(), h->d_ocam.as<int>(),
                               h->d_optfree.as<unsigned char>());
            SNK_LAUNCH_CHECK();
        }
        if (tot.max_nfc > 0 && tot.max_citems > 0)
        {
            hipLaunchKernelGGL(derive_cam_items, dim3(tot.max_nfc, count), dim3(64), 0, st, A, (const int*)h->d_ocam.as<int>(), h->d_camitems.as<int>());
            SNK_LAUNCH_CHECK();
        }
    }
    if (tot.max_citems > 0)
    {
        hipLaunchKernelGGL(gather_cam_records, dim3(ceil_div(tot.max_citems, 256), count), dim3(256), 0, st, A, h->d_csobs.as<CamObs>());
        SNK_LAUNCH_CHECK();
    }
    if (tot.max_set_items > 0)
    {
        hipLaunchKernelGGL(gather_set_records, dim3(tot.max_set_items, count), dim3(256), 0, st, A, h->d_setobs.as<SetObs>());
        SNK_LAUNCH_CHECK();
    }
    // batches that will run the point-major kernels never read the block entries (SNK_BA_CHECK_LISTS=1 builds and checks them anyway)
    const bool skip_entries = tot.dev_entries && count >= 16 && ba_sets_will_run(h) && !sw.check_lists;
    h->blk_built = !skip_entries && !imp;
    if (tot.dev_entries && !skip_entries)
    {
        if (tot.max_be_waves > 0)
        {
            hipLaunchKernelGGL(block_entries_count, dim3(tot.max_be_waves, count), dim3(64), 0, st, A, h->d_becnt.as<int>());
            SNK_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(block_entries_scan, dim3(count), dim3(BE_SCAN_THREADS), 0, st, A, h->d_becnt.as<int>(), h->d_blkstart.as<int>());
        SNK_LAUNCH_CHECK();
        if (tot.max_be_waves > 0)
        {
            const size_t be_lds = (size_t)((tot.max_nfc + 63) / 64) * 64 * 12;  // ballots (8 B) + bases (4 B) per camera
            hipLaunchKernelGGL(block_entries_fill, dim3(tot.max_be_waves, count), dim3(64), be_lds, st, A, h->d_becnt.as<int>(), h->d_blkent.as<int4>());
            SNK_LAUNCH_CHECK();
        }
    }
    t_rs = std::chrono::steady_clock::now();
    return SNK_OK;
}

// SNK_BA_CHECK_LISTS=1: the host builder's lists (never uploaded here) against what the kernels wrote
int HandOver::check_lists()
{
    if (!sw.check_lists) return SNK_OK;
    hipStream_t st = h->stream;
    SNK_HIP_CHECK(hipStreamSynchronize(st));
    std::vector<CamObs> d_rec(L.camitems.size());
    if (!d_rec.empty()) SNK_HIP_CHECK(hipMemcpy(d_rec.data(), h->d_csobs.p, d_rec.size() * sizeof(CamObs), hipMemcpyDeviceToHost));
    for (int b = 0; b < count; ++b)
    {
        const snk_ba_problem& P = problems[b];
        const Prob& pr          = L.probs[(size_t)b];
        const int n_items       = L.camstart[(size_t)pr.camstart_off + (size_t)pr.nfc];
        for (int k = 0; k < n_items; ++k)
        {
            const int s = L.camitems[(size_t)pr.citem_off + (size_t)k], o = L.oorig[(size_t)pr.obs_off + (size_t)s] - pr.orig_off;
            const CamObs& r = d_rec[(size_t)pr.citem_off + (size_t)k];
            const bool same = r.u == P.obs_uv[o][0] && r.v == P.obs_uv[o][1] && r.depth == P.obs_depth[o] && r.weight == P.obs_weight[o] &&
                              (r.ptw & 0x7FFFFFFF) == P.obs_pt[o] && r.orig == pr.orig_off + o &&
                              (r.ptw < 0 ? 1 : 0) == (P.pt_const[P.obs_pt[o]] ? 0 : 1);
            SNK_REQUIRE(same, "SNK_BA_CHECK_LISTS: a device-gathered camera record differs from the caller's observation");
        }
    }
    {
        // the work items' observation records (gather_set_records) against the caller's arrays
        std::vector<SetObs> d_sr((size_t)tot.n_setrec);
        if (!d_sr.empty()) SNK_HIP_CHECK(hipMemcpy(d_sr.data(), h->d_setobs.p, d_sr.size() * sizeof(SetObs), hipMemcpyDeviceToHost));
        for (int b = 0; b < count; ++b)
        {
            const snk_ba_problem& P = problems[b];
            const Prob& pr          = L.probs[(size_t)b];
            for (int it = 0; it < pr.n_set; ++it)
            {
                const SetItem& si = L.setitems[(size_t)pr.set_off + (size_t)it];
                for (int q = 0; q < si.n_pts; ++q)
                    for (int a = 0; a < si.run; ++a)
                    {
                        const int2 pp = L.setpts[(size_t)si.pts_off + (size_t)q];
                        const int s = pp.y + a, o = L.oorig[(size_t)pr.obs_off + (size_t)s] - pr.orig_off;
                        const SetObs& r = d_sr[(size_t)si.rec_off + (size_t)q * si.run + (size_t)a];
                        const bool same = r.u == P.obs_uv[o][0] && r.v == P.obs_uv[o][1] && r.depth == P.obs_depth[o] &&
                                          r.weight == P.obs_weight[o] && r.orig == pr.orig_off + o &&
                                          r.pk == set_pack(P.obs_img[o], L.ocam[(size_t)pr.obs_off + (size_t)s], P.pt_const[pp.x] ? 0 : 1) &&
                                          P.obs_pt[o] == pp.x;
                        SNK_REQUIRE(same, "SNK_BA_CHECK_LISTS: a device-gathered work-item record differs from the caller's observation");
                    }
            }
        }
    }
    if (tot.dev_entries)
    {
        std::vector<int> d_bs((size_t)tot.blkstart_total);
        std::vector<int4> d_ent((size_t)tot.ent_total);
        SNK_HIP_CHECK(hipMemcpy(d_bs.data(), h->d_blkstart.p, d_bs.size() * sizeof(int), hipMemcpyDeviceToHost));
        if (!d_ent.empty()) SNK_HIP_CHECK(hipMemcpy(d_ent.data(), h->d_blkent.p, d_ent.size() * sizeof(int4), hipMemcpyDeviceToHost));
        pvec<int> h_bs;
        pvec<int4> h_ent;
        for (int b = 0; b < count; ++b)
        {
            const Prob& pr  = L.probs[(size_t)b];
            const size_t nb = (size_t)pr.nfc * pr.nfc, bs_at = h_bs.size(), ent_at = h_ent.size();
            host_block_entries(b, h_bs, h_ent);
            for (size_t k = 0; k <= nb; ++k)
                SNK_REQUIRE(d_bs[(size_t)pr.blkstart_off + k] == h_bs[bs_at + k], "SNK_BA_CHECK_LISTS: device-built block starts differ from the host builder's");
            SNK_REQUIRE((long long)h_bs[bs_at + nb] <= ent_bound[(size_t)b], "SNK_BA_CHECK_LISTS: block entries exceed their bound");
            for (int k = 0; k < h_bs[bs_at + nb]; ++k)
            {
                const int4 d = d_ent[(size_t)pr.ent_off + (size_t)k], w = h_ent[ent_at + (size_t)k];
                SNK_REQUIRE(d.x == w.x && d.y == w.y && d.z == w.z, "SNK_BA_CHECK_LISTS: device-built block entries differ from the host builder's");
            }
        }
    }
    return SNK_OK;
}

// the stages behind the fill pass (host arrays) or the device stage (device rows)
int HandOver::later_stages()
{
    SNK_TRY(build_problem_lists());
    SNK_TRY(merge_decide());
    SNK_TRY(merge_copy());
    SNK_TRY(publish_totals());
    SNK_TRY(plan_block_entries());
    SNK_TRY(upload_rest());
    SNK_TRY(reserve_work());
    SNK_TRY(zero_and_launch());
    SNK_TRY(check_lists());
    return report();
}

int HandOver::host_hand_over()
{
    SNK_TRY(reserve_lists());
    SNK_TRY(size_pass());
    SNK_TRY(place_problems());
    SNK_TRY(fill_and_send());
    return later_stages();
}

// SNK_BA_PROFILE_CREATE=1: host-side cost of the hand-over, in microseconds
int HandOver::report()
{
    if (!sw.profile) return SNK_OK;
    hipStream_t st = h->stream;
    SNK_HIP_CHECK(hipStreamSynchronize(st));
    const auto t_end = std::chrono::steady_clock::now();
    auto us = [](auto a, auto b) { return (long long)std::chrono::duration_cast<std::chrono::microseconds>(b - a).count(); };
    fprintf(stderr, "[snk_ba_set_problems] lists %lld us, uploads %lld us, reserve+memset %lld us, sync %lld us\n", us(t_begin, t_lists),
            us(t_lists, t_up), us(t_up, t_rs), us(t_rs, t_end));
    fprintf(stderr, "[snk_ba_set_problems] lists in us: values+sort %lld, observation arrays %lld, wave items %lld, camera lists %lld, "
                    "block entries %lld, point sets %lld (grouping %lld, work items %lld, block lists %lld), constraints %lld, rest %lld\n",
            sec.us(SEC_VALUES_SORT), sec.us(SEC_OBS_ARRAYS), sec.us(SEC_WAVE_ITEMS), sec.us(SEC_CAMERA_LISTS), sec.us(SEC_BLOCK_ENTRIES),
            sec.us(SEC_BLOCK_LISTS) + sec.us(SEC_GROUPING) + sec.us(SEC_WORK_ITEMS), sec.us(SEC_GROUPING), sec.us(SEC_WORK_ITEMS), sec.us(SEC_BLOCK_LISTS),
            sec.us(SEC_CONSTRAINTS), sec.us(SEC_REST));
    fprintf(stderr, "[snk_ba_set_problems] input %s: device stage %lld us, readback %lld us, over the bus %lld bytes up, %lld bytes down\n",
            dev ? "device rows" : "host arrays", dev_stage_us, readback_us, bytes_up, bytes_down);
    return SNK_OK;
}
#undef SNK_TRY
}  // namespace

namespace ba
{
int ba_copy_table(const CopyTab& tab, int gx, hipStream_t stream)
{
    hipLaunchKernelGGL(copy_table_kernel, dim3(gx, tab.n), dim3(256), 0, stream, tab);
    SNK_LAUNCH_CHECK();
    return SNK_OK;
}
}  // namespace ba
}  // namespace snk

using namespace snk;

extern "C" {

int snk_ba_set_problems(snk_ba* h, const snk_ba_problem* problems, int count)
{
    SNK_REQUIRE(h != nullptr, "ba is NULL");
    // A call that fails leaves NO problem set, whichever of its many exits it takes (snake_hip.h): past the checks the early upload of a
    // batch writes into the device arrays of the previous set and the host lists are cleared, so solve / get_state / residuals must then
    // refuse ("no problem set") instead of running the old tables over half-replaced arrays -- and a refused argument or a failed HIP
    // call ends the previous set as well, so that the caller never has to tell the exits apart.
    h->count       = 0;
    h->state_fresh = false;
    struct NoSetOnFailure
    {
        snk_ba* h;
        bool ok = false;
        ~NoSetOnFailure()
        {
            if (!ok) h->count = 0, h->state_fresh = false;
        }
    } no_set_on_failure{h};
    HandOver ho(h, problems, count);
    int rc;
    if ((rc = ho.check_arguments()) != SNK_OK) return rc;
    h->implicit = ho.imp;
    SNK_HIP_CHECK(hipSetDevice(h->device));
    SNK_HIP_CHECK(hipStreamSynchronize(h->stream));
    h->drop_graphs();
    if ((rc = ho.host_hand_over()) != SNK_OK) return rc;
    no_set_on_failure.ok = true;
    return SNK_OK;
}

int snk_ba_set_problems_dev(snk_ba* h, int n_q, const snk_scene_out* out_dev, const double K[4], double bf)
{
    SNK_REQUIRE(h != nullptr, "ba is NULL");
    h->count       = 0;  // as snk_ba_set_problems: whatever happens below, a failure leaves no problem set
    h->state_fresh = false;
    struct NoSetOnFailure
    {
        snk_ba* h;
        bool ok = false;
        ~NoSetOnFailure()
        {
            if (!ok) h->count = 0, h->state_fresh = false;
        }
    } no_set_on_failure{h};
    // everything is checked before a kernel reads a row
    SNK_REQUIRE(out_dev != nullptr && K != nullptr, "out_dev / K is NULL");
    SNK_REQUIRE(n_q >= 1 && n_q <= 65535, "count must be 1..65535");
    const bool imp = h->explicit_schur == 0;
    SNK_REQUIRE(!imp || n_q == 1, "the implicit Schur form takes one problem (snk_ba_set_explicit_schur)");
    const snk_scene_out& rows = *out_dev;
    SNK_REQUIRE(rows.win_cap >= 1 && rows.win_cap <= SNK_SCENE_MAX_WINDOW && rows.pt_cap >= 1 && rows.pt_cap <= SNK_LMAP_MAX_PTS && rows.img_cap >= 1 &&
                    rows.img_cap <= SNK_SCENE_MAX_IMG && rows.obs_cap >= 1 && rows.obs_cap <= SNK_SCENE_MAX_OBS,
                "a cap of the rows is outside its range");
    SNK_REQUIRE(rows.result && rows.pose && rows.img_const && rows.pt && rows.pt_const && rows.obs_img && rows.obs_pt && rows.obs_uv && rows.obs_depth &&
                    rows.obs_weight,
                "NULL row arrays");
    SNK_HIP_CHECK(hipSetDevice(h->device));
    SNK_HIP_CHECK(hipStreamSynchronize(h->stream));  // the rows are complete on this stream (or the caller has synchronised their producer)
    std::vector<snk_scene_result> rec((size_t)n_q);
    int rc;
    if ((rc = copy_sync(rec.data(), rows.result, (size_t)n_q * sizeof(snk_scene_result), hipMemcpyDeviceToHost, h->stream)) != SNK_OK) return rc;
    bool kernels_take = true;
    for (snk_scene_result& r : rec)
    {
        SNK_REQUIRE(r.n_img >= 0 && r.n_pt >= 0 && r.n_obs >= 0 && r.n_rpc >= 0, "negative problem size");
        SNK_REQUIRE(r.n_img <= rows.img_cap && r.n_pt <= rows.pt_cap && r.n_obs <= rows.obs_cap && r.n_rpc <= rows.win_cap, "a record's count exceeds the row's cap");
        if (r.status != SNK_SCENE_OK) r.n_img = r.n_pt = r.n_obs = r.n_rpc = 0;  // an empty problem in its slot; the row is not read
        if (rows.rpc == nullptr) r.n_rpc = 0;
        kernels_take = kernels_take && ho_kernels_take(r.n_pt);
    }
    h->implicit = imp;
    h->drop_graphs();
    const long long rec_bytes = (long long)n_q * (long long)sizeof(snk_scene_result);
    RowsOnHost host_rows;
    if (kernels_take)
    {
        std::vector<snk_ba_problem> shadow((size_t)n_q, snk_ba_problem{});
        for (int b = 0; b < n_q; ++b)
        {
            snk_ba_problem& P = shadow[(size_t)b];
            P.n_img = rec[(size_t)b].n_img, P.n_pt = rec[(size_t)b].n_pt, P.n_obs = rec[(size_t)b].n_obs, P.n_rpc = rec[(size_t)b].n_rpc;
            for (int k = 0; k < 4; ++k) P.K[k] = K[k];
            P.bf = bf;
        }
        HandOver ho(h, shadow.data(), n_q, true);
        ho.bytes_down = rec_bytes;
        if ((rc = ho.reserve_lists()) != SNK_OK) return rc;
        if ((rc = ho.dev_stage(rows, shadow.data())) != SNK_OK) return rc;
        if (!ho.dev_long_run)
        {
            if (ho.sw.check_lists && (rc = ho.dev_check(rows, host_rows, rec)) != SNK_OK) return rc;
            if ((rc = ho.later_stages()) != SNK_OK) return rc;
            no_set_on_failure.ok = true;
            return SNK_OK;
        }
    }
    // a batch the kernels do not take (handover_core.hpp): the rows come down and go through the host builder
    if ((rc = host_rows.fetch(rows, rec, K, bf, h->stream)) != SNK_OK) return rc;
    HandOver ho(h, host_rows.problems.data(), n_q);
    ho.bytes_down = rec_bytes + host_rows.bytes;
    if ((rc = ho.host_hand_over()) != SNK_OK) return rc;
    no_set_on_failure.ok = true;
    return SNK_OK;
}

int snk_ba_set_problem(snk_ba* h, const snk_ba_problem* problem)
{
    return snk_ba_set_problems(h, problem, 1);
}
}
