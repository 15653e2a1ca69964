// Batched registration RANSAC for gfx950 -- replaces `solver.solve(its, compute_scale)` of LoopDetector::solve and, in the
// device-resident form, the loop that fills the solver and the corrected source pose of LoopDetector::ComputeSim3 (reference
// Snake/LoopClosing/LoopDetector.cpp:148-206, 250-278).  Semantics "snk-sim3 v1" (DESIGN.md section 3e); the per-triplet solver and
// the per-pair test are sim3_core.hpp, the sampler is the one of p3p_core.hpp.
//
// Mapping to the hardware: the one of p3p.hip.  sim3_ransac_kernel: ONE workgroup of four wavefronts per problem, one launch per
// batch.  The problem's pairs are staged once as ten planes of doubles (x y z of either point, u v of either keypoint: 80 bytes a
// pair): the first SIM3_LDS_PAIRS = 1024 pairs in LDS (80 KB), the rest -- a problem may have 2048 -- in a slab of global memory
// that only this workgroup touches and that stays in L2.  In the device-resident form the pairs come straight from the filter's
// output (ballot + mbcnt compaction of the entries whose two features carry a point, `pose * wp` on the way).  Hypotheses go 256 at
// a time: every LANE solves its own triplet and keeps the transform in registers, then the WAVEFRONT scores the transforms one
// after the other: the transform comes out of the owning lane with v_readlane, all 64 lanes test pairs, ballot + popcount adds up.
// The best (count, smaller k) is one max over a 64-bit key -- across lanes by shuffles, across the four wavefronts through LDS,
// across the groups of 256 by a running value: no atomics, the result does not depend on any order.  The winner's transform goes to
// LDS and the same workgroup writes the mask / match12 and the corrected pose.  f64 throughout, no scratch
// (tests/test_sim3_resources.py).
#include <cstddef>

#include "matcher_handle.hpp"
#include "sim3_core.hpp"

namespace snk
{
namespace
{
using u8  = unsigned char;
using u32 = unsigned int;
using u64 = unsigned long long;

constexpr int SIM3_MAX_PAIRS      = 2048;  // per problem
constexpr int SIM3_LDS_PAIRS      = 1024;  // of them in LDS: 80 bytes a pair
constexpr int SIM3_MAX_ITERATIONS = 1 << 20;

struct Sim3Meta  // host form: where a problem's pairs are, its iteration count, camera and start values
{
    int off, n, its, pad;
    Sim3Camera K;
    double T[7], scale;
};

struct Sim3Result
{
    double T[7], scale;
    int inliers, best_iteration;
};

struct Sim3Debug  // snk_sim3_debug_hypotheses: per hypothesis of problem 0 (all NULL otherwise)
{
    int* triplet;   // [iterations][3]
    int* valid;     // [iterations]
    int* counts;    // [iterations]
    double* T;      // [iterations][7]
    double* scale;  // [iterations]
};

struct Sim3Pairs  // device-resident form
{
    const snk_kp64 *kps1, *kps2;
    const int *pairs, *n_pairs;
    const u8 *pts1, *pts2;
    const int *frame_pt1, *frame_pt2, *n_pts1, *n_pts2;
    const double *poses1, *poses2;
    const int* its_table;  // [pairs_cap + 1], NULL with a forced count
    double *T, *scale, *corrected;
    int *inliers, *match12;
    int cap1, cap2, pairs_cap, pts_cap, pts_stride;
    Sim3Camera K;
};

__device__ __forceinline__ int lane_prefix(u64 mask)
{
    return __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0));
}

// pair i of the workgroup's problem: plane j of the LDS block for i < lds_cap, record i - lds_cap of the slab beyond
struct PairStore
{
    double* lds;
    double* slab;
    int lds_cap;
    __device__ __forceinline__ void put(int i, const double (&v)[10]) const
    {
        if (i < lds_cap)
        {
#pragma unroll
            for (int j = 0; j < 10; ++j) lds[j * lds_cap + i] = v[j];
        }
        else
        {
#pragma unroll
            for (int j = 0; j < 10; ++j) slab[(size_t)(i - lds_cap) * 10 + j] = v[j];
        }
    }
    __device__ __forceinline__ void get(int i, double (&v)[10]) const
    {
        if (i < lds_cap)
        {
#pragma unroll
            for (int j = 0; j < 10; ++j) v[j] = lds[j * lds_cap + i];
        }
        else
        {
#pragma unroll
            for (int j = 0; j < 10; ++j) v[j] = slab[(size_t)(i - lds_cap) * 10 + j];
        }
    }
};

__device__ __forceinline__ bool pair_inlier(const double (&sR)[9], const double (&R)[9], const double (&t)[3], const double (&v)[10],
                                            const Sim3Camera& K, double threshold)
{
    const double P1[3] = {v[0], v[1], v[2]}, P2[3] = {v[3], v[4], v[5]};
    return sim3_inlier(sR, R, t, P1, P2, v[6], v[7], v[8], v[9], K, threshold);
}

// dynamic LDS: ten planes of lds_cap doubles, then (device-resident form) idx_cap feature indices f1 and idx_cap point indices of
// keyframe 2.  slab: slab_cap pairs of ten doubles per problem, read and written by the problem's own workgroup only.
template <bool DEV>
__global__ __launch_bounds__(256) void sim3_ransac_kernel(const Sim3Meta* __restrict__ meta, const double* __restrict__ in_p1,
                                                          const double* __restrict__ in_p2, const double* __restrict__ in_ip1,
                                                          const double* __restrict__ in_ip2, Sim3Pairs F, int iterations, int compute_scale,
                                                          double threshold, u64 seed, int lds_cap, int idx_cap, double* slab, int slab_cap,
                                                          u8* __restrict__ mask_out, Sim3Result* __restrict__ result, Sim3Debug dbg)
{
    extern __shared__ double s_dyn[];
    __shared__ int s_wave[4];
    __shared__ u64 s_key[4];
    __shared__ double s_hyp[17];  // the winner: q, R, t, s
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PairStore S{s_dyn, slab + (size_t)b * (size_t)slab_cap * 10, lds_cap};
    int* sf1  = reinterpret_cast<int*>(s_dyn + (size_t)10 * lds_cap);
    int* spt2 = sf1 + idx_cap;

    // ---- stage the pairs ----
    int n = 0;
    Sim3Camera K;
    if (DEV)
    {
        K               = F.K;
        const int ne    = min(max(F.n_pairs[b], 0), F.pairs_cap);
        const int np1   = min(max(F.n_pts1[b], 0), F.pts_cap), np2 = min(max(F.n_pts2[b], 0), F.pts_cap);
        const int* pr   = F.pairs + (size_t)b * F.pairs_cap * 2;
        const size_t b1 = (size_t)b * F.cap1, b2 = (size_t)b * F.cap2;
        for (int f = tid; f < F.cap1; f += 256) F.match12[b1 + f] = -1;
        for (int e0 = 0; e0 < ne; e0 += 256)
        {
            const int e = e0 + tid;
            int f1 = -1, f2 = -1, v1 = -1, v2 = -1;
            if (e < ne)
            {
                f1 = pr[2 * e];
                f2 = pr[2 * e + 1];
                if (f1 >= 0 && f1 < F.cap1 && f2 >= 0 && f2 < F.cap2)
                {
                    v1 = F.frame_pt1[b1 + f1];
                    v2 = F.frame_pt2[b2 + f2];
                }
            }
            const bool has = v1 >= 0 && v1 < np1 && v2 >= 0 && v2 < np2;  // LoopORBMatcher.cpp:110-116
            const u64 m    = __ballot(has);
            if (lane == 0) s_wave[wave] = __popcll(m);
            __syncthreads();
            int before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w)
            {
                before += w < wave ? s_wave[w] : 0;
                total += s_wave[w];
            }
            if (has)
            {
                const int k = n + before + lane_prefix(m);  // < entries visited so far <= pairs_cap = idx_cap <= lds_cap + slab_cap
                double P1[3], P2[3];
                sim3_view_point(F.poses1 + (size_t)b * 7, reinterpret_cast<const double*>(F.pts1 + ((size_t)b * F.pts_cap + v1) * (size_t)F.pts_stride), P1);
                sim3_view_point(F.poses2 + (size_t)b * 7, reinterpret_cast<const double*>(F.pts2 + ((size_t)b * F.pts_cap + v2) * (size_t)F.pts_stride), P2);
                const snk_kp64 k1 = F.kps1[b1 + f1], k2 = F.kps2[b2 + f2];
                const double v[10] = {P1[0], P1[1], P1[2], P2[0], P2[1], P2[2], k1.x, k1.y, k2.x, k2.y};
                S.put(k, v);
                sf1[k]  = f1;
                spt2[k] = v2;
            }
            n += total;
            __syncthreads();
        }
        iterations = F.its_table != nullptr ? F.its_table[n] : iterations;  // n <= pairs_cap: the table has pairs_cap + 1 entries
    }
    else
    {
        K             = meta[b].K;
        n             = min(meta[b].n, lds_cap + slab_cap);
        iterations    = meta[b].its;
        const int off = meta[b].off;
        for (int i = tid; i < n; i += 256)
        {
            const double *a = in_p1 + (size_t)(off + i) * 3, *c = in_p2 + (size_t)(off + i) * 3;
            const double *p = in_ip1 + (size_t)(off + i) * 2, *q = in_ip2 + (size_t)(off + i) * 2;
            const double v[10] = {a[0], a[1], a[2], c[0], c[1], c[2], p[0], p[1], q[0], q[1]};
            S.put(i, v);
        }
    }
    __syncthreads();

    // ---- hypotheses, 256 at a time ----
    const u32 key = p3p_problem_key(seed, (u32)b);
    u64 best      = 0;  // (count << 32) | ~k: larger count first, then smaller k; 0 = nothing yet
    if (n >= 3)
    {
        for (int k0 = 0; k0 < iterations; k0 += 256)
        {
            const int k = k0 + tid;
            double q[4] = {0, 0, 0, 0}, R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, t[3] = {0, 0, 0}, sR[9], s = 0.0;
            int tri[3]  = {0, 0, 0};
            int valid   = 0;
            if (k < iterations)
            {
                p3p_triplet(key, (u32)k, (u32)n, tri);
                double A[3][3], B[3][3];
#pragma unroll
                for (int j = 0; j < 3; ++j)
                {
                    double v[10];
                    S.get(tri[j], v);
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                    {
                        A[j][c] = v[c];
                        B[j][c] = v[3 + c];
                    }
                }
                valid = sim3_solve(A, B, compute_scale != 0, q, R, t, s) ? 1 : 0;
            }
#pragma unroll
            for (int j = 0; j < 9; ++j) sR[j] = s * R[j];
            int cnt       = 0;
            const u64 any = __ballot(valid != 0);
            for (int h = 0; h < 64; ++h)
            {
                if (!((any >> h) & 1)) continue;
                double hR[9], hsR[9], ht[3];
#pragma unroll
                for (int j = 0; j < 9; ++j)
                {
                    hR[j]  = readlane64(R[j], h);
                    hsR[j] = readlane64(sR[j], h);
                }
#pragma unroll
                for (int j = 0; j < 3; ++j) ht[j] = readlane64(t[j], h);
                int c = 0;
                for (int i0 = 0; i0 < n; i0 += 64)
                {
                    const int i = i0 + lane;
                    bool inl    = false;
                    if (i < n)
                    {
                        double v[10];
                        S.get(i, v);
                        inl = pair_inlier(hsR, hR, ht, v, K, threshold);
                    }
                    c += __popcll(__ballot(inl));
                }
                if (lane == h) cnt = c;
            }
            const u64 mine = (valid && cnt > 0) ? (((u64)(u32)cnt << 32) | (u64)(0xffffffffu - (u32)k)) : 0;
            if (dbg.triplet != nullptr && b == 0 && k < iterations)
            {
#pragma unroll
                for (int j = 0; j < 3; ++j) dbg.triplet[(size_t)k * 3 + j] = tri[j];
                dbg.valid[k]  = valid;
                dbg.counts[k] = valid ? cnt : 0;
                dbg.scale[k]  = valid ? s : 0.0;
#pragma unroll
                for (int j = 0; j < 7; ++j) dbg.T[(size_t)k * 7 + j] = valid ? (j < 4 ? q[j] : t[j - 4]) : 0.0;
            }
            u64 top = mine;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1)
            {
                const u64 o = __shfl_xor(top, d, 64);
                top         = o > top ? o : top;
            }
            if (lane == 0) s_key[wave] = top;
            __syncthreads();
            u64 group = s_key[0];
#pragma unroll
            for (int w = 1; w < 4; ++w) group = s_key[w] > group ? s_key[w] : group;
            if (group > best)
            {
                best = group;
                if (mine == group)  // exactly one lane: the key holds k
                {
#pragma unroll
                    for (int j = 0; j < 4; ++j) s_hyp[j] = q[j];
#pragma unroll
                    for (int j = 0; j < 9; ++j) s_hyp[4 + j] = R[j];
#pragma unroll
                    for (int j = 0; j < 3; ++j) s_hyp[13 + j] = t[j];
                    s_hyp[16] = s;
                }
            }
            __syncthreads();
        }
    }
    const bool found = best != 0;

    // ---- the winner's mask and count ----
    double q[4] = {0, 0, 0, 1}, R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, sR[9], t[3] = {0, 0, 0}, s = 1.0;
    if (found)
    {
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = s_hyp[j];
#pragma unroll
        for (int j = 0; j < 9; ++j) R[j] = s_hyp[4 + j];
#pragma unroll
        for (int j = 0; j < 3; ++j) t[j] = s_hyp[13 + j];
        s = s_hyp[16];
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) sR[j] = s * R[j];
    const int off = DEV ? 0 : meta[b].off;
    int run       = 0;
    for (int i0 = 0; i0 < n; i0 += 256)
    {
        const int i = i0 + tid;
        bool inl    = false;
        if (found && i < n)
        {
            double v[10];
            S.get(i, v);
            inl = pair_inlier(sR, R, t, v, K, threshold);
        }
        const u64 m = __ballot(inl);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 4; ++w) run += s_wave[w];
        if (DEV)
        {
            if (inl) F.match12[(size_t)b * F.cap1 + sf1[i]] = spt2[i];  // sf1[i] was checked against cap1 when the pair was staged
        }
        else if (i < n)
            mask_out[off + i] = inl ? 1 : 0;
        __syncthreads();
    }
    if (tid == 0)
    {
        if (DEV)
        {
            F.inliers[b] = run;
            if (found)
            {
#pragma unroll
                for (int j = 0; j < 7; ++j) F.T[(size_t)b * 7 + j] = j < 4 ? q[j] : t[j - 4];
                F.scale[b] = s;
                double cp[7];
                sim3_corrected_pose(R, t, s, F.poses2 + (size_t)b * 7, cp);
#pragma unroll
                for (int j = 0; j < 7; ++j) F.corrected[(size_t)b * 7 + j] = cp[j];
            }
        }
        else
        {
            Sim3Result r;
#pragma unroll
            for (int j = 0; j < 7; ++j) r.T[j] = found ? (j < 4 ? q[j] : t[j - 4]) : meta[b].T[j];
            r.scale          = found ? s : meta[b].scale;
            r.inliers        = run;
            r.best_iteration = found ? (int)(0xffffffffu - (u32)best) : -1;
            result[b]        = r;
        }
    }
}

size_t lds_bytes(int lds_pairs, int idx_pairs)
{
    return (size_t)lds_pairs * 80 + (size_t)idx_pairs * 8;
}

int check_params(const snk_sim3_params* p)
{
    SNK_REQUIRE(p != nullptr, "params is NULL");
    SNK_REQUIRE(p->iterations >= 0 && p->iterations <= SIM3_MAX_ITERATIONS, "iterations outside [0, 2^20]");
    SNK_REQUIRE(p->threshold > 0.0, "threshold must be positive");
    if (p->iterations == 0)
    {
        SNK_REQUIRE(p->probability > 0.0 && p->probability < 1.0, "probability must lie inside (0, 1)");
        SNK_REQUIRE(p->min_inliers >= 1, "min_inliers must be at least 1");
        SNK_REQUIRE(p->max_iterations >= 1 && p->max_iterations <= SIM3_MAX_ITERATIONS, "max_iterations outside [1, 2^20]");
    }
    return SNK_OK;
}

int problem_iterations(const snk_sim3_params* p, int n)
{
    return p->iterations > 0 ? p->iterations : sim3_ransac_iterations(n, p->probability, p->min_inliers, p->max_iterations);
}

int ransac_host(snk_matcher* m, const snk_sim3_params* params, snk_sim3_problem* problems, int n_problems, Sim3Debug dbg)
{
    size_t total = 0;
    int n_max    = 1;
    for (int i = 0; i < n_problems; ++i)
    {
        const snk_sim3_problem& P = problems[i];
        SNK_REQUIRE(P.n >= 0 && P.n <= SIM3_MAX_PAIRS, "pairs per problem outside [0, 2048]");
        SNK_REQUIRE(P.n == 0 || (P.points1 && P.points2 && P.ips1 && P.ips2 && P.inlier_mask), "NULL pair / result array with n > 0");
        total += (size_t)P.n;
        n_max = P.n > n_max ? P.n : n_max;
    }
    SNK_REQUIRE(total < (size_t)1 << 28, "too many pairs");
    SNK_HIP_CHECK(hipSetDevice(m->device));
    const int lds_cap = n_max < SIM3_LDS_PAIRS ? n_max : SIM3_LDS_PAIRS, slab_cap = n_max - lds_cap;
    const size_t np   = (size_t)n_problems;
    // up: Sim3Meta[np] | points1 | points2 | ips1 | ips2 (the problems' rows one after the other)      back: Sim3Result[np] | mask[total]
    Block in, out;
    const int i_meta = in.add(nullptr, np * sizeof(Sim3Meta)), i_p1 = in.add(nullptr, total * 24), i_p2 = in.add(nullptr, total * 24),
              i_i1 = in.add(nullptr, total * 16), i_i2 = in.add(nullptr, total * 16);
    const int r_res = out.add(nullptr, np * sizeof(Sim3Result)), r_mask = out.add(nullptr, total);
    int rc;
    if ((rc = stage_reserve(m, in.bytes, out.end(), 64)) != SNK_OK) return rc;
    if ((rc = m->aux2.reserve(np * (size_t)slab_cap * 80 + 64)) != SNK_OK) return rc;
    char* stage    = m->h_in.as<char>();
    Sim3Meta* meta = in.at<Sim3Meta>(stage, i_meta);
    size_t off     = 0;
    for (int i = 0; i < n_problems; ++i)
    {
        const snk_sim3_problem& P = problems[i];
        meta[i].off               = (int)off;
        meta[i].n                 = P.n;
        meta[i].its               = problem_iterations(params, P.n);
        meta[i].pad               = 0;
        meta[i].K                 = Sim3Camera{P.cam.fx, P.cam.fy, P.cam.cx, P.cam.cy};
        memcpy(meta[i].T, P.T, 56);
        meta[i].scale = P.scale;
        if (P.n > 0)
        {
            memcpy(in.at<char>(stage, i_p1) + off * 24, P.points1, (size_t)P.n * 24);
            memcpy(in.at<char>(stage, i_p2) + off * 24, P.points2, (size_t)P.n * 24);
            memcpy(in.at<char>(stage, i_i1) + off * 16, P.ips1, (size_t)P.n * 16);
            memcpy(in.at<char>(stage, i_i2) + off * 16, P.ips2, (size_t)P.n * 16);
        }
        off += (size_t)P.n;
    }
    if ((rc = stage_upload(m, in)) != SNK_OK) return rc;
    char* d = m->q.as<char>();
    char* o = m->out.as<char>();
    if ((rc = set_max_lds_once(reinterpret_cast<const void*>(sim3_ransac_kernel<false>), (int)lds_bytes(SIM3_LDS_PAIRS, 0))) != SNK_OK) return rc;
    Sim3Pairs F{};
    hipLaunchKernelGGL(sim3_ransac_kernel<false>, dim3(n_problems), dim3(256), lds_bytes(lds_cap, 0), m->stream, in.at<const Sim3Meta>(d, i_meta),
                       in.at<const double>(d, i_p1), in.at<const double>(d, i_p2), in.at<const double>(d, i_i1), in.at<const double>(d, i_i2), F, 0,
                       params->compute_scale, params->threshold, (u64)params->seed, lds_cap, 0, m->aux2.as<double>(), slab_cap,
                       out.at<u8>(o, r_mask), out.at<Sim3Result>(o, r_res), dbg);
    SNK_LAUNCH_CHECK();
    if ((rc = stage_download(m, 0, out.end())) != SNK_OK) return rc;
    char* back            = m->h_res.as<char>();
    const Sim3Result* res = out.at<const Sim3Result>(back, r_res);
    off                   = 0;
    for (int i = 0; i < n_problems; ++i)
    {
        snk_sim3_problem& P = problems[i];
        if (res[i].inliers < 0 || res[i].inliers > P.n)
        {
            set_error("sim3: device returned %d inliers for %d pairs", res[i].inliers, P.n);
            return SNK_ERR_HIP;
        }
        memcpy(P.T, res[i].T, 56);
        P.scale          = res[i].scale;
        P.inliers        = res[i].inliers;
        P.best_iteration = res[i].best_iteration;
        if (P.n > 0) memcpy(P.inlier_mask, out.at<char>(back, r_mask) + off, (size_t)P.n);
        off += (size_t)P.n;
    }
    return SNK_OK;
}

// its[n], n = 0 .. cap, on the device under the parameters of `p`: refilled only when they or cap change
int iteration_table(snk_matcher* m, const snk_sim3_params* p, int cap)
{
    if (m->sim3_its_cap == cap && m->sim3_its_probability == p->probability && m->sim3_its_min == p->min_inliers &&
        m->sim3_its_max == p->max_iterations)
        return SNK_OK;
    const size_t bytes = (size_t)(cap + 1) * sizeof(int);
    int rc;
    SNK_HIP_CHECK(hipStreamSynchronize(m->stream));  // an earlier upload may still read the pinned copy, an earlier launch the table
    m->sim3_its_cap = -1;
    if ((rc = m->sim3_its_host.reserve(bytes)) != SNK_OK) return rc;
    if ((rc = m->sim3_its.reserve(bytes)) != SNK_OK) return rc;
    int* h = m->sim3_its_host.as<int>();
    for (int n = 0; n <= cap; ++n) h[n] = sim3_ransac_iterations(n, p->probability, p->min_inliers, p->max_iterations);
    SNK_HIP_CHECK(hipMemcpyAsync(m->sim3_its.p, h, bytes, hipMemcpyHostToDevice, m->stream));
    m->sim3_its_cap         = cap;
    m->sim3_its_probability = p->probability;
    m->sim3_its_min         = p->min_inliers;
    m->sim3_its_max         = p->max_iterations;
    return SNK_OK;
}
}  // namespace
}  // namespace snk

using namespace snk;

extern "C" {
int snk_ransac_iterations(int n, double probability, int min_inliers, int max_iterations)
{
    return sim3_ransac_iterations(n, probability, min_inliers, max_iterations);
}

int snk_sim3_ransac(snk_matcher* m, const snk_sim3_params* params, snk_sim3_problem* problems, int n_problems)
{
    SNK_REQUIRE(m != nullptr, "matcher is NULL");
    int rc;
    if ((rc = check_params(params)) != SNK_OK) return rc;
    SNK_REQUIRE(n_problems >= 0 && (n_problems == 0 || problems != nullptr), "bad problem array");
    if (n_problems == 0) return SNK_OK;
    return ransac_host(m, params, problems, n_problems, Sim3Debug{nullptr, nullptr, nullptr, nullptr, nullptr});
}

int snk_sim3_debug_hypotheses(snk_matcher* m, const snk_sim3_params* params, snk_sim3_problem* problem, int32_t (*triplets)[3],
                              int32_t* valid, double (*T)[7], double* scale, int32_t* counts)
{
    SNK_REQUIRE(m != nullptr && problem != nullptr, "NULL argument");
    int rc;
    if ((rc = check_params(params)) != SNK_OK) return rc;
    SNK_REQUIRE(triplets && valid && T && scale && counts, "NULL output array");
    SNK_REQUIRE(problem->n >= 0 && problem->n <= SIM3_MAX_PAIRS, "pairs per problem outside [0, 2048]");
    const size_t it = (size_t)problem_iterations(params, problem->n);
    SNK_HIP_CHECK(hipSetDevice(m->device));
    // triplet[it][3] | valid[it] | counts[it] | (pad to 8) T[it][7] | scale[it]
    const size_t o_v = it * 12, o_c = o_v + it * 4, o_T = (o_c + it * 4 + 7) & ~(size_t)7, o_s = o_T + it * 56, bytes = o_s + it * 8;
    if ((rc = m->aux.reserve(bytes)) != SNK_OK) return rc;
    char* d = m->aux.as<char>();
    SNK_HIP_CHECK(hipMemsetAsync(d, 0, bytes, m->stream));  // a problem with n < 3 runs no hypothesis
    Sim3Debug dbg{reinterpret_cast<int*>(d), reinterpret_cast<int*>(d + o_v), reinterpret_cast<int*>(d + o_c), reinterpret_cast<double*>(d + o_T),
                  reinterpret_cast<double*>(d + o_s)};
    if ((rc = ransac_host(m, params, problem, 1, dbg)) != SNK_OK) return rc;
    if ((rc = copy_sync(triplets, d, it * 12, hipMemcpyDeviceToHost, m->stream)) != SNK_OK) return rc;
    if ((rc = copy_sync(valid, d + o_v, it * 4, hipMemcpyDeviceToHost, m->stream)) != SNK_OK) return rc;
    if ((rc = copy_sync(counts, d + o_c, it * 4, hipMemcpyDeviceToHost, m->stream)) != SNK_OK) return rc;
    if ((rc = copy_sync(T, d + o_T, it * 56, hipMemcpyDeviceToHost, m->stream)) != SNK_OK) return rc;
    return copy_sync(scale, d + o_s, it * 8, hipMemcpyDeviceToHost, m->stream);
}

int snk_sim3_ransac_pairs_batch_dev(snk_matcher* m, const snk_frames_dev* frames1, const snk_frames_dev* frames2, const snk_camera* cam,
                                    const snk_sim3_params* params, const int32_t* pairs_dev, const int32_t* n_pairs_dev, int pairs_cap,
                                    const void* pts1_dev, const void* pts2_dev, int pts_stride, const int32_t* frame_pt1_dev,
                                    const int32_t* frame_pt2_dev, const int32_t* n_pts1_dev, const int32_t* n_pts2_dev, int pts_cap,
                                    const double* poses1_dev, const double* poses2_dev, double* T_dev, double* scale_dev, int32_t* inliers_dev,
                                    int32_t* match12_dev, double* corrected_pose_dev)
{
    SNK_REQUIRE(m != nullptr && frames1 != nullptr && frames2 != nullptr && cam != nullptr, "NULL argument");
    int rc;
    if ((rc = check_params(params)) != SNK_OK) return rc;
    SNK_REQUIRE(frames1->batch >= 0 && frames1->batch == frames2->batch, "the two frame sets must have one batch size");
    SNK_REQUIRE(frames1->cap >= 1 && frames2->cap >= 1 && frames1->kps != nullptr && frames2->kps != nullptr, "bad frames");
    SNK_REQUIRE(pairs_cap >= 1 && pairs_cap <= SIM3_MAX_PAIRS, "pairs_cap outside [1, 2048]");
    SNK_REQUIRE(pairs_dev && n_pairs_dev && pts1_dev && pts2_dev && frame_pt1_dev && frame_pt2_dev && n_pts1_dev && n_pts2_dev,
                "NULL device input");
    SNK_REQUIRE(poses1_dev && poses2_dev && T_dev && scale_dev && inliers_dev && match12_dev && corrected_pose_dev, "NULL device buffer");
    SNK_REQUIRE(pts_stride >= 24 && pts_stride % 8 == 0 && pts_cap >= 1, "pts_stride must be a multiple of 8, >= 24");
    if (frames1->batch == 0) return SNK_OK;
    SNK_HIP_CHECK(hipSetDevice(m->device));
    if (params->iterations == 0 && (rc = iteration_table(m, params, pairs_cap)) != SNK_OK) return rc;
    const int lds_cap = pairs_cap < SIM3_LDS_PAIRS ? pairs_cap : SIM3_LDS_PAIRS, slab_cap = pairs_cap - lds_cap;
    if ((rc = m->aux2.reserve((size_t)frames1->batch * (size_t)slab_cap * 80 + 64)) != SNK_OK) return rc;
    if ((rc = set_max_lds_once(reinterpret_cast<const void*>(sim3_ransac_kernel<true>), (int)lds_bytes(SIM3_LDS_PAIRS, SIM3_MAX_PAIRS))) != SNK_OK)
        return rc;
    Sim3Pairs F;
    F.kps1 = frames1->kps; F.kps2 = frames2->kps; F.pairs = pairs_dev; F.n_pairs = n_pairs_dev;
    F.pts1 = reinterpret_cast<const u8*>(pts1_dev); F.pts2 = reinterpret_cast<const u8*>(pts2_dev);
    F.frame_pt1 = frame_pt1_dev; F.frame_pt2 = frame_pt2_dev; F.n_pts1 = n_pts1_dev; F.n_pts2 = n_pts2_dev;
    F.poses1 = poses1_dev; F.poses2 = poses2_dev; F.its_table = params->iterations == 0 ? m->sim3_its.as<int>() : nullptr;
    F.T = T_dev; F.scale = scale_dev; F.corrected = corrected_pose_dev; F.inliers = inliers_dev; F.match12 = match12_dev;
    F.cap1 = frames1->cap; F.cap2 = frames2->cap; F.pairs_cap = pairs_cap; F.pts_cap = pts_cap; F.pts_stride = pts_stride;
    F.K = Sim3Camera{cam->fx, cam->fy, cam->cx, cam->cy};
    hipLaunchKernelGGL(sim3_ransac_kernel<true>, dim3(frames1->batch), dim3(256), lds_bytes(lds_cap, pairs_cap), m->stream, nullptr, nullptr,
                       nullptr, nullptr, nullptr, F, params->iterations, params->compute_scale, params->threshold, (u64)params->seed, lds_cap,
                       pairs_cap, m->aux2.as<double>(), slab_cap, nullptr, nullptr, Sim3Debug{nullptr, nullptr, nullptr, nullptr, nullptr});
    SNK_LAUNCH_CHECK();
    return SNK_OK;
}
}
