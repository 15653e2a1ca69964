// Batched P3P-RANSAC for gfx950 -- replaces `P3PRansac pnp2(params); pnp2.solve(wps, ips, pose, inlierMatches, inlierMask)` and the
// loop that keeps the inliers only in Tracking::TrackBruteForce (reference Snake/Tracking/TrackingCoarse.cpp:403-440).  Semantics
// "snk-p3p v1" (DESIGN.md section 3d); the per-triplet solver and the per-point test are p3p_core.hpp.
//
// Mapping to the hardware.  p3p_ransac_kernel: ONE workgroup of four wavefronts per problem, one launch per batch.  The problem's pairs
// are staged once in LDS as five planes of doubles (x y z of the world point, u v of the normalised image point: 40 bytes a pair, 40 KB
// at 1000 pairs) -- in the device-resident form straight from the frame (`frame_pt` walked in feature order, ballot + mbcnt compaction,
// K.unproject2 on the way).  Hypotheses go 256 at a time: every LANE solves its own triplet (the solver diverges, so the 64 triplets of a
// wavefront run side by side instead of one after the other), keeps its <= 4 poses in registers, and then the WAVEFRONT scores them one
// after the other: the pose comes out of the owning lane with v_readlane, all 64 lanes test points, ballot + popcount adds up.  The best
// (count, smaller k, smaller solution) is one max over a 64-bit key -- across lanes by shuffles, across the four wavefronts through
// LDS, across the groups of 256 by a running value: no atomics, the result does not depend on any order.  The winner's pose goes to LDS
// and the same workgroup writes the mask, the ascending list (ballot + mbcnt again) and -- device form -- -1 into frame_pt at every
// feature that is not an inlier.  f64 throughout, no scratch (tests/test_p3p_resources.py).
#include <cstddef>

#include "matcher_handle.hpp"
#include "p3p_core.hpp"

namespace snk
{
namespace
{
using u8  = unsigned char;
using u32 = unsigned int;
using u64 = unsigned long long;

constexpr int P3P_MAX_PAIRS      = 3072;  // per problem: 44 bytes of LDS a pair (five doubles and the feature index)
constexpr int P3P_MAX_ITERATIONS = 1 << 20;

struct P3PMeta  // host form: where a problem's pairs are, its start pose
{
    int off, n;
    double pose[7];
};

struct P3PResult
{
    double pose[7];
    int inliers, best_iteration, best_solution, pad;
};

struct P3PDebug  // snk_p3p_debug_hypotheses: per hypothesis of problem 0 (all NULL otherwise)
{
    int* triplet;   // [iterations][3]
    int* n_sol;     // [iterations]
    double* poses;  // [iterations][4][7]
    int* counts;    // [iterations][4]
};

struct P3PFrames  // device-resident form
{
    const snk_kp64* kps;
    const int* n_feat;
    const u8* pts;
    int* frame_pt;
    const int* n_pts;
    double* poses;
    int* inliers;
    int cap, pts_cap, pts_stride;
    double fx, fy, cx, cy;
};

__device__ __forceinline__ int lane_prefix(u64 mask)
{
    return __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0));
}

// lds_cap pairs fit the dynamic LDS: [x | y | z | u | v] doubles, then the feature index of each pair
template <bool FRAME>
__global__ __launch_bounds__(256) void p3p_ransac_kernel(const P3PMeta* __restrict__ meta, const double* __restrict__ wps,
                                                         const double* __restrict__ nips, P3PFrames F, int iterations, double threshold,
                                                         u64 seed, int lds_cap, u8* __restrict__ mask_out, int* __restrict__ list_out,
                                                         P3PResult* __restrict__ result, P3PDebug dbg)
{
    extern __shared__ double s_dyn[];
    __shared__ int s_wave[4];
    __shared__ u64 s_key[4];
    __shared__ double s_pose[12];
    double* sx = s_dyn;
    double* sy = sx + lds_cap;
    double* sz = sy + lds_cap;
    double* su = sz + lds_cap;
    double* sv = su + lds_cap;
    int* sfeat = reinterpret_cast<int*>(sv + lds_cap);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // ---- stage the pairs ----
    int n = 0;
    if (FRAME)
    {
        const int nf      = min(max(F.n_feat[b], 0), F.cap);
        const int n_p     = min(max(F.n_pts[b], 0), F.pts_cap);
        const size_t base = (size_t)b * F.cap;
        for (int f0 = 0; f0 < nf; f0 += 256)
        {
            const int f    = f0 + tid;
            const int v    = f < nf ? F.frame_pt[base + f] : -1;
            const bool has = v >= 0 && v < n_p;
            if (f < nf && v != -1 && !has) F.frame_pt[base + f] = -1;  // an index outside the point table is no match
            const u64 m = __ballot(has);
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
                const int k      = n + before + lane_prefix(m);  // < features visited so far <= cap <= lds_cap
                const double* pp = reinterpret_cast<const double*>(F.pts + ((size_t)b * F.pts_cap + v) * (size_t)F.pts_stride);
                const snk_kp64 kp = F.kps[base + f];
                sx[k] = pp[0];
                sy[k] = pp[1];
                sz[k] = pp[2];
                su[k] = (kp.x - F.cx) / F.fx;  // K.unproject2, TrackingCoarse.cpp:383-385
                sv[k] = (kp.y - F.cy) / F.fy;
                sfeat[k] = f;
            }
            n += total;
            __syncthreads();
        }
    }
    else
    {
        n             = min(meta[b].n, lds_cap);
        const int off = meta[b].off;
        for (int i = tid; i < n; i += 256)
        {
            const double* w = wps + (size_t)(off + i) * 3;
            const double* q = nips + (size_t)(off + i) * 2;
            sx[i] = w[0];
            sy[i] = w[1];
            sz[i] = w[2];
            su[i] = q[0];
            sv[i] = q[1];
        }
    }
    __syncthreads();

    // ---- hypotheses, 256 at a time ----
    const u32 key = p3p_problem_key(seed, (u32)b);
    u64 best      = 0;  // (count << 32) | ~(4 k + slot): larger count first, then smaller k, then smaller slot; 0 = nothing yet
    if (n >= 4)
    {
        for (int k0 = 0; k0 < iterations; k0 += 256)
        {
            const int k = k0 + tid;
            P3PSolutions S;
            S.valid = 0;
            int tri[3] = {0, 0, 0};
            if (k < iterations)
            {
                p3p_triplet(key, (u32)k, (u32)n, tri);
                double X[3][3], uv[3][2];
#pragma unroll
                for (int j = 0; j < 3; ++j)
                {
                    X[j][0]  = sx[tri[j]];
                    X[j][1]  = sy[tri[j]];
                    X[j][2]  = sz[tri[j]];
                    uv[j][0] = su[tri[j]];
                    uv[j][1] = sv[tri[j]];
                }
                p3p_solve(X, uv, S);
            }
            int cnt[P3P_SLOTS] = {0, 0, 0, 0};
            for (int h = 0; h < 64; ++h)
            {
                const int vh = __builtin_amdgcn_readlane(S.valid, h);
                if (vh == 0) continue;
#pragma unroll
                for (int s = 0; s < P3P_SLOTS; ++s)
                {
                    if (!((vh >> s) & 1)) continue;
                    double R[9], t[3];
#pragma unroll
                    for (int j = 0; j < 9; ++j) R[j] = readlane64(S.R[s][j], h);
#pragma unroll
                    for (int j = 0; j < 3; ++j) t[j] = readlane64(S.t[s][j], h);
                    int c = 0;
                    for (int i0 = 0; i0 < n; i0 += 64)
                    {
                        const int i    = i0 + lane;
                        const bool inl = i < n && p3p_inlier(R, t, sx[i], sy[i], sz[i], su[i], sv[i], threshold);
                        c += __popcll(__ballot(inl));
                    }
                    if (lane == h) cnt[s] = c;
                }
            }
            u64 mine = 0;
#pragma unroll
            for (int s = P3P_SLOTS - 1; s >= 0; --s)
            {
                const u64 cand = ((u64)(u32)cnt[s] << 32) | (u64)(0xffffffffu - (u32)(4 * k + s));
                if (((S.valid >> s) & 1) && cnt[s] > 0 && cand > mine) mine = cand;
            }
            if (dbg.triplet != nullptr && b == 0 && k < iterations)
            {
                int ns = 0;
#pragma unroll
                for (int s = 0; s < P3P_SLOTS; ++s)
                    if ((S.valid >> s) & 1)
                    {
                        double pose[7];
                        p3p_pose7(S.R[s], S.t[s], pose);
#pragma unroll
                        for (int j = 0; j < 7; ++j) dbg.poses[((size_t)k * 4 + ns) * 7 + j] = pose[j];
                        dbg.counts[(size_t)k * 4 + ns] = cnt[s];
                        ++ns;
                    }
                dbg.n_sol[k] = ns;
#pragma unroll
                for (int j = 0; j < 3; ++j) dbg.triplet[(size_t)k * 3 + j] = tri[j];
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
                if (mine == group)  // exactly one lane: the key holds k and the slot
                {
                    const int slot = (int)((0xffffffffu - (u32)group) & 3u);
#pragma unroll
                    for (int s = 0; s < P3P_SLOTS; ++s)
                        if (slot == s)
                        {
#pragma unroll
                            for (int j = 0; j < 9; ++j) s_pose[j] = S.R[s][j];
#pragma unroll
                            for (int j = 0; j < 3; ++j) s_pose[9 + j] = S.t[s][j];
                            // the solution index counts the poses of the hypothesis, not the slots
                            s_wave[0] = __popc((u32)S.valid & ((1u << s) - 1u));
                        }
                }
            }
            __syncthreads();
        }
    }
    // (s_wave[0] written under `group > best` is read below only when best != 0; the barrier at the end of the loop orders it)
    const bool found   = best != 0;
    const int best_sol = found ? s_wave[0] : -1;
    __syncthreads();

    // ---- the winner's mask, list and count ----
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
    if (found)
    {
#pragma unroll
        for (int j = 0; j < 9; ++j) R[j] = s_pose[j];
#pragma unroll
        for (int j = 0; j < 3; ++j) t[j] = s_pose[9 + j];
    }
    const int off = FRAME ? 0 : meta[b].off;
    int run       = 0;
    for (int i0 = 0; i0 < n; i0 += 256)
    {
        const int i    = i0 + tid;
        const bool inl = found && i < n && p3p_inlier(R, t, sx[i], sy[i], sz[i], su[i], sv[i], threshold);
        const u64 m    = __ballot(inl);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w)
        {
            before += w < wave ? s_wave[w] : 0;
            total += s_wave[w];
        }
        if (FRAME)
        {
            if (i < n && !inl) F.frame_pt[(size_t)b * F.cap + sfeat[i]] = -1;  // TrackingCoarse.cpp:433-440
        }
        else if (i < n)
        {
            mask_out[off + i] = inl ? 1 : 0;
            if (inl) list_out[off + run + before + lane_prefix(m)] = i;  // run + before + prefix < pairs visited <= n
        }
        run += total;
        __syncthreads();
    }
    if (tid == 0)
    {
        double pose[7];
        if (found) p3p_pose7(R, t, pose);
        if (FRAME)
        {
            F.inliers[b] = run;
            if (found)
#pragma unroll
                for (int j = 0; j < 7; ++j) F.poses[(size_t)b * 7 + j] = pose[j];
        }
        else
        {
            P3PResult r;
#pragma unroll
            for (int j = 0; j < 7; ++j) r.pose[j] = found ? pose[j] : meta[b].pose[j];
            r.inliers        = run;
            r.best_iteration = found ? (int)((0xffffffffu - (u32)best) >> 2) : -1;
            r.best_solution  = best_sol;
            r.pad            = 0;
            result[b]        = r;
        }
    }
}

size_t lds_bytes(int pairs)
{
    return (size_t)pairs * 44 + 8;
}

int check_params(const snk_p3p_params* p)
{
    SNK_REQUIRE(p != nullptr, "params is NULL");
    SNK_REQUIRE(p->iterations >= 0 && p->iterations <= P3P_MAX_ITERATIONS, "iterations outside [0, 2^20]");
    SNK_REQUIRE(p->residual_threshold > 0.0, "residual_threshold must be positive");
    return SNK_OK;
}

int ransac_host(snk_matcher* m, const snk_p3p_params* params, snk_p3p_problem* problems, int n_problems, P3PDebug dbg)
{
    size_t total = 0;
    int n_max    = 1;
    for (int i = 0; i < n_problems; ++i)
    {
        const snk_p3p_problem& P = problems[i];
        SNK_REQUIRE(P.n >= 0 && P.n <= P3P_MAX_PAIRS, "pairs per problem outside [0, 3072]");
        SNK_REQUIRE(P.n == 0 || (P.wps && P.nips && P.inlier_mask && P.inlier_matches), "NULL pair / result array with n > 0");
        total += (size_t)P.n;
        n_max = P.n > n_max ? P.n : n_max;
    }
    SNK_REQUIRE(total < (size_t)1 << 28, "too many pairs");
    SNK_HIP_CHECK(hipSetDevice(m->device));
    const size_t np = (size_t)n_problems;
    // up: P3PMeta[np] | wps[total] | nips[total] (the problems' rows one after the other)      back: P3PResult[np] | list[total] | mask[total]
    Block in, out;
    const int i_meta = in.add(nullptr, np * sizeof(P3PMeta)), i_wps = in.add(nullptr, total * 24), i_nip = in.add(nullptr, total * 16);
    const int r_res = out.add(nullptr, np * sizeof(P3PResult)), r_list = out.add(nullptr, total * 4), r_mask = out.add(nullptr, total);
    int rc;
    if ((rc = stage_reserve(m, in.bytes, out.end(), 64)) != SNK_OK) return rc;
    char* stage   = m->h_in.as<char>();
    P3PMeta* meta = in.at<P3PMeta>(stage, i_meta);
    size_t off    = 0;
    for (int i = 0; i < n_problems; ++i)
    {
        const snk_p3p_problem& P = problems[i];
        meta[i].off              = (int)off;
        meta[i].n                = P.n;
        memcpy(meta[i].pose, P.pose, 56);
        if (P.n > 0)
        {
            memcpy(in.at<char>(stage, i_wps) + off * 24, P.wps, (size_t)P.n * 24);
            memcpy(in.at<char>(stage, i_nip) + off * 16, P.nips, (size_t)P.n * 16);
        }
        off += (size_t)P.n;
    }
    if ((rc = stage_upload(m, in)) != SNK_OK) return rc;
    char* d = m->q.as<char>();
    char* o = m->out.as<char>();
    if ((rc = set_max_lds_once(reinterpret_cast<const void*>(p3p_ransac_kernel<false>), (int)lds_bytes(P3P_MAX_PAIRS))) != SNK_OK) return rc;
    P3PFrames F{};
    hipLaunchKernelGGL(p3p_ransac_kernel<false>, dim3(n_problems), dim3(256), lds_bytes(n_max), m->stream, in.at<const P3PMeta>(d, i_meta),
                       in.at<const double>(d, i_wps), in.at<const double>(d, i_nip), F, params->iterations, params->residual_threshold,
                       (u64)params->seed, n_max, out.at<u8>(o, r_mask), out.at<int>(o, r_list), out.at<P3PResult>(o, r_res), dbg);
    SNK_LAUNCH_CHECK();
    if ((rc = stage_download(m, 0, out.end())) != SNK_OK) return rc;
    char* back = m->h_res.as<char>();
    const P3PResult* res = out.at<const P3PResult>(back, r_res);
    off                  = 0;
    for (int i = 0; i < n_problems; ++i)
    {
        snk_p3p_problem& P = problems[i];
        if (res[i].inliers < 0 || res[i].inliers > P.n)
        {
            set_error("p3p: device returned %d inliers for %d pairs", res[i].inliers, P.n);
            return SNK_ERR_HIP;
        }
        memcpy(P.pose, res[i].pose, 56);
        P.inliers        = res[i].inliers;
        P.best_iteration = res[i].best_iteration;
        P.best_solution  = res[i].best_solution;
        if (P.n > 0)
        {
            memcpy(P.inlier_mask, out.at<char>(back, r_mask) + off, (size_t)P.n);
            memcpy(P.inlier_matches, out.at<char>(back, r_list) + off * 4, (size_t)res[i].inliers * 4);
        }
        off += (size_t)P.n;
    }
    return SNK_OK;
}
}  // namespace
}  // namespace snk

using namespace snk;

extern "C" {
int snk_p3p_ransac(snk_matcher* m, const snk_p3p_params* params, snk_p3p_problem* problems, int n_problems)
{
    SNK_REQUIRE(m != nullptr, "matcher is NULL");
    int rc;
    if ((rc = check_params(params)) != SNK_OK) return rc;
    SNK_REQUIRE(n_problems >= 0 && (n_problems == 0 || problems != nullptr), "bad problem array");
    if (n_problems == 0) return SNK_OK;
    return ransac_host(m, params, problems, n_problems, P3PDebug{nullptr, nullptr, nullptr, nullptr});
}

int snk_p3p_debug_hypotheses(snk_matcher* m, const snk_p3p_params* params, snk_p3p_problem* problem, int32_t (*triplets)[3],
                             int32_t* n_solutions, double (*poses)[4][7], int32_t (*counts)[4])
{
    SNK_REQUIRE(m != nullptr && problem != nullptr, "NULL argument");
    int rc;
    if ((rc = check_params(params)) != SNK_OK) return rc;
    const size_t it = (size_t)params->iterations;
    if (it == 0) return ransac_host(m, params, problem, 1, P3PDebug{nullptr, nullptr, nullptr, nullptr});
    SNK_REQUIRE(triplets && n_solutions && poses && counts, "NULL output array");
    SNK_HIP_CHECK(hipSetDevice(m->device));
    // triplet[it][3] | n_sol[it] | counts[it][4] | poses[it][4][7]
    const size_t o_ns = it * 12, o_cnt = o_ns + it * 4, o_pose = o_cnt + it * 16, bytes = o_pose + it * 224;
    if ((rc = m->aux.reserve(bytes)) != SNK_OK) return rc;
    char* d = m->aux.as<char>();
    SNK_HIP_CHECK(hipMemsetAsync(d, 0, bytes, m->stream));  // a problem with n < 4 runs no hypothesis
    P3PDebug dbg{reinterpret_cast<int*>(d), reinterpret_cast<int*>(d + o_ns), reinterpret_cast<double*>(d + o_pose),
                 reinterpret_cast<int*>(d + o_cnt)};
    if ((rc = ransac_host(m, params, problem, 1, dbg)) != SNK_OK) return rc;
    if ((rc = copy_sync(triplets, d, it * 12, hipMemcpyDeviceToHost, m->stream)) != SNK_OK) return rc;
    if ((rc = copy_sync(n_solutions, d + o_ns, it * 4, hipMemcpyDeviceToHost, m->stream)) != SNK_OK) return rc;
    if ((rc = copy_sync(counts, d + o_cnt, it * 16, hipMemcpyDeviceToHost, m->stream)) != SNK_OK) return rc;
    return copy_sync(poses, d + o_pose, it * 224, hipMemcpyDeviceToHost, m->stream);
}

int snk_p3p_ransac_frame_batch_dev(snk_matcher* m, const snk_frames_dev* frames, const snk_camera* cam, const snk_p3p_params* params,
                                   const void* pts_dev, int pts_stride, int32_t* frame_pt_dev, const int32_t* n_pts_dev, int pts_cap,
                                   double* poses_dev, int32_t* inliers_dev)
{
    SNK_REQUIRE(m != nullptr && frames != nullptr && cam != nullptr, "NULL argument");
    int rc;
    if ((rc = check_params(params)) != SNK_OK) return rc;
    SNK_REQUIRE(frames->batch >= 0 && frames->cap >= 1 && frames->kps != nullptr && frames->n != nullptr, "bad frames");
    SNK_REQUIRE(frames->cap <= P3P_MAX_PAIRS, "frames->cap above 3072 features");
    SNK_REQUIRE(pts_dev && frame_pt_dev && n_pts_dev && poses_dev && inliers_dev, "NULL device buffer");
    SNK_REQUIRE(pts_stride >= 24 && pts_stride % 8 == 0 && pts_cap >= 1, "pts_stride must be a multiple of 8, >= 24");
    SNK_REQUIRE(cam->fx != 0.0 && cam->fy != 0.0, "fx / fy must not be 0");
    if (frames->batch == 0) return SNK_OK;
    SNK_HIP_CHECK(hipSetDevice(m->device));
    if ((rc = set_max_lds_once(reinterpret_cast<const void*>(p3p_ransac_kernel<true>), (int)lds_bytes(P3P_MAX_PAIRS))) != SNK_OK) return rc;
    P3PFrames F;
    F.kps = frames->kps; F.n_feat = frames->n; F.pts = reinterpret_cast<const u8*>(pts_dev); F.frame_pt = frame_pt_dev;
    F.n_pts = n_pts_dev; F.poses = poses_dev; F.inliers = inliers_dev;
    F.cap = frames->cap; F.pts_cap = pts_cap; F.pts_stride = pts_stride;
    F.fx = cam->fx; F.fy = cam->fy; F.cx = cam->cx; F.cy = cam->cy;
    hipLaunchKernelGGL(p3p_ransac_kernel<true>, dim3(frames->batch), dim3(256), lds_bytes(frames->cap), m->stream, nullptr, nullptr, nullptr,
                       F, params->iterations, params->residual_threshold, (u64)params->seed, frames->cap, nullptr, nullptr, nullptr,
                       P3PDebug{nullptr, nullptr, nullptr, nullptr});
    SNK_LAUNCH_CHECK();
    return SNK_OK;
}
}
