// New map points from matched keyframe pairs for gfx950 — replaces
//   the geometric loop of Triangulator::triangulate       (reference Snake/LocalMapping/Triangulator.cpp:127-157, :174-291)
//   the neighbour loop and the first-wins commit test of
//   Triangulator::Process                                  (reference Snake/LocalMapping/Triangulator.cpp:42-47, :61-70)
//
// Mapping to the hardware.  tri_pairs_kernel: one workgroup per neighbour keyframe, one fp64 thread per matched pair (tri_core.hpp: the
// parallax test, the 4 x 4 homogeneous system by one-sided Jacobi in registers, the stereo fallbacks, the gates); the survivors of a
// 256-pair chunk are compacted in pair order with a ballot + mbcnt prefix inside each wavefront, the four wavefront counts through LDS
// and a running offset per workgroup -- no global scan, no atomics.  tri_commit_kernel: ONE wavefront visits the candidates in the
// reference's order (neighbour, then pair), 64 at a time; "feature already has a point or an earlier kept candidate used it" is two
// LDS bitmaps (keyframe-1 features, features of the current neighbour) for everything before the chunk and a lane-ordered pass over
// the chunk's own candidates (readlane + ballot, uniform control flow).  Two launches, one upload, one download per call.
#include <cstddef>

#include "matcher_handle.hpp"
#include "tri_core.hpp"

namespace snk
{
namespace
{
using u8  = unsigned char;
using u32 = unsigned int;
using u64 = unsigned long long;

static_assert(sizeof(snk_new_point) == 40 && offsetof(snk_new_point, commit) == 13 && offsetof(snk_new_point, pos) == 16, "snk_new_point layout");

constexpr int TRI_MAX_FEATURES = 65536;  // per keyframe: the commit pass keeps one bit per feature in LDS (2 x 8 KB)
constexpr int TRI_MAX_LEVELS   = 32;

struct TriViewDev
{
    TriPose P;
    const snk_kp64* kps;
    const float* right_points;
    const float* depth;
    const u8* has_mp;
    int pair_begin, pair_end;  // this neighbour's slice of `pairs`
    int skip;                  // the baseline gate of :140-157 said "no points from this neighbour"
    int n;
};

struct TriCallDev
{
    TriConst K;
    TriViewDev kf1;
    float level_scale[TRI_MAX_LEVELS];
};

__device__ __forceinline__ TriFeature load_feature(const TriViewDev& v, int idx, const float* scale)
{
    const snk_kp64 kp = v.kps[idx];
    TriFeature f;
    f.x     = kp.x;
    f.y     = kp.y;
    f.ur    = v.right_points[idx];
    f.depth = v.depth[idx];
    f.scale = scale[kp.octave];
    return f;
}

// cand[pair_begin + k] = k-th surviving pair of neighbour blockIdx.x (pair order), count[blockIdx.x] = how many
__global__ __launch_bounds__(256) void tri_pairs_kernel(TriCallDev C, const TriViewDev* __restrict__ views, const int2* __restrict__ pairs,
                                                        snk_new_point* __restrict__ cand, int* __restrict__ count)
{
    __shared__ float s_scale[TRI_MAX_LEVELS];
    __shared__ int s_wave[4];
    __shared__ TriViewDev s_view;
    const int nb = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < TRI_MAX_LEVELS) s_scale[tid] = C.level_scale[tid];
    if (tid == 0) s_view = views[nb];
    __syncthreads();
    const int begin = s_view.pair_begin, end = s_view.skip ? s_view.pair_begin : s_view.pair_end;
    int run = 0;
    for (int base = begin; base < end; base += 256)
    {
        const int i = base + tid;
        snk_new_point rec;
        int branch = TRI_REJECT;
        if (i < end)
        {
            const int2 pr        = pairs[i];
            const TriFeature f1  = load_feature(C.kf1, pr.x, s_scale);
            const TriFeature f2  = load_feature(s_view, pr.y, s_scale);
            bool far_away        = false;
            double X[3]          = {0, 0, 0};
            branch               = tri_pair(C.K, C.kf1.P, s_view.P, f1, f2, X, far_away);
            rec.feature1         = pr.x;
            rec.feature2         = pr.y;
            rec.neighbour        = nb;
            rec.far_away         = far_away ? 1 : 0;
            rec.commit           = 0;
            rec.branch           = (u8)branch;
            rec.pad              = 0;
            rec.pos[0]           = X[0];
            rec.pos[1]           = X[1];
            rec.pos[2]           = X[2];
        }
        const bool keep = branch != TRI_REJECT;
        const u64 mask  = __ballot(keep);
        const int below = __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0));
        if (lane == 0) s_wave[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w)
        {
            before += w < wave ? s_wave[w] : 0;
            total += s_wave[w];
        }
        if (keep) cand[begin + run + before + below] = rec;  // run + before + below < pairs visited so far <= pair_end - pair_begin
        run += total;
        __syncthreads();
    }
    if (tid == 0) count[nb] = run;
}

__device__ __forceinline__ bool bit_of(const u32* bm, int i)
{
    return (bm[i >> 5] >> (i & 31)) & 1u;
}

// out_start[0 .. n_views] = offsets of each neighbour's points, out[...] = the candidates compacted over the neighbours with `commit`
// filled by the ordered pass of :61-70.  One wavefront.
__global__ __launch_bounds__(64) void tri_commit_kernel(TriViewDev kf1, const TriViewDev* __restrict__ views, int n_views,
                                                        const snk_new_point* __restrict__ cand, const int* __restrict__ count,
                                                        int* __restrict__ out_start, snk_new_point* __restrict__ out)
{
    __shared__ u32 used1[TRI_MAX_FEATURES / 32], used2[TRI_MAX_FEATURES / 32];
    const int lane = threadIdx.x;
    for (int w = lane; w < (kf1.n + 31) / 32; w += 64) used1[w] = 0;
    int o = 0;
    for (int nb = 0; nb < n_views; ++nb)
    {
        const int n2 = views[nb].n, begin = views[nb].pair_begin, cnt = count[nb];
        const u8* has2 = views[nb].has_mp;
        for (int w = lane; w < (n2 + 31) / 32; w += 64) used2[w] = 0;
        if (lane == 0) out_start[nb] = o;
        __syncthreads();
        for (int base = 0; base < cnt; base += 64)
        {
            const int k      = base + lane;
            const bool valid = k < cnt;
            // a record as five 64-bit words (feature1 | feature2, neighbour | far_away | commit | branch | pad, pos[3]): moved in registers
            u64 w0 = 0, w1 = 0, w2 = 0, w3 = 0, w4 = 0;
            int f1 = -1, f2 = -1;
            bool ok = false;
            if (valid)
            {
                const u64* src = reinterpret_cast<const u64*>(cand + begin + k);
                w0 = src[0]; w1 = src[1]; w2 = src[2]; w3 = src[3]; w4 = src[4];
                f1 = (int)(u32)w0;
                f2 = (int)(u32)(w0 >> 32);
                ok = !kf1.has_mp[f1] && !has2[f2] && !bit_of(used1, f1) && !bit_of(used2, f2);
            }
            // the chunk's own candidates in lane order: lane l is kept iff no earlier KEPT lane used one of its two features
            u64 kept = 0;
            for (u64 todo = __ballot(ok); todo; todo &= todo - 1)
            {
                const int l     = __builtin_ctzll(todo);
                const int l1    = __builtin_amdgcn_readlane(f1, l), l2 = __builtin_amdgcn_readlane(f2, l);
                const u64 clash = __ballot(f1 == l1 || f2 == l2) & kept;  // kept holds lanes below l only
                kept |= clash ? 0ull : (1ull << l);
            }
            const bool commit = (kept >> lane) & 1ull;
            if (commit)
            {
                atomicOr(&used1[f1 >> 5], 1u << (f1 & 31));
                atomicOr(&used2[f2 >> 5], 1u << (f2 & 31));
            }
            if (valid)
            {
                u64* dst = reinterpret_cast<u64*>(out + o + k);
                dst[0]   = w0;
                dst[1]   = (w1 & ~(0xffull << 40)) | ((u64)(commit ? 1 : 0) << 40);  // byte 13 of the record = commit
                dst[2]   = w2;
                dst[3]   = w3;
                dst[4]   = w4;
            }
            __syncthreads();
        }
        o += cnt;
    }
    if (lane == 0) out_start[n_views] = o;
}

void make_pose(const double* pose, TriPose* P)
{
    const double x = pose[0], y = pose[1], z = pose[2], w = pose[3];
    double* R = P->R;
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w);     R[2] = 2 * (x * z + y * w);
    R[3] = 2 * (x * y + z * w);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
    R[6] = 2 * (x * z - y * w);     R[7] = 2 * (y * z + x * w);     R[8] = 1 - 2 * (x * x + y * y);
    for (int i = 0; i < 3; ++i) P->t[i] = pose[4 + i];
    for (int i = 0; i < 3; ++i) P->c[i] = -(R[i] * P->t[0] + R[3 + i] * P->t[1] + R[6 + i] * P->t[2]);  // pose.inverse().translation()
}

int check_view(const snk_tri_view* v)
{
    SNK_REQUIRE(v != nullptr, "keyframe view is NULL");
    SNK_REQUIRE(v->n >= 0 && v->n <= TRI_MAX_FEATURES, "keyframe view: n outside [0, 65536]");
    SNK_REQUIRE(v->n == 0 || (v->kps && v->right_points && v->depth && v->has_mp), "keyframe view: NULL array with n > 0");
    return SNK_OK;
}

// a view's arrays as four parts of the upload block (stage.hpp): kps | right_points | depth | has_mp
struct ViewParts
{
    int kps, right_points, depth, has_mp;
};
ViewParts add_view(Block& in, const snk_tri_view* v)
{
    const size_t nn = (size_t)v->n;
    return ViewParts{in.add(v->kps, nn * sizeof(snk_kp64)), in.add(v->right_points, nn * 4), in.add(v->depth, nn * 4), in.add(v->has_mp, nn)};
}

// the view as the kernels take it: its pose, its arrays at their device addresses
void view_on_device(const snk_tri_view* v, const Block& in, char* dev, const ViewParts& p, TriViewDev* V)
{
    V->n = v->n;
    make_pose(v->pose, &V->P);
    V->kps          = in.at<const snk_kp64>(dev, p.kps);
    V->right_points = in.at<const float>(dev, p.right_points);
    V->depth        = in.at<const float>(dev, p.depth);
    V->has_mp       = in.at<const u8>(dev, p.has_mp);
}

int triangulate_impl(snk_matcher* m, const snk_camera* cam, const snk_tri_params* params, const snk_tri_view* kf1, const snk_tri_view* kf2s,
                     const float* median_depth2s, int n_nb, const int32_t (*pairs)[2], const int32_t* pair_start, const float* level_scale,
                     int n_levels, snk_new_point* out, int32_t* out_start, int* n_out)
{
    SNK_REQUIRE(m != nullptr && n_out != nullptr, "NULL argument");
    *n_out = 0;
    SNK_REQUIRE(cam != nullptr && params != nullptr, "camera / params is NULL");
    SNK_REQUIRE(cam->fx != 0 && cam->fy != 0, "camera: zero focal length");
    SNK_REQUIRE(level_scale != nullptr && n_levels >= 1 && n_levels <= TRI_MAX_LEVELS, "level_scale / n_levels (1..32)");
    SNK_REQUIRE(n_nb >= 0, "negative neighbour count");
    if (out_start)
        for (int k = 0; k <= n_nb; ++k) out_start[k] = 0;
    if (n_nb == 0) return SNK_OK;
    SNK_REQUIRE(kf2s != nullptr && pair_start != nullptr && out_start != nullptr, "NULL neighbour arrays with n_neighbours > 0");
    SNK_REQUIRE(!params->mono || median_depth2s != nullptr, "mono: median_depth2 is NULL");
    int rc;
    if ((rc = check_view(kf1)) != SNK_OK) return rc;
    SNK_REQUIRE(pair_start[0] == 0, "pair_start[0] must be 0");
    // one upload: the TriViewDev table (filled in the staging buffer below) | kf1's arrays | every neighbour's | pairs
    Block in, out_b;
    const int i_views  = in.add(nullptr, (size_t)n_nb * sizeof(TriViewDev));
    const ViewParts p1 = add_view(in, kf1);
    std::vector<ViewParts> p2((size_t)n_nb);
    for (int k = 0; k < n_nb; ++k)
    {
        if ((rc = check_view(&kf2s[k])) != SNK_OK) return rc;
        SNK_REQUIRE(pair_start[k + 1] >= pair_start[k], "pair_start must be non-decreasing");
        p2[(size_t)k] = add_view(in, &kf2s[k]);
    }
    const int n_pairs = pair_start[n_nb];
    if (n_pairs == 0) return SNK_OK;
    SNK_REQUIRE(pairs != nullptr && out != nullptr, "NULL pairs / out with a non-zero pair count");
    for (int k = 0; k < n_nb; ++k)
        for (int i = pair_start[k]; i < pair_start[k + 1]; ++i)
        {
            const int a = pairs[i][0], b = pairs[i][1];
            SNK_REQUIRE(a >= 0 && a < kf1->n, "pair: keyframe-1 feature index out of range");
            SNK_REQUIRE(b >= 0 && b < kf2s[k].n, "pair: keyframe-2 feature index out of range");
            SNK_REQUIRE(kf1->kps[a].octave >= 0 && kf1->kps[a].octave < n_levels, "pair: keyframe-1 octave outside [0, n_levels)");
            SNK_REQUIRE(kf2s[k].kps[b].octave >= 0 && kf2s[k].kps[b].octave < n_levels, "pair: keyframe-2 octave outside [0, n_levels)");
        }
    const int i_pairs = in.add(pairs, (size_t)n_pairs * 8);
    // results: out_start[n_nb + 1] | points[n_pairs]; scratch behind them, on the device only: count[n_nb] | candidates[n_pairs]
    const int o_start = out_b.add(nullptr, (size_t)(n_nb + 1) * 4), o_pts = out_b.add(nullptr, (size_t)n_pairs * sizeof(snk_new_point));
    const size_t r_bytes = out_b.end();
    const int o_count = out_b.add(nullptr, (size_t)n_nb * 4), o_cand = out_b.add(nullptr, (size_t)n_pairs * sizeof(snk_new_point));
    SNK_HIP_CHECK(hipSetDevice(m->device));
    if ((rc = m->out.reserve(out_b.end())) != SNK_OK) return rc;  // with the scratch; the pinned block holds the results only
    if ((rc = stage_reserve(m, in.bytes, r_bytes)) != SNK_OK) return rc;
    char *host = m->h_in.as<char>(), *dev = m->q.as<char>();
    TriCallDev C;
    C.K.fx = cam->fx; C.K.fy = cam->fy; C.K.cx = cam->cx; C.K.cy = cam->cy; C.K.bf = cam->bf;
    C.K.th_depth     = params->th_depth;
    C.K.chi2_mono    = params->error_mono * params->error_mono;      // :127
    C.K.chi2_stereo  = params->error_stereo * params->error_stereo;  // :128
    C.K.ratio_factor = 1.5f * params->scale_factor;                  // :132
    for (int i = 0; i < TRI_MAX_LEVELS; ++i) C.level_scale[i] = level_scale[i < n_levels ? i : n_levels - 1];
    view_on_device(kf1, in, dev, p1, &C.kf1);
    C.kf1.pair_begin = 0; C.kf1.pair_end = n_pairs; C.kf1.skip = 0;
    TriViewDev* hv = in.at<TriViewDev>(host, i_views);
    for (int k = 0; k < n_nb; ++k)
    {
        view_on_device(&kf2s[k], in, dev, p2[(size_t)k], &hv[k]);
        hv[k].pair_begin = pair_start[k];
        hv[k].pair_end   = pair_start[k + 1];
        // the per-neighbour baseline gate, :140-157
        const double* c1 = C.kf1.P.c;
        const double* c2 = hv[k].P.c;
        const double dx = c1[0] - c2[0], dy = c1[1] - c2[1], dz = c1[2] - c2[2];
        const double baseline = std::sqrt(dx * dx + dy * dy + dz * dz);
        if (params->mono)
        {
            const float ratio_baseline_depth = (float)(baseline / (double)median_depth2s[k]);  // :146
            hv[k].skip                       = (double)ratio_baseline_depth < 0.01 ? 1 : 0;
        }
        else
            hv[k].skip = baseline < cam->bf / cam->fx ? 1 : 0;  // stereo_cam.baseLine() [DEFINED] = bf / fx
    }
    if ((rc = stage_upload(m, in)) != SNK_OK) return rc;  // the table is in place: it has no source
    char* dout          = m->out.as<char>();
    int* d_out_start    = out_b.at<int>(dout, o_start);
    snk_new_point* d_pt = out_b.at<snk_new_point>(dout, o_pts);
    int* d_count        = out_b.at<int>(dout, o_count);
    snk_new_point* d_cd = out_b.at<snk_new_point>(dout, o_cand);
    const TriViewDev* d_views = in.at<const TriViewDev>(dev, i_views);
    hipLaunchKernelGGL(tri_pairs_kernel, dim3(n_nb), dim3(256), 0, m->stream, C, d_views, in.at<const int2>(dev, i_pairs), d_cd, d_count);
    SNK_LAUNCH_CHECK();
    hipLaunchKernelGGL(tri_commit_kernel, dim3(1), dim3(64), 0, m->stream, C.kf1, d_views, n_nb, d_cd, d_count, d_out_start, d_pt);
    SNK_LAUNCH_CHECK();
    if ((rc = stage_download(m, 0, r_bytes)) != SNK_OK) return rc;
    const int* h_start = out_b.at<const int>(m->h_res.as<char>(), o_start);
    const int total    = h_start[n_nb];
    if (total < 0 || total > n_pairs)
    {
        set_error("triangulation: device returned %d points for %d pairs", total, n_pairs);
        return SNK_ERR_HIP;
    }
    memcpy(out_start, h_start, (size_t)(n_nb + 1) * 4);
    memcpy(out, out_b.at<char>(m->h_res.as<char>(), o_pts), (size_t)total * sizeof(snk_new_point));
    *n_out = total;
    return SNK_OK;
}
}  // namespace
}  // namespace snk

using namespace snk;

extern "C" {
int snk_triangulate_pairs(snk_matcher* m, const snk_camera* cam, const snk_tri_params* params, const snk_tri_view* kf1,
                          const snk_tri_view* kf2, float median_depth2, const int32_t (*pairs)[2], int n_pairs, const float* level_scale,
                          int n_levels, snk_new_point* out, int* n_out)
{
    SNK_REQUIRE(n_out != nullptr, "NULL argument");
    *n_out = 0;
    SNK_REQUIRE(n_pairs >= 0, "negative pair count");
    const int32_t pair_start[2] = {0, n_pairs};
    int32_t out_start[2];
    return triangulate_impl(m, cam, params, kf1, kf2, &median_depth2, 1, pairs, pair_start, level_scale, n_levels, out, out_start, n_out);
}

int snk_triangulate_neighbours(snk_matcher* m, const snk_camera* cam, const snk_tri_params* params, const snk_tri_view* kf1,
                               const snk_tri_view* kf2s, const float* median_depth2s, int n_neighbours, const int32_t (*pairs)[2],
                               const int32_t* pair_start, const float* level_scale, int n_levels, snk_new_point* out, int32_t* out_start,
                               int* n_out)
{
    return triangulate_impl(m, cam, params, kf1, kf2s, median_depth2s, n_neighbours, pairs, pair_start, level_scale, n_levels, out,
                            out_start, n_out);
}
}
