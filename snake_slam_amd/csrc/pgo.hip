// Pose-graph optimisation of the loop corrector, semantics "snk-pgo v1" (DESIGN.md section 3f): Levenberg-Marquardt over SE3 / Sim3
// vertices with exact Jacobians (pgo_core.hpp), block-Jacobi PCG on the block-sparse normal equations.  f64, gfx950.
//
//   pgo_linearise_kernel   one lane per edge: residual, J_i, J_j (three 7 x 7 work matrices per lane in LDS, interleaved by lane), then
//                          J_i^T J_i, J_i^T J_j, J_j^T J_j, J_i^T r, J_j^T r to per-edge slots
//   pgo_assemble_kernel    one wavefront per vertex: 49 lanes sum the diagonal block, 7 the gradient over the vertex's incident-edge list
//                          (CSR in edge order, built once by snk_pgo_set_graph)
//   pgo_damp_kernel        one lane per free row: D + lambda clamp(diag D), its inverse by Gauss-Jordan (in LDS, interleaved by lane)
//   pgo_pcg_kernel<true>   the whole PCG as ONE cooperative launch: a workgroup owns a contiguous range of block rows, keeps their
//                          off-diagonal blocks, the damped diagonal, its inverse and its five vectors in LDS, exchanges z = M^-1 r through
//                          global memory; two grid barriers per iteration (A p is carried by the recurrence A p = A z + beta A p)
//   pgo_pcg_kernel<false>  the same statements as one launch per phase with everything in global memory: the fallback for graphs whose
//                          rows do not fit the resident form, for a refused cooperative launch, and under SNK_PGO_PCG_LAUNCHES=1
//   pgo_update_kernel, pgo_cost_kernel, pgo_decide_kernel, pgo_commit_kernel   trial state, its cost, accept / reject and the lambda
//                          schedule on the device; the host reads one 88-byte record per LM iteration
//   pgo_transform_points_kernel   the map-point pass of OptimizeEssentialGraph
// Every sum runs in a fixed order; no floating-point atomics.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "pgo_core.hpp"

namespace snk
{
namespace pgo_impl
{
constexpr int LIN_THREADS  = 64;                          // lanes (edges) per workgroup of the linearisation
constexpr int LIN_LDS      = LIN_THREADS * 3 * 49 * 8;    // 75 264 bytes: two workgroups per compute unit
constexpr int DAMP_THREADS = 64;
constexpr int DAMP_LDS     = DAMP_THREADS * 49 * 8;       // 25 088 bytes
constexpr int PCG_THREADS  = 256;
constexpr int PCG_LDS_CAP  = 150 * 1024;                  // dynamic LDS of the resident PCG (160 KB per compute unit, one workgroup each)
constexpr int RED_THREADS  = 1024;

struct LmState  // the record the host reads after every LM iteration
{
    double cost, cost_trial, lambda, v, cost_initial, min_delta, cost_query;
    int accepted_last, stop, lm_iterations, accepted_steps, pcg_total, pcg_done, pcg_max, pad;
};
static_assert(sizeof(LmState) == 88, "LmState layout");

struct Dev
{
    int n, E, D, nrows, nwg, max_pcg;
    double pcg_tol;
    double *pose, *trial;
    const double *before, *meas, *weight;
    const int *edges, *rowof, *rowvert, *vstart, *vlist, *rbstart, *rbedge, *rbcol, *wgstart;
    const unsigned char* constant;
    double *Hii, *Hij, *Hjj, *gi, *gj, *res, *diag, *grad, *Dd, *Dinv, *Z, *X, *R, *P, *Ap, *part_pap, *part_rz, *part_rz0, *r2;
    unsigned* bar;
    LmState* lm;
};

__global__ __launch_bounds__(LIN_THREADS) void pgo_linearise_kernel(Dev G)
{
    extern __shared__ double lin_lds[];
    const int e = blockIdx.x * LIN_THREADS + threadIdx.x;
    if (e >= G.E) return;
    pgo::Mat<LIN_THREADS> N{lin_lds + threadIdx.x}, P{lin_lds + 49 * LIN_THREADS + threadIdx.x}, S{lin_lds + 98 * LIN_THREADS + threadIdx.x};
    const int i = G.edges[2 * e], j = G.edges[2 * e + 1];
    double Ti[8], Tj[8], M[8], r[7], g[7];
#pragma unroll
    for (int k = 0; k < 8; ++k) Ti[k] = G.pose[(size_t)i * 8 + k], Tj[k] = G.pose[(size_t)j * 8 + k], M[k] = G.meas[(size_t)e * 8 + k];
    pgo::edge_jacobians(Ti, Tj, M, G.weight[e], G.D, r, N, P, S);
#pragma unroll
    for (int a = 0; a < 7; ++a) G.res[(size_t)e * 7 + a] = r[a];
    pgo::at_b(P, P, G.Hii + (size_t)e * 49);
    pgo::at_b(P, S, G.Hij + (size_t)e * 49);
    pgo::at_b(S, S, G.Hjj + (size_t)e * 49);
    pgo::at_r(P, r, g);
#pragma unroll
    for (int a = 0; a < 7; ++a) G.gi[(size_t)e * 7 + a] = g[a];
    pgo::at_r(S, r, g);
#pragma unroll
    for (int a = 0; a < 7; ++a) G.gj[(size_t)e * 7 + a] = g[a];
}

__global__ __launch_bounds__(256) void pgo_assemble_kernel(Dev G)
{
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (v >= G.n || lane >= 56) return;
    double s = 0.0;
    for (int k = G.vstart[v]; k < G.vstart[v + 1]; ++k)  // edge order
    {
        const int e = G.vlist[k] >> 1, side = G.vlist[k] & 1;
        if (lane < 49)
            s += (side ? G.Hjj : G.Hii)[(size_t)e * 49 + lane];
        else
            s += (side ? G.gj : G.gi)[(size_t)e * 7 + (lane - 49)];
    }
    if (lane < 49)
        G.diag[(size_t)v * 49 + lane] = s;
    else
        G.grad[(size_t)v * 7 + (lane - 49)] = s;
}

__global__ __launch_bounds__(DAMP_THREADS) void pgo_damp_kernel(Dev G)
{
    extern __shared__ double damp_lds[];
    const int row = blockIdx.x * DAMP_THREADS + threadIdx.x;
    if (row >= G.nrows) return;
    pgo::Mat<DAMP_THREADS> A{damp_lds + threadIdx.x};
    const double* d     = G.diag + (size_t)G.rowvert[row] * 49;
    const double lambda = G.lm->lambda;
    for (int a = 0; a < 7; ++a)
        for (int b = 0; b < 7; ++b)
        {
            double x = d[a * 7 + b];
            if (a == b) x = a < G.D ? x + lambda * fmin(fmax(x, 1e-6), 1e32) : 1.0;  // the se3 form: an identity row for the unused sigma
            A(a, b)                         = x;
            G.Dd[(size_t)row * 49 + a * 7 + b] = x;
        }
    for (int k = 0; k < 7; ++k)  // Gauss-Jordan in place, no pivoting: the damped block is symmetric positive definite
    {
        const double p = 1.0 / A(k, k);
        A(k, k)        = 1.0;
        for (int b = 0; b < 7; ++b) A(k, b) *= p;
        for (int a = 0; a < 7; ++a)
        {
            if (a == k) continue;
            const double f = A(a, k);
            A(a, k)        = 0.0;
            for (int b = 0; b < 7; ++b) A(a, b) -= f * A(k, b);
        }
    }
    for (int k = 0; k < 49; ++k) G.Dinv[(size_t)row * 49 + k] = A.p[k * DAMP_THREADS];
}

// ---- PCG ----
// Flat grid barrier of ba.hip (grid_barrier_flat): one flag per workgroup, a release store and polling by the first wavefront.
__device__ __forceinline__ void pgo_grid_barrier(unsigned* bar, unsigned n_wgs, unsigned& phase)
{
    __syncthreads();
    ++phase;
    if (threadIdx.x < 64)
    {
        if (threadIdx.x == 0) __hip_atomic_store(bar + blockIdx.x, phase, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        for (;;)
        {
            bool ok = true;
            for (unsigned i = threadIdx.x; i < n_wgs; i += 64) ok = ok && __hip_atomic_load(bar + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= phase;
            if (__builtin_amdgcn_ballot_w64(ok) == ~0ull) break;
            __builtin_amdgcn_s_sleep(1);
        }
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
    }
    __syncthreads();
}

// sum of n per-workgroup partials, the same value in every lane of every wavefront: lane l adds entries l, l + 64, ..., then a butterfly
__device__ __forceinline__ double sum_partials(const double* a, int n)
{
    double t = 0.0;
    for (int i = threadIdx.x & 63; i < n; i += 64) t += __hip_atomic_load(a + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return wave_sum64_dpp(t);
}

// sum over the workgroup's threads in a fixed order, returned to every thread
__device__ __forceinline__ double block_sum(double v, double* red)
{
    v = wave_sum64_dpp(v);
    __syncthreads();  // red may still be read from the previous sum
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// phase: -1 = all of it (RES, cooperative); 0 = initialise, 1 = direction + matrix product of iteration k, 2 = step of iteration k (one
// launch each, !RES)
template <bool RES>
__global__ __launch_bounds__(PCG_THREADS) void pgo_pcg_kernel(Dev G, int phase_arg, int k_arg)
{
    extern __shared__ double pcg_lds[];
    __shared__ double red[4];
    const int tid = threadIdx.x, wg = blockIdx.x, nwg = G.nwg;
    const int r0 = G.wgstart[wg], R = G.wgstart[wg + 1] - r0, nb0 = G.rbstart[r0], NB = G.rbstart[r0 + R] - nb0;
    const int nel = R * 7;
    double* blk = pcg_lds;
    double *Dd, *Di, *xv, *rv, *zv, *pv, *apv;
    if (RES)
    {
        Dd = blk + (size_t)NB * 49, Di = Dd + R * 49, xv = Di + R * 49, rv = xv + nel, zv = rv + nel, pv = zv + nel, apv = pv + nel;
        for (int idx = tid; idx < NB * 49; idx += PCG_THREADS) blk[idx] = G.Hij[(size_t)(G.rbedge[nb0 + idx / 49] >> 1) * 49 + idx % 49];
        for (int idx = tid; idx < R * 49; idx += PCG_THREADS) Dd[idx] = G.Dd[(size_t)r0 * 49 + idx], Di[idx] = G.Dinv[(size_t)r0 * 49 + idx];
    }
    else
    {
        __shared__ int done_s;  // read once per workgroup: workgroup 0 may set the word while this launch runs
        if (tid == 0) done_s = G.lm->pcg_done;
        __syncthreads();
        if (done_s) return;
        Dd = G.Dd + (size_t)r0 * 49, Di = G.Dinv + (size_t)r0 * 49;
        xv = G.X + (size_t)r0 * 7, rv = G.R + (size_t)r0 * 7, zv = G.Z + (size_t)r0 * 7, pv = G.P + (size_t)r0 * 7, apv = G.Ap + (size_t)r0 * 7;
    }
    unsigned bphase = 0;

    if (RES || phase_arg == 0)
    {
        for (int idx = tid; idx < nel; idx += PCG_THREADS)
        {
            xv[idx] = 0.0, pv[idx] = 0.0, apv[idx] = 0.0;
            rv[idx] = -G.grad[(size_t)G.rowvert[r0 + idx / 7] * 7 + idx % 7];
        }
        __syncthreads();
        double dot = 0.0;
        for (int idx = tid; idx < nel; idx += PCG_THREADS)
        {
            const int lr = idx / 7, a = idx % 7;
            double z = 0.0;
#pragma unroll
            for (int b = 0; b < 7; ++b) z += Di[lr * 49 + a * 7 + b] * rv[lr * 7 + b];
            if (RES) zv[idx] = z;
            G.Z[(size_t)r0 * 7 + idx] = z;
            dot += rv[idx] * z;
        }
        dot = block_sum(dot, red);
        if (tid == 0) G.part_rz[wg] = dot, G.part_rz0[wg] = dot;
        if (!RES) return;
    }

    for (int k = RES ? 0 : k_arg;; ++k)
    {
        if (RES) pgo_grid_barrier(G.bar, nwg, bphase);
        const double rz = sum_partials(G.part_rz + (k & 1) * nwg, nwg);
        if (RES || phase_arg == 1)
        {
            const double rz0 = sum_partials(G.part_rz0, nwg);
            if (!(rz0 > 0.0) || rz <= G.pcg_tol * rz0 || k >= G.max_pcg)  // grid-uniform: every workgroup adds the same partials in the same order
            {
                if (wg == 0 && tid == 0)
                {
                    G.lm->pcg_done = 1;
                    if (RES) G.lm->pcg_total += k;
                    if (k > G.lm->pcg_max) G.lm->pcg_max = k;
                }
                break;
            }
            const double beta = k == 0 ? 0.0 : rz / sum_partials(G.part_rz + ((k + 1) & 1) * nwg, nwg);
            double dot        = 0.0;
            for (int idx = tid; idx < nel; idx += PCG_THREADS)
            {
                const int lr = idx / 7, a = idx % 7, row = r0 + lr;
                double acc = 0.0;
#pragma unroll
                for (int b = 0; b < 7; ++b) acc += Dd[lr * 49 + a * 7 + b] * (RES ? zv[lr * 7 + b] : G.Z[(size_t)row * 7 + b]);
                for (int bi = G.rbstart[row]; bi < G.rbstart[row + 1]; ++bi)
                {
                    const int e2 = G.rbedge[bi], tr = e2 & 1;
                    const double* H = RES ? blk + (size_t)(bi - nb0) * 49 : G.Hij + (size_t)(e2 >> 1) * 49;
                    const double* z = G.Z + (size_t)G.rbcol[bi] * 7;
#pragma unroll
                    for (int b = 0; b < 7; ++b) acc += H[tr ? b * 7 + a : a * 7 + b] * z[b];
                }
                const double apn = acc + beta * apv[idx], pn = zv[idx] + beta * pv[idx];
                apv[idx] = apn, pv[idx] = pn;
                dot += pn * apn;
            }
            dot = block_sum(dot, red);
            if (tid == 0) G.part_pap[wg] = dot;
            if (!RES) return;
        }
        if (RES) pgo_grid_barrier(G.bar, nwg, bphase);
        {
            const double pap = sum_partials(G.part_pap, nwg);
            if (!(pap > 0.0))  // breakdown (a direction of no curvature): keep x
            {
                if (wg == 0 && tid == 0)
                {
                    G.lm->pcg_done = 1;
                    if (RES) G.lm->pcg_total += k;
                    if (k > G.lm->pcg_max) G.lm->pcg_max = k;
                }
                break;
            }
            const double alpha = rz / pap;
            for (int idx = tid; idx < nel; idx += PCG_THREADS) xv[idx] += alpha * pv[idx], rv[idx] -= alpha * apv[idx];
            __syncthreads();
            double dot = 0.0;
            for (int idx = tid; idx < nel; idx += PCG_THREADS)
            {
                const int lr = idx / 7, a = idx % 7;
                double z = 0.0;
#pragma unroll
                for (int b = 0; b < 7; ++b) z += Di[lr * 49 + a * 7 + b] * rv[lr * 7 + b];
                if (RES) zv[idx] = z;
                G.Z[(size_t)r0 * 7 + idx] = z;
                dot += rv[idx] * z;
            }
            dot = block_sum(dot, red);
            if (tid == 0) G.part_rz[((k + 1) & 1) * nwg + wg] = dot;
            if (!RES)
            {
                if (wg == 0 && tid == 0) G.lm->pcg_total += 1;
                return;
            }
        }
    }
    if (RES)
        for (int idx = tid; idx < nel; idx += PCG_THREADS) G.X[(size_t)r0 * 7 + idx] = xv[idx];
}

__global__ __launch_bounds__(256) void pgo_update_kernel(Dev G)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= G.n) return;
    double T[8], o[8], d[7];
#pragma unroll
    for (int k = 0; k < 8; ++k) T[k] = o[k] = G.pose[(size_t)v * 8 + k];
    const int row = G.rowof[v];
    if (row >= 0)
    {
#pragma unroll
        for (int a = 0; a < 7; ++a) d[a] = G.X[(size_t)row * 7 + a];
        pgo::retract(T, d, G.D, o);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) G.trial[(size_t)v * 8 + k] = o[k];
}

__global__ __launch_bounds__(256) void pgo_cost_kernel(Dev G, const double* poses)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= G.E) return;
    const int i = G.edges[2 * e], j = G.edges[2 * e + 1];
    double Ti[8], Tj[8], M[8], x[7];
#pragma unroll
    for (int k = 0; k < 8; ++k) Ti[k] = poses[(size_t)i * 8 + k], Tj[k] = poses[(size_t)j * 8 + k], M[k] = G.meas[(size_t)e * 8 + k];
    pgo::edge_log(Ti, Tj, M, x);
    const double w = G.weight[e];
    double s       = 0.0;
#pragma unroll
    for (int a = 0; a < 7; ++a)
    {
        const double r = a < G.D ? w * x[a] : 0.0;
        s += r * r;
    }
    G.r2[e] = s;
}

// mode 0: the cost of the start state (resets the LM record), 1: accept / reject of the trial state (the schedule of snk-ba v1), 2: snk_pgo_cost
__global__ __launch_bounds__(RED_THREADS) void pgo_decide_kernel(Dev G, int mode, double lambda_init, double min_delta)
{
    __shared__ double red[RED_THREADS];
    double s = 0.0;
    for (int e = threadIdx.x; e < G.E; e += RED_THREADS) s += G.r2[e];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = RED_THREADS / 2; w > 0; w >>= 1)
    {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double c = red[0];
    LmState& L     = *G.lm;
    if (mode == 2)
        L.cost_query = c;
    else if (mode == 0)
    {
        L.cost = L.cost_initial = L.cost_trial = c;
        L.lambda = lambda_init, L.v = 2.0, L.min_delta = min_delta;
        L.accepted_last = L.stop = L.lm_iterations = L.accepted_steps = L.pcg_total = L.pcg_done = L.pcg_max = 0;
    }
    else
    {
        L.cost_trial = c;
        L.lm_iterations += 1;
        if (c < L.cost)
        {
            const double dec = L.cost - c;
            L.cost           = c;
            L.lambda         = L.lambda * (1.0 / 3.0);
            L.v              = 2.0;
            L.accepted_last  = 1;
            L.accepted_steps += 1;
            if (dec < L.min_delta) L.stop = 1;
        }
        else
        {
            L.lambda *= L.v;
            L.v *= 2.0;
            L.accepted_last = 0;
        }
    }
}

__global__ __launch_bounds__(256) void pgo_commit_kernel(Dev G)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= (size_t)G.n * 8 || !G.lm->accepted_last) return;
    G.pose[k] = G.trial[k];
}

// point k moves by T = after[ref] . before[ref]^-1 as a Sim3: position s R x + t, normal R n, reference depth times s
__global__ __launch_bounds__(256) void pgo_transform_points_kernel(Dev G, int n_points, const int* ref, double* pos, double* normal, double* depth)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_points) return;
    const int v = ref[k];
    if (v < 0 || v >= G.n || G.constant[v]) return;
    double A[8], B[8], Bi[8], T[8], R[9];
#pragma unroll
    for (int c = 0; c < 8; ++c) A[c] = G.pose[(size_t)v * 8 + c], B[c] = G.before[(size_t)v * 8 + c];
    pgo::inv(B, Bi);
    pgo::mul(A, Bi, T);
    pgo::quat_R(T, R);
    const double x = pos[3 * k], y = pos[3 * k + 1], z = pos[3 * k + 2];
    for (int a = 0; a < 3; ++a) pos[3 * k + a] = T[7] * (R[a * 3] * x + R[a * 3 + 1] * y + R[a * 3 + 2] * z) + T[4 + a];
    if (normal)
    {
        const double nx = normal[3 * k], ny = normal[3 * k + 1], nz = normal[3 * k + 2];
        for (int a = 0; a < 3; ++a) normal[3 * k + a] = R[a * 3] * nx + R[a * 3 + 1] * ny + R[a * 3 + 2] * nz;
    }
    if (depth) depth[k] = depth[k] * T[7];
}

static int env_int(const char* name, int dflt)
{
    const char* s = getenv(name);
    return s && *s ? atoi(s) : dflt;
}
}  // namespace pgo_impl
}  // namespace snk

using namespace snk;
using namespace snk::pgo_impl;

struct snk_pgo : HandleBase
{
    snk_pgo_options opt{};
    Dev G{};
    bool have_graph = false, resident_ok = false;
    int last_form   = 0;  // 0 none, 1 resident, 2 launches
    size_t pcg_lds  = 0;
    int cus         = 0;
    DevBuf pose, trial, before, meas, weight, edges, rowof, rowvert, vstart, vlist, rbstart, rbedge, rbcol, wgstart, constant, Hii, Hij, Hjj, gi, gj, res,
        diag, grad, Dd, Dinv, Z, X, R, P, Ap, part, r2, bar, lm, pts;
    HostBuf rec;
};

namespace
{
template <typename T>
int upload(DevBuf& b, const std::vector<T>& v, hipStream_t st, size_t min_elems = 1)
{
    int rc = b.reserve(std::max(v.size(), min_elems) * sizeof(T));
    if (rc != SNK_OK) return rc;
    return copy_sync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st);
}

int read_record(snk_pgo* h, LmState* out)
{
    int rc = h->rec.reserve(sizeof(LmState));
    if (rc != SNK_OK) return rc;
    rc = copy_sync(h->rec.p, h->lm.p, sizeof(LmState), hipMemcpyDeviceToHost, h->stream);
    if (rc != SNK_OK) return rc;
    memcpy(out, h->rec.p, sizeof(LmState));
    return SNK_OK;
}

int launch_cost(snk_pgo* h, const double* poses, int mode)
{
    const Dev& G = h->G;
    if (G.E > 0)
    {
        hipLaunchKernelGGL(pgo_cost_kernel, dim3(ceil_div(G.E, 256)), dim3(256), 0, h->stream, G, poses);
        SNK_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(pgo_decide_kernel, dim3(1), dim3(RED_THREADS), 0, h->stream, G, mode, h->opt.lambda_init, h->opt.min_chi2_delta);
    SNK_LAUNCH_CHECK();
    return SNK_OK;
}

int launch_linearise(snk_pgo* h)
{
    const Dev& G = h->G;
    if (G.E > 0)
    {
        hipLaunchKernelGGL(pgo_linearise_kernel, dim3(ceil_div(G.E, LIN_THREADS)), dim3(LIN_THREADS), LIN_LDS, h->stream, G);
        SNK_LAUNCH_CHECK();
    }
    if (G.n > 0)
    {
        hipLaunchKernelGGL(pgo_assemble_kernel, dim3(ceil_div(G.n, 4)), dim3(256), 0, h->stream, G);
        SNK_LAUNCH_CHECK();
    }
    return SNK_OK;
}

int launch_pcg(snk_pgo* h)
{
    Dev& G = h->G;
    hipLaunchKernelGGL(pgo_damp_kernel, dim3(ceil_div(G.nrows, DAMP_THREADS)), dim3(DAMP_THREADS), DAMP_LDS, h->stream, G);
    SNK_LAUNCH_CHECK();
    SNK_HIP_CHECK(hipMemsetAsync(&G.lm->pcg_done, 0, sizeof(int), h->stream));
    bool resident = h->resident_ok && getenv("SNK_PGO_PCG_LAUNCHES") == nullptr;
    if (resident)
    {
        SNK_HIP_CHECK(hipMemsetAsync(G.bar, 0, sizeof(unsigned) * G.nwg, h->stream));
        int phase = -1, k = 0;
        void* args[] = {&G, &phase, &k};
        hipError_t e = hipLaunchCooperativeKernel(reinterpret_cast<const void*>(pgo_pcg_kernel<true>), dim3(G.nwg), dim3(PCG_THREADS), args, (unsigned)h->pcg_lds, h->stream);
        if (e != hipSuccess)
        {
            (void)hipGetLastError();  // a refused cooperative launch: the multi-launch form from here on
            h->resident_ok = resident = false;
        }
    }
    h->last_form = resident ? 1 : 2;
    if (resident) return SNK_OK;
    hipLaunchKernelGGL(pgo_pcg_kernel<false>, dim3(G.nwg), dim3(PCG_THREADS), 0, h->stream, G, 0, 0);
    SNK_LAUNCH_CHECK();
    for (int k = 0; k <= G.max_pcg; ++k)
    {
        hipLaunchKernelGGL(pgo_pcg_kernel<false>, dim3(G.nwg), dim3(PCG_THREADS), 0, h->stream, G, 1, k);
        hipLaunchKernelGGL(pgo_pcg_kernel<false>, dim3(G.nwg), dim3(PCG_THREADS), 0, h->stream, G, 2, k);
        SNK_LAUNCH_CHECK();
        if ((k & 31) == 31)  // one word per 32 iterations: stop issuing launches once the device has stopped
        {
            LmState L;
            int rc = read_record(h, &L);
            if (rc != SNK_OK) return rc;
            if (L.pcg_done) break;
        }
    }
    return SNK_OK;
}
}  // namespace

extern "C" {

int snk_pgo_create(const snk_pgo_options* options, int device, void* stream, snk_pgo** out)
{
    SNK_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    SNK_REQUIRE(options != nullptr, "options is NULL");
    SNK_REQUIRE(options->max_iterations >= 0 && options->max_pcg_iterations >= 0, "negative iteration count");
    SNK_REQUIRE(options->pcg_tol >= 0.0 && options->min_chi2_delta >= 0.0 && options->lambda_init > 0.0, "pcg_tol / min_chi2_delta / lambda_init out of range");
    snk_pgo* h = new snk_pgo();
    h->opt     = *options;
    int rc     = h->init(device, stream);
    if (rc == SNK_OK) rc = h->lm.reserve(sizeof(LmState));
    if (rc == SNK_OK) rc = set_max_lds_once(reinterpret_cast<const void*>(pgo_linearise_kernel), LIN_LDS);
    if (rc == SNK_OK) rc = set_max_lds_once(reinterpret_cast<const void*>(pgo_pcg_kernel<true>), PCG_LDS_CAP);
    hipDeviceProp_t prop;
    if (rc == SNK_OK && hipGetDeviceProperties(&prop, device) == hipSuccess) h->cus = prop.multiProcessorCount;
    if (rc != SNK_OK)
    {
        h->lm.release();
        h->fini();
        delete h;
        return rc;
    }
    *out = h;
    return SNK_OK;
}

int snk_pgo_destroy(snk_pgo* h)
{
    if (!h) return SNK_OK;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    DevBuf* all[] = {&h->pose, &h->trial, &h->before, &h->meas, &h->weight, &h->edges, &h->rowof, &h->rowvert, &h->vstart, &h->vlist, &h->rbstart, &h->rbedge,
                     &h->rbcol, &h->wgstart, &h->constant, &h->Hii, &h->Hij, &h->Hjj, &h->gi, &h->gj, &h->res, &h->diag, &h->grad, &h->Dd, &h->Dinv, &h->Z,
                     &h->X, &h->R, &h->P, &h->Ap, &h->part, &h->r2, &h->bar, &h->lm, &h->pts};
    for (DevBuf* b : all) b->release();
    h->rec.release();
    h->fini();
    delete h;
    return SNK_OK;
}

int snk_pgo_set_graph(snk_pgo* h, int n_vertices, const double (*poses_measure)[8], const double (*poses_init)[8], const uint8_t* constant, int n_edges,
                      const int32_t (*edges)[2], const double* weights, const double (*measurements)[8], int fix_scale)
{
    SNK_REQUIRE(h != nullptr, "handle is NULL");
    SNK_REQUIRE(n_vertices >= 0 && n_edges >= 0, "negative count");
    SNK_REQUIRE(n_vertices <= SNK_PGO_MAX_VERTICES && n_edges <= SNK_PGO_MAX_EDGES, "more vertices or edges than SNK_PGO_MAX_VERTICES / SNK_PGO_MAX_EDGES");
    SNK_REQUIRE(n_vertices == 0 || (poses_measure != nullptr && constant != nullptr), "poses_measure or constant is NULL");
    SNK_REQUIRE(n_edges == 0 || edges != nullptr, "edges is NULL");
    SNK_REQUIRE(fix_scale == 0 || fix_scale == 1, "fix_scale must be 0 or 1");
    const int n = n_vertices, E = n_edges;
    for (int v = 0; v < n; ++v)
        for (int pass = 0; pass < 2; ++pass)
        {
            const double* T = pass == 0 ? poses_measure[v] : poses_init ? poses_init[v] : poses_measure[v];
            for (int k = 0; k < 8; ++k) SNK_REQUIRE(std::isfinite(T[k]), "a pose is not finite");
            if (fix_scale)
                SNK_REQUIRE(T[7] == 1.0, "fix_scale is set but a vertex has a scale other than 1");
            else
                SNK_REQUIRE(T[7] > 0.0, "a vertex has a scale that is not > 0");
        }
    for (int e = 0; e < E; ++e)
    {
        const int i = edges[e][0], j = edges[e][1];
        SNK_REQUIRE(i >= 0 && j >= 0 && i < n && j < n, "an edge index is out of range");
        SNK_REQUIRE(i < j, "an edge does not have i < j");
        if (e > 0)
        {
            const int pi = edges[e - 1][0], pj = edges[e - 1][1];
            SNK_REQUIRE(!(pi == i && pj == j), "duplicate edge");
            SNK_REQUIRE(pi < i || (pi == i && pj < j), "edges are not sorted");
        }
        if (weights) SNK_REQUIRE(std::isfinite(weights[e]), "an edge weight is not finite");
        if (measurements)
        {
            for (int k = 0; k < 8; ++k) SNK_REQUIRE(std::isfinite(measurements[e][k]), "a measurement is not finite");
            SNK_REQUIRE(fix_scale ? measurements[e][7] == 1.0 : measurements[e][7] > 0.0, "a measurement's scale does not fit fix_scale");
        }
    }
    SNK_HIP_CHECK(hipSetDevice(h->device));
    h->have_graph = false;  // from here on the handle's buffers change: a HIP failure below leaves it without a graph

    // host side of ConstructPGO's result: measurements, the incident-edge lists (CSR, edge order), the rows of the free vertices, their
    // off-diagonal block lists and the partition of the rows over workgroups
    std::vector<double> pm((size_t)n * 8), ps((size_t)n * 8), ms((size_t)E * 8), ws(E);
    for (int v = 0; v < n; ++v)
        for (int k = 0; k < 8; ++k) pm[(size_t)v * 8 + k] = poses_measure[v][k], ps[(size_t)v * 8 + k] = (poses_init ? poses_init : poses_measure)[v][k];
    std::vector<int> ed((size_t)E * 2), deg(n, 0), vstart(n + 1, 0), rowof(n, -1), rowvert;
    for (int e = 0; e < E; ++e)
    {
        const int i = edges[e][0], j = edges[e][1];
        ed[2 * e] = i, ed[2 * e + 1] = j;
        ws[e] = weights ? weights[e] : 1.0;
        if (measurements)
            for (int k = 0; k < 8; ++k) ms[(size_t)e * 8 + k] = measurements[e][k];
        else
        {
            double a[8];
            pgo::inv(poses_measure[i], a);
            pgo::mul(a, poses_measure[j], &ms[(size_t)e * 8]);
        }
        ++deg[i], ++deg[j];
    }
    for (int v = 0; v < n; ++v) vstart[v + 1] = vstart[v] + deg[v];
    std::vector<int> vlist((size_t)2 * E), fill(vstart.begin(), vstart.end() - 1);
    for (int e = 0; e < E; ++e) vlist[fill[ed[2 * e]]++] = e * 2, vlist[fill[ed[2 * e + 1]]++] = e * 2 + 1;
    for (int v = 0; v < n; ++v)
        if (!constant[v] && deg[v] > 0) rowof[v] = (int)rowvert.size(), rowvert.push_back(v);  // a free vertex without edges keeps its pose
    const int nrows = (int)rowvert.size();
    std::vector<int> rbstart(nrows + 1, 0), rbedge, rbcol;
    for (int r = 0; r < nrows; ++r)
    {
        const int v = rowvert[r];
        for (int k = vstart[v]; k < vstart[v + 1]; ++k)
        {
            const int e = vlist[k] >> 1, side = vlist[k] & 1, other = rowof[ed[2 * e + (side ^ 1)]];
            if (other < 0) continue;
            rbedge.push_back(e * 2 + side);  // side 1: this row is j, the block is (J_i^T J_j)^T
            rbcol.push_back(other);
        }
        rbstart[r + 1] = (int)rbedge.size();
    }
    // partition: contiguous rows per workgroup while they fit the LDS; SNK_PGO_ROWS_PER_WG forces the row count (tests)
    const int rows_forced = env_int("SNK_PGO_ROWS_PER_WG", 0);
    const int rows_target = rows_forced > 0 ? rows_forced : std::max(8, ceil_div(std::max(nrows, 1), std::max(h->cus, 1)));
    auto lds_bytes        = [](long long R, long long NB) { return (size_t)((NB + 2 * R) * 49 + 5 * R * 7) * 8; };
    std::vector<int> wgstart{0};
    bool fits = true;
    size_t lds_max = 0;
    for (int r = 0; r < nrows;)
    {
        int R = 0;
        long long NB = 0;
        while (r + R < nrows && R < rows_target)
        {
            const long long nb = rbstart[r + R + 1] - rbstart[r + R];
            if (R > 0 && lds_bytes(R + 1, NB + nb) > (size_t)PCG_LDS_CAP) break;
            ++R, NB += nb;
        }
        if (lds_bytes(R, NB) > (size_t)PCG_LDS_CAP) fits = false;  // a single row of too high a degree: the multi-launch form
        lds_max = std::max(lds_max, lds_bytes(R, NB));
        r += R;
        wgstart.push_back(r);
    }
    const int nwg = (int)wgstart.size() - 1;

    hipStream_t st = h->stream;
    int rc;
    std::vector<uint8_t> cst(constant, constant + n);
#define UP(buf, vec)                                        \
    if ((rc = upload(h->buf, vec, st)) != SNK_OK) return rc
    UP(pose, ps);
    UP(before, pm);
    UP(meas, ms);
    UP(weight, ws);
    UP(edges, ed);
    UP(rowof, rowof);
    UP(rowvert, rowvert);
    UP(vstart, vstart);
    UP(vlist, vlist);
    UP(rbstart, rbstart);
    UP(rbedge, rbedge);
    UP(rbcol, rbcol);
    UP(wgstart, wgstart);
    UP(constant, cst);
#undef UP
    struct
    {
        DevBuf* b;
        size_t bytes;
    } scratch[] = {{&h->trial, (size_t)n * 64},   {&h->Hii, (size_t)E * 392},  {&h->Hij, (size_t)E * 392},  {&h->Hjj, (size_t)E * 392},
                   {&h->gi, (size_t)E * 56},      {&h->gj, (size_t)E * 56},    {&h->res, (size_t)E * 56},   {&h->diag, (size_t)n * 392},
                   {&h->grad, (size_t)n * 56},    {&h->Dd, (size_t)nrows * 392}, {&h->Dinv, (size_t)nrows * 392}, {&h->Z, (size_t)nrows * 56},
                   {&h->X, (size_t)nrows * 56},   {&h->R, (size_t)nrows * 56}, {&h->P, (size_t)nrows * 56}, {&h->Ap, (size_t)nrows * 56},
                   {&h->part, (size_t)std::max(nwg, 1) * 4 * 8}, {&h->r2, (size_t)E * 8}, {&h->bar, (size_t)std::max(nwg, 1) * 4}};
    for (auto& s : scratch)
        if ((rc = s.b->reserve(std::max<size_t>(s.bytes, 8))) != SNK_OK) return rc;

    Dev& G = h->G;
    G.n = n, G.E = E, G.D = fix_scale ? 6 : 7, G.nrows = nrows, G.nwg = nwg, G.max_pcg = h->opt.max_pcg_iterations, G.pcg_tol = h->opt.pcg_tol;
    G.pose = h->pose.as<double>(), G.trial = h->trial.as<double>(), G.before = h->before.as<double>(), G.meas = h->meas.as<double>();
    G.weight = h->weight.as<double>(), G.edges = h->edges.as<int>(), G.rowof = h->rowof.as<int>(), G.rowvert = h->rowvert.as<int>();
    G.vstart = h->vstart.as<int>(), G.vlist = h->vlist.as<int>(), G.rbstart = h->rbstart.as<int>(), G.rbedge = h->rbedge.as<int>();
    G.rbcol = h->rbcol.as<int>(), G.wgstart = h->wgstart.as<int>(), G.constant = h->constant.as<unsigned char>();
    G.Hii = h->Hii.as<double>(), G.Hij = h->Hij.as<double>(), G.Hjj = h->Hjj.as<double>(), G.gi = h->gi.as<double>(), G.gj = h->gj.as<double>();
    G.res = h->res.as<double>(), G.diag = h->diag.as<double>(), G.grad = h->grad.as<double>(), G.Dd = h->Dd.as<double>(), G.Dinv = h->Dinv.as<double>();
    G.Z = h->Z.as<double>(), G.X = h->X.as<double>(), G.R = h->R.as<double>(), G.P = h->P.as<double>(), G.Ap = h->Ap.as<double>();
    G.part_pap = h->part.as<double>(), G.part_rz = G.part_pap + std::max(nwg, 1), G.part_rz0 = G.part_pap + 3 * std::max(nwg, 1);
    G.r2 = h->r2.as<double>(), G.bar = h->bar.as<unsigned>(), G.lm = h->lm.as<LmState>();

    h->pcg_lds     = lds_max;
    h->resident_ok = false;
    h->last_form   = 0;
    if (fits && nwg > 0)
    {
        int resident = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, reinterpret_cast<const void*>(pgo_pcg_kernel<true>), PCG_THREADS, lds_max) == hipSuccess &&
            resident >= 1 && (long long)resident * h->cus >= nwg)
            h->resident_ok = true;
        else
            (void)hipGetLastError();
    }
    h->have_graph = true;
    return SNK_OK;
}

int snk_pgo_solve(snk_pgo* h, snk_pgo_result* result)
{
    SNK_REQUIRE(h != nullptr && result != nullptr, "handle or result is NULL");
    SNK_REQUIRE(h->have_graph, "snk_pgo_set_graph has not succeeded on this handle");
    SNK_HIP_CHECK(hipSetDevice(h->device));
    Dev& G = h->G;
    int rc = launch_cost(h, G.pose, 0);
    if (rc != SNK_OK) return rc;
    LmState L;
    bool need_lin = true;
    for (int it = 0; G.nrows > 0 && it < h->opt.max_iterations; ++it)
    {
        if (need_lin && (rc = launch_linearise(h)) != SNK_OK) return rc;
        if ((rc = launch_pcg(h)) != SNK_OK) return rc;
        hipLaunchKernelGGL(pgo_update_kernel, dim3(ceil_div(G.n, 256)), dim3(256), 0, h->stream, G);
        SNK_LAUNCH_CHECK();
        if ((rc = launch_cost(h, G.trial, 1)) != SNK_OK) return rc;
        hipLaunchKernelGGL(pgo_commit_kernel, dim3(ceil_div(G.n * 8, 256)), dim3(256), 0, h->stream, G);
        SNK_LAUNCH_CHECK();
        if ((rc = read_record(h, &L)) != SNK_OK) return rc;
        need_lin = L.accepted_last != 0;
        if (L.stop) break;
    }
    if ((rc = read_record(h, &L)) != SNK_OK) return rc;
    result->cost_initial         = L.cost_initial;
    result->cost_final           = L.cost;
    result->lm_iterations        = L.lm_iterations;
    result->pcg_iterations_total = L.pcg_total;
    result->accepted_steps       = L.accepted_steps;
    result->pcg_iterations_max   = L.pcg_max;
    result->pcg_form             = h->last_form;
    result->workgroups           = h->last_form ? G.nwg : 0;
    return SNK_OK;
}

int snk_pgo_get_poses(snk_pgo* h, double (*poses)[8])
{
    SNK_REQUIRE(h != nullptr && h->have_graph, "no graph on this handle");
    SNK_REQUIRE(h->G.n == 0 || poses != nullptr, "poses is NULL");
    SNK_HIP_CHECK(hipSetDevice(h->device));
    return copy_sync(poses, h->G.pose, (size_t)h->G.n * 64, hipMemcpyDeviceToHost, h->stream);
}

int snk_pgo_cost(snk_pgo* h, double* cost)
{
    SNK_REQUIRE(h != nullptr && h->have_graph && cost != nullptr, "no graph on this handle or cost is NULL");
    SNK_HIP_CHECK(hipSetDevice(h->device));
    int rc = launch_cost(h, h->G.pose, 2);
    if (rc != SNK_OK) return rc;
    LmState L;
    if ((rc = read_record(h, &L)) != SNK_OK) return rc;
    *cost = L.cost_query;
    return SNK_OK;
}

int snk_pgo_debug_linearisation(snk_pgo* h, double (*residuals)[7], double (*gradient)[7], double (*diag)[49])
{
    SNK_REQUIRE(h != nullptr && h->have_graph, "no graph on this handle");
    SNK_HIP_CHECK(hipSetDevice(h->device));
    const Dev& G = h->G;
    int rc = launch_linearise(h);
    if (rc != SNK_OK) return rc;
    if (residuals && (rc = copy_sync(residuals, G.res, (size_t)G.E * 56, hipMemcpyDeviceToHost, h->stream)) != SNK_OK) return rc;
    if (gradient && (rc = copy_sync(gradient, G.grad, (size_t)G.n * 56, hipMemcpyDeviceToHost, h->stream)) != SNK_OK) return rc;
    if (diag && (rc = copy_sync(diag, G.diag, (size_t)G.n * 392, hipMemcpyDeviceToHost, h->stream)) != SNK_OK) return rc;
    SNK_HIP_CHECK(hipStreamSynchronize(h->stream));
    return SNK_OK;
}

int snk_pgo_transform_points(snk_pgo* h, int n_points, const int32_t* ref_vertex, double (*positions)[3], double (*normals)[3], double* reference_depth)
{
    SNK_REQUIRE(h != nullptr && h->have_graph, "no graph on this handle");
    SNK_REQUIRE(n_points >= 0, "negative count");
    if (n_points == 0) return SNK_OK;
    SNK_REQUIRE(ref_vertex != nullptr && positions != nullptr, "ref_vertex or positions is NULL");
    for (int k = 0; k < n_points; ++k) SNK_REQUIRE(ref_vertex[k] >= -1 && ref_vertex[k] < h->G.n, "a reference vertex is out of range");
    SNK_HIP_CHECK(hipSetDevice(h->device));
    const size_t N = (size_t)n_points;
    int rc = h->pts.reserve(N * (4 + 24 + 24 + 8) + 64);
    if (rc != SNK_OK) return rc;
    char* base  = h->pts.as<char>();
    double* pos = reinterpret_cast<double*>(base);
    double* nrm = pos + 3 * N;
    double* dep = nrm + 3 * N;
    int* ref    = reinterpret_cast<int*>(dep + N);
    hipStream_t st = h->stream;
    if ((rc = copy_sync(pos, positions, N * 24, hipMemcpyHostToDevice, st)) != SNK_OK) return rc;
    if (normals && (rc = copy_sync(nrm, normals, N * 24, hipMemcpyHostToDevice, st)) != SNK_OK) return rc;
    if (reference_depth && (rc = copy_sync(dep, reference_depth, N * 8, hipMemcpyHostToDevice, st)) != SNK_OK) return rc;
    if ((rc = copy_sync(ref, ref_vertex, N * 4, hipMemcpyHostToDevice, st)) != SNK_OK) return rc;
    hipLaunchKernelGGL(pgo_transform_points_kernel, dim3(ceil_div(n_points, 256)), dim3(256), 0, st, h->G, n_points, ref, pos, normals ? nrm : nullptr,
                       reference_depth ? dep : nullptr);
    SNK_LAUNCH_CHECK();
    if ((rc = copy_sync(positions, pos, N * 24, hipMemcpyDeviceToHost, st)) != SNK_OK) return rc;
    if (normals && (rc = copy_sync(normals, nrm, N * 24, hipMemcpyDeviceToHost, st)) != SNK_OK) return rc;
    if (reference_depth && (rc = copy_sync(reference_depth, dep, N * 8, hipMemcpyDeviceToHost, st)) != SNK_OK) return rc;
    return SNK_OK;
}

}  // extern "C"
