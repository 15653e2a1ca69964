// "snk-p3p v1": the sampler, the minimal solver and the per-point test of the P3P-RANSAC step of Tracking::TrackBruteForce (reference
// Snake/Tracking/TrackingCoarse.cpp:403-440; the arithmetic of P3PRansac lives in the absent saiga and is [DEFINED] in DESIGN.md
// section 3d), as functions of plain values so that the kernel (p3p.hip) and a CPU build run the same statements.  Everything is
// statically indexed: a solution is a SLOT (2 * line + root), never an entry appended to a list, so the four poses of a hypothesis
// live in registers.  The solver uses + - * / and sqrt only, each its own IEEE operation (the file is built without contraction);
// the per-point test is the one place with explicit fma().
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SNK_P3P_HD __host__ __device__ __forceinline__
#else
#define SNK_P3P_HD inline
#endif

namespace snk
{
constexpr int P3P_SLOTS        = 4;    // two lines of the degenerate conic x two roots of the quadratic on each
constexpr int P3P_CUBIC_STEPS  = 100;  // cap of the bracketed Newton iteration on the cubic
constexpr int P3P_NEWTON_STEPS = 3;    // polish of the three depths on the three distance equations
constexpr int P3P_DRAW_LIMIT   = 32;   // counters tried per hypothesis before the deterministic fall-back

// ---- sampling: a counter-based integer hash, no floating point ----
SNK_P3P_HD uint32_t p3p_mix(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

SNK_P3P_HD uint32_t p3p_problem_key(uint64_t seed, uint32_t problem)
{
    uint32_t h = p3p_mix((uint32_t)seed ^ 0x9e3779b9u);
    h          = p3p_mix(h ^ (uint32_t)(seed >> 32));
    return p3p_mix(h ^ problem);
}

// draw `c` of hypothesis `k`: an index in [0, n) by multiply-high
SNK_P3P_HD uint32_t p3p_index(uint32_t key, uint32_t k, uint32_t c, uint32_t n)
{
    const uint32_t h = p3p_mix(p3p_mix(key ^ k) ^ c);
    return (uint32_t)(((uint64_t)h * (uint64_t)n) >> 32);
}

// three distinct indices (n >= 4): a draw that repeats an earlier index is taken again with the next counter; after P3P_DRAW_LIMIT
// counters the index walks upwards (mod n) to the first free one, so the function always ends
SNK_P3P_HD void p3p_triplet(uint32_t key, uint32_t k, uint32_t n, int (&idx)[3])
{
    uint32_t c  = 0;
    uint32_t i0 = p3p_index(key, k, c++, n);
    uint32_t i1 = p3p_index(key, k, c++, n);
    while (i1 == i0 && c < (uint32_t)P3P_DRAW_LIMIT) i1 = p3p_index(key, k, c++, n);
    if (i1 == i0) i1 = (i0 + 1) % n;
    uint32_t i2 = p3p_index(key, k, c++, n);
    while ((i2 == i0 || i2 == i1) && c < (uint32_t)P3P_DRAW_LIMIT) i2 = p3p_index(key, k, c++, n);
    while (i2 == i0 || i2 == i1) i2 = (i2 + 1) % n;
    idx[0] = (int)i0;
    idx[1] = (int)i1;
    idx[2] = (int)i2;
}

// ---- the minimal solver ----
struct P3PSolutions
{
    double R[P3P_SLOTS][9];  // world -> camera, row-major
    double t[P3P_SLOTS][3];
    int valid;               // bit s = slot s holds a pose
};

SNK_P3P_HD double p3p_dot(const double (&a)[3], const double (&b)[3])
{
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

SNK_P3P_HD void p3p_cross(const double (&a)[3], const double (&b)[3], double (&c)[3])
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// determinant of the matrix with COLUMNS j of A or B (bit j of `pick` set = column j from B)
SNK_P3P_HD double p3p_det_cols(const double (&A)[3][3], const double (&B)[3][3], int pick)
{
    double c[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) c[j][i] = ((pick >> j) & 1) ? B[i][j] : A[i][j];
    double x[3];
    p3p_cross(c[1], c[2], x);
    return p3p_dot(c[0], x);
}

SNK_P3P_HD double p3p_sel3(int i, double a0, double a1, double a2)
{
    return i == 0 ? a0 : (i == 1 ? a1 : a2);
}

SNK_P3P_HD bool p3p_pos_finite(double x)
{
    return x > 0.0 && x < INFINITY;  // false for NaN
}

// X[i] = world point i, uv[i] = its normalised image point.  Fills S and returns the number of poses (0..4).
SNK_P3P_HD int p3p_solve(const double (&X)[3][3], const double (&uv)[3][2], P3PSolutions& S)
{
    S.valid = 0;
    // unit bearings and their cosines
    double y[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
    {
        const double nrm = std::sqrt((uv[i][0] * uv[i][0] + uv[i][1] * uv[i][1]) + 1.0);
        y[i][0]          = uv[i][0] / nrm;
        y[i][1]          = uv[i][1] / nrm;
        y[i][2]          = 1.0 / nrm;
    }
    const double b12 = p3p_dot(y[0], y[1]), b13 = p3p_dot(y[0], y[2]), b23 = p3p_dot(y[1], y[2]);
    // the world triangle
    double d1[3], d2[3], d12[3], cx[3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
    {
        d1[j]  = X[1][j] - X[0][j];
        d2[j]  = X[2][j] - X[0][j];
        d12[j] = X[2][j] - X[1][j];
    }
    const double a12 = p3p_dot(d1, d1), a13 = p3p_dot(d2, d2), a23 = p3p_dot(d12, d12);
    p3p_cross(d1, d2, cx);
    const double det = p3p_dot(cx, cx);
    if (!(a12 > 0.0 && a13 > 0.0 && a23 > 0.0)) return 0;  // two world points coincide
    if (!(det > 1e-18 * (a12 * a13))) return 0;            // collinear world points: no frame to align
    // the two homogeneous conics in the depths: D1 = M12 a23 - M23 a12, D2 = M13 a23 - M23 a13
    double D1[3][3] = {{a23, -(a23 * b12), 0.0}, {-(a23 * b12), a23 - a12, a12 * b23}, {0.0, a12 * b23, -a12}};
    double D2[3][3] = {{a23, 0.0, -(a23 * b13)}, {0.0, -a13, a13 * b23}, {-(a23 * b13), a13 * b23, a23 - a13}};
    // det(D1 + g D2) = c3 g^3 + c2 g^2 + c1 g + c0
    double c0 = p3p_det_cols(D1, D2, 0);
    double c1 = (p3p_det_cols(D1, D2, 1) + p3p_det_cols(D1, D2, 2)) + p3p_det_cols(D1, D2, 4);
    double c2 = (p3p_det_cols(D1, D2, 6) + p3p_det_cols(D1, D2, 5)) + p3p_det_cols(D1, D2, 3);
    double c3 = p3p_det_cols(D1, D2, 7);
    if (std::fabs(c3) < std::fabs(c0))  // the better conditioned leading coefficient: exchange the conics, reverse the cubic
    {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j)
            {
                const double w = D1[i][j];
                D1[i][j]       = D2[i][j];
                D2[i][j]       = w;
            }
        double w = c0; c0 = c3; c3 = w;
        w = c1; c1 = c2; c2 = w;
    }
    if (!(std::fabs(c3) > 0.0)) return 0;  // both conics singular together
    const double pb = c2 / c3, pc = c1 / c3, pd = c0 / c3;
    // a real root of g^3 + pb g^2 + pc g + pd by Newton's method kept inside a bracket: [lo, hi] = the Cauchy bound, where the cubic
    // is negative at lo and positive at hi; every iterate moves the end of its sign, a Newton step that leaves the bracket (or is
    // not a number) is replaced by the midpoint; it stops when the iterate no longer changes.  Starts at the inflection point.
    const double bound = 1.0 + std::fmax(std::fabs(pb), std::fmax(std::fabs(pc), std::fabs(pd)));
    double lo = -bound, hi = bound, g = -pb / 3.0;
#pragma unroll 1
    for (int it = 0; it < P3P_CUBIC_STEPS; ++it)
    {
        const double f = ((g + pb) * g + pc) * g + pd;
        if (f > 0.0) hi = g;
        else lo = g;
        const double df = (3.0 * g + 2.0 * pb) * g + pc;
        double gn       = g - f / df;
        if (!(gn > lo && gn < hi)) gn = 0.5 * (lo + hi);
        if (gn == g) break;
        g = gn;
    }
    // D0 = D1 + g D2 is a pair of planes through the origin of depth space; Q = the conic of the pencil further from D0
    double D0[3][3], Q[3][3];
    const bool use2 = std::fabs(g) <= 1.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
        {
            D0[i][j] = D1[i][j] + g * D2[i][j];
            Q[i][j]  = use2 ? D2[i][j] : D1[i][j];
        }
    // B = -adj(D0) = p p^T with p the common point of the two planes
    double B[3][3];
    B[0][0] = -(D0[1][1] * D0[2][2] - D0[1][2] * D0[1][2]);
    B[0][1] = -(D0[0][2] * D0[1][2] - D0[0][1] * D0[2][2]);
    B[0][2] = -(D0[0][1] * D0[1][2] - D0[0][2] * D0[1][1]);
    B[1][1] = -(D0[0][0] * D0[2][2] - D0[0][2] * D0[0][2]);
    B[1][2] = -(D0[0][1] * D0[0][2] - D0[0][0] * D0[1][2]);
    B[2][2] = -(D0[0][0] * D0[1][1] - D0[0][1] * D0[0][1]);
    B[1][0] = B[0][1];
    B[2][0] = B[0][2];
    B[2][1] = B[1][2];
    int bi      = 0;
    double bmax = B[0][0];
    if (B[1][1] > bmax) { bmax = B[1][1]; bi = 1; }
    if (B[2][2] > bmax) { bmax = B[2][2]; bi = 2; }
    if (!(bmax > 0.0)) return 0;  // the planes are complex: no real depths on this root
    const double beta = std::sqrt(bmax);
    double p[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) p[j] = p3p_sel3(bi, B[0][j], B[1][j], B[2][j]) / beta;
    // N = D0 + [p]x has rank one: its rows are multiples of one plane, its columns of the other
    double N[3][3];
    N[0][0] = D0[0][0];        N[0][1] = D0[0][1] - p[2]; N[0][2] = D0[0][2] + p[1];
    N[1][0] = D0[1][0] + p[2]; N[1][1] = D0[1][1];        N[1][2] = D0[1][2] - p[0];
    N[2][0] = D0[2][0] - p[1]; N[2][1] = D0[2][1] + p[0]; N[2][2] = D0[2][2];
    int br = 0, bc = 0;
    double nmax = -1.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
        {
            const double v = std::fabs(N[i][j]);
            if (v > nmax) { nmax = v; br = i; bc = j; }
        }
    if (!(nmax > 0.0)) return 0;
    double line[2][3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
    {
        line[0][j] = p3p_sel3(br, N[0][j], N[1][j], N[2][j]);
        line[1][j] = p3p_sel3(bc, N[j][0], N[j][1], N[j][2]);
    }
    // what the pose needs of the world triangle: the rows of [d1 d2 cx]^-1
    double r1[3], r2[3], r3[3];
    p3p_cross(d2, cx, r1);
    p3p_cross(cx, d1, r2);
#pragma unroll
    for (int j = 0; j < 3; ++j)
    {
        r1[j] = r1[j] / det;
        r2[j] = r2[j] / det;
        r3[j] = cx[j] / det;
    }
    const double asum = (a12 + a13) + a23;
#pragma unroll
    for (int l = 0; l < 2; ++l)
    {
        // on the plane w . lambda = 0 the depth with the largest |w| is a combination of the other two: lambda = tau gv + hv
        const double w0 = line[l][0], w1 = line[l][1], w2 = line[l][2];
        int ia    = 0;
        double wm = std::fabs(w0);
        if (std::fabs(w1) > wm) { wm = std::fabs(w1); ia = 1; }
        if (std::fabs(w2) > wm) { wm = std::fabs(w2); ia = 2; }
        const int ib = ia == 2 ? 0 : ia + 1, ic = ia == 0 ? 2 : ia - 1;
        const double wa = p3p_sel3(ia, w0, w1, w2);
        const double sb = -p3p_sel3(ib, w0, w1, w2) / wa, sc = -p3p_sel3(ic, w0, w1, w2) / wa;
        double gv[3], hv[3], Qg[3], Qh[3];
#pragma unroll
        for (int j = 0; j < 3; ++j)
        {
            gv[j] = j == ia ? sb : (j == ib ? 1.0 : 0.0);
            hv[j] = j == ia ? sc : (j == ic ? 1.0 : 0.0);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
        {
            Qg[i] = p3p_dot(Q[i], gv);
            Qh[i] = p3p_dot(Q[i], hv);
        }
        const double qa = p3p_dot(gv, Qg), qb = p3p_dot(gv, Qh), qc = p3p_dot(hv, Qh);
        const double disc = qb * qb - qa * qc;
        if (!(disc >= 0.0)) continue;  // the plane misses the conic
        const double sq = std::sqrt(disc);
        const double qq = -(qb + (qb >= 0.0 ? sq : -sq));
#pragma unroll
        for (int r = 0; r < 2; ++r)
        {
            const int s      = 2 * l + r;
            const double tau = r == 0 ? qq / qa : qc / qq;
            if (!p3p_pos_finite(tau)) continue;  // a depth ratio must be positive
            double lam[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) lam[j] = tau * gv[j] + hv[j];
            if (!(lam[0] > 0.0 && lam[1] > 0.0 && lam[2] > 0.0)) continue;  // a point behind the camera
            const double den = 2.0 * p3p_dot(lam, lam) - 2.0 * ((b12 * (lam[0] * lam[1]) + b13 * (lam[0] * lam[2])) + b23 * (lam[1] * lam[2]));
            if (!(den > 0.0)) continue;
            const double rho = std::sqrt(asum / den);
#pragma unroll
            for (int j = 0; j < 3; ++j) lam[j] = rho * lam[j];
            // Newton on the three distance equations (Cramer's rule; a singular Jacobian skips the step)
#pragma unroll 1
            for (int it = 0; it < P3P_NEWTON_STEPS; ++it)
            {
                const double l0 = lam[0], l1 = lam[1], l2 = lam[2];
                const double e12 = ((l0 * l0 + l1 * l1) - 2.0 * b12 * (l0 * l1)) - a12;
                const double e13 = ((l0 * l0 + l2 * l2) - 2.0 * b13 * (l0 * l2)) - a13;
                const double e23 = ((l1 * l1 + l2 * l2) - 2.0 * b23 * (l1 * l2)) - a23;
                const double j00 = 2.0 * (l0 - b12 * l1), j01 = 2.0 * (l1 - b12 * l0);
                const double j10 = 2.0 * (l0 - b13 * l2), j12 = 2.0 * (l2 - b13 * l0);
                const double j21 = 2.0 * (l1 - b23 * l2), j22 = 2.0 * (l2 - b23 * l1);
                // J = [j00 j01 0; j10 0 j12; 0 j21 j22]
                const double dj = -(j00 * (j12 * j21)) - j01 * (j10 * j22);
                if (!(std::fabs(dj) > 0.0)) break;
                const double x0 = (-(j12 * j21) * e12 - (j01 * j22) * e13) + (j01 * j12) * e23;
                const double x1 = (-(j10 * j22) * e12 + (j00 * j22) * e13) - (j00 * j12) * e23;
                const double x2 = ((j10 * j21) * e12 - (j00 * j21) * e13) - (j01 * j10) * e23;
                lam[0] = l0 - x0 / dj;
                lam[1] = l1 - x1 / dj;
                lam[2] = l2 - x2 / dj;
            }
            if (!(p3p_pos_finite(lam[0]) && p3p_pos_finite(lam[1]) && p3p_pos_finite(lam[2]))) continue;
            // camera points, their frame, R = [e1 e2 e3] [d1 d2 cx]^-1, t = Y0 - R X0
            double e1[3], e2[3], e3[3], Y0[3];
#pragma unroll
            for (int j = 0; j < 3; ++j)
            {
                Y0[j] = lam[0] * y[0][j];
                e1[j] = lam[1] * y[1][j] - Y0[j];
                e2[j] = lam[2] * y[2][j] - Y0[j];
            }
            p3p_cross(e1, e2, e3);
#pragma unroll
            for (int i = 0; i < 3; ++i)
            {
#pragma unroll
                for (int j = 0; j < 3; ++j) S.R[s][3 * i + j] = (e1[i] * r1[j] + e2[i] * r2[j]) + e3[i] * r3[j];
                S.t[s][i] = Y0[i] - ((S.R[s][3 * i] * X[0][0] + S.R[s][3 * i + 1] * X[0][1]) + S.R[s][3 * i + 2] * X[0][2]);
            }
            S.valid |= 1 << s;
        }
    }
    int n = 0;
#pragma unroll
    for (int s = 0; s < P3P_SLOTS; ++s) n += (S.valid >> s) & 1;
    return n;
}

// ---- the per-point test: z_c > 0 and |p_c.xy / z_c - nip|^2 < threshold, multiplied through by z_c^2 (no division) ----
SNK_P3P_HD bool p3p_inlier(const double (&R)[9], const double (&t)[3], double X, double Y, double Z, double u, double v, double threshold)
{
    const double x = std::fma(R[0], X, std::fma(R[1], Y, std::fma(R[2], Z, t[0])));
    const double y = std::fma(R[3], X, std::fma(R[4], Y, std::fma(R[5], Z, t[1])));
    const double z = std::fma(R[6], X, std::fma(R[7], Y, std::fma(R[8], Z, t[2])));
    const double ex = std::fma(-u, z, x), ey = std::fma(-v, z, y);
    return z > 0.0 && std::fma(ey, ey, ex * ex) < threshold * (z * z);
}

// (R, t) -> qx qy qz qw tx ty tz, unit quaternion with qw >= 0 (Shepperd's choice of the largest of the four candidates)
SNK_P3P_HD void p3p_pose7(const double (&R)[9], const double (&t)[3], double (&pose)[7])
{
    const double tr = (R[0] + R[4]) + R[8];
    double x, y, z, w;
    if (tr > 0.0)
    {
        const double s = 2.0 * std::sqrt(tr + 1.0);
        w = 0.25 * s; x = (R[7] - R[5]) / s; y = (R[2] - R[6]) / s; z = (R[3] - R[1]) / s;
    }
    else if (R[0] > R[4] && R[0] > R[8])
    {
        const double s = 2.0 * std::sqrt(((1.0 + R[0]) - R[4]) - R[8]);
        w = (R[7] - R[5]) / s; x = 0.25 * s; y = (R[1] + R[3]) / s; z = (R[2] + R[6]) / s;
    }
    else if (R[4] > R[8])
    {
        const double s = 2.0 * std::sqrt(((1.0 + R[4]) - R[0]) - R[8]);
        w = (R[2] - R[6]) / s; x = (R[1] + R[3]) / s; y = 0.25 * s; z = (R[5] + R[7]) / s;
    }
    else
    {
        const double s = 2.0 * std::sqrt(((1.0 + R[8]) - R[0]) - R[4]);
        w = (R[3] - R[1]) / s; x = (R[2] + R[6]) / s; y = (R[5] + R[7]) / s; z = 0.25 * s;
    }
    const double nq = std::sqrt(((x * x + y * y) + z * z) + w * w);
    const double sg = w < 0.0 ? -nq : nq;
    pose[0] = x / sg; pose[1] = y / sg; pose[2] = z / sg; pose[3] = w / sg;
    pose[4] = t[0]; pose[5] = t[1]; pose[6] = t[2];
}
}  // namespace snk
