// "snk-tri v1": the geometric loop of Triangulator::triangulate for ONE matched pair (reference
// Snake/LocalMapping/Triangulator.cpp:174-291), as a function of plain values so that the kernel (triangulate.hip) and a CPU
// build (a debugger, a host-side check) run the same statements.  The reference's mixed types are kept: the cosines and thParall
// are float, chi2 = float * float, ratioFactor and ratioOctave float, ratioDist double ("snk-tri v1").
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define SNK_TRI_HD __host__ __device__ __forceinline__
#else
#define SNK_TRI_HD inline
#endif

namespace snk
{
// One keyframe as the loop reads it: world -> camera rotation (row-major) and translation, camera centre.
struct TriPose
{
    double R[9], t[3], c[3];
};

struct TriConst
{
    double fx, fy, cx, cy, bf;
    double th_depth;
    float chi2_mono, chi2_stereo;  // errorMono^2, errorStereo^2 (:127-128)
    float ratio_factor;            // 1.5f * scalePyramid.Factor() (:132)
};

// One side of a pair: the undistorted keypoint, right_points[idx], depth[idx] and level_scale[octave].
struct TriFeature
{
    double x, y;
    float ur, depth, scale;
};

enum
{
    TRI_REJECT      = 0,
    TRI_TRIANGULATE = 1,  // :215-221
    TRI_STEREO1     = 2,  // :222-226
    TRI_STEREO2     = 3   // :227-231
};

// The right singular vector of the smallest singular value of the 4 x 4 matrix A (rows = equations), by one-sided (Hestenes)
// Jacobi: plane rotations from the right make the columns of A V orthogonal, their norms are the singular values and the
// column of V under the shortest one is the answer.  Works on A itself -- forming A^T A squares the condition number, and the
// far points this is used for have sigma_3 / sigma_1 down to 1e-4.  Fixed sweep count, statically indexed, no memory.
constexpr int TRI_JACOBI_SWEEPS = 8;

SNK_TRI_HD void tri_null_vector(double (&A)[4][4], double (&v)[4])
{
    double V[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < TRI_JACOBI_SWEEPS; ++sweep)
    {
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q)
            {
                double alpha = 0, beta = 0, gamma = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                {
                    alpha += A[i][p] * A[i][p];
                    beta += A[i][q] * A[i][q];
                    gamma += A[i][p] * A[i][q];
                }
                // tan of the rotation angle: the smaller root of t^2 + 2 zeta t - 1 = 0; gamma = 0 (columns orthogonal already, or
                // one of them zero) rotates by nothing
                const double zeta = (beta - alpha) / (2.0 * gamma);
                double t          = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                t                 = (gamma == 0.0 || !(t == t)) ? 0.0 : t;
                const double c    = 1.0 / sqrt(1.0 + t * t);
                const double s    = c * t;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                {
                    const double ap = A[i][p], aq = A[i][q];
                    A[i][p] = c * ap - s * aq;
                    A[i][q] = s * ap + c * aq;
                    const double vp = V[i][p], vq = V[i][q];
                    V[i][p] = c * vp - s * vq;
                    V[i][q] = s * vp + c * vq;
                }
            }
    }
    double best = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
        double nj = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) nj += A[i][j] * A[i][j];
        const bool take = j == 0 || nj < best;
        best            = take ? nj : best;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = take ? V[i][j] : v[i];
    }
}

// Saiga::TriangulateHomogeneous<double, true>(pose1, pose2, p1, p2) [DEFINED]: rows x P_3 - P_1, y P_3 - P_2 of both views with
// P = [R | t], each scaled to unit length; smallest right singular vector, dehomogenised.
SNK_TRI_HD void tri_homogeneous(const TriPose& P1, const TriPose& P2, double x1, double y1, double x2, double y2, double (&X)[3])
{
    double A[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
    {
        const TriPose& P = k < 2 ? P1 : P2;
        const double m   = k == 0 ? x1 : (k == 1 ? y1 : (k == 2 ? x2 : y2));
        const int row    = (k & 1) * 3;  // P_1 for the x equation, P_2 for the y equation
        double r[4];
#pragma unroll
        for (int j = 0; j < 3; ++j) r[j] = m * P.R[6 + j] - P.R[row + j];
        r[3]            = m * P.t[2] - P.t[k & 1];
        const double nr = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]);
#pragma unroll
        for (int j = 0; j < 4; ++j) A[k][j] = r[j] / nr;
    }
    double v[4];
    tri_null_vector(A, v);
#pragma unroll
    for (int j = 0; j < 3; ++j) X[j] = v[j] / v[3];
}

SNK_TRI_HD void tri_to_camera(const TriPose& P, const double (&X)[3], double (&xc)[3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) xc[i] = P.R[3 * i] * X[0] + P.R[3 * i + 1] * X[1] + P.R[3 * i + 2] * X[2] + P.t[i];
}

// pose.inverse() * v
SNK_TRI_HD void tri_to_world(const TriPose& P, const double (&v)[3], double (&X)[3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) X[i] = P.R[i] * v[0] + P.R[3 + i] * v[1] + P.R[6 + i] * v[2] + P.c[i];
}

// cos(2 atan2(b / 2, d)) of :204 / :206 as (d^2 - a^2) / (d^2 + a^2), a = b / 2: the same value to an ulp of double without the
// two transcendental calls (and without their scratch arrays on the device); rounded to float as the reference's assignment does.
SNK_TRI_HD float tri_cos_parallax_stereo(double baseline, float depth)
{
    const double a = baseline / 2, d = (double)depth;
    return (float)((d * d - a * a) / (d * d + a * a));
}

// the chi-square gate of one view (:246-272); true = the pair survives
SNK_TRI_HD bool tri_reprojection_ok(const TriConst& K, const TriFeature& f, bool stereo, const double (&xc)[3])
{
    const float sigma2 = f.scale * f.scale;  // SquaredScale(octave) [DEFINED]
    const double u = K.fx * xc[0] / xc[2] + K.cx, v = K.fy * xc[1] / xc[2] + K.cy;
    const double ex = u - f.x, ey = v - f.y;
    if (stereo)
    {
        const double er = (u - K.bf / xc[2]) - (double)f.ur;  // projectStereo(X) [DEFINED] = (u, v, u - bf / z)
        return !(ex * ex + ey * ey + er * er > (double)(K.chi2_stereo * sigma2));
    }
    return !(ex * ex + ey * ey > (double)(K.chi2_mono * sigma2));
}

// Returns the branch taken (TRI_REJECT = the pair yields no point); X and far_away are set for the others.
SNK_TRI_HD int tri_pair(const TriConst& K, const TriPose& P1, const TriPose& P2, const TriFeature& f1, const TriFeature& f2, double (&X)[3],
                        bool& far_away)
{
    const bool st1 = f1.ur >= 0, st2 = f2.ur >= 0;
    const double baseline = K.bf / K.fx;  // stereo_cam.baseLine() [DEFINED]
    // K.unproject(p, 1), rotated into the world
    const double xn1[3] = {(f1.x - K.cx) / K.fx, (f1.y - K.cy) / K.fy, 1.0};
    const double xn2[3] = {(f2.x - K.cx) / K.fx, (f2.y - K.cy) / K.fy, 1.0};
    double r1[3], r2[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
    {
        r1[i] = P1.R[i] * xn1[0] + P1.R[3 + i] * xn1[1] + P1.R[6 + i] * xn1[2];
        r2[i] = P2.R[i] * xn2[0] + P2.R[3 + i] * xn2[1] + P2.R[6 + i] * xn2[2];
    }
    const double dot = r1[0] * r2[0] + r1[1] * r2[1] + r1[2] * r2[2];
    const double n1  = sqrt(r1[0] * r1[0] + r1[1] * r1[1] + r1[2] * r1[2]);
    const double n2  = sqrt(r2[0] * r2[0] + r2[1] * r2[1] + r2[2] * r2[2]);
    const float cos_rays = (float)(dot / (n1 * n2));
    float cos_stereo     = cos_rays + 1;
    float cos_stereo1 = cos_stereo, cos_stereo2 = cos_stereo;
    if (st1)
        cos_stereo1 = tri_cos_parallax_stereo(baseline, f1.depth);
    else if (st2)
        cos_stereo2 = tri_cos_parallax_stereo(baseline, f2.depth);
    cos_stereo = cos_stereo1 < cos_stereo2 ? cos_stereo1 : cos_stereo2;
    const float th_parall = 0.9998f;
    far_away              = false;
    int branch;
    if (cos_rays < cos_stereo && cos_rays > 0 && (st1 || st2 || cos_rays < th_parall))
    {
        tri_homogeneous(P1, P2, xn1[0], xn1[1], xn2[0], xn2[1], X);
        branch = TRI_TRIANGULATE;
    }
    else if (st1 && cos_stereo1 < cos_stereo2)
    {
        const double z = (double)f1.depth, v[3] = {xn1[0] * z, xn1[1] * z, z};
        tri_to_world(P1, v, X);
        far_away = z > K.th_depth;
        branch   = TRI_STEREO1;
    }
    else if (st2 && cos_stereo2 < cos_stereo1)
    {
        const double z = (double)f2.depth, v[3] = {xn2[0] * z, xn2[1] * z, z};
        tri_to_world(P2, v, X);
        far_away = z > K.th_depth;
        branch   = TRI_STEREO2;
    }
    else
        return TRI_REJECT;
    double xc1[3], xc2[3];
    tri_to_camera(P1, X, xc1);
    tri_to_camera(P2, X, xc2);
    if (!(xc1[2] > 0) || !(xc2[2] > 0)) return TRI_REJECT;  // behind a camera (or not a number: a degenerate system)
    if (!tri_reprojection_ok(K, f1, st1, xc1)) return TRI_REJECT;
    if (!tri_reprojection_ok(K, f2, st2, xc2)) return TRI_REJECT;
    const double d1[3] = {P1.c[0] - X[0], P1.c[1] - X[1], P1.c[2] - X[2]};
    const double d2[3] = {P2.c[0] - X[0], P2.c[1] - X[1], P2.c[2] - X[2]};
    const double dist1 = sqrt(d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2]);
    const double dist2 = sqrt(d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2]);
    if (dist1 == 0 || dist2 == 0) return TRI_REJECT;
    const double ratio_dist  = dist2 / dist1;
    const float ratio_octave = f1.scale / f2.scale;
    if (ratio_dist * (double)K.ratio_factor < (double)ratio_octave || ratio_dist > (double)(ratio_octave * K.ratio_factor)) return TRI_REJECT;
    return branch;
}
}  // namespace snk
