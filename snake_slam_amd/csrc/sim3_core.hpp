// "snk-sim3 v1": the iteration count, the minimal solver and the per-pair test of the 3-point registration RANSAC of
// LoopDetector::solve (reference Snake/LoopClosing/LoopDetector.cpp:148-206; the arithmetic of RegistrationRANSAC lives in the absent
// saiga and is [DEFINED] in DESIGN.md section 3e), as functions of plain values so that the kernel (sim3.hip) and a CPU build run the
// same statements.  The sampler is the one of "snk-p3p v1" (p3p_core.hpp: p3p_problem_key, p3p_triplet), included, not copied.  The
// solver uses + - * / and sqrt only, each its own IEEE operation (the file is built without contraction); the per-pair test is the
// one place with explicit fma().
#pragma once
#include "p3p_core.hpp"

namespace snk
{
constexpr int SIM3_NEWTON_STEPS = 50;  // cap of the Newton iteration on the characteristic quartic

// RansacIterationsFromProbability(N, 0.999, 15, 100) of LoopDetector.cpp:203 (the function is in saiga): host only, the kernel looks
// the count up in a table filled by this function
inline int sim3_ransac_iterations(int n, double probability, int min_inliers, int max_iterations)
{
    if (n <= 0) return 1;
    const double eps = (double)min_inliers / (double)n;
    if (eps >= 1.0) return 1;
    const double den = std::log(1.0 - eps * eps * eps);
    if (!(den < 0.0)) return max_iterations;  // eps^3 below the resolution of 1: more iterations than any cap
    const double its = std::ceil(std::log(1.0 - probability) / den);
    if (!(its < (double)max_iterations)) return max_iterations;
    return its < 1.0 ? 1 : (int)its;
}

// determinant and adjugate of a 4 x 4 matrix from the twelve 2 x 2 minors of its upper and lower row pairs
SNK_P3P_HD double sim3_det_adj4(const double (&a)[4][4], double (&b)[4][4])
{
    const double s0 = a[0][0] * a[1][1] - a[1][0] * a[0][1];
    const double s1 = a[0][0] * a[1][2] - a[1][0] * a[0][2];
    const double s2 = a[0][0] * a[1][3] - a[1][0] * a[0][3];
    const double s3 = a[0][1] * a[1][2] - a[1][1] * a[0][2];
    const double s4 = a[0][1] * a[1][3] - a[1][1] * a[0][3];
    const double s5 = a[0][2] * a[1][3] - a[1][2] * a[0][3];
    const double c5 = a[2][2] * a[3][3] - a[3][2] * a[2][3];
    const double c4 = a[2][1] * a[3][3] - a[3][1] * a[2][3];
    const double c3 = a[2][1] * a[3][2] - a[3][1] * a[2][2];
    const double c2 = a[2][0] * a[3][3] - a[3][0] * a[2][3];
    const double c1 = a[2][0] * a[3][2] - a[3][0] * a[2][2];
    const double c0 = a[2][0] * a[3][1] - a[3][0] * a[2][1];
    b[0][0] = (a[1][1] * c5 - a[1][2] * c4) + a[1][3] * c3;
    b[0][1] = (a[0][2] * c4 - a[0][1] * c5) - a[0][3] * c3;
    b[0][2] = (a[3][1] * s5 - a[3][2] * s4) + a[3][3] * s3;
    b[0][3] = (a[2][2] * s4 - a[2][1] * s5) - a[2][3] * s3;
    b[1][0] = (a[1][2] * c2 - a[1][0] * c5) - a[1][3] * c1;
    b[1][1] = (a[0][0] * c5 - a[0][2] * c2) + a[0][3] * c1;
    b[1][2] = (a[3][2] * s2 - a[3][0] * s5) - a[3][3] * s1;
    b[1][3] = (a[2][0] * s5 - a[2][2] * s2) + a[2][3] * s1;
    b[2][0] = (a[1][0] * c4 - a[1][1] * c2) + a[1][3] * c0;
    b[2][1] = (a[0][1] * c2 - a[0][0] * c4) - a[0][3] * c0;
    b[2][2] = (a[3][0] * s4 - a[3][1] * s2) + a[3][3] * s0;
    b[2][3] = (a[2][1] * s2 - a[2][0] * s4) - a[2][3] * s0;
    b[3][0] = (a[1][1] * c1 - a[1][0] * c3) - a[1][2] * c0;
    b[3][1] = (a[0][0] * c3 - a[0][1] * c1) + a[0][2] * c0;
    b[3][2] = (a[3][1] * s1 - a[3][0] * s3) - a[3][2] * s0;
    b[3][3] = (a[2][0] * s3 - a[2][1] * s1) + a[2][2] * s0;
    return ((((s0 * c5 - s1 * c4) + s2 * c3) + s3 * c2) - s4 * c1) + s5 * c0;
}

// a squared side that is not > 0, or |cross|^2 <= 1e-18 (side12^2 side13^2): the rule of section 3d step 1
SNK_P3P_HD bool sim3_degenerate(const double (&P)[3][3])
{
    double d12[3], d13[3], d23[3], cx[3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
    {
        d12[j] = P[1][j] - P[0][j];
        d13[j] = P[2][j] - P[0][j];
        d23[j] = P[2][j] - P[1][j];
    }
    const double s12 = p3p_dot(d12, d12), s13 = p3p_dot(d13, d13), s23 = p3p_dot(d23, d23);
    p3p_cross(d12, d13, cx);
    if (!(s12 > 0.0 && s13 > 0.0 && s23 > 0.0)) return true;
    return !(p3p_dot(cx, cx) > 1e-18 * (s12 * s13));
}

// rotation matrix (row-major) of the quaternion x y z w as it is (no normalisation)
SNK_P3P_HD void sim3_quat_to_R(double x, double y, double z, double w, double (&R)[9])
{
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - z * w);       R[2] = 2.0 * (x * z + y * w);
    R[3] = 2.0 * (x * y + z * w);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - x * w);
    R[6] = 2.0 * (x * z - y * w);       R[7] = 2.0 * (y * z + x * w);       R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// `pose * wp` of LoopDetector.cpp:193-194: pose = qx qy qz qw tx ty tz (world -> camera)
SNK_P3P_HD void sim3_view_point(const double* pose, const double* wp, double (&P)[3])
{
    double R[9];
    sim3_quat_to_R(pose[0], pose[1], pose[2], pose[3], R);
#pragma unroll
    for (int r = 0; r < 3; ++r) P[r] = ((R[3 * r] * wp[0] + R[3 * r + 1] * wp[1]) + R[3 * r + 2] * wp[2]) + pose[4 + r];
}

// One hypothesis: A[i] = point i of keyframe 1, B[i] = its partner of keyframe 2, both in their camera frames.  Fills q (x y z w,
// w >= 0), R, t, s with B ~ s R A + t and returns whether the triplet gives a transform.
SNK_P3P_HD bool sim3_solve(const double (&A)[3][3], const double (&B)[3][3], bool compute_scale, double (&q)[4], double (&R)[9],
                           double (&t)[3], double& s)
{
    if (sim3_degenerate(A) || sim3_degenerate(B)) return false;
    double m1[3], m2[3], a[3][3], b[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
    {
        m1[j] = ((A[0][j] + A[1][j]) + A[2][j]) / 3.0;
        m2[j] = ((B[0][j] + B[1][j]) + B[2][j]) / 3.0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
        {
            a[i][j] = A[i][j] - m1[j];
            b[i][j] = B[i][j] - m2[j];
        }
    }
    double M[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) M[i][j] = (a[0][i] * b[0][j] + a[1][i] * b[1][j]) + a[2][i] * b[2][j];
    const double Ga = (p3p_dot(a[0], a[0]) + p3p_dot(a[1], a[1])) + p3p_dot(a[2], a[2]);
    const double Gb = (p3p_dot(b[0], b[0]) + p3p_dot(b[1], b[1])) + p3p_dot(b[2], b[2]);
    // Horn's symmetric traceless matrix, quaternion order w x y z
    double N[4][4];
    N[0][0] = (M[0][0] + M[1][1]) + M[2][2];
    N[1][1] = (M[0][0] - M[1][1]) - M[2][2];
    N[2][2] = (M[1][1] - M[0][0]) - M[2][2];
    N[3][3] = (M[2][2] - M[0][0]) - M[1][1];
    N[0][1] = N[1][0] = M[1][2] - M[2][1];
    N[0][2] = N[2][0] = M[2][0] - M[0][2];
    N[0][3] = N[3][0] = M[0][1] - M[1][0];
    N[1][2] = N[2][1] = M[0][1] + M[1][0];
    N[1][3] = N[3][1] = M[2][0] + M[0][2];
    N[2][3] = N[3][2] = M[1][2] + M[2][1];
    // its characteristic quartic l^4 + c2 l^2 + c1 l + c0 and Newton from the upper bound (Theobald's QCP)
    double adj[4][4], mx[3];
    const double c2 = -2.0 * ((((M[0][0] * M[0][0] + M[0][1] * M[0][1]) + M[0][2] * M[0][2]) +
                               ((M[1][0] * M[1][0] + M[1][1] * M[1][1]) + M[1][2] * M[1][2])) +
                              ((M[2][0] * M[2][0] + M[2][1] * M[2][1]) + M[2][2] * M[2][2]));
    p3p_cross(M[1], M[2], mx);
    const double c1 = -8.0 * p3p_dot(M[0], mx);
    const double c0 = sim3_det_adj4(N, adj);
    double lam      = 0.5 * (Ga + Gb);
#pragma unroll 1
    for (int it = 0; it < SIM3_NEWTON_STEPS; ++it)
    {
        const double l2 = lam * lam;
        const double f  = ((l2 + c2) * lam + c1) * lam + c0;
        const double df = (4.0 * l2 + 2.0 * c2) * lam + c1;
        const double ln = lam - f / df;
        if (ln == lam) break;
        lam = ln;
    }
    // the eigenvector: the column of adj(N - lam I) of largest squared norm, first on ties
#pragma unroll
    for (int i = 0; i < 4; ++i) N[i][i] = N[i][i] - lam;
    sim3_det_adj4(N, adj);
    double best = -1.0, v[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
        const double nn = ((adj[0][j] * adj[0][j] + adj[1][j] * adj[1][j]) + adj[2][j] * adj[2][j]) + adj[3][j] * adj[3][j];
        if (j == 0 || nn > best)
        {
            best = nn;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = adj[i][j];
        }
    }
    if (!p3p_pos_finite(best)) return false;
    double nrm = std::sqrt(best);
    if (v[0] < 0.0) nrm = -nrm;
    const double w = v[0] / nrm, x = v[1] / nrm, y = v[2] / nrm, z = v[3] / nrm;
    sim3_quat_to_R(x, y, z, w, R);
    s = 1.0;
    if (compute_scale)
    {
        double num = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
        {
            double Ra[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) Ra[r] = (R[3 * r] * a[i][0] + R[3 * r + 1] * a[i][1]) + R[3 * r + 2] * a[i][2];
            const double d = p3p_dot(b[i], Ra);
            num            = i == 0 ? d : num + d;
        }
        s = num / Ga;
        if (!p3p_pos_finite(s)) return false;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) t[r] = m2[r] - s * ((R[3 * r] * m1[0] + R[3 * r + 1] * m1[1]) + R[3 * r + 2] * m1[2]);
    q[0] = x; q[1] = y; q[2] = z; q[3] = w;
    const double chk = (((x + y) + (z + w)) + ((t[0] + t[1]) + t[2]));
    return chk - chk == 0.0;  // every component finite
}

// ---- the per-pair test (section 3e "Scoring"): X = s R P1 + t against ip2, Y = R^T (P2 - t) against ip1 ----
struct Sim3Camera
{
    double fx, fy, cx, cy;
};

SNK_P3P_HD bool sim3_reprojects(double x, double y, double z, double u, double v, const Sim3Camera& K, double threshold)
{
    const double ex = std::fma(K.fx, x, (K.cx - u) * z), ey = std::fma(K.fy, y, (K.cy - v) * z);
    return z > 0.0 && std::fma(ey, ey, ex * ex) < threshold * (z * z);
}

// sR = s * R entry by entry
SNK_P3P_HD bool sim3_inlier(const double (&sR)[9], const double (&R)[9], const double (&t)[3], const double (&P1)[3], const double (&P2)[3],
                            double u1, double v1, double u2, double v2, const Sim3Camera& K, double threshold)
{
    const double X0 = std::fma(sR[0], P1[0], std::fma(sR[1], P1[1], std::fma(sR[2], P1[2], t[0])));
    const double X1 = std::fma(sR[3], P1[0], std::fma(sR[4], P1[1], std::fma(sR[5], P1[2], t[1])));
    const double X2 = std::fma(sR[6], P1[0], std::fma(sR[7], P1[1], std::fma(sR[8], P1[2], t[2])));
    const double d0 = P2[0] - t[0], d1 = P2[1] - t[1], d2 = P2[2] - t[2];
    const double Y0 = std::fma(R[0], d0, std::fma(R[3], d1, R[6] * d2));
    const double Y1 = std::fma(R[1], d0, std::fma(R[4], d1, R[7] * d2));
    const double Y2 = std::fma(R[2], d0, std::fma(R[5], d1, R[8] * d2));
    return sim3_reprojects(X0, X1, X2, u2, v2, K, threshold) && sim3_reprojects(Y0, Y1, Y2, u1, v1, K, threshold);
}

// tmpPose of LoopDetector.cpp:251-255,278: (R^T R2, R^T (t2 - t) / s) with pose2 = (R2, t2) world -> camera of the target keyframe
SNK_P3P_HD void sim3_corrected_pose(const double (&R)[9], const double (&t)[3], double s, const double* pose2, double (&out)[7])
{
    double R2[9], Rc[9], tc[3];
    sim3_quat_to_R(pose2[0], pose2[1], pose2[2], pose2[3], R2);
#pragma unroll
    for (int i = 0; i < 3; ++i)
    {
#pragma unroll
        for (int j = 0; j < 3; ++j) Rc[3 * i + j] = (R[i] * R2[j] + R[3 + i] * R2[3 + j]) + R[6 + i] * R2[6 + j];
        tc[i] = ((R[i] * (pose2[4] - t[0]) + R[3 + i] * (pose2[5] - t[1])) + R[6 + i] * (pose2[6] - t[2])) / s;
    }
    p3p_pose7(Rc, tc, out);
}
}  // namespace snk
