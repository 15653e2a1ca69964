// "snk-pgo v1" (DESIGN.md section 3f): the per-edge statements of the pose-graph optimiser -- logarithm / exponential of SE3 and Sim3,
// Ad, ad, the Bernoulli series of the inverse right Jacobian, residual + Jacobians and the block products.  One text for the kernels of
// pgo.hip, for the host side of snk_pgo_set_graph and for a plain g++ build (tests/cpp/pgo_core_driver.cpp), restated in numpy by
// tests/pgo_numpy.py with the same branches, thresholds and series orders.
//
// A pose is 8 doubles qx qy qz qw tx ty tz s acting as x -> s R x + t.  A tangent vector is 7 wide: translation, rotation, sigma = log s.
// The se3 form is the sim3 form at s = 1, sigma = 0 with row / column 6 dropped (D = 6): one code path.
//
// The three 7 x 7 work matrices of an edge are addressed through Mat<STRIDE>: element k of a matrix sits at p[k * STRIDE].  The host uses
// STRIDE = 1; the kernels put them in LDS interleaved by lane (STRIDE = threads of the workgroup), because 147 doubles per lane indexed
// by loop variables would otherwise live in scratch.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define PGO_HD __host__ __device__ __forceinline__
#else
#define PGO_HD inline
#endif

namespace pgo
{
constexpr double TH_THETA = 1e-2;  // below: series in theta for W's coefficients, the quaternion of exp and the angle of log
constexpr double TH_SIGMA = 1e-8;  // below: (e^sigma - 1) / sigma = 1 + sigma / 2
constexpr int G_TERMS     = 30;    // terms of g_n(sigma) = int_0^1 tau^n e^(tau sigma) dtau = sum_k sigma^k / (k! (n + k + 1))
constexpr int ORDER       = 10;    // J_r^-1(x) = sum_{n = 0..ORDER} B_n / n! (-ad_x)^n

PGO_HD double jr_coeff(int n)  // B_n / n!, B_1 = -1/2
{
    switch (n)
    {
        case 0: return 1.0;
        case 1: return -0.5;
        case 2: return 1.0 / 12.0;
        case 4: return -1.0 / 720.0;
        case 6: return 1.0 / 30240.0;
        case 8: return -1.0 / 1209600.0;
        case 10: return 1.0 / 47900160.0;
        default: return 0.0;
    }
}

template <int STRIDE>
struct Mat
{
    double* p;
    PGO_HD double& operator()(int a, int b) const { return p[(a * 7 + b) * STRIDE]; }
};

PGO_HD void quat_R(const double* q, double* R)
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1 - 2 * (y * y + z * z), R[1] = 2 * (x * y - z * w), R[2] = 2 * (x * z + y * w);
    R[3] = 2 * (x * y + z * w), R[4] = 1 - 2 * (x * x + z * z), R[5] = 2 * (y * z - x * w);
    R[6] = 2 * (x * z - y * w), R[7] = 2 * (y * z + x * w), R[8] = 1 - 2 * (x * x + y * y);
}

PGO_HD void qmul(const double* a, const double* b, double* o)
{
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
    o[2] = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}

// o = A . B (o may not alias A or B)
PGO_HD void mul(const double* A, const double* B, double* o)
{
    double R[9];
    quat_R(A, R);
    qmul(A, B, o);
#pragma unroll
    for (int a = 0; a < 3; ++a) o[4 + a] = A[7] * (R[a * 3] * B[4] + R[a * 3 + 1] * B[5] + R[a * 3 + 2] * B[6]) + A[4 + a];
    o[7] = A[7] * B[7];
}

PGO_HD void inv(const double* A, double* o)
{
    double R[9];
    o[0] = -A[0], o[1] = -A[1], o[2] = -A[2], o[3] = A[3];
    quat_R(o, R);
    const double si = 1.0 / A[7];
#pragma unroll
    for (int a = 0; a < 3; ++a) o[4 + a] = -si * (R[a * 3] * A[4] + R[a * 3 + 1] * A[5] + R[a * 3 + 2] * A[6]);
    o[7] = si;
}

PGO_HD double g_series(int n, double sigma)
{
    double s = 0.0, term = 1.0, fact = 1.0;
    for (int k = 0; k < G_TERMS; ++k)
    {
        if (k)
        {
            term = term * sigma;
            fact *= k;
        }
        s = s + term / (fact * (n + k + 1));
    }
    return s;
}

// W = C I + A [w]x + B [w]x^2 = int_0^1 e^(tau sigma) exp(tau [w]x) dtau: (e^z - 1) / z at z = sigma + i theta gives A = Im / theta,
// B = (C - Re) / theta^2, with e^z - 1 = P + i Q written without cancellation
PGO_HD void w_coeffs(double theta, double sigma, double& A, double& B, double& C)
{
    C = fabs(sigma) < TH_SIGMA ? 1.0 + 0.5 * sigma : expm1(sigma) / sigma;
    if (theta < TH_THETA)
    {
        const double t2 = theta * theta;
        A = g_series(1, sigma) - t2 * (g_series(3, sigma) / 6.0 - t2 * (g_series(5, sigma) / 120.0));
        B = g_series(2, sigma) / 2.0 - t2 * (g_series(4, sigma) / 24.0 - t2 * (g_series(6, sigma) / 720.0));
        return;
    }
    const double sh = sin(0.5 * theta);
    const double P = expm1(sigma) * cos(theta) - 2.0 * sh * sh, Q = exp(sigma) * sin(theta), c = sigma * sigma + theta * theta;
    A = (Q * sigma - P * theta) / (theta * c);
    B = (C - (P * sigma + Q * theta) / c) / (theta * theta);
}

PGO_HD void w_matrix(const double* om, double sigma, double* W)
{
    double A, B, C;
    w_coeffs(sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]), sigma, A, B, C);
    const double x = om[0], y = om[1], z = om[2];
    const double K[9]  = {0, -z, y, z, 0, -x, -y, x, 0};
    const double K2[9] = {-(y * y + z * z), x * y, x * z, x * y, -(x * x + z * z), y * z, x * z, y * z, -(x * x + y * y)};
#pragma unroll
    for (int k = 0; k < 9; ++k) W[k] = A * K[k] + B * K2[k];
    W[0] += C, W[4] += C, W[8] += C;
}

// x (upsilon, omega, sigma) -> pose
PGO_HD void exp7(const double* x, double* T)
{
    const double t2 = x[3] * x[3] + x[4] * x[4] + x[5] * x[5], theta = sqrt(t2);
    const double k = theta < TH_THETA ? 0.5 - t2 * (1.0 / 48.0 - t2 * (1.0 / 3840.0 - t2 / 645120.0)) : sin(0.5 * theta) / theta;
    T[0] = x[3] * k, T[1] = x[4] * k, T[2] = x[5] * k, T[3] = cos(0.5 * theta);
    double W[9];
    w_matrix(x + 3, x[6], W);
#pragma unroll
    for (int a = 0; a < 3; ++a) T[4 + a] = W[a * 3] * x[0] + W[a * 3 + 1] * x[1] + W[a * 3 + 2] * x[2];
    T[7] = exp(x[6]);
}

PGO_HD void inv3(const double* M, double* o)
{
    const double a = M[0], b = M[1], c = M[2], d = M[3], e = M[4], f = M[5], g = M[6], h = M[7], i = M[8];
    const double A = e * i - f * h, Bc = c * h - b * i, Cc = b * f - c * e;
    const double det = a * A + d * Bc + g * Cc;
    o[0] = A / det, o[1] = Bc / det, o[2] = Cc / det;
    o[3] = (f * g - d * i) / det, o[4] = (a * i - c * g) / det, o[5] = (c * d - a * f) / det;
    o[6] = (d * h - e * g) / det, o[7] = (b * g - a * h) / det, o[8] = (a * e - b * d) / det;
}

// pose -> x
PGO_HD void log7(const double* T, double* x)
{
    const double sg = T[3] < 0 ? -1.0 : 1.0;
    const double v0 = T[0] * sg, v1 = T[1] * sg, v2 = T[2] * sg, w = T[3] * sg;
    const double n2 = v0 * v0 + v1 * v1 + v2 * v2, n = sqrt(n2), x2 = n2 / (w * w);
    const double k = n < 0.5 * TH_THETA ? (2.0 / w) * (1.0 - x2 * (1.0 / 3.0 - x2 * (1.0 / 5.0 - x2 / 7.0))) : 2.0 * atan2(n, w) / n;
    x[3] = v0 * k, x[4] = v1 * k, x[5] = v2 * k;
    x[6] = log(T[7]);
    double W[9], Wi[9];
    w_matrix(x + 3, x[6], W);
    inv3(W, Wi);
#pragma unroll
    for (int a = 0; a < 3; ++a) x[a] = Wi[a * 3] * T[4] + Wi[a * 3 + 1] * T[5] + Wi[a * 3 + 2] * T[6];
}

// x = log(M^-1 . T_i^-1 . T_j): the unweighted residual of an edge
PGO_HD void edge_log(const double* Ti, const double* Tj, const double* M, double* x)
{
    double a[8], b[8], c[8];
    inv(Ti, a);
    mul(a, Tj, b);
    inv(M, a);
    mul(a, b, c);
    log7(c, x);
}

template <int STRIDE>
PGO_HD void set_zero(Mat<STRIDE> M)
{
    for (int k = 0; k < 49; ++k) M.p[k * STRIDE] = 0.0;
}

// N = -ad_x
template <int STRIDE>
PGO_HD void neg_ad(const double* x, Mat<STRIDE> N)
{
    set_zero(N);
    const double u0 = x[0], u1 = x[1], u2 = x[2], w0 = x[3], w1 = x[4], w2 = x[5], s = x[6];
    const double K[9] = {0, -w2, w1, w2, 0, -w0, -w1, w0, 0}, U[9] = {0, -u2, u1, u2, 0, -u0, -u1, u0, 0};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
        {
            N(a, b)         = -(K[a * 3 + b] + (a == b ? s : 0.0));
            N(a, 3 + b)     = -U[a * 3 + b];
            N(3 + a, 3 + b) = -K[a * 3 + b];
        }
    N(0, 6) = u0, N(1, 6) = u1, N(2, 6) = u2;
}

template <int STRIDE>
PGO_HD void adjoint(const double* T, Mat<STRIDE> A)
{
    set_zero(A);
    double R[9];
    quat_R(T, R);
    const double t0 = T[4], t1 = T[5], t2 = T[6];
    const double K[9] = {0, -t2, t1, t2, 0, -t0, -t1, t0, 0};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
        {
            A(a, b)         = T[7] * R[a * 3 + b];
            A(a, 3 + b)     = K[a * 3] * R[b] + K[a * 3 + 1] * R[3 + b] + K[a * 3 + 2] * R[6 + b];
            A(3 + a, 3 + b) = R[a * 3 + b];
        }
    A(0, 6) = -t0, A(1, 6) = -t1, A(2, 6) = -t2;
    A(6, 6) = 1.0;
}

// S = sum_n B_n / n! N^n with N = -ad_x in N; P is work space
template <int STRIDE>
PGO_HD void jr_inv(Mat<STRIDE> N, Mat<STRIDE> P, Mat<STRIDE> S)
{
    for (int a = 0; a < 7; ++a)
        for (int b = 0; b < 7; ++b) P(a, b) = a == b ? 1.0 : 0.0, S(a, b) = a == b ? jr_coeff(0) : 0.0;
    for (int n = 1; n <= ORDER; ++n)
    {
        const double c = jr_coeff(n);
        for (int a = 0; a < 7; ++a)  // row a of P <- row a of P times N
        {
            double row[7];
#pragma unroll
            for (int b = 0; b < 7; ++b) row[b] = 0.0;
            for (int k = 0; k < 7; ++k)
            {
                const double pk = P(a, k);
#pragma unroll
                for (int b = 0; b < 7; ++b) row[b] += pk * N(k, b);
            }
#pragma unroll
            for (int b = 0; b < 7; ++b)
            {
                P(a, b) = row[b];
                if (c != 0.0) S(a, b) = S(a, b) + c * row[b];
            }
        }
    }
}

// The residual r[7] = weight x (entries >= D zero) and the Jacobians of an edge: J_j = weight J_r^-1(x) ends in S, J_i = -J_j Ad(T_j^-1 T_i)
// in P; N is work space.  Rows and columns >= D are zero.
template <int STRIDE>
PGO_HD void edge_jacobians(const double* Ti, const double* Tj, const double* M, double weight, int D, double* r, Mat<STRIDE> N, Mat<STRIDE> P,
                           Mat<STRIDE> S)
{
    double x[7];
    edge_log(Ti, Tj, M, x);
#pragma unroll
    for (int a = 0; a < 7; ++a) r[a] = a < D ? weight * x[a] : 0.0;
    neg_ad(x, N);
    jr_inv(N, P, S);
    double a8[8], b8[8];
    inv(Tj, a8);
    mul(a8, Ti, b8);
    adjoint(b8, N);
    for (int a = 0; a < 7; ++a)
    {
        double row[7];
#pragma unroll
        for (int b = 0; b < 7; ++b) row[b] = 0.0;
        for (int k = 0; k < 7; ++k)
        {
            const double sk = weight * S(a, k);
            S(a, k)         = a < D && k < D ? sk : 0.0;
#pragma unroll
            for (int b = 0; b < 7; ++b) row[b] += sk * N(k, b);
        }
#pragma unroll
        for (int b = 0; b < 7; ++b) P(a, b) = a < D && b < D ? -row[b] : 0.0;
    }
}

// out[a * 7 + b] = sum_k A(k, a) B(k, b)
template <int STRIDE>
PGO_HD void at_b(Mat<STRIDE> A, Mat<STRIDE> B, double* out)
{
    for (int a = 0; a < 7; ++a)
    {
        double row[7];
#pragma unroll
        for (int b = 0; b < 7; ++b) row[b] = 0.0;
        for (int k = 0; k < 7; ++k)
        {
            const double ak = A(k, a);
#pragma unroll
            for (int b = 0; b < 7; ++b) row[b] += ak * B(k, b);
        }
#pragma unroll
        for (int b = 0; b < 7; ++b) out[a * 7 + b] = row[b];
    }
}

// out[a] = sum_k A(k, a) r[k]
template <int STRIDE>
PGO_HD void at_r(Mat<STRIDE> A, const double* r, double* out)
{
#pragma unroll
    for (int a = 0; a < 7; ++a)
    {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 7; ++k) s += A(k, a) * r[k];
        out[a] = s;
    }
}

// T <- T . exp(delta), quaternion renormalised; the se3 form keeps s = 1 exactly
PGO_HD void retract(const double* T, const double* delta, int D, double* o)
{
    double x[7], E[8];
#pragma unroll
    for (int a = 0; a < 7; ++a) x[a] = a < D ? delta[a] : 0.0;
    exp7(x, E);
    mul(T, E, o);
    const double n = sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2] + o[3] * o[3]);
    o[0] /= n, o[1] /= n, o[2] /= n, o[3] /= n;
    if (D == 6) o[7] = 1.0;
}
}  // namespace pgo
