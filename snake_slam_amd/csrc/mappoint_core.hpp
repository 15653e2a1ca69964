// "snk-mp v1": the refresh of ONE map point after its observations or its position changed -- MapPoint::ComputeDistinctiveDescriptors,
// UpdateNormal and UpdateDepth (reference Snake/Map/MapPoint.cpp:60-81, :120-135, :154-166) -- as functions of plain values, so that
// the kernels (mappoint.hip) and a CPU build (tests/cpp/mappoint_core_driver.cpp, a debugger) run the same statements.
// Saiga::MeanMatcher and Eigen are absent: every rule below is [DEFINED].
//
//   observations   k of them in list order, each with a `valid` byte (= !isBad() of :71 and the operator bool of :127); invalid ones
//                  are skipped everywhere, N = number of valid ones
//   descriptor     d(i, j) = Hamming distance over the valid observations, d(i, i) = 0 included;
//                  MP_RULE_MEDIAN: m(i) = element (N - 1) / 2 of row i sorted ascending, MP_RULE_SUM: m(i) = sum of row i;
//                  best = the first valid i in list order with the smallest m(i); N = 0: best = -1, descriptor untouched
//   normal         C = -R^T t of the observing keyframe, v = C - p, s = (v.x v.x + v.y v.y) + v.z v.z, u = s > 0 ? v / sqrt(s) : v;
//                  normal = sum of u over the valid observations in list order, sequentially, normalised by the same rule; fp64,
//                  no contraction (the translation unit and the CPU driver are built with -ffp-contract=off)
//   depth          ref_depth = sqrt(s) of p - C_ref, ref_level = octave of observation ref_obs; ref_obs = -1: untouched (-1, 0)
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SNK_MP_HD __host__ __device__ __forceinline__
#else
#define SNK_MP_HD inline
#endif
#if defined(__clang__)
#define SNK_MP_NO_UNROLL _Pragma("unroll 1")
#define SNK_MP_UNROLL _Pragma("unroll")
#else
#define SNK_MP_NO_UNROLL
#define SNK_MP_UNROLL
#endif

namespace snk
{
constexpr int MP_MAX_OBS = 4096;  // observations of one point: 128 KB of descriptors in a workgroup's LDS
enum { MP_RULE_MEDIAN = 0, MP_RULE_SUM = 1 };
enum { MP_DESCRIPTOR = 1, MP_NORMAL = 2, MP_DEPTH = 4 };
enum { MP_OK = 0, MP_BAD_INDEX = 1, MP_TOO_MANY = 2 };
constexpr int MP_SELECT_STEPS = 9;  // halvings of [0, 256]: 257 -> 129 -> 65 -> 33 -> 17 -> 9 -> 5 -> 3 -> 2 -> 1 candidates

SNK_MP_HD int mp_hamming(const uint64_t a0, const uint64_t a1, const uint64_t a2, const uint64_t a3, const uint64_t* b)
{
    return __builtin_popcountll(a0 ^ b[0]) + __builtin_popcountll(a1 ^ b[1]) + __builtin_popcountll(a2 ^ b[2]) + __builtin_popcountll(a3 ^ b[3]);
}

// 1-based rank of the median among N values: the element at index (N - 1) / 2 of the sorted row
SNK_MP_HD int mp_rank(int N) { return (N - 1) / 2 + 1; }

// The element of rank `rank` of a row of distances in [0, 256] without sorting it: the smallest v with #{j : d(j) <= v} >= rank.
// count_le(v) counts the row.  Selects the same element as the sorted row.
template <typename CountLE>
SNK_MP_HD int mp_select(CountLE count_le, int rank)
{
    int lo = 0, hi = 256;
    SNK_MP_NO_UNROLL
    for (int step = 0; step < MP_SELECT_STEPS; ++step)
    {
        const int mid = (lo + hi) >> 1;
        if (count_le(mid) >= rank) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// The same element by eight-way narrowing, for a row that is too long to keep and has to be recomputed by every pass: count7(t, c) sets
// c[q] = #{j : d(j) <= t[q]} for seven thresholds at once, so three passes (257 -> 33 -> 5 -> 1 candidates) replace nine.
// Invariant: #{d <= lo - 1} < rank <= #{d <= hi}.  The thresholds cut [lo, hi] (n values) into eight parts of at most ceil(n / 8);
// the first part whose upper end reaches the rank holds the answer (an empty part repeats its neighbour's count and is never the first).
constexpr int MP_SELECT8_PASSES = 3;

template <typename Count7>
SNK_MP_HD int mp_select8(Count7 count7, int rank)
{
    int lo = 0, hi = 256;
    SNK_MP_NO_UNROLL
    for (int pass = 0; pass < MP_SELECT8_PASSES; ++pass)
    {
        const int n = hi - lo + 1;
        int t[7], c[7];
        SNK_MP_UNROLL
        for (int q = 0; q < 7; ++q) t[q] = lo + n * (q + 1) / 8 - 1;
        count7(t, c);
        int new_lo = t[6] + 1, new_hi = hi;  // the last part unless an earlier one reaches the rank
        SNK_MP_UNROLL
        for (int q = 6; q >= 0; --q)
            if (c[q] >= rank) new_hi = t[q], new_lo = q > 0 ? t[q - 1] + 1 : lo;
        lo = new_lo;
        hi = new_hi;
    }
    return lo;
}

// camera centre of a keyframe pose (qx qy qz qw tx ty tz, world -> camera): C = -R^T t  (Keyframe::CameraPosition, :128, :162)
SNK_MP_HD void mp_centre(const double* pose, double* C)
{
    const double x = pose[0], y = pose[1], z = pose[2], w = pose[3];
    const double tx = pose[4], ty = pose[5], tz = pose[6];
    const double r00 = 1 - 2 * (y * y + z * z), r01 = 2 * (x * y - z * w), r02 = 2 * (x * z + y * w);
    const double r10 = 2 * (x * y + z * w), r11 = 1 - 2 * (x * x + z * z), r12 = 2 * (y * z - x * w);
    const double r20 = 2 * (x * z - y * w), r21 = 2 * (y * z + x * w), r22 = 1 - 2 * (x * x + y * y);
    C[0] = -((r00 * tx + r10 * ty) + r20 * tz);
    C[1] = -((r01 * tx + r11 * ty) + r21 * tz);
    C[2] = -((r02 * tx + r12 * ty) + r22 * tz);
}

// u = normalized(v) by the rule above; returns s = |v|^2
SNK_MP_HD double mp_unit(const double* v, double* u)
{
    const double s = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    if (s > 0)
    {
        const double r = sqrt(s);
        u[0] = v[0] / r;
        u[1] = v[1] / r;
        u[2] = v[2] / r;
    }
    else
    {
        u[0] = v[0];
        u[1] = v[1];
        u[2] = v[2];
    }
    return s;
}

// (kfposition - position).normalized() of :130
SNK_MP_HD void mp_view_dir(const double* pose, const double* p, double* u)
{
    double C[3];
    mp_centre(pose, C);
    const double v[3] = {C[0] - p[0], C[1] - p[1], C[2] - p[2]};
    mp_unit(v, u);
}

// (position - referenceKF->CameraPosition()).norm() of :162
SNK_MP_HD double mp_ref_depth(const double* pose, const double* p)
{
    double C[3];
    mp_centre(pose, C);
    const double dx = p[0] - C[0], dy = p[1] - C[1], dz = p[2] - C[2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

// ---- the whole point on one thread: what the kernels compute, spelled as loops (host builds only use these) ----------------------
// best of :79 as an index into the full list (-1: no valid observation); *n_valid = N
// eight_way: select with mp_select8 (the wide kernel's way) instead of mp_select -- the same element either way
inline int mp_best_descriptor(const uint64_t (*desc)[4], const uint8_t* valid, int k, int rule, int* n_valid, bool eight_way = false)
{
    int N = 0;
    for (int j = 0; j < k; ++j) N += valid[j] ? 1 : 0;
    *n_valid = N;
    long long best_m = 0;
    int best = -1;
    for (int i = 0; i < k; ++i)
    {
        if (!valid[i]) continue;
        const uint64_t* a = desc[i];
        long long m;
        if (rule == MP_RULE_SUM)
        {
            m = 0;
            for (int j = 0; j < k; ++j)
                if (valid[j]) m += mp_hamming(a[0], a[1], a[2], a[3], desc[j]);
        }
        else if (eight_way)
            m = mp_select8(
                [&](const int (&t)[7], int (&c)[7]) {
                    for (int q = 0; q < 7; ++q) c[q] = 0;
                    for (int j = 0; j < k; ++j)
                    {
                        if (!valid[j]) continue;
                        const int d = mp_hamming(a[0], a[1], a[2], a[3], desc[j]);
                        for (int q = 0; q < 7; ++q) c[q] += d <= t[q] ? 1 : 0;
                    }
                },
                mp_rank(N));
        else
            m = mp_select(
                [&](int v) {
                    int c = 0;
                    for (int j = 0; j < k; ++j) c += valid[j] && mp_hamming(a[0], a[1], a[2], a[3], desc[j]) <= v ? 1 : 0;
                    return c;
                },
                mp_rank(N));
        if (best < 0 || m < best_m) best = i, best_m = m;
    }
    return best;
}

inline void mp_normal(const double (*pose)[7], const uint8_t* valid, int k, const double* p, double* normal)
{
    double acc[3] = {0, 0, 0};
    for (int j = 0; j < k; ++j)
    {
        if (!valid[j]) continue;
        double u[3];
        mp_view_dir(pose[j], p, u);
        acc[0] += u[0];
        acc[1] += u[1];
        acc[2] += u[2];
    }
    mp_unit(acc, normal);
}
}  // namespace snk
