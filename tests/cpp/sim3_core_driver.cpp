// CPU build of sim3_core.hpp (tests/test_sim3_core_cpu.py): runs the sampler, the solver and the per-pair test on the pairs in <dir>
// (p1.bin, p2.bin: n x 3 doubles; ip1.bin, ip2.bin: n x 2 doubles; params.bin: iterations, seed, problem, compute_scale, threshold,
// fx, fy, cx, cy as doubles) and writes triplets, valid flags, transforms (qx qy qz qw tx ty tz s) and inlier counts of every
// hypothesis, plus the iteration count of n = 0 .. 2048 under (0.999, 15, 100).
#include <cstdio>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "sim3_core.hpp"

template <typename T>
static std::vector<T> read_all(const std::string& path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error("sim3_core_driver: missing input " + path);
    const std::streamsize bytes = f.tellg();
    f.seekg(0);
    std::vector<T> v((size_t)bytes / sizeof(T));
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
    return v;
}

template <typename T>
static void write_all(const std::string& path, const std::vector<T>& v)
{
    std::ofstream(path, std::ios::binary).write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

int main(int argc, char** argv)
{
    try
    {
        const std::string dir = argc > 1 ? argv[1] : ".";
        const auto p1 = read_all<double>(dir + "/p1.bin"), p2 = read_all<double>(dir + "/p2.bin");
        const auto ip1 = read_all<double>(dir + "/ip1.bin"), ip2 = read_all<double>(dir + "/ip2.bin"), par = read_all<double>(dir + "/params.bin");
        const int n = (int)(p1.size() / 3), iterations = (int)par.at(0);
        const uint32_t key      = snk::p3p_problem_key((uint64_t)par.at(1), (uint32_t)par.at(2));
        const bool scale        = par.at(3) != 0.0;
        const double threshold  = par.at(4);
        const snk::Sim3Camera K = {par.at(5), par.at(6), par.at(7), par.at(8)};
        std::vector<int> tri((size_t)iterations * 3), valid((size_t)iterations), counts((size_t)iterations, 0);
        std::vector<double> T((size_t)iterations * 8, 0.0);
        for (int k = 0; k < iterations; ++k)
        {
            int idx[3];
            snk::p3p_triplet(key, (uint32_t)k, (uint32_t)n, idx);
            double A[3][3], B[3][3];
            for (int j = 0; j < 3; ++j)
            {
                tri[(size_t)k * 3 + j] = idx[j];
                for (int a = 0; a < 3; ++a)
                {
                    A[j][a] = p1[(size_t)idx[j] * 3 + a];
                    B[j][a] = p2[(size_t)idx[j] * 3 + a];
                }
            }
            double q[4], R[9], t[3], s = 0.0, sR[9];
            valid[(size_t)k] = snk::sim3_solve(A, B, scale, q, R, t, s) ? 1 : 0;
            if (!valid[(size_t)k]) continue;
            for (int j = 0; j < 9; ++j) sR[j] = s * R[j];
            for (int j = 0; j < 4; ++j) T[(size_t)k * 8 + j] = q[j];
            for (int j = 0; j < 3; ++j) T[(size_t)k * 8 + 4 + j] = t[j];
            T[(size_t)k * 8 + 7] = s;
            for (int i = 0; i < n; ++i)
            {
                const double P1[3] = {p1[(size_t)i * 3], p1[(size_t)i * 3 + 1], p1[(size_t)i * 3 + 2]};
                const double P2[3] = {p2[(size_t)i * 3], p2[(size_t)i * 3 + 1], p2[(size_t)i * 3 + 2]};
                counts[(size_t)k] += snk::sim3_inlier(sR, R, t, P1, P2, ip1[(size_t)i * 2], ip1[(size_t)i * 2 + 1], ip2[(size_t)i * 2],
                                                      ip2[(size_t)i * 2 + 1], K, threshold)
                                         ? 1
                                         : 0;
            }
        }
        std::vector<int> its(2049);
        for (int i = 0; i <= 2048; ++i) its[(size_t)i] = snk::sim3_ransac_iterations(i, 0.999, 15, 100);
        write_all(dir + "/out_tri.bin", tri);
        write_all(dir + "/out_valid.bin", valid);
        write_all(dir + "/out_T.bin", T);
        write_all(dir + "/out_counts.bin", counts);
        write_all(dir + "/out_its.bin", its);
        return 0;
    }
    catch (const std::exception& e)
    {
        std::cerr << e.what() << "\n";
        return 1;
    }
}
