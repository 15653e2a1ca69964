// CPU build of p3p_core.hpp (tests/test_p3p_core_cpu.py): runs the sampler and the solver on the pairs in <dir> (wps.bin, nips.bin,
// params.bin: iterations, seed, problem as doubles) and writes triplets, slot masks and poses of every hypothesis.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "p3p_core.hpp"

template <typename T>
static std::vector<T> read_all(const std::string& path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error("p3p_core_driver: missing input " + path);
    const std::streamsize bytes = f.tellg();
    f.seekg(0);
    std::vector<T> v((size_t)bytes / sizeof(T));
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
    return v;
}

int main(int argc, char** argv)
{
    try
    {
        const std::string dir = argc > 1 ? argv[1] : ".";
        const auto wps = read_all<double>(dir + "/wps.bin"), nips = read_all<double>(dir + "/nips.bin"), par = read_all<double>(dir + "/params.bin");
        const int n = (int)(wps.size() / 3), iterations = (int)par.at(0);
        const uint32_t key = snk::p3p_problem_key((uint64_t)par.at(1), (uint32_t)par.at(2));
        std::vector<int> tri((size_t)iterations * 3), valid((size_t)iterations);
        std::vector<double> poses((size_t)iterations * 4 * 12, 0.0);
        for (int k = 0; k < iterations; ++k)
        {
            int idx[3];
            snk::p3p_triplet(key, (uint32_t)k, (uint32_t)n, idx);
            double X[3][3], uv[3][2];
            for (int j = 0; j < 3; ++j)
            {
                tri[(size_t)k * 3 + j] = idx[j];
                for (int a = 0; a < 3; ++a) X[j][a] = wps[(size_t)idx[j] * 3 + a];
                for (int a = 0; a < 2; ++a) uv[j][a] = nips[(size_t)idx[j] * 2 + a];
            }
            snk::P3PSolutions S;
            snk::p3p_solve(X, uv, S);
            valid[(size_t)k] = S.valid;
            for (int s = 0; s < 4; ++s)
                if ((S.valid >> s) & 1)
                {
                    for (int j = 0; j < 9; ++j) poses[((size_t)k * 4 + s) * 12 + j] = S.R[s][j];
                    for (int j = 0; j < 3; ++j) poses[((size_t)k * 4 + s) * 12 + 9 + j] = S.t[s][j];
                }
        }
        std::ofstream(dir + "/out_tri.bin", std::ios::binary).write(reinterpret_cast<const char*>(tri.data()), (std::streamsize)(tri.size() * 4));
        std::ofstream(dir + "/out_valid.bin", std::ios::binary).write(reinterpret_cast<const char*>(valid.data()), (std::streamsize)(valid.size() * 4));
        std::ofstream(dir + "/out_poses.bin", std::ios::binary).write(reinterpret_cast<const char*>(poses.data()), (std::streamsize)(poses.size() * 8));
        return 0;
    }
    catch (const std::exception& e)
    {
        std::cerr << e.what() << "\n";
        return 1;
    }
}
