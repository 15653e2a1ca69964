// Driver of tests/test_cpp_p3p_gpu.py: snake_hip::P3PRansac::solve on the pairs found in <dir> (wps.bin: n x 3 doubles, nips.bin:
// n x 2 doubles, params.bin: iterations, threshold, seed as three doubles), results written back as out_pose.bin (7 doubles),
// out_mask.bin (n bytes), out_matches.bin (int32) and out_meta.bin (inliers, best iteration, best solution as int32).
#include <array>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "snake_hip.hpp"

template <typename T>
static std::vector<T> read_all(const std::string& path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error("p3p_driver: missing input " + path);
    const std::streamsize bytes = f.tellg();
    f.seekg(0);
    std::vector<T> v((size_t)bytes / sizeof(T));
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
    return v;
}

template <typename T>
static void write_all(const std::string& path, const T* data, size_t n)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(data), (std::streamsize)(n * sizeof(T)));
}

int main(int argc, char** argv)
{
    try
    {
        const std::string dir = argc > 1 ? argv[1] : ".";
        const auto wps    = read_all<std::array<double, 3>>(dir + "/wps.bin");
        const auto nips   = read_all<std::array<double, 2>>(dir + "/nips.bin");
        const auto params = read_all<double>(dir + "/params.bin");
        if (params.size() != 3) throw std::runtime_error("p3p_driver: params.bin must hold three doubles");
        snake_hip::RansacParameters rp;
        rp.maxIterations     = (int)params[0];
        rp.residualThreshold = params[1];
        rp.seed              = (uint64_t)params[2];
        snake_hip::P3PRansac pnp2(rp);
        double pose[7] = {0, 0, 0, 1, 0, 0, 0};
        std::vector<int> inlierMatches;
        std::vector<char> inlierMask;
        const int inliers = pnp2.solve(wps, nips, pose, inlierMatches, inlierMask);
        const int32_t meta[3] = {inliers, pnp2.best_iteration, pnp2.best_solution};
        write_all(dir + "/out_pose.bin", pose, 7);
        write_all(dir + "/out_mask.bin", inlierMask.data(), inlierMask.size());
        write_all(dir + "/out_matches.bin", inlierMatches.data(), inlierMatches.size());
        write_all(dir + "/out_meta.bin", meta, 3);
        std::printf("p3p_driver: %d inliers of %zu pairs\n", inliers, wps.size());
        return 0;
    }
    catch (const std::exception& e)
    {
        std::cerr << e.what() << "\n";
        return 1;
    }
}
