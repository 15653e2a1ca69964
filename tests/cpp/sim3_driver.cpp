// Driver of tests/test_cpp_sim3_gpu.py: snake_hip::RegistrationRansac filled and called as LoopDetector::solve does
// (Snake/LoopClosing/LoopDetector.cpp:152-205) on the pairs found in <dir> (p1.bin, p2.bin: n x 3 doubles; ip1.bin, ip2.bin: n x 2
// doubles; params.bin: iterations (0 = RansacIterationsFromProbability), compute_scale, threshold, seed, fx, fy, cx, cy as doubles),
// results written back as out_T.bin (qx qy qz qw tx ty tz scale), out_mask.bin (n bytes) and out_meta.bin (inliers, best iteration,
// iterations used as int32).
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
    if (!f) throw std::runtime_error("sim3_driver: missing input " + path);
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
        const auto p1     = read_all<std::array<double, 3>>(dir + "/p1.bin");
        const auto p2     = read_all<std::array<double, 3>>(dir + "/p2.bin");
        const auto ip1    = read_all<std::array<double, 2>>(dir + "/ip1.bin");
        const auto ip2    = read_all<std::array<double, 2>>(dir + "/ip2.bin");
        const auto params = read_all<double>(dir + "/params.bin");
        if (params.size() != 8) throw std::runtime_error("sim3_driver: params.bin must hold eight doubles");
        snake_hip::RegistrationRansac solver;
        solver.clear();
        solver.threshold = params[2];
        solver.seed      = (uint64_t)params[3];
        solver.camera1   = snk_camera{params[4], params[5], params[6], params[7], 0.0};
        solver.camera2   = solver.camera1;
        for (size_t i = 0; i < p1.size(); ++i)
        {
            solver.ips1.push_back(ip1.at(i));
            solver.ips2.push_back(ip2.at(i));
            solver.points1.push_back(snake_hip::RegistrationRansac::transform(solver.pose1, p1[i]));  // identity poses: the points as they are
            solver.points2.push_back(snake_hip::RegistrationRansac::transform(solver.pose2, p2.at(i)));
            solver.N++;
        }
        const int its = params[0] > 0 ? (int)params[0] : snake_hip::RansacIterationsFromProbability(solver.N, 0.999, 15, 100);
        auto [T, scale, nInliers] = solver.solve(its, params[1] != 0.0);
        double out[8];
        for (int j = 0; j < 7; ++j) out[j] = T[(size_t)j];
        out[7] = scale;
        const int32_t meta[3] = {nInliers, solver.best_iteration, its};
        write_all(dir + "/out_T.bin", out, 8);
        write_all(dir + "/out_mask.bin", solver.inlierMask.data(), solver.inlierMask.size());
        write_all(dir + "/out_meta.bin", meta, 3);
        std::printf("sim3_driver: %d inliers of %d pairs, %d iterations\n", nInliers, solver.N, its);
        return 0;
    }
    catch (const std::exception& e)
    {
        std::cerr << e.what() << "\n";
        return 1;
    }
}
