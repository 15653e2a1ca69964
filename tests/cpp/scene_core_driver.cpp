// CPU build of snake_slam_amd/csrc/scene_core.hpp and the scene part of dispatch.hpp (plain g++, no HIP): the candidate and chain rule, the
// skip rules and the weight arithmetic on rows of inputs, for tests/test_scene_core_cpu.py.
//   scene_core_driver DIR        reads rows.bin: rows of eight doubles (time a, time b, imu begin b, imu end b, preint valid b, gyro weight,
//                                acc weight, weight_translation) and flags.bin: int64 rows of (n_neighbours, size, kf_bad, earlier, point id,
//                                flags, image constant, status, n_window, win_cap); writes out.bin: per row three doubles (emitted, weight
//                                rotation, weight translation) and out_flags.bin: int64 rows of (neighbours taken, candidate survives, point
//                                skipped, point constant, record skipped, window status)
//   scene_core_driver --consts   the limits, the table sizes and the carves
#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "scene_core.hpp"
#include "dispatch.hpp"

using namespace snk;

template <typename T>
static std::vector<T> read_all(const std::string& path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error("scene_core_driver: missing " + path);
    std::vector<T> v((size_t)f.tellg() / sizeof(T));
    f.seekg(0);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
    return v;
}

template <typename T>
static void write_all(const std::string& path, const std::vector<T>& v)
{
    std::ofstream g(path, std::ios::binary);
    g.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

int main(int argc, char** argv)
{
    try
    {
        if (argc == 2 && std::strcmp(argv[1], "--consts") == 0)
        {
            std::printf("threads %d win_threads %d max_window %d max_img %d max_obs %d max_walk %d img_slots_1 %d img_slots_512 %d img_slots_max %d "
                        "sort_len_512 %d sort_len_max %d window_carve %zu points_carve_max %zu obs_carve_max %zu gather_carve_max %zu gather_carve_ref %zu "
                        "gather_carve_2048_128 %zu\n",
                        SCENE_THREADS, SCENE_WIN_THREADS, SCENE_MAX_WINDOW, SCENE_MAX_IMG, SCENE_MAX_OBS, SCENE_MAX_WALK, scene_img_slots(1), scene_img_slots(512),
                        scene_img_slots(SCENE_MAX_IMG), scene_sort_len(512), scene_sort_len(SCENE_MAX_IMG), scene_window_carve(), scene_points_carve(LMAP_MAX_PTS),
                        scene_obs_carve(SCENE_MAX_IMG), scene_gather_carve(LMAP_MAX_PTS, SCENE_MAX_IMG), scene_gather_carve(16384, 512),
                        scene_gather_carve(2048, 128));
            return 0;
        }
        if (argc != 2) throw std::runtime_error("usage: scene_core_driver DIR | --consts");
        const std::string dir = argv[1];
        const std::vector<double> in   = read_all<double>(dir + "/rows.bin");
        const std::vector<int64_t> fl  = read_all<int64_t>(dir + "/flags.bin");
        const size_t n = in.size() / 8, m = fl.size() / 10;
        std::vector<double> out(n * 3);
        std::vector<int64_t> out_fl(m * 6);
        for (size_t r = 0; r < n; ++r)
        {
            const double* a = in.data() + r * 8;
            double w_rot = -1, w_tr = -1;
            scene_rpc_weights(a[0], a[1], a[5], a[6], a[7], w_rot, w_tr);
            out[r * 3 + 0] = scene_rpc_emitted(a[0], a[1], a[2], a[3], (unsigned)a[4]) ? 1.0 : 0.0;
            out[r * 3 + 1] = w_rot;
            out[r * 3 + 2] = w_tr;
        }
        for (size_t r = 0; r < m; ++r)
        {
            const int64_t* a = fl.data() + r * 10;
            int64_t* o       = out_fl.data() + r * 6;
            o[0] = scene_n_neighbours_taken((int)a[0], (int)a[1]);
            o[1] = scene_candidate_survives((unsigned)a[2], a[3] != 0);
            o[2] = scene_point_skipped((int)a[4], (unsigned)a[5]);
            o[3] = scene_point_constant((unsigned)a[5]);
            o[4] = scene_record_skipped((unsigned)a[2], a[6] != 0, scene_point_constant((unsigned)a[5]));
            o[5] = scene_window_status((int)a[7], (int)a[8], (int)a[9]);
        }
        write_all(dir + "/out.bin", out);
        write_all(dir + "/out_flags.bin", out_fl);
        return 0;
    }
    catch (const std::exception& e)
    {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
