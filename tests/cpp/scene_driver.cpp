// Runs snake_hip::LocalSceneBuilder (snake_slam_amd/cpp/snake_hip.hpp) the way Snake's local mapping would per keyframe: the map as
// LocalSceneBuilder::Map, one Window and one Gather call for the queries, then the first scene handed to the bundle adjustment through
// Scenes::Problem (snk_ba_set_problem, snk_ba_solve).  Inputs and outputs are raw little-endian arrays in the directory argv[1] (written /
// read by tests/test_cpp_scene_gpu.py, which compares the outputs with the restatement and the oracle).
//   meta.bin (int32): n_neighbours, n_last, win_cap, pt_cap, img_cap, obs_cap;  kbf.bin (double): fx fy cx cy bf
//   q, kf_bad, kf_prev, kf_pose, conn_start, conn_list, feat_start, feat_point, feat_octave, feat_depth, feat_uv, obs_start, obs, pt_flags,
//   pt_pos, level_inv_sq_scale
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "snake_hip.hpp"

static std::string g_dir;

template <typename T>
static std::vector<T> rd(const std::string& name)
{
    std::ifstream f(g_dir + "/" + name + ".bin", std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error("missing input " + name);
    const size_t bytes = (size_t)f.tellg();
    if (bytes % sizeof(T)) throw std::runtime_error("size of " + name + " is not a multiple of its element size");
    std::vector<T> v(bytes / sizeof(T));
    f.seekg(0);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)bytes);
    return v;
}

template <typename T>
static void wr(const std::string& name, const std::vector<T>& v)
{
    std::ofstream f(g_dir + "/" + name + ".bin", std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

using snake_hip::LocalSceneBuilder;

int main(int argc, char** argv)
{
    if (argc != 2)
    {
        std::cerr << "usage: scene_driver DIR\n";
        return 2;
    }
    g_dir = argv[1];
    try
    {
        const auto meta = rd<int32_t>("meta");
        const auto kbf  = rd<double>("kbf");
        LocalSceneBuilder::Map map;
        map.kf_bad = rd<uint8_t>("kf_bad"), map.kf_prev = rd<int32_t>("kf_prev"), map.kf_pose = rd<double>("kf_pose");
        map.conn_start = rd<int32_t>("conn_start"), map.conn_list = rd<snk_covis_conn>("conn_list");
        map.feat_start = rd<int32_t>("feat_start"), map.feat_point = rd<int32_t>("feat_point"), map.feat_octave = rd<int32_t>("feat_octave");
        map.feat_depth = rd<float>("feat_depth"), map.feat_uv = rd<float>("feat_uv");
        map.obs_start = rd<int32_t>("obs_start"), map.obs = rd<int32_t>("obs");
        map.pt_flags = rd<uint8_t>("pt_flags"), map.pt_pos = rd<double>("pt_pos"), map.level_inv_sq_scale = rd<float>("level_inv_sq_scale");

        LocalSceneBuilder builder(snk_scene_params{meta[0], meta[1], 0.0, 0.0}, meta[2]);
        const LocalSceneBuilder::Windows win = builder.Window(map, rd<int32_t>("q"));
        LocalSceneBuilder::Scenes sc         = builder.Gather(map, win, meta[3], meta[4], meta[5]);
        wr("out_window_kf", win.window_kf), wr("out_window", win.result), wr("out_result", sc.result);
        wr("out_img_kf", sc.img_kf), wr("out_pose", sc.pose), wr("out_img_const", sc.img_const), wr("out_pt_id", sc.pt_id), wr("out_pt", sc.pt);
        wr("out_pt_const", sc.pt_const), wr("out_pt_valid", sc.pt_valid), wr("out_obs_img", sc.obs_img), wr("out_obs_pt", sc.obs_pt);
        wr("out_obs_uv", sc.obs_uv), wr("out_obs_depth", sc.obs_depth), wr("out_obs_weight", sc.obs_weight), wr("out_obs_src", sc.obs_src);

        // the hand-over: row 0 as it stands
        const snk_ba_problem problem = sc.Problem(0, kbf.data(), kbf[4]);
        const snk_ba_options opt{3, 30, 1e-10, 2.1, 2.3, 0.0};  // LocalBundleAdjustment.cpp:47-64
        snk_ba* ba = nullptr;
        snake_hip::check(snk_ba_create(&opt, 0, nullptr, &ba), "snk_ba_create");
        std::vector<double> cost(2);
        snake_hip::check(snk_ba_set_problem(ba, &problem), "snk_ba_set_problem");
        snake_hip::check(snk_ba_solve(ba, 3, &cost[0], &cost[1]), "snk_ba_solve");
        std::vector<double> pose((size_t)problem.n_img * 7), pt((size_t)problem.n_pt * 3);
        int pcg = 0;
        snake_hip::check(snk_ba_get_state(ba, 0, reinterpret_cast<double(*)[7]>(pose.data()), reinterpret_cast<double(*)[3]>(pt.data()), &pcg), "snk_ba_get_state");
        snk_ba_destroy(ba);
        wr("out_cost", cost), wr("out_ba_pose", pose), wr("out_ba_pt", pt);
        return 0;
    }
    catch (const std::exception& e)
    {
        std::cerr << e.what() << "\n";
        return 1;
    }
}
