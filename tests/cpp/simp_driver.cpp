// snake_hip::KeyframeCuller of the adaptor header on mock Keyframe / MapPoint objects, for tests/test_cpp_simp_gpu.py (plain g++).
//   simp_driver DIR   reads meta.bin (int32: n_kf, n_points, n_obs, n_feat, n_list, n_q, with_times, node_cap, stereo, feat_cap), th_depth.bin
//                     (float), params.bin (snk_simp_params), the tables of snk_simp_map and snk_simp_graph and q (.bin) from DIR; builds the
//                     objects, flattens them with Map::FromObjects and writes verdict.bin, stats.bin, redundancy.bin and median.bin (the
//                     cache after the call)
#include <cstdio>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "snake_hip.hpp"

struct MapPoint;
struct Keyframe  // the members Simplification.cpp and Keyframe.cpp read
{
    int slot = 0;
    bool bad = false;
    double pose[7];
    float cull_factor   = 1.0f;
    double median_depth = -1;
    std::vector<MapPoint*> observations;
    std::vector<float> depth;
    std::vector<int> octave;
    std::vector<std::pair<int, Keyframe*>> connections;
    Keyframe *previousKF = nullptr, *nextKF = nullptr;
    double timeStamp = 0;
};
struct MapPoint
{
    int slot = 0;
    bool bad = false;
    double position[3];
    std::vector<std::pair<Keyframe*, int>> observations;
};

template <typename T>
static std::vector<T> load(const std::string& dir, const char* name, size_t n)
{
    std::vector<T> v(n);
    if (n == 0) return v;
    std::ifstream f(dir + "/" + name + ".bin", std::ios::binary);
    if (!f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(T)))) throw std::runtime_error(std::string("simp_driver: missing input ") + name);
    return v;
}

template <typename T>
static void save(const std::string& dir, const char* name, const std::vector<T>& v)
{
    std::ofstream f(dir + "/" + name + ".bin", std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

int main(int argc, char** argv)
{
    try
    {
        if (argc != 2) throw std::runtime_error("usage: simp_driver DIR");
        const std::string dir = argv[1];
        const auto meta       = load<int32_t>(dir, "meta", 10);
        const size_t n_kf = (size_t)meta[0], n_points = (size_t)meta[1], n_obs = (size_t)meta[2], n_feat = (size_t)meta[3], n_list = (size_t)meta[4],
                     n_q = (size_t)meta[5];
        const bool times = meta[6] != 0;
        const auto params      = load<snk_simp_params>(dir, "params", 1)[0];
        const float th_depth   = load<float>(dir, "th_depth", 1)[0];
        const auto kf_bad      = load<uint8_t>(dir, "kf_bad", n_kf);
        const auto kf_pose     = load<double>(dir, "kf_pose", n_kf * 7);
        const auto cull_factor = load<float>(dir, "kf_cull_factor", n_kf);
        const auto median      = load<double>(dir, "kf_median_depth", n_kf);
        const auto kf_prev     = load<int32_t>(dir, "kf_prev", times ? n_kf : 0);
        const auto kf_next     = load<int32_t>(dir, "kf_next", times ? n_kf : 0);
        const auto kf_time     = load<double>(dir, "kf_time", times ? n_kf : 0);
        const auto conn_start  = load<int32_t>(dir, "conn_start", n_kf + 1);
        const auto conn_list   = load<snk_covis_conn>(dir, "conn_list", n_list);
        const auto feat_start  = load<int32_t>(dir, "feat_start", n_kf + 1);
        const auto feat_point  = load<int32_t>(dir, "feat_point", n_feat);
        const auto feat_depth  = load<float>(dir, "feat_depth", n_feat);
        const auto feat_octave = load<int32_t>(dir, "feat_octave", n_feat);
        const auto obs_start   = load<int32_t>(dir, "obs_start", n_points + 1);
        const auto obs         = load<int32_t>(dir, "obs", n_obs * 2);
        const auto pt_flags    = load<uint8_t>(dir, "pt_flags", n_points);
        const auto pt_pos      = load<double>(dir, "pt_pos", n_points * 3);
        const auto q           = load<int32_t>(dir, "q", n_q);

        // the map as objects that point at each other
        std::vector<std::unique_ptr<Keyframe>> kf_store;
        std::vector<std::unique_ptr<MapPoint>> mp_store;
        std::vector<Keyframe*> keyframes;
        std::vector<MapPoint*> points;
        for (size_t k = 0; k < n_kf; ++k) kf_store.emplace_back(new Keyframe), keyframes.push_back(kf_store.back().get());
        for (size_t p = 0; p < n_points; ++p) mp_store.emplace_back(new MapPoint), points.push_back(mp_store.back().get());
        for (size_t k = 0; k < n_kf; ++k)
        {
            Keyframe* kf = keyframes[k];
            kf->slot = (int)k, kf->bad = kf_bad[k] != 0, kf->cull_factor = cull_factor[k], kf->median_depth = median[k];
            for (int j = 0; j < 7; ++j) kf->pose[j] = kf_pose[k * 7 + (size_t)j];
            for (int f = feat_start[k]; f < feat_start[k + 1]; ++f)
            {
                kf->observations.push_back(feat_point[(size_t)f] >= 0 ? points[(size_t)feat_point[(size_t)f]] : nullptr);
                kf->depth.push_back(feat_depth[(size_t)f]);
                kf->octave.push_back(feat_octave[(size_t)f]);
            }
            for (int c = conn_start[k]; c < conn_start[k + 1]; ++c) kf->connections.emplace_back(conn_list[(size_t)c].weight, keyframes[(size_t)conn_list[(size_t)c].kf]);
            if (times)
            {
                kf->previousKF = kf_prev[k] >= 0 ? keyframes[(size_t)kf_prev[k]] : nullptr;
                kf->nextKF     = kf_next[k] >= 0 ? keyframes[(size_t)kf_next[k]] : nullptr;
                kf->timeStamp  = kf_time[k];
            }
        }
        for (size_t p = 0; p < n_points; ++p)
        {
            MapPoint* mp = points[p];
            mp->slot = (int)p, mp->bad = (pt_flags[p] & SNK_COVIS_PT_BAD) != 0;
            for (int j = 0; j < 3; ++j) mp->position[j] = pt_pos[p * 3 + (size_t)j];
            for (int o = obs_start[p]; o < obs_start[p + 1]; ++o) mp->observations.emplace_back(keyframes[(size_t)obs[(size_t)o * 2]], obs[(size_t)o * 2 + 1]);
        }

        snake_hip::KeyframeCuller::Map map = snake_hip::KeyframeCuller::Map::FromObjects(keyframes, points, times);
        snake_hip::KeyframeCuller culler(params, snk_simp_stats_params{3, meta[8], th_depth, meta[9]}, meta[7]);
        const std::vector<float> redundancy = culler.Redundancy(map, q);
        std::vector<snk_simp_stats_result> stats;
        const std::vector<snk_simp_verdict> verdict = culler.KeyFrameCullingGraph(map, q, &stats);
        save(dir, "verdict", verdict);
        save(dir, "stats", stats);
        save(dir, "redundancy", redundancy);
        save(dir, "median", map.kf_median_depth);
        return 0;
    }
    catch (const std::exception& e)
    {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
