// Runs snake_hip::Triangulator (snake_slam_amd/cpp/snake_hip.hpp) the way Snake's local mapping would call it after the
// triangulation matchers: Process over all neighbour keyframes, then triangulate for every keyframe pair on its own.
// Inputs and outputs are raw little-endian arrays in the directory argv[1] (written / read by
// tests/test_cpp_triangulator_gpu.py, which compares the outputs with the Python mirror and the numpy restatement).
#include <cstdio>
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

struct Keyframe
{
    std::vector<snk_kp64> kps;
    std::vector<float> right_points, depth;
    std::vector<uint8_t> has_mp;
    snake_hip::Triangulator::KeyframeView view;
};

static void load(Keyframe& kf, const std::string& tag)
{
    kf.kps          = rd<snk_kp64>(tag + "_kps");
    kf.right_points = rd<float>(tag + "_rp");
    kf.depth        = rd<float>(tag + "_depth");
    kf.has_mp       = rd<uint8_t>(tag + "_has");
    const auto pose = rd<double>(tag + "_pose");  // qx qy qz qw tx ty tz, median depth
    for (int i = 0; i < 7; ++i) kf.view.pose[i] = pose[i];
    kf.view.median_depth          = (float)pose[7];
    kf.view.undistorted_keypoints = &kf.kps;
    kf.view.right_points          = &kf.right_points;
    kf.view.depth                 = &kf.depth;
    kf.view.has_map_point         = &kf.has_mp;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    g_dir = argv[1];
    try
    {
        using namespace snake_hip;
        const auto cam  = rd<double>("cam");     // fx fy cx cy bf th_depth
        const auto ls   = rd<float>("ls");
        const auto meta = rd<int32_t>("meta");   // neighbours, mono
        const snk_camera K{cam[0], cam[1], cam[2], cam[3], cam[4]};
        Triangulator tri(K, ls, cam[5], meta[1] != 0);
        Triangulator::TriangulationParams params;  // reprojectionErrorThresholdMono / Stereo: 2.1 / 2.3
        Keyframe kf1;
        load(kf1, "kf1");
        std::vector<Keyframe> kf2s((size_t)meta[0]);
        std::vector<Triangulator::KeyframeView> views;
        std::vector<std::vector<std::pair<int, int>>> matches;
        for (int k = 0; k < meta[0]; ++k)
        {
            load(kf2s[k], "kf2_" + std::to_string(k));
            views.push_back(kf2s[k].view);
            const auto p = rd<int32_t>("pairs_" + std::to_string(k));
            std::vector<std::pair<int, int>> m;
            for (size_t i = 0; i + 1 < p.size(); i += 2) m.emplace_back(p[i], p[i + 1]);
            matches.push_back(m);
        }
        std::vector<Triangulator::ImageTriangulationResult> newPointsa;
        const int nnew = tri.Process(params, kf1.view, views, matches, newPointsa);
        std::vector<snk_new_point> all;
        std::vector<int32_t> counts{nnew};
        for (const auto& r : newPointsa)
        {
            all.insert(all.end(), r.newPoints.begin(), r.newPoints.end());
            counts.push_back((int32_t)r.newPoints.size());
        }
        wr("out_points", all);
        wr("out_counts", counts);
        std::vector<snk_new_point> singles;
        for (int k = 0; k < meta[0]; ++k)
        {
            const auto r = tri.triangulate(params, kf1.view, views[k], matches[k]);
            singles.insert(singles.end(), r.newPoints.begin(), r.newPoints.end());
        }
        wr("out_singles", singles);
        // no neighbours, and a neighbour without pairs: valid, nothing comes back
        std::vector<Triangulator::ImageTriangulationResult> none;
        if (tri.Process(params, kf1.view, {}, {}, none) != 0 || !none.empty()) throw std::runtime_error("empty Process");
        if (!tri.triangulate(params, kf1.view, views[0], {}).newPoints.empty()) throw std::runtime_error("empty triangulate");
        // an index out of range is an exception with the library's text, not a fault
        bool threw = false;
        try
        {
            tri.triangulate(params, kf1.view, views[0], {{(int)kf1.kps.size(), 0}});
        }
        catch (const std::exception& e)
        {
            threw = std::string(e.what()).find("out of range") != std::string::npos;
        }
        if (!threw) throw std::runtime_error("out-of-range index was not refused");
    }
    catch (const std::exception& e)
    {
        std::cerr << "triangulator_driver: " << e.what() << "\n";
        return 1;
    }
    return 0;
}
