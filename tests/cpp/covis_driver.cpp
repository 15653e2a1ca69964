// Runs snake_hip::CovisibilityGraph (snake_slam_amd/cpp/snake_hip.hpp) the way Snake's mapping and tracking loops would: mock Keyframe
// and MapPoint structs joined by pointers with the members Keyframe::UpdateConnections (Keyframe.cpp:89-171) and the vote of
// UpdateLocalKeyFrames2 (TrackingFine.cpp:230-268) read, flattened into MapTables by walking the pointers, one call per operation.
// Inputs and outputs are raw little-endian arrays in the directory argv[1] (written / read by tests/test_cpp_covis_gpu.py, which
// compares the outputs with the Python mirror).
#include <fstream>
#include <iostream>
#include <map>
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

struct Keyframe;
struct MapPoint  // Snake::MapPoint
{
    std::vector<std::pair<Keyframe*, int>> mObservations;
    bool bad = false, far_stereo_point = false;
    int id = 0;
};
struct Keyframe  // Snake::Keyframe
{
    std::vector<MapPoint*> observations;  // per feature, nullptr: none
    std::vector<float> depth;             // frame->depth
    bool bad = false;
    int id   = 0;
};

using snake_hip::CovisibilityGraph;

static void write_lists(const std::string& name, const std::vector<CovisibilityGraph::List>& lists, int cap)
{
    std::vector<snk_covis_conn> conn(lists.size() * (size_t)cap, snk_covis_conn{-1, -1});
    std::vector<int32_t> res, best, by_weight;
    for (size_t s = 0; s < lists.size(); ++s)
    {
        const auto& l = lists[s];
        std::copy(l.connections.begin(), l.connections.end(), conn.begin() + (std::ptrdiff_t)(s * (size_t)cap));
        res.insert(res.end(), {l.n_found, (int32_t)l.connections.size(), l.Best(), l.status});
        std::vector<int> b = l.BestCovisibility(5);
        b.resize(5, -1);
        best.insert(best.end(), b.begin(), b.end());
        by_weight.push_back((int32_t)l.CovisiblesByWeight(16).size());
    }
    wr(name + "_conn", conn);
    wr(name + "_res", res);
    wr(name + "_best5", best);
    wr(name + "_w16", by_weight);
}

int main(int argc, char** argv)
{
    try
    {
        if (argc != 2) throw std::runtime_error("usage: covis_driver DIR");
        g_dir           = argv[1];
        const auto meta = rd<int32_t>("meta");  // n_kf, n_points, th, cap
        const int n_kf = meta.at(0), n_points = meta.at(1), th = meta.at(2), cap = meta.at(3);
        const float th_depth = rd<float>("th_depth").at(0);
        const auto kf_bad = rd<uint8_t>("kf_bad"), pt_flags = rd<uint8_t>("pt_flags");
        const auto obs_start = rd<int32_t>("obs_start"), obs = rd<int32_t>("obs"), feat_start = rd<int32_t>("feat_start"), feat_point = rd<int32_t>("feat_point");
        const auto feat_depth = rd<float>("feat_depth");
        const auto q = rd<int32_t>("q"), set_start = rd<int32_t>("set_start"), set_point = rd<int32_t>("set_point");

        // the pointer graph
        std::vector<Keyframe> kfs((size_t)n_kf);
        std::vector<MapPoint> mps((size_t)n_points);
        for (int p = 0; p < n_points; ++p)
        {
            mps[(size_t)p].id               = p;
            mps[(size_t)p].bad              = (pt_flags[(size_t)p] & SNK_COVIS_PT_BAD) != 0;
            mps[(size_t)p].far_stereo_point = (pt_flags[(size_t)p] & SNK_COVIS_PT_FAR) != 0;
            for (int o = obs_start[(size_t)p]; o < obs_start[(size_t)p + 1]; ++o)
                mps[(size_t)p].mObservations.push_back({&kfs[(size_t)obs[(size_t)o * 2]], obs[(size_t)o * 2 + 1]});
        }
        for (int k = 0; k < n_kf; ++k)
        {
            kfs[(size_t)k].id  = k;
            kfs[(size_t)k].bad = kf_bad[(size_t)k] != 0;
            for (int i = feat_start[(size_t)k]; i < feat_start[(size_t)k + 1]; ++i)
            {
                kfs[(size_t)k].observations.push_back(feat_point[(size_t)i] < 0 ? nullptr : &mps[(size_t)feat_point[(size_t)i]]);
                kfs[(size_t)k].depth.push_back(feat_depth[(size_t)i]);
            }
        }

        // what a Snake maintainer writes: flatten by walking the pointers
        CovisibilityGraph::MapTables tables;
        for (const MapPoint& mp : mps)
        {
            std::vector<std::pair<int, int>> list;
            for (const auto& o : mp.mObservations) list.push_back({o.first->id, o.second});
            tables.AddPoint(mp.bad, mp.far_stereo_point, list);
        }
        for (const Keyframe& kf : kfs)
        {
            std::vector<int32_t> pts;
            for (const MapPoint* mp : kf.observations) pts.push_back(mp ? mp->id : -1);
            tables.AddKeyframe(kf.bad, pts, kf.depth);
        }
        std::vector<std::vector<int32_t>> frames;
        for (size_t s = 0; s + 1 < set_start.size(); ++s)
            frames.emplace_back(set_point.begin() + set_start[s], set_point.begin() + set_start[s + 1]);

        CovisibilityGraph graph(th, th_depth, cap);
        write_lists("update", graph.UpdateConnections(tables, q), cap);
        write_lists("vote", graph.VoteLocalKeyframes(tables, frames), cap);
        return 0;
    }
    catch (const std::exception& e)
    {
        std::cerr << "covis_driver: " << e.what() << "\n";
        return 1;
    }
}
