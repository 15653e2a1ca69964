// Runs snake_hip::MapPointRefresher (snake_slam_amd/cpp/snake_hip.hpp) the way Snake's mapping loops would: mock Keyframe and MapPoint
// structs with the members the three updates read (MapPoint.cpp:60-81, :120-135, :154-166), one PointView per point gathered from
// them, one call after the loop, the results written back into the MapPoints.  Inputs and outputs are raw little-endian arrays in
// the directory argv[1] (written / read by tests/test_cpp_mappoint_gpu.py, which compares the outputs with the Python mirror).
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

struct Keyframe  // Snake::Keyframe, the members the updates read
{
    double pose[7];
    std::vector<snake_hip::DescriptorORB> descriptors;  // frame->descriptors
    std::vector<int32_t> octaves;                       // frame->undistorted_keypoints[i].octave
    bool bad = false;
    bool isBad() const { return bad; }
};

struct MapPoint  // Snake::MapPoint
{
    std::vector<std::pair<Keyframe*, int>> mObservations;
    double position[3];
    Keyframe* referenceKF = nullptr;
    snake_hip::DescriptorORB descriptor{};
    double normal[3]          = {0, 0, 0};
    double reference_depth    = 0;
    int reference_scale_level = -1;

    snake_hip::MapPointRefresher::PointView view() const
    {
        snake_hip::MapPointRefresher::PointView v;
        for (size_t i = 0; i < mObservations.size(); ++i)
        {
            const auto& [kf, idx] = mObservations[i];
            v.observations.push_back({kf->pose, &kf->descriptors[(size_t)idx], kf->octaves[(size_t)idx], !kf->isBad()});
            if (kf == referenceKF) v.ref_obs = (int)i;  // indexInternal(referenceKF)
        }
        for (int i = 0; i < 3; ++i) v.position[i] = position[i];
        return v;
    }
};

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    g_dir = argv[1];
    try
    {
        using namespace snake_hip;
        const auto meta  = rd<int32_t>("meta");  // keyframes, features per keyframe, rule
        const auto poses = rd<double>("kf_pose");
        const auto desc  = rd<uint64_t>("kf_desc");
        const auto oct   = rd<int32_t>("kf_octave");
        const auto bad   = rd<uint8_t>("kf_bad");
        const auto start = rd<int32_t>("obs_start");
        const auto obs   = rd<int32_t>("obs");  // (keyframe, feature)
        const auto pos   = rd<double>("position");
        const auto refkf = rd<int32_t>("ref_kf");  // the reference keyframe of each point (-1: none)
        const int nk = meta[0], cap = meta[1];
        std::vector<Keyframe> kfs((size_t)nk);
        for (int k = 0; k < nk; ++k)
        {
            for (int i = 0; i < 7; ++i) kfs[k].pose[i] = poses[(size_t)k * 7 + i];
            kfs[k].bad = bad[k] != 0;
            for (int f = 0; f < cap; ++f)
            {
                const uint64_t* d = &desc[((size_t)k * cap + f) * 4];
                kfs[k].descriptors.push_back({d[0], d[1], d[2], d[3]});
                kfs[k].octaves.push_back(oct[(size_t)k * cap + f]);
            }
        }
        std::vector<MapPoint> mps(start.size() - 1);
        for (size_t p = 0; p < mps.size(); ++p)
        {
            for (int o = start[p]; o < start[p + 1]; ++o) mps[p].mObservations.emplace_back(&kfs[(size_t)obs[2 * o]], obs[2 * o + 1]);
            for (int i = 0; i < 3; ++i) mps[p].position[i] = pos[p * 3 + i];
            mps[p].referenceKF = refkf[p] >= 0 ? &kfs[(size_t)refkf[p]] : nullptr;
        }
        MapPointRefresher refresher(meta[2]);
        std::vector<MapPointRefresher::PointView> views;
        for (const MapPoint& mp : mps) views.push_back(mp.view());
        const auto all = refresher.Refresh(views);
        for (size_t p = 0; p < mps.size(); ++p)  // the write-back of the three updates
        {
            if (all[p].best >= 0) std::memcpy(mps[p].descriptor.data(), all[p].desc, 32);
            std::memcpy(mps[p].normal, all[p].normal, 24);
            if (views[p].ref_obs >= 0) mps[p].reference_depth = all[p].ref_depth, mps[p].reference_scale_level = all[p].ref_level;
        }
        wr("out_all", all);
        wr("out_desc", refresher.ComputeDistinctiveDescriptors(views));
        wr("out_normal", refresher.UpdateNormal(views));
        wr("out_depth", refresher.UpdateDepth(views));
        std::vector<int32_t> ref_obs;
        for (const auto& v : views) ref_obs.push_back(v.ref_obs);
        wr("out_ref_obs", ref_obs);
        // no points: valid, nothing comes back
        if (!refresher.Refresh({}).empty()) throw std::runtime_error("empty Refresh");
        // too many observations are an exception with the library's text, not a fault
        bool threw = false;
        try
        {
            MapPointRefresher::PointView big;
            big.observations.assign(SNK_MP_MAX_OBS + 1, views.empty() || views[0].observations.empty() ? MapPointRefresher::Observation{kfs[0].pose, &kfs[0].descriptors[0], 0, true}
                                                                                                       : views[0].observations[0]);
            refresher.Refresh({big});
        }
        catch (const std::exception& e)
        {
            threw = std::string(e.what()).find("SNK_MP_MAX_OBS") != std::string::npos;
        }
        if (!threw) throw std::runtime_error("a point with too many observations was not refused");
    }
    catch (const std::exception& e)
    {
        std::cerr << "mappoint_driver: " << e.what() << "\n";
        return 1;
    }
    return 0;
}
