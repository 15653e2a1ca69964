// Runs snake_hip::BARec::createDev (snake_slam_amd/cpp/snake_hip.hpp) the way a Snake-SLAM host would behind a device-side
// MakeLocalScene: the rows of a snk_scene_out are in device memory, the bundle adjustment takes them from there (snk_ba_set_problems_dev),
// solves every window and hands the states back.  Inputs and outputs are raw little-endian arrays in the directory argv[1] (written / read
// by tests/test_cpp_ba_dev_gpu.py, which compares with snk_ba_set_problems on the same rows).
//   meta.bin (int32): n_q, win_cap, pt_cap, img_cap, obs_cap;  kbf.bin (double): fx fy cx cy bf
//   pose, img_const, pt, pt_const, obs_img, obs_pt, obs_uv, obs_depth, obs_weight, rpc, result: the rows, [n_q][cap] each
#include <hip/hip_runtime_api.h>

#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "snake_hip.hpp"

static std::string g_dir;

static std::vector<char> rd(const std::string& name)
{
    std::ifstream f(g_dir + "/" + name + ".bin", std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error("missing input " + name);
    std::vector<char> v((size_t)f.tellg());
    f.seekg(0);
    f.read(v.data(), (std::streamsize)v.size());
    return v;
}

template <typename T>
static void wr(const std::string& name, const std::vector<T>& v)
{
    std::ofstream f(g_dir + "/" + name + ".bin", std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

static std::vector<void*> g_dev;
template <typename T>
static T* to_device(const std::string& name)
{
    const std::vector<char> h = rd(name);
    void* p = nullptr;
    if (hipMalloc(&p, h.size() + 16) != hipSuccess || hipMemcpy(p, h.data(), h.size(), hipMemcpyHostToDevice) != hipSuccess)
        throw std::runtime_error("device copy of " + name + " failed");
    g_dev.push_back(p);
    return static_cast<T*>(p);
}

int main(int argc, char** argv)
{
    if (argc != 2)
    {
        std::cerr << "usage: ba_dev_driver DIR\n";
        return 2;
    }
    g_dir = argv[1];
    try
    {
        const std::vector<char> meta_b = rd("meta"), kbf_b = rd("kbf"), res_b = rd("result");
        const int32_t* meta = reinterpret_cast<const int32_t*>(meta_b.data());
        const double* kbf   = reinterpret_cast<const double*>(kbf_b.data());
        const snk_scene_result* res = reinterpret_cast<const snk_scene_result*>(res_b.data());
        const int n_q = meta[0];
        snk_scene_out o{};
        o.win_cap = meta[1], o.pt_cap = meta[2], o.img_cap = meta[3], o.obs_cap = meta[4];
        o.pose = to_device<double>("pose"), o.img_const = to_device<uint8_t>("img_const"), o.pt = to_device<double>("pt");
        o.pt_const = to_device<uint8_t>("pt_const"), o.obs_img = to_device<int32_t>("obs_img"), o.obs_pt = to_device<int32_t>("obs_pt");
        o.obs_uv = to_device<double>("obs_uv"), o.obs_depth = to_device<double>("obs_depth"), o.obs_weight = to_device<double>("obs_weight");
        o.rpc = to_device<snk_ba_rpc>("rpc"), o.result = to_device<snk_scene_result>("result");
        if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("hipDeviceSynchronize failed");  // the rows' producer is complete

        snake_hip::BARec ba;
        ba.createDev(n_q, o, kbf, kbf[4]);
        const std::vector<snake_hip::OptimizationResults> r = ba.solveAll();
        std::vector<double> cost, pose, pt;
        for (int s = 0; s < n_q; ++s)
        {
            cost.push_back(r[(size_t)s].cost_initial), cost.push_back(r[(size_t)s].cost_final);
            const bool ok = res[s].status == SNK_SCENE_OK;
            std::vector<double> ps((size_t)(ok ? res[s].n_img : 0) * 7 + 7), pp((size_t)(ok ? res[s].n_pt : 0) * 3 + 3);
            snake_hip::check(snk_ba_get_state(ba.handle(), s, reinterpret_cast<double(*)[7]>(ps.data()), reinterpret_cast<double(*)[3]>(pp.data()), nullptr),
                             "snk_ba_get_state");
            pose.insert(pose.end(), ps.begin(), ps.end() - 7), pt.insert(pt.end(), pp.begin(), pp.end() - 3);
        }
        wr("out_cost", cost), wr("out_pose", pose), wr("out_pt", pt);
        for (void* p : g_dev) (void)hipFree(p);
        return 0;
    }
    catch (const std::exception& e)
    {
        std::cerr << e.what() << "\n";
        return 1;
    }
}
