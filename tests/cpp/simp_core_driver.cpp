// CPU build of snake_slam_amd/csrc/simp_core.hpp and the culling part of dispatch.hpp (plain g++, no HIP): the statements the kernels
// run per query -- depth, key, select, redundancy test, node filter, edge weight, Prim step, angle, verdict -- on one thread, for
// tests/test_simp_core_cpu.py.
//   simp_core_driver stats DIR    reads meta.bin (int32: n_kf, n_points, n_obs, n_feat, n_q, min_obs, stereo, feat_cap), th_depth.bin (float)
//                                 and the tables of snk_simp_map plus q (.bin) from DIR; writes stats.bin
//   simp_core_driver decide DIR   reads meta.bin (int32: n_kf, n_list, n_q, node_cap, 1 = with the time tables), params.bin (snk_simp_params),
//                                 the tables of snk_simp_graph, q and stats (.bin); writes verdict.bin
//   simp_core_driver angles DIR   reads meta.bin (int32: n_kf, n pairs), kf_pose, kf_median_depth and pairs (int32 [n][2]); writes angles.bin
//   simp_core_driver select DIR   reads meta.bin (int32: n) and z.bin (float [n]); writes median.bin: the element (n - 1) / 2 by simp_key / simp_select
//   simp_core_driver --consts     the limits, the long-list threshold under SNK_SIMP_LONG_MIN unset / 0 / 7 and the carves
#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "dispatch.hpp"
#include "simp_core.hpp"

using namespace snk;

template <typename T>
static std::vector<T> load(const std::string& dir, const char* name, size_t n)
{
    std::vector<T> v(n);
    if (n == 0) return v;
    std::ifstream f(dir + "/" + name + ".bin", std::ios::binary);
    if (!f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(T)))) throw std::runtime_error(std::string("simp_core_driver: missing input ") + name);
    return v;
}

template <typename T>
static void save(const std::string& dir, const char* name, const std::vector<T>& v)
{
    std::ofstream f(dir + "/" + name + ".bin", std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

static int run_stats(const std::string& dir)
{
    const auto meta = load<int32_t>(dir, "meta", 8);
    const size_t n_kf = (size_t)meta[0], n_points = (size_t)meta[1], n_obs = (size_t)meta[2], n_feat = (size_t)meta[3], n_q = (size_t)meta[4];
    const int min_obs = meta[5], stereo = meta[6], feat_cap = meta[7];
    const float th_depth   = load<float>(dir, "th_depth", 1)[0];
    const auto kf_bad      = load<uint8_t>(dir, "kf_bad", n_kf);
    const auto kf_pose     = load<double>(dir, "kf_pose", n_kf * 7);
    const auto feat_start  = load<int32_t>(dir, "feat_start", n_kf + 1);
    const auto feat_point  = load<int32_t>(dir, "feat_point", n_feat);
    const auto feat_depth  = load<float>(dir, "feat_depth", n_feat);
    const auto feat_octave = load<int32_t>(dir, "feat_octave", n_feat);
    const auto obs_start   = load<int32_t>(dir, "obs_start", n_points + 1);
    const auto obs         = load<int32_t>(dir, "obs", n_obs * 2);
    const auto pt_flags    = load<uint8_t>(dir, "pt_flags", n_points);
    const auto pt_pos      = load<double>(dir, "pt_pos", n_points * 3);
    const auto q           = load<int32_t>(dir, "q", n_q);
    const SimpMapView M{(int)n_kf,         (int)n_points,     (int)n_obs,         (int)n_feat,      kf_bad.data(),
                        kf_pose.data(),    feat_start.data(), feat_point.data(),  feat_depth.data(), feat_octave.data(),
                        obs_start.data(),  reinterpret_cast<const int32_t(*)[2]>(obs.data()), pt_flags.data(), pt_pos.data()};
    std::vector<uint32_t> keys((size_t)feat_cap);
    std::vector<SimpStats> out(n_q);
    for (size_t s = 0; s < n_q; ++s) out[s] = simp_stats_one(M, q[s], min_obs, stereo, th_depth, feat_cap, keys.data());
    save(dir, "stats", out);
    return 0;
}

static int run_decide(const std::string& dir)
{
    const auto meta = load<int32_t>(dir, "meta", 5);
    const size_t n_kf = (size_t)meta[0], n_list = (size_t)meta[1], n_q = (size_t)meta[2], nt = meta[4] ? n_kf : 0;
    const int node_cap     = meta[3];
    const auto params      = load<SimpParams>(dir, "params", 1);
    const auto kf_bad      = load<uint8_t>(dir, "kf_bad", n_kf);
    const auto kf_pose     = load<double>(dir, "kf_pose", n_kf * 7);
    const auto cull_factor = load<float>(dir, "kf_cull_factor", n_kf);
    const auto median      = load<double>(dir, "kf_median_depth", n_kf);
    const auto kf_prev     = load<int32_t>(dir, "kf_prev", nt);
    const auto kf_next     = load<int32_t>(dir, "kf_next", nt);
    const auto kf_time     = load<double>(dir, "kf_time", nt);
    const auto conn_start  = load<int32_t>(dir, "conn_start", n_kf + 1);
    const auto conn_list   = load<SimpConn>(dir, "conn_list", n_list);
    const auto q           = load<int32_t>(dir, "q", n_q);
    const auto stats       = load<SimpStats>(dir, "stats", n_q);
    const SimpGraphView G{(int)n_kf,     (int)n_list,   kf_bad.data(), kf_pose.data(), cull_factor.data(), median.data(), nt ? kf_prev.data() : nullptr,
                          nt ? kf_next.data() : nullptr, nt ? kf_time.data() : nullptr, conn_start.data(), conn_list.data()};
    std::vector<int> node_kf((size_t)node_cap);
    std::vector<uint64_t> sorted((size_t)node_cap);
    std::vector<int32_t> tri((size_t)node_cap * (size_t)node_cap / 2 + 1);
    std::vector<SimpVerdict> out(n_q);
    for (size_t s = 0; s < n_q; ++s) out[s] = simp_decide_one(G, params[0], q[s], stats[s], node_cap, node_kf.data(), sorted.data(), tri.data());
    save(dir, "verdict", out);
    return 0;
}

static int run_angles(const std::string& dir)
{
    const auto meta    = load<int32_t>(dir, "meta", 2);
    const size_t n_kf  = (size_t)meta[0], n = (size_t)meta[1];
    const auto kf_pose = load<double>(dir, "kf_pose", n_kf * 7);
    const auto median  = load<double>(dir, "kf_median_depth", n_kf);
    const auto pairs   = load<int32_t>(dir, "pairs", n * 2);
    std::vector<double> out(n);
    for (size_t i = 0; i < n; ++i)
    {
        const int a = pairs[2 * i], b = pairs[2 * i + 1];
        out[i]      = simp_angle(median[a], median[b], kf_pose.data() + 7 * (size_t)a, kf_pose.data() + 7 * (size_t)b);
    }
    save(dir, "angles", out);
    return 0;
}

static int run_select(const std::string& dir)
{
    const int n  = load<int32_t>(dir, "meta", 1)[0];
    const auto z = load<float>(dir, "z", (size_t)n);
    std::vector<uint32_t> keys((size_t)n);
    for (int i = 0; i < n; ++i) keys[(size_t)i] = simp_key(z[(size_t)i]);
    const uint32_t k = simp_select(
        [&](uint32_t T) {
            int c = 0;
            for (int i = 0; i < n; ++i) c += keys[(size_t)i] < T ? 1 : 0;
            return c;
        },
        simp_median_rank(n));
    save(dir, "median", std::vector<float>{simp_unkey(k)});
    return 0;
}

int main(int argc, char** argv)
{
    try
    {
        if (argc == 2 && std::strcmp(argv[1], "--consts") == 0)
        {
            std::printf("threads %d long_min %d long_min_env0 %d long_min_env7 %d max_nodes %d max_feat %d stats_carve_max %zu stats_carve_1 %zu stats_carve_4096 %zu "
                        "decide_carve_max %zu decide_carve_1 %zu decide_carve_16 %zu decide_carve_64 %zu\n",
                        SIMP_THREADS, simp_long_min(-1), simp_long_min(0), simp_long_min(7), SIMP_MAX_NODES, SIMP_MAX_FEAT, simp_stats_carve(SIMP_MAX_FEAT),
                        simp_stats_carve(1), simp_stats_carve(4096), simp_decide_carve(SIMP_MAX_NODES), simp_decide_carve(1), simp_decide_carve(16),
                        simp_decide_carve(64));
            return 0;
        }
        if (argc != 3) throw std::runtime_error("usage: simp_core_driver stats|decide|angles|select DIR | --consts");
        const std::string mode = argv[1];
        if (mode == "stats") return run_stats(argv[2]);
        if (mode == "decide") return run_decide(argv[2]);
        if (mode == "angles") return run_angles(argv[2]);
        if (mode == "select") return run_select(argv[2]);
        throw std::runtime_error("simp_core_driver: unknown mode");
    }
    catch (const std::exception& e)
    {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
