// CPU build of snake_slam_amd/csrc/covis_core.hpp and the covisibility part of dispatch.hpp (plain g++, no HIP): the statements the
// kernel runs per set -- gate, count, emit rule, key, cut -- on one thread, for tests/test_covis_core_cpu.py.
//   covis_core_driver DIR        reads meta.bin (int32: form 0 = connection / 1 = vote, n_kf, n_points, n_obs, n_items, n_sets, th, cap),
//                                th_depth.bin (float) and the tables kf_bad / obs_start / obs / pt_flags / item_start / item_point /
//                                item_depth / q (.bin) from DIR; writes conn.bin ([n_sets][cap], (-1, -1) where not written) and res.bin
//   covis_core_driver --consts   the long-list threshold under SNK_COVIS_LONG_MIN unset / 0 / 7 and the carves
#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "covis_core.hpp"
#include "dispatch.hpp"

using namespace snk;

template <typename T>
static std::vector<T> load(const std::string& dir, const char* name, size_t n)
{
    std::vector<T> v(n);
    if (n == 0) return v;
    std::ifstream f(dir + "/" + name + ".bin", std::ios::binary);
    if (!f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(T)))) throw std::runtime_error(std::string("covis_core_driver: missing input ") + name);
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
        if (argc == 2 && std::strcmp(argv[1], "--consts") == 0)
        {
            std::printf("long_min %d long_min_env0 %d long_min_env7 %d threads %d max_kf %d max_cap %d carve_max %zu carve_4096_64 %zu carve_1_1 %zu sort_len_1000_64 %d "
                        "sort_len_40_64 %d sort_len_max %d\n",
                        covis_long_min(-1), covis_long_min(0), covis_long_min(7), COVIS_THREADS, COVIS_MAX_KF, COVIS_MAX_CAP,
                        covis_carve(COVIS_MAX_KF, COVIS_MAX_CAP), covis_carve(4096, 64), covis_carve(1, 1), covis_sort_len(1000, 64), covis_sort_len(40, 64),
                        covis_sort_len(COVIS_MAX_KF, COVIS_MAX_CAP));
            return 0;
        }
        if (argc != 2) throw std::runtime_error("usage: covis_core_driver DIR | --consts");
        const std::string dir = argv[1];
        const auto meta       = load<int32_t>(dir, "meta", 8);
        const int form = meta[0], n_kf = meta[1], n_points = meta[2], n_obs = meta[3], n_items = meta[4], n_sets = meta[5], th = meta[6], cap = meta[7];
        const float th_depth  = load<float>(dir, "th_depth", 1)[0];
        const auto kf_bad     = load<uint8_t>(dir, "kf_bad", (size_t)n_kf);
        const auto obs_start  = load<int32_t>(dir, "obs_start", (size_t)n_points + 1);
        const auto obs        = load<int32_t>(dir, "obs", (size_t)n_obs * 2);
        const auto pt_flags   = load<uint8_t>(dir, "pt_flags", (size_t)n_points);
        const auto item_start = load<int32_t>(dir, "item_start", (size_t)(form == 0 ? n_kf : n_sets) + 1);
        const auto item_point = load<int32_t>(dir, "item_point", (size_t)n_items);
        const auto item_depth = load<float>(dir, "item_depth", form == 0 ? (size_t)n_items : 0);
        const auto q          = load<int32_t>(dir, "q", form == 0 ? (size_t)n_sets : 0);
        std::vector<CovisConn> conn((size_t)n_sets * (size_t)cap, CovisConn{-1, -1});
        std::vector<CovisResult> res((size_t)n_sets);
        std::vector<uint32_t> count((size_t)n_kf);
        const int32_t(*obs2)[2] = reinterpret_cast<const int32_t(*)[2]>(obs.data());
        for (int s = 0; s < n_sets; ++s)
        {
            std::fill(count.begin(), count.end(), 0u);
            CovisConn* row = conn.data() + (size_t)s * (size_t)cap;
            if (form == 0)
                res[s] = covis_set<true, true, true, true>(n_kf, kf_bad.data(), obs_start.data(), obs2, pt_flags.data(), item_start[q[s]], item_start[q[s] + 1],
                                                           item_point.data(), item_depth.data(), q[s], th, th_depth, cap, count.data(), row);
            else
                res[s] = covis_set<false, false, false, false>(n_kf, kf_bad.data(), obs_start.data(), obs2, pt_flags.data(), item_start[s], item_start[s + 1],
                                                               item_point.data(), nullptr, -1, th, th_depth, cap, count.data(), row);
        }
        save(dir, "conn", conn);
        save(dir, "res", res);
        return 0;
    }
    catch (const std::exception& e)
    {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
