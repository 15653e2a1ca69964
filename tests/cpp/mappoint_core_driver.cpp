// Plain g++ build of snake_slam_amd/csrc/mappoint_core.hpp and of the map-point part of dispatch.hpp (no HIP anywhere):
//   mappoint_core_driver <dir>             the per-point statements of "snk-mp v1" over the raw arrays in <dir> (written and read by
//                                          tests/test_mappoint_core_cpu.py, which compares with the numpy restatement bit for bit)
//   mappoint_core_driver --forms E k ...   "k form" per line under SNK_MP_FORM = E (0 unset, 1 packed, 2 wide), then the carves
//   mappoint_core_driver --select          mp_select and mp_select8 against sorted rows, for every rank
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "dispatch.hpp"
#include "mappoint_core.hpp"
#include "snake_hip.h"

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

int main(int argc, char** argv)
{
    using namespace snk;
    static_assert(MP_MAX_OBS == SNK_MP_MAX_OBS && MP_WIDE_MAX_K == SNK_MP_MAX_OBS && sizeof(snk_mp_result) == 80, "snk-mp constants");
    if (argc >= 3 && std::string(argv[1]) == "--forms")
    {
        const int env = atoi(argv[2]);
        for (int i = 3; i < argc; ++i)
        {
            const int k = atoi(argv[i]);
            printf("%d %s\n", k, mp_form(k, env) == MpForm::packed ? "packed" : "wide");
        }
        printf("packed_max_k %d chunk_points %d packed_rows_max %d packed_carve_max %zu wide_carve_max %zu\n", MP_PACKED_MAX_K, MP_CHUNK_POINTS,
               mp_packed_rows_max(), mp_packed_carve(mp_packed_rows_max()), mp_wide_carve(MP_WIDE_MAX_K));
        return 0;
    }
    if (argc >= 2 && std::string(argv[1]) == "--select")
    {
        // mp_select (nine halvings) and mp_select8 (three eight-way passes) against the sorted row, for every rank of random rows
        uint64_t state = 88172645463325252ull;
        auto next      = [&] { state ^= state << 13, state ^= state >> 7, state ^= state << 17; return state; };
        long checked = 0;
        for (int row = 0; row < 3000; ++row)
        {
            const int n = 1 + (int)(next() % (row % 10 == 0 ? 300 : 40));
            const int spread = row % 3 == 0 ? 257 : row % 3 == 1 ? 9 : 40;  // the whole range, near-ties, a cluster
            const int base   = (int)(next() % (257 - spread + 1));
            std::vector<int> d((size_t)n);
            for (int& v : d) v = base + (int)(next() % spread);
            std::vector<int> sorted = d;
            std::sort(sorted.begin(), sorted.end());
            for (int rank = 1; rank <= n; ++rank, ++checked)
            {
                const int a = mp_select([&](int v) { int c = 0; for (int x : d) c += x <= v; return c; }, rank);
                const int b = mp_select8(
                    [&](const int(&t)[7], int(&c)[7]) {
                        for (int q = 0; q < 7; ++q) c[q] = 0;
                        for (int x : d)
                            for (int q = 0; q < 7; ++q) c[q] += x <= t[q];
                    },
                    rank);
                if (a != sorted[(size_t)rank - 1] || b != sorted[(size_t)rank - 1])
                {
                    printf("row %d rank %d: sorted %d, mp_select %d, mp_select8 %d\n", row, rank, sorted[(size_t)rank - 1], a, b);
                    return 1;
                }
            }
        }
        printf("ok %ld\n", checked);
        return 0;
    }
    if (argc < 2) return 2;
    g_dir = argv[1];
    try
    {
        const auto meta  = rd<int32_t>("meta");  // rule, what, select by mp_select8 instead of mp_select
        const auto start = rd<int32_t>("obs_start");
        const auto desc  = rd<uint64_t>("desc");
        const auto pose  = rd<double>("pose");
        const auto oct   = rd<int32_t>("octave");
        const auto valid = rd<uint8_t>("valid");
        const auto pos   = rd<double>("position");
        const auto ref   = rd<int32_t>("ref_obs");
        const int n      = (int)start.size() - 1;
        std::vector<snk_mp_result> out((size_t)(n > 0 ? n : 0));
        for (int p = 0; p < n; ++p)
        {
            const int a = start[p], k = start[p + 1] - a;
            snk_mp_result r{};
            r.best = -1, r.ref_level = -1;
            const auto* d  = reinterpret_cast<const uint64_t(*)[4]>(desc.data()) + a;
            const auto* ps = reinterpret_cast<const double(*)[7]>(pose.data()) + a;
            int N          = 0;
            const int best = mp_best_descriptor(d, valid.data() + a, k, meta[0], &N, meta.size() > 2 && meta[2] != 0);
            r.n_valid      = N;
            if ((meta[1] & MP_DESCRIPTOR) && best >= 0)
            {
                r.best = best;
                memcpy(r.desc, d[best], 32);
            }
            if (meta[1] & MP_NORMAL) mp_normal(ps, valid.data() + a, k, &pos[(size_t)p * 3], r.normal);
            if ((meta[1] & MP_DEPTH) && ref[p] >= 0)
            {
                r.ref_depth = mp_ref_depth(ps[ref[p]], &pos[(size_t)p * 3]);
                r.ref_level = oct[a + ref[p]];
            }
            out[p] = r;
        }
        std::ofstream f(g_dir + "/out.bin", std::ios::binary);
        f.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)(out.size() * sizeof(snk_mp_result)));
    }
    catch (const std::exception& e)
    {
        std::cerr << "mappoint_core_driver: " << e.what() << "\n";
        return 1;
    }
    return 0;
}
