// CPU build of snake_slam_amd/csrc/lmap_core.hpp and the local-map part of dispatch.hpp (plain g++, no HIP): the draw, the accept rule,
// the hash and the skip rules on rows of inputs, for tests/test_localmap_core_cpu.py.
//   lmap_core_driver DIR        reads rows.bin: int64 rows of (seed, frame_id, c, k, n, h, id, flags, last_seen, kf_bad, marked, vote
//                               status, n_found, n_conn, vote_cap); writes out.bin: int64 rows of (key, draw, accept of the draw,
//                               accept of h, hash, kf point skipped, own point skipped, neighbour listed, vote status)
//   lmap_core_driver --consts   the limits, the table sizes and the carves
#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "lmap_core.hpp"
#include "dispatch.hpp"

using namespace snk;

int main(int argc, char** argv)
{
    try
    {
        if (argc == 2 && std::strcmp(argv[1], "--consts") == 0)
        {
            std::printf("threads %d max_local_kf %d max_pts %d max_neighbours %d max_order %d slots_1 %d slots_64 %d slots_256 %d slots_257 %d slots_max %d "
                        "sort_len_64_5 %d sort_len_max %d select_carve_max %zu select_carve_4096_64_5 %zu gather_carve_max %zu gather_carve_64_2048 %zu\n",
                        LMAP_THREADS, LMAP_MAX_LOCAL_KF, LMAP_MAX_PTS, LMAP_MAX_NEIGHBOURS, LMAP_MAX_ORDER, lmap_table_slots(1), lmap_table_slots(64),
                        lmap_table_slots(256), lmap_table_slots(257), lmap_table_slots(LMAP_MAX_PTS), lmap_sort_len(64, 5),
                        lmap_sort_len(LMAP_MAX_LOCAL_KF, LMAP_MAX_NEIGHBOURS), lmap_select_carve(32768, LMAP_MAX_LOCAL_KF, LMAP_MAX_NEIGHBOURS),
                        lmap_select_carve(4096, 64, 5), lmap_gather_carve(LMAP_MAX_LOCAL_KF, LMAP_MAX_PTS), lmap_gather_carve(64, 2048));
            return 0;
        }
        if (argc != 2) throw std::runtime_error("usage: lmap_core_driver DIR | --consts");
        const std::string dir = argv[1];
        std::ifstream f(dir + "/rows.bin", std::ios::binary | std::ios::ate);
        if (!f) throw std::runtime_error("lmap_core_driver: missing rows.bin");
        const size_t bytes = (size_t)f.tellg(), n = bytes / (15 * sizeof(int64_t));
        std::vector<int64_t> in(n * 15), out(n * 9);
        f.seekg(0);
        f.read(reinterpret_cast<char*>(in.data()), (std::streamsize)(n * 15 * sizeof(int64_t)));
        for (size_t r = 0; r < n; ++r)
        {
            const int64_t* a   = in.data() + r * 15;
            int64_t* o         = out.data() + r * 9;
            const uint32_t key = lmap_key((uint64_t)a[0], (int32_t)a[1]);
            const uint32_t h   = lmap_draw(key, (uint32_t)a[2]);
            o[0] = key;
            o[1] = h;
            o[2] = lmap_accept(h, (int)a[3], (int)a[4]);
            o[3] = lmap_accept((uint32_t)a[5], (int)a[3], (int)a[4]);
            o[4] = lmap_hash((int32_t)a[6]);
            o[5] = lmap_kf_point_skipped((int)a[6], (unsigned)a[7], (int)a[8], (int)a[1]);
            o[6] = lmap_own_point_skipped((int)a[6], (unsigned)a[7]);
            o[7] = lmap_neighbour_listed((unsigned)a[9], a[10] != 0);
            o[8] = lmap_vote_status((int)a[11], (int)a[12], (int)a[13], (int)a[14]);
        }
        std::ofstream g(dir + "/out.bin", std::ios::binary);
        g.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)(out.size() * sizeof(int64_t)));
        return 0;
    }
    catch (const std::exception& e)
    {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
