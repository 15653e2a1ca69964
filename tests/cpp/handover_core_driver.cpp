// CPU build of snake_slam_amd/csrc/handover_core.hpp (plain g++, no HIP) for tests/test_handover_core_cpu.py: the statements the host
// builder and the device stage of the BA hand-over share, run over problems both ways.
//   handover_core_driver DIR       reads in.bin (int32): the number of problems, then per problem n_img, n_pt, n_obs, img_const [n_img],
//                                  pt_const [n_pt], obs_img [n_obs], obs_pt [n_obs].  Writes out.bin (int32), per problem: nfc, no, k_over8,
//                                  dup, long_run, cam_idx [n_img], pt_start [n_pt + 1], valid [n_obs], then for every sorted slot its caller
//                                  index [no] and its free-camera index [no].
//                                  Every problem is built twice: the way fill_problem / size_pass do (one pass in caller order, a cursor per
//                                  point, a set of seen cameras per point) and the way ho_count_kernel / ho_fill_kernel do (histogram, prefix
//                                  sums, chunks of HO_THREADS ranked by ho_chunk_rank, one cursor writer per point and chunk, the dup rule on
//                                  the sorted runs); the two must agree or the driver fails.
//   handover_core_driver --consts  the plan: limits, carves, the take / stage decisions at their edges
#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "dispatch.hpp"  // includes handover_core.hpp, where the plan lives

using namespace snk;

struct Built
{
    int nfc = 0, no = 0, k_over8 = 0, dup = 0, long_run = 0;
    std::vector<int32_t> cam_idx, pt_start, valid, order, o_cam;
    bool operator==(const Built& o) const
    {
        return nfc == o.nfc && no == o.no && k_over8 == o.k_over8 && dup == o.dup && long_run == o.long_run && cam_idx == o.cam_idx && pt_start == o.pt_start &&
               valid == o.valid && order == o.order && o_cam == o.o_cam;
    }
};

struct Problem
{
    int n_img, n_pt, n_obs;
    std::vector<uint8_t> img_const, pt_const;
    std::vector<int32_t> obs_img, obs_pt;
};

// fill_problem / size_pass of ba_handover.hip, list for list
static Built host_way(const Problem& P)
{
    Built B;
    B.cam_idx.resize((size_t)P.n_img), B.pt_start.assign((size_t)P.n_pt + 1, 0), B.valid.assign((size_t)P.n_obs, 0);
    for (int i = 0; i < P.n_img; ++i)
    {
        B.cam_idx[(size_t)i] = ho_cam_index(P.img_const[(size_t)i] != 0, B.nfc);
        B.nfc += P.img_const[(size_t)i] ? 0 : 1;
    }
    std::vector<int> kfree((size_t)P.n_pt, 0);
    for (int o = 0; o < P.n_obs; ++o)
    {
        const int i = P.obs_img[(size_t)o], p = P.obs_pt[(size_t)o];
        if (ho_obs_by_free_camera(i, p, P.n_img, P.n_pt, P.img_const.data()) && ho_k_over8(++kfree[(size_t)p])) B.k_over8 = 1;
        if (!ho_obs_valid(i, p, P.n_img, P.n_pt, P.img_const.data(), P.pt_const.data())) continue;
        B.valid[(size_t)o] = 1;
        B.pt_start[(size_t)p + 1]++;
        ++B.no;
    }
    for (int p = 0; p < P.n_pt; ++p)
    {
        if (!ho_run_taken(B.pt_start[(size_t)p + 1])) B.long_run = 1;
        B.pt_start[(size_t)p + 1] += B.pt_start[(size_t)p];
    }
    const int words = ho_dup_words(B.nfc);
    std::vector<unsigned long long> seen((size_t)P.n_pt * (size_t)words, 0ull);
    std::vector<int> fill(B.pt_start.begin(), B.pt_start.end() - 1);
    B.order.assign((size_t)B.no, -1), B.o_cam.assign((size_t)B.no, -2);
    for (int o = 0; o < P.n_obs; ++o)
    {
        if (!B.valid[(size_t)o]) continue;
        const int i = P.obs_img[(size_t)o], p = P.obs_pt[(size_t)o], sl = fill[(size_t)p]++, c = B.cam_idx[(size_t)i];
        if (c >= 0 && words)
        {
            unsigned long long& word = seen[(size_t)p * (size_t)words + (size_t)(c >> 6)];
            if (word & (1ull << (c & 63))) B.dup = 1;
            word |= 1ull << (c & 63);
        }
        B.order[(size_t)sl] = o, B.o_cam[(size_t)sl] = c;
    }
    return B;
}

// ho_count_kernel / ho_fill_kernel, a loop over t where the kernel has lanes
static Built device_way(const Problem& P)
{
    Built B;
    B.cam_idx.resize((size_t)P.n_img), B.pt_start.assign((size_t)P.n_pt + 1, 0), B.valid.assign((size_t)P.n_obs, 0);
    for (int i = 0, before = 0; i < P.n_img; ++i)
    {
        const bool free = !P.img_const[(size_t)i];
        B.cam_idx[(size_t)i] = ho_cam_index(!free, before);
        before += free ? 1 : 0;
        B.nfc = before;
    }
    std::vector<int> cnt((size_t)P.n_pt, 0), kfree((size_t)P.n_pt, 0);
    for (int o = P.n_obs - 1; o >= 0; --o)  // (any order: the additions commute)
    {
        const int i = P.obs_img[(size_t)o], p = P.obs_pt[(size_t)o];
        if (ho_obs_valid(i, p, P.n_img, P.n_pt, P.img_const.data(), P.pt_const.data())) cnt[(size_t)p]++;
        if (ho_obs_by_free_camera(i, p, P.n_img, P.n_pt, P.img_const.data())) kfree[(size_t)p]++;
    }
    for (int p = 0; p < P.n_pt; ++p)
    {
        B.pt_start[(size_t)p] = B.no;
        B.no += cnt[(size_t)p];
        if (ho_k_over8(kfree[(size_t)p])) B.k_over8 = 1;
        if (!ho_run_taken(cnt[(size_t)p])) B.long_run = 1;
    }
    B.pt_start[(size_t)P.n_pt] = B.no;
    std::vector<int> cur(B.pt_start.begin(), B.pt_start.end() - 1);
    B.order.assign((size_t)B.no, -1), B.o_cam.assign((size_t)B.no, -2);
    alignas(16) int32_t keys[HO_THREADS];
    for (int c0 = 0; c0 < P.n_obs; c0 += HO_THREADS)
    {
        for (int t = 0; t < HO_THREADS; ++t)
        {
            const int o = c0 + t;
            const bool v = o < P.n_obs && ho_obs_valid(P.obs_img[(size_t)o], P.obs_pt[(size_t)o], P.n_img, P.n_pt, P.img_const.data(), P.pt_const.data());
            if (o < P.n_obs) B.valid[(size_t)o] = v ? 1 : 0;
            keys[t] = v ? P.obs_pt[(size_t)o] : -1;
        }
        std::vector<int> advance_pt, advance_to;
        for (int t = HO_THREADS - 1; t >= 0; --t)  // (any order: the cursors are read before any is written)
        {
            if (keys[t] < 0) continue;
            int before, total;
            ho_chunk_rank(keys, HO_THREADS / 4, t, before, total);
            const int base = cur[(size_t)keys[t]], o = c0 + t;
            if (before + 1 == total) advance_pt.push_back(keys[t]), advance_to.push_back(base + total);
            B.order[(size_t)(base + before)] = o, B.o_cam[(size_t)(base + before)] = B.cam_idx[(size_t)P.obs_img[(size_t)o]];
        }
        for (size_t k = 0; k < advance_pt.size(); ++k) cur[(size_t)advance_pt[k]] = advance_to[k];
    }
    if (ho_dup_words(B.nfc) > 0)
        for (int s = 0; s < B.no; ++s)
        {
            int lo = -1, hi = P.n_pt - 1;  // cur[p] is now the end of p's run
            while (hi - lo > 1)
            {
                const int mid = (lo + hi) >> 1;
                if (cur[(size_t)mid] <= s) lo = mid;
                else hi = mid;
            }
            if (ho_cam_seen_before(B.o_cam.data(), hi > 0 ? cur[(size_t)hi - 1] : 0, s)) B.dup = 1;
        }
    return B;
}

int main(int argc, char** argv)
{
    try
    {
        if (argc == 2 && std::strcmp(argv[1], "--consts") == 0)
        {
            std::printf("threads %d max_pts %d max_run %d misc %d dup_max_cams %d big_max_free %d count_carve_max %zu fill_carve_max %zu carve_max %zu "
                        "count_carve_1000 %zu fill_carve_1000 %zu takes_at_limit %d takes_past_limit %d run_at_limit %d run_past_limit %d dup_words_512 %d "
                        "dup_words_513 %d dup_words_65 %d\n",
                        HO_THREADS, HO_MAX_PTS, HO_MAX_RUN, HO_MISC, HO_DUP_MAX_CAMS, HO_BIG_MAX_FREE, ho_count_carve(HO_MAX_PTS), ho_fill_carve(HO_MAX_PTS),
                        ho_carve_max(), ho_count_carve(1000), ho_fill_carve(1000), (int)ho_kernels_take(HO_MAX_PTS), (int)ho_kernels_take(HO_MAX_PTS + 1),
                        (int)ho_run_taken(HO_MAX_RUN), (int)ho_run_taken(HO_MAX_RUN + 1), ho_dup_words(512), ho_dup_words(513), ho_dup_words(65));
            return 0;
        }
        if (argc != 2) throw std::runtime_error("usage: handover_core_driver DIR | --consts");
        const std::string dir = argv[1];
        std::ifstream f(dir + "/in.bin", std::ios::binary | std::ios::ate);
        if (!f) throw std::runtime_error("handover_core_driver: missing in.bin");
        std::vector<int32_t> in((size_t)f.tellg() / 4);
        f.seekg(0);
        f.read(reinterpret_cast<char*>(in.data()), (std::streamsize)(in.size() * 4));
        size_t at = 0;
        auto take = [&](size_t n)
        {
            if (at + n > in.size()) throw std::runtime_error("handover_core_driver: in.bin is short");
            const int32_t* p = in.data() + at;
            at += n;
            return p;
        };
        const int n_prob = *take(1);
        std::vector<int32_t> out;
        for (int k = 0; k < n_prob; ++k)
        {
            Problem P;
            const int32_t* hd = take(3);
            P.n_img = hd[0], P.n_pt = hd[1], P.n_obs = hd[2];
            const int32_t* a = take((size_t)P.n_img);
            P.img_const.assign(a, a + P.n_img);
            a = take((size_t)P.n_pt);
            P.pt_const.assign(a, a + P.n_pt);
            a = take((size_t)P.n_obs);
            P.obs_img.assign(a, a + P.n_obs);
            a = take((size_t)P.n_obs);
            P.obs_pt.assign(a, a + P.n_obs);
            const Built H = host_way(P), D = device_way(P);
            if (!(H == D)) throw std::runtime_error("handover_core_driver: problem " + std::to_string(k) + ": the chunked walk differs from the host builder's pass");
            for (int v : {H.nfc, H.no, H.k_over8, H.dup, H.long_run}) out.push_back(v);
            out.insert(out.end(), H.cam_idx.begin(), H.cam_idx.end());
            out.insert(out.end(), H.pt_start.begin(), H.pt_start.end());
            out.insert(out.end(), H.valid.begin(), H.valid.end());
            out.insert(out.end(), H.order.begin(), H.order.end());
            out.insert(out.end(), H.o_cam.begin(), H.o_cam.end());
        }
        std::ofstream g(dir + "/out.bin", std::ios::binary);
        g.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)(out.size() * 4));
        return 0;
    }
    catch (const std::exception& e)
    {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
