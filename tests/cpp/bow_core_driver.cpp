// CPU build of bow_core.hpp (tests/test_bow_core_cpu.py, tools/probes/bow_timing.py).  <dir> holds the vocabulary as flat arrays
// (v_child_start.bin, v_child_count.bin, v_children.bin, v_word.bin: int32; v_desc.bin: n x 4 uint64; v_weight.bin: doubles); the tree
// is validated with bow_validate first (status 2 and the reason on stderr when it is not sound).
//   bow_core_driver <dir> transform <levelsup>          desc.bin (n x 4 uint64) -> out_word.bin, out_node.bin (int32 per descriptor)
//   bow_core_driver <dir> match <threshold> <ratio>     desc{1,2}.bin, has{1,2}.bin (uint8), nid{1,2}.bin, ns{1,2}.bin, ft{1,2}.bin (int32)
//                                                       -> out_m12.bin (int32 per feature of keyframe 1)
//   bow_core_driver <dir> time <levelsup> <repeats>     prints the seconds one single-threaded pass over desc.bin takes (best of repeats)
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "bow_core.hpp"

template <typename T>
static std::vector<T> read_all(const std::string& path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error("bow_core_driver: missing input " + path);
    const std::streamsize bytes = f.tellg();
    f.seekg(0);
    std::vector<T> v((size_t)bytes / sizeof(T));
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
    return v;
}

template <typename T>
static void write_all(const std::string& path, const std::vector<T>& v)
{
    std::ofstream(path, std::ios::binary).write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

struct Side
{
    std::vector<uint64_t> desc;
    std::vector<uint8_t> has;
    std::vector<int32_t> nid, ns, ft;
    Side(const std::string& dir, const char* k)
        : desc(read_all<uint64_t>(dir + "/desc" + k + ".bin")), has(read_all<uint8_t>(dir + "/has" + k + ".bin")),
          nid(read_all<int32_t>(dir + "/nid" + k + ".bin")), ns(read_all<int32_t>(dir + "/ns" + k + ".bin")),
          ft(read_all<int32_t>(dir + "/ft" + k + ".bin"))
    {
        if (ns.size() != nid.size() + 1 || has.size() * 4 != desc.size()) throw std::runtime_error("bow_core_driver: inconsistent keyframe arrays");
        for (size_t i = 0; i < nid.size(); ++i)
            if (ns[i] < 0 || ns[i] > ns[i + 1] || (size_t)ns[i + 1] > ft.size()) throw std::runtime_error("bow_core_driver: bad node_start");
        for (int32_t f : ft)
            if (f < 0 || (size_t)f >= has.size()) throw std::runtime_error("bow_core_driver: feature index out of range");
    }
};

// LoopORBMatcher.cpp:121-215 over the statements of bow_core.hpp
static std::vector<int32_t> match_bow(const Side& A, const Side& B, int threshold, float ratio)
{
    std::vector<int32_t> m12(A.has.size(), -1);
    std::vector<uint8_t> matched(B.has.size(), 0);
    size_t i = 0, j = 0;
    while (i < A.nid.size() && j < B.nid.size())
    {
        if (A.nid[i] < B.nid[j])
            ++i;
        else if (B.nid[j] < A.nid[i])
            ++j;
        else
        {
            for (int p = A.ns[i]; p < A.ns[i + 1]; ++p)
            {
                const int f1 = A.ft[p];
                if (!A.has[f1]) continue;
                uint32_t k1 = snk::BOW_MATCH_NONE, k2 = snk::BOW_MATCH_NONE;
                for (int q = B.ns[j]; q < B.ns[j + 1]; ++q)
                {
                    const int f2 = B.ft[q];
                    if (!B.has[f2] || matched[f2]) continue;
                    snk::bow_match_update(snk::bow_match_key(snk::bow_distance(&A.desc[(size_t)f1 * 4], &B.desc[(size_t)f2 * 4]), q - B.ns[j]), k1, k2);
                }
                if (k1 != snk::BOW_MATCH_NONE && snk::bow_match_accept(k1, k2, threshold, ratio))
                {
                    const int f2 = B.ft[B.ns[j] + (int)(k1 & 0xffffu)];
                    matched[f2]  = 1;
                    m12[f1]      = f2;
                }
            }
            ++i;
            ++j;
        }
    }
    return m12;
}

int main(int argc, char** argv)
{
    try
    {
        if (argc < 3) throw std::runtime_error("bow_core_driver: usage: <dir> transform|match|time ...");
        const std::string dir = argv[1], mode = argv[2];
        const auto cs = read_all<int32_t>(dir + "/v_child_start.bin"), cc = read_all<int32_t>(dir + "/v_child_count.bin"),
                   ch = read_all<int32_t>(dir + "/v_children.bin"), wd = read_all<int32_t>(dir + "/v_word.bin");
        const auto vd = read_all<uint64_t>(dir + "/v_desc.bin");
        const auto wt = read_all<double>(dir + "/v_weight.bin");
        const int n_nodes = (int)cs.size();
        if (cc.size() != cs.size() || wd.size() != cs.size() || wt.size() != cs.size() || vd.size() != cs.size() * 4)
            throw std::runtime_error("bow_core_driver: per-node arrays differ in length");
        std::vector<int32_t> scratch(cs.size());
        int L = 0, n_words = 0;
        const char* why = snk::bow_validate(n_nodes, cs.data(), cc.data(), ch.data(), (int)ch.size(), wd.data(), wt.data(), scratch.data(), &L, &n_words);
        if (why != nullptr)
        {
            std::cerr << "bow_core_driver: invalid vocabulary: " << why << "\n";
            return 2;
        }
        // the walk's layout: slot = position in children[], the child's descriptor beside it
        std::vector<uint64_t> slot_desc(ch.size() * 4 + 4);
        for (size_t s = 0; s < ch.size(); ++s)
            for (int k = 0; k < 4; ++k) slot_desc[s * 4 + k] = vd[(size_t)ch[s] * 4 + k];
        const snk::BowTree T{cs.data(), cc.data(), ch.data(), slot_desc.data(), wd.data(), wt.data(), L};

        if (mode == "transform" || mode == "time")
        {
            if (argc < 4) throw std::runtime_error("bow_core_driver: levelsup missing");
            const int levelsup = atoi(argv[3]);
            const auto desc    = read_all<uint64_t>(dir + "/desc.bin");
            const size_t n     = desc.size() / 4;
            std::vector<int32_t> word(n), node(n);
            const int repeats = mode == "time" ? (argc > 4 ? atoi(argv[4]) : 3) : 1;
            double best       = 1e300;
            for (int r = 0; r < repeats; ++r)
            {
                const auto t0 = std::chrono::steady_clock::now();
                for (size_t i = 0; i < n; ++i)
                {
                    int leaf = 0, up = 0;
                    snk::bow_transform_one(T, &desc[i * 4], levelsup, leaf, up);
                    word[i] = wd[leaf];
                    node[i] = up;
                }
                const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                best            = dt < best ? dt : best;
            }
            if (mode == "time")
                printf("%.9f\n", best);
            else
            {
                write_all(dir + "/out_word.bin", word);
                write_all(dir + "/out_node.bin", node);
            }
        }
        else if (mode == "match")
        {
            if (argc < 5) throw std::runtime_error("bow_core_driver: threshold / ratio missing");
            const Side A(dir, "1"), B(dir, "2");
            write_all(dir + "/out_m12.bin", match_bow(A, B, atoi(argv[3]), (float)atof(argv[4])));
        }
        else
            throw std::runtime_error("bow_core_driver: unknown mode " + mode);
        return 0;
    }
    catch (const std::exception& e)
    {
        std::cerr << e.what() << "\n";
        return 1;
    }
}
