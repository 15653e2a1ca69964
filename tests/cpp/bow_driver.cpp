// snake_hip::ORBVocabulary / KeyframeDatabase / LoopORBmatcher of the C++ adaptor, used as the loop closer uses them
// (tests/test_cpp_bow_gpu.py).  <dir> holds the vocabulary as flat arrays (v_child_start.bin, v_child_count.bin, v_children.bin,
// v_word.bin: int32; v_desc.bin: n x 4 uint64; v_weight.bin: doubles), the descriptors of three keyframes (desc0.bin .. desc2.bin) and
// the map-point flags of the first two (has0.bin, has1.bin: uint8).  Writes per keyframe the bow vector (out_words<i>.bin int32,
// out_values<i>.bin double) and the feature vector (out_nodes<i>.bin uint32, out_ns<i>.bin, out_ft<i>.bin int32), out_score.bin (score of
// keyframes 0 and 1), out_loop.bin / out_reloc.bin (id, then the float score's bits, per candidate: int32 pairs), out_m12.bin and
// out_meta.bin (vocabulary size, matches, loop candidates, relocalisation candidates).
#include <cstdio>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "snake_hip.hpp"

template <typename T>
static std::vector<T> read_all(const std::string& path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error("bow_driver: missing input " + path);
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

static std::vector<int32_t> flat(const std::vector<std::pair<int, float>>& c)
{
    std::vector<int32_t> out;
    for (const auto& e : c)
    {
        int32_t bits;
        std::memcpy(&bits, &e.second, 4);
        out.push_back(e.first);
        out.push_back(bits);
    }
    return out;
}

int main(int argc, char** argv)
{
    try
    {
        const std::string dir = argc > 1 ? argv[1] : ".";
        snake_hip::VocabularyArrays a;
        a.child_start = read_all<int32_t>(dir + "/v_child_start.bin");
        a.child_count = read_all<int32_t>(dir + "/v_child_count.bin");
        a.children    = read_all<int32_t>(dir + "/v_children.bin");
        a.word_id     = read_all<int32_t>(dir + "/v_word.bin");
        a.desc        = read_all<snake_hip::DescriptorORB>(dir + "/v_desc.bin");
        a.weight      = read_all<double>(dir + "/v_weight.bin");
        std::vector<std::vector<snake_hip::DescriptorORB>> desc;
        for (int i = 0; i < 3; ++i) desc.push_back(read_all<snake_hip::DescriptorORB>(dir + "/desc" + std::to_string(i) + ".bin"));
        const auto has0 = read_all<uint8_t>(dir + "/has0.bin"), has1 = read_all<uint8_t>(dir + "/has1.bin");

        snake_hip::ORBVocabulary vocabulary(a);
        snake_hip::KeyframeDatabase db(vocabulary, 16, 512);
        std::vector<snake_hip::BowVector> bv(3);
        std::vector<snake_hip::FeatureVector> fv(3);
        for (int i = 0; i < 3; ++i)
        {
            vocabulary.transform(desc[(size_t)i], bv[(size_t)i], fv[(size_t)i], 4);
            std::vector<int32_t> words;
            std::vector<double> values;
            snake_hip::ORBVocabulary::flatten(bv[(size_t)i], words, values);
            const auto b = snake_hip::MappingORBMatcher::BowFeatureVector::from(fv[(size_t)i]);
            const std::string k = std::to_string(i);
            write_all(dir + "/out_words" + k + ".bin", words);
            write_all(dir + "/out_values" + k + ".bin", values);
            write_all(dir + "/out_nodes" + k + ".bin", b.node_id);
            write_all(dir + "/out_ns" + k + ".bin", b.node_start);
            write_all(dir + "/out_ft" + k + ".bin", b.features);
            db.Add(10 + i, bv[(size_t)i]);
        }
        write_all(dir + "/out_score.bin", std::vector<double>{vocabulary.score(bv[0], bv[1])});
        const auto loop  = db.DetectLoopCandidates(bv[0], {10}, 0.01f, 5);
        const auto reloc = db.DetectRelocalizationCandidates(bv[0], 0.5f, 5);
        db.Remove(11);
        const auto after = db.DetectRelocalizationCandidates(bv[0], 0.0f, 5);
        for (const auto& e : after)
            if (e.first == 11) throw std::runtime_error("bow_driver: a removed keyframe is still a candidate");
        write_all(dir + "/out_loop.bin", flat(loop));
        write_all(dir + "/out_reloc.bin", flat(reloc));
        snake_hip::LoopORBmatcher matcher;
        std::vector<int32_t> m12;
        const int n = matcher.MatchBoW(desc[0], has0, fv[0], desc[1], has1, fv[1], m12, 50, 0.75f);
        write_all(dir + "/out_m12.bin", m12);
        write_all(dir + "/out_meta.bin", std::vector<int32_t>{vocabulary.size(), n, (int32_t)loop.size(), (int32_t)reloc.size()});
        return 0;
    }
    catch (const std::exception& e)
    {
        std::cerr << e.what() << "\n";
        return 1;
    }
}
