// CPU: snake_slam_amd/csrc/stage.hpp with plain g++ (tests/test_stage_cpu.py).
//   stage_driver <mask> <size> ...   mask: a character per part, '1' = the part has a source, '0' = its source is NULL
// Builds a Block of these parts, prints
//   offsets <offset of every part>
//   bytes <Block::bytes> end <Block::end()>
//   at <at<char>(base, part) - base of every part>
//   buffer <hex of bytes + 16 bytes prefilled with 0xCD after copy()>
// Byte j of part i's source is (7 * j + i) & 0x7F: never 0xCD.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "stage.hpp"

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string mask = argv[1];
    const int n            = argc - 2;
    if ((int)mask.size() != n) return 2;
    std::vector<std::vector<unsigned char>> src((size_t)n);
    snk::Block b;
    for (int i = 0; i < n; ++i)
    {
        const size_t size = (size_t)strtoull(argv[2 + i], nullptr, 10);
        src[(size_t)i].resize(size);
        for (size_t j = 0; j < size; ++j) src[(size_t)i][j] = (unsigned char)((7 * j + (size_t)i) & 0x7F);
        // an empty part with a source keeps a pointer that is not NULL: copy() must skip it by its size
        static const unsigned char nothing = 0;
        const void* p = mask[(size_t)i] == '1' ? (size ? src[(size_t)i].data() : &nothing) : nullptr;
        if (b.add(p, size) != i) return 3;
    }
    printf("offsets");
    for (const snk::Block::Part& p : b.parts) printf(" %zu", p.offset);
    printf("\nbytes %zu end %zu\nat", b.bytes, b.end());
    std::vector<char> buf(b.bytes + 16, (char)0xCD);
    for (int i = 0; i < n; ++i) printf(" %td", b.at<char>(buf.data(), i) - buf.data());
    b.copy(buf.data());
    printf("\nbuffer ");
    for (char c : buf) printf("%02x", (unsigned)(unsigned char)c);
    printf("\n");
    return 0;
}
