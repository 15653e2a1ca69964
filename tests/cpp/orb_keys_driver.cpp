// CPU build of orb_keys.hpp (tests/test_cpp_orb_keys.py): for every "W H" pair of the command line builds the subdivision-key tables
// as snk_orb_configure does, checks root << 32 | interleave(keyx[x], keyy[y]) against the loop form for EVERY (x, y), and prints the
// table-form keys of a seeded sample as "W H x y key" lines for the comparison with the oracle.  Exit status 1 on a mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orb_keys.hpp"

int main(int argc, char** argv)
{
    if (argc < 3 || (argc - 1) % 2 != 0)
    {
        std::fprintf(stderr, "usage: orb_keys_driver W H [W H ...]\n");
        return 2;
    }
    uint64_t rng = 0x9E3779B97F4A7C15ull;  // xorshift64*: the sample is the same on every run
    auto next = [&rng]() {
        rng ^= rng >> 12;
        rng ^= rng << 25;
        rng ^= rng >> 27;
        return (uint32_t)((rng * 0x2545F4914F6CDD1Dull) >> 33);
    };
    long long bad = 0;
    for (int a = 1; a + 1 < argc; a += 2)
    {
        const int W = std::atoi(argv[a]), H = std::atoi(argv[a + 1]);
        if (W < 1 || H < 1 || W > 65535 || H > 65535)
        {
            std::fprintf(stderr, "orb_keys_driver: size %d x %d out of range\n", W, H);
            return 2;
        }
        const int nroots = snk::orb_key_nroots(W, H);
        std::vector<uint32_t> keyx((size_t)W), keyy((size_t)H);
        for (int x = 0; x < W; ++x) keyx[(size_t)x] = snk::orb_keyx_entry(x, W, H, nroots);
        for (int y = 0; y < H; ++y) keyy[(size_t)y] = snk::orb_keyy_entry(y, W, H);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
            {
                const uint64_t t = snk::orb_key_from_tables(keyx[(size_t)x], keyy[(size_t)y]);
                const uint64_t w = snk::orb_point_key(x, y, W, H, nroots);
                if (t != w && bad++ < 10)
                    std::fprintf(stderr, "orb_keys_driver: %d x %d, (%d, %d): tables %llx, loop %llx\n", W, H, x, y, (unsigned long long)t,
                                 (unsigned long long)w);
            }
        const int samples = (long long)W * H < 64 ? W * H : 64;
        for (int s = 0; s < samples; ++s)
        {
            // small levels: every point; the others: corners first, then random points
            int x, y;
            if ((long long)W * H < 64) x = s % W, y = s / W;
            else if (s < 4) x = (s & 1) ? W - 1 : 0, y = (s & 2) ? H - 1 : 0;
            else x = (int)(next() % (uint32_t)W), y = (int)(next() % (uint32_t)H);
            std::printf("%d %d %d %d %llu\n", W, H, x, y,
                        (unsigned long long)snk::orb_key_from_tables(keyx[(size_t)x], keyy[(size_t)y]));
        }
    }
    if (bad) std::fprintf(stderr, "orb_keys_driver: %lld mismatches\n", bad);
    return bad ? 1 : 0;
}
