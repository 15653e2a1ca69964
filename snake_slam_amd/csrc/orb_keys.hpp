// Subdivision keys of the quadtree distribution (orb.hip, distribute_body): one definition of the split rule, compiled for the host
// (the per-level tables snk_orb_configure uploads, tests/cpp/orb_keys_driver.cpp) and for the device (the loop form, kept as the
// fallback of the table form).
//
// A point's key is its root (the image is cut into nroots columns) followed by KEY_DIGITS quadtree digits, digit = cx + 2 * cy,
// where cx / cy say on which side of the node's midpoint x0 + (x1 - x0 + 1) / 2 the point lies.  The x interval of a node depends
// on x alone and the y interval on y alone, so the 32 digit bits are the bit-interleave of a 16-bit x word and a 16-bit y word:
//   keyx[x] = root << 16 | x word        x in [0, W)
//   keyy[y] = y word                     y in [0, H)
//   key     = root << 32 | interleave(x word, y word)
// A node's extent at least halves (rounded up) per digit, so after nd = bits(max(W, H) - 1) digits it is one pixel in both axes and
// every further digit is 0 (the midpoint of [x, x + 1) is x + 1): both forms stop there, the words are left-aligned.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SNK_KEYS_HD __host__ __device__ inline
#else
#define SNK_KEYS_HD inline
#endif

namespace snk
{
constexpr int ORB_KEY_DIGITS = 16;

// digits after which every node is a single pixel
SNK_KEYS_HD int orb_key_ndigits(int W, int H)
{
    int ext = W > H ? W : H;
    if (ext < 2) ext = 2;
    const int nd = 32 - __builtin_clz((unsigned)(ext - 1));
    return nd < ORB_KEY_DIGITS ? nd : ORB_KEY_DIGITS;
}

// x, W < 2^16 and nroots <= 255: every product stays under 2^24
SNK_KEYS_HD int orb_key_root(int x, int W, int nroots) { return (int)(((uint32_t)x * (uint32_t)nroots) / (uint32_t)W); }
SNK_KEYS_HD int orb_key_root_begin(int root, int W, int nroots)
{
    return (int)(((uint32_t)root * (uint32_t)W + (uint32_t)nroots - 1u) / (uint32_t)nroots);
}

// the split rule along one axis: nd binary digits of v in [lo, hi), first digit in the highest of the nd bits
SNK_KEYS_HD uint32_t orb_key_axis_digits(int v, int lo, int hi, int nd)
{
    uint32_t bits = 0;
    for (int d = 0; d < nd; ++d)
    {
        const int m = lo + (hi - lo + 1) / 2;
        const int c = v >= m;
        lo          = c ? m : lo;
        hi          = c ? hi : m;
        bits        = (bits << 1) | (uint32_t)c;
    }
    return bits;
}

// table entries (W, H: the level's extent without its border; both tables need both, nd depends on the larger)
SNK_KEYS_HD uint32_t orb_keyx_entry(int x, int W, int H, int nroots)
{
    const int nd = orb_key_ndigits(W, H), root = orb_key_root(x, W, nroots);
    const uint32_t bits = orb_key_axis_digits(x, orb_key_root_begin(root, W, nroots), orb_key_root_begin(root + 1, W, nroots), nd);
    return ((uint32_t)root << 16) | (bits << (ORB_KEY_DIGITS - nd));
}
SNK_KEYS_HD uint32_t orb_keyy_entry(int y, int W, int H)
{
    const int nd = orb_key_ndigits(W, H);
    return orb_key_axis_digits(y, 0, H, nd) << (ORB_KEY_DIGITS - nd);
}

// bit i of a 16-bit word to bit 2 i
SNK_KEYS_HD uint32_t orb_key_spread16(uint32_t v)
{
    v &= 0xFFFFu;
    v = (v | (v << 8)) & 0x00FF00FFu;
    v = (v | (v << 4)) & 0x0F0F0F0Fu;
    v = (v | (v << 2)) & 0x33333333u;
    v = (v | (v << 1)) & 0x55555555u;
    return v;
}

// table form: 8 + 32 bits
SNK_KEYS_HD uint64_t orb_key_from_tables(uint32_t kx, uint32_t ky)
{
    return ((uint64_t)(kx >> 16) << 32) | (uint64_t)(orb_key_spread16(kx) | (orb_key_spread16(ky) << 1));
}

// loop form: 8 + 32 bits
SNK_KEYS_HD uint64_t orb_point_key(int x, int y, int W, int H, int nroots)
{
    const int root = orb_key_root(x, W, nroots);
    int x0 = orb_key_root_begin(root, W, nroots), x1 = orb_key_root_begin(root + 1, W, nroots);
    int y0 = 0, y1 = H;
    uint64_t key = (uint64_t)root;
    const int nd = orb_key_ndigits(W, H);
    for (int d = 0; d < nd; ++d)
    {
        const int mx = x0 + (x1 - x0 + 1) / 2, my = y0 + (y1 - y0 + 1) / 2;
        const int cx = x >= mx, cy = y >= my;
        x0  = cx ? mx : x0;
        x1  = cx ? x1 : mx;
        y0  = cy ? my : y0;
        y1  = cy ? y1 : my;
        key = (key << 2) | (uint64_t)(cx + 2 * cy);
    }
    return key << (2 * (ORB_KEY_DIGITS - nd));
}

// number of roots of a W x H level (ORB-SLAM2: round(W / H), at least 1; 8 key bits)
SNK_KEYS_HD int orb_key_nroots(int W, int H)
{
    int n = H > 0 ? (2 * W + H) / (2 * H) : 1;
    return n < 1 ? 1 : (n > 255 ? 255 : n);
}
}  // namespace snk
