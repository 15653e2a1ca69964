// Geometry of the ORB extractor (orb.hip): the kernel argument `Layout` and the arithmetic that fills it from an image size and the
// extractor's parameters -- level sizes and scales, feature quotas, the FAST cell grid, slots, pitches, the strips and bands of the
// streaming pass, the per-wavefront LDS slice of fast_kernel -- and the LDS carves of the distribution.  Host-only arithmetic and free
// of HIP includes, split like orb_keys.hpp: orb.hip compiles it for the kernels' argument, tests/cpp/dispatch_driver.cpp with plain g++.
// What needs the device stays in orb.hip: the buffers, the resize / cell / key tables and the pointers of the struct.
#pragma once
#include <cmath>
#include <cstddef>

#include "orb_keys.hpp"
#if defined(__HIPCC__)
#include <hip/hip_vector_types.h>  // int4: the pointee of Layout::cell_tab in the device compile
#endif

namespace snk
{
namespace orb
{
constexpr int MAX_LEVELS        = 16;
constexpr int EDGE_THRESHOLD    = 19;
constexpr int MIN_BORDER        = 16;
constexpr int CELL_W            = 30;
constexpr int CELL_SLOTS        = 64;  // strongest candidates kept per cell
constexpr int DEFAULT_LEVEL_CAP = 8192;
constexpr int SM_BH             = 64;  // output rows per band of the layout's unit count (level_kernel's band heights: dispatch.hpp, orb_band_rows)
constexpr int SM_LANES_OUT      = 61;  // strip <= 244 columns: 8 loaded columns remain to the right for the down-scale taps
constexpr int STRIP_STRIDE      = 192; // strips start on 64-byte boundaries of the row
constexpr int LDS_BYTES         = 160 * 1024;  // gfx950: LDS per workgroup (common.hpp: LDS_MAX_BYTES)

#if defined(__HIPCC__)
using Cell = int4;
#else
struct alignas(16) Cell
{
    int x, y, z, w;
};
#endif
}  // namespace orb

// The kernels' argument.  The three structs keep internal linkage, as they had inside orb.hip: the kernels' symbol names carry the
// namespace of their parameter types.
namespace
{
struct LevelInfo
{
    int w, h, pitch;
    long long img_stride;  // bytes between consecutive images of this level
    unsigned char* base;   // level buffer (levels >= 1); level 0 comes from the caller
    unsigned char* blur;   // blurred level (all levels), same pitch / stride as the level buffers
    int strip_stride, n_strips, n_bands, unit_off;  // streaming pass: column strips x row bands of this level
    int store_end;         // the last strip writes the blurred row up to this column (>= w: into the row padding, whole 64-byte sectors)
    const int* ymap;      // [h] destination row of level l+1 whose upper source row is this row, or -1
    const int* strip_dx;  // [n_strips + 1] first destination dword (4 px) of level l+1 owned by each strip
    int ncols, nrows, wcell, hcell;
    int cell_off;          // first cell of this level in the per-image cell arrays
    int nfeat;             // features wanted on this level
    int slot_off, slot_cap;  // per-image slots for the selected keypoints of this level
    int nroots;
    float scale;
    const int* xofs;  // resize tables (device): source column / weight per destination column
    const int* xw1;
    const int* yofs;
    const int* yw1;
    long long blur_stride;  // bytes between consecutive images of the BLURRED level: pitch x (h rounded up to 4) -- room for the tiled layout
};

// what fast_kernel reads of a level: the head of LevelInfo, taken with one 32-byte load
struct LevelHead
{
    int w, h, pitch, pad_;
    long long img_stride;
    unsigned char* base;
};
static_assert(sizeof(LevelHead) == 32 && offsetof(LevelInfo, w) == 0 && offsetof(LevelInfo, h) == 4 && offsetof(LevelInfo, pitch) == 8 &&
                  offsetof(LevelInfo, img_stride) == 16 && offsetof(LevelInfo, base) == 24,
              "LevelHead mirrors the first 32 bytes of LevelInfo");

struct Layout
{
    int n_levels;
    int total_cells;
    int total_slots;
    int total_units;
    int level_cap;
    // per-wavefront LDS slice of fast_kernel (bytes; sized from the largest cell of the layout)
    int f_tile_pitch_dw, f_s_pitch, f_off_s, f_off_surv, f_off_list, f_off_cnt, f_lds_wave, f_surv_cap;
    const orb::Cell* cell_tab;  // [total_cells] (x0, y0, cw | ch << 16, level) of every FAST cell: one scalar load instead of a level search and two integer divisions per cell
    LevelInfo lv[orb::MAX_LEVELS];
};
// the kernels were written against these offsets (scalar loads of the argument's fields): a member that moves changes every kernel
static_assert(sizeof(LevelInfo) == 160 && offsetof(LevelInfo, blur) == 32 && offsetof(LevelInfo, strip_stride) == 40 && offsetof(LevelInfo, store_end) == 56 &&
                  offsetof(LevelInfo, ymap) == 64 && offsetof(LevelInfo, strip_dx) == 72 && offsetof(LevelInfo, ncols) == 80 && offsetof(LevelInfo, cell_off) == 96 &&
                  offsetof(LevelInfo, nroots) == 112 && offsetof(LevelInfo, scale) == 116 && offsetof(LevelInfo, xofs) == 120 && offsetof(LevelInfo, blur_stride) == 152,
              "LevelInfo is a kernel argument");
static_assert(sizeof(orb::Cell) == 16 && sizeof(Layout) == 2624 && offsetof(Layout, level_cap) == 16 && offsetof(Layout, f_tile_pitch_dw) == 20 &&
                  offsetof(Layout, f_surv_cap) == 48 && offsetof(Layout, cell_tab) == 56 && offsetof(Layout, lv) == 64,
              "Layout is a kernel argument");
}  // namespace

namespace orb
{
constexpr int cdiv(int a, int b) { return (a + b - 1) / b; }
constexpr int up16(int v) { return (v + 15) & ~15; }

// The strips of a w-column level (w > 0).  Strips START on 64-byte boundaries of the row (stride 192 columns; the last strip takes what
// is left, up to the 244 columns a wavefront can produce): a wavefront's row store then never shares a 64-byte sector with its
// neighbour strip's.  Round 5, tools/probes/hbm_write_shapes.sh: rows written as 4 x 188-byte strips (the balanced layout of a 752-px
// level) reach 3.3 TB/s, as 4 x 192-byte strips 5.1 TB/s.  balanced (SNK_ORB_BALANCED_STRIPS=1): the round-1..4 layout (equal strips
// of a multiple of 4 columns).
// The last strip's blurred store runs on to the end of the row pitch when its 61 lanes reach it (EuRoC levels 0 and 2: 576 + 192 =
// 768, 384 + 192 = 576): whole 64-byte sectors instead of a ragged end; the padding columns hold reflected-border blur values
// nobody reads.  +0.4 % end to end; one more 192-column strip wherever the rest exceeds 192 columns instead: -1.5 %
// (profiles/r05/r05z_strip_store_end.json).
inline void level_strips(LevelInfo& lv, bool balanced)
{
    if (balanced || lv.w <= 4 * SM_LANES_OUT)
    {
        lv.n_strips     = cdiv(lv.w, 4 * SM_LANES_OUT);
        lv.strip_stride = ((cdiv(lv.w, lv.n_strips) + 3) / 4) * 4;
    }
    else
    {
        lv.strip_stride = STRIP_STRIDE;
        lv.n_strips     = 1 + cdiv(lv.w - 4 * SM_LANES_OUT, STRIP_STRIDE);
    }
    lv.store_end = lv.w;
    if (!balanced && lv.w > 4 * SM_LANES_OUT && lv.pitch - (lv.n_strips - 1) * lv.strip_stride <= 4 * SM_LANES_OUT) lv.store_end = lv.pitch;
}

// The per-wavefront LDS slice of fast_kernel for cells of at most mw x mh pixels: image tile | score map with zero ring | quick-test
// survivors | 3 counters; the list of non-maximum-suppression survivors is written after the last read of the image tile, into the same
// bytes.  surv_cap_env: SNK_ORB_FAST_SURV_CAP (0 = unset; the tests that force the spill path on ordinary images).
// False: the corner list is larger than the tile it aliases.
inline bool fast_slice(Layout& L, int mw, int mh, int surv_cap_env)
{
    L.f_tile_pitch_dw = (mw + 6 + 3 + 3) / 4;
    L.f_s_pitch       = (mw + 2 + 3) & ~3;
    // compile-time pitches (fast_kernel<3> / <4>) when the widest cell allows, see fast_quads()
    if (L.f_tile_pitch_dw <= 12 && L.f_s_pitch <= 40 && mh + 6 <= 128) { L.f_tile_pitch_dw = 12; L.f_s_pitch = 40; }
    else if (L.f_tile_pitch_dw <= 16 && L.f_s_pitch <= 64 && mh + 6 <= 128) { L.f_tile_pitch_dw = 16; L.f_s_pitch = 64; }
    const int tile_b = up16((mh + 6) * L.f_tile_pitch_dw * 4);
    const int s_b    = up16((mh + 2) * L.f_s_pitch) + 16;  // zero-filled in 16-byte stores
    // survivors of the quick test kept at a time (fast_kernel scores and restarts the list when a cell has more)
    L.f_surv_cap = (mw * mh / 2 + 63) & ~63;  // measured: 0.60 / 0.55 / 0.50 / 0.485 / 0.54 ms at 320 / 384 / 512 / 640 / all pixels
    if (L.f_surv_cap < 256) L.f_surv_cap = 256;
    if (surv_cap_env > 0) L.f_surv_cap = surv_cap_env;
    const int surv_b = up16(L.f_surv_cap * 2);
    const int list_b = up16(((mw + 1) / 2) * ((mh + 1) / 2) * 4);
    L.f_off_s    = tile_b;
    L.f_off_surv = L.f_off_s + s_b;
    L.f_off_list = 0;
    L.f_off_cnt  = L.f_off_surv + surv_b;
    L.f_lds_wave = L.f_off_cnt + 16;
    return list_b <= tile_b;
}
// the compile-time pitches of fast_kernel<NQ, .>: 3 / 4 sixteen-byte quads per tile row, 0 = pitches from the layout
inline int fast_quads(const Layout& L)
{
    return L.f_tile_pitch_dw == 12 && L.f_s_pitch == 40 ? 3 : (L.f_tile_pitch_dw == 16 && L.f_s_pitch == 64 ? 4 : 0);
}
// four wavefronts' slices in a workgroup's LDS
inline bool fast_fits(const Layout& L) { return 4 * L.f_lds_wave <= LDS_BYTES; }

// Everything of `L` but its pointers, for w x h images.  The float expressions are the ORB-SLAM2 constructor's, in its order.
// Returns nullptr, or what is wrong with the shape.
inline const char* layout(Layout& L, int w, int h, int nfeatures, float scale_factor, int n_levels, int level_cap, bool balanced_strips,
                          int surv_cap_env)
{
    L           = Layout{};
    L.n_levels  = n_levels;
    L.level_cap = level_cap > 0 ? level_cap : DEFAULT_LEVEL_CAP;
    float scale[MAX_LEVELS];
    scale[0] = 1.0f;
    for (int l = 1; l < n_levels; ++l) scale[l] = scale[l - 1] * scale_factor;
    const float factor = 1.0f / scale_factor;
    float n_desired    = (float)nfeatures * (1.0f - factor) / (1.0f - (float)std::pow((double)factor, (double)n_levels));
    int sum = 0, cell_off = 0, slot_off = 0, tile_off = 0;
    for (int l = 0; l < n_levels; ++l)
    {
        LevelInfo& lv   = L.lv[l];
        const float inv = 1.0f / scale[l];
        lv.w     = (int)std::lrintf((float)w * inv);
        lv.h     = (int)std::lrintf((float)h * inv);
        lv.scale = scale[l];
        if (l < n_levels - 1)
        {
            lv.nfeat = (int)std::lrintf(n_desired);
            sum += lv.nfeat;
            n_desired *= factor;
        }
        else
            lv.nfeat = nfeatures - sum > 0 ? nfeatures - sum : 0;
        const int width = lv.w - 2 * MIN_BORDER, height = lv.h - 2 * MIN_BORDER;
        lv.ncols = width > 0 ? width / CELL_W : 0;
        lv.nrows = height > 0 ? height / CELL_W : 0;
        if (lv.ncols < 1 || lv.nrows < 1 || lv.w < 2 * EDGE_THRESHOLD + 1 || lv.h < 2 * EDGE_THRESHOLD + 1)
        {
            lv.ncols = lv.nrows = 0;
            lv.wcell = lv.hcell = 1;
        }
        else
        {
            lv.wcell = (width + lv.ncols - 1) / lv.ncols;
            lv.hcell = (height + lv.nrows - 1) / lv.nrows;
        }
        lv.cell_off = cell_off;
        cell_off += lv.ncols * lv.nrows;
        lv.nroots   = orb_key_nroots(width, height);  // orb_keys.hpp: the root count the key tables are filled with
        lv.slot_off = slot_off;
        lv.slot_cap = lv.nfeat + 3 > 4 * lv.nroots ? lv.nfeat + 3 : 4 * lv.nroots;
        slot_off += lv.slot_cap;
        lv.pitch       = (lv.w + 63) & ~63;
        lv.img_stride  = (long long)lv.pitch * lv.h;
        lv.blur_stride = (long long)lv.pitch * ((lv.h + 3) & ~3);
        if (lv.w > 0 && lv.h > 0)
        {
            level_strips(lv, balanced_strips);
            lv.n_bands = cdiv(lv.h, SM_BH);
        }
        else  // a level scaled down to nothing (small image, many levels, large scale factor): no strips, no work
        {
            lv.w = lv.w > 0 ? lv.w : 0;
            lv.h = lv.h > 0 ? lv.h : 0;
            lv.n_strips = lv.n_bands = 0;
            lv.strip_stride = 4;
        }
        lv.unit_off = tile_off;
        tile_off += lv.n_strips * lv.n_bands;
    }
    L.total_cells = cell_off;
    L.total_slots = slot_off;
    L.total_units = tile_off;
    int mw = 1, mh = 1;  // the largest cell
    for (int l = 0; l < n_levels; ++l)
        if (L.lv[l].ncols > 0)
        {
            mw = L.lv[l].wcell > mw ? L.lv[l].wcell : mw;
            mh = L.lv[l].hcell > mh ? L.lv[l].hcell : mh;
        }
    if (!fast_slice(L, mw, mh, surv_cap_env)) return "FAST: corner list larger than the tile it aliases";
    return nullptr;
}

// ---- LDS carves of distribute_kernel / distribute_large_kernel ----
constexpr int DIST_SMALL_CAP = 2048;  // candidates of an (image, level) that distribute_kernel's own carve holds; a larger level is queued for the drain launch
constexpr int DIST_CAP_MAX   = 8192;  // the largest level_cap
// dynamic LDS of a workgroup that sorts and distributes up to `cap` candidates (distribute_body's carve)
constexpr size_t dist_lds_bytes(size_t cap) { return cap * 8 + cap / 2 * 8 + cap * 2 * 2 + cap + (cap + 16) + cap; }
// the Harris ranks beside the small carve ("orb.response" = 1)
constexpr size_t dist_harris_bytes(size_t cap) { return 4 * cap + 16; }
constexpr int dist_small_cap(int level_cap) { return level_cap < DIST_SMALL_CAP ? level_cap : DIST_SMALL_CAP; }
// what set_max_lds_once asks for, process-wide: the largest of the 2048-candidate carve + the Harris ranks and the full-budget carve
// (small launches take it directly); the drain launch's full-budget carve
constexpr size_t DIST_LDS_MAX = dist_lds_bytes(DIST_SMALL_CAP) + dist_harris_bytes(DIST_SMALL_CAP) > dist_lds_bytes(DIST_CAP_MAX)
                                    ? dist_lds_bytes(DIST_SMALL_CAP) + dist_harris_bytes(DIST_SMALL_CAP)
                                    : dist_lds_bytes(DIST_CAP_MAX);
constexpr size_t DIST_LARGE_LDS_MAX = dist_lds_bytes(DIST_CAP_MAX);
static_assert(DIST_LDS_MAX <= (size_t)LDS_BYTES, "the distribution's carve fits a workgroup's LDS");
}  // namespace orb
}  // namespace snk
