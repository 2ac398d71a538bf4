// convolve_core.h -- what the sub-pel prediction kernels share (inter_pred_kernel.hip, mask_kernel.hip, obmc_kernel.hip): the six interpolation
// filter tables, the clamp / position rule of one reference, the clamped sample fetch, the staging of a tile's source window in LDS, and the
// compound (CONV_BUF_TYPE) and single-reference forms of the per-reference quad computation.  The tables and the rule exist once.
//
// Reference functions restated (Source/Lib):
//   compute_subpel_params (unscaled branch), clamp_mv_to_umv_border_sb, clamp_mv        Codec/enc_inter_prediction.c:3200-3211,30-50, Codec/inter_prediction.h:90-93
//   av1_get_convolve_filter_params, av1_get_interp_filter_params_with_block_size        Codec/inter_prediction.h:137-153
//   sub_pel_filters_8 / _4 / _8sharp / _8smooth / _4smooth, bilinear_filters             Codec/inter_prediction.c:223-254,1065-1129
//   svt_av1_jnt_convolve_{2d_copy,x,y,2d}_c, svt_av1_highbd_jnt_convolve_*_c             Codec/inter_prediction.c:494-668,852-1035
//   svt_av1_convolve_{2d_copy,x,y,2d}_sr_c, svt_av1_highbd_convolve_*_sr_c               Codec/inter_prediction.c:311-418,670-777
// Every InterpFilterParams has taps = 8 (the 4-tap tables are 8 wide with zero ends), so fo_horiz = fo_vert = 3 throughout.
#ifndef SVT_HIP_CONVOLVE_CORE_H
#define SVT_HIP_CONVOLVE_CORE_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/svt_hip_pred.h"
#include "wave_ops.h"

namespace {

constexpr int kWinU16 = 640; // (tile rows + 7) x (tile width + 8): 23 x 24 = 552, 39 x 16 = 624
constexpr int kMidU16 = 368; // (tile rows + 7) x tile width: 23 x 16 = 368, 39 x 8 = 312

// [0] sub_pel_filters_8, [1] sub_pel_filters_8smooth, [2] sub_pel_filters_8sharp, [3] bilinear_filters (InterpFilter's order), then the
// tables of a dimension <= 4: [4] sub_pel_filters_4, [5] sub_pel_filters_4smooth
__constant__ int16_t c_interp[6][16][8] = {
    {{0, 0, 0, 128, 0, 0, 0, 0}, {0, 2, -6, 126, 8, -2, 0, 0}, {0, 2, -10, 122, 18, -4, 0, 0}, {0, 2, -12, 116, 28, -8, 2, 0},
     {0, 2, -14, 110, 38, -10, 2, 0}, {0, 2, -14, 102, 48, -12, 2, 0}, {0, 2, -16, 94, 58, -12, 2, 0}, {0, 2, -14, 84, 66, -12, 2, 0},
     {0, 2, -14, 76, 76, -14, 2, 0}, {0, 2, -12, 66, 84, -14, 2, 0}, {0, 2, -12, 58, 94, -16, 2, 0}, {0, 2, -12, 48, 102, -14, 2, 0},
     {0, 2, -10, 38, 110, -14, 2, 0}, {0, 2, -8, 28, 116, -12, 2, 0}, {0, 0, -4, 18, 122, -10, 2, 0}, {0, 0, -2, 8, 126, -6, 2, 0}},
    {{0, 0, 0, 128, 0, 0, 0, 0}, {0, 2, 28, 62, 34, 2, 0, 0}, {0, 0, 26, 62, 36, 4, 0, 0}, {0, 0, 22, 62, 40, 4, 0, 0},
     {0, 0, 20, 60, 42, 6, 0, 0}, {0, 0, 18, 58, 44, 8, 0, 0}, {0, 0, 16, 56, 46, 10, 0, 0}, {0, -2, 16, 54, 48, 12, 0, 0},
     {0, -2, 14, 52, 52, 14, -2, 0}, {0, 0, 12, 48, 54, 16, -2, 0}, {0, 0, 10, 46, 56, 16, 0, 0}, {0, 0, 8, 44, 58, 18, 0, 0},
     {0, 0, 6, 42, 60, 20, 0, 0}, {0, 0, 4, 40, 62, 22, 0, 0}, {0, 0, 4, 36, 62, 26, 0, 0}, {0, 0, 2, 34, 62, 28, 2, 0}},
    {{0, 0, 0, 128, 0, 0, 0, 0}, {-2, 2, -6, 126, 8, -2, 2, 0}, {-2, 6, -12, 124, 16, -6, 4, -2}, {-2, 8, -18, 120, 26, -10, 6, -2},
     {-4, 10, -22, 116, 38, -14, 6, -2}, {-4, 10, -22, 108, 48, -18, 8, -2}, {-4, 10, -24, 100, 60, -20, 8, -2}, {-4, 10, -24, 90, 70, -22, 10, -2},
     {-4, 12, -24, 80, 80, -24, 12, -4}, {-2, 10, -22, 70, 90, -24, 10, -4}, {-2, 8, -20, 60, 100, -24, 10, -4}, {-2, 8, -18, 48, 108, -22, 10, -4},
     {-2, 6, -14, 38, 116, -22, 10, -4}, {-2, 6, -10, 26, 120, -18, 8, -2}, {-2, 4, -6, 16, 124, -12, 6, -2}, {0, 2, -2, 8, 126, -6, 2, -2}},
    {{0, 0, 0, 128, 0, 0, 0, 0}, {0, 0, 0, 120, 8, 0, 0, 0}, {0, 0, 0, 112, 16, 0, 0, 0}, {0, 0, 0, 104, 24, 0, 0, 0},
     {0, 0, 0, 96, 32, 0, 0, 0}, {0, 0, 0, 88, 40, 0, 0, 0}, {0, 0, 0, 80, 48, 0, 0, 0}, {0, 0, 0, 72, 56, 0, 0, 0},
     {0, 0, 0, 64, 64, 0, 0, 0}, {0, 0, 0, 56, 72, 0, 0, 0}, {0, 0, 0, 48, 80, 0, 0, 0}, {0, 0, 0, 40, 88, 0, 0, 0},
     {0, 0, 0, 32, 96, 0, 0, 0}, {0, 0, 0, 24, 104, 0, 0, 0}, {0, 0, 0, 16, 112, 0, 0, 0}, {0, 0, 0, 8, 120, 0, 0, 0}},
    {{0, 0, 0, 128, 0, 0, 0, 0}, {0, 0, -4, 126, 8, -2, 0, 0}, {0, 0, -8, 122, 18, -4, 0, 0}, {0, 0, -10, 116, 28, -6, 0, 0},
     {0, 0, -12, 110, 38, -8, 0, 0}, {0, 0, -12, 102, 48, -10, 0, 0}, {0, 0, -14, 94, 58, -10, 0, 0}, {0, 0, -12, 84, 66, -10, 0, 0},
     {0, 0, -12, 76, 76, -12, 0, 0}, {0, 0, -10, 66, 84, -12, 0, 0}, {0, 0, -10, 58, 94, -14, 0, 0}, {0, 0, -10, 48, 102, -12, 0, 0},
     {0, 0, -8, 38, 110, -12, 0, 0}, {0, 0, -6, 28, 116, -10, 0, 0}, {0, 0, -4, 18, 122, -8, 0, 0}, {0, 0, -2, 8, 126, -4, 0, 0}},
    {{0, 0, 0, 128, 0, 0, 0, 0}, {0, 0, 30, 62, 34, 2, 0, 0}, {0, 0, 26, 62, 36, 4, 0, 0}, {0, 0, 22, 62, 40, 4, 0, 0},
     {0, 0, 20, 60, 42, 6, 0, 0}, {0, 0, 18, 58, 44, 8, 0, 0}, {0, 0, 16, 56, 46, 10, 0, 0}, {0, 0, 14, 54, 48, 12, 0, 0},
     {0, 0, 12, 52, 52, 12, 0, 0}, {0, 0, 12, 48, 54, 14, 0, 0}, {0, 0, 10, 46, 56, 16, 0, 0}, {0, 0, 8, 44, 58, 18, 0, 0},
     {0, 0, 6, 42, 60, 20, 0, 0}, {0, 0, 4, 40, 62, 22, 0, 0}, {0, 0, 4, 36, 62, 26, 0, 0}, {0, 0, 2, 34, 62, 30, 0, 0}}};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); } // clamp(), Codec/definitions.h
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// av1_get_interp_filter_params_with_block_size: the table of a filter type on a dimension
__device__ __forceinline__ int filter_table(int filter, int dim) {
    if (dim <= 4 && (filter == 2 || filter == 0)) return 4;
    if (dim <= 4 && filter == 1) return 5;
    return filter;
}

__device__ __forceinline__ bool is_block_size(int w, int h) {
    const bool pw = w >= 4 && w <= 128 && (w & (w - 1)) == 0, ph = h >= 4 && h <= 128 && (h & (h - 1)) == 0;
    if (!pw || !ph) return false;
    const int big = w > h ? w : h, small = w > h ? h : w;
    return big == small || big == 2 * small || (big == 4 * small && big <= 64);
}

// what one reference of a job needs, all of it wave-uniform
struct RefView {
    const void *plane;
    int stride, org_x, org_y, max_x, max_y;
    int pos_x, pos_y; // of the block's first sample in the picture, after the clamp
    int sx, sy;       // subpel phases
};

// compute_subpel_params, unscaled branch: the clamp, the position and the phases of one reference (Desc: anything with ss_x / ss_y)
template <typename Desc> __device__ __forceinline__ RefView ref_view(const Desc &d, const SvtHipInterPredJob &j, const SvtHipInterPredRef r, int mvr, int mvc) {
    const int w = j.width, h = j.height, shx = 1 - d.ss_x, shy = 1 - d.ss_y;
    int row = (int16_t)(mvr * (1 << shy)), col = (int16_t)(mvc * (1 << shx)); // the (int16_t) cast of clamp_mv_to_umv_border_sb
    const int spel_left = (4 + w) << 4, spel_right = spel_left - 16, spel_top = (4 + h) << 4, spel_bottom = spel_top - 16;
    const int min_col = (int)((uint32_t)j.mb_to_left_edge << shx) - spel_left, max_col = (int)((uint32_t)j.mb_to_right_edge << shx) + spel_right;
    const int min_row = (int)((uint32_t)j.mb_to_top_edge << shy) - spel_top, max_row = (int)((uint32_t)j.mb_to_bottom_edge << shy) + spel_bottom;
    col = (int16_t)clampi(col, min_col, max_col);
    row = (int16_t)clampi(row, min_row, max_row);
    RefView v;
    v.plane = r.plane; v.stride = (int)r.stride; v.org_x = r.org_x; v.org_y = r.org_y;
    v.max_x = (int)r.width - 1; v.max_y = (int)r.height - 1;
    v.pos_x = j.org_x + (col >> 4); v.pos_y = j.org_y + (row >> 4);
    v.sx = col & 15; v.sy = row & 15;
    return v;
}

template <typename Px> __device__ __forceinline__ int sample(const RefView &r, int x, int y) {
    const int cx = clampi(x + r.org_x, 0, r.max_x), cy = clampi(y + r.org_y, 0, r.max_y);
    return ((const Px *)r.plane)[(size_t)cy * (size_t)r.stride + (size_t)cx];
}

// rows x cols samples from picture position (x0, y0) into win (row pitch ws)
template <typename Px> __device__ __forceinline__ void stage(uint16_t *win, const RefView &r, int x0, int y0, int cols, int rows, int ws, int lane) {
    const uint32_t magic = (65536u + (uint32_t)cols - 1) / (uint32_t)cols; // i / cols for i < 1024, cols <= 23: exact
    const int n = rows * cols;
    for (int i = lane; i < n; i += 64) {
        const int y = (int)(((uint32_t)i * magic) >> 16), x = i - y * cols;
        win[y * ws + x] = (uint16_t)sample<Px>(r, x0 + x, y0 + y);
    }
}

__device__ __forceinline__ void load4u(const uint16_t *p, int *v) { // 8-byte aligned
    const uint2 t = *(const uint2 *)p;
    v[0] = (int)(t.x & 0xFFFFu); v[1] = (int)(t.x >> 16); v[2] = (int)(t.y & 0xFFFFu); v[3] = (int)(t.y >> 16);
}
__device__ __forceinline__ void load4s(const int16_t *p, int *v) {
    const uint2 t = *(const uint2 *)p;
    v[0] = (int)(int16_t)(t.x & 0xFFFFu); v[1] = (int)t.x >> 16; v[2] = (int)(int16_t)(t.y & 0xFFFFu); v[3] = (int)t.y >> 16;
}

// The tile walk both kernels use: tiles of up to 64 quads (four horizontally adjacent samples), 4 x h, 8 x min(h, 32) or 16 x 16, one quad
// per lane.  All of it is wave-uniform but qx / qy / active.
struct TileWalk {
    int  TW, TH, qpr, qsh; // tile width and rows, quads per row and its log2
    int  qx, qy;           // the lane's quad in the tile
    bool active;
};
__device__ __forceinline__ TileWalk tile_walk(int w, int h, int lane) {
    TileWalk t;
    t.TW = w < 16 ? w : 16; t.qpr = t.TW >> 2; t.qsh = t.qpr == 1 ? 0 : (t.qpr == 2 ? 1 : 2);
    t.TH = h < (256 / t.TW) ? h : (256 / t.TW);
    t.active = lane < t.qpr * t.TH;
    t.qy = lane >> t.qsh; t.qx = (lane & (t.qpr - 1)) << 2;
    return t;
}

// tile_walk for strips that are no block sizes (obmc_kernel.hip), with a guard: at most 32 rows to a tile, which keeps every tile's window and
// intermediate inside the LDS slices whatever the strip -- the bound lives here, beside the slices' sizes.  With the 14 luma sizes the OBMC
// batches accept no 4-wide strip is higher than 32 rows (8x32 luma left, 16x64 chroma left), so the cap does not fire today
constexpr int kFitRows = 32;
static_assert((kFitRows + 7) * (4 + 8) <= kWinU16 && (kFitRows + 7) * (8 + 8) <= kWinU16 && (16 + 7) * (16 + 8) <= kWinU16, "a tile's window fits its LDS slice");
static_assert((kFitRows + 7) * 8 <= kMidU16 && (16 + 7) * 16 <= kMidU16, "a tile's intermediate fits its LDS slice");
__device__ __forceinline__ TileWalk tile_walk_fit(int w, int h, int lane) {
    TileWalk t = tile_walk(w, h, lane);
    if (t.TH > kFitRows) { t.TH = kFitRows; t.active = lane < t.qpr * kFitRows; } // only a 4-wide tile is higher: qpr = 1
    return t;
}

// One reference of a compound on one tile: the lane's quad of CONV_BUF_TYPE values, as svt_av1_jnt_convolve_{2d_copy,x,y,2d}_c and the
// highbd forms store them with do_average = 0 (round_0 = 3, round_1 = 7): res[i] in 0..65535.  (bx, by): the tile's first sample in the
// picture; win / mid: the wave's LDS slices (kWinU16 / kMidU16).  Inactive lanes take part in the staging and get res = 0.
template <bool HBD> __device__ __forceinline__ void compound_quad(const RefView &r, int tabx, int taby, const TileWalk &t, int bx, int by, uint16_t *win,
                                                                  int16_t *mid, int lane, int *res) {
    using Px = typename std::conditional<HBD, uint16_t, uint8_t>::type;
    constexpr int bd = HBD ? 10 : 8;
    constexpr int ro = (1 << (bd + 4)) + (1 << (bd + 3)); // round_offset: offset_bits = bd + 11, round_1 = 7
    const int  TW = t.TW, TH = t.TH, qx = t.qx, qy = t.qy;
    const bool fx = r.sx != 0, fy = r.sy != 0;
#pragma unroll
    for (int i = 0; i < 4; i++) res[i] = 0;
    if (!fx && !fy) { // svt_av1_jnt_convolve_2d_copy_c
        if (t.active)
#pragma unroll
            for (int i = 0; i < 4; i++) res[i] = (int)(uint16_t)((uint16_t)(sample<Px>(r, bx + qx + i, by + qy) << 4) + (uint16_t)ro);
        return;
    }
    const int ws = TW + 8, mx = fx ? 3 : 0, my = fy ? 3 : 0;
    wave_sync(); // the previous reads of win are done
    stage<Px>(win, r, bx - mx, by - my, TW + (fx ? 7 : 0), TH + (fy ? 7 : 0), ws, lane);
    wave_sync();
    int tx8[8], ty8[8];
#pragma unroll
    for (int k = 0; k < 8; k++) { tx8[k] = c_interp[tabx][r.sx][k]; ty8[k] = c_interp[taby][r.sy][k]; }
    if (fx && fy) { // the horizontal pass of *_2d_*: im_block, (TH + 7) rows
        const int units = (TH + 7) << t.qsh;
        for (int u = lane; u < units; u += 64) {
            const int rr = u >> t.qsh, cc = (u & (t.qpr - 1)) << 2;
            int in[12];
            load4u(win + rr * ws + cc, in); load4u(win + rr * ws + cc + 4, in + 4); load4u(win + rr * ws + cc + 8, in + 8);
            uint32_t o[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                int sum = 1 << (bd + 6);
#pragma unroll
                for (int k = 0; k < 8; k++) sum += tx8[k] * in[i + k];
                o[i] = (uint32_t)(uint16_t)(int16_t)((sum + 4) >> 3);
            }
            *(uint2 *)(mid + rr * TW + cc) = make_uint2(o[0] | (o[1] << 16), o[2] | (o[3] << 16));
        }
        wave_sync();
        if (t.active) {
            int sum[4];
#pragma unroll
            for (int i = 0; i < 4; i++) sum[i] = 1 << (bd + 11);
#pragma unroll
            for (int k = 0; k < 8; k++) {
                int v[4];
                load4s(mid + (qy + k) * TW + qx, v);
#pragma unroll
                for (int i = 0; i < 4; i++) sum[i] += ty8[k] * v[i];
            }
#pragma unroll
            for (int i = 0; i < 4; i++) res[i] = (int)(uint16_t)((sum[i] + 64) >> 7);
        }
    } else if (fx) { // *_x_*
        if (t.active) {
            int in[12];
            load4u(win + qy * ws + qx, in); load4u(win + qy * ws + qx + 4, in + 4); load4u(win + qy * ws + qx + 8, in + 8);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                int sum = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) sum += tx8[k] * in[i + k];
                res[i] = (int)(uint16_t)(((sum + 4) >> 3) + ro);
            }
        }
    } else { // *_y_*
        if (t.active) {
            int sum[4] = {0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < 8; k++) {
                int v[4];
                load4u(win + (qy + k) * ws + qx, v);
#pragma unroll
                for (int i = 0; i < 4; i++) sum[i] += ty8[k] * v[i];
            }
#pragma unroll
            for (int i = 0; i < 4; i++) res[i] = (int)(uint16_t)(((sum[i] * 16 + 64) >> 7) + ro);
        }
    }
}

// A single reference on one tile: the lane's quad of samples, as svt_av1_convolve_{2d_copy,x,y,2d}_sr_c and the highbd forms store them
// (round_0 = 3, round_1 = 11, each variant with its own rounding), clipped to the depth.  Arguments as compound_quad's; the window may be any
// tile with (TH + 7) * (TW + 8) <= kWinU16 and (TH + 7) * TW <= kMidU16.  Inactive lanes take part in the staging and get res = 0.
template <bool HBD> __device__ __forceinline__ void single_quad(const RefView &r, int tabx, int taby, const TileWalk &t, int bx, int by, uint16_t *win,
                                                                int16_t *mid, int lane, int *res) {
    using Px = typename std::conditional<HBD, uint16_t, uint8_t>::type;
    constexpr int bd = HBD ? 10 : 8, px_max = (1 << bd) - 1;
    const int  TW = t.TW, TH = t.TH, qx = t.qx, qy = t.qy;
    const bool fx = r.sx != 0, fy = r.sy != 0;
#pragma unroll
    for (int i = 0; i < 4; i++) res[i] = 0;
    if (!fx && !fy) { // svt_av1_convolve_2d_copy_sr_c
        if (t.active)
#pragma unroll
            for (int i = 0; i < 4; i++) res[i] = sample<Px>(r, bx + qx + i, by + qy);
        return;
    }
    const int ws = TW + 8, mx = fx ? 3 : 0, my = fy ? 3 : 0;
    wave_sync(); // the previous reads of win are done
    stage<Px>(win, r, bx - mx, by - my, TW + (fx ? 7 : 0), TH + (fy ? 7 : 0), ws, lane);
    wave_sync();
    int tx8[8], ty8[8];
#pragma unroll
    for (int k = 0; k < 8; k++) { tx8[k] = c_interp[tabx][r.sx][k]; ty8[k] = c_interp[taby][r.sy][k]; }
    if (fx && fy) { // the horizontal pass of *_2d_sr: im_block, (TH + 7) rows
        const int units = (TH + 7) << t.qsh;
        for (int u = lane; u < units; u += 64) {
            const int rr = u >> t.qsh, cc = (u & (t.qpr - 1)) << 2;
            int in[12];
            load4u(win + rr * ws + cc, in); load4u(win + rr * ws + cc + 4, in + 4); load4u(win + rr * ws + cc + 8, in + 8);
            uint32_t o[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                int sum = 1 << (bd + 6);
#pragma unroll
                for (int k = 0; k < 8; k++) sum += tx8[k] * in[i + k];
                o[i] = (uint32_t)(uint16_t)(int16_t)((sum + 4) >> 3);
            }
            *(uint2 *)(mid + rr * TW + cc) = make_uint2(o[0] | (o[1] << 16), o[2] | (o[3] << 16));
        }
        wave_sync();
        if (t.active) {
            int sum[4];
#pragma unroll
            for (int i = 0; i < 4; i++) sum[i] = 1 << (bd + 11);
#pragma unroll
            for (int k = 0; k < 8; k++) {
                int v[4];
                load4s(mid + (qy + k) * TW + qx, v);
#pragma unroll
                for (int i = 0; i < 4; i++) sum[i] += ty8[k] * v[i];
            }
#pragma unroll
            for (int i = 0; i < 4; i++) { // round_1 = 11, bits = 0; the 8-bit function holds res in an int16_t
                const int v = ((sum[i] + 1024) >> 11) - ((1 << bd) + (1 << (bd - 1)));
                res[i] = clampi(HBD ? v : (int)(int16_t)(uint16_t)v, 0, px_max);
            }
        }
    } else if (fx) { // *_x_sr
        if (t.active) {
            int in[12];
            load4u(win + qy * ws + qx, in); load4u(win + qy * ws + qx + 4, in + 4); load4u(win + qy * ws + qx + 8, in + 8);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                int sum = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) sum += tx8[k] * in[i + k];
                res[i] = clampi((((sum + 4) >> 3) + 8) >> 4, 0, px_max);
            }
        }
    } else { // *_y_sr
        if (t.active) {
            int sum[4] = {0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < 8; k++) {
                int v[4];
                load4u(win + (qy + k) * ws + qx, v);
#pragma unroll
                for (int i = 0; i < 4; i++) sum[i] += ty8[k] * v[i];
            }
#pragma unroll
            for (int i = 0; i < 4; i++) res[i] = clampi((sum[i] + 64) >> 7, 0, px_max);
        }
    }
}

} // namespace
#endif
