// mask_kernel.hip -- the masked predictions and their parameter searches on gfx950: svt_hip_masked_pred_batch (COMPOUND_WEDGE / COMPOUND_DIFFWTD),
// svt_hip_interintra_blend_batch (smooth and wedge inter-intra) and svt_hip_mask_search_batch (pick_interinter_wedge, pick_interinter_seg,
// inter_intra_search).  include/svt_hip_mask.h names the reference functions restated; all arithmetic is integer.
//
// The wedge masks.  The library holds what the reference's svt_av1_init_wedge_masks builds first: the twelve 64 x 64 primaries (two signs x six
// directions, 48 KB), generated at compile time from the AV1 specification's three 64-entry master rows, and the sign-flip table of the nine
// sizes by init_wedge_signs' rule.  A (size, index, sign) mask is a window of a primary -- direction, x_offset, y_offset from the codebook,
// sign XOR sign-flip -- and is read in place from global memory: there are no 9 x 32 contiguous copies.  The table is shared by every job of every
// batch and stays in the caches; a search job uses each byte of a window once (the other sign's mask is 64 - m, formed in registers), so a copy
// in LDS would cost the same global reads plus the LDS traffic.
//
// Prediction: inter_pred_kernel's lay-out (convolve_core.h): one wave per job, four jobs per workgroup, no workgroup barrier, tiles of up to 64
// quads, both references' CONV_BUF_TYPE quads in the lane's registers.  The lane fetches its four mask values (1, 2 or 4 bytes each with
// sub-sampling) -- wedge bytes from the primaries, DIFFWTD values from |a - b| (luma) or the mask buffer (chroma) -- blends, subtracts the round
// offset, rounds by 4 and clips.  Mask type, sub-sampling and depth are wave-uniform: the branches are per job.
//
// Searches: one wave per job.  Kinds 0 and 2 hold the block (at most 1024 samples, 16 per lane) in registers as packed int16 pairs, (r1, d) per
// sample and ds per two samples, for all 16 wedges; source and predictions are read once.  Kind 1 walks up to 16384 samples in strips of 64 quads
// and forms both masks' terms in the same pass.  Sum widths:
//   SAD              <= 16384 * 1023 < 2^24                                      32 bits
//   sum r^2          <= 1024 * 1023^2 < 2^30 (kinds 0 / 2: at most 1024 samples)  32 bits
//   sum ds * m       |.| <= 1024 * 32768 * 64 = 2^31: the minimum -2^31 and the maximum 1024 * 32767 * 64 both fit int32 (static_assert below);
//                    a lane's 16 terms reach 2^25; the wave's sum is taken modulo 2^32 and read as int32
//   sum t^2          t^2 <= 2^30: a lane's 16 (kinds 0 / 2) or 256 (kind 1) terms reach 2^34 / 2^38, held in 64 bits; the wave's sum in three pieces
//                    that cannot overflow (wave_sum64_dpp)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include "batch_host.h"
#include "../../include/svt_hip_mask.h"
#include "wave_ops.h"
#include "convolve_core.h"

namespace {

constexpr int kWaves = 4;

// ---- tables ------------------------------------------------------------------------------------------------------------------------------
// AV1 specification, Wedge_Master_Oblique_Odd / _Even / _Vertical
constexpr uint8_t kObliqueOdd[64]  = {0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  1,  2,  6,  18,
                                      37, 53, 60, 63, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64};
constexpr uint8_t kObliqueEven[64] = {0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  1,  4,  11, 27,
                                      46, 58, 62, 63, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64};
constexpr uint8_t kVertical[64]    = {0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  2,  7,  21,
                                      43, 57, 62, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64};
// WedgeDirectionType
enum { kHor = 0, kVer = 1, kO27 = 2, kO63 = 3, kO117 = 4, kO153 = 5 };
struct WedgeCode { uint8_t dir, x, y; };
// AV1 specification, Wedge_Codebook: [0] height > width, [1] height < width, [2] square
constexpr WedgeCode kCodebook[3][16] = {
    {{kO27, 4, 4}, {kO63, 4, 4}, {kO117, 4, 4}, {kO153, 4, 4}, {kHor, 4, 2}, {kHor, 4, 4}, {kHor, 4, 6}, {kVer, 4, 4},
     {kO27, 4, 2}, {kO27, 4, 6}, {kO153, 4, 2}, {kO153, 4, 6}, {kO63, 2, 4}, {kO63, 6, 4}, {kO117, 2, 4}, {kO117, 6, 4}},
    {{kO27, 4, 4}, {kO63, 4, 4}, {kO117, 4, 4}, {kO153, 4, 4}, {kVer, 2, 4}, {kVer, 4, 4}, {kVer, 6, 4}, {kHor, 4, 4},
     {kO27, 4, 2}, {kO27, 4, 6}, {kO153, 4, 2}, {kO153, 4, 6}, {kO63, 2, 4}, {kO63, 6, 4}, {kO117, 2, 4}, {kO117, 6, 4}},
    {{kO27, 4, 4}, {kO63, 4, 4}, {kO117, 4, 4}, {kO153, 4, 4}, {kHor, 4, 2}, {kHor, 4, 6}, {kVer, 2, 4}, {kVer, 6, 4},
     {kO27, 4, 2}, {kO27, 4, 6}, {kO153, 4, 2}, {kO153, 4, 6}, {kO63, 2, 4}, {kO63, 6, 4}, {kO117, 2, 4}, {kO117, 6, 4}}};
// the nine sizes with wedges, in BlockSize's order: 8x8, 8x16, 16x8, 16x16, 16x32, 32x16, 32x32, 8x32, 32x8
constexpr uint8_t kWedgeW[9] = {8, 8, 16, 16, 16, 32, 32, 8, 32}, kWedgeH[9] = {8, 16, 8, 16, 32, 16, 32, 32, 8};
// AV1 specification, Ii_Weights_1d (ii_weights1d); ii_size_scales[bsize] is 128 / max(width, height)
__constant__ uint8_t c_ii_weights[128] = {60, 58, 56, 54, 52, 50, 48, 47, 45, 44, 42, 41, 39, 38, 37, 35, 34, 33, 32, 31, 30, 29, 28, 27, 26, 25, 24, 23, 22, 22, 21, 20,
                                          19, 19, 18, 18, 17, 16, 16, 15, 15, 14, 14, 13, 13, 12, 12, 12, 11, 11, 10, 10, 10, 9,  9,  9,  8,  8,  8,  8,  7,  7,  7,  7,
                                          6,  6,  6,  6,  6,  5,  5,  5,  5,  5,  4,  4,  4,  4,  4,  4,  4,  4,  3,  3,  3,  3,  3,  3,  3,  3,  3,  2,  2,  2,  2,  2,
                                          2,  2,  2,  2,  2,  2,  2,  2,  2,  2,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1};

struct WedgeTables {
    uint8_t prim[2][6][64 * 64]; // wedge_mask_obl: [negative][direction]
    uint8_t flip[9][16];         // wedge_signflip_lookup of the nine sizes
    uint8_t dir[9][16];          // the codebook's direction of (size, index)
    uint16_t off[9][16];         // get_wedge_mask_inplace: the window's first byte in a primary
};

constexpr int codebook_of(int w, int h) { return h > w ? 0 : (h < w ? 1 : 2); }
// get_wedge_mask_inplace: the window's first byte in a primary
constexpr int window_offset(int size, int index) {
    const WedgeCode c = kCodebook[codebook_of(kWedgeW[size], kWedgeH[size])][index];
    return 64 * (32 - ((c.y * kWedgeH[size]) >> 3)) + 32 - ((c.x * kWedgeW[size]) >> 3);
}

constexpr WedgeTables make_wedge_tables() {
    WedgeTables t = {};
    // init_wedge_primary_masks: the even / odd master rows shifted along the oblique, the vertical row repeated (shift_copy)
    int shift = 16;
    for (int i = 0; i < 64; i++) {
        if (i & 1) shift--;
        const uint8_t *row = (i & 1) ? kObliqueOdd : kObliqueEven;
        for (int x = 0; x < 64; x++) {
            const int s = x - shift;
            t.prim[0][kO63][i * 64 + x] = row[s < 0 ? 0 : (s > 63 ? 63 : s)];
            t.prim[0][kVer][i * 64 + x] = kVertical[x];
        }
    }
    for (int i = 0; i < 64; i++)
        for (int j = 0; j < 64; j++) {
            const uint8_t msk = t.prim[0][kO63][i * 64 + j], mskx = t.prim[0][kVer][i * 64 + j];
            t.prim[0][kO27][j * 64 + i]         = msk;
            t.prim[0][kO117][i * 64 + 63 - j]   = (uint8_t)(64 - msk);
            t.prim[0][kO153][(63 - j) * 64 + i] = (uint8_t)(64 - msk);
            t.prim[1][kO63][i * 64 + j]         = (uint8_t)(64 - msk);
            t.prim[1][kO27][j * 64 + i]         = (uint8_t)(64 - msk);
            t.prim[1][kO117][i * 64 + 63 - j]   = msk;
            t.prim[1][kO153][(63 - j) * 64 + i] = msk;
            t.prim[0][kHor][j * 64 + i]         = mskx;
            t.prim[1][kVer][i * 64 + j]         = (uint8_t)(64 - mskx);
            t.prim[1][kHor][j * 64 + i]         = (uint8_t)(64 - mskx);
        }
    // init_wedge_signs: the average of the sign-0 window's first row and first column
    for (int s = 0; s < 9; s++)
        for (int k = 0; k < 16; k++) {
            const int      bw = kWedgeW[s], bh = kWedgeH[s];
            const uint8_t *m  = t.prim[0][kCodebook[codebook_of(bw, bh)][k].dir] + window_offset(s, k);
            int            avg = 0;
            for (int i = 0; i < bw; i++) avg += m[i];
            for (int i = 1; i < bh; i++) avg += m[i * 64];
            avg          = (avg + (bw + bh - 1) / 2) / (bw + bh - 1);
            t.flip[s][k] = avg < 32;
            t.dir[s][k]  = kCodebook[codebook_of(bw, bh)][k].dir;
            t.off[s][k]  = (uint16_t)window_offset(s, k);
        }
    return t;
}

constexpr WedgeTables       kWedgeHost = make_wedge_tables();
__device__ const WedgeTables kWedge     = make_wedge_tables();

__device__ __forceinline__ int wedge_size(int w, int h) { // the index in kWedgeW / kWedgeH, -1: a size without wedges
    if (w == 8) return h == 8 ? 0 : (h == 16 ? 1 : (h == 32 ? 7 : -1));
    if (w == 16) return h == 8 ? 2 : (h == 16 ? 3 : (h == 32 ? 4 : -1));
    if (w == 32) return h == 16 ? 5 : (h == 32 ? 6 : (h == 8 ? 8 : -1));
    return -1;
}
// svt_aom_get_contiguous_soft_mask(index, sign, size) in place: row pitch 64
__device__ __forceinline__ const uint8_t *wedge_window(int size, int index, int sign) {
    return kWedge.prim[sign ^ kWedge.flip[size][index]][kWedge.dir[size][index]] + kWedge.off[size][index];
}
// the mask value of the plane's sample (x, y): the blend functions' four subw / subh branches
__device__ __forceinline__ int mask_at(const uint8_t *m, int pitch, int x, int y, int subw, int subh) {
    const uint8_t *p = m + (y << subh) * pitch + (x << subw);
    if (subw && subh) return (p[0] + p[pitch] + p[1] + p[pitch + 1] + 2) >> 2;
    if (subw) return (p[0] + p[1] + 1) >> 1;   // AOM_BLEND_AVG
    if (subh) return (p[0] + p[pitch] + 1) >> 1;
    return p[0];
}
// build_smooth_interintra_mask: the value at (x, y) of a w x h block
__device__ __forceinline__ int smooth_mask(int mode, int scale, int x, int y) {
    if (mode == 0) return 32;                                                   // II_DC_PRED
    return c_ii_weights[(mode == 1 ? y : (mode == 2 ? x : (y < x ? y : x))) * scale]; // II_V_PRED, II_H_PRED, II_SMOOTH_PRED
}
__device__ __forceinline__ bool is_interintra_size(int w, int h) { return w >= 8 && h >= 8 && w <= 32 && h <= 32 && w <= 2 * h && h <= 2 * w && wedge_size(w, h) >= 0; }

template <typename Px> __device__ __forceinline__ void store_quad(Px *p, const int *out) {
    if (sizeof(Px) == 2) {
        if (((uintptr_t)p & 7u) == 0) *(uint2 *)p = make_uint2((uint32_t)out[0] | ((uint32_t)out[1] << 16), (uint32_t)out[2] | ((uint32_t)out[3] << 16));
        else { p[0] = (Px)out[0]; p[1] = (Px)out[1]; p[2] = (Px)out[2]; p[3] = (Px)out[3]; }
    } else {
        if (((uintptr_t)p & 3u) == 0) *(uint32_t *)p = (uint32_t)out[0] | ((uint32_t)out[1] << 8) | ((uint32_t)out[2] << 16) | ((uint32_t)out[3] << 24);
        else { p[0] = (Px)out[0]; p[1] = (Px)out[1]; p[2] = (Px)out[2]; p[3] = (Px)out[3]; }
    }
}
template <typename Px> __device__ __forceinline__ void load_quad(const Px *p, int *v) {
    if (sizeof(Px) == 2) {
        if (((uintptr_t)p & 7u) == 0) {
            const uint2 t = *(const uint2 *)p;
            v[0] = (int)(t.x & 0xFFFFu); v[1] = (int)(t.x >> 16); v[2] = (int)(t.y & 0xFFFFu); v[3] = (int)(t.y >> 16);
            return;
        }
    } else if (((uintptr_t)p & 3u) == 0) {
        const uint32_t t = *(const uint32_t *)p;
        v[0] = (int)(t & 0xFFu); v[1] = (int)((t >> 8) & 0xFFu); v[2] = (int)((t >> 16) & 0xFFu); v[3] = (int)(t >> 24);
        return;
    }
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
}
// a w x h block at `offset` of a plane of `samples` samples with row pitch `stride` ends inside it
__device__ __forceinline__ bool block_inside(uint32_t offset, int w, int h, uint32_t stride, uint64_t samples) {
    return (uint64_t)offset + (uint64_t)(h - 1) * stride + (uint64_t)w <= samples;
}

// o[k] by selects: a run-time index would send the job record to memory
__device__ __forceinline__ uint32_t pick4(const uint32_t *o, int k) { return k == 0 ? o[0] : (k == 1 ? o[1] : (k == 2 ? o[2] : o[3])); }

// ---- masked compound prediction -----------------------------------------------------------------------------------------------------------
template <bool HBD> __global__ __launch_bounds__(64 * kWaves) void masked_pred_kernel(const SvtHipMaskedPredDesc d) {
    using Px = typename std::conditional<HBD, uint16_t, uint8_t>::type;
    __shared__ __attribute__((aligned(16))) uint16_t s_win[kWaves][kWinU16];
    __shared__ __attribute__((aligned(16))) int16_t  s_mid[kWaves][kMidU16];
    constexpr int bd = HBD ? 10 : 8, px_max = (1 << bd) - 1;
    const int      lane = (int)(threadIdx.x & 63u);
    const int      wave = uniform((int)(threadIdx.x >> 6));
    const uint32_t job  = blockIdx.x * (uint32_t)kWaves + (uint32_t)wave;
    if (job >= d.n_jobs) return;
    const SvtHipMaskedPredJob mj = d.jobs[job];
    const SvtHipInterPredJob &j  = mj.pred;
    const int  w = j.width, h = j.height, lw = mj.luma_width, lh = mj.luma_height;
    const bool diffwtd = mj.comp_type == SVT_HIP_MASK_DIFFWTD;

    bool ok = is_block_size(lw, lh) && w >= 4 && h >= 4 && w == (lw >> d.ss_x) && h == (lh >> d.ss_y) && j.filter_x <= 3 && j.filter_y <= 3;
    ok = ok && j.ref[0] < d.n_refs && j.ref[1] < d.n_refs && mj.comp_type <= 1; // NO_REF is above every n_refs
    if (j.flags & SVT_HIP_INTER_PRED_MV0_FROM_ARRAY) ok = ok && d.mv_array != nullptr && j.mv_index[0] < d.n_mvs;
    if (j.flags & SVT_HIP_INTER_PRED_MV1_FROM_ARRAY) ok = ok && d.mv_array != nullptr && j.mv_index[1] < d.n_mvs;
    int widx = mj.wedge_index, wsign = mj.wedge_sign, mtype = mj.mask_type;
    if (j.flags & SVT_HIP_MASK_PARAMS_FROM_ARRAY) {
        ok = ok && d.results != nullptr && mj.result_index < d.n_results;
        if (ok) {
            const SvtHipMaskSearchResult r = d.results[mj.result_index];
            widx = (int)(uint8_t)r.wedge_index; wsign = r.wedge_sign; mtype = r.mask_type;
        }
    }
    const int wsize = wedge_size(lw, lh);
    if (diffwtd) {
        ok = ok && lw >= 8 && lh >= 8 && mtype <= 1;
        if (d.plane != 0 || d.mask_buf != nullptr) ok = ok && d.mask_buf != nullptr && (uint64_t)mj.mask_offset + (uint64_t)(lw * lh) <= d.mask_bytes;
    } else
        ok = ok && wsize >= 0 && widx < 16 && wsign <= 1;
    ok = ok && block_inside(j.dst_offset, w, h, d.dst_stride, d.dst_samples);
    if (!ok) {
        if (lane == 0) d.status[job] = SVT_HIP_MASK_UNDEFINED;
        return;
    }

    RefView rv0, rv1;
    {
        const int mi0 = (int)j.mv_index[0], mi1 = (int)j.mv_index[1];
        int mvr0 = j.mv[0][0], mvc0 = j.mv[0][1], mvr1 = j.mv[1][0], mvc1 = j.mv[1][1];
        if (j.flags & SVT_HIP_INTER_PRED_MV0_FROM_ARRAY) { mvr0 = d.mv_array[2 * (size_t)mi0]; mvc0 = d.mv_array[2 * (size_t)mi0 + 1]; }
        if (j.flags & SVT_HIP_INTER_PRED_MV1_FROM_ARRAY) { mvr1 = d.mv_array[2 * (size_t)mi1]; mvc1 = d.mv_array[2 * (size_t)mi1 + 1]; }
        rv0 = ref_view(d, j, d.refs[j.ref[0]], uniform(mvr0), uniform(mvc0));
        rv1 = ref_view(d, j, d.refs[j.ref[1]], uniform(mvr1), uniform(mvc1));
    }
    const int tabx = filter_table(j.filter_x, w), taby = filter_table(j.filter_y, h);
    const TileWalk t = tile_walk(w, h, lane);
    // svt_aom_build_masked_compound_no_round derives the sub-sampling from the sizes
    const int subw = uniform(lw == 2 * w), subh = uniform(lh == 2 * h);
    const uint8_t *const wmask = diffwtd ? nullptr : wedge_window(wsize, uniform(widx), uniform(wsign));
    uint8_t *const       dmask = diffwtd && d.mask_buf ? d.mask_buf + mj.mask_offset : nullptr; // null for a luma batch without a mask buffer
    constexpr int ro = (1 << (bd + 4)) + (1 << (bd + 3)); // round_offset: offset_bits = bd + 11, round_1 = 7; round_bits = 4
    Px *const dst = (Px *)d.dst;

    for (int ty = 0; ty < h; ty += t.TH)
        for (int tx = 0; tx < w; tx += t.TW) {
            int a[4], b[4], m[4], out[4];
            compound_quad<HBD>(rv0, tabx, taby, t, rv0.pos_x + tx, rv0.pos_y + ty, s_win[wave], s_mid[wave], lane, a);
            compound_quad<HBD>(rv1, tabx, taby, t, rv1.pos_x + tx, rv1.pos_y + ty, s_win[wave], s_mid[wave], lane, b);
            if (!t.active) continue;
            const int x = tx + t.qx, y = ty + t.qy;
            if (!diffwtd) {
#pragma unroll
                for (int i = 0; i < 4; i++) m[i] = mask_at(wmask, 64, x + i, y, subw, subh);
            } else if (d.plane == 0) { // diffwtd_mask_d16: round = 4 + (bd - 8)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int diff = a[i] > b[i] ? a[i] - b[i] : b[i] - a[i];
                    const int v    = 38 + (((diff + (1 << (bd - 5))) >> (bd - 4)) >> 4);
                    m[i]           = v > 64 ? 64 : v;
                    if (mtype) m[i] = 64 - m[i];
                }
                if (dmask) {
                    uint8_t *p = dmask + y * lw + x;
                    if (((uintptr_t)p & 3u) == 0) *(uint32_t *)p = (uint32_t)m[0] | ((uint32_t)m[1] << 8) | ((uint32_t)m[2] << 16) | ((uint32_t)m[3] << 24);
                    else { p[0] = (uint8_t)m[0]; p[1] = (uint8_t)m[1]; p[2] = (uint8_t)m[2]; p[3] = (uint8_t)m[3]; }
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) m[i] = mask_at(dmask, lw, x + i, y, subw, subh);
            }
#pragma unroll
            for (int i = 0; i < 4; i++) { // svt_aom_{lowbd,highbd}_blend_a64_d16_mask_c
                const int res = ((m[i] * a[i] + (64 - m[i]) * b[i]) >> 6) - ro;
                out[i]        = clampi((res + 8) >> 4, 0, px_max);
            }
            store_quad<Px>(dst + (size_t)j.dst_offset + (size_t)y * d.dst_stride + (size_t)x, out);
        }
    if (lane == 0) d.status[job] = SVT_HIP_MASK_OK;
}

// ---- inter-intra combination --------------------------------------------------------------------------------------------------------------
template <bool HBD> __global__ __launch_bounds__(64 * kWaves) void interintra_blend_kernel(const SvtHipInterIntraDesc d) {
    using Px = typename std::conditional<HBD, uint16_t, uint8_t>::type;
    const int      lane = (int)(threadIdx.x & 63u);
    const uint32_t job  = blockIdx.x * (uint32_t)kWaves + (uint32_t)uniform((int)(threadIdx.x >> 6));
    if (job >= d.n_jobs) return;
    const SvtHipInterIntraJob j = d.jobs[job];
    const int w = j.width, h = j.height, lw = j.luma_width, lh = j.luma_height;
    const int subw = uniform(lw == 2 * w), subh = uniform(lh == 2 * h);
    bool ok = is_interintra_size(lw, lh) && w >= 4 && h >= 4 && (w == lw || subw) && (h == lh || subh);
    int mode = j.interintra_mode, use_wedge = j.use_wedge, widx = j.wedge_index;
    if (j.flags & SVT_HIP_MASK_PARAMS_FROM_ARRAY) {
        ok = ok && d.results != nullptr && j.result_index < d.n_results;
        if (ok) {
            const SvtHipMaskSearchResult r = d.results[j.result_index];
            mode = r.interintra_mode; use_wedge = r.use_wedge_interintra; widx = (int)(uint8_t)r.wedge_index;
        }
    }
    ok = ok && mode <= 3 && use_wedge <= 1 && (!use_wedge || (widx < 16 && j.wedge_sign <= 1));
    const uint32_t intra_offset = pick4(j.intra_offset, mode);
    ok = ok && block_inside(intra_offset, w, h, d.intra_stride, d.intra_samples) && block_inside(j.inter_offset, w, h, d.inter_stride, d.inter_samples) &&
        block_inside(j.dst_offset, w, h, d.dst_stride, d.dst_samples);
    if (!ok) {
        if (lane == 0) d.status[job] = SVT_HIP_MASK_UNDEFINED;
        return;
    }
    mode = uniform(mode); use_wedge = uniform(use_wedge);
    const uint8_t *const wmask = use_wedge ? wedge_window(wedge_size(lw, lh), uniform(widx), j.wedge_sign) : nullptr;
    const int scale = 128 / (w > h ? w : h); // ii_size_scales of the plane's block size
    const int qsh = w == 4 ? 0 : (w == 8 ? 1 : (w == 16 ? 2 : 3)), nq = (w * h) >> 2;
    const Px *const intra = (const Px *)d.intra + intra_offset;
    const Px *const inter = (const Px *)d.inter + j.inter_offset;
    Px *const       dst   = (Px *)d.dst + j.dst_offset;
    for (int q = lane; q < nq; q += 64) { // a sample is read and written by the same lane: the destination may be the inter block itself
        const int y = q >> qsh, x = (q & ((1 << qsh) - 1)) << 2;
        int a[4], b[4], out[4];
        load_quad<Px>(intra + (size_t)y * d.intra_stride + x, a);
        load_quad<Px>(inter + (size_t)y * d.inter_stride + x, b);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int m = use_wedge ? mask_at(wmask, 64, x + i, y, subw, subh) : smooth_mask(mode, scale, x + i, y);
            out[i]      = (m * a[i] + (64 - m) * b[i] + 32) >> 6; // AOM_BLEND_A64
        }
        store_quad<Px>(dst + (size_t)y * d.dst_stride + x, out);
    }
    if (lane == 0) d.status[job] = SVT_HIP_MASK_OK;
}

// ---- the searches ------------------------------------------------------------------------------------------------------------------------
static_assert(1024ll * 32768 * 64 == (1ll << 31) && 1024ll * 32767 * 64 <= INT32_MAX, "sum ds * m over a 32 x 32 block fits int32");

__device__ __forceinline__ uint32_t pack2(int lo, int hi) { return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16); }
__device__ __forceinline__ int lo16(uint32_t v) { return (int)(int16_t)(v & 0xFFFFu); }
__device__ __forceinline__ int hi16(uint32_t v) { return (int)v >> 16; }
typedef short short2v __attribute__((ext_vector_type(2)));
// c + a.lo * b.lo + a.hi * b.hi on packed int16 pairs: v_dot2_i32_i16
__device__ __forceinline__ int dot2(uint32_t a, uint32_t b, int c) {
#if __has_builtin(__builtin_amdgcn_sdot2)
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, a), __builtin_bit_cast(short2v, b), c, false);
#else
    return c + lo16(a) * lo16(b) + hi16(a) * hi16(b);
#endif
}
__device__ __forceinline__ int sat16(int v) { return clampi(v, -32768, 32767); } // one v_med3_i32
// ROUND_POWER_OF_TWO(csse, 2 * WEDGE_WEIGHT_BITS) of svt_av1_wedge_sse_from_residuals_c
__device__ __forceinline__ int64_t wedge_sse_round(uint64_t csse) { return (int64_t)((csse + 2048) >> 12); }

// The block of a kind-0 / kind-2 job in a lane's registers: quad k of the lane is quad 64 k + lane of the block, row-major
struct HeldBlock {
    uint32_t rd[4][4]; // per sample (r1, d) = (src - pred1, pred1 - pred0)
    int      x[4], y[4];
    bool     on[4];
};
// pick_wedge's loop body for one wedge on the mask of `sign` (with `ds`: the sign is chosen first): the wedge's sse
template <bool PICK_SIGN>
__device__ __forceinline__ int64_t wedge_sse(const HeldBlock &hb, const uint32_t (*ds)[2], int size, int index, int64_t sign_limit, int &sign) {
    const uint8_t *const win = wedge_window(size, index, 0);
    int m[4][4];
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int i = 0; i < 4; i++) m[k][i] = hb.on[k] ? win[hb.y[k] * 64 + hb.x[k] + i] : 0;
    sign = 0;
    if (PICK_SIGN) { // svt_av1_wedge_sign_from_residuals_c on the sign-0 mask
        int acc = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            acc = dot2(ds[k][0], pack2(m[k][0], m[k][1]), acc);
            acc = dot2(ds[k][1], pack2(m[k][2], m[k][3]), acc);
        }
        sign = (int64_t)(int32_t)wave_sum_dpp((uint32_t)acc) > sign_limit;
    }
    uint64_t csse = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int i = 0; i < 4; i++) { // the other sign's mask is 64 - m
            const int t = sat16(dot2(hb.rd[k][i], pack2(64, sign ? 64 - m[k][i] : m[k][i]), 0));
            csse += (uint32_t)(t * t);
        }
    return wedge_sse_round(wave_sum64_dpp(csse));
}

template <bool HBD> __global__ __launch_bounds__(64 * kWaves) void mask_search_kernel(const SvtHipMaskSearchDesc d) {
    using Px = typename std::conditional<HBD, uint16_t, uint8_t>::type;
    constexpr int bd = HBD ? 10 : 8;
    const int      lane = (int)(threadIdx.x & 63u);
    const uint32_t job  = blockIdx.x * (uint32_t)kWaves + (uint32_t)uniform((int)(threadIdx.x >> 6));
    if (job >= d.n_jobs) return;
    const SvtHipMaskSearchJob j = d.jobs[job];
    const int w = j.width, h = j.height, kind = uniform(j.kind);
    const int wsize = wedge_size(w, h);
    bool ok = kind <= 2 && block_inside(j.src_offset, w, h, d.src_stride, d.src_samples) && block_inside(j.pred1_offset, w, h, d.pred1_stride, d.pred1_samples);
    if (kind == SVT_HIP_MASK_SEARCH_WEDGE) ok = ok && wsize >= 0;
    if (kind == SVT_HIP_MASK_SEARCH_DIFFWTD) ok = ok && is_block_size(w, h) && w >= 8 && h >= 8;
    if (kind <= 1) ok = ok && d.pred0 != nullptr && block_inside(j.pred0_offset, w, h, d.pred0_stride, d.pred0_samples);
    if (kind == SVT_HIP_MASK_SEARCH_INTERINTRA) {
        ok = ok && is_interintra_size(w, h) && j.ii_wedge_mode <= 2 && d.intra != nullptr;
        for (int k = 0; k < 4; k++) ok = ok && block_inside(j.intra_offset[k], w, h, d.intra_stride, d.intra_samples);
    }
    if (!ok) {
        if (lane == 0) d.status[job] = SVT_HIP_MASK_UNDEFINED;
        return;
    }
    const int qsh = 31 - __builtin_clz(w >> 2), nq = (w * h) >> 2;
    const Px *const src = (const Px *)d.src + j.src_offset;
    const Px *const p1  = (const Px *)d.pred1 + j.pred1_offset;
    SvtHipMaskSearchResult res;
    memset(&res, 0, sizeof(res));

    if (kind == SVT_HIP_MASK_SEARCH_DIFFWTD) {
        const Px *const p0 = (const Px *)d.pred0 + j.pred0_offset;
        if (d.pred0_to_pred1_mult) { // a multiplier of 0 never exits: the SAD pass is not needed
            uint32_t sad = 0;
            for (int q = lane; q < nq; q += 64) {
                const int y = q >> qsh, x = (q & ((1 << qsh) - 1)) << 2;
                int a[4], b[4];
                load_quad<Px>(p0 + (size_t)y * d.pred0_stride + x, a);
                load_quad<Px>(p1 + (size_t)y * d.pred1_stride + x, b);
#pragma unroll
                for (int i = 0; i < 4; i++) sad += (uint32_t)(a[i] > b[i] ? a[i] - b[i] : b[i] - a[i]);
            }
            if (wave_sum_dpp(sad) < (uint32_t)(w * h) * d.pred0_to_pred1_mult) {
                if (lane == 0) { d.results[job].exit = 1; d.status[job] = SVT_HIP_MASK_OK; }
                return;
            }
        }
        uint64_t csse0 = 0, csse1 = 0;
        for (int q = lane; q < nq; q += 64) {
            const int y = q >> qsh, x = (q & ((1 << qsh) - 1)) << 2;
            int s[4], a[4], b[4];
            load_quad<Px>(src + (size_t)y * d.src_stride + x, s);
            load_quad<Px>(p0 + (size_t)y * d.pred0_stride + x, a);
            load_quad<Px>(p1 + (size_t)y * d.pred1_stride + x, b);
#pragma unroll
            for (int i = 0; i < 4; i++) { // diffwtd_mask / diffwtd_mask_highbd, base 38, and its inverse
                const int r1 = s[i] - b[i], dd = b[i] - a[i];
                const int v  = 38 + (((dd < 0 ? -dd : dd) >> (bd - 8)) >> 4), m0 = v > 64 ? 64 : v;
                const int t0 = sat16(64 * r1 + m0 * dd), t1 = sat16(64 * r1 + (64 - m0) * dd);
                csse0 += (uint32_t)(t0 * t0);
                csse1 += (uint32_t)(t1 * t1);
            }
        }
        const int64_t rd0 = wedge_sse_round(wave_sum64_dpp(csse0)), rd1 = wedge_sse_round(wave_sum64_dpp(csse1));
        res.mask_type = rd1 < rd0;
        res.best_rd   = rd1 < rd0 ? rd1 : rd0;
    } else {
        HeldBlock hb;
        uint32_t  sp[4][4]; // kind 2: per sample (source, inter prediction)
        uint32_t  ds[4][2]; // kind 0: svt_av1_wedge_compute_delta_squares_c, two samples a register
        uint32_t  sad = 0, ss0 = 0, ss1 = 0;
        const Px *const p0 = kind == SVT_HIP_MASK_SEARCH_WEDGE ? (const Px *)d.pred0 + j.pred0_offset : nullptr;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int q = 64 * k + lane;
            hb.on[k] = q < nq;
            hb.y[k] = q >> qsh; hb.x[k] = (q & ((1 << qsh) - 1)) << 2;
            int s[4] = {0, 0, 0, 0}, a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
            if (hb.on[k]) {
                load_quad<Px>(src + (size_t)hb.y[k] * d.src_stride + hb.x[k], s);
                load_quad<Px>(p1 + (size_t)hb.y[k] * d.pred1_stride + hb.x[k], b);
                if (p0) load_quad<Px>(p0 + (size_t)hb.y[k] * d.pred0_stride + hb.x[k], a);
            }
            int dsq[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int r1 = s[i] - b[i], r0 = s[i] - a[i], dd = b[i] - a[i];
                hb.rd[k][i] = pack2(r1, dd);
                sp[k][i]    = pack2(s[i], b[i]);
                sad += (uint32_t)(dd < 0 ? -dd : dd);
                ss0 += (uint32_t)(r0 * r0);
                ss1 += (uint32_t)(r1 * r1);
                dsq[i] = sat16(r0 * r0 - r1 * r1);
            }
            ds[k][0] = pack2(dsq[0], dsq[1]);
            ds[k][1] = pack2(dsq[2], dsq[3]);
        }
        if (kind == SVT_HIP_MASK_SEARCH_WEDGE) {
            if (wave_sum_dpp(sad) < (uint32_t)(w * h) * d.pred0_to_pred1_mult) {
                if (lane == 0) { d.results[job].exit = 1; d.status[job] = SVT_HIP_MASK_OK; }
                return;
            }
            const int64_t sign_limit = ((int64_t)wave_sum_dpp(ss0) - (int64_t)wave_sum_dpp(ss1)) * 32;
            int64_t best = INT64_MAX;
#pragma unroll 1
            for (int index = 0; index < 16; index++) {
                int           sign;
                const int64_t rd = wedge_sse<true>(hb, ds, wsize, index, sign_limit, sign);
                if (rd < best) { best = rd; res.wedge_index = (int8_t)index; res.wedge_sign = (uint8_t)sign; }
            }
            res.best_rd = best;
        } else {
            const int scale = 128 / (w > h ? w : h);
            int64_t   best  = INT64_MAX;
#pragma unroll 1
            for (int mode = 0; mode < 4; mode++) { // the smooth blend of intra block `mode` and its svt_aom_sse / svt_aom_highbd_sse
                const Px *const in = (const Px *)d.intra + pick4(j.intra_offset, mode);
                uint32_t        sse = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    int a[4] = {0, 0, 0, 0};
                    if (hb.on[k]) load_quad<Px>(in + (size_t)hb.y[k] * d.intra_stride + hb.x[k], a);
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int m = smooth_mask(mode, scale, hb.on[k] ? hb.x[k] + i : 0, hb.on[k] ? hb.y[k] : 0);
                        const int s = (int)(sp[k][i] & 0xFFFFu), b = (int)(sp[k][i] >> 16);
                        const int e = s - ((m * a[i] + (64 - m) * b + 32) >> 6);
                        sse += hb.on[k] ? (uint32_t)(e * e) : 0u;
                    }
                }
                const int64_t rd = (int64_t)wave_sum_dpp(sse);
                if (rd < best) { best = rd; res.interintra_mode = (uint8_t)mode; }
            }
            res.best_rd     = best;
            res.rd_wedge    = INT64_MAX;
            res.wedge_index = -1;
            if (j.ii_wedge_mode) { // pick_interintra_wedge: pred0 = the best mode's intra block, pred1 = the inter prediction, sign 0
                const Px *const in = (const Px *)d.intra + pick4(j.intra_offset, res.interintra_mode);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    int a[4] = {0, 0, 0, 0};
                    if (hb.on[k]) load_quad<Px>(in + (size_t)hb.y[k] * d.intra_stride + hb.x[k], a);
#pragma unroll
                    for (int i = 0; i < 4; i++) hb.rd[k][i] = hb.on[k] ? pack2(lo16(hb.rd[k][i]), (int)(sp[k][i] >> 16) - a[i]) : 0u;
                }
                int64_t bw = INT64_MAX;
#pragma unroll 1
                for (int index = 0; index < 16; index++) {
                    int           sign;
                    const int64_t rd = wedge_sse<false>(hb, ds, wsize, index, 0, sign);
                    if (rd < bw) { bw = rd; res.wedge_index = (int8_t)index; }
                }
                res.rd_wedge = bw;
            }
            res.use_wedge_interintra = j.ii_wedge_mode == 1 || res.rd_wedge < res.best_rd;
        }
    }
    if (lane == 0) { d.results[job] = res; d.status[job] = SVT_HIP_MASK_OK; }
}

} // namespace

extern "C" {

const uint8_t *svt_hip_wedge_primaries(void) { return &kWedgeHost.prim[0][0][0]; }
const uint8_t *svt_hip_wedge_signflip(void) { return &kWedgeHost.flip[0][0]; }

int svt_hip_masked_pred_check_desc(const SvtHipMaskedPredDesc *d) {
    if (!d) BAD("svt_hip_masked_pred_check_desc: null descriptor");
    if (!d->dst || !d->jobs || !d->status) BAD("svt_hip_masked_pred_check_desc: a mandatory pointer (dst, jobs, status) is null");
    if (d->bit_depth != 8 && d->bit_depth != 10) BAD("svt_hip_masked_pred_check_desc: bit_depth %u (8 or 10)", d->bit_depth);
    if (d->ss_x > 1 || d->ss_y > 1) BAD("svt_hip_masked_pred_check_desc: ss_x %u / ss_y %u (0 or 1)", d->ss_x, d->ss_y);
    if (d->plane > 2) BAD("svt_hip_masked_pred_check_desc: plane %u (0..2)", d->plane);
    if (d->plane == 0 && (d->ss_x || d->ss_y)) BAD("svt_hip_masked_pred_check_desc: a luma batch with ss_x %u / ss_y %u", d->ss_x, d->ss_y);
    const int rc = svt_hip_check_inter_pred_refs("svt_hip_masked_pred_check_desc", d->refs, d->n_refs);
    if (rc) return rc;
    if (d->dst_stride == 0 || d->dst_samples == 0) BAD("svt_hip_masked_pred_check_desc: dst_stride %u / dst_samples %llu is zero", d->dst_stride, (unsigned long long)d->dst_samples);
    if (d->n_mvs && !d->mv_array) BAD("svt_hip_masked_pred_check_desc: n_mvs %u without mv_array", d->n_mvs);
    if (d->n_results && !d->results) BAD("svt_hip_masked_pred_check_desc: n_results %u without results", d->n_results);
    if (d->mask_bytes && !d->mask_buf) BAD("svt_hip_masked_pred_check_desc: mask_bytes %llu without mask_buf", (unsigned long long)d->mask_bytes);
    return SVT_HIP_OK;
}

int svt_hip_interintra_blend_check_desc(const SvtHipInterIntraDesc *d) {
    if (!d) BAD("svt_hip_interintra_blend_check_desc: null descriptor");
    if (!d->intra || !d->inter || !d->dst || !d->jobs || !d->status)
        BAD("svt_hip_interintra_blend_check_desc: a mandatory pointer (intra, inter, dst, jobs, status) is null");
    if (d->bit_depth != 8 && d->bit_depth != 10) BAD("svt_hip_interintra_blend_check_desc: bit_depth %u (8 or 10)", d->bit_depth);
    if (d->intra_stride == 0 || d->inter_stride == 0 || d->dst_stride == 0) BAD("svt_hip_interintra_blend_check_desc: a stride is zero");
    if (d->intra_samples == 0 || d->inter_samples == 0 || d->dst_samples == 0) BAD("svt_hip_interintra_blend_check_desc: a sample count is zero");
    if (d->n_results && !d->results) BAD("svt_hip_interintra_blend_check_desc: n_results %u without results", d->n_results);
    return SVT_HIP_OK;
}

int svt_hip_mask_search_check_desc(const SvtHipMaskSearchDesc *d) {
    if (!d) BAD("svt_hip_mask_search_check_desc: null descriptor");
    if (!d->src || !d->pred1 || !d->jobs || !d->results || !d->status)
        BAD("svt_hip_mask_search_check_desc: a mandatory pointer (src, pred1, jobs, results, status) is null");
    if (d->bit_depth != 8 && d->bit_depth != 10) BAD("svt_hip_mask_search_check_desc: bit_depth %u (8 or 10)", d->bit_depth);
    if (d->use_rate) BAD("svt_hip_mask_search_check_desc: use_rate %u: the curve-fit rate model stays on the host", d->use_rate);
    if (d->use_rd_model) BAD("svt_hip_mask_search_check_desc: use_rd_model %u: the curve-fit rate model stays on the host", d->use_rd_model);
    if (d->src_stride == 0 || d->src_samples == 0 || d->pred1_stride == 0 || d->pred1_samples == 0)
        BAD("svt_hip_mask_search_check_desc: a stride or sample count of src / pred1 is zero");
    if (d->pred0 && (d->pred0_stride == 0 || d->pred0_samples == 0)) BAD("svt_hip_mask_search_check_desc: pred0 with a zero stride or sample count");
    if (d->intra && (d->intra_stride == 0 || d->intra_samples == 0)) BAD("svt_hip_mask_search_check_desc: intra with a zero stride or sample count");
    return SVT_HIP_OK;
}

size_t svt_hip_masked_pred_layout(int what, int field) {
#define D(f) offsetof(SvtHipMaskedPredDesc, f)
#define J(f) offsetof(SvtHipMaskedPredJob, f)
#define R(f) offsetof(SvtHipMaskSearchResult, f)
    static const size_t desc[] = {D(bit_depth), D(ss_x), D(ss_y), D(n_refs), D(n_jobs), D(refs), D(dst), D(dst_stride), D(plane), D(reserved), D(dst_samples),
                                  D(jobs), D(mv_array), D(n_mvs), D(n_results), D(results), D(mask_buf), D(mask_bytes), D(status)};
    static const size_t job[]  = {J(pred), J(comp_type), J(wedge_index), J(wedge_sign), J(mask_type), J(luma_width), J(luma_height), J(reserved), J(mask_offset),
                                  J(result_index)};
    static const size_t res[]  = {R(best_rd), R(rd_wedge), R(wedge_index), R(wedge_sign), R(mask_type), R(interintra_mode), R(use_wedge_interintra), R(exit),
                                  R(reserved)};
#undef D
#undef J
#undef R
    const SvtHipLayoutRow rows[] = {layout_row<SvtHipMaskedPredDesc>(desc), layout_row<SvtHipMaskedPredJob>(job), layout_row<SvtHipMaskSearchResult>(res)};
    return layout_lookup(rows, what, field);
}

size_t svt_hip_interintra_blend_layout(int what, int field) {
#define D(f) offsetof(SvtHipInterIntraDesc, f)
#define J(f) offsetof(SvtHipInterIntraJob, f)
    static const size_t desc[] = {D(bit_depth), D(reserved), D(n_jobs), D(intra), D(inter), D(dst), D(intra_stride), D(inter_stride), D(dst_stride), D(n_results),
                                  D(intra_samples), D(inter_samples), D(dst_samples), D(jobs), D(results), D(status)};
    static const size_t job[]  = {J(intra_offset), J(inter_offset), J(dst_offset), J(result_index), J(width), J(height), J(luma_width), J(luma_height),
                                  J(interintra_mode), J(use_wedge), J(wedge_index), J(wedge_sign), J(flags), J(reserved)};
#undef D
#undef J
    const SvtHipLayoutRow rows[] = {layout_row<SvtHipInterIntraDesc>(desc), layout_row<SvtHipInterIntraJob>(job)};
    return layout_lookup(rows, what, field);
}

size_t svt_hip_mask_search_layout(int what, int field) {
#define D(f) offsetof(SvtHipMaskSearchDesc, f)
#define J(f) offsetof(SvtHipMaskSearchJob, f)
    static const size_t desc[] = {D(bit_depth), D(pred0_to_pred1_mult), D(use_rate), D(use_rd_model), D(n_jobs), D(src), D(pred0), D(pred1), D(intra), D(src_stride),
                                  D(pred0_stride), D(pred1_stride), D(intra_stride), D(src_samples), D(pred0_samples), D(pred1_samples), D(intra_samples), D(jobs),
                                  D(results), D(status)};
    static const size_t job[]  = {J(src_offset), J(pred0_offset), J(pred1_offset), J(intra_offset), J(width), J(height), J(kind), J(ii_wedge_mode)};
#undef D
#undef J
    const SvtHipLayoutRow rows[] = {layout_row<SvtHipMaskSearchDesc>(desc), layout_row<SvtHipMaskSearchJob>(job)};
    return layout_lookup(rows, what, field);
}
int svt_hip_masked_pred_batch(SvtHipContext *ctx, const SvtHipMaskedPredDesc *d) {
    return enqueue_batch("svt_hip_masked_pred_batch", ctx, d, svt_hip_masked_pred_check_desc, &SvtHipMaskedPredDesc::n_jobs, [=] {
        hipLaunchKernelGGL(pick_hbd(d->bit_depth, masked_pred_kernel<true>, masked_pred_kernel<false>), dim3(ceil_div(d->n_jobs, kWaves)), dim3(64 * kWaves), 0,
                           ctx->stream, *d);
    });
}

int svt_hip_interintra_blend_batch(SvtHipContext *ctx, const SvtHipInterIntraDesc *d) {
    return enqueue_batch("svt_hip_interintra_blend_batch", ctx, d, svt_hip_interintra_blend_check_desc, &SvtHipInterIntraDesc::n_jobs, [=] {
        hipLaunchKernelGGL(pick_hbd(d->bit_depth, interintra_blend_kernel<true>, interintra_blend_kernel<false>), dim3(ceil_div(d->n_jobs, kWaves)), dim3(64 * kWaves), 0,
                           ctx->stream, *d);
    });
}

int svt_hip_mask_search_batch(SvtHipContext *ctx, const SvtHipMaskSearchDesc *d) {
    return enqueue_batch("svt_hip_mask_search_batch", ctx, d, svt_hip_mask_search_check_desc, &SvtHipMaskSearchDesc::n_jobs, [=] {
        hipLaunchKernelGGL(pick_hbd(d->bit_depth, mask_search_kernel<true>, mask_search_kernel<false>), dim3(ceil_div(d->n_jobs, kWaves)), dim3(64 * kWaves), 0,
                           ctx->stream, *d);
    });
}

} // extern "C"
