// obmc_kernel.hip -- overlapped block motion compensation (OBMC_CAUSAL) on gfx950: svt_hip_obmc_neighbour_batch, svt_hip_obmc_blend_batch,
// svt_hip_obmc_target_batch and svt_hip_obmc_search_batch, the steps between svt_hip_inter_pred_batch's prediction plane and the plane svt_hip_rd_batch reads.
//
// Reference functions restated (Source/Lib):
//   build_prediction_by_above_preds / _left_preds, build_prediction_by_above_pred / _left_pred     Codec/enc_inter_prediction.c:1133-1417
//   av1_setup_build_prediction_by_above_pred / _left_pred (the per-neighbour edges)                 Codec/enc_inter_prediction.c:743-777
//   get_single_prediction_for_obmc_luma / _chroma and their _hbd forms (the chroma origins)         Codec/enc_inter_prediction.c:778-1132
//   svt_av1_skip_u4x4_pred_in_obmc (DISABLE_CHROMA_U8X8_OBMC = 0)                                   Codec/inter_prediction.c:2282-2298
//   av1_build_obmc_inter_prediction, build_obmc_inter_pred_above / _left                            Codec/enc_inter_prediction.c:1430-1579
//   svt_aom_blend_a64_vmask_c / _hmask_c, svt_aom_highbd_blend_a64_vmask_16bit_c / _hmask_16bit_c   Codec/blend_a64_mask.c:302-340, Codec/inter_prediction.c:2374
//   calc_target_weighted_pred, svt_av1_calc_target_weighted_pred_above_c / _left_c                  Codec/enc_inter_prediction.c:1581-1638,1756-1816
//   svt_aom_precompute_obmc_data's svt_aom_un_pack2d of the 10-bit luma strips (sample >> 2)        Codec/enc_inter_prediction.c:1857-1874
//   svt_av1_get_obmc_mask                                                                           Codec/inter_prediction.c:2406-2429
//   single_motion_search (OBMC_CAUSAL), svt_av1_set_mv_search_range                                 Codec/mode_decision.c:2290-2398, Codec/av1me.c:205-226
//   svt_av1_obmc_full_pixel_search, obmc_refining_search_sad, get_obmc_mvpred_var                   Codec/av1me.c:709-776
//   svt_av1_find_best_obmc_sub_pixel_tree_up, set_subpel_mv_search_range                            Codec/av1me.c:778-790,963-1132
//   obmc_sad, obmc_variance                                                                         C_DEFAULT/sad_av1.c:18-32, C_DEFAULT/variance.c:347-373
// The per-neighbour prediction is convolve_core.h's: ref_view for the clamp and the position, single_quad for the four *_sr variants.
//
// Lay-out: one wave per job, four jobs per workgroup, no workgroup barrier.
//   neighbours  per span the wave walks the strip in tiles of up to 64 quads (tile_walk; a 4-wide strip in tiles of 32 rows, so that the window
//               fits the LDS slice), exactly as inter_pred_kernel walks a block; everything about a span is wave-uniform
//   blend       a lane per quad of the plane block; a sample depends on itself and on one sample of each strip, so the above pass, the left pass
//               and the corner where both act are three steps on the lane's four registers, with no synchronisation; untouched quads are skipped
//   target      a lane per quad of the luma block; the five steps of calc_target_weighted_pred collapse to one expression per sample for the
//               same reason.  wsrc is at most 255 * 4096 in magnitude and mask at most 4096: both are exact in int32.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include "batch_host.h"
#include "../../include/svt_hip_obmc.h"
#include "wave_ops.h"
#include "convolve_core.h"
#include "obmc_masks.h"
#include "mv_cost.h"
#include "subpel_interp.h"
#include <limits.h>

namespace {

constexpr int kWaves = 4;

__constant__ uint8_t c_obmc_mask[64] = SVT_HIP_OBMC_MASK_ROWS;
const uint8_t        h_obmc_mask[64] = SVT_HIP_OBMC_MASK_ROWS;

// one direction's spans: an even position, a size of 2, 4, 8 or 16 units (a block's side), ascending, inside the n4 units of the block's side
__device__ __forceinline__ bool spans_ok(const SvtHipObmcNeighbour *nb, int n, int n4) {
    bool ok  = true;
    int  end = 0;
    for (int k = 0; k < n; k++) {
        const int rel = nb[k].rel_pos, size = nb[k].size;
        ok  = ok && (rel & 1) == 0 && size >= 2 && (size & (size - 1)) == 0 && rel >= end && rel + size <= n4;
        end = rel + size;
    }
    return ok;
}

// what all three kernels ask of a block record
__device__ __forceinline__ bool block_ok(const SvtHipObmcBlock &b) {
    const int w = b.width, h = b.height;
    if (!is_block_size(w, h) || w < 8 || h < 8 || w > 64 || h > 64) return false;
    if (b.n_above > SVT_HIP_OBMC_MAX_NEIGHBOURS || b.n_left > SVT_HIP_OBMC_MAX_NEIGHBOURS) return false;
    return spans_ok(b.above, b.n_above, w >> 2) && spans_ok(b.left, b.n_left, h >> 2);
}

// svt_av1_skip_u4x4_pred_in_obmc, dir 0: the plane block sizes without above strips
__device__ __forceinline__ bool skips_above(int pw, int ph) { return (pw == 4 && ph <= 8) || (pw == 8 && ph == 4); }

// the span that covers position `pos` of the plane (sub-sampling ss), or -1
__device__ __forceinline__ int covering(const SvtHipObmcNeighbour *nb, int n, int pos, int ss) {
    int hit = -1;
    for (int k = 0; k < n; k++) {
        const int a = (nb[k].rel_pos * 4) >> ss, e = ((nb[k].rel_pos + nb[k].size) * 4) >> ss;
        if (pos >= a && pos < e) hit = k;
    }
    return hit;
}

template <typename Px> __device__ __forceinline__ void load_quad(const Px *p, int *v) {
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = p[i];
}
template <typename Px> __device__ __forceinline__ void store_quad(Px *p, const int *v) {
    if (sizeof(Px) == 2) {
        if (((uintptr_t)p & 7u) == 0) *(uint2 *)p = make_uint2((uint32_t)v[0] | ((uint32_t)v[1] << 16), (uint32_t)v[2] | ((uint32_t)v[3] << 16));
        else { p[0] = (Px)v[0]; p[1] = (Px)v[1]; p[2] = (Px)v[2]; p[3] = (Px)v[3]; }
    } else {
        if (((uintptr_t)p & 3u) == 0) *(uint32_t *)p = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
        else { p[0] = (Px)v[0]; p[1] = (Px)v[1]; p[2] = (Px)v[2]; p[3] = (Px)v[3]; }
    }
}

template <bool HBD> __global__ __launch_bounds__(64 * kWaves) void obmc_neighbour_kernel(const SvtHipObmcNeighbourDesc d) {
    using Px = typename std::conditional<HBD, uint16_t, uint8_t>::type;
    __shared__ __attribute__((aligned(16))) uint16_t s_win[kWaves][kWinU16];
    __shared__ __attribute__((aligned(16))) int16_t  s_mid[kWaves][kMidU16];
    const int      lane = (int)(threadIdx.x & 63u);
    const int      wave = uniform((int)(threadIdx.x >> 6));
    const uint32_t job  = blockIdx.x * (uint32_t)kWaves + (uint32_t)wave;
    if (job >= d.n_jobs) return;
    const SvtHipObmcJob jb = d.jobs[job];
    if (jb.block >= d.n_blocks) {
        if (lane == 0) d.status[job] = SVT_HIP_OBMC_UNDEFINED;
        return;
    }
    const SvtHipObmcBlock &b = d.blocks[jb.block];
    bool ok = block_ok(b);
    const int W = b.width, H = b.height, area = W * H;
    if (ok) {
        ok = (uint64_t)b.strip_offset + (uint64_t)(d.plane + 1) * (uint64_t)area <= d.strip_samples;
        for (int dir = 0; dir < 2; dir++) {
            const SvtHipObmcNeighbour *nb = dir ? b.left : b.above;
            const int n = dir ? b.n_left : b.n_above;
            for (int k = 0; k < n; k++) {
                ok = ok && nb[k].ref < d.n_refs && nb[k].filter_x <= 3 && nb[k].filter_y <= 3;
                if (nb[k].flags & SVT_HIP_OBMC_MV_FROM_ARRAY) ok = ok && d.mv_array != nullptr && nb[k].mv_index < d.n_mvs;
            }
        }
    }
    if (!ok) {
        if (lane == 0) d.status[job] = SVT_HIP_OBMC_UNDEFINED;
        return;
    }
    const int ssx = d.ss_x, ssy = d.ss_y, n4w = W >> 2, n4h = H >> 2;
    const bool chroma = d.plane != 0;
    uint16_t *win = s_win[wave];
    int16_t  *mid = s_mid[wave];
    for (int dir = 0; dir < 2; dir++) {
        if (dir == 0 && skips_above(W >> ssx, H >> ssy)) continue;
        const SvtHipObmcNeighbour *nbs = dir ? b.left : b.above;
        const int n = dir ? b.n_left : b.n_above;
        Px *const strip = (Px *)(dir ? d.left : d.above) + (size_t)b.strip_offset + (size_t)d.plane * (size_t)area;
#pragma unroll 1
        for (int k = 0; k < n; k++) {
            const SvtHipObmcNeighbour nb = nbs[k];
            const int rel = nb.rel_pos, size = nb.size;
            // the prediction size, the luma origin of the neighbour's part, the strip position and the four edges of this neighbour
            int bw, bh, lx = b.org_x, ly = b.org_y, dcol = 0, drow = 0;
            SvtHipInterPredJob pj;
            pj.mb_to_left_edge = b.mb_to_left_edge; pj.mb_to_right_edge = b.mb_to_right_edge;
            pj.mb_to_top_edge = b.mb_to_top_edge; pj.mb_to_bottom_edge = b.mb_to_bottom_edge;
            if (dir == 0) {
                bw = (size * 4) >> ssx; bh = H >> (ssy + 1); bh = bh < 4 ? 4 : bh;
                lx += rel * 4;
                dcol = chroma ? (((rel * 4) >> 3) << 3) >> ssx : rel * 4;
                pj.mb_to_left_edge   = -32 * ((b.org_x >> 2) + rel);
                pj.mb_to_right_edge  = b.mb_to_right_edge + (n4w - rel - size) * 32;
                pj.mb_to_bottom_edge = b.mb_to_bottom_edge + (H - (H / 2 < 32 ? H / 2 : 32)) * 8;
            } else {
                bw = W >> (ssx + 1); bw = bw < 4 ? 4 : bw; bh = (size * 4) >> ssy;
                ly += rel * 4;
                drow = chroma ? (((rel * 4) >> 3) << 3) >> ssy : rel * 4;
                pj.mb_to_top_edge    = -32 * ((b.org_y >> 2) + rel);
                pj.mb_to_bottom_edge = b.mb_to_bottom_edge + (n4h - rel - size) * 32;
                pj.mb_to_right_edge  = b.mb_to_right_edge + (W - (W / 2 < 32 ? W / 2 : 32)) * 8;
            }
            pj.width = (uint8_t)bw; pj.height = (uint8_t)bh;
            pj.org_x = (int16_t)(chroma ? ((lx >> 3) << 3) >> ssx : lx);
            pj.org_y = (int16_t)(chroma ? ((ly >> 3) << 3) >> ssy : ly);
            int mvr = nb.mv[0], mvc = nb.mv[1];
            if (nb.flags & SVT_HIP_OBMC_MV_FROM_ARRAY) { mvr = d.mv_array[2 * (size_t)nb.mv_index]; mvc = d.mv_array[2 * (size_t)nb.mv_index + 1]; }
            const RefView r = ref_view(d, pj, d.refs[nb.ref], uniform(mvr), uniform(mvc));
            const int tabx = filter_table(nb.filter_x, bw), taby = filter_table(nb.filter_y, bh);
            const TileWalk t = tile_walk_fit(bw, bh, lane);
            for (int ty = 0; ty < bh; ty += t.TH)
                for (int tx = 0; tx < bw; tx += t.TW) {
                    int out[4];
                    single_quad<HBD>(r, tabx, taby, t, r.pos_x + tx, r.pos_y + ty, win, mid, lane, out);
                    if (t.active && tx + t.qx < bw && ty + t.qy < bh) store_quad<Px>(strip + (size_t)(drow + ty + t.qy) * W + (size_t)(dcol + tx + t.qx), out);
                }
        }
    }
    if (lane == 0) d.status[job] = SVT_HIP_OBMC_OK;
}

template <bool HBD> __global__ __launch_bounds__(64 * kWaves) void obmc_blend_kernel(const SvtHipObmcBlendDesc d) {
    using Px = typename std::conditional<HBD, uint16_t, uint8_t>::type;
    const int      lane = (int)(threadIdx.x & 63u);
    const int      wave = uniform((int)(threadIdx.x >> 6));
    const uint32_t job  = blockIdx.x * (uint32_t)kWaves + (uint32_t)wave;
    if (job >= d.n_jobs) return;
    const SvtHipObmcJob jb = d.jobs[job];
    if (jb.block >= d.n_blocks) {
        if (lane == 0) d.status[job] = SVT_HIP_OBMC_UNDEFINED;
        return;
    }
    const SvtHipObmcBlock &b = d.blocks[jb.block];
    const int W = b.width, H = b.height, area = W * H, ssx = d.ss_x, ssy = d.ss_y, pw = W >> ssx, ph = H >> ssy;
    bool ok = block_ok(b);
    ok = ok && (uint64_t)b.strip_offset + (uint64_t)(d.plane + 1) * (uint64_t)area <= d.strip_samples;
    ok = ok && (uint64_t)jb.offset + (uint64_t)(ph > 0 ? ph - 1 : 0) * d.dst_stride + (uint64_t)pw <= d.dst_samples;
    if (!ok) {
        if (lane == 0) d.status[job] = SVT_HIP_OBMC_UNDEFINED;
        return;
    }
    // overlap: AOMMIN(block_size_high, 64) >> 1 rows above, AOMMIN(block_size_wide, 64) >> 1 columns on the left, on this plane
    const int  ov_a = (H >> 1) >> ssy, ov_l = (W >> 1) >> ssx;
    const int  n_above = skips_above(pw, ph) ? 0 : b.n_above;
    const Px  *above = (const Px *)d.above + (size_t)b.strip_offset + (size_t)d.plane * (size_t)area;
    const Px  *left  = (const Px *)d.left + (size_t)b.strip_offset + (size_t)d.plane * (size_t)area;
    Px *const  dst   = (Px *)d.dst + (size_t)jb.offset;
    const int  qpr = pw >> 2, qsh = 31 - __builtin_clz(qpr), nq = qpr * ph;
    for (int q = lane; q < nq; q += 64) {
        const int  y = q >> qsh, x = (q & (qpr - 1)) << 2;
        const bool in_a = y < ov_a && covering(b.above, n_above, x, ssx) >= 0;
        const bool in_l = x < ov_l && covering(b.left, b.n_left, y, ssy) >= 0;
        if (!in_a && !in_l) continue;
        Px *p = dst + (size_t)y * d.dst_stride + (size_t)x;
        int v[4], t[4];
        load_quad<Px>(p, v);
        if (in_a) { // svt_aom_blend_a64_vmask: AOM_BLEND_A64(mask[row], dst, above)
            const int m = c_obmc_mask[ov_a + y];
            load_quad<Px>(above + (size_t)y * W + x, t);
#pragma unroll
            for (int i = 0; i < 4; i++) v[i] = (m * v[i] + (64 - m) * t[i] + 32) >> 6;
        }
        if (in_l) { // svt_aom_blend_a64_hmask on the result of the above pass: AOM_BLEND_A64(mask[col], dst, left)
            load_quad<Px>(left + (size_t)y * W + x, t);
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (x + i < ov_l) {
                    const int m = c_obmc_mask[ov_l + x + i];
                    v[i] = (m * v[i] + (64 - m) * t[i] + 32) >> 6;
                }
        }
        store_quad<Px>(p, v);
    }
    if (lane == 0) d.status[job] = SVT_HIP_OBMC_OK;
}

template <bool HBD> __global__ __launch_bounds__(64 * kWaves) void obmc_target_kernel(const SvtHipObmcTargetDesc d) {
    using Px = typename std::conditional<HBD, uint16_t, uint8_t>::type;
    const int      lane = (int)(threadIdx.x & 63u);
    const int      wave = uniform((int)(threadIdx.x >> 6));
    const uint32_t job  = blockIdx.x * (uint32_t)kWaves + (uint32_t)wave;
    if (job >= d.n_jobs) return;
    const SvtHipObmcJob jb = d.jobs[job];
    if (jb.block >= d.n_blocks) {
        if (lane == 0) d.status[job] = SVT_HIP_OBMC_UNDEFINED;
        return;
    }
    const SvtHipObmcBlock &b = d.blocks[jb.block];
    const int W = b.width, H = b.height, area = W * H;
    bool ok = block_ok(b);
    ok = ok && (uint64_t)b.strip_offset + (uint64_t)area <= d.strip_samples && (uint64_t)jb.offset + (uint64_t)area <= d.out_values;
    ok = ok && b.org_x >= 0 && b.org_y >= 0 && (uint64_t)(b.org_y + H - 1) * d.src_stride + (uint64_t)(b.org_x + W) <= d.src_samples;
    if (!ok) {
        if (lane == 0) d.status[job] = SVT_HIP_OBMC_UNDEFINED;
        return;
    }
    const int      ov_a = H >> 1, ov_l = W >> 1;
    const Px      *above = (const Px *)d.above + (size_t)b.strip_offset, *left = (const Px *)d.left + (size_t)b.strip_offset;
    const uint8_t *src  = d.src + (size_t)b.org_y * d.src_stride + (size_t)b.org_x;
    int32_t *const wsrc = d.wsrc + (size_t)jb.offset, *const mask = d.mask + (size_t)jb.offset;
    const int      qpr = W >> 2, qsh = 31 - __builtin_clz(qpr), nq = qpr * H;
    for (int q = lane; q < nq; q += 64) {
        const int  y = q >> qsh, x = (q & (qpr - 1)) << 2;
        const bool in_a = y < ov_a && covering(b.above, b.n_above, x, 0) >= 0;
        const bool in_l = x < ov_l && covering(b.left, b.n_left, y, 0) >= 0;
        int w4[4] = {0, 0, 0, 0}, m4[4] = {64, 64, 64, 64}, t[4], s[4];
        if (in_a) { // svt_av1_calc_target_weighted_pred_above_c
            const int m0 = c_obmc_mask[ov_a + y];
            load_quad<Px>(above + (size_t)y * W + x, t);
#pragma unroll
            for (int i = 0; i < 4; i++) { w4[i] = (64 - m0) * (HBD ? (t[i] >> 2) & 0xFF : t[i]); m4[i] = m0; }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) { w4[i] *= 64; m4[i] *= 64; }
        if (in_l) { // svt_av1_calc_target_weighted_pred_left_c: ov_l is a multiple of 4, so the quad is inside or outside as a whole
            load_quad<Px>(left + (size_t)y * W + x, t);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int m0 = c_obmc_mask[ov_l + x + i], tl = HBD ? (t[i] >> 2) & 0xFF : t[i];
                w4[i] = (w4[i] >> 6) * m0 + (tl << 6) * (64 - m0);
                m4[i] = (m4[i] >> 6) * m0;
            }
        }
        load_quad<uint8_t>(src + (size_t)y * d.src_stride + x, s);
#pragma unroll
        for (int i = 0; i < 4; i++) w4[i] = s[i] * 4096 - w4[i];
        int32_t *pw = wsrc + (size_t)y * W + x, *pm = mask + (size_t)y * W + x;
        if ((((uintptr_t)pw | (uintptr_t)pm) & 15u) == 0) {
            *(int4 *)pw = make_int4(w4[0], w4[1], w4[2], w4[3]);
            *(int4 *)pm = make_int4(m4[0], m4[1], m4[2], m4[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) { pw[i] = w4[i]; pm[i] = m4[i]; }
        }
    }
    if (lane == 0) d.status[job] = SVT_HIP_OBMC_OK;
}


// ---- the OBMC motion search ---------------------------------------------------------------------------------------------------------------
// One wave per job; the control flow of both searches is wave-uniform scalar code, a candidate's error spreads the block's samples over the lanes.
// wsrc / mask stay where svt_hip_obmc_target_batch wrote them (global memory, 8 bytes per sample): a search evaluates at most
// fpel_search_range * 8 + 1 full-pel and 25 sub-pel positions, each one coalesced pass over at most 32 KiB that the caches hold; an LDS copy
// of a 64x64 block (32 KiB) would leave five waves to a CU.
// Sum widths: |diff| <= 255 per sample (wsrc and pre * mask are both within 255 * 4096), so the SAD and the sum over 4096 samples are below
// 2^21 and the sum of squares below 2^28: 32 bits; sum * sum needs 64.
struct ObmcSearch {
    const int32_t *wsrc, *mask;
    const uint8_t *ref; // the co-located block's first sample
    int            stride, w, h, lw;
    bool           light;
    int            sadpb, epb;
    const int32_t *mvjcost, *trow, *tcol;
    SvtHipMv       ref_mv;
};

// obmc_sad (C_DEFAULT/sad_av1.c:18-32) at the full-pel position (row, col)
__device__ __forceinline__ uint32_t wave_obmc_sad(const ObmcSearch &s, int row, int col) {
    const uint8_t *p = s.ref + (ptrdiff_t)row * s.stride + col;
    uint32_t sad = 0;
    const int n = s.w * s.h;
    for (int i = threadIdx.x & 63; i < n; i += 64) {
        const int y = i >> s.lw, x = i & (s.w - 1);
        const int d = s.wsrc[i] - (int)p[(ptrdiff_t)y * s.stride + x] * s.mask[i];
        sad += (uint32_t)((d < 0 ? -d : d) + 2048) >> 12;
    }
    return wave_sum(sad);
}

// obmc_variance (C_DEFAULT/variance.c:347-373) of svt_aom_upsampled_pred (USE_8_TAPS) at the 1/8 vector (row, col)
__device__ __forceinline__ uint32_t wave_obmc_variance(const ObmcSearch &s, int row, int col, uint32_t &sse_out) {
    const uint8_t *p = s.ref + (ptrdiff_t)(row >> 3) * s.stride + (col >> 3);
    const int xo = col & 7, yo = row & 7;
    int fx[8], fy[8];
#pragma unroll
    for (int k = 0; k < 8; k++) { fx[k] = c_subpel_filters[2][xo][k]; fy[k] = c_subpel_filters[2][yo][k]; }
    int      sum = 0;
    uint32_t sse = 0;
    const int n = s.w * s.h;
    for (int i = threadIdx.x & 63; i < n; i += 64) {
        const int y = i >> s.lw, x = i & (s.w - 1);
        const int v = upsampled_sample(p + (ptrdiff_t)y * s.stride + x, (uint32_t)s.stride, xo, yo, fx, fy);
        const int d = s.wsrc[i] - v * s.mask[i];
        const int diff = d < 0 ? -((-d + 2048) >> 12) : (d + 2048) >> 12; // ROUND_POWER_OF_TWO_SIGNED
        sum += diff;
        sse += (uint32_t)(diff * diff);
    }
    sum = wave_sum(sum);
    sse = wave_sum(sse);
    sse_out = sse;
    return sse - (uint32_t)(((long long)sum * sum) / n);
}

// svt_aom_mv_err_cost / svt_aom_mv_err_cost_light of the 1/8 vector (row, col) as an MV (int16)
__device__ __forceinline__ int obmc_mv_err_cost(const ObmcSearch &s, int row, int col) {
    if (s.light) return mv_err_cost_light((int16_t)row, (int16_t)col, s.ref_mv);
    const MvCost mc = {s.ref_mv, SVT_HIP_MV_COST_ENTROPY, s.epb, s.mvjcost, s.trow, s.tcol};
    return mv_err_cost((int16_t)row, (int16_t)col, mc);
}

__global__ void __launch_bounds__(64) obmc_search_kernel(const SvtHipObmcSearchDesc d) {
    const uint32_t job  = blockIdx.x;
    const int      lane = (int)threadIdx.x;
    const SvtHipObmcSearchJob jb = d.jobs[job];
    const int  w = jb.width, h = jb.height;
    const bool do_full = d.refine_level == 0 || d.refine_level == 1 || d.refine_level == 3;
    bool ok = is_block_size(w, h) && w >= 8 && h >= 8 && w <= 64 && h <= 64;
    ok = ok && (uint64_t)jb.target_offset + (uint64_t)(w * h) <= d.target_values;
    // single_motion_search: the full-pel limits narrowed by svt_av1_set_mv_search_range (Codec/av1me.c:205-226), and the start
    int col_min = jb.col_min, col_max = jb.col_max, row_min = jb.row_min, row_max = jb.row_max;
    int br = jb.start_mv.row >> 3, bc = jb.start_mv.col >> 3;
    if (do_full) {
        const int rc = jb.ref_mv.col, rr = jb.ref_mv.row;
        int cmin = (rc >> 3) - 1023 + ((rc & 7) != 0), rmin = (rr >> 3) - 1023 + ((rr & 7) != 0), cmax = (rc >> 3) + 1023, rmax = (rr >> 3) + 1023; // MAX_FULL_PEL_VAL
        cmin = cmin > -2047 ? cmin : -2047; rmin = rmin > -2047 ? rmin : -2047; // (MV_LOW >> 3) + 1
        cmax = cmax < 2047 ? cmax : 2047; rmax = rmax < 2047 ? rmax : 2047;     // (MV_UPP >> 3) - 1
        col_min = col_min < cmin ? cmin : col_min; col_max = col_max > cmax ? cmax : col_max;
        row_min = row_min < rmin ? rmin : row_min; row_max = row_max > rmax ? rmax : row_max;
        bc = clip3(col_min, col_max, bc); br = clip3(row_min, row_max, br); // clamp_mv, twice in the reference
    }
    { // every position the search can reach reads inside the reference buffer.  From the start the full-pel search moves at most fpel_search_range
      // samples; from where it ends the tree moves at most 4 + 4, 2 + 2, 1 + 1 = 14 eighths either way in each axis (a round's step plus its
      // second-level check): floor(-14 / 8) = -2 samples and floor(14 / 8) = 1; the eight taps then reach 3 samples before and 4 after
        const long long range = do_full ? (long long)d.fpel_search_range : 0, before = range + 2 + 3, after = range + 1 + 4;
        const long long lo = (long long)jb.ref_offset + (br - before) * (long long)d.ref_stride + (bc - before);
        const long long hi = (long long)jb.ref_offset + (br + after + h - 1) * (long long)d.ref_stride + (bc + after + w - 1);
        ok = ok && lo >= 0 && hi < (long long)d.ref_samples;
    }
    if (!ok) {
        if (lane == 0) d.status[job] = SVT_HIP_OBMC_UNDEFINED;
        return;
    }
    ObmcSearch s;
    s.wsrc = d.wsrc + jb.target_offset; s.mask = d.mask + jb.target_offset; s.ref = d.ref + jb.ref_offset;
    s.stride = (int)d.ref_stride; s.w = w; s.h = h; s.lw = 31 - __builtin_clz(w);
    s.light = d.approx_inter_rate != 0; s.sadpb = d.sadpb; s.epb = d.error_per_bit;
    s.mvjcost = d.mvjcost; s.trow = d.mvcost[0]; s.tcol = d.mvcost[1]; s.ref_mv = jb.ref_mv;

    int fullpel_value = 0;
    if (do_full) { // obmc_refining_search_sad, then get_obmc_mvpred_var
        const int nr[8] = {-1, 0, 0, 1, -1, 1, 1, -1}, nc[8] = {0, -1, 1, 0, 1, 1, -1, -1};
        const int fr = jb.ref_mv.row >> 3, fc = jb.ref_mv.col >> 3;
        uint32_t best_sad = wave_obmc_sad(s, br, bc) + (uint32_t)mvsad_err_cost(br, bc, fr, fc, s.light, s.sadpb, s.mvjcost, s.trow, s.tcol);
        const int sites = d.fpel_search_diag ? 8 : 4;
        for (uint32_t i = 0; i < d.fpel_search_range; i++) {
            int best_site = -1;
#pragma unroll 1
            for (int j = 0; j < sites; j++) {
                const int r = br + nr[j], c = bc + nc[j];
                if (c >= col_min && c <= col_max && r >= row_min && r <= row_max) { // is_mv_in
                    uint32_t sad = wave_obmc_sad(s, r, c);
                    if (sad < best_sad) {
                        sad += (uint32_t)mvsad_err_cost(r, c, fr, fc, s.light, s.sadpb, s.mvjcost, s.trow, s.tcol);
                        if (sad < best_sad) { best_sad = sad; best_site = j; }
                    }
                }
            }
            if (best_site == -1) break;
            br += nr[best_site]; bc += nc[best_site];
        }
        uint32_t unused;
        fullpel_value = (int)(wave_obmc_variance(s, br * 8, bc * 8, unused) + (uint32_t)obmc_mv_err_cost(s, br * 8, bc * 8));
    }

    // svt_av1_find_best_obmc_sub_pixel_tree_up: set_subpel_mv_search_range on the limits single_motion_search restored (the job's own)
    const int max_mv = 1023 * 8;
    int minc = jb.col_min * 8 > jb.ref_mv.col - max_mv ? jb.col_min * 8 : jb.ref_mv.col - max_mv;
    int maxc = jb.col_max * 8 < jb.ref_mv.col + max_mv ? jb.col_max * 8 : jb.ref_mv.col + max_mv;
    int minr = jb.row_min * 8 > jb.ref_mv.row - max_mv ? jb.row_min * 8 : jb.ref_mv.row - max_mv;
    int maxr = jb.row_max * 8 < jb.ref_mv.row + max_mv ? jb.row_max * 8 : jb.ref_mv.row + max_mv;
    minc = minc > -16383 ? minc : -16383; maxc = maxc < 16383 ? maxc : 16383; minr = minr > -16383 ? minr : -16383; maxr = maxr < 16383 ? maxr : 16383;
    br *= 8; bc *= 8;
    uint32_t sse1 = 0, sse = 0, besterr;
    int      distortion;
    besterr    = wave_obmc_variance(s, br, bc, sse1); // upsampled_setup_obmc_center_error
    distortion = (int)besterr;
    besterr += (uint32_t)obmc_mv_err_cost(s, br, bc);
    const int round = d.allow_hp ? 3 : 2;
    int hstep = 4, tr = 0, tc = 0;
    // CHECK_BETTER1
    auto check = [&](int r, int c) -> uint32_t {
        if (c >= minc && c <= maxc && r >= minr && r <= maxr) {
            const uint32_t thismse = wave_obmc_variance(s, r, c, sse);
            const uint32_t v = (uint32_t)obmc_mv_err_cost(s, r, c);
            if (v + thismse < besterr) { besterr = v + thismse; br = r; bc = c; distortion = (int)thismse; sse1 = sse; }
            return v;
        }
        return (uint32_t)INT_MAX;
    };
#pragma unroll 1
    for (int iter = 0; iter < round; iter++) {
        const int sr[4] = {0, 0, -hstep, hstep}, sc[4] = {-hstep, hstep, 0, 0}; // search_step_table: left, right, up, down
        uint32_t cost[5];
        int best_idx = -1;
#pragma unroll 1
        for (int idx = 0; idx < 4; idx++) {
            tr = br + sr[idx]; tc = bc + sc[idx];
            if (tc >= minc && tc <= maxc && tr >= minr && tr <= maxr) {
                const uint32_t thismse = wave_obmc_variance(s, tr, tc, sse);
                cost[idx] = thismse + (uint32_t)obmc_mv_err_cost(s, tr, tc);
                if (cost[idx] < besterr) { best_idx = idx; besterr = cost[idx]; distortion = (int)thismse; sse1 = sse; }
            } else
                cost[idx] = (uint32_t)INT_MAX;
        }
        int kc = cost[0] <= cost[1] ? -hstep : hstep, kr = cost[2] <= cost[3] ? -hstep : hstep;
        tc = bc + kc; tr = br + kr;
        if (tc >= minc && tc <= maxc && tr >= minr && tr <= maxr) {
            const uint32_t thismse = wave_obmc_variance(s, tr, tc, sse);
            cost[4] = thismse + (uint32_t)obmc_mv_err_cost(s, tr, tc);
            if (cost[4] < besterr) { best_idx = 4; besterr = cost[4]; distortion = (int)thismse; sse1 = sse; }
        }
        if (best_idx >= 0 && best_idx < 4) { br += sr[best_idx]; bc += sc[best_idx]; }
        else if (best_idx == 4) { br = tr; bc = tc; }
        if (best_idx != -1) { // SECOND_LEVEL_CHECKS_BEST(1), iters_per_step = 2
            const int br0 = br, bc0 = bc;
            if (tr == br && tc != bc) kc = bc - tc;
            else if (tr != br && tc == bc) kr = br - tr;
            check(br0 + kr, bc0);
            check(br0, bc0 + kc);
            if (br0 != br || bc0 != bc) check(br0 + kr, bc0 + kc);
        }
        hstep >>= 1;
    }
    if (lane == 0) {
        d.best_mv[2 * (size_t)job] = (int16_t)br; d.best_mv[2 * (size_t)job + 1] = (int16_t)bc;
        SvtHipObmcSearchResult r;
        r.fullpel_value = fullpel_value; r.besterr = besterr; r.distortion = distortion; r.sse1 = sse1;
        r.rate_mv = mv_bit_cost((int16_t)br, (int16_t)bc, jb.ref_mv, s.light, s.mvjcost, s.trow, s.tcol); r.reserved = 0;
        d.results[job] = r;
        d.status[job] = SVT_HIP_OBMC_OK;
    }
}

} // namespace

extern "C" {

int svt_hip_obmc_neighbour_check_desc(const SvtHipObmcNeighbourDesc *d) {
    if (!d) BAD("svt_hip_obmc_neighbour_check_desc: null descriptor");
    if (!d->blocks || !d->jobs || !d->above || !d->left || !d->status)
        BAD("svt_hip_obmc_neighbour_check_desc: a mandatory pointer (blocks, jobs, above, left, status) is null");
    if (d->bit_depth != 8 && d->bit_depth != 10) BAD("svt_hip_obmc_neighbour_check_desc: bit_depth %u (8 or 10)", d->bit_depth);
    if (d->ss_x > 1 || d->ss_y > 1) BAD("svt_hip_obmc_neighbour_check_desc: ss_x %u / ss_y %u (0 or 1)", d->ss_x, d->ss_y);
    if (d->plane > 2) BAD("svt_hip_obmc_neighbour_check_desc: plane %u (0 luma, 1 Cb, 2 Cr)", d->plane);
    if (d->plane == 0 && (d->ss_x || d->ss_y)) BAD("svt_hip_obmc_neighbour_check_desc: a luma batch with sub-sampling %u / %u", d->ss_x, d->ss_y);
    const int rc = svt_hip_check_inter_pred_refs("svt_hip_obmc_neighbour_check_desc", d->refs, d->n_refs);
    if (rc) return rc;
    if (d->n_blocks == 0 || d->strip_samples == 0)
        BAD("svt_hip_obmc_neighbour_check_desc: n_blocks %u / strip_samples %llu is zero", d->n_blocks, (unsigned long long)d->strip_samples);
    if (d->n_mvs && !d->mv_array) BAD("svt_hip_obmc_neighbour_check_desc: n_mvs %u without mv_array", d->n_mvs);
    return SVT_HIP_OK;
}

int svt_hip_obmc_blend_check_desc(const SvtHipObmcBlendDesc *d) {
    if (!d) BAD("svt_hip_obmc_blend_check_desc: null descriptor");
    if (!d->blocks || !d->jobs || !d->above || !d->left || !d->dst || !d->status)
        BAD("svt_hip_obmc_blend_check_desc: a mandatory pointer (blocks, jobs, above, left, dst, status) is null");
    if (d->bit_depth != 8 && d->bit_depth != 10) BAD("svt_hip_obmc_blend_check_desc: bit_depth %u (8 or 10)", d->bit_depth);
    if (d->ss_x > 1 || d->ss_y > 1) BAD("svt_hip_obmc_blend_check_desc: ss_x %u / ss_y %u (0 or 1)", d->ss_x, d->ss_y);
    if (d->plane > 2) BAD("svt_hip_obmc_blend_check_desc: plane %u (0 luma, 1 Cb, 2 Cr)", d->plane);
    if (d->plane == 0 && (d->ss_x || d->ss_y)) BAD("svt_hip_obmc_blend_check_desc: a luma batch with sub-sampling %u / %u", d->ss_x, d->ss_y);
    if (d->n_blocks == 0 || d->strip_samples == 0 || d->dst_stride == 0 || d->dst_samples == 0)
        BAD("svt_hip_obmc_blend_check_desc: n_blocks %u / strip_samples %llu / dst_stride %u / dst_samples %llu is zero", d->n_blocks,
            (unsigned long long)d->strip_samples, d->dst_stride, (unsigned long long)d->dst_samples);
    return SVT_HIP_OK;
}

int svt_hip_obmc_target_check_desc(const SvtHipObmcTargetDesc *d) {
    if (!d) BAD("svt_hip_obmc_target_check_desc: null descriptor");
    if (!d->blocks || !d->jobs || !d->above || !d->left || !d->src || !d->wsrc || !d->mask || !d->status)
        BAD("svt_hip_obmc_target_check_desc: a mandatory pointer (blocks, jobs, above, left, src, wsrc, mask, status) is null");
    if (d->strip_bit_depth != 8 && d->strip_bit_depth != 10) BAD("svt_hip_obmc_target_check_desc: strip_bit_depth %u (8 or 10)", d->strip_bit_depth);
    if (d->n_blocks == 0 || d->strip_samples == 0 || d->src_stride == 0 || d->src_samples == 0 || d->out_values == 0)
        BAD("svt_hip_obmc_target_check_desc: n_blocks %u / strip_samples %llu / src_stride %u / src_samples %llu / out_values %llu is zero", d->n_blocks,
            (unsigned long long)d->strip_samples, d->src_stride, (unsigned long long)d->src_samples, (unsigned long long)d->out_values);
    return SVT_HIP_OK;
}

int svt_hip_obmc_search_check_desc(const SvtHipObmcSearchDesc *d) {
    if (!d) BAD("svt_hip_obmc_search_check_desc: null descriptor");
    if (!d->ref || !d->wsrc || !d->mask || !d->jobs || !d->best_mv || !d->results || !d->status)
        BAD("svt_hip_obmc_search_check_desc: a mandatory pointer (ref, wsrc, mask, jobs, best_mv, results, status) is null");
    if (!d->approx_inter_rate && (!d->mvjcost || !d->mvcost[0] || !d->mvcost[1]))
        BAD("svt_hip_obmc_search_check_desc: mvjcost / mvcost are null and approx_inter_rate is 0");
    if (d->ref_bit_depth != 8) BAD("svt_hip_obmc_search_check_desc: ref_bit_depth %u (the search works on 8-bit reference planes)", d->ref_bit_depth);
    if (d->refine_level > 4) BAD("svt_hip_obmc_search_check_desc: refine_level %u (0..4)", d->refine_level);
    if (d->fpel_search_range > SVT_HIP_OBMC_MAX_FPEL_RANGE)
        BAD("svt_hip_obmc_search_check_desc: fpel_search_range %u (at most %d)", d->fpel_search_range, SVT_HIP_OBMC_MAX_FPEL_RANGE);
    if (d->ref_stride == 0 || d->ref_samples == 0 || d->target_values == 0)
        BAD("svt_hip_obmc_search_check_desc: ref_stride %u / ref_samples %llu / target_values %llu is zero", d->ref_stride, (unsigned long long)d->ref_samples,
            (unsigned long long)d->target_values);
    return SVT_HIP_OK;
}

size_t svt_hip_obmc_layout(int what, int field) {
#define N(f) offsetof(SvtHipObmcNeighbourDesc, f)
#define B(f) offsetof(SvtHipObmcBlendDesc, f)
#define T(f) offsetof(SvtHipObmcTargetDesc, f)
#define K(f) offsetof(SvtHipObmcBlock, f)
#define H(f) offsetof(SvtHipObmcNeighbour, f)
#define J(f) offsetof(SvtHipObmcJob, f)
#define S(f) offsetof(SvtHipObmcSearchDesc, f)
#define Q(f) offsetof(SvtHipObmcSearchJob, f)
#define R(f) offsetof(SvtHipObmcSearchResult, f)
    static const size_t nbd[] = {N(bit_depth), N(ss_x), N(ss_y), N(plane), N(n_refs), N(reserved), N(n_jobs), N(n_blocks), N(refs), N(blocks), N(jobs), N(above),
                                 N(left), N(strip_samples), N(mv_array), N(n_mvs), N(reserved2), N(status)};
    static const size_t bld[] = {B(bit_depth), B(ss_x), B(ss_y), B(plane), B(n_jobs), B(n_blocks), B(dst_stride), B(blocks), B(jobs), B(above), B(left),
                                 B(strip_samples), B(dst), B(dst_samples), B(status)};
    static const size_t tgd[] = {T(strip_bit_depth), T(reserved), T(n_jobs), T(n_blocks), T(src_stride), T(blocks), T(jobs), T(above), T(left), T(strip_samples),
                                 T(src), T(src_samples), T(wsrc), T(mask), T(out_values), T(status)};
    static const size_t blk[] = {K(org_x), K(org_y), K(width), K(height), K(n_above), K(n_left), K(mb_to_left_edge), K(mb_to_right_edge), K(mb_to_top_edge),
                                 K(mb_to_bottom_edge), K(strip_offset), K(reserved), K(above), K(left)};
    static const size_t nbr[] = {H(rel_pos), H(size), H(ref), H(filter_x), H(filter_y), H(flags), H(mv), H(reserved), H(mv_index)};
    static const size_t job[] = {J(block), J(offset)};
    static const size_t sed[] = {S(ref_bit_depth), S(refine_level), S(fpel_search_diag), S(approx_inter_rate), S(allow_hp), S(reserved), S(n_jobs), S(fpel_search_range),
                                 S(sadpb), S(error_per_bit), S(ref_stride), S(reserved2), S(ref), S(ref_samples), S(wsrc), S(mask), S(target_values), S(mvjcost),
                                 S(mvcost), S(jobs), S(best_mv), S(results), S(status)};
    static const size_t sej[] = {Q(target_offset), Q(ref_offset), Q(width), Q(height), Q(reserved), Q(start_mv), Q(ref_mv), Q(col_min), Q(col_max), Q(row_min),
                                 Q(row_max), Q(reserved2)};
    static const size_t ser[] = {R(fullpel_value), R(besterr), R(distortion), R(sse1), R(rate_mv), R(reserved)};
#undef S
#undef Q
#undef R
#undef N
#undef B
#undef T
#undef K
#undef H
#undef J
    const SvtHipLayoutRow rows[] = {layout_row<SvtHipObmcNeighbourDesc>(nbd), layout_row<SvtHipObmcBlendDesc>(bld),  layout_row<SvtHipObmcTargetDesc>(tgd),
                                    layout_row<SvtHipObmcBlock>(blk),         layout_row<SvtHipObmcNeighbour>(nbr),  layout_row<SvtHipObmcJob>(job),
                                    layout_row<SvtHipObmcSearchDesc>(sed),    layout_row<SvtHipObmcSearchJob>(sej),  layout_row<SvtHipObmcSearchResult>(ser)};
    return layout_lookup(rows, what, field);
}

const uint8_t *svt_hip_obmc_masks(void) { return h_obmc_mask; }

int svt_hip_obmc_neighbour_batch(SvtHipContext *ctx, const SvtHipObmcNeighbourDesc *d) {
    return enqueue_batch("svt_hip_obmc_neighbour_batch", ctx, d, svt_hip_obmc_neighbour_check_desc, &SvtHipObmcNeighbourDesc::n_jobs, [=] {
        hipLaunchKernelGGL(pick_hbd(d->bit_depth, obmc_neighbour_kernel<true>, obmc_neighbour_kernel<false>), dim3(ceil_div(d->n_jobs, kWaves)), dim3(64 * kWaves), 0,
                           ctx->stream, *d);
    });
}

int svt_hip_obmc_blend_batch(SvtHipContext *ctx, const SvtHipObmcBlendDesc *d) {
    return enqueue_batch("svt_hip_obmc_blend_batch", ctx, d, svt_hip_obmc_blend_check_desc, &SvtHipObmcBlendDesc::n_jobs, [=] {
        hipLaunchKernelGGL(pick_hbd(d->bit_depth, obmc_blend_kernel<true>, obmc_blend_kernel<false>), dim3(ceil_div(d->n_jobs, kWaves)), dim3(64 * kWaves), 0,
                           ctx->stream, *d);
    });
}

int svt_hip_obmc_target_batch(SvtHipContext *ctx, const SvtHipObmcTargetDesc *d) {
    return enqueue_batch("svt_hip_obmc_target_batch", ctx, d, svt_hip_obmc_target_check_desc, &SvtHipObmcTargetDesc::n_jobs, [=] {
        hipLaunchKernelGGL(pick_hbd(d->strip_bit_depth, obmc_target_kernel<true>, obmc_target_kernel<false>), dim3(ceil_div(d->n_jobs, kWaves)), dim3(64 * kWaves), 0,
                           ctx->stream, *d);
    });
}

int svt_hip_obmc_search_batch(SvtHipContext *ctx, const SvtHipObmcSearchDesc *d) {
    return enqueue_batch("svt_hip_obmc_search_batch", ctx, d, svt_hip_obmc_search_check_desc, &SvtHipObmcSearchDesc::n_jobs,
                         [=] { hipLaunchKernelGGL(obmc_search_kernel, dim3(d->n_jobs), dim3(64), 0, ctx->stream, *d); });
}

} // extern "C"
