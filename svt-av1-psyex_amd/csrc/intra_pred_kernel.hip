// intra_pred_kernel.hip -- intra prediction (all modes, the edge filters, filter-intra) on gfx950: svt_hip_intra_pred_batch, which writes an
// intra candidate's prediction into the plane svt_hip_rd_batch reads.
//
// Reference functions restated (Source/Lib):
//   build_intra_predictors, build_intra_predictors_high                                   Codec/enc_intra_prediction.c:60-436
//   extend_modes, mode_to_angle_map, eb_dr_intra_derivative, sm_weight_arrays             Codec/intra_prediction.c:26-45,245-277,469-483, intra_prediction.h:65-79
//   svt_aom_use_intra_edge_upsample, svt_aom_intra_edge_filter_strength                   Codec/intra_prediction.c:146-152,180-243
//   svt_av1_filter_intra_edge_c / _high_c, filter_intra_edge_corner / _high               Codec/intra_prediction.c:156-178,2293-2300,2393-2422
//   svt_av1_upsample_intra_edge_c / _high_c, svt_av1_highbd_dr_prediction_z3_c            C_DEFAULT/intra_prediction_c.c
//   svt_av1_dr_prediction_z1_c / _z2_c / _z3_c, the highbd forms, svt_aom_dr_predictor    Codec/intra_prediction.c:314-413,2273-2391
//   dc_128 / dc_left / dc_top / dc, v, h, smooth, smooth_v, smooth_h, paeth and highbd    Codec/intra_prediction.c:1023-1348
//   svt_av1_filter_intra_predictor_c, svt_aom_highbd_filter_intra_predictor               C_DEFAULT/filterintra_c.c, Codec/intra_prediction.c:2474-2515
//
// Lay-out: one wave per job, four jobs per workgroup, no workgroup barrier.  The two edges live in the wave's LDS slice as uint16, the corner
// at index -1, room for the upsampled index -2 in front and 128 samples behind.  They are built by all lanes at once: load (the index clamped
// to the last available sample, which is the replication), fallback values, corner, corner filter, edge filter and upsampling -- the last
// two read every input into registers before any lane writes, which is the reference's copy.  Mode, zone, strengths, dx / dy and the upsample
// flags are the same for the whole wave: they are scalar, and the branches on them are per job, never per lane.  The wave then walks the
// block one quad (four horizontally adjacent samples) per lane and step.  The DC sum is one DPP reduction.  Filter-intra walks the
// anti-diagonals of 4x2 sub-blocks through a (bh + 1) x (bw + 1) LDS tile, eight lanes per sub-block: sub-block (R, C) reads only (R - 1, C - 1),
// (R - 1, C) and (R, C - 1), so those of one R + C are independent.  Stores are plain vector stores: 4 (8-bit) or 8 (10-bit) bytes per lane
// where the address allows, single samples otherwise.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include "batch_host.h"
#include "../../include/svt_hip_intra.h"
#include "wave_ops.h"

namespace {

constexpr int kWaves = 4;
constexpr int kOff   = 16;             // of index 0 in an edge
constexpr int kEdge  = kOff + 128 + 16; // samples an edge holds
constexpr int kPitch = 34;             // of the filter-intra tile: 33 columns used
constexpr int kTile  = 33 * kPitch;

enum Kind { K_FILL, K_V, K_H, K_SMOOTH, K_SMOOTH_V, K_SMOOTH_H, K_PAETH, K_Z1, K_Z2, K_Z3, K_TILE };

__constant__ uint8_t c_txw[19] = {4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64}; // tx_size_wide
__constant__ uint8_t c_txh[19] = {4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16}; // tx_size_high
__constant__ uint8_t c_mode_angle[13] = {0, 90, 180, 45, 135, 113, 157, 203, 67, 0, 0, 0, 0};           // mode_to_angle_map
__constant__ uint8_t c_sm[128] = { // sm_weight_arrays
    0, 0, 255, 128, 255, 149, 85, 64, 255, 197, 146, 105, 73, 50, 37, 32,
    255, 225, 196, 170, 145, 123, 102, 84, 68, 54, 43, 33, 26, 20, 17, 16,
    255, 240, 225, 210, 196, 182, 169, 157, 145, 133, 122, 111, 101, 92, 83, 74, 66, 59, 52, 45, 39, 34, 29, 25, 21, 17, 14, 12, 10, 9, 8, 8,
    255, 248, 240, 233, 225, 218, 210, 203, 196, 189, 182, 176, 169, 163, 156, 150, 144, 138, 133, 127, 121, 116, 111, 106, 101, 96, 91, 86, 82, 77, 73, 69,
    65, 61, 57, 54, 50, 47, 44, 41, 38, 35, 32, 29, 27, 25, 22, 20, 18, 16, 15, 13, 12, 10, 9, 8, 7, 6, 6, 5, 5, 4, 4, 4};
__constant__ uint16_t c_deriv[90] = { // eb_dr_intra_derivative
    0, 0, 0, 1023, 0, 0, 547, 0, 0, 372, 0, 0, 0, 0, 273, 0, 0, 215, 0, 0, 178, 0, 0, 151, 0, 0, 132, 0, 0, 116, 0, 0, 102, 0, 0, 0, 90, 0, 0, 80, 0, 0, 71, 0, 0,
    64, 0, 0, 57, 0, 0, 51, 0, 0, 45, 0, 0, 0, 40, 0, 0, 35, 0, 0, 31, 0, 0, 27, 0, 0, 23, 0, 0, 19, 0, 0, 15, 0, 0, 0, 0, 11, 0, 0, 7, 0, 0, 3, 0, 0};
__constant__ int8_t c_fi_taps[5][8][8] = { // eb_av1_filter_intra_taps
    {{-6, 10, 0, 0, 0, 12, 0, 0}, {-5, 2, 10, 0, 0, 9, 0, 0}, {-3, 1, 1, 10, 0, 7, 0, 0}, {-3, 1, 1, 2, 10, 5, 0, 0},
     {-4, 6, 0, 0, 0, 2, 12, 0}, {-3, 2, 6, 0, 0, 2, 9, 0}, {-3, 2, 2, 6, 0, 2, 7, 0}, {-3, 1, 2, 2, 6, 3, 5, 0}},
    {{-10, 16, 0, 0, 0, 10, 0, 0}, {-6, 0, 16, 0, 0, 6, 0, 0}, {-4, 0, 0, 16, 0, 4, 0, 0}, {-2, 0, 0, 0, 16, 2, 0, 0},
     {-10, 16, 0, 0, 0, 0, 10, 0}, {-6, 0, 16, 0, 0, 0, 6, 0}, {-4, 0, 0, 16, 0, 0, 4, 0}, {-2, 0, 0, 0, 16, 0, 2, 0}},
    {{-8, 8, 0, 0, 0, 16, 0, 0}, {-8, 0, 8, 0, 0, 16, 0, 0}, {-8, 0, 0, 8, 0, 16, 0, 0}, {-8, 0, 0, 0, 8, 16, 0, 0},
     {-4, 4, 0, 0, 0, 0, 16, 0}, {-4, 0, 4, 0, 0, 0, 16, 0}, {-4, 0, 0, 4, 0, 0, 16, 0}, {-4, 0, 0, 0, 4, 0, 16, 0}},
    {{-2, 8, 0, 0, 0, 10, 0, 0}, {-1, 3, 8, 0, 0, 6, 0, 0}, {-1, 2, 3, 8, 0, 4, 0, 0}, {0, 1, 2, 3, 8, 2, 0, 0},
     {-1, 4, 0, 0, 0, 3, 10, 0}, {-1, 3, 4, 0, 0, 4, 6, 0}, {-1, 2, 3, 4, 0, 4, 4, 0}, {-1, 2, 2, 3, 4, 3, 3, 0}},
    {{-12, 14, 0, 0, 0, 14, 0, 0}, {-10, 0, 14, 0, 0, 12, 0, 0}, {-9, 0, 0, 14, 0, 11, 0, 0}, {-8, 0, 0, 0, 14, 10, 0, 0},
     {-10, 12, 0, 0, 0, 0, 14, 0}, {-9, 1, 12, 0, 0, 0, 12, 0}, {-8, 0, 0, 12, 0, 1, 11, 0}, {-7, 0, 0, 1, 12, 1, 9, 0}}};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// svt_aom_intra_edge_filter_strength
__device__ __forceinline__ int edge_strength(int bs0, int bs1, int delta, int type) {
    const int d = delta < 0 ? -delta : delta, wh = bs0 + bs1;
    int s = 0;
    if (type == 0) {
        if (wh <= 8) s = d >= 56 ? 1 : 0;
        else if (wh <= 16) s = d >= 40 ? 1 : 0;
        else if (wh <= 24) s = d >= 32 ? 3 : (d >= 16 ? 2 : (d >= 8 ? 1 : 0));
        else if (wh <= 32) s = d >= 32 ? 3 : (d >= 4 ? 2 : (d >= 1 ? 1 : 0));
        else s = d >= 1 ? 3 : 0;
    } else {
        if (wh <= 8) s = d >= 64 ? 2 : (d >= 40 ? 1 : 0);
        else if (wh <= 16) s = d >= 48 ? 2 : (d >= 20 ? 1 : 0);
        else if (wh <= 24) s = d >= 4 ? 3 : 0;
        else s = d >= 1 ? 3 : 0;
    }
    return s;
}
// svt_aom_use_intra_edge_upsample
__device__ __forceinline__ int use_upsample(int bs0, int bs1, int delta, int type) {
    const int d = delta < 0 ? -delta : delta;
    if (d <= 0 || d >= 40) return 0;
    return type ? (bs0 + bs1 <= 8) : (bs0 + bs1 <= 16);
}

// svt_av1_filter_intra_edge: p[1 .. n - 1] from p[0 .. n - 1], n <= 129; every lane reads its inputs before any lane writes
__device__ __forceinline__ void edge_filter(uint16_t *p, int n, int strength, int lane) {
    if (!strength) return;
    const int k0 = strength == 3 ? 2 : 0, k1 = strength == 2 ? 5 : 4, k2 = strength == 1 ? 8 : (strength == 2 ? 6 : 4); // {k0, k1, k2, k1, k0}
    int res[3] = {0, 0, 0};
#pragma unroll
    for (int t = 0; t < 3; t++) {
        const int i = lane + 64 * t;
        if (i >= 1 && i < n) {
            const int a = p[i - 2 < 0 ? 0 : i - 2], b = p[i - 1], c = p[i], e = p[i + 1 > n - 1 ? n - 1 : i + 1], f = p[i + 2 > n - 1 ? n - 1 : i + 2];
            res[t] = (k0 * (a + f) + k1 * (b + e) + k2 * c + 8) >> 4;
        }
    }
    wave_sync();
#pragma unroll
    for (int t = 0; t < 3; t++) {
        const int i = lane + 64 * t;
        if (i >= 1 && i < n) p[i] = (uint16_t)res[t];
    }
    wave_sync();
}

// svt_av1_upsample_intra_edge: p[-2 .. 2n - 2] from p[-1 .. n - 1], n <= 16
__device__ __forceinline__ void edge_upsample(uint16_t *p, int n, int px_max, int lane) {
    int s = 0, mid = 0, first = 0;
    if (lane < n) {
        const int a = p[lane - 2 < -1 ? -1 : lane - 2], b = p[lane - 1], e = p[lane + 1 > n - 1 ? n - 1 : lane + 1];
        mid   = p[lane];
        first = p[-1];
        s     = clampi((-a + 9 * b + 9 * mid - e + 8) >> 4, 0, px_max);
    }
    wave_sync();
    if (lane < n) {
        p[2 * lane - 1] = (uint16_t)s;
        p[2 * lane]     = (uint16_t)mid;
        if (lane == 0) p[-2] = (uint16_t)first;
    }
    wave_sync();
}

// paeth_predictor_single
__device__ __forceinline__ int paeth(int left, int top, int tl) {
    const int base = top + left - tl;
    const int pl = base > left ? base - left : left - base, pt = base > top ? base - top : top - base, ptl = base > tl ? base - tl : tl - base;
    return (pl <= pt && pl <= ptl) ? left : (pt <= ptl ? top : tl);
}

template <bool HBD> __global__ __launch_bounds__(64 * kWaves) void intra_pred_kernel(const SvtHipIntraPredDesc d) {
    using Px = typename std::conditional<HBD, uint16_t, uint8_t>::type;
    __shared__ __attribute__((aligned(16))) uint16_t s_edge[kWaves][2 * kEdge];
    __shared__ __attribute__((aligned(16))) uint16_t s_tile[kWaves][kTile];
    constexpr int bd = HBD ? 10 : 8, px_max = (1 << bd) - 1, base = 128 << (bd - 8);
    const int      lane = (int)(threadIdx.x & 63u);
    const int      wave = uniform((int)(threadIdx.x >> 6));
    const uint32_t job  = blockIdx.x * (uint32_t)kWaves + (uint32_t)wave;
    if (job >= d.n_jobs) return;
    const SvtHipIntraPredJob j = d.jobs[job];

    bool       ok = j.tx_size <= 18 && j.mode <= 12 && j.filter_intra_mode <= SVT_HIP_INTRA_PRED_NO_FILTER_INTRA;
    const int  tx = ok ? j.tx_size : 0, mode = ok ? j.mode : 0;
    const int  w = c_txw[tx], h = c_txh[tx];
    const bool is_dr = mode >= 1 && mode <= 8, use_fi = j.filter_intra_mode != SVT_HIP_INTRA_PRED_NO_FILTER_INTRA;
    const int  nt = j.n_top_px, ntr = j.n_topright_px, nl = j.n_left_px, nbl = j.n_bottomleft_px;
    if (is_dr) ok = ok && j.angle_delta >= -3 && j.angle_delta <= 3;
    if (use_fi) ok = ok && w <= 32 && h <= 32 && mode == 0;
    ok = ok && nt <= w && ntr <= w && (ntr == 0 || nt == w) && nl <= h && nbl <= h && (nbl == 0 || nl == h);

    // the needed edges: extend_modes[] for DC / SMOOTH* / PAETH, p_angle's zone for a directional mode, all three for filter-intra
    int  p_angle = 0;
    bool need_above = true, need_left = true, need_al = mode == 12 || use_fi, need_right = false, need_bottom = false;
    if (is_dr) {
        p_angle    = (int)c_mode_angle[mode] + 3 * (int)j.angle_delta;
        need_above = p_angle < 180; need_left = p_angle > 90; need_al = true;
        need_right = p_angle < 90; need_bottom = p_angle > 180;
    }
    const bool early = (!need_above && nl == 0) || (!need_left && nt == 0);
    // the reference's reads: a_n samples of the row above, l_n of the column on the left, the corner
    int  a_n, l_n;
    bool corner = false;
    if (early) {
        a_n = (need_left && nt > 0) ? 1 : 0;
        l_n = (!need_left && nl > 0) ? 1 : 0;
    } else {
        a_n    = (need_above && nt > 0) ? nt + (need_right ? ntr : 0) : 0;
        l_n    = (need_left && nl > 0) ? nl + (need_bottom ? nbl : 0) : 0;
        corner = need_al && nt > 0 && nl > 0;
    }
    {
        const long long x0 = j.nbr_x, y0 = j.nbr_y, W = d.nbr_width, H = d.nbr_height;
        if (a_n > 0) ok = ok && y0 >= 1 && y0 - 1 < H && x0 >= 0 && x0 + a_n <= W;
        if (l_n > 0) ok = ok && x0 >= 1 && x0 - 1 < W && y0 >= 0 && y0 + l_n <= H;
        if (corner) ok = ok && x0 >= 1 && y0 >= 1 && x0 - 1 < W && y0 - 1 < H;
    }
    ok = ok && (uint64_t)j.dst_offset + (uint64_t)(h - 1) * d.dst_stride + (uint64_t)w <= d.dst_samples;
    if (!ok) {
        if (lane == 0) d.status[job] = SVT_HIP_INTRA_PRED_UNDEFINED;
        return;
    }

    const Px *const nbr    = (const Px *)d.nbr;
    const ptrdiff_t stride = (ptrdiff_t)d.nbr_stride;
    const Px *const above_ref = nbr + ((ptrdiff_t)j.nbr_y - 1) * stride + j.nbr_x; // dereferenced inside the checked ranges alone
    const Px *const left_ref  = nbr + (ptrdiff_t)j.nbr_y * stride + j.nbr_x - 1;
    uint16_t *const E = s_edge[wave];
    uint16_t *const A = E + kOff, *const L = E + kEdge + kOff;
    uint16_t *const T = s_tile[wave];

    int kind = K_FILL, fillv = 0, dx = 1, dy = 1, upa = 0, upl = 0;
    if (early) {
        if (need_left) fillv = nt > 0 ? (int)above_ref[0] : base + 1;
        else fillv = nl > 0 ? (int)left_ref[0] : base - 1;
    } else {
        const int need_a = need_above ? w + (need_right ? h : 0) : 0, need_l = need_left ? h + (need_bottom ? w : 0) : 0;
        // what is available, the index clamped to the last of it: the replication
        if (a_n > 0)
            for (int i = lane; i < need_a; i += 64) A[i] = (uint16_t)above_ref[i < a_n ? i : a_n - 1];
        if (l_n > 0)
            for (int i = lane; i < need_l; i += 64) L[i] = (uint16_t)left_ref[(ptrdiff_t)(i < l_n ? i : l_n - 1) * stride];
        wave_sync();
        if (need_above && nt == 0) {
            const int v = nl > 0 ? (int)L[0] : base - 1;
            for (int i = lane; i < need_a; i += 64) A[i] = (uint16_t)v;
        }
        if (need_left && nl == 0) {
            const int v = nt > 0 ? (int)A[0] : base + 1;
            for (int i = lane; i < need_l; i += 64) L[i] = (uint16_t)v;
        }
        wave_sync();
        if (need_al) {
            const int cv = corner ? (int)above_ref[-1] : (nt > 0 ? (int)A[0] : (nl > 0 ? (int)L[0] : base));
            if (lane == 0) { A[-1] = (uint16_t)cv; L[-1] = (uint16_t)cv; }
            wave_sync();
        }

        if (use_fi) {
            kind = K_TILE;
            for (int i = lane; i <= w; i += 64) T[i] = A[i - 1];
            for (int i = lane; i < h; i += 64) T[(i + 1) * kPitch] = L[i];
            wave_sync();
            const int nC = w >> 2, nR = h >> 1, sub = lane >> 3, k = lane & 7;
            int tap[7];
#pragma unroll
            for (int t = 0; t < 7; t++) tap[t] = c_fi_taps[j.filter_intra_mode][k][t];
            for (int dg = 0; dg < nR + nC - 1; dg++) { // the sub-blocks (R, C) with R + C = dg
                const int  cmin = dg - (nR - 1) > 0 ? dg - (nR - 1) : 0, cmax = dg < nC - 1 ? dg : nC - 1;
                const int  C = cmin + sub, r = 1 + 2 * (dg - C), c = 1 + 4 * C;
                const bool act = C <= cmax;
                int        v = 0;
                if (act) {
                    const uint16_t *up = T + (r - 1) * kPitch + c - 1;
                    const int sum = tap[0] * up[0] + tap[1] * up[1] + tap[2] * up[2] + tap[3] * up[3] + tap[4] * up[4] + tap[5] * up[kPitch] + tap[6] * up[2 * kPitch];
                    v = clampi(sum < 0 ? -((-sum + 8) >> 4) : (sum + 8) >> 4, 0, px_max); // ROUND_POWER_OF_TWO_SIGNED(sum, 4)
                }
                wave_sync();
                if (act) T[(r + (k >> 2)) * kPitch + c + (k & 3)] = (uint16_t)v;
                wave_sync();
            }
        } else if (is_dr) {
            if (!d.disable_edge_filter) {
                const int ft = j.filt_type != 0;
                if (p_angle != 90 && p_angle != 180) {
                    if (need_above && need_left && w + h >= 24) { // filter_intra_edge_corner
                        const int cv = (5 * (int)L[0] + 6 * (int)A[-1] + 5 * (int)A[0] + 8) >> 4;
                        wave_sync();
                        if (lane == 0) { A[-1] = (uint16_t)cv; L[-1] = (uint16_t)cv; }
                        wave_sync();
                    }
                    if (need_above && nt > 0) edge_filter(A - 1, nt + 1 + (need_right ? h : 0), edge_strength(w, h, p_angle - 90, ft), lane);
                    if (need_left && nl > 0) edge_filter(L - 1, nl + 1 + (need_bottom ? w : 0), edge_strength(h, w, p_angle - 180, ft), lane);
                }
                upa = use_upsample(w, h, p_angle - 90, ft);
                if (need_above && upa) edge_upsample(A, need_a, px_max, lane);
                upl = use_upsample(h, w, p_angle - 180, ft);
                if (need_left && upl) edge_upsample(L, need_l, px_max, lane);
            }
            if (p_angle == 90) kind = K_V;
            else if (p_angle == 180) kind = K_H;
            else if (p_angle < 90) { kind = K_Z1; dx = c_deriv[p_angle]; }
            else if (p_angle < 180) { kind = K_Z2; dx = c_deriv[180 - p_angle]; dy = c_deriv[p_angle - 90]; }
            else { kind = K_Z3; dy = c_deriv[270 - p_angle]; }
        } else if (mode == 0) { // svt_aom_dc_pred[n_left_px > 0][n_top_px > 0]
            if (nt == 0 && nl == 0) fillv = base;
            else {
                const uint32_t v = ((nt > 0 && lane < w) ? (uint32_t)A[lane] : 0u) + ((nl > 0 && lane < h) ? (uint32_t)L[lane] : 0u);
                const uint32_t sum = wave_sum_dpp(v), count = (uint32_t)((nt > 0 ? w : 0) + (nl > 0 ? h : 0));
                fillv = (int)((sum + (count >> 1)) / count);
            }
        } else
            kind = mode == 9 ? K_SMOOTH : (mode == 10 ? K_SMOOTH_V : (mode == 11 ? K_SMOOTH_H : K_PAETH));
    }

    const int qsh = w == 4 ? 0 : (w == 8 ? 1 : (w == 16 ? 2 : (w == 32 ? 3 : 4))), nq = (w * h) >> 2;
    const int below = L[h - 1], right = A[w - 1], tl = A[-1]; // SMOOTH* / PAETH read them; harmless LDS reads otherwise
    Px *const dst = (Px *)d.dst + (size_t)j.dst_offset;
    for (int q = lane; q < nq; q += 64) {
        const int r = q >> qsh, c = (q & ((w >> 2) - 1)) << 2;
        int out[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int cc = c + i;
            int v;
            switch (kind) {
            case K_FILL: v = fillv; break;
            case K_V: v = A[cc]; break;
            case K_H: v = L[r]; break;
            case K_SMOOTH: {
                const int wh = c_sm[h + r], ww = c_sm[w + cc];
                v = (wh * (int)A[cc] + (256 - wh) * below + ww * (int)L[r] + (256 - ww) * right + 256) >> 9;
            } break;
            case K_SMOOTH_V: {
                const int wh = c_sm[h + r];
                v = (wh * (int)A[cc] + (256 - wh) * below + 128) >> 8;
            } break;
            case K_SMOOTH_H: {
                const int ww = c_sm[w + cc];
                v = (ww * (int)L[r] + (256 - ww) * right + 128) >> 8;
            } break;
            case K_PAETH: v = paeth(L[r], A[cc], tl); break;
            case K_TILE: v = T[(r + 1) * kPitch + 1 + cc]; break;
            default: { // the three zones: an index into E (A or L), a shift, or the fill past max_base
                int at, shift;
                bool past = false;
                if (kind == K_Z1) {
                    const int x = (r + 1) * dx, b = (x >> (6 - upa)) + (cc << upa), maxb = (w + h - 1) << upa;
                    past = b >= maxb; at = kOff + (past ? maxb : b); shift = ((x << upa) & 0x3F) >> 1;
                } else if (kind == K_Z3) {
                    const int y = (cc + 1) * dy, b = (y >> (6 - upl)) + (r << upl), maxb = (w + h - 1) << upl;
                    past = b >= maxb; at = kEdge + kOff + (past ? maxb : b); shift = ((y << upl) & 0x3F) >> 1;
                } else {
                    const int x = (cc << 6) - (r + 1) * dx, bx = x >> (6 - upa);
                    if (bx >= -(1 << upa)) { at = kOff + bx; shift = ((x * (1 << upa)) & 0x3F) >> 1; }
                    else {
                        const int y = (r << 6) - (cc + 1) * dy;
                        at = kEdge + kOff + (y >> (6 - upl)); shift = ((y * (1 << upl)) & 0x3F) >> 1;
                    }
                }
                v = past ? (int)E[at] : clampi(((int)E[at] * (32 - shift) + (int)E[at + 1] * shift + 16) >> 5, 0, px_max);
            } break;
            }
            out[i] = v;
        }
        Px *p = dst + (size_t)r * d.dst_stride + (size_t)c;
        if (HBD) {
            if (((uintptr_t)p & 7u) == 0) *(uint2 *)p = make_uint2((uint32_t)out[0] | ((uint32_t)out[1] << 16), (uint32_t)out[2] | ((uint32_t)out[3] << 16));
            else { p[0] = (Px)out[0]; p[1] = (Px)out[1]; p[2] = (Px)out[2]; p[3] = (Px)out[3]; }
        } else {
            if (((uintptr_t)p & 3u) == 0) *(uint32_t *)p = (uint32_t)out[0] | ((uint32_t)out[1] << 8) | ((uint32_t)out[2] << 16) | ((uint32_t)out[3] << 24);
            else { p[0] = (Px)out[0]; p[1] = (Px)out[1]; p[2] = (Px)out[2]; p[3] = (Px)out[3]; }
        }
    }
    if (lane == 0) d.status[job] = SVT_HIP_INTRA_PRED_OK;
}

} // namespace

extern "C" {

int svt_hip_intra_pred_check_desc(const SvtHipIntraPredDesc *d) {
    if (!d) BAD("svt_hip_intra_pred_check_desc: null descriptor");
    if (!d->nbr || !d->dst || !d->jobs || !d->status) BAD("svt_hip_intra_pred_check_desc: a mandatory pointer (nbr, dst, jobs, status) is null");
    if (d->bit_depth != 8 && d->bit_depth != 10) BAD("svt_hip_intra_pred_check_desc: bit_depth %u (8 or 10)", d->bit_depth);
    if (d->nbr_stride == 0 || d->nbr_width == 0 || d->nbr_height == 0 || d->nbr_stride < d->nbr_width)
        BAD("svt_hip_intra_pred_check_desc: neighbour plane stride %u, size %u x %u (stride and size non-zero, stride >= width)", d->nbr_stride, d->nbr_width,
            d->nbr_height);
    if (d->dst_stride == 0 || d->dst_samples == 0)
        BAD("svt_hip_intra_pred_check_desc: dst_stride %u / dst_samples %llu is zero", d->dst_stride, (unsigned long long)d->dst_samples);
    const uint64_t px = d->bit_depth > 8 ? 2 : 1;
    const uint64_t n0 = (uint64_t)(uintptr_t)d->nbr, n1 = n0 + ((uint64_t)(d->nbr_height - 1) * d->nbr_stride + d->nbr_width) * px;
    const uint64_t d0 = (uint64_t)(uintptr_t)d->dst, d1 = d0 + d->dst_samples * px;
    if (d0 < n1 && n0 < d1) BAD("svt_hip_intra_pred_check_desc: the destination range overlaps the neighbour plane (a batch must not read what it writes)");
    return SVT_HIP_OK;
}

size_t svt_hip_intra_pred_layout(int what, int field) {
#define D(f) offsetof(SvtHipIntraPredDesc, f)
#define J(f) offsetof(SvtHipIntraPredJob, f)
    static const size_t desc[] = {D(bit_depth), D(disable_edge_filter), D(reserved), D(n_jobs), D(nbr), D(nbr_stride), D(nbr_width), D(nbr_height), D(reserved2),
                                  D(dst), D(dst_stride), D(reserved3), D(dst_samples), D(jobs), D(status)};
    static const size_t job[]  = {J(dst_offset), J(nbr_x), J(nbr_y), J(tx_size), J(mode), J(angle_delta), J(filter_intra_mode), J(n_top_px), J(n_topright_px),
                                  J(n_left_px), J(n_bottomleft_px), J(filt_type), J(reserved)};
#undef D
#undef J
    const SvtHipLayoutRow rows[] = {layout_row<SvtHipIntraPredDesc>(desc), layout_row<SvtHipIntraPredJob>(job)};
    return layout_lookup(rows, what, field);
}

int svt_hip_intra_pred_batch(SvtHipContext *ctx, const SvtHipIntraPredDesc *d) {
    return enqueue_batch("svt_hip_intra_pred_batch", ctx, d, svt_hip_intra_pred_check_desc, &SvtHipIntraPredDesc::n_jobs, [=] {
        hipLaunchKernelGGL(pick_hbd(d->bit_depth, intra_pred_kernel<true>, intra_pred_kernel<false>), dim3(ceil_div(d->n_jobs, kWaves)), dim3(64 * kWaves), 0,
                           ctx->stream, *d);
    });
}

} // extern "C"
