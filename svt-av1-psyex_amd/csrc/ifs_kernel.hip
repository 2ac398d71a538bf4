// ifs_kernel.hip -- the interpolation-filter search on gfx950: svt_hip_ifs_batch, the step between the motion searches' MVs and the final
// prediction of an inter candidate, and svt_hip_ifs_scatter_filters, which hands the chosen filters to the prediction batches' job records.
//
// Reference functions restated (Source/Lib):
//   interpolation_filter_search, filter_sets                                            Codec/enc_inter_prediction.c:2424-2577
//   svt_av1_get_switchable_rate                                                         Codec/enc_inter_prediction.c:2146-2165
//   model_rd_for_sb (plane 0), model_rd_from_sse, svt_av1_model_rd_from_var_lapndz, model_rd_norm   Codec/enc_inter_prediction.c:2167-2388
//   svt_psy_distortion / _hbd, get_svt_psy_full_dist                                    Codec/psy_rd.c:135-293 (psy_energy.h)
//   RDCOST                                                                              Codec/rd_cost.h:37-39
//   av1_make_interp_filters, av1_extract_interp_filter                                  Codec/filter.h:59-67
//   the luma prediction of a pair: everything inter_pred_kernel.hip restates, through convolve_core.h
//
// Lay-out: one wave per job, four jobs per workgroup, no workgroup barrier.  The wave walks the block in the tiles of tile_walk (up to 64
// quads, one per lane).  Per tile:
//   1  each reference's source window is staged once in the wave's LDS (tile + 7 in each direction its MV has a phase in); a reference
//      with no phase at all is read straight from the plane, once
//   2  per x filter (three, or one when no reference has an x phase) the horizontal pass of each 2-D reference runs once into that
//      reference's intermediate; per y filter on it (three, or one when no reference has a y phase) the vertical pass runs per reference
//      and a compound is combined in registers.  A pair whose filters differ from another's only in a direction without a phase is that
//      other pair's prediction and is not computed: `need` holds the distinct ones, at most nine
//   3  every distinct prediction of the tile goes to a slot of the wave's LDS (never to memory); the source tile goes to a tenth slot
//   4  SSE: a lane squares its own quad of every slot against its source quad, into one 32-bit sum per slot (registers)
//      psy: lane (slot, psy tile) computes the energy of one 8x8 / 4x4 tile of one slot, the source's slot included, so the source
//      energies are computed once per tile and all slots' energies in one pass of psy_tile_energy; |source - prediction| goes to the
//      lane's 64-bit sum
// After the last tile the sums are reduced, lanes 0..8 run the model and the cost of one pair each, and the first minimum is taken in the
// reference's order.  The winner's samples: a block of one tile still has them in its LDS slot and stores them; a larger block computes
// the winning pair once more tile by tile (one horizontal and one vertical pass per reference against the three and nine of the search)
// rather than keeping nine predictions of up to 128 x 128 samples.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include "batch_host.h"
#include "../../include/svt_hip_ifs.h"
#include "wave_ops.h"
#include "convolve_core.h"
#include "psy_energy.h"

#define IFS_RATE_TAB                                                                                                                         \
    {65536, 6086, 5574, 5275, 5063, 4899, 4764, 4651, 4553, 4389, 4255, 4142, 4044, 3958, 3881, 3811, 3748, 3635, 3538, 3453, 3376, 3307,    \
     3244,  3186, 3133, 3037, 2952, 2877, 2809, 2747, 2690, 2638, 2589, 2501, 2423, 2353, 2290, 2232, 2179, 2130, 2084, 2001, 1928, 1862,    \
     1802,  1748, 1698, 1651, 1608, 1530, 1460, 1398, 1342, 1290, 1243, 1199, 1159, 1086, 1021, 963,  911,  864,  821,  781,  745,  680,     \
     623,   574,  530,  490,  455,  424,  395,  345,  304,  269,  239,  213,  190,  171,  154,  126,  104,  87,   73,   61,   52,   44,      \
     38,    28,   21,   16,   12,   10,   8,    6,    5,    3,    2,    1,    1,    1,    0,    0}
#define IFS_DIST_TAB                                                                                                                         \
    {0,   0,   1,   1,   1,   2,   2,   2,   3,   3,   4,   5,   5,   6,   7,   7,   8,   9,   11,  12,  13,  15,  16,  17,   18,   21,      \
     24,  26,  29,  31,  34,  36,  39,  44,  49,  54,  59,  64,  69,  73,  78,  88,  97,  106, 115, 124, 133, 142, 151,  167,  184,  200,     \
     215, 231, 245, 260, 274, 301, 327, 351, 375, 397, 418, 439, 458, 495, 528, 559, 587, 613, 637, 659, 680, 717,  749,  777,  801,  823,   \
     842, 859, 874, 899, 919, 936, 949, 960, 969, 977, 983, 994, 1001, 1006, 1010, 1013, 1015, 1017, 1018, 1020, 1022, 1022, 1023, 1023,   \
     1023, 1024}
#define IFS_XSQ_TAB                                                                                                                          \
    {0,     4,     8,     12,    16,    20,    24,    28,    32,    40,    48,     56,     64,     72,     80,     88,     96,     112,      \
     128,   144,   160,   176,   192,   208,   224,   256,   288,   320,   352,    384,    416,    448,    480,    544,    608,    672,      \
     736,   800,   864,   928,   992,   1120,  1248,  1376,  1504,  1632,  1760,   1888,   2016,   2272,   2528,   2784,   3040,   3296,     \
     3552,  3808,  4064,  4576,  5088,  5600,  6112,  6624,  7136,  7648,  8160,   9184,   10208,  11232,  12256,  13280,  14304,  15328,    \
     16352, 18400, 20448, 22496, 24544, 26592, 28640, 30688, 32736, 36832, 40928,  45024,  49120,  53216,  57312,  61408,  65504,  73696,    \
     81888, 90080, 98272, 106464, 114656, 122848, 131040, 147424, 163808, 180192, 196576, 212960, 229344, 245728}

namespace {

constexpr int kWaves    = 4;
constexpr int kSlots    = SVT_HIP_IFS_PAIRS;  // one per distinct prediction; slot kSlots holds the source tile
constexpr int kTileSamples = 256;
constexpr int kN = SVT_HIP_IFS_MODEL_ENTRIES;

// model_rd_norm's tables: [0] rate_tab_q10, [1] dist_tab_q10, [2] xsq_iq_q10
__constant__ int32_t c_model[3][kN] = {IFS_RATE_TAB, IFS_DIST_TAB, IFS_XSQ_TAB};
const int32_t        h_model[3][kN] = {IFS_RATE_TAB, IFS_DIST_TAB, IFS_XSQ_TAB};

struct LumaPlane { int ss_x = 0, ss_y = 0; }; // what ref_view wants of a descriptor

// the wave's LDS: a window and an intermediate per reference, the prediction slots and the source tile
template <typename Px> struct WaveLds {
    uint16_t win[2][kWinU16];
    int16_t  mid[2][kMidU16];
    Px       pred[kSlots + 1][kTileSamples];
};

// model_rd_from_sse with simple_model_rd_from_var = 0, then the `dist <<= 4` of its caller's callee (:2223-2264)
__device__ __forceinline__ void model_rd(u64 sse, int n_log2, int qstep, int32_t *rate, u64 *dist) {
    const i64 var = (i64)sse;
    if (var == 0) { *rate = 0; *dist = 0; return; }
    const u64 xsq64 = ((((u64)(uint32_t)qstep * (u64)(uint32_t)qstep) << (n_log2 + 10)) + (u64)(var >> 1)) / (u64)var;
    const int32_t xsq = (int32_t)(xsq64 < 245727ull ? xsq64 : 245727ull); // MAX_XSQ_Q10
    const int32_t tmp = (xsq >> 2) + 8;
    const int32_t k   = (31 - __builtin_clz((uint32_t)tmp)) - 3; // get_msb
    const int32_t xq  = (k << 3) + ((tmp >> k) & 0x7);
    const int32_t a   = ((xsq - c_model[2][xq]) << 10) >> (2 + k);
    const int32_t b   = (1 << 10) - a;
    const int32_t r_q10 = (c_model[0][xq] * b + c_model[0][xq + 1] * a) >> 10;
    const int32_t d_q10 = (c_model[1][xq] * b + c_model[1][xq + 1] * a) >> 10;
    *rate = ((r_q10 << n_log2) + 1) >> 1; // ROUND_POWER_OF_TWO(., 10 - AV1_PROB_COST_SHIFT)
    *dist = (u64)((var * (i64)d_q10 + 512) >> 10) << 4;
}

// The distinct predictions in `need` (bit yf * 3 + xf) of the tile at (tx, ty), each into its slot of L.pred.  Wave-uniform but for the quad.
template <bool HBD>
__device__ __forceinline__ void tile_preds(WaveLds<typename std::conditional<HBD, uint16_t, uint8_t>::type> &L, const RefView &rv0, const RefView &rv1, int nrefs,
                                           const SvtHipInterPredJob &j, const TileWalk &t, int tx, int ty, uint32_t need, bool ux, bool uy, int lane) {
    using Px = typename std::conditional<HBD, uint16_t, uint8_t>::type;
    constexpr int bd = HBD ? 10 : 8, px_max = (1 << bd) - 1;
    constexpr int ro = (1 << (bd + 4)) + (1 << (bd + 3)); // compound round_offset: offset_bits = bd + 11, round_1 = 7
    const bool comp = nrefs == 2;
    const int  w = j.width, h = j.height, TW = t.TW, TH = t.TH, ws = TW + 8, qx = t.qx, qy = t.qy;
    int cp[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}; // a copy-variant reference's samples
    wave_sync(); // the previous reads of the windows, intermediates and slots are done
#pragma unroll
    for (int k = 0; k < 2; k++) {
        if (k < nrefs) {
            const RefView r = k ? rv1 : rv0;
            const int  bx = r.pos_x + tx, by = r.pos_y + ty;
            const bool fx = r.sx != 0, fy = r.sy != 0;
            if (!fx && !fy) {
                if (t.active)
#pragma unroll
                    for (int i = 0; i < 4; i++) cp[k][i] = sample<Px>(r, bx + qx + i, by + qy);
            } else
                stage<Px>(L.win[k], r, bx - (fx ? 3 : 0), by - (fy ? 3 : 0), TW + (fx ? 7 : 0), TH + (fy ? 7 : 0), ws, lane);
        }
    }
    wave_sync();
    const int nx = ux ? 3 : 1, ny = uy ? 3 : 1;
#pragma unroll 1
    for (int xf = 0; xf < nx; xf++) {
        if (!((need >> xf) & 0x49u)) continue; // no needed slot with this x filter
        const int tabx = filter_table(xf, w);
        wave_sync(); // the vertical passes of the previous x filter have read the intermediates
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const RefView r = k ? rv1 : rv0;
            if (k < nrefs && r.sx != 0 && r.sy != 0) { // the horizontal pass of *_2d_*: im_block, (TH + 7) rows
                int tx8[8];
#pragma unroll
                for (int i = 0; i < 8; i++) tx8[i] = c_interp[tabx][r.sx][i];
                const uint16_t *win = L.win[k];
                int16_t        *mid = L.mid[k];
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
                        for (int m = 0; m < 8; m++) sum += tx8[m] * in[i + m];
                        o[i] = (uint32_t)(uint16_t)(int16_t)((sum + 4) >> 3);
                    }
                    *(uint2 *)(mid + rr * TW + cc) = make_uint2(o[0] | (o[1] << 16), o[2] | (o[3] << 16));
                }
            }
        }
        wave_sync();
#pragma unroll 1
        for (int yf = 0; yf < ny; yf++) {
            const int slot = yf * 3 + xf;
            if (!((need >> slot) & 1u)) continue;
            const int taby = filter_table(yf, h);
            int acc[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < 2; k++) {
                if (k >= nrefs) continue;
                const RefView r = k ? rv1 : rv0;
                const bool fx = r.sx != 0, fy = r.sy != 0;
                const uint16_t *win = L.win[k];
                const int16_t  *mid = L.mid[k];
                int res[4] = {0, 0, 0, 0}; // single: the sample; compound: the function's `res`
                if (!fx && !fy) { // svt_av1_convolve_2d_copy_sr_c / svt_av1_jnt_convolve_2d_copy_c
#pragma unroll
                    for (int i = 0; i < 4; i++) res[i] = comp ? (int)(uint16_t)((uint16_t)(cp[k][i] << 4) + (uint16_t)ro) : cp[k][i];
                } else if (t.active) {
                    if (fx && fy) { // the vertical pass of *_2d_*
                        int sum[4];
#pragma unroll
                        for (int i = 0; i < 4; i++) sum[i] = 1 << (bd + 11);
#pragma unroll
                        for (int m = 0; m < 8; m++) {
                            int v[4];
                            load4s(mid + (qy + m) * TW + qx, v);
                            const int c = c_interp[taby][r.sy][m];
#pragma unroll
                            for (int i = 0; i < 4; i++) sum[i] += c * v[i];
                        }
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            if (comp) res[i] = (int)(uint16_t)((sum[i] + 64) >> 7);
                            else { // round_1 = 11, bits = 0; the 8-bit function holds res in an int16_t
                                const int v = ((sum[i] + 1024) >> 11) - ((1 << bd) + (1 << (bd - 1)));
                                res[i] = clampi(HBD ? v : (int)(int16_t)(uint16_t)v, 0, px_max);
                            }
                        }
                    } else if (fx) { // *_x_*
                        int in[12];
                        load4u(win + qy * ws + qx, in); load4u(win + qy * ws + qx + 4, in + 4); load4u(win + qy * ws + qx + 8, in + 8);
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            int sum = 0;
#pragma unroll
                            for (int m = 0; m < 8; m++) sum += c_interp[tabx][r.sx][m] * in[i + m];
                            const int r0 = (sum + 4) >> 3;
                            res[i] = comp ? r0 + ro : clampi((r0 + 8) >> 4, 0, px_max);
                        }
                    } else { // *_y_*
                        int sum[4] = {0, 0, 0, 0};
#pragma unroll
                        for (int m = 0; m < 8; m++) {
                            int v[4];
                            load4u(win + (qy + m) * ws + qx, v);
                            const int c = c_interp[taby][r.sy][m];
#pragma unroll
                            for (int i = 0; i < 4; i++) sum[i] += c * v[i];
                        }
#pragma unroll
                        for (int i = 0; i < 4; i++) res[i] = comp ? ((sum[i] * 16 + 64) >> 7) + ro : clampi((sum[i] + 64) >> 7, 0, px_max);
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    if (!comp) out[i] = res[i];
                    else if (k == 0) acc[i] = (int)(uint16_t)res[i]; // the CONV_BUF_TYPE store
                    else {
                        int tmp = acc[i];
                        tmp = j.comp_mode ? (tmp * (int)j.fwd_offset + res[i] * (int)j.bck_offset) >> 4 : (tmp + res[i]) >> 1;
                        tmp -= ro;
                        out[i] = clampi((tmp + 8) >> 4, 0, px_max);
                    }
                }
            }
            if (t.active) {
                Px *p = L.pred[slot] + lane * 4; // the tile row-major, TW wide: the lane's quad is its lane-th
                p[0] = (Px)out[0]; p[1] = (Px)out[1]; p[2] = (Px)out[2]; p[3] = (Px)out[3];
            }
        }
    }
    wave_sync();
}

template <bool HBD> __global__ __launch_bounds__(64 * kWaves) void ifs_kernel(const SvtHipIfsDesc d) {
    using Px = typename std::conditional<HBD, uint16_t, uint8_t>::type;
    __shared__ __attribute__((aligned(16))) WaveLds<Px> s_lds[kWaves];
    constexpr int bd = HBD ? 10 : 8;
    const int      lane = (int)(threadIdx.x & 63u);
    const int      wave = uniform((int)(threadIdx.x >> 6));
    const uint32_t job  = blockIdx.x * (uint32_t)kWaves + (uint32_t)wave;
    if (job >= d.n_jobs) return;
    const SvtHipIfsJob       ij = d.jobs[job];
    const SvtHipInterPredJob j  = ij.pred;
    const int  w = j.width, h = j.height;
    const bool comp  = j.ref[1] != SVT_HIP_INTER_PRED_NO_REF;
    const int  nrefs = comp ? 2 : 1;

    bool ok = is_block_size(w, h) && j.ref[0] < d.n_refs && ij.pred_ctx[0] < SVT_HIP_IFS_CONTEXTS && ij.pred_ctx[1] < SVT_HIP_IFS_CONTEXTS;
    if (comp) {
        ok = ok && j.ref[1] < d.n_refs && j.comp_mode <= 1;
        if (j.comp_mode == 1) { // quant_dist_lookup_table: {9,7} {11,5} {12,4} {13,3} and their mirrors
            const int f = j.fwd_offset, b = j.bck_offset;
            ok = ok && f + b == 16 && (f == 9 || f == 11 || f == 12 || f == 13 || f == 7 || f == 5 || f == 4 || f == 3);
        }
    }
    if (j.flags & SVT_HIP_INTER_PRED_MV0_FROM_ARRAY) ok = ok && d.mv_array != nullptr && j.mv_index[0] < d.n_mvs;
    if (comp && (j.flags & SVT_HIP_INTER_PRED_MV1_FROM_ARRAY)) ok = ok && d.mv_array != nullptr && j.mv_index[1] < d.n_mvs;
    if (d.dst) ok = ok && (uint64_t)j.dst_offset + (uint64_t)(h > 0 ? h - 1 : 0) * d.dst_stride + (uint64_t)w <= d.dst_samples;
    ok = ok && (uint64_t)ij.src_offset + (uint64_t)(h > 0 ? h - 1 : 0) * d.src_stride + (uint64_t)w <= d.src_samples;
    if (!ok) {
        if (lane == 0) d.status[job] = SVT_HIP_IFS_UNDEFINED;
        return;
    }

    RefView rv0, rv1;
    {
        const LumaPlane luma{};
        const int mi0 = (int)j.mv_index[0], mi1 = (int)j.mv_index[1];
        int mvr0 = j.mv[0][0], mvc0 = j.mv[0][1], mvr1 = j.mv[1][0], mvc1 = j.mv[1][1];
        if (j.flags & SVT_HIP_INTER_PRED_MV0_FROM_ARRAY) { mvr0 = d.mv_array[2 * (size_t)mi0]; mvc0 = d.mv_array[2 * (size_t)mi0 + 1]; }
        if (comp && (j.flags & SVT_HIP_INTER_PRED_MV1_FROM_ARRAY)) { mvr1 = d.mv_array[2 * (size_t)mi1]; mvc1 = d.mv_array[2 * (size_t)mi1 + 1]; }
        rv0 = ref_view(luma, j, d.refs[j.ref[0]], uniform(mvr0), uniform(mvc0));
        rv1 = comp ? ref_view(luma, j, d.refs[j.ref[1]], uniform(mvr1), uniform(mvc1)) : rv0;
    }
    const bool ux = rv0.sx != 0 || (comp && rv1.sx != 0), uy = rv0.sy != 0 || (comp && rv1.sy != 0);
    // the pairs the search visits, and the distinct predictions behind them
    uint32_t searched = 0, need = 0;
    for (int p = 0; p < kSlots; p++) {
        const int yf = p / 3, xf = p % 3;
        if (!d.enable_dual_filter && yf != xf) continue;
        searched |= 1u << p;
        need |= 1u << ((uy ? yf : 0) * 3 + (ux ? xf : 0));
    }

    const TileWalk t = tile_walk(w, h, lane);
    WaveLds<Px>   &L = s_lds[wave];
    const int  shift = (d.subsampled_distortion && h > 16) ? 1 : 0;
    const bool psy   = d.psy_rd > 0.0;
    const int  pn    = (w >= 8 && (h >> shift) >= 8) ? 8 : 4;           // the psy tile
    const int  ptx   = t.TW / pn, pt = ptx * ((t.TH >> shift) / pn);     // psy tiles per row of a tile, per tile: 1, 2 or 4
    const int  pslot = lane / pt, ptile = lane - pslot * pt;             // the lane's part of the psy pass
    const Px  *src   = (const Px *)d.src + ij.src_offset;

    uint32_t sse_acc[kSlots];
#pragma unroll
    for (int s = 0; s < kSlots; s++) sse_acc[s] = 0;
    u64 nrg_acc = 0;

    for (int ty = 0; ty < h; ty += t.TH)
        for (int tx = 0; tx < w; tx += t.TW) {
            tile_preds<HBD>(L, rv0, rv1, nrefs, j, t, tx, ty, need, ux, uy, lane);
            int s4[4] = {0, 0, 0, 0};
            const bool row_counts = t.active && (t.qy & shift) == 0;
            if (t.active) {
                const Px *p = src + (size_t)(ty + t.qy) * d.src_stride + (size_t)(tx + t.qx);
#pragma unroll
                for (int i = 0; i < 4; i++) s4[i] = (int)p[i];
                if (psy) {
                    Px *q = L.pred[kSlots] + lane * 4;
                    q[0] = (Px)s4[0]; q[1] = (Px)s4[1]; q[2] = (Px)s4[2]; q[3] = (Px)s4[3];
                }
            }
#pragma unroll
            for (int s = 0; s < kSlots; s++)
                if ((need >> s) & 1u) {
                    if (row_counts) {
                        const Px *q = L.pred[s] + lane * 4;
#pragma unroll
                        for (int i = 0; i < 4; i++) { const int df = s4[i] - (int)q[i]; sse_acc[s] += (uint32_t)(df * df); }
                    }
                }
            if (psy) {
                wave_sync(); // the source tile is in its slot
                int32_t e = 0;
                if (pslot <= kSlots && (pslot == kSlots || ((need >> pslot) & 1u))) {
                    const int py = ptile / ptx, px = ptile - py * ptx;
                    View<Px> v;
                    v.p = L.pred[pslot] + ((py * pn) << shift) * t.TW + px * pn; v.stride = (uint32_t)(t.TW << shift); v.fx1 = 0; v.fy1 = 0;
                    e = psy_tile_energy<Px>(v, pn);
                }
                const int32_t es = __shfl(e, kSlots * pt + ptile, 64);
                if (pslot < kSlots && ((need >> pslot) & 1u)) { const int32_t df = es - e; nrg_acc += (u64)(df < 0 ? -df : df); }
            }
        }

    // the sums of a slot: the SSE over the wave, the energy over the slot's psy lanes
    u64 sse_tot[kSlots];
#pragma unroll
    for (int s = 0; s < kSlots; s++) sse_tot[s] = wave_sum64_dpp((u64)sse_acc[s]);
    const int  pair = lane < kSlots ? lane : 0, yf = pair / 3, xf = pair - yf * 3;
    const int  slot = (uy ? yf : 0) * 3 + (ux ? xf : 0);
    u64 sse = 0, nrg = 0;
#pragma unroll
    for (int s = 0; s < kSlots; s++) sse = slot == s ? sse_tot[s] : sse;
    for (int k = 0; k < pt; k++) {
        const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)nrg_acc, slot * pt + k, 64), hi = (uint32_t)__shfl((int)(uint32_t)(nrg_acc >> 32), slot * pt + k, 64);
        nrg += ((u64)hi << 32) | lo;
    }
    sse <<= shift;
    if (psy) {
        const u64 total = HBD ? nrg << 2 : nrg >> 1; // svt_psy_distortion_hbd / svt_psy_distortion's last line
        sse += (u64)((double)total * d.psy_rd) << shift; // get_svt_psy_full_dist
    }
    // model_rd_for_sb's tail, svt_av1_get_switchable_rate, RDCOST and the biases, one pair per lane
    int32_t rate = 0;
    u64     dist;
    if (d.skip_sse_rd_model) dist = sse * 10;
    else {
        int n_log2 = 0;
        for (int v = w * h; v > 1; v >>= 1) n_log2++;
        model_rd((sse + ((1ull << (2 * (bd - 8))) >> 1)) >> (2 * (bd - 8)), n_log2, (int)(int16_t)d.quantizer >> (bd - 5), &rate, &dist);
    }
    int32_t rs = d.switchable_interp_fac_bits[ij.pred_ctx[0] * 3 + yf];
    if (d.enable_dual_filter) rs += d.switchable_interp_fac_bits[ij.pred_ctx[1] * 3 + xf];
    u64 rd = (u64)((((i64)(rs + rate) * (i64)d.lambda + 256) >> 9) + (i64)dist * 128);
    if (d.smooth_bias_pct && (yf == 1 || xf == 1)) rd = (rd * d.smooth_bias_pct) / 100;
    if (d.spy_rd) {
        if (yf == 2 || xf == 2) rd = (rd * 75) / 100;
        if (yf == 0 || xf == 0) rd = (rd * 80) / 100;
    }
    const bool visited = lane < kSlots && ((searched >> lane) & 1u);
    if (lane < kSlots) {
        if (d.rd) d.rd[(size_t)job * kSlots + lane] = visited ? rd : SVT_HIP_IFS_SKIPPED;
        if (d.sse) d.sse[(size_t)job * kSlots + lane] = visited ? sse : SVT_HIP_IFS_SKIPPED;
    }
    // the first minimum, in the reference's order
    u64 best = ~0ull;
    int winner = 0, best_rs = 0; // best_filters = 0, switchable_rate = 0 when no pair is below ~0
    for (int p = 0; p < kSlots; p++) {
        if (!((searched >> p) & 1u)) continue;
        const u64 v = ((u64)(uint32_t)__shfl((int)(uint32_t)(rd >> 32), p, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)rd, p, 64);
        const int r = __shfl(rs, p, 64);
        if (v < best) { best = v; winner = p; best_rs = r; }
    }
    winner = uniform(winner);
    const int wy = winner / 3, wx = winner - wy * 3;
    if (lane == 0) {
        SvtHipIfsResult res;
        memset(&res, 0, sizeof(res));
        res.best_rd = best; res.interp_filters = (uint32_t)wy | ((uint32_t)wx << 16); res.switchable_rate = best_rs;
        res.filter_x = (uint8_t)wx; res.filter_y = (uint8_t)wy; res.winner = (uint8_t)winner;
        d.results[job] = res;
    }

    if (d.dst) { // the winner's samples
        const int  wslot  = (uy ? wy : 0) * 3 + (ux ? wx : 0);
        const bool one    = t.TW == w && t.TH == h; // its slot still holds the whole block
        Px *const  dst    = (Px *)d.dst;
        for (int ty = 0; ty < h; ty += t.TH)
            for (int tx = 0; tx < w; tx += t.TW) {
                if (!one) tile_preds<HBD>(L, rv0, rv1, nrefs, j, t, tx, ty, 1u << wslot, ux, uy, lane);
                if (t.active) {
                    const Px *q = L.pred[wslot] + lane * 4;
                    const uint32_t o0 = q[0], o1 = q[1], o2 = q[2], o3 = q[3];
                    Px *p = dst + (size_t)j.dst_offset + (size_t)(ty + t.qy) * d.dst_stride + (size_t)(tx + t.qx);
                    if (HBD) {
                        if (((uintptr_t)p & 7u) == 0) *(uint2 *)p = make_uint2(o0 | (o1 << 16), o2 | (o3 << 16));
                        else { p[0] = (Px)o0; p[1] = (Px)o1; p[2] = (Px)o2; p[3] = (Px)o3; }
                    } else {
                        if (((uintptr_t)p & 3u) == 0) *(uint32_t *)p = o0 | (o1 << 8) | (o2 << 16) | (o3 << 24);
                        else { p[0] = (Px)o0; p[1] = (Px)o1; p[2] = (Px)o2; p[3] = (Px)o3; }
                    }
                }
            }
    }
    if (lane == 0) d.status[job] = SVT_HIP_IFS_OK;
}

// one lane per patch
__global__ __launch_bounds__(256) void ifs_scatter_kernel(const SvtHipIfsScatterDesc d) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= d.n_patches) return;
    const SvtHipIfsPatch p = d.patches[i];
    if (p.result_index >= d.n_results || p.record_index >= d.n_records || d.result_status[p.result_index] != SVT_HIP_IFS_OK) {
        d.status[i] = SVT_HIP_IFS_UNDEFINED;
        return;
    }
    uint8_t *rec = (uint8_t *)d.base + (size_t)p.record_index * d.record_stride + d.filter_x_offset;
    rec[0] = d.results[p.result_index].filter_x;
    rec[1] = d.results[p.result_index].filter_y;
    d.status[i] = SVT_HIP_IFS_OK;
}

} // namespace

extern "C" {

int svt_hip_ifs_check_desc(const SvtHipIfsDesc *d) {
    if (!d) BAD("svt_hip_ifs_check_desc: null descriptor");
    if (!d->src || !d->jobs || !d->results || !d->status || !d->switchable_interp_fac_bits)
        BAD("svt_hip_ifs_check_desc: a mandatory pointer (src, jobs, results, status, switchable_interp_fac_bits) is null");
    if (d->bit_depth != 8 && d->bit_depth != 10) BAD("svt_hip_ifs_check_desc: bit_depth %u (8 or 10)", d->bit_depth);
    const int rc = svt_hip_check_inter_pred_refs("svt_hip_ifs_check_desc", d->refs, d->n_refs);
    if (rc) return rc;
    if (d->src_stride == 0 || d->src_samples == 0) BAD("svt_hip_ifs_check_desc: src_stride %u / src_samples %llu is zero", d->src_stride, (unsigned long long)d->src_samples);
    if (d->dst && (d->dst_stride == 0 || d->dst_samples == 0))
        BAD("svt_hip_ifs_check_desc: dst with dst_stride %u / dst_samples %llu zero", d->dst_stride, (unsigned long long)d->dst_samples);
    if (d->n_mvs && !d->mv_array) BAD("svt_hip_ifs_check_desc: n_mvs %u without mv_array", d->n_mvs);
    if (d->quantizer < 1 || d->quantizer > 32767) BAD("svt_hip_ifs_check_desc: quantizer %d (1..32767)", d->quantizer);
    if (d->smooth_bias_pct > 1000) BAD("svt_hip_ifs_check_desc: smooth_bias_pct %u (0: off, else a percentage up to 1000)", d->smooth_bias_pct);
    return SVT_HIP_OK;
}

// svt_hip_ifs_scatter_filters has no check_desc entry: what it refuses
static int ifs_scatter_check(const SvtHipIfsScatterDesc *d) {
    if (!d->patches || !d->results || !d->result_status || !d->base || !d->status)
        BAD("svt_hip_ifs_scatter_filters: a pointer (patches, results, result_status, base, status) is null");
    if (d->record_stride == 0 || (uint64_t)d->filter_x_offset + 2 > d->record_stride)
        BAD("svt_hip_ifs_scatter_filters: record_stride %u, filter_x_offset %u (the two bytes lie inside a record)", d->record_stride, d->filter_x_offset);
    return SVT_HIP_OK;
}

const int32_t *svt_hip_ifs_model_table(int which) { return which >= 0 && which < 3 ? h_model[which] : nullptr; }

size_t svt_hip_ifs_layout(int what, int field) {
#define D(f) offsetof(SvtHipIfsDesc, f)
#define J(f) offsetof(SvtHipIfsJob, f)
#define R(f) offsetof(SvtHipIfsResult, f)
#define P(f) offsetof(SvtHipIfsPatch, f)
#define S(f) offsetof(SvtHipIfsScatterDesc, f)
    static const size_t desc[] = {D(bit_depth), D(n_refs), D(enable_dual_filter), D(subsampled_distortion), D(skip_sse_rd_model), D(spy_rd), D(reserved), D(n_jobs),
                                  D(n_mvs), D(refs), D(src), D(src_stride), D(dst_stride), D(src_samples), D(dst), D(dst_samples), D(jobs), D(mv_array),
                                  D(quantizer), D(lambda), D(smooth_bias_pct), D(reserved2), D(psy_rd), D(switchable_interp_fac_bits), D(results), D(rd), D(sse),
                                  D(status)};
    static const size_t job[]  = {J(pred), J(src_offset), J(pred_ctx), J(reserved)};
    static const size_t res[]  = {R(best_rd), R(interp_filters), R(switchable_rate), R(filter_x), R(filter_y), R(winner), R(reserved)};
    static const size_t pat[]  = {P(result_index), P(record_index)};
    static const size_t sca[]  = {S(n_patches), S(n_results), S(n_records), S(record_stride), S(filter_x_offset), S(reserved), S(patches), S(results),
                                  S(result_status), S(base), S(status)};
#undef D
#undef J
#undef R
#undef P
#undef S
    const SvtHipLayoutRow rows[] = {layout_row<SvtHipIfsDesc>(desc), layout_row<SvtHipIfsJob>(job), layout_row<SvtHipIfsResult>(res), layout_row<SvtHipIfsPatch>(pat),
                                    layout_row<SvtHipIfsScatterDesc>(sca)};
    return layout_lookup(rows, what, field);
}

int svt_hip_ifs_batch(SvtHipContext *ctx, const SvtHipIfsDesc *d) {
    return enqueue_batch("svt_hip_ifs_batch", ctx, d, svt_hip_ifs_check_desc, &SvtHipIfsDesc::n_jobs, [=] {
        hipLaunchKernelGGL(pick_hbd(d->bit_depth, ifs_kernel<true>, ifs_kernel<false>), dim3(ceil_div(d->n_jobs, kWaves)), dim3(64 * kWaves), 0, ctx->stream, *d);
    });
}

int svt_hip_ifs_scatter_filters(SvtHipContext *ctx, const SvtHipIfsScatterDesc *d) {
    return enqueue_batch("svt_hip_ifs_scatter_filters", ctx, d, ifs_scatter_check, &SvtHipIfsScatterDesc::n_patches,
                         [=] { hipLaunchKernelGGL(ifs_scatter_kernel, dim3(ceil_div(d->n_patches, 256)), dim3(256), 0, ctx->stream, *d); });
}

} // extern "C"
