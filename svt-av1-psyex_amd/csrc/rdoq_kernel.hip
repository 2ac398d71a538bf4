// rdoq_kernel.hip -- RDOQ (the trellis pass over quantised coefficients) on gfx950: svt_hip_rdoq_batch, the step between the "fp" quantizer of
// svt_hip_rd_batch and the rate of svt_hip_coeff_rate_batch.
//
// Reference functions restated (Source/Lib):
//   the caller's frame of svt_aom_quantize_inv_quantize (is_encode_pass == 0)       Codec/full_loop.c:1764-1817,1832-1836
//   svt_av1_optimize_b                                                               Codec/full_loop.c:1127-1336
//   update_coeff_general, update_coeff_eob, update_coeff_simple, update_skip         Codec/full_loop.c:948-999,847-947,1001-1045,1046-1061
//   get_coeff_cost_general / _eob, get_two_coeff_cost_simple, get_br_cost_with_diff and its two Golomb tables   Codec/full_loop.c:734-838
//   get_dqv, get_qc_dqc_low, get_coeff_dist, plane_rd_mult                           Codec/full_loop.c:840-845,762-772,1077-1085
//   svt_fast_optimize_b = update_coeff_eob_fast                                      Codec/full_loop.c:1092-1126
//   RDCOST (signed 64-bit: dist - dist0 is negative)                                 Codec/rd_cost.h:37
//   svt_av1_compute_cul_level_c, svt_full_distortion_kernel32_bits                   Codec/full_loop.c:1449-1466, Codec/pic_operators.c:150-172
// TUNE_CHROMA_SSIM is 1 in the reference tree (Source/API/EbDebugMacros.h:43): plane_rd_mult = {17, 13}, {16, 10}.
//
// The lay-out (the cost tables and a group's padded levels array in LDS, G lanes per job), the context rules and the shared cost terms of the
// level map: lvmap_core.h.  Beside its levels a group keeps one decision byte per coefficient in LDS.  The coefficient arrays are only READ
// until the tail: a coefficient is decided once, before that its value is the caller's, so a decision is a byte (0 kept, 1 lowered by one,
// 2 zeroed) and the tail writes the changed coefficients.
//   head    update_coeff_eob until more than four non-zeros are kept, then update_skip: serial in accu_rate / accu_dist.  Every lane of the
//           group carries the same state and takes the same decision (the loads are broadcasts); between two non-zeros the zeros only add
//           base_cost[ctx][0], with contexts that are fixed once the previous decision is made: a lane-parallel sum.
//   simple  update_coeff_simple for every remaining scan index down to 1.  accu_rate is dead from here on, and a decision reads the levels
//           of context neighbours alone, all of which have a larger row + column AND a larger scan index (tests/test_rdoq.py proves that for
//           every size and scan): the positions of one anti-diagonal are independent, and walking the anti-diagonals from the far corner
//           gives the serial result in at most w + h - 2 steps of up to 32 lanes (the walk starts at the farthest anti-diagonal that holds a non-zero).
//   DC      update_coeff_general, then the lane-parallel tail: stores, eob, dist_coeff, cul_level.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "svt_hip_internal.h"
#include "batch_host.h"
#include "../../include/svt_hip_dsp.h"
#include "lvmap_core.h"
#include "wave_ops.h"

namespace {

enum : uint8_t { kKept = 0, kLowered = 1, kZeroed = 2 };
enum : uint8_t { kStOptimised = 0, kStEmpty = 1, kStGated = 2, kStUndefined = 0xFF };

struct RdoqParams {
    SvtHipRdoqDesc d;
    const int16_t *iscan;    // [3][1024]: default, row (V_*), column (H_*) inverse scans of this tx_size
    LvMapGeom g;             // the packed block is (1 << g.bwl) wide; g.area: eob_perc
    int rshift;              // MAX(2, CLIP3(0, 7, sharpness))
    uint32_t n_packs;
};

// what a job's walk needs of its block
struct Blk : LvBlk {
    const SvtHipLvMapCoeffCost *cc;
    const SvtHipLvMapEobCost   *ec;
    const uint8_t *iqm; // null: flat
    int w, shift, dc_sign_ctx;
    int dq0, dq1;
    int64_t rdmult;
};

__device__ __forceinline__ int64_t rdcost(int64_t rm, int64_t r, int64_t d) { return ((r * rm + 256) >> 9) + d * 128; }
__device__ __forceinline__ int64_t coeff_dist(int64_t t, int64_t d, int shift) { const int64_t e = (t - d) * ((int64_t)1 << shift); return e * e; }
__device__ __forceinline__ int dqv_at(const Blk &b, int pos) {
    const int d = pos ? b.dq1 : b.dq0;
    return b.iqm ? (b.iqm[pos] * d + 16) >> 5 : d;
}
// get_coeff_cost_general; is_last: get_coeff_cost_eob (ctx is then get_lower_levels_ctx_eob's)
__device__ __forceinline__ int coeff_cost(const Blk &b, bool is_last, int pos, int a, int sign, int ctx) {
    int cost = is_last ? b.cc->base_eob_cost[ctx][min3(a) - 1] : b.cc->base_cost[ctx][min3(a)];
    if (a != 0) {
        cost += pos == 0 ? b.cc->dc_sign_cost[b.dc_sign_ctx][sign] : kCostLiteral;
        if (a > 2) cost += range_cost(b.cc, is_last ? br_ctx_eob(b, pos) : br_ctx(b, pos), a);
    }
    return cost;
}
// get_two_coeff_cost_simple (a >= 1, not the DC, not the last): the cost of the level and of the level below it
__device__ __forceinline__ int two_coeff_cost(const Blk &b, int pos, int a, int ctx, int &cost_low) {
    int cost = b.cc->base_cost[ctx][min3(a)] + kCostLiteral;
    int diff = a <= 3 ? b.cc->base_cost[ctx][a + 4] : 0;
    if (a > 2) { // get_br_cost_with_diff
        const int *lps = b.cc->lps_cost[br_ctx(b, pos)];
        const int  base_range = a - 3 < 12 ? a - 3 : 12;
        int        golomb = 0;
        if (a <= 15) diff += lps[base_range + 13];
        if (a >= 15) { // golomb_bits_cost / golomb_cost_diff: the cost steps by two literals where r is a power of two (one at r == 1)
            const int r = a - 14;
            golomb = golomb_cost(a);
            diff += (r & (r - 1)) == 0 ? (r == 1 ? kCostLiteral : 2 * kCostLiteral) : 0;
        }
        cost += lps[base_range] + golomb;
    }
    cost_low = cost - diff;
    return cost;
}

// update_coeff_general at (si, pos) on the caller's values; returns whether the level is lowered, adds the accumulators' terms
__device__ __forceinline__ bool general_step(const Blk &b, bool is_last, int si, int pos, int32_t qc, int32_t dqc, int32_t tqc, int &accu_rate, int64_t &accu_dist) {
    const int ctx = is_last ? eob_ctx(b, si) : lower_ctx(b, pos);
    if (qc == 0) { accu_rate += b.cc->base_cost[ctx][0]; return false; }
    const int     sign = qc < 0 ? 1 : 0, a = qc < 0 ? -qc : qc;
    const int64_t dist = coeff_dist(tqc, dqc, b.shift), dist0 = coeff_dist(tqc, 0, b.shift);
    const int     rate = coeff_cost(b, is_last, pos, a, sign, ctx);
    int64_t dist_low;
    int     rate_low;
    if (a == 1) { dist_low = dist0; rate_low = b.cc->base_cost[ctx][0]; }
    else {
        const int64_t adl = ((int64_t)(a - 1) * dqv_at(b, pos)) >> b.shift;
        dist_low = coeff_dist(tqc, sign ? -adl : adl, b.shift);
        rate_low = coeff_cost(b, is_last, pos, a - 1, sign, ctx);
    }
    if (rdcost(b.rdmult, rate_low, dist_low) < rdcost(b.rdmult, rate, dist)) { accu_rate += rate_low; accu_dist += dist_low - dist0; return true; }
    accu_rate += rate;
    accu_dist += dist - dist0;
    return false;
}

template <int N> __global__ void __launch_bounds__(64 * kWaves) rdoq_kernel(const RdoqParams p) {
    constexpr int G = N < 64 ? N : 64, PPL = N / G, JPW = 64 / G;
    __shared__ int32_t tab[kCoeffInts + kEobInts];
    __shared__ __attribute__((aligned(16))) uint8_t levels[kWaves][kLevelBytes];
    __shared__ uint8_t decisions[kWaves][1024];
    stage_cost_tables(tab, p.d.tables, p.g.txs_ctx, p.g.eob_multi, p.d.plane_type);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, grp = lane / G, gl = lane % G;
    const int w = 1 << p.g.bwl, h = N >> p.g.bwl;
    const int stride = w + 4, lev_bytes = stride * (h + 4); // a multiple of 16
    uint8_t  *lev = levels[wave] + grp * lev_bytes;
    uint8_t  *dec = decisions[wave] + grp * N;
    Blk b;
    b.cc = reinterpret_cast<const SvtHipLvMapCoeffCost *>(tab);
    b.ec = reinterpret_cast<const SvtHipLvMapEobCost *>(tab + kCoeffInts);
    b.lev = lev; b.stride = stride; b.bwl = p.g.bwl; b.w = w; b.n = N; b.shape = p.g.shape; b.shift = p.g.log_scale;
    for (uint32_t pack = blockIdx.x * kWaves + wave; pack < p.n_packs; pack += gridDim.x * kWaves) { // uniform per wave
        const uint32_t job   = pack * JPW + grp;
        const bool     valid = job < p.d.n_jobs;
        SvtHipRdoqJob  jb    = {};
        int            eob   = 0;
        if (valid) {
            const uint2 raw = *reinterpret_cast<const uint2 *>(p.d.jobs + job); // the job's eight bytes in one load
            jb.tx_type = raw.x & 255u; jb.txb_skip_ctx = (raw.x >> 8) & 255u; jb.dc_sign_ctx = (raw.x >> 16) & 255u; jb.is_inter = raw.x >> 24;
            jb.quant_row = raw.y & 255u; jb.flags = (raw.y >> 8) & 255u;
            eob = p.d.eob[job];
        }
        const bool defined = jb.tx_type < 16 && jb.txb_skip_ctx < 13 && jb.dc_sign_ctx < 3 && jb.quant_row < p.d.n_quant_rows;
        const int  kind = tx_scan_kind(jb.tx_type);
        const int16_t *iscan = p.iscan + (defined ? kind : 0) * 1024;
        const size_t   base  = (size_t)job * N;
        b.cls = tx_class(jb.tx_type);
        b.dc_sign_ctx = jb.dc_sign_ctx;
        b.iqm = jb.tx_type < 9 ? p.d.iqmatrix : nullptr; // IS_2D_TRANSFORM (full_loop.c:1606-1608)
        const bool walk = valid && defined && eob > 0 && eob <= N; // the job reads its coefficients
        int status = !valid || !defined || eob > N ? kStUndefined : (eob == 0 ? kStEmpty : kStOptimised);

        // svt_av1_txb_init_levels: min(|qcoeff|, 127) over the WHOLE block in a zero frame; no decision yet
        zero_levels<G>(lev, lev_bytes, gl);
        wave_sync();
#pragma unroll 1
        for (int it = 0; it < PPL; it++) {
            const int     pos = it * G + gl, row = pos >> p.g.bwl, col = pos - (row << p.g.bwl);
            const int32_t q   = walk ? p.d.qcoeff[base + pos] : 0;
            const uint32_t a  = q < 0 ? 0u - (uint32_t)q : (uint32_t)q;
            lev[row * stride + col] = (uint8_t)(a < 127u ? a : 127u);
            dec[pos] = kKept;
        }
        wave_sync();
        // (scan index << 10 | position) of the last non-zero level below scan index `bound`, -1 when there is none
        auto last_nz_below = [&](int bound) {
            int key = -1;
#pragma unroll 1
            for (int it = 0; it < PPL; it++) {
                const int pos = it * G + gl, row = pos >> p.g.bwl, col = pos - (row << p.g.bwl);
                const int si  = (int)(uint16_t)iscan[pos];
                if (si < bound && lev[row * stride + col] != 0) { const int k = (si << 10) | pos; key = k > key ? k : key; }
            }
            return group_max<G>(key);
        };
        auto zero_at = [&](int pos) {
            const int row = pos >> p.g.bwl, col = pos - (row << p.g.bwl);
            lev[row * stride + col] = 0;
            dec[pos] = kZeroed;
        };
        int last_key = -1;
        if (walk) {
            last_key = last_nz_below(eob);
            if ((last_key >> 10) != eob - 1) status = kStUndefined; // a zero at scan[eob - 1]
        }
        bool optimise = walk && status == kStOptimised, copy_b = false;
        const SvtHipQuantRow *qr = p.d.quant_rows + (defined ? jb.quant_row : 0);
        if (optimise) { b.dq0 = qr->dequant[0]; b.dq1 = qr->dequant[1]; }
        int eob_for_cost = eob;
        if (optimise) { // the caller's frame (full_loop.c:1764-1796)
            const int  eob_perc  = eob * 100 / p.g.area;
            const bool fast_mode = jb.is_inter ? p.d.eob_fast_inter != 0 : p.d.eob_fast_intra != 0;
            if (eob_perc >= p.d.eob_th) {
                status   = kStGated;
                optimise = false;
                copy_b   = p.d.qcoeff_b != nullptr;
            } else if (eob_perc >= p.d.eob_fast_th || fast_mode) {
                // update_coeff_eob_fast with the un-weighted dequant: the first scan index from the end whose coefficient stays.  svt_av1_optimize_b's
                // own trim (fast_mode) repeats the same test, so it changes nothing behind the caller's; alone it leaves the eob cost at the old eob
                const int z0 = b.dq0 + ((b.dq0 * 70 + 64) >> 7), z1 = b.dq1 + ((b.dq1 * 70 + 64) >> 7);
                int key = -1;
#pragma unroll 1
                for (int it = 0; it < PPL; it++) {
                    const int pos = it * G + gl, row = pos >> p.g.bwl, col = pos - (row << p.g.bwl);
                    const int si  = (int)(uint16_t)iscan[pos];
                    if (si < eob && lev[row * stride + col] != 0) {
                        const int32_t c  = p.d.coeff[base + pos];
                        const int64_t ac = c < 0 ? -(int64_t)c : (int64_t)c;
                        if (!((ac << (1 + p.g.log_scale)) < (pos ? z1 : z0))) { const int k = (si << 10) | pos; key = k > key ? k : key; }
                    }
                }
                key = group_max<G>(key);
                const int new_eob = (key >> 10) + 1; // key == -1: 0
#pragma unroll 1
                for (int it = 0; it < PPL; it++) {
                    const int pos = it * G + gl, row = pos >> p.g.bwl, col = pos - (row << p.g.bwl);
                    const int si  = (int)(uint16_t)iscan[pos];
                    if (si >= new_eob && si < eob && lev[row * stride + col] != 0) { lev[row * stride + col] = 0; dec[pos] = kZeroed; }
                }
                wave_sync();
                if (eob_perc >= p.d.eob_fast_th) eob_for_cost = new_eob;
                eob      = new_eob;
                last_key = key;
                if (eob == 0) {
                    optimise = false;
                    status   = eob_perc >= p.d.eob_fast_th ? kStEmpty : kStOptimised;
                }
            }
            if (optimise) { // svt_av1_optimize_b
                const bool sharp     = (jb.flags & 1) != 0;
                const int  mult      = jb.is_inter ? (p.d.plane_type ? 10 : 16) : (p.d.plane_type ? 13 : 17); // plane_rd_mult
                b.rdmult             = (((int64_t)p.d.lambda * mult * (sharp ? 0 : 100)) / 100 + 2) >> p.rshift;
                int     accu_rate    = eob_cost(b.cc, b.ec, b.cls, eob_for_cost);
                int64_t accu_dist    = 0;
                int     nz_num       = 1, nz0 = last_key & 1023, nz1 = 0, nz2 = 0, nz3 = 0, nz4 = 0;
                int     S            = eob - 2; // the next scan index to visit
                { // the last coefficient
                    const int     pos = nz0;
                    const int32_t qc = p.d.qcoeff[base + pos], dqc = p.d.dqcoeff[base + pos], tqc = p.d.coeff[base + pos];
                    const int     a = qc < 0 ? -qc : qc;
                    if (a >= 2) {
                        if (general_step(b, true, eob - 1, pos, qc, dqc, tqc, accu_rate, accu_dist) && gl == 0) {
                            const int row = pos >> p.g.bwl, col = pos - (row << p.g.bwl);
                            lev[row * stride + col] = (uint8_t)(a - 1 < 127 ? a - 1 : 127);
                            dec[pos] = kLowered;
                        }
                    } else {
                        accu_rate += coeff_cost(b, true, pos, a, qc < 0 ? 1 : 0, eob_ctx(b, eob - 1));
                        accu_dist += coeff_dist(tqc, dqc, p.g.log_scale) - coeff_dist(tqc, 0, p.g.log_scale);
                    }
                    wave_sync();
                }
                if (!fast_mode) {
                    while (S >= 0 && nz_num <= 4) { // update_coeff_eob
                        const int key = last_nz_below(S + 1), nsi = key >> 10; // key == -1: nsi == -1
                        { // the zeros on the way: base_cost[ctx][0] each
                            int sum = 0;
#pragma unroll 1
                            for (int it = 0; it < PPL; it++) {
                                const int pos = it * G + gl, row = pos >> p.g.bwl, col = pos - (row << p.g.bwl);
                                const int si  = (int)(uint16_t)iscan[pos];
                                if (si > nsi && si <= S && lev[row * stride + col] == 0) sum += b.cc->base_cost[lower_ctx(b, pos)][0];
                            }
                            accu_rate += group_sum<G>(sum);
                        }
                        S = nsi - 1;
                        if (key < 0) { S = -1; break; }
                        const int     pos = key & 1023, row = pos >> p.g.bwl, col = pos - (row << p.g.bwl);
                        const int32_t qc = p.d.qcoeff[base + pos], dqc = p.d.dqcoeff[base + pos], tqc = p.d.coeff[base + pos];
                        const int     a = qc < 0 ? -qc : qc, sign = qc < 0 ? 1 : 0;
                        const int     ctx = lower_ctx(b, pos);
                        const int64_t dist0 = coeff_dist(tqc, 0, p.g.log_scale);
                        int64_t       dist  = coeff_dist(tqc, dqc, p.g.log_scale) - dist0;
                        int           rate  = coeff_cost(b, false, pos, a, sign, ctx);
                        int64_t       rd    = rdcost(b.rdmult, (int64_t)accu_rate + rate, accu_dist + dist);
                        int64_t dist_low, rd_low;
                        int     rate_low;
                        if (a == 1) {
                            dist_low = 0;
                            rate_low = b.cc->base_cost[ctx][0];
                            rd_low   = rdcost(b.rdmult, (int64_t)accu_rate + rate_low, accu_dist);
                        } else {
                            const int64_t adl = ((int64_t)(a - 1) * dqv_at(b, pos)) >> p.g.log_scale;
                            dist_low = coeff_dist(tqc, sign ? -adl : adl, p.g.log_scale) - dist0;
                            rate_low = coeff_cost(b, false, pos, a - 1, sign, ctx);
                            rd_low   = rdcost(b.rdmult, (int64_t)accu_rate + rate_low, accu_dist + dist_low);
                        }
                        bool      lower_new_eob = false, lower = false;
                        const int ctx_new = eob_ctx(b, nsi), new_eob_cost = eob_cost(b.cc, b.ec, b.cls, nsi + 1);
                        int       rate_coeff_eob = new_eob_cost + coeff_cost(b, true, pos, a, sign, ctx_new);
                        int64_t   dist_new_eob = dist, rd_new_eob = rdcost(b.rdmult, rate_coeff_eob, dist_new_eob);
                        if (a > 1) {
                            const int     rate_low_eob = new_eob_cost + coeff_cost(b, true, pos, a - 1, sign, ctx_new);
                            const int64_t rd_low_eob   = rdcost(b.rdmult, rate_low_eob, dist_low);
                            if (rd_low_eob < rd_new_eob) { lower_new_eob = true; rd_new_eob = rd_low_eob; rate_coeff_eob = rate_low_eob; dist_new_eob = dist_low; }
                        }
                        if (rd_low < rd) { lower = true; rd = rd_low; rate = rate_low; dist = dist_low; }
                        if (!sharp && rd_new_eob < rd) {
                            if (gl == 0) {
                                if (nz_num > 0) zero_at(nz0);
                                if (nz_num > 1) zero_at(nz1);
                                if (nz_num > 2) zero_at(nz2);
                                if (nz_num > 3) zero_at(nz3);
                                if (nz_num > 4) zero_at(nz4);
                            }
                            eob       = nsi + 1;
                            nz_num    = 0;
                            accu_rate = rate_coeff_eob;
                            accu_dist = dist_new_eob;
                            lower     = lower_new_eob;
                        } else {
                            accu_rate += rate;
                            accu_dist += dist;
                        }
                        if (lower && gl == 0) {
                            lev[row * stride + col] = (uint8_t)(a - 1 < 127 ? a - 1 : 127);
                            dec[pos] = kLowered;
                        }
                        if (!(lower && a == 1)) { // the coefficient is still non-zero
                            nz0 = nz_num == 0 ? pos : nz0; nz1 = nz_num == 1 ? pos : nz1; nz2 = nz_num == 2 ? pos : nz2;
                            nz3 = nz_num == 3 ? pos : nz3; nz4 = nz_num == 4 ? pos : nz4;
                            nz_num++;
                        }
                        wave_sync();
                    }
                }
                if (S == -1 && nz_num <= 4) { // update_skip
                    const int64_t rd     = rdcost(b.rdmult, (int64_t)accu_rate + b.cc->txb_skip_cost[jb.txb_skip_ctx][0], accu_dist);
                    const int64_t rd_new = rdcost(b.rdmult, b.cc->txb_skip_cost[jb.txb_skip_ctx][1], 0);
                    if (!sharp && rd_new < rd) {
                        if (gl == 0) { // the levels are not read again: this is the last step (the DC is among the zeroed)
                            if (nz_num > 0) zero_at(nz0);
                            if (nz_num > 1) zero_at(nz1);
                            if (nz_num > 2) zero_at(nz2);
                            if (nz_num > 3) zero_at(nz3);
                        }
                        eob = 0;
                        wave_sync();
                    }
                }
                // update_coeff_simple for scan indices S .. 1, one anti-diagonal at a time
                if (S >= 1) {
                    int d_first = 0; // the farthest anti-diagonal that holds a non-zero of this phase: nothing is decided beyond it
#pragma unroll 1
                    for (int it = 0; it < PPL; it++) {
                        const int pos = it * G + gl, row = pos >> p.g.bwl, col = pos - (row << p.g.bwl);
                        const int si  = (int)(uint16_t)iscan[pos];
                        if (si >= 1 && si <= S && lev[row * stride + col] != 0) d_first = row + col > d_first ? row + col : d_first;
                    }
                    d_first = group_max<G>(d_first);
#pragma unroll 1
                    for (int d = d_first; d >= 1; d--) {
                        const int rmin = d - (w - 1) > 0 ? d - (w - 1) : 0, rmax = d < h - 1 ? d : h - 1;
                        const int row = rmin + gl, col = d - row;
                        if (row <= rmax) {
                            const int pos = (row << p.g.bwl) + col;
                            const int si  = (int)(uint16_t)iscan[pos];
                            if (si >= 1 && si <= S && lev[row * stride + col] != 0) {
                                const int32_t qc = p.d.qcoeff[base + pos], dqc = p.d.dqcoeff[base + pos], tqc = p.d.coeff[base + pos];
                                const int     a = qc < 0 ? -qc : qc;
                                const int64_t at = tqc < 0 ? -(int64_t)tqc : (int64_t)tqc, ad = dqc < 0 ? -(int64_t)dqc : (int64_t)dqc;
                                if (!(ad < at)) {
                                    int       rate_low;
                                    const int rate = two_coeff_cost(b, pos, a, lower_ctx(b, pos), rate_low);
                                    const int64_t adl = ((int64_t)(a - 1) * dqv_at(b, pos)) >> p.g.log_scale;
                                    if (rdcost(b.rdmult, rate_low, coeff_dist(at, adl, p.g.log_scale)) < rdcost(b.rdmult, rate, coeff_dist(at, ad, p.g.log_scale))) {
                                        lev[row * stride + col] = (uint8_t)(a - 1 < 127 ? a - 1 : 127);
                                        dec[pos] = kLowered;
                                    }
                                }
                            }
                        }
                        wave_sync();
                    }
                }
                if (S >= 0) { // the DC: update_coeff_general, its accumulators are dead
                    const int32_t qc = p.d.qcoeff[base], dqc = p.d.dqcoeff[base], tqc = p.d.coeff[base];
                    int     r_ = 0;
                    int64_t d_ = 0;
                    if (general_step(b, eob == 1, 0, 0, qc, dqc, tqc, r_, d_) && gl == 0) dec[0] = kLowered;
                    wave_sync();
                }
            }
        }

        // the tail: the changed coefficients, the distortion and the context of the result
        const bool write = valid && (status == kStOptimised || status == kStEmpty || copy_b);
        if (copy_b) eob = p.d.eob_b[job];
        uint64_t dist = 0, energy = 0;
        uint32_t cul = 0, dc_sign = 0;
        if (write) {
#pragma unroll 1
            for (int it = 0; it < PPL; it++) {
                const int pos = it * G + gl;
                int32_t   q, dq;
                const int32_t c = p.d.coeff[base + pos];
                if (copy_b) {
                    q = p.d.qcoeff_b[base + pos]; dq = p.d.dqcoeff_b[base + pos];
                    p.d.qcoeff[base + pos] = q; p.d.dqcoeff[base + pos] = dq;
                } else if (walk) {
                    q = p.d.qcoeff[base + pos]; dq = p.d.dqcoeff[base + pos];
                    const uint8_t how = dec[pos];
                    if (how != kKept) {
                        if (how == kZeroed) q = dq = 0;
                        else { // get_qc_dqc_low
                            const int     a   = (q < 0 ? -q : q) - 1;
                            const int32_t adl = (int32_t)(((int64_t)a * dqv_at(b, pos)) >> p.g.log_scale);
                            dq = q < 0 ? -adl : adl;
                            q  = q < 0 ? -a : a;
                        }
                        p.d.qcoeff[base + pos] = q; p.d.dqcoeff[base + pos] = dq;
                    }
                } else { q = p.d.qcoeff[base + pos]; dq = p.d.dqcoeff[base + pos]; } // eob == 0 on entry: nothing to change
                const int64_t e = (int64_t)c - dq;
                dist += (uint64_t)(e * e);
                energy += (uint64_t)((int64_t)c * c);
                if ((int)(uint16_t)iscan[pos] < eob) cul += q < 0 ? 0u - (uint32_t)q : (uint32_t)q;
                if (pos == 0) dc_sign = q < 0 ? 1u : (q > 0 ? 2u : 0u);
            }
        }
        dist    = group_sum<G>((unsigned long long)dist);
        energy  = group_sum<G>((unsigned long long)energy);
        cul     = group_sum<G>(cul < 63u ? cul : 63u); // every term is clamped, so the sum of up to 64 of them cannot wrap
        dc_sign = group_or<G>(dc_sign);
        if (gl == 0 && valid) {
            if (p.d.status) p.d.status[job] = (uint8_t)status;
            if (write) {
                if (status != kStEmpty || walk) p.d.eob[job] = (uint16_t)eob;
                if (p.d.dist_coeff) { p.d.dist_coeff[2 * (size_t)job] = dist; p.d.dist_coeff[2 * (size_t)job + 1] = energy; }
                if (p.d.cul_level) { // svt_av1_compute_cul_level_c: min(63, sum), the DC's sign in bits 6-7
                    uint32_t v = cul < 63u ? cul : 63u;
                    v = dc_sign == 1u ? (v | 64u) : (dc_sign == 2u ? v + 128u : v);
                    p.d.cul_level[job] = (uint8_t)v;
                }
            }
        }
        wave_sync(); // the next job's zero fill must not overtake this one's reads
    }
}

} // namespace

extern "C" {

size_t svt_hip_rdoq_desc_size(void) { return sizeof(SvtHipRdoqDesc); }

static int rdoq_check(const SvtHipRdoqDesc *d) {
    if (d->tx_size >= SVT_HIP_TX_SIZES_ALL || d->plane_type > 1 || d->sharpness > 7)
        BAD("svt_hip_rdoq_batch: tx_size %u (below 19) / plane_type %u (0 or 1) / sharpness %u (0..7)", d->tx_size, d->plane_type, d->sharpness);
    if (!d->jobs || !d->tables || !d->quant_rows || !d->coeff || !d->qcoeff || !d->dqcoeff || !d->eob)
        BAD("svt_hip_rdoq_batch: a mandatory pointer (jobs, tables, quant_rows, coeff, qcoeff, dqcoeff, eob) is null");
    if (d->n_quant_rows == 0) BAD("svt_hip_rdoq_batch: no quantizer rows");
    if ((d->qcoeff_b || d->dqcoeff_b || d->eob_b) && !(d->qcoeff_b && d->dqcoeff_b && d->eob_b)) BAD("svt_hip_rdoq_batch: the fallback needs qcoeff_b, dqcoeff_b and eob_b");
    return SVT_HIP_OK;
}

int svt_hip_rdoq_batch(SvtHipContext *ctx, const SvtHipRdoqDesc *d) {
    return enqueue_batch("svt_hip_rdoq_batch", ctx, d, rdoq_check, &SvtHipRdoqDesc::n_jobs, [=] {
        RdoqParams p;
        memset(&p, 0, sizeof(p));
        p.d = *d;
        p.iscan  = ctx->iscan_dev + (size_t)d->tx_size * 3 * 1024;
        p.g      = lvmap_geom(d->tx_size);
        p.rshift = d->sharpness > 2 ? d->sharpness : 2;
        const uint32_t grid = lvmap_grid(p.g, d->n_jobs, ctx->lvmap_max_grid, p.n_packs);
        switch (p.g.n) { // lvmap_geom gives one of these for every tx_size the check accepted
#define CASE(N) case N: hipLaunchKernelGGL(rdoq_kernel<N>, dim3(grid), dim3(64 * kWaves), 0, ctx->stream, p); break;
            CASE(16) CASE(32) CASE(64) CASE(128) CASE(256) CASE(512) CASE(1024)
#undef CASE
        }
    });
}

} // extern "C"
