// rd_kernel.hip -- batched mode-decision RD evaluation on gfx950: one wave64 workgroup per transform block runs
//   residual -> forward 2-D transform -> SATD -> quantize/dequantize (+eob) -> coefficient-domain distortion
//   -> inverse 2-D transform + reconstruction -> pixel-domain SSE
// i.e. one iteration of the reference's tx_type_search body (Source/Lib/Codec/product_coding_loop.c:4764-4934).
//
// Mapping: the W x H block lives in LDS as int32; a lane owns one column (then one row) of the separable
// transform and keeps the whole 1-D vector in registers -- the butterfly networks are fully unrolled at compile
// time from their structure (see dct_* below), so every register index and every cosine is a constant.  All
// arithmetic is the reference's integer arithmetic (32-bit wrapping products, 64-bit rounding: half_btf,
// Codec/inv_transforms.h:264-285), hence bit-exact.  Elementwise phases (quantizer, distortions) stride the block
// across the 64 lanes and reduce inside the wave (DPP where the range allows, see SVT_RD_DPP_REDUCE).  Source and prediction are read
// twice, once for the residual and once for the reconstruction (the second read is served by the caches); outputs are written once.  The
// kernels are bound by instruction issue, not by HBM.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include "svt_hip_internal.h"
#include "batch_host.h"
#include "../../include/svt_hip_dsp.h"

#include "txfm_core.h"

namespace {

struct RdParams {
    SvtHipRdBatchDesc d;
    const int16_t    *iscan[3]; // default, row (V_*), column (H_*) scans of this tx_size
    int               tx_size;
};

template <typename T> __device__ __forceinline__ int ldpix(const void *p, size_t i) { return (int)static_cast<const T *>(p)[i]; }

__host__ __device__ constexpr int rd_lanes_per_block(int ts) { return tx_wide(ts) > tx_high(ts) ? tx_wide(ts) : tx_high(ts); }
__host__ __device__ constexpr int rd_blocks_per_wave(int ts) { return 64 / rd_lanes_per_block(ts); }

// =========================================================================================================
// One wave64 per workgroup; the wave holds 64 / max(W, H) transform blocks side by side (lane = block * LW + l), so
// the 1-D passes keep every lane busy for all sizes.  A block lives in ONE LDS array with row pitch W + 1 dwords:
// column reads (stride 1) and row reads (stride W + 1) are both bank-conflict free.  The passes run in place --
// a wave executes its LDS loads before the stores that follow them in program order -- and the packed
// (top-left 32x32) coefficients of the 64-point sizes are compacted in place as well, which is what lets nine
// 64x64 workgroups share a CU's LDS.
// =========================================================================================================
// resident waves per SIMD the register allocation aims for: enough workgroups in flight that a picture's blocks of one size
// run as a single round (e.g. 32x32: 4,020 two-block workgroups on 256 CUs x 4 SIMDs x 4 waves)
#ifndef SVT_RD_WAVES_64
#define SVT_RD_WAVES_64 2
#endif
#ifndef SVT_RD_WAVES_32
#define SVT_RD_WAVES_32 4
#endif
#ifndef SVT_RD_RESIDUAL_AHEAD
#define SVT_RD_RESIDUAL_AHEAD 8 /* runs of 8 samples a lane has in flight while it forms the residual */
#endif
#ifndef SVT_RD_SCAN_AHEAD
#define SVT_RD_SCAN_AHEAD 16 /* coefficients per lane whose scan positions are fetched ahead of the quantizer loop */
#endif
#ifndef SVT_RD_WAVES_16
#define SVT_RD_WAVES_16 4
#endif
#ifndef SVT_RD_FOLD_INV_32LANE
#define SVT_RD_FOLD_INV_32LANE 1 /* the 32-lane layout folds the inverse DCT's round-shift as well (0: it keeps its 64-bit shift loop) */
#endif
// The bounded butterflies of a size's passes: 2 = hbtf2 (two v_mad_i32_i24 and a shift, the passes' round-shifts folded in), 3 = the same
// arithmetic left to the compiler, with the shift loops behind the passes.  The rectangular 32-lane layouts and 64x16 are at their register
// limit (128 / 256 VGPRs), and with the opaque instructions their allocation spills more than without: they keep the compiler's form.
__host__ __device__ constexpr int rd_bounded_btf(int ts) {
    return ((rd_lanes_per_block(ts) == 32 && tx_wide(ts) != tx_high(ts)) || (tx_wide(ts) == 64 && tx_high(ts) == 16)) ? 3 : 2;
}
// The inverse passes of a size may have a third, clamp-free tier (ipass_clamp_free, txfm_core.h) beside the bounded and the general one.  It is
// one more copy of both unrolled passes, and only 64x64 pays for it (-12.6 % per launch with the input clamps below).  16x16 and 32x32 measured
// SLOWER with it, +7.6 % and +20 % (32x32 executes 11 instructions per pixel fewer, but its allocation at the 128-register limit goes from 2 to 28
// spilled registers and VALU busy falls from 95 to 69 %; 16x16 executes more): profiles/r13_rd_clampfree_before_after.txt.  SVT_RD_CLAMP_FREE: 0 no
// size, 1 64x64, 2 the square 16 / 32 / 64-point sizes (the build that was measured).
#ifndef SVT_RD_CLAMP_FREE
#define SVT_RD_CLAMP_FREE 1
#endif
#ifndef SVT_RD_SKIP_ENTRY_CLAMPS
#define SVT_RD_SKIP_ENTRY_CLAMPS 1 /* the input clamps of both inverse passes run only in a wave whose largest raw input is outside their range */
#endif
#ifndef SVT_RD_PAIR_RESIDUAL_MAX
#define SVT_RD_PAIR_RESIDUAL_MAX 1 /* the residual loop tracks its extremes per pair of samples */
#endif
#ifndef SVT_RD_ROW_BOUND_FROM_QUANT
#define SVT_RD_ROW_BOUND_FROM_QUANT 1 /* a lean-quantizer wave whose bound M on |dqcoeff| passes the clamp-free test skips measuring the row input */
#endif
// The cost a lane pays once per block, whatever the block holds (profiles/r23_rd_fixed_cost_before_after.txt):
#ifndef SVT_RD_DPP_REDUCE
#define SVT_RD_DPP_REDUCE 1 /* the wave's five magnitudes and the block's sums on DPP and scalar registers, not ds_bpermute butterflies through the LDS crossbar */
#endif
#ifndef SVT_RD_RUN_BASE
#define SVT_RD_RUN_BASE 1 /* a lane's runs of samples addressed from one base per plane plus a wave-uniform multiple of the stride, not by one 64-bit product per run */
#endif
// Measured: -5 % at 16x16, -3 % at 64x64.  32x32 sits at its 128-register limit: with the magnitudes on DPP it spills 9 registers more, and with
// the sums alone it keeps its allocation and its time (+-0.5 %): it keeps the butterflies.  So do the sizes that were not timed (64x16 spills 21
// registers more with either switch).
__host__ __device__ constexpr bool rd_square_16_or_64(int ts) { return tx_wide(ts) == tx_high(ts) && (tx_wide(ts) == 16 || tx_wide(ts) == 64); }
__host__ __device__ constexpr bool rd_dpp_reduce(int ts) { return SVT_RD_DPP_REDUCE && rd_square_16_or_64(ts); }
// Measured: a further -2 % at 64x64 (eight runs per lane and plane); nothing at 16x16 (two runs); 32x32 spills 9 registers more with it.  The
// reconstruction forms its bases anew, from a lane index the compiler cannot tell from the first: 64x64 has no registers to keep them through the passes.
__host__ __device__ constexpr bool rd_run_base(int ts) { return SVT_RD_RUN_BASE && tx_wide(ts) == 64 && tx_high(ts) == 64; }
// one answer for the wave, in a scalar register; every lane of the wave calls it
template <bool DPP> __device__ __forceinline__ uint32_t rd_wave_max(uint32_t v) {
    if constexpr (DPP) return wave_max_dpp(v);
    else return (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max(v));
}
__host__ __device__ constexpr bool rd_clamp_free_tier(int ts) {
    return tx_wide(ts) == tx_high(ts) && (SVT_RD_CLAMP_FREE == 1 ? tx_wide(ts) == 64 : SVT_RD_CLAMP_FREE == 2 && tx_wide(ts) >= 16);
}
// The rectangular 32-lane layouts spill more with the input clamps in a branch of their own (16x32: 3 -> 10 registers); they and 64x16 clamp on load.
__host__ __device__ constexpr bool rd_skip_entry_clamps(int ts) { return SVT_RD_SKIP_ENTRY_CLAMPS && rd_bounded_btf(ts) == 2; }
#ifdef SVT_RD_TIER_STATS
// diagnostic build only: waves of rd_tx_kernel by the tier of their inverse row pass x that of their column pass (0 general, 1 bounded, 2 clamp-free),
// and [9] the waves whose row tier came from the quantizer's bound; svt_hip_rd_batch prints and clears them after every launch
__device__ unsigned int g_rd_tier_stats[10];
#endif
// the tier of an inverse pass: 2 clamp-free, 1 bounded butterflies, 0 general
template <bool FREE> __device__ __forceinline__ int ipass_tier(uint32_t wave_max_abs_input, int n, int clamp_bits) {
    if (FREE && ipass_clamp_free(wave_max_abs_input, n, clamp_bits)) return 2;
    return ipass_fits_18_bits(wave_max_abs_input, n) ? 1 : 0;
}
__host__ __device__ constexpr int rd_waves_per_simd(int ts) {
    return rd_lanes_per_block(ts) == 64 ? SVT_RD_WAVES_64 : rd_lanes_per_block(ts) == 32 ? SVT_RD_WAVES_32 : SVT_RD_WAVES_16;
}
template <int TS, int BD> __global__ void __launch_bounds__(64, rd_waves_per_simd(TS)) rd_tx_kernel(const RdParams p) {
    constexpr int W = tx_wide(TS), H = tx_high(TS), WP = W > 32 ? 32 : W, HP = H > 32 ? 32 : H, NP = WP * HP;
    constexpr int LW = rd_lanes_per_block(TS), BPW = rd_blocks_per_wave(TS);
    constexpr bool kShift32 = LW != 32; // bounded passes round-shift in 32 bits (measured: 64x64 -4 %; the 32-lane layout, at its 128-register limit, spills on it: +12 %)
    constexpr bool kFoldInv = LW != 32 || SVT_RD_FOLD_INV_32LANE; // the inverse DCT's last stage round-shifts (in 32 bits, in every layout)
    constexpr int kBtf = rd_bounded_btf(TS);
    constexpr bool kFree = rd_clamp_free_tier(TS), kSkipEntry = rd_skip_entry_clamps(TS);
    constexpr int PA = W + 1, PB = WP + 1; // row pitches (dwords) of the full block and of the packed coefficients
    constexpr int ROW_CLAMP = BD == 8 ? 16 : 18, COL_CLAMP = 16; // svt_av1_gen_inv_stage_range, inv_transforms.c:42-80
    constexpr bool RECT = (W == 2 * H || H == 2 * W);
    using Pix = typename std::conditional<BD == 8, uint8_t, uint16_t>::type;
    __shared__ int32_t lds[BPW][H * PA];
    const int      lane = threadIdx.x, blk = lane / LW, l = lane % LW;
    const uint32_t job   = blockIdx.x * BPW + blk;
    const bool     valid = job < p.d.n_jobs; // lanes of a missing block run along on job 0 and write nothing
    int32_t *A = lds[blk];
    const SvtHipTxJob jb = p.d.jobs[valid ? job : 0];
    const int tt = jb.tx_type & 15, vt = c_vtx[tt], ht = c_htx[tt];
    const bool ud = (vt == 2), lr = (ht == 2);
    const Pix *src  = static_cast<const Pix *>(p.d.src) + jb.src_offset;
    const Pix *pred = static_cast<const Pix *>(p.d.pred) + jb.pred_offset;
    const int8_t *fsh = c_fwd_shift[TS];
    const int bit_col = c_fwd_cos_col[ilog2c(W) - 2][ilog2c(H) - 2], bit_row = c_fwd_cos_row[ilog2c(W) - 2][ilog2c(H) - 2];

    // residual (svt_residual_kernel8bit / 16bit): int16 arithmetic as in the reference
    // runs of RUN samples per (unaligned) vector load: the planes' offsets and strides are the caller's
    constexpr int RUN = W < 8 ? W : 8, RPR = W / RUN; // run length, runs per row
    typedef Pix __attribute__((ext_vector_type(RUN), aligned(sizeof(Pix)))) RunU;
    // A lane's runs lie RSTEP rows apart in one column of runs (i = l + it * LW, LW a multiple of RPR): run `it` of a plane is the lane's first run
    // plus it * RSTEP * stride samples, a wave-uniform distance
    static_assert(LW % RPR == 0, "a lane's runs share their column");
    constexpr int RSTEP = LW / RPR;
    constexpr bool kRunBase = rd_run_base(TS), kDpp = rd_dpp_reduce(TS);
    auto first_run = [&](const Pix *plane, uint32_t stride, int lx) { return plane + (size_t)(lx / RPR) * stride + (lx % RPR) * RUN; };
    auto run_at = [&](bool by_base, const Pix *plane, const Pix *first, uint32_t stride, int it, int r, int c) {
        return reinterpret_cast<const RunU *>(by_base ? first + (size_t)(it * RSTEP) * stride : plane + (size_t)r * stride + c);
    };
    uint32_t rmax = 0; // largest |residual| this lane produced
    {
        HiLo rhl;
        const Pix *src0 = first_run(src, p.d.src_stride, l), *pred0 = first_run(pred, p.d.pred_stride, l);
        // a lane's runs are fetched kResidualAhead at a time, all of a group in flight before the first is used (the loop's trip count depends
        // on the lane: left to itself every run is a round trip of its own)
        constexpr int NIT = (RPR * H + LW - 1) / LW, kResidualAhead = NIT < SVT_RD_RESIDUAL_AHEAD ? NIT : SVT_RD_RESIDUAL_AHEAD;
        for (int it0 = 0; it0 < NIT; it0 += kResidualAhead) {
            RunU sv[kResidualAhead], pv[kResidualAhead];
#pragma unroll
            for (int j = 0; j < kResidualAhead; j++) {
                const int i = l + (it0 + j) * LW;
                if (it0 + j < NIT && i < RPR * H) {
                    const int r = i / RPR, c = (i - r * RPR) * RUN;
                    sv[j] = *run_at(kRunBase, src, src0, p.d.src_stride, it0 + j, r, c);
                    pv[j] = *run_at(kRunBase, pred, pred0, p.d.pred_stride, it0 + j, r, c);
                }
            }
#pragma unroll
            for (int j = 0; j < kResidualAhead; j++) {
                const int i = l + (it0 + j) * LW;
                if (it0 + j < NIT && i < RPR * H) {
                    const int r = i / RPR, c = (i - r * RPR) * RUN;
                    static_assert(RUN % 2 == 0, "the extremes are taken per pair of samples");
#pragma unroll
                    for (int k = 0; k < RUN; k += 2) {
                        const int32_t d0 = (int16_t)((int16_t)sv[j][k] - (int16_t)pv[j][k]), d1 = (int16_t)((int16_t)sv[j][k + 1] - (int16_t)pv[j][k + 1]);
                        A[r * PA + c + k]     = d0;
                        A[r * PA + c + k + 1] = d1;
#if SVT_RD_PAIR_RESIDUAL_MAX
                        rhl.take(d0, d1);
#else
                        rhl.take(d0);
                        rhl.take(d1);
#endif
                    }
                }
            }
        }
        rmax = rhl.max_abs();
    }
    // one answer for the wave (all its blocks): every residual small enough for the 24-bit multiplies of the forward passes?
    // one answer for the wave (all its blocks): small enough data for the three-instruction butterflies?  The column pass sees the residual
    // shifted up by fsh[0] (0 or 2)
    const bool fast_col = pass_fits_17_bits(rd_wave_max<kDpp>(rmax) << (fsh[0] > 0 ? fsh[0] : 0), H);
    __syncthreads();
    // forward columns (av1_tranform_two_d_core_c, transforms.c:2287-2308)
    uint32_t cmax = 0; // largest |column output| of this lane
    if (l < W) {
        int32_t x[H];
#pragma unroll
        for (int r = 0; r < H; r++) x[r] = A[(ud ? H - 1 - r : r) * PA + l];
        shift_vec<H>(x, fsh[0]);
        // the shifted values are all the passes below may start from: left to itself the compiler forms the identity pass's x << 4 from the unshifted
        // samples and keeps both sets alive across the type switch, which the 32-lane layouts (at their 128-register limit) pay for in scratch
        if constexpr (kBtf == 2) {
#pragma unroll
            for (int r = 0; r < H; r++) x[r] = held_in_vgpr(x[r]);
        }
        if (fast_col) fwd_1d_bounded<H, kShift32, kBtf>(x, vt, bit_col, fsh[1]); else { fwd_1d<H, 0>(x, vt, bit_col); shift_vec<H>(x, fsh[1]); } // wave-uniform
        const int oc = lr ? W - 1 - l : l;
#pragma unroll
        for (int r = 0; r < H; r++) A[r * PA + oc] = x[r];
        cmax = vec_max_abs<H>(x);
    }
    const bool fast_row = pass_fits_17_bits(rd_wave_max<kDpp>(cmax), W); // the row pass's input
    __syncthreads();
    // forward rows (:2310-2323)
    uint32_t comax = 0; // largest |coefficient| of this lane
    if (l < H) {
        int32_t x[W];
#pragma unroll
        for (int c = 0; c < W; c++) x[c] = A[l * PA + c];
        if (fast_row) fwd_1d_bounded<W, kShift32, kBtf>(x, ht, bit_row, fsh[2]); else { fwd_1d<W, 0>(x, ht, bit_row); shift_vec<W>(x, fsh[2]); }
        if constexpr (RECT) {
#pragma unroll
            for (int c = 0; c < W; c++) x[c] = rshift64((i64)x[c] * 5793, 12);
        }
#pragma unroll
        for (int c = 0; c < W; c++) A[l * PA + c] = x[c];
        comax = vec_max_abs<W>(x);
    }
    // coefficients below 2^16 in every block of the wave: the quantizer's products fit 24-bit multiplies (see the loop below)
    const uint32_t comax_w = rd_wave_max<kDpp>(comax);
    const bool q24 = comax_w < (1u << 16);
    __syncthreads();
    // 64-point sizes keep the top-left 32x32 (svt_handle_transform*_c, transforms.c:2374-2505)
    // partial-frequency shapes (av1_estimate_transform_N2 / _N4 / _ONLY_DC, transforms.c:2633-2948): the pruned 1-D kernels
    // of the reference produce the full transform's low-frequency outputs; everything else is zero and no energy is
    // attributed to the discarded frequencies (svt_handle_transform*_N2_N4_c, :2514-2543)
    const int pf = jb.pf_shape & 3;
    const int keep_w = pf == 3 ? 1 : (W >> pf), keep_h = pf == 3 ? 1 : (H >> pf);
    u64 tq = 0;
    if (pf == 0) if constexpr (W > 32 || H > 32) {
        for (int i = l; i < W * H; i += LW) {
            const int r = i / W, c = i - r * W;
            if (r >= HP || c >= WP) { const int32_t v = A[r * PA + c]; tq += (u64)((i64)v * v); }
        }
        // |coefficient| < 2^16 in the wave: a lane's 48 squares sum below 2^38.  The DPP form needs every lane of the wave here: `pf` is the
        // block's, and a 64-point size has one block per wave (LW == 64), so the branch above is taken by all lanes or by none
        static_assert(LW == 64, "one block per wave: pf is wave-uniform");
        tq = (kDpp && q24) ? group_sum64_dpp<LW, 38>(tq) : group_sum<LW>(tq);
    }
    if constexpr (W > 32 || H > 32) __syncthreads(); // the compaction below overwrites discarded coefficients
    // SATD, quantize, coefficient-domain distortion over the kept NP coefficients (packed index rc = r*WP + c).  The
    // dequantized value replaces the coefficient at the packed position r*PB + c <= r*PA + c: a later iteration never
    // reads what an earlier one overwrote (its reads start beyond the earlier iteration's writes), and within one
    // iteration the wave's loads precede its stores.
    const SvtHipQuantRow q = p.d.quant_rows[jb.quant_row];
    const int     log_scale = p.d.quant_kind == 2 ? 0 : c_log_scale[TS]; // quant_kind 2: the TPL dispenser's plain svt_av1_quantize_fp call (src_ops_process.c:225-249)
    const int16_t *iscan    = p.iscan[(tt >= 10) ? ((tt & 1) ? 2 : 1) : 0];
    const uint8_t *qm = (tt < 9) ? p.d.qmatrix : nullptr, *iqm = (tt < 9) ? p.d.iqmatrix : nullptr; // IS_2D_TRANSFORM, full_loop.c:1606-1608
    uint32_t satd = 0, eob = 0, qsum = 0; // qsum: sum of min(|qcoeff|, 63) = svt_av1_compute_cul_level's running sum up to its clamp
    int32_t  dc_q = 0;                    // lane 0 of a block: the quantized DC coefficient (rc == 0 is its first iteration)
    u64      dres = 0, dpred = 0;
    int32_t *co_out = (p.d.coeff && valid) ? p.d.coeff + (size_t)job * NP : nullptr;
    int32_t *q_out  = (p.d.qcoeff && valid) ? p.d.qcoeff + (size_t)job * NP : nullptr;
    int32_t *dq_out = (p.d.dqcoeff && valid) ? p.d.dqcoeff + (size_t)job * NP : nullptr;
    const int32_t zb_c[2]  = {log_scale ? ((q.zbin[0] + (1 << (log_scale - 1))) >> log_scale) : q.zbin[0], log_scale ? ((q.zbin[1] + (1 << (log_scale - 1))) >> log_scale) : q.zbin[1]};
    const int32_t rnd_c[2] = {log_scale ? ((q.round[0] + (1 << (log_scale - 1))) >> log_scale) : q.round[0], log_scale ? ((q.round[1] + (1 << (log_scale - 1))) >> log_scale) : q.round[1]};
    // The common case as a loop of its own: "b" quantizer, flat matrix, every coefficient of the wave below 2^16, the whole
    // block kept, nothing but the quantized coefficients asked for.  A lane's first coefficient may be the DC one (its constants are
    // selected per lane); all later ones are AC, whose constants stay in scalar registers.  Every product has 24-bit operands (see the
    // general loop below), |coeff - dqcoeff| <= max(|coeff|, dequant) < 2^16: the squares are exact in 32 bits.
    // Not always wave-uniform: in a partial last wave with coeff or dqcoeff requested, the lanes of the missing blocks (null co_out / dq_out)
    // take this loop while the wave's real blocks take the general one.  Both loops are exact and the missing blocks store nothing.
    const bool fast_q = q24 && !qm && p.d.quant_kind == 0 && !co_out && !dq_out && __all(pf == 0);
    // The same loop with unsigned 32-bit products, signs by multiplication, 32-bit distortion sums and unpredicated qcoeff stores, taken
    // when EVERY lane of the wave passes the tests below (wave-uniform; a partial last wave has null q_out lanes and keeps the loop below).
    //   t = |coeff| + round (8 bits: clamped to 32767) <= tmax = comax_w + max(round) (8 bits: min(.., 32767)), round >= 0.
    //   The reference's tmp = ((32 t * quant) >> 16) + 32 t equals floor(t * Q / 2^11) with Q = quant + 65536 in [2^15, 2^17) for any int16
    //   quant (the shift is arithmetic, so the identity holds for negative quant as well).  tmax < 2^(18 - KT) <= 2^15 gives t * Q < 2^32:
    //   one v_mul_u32_u24, and tmp < 2^(24 - KT).
    //   qv = (tmp * S) >> (21 - LS) is bits 32.. of (tmp << KT) * (S << (11 + LS - KT)); with 0 <= S < 2^15 (int16) and 11 + LS - KT <= 9
    //   both factors are below 2^24 and the product below 2^48: one v_mul_hi_u32_u24.  KT = 3, or 4 at log-scale 2 (where S << 10 would not fit).
    //   Signs: sg = +-1, |coeff| = coeff * sg, qcoeff = qv * sg; at log-scale 0 dqcoeff = qcoeff * dequant, else the shift stays on the magnitude.
    //   Distortions: |coeff - dqcoeff| = |a - dq| <= max(a, dq) <= M = max(comax_w, dqmax), where dqmax is the quantizer applied to tmax with the
    //   lane's larger quant, quant_shift and dequant (every step is monotonic in each of them, all >= 0).  (NP / LW) * M^2 < 2^32: a lane's
    //   NP / LW squares sum without overflow in 32 bits, one v_mad_*24 each; M < 2^16 keeps dq * sg and qv * dequant within 24 x 24 -> 32 bits.
    constexpr int LS = tx_log_scale(TS), KT = LS == 2 ? 4 : 3;
    bool lane_lean = fast_q && q_out != nullptr && log_scale == LS;
    // M bounds every |dqcoeff| of the lane's block, and with the rectangular sizes' 2896 / 4096 scaling every input of its inverse row pass:
    // where that passes the clamp-free test in every lane of a lean wave, the row pass's tier is known without a look at its input
    bool lane_row_free = false;
    {
        const int32_t  rndm = rnd_c[0] > rnd_c[1] ? rnd_c[0] : rnd_c[1], sm = q.quant_shift[0] > q.quant_shift[1] ? q.quant_shift[0] : q.quant_shift[1];
        const int32_t  dm = q.dequant[0] > q.dequant[1] ? q.dequant[0] : q.dequant[1], qm2 = (q.quant[0] > q.quant[1] ? q.quant[0] : q.quant[1]) + 65536;
        const bool     nonneg = (rnd_c[0] | rnd_c[1] | q.quant_shift[0] | q.quant_shift[1] | q.dequant[0] | q.dequant[1]) >= 0;
        uint32_t       tmax = comax_w + (uint32_t)(nonneg ? rndm : 0);
        if (BD == 8) tmax = tmax > 32767u ? 32767u : tmax;
        const u64 qvmax = ((((u64)tmax * (uint32_t)qm2) >> 11) * (u64)(uint32_t)(nonneg ? sm : 0)) >> (21 - LS);
        const u64 dqmax = (qvmax * (u64)(uint32_t)(nonneg ? dm : 0)) >> LS;
        const u64 M = dqmax > comax_w ? dqmax : (u64)comax_w;
        lane_lean = lane_lean && nonneg && tmax < (1u << (18 - KT)) && M < (1u << 16) && M * M * (NP / LW) < (1ull << 32);
        if constexpr (kFree && SVT_RD_ROW_BOUND_FROM_QUANT)
            lane_row_free = lane_lean && ipass_clamp_free((uint32_t)(RECT ? (M * 2896 + 2048) >> 12 : M), W, ROW_CLAMP); // M < 2^16 behind lane_lean
    }
    const bool lean_q = __all(lane_lean);
    const bool row_free_q = kFree && SVT_RD_ROW_BOUND_FROM_QUANT && __all(lane_row_free); // implies lean_q
    if (lean_q) {
        static_assert(NP % LW == 0, "every lane of a block walks the same number of coefficients");
        constexpr int kScanAhead = NP / LW < SVT_RD_SCAN_AHEAD ? ((NP / LW) & ~1) : SVT_RD_SCAN_AHEAD; // as in the loop below
        static_assert(kScanAhead >= 2 && kScanAhead % 2 == 0 && NP / LW >= kScanAhead, "ahead of the loop");
        uint32_t scan2[kScanAhead / 2];
#pragma unroll
        for (int k = 0; k < kScanAhead; k += 2) scan2[k / 2] = (uint32_t)(uint16_t)iscan[l + LW * k] | ((uint32_t)(uint16_t)iscan[l + LW * (k + 1)] << 16);
        uint32_t dres32 = 0, dpred32 = 0;
        int32_t  last = -1; // largest scan position of a non-zero level
        // |coeff| itself is never formed: t = coeff * sg + round, the zero-bin test is t >= zbin + round (zbr), SATD is the sum of the t less the
        // rounds added (below), coeff^2 and (coeff - dqcoeff)^2 take the signed values.  The cul_level sum is clamped once: min(sum of
        // min(|q|, 63), 63) == min(sum of |q|, 63), and the sum of a wave's |q| < 2^16 fits 32 bits.
        auto one = [&](int rc, int32_t zbr, int32_t rnd, uint32_t qq, uint32_t qshift, int32_t deq, int ahead = -1) {
            const int r = rc / WP, c = rc - r * WP; // WP is a power of two
            const int32_t co = A[r * PA + c], sg = (co >> 31) | 1, tu = __mul24(co, sg) + rnd;
            satd += (uint32_t)tu;
            uint32_t t = (uint32_t)tu;
            if (BD == 8) t = t > 32767u ? 32767u : t;
            const uint32_t tmp = umul24_lo(t, qq) >> 11;
            uint32_t qv = umul24_hi(tmp << KT, qshift);
            qv = tu >= zbr ? qv : 0u;
            const int32_t qs = __mul24((int32_t)qv, sg);
            int32_t dqs;
            if constexpr (LS == 0) dqs = __mul24(qs, deq);
            else dqs = __mul24(__mul24((int32_t)qv, deq) >> LS, sg);
            const int32_t dd = co - dqs;
            int32_t e; // the scan position itself, -1 for a zero level: the + 1 is added once behind the loop
            if (ahead >= 0) e = qv ? (int32_t)((scan2[ahead >> 1] >> (16 * (ahead & 1))) & 0xFFFFu) : -1; // (compile-time `ahead`)
            else e = qv ? (int32_t)iscan[rc] : -1;
            last = e > last ? e : last;
            qsum += qv;
            dres32 += (uint32_t)__mul24(dd, dd);
            dpred32 += (uint32_t)__mul24(co, co);
            A[r * PB + c] = dqs;
            q_out[rc] = qs;
            return qs;
        };
        const int ac0 = l != 0;
        dc_q = one(l, zb_c[ac0] + rnd_c[ac0], rnd_c[ac0], (uint32_t)(q.quant[ac0] + 65536), (uint32_t)q.quant_shift[ac0] << (11 + LS - KT), q.dequant[ac0], 0);
        const int32_t  zb1 = zb_c[1] + rnd_c[1], rnd1 = rnd_c[1], deq1 = q.dequant[1];
        const uint32_t qq1 = (uint32_t)(q.quant[1] + 65536), qshift1 = (uint32_t)q.quant_shift[1] << (11 + LS - KT);
#pragma unroll
        for (int k = 1; k < kScanAhead; k++) one(l + LW * k, zb1, rnd1, qq1, qshift1, deq1, k);
        if constexpr (LW >= 32) {
            static_assert((NP / LW - kScanAhead) % 2 == 0, "pairs");
            for (int rc = l + kScanAhead * LW; rc < NP; rc += 2 * LW) {
                one(rc, zb1, rnd1, qq1, qshift1, deq1);
                one(rc + LW, zb1, rnd1, qq1, qshift1, deq1);
            }
        } else {
#pragma unroll 4
            for (int rc = l + kScanAhead * LW; rc < NP; rc += LW) one(rc, zb1, rnd1, qq1, qshift1, deq1);
        }
        satd -= (uint32_t)(rnd_c[ac0] + (NP / LW - 1) * rnd1);
        eob   = (uint32_t)(last + 1);
        if constexpr (kDpp) {
            // a lane's sums fit 32 bits (above), a block's need not: they are widened inside the reduction
            dres  = group_sum_wide_dpp<LW>(dres32);
            dpred = group_sum_wide_dpp<LW>(dpred32);
        } else {
            dres  = dres32;
            dpred = dpred32;
        }
    } else if (fast_q) {
        static_assert(NP % LW == 0, "every lane of a block walks the same number of coefficients");
        // The scan positions of a lane's first kScanAhead coefficients (the low frequencies: where the non-zero levels are) are fetched ahead,
        // unconditionally, two to a register.  A load behind the `qv != 0` branch waits with s_waitcnt vmcnt(0) -- which on this ISA also
        // waits for the coefficient STORES of the iterations before it: the loop stalled on store completion exactly where it has work.
        constexpr int kScanAhead = NP / LW < SVT_RD_SCAN_AHEAD ? ((NP / LW) & ~1) : SVT_RD_SCAN_AHEAD;
        static_assert(kScanAhead >= 2 && kScanAhead % 2 == 0 && NP / LW >= kScanAhead, "ahead of the loop");
        uint32_t scan2[kScanAhead / 2];
#pragma unroll
        for (int k = 0; k < kScanAhead; k += 2) scan2[k / 2] = (uint32_t)(uint16_t)iscan[l + LW * k] | ((uint32_t)(uint16_t)iscan[l + LW * (k + 1)] << 16);
        auto one = [&](int rc, int32_t zb, int32_t rnd, int32_t quant, int32_t qshift, int32_t deq, int ahead = -1) {
            const int r = rc / WP, c = rc - r * WP; // WP is a power of two
            const int32_t co = A[r * PA + c], sign = co >> 31, a = (co ^ sign) - sign;
            satd += (uint32_t)a;
            int32_t t = a + rnd;
            if (BD == 8) t = t > 32767 ? 32767 : t;
            const int32_t tmp = mul24_shr(t, quant, 11) + (t << 5);
            int32_t qv = mul24_shr(tmp, qshift, 21 - log_scale);
            qv = a >= zb ? qv : 0;
            const int32_t dq = __mul24(qv, deq) >> log_scale;
            const int32_t qs = (qv ^ sign) - sign, dqs = (dq ^ sign) - sign;
            uint32_t e;
            if (ahead >= 0) e = qv ? ((scan2[ahead >> 1] >> (16 * (ahead & 1))) & 0xFFFFu) + 1u : 0u; // (compile-time `ahead`)
            else e = qv ? (uint32_t)iscan[rc] + 1u : 0u;
            eob = e > eob ? e : eob;
            qsum += (uint32_t)(qv > 63 ? 63 : qv);
            const int32_t dd = a - dq; // == |coeff - dqcoeff|: both carry the coefficient's sign
            dres += (u64)(uint32_t)__mul24(dd, dd);
            dpred += (u64)(uint32_t)__umul24((uint32_t)a, (uint32_t)a);
            A[r * PB + c] = dqs;
            if (q_out) q_out[rc] = qs;
            return qs;
        };
        const int ac0 = l != 0;
        dc_q = one(l, zb_c[ac0], rnd_c[ac0], q.quant[ac0], q.quant_shift[ac0], q.dequant[ac0], 0);
        const int32_t zb1 = zb_c[1], rnd1 = rnd_c[1], quant1 = q.quant[1], qshift1 = q.quant_shift[1], deq1 = q.dequant[1];
#pragma unroll
        for (int k = 1; k < kScanAhead; k++) one(l + LW * k, zb1, rnd1, quant1, qshift1, deq1, k);
        if constexpr (LW >= 32) {
            // two coefficients per trip: two independent chains for the scheduler.
            // Measured 64x64 0.718 -> 0.707 ms, 32x32 0.623 -> 0.611; at 16x16 the two extra registers cross an occupancy step (0.540 -> 0.564).
            static_assert((NP / LW - kScanAhead) % 2 == 0, "pairs");
            for (int rc = l + kScanAhead * LW; rc < NP; rc += 2 * LW) {
                one(rc, zb1, rnd1, quant1, qshift1, deq1);
                one(rc + LW, zb1, rnd1, quant1, qshift1, deq1);
            }
        } else {
#pragma unroll 4
            for (int rc = l + kScanAhead * LW; rc < NP; rc += LW) one(rc, zb1, rnd1, quant1, qshift1, deq1);
        }
    } else
    for (int rc = l; rc < NP; rc += LW) {
        const int r = rc / WP, c = rc - r * WP, ac = rc != 0;
        const bool kept = pf == 0 || (c < keep_w && r < keep_h);
        const int32_t co = kept ? A[r * PA + c] : 0, sign = co < 0 ? -1 : 0, a = (co ^ sign) - sign;
        satd += (uint32_t)a;
        int32_t qv = 0, dq = 0;
        const int32_t wt = qm ? qm[rc] : 32, iwt = qm ? iqm[rc] : 32; // AOM_QM_BITS = 5
        if (q24 && !qm) { // either quantizer with the flat matrix while |coeff| < 2^16 (wave-uniform): every product has 24-bit operands
            // "b": t = |coeff| + round < 2^17; (t << 5) * quant >> 16 == t * quant >> 11; tmp = that + (t << 5) lies in t * [16, 48) < 2^23
            if (p.d.quant_kind == 0) {
                if (a >= zb_c[ac]) {
                    int32_t t = a + rnd_c[ac];
                    if (BD == 8) t = t > 32767 ? 32767 : t;
                    const int32_t tmp = mul24_shr(t, q.quant[ac], 11) + (t << 5);
                    qv = mul24_shr(tmp, q.quant_shift[ac], 21 - log_scale);
                    dq = __mul24(qv, (int32_t)q.dequant[ac]) >> log_scale;
                }
            } else { // "fp": (|coeff| + round_fp) * quant_fp >> (16 - log_scale)
                const bool keep = (a << (1 + log_scale)) >= q.dequant[ac];
                if (keep) {
                    int32_t t = a + (log_scale ? ((q.round_fp[ac] + (1 << (log_scale - 1))) >> log_scale) : q.round_fp[ac]);
                    if (BD == 8) t = t < -32768 ? -32768 : (t > 32767 ? 32767 : t);
                    qv = mul24_shr(t, q.quant_fp[ac], 16 - log_scale);
                    dq = __mul24(qv, (int32_t)q.dequant[ac]) >> log_scale;
                }
            }
        } else if (p.d.quant_kind == 0 && !qm) { // the same "b" quantizer with the flat matrix (wt = iwt = 32), in 32-bit arithmetic:
            // |coeff| < 2^24 for any int16 residual (forward gain <= N per pass, minus the stage shifts), so (|coeff| + round) << 5
            // and its products' high parts fit 32 bits; every intermediate equals the reference's 64-bit value
            const int32_t zb = zb_c[ac];
            if (a >= zb) {
                int32_t t = a + rnd_c[ac];
                if (BD == 8) t = t > 32767 ? 32767 : t;
                const int32_t tw  = t << 5;
                const int32_t tmp = (int32_t)(((i64)tw * q.quant[ac]) >> 16) + tw;
                qv = (int32_t)(((i64)tmp * q.quant_shift[ac]) >> (16 - log_scale + 5));
                dq = (qv * (int32_t)q.dequant[ac]) >> log_scale;
            }
        } else if (p.d.quant_kind == 0) { // svt_aom_quantize_b_c_ii / svt_aom_highbd_quantize_b_c (full_loop.c:29-79,149-198)
            const int32_t zb = log_scale ? ((q.zbin[ac] + (1 << (log_scale - 1))) >> log_scale) : q.zbin[ac];
            if ((i64)a * wt >= ((i64)zb << 5)) {
                i64 t = (i64)a + (log_scale ? ((q.round[ac] + (1 << (log_scale - 1))) >> log_scale) : q.round[ac]);
                if (BD == 8) t = t < -32768 ? -32768 : (t > 32767 ? 32767 : t);
                t *= wt;
                qv = (int32_t)(((((t * q.quant[ac]) >> 16) + t) * q.quant_shift[ac]) >> (16 - log_scale + 5));
                const int32_t deq = ((int32_t)q.dequant[ac] * iwt + 16) >> 5;
                dq = (qv * deq) >> log_scale;
            }
        } else if (!qm) { // quantize_fp_helper_c / highbd_quantize_fp_helper_c without matrices (full_loop.c:282-343,387-452)
            const bool keep = (BD == 8) ? (((i64)a << (1 + log_scale)) >= (int32_t)q.dequant[ac]) : ((a << (1 + log_scale)) >= q.dequant[ac]);
            if (keep) {
                i64 t = (i64)a + (log_scale ? ((q.round_fp[ac] + (1 << (log_scale - 1))) >> log_scale) : q.round_fp[ac]);
                if (BD == 8) t = t < -32768 ? -32768 : (t > 32767 ? 32767 : t);
                qv = (int32_t)((t * q.quant_fp[ac]) >> (16 - log_scale));
                dq = (qv * (int32_t)q.dequant[ac]) >> log_scale;
            }
        } else { // the same helpers' matrix branch
            if ((i64)a * wt >= ((int32_t)q.dequant[ac] << (5 - (1 + log_scale)))) {
                i64 t = (i64)a + (log_scale ? ((q.round_fp[ac] + (1 << (log_scale - 1))) >> log_scale) : q.round_fp[ac]);
                if (BD == 8) t = t < -32768 ? -32768 : (t > 32767 ? 32767 : t);
                qv = (int32_t)((t * q.quant_fp[ac] * wt) >> (16 - log_scale + 5));
                const int32_t deq = ((int32_t)q.dequant[ac] * iwt + 16) >> 5;
                dq = (qv * deq) >> log_scale;
            }
        }
        const int32_t qs = (qv ^ sign) - sign, dqs = (dq ^ sign) - sign;
        if (qv) { const uint32_t e = (uint32_t)iscan[rc] + 1; eob = e > eob ? e : eob; }
        qsum += (uint32_t)(qv > 63 ? 63 : qv);
        if (rc == 0) dc_q = qs;
        const i64 dd = (i64)co - dqs;
        dres += (u64)(dd * dd);
        dpred += (u64)((i64)co * co);
        A[r * PB + c] = dqs; // packed dequantized coefficients feed the inverse transform
        if (co_out) co_out[rc] = co;
        if (q_out) q_out[rc] = qs;
        if (dq_out) dq_out[rc] = dqs;
    }
    if constexpr (kDpp) {
        // 32-bit sums (mod 2^32) and a maximum: the same values by either form; the 64-bit sums of the other two loops keep the butterfly
        satd = group_sum_dpp<LW>(satd);
        qsum = group_sum_dpp<LW>(qsum);
        eob  = group_max_dpp<LW>(eob);
        if (!lean_q) {
            dres  = group_sum<LW>(dres);
            dpred = group_sum<LW>(dpred);
        }
    } else {
        satd  = group_sum<LW>(satd);
        qsum  = group_sum<LW>(qsum);
        eob   = group_max<LW>(eob);
        dres  = group_sum<LW>(dres);
        dpred = group_sum<LW>(dpred);
    }
    __syncthreads();
    // inverse rows (inv_txfm2d_add_c, inv_transforms.c:2497-2511): discarded frequencies are zero
    int32_t xr[W];
    // The reference clamps the input of the row pass to bd + 8 bits and that of the column pass to 16.  Both magnitudes are taken of the RAW values:
    // a clamp only shrinks them, so the raw maximum bounds the clamped data in every test below, and the clamp itself runs only in a wave
    // whose raw maximum is outside its range (a wave-uniform branch; such a wave is never in the clamp-free tier).
    uint32_t irmax = 0; // largest |row-pass input| of this lane
    if (l < H) {
#pragma unroll
        for (int c = 0; c < W; c++) {
            int32_t v = (l < HP && c < WP) ? A[l * PB + c] : 0;
            if constexpr (RECT) v = rshift64((i64)v * 2896, 12);
            xr[c] = kSkipEntry ? v : clampv(v, BD + 8);
        }
        if (!row_free_q) irmax = vec_max_abs<W>(xr);
    }
    const uint32_t irmax_w = rd_wave_max<kDpp>(irmax); // wave-uniform, as everything decided from it
    const int irow_tier = row_free_q ? 2 : ipass_tier<kFree>(irmax_w, W, ROW_CLAMP);
    uint32_t icmax = 0; // largest |row-pass output|: the column pass's input
    if (l < H) {
        if (kSkipEntry && irmax_w >= (1u << (BD + 7))) {
#pragma unroll
            for (int c = 0; c < W; c++) xr[c] = clampv(xr[c], BD + 8);
        }
        if (irow_tier == 2) inv_1d_bounded<W, -1, kShift32, kFoldInv, kBtf>(xr, ht, c_inv_shift0[TS]);
        else if (irow_tier == 1) inv_1d_bounded<W, ROW_CLAMP, kShift32, kFoldInv, kBtf>(xr, ht, c_inv_shift0[TS]);
        else { inv_1d<W, ROW_CLAMP, 1>(xr, ht); shift_vec<W, kShift32>(xr, c_inv_shift0[TS]); }
#pragma unroll
        for (int c = 0; c < W; c++) A[l * PA + c] = xr[c];
        icmax = vec_max_abs<W>(xr);
    }
    const uint32_t icmax_w = rd_wave_max<kDpp>(icmax);
    const int icol_tier = ipass_tier<kFree>(icmax_w, H, COL_CLAMP);
#ifdef SVT_RD_TIER_STATS
    if (lane == 0) { atomicAdd(&g_rd_tier_stats[irow_tier * 3 + icol_tier], 1u); if (row_free_q) atomicAdd(&g_rd_tier_stats[9], 1u); }
#endif
    __syncthreads();
    // inverse columns + reconstruction + SSE (:2513-2534; svt_spatial_full_distortion_kernel / 16-bit variant)
    u64 sse = 0;
    if (l < W) {
        int32_t x[H];
        const int ic = lr ? W - 1 - l : l;
        constexpr int kColIn = BD + 6 > 16 ? BD + 6 : 16;
#pragma unroll
        for (int r = 0; r < H; r++) x[r] = (r < HP) ? (kSkipEntry ? A[r * PA + ic] : clampv(A[r * PA + ic], kColIn)) : 0; // rows >= 32 of a 64-row block are exactly zero after the row pass: constants, so the network prunes itself
        if (kSkipEntry && icmax_w >= (1u << (kColIn - 1))) {
#pragma unroll
            for (int r = 0; r < HP; r++) x[r] = clampv(x[r], kColIn);
        }
        if (icol_tier == 2) inv_1d_bounded<H, -1, kShift32, kFoldInv, kBtf>(x, vt, -4);
        else if (icol_tier == 1) inv_1d_bounded<H, COL_CLAMP, kShift32, kFoldInv, kBtf>(x, vt, -4);
        else { inv_1d<H, COL_CLAMP, 1>(x, vt); shift_vec<H, kShift32>(x, -4); }
        // residual (with the vertical flip undone) back to LDS, row-major: the reconstruction below moves whole runs
#pragma unroll
        for (int r = 0; r < H; r++) A[r * PA + l] = x[ud ? H - 1 - r : r];
    }
    __syncthreads();
    {
        Pix *rec = (p.d.recon && valid) ? static_cast<Pix *>(p.d.recon) + jb.pred_offset : nullptr;
        // the bases of the lane's first runs, formed anew from a lane index the compiler cannot tell from `l`, or it keeps the residual loop's
        // bases alive through the passes
        const int lb = kRunBase ? held_in_vgpr(l) : l;
        const Pix *src0 = first_run(src, p.d.src_stride, lb), *pred0 = first_run(pred, p.d.pred_stride, lb);
        // every run's prediction and source samples are requested BEFORE the first reconstruction run is stored: vector memory operations
        // complete in issue order on this ISA, so a load issued behind a store waits for the store's acknowledgement as well
        constexpr int NIT = (RPR * H + LW - 1) / LW; // runs per lane
        RunU pv[NIT], sv[NIT];
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int i = l + it * LW;
            if (i < RPR * H) {
                const int r = i / RPR, c = (i - r * RPR) * RUN;
                pv[it] = *run_at(kRunBase, pred, pred0, p.d.pred_stride, it, r, c);
                sv[it] = *run_at(kRunBase, src, src0, p.d.src_stride, it, r, c);
            }
        }
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int i = l + it * LW;
            if (i < RPR * H) {
                const int r = i / RPR, c = (i - r * RPR) * RUN;
                RunU out;
#pragma unroll
                for (int k = 0; k < RUN; k++) {
                    int v = (int)pv[it][k] + A[r * PA + c + k];
                    v = v < 0 ? 0 : (v > (1 << BD) - 1 ? (1 << BD) - 1 : v);
                    out[k] = (Pix)v;
                    const int e = (int)sv[it][k] - v;
                    sse += (u64)((uint32_t)e * (uint32_t)e); // |e| < 2^16: the low 32 bits of the (wrapping) product are the square, whatever the sign
                }
                if (rec) *const_cast<RunU *>(run_at(kRunBase, rec, rec + (pred0 - pred), p.d.pred_stride, it, r, c)) = out;
            }
        }
    }
    if constexpr (kDpp) sse = group_sum64_dpp<LW, 38>(sse); // a lane's W * H / LW <= 64 squares, each below 2^32
    else sse = group_sum<LW>(sse);
    if (l == 0 && valid) {
        p.d.eob[job]  = (uint16_t)eob;
        p.d.satd[job] = satd;
        p.d.dist_coeff[2 * (size_t)job]     = dres;
        p.d.dist_coeff[2 * (size_t)job + 1] = dpred;
        p.d.three_quad_energy[job] = tq;
        p.d.sse[job]  = sse;
        // svt_av1_compute_cul_level (full_loop.c:1449-1466): coefficients past eob are zero, so the sum over the scan equals the sum over
        // the block; set_dc_sign (:1338-1343)
        if (p.d.cul_level) p.d.cul_level[job] = (uint8_t)((qsum > 63 ? 63 : qsum) | (dc_q < 0 ? 64 : 0)) + (uint8_t)(dc_q > 0 ? 128 : 0);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Inverse transform + reconstruction alone (inv_txfm2d_add_c, inv_transforms.c:2459-2535; svt_av1_inv_txfm2d_add_{W}x{H}_c
// :2545-2716): the tail of rd_tx_kernel fed with caller-supplied dequantized coefficients (packed min(W,32) x min(H,32), as
// the reference's own inverse entries take them).  Same wave layout and LDS use as rd_tx_kernel.
// ---------------------------------------------------------------------------------------------------------
struct InvParams {
    SvtHipInvTxBatchDesc d;
};
template <int TS, int BD, typename Pix> __global__ void __launch_bounds__(64, rd_waves_per_simd(TS)) inv_tx_kernel(const InvParams p) {
    constexpr int W = tx_wide(TS), H = tx_high(TS), WP = W > 32 ? 32 : W, HP = H > 32 ? 32 : H, NP = WP * HP;
    constexpr int LW = rd_lanes_per_block(TS), BPW = rd_blocks_per_wave(TS);
    constexpr bool kShift32 = LW != 32, kFoldInv = LW != 32 || SVT_RD_FOLD_INV_32LANE;
    constexpr int kBtf = rd_bounded_btf(TS);
    constexpr bool kFree = rd_clamp_free_tier(TS), kSkipEntry = rd_skip_entry_clamps(TS);
    constexpr int PA = W + 1, PB = WP + 1;
    constexpr int ROW_CLAMP = BD == 8 ? 16 : 18, COL_CLAMP = 16;
    constexpr bool RECT = (W == 2 * H || H == 2 * W);
    __shared__ int32_t lds[BPW][H * PA];
    const int      lane = threadIdx.x, blk = lane / LW, l = lane % LW;
    const uint32_t job   = blockIdx.x * BPW + blk;
    const bool     valid = job < p.d.n_jobs;
    int32_t *A = lds[blk];
    const SvtHipTxJob jb = p.d.jobs[valid ? job : 0];
    const int tt = jb.tx_type & 15, vt = c_vtx[tt], ht = c_htx[tt];
    const bool ud = (vt == 2), lr = (ht == 2);
    const Pix *pred = static_cast<const Pix *>(p.d.pred) + jb.pred_offset;
    const int32_t *dq = p.d.dqcoeff + (size_t)(valid ? job : 0) * NP;
    for (int rc = l; rc < NP; rc += LW) { const int r = rc / WP, c = rc - r * WP; A[r * PB + c] = dq[rc]; }
    __syncthreads();
    int32_t xr[W];
    uint32_t irmax = 0; // largest |row-pass input| of this lane
    if (l < H) { // inverse rows (:2497-2511)
#pragma unroll
        for (int c = 0; c < W; c++) {
            int32_t v = (l < HP && c < WP) ? A[l * PB + c] : 0;
            if constexpr (RECT) v = rshift64((i64)v * 2896, 12);
            xr[c] = kSkipEntry ? v : clampv(v, BD + 8); // magnitudes of the raw values, clamps where a wave needs them: as in rd_tx_kernel
        }
        irmax = vec_max_abs<W>(xr);
    }
    const uint32_t irmax_w = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max(irmax)); // wave-uniform
    const int irow_tier = ipass_tier<kFree>(irmax_w, W, ROW_CLAMP);
    uint32_t icmax = 0; // largest |row-pass output|: the column pass's input
    if (l < H) {
        if (kSkipEntry && irmax_w >= (1u << (BD + 7))) {
#pragma unroll
            for (int c = 0; c < W; c++) xr[c] = clampv(xr[c], BD + 8);
        }
        if (irow_tier == 2) inv_1d_bounded<W, -1, kShift32, kFoldInv, kBtf>(xr, ht, c_inv_shift0[TS]);
        else if (irow_tier == 1) inv_1d_bounded<W, ROW_CLAMP, kShift32, kFoldInv, kBtf>(xr, ht, c_inv_shift0[TS]);
        else { inv_1d<W, ROW_CLAMP, 1>(xr, ht); shift_vec<W, kShift32>(xr, c_inv_shift0[TS]); }
#pragma unroll
        for (int c = 0; c < W; c++) A[l * PA + c] = xr[c];
        icmax = vec_max_abs<W>(xr);
    }
    const uint32_t icmax_w = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max(icmax));
    const int icol_tier = ipass_tier<kFree>(icmax_w, H, COL_CLAMP);
    __syncthreads();
    if (l < W) { // inverse columns (:2513-2534)
        int32_t x[H];
        const int ic = lr ? W - 1 - l : l;
        constexpr int kColIn = BD + 6 > 16 ? BD + 6 : 16;
#pragma unroll
        for (int r = 0; r < H; r++) x[r] = (r < HP) ? (kSkipEntry ? A[r * PA + ic] : clampv(A[r * PA + ic], kColIn)) : 0;
        if (kSkipEntry && icmax_w >= (1u << (kColIn - 1))) {
#pragma unroll
            for (int r = 0; r < HP; r++) x[r] = clampv(x[r], kColIn);
        }
        if (icol_tier == 2) inv_1d_bounded<H, -1, kShift32, kFoldInv, kBtf>(x, vt, -4);
        else if (icol_tier == 1) inv_1d_bounded<H, COL_CLAMP, kShift32, kFoldInv, kBtf>(x, vt, -4);
        else { inv_1d<H, COL_CLAMP, 1>(x, vt); shift_vec<H, kShift32>(x, -4); }
#pragma unroll
        for (int r = 0; r < H; r++) A[r * PA + l] = x[ud ? H - 1 - r : r];
    }
    __syncthreads();
    if (valid) {
        Pix *rec = static_cast<Pix *>(p.d.recon) + jb.src_offset;
        for (int i = l; i < W * H; i += LW) {
            const int r = i / W, c = i - r * W;
            int v = (int)pred[(size_t)r * p.d.pred_stride + c] + A[r * PA + c];
            v = v < 0 ? 0 : (v > (1 << BD) - 1 ? (1 << BD) - 1 : v);
            rec[(size_t)r * p.d.recon_stride + c] = (Pix)v;
        }
    }
}

template <int BD, typename Pix> void launch_inv(SvtHipContext *ctx, const InvParams &p) {
    const dim3 b(64);
#define CASE(S) case S: hipLaunchKernelGGL((inv_tx_kernel<S, BD, Pix>), dim3(ceil_div(p.d.n_jobs, rd_blocks_per_wave(S))), b, 0, ctx->stream, p); break;
    switch (p.d.tx_size) { // like launch_fwd and launch_size: no default, the entry's check let only these sizes through
        CASE(0) CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16) CASE(17) CASE(18)
    }
#undef CASE
}

// ---------------------------------------------------------------------------------------------------------
// Forward transform alone (av1_tranform_two_d_core_c, transforms.c:2259-2324; svt_av1_fwd_txfm2d_{W}x{H}{,_N2,_N4}_c): the
// head of rd_tx_kernel on a caller-supplied int16 residual, writing the FULL W x H coefficient array the per-size pointers
// return (the 64-point sizes included: packing to 32 x 32 is svt_handle_transform*'s job in the reference, :2374-2505).
// ---------------------------------------------------------------------------------------------------------
struct FwdParams {
    SvtHipFwdTxBatchDesc d;
};
template <int TS> __global__ void __launch_bounds__(64, rd_waves_per_simd(TS)) fwd_tx_kernel(const FwdParams p) {
    constexpr int W = tx_wide(TS), H = tx_high(TS);
    constexpr int LW = rd_lanes_per_block(TS), BPW = rd_blocks_per_wave(TS);
    constexpr int PA = W + 1;
    constexpr bool RECT = (W == 2 * H || H == 2 * W);
    __shared__ int32_t lds[BPW][H * PA];
    const int      lane = threadIdx.x, blk = lane / LW, l = lane % LW;
    const uint32_t job   = blockIdx.x * BPW + blk;
    const bool     valid = job < p.d.n_jobs;
    int32_t *A = lds[blk];
    const SvtHipTxJob jb = p.d.jobs[valid ? job : 0];
    const int tt = jb.tx_type & 15, vt = c_vtx[tt], ht = c_htx[tt];
    const bool ud = (vt == 2), lr = (ht == 2);
    const int16_t *res = p.d.residual + jb.src_offset;
    const int8_t *fsh = c_fwd_shift[TS];
    const int bit_col = c_fwd_cos_col[ilog2c(W) - 2][ilog2c(H) - 2], bit_row = c_fwd_cos_row[ilog2c(W) - 2][ilog2c(H) - 2];
    uint32_t rmax = 0;
    for (int i = l; i < W * H; i += LW) {
        const int r = i / W, c = i - r * W;
        const int32_t d = res[(size_t)r * p.d.residual_stride + c];
        A[r * PA + c] = d;
        rmax = max(rmax, (uint32_t)(d < 0 ? -d : d));
    }
    // one answer for the wave (all its blocks): small enough data for the three-instruction butterflies?  The column pass sees the residual
    // shifted up by fsh[0] (0 or 2)
    const bool fast_col = pass_fits_17_bits((uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max(rmax)) << (fsh[0] > 0 ? fsh[0] : 0), H); // see kFwdMul24MaxResidual
    __syncthreads();
    uint32_t cmax = 0;
    if (l < W) { // columns (:2287-2308)
        int32_t x[H];
#pragma unroll
        for (int r = 0; r < H; r++) x[r] = A[(ud ? H - 1 - r : r) * PA + l];
        shift_vec<H>(x, fsh[0]);
        if (fast_col) fwd_1d<H, 2>(x, vt, bit_col); else fwd_1d<H, 0>(x, vt, bit_col); // wave-uniform
        shift_vec<H>(x, fsh[1]);
        const int oc = lr ? W - 1 - l : l;
#pragma unroll
        for (int r = 0; r < H; r++) { A[r * PA + oc] = x[r]; cmax = max(cmax, (uint32_t)(x[r] < 0 ? -x[r] : x[r])); }
    }
    const bool fast_row = pass_fits_17_bits((uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max(cmax)), W); // the row pass's input
    __syncthreads();
    if (l < H) { // rows (:2310-2323)
        int32_t x[W];
#pragma unroll
        for (int c = 0; c < W; c++) x[c] = A[l * PA + c];
        if (fast_row) fwd_1d<W, 2>(x, ht, bit_row); else fwd_1d<W, 0>(x, ht, bit_row);
        shift_vec<W>(x, fsh[2]);
        if constexpr (RECT) {
#pragma unroll
            for (int c = 0; c < W; c++) x[c] = rshift64((i64)x[c] * 5793, 12);
        }
#pragma unroll
        for (int c = 0; c < W; c++) A[l * PA + c] = x[c];
    }
    __syncthreads();
    if (valid) { // the partial-frequency entries (_N2 / _N4, transforms.c:5202-5425,6769-6990) keep the top-left half / quarter and store zeros elsewhere
        const int pf = jb.pf_shape & 3;
        const int keep_w = pf == 3 ? 1 : (W >> pf), keep_h = pf == 3 ? 1 : (H >> pf);
        int32_t *out = p.d.coeff + (size_t)job * W * H;
        for (int i = l; i < W * H; i += LW) { const int r = i / W, c = i - r * W; out[i] = (c < keep_w && r < keep_h) ? A[r * PA + c] : 0; }
    }
}

void launch_fwd(SvtHipContext *ctx, const FwdParams &p) {
    const dim3 b(64);
#define CASE(S) case S: hipLaunchKernelGGL((fwd_tx_kernel<S>), dim3(ceil_div(p.d.n_jobs, rd_blocks_per_wave(S))), b, 0, ctx->stream, p); break;
    switch (p.d.tx_size) {
        CASE(0) CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16) CASE(17) CASE(18)
    }
#undef CASE
}

template <int BD> void launch_size(SvtHipContext *ctx, const RdParams &p) {
    const dim3 b(64);
#define CASE(S) case S: hipLaunchKernelGGL((rd_tx_kernel<S, BD>), dim3(ceil_div(p.d.n_jobs, rd_blocks_per_wave(S))), b, 0, ctx->stream, p); break;
    switch (p.tx_size) {
        CASE(0) CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16) CASE(17) CASE(18)
    }
#undef CASE
}

// host-side scan order generator (av1_scan_orders, Codec/coefficients.h:2197): diagonal scan for 2-D types and IDTX
// (zig-zag on square blocks, single-direction diagonals on rectangular ones), row scan for V_*, column scan for H_*
int scan_order(int tx_size, int tx_type, int16_t *scan, int16_t *iscan) {
    const int w = tx_wide(tx_size) > 32 ? 32 : tx_wide(tx_size), h = tx_high(tx_size) > 32 ? 32 : tx_high(tx_size), n = w * h;
    int k = 0;
    if (tx_type >= 10 && (tx_type & 1) == 0) { for (int i = 0; i < n; i++) scan[k++] = (int16_t)i; }
    else if (tx_type >= 11) { for (int c = 0; c < w; c++) for (int r = 0; r < h; r++) scan[k++] = (int16_t)(r * w + c); }
    else
        for (int d = 0; d < w + h - 1; d++) {
            const int down = (w < h) ? 1 : (w > h) ? 0 : (d & 1);
            for (int i = 0; i <= d; i++) { const int r = down ? i : d - i, c = d - r; if (r < h && c < w) scan[k++] = (int16_t)(r * w + c); }
        }
    for (int i = 0; i < n; i++) iscan[scan[i]] = (int16_t)i;
    return n;
}

} // namespace

extern "C" {

int svt_hip_tx_size_wide(int tx_size) { return (tx_size >= 0 && tx_size < 19) ? tx_wide(tx_size) : 0; }
int svt_hip_tx_size_high(int tx_size) { return (tx_size >= 0 && tx_size < 19) ? tx_high(tx_size) : 0; }

int svt_hip_scan_order(int tx_size, int tx_type, int16_t *scan, int16_t *iscan) {
    if (tx_size < 0 || tx_size >= 19 || tx_type < 0 || tx_type >= 16 || !scan || !iscan) return 0;
    return scan_order(tx_size, tx_type, scan, iscan);
}

static int rd_batch_check(const SvtHipRdBatchDesc *d) {
    if (d->n_jobs == 0) return SVT_HIP_OK; // like the transform, MD search, PME and statistics entries: an empty batch is accepted whatever else it holds
    if ((d->bit_depth != 8 && d->bit_depth != 10) || d->quant_kind > 2) BAD("bit_depth %u / quant_kind %u", d->bit_depth, d->quant_kind);
    if (!d->src || !d->pred || !d->jobs || !d->quant_rows || !d->eob || !d->satd || !d->dist_coeff || !d->three_quad_energy || !d->sse)
        BAD("a mandatory pointer of the RD batch is null");
    if ((d->qmatrix == nullptr) != (d->iqmatrix == nullptr)) BAD("qmatrix and iqmatrix go together");
    if (d->tx_size >= SVT_HIP_TX_SIZES_ALL) BAD("tx_size %d", d->tx_size);
    return SVT_HIP_OK;
}

int svt_hip_rd_batch(SvtHipContext *ctx, const SvtHipRdBatchDesc *d) {
    const int rc = enqueue_batch("svt_hip_rd_batch", ctx, d, rd_batch_check, &SvtHipRdBatchDesc::n_jobs, [=] {
        RdParams p = {*d, {}, d->tx_size};
        for (int k = 0; k < 3; k++) p.iscan[k] = ctx->iscan_dev + ((size_t)p.tx_size * 3 + k) * 1024;
        if (d->bit_depth == 8) launch_size<8>(ctx, p);
        else launch_size<10>(ctx, p);
    });
#ifdef SVT_RD_TIER_STATS
    unsigned int st[10] = {0}, zero[10] = {0};
    if (rc == SVT_HIP_OK && d->n_jobs && hipStreamSynchronize(ctx->stream) == hipSuccess &&
        hipMemcpyFromSymbol(st, HIP_SYMBOL(g_rd_tier_stats), sizeof(st)) == hipSuccess && hipMemcpyToSymbol(HIP_SYMBOL(g_rd_tier_stats), zero, sizeof(zero)) == hipSuccess)
        fprintf(stderr, "rd_tier_stats tx_size %d jobs %u  row x col (0 general, 1 bounded, 2 clamp-free): %u %u %u | %u %u %u | %u %u %u  row tier from the quantizer: %u\n",
                d->tx_size, d->n_jobs, st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7], st[8], st[9]);
#endif
    return rc;
}

} // extern "C"

// ---------------------------------------------------------------------------------------------------------
// Full-pel motion-compensated prediction from the ME results: for every 16x16 PU of every b64, copy the 16x16
// block of the reference plane displaced by that PU's best full-pel MV (MeContext.p_sb_best_mv layout as written
// by svt_hip_me_picture: [b64][list][ref][85], 16x16 PUs at n_idx 5..20 in quad-tree order).  Coordinates are
// clamped into the picture (edge replication).  This is the integer-MV case of inter prediction -- the only part
// of prediction this path needs to feed the RD kernels; sub-pel interpolation is out of scope.
// ---------------------------------------------------------------------------------------------------------
namespace {
// one workgroup per 64x64 block; a thread copies runs of 8 samples (one 8- or 16-byte store; the source run starts at an
// arbitrary sample, so its load is unaligned) and falls back to per-sample clamping where the run touches a picture edge
template <typename Pix> __device__ __forceinline__ void fullpel_pred_b64(const Pix *ref, uint32_t ref_stride, int width, int height, const uint32_t *sb_best_mv,
                                                                         int list, int ref_idx, uint32_t w64, int bx, int by, Pix *pred, uint32_t pred_stride,
                                                                         int vec_ok) {
    typedef Pix __attribute__((ext_vector_type(8), aligned(sizeof(Pix)))) RunU; // unaligned run of 8 samples
    typedef Pix __attribute__((ext_vector_type(8))) Run;
    const uint32_t b = (uint32_t)bx + (uint32_t)by * w64;
    const uint32_t *mvs = sb_best_mv + ((size_t)b * 8 + list * 4 + ref_idx) * 85 + 5; // the 16 16x16 PUs, quad-tree order
    for (int seg = threadIdx.x; seg < 64 * 8; seg += 256) {
        const int ly = seg >> 3, lx = (seg & 7) * 8, x = bx * 64 + lx, y = by * 64 + ly;
        if (x >= width || y >= height) continue;
        const int qx = lx >> 4, qy = ly >> 4;
        const uint32_t mv = mvs[(qx & 1) | ((qy & 1) << 1) | ((qx >> 1) << 2) | ((qy >> 1) << 3)];
        const int mvx = (int16_t)(mv & 0xFFFF), mvy = (int16_t)(mv >> 16);
        int sy = y + mvy;
        sy = sy < 0 ? 0 : (sy > height - 1 ? height - 1 : sy);
        const int sx = x + mvx;
        const Pix *srow = ref + (size_t)sy * ref_stride;
        Pix       *drow = pred + (size_t)y * pred_stride + x;
        if (vec_ok && sx >= 0 && sx + 8 <= width && x + 8 <= width) {
            *reinterpret_cast<Run *>(drow) = *reinterpret_cast<const RunU *>(srow + sx);
        } else {
            for (int i = 0; i < 8 && x + i < width; i++) {
                int cx = sx + i;
                cx = cx < 0 ? 0 : (cx > width - 1 ? width - 1 : cx);
                drow[i] = srow[cx];
            }
        }
    }
}

template <typename Pix> __global__ void __launch_bounds__(256) fullpel_pred_kernel(const Pix *ref, uint32_t ref_stride, int width, int height,
                                                                                   const uint32_t *sb_best_mv, int list, int ref_idx, uint32_t w64, int by64_first,
                                                                                   Pix *pred, uint32_t pred_stride, int vec_ok) {
    fullpel_pred_b64<Pix>(ref, ref_stride, width, height, sb_best_mv, list, ref_idx, w64, (int)blockIdx.x, by64_first + (int)blockIdx.y, pred, pred_stride, vec_ok);
}

// several pictures in one launch (blockIdx.z = picture): the per-picture launches of a row band are launch-bound
struct PredBatch {
    SvtHipPredJob job[SVT_HIP_PRED_MAX_JOBS];
};
template <typename Pix> __global__ void __launch_bounds__(256) fullpel_pred_batch_kernel(const PredBatch pb, uint32_t ref_stride, int width, int height, uint32_t w64,
                                                                                         uint32_t pred_stride, int vec_ok) {
    const SvtHipPredJob &j = pb.job[blockIdx.z];
    if (blockIdx.y >= j.b64_row_count) return;
    fullpel_pred_b64<Pix>(static_cast<const Pix *>(j.ref), ref_stride, width, height, j.sb_best_mv, j.list, j.ref_idx, w64, (int)blockIdx.x,
                          (int)(j.b64_row_start + blockIdx.y), static_cast<Pix *>(j.pred), pred_stride, vec_ok);
}
} // namespace

extern "C" int svt_hip_fullpel_pred(SvtHipContext *ctx, const void *ref, uint32_t ref_stride, uint32_t width, uint32_t height, uint8_t bit_depth,
                                    const uint32_t *sb_best_mv, uint8_t list, uint8_t ref_idx, uint32_t b64_row_start, uint32_t b64_row_count, void *pred,
                                    uint32_t pred_stride) {
    if (!ctx || !ref || !sb_best_mv || !pred || list > 1 || ref_idx > 3 || (bit_depth != 8 && bit_depth != 10) || !width || !height)
        return svt_hip_fail(ctx, SVT_HIP_ERR_BAD_PARAM, "svt_hip_fullpel_pred: bad argument");
    const uint32_t w64 = ceil_div(width, 64), h64 = ceil_div(height, 64);
    if (b64_row_start >= h64) return svt_hip_fail(ctx, SVT_HIP_ERR_BAD_PARAM, "svt_hip_fullpel_pred: b64_row_start %u >= %u", b64_row_start, h64);
    if (b64_row_count == 0 || b64_row_start + b64_row_count > h64) b64_row_count = h64 - b64_row_start;
    const dim3 g(w64, b64_row_count), blk(256);
    const size_t bpp = bit_depth == 8 ? 1 : 2;
    const int vec_ok = ((reinterpret_cast<uintptr_t>(pred) % (8 * bpp)) == 0 && pred_stride % 8 == 0) ? 1 : 0; // aligned 8-sample stores
    return enqueue_locked("svt_hip_fullpel_pred", ctx, [=] {
        if (bit_depth == 8)
            hipLaunchKernelGGL(fullpel_pred_kernel<uint8_t>, g, blk, 0, ctx->stream, static_cast<const uint8_t *>(ref), ref_stride, (int)width, (int)height,
                               sb_best_mv, (int)list, (int)ref_idx, w64, (int)b64_row_start, static_cast<uint8_t *>(pred), pred_stride, vec_ok);
        else
            hipLaunchKernelGGL(fullpel_pred_kernel<uint16_t>, g, blk, 0, ctx->stream, static_cast<const uint16_t *>(ref), ref_stride, (int)width, (int)height,
                               sb_best_mv, (int)list, (int)ref_idx, w64, (int)b64_row_start, static_cast<uint16_t *>(pred), pred_stride, vec_ok);
    });
}

extern "C" int svt_hip_fullpel_pred_batch(SvtHipContext *ctx, uint32_t ref_stride, uint32_t width, uint32_t height, uint8_t bit_depth, uint32_t pred_stride,
                                          uint32_t n_jobs, const SvtHipPredJob *jobs) {
    if (!ctx) return SVT_HIP_ERR_BAD_PARAM;
    if (!jobs || n_jobs == 0 || n_jobs > SVT_HIP_PRED_MAX_JOBS || (bit_depth != 8 && bit_depth != 10) || !width || !height)
        return svt_hip_fail(ctx, SVT_HIP_ERR_BAD_PARAM, "svt_hip_fullpel_pred_batch: bad argument (1..%d jobs)", SVT_HIP_PRED_MAX_JOBS);
    const uint32_t w64 = ceil_div(width, 64), h64 = ceil_div(height, 64);
    const size_t   bpp = bit_depth == 8 ? 1 : 2;
    PredBatch pb;
    memset(&pb, 0, sizeof(pb));
    uint32_t rows_max = 0;
    int      vec_ok   = pred_stride % 8 == 0;
    for (uint32_t i = 0; i < n_jobs; i++) {
        SvtHipPredJob j = jobs[i];
        if (!j.ref || !j.sb_best_mv || !j.pred || j.list > 1 || j.ref_idx > 3 || j.b64_row_start >= h64)
            return svt_hip_fail(ctx, SVT_HIP_ERR_BAD_PARAM, "svt_hip_fullpel_pred_batch: job %u: null pointer, list / ref_idx or b64_row_start %u out of range", i,
                                j.b64_row_start);
        if (j.b64_row_count == 0 || j.b64_row_start + j.b64_row_count > h64) j.b64_row_count = h64 - j.b64_row_start;
        rows_max = j.b64_row_count > rows_max ? j.b64_row_count : rows_max;
        vec_ok   = vec_ok && (reinterpret_cast<uintptr_t>(j.pred) % (8 * bpp)) == 0;
        pb.job[i] = j;
    }
    const dim3 g(w64, rows_max, n_jobs), blk(256);
    return enqueue_locked("svt_hip_fullpel_pred_batch", ctx, [&] {
        if (bit_depth == 8) hipLaunchKernelGGL(fullpel_pred_batch_kernel<uint8_t>, g, blk, 0, ctx->stream, pb, ref_stride, (int)width, (int)height, w64, pred_stride, vec_ok);
        else hipLaunchKernelGGL(fullpel_pred_batch_kernel<uint16_t>, g, blk, 0, ctx->stream, pb, ref_stride, (int)width, (int)height, w64, pred_stride, vec_ok);
    });
}

static int inv_txfm_check(const SvtHipInvTxBatchDesc *d) {
    if (d->n_jobs == 0) return SVT_HIP_OK;
    if ((d->bit_depth != 8 && d->bit_depth != 10) || (d->sample_bytes != 1 && d->sample_bytes != 2) || (d->bit_depth == 10 && d->sample_bytes != 2))
        BAD("inverse batch: bit_depth %u with %u-byte samples", d->bit_depth, d->sample_bytes);
    if (d->tx_size >= SVT_HIP_TX_SIZES_ALL) BAD("tx_size %u", d->tx_size);
    if (!d->pred || !d->recon || !d->jobs || !d->dqcoeff) BAD("a pointer of the inverse batch is null");
    return SVT_HIP_OK;
}

extern "C" int svt_hip_inv_txfm_batch(SvtHipContext *ctx, const SvtHipInvTxBatchDesc *d) {
    return enqueue_batch("svt_hip_inv_txfm_batch", ctx, d, inv_txfm_check, &SvtHipInvTxBatchDesc::n_jobs, [=] {
        const InvParams p = {*d};
        if (d->bit_depth == 10) launch_inv<10, uint16_t>(ctx, p);
        else if (d->sample_bytes == 1) launch_inv<8, uint8_t>(ctx, p);
        else launch_inv<8, uint16_t>(ctx, p);
    });
}

static int fwd_txfm_check(const SvtHipFwdTxBatchDesc *d) {
    if (d->n_jobs == 0) return SVT_HIP_OK;
    if (d->tx_size >= SVT_HIP_TX_SIZES_ALL) BAD("tx_size %u", d->tx_size);
    if (!d->residual || !d->jobs || !d->coeff) BAD("a pointer of the forward batch is null");
    return SVT_HIP_OK;
}

extern "C" int svt_hip_fwd_txfm_batch(SvtHipContext *ctx, const SvtHipFwdTxBatchDesc *d) {
    return enqueue_batch("svt_hip_fwd_txfm_batch", ctx, d, fwd_txfm_check, &SvtHipFwdTxBatchDesc::n_jobs, [=] { launch_fwd(ctx, FwdParams{*d}); });
}

// The cosine table (constant memory of this device's copy of the code object) and the inverse scan orders, made once per
// context at svt_hip_context_create: no lazily initialised process-global state (several threads, several GPUs per process).
int svt_hip_rd_tables_init(SvtHipContext *ctx) {
    SVT_HIP_CHECK(ctx, txfm_upload_cospi());
    const size_t bytes = sizeof(int16_t) * 19 * 3 * 1024;
    int16_t *tab = static_cast<int16_t *>(calloc(1, bytes)), scan[1024];
    if (!tab) return svt_hip_fail(ctx, SVT_HIP_ERR_NO_MEMORY, "iscan tables");
    for (int s = 0; s < 19; s++)
        for (int kind = 0; kind < 3; kind++) scan_order(s, kind == 0 ? 0 : (kind == 1 ? 10 : 11), scan, tab + ((size_t)s * 3 + kind) * 1024);
    int rc = SVT_HIP_OK;
    if (hipMalloc(reinterpret_cast<void **>(&ctx->iscan_dev), bytes) != hipSuccess) rc = svt_hip_fail(ctx, SVT_HIP_ERR_NO_MEMORY, "iscan tables");
    else if (hipMemcpy(ctx->iscan_dev, tab, bytes, hipMemcpyHostToDevice) != hipSuccess) rc = svt_hip_fail(ctx, SVT_HIP_ERR_LAUNCH, "iscan tables: copy failed");
    free(tab);
    return rc;
}

void svt_hip_rd_tables_free(SvtHipContext *ctx) {
    if (ctx->iscan_dev) (void)hipFree(ctx->iscan_dev); // teardown
    ctx->iscan_dev = nullptr;
}
