// txfm_core.h -- device code shared by the kernels that run the AV1 integer transforms (rd_kernel.hip, tpl_kernel.hip): the 1-D
// forward / inverse DCT, ADST and identity kernels of the reference, by structure, the shift / clamp helpers of the 2-D passes (the wave
// reductions: wave_ops.h; tx_wide / tx_high / ilog2c / tx_log_scale: tx_geom.h).  Each translation unit that includes it has its own copy of the constant tables; c_cospi is filled at context
// creation by txfm_upload_cospi() (svt_hip_rd_tables_init, svt_hip_tpl_tables_init).
#ifndef SVT_HIP_TXFM_CORE_H
#define SVT_HIP_TXFM_CORE_H
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "tx_geom.h"
#include "wave_ops.h"

namespace {

typedef unsigned long long u64;
typedef long long          i64;

__constant__ int32_t c_cospi[4][64]; // cospi_arr(bit), bit 10..13 (round(cos(j*pi/128) * 2^bit)), filled at init
// host: computes the table and fills the including translation unit's copy
inline hipError_t txfm_upload_cospi() {
    int32_t cosp[4][64];
    for (int b = 0; b < 4; b++)
        for (int j = 0; j < 64; j++) cosp[b][j] = (int32_t)(cos(3.14159265358979323846 * j / 128.0) * (double)(1 << (10 + b)) + 0.5);
    return hipMemcpyToSymbol(HIP_SYMBOL(c_cospi), cosp, sizeof(cosp));
}
// svt_aom_eb_av1_sinpi_arr_data rows for cos_bit 10..13 (Codec/inv_transforms.c:3228-3234)
__constant__ int32_t c_sinpi[4][5] = {{0, 330, 621, 836, 951}, {0, 660, 1241, 1672, 1901}, {0, 1321, 2482, 3344, 3803}, {0, 2642, 4964, 6689, 7606}};

struct TxGeom { uint8_t w, h; };
__host__ __device__ constexpr int brevc(int v, int bits) { int r = 0; for (int i = 0; i < bits; i++) r |= ((v >> i) & 1) << (bits - 1 - i); return r; }

// fwd_txfm_shift_ls (Codec/transforms.h:27-45), fwd_cos_bit_col/row (:47-50), inv shifts (Codec/inv_transforms.c:17-35),
// av1_get_tx_scale_tab (Codec/full_loop.h:53)
__device__ const int8_t  c_fwd_shift[19][3] = {{2, 0, 0},  {2, -1, 0}, {2, -2, 0}, {2, -4, 0}, {0, -2, -2}, {2, -1, 0}, {2, -1, 0}, {2, -2, 0}, {2, -2, 0}, {2, -4, 0},
                                               {2, -4, 0}, {0, -2, -2}, {2, -4, -2}, {2, -1, 0}, {2, -1, 0}, {2, -2, 0}, {2, -2, 0}, {0, -2, 0}, {2, -4, 0}};
__device__ const int8_t  c_fwd_cos_col[5][5] = {{13, 13, 13, 0, 0}, {13, 13, 13, 12, 0}, {13, 13, 13, 12, 13}, {0, 13, 13, 12, 13}, {0, 0, 13, 12, 13}};
__device__ const int8_t  c_fwd_cos_row[5][5] = {{13, 13, 12, 0, 0}, {13, 13, 13, 12, 0}, {13, 13, 12, 13, 12}, {0, 12, 13, 12, 11}, {0, 0, 12, 11, 10}};
__device__ const int8_t  c_inv_shift0[19]    = {0, -1, -2, -2, -2, 0, 0, -1, -1, -1, -1, -1, -1, -1, -1, -2, -2, -2, -2};
__device__ const uint8_t c_log_scale[19]     = {0, 0, 0, 1, 2, 0, 0, 0, 0, 1, 1, 2, 2, 0, 0, 0, 0, 1, 1};
// 1-D kernel of the column (vertical) / row (horizontal) pass per TxType: 0 DCT, 1 ADST, 2 FLIPADST, 3 identity (vtx_tab/htx_tab)
__device__ const uint8_t c_vtx[16] = {0, 1, 0, 1, 2, 0, 2, 1, 2, 3, 0, 3, 1, 3, 2, 3};
__device__ const uint8_t c_htx[16] = {0, 0, 1, 1, 0, 2, 2, 2, 1, 3, 3, 0, 3, 1, 3, 2};

// ((int64)a * b) >> sh (0 < sh < 32) for operands that fit 24 signed bits, low 32 bits of the result: three full-rate instructions
// (v_mul_i32_i24, v_mul_hi_i32_i24, v_alignbit_b32) instead of the quarter-rate 32 x 32 -> 64 multiply
__device__ __forceinline__ int32_t mul24_shr(int32_t a, int32_t b, int sh) {
    int32_t hi;
    asm("v_mul_hi_i32_i24 %0, %1, %2" : "=v"(hi) : "v"(a), "v"(b));
    return (int32_t)__builtin_amdgcn_alignbit((uint32_t)hi, (uint32_t)__mul24(a, b), (uint32_t)sh);
}
// low 32 bits / bits 32..47 of a * b for operands below 2^24: one full-rate instruction each (the compiler picks the quarter-rate v_mul_lo_u32
// for a masked product it cannot prove to be 24-bit)
__device__ __forceinline__ uint32_t umul24_lo(uint32_t a, uint32_t b) {
    uint32_t lo;
    asm("v_mul_u32_u24 %0, %1, %2" : "=v"(lo) : "v"(a), "v"(b));
    return lo;
}
__device__ __forceinline__ uint32_t umul24_hi(uint32_t a, uint32_t b) {
    uint32_t hi;
    asm("v_mul_hi_u32_u24 %0, %1, %2" : "=v"(hi) : "v"(a), "v"(b));
    return hi;
}
__device__ __forceinline__ int32_t rshift64(i64 v, int bit) { return (int32_t)((v + ((i64)1 << (bit - 1))) >> bit); }
// half_btf of the reference (Codec/transforms.h / inv_transforms.h): two 32-bit wrapping products, summed and rounded in
// 64 bits.  MUL == 1 (inverse transforms): both operands of every product fit 24 signed bits -- cos weights < 2^13, data
// < 2^19 behind the reference's own stage clamps (clamp_value to bd + 8 / 16..18 bits) -- so the full-rate v_mul_i32_i24
// returns the same low 32 bits as the quarter-rate v_mul_lo_u32.  Forward transforms keep the 32-bit multiply: their
// data range depends on the caller's samples.
// MUL == 2: the caller has bounded the data so that |a| + |b| < 2^18 (weights <= 2^13): neither product wraps and their sum with the rounding
// term stays below 2^31, so the whole butterfly is three full-rate 32-bit instructions with the reference's exact result (hbtf2 below).
#ifndef SVT_TX_FOLD_FWD
#define SVT_TX_FOLD_FWD 1 /* bounded forward passes: the round-shift behind the pass lives in the final butterflies (see fwd_1d) */
#endif
#ifndef SVT_TX_FOLD_INV
#define SVT_TX_FOLD_INV 1 /* bounded inverse DCT passes: the round-shift behind the pass lives in the last butterfly stage (see idct_core) */
#endif
// What the butterflies of one 1-D pass round with.  MUL 0 / 1 read `bit` alone.  The bounded butterflies (MUL == 2) add `rnd` = 2^(bit - 1), which
// the whole pass keeps in ONE VGPR (v_mad_i32_i24 takes the wave-uniform weight as its only scalar operand and no literal).  obit / ornd are
// what the butterflies that produce a forward pass's OUTPUTS use: the same, or with the pass's round-shift folded in (btf_folded).
struct Btf {
    int     bit;
    int32_t rnd;
    int     obit;
    int32_t ornd;
};
// a value the compiler has to keep in a vector register: it can neither fold it into an operand nor form it again at every use
__device__ __forceinline__ int32_t held_in_vgpr(int32_t v) {
    asm("" : "+v"(v));
    return v;
}
__device__ __forceinline__ Btf btf_plain(int bit) { return Btf{bit, 0, bit, 0}; } // MUL 0 / 1
__device__ __forceinline__ Btf btf_bounded(int bit) {
    const int32_t r = held_in_vgpr(1 << (bit - 1));
    return Btf{bit, r, bit, r};
}
// A bounded FORWARD pass followed by svt_av1_round_shift_array_c(.., s), s > 0.  Every output y of a forward DCT or ADST 8 / 16 is the result of
// a final half_btf, y = (S + 2^(bit-1)) >> bit with S = w0 a + w1 b, and floor of floor is floor:
//   (y + 2^(s-1)) >> s == (S + 2^(bit-1) + 2^(s-1+bit)) >> (bit + s).
// No overflow: the two weights are a cosine and a sine scaled by 2^bit <= 2^13, so |S| <= 2^13 sqrt(2) max(|a|, |b|) (+ 2^17 for the weights'
// own rounding), and under pass_fits_17_bits max(|a|, |b|) < 2^17: |S| < 1.42 * 2^30.  The rounding term is at most 2^12 + 2^16 (bit <= 13,
// s <= 4): the sum stays below 2^31.
__device__ __forceinline__ Btf btf_folded(int bit, int s) {
    const int32_t r = held_in_vgpr(1 << (bit - 1));
    if (s <= 0) return Btf{bit, r, bit, r};
    return Btf{bit, r, bit + s, held_in_vgpr((1 << (bit - 1)) + (1 << (s - 1 + bit)))};
}
// acc + w * a for 24-bit w and a, low 32 bits: one v_mad_i32_i24 with the weight as its scalar operand (c_cospi at a wave-uniform index).  Written
// out because the compiler re-associates the C++ form into two multiplies and a v_add3_u32, and, where the two weights are equal, into
// w * (a + b) with a quarter-rate v_mul_lo_u32 (it no longer knows the sum to be a 24-bit number).
__device__ __forceinline__ int32_t mad24_sv(int32_t w, int32_t a, int32_t acc) {
    int32_t r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "s"(w), "v"(a), "v"(acc));
    return r;
}
// the bounded butterfly: exactly two v_mad_i32_i24 and one shift.  An operand that is a literal zero (rows and columns >= 32 of the 64-point
// inverse passes) is seen on the C++ side, so that such a butterfly is one multiply-add or nothing and the dead half of the network still
// disappears: the asm statement itself is opaque to the optimizer.
__device__ __forceinline__ int32_t hbtf2(int32_t w0, int32_t a, int32_t w1, int32_t b, int32_t rnd, int bit) {
    bool za = false, zb = false; // (not const: a constant's initializer is folded by the front end, where nothing is known to be constant yet)
    if (__builtin_constant_p(a) && a == 0) za = true;
    if (__builtin_constant_p(b) && b == 0) zb = true;
    if (za && zb) return 0; // rnd < 2^bit
    int32_t acc = rnd;
    if (!za) acc = mad24_sv(w0, a, acc);
    if (!zb) acc = mad24_sv(w1, b, acc);
    return acc >> bit;
}
// MUL == 3: the same bound as MUL == 2 with the expression left to the compiler (two multiplies, a three-operand add, a shift; a quarter-rate
// multiply where the weights are equal).  For the layouts whose register allocation the opaque instructions cost scratch (see rd_tx_kernel).
template <int MUL> __device__ __forceinline__ int32_t hbtf(int32_t w0, int32_t a, int32_t w1, int32_t b, const Btf &P) {
    if constexpr (MUL == 2) return hbtf2(w0, a, w1, b, P.rnd, P.bit);
    const int bit = P.bit;
    if constexpr (MUL == 3) return (__mul24(w1, b) + (__mul24(w0, a) + (1 << (bit - 1)))) >> bit;
    i64 s;
    if constexpr (MUL == 1) s = (i64)__mul24(w0, a) + (i64)__mul24(w1, b);
    else s = (i64)(int32_t)((uint32_t)w0 * (uint32_t)a) + (i64)(int32_t)((uint32_t)w1 * (uint32_t)b);
    return (int32_t)((s + ((i64)1 << (bit - 1))) >> bit);
}
// a butterfly that produces an output of a forward pass
template <int MUL> __device__ __forceinline__ int32_t hbtf_out(int32_t w0, int32_t a, int32_t w1, int32_t b, const Btf &P) {
    if constexpr (MUL == 2) return hbtf2(w0, a, w1, b, P.ornd, P.obit);
    else return hbtf<MUL>(w0, a, w1, b, P);
}
// clamp_value of a SUM or DIFFERENCE inside an inverse pass.  The reference widens to 64 bits before it clamps; here the operands are at most
// 20-bit numbers -- the pass inputs are clamped to bd + 8 / 16 bits on entry, every butterfly output is clamped again, and a half_btf output is
// below sqrt(2) times its inputs -- so the 32-bit sum is the same number and the clamp is one v_med3_i32.
__device__ __forceinline__ int32_t clamp32(int32_t v, int bit) {
    const int32_t hi = (1 << (bit - 1)) - 1, lo = -(1 << (bit - 1));
    return v < lo ? lo : (v > hi ? hi : v);
}
__device__ __forceinline__ int32_t clampv(i64 v, int bit) {
    const i64 hi = ((i64)1 << (bit - 1)) - 1, lo = -((i64)1 << (bit - 1));
    return (int32_t)(v < lo ? lo : (v > hi ? hi : v));
}
__device__ __forceinline__ int32_t clampv(int32_t v, int bit) { return clamp32(v, bit); } // a 32-bit value against a range of at most 32 bits: the same number
__device__ __forceinline__ int32_t wadd(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
__device__ __forceinline__ int32_t wsub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }

// ---------------------------------------------------------------------------------------------------------
// DCT flow graph, by structure.  x[M..2M) is the odd part of a 2M-point DCT:
//   rotation stage k (k = 1..log2(M)-1): lanes in the middle half of every group of 2t (t = M >> k) are rotated
//     with their mirror image (3M-1-p); angle (1 + 4*brev(group)) * (64 >> k); symmetric 2x2 blocks, so the same
//     stage serves both directions;
//   butterfly stage k: groups of t, even groups sum-first, odd groups difference-first;
//   final stage: lane M+i with 2M-1-i, angle 64 - (2*brev(i)+1)*(32/M).
// CLAMP < 0: forward transform (no clamps); otherwise the reference's clamp_value(stage_range) of the inverse.
// ---------------------------------------------------------------------------------------------------------
template <int M, int K, int MUL> __device__ __forceinline__ void odd_rot(int32_t *x, const int32_t *c, const Btf &bit) {
    constexpr int t = M >> K;
    if constexpr (K == 1) {
#pragma unroll
        for (int j = 0; j < M / 4; j++) {
            const int p = M + M / 4 + j, m = 3 * M - 1 - p;
            const int32_t a = x[p], b = x[m];
            x[p] = hbtf<MUL>(-c[32], a, c[32], b, bit);
            x[m] = hbtf<MUL>(c[32], b, c[32], a, bit);
        }
    } else {
#pragma unroll
        for (int g = 0; g < (1 << (K - 2)); g++) {
            const int A = (1 + 4 * brevc(g, K - 2)) * (64 >> K), B = 64 - A, base = M + g * 2 * t;
#pragma unroll
            for (int j = 0; j < t / 2; j++) {
                const int p = base + t / 2 + j, m = 3 * M - 1 - p;
                const int32_t a = x[p], b = x[m];
                x[p] = hbtf<MUL>(-c[A], a, c[B], b, bit);
                x[m] = hbtf<MUL>(c[A], b, c[B], a, bit);
            }
#pragma unroll
            for (int j = 0; j < t / 2; j++) {
                const int p = base + t + j, m = 3 * M - 1 - p;
                const int32_t a = x[p], b = x[m];
                x[p] = hbtf<MUL>(-c[B], a, -c[A], b, bit);
                x[m] = hbtf<MUL>(c[B], b, -c[A], a, bit);
            }
        }
    }
}
template <int M, int K, int CLAMP> __device__ __forceinline__ void odd_bfly(int32_t *x) {
    constexpr int t = M >> K;
#pragma unroll
    for (int g = 0; g < M / t; g++) {
#pragma unroll
        for (int j = 0; j < t / 2; j++) {
            const int i0 = M + g * t + j, i1 = M + g * t + t - 1 - j;
            const int32_t lo = x[i0], hi = x[i1];
            int32_t s, d;
            if constexpr (CLAMP < 0) { s = wadd(lo, hi); d = (g & 1) ? wsub(hi, lo) : wsub(lo, hi); }
            else { s = clamp32(lo + hi, CLAMP); d = clamp32((g & 1) ? hi - lo : lo - hi, CLAMP); }
            x[i0] = (g & 1) ? d : s;
            x[i1] = (g & 1) ? s : d;
        }
    }
}
template <int M, bool INV, int MUL = INV ? 1 : 0> __device__ __forceinline__ void odd_final(int32_t *x, const int32_t *c, const Btf &bit) {
#pragma unroll
    for (int i = 0; i < M / 2; i++) {
        const int A = 64 - (2 * brevc(i, ilog2c(M)) + 1) * (32 / M), B = 64 - A, p = M + i, m = 2 * M - 1 - i;
        const int32_t a = x[p], b = x[m];
        if constexpr (!INV) { x[p] = hbtf_out<MUL>(c[A], a, c[B], b, bit); x[m] = hbtf_out<MUL>(c[A], b, -c[B], a, bit); } // outputs of the forward DCT
        else { x[p] = hbtf<MUL>(c[A], a, -c[B], b, bit); x[m] = hbtf<MUL>(c[B], a, c[A], b, bit); }
    }
}
template <int M, int K, int FM> struct OddFwd {
    static __device__ __forceinline__ void run(int32_t *x, const int32_t *c, const Btf &bit) {
        if constexpr (K < ilog2c(M)) {
            odd_rot<M, K, FM>(x, c, bit);
            odd_bfly<M, K, -1>(x);
            OddFwd<M, K + 1, FM>::run(x, c, bit);
        }
    }
};
template <int M, int K, int CLAMP, int IM> struct OddInv {
    static __device__ __forceinline__ void run(int32_t *x, const int32_t *c, const Btf &bit) {
        if constexpr (K >= 1) {
            odd_bfly<M, K, CLAMP>(x);
            odd_rot<M, K, IM>(x, c, bit);
            OddInv<M, K - 1, CLAMP, IM>::run(x, c, bit);
        }
    }
};
// FM (forward multiply mode): 0 = 32-bit wrapping products (any input), 1 = full-rate 24-bit multiplies -- exact whenever every node of the
// pass fits 24 signed bits, which the callers establish from the block's largest residual (see fwd_mul24_safe)
template <int N, int FM> __device__ __forceinline__ void fdct_core(int32_t *x, const int32_t *c, const Btf &bit) {
    if constexpr (N == 2) {
        const int32_t a = x[0], b = x[1];
        x[0] = hbtf_out<FM>(c[32], a, c[32], b, bit); // outputs of the forward DCT, as are odd_final's at every level of the recursion
        x[1] = hbtf_out<FM>(-c[32], b, c[32], a, bit);
    } else {
        constexpr int M = N / 2;
#pragma unroll
        for (int i = 0; i < M; i++) { const int32_t a = x[i], b = x[N - 1 - i]; x[i] = wadd(a, b); x[N - 1 - i] = wsub(a, b); }
        fdct_core<M, FM>(x, c, bit);
        OddFwd<M, 1, FM>::run(x, c, bit);
        odd_final<M, false, FM>(x, c, bit);
    }
}
// IM (inverse multiply mode): 1 = 24-bit products summed in 64 bits (any clamped input), 2 = the three-instruction butterflies, exact while
// every node of the pass is below 2^18 (weights <= 2^12): the callers measure the pass input
// out_s > 0 (the outermost call of a bounded pass): the pass is followed by svt_av1_round_shift_array_c(.., out_s), and the last stage does it.
// With r = 2^(out_s-1): (clamp(a +- b, lo, hi) + r) >> out_s == clamp(a + r +- b, lo + r, hi + r) >> out_s -- adding r commutes with the clamp --
// so t = a + r is shared by the pair: seven instructions for two outputs instead of eight.  |a|, |b| < 2^18 behind the stage clamps.
// CLAMP < 0: the caller has shown that no node of the pass leaves the reference's clamp range (ipass_clamp_free), so every clamp_value is the
// identity and none is computed: the sums and differences are plain, the folded last stage is t = a + r; (t +- b) >> out_s.
template <int N, int CLAMP, int IM> __device__ __forceinline__ void idct_core(int32_t *x, const int32_t *c, const Btf &bit, int out_s = 0) {
    if constexpr (N == 2) {
        const int32_t a = x[0], b = x[1];
        x[0] = hbtf<IM>(c[32], a, c[32], b, bit);
        x[1] = hbtf<IM>(c[32], a, -c[32], b, bit);
    } else {
        constexpr int M = N / 2;
        odd_final<M, true, IM>(x, c, bit);
        OddInv<M, ilog2c(M) - 1, CLAMP, IM>::run(x, c, bit);
        idct_core<M, CLAMP, IM>(x, c, bit);
#pragma unroll
        for (int i = 0; i < M; i++) {
            const int32_t a = x[i], b = x[N - 1 - i];
            if constexpr (CLAMP < 0) { // no node of the pass leaves the clamp range (ipass_clamp_free): every clamp is the identity
                if (out_s > 0) { const int32_t t = a + (1 << (out_s - 1)); x[i] = (t + b) >> out_s; x[N - 1 - i] = (t - b) >> out_s; }
                else { x[i] = a + b; x[N - 1 - i] = a - b; }
            } else if (out_s > 0) {
                const int32_t r = 1 << (out_s - 1), lo = -(1 << (CLAMP - 1)) + r, hi = (1 << (CLAMP - 1)) - 1 + r, t = a + r;
                x[i]         = max(min(t + b, hi), lo) >> out_s;
                x[N - 1 - i] = max(min(t - b, hi), lo) >> out_s;
            } else { x[i] = clamp32(a + b, CLAMP); x[N - 1 - i] = clamp32(a - b, CLAMP); }
        }
    }
}
template <int N> __device__ __forceinline__ void permute_brev(int32_t *x) { // out[k] = in[brev(k)]: an involution, swap pairs
#pragma unroll
    for (int k = 0; k < N; k++) {
        const int r = brevc(k, ilog2c(N));
        if (r > k) { const int32_t t = x[k]; x[k] = x[r]; x[r] = t; }
    }
}

// ---- ADST 8 / 16 (svt_av1_fadst8/16_new, iadst8/16_new) and ADST 4 ----
template <int N> __host__ __device__ constexpr int adst_perm(int k) { // P_N[2j] = P_{N/2}[j], P_N[2j+1] = N-1-P_{N/2}[j], P_2 = {0,1}
    if constexpr (N == 2) return k;
    else return (k & 1) ? N - 1 - adst_perm<N / 2>(k >> 1) : adst_perm<N / 2>(k >> 1);
}
template <int N, int HH, int MUL> __device__ __forceinline__ void adst_rot(int32_t *x, const int32_t *c, const Btf &bit) {
#pragma unroll
    for (int b = 0; b < N; b += 2 * HH) {
        if constexpr (HH == 2) {
            const int32_t a = x[b + 2], d = x[b + 3];
            x[b + 2] = hbtf<MUL>(c[32], a, c[32], d, bit);
            x[b + 3] = hbtf<MUL>(c[32], a, -c[32], d, bit);
        } else {
#pragma unroll
            for (int j = 0; j < HH / 4; j++) {
                const int A = (4 * j + 1) * (64 / HH), B = 64 - A, p = b + HH + 2 * j, q = b + HH + HH / 2 + 2 * j;
                int32_t a = x[p], d = x[p + 1];
                x[p]     = hbtf<MUL>(c[A], a, c[B], d, bit);
                x[p + 1] = hbtf<MUL>(c[B], a, -c[A], d, bit);
                a = x[q]; d = x[q + 1];
                x[q]     = hbtf<MUL>(-c[B], a, c[A], d, bit);
                x[q + 1] = hbtf<MUL>(c[A], a, c[B], d, bit);
            }
        }
    }
}
template <int N, int HH, int CLAMP> __device__ __forceinline__ void adst_bfly(int32_t *x) {
#pragma unroll
    for (int b = 0; b < N; b += 2 * HH)
#pragma unroll
        for (int j = 0; j < HH; j++) {
            const int32_t a = x[b + j], d = x[b + j + HH];
            if constexpr (CLAMP < 0) { x[b + j] = wadd(a, d); x[b + j + HH] = wsub(a, d); }
            else { x[b + j] = clamp32(a + d, CLAMP); x[b + j + HH] = clamp32(a - d, CLAMP); }
        }
}
template <int N, int MUL, bool OUT> __device__ __forceinline__ void adst_last(int32_t *x, const int32_t *c, const Btf &bit) { // OUT: the forward ADST's outputs
#pragma unroll
    for (int j = 0; j < N / 2; j++) {
        const int A = (4 * j + 1) * (64 / (2 * N)), B = 64 - A;
        const int32_t a = x[2 * j], d = x[2 * j + 1];
        if constexpr (OUT) { x[2 * j] = hbtf_out<MUL>(c[A], a, c[B], d, bit); x[2 * j + 1] = hbtf_out<MUL>(c[B], a, -c[A], d, bit); }
        else { x[2 * j] = hbtf<MUL>(c[A], a, c[B], d, bit); x[2 * j + 1] = hbtf<MUL>(c[B], a, -c[A], d, bit); }
    }
}
template <int N, int HH, int FM> struct AdstFwd {
    static __device__ __forceinline__ void run(int32_t *x, const int32_t *c, const Btf &bit) {
        if constexpr (HH < N) { adst_rot<N, HH, FM>(x, c, bit); adst_bfly<N, HH, -1>(x); AdstFwd<N, HH * 2, FM>::run(x, c, bit); }
    }
};
template <int N, int HH, int CLAMP, int IM> struct AdstInv {
    static __device__ __forceinline__ void run(int32_t *x, const int32_t *c, const Btf &bit) {
        if constexpr (HH >= 2) { adst_bfly<N, HH, CLAMP>(x); adst_rot<N, HH, IM>(x, c, bit); AdstInv<N, HH / 2, CLAMP, IM>::run(x, c, bit); }
    }
};
template <int N, int FM> __device__ __forceinline__ void fadst(int32_t *x, const int32_t *c, const Btf &bit) {
    int32_t y[N];
#pragma unroll
    for (int k = 0; k < N; k++) { const int32_t v = x[adst_perm<N>(k)]; y[k] = (__builtin_popcount(k) & 1) ? (int32_t)(0u - (uint32_t)v) : v; }
    AdstFwd<N, 2, FM>::run(y, c, bit);
    adst_last<N, FM, true>(y, c, bit);
#pragma unroll
    for (int j = 0; j < N / 2; j++) { x[2 * j] = y[2 * j + 1]; x[2 * j + 1] = y[N - 2 - 2 * j]; }
}
template <int N, int CLAMP, int IM> __device__ __forceinline__ void iadst(int32_t *x, const int32_t *c, const Btf &bit) {
    int32_t y[N];
#pragma unroll
    for (int j = 0; j < N / 2; j++) { y[2 * j + 1] = x[2 * j]; y[N - 2 - 2 * j] = x[2 * j + 1]; }
    adst_last<N, IM, false>(y, c, bit);
    AdstInv<N, N / 2, CLAMP, IM>::run(y, c, bit);
#pragma unroll
    for (int k = 0; k < N; k++) x[adst_perm<N>(k)] = (__builtin_popcount(k) & 1) ? (int32_t)(0u - (uint32_t)y[k]) : y[k];
}
#define MUL32(a, b) ((int32_t)((uint32_t)(a) * (uint32_t)(b)))
__device__ __forceinline__ void adst4(int32_t *x, int bit, bool inverse) { // transforms.c:1415-1503, inv_transforms.c:722-806
    const int32_t *s = c_sinpi[bit - 10];
    const int32_t x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3];
    if (!(x0 | x1 | x2 | x3)) return;
    if (!inverse) {
        const int32_t s7 = wsub(wadd(x0, x1), x3);
        const int32_t a0 = wadd(wadd(MUL32(s[1], x0), MUL32(s[2], x1)), MUL32(s[4], x3)), a1 = MUL32(s[3], s7);
        const int32_t a2 = wadd(wsub(MUL32(s[4], x0), MUL32(s[1], x1)), MUL32(s[2], x3)), a3 = MUL32(s[3], x2);
        x[0] = rshift64(wadd(a0, a3), bit); x[1] = rshift64(a1, bit); x[2] = rshift64(wsub(a2, a3), bit); x[3] = rshift64(wadd(wsub(a2, a0), a3), bit);
    } else {
        const int32_t s7 = wadd(wsub(x0, x2), x3);
        const int32_t a0 = wadd(wadd(MUL32(s[1], x0), MUL32(s[4], x2)), MUL32(s[2], x3));
        const int32_t a1 = wsub(wsub(MUL32(s[2], x0), MUL32(s[1], x2)), MUL32(s[4], x3)), a3 = MUL32(s[3], x1), a2 = MUL32(s[3], s7);
        x[0] = rshift64(wadd(a0, a3), bit); x[1] = rshift64(wadd(a1, a3), bit); x[2] = rshift64(a2, bit); x[3] = rshift64(wsub(wadd(a0, a1), a3), bit);
    }
}
template <int N> __device__ __forceinline__ void identity(int32_t *x) { // transforms.c:2205-2236, inv_transforms.c:2331-2363
#pragma unroll
    for (int i = 0; i < N; i++) {
        if constexpr (N == 4) x[i] = rshift64((i64)x[i] * 5793, 12);
        else if constexpr (N == 8) x[i] = (int32_t)((uint32_t)x[i] * 2u);
        else if constexpr (N == 16) x[i] = rshift64((i64)x[i] * 2 * 5793, 12);
        else if constexpr (N == 32) x[i] = (int32_t)((uint32_t)x[i] * 4u);
        else x[i] = rshift64((i64)x[i] * 4 * 5793, 12);
    }
}
// 1-D dispatch: type 0 DCT, 1/2 ADST (flips are applied by the 2-D passes), 3 identity.  Wave-uniform switch.
template <int N, int FM> __device__ __forceinline__ void fwd_1d(int32_t *x, int type, int bit) {
    const int32_t *c = c_cospi[bit - 10];
    const Btf P = FM == 2 ? btf_bounded(bit) : btf_plain(bit);
    if (type == 3) identity<N>(x);
    else if (type == 0) { fdct_core<N, FM>(x, c, P); permute_brev<N>(x); }
    else if constexpr (N == 4) adst4(x, bit, false);
    else if constexpr (N <= 16) fadst<N, FM>(x, c, P);
}
// A block's forward transform may use the 24-bit multiplies when |residual| <= 4095: a node of a 1-D pass is a sum of at most N inputs of that
// pass with weights of magnitude <= 1, so with the up-shift of at most 2 in front of the column pass and the down-shifts between the passes
// (fwd_txfm_shift_ls, transforms.h:27-45) no node of any of the 19 sizes exceeds 64 * 65,520 < 2^22; the cosine weights are < 2^14.  Any
// 8- / 10-bit picture satisfies it; samples outside the bit depth (the reference accepts any uint16) take the 32-bit path.
// The three-instruction butterflies (hbtf<2>) need every node of the pass below 2^17: N x the largest input of the pass (measured over the wave).
__device__ __forceinline__ bool pass_fits_17_bits(uint32_t wave_max_abs_input, int n) { return (unsigned long long)wave_max_abs_input * (unsigned)n < (1u << 17); }
template <int N, int CLAMP, int IM> __device__ __forceinline__ void inv_1d(int32_t *x, int type) {
    const int32_t *c = c_cospi[2]; // INV_COS_BIT = 12
    const Btf P = IM == 2 ? btf_bounded(12) : btf_plain(12);
    if (type == 3) identity<N>(x);
    else if (type == 0) { permute_brev<N>(x); idct_core<N, CLAMP, IM>(x, c, P); }
    else if constexpr (N == 4) adst4(x, 12, true);
    else if constexpr (N <= 16) iadst<N, CLAMP, IM>(x, c, P);
}
// every node of an inverse pass is a sum of at most N pass inputs with weights of magnitude <= 1 (the stage clamps only shrink it): below 2^18
// when N x the largest |input| is
__device__ __forceinline__ bool ipass_fits_18_bits(uint32_t wave_max_abs_input, int n) { return (unsigned long long)wave_max_abs_input * (unsigned)n < (1u << 18); }
// The clamp-free tier.  Every node of an n-point inverse pass (DCT, ADST 8 / 16) is a linear map of the pass inputs plus what the half_btfs
// upstream of it rounded: |node| <= G_n max|input| + e_n, with G_n the largest L1 norm of any node's weights (the 12-bit cosines taken as
// they are, the 64-point passes over their 32 live inputs) and e_n the largest accumulated rounding (each half_btf adds at most 1/2 and
// scales what its operands carry by its weights' magnitudes).  While that stays below 2^(clamp_bits - 1) every clamp_value of the pass
// is the identity, the butterflies' operands stay below 2^17, and the pass may run with CLAMP < 0.  tests/test_inv_clamp_bounds.py
// derives both tables from the flow graphs (G_n = 2.72, 5.28, 10.38, 20.57, 28.66; here in 64ths, rounded up) and checks them.
__host__ __device__ constexpr int inv_gain64(int n) { return n == 4 ? 175 : n == 8 ? 339 : n == 16 ? 665 : n == 32 ? 1317 : 1835; }
__host__ __device__ constexpr int inv_slack(int n) { return n == 4 ? 1 : n == 8 ? 6 : n == 16 ? 16 : n == 32 ? 24 : 63; }
__device__ __forceinline__ bool ipass_clamp_free(uint32_t wave_max_abs_input, int n, int clamp_bits) {
    return (u64)wave_max_abs_input * (unsigned)inv_gain64(n) + 64u * (unsigned)inv_slack(n) < ((u64)64 << (clamp_bits - 1));
}
// largest magnitude of a vector: the largest and the smallest element are tracked instead (one v_max3_i32 / v_min3_i32 per PAIR of elements
// each; |x| first would be two instructions per element before the max)
struct HiLo {
    int32_t hi = 0, lo = 0;
    __device__ __forceinline__ void take(int32_t a, int32_t b) { hi = max(max(hi, a), b); lo = min(min(lo, a), b); }
    __device__ __forceinline__ void take(int32_t a) { hi = max(hi, a); lo = min(lo, a); }
    __device__ __forceinline__ uint32_t max_abs() const { return max((uint32_t)hi, 0u - (uint32_t)lo); } // hi >= 0 >= lo; unsigned, so that INT32_MIN counts as 2^31
};
template <int N> __device__ __forceinline__ uint32_t vec_max_abs(const int32_t *x) {
    HiLo m;
    if constexpr (N % 2 == 0) {
#pragma unroll
        for (int i = 0; i < N; i += 2) m.take(x[i], x[i + 1]);
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) m.take(x[i]);
    }
    return m.max_abs();
}
// SAFE32: the caller knows |x| < 2^30 (a pass that took the bounded butterflies, or an inverse pass, whose outputs are clamped to <= 18 bits):
// the rounding add cannot wrap and the reference's 64-bit round_shift is the same two 32-bit instructions
template <int N, bool SAFE32 = false> __device__ __forceinline__ void shift_vec(int32_t *x, int sh) { // svt_av1_round_shift_array_c(x, N, -sh)
    if (sh < 0) {
#pragma unroll
        for (int i = 0; i < N; i++) x[i] = SAFE32 ? ((x[i] + (1 << (-sh - 1))) >> -sh) : rshift64(x[i], -sh);
    } else if (sh > 0) {
#pragma unroll
        for (int i = 0; i < N; i++) x[i] = (int32_t)((uint32_t)x[i] << sh);
    }
}

// the bounded pass (pass_fits_17_bits) together with the shift_vec<N, SAFE32>(x, sh) behind it, sh <= 0: the DCT and the ADST 8 / 16 round-shift
// in their final butterflies (btf_folded); identity and ADST4 keep the loop
template <int N, bool SAFE32, int BM = 2> __device__ __forceinline__ void fwd_1d_bounded(int32_t *x, int type, int bit, int sh) {
    if constexpr (BM != 2) {
        fwd_1d<N, BM>(x, type, bit);
        shift_vec<N, SAFE32>(x, sh);
        return;
    }
#if SVT_TX_FOLD_FWD
    const int32_t *c = c_cospi[bit - 10];
    const Btf P = btf_folded(bit, -sh);
    if (type == 3) { identity<N>(x); shift_vec<N, SAFE32>(x, sh); }
    else if (type == 0) { fdct_core<N, 2>(x, c, P); permute_brev<N>(x); }
    else if constexpr (N == 4) { adst4(x, bit, false); shift_vec<N, SAFE32>(x, sh); }
    else if constexpr (N <= 16) fadst<N, 2>(x, c, P);
#else
    fwd_1d<N, 2>(x, type, bit);
    shift_vec<N, SAFE32>(x, sh);
#endif
}
// the bounded inverse pass (ipass_fits_18_bits) together with the shift_vec<N, SAFE32>(x, sh) behind it, sh <= 0.  FOLD: the DCT round-shifts in its
// last butterfly stage (idct_core), in 32 bits whatever SAFE32 says (the stage's clamp bounds its operand); the inverse ADST ends in negations
// and keeps the loop, as do identity and ADST4.  With SAFE32 only passes that clamp to more than 16 bits fold (the row pass at 10 bits): a 16-bit
// clamp of a sum is the saturating v_add_i16 / v_sub_i16 itself, three instructions per output with the 32-bit shift loop against three and a
// half folded.  Without SAFE32 the loop is the 64-bit one, and every pass folds.
template <int N, int CLAMP, bool SAFE32, bool FOLD, int BM = 2> __device__ __forceinline__ void inv_1d_bounded(int32_t *x, int type, int sh) {
    const int32_t *c = c_cospi[2]; // INV_COS_BIT = 12
    if constexpr (BM != 2) {
        inv_1d<N, CLAMP, BM>(x, type);
        shift_vec<N, SAFE32>(x, sh);
        return;
    }
    if (type == 3) { identity<N>(x); shift_vec<N, SAFE32>(x, sh); }
    else if (type == 0) {
        permute_brev<N>(x);
        if constexpr (FOLD && SVT_TX_FOLD_INV && (CLAMP < 0 || CLAMP > 16 || !SAFE32)) idct_core<N, CLAMP, 2>(x, c, btf_bounded(12), -sh);
        else { idct_core<N, CLAMP, 2>(x, c, btf_bounded(12)); shift_vec<N, SAFE32>(x, sh); }
    } else {
        if constexpr (N == 4) adst4(x, 12, true);
        else if constexpr (N <= 16) iadst<N, CLAMP, 2>(x, c, btf_bounded(12));
        shift_vec<N, SAFE32>(x, sh);
    }
}

} // namespace
#endif
