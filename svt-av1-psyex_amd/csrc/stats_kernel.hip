// stats_kernel.hip -- batched block statistics on gfx950: SAD, SSE, variance and Hadamard SATD of (source - reference)
// blocks (svt_hip_block_stats_batch), and the stand-alone Hadamard kernel that shares hadamard_tile with them.
//
// Reference functions restated (Source/Lib):
//   svt_nxm_sad_kernel_helper_c / svt_aom_sad_16b_kernel_c          C_DEFAULT/compute_sad_c.c:20-56,209
//   svt_spatial_full_distortion_kernel_c / svt_full_distortion_kernel16_bits_c / svt_aom_sse_c / svt_aom_highbd_sse_c
//                                                                   C_DEFAULT/picture_operators_c.c:65-83, Codec/pic_operators.c:174-197,
//                                                                   Codec/enc_inter_prediction.c:559-583
//   svt_aom_variance{W}x{H}_c / svt_aom_variance_highbd_c           C_DEFAULT/variance.c:256-296
//   svt_aom_hadamard_{4x4,8x8,16x16,32x32}_c, svt_aom_satd_c        C_DEFAULT/picture_operators_c.c:176-326, Codec/common_dsp_rtcd.c:70-77
//   hadamard_path_c                                                 Codec/enc_mode_config.c:2151-2217
//
// One wave64 works through kJobsPerWave consecutive jobs (a wave per 8x8 block is launch-bound: 43k single-job waves of a 1080p picture
// took as long as 11k four-job waves).  Pixel statistics: a lane takes 4 neighbouring samples at a time (one 4- or 8-byte load per plane;
// 8-bit: v_sad_u8 and three v_dot4_u32_u8 give SAD, sum and sum of squares; 10-bit: packed 16-bit differences, v_sad_u16, v_dot2_i32_i16),
// lane sums reduced across the wave by DPP.  hadamard_path: <= 32x32 tiles staged in LDS; 16x16 / 32x32 tiles run their 8x8 cores on the matrix
// cores (exact in f16 operands) and the reference's truncating 16 / 32 combines on the VALU, 4x4 / 8x8 tiles are VALU butterflies with the
// reference's 16-bit intermediates.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "svt_hip_internal.h"
#include "batch_host.h"
#include "psy_energy.h"
#include "wave_ops.h"
#include "../../include/svt_hip_spy_rd.h"
#include "../../include/svt_hip_dsp.h"

namespace {

// ---- Hadamard building blocks (same operation order and intermediate widths as the reference) -----------------
__device__ __forceinline__ void had_col4(const int16_t *s, int st, int16_t *o) {
    const int16_t b0 = (int16_t)((s[0] + s[st]) >> 1), b1 = (int16_t)((s[0] - s[st]) >> 1);
    const int16_t b2 = (int16_t)((s[2 * st] + s[3 * st]) >> 1), b3 = (int16_t)((s[2 * st] - s[3 * st]) >> 1);
    o[0] = (int16_t)(b0 + b2);
    o[1] = (int16_t)(b1 + b3);
    o[2] = (int16_t)(b0 - b2);
    o[3] = (int16_t)(b1 - b3);
}
__device__ __forceinline__ void had_col8(const int16_t *s, int st, int16_t *o) {
    int16_t b[8], c[8];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        b[2 * i]     = (int16_t)(s[2 * i * st] + s[(2 * i + 1) * st]);
        b[2 * i + 1] = (int16_t)(s[2 * i * st] - s[(2 * i + 1) * st]);
    }
#pragma unroll
    for (int g = 0; g < 2; g++) {
        c[4 * g + 0] = (int16_t)(b[4 * g + 0] + b[4 * g + 2]);
        c[4 * g + 1] = (int16_t)(b[4 * g + 1] + b[4 * g + 3]);
        c[4 * g + 2] = (int16_t)(b[4 * g + 0] - b[4 * g + 2]);
        c[4 * g + 3] = (int16_t)(b[4 * g + 1] - b[4 * g + 3]);
    }
    // output slots of c[i] + c[i+4] and c[i] - c[i+4]
    o[0] = (int16_t)(c[0] + c[4]); o[2] = (int16_t)(c[0] - c[4]);
    o[7] = (int16_t)(c[1] + c[5]); o[6] = (int16_t)(c[1] - c[5]);
    o[3] = (int16_t)(c[2] + c[6]); o[1] = (int16_t)(c[2] - c[6]);
    o[4] = (int16_t)(c[3] + c[7]); o[5] = (int16_t)(c[3] - c[7]);
}

constexpr int kResPitch = 34; // int16 row pitch of the residual tile in LDS (17 dwords: rows land on different banks)

struct HadLds {
    int16_t res[32 * kResPitch];
    int16_t t[1024];
    int32_t c[1024];
};

// Hadamard of the n x n residual tile in L.res (n = 4, 8, 16, 32); coefficients in L.c in the reference's order.
// One wave; every step ends with a barrier.
__device__ void hadamard_tile(HadLds &L, int n, int lane) {
    if (n == 4) {
        if (lane < 4) had_col4(L.res + lane, kResPitch, L.t + 4 * lane);
        wave_sync();
        if (lane < 4) {
            int16_t o[4];
            had_col4(L.t + lane, 4, o);
            for (int k = 0; k < 4; k++) L.c[4 * lane + k] = o[k];
        }
        wave_sync();
        return;
    }
    const int nb = n >> 3; // 8x8 sub-blocks per side
    // coefficient base of the 8x8 sub-block at (by, bx): 16x16 blocks in raster order, 8x8 blocks in raster order inside
    auto base_of = [&](int by, int bx) {
        if (n == 8) return 0;
        if (n == 16) return 64 * (2 * by + bx);
        return 256 * (2 * (by >> 1) + (bx >> 1)) + 64 * (2 * (by & 1) + (bx & 1));
    };
    for (int it = lane; it < nb * nb * 8; it += 64) { // first pass: columns of every 8x8 sub-block
        const int i = it & 7, sb = it >> 3, by = sb / nb, bx = sb - by * nb;
        had_col8(L.res + (8 * by) * kResPitch + 8 * bx + i, kResPitch, L.t + base_of(by, bx) + 8 * i);
    }
    wave_sync();
    for (int it = lane; it < nb * nb * 8; it += 64) { // second pass: rows of the intermediate
        const int i = it & 7, sb = it >> 3, by = sb / nb, bx = sb - by * nb;
        const int base = base_of(by, bx);
        int16_t   o[8];
        had_col8(L.t + base + i, 8, o);
        for (int k = 0; k < 8; k++) L.c[base + 8 * i + k] = o[k];
    }
    wave_sync();
    auto combine = [&](int32_t *c, int cn, int shift, int i) {
        const int32_t a0 = c[i], a1 = c[cn + i], a2 = c[2 * cn + i], a3 = c[3 * cn + i];
        const int32_t b0 = (a0 + a1) >> shift, b1 = (a0 - a1) >> shift, b2 = (a2 + a3) >> shift, b3 = (a2 - a3) >> shift;
        c[i] = b0 + b2; c[cn + i] = b1 + b3; c[2 * cn + i] = b0 - b2; c[3 * cn + i] = b1 - b3;
    };
    if (n >= 16) {
        const int n16 = (n == 16) ? 1 : 4;
        for (int it = lane; it < n16 * 64; it += 64) combine(L.c + 256 * (it >> 6), 64, 1, it & 63);
        wave_sync();
    }
    if (n == 32) {
        for (int it = lane; it < 256; it += 64) combine(L.c, 256, 2, it);
        wave_sync();
    }
}

// ---- hadamard_path's 16x16 / 32x32 tiles on the matrix cores --------------------------------------------------------------
// The 8x8 cores of a 16x16 block are Y = H16 * (X * H16) with H16 = diag(H8, H8): two v_mfma_f32_16x16x16_f16.  Exact: 9-bit residuals and
// +-1 weights are f16 values, |X * H16| <= 8 * 255 = 2040 < 2048 is still an f16 integer, the f32 sums stay below 2^15; and the first
// product's C layout (lane holds rows k0 .. k0 + 3 of column r) is the second product's B layout.  The reference's 8-point transform is
// the same set of Walsh rows in another order without sign changes (every row starts with +1), so combining the four 8x8 blocks of a 16x16
// element by element (picture_operators_c.c:270-297: (a0 +- a1) >> 1 ...) and the four 16x16 blocks of a 32x32 (:299-326, >> 2) gives the
// reference's coefficients in a permuted order -- and SATD is a sum.  (tools/ubench/hadamard_mfma.hip measures the 8x8 core alone.)
typedef _Float16 had_half4 __attribute__((ext_vector_type(4)));
typedef float    had_float4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ had_half4 had16_weights(int lane) { // H16[r][k0 + j] = H16[k0 + j][r]
    const int r = lane & 15, k0 = 4 * (lane >> 4);
    had_half4 h;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int k = k0 + j;
        h[j] = ((k >> 3) != (r >> 3)) ? (_Float16)0 : ((__builtin_popcount((k & 7) & (r & 7)) & 1) ? (_Float16)-1 : (_Float16)1);
    }
    return h;
}

// the four 8x8 Hadamards of the 16x16 block of L.res at (16 by, 16 bx): this lane's coefficients Y[k0 + j][r] of 8x8 block (k0 / 8, r / 8)
__device__ __forceinline__ void had8x4_mfma(const HadLds &L, int by, int bx, int lane, had_half4 h, int32_t out[4]) {
    const int      r = lane & 15, k0 = 4 * (lane >> 4);
    const int16_t *x = L.res + (16 * by + r) * kResPitch + 16 * bx + k0;
    had_half4 a;
#pragma unroll
    for (int j = 0; j < 4; j++) a[j] = (_Float16)x[j];
    had_float4 t = {0, 0, 0, 0};
    t = __builtin_amdgcn_mfma_f32_16x16x16f16(a, h, t, 0, 0, 0); // T = X * H16: lane holds T[k0 + j][r]
    had_half4 tb;
#pragma unroll
    for (int j = 0; j < 4; j++) tb[j] = (_Float16)t[j];
    had_float4 y = {0, 0, 0, 0};
    y = __builtin_amdgcn_mfma_f32_16x16x16f16(h, tb, y, 0, 0, 0); // Y = H16 * T: lane holds Y[k0 + j][r], 8x8 block (k0 / 8, r / 8)
#pragma unroll
    for (int j = 0; j < 4; j++) out[j] = (int)y[j];
}

// the 16x16 block of L.res at (16 by, 16 bx): this lane's four 16x16-Hadamard coefficients (svt_aom_hadamard_16x16_c arithmetic)
__device__ __forceinline__ void had16_mfma(const HadLds &L, int by, int bx, int lane, had_half4 h, int32_t out[4]) {
    int32_t y[4];
    had8x4_mfma(L, by, bx, lane, h, y);
    const bool right = (lane & 8) != 0, bottom = (lane & 32) != 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int v = y[j], p8 = __shfl_xor(v, 8, 64), p32 = __shfl_xor(v, 32, 64), p40 = __shfl_xor(v, 40, 64);
        // the element's four 8x8 blocks in raster order
        const int l0 = right ? p8 : v, r0 = right ? v : p8;       // this lane's row of blocks: left, right
        const int l1 = right ? p40 : p32, r1 = right ? p32 : p40; // the other row of blocks
        const int a0 = bottom ? l1 : l0, a1 = bottom ? r1 : r0, a2 = bottom ? l0 : l1, a3 = bottom ? r0 : r1;
        const int b0 = (a0 + a1) >> 1, b1 = (a0 - a1) >> 1, b2 = (a2 + a3) >> 1, b3 = (a2 - a3) >> 1;
        out[j] = right ? (bottom ? b1 - b3 : b1 + b3) : (bottom ? b0 - b2 : b0 + b2);
    }
}

// sum of the absolute Hadamard coefficients of the n x n residual tile in L.res, n = 16 or 32 (this lane's share)
__device__ __forceinline__ uint32_t hadamard_satd_mfma(const HadLds &L, int n, int lane) {
    const had_half4 h = had16_weights(lane);
    uint32_t s = 0;
    if (n == 16) {
        int32_t o[4];
        had16_mfma(L, 0, 0, lane, h, o);
#pragma unroll
        for (int j = 0; j < 4; j++) s += (uint32_t)(o[j] < 0 ? -o[j] : o[j]);
        return s;
    }
    int32_t o0[4], o1[4], o2[4], o3[4];
    had16_mfma(L, 0, 0, lane, h, o0); had16_mfma(L, 0, 1, lane, h, o1); had16_mfma(L, 1, 0, lane, h, o2); had16_mfma(L, 1, 1, lane, h, o3);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int b0 = (o0[j] + o1[j]) >> 2, b1 = (o0[j] - o1[j]) >> 2, b2 = (o2[j] + o3[j]) >> 2, b3 = (o2[j] - o3[j]) >> 2;
        const int c0 = b0 + b2, c1 = b1 + b3, c2 = b0 - b2, c3 = b1 - b3;
        s += (uint32_t)(c0 < 0 ? -c0 : c0) + (uint32_t)(c1 < 0 ? -c1 : c1) + (uint32_t)(c2 < 0 ? -c2 : c2) + (uint32_t)(c3 < 0 ? -c3 : c3);
    }
    return s;
}

// (View and the psy-RD tile energy: psy_energy.h, shared with ssim_kernel.hip)

struct StatsParams {
    SvtHipBlockStatsDesc d;
    uint32_t n_front; // workgroups [0, n_front) of the launch take the regions (d.pyramids), the rest the flat jobs
    uint32_t jpw;     // flat jobs per wave: kJobsPerWave, or 1 when the batch is too small to fill the chip that way (a wave's jobs run one after the other)
};

constexpr int kJobsPerWave = 4; // a multiple of 4, at most 16 (the psy prefix sum runs inside one DPP row).  Measured: 16 jobs per wave bring the 2160p psy batch from 0.29 to 0.21 ms but the 1080p statistics batch from 0.065 to 0.22 ms (sixteen 64x64 blocks in a row make a long, lonely wave)
typedef uint32_t U32U __attribute__((aligned(1)));
typedef uint32_t U64U __attribute__((ext_vector_type(2), aligned(2)));
typedef short    short2v __attribute__((ext_vector_type(2)));

// SAD, sum and sum of squares of the differences of 4 neighbouring samples, added to the lane's running sums
__device__ __forceinline__ void quad_stats(const uint8_t *s, const uint8_t *r, uint32_t &sad, int32_t &sum, uint32_t &sq) {
    const uint32_t a = *reinterpret_cast<const U32U *>(s), b = *reinterpret_cast<const U32U *>(r);
    sad = __builtin_amdgcn_sad_u8(a, b, sad);
    sum += (int32_t)__builtin_amdgcn_sad_u8(a, 0u, 0u) - (int32_t)__builtin_amdgcn_sad_u8(b, 0u, 0u);
    // sum (a - b)^2 = a.a + b.b - 2 a.b on the packed-byte dot product
    sq += __builtin_amdgcn_udot4(a, a, __builtin_amdgcn_udot4(b, b, 0u, false), false) - 2u * __builtin_amdgcn_udot4(a, b, 0u, false);
}
__device__ __forceinline__ void quad_stats(const uint16_t *s, const uint16_t *r, uint32_t &sad, int32_t &sum, uint32_t &sq) {
    const U64U a = *reinterpret_cast<const U64U *>(s), b = *reinterpret_cast<const U64U *>(r);
    const short2v one = {1, 1};
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const uint32_t x = k ? a.y : a.x, y = k ? b.y : b.x;
        const short2v  d = __builtin_bit_cast(short2v, x) - __builtin_bit_cast(short2v, y); // 10-bit samples: no wrap
        sad = __builtin_amdgcn_sad_u16(x, y, sad);
        sum = __builtin_amdgcn_sdot2(d, one, sum, false);
        sq  = (uint32_t)__builtin_amdgcn_sdot2(d, d, (int)sq, false);
    }
}

// residuals of 4 neighbouring samples -> 4 x int16 in the LDS tile
__device__ __forceinline__ void quad_residual(const uint8_t *s, const uint8_t *r, int16_t *dst) {
    const uint32_t a = *reinterpret_cast<const U32U *>(s), b = *reinterpret_cast<const U32U *>(r);
#pragma unroll
    for (int k = 0; k < 4; k++) dst[k] = (int16_t)((int)((a >> (8 * k)) & 0xFF) - (int)((b >> (8 * k)) & 0xFF));
}
__device__ __forceinline__ void quad_residual(const uint16_t *s, const uint16_t *r, int16_t *dst) {
#pragma unroll
    for (int k = 0; k < 4; k++) dst[k] = (int16_t)((int16_t)s[k] - (int16_t)r[k]);
}

// a non-negative 64-bit value by a block's sample count (a power of two for every AV1 block shape)
__device__ __forceinline__ i64 div_by_area(i64 v, int area) { return (area & (area - 1)) ? v / area : v >> (31 - __builtin_clz(area)); }

// the per-block outputs that follow from the SAD, the sum and the sum of squares of the differences (one lane)
__device__ __forceinline__ void write_pixel_outputs(const StatsParams &p, uint32_t job, int w, int h, uint32_t sad, int32_t sum, u64 sse) {
    const uint32_t sq32 = (uint32_t)sse; // the reference's 32-bit accumulator (variance.c) wraps the same way
    if (p.d.sad) p.d.sad[job] = sad;
    if (p.d.sse) p.d.sse[job] = sse;
    if (p.d.var_sse) p.d.var_sse[job] = sq32;
    if (p.d.variance) p.d.variance[job] = sq32 - (uint32_t)div_by_area((i64)sum * sum, w * h);
    if (p.d.variance10 || p.d.var_sse10) { // highbd_10_variance (svt_psnr.c:160-177): rounding shifts, then the clamped variance
        const uint32_t sse10 = (uint32_t)((sse + 8) >> 4);
        const i64      sum10 = ((i64)sum + 2) >> 2;
        const i64      var   = (i64)sse10 - div_by_area(sum10 * sum10, w * h);
        if (p.d.var_sse10) p.d.var_sse10[job] = sse10;
        if (p.d.variance10) p.d.variance10[job] = var >= 0 ? (uint32_t)var : 0u;
    }
    // svt_spatial_full_distortion_kernel_facade (picture_operators_c.c:115-174)
    if (p.d.facade_dist)
        p.d.facade_dist[job] = (u64)svt_hip_spy_rd_bias_inline((i64)sse, (uint32_t)w, (uint32_t)h, p.d.pred_mode[job], p.d.compound_type[job],
                                                               p.d.temporal_layer_index, p.d.psy_rd, p.d.spy_rd);
}

template <typename Pix>
__device__ __forceinline__ void block_stats_job(const StatsParams &p, HadLds &L, const uint32_t job, const int lane, const bool with_satd, uint32_t &o_sad, int32_t &o_sum, u64 &o_sse) {
    const SvtHipBlockJob jb = p.d.jobs[job];
    const int w = jb.width, h = jb.height;
    const View<Pix> src = {static_cast<const Pix *>(p.d.src) + jb.src_offset, p.d.src_stride, 16 * (jb.subpel_x & 7), 16 * (jb.subpel_y & 7)};
    const View<Pix> ref = {static_cast<const Pix *>(p.d.ref) + jb.ref_offset, p.d.ref_stride, 0, 0};
    uint32_t sad = 0, sq = 0; // a lane sees at most 128 * 128 / 64 samples: its sum of squares stays below 2^32
    int32_t  sum = 0;
    if (!(src.fx1 | src.fy1) && !(w & 3)) { // uniform: plain blocks, 4 samples per lane and step
        const int   wq = w >> 2;
        const float rq = __builtin_amdgcn_rcpf((float)wq);
        for (int i = lane; i < wq * h; i += 64) {
            const int r = (int)(((float)i + 0.5f) * rq), c = 4 * (i - r * wq);
            quad_stats(src.p + (size_t)r * src.stride + c, ref.p + (size_t)r * ref.stride + c, sad, sum, sq);
        }
    } else {
        const float rw = __builtin_amdgcn_rcpf((float)w);
        for (int i = lane; i < w * h; i += 64) {
            const int r = (int)(((float)i + 0.5f) * rw), c = i - r * w; // exact for i < 2^21
            const int d = src.at(r, c) - ref.at(r, c);
            sad += (uint32_t)(d < 0 ? -d : d);
            sum += d;
            sq += (uint32_t)(d * d);
        }
    }
    sad = wave_sum_dpp(sad);
    sum = (int32_t)wave_sum_dpp((uint32_t)sum);
    const u64      sse  = (u64)wave_sum_dpp(sq & 0xFFFFu) + ((u64)wave_sum_dpp(sq >> 16) << 16);
    o_sad = sad; o_sum = sum; o_sse = sse; // the outputs derived from them are written by the caller, one lane per job of the wave
    if (p.d.satd && with_satd) { // hadamard_path_c: square blocks, <= 32x32 tiles
        uint32_t satd = 0;
        const int n = w < 32 ? w : 32;
        if (w == h && (w == 4 || w == 8 || w == 16 || w == 32 || w == 64 || w == 128)) {
            for (int ty = 0; ty < h; ty += n)
                for (int tx = 0; tx < w; tx += n) {
                    if (!(src.fx1 | src.fy1)) { // uniform: 4 samples per lane and step (n = 4 .. 32: powers of two)
                        const int sh = n == 4 ? 0 : n == 8 ? 1 : n == 16 ? 2 : 3;
                        for (int i = lane; i < (n * n) >> 2; i += 64) {
                            const int r = i >> sh, c = 4 * (i - (r << sh));
                            quad_residual(src.p + (size_t)(ty + r) * src.stride + tx + c, ref.p + (size_t)(ty + r) * ref.stride + tx + c, &L.res[r * kResPitch + c]);
                        }
                    } else
                        for (int i = lane; i < n * n; i += 64) {
                            const int r = i / n, c = i - r * n;
                            L.res[r * kResPitch + c] = (int16_t)((int16_t)src.at(ty + r, tx + c) - (int16_t)ref.at(ty + r, tx + c));
                        }
                    wave_sync();
                    if (n >= 16) satd += hadamard_satd_mfma(L, n, lane); // uniform
                    else {
                        hadamard_tile(L, n, lane);
                        for (int i = lane; i < n * n; i += 64) { const int32_t v = L.c[i]; satd += (uint32_t)(v < 0 ? -v : v); }
                    }
                    wave_sync();
                }
        }
        satd = wave_sum(satd);
        if (lane == 0) p.d.satd[job] = satd;
    }
}

struct FlatLds { // one wave's tiles
    HadLds   L;
    uint32_t tile0[kJobsPerWave + 1], esum[kJobsPerWave]; // psy: first tile of each job in the wave's tile sequence, energy sums
};
// jobs [wave * kJobsPerWave, ...) of the flat list, by one wave
template <typename Pix> __device__ __forceinline__ void block_stats_flat(const StatsParams &p, FlatLds &F, const uint32_t wave, const int lane) {
    HadLds   &L = F.L;
    uint32_t *tile0 = F.tile0, *esum = F.esum;
    const uint32_t j0 = wave * p.jpw, j1 = j0 + p.jpw < p.d.n_jobs ? j0 + p.jpw : p.d.n_jobs;
    const int      nj = (int)(j1 - j0);
    // Four consecutive plain 8x8 blocks share one matrix-core tile: their residuals side by side in the LDS tile, one pair of MFMAs, four SATDs
    uint32_t quad8 = 0; // bit g: jobs 4g .. 4g + 3 of the wave
    if (p.d.satd) { // uniform
        bool plain8 = false;
        if (lane < nj) {
            const SvtHipBlockJob jb = p.d.jobs[j0 + lane];
            plain8 = jb.width == 8 && jb.height == 8 && !(jb.subpel_x & 7) && !(jb.subpel_y & 7);
        }
        const u64 m = __ballot(plain8);
#pragma unroll
        for (int g = 0; g < kJobsPerWave / 4; g++) quad8 |= (((m >> (4 * g)) & 0xF) == 0xF) ? 1u << g : 0u;
    }
    uint32_t my_sad = 0;
    int32_t  my_sum = 0;
    u64      my_sse = 0;
    for (int k = 0; k < nj; k++) {
        uint32_t sad;
        int32_t  sum;
        u64      sse;
        block_stats_job<Pix>(p, L, j0 + k, lane, !((quad8 >> (k >> 2)) & 1), sad, sum, sse);
        if (lane == k) { my_sad = sad; my_sum = sum; my_sse = sse; }
        wave_sync(); // the LDS tile is reused by the next job
    }
    // svt_psy_distortion{,_hbd}: one lane per 8x8 (or 4x4) tile, the tiles of the wave's jobs side by side
    u64 my_e = 0;
    const bool psy = p.d.psy_energy || p.d.psy_dist || (p.d.psy_sse && p.d.psy_rd > 0.0);
    if (psy) { // uniform
        int nt = 0;
        if (lane < nj) {
            const SvtHipBlockJob jb = p.d.jobs[j0 + lane];
            const int n = (jb.width >= 8 && jb.height >= 8) ? 8 : 4; // the reference's loops: i < height; i += n
            nt = ((jb.width + n - 1) / n) * ((jb.height + n - 1) / n);
        }
        int incl = nt; // inclusive prefix over lanes 0 .. 15
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xF, 0xF, true); // row_shr:1, zero fill
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xF, 0xF, true);
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xF, 0xF, true);
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xF, 0xF, true);
        static_assert(kJobsPerWave <= 16, "the prefix sum runs inside one DPP row");
        if (lane < kJobsPerWave) { tile0[lane + 1] = (uint32_t)incl; esum[lane] = 0; }
        if (lane == 0) tile0[0] = 0;
        wave_sync();
        const int total = (int)tile0[kJobsPerWave];
        for (int t = lane; t < total; t += 64) {
            int k = 0;
#pragma unroll
            for (int i = 1; i < kJobsPerWave; i++) k += t >= (int)tile0[i] ? 1 : 0; // broadcast reads
            const int tl = t - (int)tile0[k];
            const SvtHipBlockJob jb = p.d.jobs[j0 + k];
            const int n = (jb.width >= 8 && jb.height >= 8) ? 8 : 4, ntx = (jb.width + n - 1) / n;
            const int ty = tl / ntx, tx = tl - ty * ntx;
            const View<Pix> src = {static_cast<const Pix *>(p.d.src) + jb.src_offset, p.d.src_stride, 16 * (jb.subpel_x & 7), 16 * (jb.subpel_y & 7)};
            const View<Pix> ref = {static_cast<const Pix *>(p.d.ref) + jb.ref_offset, p.d.ref_stride, 0, 0};
            const int32_t a = psy_tile_energy<Pix>(src.sub(ty * n, tx * n), n);
            const int32_t b = psy_tile_energy<Pix>(ref.sub(ty * n, tx * n), n);
            atomicAdd(&esum[k], (uint32_t)(a > b ? a - b : b - a)); // a job's sum stays below 2^32: 256 tiles x 64 x 64 x 1023
        }
        wave_sync();
        const u64 e = lane < kJobsPerWave ? esum[lane] : 0;
        my_e = sizeof(Pix) == 1 ? e >> 1 : e << 2;
    }
    if (lane < nj) { // lane k finishes job k of the wave
        const uint32_t job = j0 + lane;
        const SvtHipBlockJob jb = p.d.jobs[job];
        write_pixel_outputs(p, job, jb.width, jb.height, my_sad, my_sum, my_sse);
        if (psy) {
            if (p.d.psy_energy) p.d.psy_energy[job] = my_e;
            if (p.d.psy_dist) p.d.psy_dist[job] = (u64)((double)my_e * p.d.psy_rd); // get_svt_psy_full_dist, psy_rd.c:277-293
            if (p.d.psy_sse) p.d.psy_sse[job] = my_sse + (u64)((double)my_e * p.d.psy_rd); // svt_spatial_psy_distortion_kernel_c, picture_operators_c.c:85-112
        } else if (p.d.psy_sse) p.d.psy_sse[job] = my_sse; // psy_rd <= 0: the plain SSE
    }
    for (int g = 0; g < kJobsPerWave / 4; g++)
        if ((quad8 >> g) & 1) { // uniform
            const int q = lane >> 4, r = (lane & 15) >> 1, c = 4 * (lane & 1); // block, row, first column of this lane's 4 samples
            const SvtHipBlockJob jb = p.d.jobs[j0 + 4 * g + q];
            quad_residual(static_cast<const Pix *>(p.d.src) + jb.src_offset + (size_t)r * p.d.src_stride + c, static_cast<const Pix *>(p.d.ref) + jb.ref_offset + (size_t)r * p.d.ref_stride + c,
                          &L.res[(8 * (q >> 1) + r) * kResPitch + 8 * (q & 1) + c]);
            wave_sync();
            int32_t y[4];
            had8x4_mfma(L, 0, 0, lane, had16_weights(lane), y);
            uint32_t sv = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) sv += (uint32_t)(y[j] < 0 ? -y[j] : y[j]);
            // block (k0 / 8, r / 8) = (lane bit 5, lane bit 3): sum over the other four lane bits
            sv += __shfl_xor(sv, 1, 64); sv += __shfl_xor(sv, 2, 64); sv += __shfl_xor(sv, 4, 64); sv += __shfl_xor(sv, 16, 64);
            if ((lane & 23) == 0) p.d.satd[j0 + 4 * g + 2 * (lane >> 5) + ((lane >> 3) & 1)] = sv;
            wave_sync(); // the tile is rewritten by the next group
        }
}

// ---- hierarchical block statistics: one workgroup <-> one 64x64 region.  The region's samples are read once for the pixel statistics (and once
// more, as residuals into the LDS tiles, for hadamard_path); the sums of the nested blocks are DPP reductions.  Output slot of nested block z:
// out0 + z with z = 0 (64x64), 1 + raster (32x32), 5 + raster (16x16), 21 + raster (8x8).
// Without hadamard_path (the psy / facade batches): ONE wave per region, lane <-> one 8x8 block in Morton order (one psy tile per lane: every
// lane busy in the tile transforms), 16x16 = quad, 32x32 = 16-lane row, 64x64 = the wave.
template <typename Pix> __device__ __forceinline__ void block_stats_pyramid1(const StatsParams &p, const uint32_t reg, const int lane) {
    const uint32_t out0 = p.d.pyramid_out_base + SVT_HIP_PYRAMID_BLOCKS * reg;
    const SvtHipBlockJob jb = p.d.pyramids[reg];
    const Pix *src = static_cast<const Pix *>(p.d.src) + jb.src_offset, *ref = static_cast<const Pix *>(p.d.ref) + jb.ref_offset;
    // lane -> 8x8 block coordinates: bits x0 y0 x1 y1 x2 y2
    const int bx = (lane & 1) | ((lane >> 1) & 2) | ((lane >> 2) & 4), by = ((lane >> 1) & 1) | ((lane >> 2) & 2) | ((lane >> 3) & 4);
    uint32_t sad = 0, sq = 0;
    int32_t  sum = 0;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const Pix *s = src + (size_t)(8 * by + r) * p.d.src_stride + 8 * bx, *q = ref + (size_t)(8 * by + r) * p.d.ref_stride + 8 * bx;
        quad_stats(s, q, sad, sum, sq);
        quad_stats(s + 4, q + 4, sad, sum, sq);
    }
    const bool psy = p.d.psy_energy || p.d.psy_dist || (p.d.psy_sse && p.d.psy_rd > 0.0);
    uint32_t e8 = 0; // |energy(src tile) - energy(ref tile)| of this lane's 8x8 tile
    if (psy) { // uniform
        const View<Pix> sv = {src + (size_t)(8 * by) * p.d.src_stride + 8 * bx, p.d.src_stride, 0, 0}, rv = {ref + (size_t)(8 * by) * p.d.ref_stride + 8 * bx, p.d.ref_stride, 0, 0};
        const int32_t a = psy_tile_energy<Pix>(sv, 8), b = psy_tile_energy<Pix>(rv, 8);
        e8 = (uint32_t)(a > b ? a - b : b - a);
    }
    const uint32_t sad16 = quad_sum(sad), sq16 = quad_sum(sq), e16 = quad_sum(e8);
    const int32_t  sum16 = (int32_t)quad_sum((uint32_t)sum);
    const uint32_t sad32 = row16_sum_of_quads(sad16), sq32 = row16_sum_of_quads(sq16), e32 = row16_sum_of_quads(e16); // a 32x32 block: 1024 x 1023^2 < 2^32
    const int32_t  sum32 = (int32_t)row16_sum_of_quads((uint32_t)sum16);
    const uint32_t sad64 = wave_sum_dpp(sad), e64lo = wave_sum_dpp(e8 & 0xFFFFu), e64hi = wave_sum_dpp(e8 >> 16);
    const int32_t  sum64 = (int32_t)wave_sum_dpp((uint32_t)sum);
    const u64      sse64 = (u64)wave_sum_dpp(sq & 0xFFFFu) + ((u64)wave_sum_dpp(sq >> 16) << 16), e64 = (u64)e64lo + ((u64)e64hi << 16);
    auto emit = [&](uint32_t slot, int n, uint32_t a_sad, int32_t a_sum, u64 a_sse, u64 a_e) {
        write_pixel_outputs(p, slot, n, n, a_sad, a_sum, a_sse);
        const u64 e = sizeof(Pix) == 1 ? a_e >> 1 : a_e << 2;
        if (psy) {
            if (p.d.psy_energy) p.d.psy_energy[slot] = e;
            if (p.d.psy_dist) p.d.psy_dist[slot] = (u64)((double)e * p.d.psy_rd);
            if (p.d.psy_sse) p.d.psy_sse[slot] = a_sse + (u64)((double)e * p.d.psy_rd);
        } else if (p.d.psy_sse) p.d.psy_sse[slot] = a_sse;
    };
    emit(out0 + 21 + 8 * by + bx, 8, sad, sum, sq, e8);
    if ((lane & 3) == 0) emit(out0 + 5 + 4 * (by >> 1) + (bx >> 1), 16, sad16, sum16, sq16, e16);
    if ((lane & 15) == 0) emit(out0 + 1 + 2 * (by >> 2) + (bx >> 2), 32, sad32, sum32, sq32, e32);
    if (lane == 0) emit(out0, 64, sad64, sum64, sse64, e64);
}

// With hadamard_path -- four waves per region: wave q <-> 32x32 quadrant q (raster), lane <-> (8x8 block of the quadrant in Morton order, pair of rows): the 8x8 sums are
// quad sums, the 16x16 sums 16-lane row sums, the 32x32 sums wave sums, the 64x64 sums meet in LDS.  Each wave stages its own quadrant's
// residuals once for hadamard_path's 8x8 / 16x16 / 32x32 SATDs.
struct PyrLds {
    int16_t  res[4][32 * kResPitch];
    uint32_t sad[4], e_lo[4], e_hi[4], satd[4];
    int32_t  sum[4];
    u64      sse[4];
};
template <typename Pix> __device__ __forceinline__ void block_stats_pyramid4(const StatsParams &p, PyrLds &S, const uint32_t reg) {
    const int      lane = threadIdx.x & 63, q = threadIdx.x >> 6, qy = q >> 1, qx = q & 1;
    const uint32_t out0 = p.d.pyramid_out_base + SVT_HIP_PYRAMID_BLOCKS * reg;
    const SvtHipBlockJob jb = p.d.pyramids[reg];
    const Pix *src = static_cast<const Pix *>(p.d.src) + jb.src_offset + (size_t)(32 * qy) * p.d.src_stride + 32 * qx;
    const Pix *ref = static_cast<const Pix *>(p.d.ref) + jb.ref_offset + (size_t)(32 * qy) * p.d.ref_stride + 32 * qx;
    // lane = blk * 4 + row pair; blk bits x0 y0 x1 y1 -> 8x8 block (bx, by) of the quadrant
    const int blk = lane >> 2, rp = lane & 3, bx = (blk & 1) | ((blk >> 1) & 2), by = ((blk >> 1) & 1) | ((blk >> 2) & 2);
    uint32_t sad = 0, sq = 0;
    int32_t  sum = 0;
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const Pix *sp = src + (size_t)(8 * by + 2 * rp + r) * p.d.src_stride + 8 * bx, *qp = ref + (size_t)(8 * by + 2 * rp + r) * p.d.ref_stride + 8 * bx;
        quad_stats(sp, qp, sad, sum, sq);
        quad_stats(sp + 4, qp + 4, sad, sum, sq);
    }
    const bool psy = p.d.psy_energy || p.d.psy_dist || (p.d.psy_sse && p.d.psy_rd > 0.0);
    uint32_t e8 = 0; // |energy(src tile) - energy(ref tile)| of the block's 8x8 tile: computed by the block's first lane, zero in the others
    if (psy && rp == 0) {
        const View<Pix> sv = {src + (size_t)(8 * by) * p.d.src_stride + 8 * bx, p.d.src_stride, 0, 0}, rv = {ref + (size_t)(8 * by) * p.d.ref_stride + 8 * bx, p.d.ref_stride, 0, 0};
        const int32_t a = psy_tile_energy<Pix>(sv, 8), b = psy_tile_energy<Pix>(rv, 8);
        e8 = (uint32_t)(a > b ? a - b : b - a);
    }
    // the tree: 8x8 = quad, 16x16 = 16-lane row, 32x32 = the wave, 64x64 = the four waves
    const uint32_t sad8 = quad_sum(sad), sq8 = quad_sum(sq), e8s = quad_sum(e8);
    const int32_t  sum8 = (int32_t)quad_sum((uint32_t)sum);
    const uint32_t sad16 = row16_sum_of_quads(sad8), sq16 = row16_sum_of_quads(sq8), e16 = row16_sum_of_quads(e8s);
    const int32_t  sum16 = (int32_t)row16_sum_of_quads((uint32_t)sum8);
    const uint32_t sad32 = wave_sum_dpp(sad), sq32 = wave_sum_dpp(sq), e32lo = wave_sum_dpp(e8 & 0xFFFFu), e32hi = wave_sum_dpp(e8 >> 16); // 1024 x 1023^2 < 2^32
    const int32_t  sum32 = (int32_t)wave_sum_dpp((uint32_t)sum);
    auto emit = [&](uint32_t slot, int n, uint32_t a_sad, int32_t a_sum, u64 a_sse, u64 a_e) {
        write_pixel_outputs(p, slot, n, n, a_sad, a_sum, a_sse);
        const u64 e = sizeof(Pix) == 1 ? a_e >> 1 : a_e << 2;
        if (psy) {
            if (p.d.psy_energy) p.d.psy_energy[slot] = e;
            if (p.d.psy_dist) p.d.psy_dist[slot] = (u64)((double)e * p.d.psy_rd);
            if (p.d.psy_sse) p.d.psy_sse[slot] = a_sse + (u64)((double)e * p.d.psy_rd);
        } else if (p.d.psy_sse) p.d.psy_sse[slot] = a_sse;
    };
    if (rp == 0) emit(out0 + 21 + 8 * (4 * qy + by) + 4 * qx + bx, 8, sad8, sum8, sq8, e8s);
    if ((lane & 15) == 0) emit(out0 + 5 + 4 * (2 * qy + (by >> 1)) + 2 * qx + (bx >> 1), 16, sad16, sum16, sq16, e16);
    if (lane == 0) {
        emit(out0 + 1 + q, 32, sad32, sum32, sq32, (u64)e32lo + ((u64)e32hi << 16));
        S.sad[q] = sad32; S.sum[q] = sum32; S.sse[q] = sq32; S.e_lo[q] = e32lo; S.e_hi[q] = e32hi;
    }
    uint32_t s32 = 0;
    if (p.d.satd) { // uniform; 8-bit planes (checked by the host): hadamard_path of the quadrant's nested blocks from one staged residual
        const had_half4 h = had16_weights(lane);
        HadLds &L = *reinterpret_cast<HadLds *>(S.res[q]); // only .res is touched by the matrix-core path
        for (int i = lane; i < 256; i += 64) {
            const int r = i >> 3, c = 4 * (i & 7);
            quad_residual(src + (size_t)r * p.d.src_stride + c, ref + (size_t)r * p.d.ref_stride + c, &L.res[r * kResPitch + c]);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier(); // a wave's own LDS writes are ordered before its later reads; only this wave touches its tile
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        int32_t  o[4][4];
        uint32_t sv8[4], sv16[4];
#pragma unroll
        for (int sb = 0; sb < 4; sb++) { // the quadrant's 16x16 blocks: their four 8x8 SATDs, then their own (the sums are reduced together below)
            int32_t y[4];
            had8x4_mfma(L, sb >> 1, sb & 1, lane, h, y);
            sv8[sb] = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) sv8[sb] += (uint32_t)(y[j] < 0 ? -y[j] : y[j]);
            had16_mfma(L, sb >> 1, sb & 1, lane, h, o[sb]);
            sv16[sb] = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) sv16[sb] += (uint32_t)(o[sb][j] < 0 ? -o[sb][j] : o[sb][j]);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) { // svt_aom_hadamard_32x32_c's combine of the four 16x16 transforms (picture_operators_c.c:299-326), as hadamard_satd_mfma
            const int b0 = (o[0][j] + o[1][j]) >> 2, b1 = (o[0][j] - o[1][j]) >> 2, b2 = (o[2][j] + o[3][j]) >> 2, b3 = (o[2][j] - o[3][j]) >> 2;
            const int c0 = b0 + b2, c1 = b1 + b3, c2 = b0 - b2, c3 = b1 - b3;
            s32 += (uint32_t)(c0 < 0 ? -c0 : c0) + (uint32_t)(c1 < 0 ? -c1 : c1) + (uint32_t)(c2 < 0 ? -c2 : c2) + (uint32_t)(c3 < 0 ? -c3 : c3);
        }
#pragma unroll
        for (int sb = 0; sb < 4; sb++) {
            // 8x8 block (k0 / 8, r / 8) = (lane bit 5, lane bit 3) of the 16x16: sum over the other four lane bits
            uint32_t sv = sv8[sb];
            sv += __shfl_xor(sv, 1, 64); sv += __shfl_xor(sv, 2, 64); sv += __shfl_xor(sv, 4, 64); sv += __shfl_xor(sv, 16, 64);
            if ((lane & 23) == 0) p.d.satd[out0 + 21 + 8 * (4 * qy + 2 * (sb >> 1) + (lane >> 5)) + 4 * qx + 2 * (sb & 1) + ((lane >> 3) & 1)] = sv;
            const uint32_t s16 = wave_sum_dpp(sv16[sb]);
            if (lane == 0) p.d.satd[out0 + 5 + 4 * (2 * qy + (sb >> 1)) + 2 * qx + (sb & 1)] = s16;
        }
        s32 = wave_sum_dpp(s32);
        if (lane == 0) { p.d.satd[out0 + 1 + q] = s32; S.satd[q] = s32; }
    }
    __syncthreads();
    if (threadIdx.x == 0) { // the 64x64 block
        u64 sse = 0, e = 0;
        uint32_t sd = 0, st = 0;
        int32_t  sm = 0;
        for (int k = 0; k < 4; k++) { sse += S.sse[k]; e += (u64)S.e_lo[k] + ((u64)S.e_hi[k] << 16); sd += S.sad[k]; sm += S.sum[k]; st += S.satd[k]; }
        emit(out0, 64, sd, sm, sse, e);
        if (p.d.satd) p.d.satd[out0] = st; // hadamard_path_c: a 64x64 block is four 32x32 tiles
    }
}

// One launch per batch: the regions first, the flat jobs behind them (two launches on one stream would run one after the other, and a batch of one
// picture is a few microseconds of work per kernel).
// without hadamard_path: a wave per workgroup -- region `blockIdx.x`, or wave (blockIdx.x - n_pyramids) of the flat list
template <typename Pix> __global__ void __launch_bounds__(64) block_stats_kernel(const StatsParams p) {
    __shared__ FlatLds F;
    if (blockIdx.x < p.n_front) block_stats_pyramid1<Pix>(p, blockIdx.x, threadIdx.x);
    else block_stats_flat<Pix>(p, F, blockIdx.x - p.n_front, threadIdx.x);
}
// with hadamard_path: four waves per workgroup -- region `blockIdx.x`, or four waves of the flat list (a workgroup takes one branch as a whole:
// the region's barrier is reached by all of its waves)
union Stats4Lds {
    PyrLds  S;
    FlatLds F[4];
};
template <typename Pix> __global__ void __launch_bounds__(256) block_stats4_kernel(const StatsParams p) {
    __shared__ Stats4Lds U;
    if (blockIdx.x < p.n_front) block_stats_pyramid4<Pix>(p, U.S, blockIdx.x);
    else {
        const uint32_t wave = (blockIdx.x - p.n_front) * 4 + (threadIdx.x >> 6);
        if (wave * p.jpw < p.d.n_jobs) block_stats_flat<Pix>(p, U.F[threadIdx.x >> 6], wave, threadIdx.x & 63);
    }
}

// ---- stand-alone Hadamard (coefficients out) ------------------------------------------------------------------------
__global__ void __launch_bounds__(64) hadamard_kernel(const int16_t *src, int stride, int n, int32_t *coeff) {
    __shared__ HadLds L;
    const int lane = threadIdx.x;
    for (int i = lane; i < n * n; i += 64) { const int r = i / n, c = i - r * n; L.res[r * kResPitch + c] = src[r * stride + c]; }
    __syncthreads();
    hadamard_tile(L, n, lane);
    for (int i = lane; i < n * n; i += 64) coeff[i] = L.c[i];
}


} // namespace

extern "C" {

uint32_t svt_hip_block_stats_jobs_per_wave(SvtHipContext *ctx, const SvtHipBlockStatsDesc *d) {
    if (!ctx || !d) return 0;
    return (d->satd && d->n_jobs < (uint32_t)ctx->num_cus * 8u * kJobsPerWave) ? 1 : kJobsPerWave;
}

static int block_stats_check(const SvtHipBlockStatsDesc *d) {
    if (d->n_jobs == 0 && d->n_pyramids == 0) return SVT_HIP_OK;
    if (d->bit_depth != 8 && d->bit_depth != 10) BAD("bit_depth %u", d->bit_depth);
    if (!d->src || !d->ref || (d->n_jobs && !d->jobs) || (d->n_pyramids && !d->pyramids)) BAD("a mandatory pointer of the block-stats batch is null");
    if (d->satd && d->bit_depth != 8) BAD("hadamard_path works on 8-bit input (enc_mode_config.c:2186)");
    if ((d->variance10 || d->var_sse10) && d->bit_depth != 10) BAD("variance10 is defined on 10-bit planes");
    if (d->facade_dist && (!d->pred_mode || !d->compound_type || d->temporal_layer_index > 5))
        BAD("facade_dist needs pred_mode, compound_type and temporal_layer_index <= 5 (got %u)", d->temporal_layer_index);
    return SVT_HIP_OK;
}

int svt_hip_block_stats_batch(SvtHipContext *ctx, const SvtHipBlockStatsDesc *d) {
    return enqueue_batch("svt_hip_block_stats_batch", ctx, d, block_stats_check, &SvtHipBlockStatsDesc::n_jobs, &SvtHipBlockStatsDesc::n_pyramids, [=] {
        StatsParams p = {*d};
        // a wave works through its jobs one after the other: four per wave (shared matrix-core tiles for 8x8 blocks, fewer waves) only when that
        // still gives every CU several waves -- a one-picture batch's edge jobs are otherwise the launch's critical path
        // (hadamard_path batches only: the psy / facade batches finish a wave's four jobs side by side, one tile per lane -- measured 32 us with four
        // jobs per wave, 42 us with one, on the 2160p batch's 3,720 edge jobs)
        p.jpw = svt_hip_block_stats_jobs_per_wave(ctx, d);
        const uint32_t flat = ceil_div(d->n_jobs, p.jpw); // waves of the flat list
        p.n_front = d->n_pyramids;
        if (d->satd && d->n_pyramids) // (8-bit planes: the check saw to it)
            hipLaunchKernelGGL(block_stats4_kernel<uint8_t>, dim3(d->n_pyramids + ceil_div(flat, 4)), dim3(256), 0, ctx->stream, p);
        else if (d->bit_depth == 8) hipLaunchKernelGGL(block_stats_kernel<uint8_t>, dim3(d->n_pyramids + flat), dim3(64), 0, ctx->stream, p);
        else hipLaunchKernelGGL(block_stats_kernel<uint16_t>, dim3(d->n_pyramids + flat), dim3(64), 0, ctx->stream, p);
    });
}

} // extern "C"

// hadamard_kernel on the context stream, for svt_aom_hadamard_{4x4,8x8,16x16,32x32}_hip (leaf_kernels.hip).  The kernel stays in this file: it shares
// hadamard_tile with block_stats_kernel, and the compiler specialises that function on the callers it sees in one translation unit.
hipError_t svt_hip_hadamard_launch(SvtHipContext *ctx, const int16_t *src, int stride, int n, int32_t *coeff) {
    hipLaunchKernelGGL(hadamard_kernel, dim3(1), dim3(64), 0, ctx->stream, src, stride, n, coeff);
    return hipGetLastError();
}
