// psy_energy.h -- device code shared by the kernels that need the PSYEX psy-RD energy of a block (stats_kernel.hip, ssim_kernel.hip):
// the plane view (with the optional 2-tap sub-pixel interpolation of the variance kernels) and the energy of one 8x8 / 4x4 tile.
#ifndef SVT_HIP_PSY_ENERGY_H
#define SVT_HIP_PSY_ENERGY_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef unsigned long long u64;
typedef long long          i64;

// A block of a plane, optionally seen through the 2-tap bilinear interpolation of svt_aom_sub_pixel_variance{W}x{H}_c
// (C_DEFAULT/variance.c:28-75,308-318; taps {128 - 16k, 16k}, filter.h:39-48): horizontal pass into 16 bit, vertical pass
// back to the pixel range, each with a rounding shift by FILTER_BITS = 7.  Evaluated on the fly (4 cached reads per
// sample); a neighbour is only read when its tap is non-zero.
template <typename Pix> struct View {
    const Pix *p;
    uint32_t   stride;
    int        fx1, fy1; // second taps (0 = no interpolation in that direction)
    __device__ __forceinline__ int at(int y, int x) const {
        const Pix *q = p + (size_t)y * stride + x;
        if ((fx1 | fy1) == 0) return (int)q[0];
        const int fx0 = 128 - fx1, fy0 = 128 - fy1;
        const int m0 = ((int)q[0] * fx0 + (fx1 ? (int)q[1] * fx1 : 0) + 64) >> 7;
        if (!fy1) return (m0 * fy0 + 64) >> 7;
        const int m1 = ((int)q[stride] * fx0 + (fx1 ? (int)q[stride + 1] * fx1 : 0) + 64) >> 7;
        return (m0 * fy0 + m1 * fy1 + 64) >> 7;
    }
    __device__ __forceinline__ View sub(int y, int x) const { View v = *this; v.p = p + (size_t)y * stride + x; return v; }
};

// ---- PSYEX psy-RD energy (Codec/psy_rd.c:64-274) -----------------------------------------------------------------
// 8-bit: the reference's packed 2 x 16-bit Hadamard never overflows a half on pixel data, so it equals the plain
// unnormalised 2-D Hadamard.  10-bit: its 4-point butterflies keep 32-bit temporaries, so only the low half of the
// packed 2 x 32-bit values survives each butterfly; restated bit for bit (see oracle/stats_oracle.c for the derivation).
__device__ __forceinline__ void had8_inplace(int32_t *v) { // unnormalised 8-point Hadamard of v[0..7]
#pragma unroll
    for (int len = 1; len < 8; len <<= 1)
#pragma unroll
        for (int i = 0; i < 8; i += 2 * len)
#pragma unroll
            for (int j = i; j < i + len; j++) { const int32_t a = v[j], b = v[j + len]; v[j] = a + b; v[j + len] = a - b; }
}
__device__ __forceinline__ u64 pack32(int32_t x0, int32_t x1) { return (u64)(i64)(x0 + x1) + ((u64)(i64)(x0 - x1) << 32); }
__device__ __forceinline__ void bfly_low(u64 d[4], u64 s0, u64 s1, u64 s2, u64 s3) {
    const uint32_t t0 = (uint32_t)(s0 + s1), t1 = (uint32_t)(s0 - s1), t2 = (uint32_t)(s2 + s3), t3 = (uint32_t)(s2 - s3);
    d[0] = (uint32_t)(t0 + t2); d[1] = (uint32_t)(t1 + t3); d[2] = (uint32_t)(t0 - t2); d[3] = (uint32_t)(t1 - t3);
}
__device__ __forceinline__ u64 abs_halves(u64 a) { const u64 m = (a >> 31) & 0x100000001ull, s = (m << 32) - m; return (a + s) ^ s; }
__device__ __forceinline__ u64 fold_halves(u64 b) { return (uint32_t)b + (b >> 32); }

// energy of one n x n tile (n = 8 or 4) of plane p: Hadamard sum - (sum of pixels >> 2)
template <typename Pix> __device__ int32_t psy_tile_energy(const View<Pix> &pv, int n) {
    i64 sum = 0, had;
    if (sizeof(Pix) == 1) {
        int32_t m[8][8];
        if (n == 8) {
#pragma unroll
            for (int y = 0; y < 8; y++) {
#pragma unroll
                for (int x = 0; x < 8; x++) { m[y][x] = (int32_t)pv.at(y, x); sum += m[y][x]; }
                had8_inplace(m[y]);
            }
            i64 acc = 0;
#pragma unroll
            for (int x = 0; x < 8; x++) {
                int32_t c[8];
#pragma unroll
                for (int y = 0; y < 8; y++) c[y] = m[y][x];
                had8_inplace(c);
#pragma unroll
                for (int y = 0; y < 8; y++) acc += c[y] < 0 ? -c[y] : c[y];
            }
            had = (acc + 2) >> 2;
        } else {
            int32_t q[4][4];
            i64     acc = 0;
#pragma unroll
            for (int y = 0; y < 4; y++) {
#pragma unroll
                for (int x = 0; x < 4; x++) { q[y][x] = (int32_t)pv.at(y, x); sum += q[y][x]; }
                const int32_t a = q[y][0] + q[y][1], b = q[y][0] - q[y][1], c = q[y][2] + q[y][3], d = q[y][2] - q[y][3];
                q[y][0] = a + c; q[y][1] = b + d; q[y][2] = a - c; q[y][3] = b - d;
            }
#pragma unroll
            for (int x = 0; x < 4; x++) {
                const int32_t a = q[0][x] + q[1][x], b = q[0][x] - q[1][x], c = q[2][x] + q[3][x], d = q[2][x] - q[3][x];
                const int32_t o0 = a + c, o1 = b + d, o2 = a - c, o3 = b - d;
                acc += (o0 < 0 ? -o0 : o0) + (o1 < 0 ? -o1 : o1) + (o2 < 0 ? -o2 : o2) + (o3 < 0 ? -o3 : o3);
            }
            had = acc >> 1;
        }
    } else {
        u64 t[8][4], hs = 0;
        if (n == 8) {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                int32_t r[8];
#pragma unroll
                for (int x = 0; x < 8; x++) { r[x] = (int32_t)pv.at(i, x); sum += r[x]; }
                bfly_low(t[i], pack32(r[0], r[1]), pack32(r[2], r[3]), pack32(r[4], r[5]), pack32(r[6], r[7]));
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                u64 a[8], b = 0;
                bfly_low(a, t[0][i], t[1][i], t[2][i], t[3][i]);
                bfly_low(a + 4, t[4][i], t[5][i], t[6][i], t[7][i]);
#pragma unroll
                for (int k = 0; k < 4; k++) b += abs_halves(a[k] + a[k + 4]) + abs_halves(a[k] - a[k + 4]);
                hs += fold_halves(b);
            }
            had = (i64)((hs + 2) >> 2);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                int32_t r[4];
#pragma unroll
                for (int x = 0; x < 4; x++) { r[x] = (int32_t)pv.at(i, x); sum += r[x]; }
                const u64 b0 = pack32(r[0], r[1]), b1 = pack32(r[2], r[3]);
                t[i][0] = b0 + b1; t[i][1] = b0 - b1;
            }
#pragma unroll
            for (int i = 0; i < 2; i++) {
                u64 a[4];
                bfly_low(a, t[0][i], t[1][i], t[2][i], t[3][i]);
                hs += fold_halves(abs_halves(a[0]) + abs_halves(a[1]) + abs_halves(a[2]) + abs_halves(a[3]));
            }
            had = (i64)(hs >> 1);
        }
    }
    return (int32_t)(had - (sum >> 2));
}

} // namespace
#endif
