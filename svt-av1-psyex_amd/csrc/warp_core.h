// warp_core.h -- what the warp kernels share (warp_kernel.hip: prediction, fit and MV refinement of the local warp; gm_kernel.hip: the refinement of
// the global-motion models): the filter and divisor tables, the 8x8 tile of svt_av1_warp_affine_c / svt_av1_highbd_warp_affine_c, and the integer
// pieces of svt_get_shear_params (warped_motion.c:320-363, :898-921).  Every file that includes it holds its own copy of the 3.5 KB of tables in
// constant memory.  And the host-side check of SvtHipWarpRef planes that their *_check_desc entries share.
#ifndef SVT_HIP_WARP_CORE_H
#define SVT_HIP_WARP_CORE_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "batch_host.h"
#include "../../include/svt_hip_warp.h"
#include "wave_ops.h"

// What every descriptor that carries SvtHipWarpRef planes asks of them (host side): a plane, a stride and a picture, and the picture inside the
// plane.  `who` is the *_check_desc that asks, `what` names the planes in the refusal.
static inline int svt_hip_check_warp_refs(const char *who, const char *what, const SvtHipWarpRef *refs, int n_refs) {
    for (int i = 0; i < n_refs; i++) {
        const SvtHipWarpRef *r = &refs[i];
        if (!r->plane) BAD("%s: %s %d has a null plane", who, what, i);
        if (r->stride == 0 || r->width == 0 || r->height == 0) BAD("%s: %s %d: stride %u, picture %u x %u (all non-zero)", who, what, i, r->stride, r->width, r->height);
        if ((uint32_t)r->org_x + r->width > r->stride || (uint32_t)r->org_y + r->height > r->rows)
            BAD("%s: %s %d: the picture %u x %u at (%u, %u) lies outside its plane (stride %u, %u rows)", who, what, i, r->width, r->height, r->org_x, r->org_y, r->stride,
                r->rows);
    }
    return SVT_HIP_OK;
}

namespace {

// Warped_Filters of the AV1 specification (7.11.3.5), 1/64 sample steps.  Rows 0..63 (offsets [-1, 0)) are the six taps of kSide at positions
// 0..5, rows 128..191 (offsets [1, 2)) the same six at positions 2..7 -- but for row 128, which is kRow128 --, rows 64..127 (offsets [0, 1)) the
// eight taps of kMid, row 192 repeats 191.
constexpr int8_t kRow128[8] = {0, 0, 0, 1, 127, 0, 0, 0};
constexpr int8_t kSide[64][6] = {
    {0, 0, 127, 1, 0, 0},      {0, -1, 127, 2, 0, 0},     {1, -3, 127, 4, -1, 0},    {1, -4, 126, 6, -2, 1},    {1, -5, 126, 8, -3, 1},
    {1, -6, 125, 11, -4, 1},   {1, -7, 124, 13, -4, 1},   {2, -8, 123, 15, -5, 1},   {2, -9, 122, 18, -6, 1},   {2, -10, 121, 20, -6, 1},
    {2, -11, 120, 22, -7, 2},  {2, -12, 119, 25, -8, 2},  {3, -13, 117, 27, -8, 2},  {3, -13, 116, 29, -9, 2},  {3, -14, 114, 32, -10, 3},
    {3, -15, 113, 35, -10, 2}, {3, -15, 111, 37, -11, 3}, {3, -16, 109, 40, -11, 3}, {3, -16, 108, 42, -12, 3}, {4, -17, 106, 45, -13, 3},
    {4, -17, 104, 47, -13, 3}, {4, -17, 102, 50, -14, 3}, {4, -17, 100, 52, -14, 3}, {4, -18, 98, 55, -15, 4},  {4, -18, 96, 58, -15, 3},
    {4, -18, 94, 60, -16, 4},  {4, -18, 91, 63, -16, 4},  {4, -18, 89, 65, -16, 4},  {4, -18, 87, 68, -17, 4},  {4, -18, 85, 70, -17, 4},
    {4, -18, 82, 73, -17, 4},  {4, -18, 80, 75, -17, 4},  {4, -18, 78, 78, -18, 4},  {4, -17, 75, 80, -18, 4},  {4, -17, 73, 82, -18, 4},
    {4, -17, 70, 85, -18, 4},  {4, -17, 68, 87, -18, 4},  {4, -16, 65, 89, -18, 4},  {4, -16, 63, 91, -18, 4},  {4, -16, 60, 94, -18, 4},
    {3, -15, 58, 96, -18, 4},  {4, -15, 55, 98, -18, 4},  {3, -14, 52, 100, -17, 4}, {3, -14, 50, 102, -17, 4}, {3, -13, 47, 104, -17, 4},
    {3, -13, 45, 106, -17, 4}, {3, -12, 42, 108, -16, 3}, {3, -11, 40, 109, -16, 3}, {3, -11, 37, 111, -15, 3}, {2, -10, 35, 113, -15, 3},
    {3, -10, 32, 114, -14, 3}, {2, -9, 29, 116, -13, 3},  {2, -8, 27, 117, -13, 3},  {2, -8, 25, 119, -12, 2},  {2, -7, 22, 120, -11, 2},
    {1, -6, 20, 121, -10, 2},  {1, -6, 18, 122, -9, 2},   {1, -5, 15, 123, -8, 2},   {1, -4, 13, 124, -7, 1},   {1, -4, 11, 125, -6, 1},
    {1, -3, 8, 126, -5, 1},    {1, -2, 6, 126, -4, 1},    {0, -1, 4, 127, -3, 1},    {0, 0, 2, 127, -1, 0}};
constexpr int8_t kMid[64][8] = {
    {0, 0, 0, 127, 1, 0, 0, 0},         {0, 0, -1, 127, 2, 0, 0, 0},        {0, 1, -3, 127, 4, -2, 1, 0},       {0, 1, -5, 127, 6, -2, 1, 0},
    {0, 2, -6, 126, 8, -3, 1, 0},       {-1, 2, -7, 126, 11, -4, 2, -1},    {-1, 3, -8, 125, 13, -5, 2, -1},    {-1, 3, -10, 124, 16, -6, 3, -1},
    {-1, 4, -11, 123, 18, -7, 3, -1},   {-1, 4, -12, 122, 20, -7, 3, -1},   {-1, 4, -13, 121, 23, -8, 3, -1},   {-2, 5, -14, 120, 25, -9, 4, -1},
    {-1, 5, -15, 119, 27, -10, 4, -1},  {-1, 5, -16, 118, 30, -11, 4, -1},  {-2, 6, -17, 116, 33, -12, 5, -1},  {-2, 6, -17, 114, 35, -12, 5, -1},
    {-2, 6, -18, 113, 38, -13, 5, -1},  {-2, 7, -19, 111, 41, -14, 6, -2},  {-2, 7, -19, 110, 43, -15, 6, -2},  {-2, 7, -20, 108, 46, -15, 6, -2},
    {-2, 7, -20, 106, 49, -16, 6, -2},  {-2, 7, -21, 104, 51, -16, 7, -2},  {-2, 7, -21, 102, 54, -17, 7, -2},  {-2, 8, -21, 100, 56, -18, 7, -2},
    {-2, 8, -22, 98, 59, -18, 7, -2},   {-2, 8, -22, 96, 62, -19, 7, -2},   {-2, 8, -22, 94, 64, -19, 7, -2},   {-2, 8, -22, 91, 67, -20, 8, -2},
    {-2, 8, -22, 89, 69, -20, 8, -2},   {-2, 8, -22, 87, 72, -21, 8, -2},   {-2, 8, -21, 84, 74, -21, 8, -2},   {-2, 8, -22, 82, 77, -21, 8, -2},
    {-2, 8, -21, 79, 79, -21, 8, -2},   {-2, 8, -21, 77, 82, -22, 8, -2},   {-2, 8, -21, 74, 84, -21, 8, -2},   {-2, 8, -21, 72, 87, -22, 8, -2},
    {-2, 8, -20, 69, 89, -22, 8, -2},   {-2, 8, -20, 67, 91, -22, 8, -2},   {-2, 7, -19, 64, 94, -22, 8, -2},   {-2, 7, -19, 62, 96, -22, 8, -2},
    {-2, 7, -18, 59, 98, -22, 8, -2},   {-2, 7, -18, 56, 100, -21, 8, -2},  {-2, 7, -17, 54, 102, -21, 7, -2},  {-2, 7, -16, 51, 104, -21, 7, -2},
    {-2, 6, -16, 49, 106, -20, 7, -2},  {-2, 6, -15, 46, 108, -20, 7, -2},  {-2, 6, -15, 43, 110, -19, 7, -2},  {-2, 6, -14, 41, 111, -19, 7, -2},
    {-1, 5, -13, 38, 113, -18, 6, -2},  {-1, 5, -12, 35, 114, -17, 6, -2},  {-1, 5, -12, 33, 116, -17, 6, -2},  {-1, 4, -11, 30, 118, -16, 5, -1},
    {-1, 4, -10, 27, 119, -15, 5, -1},  {-1, 4, -9, 25, 120, -14, 5, -2},   {-1, 3, -8, 23, 121, -13, 4, -1},   {-1, 3, -7, 20, 122, -12, 4, -1},
    {-1, 3, -7, 18, 123, -11, 4, -1},   {-1, 3, -6, 16, 124, -10, 3, -1},   {-1, 2, -5, 13, 125, -8, 3, -1},    {-1, 2, -4, 11, 126, -7, 2, -1},
    {0, 1, -3, 8, 126, -6, 2, 0},       {0, 1, -2, 6, 127, -5, 1, 0},       {0, 1, -2, 4, 127, -3, 1, 0},       {0, 0, 0, 2, 127, -1, 0, 0}};

struct WarpTables {
    int16_t  filter[193][8]; // 16-byte rows
    uint16_t div_lut[257];   // round(2^22 / (256 + i)): DIV_LUT_PREC_BITS 14 over DIV_LUT_BITS 8
};
constexpr WarpTables make_tables() {
    WarpTables t{};
    for (int i = 0; i < 64; i++) {
        for (int m = 0; m < 6; m++) { t.filter[i][m] = kSide[i][m]; t.filter[128 + i][m + 2] = kSide[i][m]; }
        for (int m = 0; m < 8; m++) t.filter[64 + i][m] = kMid[i][m];
    }
    for (int m = 0; m < 8; m++) t.filter[128][m] = kRow128[m];
    for (int m = 0; m < 8; m++) t.filter[192][m] = t.filter[191][m];
    for (int i = 0; i <= 256; i++) t.div_lut[i] = (uint16_t)(((1u << 22) + (256u + (unsigned)i) / 2u) / (256u + (unsigned)i));
    return t;
}
constexpr WarpTables                                       kTablesHost = make_tables();
__constant__ __attribute__((aligned(16))) const WarpTables kTables     = make_tables();

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int iabs(int v) { return v < 0 ? -v : v; }

// is_affine_shear_allowed, and what the filter takes for granted: multiples of 1 << WARP_PARAM_REDUCE_BITS
__device__ __forceinline__ bool shear_allowed(int alpha, int beta, int gamma, int delta) {
    if (((alpha | beta | gamma | delta) & 63) != 0) return false;
    return 4 * iabs(alpha) + 7 * iabs(beta) < (1 << 16) && 4 * iabs(gamma) + 4 * iabs(delta) < (1 << 16);
}

// the eight taps of the filter at offset s (1/65536 sample): ROUND_POWER_OF_TWO(s, WARPEDDIFF_PREC_BITS) + WARPEDPIXEL_PREC_SHIFTS, which the
// shear test keeps inside [0, 192]; the clamp costs one instruction and keeps the load inside the table whatever the job says
__device__ __forceinline__ void load_taps(int s, int *f) {
    const int   offs = clampi(((s + 512) >> 10) + 64, 0, 192);
    const uint4 t    = *(const uint4 *)&kTables.filter[offs][0];
    f[0] = (int)(int16_t)(t.x & 0xFFFFu); f[1] = (int)t.x >> 16; f[2] = (int)(int16_t)(t.y & 0xFFFFu); f[3] = (int)t.y >> 16;
    f[4] = (int)(int16_t)(t.z & 0xFFFFu); f[5] = (int)t.z >> 16; f[6] = (int)(int16_t)(t.w & 0xFFFFu); f[7] = (int)t.w >> 16;
}

struct Model { // wave-uniform
    int mat[6], alpha, beta, gamma, delta;
};

// One 8x8 tile of one reference: the vertical filter's sum of this lane's sample, rounded by `reduce_vert`
template <bool HBD>
__device__ __forceinline__ int warp_tile(const SvtHipWarpRef &r, const Model &m, int jx, int iy, int ss_x, int ss_y, int reduce_vert, uint16_t *s_src,
                                         uint16_t *s_mid, int lane) {
    using Px = typename std::conditional<HBD, uint16_t, uint8_t>::type;
    constexpr int bd = HBD ? 10 : 8;
    // the tile's centre, projected: 32-bit arithmetic as the reference's
    const uint32_t src_x = (uint32_t)(jx + 4) << ss_x, src_y = (uint32_t)(iy + 4) << ss_y;
    const int x4  = (int)((uint32_t)m.mat[2] * src_x + (uint32_t)m.mat[3] * src_y + (uint32_t)m.mat[0]) >> ss_x;
    const int y4  = (int)((uint32_t)m.mat[4] * src_x + (uint32_t)m.mat[5] * src_y + (uint32_t)m.mat[1]) >> ss_y;
    const int ix4 = x4 >> 16, iy4 = y4 >> 16;
    const int sx4 = ((x4 & 0xFFFF) - 4 * (m.alpha + m.beta)) & ~63, sy4 = ((y4 & 0xFFFF) - 4 * (m.gamma + m.delta)) & ~63;

    // the window: rows iy4 - 7 .. iy4 + 7, columns ix4 - 7 .. ix4 + 7, every coordinate clamped to the picture
    const Px *plane = (const Px *)r.plane + (size_t)r.org_y * r.stride + r.org_x;
    const int max_x = (int)r.width - 1, max_y = (int)r.height - 1;
    {
        const int wc = lane & 15, x = clampi(ix4 + wc - 7, 0, max_x);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int wr = (lane >> 4) + 4 * i;
            if (wr < 15) s_src[wr * 16 + wc] = (uint16_t)plane[(size_t)clampi(iy4 + wr - 7, 0, max_y) * r.stride + (size_t)x];
        }
    }
    wave_sync();
    const int c = lane & 7, rr = lane >> 3;
    // horizontal: row k = wr - 7, column l = c - 4; sx = sx4 + beta * (k + 4) + alpha * (l + 4)
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const int wr = rr + 8 * p;
        if (wr < 15) {
            int f[8];
            load_taps(sx4 + m.beta * (wr - 3) + m.alpha * c, f);
            int sum = 1 << (bd + 6);
#pragma unroll
            for (int t = 0; t < 8; t++) sum += (int)s_src[wr * 16 + c + t] * f[t];
            s_mid[wr * 8 + c] = (uint16_t)((sum + 4) >> 3); // round_0 = 3; below 1 << (bd + 5)
        }
    }
    wave_sync();
    // vertical: row k = rr - 4, column l = c - 4; sy = sy4 + delta * (k + 4) + gamma * (l + 4)
    int f[8];
    load_taps(sy4 + m.delta * rr + m.gamma * c, f);
    int sum = 1 << (bd + 11);
#pragma unroll
    for (int t = 0; t < 8; t++) sum += (int)s_mid[(rr + t) * 8 + c] * f[t];
    wave_sync(); // the next tile's window and intermediate may follow
    return (sum + ((1 << reduce_vert) >> 1)) >> reduce_vert;
}

// ---- the integer pieces of the fit and of svt_get_shear_params ----
__device__ __forceinline__ int msb64(uint64_t v) { return 63 - __builtin_clzll(v); }
__device__ __forceinline__ int64_t round_shift_signed_64(int64_t v, int n) { // ROUND_POWER_OF_TWO_SIGNED_64
    const int64_t half = ((int64_t)1 << n) >> 1;
    return v < 0 ? -((-v + half) >> n) : (v + half) >> n;
}
__device__ __forceinline__ int round_shift_signed(int v, int n) { // ROUND_POWER_OF_TWO_SIGNED
    const int half = (1 << n) >> 1;
    return v < 0 ? -((-v + half) >> n) : (v + half) >> n;
}
// resolve_divisor_64 (resolve_divisor_32 is the same on a narrower argument): 1 / D = y / 2^shift
__device__ __forceinline__ int resolve_divisor(uint64_t D, int *shift) {
    const int     s = msb64(D);
    const int64_t e = (int64_t)(D - ((uint64_t)1 << s));
    const int64_t f = s > 8 ? (e + (((int64_t)1 << (s - 8)) >> 1)) >> (s - 8) : e << (8 - s);
    *shift = s + 14;
    return kTables.div_lut[f];
}
__device__ __forceinline__ int clamp64(int64_t v, int lo, int hi) { return (int)(v < lo ? lo : (v > hi ? hi : v)); }
__device__ __forceinline__ int reduce_shear(int v) { return (int16_t)(round_shift_signed((int16_t)clampi(v, INT16_MIN, INT16_MAX), 6) * 64); }

// svt_get_shear_params behind its is_affine_valid test (m2 > 0 is the caller's): the four parameters of the matrix, reduced to multiples of 64,
// and what is_affine_shear_allowed says of them
__device__ __forceinline__ bool shear_params(int m2, int m3, int m4, int m5, int *al, int *be, int *ga, int *de) {
    int       sh;
    const int y = (int16_t)resolve_divisor((uint64_t)m2, &sh);
    *al = reduce_shear(m2 - (1 << 16));
    *be = reduce_shear(m3);
    *ga = reduce_shear((int)round_shift_signed_64((int64_t)m4 * (1 << 16) * y, sh));
    *de = reduce_shear(m5 - (int)round_shift_signed_64((int64_t)m3 * m4 * y, sh) - (1 << 16));
    return 4 * iabs(*al) + 7 * iabs(*be) < (1 << 16) && 4 * iabs(*ga) + 4 * iabs(*de) < (1 << 16);
}

} // namespace
#endif
