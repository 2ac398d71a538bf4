// cdef_kernel.hip -- the constrained directional enhancement filter on gfx950: svt_hip_cdef_search_batch (the strength search),
// svt_hip_cdef_pick_batch (the joint strength selection) and svt_hip_cdef_apply_batch (the filter with the chosen strengths).
//
// Reference functions restated (Source/Lib/Codec):
//   cdef_seg_search                                                                                   cdef_process.c:106-349
//   constrain, adjust_strength, svt_aom_cdef_find_dir_c, svt_cdef_filter_block_c, svt_cdef_filter_fb  cdef.c:84-430
//   dist_8xn_*_c, mse_4xn_*_c, svt_aom_compute_cdef_dist_{8bit_,}c                                    enc_cdef.c:23-219
//   svt_av1_cdef_frame                                                                                enc_cdef.c:284-610
//   svt_search_one_dual_c, joint_strength_search_dual, finish_cdef_search                             enc_cdef.c:627-965
//
// Search.  A workgroup of four waves per filter block, the luma launch before the chroma launch (chroma filters along luma's directions, which it
// reads from the dir output).  The window -- the filter block, 3 rows and 8 columns of its neighbours, CDEF_VERY_LARGE where the picture ends --
// is staged once in LDS as uint16_t, the source block beside it.  A luma wave is one 8x8 block, lane = sample; a chroma wave is four 4x4 blocks.
// First the waves share the listed blocks for the directions; then every wave walks all listed blocks for the strengths it owns (gi % 4 == wave),
// so a (filter block, strength) sum has one owner, needs no atomic and does not depend on arrival order.  The taps of a block are loaded once for
// all strengths with a primary part and once, along direction 0, for those without.
// The luma distortion is IEEE double: contraction is off for this file, the division is IEEE, and the square root is settled in integers (see
// sqrt_exact).
//
// Pick.  An init launch (bias, zero_cost, the first baseline), then per svt_search_one_dual call a launch that adds up tot[j][k] over the filter
// blocks with 64-bit integer atomics and a one-workgroup launch that takes the first minimum, moves the reference's state on (the greedy additions,
// then drop-the-oldest and re-add; the bit-count choice behind the last call of each count) and leaves the next call's baseline per block.  The
// calls follow each other by stream order alone.
//
// Apply.  A workgroup per (filter block, plane).  Every tap reads the input plane, which is what the reference's line and column buffers hold.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "batch_host.h"
#include "../../include/svt_hip_cdef.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace {

constexpr int      kWaves = 4, kThreads = 64 * kWaves;
constexpr int      kLarge = 0x7F7F;      // CDEF_VERY_LARGE
constexpr int      kLStride = 88;        // LDS row of the luma window in samples: 80 used.  44 dwords: the 8 rows of a block start at banks
                                         // 0 44 24 4 48 28 8 52, four dwords each, so a wave's read of one tap touches every bank at most once
constexpr int      kCStride = 48;        // chroma: 24 dwords, the 4 rows of a 4x4 row of blocks start at banks 0 24 48 8, eight dwords each
constexpr int      kLRows = 70, kCRows = 38;
constexpr uint64_t kNone = (uint64_t)1 << 63;
constexpr int      kMaxSlices = 64;

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int msb(int v) { return 31 - __clz(v); } // v > 0

template <bool HBD> __device__ __forceinline__ int sample_at(const void *p, size_t i) {
    if constexpr (HBD) return ((const uint16_t *)p)[i];
    else return ((const uint8_t *)p)[i];
}
template <bool HBD> __device__ __forceinline__ void store_at(void *p, size_t i, int v) {
    if constexpr (HBD) ((uint16_t *)p)[i] = (uint16_t)v;
    else ((uint8_t *)p)[i] = (uint8_t)v;
}

// What a filter block is in one plane: bs 64 (luma) or 32 (chroma)
struct FbGeom {
    int x0, y0, hs, vs;         // origin and size inside the picture
    int xlo, xhi, ylo, yhi;     // the samples the window may take from the plane
};
__device__ __forceinline__ FbGeom fb_geom(const SvtHipCdefPlane &p, int fb, int nhfb, int nvfb, int bs) {
    FbGeom g;
    const int fbr = fb / nhfb, fbc = fb % nhfb;
    g.x0 = fbc * bs; g.y0 = fbr * bs;
    g.hs = imin(bs, (int)p.width - g.x0); g.vs = imin(bs, (int)p.height - g.y0);
    // cdef_process.c:215-218; the last filter block of a row may be narrower than the border: taps reach 2 samples, and the plane is not read past its picture
    g.xlo = g.x0 - (fbc != 0 ? 8 : 0); g.xhi = imin(g.x0 + g.hs + (fbc + 1 < nhfb ? 8 : 0), (int)p.width);
    g.ylo = g.y0 - (fbr != 0 ? 3 : 0); g.yhi = imin(g.y0 + g.vs + (fbr + 1 < nvfb ? 3 : 0), (int)p.height);
    return g;
}
// window[r][c] = plane(y0 - 3 + r, x0 - 8 + c) for r < bs + 6, c < bs + 16
template <bool HBD> __device__ __forceinline__ void stage_window(uint16_t *win, int stride, const SvtHipCdefPlane &p, const FbGeom &g, int bs) {
    const int cols = bs + 16, n = (bs + 6) * cols;
    for (int idx = (int)threadIdx.x; idx < n; idx += kThreads) {
        const int r = idx / cols, c = idx - r * cols, y = g.y0 - 3 + r, x = g.x0 - 8 + c;
        const bool in = x >= g.xlo && x < g.xhi && y >= g.ylo && y < g.yhi;
        win[r * stride + c] = (uint16_t)(in ? sample_at<HBD>(p.plane, (size_t)y * p.stride + (size_t)x) : kLarge);
    }
}
// block[r][c] = plane(y0 + r, x0 + c) inside the filter block, 0 outside
template <bool HBD> __device__ __forceinline__ void stage_block(uint16_t *blk, const SvtHipCdefPlane &p, const FbGeom &g, int bs) {
    for (int idx = (int)threadIdx.x; idx < bs * bs; idx += kThreads) {
        const int r = idx / bs, c = idx - r * bs;
        blk[idx] = (uint16_t)((r < g.vs && c < g.hs) ? sample_at<HBD>(p.plane, (size_t)(g.y0 + r) * p.stride + (size_t)(g.x0 + c)) : 0);
    }
}
// the 8x8 blocks a filter block has inside the picture (nhb / 2 by nvb / 2), as a mask in the order of the host's
__device__ __forceinline__ uint64_t valid_mask(int hs, int vs) {
    const uint64_t row = ((uint64_t)1 << (hs >> 3)) - 1; // hs / 8 in 1..8
    uint64_t       m = 0;
    for (int by = 0; by < (vs >> 3); by++) m |= row << (8 * by);
    return m;
}

// ---- svt_aom_cdef_find_dir_c on one wave: lane = sample ----
// The 8 directions have 15 + 11 + 8 + 11 + 15 + 11 + 8 + 11 lines; laid out as 8 x 15 = 120 slots, slot = lane + 64 * pass.  A lane keeps, per pass,
// the samples of its line as a 64-bit mask and the line's weight 840 / (number of samples), 0 for a slot without a line.
struct DirLane { uint64_t m[2]; int w[2]; };
__device__ __forceinline__ int line_of(int d, int i, int j) {
    switch (d) {
    case 0: return i + j;
    case 1: return i + (j >> 1);
    case 2: return i;
    case 3: return 3 + i - (j >> 1);
    case 4: return 7 + i - j;
    case 5: return 3 - (i >> 1) + j;
    case 6: return j;
    default: return (i >> 1) + j;
    }
}
__device__ __forceinline__ DirLane dir_lane(int lane) {
    DirLane L;
    for (int pass = 0; pass < 2; pass++) {
        const int slot = lane + 64 * pass, d = slot / 15, n = slot - d * 15;
        uint64_t  m = 0;
        if (slot < 120)
            for (int k = 0; k < 64; k++) m |= (uint64_t)(line_of(d, k >> 3, k & 7) == n) << k;
        const int cnt = __popcll(m);
        L.m[pass] = m;
        L.w[pass] = cnt ? 840 / cnt : 0; // div_table: 840 420 280 210 168 140 120 105
    }
    return L;
}
// x: the lane's sample, (v >> coeff_shift) - 128.  scr: 128 ints of the wave's own.  Every lane gets dir and var.
__device__ __forceinline__ void find_dir(int x, const DirLane &L, int *scr, int lane, int &dir, int &var) {
    int p0 = 0, p1 = 0;
#pragma unroll
    for (int k = 0; k < 64; k++) {
        const int xv = __builtin_amdgcn_readlane(x, k);
        p0 += ((L.m[0] >> k) & 1) ? xv : 0;
        p1 += ((L.m[1] >> k) & 1) ? xv : 0;
    }
    wave_sync();
    scr[lane]      = p0 * p0 * L.w[0];
    scr[64 + lane] = p1 * p1 * L.w[1];
    wave_sync();
    int cost = 0;
    if (lane < 8)
        for (int n = 0; n < 15; n++) cost += scr[lane * 15 + n];
    int best = 0, bd = 0, c[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        c[k] = __builtin_amdgcn_readlane(cost, k);
        if (c[k] > best) { best = c[k]; bd = k; }
    }
    int opp = c[0];
#pragma unroll
    for (int k = 1; k < 8; k++) opp = (((bd + 4) & 7) == k) ? c[k] : opp;
    dir = bd;
    var = (best - opp) >> 10;
}

// ---- the filter of one sample ----
// svt_aom_eb_cdef_directions as nibbles (dy0 + 2, dx0 + 2, dy1 + 2, dx1 + 2) per direction
__device__ __forceinline__ int dir_offset(int d, int k, int stride) {
    const uint64_t t = (d & 4) ? 0x1423242334234433ull : 0x4332423241324031ull;
    const int      w = (int)(t >> (16 * (d & 3))) >> (8 * k);
    return ((w & 15) - 2) * stride + (((w >> 4) & 15) - 2);
}
struct Taps { int p[4], s[8], mn, mx; };
// the 12 taps of the sample at win[pos] along direction d: p[2k], p[2k + 1] = +-directions[d][k]; s[4k .. 4k + 3] = +-directions[d + 2][k], +-directions[d - 2][k]
__device__ __forceinline__ void load_taps(const uint16_t *win, int pos, int stride, int d, int x, Taps &t) {
    t.mn = t.mx = x;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int o = dir_offset(d, k, stride), o2 = dir_offset((d + 2) & 7, k, stride), o3 = dir_offset((d - 2) & 7, k, stride);
        t.p[2 * k] = win[pos + o]; t.p[2 * k + 1] = win[pos - o];
        t.s[4 * k] = win[pos + o2]; t.s[4 * k + 1] = win[pos - o2]; t.s[4 * k + 2] = win[pos + o3]; t.s[4 * k + 3] = win[pos - o3];
    }
#pragma unroll
    for (int k = 0; k < 4; k++) { t.mn = imin(t.mn, t.p[k]); t.mx = t.p[k] != kLarge ? imax(t.mx, t.p[k]) : t.mx; }
#pragma unroll
    for (int k = 0; k < 8; k++) { t.mn = imin(t.mn, t.s[k]); t.mx = t.s[k] != kLarge ? imax(t.mx, t.s[k]) : t.mx; }
}
__device__ __forceinline__ int constrain(int diff, int threshold, int shift) { // a zero threshold gives 0 by itself
    const int a = diff < 0 ? -diff : diff, m = imin(a, imax(0, threshold - (a >> shift)));
    return diff < 0 ? -m : m;
}
__device__ __forceinline__ int damping_shift(int threshold, int damping) { return threshold ? imax(0, damping - msb(threshold)) : 0; }
// svt_cdef_filter_block_c for one sample: pri the (adjusted) primary strength, sec the secondary, both shifted; sel = (pri >> coeff_shift) & 1
__device__ __forceinline__ int filter_sample(int x, const Taps &t, int pri, int sec, int damping, int coeff_shift) {
    const int sel = (pri >> coeff_shift) & 1, pt0 = sel ? 3 : 4, pt1 = sel ? 3 : 2;
    const int ps = damping_shift(pri, damping), ss = damping_shift(sec, damping);
    int       sum = pt0 * (constrain(t.p[0] - x, pri, ps) + constrain(t.p[1] - x, pri, ps)) + pt1 * (constrain(t.p[2] - x, pri, ps) + constrain(t.p[3] - x, pri, ps));
    sum += 2 * (constrain(t.s[0] - x, sec, ss) + constrain(t.s[1] - x, sec, ss) + constrain(t.s[2] - x, sec, ss) + constrain(t.s[3] - x, sec, ss));
    sum += constrain(t.s[4] - x, sec, ss) + constrain(t.s[5] - x, sec, ss) + constrain(t.s[6] - x, sec, ss) + constrain(t.s[7] - x, sec, ss);
    const int y = x + ((8 + sum - (sum < 0)) >> 4);
    return y < t.mn ? t.mn : (y > t.mx ? t.mx : y);
}
__device__ __forceinline__ int adjust_strength(int strength, int var) {
    const int i = (var >> 6) ? imin(msb(var >> 6), 12) : 0;
    return var ? (strength * (4 + i) + 8) >> 4 : 0;
}
__device__ __forceinline__ int sec_of(int v) { const int s = v & 3; return s + (s == 3); }

// ---- the luma distortion ----
// The correctly rounded square root of an integer x, 20000 <= x < 2^62.  The library root r is within an ulp or so; with r = m * 2^-k, m in
// [2^52, 2^53), sqrt(x) lies above the midpoint to the next double iff x * 2^(2k + 2) > (2m + 1)^2, and below the midpoint to the previous one iff
// x * 2^(2k + 2) < (2m - 1)^2: both sides are integers below 2^110, compared exactly.  (An fma residual x - r * r rounds at the scale of the
// margin it is to decide, so the integer form was kept.)  Equality cannot occur: the right sides are odd.
__device__ __forceinline__ double sqrt_exact(double x) {
    const double   r = sqrt(x);
    const int      k = 52 - ilogb(r);
    uint64_t       m = (uint64_t)ldexp(r, k);
    const unsigned __int128 xs = (unsigned __int128)(uint64_t)x << (2 * k + 2);
    for (int it = 0; it < 4; it++) {
        const unsigned __int128 up = (unsigned __int128)(2 * m + 1) * (2 * m + 1);
        if (xs > up) { m++; continue; }
        if (m == ((uint64_t)1 << 52)) { // the doubles below a power of two lie half as far apart
            const unsigned __int128 dn = (unsigned __int128)(4 * m - 1) * (4 * m - 1);
            if ((xs << 2) < dn) return ldexp((double)(2 * m - 1), -(k + 1));
            break;
        }
        const unsigned __int128 dn = (unsigned __int128)(2 * m - 1) * (2 * m - 1);
        if (xs < dn) { m--; continue; }
        break;
    }
    return ldexp((double)m, -k);
}
// dist_8xn_*_c behind its five sums; "s" is the source, "d" the filtered block (the formula is symmetric in the two)
__device__ __forceinline__ uint64_t luma_dist(uint64_t sum_s, uint64_t sum_d, uint64_t sum_s2, uint64_t sum_d2, uint64_t sum_sd, int cs) {
    const uint64_t svar = sum_s2 - ((sum_s * sum_s + 32) >> 6), dvar = sum_d2 - ((sum_d * sum_d + 32) >> 6);
    const double   num = (double)(sum_d2 + sum_s2 - 2 * sum_sd) * .5 * (double)(svar + dvar + (uint64_t)(400 << 2 * cs));
    const double   den = sqrt_exact((double)(20000 << 4 * cs) + (double)svar * (double)dvar);
    return (uint64_t)floor(.5 + num / den);
}

// ---- the search: luma ----
template <bool HBD> __global__ __launch_bounds__(kThreads) void cdef_search_luma_kernel(const SvtHipCdefSearchDesc d, const int nhfb, const int nvfb) {
    __shared__ uint16_t s_win[kLRows * kLStride];
    __shared__ uint16_t s_src[64 * 64];
    __shared__ uint64_t s_acc[64];
    __shared__ int      s_var[64];
    __shared__ uint8_t  s_dir[64];
    __shared__ int      s_scr[kWaves][128];
    constexpr int  cs = HBD ? 2 : 0;
    const int      fb = (int)blockIdx.x, lane = (int)(threadIdx.x & 63u), wave = uni((int)(threadIdx.x >> 6));
    const FbGeom   g = fb_geom(d.recon[0], fb, nhfb, nvfb, 64);
    const uint64_t mask = d.masks[fb] & valid_mask(g.hs, g.vs);
    if (mask == 0) return; // the whole workgroup: nothing is written for a skipped filter block
    stage_window<HBD>(s_win, kLStride, d.recon[0], g, 64);
    stage_block<HBD>(s_src, d.src[0], g, 64);
    if (threadIdx.x < 64) s_acc[threadIdx.x] = 0;
    const DirLane L = dir_lane(lane);
    __syncthreads();
    const int i = lane >> 3, j = lane & 7;
    // directions: the waves share the listed blocks
    for (int b = wave; b < 64; b += kWaves) {
        if (!((mask >> b) & 1)) continue;
        const int x = s_win[(3 + 8 * (b >> 3) + i) * kLStride + 8 + 8 * (b & 7) + j];
        int       dir, var;
        find_dir((x >> cs) - 128, L, s_scr[wave], lane, dir, var);
        if (lane == 0) {
            s_dir[b] = (uint8_t)dir; s_var[b] = var;
            d.dir[(size_t)fb * 64 + b] = (uint8_t)dir; d.var[(size_t)fb * 64 + b] = var;
        }
    }
    __syncthreads();
    const int  sf = imin((int)d.subsampling_factor, 4), damping = 3 + (d.base_q_idx >> 6) + cs, n = d.n_strengths;
    const bool row_on = (i % sf) == 0;
    bool       any_sec_only = false;
    for (int gi = wave; gi < n; gi += kWaves) any_sec_only |= (d.strength_y[gi] >> 2) == 0;
    for (int b = 0; b < 64; b++) {
        if (!((mask >> b) & 1)) continue;
        const int      pos = (3 + 8 * (b >> 3) + i) * kLStride + 8 + 8 * (b & 7) + j;
        const int      x = s_win[pos], s = s_src[(8 * (b >> 3) + i) * 64 + 8 * (b & 7) + j];
        const int      dir = uni(s_dir[b]), var = uni(s_var[b]);
        const uint64_t sum_s = wave_sum_dpp(row_on ? (uint32_t)s : 0u), sum_s2 = wave_sum_dpp(row_on ? (uint32_t)(s * s) : 0u);
        for (int pass = 0; pass < 2; pass++) { // strengths with a primary part filter along dir, those without along direction 0
            if (pass == 1 && !any_sec_only) break;
            Taps t;
            load_taps(s_win, pos, kLStride, pass ? 0 : dir, x, t);
            for (int gi = wave; gi < n; gi += kWaves) {
                const int v = d.strength_y[gi], pri = (v >> 2) << cs, sec = sec_of(v) << cs;
                if ((pri == 0) != (pass == 1)) continue;
                const int      y = filter_sample(x, t, adjust_strength(pri, var), sec, damping, cs);
                const uint64_t sum_d = wave_sum_dpp(row_on ? (uint32_t)y : 0u), sum_d2 = wave_sum_dpp(row_on ? (uint32_t)(y * y) : 0u);
                const uint64_t sum_sd = wave_sum_dpp(row_on ? (uint32_t)(y * s) : 0u);
                const uint64_t dist = luma_dist(sum_s, sum_d, sum_s2, sum_d2, sum_sd, cs);
                if (lane == 0) {
                    s_acc[gi] += dist;
                    if (d.block_dist) d.block_dist[((size_t)fb * n + gi) * 64 + b] = dist;
                }
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < n) d.mse[(size_t)fb * 64 + threadIdx.x] = (s_acc[threadIdx.x] >> 2 * cs) * (uint64_t)sf; // enc_cdef.c:172: the sum of every plane is shifted
}

// ---- the search: chroma, Cb and Cr in one workgroup; sf is 1 for 4x4 blocks ----
// A wave is a group of four 4x4 blocks: block by * 8 + bx with by = grp >> 1, bx = 4 * (grp & 1) + (lane >> 4); the lane's sample is
// (i, j) = ((lane >> 2) & 3, lane & 3) of it.
template <bool HBD> __global__ __launch_bounds__(kThreads) void cdef_search_chroma_kernel(const SvtHipCdefSearchDesc d, const int nhfb, const int nvfb) {
    __shared__ uint16_t s_win[2][kCRows * kCStride];
    __shared__ uint16_t s_src[2][32 * 32];
    __shared__ uint64_t s_acc[2][64];
    constexpr int  cs = HBD ? 2 : 0;
    const int      fb = (int)blockIdx.x, lane = (int)(threadIdx.x & 63u), wave = uni((int)(threadIdx.x >> 6)), n = d.n_strengths;
    const FbGeom   gl = fb_geom(d.recon[0], fb, nhfb, nvfb, 64);
    const uint64_t mask = d.masks[fb] & valid_mask(gl.hs, gl.vs);
    if (mask == 0) return;
    const FbGeom g = fb_geom(d.recon[1], fb, nhfb, nvfb, 32);
    for (int pl = 0; pl < 2; pl++) {
        stage_window<HBD>(s_win[pl], kCStride, d.recon[1 + pl], g, 32);
        stage_block<HBD>(s_src[pl], d.src[1 + pl], g, 32);
    }
    if (threadIdx.x < 128) s_acc[threadIdx.x >> 6][threadIdx.x & 63] = 0;
    __syncthreads();
    const int q = lane >> 4, i = (lane >> 2) & 3, j = lane & 3, damping = 3 + (d.base_q_idx >> 6) + cs - 1;
    bool      any_sec_only = false, any_pri = false;
    for (int gi = wave; gi < n; gi += kWaves) {
        const int v = d.strength_uv[gi];
        if (v >= 0) { any_sec_only |= (v >> 2) == 0; any_pri |= (v >> 2) != 0; }
    }
    for (int grp = 0; grp < 16; grp++) {
        const int by = grp >> 1, bx = 4 * (grp & 1) + q, b = by * 8 + bx;
        if (uni((int)((mask >> (8 * by + 4 * (grp & 1))) & 15)) == 0) continue;
        const bool on = (mask >> b) & 1;
        const int  dir = on ? d.dir[(size_t)fb * 64 + b] : 0; // the luma launch wrote it
        const int  pos = (3 + 4 * by + i) * kCStride + 8 + 4 * bx + j;
        for (int pl = 0; pl < 2; pl++) {
            const int x = s_win[pl][pos], s = s_src[pl][(4 * by + i) * 32 + 4 * bx + j];
            for (int pass = 0; pass < 2; pass++) {
                if (pass ? !any_sec_only : !any_pri) continue;
                Taps t;
                load_taps(s_win[pl], pos, kCStride, pass ? 0 : dir, x, t);
                for (int gi = wave; gi < n; gi += kWaves) {
                    const int v = d.strength_uv[gi];
                    if (v < 0 || ((v >> 2) == 0) != (pass == 1)) continue;
                    const int      e = filter_sample(x, t, (v >> 2) << cs, sec_of(v) << cs, damping, cs) - s;
                    const uint32_t sum = wave_sum_dpp(on ? (uint32_t)(e * e) : 0u);
                    if (lane == 0) s_acc[pl][gi] += sum;
                }
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < n) {
        const int gi = (int)threadIdx.x;
        d.mse[((size_t)d.n_fb + fb) * 64 + gi] = d.strength_uv[gi] < 0 ? SVT_HIP_CDEF_DEFAULT_MSE_UV : (s_acc[0][gi] >> 2 * cs) + (s_acc[1][gi] >> 2 * cs);
    }
}

// ---- apply: a workgroup per (filter block, plane) ----
template <bool HBD> __global__ __launch_bounds__(kThreads) void cdef_apply_kernel(const SvtHipCdefApplyDesc d, const int nhfb, const int nvfb) {
    __shared__ uint16_t s_win[kLRows * kLStride];
    __shared__ int      s_var[64];
    __shared__ uint8_t  s_dir[64];
    __shared__ int      s_scr[kWaves][128];
    constexpr int  cs = HBD ? 2 : 0;
    const int      fb = (int)blockIdx.x, pli = (int)blockIdx.y, lane = (int)(threadIdx.x & 63u), wave = uni((int)(threadIdx.x >> 6));
    const FbGeom   gl = fb_geom(d.in[0], fb, nhfb, nvfb, 64);
    const uint64_t mask = d.masks[fb] & valid_mask(gl.hs, gl.vs);
    const int      bs = pli ? 32 : 64;
    const FbGeom   g = pli ? fb_geom(d.in[pli], fb, nhfb, nvfb, 32) : gl;
    int            pri = 0, sec = 0;
    bool           filter = false;
    if (mask) {
        const int idx = d.fb_strength[fb] & 7, vy = d.y_strength[idx], vuv = d.uv_strength[idx], v = pli ? vuv : vy;
        pri = (v >> 2) << cs; sec = sec_of(v) << cs;
        filter = (pri | sec) != 0; // with all four strengths 0 this holds for no plane
    }
    if (!filter) { // the filter block, or this plane of it, is copied through
        for (int idx = (int)threadIdx.x; idx < bs * bs; idx += kThreads) {
            const int r = idx / bs, c = idx - r * bs;
            if (r < g.vs && c < g.hs) {
                const size_t at = (size_t)(g.y0 + r), col = (size_t)(g.x0 + c);
                store_at<HBD>(d.out[pli].plane, at * d.out[pli].stride + col, sample_at<HBD>(d.in[pli].plane, at * d.in[pli].stride + col));
            }
        }
        return;
    }
    // luma's directions, in every plane's workgroup
    stage_window<HBD>(s_win, kLStride, d.in[0], gl, 64);
    const DirLane L = dir_lane(lane);
    __syncthreads();
    for (int b = wave; b < 64; b += kWaves) {
        if (!((mask >> b) & 1)) continue;
        const int x = s_win[(3 + 8 * (b >> 3) + (lane >> 3)) * kLStride + 8 + 8 * (b & 7) + (lane & 7)];
        int       dir, var;
        find_dir((x >> cs) - 128, L, s_scr[wave], lane, dir, var);
        if (lane == 0) { s_dir[b] = (uint8_t)dir; s_var[b] = var; }
    }
    __syncthreads();
    const int damping = d.cdef_damping + cs - (pli != 0);
    if (pli == 0) {
        const int i = lane >> 3, j = lane & 7;
        for (int b = wave; b < 64; b += kWaves) {
            const int by = b >> 3, bx = b & 7;
            if (8 * by >= g.vs || 8 * bx >= g.hs) continue;
            const int pos = (3 + 8 * by + i) * kLStride + 8 + 8 * bx + j, x = s_win[pos];
            int       y = x;
            if ((mask >> b) & 1) {
                Taps t;
                load_taps(s_win, pos, kLStride, pri ? uni(s_dir[b]) : 0, x, t);
                y = filter_sample(x, t, adjust_strength(pri, uni(s_var[b])), sec, damping, cs);
            }
            store_at<HBD>(d.out[0].plane, (size_t)(g.y0 + 8 * by + i) * d.out[0].stride + (size_t)(g.x0 + 8 * bx + j), y);
        }
        return;
    }
    __syncthreads(); // every wave has read the luma window
    stage_window<HBD>(s_win, kCStride, d.in[pli], g, 32);
    __syncthreads();
    const int q = lane >> 4, i = (lane >> 2) & 3, j = lane & 3;
    for (int grp = wave; grp < 16; grp += kWaves) {
        const int by = grp >> 1, bx = 4 * (grp & 1) + q, b = by * 8 + bx;
        if (4 * by >= g.vs || 4 * bx >= g.hs) continue; // per lane
        const int pos = (3 + 4 * by + i) * kCStride + 8 + 4 * bx + j, x = s_win[pos];
        int       y = x;
        if ((mask >> b) & 1) {
            Taps t;
            load_taps(s_win, pos, kCStride, pri ? s_dir[b] : 0, x, t);
            y = filter_sample(x, t, pri, sec, damping, cs);
        }
        store_at<HBD>(d.out[pli].plane, (size_t)(g.y0 + 4 * by + i) * d.out[pli].stride + (size_t)(g.x0 + 4 * bx + j), y);
    }
}

// ---- pick ----
// work: PickState | uint64 tot[64][64] | uint64 base[n_fb]
struct PickState {
    uint64_t best_cost, zero_cost;
    uint32_t sb_count;
    int32_t  best_bits;
    int32_t  lev0[8], lev1[8];   // the call's lists; the call to come reads the first `chosen`
    int32_t  best0[8], best1[8]; // of the winning bit count, as indices
    int32_t  chosen, reserved;
};
struct PickWork { PickState *st; unsigned long long *tot; uint64_t *base; };
__host__ __device__ inline PickWork pick_work(void *p) {
    PickWork w;
    w.st   = (PickState *)p;
    w.tot  = (unsigned long long *)((char *)p + 256);
    w.base = (uint64_t *)((char *)p + 256 + 64 * 64 * 8);
    return w;
}
static_assert(sizeof(PickState) <= 256, "the state has 256 bytes of the scratch");
constexpr size_t kPickMaxFb = 65536;
inline size_t    pick_work_bytes() { return 256 + 64 * 64 * 8 + kPickMaxFb * 8; }

__device__ __forceinline__ uint64_t rdcost(uint64_t lambda, int64_t rate, uint64_t dist) { // RDCOST, rd_cost.h:37
    return (uint64_t)(((rate * (int64_t)lambda + 256) >> 9) + ((int64_t)dist * 128));
}
__device__ __forceinline__ uint64_t biased(uint64_t mse, int bias, bool hbd) { // enc_cdef.c:846-885
    int f = bias;
    if (hbd) {
        if (mse < 5000) f = imin(f - 10, 64);
        else if (mse < 10000) f = imin(f - 5, 64);
        else if (mse > 25000) f = imin(f + 1, 64);
    } else {
        if (mse > 25000) f = imin(f + 2, 64);
        else if (mse > 10000) f = imin(f + 1, 64);
    }
    return ((uint64_t)f * mse) >> 6;
}
// a filter block the search did not skip: its mask lists a block inside the picture
__device__ __forceinline__ bool pick_live(const SvtHipCdefPickDesc &d, uint32_t i) {
    const uint32_t nhfb = (d.width + 63u) >> 6;
    const int      hs = imin(64, (int)d.width - 64 * (int)(i % nhfb)), vs = imin(64, (int)d.height - 64 * (int)(i / nhfb));
    return (d.masks[i] & valid_mask(hs, vs)) != 0;
}
// the baseline of a filter block: the best of the pairs already chosen
__device__ __forceinline__ uint64_t baseline(const uint64_t *m0, const uint64_t *m1, const int32_t *lev0, const int32_t *lev1, int chosen) {
    uint64_t best = kNone;
    for (int gi = 0; gi < chosen; gi++) {
        const uint64_t cur = m0[lev0[gi]] + m1[lev1[gi]];
        if (cur < best) best = cur;
    }
    return best;
}

__global__ __launch_bounds__(kThreads) void cdef_pick_init_kernel(const SvtHipCdefPickDesc d) {
    __shared__ uint64_t s_sum[kThreads];
    __shared__ uint32_t s_cnt[kThreads];
    const PickWork w = pick_work(d.work);
    uint64_t      *m0 = d.mse, *m1 = d.mse + (size_t)d.n_fb * 64;
    uint64_t       sum = 0;
    uint32_t       cnt = 0;
    for (uint32_t i = threadIdx.x; i < d.n_fb; i += kThreads) {
        w.base[i] = kNone;
        if (!pick_live(d, i)) continue;
        if (d.zero_fs_cost_bias) {
            m0[(size_t)i * 64] = biased(m0[(size_t)i * 64], (int)d.zero_fs_cost_bias, d.is_hbd != 0);
            m1[(size_t)i * 64] = biased(m1[(size_t)i * 64], (int)d.zero_fs_cost_bias, d.is_hbd != 0);
        }
        sum += m0[(size_t)i * 64] + m1[(size_t)i * 64];
        cnt++;
    }
    for (uint32_t i = threadIdx.x; i < 64 * 64; i += kThreads) w.tot[i] = 0;
    s_sum[threadIdx.x] = sum; s_cnt[threadIdx.x] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kThreads; k++) { sum += s_sum[k]; cnt += s_cnt[k]; }
        PickState *st = w.st;
        memset(st, 0, sizeof(*st));
        st->best_cost = kNone;
        st->zero_cost = rdcost(d.full_lambda, 512 * 12, sum << 4);
        st->sb_count  = cnt;
    }
}

// tot[j][k] += min(base_i, mse0[i][j] + mse1[i][k]) over the filter blocks of the slice
__global__ __launch_bounds__(kThreads) void cdef_pick_tot_kernel(const SvtHipCdefPickDesc d, const int slices) {
    __shared__ uint64_t s_part[kWaves][64];
    const PickWork  w = pick_work(d.work);
    const int       j = (int)blockIdx.x, k = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6), n = (int)d.n_strengths;
    const uint64_t *m0 = d.mse, *m1 = d.mse + (size_t)d.n_fb * 64;
    uint64_t        tot = 0;
    for (uint32_t i = blockIdx.y * kWaves + wave; i < d.n_fb; i += (uint32_t)slices * kWaves) {
        if (k >= n || !pick_live(d, i)) continue;
        const uint64_t cur = m0[(size_t)i * 64 + j] + m1[(size_t)i * 64 + k], best = w.base[i];
        tot += cur < best ? cur : best;
    }
    s_part[wave][k] = tot;
    __syncthreads();
    if (threadIdx.x < 64 && k < n) {
        for (int p = 1; p < kWaves; p++) tot += s_part[p][k];
        if (tot) atomicAdd(w.tot + j * 64 + k, (unsigned long long)tot);
    }
}

// Behind call `step` of bit count `bits` (nb = 1 << bits pairs; steps 0 .. nb - 1 add, nb .. 5 nb - 1 drop the oldest and re-add)
__global__ __launch_bounds__(kThreads) void cdef_pick_decide_kernel(const SvtHipCdefPickDesc d, const int bits, const int step) {
    __shared__ uint64_t s_val[kThreads];
    __shared__ int      s_idx[kThreads];
    const PickWork  w = pick_work(d.work);
    PickState      *st = w.st;
    const int       n = (int)d.n_strengths, nb = 1 << bits;
    const uint64_t *m0 = d.mse, *m1 = d.mse + (size_t)d.n_fb * 64;
    // the first minimum of tot in (j, k) raster order, strict < from 1 << 63
    uint64_t val = kNone;
    int      at = 0;
    for (int e = (int)threadIdx.x; e < n * n; e += kThreads) {
        const uint64_t t = w.tot[(e / n) * 64 + e % n];
        if (t < val) { val = t; at = e; }
    }
    s_val[threadIdx.x] = val; s_idx[threadIdx.x] = at;
    __syncthreads();
    for (int e = (int)threadIdx.x; e < 64 * 64; e += kThreads) w.tot[e] = 0; // for the call to come
    const bool last = bits == 3 && step == 5 * nb - 1;
    if (threadIdx.x == 0) {
        for (int k = 1; k < kThreads; k++)
            if (s_val[k] < val || (s_val[k] == val && val != kNone && s_idx[k] < at)) { val = s_val[k]; at = s_idx[k]; }
        const int chosen = st->chosen;
        st->lev0[chosen] = at / n; st->lev1[chosen] = at % n;
        if (step == 5 * nb - 1) { // the bit count's last call: its cost against the best so far
            const uint64_t cost = rdcost(d.full_lambda, (int64_t)512 * ((int64_t)st->sb_count * bits + nb * 12), val * 16);
            if (cost < st->best_cost) {
                st->best_cost = cost; st->best_bits = bits;
                for (int q = 0; q < nb; q++) { st->best0[q] = st->lev0[q]; st->best1[q] = st->lev1[q]; }
            }
            st->chosen = 0;
        } else if (step + 1 < nb) {
            st->chosen = step + 1;
        } else {
            for (int q = 0; q < nb - 1; q++) { st->lev0[q] = st->lev0[q + 1]; st->lev1[q] = st->lev1[q + 1]; }
            st->chosen = nb - 1;
        }
        if (last) {
            SvtHipCdefPick *r = d.result;
            r->cdef_bits = st->best_bits; r->nb_strengths = 1 << st->best_bits;
            for (int q = 0; q < SVT_HIP_CDEF_MAX_PAIRS; q++) {
                r->y_strength[q]  = q < r->nb_strengths ? d.filter_map_y[st->best0[q]] : 0;
                r->uv_strength[q] = q < r->nb_strengths ? d.filter_map_uv[st->best1[q]] : 0;
            }
            r->best_cost = st->best_cost; r->zero_cost = st->zero_cost;
            r->cdef_dist_dev = st->zero_cost == 0 ? 0 : (int32_t)(1000 - ((1000 * st->best_cost) / st->zero_cost));
            r->reserved = 0;
        }
    }
    __syncthreads();
    __threadfence_block();
    if (!last) {
        const int chosen = st->chosen;
        for (uint32_t i = threadIdx.x; i < d.n_fb; i += kThreads)
            if (pick_live(d, i)) w.base[i] = baseline(m0 + (size_t)i * 64, m1 + (size_t)i * 64, st->lev0, st->lev1, chosen);
        return;
    }
    const int nbest = 1 << st->best_bits;
    for (uint32_t i = threadIdx.x; i < d.n_fb; i += kThreads) {
        if (!pick_live(d, i)) continue;
        uint64_t best = kNone;
        int      gi_best = 0;
        for (int gi = 0; gi < nbest; gi++) {
            const uint64_t cur = m0[(size_t)i * 64 + st->best0[gi]] + m1[(size_t)i * 64 + st->best1[gi]];
            if (cur < best) { best = cur; gi_best = gi; }
        }
        d.fb_strength[i] = (int8_t)gi_best;
    }
}

// ---- host ----
int check_planes(const char *who, const char *a_name, const SvtHipCdefPlane *a, const char *b_name, const SvtHipCdefPlane *b, int n_planes) {
    for (int k = 0; k < 2; k++) {
        const SvtHipCdefPlane *p = k ? b : a;
        const char            *name = k ? b_name : a_name;
        for (int i = 0; i < n_planes; i++) {
            if (!p[i].plane) BAD("%s: %s plane %d is null", who, name, i);
            if (p[i].width == 0 || p[i].height == 0 || p[i].stride < p[i].width)
                BAD("%s: %s plane %d: %u x %u, stride %u (a size, stride >= width)", who, name, i, p[i].width, p[i].height, p[i].stride);
            if (i && (p[i].width * 2 != p[0].width || p[i].height * 2 != p[0].height))
                BAD("%s: %s plane %d: %u x %u, half of luma's %u x %u is wanted (4:2:0)", who, name, i, p[i].width, p[i].height, p[0].width, p[0].height);
        }
    }
    if ((a[0].width & 7) || (a[0].height & 7) || a[0].width > 16384 || a[0].height > 16384)
        BAD("%s: picture %u x %u (multiples of 8, at most 16384)", who, a[0].width, a[0].height);
    for (int i = 0; i < n_planes; i++)
        if (a[i].width != b[i].width || a[i].height != b[i].height)
            BAD("%s: plane %d: %s %u x %u, %s %u x %u", who, i, a_name, a[i].width, a[i].height, b_name, b[i].width, b[i].height);
    return SVT_HIP_OK;
}
inline uint32_t fb_count(const SvtHipCdefPlane &luma) { return ceil_div(luma.width, 64) * ceil_div(luma.height, 64); }

} // namespace

extern "C" {

int svt_hip_cdef_search_check_desc(const SvtHipCdefSearchDesc *d) {
    static const char who[] = "svt_hip_cdef_search_check_desc";
    if (!d) BAD("%s: null descriptor", who);
    if (!d->masks || !d->mse || !d->dir || !d->var) BAD("%s: a mandatory pointer (masks, mse, dir, var) is null", who);
    if (d->bit_depth != 8 && d->bit_depth != 10) BAD("%s: bit_depth %u (8 or 10)", who, d->bit_depth);
    if (d->subsampling_factor != 1 && d->subsampling_factor != 2 && d->subsampling_factor != 4)
        BAD("%s: subsampling_factor %u (1, 2 or 4)", who, d->subsampling_factor);
    if (d->n_strengths == 0 || d->n_strengths > SVT_HIP_CDEF_MAX_STRENGTHS) BAD("%s: n_strengths %u (1 .. %d)", who, d->n_strengths, SVT_HIP_CDEF_MAX_STRENGTHS);
    for (int i = 0; i < d->n_strengths; i++)
        if (d->strength_y[i] < 0 || d->strength_y[i] > 63 || d->strength_uv[i] < -1 || d->strength_uv[i] > 63)
            BAD("%s: strength %d: luma %d (0 .. 63), chroma %d (-1 .. 63)", who, i, d->strength_y[i], d->strength_uv[i]);
    if (const int rc = check_planes(who, "reconstruction", d->recon, "source", d->src, 3)) return rc;
    if (d->n_fb && d->n_fb != fb_count(d->recon[0])) BAD("%s: n_fb %u, the picture has %u filter blocks", who, d->n_fb, fb_count(d->recon[0]));
    return SVT_HIP_OK;
}

int svt_hip_cdef_pick_check_desc(const SvtHipCdefPickDesc *d) {
    static const char who[] = "svt_hip_cdef_pick_check_desc";
    if (!d) BAD("%s: null descriptor", who);
    if (!d->masks || !d->mse || !d->work || !d->result || !d->fb_strength) BAD("%s: a mandatory pointer (masks, mse, work, result, fb_strength) is null", who);
    if (((uintptr_t)d->work & 7) != 0) BAD("%s: work is not 8-byte aligned", who);
    if (d->n_strengths == 0 || d->n_strengths > SVT_HIP_CDEF_MAX_STRENGTHS) BAD("%s: n_strengths %u (1 .. %d)", who, d->n_strengths, SVT_HIP_CDEF_MAX_STRENGTHS);
    if (d->is_hbd > 1) BAD("%s: is_hbd %u (0 or 1)", who, d->is_hbd);
    if (d->zero_fs_cost_bias && (d->zero_fs_cost_bias < 10 || d->zero_fs_cost_bias > 64)) BAD("%s: zero_fs_cost_bias %u (0, or 10 .. 64)", who, d->zero_fs_cost_bias);
    if (d->width == 0 || d->height == 0 || (d->width & 7) || (d->height & 7) || d->width > 16384 || d->height > 16384)
        BAD("%s: picture %u x %u (multiples of 8, at most 16384)", who, d->width, d->height);
    const uint32_t count = ceil_div(d->width, 64) * ceil_div(d->height, 64);
    if (d->n_fb && d->n_fb != count) BAD("%s: n_fb %u, the picture has %u filter blocks", who, d->n_fb, count);
    return SVT_HIP_OK;
}

int svt_hip_cdef_apply_check_desc(const SvtHipCdefApplyDesc *d) {
    static const char who[] = "svt_hip_cdef_apply_check_desc";
    if (!d) BAD("%s: null descriptor", who);
    if (!d->masks || !d->fb_strength || !d->y_strength || !d->uv_strength) BAD("%s: a mandatory pointer (masks, fb_strength, y_strength, uv_strength) is null", who);
    if (d->bit_depth != 8 && d->bit_depth != 10) BAD("%s: bit_depth %u (8 or 10)", who, d->bit_depth);
    if (d->cdef_damping < 3 || d->cdef_damping > 6) BAD("%s: cdef_damping %u (3 .. 6)", who, d->cdef_damping);
    if (d->n_planes != 1 && d->n_planes != 3) BAD("%s: n_planes %u (1 or 3)", who, d->n_planes);
    if (const int rc = check_planes(who, "input", d->in, "output", d->out, d->n_planes)) return rc;
    const size_t bytes = d->bit_depth == 10 ? 2 : 1;
    struct Span { uintptr_t lo, hi; } span[6];
    for (int i = 0; i < 2 * d->n_planes; i++) {
        const SvtHipCdefPlane *p = i < d->n_planes ? &d->in[i] : &d->out[i - d->n_planes];
        span[i].lo = (uintptr_t)p->plane;
        span[i].hi = span[i].lo + (((size_t)p->height - 1) * p->stride + p->width) * bytes;
    }
    for (int o = d->n_planes; o < 2 * d->n_planes; o++)
        for (int i = 0; i < o; i++)
            if (span[o].lo < span[i].hi && span[i].lo < span[o].hi)
                BAD("%s: output plane %d overlaps %s plane %d (the filter runs out of place)", who, o - d->n_planes, i < d->n_planes ? "input" : "output", i < d->n_planes ? i : i - d->n_planes);
    if (d->n_fb && d->n_fb != fb_count(d->in[0])) BAD("%s: n_fb %u, the picture has %u filter blocks", who, d->n_fb, fb_count(d->in[0]));
    return SVT_HIP_OK;
}

size_t svt_hip_cdef_pick_work_bytes(void) { return pick_work_bytes(); }

size_t svt_hip_cdef_layout(int what, int field) {
#define P(f) offsetof(SvtHipCdefPlane, f)
#define S(f) offsetof(SvtHipCdefSearchDesc, f)
#define R(f) offsetof(SvtHipCdefPick, f)
#define K(f) offsetof(SvtHipCdefPickDesc, f)
#define A(f) offsetof(SvtHipCdefApplyDesc, f)
    static const size_t plane[]  = {P(plane), P(stride), P(width), P(height), P(reserved)};
    static const size_t search[] = {S(n_fb), S(bit_depth), S(base_q_idx), S(subsampling_factor), S(n_strengths), S(recon), S(src), S(strength_y), S(strength_uv),
                                    S(masks), S(mse), S(dir), S(var), S(block_dist)};
    static const size_t pick[]   = {R(cdef_bits), R(nb_strengths), R(y_strength), R(uv_strength), R(best_cost), R(zero_cost), R(cdef_dist_dev), R(reserved)};
    static const size_t pdesc[]  = {K(n_fb), K(n_strengths), K(is_hbd), K(zero_fs_cost_bias), K(full_lambda), K(width), K(height), K(reserved), K(filter_map_y), K(filter_map_uv),
                                    K(masks), K(mse), K(work), K(result), K(fb_strength)};
    static const size_t apply[]  = {A(n_fb), A(bit_depth), A(cdef_damping), A(n_planes), A(reserved), A(in), A(out), A(masks), A(fb_strength), A(y_strength),
                                    A(uv_strength)};
#undef P
#undef S
#undef R
#undef K
#undef A
    const SvtHipLayoutRow rows[] = {layout_row<SvtHipCdefPlane>(plane), layout_row<SvtHipCdefSearchDesc>(search), layout_row<SvtHipCdefPick>(pick),
                                    layout_row<SvtHipCdefPickDesc>(pdesc), layout_row<SvtHipCdefApplyDesc>(apply)};
    return layout_lookup(rows, what, field);
}

int svt_hip_cdef_search_batch(SvtHipContext *ctx, const SvtHipCdefSearchDesc *d) {
    return enqueue_batch("svt_hip_cdef_search_batch", ctx, d, svt_hip_cdef_search_check_desc, &SvtHipCdefSearchDesc::n_fb, [=] {
        const int nhfb = (int)ceil_div(d->recon[0].width, 64), nvfb = (int)ceil_div(d->recon[0].height, 64);
        hipLaunchKernelGGL(pick_hbd(d->bit_depth, cdef_search_luma_kernel<true>, cdef_search_luma_kernel<false>), dim3(d->n_fb), dim3(kThreads), 0, ctx->stream, *d,
                           nhfb, nvfb);
        hipLaunchKernelGGL(pick_hbd(d->bit_depth, cdef_search_chroma_kernel<true>, cdef_search_chroma_kernel<false>), dim3(d->n_fb), dim3(kThreads), 0, ctx->stream,
                           *d, nhfb, nvfb);
    });
}

int svt_hip_cdef_pick_batch(SvtHipContext *ctx, const SvtHipCdefPickDesc *d) {
    return enqueue_batch("svt_hip_cdef_pick_batch", ctx, d, svt_hip_cdef_pick_check_desc, &SvtHipCdefPickDesc::n_fb, [=] {
        const int slices = (int)(ceil_div(d->n_fb, 64) < (uint32_t)kMaxSlices ? ceil_div(d->n_fb, 64) : (uint32_t)kMaxSlices);
        hipLaunchKernelGGL(cdef_pick_init_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, *d);
        for (int bits = 0; bits <= 3; bits++)
            for (int step = 0; step < 5 << bits; step++) {
                hipLaunchKernelGGL(cdef_pick_tot_kernel, dim3(d->n_strengths, slices), dim3(kThreads), 0, ctx->stream, *d, slices);
                hipLaunchKernelGGL(cdef_pick_decide_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, *d, bits, step);
            }
    });
}

int svt_hip_cdef_apply_batch(SvtHipContext *ctx, const SvtHipCdefApplyDesc *d) {
    return enqueue_batch("svt_hip_cdef_apply_batch", ctx, d, svt_hip_cdef_apply_check_desc, &SvtHipCdefApplyDesc::n_fb, [=] {
        const int nhfb = (int)ceil_div(d->in[0].width, 64), nvfb = (int)ceil_div(d->in[0].height, 64);
        hipLaunchKernelGGL(pick_hbd(d->bit_depth, cdef_apply_kernel<true>, cdef_apply_kernel<false>), dim3(d->n_fb, d->n_planes), dim3(kThreads), 0, ctx->stream, *d,
                           nhfb, nvfb);
    });
}

} // extern "C"
