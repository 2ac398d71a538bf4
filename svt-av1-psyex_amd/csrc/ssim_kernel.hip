// ssim_kernel.hip -- the SSIM distortion of the SSIM tunes (--tune 2 / 3 / 4) on gfx950: svt_hip_ssim_batch and the pointer-level
// entries svt_ssim_{8x8,4x4}{,_hbd}_hip, svt_spatial_full_distortion_ssim_kernel_hip of include/svt_hip_leaf.h.
//
// Reference functions restated (Source/Lib):
//   svt_ssim_{8x8,4x4}{,_hbd}_c                                  Codec/mode_decision.c:4682-4780
//   similarity                                                   Codec/enc_dec_process.c:709-735
//   ssim, ssim_hbd, ssim_{8x8,4x4}_blocks{,_hbd}                 Codec/mode_decision.c:4781-4878
//   svt_spatial_full_distortion_ssim_kernel                      Codec/mode_decision.c:4879-4921
//   svt_psy_distortion / svt_psy_distortion_hbd (psy term)       Codec/psy_rd.c:135-274 (psy_energy.h)
//
// One wave per job (or per 64x64 region of the pyramid form).  Lane groups take tiles side by side -- 8 lanes per 8x8 tile (one row each),
// 4 lanes per 4x4 tile -- and reduce the five 32-bit moments inside the group by DPP (the sums wrap modulo 2^32 like the reference's).  The
// group's first lane turns them into the tile's score and keeps the clamped score in LDS.  One lane per output then adds the scores in the
// block's raster order, divides by the tile count and forms the distortion.
//
// Exactness: the reference is fp64 evaluated operation by operation (gcc on x86-64, no FMA).  Contraction is off in this file (a fused
// a * b + c rounds once, not twice), division is the default correctly rounded one, and the mean is the ordered sum the reference's loop
// makes -- a tree of the same scores rounds differently.  The integer moments are exact in any order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <mutex>
#include "svt_hip_internal.h"
#include "batch_host.h"
#include "leaf_guard.h"
#include "psy_energy.h"
#include "wave_ops.h"
#include "../../include/svt_hip_dsp.h"
#include "../../include/svt_hip_leaf.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxTiles = 1024; // 4x4 tiles of a block of at most 128x128 samples

struct SsimParams {
    SvtHipSsimBatchDesc d;
    int unclamped; // the pointer-level tile entries: the raw score of a one-tile job (svt_ssim_*_c return it unclamped)
};

// C's truncating double -> uint64_t conversion of 0 <= x < 2^64, as two exact 32-bit halves (the compiler's own lowering has an fma in it;
// this one is exact without: hi * 2^32 is exact and so is x - hi * 2^32, a multiple of x's ulp below 2^32)
__device__ __forceinline__ u64 f64_to_u64(double x) {
    const double hi = __builtin_floor(x * 0x1p-32);
    const double lo = x - hi * 0x1p32;
    return ((u64)(uint32_t)hi << 32) + (u64)(uint32_t)lo;
}

// similarity (enc_dec_process.c:709-735) for count = kCount and bd = kBd, operation for operation
template <int kCount, int kBd>
__device__ __forceinline__ double similarity(uint32_t sum_s, uint32_t sum_r, uint32_t sum_sq_s, uint32_t sum_sq_r, uint32_t sum_sxr) {
    constexpr int64_t cc1 = kBd == 8 ? 26634 : 428658, cc2 = kBd == 8 ? 239708 : 3857925;
    constexpr int64_t c1 = (cc1 * kCount * kCount) >> 12, c2 = (cc2 * kCount * kCount) >> 12;
    const int count = kCount;
    const double ssim_n = (2.0 * sum_s * sum_r + c1) * (2.0 * count * sum_sxr - 2.0 * sum_s * sum_r + c2);
    const double ssim_d = ((double)sum_s * sum_s + (double)sum_r * sum_r + c1) *
                          ((double)count * sum_sq_s - (double)sum_s * sum_s + (double)count * sum_sq_r - (double)sum_r * sum_r + c2);
    return ssim_n / ssim_d;
}

// the five moments of one row of N samples of a tile (uint32_t, wrapping like the reference's accumulators)
template <typename Pix, int N> __device__ __forceinline__ void row_moments(const Pix *s, const Pix *r, uint32_t m[5]) {
#pragma unroll
    for (int j = 0; j < N; j++) {
        const uint32_t a = s[j], b = r[j];
        m[0] += a; m[1] += b; m[2] += a * a; m[3] += b * b; m[4] += a * b;
    }
}

// the clamped scores of the (w / N) x (h / N) tiles of the block at s / r, into sc[] in raster order.  Every lane of the wave calls it.
template <typename Pix, int N>
__device__ __forceinline__ void tile_scores(const Pix *s, uint32_t sp, const Pix *r, uint32_t rp, int w, int h, double *sc, int lane, bool clamp) {
    constexpr int G = 64 / N; // tiles side by side
    const int ntx = w / N, nt = ntx * (h / N);
    const int g = lane / N, row = lane % N;
    for (int t0 = 0; t0 < nt; t0 += G) { // uniform
        const int t = t0 + g;
        uint32_t m[5] = {0, 0, 0, 0, 0};
        if (t < nt) {
            const int ty = t / ntx, tx = t - ty * ntx;
            row_moments<Pix, N>(s + (size_t)(N * ty + row) * sp + N * tx, r + (size_t)(N * ty + row) * rp + N * tx, m);
        }
#pragma unroll
        for (int k = 0; k < 5; k++) m[k] = N == 8 ? oct_sum(m[k]) : quad_sum(m[k]);
        if (row == 0 && t < nt) {
            double v = similarity<N * N, sizeof(Pix) == 1 ? 8 : 10>(m[0], m[1], m[2], m[3], m[4]);
            if (clamp) v = v < 0 ? 0 : (v > 1 ? 1 : v); // CLIP3(0, 1, v)
            sc[t] = v;
        }
    }
}

// the outputs of one block: its mean score, and (1 - ssim) * count * 100 * 7 * m [+ (uint64_t)(psy energy * psy_rd)]
__device__ __forceinline__ void ssim_write(const SsimParams &p, uint32_t slot, double ssim, uint32_t count, u64 psy_energy) {
    if (p.d.ssim) p.d.ssim[slot] = ssim;
    if (p.d.ssim_dist) {
        const uint8_t m = p.d.bit_depth == 8 ? 1 : 8;
        u64 dist = f64_to_u64((1 - ssim) * count * 100 * 7 * m);
        if (p.d.psy_rd > 0.0) dist += f64_to_u64((double)psy_energy * p.d.psy_rd);
        p.d.ssim_dist[slot] = dist;
    }
}
__device__ __forceinline__ void ssim_write_bad(const SsimParams &p, uint32_t slot) { // a job the host check would have refused: no sample is read
    if (p.d.ssim) p.d.ssim[slot] = -1.0;
    if (p.d.ssim_dist) p.d.ssim_dist[slot] = ~0ull;
}
__device__ __forceinline__ bool job_ok(const SvtHipBlockJob &jb) {
    return jb.width >= 4 && jb.width <= 128 && !(jb.width & 3) && jb.height >= 4 && jb.height <= 128 && !(jb.height & 3) && !jb.subpel_x && !jb.subpel_y;
}

// one plain job by one wave
template <typename Pix> __device__ __forceinline__ void ssim_job(const SsimParams &p, double *sc, uint32_t job, int lane) {
    const SvtHipBlockJob jb = p.d.jobs[job];
    if (!job_ok(jb)) {
        if (lane == 0) ssim_write_bad(p, job);
        return;
    }
    const int  w = jb.width, h = jb.height;
    const Pix *s = static_cast<const Pix *>(p.d.src) + jb.src_offset, *r = static_cast<const Pix *>(p.d.ref) + jb.ref_offset;
    const bool t8 = !(w & 7) && !(h & 7); // ssim(): 8x8 tiles when both sides are multiples of 8
    if (t8) tile_scores<Pix, 8>(s, p.d.src_stride, r, p.d.ref_stride, w, h, sc, lane, !p.unclamped);
    else tile_scores<Pix, 4>(s, p.d.src_stride, r, p.d.ref_stride, w, h, sc, lane, !p.unclamped);
    u64 e = 0;
    if (p.d.ssim_dist && p.d.psy_rd > 0.0) { // svt_psy_distortion{,_hbd}: one lane per 8x8 (or 4x4) tile of the reference's loops
        const int n = (w >= 8 && h >= 8) ? 8 : 4, ntx = (w + n - 1) / n, nt = ntx * ((h + n - 1) / n);
        for (int t = lane; t < nt; t += 64) {
            const int ty = t / ntx, tx = t - ty * ntx;
            const View<Pix> sv = {s + (size_t)(n * ty) * p.d.src_stride + n * tx, p.d.src_stride, 0, 0};
            const View<Pix> rv = {r + (size_t)(n * ty) * p.d.ref_stride + n * tx, p.d.ref_stride, 0, 0};
            int32_t a, b;
            [[clang::always_inline]] a = psy_tile_energy<Pix>(sv, n); // a call would pass the views through scratch
            [[clang::always_inline]] b = psy_tile_energy<Pix>(rv, n);
            e += (u64)(uint32_t)(a > b ? a - b : b - a);
        }
        e = wave_sum(e);
        e = sizeof(Pix) == 1 ? e >> 1 : e << 2;
    }
    wave_sync();
    if (lane == 0) { // ssim_{8x8,4x4}_blocks: the ordered sum of the clamped scores, then the division by the tile count
        const int nt = t8 ? (w >> 3) * (h >> 3) : (w >> 2) * (h >> 2);
        double tot = 0;
        for (int t = 0; t < nt; t++) tot += sc[t];
        tot /= nt;
        ssim_write(p, job, tot, (uint32_t)(w * h), e);
    }
}

// one 64x64 region by one wave: its 64 8x8 tile scores (and psy tile energies) once, then the 85 nested blocks, one lane each, every block
// adding its own tiles in its own raster order.  Slot of nested block z: out0 + z, z = 0 (64x64), 1 + raster (32x32), 5 + raster (16x16),
// 21 + raster (8x8) -- the layout of SvtHipBlockStatsDesc's pyramids.
template <typename Pix> __device__ __forceinline__ void ssim_pyramid(const SsimParams &p, double *sc, uint32_t *e8, uint32_t reg, int lane) {
    const uint32_t       out0 = p.d.pyramid_out_base + SVT_HIP_PYRAMID_BLOCKS * reg;
    const SvtHipBlockJob jb   = p.d.pyramids[reg];
    if (jb.width != 64 || jb.height != 64 || jb.subpel_x || jb.subpel_y) {
        for (int z = lane; z < SVT_HIP_PYRAMID_BLOCKS; z += 64) ssim_write_bad(p, out0 + z);
        return;
    }
    const Pix *s = static_cast<const Pix *>(p.d.src) + jb.src_offset, *r = static_cast<const Pix *>(p.d.ref) + jb.ref_offset;
    tile_scores<Pix, 8>(s, p.d.src_stride, r, p.d.ref_stride, 64, 64, sc, lane, true);
    const bool psy = p.d.ssim_dist && p.d.psy_rd > 0.0;
    if (psy) { // lane <-> 8x8 tile in raster order (every nested block is 8x8 or larger: the psy tiles are 8x8)
        const int ty = lane >> 3, tx = lane & 7;
        const View<Pix> sv = {s + (size_t)(8 * ty) * p.d.src_stride + 8 * tx, p.d.src_stride, 0, 0};
        const View<Pix> rv = {r + (size_t)(8 * ty) * p.d.ref_stride + 8 * tx, p.d.ref_stride, 0, 0};
        int32_t a, b;
        [[clang::always_inline]] a = psy_tile_energy<Pix>(sv, 8);
        [[clang::always_inline]] b = psy_tile_energy<Pix>(rv, 8);
        e8[lane] = (uint32_t)(a > b ? a - b : b - a);
    }
    wave_sync();
    for (int z = lane; z < SVT_HIP_PYRAMID_BLOCKS; z += 64) {
        int n, k;
        if (z == 0) { n = 64; k = 0; }
        else if (z < 5) { n = 32; k = z - 1; }
        else if (z < 21) { n = 16; k = z - 5; }
        else { n = 8; k = z - 21; }
        const int m = n >> 3, per_row = 8 / m, ty0 = (k / per_row) * m, tx0 = (k % per_row) * m; // the block's tiles: m x m from (ty0, tx0)
        double tot = 0;
        u64    e   = 0;
        for (int i = 0; i < m; i++)
            for (int j = 0; j < m; j++) {
                tot += sc[8 * (ty0 + i) + tx0 + j];
                if (psy) e += e8[8 * (ty0 + i) + tx0 + j];
            }
        tot /= m * m;
        ssim_write(p, out0 + z, tot, (uint32_t)(n * n), sizeof(Pix) == 1 ? e >> 1 : e << 2);
    }
}

// one launch per batch, a wave per workgroup: the regions first (workgroups [0, n_pyramids)), the plain jobs behind them
template <typename Pix> __global__ void __launch_bounds__(64) ssim_kernel(const SsimParams p) {
    __shared__ double   sc[kMaxTiles];
    __shared__ uint32_t e8[64];
    if (blockIdx.x < p.d.n_pyramids) ssim_pyramid<Pix>(p, sc, e8, blockIdx.x, threadIdx.x);
    else ssim_job<Pix>(p, sc, blockIdx.x - p.d.n_pyramids, threadIdx.x);
}

const char *bad_job(const SvtHipBlockJob &jb, bool pyramid) {
    if (jb.subpel_x || jb.subpel_y) return "a sub-pixel view (subpel_x / subpel_y must be 0)";
    if (pyramid) return (jb.width == 64 && jb.height == 64) ? nullptr : "a pyramid region that is not 64x64";
    if (jb.width < 4 || jb.width > 128 || (jb.width & 3) || jb.height < 4 || jb.height > 128 || (jb.height & 3)) return "a size that is not a multiple of 4 in 4..128";
    return nullptr;
}

// the launch alone, under the caller's lock: ctx->async_mu for the batch entry (batch_host.h), leaf_mutex() for the pointer-level entries
void ssim_enqueue(SvtHipContext *ctx, const SvtHipSsimBatchDesc *d, int unclamped) {
    const SsimParams p = {*d, unclamped};
    const uint32_t   n = d->n_pyramids + d->n_jobs;
    if (d->bit_depth == 8) hipLaunchKernelGGL(ssim_kernel<uint8_t>, dim3(n), dim3(64), 0, ctx->stream, p);
    else hipLaunchKernelGGL(ssim_kernel<uint16_t>, dim3(n), dim3(64), 0, ctx->stream, p);
}

int ssim_batch_check(const SvtHipSsimBatchDesc *d) {
    if (d->bit_depth != 8 && d->bit_depth != 10) BAD("svt_hip_ssim_batch: bit_depth %u (8 or 10)", d->bit_depth);
    if (d->n_jobs == 0 && d->n_pyramids == 0) return SVT_HIP_OK; // behind bit_depth, ahead of the rest
    if (!d->src || !d->ref || (d->n_jobs && !d->jobs) || (d->n_pyramids && !d->pyramids))
        BAD("svt_hip_ssim_batch: a mandatory pointer (src, ref, jobs, pyramids) is null");
    if (!d->ssim && !d->ssim_dist) BAD("svt_hip_ssim_batch: no output (ssim, ssim_dist)");
    if (!d->src_stride || !d->ref_stride) BAD("svt_hip_ssim_batch: zero stride");
    if (!(d->psy_rd == d->psy_rd)) BAD("svt_hip_ssim_batch: psy_rd is NaN");
    if ((uint64_t)d->pyramid_out_base + (uint64_t)SVT_HIP_PYRAMID_BLOCKS * d->n_pyramids > 0xFFFFFFFFull) BAD("svt_hip_ssim_batch: pyramid output slots beyond 2^32");
    return SVT_HIP_OK;
}

} // namespace

extern "C" {

size_t svt_hip_ssim_desc_size(void) { return sizeof(SvtHipSsimBatchDesc); }

int svt_hip_ssim_check_jobs(const SvtHipBlockJob *jobs, uint32_t n_jobs, int pyramids) {
    if (!jobs && n_jobs) return svt_hip_fail(nullptr, SVT_HIP_ERR_BAD_PARAM, "svt_hip_ssim_check_jobs: jobs is null");
    for (uint32_t i = 0; i < n_jobs; i++)
        if (const char *why = bad_job(jobs[i], pyramids != 0))
            return svt_hip_fail(nullptr, SVT_HIP_ERR_BAD_PARAM, "SSIM %s %u: %s (%ux%u, subpel %u/%u)", pyramids ? "region" : "job", i, why, jobs[i].width,
                                jobs[i].height, jobs[i].subpel_x, jobs[i].subpel_y);
    return SVT_HIP_OK;
}

int svt_hip_ssim_batch(SvtHipContext *ctx, const SvtHipSsimBatchDesc *d) {
    return enqueue_batch("svt_hip_ssim_batch", ctx, d, ssim_batch_check, &SvtHipSsimBatchDesc::n_jobs, &SvtHipSsimBatchDesc::n_pyramids,
                         [=] { ssim_enqueue(ctx, d, 0); });
}

} // extern "C"

// ---- pointer-level entries (include/svt_hip_leaf.h): host pointers in, host result out, synchronous; fail closed (leaf_guard.h) ----------
namespace {

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct SsimLeafOut { double ssim; u64 dist; };

// one w x h block (samples of `bpp` bytes, strides in samples) through ssim_kernel.  The psy term reads whole 8x8 (4x4) tiles, which for a
// cropped size reach past the block as in the reference (psy_rd.c:141-160): those rows / columns are staged too.
SsimLeafOut leaf_ssim(const void *src, uint32_t sp, const void *ref, uint32_t rp, int w, int h, int bit_depth, double psy_rd, int unclamped) {
    if (w < 4 || w > 128 || (w & 3) || h < 4 || h > 128 || (h & 3)) leaf_fail("SSIM block %dx%d: sides must be multiples of 4 in 4..128", w, h);
    std::lock_guard<std::mutex> lock(leaf_mutex());
    SvtHipContext *ctx = leaf_ctx();
    const size_t bpp = bit_depth == 8 ? 1 : 2;
    const int    n   = (w >= 8 && h >= 8) ? 8 : 4;
    const int    sw  = psy_rd > 0.0 ? (w + n - 1) / n * n : w, sh = psy_rd > 0.0 ? (h + n - 1) / n * n : h;
    const size_t sb = align256(((size_t)sh - 1) * sp * bpp + (size_t)sw * bpp), rb = align256(((size_t)sh - 1) * rp * bpp + (size_t)sw * bpp);
    uint8_t *base = leaf_scratch(ctx, sb + rb + 512);
    uint8_t *d_src = base, *d_ref = base + sb, *d_job = d_ref + rb, *d_out = d_job + 256;
    leaf_check(ctx, hipMemcpyAsync(d_src, src, ((size_t)sh - 1) * sp * bpp + (size_t)sw * bpp, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(d_ref, ref, ((size_t)sh - 1) * rp * bpp + (size_t)sw * bpp, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    SvtHipBlockJob job;
    memset(&job, 0, sizeof(job));
    job.width = (uint8_t)w; job.height = (uint8_t)h;
    leaf_check(ctx, hipMemcpyAsync(d_job, &job, sizeof(job), hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    SsimLeafOut *o = reinterpret_cast<SsimLeafOut *>(d_out);
    SvtHipSsimBatchDesc d;
    memset(&d, 0, sizeof(d));
    d.bit_depth = (uint8_t)bit_depth; d.n_jobs = 1; d.src_stride = sp; d.ref_stride = rp; d.src = d_src; d.ref = d_ref;
    d.jobs = reinterpret_cast<const SvtHipBlockJob *>(d_job); d.psy_rd = psy_rd; d.ssim = &o->ssim; d.ssim_dist = reinterpret_cast<uint64_t *>(&o->dist);
    ssim_enqueue(ctx, &d, unclamped);
    leaf_check(ctx, hipGetLastError(), "the ssim_kernel launch");
    SsimLeafOut out;
    leaf_check(ctx, hipMemcpyAsync(&out, d_out, sizeof(out), hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return out;
}

} // namespace

extern "C" {

double svt_ssim_8x8_hip(const uint8_t *s, uint32_t sp, const uint8_t *r, uint32_t rp) LEAF_TRY
    return leaf_ssim(s, sp, r, rp, 8, 8, 8, 0.0, 1).ssim;
LEAF_CATCH(svt_ssim_8x8_hip, s, sp, r, rp)

double svt_ssim_4x4_hip(const uint8_t *s, uint32_t sp, const uint8_t *r, uint32_t rp) LEAF_TRY
    return leaf_ssim(s, sp, r, rp, 4, 4, 8, 0.0, 1).ssim;
LEAF_CATCH(svt_ssim_4x4_hip, s, sp, r, rp)

double svt_ssim_8x8_hbd_hip(const uint16_t *s, uint32_t sp, const uint16_t *r, uint32_t rp) LEAF_TRY
    return leaf_ssim(s, sp, r, rp, 8, 8, 10, 0.0, 1).ssim;
LEAF_CATCH(svt_ssim_8x8_hbd_hip, s, sp, r, rp)

double svt_ssim_4x4_hbd_hip(const uint16_t *s, uint32_t sp, const uint16_t *r, uint32_t rp) LEAF_TRY
    return leaf_ssim(s, sp, r, rp, 4, 4, 10, 0.0, 1).ssim;
LEAF_CATCH(svt_ssim_4x4_hbd_hip, s, sp, r, rp)

uint64_t svt_spatial_full_distortion_ssim_kernel_hip(uint8_t *input, uint32_t input_offset, uint32_t input_stride, uint8_t *recon, int32_t recon_offset,
                                                     uint32_t recon_stride, uint32_t area_width, uint32_t area_height, bool hbd, double psy_rd) LEAF_TRY
    if (hbd)
        return leaf_ssim(reinterpret_cast<uint16_t *>(input) + input_offset, input_stride, reinterpret_cast<uint16_t *>(recon) + recon_offset, recon_stride,
                         (int)area_width, (int)area_height, 10, psy_rd, 0).dist;
    return leaf_ssim(input + input_offset, input_stride, recon + recon_offset, recon_stride, (int)area_width, (int)area_height, 8, psy_rd, 0).dist;
LEAF_CATCH(svt_spatial_full_distortion_ssim_kernel_hip, input, input_offset, input_stride, recon, recon_offset, recon_stride, area_width, area_height, hbd, psy_rd)

} // extern "C"
