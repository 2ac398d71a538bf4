// leaf_kernels.hip -- the pointer-level `_hip` entries of include/svt_hip_leaf.h that wrap no batch kernel file of their own, with their
// single-workgroup kernels and staging helpers: the block statistics through block_stats_kernel (SAD, SSE, variance, psy distortion,
// hadamard_path), the exhaustive SAD search (svt_sad_loop_kernel), the stand-alone Hadamard transforms (their kernel: stats_kernel.hip) and SATD, cul_level, the 4x4 WHT,
// the coefficient-domain distortions, the residual, the 8x8-based SAD pyramid, the quantizers, and the forward / inverse transforms through
// the batches of rd_kernel.hip.
//
// Pointer-level entries: host pointers in, host results out, synchronous.  Each call stages the few rows it
// needs into the context's scratch buffer, launches, and copies the result back -- a validation / drop-in path,
// three PCIe round trips per call; production goes through the batched entries.  An entry that cannot run (no bound context, a
// device error) hands the call to the kernel the encoder had in the slot before the installer (leaf_guard.h): fail closed, never abort.
//
// Reference functions restated (Source/Lib):
//   svt_sad_loop_kernel_c                                           C_DEFAULT/compute_sad_c.c:58-101
//   svt_aom_hadamard_{4x4,8x8,16x16,32x32}_c, svt_aom_satd_c        C_DEFAULT/picture_operators_c.c:176-326, Codec/common_dsp_rtcd.c:70-77
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include "svt_hip_internal.h"
#include "leaf_guard.h"
#include "wave_ops.h"
#include "../../include/svt_hip_spy_rd.h"
#include "../../include/svt_hip_dsp.h"
#include "../../include/svt_hip_leaf.h"

namespace {

typedef unsigned long long u64;
typedef long long          i64;

// ---- svt_sad_loop_kernel: one thread per search position, first minimum in raster order through a 64-bit key ------
struct SadLoopParams {
    const uint8_t *src, *ref;
    uint32_t       src_stride, ref_stride, block_height, block_width, src_stride_raw;
    int            sa_w, sa_h, skip_even;
    u64           *best; // initialised to (0xffffff << 32) | 0xffffffff
};
__global__ void __launch_bounds__(256) sad_loop_kernel(const SadLoopParams p) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    u64       key = ~0ull;
    if (idx < p.sa_w * p.sa_h) {
        const int ys = idx / p.sa_w, xs = idx - ys * p.sa_w;
        if (!(p.skip_even && !(ys & 1))) {
            const uint8_t *r0 = p.ref + (size_t)ys * p.src_stride_raw + xs;
            uint32_t       s  = 0;
            for (uint32_t r = 0; r < p.block_height; r++)
                for (uint32_t c = 0; c < p.block_width; c++) {
                    const int d = (int)p.src[r * p.src_stride + c] - (int)r0[r * p.ref_stride + c];
                    s += (uint32_t)(d < 0 ? -d : d);
                }
            key = ((u64)s << 32) | ((u64)(uint32_t)ys << 16) | (uint32_t)xs;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u64 t = __shfl_xor(key, o, 64); key = t < key ? t : key; }
    if ((threadIdx.x & 63) == 0 && key != ~0ull) atomicMin(p.best, key);
}

__global__ void __launch_bounds__(64) satd_kernel(const int32_t *coeff, int n, int *out) {
    int acc = 0;
    for (int i = threadIdx.x; i < n; i += 64) { const int v = coeff[i]; acc += v < 0 ? -v : v; }
    acc = wave_sum(acc);
    if (threadIdx.x == 0) *out = acc;
}

// svt_av1_compute_cul_level (full_loop.c:1449-1466): min(63, sum over the first eob scan positions of |q|) + the DC sign bits.  A lane's terms
// are clamped to 63 each, which leaves the clamped total unchanged (and keeps the sum far from overflow, like the reference's early exit).
__global__ void __launch_bounds__(64) cul_level_kernel(const int16_t *scan, const int32_t *q, int eob, uint8_t *out) {
    uint32_t acc = 0;
    for (int c = threadIdx.x; c < eob; c += 64) { const int32_t v = q[scan[c]]; const uint32_t a = (uint32_t)(v < 0 ? -v : v); acc += a > 63u ? 63u : a; }
    acc = wave_sum(acc);
    if (threadIdx.x == 0) { const int32_t dc = q[0]; *out = (uint8_t)((acc > 63u ? 63u : acc) + (dc < 0 ? 64u : (dc > 0 ? 128u : 0u))); }
}

// svt_av1_fwht4x4 (transforms.c:3099-3151): 4-point reversible Walsh-Hadamard on columns, then on the rows of the intermediate; lane i < 4 owns
// column i in both passes (the second pass reads the transposed intermediate through LDS).  64-bit temporaries like the reference.
__device__ __forceinline__ void wht4(i64 a, i64 b, i64 c, i64 d, i64 o[4]) {
    a += b; d -= c;
    const i64 e = (a - d) >> 1;
    b = e - b; c = e - c; a -= c; d += b;
    o[0] = a; o[1] = c; o[2] = d; o[3] = b;
}
__global__ void __launch_bounds__(64) fwht4x4_kernel(const int16_t *in, uint32_t stride, int32_t *out) {
    __shared__ int32_t t[16];
    const int i = threadIdx.x;
    i64 o[4];
    if (i < 4) { wht4(in[i], in[stride + i], in[2 * stride + i], in[3 * stride + i], o); for (int k = 0; k < 4; k++) t[4 * i + k] = (int32_t)o[k]; }
    __syncthreads();
    if (i < 4) { wht4(t[i], t[4 + i], t[8 + i], t[12 + i], o); for (int k = 0; k < 4; k++) out[4 * k + i] = (int32_t)(o[k] * 4); }
}

// ---- coefficient-domain distortion (svt_full_distortion_kernel32_bits_c / _cbf_zero32_bits_c, pic_operators.c:150-222;
// svt_av1_block_error_c, common_dsp_rtcd.c:79-91): out[0] = sum (coeff - recon)^2 (recon == nullptr: 0), out[1] = sum coeff^2
// wrap32: svt_av1_block_error_c squares with SQR() on `int` operands -- a 32-bit wrapping product, widened afterwards
__global__ void __launch_bounds__(256) coeff_dist_kernel(const int32_t *coeff, uint32_t cstride, const int32_t *recon, uint32_t rstride, int w, int h, u64 *out,
                                                         int wrap32) {
    u64 d = 0, e = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < w * h; i += gridDim.x * 256) {
        const int r = i / w, c = i - r * w;
        const i64 a = coeff[(size_t)r * cstride + c];
        if (wrap32) {
            const uint32_t t = (uint32_t)a - (uint32_t)(recon ? recon[(size_t)r * rstride + c] : 0), ua = (uint32_t)a;
            d += (u64)(i64)(int32_t)(t * t);
            e += (u64)(i64)(int32_t)(ua * ua);
            continue;
        }
        if (recon) { const i64 t = a - recon[(size_t)r * rstride + c]; d += (u64)(t * t); }
        e += (u64)(a * a);
    }
    d = wave_sum(d); e = wave_sum(e);
    if ((threadIdx.x & 63) == 0) { atomicAdd(&out[0], d); atomicAdd(&out[1], e); }
}

// ---- residual (svt_residual_kernel8bit_c / 16bit_c, pic_operators.c:101-148): int16 arithmetic like the reference
template <typename Pix> __global__ void __launch_bounds__(256) residual_kernel(const Pix *in, uint32_t in_stride, const Pix *pred, uint32_t pred_stride, int16_t *res,
                                                                               uint32_t res_stride, int w, int h) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < w * h; i += gridDim.x * 256) {
        const int r = i / w, c = i - r * w;
        res[(size_t)r * res_stride + c] = (int16_t)((int16_t)in[(size_t)r * in_stride + c] - (int16_t)pred[(size_t)r * pred_stride + c]);
    }
}
size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// copies `rows` rows of `row_bytes` bytes (host stride `stride_bytes`) to the device, packed with the same stride
void upload_rows(SvtHipContext *ctx, void *dst, const void *src, size_t stride_bytes, size_t rows, size_t row_bytes) {
    if (rows == 0) return;
    leaf_check(ctx, hipMemcpyAsync(dst, src, (rows - 1) * stride_bytes + row_bytes, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
}

struct StatsOut { uint32_t sad, variance, var_sse, satd; u64 sse, psy_energy, psy_dist; uint32_t variance10, var_sse10; };

// one (src, ref) block through block_stats_kernel
StatsOut leaf_stats(const void *src, size_t src_stride, const void *ref, size_t ref_stride, int w, int h, int bit_depth, bool want_satd,
                    bool want_psy = false, double psy_rd = 0.0, int xo = 0, int yo = 0) {
    std::lock_guard<std::mutex> lock(leaf_mutex());
    SvtHipContext *ctx = leaf_ctx();
    const size_t bpp = bit_depth == 8 ? 1 : 2;
    const int sh = h + (yo ? 1 : 0), sw = w + (xo ? 1 : 0); // the interpolation reads one more row / column
    const size_t sb = align256(((size_t)sh - 1) * src_stride * bpp + (size_t)sw * bpp), rb = align256(((size_t)h - 1) * ref_stride * bpp + (size_t)w * bpp);
    uint8_t *base = leaf_scratch(ctx, sb + rb + 512);
    uint8_t *d_src = base, *d_ref = base + sb, *d_job = d_ref + rb, *d_out = d_job + 256;
    upload_rows(ctx, d_src, src, src_stride * bpp, sh, (size_t)sw * bpp);
    upload_rows(ctx, d_ref, ref, ref_stride * bpp, h, (size_t)w * bpp);
    SvtHipBlockJob job;
    memset(&job, 0, sizeof(job));
    job.width = (uint8_t)w; job.height = (uint8_t)h; job.subpel_x = (uint8_t)xo; job.subpel_y = (uint8_t)yo;
    leaf_check(ctx, hipMemcpyAsync(d_job, &job, sizeof(job), hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    SvtHipBlockStatsDesc d;
    memset(&d, 0, sizeof(d));
    d.bit_depth = (uint8_t)bit_depth; d.n_jobs = 1; d.src_stride = (uint32_t)src_stride; d.ref_stride = (uint32_t)ref_stride;
    d.src = d_src; d.ref = d_ref; d.jobs = reinterpret_cast<const SvtHipBlockJob *>(d_job);
    StatsOut *o = reinterpret_cast<StatsOut *>(d_out);
    d.sad = &o->sad; d.variance = &o->variance; d.var_sse = &o->var_sse; d.sse = reinterpret_cast<uint64_t *>(&o->sse); d.satd = want_satd ? &o->satd : nullptr;
    if (bit_depth == 10) { d.variance10 = &o->variance10; d.var_sse10 = &o->var_sse10; }
    if (want_psy) { d.psy_rd = psy_rd; d.psy_energy = reinterpret_cast<uint64_t *>(&o->psy_energy); d.psy_dist = reinterpret_cast<uint64_t *>(&o->psy_dist); }
    if (svt_hip_block_stats_batch(ctx, &d) != SVT_HIP_OK) leaf_fail("%s", svt_hip_err_buf());
    StatsOut out;
    memset(&out, 0, sizeof(out));
    leaf_check(ctx, hipMemcpyAsync(&out, d_out, sizeof(out), hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return out;
}

} // namespace

extern "C" {

void svt_sad_loop_kernel_hip(uint8_t *src, uint32_t src_stride, uint8_t *ref, uint32_t ref_stride, uint32_t block_height,
                             uint32_t block_width, uint64_t *best_sad, int16_t *x_search_center, int16_t *y_search_center,
                             uint32_t src_stride_raw, uint8_t skip_search_line, int16_t search_area_width, int16_t search_area_height) LEAF_TRY
    std::lock_guard<std::mutex> lock(leaf_mutex());
    SvtHipContext *ctx = leaf_ctx();
    *best_sad = 0xffffff;
    if (search_area_width <= 0 || search_area_height <= 0 || block_height == 0 || block_width == 0) return;
    const size_t sb = align256(((size_t)block_height - 1) * src_stride + block_width);
    const size_t ref_rows_bytes = ((size_t)search_area_height - 1) * src_stride_raw + ((size_t)block_height - 1) * ref_stride + block_width + search_area_width - 1;
    const size_t rb = align256(ref_rows_bytes);
    uint8_t *base = leaf_scratch(ctx, sb + rb + 256);
    uint8_t *d_src = base, *d_ref = base + sb;
    u64     *d_best = reinterpret_cast<u64 *>(d_ref + rb);
    leaf_check(ctx, hipMemcpyAsync(d_src, src, ((size_t)block_height - 1) * src_stride + block_width, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(d_ref, ref, ref_rows_bytes, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    const u64 init = (0xffffffull << 32) | 0xffffffffull;
    leaf_check(ctx, hipMemcpyAsync(d_best, &init, sizeof(init), hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    SadLoopParams p;
    p.src = d_src; p.ref = d_ref; p.src_stride = src_stride; p.ref_stride = ref_stride; p.block_height = block_height; p.block_width = block_width;
    p.src_stride_raw = src_stride_raw; p.sa_w = search_area_width; p.sa_h = search_area_height;
    p.skip_even = (block_width == 16 && block_height <= 16 && skip_search_line) ? 1 : 0;
    p.best = d_best;
    const int npos = (int)search_area_width * (int)search_area_height;
    hipLaunchKernelGGL(sad_loop_kernel, dim3((npos + 255) / 256), dim3(256), 0, ctx->stream, p);
    leaf_check(ctx, hipGetLastError(), "sad_loop_kernel launch");
    u64 best = 0;
    leaf_check(ctx, hipMemcpyAsync(&best, d_best, sizeof(best), hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    if ((uint32_t)(best >> 32) < 0xffffff) { // strict `<` against the initial value, like the reference
        *best_sad        = best >> 32;
        *x_search_center = (int16_t)(best & 0xFFFF);
        *y_search_center = (int16_t)((best >> 16) & 0xFFFF);
    }
LEAF_CATCH(svt_sad_loop_kernel_hip, src, src_stride, ref, ref_stride, block_height, block_width, best_sad, x_search_center, y_search_center, src_stride_raw, skip_search_line, search_area_width, search_area_height)

uint32_t svt_nxm_sad_kernel_helper_hip(const uint8_t *src, uint32_t src_stride, const uint8_t *ref, uint32_t ref_stride, uint32_t height, uint32_t width) LEAF_TRY
    return leaf_stats(src, src_stride, ref, ref_stride, (int)width, (int)height, 8, false).sad;
LEAF_CATCH(svt_nxm_sad_kernel_helper_hip, src, src_stride, ref, ref_stride, height, width)

uint32_t svt_aom_sad_16b_kernel_hip(uint16_t *src, uint32_t src_stride, uint16_t *ref, uint32_t ref_stride, uint32_t height, uint32_t width) LEAF_TRY
    return leaf_stats(src, src_stride, ref, ref_stride, (int)width, (int)height, 10, false).sad;
LEAF_CATCH(svt_aom_sad_16b_kernel_hip, src, src_stride, ref, ref_stride, height, width)

unsigned int svt_aom_variance_hip(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, int width, int height, unsigned int *sse) LEAF_TRY
    const StatsOut o = leaf_stats(src, (size_t)src_stride, ref, (size_t)ref_stride, width, height, 8, false);
    *sse = o.var_sse;
    return o.variance;
LEAF_CATCH(svt_aom_variance_hip, src, src_stride, ref, ref_stride, width, height, sse)

unsigned int svt_aom_sub_pixel_variance_hip(const uint8_t *src, int src_stride, int xoffset, int yoffset, const uint8_t *ref, int ref_stride, int width,
                                            int height, unsigned int *sse) LEAF_TRY
    const StatsOut o = leaf_stats(src, (size_t)src_stride, ref, (size_t)ref_stride, width, height, 8, false, false, 0.0, xoffset & 7, yoffset & 7);
    *sse = o.var_sse;
    return o.variance;
LEAF_CATCH(svt_aom_sub_pixel_variance_hip, src, src_stride, xoffset, yoffset, ref, ref_stride, width, height, sse)

#define SVT_HIP_VAR(W, H)                                                                                                             \
    unsigned int svt_aom_variance##W##x##H##_hip(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse) LEAF_TRY \
        return svt_aom_variance_hip(src, src_stride, ref, ref_stride, W, H, sse);                                                       \
    LEAF_CATCH(svt_aom_variance##W##x##H##_hip, src, src_stride, ref, ref_stride, sse)                                                  \
    unsigned int svt_aom_sub_pixel_variance##W##x##H##_hip(const uint8_t *src, int src_stride, int xoffset, int yoffset, const uint8_t *ref, \
                                                           int ref_stride, unsigned int *sse) LEAF_TRY                               \
        return svt_aom_sub_pixel_variance_hip(src, src_stride, xoffset, yoffset, ref, ref_stride, W, H, sse);                           \
    LEAF_CATCH(svt_aom_sub_pixel_variance##W##x##H##_hip, src, src_stride, xoffset, yoffset, ref, ref_stride, sse)
SVT_HIP_VAR(4, 4) SVT_HIP_VAR(4, 8) SVT_HIP_VAR(4, 16) SVT_HIP_VAR(8, 4) SVT_HIP_VAR(8, 8) SVT_HIP_VAR(8, 16) SVT_HIP_VAR(8, 32)
SVT_HIP_VAR(16, 4) SVT_HIP_VAR(16, 8) SVT_HIP_VAR(16, 16) SVT_HIP_VAR(16, 32) SVT_HIP_VAR(16, 64) SVT_HIP_VAR(32, 8) SVT_HIP_VAR(32, 16)
SVT_HIP_VAR(32, 32) SVT_HIP_VAR(32, 64) SVT_HIP_VAR(64, 16) SVT_HIP_VAR(64, 32) SVT_HIP_VAR(64, 64) SVT_HIP_VAR(64, 128) SVT_HIP_VAR(128, 64)
SVT_HIP_VAR(128, 128)
#undef SVT_HIP_VAR

int64_t svt_aom_sse_hip(const uint8_t *a, int a_stride, const uint8_t *b, int b_stride, int width, int height) LEAF_TRY
    return (int64_t)leaf_stats(a, (size_t)a_stride, b, (size_t)b_stride, width, height, 8, false).sse;
LEAF_CATCH(svt_aom_sse_hip, a, a_stride, b, b_stride, width, height)

// svt_aom_highbd_sse (aom_dsp_rtcd.h:56; enc_inter_prediction.c:559-570): the uint8_t pointers ARE the uint16_t pointers (plain cast there)
int64_t svt_aom_highbd_sse_hip(const uint8_t *a8, int a_stride, const uint8_t *b8, int b_stride, int width, int height) LEAF_TRY
    return (int64_t)leaf_stats(reinterpret_cast<const uint16_t *>(a8), (size_t)a_stride, reinterpret_cast<const uint16_t *>(b8), (size_t)b_stride, width, height, 10,
                               false).sse;
LEAF_CATCH(svt_aom_highbd_sse_hip, a8, a_stride, b8, b_stride, width, height)

uint64_t svt_spatial_full_distortion_kernel_hip(uint8_t *input, uint32_t input_offset, uint32_t input_stride, uint8_t *recon, int32_t recon_offset,
                                                uint32_t recon_stride, uint32_t area_width, uint32_t area_height) LEAF_TRY
    return leaf_stats(input + input_offset, input_stride, recon + recon_offset, recon_stride, (int)area_width, (int)area_height, 8, false).sse;
LEAF_CATCH(svt_spatial_full_distortion_kernel_hip, input, input_offset, input_stride, recon, recon_offset, recon_stride, area_width, area_height)

uint64_t svt_full_distortion_kernel16_bits_hip(uint8_t *input, uint32_t input_offset, uint32_t input_stride, uint8_t *recon, int32_t recon_offset,
                                               uint32_t recon_stride, uint32_t area_width, uint32_t area_height) LEAF_TRY
    return leaf_stats(reinterpret_cast<uint16_t *>(input) + input_offset, input_stride, reinterpret_cast<uint16_t *>(recon) + recon_offset, recon_stride,
                      (int)area_width, (int)area_height, 10, false).sse;
LEAF_CATCH(svt_full_distortion_kernel16_bits_hip, input, input_offset, input_stride, recon, recon_offset, recon_stride, area_width, area_height)

uint64_t svt_hip_spy_rd_bias(uint64_t sse, uint32_t area_width, uint32_t area_height, uint8_t mode, uint8_t compound_type, uint8_t temporal_layer_index,
                             double psy_rd, uint8_t spy_rd) {
    return (uint64_t)svt_hip_spy_rd_bias_inline((int64_t)sse, area_width, area_height, mode, compound_type, temporal_layer_index, psy_rd, spy_rd);
}

uint64_t svt_spatial_full_distortion_kernel_facade_hip(uint8_t *input, uint32_t input_offset, uint32_t input_stride, uint8_t *recon, int32_t recon_offset,
                                                       uint32_t recon_stride, uint32_t area_width, uint32_t area_height, bool hbd_md, uint8_t mode,
                                                       uint8_t compound_type, uint8_t temporal_layer_index, double psy_rd, uint8_t spy_rd) LEAF_TRY
    const uint64_t sse = hbd_md ? svt_full_distortion_kernel16_bits_hip(input, input_offset, input_stride, recon, recon_offset, recon_stride, area_width, area_height)
                                : svt_spatial_full_distortion_kernel_hip(input, input_offset, input_stride, recon, recon_offset, recon_stride, area_width, area_height);
    return svt_hip_spy_rd_bias(sse, area_width, area_height, mode, compound_type, temporal_layer_index, psy_rd, spy_rd);
LEAF_CATCH(svt_spatial_full_distortion_kernel_facade_hip, input, input_offset, input_stride, recon, recon_offset, recon_stride, area_width, area_height, hbd_md, mode, compound_type, temporal_layer_index, psy_rd, spy_rd)

uint64_t svt_spatial_psy_distortion_kernel_hip(uint8_t *input, uint32_t input_offset, uint32_t input_stride, uint8_t *recon, int32_t recon_offset,
                                               uint32_t recon_stride, uint32_t area_width, uint32_t area_height, double psy_rd) LEAF_TRY
    const StatsOut o = leaf_stats(input + input_offset, input_stride, recon + recon_offset, recon_stride, (int)area_width, (int)area_height, 8, false,
                                  psy_rd > 0.0, psy_rd);
    return o.sse + (psy_rd > 0.0 ? o.psy_dist : 0);
LEAF_CATCH(svt_spatial_psy_distortion_kernel_hip, input, input_offset, input_stride, recon, recon_offset, recon_stride, area_width, area_height, psy_rd)

uint64_t svt_psy_distortion_hip(const uint8_t *input, uint32_t input_stride, const uint8_t *recon, uint32_t recon_stride, uint32_t width, uint32_t height) LEAF_TRY
    return leaf_stats(input, input_stride, recon, recon_stride, (int)width, (int)height, 8, false, true, 0.0).psy_energy;
LEAF_CATCH(svt_psy_distortion_hip, input, input_stride, recon, recon_stride, width, height)
uint64_t svt_psy_distortion_hbd_hip(const uint16_t *input, uint32_t input_stride, const uint16_t *recon, uint32_t recon_stride, uint32_t width, uint32_t height) LEAF_TRY
    return leaf_stats(input, input_stride, recon, recon_stride, (int)width, (int)height, 10, false, true, 0.0).psy_energy;
LEAF_CATCH(svt_psy_distortion_hbd_hip, input, input_stride, recon, recon_stride, width, height)
uint64_t get_svt_psy_full_dist_hip(const void *s, uint32_t so, uint32_t sp, const void *r, uint32_t ro, uint32_t rp, uint32_t w, uint32_t h, uint8_t is_hbd,
                                   double psy_rd) LEAF_TRY
    if (is_hbd == 1)
        return leaf_stats(static_cast<const uint16_t *>(s) + so, sp, static_cast<const uint16_t *>(r) + ro, rp, (int)w, (int)h, 10, false, true, psy_rd).psy_dist;
    return leaf_stats(static_cast<const uint8_t *>(s) + so, sp, static_cast<const uint8_t *>(r) + ro, rp, (int)w, (int)h, 8, false, true, psy_rd).psy_dist;
LEAF_CATCH(get_svt_psy_full_dist_hip, s, so, sp, r, ro, rp, w, h, is_hbd, psy_rd)

uint32_t svt_hip_hadamard_path(const uint8_t *input, uint32_t input_stride, const uint8_t *pred, uint32_t pred_stride, uint32_t block_size_wide) LEAF_TRY
    return leaf_stats(input, input_stride, pred, pred_stride, (int)block_size_wide, (int)block_size_wide, 8, true).satd;
LEAF_CATCH(svt_hip_hadamard_path, input, input_stride, pred, pred_stride, block_size_wide)

static void leaf_hadamard(const int16_t *src_diff, ptrdiff_t src_stride, int32_t *coeff, int n) {
    std::lock_guard<std::mutex> lock(leaf_mutex());
    SvtHipContext *ctx = leaf_ctx();
    const size_t sb = align256((((size_t)n - 1) * (size_t)src_stride + n) * 2);
    uint8_t *base = leaf_scratch(ctx, sb + (size_t)n * n * 4);
    leaf_check(ctx, hipMemcpyAsync(base, src_diff, (((size_t)n - 1) * (size_t)src_stride + n) * 2, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, svt_hip_hadamard_launch(ctx, reinterpret_cast<const int16_t *>(base), (int)src_stride, n, reinterpret_cast<int32_t *>(base + sb)), "hadamard_kernel launch");
    leaf_check(ctx, hipMemcpyAsync(coeff, base + sb, (size_t)n * n * 4, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
}
void svt_aom_hadamard_4x4_hip(const int16_t *src_diff, ptrdiff_t src_stride, int32_t *coeff) LEAF_TRY leaf_hadamard(src_diff, src_stride, coeff, 4); LEAF_CATCH(svt_aom_hadamard_4x4_hip, src_diff, src_stride, coeff)
void svt_aom_hadamard_8x8_hip(const int16_t *src_diff, ptrdiff_t src_stride, int32_t *coeff) LEAF_TRY leaf_hadamard(src_diff, src_stride, coeff, 8); LEAF_CATCH(svt_aom_hadamard_8x8_hip, src_diff, src_stride, coeff)
void svt_aom_hadamard_16x16_hip(const int16_t *src_diff, ptrdiff_t src_stride, int32_t *coeff) LEAF_TRY leaf_hadamard(src_diff, src_stride, coeff, 16); LEAF_CATCH(svt_aom_hadamard_16x16_hip, src_diff, src_stride, coeff)
void svt_aom_hadamard_32x32_hip(const int16_t *src_diff, ptrdiff_t src_stride, int32_t *coeff) LEAF_TRY leaf_hadamard(src_diff, src_stride, coeff, 32); LEAF_CATCH(svt_aom_hadamard_32x32_hip, src_diff, src_stride, coeff)

int svt_aom_satd_hip(const int32_t *coeff, int length) LEAF_TRY
    std::lock_guard<std::mutex> lock(leaf_mutex());
    SvtHipContext *ctx = leaf_ctx();
    if (length <= 0) return 0;
    const size_t cb = align256((size_t)length * 4);
    uint8_t *base = leaf_scratch(ctx, cb + 256);
    leaf_check(ctx, hipMemcpyAsync(base, coeff, (size_t)length * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    hipLaunchKernelGGL(satd_kernel, dim3(1), dim3(64), 0, ctx->stream, reinterpret_cast<const int32_t *>(base), length, reinterpret_cast<int *>(base + cb));
    leaf_check(ctx, hipGetLastError(), "satd_kernel launch");
    int out = 0;
    leaf_check(ctx, hipMemcpyAsync(&out, base + cb, sizeof(out), hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return out;
LEAF_CATCH(svt_aom_satd_hip, coeff, length)

// svt_av1_compute_cul_level (aom_dsp_rtcd.h:904): the prototype carries no array length; scan[0 .. eob) and the coefficients those
// positions (and position 0) name are what the reference reads, so that is what travels
uint8_t svt_av1_compute_cul_level_hip(const int16_t *const scan, const int32_t *const quant_coeff, uint16_t *eob) LEAF_TRY
    std::lock_guard<std::mutex> lock(leaf_mutex());
    SvtHipContext *ctx = leaf_ctx();
    const int n = *eob;
    int       top = 0;
    for (int c = 0; c < n; c++) top = scan[c] > top ? scan[c] : top;
    const size_t sb = align256((size_t)(n ? n : 1) * 2), qb = align256((size_t)(top + 1) * 4);
    uint8_t *base = leaf_scratch(ctx, sb + qb + 256);
    if (n) leaf_check(ctx, hipMemcpyAsync(base, scan, (size_t)n * 2, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(base + sb, quant_coeff, (size_t)(top + 1) * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    hipLaunchKernelGGL(cul_level_kernel, dim3(1), dim3(64), 0, ctx->stream, reinterpret_cast<const int16_t *>(base), reinterpret_cast<const int32_t *>(base + sb), n, base + sb + qb);
    leaf_check(ctx, hipGetLastError(), "cul_level_kernel launch");
    uint8_t out = 0;
    leaf_check(ctx, hipMemcpyAsync(&out, base + sb + qb, 1, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return out;
LEAF_CATCH(svt_av1_compute_cul_level_hip, scan, quant_coeff, eob)

// svt_av1_fwht4x4 (aom_dsp_rtcd.h:208)
void svt_av1_fwht4x4_hip(int16_t *input, int32_t *output, uint32_t stride) LEAF_TRY
    std::lock_guard<std::mutex> lock(leaf_mutex());
    SvtHipContext *ctx = leaf_ctx();
    const size_t ib = align256((3 * (size_t)stride + 4) * 2);
    uint8_t *base = leaf_scratch(ctx, ib + 256);
    leaf_check(ctx, hipMemcpyAsync(base, input, (3 * (size_t)stride + 4) * 2, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    hipLaunchKernelGGL(fwht4x4_kernel, dim3(1), dim3(64), 0, ctx->stream, reinterpret_cast<const int16_t *>(base), stride, reinterpret_cast<int32_t *>(base + ib));
    leaf_check(ctx, hipGetLastError(), "fwht4x4_kernel launch");
    leaf_check(ctx, hipMemcpyAsync(output, base + ib, 16 * 4, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
LEAF_CATCH(svt_av1_fwht4x4_hip, input, output, stride)

// get_hvs_modulation_factor (psy_rd.c:295-307): host arithmetic
double svt_hip_hvs_modulation_factor(double psy_rd, int is_islice, uint8_t temporal_layer_index) {
    if (is_islice) return psy_rd * 0.4;
    if (temporal_layer_index == 0) return psy_rd * 0.75;
    if (temporal_layer_index == 1) return psy_rd * 0.9;
    if (temporal_layer_index == 2) return psy_rd * 0.95;
    return psy_rd;
}


// svt_aom_sad{W}x{H} and the four-reference form (aom_dsp_rtcd.h:267-347; macros at C_DEFAULT/compute_sad_c.c:117-207)
#define SVT_HIP_SAD(W, H)                                                                                                              \
    uint32_t svt_aom_sad##W##x##H##_hip(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride) LEAF_TRY              \
        return leaf_stats(src, (size_t)src_stride, ref, (size_t)ref_stride, W, H, 8, false).sad;                                        \
    LEAF_CATCH(svt_aom_sad##W##x##H##_hip, src, src_stride, ref, ref_stride)                                                           \
    void svt_aom_sad##W##x##H##x4d_hip(const uint8_t *src, int src_stride, const uint8_t *const ref[], int ref_stride, uint32_t *sad_array) LEAF_TRY \
        for (int i = 0; i < 4; i++) sad_array[i] = leaf_stats(src, (size_t)src_stride, ref[i], (size_t)ref_stride, W, H, 8, false).sad; \
    LEAF_CATCH(svt_aom_sad##W##x##H##x4d_hip, src, src_stride, ref, ref_stride, sad_array)
SVT_HIP_SAD(4, 4) SVT_HIP_SAD(4, 8) SVT_HIP_SAD(4, 16) SVT_HIP_SAD(8, 4) SVT_HIP_SAD(8, 8) SVT_HIP_SAD(8, 16) SVT_HIP_SAD(8, 32)
SVT_HIP_SAD(16, 4) SVT_HIP_SAD(16, 8) SVT_HIP_SAD(16, 16) SVT_HIP_SAD(16, 32) SVT_HIP_SAD(16, 64) SVT_HIP_SAD(32, 8) SVT_HIP_SAD(32, 16)
SVT_HIP_SAD(32, 32) SVT_HIP_SAD(32, 64) SVT_HIP_SAD(64, 16) SVT_HIP_SAD(64, 32) SVT_HIP_SAD(64, 64) SVT_HIP_SAD(64, 128) SVT_HIP_SAD(128, 64)
SVT_HIP_SAD(128, 128)
#undef SVT_HIP_SAD

// svt_aom_highbd_10_variance{W}x{H} (aom_dsp_rtcd.h:546-568): the uint8_t pointers carry uint16_t addresses >> 1 (CONVERT_TO_SHORTPTR)
#define SVT_HIP_VAR10(W, H)                                                                                                           \
    unsigned int svt_aom_highbd_10_variance##W##x##H##_hip(const uint8_t *src8, int src_stride, const uint8_t *ref8, int ref_stride, unsigned int *sse) LEAF_TRY \
        const StatsOut o = leaf_stats(reinterpret_cast<const uint16_t *>(reinterpret_cast<uintptr_t>(src8) << 1), (size_t)src_stride,  \
                                      reinterpret_cast<const uint16_t *>(reinterpret_cast<uintptr_t>(ref8) << 1), (size_t)ref_stride, W, H, 10, false); \
        *sse = o.var_sse10;                                                                                                            \
        return o.variance10;                                                                                                           \
    LEAF_CATCH(svt_aom_highbd_10_variance##W##x##H##_hip, src8, src_stride, ref8, ref_stride, sse)
SVT_HIP_VAR10(4, 4) SVT_HIP_VAR10(4, 8) SVT_HIP_VAR10(4, 16) SVT_HIP_VAR10(8, 4) SVT_HIP_VAR10(8, 8) SVT_HIP_VAR10(8, 16) SVT_HIP_VAR10(8, 32)
SVT_HIP_VAR10(16, 4) SVT_HIP_VAR10(16, 8) SVT_HIP_VAR10(16, 16) SVT_HIP_VAR10(16, 32) SVT_HIP_VAR10(16, 64) SVT_HIP_VAR10(32, 8) SVT_HIP_VAR10(32, 16)
SVT_HIP_VAR10(32, 32) SVT_HIP_VAR10(32, 64) SVT_HIP_VAR10(64, 16) SVT_HIP_VAR10(64, 32) SVT_HIP_VAR10(64, 64) SVT_HIP_VAR10(64, 128) SVT_HIP_VAR10(128, 64)
SVT_HIP_VAR10(128, 128)
#undef SVT_HIP_VAR10

uint32_t svt_aom_variance_highbd_hip(const uint16_t *a, int a_stride, const uint16_t *b, int b_stride, int w, int h, uint32_t *sse) LEAF_TRY
    const StatsOut o = leaf_stats(a, (size_t)a_stride, b, (size_t)b_stride, w, h, 10, false);
    *sse = o.var_sse;
    return o.variance;
LEAF_CATCH(svt_aom_variance_highbd_hip, a, a_stride, b, b_stride, w, h, sse)

static void leaf_coeff_dist(const int32_t *coeff, uint32_t cstride, const int32_t *recon, uint32_t rstride, uint32_t w, uint32_t h, uint64_t out[2], int wrap32 = 0) {
    std::lock_guard<std::mutex> lock(leaf_mutex());
    SvtHipContext *ctx = leaf_ctx();
    out[0] = out[1] = 0;
    if (!w || !h) return;
    const size_t cb = align256((((size_t)h - 1) * cstride + w) * 4), rb = recon ? align256((((size_t)h - 1) * rstride + w) * 4) : 0;
    uint8_t *base = leaf_scratch(ctx, cb + rb + 256);
    leaf_check(ctx, hipMemcpyAsync(base, coeff, (((size_t)h - 1) * cstride + w) * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    if (recon) leaf_check(ctx, hipMemcpyAsync(base + cb, recon, (((size_t)h - 1) * rstride + w) * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    u64 *d_out = reinterpret_cast<u64 *>(base + cb + rb);
    leaf_check(ctx, hipMemsetAsync(d_out, 0, 16, ctx->stream), "hipMemsetAsync");
    const int n = (int)(w * h), grid = n < 256 * 64 ? (n + 255) / 256 : 64;
    hipLaunchKernelGGL(coeff_dist_kernel, dim3(grid), dim3(256), 0, ctx->stream, reinterpret_cast<const int32_t *>(base), cstride,
                       recon ? reinterpret_cast<const int32_t *>(base + cb) : nullptr, rstride, (int)w, (int)h, d_out, wrap32);
    leaf_check(ctx, hipGetLastError(), "coeff_dist_kernel launch");
    leaf_check(ctx, hipMemcpyAsync(out, d_out, 16, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
}
void svt_full_distortion_kernel32_bits_hip(int32_t *coeff, uint32_t coeff_stride, int32_t *recon_coeff, uint32_t recon_coeff_stride, uint64_t distortion_result[2],
                                           uint32_t area_width, uint32_t area_height) LEAF_TRY
    leaf_coeff_dist(coeff, coeff_stride, recon_coeff, recon_coeff_stride, area_width, area_height, distortion_result);
LEAF_CATCH(svt_full_distortion_kernel32_bits_hip, coeff, coeff_stride, recon_coeff, recon_coeff_stride, distortion_result, area_width, area_height)
void svt_full_distortion_kernel_cbf_zero32_bits_hip(int32_t *coeff, uint32_t coeff_stride, uint64_t distortion_result[2], uint32_t area_width, uint32_t area_height) LEAF_TRY
    uint64_t o[2];
    leaf_coeff_dist(coeff, coeff_stride, nullptr, 0, area_width, area_height, o);
    distortion_result[0] = o[1]; // DIST_CALC_RESIDUAL = DIST_CALC_PREDICTION = sum coeff^2 (pic_operators.c:202-222)
    distortion_result[1] = o[1];
LEAF_CATCH(svt_full_distortion_kernel_cbf_zero32_bits_hip, coeff, coeff_stride, distortion_result, area_width, area_height)
int64_t svt_av1_block_error_hip(const int32_t *coeff, const int32_t *dqcoeff, intptr_t block_size, int64_t *ssz) LEAF_TRY
    uint64_t o[2];
    leaf_coeff_dist(coeff, (uint32_t)block_size, dqcoeff, (uint32_t)block_size, (uint32_t)block_size, 1, o, 1);
    *ssz = (int64_t)o[1];
    return (int64_t)o[0];
LEAF_CATCH(svt_av1_block_error_hip, coeff, dqcoeff, block_size, ssz)

} // extern "C"
template <typename Pix> static void leaf_residual(const Pix *in, uint32_t in_stride, const Pix *pred, uint32_t pred_stride, int16_t *res, uint32_t res_stride, uint32_t w, uint32_t h) {
    std::lock_guard<std::mutex> lock(leaf_mutex());
    SvtHipContext *ctx = leaf_ctx();
    if (!w || !h) return;
    const size_t ib = align256((((size_t)h - 1) * in_stride + w) * sizeof(Pix)), pb = align256((((size_t)h - 1) * pred_stride + w) * sizeof(Pix));
    const size_t rbytes = (((size_t)h - 1) * res_stride + w) * 2;
    uint8_t *base = leaf_scratch(ctx, ib + pb + align256(rbytes));
    leaf_check(ctx, hipMemcpyAsync(base, in, (((size_t)h - 1) * in_stride + w) * sizeof(Pix), hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(base + ib, pred, (((size_t)h - 1) * pred_stride + w) * sizeof(Pix), hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    // the rows between the block's columns belong to the caller: bring them over so that the copy back leaves them unchanged
    leaf_check(ctx, hipMemcpyAsync(base + ib + pb, res, rbytes, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    const int n = (int)(w * h), grid = n < 256 * 64 ? (n + 255) / 256 : 64;
    hipLaunchKernelGGL(residual_kernel<Pix>, dim3(grid), dim3(256), 0, ctx->stream, reinterpret_cast<const Pix *>(base), in_stride, reinterpret_cast<const Pix *>(base + ib),
                       pred_stride, reinterpret_cast<int16_t *>(base + ib + pb), res_stride, (int)w, (int)h);
    leaf_check(ctx, hipGetLastError(), "residual_kernel launch");
    leaf_check(ctx, hipMemcpyAsync(res, base + ib + pb, rbytes, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
}
extern "C" {
void svt_residual_kernel8bit_hip(uint8_t *input, uint32_t input_stride, uint8_t *pred, uint32_t pred_stride, int16_t *residual, uint32_t residual_stride,
                                 uint32_t area_width, uint32_t area_height) LEAF_TRY
    leaf_residual<uint8_t>(input, input_stride, pred, pred_stride, residual, residual_stride, area_width, area_height);
LEAF_CATCH(svt_residual_kernel8bit_hip, input, input_stride, pred, pred_stride, residual, residual_stride, area_width, area_height)
void svt_residual_kernel16bit_hip(uint16_t *input, uint32_t input_stride, uint16_t *pred, uint32_t pred_stride, int16_t *residual, uint32_t residual_stride,
                                  uint32_t area_width, uint32_t area_height) LEAF_TRY
    leaf_residual<uint16_t>(input, input_stride, pred, pred_stride, residual, residual_stride, area_width, area_height);
LEAF_CATCH(svt_residual_kernel16bit_hip, input, input_stride, pred, pred_stride, residual, residual_stride, area_width, area_height)

// svt_aom_estimate_transform (Codec/transforms.c:3158-3225) without the pcs / ctx arguments (they only select the lossless WHT):
// int16 residual -> packed coefficients (min(W,32) x min(H,32)) + the energy of the discarded frequencies, through the fused
// RD kernel (a uint16 plane holding the residual's bit pattern against an all-zero prediction reproduces the residual exactly)
int svt_hip_estimate_transform(int16_t *residual, uint32_t residual_stride, int32_t *coeff, int tx_size, uint64_t *three_quad_energy, int tx_type, int pf_shape) {
    if (tx_size < 0 || tx_size >= SVT_HIP_TX_SIZES_ALL || tx_type < 0 || tx_type >= SVT_HIP_TX_TYPES || pf_shape < 0 || pf_shape > 3 || !residual || !coeff) return SVT_HIP_ERR_BAD_PARAM;
    try {
    std::lock_guard<std::mutex> lock(leaf_mutex());
    SvtHipContext *ctx = leaf_ctx();
    const int W = svt_hip_tx_size_wide(tx_size), H = svt_hip_tx_size_high(tx_size), NP = (W > 32 ? 32 : W) * (H > 32 ? 32 : H);
    const size_t sb = align256((((size_t)H - 1) * residual_stride + W) * 2), zb = align256((size_t)W * H * 2);
    uint8_t *base = leaf_scratch(ctx, sb + zb + 256 + 256 + 256 + align256((size_t)NP * 4));
    uint8_t *d_src = base, *d_zero = d_src + sb, *d_job = d_zero + zb, *d_row = d_job + 256, *d_out = d_row + 256, *d_coeff = d_out + 256;
    leaf_check(ctx, hipMemcpyAsync(d_src, residual, (((size_t)H - 1) * residual_stride + W) * 2, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemsetAsync(d_zero, 0, zb, ctx->stream), "hipMemsetAsync");
    SvtHipTxJob job;
    memset(&job, 0, sizeof(job));
    job.tx_type = (uint8_t)tx_type; job.pf_shape = (uint8_t)pf_shape;
    SvtHipQuantRow row;
    memset(&row, 0, sizeof(row));
    for (int k = 0; k < 2; k++) { row.zbin[k] = 32767; row.quant[k] = 1; row.quant_shift[k] = 1; row.dequant[k] = 1; } // quantizer output unused
    leaf_check(ctx, hipMemcpyAsync(d_job, &job, sizeof(job), hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(d_row, &row, sizeof(row), hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    SvtHipRdBatchDesc d;
    memset(&d, 0, sizeof(d));
    d.bit_depth = 10; d.quant_kind = 0; d.tx_size = (uint8_t)tx_size; d.n_jobs = 1; d.src_stride = residual_stride; d.pred_stride = (uint32_t)W;
    d.src = d_src; d.pred = d_zero; d.jobs = reinterpret_cast<const SvtHipTxJob *>(d_job); d.quant_rows = reinterpret_cast<const SvtHipQuantRow *>(d_row); d.n_quant_rows = 1;
    d.eob = reinterpret_cast<uint16_t *>(d_out); d.satd = reinterpret_cast<uint32_t *>(d_out + 8); d.dist_coeff = reinterpret_cast<uint64_t *>(d_out + 16);
    d.three_quad_energy = reinterpret_cast<uint64_t *>(d_out + 32); d.sse = reinterpret_cast<uint64_t *>(d_out + 40); d.coeff = reinterpret_cast<int32_t *>(d_coeff);
    if (svt_hip_rd_batch(ctx, &d) != SVT_HIP_OK) leaf_fail("%s", svt_hip_err_buf());
    leaf_check(ctx, hipMemcpyAsync(coeff, d_coeff, (size_t)NP * 4, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    uint64_t tq = 0;
    leaf_check(ctx, hipMemcpyAsync(&tq, d_out + 32, 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    if (three_quad_energy) *three_quad_energy = tq;
    return SVT_HIP_OK;
    } catch (const LeafFailure &f) { return svt_hip_fail(nullptr, SVT_HIP_ERR_LAUNCH, "svt_hip_estimate_transform: %s", f.what); }
}

} // extern "C"

// ---------------------------------------------------------------------------------------------------------
// The 8x8-based SAD pyramid of the integer search as pointer-level entries (aom_dsp_rtcd.h:842-855; bodies
// Codec/motion_estimation.c:98-425).  In production these live inside svt_hip_me_b64_kernel; here one small launch per call.
// ---------------------------------------------------------------------------------------------------------
namespace {

struct ExtSadParams {
    const uint8_t *src, *ref;
    uint32_t       src_stride, ref_stride, mv;
    int            n16, npos, sub_sad;
    uint32_t      *best8, *best16, *mv8, *mv16, *sad16, *sad8;
};

__device__ __forceinline__ uint32_t mv_plus_x(uint32_t mv, int k) {
    const int16_t x = (int16_t)((int16_t)(mv & 0xFFFF) + (int16_t)k);
    return (mv & 0xFFFF0000u) | (uint16_t)x;
}

// lane = 8x8 block in the order of the best arrays: (16x16 in the reference's PU order) * 4 + quadrant (motion_estimation.c:341)
__global__ void __launch_bounds__(64) ext_sad_8x8_16x16_kernel(const ExtSadParams p) {
    const int  lane = threadIdx.x, z16 = lane >> 2, q = lane & 3;
    const bool live = z16 < p.n16;
    const int  z2r[16] = {0, 1, 4, 5, 2, 3, 6, 7, 8, 9, 12, 13, 10, 11, 14, 15}; // raster <-> PU order of the 16x16s (its own inverse)
    const int  b   = p.n16 == 16 ? z2r[z16 & 15] : 0;
    const int  row = (b >> 2) * 16 + (q >> 1) * 8, col = (b & 3) * 16 + (q & 1) * 8;
    uint32_t best = live ? p.best8[lane] : 0, bmv = live ? p.mv8[lane] : 0;
    uint32_t b16 = (live && q == 0) ? p.best16[z16] : 0, m16 = (live && q == 0) ? p.mv16[z16] : 0;
    for (int k = 0; k < p.npos; k++) {
        uint32_t v = 0;
        if (live) {
            const int step = p.sub_sad ? 2 : 1; // svt_aom_compute8x4_sad_kernel_c on every other row, doubled (:42-91,105-136)
            for (int r = 0; r < 8; r += step)
                for (int c = 0; c < 8; c++) {
                    const int d = (int)p.src[(size_t)(row + r) * p.src_stride + col + c] - (int)p.ref[(size_t)(row + r) * p.ref_stride + col + c + k];
                    v += (uint32_t)(d < 0 ? -d : d);
                }
            if (p.sub_sad) v <<= 1;
            if (v < best) { best = v; bmv = mv_plus_x(p.mv, k); }
            if (p.sad8 && p.npos == 1) p.sad8[lane] = v;
        }
        uint32_t total = v + __shfl_xor(v, 1, 64);
        total += __shfl_xor(total, 2, 64);
        if (live && q == 0) {
            p.sad16[z16 * p.npos + k] = total;
            if (total < b16) { b16 = total; m16 = mv_plus_x(p.mv, k); }
        }
    }
    if (live) { p.best8[lane] = best; p.mv8[lane] = bmv; }
    if (live && q == 0) { p.best16[z16] = b16; p.mv16[z16] = m16; }
}

// svt_ext_{eight_,}sad_calculation_32x32_64x64 (:171-205,369-425): sums of four 16x16 SADs per 32x32, of four 32x32 per 64x64
__global__ void ext_sad_32x32_64x64_kernel(const uint32_t *sad16, int npos, uint32_t mv, uint32_t *best32, uint32_t *best64, uint32_t *mv32, uint32_t *mv64,
                                           uint32_t *sad32) {
    if (threadIdx.x != 0) return;
    for (int k = 0; k < npos; k++) {
        uint32_t total = 0;
        for (int q = 0; q < 4; q++) {
            const uint32_t s = sad16[(4 * q) * npos + k] + sad16[(4 * q + 1) * npos + k] + sad16[(4 * q + 2) * npos + k] + sad16[(4 * q + 3) * npos + k];
            sad32[q * npos + k] = s;
            if (s < best32[q]) { best32[q] = s; mv32[q] = mv_plus_x(mv, k); }
            total += s;
        }
        if (total < best64[0]) { best64[0] = total; mv64[0] = mv_plus_x(mv, k); }
    }
}

__global__ void fill_u32_kernel(uint32_t *p, uint32_t n, uint32_t v) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

void leaf_ext_8x8_16x16(const uint8_t *src, uint32_t src_stride, const uint8_t *ref, uint32_t ref_stride, uint32_t mv, uint32_t *best8, uint32_t *best16,
                        uint32_t *mv8, uint32_t *mv16, uint32_t *sad16, uint32_t *sad8, bool sub_sad, int n16, int npos) {
    std::lock_guard<std::mutex> lock(leaf_mutex());
    SvtHipContext *ctx = leaf_ctx();
    const int    side = n16 == 16 ? 64 : 16, n8 = n16 * 4;
    const size_t sbytes = ((size_t)side - 1) * src_stride + side, rbytes = ((size_t)side - 1) * ref_stride + side + npos - 1;
    const size_t sb = align256(sbytes), rb = align256(rbytes);
    uint8_t *base = leaf_scratch(ctx, sb + rb + 4096);
    uint32_t *d_u = reinterpret_cast<uint32_t *>(base + sb + rb); // best8[64] best16[16] mv8[64] mv16[16] sad16[128] sad8[64]
    leaf_check(ctx, hipMemcpyAsync(base, src, sbytes, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(base + sb, ref, rbytes, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(d_u, best8, n8 * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(d_u + 64, best16, n16 * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(d_u + 80, mv8, n8 * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(d_u + 144, mv16, n16 * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    ExtSadParams p;
    p.src = base; p.ref = base + sb; p.src_stride = src_stride; p.ref_stride = ref_stride; p.mv = mv; p.n16 = n16; p.npos = npos; p.sub_sad = sub_sad ? 1 : 0;
    p.best8 = d_u; p.best16 = d_u + 64; p.mv8 = d_u + 80; p.mv16 = d_u + 144; p.sad16 = d_u + 160; p.sad8 = sad8 ? d_u + 288 : nullptr;
    hipLaunchKernelGGL(ext_sad_8x8_16x16_kernel, dim3(1), dim3(64), 0, ctx->stream, p);
    leaf_check(ctx, hipGetLastError(), "ext_sad_8x8_16x16_kernel launch");
    leaf_check(ctx, hipMemcpyAsync(best8, d_u, n8 * 4, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(best16, d_u + 64, n16 * 4, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(mv8, d_u + 80, n8 * 4, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(mv16, d_u + 144, n16 * 4, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(sad16, d_u + 160, (size_t)n16 * npos * 4, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    if (sad8) leaf_check(ctx, hipMemcpyAsync(sad8, d_u + 288, n8 * 4, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
}

void leaf_ext_32x32_64x64(const uint32_t *sad16, int npos, uint32_t mv, uint32_t *best32, uint32_t *best64, uint32_t *mv32, uint32_t *mv64, uint32_t *sad32) {
    std::lock_guard<std::mutex> lock(leaf_mutex());
    SvtHipContext *ctx = leaf_ctx();
    uint32_t *d_u = reinterpret_cast<uint32_t *>(leaf_scratch(ctx, 2048)); // sad16[128] best32[4] best64[1] mv32[4] mv64[1] sad32[32]
    leaf_check(ctx, hipMemcpyAsync(d_u, sad16, (size_t)16 * npos * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(d_u + 128, best32, 16, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(d_u + 132, best64, 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(d_u + 136, mv32, 16, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(d_u + 140, mv64, 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    hipLaunchKernelGGL(ext_sad_32x32_64x64_kernel, dim3(1), dim3(64), 0, ctx->stream, d_u, npos, mv, d_u + 128, d_u + 132, d_u + 136, d_u + 140, d_u + 144);
    leaf_check(ctx, hipGetLastError(), "ext_sad_32x32_64x64_kernel launch");
    leaf_check(ctx, hipMemcpyAsync(best32, d_u + 128, 16, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(best64, d_u + 132, 4, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(mv32, d_u + 136, 16, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(mv64, d_u + 140, 4, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(sad32, d_u + 144, (size_t)4 * npos * 4, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
}

} // namespace

extern "C" {

void svt_ext_all_sad_calculation_8x8_16x16_hip(uint8_t *src, uint32_t src_stride, uint8_t *ref, uint32_t ref_stride, uint32_t mv, uint32_t *p_best_sad_8x8,
                                               uint32_t *p_best_sad_16x16, uint32_t *p_best_mv8x8, uint32_t *p_best_mv16x16, uint32_t p_eight_sad16x16[16][8],
                                               uint32_t p_eight_sad8x8[64][8], bool sub_sad) LEAF_TRY
    (void)p_eight_sad8x8; // left untouched, like the C body (motion_estimation.c:335-362 never stores to it)
    leaf_ext_8x8_16x16(src, src_stride, ref, ref_stride, mv, p_best_sad_8x8, p_best_sad_16x16, p_best_mv8x8, p_best_mv16x16, &p_eight_sad16x16[0][0], nullptr,
                       sub_sad, 16, 8);
LEAF_CATCH(svt_ext_all_sad_calculation_8x8_16x16_hip, src, src_stride, ref, ref_stride, mv, p_best_sad_8x8, p_best_sad_16x16, p_best_mv8x8, p_best_mv16x16, p_eight_sad16x16, p_eight_sad8x8, sub_sad)

void svt_ext_sad_calculation_8x8_16x16_hip(uint8_t *src, uint32_t src_stride, uint8_t *ref, uint32_t ref_stride, uint32_t *p_best_sad_8x8,
                                           uint32_t *p_best_sad_16x16, uint32_t *p_best_mv8x8, uint32_t *p_best_mv16x16, uint32_t mv, uint32_t *p_sad16x16,
                                           uint32_t *p_sad8x8, bool sub_sad) LEAF_TRY
    leaf_ext_8x8_16x16(src, src_stride, ref, ref_stride, mv, p_best_sad_8x8, p_best_sad_16x16, p_best_mv8x8, p_best_mv16x16, p_sad16x16, p_sad8x8, sub_sad, 1, 1);
LEAF_CATCH(svt_ext_sad_calculation_8x8_16x16_hip, src, src_stride, ref, ref_stride, p_best_sad_8x8, p_best_sad_16x16, p_best_mv8x8, p_best_mv16x16, mv, p_sad16x16, p_sad8x8, sub_sad)

void svt_ext_eight_sad_calculation_32x32_64x64_hip(uint32_t p_sad16x16[16][8], uint32_t *p_best_sad_32x32, uint32_t *p_best_sad_64x64, uint32_t *p_best_mv32x32,
                                                   uint32_t *p_best_mv64x64, uint32_t mv, uint32_t p_sad32x32[4][8]) LEAF_TRY
    leaf_ext_32x32_64x64(&p_sad16x16[0][0], 8, mv, p_best_sad_32x32, p_best_sad_64x64, p_best_mv32x32, p_best_mv64x64, &p_sad32x32[0][0]);
LEAF_CATCH(svt_ext_eight_sad_calculation_32x32_64x64_hip, p_sad16x16, p_best_sad_32x32, p_best_sad_64x64, p_best_mv32x32, p_best_mv64x64, mv, p_sad32x32)

void svt_ext_sad_calculation_32x32_64x64_hip(uint32_t *p_sad16x16, uint32_t *p_best_sad_32x32, uint32_t *p_best_sad_64x64, uint32_t *p_best_mv32x32,
                                             uint32_t *p_best_mv64x64, uint32_t mv, uint32_t *p_sad32x32) LEAF_TRY
    leaf_ext_32x32_64x64(p_sad16x16, 1, mv, p_best_sad_32x32, p_best_sad_64x64, p_best_mv32x32, p_best_mv64x64, p_sad32x32);
LEAF_CATCH(svt_ext_sad_calculation_32x32_64x64_hip, p_sad16x16, p_best_sad_32x32, p_best_sad_64x64, p_best_mv32x32, p_best_mv64x64, mv, p_sad32x32)

void svt_initialize_buffer_32bits_hip(uint32_t *pointer, uint32_t count128, uint32_t count32, uint32_t value) LEAF_TRY
    const uint32_t n = count128 * 4 + count32; // me_sad_calculation.c:14-17
    if (!n) return;
    std::lock_guard<std::mutex> lock(leaf_mutex());
    SvtHipContext *ctx = leaf_ctx();
    uint32_t *d = reinterpret_cast<uint32_t *>(leaf_scratch(ctx, (size_t)n * 4));
    hipLaunchKernelGGL(fill_u32_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, d, n, value);
    leaf_check(ctx, hipGetLastError(), "fill_u32_kernel launch");
    leaf_check(ctx, hipMemcpyAsync(pointer, d, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
LEAF_CATCH(svt_initialize_buffer_32bits_hip, pointer, count128, count32, value)

} // extern "C"

// ---------------------------------------------------------------------------------------------------------
// Quantizers as pointer-level entries (aom_dsp_rtcd.h:244-263; bodies Codec/full_loop.c:29-79,149-198 ("b"), :282-474 ("fp")).
// In production they are a stage of rd_tx_kernel; here one launch over a caller-supplied coefficient array.
// ---------------------------------------------------------------------------------------------------------
namespace {

struct QuantLeafParams {
    const int32_t *coeff;
    int32_t       *qcoeff, *dqcoeff;
    uint32_t      *eob;
    const int16_t *iscan;
    const uint8_t *qm, *iqm; // null = flat (1 << AOM_QM_BITS)
    int            n, log_scale, hbd, fp;
    int16_t        zbin[2], round[2], quant[2], quant_shift[2], dequant[2]; // [0] = DC, [1] = AC; round / quant are the fp rows when fp
};

__global__ void __launch_bounds__(256) quantize_leaf_kernel(const QuantLeafParams p) {
    __shared__ uint32_t s_eob;
    if (threadIdx.x == 0) s_eob = 0;
    __syncthreads();
    const int ls = p.log_scale;
    uint32_t  eob = 0;
    for (int rc = threadIdx.x; rc < p.n; rc += 256) {
        const int     ac = rc != 0;
        const int32_t co = p.coeff[rc], sign = co < 0 ? -1 : 0, a = (co ^ sign) - sign;
        const int32_t wt = p.qm ? p.qm[rc] : 32, iwt = p.iqm ? p.iqm[rc] : 32; // AOM_QM_BITS = 5
        const int32_t rnd = ls ? ((p.round[ac] + (1 << (ls - 1))) >> ls) : p.round[ac];
        int32_t qv = 0, dq = 0;
        if (!p.fp) { // svt_aom_quantize_b_c_ii / svt_aom_highbd_quantize_b_c
            const int32_t zb = ls ? ((p.zbin[ac] + (1 << (ls - 1))) >> ls) : p.zbin[ac];
            if ((i64)a * wt >= ((i64)zb << 5)) {
                i64 t = (i64)a + rnd;
                if (!p.hbd) t = t < -32768 ? -32768 : (t > 32767 ? 32767 : t);
                t *= wt;
                qv = (int32_t)(((((t * p.quant[ac]) >> 16) + t) * p.quant_shift[ac]) >> (16 - ls + 5));
                dq = (qv * (((int32_t)p.dequant[ac] * iwt + 16) >> 5)) >> ls;
            }
        } else if (!p.qm && !p.iqm) { // quantize_fp_helper_c / highbd_quantize_fp_helper_c, flat
            const bool keep = p.hbd ? ((a << (1 + ls)) >= p.dequant[ac]) : (((i64)a << (1 + ls)) >= (int32_t)p.dequant[ac]);
            if (keep) {
                i64 t = (i64)a + rnd;
                if (!p.hbd) t = t < -32768 ? -32768 : (t > 32767 ? 32767 : t);
                qv = (int32_t)((t * p.quant[ac]) >> (16 - ls));
                dq = (qv * (int32_t)p.dequant[ac]) >> ls;
            }
        } else if ((i64)a * wt >= ((int32_t)p.dequant[ac] << (5 - (1 + ls)))) { // the helpers' matrix branch
            i64 t = (i64)a + rnd;
            if (!p.hbd) t = t < -32768 ? -32768 : (t > 32767 ? 32767 : t);
            qv = (int32_t)((t * p.quant[ac] * wt) >> (16 - ls + 5));
            dq = (qv * (((int32_t)p.dequant[ac] * iwt + 16) >> 5)) >> ls;
        }
        p.qcoeff[rc]  = (qv ^ sign) - sign;
        p.dqcoeff[rc] = (dq ^ sign) - sign;
        if (qv) { const uint32_t e = (uint32_t)p.iscan[rc] + 1; eob = e > eob ? e : eob; }
    }
    atomicMax(&s_eob, eob);
    __syncthreads();
    if (threadIdx.x == 0) *p.eob = s_eob;
}

void leaf_quantize(const int32_t *coeff, intptr_t n, const int16_t *zbin, const int16_t *round, const int16_t *quant, const int16_t *quant_shift, int32_t *qcoeff,
                   int32_t *dqcoeff, const int16_t *dequant, uint16_t *eob, const int16_t *iscan, const uint8_t *qm, const uint8_t *iqm, int log_scale, int hbd,
                   int fp) {
    std::lock_guard<std::mutex> lock(leaf_mutex());
    SvtHipContext *ctx = leaf_ctx();
    *eob = 0;
    if (n <= 0) return;
    const size_t cb = align256((size_t)n * 4), ib = align256((size_t)n * 2), mb = align256((size_t)n);
    uint8_t *base = leaf_scratch(ctx, 3 * cb + ib + 2 * mb + 256);
    QuantLeafParams p;
    memset(&p, 0, sizeof(p));
    p.coeff = reinterpret_cast<int32_t *>(base); p.qcoeff = reinterpret_cast<int32_t *>(base + cb); p.dqcoeff = reinterpret_cast<int32_t *>(base + 2 * cb);
    p.iscan = reinterpret_cast<int16_t *>(base + 3 * cb);
    uint8_t *d_qm = base + 3 * cb + ib, *d_iqm = d_qm + mb;
    p.eob = reinterpret_cast<uint32_t *>(d_iqm + mb);
    leaf_check(ctx, hipMemcpyAsync(base, coeff, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(base + 3 * cb, iscan, (size_t)n * 2, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    if (qm) { leaf_check(ctx, hipMemcpyAsync(d_qm, qm, (size_t)n, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync"); p.qm = d_qm; }
    if (iqm) { leaf_check(ctx, hipMemcpyAsync(d_iqm, iqm, (size_t)n, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync"); p.iqm = d_iqm; }
    p.n = (int)n; p.log_scale = log_scale; p.hbd = hbd; p.fp = fp;
    for (int k = 0; k < 2; k++) { // MacroblockPlane rows: [0] = DC, [1..7] = AC
        p.zbin[k] = zbin ? zbin[k] : 0; p.round[k] = round[k]; p.quant[k] = quant[k]; p.quant_shift[k] = quant_shift ? quant_shift[k] : 0; p.dequant[k] = dequant[k];
    }
    hipLaunchKernelGGL(quantize_leaf_kernel, dim3(1), dim3(256), 0, ctx->stream, p);
    leaf_check(ctx, hipGetLastError(), "quantize_leaf_kernel launch");
    uint32_t e = 0;
    leaf_check(ctx, hipMemcpyAsync(qcoeff, p.qcoeff, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(dqcoeff, p.dqcoeff, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(&e, p.eob, 4, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    *eob = (uint16_t)e;
}

} // namespace

extern "C" {

#define SVT_HIP_QUANT_B(NAME, HBD)                                                                                                                        \
    void NAME(const int32_t *coeff_ptr, intptr_t n_coeffs, const int16_t *zbin_ptr, const int16_t *round_ptr, const int16_t *quant_ptr,                 \
              const int16_t *quant_shift_ptr, int32_t *qcoeff_ptr, int32_t *dqcoeff_ptr, const int16_t *dequant_ptr, uint16_t *eob_ptr, const int16_t *scan, \
              const int16_t *iscan, const uint8_t *qm_ptr, const uint8_t *iqm_ptr, const int32_t log_scale) LEAF_TRY                                     \
        (void)scan;                                                                                                                                      \
        leaf_quantize(coeff_ptr, n_coeffs, zbin_ptr, round_ptr, quant_ptr, quant_shift_ptr, qcoeff_ptr, dqcoeff_ptr, dequant_ptr, eob_ptr, iscan, qm_ptr, iqm_ptr, \
                      log_scale, HBD, 0);                                                                                                                \
    LEAF_CATCH(NAME, coeff_ptr, n_coeffs, zbin_ptr, round_ptr, quant_ptr, quant_shift_ptr, qcoeff_ptr, dqcoeff_ptr, dequant_ptr, eob_ptr, scan, iscan, qm_ptr, iqm_ptr, log_scale)
SVT_HIP_QUANT_B(svt_aom_quantize_b_hip, 0)
SVT_HIP_QUANT_B(svt_aom_highbd_quantize_b_hip, 1)
SVT_HIP_QUANT_B(svt_av1_quantize_b_qm_hip, 0)
SVT_HIP_QUANT_B(svt_av1_highbd_quantize_b_qm_hip, 1)
#undef SVT_HIP_QUANT_B

#define SVT_HIP_QUANT_FP(NAME, LS)                                                                                                                       \
    void NAME(const int32_t *coeff_ptr, intptr_t n_coeffs, const int16_t *zbin_ptr, const int16_t *round_ptr, const int16_t *quant_ptr,                 \
              const int16_t *quant_shift_ptr, int32_t *qcoeff_ptr, int32_t *dqcoeff_ptr, const int16_t *dequant_ptr, uint16_t *eob_ptr, const int16_t *scan, \
              const int16_t *iscan) LEAF_TRY                                                                                                             \
        (void)scan;                                                                                                                                      \
        leaf_quantize(coeff_ptr, n_coeffs, zbin_ptr, round_ptr, quant_ptr, quant_shift_ptr, qcoeff_ptr, dqcoeff_ptr, dequant_ptr, eob_ptr, iscan, nullptr, nullptr, \
                      LS, 0, 1);                                                                                                                         \
    LEAF_CATCH(NAME, coeff_ptr, n_coeffs, zbin_ptr, round_ptr, quant_ptr, quant_shift_ptr, qcoeff_ptr, dqcoeff_ptr, dequant_ptr, eob_ptr, scan, iscan)
SVT_HIP_QUANT_FP(svt_av1_quantize_fp_hip, 0)
SVT_HIP_QUANT_FP(svt_av1_quantize_fp_32x32_hip, 1)
SVT_HIP_QUANT_FP(svt_av1_quantize_fp_64x64_hip, 2)
#undef SVT_HIP_QUANT_FP

void svt_av1_quantize_fp_qm_hip(const int32_t *coeff_ptr, intptr_t n_coeffs, const int16_t *zbin_ptr, const int16_t *round_ptr, const int16_t *quant_ptr,
                                const int16_t *quant_shift_ptr, int32_t *qcoeff_ptr, int32_t *dqcoeff_ptr, const int16_t *dequant_ptr, uint16_t *eob_ptr,
                                const int16_t *scan, const int16_t *iscan, const uint8_t *qm_ptr, const uint8_t *iqm_ptr, int16_t log_scale) LEAF_TRY
    (void)scan;
    leaf_quantize(coeff_ptr, n_coeffs, zbin_ptr, round_ptr, quant_ptr, quant_shift_ptr, qcoeff_ptr, dqcoeff_ptr, dequant_ptr, eob_ptr, iscan, qm_ptr, iqm_ptr, log_scale, 0, 1);
LEAF_CATCH(svt_av1_quantize_fp_qm_hip, coeff_ptr, n_coeffs, zbin_ptr, round_ptr, quant_ptr, quant_shift_ptr, qcoeff_ptr, dqcoeff_ptr, dequant_ptr, eob_ptr, scan, iscan, qm_ptr, iqm_ptr, log_scale)
void svt_av1_highbd_quantize_fp_hip(const int32_t *coeff_ptr, intptr_t n_coeffs, const int16_t *zbin_ptr, const int16_t *round_ptr, const int16_t *quant_ptr,
                                    const int16_t *quant_shift_ptr, int32_t *qcoeff_ptr, int32_t *dqcoeff_ptr, const int16_t *dequant_ptr, uint16_t *eob_ptr,
                                    const int16_t *scan, const int16_t *iscan, int16_t log_scale) LEAF_TRY
    (void)scan;
    leaf_quantize(coeff_ptr, n_coeffs, zbin_ptr, round_ptr, quant_ptr, quant_shift_ptr, qcoeff_ptr, dqcoeff_ptr, dequant_ptr, eob_ptr, iscan, nullptr, nullptr, log_scale, 1, 1);
LEAF_CATCH(svt_av1_highbd_quantize_fp_hip, coeff_ptr, n_coeffs, zbin_ptr, round_ptr, quant_ptr, quant_shift_ptr, qcoeff_ptr, dqcoeff_ptr, dequant_ptr, eob_ptr, scan, iscan, log_scale)
void svt_av1_highbd_quantize_fp_qm_hip(const int32_t *coeff_ptr, intptr_t n_coeffs, const int16_t *zbin_ptr, const int16_t *round_ptr, const int16_t *quant_ptr,
                                       const int16_t *quant_shift_ptr, int32_t *qcoeff_ptr, int32_t *dqcoeff_ptr, const int16_t *dequant_ptr, uint16_t *eob_ptr,
                                       const int16_t *scan, const int16_t *iscan, const uint8_t *qm_ptr, const uint8_t *iqm_ptr, int16_t log_scale) LEAF_TRY
    (void)scan;
    leaf_quantize(coeff_ptr, n_coeffs, zbin_ptr, round_ptr, quant_ptr, quant_shift_ptr, qcoeff_ptr, dqcoeff_ptr, dequant_ptr, eob_ptr, iscan, qm_ptr, iqm_ptr, log_scale, 1, 1);
LEAF_CATCH(svt_av1_highbd_quantize_fp_qm_hip, coeff_ptr, n_coeffs, zbin_ptr, round_ptr, quant_ptr, quant_shift_ptr, qcoeff_ptr, dqcoeff_ptr, dequant_ptr, eob_ptr, scan, iscan, qm_ptr, iqm_ptr, log_scale)

} // extern "C"

// ---------------------------------------------------------------------------------------------------------
// svt_av1_inv_txfm2d_add_{W}x{H} (common_dsp_rtcd.h:100-141; bodies Codec/inv_transforms.c:2459-2716) as pointer-level
// entries: uint16 planes for either bit depth, separate read / write pointers, packed coefficients for the 64-point sizes.
// ---------------------------------------------------------------------------------------------------------
namespace {
void leaf_inv_txfm(const int32_t *input, const uint16_t *out_r, int32_t stride_r, uint16_t *out_w, int32_t stride_w, int tx_type, int tx_size, int bd) {
    std::lock_guard<std::mutex> lock(leaf_mutex());
    SvtHipContext *ctx = leaf_ctx();
    if ((bd != 8 && bd != 10) || tx_size < 0 || tx_size >= SVT_HIP_TX_SIZES_ALL || tx_type < 0 || tx_type >= SVT_HIP_TX_TYPES || stride_r <= 0 || stride_w <= 0) {
        leaf_fail("svt_av1_inv_txfm2d_add_hip: unsupported bd %d / tx_size %d / tx_type %d", bd, tx_size, tx_type);
    }
    const int W = svt_hip_tx_size_wide(tx_size), H = svt_hip_tx_size_high(tx_size), NP = (W > 32 ? 32 : W) * (H > 32 ? 32 : H);
    const size_t cb = align256((size_t)NP * 4), rbytes = (((size_t)H - 1) * stride_r + W) * 2, wbytes = (size_t)W * H * 2;
    uint8_t *base = leaf_scratch(ctx, cb + align256(rbytes) + align256(wbytes) + 256);
    uint8_t *d_co = base, *d_pred = d_co + cb, *d_rec = d_pred + align256(rbytes), *d_job = d_rec + align256(wbytes);
    leaf_check(ctx, hipMemcpyAsync(d_co, input, (size_t)NP * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(d_pred, out_r, rbytes, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    SvtHipTxJob job;
    memset(&job, 0, sizeof(job));
    job.tx_type = (uint8_t)tx_type;
    leaf_check(ctx, hipMemcpyAsync(d_job, &job, sizeof(job), hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    SvtHipInvTxBatchDesc d;
    memset(&d, 0, sizeof(d));
    d.bit_depth = (uint8_t)bd; d.sample_bytes = 2; d.tx_size = (uint8_t)tx_size; d.n_jobs = 1; d.pred_stride = (uint32_t)stride_r; d.recon_stride = (uint32_t)W;
    d.pred = d_pred; d.recon = d_rec; d.jobs = reinterpret_cast<const SvtHipTxJob *>(d_job); d.dqcoeff = reinterpret_cast<const int32_t *>(d_co);
    if (svt_hip_inv_txfm_batch(ctx, &d) != SVT_HIP_OK) leaf_fail("%s", svt_hip_err_buf());
    leaf_check(ctx, hipMemcpy2DAsync(out_w, (size_t)stride_w * 2, d_rec, (size_t)W * 2, (size_t)W * 2, H, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy2DAsync");
    leaf_check(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
}
} // namespace

extern "C" {
// TxType and TxSize are one-byte (ATTRIBUTE_PACKED) enums in the reference (definitions.h): uint8_t is the same ABI
#define SVT_HIP_INV_SQ(W, H, TS)                                                                                                                       \
    void svt_av1_inv_txfm2d_add_##W##x##H##_hip(const int32_t *input, uint16_t *output_r, int32_t stride_r, uint16_t *output_w, int32_t stride_w, uint8_t tx_type, \
                                                int32_t bd) LEAF_TRY                                                                                  \
        leaf_inv_txfm(input, output_r, stride_r, output_w, stride_w, tx_type, TS, bd);                                                                \
    LEAF_CATCH(svt_av1_inv_txfm2d_add_##W##x##H##_hip, input, output_r, stride_r, output_w, stride_w, tx_type, bd)
SVT_HIP_INV_SQ(4, 4, 0) SVT_HIP_INV_SQ(8, 8, 1) SVT_HIP_INV_SQ(16, 16, 2) SVT_HIP_INV_SQ(32, 32, 3) SVT_HIP_INV_SQ(64, 64, 4)
#undef SVT_HIP_INV_SQ
#define SVT_HIP_INV_RECT(W, H, TS)                                                                                                                     \
    void svt_av1_inv_txfm2d_add_##W##x##H##_hip(const int32_t *input, uint16_t *output_r, int32_t stride_r, uint16_t *output_w, int32_t stride_w, uint8_t tx_type, \
                                                uint8_t tx_size, int32_t eob, int32_t bd) LEAF_TRY                                                    \
        /* eob only lets the reference skip zero rows; the result does not depend on it */                                                            \
        leaf_inv_txfm(input, output_r, stride_r, output_w, stride_w, tx_type, TS, bd);                                                                \
    LEAF_CATCH(svt_av1_inv_txfm2d_add_##W##x##H##_hip, input, output_r, stride_r, output_w, stride_w, tx_type, tx_size, eob, bd)
SVT_HIP_INV_RECT(8, 16, 7) SVT_HIP_INV_RECT(16, 8, 8) SVT_HIP_INV_RECT(16, 32, 9) SVT_HIP_INV_RECT(32, 16, 10) SVT_HIP_INV_RECT(32, 64, 11) SVT_HIP_INV_RECT(64, 32, 12)
SVT_HIP_INV_RECT(8, 32, 15) SVT_HIP_INV_RECT(32, 8, 16) SVT_HIP_INV_RECT(16, 64, 17) SVT_HIP_INV_RECT(64, 16, 18)
#undef SVT_HIP_INV_RECT
#define SVT_HIP_INV_SMALL(W, H, TS)                                                                                                                    \
    void svt_av1_inv_txfm2d_add_##W##x##H##_hip(const int32_t *input, uint16_t *output_r, int32_t stride_r, uint16_t *output_w, int32_t stride_w, uint8_t tx_type, \
                                                uint8_t tx_size, int32_t bd) LEAF_TRY                                                                 \
        leaf_inv_txfm(input, output_r, stride_r, output_w, stride_w, tx_type, TS, bd);                                                                \
    LEAF_CATCH(svt_av1_inv_txfm2d_add_##W##x##H##_hip, input, output_r, stride_r, output_w, stride_w, tx_type, tx_size, bd)
SVT_HIP_INV_SMALL(4, 8, 5) SVT_HIP_INV_SMALL(8, 4, 6) SVT_HIP_INV_SMALL(4, 16, 13) SVT_HIP_INV_SMALL(16, 4, 14)
#undef SVT_HIP_INV_SMALL
} // extern "C"

// ---------------------------------------------------------------------------------------------------------
// svt_av1_fwd_txfm2d_{W}x{H}{,_N2,_N4} (aom_dsp_rtcd.h / aom_dsp_rtcd.c:421-487; bodies Codec/transforms.c) as pointer-level
// entries: the full W x H coefficient array, like the reference's per-size pointers (bd only selects stage ranges there).
// ---------------------------------------------------------------------------------------------------------
namespace {
void leaf_fwd_txfm(const int16_t *input, int32_t *output, uint32_t stride, int tx_type, int tx_size, int pf_shape) {
    std::lock_guard<std::mutex> lock(leaf_mutex());
    SvtHipContext *ctx = leaf_ctx();
    if (tx_type < 0 || tx_type >= SVT_HIP_TX_TYPES) leaf_fail("svt_av1_fwd_txfm2d_hip: tx_type %d", tx_type);
    const int W = svt_hip_tx_size_wide(tx_size), H = svt_hip_tx_size_high(tx_size);
    const size_t rbytes = (((size_t)H - 1) * stride + W) * 2, obytes = (size_t)W * H * 4;
    uint8_t *base = leaf_scratch(ctx, align256(rbytes) + align256(obytes) + 256);
    uint8_t *d_res = base, *d_out = d_res + align256(rbytes), *d_job = d_out + align256(obytes);
    leaf_check(ctx, hipMemcpyAsync(d_res, input, rbytes, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    SvtHipTxJob job;
    memset(&job, 0, sizeof(job));
    job.tx_type = (uint8_t)tx_type; job.pf_shape = (uint8_t)pf_shape;
    leaf_check(ctx, hipMemcpyAsync(d_job, &job, sizeof(job), hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    SvtHipFwdTxBatchDesc d;
    memset(&d, 0, sizeof(d));
    d.tx_size = (uint8_t)tx_size; d.n_jobs = 1; d.residual_stride = stride; d.residual = reinterpret_cast<const int16_t *>(d_res);
    d.jobs = reinterpret_cast<const SvtHipTxJob *>(d_job); d.coeff = reinterpret_cast<int32_t *>(d_out);
    if (svt_hip_fwd_txfm_batch(ctx, &d) != SVT_HIP_OK) leaf_fail("%s", svt_hip_err_buf());
    leaf_check(ctx, hipMemcpyAsync(output, d_out, obytes, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
}
} // namespace

extern "C" {
#define SVT_HIP_FWD(W, H, TS)                                                                                                                   \
    void svt_av1_fwd_txfm2d_##W##x##H##_hip(int16_t *input, int32_t *output, uint32_t stride, uint8_t tx_type, uint8_t bd) LEAF_TRY                   \
        leaf_fwd_txfm(input, output, stride, tx_type, TS, 0);                                                                         \
    LEAF_CATCH(svt_av1_fwd_txfm2d_##W##x##H##_hip, input, output, stride, tx_type, bd)                                                                                                                                           \
    void svt_av1_fwd_txfm2d_##W##x##H##_N2_hip(int16_t *input, int32_t *output, uint32_t stride, uint8_t tx_type, uint8_t bd) LEAF_TRY                \
        leaf_fwd_txfm(input, output, stride, tx_type, TS, 1);                                                                         \
    LEAF_CATCH(svt_av1_fwd_txfm2d_##W##x##H##_N2_hip, input, output, stride, tx_type, bd)                                                                                                                                           \
    void svt_av1_fwd_txfm2d_##W##x##H##_N4_hip(int16_t *input, int32_t *output, uint32_t stride, uint8_t tx_type, uint8_t bd) LEAF_TRY                \
        leaf_fwd_txfm(input, output, stride, tx_type, TS, 2);                                                                         \
    LEAF_CATCH(svt_av1_fwd_txfm2d_##W##x##H##_N4_hip, input, output, stride, tx_type, bd)
SVT_HIP_FWD(4, 4, 0) SVT_HIP_FWD(8, 8, 1) SVT_HIP_FWD(16, 16, 2) SVT_HIP_FWD(32, 32, 3) SVT_HIP_FWD(64, 64, 4) SVT_HIP_FWD(4, 8, 5) SVT_HIP_FWD(8, 4, 6)
SVT_HIP_FWD(8, 16, 7) SVT_HIP_FWD(16, 8, 8) SVT_HIP_FWD(16, 32, 9) SVT_HIP_FWD(32, 16, 10) SVT_HIP_FWD(32, 64, 11) SVT_HIP_FWD(64, 32, 12) SVT_HIP_FWD(4, 16, 13)
SVT_HIP_FWD(16, 4, 14) SVT_HIP_FWD(8, 32, 15) SVT_HIP_FWD(32, 8, 16) SVT_HIP_FWD(16, 64, 17) SVT_HIP_FWD(64, 16, 18)
#undef SVT_HIP_FWD
} // extern "C"

// ---------------------------------------------------------------------------------------------------------
// svt_handle_transform{16x64,32x64,64x16,64x32,64x64}{,_N2_N4} (aom_dsp_rtcd.c:440-449; Codec/transforms.c:2374-2543): energy of
// the frequencies a 64-point size discards + in-place packing of the kept 32-wide rows, on a host coefficient array.
// ---------------------------------------------------------------------------------------------------------
namespace {
__global__ void __launch_bounds__(256) handle_transform_kernel(const int32_t *in, int w, int h, int with_energy, int32_t *packed, u64 *energy) {
    __shared__ u64 part[4];
    const int wp = w > 32 ? 32 : w, hp = h > 32 ? 32 : h;
    u64 e = 0;
    for (int i = threadIdx.x; i < w * h; i += 256) {
        const int r = i / w, c = i - r * w;
        const int32_t v = in[i];
        if (r < hp && c < wp) packed[r * wp + c] = v;
        else if (with_energy) e += (u64)((i64)v * v);
    }
    for (int o = 32; o > 0; o >>= 1) e += __shfl_xor((unsigned long long)e, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) *energy = part[0] + part[1] + part[2] + part[3];
}

uint64_t leaf_handle_transform(int32_t *output, int w, int h, int with_energy) {
    std::lock_guard<std::mutex> lock(leaf_mutex());
    SvtHipContext *ctx = leaf_ctx();
    const int    wp = w > 32 ? 32 : w, hp = h > 32 ? 32 : h;
    const size_t ib = align256((size_t)w * h * 4), pb = align256((size_t)wp * hp * 4);
    uint8_t *base = leaf_scratch(ctx, ib + pb + 256);
    leaf_check(ctx, hipMemcpyAsync(base, output, (size_t)w * h * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    hipLaunchKernelGGL(handle_transform_kernel, dim3(1), dim3(256), 0, ctx->stream, reinterpret_cast<const int32_t *>(base), w, h, with_energy,
                       reinterpret_cast<int32_t *>(base + ib), reinterpret_cast<u64 *>(base + ib + pb));
    leaf_check(ctx, hipGetLastError(), "handle_transform_kernel launch");
    uint64_t e = 0;
    // only the 64-wide sizes are re-packed (rows of 64 -> rows of 32 at the front of the array; what lies behind keeps its content)
    if (w == 64) leaf_check(ctx, hipMemcpyAsync(output, base + ib, (size_t)wp * hp * 4, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipMemcpyAsync(&e, base + ib + pb, 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    leaf_check(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return e;
}
} // namespace

extern "C" {
uint64_t svt_handle_transform16x64_hip(int32_t *output) LEAF_TRY return leaf_handle_transform(output, 16, 64, 1); LEAF_CATCH(svt_handle_transform16x64_hip, output)
uint64_t svt_handle_transform32x64_hip(int32_t *output) LEAF_TRY return leaf_handle_transform(output, 32, 64, 1); LEAF_CATCH(svt_handle_transform32x64_hip, output)
uint64_t svt_handle_transform64x16_hip(int32_t *output) LEAF_TRY return leaf_handle_transform(output, 64, 16, 1); LEAF_CATCH(svt_handle_transform64x16_hip, output)
uint64_t svt_handle_transform64x32_hip(int32_t *output) LEAF_TRY return leaf_handle_transform(output, 64, 32, 1); LEAF_CATCH(svt_handle_transform64x32_hip, output)
uint64_t svt_handle_transform64x64_hip(int32_t *output) LEAF_TRY return leaf_handle_transform(output, 64, 64, 1); LEAF_CATCH(svt_handle_transform64x64_hip, output)
uint64_t svt_handle_transform16x64_N2_N4_hip(int32_t *output) LEAF_TRY (void)output; return 0; LEAF_CATCH(svt_handle_transform16x64_N2_N4_hip, output) // the reference's bodies are empty too (transforms.c:2514-2521)
uint64_t svt_handle_transform32x64_N2_N4_hip(int32_t *output) LEAF_TRY (void)output; return 0; LEAF_CATCH(svt_handle_transform32x64_N2_N4_hip, output)
uint64_t svt_handle_transform64x16_N2_N4_hip(int32_t *output) LEAF_TRY return leaf_handle_transform(output, 64, 16, 0); LEAF_CATCH(svt_handle_transform64x16_N2_N4_hip, output)
uint64_t svt_handle_transform64x32_N2_N4_hip(int32_t *output) LEAF_TRY return leaf_handle_transform(output, 64, 32, 0); LEAF_CATCH(svt_handle_transform64x32_N2_N4_hip, output)
uint64_t svt_handle_transform64x64_N2_N4_hip(int32_t *output) LEAF_TRY return leaf_handle_transform(output, 64, 64, 0); LEAF_CATCH(svt_handle_transform64x64_N2_N4_hip, output)
} // extern "C"
