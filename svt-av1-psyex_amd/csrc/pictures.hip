// pictures.hip -- HBM-resident luma pyramids (EbPaReferenceObject equivalents) and the 2x2
// decimation + edge padding kernels (reference: Codec/pic_analysis_process.c:130-158,2139-2196,
// Codec/pic_operators.c:397-443).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include "svt_hip_internal.h"

namespace {

constexpr size_t kFrontSlack = 256, kBackSlack = 512;

// One thread per output byte of the PADDED destination plane: coordinates are clamped into the picture, so the
// padding replicates the decimated edge samples exactly as svt_aom_generate_padding does after downsample_2d.
__global__ void downsample2x_pad_kernel(DevPlane src, DevPlane dst) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x; // padded coordinates
    const int y = blockIdx.y;
    const int pw = dst.width + 2 * dst.org_x, ph = dst.height + 2 * dst.org_y;
    if (x >= pw || y >= ph) return;
    int ix = x - dst.org_x, iy = y - dst.org_y;
    ix = ix < 0 ? 0 : (ix > dst.width - 1 ? dst.width - 1 : ix);
    iy = iy < 0 ? 0 : (iy > dst.height - 1 ? dst.height - 1 : iy);
    const uint8_t *s = src.base + (size_t)(src.org_y + 2 * iy) * src.stride + src.org_x + 2 * ix;
    const uint32_t sum = (uint32_t)s[0] + s[1] + s[src.stride] + s[src.stride + 1];
    const_cast<uint8_t *>(dst.base)[(size_t)y * dst.stride + x] = (uint8_t)((sum + 2) >> 2);
}

int alloc_plane(SvtHipContext *ctx, int width, int height, int org_x, int org_y, DevPlane *pl, void **mem, size_t *bytes) {
    const uint32_t stride = (uint32_t)(((width + 2 * org_x + 63) & ~63) + 64);
    const size_t   rows   = (size_t)height + 2 * (size_t)org_y;
    *bytes                = kFrontSlack + (size_t)stride * rows + kBackSlack;
    if (hipMalloc(mem, *bytes) != hipSuccess)
        return svt_hip_fail(ctx, SVT_HIP_ERR_NO_MEMORY, "hipMalloc(%zu) failed", *bytes);
    pl->base   = static_cast<uint8_t *>(*mem) + kFrontSlack;
    pl->stride = stride;
    pl->org_x  = org_x;
    pl->org_y  = org_y;
    pl->width  = width;
    pl->height = height;
    return SVT_HIP_OK;
}

int check_plane(SvtHipContext *ctx, const SvtHipPlaneDesc *p, int min_pad, const char *what) {
    if (!p || !p->buffer_y) return svt_hip_fail(ctx, SVT_HIP_ERR_BAD_PARAM, "%s plane: null", what);
    if (p->width == 0 || p->height == 0 || p->org_x < min_pad || p->org_y < min_pad ||
        p->stride_y < (uint32_t)p->width + 2u * p->org_x)
        return svt_hip_fail(ctx, SVT_HIP_ERR_BAD_PARAM, "%s plane: %ux%u org %u,%u stride %u (needs padding >= %d on every side)", what,
                            p->width, p->height, p->org_x, p->org_y, p->stride_y, min_pad);
    return SVT_HIP_OK;
}

int upload_plane(SvtHipContext *ctx, const SvtHipPlaneDesc *h, DevPlane *d, bool from_device, hipStream_t stream = nullptr) {
    const size_t w = (size_t)h->width + 2 * (size_t)h->org_x, rows = (size_t)h->height + 2 * (size_t)h->org_y;
    SVT_HIP_CHECK(ctx, hipMemcpy2DAsync(const_cast<uint8_t *>(d->base), d->stride, h->buffer_y, h->stride_y, w, rows,
                                        from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream ? stream : ctx->stream));
    return SVT_HIP_OK;
}

int make_level(SvtHipContext *ctx, SvtHipPaPicture *pic, int level, const SvtHipPlaneDesc *host) {
    const DevPlane &src = pic->pyr.lvl[level + 1];
    const int       pad = (level == 1) ? 32 : 16; // b64_size >> 1, b64_size >> 2 (Globals/enc_handle.c:1260-1279)
    int rc = alloc_plane(ctx, src.width >> 1, src.height >> 1, pad, pad, &pic->pyr.lvl[level], &pic->mem[level], &pic->bytes[level]);
    if (rc) return rc;
    DevPlane &dst = pic->pyr.lvl[level];
    if (host) {
        if (host->width != dst.width || host->height != dst.height || host->org_x != pad || host->org_y != pad)
            return svt_hip_fail(ctx, SVT_HIP_ERR_BAD_PARAM, "level %d plane geometry %ux%u pad %u,%u does not match %dx%d pad %d", level,
                                host->width, host->height, host->org_x, host->org_y, dst.width, dst.height, pad);
        return upload_plane(ctx, host, &dst, false);
    }
    const int pw = dst.width + 2 * pad, ph = dst.height + 2 * pad;
    hipLaunchKernelGGL(downsample2x_pad_kernel, dim3((pw + 255) / 256, ph), dim3(256), 0, ctx->stream, src, dst);
    SVT_HIP_CHECK(ctx, hipGetLastError());
    return SVT_HIP_OK;
}

int create_common(SvtHipContext *ctx, const SvtHipPlaneDesc *full, const SvtHipPlaneDesc *quarter, const SvtHipPlaneDesc *sixteenth,
                  bool full_on_device, SvtHipPaPicture **out) {
    if (!ctx || !out) return SVT_HIP_ERR_BAD_PARAM;
    int rc = check_plane(ctx, full, 64, "full");
    if (rc) return rc;
    if (quarter && (rc = check_plane(ctx, quarter, 32, "quarter"))) return rc;
    if (sixteenth && (rc = check_plane(ctx, sixteenth, 16, "sixteenth"))) return rc;
    if ((full->width & 7) || (full->height & 7))
        return svt_hip_fail(ctx, SVT_HIP_ERR_BAD_PARAM, "full plane %ux%u: width and height must be multiples of 8", full->width, full->height);
    SvtHipPaPicture *pic = static_cast<SvtHipPaPicture *>(calloc(1, sizeof(SvtHipPaPicture)));
    if (!pic) return svt_hip_fail(ctx, SVT_HIP_ERR_NO_MEMORY, "calloc");
    rc = svt_hip_use_device(ctx);
    if (!rc) rc = alloc_plane(ctx, full->width, full->height, full->org_x, full->org_y, &pic->pyr.lvl[2], &pic->mem[2], &pic->bytes[2]);
    if (!rc) rc = upload_plane(ctx, full, &pic->pyr.lvl[2], full_on_device);
    if (!rc) rc = make_level(ctx, pic, 1, quarter);
    if (!rc) rc = make_level(ctx, pic, 0, sixteenth);
    // whoever reads the planes on another stream (a synchronous entry on a borrowed lane) waits for this event first
    if (!rc && hipEventCreateWithFlags(&pic->ready, hipEventDisableTiming) != hipSuccess) rc = svt_hip_fail(ctx, SVT_HIP_ERR_LAUNCH, "hipEventCreate failed");
    if (!rc && hipEventRecord(pic->ready, ctx->stream) != hipSuccess) rc = svt_hip_fail(ctx, SVT_HIP_ERR_LAUNCH, "hipEventRecord failed");
    pic->ready_stream = ctx->stream;
    if (rc) {
        svt_hip_pa_picture_destroy(ctx, pic);
        return rc;
    }
    *out = pic;
    return SVT_HIP_OK;
}

} // namespace

extern "C" {

int svt_hip_pa_picture_create(SvtHipContext *ctx, const SvtHipPlaneDesc *full, const SvtHipPlaneDesc *quarter,
                              const SvtHipPlaneDesc *sixteenth, SvtHipPaPicture **pic) {
    return create_common(ctx, full, quarter, sixteenth, false, pic);
}

int svt_hip_pa_picture_create_dev(SvtHipContext *ctx, const SvtHipPlaneDesc *full_dev, SvtHipPaPicture **pic) {
    return create_common(ctx, full_dev, nullptr, nullptr, true, pic);
}

// A picture buffer taken from a pool and filled with the next input picture (the reference recycles its EbPaReferenceObject buffers the
// same way, Codec/reference_object.c): the full plane is copied in again (from page-locked host memory the copy is asynchronous), the
// 1/4 and 1/16 planes are rebuilt on the device.  Enqueued on the context stream.
static int picture_update_on(SvtHipContext *ctx, SvtHipPaPicture *pic, const SvtHipPlaneDesc *full, int full_on_device, hipStream_t stream) {
    int rc = check_plane(ctx, full, 64, "full");
    if (rc) return rc;
    DevPlane &f = pic->pyr.lvl[2];
    if (full->width != f.width || full->height != f.height || full->org_x != f.org_x || full->org_y != f.org_y)
        return svt_hip_fail(ctx, SVT_HIP_ERR_BAD_PARAM, "update: plane %ux%u pad %u,%u does not match the picture's %dx%d pad %d,%d", full->width, full->height,
                            full->org_x, full->org_y, f.width, f.height, f.org_x, f.org_y);
    if ((rc = upload_plane(ctx, full, &f, full_on_device != 0, stream))) return rc;
    for (int level = 1; level >= 0; level--) {
        const DevPlane &src = pic->pyr.lvl[level + 1], &dst = pic->pyr.lvl[level];
        const int pw = dst.width + 2 * dst.org_x, ph = dst.height + 2 * dst.org_y;
        hipLaunchKernelGGL(downsample2x_pad_kernel, dim3((pw + 255) / 256, ph), dim3(256), 0, stream, src, dst);
    }
    SVT_HIP_CHECK(ctx, hipGetLastError());
    SVT_HIP_CHECK(ctx, hipEventRecord(pic->ready, stream));
    pic->ready_stream = stream;
    return SVT_HIP_OK;
}

int svt_hip_pa_picture_update(SvtHipContext *ctx, SvtHipPaPicture *pic, const SvtHipPlaneDesc *full, int full_on_device) {
    if (!ctx || !pic) return SVT_HIP_ERR_BAD_PARAM;
    if (int rc = svt_hip_use_device(ctx)) return rc;
    return picture_update_on(ctx, pic, full, full_on_device, ctx->stream);
}

// The refill on the context's transfer stream: ordered behind everything enqueued on the context stream so far (whatever still reads the
// picture's old content), beside whatever is enqueued afterwards; readers wait through the picture's `ready` event.
int svt_hip_pa_picture_update_ahead(SvtHipContext *ctx, SvtHipPaPicture *pic, const SvtHipPlaneDesc *full, int full_on_device) {
    if (!ctx || !pic) return SVT_HIP_ERR_BAD_PARAM;
    if (int rc = svt_hip_use_device(ctx)) return rc;
    std::lock_guard<std::mutex> lock(ctx->async_mu);
    if (int rc = svt_hip_transfer_stream_make(ctx)) return rc;
    SVT_HIP_CHECK(ctx, hipEventRecord(ctx->io_fence, ctx->stream));
    SVT_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->io_stream, ctx->io_fence, 0));
    return picture_update_on(ctx, pic, full, full_on_device, ctx->io_stream);
}

void svt_hip_pa_picture_destroy(SvtHipContext *ctx, SvtHipPaPicture *pic) {
    if (!pic) return;
    // teardown: a failure below leaves nothing to do differently
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    for (int l = 0; l < 3; l++)
        if (pic->mem[l]) (void)hipFree(pic->mem[l]);
    if (pic->ready) (void)hipEventDestroy(pic->ready);
    free(pic);
}

int svt_hip_pa_picture_geometry(const SvtHipPaPicture *pic, int level, SvtHipPlaneDesc *out) {
    if (!pic || !out || level < 0 || level > 2) return SVT_HIP_ERR_BAD_PARAM;
    const DevPlane &p = pic->pyr.lvl[level];
    out->buffer_y = p.base;
    out->stride_y = p.stride;
    out->org_x    = (uint16_t)p.org_x;
    out->org_y    = (uint16_t)p.org_y;
    out->width    = (uint16_t)p.width;
    out->height   = (uint16_t)p.height;
    return SVT_HIP_OK;
}

int svt_hip_pa_picture_download(SvtHipContext *ctx, const SvtHipPaPicture *pic, int level, uint8_t *dst, uint32_t dst_stride) {
    if (!ctx || !pic || !dst || level < 0 || level > 2) return SVT_HIP_ERR_BAD_PARAM;
    const DevPlane &p = pic->pyr.lvl[level];
    const size_t    w = (size_t)p.width + 2 * (size_t)p.org_x, rows = (size_t)p.height + 2 * (size_t)p.org_y;
    if (dst_stride < w) return svt_hip_fail(ctx, SVT_HIP_ERR_BAD_PARAM, "dst_stride %u < %zu", dst_stride, w);
    if (int rc = svt_hip_wait_picture(ctx, ctx->stream, pic)) return rc; // filled on another stream (a refill ahead): wait for it
    SVT_HIP_CHECK(ctx, hipMemcpy2DAsync(dst, dst_stride, p.base, p.stride, w, rows, hipMemcpyDeviceToHost, ctx->stream));
    SVT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return SVT_HIP_OK;
}

} // extern "C"
