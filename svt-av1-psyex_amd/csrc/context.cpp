// context.cpp -- the host runtime under every entry, host code only: the context, its lanes (svt_hip_internal.h: the threading model) and the
// lane pool, the calling thread's error text, the grow-on-demand device buffers and the transfer stream.
#include <hip/hip_runtime_api.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include "svt_hip_internal.h"

char *svt_hip_err_buf(void) {
    static thread_local char buf[SVT_HIP_ERR_BYTES] = "";
    return buf;
}

int svt_hip_use_device(SvtHipContext *ctx) {
    SVT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    return SVT_HIP_OK;
}

// ---- buffers ---------------------------------------------------------------------------------------------------------
int svt_hip_buffer_reserve(SvtHipContext *ctx, SvtHipBuffer *b, size_t need, hipStream_t reader, const char *failed_fmt) {
    if (need <= b->bytes) return SVT_HIP_OK;
    if (b->ptr) {
        SVT_HIP_CHECK(ctx, hipStreamSynchronize(reader)); // work queued earlier may still read the old block
        svt_hip_buffer_release(b);
    }
    if (hipMalloc(&b->ptr, need) != hipSuccess) {
        b->ptr = nullptr;
        return svt_hip_fail(ctx, SVT_HIP_ERR_NO_MEMORY, failed_fmt, need);
    }
    b->bytes = need;
    return SVT_HIP_OK;
}

void svt_hip_buffer_release(SvtHipBuffer *b) {
    if (b->ptr) (void)hipFree(b->ptr); // nothing to do about a block the runtime will not take back
    b->ptr   = nullptr;
    b->bytes = 0;
}

int svt_hip_scratch(SvtHipContext *ctx, SvtHipLane *l, size_t bytes, void **out) {
    if (int rc = svt_hip_buffer_reserve(ctx, &l->scratch, bytes, l->stream, "hipMalloc(%zu) failed")) return rc;
    *out = l->scratch.ptr;
    return SVT_HIP_OK;
}

// ---- lanes -----------------------------------------------------------------------------------------------------------
int svt_hip_lane_setup(SvtHipContext *ctx, SvtHipLane *l, bool make_stream) {
    if (l->ready) return SVT_HIP_OK;
    // a set-up that failed part-way is retried by the lane's next holder: only the objects that do not exist yet are made
    if (make_stream && !l->stream) SVT_HIP_CHECK(ctx, hipStreamCreateWithFlags(&l->stream, hipStreamNonBlocking));
    if (!l->queue_head) {
        if (hipMalloc(reinterpret_cast<void **>(&l->queue_head), SVT_HIP_ME_QUEUE_BLOCK_BYTES) != hipSuccess) return svt_hip_fail(ctx, SVT_HIP_ERR_NO_MEMORY, "lane set-up: hipMalloc failed");
        if (hipMemset(l->queue_head, 0, SVT_HIP_ME_QUEUE_BLOCK_BYTES) != hipSuccess) {
            (void)hipFree(l->queue_head); // the memset's failure is the one reported
            l->queue_head = nullptr;
            return svt_hip_fail(ctx, SVT_HIP_ERR_NO_MEMORY, "lane set-up: hipMemset failed");
        }
    }
    if (!l->params_dev && hipMalloc(reinterpret_cast<void **>(&l->params_dev), SVT_HIP_ME_PARAM_BYTES) != hipSuccess)
        return svt_hip_fail(ctx, SVT_HIP_ERR_NO_MEMORY, "lane set-up: hipMalloc failed");
    for (int k = 0; k < SVT_HIP_PARAM_RING; k++) {
        if (!l->params_host[k] && hipHostMalloc(reinterpret_cast<void **>(&l->params_host[k]), SVT_HIP_ME_PARAM_BYTES, hipHostMallocDefault) != hipSuccess)
            return svt_hip_fail(ctx, SVT_HIP_ERR_NO_MEMORY, "lane set-up: hipHostMalloc failed");
        if (!l->params_copied[k]) SVT_HIP_CHECK(ctx, hipEventCreateWithFlags(&l->params_copied[k], hipEventDisableTiming));
    }
    l->ring_next = 0;
    l->ready     = true;
    return SVT_HIP_OK;
}

SvtHipLaneGuard::SvtHipLaneGuard(SvtHipContext *ctx) : ctx_(ctx), lane_(nullptr), index_(-1) {
    std::unique_lock<std::mutex> lk(ctx->pool_mu);
    ctx->pool_cv.wait(lk, [&] { return ctx->lane_busy != (1u << SVT_HIP_LANES) - 1u; });
    for (int i = 1; i < SVT_HIP_LANES; i++)
        if (!(ctx->lane_busy & (1u << i))) { index_ = i; break; }
    ctx->lane_busy |= 1u << index_;
    lk.unlock();
    // only the holder touches a borrowed lane, so its one-time set-up needs no lock
    if (svt_hip_use_device(ctx) == SVT_HIP_OK && svt_hip_lane_setup(ctx, &ctx->lane[index_], true) == SVT_HIP_OK) lane_ = &ctx->lane[index_];
}

SvtHipLaneGuard::~SvtHipLaneGuard() {
    // A holder that leaves early (an error return between two enqueues) may leave work queued on the lane's stream: the next holder must not
    // reuse -- or grow, i.e. free -- the lane's buffers under it.  After a normal call the stream is already idle and this returns at once.
    // A destructor has nobody to report a failure to.
    if (lane_ && lane_->stream) (void)hipStreamSynchronize(lane_->stream);
    {
        std::lock_guard<std::mutex> lk(ctx_->pool_mu);
        ctx_->lane_busy &= ~(1u << index_);
    }
    ctx_->pool_cv.notify_one();
}

int svt_hip_wait_picture(SvtHipContext *ctx, hipStream_t stream, const SvtHipPaPicture *pic) {
    if (pic && pic->ready && pic->ready_stream != stream) SVT_HIP_CHECK(ctx, hipStreamWaitEvent(stream, pic->ready, 0));
    return SVT_HIP_OK;
}

// ---- transfer stream -------------------------------------------------------------------------------------------------
int svt_hip_transfer_stream_make(SvtHipContext *ctx) {
    if (!ctx->io_stream) SVT_HIP_CHECK(ctx, hipStreamCreateWithFlags(&ctx->io_stream, hipStreamNonBlocking));
    if (!ctx->io_fence) SVT_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->io_fence, hipEventDisableTiming));
    return SVT_HIP_OK;
}

// ---- the context -----------------------------------------------------------------------------------------------------
extern "C" {

int svt_hip_context_create(SvtHipContext **out, int device) {
    if (!out) return SVT_HIP_ERR_BAD_PARAM;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return SVT_HIP_ERR_NO_DEVICE;
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return SVT_HIP_ERR_NO_DEVICE;
    if (device >= n) return SVT_HIP_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return SVT_HIP_ERR_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return SVT_HIP_ERR_NO_DEVICE; // code objects are gfx950 only
    if (hipSetDevice(device) != hipSuccess) return SVT_HIP_ERR_NO_DEVICE;
    SvtHipContext *ctx = new (std::nothrow) SvtHipContext();
    if (!ctx) return SVT_HIP_ERR_NO_MEMORY;
    ctx->device  = device;
    ctx->num_cus = prop.multiProcessorCount;
    { const char *e = getenv("SVT_HIP_ME_DENSE"); ctx->me_dense = !(e && e[0] == '0'); }
    { const char *e = getenv("SVT_HIP_ME_DENSE_FAST"); ctx->me_dense_fast = !(e && e[0] == '0'); }
    { const char *e = getenv("SVT_HIP_ME_STAGED"); ctx->me_staged = (e && e[0] >= '0' && e[0] <= '2') ? e[0] - '0' : 1; }
    // lane 0 (the asynchronous entries' stream) and this device's transform tables exist from the start; the borrowed
    // lanes are made when a synchronous entry first needs one
    if (svt_hip_lane_setup(ctx, &ctx->lane[0], true) != SVT_HIP_OK || svt_hip_rd_tables_init(ctx) != SVT_HIP_OK ||
        svt_hip_tpl_tables_init(ctx) != SVT_HIP_OK) {
        svt_hip_context_destroy(ctx);
        return SVT_HIP_ERR_NO_DEVICE;
    }
    ctx->stream    = ctx->lane[0].stream;
    ctx->lane_busy = 1u; // lane 0 is never borrowed
    *out = ctx;
    return SVT_HIP_OK;
}

// Teardown cannot act on a failure of the runtime: every result below is dropped on purpose.
void svt_hip_context_destroy(SvtHipContext *ctx) {
    if (!ctx) return;
    svt_hip_leaf_unbind(ctx); // from here on the pointer-level entries find no context and go to the previous kernels
    (void)hipSetDevice(ctx->device);
    for (int i = 0; i < SVT_HIP_LANES; i++) {
        SvtHipLane &l = ctx->lane[i];
        if (l.stream) (void)hipStreamSynchronize(l.stream);
        for (SvtHipBuffer *b : {&l.scratch, &l.dense, &l.stage}) svt_hip_buffer_release(b);
        for (hipEvent_t &e : l.me_mark) if (e) (void)hipEventDestroy(e);
        if (l.queue_head) (void)hipFree(l.queue_head);
        if (l.params_dev) (void)hipFree(l.params_dev);
        for (int k = 0; k < SVT_HIP_PARAM_RING; k++) {
            if (l.params_host[k]) (void)hipHostFree(l.params_host[k]);
            if (l.params_copied[k]) (void)hipEventDestroy(l.params_copied[k]);
        }
        if (l.stream) (void)hipStreamDestroy(l.stream);
    }
    if (ctx->io_stream) { (void)hipStreamSynchronize(ctx->io_stream); (void)hipStreamDestroy(ctx->io_stream); }
    if (ctx->io_fence) (void)hipEventDestroy(ctx->io_fence);
    svt_hip_rd_tables_free(ctx);
    svt_hip_tpl_free(ctx);
    delete ctx;
}

const char *svt_hip_last_error(const SvtHipContext *) { return svt_hip_err_buf(); }
void       *svt_hip_context_stream(SvtHipContext *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

int svt_hip_context_sync(SvtHipContext *ctx) {
    if (!ctx) return SVT_HIP_ERR_BAD_PARAM;
    SVT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->io_stream) SVT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->io_stream));
    return SVT_HIP_OK;
}

void *svt_hip_context_transfer_stream(SvtHipContext *ctx) {
    if (!ctx) return nullptr;
    std::lock_guard<std::mutex> lock(ctx->async_mu);
    if (svt_hip_use_device(ctx) != SVT_HIP_OK || svt_hip_transfer_stream_make(ctx) != SVT_HIP_OK) return nullptr;
    return (void *)ctx->io_stream;
}

} // extern "C"
