// me_switches.cpp -- the context's ME switches and diagnostics (include/svt_hip_me.h), host code only: what svt_hip_me_launch (me_kernel.hip)
// reads from the context, and what its kernels leave in the lanes' queue_head blocks (me_kernel.h) read back.
#include <hip/hip_runtime_api.h>
#include <string.h>
#include "svt_hip_internal.h"

namespace {

const char *const kChainKernelNames[SVT_HIP_ME_CHAIN_KERNELS] = {"svt_hip_me_dense_kernel", "svt_hip_me_mid1_kernel", "svt_hip_me_s1_kernel",  "svt_hip_me_mid2_kernel",
                                                                 "svt_hip_me_s2_kernel",    "svt_hip_me_tail_kernel", "svt_hip_me_b64_kernel"};

// `count` u64 counters from u32 index `word` of the lanes' queue_head blocks: waits for each ready lane's stream, copies, clears, adds
constexpr int kMostCounters = SVT_HIP_ME_PROFILE_SUMS;
static_assert(SVT_HIP_ME_DENSE_PATH_COUNTERS <= kMostCounters, "counters");
int read_lane_counters(SvtHipContext *ctx, int word, int count, unsigned long long *out) {
    if (!ctx || !out) return SVT_HIP_ERR_BAD_PARAM;
    memset(out, 0, count * sizeof(out[0]));
    if (int rc = svt_hip_use_device(ctx)) return rc;
    for (int i = 0; i < SVT_HIP_LANES; i++) {
        SvtHipLane &l = ctx->lane[i];
        if (!l.ready) continue;
        unsigned long long v[kMostCounters];
        SVT_HIP_CHECK(ctx, hipStreamSynchronize(l.stream));
        SVT_HIP_CHECK(ctx, hipMemcpy(v, l.queue_head + word, count * sizeof(v[0]), hipMemcpyDeviceToHost));
        SVT_HIP_CHECK(ctx, hipMemset(l.queue_head + word, 0, count * sizeof(v[0])));
        for (int k = 0; k < count; k++) out[k] += v[k];
    }
    return SVT_HIP_OK;
}

} // namespace

extern "C" {

const char *svt_hip_me_chain_kernel_name(int i) { return i >= 0 && i < SVT_HIP_ME_CHAIN_KERNELS ? kChainKernelNames[i] : nullptr; }

int svt_hip_context_set_me_counting(SvtHipContext *ctx, int on) {
    if (!ctx) return SVT_HIP_ERR_BAD_PARAM;
    ctx->me_counting = on != 0;
    return SVT_HIP_OK;
}

int svt_hip_context_set_me_timing(SvtHipContext *ctx, int on) {
    if (!ctx) return SVT_HIP_ERR_BAD_PARAM;
    ctx->me_timing = on != 0;
    return SVT_HIP_OK;
}

// The kernels of the last launch enqueued through lane 0 (the context stream).  For measurement from ONE thread: with several threads
// enqueueing, "the last launch" is whichever took async_mu last.  The lock only keeps a launch on another thread from rewriting the lane's
// events while they are read.
int svt_hip_me_launch_times(SvtHipContext *ctx, float ms[SVT_HIP_ME_CHAIN_KERNELS]) {
    if (!ctx || !ms) return SVT_HIP_ERR_BAD_PARAM;
    SvtHipLane &l = ctx->lane[0];
    if (int rc = svt_hip_use_device(ctx)) return rc;
    std::lock_guard<std::mutex> lock(ctx->async_mu);
    SVT_HIP_CHECK(ctx, hipStreamSynchronize(l.stream));
    for (int i = 0; i < SVT_HIP_ME_CHAIN_KERNELS; i++) {
        ms[i] = 0.f;
        if (!(l.me_marked >> i & 1u)) continue;
        // the event behind kernel i is the next one recorded: the one in front of the next kernel that ran, or the closing event
        int j = i + 1;
        while (j < SVT_HIP_ME_CHAIN_KERNELS && !(l.me_marked >> j & 1u)) j++;
        SVT_HIP_CHECK(ctx, hipEventElapsedTime(&ms[i], l.me_mark[i], l.me_mark[j]));
    }
    return SVT_HIP_OK;
}

int svt_hip_context_set_me_staged(SvtHipContext *ctx, int on) {
    if (!ctx) return SVT_HIP_ERR_BAD_PARAM;
    if (on < 0 || on > 2) return svt_hip_fail(ctx, SVT_HIP_ERR_BAD_PARAM, "svt_hip_context_set_me_staged: %d is not 0 (off), 1 (large launches) or 2 (every launch)", on);
    ctx->me_staged = on;
    return SVT_HIP_OK;
}

int svt_hip_context_set_me_dense(SvtHipContext *ctx, int on) {
    if (!ctx) return SVT_HIP_ERR_BAD_PARAM;
    ctx->me_dense = on != 0;
    return SVT_HIP_OK;
}

int svt_hip_context_set_me_dense_fast(SvtHipContext *ctx, int on) {
    if (!ctx) return SVT_HIP_ERR_BAD_PARAM;
    ctx->me_dense_fast = on != 0;
    return SVT_HIP_OK;
}

int svt_hip_context_set_me_dense_plan(SvtHipContext *ctx, int plan) {
    if (!ctx) return SVT_HIP_ERR_BAD_PARAM;
    if (plan < 0 || plan > 3) return svt_hip_fail(ctx, SVT_HIP_ERR_BAD_PARAM, "svt_hip_context_set_me_dense_plan: %d is not 0 (by launch size), 1 (long units), 2 or 3 (fine units)", plan);
    ctx->me_dense_plan = plan;
    return SVT_HIP_OK;
}

int svt_hip_context_set_me_waves_per_cu(SvtHipContext *ctx, uint32_t waves) {
    if (!ctx) return SVT_HIP_ERR_BAD_PARAM;
    ctx->me_waves_per_cu = waves;
    return SVT_HIP_OK;
}

int svt_hip_context_set_me_max_waves(SvtHipContext *ctx, uint32_t waves) {
    if (!ctx) return SVT_HIP_ERR_BAD_PARAM;
    ctx->me_max_waves = waves;
    return SVT_HIP_OK;
}

// Diagnostics: searches the per-block kernel took from the dense pre-pass / pushed searches it found no slot for, summed over the lanes
// since the last call (the call waits for the lanes' streams).
int svt_hip_me_dense_counters(SvtHipContext *ctx, unsigned long long out[2]) { return read_lane_counters(ctx, SVT_HIP_ME_COUNTER_WORD, 2, out); }

// Diagnostics: the units of the pre-pass by the walk they took, and the (source row, search row) pairs of their waves, since the last call
int svt_hip_me_dense_path_counters(SvtHipContext *ctx, unsigned long long out[2 * SVT_HIP_ME_DENSE_PATHS + 7]) {
    return read_lane_counters(ctx, SVT_HIP_ME_DENSE_PATH_WORD, SVT_HIP_ME_DENSE_PATH_COUNTERS, out);
}

// Diagnostic: per-phase shader-clock sums of the ME kernel (non-zero only in a -DSVT_HIP_ME_PROFILE build), summed over the
// lanes; clears them.
int svt_hip_me_profile_read(SvtHipContext *ctx, unsigned long long out[SVT_HIP_ME_PROFILE_SUMS]) {
    return read_lane_counters(ctx, SVT_HIP_ME_PROFILE_WORD, SVT_HIP_ME_PROFILE_SUMS, out);
}

// Diagnostics: the slot buffer of the context's most recent launch with a pre-pass (waits for that launch).  *bytes = its size; the slots are
// copied when they fit `capacity`.
int svt_hip_me_dense_slots(SvtHipContext *ctx, void *out, size_t capacity, size_t *bytes) {
    if (!ctx || !bytes) return SVT_HIP_ERR_BAD_PARAM;
    *bytes = 0;
    if (int rc = svt_hip_use_device(ctx)) return rc;
    const SvtHipLane *last = nullptr;
    for (int i = 0; i < SVT_HIP_LANES; i++)
        if (ctx->lane[i].ready && ctx->lane[i].dense_seq && (!last || ctx->lane[i].dense_seq > last->dense_seq)) last = &ctx->lane[i];
    if (!last) return SVT_HIP_OK;
    *bytes = last->dense_used;
    if (!out || capacity < last->dense_used) return SVT_HIP_OK;
    SVT_HIP_CHECK(ctx, hipStreamSynchronize(last->stream));
    SVT_HIP_CHECK(ctx, hipMemcpy(out, last->dense.ptr, last->dense_used, hipMemcpyDeviceToHost));
    return SVT_HIP_OK;
}

} // extern "C"
