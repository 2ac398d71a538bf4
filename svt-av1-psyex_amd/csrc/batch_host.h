// batch_host.h -- the host side that the asynchronous batch entries share: the enqueue sequence of a batch entry (the
// ten files of inter, intra, CfL, warp, masked compound / inter-intra, OBMC, the interpolation-filter search, palette, global motion and CDEF;
// RD and the transforms alone, the MD searches, PME, statistics, SSIM, rate, RDOQ), and for the first eight the refusal
// macro of their *_check_desc functions, the validation of an SvtHipInterPredRef array and the lookup behind every
// *_layout entry.  A new batch entry supplies a check, a count and a launch; the order of the steps is here.
#ifndef SVT_HIP_BATCH_HOST_H
#define SVT_HIP_BATCH_HOST_H
#include <stddef.h>
#include "svt_hip_internal.h"
#include "../../include/svt_hip_pred.h"

#define BAD(...) return svt_hip_fail(nullptr, SVT_HIP_ERR_BAD_PARAM, __VA_ARGS__)

// The n_refs range and every reference plane of a descriptor that carries SvtHipInterPredRef refs[]; `who` is the
// *_check_desc that asks.
static inline int svt_hip_check_inter_pred_refs(const char *who, const SvtHipInterPredRef *refs, unsigned n_refs) {
    if (n_refs == 0 || n_refs > SVT_HIP_INTER_PRED_MAX_REFS) BAD("%s: %u reference planes (1..%d)", who, n_refs, SVT_HIP_INTER_PRED_MAX_REFS);
    for (unsigned i = 0; i < n_refs; i++) {
        const SvtHipInterPredRef *r = &refs[i];
        if (!r->plane) BAD("%s: reference %u: null plane", who, i);
        if (r->stride == 0 || r->width == 0 || r->height == 0 || r->stride < r->width)
            BAD("%s: reference %u: stride %u, padded size %u x %u (stride and size non-zero, stride >= width)", who, i, r->stride, r->width, r->height);
        if (r->org_x >= r->width || r->org_y >= r->height)
            BAD("%s: reference %u: origin (%u, %u) outside the padded plane %u x %u", who, i, r->org_x, r->org_y, r->width, r->height);
    }
    return SVT_HIP_OK;
}

// One struct of a *_layout entry: its size and the offsets of its fields, in the order of the header it mirrors.
struct SvtHipLayoutRow {
    size_t        size;
    const size_t *offset;
    size_t        n;
};
template <class T, size_t N> constexpr SvtHipLayoutRow layout_row(const size_t (&offset)[N]) { return {sizeof(T), offset, N}; }

// svt_hip_*_layout(what, field): the size of struct `what` for field < 0, else the offset of its field; (size_t)-1 past
// the last field and for a `what` outside the rows.
template <size_t N> size_t layout_lookup(const SvtHipLayoutRow (&rows)[N], int what, int field) {
    if (what < 0 || (size_t)what >= N) return (size_t)-1;
    if (field < 0) return rows[what].size;
    return (size_t)field < rows[what].n ? rows[what].offset[field] : (size_t)-1;
}

static inline uint32_t ceil_div(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

// The 10-bit or the 8-bit instantiation of a kernel template: pick_hbd(d->bit_depth, kernel<true>, kernel<false>)
template <class Kernel> Kernel pick_hbd(unsigned bit_depth, Kernel hbd, Kernel lbd) { return bit_depth == 10 ? hbd : lbd; }

// The enqueue itself, on ctx->stream under ctx->async_mu, with one question to the runtime behind all of `launch`'s
// hipLaunchKernelGGL calls.  An entry that takes an argument list, not a descriptor, calls this after its own checks.
template <class Launch> int enqueue_locked(const char *entry, SvtHipContext *ctx, Launch launch) {
    if (int rc = svt_hip_use_device(ctx)) return rc;
    std::lock_guard<std::mutex> lock(ctx->async_mu);
    launch();
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return svt_hip_fail(ctx, SVT_HIP_ERR_LAUNCH, "%s: the launch failed: %s", entry, hipGetErrorString(e));
    return SVT_HIP_OK;
}

// An asynchronous batch entry: refuses null arguments and what `check` refuses, returns for an empty batch before it
// touches the context, then enqueues.  `count` (and `count2`: both zero) is the descriptor's member that says how much
// there is to do; `launch` holds the entry's hipLaunchKernelGGL calls and its grid arithmetic.
template <class Desc, class Check, class Launch>
int enqueue_batch(const char *entry, SvtHipContext *ctx, const Desc *d, Check check, uint32_t Desc::*count, uint32_t Desc::*count2, Launch launch) {
    if (!ctx || !d) BAD("%s: null context or descriptor", entry);
    const int rc = check(d);
    if (rc) return rc;
    if (d->*count == 0 && d->*count2 == 0) return SVT_HIP_OK;
    return enqueue_locked(entry, ctx, launch);
}
template <class Desc, class Check, class Launch>
int enqueue_batch(const char *entry, SvtHipContext *ctx, const Desc *d, Check check, uint32_t Desc::*count, Launch launch) {
    return enqueue_batch(entry, ctx, d, check, count, count, launch);
}
#endif
