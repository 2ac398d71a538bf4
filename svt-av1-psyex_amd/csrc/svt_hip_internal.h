// svt_hip_internal.h -- private host-side declarations of libsvthip.so
#ifndef SVT_HIP_INTERNAL_H
#define SVT_HIP_INTERNAL_H
#include <hip/hip_runtime_api.h>
#include <stdarg.h>
#include <stdio.h>
#include <condition_variable>
#include <mutex>
#include "me_kernel.h"

// Threading model (the reference calls the kernels from several ME / mode-decision threads with several pictures in
// flight: Globals/enc_handle.c:2265,2293, Codec/me_process.c:140-172):
//   * a LANE owns everything one host call in flight needs on the device: a stream, the ME job-queue counters, the ME
//     parameter block (a ring of pinned host copies + one device copy) and grow-on-demand buffers (SvtHipBuffer);
//   * lane 0 belongs to the asynchronous entries (they enqueue on svt_hip_context_stream(), whose order the caller
//     owns); its enqueues are serialised by `async_mu`;
//   * every synchronous (host-pointer) entry borrows one of the other lanes for the duration of the call, so calls
//     from different host threads neither share result memory nor wait for each other's kernels.
#define SVT_HIP_LANES 9       /* lane 0 + 8 borrowed lanes (more callers than that wait for a free lane) */
#define SVT_HIP_PARAM_RING 4  /* ME launches that may be enqueued ahead on one lane before the host waits */

// A device block that grows on demand and never shrinks (svt_hip_buffer_reserve / svt_hip_buffer_release, context.cpp)
struct SvtHipBuffer {
    void  *ptr;
    size_t bytes;
};

struct SvtHipLane {
    hipStream_t stream;
    uint32_t   *queue_head;  // SVT_HIP_ME_QUEUE_BLOCK_BYTES: job-queue counters of the ME kernels, the profiling build's phase sums, list cursors (me_kernel.h)
    uint8_t    *params_dev;  // MeBatchHeader (SVT_HIP_ME_HEADER_BYTES) + MeKernelParams[SVT_HIP_ME_MAX_PICTURES]
    uint8_t    *params_host[SVT_HIP_PARAM_RING];   // pinned staging copies of the same block
    hipEvent_t  params_copied[SVT_HIP_PARAM_RING]; // recorded behind the H2D copy that reads params_host[i]
    int         ring_next;
    SvtHipBuffer scratch;    // result buffer of the synchronous entries (only touched by the lane's holder)
    SvtHipBuffer dense;      // slots of the ME dense pre-pass (me_dense.inl)
    size_t      dense_used;  // bytes of `dense` the lane's last launch with a pre-pass filled, and that launch's number in the context (svt_hip_me_dense_slots)
    unsigned long long dense_seq;
    SvtHipBuffer stage;      // staged ME launches: the blocks' travelling records, flag words and the three job lists
    hipEvent_t  me_mark[SVT_HIP_ME_CHAIN_KERNELS + 1]; // svt_hip_context_set_me_timing: events around the kernels of the last ME launch (created on first use)
    uint32_t    me_marked;   // bit i: kernel i of the chain ran in the last launch and both events around it were recorded (me_mark[i] .. the next recorded one)
    bool        ready;       // device objects exist (lanes are set up on first use)
};

struct SvtHipContext {
    int         device;
    int         num_cus;
    // lanes and pool (context.cpp)
    hipStream_t stream; // == lane[0].stream
    SvtHipLane  lane[SVT_HIP_LANES];
    std::mutex  async_mu;              // serialises enqueues through lane 0
    std::mutex  pool_mu;               // guards lane_busy / lane set-up
    std::condition_variable pool_cv;
    uint32_t    lane_busy;             // bit i: lane i is borrowed
    // ME switches (me_switches.cpp; svt_hip_me_launch reads them)
    bool        me_attr_set;           // hipFuncSetAttribute done for the ME kernel on this device
    int         me_staged;             // with a pre-pass, the per-block pipeline runs as a chain of small kernels: 0 never, 1 launches of many blocks, 2 always (svt_hip_context_set_me_staged)
    bool        me_counting;           // ME waves report what they took from the dense pre-pass (svt_hip_context_set_me_counting)
    bool        me_timing;             // ME launches record events around their kernels (svt_hip_context_set_me_timing)
    bool        me_dense;              // the dense pre-HME / level-0 pre-pass runs ahead of the per-block ME kernel (svt_hip_context_set_me_dense)
    bool        me_dense_fast;         // the pre-pass takes its static walk where a unit allows it (svt_hip_context_set_me_dense_fast)
    int         me_dense_plan;         // 0: the pre-pass's units are sized by the launch; 1 .. 3: long / middle / fine units (svt_hip_context_set_me_dense_plan)
    unsigned long long me_dense_seq;   // launches with a pre-pass so far
    uint32_t    me_waves_per_cu;       // 0: as many persistent ME waves per CU as fit; else an upper limit (svt_hip_context_set_me_waves_per_cu)
    uint32_t    me_max_waves;          // 0: no limit; else the most persistent waves an ME kernel is launched with (svt_hip_context_set_me_max_waves)
    // transfer stream (context.cpp: svt_hip_transfer_stream_make)
    hipStream_t io_stream;             // transfer stream of svt_hip_pa_picture_update_ahead (created on first use)
    hipEvent_t  io_fence;              // orders the transfer stream behind the context stream
    // RD tables (rd_kernel.hip) and the rate / RDOQ batches' switch
    int16_t    *iscan_dev;             // [19][3][1024] inverse scan orders, this device's copy
    uint32_t    lvmap_max_grid;        // 0: the rate / RDOQ batches launch at most 2048 workgroups; else that many (svt_hip_context_set_lvmap_max_grid)
    // TPL (tpl_kernel.hip, tpl_synth_kernel.hip)
    SvtHipBuffer tpl_scratch;          // per-block state of svt_hip_tpl_dispense, used in stream order on the context stream
    void       *tpl_group_dev;         // svt_hip_tpl_group's frame tables: SVT_HIP_TPL_GROUP_RING slots on the device
    void       *tpl_group_host;        // their pinned staging copies
    hipEvent_t  tpl_group_done[4];     // recorded behind the last launch that reads slot i (SVT_HIP_TPL_GROUP_RING)
    int         tpl_group_next;
};

struct SvtHipPaPicture {
    DevPyramid  pyr;
    void       *mem[3];
    size_t      bytes[3];
    hipEvent_t  ready;        // recorded behind the uploads / decimation kernels that fill the planes
    hipStream_t ready_stream; // the stream that work was enqueued on: other streams wait for `ready` before reading
};

// The last error message of the CALLING thread (svt_hip_last_error, context.cpp): contexts are shared between threads
char *svt_hip_err_buf(void);
#define SVT_HIP_ERR_BYTES 512

static inline int svt_hip_fail(SvtHipContext *, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(svt_hip_err_buf(), SVT_HIP_ERR_BYTES, fmt, ap);
    va_end(ap);
    return code;
}

#define SVT_HIP_CHECK(ctx, call)                                                                                  \
    do {                                                                                                          \
        hipError_t e_ = (call);                                                                                   \
        if (e_ != hipSuccess)                                                                                     \
            return svt_hip_fail(ctx, SVT_HIP_ERR_LAUNCH, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                                __FILE__, __LINE__);                                                              \
    } while (0)

// Internal functions that stay out of the library's dynamic symbol table
#define SVT_HIP_HIDDEN __attribute__((visibility("hidden")))

// context.cpp
// Makes the context's device the calling thread's current one; every entry that touches the runtime starts with it
SVT_HIP_HIDDEN int svt_hip_use_device(SvtHipContext *ctx);
// Borrow / return a lane for a synchronous entry (RAII).  lane() is null when the lane's device objects could not be made.
class SvtHipLaneGuard {
public:
    explicit SvtHipLaneGuard(SvtHipContext *ctx);
    ~SvtHipLaneGuard();
    SvtHipLane *lane() const { return lane_; }
private:
    SvtHipContext *ctx_;
    SvtHipLane    *lane_;
    int            index_;
};
int svt_hip_lane_setup(SvtHipContext *ctx, SvtHipLane *l, bool make_stream);
// makes `stream` wait for the work that fills `pic` when that was enqueued on another stream
int svt_hip_wait_picture(SvtHipContext *ctx, hipStream_t stream, const SvtHipPaPicture *pic);
// The buffer rule.  Nothing to do when `need` <= b->bytes.  Otherwise `reader`, the one stream whose queued work may still read the old block, is
// synchronised, the block is freed and a new one of `need` bytes allocated; on failure the buffer is left empty and the result is
// SVT_HIP_ERR_NO_MEMORY, its text `failed_fmt`, the caller's wording with one %zu for `need`.  The caller is the buffer's only user at that
// moment: a borrowed lane's holder; for lane 0's dense / stage and tpl_scratch whoever holds async_mu; for lane 0's scratch the pointer-level
// entry that holds leaf_mutex.
SVT_HIP_HIDDEN int  svt_hip_buffer_reserve(SvtHipContext *ctx, SvtHipBuffer *b, size_t need, hipStream_t reader, const char *failed_fmt);
// Frees the block and leaves the buffer empty.  The caller has synchronised every stream that used it: svt_hip_buffer_reserve when it grows,
// and teardown.
SVT_HIP_HIDDEN void svt_hip_buffer_release(SvtHipBuffer *b);
// the lane's result buffer, at least `bytes` long
int    svt_hip_scratch(SvtHipContext *ctx, SvtHipLane *lane, size_t bytes, void **out);
// The transfer stream and the fence that orders it behind the context stream, made on first use with ctx->async_mu HELD by the caller.  A call
// that made only one of the two fails; the next call makes the other.
SVT_HIP_HIDDEN int svt_hip_transfer_stream_make(SvtHipContext *ctx);

// leaf_runtime.cpp: the pointer-level entries stop using `ctx` (svt_hip_context_destroy)
SVT_HIP_HIDDEN void svt_hip_leaf_unbind(SvtHipContext *ctx);

// me_kernel.hip
size_t svt_hip_me_kernel_lds_bytes(void);
int    svt_hip_me_launch(SvtHipContext *ctx, SvtHipLane *lane, const MeKernelParams *params, const uint32_t *n_jobs, uint32_t n_pictures);
// me_picture.hip: the asynchronous ME entry on an explicit lane
int    svt_hip_me_pictures_on_lane(SvtHipContext *ctx, SvtHipLane *lane, uint32_t n_pictures, const SvtHipMeJob *jobs);
// stats_kernel.hip: launches hadamard_kernel for the pointer-level Hadamard entries (not exported)
SVT_HIP_HIDDEN hipError_t svt_hip_hadamard_launch(SvtHipContext *ctx, const int16_t *src, int stride, int n, int32_t *coeff);
// rd_kernel.hip: cosine / inverse-scan tables of the context's device
int    svt_hip_rd_tables_init(SvtHipContext *ctx);
void   svt_hip_rd_tables_free(SvtHipContext *ctx);
// tpl_kernel.hip: its copy of the cosine table; the dispenser's scratch
int    svt_hip_tpl_tables_init(SvtHipContext *ctx);
void   svt_hip_tpl_free(SvtHipContext *ctx);
// the dispenser's launches for a descriptor svt_hip_tpl_check_desc accepted, with ctx->async_mu HELD by the caller
struct SvtHipTplDesc;
int    svt_hip_tpl_dispense_locked(SvtHipContext *ctx, const SvtHipTplDesc *d);
// tpl_synth_kernel.hip: the group entry's frame tables
#define SVT_HIP_TPL_GROUP_RING 4
void   svt_hip_tpl_group_free(SvtHipContext *ctx);
#endif
