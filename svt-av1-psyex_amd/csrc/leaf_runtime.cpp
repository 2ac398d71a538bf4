// leaf_runtime.cpp -- the process-global runtime of the pointer-level `_hip` entries (include/svt_hip_leaf.h), host code only: the bound context and
// the entries' common lock, the installer that writes this library's entries into the encoder's function pointers and keeps what they held
// before, the failure counters, and the bodies of the helpers leaf_guard.h declares.  The entries themselves sit next to their kernels
// (leaf_kernels.hip, rd_kernel.hip, pme_kernel.hip, ssim_kernel.hip).
#include <dlfcn.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <atomic>
#include <mutex>
#include "svt_hip_internal.h"
#include "leaf_guard.h"
#include "../../include/svt_hip_leaf.h"

namespace {

// ---- process-global state of the pointer-level entries -----------------------------------------------------------
SvtHipContext *g_leaf_ctx = nullptr;
std::mutex     g_leaf_mutex; // the reference calls its kernels from many threads; these entries serialise on one stream
// previous kernels of the slots svt_hip_install_rtcd wrote to, by this library's symbol name
struct LeafPrev { char symbol[96]; void *prev; void **slot; void *entry; }; // entry: what the installer wrote to *slot
LeafPrev   g_leaf_prev[640];
int        g_leaf_nprev = 0;
std::mutex g_leaf_prev_mutex;
std::atomic<unsigned long long> g_leaf_fallbacks{0}, g_leaf_unhandled{0};
std::atomic<int>                g_leaf_inject{0};
char       g_leaf_msg[SVT_HIP_ERR_BYTES] = "";
thread_local int t_leaf_depth = 0;

} // namespace

// (leaf_guard.h) the helpers of the pointer-level entries: failures throw, the entry's handler hands the call to the previous kernel
[[noreturn]] void leaf_fail(const char *fmt, ...) {
    LeafFailure f;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(f.what, sizeof(f.what), fmt, ap);
    va_end(ap);
    throw f;
}
SvtHipContext *leaf_ctx() {
    if (g_leaf_inject.load()) leaf_fail("injected failure (svt_hip_leaf_inject_failure)");
    if (!g_leaf_ctx) leaf_fail("a _hip leaf kernel was called with no context bound (svt_hip_leaf_bind / svt_hip_install_rtcd)");
    leaf_check(g_leaf_ctx, hipSetDevice(g_leaf_ctx->device), "hipSetDevice"); // what svt_hip_use_device does for the entries that return a code
    return g_leaf_ctx;
}
void leaf_check(SvtHipContext *, hipError_t e, const char *what) {
    if (e != hipSuccess) leaf_fail("%s failed in a _hip leaf kernel: %s", what, hipGetErrorString(e));
}
// device staging area: [0, bytes) carved by the caller.  The pointer-level entries run one at a time (leaf_mutex) on the context
// stream; lane 0's result buffer is theirs alone (the asynchronous entries use none, the synchronous ones borrow other lanes).
uint8_t *leaf_scratch(SvtHipContext *ctx, size_t bytes) {
    void *pp = nullptr;
    if (svt_hip_scratch(ctx, &ctx->lane[0], bytes, &pp) != SVT_HIP_OK) leaf_fail("out of device memory in a _hip leaf kernel (%zu bytes)", bytes);
    return static_cast<uint8_t *>(pp);
}
std::mutex &leaf_mutex() { return g_leaf_mutex; }
int         leaf_depth() { return t_leaf_depth; }
LeafEnter::LeafEnter() { t_leaf_depth++; }
LeafEnter::~LeafEnter() { t_leaf_depth--; }
const void *leaf_previous(const char *symbol) {
    std::lock_guard<std::mutex> lock(g_leaf_prev_mutex);
    for (int k = 0; k < g_leaf_nprev; k++)
        if (!strcmp(g_leaf_prev[k].symbol, symbol)) return g_leaf_prev[k].prev;
    return nullptr;
}
static void leaf_note(const char *symbol, const LeafFailure &f, const char *how) {
    std::lock_guard<std::mutex> lock(g_leaf_prev_mutex);
    snprintf(g_leaf_msg, sizeof(g_leaf_msg), "%s: %s -- %s", symbol, f.what, how);
    snprintf(svt_hip_err_buf(), SVT_HIP_ERR_BYTES, "%s", g_leaf_msg); // svt_hip_last_error() of the calling thread
}
void leaf_note_fallback(const char *symbol, const LeafFailure &f) {
    g_leaf_fallbacks++;
    leaf_note(symbol, f, "the call went to the kernel the encoder had installed before");
}
void leaf_note_unhandled(const char *symbol, const LeafFailure &f) {
    g_leaf_unhandled++;
    leaf_note(symbol, f, "no previous kernel is known for this entry: nothing was computed");
    fprintf(stderr, "libsvthip: %s\n", g_leaf_msg);
}

extern "C" {

int svt_hip_leaf_bind(SvtHipContext *ctx) {
    std::lock_guard<std::mutex> lock(g_leaf_mutex);
    g_leaf_ctx = ctx;
    return SVT_HIP_OK;
}

} // extern "C"

// svt_hip_context_destroy: a context that goes away is bound no longer (the lock waits for an entry that is running on it)
void svt_hip_leaf_unbind(SvtHipContext *ctx) {
    std::lock_guard<std::mutex> lock(g_leaf_mutex);
    if (g_leaf_ctx == ctx) g_leaf_ctx = nullptr;
}

extern "C" {

// The `_hip` entry that takes the place of the reference's function pointer `name`: the exported symbol <name>_hip of this library
// (the pointer-level entries carry the reference's pointer names), or the one the short alias table names where the reference's
// pointer and its `_c` body are called differently.
static const void *rtcd_lookup_symbol(const char *name, char *sym, size_t sym_bytes) {
    static const struct { const char *pointer, *symbol; } alias[] = {
        {"svt_nxm_sad_kernel", "svt_nxm_sad_kernel_helper_hip"},          // aom_dsp_rtcd.h:125 -> svt_nxm_sad_kernel_helper_c
        {"svt_aom_quantize_b", "svt_aom_quantize_b_hip"},                 // -> svt_aom_quantize_b_c_ii
        {"svt_aom_sad_16b_kernel", "svt_aom_sad_16b_kernel_hip"},
    };
    if (!name || !*name || strlen(name) > 200) return nullptr;
    Dl_info info;
    if (!dladdr(reinterpret_cast<const void *>(&svt_hip_leaf_bind), &info) || !info.dli_fname) return nullptr;
    void *self = dlopen(info.dli_fname, RTLD_NOW | RTLD_NOLOAD);
    if (!self) return nullptr;
    snprintf(sym, sym_bytes, "%s_hip", name);
    for (const auto &a : alias)
        if (!strcmp(a.pointer, name)) snprintf(sym, sym_bytes, "%s", a.symbol);
    const void *fn = dlsym(self, sym);
    dlclose(self);
    return fn;
}
const void *svt_hip_rtcd_lookup(const char *name) {
    char sym[256];
    return rtcd_lookup_symbol(name, sym, sizeof(sym));
}

// Stores this library's entries into the slots and keeps what each slot held before -- the encoder's own kernel -- as the entry's way
// out: a `_hip` entry that cannot run (no bound context, a device error) calls it with the same arguments (leaf_guard.h).  No context is
// bound: until svt_hip_leaf_bind() every call goes to the previous kernels.
int svt_hip_rtcd_store(const SvtHipRtcdSlot *slots, uint32_t n_slots, uint32_t *n_skipped) {
    if (!slots && n_slots) return SVT_HIP_ERR_BAD_PARAM;
    uint32_t skipped = 0;
    for (uint32_t i = 0; i < n_slots; i++)
        if (!slots[i].slot) return svt_hip_fail(nullptr, SVT_HIP_ERR_BAD_PARAM, "rtcd slot %u (%s): null address", i, slots[i].name ? slots[i].name : "?");
    std::lock_guard<std::mutex> lock(g_leaf_prev_mutex);
    for (uint32_t i = 0; i < n_slots; i++) {
        char sym[256];
        const void *fn = rtcd_lookup_symbol(slots[i].name, sym, sizeof(sym));
        if (!fn) { skipped++; continue; }
        void *prev = *slots[i].slot;
        if (prev == fn) continue; // installed already: keep the previous kernel recorded then
        int k = 0;
        while (k < g_leaf_nprev && strcmp(g_leaf_prev[k].symbol, sym)) k++;
        if (k == g_leaf_nprev) {
            if (g_leaf_nprev == (int)(sizeof(g_leaf_prev) / sizeof(g_leaf_prev[0]))) return svt_hip_fail(nullptr, SVT_HIP_ERR_NO_MEMORY, "rtcd: too many slots");
            snprintf(g_leaf_prev[k].symbol, sizeof(g_leaf_prev[k].symbol), "%s", sym);
            g_leaf_nprev++;
        }
        g_leaf_prev[k].prev = prev;
        g_leaf_prev[k].slot = slots[i].slot;
        g_leaf_prev[k].entry = const_cast<void *>(fn);
        *slots[i].slot = const_cast<void *>(fn);
    }
    if (n_skipped) *n_skipped = skipped;
    return SVT_HIP_OK;
}

// What svt_aom_setup_rtcd_internal (Codec/aom_dsp_rtcd.c:188, called at Globals/enc_handle.c:1444-1445) does for a SIMD flavour: assign
// this backend's entries into the encoder's function pointers.  `slots[i].slot` is the ADDRESS of the encoder's pointer variable
// `slots[i].name`.  Names this library has no entry for are left as they are (the encoder keeps its own kernel there) and counted in
// *n_skipped.  Binds `ctx` for the pointer-level entries (they have no context argument).  Without a context nothing is touched: the
// encoder keeps its dispatch.  Call it before init_fn_ptr() (Codec/av1me.c:31, enc_handle.c:1460), which copies pointer VALUES into
// svt_aom_mefn_ptr[].
int svt_hip_install_rtcd(SvtHipContext *ctx, const SvtHipRtcdSlot *slots, uint32_t n_slots, uint32_t *n_skipped) {
    if (!ctx || (!slots && n_slots)) return SVT_HIP_ERR_BAD_PARAM;
    if (int rc = svt_hip_rtcd_store(slots, n_slots, n_skipped)) return rc;
    return svt_hip_leaf_bind(ctx);
}

// Puts the previous kernels back into the slots svt_hip_install_rtcd / svt_hip_rtcd_store wrote to (an encoder that gives the device up).  A slot
// that holds this library's entry no longer (the encoder ran its own set-up again) is left alone.  Either way the record goes: a later direct
// call of the entry finds no previous kernel, not a pointer into code that may be gone.
int svt_hip_uninstall_rtcd(const SvtHipRtcdSlot *slots, uint32_t n_slots) {
    if (!slots && n_slots) return SVT_HIP_ERR_BAD_PARAM;
    std::lock_guard<std::mutex> lock(g_leaf_prev_mutex);
    for (uint32_t i = 0; i < n_slots; i++) {
        if (!slots[i].slot) continue;
        for (int k = 0; k < g_leaf_nprev; k++) {
            LeafPrev &r = g_leaf_prev[k];
            if (r.slot != slots[i].slot) continue;
            if (r.prev && *r.slot == r.entry) *r.slot = r.prev;
            r = g_leaf_prev[--g_leaf_nprev]; // the table keeps no order
            break;
        }
    }
    return SVT_HIP_OK;
}

// Calls the previous kernels served since the last call (`fallbacks`), calls that failed with no previous kernel to go to (`unhandled`:
// their outputs are zero / untouched), and the last failure's text.  Any pointer may be null.  Returns the sum of both counts (saturated).
int svt_hip_leaf_status(unsigned long long *fallbacks, unsigned long long *unhandled, char *message, size_t message_bytes) {
    const unsigned long long f = g_leaf_fallbacks.exchange(0), u = g_leaf_unhandled.exchange(0);
    if (fallbacks) *fallbacks = f;
    if (unhandled) *unhandled = u;
    if (message && message_bytes) {
        std::lock_guard<std::mutex> lock(g_leaf_prev_mutex);
        snprintf(message, message_bytes, "%s", g_leaf_msg);
    }
    return (int)((f + u) > 0x7fffffffull ? 0x7fffffff : (f + u));
}

// Testing aid: while on, every pointer-level entry behaves as if the device had failed.
void svt_hip_leaf_inject_failure(int on) { g_leaf_inject.store(on ? 1 : 0); }

} // extern "C"
