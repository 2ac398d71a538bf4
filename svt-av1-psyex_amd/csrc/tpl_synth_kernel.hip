// tpl_synth_kernel.hip -- the TPL group on gfx950: tpl_mc_flow's frame loop (Source/Lib/Codec/src_ops_process.c:1783-1956), the
// synthesizer tpl_mc_flow_synthesizer (:1571-1584, tpl_model_update{,_b} :1480-1565) and svt_aom_generate_r0beta (:1585-1677) with
// generate_lambda_scaling_factor (:176-223).  C-ABI in include/svt_hip_tpl.h.
//
// Launches on the context stream, in this order:
//   stage 1  per frame: a memset of the grid, then the dispenser's five launches (tpl_kernel.hip) when tpl_valid_pic
//   stage 2  tpl_synth_kernel once per valid frame, last frame first: one thread per cell of the frame; the cell's <= 4 quadrants are
//            added to the reference frame's cells with 64-bit integer atomics (order-free, so bit-exact).  The frames stay one launch
//            each: frame f's mc_dep_dist is final only once every later frame has been propagated.
//   stage 3  tpl_r0beta_kernel: one workgroup per frame; the picture sums, r0, then the scaling factors and the per-SB beta.
// The window's frame table (picture_number, grid, outputs) is copied once per call into one of SVT_HIP_TPL_GROUP_RING device slots;
// an event recorded behind the call's last launch guards the slot (and its pinned staging copy) against the next reuse.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <mutex>
#include "svt_hip_internal.h"
#include "../../include/svt_hip_tpl.h"

// the reference's fp64 arithmetic: no contraction into fma, no fast-math
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kRddivBits = 7;         // RDDIV_BITS (Codec/rd_cost.h:35)
constexpr int kProbCostShift = 9;     // AV1_PROB_COST_SHIFT

// one frame of the window as the kernels read it
struct GroupEntry {
    uint64_t        picture_number;
    SvtHipTplStats *grid;
    double         *r0;
    uint8_t        *valid;
    double         *beta;
    double         *scaling;
    int32_t         base_rdmult;
    uint32_t        reserved;
};
constexpr size_t kSlotBytes = sizeof(GroupEntry) * SVT_HIP_TPL_MAX_GROUP;

// the geometry every stage derives from the group descriptor (mi units are 4x4)
struct GroupGeom {
    int n_frames;
    int s, shift;            // synth size, log2(s / 4): s / 4 = 1 << shift is both the mi size of a cell and the loops' step
    int mi_rows, mi_cols;    // aligned_height >> 2, aligned_width >> 2
    int stride_a;            // ((aligned_width + 15) / 16 * 4) >> shift: the synthesizer's row stride
    int mi_cols_sr, stride_u; // (width + 15) / 16 * 4 and >> shift: generate_r0beta's / generate_lambda_scaling_factor's
    int mi_rows_u;           // (height + 15) / 16 * 4: the per-SB cut
    int rows_s, cols_s;      // cells the synthesizer walks
    int rows_p, cols_p;      // cells of the picture sum, = the scaling grid
    int sb_mi, sb_w, sb_h;   // sb_size / 4, superblocks per row / column
};

// int64 arithmetic of the reference: two's complement wrap-around, C's truncating division
__device__ __forceinline__ int64_t wadd(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }
__device__ __forceinline__ int64_t wsub(int64_t a, int64_t b) { return (int64_t)((uint64_t)a - (uint64_t)b); }
__device__ __forceinline__ int64_t wmul(int64_t a, int64_t b) { return (int64_t)((uint64_t)a * (uint64_t)b); }
__device__ __forceinline__ int64_t tdiv(int64_t a, int64_t b) { return b == -1 ? wsub(0, a) : a / b; } // b != 0
__device__ __forceinline__ int64_t wshl(int64_t a, int n) { return (int64_t)((uint64_t)a << n); }

// RDCOST (Codec/rd_cost.h:37-39): ROUND_POWER_OF_TWO(R * RM, AV1_PROB_COST_SHIFT) + D * (1 << RDDIV_BITS)
__device__ __forceinline__ int64_t rdcost(int64_t rm, int64_t r, int64_t d) {
    return wadd(wadd(wmul(r, rm), (1 << kProbCostShift) >> 1) >> kProbCostShift, wmul(d, (int64_t)1 << kRddivBits));
}

__device__ __forceinline__ int round_floor(int x, int b) { return x < 0 ? -(1 + (-x - 1) / b) : x / b; } // :1440-1448

__device__ __forceinline__ int overlap_area(int gr, int gc, int rr, int rc, int block, int b) { // get_overlap_area (:1411-1438)
    const int w = (block & 1) ? rc + b - gc : gc + b - rc;
    const int h = (block >> 1) ? rr + b - gr : gr + b - rr;
    return w * h;
}

// tpl_model_update + tpl_model_update_b for every cell of frame f (the synth block of a cell is one synth cell: one iteration of
// tpl_model_update's loops).  compute_rate is 0, so mc_dep_rate's own term is 0.
__global__ void __launch_bounds__(kThreads) tpl_synth_kernel(const GroupEntry *tab, const GroupGeom g, int f) {
    __shared__ uint64_t pn[SVT_HIP_TPL_MAX_GROUP];
    for (int i = threadIdx.x; i < g.n_frames; i += kThreads) pn[i] = tab[i].picture_number;
    __syncthreads();
    const int cell = blockIdx.x * kThreads + threadIdx.x;
    if (cell >= g.rows_s * g.cols_s) return;
    const int cy = cell / g.cols_s, cx = cell - cy * g.cols_s;
    const SvtHipTplStats st = tab[f].grid[(size_t)cy * g.stride_a + cx];
    int i = 0; // the FIRST frame of the window with that picture number (:1559)
    while (i < g.n_frames && pn[i] != st.ref_frame_poc) i++;
    // no match: nothing.  Its own frame: nothing (only intra cells name it; they add zero).  recrf_dist == 0: nothing (the reference
    // divides by zero there)
    if (i == g.n_frames || i == f || st.recrf_dist == 0) return;
    const int S = g.s, pix_num = S * S;
    const int mv_r = (int16_t)((st.mv_row + 3 + (st.mv_row >= 0)) >> 3); // GET_MV_RAWPEL (block_structures.h:41)
    const int mv_c = (int16_t)((st.mv_col + 3 + (st.mv_col >= 0)) >> 3);
    const int ref_r = cy * S + mv_r, ref_c = cx * S + mv_c;
    const int base_r = round_floor(ref_r, S) * S, base_c = round_floor(ref_c, S) * S;
    const int64_t cur_dep = wsub(st.recrf_dist, st.srcrf_dist);
    const int64_t mc_dep = tdiv(wmul(st.mc_dep_dist, cur_dep), st.recrf_dist);
    const int64_t dist = wadd(cur_dep, mc_dep), rate = wsub(st.recrf_rate, st.srcrf_rate);
    SvtHipTplStats *ref = tab[i].grid;
    for (int block = 0; block < 4; block++) {
        const int gr = base_r + S * (block >> 1), gc = base_c + S * (block & 1);
        if (gr < 0 || gr >= g.mi_rows * 4 || gc < 0 || gc >= g.mi_cols * 4) continue; // the reference frame's aligned size
        const int area = overlap_area(gr, gc, ref_r, ref_c, block, S);
        SvtHipTplStats *t = ref + (size_t)(gr / S) * g.stride_a + gc / S;
        atomicAdd(reinterpret_cast<unsigned long long *>(&t->mc_dep_dist), (unsigned long long)(wmul(dist, area) / pix_num));
        atomicAdd(reinterpret_cast<unsigned long long *>(&t->mc_dep_rate), (unsigned long long)(wmul(rate, area) / pix_num));
    }
}

// svt_aom_generate_r0beta + generate_lambda_scaling_factor of one frame per workgroup
__global__ void __launch_bounds__(kThreads) tpl_r0beta_kernel(const GroupEntry *tab, const GroupGeom g) {
    __shared__ int64_t s_rec[kThreads], s_del[kThreads], s_max[kThreads];
    __shared__ double s_r0;
    __shared__ int s_cost_nz;
    const GroupEntry e = tab[blockIdx.x];
    if (!e.r0) return;
    const int tid = threadIdx.x;
    const SvtHipTplStats *grid = e.grid;
    const int64_t rm = e.base_rdmult;
    int64_t rec = 0, del = 0, mx = 0;
    const int n_p = g.rows_p * g.cols_p;
    for (int k = tid; k < n_p; k += kThreads) { // row < mi_rows (aligned), col < mi_cols_sr (unscaled width rounded up to 16)
        const int r = k / g.cols_p, c = k - r * g.cols_p;
        const SvtHipTplStats &t = grid[(size_t)r * g.stride_u + c];
        const int64_t d = rdcost(rm, t.mc_dep_rate, t.mc_dep_dist);
        rec = wadd(rec, t.recrf_dist);
        del = wadd(del, d);
        mx = d > mx ? d : mx;
    }
    s_rec[tid] = rec; s_del[tid] = del; s_max[tid] = mx;
    __syncthreads();
    for (int h = kThreads / 2; h > 0; h >>= 1) { // wrap-around sums and a max: the order does not change them
        if (tid < h) {
            s_rec[tid] = wadd(s_rec[tid], s_rec[tid + h]);
            s_del[tid] = wadd(s_del[tid], s_del[tid + h]);
            s_max[tid] = s_max[tid + h] > s_max[tid] ? s_max[tid + h] : s_max[tid];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int64_t rsum = s_rec[0], dsum = s_del[0], max_dist = s_max[0], count = n_p;
        const int64_t cost = wadd(wshl(rsum, kRddivBits), dsum); // mc_dep_cost_base
        double r0 = *e.r0; // kept when cost == 0: beta reads it
        if (cost != 0) {
            r0 = (double)wshl(rsum, kRddivBits) / (double)cost;
            if (max_dist > wmul(tdiv(dsum, count), 100) && max_dist > tdiv(wmul(dsum, 9), 10)) r0 = 1.0; // outlier blocks
            *e.r0 = r0;
            *e.valid = 1;
        } else
            *e.valid = 0;
        s_r0 = r0;
        s_cost_nz = cost != 0;
    }
    __syncthreads();
    const double r0 = s_r0;
    for (int k = tid; k < n_p; k += kThreads) { // generate_lambda_scaling_factor: index row * num_cols + col, grid at stride_u
        const int r = k / g.cols_p, c = k - r * g.cols_p;
        const SvtHipTplStats &t = grid[(size_t)r * g.stride_u + c];
        double sf = 1.2;
        if (s_cost_nz && t.recrf_dist > 0) {
            const int64_t num = wshl(t.recrf_dist, kRddivBits);
            const double rk = (double)num / (double)wadd(num, rdcost(rm, t.mc_dep_rate, t.mc_dep_dist));
            sf += rk / r0;
        }
        e.scaling[k] = sf;
    }
    for (int k = tid; k < g.sb_w * g.sb_h; k += kThreads) { // the superblocks
        const int sy = k / g.sb_w, sx = k - sy * g.sb_w;
        const int mi_row = sy * g.sb_mi, mi_col = sx * g.sb_mi, step = 1 << g.shift;
        int64_t rsum = 0, dsum = 0;
        for (int row = mi_row; row < mi_row + g.sb_mi; row += step) {
            if (row >= g.mi_rows_u) break;
            for (int col = mi_col; col < mi_col + g.sb_mi; col += step) {
                if (col >= g.mi_cols_sr) break;
                const SvtHipTplStats &t = grid[(size_t)(row >> g.shift) * g.stride_u + (col >> g.shift)];
                rsum = wadd(rsum, t.recrf_dist);
                dsum = wadd(dsum, rdcost(rm, t.mc_dep_rate, t.mc_dep_dist));
            }
        }
        double beta = 1.0;
        if (rsum > 0) {
            const int64_t num = wshl(rsum, kRddivBits);
            const double rk = (double)num / (double)wadd(num, dsum);
            beta = r0 / rk;
        }
        e.beta[k] = beta;
    }
}

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

GroupGeom geom_of(const SvtHipTplGroupDesc *d) {
    GroupGeom g;
    g.n_frames   = (int)d->n_frames;
    g.s          = d->synth_blk_size;
    g.shift      = g.s == 16 ? 2 : 3;
    g.mi_rows    = d->aligned_height >> 2;
    g.mi_cols    = d->aligned_width >> 2;
    g.stride_a   = (((d->aligned_width + 15) / 16) << 2) >> g.shift;
    g.mi_cols_sr = ((d->width + 15) / 16) << 2;
    g.stride_u   = g.mi_cols_sr >> g.shift;
    g.mi_rows_u  = ((d->height + 15) / 16) << 2;
    const int n = 1 << g.shift;
    g.rows_s = cdiv(g.mi_rows, n);
    g.cols_s = cdiv(g.mi_cols, n);
    g.rows_p = cdiv(g.mi_rows, n);
    g.cols_p = cdiv(g.mi_cols_sr, n);
    g.sb_mi  = d->sb_size >> 2;
    g.sb_w   = cdiv(d->aligned_width, d->sb_size);
    g.sb_h   = cdiv(d->aligned_height, d->sb_size);
    return g;
}

// the cells stage 1 zeroes: the reference's allocation, ceil(width / s) x ceil(height / s) (pcs.c:1446-1479, :1841-1845)
uint32_t zeroed_cells(const SvtHipTplGroupDesc *d) {
    return (uint32_t)cdiv(d->width, d->synth_blk_size) * (uint32_t)cdiv(d->height, d->synth_blk_size);
}

bool any_outputs(const SvtHipTplGroupFrame &f) { return f.r0 || f.tpl_is_valid || f.beta || f.scaling; }

} // namespace

void svt_hip_tpl_group_free(SvtHipContext *ctx) { // teardown: nothing here can act on a failure
    for (hipEvent_t &e : ctx->tpl_group_done)
        if (e) { (void)hipEventSynchronize(e); (void)hipEventDestroy(e); e = nullptr; }
    if (ctx->tpl_group_dev) (void)hipFree(ctx->tpl_group_dev);
    if (ctx->tpl_group_host) (void)hipHostFree(ctx->tpl_group_host);
    ctx->tpl_group_dev = ctx->tpl_group_host = nullptr;
}

extern "C" {

size_t svt_hip_tpl_group_desc_size(void) { return sizeof(SvtHipTplGroupDesc); }
size_t svt_hip_tpl_group_frame_size(void) { return sizeof(SvtHipTplGroupFrame); }

int svt_hip_tpl_group_check_desc(const SvtHipTplGroupDesc *d) {
#define BAD(...) return svt_hip_fail(nullptr, SVT_HIP_ERR_BAD_PARAM, __VA_ARGS__)
    if (!d) BAD("svt_hip_tpl_group_check_desc: null descriptor");
    if (!d->stages || (d->stages & ~(SVT_HIP_TPL_STAGE_DISPENSE | SVT_HIP_TPL_STAGE_SYNTHESIZE | SVT_HIP_TPL_STAGE_R0BETA)))
        BAD("TPL group: stages 0x%x", d->stages);
    if (d->compute_rate != 0) BAD("TPL group: compute_rate (delta_rate_cost's log / pow) runs on the host");
    if (d->synth_blk_size != 16 && d->synth_blk_size != 32) BAD("TPL group: synth_blk_size %u (16 or 32)", d->synth_blk_size);
    if (d->superres_denom != 8) BAD("TPL group: superres_denom %u (super-res / resize run on the host)", d->superres_denom);
    if (d->sb_size != 64 && d->sb_size != 128) BAD("TPL group: sb_size %u (64 or 128)", d->sb_size);
    if (!d->n_frames || d->n_frames > SVT_HIP_TPL_MAX_GROUP) BAD("TPL group: n_frames %u (1 .. %d)", d->n_frames, SVT_HIP_TPL_MAX_GROUP);
    if (!d->frames) BAD("TPL group: null frame array");
    if (!d->width || !d->height || d->aligned_width < d->width || d->aligned_height < d->height)
        BAD("TPL group: picture %ux%u, aligned %ux%u", d->width, d->height, d->aligned_width, d->aligned_height);
    const GroupGeom g = geom_of(d);
    const bool st1 = d->stages & SVT_HIP_TPL_STAGE_DISPENSE, st2 = d->stages & SVT_HIP_TPL_STAGE_SYNTHESIZE,
               st3 = d->stages & SVT_HIP_TPL_STAGE_R0BETA;
    // the last cell each stage touches + 1
    uint64_t need = zeroed_cells(d);
    const uint64_t need_s = (uint64_t)(g.rows_s - 1) * g.stride_a + g.cols_s;
    const uint64_t need_p = (uint64_t)(g.rows_p - 1) * g.stride_u + g.cols_p;
    const int last_row = (g.mi_rows_u < g.sb_h * g.sb_mi ? g.mi_rows_u : g.sb_h * g.sb_mi) - 1;
    const int last_col = (g.mi_cols_sr < g.sb_w * g.sb_mi ? g.mi_cols_sr : g.sb_w * g.sb_mi) - 1;
    const uint64_t need_b = (uint64_t)(last_row >> g.shift) * g.stride_u + (last_col >> g.shift) + 1;
    if (st1 || st2) need = need > need_s ? need : need_s;
    const uint64_t n_beta = (uint64_t)g.sb_w * g.sb_h, n_scaling = (uint64_t)g.rows_p * g.cols_p;
    for (uint32_t i = 0; i < d->n_frames; i++) {
        const SvtHipTplGroupFrame &f = d->frames[i];
        if (!f.tpl_stats) BAD("TPL group: frame %u: null grid", i);
        uint64_t need_f = need;
        if (st3 && any_outputs(f)) {
            if (!f.r0 || !f.tpl_is_valid || !f.beta || !f.scaling) BAD("TPL group: frame %u: r0 / tpl_is_valid / beta / scaling: all or none", i);
            if (f.n_beta < n_beta) BAD("TPL group: frame %u: beta holds %u entries, the superblocks %llu", i, f.n_beta, (unsigned long long)n_beta);
            if (f.n_scaling < n_scaling) BAD("TPL group: frame %u: scaling holds %u entries, the grid %llu", i, f.n_scaling, (unsigned long long)n_scaling);
            need_f = need_f > need_p ? need_f : need_p;
            need_f = need_f > need_b ? need_f : need_b;
        }
        if (f.n_tpl_stats < need_f) BAD("TPL group: frame %u: grid holds %u cells, %llu needed", i, f.n_tpl_stats, (unsigned long long)need_f);
        if (st1 && f.tpl_valid_pic) {
            const SvtHipTplDesc *t = f.dispense;
            if (!t) BAD("TPL group: frame %u: no dispenser descriptor", i);
            const int rc = svt_hip_tpl_check_desc(t);
            if (rc) return rc;
            if (t->tpl_stats != f.tpl_stats || t->n_tpl_stats > f.n_tpl_stats || t->synth_blk_size != d->synth_blk_size ||
                t->aligned_width != d->aligned_width || t->aligned_height != d->aligned_height || t->cur.width != d->width || t->cur.height != d->height)
                BAD("TPL group: frame %u: the dispenser descriptor does not match the frame (grid, synth size or picture size)", i);
        }
    }
    if (st1 || st2) // grids written by one stage and read by another must not share cells
        for (uint32_t i = 0; i < d->n_frames; i++)
            for (uint32_t j = i + 1; j < d->n_frames; j++) {
                const uintptr_t a0 = (uintptr_t)d->frames[i].tpl_stats, a1 = a0 + (uintptr_t)d->frames[i].n_tpl_stats * sizeof(SvtHipTplStats);
                const uintptr_t b0 = (uintptr_t)d->frames[j].tpl_stats, b1 = b0 + (uintptr_t)d->frames[j].n_tpl_stats * sizeof(SvtHipTplStats);
                if (a0 < b1 && b0 < a1) BAD("TPL group: frames %u and %u share grid cells", i, j);
            }
    return SVT_HIP_OK;
#undef BAD
}

int svt_hip_tpl_group(SvtHipContext *ctx, const SvtHipTplGroupDesc *d) {
    if (!ctx) return svt_hip_fail(nullptr, SVT_HIP_ERR_BAD_PARAM, "svt_hip_tpl_group: null context");
    int rc = svt_hip_tpl_group_check_desc(d);
    if (rc) return rc;
    const GroupGeom g = geom_of(d);
    std::lock_guard<std::mutex> lk(ctx->async_mu);
    if ((rc = svt_hip_use_device(ctx))) return rc;
    if (!ctx->tpl_group_dev) {
        if (hipMalloc(&ctx->tpl_group_dev, kSlotBytes * SVT_HIP_TPL_GROUP_RING) != hipSuccess) {
            ctx->tpl_group_dev = nullptr;
            return svt_hip_fail(ctx, SVT_HIP_ERR_NO_MEMORY, "TPL group: hipMalloc of the frame tables failed");
        }
        if (hipHostMalloc(&ctx->tpl_group_host, kSlotBytes * SVT_HIP_TPL_GROUP_RING) != hipSuccess) {
            ctx->tpl_group_host = nullptr;
            (void)hipFree(ctx->tpl_group_dev); // the host allocation's failure is the one reported
            ctx->tpl_group_dev = nullptr;
            return svt_hip_fail(ctx, SVT_HIP_ERR_NO_MEMORY, "TPL group: hipHostMalloc of the frame tables failed");
        }
        for (hipEvent_t &e : ctx->tpl_group_done) SVT_HIP_CHECK(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    const int slot = ctx->tpl_group_next;
    ctx->tpl_group_next = (slot + 1) % SVT_HIP_TPL_GROUP_RING;
    SVT_HIP_CHECK(ctx, hipEventSynchronize(ctx->tpl_group_done[slot])); // an earlier call's copy of this slot is read no more
    GroupEntry *host = reinterpret_cast<GroupEntry *>(static_cast<uint8_t *>(ctx->tpl_group_host) + kSlotBytes * slot);
    GroupEntry *dev  = reinterpret_cast<GroupEntry *>(static_cast<uint8_t *>(ctx->tpl_group_dev) + kSlotBytes * slot);
    const bool st3 = d->stages & SVT_HIP_TPL_STAGE_R0BETA;
    for (uint32_t i = 0; i < d->n_frames; i++) {
        const SvtHipTplGroupFrame &f = d->frames[i];
        GroupEntry &e = host[i];
        memset(&e, 0, sizeof(e));
        e.picture_number = f.picture_number;
        e.grid = f.tpl_stats;
        e.base_rdmult = f.base_rdmult;
        if (st3 && any_outputs(f)) { e.r0 = f.r0; e.valid = f.tpl_is_valid; e.beta = f.beta; e.scaling = f.scaling; }
    }
    SVT_HIP_CHECK(ctx, hipMemcpyAsync(dev, host, sizeof(GroupEntry) * d->n_frames, hipMemcpyHostToDevice, ctx->stream));
    auto stages = [&]() -> int {
        if (d->stages & SVT_HIP_TPL_STAGE_DISPENSE) { // tpl_mc_flow's frame loop
            const size_t zero_bytes = sizeof(SvtHipTplStats) * zeroed_cells(d);
            for (uint32_t i = 0; i < d->n_frames; i++) {
                const SvtHipTplGroupFrame &f = d->frames[i];
                SVT_HIP_CHECK(ctx, hipMemsetAsync(f.tpl_stats, 0, zero_bytes, ctx->stream));
                if (f.tpl_valid_pic) {
                    const int r = svt_hip_tpl_dispense_locked(ctx, f.dispense);
                    if (r) return r;
                }
            }
        }
        if (d->stages & SVT_HIP_TPL_STAGE_SYNTHESIZE) {
            const int blocks = (g.rows_s * g.cols_s + kThreads - 1) / kThreads;
            for (int i = (int)d->n_frames - 1; i >= 0; i--)
                if (d->frames[i].tpl_valid_pic) hipLaunchKernelGGL(tpl_synth_kernel, dim3(blocks), dim3(kThreads), 0, ctx->stream, dev, g, i);
            SVT_HIP_CHECK(ctx, hipGetLastError());
        }
        if (st3) {
            hipLaunchKernelGGL(tpl_r0beta_kernel, dim3(d->n_frames), dim3(kThreads), 0, ctx->stream, dev, g);
            SVT_HIP_CHECK(ctx, hipGetLastError());
        }
        return SVT_HIP_OK;
    };
    rc = stages();
    const hipError_t er = hipEventRecord(ctx->tpl_group_done[slot], ctx->stream); // also after a failed launch: the copy is in flight
    if (rc) return rc;
    SVT_HIP_CHECK(ctx, er);
    return SVT_HIP_OK;
}

} // extern "C"
