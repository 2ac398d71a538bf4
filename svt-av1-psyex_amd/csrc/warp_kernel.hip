// warp_kernel.hip -- warped motion on gfx950: svt_hip_warp_pred_batch, the 8x8-tile warp filter into the plane svt_hip_rd_batch reads, and
// svt_hip_warp_model_batch, the least-squares fit of the local-warp model for an MV that is already on the device, and svt_hip_wm_refine_batch,
// the MV refinement that runs both up to 129 times per block.
//
// Reference functions restated (Source/Lib/Codec):
//   svt_av1_warp_plane, svt_warp_plane, svt_highbd_warp_plane, svt_av1_warp_affine_c, svt_av1_highbd_warp_affine_c   warped_motion.c:569-895
//   plane_warped_motion_prediction (the ConvolveParams: round_0 3, round_1 7 for a compound)                          enc_inter_prediction.c:2040-2145
//   svt_aom_warped_motion_parameters (from the MV on), svt_aom_select_samples                                          adaptive_mv_pred.c:1736-1754, warped_motion.c:924-972
//   find_affine_int, svt_find_projection, svt_get_shear_params, is_affine_shear_allowed, resolve_divisor_64 / _32      warped_motion.c:320-483, 898-921
//   get_mult_shift_diag / _ndiag (USE_LIMITED_PREC_MULT 0)                                                              warped_motion.c:277-289
//   svt_aom_wm_motion_refinement (the search loop), svt_aom_variance{W}x{H}_c, svt_aom_mv_err_cost / _light           mode_decision.c:2082-2204, C_DEFAULT/variance.c, av1me.c:229-252
//
// Lay-out of the prediction: a workgroup of four waves per job, a wave per 8x8 tile at a time, a lane per output sample.  The tile's geometry
// (ix4, iy4, sx4, sy4) comes from the job alone and lives in scalar registers.  The 15 x 15 source window (every coordinate clamped to the
// picture) is staged into the wave's own LDS once, four samples per lane; the horizontal filter runs as two passes of 8 x 8 lanes over it and
// leaves its 15 x 8 intermediate (at most 15 bits) in LDS; the vertical filter reads a column of eight from there.  Only wave_sync() orders the
// traffic: no wave waits for another.  The filter of a lane differs per lane and per row, so the 193 x 8 table is read with one 16-byte load per
// lane from constant memory, where its 3 KB stay in the vector cache; an LDS copy would cost every workgroup a fill and a barrier it cannot
// amortise over one job.  A compound job runs both references per tile and keeps the first result in a register.
//
// The tables, the tile (warp_tile) and the integer pieces of svt_get_shear_params live in warp_core.h, which gm_kernel.hip shares.
//
// The fit is one lane per job, 32- and 64-bit integer code.  svt_aom_select_samples only reorders: the least-squares sums do not depend on the
// order, so the kept samples are summed where they lie, and no array is indexed by a register.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include "batch_host.h"
#include "../../include/svt_hip_warp.h"
#include "wave_ops.h"
#include "warp_core.h"
#include "mv_cost.h"

namespace {

constexpr int kWaves = 4;

__device__ __forceinline__ bool is_warp_size(int w, int h) { // the 17 block sizes with both dimensions >= 8
    const bool pw = w >= 8 && w <= 128 && (w & (w - 1)) == 0, ph = h >= 8 && h <= 128 && (h & (h - 1)) == 0;
    if (!pw || !ph) return false;
    const int big = w > h ? w : h, small = w > h ? h : w;
    return big == small || big == 2 * small || (big == 4 * small && big <= 64);
}

template <bool HBD> __global__ __launch_bounds__(64 * kWaves) void warp_pred_kernel(const SvtHipWarpPredDesc d) {
    using Px = typename std::conditional<HBD, uint16_t, uint8_t>::type;
    __shared__ uint16_t s_src[kWaves][15 * 16];
    __shared__ uint16_t s_mid[kWaves][15 * 8];
    constexpr int bd = HBD ? 10 : 8, px_max = (1 << bd) - 1;
    const int      lane = (int)(threadIdx.x & 63u);
    const int      wave = uniform((int)(threadIdx.x >> 6));
    const uint32_t job  = blockIdx.x;
    if (job >= d.n_jobs) return;
    const SvtHipWarpPredJob *jp = d.jobs + job;
    const int  w = jp->width, h = jp->height, flags = jp->flags;
    const int  ref0 = jp->ref[0], ref1 = jp->ref[1];
    const bool comp = ref1 != SVT_HIP_WARP_NO_REF;
    const int  comp_mode = jp->comp_mode, fwd = jp->fwd_offset, bck = jp->bck_offset;
    const bool first = wave == 0 && lane == 0;

    bool ok = is_warp_size(w, h) && ref0 < d.n_refs;
    if (comp) {
        ok = ok && ref1 < d.n_refs && comp_mode <= 1;
        if (comp_mode == 1) // quant_dist_lookup_table: {9,7} {11,5} {12,4} {13,3} and their mirrors
            ok = ok && fwd + bck == 16 && (fwd == 9 || fwd == 11 || fwd == 12 || fwd == 13 || fwd == 7 || fwd == 5 || fwd == 4 || fwd == 3);
    }
    const bool arr0 = (flags & SVT_HIP_WARP_MODEL0_FROM_ARRAY) != 0, arr1 = comp && (flags & SVT_HIP_WARP_MODEL1_FROM_ARRAY) != 0;
    if (arr0) ok = ok && d.models != nullptr && jp->model_index[0] < d.n_models;
    if (arr1) ok = ok && d.models != nullptr && jp->model_index[1] < d.n_models;
    ok = ok && (uint64_t)jp->dst_offset + (uint64_t)(h > 0 ? h - 1 : 0) * d.dst_stride + (uint64_t)w <= d.dst_samples;
    if (!ok) {
        if (first) d.status[job] = SVT_HIP_WARP_UNDEFINED;
        return;
    }
    const SvtHipWarpModel *mp0 = arr0 ? d.models + jp->model_index[0] : &jp->model[0];
    const SvtHipWarpModel *mp1 = !comp ? mp0 : (arr1 ? d.models + jp->model_index[1] : &jp->model[1]);
    if ((arr0 && mp0->valid == 0) || (arr1 && mp1->valid == 0)) {
        if (first) d.status[job] = SVT_HIP_WARP_NO_MODEL;
        return;
    }
    Model m[2];
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const SvtHipWarpModel *mp = r ? mp1 : mp0;
        const int type = mp->wmtype;
#pragma unroll
        for (int i = 0; i < 6; i++) m[r].mat[i] = uniform(mp->wmmat[i]);
        if (type == SVT_HIP_WARP_ROTZOOM) { m[r].mat[5] = m[r].mat[2]; m[r].mat[4] = (int)(0u - (uint32_t)m[r].mat[3]); }
        m[r].alpha = uniform(mp->alpha); m[r].beta = uniform(mp->beta); m[r].gamma = uniform(mp->gamma); m[r].delta = uniform(mp->delta);
        ok = ok && (type == SVT_HIP_WARP_ROTZOOM || type == SVT_HIP_WARP_AFFINE) && shear_allowed(m[r].alpha, m[r].beta, m[r].gamma, m[r].delta);
    }
    if (!ok) {
        if (first) d.status[job] = SVT_HIP_WARP_UNDEFINED;
        return;
    }

    const SvtHipWarpRef r0 = d.refs[ref0], r1 = d.refs[comp ? ref1 : ref0];
    const int ss_x = d.ss_x, ss_y = d.ss_y, p_col = jp->p_col, p_row = jp->p_row;
    const int log2_tx = 31 - __builtin_clz((unsigned)(w >> 3)), n_tiles = (w >> 3) * (h >> 3);
    Px *const dst = (Px *)d.dst + (size_t)jp->dst_offset;
    const int c = lane & 7, rr = lane >> 3;
    for (int t = wave; t < n_tiles; t += kWaves) {
        const int ty = t >> log2_tx, tx = t & ((1 << log2_tx) - 1);
        const int jx = p_col + 8 * tx, iy = p_row + 8 * ty;
        int v;
        if (!comp) {
            v = warp_tile<HBD>(r0, m[0], jx, iy, ss_x, ss_y, 11, s_src[wave], s_mid[wave], lane) - (1 << (bd - 1)) - (1 << bd);
        } else {
            const int a = warp_tile<HBD>(r0, m[0], jx, iy, ss_x, ss_y, 7, s_src[wave], s_mid[wave], lane);
            const int b = warp_tile<HBD>(r1, m[1], jx, iy, ss_x, ss_y, 7, s_src[wave], s_mid[wave], lane);
            int tmp = comp_mode ? (a * fwd + b * bck) >> 4 : (a + b) >> 1;
            tmp -= (1 << (bd + 4)) + (1 << (bd + 3)); // offset_bits - round_1 and one below, offset_bits = bd + 2 * FILTER_BITS - round_0
            v = (tmp + 8) >> 4;                       // round_bits = 2 * FILTER_BITS - round_0 - round_1
        }
        dst[(size_t)(8 * ty + rr) * d.dst_stride + (size_t)(8 * tx + c)] = (Px)clampi(v, 0, px_max);
    }
    if (first) d.status[job] = SVT_HIP_WARP_OK;
}

// ---- the fit ----

// What the two jobs that fit a model share: the samples and the block (the head of SvtHipWarpModelJob and of SvtHipWmRefineJob)
struct FitInput {
    const int32_t *pts, *pts_inref;
    int n, bw, bh, org_x, org_y;
    bool shut_approx;
    int  lower_band_th, upper_band_th;
};

// The MV-dependent half of svt_aom_warped_motion_parameters for the MV (mvy, mvx): the record as svt_hip_warp_model_batch writes it
__device__ __forceinline__ SvtHipWarpModel fit_model(const FitInput &in, int mvy, int mvx) {
    const int32_t *const pts = in.pts, *const pts_inref = in.pts_inref;
    const int bw = in.bw, bh = in.bh, n = in.n;
    SvtHipWarpModel out;
    memset(&out, 0, sizeof(out));
    out.wmtype = SVT_HIP_WARP_AFFINE;
    bool valid = n > 0;
    if (valid) {
        // svt_aom_select_samples: which samples stay (bit i), and how many
        const int thresh = clampi(bw > bh ? bw : bh, 16, 112);
        uint32_t  keep = 0;
        int       np = 0;
#pragma unroll
        for (int i = 0; i < SVT_HIP_WARP_MAX_SAMPLES; i++) {
            if (i < n) {
                const int mvd = iabs(pts_inref[2 * i] - pts[2 * i] - mvx) + iabs(pts_inref[2 * i + 1] - pts[2 * i + 1] - mvy);
                if (mvd <= thresh) { keep |= 1u << i; np++; }
            }
        }
        if (n == 1 || np == 0) { keep = 1; np = 1; } // a single sample is not selected; none kept: the first one, untouched
        out.num_samples = (uint16_t)np;

        // find_affine_int
        const int rsuy = bh / 2 - 1, rsux = bw / 2 - 1, suy = rsuy * 8, sux = rsux * 8, duy = suy + mvy, dux = sux + mvx;
        const int isuy = (in.org_y >> 2) * 4 + rsuy, isux = (in.org_x >> 2) * 4 + rsux;
        int32_t   a00 = 0, a01 = 0, a11 = 0, bx0 = 0, bx1 = 0, by0 = 0, by1 = 0;
#pragma unroll
        for (int i = 0; i < SVT_HIP_WARP_MAX_SAMPLES; i++) {
            if (keep & (1u << i)) {
                const int dx = pts_inref[2 * i] - dux, dy = pts_inref[2 * i + 1] - duy, sx = pts[2 * i] - sux, sy = pts[2 * i + 1] - suy;
                if (iabs(sx - dx) < 256 && iabs(sy - dy) < 256) { // LS_MV_MAX; LS_SQUARE, LS_PRODUCT1, LS_PRODUCT2 with LS_STEP 8
                    a00 += (sx * sx * 4 + sx * 32 + 128) >> 4;
                    a01 += (sx * sy * 4 + (sx + sy) * 16 + 64) >> 4;
                    a11 += (sy * sy * 4 + sy * 32 + 128) >> 4;
                    bx0 += (sx * dx * 4 + (sx + dx) * 16 + 128) >> 4;
                    bx1 += (sy * dx * 4 + (sy + dx) * 16 + 64) >> 4;
                    by0 += (sx * dy * 4 + (sx + dy) * 16 + 64) >> 4;
                    by1 += (sy * dy * 4 + (sy + dy) * 16 + 128) >> 4;
                }
            }
        }
        const int64_t det = (int64_t)a00 * a11 - (int64_t)a01 * a01;
        valid = det != 0;
        if (valid) {
            int shift;
            int i_det = (int16_t)(resolve_divisor((uint64_t)(det < 0 ? -det : det), &shift) * (det < 0 ? -1 : 1));
            shift -= 16;
            if (shift < 0) { i_det = (int16_t)(i_det * (1 << -shift)); shift = 0; } // i_det is an int16_t in the reference
            const int64_t px0 = (int64_t)a11 * bx0 - (int64_t)a01 * bx1, px1 = -(int64_t)a01 * bx0 + (int64_t)a00 * bx1;
            const int64_t py0 = (int64_t)a11 * by0 - (int64_t)a01 * by1, py1 = -(int64_t)a01 * by0 + (int64_t)a00 * by1;
            const int     lo = -(1 << 13) + 1, hi = (1 << 13) - 1;
            const int m2 = clamp64(round_shift_signed_64(px0 * i_det, shift), (1 << 16) + lo, (1 << 16) + hi);
            const int m3 = clamp64(round_shift_signed_64(px1 * i_det, shift), lo, hi);
            const int m4 = clamp64(round_shift_signed_64(py0 * i_det, shift), lo, hi);
            const int m5 = clamp64(round_shift_signed_64(py1 * i_det, shift), (1 << 16) + lo, (1 << 16) + hi);
            const int vx = (int)((uint32_t)mvx * (1u << 13) - ((uint32_t)isux * (uint32_t)(m2 - (1 << 16)) + (uint32_t)isuy * (uint32_t)m3));
            const int vy = (int)((uint32_t)mvy * (1u << 13) - ((uint32_t)isux * (uint32_t)m4 + (uint32_t)isuy * (uint32_t)(m5 - (1 << 16))));
            const int m0 = clampi(vx, -(1 << 23), (1 << 23) - 1), m1 = clampi(vy, -(1 << 23), (1 << 23) - 1);
            // svt_get_shear_params
            valid = m2 > 0;
            if (valid) {
                int al, be, ga, de;
                valid = shear_params(m2, m3, m4, m5, &al, &be, &ga, &de);
                if (valid && !in.shut_approx) {
                    if (iabs(al) + iabs(be) < in.lower_band_th && iabs(ga) + iabs(de) < in.lower_band_th) valid = false;
                    if (4 * iabs(al) + 7 * iabs(be) > in.upper_band_th && 4 * iabs(ga) + 4 * iabs(de) > in.upper_band_th) valid = false;
                }
                if (valid) {
                    out.wmmat[0] = m0; out.wmmat[1] = m1; out.wmmat[2] = m2; out.wmmat[3] = m3; out.wmmat[4] = m4; out.wmmat[5] = m5;
                    out.alpha = (int16_t)al; out.beta = (int16_t)be; out.gamma = (int16_t)ga; out.delta = (int16_t)de;
                }
            }
        }
    }
    out.valid = valid ? 1 : 0;
    return out;
}

__global__ __launch_bounds__(64) void warp_model_kernel(const SvtHipWarpModelDesc d) {
    const uint32_t job = blockIdx.x * 64u + threadIdx.x;
    if (job >= d.n_jobs) return;
    const SvtHipWarpModelJob *jp = d.jobs + job;
    const int bw = jp->bwidth, bh = jp->bheight, n = jp->n_samples;
    const bool from_array = (jp->flags & SVT_HIP_WARP_MV_FROM_ARRAY) != 0;
    if (!is_warp_size(bw, bh) || n > SVT_HIP_WARP_MAX_SAMPLES || (from_array && (d.mv_array == nullptr || jp->mv_index >= d.n_mvs))) {
        d.status[job] = SVT_HIP_WARP_UNDEFINED;
        return;
    }
    const int mvy = from_array ? d.mv_array[2 * (size_t)jp->mv_index] : jp->mv[0];
    const int mvx = from_array ? d.mv_array[2 * (size_t)jp->mv_index + 1] : jp->mv[1];
    const FitInput in = {jp->pts, jp->pts_inref, n, bw, bh, jp->blk_org_x, jp->blk_org_y, d.shut_approx != 0, d.lower_band_th, d.upper_band_th};
    d.models[job] = fit_model(in, mvy, mvx);
    d.status[job] = SVT_HIP_WARP_OK;
}

// ---- the refinement ----
// neighbors[9] of svt_aom_wm_motion_refinement as (row, col): the centre, the four sides, the four corners
__constant__ const int8_t kNeighbour[9][2] = {{0, 0}, {0, -1}, {1, 0}, {0, 1}, {-1, 0}, {-1, 1}, {1, 1}, {1, -1}, {-1, -1}};

// A workgroup of WAVES waves per job.  The search is one sequence of decisions, so every lane of the workgroup walks it with the same values:
// the positions, the record of tested MVs (in LDS, scanned 64 entries at a time), the fit (every lane computes it; it is a few hundred
// instructions against the thousands of a warp) and the comparison.  Only the warp is shared out: a wave takes every WAVES-th tile, reduces
// sum and SSE of its samples against the source, and the partial sums meet in LDS.
// The descriptor as it lies in the kernel-argument segment (it is the only argument), behind a barrier the compiler cannot see through: a field
// read through it is loaded where it is used, instead of being held in a scalar register across the whole search loop.
typedef __attribute__((address_space(4))) const SvtHipWmRefineDesc *KernargDesc; // the constant address space: scalar loads
__device__ __forceinline__ KernargDesc desc_in_kernarg() {
    KernargDesc p = (KernargDesc)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}

template <int WAVES> __global__ __launch_bounds__(64 * WAVES) void wm_refine_kernel(const SvtHipWmRefineDesc d) {
    __shared__ uint16_t s_src[WAVES][15 * 16];
    __shared__ uint16_t s_mid[WAVES][15 * 8];
    __shared__ uint32_t s_rec[1 + 8 * SVT_HIP_WM_MAX_ITERATIONS]; // mv_record: 9 positions in the first round, 8 in every other
    __shared__ uint32_t s_part[WAVES][2];
    const int      lane = (int)(threadIdx.x & 63u);
    const int      wave = uniform((int)(threadIdx.x >> 6));
    const uint32_t job  = blockIdx.x;
    if (job >= d.n_jobs) return;
    const SvtHipWmRefineJob *jp = d.jobs + job;
    const int  bw = jp->bwidth, bh = jp->bheight, n = jp->n_samples, ref = jp->ref;
    const bool from_array = (jp->flags & SVT_HIP_WM_START_FROM_ARRAY) != 0;
    bool ok = is_warp_size(bw, bh) && n <= SVT_HIP_WARP_MAX_SAMPLES && ref < d.n_refs;
    if (from_array) ok = ok && d.mv_array != nullptr && jp->mv_index < d.n_mvs;
    ok = ok && (uint64_t)jp->src_offset + (uint64_t)(bh > 0 ? bh - 1 : 0) * d.src_stride + (uint64_t)bw <= d.src_samples;
    if (!uniform((int)ok)) { // a scalar branch: the whole workgroup leaves here
        if (threadIdx.x == 0) d.status[job] = SVT_HIP_WARP_UNDEFINED;
        return;
    }
    const int  org_x = jp->blk_org_x, org_y = jp->blk_org_y;
    const int  c = lane & 7, rr = lane >> 3;

    // an MV is one word, as Mv.as_int is: the row in the upper half, the column in the lower
    const int start_r = uniform(from_array ? d.mv_array[2 * (size_t)jp->mv_index] : jp->start_mv[0]);
    const int start_c = uniform(from_array ? d.mv_array[2 * (size_t)jp->mv_index + 1] : jp->start_mv[1]);
    uint32_t  centre = ((uint32_t)start_r << 16) | ((uint32_t)start_c & 0xFFFFu), best = centre, prev = centre;
    int       best_cost = INT32_MAX, tot = 0;
    for (int iter = 0; iter < (int)desc_in_kernarg()->iterations; iter++) {
        const int shift = desc_in_kernarg()->mv_prec_shift, n_pos = desc_in_kernarg()->refine_diag ? 9 : 5;
        for (int i = iter ? 1 : 0; i < n_pos; i++) { // offset (0, 0) in the first round only
            const int      test_r = (int16_t)((int)(int16_t)(centre >> 16) + ((int)kNeighbour[i][0] << shift));
            const int      test_c = (int16_t)((int)(int16_t)(centre & 0xFFFFu) + ((int)kNeighbour[i][1] << shift));
            const uint32_t key    = ((uint32_t)test_r << 16) | ((uint32_t)test_c & 0xFFFFu);
            if (iter) { // positions tested before are not tested again
                if (key == prev) continue;
                bool hit = false;
                for (int e = lane; e < tot; e += 64) hit = hit || s_rec[e] == key;
                if (__ballot(hit) != 0) continue;
            }
            if (threadIdx.x == 0) s_rec[tot] = key; // recorded whether or not its fit is valid
            tot++;
            __syncthreads();
            // The fit's inputs are wave-uniform, and left to itself the compiler runs all of it on the scalar unit and keeps the 32 sample
            // coordinates in scalar registers across the loop, which the loop's own state already fills: handing the MV and the samples' address
            // over in vector registers keeps the fit on the vector unit, one copy per lane.
            int      vec_r = test_r, vec_c = test_c;
            const KernargDesc kd = desc_in_kernarg();
            FitInput vin = {jp->pts, jp->pts_inref, n, bw, bh, org_x, org_y, kd->shut_approx != 0, kd->lower_band_th, kd->upper_band_th};
            asm volatile("" : "+v"(vec_r), "+v"(vec_c), "+v"(vin.pts), "+v"(vin.pts_inref), "+v"(vin.n), "+v"(vin.bw), "+v"(vin.bh), "+v"(vin.org_x),
                         "+v"(vin.org_y)); // n: else eight `i < n` masks stay in scalar pairs; the block: else what the fit derives from it does
            const SvtHipWarpModel fit = fit_model(vin, vec_r, vec_c);
            if (uniform(fit.valid) == 0) continue;
            Model m;
#pragma unroll
            for (int k = 0; k < 6; k++) m.mat[k] = uniform(fit.wmmat[k]);
            m.alpha = uniform(fit.alpha); m.beta = uniform(fit.beta); m.gamma = uniform(fit.gamma); m.delta = uniform(fit.delta);
            const SvtHipWarpRef r          = {kd->refs[ref].plane, kd->refs[ref].stride, kd->refs[ref].org_x, kd->refs[ref].org_y, kd->refs[ref].width,
                                              kd->refs[ref].height, kd->refs[ref].rows, 0};
            const uint8_t      *src        = kd->src + jp->src_offset;
            const uint32_t      src_stride = kd->src_stride;
            const int           log2_tx = 31 - __builtin_clz((unsigned)(bw >> 3)), n_tiles = (bw >> 3) * (bh >> 3);
            uint32_t            sse = 0, sum = 0;
            for (int t = wave; t < n_tiles; t += WAVES) {
                const int ty = t >> log2_tx, tx = t & ((1 << log2_tx) - 1);
                const int v  = clampi(warp_tile<false>(r, m, org_x + 8 * tx, org_y + 8 * ty, 0, 0, 11, s_src[wave], s_mid[wave], lane) - 128 - 256, 0, 255);
                const int df = v - (int)src[(size_t)(8 * ty + rr) * src_stride + (size_t)(8 * tx + c)];
                sum += (uint32_t)df;
                sse += (uint32_t)(df * df);
            }
            sse = wave_sum_dpp(sse);
            sum = wave_sum_dpp(sum);
            if (WAVES > 1) {
                // no wave writes the next test's partial sums before every wave has read these: the barrier behind the record lies between
                if (lane == 0) { s_part[wave][0] = sse; s_part[wave][1] = sum; }
                __syncthreads();
                sse = sum = 0;
#pragma unroll
                for (int w = 0; w < WAVES; w++) { sse += s_part[w][0]; sum += s_part[w][1]; }
            }
            // svt_aom_variance{W}x{H} as an int, plus the MV rate
            const int64_t s64 = (int64_t)(int32_t)sum;
            int cost = (int)(sse - (uint32_t)((s64 * s64) >> (31 - __builtin_clz((unsigned)(bw * bh)))));
            const SvtHipWmRefineJob *jq = jp; // behind a barrier too: the predicted MV is loaded here, not held across the loop
            asm volatile("" : "+s"(jq));
            const SvtHipMv pred_mv = {jq->pred_mv[0], jq->pred_mv[1]};
            int            rate;
            if (kd->approx_inter_rate) {
                rate = mv_err_cost_light(test_r, test_c, pred_mv);
            } else {
                const MvCost mc = {pred_mv, SVT_HIP_MV_COST_ENTROPY, kd->error_per_bit > 0 ? kd->error_per_bit : 1, kd->mvjcost, kd->mvcost[0], kd->mvcost[1]};
                rate = mv_err_cost((int16_t)test_r, (int16_t)test_c, mc);
            }
            cost           = (int)((uint32_t)cost + (uint32_t)rate);
            if (cost < best_cost) { best = key; best_cost = cost; }
        }
        prev   = centre;
        centre = best;
        if (prev == best) break;
    }
    if (threadIdx.x == 0) {
        const KernargDesc kd = desc_in_kernarg();
        uint32_t job = blockIdx.x; // taken again, behind a barrier: else its 64-bit form is held across the search for these four stores
        asm volatile("" : "+s"(job));
        kd->best_mv[2 * (size_t)job] = (int16_t)(best >> 16); kd->best_mv[2 * (size_t)job + 1] = (int16_t)(best & 0xFFFFu);
        kd->best_cost[job] = best_cost;
        kd->n_checked[job] = (uint32_t)tot;
        kd->status[job]    = SVT_HIP_WARP_OK;
    }
}

} // namespace

extern "C" {

int svt_hip_warp_check_desc(const SvtHipWarpPredDesc *d) {
    if (!d) BAD("svt_hip_warp_check_desc: null descriptor");
    if (!d->dst || !d->jobs || !d->status) BAD("svt_hip_warp_check_desc: a mandatory pointer (dst, jobs, status) is null");
    if (d->bit_depth != 8 && d->bit_depth != 10) BAD("svt_hip_warp_check_desc: bit_depth %u (8 or 10)", d->bit_depth);
    if (d->ss_x > 1 || d->ss_y > 1) BAD("svt_hip_warp_check_desc: ss_x %u, ss_y %u (0 or 1)", d->ss_x, d->ss_y);
    if (d->n_refs == 0 || d->n_refs > SVT_HIP_WARP_MAX_REFS) BAD("svt_hip_warp_check_desc: n_refs %u (1 .. %d)", d->n_refs, SVT_HIP_WARP_MAX_REFS);
    const int rc = svt_hip_check_warp_refs("svt_hip_warp_check_desc", "reference", d->refs, d->n_refs);
    if (rc) return rc;
    if (d->dst_stride == 0 || d->dst_samples == 0) BAD("svt_hip_warp_check_desc: dst_stride %u / dst_samples %llu is zero", d->dst_stride, (unsigned long long)d->dst_samples);
    if (d->n_models && !d->models) BAD("svt_hip_warp_check_desc: n_models %u without a model array", d->n_models);
    return SVT_HIP_OK;
}

int svt_hip_wm_refine_check_desc(const SvtHipWmRefineDesc *d) {
    if (!d) BAD("svt_hip_wm_refine_check_desc: null descriptor");
    if (!d->src || !d->jobs || !d->best_mv || !d->best_cost || !d->n_checked || !d->status)
        BAD("svt_hip_wm_refine_check_desc: a mandatory pointer (src, jobs, best_mv, best_cost, n_checked, status) is null");
    if (d->iterations == 0 || d->iterations > SVT_HIP_WM_MAX_ITERATIONS) BAD("svt_hip_wm_refine_check_desc: iterations %u (1 .. %d)", d->iterations, SVT_HIP_WM_MAX_ITERATIONS);
    if (d->mv_prec_shift > 1) BAD("svt_hip_wm_refine_check_desc: mv_prec_shift %u (0 or 1)", d->mv_prec_shift);
    if (d->waves_per_job != 0 && d->waves_per_job != 1 && d->waves_per_job != 4) BAD("svt_hip_wm_refine_check_desc: waves_per_job %u (0, 1 or 4)", d->waves_per_job);
    if (d->n_refs == 0 || d->n_refs > SVT_HIP_WARP_MAX_REFS) BAD("svt_hip_wm_refine_check_desc: n_refs %u (1 .. %d)", d->n_refs, SVT_HIP_WARP_MAX_REFS);
    const int rc = svt_hip_check_warp_refs("svt_hip_wm_refine_check_desc", "reference", d->refs, d->n_refs);
    if (rc) return rc;
    if (d->src_stride == 0 || d->src_samples == 0) BAD("svt_hip_wm_refine_check_desc: src_stride %u / src_samples %llu is zero", d->src_stride, (unsigned long long)d->src_samples);
    if (d->n_mvs && !d->mv_array) BAD("svt_hip_wm_refine_check_desc: n_mvs %u without mv_array", d->n_mvs);
    if (d->error_per_bit < 0) BAD("svt_hip_wm_refine_check_desc: error_per_bit %d is negative", d->error_per_bit);
    if (!d->approx_inter_rate && (!d->mvjcost || !d->mvcost[0] || !d->mvcost[1])) BAD("svt_hip_wm_refine_check_desc: a cost table is null and approx_inter_rate is not set");
    return SVT_HIP_OK;
}

// svt_hip_warp_model_batch has no check_desc entry: what it refuses
static int warp_model_check(const SvtHipWarpModelDesc *d) {
    if (!d->jobs || !d->models || !d->status) BAD("svt_hip_warp_model_batch: a mandatory pointer (jobs, models, status) is null");
    if (d->n_mvs && !d->mv_array) BAD("svt_hip_warp_model_batch: n_mvs %u without mv_array", d->n_mvs);
    return SVT_HIP_OK;
}

size_t svt_hip_warp_layout(int what, int field) {
#define D(f) offsetof(SvtHipWarpPredDesc, f)
#define J(f) offsetof(SvtHipWarpPredJob, f)
#define R(f) offsetof(SvtHipWarpRef, f)
#define M(f) offsetof(SvtHipWarpModel, f)
#define E(f) offsetof(SvtHipWarpModelDesc, f)
#define K(f) offsetof(SvtHipWarpModelJob, f)
    static const size_t desc[]  = {D(bit_depth), D(ss_x), D(ss_y), D(n_refs), D(n_jobs), D(refs), D(dst), D(dst_stride), D(reserved), D(dst_samples), D(jobs),
                                   D(models), D(n_models), D(reserved2), D(status)};
    static const size_t job[]   = {J(dst_offset), J(p_col), J(p_row), J(width), J(height), J(ref), J(flags), J(comp_mode), J(fwd_offset), J(bck_offset),
                                   J(model_index), J(model)};
    static const size_t ref[]   = {R(plane), R(stride), R(org_x), R(org_y), R(width), R(height), R(rows), R(reserved)};
    static const size_t model[] = {M(wmmat), M(alpha), M(beta), M(gamma), M(delta), M(wmtype), M(valid), M(num_samples), M(reserved)};
    static const size_t mdesc[] = {E(n_jobs), E(shut_approx), E(reserved), E(lower_band_th), E(upper_band_th), E(reserved2), E(n_mvs), E(jobs), E(mv_array),
                                   E(models), E(status)};
    static const size_t mjob[]  = {K(pts), K(pts_inref), K(blk_org_x), K(blk_org_y), K(bwidth), K(bheight), K(n_samples), K(flags), K(mv), K(mv_index)};
#define F(f) offsetof(SvtHipWmRefineDesc, f)
#define G(f) offsetof(SvtHipWmRefineJob, f)
    static const size_t rdesc[] = {F(n_jobs), F(iterations), F(refine_diag), F(mv_prec_shift), F(shut_approx), F(lower_band_th), F(upper_band_th), F(approx_inter_rate),
                                   F(n_refs), F(waves_per_job), F(reserved), F(error_per_bit), F(src_stride), F(src), F(src_samples), F(refs), F(jobs), F(mv_array),
                                   F(n_mvs), F(reserved2), F(mvjcost), F(mvcost), F(best_mv), F(best_cost), F(n_checked), F(status)};
    static const size_t rjob[]  = {G(pts), G(pts_inref), G(src_offset), G(blk_org_x), G(blk_org_y), G(bwidth), G(bheight), G(n_samples), G(flags), G(start_mv),
                                   G(pred_mv), G(mv_index), G(ref), G(reserved)};
#undef D
#undef J
#undef R
#undef M
#undef E
#undef K
#undef F
#undef G
    const SvtHipLayoutRow rows[] = {layout_row<SvtHipWarpPredDesc>(desc),   layout_row<SvtHipWarpPredJob>(job),   layout_row<SvtHipWarpRef>(ref),
                                    layout_row<SvtHipWarpModel>(model),     layout_row<SvtHipWarpModelDesc>(mdesc), layout_row<SvtHipWarpModelJob>(mjob),
                                    layout_row<SvtHipWmRefineDesc>(rdesc), layout_row<SvtHipWmRefineJob>(rjob)};
    return layout_lookup(rows, what, field);
}

const int16_t  *svt_hip_warp_filter_table(void) { return &kTablesHost.filter[0][0]; }
const uint16_t *svt_hip_warp_div_lut(void) { return kTablesHost.div_lut; }

int svt_hip_warp_pred_batch(SvtHipContext *ctx, const SvtHipWarpPredDesc *d) {
    return enqueue_batch("svt_hip_warp_pred_batch", ctx, d, svt_hip_warp_check_desc, &SvtHipWarpPredDesc::n_jobs, [=] {
        hipLaunchKernelGGL(pick_hbd(d->bit_depth, warp_pred_kernel<true>, warp_pred_kernel<false>), dim3(d->n_jobs), dim3(64 * kWaves), 0, ctx->stream, *d);
    });
}

int svt_hip_warp_model_batch(SvtHipContext *ctx, const SvtHipWarpModelDesc *d) {
    return enqueue_batch("svt_hip_warp_model_batch", ctx, d, warp_model_check, &SvtHipWarpModelDesc::n_jobs,
                         [=] { hipLaunchKernelGGL(warp_model_kernel, dim3(ceil_div(d->n_jobs, 64)), dim3(64), 0, ctx->stream, *d); });
}

int svt_hip_wm_refine_batch(SvtHipContext *ctx, const SvtHipWmRefineDesc *d) {
    return enqueue_batch("svt_hip_wm_refine_batch", ctx, d, svt_hip_wm_refine_check_desc, &SvtHipWmRefineDesc::n_jobs, [=] {
        if (d->waves_per_job == 1) hipLaunchKernelGGL(wm_refine_kernel<1>, dim3(d->n_jobs), dim3(64), 0, ctx->stream, *d);
        else hipLaunchKernelGGL(wm_refine_kernel<kWaves>, dim3(d->n_jobs), dim3(64 * kWaves), 0, ctx->stream, *d);
    });
}

} // extern "C"
