// cfl_kernel.hip -- chroma-from-luma on gfx950: svt_hip_cfl_pred_batch, which writes the predictions of every requested alpha of a chroma block
// into the plane svt_hip_rd_batch reads, and svt_hip_cfl_pick_alpha_batch, which replays the alpha search over the resulting costs.
//
// Reference functions restated (Source/Lib):
//   compute_cfl_ac_components, av1_cost_calc_cfl (the prediction calls), md_cfl_rd_pick_alpha   Codec/product_coding_loop.c:3751-3786, 3453-3617, 3624-3748
//   svt_cfl_luma_subsampling_420_lbd_c / _hbd_c, svt_subtract_average_c                         Codec/intra_prediction.c:420-465
//   svt_cfl_predict_lbd_c / _hbd_c, get_scaled_luma_q0                                          C_DEFAULT/cfl_c.c, Codec/intra_prediction.h
//   cfl_idx_to_alpha, PLANE_SIGN_TO_JOINT_SIGN, RDCOST, MAX_MODE_COST                           Codec/intra_prediction.h:137-143, product_coding_loop.c:3619, rd_cost.h:37
//
// Lay-out of the prediction: the block size is the batch's, so the lanes map statically.  A lane owns runs of four chroma samples of one row:
// two 8-byte (8-bit) or 16-byte (10-bit) luma loads, exactly the 8 x 2 samples under them.  A block of W * H / 4 runs takes that many lanes, so
// 16 4x4 jobs share a wave, a 16x16 job is one wave, and a 32x32 job gives every lane four runs.  The sum meets by a reduction over the
// job's lanes (wave_ops.h); the AC stays in registers, there is no LDS.  The DC runs of both planes are loaded before the first store; the alpha
// loop is wave-uniform, alpha in a scalar register.  Nothing returns early: an undefined job's lanes and the lanes behind the last job run
// predicated, so the reductions see a whole wave.  The kernel is bound by its stores, 2 * n_alpha * W * H samples per job.
//
// The alpha search is one lane per block: the loops over plane, sign and the paired sign are unrolled, so best_rd_uv[8][2] and best_c[8][2] are
// registers; the loop over the magnitude c stays a loop, because its break is the point of it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include "batch_host.h"
#include "../../include/svt_hip_cfl.h"
#include "wave_ops.h"

namespace {

constexpr int kWaves = 4;

template <int N> struct Log2 { static constexpr int v = 1 + Log2<N / 2>::v; };
template <> struct Log2<1> { static constexpr int v = 0; };

// the sum over the G consecutive lanes of a job, in all of them (G == 64: a scalar)
template <int G> __device__ __forceinline__ uint32_t job_sum(uint32_t v) {
    if constexpr (G == 64) return wave_sum_dpp(v);
    else if constexpr (G == 4) return quad_sum(v);
    else if constexpr (G == 8) return oct_sum(v);
    else return group_sum<G>(v);
}

template <bool HBD, int W, int H> __global__ __launch_bounds__(64 * kWaves) void cfl_pred_kernel(const SvtHipCflPredDesc d) {
    using Px = typename std::conditional<HBD, uint16_t, uint8_t>::type;
    constexpr int px_max = HBD ? 1023 : 255;
    constexpr int kRuns  = W * H / 4;                 // of four chroma samples
    constexpr int LPJ    = kRuns < 64 ? kRuns : 64;   // lanes per job
    constexpr int R      = kRuns / LPJ;               // runs per lane
    constexpr int JPW    = 64 / LPJ;                  // jobs per wave
    constexpr int RPR    = W / 4;                     // runs per row
    const int      lane = (int)(threadIdx.x & 63u);
    const uint32_t wave = blockIdx.x * (uint32_t)kWaves + (threadIdx.x >> 6);
    const uint32_t job  = wave * (uint32_t)JPW + (uint32_t)(lane / LPJ);
    const int      sub  = lane % LPJ;
    const bool     have = job < d.n_jobs;

    SvtHipCflPredJob j;
    memset(&j, 0, sizeof(j));
    if (have) j = d.jobs[job];
    bool ok = have && j.luma_x >= 0 && j.luma_y >= 0 && (uint64_t)j.luma_x + 2 * W <= d.luma_width && (uint64_t)j.luma_y + 2 * H <= d.luma_height;
#pragma unroll
    for (int p = 0; p < 2; p++) {
        ok = ok && (uint64_t)j.dc_offset[p] + (uint64_t)(H - 1) * d.plane[p].dc_stride + W <= d.plane[p].dc_samples;
        ok = ok && (uint64_t)j.dst_offset[p] + (uint64_t)(d.n_alpha - 1) * d.slot_stride + (uint64_t)(H - 1) * d.plane[p].dst_stride + W <= d.plane[p].dst_samples;
    }

    // the sub-sampled luma of the lane's runs: q3 = (a + b + c + d) << 1
    int      q3[R][4];
    uint32_t sum = 0;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int q = r * LPJ + sub, row = q / RPR, col = (q % RPR) * 4;
        int a[8], b[8];
#pragma unroll
        for (int i = 0; i < 8; i++) a[i] = b[i] = 0;
        if (ok) { // inside the job's extent, which is inside the plane
            const Px *p0 = (const Px *)d.luma + ((size_t)j.luma_y + 2 * (size_t)row) * d.luma_stride + (size_t)j.luma_x + 2 * (size_t)col;
            const Px *p1 = p0 + d.luma_stride;
            if (HBD) {
                if ((((uintptr_t)p0 | (uintptr_t)p1) & 15u) == 0) {
                    const uint4 u = *(const uint4 *)p0, v = *(const uint4 *)p1;
                    const uint32_t uu[4] = {u.x, u.y, u.z, u.w}, vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        a[2 * i] = (int)(uu[i] & 0xFFFFu); a[2 * i + 1] = (int)(uu[i] >> 16);
                        b[2 * i] = (int)(vv[i] & 0xFFFFu); b[2 * i + 1] = (int)(vv[i] >> 16);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 8; i++) { a[i] = p0[i]; b[i] = p1[i]; }
                }
            } else {
                if ((((uintptr_t)p0 | (uintptr_t)p1) & 7u) == 0) {
                    const uint2 u = *(const uint2 *)p0, v = *(const uint2 *)p1;
                    const uint32_t uu[2] = {u.x, u.y}, vv[2] = {v.x, v.y};
#pragma unroll
                    for (int i = 0; i < 8; i++) {
                        a[i] = (int)((uu[i >> 2] >> (8 * (i & 3))) & 0xFFu);
                        b[i] = (int)((vv[i >> 2] >> (8 * (i & 3))) & 0xFFu);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 8; i++) { a[i] = p0[i]; b[i] = p1[i]; }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            q3[r][i] = (a[2 * i] + a[2 * i + 1] + b[2 * i] + b[2 * i + 1]) << 1;
            sum += (uint32_t)q3[r][i];
        }
    }
    // svt_subtract_average: at most 32 * 32 * 8184 in the sum
    const int avg = (int)(int16_t)((job_sum<LPJ>(sum) + (uint32_t)((W * H) >> 1)) >> (Log2<W>::v + Log2<H>::v));

    if (ok) {
        int ac[R][4], dc[2][R][4];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int q = r * LPJ + sub, row = q / RPR, col = (q % RPR) * 4;
#pragma unroll
            for (int i = 0; i < 4; i++) ac[r][i] = (int)(int16_t)(q3[r][i] - avg);
            if (d.ac) { // dense, 8-byte aligned: the descriptor check
                int16_t *o = d.ac + (size_t)job * (W * H) + (size_t)row * W + (size_t)col;
                *(uint2 *)o = make_uint2(((uint32_t)ac[r][0] & 0xFFFFu) | ((uint32_t)ac[r][1] << 16), ((uint32_t)ac[r][2] & 0xFFFFu) | ((uint32_t)ac[r][3] << 16));
            }
#pragma unroll
            for (int p = 0; p < 2; p++) {
                const Px *s = (const Px *)d.plane[p].dc + (size_t)j.dc_offset[p] + (size_t)row * d.plane[p].dc_stride + (size_t)col;
                if (HBD && ((uintptr_t)s & 7u) == 0) {
                    const uint2 u = *(const uint2 *)s;
                    dc[p][r][0] = (int)(u.x & 0xFFFFu); dc[p][r][1] = (int)(u.x >> 16); dc[p][r][2] = (int)(u.y & 0xFFFFu); dc[p][r][3] = (int)(u.y >> 16);
                } else if (!HBD && ((uintptr_t)s & 3u) == 0) {
                    const uint32_t u = *(const uint32_t *)s;
                    dc[p][r][0] = (int)(u & 0xFFu); dc[p][r][1] = (int)((u >> 8) & 0xFFu); dc[p][r][2] = (int)((u >> 16) & 0xFFu); dc[p][r][3] = (int)(u >> 24);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++) dc[p][r][i] = s[i];
                }
            }
        }
        // every DC run is in registers: the stores begin
        const int n_alpha = d.n_alpha;
        for (int k = 0; k < n_alpha; k++) {
            const int alpha = __builtin_amdgcn_readfirstlane((int)d.alpha_q3[k]); // wave-uniform: the multiplies take it from a scalar register
#pragma unroll
            for (int p = 0; p < 2; p++) {
                Px *const slot = (Px *)d.plane[p].dst + (size_t)j.dst_offset[p] + (size_t)k * d.slot_stride;
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int q = r * LPJ + sub, row = q / RPR, col = (q % RPR) * 4;
                    uint32_t out[4];
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int t = alpha * ac[r][i];
                        const int s = t < 0 ? -((-t + 32) >> 6) : (t + 32) >> 6; // ROUND_POWER_OF_TWO_SIGNED(t, 6)
                        const int v = s + dc[p][r][i];
                        out[i] = (uint32_t)(v < 0 ? 0 : (v > px_max ? px_max : v));
                    }
                    Px *o = slot + (size_t)row * d.plane[p].dst_stride + (size_t)col;
                    if (HBD) {
                        if (((uintptr_t)o & 7u) == 0) *(uint2 *)o = make_uint2(out[0] | (out[1] << 16), out[2] | (out[3] << 16));
                        else { o[0] = (Px)out[0]; o[1] = (Px)out[1]; o[2] = (Px)out[2]; o[3] = (Px)out[3]; }
                    } else {
                        if (((uintptr_t)o & 3u) == 0) *(uint32_t *)o = out[0] | (out[1] << 8) | (out[2] << 16) | (out[3] << 24);
                        else { o[0] = (Px)out[0]; o[1] = (Px)out[1]; o[2] = (Px)out[2]; o[3] = (Px)out[3]; }
                    }
                }
            }
        }
    }
    if (have && sub == 0) d.status[job] = ok ? SVT_HIP_CFL_OK : SVT_HIP_CFL_UNDEFINED;
}

template <bool HBD, int W, int H> void launch_pred(SvtHipContext *ctx, const SvtHipCflPredDesc &d) {
    constexpr int      runs = W * H / 4, jpw = runs < 64 ? 64 / runs : 1;
    const uint32_t waves = (d.n_jobs + (uint32_t)jpw - 1) / (uint32_t)jpw, grid = (waves + (uint32_t)kWaves - 1) / (uint32_t)kWaves;
    hipLaunchKernelGGL((cfl_pred_kernel<HBD, W, H>), dim3(grid), dim3(64 * kWaves), 0, ctx->stream, d);
}
template <bool HBD, int W> void launch_pred_h(SvtHipContext *ctx, const SvtHipCflPredDesc &d) {
    switch (d.height) {
    case 4: launch_pred<HBD, W, 4>(ctx, d); break;
    case 8: launch_pred<HBD, W, 8>(ctx, d); break;
    case 16: launch_pred<HBD, W, 16>(ctx, d); break;
    default: launch_pred<HBD, W, 32>(ctx, d); break;
    }
}
template <bool HBD> void launch_pred_w(SvtHipContext *ctx, const SvtHipCflPredDesc &d) {
    switch (d.width) {
    case 4: launch_pred_h<HBD, 4>(ctx, d); break;
    case 8: launch_pred_h<HBD, 8>(ctx, d); break;
    case 16: launch_pred_h<HBD, 16>(ctx, d); break;
    default: launch_pred_h<HBD, 32>(ctx, d); break;
    }
}

// ---- the alpha search ----
constexpr uint64_t kMaxModeCost = SVT_HIP_CFL_MAX_MODE_COST;

// RDCOST(RM, R, D)
__device__ __forceinline__ uint64_t rdcost(uint32_t lambda, uint64_t rate, uint64_t dist) {
    return (uint64_t)((((int64_t)rate * (int64_t)lambda + 256) >> 9) + ((int64_t)dist * 128));
}
// PLANE_SIGN_TO_JOINT_SIGN(plane, a, b)
__device__ __forceinline__ constexpr int joint_sign(int plane, int a, int b) { return plane == 0 ? a * 3 + b - 1 : b * 3 + a - 1; }

__global__ __launch_bounds__(64) void cfl_pick_alpha_kernel(const SvtHipCflPickDesc d) {
    const uint32_t b = blockIdx.x * 64u + threadIdx.x;
    if (b >= d.n_blocks) return;
    const uint32_t  stride = d.dist_stride ? d.dist_stride : 1u;
    const size_t    base   = (size_t)b * 2 * SVT_HIP_CFL_SLOTS;
    const uint32_t  lambda = d.lambda;
    const int       itr_th = d.itr_th, n_mag = d.n_mag;
    const int32_t  *fac    = d.alpha_fac_bits;
    const uint64_t  mode_rd = rdcost(lambda, (uint64_t)(int64_t)d.mode_bits[b], 0);

    uint64_t best_uv[8][2];
    int      best_c[8][2];
    bool     undef = false, trunc = false;
#pragma unroll
    for (int plane = 0; plane < 2; plane++) {
#pragma unroll
        for (int js = 0; js < 8; js++) { best_uv[js][plane] = kMaxModeCost; best_c[js][plane] = 0; }
        // alpha zero in this plane: CFL_SIGN_NEG and CFL_SIGN_POS in the other
        const uint64_t bits = d.bits[base + plane * SVT_HIP_CFL_SLOTS + 16], dist = d.dist[(base + plane * SVT_HIP_CFL_SLOTS + 16) * stride];
        undef = undef || bits == UINT64_MAX;
        constexpr int kNeg = 1, kPos = 2;
        const int     js_neg = joint_sign(plane, 0, kNeg), js_pos = joint_sign(plane, 0, kPos);
        best_uv[js_neg][plane] = rdcost(lambda, bits + (uint64_t)(int64_t)fac[(js_neg * 2 + plane) * 16], dist);
        best_uv[js_pos][plane] = rdcost(lambda, bits + (uint64_t)(int64_t)fac[(js_pos * 2 + plane) * 16], dist);
    }

    uint64_t best_rd = kMaxModeCost;
    int      best_js = 0;
#pragma unroll
    for (int plane = 0; plane < 2; plane++) {
#pragma unroll
        for (int pn = 1; pn < 3; pn++) { // CFL_SIGN_NEG, CFL_SIGN_POS
            uint8_t progress = 0;
            for (int c = 0; c < 16; c++) {
                if (c > itr_th && (int)progress < c) break;
                if (c >= n_mag) { trunc = true; break; } // the reference would evaluate an alpha the table does not hold
                const size_t   at   = base + plane * SVT_HIP_CFL_SLOTS + (pn == 1 ? 15 - c : 17 + c);
                const uint64_t bits = d.bits[at], dist = d.dist[at * stride];
                undef = undef || bits == UINT64_MAX;
                uint8_t flag = 0;
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    const int js      = joint_sign(plane, pn, i);
                    uint64_t  this_rd = rdcost(lambda, bits + (uint64_t)(int64_t)fac[(js * 2 + plane) * 16 + c], dist);
                    if (this_rd < best_uv[js][plane]) {
                        best_uv[js][plane] = this_rd;
                        best_c[js][plane]  = c;
                        flag               = (uint8_t)itr_th;
                        if (best_uv[js][1 - plane] != kMaxModeCost) {
                            this_rd += mode_rd + best_uv[js][1 - plane];
                            if (this_rd < best_rd) { best_rd = this_rd; best_js = js; }
                        }
                    }
                }
                progress = (uint8_t)(progress + flag);
            }
        }
    }

    int ind = 0;
#pragma unroll
    for (int js = 0; js < 8; js++)
        if (js == best_js) ind = (best_c[js][0] << 4) + best_c[js][1];
    const bool found = !undef && best_rd != kMaxModeCost;
    d.best_rd[b]         = found ? best_rd : kMaxModeCost;
    d.cfl_alpha_idx[b]   = (uint8_t)(found ? ind : 0);
    d.cfl_alpha_signs[b] = (uint8_t)(found ? best_js : 0);
    d.status[b]          = undef ? SVT_HIP_CFL_PICK_UNDEFINED : (trunc ? SVT_HIP_CFL_PICK_TRUNCATED : 0);
}

} // namespace

extern "C" {

int svt_hip_cfl_pred_check_desc(const SvtHipCflPredDesc *d) {
    if (!d) BAD("svt_hip_cfl_pred_check_desc: null descriptor");
    if (!d->luma || !d->jobs || !d->status || !d->plane[0].dc || !d->plane[0].dst || !d->plane[1].dc || !d->plane[1].dst)
        BAD("svt_hip_cfl_pred_check_desc: a mandatory pointer (luma, jobs, status, a plane's dc or dst) is null");
    if (d->bit_depth != 8 && d->bit_depth != 10) BAD("svt_hip_cfl_pred_check_desc: bit_depth %u (8 or 10)", d->bit_depth);
    for (int k = 0; k < 2; k++) {
        const unsigned s = k ? d->height : d->width;
        if (s != 4 && s != 8 && s != 16 && s != 32) BAD("svt_hip_cfl_pred_check_desc: chroma block %u x %u (each side 4, 8, 16 or 32)", d->width, d->height);
    }
    if (d->n_alpha == 0 || d->n_alpha > SVT_HIP_CFL_SLOTS) BAD("svt_hip_cfl_pred_check_desc: n_alpha %u (1 .. %d)", d->n_alpha, SVT_HIP_CFL_SLOTS);
    for (int k = 0; k < d->n_alpha; k++)
        if (d->alpha_q3[k] < -16 || d->alpha_q3[k] > 16) BAD("svt_hip_cfl_pred_check_desc: alpha_q3[%d] = %d (-16 .. 16)", k, d->alpha_q3[k]);
    if (d->luma_stride == 0 || d->luma_width == 0 || d->luma_height == 0 || d->luma_stride < d->luma_width)
        BAD("svt_hip_cfl_pred_check_desc: luma plane stride %u, size %u x %u (stride and size non-zero, stride >= width)", d->luma_stride, d->luma_width,
            d->luma_height);
    if (d->slot_stride == 0) BAD("svt_hip_cfl_pred_check_desc: slot_stride is zero");
    if (d->ac && ((uintptr_t)d->ac & 7u)) BAD("svt_hip_cfl_pred_check_desc: ac is not 8-byte aligned");
    const uint64_t px = d->bit_depth > 8 ? 2 : 1;
    const uint64_t l0 = (uint64_t)(uintptr_t)d->luma, l1 = l0 + ((uint64_t)(d->luma_height - 1) * d->luma_stride + d->luma_width) * px;
    for (int p = 0; p < 2; p++) {
        const SvtHipCflPlane *pl = &d->plane[p];
        if (pl->dc_stride == 0 || pl->dst_stride == 0 || pl->dc_samples == 0 || pl->dst_samples == 0)
            BAD("svt_hip_cfl_pred_check_desc: plane %d: dc_stride %u / dst_stride %u / dc_samples %llu / dst_samples %llu is zero", p, pl->dc_stride, pl->dst_stride,
                (unsigned long long)pl->dc_samples, (unsigned long long)pl->dst_samples);
    }
    for (int p = 0; p < 2; p++) {
        const uint64_t d0 = (uint64_t)(uintptr_t)d->plane[p].dst, d1 = d0 + d->plane[p].dst_samples * px;
        if (d0 < l1 && l0 < d1) BAD("svt_hip_cfl_pred_check_desc: plane %d's destination range overlaps the luma plane (a batch must not read what it writes)", p);
        for (int q = 0; q < 2; q++) {
            const uint64_t c0 = (uint64_t)(uintptr_t)d->plane[q].dc, c1 = c0 + d->plane[q].dc_samples * px;
            if (d0 < c1 && c0 < d1)
                BAD("svt_hip_cfl_pred_check_desc: plane %d's destination range overlaps plane %d's DC plane (a batch must not read what it writes)", p, q);
        }
    }
    return SVT_HIP_OK;
}

// svt_hip_cfl_pick_alpha_batch has no check_desc entry: what it refuses
static int cfl_pick_alpha_check(const SvtHipCflPickDesc *d) {
    if (!d->bits || !d->dist || !d->mode_bits || !d->alpha_fac_bits || !d->best_rd || !d->cfl_alpha_idx || !d->cfl_alpha_signs || !d->status)
        BAD("svt_hip_cfl_pick_alpha_batch: a mandatory pointer is null");
    if (d->itr_th > 16 || d->n_mag == 0 || d->n_mag > 16) BAD("svt_hip_cfl_pick_alpha_batch: itr_th %u (0 .. 16), n_mag %u (1 .. 16)", d->itr_th, d->n_mag);
    return SVT_HIP_OK;
}

size_t svt_hip_cfl_layout(int what, int field) {
#define D(f) offsetof(SvtHipCflPredDesc, f)
#define J(f) offsetof(SvtHipCflPredJob, f)
#define P(f) offsetof(SvtHipCflPlane, f)
#define K(f) offsetof(SvtHipCflPickDesc, f)
    static const size_t desc[]  = {D(bit_depth), D(width), D(height), D(n_alpha), D(n_jobs), D(alpha_q3), D(reserved), D(luma), D(luma_stride), D(luma_width),
                                   D(luma_height), D(slot_stride), D(plane), D(jobs), D(status), D(ac)};
    static const size_t job[]   = {J(luma_x), J(luma_y), J(dc_offset), J(dst_offset)};
    static const size_t plane[] = {P(dc), P(dc_stride), P(dst_stride), P(dc_samples), P(dst), P(dst_samples)};
    static const size_t pick[]  = {K(n_blocks), K(lambda), K(itr_th), K(n_mag), K(reserved), K(dist_stride), K(bits), K(dist), K(mode_bits), K(alpha_fac_bits),
                                   K(best_rd), K(cfl_alpha_idx), K(cfl_alpha_signs), K(status)};
#undef D
#undef J
#undef P
#undef K
    const SvtHipLayoutRow rows[] = {layout_row<SvtHipCflPredDesc>(desc), layout_row<SvtHipCflPredJob>(job), layout_row<SvtHipCflPlane>(plane),
                                    layout_row<SvtHipCflPickDesc>(pick)};
    return layout_lookup(rows, what, field);
}

int svt_hip_cfl_pred_batch(SvtHipContext *ctx, const SvtHipCflPredDesc *d) {
    return enqueue_batch("svt_hip_cfl_pred_batch", ctx, d, svt_hip_cfl_pred_check_desc, &SvtHipCflPredDesc::n_jobs, [=] {
        if (d->bit_depth == 10) launch_pred_w<true>(ctx, *d);
        else launch_pred_w<false>(ctx, *d);
    });
}

int svt_hip_cfl_pick_alpha_batch(SvtHipContext *ctx, const SvtHipCflPickDesc *d) {
    return enqueue_batch("svt_hip_cfl_pick_alpha_batch", ctx, d, cfl_pick_alpha_check, &SvtHipCflPickDesc::n_blocks,
                         [=] { hipLaunchKernelGGL(cfl_pick_alpha_kernel, dim3(ceil_div(d->n_blocks, 64)), dim3(64), 0, ctx->stream, *d); });
}

} // extern "C"
