// inter_pred_kernel.hip -- sub-pel inter prediction, single and compound, on gfx950: svt_hip_inter_pred_batch, the step between the motion
// searches (svt_hip_md_subpel_batch's best_mv) and the prediction plane svt_hip_rd_batch reads.
//
// Reference functions restated (Source/Lib):
//   svt_aom_enc_make_inter_predictor, unscaled / non-masked / packed 16-bit path       Codec/enc_inter_prediction.c:3274-3391
//   compute_subpel_params (unscaled branch), clamp_mv_to_umv_border_sb, clamp_mv        Codec/enc_inter_prediction.c:3200-3211,30-50, Codec/inter_prediction.h:90-93
//   av1_get_convolve_filter_params, av1_get_interp_filter_params_with_block_size        Codec/inter_prediction.h:137-153
//   sub_pel_filters_8 / _4 / _8sharp / _8smooth / _4smooth, bilinear_filters             Codec/inter_prediction.c:223-254,1065-1129
//   svt_inter_predictor / svt_highbd_inter_predictor's dispatch                          Codec/inter_prediction.c:1308-1435
//   svt_av1_convolve_{2d_copy,x,y,2d}_sr_c, svt_av1_highbd_convolve_*_sr_c               Codec/inter_prediction.c:311-418,670-777
//   svt_av1_jnt_convolve_{2d_copy,x,y,2d}_c, svt_av1_highbd_jnt_convolve_*_c             Codec/inter_prediction.c:494-668,852-1035
//   get_conv_params_no_round (round_0 = 3; round_1 = 11 single, 7 compound)              Codec/convolve.h:40-64
//   quant_dist_lookup_table                                                              Codec/inter_prediction.c:268-271
// Every InterpFilterParams has taps = 8 (the 4-tap tables are 8 wide with zero ends), so fo_horiz = fo_vert = 3 throughout.
//
// Lay-out: one wave per job, four jobs per workgroup, no workgroup barrier.  The wave walks the block in tiles of up to 64 quads (four
// horizontally adjacent samples): 4 x h, 8 x min(h, 32) or 16 x 16, one quad per lane.  Per reference the variant (copy / x / y / 2d), the
// taps and the rounding are wave-uniform: they live in scalar registers and the branches are per job, never per lane.
//   copy   the lane loads its four samples straight from the plane
//   x, y   the tile's source window (tile + 7 columns or rows) is staged in the wave's LDS slice, every coordinate clamped to the padded
//          plane; a lane filters its quad from 12 (x) or 8 x 4 (y) staged samples, read 8 bytes at a time
//   2d     the window is tile + 7 both ways; the horizontal pass writes the (rows + 7) x width int16 intermediate to a second LDS slice,
//          a quad per step, and the vertical pass reads a lane's 8 x 4 of it
// A compound job runs both references per tile; the first one's CONV_BUF_TYPE results stay in four registers of the lane.  Stores are
// plain vector stores: 4 (8-bit) or 8 (10-bit) bytes per lane where the address allows, single samples otherwise.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include "batch_host.h"
#include "../../include/svt_hip_pred.h"
#include "wave_ops.h"
#include "convolve_core.h"

namespace {

constexpr int kWaves  = 4;

template <bool HBD> __global__ __launch_bounds__(64 * kWaves) void inter_pred_kernel(const SvtHipInterPredDesc d) {
    using Px = typename std::conditional<HBD, uint16_t, uint8_t>::type;
    __shared__ __attribute__((aligned(16))) uint16_t s_win[kWaves][kWinU16];
    __shared__ __attribute__((aligned(16))) int16_t  s_mid[kWaves][kMidU16];
    constexpr int bd = HBD ? 10 : 8, px_max = (1 << bd) - 1;
    const int      lane = (int)(threadIdx.x & 63u);
    const int      wave = uniform((int)(threadIdx.x >> 6));
    const uint32_t job  = blockIdx.x * (uint32_t)kWaves + (uint32_t)wave;
    if (job >= d.n_jobs) return;
    const SvtHipInterPredJob j = d.jobs[job];
    const int  w = j.width, h = j.height;
    const bool comp  = j.ref[1] != SVT_HIP_INTER_PRED_NO_REF;
    const int  nrefs = comp ? 2 : 1;

    bool ok = is_block_size(w, h) && j.filter_x <= 3 && j.filter_y <= 3 && j.ref[0] < d.n_refs;
    if (comp) {
        ok = ok && j.ref[1] < d.n_refs && j.comp_mode <= 1;
        if (j.comp_mode == 1) { // quant_dist_lookup_table: {9,7} {11,5} {12,4} {13,3} and their mirrors
            const int f = j.fwd_offset, b = j.bck_offset;
            ok = ok && f + b == 16 && (f == 9 || f == 11 || f == 12 || f == 13 || f == 7 || f == 5 || f == 4 || f == 3);
        }
    }
    if (j.flags & SVT_HIP_INTER_PRED_MV0_FROM_ARRAY) ok = ok && d.mv_array != nullptr && j.mv_index[0] < d.n_mvs;
    if (comp && (j.flags & SVT_HIP_INTER_PRED_MV1_FROM_ARRAY)) ok = ok && d.mv_array != nullptr && j.mv_index[1] < d.n_mvs;
    ok = ok && (uint64_t)j.dst_offset + (uint64_t)(h > 0 ? h - 1 : 0) * d.dst_stride + (uint64_t)w <= d.dst_samples;
    if (!ok) {
        if (lane == 0) d.status[job] = SVT_HIP_INTER_PRED_UNDEFINED;
        return;
    }

    RefView rv0, rv1;
    {
        const int mi0 = (int)j.mv_index[0], mi1 = (int)j.mv_index[1];
        int mvr0 = j.mv[0][0], mvc0 = j.mv[0][1], mvr1 = j.mv[1][0], mvc1 = j.mv[1][1];
        if (j.flags & SVT_HIP_INTER_PRED_MV0_FROM_ARRAY) { mvr0 = d.mv_array[2 * (size_t)mi0]; mvc0 = d.mv_array[2 * (size_t)mi0 + 1]; }
        if (comp && (j.flags & SVT_HIP_INTER_PRED_MV1_FROM_ARRAY)) { mvr1 = d.mv_array[2 * (size_t)mi1]; mvc1 = d.mv_array[2 * (size_t)mi1 + 1]; }
        rv0 = ref_view(d, j, d.refs[j.ref[0]], uniform(mvr0), uniform(mvc0));
        rv1 = comp ? ref_view(d, j, d.refs[j.ref[1]], uniform(mvr1), uniform(mvc1)) : rv0;
    }
    const int tabx = filter_table(j.filter_x, w), taby = filter_table(j.filter_y, h);

    const int  TW = w < 16 ? w : 16, qpr = TW >> 2, qsh = qpr == 1 ? 0 : (qpr == 2 ? 1 : 2);
    const int  TH = h < (256 / TW) ? h : (256 / TW);
    const bool active = lane < qpr * TH;
    const int  qy = lane >> qsh, qx = (lane & (qpr - 1)) << 2;
    uint16_t  *win = s_win[wave];
    int16_t   *mid = s_mid[wave];
    // compound: ConvolveParams.round_1 = 7, round_offset = (1 << (offset_bits - 7)) + (1 << (offset_bits - 8)), offset_bits = bd + 11
    constexpr int ro = (1 << (bd + 4)) + (1 << (bd + 3));
    Px *const dst = (Px *)d.dst;

    for (int ty = 0; ty < h; ty += TH)
        for (int tx = 0; tx < w; tx += TW) {
            int acc[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0};
#pragma unroll 1
            for (int k = 0; k < nrefs; k++) {
                const RefView r = k ? rv1 : rv0;
                const int bx = r.pos_x + tx, by = r.pos_y + ty;
                const bool fx = r.sx != 0, fy = r.sy != 0;
                int res[4] = {0, 0, 0, 0}; // single: the sample; compound: the function's `res`
                if (!fx && !fy) { // svt_av1_convolve_2d_copy_sr_c / svt_av1_jnt_convolve_2d_copy_c
                    if (active)
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const int s = sample<Px>(r, bx + qx + i, by + qy);
                            res[i] = comp ? (int)(uint16_t)((uint16_t)(s << 4) + (uint16_t)ro) : s;
                        }
                } else {
                    const int ws = TW + 8, mx = fx ? 3 : 0, my = fy ? 3 : 0;
                    wave_sync(); // the previous reads of win are done
                    stage<Px>(win, r, bx - mx, by - my, TW + (fx ? 7 : 0), TH + (fy ? 7 : 0), ws, lane);
                    wave_sync();
                    int tx8[8], ty8[8];
#pragma unroll
                    for (int t = 0; t < 8; t++) { tx8[t] = c_interp[tabx][r.sx][t]; ty8[t] = c_interp[taby][r.sy][t]; }
                    if (fx && fy) { // the horizontal pass of *_2d_*: im_block, (TH + 7) rows
                        const int units = (TH + 7) << qsh;
                        for (int u = lane; u < units; u += 64) {
                            const int rr = u >> qsh, cc = (u & (qpr - 1)) << 2;
                            int in[12];
                            load4u(win + rr * ws + cc, in); load4u(win + rr * ws + cc + 4, in + 4); load4u(win + rr * ws + cc + 8, in + 8);
                            uint32_t o[4];
#pragma unroll
                            for (int i = 0; i < 4; i++) {
                                int sum = 1 << (bd + 6);
#pragma unroll
                                for (int t = 0; t < 8; t++) sum += tx8[t] * in[i + t];
                                o[i] = (uint32_t)(uint16_t)(int16_t)((sum + 4) >> 3);
                            }
                            *(uint2 *)(mid + rr * TW + cc) = make_uint2(o[0] | (o[1] << 16), o[2] | (o[3] << 16));
                        }
                        wave_sync();
                        if (active) {
                            int sum[4];
#pragma unroll
                            for (int i = 0; i < 4; i++) sum[i] = 1 << (bd + 11);
#pragma unroll
                            for (int t = 0; t < 8; t++) {
                                int v[4];
                                load4s(mid + (qy + t) * TW + qx, v);
#pragma unroll
                                for (int i = 0; i < 4; i++) sum[i] += ty8[t] * v[i];
                            }
#pragma unroll
                            for (int i = 0; i < 4; i++) {
                                if (comp) res[i] = (int)(uint16_t)((sum[i] + 64) >> 7);
                                else { // round_1 = 11, bits = 0
                                    const int v = ((sum[i] + 1024) >> 11) - ((1 << bd) + (1 << (bd - 1)));
                                    res[i] = clampi(HBD ? v : (int)(int16_t)(uint16_t)v, 0, px_max);
                                }
                            }
                        }
                    } else if (fx) { // *_x_*
                        if (active) {
                            int in[12];
                            load4u(win + qy * ws + qx, in); load4u(win + qy * ws + qx + 4, in + 4); load4u(win + qy * ws + qx + 8, in + 8);
#pragma unroll
                            for (int i = 0; i < 4; i++) {
                                int sum = 0;
#pragma unroll
                                for (int t = 0; t < 8; t++) sum += tx8[t] * in[i + t];
                                const int r0 = (sum + 4) >> 3;
                                res[i] = comp ? r0 + ro : clampi((r0 + 8) >> 4, 0, px_max);
                            }
                        }
                    } else { // *_y_*
                        if (active) {
                            int sum[4] = {0, 0, 0, 0};
#pragma unroll
                            for (int t = 0; t < 8; t++) {
                                int v[4];
                                load4u(win + (qy + t) * ws + qx, v);
#pragma unroll
                                for (int i = 0; i < 4; i++) sum[i] += ty8[t] * v[i];
                            }
#pragma unroll
                            for (int i = 0; i < 4; i++) res[i] = comp ? ((sum[i] * 16 + 64) >> 7) + ro : clampi((sum[i] + 64) >> 7, 0, px_max);
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    if (!comp) out[i] = res[i];
                    else if (k == 0) acc[i] = (int)(uint16_t)res[i]; // the CONV_BUF_TYPE store
                    else {
                        int tmp = acc[i];
                        tmp = j.comp_mode ? (tmp * (int)j.fwd_offset + res[i] * (int)j.bck_offset) >> 4 : (tmp + res[i]) >> 1;
                        tmp -= ro;
                        out[i] = clampi((tmp + 8) >> 4, 0, px_max);
                    }
                }
            }
            if (active) {
                Px *p = dst + (size_t)j.dst_offset + (size_t)(ty + qy) * d.dst_stride + (size_t)(tx + qx);
                if (HBD) {
                    if (((uintptr_t)p & 7u) == 0) *(uint2 *)p = make_uint2((uint32_t)out[0] | ((uint32_t)out[1] << 16), (uint32_t)out[2] | ((uint32_t)out[3] << 16));
                    else { p[0] = (Px)out[0]; p[1] = (Px)out[1]; p[2] = (Px)out[2]; p[3] = (Px)out[3]; }
                } else {
                    if (((uintptr_t)p & 3u) == 0) *(uint32_t *)p = (uint32_t)out[0] | ((uint32_t)out[1] << 8) | ((uint32_t)out[2] << 16) | ((uint32_t)out[3] << 24);
                    else { p[0] = (Px)out[0]; p[1] = (Px)out[1]; p[2] = (Px)out[2]; p[3] = (Px)out[3]; }
                }
            }
        }
    if (lane == 0) d.status[job] = SVT_HIP_INTER_PRED_OK;
}

} // namespace

extern "C" {

int svt_hip_inter_pred_check_desc(const SvtHipInterPredDesc *d) {
    if (!d) BAD("svt_hip_inter_pred_check_desc: null descriptor");
    if (!d->dst || !d->jobs || !d->status) BAD("svt_hip_inter_pred_check_desc: a mandatory pointer (dst, jobs, status) is null");
    if (d->bit_depth != 8 && d->bit_depth != 10) BAD("svt_hip_inter_pred_check_desc: bit_depth %u (8 or 10)", d->bit_depth);
    if (d->ss_x > 1 || d->ss_y > 1) BAD("svt_hip_inter_pred_check_desc: ss_x %u / ss_y %u (0 or 1)", d->ss_x, d->ss_y);
    const int rc = svt_hip_check_inter_pred_refs("svt_hip_inter_pred_check_desc", d->refs, d->n_refs);
    if (rc) return rc;
    if (d->dst_stride == 0 || d->dst_samples == 0) BAD("svt_hip_inter_pred_check_desc: dst_stride %u / dst_samples %llu is zero", d->dst_stride, (unsigned long long)d->dst_samples);
    if (d->n_mvs && !d->mv_array) BAD("svt_hip_inter_pred_check_desc: n_mvs %u without mv_array", d->n_mvs);
    return SVT_HIP_OK;
}

size_t svt_hip_inter_pred_layout(int what, int field) {
#define D(f) offsetof(SvtHipInterPredDesc, f)
#define J(f) offsetof(SvtHipInterPredJob, f)
#define R(f) offsetof(SvtHipInterPredRef, f)
    static const size_t desc[] = {D(bit_depth), D(ss_x), D(ss_y), D(n_refs), D(n_jobs), D(refs), D(dst), D(dst_stride), D(reserved), D(dst_samples), D(jobs),
                                  D(mv_array), D(n_mvs), D(reserved2), D(status)};
    static const size_t job[]  = {J(dst_offset), J(org_x), J(org_y), J(width), J(height), J(filter_x), J(filter_y), J(ref), J(flags), J(comp_mode), J(mv),
                                  J(mv_index), J(mb_to_left_edge), J(mb_to_right_edge), J(mb_to_top_edge), J(mb_to_bottom_edge), J(fwd_offset), J(bck_offset),
                                  J(reserved)};
    static const size_t ref[]  = {R(plane), R(stride), R(org_x), R(org_y), R(width), R(height), R(reserved)};
#undef D
#undef J
#undef R
    const SvtHipLayoutRow rows[] = {layout_row<SvtHipInterPredDesc>(desc), layout_row<SvtHipInterPredJob>(job), layout_row<SvtHipInterPredRef>(ref)};
    return layout_lookup(rows, what, field);
}

int svt_hip_inter_pred_batch(SvtHipContext *ctx, const SvtHipInterPredDesc *d) {
    return enqueue_batch("svt_hip_inter_pred_batch", ctx, d, svt_hip_inter_pred_check_desc, &SvtHipInterPredDesc::n_jobs, [=] {
        hipLaunchKernelGGL(pick_hbd(d->bit_depth, inter_pred_kernel<true>, inter_pred_kernel<false>), dim3(ceil_div(d->n_jobs, kWaves)), dim3(64 * kWaves), 0,
                           ctx->stream, *d);
    });
}

} // extern "C"
