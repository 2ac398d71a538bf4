// tpl_kernel.hip -- the TPL dispenser of one picture on gfx950 (levels 4 and 5: SAD source search, DC-only intra, full-pel,
// no rate): tpl_mc_flow_dispenser_sb_generic (Source/Lib/Codec/src_ops_process.c:519-1200) for every b64, result_model_store
// (:266-340) and svt_aom_generate_padding of the TPL recon picture (:1400-1406).  C-ABI in include/svt_hip_tpl.h.
//
// Five launches on the context stream:
//   tpl_src_kernel    one wave per block: the source-based decision (intra DC cost, ME candidates, NEWMV's srcrf_dist)
//   tpl_inter_kernel  one wave per NEWMV block: prediction from the recon-path reference, transform chain, reconstruction
//   tpl_intra_kernel  ONE workgroup: the other blocks, whose DC prediction reads the current recon picture's above row and left
//                     column, walked anti-diagonal by anti-diagonal (a barrier between diagonals; no inter-workgroup hand-off)
//   tpl_pad_kernel / tpl_grid_kernel  the padding of the recon plane and the synthesizer grid
// A block's transform chain runs on one wave: residual -> forward DCT_DCT with the partial-frequency shape -> svt_av1_quantize_fp
// (log-scale 0) -> svt_av1_block_error -> inverse DCT_DCT -> reconstruction, in the arithmetic of rd_kernel.hip (txfm_core.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <mutex>
#include "svt_hip_internal.h"
#include "../../include/svt_hip_tpl.h"

#include "txfm_core.h"

namespace {

constexpr int kNewMv = 16; // NEWMV (Codec/definitions.h PredictionMode)
constexpr int kIntraWaves = 16; // waves of the intra wavefront's one workgroup

// per-block state between the launches: the decision (TplSrcStats, reserved[0] = 1 when the block is at least half inside) and the
// block's TplStats after result_model_store's max(1, .)
struct TplBlk {
    SvtHipTplSrcStats dec;
    SvtHipTplStats    fin;
};

struct TplParams {
    SvtHipTplDesc   d;
    const int16_t  *iscan; // default scan of the transform size, inverse
    TplBlk         *blk;
    int             size, k, nbx, nby, nb64x, sub;
};

__device__ __forceinline__ const uint8_t *pix(const SvtHipPlaneDesc &p, int x, int y) {
    return p.buffer_y + (ptrdiff_t)(p.org_y + y) * p.stride_y + p.org_x + x;
}

// svt_aom_dc_pred[x > 0][y > 0] (Codec/intra_prediction.c:2579-2597) on the neighbours both fills produce for DC: the above row
// cut at the picture width (127 past it), the left column cut at the picture height (129 past it) -- get_neighbor_samples_dc,
// svt_aom_update_neighbor_samples_array_open_loop_mb{,_recon} (Codec/enc_intra_prediction.c:1127-1290) agree on these samples
__device__ int dc_value(const SvtHipPlaneDesc &p, int x, int y, int S, int W, int H, int l) {
    uint32_t sa = 0, sl = 0;
    if (l < S) {
        if (y > 0) sa = (x + l < W) ? *pix(p, x + l, y - 1) : 127;
        if (x > 0) sl = (y + l < H) ? *pix(p, x - 1, y + l) : 129;
    }
    sa = wave_sum(sa);
    sl = wave_sum(sl);
    if (x > 0 && y > 0) return (int)((sa + sl + S) / (2 * S));
    if (x > 0) return (int)((sl + S / 2) / S);
    if (y > 0) return (int)((sa + S / 2) / S);
    return 128;
}

// the transform chain of one block on one wave.  A: LDS [H][W + 1] holding the residual (rows of the sub-sampled block); on return
// with inv set and eob != 0, the inverse transform's residual.  Returns get_quantize_error's recon_error (>= 1), sets eob.
template <int TS> __device__ int64_t tx_chain(int32_t *A, int l, int pf, const SvtHipQuantRow &q, const int16_t *iscan, bool inv, uint32_t &eob_out) {
    constexpr int W = tx_wide(TS), H = tx_high(TS), PA = W + 1;
    constexpr bool RECT = (W == 2 * H || H == 2 * W);
    const int8_t *fsh = c_fwd_shift[TS];
    const int bit_col = c_fwd_cos_col[ilog2c(W) - 2][ilog2c(H) - 2], bit_row = c_fwd_cos_row[ilog2c(W) - 2][ilog2c(H) - 2];
    if (l < W) { // forward columns
        int32_t x[H];
#pragma unroll
        for (int r = 0; r < H; r++) x[r] = A[r * PA + l];
        shift_vec<H>(x, fsh[0]);
        fwd_1d<H, 0>(x, 0, bit_col);
        shift_vec<H>(x, fsh[1]);
#pragma unroll
        for (int r = 0; r < H; r++) A[r * PA + l] = x[r];
    }
    wave_sync_workgroup_fences();
    if (l < H) { // forward rows
        int32_t x[W];
#pragma unroll
        for (int c = 0; c < W; c++) x[c] = A[l * PA + c];
        fwd_1d<W, 0>(x, 0, bit_row);
        shift_vec<W>(x, fsh[2]);
        if constexpr (RECT) {
#pragma unroll
            for (int c = 0; c < W; c++) x[c] = rshift64((i64)x[c] * 5793, 12);
        }
#pragma unroll
        for (int c = 0; c < W; c++) A[l * PA + c] = x[c];
    }
    wave_sync_workgroup_fences();
    // svt_av1_quantize_fp (quantize_fp_helper_c, 8-bit, log_scale 0, no matrix) + svt_av1_block_error over the kept coefficients
    // svt_av1_wht_fwd_txfm (Codec/transforms.c) switches on N2 and N4 alone: ONLY_DC_SHAPE (3) runs the whole transform
    if (pf == 3) pf = 0;
    const int keep_w = W >> pf, keep_h = H >> pf;
    uint32_t eob = 0;
    u64 err = 0;
    for (int rc = l; rc < W * H; rc += 64) {
        const int r = rc / W, c = rc - r * W, ac = rc != 0;
        const bool kept = pf == 0 || (c < keep_w && r < keep_h);
        const int32_t co = kept ? A[r * PA + c] : 0, sign = co < 0 ? -1 : 0, a = (co ^ sign) - sign;
        int32_t qv = 0, dq = 0;
        if (((i64)a << 1) >= (int32_t)q.dequant[ac]) {
            i64 t = (i64)a + q.round_fp[ac];
            t = t < -32768 ? -32768 : (t > 32767 ? 32767 : t);
            qv = (int32_t)((t * q.quant_fp[ac]) >> 16);
            dq = qv * (int32_t)q.dequant[ac];
        }
        const int32_t dqs = (dq ^ sign) - sign;
        if (qv) { const uint32_t e = (uint32_t)iscan[rc] + 1; eob = e > eob ? e : eob; }
        const i64 dd = (i64)co - dqs;
        err += (u64)(dd * dd);
        A[r * PA + c] = dqs;
    }
    eob = wave_max(eob);
    err = wave_sum(err);
    eob_out = eob;
    wave_sync_workgroup_fences();
    if (inv && eob) { // inverse DCT_DCT (inv_txfm2d_add_c, inv_transforms.c:2497-2534), 8-bit clamps
        if (l < H) {
            int32_t xr[W];
#pragma unroll
            for (int c = 0; c < W; c++) {
                int32_t v = A[l * PA + c];
                if constexpr (RECT) v = rshift64((i64)v * 2896, 12);
                xr[c] = clampv(v, 16);
            }
            inv_1d<W, 16, 1>(xr, 0);
            shift_vec<W>(xr, c_inv_shift0[TS]);
#pragma unroll
            for (int c = 0; c < W; c++) A[l * PA + c] = xr[c];
        }
        wave_sync_workgroup_fences();
        if (l < W) {
            int32_t x[H];
#pragma unroll
            for (int r = 0; r < H; r++) x[r] = clampv(A[r * PA + l], 16);
            inv_1d<H, 16, 1>(x, 0);
            shift_vec<H>(x, -4);
#pragma unroll
            for (int r = 0; r < H; r++) A[r * PA + l] = x[r];
        }
        wave_sync_workgroup_fences();
    }
    const int shift = TS == 3 ? 0 : 2; // TX_32X32 (get_quantize_error, src_ops_process.c:225-249)
    const int64_t re = (int64_t)(err >> shift);
    return re > 1 ? re : 1;
}

// The block's geometry.  Blocks are numbered over the grid of the b64-aligned picture, raster order.
struct Blk {
    int bx, by, x, y, b64, mbo, z;
};
__device__ __forceinline__ Blk block_of(const TplParams &p, int i) {
    Blk b;
    b.bx = i % p.nbx; b.by = i / p.nbx;
    b.x = b.bx * p.size; b.y = b.by * p.size;
    const int lx = b.bx % p.k, ly = b.by % p.k;
    b.b64 = (b.by / p.k) * p.nb64x + b.bx / p.k;
    // tpl_blk_idx_tab[1] (:353-355): the ME's raster PU index; without 16x16 PUs, (idx - 1) / 4 (:761-763)
    int me = p.size == 16 ? 5 + ly * 4 + lx : 1 + ly * 2 + lx;
    if (!p.d.enable_me_16x16) me = (me - 1) / 4;
    b.mbo = me;
    b.z = p.size == 16 ? (ly >> 1) * 8 + (lx >> 1) * 4 + (ly & 1) * 2 + (lx & 1) : ly * 2 + lx; // tpl_blk_idx_tab[0] order
    return b;
}
__device__ __forceinline__ bool half_inside(const TplParams &p, const Blk &b) { // :578-581
    return b.x + p.size / 2 <= p.d.cur.width && b.y + p.size / 2 <= p.d.cur.height;
}

// The MV clamp of the source search (:792-803), in the reference's int16 arithmetic
__device__ __forceinline__ void clamp_mv(int x, int y, int S, int max_w, int max_h, int16_t &mx, int16_t &my) {
    constexpr int PAD = SVT_HIP_TPL_PAD;
    if (x + (mx >> 3) < -PAD) mx = (int16_t)((-PAD - x) * 8);
    if (x + S + (mx >> 3) > PAD + max_w - 1) mx = (int16_t)(((PAD + max_w - 1) - (x + S)) * 8);
    if (y + (my >> 3) < -PAD) my = (int16_t)((-PAD - y) * 8);
    if (y + S + (my >> 3) > PAD + max_h - 1) my = (int16_t)(((PAD + max_h - 1) - (y + S)) * 8);
}

template <int TS> __global__ void __launch_bounds__(64) tpl_src_kernel(const TplParams p) {
    constexpr int W = tx_wide(TS), H = tx_high(TS);
    __shared__ int32_t A[H * (W + 1)];
    const int l = threadIdx.x, S = p.size, step = 1 << p.sub;
    const Blk b = block_of(p, blockIdx.x);
    TplBlk *out = p.blk + blockIdx.x;
    const SvtHipTplDesc &d = p.d;
    SvtHipTplSrcStats st = {};
    if (!half_inside(p, b)) {
        if (l == 0) out->dec = st; // reserved[0] = 0: skipped
        return;
    }
    const int a16w = (d.aligned_width + 15) >> 4;
    const size_t src_idx = (size_t)(b.y >> 4) * a16w + (b.x >> 4);
    if (!d.src_pass) { // stats of an earlier TPL group (:968-977)
        if (l == 0) {
            st = d.tpl_src_stats[src_idx];
            // a NEWMV decision naming a reference without a recon plane cannot come from the reference's source pass: such a block is
            // skipped as a whole (recon samples and grid cells untouched), never published with stale scratch
            const int rf = st.best_rf_idx;
            const bool ok = st.best_mode != kNewMv || (rf >= 0 && rf <= 7 && d.refs[rf >> 2][rf & 3].recon.buffer_y);
            st.reserved[0] = ok ? 1 : 0;
            out->dec = st;
        }
        return;
    }
    const int cw = d.cur.width, ch = d.cur.height;
    int64_t best_intra = INT64_MAX, best_inter = INT64_MAX;
    if (!d.disable_intra_pred) { // DC prediction from the source + SAD (:624-659)
        const int dc = dc_value(d.cur, b.x, b.y, S, cw, ch, l);
        uint32_t sad = 0;
        for (int i = l; i < S * S; i += 64) { const int r = i / S, c = i - r * S; sad += (uint32_t)abs((int)*pix(d.cur, b.x + c, b.y + r) - dc); }
        best_intra = wave_sum(sad);
    }
    st.best_rf_idx = -1;
    const int cnt_raw = d.slice_is_i ? 0 : d.me.total_me_candidate_index[(size_t)b.b64 * d.n_pu + b.mbo];
    const int cnt = cnt_raw < d.max_cand ? cnt_raw : d.max_cand;
    for (int ci = 0; ci < cnt; ci++) { // ME candidates (:771-884)
        const uint8_t cand = d.me.me_candidate_array[((size_t)b.b64 * d.n_pu + b.mbo) * d.max_cand + ci];
        const int dir = cand & 3;
        if (dir > 1) continue; // single references only
        const int list = dir, ref = list == 0 ? (cand >> 2) & 3 : (cand >> 4) & 3;
        const SvtHipTplRef &rf = d.refs[list][ref];
        const int slot = (list ? d.max_l0 : 0) + ref;
        if (!rf.usable || !rf.src.buffer_y || slot >= d.max_refs) continue;
        const uint32_t mv = d.me.me_mv_array[((size_t)b.b64 * d.n_pu + b.mbo) * d.max_refs + slot];
        int16_t mx = (int16_t)((int16_t)(mv & 0xFFFF) * 8), my = (int16_t)((int16_t)(mv >> 16) * 8);
        clamp_mv(b.x, b.y, S, rf.max_width, rf.max_height, mx, my);
        const int rx = b.x + (mx >> 3), ry = b.y + (my >> 3);
        uint32_t sad = 0;
        for (int i = l; i < S * S; i += 64) { const int r = i / S, c = i - r * S; sad += (uint32_t)abs((int)*pix(d.cur, b.x + c, b.y + r) - (int)*pix(rf.src, rx + c, ry + r)); }
        const int64_t cost = wave_sum(sad);
        if (cost < best_inter) {
            best_inter = cost;
            st.ref_frame_poc = rf.picture_number;
            st.best_rf_idx = list * 4 + ref;
            st.mv_row = my; st.mv_col = mx;
        }
    }
    st.best_mode = best_inter < best_intra ? kNewMv : 0;
    if (st.best_mode == kNewMv) { // source-path residual of the winner -> get_quantize_error (:889-957)
        const SvtHipTplRef &rf = d.refs[st.best_rf_idx >> 2][st.best_rf_idx & 3];
        const int rx = b.x + (st.mv_col >> 3), ry = b.y + (st.mv_row >> 3);
        for (int i = l; i < W * H; i += 64) {
            const int r = i / W, c = i - r * W;
            A[r * (W + 1) + c] = (int)*pix(d.cur, b.x + c, b.y + r * step) - (int)*pix(rf.src, rx + c, ry + r * step);
        }
        wave_sync_workgroup_fences();
        uint32_t eob;
        const int64_t re = tx_chain<TS>(A, l, d.pf_shape, d.quant, p.iscan, false, eob);
        st.srcrf_dist = (re << 4) << p.sub; // TPL_DEP_COST_SCALE_LOG2
        st.srcrf_rate = 0;
    }
    st.best_intra_mode = 0; // DC_PRED
    if (l == 0) {
        if (d.store_src_stats) d.tpl_src_stats[src_idx] = st;
        st.reserved[0] = 1;
        out->dec = st;
    }
}

// Reconstruction of one block (:1131-1198) from its prediction (pred(r, c), r < S, c < S) and the stats of result_model_store
template <int TS, typename Pred> __device__ void recon_block(const TplParams &p, const Blk &b, TplBlk *out, int32_t *A, int l, Pred pred) {
    constexpr int W = tx_wide(TS), H = tx_high(TS);
    const SvtHipTplDesc &d = p.d;
    const int S = p.size, step = 1 << p.sub;
    for (int i = l; i < W * H; i += 64) {
        const int r = i / W, c = i - r * W;
        A[r * (W + 1) + c] = (int)*pix(d.cur, b.x + c, b.y + r * step) - pred(r * step, c);
    }
    wave_sync_workgroup_fences();
    const bool inv = !d.disable_intra_pred || d.is_ref;
    uint32_t eob;
    const int64_t re = tx_chain<TS>(A, l, d.pf_shape, d.quant, p.iscan, inv, eob);
    const bool added = inv && eob; // otherwise the recon keeps the prediction, rows included (no duplication)
    uint8_t *rec = const_cast<uint8_t *>(d.recon.buffer_y) + (ptrdiff_t)(d.recon.org_y + b.y) * d.recon.stride_y + d.recon.org_x + b.x;
    for (int i = l; i < S * S; i += 64) {
        const int r = i / S, c = i - r * S;
        int v;
        if (added) { // transform row r / step, then the copies of the missing rows (:1161-1179)
            const int r0 = r & ~(step - 1);
            v = pred(r0, c) + A[(r0 >> p.sub) * (W + 1) + c];
            v = v < 0 ? 0 : (v > 255 ? 255 : v);
        } else
            v = pred(r, c);
        rec[(ptrdiff_t)r * d.recon.stride_y + c] = (uint8_t)v;
    }
    if (l == 0) {
        const SvtHipTplSrcStats &st = out->dec;
        SvtHipTplStats f = {};
        f.recrf_dist = (re << 4) << p.sub;
        f.recrf_rate = 0;
        if (st.best_mode != kNewMv) { f.srcrf_dist = f.recrf_dist; f.srcrf_rate = 0; }
        else { f.srcrf_dist = st.srcrf_dist; f.srcrf_rate = st.srcrf_rate; }
        f.recrf_dist = f.srcrf_dist > f.recrf_dist ? f.srcrf_dist : f.recrf_dist;
        f.recrf_rate = f.srcrf_rate > f.recrf_rate ? f.srcrf_rate : f.recrf_rate;
        if (!d.tpl_slice_is_i && st.best_rf_idx != -1) { f.mv_row = st.mv_row; f.mv_col = st.mv_col; f.ref_frame_poc = st.ref_frame_poc; }
        f.srcrf_dist = f.srcrf_dist > 1 ? f.srcrf_dist : 1; // result_model_store (:268-271)
        f.recrf_dist = f.recrf_dist > 1 ? f.recrf_dist : 1;
        f.srcrf_rate = f.srcrf_rate > 1 ? f.srcrf_rate : 1;
        f.recrf_rate = f.recrf_rate > 1 ? f.recrf_rate : 1;
        out->fin = f;
    }
}

template <int TS> __global__ void __launch_bounds__(64) tpl_inter_kernel(const TplParams p) {
    constexpr int W = tx_wide(TS), H = tx_high(TS);
    __shared__ int32_t A[H * (W + 1)];
    TplBlk *out = p.blk + blockIdx.x;
    const SvtHipTplSrcStats st = out->dec;
    if (!st.reserved[0] || st.best_mode != kNewMv) return;
    const int rf_idx = st.best_rf_idx;
    const SvtHipTplRef &rf = p.d.refs[rf_idx >> 2][rf_idx & 3]; // 0..7 with a recon plane: tpl_src_kernel checked it
    const Blk b = block_of(p, blockIdx.x);
    // the recon-path block at the decision's MV; a stored MV (src_pass == 0) is kept inside the clamp window of the search
    constexpr int PAD = SVT_HIP_TPL_PAD;
    int rx = b.x + (st.mv_col >> 3), ry = b.y + (st.mv_row >> 3);
    rx = rx < -PAD ? -PAD : (rx > PAD + rf.max_width - 1 - p.size ? PAD + rf.max_width - 1 - p.size : rx);
    ry = ry < -PAD ? -PAD : (ry > PAD + rf.max_height - 1 - p.size ? PAD + rf.max_height - 1 - p.size : ry);
    const SvtHipPlaneDesc rp = rf.recon;
    recon_block<TS>(p, b, out, A, threadIdx.x, [&](int r, int c) { return (int)*pix(rp, rx + c, ry + r); });
}

// The blocks that are not NEWMV, on ONE workgroup: anti-diagonal t holds the blocks (bx, by) with bx + by == t; each wave takes
// blocks of the diagonal in turn, and the workgroup barrier between diagonals makes the recon samples of diagonal t visible to
// diagonal t + 1 (a block's DC reads its above and left neighbours only)
template <int TS> __global__ void __launch_bounds__(64 * kIntraWaves) tpl_intra_kernel(const TplParams p) {
    constexpr int W = tx_wide(TS), H = tx_high(TS);
    __shared__ int32_t A_all[kIntraWaves][H * (W + 1)];
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63;
    int32_t *A = A_all[wave];
    const SvtHipTplDesc &d = p.d;
    for (int t = 0; t < p.nbx + p.nby - 1; t++) {
        const int by0 = t - (p.nbx - 1) > 0 ? t - (p.nbx - 1) : 0, by1 = t < p.nby - 1 ? t : p.nby - 1;
        for (int by = by0 + wave; by <= by1; by += kIntraWaves) {
            const int i = by * p.nbx + (t - by);
            TplBlk *out = p.blk + i;
            const uint8_t processed = out->dec.reserved[0], mode = out->dec.best_mode;
            if (!processed || mode == kNewMv) continue;
            const Blk b = block_of(p, i);
            // intra recon (:1042-1087): DC from the current recon picture
            const int dc = dc_value(d.recon, b.x, b.y, p.size, d.cur.width, d.cur.height, l);
            recon_block<TS>(p, b, out, A, l, [&](int, int) { return dc; });
        }
        __syncthreads();
    }
}

// svt_aom_generate_padding (Codec/pic_operators.c:397-443) of the recon plane: each padding sample computed from interior samples
// that nobody writes (in-place safe in one launch)
__global__ void __launch_bounds__(256) tpl_pad_kernel(SvtHipPlaneDesc rp) {
    const int X = blockIdx.x * 256 + threadIdx.x, Y = blockIdx.y;
    const int ox = rp.org_x, oy = rp.org_y, w = rp.width, h = rp.height;
    if (X >= (int)rp.stride_y) return;
    uint8_t *buf = const_cast<uint8_t *>(rp.buffer_y);
    const bool in_rows = Y >= oy && Y < oy + h, pad_col = X < ox || (X >= ox + w && X < 2 * ox + w);
    if (in_rows && !pad_col) return;
    const int sy = Y < oy ? oy : (Y >= oy + h ? oy + h - 1 : Y);
    const int sx = X < ox ? ox : ((X >= ox + w && X < 2 * ox + w) ? ox + w - 1 : X);
    buf[(size_t)Y * rp.stride_y + X] = buf[(size_t)sy * rp.stride_y + sx];
}

// result_model_store (:272-295) as a gather: every cell takes the block the reference wrote into it LAST -- the latest in the
// order of b64s in raster order, blocks in z-order (synth 32 with 16x16 blocks: the last block at least half inside; synth 16 with
// 32x32 blocks: the 2x2 writes run on in linear cell order, past the end of a grid row like the reference's)
__global__ void __launch_bounds__(256) tpl_grid_kernel(const TplParams p) {
    const uint32_t cell = blockIdx.x * 256 + threadIdx.x;
    const SvtHipTplDesc &d = p.d;
    if (cell >= d.n_tpl_stats) return;
    const int G = d.synth_blk_size, gs = (d.aligned_width + G - 1) / G;
    int best = -1, best_key = -1;
    auto consider = [&](int bx, int by) {
        if (bx < 0 || by < 0 || bx >= p.nbx || by >= p.nby) return;
        const int i = by * p.nbx + bx;
        if (!p.blk[i].dec.reserved[0]) return;
        const Blk b = block_of(p, i);
        const int key = b.b64 * 16 + b.z;
        if (key > best_key) { best_key = key; best = i; }
    };
    const int cy = (int)(cell / gs), cx = (int)(cell % gs);
    if (G == p.size) consider(cx, cy);
    else if (G == 32) { // 16x16 blocks
        for (int dy = 0; dy < 2; dy++)
            for (int dx = 0; dx < 2; dx++) consider(2 * cx + dx, 2 * cy + dy);
    } else { // 32x32 blocks on the 16 grid: bases cell, cell - 1, cell - gs, cell - gs - 1
        const int offs[4] = {0, 1, gs, gs + 1};
        for (int k = 0; k < 4; k++) {
            const int base = (int)cell - offs[k];
            if (base < 0) continue;
            const int row = base / gs, col = base % gs;
            if ((row & 1) || (col & 1)) continue;
            consider(col / 2, row / 2);
        }
    }
    if (best < 0) return;
    SvtHipTplStats f = p.blk[best].fin;
    if (G == 16 && p.size == 32) { // normalise to the 16x16 block (:284-288)
        f.srcrf_dist = f.srcrf_dist / 4 > 1 ? f.srcrf_dist / 4 : 1;
        f.recrf_dist = f.recrf_dist / 4 > 1 ? f.recrf_dist / 4 : 1;
        f.srcrf_rate = f.srcrf_rate / 4 > 1 ? f.srcrf_rate / 4 : 1;
        f.recrf_rate = f.recrf_rate / 4 > 1 ? f.recrf_rate / 4 : 1;
    }
    d.tpl_stats[cell] = f;
}

const char *plane_problem(const SvtHipPlaneDesc &p, int min_pad) {
    if (!p.buffer_y) return "null plane";
    if (p.org_x < min_pad || p.org_y < min_pad) return "padding too small";
    if (p.stride_y < (uint32_t)p.width + 2u * p.org_x) return "stride below width + 2 * org_x";
    if (!p.width || !p.height) return "empty plane";
    return nullptr;
}

template <int TS> int launch_all(SvtHipContext *ctx, const TplParams &p, int n_blk) {
    hipLaunchKernelGGL((tpl_src_kernel<TS>), dim3(n_blk), dim3(64), 0, ctx->stream, p);
    hipLaunchKernelGGL((tpl_inter_kernel<TS>), dim3(n_blk), dim3(64), 0, ctx->stream, p);
    hipLaunchKernelGGL((tpl_intra_kernel<TS>), dim3(1), dim3(64 * kIntraWaves), 0, ctx->stream, p);
    const SvtHipPlaneDesc &rp = p.d.recon;
    hipLaunchKernelGGL(tpl_pad_kernel, dim3((rp.stride_y + 255) / 256, 2 * rp.org_y + rp.height), dim3(256), 0, ctx->stream, rp);
    hipLaunchKernelGGL(tpl_grid_kernel, dim3((p.d.n_tpl_stats + 255) / 256), dim3(256), 0, ctx->stream, p);
    SVT_HIP_CHECK(ctx, hipGetLastError());
    return SVT_HIP_OK;
}

} // namespace

// The cosine table of this translation unit's copy of txfm_core.h (svt_hip_rd_tables_init fills rd_kernel.hip's)
int svt_hip_tpl_tables_init(SvtHipContext *ctx) {
    SVT_HIP_CHECK(ctx, txfm_upload_cospi());
    return SVT_HIP_OK;
}

void svt_hip_tpl_free(SvtHipContext *ctx) {
    svt_hip_tpl_group_free(ctx);
    svt_hip_buffer_release(&ctx->tpl_scratch);
}

extern "C" {

size_t svt_hip_tpl_desc_size(void) { return sizeof(SvtHipTplDesc); }

int svt_hip_tpl_check_desc(const SvtHipTplDesc *d) {
#define BAD(...) return svt_hip_fail(nullptr, SVT_HIP_ERR_BAD_PARAM, __VA_ARGS__)
    if (!d) BAD("svt_hip_tpl_check_desc: null descriptor");
    if (d->use_sad_in_src_search != 1) BAD("TPL: use_sad_in_src_search 0 (SATD source search, level 1) runs on the host");
    if (d->intra_mode_end != 0) BAD("TPL: intra_mode_end %u (only DC_PRED, levels 4 / 5)", d->intra_mode_end);
    if (d->subpel_depth != 3) BAD("TPL: subpel_depth %u (only FULL_PEL = 3, levels 4 / 5)", d->subpel_depth); // SUBPEL_FORCE_STOP, definitions.h:741
    if (d->compute_rate != 0) BAD("TPL: compute_rate (level 1) runs on the host");
    if (d->dispenser_search_level > 1) BAD("TPL: dispenser_search_level %u (0 or 1)", d->dispenser_search_level);
    if (d->synth_blk_size != 16 && d->synth_blk_size != 32) BAD("TPL: synth_blk_size %u (16 or 32)", d->synth_blk_size);
    if (d->in_loop_ois != 1) BAD("TPL: in_loop_ois 0 (the OIS results are not an input)");
    if (d->subsample_tx > 2 || d->pf_shape > 3) BAD("TPL: subsample_tx %u / pf_shape %u", d->subsample_tx, d->pf_shape);
    const char *why;
    if ((why = plane_problem(d->cur, 16))) BAD("TPL: current picture: %s", why);
    if ((why = plane_problem(d->recon, SVT_HIP_TPL_PAD))) BAD("TPL: recon picture: %s (padding >= %d)", why, SVT_HIP_TPL_PAD);
    if (d->recon.width < d->cur.width || d->recon.height < d->cur.height) BAD("TPL: recon picture smaller than the current one");
    if (d->aligned_width < d->cur.width || d->aligned_height < d->cur.height) BAD("TPL: aligned size below the picture size");
    for (int li = 0; li < SVT_HIP_MAX_LISTS; li++)
        for (int ri = 0; ri < SVT_HIP_MAX_REFS; ri++) {
            const SvtHipTplRef &r = d->refs[li][ri];
            // a usable reference may be searched; with stored stats (src_pass 0) any reference that has planes may be named
            if (d->slice_is_i || !(r.usable || (!d->src_pass && (r.src.buffer_y || r.recon.buffer_y)))) continue;
            if ((why = plane_problem(r.src, SVT_HIP_TPL_PAD)) || (why = plane_problem(r.recon, SVT_HIP_TPL_PAD)))
                BAD("TPL: reference [%d][%d]: %s (padding >= %d)", li, ri, why, SVT_HIP_TPL_PAD);
            if (r.max_width > r.src.width || r.max_height > r.src.height || r.max_width > r.recon.width || r.max_height > r.recon.height ||
                !r.max_width || !r.max_height)
                BAD("TPL: reference [%d][%d]: max_width / max_height %ux%u outside its planes", li, ri, r.max_width, r.max_height);
        }
    if (!d->slice_is_i) {
        if (!d->me.total_me_candidate_index || !d->me.me_mv_array || !d->me.me_candidate_array) BAD("TPL: ME results missing");
        if (d->n_pu < (d->enable_me_16x16 ? 21 : 5) || !d->max_cand || !d->max_refs || d->max_l0 > d->max_refs)
            BAD("TPL: ME layout n_pu %u, max_cand %u, max_refs %u, max_l0 %u", d->n_pu, d->max_cand, d->max_refs, d->max_l0);
    }
    const uint32_t G = d->synth_blk_size;
    const uint32_t cells = ((d->aligned_width + G - 1) / G) * ((d->aligned_height + G - 1) / G);
    if (!d->tpl_stats || d->n_tpl_stats < cells) BAD("TPL: tpl_stats holds %u cells, the grid %u", d->n_tpl_stats, cells);
    const uint32_t cells16 = ((d->aligned_width + 15) / 16) * ((d->aligned_height + 15) / 16);
    if ((!d->src_pass || d->store_src_stats) && (!d->tpl_src_stats || d->n_tpl_src_stats < cells16))
        BAD("TPL: tpl_src_stats holds %u entries, the aligned-16 grid %u", d->n_tpl_src_stats, cells16);
    return SVT_HIP_OK;
#undef BAD
}

} // extern "C"

int svt_hip_tpl_dispense_locked(SvtHipContext *ctx, const SvtHipTplDesc *d) {
    TplParams p;
    p.d     = *d;
    p.size  = 16 << d->dispenser_search_level;
    p.k     = 64 / p.size;
    p.nb64x = (d->aligned_width + 63) / 64;
    p.nbx   = p.nb64x * p.k;
    p.nby   = ((d->aligned_height + 63) / 64) * p.k;
    p.sub   = d->subsample_tx;
    // tx_size_array / sub2_tx_size_array / sub4_tx_size_array (:380-382): TX_16X16, TX_16X8, TX_16X4 / TX_32X32, TX_32X16, TX_32X8
    static const int ts_tab[2][3] = {{2, 8, 14}, {3, 10, 16}};
    const int ts = ts_tab[d->dispenser_search_level][p.sub];
    p.iscan = ctx->iscan_dev + (size_t)ts * 3 * 1024;
    const int n_blk = p.nbx * p.nby;
    if (int rc = svt_hip_buffer_reserve(ctx, &ctx->tpl_scratch, sizeof(TplBlk) * (size_t)n_blk, ctx->stream, "TPL: hipMalloc(%zu) failed")) return rc;
    p.blk = static_cast<TplBlk *>(ctx->tpl_scratch.ptr);
    switch (ts) {
    case 2: return launch_all<2>(ctx, p, n_blk);
    case 8: return launch_all<8>(ctx, p, n_blk);
    case 14: return launch_all<14>(ctx, p, n_blk);
    case 3: return launch_all<3>(ctx, p, n_blk);
    case 10: return launch_all<10>(ctx, p, n_blk);
    default: return launch_all<16>(ctx, p, n_blk);
    }
}

extern "C" {

int svt_hip_tpl_dispense(SvtHipContext *ctx, const SvtHipTplDesc *d) {
    if (!ctx) return svt_hip_fail(nullptr, SVT_HIP_ERR_BAD_PARAM, "svt_hip_tpl_dispense: null context");
    int rc = svt_hip_tpl_check_desc(d);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(ctx->async_mu);
    if ((rc = svt_hip_use_device(ctx))) return rc;
    return svt_hip_tpl_dispense_locked(ctx, d);
}

} // extern "C"
