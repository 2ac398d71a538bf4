// coeff_rate_kernel.hip -- the rate half of the RD cost on gfx950: svt_hip_coeff_rate_batch (coefficient rate estimation per job, the RD
// cost, the winner of every group of candidates).
//
// Reference functions restated (Source/Lib):
//   svt_av1_cost_coeffs_txb, allow_update_cdf == 0              Codec/rd_cost.c:434-559
//   svt_av1_txb_init_levels_c                                   Codec/rd_cost.c:99-111
//   av1_transform_type_rate_estimation, get_ext_tx_set{,_type}  Codec/rd_cost.c:113-158, Codec/definitions.h:1787-1828
//   av1_cost_coeffs_txb_loop_cost_{one_,}eob                    Codec/rd_cost.c:310-431
//   svt_aom_txb_estimate_coeff_bits, av1_cost_skip_txb          Codec/rd_cost.c:1405-1450,299-308
//   the short-cuts and the winner of tx_type_search             Codec/product_coding_loop.c:4947-4952,4976-4985
//   RDCOST                                                      Codec/rd_cost.h:37
//
// The lay-out (the cost tables and a group's padded levels array in LDS, G lanes per job), the context rules and the cost terms of the level
// map: lvmap_core.h.  Every lane takes raster positions (four in a row from 256 coefficients up), writes their clamped levels into the group's
// levels array, and then adds the cost terms of its own positions: a position's place in the scan comes from the inverse scan table, its
// contexts from the levels array alone.  There is no serial dependency, and the 32-bit sums of the lanes meet by cross-lane adds in any order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "svt_hip_internal.h"
#include "batch_host.h"
#include "../../include/svt_hip_dsp.h"
#include "lvmap_core.h"
#include "wave_ops.h"

namespace {

struct RateParams {
    SvtHipCoeffRateDesc d;
    const int16_t *iscan[3];  // default, row (V_*), column (H_*) inverse scans of this tx_size
    LvMapGeom g;
    int      ext_set[2];      // get_ext_tx_set(tx_size, is_inter, reduced) by is_inter, 0 where get_ext_tx_types <= 1
    uint32_t c_div;           // MAX(1, mds_fast_coeff_est_level - mds_subres_step)
    uint32_t n_packs;
};

// The cost terms of the coefficient at raster position `pos` (scan index si < eob) of a block with eob >= 2; `bad` is set where the reference
// would index base_eob_cost[..][-1].
__device__ __forceinline__ uint32_t position_cost(const LvBlk &b, const SvtHipLvMapCoeffCost *cc, uint32_t eob, uint32_t c_start, int dc_sign_ctx, int pos,
                                                  uint32_t si, int32_t v, uint32_t &bad) {
    const bool last = si == eob - 1u;
    if (!last && si > c_start) return 0u; // si == 0 is the DC: always counted
    const uint32_t a = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
    uint32_t       cost;
    if (last) { // rd_cost.c:351-376
        if (a == 0u) { bad = 1u; return 0u; }
        cost = (uint32_t)(cc->base_eob_cost[eob_ctx(b, (int)si)][(a < 3u ? a : 3u) - 1u] + kCostLiteral);
    } else { // the DC (:377-404) and the middle loop (:410-427)
        cost = (uint32_t)cc->base_cost[lower_ctx(b, pos)][a < 3u ? a : 3u];
        if (a != 0u) cost += (uint32_t)(pos == 0 ? cc->dc_sign_cost[dc_sign_ctx][v < 0 ? 1 : 0] : kCostLiteral);
    }
    // get_br_ctx, not get_br_ctx_eob, for the last one too: the reference reads its neighbours, and levels behind eob count
    if (a > 2u) cost += (uint32_t)range_cost(cc, br_ctx(b, pos), (int)a);
    return cost;
}

// V coefficients in a row (zeros where `on` is false: nothing is read)
template <int V> __device__ __forceinline__ void load_coeffs(bool on, const int32_t *src, int32_t (&q)[V]) {
    if constexpr (V == 4) {
        int4 qv = make_int4(0, 0, 0, 0);
        if (on) qv = *reinterpret_cast<const int4 *>(src);
        q[0] = qv.x; q[1] = qv.y; q[2] = qv.z; q[3] = qv.w;
    } else q[0] = on ? src[0] : 0;
}

// N coefficients per job; G lanes per job, V coefficients in a row per lane and step
template <int N> __global__ void __launch_bounds__(64 * kWaves) coeff_rate_kernel(const RateParams p) {
    constexpr int V = N >= 256 ? 4 : 1, G = N / V < 64 ? N / V : 64, ITER = N / (G * V), JPW = 64 / G;
    __shared__ int32_t tab[kCoeffInts + kEobInts];
    __shared__ __attribute__((aligned(16))) uint8_t levels[kWaves][kLevelBytes];
    stage_cost_tables(tab, p.d.tables, p.g.txs_ctx, p.g.eob_multi, p.d.plane_type);
    const SvtHipLvMapCoeffCost *cc = reinterpret_cast<const SvtHipLvMapCoeffCost *>(tab);
    const SvtHipLvMapEobCost   *ec = reinterpret_cast<const SvtHipLvMapEobCost *>(tab + kCoeffInts);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, grp = lane / G, gl = lane % G;
    const int stride = p.g.w + 4, lev_bytes = stride * (p.g.h + 4); // a multiple of 16
    uint8_t  *lev = levels[wave] + grp * lev_bytes;
    LvBlk     b   = {lev, stride, p.g.bwl, p.g.shape, 0, N};
    for (uint32_t pack = blockIdx.x * kWaves + wave; pack < p.n_packs; pack += gridDim.x * kWaves) { // uniform per wave
        const uint32_t job   = pack * JPW + grp;
        const bool     valid = job < p.d.n_jobs;
        SvtHipRateJob  jb    = {};
        uint32_t       eob   = 0;
        if (valid) { jb = p.d.jobs[job]; eob = p.d.eob[job]; }
        // the caller's frame: the two short-cuts (product_coding_loop.c:4947-4952, luma only), then svt_aom_txb_estimate_coeff_bits
        const uint32_t lvl = p.d.coeff_rate_est_lvl;
        uint64_t bits    = ~0ull;
        bool     compute = false;
        if (p.d.plane_type == 0 && lvl != 1 && eob < (uint32_t)p.g.area >> 6) bits = 6000ull + (uint64_t)eob * 1000ull;
        else if (p.d.plane_type == 0 && lvl == 0) bits = 3000ull + (uint64_t)eob * 100ull;
        else if (jb.txb_skip_ctx >= 13) bits = ~0ull; // a context outside its table: undefined, nothing is read
        else if (eob == 0) bits = (uint64_t)(int64_t)cc->txb_skip_cost[jb.txb_skip_ctx][1]; // av1_cost_skip_txb
        else // intra_dir is read by intra luma jobs alone (rd_cost.c:137-153): an inter candidate's pred_mode is 13 or above and is fine
            compute = valid && eob <= (uint32_t)N && jb.tx_type < 16 && jb.dc_sign_ctx < 3 && (p.d.plane_type != 0 || jb.is_inter || jb.intra_dir < 13);
        const int      kind    = tx_scan_kind(jb.tx_type);
        b.cls                  = tx_class(jb.tx_type);
        const uint32_t c_start = eob >= 2 ? (eob - 2u < eob / p.c_div ? eob - 2u : eob / p.c_div) : 0u; // rd_cost.c:408

        // svt_av1_txb_init_levels_c: min(|qcoeff|, 127) over the WHOLE block, in a zero frame
        zero_levels<G>(lev, lev_bytes, gl);
        wave_sync();
#pragma unroll 1
        for (int it = 0; it < ITER; it++) {
            const int pos = (it * G + gl) * V;
            int32_t   q[V];
            load_coeffs<V>(compute, p.d.qcoeff + (size_t)job * N + pos, q);
            uint32_t packed = 0;
#pragma unroll
            for (int v = 0; v < V; v++) {
                const uint32_t a = q[v] < 0 ? 0u - (uint32_t)q[v] : (uint32_t)q[v];
                packed |= (a < 127u ? a : 127u) << (8 * v);
            }
            const int row = pos >> p.g.bwl, col = pos - (row << p.g.bwl); // four positions in a row never straddle rows: the width is a multiple of 4
            if constexpr (V == 4) *reinterpret_cast<uint32_t *>(lev + row * stride + col) = packed;
            else lev[row * stride + col] = (uint8_t)packed;
        }
        wave_sync();

        uint32_t cost = 0, bad = 0;
        if (compute) {
            if (eob == 1) { // av1_cost_coeffs_txb_loop_cost_one_eob (rd_cost.c:310-337): the DC alone, contexts 0
                if (gl == 0) {
                    const int32_t  v = p.d.qcoeff[(size_t)job * N];
                    const uint32_t a = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
                    if (a == 0u) bad = 1u;
                    else {
                        cost = (uint32_t)cc->base_eob_cost[0][(a < 3u ? a : 3u) - 1u] + (uint32_t)cc->dc_sign_cost[jb.dc_sign_ctx][v < 0 ? 1 : 0];
                        if (a > 2u) cost += (uint32_t)range_cost(cc, 0, (int)a);
                    }
                }
            } else {
                // the second pass reads the coefficients again (they are in the vector cache) rather than holding up to 16 of them per lane
#pragma unroll 1
                for (int it = 0; it < ITER; it++) {
                    const int pos = (it * G + gl) * V;
                    int32_t   q[V];
                    int16_t   si[V];
                    load_coeffs<V>(true, p.d.qcoeff + (size_t)job * N + pos, q);
                    if constexpr (V == 4) {
                        const short4 sv = *reinterpret_cast<const short4 *>(p.iscan[kind] + pos);
                        si[0] = sv.x; si[1] = sv.y; si[2] = sv.z; si[3] = sv.w;
                    } else si[0] = p.iscan[kind][pos];
#pragma unroll
                    for (int v = 0; v < V; v++) {
                        const uint32_t s = (uint32_t)(uint16_t)si[v];
                        if (s < eob) cost += position_cost(b, cc, eob, c_start, jb.dc_sign_ctx, pos + v, s, q[v], bad);
                    }
                }
            }
        }
        cost = group_sum<G>(cost);
        bad  = group_or<G>(bad);
        if (gl == 0 && valid) {
            if (compute && !bad) {
                // txb_skip_cost[ctx][0] + the transform type's rate (luma) + get_eob_cost
                cost += (uint32_t)cc->txb_skip_cost[jb.txb_skip_ctx][0];
                if (p.d.plane_type == 0) { // av1_transform_type_rate_estimation
                    const int inter = jb.is_inter ? 1 : 0, set = p.ext_set[inter];
                    if (set > 0)
                        cost += (uint32_t)(inter ? p.d.tables->inter_tx_type_fac_bits[set][p.g.sq][jb.tx_type]
                                                 : p.d.tables->intra_tx_type_fac_bits[set][p.g.sq][jb.intra_dir][jb.tx_type]);
                }
                cost += (uint32_t)eob_cost(cc, ec, b.cls, (int)eob);
                bits = (uint64_t)(int64_t)(int32_t)cost; // the reference's int32_t cost, returned as uint64_t
                if (p.d.plane_type == 0) bits <<= p.d.mds_subres_step;
            }
            p.d.bits[job] = bits;
            if (p.d.rd_cost) { // RDCOST(lambda, bits, dist) = ROUND_POWER_OF_TWO(bits * lambda, AV1_PROB_COST_SHIFT) + (dist << RDDIV_BITS)
                const uint64_t dist = p.d.dist[(size_t)job * (p.d.dist_stride ? p.d.dist_stride : 1u)];
                p.d.rd_cost[job]    = bits == ~0ull ? ~0ull : ((bits * (uint64_t)p.d.lambda + 256ull) >> 9) + (dist << 7);
            }
        }
        wave_sync(); // the next job's zero fill must not overtake this one's reads
    }
}

// tx_type_search keeps the first strict minimum in visiting order (product_coding_loop.c:4976-4985): one thread per group
__global__ void __launch_bounds__(256) rate_group_kernel(const SvtHipCoeffRateDesc d) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= d.n_groups) return;
    uint32_t first = d.group_start[g], end = d.group_start[g + 1];
    end = end < d.n_jobs ? end : d.n_jobs;
    uint32_t best_job  = 0xFFFFFFFFu;
    uint64_t best_cost = ~0ull;
    for (uint32_t j = first; j < end; j++) {
        const uint64_t c = d.rd_cost[j];
        if (c < best_cost) { best_cost = c; best_job = j; }
    }
    d.best_job[g]  = best_job;
    d.best_cost[g] = best_cost;
}

// get_ext_tx_set (Codec/definitions.h:1787-1828), 0 where get_ext_tx_types <= 1 or the set carries no rate
int ext_tx_set(int tx_size, int is_inter, int reduced) {
    const int up = kSqrUpMap[tx_size], sq = kSqrMap[tx_size];
    if (up > 3) return 0;                   // EXT_TX_SET_DCTONLY
    if (up == 3) return is_inter ? 3 : 0;   // EXT_TX_SET_DCT_IDTX : EXT_TX_SET_DCTONLY
    if (reduced) return is_inter ? 3 : 2;   // EXT_TX_SET_DCT_IDTX : EXT_TX_SET_DTT4_IDTX
    if (is_inter) return sq == 2 ? 2 : 1;   // EXT_TX_SET_DTT9_IDTX_1DDCT : EXT_TX_SET_ALL16
    return sq == 2 ? 2 : 1;                 // EXT_TX_SET_DTT4_IDTX : EXT_TX_SET_DTT4_IDTX_1DDCT
}

} // namespace

extern "C" {

size_t svt_hip_coeff_rate_desc_size(void) { return sizeof(SvtHipCoeffRateDesc); }
size_t svt_hip_rate_tables_size(void) { return sizeof(SvtHipRateTables); }

// the launch of the rate and RDOQ batches (lvmap_grid), for a caller or a test that wants to know how many trips a wave makes
int svt_hip_lvmap_plan(uint32_t tx_size, uint32_t n_jobs, uint32_t max_grid, uint32_t *grid, uint32_t *n_packs, uint32_t *jobs_per_pack) {
    if (tx_size >= SVT_HIP_TX_SIZES_ALL || !grid || !n_packs || !jobs_per_pack)
        return svt_hip_fail(nullptr, SVT_HIP_ERR_BAD_PARAM, "svt_hip_lvmap_plan: tx_size %u (below 19) or a null output", tx_size);
    const LvMapGeom g = lvmap_geom((int)tx_size);
    *grid          = lvmap_grid(g, n_jobs, max_grid, *n_packs); // no jobs: no packs and no launch
    *jobs_per_pack = (uint32_t)g.jobs_per_wave;
    return SVT_HIP_OK;
}

int svt_hip_context_set_lvmap_max_grid(SvtHipContext *ctx, uint32_t max_grid) {
    if (!ctx) return SVT_HIP_ERR_BAD_PARAM;
    ctx->lvmap_max_grid = max_grid;
    return SVT_HIP_OK;
}

static int coeff_rate_check(const SvtHipCoeffRateDesc *d) {
    if (d->tx_size >= SVT_HIP_TX_SIZES_ALL || d->plane_type > 1)
        BAD("svt_hip_coeff_rate_batch: tx_size %u (below 19) / plane_type %u (0 or 1)", d->tx_size, d->plane_type);
    if (d->mds_subres_step > 2 || d->mds_fast_coeff_est_level == 0)
        BAD("svt_hip_coeff_rate_batch: mds_subres_step %u (0..2) / mds_fast_coeff_est_level %u (not 0)", d->mds_subres_step, d->mds_fast_coeff_est_level);
    if (!d->jobs || !d->tables || !d->qcoeff || !d->eob || !d->bits) BAD("svt_hip_coeff_rate_batch: a mandatory pointer (jobs, tables, qcoeff, eob, bits) is null");
    if (((uintptr_t)d->qcoeff & 15) && lvmap_geom(d->tx_size).n >= 256)
        BAD("svt_hip_coeff_rate_batch: qcoeff is not 16-byte aligned (sizes of 256 coefficients and more are read 16 bytes at a time)");
    if (d->rd_cost && !d->dist) BAD("svt_hip_coeff_rate_batch: rd_cost without dist");
    const bool groups = d->n_groups || d->group_start || d->best_job || d->best_cost;
    if (groups && !d->rd_cost) BAD("svt_hip_coeff_rate_batch: groups without rd_cost");
    if (groups && (!d->group_start || !d->best_job || !d->best_cost)) BAD("svt_hip_coeff_rate_batch: groups need group_start, best_job and best_cost");
    return SVT_HIP_OK;
}

int svt_hip_coeff_rate_batch(SvtHipContext *ctx, const SvtHipCoeffRateDesc *d) {
    // both launches under one hold of the lock: the winners' launch follows its own costs' when several threads enqueue
    return enqueue_batch("svt_hip_coeff_rate_batch", ctx, d, coeff_rate_check, &SvtHipCoeffRateDesc::n_jobs, &SvtHipCoeffRateDesc::n_groups, [=] {
        const int  ts = d->tx_size;
        RateParams p;
        memset(&p, 0, sizeof(p));
        p.d = *d;
        for (int k = 0; k < 3; k++) p.iscan[k] = ctx->iscan_dev + ((size_t)ts * 3 + k) * 1024;
        p.g = lvmap_geom(ts);
        for (int inter = 0; inter < 2; inter++) p.ext_set[inter] = ext_tx_set(ts, inter, d->reduced_tx_set != 0);
        p.c_div = d->mds_fast_coeff_est_level > d->mds_subres_step ? (uint32_t)(d->mds_fast_coeff_est_level - d->mds_subres_step) : 1u;
        const uint32_t grid = lvmap_grid(p.g, d->n_jobs, ctx->lvmap_max_grid, p.n_packs);
        if (d->n_jobs) switch (p.g.n) { // lvmap_geom gives one of these for every tx_size the check accepted
#define CASE(N) case N: hipLaunchKernelGGL(coeff_rate_kernel<N>, dim3(grid), dim3(64 * kWaves), 0, ctx->stream, p); break;
            CASE(16) CASE(32) CASE(64) CASE(128) CASE(256) CASE(512) CASE(1024)
#undef CASE
        }
        if (d->n_groups) hipLaunchKernelGGL(rate_group_kernel, dim3(ceil_div(d->n_groups, 256)), dim3(256), 0, ctx->stream, *d);
    });
}

} // extern "C"
