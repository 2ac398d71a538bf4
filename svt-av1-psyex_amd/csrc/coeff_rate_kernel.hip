// coeff_rate_kernel.hip -- the rate half of the RD cost on gfx950: svt_hip_coeff_rate_batch (coefficient rate estimation per job, the RD
// cost, the winner of every group of candidates).
//
// Reference functions restated (Source/Lib):
//   svt_av1_cost_coeffs_txb, allow_update_cdf == 0              Codec/rd_cost.c:434-559
//   svt_av1_txb_init_levels_c                                   Codec/rd_cost.c:99-111
//   svt_av1_get_nz_map_contexts_c, get_nz_map_ctx               C_DEFAULT/encode_txb_ref_c.c:17-40
//   get_nz_mag, get_nz_map_ctx_from_stats                       Codec/coefficients.h:2884-2943
//   get_br_ctx                                                  Codec/common_utils.h:114-151
//   get_eob_cost, get_eob_pos_token                             Codec/rd_cost.c:281-298,188-201
//   av1_transform_type_rate_estimation, get_ext_tx_set{,_type}  Codec/rd_cost.c:113-158, Codec/definitions.h:1787-1828
//   av1_cost_coeffs_txb_loop_cost_{one_,}eob                    Codec/rd_cost.c:310-431
//   svt_aom_txb_estimate_coeff_bits, av1_cost_skip_txb          Codec/rd_cost.c:1405-1450,299-308
//   the short-cuts and the winner of tx_type_search             Codec/product_coding_loop.c:4947-4952,4976-4985
//   RDCOST                                                      Codec/rd_cost.h:37
//
// A batch shares tx_size and plane_type, hence ONE LvMapCoeffCost and one LvMapEobCost: a workgroup of four waves copies both into LDS
// once and then walks its share of the jobs.  A group of G = min(64, coefficients) lanes takes one job, so a wave holds four 4x4 jobs,
// two 4x8 / 8x4 jobs, one job of any other size.  Every lane takes raster positions (four in a row from 256
// coefficients up), writes their clamped levels into the group's padded levels array in LDS (one byte per level, stride width + 4, four
// zero rows below: the lay-out of svt_av1_txb_init_levels_c without the two rows above, which nothing reads), and then adds the cost terms
// of its own positions: a position's place in the scan comes from the inverse scan table, its contexts from the levels array alone.
// There is no serial dependency, and the 32-bit sums of the lanes meet by cross-lane adds in any order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "svt_hip_internal.h"
#include "../../include/svt_hip_dsp.h"
#include "wave_ops.h"

namespace {

constexpr int kWaves      = 4;                   // waves of a workgroup
constexpr int kCoeffInts  = sizeof(SvtHipLvMapCoeffCost) / 4;
constexpr int kEobInts    = sizeof(SvtHipLvMapEobCost) / 4;
constexpr int kLevelBytes = (32 + 4) * (32 + 4); // TX_PAD_HOR = 4 columns, TX_PAD_BOTTOM = 4 rows
constexpr int kMaxGrid    = 2048;
constexpr uint32_t kCostLiteral = 512;           // av1_cost_literal(1)

struct RateParams {
    SvtHipCoeffRateDesc d;
    const int16_t *iscan[3];  // default, row (V_*), column (H_*) inverse scans of this tx_size
    int      bwl, w, h;       // get_txb_bwl_tab / get_txb_wide_tab / get_txb_high_tab: the packed block
    int      txs_ctx;         // (txsize_sqr_map + txsize_sqr_up_map + 1) >> 1
    int      eob_multi;       // txsize_log2_minus4
    int      shape;           // 0 square, 1 tx width < tx height, 2 tx width > tx height (the real dimensions)
    int      ext_set[2];      // get_ext_tx_set(tx_size, is_inter, reduced) by is_inter, 0 where get_ext_tx_types <= 1
    int      sq;              // txsize_sqr_map
    uint32_t th;              // (tx_width * tx_height) >> 6
    uint32_t c_div;           // MAX(1, mds_fast_coeff_est_level - mds_subres_step)
    uint32_t n_packs;
};

// get_golomb_cost (rd_cost.c:90-97) of a level >= 1 + NUM_BASE_LEVELS + COEFF_BASE_RANGE = 15
__device__ __forceinline__ uint32_t golomb_cost(uint32_t a) { return kCostLiteral * (2u * (32u - (uint32_t)__builtin_clz(a - 14u)) - 1u); }

// lps_cost[ctx][min(level - 1 - NUM_BASE_LEVELS, COEFF_BASE_RANGE)] (+ the Golomb tail) of a level above NUM_BASE_LEVELS
__device__ __forceinline__ uint32_t range_cost(const SvtHipLvMapCoeffCost *cc, int br, uint32_t a) {
    const uint32_t base_range = a - 3u;
    return (uint32_t)cc->lps_cost[br][base_range < 12u ? base_range : 12u] + (a >= 15u ? golomb_cost(a) : 0u);
}

// The cost terms of the coefficient at raster position `pos` (scan index si < eob) of a block with eob >= 2; `bad` is set where the reference
// would index base_eob_cost[..][-1].  lev: the group's levels array.
__device__ __forceinline__ uint32_t position_cost(const RateParams &p, const SvtHipLvMapCoeffCost *cc, const uint8_t *lev, int cls, int n, uint32_t eob,
                                                  uint32_t c_start, int dc_sign_ctx, int pos, uint32_t si, int32_t v, uint32_t &bad) {
    const bool last = si == eob - 1u;
    if (!last && si > c_start) return 0u; // si == 0 is the DC: always counted
    const uint32_t a      = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
    const int      stride = p.w + 4, row = pos >> p.bwl, col = pos - (row << p.bwl);
    const uint8_t *l      = lev + row * stride + col;
    uint32_t       cost   = 0;
    if (last) { // rd_cost.c:351-376; get_nz_map_ctx with is_eob (encode_txb_ref_c.c:19-27)
        if (a == 0u) { bad = 1u; return 0u; }
        const int ctx = si <= (uint32_t)(n >> 3) ? 1 : (si <= (uint32_t)(n >> 2) ? 2 : 3);
        cost = (uint32_t)cc->base_eob_cost[ctx][(a < 3u ? a : 3u) - 1u] + kCostLiteral;
    } else { // the DC (:377-404) and the middle loop (:410-427)
        int mag = (l[1] < 3 ? l[1] : 3) + (l[stride] < 3 ? l[stride] : 3); // get_nz_mag: clip_max3 of {0,1}, {1,0}
        int off;
        if (cls == 0) { // {1,1}, {0,2}, {2,0}
            mag += (l[stride + 1] < 3 ? l[stride + 1] : 3) + (l[2] < 3 ? l[2] : 3) + (l[2 * stride] < 3 ? l[2 * stride] : 3);
            // the rule behind eb_av1_nz_map_ctx_offset (coefficients.h:2918-2928), on the real transform dimensions
            if (p.shape == 1 && row < 2) off = 11;
            else if (p.shape == 2 && col < 2) off = 16;
            else off = row + col < 2 ? 1 : (row + col < 4 ? 6 : 21);
        } else if (cls == 2) { // TX_CLASS_VERT: {2,0}, {3,0}, {4,0}
            mag += (l[2 * stride] < 3 ? l[2 * stride] : 3) + (l[3 * stride] < 3 ? l[3 * stride] : 3) + (l[4 * stride] < 3 ? l[4 * stride] : 3);
            off = row == 0 ? 26 : (row == 1 ? 31 : 36); // nz_map_ctx_offset_1d
        } else { // TX_CLASS_HORIZ: {0,2}, {0,3}, {0,4}
            mag += (l[2] < 3 ? l[2] : 3) + (l[3] < 3 ? l[3] : 3) + (l[4] < 3 ? l[4] : 3);
            off = col == 0 ? 26 : (col == 1 ? 31 : 36);
        }
        int ctx = (mag + 1) >> 1;
        ctx     = (ctx < 4 ? ctx : 4) + off;
        if ((cls | pos) == 0) ctx = 0;
        cost = (uint32_t)cc->base_cost[ctx][a < 3u ? a : 3u];
        if (a != 0u) cost += pos == 0 ? (uint32_t)cc->dc_sign_cost[dc_sign_ctx][v < 0 ? 1 : 0] : kCostLiteral;
    }
    if (a > 2u) { // get_br_ctx (common_utils.h:114-151)
        int  mag = l[1] + l[stride];
        bool near;
        if (cls == 0) { mag += l[stride + 1]; near = row < 2 && col < 2; }
        else if (cls == 1) { mag += l[2]; near = col == 0; }
        else { mag += l[2 * stride]; near = row == 0; }
        mag = (mag + 1) >> 1;
        mag = mag < 6 ? mag : 6;
        cost += range_cost(cc, pos == 0 ? mag : mag + (near ? 7 : 14), a);
    }
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
    {
        const int32_t *src_c = reinterpret_cast<const int32_t *>(&p.d.tables->coeff_fac_bits[p.txs_ctx][p.d.plane_type]);
        const int32_t *src_e = reinterpret_cast<const int32_t *>(&p.d.tables->eob_frac_bits[p.eob_multi][p.d.plane_type]);
        for (int i = threadIdx.x; i < kCoeffInts + kEobInts; i += 64 * kWaves) tab[i] = i < kCoeffInts ? src_c[i] : src_e[i - kCoeffInts];
    }
    __syncthreads();
    const SvtHipLvMapCoeffCost *cc = reinterpret_cast<const SvtHipLvMapCoeffCost *>(tab);
    const SvtHipLvMapEobCost   *ec = reinterpret_cast<const SvtHipLvMapEobCost *>(tab + kCoeffInts);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, grp = lane / G, gl = lane % G;
    const int stride = p.w + 4, lev_bytes = stride * (p.h + 4); // a multiple of 16
    uint8_t  *lev = levels[wave] + grp * lev_bytes;
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
        if (p.d.plane_type == 0 && lvl != 1 && eob < p.th) bits = 6000ull + (uint64_t)eob * 1000ull;
        else if (p.d.plane_type == 0 && lvl == 0) bits = 3000ull + (uint64_t)eob * 100ull;
        else if (jb.txb_skip_ctx >= 13) bits = ~0ull; // a context outside its table: undefined, nothing is read
        else if (eob == 0) bits = (uint64_t)(int64_t)cc->txb_skip_cost[jb.txb_skip_ctx][1]; // av1_cost_skip_txb
        else // intra_dir is read by intra luma jobs alone (rd_cost.c:137-153): an inter candidate's pred_mode is 13 or above and is fine
            compute = valid && eob <= (uint32_t)N && jb.tx_type < 16 && jb.dc_sign_ctx < 3 && (p.d.plane_type != 0 || jb.is_inter || jb.intra_dir < 13);
        const int      kind    = jb.tx_type >= 10 ? ((jb.tx_type & 1) ? 2 : 1) : 0; // the scan: default, rows (V_*), columns (H_*)
        const int      cls     = jb.tx_type >= 10 ? ((jb.tx_type & 1) ? 1 : 2) : 0; // tx_type_to_class: TX_CLASS_2D / HORIZ / VERT
        const uint32_t c_start = eob >= 2 ? (eob - 2u < eob / p.c_div ? eob - 2u : eob / p.c_div) : 0u; // rd_cost.c:408

        // svt_av1_txb_init_levels_c: min(|qcoeff|, 127) over the WHOLE block, in a zero frame
        for (int i = gl * 16; i < lev_bytes; i += G * 16) *reinterpret_cast<uint4 *>(lev + i) = make_uint4(0, 0, 0, 0);
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
            const int row = pos >> p.bwl, col = pos - (row << p.bwl); // four positions in a row never straddle rows: the width is a multiple of 4
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
                        if (a > 2u) cost += range_cost(cc, 0, a);
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
                        if (s < eob) cost += position_cost(p, cc, lev, cls, N, eob, c_start, jb.dc_sign_ctx, pos + v, s, q[v], bad);
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
                        cost += (uint32_t)(inter ? p.d.tables->inter_tx_type_fac_bits[set][p.sq][jb.tx_type]
                                                 : p.d.tables->intra_tx_type_fac_bits[set][p.sq][jb.intra_dir][jb.tx_type]);
                }
                // get_eob_pos_token: 1, 2, then one token per power of two: eb_k_eob_group_start = 0 1 2 3 5 9 17 .. 513, eb_k_eob_offset_bits = 0 0 0 1 2 .. 9
                const int eob_pt = 33 - (eob > 1 ? __builtin_clz(eob - 1u) : 32);
                cost += (uint32_t)ec->eob_cost[cls == 0 ? 0 : 1][eob_pt - 1];
                if (eob_pt > 2) {
                    const int      offset_bits = eob_pt - 2;
                    const uint32_t eob_extra   = eob - ((1u << offset_bits) + 1u);
                    cost += (uint32_t)cc->eob_extra_cost[eob_pt - 3][(eob_extra >> (offset_bits - 1)) & 1u];
                    if (offset_bits > 1) cost += kCostLiteral * (uint32_t)(offset_bits - 1);
                }
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

const int kTxW[19]      = {4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64};
const int kTxH[19]      = {4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16};
const int kSqrMap[19]   = {0, 1, 2, 3, 4, 0, 0, 1, 1, 2, 2, 3, 3, 0, 0, 1, 1, 2, 2}; // txsize_sqr_map (Codec/definitions.h:1509)
const int kSqrUpMap[19] = {0, 1, 2, 3, 4, 1, 1, 2, 2, 3, 3, 4, 4, 2, 2, 3, 3, 4, 4}; // txsize_sqr_up_map (:1530)
const int kLog2M4[19]   = {0, 2, 4, 6, 6, 1, 1, 3, 3, 5, 5, 6, 6, 2, 2, 4, 4, 5, 5}; // txsize_log2_minus4 (Codec/inv_transforms.h:329)

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

int svt_hip_coeff_rate_batch(SvtHipContext *ctx, const SvtHipCoeffRateDesc *d) {
    if (!ctx || !d) return svt_hip_fail(nullptr, SVT_HIP_ERR_BAD_PARAM, "svt_hip_coeff_rate_batch: null context or descriptor");
    if (d->tx_size >= SVT_HIP_TX_SIZES_ALL || d->plane_type > 1)
        return svt_hip_fail(ctx, SVT_HIP_ERR_BAD_PARAM, "svt_hip_coeff_rate_batch: tx_size %u (below 19) / plane_type %u (0 or 1)", d->tx_size, d->plane_type);
    if (d->mds_subres_step > 2 || d->mds_fast_coeff_est_level == 0)
        return svt_hip_fail(ctx, SVT_HIP_ERR_BAD_PARAM, "svt_hip_coeff_rate_batch: mds_subres_step %u (0..2) / mds_fast_coeff_est_level %u (not 0)",
                            d->mds_subres_step, d->mds_fast_coeff_est_level);
    if (!d->jobs || !d->tables || !d->qcoeff || !d->eob || !d->bits)
        return svt_hip_fail(ctx, SVT_HIP_ERR_BAD_PARAM, "svt_hip_coeff_rate_batch: a mandatory pointer (jobs, tables, qcoeff, eob, bits) is null");
    if (((uintptr_t)d->qcoeff & 15) && (kTxW[d->tx_size] > 32 ? 32 : kTxW[d->tx_size]) * (kTxH[d->tx_size] > 32 ? 32 : kTxH[d->tx_size]) >= 256)
        return svt_hip_fail(ctx, SVT_HIP_ERR_BAD_PARAM, "svt_hip_coeff_rate_batch: qcoeff is not 16-byte aligned (sizes of 256 coefficients and more are read 16 bytes at a time)");
    if (d->rd_cost && !d->dist) return svt_hip_fail(ctx, SVT_HIP_ERR_BAD_PARAM, "svt_hip_coeff_rate_batch: rd_cost without dist");
    const bool groups = d->n_groups || d->group_start || d->best_job || d->best_cost;
    if (groups && !d->rd_cost) return svt_hip_fail(ctx, SVT_HIP_ERR_BAD_PARAM, "svt_hip_coeff_rate_batch: groups without rd_cost");
    if (groups && (!d->group_start || !d->best_job || !d->best_cost))
        return svt_hip_fail(ctx, SVT_HIP_ERR_BAD_PARAM, "svt_hip_coeff_rate_batch: groups need group_start, best_job and best_cost");
    if (d->n_jobs == 0 && d->n_groups == 0) return SVT_HIP_OK;
    hipSetDevice(ctx->device);
    const int ts = d->tx_size;
    RateParams p;
    memset(&p, 0, sizeof(p));
    p.d = *d;
    for (int k = 0; k < 3; k++) p.iscan[k] = ctx->iscan_dev + ((size_t)ts * 3 + k) * 1024;
    p.w = kTxW[ts] > 32 ? 32 : kTxW[ts];
    p.h = kTxH[ts] > 32 ? 32 : kTxH[ts];
    p.bwl = p.w == 4 ? 2 : (p.w == 8 ? 3 : (p.w == 16 ? 4 : 5));
    p.txs_ctx   = (kSqrMap[ts] + kSqrUpMap[ts] + 1) >> 1;
    p.eob_multi = kLog2M4[ts];
    p.shape     = kTxW[ts] < kTxH[ts] ? 1 : (kTxW[ts] > kTxH[ts] ? 2 : 0);
    p.sq        = kSqrMap[ts];
    for (int inter = 0; inter < 2; inter++) p.ext_set[inter] = ext_tx_set(ts, inter, d->reduced_tx_set != 0);
    p.th    = (uint32_t)(kTxW[ts] * kTxH[ts]) >> 6;
    p.c_div = d->mds_fast_coeff_est_level > d->mds_subres_step ? (uint32_t)(d->mds_fast_coeff_est_level - d->mds_subres_step) : 1u;
    const int n   = p.w * p.h;
    const int jpw = n >= 64 ? 1 : 64 / n;
    p.n_packs     = (d->n_jobs + (uint32_t)jpw - 1) / (uint32_t)jpw;
    std::lock_guard<std::mutex> lock(ctx->async_mu); // the winners' launch follows its own costs' when several threads enqueue
    if (d->n_jobs) {
        uint32_t grid = (p.n_packs + kWaves - 1) / kWaves;
        grid = grid < (uint32_t)kMaxGrid ? grid : (uint32_t)kMaxGrid;
        switch (n) {
#define CASE(N) case N: hipLaunchKernelGGL(coeff_rate_kernel<N>, dim3(grid), dim3(64 * kWaves), 0, ctx->stream, p); break;
            CASE(16) CASE(32) CASE(64) CASE(128) CASE(256) CASE(512) CASE(1024)
#undef CASE
        default: return svt_hip_fail(ctx, SVT_HIP_ERR_BAD_PARAM, "svt_hip_coeff_rate_batch: %d coefficients", n);
        }
        SVT_HIP_CHECK(ctx, hipGetLastError());
    }
    if (d->n_groups) {
        hipLaunchKernelGGL(rate_group_kernel, dim3((d->n_groups + 255) / 256), dim3(256), 0, ctx->stream, *d);
        SVT_HIP_CHECK(ctx, hipGetLastError());
    }
    return SVT_HIP_OK;
}

} // extern "C"
