// lvmap_core.h -- what the kernels that cost AV1's level map share (coeff_rate_kernel.hip, rdoq_kernel.hip): the context rules, the cost terms,
// the wave scaffolding and the host-side geometry, each reference function restated once, on int as the reference has it.
//
// A batch shares tx_size and plane_type, hence ONE LvMapCoeffCost and one LvMapEobCost: a workgroup of kWaves waves copies both into LDS once
// and then walks its share of the jobs.  A group of G = min(64, coefficients) lanes takes one job, so a wave holds four 4x4 jobs, two 4x8 / 8x4
// jobs, one job of any other size (a "pack").  A group keeps its job's padded levels array in LDS: one byte per level, stride width + 4, four
// zero rows below -- the lay-out of svt_av1_txb_init_levels_c (Codec/rd_cost.c:99-111) without the two rows above, which nothing reads.
#ifndef SVT_HIP_LVMAP_CORE_H
#define SVT_HIP_LVMAP_CORE_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/svt_hip_dsp.h"
#include "tx_geom.h"

namespace {

constexpr int kWaves       = 4;                   // waves of a workgroup
constexpr int kCoeffInts   = sizeof(SvtHipLvMapCoeffCost) / 4;
constexpr int kEobInts     = sizeof(SvtHipLvMapEobCost) / 4;
constexpr int kLevelBytes  = (32 + 4) * (32 + 4); // TX_PAD_HOR = 4 columns, TX_PAD_BOTTOM = 4 rows
constexpr int kMaxGrid     = 2048;
constexpr int kCostLiteral = 512;                 // av1_cost_literal(1)

// ---- host: what a tx_size means to these kernels
constexpr int kSqrMap[19]   = {0, 1, 2, 3, 4, 0, 0, 1, 1, 2, 2, 3, 3, 0, 0, 1, 1, 2, 2}; // txsize_sqr_map (Codec/definitions.h:1509)
constexpr int kSqrUpMap[19] = {0, 1, 2, 3, 4, 1, 1, 2, 2, 3, 3, 4, 4, 2, 2, 3, 3, 4, 4}; // txsize_sqr_up_map (:1530)
constexpr int kLog2M4[19]   = {0, 2, 4, 6, 6, 1, 1, 3, 3, 5, 5, 6, 6, 2, 2, 4, 4, 5, 5}; // txsize_log2_minus4 (Codec/inv_transforms.h:329)

struct LvMapGeom {
    int w, h, bwl, n;  // get_txb_wide_tab / get_txb_high_tab / get_txb_bwl_tab: the packed block (64 -> 32) and its coefficients
    int txs_ctx;       // (txsize_sqr_map + txsize_sqr_up_map + 1) >> 1
    int eob_multi;     // txsize_log2_minus4
    int shape;         // 0 square, 1 tx width < tx height, 2 tx width > tx height (the real dimensions)
    int sq;            // txsize_sqr_map
    int log_scale;     // av1_get_tx_scale_tab
    int area;          // tx_width * tx_height, the real dimensions
    int jobs_per_wave;
};
inline LvMapGeom lvmap_geom(int ts) {
    const int tw = tx_wide(ts), th = tx_high(ts);
    LvMapGeom g;
    g.w = tw > 32 ? 32 : tw;
    g.h = th > 32 ? 32 : th;
    g.bwl = ilog2c(g.w);
    g.n = g.w * g.h;
    g.txs_ctx = (kSqrMap[ts] + kSqrUpMap[ts] + 1) >> 1;
    g.eob_multi = kLog2M4[ts];
    g.shape = tw < th ? 1 : (tw > th ? 2 : 0);
    g.sq = kSqrMap[ts];
    g.log_scale = tx_log_scale(ts);
    g.area = tw * th;
    g.jobs_per_wave = g.n >= 64 ? 1 : 64 / g.n;
    return g;
}
// the packs of n_jobs jobs, and the grid of at most max_grid workgroups (0: kMaxGrid) that walks them wave-strided
inline uint32_t lvmap_grid(const LvMapGeom &g, uint32_t n_jobs, uint32_t max_grid, uint32_t &n_packs) {
    const uint32_t jpw = (uint32_t)g.jobs_per_wave;
    n_packs = n_jobs / jpw + (n_jobs % jpw != 0); // no sum that could wrap
    const uint32_t grid = n_packs / kWaves + (n_packs % kWaves != 0), cap = max_grid ? max_grid : (uint32_t)kMaxGrid;
    return grid < cap ? grid : cap;
}

// ---- device: the scaffolding
// coeff_fac_bits[txs_ctx][plane_type] and eob_frac_bits[eob_multi][plane_type] into tab[kCoeffInts + kEobInts] of LDS, by the whole workgroup
__device__ __forceinline__ void stage_cost_tables(int32_t *tab, const SvtHipRateTables *t, int txs_ctx, int eob_multi, int plane_type) {
    const int32_t *src_c = reinterpret_cast<const int32_t *>(&t->coeff_fac_bits[txs_ctx][plane_type]);
    const int32_t *src_e = reinterpret_cast<const int32_t *>(&t->eob_frac_bits[eob_multi][plane_type]);
    for (int i = threadIdx.x; i < kCoeffInts + kEobInts; i += 64 * kWaves) tab[i] = i < kCoeffInts ? src_c[i] : src_e[i - kCoeffInts];
    __syncthreads();
}
// the zero frame of a group's levels array (lev_bytes = (w + 4) * (h + 4), a multiple of 16), by the group's G lanes
template <int G> __device__ __forceinline__ void zero_levels(uint8_t *lev, int lev_bytes, int gl) {
    for (int i = gl * 16; i < lev_bytes; i += G * 16) *reinterpret_cast<uint4 *>(lev + i) = make_uint4(0, 0, 0, 0);
}
// the scan of a tx_type: 0 default, 1 rows (V_*), 2 columns (H_*); tx_type_to_class: 0 TX_CLASS_2D, 1 HORIZ, 2 VERT
__device__ __forceinline__ int tx_scan_kind(int tx_type) { return tx_type >= 10 ? ((tx_type & 1) ? 2 : 1) : 0; }
__device__ __forceinline__ int tx_class(int tx_type) { return tx_type >= 10 ? ((tx_type & 1) ? 1 : 2) : 0; }

// ---- device: the context rules.  What they need of a job's block:
struct LvBlk {
    const uint8_t *lev; // the group's levels array
    int stride, bwl, shape, cls, n; // stride = (1 << bwl) + 4; shape as in LvMapGeom; cls: tx_class(); n coefficients
};

__device__ __forceinline__ int min3(int v) { return v < 3 ? v : 3; }
// get_lower_levels_ctx = get_nz_map_ctx without is_eob (Codec/coefficients.h:2884-2950, C_DEFAULT/encode_txb_ref_c.c:17-40): get_nz_mag over
// the class's five neighbours, get_nz_map_ctx_from_stats
__device__ __forceinline__ int lower_ctx(const LvBlk &b, int pos) {
    const int      row = pos >> b.bwl, col = pos - (row << b.bwl), stride = b.stride;
    const uint8_t *l = b.lev + pos + (row << 2); // get_padded_idx (coefficients.h:2882): stride = width + TX_PAD_HOR
    int mag = min3(l[1]) + min3(l[stride]), off; // {0,1}, {1,0}
    if (b.cls == 0) { // {1,1}, {0,2}, {2,0}
        mag += min3(l[stride + 1]) + min3(l[2]) + min3(l[2 * stride]);
        // the rule behind eb_av1_nz_map_ctx_offset (coefficients.h:2918-2928), on the real transform dimensions
        if (b.shape == 1 && row < 2) off = 11;
        else if (b.shape == 2 && col < 2) off = 16;
        else off = row + col < 2 ? 1 : (row + col < 4 ? 6 : 21);
    } else if (b.cls == 2) { // TX_CLASS_VERT: {2,0}, {3,0}, {4,0}
        mag += min3(l[2 * stride]) + min3(l[3 * stride]) + min3(l[4 * stride]);
        off = row == 0 ? 26 : (row == 1 ? 31 : 36); // nz_map_ctx_offset_1d
    } else { // TX_CLASS_HORIZ: {0,2}, {0,3}, {0,4}
        mag += min3(l[2]) + min3(l[3]) + min3(l[4]);
        off = col == 0 ? 26 : (col == 1 ? 31 : 36);
    }
    const int ctx = (mag + 1) >> 1;
    return (b.cls | pos) == 0 ? 0 : (ctx < 4 ? ctx : 4) + off; // the DC of a 2-D class: context 0
}
// get_lower_levels_ctx_eob (coefficients.h:2851-2860) = get_nz_map_ctx with is_eob (encode_txb_ref_c.c:19-27), of the coefficient at scan index si
__device__ __forceinline__ int eob_ctx(const LvBlk &b, int si) { return si == 0 ? 0 : (si <= (b.n >> 3) ? 1 : (si <= (b.n >> 2) ? 2 : 3)); }
__device__ __forceinline__ bool near_origin(const LvBlk &b, int pos) {
    const int row = pos >> b.bwl, col = pos - (row << b.bwl);
    return b.cls == 0 ? (row < 2 && col < 2) : (b.cls == 1 ? col == 0 : row == 0);
}
// get_br_ctx_eob (coefficients.h:2861-2881) / get_br_ctx (Codec/common_utils.h:114-151)
__device__ __forceinline__ int br_ctx_eob(const LvBlk &b, int pos) { return pos == 0 ? 0 : (near_origin(b, pos) ? 7 : 14); }
__device__ __forceinline__ int br_ctx(const LvBlk &b, int pos) {
    const int      row = pos >> b.bwl, col = pos - (row << b.bwl), stride = b.stride;
    const uint8_t *l = b.lev + pos + (row << 2);
    int  mag = l[1] + l[stride];
    bool near;
    if (b.cls == 0) { mag += l[stride + 1]; near = row < 2 && col < 2; }
    else if (b.cls == 1) { mag += l[2]; near = col == 0; }
    else { mag += l[2 * stride]; near = row == 0; }
    mag = (mag + 1) >> 1;
    mag = mag < 6 ? mag : 6;
    return pos == 0 ? mag : mag + (near ? 7 : 14);
}

// ---- device: the cost terms
// get_golomb_cost (rd_cost.c:90-97) of a level >= 1 + NUM_BASE_LEVELS + COEFF_BASE_RANGE = 15
__device__ __forceinline__ int golomb_cost(int a) { return kCostLiteral * (2 * (32 - __builtin_clz((uint32_t)(a - 14))) - 1); }
// get_br_cost: lps_cost[ctx][min(level - 1 - NUM_BASE_LEVELS, COEFF_BASE_RANGE)] (+ the Golomb tail) of a level above NUM_BASE_LEVELS
__device__ __forceinline__ int range_cost(const SvtHipLvMapCoeffCost *cc, int br, int a) {
    const int base_range = a - 3;
    return cc->lps_cost[br][base_range < 12 ? base_range : 12] + (a >= 15 ? golomb_cost(a) : 0);
}
// get_eob_cost (rd_cost.c:281-298, full_loop.c:694-711).  get_eob_pos_token (rd_cost.c:188-201) in closed form: 1, 2, then one token per power of
// two: eb_k_eob_group_start = 0 1 2 3 5 9 17 .. 513, eb_k_eob_offset_bits = 0 0 0 1 2 .. 9
__device__ __forceinline__ int eob_cost(const SvtHipLvMapCoeffCost *cc, const SvtHipLvMapEobCost *ec, int cls, int eob) {
    const int eob_pt = 33 - (eob > 1 ? __builtin_clz((uint32_t)eob - 1u) : 32);
    int cost = ec->eob_cost[cls == 0 ? 0 : 1][eob_pt - 1];
    if (eob_pt > 2) {
        const int offset_bits = eob_pt - 2, eob_extra = eob - ((1 << offset_bits) + 1);
        cost += cc->eob_extra_cost[eob_pt - 3][(eob_extra >> (offset_bits - 1)) & 1];
        if (offset_bits > 1) cost += kCostLiteral * (offset_bits - 1);
    }
    return cost;
}

} // namespace
#endif
