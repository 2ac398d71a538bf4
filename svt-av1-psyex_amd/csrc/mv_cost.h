// mv_cost.h -- the MV rate term of the mode-decision motion searches (pme_kernel.hip, md_search_kernel.hip, obmc_kernel.hip): the reference's
// svt_mv_err_cost (Codec/mcomp.c:44-69; mcomp.h:135-138, rd_cost.c:55-60) with its six cost modes, the one place it is restated.
#ifndef SVT_HIP_MV_COST_H
#define SVT_HIP_MV_COST_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/svt_hip_pme.h"

namespace {

__device__ __forceinline__ int clip3(int lo, int hi, int v) { return v < lo ? lo : (v > hi ? hi : v); }

struct MvCost {
    SvtHipMv       ref_mv;
    int            type, error_per_bit; // type: SVT_HIP_MV_COST_*
    const int32_t *mvjcost, *row, *col; // the joint and the component cost tables, read for SVT_HIP_MV_COST_ENTROPY only
};

// svt_mv_err_cost of the int16 vector (row, col) against m.ref_mv
__device__ __forceinline__ int mv_err_cost(int16_t row, int16_t col, const MvCost &m) {
    const int16_t dr = (int16_t)(row - m.ref_mv.row), dc = (int16_t)(col - m.ref_mv.col); // MV fields are int16
    const int16_t ar = (int16_t)(dr < 0 ? -dr : dr), ac = (int16_t)(dc < 0 ? -dc : dc);
    switch (m.type) {
    case SVT_HIP_MV_COST_ENTROPY: {
        const int joint = dr == 0 ? (dc == 0 ? 0 : 1) : (dc == 0 ? 2 : 3); // svt_av1_get_mv_joint
        const int bits  = m.mvjcost[joint] + m.row[clip3(-(1 << 14), 1 << 14, dr)] + m.col[clip3(-(1 << 14), 1 << 14, dc)];
        return (int)((((long long)bits * m.error_per_bit) + (1ll << 13)) >> 14); // ROUND_POWER_OF_TWO_64(.., RDDIV_BITS + AV1_PROB_COST_SHIFT - RD_EPB_SHIFT + 4)
    }
    case SVT_HIP_MV_COST_L1_LOWRES: return (2 * (ar + ac)) >> 3;
    case SVT_HIP_MV_COST_L1_MIDRES: return 0;
    case SVT_HIP_MV_COST_L1_HDRES: return (ar + ac) >> 3;
    case SVT_HIP_MV_COST_OPT: return (int)((((long long)((ar + ac) << 8) * m.error_per_bit) + (1ll << 13)) >> 14);
    default: return 0;
    }
}

// svt_aom_mv_err_cost_light (Codec/av1me.c:229-235): what the warped-motion refinement (warp_kernel.hip) adds instead when approx_inter_rate is
// set; svt_aom_mv_err_cost (:244-252) itself is the SVT_HIP_MV_COST_ENTROPY case above
__device__ __forceinline__ int mv_err_cost_light(int row, int col, const SvtHipMv &ref_mv) {
    const int dr = row - ref_mv.row, dc = col - ref_mv.col; // int arithmetic on the int16 fields: no wrap
    return (int)(1296u + 50u * (uint32_t)((dr < 0 ? -dr : dr) + (dc < 0 ? -dc : dc)));
}

// mvsad_err_cost (Codec/av1me.c:237-261) of the FULL-PEL vector (row, col) against the full-pel centre (ref_mv >> 3): the light form when
// approx_inter_rate is set, else svt_mv_cost of the difference in 1/8 sample (an MV: int16) times sad_per_bit, rounded by AV1_PROB_COST_SHIFT = 9
__device__ __forceinline__ int mvsad_err_cost(int row, int col, int crow, int ccol, bool light, int sad_per_bit, const int32_t *mvjcost, const int32_t *trow,
                                              const int32_t *tcol) {
    const int dr = row - crow, dc = col - ccol;
    if (light) return (int)(1296u + 50u * ((uint32_t)(dc < 0 ? -dc : dc) * 8u + (uint32_t)(dr < 0 ? -dr : dr) * 8u));
    const int16_t r8 = (int16_t)(dr * 8), c8 = (int16_t)(dc * 8);
    const int joint = r8 == 0 ? (c8 == 0 ? 0 : 1) : (c8 == 0 ? 2 : 3);
    const int bits  = mvjcost[joint] + trow[clip3(-(1 << 14), 1 << 14, r8)] + tcol[clip3(-(1 << 14), 1 << 14, c8)];
    return (int)(((uint32_t)bits * (uint32_t)sad_per_bit + 256u) >> 9);
}

// svt_av1_mv_bit_cost with MV_COST_WEIGHT = 108, or svt_av1_mv_bit_cost_light (Codec/rd_cost.c:61-87)
__device__ __forceinline__ int mv_bit_cost(int row, int col, const SvtHipMv &ref_mv, bool light, const int32_t *mvjcost, const int32_t *trow, const int32_t *tcol) {
    if (light) return mv_err_cost_light(row, col, ref_mv);
    const int dr = clip3(-(1 << 14), 1 << 14, (int16_t)(row - ref_mv.row)), dc = clip3(-(1 << 14), 1 << 14, (int16_t)(col - ref_mv.col)); // temp_diff is an MV
    const int joint = dr == 0 ? (dc == 0 ? 0 : 1) : (dc == 0 ? 2 : 3);
    return ((mvjcost[joint] + trow[dr] + tcol[dc]) * 108 + 64) >> 7;
}

} // namespace
#endif
