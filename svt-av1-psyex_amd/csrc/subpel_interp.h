// subpel_interp.h -- the interpolation of svt_aom_upsampled_pred, shared by the sub-pel searches that score an interpolated prediction
// (md_search_kernel.hip: svt_av1_find_best_sub_pixel_tree; obmc_kernel.hip: svt_av1_find_best_obmc_sub_pixel_tree_up).  The one place it is restated.
#ifndef SVT_HIP_SUBPEL_INTERP_H
#define SVT_HIP_SUBPEL_INTERP_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace {

// rows 0, 2, .. 14 of av1_bilinear_filters / av1_sub_pel_filters_4 / av1_sub_pel_filters_8 (C_DEFAULT/variance.c:72-135): what
// av1_get_interp_filter_subpel_kernel(av1_get_filter(subpel_search_type), subpel_q3 << 1) selects (:191-201, :219-222)
__device__ const int8_t c_subpel_filters[3][8][8] = {
    {{0, 0, 0, 127, 0, 0, 0, 0}, {0, 0, 0, 112, 16, 0, 0, 0}, {0, 0, 0, 96, 32, 0, 0, 0}, {0, 0, 0, 80, 48, 0, 0, 0}, {0, 0, 0, 64, 64, 0, 0, 0}, {0, 0, 0, 48, 80, 0, 0, 0},
     {0, 0, 0, 32, 96, 0, 0, 0}, {0, 0, 0, 16, 112, 0, 0, 0}},
    {{0, 0, 0, 127, 0, 0, 0, 0}, {0, 0, -8, 122, 18, -4, 0, 0}, {0, 0, -12, 110, 38, -8, 0, 0}, {0, 0, -14, 94, 58, -10, 0, 0}, {0, 0, -12, 76, 76, -12, 0, 0},
     {0, 0, -10, 58, 94, -14, 0, 0}, {0, 0, -8, 38, 110, -12, 0, 0}, {0, 0, -4, 18, 122, -8, 0, 0}},
    {{0, 0, 0, 127, 0, 0, 0, 0}, {0, 2, -10, 122, 18, -4, 0, 0}, {0, 2, -14, 110, 38, -10, 2, 0}, {0, 2, -16, 94, 58, -12, 2, 0}, {0, 2, -14, 76, 76, -14, 2, 0},
     {0, 2, -12, 58, 94, -16, 2, 0}, {0, 2, -10, 38, 110, -14, 2, 0}, {0, 0, -4, 18, 122, -10, 2, 0}}};
// (phase 0 -- weight 128, which an int8 cannot hold -- is never read: a pass with phase 0 is skipped, as in the reference)

__device__ __forceinline__ int clip_u8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// One sample of svt_aom_upsampled_pred (C_DEFAULT/variance.c:204-254; svt_aom_convolve8_horiz_c / _vert_c, Codec/convolve.c:244-301) at `r` (the
// sample at the MV's floor, row pitch `as`) for the 1/8 offsets (xo, yo) with the taps fx / fy of those offsets.  8 taps at offsets -3 .. +4,
// (sum + 64) >> 7 and a clip to 8 bits after EACH pass (the reference's intermediate is an 8-bit array): a 2-D position recomputes the eight
// horizontally filtered samples above and below itself (64 multiply-adds per pixel)
__device__ __forceinline__ int upsampled_sample(const uint8_t *r, uint32_t as, int xo, int yo, const int *fx, const int *fy) {
    int v;
    if (!xo && !yo)
        v = r[0];
    else if (!yo) {
        int t = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) t += (int)r[k - 3] * fx[k];
        v = clip_u8((t + 64) >> 7);
    } else if (!xo) {
        int t = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) t += (int)r[(ptrdiff_t)(k - 3) * (ptrdiff_t)as] * fy[k];
        v = clip_u8((t + 64) >> 7);
    } else {
        int t2 = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint8_t *rr = r + (ptrdiff_t)(j - 3) * (ptrdiff_t)as;
            int t = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) t += (int)rr[k - 3] * fx[k];
            t2 += clip_u8((t + 64) >> 7) * fy[j];
        }
        v = clip_u8((t2 + 64) >> 7);
    }
    return v;
}

} // namespace
#endif
