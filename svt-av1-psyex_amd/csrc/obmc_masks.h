// obmc_masks.h -- the 1-D OBMC mask rows, once: the AV1 specification's Obmc_Mask_2 .. Obmc_Mask_32 (svt_av1_get_obmc_mask,
// Source/Lib/Codec/inter_prediction.c:2406-2429), packed so that the row of length n lies at [n, 2n): byte 0 is unused, byte 1 is the row of length 1.
#ifndef SVT_HIP_OBMC_MASKS_H
#define SVT_HIP_OBMC_MASKS_H
#define SVT_HIP_OBMC_MASK_ROWS                                                                                                                   \
    {0,  64, 45, 64, 39, 50, 59, 64, 36, 42, 48, 53, 57, 61, 64, 64, 34, 37, 40, 43, 46, 49, 52, 54, 56, 58, 60, 61, 64, 64, 64, 64,             \
     33, 35, 36, 38, 40, 41, 43, 44, 45, 47, 48, 50, 51, 52, 53, 55, 56, 57, 58, 59, 60, 60, 61, 62, 64, 64, 64, 64, 64, 64, 64, 64}
#endif
