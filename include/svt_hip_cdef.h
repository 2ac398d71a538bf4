/*
 * svt_hip_cdef.h -- C-ABI of the constrained directional enhancement filter (CDEF) of the MI355X path: the strength search
 * (cdef_seg_search, Source/Lib/Codec/cdef_process.c:106-349), the joint strength selection (finish_cdef_search, enc_cdef.c:728-965) and the
 * filter itself (svt_av1_cdef_frame, enc_cdef.c:284-610).  With the three a picture goes from the deblocked reconstruction to the CDEF-filtered
 * reconstruction and the frame header's strengths on the device; the host reads one SvtHipCdefPick and the per-block indices.
 *
 * Scope.  4:2:0 (the reference's search hard-codes it); 8-bit planes of uint8_t with coeff_shift 0 and 10-bit planes of uint16_t with
 * coeff_shift 2; picture width and height multiples of 8 (the encoder's aligned size, so mi_cols = width / 4); 64x64 filter blocks, in raster
 * order, n_fb = ceil(width / 64) * ceil(height / 64) of them.
 * What stays on the host: a picture coded with 128x128 superblocks; the 16-bit pipeline at 8-bit depth; 12-bit; me_based_cdef_skip;
 * use_reference_cdef_fs; the mode-info walk (svt_sb_compute_cdef_list, and the write of cdef_strength into the mode-info grid).
 * The host passes one uint64_t per filter block: bit by * 8 + bx is set for an 8x8 block to filter (the order of the reference's dlist).  The
 * kernels AND it with the mask of the blocks the filter block has inside the picture (nhb, nvb), so a stray bit cannot reach past the picture.
 *
 * A plane is given by the address of its sample (0, 0), its stride in samples and the size of the picture in that plane (chroma: half the
 * luma's each way).  Nothing outside the picture is read.
 *
 * svt_hip_cdef_search_batch.  For every filter block whose mask is not empty and every strength index gi < n_strengths -- the two passes' lists
 * concatenated -- the distortion of the filtered block against the source, bit-exact with cdef_seg_search over svt_cdef_filter_fb,
 * svt_cdef_filter_block_c, svt_aom_cdef_find_dir_c and svt_aom_compute_cdef_dist_{8bit_,}c:
 *   window      the filter block with 8 columns and 3 rows of unfiltered reconstruction from its neighbours; CDEF_VERY_LARGE (0x7F7F) on a side
 *               that is the picture's edge.  Such a tap takes part in the minimum, not in the maximum, and its constrained difference is 0
 *   direction   dir and var from the luma block, var = (best_cost - cost[(dir + 4) & 7]) >> 10, the first maximum wins; chroma uses luma's dir
 *   strengths   pri = v / 4, sec = v % 4, sec += (sec == 3), both << coeff_shift; damping 3 + (base_q_idx >> 6) + coeff_shift - (plane != 0).
 *               Luma filters with t = adjust_strength(pri, var), the tap set by (t >> coeff_shift) & 1, along pri ? dir : 0
 *   rows        subsampling_factor 1, 2 or 4, capped at 4 for luma and at 1 for chroma's 4x4 blocks: rows i % sf == 0 are filtered and
 *               measured, and the plane's sum is multiplied by sf
 *   distortion  luma: the five sums of the reference's dist_8xn and floor(.5 + (sum_d2 + sum_s2 - 2 sum_sd) * .5 * (svar + dvar + (400 << 2cs))
 *               / sqrt((20000 << 4cs) + svar * (double)dvar)) in IEEE double, left to right, with a correctly rounded root, summed over
 *               the listed blocks and then >> 2cs (svt_aom_compute_cdef_dist_c shifts the sum of every plane).  Chroma: the squared error
 *               >> 2cs of Cb, plus that of Cr.  strength_uv[gi] == -1: mse[1] = 1040400 * 64 and no chroma filter for gi
 * Outputs: mse[2][n_fb][64] (row 1 is Cb + Cr; entries gi >= n_strengths are not written), dir[n_fb][8][8] and var[n_fb][8][8] for listed
 * blocks only, and, when non-null, block_dist[n_fb][n_strengths][64]: the luma distortion per listed block (index by * 8 + bx) before the sum, its
 * shift and the multiplication by sf.  A filter block whose mask is empty gets nothing written.
 *
 * svt_hip_cdef_pick_batch.  finish_cdef_search without the mode-info writes, on mse and the masks where the search left them: the
 * zero_fs_cost_bias on mse[.][i][0] IN PLACE (so a second call on the same mse biases again), zero_cost, the greedy joint search for 1, 2, 4
 * and 8 strength pairs (75 calls of svt_search_one_dual, first minimum in raster order), the choice of cdef_bits by RDCOST with full_lambda, the
 * per-block index (first minimum among the chosen pairs) and cdef_dist_dev.  The strengths in SvtHipCdefPick are mapped through filter_map.
 * fb_strength[n_fb] is written for filter blocks with a non-empty mask only.  Sums are 64-bit integers, so their order does not matter.
 * The descriptor carries the luma picture's size so that "non-empty" means here what it means to the search: a mask whose bits all lie outside
 * the picture is a skipped filter block.  The two costs are RDCOST(full_lambda, av1_cost_literal(bits), dist << 4) as the reference forms them.
 *
 * svt_hip_cdef_apply_batch.  svt_av1_cdef_frame, out of place: from the unfiltered planes to three (n_planes == 1: one) distinct output planes.
 * fb_strength, y_strength and uv_strength are device pointers -- the pick's outputs, read where they lie.  A filter block is copied through when
 * the four strengths of its pair are 0 or its mask is empty, a plane of it when its two strengths are 0, and every block the mask does not list.
 * dir and var are computed from the input, never read from the search's arrays.  Always subsampling_factor 1.
 *
 * All three are asynchronous on the context stream; grids are sized by the picture.
 */
#ifndef SVT_HIP_CDEF_H
#define SVT_HIP_CDEF_H

#include <stdint.h>
#include <stddef.h>
#include "svt_hip_me.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVT_HIP_CDEF_MAX_STRENGTHS 64      /* TOTAL_STRENGTHS */
#define SVT_HIP_CDEF_MAX_PAIRS 8           /* CDEF_MAX_STRENGTHS */
#define SVT_HIP_CDEF_DEFAULT_MSE_UV (1040400ull * 64)

typedef struct SvtHipCdefPlane {
    void    *plane;           /* device pointer: sample (0, 0); uint8_t at 8 bits, uint16_t at 10 */
    uint32_t stride;          /* in samples */
    uint32_t width, height;   /* of the picture in this plane */
    uint32_t reserved;
} SvtHipCdefPlane;

typedef struct SvtHipCdefSearchDesc {
    uint32_t n_fb;            /* ceil(width / 64) * ceil(height / 64) of the luma plane; 0: nothing to do */
    uint8_t  bit_depth;       /* 8 or 10 */
    uint8_t  base_q_idx;      /* damping = 3 + (base_q_idx >> 6) */
    uint8_t  subsampling_factor; /* 1, 2 or 4 */
    uint8_t  n_strengths;     /* 1..64 */
    SvtHipCdefPlane recon[3]; /* the deblocked reconstruction: Y, Cb, Cr */
    SvtHipCdefPlane src[3];   /* the source */
    int8_t   strength_y[SVT_HIP_CDEF_MAX_STRENGTHS];  /* 0..63 */
    int8_t   strength_uv[SVT_HIP_CDEF_MAX_STRENGTHS]; /* -1 or 0..63 */
    const uint64_t *masks;    /* device pointer: [n_fb] */
    uint64_t *mse;            /* outputs, device pointers: [2][n_fb][64] */
    uint8_t  *dir;            /* [n_fb][8][8] */
    int32_t  *var;            /* [n_fb][8][8] */
    uint64_t *block_dist;     /* optional: [n_fb][n_strengths][64] */
} SvtHipCdefSearchDesc;

typedef struct SvtHipCdefPick {
    int32_t  cdef_bits;       /* 0..3 */
    int32_t  nb_strengths;    /* 1 << cdef_bits */
    int32_t  y_strength[SVT_HIP_CDEF_MAX_PAIRS];  /* strength values (through filter_map); entries past nb_strengths are 0 */
    int32_t  uv_strength[SVT_HIP_CDEF_MAX_PAIRS];
    uint64_t best_cost;       /* the winning RDCOST */
    uint64_t zero_cost;
    int32_t  cdef_dist_dev;
    int32_t  reserved;
} SvtHipCdefPick;

typedef struct SvtHipCdefPickDesc {
    uint32_t n_fb;            /* 0: nothing to do */
    uint32_t n_strengths;     /* 1..64 */
    uint32_t is_hbd;          /* which of the two bias rules: encoder_bit_depth > 8 */
    uint32_t zero_fs_cost_bias; /* 0 (none) or 10..64 */
    uint32_t full_lambda;
    uint32_t width, height;   /* of the luma picture, as in the search: the masks are ANDed with the blocks inside it here too */
    uint32_t reserved;
    uint8_t  filter_map_y[SVT_HIP_CDEF_MAX_STRENGTHS];  /* the strength value of an index */
    uint8_t  filter_map_uv[SVT_HIP_CDEF_MAX_STRENGTHS];
    const uint64_t *masks;    /* device pointers: [n_fb] */
    uint64_t *mse;            /* [2][n_fb][64], biased in place */
    void     *work;           /* svt_hip_cdef_pick_work_bytes() bytes of scratch, 8-byte aligned */
    SvtHipCdefPick *result;   /* outputs, device pointers */
    int8_t   *fb_strength;    /* [n_fb] */
} SvtHipCdefPickDesc;

typedef struct SvtHipCdefApplyDesc {
    uint32_t n_fb;            /* as in the search; 0: nothing to do */
    uint8_t  bit_depth;       /* 8 or 10 */
    uint8_t  cdef_damping;    /* 3..6 */
    uint8_t  n_planes;        /* 1 or 3 */
    uint8_t  reserved;
    SvtHipCdefPlane in[3];    /* the unfiltered planes */
    SvtHipCdefPlane out[3];   /* distinct from them and from each other */
    const uint64_t *masks;    /* device pointers: [n_fb] */
    const int8_t   *fb_strength; /* [n_fb]: the index of the filter block's pair; read for non-empty masks only */
    const int32_t  *y_strength;  /* [8]: SvtHipCdefPick.y_strength where the pick left it */
    const int32_t  *uv_strength; /* [8] */
} SvtHipCdefApplyDesc;

/* Each enqueues on the context stream (asynchronous), returns SVT_HIP_ERR_BAD_PARAM and enqueues nothing for what its check refuses, and returns 0
 * without touching the context for n_fb == 0. */
int    svt_hip_cdef_search_batch(SvtHipContext *ctx, const SvtHipCdefSearchDesc *d);
int    svt_hip_cdef_pick_batch(SvtHipContext *ctx, const SvtHipCdefPickDesc *d);
int    svt_hip_cdef_apply_batch(SvtHipContext *ctx, const SvtHipCdefApplyDesc *d);
/* Host-only validation.  Search: a null descriptor, masks, mse, dir or var; bit_depth other than 8 or 10; subsampling_factor other than 1, 2, 4;
 * n_strengths outside 1..64; strength_y outside 0..63 or strength_uv outside -1..63 below n_strengths; a plane that is null or has a zero size
 * or a stride below its width; a luma size that is no multiple of 8 or above 16384; a chroma size other than half the luma's; a source size other
 * than the reconstruction's; n_fb other than 0 or the picture's count. */
int    svt_hip_cdef_search_check_desc(const SvtHipCdefSearchDesc *d);
/* Pick: a null descriptor, masks, mse, work, result or fb_strength; work not 8-byte aligned; n_strengths outside 1..64; is_hbd above 1;
 * zero_fs_cost_bias other than 0 or 10..64; a width or height that is 0, no multiple of 8 or above 16384; n_fb other than 0 or the picture's count. */
int    svt_hip_cdef_pick_check_desc(const SvtHipCdefPickDesc *d);
/* Apply: a null descriptor, masks, fb_strength, y_strength or uv_strength; bit_depth other than 8 or 10; cdef_damping outside 3..6; n_planes other
 * than 1 or 3; the planes as in the search (in against out as recon against src); an output plane whose samples overlap an input plane's or
 * another output's; n_fb other than 0 or the picture's count. */
int    svt_hip_cdef_apply_check_desc(const SvtHipCdefApplyDesc *d);
/* Bytes of SvtHipCdefPickDesc.work (the same for every picture) */
size_t svt_hip_cdef_pick_work_bytes(void);

/* sizeof / offsetof as compiled, for the bindings: what = 0 the plane, 1 the search descriptor, 2 the pick result, 3 the pick descriptor, 4 the
 * apply descriptor; `field` < 0 the size, else the offset of the field-th member in declaration order ((size_t)-1 past the last) */
size_t svt_hip_cdef_layout(int what, int field);

#ifdef __cplusplus
}
#endif
#endif
