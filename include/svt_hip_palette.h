/*
 * svt_hip_palette.h -- C-ABI of the batched luma palette search of the MI355X path, of the palette rate of every candidate it keeps, and of the
 * palette prediction that follows it on the device.
 *
 * One search job = one call of search_palette_luma (Source/Lib/Codec/palette.c:303-428) for a luma block, followed by the palette branch of the luma
 * rate (Codec/rd_cost.c:679-706) for every candidate the search keeps:
 *   count     svt_av1_count_colors{,_highbd} (Codec/pic_analysis_process.c:1809-1846) over the rows x cols samples inside the picture; a 10-bit sample
 *             >= 1 << bit_depth gives 0 colours; the search runs when 1 < colours <= 64, else n_cands = 0
 *   dominant  top_colors: the min(colours, 8) most frequent values, the lower value first among equal counts; candidates of n = min(colours, 8),
 *             n - step, ... >= 2 colours, the first n of top_colors
 *   k-means   then n = min(colours, 8) down to 2: centroids lb + (2i + 1)(ub - lb) / n / 2 through svt_av1_k_means_dim1_c (Codec/k_means_template.h):
 *             calc_indices with strict <, calc_centroids with DIVIDE_AND_ROUND and an empty cluster taking data[lcg_rand16(&state) % (rows * cols)]
 *             (state seeded from data[0] at every call), the stop on unchanged centroids, the 50 iterations, the restore when the distance rises;
 *             colours == 2: the centroids are lb and ub
 *   candidate palette_rd_y (:272-296): optimize_palette_colors (a centroid within 1 of a cache colour becomes it, first minimum), sort,
 *             av1_remove_duplicates, clip, indices over rows x cols against the sorted unique centroids, extend_palette_color_map to width x height;
 *             kept when more than 2 colours are left, in the reference's order
 *   rate      palette_ymode_fac_bits[bsize_ctx][mode_ctx][1] + palette_ysize_fac_bits[bsize_ctx][size - 2] + svt_aom_write_uniform_cost(size,
 *             color_map[0]) + svt_av1_palette_color_cost_y (:78-143, with cost_bit_depth) + svt_av1_cost_color_map (:487-547, the contexts of
 *             svt_aom_get_palette_color_index_context_optimized, Codec/cabac_context_model.c:2453-2560) unless reduce_palette_cost_precision
 * One prediction job = the palette branch of svt_av1_predict_intra_block{,_16bit} (Codec/enc_intra_prediction.c:501-510, :647-656) for one kept
 * candidate over the whole block: palette[map[r][c]], the map recomputed from the source plane as palette_rd_y computes it.
 * All outputs are integers and bit-exact with the reference's C path, 8-bit planes (uint8) and 10-bit planes (packed uint16), the 16 block sizes of
 * svt_av1_allow_palette: 8x8 ... 64x64 without a side of 128, with 4x16 and 16x4.
 *
 * These keep the host path: chroma palette (the reference has none: palette_size[1] = 0), dim-2 k-means, 12-bit, the derivation of the colour cache
 * (svt_get_palette_cache_y), svt_aom_get_palette_bsize_ctx / svt_aom_get_palette_mode_ctx, the tokenizer side of cost_and_tokenize_map, the candidate
 * bookkeeping of inject_palette_candidates.
 *
 * A cache colour may lie above the planes' maximum: in a 10-bit encode searched at 8 bits (hbd_md == 0) the neighbours' palettes come back
 * multiplied by 4.  Such a colour only counts in n_cache, but for maximum + 1, which attracts a centroid at the maximum as any colour one step away
 * does: the candidate's colour is then the clipped maximum while its indices are computed against maximum + 1, as palette_rd_y does; the record
 * says so in top_over, which the prediction batch reads.
 *
 * A search job gets status 0xFF, and writes nothing else, when its size is not one of the 16; rows / cols are 0 or above height / width; n_cache > 16;
 * bsize_ctx >= 7; mode_ctx >= 3; src_offset plus the rows x cols samples it reads leaves the source plane; or, with color_maps, map_offset +
 * SVT_HIP_PALETTE_MAX_CANDS * width * height > map_bytes.  A prediction job gets 0xFF, and writes nothing else, when search_index >= n_search_jobs, that search job's status is not 0, cand_index >= its n_cands, its
 * rows x cols samples leave the source plane, dst_offset plus the block leaves the destination, or, with color_map, map_offset + width * height > map_bytes.
 * Every other job writes status 0.
 */
#ifndef SVT_HIP_PALETTE_H
#define SVT_HIP_PALETTE_H

#include <stdint.h>
#include <stddef.h>
#include "svt_hip_me.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVT_HIP_PALETTE_MAX_CANDS 14   /* the reference's array; at most 12 are ever kept */
#define SVT_HIP_PALETTE_MAX_SIZE 8     /* PALETTE_MAX_SIZE */
#define SVT_HIP_PALETTE_MAX_CACHE 16   /* 2 * PALETTE_MAX_SIZE */
#define SVT_HIP_PALETTE_BSIZE_CTXS 7   /* PALATTE_BSIZE_CTXS */
#define SVT_HIP_PALETTE_MODE_CTXS 3    /* PALETTE_Y_MODE_CONTEXTS */
#define SVT_HIP_PALETTE_OK 0
#define SVT_HIP_PALETTE_UNDEFINED 0xFF

typedef struct SvtHipPaletteJob {
    uint32_t src_offset;      /* of the block's first sample in the source plane, in samples */
    uint32_t map_offset;      /* of the job's first colour map in color_maps, in bytes; candidate c's map is at map_offset + c * width * height */
    uint8_t  width, height;   /* of the block */
    uint8_t  rows, cols;      /* svt_aom_get_block_dimensions' rows_within_bounds / cols_within_bounds */
    uint8_t  n_cache;         /* svt_get_palette_cache_y's return (neighbour logic: the host's) */
    uint8_t  bsize_ctx;       /* svt_aom_get_palette_bsize_ctx */
    uint8_t  mode_ctx;        /* svt_aom_get_palette_mode_ctx */
    uint8_t  reserved;
    uint16_t color_cache[SVT_HIP_PALETTE_MAX_CACHE]; /* the first n_cache are read */
} SvtHipPaletteJob;

typedef struct SvtHipPaletteCand {
    uint8_t  size;            /* 3..8: palette_size[0] */
    uint8_t  first_index;     /* color_map[0] */
    uint16_t colors[SVT_HIP_PALETTE_MAX_SIZE]; /* pmi.palette_colors: sorted, unique, clipped; the first `size` are meaningful, the rest 0 */
    uint8_t  top_over;        /* 1: the last centroid was the planes' maximum + 1 before its clip (a cache colour there attracted it), and the map's
                                 indices are computed against colors[size - 1] + 1; else 0 */
    uint8_t  reserved;
    int32_t  color_cost;      /* svt_av1_palette_color_cost_y */
    int32_t  map_cost;        /* svt_av1_cost_color_map; 0 under reduce_palette_cost_precision */
    int32_t  index0_cost;     /* svt_aom_write_uniform_cost(size, first_index) */
    int32_t  size_cost;       /* palette_ysize_fac_bits[bsize_ctx][size - 2] */
    int32_t  rate;            /* palette_ymode_fac_bits[bsize_ctx][mode_ctx][1] + the four above: what rd_cost.c:684-704 adds to intra_luma_mode_bits_num */
} SvtHipPaletteCand;

typedef struct SvtHipPaletteResult {
    uint32_t n_colors;        /* what svt_av1_count_colors{,_highbd} returns */
    uint32_t n_cands;         /* tot_palette_cands; the records past it are not written */
    SvtHipPaletteCand cands[SVT_HIP_PALETTE_MAX_CANDS];
} SvtHipPaletteResult;

typedef struct SvtHipPaletteDesc {
    uint8_t  bit_depth;       /* 8: the plane is uint8; 10: uint16.  bit_depth_pal: the clip and the bound of the top_colors scan */
    uint8_t  cost_bit_depth;  /* 8 or 10: encoder_bit_depth, which svt_av1_palette_color_cost_y gets, and svt_av1_count_colors_highbd as its bound:
                                 10-bit planes go with cost_bit_depth 10 only, so that bound is 1 << bit_depth; 8-bit planes take either */
    uint8_t  dominant_color_step;           /* 1 or 2: palette_ctrls.dominant_color_step */
    uint8_t  reduce_palette_cost_precision; /* palette_ctrls.reduce_palette_cost_precision */
    uint32_t n_jobs;
    const void *src;          /* device pointer: the source luma plane (enhanced_pic, or input_frame16bit at 10 bits) */
    uint32_t src_stride;      /* in samples */
    uint32_t reserved;
    uint64_t src_samples;     /* samples the source holds from `src` on */
    const int32_t *palette_ycolor_fac_bitss; /* device pointer, [7][5][8]: md_rate_est_ctx's, indexed [size - 2][ctx][index] */
    const int32_t *palette_ysize_fac_bits;   /* device pointer, [7][8] */
    const int32_t *palette_ymode_fac_bits;   /* device pointer, [7][3][3] */
    const SvtHipPaletteJob *jobs;            /* device pointer, n_jobs entries */
    SvtHipPaletteResult *results;            /* device pointer, [n_jobs] */
    uint8_t *status;          /* device pointer, [n_jobs] */
    uint8_t *color_maps;      /* optional device pointer: every kept candidate's width x height colour map, see map_offset */
    uint64_t map_bytes;       /* bytes color_maps holds */
} SvtHipPaletteDesc;

typedef struct SvtHipPalettePredJob {
    uint32_t search_index;    /* which search job: its block, its result */
    uint32_t cand_index;      /* which of that result's candidates */
    uint32_t dst_offset;      /* of the block's first sample in the prediction plane, in samples */
    uint32_t map_offset;      /* of the width x height colour map in color_map, in bytes */
} SvtHipPalettePredJob;

typedef struct SvtHipPalettePredDesc {
    uint8_t  bit_depth;       /* 8 or 10: both planes */
    uint8_t  reserved[3];
    uint32_t n_jobs;
    uint32_t n_search_jobs;
    uint32_t src_stride;      /* in samples */
    const void *src;          /* device pointer: the source plane the search ran on */
    uint64_t src_samples;
    void    *dst;             /* device pointer: the prediction plane */
    uint32_t dst_stride;      /* in samples */
    uint32_t reserved2;
    uint64_t dst_samples;
    const SvtHipPaletteJob    *search_jobs;    /* device pointer, [n_search_jobs]: svt_hip_palette_search_batch's jobs */
    const SvtHipPaletteResult *search_results; /* device pointer, [n_search_jobs]: its results, read on the device */
    const uint8_t             *search_status;  /* device pointer, [n_search_jobs]: its status */
    const SvtHipPalettePredJob *jobs;          /* device pointer, n_jobs entries */
    uint8_t *status;          /* device pointer, [n_jobs] */
    uint8_t *color_map;       /* optional device pointer: the colour maps the entropy coder needs, byte for byte the search's */
    uint64_t map_bytes;
} SvtHipPalettePredDesc;

/* Enqueues one batch on the context stream (asynchronous); one wave per job.  Returns SVT_HIP_ERR_BAD_PARAM (and svt_hip_last_error) and enqueues
 * nothing when svt_hip_palette_check_desc refuses the descriptor; n_jobs == 0 returns 0 and enqueues nothing. */
int    svt_hip_palette_search_batch(SvtHipContext *ctx, const SvtHipPaletteDesc *d);
/* Host-only validation: null descriptor or src / jobs / results / status / one of the three tables, bit_depth or cost_bit_depth other than 8 / 10,
 * bit_depth 10 with cost_bit_depth 8, dominant_color_step other than 1 / 2, a zero src_stride or src_samples, color_maps with map_bytes 0. */
int    svt_hip_palette_check_desc(const SvtHipPaletteDesc *d);
/* Enqueues the predictions on the context stream (asynchronous); one wave per job, ordinary vector stores.  Refused (SVT_HIP_ERR_BAD_PARAM): a null
 * descriptor or src / dst / search_jobs / search_results / search_status / jobs / status, bit_depth other than 8 / 10, a zero stride or sample
 * count, n_search_jobs 0, color_map with map_bytes 0 (svt_hip_palette_pred_check_desc). */
int    svt_hip_palette_pred_batch(SvtHipContext *ctx, const SvtHipPalettePredDesc *d);
int    svt_hip_palette_pred_check_desc(const SvtHipPalettePredDesc *d);
/* sizeof / offsetof as compiled: what = 0 the search descriptor, 1 the search job, 2 the candidate, 3 the result, 4 the prediction job, 5 the
 * prediction descriptor; `field` < 0 the size, else the offset of the field-th member in declaration order ((size_t)-1 past the last) */
size_t svt_hip_palette_layout(int what, int field);

#ifdef __cplusplus
}
#endif
#endif
