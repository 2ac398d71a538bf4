/*
 * svt_hip_tpl.h -- C-ABI of the MI355X TPL dispenser (temporal dependency model, levels 4 and 5).
 *
 * One call = tpl_mc_flow_dispenser_sb_generic (Source/Lib/Codec/src_ops_process.c:519-1200) for every b64 of one picture, in the
 * reference's order, followed by the padding of the TPL recon picture (svt_aom_generate_padding, :1400-1406):
 *   a) source pass (every block at least half inside the picture, in parallel): DC intra prediction from the source and its SAD,
 *      the ME candidates' full-pel SADs against the source-path references after the +-TPL_PADX / TPL_PADY clamp, the arg-min,
 *      and for a NEWMV winner the forward transform + get_quantize_error of the source-path residual (:608-977);
 *   b) inter recon (every NEWMV block, in parallel): the prediction copied from the recon-path reference, the transform chain,
 *      the inverse transform into the TPL recon picture (:980-1040,1131-1198);
 *   c) intra recon: DC prediction from the CURRENT recon picture's neighbours, so the intra blocks are walked by ONE workgroup over
 *      the anti-diagonals of the block grid (a block's above and left neighbours are reconstructed first, as in the reference's
 *      raster-of-b64 / z-order walk);
 *   d) padding of the recon plane and the synthesizer grid writes of result_model_store (:266-340).
 * Levels 1-3 (SATD source search, the other intra modes, sub-pel search, compute_rate) are refused: the host keeps its own loop.
 */
#ifndef SVT_HIP_TPL_H
#define SVT_HIP_TPL_H

#include <stdint.h>
#include <stddef.h>
#include "svt_hip_me.h"
#include "svt_hip_dsp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVT_HIP_TPL_PAD 32 /* TPL_PADX / TPL_PADY, Codec/definitions.h */

/* TplStats (Codec/coding_unit.h:312-321); mc_dep_rate / mc_dep_dist are written as 0.  mv = {row, col} in 1/8 sample. */
typedef struct SvtHipTplStats {
    int64_t  srcrf_dist, recrf_dist, srcrf_rate, recrf_rate, mc_dep_rate, mc_dep_dist;
    int16_t  mv_row, mv_col;
    uint32_t reserved;
    uint64_t ref_frame_poc;
} SvtHipTplStats;

/* TplSrcStats (Codec/coding_unit.h:323-331); PredictionMode is ATTRIBUTE_PACKED (Codec/definitions.h:1126-1165): one byte. */
typedef struct SvtHipTplSrcStats {
    int64_t  srcrf_dist, srcrf_rate;
    uint64_t ref_frame_poc;
    int16_t  mv_row, mv_col;
    uint8_t  best_mode; /* DC_PRED 0 or NEWMV 16 */
    uint8_t  reserved[3];
    int32_t  best_rf_idx; /* -1: none; 0..3 list 0, 4..7 list 1 */
    uint8_t  best_intra_mode;
    uint8_t  reserved2[3];
} SvtHipTplSrcStats;

/* One reference of the picture, per (list, ref_idx) as pcs->tpl_data holds it. */
typedef struct SvtHipTplRef {
    SvtHipPlaneDesc src;   /* tpl_ref_ds_ptr_array[list][ref].picture_ptr: the padded input (source-path search)            */
    SvtHipPlaneDesc recon; /* mc_flow_rec_picture_buffer[poc_map_idx] when ref_in_slide_window, else the same plane as src  */
    uint64_t picture_number;        /* tpl_ref_ds_ptr_array[..].picture_number (stored as ref_frame_poc) */
    uint16_t max_width, max_height; /* the source plane's max_width / max_height, read by the MV clamp (:790-803) */
    uint8_t  usable;                /* 0: candidates on it are skipped (ref_tpl_group_idx > 0 && !tpl_valid_pic, :779-782); stored stats
                                     * (src_pass 0) may still name it for the recon path */
    uint8_t  reserved[3];
} SvtHipTplRef;

typedef struct SvtHipTplDesc {
    /* current picture: pcs->enhanced_pic (8-bit, padded; width / height = the input size) and pcs->aligned_width / height */
    SvtHipPlaneDesc cur;
    uint16_t        aligned_width, aligned_height;
    /* the TPL recon picture mc_flow_rec_picture_buffer[frame_idx]: WRITTEN through recon.buffer_y (blocks, then the padding);
     * org_x / org_y >= SVT_HIP_TPL_PAD, width / height >= cur's */
    SvtHipPlaneDesc recon;
    /* ME results of the picture in the layout svt_hip_me_picture* writes (device pointers; total_me_candidate_index,
     * me_mv_array and me_candidate_array are read).  May be NULL when slice_is_i (no candidate is read). */
    SvtHipMeResults me;
    uint8_t         n_pu, max_cand, max_refs, max_l0, enable_me_16x16;
    uint8_t         reserved0[3];
    /* only the entries candidates or stored stats name are read.  A stored NEWMV decision (src_pass 0) naming a reference without
     * planes is not something the reference produces: that block is skipped (recon and grid cells untouched). */
    SvtHipTplRef    refs[SVT_HIP_MAX_LISTS][SVT_HIP_MAX_REFS];
    /* controls (pcs->tpl_ctrls and friends) */
    uint8_t dispenser_search_level; /* 0: 16x16 blocks, 1: 32x32 blocks */
    uint8_t subsample_tx;           /* 0, 1, 2: rows of the transform taken every 1 / 2 / 4 rows */
    uint8_t pf_shape;               /* EB_TRANS_COEFF_SHAPE 0..3 of the forward transform; 3 (ONLY_DC) keeps every coefficient, as
                                     * svt_av1_wht_fwd_txfm does (it has cases for N2 and N4 alone) */
    uint8_t synth_blk_size;         /* 16 or 32: the TplStats grid */
    uint8_t disable_intra_pred;     /* disable_intra_pred_nref && temporal_layer_index == hierarchical_levels */
    uint8_t is_ref;                 /* tpl_data.is_ref */
    uint8_t slice_is_i;             /* pcs->slice_type == I_SLICE: no candidate is read (:767-769) */
    uint8_t tpl_slice_is_i;         /* tpl_data.tpl_slice_type == I_SLICE: mv / poc not stored (:1192) */
    uint8_t src_pass;               /* tpl_src_data_ready == 0: run the source pass; else read tpl_src_stats */
    uint8_t store_src_stats;        /* scs->tpl_lad_mg > 0: the source pass writes tpl_src_stats */
    /* level-1 behaviour, carried so that the refusal is explicit: only 1 / DC_PRED (0) / FULL_PEL (3, SUBPEL_FORCE_STOP of
     * Codec/definitions.h: EIGHTH_PEL 0, QUARTER_PEL 1, HALF_PEL 2) / 0 are accepted */
    uint8_t use_sad_in_src_search, intra_mode_end, subpel_depth, compute_rate;
    uint8_t in_loop_ois;            /* scs->in_loop_ois: must be 1 (the OIS results are not an input) */
    uint8_t reserved1[3];
    SvtHipQuantRow quant;           /* the 8-bit tables' row of qIndex (quants_8bit / deq_8bit, :551-557) */
    /* outputs (device pointers) */
    SvtHipTplStats    *tpl_stats;   /* synthesizer grid, stride (aligned_width + synth - 1) / synth; cells of skipped blocks untouched */
    uint32_t           n_tpl_stats; /* cells the buffer holds: >= stride * ((aligned_height + synth - 1) / synth); writes past it are dropped */
    uint32_t           n_tpl_src_stats;
    SvtHipTplSrcStats *tpl_src_stats; /* aligned-16 grid, stride (aligned_width + 15) / 16; read when src_pass == 0, written when
                                       * src_pass && store_src_stats; may be NULL otherwise */
} SvtHipTplDesc;

/* Enqueues the dispenser of one picture on the context stream (asynchronous; every pointer a DEVICE pointer).  Returns non-zero and
 * enqueues nothing when svt_hip_tpl_check_desc refuses the descriptor (SVT_HIP_ERR_BAD_PARAM). */
int    svt_hip_tpl_dispense(SvtHipContext *ctx, const SvtHipTplDesc *d);
/* Host-only validation: SVT_HIP_ERR_BAD_PARAM (and svt_hip_last_error) for level-1 behaviour (use_sad_in_src_search 0, intra_mode_end
 * other than DC_PRED, subpel_depth other than FULL_PEL, compute_rate), dispenser_search_level 2, a synth_blk_size other than 16 / 32,
 * in_loop_ois 0, recon / reference padding below SVT_HIP_TPL_PAD, missing pointers or short output buffers. */
int    svt_hip_tpl_check_desc(const SvtHipTplDesc *d);
size_t svt_hip_tpl_desc_size(void); /* sizeof(SvtHipTplDesc) as compiled */

/* ---- The TPL group: tpl_mc_flow (Source/Lib/Codec/src_ops_process.c:1783-1956) and svt_aom_generate_r0beta (:1585-1677) ----
 *
 * One call runs up to three stages over the window of a TPL group (frames in decode order, frames_in_sw <= 512), all on the context
 * stream, asynchronously:
 *   1. DISPENSE: tpl_mc_flow's frame loop.  For f = 0 .. n-1: the grid's first ceil(width / s) * ceil(height / s) cells are zeroed
 *      (:1841-1845, s = synth_blk_size), then, when tpl_valid_pic, the dispenser runs on frame f's SvtHipTplDesc.
 *   2. SYNTHESIZE: for f = n-1 .. 0 with tpl_valid_pic, tpl_mc_flow_synthesizer (:1571-1584, tpl_model_update{,_b} :1480-1565):
 *      mc_dep_dist / mc_dep_rate of every cell of frame f propagated into the cells of the frame its ref_frame_poc names (the FIRST
 *      frame of the window with that picture_number; none: nothing).  One launch per frame; the adds are 64-bit integer atomics, so
 *      the grids are bit-exact whatever the order of arrival.
 *   3. R0BETA: svt_aom_generate_r0beta + generate_lambda_scaling_factor (:176-223) for every frame that supplies outputs: r0 and
 *      tpl_is_valid, one tpl_beta per superblock, one tpl_rdmult_scaling_factors entry per synth cell.  Running stage 3 alone on one
 *      frame is how rate control asks for r0 / beta later (rc_process.c:3316-3319), e.g. after another group rewrote the grid.
 *
 * Reproduced as the reference has it:
 *   - the synthesizer, generate_r0beta and generate_lambda_scaling_factor index the grid at row stride (mi_cols_sr >> shift), i.e.
 *     floor(ceil(w / 16) / 2) with synth 32, while the dispenser writes at ceil(aligned_width / 32): when ceil(w / 16) is odd the last
 *     column of a row reads the next row's first cell (e.g. 720x1280);
 *   - the synthesizer bounds the quadrants by the reference picture's aligned size; generate_r0beta's picture sum runs over the aligned
 *     rows and the unscaled columns (rounded up to 16), its per-superblock sums cut at the unscaled height rounded up to 16;
 *   - GET_MV_RAWPEL rounding of the MV, round_floor, RDCOST, int64 wrap-around and C's truncating division;
 *   - r0 is written only when mc_dep_cost_base != 0; otherwise it keeps its value, which beta then reads.
 * Defined where the reference is not:
 *   - a cell with recrf_dist == 0 propagates nothing.  The dispenser leaves such cells (blocks less than half inside, :578-580) at
 *     zero with ref_frame_poc 0, so with picture 0 in the window the reference divides by zero there (SIGFPE on x86);
 *   - a cell whose ref_frame_poc resolves to its own frame propagates nothing.  Every such cell the dispenser writes is intra
 *     (recrf == srcrf, equal rates) and propagates zero in the reference, so this only removes a read / write race.
 */
#define SVT_HIP_TPL_MAX_GROUP 512 /* MAX_TPL_GROUP_SIZE */
#define SVT_HIP_TPL_STAGE_DISPENSE   1u
#define SVT_HIP_TPL_STAGE_SYNTHESIZE 2u
#define SVT_HIP_TPL_STAGE_R0BETA     4u

/* One frame of the window, in decode order.  Every buffer pointer is a DEVICE pointer; `dispense` is a host pointer. */
typedef struct SvtHipTplGroupFrame {
    uint64_t        picture_number;
    uint8_t         tpl_valid_pic;  /* pcs->tpl_valid_pic[frame_idx] */
    uint8_t         reserved[3];
    int32_t         base_rdmult;    /* pa_me_data->base_rdmult (the host computes it from qIndex as :1372 does); read by stage 3 */
    SvtHipTplStats *tpl_stats;      /* the frame's grid (pa_me_data->tpl_stats) */
    uint32_t        n_tpl_stats;    /* cells it holds: >= ceil(width / s) * ceil(height / s) */
    uint32_t        n_beta;         /* entries of beta: >= ceil(aligned_width / sb_size) * ceil(aligned_height / sb_size) */
    /* stage 1: the dispenser of this frame, read when tpl_valid_pic (may be NULL otherwise); its tpl_stats must be this frame's grid,
     * its aligned size and synth_blk_size the group's, its cur plane width x height */
    const SvtHipTplDesc *dispense;
    /* stage 3 outputs; all four NULL: the frame supplies none.  r0 is read as well (see above). */
    double         *r0;
    uint8_t        *tpl_is_valid;
    double         *beta;           /* pa_me_data->tpl_beta, raster order of the superblocks */
    double         *scaling;        /* pa_me_data->tpl_rdmult_scaling_factors */
    uint32_t        n_scaling;      /* entries: >= ceil(mi_cols_sr / n) * ceil(mi_rows / n), n = s / 4, mi_cols_sr = ceil(width / 16) * 4 */
    uint32_t        reserved2;
} SvtHipTplGroupFrame;

typedef struct SvtHipTplGroupDesc {
    uint16_t width, height;                 /* enhanced_unscaled_pic (== enhanced_pic without super-res) */
    uint16_t aligned_width, aligned_height; /* pcs->aligned_width / height: mi_cols / mi_rows = >> 2 */
    uint8_t  synth_blk_size;                /* 16 or 32 */
    uint8_t  sb_size;                       /* scs->sb_size: 64 or 128 */
    uint8_t  compute_rate;                  /* must be 0: delta_rate_cost's log / pow are not reproduced bit for bit on the device */
    uint8_t  superres_denom;                /* must be 8 (SCALE_NUMERATOR: no super-res / resize) */
    uint32_t stages;                        /* SVT_HIP_TPL_STAGE_* */
    uint32_t n_frames;                      /* 1 .. SVT_HIP_TPL_MAX_GROUP */
    const SvtHipTplGroupFrame *frames;      /* host array of n_frames */
} SvtHipTplGroupDesc;

/* Enqueues the selected stages on the context stream (asynchronous).  Returns non-zero and enqueues nothing -- no grid or output is
 * written -- when svt_hip_tpl_group_check_desc refuses the descriptor (SVT_HIP_ERR_BAD_PARAM). */
int    svt_hip_tpl_group(SvtHipContext *ctx, const SvtHipTplGroupDesc *d);
/* Host-only validation of the whole descriptor, every frame and every embedded SvtHipTplDesc (svt_hip_tpl_check_desc) included:
 * SVT_HIP_ERR_BAD_PARAM for compute_rate, a synth_blk_size other than 16 / 32, superres_denom other than 8, sb_size other than
 * 64 / 128, n_frames 0 or above 512, no or unknown stages, aligned sizes below the picture size, null pointers, grids shorter than
 * the reference's allocation or than any cell a stage reads, two frames sharing grid cells (stage 2), beta / scaling shorter than
 * stage 3 writes, a dispenser descriptor that does not match the frame. */
int    svt_hip_tpl_group_check_desc(const SvtHipTplGroupDesc *d);
size_t svt_hip_tpl_group_desc_size(void);  /* sizeof(SvtHipTplGroupDesc) as compiled */
size_t svt_hip_tpl_group_frame_size(void); /* sizeof(SvtHipTplGroupFrame) as compiled */

#ifdef __cplusplus
}
#endif
#endif /* SVT_HIP_TPL_H */
