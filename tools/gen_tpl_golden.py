#!/usr/bin/env python3
"""Writes tests/golden/tpl_dispenser.npz and tests/golden/tpl_dispenser_edges.npz: the reference encoder's own TPL dispenser on the seeded
cases (FIXTURE_CASES) and on the edge cases (edge_cases, groups A-F and H) of tests/tpl_dispenser_cases.py.

Run by hand on a machine that has the reference's sources (--ref: the root of its source tree); never by the tests, build(), smoke() or
bench.py.  It compiles, where they lie, the reference's Codec/src_ops_process.c -- #included by a small harness of its own, because
tpl_mc_flow_dispenser_sb_generic is static -- and the sources that file needs for levels 4 / 5, into a temporary directory outside the tree
(gcc -O2 -DNDEBUG; the few functions only the level-1 paths call -- sub-pel search, rate, rdmult -- are stubs that abort), links with
--gc-sections and a version script that exports the harness alone.  The harness fills PictureParentControlSet, SequenceControlSet and
EncodeContext with the fields the dispenser reads (from an SvtHipTplDesc of host pointers), installs the `_c` kernels in the rtcd pointers
it reaches, calls the dispenser for every b64 in raster order and then svt_aom_generate_padding of the recon picture.

The fixture holds numbers only: per case its generator arguments (the inputs are the deterministic planes, candidate lists and MVs of
tpl_dispenser_cases.make_case, pinned by a checksum of every input array) and the outputs -- the TplStats grid, the TplSrcStats and the whole
padded recon plane.  The sliding-window case dispenses two pictures: the second's list-0 recon-path reference is the first's TPL recon.
The edge-case file has the same layout, except that the recon plane of the groups with many or large pictures is stored as its sha256.
--check recomputes everything and compares it with the two committed files instead of writing them."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import tpl_dispenser_cases as tc  # noqa: E402
from svt_av1_psyex_amd import tpl  # noqa: E402
import refbuild  # noqa: E402

HARNESS = r"""
/* Calls the reference's own tpl_mc_flow_dispenser_sb_generic (static: included) for every b64 in raster order, then
 * svt_aom_generate_padding, on host planes described by an SvtHipTplDesc. */
#include "src_ops_process.c"
#include "svt_hip_tpl.h"
uint32_t svt_nxm_sad_kernel_helper_c(const uint8_t *src, uint32_t src_stride, const uint8_t *ref, uint32_t ref_stride, uint32_t height, uint32_t width);

static EbPictureBufferDesc to_desc(const SvtHipPlaneDesc *p, uint16_t max_w, uint16_t max_h) {
    EbPictureBufferDesc d;
    memset(&d, 0, sizeof(d));
    d.buffer_y = (uint8_t *)p->buffer_y; d.stride_y = p->stride_y; d.org_x = p->org_x; d.org_y = p->org_y;
    d.width = p->width; d.height = p->height; d.max_width = max_w; d.max_height = max_h; d.bit_depth = EB_EIGHT_BIT;
    return d;
}

void harness_init(void) {
    svt_aom_dc_predictor_4x4 = svt_aom_dc_predictor_4x4_c;
    svt_aom_dc_predictor_8x8 = svt_aom_dc_predictor_8x8_c;
    svt_aom_dc_predictor_16x16 = svt_aom_dc_predictor_16x16_c;
    svt_aom_dc_predictor_32x32 = svt_aom_dc_predictor_32x32_c;
    svt_aom_dc_predictor_64x64 = svt_aom_dc_predictor_64x64_c;
    svt_aom_dc_predictor_16x32 = svt_aom_dc_predictor_16x32_c;
    svt_aom_dc_predictor_16x4 = svt_aom_dc_predictor_16x4_c;
    svt_aom_dc_predictor_16x64 = svt_aom_dc_predictor_16x64_c;
    svt_aom_dc_predictor_16x8 = svt_aom_dc_predictor_16x8_c;
    svt_aom_dc_predictor_32x16 = svt_aom_dc_predictor_32x16_c;
    svt_aom_dc_predictor_32x64 = svt_aom_dc_predictor_32x64_c;
    svt_aom_dc_predictor_32x8 = svt_aom_dc_predictor_32x8_c;
    svt_aom_dc_predictor_4x16 = svt_aom_dc_predictor_4x16_c;
    svt_aom_dc_predictor_4x8 = svt_aom_dc_predictor_4x8_c;
    svt_aom_dc_predictor_64x16 = svt_aom_dc_predictor_64x16_c;
    svt_aom_dc_predictor_64x32 = svt_aom_dc_predictor_64x32_c;
    svt_aom_dc_predictor_8x16 = svt_aom_dc_predictor_8x16_c;
    svt_aom_dc_predictor_8x32 = svt_aom_dc_predictor_8x32_c;
    svt_aom_dc_predictor_8x4 = svt_aom_dc_predictor_8x4_c;
    svt_aom_dc_left_predictor_4x4 = svt_aom_dc_left_predictor_4x4_c;
    svt_aom_dc_left_predictor_8x8 = svt_aom_dc_left_predictor_8x8_c;
    svt_aom_dc_left_predictor_16x16 = svt_aom_dc_left_predictor_16x16_c;
    svt_aom_dc_left_predictor_32x32 = svt_aom_dc_left_predictor_32x32_c;
    svt_aom_dc_left_predictor_64x64 = svt_aom_dc_left_predictor_64x64_c;
    svt_aom_dc_left_predictor_16x32 = svt_aom_dc_left_predictor_16x32_c;
    svt_aom_dc_left_predictor_16x4 = svt_aom_dc_left_predictor_16x4_c;
    svt_aom_dc_left_predictor_16x64 = svt_aom_dc_left_predictor_16x64_c;
    svt_aom_dc_left_predictor_16x8 = svt_aom_dc_left_predictor_16x8_c;
    svt_aom_dc_left_predictor_32x16 = svt_aom_dc_left_predictor_32x16_c;
    svt_aom_dc_left_predictor_32x64 = svt_aom_dc_left_predictor_32x64_c;
    svt_aom_dc_left_predictor_32x8 = svt_aom_dc_left_predictor_32x8_c;
    svt_aom_dc_left_predictor_4x16 = svt_aom_dc_left_predictor_4x16_c;
    svt_aom_dc_left_predictor_4x8 = svt_aom_dc_left_predictor_4x8_c;
    svt_aom_dc_left_predictor_64x16 = svt_aom_dc_left_predictor_64x16_c;
    svt_aom_dc_left_predictor_64x32 = svt_aom_dc_left_predictor_64x32_c;
    svt_aom_dc_left_predictor_8x16 = svt_aom_dc_left_predictor_8x16_c;
    svt_aom_dc_left_predictor_8x32 = svt_aom_dc_left_predictor_8x32_c;
    svt_aom_dc_left_predictor_8x4 = svt_aom_dc_left_predictor_8x4_c;
    svt_aom_dc_top_predictor_4x4 = svt_aom_dc_top_predictor_4x4_c;
    svt_aom_dc_top_predictor_8x8 = svt_aom_dc_top_predictor_8x8_c;
    svt_aom_dc_top_predictor_16x16 = svt_aom_dc_top_predictor_16x16_c;
    svt_aom_dc_top_predictor_32x32 = svt_aom_dc_top_predictor_32x32_c;
    svt_aom_dc_top_predictor_64x64 = svt_aom_dc_top_predictor_64x64_c;
    svt_aom_dc_top_predictor_16x32 = svt_aom_dc_top_predictor_16x32_c;
    svt_aom_dc_top_predictor_16x4 = svt_aom_dc_top_predictor_16x4_c;
    svt_aom_dc_top_predictor_16x64 = svt_aom_dc_top_predictor_16x64_c;
    svt_aom_dc_top_predictor_16x8 = svt_aom_dc_top_predictor_16x8_c;
    svt_aom_dc_top_predictor_32x16 = svt_aom_dc_top_predictor_32x16_c;
    svt_aom_dc_top_predictor_32x64 = svt_aom_dc_top_predictor_32x64_c;
    svt_aom_dc_top_predictor_32x8 = svt_aom_dc_top_predictor_32x8_c;
    svt_aom_dc_top_predictor_4x16 = svt_aom_dc_top_predictor_4x16_c;
    svt_aom_dc_top_predictor_4x8 = svt_aom_dc_top_predictor_4x8_c;
    svt_aom_dc_top_predictor_64x16 = svt_aom_dc_top_predictor_64x16_c;
    svt_aom_dc_top_predictor_64x32 = svt_aom_dc_top_predictor_64x32_c;
    svt_aom_dc_top_predictor_8x16 = svt_aom_dc_top_predictor_8x16_c;
    svt_aom_dc_top_predictor_8x32 = svt_aom_dc_top_predictor_8x32_c;
    svt_aom_dc_top_predictor_8x4 = svt_aom_dc_top_predictor_8x4_c;
    svt_aom_dc_128_predictor_4x4 = svt_aom_dc_128_predictor_4x4_c;
    svt_aom_dc_128_predictor_8x8 = svt_aom_dc_128_predictor_8x8_c;
    svt_aom_dc_128_predictor_16x16 = svt_aom_dc_128_predictor_16x16_c;
    svt_aom_dc_128_predictor_32x32 = svt_aom_dc_128_predictor_32x32_c;
    svt_aom_dc_128_predictor_64x64 = svt_aom_dc_128_predictor_64x64_c;
    svt_aom_dc_128_predictor_16x32 = svt_aom_dc_128_predictor_16x32_c;
    svt_aom_dc_128_predictor_16x4 = svt_aom_dc_128_predictor_16x4_c;
    svt_aom_dc_128_predictor_16x64 = svt_aom_dc_128_predictor_16x64_c;
    svt_aom_dc_128_predictor_16x8 = svt_aom_dc_128_predictor_16x8_c;
    svt_aom_dc_128_predictor_32x16 = svt_aom_dc_128_predictor_32x16_c;
    svt_aom_dc_128_predictor_32x64 = svt_aom_dc_128_predictor_32x64_c;
    svt_aom_dc_128_predictor_32x8 = svt_aom_dc_128_predictor_32x8_c;
    svt_aom_dc_128_predictor_4x16 = svt_aom_dc_128_predictor_4x16_c;
    svt_aom_dc_128_predictor_4x8 = svt_aom_dc_128_predictor_4x8_c;
    svt_aom_dc_128_predictor_64x16 = svt_aom_dc_128_predictor_64x16_c;
    svt_aom_dc_128_predictor_64x32 = svt_aom_dc_128_predictor_64x32_c;
    svt_aom_dc_128_predictor_8x16 = svt_aom_dc_128_predictor_8x16_c;
    svt_aom_dc_128_predictor_8x32 = svt_aom_dc_128_predictor_8x32_c;
    svt_aom_dc_128_predictor_8x4 = svt_aom_dc_128_predictor_8x4_c;
    svt_aom_init_intra_predictors_internal();
    svt_nxm_sad_kernel     = svt_nxm_sad_kernel_helper_c;
    svt_aom_subtract_block = svt_aom_subtract_block_c;
    svt_av1_quantize_fp    = svt_av1_quantize_fp_c;
    svt_av1_block_error    = svt_av1_block_error_c;
    svt_av1_inv_txfm_add   = svt_av1_inv_txfm_add_c;
    svt_memcpy = svt_memcpy_c;
    svt_av1_inv_txfm2d_add_4x4 = svt_av1_inv_txfm2d_add_4x4_c;
    svt_av1_inv_txfm2d_add_8x8 = svt_av1_inv_txfm2d_add_8x8_c;
    svt_av1_inv_txfm2d_add_16x16 = svt_av1_inv_txfm2d_add_16x16_c;
    svt_av1_inv_txfm2d_add_32x32 = svt_av1_inv_txfm2d_add_32x32_c;
    svt_av1_inv_txfm2d_add_64x64 = svt_av1_inv_txfm2d_add_64x64_c;
    svt_av1_inv_txfm2d_add_8x16 = svt_av1_inv_txfm2d_add_8x16_c;
    svt_av1_inv_txfm2d_add_16x8 = svt_av1_inv_txfm2d_add_16x8_c;
    svt_av1_inv_txfm2d_add_16x32 = svt_av1_inv_txfm2d_add_16x32_c;
    svt_av1_inv_txfm2d_add_32x16 = svt_av1_inv_txfm2d_add_32x16_c;
    svt_av1_inv_txfm2d_add_32x8 = svt_av1_inv_txfm2d_add_32x8_c;
    svt_av1_inv_txfm2d_add_8x32 = svt_av1_inv_txfm2d_add_8x32_c;
    svt_av1_inv_txfm2d_add_32x64 = svt_av1_inv_txfm2d_add_32x64_c;
    svt_av1_inv_txfm2d_add_64x32 = svt_av1_inv_txfm2d_add_64x32_c;
    svt_av1_inv_txfm2d_add_16x64 = svt_av1_inv_txfm2d_add_16x64_c;
    svt_av1_inv_txfm2d_add_64x16 = svt_av1_inv_txfm2d_add_64x16_c;
    svt_av1_inv_txfm2d_add_4x8 = svt_av1_inv_txfm2d_add_4x8_c;
    svt_av1_inv_txfm2d_add_8x4 = svt_av1_inv_txfm2d_add_8x4_c;
    svt_av1_inv_txfm2d_add_4x16 = svt_av1_inv_txfm2d_add_4x16_c;
    svt_av1_inv_txfm2d_add_16x4 = svt_av1_inv_txfm2d_add_16x4_c;
    svt_av1_fwd_txfm2d_16x16 = svt_av1_transform_two_d_16x16_c; svt_av1_fwd_txfm2d_16x8 = svt_av1_fwd_txfm2d_16x8_c; svt_av1_fwd_txfm2d_16x4 = svt_av1_fwd_txfm2d_16x4_c;
    svt_av1_fwd_txfm2d_16x16_N2 = svt_aom_transform_two_d_16x16_N2_c; svt_av1_fwd_txfm2d_16x8_N2 = svt_av1_fwd_txfm2d_16x8_N2_c; svt_av1_fwd_txfm2d_16x4_N2 = svt_av1_fwd_txfm2d_16x4_N2_c;
    svt_av1_fwd_txfm2d_16x16_N4 = svt_aom_transform_two_d_16x16_N4_c; svt_av1_fwd_txfm2d_16x8_N4 = svt_av1_fwd_txfm2d_16x8_N4_c; svt_av1_fwd_txfm2d_16x4_N4 = svt_av1_fwd_txfm2d_16x4_N4_c;
    svt_av1_fwd_txfm2d_32x32 = svt_av1_transform_two_d_32x32_c; svt_av1_fwd_txfm2d_32x16 = svt_av1_fwd_txfm2d_32x16_c; svt_av1_fwd_txfm2d_32x8 = svt_av1_fwd_txfm2d_32x8_c;
    svt_av1_fwd_txfm2d_32x32_N2 = svt_aom_transform_two_d_32x32_N2_c; svt_av1_fwd_txfm2d_32x16_N2 = svt_av1_fwd_txfm2d_32x16_N2_c; svt_av1_fwd_txfm2d_32x8_N2 = svt_av1_fwd_txfm2d_32x8_N2_c;
    svt_av1_fwd_txfm2d_32x32_N4 = svt_aom_transform_two_d_32x32_N4_c; svt_av1_fwd_txfm2d_32x16_N4 = svt_av1_fwd_txfm2d_32x16_N4_c; svt_av1_fwd_txfm2d_32x8_N4 = svt_av1_fwd_txfm2d_32x8_N4_c;
}

/* d: host pointers throughout; tpl_stats holds d->n_tpl_stats cells, tpl_src_stats d->n_tpl_src_stats entries */
int harness_dispense(const SvtHipTplDesc *d) {
    static SequenceControlSet scs;
    static EncodeContext enc;
    static PictureParentControlSet pcs;
    static MotionEstimationData me_data;
    static Av1Common cm;
    static EbPictureBufferDesc cur, rec, ref_src[2][4], ref_rec[2][4];
    memset(&scs, 0, sizeof(scs)); memset(&enc, 0, sizeof(enc)); memset(&pcs, 0, sizeof(pcs)); memset(&me_data, 0, sizeof(me_data)); memset(&cm, 0, sizeof(cm));
    const int nb64x = (d->aligned_width + 63) / 64, nb64y = (d->aligned_height + 63) / 64, n_b64 = nb64x * nb64y;
    B64Geom *geom = calloc(n_b64, sizeof(B64Geom));
    MeSbResults *res = calloc(n_b64, sizeof(MeSbResults));
    MeSbResults **resp = calloc(n_b64, sizeof(MeSbResults *));
    TplStats **cells = calloc(d->n_tpl_stats, sizeof(TplStats *));
    for (int i = 0; i < n_b64; i++) {
        geom[i].org_x = (i % nb64x) * 64; geom[i].org_y = (i / nb64x) * 64;
        if (d->me.total_me_candidate_index) {
            res[i].total_me_candidate_index = d->me.total_me_candidate_index + (size_t)i * d->n_pu;
            res[i].me_mv_array = (MvCandidate *)d->me.me_mv_array + (size_t)i * d->n_pu * d->max_refs;
            res[i].me_candidate_array = (MeCandidate *)d->me.me_candidate_array + (size_t)i * d->n_pu * d->max_cand;
        }
        resp[i] = &res[i];
    }
    for (uint32_t i = 0; i < d->n_tpl_stats; i++) cells[i] = (TplStats *)d->tpl_stats + i;
    scs.b64_geom = geom; scs.in_loop_ois = 1; scs.tpl_lad_mg = d->store_src_stats ? 1 : 0; scs.enc_ctx = &enc;
    for (int k = 0; k < 8; k++) {
        const int ac = k != 0;
        enc.quants_8bit.y_quant[0][k] = d->quant.quant[ac];        enc.quants_8bit.y_quant_fp[0][k] = d->quant.quant_fp[ac];
        enc.quants_8bit.y_round_fp[0][k] = d->quant.round_fp[ac];  enc.quants_8bit.y_quant_shift[0][k] = d->quant.quant_shift[ac];
        enc.quants_8bit.y_zbin[0][k] = d->quant.zbin[ac];          enc.quants_8bit.y_round[0][k] = d->quant.round[ac];
        enc.deq_8bit.y_dequant_qtx[0][k] = d->quant.dequant[ac];
    }
    for (int k = 0; k < MAX_TPL_LA_SW; k++) enc.poc_map_idx[k] = UINT64_MAX;
    cur = to_desc(&d->cur, d->cur.width, d->cur.height);
    rec = to_desc(&d->recon, d->recon.width, d->recon.height);
    enc.mc_flow_rec_picture_buffer[0] = &rec;
    enc.poc_map_idx[0] = UINT64_MAX - 1;
    pcs.enhanced_pic = &cur;
    pcs.aligned_width = d->aligned_width; pcs.aligned_height = d->aligned_height;
    pcs.tpl_ctrls.disable_intra_pred_nref = d->disable_intra_pred; pcs.temporal_layer_index = 0; pcs.hierarchical_levels = 0;
    pcs.tpl_ctrls.use_sad_in_src_search = d->use_sad_in_src_search; pcs.tpl_ctrls.intra_mode_end = d->intra_mode_end;
    pcs.tpl_ctrls.subpel_depth = d->subpel_depth; pcs.tpl_ctrls.compute_rate = d->compute_rate;
    pcs.tpl_ctrls.subsample_tx = d->subsample_tx; pcs.tpl_ctrls.pf_shape = d->pf_shape; pcs.tpl_ctrls.synth_blk_size = d->synth_blk_size;
    pcs.tpl_ctrls.dispenser_search_level = d->dispenser_search_level;
    pcs.tpl_src_data_ready = d->src_pass ? 0 : 1;
    pcs.enable_me_16x16 = d->enable_me_16x16;
    pcs.slice_type = d->slice_is_i ? I_SLICE : B_SLICE;
    pcs.tpl_data.tpl_slice_type = d->tpl_slice_is_i ? I_SLICE : B_SLICE;
    pcs.tpl_data.is_ref = d->is_ref;
    pcs.tpl_data.base_pcs = &pcs;
    pcs.av1_cm = &cm;
    cm.mi_rows = d->aligned_height >> 2; cm.mi_cols = d->aligned_width >> 2;
    pcs.pa_me_data = &me_data;
    me_data.me_results = resp; me_data.max_cand = d->max_cand; me_data.max_refs = d->max_refs; me_data.max_l0 = d->max_l0;
    me_data.tpl_stats = cells; me_data.tpl_src_stats_buffer = (TplSrcStats *)d->tpl_src_stats;
    for (int l = 0; l < 2; l++)
        for (int r = 0; r < 4; r++) {
            const SvtHipTplRef *t = &d->refs[l][r];
            if (!t->src.buffer_y) continue;
            const int g = 1 + l * 4 + r;
            ref_src[l][r] = to_desc(&t->src, t->max_width, t->max_height);
            ref_rec[l][r] = to_desc(&t->recon, t->max_width, t->max_height);
            pcs.tpl_data.tpl_ref_ds_ptr_array[l][r].picture_ptr = &ref_src[l][r];
            pcs.tpl_data.tpl_ref_ds_ptr_array[l][r].picture_number = t->picture_number;
            pcs.tpl_data.ref_tpl_group_idx[l][r] = g;
            pcs.tpl_valid_pic[g] = t->usable;
            pcs.tpl_data.ref_in_slide_window[l][r] = true;
            enc.poc_map_idx[g] = t->picture_number;
            enc.mc_flow_rec_picture_buffer[g] = &ref_rec[l][r];
        }
    for (int sb = 0; sb < n_b64; sb++) tpl_mc_flow_dispenser_sb_generic(&enc, &scs, &pcs, 0, sb, 0, d->dispenser_search_level);
    svt_aom_generate_padding(rec.buffer_y, rec.stride_y, rec.width, rec.height, rec.org_x, rec.org_y);
    free(geom); free(res); free(resp); free(cells);
    return 0;
}

/* Level-1 paths only (sub-pel search, rate, rdmult): never reached by levels 4 / 5; stopping here would show a wrong case */
void svt_aom_enc_make_inter_predictor(SequenceControlSet *scs, uint8_t *src_ptr, uint8_t *src_ptr_2b, uint8_t *dst_ptr, int16_t pre_y, int16_t pre_x,
                                      MV mv, const struct ScaleFactors *const sf, ConvolveParams *conv_params, InterpFilters interp_filters,
                                      InterInterCompoundData *interinter_comp, uint8_t *seg_mask, uint16_t frame_width, uint16_t frame_height,
                                      uint8_t blk_width, uint8_t blk_height, BlockSize bsize, MacroBlockD *av1xd, int32_t src_stride,
                                      int32_t dst_stride, uint8_t plane, const uint32_t ss_y, const uint32_t ss_x, uint8_t bit_depth,
                                      uint8_t use_intrabc, uint8_t is_masked_compound, uint8_t is16bit) { abort(); }
void svt_av1_set_mv_search_range(MvLimits *mv_limits, const MV *mv) { abort(); }
int svt_av1_find_best_sub_pixel_tree_pruned(void *ictx, MacroBlockD *xd, const struct AV1Common *const cm, SUBPEL_MOTION_SEARCH_PARAMS *ms_params,
                                            MV start_mv, MV *bestmv, int *distortion, unsigned int *sse1, int qp, BlockSize bsize,
                                            uint8_t is_intra_bordered) { abort(); }
AomVarianceFnPtr svt_aom_mefn_ptr[BlockSizeS_ALL];
int svt_aom_compute_rd_mult_based_on_qindex(EbBitDepth bit_depth, SvtAv1FrameUpdateType update_type, int qindex) { abort(); }

"""
SOURCES = ["Codec/enc_intra_prediction.c", "Codec/intra_prediction.c", "Codec/transforms.c", "Codec/inv_transforms.c", "Codec/pic_operators.c",
           "Codec/utility.c", "C_DEFAULT/compute_sad_c.c", "C_DEFAULT/picture_operators_c.c", "Codec/full_loop.c", "Codec/common_dsp_rtcd.c",
           "Codec/aom_dsp_rtcd.c", "Codec/svt_log.c", "Codec/mode_decision.c", "Codec/inter_prediction.c", "ASM_SSE2/pic_operators_intrin_sse2.c"]


def build(ref, tmp, harness=HARNESS):
    """Compiles the reference sources with `harness` (C text that #includes src_ops_process.c) into a library; returns it, initialised."""
    # -DNDEBUG: svt_aom_generate_r0beta asserts beta > 0, which the group cases of gen_tpl_group_golden.py do not keep; include/: the harness includes svt_hip_tpl.h
    L = refbuild.build(ref, tmp, "tplref", SOURCES, [("harness", harness)], flags=["-DNDEBUG"], includes=[os.path.join(ROOT, "include")])
    L.harness_init()
    return L


def run_ref(L, c):
    """The reference's dispense of a case: (tpl_stats, tpl_src_stats, padded recon)."""
    rec, grid, src = c["recon"].copy(), c["tpl_stats"].copy(), c["tpl_src_stats"].copy()
    refs = {k: (r["src"].ctypes.data, r["recon"].ctypes.data) for k, r in c["refs"].items()}
    me = None if c["slice_is_i"] else tuple(c["me"][k].ctypes.data for k in ("total", "mv", "cand"))
    d = tpl.make_desc(c, c.get("pad", tc.PAD), c["cur"].ctypes.data, rec.ctypes.data, refs, me, grid.ctypes.data, src.ctypes.data)
    if L.harness_dispense(C.byref(d)) != 0:
        raise RuntimeError("harness_dispense failed")
    return grid, src, rec


def generate(L):
    out = {}
    for i, (name, kw, c) in enumerate(tc.fixture_cases(lambda c: run_ref(L, c)[2])):
        g, s, r = run_ref(L, c)
        out[f"name_{i}"] = np.array(name)
        out[f"checksum_{i}"] = tc.input_checksum(c)
        out[f"tpl_stats_{i}"], out[f"tpl_src_stats_{i}"], out[f"recon_{i}"] = g, s, r
    return out


def generate_edges(L):
    """The edge cases (groups A-F and H of tpl_dispenser_cases.edge_cases; G is the project's own definition) in the same layout.  The
    recon plane is stored whole for the groups in tc.EDGE_PLANES_STORED; the others (many pictures, or large ones) store its sha256 as
    recon_sha_<i> instead, next to the full grids, to keep the file small."""
    out = {}
    for i, (name, c) in enumerate(tc.edge_cases(tc.EDGE_FIXTURE_GROUPS)):
        g, s, r = run_ref(L, c)
        out[f"name_{i}"] = np.array(name)
        out[f"checksum_{i}"] = tc.input_checksum(c)
        out[f"tpl_stats_{i}"], out[f"tpl_src_stats_{i}"] = g, s
        if name[0] in tc.EDGE_PLANES_STORED:
            out[f"recon_{i}"] = r
        else:
            out[f"recon_sha_{i}"] = tc.plane_checksum(r)
    return out


def wrote(path, out):
    return f"wrote {path}: {len([k for k in out if k.startswith('name_')])} cases, {os.path.getsize(path)} bytes"


if __name__ == "__main__":
    refbuild.main(__doc__, build, {tc.GOLDEN: generate, tc.GOLDEN_EDGES: generate_edges}, save=refbuild.savez, wrote=wrote)
