"""ctypes mirror of include/svt_hip_me.h (the C-ABI).  Pure declarations; no compute.

The structures follow the field order of the header exactly; tests/test_abi.py checks the sizes against
the compiled libraries (``svt_hip_sizeof`` / ``orc_sizeof``).
"""
import ctypes as C

import numpy as np

MAX_LISTS = 2
MAX_REFS = 4
SQUARE_PU_COUNT = 85
MAX_SAD_VALUE = 128 * 128 * 255


class SearchArea(C.Structure):
    _fields_ = [("width", C.c_uint16), ("height", C.c_uint16)]


class SearchAreaMinMax(C.Structure):
    _fields_ = [("sa_min", SearchArea), ("sa_max", SearchArea)]


class MeConfig(C.Structure):
    _fields_ = [
        ("hme_search_method", C.c_uint8), ("me_search_method", C.c_uint8),
        ("enable_hme_flag", C.c_uint8), ("enable_hme_level0_flag", C.c_uint8),
        ("enable_hme_level1_flag", C.c_uint8), ("enable_hme_level2_flag", C.c_uint8),
        ("num_hme_sa_w", C.c_uint16), ("num_hme_sa_h", C.c_uint16),
        ("hme_l0_sa", SearchAreaMinMax), ("hme_l1_sa", SearchArea), ("hme_l2_sa", SearchArea),
        ("me_sa", SearchAreaMinMax),
        ("prehme_enable", C.c_uint8), ("prehme_skip_search_line", C.c_uint8), ("prehme_l1_early_exit", C.c_uint8), ("me_type", C.c_uint8),
        ("prehme_sa_cfg", SearchAreaMinMax * 2),
        ("enable_me_hme_ref_pruning", C.c_uint8),
        ("prune_ref_if_hme_sad_dev_bigger_than_th", C.c_uint16), ("prune_ref_if_me_sad_dev_bigger_than_th", C.c_uint16),
        ("zz_sad_th", C.c_uint32), ("zz_sad_pct", C.c_uint16), ("phme_sad_th", C.c_uint32), ("phme_sad_pct", C.c_uint16),
        ("enable_me_sr_adjustment", C.c_uint8),
        ("reduce_me_sr_based_on_mv_length_th", C.c_uint16), ("stationary_hme_sad_abs_th", C.c_uint16),
        ("stationary_me_sr_divisor", C.c_uint16), ("reduce_me_sr_based_on_hme_sad_abs_th", C.c_uint16),
        ("me_sr_divisor_for_low_hme_sad", C.c_uint16), ("distance_based_hme_resizing", C.c_uint8),
        ("me_8x8_var_enabled", C.c_uint8),
        ("me_sr_div4_th", C.c_uint32), ("me_sr_div2_th", C.c_uint32), ("me_sr_mult2_th", C.c_uint32),
        ("mv_sa_adj_enabled", C.c_uint8), ("mv_sa_adj_nearest_ref_only", C.c_uint8),
        ("mv_sa_adj_mv_size_th", C.c_uint16), ("mv_sa_adj_sa_multiplier", C.c_uint16),
        ("prune_me_candidates_th", C.c_int32), ("use_best_unipred_cand_only", C.c_uint8),
        ("reduce_hme_l0_sr_th_min", C.c_uint8), ("reduce_hme_l0_sr_th_max", C.c_uint8),
        ("me_early_exit_th", C.c_uint32), ("me_safe_limit_zz_th", C.c_uint32), ("prev_me_stage_based_exit_th", C.c_uint32),
    ]

    def as_dict(self):
        def conv(v):
            if isinstance(v, C.Structure):
                return {n: conv(getattr(v, n)) for n, _ in v._fields_}
            if isinstance(v, C.Array):
                return [conv(x) for x in v]
            return int(v)
        return conv(self)


class MePresetDesc(C.Structure):
    _fields_ = [
        ("enc_mode", C.c_int8), ("input_resolution", C.c_uint8), ("sc_class1", C.c_uint8), ("rtc_tune", C.c_uint8),
        ("temporal_layer_index", C.c_uint8), ("hierarchical_levels", C.c_uint8),
        ("qp", C.c_uint32), ("frame_rate_q16", C.c_uint32), ("safe_limit_nref", C.c_uint8), ("safe_limit_zz_th", C.c_uint32),
    ]


class PlaneDesc(C.Structure):
    _fields_ = [
        ("buffer_y", C.c_void_p), ("stride_y", C.c_uint32), ("org_x", C.c_uint16), ("org_y", C.c_uint16),
        ("width", C.c_uint16), ("height", C.c_uint16),
    ]


class MePictureDesc(C.Structure):
    _fields_ = [
        ("picture_number", C.c_uint64), ("aligned_width", C.c_uint16), ("aligned_height", C.c_uint16),
        ("num_of_list_to_search", C.c_uint8), ("num_of_ref_pic_to_search", C.c_uint8 * MAX_LISTS),
        ("temporal_layer_index", C.c_uint8), ("hierarchical_levels", C.c_uint8), ("is_ref", C.c_uint8),
        ("similar_brightness_refs", C.c_uint8), ("enable_me_8x8", C.c_uint8), ("enable_me_16x16", C.c_uint8),
        ("max_number_of_pus_per_sb", C.c_uint8), ("max_cand", C.c_uint8), ("max_refs", C.c_uint8), ("max_l0", C.c_uint8),
        ("input_resolution", C.c_uint8), ("only_l_bwd", C.c_uint8), ("gm_enabled", C.c_uint8),
        ("gm_use_distance_based_active_th", C.c_uint8), ("b64_row_start", C.c_uint16), ("b64_row_count", C.c_uint16), ("tf_me_exit_th", C.c_uint32),
        ("ref_picture_number", (C.c_uint64 * MAX_REFS) * MAX_LISTS),
    ]


class MeResults(C.Structure):
    _fields_ = [
        ("total_me_candidate_index", C.c_void_p), ("me_mv_array", C.c_void_p), ("me_candidate_array", C.c_void_p),
        ("me_64x64_distortion", C.c_void_p), ("me_32x32_distortion", C.c_void_p), ("me_16x16_distortion", C.c_void_p),
        ("me_8x8_distortion", C.c_void_p), ("rc_me_distortion", C.c_void_p), ("me_8x8_cost_variance", C.c_void_p),
        ("stationary_block_present_sb", C.c_void_p), ("rc_me_allow_gm", C.c_void_p),
        ("sb_best_sad", C.c_void_p), ("sb_best_mv", C.c_void_p), ("hme_sc", C.c_void_p), ("hme_sad", C.c_void_p),
        ("do_ref", C.c_void_p),
    ]


class InvTxBatchDesc(C.Structure):
    """SvtHipInvTxBatchDesc (include/svt_hip_dsp.h)."""
    _fields_ = [("bit_depth", C.c_uint8), ("sample_bytes", C.c_uint8), ("tx_size", C.c_uint8), ("reserved", C.c_uint8), ("n_jobs", C.c_uint32),
                ("pred_stride", C.c_uint32), ("recon_stride", C.c_uint32), ("pred", C.c_void_p), ("recon", C.c_void_p), ("jobs", C.c_void_p),
                ("dqcoeff", C.c_void_p)]


class FwdTxBatchDesc(C.Structure):
    """SvtHipFwdTxBatchDesc (include/svt_hip_dsp.h)."""
    _fields_ = [("tx_size", C.c_uint8), ("reserved", C.c_uint8 * 3), ("n_jobs", C.c_uint32), ("residual_stride", C.c_uint32), ("residual", C.c_void_p),
                ("jobs", C.c_void_p), ("coeff", C.c_void_p)]


class PredJob(C.Structure):
    """SvtHipPredJob (include/svt_hip_dsp.h)."""
    _fields_ = [("ref", C.c_void_p), ("sb_best_mv", C.c_void_p), ("pred", C.c_void_p), ("b64_row_start", C.c_uint32), ("b64_row_count", C.c_uint32),
                ("list", C.c_uint8), ("ref_idx", C.c_uint8), ("reserved", C.c_uint8 * 6)]


class DgMetrics(C.Structure):
    """SvtHipDgMetrics (include/svt_hip_me.h)."""
    _fields_ = [("tot_dist", C.c_uint64), ("tot_cplx", C.c_uint32), ("tot_active", C.c_uint32), ("sum_in_vectors", C.c_int32),
                ("reserved", C.c_uint32)]

    def as_dict(self):
        return {"tot_dist": self.tot_dist, "tot_cplx": self.tot_cplx, "tot_active": self.tot_active, "sum_in_vectors": self.sum_in_vectors}


class MeJob(C.Structure):
    _fields_ = [("cfg", C.c_void_p), ("desc", C.c_void_p), ("cur", C.c_void_p), ("refs", (C.c_void_p * 4) * 2), ("results", C.c_void_p)]


# (field, numpy dtype, per-b64 element count as a function of (n_pu, max_refs, max_cand))
RESULT_FIELDS = [
    ("total_me_candidate_index", "u1", lambda n, r, c: n),
    ("me_mv_array", "u4", lambda n, r, c: n * r),
    ("me_candidate_array", "u1", lambda n, r, c: n * c),
    ("me_64x64_distortion", "u4", lambda n, r, c: 1), ("me_32x32_distortion", "u4", lambda n, r, c: 1),
    ("me_16x16_distortion", "u4", lambda n, r, c: 1), ("me_8x8_distortion", "u4", lambda n, r, c: 1),
    ("rc_me_distortion", "u4", lambda n, r, c: 1), ("me_8x8_cost_variance", "u4", lambda n, r, c: 1),
    ("stationary_block_present_sb", "u1", lambda n, r, c: 1), ("rc_me_allow_gm", "u1", lambda n, r, c: 1),
    ("sb_best_sad", "u4", lambda n, r, c: 2 * 4 * 85), ("sb_best_mv", "u4", lambda n, r, c: 2 * 4 * 85),
    ("hme_sc", "i2", lambda n, r, c: 2 * 4 * 2), ("hme_sad", "u4", lambda n, r, c: 2 * 4), ("do_ref", "u1", lambda n, r, c: 2 * 4),
]


def n_pu(enable_me_16x16, enable_me_8x8):
    return (85 if enable_me_8x8 else 21) if enable_me_16x16 else 5


# ---- include/svt_hip_dsp.h ------------------------------------------------------------------------------
class QuantRow(C.Structure):
    _fields_ = [("zbin", C.c_int16 * 2), ("round", C.c_int16 * 2), ("quant", C.c_int16 * 2), ("quant_shift", C.c_int16 * 2),
                ("round_fp", C.c_int16 * 2), ("quant_fp", C.c_int16 * 2), ("dequant", C.c_int16 * 2)]


class TxJob(C.Structure):
    _fields_ = [("src_offset", C.c_uint32), ("pred_offset", C.c_uint32), ("tx_type", C.c_uint8), ("quant_row", C.c_uint8),
                ("pf_shape", C.c_uint8), ("reserved", C.c_uint8)]


class RdBatchDesc(C.Structure):
    _fields_ = [("bit_depth", C.c_uint8), ("quant_kind", C.c_uint8), ("tx_size", C.c_uint8), ("reserved", C.c_uint8),
                ("n_jobs", C.c_uint32), ("src_stride", C.c_uint32), ("pred_stride", C.c_uint32),
                ("src", C.c_void_p), ("pred", C.c_void_p), ("recon", C.c_void_p), ("jobs", C.c_void_p), ("quant_rows", C.c_void_p),
                ("n_quant_rows", C.c_uint32),
                ("eob", C.c_void_p), ("satd", C.c_void_p), ("dist_coeff", C.c_void_p), ("three_quad_energy", C.c_void_p), ("sse", C.c_void_p),
                ("coeff", C.c_void_p), ("qcoeff", C.c_void_p), ("dqcoeff", C.c_void_p), ("qmatrix", C.c_void_p), ("iqmatrix", C.c_void_p),
                ("cul_level", C.c_void_p)]


TX_W = [4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64]
TX_H = [4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16]
JOB_DTYPE = [("src_offset", "<u4"), ("pred_offset", "<u4"), ("tx_type", "u1"), ("quant_row", "u1"), ("pf_shape", "u1"), ("reserved", "u1")]
QUANT_ROW_DTYPE = [(n, "<i2", (2,)) for n in ("zbin", "round", "quant", "quant_shift", "round_fp", "quant_fp", "dequant")]
RD_OUT_FIELDS = [("eob", "<u2", 1), ("satd", "<u4", 1), ("dist_coeff", "<u8", 2), ("three_quad_energy", "<u8", 1), ("sse", "<u8", 1), ("cul_level", "u1", 1)]


class BlockJob(C.Structure):
    _fields_ = [("src_offset", C.c_uint32), ("ref_offset", C.c_uint32), ("width", C.c_uint8), ("height", C.c_uint8), ("subpel_x", C.c_uint8), ("subpel_y", C.c_uint8)]


class BlockStatsDesc(C.Structure):
    _fields_ = [("bit_depth", C.c_uint8), ("temporal_layer_index", C.c_uint8), ("spy_rd", C.c_uint8), ("reserved", C.c_uint8), ("n_jobs", C.c_uint32),
                ("src_stride", C.c_uint32), ("ref_stride", C.c_uint32),
                ("src", C.c_void_p), ("ref", C.c_void_p), ("jobs", C.c_void_p),
                ("sad", C.c_void_p), ("sse", C.c_void_p), ("variance", C.c_void_p), ("var_sse", C.c_void_p), ("satd", C.c_void_p),
                ("psy_rd", C.c_double), ("psy_energy", C.c_void_p), ("psy_dist", C.c_void_p),
                ("psy_sse", C.c_void_p), ("pred_mode", C.c_void_p), ("compound_type", C.c_void_p), ("facade_dist", C.c_void_p),
                ("variance10", C.c_void_p), ("var_sse10", C.c_void_p),
                ("n_pyramids", C.c_uint32), ("pyramid_out_base", C.c_uint32), ("pyramids", C.c_void_p)]


class SsimBatchDesc(C.Structure):  # SvtHipSsimBatchDesc
    _fields_ = [("bit_depth", C.c_uint8), ("reserved", C.c_uint8 * 3), ("n_jobs", C.c_uint32), ("src_stride", C.c_uint32), ("ref_stride", C.c_uint32),
                ("src", C.c_void_p), ("ref", C.c_void_p), ("jobs", C.c_void_p), ("psy_rd", C.c_double), ("ssim", C.c_void_p), ("ssim_dist", C.c_void_p),
                ("n_pyramids", C.c_uint32), ("pyramid_out_base", C.c_uint32), ("pyramids", C.c_void_p)]


SSIM_OUT_FIELDS = [("ssim", "<f8"), ("ssim_dist", "<u8")]
PYRAMID_BLOCKS = 85  # nested square blocks of a 64x64 region: 1 + 4 + 16 + 64, each level in raster order
BLOCK_JOB_DTYPE = [("src_offset", "<u4"), ("ref_offset", "<u4"), ("width", "u1"), ("height", "u1"), ("subpel_x", "u1"), ("subpel_y", "u1")]
STATS_OUT_FIELDS = [("sad", "<u4"), ("sse", "<u8"), ("variance", "<u4"), ("var_sse", "<u4"), ("satd", "<u4")]
PSY_OUT_FIELDS = [("psy_energy", "<u8"), ("psy_dist", "<u8"), ("psy_sse", "<u8")]
FACADE_OUT_FIELDS = [("facade_dist", "<u8")]
VAR10_OUT_FIELDS = [("variance10", "<u4"), ("var_sse10", "<u4")]  # 10-bit planes only
VARIANCE_SIZES = [(4, 4), (4, 8), (4, 16), (8, 4), (8, 8), (8, 16), (8, 32), (16, 4), (16, 8), (16, 16), (16, 32), (16, 64), (32, 8), (32, 16),
                  (32, 32), (32, 64), (64, 16), (64, 32), (64, 64), (64, 128), (128, 64), (128, 128)]


class LvMapCoeffCost(C.Structure):  # SvtHipLvMapCoeffCost
    _fields_ = [("txb_skip_cost", (C.c_int32 * 2) * 13), ("base_eob_cost", (C.c_int32 * 3) * 4), ("base_cost", (C.c_int32 * 8) * 42),
                ("eob_extra_cost", (C.c_int32 * 2) * 22), ("dc_sign_cost", (C.c_int32 * 2) * 3), ("lps_cost", (C.c_int32 * 26) * 21)]


class LvMapEobCost(C.Structure):  # SvtHipLvMapEobCost
    _fields_ = [("eob_cost", (C.c_int32 * 11) * 2)]


class RateTables(C.Structure):  # SvtHipRateTables
    _fields_ = [("coeff_fac_bits", (LvMapCoeffCost * 2) * 5), ("eob_frac_bits", (LvMapEobCost * 2) * 7),
                ("intra_tx_type_fac_bits", ((((C.c_int32 * 17) * 13) * 4) * 3)), ("inter_tx_type_fac_bits", ((C.c_int32 * 17) * 4) * 4)]


class RateJob(C.Structure):  # SvtHipRateJob
    _fields_ = [("tx_type", C.c_uint8), ("txb_skip_ctx", C.c_uint8), ("dc_sign_ctx", C.c_uint8), ("is_inter", C.c_uint8), ("intra_dir", C.c_uint8),
                ("reserved", C.c_uint8 * 3)]


class CoeffRateDesc(C.Structure):  # SvtHipCoeffRateDesc
    _fields_ = [("tx_size", C.c_uint8), ("plane_type", C.c_uint8), ("reduced_tx_set", C.c_uint8), ("coeff_rate_est_lvl", C.c_uint8),
                ("mds_fast_coeff_est_level", C.c_uint8), ("mds_subres_step", C.c_uint8), ("reserved", C.c_uint8 * 2), ("n_jobs", C.c_uint32),
                ("n_groups", C.c_uint32), ("jobs", C.c_void_p), ("tables", C.c_void_p), ("qcoeff", C.c_void_p), ("eob", C.c_void_p), ("bits", C.c_void_p),
                ("lambda_", C.c_uint32), ("dist_stride", C.c_uint32), ("dist", C.c_void_p), ("rd_cost", C.c_void_p),
                ("group_start", C.c_void_p), ("best_job", C.c_void_p), ("best_cost", C.c_void_p)]


RATE_JOB_DTYPE = [("tx_type", "u1"), ("txb_skip_ctx", "u1"), ("dc_sign_ctx", "u1"), ("is_inter", "u1"), ("intra_dir", "u1"), ("reserved", "u1", (3,))]
# the members of SvtHipRateTables in their order, as int32 arrays (an LvMapCoeffCost is 970 int32, an LvMapEobCost 22)
RATE_TABLE_SHAPES = [("coeff_fac_bits", (5, 2, 970)), ("eob_frac_bits", (7, 2, 2, 11)), ("intra_tx_type_fac_bits", (3, 4, 13, 17)),
                     ("inter_tx_type_fac_bits", (4, 4, 17))]
RATE_UNDEFINED = 0xFFFFFFFFFFFFFFFF  # bits / rd_cost / best_cost of a job (group) the reference leaves undefined
RATE_NO_JOB = 0xFFFFFFFF             # best_job of such a group



class RdoqJob(C.Structure):  # SvtHipRdoqJob
    _fields_ = [("tx_type", C.c_uint8), ("txb_skip_ctx", C.c_uint8), ("dc_sign_ctx", C.c_uint8), ("is_inter", C.c_uint8), ("quant_row", C.c_uint8),
                ("flags", C.c_uint8), ("reserved", C.c_uint8 * 2)]


class RdoqDesc(C.Structure):  # SvtHipRdoqDesc
    _fields_ = [("tx_size", C.c_uint8), ("plane_type", C.c_uint8), ("sharpness", C.c_uint8), ("eob_fast_inter", C.c_uint8), ("eob_fast_intra", C.c_uint8),
                ("eob_th", C.c_uint8), ("eob_fast_th", C.c_uint8), ("reserved", C.c_uint8), ("n_jobs", C.c_uint32), ("lambda_", C.c_uint32),
                ("jobs", C.c_void_p), ("tables", C.c_void_p), ("quant_rows", C.c_void_p), ("n_quant_rows", C.c_uint32), ("reserved2", C.c_uint32),
                ("iqmatrix", C.c_void_p), ("coeff", C.c_void_p), ("qcoeff", C.c_void_p), ("dqcoeff", C.c_void_p), ("eob", C.c_void_p),
                ("status", C.c_void_p), ("dist_coeff", C.c_void_p), ("cul_level", C.c_void_p),
                ("qcoeff_b", C.c_void_p), ("dqcoeff_b", C.c_void_p), ("eob_b", C.c_void_p)]


RDOQ_JOB_DTYPE = [("tx_type", "u1"), ("txb_skip_ctx", "u1"), ("dc_sign_ctx", "u1"), ("is_inter", "u1"), ("quant_row", "u1"), ("flags", "u1"),
                  ("reserved", "u1", (2,))]
RDOQ_FLAG_SHARP = 1
# SvtHipRdoqDesc.status
RDOQ_OPTIMISED, RDOQ_EMPTY, RDOQ_GATED, RDOQ_UNDEFINED = 0, 1, 2, 0xFF

# ---- include/svt_hip_pme.h ----
class Mv(C.Structure):
    _fields_ = [("row", C.c_int16), ("col", C.c_int16)]


class MvCostParam(C.Structure):  # MV_COST_PARAMS, Codec/mcomp.h:37-48
    _fields_ = [("ref_mv", C.POINTER(Mv)), ("full_ref_mv", Mv), ("mv_cost_type", C.c_uint8), ("mvjcost", C.c_void_p), ("mvcost", C.c_void_p * 2),
                ("error_per_bit", C.c_int), ("early_exit_th", C.c_int), ("sad_per_bit", C.c_int)]


PME_JOB_DTYPE = np.dtype([("src_offset", "<u4"), ("ref_offset", "<u4"), ("width", "u1"), ("height", "u1"), ("start_x", "<i2"), ("start_y", "<i2"), ("sa_w", "<i2"),
                          ("sa_h", "<i2"), ("step", "<i2"), ("mvx", "<i2"), ("mvy", "<i2"), ("ref_mv", "<i2", (2,)), ("best_cost", "<u4"), ("best_mvx", "<i2"),
                          ("best_mvy", "<i2")], align=True)


class PmeBatchDesc(C.Structure):
    _fields_ = [("n_jobs", C.c_uint32), ("src_stride", C.c_uint32), ("ref_stride", C.c_uint32), ("src", C.c_void_p), ("ref", C.c_void_p), ("jobs", C.c_void_p),
                ("mv_cost_type", C.c_int32), ("error_per_bit", C.c_int32), ("mvjcost", C.c_void_p), ("mvcost", C.c_void_p * 2), ("best_cost", C.c_void_p),
                ("best_mv", C.c_void_p)]


# ---- include/svt_hip_md_search.h ----
FULLPEL_JOB_DTYPE = np.dtype([("src_offset", "<u4"), ("blk_org_x", "<i4"), ("blk_org_y", "<i4"), ("width", "u1"), ("height", "u1"), ("dist_type", "u1"), ("flags", "u1"),
                              ("mvx", "<i2"), ("mvy", "<i2"), ("start_x", "<i2"), ("end_x", "<i2"), ("start_y", "<i2"), ("end_y", "<i2"), ("step", "<i2"),
                              ("sprs_lev0_start_x", "<i2"), ("sprs_lev0_end_x", "<i2"), ("sprs_lev0_start_y", "<i2"), ("sprs_lev0_end_y", "<i2"), ("ref_mv", "<i2", (2,)),
                              ("best_cost", "<u4"), ("best_mvx", "<i2"), ("best_mvy", "<i2"), ("chain_from", "<i4")], align=True)
FP_CENTRE_FROM_CHAIN, FP_BEST_FROM_CHAIN, FP_SPRS_LEV0_DONE, FP_ENABLE_PSAD = 1, 2, 4, 8


class FullpelBatchDesc(C.Structure):
    _fields_ = [("n_jobs", C.c_uint32), ("src_stride", C.c_uint32), ("ref_stride", C.c_uint32), ("src", C.c_void_p), ("ref", C.c_void_p), ("ref_org_x", C.c_int32),
                ("ref_org_y", C.c_int32), ("ref_max_width", C.c_int32), ("ref_max_height", C.c_int32), ("jobs", C.c_void_p), ("mv_cost_type", C.c_int32),
                ("error_per_bit", C.c_int32), ("mvjcost", C.c_void_p), ("mvcost", C.c_void_p * 2), ("best_cost", C.c_void_p), ("best_mv", C.c_void_p)]


SUBPEL_JOB_DTYPE = np.dtype([("src_offset", "<u4"), ("ref_offset", "<u4"), ("width", "u1"), ("height", "u1"), ("log2_pels", "u1"), ("early_neigh_check_exit", "u1"),
                             ("start_mv", "<i2", (2,)), ("ref_mv", "<i2", (2,)), ("col_min", "<i2"), ("col_max", "<i2"), ("row_min", "<i2"), ("row_max", "<i2"),
                             ("early_exit_th", "<i4"), ("best_mvp_dist", "<u4"), ("best_mvp", "<i2", (2,))], align=True)
USE_2_TAPS, USE_4_TAPS, USE_8_TAPS = 1, 2, 3


class SubpelBatchDesc(C.Structure):
    _fields_ = [("n_jobs", C.c_uint32), ("src_stride", C.c_uint32), ("ref_stride", C.c_uint32), ("src", C.c_void_p), ("ref", C.c_void_p), ("jobs", C.c_void_p),
                ("allow_hp", C.c_int32), ("forced_stop", C.c_int32), ("iters_per_step", C.c_int32), ("pred_variance_th", C.c_int32), ("abs_th_mult", C.c_int32),
                ("round_dev_th", C.c_int32), ("skip_diag_refinement", C.c_int32), ("bias_fp", C.c_int32), ("qp", C.c_int32), ("search_method", C.c_int32),
                ("subpel_search_type", C.c_int32), ("mvp_th", C.c_int32), ("hp_mv_th", C.c_int32), ("mv_cost_type", C.c_int32),
                ("error_per_bit", C.c_int32), ("mvjcost", C.c_void_p), ("mvcost", C.c_void_p * 2), ("best_mv", C.c_void_p), ("besterr", C.c_void_p),
                ("distortion", C.c_void_p), ("sse", C.c_void_p), ("center_err", C.c_void_p)]


# ---- include/svt_hip_tpl.h ----
TPL_STATS_DTYPE = np.dtype([("srcrf_dist", "<i8"), ("recrf_dist", "<i8"), ("srcrf_rate", "<i8"), ("recrf_rate", "<i8"), ("mc_dep_rate", "<i8"),
                            ("mc_dep_dist", "<i8"), ("mv_row", "<i2"), ("mv_col", "<i2"), ("reserved", "<u4"), ("ref_frame_poc", "<u8")])
TPL_SRC_STATS_DTYPE = np.dtype([("srcrf_dist", "<i8"), ("srcrf_rate", "<i8"), ("ref_frame_poc", "<u8"), ("mv_row", "<i2"), ("mv_col", "<i2"),
                                ("best_mode", "u1"), ("reserved", "u1", (3,)), ("best_rf_idx", "<i4"), ("best_intra_mode", "u1"),
                                ("reserved2", "u1", (3,))])
TPL_PAD = 32


class TplRef(C.Structure):  # SvtHipTplRef
    _fields_ = [("src", PlaneDesc), ("recon", PlaneDesc), ("picture_number", C.c_uint64), ("max_width", C.c_uint16), ("max_height", C.c_uint16),
                ("usable", C.c_uint8), ("reserved", C.c_uint8 * 3)]


class TplDesc(C.Structure):  # SvtHipTplDesc
    _fields_ = [("cur", PlaneDesc), ("aligned_width", C.c_uint16), ("aligned_height", C.c_uint16), ("recon", PlaneDesc), ("me", MeResults),
                ("n_pu", C.c_uint8), ("max_cand", C.c_uint8), ("max_refs", C.c_uint8), ("max_l0", C.c_uint8), ("enable_me_16x16", C.c_uint8),
                ("reserved0", C.c_uint8 * 3), ("refs", (TplRef * MAX_REFS) * MAX_LISTS),
                ("dispenser_search_level", C.c_uint8), ("subsample_tx", C.c_uint8), ("pf_shape", C.c_uint8), ("synth_blk_size", C.c_uint8),
                ("disable_intra_pred", C.c_uint8), ("is_ref", C.c_uint8), ("slice_is_i", C.c_uint8), ("tpl_slice_is_i", C.c_uint8),
                ("src_pass", C.c_uint8), ("store_src_stats", C.c_uint8), ("use_sad_in_src_search", C.c_uint8), ("intra_mode_end", C.c_uint8),
                ("subpel_depth", C.c_uint8), ("compute_rate", C.c_uint8), ("in_loop_ois", C.c_uint8), ("reserved1", C.c_uint8 * 3),
                ("quant", QuantRow), ("tpl_stats", C.c_void_p), ("n_tpl_stats", C.c_uint32), ("n_tpl_src_stats", C.c_uint32), ("tpl_src_stats", C.c_void_p)]

TPL_MAX_GROUP = 512
TPL_STAGE_DISPENSE, TPL_STAGE_SYNTHESIZE, TPL_STAGE_R0BETA = 1, 2, 4


class TplGroupFrame(C.Structure):  # SvtHipTplGroupFrame
    _fields_ = [("picture_number", C.c_uint64), ("tpl_valid_pic", C.c_uint8), ("reserved", C.c_uint8 * 3), ("base_rdmult", C.c_int32),
                ("tpl_stats", C.c_void_p), ("n_tpl_stats", C.c_uint32), ("n_beta", C.c_uint32), ("dispense", C.POINTER(TplDesc)),
                ("r0", C.c_void_p), ("tpl_is_valid", C.c_void_p), ("beta", C.c_void_p), ("scaling", C.c_void_p), ("n_scaling", C.c_uint32),
                ("reserved2", C.c_uint32)]


class TplGroupDesc(C.Structure):  # SvtHipTplGroupDesc
    _fields_ = [("width", C.c_uint16), ("height", C.c_uint16), ("aligned_width", C.c_uint16), ("aligned_height", C.c_uint16),
                ("synth_blk_size", C.c_uint8), ("sb_size", C.c_uint8), ("compute_rate", C.c_uint8), ("superres_denom", C.c_uint8),
                ("stages", C.c_uint32), ("n_frames", C.c_uint32), ("frames", C.POINTER(TplGroupFrame))]


# ---- include/svt_hip_pred.h ----
INTER_PRED_MAX_REFS = 8
INTER_PRED_NO_REF = 0xFF
INTER_PRED_MV0_FROM_ARRAY, INTER_PRED_MV1_FROM_ARRAY = 1, 2
INTER_PRED_OK, INTER_PRED_UNDEFINED = 0, 0xFF


class InterPredRef(C.Structure):  # SvtHipInterPredRef
    _fields_ = [("plane", C.c_void_p), ("stride", C.c_uint32), ("org_x", C.c_uint16), ("org_y", C.c_uint16), ("width", C.c_uint16), ("height", C.c_uint16),
                ("reserved", C.c_uint32)]


class InterPredJob(C.Structure):  # SvtHipInterPredJob
    _fields_ = [("dst_offset", C.c_uint32), ("org_x", C.c_int16), ("org_y", C.c_int16), ("width", C.c_uint8), ("height", C.c_uint8), ("filter_x", C.c_uint8),
                ("filter_y", C.c_uint8), ("ref", C.c_uint8 * 2), ("flags", C.c_uint8), ("comp_mode", C.c_uint8), ("mv", (C.c_int16 * 2) * 2),
                ("mv_index", C.c_uint32 * 2), ("mb_to_left_edge", C.c_int32), ("mb_to_right_edge", C.c_int32), ("mb_to_top_edge", C.c_int32),
                ("mb_to_bottom_edge", C.c_int32), ("fwd_offset", C.c_uint8), ("bck_offset", C.c_uint8), ("reserved", C.c_uint8 * 6)]


class InterPredDesc(C.Structure):  # SvtHipInterPredDesc
    _fields_ = [("bit_depth", C.c_uint8), ("ss_x", C.c_uint8), ("ss_y", C.c_uint8), ("n_refs", C.c_uint8), ("n_jobs", C.c_uint32),
                ("refs", InterPredRef * INTER_PRED_MAX_REFS), ("dst", C.c_void_p), ("dst_stride", C.c_uint32), ("reserved", C.c_uint32),
                ("dst_samples", C.c_uint64), ("jobs", C.c_void_p), ("mv_array", C.c_void_p), ("n_mvs", C.c_uint32), ("reserved2", C.c_uint32),
                ("status", C.c_void_p)]


INTER_PRED_JOB_DTYPE = [("dst_offset", "<u4"), ("org_x", "<i2"), ("org_y", "<i2"), ("width", "u1"), ("height", "u1"), ("filter_x", "u1"), ("filter_y", "u1"),
                        ("ref", "u1", (2,)), ("flags", "u1"), ("comp_mode", "u1"), ("mv", "<i2", (2, 2)), ("mv_index", "<u4", (2,)),
                        ("mb_to_left_edge", "<i4"), ("mb_to_right_edge", "<i4"), ("mb_to_top_edge", "<i4"), ("mb_to_bottom_edge", "<i4"),
                        ("fwd_offset", "u1"), ("bck_offset", "u1"), ("reserved", "u1", (6,))]


# ---- include/svt_hip_intra.h ----
INTRA_PRED_NO_FILTER_INTRA = 5
INTRA_PRED_OK, INTRA_PRED_UNDEFINED = 0, 0xFF


class IntraPredJob(C.Structure):  # SvtHipIntraPredJob
    _fields_ = [("dst_offset", C.c_uint32), ("nbr_x", C.c_int32), ("nbr_y", C.c_int32), ("tx_size", C.c_uint8), ("mode", C.c_uint8), ("angle_delta", C.c_int8),
                ("filter_intra_mode", C.c_uint8), ("n_top_px", C.c_uint8), ("n_topright_px", C.c_uint8), ("n_left_px", C.c_uint8), ("n_bottomleft_px", C.c_uint8),
                ("filt_type", C.c_uint8), ("reserved", C.c_uint8 * 3)]


class IntraPredDesc(C.Structure):  # SvtHipIntraPredDesc
    _fields_ = [("bit_depth", C.c_uint8), ("disable_edge_filter", C.c_uint8), ("reserved", C.c_uint8 * 2), ("n_jobs", C.c_uint32), ("nbr", C.c_void_p),
                ("nbr_stride", C.c_uint32), ("nbr_width", C.c_uint32), ("nbr_height", C.c_uint32), ("reserved2", C.c_uint32), ("dst", C.c_void_p),
                ("dst_stride", C.c_uint32), ("reserved3", C.c_uint32), ("dst_samples", C.c_uint64), ("jobs", C.c_void_p), ("status", C.c_void_p)]


INTRA_PRED_JOB_DTYPE = [("dst_offset", "<u4"), ("nbr_x", "<i4"), ("nbr_y", "<i4"), ("tx_size", "u1"), ("mode", "u1"), ("angle_delta", "i1"),
                        ("filter_intra_mode", "u1"), ("n_top_px", "u1"), ("n_topright_px", "u1"), ("n_left_px", "u1"), ("n_bottomleft_px", "u1"),
                        ("filt_type", "u1"), ("reserved", "u1", (3,))]


# ---- include/svt_hip_cfl.h ----
CFL_SLOTS = 33
CFL_OK, CFL_UNDEFINED = 0, 0xFF
CFL_PICK_TRUNCATED, CFL_PICK_UNDEFINED = 1, 0xFF
CFL_MAX_MODE_COST = 13754408443200 * 8


class CflPredJob(C.Structure):  # SvtHipCflPredJob
    _fields_ = [("luma_x", C.c_int32), ("luma_y", C.c_int32), ("dc_offset", C.c_uint32 * 2), ("dst_offset", C.c_uint32 * 2)]


class CflPlane(C.Structure):  # SvtHipCflPlane
    _fields_ = [("dc", C.c_void_p), ("dc_stride", C.c_uint32), ("dst_stride", C.c_uint32), ("dc_samples", C.c_uint64), ("dst", C.c_void_p),
                ("dst_samples", C.c_uint64)]


class CflPredDesc(C.Structure):  # SvtHipCflPredDesc
    _fields_ = [("bit_depth", C.c_uint8), ("width", C.c_uint8), ("height", C.c_uint8), ("n_alpha", C.c_uint8), ("n_jobs", C.c_uint32),
                ("alpha_q3", C.c_int8 * CFL_SLOTS), ("reserved", C.c_uint8 * 7), ("luma", C.c_void_p), ("luma_stride", C.c_uint32),
                ("luma_width", C.c_uint32), ("luma_height", C.c_uint32), ("slot_stride", C.c_uint32), ("plane", CflPlane * 2), ("jobs", C.c_void_p),
                ("status", C.c_void_p), ("ac", C.c_void_p)]


class CflPickDesc(C.Structure):  # SvtHipCflPickDesc
    _fields_ = [("n_blocks", C.c_uint32), ("lambda_", C.c_uint32), ("itr_th", C.c_uint8), ("n_mag", C.c_uint8), ("reserved", C.c_uint8 * 2),
                ("dist_stride", C.c_uint32), ("bits", C.c_void_p), ("dist", C.c_void_p), ("mode_bits", C.c_void_p), ("alpha_fac_bits", C.c_void_p),
                ("best_rd", C.c_void_p), ("cfl_alpha_idx", C.c_void_p), ("cfl_alpha_signs", C.c_void_p), ("status", C.c_void_p)]


CFL_PRED_JOB_DTYPE = [("luma_x", "<i4"), ("luma_y", "<i4"), ("dc_offset", "<u4", (2,)), ("dst_offset", "<u4", (2,))]


# ---- include/svt_hip_warp.h ----
WARP_MAX_REFS = 8
WARP_NO_REF = 0xFF
WARP_MODEL0_FROM_ARRAY, WARP_MODEL1_FROM_ARRAY = 1, 2
WARP_MV_FROM_ARRAY = 1
WARP_OK, WARP_NO_MODEL, WARP_UNDEFINED = 0, 0xFE, 0xFF
WARP_ROTZOOM, WARP_AFFINE = 2, 3
WARP_MAX_SAMPLES = 8


class WarpModel(C.Structure):  # SvtHipWarpModel
    _fields_ = [("wmmat", C.c_int32 * 6), ("alpha", C.c_int16), ("beta", C.c_int16), ("gamma", C.c_int16), ("delta", C.c_int16), ("wmtype", C.c_uint8),
                ("valid", C.c_uint8), ("num_samples", C.c_uint16), ("reserved", C.c_uint32)]


class WarpRef(C.Structure):  # SvtHipWarpRef
    _fields_ = [("plane", C.c_void_p), ("stride", C.c_uint32), ("org_x", C.c_uint16), ("org_y", C.c_uint16), ("width", C.c_uint16), ("height", C.c_uint16),
                ("rows", C.c_uint16), ("reserved", C.c_uint16)]


class WarpPredJob(C.Structure):  # SvtHipWarpPredJob
    _fields_ = [("dst_offset", C.c_uint32), ("p_col", C.c_int16), ("p_row", C.c_int16), ("width", C.c_uint8), ("height", C.c_uint8), ("ref", C.c_uint8 * 2),
                ("flags", C.c_uint8), ("comp_mode", C.c_uint8), ("fwd_offset", C.c_uint8), ("bck_offset", C.c_uint8), ("model_index", C.c_uint32 * 2),
                ("model", WarpModel * 2)]


class WarpPredDesc(C.Structure):  # SvtHipWarpPredDesc
    _fields_ = [("bit_depth", C.c_uint8), ("ss_x", C.c_uint8), ("ss_y", C.c_uint8), ("n_refs", C.c_uint8), ("n_jobs", C.c_uint32),
                ("refs", WarpRef * WARP_MAX_REFS), ("dst", C.c_void_p), ("dst_stride", C.c_uint32), ("reserved", C.c_uint32), ("dst_samples", C.c_uint64),
                ("jobs", C.c_void_p), ("models", C.c_void_p), ("n_models", C.c_uint32), ("reserved2", C.c_uint32), ("status", C.c_void_p)]


class WarpModelJob(C.Structure):  # SvtHipWarpModelJob
    _fields_ = [("pts", C.c_int32 * 16), ("pts_inref", C.c_int32 * 16), ("blk_org_x", C.c_uint16), ("blk_org_y", C.c_uint16), ("bwidth", C.c_uint8),
                ("bheight", C.c_uint8), ("n_samples", C.c_uint8), ("flags", C.c_uint8), ("mv", C.c_int16 * 2), ("mv_index", C.c_uint32)]


class WarpModelDesc(C.Structure):  # SvtHipWarpModelDesc
    _fields_ = [("n_jobs", C.c_uint32), ("shut_approx", C.c_uint8), ("reserved", C.c_uint8), ("lower_band_th", C.c_uint16), ("upper_band_th", C.c_uint16),
                ("reserved2", C.c_uint16), ("n_mvs", C.c_uint32), ("jobs", C.c_void_p), ("mv_array", C.c_void_p), ("models", C.c_void_p), ("status", C.c_void_p)]


WM_START_FROM_ARRAY = 1
WM_MAX_ITERATIONS = 16
WM_NO_COST = 0x7FFFFFFF  # best_cost when no position had a valid fit (INT_MAX)


class WmRefineJob(C.Structure):  # SvtHipWmRefineJob
    _fields_ = [("pts", C.c_int32 * 16), ("pts_inref", C.c_int32 * 16), ("src_offset", C.c_uint32), ("blk_org_x", C.c_uint16), ("blk_org_y", C.c_uint16),
                ("bwidth", C.c_uint8), ("bheight", C.c_uint8), ("n_samples", C.c_uint8), ("flags", C.c_uint8), ("start_mv", C.c_int16 * 2),
                ("pred_mv", C.c_int16 * 2), ("mv_index", C.c_uint32), ("ref", C.c_uint8), ("reserved", C.c_uint8 * 7)]


class WmRefineDesc(C.Structure):  # SvtHipWmRefineDesc
    _fields_ = [("n_jobs", C.c_uint32), ("iterations", C.c_uint8), ("refine_diag", C.c_uint8), ("mv_prec_shift", C.c_uint8), ("shut_approx", C.c_uint8),
                ("lower_band_th", C.c_uint16), ("upper_band_th", C.c_uint16), ("approx_inter_rate", C.c_uint8), ("n_refs", C.c_uint8),
                ("waves_per_job", C.c_uint8), ("reserved", C.c_uint8), ("error_per_bit", C.c_int32), ("src_stride", C.c_uint32), ("src", C.c_void_p),
                ("src_samples", C.c_uint64), ("refs", WarpRef * WARP_MAX_REFS), ("jobs", C.c_void_p), ("mv_array", C.c_void_p), ("n_mvs", C.c_uint32),
                ("reserved2", C.c_uint32), ("mvjcost", C.c_void_p), ("mvcost", C.c_void_p * 2), ("best_mv", C.c_void_p), ("best_cost", C.c_void_p),
                ("n_checked", C.c_void_p), ("status", C.c_void_p)]


WM_REFINE_JOB_DTYPE = [("pts", "<i4", (16,)), ("pts_inref", "<i4", (16,)), ("src_offset", "<u4"), ("blk_org_x", "<u2"), ("blk_org_y", "<u2"), ("bwidth", "u1"),
                       ("bheight", "u1"), ("n_samples", "u1"), ("flags", "u1"), ("start_mv", "<i2", (2,)), ("pred_mv", "<i2", (2,)), ("mv_index", "<u4"),
                       ("ref", "u1"), ("reserved", "u1", (7,))]
WARP_MODEL_DTYPE = [("wmmat", "<i4", (6,)), ("alpha", "<i2"), ("beta", "<i2"), ("gamma", "<i2"), ("delta", "<i2"), ("wmtype", "u1"), ("valid", "u1"),
                    ("num_samples", "<u2"), ("reserved", "<u4")]
WARP_PRED_JOB_DTYPE = [("dst_offset", "<u4"), ("p_col", "<i2"), ("p_row", "<i2"), ("width", "u1"), ("height", "u1"), ("ref", "u1", (2,)), ("flags", "u1"),
                       ("comp_mode", "u1"), ("fwd_offset", "u1"), ("bck_offset", "u1"), ("model_index", "<u4", (2,)), ("model", WARP_MODEL_DTYPE, (2,))]
WARP_MODEL_JOB_DTYPE = [("pts", "<i4", (16,)), ("pts_inref", "<i4", (16,)), ("blk_org_x", "<u2"), ("blk_org_y", "<u2"), ("bwidth", "u1"), ("bheight", "u1"),
                        ("n_samples", "u1"), ("flags", "u1"), ("mv", "<i2", (2,)), ("mv_index", "<u4")]


# ---- include/svt_hip_mask.h ----
MASK_WEDGE, MASK_DIFFWTD = 0, 1
MASK_PARAMS_FROM_ARRAY = 4
MASK_OK, MASK_UNDEFINED = 0, 0xFF
MASK_SEARCH_WEDGE, MASK_SEARCH_DIFFWTD, MASK_SEARCH_INTERINTRA = 0, 1, 2
MASK_NO_RD = 0x7FFFFFFFFFFFFFFF  # rd_wedge when no wedge search ran (INT64_MAX)


class MaskSearchResult(C.Structure):  # SvtHipMaskSearchResult
    _fields_ = [("best_rd", C.c_int64), ("rd_wedge", C.c_int64), ("wedge_index", C.c_int8), ("wedge_sign", C.c_uint8), ("mask_type", C.c_uint8),
                ("interintra_mode", C.c_uint8), ("use_wedge_interintra", C.c_uint8), ("exit", C.c_uint8), ("reserved", C.c_uint8 * 2)]


class MaskedPredJob(C.Structure):  # SvtHipMaskedPredJob
    _fields_ = [("pred", InterPredJob), ("comp_type", C.c_uint8), ("wedge_index", C.c_uint8), ("wedge_sign", C.c_uint8), ("mask_type", C.c_uint8),
                ("luma_width", C.c_uint8), ("luma_height", C.c_uint8), ("reserved", C.c_uint8 * 2), ("mask_offset", C.c_uint32), ("result_index", C.c_uint32)]


class MaskedPredDesc(C.Structure):  # SvtHipMaskedPredDesc
    _fields_ = [("bit_depth", C.c_uint8), ("ss_x", C.c_uint8), ("ss_y", C.c_uint8), ("n_refs", C.c_uint8), ("n_jobs", C.c_uint32),
                ("refs", InterPredRef * INTER_PRED_MAX_REFS), ("dst", C.c_void_p), ("dst_stride", C.c_uint32), ("plane", C.c_uint8), ("reserved", C.c_uint8 * 3),
                ("dst_samples", C.c_uint64), ("jobs", C.c_void_p), ("mv_array", C.c_void_p), ("n_mvs", C.c_uint32), ("n_results", C.c_uint32),
                ("results", C.c_void_p), ("mask_buf", C.c_void_p), ("mask_bytes", C.c_uint64), ("status", C.c_void_p)]


class InterIntraJob(C.Structure):  # SvtHipInterIntraJob
    _fields_ = [("intra_offset", C.c_uint32 * 4), ("inter_offset", C.c_uint32), ("dst_offset", C.c_uint32), ("result_index", C.c_uint32), ("width", C.c_uint8),
                ("height", C.c_uint8), ("luma_width", C.c_uint8), ("luma_height", C.c_uint8), ("interintra_mode", C.c_uint8), ("use_wedge", C.c_uint8),
                ("wedge_index", C.c_uint8), ("wedge_sign", C.c_uint8), ("flags", C.c_uint8), ("reserved", C.c_uint8 * 3)]


class InterIntraDesc(C.Structure):  # SvtHipInterIntraDesc
    _fields_ = [("bit_depth", C.c_uint8), ("reserved", C.c_uint8 * 3), ("n_jobs", C.c_uint32), ("intra", C.c_void_p), ("inter", C.c_void_p), ("dst", C.c_void_p),
                ("intra_stride", C.c_uint32), ("inter_stride", C.c_uint32), ("dst_stride", C.c_uint32), ("n_results", C.c_uint32),
                ("intra_samples", C.c_uint64), ("inter_samples", C.c_uint64), ("dst_samples", C.c_uint64), ("jobs", C.c_void_p), ("results", C.c_void_p),
                ("status", C.c_void_p)]


class MaskSearchJob(C.Structure):  # SvtHipMaskSearchJob
    _fields_ = [("src_offset", C.c_uint32), ("pred0_offset", C.c_uint32), ("pred1_offset", C.c_uint32), ("intra_offset", C.c_uint32 * 4), ("width", C.c_uint8),
                ("height", C.c_uint8), ("kind", C.c_uint8), ("ii_wedge_mode", C.c_uint8)]


class MaskSearchDesc(C.Structure):  # SvtHipMaskSearchDesc
    _fields_ = [("bit_depth", C.c_uint8), ("pred0_to_pred1_mult", C.c_uint8), ("use_rate", C.c_uint8), ("use_rd_model", C.c_uint8), ("n_jobs", C.c_uint32),
                ("src", C.c_void_p), ("pred0", C.c_void_p), ("pred1", C.c_void_p), ("intra", C.c_void_p), ("src_stride", C.c_uint32),
                ("pred0_stride", C.c_uint32), ("pred1_stride", C.c_uint32), ("intra_stride", C.c_uint32), ("src_samples", C.c_uint64),
                ("pred0_samples", C.c_uint64), ("pred1_samples", C.c_uint64), ("intra_samples", C.c_uint64), ("jobs", C.c_void_p), ("results", C.c_void_p),
                ("status", C.c_void_p)]


MASK_SEARCH_RESULT_DTYPE = [("best_rd", "<i8"), ("rd_wedge", "<i8"), ("wedge_index", "i1"), ("wedge_sign", "u1"), ("mask_type", "u1"), ("interintra_mode", "u1"),
                            ("use_wedge_interintra", "u1"), ("exit", "u1"), ("reserved", "u1", (2,))]
MASKED_PRED_JOB_DTYPE = [("pred", INTER_PRED_JOB_DTYPE), ("comp_type", "u1"), ("wedge_index", "u1"), ("wedge_sign", "u1"), ("mask_type", "u1"), ("luma_width", "u1"),
                         ("luma_height", "u1"), ("reserved", "u1", (2,)), ("mask_offset", "<u4"), ("result_index", "<u4")]
INTERINTRA_JOB_DTYPE = [("intra_offset", "<u4", (4,)), ("inter_offset", "<u4"), ("dst_offset", "<u4"), ("result_index", "<u4"), ("width", "u1"), ("height", "u1"),
                        ("luma_width", "u1"), ("luma_height", "u1"), ("interintra_mode", "u1"), ("use_wedge", "u1"), ("wedge_index", "u1"), ("wedge_sign", "u1"),
                        ("flags", "u1"), ("reserved", "u1", (3,))]
MASK_SEARCH_JOB_DTYPE = [("src_offset", "<u4"), ("pred0_offset", "<u4"), ("pred1_offset", "<u4"), ("intra_offset", "<u4", (4,)), ("width", "u1"), ("height", "u1"),
                         ("kind", "u1"), ("ii_wedge_mode", "u1")]


# ---- include/svt_hip_obmc.h ----
OBMC_MAX_NEIGHBOURS = 4
OBMC_MV_FROM_ARRAY = 1
OBMC_OK, OBMC_UNDEFINED = 0, 0xFF


class ObmcNeighbour(C.Structure):  # SvtHipObmcNeighbour
    _fields_ = [("rel_pos", C.c_uint8), ("size", C.c_uint8), ("ref", C.c_uint8), ("filter_x", C.c_uint8), ("filter_y", C.c_uint8), ("flags", C.c_uint8),
                ("mv", C.c_int16 * 2), ("reserved", C.c_uint16), ("mv_index", C.c_uint32)]


class ObmcBlock(C.Structure):  # SvtHipObmcBlock
    _fields_ = [("org_x", C.c_int16), ("org_y", C.c_int16), ("width", C.c_uint8), ("height", C.c_uint8), ("n_above", C.c_uint8), ("n_left", C.c_uint8),
                ("mb_to_left_edge", C.c_int32), ("mb_to_right_edge", C.c_int32), ("mb_to_top_edge", C.c_int32), ("mb_to_bottom_edge", C.c_int32),
                ("strip_offset", C.c_uint32), ("reserved", C.c_uint32), ("above", ObmcNeighbour * OBMC_MAX_NEIGHBOURS), ("left", ObmcNeighbour * OBMC_MAX_NEIGHBOURS)]


class ObmcJob(C.Structure):  # SvtHipObmcJob
    _fields_ = [("block", C.c_uint32), ("offset", C.c_uint32)]


class ObmcNeighbourDesc(C.Structure):  # SvtHipObmcNeighbourDesc
    _fields_ = [("bit_depth", C.c_uint8), ("ss_x", C.c_uint8), ("ss_y", C.c_uint8), ("plane", C.c_uint8), ("n_refs", C.c_uint8), ("reserved", C.c_uint8 * 3),
                ("n_jobs", C.c_uint32), ("n_blocks", C.c_uint32), ("refs", InterPredRef * INTER_PRED_MAX_REFS), ("blocks", C.c_void_p), ("jobs", C.c_void_p),
                ("above", C.c_void_p), ("left", C.c_void_p), ("strip_samples", C.c_uint64), ("mv_array", C.c_void_p), ("n_mvs", C.c_uint32),
                ("reserved2", C.c_uint32), ("status", C.c_void_p)]


class ObmcBlendDesc(C.Structure):  # SvtHipObmcBlendDesc
    _fields_ = [("bit_depth", C.c_uint8), ("ss_x", C.c_uint8), ("ss_y", C.c_uint8), ("plane", C.c_uint8), ("n_jobs", C.c_uint32), ("n_blocks", C.c_uint32),
                ("dst_stride", C.c_uint32), ("blocks", C.c_void_p), ("jobs", C.c_void_p), ("above", C.c_void_p), ("left", C.c_void_p),
                ("strip_samples", C.c_uint64), ("dst", C.c_void_p), ("dst_samples", C.c_uint64), ("status", C.c_void_p)]


class ObmcTargetDesc(C.Structure):  # SvtHipObmcTargetDesc
    _fields_ = [("strip_bit_depth", C.c_uint8), ("reserved", C.c_uint8 * 3), ("n_jobs", C.c_uint32), ("n_blocks", C.c_uint32), ("src_stride", C.c_uint32),
                ("blocks", C.c_void_p), ("jobs", C.c_void_p), ("above", C.c_void_p), ("left", C.c_void_p), ("strip_samples", C.c_uint64), ("src", C.c_void_p),
                ("src_samples", C.c_uint64), ("wsrc", C.c_void_p), ("mask", C.c_void_p), ("out_values", C.c_uint64), ("status", C.c_void_p)]


OBMC_NEIGHBOUR_DTYPE = [("rel_pos", "u1"), ("size", "u1"), ("ref", "u1"), ("filter_x", "u1"), ("filter_y", "u1"), ("flags", "u1"), ("mv", "<i2", (2,)),
                        ("reserved", "<u2"), ("mv_index", "<u4")]
OBMC_BLOCK_DTYPE = [("org_x", "<i2"), ("org_y", "<i2"), ("width", "u1"), ("height", "u1"), ("n_above", "u1"), ("n_left", "u1"), ("mb_to_left_edge", "<i4"),
                    ("mb_to_right_edge", "<i4"), ("mb_to_top_edge", "<i4"), ("mb_to_bottom_edge", "<i4"), ("strip_offset", "<u4"), ("reserved", "<u4"),
                    ("above", OBMC_NEIGHBOUR_DTYPE, (OBMC_MAX_NEIGHBOURS,)), ("left", OBMC_NEIGHBOUR_DTYPE, (OBMC_MAX_NEIGHBOURS,))]
OBMC_JOB_DTYPE = [("block", "<u4"), ("offset", "<u4")]
OBMC_MAX_FPEL_RANGE = 64


class ObmcSearchJob(C.Structure):  # SvtHipObmcSearchJob
    _fields_ = [("target_offset", C.c_uint32), ("ref_offset", C.c_uint32), ("width", C.c_uint8), ("height", C.c_uint8), ("reserved", C.c_uint8 * 2),
                ("start_mv", Mv), ("ref_mv", Mv), ("col_min", C.c_int32), ("col_max", C.c_int32), ("row_min", C.c_int32), ("row_max", C.c_int32),
                ("reserved2", C.c_uint32)]


class ObmcSearchResult(C.Structure):  # SvtHipObmcSearchResult
    _fields_ = [("fullpel_value", C.c_int32), ("besterr", C.c_uint32), ("distortion", C.c_int32), ("sse1", C.c_uint32), ("rate_mv", C.c_int32),
                ("reserved", C.c_uint32)]


class ObmcSearchDesc(C.Structure):  # SvtHipObmcSearchDesc
    _fields_ = [("ref_bit_depth", C.c_uint8), ("refine_level", C.c_uint8), ("fpel_search_diag", C.c_uint8), ("approx_inter_rate", C.c_uint8), ("allow_hp", C.c_uint8),
                ("reserved", C.c_uint8 * 3), ("n_jobs", C.c_uint32), ("fpel_search_range", C.c_uint32), ("sadpb", C.c_int32), ("error_per_bit", C.c_int32),
                ("ref_stride", C.c_uint32), ("reserved2", C.c_uint32), ("ref", C.c_void_p), ("ref_samples", C.c_uint64), ("wsrc", C.c_void_p), ("mask", C.c_void_p),
                ("target_values", C.c_uint64), ("mvjcost", C.c_void_p), ("mvcost", C.c_void_p * 2), ("jobs", C.c_void_p), ("best_mv", C.c_void_p),
                ("results", C.c_void_p), ("status", C.c_void_p)]


OBMC_SEARCH_JOB_DTYPE = [("target_offset", "<u4"), ("ref_offset", "<u4"), ("width", "u1"), ("height", "u1"), ("reserved", "u1", (2,)), ("start_mv", "<i2", (2,)),
                         ("ref_mv", "<i2", (2,)), ("col_min", "<i4"), ("col_max", "<i4"), ("row_min", "<i4"), ("row_max", "<i4"), ("reserved2", "<u4")]
OBMC_SEARCH_RESULT_DTYPE = [("fullpel_value", "<i4"), ("besterr", "<u4"), ("distortion", "<i4"), ("sse1", "<u4"), ("rate_mv", "<i4"), ("reserved", "<u4")]


# ---- include/svt_hip_ifs.h ----
IFS_PAIRS = 9
IFS_CONTEXTS = 16
IFS_MODEL_ENTRIES = 104
IFS_OK, IFS_UNDEFINED = 0, 0xFF
IFS_SKIPPED = 0xFFFFFFFFFFFFFFFF  # rd / sse of a pair the search skipped


class IfsJob(C.Structure):  # SvtHipIfsJob
    _fields_ = [("pred", InterPredJob), ("src_offset", C.c_uint32), ("pred_ctx", C.c_uint8 * 2), ("reserved", C.c_uint8 * 2)]


class IfsResult(C.Structure):  # SvtHipIfsResult
    _fields_ = [("best_rd", C.c_uint64), ("interp_filters", C.c_uint32), ("switchable_rate", C.c_int32), ("filter_x", C.c_uint8), ("filter_y", C.c_uint8),
                ("winner", C.c_uint8), ("reserved", C.c_uint8 * 5)]


class IfsDesc(C.Structure):  # SvtHipIfsDesc
    _fields_ = [("bit_depth", C.c_uint8), ("n_refs", C.c_uint8), ("enable_dual_filter", C.c_uint8), ("subsampled_distortion", C.c_uint8),
                ("skip_sse_rd_model", C.c_uint8), ("spy_rd", C.c_uint8), ("reserved", C.c_uint8 * 2), ("n_jobs", C.c_uint32), ("n_mvs", C.c_uint32),
                ("refs", InterPredRef * INTER_PRED_MAX_REFS), ("src", C.c_void_p), ("src_stride", C.c_uint32), ("dst_stride", C.c_uint32),
                ("src_samples", C.c_uint64), ("dst", C.c_void_p), ("dst_samples", C.c_uint64), ("jobs", C.c_void_p), ("mv_array", C.c_void_p),
                ("quantizer", C.c_int32), ("lambda_", C.c_uint32), ("smooth_bias_pct", C.c_uint32), ("reserved2", C.c_uint32), ("psy_rd", C.c_double),
                ("switchable_interp_fac_bits", C.c_void_p), ("results", C.c_void_p), ("rd", C.c_void_p), ("sse", C.c_void_p), ("status", C.c_void_p)]


class IfsPatch(C.Structure):  # SvtHipIfsPatch
    _fields_ = [("result_index", C.c_uint32), ("record_index", C.c_uint32)]


class IfsScatterDesc(C.Structure):  # SvtHipIfsScatterDesc
    _fields_ = [("n_patches", C.c_uint32), ("n_results", C.c_uint32), ("n_records", C.c_uint32), ("record_stride", C.c_uint32), ("filter_x_offset", C.c_uint32),
                ("reserved", C.c_uint32), ("patches", C.c_void_p), ("results", C.c_void_p), ("result_status", C.c_void_p), ("base", C.c_void_p),
                ("status", C.c_void_p)]


IFS_JOB_DTYPE = [("pred", INTER_PRED_JOB_DTYPE), ("src_offset", "<u4"), ("pred_ctx", "u1", (2,)), ("reserved", "u1", (2,))]
IFS_RESULT_DTYPE = [("best_rd", "<u8"), ("interp_filters", "<u4"), ("switchable_rate", "<i4"), ("filter_x", "u1"), ("filter_y", "u1"), ("winner", "u1"),
                    ("reserved", "u1", (5,))]
IFS_PATCH_DTYPE = [("result_index", "<u4"), ("record_index", "<u4")]


# ---- include/svt_hip_palette.h ----
PALETTE_MAX_CANDS = 14
PALETTE_MAX_SIZE = 8
PALETTE_MAX_CACHE = 16
PALETTE_BSIZE_CTXS = 7
PALETTE_MODE_CTXS = 3
PALETTE_OK, PALETTE_UNDEFINED = 0, 0xFF


class PaletteJob(C.Structure):  # SvtHipPaletteJob
    _fields_ = [("src_offset", C.c_uint32), ("map_offset", C.c_uint32), ("width", C.c_uint8), ("height", C.c_uint8), ("rows", C.c_uint8), ("cols", C.c_uint8),
                ("n_cache", C.c_uint8), ("bsize_ctx", C.c_uint8), ("mode_ctx", C.c_uint8), ("reserved", C.c_uint8), ("color_cache", C.c_uint16 * PALETTE_MAX_CACHE)]


class PaletteCand(C.Structure):  # SvtHipPaletteCand
    _fields_ = [("size", C.c_uint8), ("first_index", C.c_uint8), ("colors", C.c_uint16 * PALETTE_MAX_SIZE), ("top_over", C.c_uint8), ("reserved", C.c_uint8),
                ("color_cost", C.c_int32), ("map_cost", C.c_int32), ("index0_cost", C.c_int32), ("size_cost", C.c_int32), ("rate", C.c_int32)]


class PaletteResult(C.Structure):  # SvtHipPaletteResult
    _fields_ = [("n_colors", C.c_uint32), ("n_cands", C.c_uint32), ("cands", PaletteCand * PALETTE_MAX_CANDS)]


class PaletteDesc(C.Structure):  # SvtHipPaletteDesc
    _fields_ = [("bit_depth", C.c_uint8), ("cost_bit_depth", C.c_uint8), ("dominant_color_step", C.c_uint8), ("reduce_palette_cost_precision", C.c_uint8),
                ("n_jobs", C.c_uint32), ("src", C.c_void_p), ("src_stride", C.c_uint32), ("reserved", C.c_uint32), ("src_samples", C.c_uint64),
                ("palette_ycolor_fac_bitss", C.c_void_p), ("palette_ysize_fac_bits", C.c_void_p), ("palette_ymode_fac_bits", C.c_void_p), ("jobs", C.c_void_p),
                ("results", C.c_void_p), ("status", C.c_void_p), ("color_maps", C.c_void_p), ("map_bytes", C.c_uint64)]


class PalettePredJob(C.Structure):  # SvtHipPalettePredJob
    _fields_ = [("search_index", C.c_uint32), ("cand_index", C.c_uint32), ("dst_offset", C.c_uint32), ("map_offset", C.c_uint32)]


class PalettePredDesc(C.Structure):  # SvtHipPalettePredDesc
    _fields_ = [("bit_depth", C.c_uint8), ("reserved", C.c_uint8 * 3), ("n_jobs", C.c_uint32), ("n_search_jobs", C.c_uint32), ("src_stride", C.c_uint32),
                ("src", C.c_void_p), ("src_samples", C.c_uint64), ("dst", C.c_void_p), ("dst_stride", C.c_uint32), ("reserved2", C.c_uint32),
                ("dst_samples", C.c_uint64), ("search_jobs", C.c_void_p), ("search_results", C.c_void_p), ("search_status", C.c_void_p), ("jobs", C.c_void_p),
                ("status", C.c_void_p), ("color_map", C.c_void_p), ("map_bytes", C.c_uint64)]


PALETTE_JOB_DTYPE = [("src_offset", "<u4"), ("map_offset", "<u4"), ("width", "u1"), ("height", "u1"), ("rows", "u1"), ("cols", "u1"), ("n_cache", "u1"),
                     ("bsize_ctx", "u1"), ("mode_ctx", "u1"), ("reserved", "u1"), ("color_cache", "<u2", (PALETTE_MAX_CACHE,))]
PALETTE_CAND_DTYPE = [("size", "u1"), ("first_index", "u1"), ("colors", "<u2", (PALETTE_MAX_SIZE,)), ("top_over", "u1"), ("reserved", "u1"), ("color_cost", "<i4"),
                      ("map_cost", "<i4"), ("index0_cost", "<i4"), ("size_cost", "<i4"), ("rate", "<i4")]
PALETTE_RESULT_DTYPE = [("n_colors", "<u4"), ("n_cands", "<u4"), ("cands", PALETTE_CAND_DTYPE, (PALETTE_MAX_CANDS,))]
PALETTE_PRED_JOB_DTYPE = [("search_index", "<u4"), ("cand_index", "<u4"), ("dst_offset", "<u4"), ("map_offset", "<u4")]


# ---- include/svt_hip_gm.h ----
GM_OK, GM_IDENTICAL, GM_UNDEFINED = 0, 1, 0xFF
GM_IDENTITY, GM_TRANSLATION, GM_ROTZOOM, GM_AFFINE = 0, 1, 2, 3  # TransformationType
GM_MAX_REFINEMENTS = 5
GM_ROUND_ERRORS = 61
GM_MAX_PAIRS = 8
GM_MAX_JOBS = 65535
GM_NO_FRAME_ERROR = 0x7FFFFFFFFFFFFFFF  # best_frame_error as the reference passes it (INT64_MAX)


class GmRefineJob(C.Structure):  # SvtHipGmRefineJob
    _fields_ = [("wmmat", C.c_int32 * 6), ("params_cost", C.c_int32), ("ref", C.c_uint8), ("wmtype", C.c_uint8), ("reserved", C.c_uint8 * 2),
                ("best_frame_error", C.c_int64)]


class GmRefineDesc(C.Structure):  # SvtHipGmRefineDesc
    _fields_ = [("n_jobs", C.c_uint32), ("n_refs", C.c_uint8), ("n_refinements", C.c_uint8), ("chess_refn", C.c_uint8), ("rfn_early_exit", C.c_uint8),
                ("src", WarpRef), ("refs", WarpRef * WARP_MAX_REFS), ("jobs", C.c_void_p), ("work", C.c_void_p), ("models", C.c_void_p),
                ("best_error", C.c_void_p), ("pic_sad", C.c_void_p), ("status", C.c_void_p), ("round_error", C.c_void_p)]


class GmPair(C.Structure):  # SvtHipGmPair
    _fields_ = [("list", C.c_uint8), ("ref", C.c_uint8), ("reserved", C.c_uint8 * 2)]


class GmCorrDesc(C.Structure):  # SvtHipGmCorrDesc
    _fields_ = [("aligned_width", C.c_uint16), ("aligned_height", C.c_uint16), ("enable_me_8x8", C.c_uint8), ("enable_me_16x16", C.c_uint8),
                ("max_cand", C.c_uint8), ("max_refs", C.c_uint8), ("max_l0", C.c_uint8), ("n_pu", C.c_uint8), ("method", C.c_uint8), ("shift", C.c_uint8),
                ("n_pairs", C.c_uint32), ("cap", C.c_uint32), ("pairs", GmPair * GM_MAX_PAIRS), ("me", MeResults), ("corr", C.c_void_p), ("count", C.c_void_p),
                ("sums", C.c_void_p)]


GM_REFINE_JOB_DTYPE = [("wmmat", "<i4", (6,)), ("params_cost", "<i4"), ("ref", "u1"), ("wmtype", "u1"), ("reserved", "u1", (2,)), ("best_frame_error", "<i8")]
