"""A descriptor that its check accepts, for every asynchronous batch entry that runs through csrc/batch_host.h: the prediction families (inter, intra, CfL,
warp, masked compound / inter-intra, OBMC, the interpolation-filter search, palette) in ENTRIES, and the older ones (RD, the transforms alone, the MD
searches, PME, statistics, SSIM, rate, RDOQ) in OLDER.  The pointers are never dereferenced: the validations read the descriptor alone, so these serve the
CPU tests of the refusals (tests/test_<family>.py) and of the entries' common contract (tests/test_batch_entries.py)."""
from svt_av1_psyex_amd import abi, cfl, warp

P = 0x1000
Q = 0x100000  # the families whose validation compares address ranges need room between their planes


def good_inter_pred_desc(n_refs=2):
    d = abi.InterPredDesc(bit_depth=10, ss_x=1, ss_y=1, n_refs=n_refs, n_jobs=4, dst=P, dst_stride=256, dst_samples=256 * 64, jobs=P, status=P)
    for i in range(min(n_refs, abi.INTER_PRED_MAX_REFS)):
        d.refs[i] = abi.InterPredRef(plane=P, stride=512, org_x=160, org_y=160, width=512, height=448)
    return d


def good_intra_pred_desc(bd=10):
    return abi.IntraPredDesc(bit_depth=bd, disable_edge_filter=0, n_jobs=4, nbr=Q, nbr_stride=256, nbr_width=208, nbr_height=144, dst=Q + 0x100000,
                             dst_stride=256, dst_samples=256 * 64, jobs=Q, status=Q)


def good_cfl_pred_desc(bd=10, n_alpha=33):
    planes = [dict(dc=Q + 0x100000 * (1 + q), dc_stride=128, dc_samples=128 * 72, dst=Q + 0x1000000 * (1 + q), dst_stride=128, dst_samples=33 * 128 * 72)
              for q in range(2)]
    return cfl.pred_desc(bd, 8, 16, list(range(-16, 17))[:n_alpha], Q, 256, 208, 144, planes, 128 * 72, Q, 4, Q, Q + 8)


def good_cfl_pick_desc():
    return abi.CflPickDesc(n_blocks=3, lambda_=41000, itr_th=1, n_mag=16, dist_stride=1, bits=Q, dist=Q, mode_bits=Q, alpha_fac_bits=Q, best_rd=Q, cfl_alpha_idx=Q,
                           cfl_alpha_signs=Q, status=Q)


def good_warp_pred_desc(bd=10, n_refs=2):
    refs = [abi.WarpRef(plane=Q + 0x100000 * r, stride=160, org_x=16, org_y=8, width=128, height=96, rows=112) for r in range(n_refs)]
    return warp.pred_desc(bd, 0, 0, refs, Q * 64, 128, 128 * 128, Q * 65, 5, Q * 66, Q * 67, 4)


def good_warp_model_desc():
    return abi.WarpModelDesc(n_jobs=3, n_mvs=2, jobs=Q, mv_array=Q, models=Q, status=Q)


def good_wm_refine_desc(light=0):
    refs = [abi.WarpRef(plane=Q, stride=160, org_x=16, org_y=8, width=128, height=96, rows=112)]
    settings = dict(iterations=8, refine_diag=1, mv_prec_shift=1, shut_approx=0, lower_band_th=0, upper_band_th=65535, approx_inter_rate=light, error_per_bit=90)
    outs = dict(best_mv=Q * 3, best_cost=Q * 4, n_checked=Q * 5, status=Q * 6)
    return warp.refine_desc(4, settings, refs, Q * 2, 128, 128 * 96, Q * 7, outs, Q * 8, 4, None if light else (Q * 9, Q * 10, Q * 11))


def good_masked_pred_desc(plane=1):
    d = abi.MaskedPredDesc(bit_depth=10, ss_x=plane and 1, ss_y=plane and 1, n_refs=2, n_jobs=4, dst=P, dst_stride=256, plane=plane, dst_samples=256 * 64, jobs=P,
                           status=P, mask_buf=P, mask_bytes=4096)
    for i in range(2):
        d.refs[i] = abi.InterPredRef(plane=P, stride=512, org_x=160, org_y=160, width=512, height=448)
    return d


def good_interintra_blend_desc():
    return abi.InterIntraDesc(bit_depth=8, n_jobs=3, intra=P, inter=P, dst=P, intra_stride=64, inter_stride=72, dst_stride=72, intra_samples=4096,
                              inter_samples=4608, dst_samples=4608, jobs=P, status=P)


def good_mask_search_desc():
    return abi.MaskSearchDesc(bit_depth=10, pred0_to_pred1_mult=4, n_jobs=3, src=P, pred0=P, pred1=P, intra=P, src_stride=64, pred0_stride=64, pred1_stride=64,
                              intra_stride=64, src_samples=4096, pred0_samples=4096, pred1_samples=4096, intra_samples=4096, jobs=P, results=P, status=P)


def good_obmc_neighbour_desc(plane=1):
    d = abi.ObmcNeighbourDesc(bit_depth=10, ss_x=plane and 1, ss_y=plane and 1, plane=plane, n_refs=2, n_jobs=4, n_blocks=4, blocks=P, jobs=P, above=P, left=P,
                              strip_samples=4096, status=P)
    for i in range(2):
        d.refs[i] = abi.InterPredRef(plane=P, stride=256, org_x=80, org_y=80, width=256, height=224)
    return d


def good_obmc_blend_desc(plane=2):
    return abi.ObmcBlendDesc(bit_depth=8, ss_x=plane and 1, ss_y=plane and 1, plane=plane, n_jobs=3, n_blocks=3, dst_stride=96, blocks=P, jobs=P, above=P, left=P,
                             strip_samples=4096, dst=P, dst_samples=96 * 64, status=P)


def good_obmc_target_desc():
    return abi.ObmcTargetDesc(strip_bit_depth=10, n_jobs=3, n_blocks=3, src_stride=192, blocks=P, jobs=P, above=P, left=P, strip_samples=4096, src=P,
                              src_samples=192 * 128, wsrc=P, mask=P, out_values=4096, status=P)


def good_obmc_search_desc(light=0):
    d = abi.ObmcSearchDesc(ref_bit_depth=8, refine_level=3, fpel_search_diag=1, approx_inter_rate=light, allow_hp=1, n_jobs=4, fpel_search_range=16, sadpb=40,
                           error_per_bit=60, ref_stride=384, ref=P, ref_samples=384 * 320, wsrc=P, mask=P, target_values=4096, jobs=P, best_mv=P, results=P, status=P)
    if not light:
        d.mvjcost, d.mvcost[0], d.mvcost[1] = P, P, P
    return d


def good_ifs_desc():
    d = abi.IfsDesc(bit_depth=8, n_refs=2, n_jobs=1, n_mvs=2, src=64, src_stride=256, dst_stride=256, src_samples=4096, dst=64, dst_samples=4096, jobs=64,
                    mv_array=64, quantizer=400, lambda_=3000, smooth_bias_pct=130, psy_rd=1.0, switchable_interp_fac_bits=64, results=64, rd=64, sse=64, status=64)
    for i in range(2):
        d.refs[i] = abi.InterPredRef(plane=64, stride=512, org_x=160, org_y=160, width=512, height=448)
    return d


def good_ifs_scatter_desc():
    return abi.IfsScatterDesc(n_patches=1, n_results=1, n_records=1, record_stride=8, filter_x_offset=6, patches=64, results=64, result_status=64, base=64, status=64)


def good_palette_desc():
    return abi.PaletteDesc(bit_depth=8, cost_bit_depth=10, dominant_color_step=2, reduce_palette_cost_precision=1, n_jobs=1, src=64, src_stride=256,
                           src_samples=4096, palette_ycolor_fac_bitss=64, palette_ysize_fac_bits=64, palette_ymode_fac_bits=64, jobs=64, results=64, status=64,
                           color_maps=64, map_bytes=4096)


def good_palette_pred_desc():
    return abi.PalettePredDesc(bit_depth=10, n_jobs=1, n_search_jobs=1, src_stride=256, src=64, src_samples=4096, dst=64, dst_stride=64, dst_samples=4096,
                               search_jobs=64, search_results=64, search_status=64, jobs=64, status=64, color_map=64, map_bytes=4096)


def good_rd_desc():
    return abi.RdBatchDesc(bit_depth=10, quant_kind=0, tx_size=2, n_jobs=4, src_stride=256, pred_stride=256, src=P, pred=P, jobs=P, quant_rows=P, n_quant_rows=1,
                           eob=P, satd=P, dist_coeff=P, three_quad_energy=P, sse=P)


def good_inv_txfm_desc():
    return abi.InvTxBatchDesc(bit_depth=10, sample_bytes=2, tx_size=2, n_jobs=4, pred_stride=256, recon_stride=256, pred=P, recon=P, jobs=P, dqcoeff=P)


def good_fwd_txfm_desc():
    return abi.FwdTxBatchDesc(tx_size=2, n_jobs=4, residual_stride=256, residual=P, jobs=P, coeff=P)


MV_COST_NONE = 5  # SVT_HIP_MV_COST_NONE: no cost table is mandatory


def good_md_fullpel_desc():
    return abi.FullpelBatchDesc(n_jobs=4, src_stride=256, ref_stride=512, src=P, ref=P, ref_max_width=512, ref_max_height=448, jobs=P, mv_cost_type=MV_COST_NONE,
                                best_cost=P, best_mv=P)


def good_md_subpel_desc():
    return abi.SubpelBatchDesc(n_jobs=4, src_stride=256, ref_stride=512, src=P, ref=P, jobs=P, forced_stop=0, iters_per_step=2, search_method=0,
                               mv_cost_type=MV_COST_NONE, best_mv=P, besterr=P, distortion=P, sse=P)


def good_pme_desc():
    return abi.PmeBatchDesc(n_jobs=4, src_stride=256, ref_stride=512, src=P, ref=P, jobs=P, mv_cost_type=MV_COST_NONE, best_cost=P, best_mv=P)


def good_block_stats_desc():
    return abi.BlockStatsDesc(bit_depth=8, n_jobs=4, src_stride=256, ref_stride=256, src=P, ref=P, jobs=P, sad=P, n_pyramids=1, pyramids=P)


def good_ssim_desc(n_pyramids=1):
    return abi.SsimBatchDesc(bit_depth=8, n_jobs=4, src_stride=64, ref_stride=64, src=P, ref=P, jobs=P, ssim=P, ssim_dist=P, n_pyramids=n_pyramids,
                             pyramids=P if n_pyramids else None)


def good_coeff_rate_desc(n_groups=2):
    d = abi.CoeffRateDesc(tx_size=2, plane_type=0, coeff_rate_est_lvl=1, mds_fast_coeff_est_level=1, n_jobs=4, jobs=P, tables=P, qcoeff=P, eob=P, bits=P)
    if n_groups:
        d.n_groups, d.lambda_, d.dist, d.rd_cost, d.group_start, d.best_job, d.best_cost = n_groups, 100, P, P, P, P, P
    return d


def good_rdoq_desc():
    return abi.RdoqDesc(tx_size=2, plane_type=0, eob_th=255, eob_fast_th=255, n_jobs=4, lambda_=100, jobs=P, tables=P, quant_rows=P, n_quant_rows=1,
                        coeff=P, qcoeff=P, dqcoeff=P, eob=P)


# (the entry, a descriptor it accepts, the member whose zero means "nothing to do")
ENTRIES = [("svt_hip_inter_pred_batch", good_inter_pred_desc, "n_jobs"),
           ("svt_hip_intra_pred_batch", good_intra_pred_desc, "n_jobs"),
           ("svt_hip_cfl_pred_batch", good_cfl_pred_desc, "n_jobs"),
           ("svt_hip_cfl_pick_alpha_batch", good_cfl_pick_desc, "n_blocks"),
           ("svt_hip_warp_pred_batch", good_warp_pred_desc, "n_jobs"),
           ("svt_hip_warp_model_batch", good_warp_model_desc, "n_jobs"),
           ("svt_hip_wm_refine_batch", good_wm_refine_desc, "n_jobs"),
           ("svt_hip_masked_pred_batch", good_masked_pred_desc, "n_jobs"),
           ("svt_hip_interintra_blend_batch", good_interintra_blend_desc, "n_jobs"),
           ("svt_hip_mask_search_batch", good_mask_search_desc, "n_jobs"),
           ("svt_hip_obmc_neighbour_batch", good_obmc_neighbour_desc, "n_jobs"),
           ("svt_hip_obmc_blend_batch", good_obmc_blend_desc, "n_jobs"),
           ("svt_hip_obmc_target_batch", good_obmc_target_desc, "n_jobs"),
           ("svt_hip_obmc_search_batch", good_obmc_search_desc, "n_jobs"),
           ("svt_hip_ifs_batch", good_ifs_desc, "n_jobs"),
           ("svt_hip_ifs_scatter_filters", good_ifs_scatter_desc, "n_patches"),
           ("svt_hip_palette_search_batch", good_palette_desc, "n_jobs"),
           ("svt_hip_palette_pred_batch", good_palette_pred_desc, "n_jobs")]

# The older entries that run through the same sequence.  Their checks keep the order each had against "nothing to do":
EMPTY_FIRST = "an empty batch is accepted whatever else the descriptor holds"
BIT_DEPTH_THEN_EMPTY = "bit_depth is looked at, then an empty batch is accepted, then the rest"
CHECK_FIRST = "everything is checked, then an empty batch is accepted"
# (the entry, a descriptor it accepts, the members that are all zero when there is nothing to do, a mandatory pointer, the order)
OLDER = [("svt_hip_rd_batch", good_rd_desc, ("n_jobs",), "src", EMPTY_FIRST),
         ("svt_hip_inv_txfm_batch", good_inv_txfm_desc, ("n_jobs",), "dqcoeff", EMPTY_FIRST),
         ("svt_hip_fwd_txfm_batch", good_fwd_txfm_desc, ("n_jobs",), "coeff", EMPTY_FIRST),
         ("svt_hip_md_fullpel_batch", good_md_fullpel_desc, ("n_jobs",), "best_mv", EMPTY_FIRST),
         ("svt_hip_md_subpel_batch", good_md_subpel_desc, ("n_jobs",), "besterr", EMPTY_FIRST),
         ("svt_hip_pme_sad_batch", good_pme_desc, ("n_jobs",), "best_cost", EMPTY_FIRST),
         ("svt_hip_block_stats_batch", good_block_stats_desc, ("n_jobs", "n_pyramids"), "ref", EMPTY_FIRST),
         ("svt_hip_ssim_batch", good_ssim_desc, ("n_jobs", "n_pyramids"), "src", BIT_DEPTH_THEN_EMPTY),
         ("svt_hip_coeff_rate_batch", good_coeff_rate_desc, ("n_jobs", "n_groups"), "tables", CHECK_FIRST),
         ("svt_hip_rdoq_batch", good_rdoq_desc, ("n_jobs",), "quant_rows", CHECK_FIRST)]
