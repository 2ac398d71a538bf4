#!/usr/bin/env python3
"""Writes tests/golden/palette.npz: the reference encoder's own luma palette search, palette rate and palette prediction on the cases of
tests/palette_cases.py.

Run by hand on a machine that has the reference's sources (--ref: the root of its source tree); never by the tests, build(), smoke() or bench.py.
It compiles a harness of its own into a temporary directory outside the tree (gcc, -O2, -DNDEBUG as a release build of the encoder has it: the case
with a 10-bit sample out of range is one the reference only asserts against).  The harness #includes Codec/palette.c where it lies,
because palette_rd_y, optimize_palette_colors, av1_remove_duplicates and extend_palette_color_map are static, and links Codec/entropy_coding.c
(svt_aom_write_uniform_cost, svt_aom_get_palette_bsize_ctx, svt_aom_get_palette_mode_ctx), Codec/pic_analysis_process.c (svt_av1_count_colors and
svt_av1_count_colors_highbd), Codec/mode_decision.c (svt_av1_allow_palette), Codec/enc_intra_prediction.c (the palette prediction), Codec/utility.c (svt_aom_log2f_32), Codec/cabac_context_model.c
(svt_aom_get_palette_color_index_context_optimized) and the two rtcd
files where they lie, with the _c k-means installed in the rtcd pointers.  Whatever else the link still wants gets a stand-in that aborts.

Per job the harness scripts a PictureControlSet, a ModeDecisionContext and a MacroBlockD: a source picture whose origin is the block's first sample,
the block's size and the two edges that crop it, the palette controls, the encoder bit depth, the rate tables, and an above and a left MbModeInfo
holding the scripted neighbours' palettes, so that svt_get_palette_cache_y and svt_aom_get_palette_mode_ctx work out the cache and the context
themselves.  It then
  1  calls svt_av1_count_colors / svt_av1_count_colors_highbd for the colour count,
  2  calls search_palette_luma for the candidates,
  3  for each candidate kept calls svt_av1_palette_color_cost_y, svt_av1_cost_color_map and svt_aom_write_uniform_cost and adds them up as
     Codec/rd_cost.c:679-706 does,
  4  and calls svt_av1_predict_intra_block / _16bit with use_palette for the candidate's samples.
The cache, the two contexts and the cropped dimensions the reference works out are compared with the job's fields, which the host fills.

The fixture holds numbers only.  --check recomputes everything and compares it with the committed file instead of writing it; either way the
restatement of tests/palette_cases.py is compared with the reference on every output of every job, the set of block sizes is compared with
svt_av1_allow_palette, the conditions of the case list are asserted -- the k-means restore among them, which must never fire -- and the most
candidates the reference keeps is reported."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import palette_cases as pc  # noqa: E402
import refbuild  # noqa: E402

HARNESS = r"""
#include "palette.c"
#include <stdlib.h>
#include <string.h>
#include "sequence_control_set.h"
#include "pcs.h"
#include "md_process.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"
#include "utility.h"
#include "md_rate_estimation.h"

int  svt_av1_allow_palette(int allow_palette, BlockSize bsize);
int  svt_aom_get_palette_bsize_ctx(BlockSize bsize);
int  svt_aom_get_palette_mode_ctx(const MacroBlockD *xd);
int  svt_aom_write_uniform_cost(int n, int v);
void svt_av1_predict_intra_block(STAGE stage, const BlockGeom *blk_geom, MacroBlockD *xd, int32_t wpx, int32_t hpx, TxSize tx_size, PredictionMode mode,
                                 int32_t angle_delta, int32_t use_palette, PaletteInfo *palette_info, FilterIntraMode filter_intra_mode,
                                 uint8_t *top_neigh_array, uint8_t *left_neigh_array, EbPictureBufferDesc *recon_buffer, int32_t col_off, int32_t row_off,
                                 int32_t plane, BlockSize bsize, uint32_t txb_org_x_pict, uint32_t txb_org_y_pict, uint32_t bl_org_x_pict,
                                 uint32_t bl_org_y_pict, uint32_t bl_org_x_mb, uint32_t bl_org_y_mb, SeqHeader *seq_header_ptr);
void svt_av1_predict_intra_block_16bit(EbBitDepth bit_depth, STAGE stage, const BlockGeom *blk_geom, MacroBlockD *xd, int32_t wpx, int32_t hpx,
                                       TxSize tx_size, PredictionMode mode, int32_t angle_delta, int32_t use_palette, PaletteInfo *palette_info,
                                       FilterIntraMode filter_intra_mode, uint16_t *top_neigh_array, uint16_t *left_neigh_array,
                                       EbPictureBufferDesc *recon_buffer, int32_t col_off, int32_t row_off, int32_t plane, BlockSize bsize,
                                       uint32_t txb_org_x_pict, uint32_t txb_org_y_pict, uint32_t bl_org_x_pict, uint32_t bl_org_y_pict,
                                       uint32_t bl_org_x_mb, uint32_t bl_org_y_mb, SeqHeader *seq_header_ptr);

static BlockSize bsize_of(int w, int h) {
    for (int b = 0; b < BlockSizeS_ALL; b++)
        if (block_size_wide[b] == w && block_size_high[b] == h) return (BlockSize)b;
    return BLOCK_INVALID;
}
static void plain_memcpy(void *dst, void const *src, size_t size) { memcpy(dst, src, size); }

int harness_init(void) {
    svt_memcpy = plain_memcpy;
    svt_log2f = svt_aom_log2f_32; /* av1_ceil_log2 */
    svt_av1_k_means_dim1 = svt_av1_k_means_dim1_c; svt_av1_calc_indices_dim1 = svt_av1_calc_indices_dim1_c;
    svt_av1_k_means_dim2 = svt_av1_k_means_dim2_c; svt_av1_calc_indices_dim2 = svt_av1_calc_indices_dim2_c;
    return 0;
}

/* every block size for which svt_av1_allow_palette is true: out[2 * i] = width, out[2 * i + 1] = height; returns their number */
int harness_allowed(int *out) {
    int n = 0;
    for (int b = 0; b < BlockSizeS_ALL; b++)
        if (svt_av1_allow_palette(1, (BlockSize)b)) { out[2 * n] = block_size_wide[b]; out[2 * n + 1] = block_size_high[b]; n++; }
    return n;
}

/* p: 0 bit depth of the planes, 1 encoder_bit_depth, 2 width, 3 height, 4 rows, 5 cols, 6 dominant_color_step, 7 reduce_palette_cost_precision,
 *    8 size of the above palette (-1: no above block), 9 of the left one
 * hdr: 0 colours, 1 candidates, 2 n_cache, 3 bsize_ctx, 4 mode_ctx, 5 rows, 6 cols, 7.. the cache
 * cands: [14][16] = size, first index, color_cost, map_cost, index0_cost, size_cost, rate, -, colours[8]
 * maps: [14][width * height] bytes; preds: [14][width * height] samples of the planes' type */
int harness_palette(const int *p, uint8_t *src, int src_stride, const int32_t *ycolor, const int32_t *ysize, const int32_t *ymode, const uint16_t *above,
                    const uint16_t *left, int32_t *hdr, int32_t *cands, uint8_t *maps, uint8_t *preds) {
    const int bd = p[0], is16 = bd > 8, w = p[2], h = p[3];
    const BlockSize bsize = bsize_of(w, h);
    SequenceControlSet      *scs  = (SequenceControlSet *)calloc(1, sizeof(*scs));
    PictureControlSet       *pcs  = (PictureControlSet *)calloc(1, sizeof(*pcs));
    PictureParentControlSet *ppcs = (PictureParentControlSet *)calloc(1, sizeof(*ppcs));
    ModeDecisionContext     *ctx  = (ModeDecisionContext *)calloc(1, sizeof(*ctx));
    MdRateEstimationContext *rate = (MdRateEstimationContext *)calloc(1, sizeof(*rate));
    BlkStruct               *blk  = (BlkStruct *)calloc(1, sizeof(*blk));
    EbPictureBufferDesc     *pic  = (EbPictureBufferDesc *)calloc(2, sizeof(*pic)); /* the source, the prediction */
    MbModeInfo              *nbr  = (MbModeInfo *)calloc(2, sizeof(*nbr));
    PALETTE_BUFFER          *pbuf = (PALETTE_BUFFER *)calloc(1, sizeof(*pbuf));
    ModeDecisionCandidate   *cand = (ModeDecisionCandidate *)calloc(1, sizeof(*cand));
    uint8_t                 *pred = (uint8_t *)calloc((size_t)w * h, 2);
    PaletteInfo              pal[MAX_PAL_CAND];
    uint8_t                  sizes[MAX_PAL_CAND];
    uint32_t                 tot = 0;
    MacroBlockD              xd;
    BlockGeom                geo_s, *geo = &geo_s;
    if (!scs || !pcs || !ppcs || !ctx || !rate || !blk || !pic || !nbr || !pbuf || !cand || !pred) return 2;
    if (bsize == BLOCK_INVALID) return 3;
    if (sizeof(rate->palette_ycolor_fac_bitss) != 7 * 5 * 8 * 4 || sizeof(rate->palette_ysize_fac_bits) != 7 * 8 * 4 || sizeof(rate->palette_ymode_fac_bits) != 7 * 3 * 3 * 4)
        return 4;
    memset(&xd, 0, sizeof(xd));
    memset(geo, 0, sizeof(*geo));
    memset(pal, 0, sizeof(pal));
    memset(sizes, 0, sizeof(sizes));
    for (int i = 0; i < MAX_PAL_CAND; i++)
        if (!(pal[i].color_idx_map = (uint8_t *)calloc(MAX_PALETTE_SQUARE, 1))) return 2;
    scs->encoder_bit_depth = (uint32_t)p[1];
    pcs->scs = scs; pcs->ppcs = ppcs; ppcs->scs = scs;
    ppcs->palette_ctrls.dominant_color_step = (uint8_t)p[6]; ppcs->palette_ctrls.reduce_palette_cost_precision = (uint8_t)p[7];
    pic[0].buffer_y = src; pic[0].stride_y = (uint16_t)src_stride; /* its (org_x, org_y) = (0, 0) is the block's first sample */
    ppcs->enhanced_pic = &pic[0]; pcs->input_frame16bit = &pic[0];
    pic[1].buffer_y = pred; pic[1].stride_y = (uint16_t)w; pic[1].width = (uint16_t)w; pic[1].height = (uint16_t)h;
    geo->bsize = bsize; geo->bwidth = (uint8_t)w; geo->bheight = (uint8_t)h;
    ctx->blk_geom = geo; ctx->blk_ptr = blk; blk->av1xd = &xd;
    ctx->blk_org_x = 0; ctx->blk_org_y = 0;
    ctx->hbd_md = (uint8_t)is16; ctx->palette_buffer = pbuf; ctx->md_rate_est_ctx = rate;
    memcpy(rate->palette_ycolor_fac_bitss, ycolor, sizeof(rate->palette_ycolor_fac_bitss));
    memcpy(rate->palette_ysize_fac_bits, ysize, sizeof(rate->palette_ysize_fac_bits));
    memcpy(rate->palette_ymode_fac_bits, ymode, sizeof(rate->palette_ymode_fac_bits));
    xd.mb_to_top_edge = -8 * 8; xd.mb_to_left_edge = -8 * 8; /* row 8 of the picture: the above block is in the same SB row */
    xd.mb_to_bottom_edge = (p[4] - h) * 8; xd.mb_to_right_edge = (p[5] - w) * 8;
    xd.bsize = bsize;
    for (int k = 0; k < 2; k++) {
        const int n = p[8 + k];
        const uint16_t *c = k ? left : above;
        if (n < 0) continue;
        nbr[k].palette_mode_info.palette_size = (uint8_t)n;
        for (int i = 0; i < n; i++) nbr[k].palette_mode_info.palette_colors[i] = c[i];
        if (k) xd.left_mbmi = &nbr[k]; else xd.above_mbmi = &nbr[k];
    }

    int *count = (int *)calloc(1 << 12, sizeof(int));
    if (!count) return 2;
    hdr[0] = is16 ? svt_av1_count_colors_highbd((uint16_t *)src, src_stride, p[4], p[5], p[1], count) : svt_av1_count_colors(src, src_stride, p[4], p[5], count);
    free(count);
    search_palette_luma(pcs, ctx, pal, sizes, &tot);
    if (tot > MAX_PAL_CAND) return 5;
    hdr[1] = (int32_t)tot;
    uint16_t  cache[2 * PALETTE_MAX_SIZE];
    const int n_cache = svt_get_palette_cache_y(&xd, cache);
    hdr[2] = n_cache;
    for (int i = 0; i < n_cache; i++) hdr[7 + i] = cache[i];
    const int bsize_ctx = svt_aom_get_palette_bsize_ctx(bsize), mode_ctx = svt_aom_get_palette_mode_ctx(&xd);
    hdr[3] = bsize_ctx; hdr[4] = mode_ctx;
    int bw, bh, rows, cols;
    svt_aom_get_block_dimensions(bsize, 0, &xd, &bw, &bh, &rows, &cols);
    if (bw != w || bh != h) return 6;
    hdr[5] = rows; hdr[6] = cols;
    TxSize tx = TX_INVALID;
    for (int t = 0; t < TX_SIZES_ALL; t++)
        if (tx_size_wide[t] == w && tx_size_high[t] == h) tx = (TxSize)t;
    if (tx == TX_INVALID) return 7;
    for (uint32_t i = 0; i < tot; i++) {
        int32_t *o = cands + 16 * i;
        const int size = sizes[i];
        const uint8_t *map = pal[i].color_idx_map;
        cand->palette_info = &pal[i]; cand->palette_size[0] = (uint8_t)size; cand->palette_size[1] = 0;
        /* Codec/rd_cost.c:684-704 */
        int mode_bits = rate->palette_ymode_fac_bits[bsize_ctx][mode_ctx][1];
        const int size_cost = rate->palette_ysize_fac_bits[bsize_ctx][size - PALETTE_MIN_SIZE];
        const int index0_cost = svt_aom_write_uniform_cost(size, map[0]);
        int palette_mode_cost = size_cost + index0_cost;
        const int color_cost = svt_av1_palette_color_cost_y(&pal[i].pmi, cache, size, n_cache, (int)scs->encoder_bit_depth);
        palette_mode_cost += color_cost;
        int map_cost = 0;
        if (!ppcs->palette_ctrls.reduce_palette_cost_precision) {
            map_cost = svt_av1_cost_color_map(cand, rate, blk, 0, bsize, PALETTE_MAP);
            palette_mode_cost += map_cost;
        }
        o[0] = size; o[1] = map[0]; o[2] = color_cost; o[3] = map_cost; o[4] = index0_cost; o[5] = size_cost; o[6] = mode_bits + palette_mode_cost; o[7] = 0;
        for (int q = 0; q < PALETTE_MAX_SIZE; q++) o[8 + q] = q < size ? pal[i].pmi.palette_colors[q] : 0;
        memcpy(maps + (size_t)i * w * h, map, (size_t)w * h);
        memset(pred, 0, (size_t)w * h * 2);
        if (is16)
            svt_av1_predict_intra_block_16bit((EbBitDepth)bd, 0, geo, &xd, w, h, tx, DC_PRED, 0, 1, &pal[i], FILTER_INTRA_MODES, NULL, NULL, &pic[1], 0, 0, 0, bsize, 0, 0,
                                              0, 0, 0, 0, &scs->seq_header);
        else
            svt_av1_predict_intra_block(0, geo, &xd, w, h, tx, DC_PRED, 0, 1, &pal[i], FILTER_INTRA_MODES, NULL, NULL, &pic[1], 0, 0, 0, bsize, 0, 0, 0, 0, 0, 0,
                                        &scs->seq_header);
        memcpy(preds + ((size_t)i * w * h << is16), pred, (size_t)w * h << is16);
    }
    for (int i = 0; i < MAX_PAL_CAND; i++) free(pal[i].color_idx_map);
    free(scs); free(pcs); free(ppcs); free(ctx); free(rate); free(blk); free(pic); free(nbr); free(pbuf); free(cand); free(pred);
    return 0;
}
"""

SOURCES = ["Codec/entropy_coding.c", "Codec/pic_analysis_process.c", "Codec/mode_decision.c", "Codec/enc_intra_prediction.c", "Codec/utility.c", "Codec/cabac_context_model.c",
           "Codec/aom_dsp_rtcd.c", "Codec/common_dsp_rtcd.c"]


def build(ref, tmp):
    """Symbols the link still wants get stand-ins: the SIMD bodies the rtcd files name and what the rest of the compiled sources calls."""
    # -DNDEBUG: svt_av1_count_colors_highbd asserts that every sample fits the bit depth, and the cases hold samples above it on purpose
    L = refbuild.build(ref, tmp, "paletteref", SOURCES, [("harness", HARNESS)], flags=["-DNDEBUG"], standins=True)
    P = C.c_void_p
    L.harness_palette.argtypes = [P, P, C.c_int, P, P, P, P, P, P, P, P, P]
    L.harness_allowed.argtypes = [P]
    if L.harness_init():
        raise RuntimeError("harness_init failed")
    return L


def reference_batch(L, name):
    """the reference's results of a batch, laid out as palette_cases.restated()'s"""
    b = pc.batch(name)
    bd, prm, t = b["bit_depth"], b["params"], b["tables"]
    dt = np.uint16 if bd > 8 else np.uint8
    src = np.ascontiguousarray(b["src"])
    tabs = [np.ascontiguousarray(t[k], np.int32) for k in ("ycolor", "ysize", "ymode")]
    res = []
    for i, (job, (above, left)) in enumerate(zip(b["jobs"], b["nbrs"])):
        w, h, rows, cols = (int(job[k]) for k in ("width", "height", "rows", "cols"))
        p = np.array([bd, prm["cost_bit_depth"], w, h, rows, cols, prm["dominant_color_step"], prm["reduce_palette_cost_precision"],
                      -1 if above is None else len(above), -1 if left is None else len(left)], np.int32)
        nb = [np.array(list(v or []) + [0] * 8, np.uint16)[:8].copy() for v in (above, left)]
        hdr, cands = np.zeros(7 + 16, np.int32), np.zeros((pc.MAX_CANDS, 16), np.int32)
        maps, preds = np.zeros((pc.MAX_CANDS, h, w), np.uint8), np.zeros((pc.MAX_CANDS, h, w), dt)
        rc = L.harness_palette(p.ctypes.data, src.ctypes.data + int(job["src_offset"]) * src.itemsize, src.shape[1], tabs[0].ctypes.data, tabs[1].ctypes.data,
                               tabs[2].ctypes.data, nb[0].ctypes.data, nb[1].ctypes.data, hdr.ctypes.data, cands.ctypes.data, maps.ctypes.data, preds.ctypes.data)
        if rc:
            raise RuntimeError(f"{name} job {i}: the harness returned {rc}")
        # what the host fills is what the reference works out
        host = (int(job["n_cache"]), int(job["bsize_ctx"]), int(job["mode_ctx"]), rows, cols)
        if tuple(int(v) for v in hdr[2:7]) != host or [int(v) for v in hdr[7:7 + hdr[2]]] != pc.job_cache(job):
            raise RuntimeError(f"{name} job {i}: cache / contexts / dimensions {hdr[2:].tolist()} of the reference, {host} {pc.job_cache(job)} in the job")
        r = {"n_colors": int(hdr[0]), "n_cands": int(hdr[1]), "cands": []}
        for q in range(r["n_cands"]):
            o = cands[q]
            c = {"size": int(o[0]), "first_index": int(o[1]), "colors": [int(v) for v in o[8:8 + o[0]]], "map": maps[q].copy(), "pred": preds[q].astype(np.uint16)}
            c.update({k: int(o[2 + n]) for n, k in enumerate(pc.COSTS)})
            r["cands"].append(c)
        res.append(r)
    return res


def generate(L):
    sizes = np.zeros(64, np.int32)
    n = L.harness_allowed(sizes.ctypes.data)
    allowed = sorted((int(sizes[2 * i]), int(sizes[2 * i + 1])) for i in range(n))
    if allowed != sorted(pc.SIZES):
        raise RuntimeError(f"svt_av1_allow_palette allows {allowed}, the case list has {sorted(pc.SIZES)}")
    out, mismatch, n_jobs, most = {}, [], 0, 0
    for name in pc.batch_names():
        ref, want = reference_batch(L, name), pc.restated(name)
        got, mine = pc.fixture_arrays(name, ref), pc.fixture_arrays(name, want)
        for k in got:
            if not (got[k].dtype == mine[k].dtype and np.array_equal(got[k], mine[k])):
                mismatch.append((k, np.argwhere(got[k] != mine[k])[:4].tolist() if got[k].shape == mine[k].shape else "shape"))
        out.update(got)
        n_jobs += len(ref)
        most = max(most, max(r["n_cands"] for r in ref))
    if mismatch:
        raise RuntimeError(f"the restatement differs from the reference in {len(mismatch)} arrays, first: {mismatch[:8]}")
    missing = pc.coverage_missing()
    if missing:
        raise RuntimeError(f"conditions of the case list that are not met: {missing[:10]}")
    print(f"{n_jobs} jobs in {len(pc.batch_names())} batches: colour counts, candidates, colours, first indices, rate terms, maps and predictions of the "
          f"restatement equal to the reference's on all of them; the reference keeps at most {most} candidates; the k-means restore never fired")
    return out


if __name__ == "__main__":
    refbuild.main(__doc__, build, {pc.GOLDEN: generate})
