#!/usr/bin/env python3
"""Writes tests/golden/cdef.npz: the reference encoder's own cdef_seg_search, finish_cdef_search and svt_av1_cdef_frame on the cases of
tests/cdef_cases.py.

Run by hand on a machine that has the reference's sources (--ref: the root of its source tree); never by the tests, build(), smoke() or bench.py.
It compiles a harness of its own into a temporary directory outside the tree.  The harness #includes Codec/cdef_process.c where it lies, because
cdef_seg_search is static, and links Codec/cdef.c, Codec/enc_cdef.c and the two rtcd files with the _c kernels stored in the rtcd pointers.  It
defines svt_aom_get_recon_pic (the scripted picture) and svt_aom_av1_lambda_assignment_function_table (a scripted lambda) itself; whatever else the
link still wants gets a stand-in that aborts.

Per case the harness scripts a PictureControlSet: the planes in padded buffers, a mode-info grid whose skip flags say what the masks say, the
strength lists as the first pass's, the controls.  A search case runs the three functions in the encoder's order; a pick case runs
finish_cdef_search on a scripted mse_seg; an apply case runs svt_av1_cdef_frame with scripted strengths and use_reference_cdef_fs set, which makes
it compute the directions itself.  The reference's chroma strength is the luma strength of the same index (its _uv list only switches an index
off), so the cases' chroma lists are that.

The fixture holds numbers only; pictures come from seeds.  The two costs of the pick are locals of finish_cdef_search and are not in the fixture.
--check recomputes everything and compares it with the committed file instead of writing it.  Either way the restatement of tests/cdef_cases.py is
compared with the reference on every output of every case, and the conditions of the case list are asserted: they are read off the restatement's
run, whose every output is the reference's.  --time reports the reference's C time on a 3840x2160 picture."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import cdef_cases as cc  # noqa: E402
import refbuild  # noqa: E402

HARNESS = r"""
#include "cdef_process.c"
#include <string.h>
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"
#include "md_process.h"

static EbPictureBufferDesc g_recon;
static uint32_t            g_lambda;
void svt_aom_get_recon_pic(PictureControlSet *pcs, EbPictureBufferDesc **recon_ptr, bool is_highbd) { (void)pcs; (void)is_highbd; *recon_ptr = &g_recon; }
static void harness_lambda(PictureControlSet *pcs, uint32_t *fast_lambda, uint32_t *full_lambda, uint8_t bit_depth, uint16_t qp_index, bool multiply_lambda) {
    (void)pcs; (void)bit_depth; (void)qp_index; (void)multiply_lambda;
    *fast_lambda = g_lambda; *full_lambda = g_lambda;
}
const EbAv1LambdaAssignFunc svt_aom_av1_lambda_assignment_function_table[4] = {harness_lambda, harness_lambda, harness_lambda, harness_lambda};
static void harness_memcpy(void *dst, void const *src, size_t size) { memcpy(dst, src, size); }

uint8_t  svt_aom_cdef_find_dir_c(const uint16_t *img, int32_t stride, int32_t *var, int32_t coeff_shift);
void     svt_aom_cdef_find_dir_dual_c(const uint16_t *img1, const uint16_t *img2, int stride, int32_t *var1, int32_t *var2, int32_t coeff_shift, uint8_t *out1, uint8_t *out2);

int harness_init(void) {
    svt_cdef_filter_block            = svt_cdef_filter_block_c;
    svt_aom_cdef_find_dir            = svt_aom_cdef_find_dir_c;
    svt_aom_cdef_find_dir_dual       = svt_aom_cdef_find_dir_dual_c;
    svt_aom_copy_rect8_8bit_to_16bit = svt_aom_copy_rect8_8bit_to_16bit_c;
    svt_compute_cdef_dist_16bit      = svt_aom_compute_cdef_dist_c;
    svt_compute_cdef_dist_8bit       = svt_aom_compute_cdef_dist_8bit_c;
    svt_search_one_dual              = svt_search_one_dual_c;
    svt_memcpy                       = harness_memcpy;
    return 0;
}

#define PAD 32
/* p: 0 width, 1 height, 2 bit depth, 3 base_q_idx, 4 subsampling_factor, 5 n_strengths, 6 zero_fs_cost_bias, 7 full_lambda, 8 stages (1 search, 2 pick,
 *    4 apply), 9 cdef_damping of an apply on its own
 * planes: the three reconstruction planes and the three source planes, tightly packed; masks [n_fb]
 * mse [2][n_fb][64]: out of the search, in and out (biased) of a pick on its own; dir [n_fb][64], var [n_fb][64]: as the reference leaves them
 * hdr: 0 cdef_bits, 1 nb_cdef_strengths, 2..9 cdef_y_strength, 10..17 cdef_uv_strength, 18 cdef_dist_dev, 19 cdef_damping: out of the pick, in of an apply on its own
 * fb_strength [n_fb]: mbmi.cdef_strength of the filter block's first mode info: out of the pick, in of an apply on its own
 * out: the three filtered planes, tightly packed */
int harness_run(const int *p, const uint8_t *strengths, const int8_t *strengths_uv, const uint64_t *masks, void *const *planes, uint64_t *mse, uint8_t *dir,
                int32_t *var, int32_t *hdr, int8_t *fb_strength, void *const *out) {
    const int w = p[0], h = p[1], hbd = p[2] > 8, n = p[5], stages = p[8], bytes = hbd ? 2 : 1;
    const int mi_cols = w / 4, mi_rows = h / 4, nhfb = (w + 63) / 64, nvfb = (h + 63) / 64, n_fb = nhfb * nvfb;
    PictureControlSet       *pcs = (PictureControlSet *)calloc(1, sizeof(*pcs));
    PictureParentControlSet *ppcs = (PictureParentControlSet *)calloc(1, sizeof(*ppcs));
    SequenceControlSet      *scs = (SequenceControlSet *)calloc(1, sizeof(*scs));
    Av1Common               *cm = (Av1Common *)calloc(1, sizeof(*cm));
    EbPictureBufferDesc     *input = (EbPictureBufferDesc *)calloc(1, sizeof(*input));
    ModeInfo                *mi = (ModeInfo *)calloc((size_t)mi_cols * mi_rows, sizeof(*mi));
    ModeInfo               **grid = (ModeInfo **)calloc((size_t)mi_cols * mi_rows, sizeof(*grid));
    if (!pcs || !ppcs || !scs || !cm || !input || !mi || !grid) return -2;
    pcs->ppcs = ppcs; pcs->scs = scs; ppcs->scs = scs; ppcs->av1_cm = cm;
    cm->mi_rows = mi_rows; cm->mi_cols = mi_cols; cm->mi_stride = mi_cols;
    pcs->mi_stride = mi_cols; pcs->mi_grid_base = grid;
    ppcs->aligned_width = (uint16_t)w; ppcs->aligned_height = (uint16_t)h;
    pcs->cdef_segments_column_count = 1; pcs->cdef_segments_row_count = 1;
    scs->is_16bit_pipeline = hbd; scs->static_config.encoder_bit_depth = (uint32_t)p[2]; scs->super_block_size = 64;
    ppcs->frm_hdr.quantization_params.base_q_idx = (uint8_t)p[3];
    ppcs->enhanced_pic = input; pcs->input_frame16bit = input; input->bit_depth = hbd ? EB_TEN_BIT : EB_EIGHT_BIT;
    ppcs->cdef_search_ctrls.first_pass_fs_num = (uint8_t)n; ppcs->cdef_search_ctrls.default_second_pass_fs_num = 0;
    ppcs->cdef_search_ctrls.subsampling_factor = (uint8_t)p[4];
    for (int i = 0; i < n; i++) { ppcs->cdef_search_ctrls.default_first_pass_fs[i] = strengths[i]; ppcs->cdef_search_ctrls.default_first_pass_fs_uv[i] = strengths_uv[i]; }
    ppcs->cdef_recon_ctrls.zero_fs_cost_bias = (uint16_t)p[6];
    g_lambda = (uint32_t)p[7];
    for (int r = 0; r < mi_rows; r++)
        for (int c = 0; c < mi_cols; c++) {
            ModeInfo *m = &mi[(size_t)r * mi_cols + c];
            const int fb = (r / 16) * nhfb + c / 16, bit = ((r % 16) / 2) * 8 + (c % 16) / 2;
            m->mbmi.block_mi.skip = !((masks[fb] >> bit) & 1);
            m->mbmi.block_mi.bsize = BLOCK_64X64;
            m->mbmi.cdef_strength = 0;
            grid[(size_t)r * mi_cols + c] = m;
        }
    /* the planes in padded buffers: the reference reads up to 8 columns past a narrow last filter block */
    uint8_t *rec[3], *src[3];
    int      stride[3];
    for (int pl = 0; pl < 3; pl++) {
        const int pw = pl ? w / 2 : w, ph = pl ? h / 2 : h, pad = pl ? PAD / 2 : PAD;
        stride[pl] = pw + 2 * pad;
        rec[pl] = (uint8_t *)malloc((size_t)stride[pl] * (ph + 2 * pad) * bytes);
        src[pl] = (uint8_t *)malloc((size_t)stride[pl] * (ph + 2 * pad) * bytes);
        if (!rec[pl] || !src[pl]) return -2;
        memset(rec[pl], 0x33, (size_t)stride[pl] * (ph + 2 * pad) * bytes);
        memset(src[pl], 0x44, (size_t)stride[pl] * (ph + 2 * pad) * bytes);
        for (int y = 0; y < ph; y++) {
            memcpy(rec[pl] + ((size_t)(y + pad) * stride[pl] + pad) * bytes, (const uint8_t *)planes[pl] + (size_t)y * pw * bytes, (size_t)pw * bytes);
            memcpy(src[pl] + ((size_t)(y + pad) * stride[pl] + pad) * bytes, (const uint8_t *)planes[3 + pl] + (size_t)y * pw * bytes, (size_t)pw * bytes);
        }
        pcs->cdef_input_recon[pl]  = rec[pl] + ((size_t)pad * stride[pl] + pad) * bytes;
        pcs->cdef_input_source[pl] = src[pl] + ((size_t)pad * stride[pl] + pad) * bytes;
    }
    memset(&g_recon, 0, sizeof(g_recon));
    g_recon.org_x = PAD; g_recon.org_y = PAD;
    g_recon.stride_y = (uint16_t)stride[0]; g_recon.stride_cb = (uint16_t)stride[1]; g_recon.stride_cr = (uint16_t)stride[2];
    g_recon.buffer_y = rec[0]; g_recon.buffer_cb = rec[1]; g_recon.buffer_cr = rec[2];
    input->stride_y = (uint16_t)stride[0]; input->stride_cb = (uint16_t)stride[1]; input->stride_cr = (uint16_t)stride[2];
    pcs->mse_seg[0] = (uint64_t(*)[TOTAL_STRENGTHS])calloc((size_t)n_fb, sizeof(uint64_t[TOTAL_STRENGTHS]));
    pcs->mse_seg[1] = (uint64_t(*)[TOTAL_STRENGTHS])calloc((size_t)n_fb, sizeof(uint64_t[TOTAL_STRENGTHS]));
    pcs->skip_cdef_seg = (uint8_t *)calloc((size_t)n_fb, 1);
    pcs->cdef_dir_data = (CdefDirData *)calloc((size_t)n_fb, sizeof(CdefDirData));
    if (!pcs->mse_seg[0] || !pcs->mse_seg[1] || !pcs->skip_cdef_seg || !pcs->cdef_dir_data) return -2;

    if (stages & 1) {
        cdef_seg_search(pcs, scs, 0);
        memcpy(mse, pcs->mse_seg[0], (size_t)n_fb * 64 * 8);
        memcpy(mse + (size_t)n_fb * 64, pcs->mse_seg[1], (size_t)n_fb * 64 * 8);
        for (int fb = 0; fb < n_fb; fb++) {
            for (int b = 0; b < 64; b++) { /* the reference's arrays are CDEF_NBLOCKS wide */
                dir[(size_t)fb * 64 + b] = pcs->cdef_dir_data[fb].dir[b >> 3][b & 7];
                var[(size_t)fb * 64 + b] = pcs->cdef_dir_data[fb].var[b >> 3][b & 7];
            }
        }
    } else {
        memcpy(pcs->mse_seg[0], mse, (size_t)n_fb * 64 * 8);
        memcpy(pcs->mse_seg[1], mse + (size_t)n_fb * 64, (size_t)n_fb * 64 * 8);
        for (int fb = 0; fb < n_fb; fb++) pcs->skip_cdef_seg[fb] = masks[fb] == 0;
    }
    if (stages & 2) {
        finish_cdef_search(pcs);
        hdr[0] = ppcs->frm_hdr.cdef_params.cdef_bits; hdr[1] = ppcs->nb_cdef_strengths;
        for (int i = 0; i < 8; i++) {
            hdr[2 + i]  = i < ppcs->nb_cdef_strengths ? ppcs->frm_hdr.cdef_params.cdef_y_strength[i] : 0;
            hdr[10 + i] = i < ppcs->nb_cdef_strengths ? ppcs->frm_hdr.cdef_params.cdef_uv_strength[i] : 0;
        }
        hdr[18] = pcs->cdef_dist_dev; hdr[19] = ppcs->frm_hdr.cdef_params.cdef_damping;
        for (int fb = 0; fb < n_fb; fb++)
            if (!pcs->skip_cdef_seg[fb]) fb_strength[fb] = grid[(size_t)(fb / nhfb) * 16 * mi_cols + (fb % nhfb) * 16]->mbmi.cdef_strength;
        for (int fb = 0; fb < n_fb; fb++) { mse[(size_t)fb * 64] = pcs->mse_seg[0][fb][0]; mse[((size_t)n_fb + fb) * 64] = pcs->mse_seg[1][fb][0]; }
    } else if (stages & 4) {
        ppcs->cdef_search_ctrls.use_reference_cdef_fs = 1; /* svt_av1_cdef_frame computes the directions itself */
        ppcs->frm_hdr.cdef_params.cdef_damping = (uint8_t)p[9];
        for (int i = 0; i < 8; i++) { ppcs->frm_hdr.cdef_params.cdef_y_strength[i] = hdr[2 + i]; ppcs->frm_hdr.cdef_params.cdef_uv_strength[i] = hdr[10 + i]; }
        for (int fb = 0; fb < n_fb; fb++) grid[(size_t)(fb / nhfb) * 16 * mi_cols + (fb % nhfb) * 16]->mbmi.cdef_strength = fb_strength[fb];
    }
    if (stages & 4) {
        svt_av1_cdef_frame(scs, pcs);
        for (int pl = 0; pl < 3; pl++) {
            const int pw = pl ? w / 2 : w, ph = pl ? h / 2 : h, pad = pl ? PAD / 2 : PAD;
            for (int y = 0; y < ph; y++)
                memcpy((uint8_t *)out[pl] + (size_t)y * pw * bytes, rec[pl] + ((size_t)(y + pad) * stride[pl] + pad) * bytes, (size_t)pw * bytes);
        }
    }
    for (int pl = 0; pl < 3; pl++) { free(rec[pl]); free(src[pl]); }
    free(pcs->mse_seg[0]); free(pcs->mse_seg[1]); free(pcs->skip_cdef_seg); free(pcs->cdef_dir_data);
    free(grid); free(mi); free(input); free(cm); free(scs); free(ppcs); free(pcs);
    return 0;
}
"""

SOURCES = ["Codec/cdef.c", "Codec/enc_cdef.c", "Codec/aom_dsp_rtcd.c", "Codec/common_dsp_rtcd.c"]


def build(ref, tmp):
    """Symbols the link still wants get stand-ins: the SIMD bodies the rtcd files name, the system-resource calls of the CDEF process's thread function
    and what the rest of the compiled sources calls."""
    L = refbuild.build(ref, tmp, "cdefref", SOURCES, [("harness", HARNESS)], flags=["-DNDEBUG"], standins=True)
    L.harness_run.argtypes = [C.c_void_p] * 11
    if L.harness_init():
        raise RuntimeError("harness_init failed")
    return L


def run(L, w, h, bd, q, sf, sy, suv, bias, lam, stages, masks, planes, mse=None, hdr=None, fb_strength=None, damping=3):
    """the harness on one picture: (mse [2][n_fb][64], dir, var, hdr [20], fb_strength, the three output planes)"""
    n_fb = cc.n_fb_of(w, h)
    dt = np.uint16 if bd > 8 else np.uint8
    p = np.array([w, h, bd, q, sf, len(sy), bias, lam, stages, damping], np.int32)
    a_sy, a_suv = np.array(list(sy) + [0] * (64 - len(sy)), np.uint8), np.array(list(suv) + [0] * (64 - len(suv)), np.int8)
    keep = [np.ascontiguousarray(pl, dt) for pl in planes]
    ptrs = (C.c_void_p * 6)(*[a.ctypes.data for a in keep])
    mse = np.zeros((2, n_fb, 64), np.uint64) if mse is None else np.ascontiguousarray(mse, np.uint64).copy()
    dirs, var = np.zeros((n_fb, 64), np.uint8), np.zeros((n_fb, 64), np.int32)
    hdr = np.zeros(20, np.int32) if hdr is None else np.ascontiguousarray(hdr, np.int32).copy()
    fbs = np.full(n_fb, cc.FILL, np.uint8).view(np.int8) if fb_strength is None else np.ascontiguousarray(fb_strength, np.int8).copy()
    outs = [np.zeros_like(a) for a in keep[:3]]
    optrs = (C.c_void_p * 3)(*[a.ctypes.data for a in outs])
    m = np.ascontiguousarray(masks, np.uint64)
    rc = L.harness_run(p.ctypes.data, a_sy.ctypes.data, a_suv.ctypes.data, m.ctypes.data, ptrs, mse.ctypes.data, dirs.ctypes.data, var.ctypes.data, hdr.ctypes.data,
                       fbs.ctypes.data, optrs)
    if rc:
        raise RuntimeError(f"harness_run returned {rc}")
    return mse, dirs, var, hdr, fbs, outs


def pick_of(hdr, fbs, mse, like):
    """the reference's pick laid out as cdef_cases.restate_pick's; the two costs, locals of the reference, are the restatement's"""
    return {"cdef_bits": int(hdr[0]), "nb_strengths": int(hdr[1]), "y_strength": [int(v) for v in hdr[2:10]], "uv_strength": [int(v) for v in hdr[10:18]],
            "best_cost": like["best_cost"], "zero_cost": like["zero_cost"], "cdef_dist_dev": int(hdr[18]), "fb_strength": fbs, "mse": mse}


def reference(L):
    """the reference's outputs of every case, laid out as the restatements'"""
    search, pick, apply = {}, {}, {}
    for name in cc.SEARCH_CASES:
        c = cc.search_case(name)
        want_s, want_p, _, _ = cc.restated_chain(name)
        searched = cc.searched_masks(name)
        args = (c["w"], c["h"], c["bd"], c["base_q_idx"], c["sf"], c["sy"], c["suv"], c["bias"], c["lam"])
        mse, dirs, var = run(L, *args, 1, searched, list(c["recon"]) + list(c["src"]))[:3]  # the search on its own: mse before the bias
        s = {k: v.copy() for k, v in want_s.items()}  # what the device leaves alone keeps the fill; the rest is the reference's
        n, live = len(c["sy"]), searched != 0
        for fb in np.flatnonzero(live):
            blocks = [b for b in range(64) if (int(searched[fb]) >> b) & 1]
            s["dir"][fb, blocks], s["var"][fb, blocks] = dirs[fb, blocks], var[fb, blocks]
            s["mse"][:, fb, :n] = mse[:, fb, :n]
        mse_b, _, _, hdr, fbs, outs = run(L, *args, 7, searched, list(c["recon"]) + list(c["src"]))  # the three in the encoder's order
        assert int(hdr[19]) == c["damping"]
        biased = s["mse"].copy()
        biased[:, live, 0] = mse_b[:, live, 0]
        search[name] = (s, pick_of(hdr, fbs, biased, want_p), outs, None)
    for name in cc.PICK_CASES:
        c = cc.pick_case(name)
        want = cc.restated_pick(name)[0]
        flat = [np.zeros((c["h"] >> (i > 0), c["w"] >> (i > 0)), np.uint8) for i in (0, 1, 2)] * 2
        mse, _, _, hdr, fbs, _ = run(L, c["w"], c["h"], 10 if c["is_hbd"] else 8, 0, 1, c["map_y"], c["map_y"], c["bias"], c["lam"], 2, c["masks"], flat, mse=c["mse"])
        p = pick_of(hdr, fbs, mse, want)
        p["uv_strength"] = [c["map_uv"][c["map_y"].index(v)] if g < p["nb_strengths"] else 0 for g, v in enumerate(p["uv_strength"])]  # the reference maps both through one list
        pick[name] = p
    for name in cc.APPLY_CASES:
        c = cc.apply_case(name)
        hdr = np.zeros(20, np.int32)
        hdr[2:2 + len(c["y_strength"])], hdr[10:10 + len(c["uv_strength"])] = c["y_strength"], c["uv_strength"]
        masks = np.array([int(m) & cc.valid_mask(min(64, c["w"] - 64 * (fb % ((c["w"] + 63) // 64))), min(64, c["h"] - 64 * (fb // ((c["w"] + 63) // 64))))
                          for fb, m in enumerate(c["masks"])], np.uint64)
        outs = run(L, c["w"], c["h"], c["bd"], 0, 1, [0], [0], 0, 0, 4, masks, list(c["planes"]) * 2, hdr=hdr, fb_strength=c["fb_strength"], damping=c["damping"])[5]
        apply[name] = outs[:c["n_planes"]]
    return search, pick, apply


def generate(L):
    search, pick, apply = reference(L)
    got, mine = cc.fixture_arrays(search, pick, apply), cc.fixture_arrays()
    bad = refbuild.compare(mine, got)
    if bad:
        raise RuntimeError(f"the restatement differs from the reference in {len(bad)} arrays: {bad[:12]}")
    missing = cc.coverage_missing()
    if missing:
        raise RuntimeError(f"conditions of the case list that are not met: {missing}")
    print(f"{len(cc.SEARCH_CASES)} search-pick-apply chains, {len(cc.PICK_CASES)} picks and {len(cc.APPLY_CASES)} applies: every output of the restatement equal to "
          f"the reference's; all {len(cc.CONDITIONS)} conditions met")
    return got


def time_reference(L):
    """the reference's C time on a 3840x2160 picture, full masks: this machine's CPU, one thread"""
    w, h = 3840, 2160
    masks = cc.masks_of("full", w, h)
    for bd in (8, 10):
        recon, src = cc.picture("noise", w, h, bd, 99)
        for n in (64, 4):
            sy = list(range(n)) if n == 64 else [0, 9, 33, 63]
            t0 = time.perf_counter()
            mse = run(L, w, h, bd, 100, 1, sy, sy, 60, 500, 1, masks, list(recon) + list(src))[0]
            t1 = time.perf_counter()
            run(L, w, h, bd, 100, 1, sy, sy, 60, 500, 2, masks, list(recon) + list(src), mse=mse)
            t2 = time.perf_counter()
            print(f"reference C, {w}x{h}, {bd}-bit, {n} strengths: search {1e3 * (t1 - t0):.0f} ms, pick {1e3 * (t2 - t1):.0f} ms (each with the harness's copies)")
        hdr = np.zeros(20, np.int32)
        hdr[2:6], hdr[10:14] = [13, 40, 63, 2], [13, 40, 63, 2]
        t0 = time.perf_counter()
        run(L, w, h, bd, 0, 1, [0], [0], 0, 0, 4, masks, list(recon) * 2, hdr=hdr, fb_strength=np.arange(len(masks)) % 4, damping=4)
        print(f"reference C, {w}x{h}, {bd}-bit: apply {1e3 * (time.perf_counter() - t0):.0f} ms")


if __name__ == "__main__":
    refbuild.main(__doc__, build, {cc.GOLDEN: generate}, flags=[("--time", "report the reference's C time on a 3840x2160 picture and stop")],
                  first=lambda a, L: a.time and (time_reference(L) or True))
