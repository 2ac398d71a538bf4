#!/usr/bin/env python3
"""Writes tests/golden/gm.npz: the reference encoder's own svt_av1_refine_integerized_param and correspondence_from_mvs on the cases of
tests/gm_cases.py.

Run by hand on a machine that has the reference's sources (--ref: the root of its source tree); never by the tests, build(), smoke() or bench.py.
It compiles a harness of its own into a temporary directory outside the tree (gcc, -O2, -DNDEBUG as a release build of the encoder has it).  The
harness #includes Codec/global_motion.c where it lies, because correspondence_from_mvs is static, with svt_av1_warp_error renamed in it to a
function of the harness that calls the real one twice -- once as the reference does, once on a copy of the parameters with best_error INT64_MAX,
which is the evaluation without its early exit -- and records both, the best_error it was given and the parameters it left.  It links
Codec/enc_warped_motion.c, Codec/warped_motion.c, C_DEFAULT/compute_sad_c.c and the two rtcd files where they lie, with svt_nxm_sad_kernel_helper_c
and svt_av1_warp_affine_c installed in the rtcd pointers.  Whatever else the link still wants gets a stand-in that aborts.

Per refinement job the harness computes the picture SAD as global_me.c:354 does and, unless it is 0, calls svt_av1_refine_integerized_param.  Per
correspondence case it scripts a PictureParentControlSet (aligned size, the two ME switches, pa_me_data with one MeSbResults per b64, the
correspondence method, the down-sampling level that gives the shift) and calls correspondence_from_mvs for every pair.  The three picture sums of
global_me.c:162-169 are plain sums over per-b64 arrays and are not part of the fixture.

The fixture holds numbers only; pictures are regenerated from seeds.  --check recomputes everything and compares it with the committed file instead
of writing it.  Either way the restatement of tests/gm_cases.py is compared with the reference on every output of every case -- the error of every
evaluation without its early exit among them --, and the conditions of the case list are asserted on the REFERENCE's run: which side was accepted,
the refusals (an evaluation that returns 1 and leaves the parameters as they were), the ROTZOOM state (gamma and delta the reference used differ
from those of the fresh matrix, in a job whose kept parameters would differ with fresh ones), both ends of rfn_early_exit.  For every evaluation the
reference's own return and the full error are shown to lead to the same decision.  --time reports the reference's C time of picture-sized jobs."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import gm_cases as gc  # noqa: E402
import refbuild  # noqa: E402

HARNESS = r"""
#define svt_av1_warp_error harness_spy_warp_error
#include "global_motion.c"
#undef svt_av1_warp_error
#include <string.h>
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"
#include "pcs.h"
#include "sequence_control_set.h"

int64_t svt_av1_warp_error(EbWarpedMotionParams *wm, const uint8_t *ref, int width, int height, int stride, uint8_t *dst, int p_col, int p_row,
                           int p_width, int p_height, int p_stride, int subsampling_x, int subsampling_y, uint8_t chess_refn, int64_t best_error);
uint32_t svt_nxm_sad_kernel_helper_c(const uint8_t *src, uint32_t src_stride, const uint8_t *ref, uint32_t ref_stride, uint32_t height, uint32_t width);

/* per evaluation: 0 the return, 1 the full error, 2 best_error as given, 3..8 wmmat as left, 9..12 alpha beta gamma delta as left, 13..18 wmmat as found */
#define LOG_W 19
static int64_t *g_log;
static int      g_n, g_cap;

int64_t harness_spy_warp_error(EbWarpedMotionParams *wm, const uint8_t *ref, int width, int height, int stride, uint8_t *dst, int p_col, int p_row,
                               int p_width, int p_height, int p_stride, int subsampling_x, int subsampling_y, uint8_t chess_refn, int64_t best_error) {
    EbWarpedMotionParams copy = *wm;
    const int64_t full = svt_av1_warp_error(&copy, ref, width, height, stride, dst, p_col, p_row, p_width, p_height, p_stride, subsampling_x, subsampling_y,
                                            chess_refn, INT64_MAX);
    int64_t before[6];
    for (int i = 0; i < 6; i++) before[i] = wm->wmmat[i];
    const int64_t ret = svt_av1_warp_error(wm, ref, width, height, stride, dst, p_col, p_row, p_width, p_height, p_stride, subsampling_x, subsampling_y,
                                           chess_refn, best_error);
    if (g_log && g_n < g_cap) {
        int64_t *o = g_log + (size_t)g_n * LOG_W;
        o[0] = ret; o[1] = full; o[2] = best_error;
        for (int i = 0; i < 6; i++) { o[3 + i] = wm->wmmat[i]; o[13 + i] = before[i]; }
        o[9] = wm->alpha; o[10] = wm->beta; o[11] = wm->gamma; o[12] = wm->delta;
    }
    g_n++;
    return ret;
}

int harness_init(void) {
    svt_nxm_sad_kernel  = svt_nxm_sad_kernel_helper_c;
    svt_av1_warp_affine = svt_av1_warp_affine_c;
    return 0;
}

/* p: 0 width, 1 height, 2 source stride, 3 reference stride, 4 n_refinements, 5 chess_refn, 6 rfn_early_exit, 7 wmtype, 8 params_cost
 * out: 0 status (0 refined, 1 picture SAD 0), 1 best_error, 2 pic_sad, 3..8 wmmat, 9 wmtype, 10 valid, 11..14 the shear parameters of the final matrix,
 *      15 evaluations */
int harness_refine(const int *p, uint8_t *src, uint8_t *ref, const int32_t *wmmat, int64_t best_frame_error, int64_t *out, int64_t *log, int log_cap) {
    GmControls ctrls;
    memset(&ctrls, 0, sizeof(ctrls));
    ctrls.rfn_early_exit = (uint8_t)p[6];
    const uint32_t sad = svt_nxm_sad_kernel(ref, (uint32_t)p[3], src, (uint32_t)p[2], (uint32_t)p[1], (uint32_t)p[0]); /* global_me.c:354 */
    out[2] = sad;
    EbWarpedMotionParams wm = default_warp_params;
    g_log = log; g_n = 0; g_cap = log_cap;
    if (sad == 0) {
        out[0] = 1; out[1] = 0;
    } else {
        for (int i = 0; i < 6; i++) wm.wmmat[i] = wmmat[i];
        wm.wmtype = (TransformationType)p[7];
        out[0] = 0;
        out[1] = svt_av1_refine_integerized_param(&ctrls, &wm, (TransformationType)p[7], ref, p[0], p[1], p[3], src, p[0], p[1], p[2], p[4], (uint8_t)p[5],
                                                  best_frame_error, sad, p[8]);
    }
    for (int i = 0; i < 6; i++) out[3 + i] = wm.wmmat[i];
    out[9]  = wm.wmtype;
    out[10] = svt_get_shear_params(&wm); /* as compute_global_motion asks of the kept model (global_me.c:444) */
    out[11] = wm.alpha; out[12] = wm.beta; out[13] = wm.gamma; out[14] = wm.delta;
    out[15] = g_n;
    g_log = NULL;
    return 0;
}

/* p: 0 aligned_width, 1 aligned_height, 2 enable_me_8x8, 3 enable_me_16x16, 4 max_cand, 5 max_refs, 6 max_l0, 7 n_pu, 8 method, 9 shift, 10 list, 11 ref
 * out: [cap][4]; returns the count, or a negative number */
int harness_corr(const int *p, uint8_t *total, uint8_t *cands, uint32_t *mvs, int32_t *out, int cap) {
    PictureParentControlSet *pcs = (PictureParentControlSet *)calloc(1, sizeof(*pcs));
    SequenceControlSet      *scs = (SequenceControlSet *)calloc(1, sizeof(*scs));
    MotionEstimationData    *med = (MotionEstimationData *)calloc(1, sizeof(*med));
    if (!pcs || !scs || !med) return -2;
    if (sizeof(MeCandidate) != 1 || sizeof(MvCandidate) != 4) return -3;
    const int n_b64 = ((p[0] + 63) / 64) * ((p[1] + 63) / 64);
    scs->b64_size = 64;
    pcs->scs = scs; pcs->pa_me_data = med;
    pcs->aligned_width = (uint16_t)p[0]; pcs->aligned_height = (uint16_t)p[1];
    pcs->b64_total_count = (uint16_t)n_b64;
    pcs->enable_me_8x8 = (uint8_t)p[2]; pcs->enable_me_16x16 = (uint8_t)p[3];
    med->max_cand = (uint8_t)p[4]; med->max_refs = (uint8_t)p[5]; med->max_l0 = (uint8_t)p[6];
    med->me_results = (MeSbResults **)calloc((size_t)n_b64, sizeof(*med->me_results));
    MeSbResults *res = (MeSbResults *)calloc((size_t)n_b64, sizeof(*res));
    if (!med->me_results || !res) return -2;
    for (int b = 0; b < n_b64; b++) {
        res[b].total_me_candidate_index = total + (size_t)b * p[7];
        res[b].me_candidate_array = (MeCandidate *)(cands + (size_t)b * p[7] * p[4]);
        res[b].me_mv_array = (MvCandidate *)(mvs + (size_t)b * p[7] * p[5]);
        med->me_results[b] = &res[b];
    }
    pcs->gm_ctrls.correspondence_method = (CorrespondenceMethod)p[8];
    pcs->gm_downsample_level = p[9] == 0 ? GM_FULL : (p[9] == 1 ? GM_DOWN : GM_DOWN16);
    Correspondence *c = (Correspondence *)calloc((size_t)cap, sizeof(*c));
    if (!c) return -2;
    int n = 0;
    correspondence_from_mvs(pcs, c, &n, (uint8_t)p[10], (uint8_t)p[11]);
    if (n > cap) return -4;
    for (int i = 0; i < n; i++) { out[4 * i] = c[i].x; out[4 * i + 1] = c[i].y; out[4 * i + 2] = c[i].rx; out[4 * i + 3] = c[i].ry; }
    free(c); free(res); free(med->me_results); free(med); free(scs); free(pcs);
    return n;
}
"""

SOURCES = ["Codec/enc_warped_motion.c", "Codec/warped_motion.c", "C_DEFAULT/compute_sad_c.c", "Codec/aom_dsp_rtcd.c", "Codec/common_dsp_rtcd.c"]
LOG_W = 19


def build(ref, tmp):
    """Symbols the link still wants get stand-ins: the SIMD bodies the rtcd files name and what the rest of the compiled sources calls."""
    L = refbuild.build(ref, tmp, "gmref", SOURCES, [("harness", HARNESS)], standins=True)
    P = C.c_void_p
    L.harness_refine.argtypes = [P, P, P, P, C.c_int64, P, P, C.c_int]
    L.harness_corr.argtypes = [P, P, P, P, P, C.c_int]
    if L.harness_init():
        raise RuntimeError("harness_init failed")
    return L


def origin(plane):
    p, ox, oy, _, _ = plane
    return p.ctypes.data + oy * p.strides[0] + ox


def run_refine(L, b, job):
    """(out[16], the evaluation log [n][LOG_W]) of the reference for one defined job"""
    src, ref = b["src"], b["planes"][int(job["ref"])]
    p = np.array([src[3], src[4], src[0].shape[1], ref[0].shape[1], b["n_refinements"], b["chess_refn"], b["rfn_early_exit"], int(job["wmtype"]),
                  int(job["params_cost"])], np.int32)
    out, log = np.zeros(16, np.int64), np.zeros((gc.N_ERRORS, LOG_W), np.int64)
    mat = np.ascontiguousarray(job["wmmat"], np.int32)
    if L.harness_refine(p.ctypes.data, origin(src), origin(ref), mat.ctypes.data, int(job["best_frame_error"]), out.ctypes.data, log.ctypes.data, gc.N_ERRORS):
        raise RuntimeError("harness_refine failed")
    return out, log[:int(out[15])]


def reference_refine(L, name, seen, decisions):
    """the reference's outputs of a batch laid out as gm_cases.restate_refine's, and the conditions its run meets"""
    b = gc.batch(name)
    want, _ = gc.restated(name)
    out = {k: v.copy() for k, v in want.items()}  # the undefined jobs keep the fill; every defined one is overwritten below
    for i, job in enumerate(b["jobs"]):
        if want["status"][i] == gc.ST_UNDEFINED:
            continue
        t = int(job["wmtype"])
        o, log = run_refine(L, b, job)
        rec = np.zeros((), gc.MODEL_DTYPE)
        rec["wmmat"], rec["wmtype"], rec["valid"] = o[3:9], o[9], o[10]
        if o[5] > 0:  # with wmmat[2] <= 0 the reference leaves the four as they were: defined as 0 here
            rec["alpha"], rec["beta"], rec["gamma"], rec["delta"] = o[11:15]
        errs = np.full(gc.N_ERRORS, -1, np.int64)
        errs[:len(log)] = log[:, 1]
        out["models"][i], out["best_error"][i], out["pic_sad"][i], out["status"][i], out["round_error"][i] = rec, o[1], o[2], o[0], errs
        if o[0] == 1:
            seen.add("pic_sad0")
            continue
        # the early exit inside warp_error changes no decision
        bfe = int(job["best_frame_error"])
        for n, ev in enumerate(log):
            ret, full, best = int(ev[0]), int(ev[1]), int(ev[2])
            decisions[0] += 1
            if ret != full:
                decisions[1] += 1
            if n == 0:
                assert best == bfe and min(ret, bfe) == min(full, bfe), (name, i, n, ret, full, bfe)
            else:
                assert (ret < best) == (full < best), (name, i, n, ret, full, best)
        if bfe < log[0, 1]:
            seen.add("bfe_below_first")
        n_evals = len(log)
        if b["rfn_early_exit"]:
            seen.add("early_exit_taken" if n_evals == 1 and b["n_refinements"] else "early_exit_not_taken")
        refused = [int(ev[1]) == 1 and list(ev[3:9]) == list(ev[13:19]) and (ev[5] <= 0 or not gc.shear_of([int(v) for v in ev[3:9]])[0]) for ev in log]
        for n, ev in enumerate(log):
            if refused[n]:
                seen.add("refused_mat2" if ev[5] <= 0 else "refused_shear")
                if any(not r for r in refused[:n]):
                    seen.add("refused_after_warped")
            elif t == gc.ROTZOOM:
                fresh = gc.shear_of([int(v) for v in ev[3:9]])[1]
                if tuple(int(v) for v in ev[9:13]) != fresh:
                    seen.add(("stale", name, i))
        for k in range((n_evals - 1) // 2):
            (rl, _, bl), (rr, _, br) = log[1 + 2 * k, :3], log[2 + 2 * k, :3]
            tl, tr = rl < bl, rr < br
            seen.update((["left_accepted"] if tl else []) + (["right_accepted"] if tr else []) + (["right_after_left"] if tl and tr else []) +
                        (["right_equal_left"] if log[1 + 2 * k, 1] == log[2 + 2 * k, 1] else []) + (["none_accepted"] if not tl and not tr else []))
            p = k % (2 * t)
            for ev in log[1 + 2 * k:3 + 2 * k]:
                if abs(int(ev[3 + p]) - (gc.ONE if p in (2, 5) else 0)) == gc.GM_MAX << (10 if p < 2 else 1):
                    seen.add("clamp_trans" if p < 2 else "clamp_alpha")
        if n_evals > 1 or not b["rfn_early_exit"]:
            if int(o[9]) != t:
                seen.add("wmtype_changed")
    return out


def reference_corr(L, name):
    c = gc.corr_case(name)
    pic, a = c["pic"], c["arrays"]
    n_pu = gc.n_pu_of(pic["enable_me_16x16"], pic["enable_me_8x8"])
    out = {k: v.copy() for k, v in gc.restated_corr(name).items()}
    arr = [np.ascontiguousarray(a[k]) for k in ("total_me_candidate_index", "me_candidate_array", "me_mv_array")]
    for q, (li, ri) in enumerate(c["pairs"]):
        p = np.array([pic["aligned_width"], pic["aligned_height"], pic["enable_me_8x8"], pic["enable_me_16x16"], pic["max_cand"], pic["max_refs"], pic["max_l0"], n_pu,
                      c["method"], c["shift"], li, ri], np.int32)
        buf = np.zeros((c["cap"], 4), np.int32)
        n = L.harness_corr(p.ctypes.data, arr[0].ctypes.data, arr[1].ctypes.data, arr[2].ctypes.data, buf.ctypes.data, c["cap"])
        if n < 0:
            raise RuntimeError(f"{name} pair {q}: the harness returned {n}")
        out["count"][q] = n
        out["corr"][q] = np.frombuffer(bytes([gc.FILL]) * (c["cap"] * 16), "<i4").reshape(c["cap"], 4)
        out["corr"][q, :n] = buf[:n]
    return out


def generate(L):
    out, mismatch, seen, decisions, n_jobs = {}, [], set(), [0, 0], 0
    for name in gc.batch_names():
        ref, (want, _) = reference_refine(L, name, seen, decisions), gc.restated(name)
        got, mine = gc.fixture_arrays(name, ref), gc.fixture_arrays(name, want)
        for k in got:
            if not (got[k].dtype == mine[k].dtype and np.array_equal(got[k], mine[k])):
                mismatch.append((k, np.argwhere(got[k] != mine[k])[:4].tolist() if got[k].shape == mine[k].shape else "shape"))
        out.update(got)
        n_jobs += len(want["status"])
    for name in gc.CORR_CASES:
        ref, want = reference_corr(L, name), gc.restated_corr(name)
        if not (np.array_equal(ref["corr"], want["corr"]) and np.array_equal(ref["count"], want["count"])):
            mismatch.append((f"corr_{name}", ref["count"].tolist(), want["count"].tolist()))
        out.update(gc.corr_fixture_arrays(name, ref))
    if mismatch:
        raise RuntimeError(f"the restatement differs from the reference in {len(mismatch)} arrays, first: {mismatch[:8]}")
    # the ROTZOOM state: a job in which the reference used stale gamma / delta AND fresh ones would keep another parameter
    stale = {(n, i) for k in seen if isinstance(k, tuple) for _, n, i in [k]}
    if stale & set(gc.stale_shear_decides()):
        seen.add("stale_shear_decides")
    seen = {k for k in seen if not isinstance(k, tuple)}
    shapes = {"chess_empty_row", "straddle_x", "straddle_y"}  # properties of the pictures, not of a run: the restatement's own
    missing = [c for c in gc.CONDITIONS if c not in seen | shapes] + gc.coverage_missing() + gc.corr_coverage_missing()
    if missing:
        raise RuntimeError(f"conditions of the case list that are not met: {missing}")
    print(f"{n_jobs} refinement jobs in {len(gc.batch_names())} batches and {len(gc.CORR_CASES)} correspondence cases: every output of the restatement equal to the "
          f"reference's; {decisions[0]} evaluations, {decisions[1]} of them cut short by the early exit, none with another decision; stale shear in {sorted(stale)}")
    return out


def time_reference(L):
    """the reference's C time of one picture-sized job per type: this machine's CPU, one thread"""
    for (w, h), chess in (((3840, 2160), 1), ((1920, 1080), 1), ((960, 540), 1)):
        src, planes = gc.pictures(1, w, h)
        b = {"src": src, "planes": planes, "chess_refn": chess, "n_refinements": 5, "rfn_early_exit": 0}
        for t, m in ((gc.TRANSLATION, gc.T_NEAR), (gc.ROTZOOM, gc.R_NEAR), (gc.AFFINE, gc.A_NEAR)):
            t0 = time.perf_counter()
            o, log = run_refine(L, b, gc.job(m, t, 0 if t == gc.TRANSLATION else 1))
            print(f"reference C, {w}x{h} chess {chess}, wmtype {t}, 5 refinements: {len(log)} evaluations, {1e3 * (time.perf_counter() - t0) / 2:.1f} ms "
                  f"(half of the harness's, which evaluates twice)")


if __name__ == "__main__":
    refbuild.main(__doc__, build, {gc.GOLDEN: generate}, flags=[("--time", "report the reference's C time of picture-sized jobs and stop")],
                  first=lambda a, L: a.time and (time_reference(L) or True))
