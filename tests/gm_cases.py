"""The cases of the global-motion entries (svt_hip_gm_refine_batch, svt_hip_gm_correspondence_batch) and numpy restatements of both, shared by
tests/test_gm.py, tests/test_gm_gpu.py and tools/gen_gm_golden.py, which compares the restatements with the reference encoder on every output of
every case and writes golden/gm.npz.  The restatements follow the reference's C line by line (Source/Lib/Codec/global_motion.c:
svt_av1_refine_integerized_param, add_param_offset, force_wmtype, get_wmtype, correspondence_from_mvs; enc_warped_motion.c: svt_av1_warp_error
without its early exit -- see include/svt_hip_gm.h for why that changes nothing; global_me.c:162-169, :354-360), in Python integers where C has 32-
and 64-bit ones.  The tile arithmetic, svt_get_shear_params and is_affine_shear_allowed are warp_cases'."""
import functools
import os

import numpy as np

import warp_cases as wc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gm.npz")
ST_OK, ST_IDENTICAL, ST_UNDEFINED = 0, 1, 0xFF
IDENTITY, TRANSLATION, ROTZOOM, AFFINE = 0, 1, 2, 3
N_ERRORS = 61
INT64_MAX = (1 << 63) - 1
FILL = 0xA5
ONE = 1 << 16
GM_MAX = 1 << 12  # GM_TRANS_MAX and GM_ALPHA_MAX
REFINE_JOB_DTYPE = [("wmmat", "<i4", (6,)), ("params_cost", "<i4"), ("ref", "u1"), ("wmtype", "u1"), ("reserved", "u1", (2,)), ("best_frame_error", "<i8")]
MODEL_DTYPE = wc.MODEL_DTYPE
i32 = wc.i32


# ---- the refinement ----
def force_wmtype(m, t):
    if t <= TRANSLATION:
        m[2], m[3] = ONE, 0
    if t <= ROTZOOM:
        m[4], m[5] = i32(-m[3]), m[2]


def get_wmtype(m):
    if m[5] == ONE and not m[4] and m[2] == ONE and not m[3]:
        return IDENTITY if not m[1] and not m[0] else TRANSLATION
    return ROTZOOM if m[2] == m[5] and m[3] == i32(-m[4]) else AFFINE


def add_param_offset(p, v, offset, trace=None):
    scale, centre = (10 if p < 2 else 1), (ONE if p in (2, 5) else 0)
    v = (i32(v - centre) >> scale) + offset
    if trace is not None and abs(v) > GM_MAX:
        trace.add("clamp_trans" if p < 2 else "clamp_alpha")
    return wc.clamp(v, -GM_MAX, GM_MAX) * (1 << scale) + centre


def warp_error(src, ref, mat, shear, chess, trace=None):
    """warp_error without its early exit: the SAD over the selected 32x32 blocks, cropped to the picture, doubled with chess"""
    splane, sox, soy, pw, ph = src
    total = 0
    for by, i in enumerate(range(0, ph, 32)):
        jstart, step = ((0 if by & 1 else 32), 64) if chess else (0, 32)
        if trace is not None and jstart >= pw:
            trace.add("chess_empty_row")
        for j in range(jstart, pw, step):
            for iy in range(i, min(i + 32, ph), 8):
                for jx in range(j, min(j + 32, pw), 8):
                    v = np.clip(wc.warp_tile(*ref, mat, shear, jx, iy, 0, 0, 8, 11) - 128 - 256, 0, 255)
                    h, w = min(8, ph - iy), min(8, pw - jx)
                    if trace is not None:
                        trace.update((["straddle_x"] if w < 8 else []) + (["straddle_y"] if h < 8 else []))
                    total += int(np.abs(v[:h, :w] - splane[soy + iy:soy + iy + h, sox + jx:sox + jx + w].astype(np.int64)).sum())
    return 2 * total if chess else total


def pic_sad(src, ref):
    (a, ax, ay, pw, ph), (b, bx, by, _, _) = ref, src
    return int(np.abs(a[ay:ay + ph, ax:ax + pw].astype(np.int64) - b[by:by + ph, bx:bx + pw].astype(np.int64)).sum()) & 0xFFFFFFFF


def shear_of(m):
    """svt_get_shear_params on the matrix as it stands"""
    return wc.shear_params(m)


def refine(b, job, trace=None, fresh=False):
    """one job: {"status", "wmmat", "shear", "wmtype", "valid", "best_error", "pic_sad", "round_error"}; None values are not written.  fresh: the
    counterfactual in which svt_warp_plane's ROTZOOM rewrite came before svt_get_shear_params (coverage only)"""
    t, ref = int(job["wmtype"]), int(job["ref"])
    out = {"status": ST_UNDEFINED, "wmmat": None, "shear": None, "wmtype": None, "valid": None, "best_error": None, "pic_sad": None, "round_error": None}
    if ref >= len(b["planes"]) or not TRANSLATION <= t <= AFFINE:
        return out
    trace = set() if trace is None else trace
    src, plane, chess = b["src"], b["planes"][ref], b["chess_refn"]
    errs = [-1] * N_ERRORS
    out["pic_sad"], out["round_error"] = pic_sad(src, plane), errs
    if out["pic_sad"] == 0:
        trace.add("pic_sad0")
        out.update(status=ST_IDENTICAL, wmmat=[0, 0, ONE, 0, 0, ONE], shear=(0, 0, 0, 0), wmtype=IDENTITY, valid=1, best_error=0)
        return out
    m = [int(v) for v in job["wmmat"]]
    force_wmtype(m, t)
    state = {"warped": False}

    def evaluate():
        """svt_av1_warp_error on m as it stands: the shear test first, then svt_warp_plane's rewrite"""
        look = list(m)
        if fresh and t == ROTZOOM:
            look[5], look[4] = look[2], i32(-look[3])
        ok, sh = shear_of(look)
        if t == ROTZOOM:
            fr = list(m)
            fr[5], fr[4] = fr[2], i32(-fr[3])
            if ok and shear_of(fr) != (ok, sh):
                trace.add("stale_differs")
        if not ok:
            trace.add("refused_mat2" if m[2] <= 0 else "refused_shear")
            if state["warped"]:
                trace.add("refused_after_warped")
            return 1
        if t == ROTZOOM:
            m[5], m[4] = m[2], i32(-m[3])
        state["warped"] = True
        return warp_error(src, plane, m, sh, chess, trace)

    def finish(wmtype):
        ok, sh = shear_of(m)
        out.update(status=ST_OK, wmmat=list(m), shear=sh, wmtype=wmtype, valid=ok, best_error=best)
        return out

    errs[0] = evaluate()
    bfe = int(job["best_frame_error"])
    if bfe < errs[0]:
        trace.add("bfe_below_first")
    best = min(errs[0], bfe)
    if b["rfn_early_exit"]:
        e = float(best) / float(out["pic_sad"])
        if not (e < 0.50 and e * float(int(job["params_cost"])) < 15000.0):
            trace.add("early_exit_taken")
            return finish(t)
        trace.add("early_exit_not_taken")
    n_params, k = 2 * t, 0
    for i in range(b["n_refinements"]):
        step = 16 >> i
        for p in range(n_params):
            cur = best_param = m[p]
            m[p] = left = add_param_offset(p, cur, -step, trace)
            errs[1 + 2 * k] = el = evaluate()
            took_left = el < best
            if took_left:
                best, best_param = el, left
            m[p] = right = add_param_offset(p, cur, step, trace)
            errs[2 + 2 * k] = er = evaluate()
            took_right = er < best
            if took_right:
                best, best_param = er, right
            m[p] = best_param
            trace.update((["left_accepted"] if took_left else []) + (["right_accepted"] if took_right else []) +
                         (["right_after_left"] if took_left and took_right else []) + (["right_equal_left"] if er == el else []) +
                         (["none_accepted"] if not took_left and not took_right else []))
            k += 1
    force_wmtype(m, t)
    if get_wmtype(m) != t:
        trace.add("wmtype_changed")
    return finish(get_wmtype(m))


def restate_refine(b, traces=None, fresh=False):
    """the outputs of a batch as the device leaves them over buffers that start as the byte FILL"""
    n = len(b["jobs"])
    out = {"models": np.frombuffer(bytes([FILL]) * (n * np.dtype(MODEL_DTYPE).itemsize), MODEL_DTYPE).copy(),
           "best_error": np.frombuffer(bytes([FILL]) * (8 * n), "<i8").copy(), "pic_sad": np.frombuffer(bytes([FILL]) * (4 * n), "<u4").copy(),
           "status": np.zeros(n, np.uint8), "round_error": np.frombuffer(bytes([FILL]) * (8 * n * N_ERRORS), "<i8").reshape(n, N_ERRORS).copy()}
    for i, job in enumerate(b["jobs"]):
        tr = set()
        r = refine(b, job, tr, fresh)
        if traces is not None:
            traces.append(tr)
        out["status"][i] = r["status"]
        if r["status"] == ST_UNDEFINED:
            continue
        rec = np.zeros((), MODEL_DTYPE)
        rec["wmmat"], rec["wmtype"], rec["valid"] = r["wmmat"], r["wmtype"], r["valid"]
        rec["alpha"], rec["beta"], rec["gamma"], rec["delta"] = r["shear"]
        out["models"][i], out["best_error"][i], out["pic_sad"][i], out["round_error"][i] = rec, r["best_error"], r["pic_sad"], r["round_error"]
    return out


# ---- the pictures and the case list ----
def pictures(seed, pw, ph, pad=8):
    """(source, [reference 0: the source moved by (+3, -2) samples; reference 1: zoomed and turned a little; reference 2: the source itself]); planes as
    warp_cases.make_plane's, regenerated from the seed"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:ph + 32, 0:pw + 32].astype(np.float64)
    base = 128 + 50 * np.sin(xx / 6.5 + yy / 11.0) + 40 * np.sin(xx / 3.1 - yy / 4.7) + 25 * np.sin((xx * yy) / 190.0) + rng.integers(-5, 6, xx.shape)
    base = np.clip(base, 0, 255).astype(np.uint8)

    def plane(pic):
        p = np.full((ph + 2 * pad, pw + 2 * pad + 3), 0x55, np.uint8)
        p[pad:pad + ph, pad:pad + pw] = pic
        return (p, pad, pad, pw, ph)
    o = 16
    src = base[o:o + ph, o:o + pw]
    moved = base[o - 2:o - 2 + ph, o + 3:o + 3 + pw]
    y, x = np.mgrid[0:ph, 0:pw]
    sx = np.clip(np.rint(o + 1.02 * x + 0.015 * y + 1.5), 0, pw + 31).astype(int)
    sy = np.clip(np.rint(o - 0.015 * x + 1.02 * y - 1.0), 0, ph + 31).astype(int)
    return plane(src), [plane(moved), plane(base[sy, sx]), plane(src.copy())]


def job(wmmat, wmtype, ref=0, params_cost=300, bfe=INT64_MAX):
    j = np.zeros((), REFINE_JOB_DTYPE)
    j["wmmat"], j["wmtype"], j["ref"], j["params_cost"], j["best_frame_error"] = wmmat, wmtype, ref, params_cost, bfe
    return j


def px(v):
    """a translation in samples as a wmmat entry (a multiple of GM_TRANS_DECODE_FACTOR)"""
    return int(round(v * 64)) << 10


T_NEAR = [px(-3.3), px(1.8), ONE, 0, 0, ONE]            # near reference 0's motion
R_NEAR = [px(-1.4), px(1.2), ONE - 1280, -960, 960, ONE - 1280]  # near reference 1's
A_NEAR = [px(-1.6), px(0.9), ONE - 1200, -1100, 900, ONE - 1400]
SIZES = [(32, 32), (40, 24), (72, 44), (100, 70), (176, 144)]


def _raw_jobs():
    # n_refinements 0 pins the raw warp error; the AFFINE job with a translation's matrix ends as TRANSLATION
    return [job(T_NEAR, TRANSLATION, 0), job(R_NEAR, ROTZOOM, 1), job(A_NEAR, AFFINE, 1), job(T_NEAR, AFFINE, 0)]


# name: (seed, (width, height), chess_refn, n_refinements, rfn_early_exit, jobs)
def _batches():
    b = {}
    for n, (w, h) in enumerate(SIZES):
        for chess in (0, 1):
            b[f"raw_{w}x{h}_{chess}"] = (10 + n, (w, h), chess, 0, 0, _raw_jobs())
    b["one_72x44"] = (21, (72, 44), 0, 1, 0, [job(R_NEAR, ROTZOOM, 1)])
    b["two_100x70"] = (22, (100, 70), 1, 5, 0, [job(T_NEAR, TRANSLATION, 0), job(A_NEAR, AFFINE, 1)])
    b["rot_40x24"] = (23, (40, 24), 0, 5, 0, [job(R_NEAR, ROTZOOM, 1), job([px(2.0), px(-1.0), ONE + 900, -2040, 0, 0], ROTZOOM, 1)])
    b["chess_32x32"] = (24, (32, 32), 1, 1, 0, [job(T_NEAR, TRANSLATION, 0), job(A_NEAR, AFFINE, 1)])
    # five jobs that end at different rounds: an early exit (a model far off), a refused start (wmmat[2] <= 0), a picture equal to the source, a
    # best_frame_error below the first error, and a model at both clamps
    b["mixed_72x44"] = (25, (72, 44), 1, 5, 1, [
        job([px(-9.0), px(9.0), ONE, 0, 0, ONE], TRANSLATION, 0, params_cost=800),
        job([px(1.0), px(1.0), -5, 300, 0, 0], ROTZOOM, 1),
        job(A_NEAR, AFFINE, 2),
        job(T_NEAR, TRANSLATION, 0, bfe=900),
        job(R_NEAR, ROTZOOM, 1)])
    # the shear test on the edge: beta = 7936 with alpha = 2432 is allowed, the next multiple of 64 is not; and a model at both clamps
    b["shear_72x44"] = (26, (72, 44), 0, 2, 0, [job([px(1.0), px(-1.0), ONE + 2432, 7936, -900, ONE + 1400], AFFINE, 1), job(R_NEAR, ROTZOOM, 0),
                                                job([GM_MAX << 10, -(GM_MAX << 10), ONE, 0, -2 * GM_MAX, ONE], AFFINE, 1)])
    b["undefined_32x32"] = (27, (32, 32), 0, 1, 0, [job(T_NEAR, TRANSLATION, 3), job(T_NEAR, 0, 0), job(T_NEAR, 4, 0), job(T_NEAR, TRANSLATION, 0)])
    b["big_176x144"] = (28, (176, 144), 1, 1, 1, [job(R_NEAR, ROTZOOM, 1, params_cost=200), job(T_NEAR, TRANSLATION, 0, params_cost=200)])
    return b


BATCHES = _batches()


def batch_names():
    return list(BATCHES)


@functools.lru_cache(maxsize=None)
def batch(name):
    seed, (w, h), chess, n_ref, early, jobs = BATCHES[name]
    src, planes = pictures(seed, w, h)
    return {"name": name, "src": src, "planes": planes, "chess_refn": chess, "n_refinements": n_ref, "rfn_early_exit": early,
            "jobs": wc.pack_jobs(jobs, REFINE_JOB_DTYPE)}


@functools.lru_cache(maxsize=None)
def restated(name):
    traces = []
    return restate_refine(batch(name), traces), traces


def fixture_arrays(name, out):
    """the outputs of a batch as golden/gm.npz holds them: numbers only"""
    m = out["models"]
    ok = out["status"] != ST_UNDEFINED
    return {f"refine_{name}_wmmat": m["wmmat"][ok].astype(np.int32), f"refine_{name}_shear": np.stack([m[k][ok] for k in ("alpha", "beta", "gamma", "delta")], 1).astype(np.int16),
            f"refine_{name}_type_valid": np.stack([m["wmtype"][ok], m["valid"][ok]], 1).astype(np.uint8), f"refine_{name}_best_error": out["best_error"][ok].astype(np.int64),
            f"refine_{name}_pic_sad": out["pic_sad"][ok].astype(np.uint32), f"refine_{name}_status": out["status"].astype(np.uint8),
            f"refine_{name}_round_error": out["round_error"][ok].astype(np.int64)}


CONDITIONS = ["left_accepted", "right_accepted", "right_after_left", "right_equal_left", "none_accepted", "clamp_trans", "clamp_alpha", "refused_mat2",
              "refused_shear", "refused_after_warped", "stale_shear_decides", "early_exit_taken", "early_exit_not_taken", "bfe_below_first", "pic_sad0",
              "wmtype_changed", "chess_empty_row", "straddle_x", "straddle_y"]


def stale_shear_decides(names=None):
    """the (batch, job) pairs of ROTZOOM jobs in which an evaluation's stale and fresh shear parameters differ AND the search with fresh ones keeps
    another parameter value"""
    hits = []
    for name in names or batch_names():
        b, (out, traces) = batch(name), restated(name)
        for i, (j, tr) in enumerate(zip(b["jobs"], traces)):
            if int(j["wmtype"]) == ROTZOOM and "stale_differs" in tr and out["status"][i] == ST_OK:
                other = refine(b, j, fresh=True)
                if other["wmmat"][:4] != [int(v) for v in out["models"][i]["wmmat"][:4]]:
                    hits.append((name, i))
    return hits


def coverage_missing(names=None):
    """the conditions that no job of the named batches (default: all) meets, and the picture sizes they leave out with the chess pattern on or off"""
    names = names or batch_names()
    seen = set()
    for name in names:
        for tr in restated(name)[1]:
            seen |= tr
    if stale_shear_decides(names):
        seen.add("stale_shear_decides")
    missing = [c for c in CONDITIONS if c not in seen]
    have = {(BATCHES[n][1], BATCHES[n][2]) for n in names}
    return missing + [f"shape_{w}x{h}_{c}" for (w, h) in SIZES for c in (0, 1) if ((w, h), c) not in have]


# ---- the correspondences ----
MV_64x64, MV_32x32, MV_16x16, MV_8x8 = range(4)
ME_ARRAYS = ("total_me_candidate_index", "me_candidate_array", "me_mv_array", "rc_me_distortion", "stationary_block_present_sb", "rc_me_allow_gm")


def cand_byte(direction, ref_idx_l0=0, ref_idx_l1=0, ref0_list=0, ref1_list=0):
    """MeCandidate (me_sb_results.h:28-34) as its byte"""
    return direction | ref_idx_l0 << 2 | ref_idx_l1 << 4 | ref0_list << 6 | ref1_list << 7


def n_pu_of(e16, e8):
    return (85 if e8 else 21) if e16 else 5


def fold_pu(n, e8, e16):
    """global_motion.c:263-269 over me_idx_85_8x8_to_16x16_conversion and me_idx_16x16_to_parent_32x32_conversion"""
    if not e8:
        if n >= 21:
            i = n - 21
            n = 5 + ((i >> 4) << 2) + ((i & 7) >> 1)
        if not e16 and n >= 5:
            i = n - 5
            n = 1 + ((i >> 3) << 1) + ((i & 3) >> 1)
    return n


def restate_corr(c):
    """{"corr": int32 [pairs][cap][4] over the byte FILL, "count": uint32 [pairs], "sums": uint32 [3]}"""
    pic, a = c["pic"], c["arrays"]
    aw, ah, e8, e16 = pic["aligned_width"], pic["aligned_height"], pic["enable_me_8x8"], pic["enable_me_16x16"]
    w64, h64 = (aw + 63) // 64, (ah + 63) // 64
    bpl, bsize, start = 1 << c["method"], 64 >> c["method"], (0, 1, 5, 21)[c["method"]]
    corr = np.frombuffer(bytes([FILL]) * (len(c["pairs"]) * c["cap"] * 16), "<i4").reshape(len(c["pairs"]), c["cap"], 4).copy()
    count = np.zeros(len(c["pairs"]), np.uint32)
    for q, (li, ri) in enumerate(c["pairs"]):
        n = 0
        for b64 in range(w64 * h64):
            for i in range(bpl * bpl):
                x, y = (b64 % w64) * 64 + (i % bpl) * bsize, (b64 // w64) * 64 + (i // bpl) * bsize
                if x >= aw or y >= ah:
                    continue
                pu = fold_pu(start + i, e8, e16)
                found = False
                for k in range(int(a["total_me_candidate_index"][b64, pu])):
                    cd = int(a["me_candidate_array"][b64, pu * pic["max_cand"] + k])
                    d = cd & 3
                    if (d == 0 and li == (cd >> 6) & 1 and ri == (cd >> 2) & 3) or (d == 1 and li == (cd >> 7) & 1 and ri == (cd >> 4) & 3):
                        found = True
                        break
                if found:
                    mv = int(a["me_mv_array"][b64, pu * pic["max_refs"] + (pic["max_l0"] if li else 0) + ri])
                    mvx, mvy = wc.i16(mv & 0xFFFF), wc.i16(mv >> 16)
                    corr[q, n] = [x >> c["shift"], y >> c["shift"], (x + mvx) >> c["shift"], (y + mvy) >> c["shift"]]
                    n += 1
        count[q] = n
    sums = np.array([int(a["rc_me_distortion"].astype(np.uint64).sum()) & 0xFFFFFFFF, int(a["stationary_block_present_sb"].sum()), int(a["rc_me_allow_gm"].sum())], np.uint32)
    return {"corr": corr, "count": count, "sums": sums}


# name: (seed, method, shift, (enable_me_16x16, enable_me_8x8), slice: "P" one list / "B" two)
CORR_CASES = {"m64_p": (40, MV_64x64, 0, (1, 1), "P"), "m32_b": (41, MV_32x32, 1, (1, 1), "B"), "m16_b": (42, MV_16x16, 2, (1, 1), "B"),
              "m8_b": (43, MV_8x8, 0, (1, 1), "B"), "m8_no8_b": (44, MV_8x8, 1, (1, 0), "B"), "m8_no16_p": (45, MV_8x8, 0, (0, 0), "P"),
              "m16_no16_b": (46, MV_16x16, 2, (0, 0), "B")}


@functools.lru_cache(maxsize=None)
def corr_case(name):
    """a 3 x 2-b64 picture whose aligned size (168 x 104) cuts the last column and row of 8x8 and 16x16 blocks; candidates and MVs from the seed"""
    seed, method, shift, (e16, e8), kind = CORR_CASES[name]
    rng = np.random.default_rng(seed)
    r0, r1 = (3, 0) if kind == "P" else (2, 2)  # P: a third reference that no candidate names
    pic = {"aligned_width": 168, "aligned_height": 104, "enable_me_8x8": e8, "enable_me_16x16": e16, "max_refs": r0 + r1, "max_l0": r0,
           "max_cand": r0 + r1 + r0 * r1 + (r0 - 1)}
    n_b64, n_pu, mc = 6, n_pu_of(e16, e8), pic["max_cand"]
    a = {"total_me_candidate_index": np.zeros((n_b64, n_pu), np.uint8), "me_candidate_array": np.zeros((n_b64, n_pu * mc), np.uint8),
         "me_mv_array": np.zeros((n_b64, n_pu * pic["max_refs"]), np.uint32), "rc_me_distortion": rng.integers(0, 1 << 31, (n_b64, 1)).astype(np.uint32),
         "stationary_block_present_sb": rng.integers(0, 2, (n_b64, 1)).astype(np.uint8), "rc_me_allow_gm": rng.integers(0, 2, (n_b64, 1)).astype(np.uint8)}
    uni = [cand_byte(0, ref_idx_l0=r) for r in range(2)] + [cand_byte(1, ref_idx_l1=r, ref1_list=1) for r in range(r1)]
    if kind == "B":
        uni.append(cand_byte(1, ref_idx_l1=1, ref1_list=0))  # a backward candidate of list 0, as only_l_bwd leaves it
    bi = [cand_byte(2, ref_idx_l0=0, ref_idx_l1=0, ref0_list=0, ref1_list=1)] if r1 else []
    for b in range(n_b64):
        for p in range(n_pu):
            k = int(rng.integers(0, mc + 1))
            pool = [uni[i] for i in rng.permutation(len(uni))] + bi
            pick = [pool[i] for i in rng.permutation(len(pool))[:k]]
            a["total_me_candidate_index"][b, p] = len(pick)
            a["me_candidate_array"][b, p * mc:p * mc + len(pick)] = pick
            mv = rng.integers(-200, 60, (pic["max_refs"], 2))  # (x, y): far enough left and up for a negative pos + mv
            a["me_mv_array"][b, p * pic["max_refs"]:(p + 1) * pic["max_refs"]] = (mv[:, 0] & 0xFFFF) | ((mv[:, 1] & 0xFFFF) << 16)
    pairs = [(0, 0), (0, 1)] + ([(1, 0), (1, 1), (0, 0)] if r1 else [(0, 2)])  # P: a pair no candidate names; B: the same pair twice
    cap = (1 << (2 * method)) * n_b64
    return {"name": name, "pic": pic, "arrays": a, "method": method, "shift": shift, "pairs": pairs, "cap": cap}


@functools.lru_cache(maxsize=None)
def restated_corr(name):
    return restate_corr(corr_case(name))


def corr_fixture_arrays(name, out):
    n = out["count"]
    return {f"corr_{name}_count": n.astype(np.uint32), f"corr_{name}_entries": np.concatenate([out["corr"][q, :int(n[q])] for q in range(len(n))]).astype(np.int32)}


CORR_CONDITIONS = ["count0", "negative", "cut_column", "cut_row", "bipred_skipped", "fold_8x8", "fold_16x16", "not_first_candidate"]


def corr_coverage_missing(names=None):
    seen = set()
    for name in names or list(CORR_CASES):
        c, out = corr_case(name), restated_corr(name)
        pic, a = c["pic"], c["arrays"]
        if (out["count"] == 0).any():
            seen.add("count0")
        for q in range(len(c["pairs"])):
            if (out["corr"][q, :int(out["count"][q])] < 0).any():
                seen.add("negative")
        bsize = 64 >> c["method"]
        if bsize <= 16:
            seen |= {"cut_column", "cut_row"}  # 168 = 2 * 64 + 40 and 104 = 64 + 40: origins 48 and 56 of the last b64 lie beyond
        if ((a["me_candidate_array"] & 3) == 2).any():
            seen.add("bipred_skipped")
        if c["method"] == MV_8x8 and not pic["enable_me_8x8"]:
            seen.add("fold_8x8")
        if c["method"] >= MV_16x16 and not pic["enable_me_16x16"]:
            seen.add("fold_16x16")
        if pic["max_cand"] > 1:
            seen.add("not_first_candidate")
    return [c for c in CORR_CONDITIONS if c not in seen]
