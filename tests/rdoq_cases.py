"""RDOQ of the mode decision (the trellis pass over quantised coefficients), restated in Python integers, and the case lists of its tests.
Reference (Source/Lib):
  the caller's frame of svt_aom_quantize_inv_quantize, is_encode_pass == 0   Codec/full_loop.c:1764-1817,1832-1836
  svt_av1_optimize_b                                                          Codec/full_loop.c:1127-1336
  update_coeff_general / _eob / _simple, update_skip                          Codec/full_loop.c:948-999,847-947,1001-1045,1046-1061
  get_coeff_cost_general / _eob, get_two_coeff_cost_simple, get_br_cost_with_diff (and its two Golomb tables)   Codec/full_loop.c:734-838
  get_eob_cost, get_dqv, get_qc_dqc_low, get_coeff_dist, plane_rd_mult        Codec/full_loop.c:694-711,840-845,762-772,1077-1085
  svt_fast_optimize_b = update_coeff_eob_fast                                 Codec/full_loop.c:1092-1126
  get_lower_levels_ctx, get_lower_levels_ctx_eob, get_br_ctx_eob, get_padded_idx   Codec/coefficients.h:2851-2950
  get_br_ctx                                                                  Codec/common_utils.h:114-151
  RDCOST (signed 64-bit)                                                      Codec/rd_cost.h:37
  svt_av1_compute_cul_level_c                                                 Codec/full_loop.c:1449-1466
TUNE_CHROMA_SSIM is 1 (Source/API/EbDebugMacros.h:43): plane_rd_mult = {17, 13}, {16, 10}; the fixture pins it.
The fixture (golden/rdoq.npz, written by tools/gen_rdoq_golden.py) holds the reference's own results on CASES; the rate tables are those of
golden/coeff_rate.npz (the generator derives them again and compares).  Inputs are regenerated from the seeds: the coefficients here, their "fp"
and "b" quantizations by the CPU oracle (oracle/liboracle.so), which the generator compares with the reference's."""
import ctypes as C
import os
import zlib

import numpy as np

import coeff_rate_cases as cr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rdoq.npz")

LOG_SCALE = [0, 0, 0, 1, 2, 0, 0, 0, 0, 1, 1, 2, 2, 0, 0, 0, 0, 1, 1]  # av1_get_tx_scale_tab (Codec/full_loop.h:53)
PLANE_RD_MULT = [[17, 13], [16, 10]]                                  # [is_inter][plane_type], TUNE_CHROMA_SSIM == 1
GOLOMB_BITS_COST = [0, 512] + [512 * 3] * 2 + [512 * 5] * 4 + [512 * 7] * 8 + [512 * 9] * 16
GOLOMB_COST_DIFF = [0, 512, 1024, 0, 1024, 0, 0, 0, 1024] + [0] * 7 + [1024] + [0] * 15
ST_OPTIMISED, ST_EMPTY, ST_GATED, ST_UNDEFINED = 0, 1, 2, 0xFF
RDOQ_JOB_DTYPE = [("tx_type", "u1"), ("txb_skip_ctx", "u1"), ("dc_sign_ctx", "u1"), ("is_inter", "u1"), ("quant_row", "u1"), ("flags", "u1"),
                  ("reserved", "u1", (2,))]
EVENTS = ("head_shortens", "skip_zeroes", "fifth_then_lower", "one_to_zero", "dc_lowered", "last_lowered", "early_return", "full_decision", "nothing")


def rdcost(rm, r, d):
    """RDCOST: ROUND_POWER_OF_TWO((int64)R * RM, 9) + D * 128, signed (D = dist - dist0 is negative)"""
    return ((r * rm + 256) >> 9) + d * 128


def coeff_dist(t, d, shift):
    return ((t - d) * (1 << shift)) ** 2


def rdmult_of(lam, is_inter, plane, sharp, sharpness):
    rweight = 0 if sharp else 100
    return ((lam * PLANE_RD_MULT[1 if is_inter else 0][plane] * rweight) // 100 + 2) >> max(2, min(7, max(0, sharpness)))


def cost_lists(T, tx_size, plane):
    """the LvMapCoeffCost of (tx_size, plane) as nested Python lists (the walk indexes them element by element)"""
    cache = T.__dict__.setdefault("_cost_lists", {})
    key = ((cr.SQR_MAP[tx_size] + cr.SQR_UP_MAP[tx_size] + 1) >> 1, plane)
    if key not in cache:
        cache[key] = {m: a.tolist() for m, a in T.coeff_costs(tx_size, plane).items()}
    return cache[key]


class Walk:
    """svt_av1_optimize_b's state on one block: Python lists q / dq (updated in place), the padded levels array, the contexts"""

    def __init__(self, T, tx_size, plane, tx_type, coeff, q, dq, dequant, iqm):
        self.ts, self.plane, self.cls = tx_size, plane, cr.tx_class(tx_type)
        self.w, self.h = cr.packed_dims(tx_size)
        self.bwl = self.w.bit_length() - 1
        self.stride = self.w + 4
        self.shift = LOG_SCALE[tx_size]
        self.cc = cost_lists(T, tx_size, plane)
        self.T = T
        self.t, self.q, self.dq, self.dequant, self.iqm = coeff, q, dq, dequant, iqm
        self.shape = 1 if cr.TX_W[tx_size] < cr.TX_H[tx_size] else (2 if cr.TX_W[tx_size] > cr.TX_H[tx_size] else 0)
        self.lv = [0] * (self.stride * (self.h + 4))

    def init_levels(self):
        w, s, lv, q = self.w, self.stride, self.lv, self.q
        for r in range(self.h):
            for c in range(w):
                v = abs(q[r * w + c])
                lv[r * s + c] = v if v < 127 else 127

    def set_level(self, ci, a):
        self.lv[(ci >> self.bwl) * self.stride + (ci & (self.w - 1))] = a if a < 127 else 127

    def dqv(self, ci):
        d = self.dequant[1 if ci else 0]
        return d if self.iqm is None else (self.iqm[ci] * d + 16) >> 5

    def ctx(self, ci):
        """get_lower_levels_ctx"""
        row, col = ci >> self.bwl, ci & (self.w - 1)
        s, lv, i = self.stride, self.lv, (ci >> self.bwl) * self.stride + (ci & (self.w - 1))
        m = min(lv[i + 1], 3) + min(lv[i + s], 3)
        if self.cls == 0:
            if ci == 0:
                return 0
            m += min(lv[i + s + 1], 3) + min(lv[i + 2], 3) + min(lv[i + 2 * s], 3)
            if self.shape == 1 and row < 2:
                off = 11
            elif self.shape == 2 and col < 2:
                off = 16
            else:
                off = 1 if row + col < 2 else (6 if row + col < 4 else 21)
        elif self.cls == 2:
            m += min(lv[i + 2 * s], 3) + min(lv[i + 3 * s], 3) + min(lv[i + 4 * s], 3)
            off = 26 if row == 0 else (31 if row == 1 else 36)
        else:
            m += min(lv[i + 2], 3) + min(lv[i + 3], 3) + min(lv[i + 4], 3)
            off = 26 if col == 0 else (31 if col == 1 else 36)
        return min((m + 1) >> 1, 4) + off

    def ctx_eob(self, si):
        """get_lower_levels_ctx_eob"""
        n = self.w * self.h
        return 0 if si == 0 else (1 if si <= n // 8 else (2 if si <= n // 4 else 3))

    def near(self, ci):
        row, col = ci >> self.bwl, ci & (self.w - 1)
        return (row < 2 and col < 2) if self.cls == 0 else (col == 0 if self.cls == 1 else row == 0)

    def br_ctx_eob(self, ci):
        return 0 if ci == 0 else (7 if self.near(ci) else 14)

    def br_ctx(self, ci):
        s, lv, i = self.stride, self.lv, (ci >> self.bwl) * self.stride + (ci & (self.w - 1))
        m = lv[i + 1] + lv[i + s] + (lv[i + s + 1] if self.cls == 0 else (lv[i + 2] if self.cls == 1 else lv[i + 2 * s]))
        m = min((m + 1) >> 1, 6)
        return m if ci == 0 else m + (7 if self.near(ci) else 14)

    def br_cost(self, level, lps):
        """get_br_cost"""
        g = 0
        if level >= 15:
            g = 512 * (2 * (level - 14).bit_length() - 1)
        return lps[min(level - 3, 12)] + g

    def cost_general(self, is_last, ci, a, sign, ctx, dc_ctx):
        """get_coeff_cost_general (is_last: get_coeff_cost_eob)"""
        cc = self.cc
        cost = cc["base_eob_cost"][ctx][min(a, 3) - 1] if is_last else cc["base_cost"][ctx][min(a, 3)]
        if a:
            cost += cc["dc_sign_cost"][dc_ctx][sign] if ci == 0 else 512
            if a > 2:
                cost += self.br_cost(a, cc["lps_cost"][self.br_ctx_eob(ci) if is_last else self.br_ctx(ci)])
        return cost

    def two_cost_simple(self, ci, a, ctx, ev):
        """get_two_coeff_cost_simple: (cost, cost_low)"""
        cc = self.cc
        cost = cc["base_cost"][ctx][min(a, 3)]
        diff = cc["base_cost"][ctx][a + 4] if a <= 3 else 0
        if a:
            cost += 512
            if a > 2:  # get_br_cost_with_diff
                lps = cc["lps_cost"][self.br_ctx(ci)]
                base_range = min(a - 3, 12)
                g = 0
                if a <= 15:
                    diff += lps[base_range + 13]
                if a >= 15:
                    r = a - 14
                    if r < 32:
                        g = GOLOMB_BITS_COST[r]
                        diff += GOLOMB_COST_DIFF[r]
                    else:
                        g = 512 * (2 * r.bit_length() - 1)
                        diff += 1024 if r & (r - 1) == 0 else 0
                    if ev is not None:
                        ev["golomb_table" if r < 32 else "golomb_formula"] = True
                cost += lps[base_range] + g
        return cost, cost - diff

    def low(self, a, sign, dqv):
        """get_qc_dqc_low: (qc_low, dqc_low)"""
        al = a - 1
        dl = (al * dqv) >> self.shift
        return (-al if sign else al), (-dl if sign else dl)


def eob_fast_trim(scan, shift, dequant, coeff, q, dq, eob):
    """update_coeff_eob_fast: the un-weighted dequant, zbin = dq + ROUND_POWER_OF_TWO(dq * 70, 7)"""
    zbin = [dequant[k] + ((dequant[k] * 70 + 64) >> 7) for k in (0, 1)]
    out = eob
    for i in range(eob - 1, -1, -1):
        rc = int(scan[i])
        if (abs(coeff[rc]) << (1 + shift)) < zbin[1 if rc else 0] or q[rc] == 0:
            out -= 1
            q[rc] = dq[rc] = 0
        else:
            break
    return out


def optimize_b(T, tx_size, plane, job, coeff, q, dq, eob, dequant, iqm, lam, sharpness, fast_mode, ev=None):
    """svt_av1_optimize_b on Python lists q / dq (in place); returns the new eob.  job: (tx_type, txb_skip_ctx, dc_sign_ctx, is_inter, sharp).
    ev: optional dict that collects what the walk did (EVENTS, golomb_table / golomb_formula)."""
    tx_type, skip_ctx, dc_ctx, is_inter, sharp = job
    W = Walk(T, tx_size, plane, tx_type, coeff, q, dq, dequant, iqm)
    cc, shift, cls = W.cc, W.shift, W.cls
    scan = cr.scan_order(tx_size, tx_type).tolist()
    non_skip_cost, skip_cost = cc["txb_skip_cost"][skip_ctx]
    accu_rate = cr.eob_cost(T, cc, tx_size, plane, eob, cls)
    if fast_mode:
        eob = eob_fast_trim(scan, shift, dequant, coeff, q, dq, eob)
        if eob == 0:
            return 0
    sharp = 1 if sharp else 0
    rdmult = rdmult_of(lam, is_inter, plane, sharp, sharpness)
    if eob > 1:
        W.init_levels()
    accu_dist = 0
    si = eob - 1
    ci = scan[si]
    changed = False

    def general(si, eob):
        """update_coeff_general without its accumulators' rate half (returns the accu_dist term); True when the level was lowered"""
        ci = scan[si]
        qc = q[ci]
        is_last = si == eob - 1
        ctx = W.ctx_eob(si) if is_last else W.ctx(ci)
        if qc == 0:
            return (0, 0), False
        sign, a, tqc = (1 if qc < 0 else 0), abs(qc), coeff[ci]
        dist, dist0 = coeff_dist(tqc, dq[ci], shift), coeff_dist(tqc, 0, shift)
        rate = W.cost_general(is_last, ci, a, sign, ctx, dc_ctx)
        rd = rdcost(rdmult, rate, dist)
        if a == 1:
            qc_low = dqc_low = 0
            dist_low, rate_low = dist0, cc["base_cost"][ctx][0]
        else:
            qc_low, dqc_low = W.low(a, sign, W.dqv(ci))
            dist_low = coeff_dist(tqc, dqc_low, shift)
            rate_low = W.cost_general(is_last, ci, a - 1, sign, ctx, dc_ctx)
        if rdcost(rdmult, rate_low, dist_low) < rd:
            q[ci], dq[ci] = qc_low, dqc_low
            W.set_level(ci, a - 1)
            return (rate_low, dist_low - dist0), True
        return (rate, dist - dist0), False

    qc = q[ci]
    nz_ci = [ci]
    if abs(qc) >= 2:
        (r, d), lowered = general(si, eob)
        accu_rate += r
        accu_dist += d
        changed |= lowered
        if lowered and ev is not None:
            ev["last_lowered"] = True
    else:
        accu_rate += W.cost_general(True, ci, 1, 1 if qc < 0 else 0, W.ctx_eob(si), dc_ctx)
        accu_dist += coeff_dist(coeff[ci], dq[ci], shift) - coeff_dist(coeff[ci], 0, shift)
    si -= 1
    while si >= 0 and len(nz_ci) <= 4 and not fast_mode:  # update_coeff_eob
        ci = scan[si]
        qc = q[ci]
        ctx = W.ctx(ci)
        if qc == 0:
            accu_rate += cc["base_cost"][ctx][0]
        else:
            lower = False
            a, tqc, sign = abs(qc), coeff[ci], 1 if qc < 0 else 0
            dist0 = coeff_dist(tqc, 0, shift)
            dist = coeff_dist(tqc, dq[ci], shift) - dist0
            rate = W.cost_general(False, ci, a, sign, ctx, dc_ctx)
            rd = rdcost(rdmult, accu_rate + rate, accu_dist + dist)
            if a == 1:
                al, qc_low, dqc_low, dist_low = 0, 0, 0, 0
                rate_low = cc["base_cost"][ctx][0]
                rd_low = rdcost(rdmult, accu_rate + rate_low, accu_dist)
            else:
                qc_low, dqc_low = W.low(a, sign, W.dqv(ci))
                al = a - 1
                dist_low = coeff_dist(tqc, dqc_low, shift) - dist0
                rate_low = W.cost_general(False, ci, al, sign, ctx, dc_ctx)
                rd_low = rdcost(rdmult, accu_rate + rate_low, accu_dist + dist_low)
            lower_new_eob = False
            ctx_new = W.ctx_eob(si)
            new_eob_cost = cr.eob_cost(T, cc, tx_size, plane, si + 1, cls)
            rate_coeff_eob = new_eob_cost + W.cost_general(True, ci, a, sign, ctx_new, dc_ctx)
            dist_new_eob = dist
            rd_new_eob = rdcost(rdmult, rate_coeff_eob, dist_new_eob)
            if al > 0:
                rate_low_eob = new_eob_cost + W.cost_general(True, ci, al, sign, ctx_new, dc_ctx)
                rd_new_eob_low = rdcost(rdmult, rate_low_eob, dist_low)
                if rd_new_eob_low < rd_new_eob:
                    lower_new_eob, rd_new_eob, rate_coeff_eob, dist_new_eob = True, rd_new_eob_low, rate_low_eob, dist_low
            if rd_low < rd:
                lower, rd, rate, dist = True, rd_low, rate_low, dist_low
            if sharp == 0 and rd_new_eob < rd:
                for k in nz_ci:
                    W.set_level(k, 0)
                    q[k] = dq[k] = 0
                eob = si + 1
                nz_ci = []
                accu_rate, accu_dist = rate_coeff_eob, dist_new_eob
                lower = lower_new_eob
                changed = True
                if ev is not None:
                    ev["head_shortens"] = True
            else:
                accu_rate += rate
                accu_dist += dist
            if lower:
                q[ci], dq[ci] = qc_low, dqc_low
                W.set_level(ci, al)
                changed = True
            if q[ci]:
                nz_ci.append(ci)
        si -= 1
    if si == -1 and len(nz_ci) <= 4:  # update_skip
        if sharp == 0 and rdcost(rdmult, skip_cost, 0) < rdcost(rdmult, accu_rate + non_skip_cost, accu_dist):
            for k in nz_ci:
                q[k] = dq[k] = 0
            eob = 0
            changed = True
            if ev is not None:
                ev["skip_zeroes"] = True
    fifth = len(nz_ci) > 4 and not fast_mode
    while si >= 1:  # update_coeff_simple: accu_rate is dead from here on
        ci = scan[si]
        qc = q[ci]
        if qc:
            a, at, ad = abs(qc), abs(coeff[ci]), abs(dq[ci])
            rate, rate_low = W.two_cost_simple(ci, a, W.ctx(ci), ev)
            if ad < at:
                if ev is not None:
                    ev["early_return"] = True
            else:
                if ev is not None:
                    ev["full_decision"] = True
                adl = ((a - 1) * W.dqv(ci)) >> shift
                if rdcost(rdmult, rate_low, coeff_dist(at, adl, shift)) < rdcost(rdmult, rate, coeff_dist(at, ad, shift)):
                    q[ci] = -(a - 1) if qc < 0 else a - 1
                    dq[ci] = -adl if qc < 0 else adl
                    W.set_level(ci, a - 1)
                    changed = True
                    if ev is not None:
                        if a == 1:
                            ev["one_to_zero"] = True
                        if fifth:
                            ev["fifth_then_lower"] = True
        si -= 1
    if si == 0:
        _, lowered = general(0, eob)
        changed |= lowered
        if lowered and ev is not None:
            ev["dc_lowered"] = True
    if ev is not None:
        if not changed:
            ev["nothing"] = True
        if ev.get("head_shortens") and eob == 0:
            ev["head_shortens"] = False  # the condition asks for a smaller NON-ZERO eob
    return eob


def cul_level(scan, q, eob):
    """svt_av1_compute_cul_level_c"""
    s = min(63, int(sum(abs(int(q[int(scan[c])])) for c in range(eob))))
    return (s | 64) if q[0] < 0 else (s + 128 if q[0] > 0 else s)


def job_defined(tx_size, job, n_quant_rows):
    return job["tx_type"] < 16 and job["txb_skip_ctx"] < 13 and job["dc_sign_ctx"] < 3 and job["quant_row"] < n_quant_rows


def run_job(T, case, i, q_in, dq_in, eob_in, fallback=None, ev=None):
    """What svt_hip_rdoq_batch leaves of job i: (status, qcoeff, dqcoeff, eob, dist_coeff or None, cul_level or None).  None = not written.
    fallback: (qcoeff_b, dqcoeff_b, eob_b) of the job, or None."""
    ts, plane = case["tx_size"], case["plane"]
    job = case["jobs"][i]
    w, h = cr.packed_dims(ts)
    n = w * h
    coeff = case["coeff"][i]
    eob = int(eob_in)
    untouched = lambda st: (st, np.array(q_in, np.int32), np.array(dq_in, np.int32), eob, None, None)
    if not job_defined(ts, job, len(case["quant_rows"])):
        return untouched(ST_UNDEFINED)
    tx_type = int(job["tx_type"])
    scan = cr.scan_order(ts, tx_type)
    q, dq = [int(v) for v in q_in], [int(v) for v in dq_in]
    status = ST_OPTIMISED
    if eob == 0:
        status = ST_EMPTY
    elif eob > n or q[int(scan[eob - 1])] == 0:
        return untouched(ST_UNDEFINED)
    else:
        dequant = [int(v) for v in case["quant_rows"][int(job["quant_row"])]["dequant"]]
        eob_perc = eob * 100 // (cr.TX_W[ts] * cr.TX_H[ts])
        if eob_perc >= case["eob_th"]:
            if fallback is None:
                return untouched(ST_GATED)
            status = ST_GATED
            q, dq, eob = [int(v) for v in fallback[0]], [int(v) for v in fallback[1]], int(fallback[2])
            if ev is not None:
                ev["eob_th_fires"] = True
        else:
            cl = [int(v) for v in coeff]
            if ev is not None:
                ev["eob_th_passes"] = True
            if eob_perc >= case["eob_fast_th"]:
                eob = eob_fast_trim(scan, LOG_SCALE[ts], dequant, cl, q, dq, eob)
                if ev is not None:
                    ev["fast_th_fires"] = True
                    if eob == 0:
                        ev["fast_trim_empties"] = True
            elif ev is not None:
                ev["fast_th_passes"] = True
            if eob == 0:
                status = ST_EMPTY
            else:
                iqm = None if case["iqmatrix"] is None or tx_type >= 9 else case["iqmatrix"].tolist()  # IS_2D_TRANSFORM (full_loop.c:1606)
                fast_mode = bool(case["eob_fast_inter"] if job["is_inter"] else case["eob_fast_intra"])
                eob = optimize_b(T, ts, plane, (tx_type, int(job["txb_skip_ctx"]), int(job["dc_sign_ctx"]), int(job["is_inter"]), int(job["flags"]) & 1),
                                 cl, q, dq, eob, dequant, iqm, case["lam"], case["sharpness"], fast_mode, ev)
    qa, dqa = np.array(q, np.int32), np.array(dq, np.int32)
    c64, d64 = coeff.astype(np.int64), dqa.astype(np.int64)
    dist = np.array([np.sum((c64 - d64) ** 2), np.sum(c64 ** 2)], np.uint64)  # svt_full_distortion_kernel32_bits
    return status, qa, dqa, eob, dist, cul_level(scan, q, eob)


def run_case(T, case, inputs, with_fallback=True, events=None):
    """run_job over a case: dict of arrays status / qcoeff / dqcoeff / eob / dist_coeff / cul_level (+ `written`: where dist_coeff and
    cul_level are written).  inputs: quantized(case).  events: optional list that receives one dict per job."""
    n = len(case["jobs"])
    out = {"status": np.zeros(n, np.uint8), "qcoeff": np.zeros_like(inputs["qcoeff"]), "dqcoeff": np.zeros_like(inputs["qcoeff"]),
           "eob": np.zeros(n, np.uint16), "dist_coeff": np.zeros((n, 2), np.uint64), "cul_level": np.zeros(n, np.uint8), "written": np.zeros(n, bool)}
    for i in range(n):
        ev = {} if events is not None else None
        fb = (inputs["qcoeff_b"][i], inputs["dqcoeff_b"][i], inputs["eob_b"][i]) if with_fallback else None
        st, q, dq, eob, dist, cul = run_job(T, case, i, inputs["qcoeff"][i], inputs["dqcoeff"][i], inputs["eob"][i], fb, ev)
        out["status"][i], out["qcoeff"][i], out["dqcoeff"][i], out["eob"][i] = st, q, dq, eob
        if dist is not None:
            out["dist_coeff"][i], out["cul_level"][i], out["written"][i] = dist, cul, True
        if events is not None:
            ev["cls"], ev["status"] = cr.tx_class(int(case["jobs"][i]["tx_type"])) if case["jobs"][i]["tx_type"] < 16 else -1, st
            events.append(ev)
    return out


# ---- the anti-diagonal property the kernel's simple phase relies on ---------------------------------------------------------------------
def context_neighbours(cls):
    """(row, column) offsets of every level get_nz_mag and get_br_ctx read around a position, by TxClass"""
    return {0: [(0, 1), (1, 0), (1, 1), (0, 2), (2, 0)], 1: [(0, 1), (1, 0), (0, 2), (0, 3), (0, 4)], 2: [(0, 1), (1, 0), (2, 0), (3, 0), (4, 0)]}[cls]


def antidiagonal_violations(tx_size, tx_type):
    """positions with a context neighbour (inside the block) whose row + column or whose scan index is not larger than their own"""
    w, h = cr.packed_dims(tx_size)
    scan = cr.scan_order(tx_size, tx_type)
    iscan = np.empty(w * h, np.int64)
    iscan[scan] = np.arange(w * h)
    bad = []
    for pos in range(w * h):
        r, c = divmod(pos, w)
        for dr, dc in context_neighbours(cr.tx_class(tx_type)):
            if r + dr < h and c + dc < w and not (dr + dc > 0 and iscan[(r + dr) * w + c + dc] > iscan[pos]):
                bad.append(pos)
    return bad


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
VARIANTS = [  # name, control overrides (sharp_mix: every third luma job carries the `sharp` flag)
    ("plain_y", dict(plane=0)), ("plain_uv", dict(plane=1)), ("sharp", dict(plane=0, sharp_mix=True)), ("sharpness4", dict(plane=1, sharpness=4)),
    ("sharpness7", dict(plane=0, sharpness=7)), ("eob_fast", dict(plane=0, eob_fast=True)), ("fast_th30", dict(plane=1, eob_fast_th=30)),
    ("fast_th0", dict(plane=0, eob_fast_th=0)), ("eob_th85", dict(plane=0, eob_th=85))]
LAMBDAS = (64, 6000, 400000, 1 << 24)   # against steps of 10, 75 and 640: from "changes nothing" to "zeroes most blocks"
AMPLITUDES = (0.6, 1.3, 3.0, 8.0, 30.0, 120.0)  # mean level of the DC, in quantizer steps
JOBS_PER_CASE = 25                      # odd: no multiple of the four / two jobs a wave holds at the small sizes


def quant_rows():
    """the rows of tests/rd_cases.py:quant_rows()"""
    from svt_av1_psyex_amd import rd
    return np.stack([rd.quant_row_from_step(8, 10), rd.quant_row_from_step(60, 75), rd.quant_row_from_step(500, 640)])


def matrices(tx_size):
    """one quantization matrix pair of the packed block (AOM_QM_BITS = 5: 32 is flat), weights rising with the frequency: (qmatrix, iqmatrix)"""
    w, h = cr.packed_dims(tx_size)
    r, c = np.mgrid[0:h, 0:w]
    iqm = 32 + ((r * 64 // h + c * 64 // w) * 3 // 4)
    qm = np.clip((1024 + iqm // 2) // iqm, 1, 255)
    return qm.reshape(-1).astype(np.uint8), iqm.reshape(-1).astype(np.uint8)


def build_case(tx_size, vi, seed=20261018):
    name, ctl = VARIANTS[vi]
    rng = np.random.default_rng([seed, tx_size, vi])
    w, h = cr.packed_dims(tx_size)
    n = JOBS_PER_CASE
    plane = ctl["plane"]
    rows = quant_rows()
    shift = LOG_SCALE[tx_size]
    jobs = np.zeros(n, RDOQ_JOB_DTYPE)
    coeff = np.zeros((n, w * h), np.int32)
    types = [cr.class_types(tx_size, k, 0, rng) for k in (0, 1)]
    r, c = np.mgrid[0:h, 0:w]
    for i in range(n):
        inter = (i >> 1) & 1
        jobs[i]["tx_type"] = types[inter][(i >> 2) % len(types[inter])]
        jobs[i]["txb_skip_ctx"], jobs[i]["dc_sign_ctx"], jobs[i]["is_inter"] = rng.integers(13), rng.integers(3), inter
        jobs[i]["quant_row"] = i % 3
        jobs[i]["flags"] = 1 if ctl.get("sharp_mix") and i % 3 == 1 else 0
        step = float(rows[i % 3]["dequant"][1]) / (1 << shift)
        amp = AMPLITUDES[(i // 3 + tx_size) % len(AMPLITUDES)] * np.exp(-(r + c) / ((w + h) * (0.06, 0.2, 0.6)[(i + vi) % 3]))
        mag = rng.exponential(1.0, (h, w)) * amp * step  # Laplacian magnitudes decaying with the frequency
        coeff[i] = (np.rint(mag) * rng.choice([-1, 1], (h, w))).reshape(-1).astype(np.int32)
    use_qm = (tx_size + vi) % 3 == 0
    fast = ctl.get("eob_fast", False)
    return {"tx_size": tx_size, "variant": vi, "plane": plane, "sharpness": ctl.get("sharpness", 0), "eob_fast_inter": int(fast),
            "eob_fast_intra": int(fast and tx_size % 3 != 1), "eob_th": ctl.get("eob_th", 255), "eob_fast_th": ctl.get("eob_fast_th", 255),
            "lam": LAMBDAS[(tx_size + vi) % len(LAMBDAS)], "table": (tx_size + vi) & 1, "bit_depth": 8 if (tx_size + (vi >> 1)) & 1 else 10,
            "qmatrix": matrices(tx_size)[0] if use_qm else None, "iqmatrix": matrices(tx_size)[1] if use_qm else None,
            "quant_rows": rows, "jobs": jobs, "coeff": coeff}


CASE_KEYS = [(ts, vi) for ts in range(cr.N_TX_SIZES) for vi in range(len(VARIANTS))]


def build_cases():
    return [build_case(*key) for key in CASE_KEYS]


def quantized(case):
    """the "fp" quantization of a case (what svt_hip_rd_batch writes with quant_kind 1: the kernel's input) and the "b" one (quant_kind 0: the
    fallback arrays), by the CPU oracle: dict qcoeff / dqcoeff / eob / qcoeff_b / dqcoeff_b / eob_b"""
    import pyoracle
    L = pyoracle.load_oracle()
    ts = case["tx_size"]
    n, npk = case["coeff"].shape
    out = {k: np.zeros((n, npk), np.int32) for k in ("qcoeff", "dqcoeff", "qcoeff_b", "dqcoeff_b")}
    out["eob"], out["eob_b"] = np.zeros(n, np.uint16), np.zeros(n, np.uint16)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    hbd = int(case["bit_depth"] != 8)
    for i in range(n):
        tt = int(case["jobs"][i]["tx_type"])
        scan = cr.scan_order(ts, tt).astype(np.int16)
        row = {k: np.ascontiguousarray(case["quant_rows"][int(case["jobs"][i]["quant_row"])][k]) for k in np.dtype(case["quant_rows"].dtype).names}
        two_d = tt < 9 and case["qmatrix"] is not None
        qm, iqm = (p(case["qmatrix"]), p(case["iqmatrix"])) if two_d else (None, None)
        co = np.ascontiguousarray(case["coeff"][i])
        L.orc_quantize_fp(p(co), C.c_ssize_t(npk), p(row["round_fp"]), p(row["quant_fp"]), p(out["qcoeff"][i]), p(out["dqcoeff"][i]), p(row["dequant"]),
                          p(out["eob"][i:]), p(scan), qm, iqm, LOG_SCALE[ts], hbd)
        L.orc_quantize_b(p(co), C.c_ssize_t(npk), p(row["zbin"]), p(row["round"]), p(row["quant"]), p(row["quant_shift"]), p(out["qcoeff_b"][i]),
                         p(out["dqcoeff_b"][i]), p(row["dequant"]), p(out["eob_b"][i:]), p(scan), qm, iqm, LOG_SCALE[ts], hbd)
    return out


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


SPOILS = 7


def spoil(c, inp, i, m):
    """makes job i (eob >= 2) of a case and its inputs, in place, one the reference leaves undefined: the m-th way of SPOILS"""
    n = c["coeff"].shape[1]
    if m == 0:
        inp["eob"][i] = n + 1
    elif m == 1:
        inp["eob"][i] = 65535
    elif m == 2:
        inp["qcoeff"][i, cr.scan_order(c["tx_size"], int(c["jobs"][i]["tx_type"]))[int(inp["eob"][i]) - 1]] = 0
    elif m == 3:
        c["jobs"][i]["txb_skip_ctx"] = 13
    elif m == 4:
        c["jobs"][i]["dc_sign_ctx"] = 3
    elif m == 5:
        c["jobs"][i]["tx_type"] = 16
    else:
        c["jobs"][i]["quant_row"] = len(c["quant_rows"])


def undefined_case(tx_size, seed=7):
    """jobs the reference leaves undefined among ordinary ones: (case, inputs, the indices of the undefined jobs)"""
    c = build_case(tx_size, 0, seed)
    inp = quantized(c)
    ok = [i for i in range(len(c["jobs"])) if inp["eob"][i] >= 2]
    bad = ok[1::2][:SPOILS]
    for m, i in enumerate(bad):
        spoil(c, inp, i, m)
    return c, inp, bad


PER_CLASS = EVENTS
OVERALL = ("golomb_table", "golomb_formula", "eob_th_fires", "eob_th_passes", "fast_th_fires", "fast_th_passes", "fast_trim_empties")


def coverage_missing(records):
    """The coverage conditions on the walks of `records` = [(case, events of run_case, ...)]: the names of those no job meets.  Per TxClass:
    the head shortens eob to a smaller non-zero value, update_skip zeroes the block, the head ends on the fifth non-zero and the simple phase
    lowers a level, a level goes 1 -> 0 in the simple phase, the DC is lowered, the last coefficient (>= 2) is lowered, abs_dqc < abs_tqc
    returns early and does not, nothing changes.  Over all cases: both Golomb branches of get_br_cost_with_diff in the simple phase (levels
    >= 15 and >= 46), each gate fires and does not, log-scale 0, 1 and 2, the fast trim empties a block."""
    seen = set()
    for rec in records:
        case, events = rec[0], rec[1]
        seen.add(("log_scale", LOG_SCALE[case["tx_size"]]))
        for ev in events:
            for name in PER_CLASS:
                if ev.get(name):
                    seen.add((name, ev["cls"]))
            for name in OVERALL:
                if ev.get(name):
                    seen.add(name)
    want = [(name, cls) for name in PER_CLASS for cls in (0, 1, 2)] + list(OVERALL) + [("log_scale", s) for s in (0, 1, 2)]
    return [w for w in want if w not in seen]


def cases_from_golden(z):
    """the fixture's cases: each build_case(...) with the reference's results as "ref" (qcoeff int32 [n][npk], eob, cul_level, status, dqcoeff_crc)"""
    out, j0, q0 = [], 0, 0
    for k, meta in enumerate(z["case_meta"].tolist()):
        c = build_case(meta[0], meta[1])
        assert case_meta(c) == meta, (meta, case_meta(c))
        n, npk = c["coeff"].shape
        c["ref"] = {"qcoeff": z["qcoeff"][q0:q0 + n * npk].reshape(n, npk).astype(np.int32), "eob": z["eob"][j0:j0 + n], "cul_level": z["cul_level"][j0:j0 + n],
                    "status": z["status"][j0:j0 + n], "dqcoeff_crc": int(z["dqcoeff_crc"][k])}
        out.append(c)
        j0, q0 = j0 + n, q0 + n * npk
    return out


def case_meta(c):
    return [c["tx_size"], c["variant"], c["plane"], c["sharpness"], c["eob_fast_inter"], c["eob_fast_intra"], c["eob_th"], c["eob_fast_th"], c["lam"],
            c["table"], c["bit_depth"], int(c["qmatrix"] is not None), len(c["jobs"])]


# ---- shared by tests/test_rdoq.py and tests/test_rdoq_gpu.py: everything is computed once per process ------------------------------------
_SHARED = {}


def shared():
    """{"cases": the fixture's cases, "tables": the rate tables of golden/coeff_rate.npz by table index}"""
    if not _SHARED:
        z = np.load(cr.GOLDEN)
        _SHARED["tables"] = [cr.Tables.from_golden(z, k) for k in range(len(cr.QINDEXES))]
        _SHARED["cases"] = cases_from_golden(np.load(GOLDEN))
        _SHARED["restated"] = {}
    return _SHARED


def restated(k):
    """(inputs, results with the fallback arrays, events) of fixture case k by the restatement, computed on first use and kept unchanged"""
    s = shared()
    if k not in s["restated"]:
        c = s["cases"][k]
        inp, ev = quantized(c), []
        want = run_case(s["tables"][c["table"]], c, inp, True, ev)
        for a in list(inp.values()) + list(want.values()):
            a.setflags(write=False)
        s["restated"][k] = (inp, want, ev)
    return s["restated"][k]
