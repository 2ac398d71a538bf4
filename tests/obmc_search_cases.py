"""The cases of svt_hip_obmc_search_batch and a numpy restatement of one job: single_motion_search for OBMC_CAUSAL (Source/Lib/Codec/mode_decision.c:
2290-2398) = svt_av1_set_mv_search_range (Codec/av1me.c:205-226), svt_av1_obmc_full_pixel_search -> obmc_refining_search_sad + get_obmc_mvpred_var
(:709-776), svt_av1_find_best_obmc_sub_pixel_tree_up (:963-1132; forced_stop 0, iters_per_step 2, USE_8_TAPS: svt_aom_upsampled_pred + the obmc
variance), mvsad_err_cost / svt_aom_mv_err_cost / their light forms (:229-261), svt_av1_mv_bit_cost{,_light} (Codec/rd_cost.c:61-87), obmc_sad and
obmc_variance (C_DEFAULT/sad_av1.c:18-32, C_DEFAULT/variance.c:347-373).

The reference's own results -- single_motion_search and the two av1me.c functions driven by tools/gen_obmc_golden.py -- are in golden/obmc.npz:
every output of every job.  The restatement also reports what happened inside a job (events), which is how the planted inputs are checked.

Geometry: a 192x128 picture inside a padding of 96, 8-bit.  A job's wsrc / mask come from obmc_cases.restate_target_block on strips cut from the
reference plane at a displacement of their own, so that they are what svt_hip_obmc_target_batch writes."""
import functools

import numpy as np

import obmc_cases as oc

PIC_W, PIC_H, PAD = 192, 128, 96
MV_CENTRE = 1 << 14
SIZES = [(8, 8), (16, 8), (32, 32), (64, 64)]
JOB_DTYPE = [("target_offset", "<u4"), ("ref_offset", "<u4"), ("width", "u1"), ("height", "u1"), ("reserved", "u1", (2,)), ("start_mv", "<i2", (2,)),
             ("ref_mv", "<i2", (2,)), ("col_min", "<i4"), ("col_max", "<i4"), ("row_min", "<i4"), ("row_max", "<i4"), ("reserved2", "<u4")]
RESULT_DTYPE = [("fullpel_value", "<i4"), ("besterr", "<u4"), ("distortion", "<i4"), ("sse1", "<u4"), ("rate_mv", "<i4"), ("reserved", "<u4")]
INT_MAX = 2 ** 31 - 1
# rows 0, 2, .. 14 of av1_sub_pel_filters_8 (C_DEFAULT/variance.c): what USE_8_TAPS selects for the 1/8 phases
TAPS8 = np.array([[0, 0, 0, 128, 0, 0, 0, 0], [0, 2, -10, 122, 18, -4, 0, 0], [0, 2, -14, 110, 38, -10, 2, 0], [0, 2, -16, 94, 58, -12, 2, 0],
                  [0, 2, -14, 76, 76, -14, 2, 0], [0, 2, -12, 58, 94, -16, 2, 0], [0, 2, -10, 38, 110, -14, 2, 0], [0, 0, -4, 18, 122, -10, 2, 0]], np.int64)
NEIGHBORS = [(-1, 0), (0, -1), (0, 1), (1, 0), (-1, 1), (1, 1), (1, -1), (-1, -1)]


def i16(v):
    return ((int(v) + 32768) & 0xFFFF) - 32768


def u32(v):
    return int(v) & 0xFFFFFFFF


def cost_tables(seed=3):
    """(mvjcost [4], row table, column table [32769]): the rate grows with the component, like a real table"""
    rng = np.random.default_rng([20261020, seed])
    j = np.array([11, 54, 5437, 342], np.int32)
    ramp = (np.abs(np.arange(-MV_CENTRE, MV_CENTRE + 1)) * 3 + 200).astype(np.int32)
    return j, (ramp + rng.integers(0, 64, ramp.size)).astype(np.int32), (ramp + rng.integers(0, 64, ramp.size)).astype(np.int32)


def mv_cost(dr, dc, tables):  # svt_mv_cost of an MV difference (int16)
    dr, dc = i16(dr), i16(dc)
    joint = (0 if dc == 0 else 1) if dr == 0 else (2 if dc == 0 else 3)
    clip = lambda v: max(-MV_CENTRE, min(MV_CENTRE, v))
    return int(tables[0][joint]) + int(tables[1][MV_CENTRE + clip(dr)]) + int(tables[2][MV_CENTRE + clip(dc)])


def upsampled(ref, y0, x0, w, h, row, col):
    """svt_aom_upsampled_pred with USE_8_TAPS of the w x h block whose co-located first sample is ref[y0][x0], at the 1/8 vector (row, col): an 8-bit
    intermediate after the horizontal pass"""
    y, x, yo, xo = y0 + (row >> 3), x0 + (col >> 3), row & 7, col & 7
    if not xo and not yo:
        return ref[y:y + h, x:x + w].astype(np.int64)
    if not yo:
        S = ref[y:y + h, x - 3:x + w + 5].astype(np.int64)
        return np.clip((sum(TAPS8[xo][k] * S[:, k:k + w] for k in range(8)) + 64) >> 7, 0, 255)
    if not xo:
        S = ref[y - 3:y + h + 5, x:x + w].astype(np.int64)
        return np.clip((sum(TAPS8[yo][k] * S[k:k + h] for k in range(8)) + 64) >> 7, 0, 255)
    S = ref[y - 3:y + h + 5, x - 3:x + w + 5].astype(np.int64)
    T = np.clip((sum(TAPS8[xo][k] * S[:, k:k + w] for k in range(8)) + 64) >> 7, 0, 255)
    return np.clip((sum(TAPS8[yo][k] * T[k:k + h] for k in range(8)) + 64) >> 7, 0, 255)


def restate_job(p, ref, wsrc_all, mask_all, job, tables):
    """One job: ((row, col), result record, events) or None when the job is undefined.  p: the batch's parameters; ref: the reference plane [rows][stride]."""
    w, h, stride = int(job["width"]), int(job["height"]), ref.shape[1]
    do_full = p["refine_level"] in (0, 1, 3)
    if (w, h) not in oc.SIZES or int(job["target_offset"]) + w * h > len(wsrc_all):
        return None
    light = bool(p["approx_inter_rate"])
    lim = {k: int(job[k]) for k in ("col_min", "col_max", "row_min", "row_max")}
    rmv = (int(job["ref_mv"][0]), int(job["ref_mv"][1]))
    br, bc = int(job["start_mv"][0]) >> 3, int(job["start_mv"][1]) >> 3
    fl = dict(lim)
    if do_full:  # svt_av1_set_mv_search_range and the double clamp_mv
        cmin, rmin = (rmv[1] >> 3) - 1023 + (rmv[1] & 7 != 0), (rmv[0] >> 3) - 1023 + (rmv[0] & 7 != 0)
        fl["col_min"], fl["row_min"] = max(lim["col_min"], max(cmin, -2047)), max(lim["row_min"], max(rmin, -2047))
        fl["col_max"], fl["row_max"] = min(lim["col_max"], min((rmv[1] >> 3) + 1023, 2047)), min(lim["row_max"], min((rmv[0] >> 3) + 1023, 2047))
        bc, br = max(fl["col_min"], min(fl["col_max"], bc)), max(fl["row_min"], min(fl["row_max"], br))
    # the guard: range samples of full-pel movement, then at most 14 / 8 sample either way (floor -2 / +1), then the taps (3 before, 4 after)
    rng_ = p["fpel_search_range"] if do_full else 0
    off = int(job["ref_offset"])
    g_lo, g_hi = (br - rng_ - 5, bc - rng_ - 5), (br + rng_ + 5 + h - 1, bc + rng_ + 5 + w - 1)
    if off + g_lo[0] * stride + g_lo[1] < 0 or off + g_hi[0] * stride + g_hi[1] >= ref.size:
        return None
    reads = [10 ** 9, 10 ** 9, -10 ** 9, -10 ** 9]  # the rows and columns actually read, relative to the co-located block: first row, first column, last, last

    def touch(r, c):  # a candidate at the 1/8 vector (r, c): its floor, and the taps where the phase is not 0
        r0, c0 = (r >> 3) - (3 if r & 7 else 0), (c >> 3) - (3 if c & 7 else 0)
        r1, c1 = (r >> 3) + h - 1 + (4 if r & 7 else 0), (c >> 3) + w - 1 + (4 if c & 7 else 0)
        reads[:] = [min(reads[0], r0), min(reads[1], c0), max(reads[2], r1), max(reads[3], c1)]
    y0, x0 = divmod(off, stride)
    o = int(job["target_offset"])
    wsrc, mask = wsrc_all[o:o + w * h].reshape(h, w).astype(np.int64), mask_all[o:o + w * h].reshape(h, w).astype(np.int64)
    ev = {"fp_steps": 0, "fp_stop": None, "fp_rejected": False, "fp_tie": False, "fp_cost_rejects": False, "sp_moved": [], "sp_diag_won": False, "sp_second_won": False,
          "sp_out_of_range": False}

    def obmc_sad(r, c):
        touch(r * 8, c * 8)
        d = np.abs(wsrc - ref[y0 + r:y0 + r + h, x0 + c:x0 + c + w].astype(np.int64) * mask)
        return int(((d + 2048) >> 12).sum())

    def obmc_var(r, c):  # (variance, sse) at the 1/8 vector
        touch(r, c)
        d = wsrc - upsampled(ref, y0, x0, w, h, r, c) * mask
        diff = np.where(d < 0, -((-d + 2048) >> 12), (d + 2048) >> 12)
        s, sse = int(diff.sum()), int((diff * diff).sum())
        return u32(sse - u32((s * s) // (w * h))), sse

    def err_cost(r, c):  # svt_aom_mv_err_cost{,_light} of an MV (int16)
        r, c = i16(r), i16(c)
        if light:
            return 1296 + 50 * (abs(c - rmv[1]) + abs(r - rmv[0]))
        return (mv_cost(r - rmv[0], c - rmv[1], tables) * p["error_per_bit"] + (1 << 13)) >> 14

    def sad_cost(r, c):  # mvsad_err_cost against ref_mv >> 3
        dr, dc = r - (rmv[0] >> 3), c - (rmv[1] >> 3)
        if light:
            return 1296 + 50 * (abs(dc) * 8 + abs(dr) * 8)
        return (u32(mv_cost(dr * 8, dc * 8, tables)) * p["sadpb"] + 256 & 0xFFFFFFFF) >> 9

    fullpel_value = 0
    if do_full:
        best = u32(obmc_sad(br, bc) + sad_cost(br, bc))
        ev["fp_stop"] = "range"
        for _ in range(p["fpel_search_range"]):
            site, site_total = -1, None
            for j in range(8 if p["fpel_search_diag"] else 4):
                r, c = br + NEIGHBORS[j][0], bc + NEIGHBORS[j][1]
                if not (fl["col_min"] <= c <= fl["col_max"] and fl["row_min"] <= r <= fl["row_max"]):
                    ev["fp_rejected"] = True
                    continue
                sad = obmc_sad(r, c)
                if site != -1 and u32(sad + sad_cost(r, c)) == site_total:
                    ev["fp_tie"] = True  # as good as the winner so far: the earlier site keeps it
                if sad < best:
                    total = u32(sad + sad_cost(r, c))
                    if total < best:
                        best, site, site_total = total, j, total
                    else:
                        ev["fp_cost_rejects"] = True
            if site == -1:
                ev["fp_stop"] = "none"
                break
            br, bc = br + NEIGHBORS[site][0], bc + NEIGHBORS[site][1]
            ev["fp_steps"] += 1
        fullpel_value = u32(obmc_var(br * 8, bc * 8)[0] + err_cost(br * 8, bc * 8))
        fullpel_value -= (fullpel_value >> 31) << 32  # returned as an int
    mx = 1023 * 8
    minc, maxc = max(-16383, max(lim["col_min"] * 8, rmv[1] - mx)), min(16383, min(lim["col_max"] * 8, rmv[1] + mx))
    minr, maxr = max(-16383, max(lim["row_min"] * 8, rmv[0] - mx)), min(16383, min(lim["row_max"] * 8, rmv[0] + mx))
    inside = lambda r, c: minc <= c <= maxc and minr <= r <= maxr
    br, bc = br * 8, bc * 8
    st = {"br": br, "bc": bc}
    dist, sse1 = obmc_var(br, bc)
    st.update(besterr=u32(dist + err_cost(br, bc)), dist=dist, sse1=sse1)

    def check(r, c):  # CHECK_BETTER1
        if not inside(r, c):
            ev["sp_out_of_range"] = True
            return False
        v, sse = obmc_var(r, c)
        if u32(err_cost(r, c) + v) < st["besterr"]:
            st.update(besterr=u32(err_cost(r, c) + v), br=r, bc=c, dist=v, sse1=sse)
            return True
        return False

    hstep = 4
    for _ in range(3 if p["allow_hp"] else 2):
        steps = [(0, -hstep), (0, hstep), (-hstep, 0), (hstep, 0)]
        cost, best_idx = [INT_MAX] * 5, -1
        br, bc = st["br"], st["bc"]
        for idx in range(4):
            tr, tc = br + steps[idx][0], bc + steps[idx][1]
            if inside(tr, tc):
                v, sse = obmc_var(tr, tc)
                cost[idx] = u32(v + err_cost(tr, tc))
                if cost[idx] < st["besterr"]:
                    best_idx = idx
                    st.update(besterr=cost[idx], dist=v, sse1=sse)
            else:
                ev["sp_out_of_range"] = True
        kc, kr = (-hstep if cost[0] <= cost[1] else hstep), (-hstep if cost[2] <= cost[3] else hstep)
        tc, tr = bc + kc, br + kr
        if inside(tr, tc):
            v, sse = obmc_var(tr, tc)
            cost[4] = u32(v + err_cost(tr, tc))
            if cost[4] < st["besterr"]:
                best_idx = 4
                st.update(besterr=cost[4], dist=v, sse1=sse)
        else:
            ev["sp_out_of_range"] = True
        if 0 <= best_idx < 4:
            br, bc = br + steps[best_idx][0], bc + steps[best_idx][1]
        elif best_idx == 4:
            br, bc = tr, tc
            ev["sp_diag_won"] = True
        st["br"], st["bc"] = br, bc
        if best_idx != -1:  # SECOND_LEVEL_CHECKS_BEST(1)
            br0, bc0 = br, bc
            if tr == br and tc != bc:
                kc = bc - tc
            elif tr != br and tc == bc:
                kr = br - tr
            won = check(br0 + kr, bc0)
            won = check(br0, bc0 + kc) or won
            if br0 != st["br"] or bc0 != st["bc"]:
                won = check(br0 + kr, bc0 + kc) or won
            ev["sp_second_won"] = ev["sp_second_won"] or won
        ev["sp_moved"].append(best_idx != -1)
        hstep >>= 1
    br, bc = st["br"], st["bc"]
    if light:
        rate = 1296 + 50 * (abs(bc - rmv[1]) + abs(br - rmv[0]))
    else:
        clip = lambda v: max(-MV_CENTRE, min(MV_CENTRE, i16(v)))
        rate = (mv_cost(clip(br - rmv[0]), clip(bc - rmv[1]), tables) * 108 + 64) >> 7
    # what was read lies inside what the guard proved, and (numpy would wrap a negative index silently) inside the plane
    assert reads[0] >= g_lo[0] and reads[1] >= g_lo[1] and reads[2] <= g_hi[0] and reads[3] <= g_hi[1], (reads, g_lo, g_hi)
    assert off + reads[0] * stride + reads[1] >= 0 and off + reads[2] * stride + reads[3] < ref.size
    ev["reads"] = (y0 + reads[0], x0 + reads[1], y0 + reads[2], x0 + reads[3])  # in the plane: first row, first column, last row, last column
    ev["reads_at_guard"] = (reads[0] == g_lo[0], reads[1] == g_lo[1], reads[2] == g_hi[0], reads[3] == g_hi[1])
    res = np.zeros((), RESULT_DTYPE)
    res["fullpel_value"], res["besterr"], res["distortion"], res["sse1"], res["rate_mv"] = fullpel_value, st["besterr"], st["dist"], st["sse1"], rate
    return (br, bc), res, ev


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_plane(kind="smooth"):
    """the padded 8-bit reference plane: low-pass noise (the searches have slopes to follow), a paraboloid, or a V of columns around x = 99.5 (mirror-symmetric)"""
    shape = (PIC_H + 2 * PAD, PIC_W + 2 * PAD)
    if kind == "bowl":  # a paraboloid around the plane's middle: the error falls all the way to the true displacement
        yy, xx = np.indices(shape)
        a = np.clip(((xx - shape[1] // 2) ** 2 + (yy - shape[0] // 2) ** 2) // 64, 0, 255).astype(np.uint8)
    elif kind == "vee":
        a = np.broadcast_to(np.minimum(np.abs(2 * (np.arange(shape[1]) - PAD) - 199) * 2, 250), shape).astype(np.uint8)
    else:
        n = np.random.default_rng([20261020, 4]).normal(0, 1, shape)
        k = np.exp(-0.5 * (np.arange(-12, 13) / 4.0) ** 2)
        for ax in (0, 1):
            n = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), ax, n)
        a = np.clip(128 + n * (90 / n.std()), 0, 255).astype(np.uint8)
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def mv_limits(org, w, h):
    """x->mv_limits as single_motion_search computes them: (col_min, col_max, row_min, row_max)"""
    mi_row, mi_col = org[1] >> 2, org[0] >> 2
    return (-((mi_col + (w >> 2)) * 4 + 4), ((PIC_W >> 2) - mi_col) * 4 + 4, -((mi_row + (h >> 2)) * 4 + 4), ((PIC_H >> 2) - mi_row) * 4 + 4)


def make_job(ref, org, w, h, true_mv, start_mv, ref_mv, nb_mv=(16, -24), neighbours=True, noise=0, src_const=None, seed=0):
    """(job without target_offset, wsrc, mask): the source is the reference's 8-tap prediction at true_mv (1/8) plus noise, the strips are the reference
    at nb_mv (full-pel part), both sides covered by one neighbour each (or none)"""
    y0, x0 = PAD + org[1], PAD + org[0]
    rng = np.random.default_rng([20261020, 5, seed])
    src = upsampled(ref, y0, x0, w, h, true_mv[0], true_mv[1]) if src_const is None else np.full((h, w), src_const, np.int64)
    src = np.clip(src + (rng.integers(-noise, noise + 1, (h, w)) if noise else 0), 0, 255).astype(np.uint8)
    strip = ref[y0 + (nb_mv[0] >> 3):y0 + (nb_mv[0] >> 3) + h, x0 + (nb_mv[1] >> 3):x0 + (nb_mv[1] >> 3) + w].reshape(-1)
    blk = oc.make_block(w, h, org, [oc.nb(0, w >> 2, nb_mv)] if neighbours else [], [oc.nb(0, h >> 2, nb_mv)] if neighbours else [])
    wsrc, mask = oc.restate_target_block(blk, strip, strip, src, 8)
    j = np.zeros((), JOB_DTYPE)
    j["ref_offset"], j["width"], j["height"], j["start_mv"], j["ref_mv"] = y0 * ref.shape[1] + x0, w, h, start_mv, ref_mv
    j["col_min"], j["col_max"], j["row_min"], j["row_max"] = mv_limits(org, w, h)
    return j, wsrc, mask


def finish(name, params, ref_kind, items):
    jobs = np.zeros(len(items), JOB_DTYPE)
    ws, ms, at = [], [], 3
    for i, (j, wsrc, mask) in enumerate(items):
        jobs[i] = j
        jobs[i]["target_offset"] = at
        ws.append((at, wsrc))
        ms.append(mask)
        at += len(wsrc) + 5
    W, M = oc.fill_i32(at), oc.fill_i32(at)
    for (o, wsrc), mask in zip(ws, ms):
        W[o:o + len(wsrc)], M[o:o + len(wsrc)] = wsrc, mask
    return {"name": name, "params": params, "ref": ref_kind, "jobs": jobs, "wsrc": W, "mask": M}


def params(level=0, light=0, diag=0, rng_=8, hp=1, sadpb=40, epb=60):
    return {"refine_level": level, "fpel_search_diag": diag, "fpel_search_range": rng_, "approx_inter_rate": light, "allow_hp": hp, "sadpb": sadpb, "error_per_bit": epb}


GRID = [(level, light, diag, r, hp) for level in range(5) for light in (0, 1) for diag in (0, 1) for r in (8, 16) for hp in (0, 1)]


def grid_batch(level, light, diag, r, hp):
    """group 1: every combination of refine level, rate mode, diagonal sites, range and allow_hp on the four sizes, true displacements of a few samples
    and every 1/8 phase in turn"""
    ref = ref_plane()
    rng = np.random.default_rng([6, level, light, diag, r, hp])
    items = []
    for k, (w, h) in enumerate(SIZES):
        org = (int(rng.integers(2, (PIC_W - w) // 8 - 1)) * 8, int(rng.integers(2, (PIC_H - h) // 8 - 1)) * 8)
        true = (int(rng.integers(-28, 29)), int(rng.integers(-28, 29)))
        start = (true[0] + int(rng.integers(-20, 21)), true[1] + int(rng.integers(-20, 21)))
        items.append(make_job(ref, org, w, h, true, start, (start[0] + int(rng.integers(-9, 10)), start[1] + int(rng.integers(-9, 10))), noise=2, seed=k))
    return finish(f"grid_{level}_{light}_{diag}_{r}_{hp}", params(level, light, diag, r, hp), "smooth", items)


def planted_batches():
    """group 2: the inputs planted for what the issue lists; {name: batch}"""
    ref = ref_plane()
    out = {}
    # far: the true displacement is 20 samples away: the full-pel search moves for several steps and the range stops it; at once: it starts where it ends
    bowl = ref_plane("bowl")
    far = [make_job(bowl, (64, 48), w, h, (160, -120), (0, 0), (0, 0), neighbours=False) for w, h in SIZES]
    near = [make_job(bowl, (64, 48), w, h, (24, 16), (24, 16), (24, 16), neighbours=False) for w, h in SIZES]
    out["far_8"] = finish("far_8", params(0, 0, 0, 8, 1, sadpb=4), "bowl", far)
    out["far_16_diag"] = finish("far_16_diag", params(1, 0, 1, 16), "bowl", far)
    out["start_is_best"] = finish("start_is_best", params(0, 1, 1, 8), "bowl", near)
    # edge: blocks in the picture's corners whose start lies on their limits: sites rejected by is_mv_in, sub-pel sites out of range
    edge = []
    for k, (w, h) in enumerate(SIZES):
        for org in ((0, 0), (PIC_W - w, PIC_H - h)):
            lim = mv_limits(org, w, h)
            s = (lim[2] * 8, lim[0] * 8) if org == (0, 0) else (lim[3] * 8, lim[1] * 8)
            edge.append(make_job(ref, org, w, h, s, s, s, seed=30 + k))
    out["edge"] = finish("edge", params(0, 0, 1, 8), "smooth", edge)
    out["edge_subpel"] = finish("edge_subpel", params(2, 1, 0, 8), "smooth", edge)
    # tie: a reference that is a V of columns, mirror-symmetric about the block's middle, under a flat bright source without neighbours: the sites to
    # the left and to the right gain the same, and the rate is the same (sadpb 0: no rate in the full-pel search): site order decides
    tie = [make_job(ref_plane("vee"), (100 - w // 2, 40), w, h, (0, 0), (0, 0), (0, 0), neighbours=False, src_const=255) for w, h in SIZES]
    out["tie"] = finish("tie", params(0, 0, 0, 8, 1, sadpb=0), "vee", tie)
    # cost: a displacement of one sample whose gain in SAD is smaller than what the rate asks for it
    cost = [make_job(ref, (40 + 8 * k, 32), 8, 8, (8, 8 * (k % 3 - 1)), (0, 0), (0, 0), noise=1, seed=40 + k) for k in range(12)]
    out["cost"] = finish("cost", params(0, 0, 0, 8, 1, sadpb=2500), "smooth", cost)
    # phases: every 1/8 displacement from a full-pel start: the rounds move, the diagonal wins, a second-level check wins
    for (w, h) in ((8, 8), (16, 8)):
        ph = [make_job(ref, (48, 40), w, h, (8 + (q >> 3), -16 + (q & 7)), (8, -16), (8, -16), seed=50 + q) for q in range(64)]
        out[f"phases_{w}x{h}"] = finish(f"phases_{w}x{h}", params(4, 1, 0, 8, 1), "smooth", ph)
    return out


@functools.lru_cache(maxsize=None)
def batches():
    out = {b["name"]: b for b in (grid_batch(*g) for g in GRID)}
    out.update(planted_batches())
    return out


@functools.lru_cache(maxsize=None)
def restated(name):
    """(best_mv [n][2], results, events) of a batch; every job of the case lists is defined"""
    b = batches()[name]
    ref, tables = ref_plane(b["ref"]), cost_tables()
    res = [restate_job(b["params"], ref, b["wsrc"], b["mask"], j, tables) for j in b["jobs"]]
    assert all(r is not None for r in res), name
    return np.array([r[0] for r in res], np.int16), np.array([r[1] for r in res], RESULT_DTYPE), [r[2] for r in res]


def planted_missing():
    """the conditions of the planted inputs that the restatement's events do not show, as text"""
    ev = {n: restated(n)[2] for n in planted_batches()}
    mv = {n: restated(n)[0] for n in planted_batches()}
    b = batches()
    miss = []
    if not all(e["fp_steps"] == 8 and e["fp_stop"] == "range" for e in ev["far_8"]):
        miss.append("far_8: not every search moves 8 steps and is stopped by search_range")
    if not all(e["fp_steps"] > 8 for e in ev["far_16_diag"]):
        miss.append("far_16_diag: not every search moves for more than 8 steps")
    if not all(e["fp_steps"] == 0 and e["fp_stop"] == "none" and not any(e["sp_moved"]) for e in ev["start_is_best"]) or \
            not np.array_equal(mv["start_is_best"], b["start_is_best"]["jobs"]["start_mv"]):
        miss.append("start_is_best: a search moves")
    if not all(e["fp_rejected"] for e in ev["edge"]):
        miss.append("edge: a job without a site rejected by is_mv_in")
    if not all(e["sp_out_of_range"] for e in ev["edge_subpel"]):
        miss.append("edge_subpel: a job without a site out of the sub-pel range")
    if not all(e["fp_tie"] and e["fp_steps"] >= 1 for e in ev["tie"]) or not all(m[1] < 0 for m in mv["tie"]):
        miss.append("tie: no tie between two sites, or the later site won")
    if not any(e["fp_cost_rejects"] and e["fp_steps"] == 0 for e in ev["cost"]):
        miss.append("cost: no site with sad < best whose sad + cost is not")
    for n in ("phases_8x8", "phases_16x8"):
        if not (any(all(e["sp_moved"]) for e in ev[n]) and all(any(e["sp_moved"][r] for e in ev[n]) for r in range(3))):
            miss.append(f"{n}: a sub-pel round never moves")
        if not any(e["sp_diag_won"] for e in ev[n]) or not any(e["sp_second_won"] for e in ev[n]):
            miss.append(f"{n}: the diagonal or a second-level check never wins")
    return miss


UNDEFINED_KINDS = ["size", "target_end", "ref_before", "ref_before_by_one", "ref_after", "ref_after_by_one"]


def undefined_batch():
    """ordinary jobs with one undefined job of every kind among them: (batch, {kind: job index})"""
    ref = ref_plane()
    items, bad = [], {}
    for k, kind in enumerate(UNDEFINED_KINDS):
        items += [make_job(ref, (32 + 16 * k, 40), 16, 8, (10, -6), (0, 0), (3, 3), seed=60 + k), make_job(ref, (48, 48), 8, 8, (-9, 12), (8, 8), (0, 0), seed=70 + k)]
        bad[kind] = len(items)
        items.append(make_job(ref, (64, 64), 16, 16, (5, 5), (0, 0), (0, 0), seed=80 + k))
    b = finish("undefined", params(0, 0, 1, 8), "smooth", items)
    j = b["jobs"]
    j[bad["size"]]["width"] = 12
    j[bad["target_end"]]["target_offset"] = len(b["wsrc"]) - 16 * 16 + 1
    # range 8: 13 rows and columns before the co-located block (8 + 2 of sub-pel movement + 3 taps), 13 after it (8 + 1 + 4)
    s = ref.shape[1]
    j[bad["ref_before"]]["ref_offset"] = 11 * s
    j[bad["ref_before_by_one"]]["ref_offset"] = 13 * s + 12             # the guard's first sample is one before the buffer ...
    j[bad["ref_before_by_one"] - 2]["ref_offset"] = 13 * s + 13         # ... and the job two before it starts exactly at the buffer: defined
    j[bad["ref_after"]]["ref_offset"] = ref.size - (16 + 12) * s
    j[bad["ref_after_by_one"]]["ref_offset"] = ref.size - (15 + 13) * s - (15 + 13)       # 16 x 16: the guard's last sample is one past the end ...
    j[bad["ref_after_by_one"] - 2]["ref_offset"] = ref.size - 1 - (7 + 13) * s - (15 + 13)  # ... and this 16 x 8 job's is the buffer's last: defined
    return b, bad
