"""Coefficient rate estimation of the mode decision, restated in numpy / Python integers, and the case lists of its tests.  Reference
(Source/Lib):
  svt_av1_cost_coeffs_txb (allow_update_cdf == 0)     Codec/rd_cost.c:434-559
  svt_av1_txb_init_levels_c                           Codec/rd_cost.c:99-111
  svt_av1_get_nz_map_contexts_c                       C_DEFAULT/encode_txb_ref_c.c:17-40
  get_nz_mag, get_nz_map_ctx_from_stats               Codec/coefficients.h:2884-2943
  get_br_ctx                                          Codec/common_utils.h:114-151
  get_eob_cost, get_eob_pos_token                     Codec/rd_cost.c:281-298,188-201
  av1_transform_type_rate_estimation                  Codec/rd_cost.c:113-158
  av1_cost_coeffs_txb_loop_cost_eob                   Codec/rd_cost.c:339-431
  svt_aom_txb_estimate_coeff_bits (the luma frame)    Codec/rd_cost.c:1405-1450
  the short-cuts of tx_type_search, RDCOST            Codec/product_coding_loop.c:4947-4952, Codec/rd_cost.h:37
The fixture (golden/coeff_rate.npz, written by tools/gen_coeff_rate_golden.py) holds the reference's own tables and its results on CASES."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coeff_rate.npz")

TX_W = [4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64]
TX_H = [4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16]
N_TX_SIZES = 19
SQR_MAP = [0, 1, 2, 3, 4, 0, 0, 1, 1, 2, 2, 3, 3, 0, 0, 1, 1, 2, 2]        # txsize_sqr_map, Codec/definitions.h:1509
SQR_UP_MAP = [0, 1, 2, 3, 4, 1, 1, 2, 2, 3, 3, 4, 4, 2, 2, 3, 3, 4, 4]     # txsize_sqr_up_map, :1530
LOG2_MINUS4 = [0, 2, 4, 6, 6, 1, 1, 3, 3, 5, 5, 6, 6, 2, 2, 4, 4, 5, 5]    # txsize_log2_minus4, Codec/inv_transforms.h:329
NUM_BASE_LEVELS, COEFF_BASE_RANGE, COST_LITERAL = 2, 12, 512
UNDEFINED = 0xFFFFFFFFFFFFFFFF
NO_JOB = 0xFFFFFFFF

# LvMapCoeffCost as 970 int32 (Codec/md_rate_estimation.h:41-49): member -> (first element, shape)
COEFF_MEMBERS = {"txb_skip_cost": (0, (13, 2)), "base_eob_cost": (26, (4, 3)), "base_cost": (38, (42, 8)), "eob_extra_cost": (374, (22, 2)),
                 "dc_sign_cost": (418, (3, 2)), "lps_cost": (424, (21, 26))}
COEFF_COST_INTS = 970
TABLE_SHAPES = {"coeff_fac_bits": (5, 2, COEFF_COST_INTS), "eob_frac_bits": (7, 2, 2, 11), "intra_tx_type_fac_bits": (3, 4, 13, 17),
                "inter_tx_type_fac_bits": (4, 4, 17)}  # the members of MdRateEstimationContext the function reads, in their order (:127-133)
QINDEXES = (40, 200)  # two classes of svt_av1_default_coef_probs

# TxSetType (Codec/definitions.h:1029-1039): DCTONLY, DCT_IDTX, DTT4_IDTX, DTT4_IDTX_1DDCT, DTT9_IDTX_1DDCT, ALL16
NUM_EXT_TX_SET = [1, 2, 5, 7, 12, 16]
EXT_TX_USED = [[1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0],
               [1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0],
               [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0], [1] * 16]
EXT_TX_SET_INDEX = [[0, -1, 2, 1, -1, -1], [0, 3, -1, -1, 2, 1]]
RATE_VARIANTS = [(f, s) for s in (0, 1, 2) for f in (1, 2, 4)]  # (mds_fast_coeff_est_level, mds_subres_step)
MAGNITUDES = (1, 2, 3, 14, 15, 127, 128, 1000, 30000)


def packed_dims(tx_size):
    return min(TX_W[tx_size], 32), min(TX_H[tx_size], 32)


def tx_class(tx_type):
    """tx_type_to_class (Codec/cabac_context_model.h:459): 0 2-D, 1 horizontal (H_*), 2 vertical (V_*)"""
    return 0 if tx_type < 10 else (1 if tx_type & 1 else 2)


def ext_tx_set_type(tx_size, is_inter, reduced):
    """get_ext_tx_set_type (Codec/definitions.h:1787-1802)"""
    up = SQR_UP_MAP[tx_size]
    if up > 3:
        return 0
    if up == 3:
        return 1 if is_inter else 0
    if reduced:
        return 1 if is_inter else 2
    if is_inter:
        return 4 if SQR_MAP[tx_size] == 2 else 5
    return 2 if SQR_MAP[tx_size] == 2 else 3


def scan_order(tx_size, tx_type):
    """av1_scan_orders[tx_size][tx_type].scan on the packed block: the diagonal scan for the 2-D types (zig-zag on squares, one direction on
    rectangles), rows for V_*, columns for H_*"""
    w, h = packed_dims(tx_size)
    cls = tx_class(tx_type)
    if cls == 2:
        return np.arange(w * h, dtype=np.int32)
    if cls == 1:
        return np.array([r * w + c for c in range(w) for r in range(h)], np.int32)
    out = []
    for d in range(w + h - 1):
        down = 1 if w < h else (0 if w > h else d & 1)
        for i in range(d + 1):
            r = i if down else d - i
            c = d - r
            if r < h and c < w:
                out.append(r * w + c)
    return np.array(out, np.int32)


class Tables:
    """the four table members as int32 arrays of TABLE_SHAPES"""

    def __init__(self, **members):
        for name, shape in TABLE_SHAPES.items():
            a = np.ascontiguousarray(members[name], np.int32)
            assert a.shape == shape, (name, a.shape)
            setattr(self, name, a)

    @classmethod
    def from_golden(cls, z, k):
        return cls(**{name: z[f"{name}_{k}"] for name in TABLE_SHAPES})

    def coeff_costs(self, tx_size, plane):
        flat = self.coeff_fac_bits[(SQR_MAP[tx_size] + SQR_UP_MAP[tx_size] + 1) >> 1][plane]
        return {m: flat[o:o + int(np.prod(s))].reshape(s) for m, (o, s) in COEFF_MEMBERS.items()}

    def to_bytes(self):
        """the layout of SvtHipRateTables"""
        return b"".join(getattr(self, name).tobytes() for name in TABLE_SHAPES)


def eob_pos_token(eob):
    """get_eob_pos_token (rd_cost.c:188-201): (token, extra)"""
    if eob < 33:
        t = [0, 1, 2, 3, 3, 4, 4, 4, 4][eob] if eob < 9 else (5 if eob < 17 else 6)
    else:
        t = [6, 7, 8, 8, 9, 9, 9, 9, 10, 10, 10, 10, 10, 10, 10, 10, 11][min((eob - 1) >> 5, 16)]
    return t, eob - [0, 1, 2, 3, 5, 9, 17, 33, 65, 129, 257, 513][t]


def eob_cost(T, cc, tx_size, plane, eob, cls):
    """get_eob_cost (rd_cost.c:281-298)"""
    pt, extra = eob_pos_token(eob)
    cost = int(T.eob_frac_bits[LOG2_MINUS4[tx_size]][plane][0 if cls == 0 else 1][pt - 1])
    offset_bits = [0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9][pt]
    if offset_bits > 0:
        bit = 1 if extra & (1 << (offset_bits - 1)) else 0
        cost += int(cc["eob_extra_cost"][pt - 3][bit])
        if offset_bits > 1:
            cost += COST_LITERAL * (offset_bits - 1)
    return cost


def tx_type_rate(T, tx_size, tx_type, is_inter, intra_dir, reduced):
    """av1_transform_type_rate_estimation (rd_cost.c:113-158); intra_dir is already resolved through fimode_to_intradir"""
    st = ext_tx_set_type(tx_size, is_inter, reduced)
    if NUM_EXT_TX_SET[st] <= 1:
        return 0
    s = EXT_TX_SET_INDEX[1 if is_inter else 0][st]
    if s <= 0:
        return 0
    if is_inter:
        return int(T.inter_tx_type_fac_bits[s][SQR_MAP[tx_size]][tx_type])
    return int(T.intra_tx_type_fac_bits[s][SQR_MAP[tx_size]][intra_dir][tx_type])


def golomb_cost(level):
    """get_golomb_cost (rd_cost.c:90-97), vectorised"""
    r = np.maximum(level - COEFF_BASE_RANGE - NUM_BASE_LEVELS, 1).astype(np.int64)
    length = np.floor(np.log2(r)).astype(np.int64) + 1  # r < 2^31: exact in fp64
    return np.where(level >= 1 + NUM_BASE_LEVELS + COEFF_BASE_RANGE, COST_LITERAL * (2 * length - 1), 0)


def block_contexts(q, tx_size, cls):
    """Per raster position of the packed block: (coefficient context of a position that is not the last, br context, |q|).  The levels array
    is the whole block clamped to 127 in a zero frame (svt_av1_txb_init_levels_c); get_nz_mag / get_nz_map_ctx_from_stats / get_br_ctx."""
    w, h = packed_dims(tx_size)
    a = np.abs(q.astype(np.int64)).reshape(h, w)
    lv = np.zeros((h + 4, w + 4), np.int64)
    lv[:h, :w] = np.minimum(a, 127)
    c3 = np.minimum(lv, 3)
    at = lambda m, dy, dx: m[dy:dy + h, dx:dx + w]
    mag = at(c3, 0, 1) + at(c3, 1, 0)
    br = at(lv, 0, 1) + at(lv, 1, 0)
    row, col = np.mgrid[0:h, 0:w]
    if cls == 0:
        mag = mag + at(c3, 1, 1) + at(c3, 0, 2) + at(c3, 2, 0)
        br = br + at(lv, 1, 1)
        near = (row < 2) & (col < 2)
        tw, th = TX_W[tx_size], TX_H[tx_size]
        off = np.where(row + col < 2, 1, np.where(row + col < 4, 6, 21))  # the rule behind eb_av1_nz_map_ctx_offset (coefficients.h:2918-2928)
        if tw < th:
            off = np.where(row < 2, 11, off)
        elif tw > th:
            off = np.where(col < 2, 16, off)
    elif cls == 1:
        mag = mag + at(c3, 0, 2) + at(c3, 0, 3) + at(c3, 0, 4)
        br = br + at(lv, 0, 2)
        near = col == 0
        off = np.where(col == 0, 26, np.where(col == 1, 31, 36))  # nz_map_ctx_offset_1d
    else:
        mag = mag + at(c3, 2, 0) + at(c3, 3, 0) + at(c3, 4, 0)
        br = br + at(lv, 2, 0)
        near = row == 0
        off = np.where(row == 0, 26, np.where(row == 1, 31, 36))
    ctx = np.minimum((mag + 1) >> 1, 4) + off
    if cls == 0:
        ctx[0, 0] = 0
    br = np.minimum((br + 1) >> 1, 6)
    br = br + np.where(near, 7, 14)
    br[0, 0] -= 7 if near[0, 0] else 14
    return ctx.reshape(-1), br.reshape(-1), a.reshape(-1)


def cost_coeffs_txb(T, tx_size, plane, q, eob, job, reduced, variants=((1, 0),), stats=None):
    """svt_av1_cost_coeffs_txb for every (mds_fast_coeff_est_level, mds_subres_step) of `variants`: a list of costs, or None where the
    reference is undefined (eob of 0 or above the coefficient count, a zero coefficient at scan[eob - 1], a context outside its table;
    intra_dir is read, and so checked, for intra luma jobs only: an inter candidate's pred_mode is 13 or above).
    job: (tx_type, txb_skip_ctx, dc_sign_ctx, is_inter, intra_dir).  stats: optional dict of sets / counters of what was read."""
    tx_type, skip_ctx, dc_ctx, is_inter, intra_dir = (int(v) for v in job)
    w, h = packed_dims(tx_size)
    n = w * h
    q = np.asarray(q, np.int64).reshape(-1)
    if tx_type >= 16 or skip_ctx >= 13 or dc_ctx >= 3 or (plane == 0 and not is_inter and intra_dir >= 13) or eob < 1 or eob > n:
        return None
    cls = tx_class(tx_type)
    scan = scan_order(tx_size, tx_type)
    last = int(scan[eob - 1])
    if q[last] == 0:
        return None
    cc = T.coeff_costs(tx_size, plane)
    cost = int(cc["txb_skip_cost"][skip_ctx][0])
    if plane == 0:
        cost += tx_type_rate(T, tx_size, tx_type, is_inter, intra_dir, reduced)
    cost += eob_cost(T, cc, tx_size, plane, eob, cls)
    dc = int(q[0])
    if eob == 1:  # av1_cost_coeffs_txb_loop_cost_one_eob
        lvl = abs(dc)
        cost += int(cc["base_eob_cost"][0][min(lvl, 3) - 1]) + int(cc["dc_sign_cost"][dc_ctx][1 if dc < 0 else 0])
        if lvl > NUM_BASE_LEVELS:
            cost += int(cc["lps_cost"][0][min(lvl - 1 - NUM_BASE_LEVELS, COEFF_BASE_RANGE)]) + int(golomb_cost(np.int64(lvl)))
        if stats is not None:
            stats["base_eob"].add(0)
            stats["nonzero"] += 1
            if lvl > NUM_BASE_LEVELS:
                stats["lps"].add(0)
                stats["golomb"] += int(lvl >= 15)
        return [cost] * len(variants)
    ctx, br, a = block_contexts(q, tx_size, cls)
    lps = lambda pos: int(cc["lps_cost"][br[pos]][min(int(a[pos]) - 1 - NUM_BASE_LEVELS, COEFF_BASE_RANGE)]) + int(golomb_cost(a[pos]))
    # the last coefficient of the scan
    eob_ctx = 1 if eob - 1 <= n // 8 else (2 if eob - 1 <= n // 4 else 3)
    cost += int(cc["base_eob_cost"][eob_ctx][min(int(a[last]), 3) - 1]) + COST_LITERAL
    if a[last] > NUM_BASE_LEVELS:
        cost += lps(last)
    # the DC
    cost += int(cc["base_cost"][ctx[0]][min(int(a[0]), 3)])
    if dc != 0:
        cost += int(cc["dc_sign_cost"][dc_ctx][1 if dc < 0 else 0])
        if a[0] > NUM_BASE_LEVELS:
            cost += lps(0)
    # the middle loop, c = c_start .. 1: a prefix sum over the scan index
    mid = scan[1:eob - 1]
    am = a[mid]
    big = am > NUM_BASE_LEVELS
    term = cc["base_cost"][ctx[mid], np.minimum(am, 3)].astype(np.int64) + np.where(am != 0, COST_LITERAL, 0)
    term += np.where(big, cc["lps_cost"][br[mid], np.clip(am - 1 - NUM_BASE_LEVELS, 0, COEFF_BASE_RANGE)] + golomb_cost(am), 0)
    cum = np.concatenate([[0], np.cumsum(term)])
    out = []
    for fast, subres in variants:
        c_start = min(eob - 2, eob // max(1, fast - subres))
        out.append(cost + int(cum[c_start]))
    if stats is not None:
        c_min = min(min(eob - 2, eob // max(1, f - s)) for f, s in variants)
        stats["short_loop"] |= c_min < eob - 2
        stats["base_eob"].add(eob_ctx)
        stats["base"].update([int(ctx[0])] + ctx[mid].tolist())
        read = [p for p in [last, 0] + mid.tolist() if a[p] > NUM_BASE_LEVELS]
        stats["lps"].update(br[read].tolist())
        nz = [p for p in [last, 0] + mid.tolist() if a[p] != 0]
        stats["nonzero"] += len(nz)
        stats["golomb"] += int(np.sum(a[nz] >= 15))
    return out


def new_stats():
    return {"base": set(), "base_eob": set(), "lps": set(), "nonzero": 0, "golomb": 0, "short_loop": False}


def shortcut_threshold(tx_size):
    return (TX_W[tx_size] * TX_H[tx_size]) >> 6  # the real transform dimensions (product_coding_loop.c:4947)


def frame_bits(T, tx_size, plane, raw, eob, skip_ctx, coeff_rate_est_lvl, subres):
    """What the caller makes of svt_av1_cost_coeffs_txb's result `raw` (None: undefined): the two short-cuts of tx_type_search (luma only,
    product_coding_loop.c:4947-4952), else svt_aom_txb_estimate_coeff_bits' frame (rd_cost.c:1429-1450)."""
    if plane == 0:
        if coeff_rate_est_lvl != 1 and eob < shortcut_threshold(tx_size):
            return 6000 + eob * 1000
        if coeff_rate_est_lvl == 0:
            return 3000 + eob * 100
    if eob == 0:
        return UNDEFINED if skip_ctx >= 13 else int(T.coeff_costs(tx_size, plane)["txb_skip_cost"][skip_ctx][1])
    if raw is None:
        return UNDEFINED
    return (raw << subres) if plane == 0 else raw


def rdcost(lam, bits, dist):
    """RDCOST (Codec/rd_cost.h:37) in 64-bit wrapping arithmetic"""
    if bits == UNDEFINED:
        return UNDEFINED
    return (((bits * lam + 256) >> 9) + (dist << 7)) & UNDEFINED


def group_winners(cost, group_start):
    """the first strict minimum of every group in job order (tx_type_search, product_coding_loop.c:4976-4985): (best_job, best_cost)"""
    jobs, best = [], []
    for g in range(len(group_start) - 1):
        bj, bc = NO_JOB, UNDEFINED
        for j in range(int(group_start[g]), int(group_start[g + 1])):
            if int(cost[j]) < bc:
                bj, bc = j, int(cost[j])
        jobs.append(bj)
        best.append(bc)
    return np.array(jobs, np.uint32), np.array(best, np.uint64)


def run_case(T, case, coeff_rate_est_lvl=1, variants=RATE_VARIANTS, stats=None):
    """(raw [len(variants)][n] as Python ints or None, bits [len(variants)][n] uint64) of a case"""
    ts, pl, red = case["tx_size"], case["plane"], case["reduced"]
    raws = [cost_coeffs_txb(T, ts, pl, q, int(e), tuple(j)[:5], red, variants, stats) if e else None
            for q, e, j in zip(case["qcoeff"], case["eob"], case["jobs"])]
    raw = [[None if r is None else r[v] for r in raws] for v in range(len(variants))]
    bits = np.array([[frame_bits(T, ts, pl, r, int(e), int(j["txb_skip_ctx"]), coeff_rate_est_lvl, sub) for r, e, j in zip(raw[v], case["eob"], case["jobs"])]
                     for v, (_, sub) in enumerate(variants)], np.uint64)
    return raw, bits


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
RATE_JOB_DTYPE = [("tx_type", "u1"), ("txb_skip_ctx", "u1"), ("dc_sign_ctx", "u1"), ("is_inter", "u1"), ("intra_dir", "u1"), ("reserved", "u1", (3,))]


def eob_grid(n):
    return sorted({e for e in (0, 1, 2, 3, n // 8, n // 8 + 1, n // 4, n // 4 + 1, n - 1, n) if 0 <= e <= n})


def class_types(tx_size, is_inter, reduced, rng):
    """one tx_type of every TxClass the size's set admits (av1_ext_tx_used); DCT_DCT first"""
    used = EXT_TX_USED[ext_tx_set_type(tx_size, is_inter, reduced)]
    out = [0]
    two_d = [t for t in range(1, 10) if used[t]]
    if two_d:
        out.append(int(rng.choice(two_d)))
    for cls in (1, 2):
        ts = [t for t in range(10, 16) if used[t] and tx_class(t) == cls]
        if ts:
            out.append(int(rng.choice(ts)))
    return out


def make_block(rng, tx_size, tx_type, eob, dense, k):
    """a packed coefficient block with `eob` scan positions in use.  dense: every position below eob holds a level >= 3 (every neighbour
    sum saturates); else about a third of them are non-zero.  The last, the DC and a middle position take magnitudes of MAGNITUDES in
    turn (by `k`); every seventh block also has non-zero coefficients behind eob, which the levels array sees like the reference's."""
    w, h = packed_dims(tx_size)
    n = w * h
    q = np.zeros(n, np.int64)
    scan = scan_order(tx_size, tx_type)
    if eob:
        pos = scan[:eob]
        if dense:
            lv = rng.choice([3, 4, 5, 6, 9, 14, 15, 16, 40], size=eob, p=[.3, .2, .12, .1, .08, .05, .05, .05, .05])
        else:
            lv = rng.choice([0, 1, 2, 3, 5, 15, 200], size=eob, p=[.66, .14, .08, .05, .03, .02, .02])
        q[pos] = lv * rng.choice([-1, 1], size=eob)
        q[scan[eob - 1]] = MAGNITUDES[k % 9] * (1 if rng.integers(2) else -1)
        if eob >= 2:
            q[0] = MAGNITUDES[(k // 9 + k) % 9] * (1 if k & 1 else -1)
            if dense == 0 and k % 5 == 0:
                q[0] = 0
        if eob >= 3:
            q[scan[eob // 2]] = MAGNITUDES[(k // 3 + 2 * k) % 9] * (1 if rng.integers(2) else -1)
    if k % 7 == 3 and eob < n:
        tail = scan[eob:]
        sel = tail[rng.random(len(tail)) < 0.2]
        q[sel] = rng.integers(1, 9, len(sel)) * rng.choice([-1, 1], size=len(sel))
    return q.astype(np.int32)


def build_case(tx_size, plane, reduced, seed=20261017):
    rng = np.random.default_rng([seed, tx_size, plane, reduced])
    w, h = packed_dims(tx_size)
    jobs, blocks, eobs = [], [], []
    k = 0
    for is_inter in (0, 1):
        for tx_type in class_types(tx_size, is_inter, reduced, rng):
            for eob in eob_grid(w * h):
                for dense in ((0, 1) if eob >= 2 else (0,)):
                    jobs.append((tx_type, int(rng.integers(13)), int(rng.integers(3)), is_inter, int(rng.integers(13)), (0, 0, 0)))
                    blocks.append(make_block(rng, tx_size, tx_type, eob, dense, k))
                    eobs.append(eob)
                    k += 1
    return {"tx_size": tx_size, "plane": plane, "reduced": reduced, "table": (tx_size + plane + reduced) & 1,
            "jobs": np.array(jobs, dtype=RATE_JOB_DTYPE), "qcoeff": np.stack(blocks), "eob": np.array(eobs, np.uint16)}


CASE_KEYS = [(ts, pl, red) for ts in range(N_TX_SIZES) for (pl, red) in ((0, 0), (0, 1), (1, 0))]


def build_cases():
    return [build_case(*key) for key in CASE_KEYS]


def cases_to_arrays(cases):
    """the cases as the flat arrays the fixture stores"""
    return {"case_meta": np.array([(c["tx_size"], c["plane"], c["reduced"], c["table"], len(c["jobs"])) for c in cases], np.int32),
            "jobs": np.concatenate([c["jobs"] for c in cases]).view(np.uint8).reshape(-1, 8),
            "eob": np.concatenate([c["eob"] for c in cases]),
            "qcoeff": np.concatenate([c["qcoeff"].reshape(-1) for c in cases])}


def cases_from_arrays(z):
    out, j0, q0 = [], 0, 0
    jobs = np.ascontiguousarray(z["jobs"]).view(RATE_JOB_DTYPE).reshape(-1)
    for ts, pl, red, tab, n in z["case_meta"].tolist():
        w, h = packed_dims(ts)
        c = {"tx_size": ts, "plane": pl, "reduced": red, "table": tab, "jobs": jobs[j0:j0 + n], "eob": z["eob"][j0:j0 + n],
             "qcoeff": z["qcoeff"][q0:q0 + n * w * h].reshape(n, w * h), "first_job": j0}
        out.append(c)
        j0, q0 = j0 + n, q0 + n * w * h
    return out


def undefined_case(tx_size, seed=5):
    """jobs the reference leaves undefined among ordinary ones: eob above the coefficient count, a zero coefficient at scan[eob - 1], a context
    or a tx_type outside its range, an intra luma job with intra_dir 13.  (case, the indices of the undefined jobs)"""
    c = build_case(tx_size, 0, 0, seed)
    w, h = packed_dims(tx_size)
    n = w * h
    c["eob"] = c["eob"].copy()
    c["jobs"] = c["jobs"].copy()
    ok = [i for i in range(len(c["jobs"])) if c["eob"][i] >= 2]
    bad = ok[1:len(ok) - 1:3][:8]
    kinds = []
    for m, i in enumerate(bad):
        kind = m % 7
        if kind == 0:
            c["eob"][i] = n + 1
        elif kind == 1:
            c["eob"][i] = 65535
        elif kind == 2:
            c["qcoeff"][i, scan_order(tx_size, int(c["jobs"][i]["tx_type"]))[int(c["eob"][i]) - 1]] = 0
        elif kind == 3:
            c["jobs"][i]["txb_skip_ctx"] = 13
        elif kind == 4:
            c["jobs"][i]["dc_sign_ctx"] = 3
        elif kind == 5:
            c["jobs"][i]["tx_type"] = 16
        else:
            c["jobs"][i]["is_inter"], c["jobs"][i]["intra_dir"] = 0, 13
        kinds.append(kind)
    return c, bad


def with_inter_pred_modes(case):
    """the case with intra_dir as a host that copies cand->pred_mode unconditionally fills it: 13 .. 24 (NEARESTMV .. NEW_NEWMV) on the inter jobs
    and, for a chroma case, out-of-range values on every job.  The reference does not read it there, so its results do not change."""
    c = dict(case)
    c["jobs"] = case["jobs"].copy()
    sel = np.ones(len(c["jobs"]), bool) if case["plane"] else c["jobs"]["is_inter"] != 0
    c["jobs"]["intra_dir"][sel] = (13 + np.arange(len(c["jobs"])) % 12)[sel]
    if case["plane"]:
        c["jobs"]["intra_dir"][::5] = 255
    return c
