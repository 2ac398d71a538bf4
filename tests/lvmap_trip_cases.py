"""The rate and RDOQ batches (svt_hip_coeff_rate_batch, svt_hip_rdoq_batch) past one trip of their capped grid: the launch plan restated, and
the builders that turn a fixture case into a batch whose waves take several packs in turn.

Both kernels launch `grid` workgroups (at most the cap) of K_WAVES waves.  A wave holds JPW jobs (a pack: four jobs of 16 coefficients, two of
32, one of any other size) and walks the packs wave-strided: pack = workgroup * K_WAVES + wave, then + grid * K_WAVES per trip.  With
job = pack * JPW + group, the group of lanes that takes job j is WAVE SLOT j % S on TRIP j // S, S = grid * K_WAVES * JPW: the jobs a slot meets
on consecutive trips are j, j + S, j + 2 S, ...  Everything a wave could carry from one job into the next (its levels array and decisions in
LDS, the registers of the job frame) travels along that sequence, so the builders here decide what stands S jobs apart.

The restatements (rdoq_cases.run_case, coeff_rate_cases.run_case) work job by job, so the expectation of a re-ordered or repeated batch is the
re-ordered or repeated expectation; tests/test_lvmap_trips.py checks that too."""
import numpy as np

import coeff_rate_cases as cr
import rdoq_cases as rq

K_WAVES, MAX_GRID = 4, 2048
GRIDS = (1, 2)  # the caps the small batches run under
RDOQ_JOB_KEYS, RATE_JOB_KEYS = ("jobs", "coeff"), ("jobs", "qcoeff", "eob")  # the per-job arrays of a case


def plan(tx_size, n_jobs, max_grid=0):
    """(grid, n_packs, jobs per pack) of a batch under the cap max_grid (0: the default): svt_hip_lvmap_plan restated"""
    w, h = cr.packed_dims(tx_size)
    jpw = max(1, 64 // (w * h))
    n_packs = -(-n_jobs // jpw)
    return min(-(-n_packs // K_WAVES), max_grid or MAX_GRID), n_packs, jpw


def slots_of(p):
    """the wave slots of a plan: jobs taken per trip"""
    return p[0] * K_WAVES * p[2]


def trips_of(p):
    """the trips of the busiest wave of a plan"""
    return -(-p[1] // (p[0] * K_WAVES)) if p[0] else 0


def take(d, order, keys=None):
    """a dict with its per-job arrays (`keys`, default all) in another order; `order` may repeat jobs"""
    out = dict(d)
    for k in (list(d) if keys is None else keys):
        out[k] = d[k][order]
    return out


def tiled(n_case, n_jobs, tx_size, max_grid=0):
    """the job indices of a case of n_case jobs repeated up to n_jobs.  The period is no divisor of the wave slots, so the job a slot meets on one
    trip is not the one it met on the trip before; a case whose length fails that gives up its last job."""
    s = slots_of(plan(tx_size, n_jobs, max_grid))
    period = n_case if s % n_case else n_case - 1
    assert period > 0 and s % period != 0, (s, n_case)
    return np.arange(n_jobs) % period


# ---- what a job is to a wave ---------------------------------------------------------------------------------------------------------------
RDOQ_LIGHT = ("eob0", "eob1", "gated", "undefined", "eob_gt_n")
RATE_LIGHT = ("shortcut", "eob0", "skip_ctx", "tx_type")


def rdoq_kinds(c, inp, want, n_base):
    """One of "heavy", RDOQ_LIGHT or "other" per job.  heavy: optimised, an eob in the top quartile of those of the case's first n_base jobs
    that reach the optimiser (which is no less than the top quartile of them all, and still leaves some where the eob_th gate takes the longest),
    at least one level lowered and one coefficient zeroed.  Light: eob == 0, eob == 1, behind the eob_th gate, undefined, eob above the
    coefficient count."""
    n = c["coeff"].shape[1]
    eob = inp["eob"].astype(np.int64)
    top = np.percentile(eob[:n_base][want["status"][:n_base] == rq.ST_OPTIMISED], 75)
    kinds = []
    for i in range(len(eob)):
        qi, qo, st = inp["qcoeff"][i], want["qcoeff"][i], int(want["status"][i])
        if st == rq.ST_UNDEFINED:
            kinds.append("eob_gt_n" if eob[i] > n else "undefined")
        elif st == rq.ST_GATED:
            kinds.append("gated")
        elif eob[i] <= 1:
            kinds.append("eob0" if eob[i] == 0 else "eob1")
        elif st == rq.ST_OPTIMISED and eob[i] >= top and np.any((qo != 0) & (qo != qi)) and np.any((qi != 0) & (qo == 0)):
            kinds.append("heavy")
        else:
            kinds.append("other")
    return kinds


def rate_kinds(c, lvl):
    """One of "heavy", RATE_LIGHT or "other" per job at coeff_rate_est_lvl `lvl` (1 or 2).  heavy: the table path with an eob of the coefficient
    count or one below it and a level of 127 or more (the clamp of the levels array).  Light: a short-cut job (luma, eob < area >> 6), eob == 0,
    txb_skip_ctx >= 13, tx_type >= 16 -- tested in the kernel's order."""
    ts, n = c["tx_size"], c["qcoeff"].shape[1]
    kinds = []
    for q, e, j in zip(c["qcoeff"], c["eob"].astype(np.int64), c["jobs"]):
        if c["plane"] == 0 and lvl != 1 and e < cr.shortcut_threshold(ts):
            kinds.append("shortcut")
        elif j["txb_skip_ctx"] >= 13:
            kinds.append("skip_ctx")
        elif e == 0:
            kinds.append("eob0")
        elif j["tx_type"] >= 16:
            kinds.append("tx_type")
        elif n - 1 <= e <= n and np.max(np.abs(q)) >= 127 and j["dc_sign_ctx"] < 3 and q[cr.scan_order(ts, int(j["tx_type"]))[e - 1]] != 0 \
                and (c["plane"] or j["is_inter"] or j["intra_dir"] < 13):
            kinds.append("heavy")
        else:
            kinds.append("other")
    return kinds


def rdoq_light_kinds(c):
    """the light kinds a case can hold: the eob_th gate fires only where it is set and the longest block reaches it (no 64-point size does)"""
    ts, n = c["tx_size"], c["coeff"].shape[1]
    gate = n * 100 // (cr.TX_W[ts] * cr.TX_H[ts]) >= c["eob_th"]
    return tuple(kind for kind in RDOQ_LIGHT if kind != "gated" or gate)


def rate_light_kinds(c, lvl):
    """the light kinds a case can hold at coeff_rate_est_lvl `lvl`: where the short-cut exists (luma, not level 1, 64 pixels and more) it takes
    the jobs of eob 0"""
    cut = c["plane"] == 0 and lvl != 1 and cr.shortcut_threshold(c["tx_size"]) > 0
    return tuple(kind for kind in RATE_LIGHT if (kind == "shortcut") == cut or kind in ("skip_ctx", "tx_type"))


# ---- the fixture cases with the light kinds they lack ----------------------------------------------------------------------------------
_EXT = {}
MORE_LAMBDAS = (100000, 20000)  # between the fixture's: behind the eob_th gate the short TX_4X4 blocks are lowered AND cut at 100000 alone


def rdoq_extended(k):
    """Fixture case k of rdoq_cases.shared() with a handful of light jobs behind it: one of eob 0, one of eob 1 (the DC alone) and the seven
    spoiled ones of rdoq_cases.spoil, all made from the case's longest optimised job.  Where the case's lambda leaves no heavy job (64 changes
    nothing), the case takes the first of 6000, 400000, 1 << 24 and MORE_LAMBDAS that does: the expectations are the restatement's, not the
    fixture's.
    (case, inputs, kinds, the fixture's job count); computed once and kept unchanged."""
    if k not in _EXT:
        c0 = rq.shared()["cases"][k]
        inp0, want0, _ = rq.restated(k)
        n0 = len(c0["jobs"])
        ok = [i for i in range(n0) if want0["status"][i] == rq.ST_OPTIMISED and inp0["eob"][i] >= 2 and inp0["qcoeff"][i][0] != 0]
        src = max(ok, key=lambda i: int(inp0["eob"][i]))
        order = np.concatenate([np.arange(n0), np.full(2 + rq.SPOILS, src)])
        c = take(c0, order, RDOQ_JOB_KEYS)
        c.pop("ref")
        inp = {name: a[order].copy() for name, a in inp0.items()}
        c["jobs"], c["coeff"] = c["jobs"].copy(), c["coeff"].copy()
        for i, keep in ((n0, 0), (n0 + 1, 1)):  # eob 0: a block of zeros; eob 1: the DC alone
            for a in (c["coeff"], inp["qcoeff"], inp["dqcoeff"], inp["qcoeff_b"], inp["dqcoeff_b"]):
                a[i, keep:] = 0
            inp["eob"][i], inp["eob_b"][i] = keep, keep if inp["qcoeff_b"][i][0] else 0
        for m in range(rq.SPOILS):
            rq.spoil(c, inp, n0 + 2 + m, m)
        for a in [c["jobs"], c["coeff"]] + list(inp.values()):
            a.setflags(write=False)
        T = rq.shared()["tables"][c["table"]]
        for lam in [c0["lam"]] + [lam for lam in rq.LAMBDAS[1:] + MORE_LAMBDAS if lam != c0["lam"]]:
            c["lam"] = lam
            kinds = rdoq_kinds(c, inp, rq.run_case(T, c, inp, True), n0)
            if "heavy" in kinds:
                break
        else:
            raise AssertionError(f"fixture case {k}: no lambda leaves a heavy job")
        _EXT[k] = (c, inp, kinds, n0)
    return _EXT[k]


def rate_extended(c0):
    """A rate fixture case with two spoiled copies of its heaviest job behind it: txb_skip_ctx 13 and tx_type 16, as
    coeff_rate_cases.undefined_case spoils them.  (case, the fixture's job count)"""
    n0 = len(c0["jobs"])
    heavy = [i for i, kind in enumerate(rate_kinds(c0, 1)) if kind == "heavy"]
    order = np.concatenate([np.arange(n0), np.full(2, heavy[0])])
    c = take(c0, order, RATE_JOB_KEYS)
    c.pop("first_job", None)
    c["jobs"] = c["jobs"].copy()
    c["jobs"][n0]["txb_skip_ctx"], c["jobs"][n0 + 1]["tx_type"] = 13, 16
    return c, n0


# ---- the orders ------------------------------------------------------------------------------------------------------------------------------
MAX_HEAVY = 4  # the distinct heavy jobs of an order


def adversarial_order(kinds, light_kinds, slots, light_first=False, ragged=False):
    """Job indices (with repeats) in which every wave slot of `slots` meets heavy and light jobs in turn: the batch is a sequence of rows of
    `slots` jobs, one row per trip, all heavy or all light.  Every pair (light kind, heavy job) of light_kinds x the first MAX_HEAVY heavy jobs
    stands once as light -> heavy on some slot; the rows are L0 H0 L1 H1 .. L0 (light_first) or H L0 H0 L1 H1 .., so every light row but the
    first follows a heavy one.  ragged: the last job is left out (the last pack is then short where a pack holds several jobs)."""
    heavy = [i for i, kind in enumerate(kinds) if kind == "heavy"][:MAX_HEAVY]
    light = {kind: [i for i, have in enumerate(kinds) if have == kind] for kind in light_kinds}
    assert heavy and all(light.values()), (len(heavy), {kind: len(v) for kind, v in light.items()})
    pairs = [(kind, hv) for hv in heavy for kind in light_kinds]
    pairs += [pairs[i % len(pairs)] for i in range(-len(pairs) % slots)]
    used = {kind: 0 for kind in light_kinds}
    rows = []
    for r in range(0, len(pairs), slots):
        l_row = []
        for kind, _ in pairs[r:r + slots]:
            l_row.append(light[kind][used[kind] % len(light[kind])])  # the jobs of a kind in turn
            used[kind] += 1
        rows += [l_row, [hv for _, hv in pairs[r:r + slots]]]
    rows = rows + [rows[0]] if light_first else [rows[-1]] + rows
    order = np.array([i for row in rows for i in row], np.int64)
    return order[:-1] if ragged else order


def order_faults(kinds, order, light_kinds, slots):
    """What an order lacks, as a list of strings (empty: nothing): a pair of consecutive trips on a wave slot that is not heavy / light in turn,
    a light kind that never follows a heavy job, a heavy job that never follows one of the light kinds."""
    seq = [kinds[i] for i in order]
    bad, after_heavy, after_light = [], set(), set()
    for j in range(len(seq) - slots):
        a, b = seq[j], seq[j + slots]
        if a == "heavy" and b in light_kinds:
            after_heavy.add(b)
        elif a in light_kinds and b == "heavy":
            after_light.add((a, int(order[j + slots])))
        else:
            bad.append(f"slot {j % slots}, trips {j // slots} and {j // slots + 1}: {a} then {b}")
    bad += [f"{kind} never follows a heavy job" for kind in light_kinds if kind not in after_heavy]
    heavy = sorted({int(i) for i in order if kinds[i] == "heavy"})
    bad += [f"heavy job {hv} never follows {kind}" for hv in heavy for kind in light_kinds if (kind, hv) not in after_light]
    return bad


# ---- the batches of tests/test_lvmap_trips.py and tests/test_lvmap_trips_gpu.py ---------------------------------------------------------------
ORDER_SIZES = (0, 5, 1, 2, 4)  # TX_4X4 (four jobs per wave), TX_4X8 (two), TX_8X8, TX_16X16, TX_64X64
RATE_ORDER_SIZES = ORDER_SIZES + (3,)  # and TX_32X32: 256 coefficients and more are loaded 16 bytes at a time
RDOQ_ORDER_CASES = [(ts, name, fb) for ts in ORDER_SIZES for name, fb in (("plain", True), ("eob_th85", True), ("eob_th85", False), ("sharp", True))]
ORDERS = [(g, light_first) for g in GRIDS for light_first in (False, True)]
CAP_PACKS = MAX_GRID * K_WAVES  # the packs of one trip under the default cap
# the launches under the default cap: (tx_size, packs, jobs of the last pack)
PRODUCTION = [(0, 2 * CAP_PACKS + 1, 1), (5, 2 * CAP_PACKS + 1, 1), (1, CAP_PACKS, 1), (1, CAP_PACKS + 1, 1), (1, 2 * CAP_PACKS + 1, 1),
              (2, CAP_PACKS + 2 * K_WAVES + 1, 1), (4, CAP_PACKS + 2 * K_WAVES + 1, 1)]
SPARE = 8  # spare slots behind the large batches


def production_jobs(tx_size, n_packs, last):
    return (n_packs - 1) * plan(tx_size, 1)[2] + last


def rdoq_case(tx_size, name):
    """the index of a fixture case by size and variant name.  "plain": of plain_y and plain_uv the one whose restatement changes more
    coefficients (a lambda of 64 changes next to nothing)"""
    cases = rq.shared()["cases"]
    find = lambda v: next(k for k, c in enumerate(cases) if c["tx_size"] == tx_size and rq.VARIANTS[c["variant"]][0] == v)
    if name != "plain":
        return find(name)
    changed = lambda k: int(np.count_nonzero(rq.restated(k)[0]["qcoeff"] != rq.restated(k)[1]["qcoeff"]))
    return max((find("plain_y"), find("plain_uv")), key=changed)


def rdoq_ordered(k, max_grid, light_first):
    """rdoq_extended(k) in its adversarial order for the cap max_grid: (case, inputs, kinds, light kinds, order, wave slots)"""
    c, inp, kinds, _ = rdoq_extended(k)
    jpw = plan(c["tx_size"], 1)[2]
    slots, light = max_grid * K_WAVES * jpw, rdoq_light_kinds(c)
    order = adversarial_order(kinds, light, slots, light_first, ragged=jpw > 1)
    return take(c, order, RDOQ_JOB_KEYS), take(inp, order), kinds, light, order, slots


def rate_ordered(c0, lvl, max_grid, light_first):
    """rate_extended(c0) in its adversarial order at coeff_rate_est_lvl `lvl` for the cap max_grid: (case, kinds, light kinds, order, wave slots)"""
    c, _ = rate_extended(c0)
    jpw = plan(c["tx_size"], 1)[2]
    slots, kinds, light = max_grid * K_WAVES * jpw, rate_kinds(c, lvl), rate_light_kinds(c, lvl)
    order = adversarial_order(kinds, light, slots, light_first, ragged=jpw > 1)
    return take(c, order, RATE_JOB_KEYS), kinds, light, order, slots


def repeats_for_three_trips(tx_size, n_case):
    """how often a case of n_case jobs is repeated so that a cap of one workgroup gives its waves three trips"""
    reps = 1
    while trips_of(plan(tx_size, reps * n_case, 1)) < 3:
        reps += 1
    return reps


def ragged_groups(n_jobs, sizes=(1, 2, 3, 4, 5, 6, 7)):
    """group_start of groups whose sizes cycle through `sizes` over n_jobs jobs (the last one cut short)"""
    starts = [0]
    while starts[-1] < n_jobs:
        starts.append(min(n_jobs, starts[-1] + sizes[(len(starts) - 1) % len(sizes)]))
    return np.array(starts, np.uint32)
