"""Inputs of the block-statistics edge tests (tests/test_stats_edges.py on the CPU, tests/test_stats_edges_gpu.py on the device, the fixture
generator oracle/gen_golden.py block_stats_edges): job lists that mix block kinds inside a wave's four jobs, residuals at the limits of the
value ranges the kernel's comments argue with, and the reference's own `_c` functions on them.  Seeded, no I/O besides loading the fixture."""
import ctypes as C
import functools
import os
import zlib

import numpy as np

from svt_av1_psyex_amd import abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "block_stats_edges.npz")
W, H, REF_STRIDE = 256, 160, 272  # the planes of the packed lists and the psy patterns: source 256 x 160, reference stride 272
OTHER_AV1 = [(4, 4), (16, 16), (8, 16), (16, 8), (4, 16), (64, 16), (32, 32), (64, 64), (128, 128)]  # (width, height) beside 8x8
OTHER_ODD = [(12, 20), (3, 128), (1, 1)]  # not AV1 shapes: still defined (SvtHipBlockJob: sides 1..128)
SUBPEL_PHASES = [(3, 0), (0, 5), (6, 1)]  # x only, y only, both
PACKED_SEED, PACKED_N_MIN, PACKED_FIXTURE_JOBS = 20260, 8192, 600
COLUMNS = ["sad", "sse", "variance", "var_sse", "satd", "psy_energy", "variance10", "var_sse10"]
COLUMN_DTYPES = dict(abi.STATS_OUT_FIELDS + abi.PSY_OUT_FIELDS + abi.VAR10_OUT_FIELDS)


def random_job(rng, src_w, ref_stride, h, bw, bh, subpel=(0, 0)):
    sp = int(any(subpel))  # a sub-pel view reads one more source row / column
    x0, y0 = int(rng.integers(0, src_w - bw + 1 - sp)), int(rng.integers(0, h - bh + 1 - sp))
    x1, y1 = int(rng.integers(0, ref_stride - bw + 1)), int(rng.integers(0, h - bh + 1))
    return (y0 * src_w + x0, y1 * ref_stride + x1, bw, bh, subpel[0], subpel[1])


def packed_jobs(rng, src_w, ref_stride, h, n_min, av1_only):
    """(jobs, kinds): groups of four jobs, as many as reach n_min jobs, then a tail of one to three plain 8x8 jobs.  kinds[g] of group g:
    A  four plain 8x8 jobs (one shared matrix-core tile)
    B  three plain 8x8 jobs and one job of another size at a random position of the four
    C  four 8x8 jobs, one of them with a sub-pel phase (x only, y only or both) at a random position
    D  no 8x8 job
    The source plane is src_w wide, the reference plane ref_stride wide, both h high.  The same rng state gives the same groups for every
    n_min: a longer list repeats a shorter one's groups and goes on."""
    others = OTHER_AV1 + ([] if av1_only else OTHER_ODD)
    other = lambda: others[int(rng.integers(len(others)))]
    jobs, kinds = [], []
    while len(jobs) < n_min:
        kind = "ABCD"[int(rng.integers(4))]
        group = [(8, 8, (0, 0))] * 4
        if kind == "B":
            group[int(rng.integers(4))] = other() + ((0, 0),)
        elif kind == "C":
            group[int(rng.integers(4))] = (8, 8, SUBPEL_PHASES[int(rng.integers(3))])
        elif kind == "D":
            group = [other() + ((0, 0),) for _ in range(4)]
        jobs += [random_job(rng, src_w, ref_stride, h, bw, bh, sp) for bw, bh, sp in group]
        kinds.append(kind)
    jobs += [random_job(rng, src_w, ref_stride, h, 8, 8) for _ in range(int(rng.integers(1, 4)))]
    return np.array(jobs, dtype=abi.BLOCK_JOB_DTYPE), np.array(kinds)


def psy_defined(w, h):
    """svt_psy_distortion walks 8x8 tiles when both sides are >= 8, else 4x4 tiles: defined where the tiles fit the block (every AV1 shape)"""
    n = np.where((w >= 8) & (h >= 8), 8, 4)
    return (w % n == 0) & (h % n == 0)


def is_plain8(jobs):
    return (jobs["width"] == 8) & (jobs["height"] == 8) & (jobs["subpel_x"] == 0) & (jobs["subpel_y"] == 0)


def packed_coverage(jobs, kinds):
    """what a packed list covers, recomputed from the jobs themselves (kinds is only compared with it)"""
    ng = len(kinds)
    g = jobs[:4 * ng].reshape(ng, 4)
    plain, is8 = is_plain8(g), (g["width"] == 8) & (g["height"] == 8)
    found = np.where(plain.all(1), "A", np.where(is8.all(1), "C", np.where(plain.sum(1) == 3, "B", np.where(~is8.any(1), "D", "?"))))
    big_square_last = (g["width"][:, 3] == g["height"][:, 3]) & (g["width"][:, 3] >= 16)
    tail = jobs[4 * ng:]
    return dict(kinds_agree=bool((found == kinds).all()), groups={k: int((found == k).sum()) for k in "ABCD"},
                b_position=[int(((found == "B") & ~plain[:, i]).sum()) for i in range(4)],
                c_position=[int(((found == "C") & ~plain[:, i]).sum()) for i in range(4)],
                tile_reuse=int(((found[1:] == "A") & np.isin(found[:-1], ["B", "D"]) & big_square_last[:-1]).sum()),
                tail=len(tail), tail_plain8=bool(is_plain8(tail).all()))


def assert_packed_coverage(jobs, kinds, satd):
    """the conditions a packed list must meet before a test built on it means anything; satd: its SATD column"""
    c = packed_coverage(jobs, kinds)
    assert c["kinds_agree"], c
    assert min(c["groups"].values()) >= 100, c
    assert min(c["b_position"]) >= 20 and min(c["c_position"]) >= 20, c
    assert c["tile_reuse"] >= 50, c  # an A group right behind a 16x16 .. 128x128 job: the quad reuses the LDS tile hadamard_path just left
    assert 1 <= c["tail"] <= 3 and c["tail_plain8"], c
    assert len(np.unique(satd)) > 1000, len(np.unique(satd))
    return c


def packed_planes(seed=PACKED_SEED):
    """8-bit planes whose block residuals run from near zero to +-255: two smooth surfaces with noise, a corner of extremes"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:REF_STRIDE]
    base = 128 + 70 * np.sin(x / 23.0) * np.cos(y / 17.0)
    src = np.clip(base[:, :W] + rng.integers(-12, 13, (H, W)), 0, 255).astype(np.uint8)
    ref = np.clip(base + 25 * np.sin((x + y) / 9.0) + rng.integers(-20, 21, (H, REF_STRIDE)), 0, 255).astype(np.uint8)
    src[:40, :40], ref[:40, :40] = 255, 0
    src[120:, 200:], ref[120:, 200:] = 0, 255
    return src, ref


@functools.lru_cache(maxsize=None)
def standard_packed(av1_only, n_min=PACKED_N_MIN):
    """(src, ref, jobs, kinds) of the packed list every test and the fixture start from"""
    src, ref = packed_planes()
    jobs, kinds = packed_jobs(np.random.default_rng(PACKED_SEED + int(av1_only)), W, REF_STRIDE, H, n_min, av1_only)
    return src, ref, jobs, kinds


# ---- Walsh planes: residuals of +-255 that put a whole block's energy into one Hadamard coefficient ---------------------------------------
WALSH_SATD = {8: 16320, 16: 32640, 32: 32640}  # 64 * 255; the 16 and 32 combines ((a0 +- a1) >> 1, >> 2) bring four equal blocks to twice that
WALSH_MIXED16_SATD = 130560  # four 8x8 blocks with their coefficient at four different places: each gives (16320 +- 0) >> 1 to four outputs


def wal(u, i):
    return 1 - 2 * (bin(u & i).count("1") & 1)


def walsh_planes(n, u, v, sign):
    """8-bit n x n source and reference whose residual is sign * 255 * wal_u(row & 7) * wal_v(col & 7)"""
    k = np.arange(n) & 7
    pat = sign * np.outer([wal(u, int(i)) for i in k], [wal(v, int(i)) for i in k])
    return np.where(pat > 0, 255, 0).astype(np.uint8), np.where(pat > 0, 0, 255).astype(np.uint8)


def walsh_mixed16(specs):
    """a 16x16 whose four 8x8 blocks (raster order) are the Walsh planes of four (u, v, sign)"""
    src, ref = np.zeros((16, 16), np.uint8), np.zeros((16, 16), np.uint8)
    for q, (u, v, sign) in enumerate(specs):
        src[8 * (q >> 1):8 * (q >> 1) + 8, 8 * (q & 1):8 * (q & 1) + 8], ref[8 * (q >> 1):8 * (q >> 1) + 8, 8 * (q & 1):8 * (q & 1) + 8] = walsh_planes(8, u, v, sign)
    return src, ref


WALSH_REF_X0 = 16  # the reference plane's tiles start at this column


@functools.lru_cache(maxsize=None)
def walsh_atlas():
    """all 64 (u, v) as 32x32 tiles, tile (u, v) at (32 u, 32 v); rows 0..255 with sign +1, rows 256..511 with sign -1.  Source 512 x 256,
    reference 512 x 272 with its tiles 16 columns to the right.  A tile's aligned 8x8 and 16x16 blocks are Walsh planes of the same (u, v)."""
    src, ref = np.zeros((512, W), np.uint8), np.full((512, REF_STRIDE), 0x55, np.uint8)
    for s, sign in enumerate((1, -1)):
        for u in range(8):
            for v in range(8):
                a, b = walsh_planes(32, u, v, sign)
                src[256 * s + 32 * u:256 * s + 32 * u + 32, 32 * v:32 * v + 32] = a
                ref[256 * s + 32 * u:256 * s + 32 * u + 32, WALSH_REF_X0 + 32 * v:WALSH_REF_X0 + 32 * v + 32] = b
    return src, ref


def _atlas_job(y, x, n):
    return (y * W + x, y * REF_STRIDE + WALSH_REF_X0 + x, n, n, 0, 0)


@functools.lru_cache(maxsize=None)
def walsh_jobs():
    """(jobs, satd): every tile's 32x32, its four 16x16 and sixteen 8x8 blocks, then the 16x16 blocks on the corners where four tiles meet
    -- four different (u, v), and on the row between the two signs four different (u, v, sign) -- each with the SATD it must have"""
    jobs, satd = [], []
    for ty in range(16):
        for tx in range(8):
            for n in (32, 16, 8):
                for y in range(0, 32, n):
                    for x in range(0, 32, n):
                        jobs.append(_atlas_job(32 * ty + y, 32 * tx + x, n))
                        satd.append(WALSH_SATD[n])
    for ty in range(15):
        for tx in range(7):
            jobs.append(_atlas_job(32 * ty + 24, 32 * tx + 24, 16))
            satd.append(WALSH_MIXED16_SATD)
    return np.array(jobs, dtype=abi.BLOCK_JOB_DTYPE), np.array(satd, np.int64)


def walsh_quads(rng, n_min):
    """(jobs, satd): the atlas's 2,048 8x8 blocks in random order, over and over, until a multiple of four >= n_min: A groups only.  One job
    in three takes its reference block from the same tile of the other sign, where the reference equals the source: SATD 0 beside the
    others' 16,320, so that a quad's four results are told apart"""
    jobs, _ = walsh_jobs()
    j8 = jobs[jobs["width"] == 8][:2048]
    out = np.concatenate([j8[rng.permutation(len(j8))] for _ in range((n_min + len(j8) - 1) // len(j8))])[:(n_min + 3) // 4 * 4]
    zero = rng.integers(0, 3, len(out)) == 0
    top = out["src_offset"] < 256 * W  # rows 0..255: sign +1
    out["ref_offset"] = np.where(zero, np.where(top, out["ref_offset"] + 256 * REF_STRIDE, out["ref_offset"] - 256 * REF_STRIDE), out["ref_offset"])
    return out, np.where(zero, 0, WALSH_SATD[8]).astype(np.uint32)


def walsh_regions():
    """64x64 regions of the atlas: the aligned ones (four tiles each), some shifted by 32 rows and columns, some across the two signs"""
    pos = [(y, x) for y in range(0, 512, 64) for x in range(0, 256, 64)] + [(y, x) for y in (32, 224, 416) for x in (32, 96, 160)]
    return np.array([_atlas_job(y, x, 64) for y, x in pos], dtype=abi.BLOCK_JOB_DTYPE)


def walsh_region_satd(n_regions):
    """SATD of a Walsh region's 85 nested blocks: a 64x64 is four 32x32 tiles"""
    return np.tile(np.array([4 * WALSH_SATD[32]] + [WALSH_SATD[32]] * 4 + [WALSH_SATD[16]] * 16 + [WALSH_SATD[8]] * 64, np.uint32), n_regions)


# ---- range limits ----------------------------------------------------------------------------------------------------------------------
RANGE_W, RANGE_REF_STRIDE = 128, 144


def range_planes(bd, kind):
    """kind "max": every source sample at the maximum, every reference sample 0.  kind "split" (10-bit): left half +1023, right half -1023"""
    dt, hi = (np.uint8, 255) if bd == 8 else (np.uint16, 1023)
    src, ref = np.full((128, RANGE_W), hi, dt), np.zeros((128, RANGE_REF_STRIDE), dt)
    if kind == "split":
        src[:, 64:], ref[:, 64:128] = 0, hi
    return src, ref


def range_jobs(kind):
    """max: a block of every size in abi.VARIANCE_SIZES.  split: the 128x128 (sum 0: the variance is the wrapped var_sse), the 64x64 and
    32x32 blocks across the middle, and one-sided blocks"""
    at = lambda x, y, w, h: (y * RANGE_W + x, y * RANGE_REF_STRIDE + x, w, h, 0, 0)
    if kind == "max":
        return np.array([at(0, 0, w, h) for w, h in abi.VARIANCE_SIZES], dtype=abi.BLOCK_JOB_DTYPE)
    return np.array([at(0, 0, 128, 128), at(32, 32, 64, 64), at(48, 64, 32, 32), at(0, 0, 64, 128), at(64, 0, 64, 64), at(56, 8, 16, 16), at(60, 3, 8, 8), at(40, 0, 64, 16)],
                    dtype=abi.BLOCK_JOB_DTYPE)


def range_regions(kind):
    at = lambda x, y: (y * RANGE_W + x, y * RANGE_REF_STRIDE + x, 64, 64, 0, 0)
    return np.array([at(0, 0), at(64, 64), at(32, 17)] if kind == "max" else [at(32, 0), at(0, 64), at(64, 32), at(24, 40)], dtype=abi.BLOCK_JOB_DTYPE)


RANGE_SETS = {"max8": (8, "max"), "max10": (10, "max"), "split10": (10, "split")}

# ---- the psy patterns of test_psy_distortion_against_reference, as whole planes ------------------------------------------------------------
PSY_PATTERNS = ("max", "checker", "minmax", "low")
AV1_SHAPES = [(w, h) for w in (4, 8, 16, 32, 64, 128) for h in (4, 8, 16, 32, 64, 128) if max(w, h) <= 4 * min(w, h)]


def psy_planes(bd, pat):
    rng = np.random.default_rng(PSY_PATTERNS.index(pat) * 16 + bd)
    dt, hi = (np.uint8, 255) if bd == 8 else (np.uint16, 1023)
    a, b = np.zeros((H, W), dt), np.zeros((H, REF_STRIDE), dt)
    if pat == "max":
        a[:] = hi
    elif pat == "checker":
        a[::2, ::2] = hi; a[1::2, 1::2] = hi; b[:] = hi // 2
    elif pat == "minmax":
        a[:] = np.where(rng.integers(0, 2, a.shape) == 0, 0, hi); b[:] = hi - np.where(rng.integers(0, 2, b.shape) == 0, 0, hi)
    else:
        a[:] = rng.integers(0, 4, a.shape); b[:] = rng.integers(0, 2, b.shape)
    return a, b


def psy_jobs(seed=7):
    """every AV1 block shape three times at random positions of the W x H / REF_STRIDE x H planes, shuffled: a wave's four jobs are of four sizes"""
    rng = np.random.default_rng(seed)
    jobs = np.array([random_job(rng, W, REF_STRIDE, H, w, h) for w, h in AV1_SHAPES * 3], dtype=abi.BLOCK_JOB_DTYPE)
    return jobs[rng.permutation(len(jobs))][:len(jobs) - 2]  # a last wave of two jobs


def regions(rng, src_w, ref_stride, h, n):
    """n 64x64 regions at random, different positions of the two planes"""
    return np.array([random_job(rng, src_w, ref_stride, h, 64, 64) for _ in range(n)], dtype=abi.BLOCK_JOB_DTYPE)


# ---- the reference's own functions on a job list ----------------------------------------------------------------------------------------
def reference_outputs(ref, src, refp, jobs, bd):
    """(values, ok): per column of COLUMNS the reference's `_c` function on every job, and the mask of the jobs it is defined on
    (hadamard_path: 8-bit squares; psy: blocks its tiles fit; highbd_10 variance: 10-bit AV1 shapes; a sub-pel job: only the
    variance pair, from svt_aom_sub_pixel_variance{W}x{H}_c)."""
    P = C.c_void_p
    u32 = C.c_uint32
    ref.svt_spatial_full_distortion_kernel_c.restype = ref.svt_full_distortion_kernel16_bits_c.restype = C.c_uint64
    ref.svt_psy_distortion.restype = ref.svt_psy_distortion_hbd.restype = C.c_uint64
    ref.ref_hadamard_path.restype = C.c_uint32
    n, ss, rs = len(jobs), src.shape[1], refp.shape[1]
    val = {k: np.zeros(n, COLUMN_DTYPES[k]) for k in COLUMNS}
    ok = {k: np.zeros(n, bool) for k in COLUMNS}
    flat_s, flat_r = np.ascontiguousarray(src).reshape(-1), np.ascontiguousarray(refp).reshape(-1)
    for j, jb in enumerate(jobs):
        w, h = int(jb["width"]), int(jb["height"])
        s, r = flat_s[int(jb["src_offset"]):], flat_r[int(jb["ref_offset"]):]
        ps, pr = s.ctypes.data_as(P), r.ctypes.data_as(P)
        vs = u32()
        if jb["subpel_x"] or jb["subpel_y"]:
            assert bd == 8 and (w, h) in abi.VARIANCE_SIZES
            val["variance"][j] = getattr(ref, f"svt_aom_sub_pixel_variance{w}x{h}_c")(ps, ss, int(jb["subpel_x"]), int(jb["subpel_y"]), pr, rs, C.byref(vs)) & 0xFFFFFFFF
            val["var_sse"][j] = vs.value
            ok["variance"][j] = ok["var_sse"][j] = True
            continue
        if bd == 8:
            val["sad"][j] = ref.svt_nxm_sad_kernel_helper_c(ps, u32(ss), pr, u32(rs), u32(h), u32(w))
            val["sse"][j] = ref.svt_spatial_full_distortion_kernel_c(ps, u32(0), u32(ss), pr, C.c_int32(0), u32(rs), u32(w), u32(h))
            if (w, h) in abi.VARIANCE_SIZES:
                val["variance"][j] = getattr(ref, f"svt_aom_variance{w}x{h}_c")(ps, ss, pr, rs, C.byref(vs)) & 0xFFFFFFFF
            else:  # no svt_aom_variance{W}x{H} of this shape: the generic 16-bit function on widened samples defines it
                s16 = np.ascontiguousarray(s[:(h - 1) * ss + w].astype(np.uint16))
                r16 = np.ascontiguousarray(r[:(h - 1) * rs + w].astype(np.uint16))
                val["variance"][j] = ref.svt_aom_variance_highbd_c(s16.ctypes.data_as(P), ss, r16.ctypes.data_as(P), rs, w, h, C.byref(vs)) & 0xFFFFFFFF
            if w == h and w in (4, 8, 16, 32, 64, 128):
                val["satd"][j] = ref.ref_hadamard_path(ps, u32(ss), pr, u32(rs), u32(w))
                ok["satd"][j] = True
        else:
            val["sad"][j] = ref.svt_aom_sad_16b_kernel_c(ps, u32(ss), pr, u32(rs), u32(h), u32(w))
            val["sse"][j] = ref.svt_full_distortion_kernel16_bits_c(ps, u32(0), u32(ss), pr, C.c_int32(0), u32(rs), u32(w), u32(h))
            val["variance"][j] = ref.svt_aom_variance_highbd_c(ps, ss, pr, rs, w, h, C.byref(vs)) & 0xFFFFFFFF
            if (w, h) in abi.VARIANCE_SIZES:  # pointers CONVERT_TO_BYTEPTR'd: address >> 1
                v10 = u32()
                val["variance10"][j] = getattr(ref, f"svt_aom_highbd_10_variance{w}x{h}_c")(P(s.ctypes.data >> 1), ss, P(r.ctypes.data >> 1), rs, C.byref(v10)) & 0xFFFFFFFF
                val["var_sse10"][j] = v10.value
                ok["variance10"][j] = ok["var_sse10"][j] = True
        val["var_sse"][j] = vs.value
        for k in ("sad", "sse", "variance", "var_sse"):
            ok[k][j] = True
        if psy_defined(w, h):
            val["psy_energy"][j] = (ref.svt_psy_distortion if bd == 8 else ref.svt_psy_distortion_hbd)(ps, u32(ss), pr, u32(rs), u32(w), u32(h))
            ok["psy_energy"][j] = True
    return val, ok


def oracle_outputs(oracle, src, refp, jobs, bd):
    """the oracle's columns on a job list: one batch with hadamard_path (8-bit), one with the psy energy on the jobs that have one"""
    import pyoracle
    out = pyoracle.block_stats(oracle, src, refp, jobs, bd, satd=(bd == 8))
    psy_ok = psy_defined(jobs["width"], jobs["height"])
    out["psy_energy"] = np.zeros(len(jobs), np.uint64)
    if psy_ok.any():
        out["psy_energy"][psy_ok] = pyoracle.block_stats(oracle, src, refp, jobs[psy_ok], bd, satd=False, psy_rd=0.0)["psy_energy"]
    return out


def disagreements(val, ok, got):
    """columns (of those `got` has) on which `got` differs from the reference values where they are defined"""
    bad = []
    for k in COLUMNS:
        if k in got and ok[k].any() and not np.array_equal(np.asarray(got[k])[ok[k]], val[k][ok[k]]):
            i = int(np.flatnonzero(ok[k] & (np.asarray(got[k]) != val[k]))[0])
            bad.append(f"{k}: first mismatch at job {i}: {val[k][i]} expected, got {got[k][i]}")
    return bad


# ---- the fixture -------------------------------------------------------------------------------------------------------------------------
def fixture_sets():
    """name -> (bit depth, source, reference, jobs) of everything tests/golden/block_stats_edges.npz has the reference's outputs for"""
    sets = {"walsh": (8,) + walsh_atlas() + (walsh_jobs()[0],)}
    for name, (bd, kind) in RANGE_SETS.items():
        sets[name] = (bd,) + range_planes(bd, kind) + (range_jobs(kind),)
    src, ref, jobs, _ = standard_packed(True)
    sets["packed"] = (8, src, ref, jobs[:PACKED_FIXTURE_JOBS])
    return sets


def inputs_crc(src, ref, jobs):
    return zlib.crc32(np.ascontiguousarray(jobs).tobytes(), zlib.crc32(np.ascontiguousarray(ref).tobytes(), zlib.crc32(np.ascontiguousarray(src).tobytes())))


def load_fixture(name):
    """(bit depth, source, reference, jobs, values, ok) of one fixture set; the regenerated inputs are checked against the stored CRC"""
    z = np.load(GOLDEN)
    bd, src, ref, jobs = fixture_sets()[name]
    assert int(z[f"{name}_crc"]) == inputs_crc(src, ref, jobs), f"{name}: the regenerated inputs are not the ones the fixture was made from"
    cols = [k for k in COLUMNS if f"{name}_{k}" in z.files]
    return bd, src, ref, jobs, {k: z[f"{name}_{k}"] for k in cols}, {k: z[f"{name}_ok_{k}"].astype(bool) for k in cols}
