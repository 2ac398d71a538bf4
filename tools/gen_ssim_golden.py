#!/usr/bin/env python3
"""Writes tests/golden/ssim.npz: the reference encoder's own SSIM leaves and SSIM distortion on seeded inputs.

Run by hand on a machine that has the reference's sources (--ref: the root of its source tree); never by the tests, build(), smoke() or
bench.py.  It compiles the reference's Codec/mode_decision.c, Codec/enc_dec_process.c, Codec/aom_dsp_rtcd.c and Codec/psy_rd.c where they lie, together
with a small harness of its own, into a temporary directory outside the tree (gcc, -O2, no -ffast-math: x86-64 doubles without FMA, like the
reference's default build), links with --gc-sections and a version script that exports the harness alone, and calls
  svt_ssim_{8x8,4x4}{,_hbd}_c                 on tiles of the fixture planes (the four rtcd pointers set to their _c bodies)
  svt_spatial_full_distortion_ssim_kernel     on jobs of every AV1 block size, every transform size and cropped shapes, psy_rd in PSY_RDS
The fixture holds numbers only: the planes, the tile positions with the leaves' results as uint64 bit patterns, and the jobs with their
distortions.  --check recomputes everything and compares it with the committed file instead of writing it."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import ssim_cases as sc  # noqa: E402

HARNESS = r"""
#include <stdbool.h>
#include <stdint.h>
extern double (*svt_ssim_8x8)(const uint8_t *s, uint32_t sp, const uint8_t *r, uint32_t rp);
extern double (*svt_ssim_4x4)(const uint8_t *s, uint32_t sp, const uint8_t *r, uint32_t rp);
extern double (*svt_ssim_8x8_hbd)(const uint16_t *s, uint32_t sp, const uint16_t *r, uint32_t rp);
extern double (*svt_ssim_4x4_hbd)(const uint16_t *s, uint32_t sp, const uint16_t *r, uint32_t rp);
double svt_ssim_8x8_c(const uint8_t *s, uint32_t sp, const uint8_t *r, uint32_t rp);
double svt_ssim_4x4_c(const uint8_t *s, uint32_t sp, const uint8_t *r, uint32_t rp);
double svt_ssim_8x8_hbd_c(const uint16_t *s, uint32_t sp, const uint16_t *r, uint32_t rp);
double svt_ssim_4x4_hbd_c(const uint16_t *s, uint32_t sp, const uint16_t *r, uint32_t rp);
uint64_t svt_spatial_full_distortion_ssim_kernel(uint8_t *input, uint32_t input_offset, uint32_t input_stride, uint8_t *recon, int32_t recon_offset,
                                                 uint32_t recon_stride, uint32_t area_width, uint32_t area_height, bool hbd, double psy_rd);

void harness_init(void) {
    svt_ssim_8x8 = svt_ssim_8x8_c;
    svt_ssim_4x4 = svt_ssim_4x4_c;
    svt_ssim_8x8_hbd = svt_ssim_8x8_hbd_c;
    svt_ssim_4x4_hbd = svt_ssim_4x4_hbd_c;
}
/* kind: 0 svt_ssim_8x8_c, 1 svt_ssim_4x4_c, 2 svt_ssim_8x8_hbd_c, 3 svt_ssim_4x4_hbd_c */
double harness_tile(int kind, const void *s, uint32_t sp, const void *r, uint32_t rp) {
    switch (kind) {
    case 0: return svt_ssim_8x8_c(s, sp, r, rp);
    case 1: return svt_ssim_4x4_c(s, sp, r, rp);
    case 2: return svt_ssim_8x8_hbd_c(s, sp, r, rp);
    default: return svt_ssim_4x4_hbd_c(s, sp, r, rp);
    }
}
uint64_t harness_ssim_dist(void *input, uint32_t input_offset, uint32_t input_stride, void *recon, int32_t recon_offset, uint32_t recon_stride,
                           uint32_t w, uint32_t h, int hbd, double psy_rd) {
    return svt_spatial_full_distortion_ssim_kernel(input, input_offset, input_stride, recon, recon_offset, recon_stride, w, h, hbd != 0, psy_rd);
}
"""
VERSION_SCRIPT = "{ global: harness_*; local: *; };\n"
SOURCES = ["Codec/mode_decision.c", "Codec/enc_dec_process.c", "Codec/aom_dsp_rtcd.c", "Codec/psy_rd.c"]


def build(ref, tmp):
    lib = os.path.join(ref, "Source", "Lib")
    inc = [f"-I{ref}/Source/API"] + [f"-I{lib}/{d}" for d in ("Codec", "C_DEFAULT", "Globals", "ASM_SSE2", "ASM_SSSE3", "ASM_SSE4_1", "ASM_AVX2")]
    inc += [f"-I{ref}/third_party/fastfeat", f"-I{ref}/third_party/safestringlib"]
    flags = ["-O2", "-fPIC", "-ffunction-sections", "-fdata-sections", "-w", "-DARCH_X86_64=1", "-DEN_AVX512_SUPPORT=0", "-DEXCLUDE_HASH=1",
             "-DREPRODUCIBLE_BUILDS=0"] + inc
    open(os.path.join(tmp, "harness.c"), "w").write(HARNESS)
    open(os.path.join(tmp, "exports.map"), "w").write(VERSION_SCRIPT)
    objs = []
    for src in [os.path.join(lib, s) for s in SOURCES] + [os.path.join(tmp, "harness.c")]:
        obj = os.path.join(tmp, os.path.basename(src)[:-2] + ".o")
        subprocess.run(["gcc"] + flags + ["-c", src, "-o", obj], check=True)
        objs.append(obj)
    so = os.path.join(tmp, "libssimref.so")
    subprocess.run(["gcc", "-shared", "-o", so] + objs + ["-Wl,--gc-sections", "-Wl,-z,defs", f"-Wl,--version-script={tmp}/exports.map", "-lm"], check=True)
    L = C.CDLL(so)
    L.harness_tile.restype = C.c_double
    L.harness_tile.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    L.harness_ssim_dist.restype = C.c_uint64
    L.harness_ssim_dist.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_double]
    L.harness_init()
    return L


def generate(L):
    rng = np.random.default_rng(20261016)
    out = {}
    for bd in (8, 10):
        src, ref = sc.make_planes(rng, bd)
        out[f"src{bd}"], out[f"ref{bd}"] = src, ref
        stride = src.shape[1]
        bpp = src.itemsize
        # leaves: tiles at random positions of every (src region, ref region) pair
        tiles = []
        for n in (8, 4):
            kind = (0 if n == 8 else 1) + (2 if bd == 10 else 0)
            for (a, b) in sc.ALL_PAIRS:
                for _ in range(6):
                    y, x = int(rng.integers(0, sc.REGION - n + 1)), int(rng.integers(0, sc.REGION - n + 1))
                    so, ro = y * stride + a * sc.REGION + x, y * stride + b * sc.REGION + x
                    v = L.harness_tile(kind, src.ctypes.data + so * bpp, stride, ref.ctypes.data + ro * bpp, stride)
                    tiles.append((kind, so, ro, np.float64(v).view(np.uint64)))
        t = np.array(tiles, dtype=np.uint64)
        out[f"tile_kind{bd}"], out[f"tile_src{bd}"], out[f"tile_ref{bd}"], out[f"tile_bits{bd}"] = (t[:, 0].astype(np.uint8), t[:, 1].astype(np.uint32),
                                                                                                  t[:, 2].astype(np.uint32), t[:, 3])
        # the distortion: every size on every pair, each psy_rd
        jobs = sc.region_jobs(rng, sc.SIZES, sc.ALL_PAIRS)
        out[f"jobs{bd}"] = jobs
        dist = np.zeros((len(sc.PSY_RDS), len(jobs)), np.uint64)
        for k, psy in enumerate(sc.PSY_RDS):
            for i, j in enumerate(jobs):
                dist[k, i] = L.harness_ssim_dist(src.ctypes.data, int(j["src_offset"]), stride, ref.ctypes.data, int(j["ref_offset"]), stride,
                                                 int(j["width"]), int(j["height"]), 1 if bd == 10 else 0, psy)
        out[f"dist{bd}"] = dist
    out["psy_rds"] = np.array(sc.PSY_RDS, np.float64)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ref", required=True, help="root of the reference encoder's source tree")
    ap.add_argument("--check", action="store_true", help="compare with the committed fixture instead of writing it")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        out = generate(build(a.ref, tmp))
    if a.check:
        z = np.load(sc.GOLDEN)
        bad = sorted(set(z.files) ^ set(out)) + [k for k in out if k in z.files and not (z[k].dtype == out[k].dtype and np.array_equal(z[k], out[k]))]
        print("identical" if not bad else f"differs: {bad}")
        sys.exit(1 if bad else 0)
    np.savez_compressed(sc.GOLDEN, **out)
    print(f"wrote {sc.GOLDEN}: " + ", ".join(f"{k}{list(v.shape)}" for k, v in out.items()))


if __name__ == "__main__":
    main()
