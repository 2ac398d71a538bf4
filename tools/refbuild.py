"""What the tools/gen_*_golden.py generators share: the build of a reference harness into a shared object, and the check-or-write driver.

A generator keeps what is its own -- SOURCES, the HARNESS* texts, the argtypes, the cases and the coverage assertions -- and calls
  build()   the reference's sources and the harness units, compiled in parallel with one flag set and linked with --gc-sections, -z defs and a version
            script that exports harness_* alone; where the caller asks, symbols the link still wants get stand-ins (functions that abort)
  main()    --ref and --check (and the flags a generator registers), the fixtures generated, then either compared with the committed files or written
Every departure from the defaults is an argument at the call site, with its reason beside it.  Nothing here is run by the tests, build(), smoke() or
bench.py, except the pure functions undefined_symbols() and compare(), which tests/test_tools_common.py checks."""
import argparse
import ctypes as C
import io
import os
import subprocess
import sys
import tempfile
import zipfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VERSION_SCRIPT = "{ global: harness_*; local: *; };\n"
FLAGS = ["-O2", "-fPIC", "-ffunction-sections", "-fdata-sections", "-w", "-msse4.1", "-DARCH_X86_64=1", "-DEN_AVX512_SUPPORT=0", "-DEXCLUDE_HASH=1",
         "-DREPRODUCIBLE_BUILDS=0"]
INCLUDES = ["Source/API"] + ["Source/Lib/" + d for d in ("Codec", "C_DEFAULT", "Globals", "ASM_SSE2", "ASM_SSSE3", "ASM_SSE4_1", "ASM_AVX2")]
INCLUDES += ["third_party/fastfeat", "third_party/safestringlib"]
MAX_JOBS = 16
MAX_LINKS = 8


def undefined_symbols(stderr):
    """The symbols a failed link reports as undefined, sorted, each once (GNU ld: "undefined reference to `name'")."""
    return sorted({ln.split("undefined reference to `")[1].split("'")[0] for ln in stderr.splitlines() if "undefined reference to `" in ln})


def build(ref, tmp, name, sources, harnesses, flags=(), includes=(), libs=(), source_flags=None, standins=False):
    """Compiles `sources` (paths under <ref>/Source/Lib) and `harnesses` ((unit name, C text) pairs) into <tmp>/lib<name>.so and returns it loaded.

    flags, includes (absolute directories) and libs (as "-lm" is) come on top of the defaults; source_flags is {source: flags for that unit alone}.
    With standins, a link that fails on undefined symbols is repeated, at most MAX_LINKS times in all, with a function that aborts for each of them;
    without, the link is made once and must succeed."""
    lib = os.path.join(ref, "Source", "Lib")
    cc = ["gcc"] + FLAGS + list(flags) + [f"-I{ref}/{d}" for d in INCLUDES] + [f"-I{d}" for d in includes]
    with open(os.path.join(tmp, "exports.map"), "w") as f:
        f.write(VERSION_SCRIPT)
    units = [(os.path.join(lib, s), (source_flags or {}).get(s, [])) for s in sources]
    for unit, text in harnesses:
        with open(os.path.join(tmp, unit + ".c"), "w") as f:
            f.write(text)
        units.append((os.path.join(tmp, unit + ".c"), []))
    objs = [os.path.join(tmp, os.path.basename(src)[:-2] + ".o") for src, _ in units]
    if len(set(objs)) != len(objs):
        raise ValueError("two units with the same base name")
    with ThreadPoolExecutor(MAX_JOBS) as pool:
        for r in list(pool.map(lambda u, o: subprocess.run(cc + u[1] + ["-c", u[0], "-o", o]), units, objs)):
            r.check_returncode()
    so = os.path.join(tmp, f"lib{name}.so")
    link = ["-Wl,--gc-sections", "-Wl,-z,defs", f"-Wl,--version-script={tmp}/exports.map", "-lm"] + list(libs)
    wanted = []
    for _ in range(MAX_LINKS if standins else 1):
        extra = []
        if standins:
            with open(os.path.join(tmp, "standins.c"), "w") as f:
                f.write("#include <stdio.h>\n#include <stdlib.h>\n" +
                        "".join(f'void {s}(void) {{ fputs("stand-in called: {s}\\n", stderr); abort(); }}\n' for s in wanted))
            extra = [os.path.join(tmp, "standins.o")]
            subprocess.run(cc + ["-c", os.path.join(tmp, "standins.c"), "-o", extra[0]], check=True)
        r = subprocess.run(["gcc", "-shared", "-o", so] + objs + extra + link, capture_output=True, text=True)
        if r.returncode == 0:
            break
        more = undefined_symbols(r.stderr)
        if not standins or set(more) <= set(wanted):
            raise RuntimeError(r.stderr[-4000:])
        wanted = sorted(set(wanted) | set(more))
    else:
        raise RuntimeError(r.stderr[-4000:])
    if wanted:
        print(f"stand-ins for {len(wanted)} symbols the link still wants: {wanted[:6]}")
    return C.CDLL(so)


def save(path, arrays):
    """an .npz with fixed time stamps, so that the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def savez(path, arrays):
    """numpy's own .npz, the arrays in the order of the dict: how the fixtures older than save() were written, and how their generators still write"""
    np.savez_compressed(path, **arrays)


def compare(committed, made):
    """The sorted names of what differs between two {name: array} mappings: a name only one of them has, another dtype, other values."""
    return sorted(k for k in set(committed) | set(made)
                  if not (k in committed and k in made and committed[k].dtype == made[k].dtype and np.array_equal(committed[k], made[k])))


def wrote(path, arrays):
    return f"wrote {path} ({os.path.getsize(path)} bytes), {len(arrays)} arrays"


def wrote_shapes(path, arrays):
    return f"wrote {path} ({os.path.getsize(path)} bytes): " + ", ".join(f"{k}{list(v.shape)}" for k, v in arrays.items())


def main(doc, build_lib, fixtures, save=save, wrote=wrote, flags=(), first=None, select=None):
    """The generators' command line.  build_lib(ref, tmp) gives the library; fixtures is {fixture path: generate(library) -> {name: array}}.

    --check compares every fixture with the committed file, prints "identical" or "differs: [names]" (after the file's name where there are several) and
    exits with 1 if any differs.  Otherwise the fixtures, or those for which select(args, path) holds, are written with `save` and the line wrote(path,
    arrays) is printed for each.  flags are (option, help) pairs of switches of the generator's own; first(args, library), where given, runs before
    anything is generated, and a true result ends the run there."""
    ap = argparse.ArgumentParser(description=doc.split("\n")[0])
    ap.add_argument("--ref", required=True, help="root of the reference encoder's source tree")
    ap.add_argument("--check", action="store_true", help="compare with the committed fixtures instead of writing them")
    for option, text in flags:
        ap.add_argument(option, action="store_true", help=text)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        L = build_lib(a.ref, tmp)
        if first and first(a, L):
            return
        made = {path: gen(L) for path, gen in fixtures.items() if a.check or not select or select(a, path)}
    if a.check:
        differs = False
        for path, arrays in made.items():
            bad = compare(np.load(path), arrays)
            print((f"{os.path.basename(path)}: " if len(made) > 1 else "") + ("identical" if not bad else f"differs: {bad}"))
            differs = differs or bool(bad)
        sys.exit(1 if differs else 0)
    for path, arrays in made.items():
        save(path, arrays)
        print(wrote(path, arrays))
