#!/usr/bin/env python3
"""Is the device code of this work tree the same as that of <git-rev>?

  python scripts/isa_identity.py <git-rev> [--units a,b] [--flags="-DX=1 ..."] [--jobs N]

(write --flags=... with the equals sign: the value starts with a dash)

Exports include/ and yolo-v4-tf.keras_amd/csrc/ of <git-rev> into a temporary directory (git archive; the work tree is not
touched), compiles every translation unit of csrc/build.py in both trees with build.py's flags plus `-S --cuda-device-only`,
drops the lines that carry the per-compilation `__hip_cuid_<hash>` symbol and compares the listings as text.  Prints per unit
`identical`, or the kernel symbol and line of the first difference; exits non-zero on any difference or compile error.

What it is for: a change that only moves kernel source around must not change a kernel that runs at 254-256 registers.
Identical listings are bit-identical results and identical speed by construction, checkable without a GPU.  A full run is two
library builds, which is why this is a script and not a test.
"""
import argparse
import importlib.util
import os
import re
import shlex
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("yolo-v4-tf.keras_amd", "csrc")
SYMBOL = re.compile(r"^([A-Za-z_$][\w$.]*):")


def load_build():
    spec = importlib.util.spec_from_file_location("y4_build", os.path.join(ROOT, CSRC, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def listing(hipcc, flags, tree, unit, out):
    """The device listing of `unit` in `tree` without its cuid lines, or the compiler's complaint."""
    asm = os.path.join(out, unit + ".s")
    r = subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", unit + ".hip", "-o", asm],
                       cwd=os.path.join(tree, CSRC), capture_output=True, text=True)
    if r.returncode != 0:
        return None, r.stderr[:4000]           # (the head: the first error is the informative one)
    # warnings (build.py's -Wall is among the flags), without the driver's own about a link flag that -S leaves unused
    warn = "".join(l for l in r.stderr.splitlines(True) if "argument unused during compilation" not in l)
    if warn.strip():
        sys.stderr.write(f"{unit} in {tree}:\n{warn[-3000:]}")
    with open(asm) as f:
        lines = [l for l in f if "__hip_cuid_" not in l]
    os.remove(asm)
    return lines, None


def first_difference(a, b):
    symbol = "(no symbol yet)"
    for n, (la, lb) in enumerate(zip(a, b), 1):
        if la != lb:
            return f"differs in {symbol}, line {n}:\n    - {la.rstrip()}\n    + {lb.rstrip()}"
        m = SYMBOL.match(la)
        if m:
            symbol = m.group(1)
    if len(a) != len(b):
        return f"differs in length behind {symbol}: {len(a)} lines against {len(b)}"
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("rev", help="the commit to compare the work tree with")
    ap.add_argument("--units", default="", help="comma-separated subset of build.py's UNITS")
    ap.add_argument("--flags", default="", help="extra compiler flags for both trees (the -D defines of a variant build); write --flags=\"...\"")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1), help="parallel hipcc processes (at most 16)")
    args = ap.parse_args()

    build = load_build()
    units = [u for u in args.units.split(",") if u] or list(build.UNITS)
    unknown = [u for u in units if u not in build.UNITS]
    if unknown:
        sys.exit("not in build.py's UNITS: " + ", ".join(unknown))
    flags = list(build.FLAGS) + shlex.split(args.flags)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    jobs = max(1, min(16, args.jobs))

    with tempfile.TemporaryDirectory(prefix="isa_identity_") as tmp:
        ref, out_ref, out_new = (os.path.join(tmp, d) for d in ("ref", "s_ref", "s_new"))
        for d in (ref, out_ref, out_new):
            os.makedirs(d)
        archive = subprocess.run(["git", "-C", ROOT, "archive", args.rev, "include", CSRC.replace(os.sep, "/")], check=True, capture_output=True)
        subprocess.run(["tar", "-x", "-C", ref], input=archive.stdout, check=True)
        sha = subprocess.run(["git", "-C", ROOT, "rev-parse", args.rev], check=True, capture_output=True, text=True).stdout.strip()
        print(f"work tree against {sha}" + (f", extra flags: {args.flags}" if args.flags else ""))

        def compare(unit):
            a, err_a = listing(hipcc, flags, ref, unit, out_ref)
            b, err_b = listing(hipcc, flags, ROOT, unit, out_new)
            if err_a or err_b:
                return unit, "does not compile in " + " and ".join(w for w, e in (("the reference tree", err_a), ("the work tree", err_b)) if e) + \
                    ":\n" + (err_a or err_b)
            return unit, first_difference(a, b)

        bad = 0
        with ThreadPoolExecutor(max_workers=jobs) as ex:
            for unit, diff in ex.map(compare, units):
                print(f"{unit}: {diff or 'identical'}", flush=True)
                bad += diff is not None
    print(f"{len(units) - bad} of {len(units)} units identical")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
