#!/usr/bin/env python3
"""Device assembly of a git revision against the working tree's, per kernel file (developer tool).

Compiles every kernel translation unit of phase-vocoder_amd/csrc to gfx950 assembly (device
only, the flags of scripts/isa_static.py, -fno-slp-vectorize for pv_analysis and pv_resident) twice — from the
sources of REV, taken with `git show REV:path` into a temporary directory, and from the working
tree — and counts the lines that differ.  Before the comparison the `.file` and `.ident` lines
are dropped, the per-compilation `__hip_cuid_<hash>` symbol is normalised, and every --rename
pair is applied to both sides (so a kernel that changed its name can be mapped onto one
spelling).  Nothing is run; the exit status is non-zero if any file differs.

  python3 scripts/asm_diff.py HEAD~1
  python3 scripts/asm_diff.py HEAD~1 --rename '_ZN2pv5k_oldILi(\\d+)EE=>_ZN2pv5k_newILi\\1ELb0EE'
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_static import FLAGS  # noqa: E402

CSRC = "phase-vocoder_amd/csrc"
EXTRA = {"pv_analysis": ["-fno-slp-vectorize"], "pv_resident": ["-fno-slp-vectorize"]}


def checkout(rev, dst):
    """csrc/ and include/ of `rev` under dst"""
    names = subprocess.run(["git", "ls-tree", "-r", "--name-only", rev, "--", CSRC, "include"],
                           cwd=ROOT, check=True, capture_output=True, text=True).stdout.split("\n")
    for name in filter(None, names):
        path = os.path.join(dst, name)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(subprocess.run(["git", "show", f"{rev}:{name}"], cwd=ROOT, check=True,
                                   capture_output=True).stdout)


def kernels_of(root):
    return sorted(f[:-4] for f in os.listdir(os.path.join(root, CSRC)) if f.endswith(".hip"))


def compile_asm(root, name, out):
    r = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, *EXTRA.get(name, []), "-I", os.path.join(root, "include"),
                        "-o", out, os.path.join(root, CSRC, name + ".hip")], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{name}.hip of {root}:\n{r.stderr[-2000:]}")
    return out


def normalised(path, renames):
    text = open(path).read()
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", text)
    for pat, repl in renames:
        text = pat.sub(repl, text)
    return [ln for ln in text.split("\n") if not ln.lstrip().startswith((".file", ".ident"))]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("rev", help="the git revision to compare the working tree with")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=>REPL",
                    help="re.sub applied to both assemblies before the comparison (repeatable)")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--show", type=int, default=0, metavar="N", help="print the first N differing lines per file")
    a = ap.parse_args()
    renames = []
    for r in a.rename:
        pat, sep, repl = r.partition("=>")
        if not sep:
            ap.error(f"--rename {r!r}: expected REGEX=>REPL")
        renames.append((re.compile(pat), repl))

    with tempfile.TemporaryDirectory() as td:
        old = os.path.join(td, "rev")
        checkout(a.rev, old)
        names = kernels_of(ROOT)
        added = [n for n in names if n not in kernels_of(old)]
        if added:  # a new translation unit has nothing to be compared with
            print(f"only in the tree (not compared): {added}")
            names = [n for n in names if n not in added]
        if kernels_of(old) != names:
            print(f"kernel files differ: {a.rev} has {kernels_of(old)}, the tree {names}")
            return 1
        with ThreadPoolExecutor(a.jobs) as ex:
            jobs = {(side, n): ex.submit(compile_asm, root, n, os.path.join(td, f"{side}_{n}.s"))
                    for n in names for side, root in (("rev", old), ("tree", ROOT))}
            asm = {k: f.result() for k, f in jobs.items()}
        bad = 0
        print(f"{'file':<14} {'lines':>8} {'kernels':>8} {'differing':>10}")
        for n in names:
            x, y = normalised(asm["rev", n], renames), normalised(asm["tree", n], renames)
            kernels = sum(1 for ln in y if ln.lstrip().startswith(".amdhsa_kernel"))
            if x == y:
                diff = []
            else:
                diff = [ln for ln in difflib.unified_diff(x, y, lineterm="", n=0)
                        if ln[:1] in "+-" and not ln.startswith(("+++", "---"))]
            print(f"{n:<14} {len(y):>8} {kernels:>8} {len(diff):>10}")
            for ln in diff[:a.show]:
                print("    " + ln)
            bad += bool(diff)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
