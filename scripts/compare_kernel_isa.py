#!/usr/bin/env python3
"""Compare the gfx950 code of two builds kernel by kernel (a refactor must leave every kernel as it was).

  scripts/compare_kernel_isa.py --old OLD.s [OLD2.s ...] --new NEW.s [NEW2.s ...] [--map REGEX=REPL ...]

The .s files are what `hipcc <library flags> --save-temps=obj -c file.hip` leaves as
`*-hip-amdgcn-amd-amdhsa-gfx950.s`.  Per kernel the instruction text from its label to its .Lfunc_end and
its .amdhsa_ descriptor block are compared after local label numbers, comment padding and the IR block
names in comments are normalised; --map rewrites the
OLD text first, for the mangled names of templates that lost a parameter, e.g.
  --map '(warp_rigid_dmaILb[01]ELb[01]E)Li1ELi2ELi4E=\\1'
Prints one line per kernel that differs or is missing, a VGPR / SGPR / LDS / scratch line per kernel with
--table, and exits 1 unless both sides hold the same kernels with identical text.
"""
import argparse
import re
import sys

LOCAL = [(re.compile(r"\.LBB\d+_"), ".LBB_"), (re.compile(r"\.Lfunc_(begin|end)\d+"), r".Lfunc_\1"),
         (re.compile(r"\.Ltmp\d+"), ".Ltmp"), (re.compile(r"\bBB\d+_"), "BB_"), (re.compile(r"[ \t]+"), " "),
         (re.compile(r" ?; %\S.*$", re.M), "")]  # the compiler's names of IR blocks, in comments
RES = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(paths, maps):
    out = {}
    for path in paths:
        text = open(path).read()
        for pat, repl in maps:
            text = re.sub(pat, repl, text)
        lines = text.split("\n")
        for i, line in enumerate(lines):
            m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
            if not m:
                continue
            name = m.group(1)
            # the descriptor block sits between the kernel's label and its .Lfunc_end
            start = next(j for j in range(i, -1, -1) if lines[j].startswith(name + ":"))
            end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
            body = "\n".join(lines[start:end])
            for pat, repl in LOCAL:
                body = pat.sub(repl, body)
            assert name not in out, f"{name} defined twice"
            out[name] = body
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--map", action="append", default=[])
    ap.add_argument("--table", action="store_true")
    a = ap.parse_args()
    maps = [tuple(m.split("=", 1)) for m in a.map]
    old, new = kernels(a.old, maps), kernels(a.new, [])
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print(f"only in {'new' if name in new else 'old'}: {name}")
            bad += 1
        elif old[name] != new[name]:
            print(f"differs: {name}")
            bad += 1
        if a.table and name in new:
            print(name, *(f"{k}={re.search(k + r'[ ]+(.+)', new[name]).group(1)}" for k in RES))
    print(f"{len(old)} kernels before, {len(new)} after, {bad} differ or are missing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
