#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel.

    hipcc $(HIPFLAGS) --offload-device-only -S csrc/x.hip -o DIR/x.s     (every csrc/*.hip, both trees)
    tools/kernel_isa_cmp.py OLD_DIR NEW_DIR

For a refactor that moves kernels between files: a whole-file diff of the assembly no longer lines
up, but every kernel's own text must. Per kernel symbol (every `.amdhsa_kernel NAME`) this takes the
instructions, from the label `NAME:` to the next `.section`, and the descriptor block, `.amdhsa_kernel`
to `.end_amdhsa_kernel` (registers, LDS, scratch, kernarg size). Assembler comments (from `;`, they
carry per-file block numbers) are stripped, local labels (`.L...`) are renumbered in order of first
use, and `__hip_cuid_` lines are dropped. A header's kernels are emitted by every file that includes
it: all copies of a symbol on one side must then equal the copies on the other.

Prints one line per kernel (same / differ / missing) and a summary; exits non-zero on any difference.
It compares text and knows nothing about any instruction.
"""
import glob
import os
import re
import sys

LOCAL = re.compile(r"\.L[A-Za-z0-9_$.]+")


def normalise(lines):
    names = {}
    out = []
    for line in lines:
        line = line.split(";", 1)[0].strip()
        if not line or "__hip_cuid_" in line:
            continue
        out.append(LOCAL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), line))
    return "\n".join(out)


def kernels_of(path):
    """{symbol: (instruction text, descriptor text)} of one .s file."""
    lines = open(path).read().split("\n")
    found = {}
    for i, line in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if not m:
            continue
        sym = m.group(1)
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        label = next(j for j in range(i, -1, -1) if lines[j].split(";", 1)[0].strip() == sym + ":")
        stop = next(j for j in range(label, len(lines)) if lines[j].strip().startswith(".section"))
        found[sym] = (normalise(lines[label:stop]), normalise(lines[i:end + 1]))
    return found


def collect(d):
    """{symbol: {file: (text, descriptor)}} over every .s file of a directory."""
    table = {}
    files = sorted(glob.glob(os.path.join(d, "*.s")))
    if not files:
        sys.exit("no .s files in %s" % d)
    for path in files:
        for sym, body in kernels_of(path).items():
            table.setdefault(sym, {})[os.path.basename(path)] = body
    return table


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = collect(sys.argv[1]), collect(sys.argv[2])
    counts = {"same": 0, "differ": 0, "missing": 0}
    for sym in sorted(set(old) | set(new)):
        where = "%s -> %s" % (",".join(sorted(old.get(sym, {}))) or "-", ",".join(sorted(new.get(sym, {}))) or "-")
        if sym not in old or sym not in new:
            verdict = "missing"
        else:
            a, b = set(old[sym].values()), set(new[sym].values())
            verdict = "same" if a == b and len(a) == 1 else "differ"
            if verdict == "differ":
                what = [n for n, k in (("instructions", 0), ("descriptor", 1)) if {x[k] for x in a} != {x[k] for x in b}]
                where += "  (%s)" % (", ".join(what) or "copies on one side differ from each other")
        counts[verdict] += 1
        print("%-7s %s  [%s]" % (verdict, sym, where))
    print("kernels: %d same, %d differ, %d missing" % (counts["same"], counts["differ"], counts["missing"]))
    return 1 if counts["differ"] or counts["missing"] else 0


if __name__ == "__main__":
    sys.exit(main())
