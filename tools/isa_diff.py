#!/usr/bin/env python3
"""Per-kernel comparison of two device-assembly dumps (no GPU needed): did a source change move
any kernel's instruction stream?

    python tools/isa_diff.py A.s B.s [--lines 6]

A dump is the build's own command line (f16_jsb_amd/build.py) with `--cuda-device-only -S` in
place of `-shared -fPIC` (tools/isa_stats.py --dump writes one). Per kernel symbol the
instruction streams are compared as text, comments and directives stripped and the function
index taken out of local labels (.LBB<fn>_<n>: a kernel added or removed renumbers every later
one). Prints the kernels present in one dump only and the kernels that differ, with their first
differing lines; exit status 1 if a kernel present in both differs.
"""
from __future__ import annotations

import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_stats import kernel_spans  # noqa: E402

LOCAL = re.compile(r"\.L([A-Za-z_]+)\d+_(\d+)")


def streams(path):
    lines = open(path).read().splitlines()
    out = {}
    for name, (start, end) in kernel_spans(lines).items():
        body = []
        for l in lines[start + 1:end]:
            l = l.split(";")[0].strip()
            if not l or (l.startswith(".") and not l.endswith(":")):  # comment / directive
                continue
            body.append(LOCAL.sub(r".L\1_\2", " ".join(l.split())))
        out[name] = body
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    show = int(sys.argv[sys.argv.index("--lines") + 1]) if "--lines" in sys.argv else 6
    if "--lines" in sys.argv:
        args.remove(str(show))
    a, b = streams(args[0]), streams(args[1])
    for tag, only in (("A", sorted(set(a) - set(b))), ("B", sorted(set(b) - set(a)))):
        print("only in %s (%s): %d" % (tag, args[0 if tag == "A" else 1], len(only)))
        for k in only:
            print("  " + k)
    common = [k for k in a if k in b]
    differ = [k for k in common if a[k] != b[k]]
    print("common kernels: %d, identical: %d, differing: %d" % (len(common), len(common) - len(differ), len(differ)))
    for k in differ:
        x, y = a[k], b[k]
        i = next((j for j in range(min(len(x), len(y))) if x[j] != y[j]), min(len(x), len(y)))
        print("  %s: %d vs %d instructions and labels, first difference at %d" % (k, len(x), len(y), i))
        for j in range(i, i + show):
            print("    A %-60s | B %s" % (x[j] if j < len(x) else "", y[j] if j < len(y) else ""))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
