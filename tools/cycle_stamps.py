#!/usr/bin/env python3
"""Reads the cycle stamps of a measurement build (mrcal_amd/csrc/cycle_stamps.hpp) from the text of a run on stdin:

    ts <kernel> <i>/<n>[ <j>/<m>] name=value name=value ...

and prints, per kernel and name, the count, median, minimum and maximum of the values. Other lines are passed over.
usage: MRCAL_AMD_LIB=mrcal_amd/libmrcal_amd_dev.so python tools/probe_asm_ts.py | python tools/cycle_stamps.py [--where I/N]
   --where I/N: only the lines of that reporter (0/1000: the first frame of 1000)"""
import re, statistics, sys

LINE = re.compile(r"^ts (\S+) (\d+/\d+)((?: \d+/\d+)?)((?: [^\s=]+=-?\d+)+)\s*$")

def parse(text):
    """-> [(kernel, "i/n", "j/m" or "", [(name, value), ...]), ...] in the order of the lines"""
    out = []
    for line in text.splitlines():
        m = LINE.match(line)
        if m is None: continue
        pairs = [(name, int(value)) for name, value in (p.split("=") for p in m.group(4).split())]
        out.append((m.group(1), m.group(2), m.group(3).strip(), pairs))
    return out

def summarize(records):
    """-> {(kernel, name): (count, median, min, max)}, keys in the order of first appearance"""
    values = {}
    for kernel, _, _, pairs in records:
        for name, value in pairs:
            values.setdefault((kernel, name), []).append(value)
    return {k: (len(v), statistics.median(v), min(v), max(v)) for k, v in values.items()}

def main(argv):
    where = argv[argv.index("--where") + 1] if "--where" in argv else None
    records = [r for r in parse(sys.stdin.read()) if where is None or r[1] == where]
    if not records:
        print("no cycle stamps in the input (a library built with a -D..._TS flag prints them: tools/README.md)")
        return 1
    print(f"{'kernel':<14} {'name':<18} {'count':>6} {'median':>14} {'min':>14} {'max':>14}")
    for (kernel, name), (count, median, lo, hi) in summarize(records).items():
        print(f"{kernel:<14} {name:<18} {count:>6} {median:>14.1f} {lo:>14} {hi:>14}")
    return 0

if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
