"""Summarise hipcc -Rpass-analysis=kernel-resource-usage output (make -C .../csrc asm).

    python tools/resource_usage.py [FILE.resource.txt]          one file's kernels
    python tools/resource_usage.py --compare DIR_A DIR_B        every kernel of two trees' build/asm directories:
        the kernels present in both with different VGPRs / AGPRs / scratch / occupancy / LDS, the kernels only in
        one of them, and (--grep RE) the kernels of DIR_B whose demangled-ish name matches RE
"""
import glob
import os
import re
import sys

KEYS = (("VGPRs:", "v"), ("AGPRs:", "a"), ("ScratchSize", "scr"), ("Occupancy", "occ"), ("LDS Size", "lds"))


def parse(path):
    rows, cur = [], None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)}
            rows.append(cur)
            continue
        for key, lab in KEYS:
            if cur is not None and key in line:
                cur[lab] = line.split(":")[-1].split("[")[0].strip()
    return rows


def fmt(r):
    return "v=%-4s a=%-4s scr=%-4s occ=%-2s lds=%s" % tuple(r.get(k) for _, k in KEYS)


def tree(d):
    out = {}
    for f in sorted(glob.glob(os.path.join(d, "*.resource.txt"))):
        for r in parse(f):
            out[r["name"]] = dict(r, unit=os.path.basename(f)[:-len(".resource.txt")])
    return out


def compare(da, db, pattern):
    a, b = tree(da), tree(db)
    both = sorted(set(a) & set(b))
    diff = [n for n in both if any(a[n].get(k) != b[n].get(k) for _, k in KEYS)]
    print("kernels: %d in A, %d in B, %d in both; %d of those differ in VGPRs / AGPRs / scratch / occupancy / LDS"
          % (len(a), len(b), len(both), len(diff)))
    for n in diff:
        print("DIFFERS %s\n    A %s\n    B %s" % (n, fmt(a[n]), fmt(b[n])))
    for tag, x, y in (("only in A", a, b), ("only in B", b, a)):
        only = sorted(set(x) - set(y))
        by_unit = {}
        for n in only:
            by_unit[x[n]["unit"]] = by_unit.get(x[n]["unit"], 0) + 1
        print("%s: %d %s" % (tag, len(only), by_unit if only else ""))
    if pattern:
        print("kernels of B matching %r:" % pattern)
        for n in sorted(b):
            if re.search(pattern, n):
                print("  %-12s %s  %s" % (b[n]["unit"], fmt(b[n]), n))
    return len(diff)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--compare":
        pattern = sys.argv[sys.argv.index("--grep") + 1] if "--grep" in sys.argv else None
        sys.exit(1 if compare(sys.argv[2], sys.argv[3], pattern) else 0)
    path = sys.argv[1] if len(sys.argv) > 1 else \
        "omnidirectional_collaborative_filtering_amd/csrc/build/asm/ocf_gemm.resource.txt"
    for r in parse(path):
        n = re.sub(r"_ZN3ocf11gemm_kernelI", "gemm<", r["name"])[:60]
        print("%-60s %s" % (n, fmt(r)))


if __name__ == "__main__":
    main()
