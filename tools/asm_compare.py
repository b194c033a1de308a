#!/usr/bin/env python3
"""Per-kernel comparison of two builds' device assembly (the csrc/build/*-gfx950.s listings build.py keeps).

Usage: tools/asm_compare.py DIR_A DIR_B [name filter, default ncc_mfma_kernel] [--units mtm_mfma_] [--by-kernel]

For every kernel whose name contains the filter, in every listing whose file name starts with the unit prefix and exists in
both directories, one line: the six resource figures of the code object's metadata (VGPRs, SGPRs, VGPR / SGPR spills, scratch
and LDS bytes), the instruction count, and the difference of the opcode histograms with the encoding suffix (_e32, _e64,
_dpp, _sdwa) dropped.  `=` where B equals A, else `A->B`.  Exit status 1 if any kernel differs or is missing on one side.
What a refactor of device code has to show: equivalent code, not byte-identical code - register numbers and the order of
independent instructions are free to move, the counts are not.
--by-kernel: kernels are paired by name across ALL listings of a directory, whichever unit holds them (a kernel that moved
between units; the unit column then names B's).  A kernel compiled into two units of one build counts as a difference.
"""
import collections
import os
import re
import sys

RES = [("vgpr", "vgpr_count"), ("sgpr", "sgpr_count"), ("vspill", "vgpr_spill_count"), ("sspill", "sgpr_spill_count"),
       ("scratch", "private_segment_fixed_size"), ("lds", "group_segment_fixed_size")]
_SUFFIX = re.compile(r"_(e32|e64|dpp|sdwa)\b")
_INSN = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")


def parse_listing(path):
    """{kernel: (resources dict, instruction count, Counter of opcodes)} of one listing."""
    hist, meta = {}, {}
    name = None                 # the function whose body is being read
    in_meta, entry = False, None
    with open(path) as f:
        for line in f:
            if in_meta:
                if line.startswith("  - ."):
                    entry = {}
                m = re.match(r"^(?:  - |    )\.(\w+):\s+(\S+)\s*$", line)
                if m and entry is not None:
                    entry[m.group(1)] = m.group(2)
                    if m.group(1) == "name":
                        meta[m.group(2)] = entry
                if line.startswith("amdhsa.target") or line.startswith("..."):
                    in_meta = False
                continue
            if line.startswith("amdhsa.kernels:"):
                in_meta = True
                continue
            m = re.match(r"^([A-Za-z_][\w$.]*):", line)
            if m and not line.startswith(".L"):
                name = m.group(1)
                hist[name] = collections.Counter()
                continue
            if name is None:
                continue
            if line.startswith(".Lfunc_end") or line.startswith("\t.section"):
                name = None
                continue
            m = _INSN.match(line)
            if m:
                hist[name][_SUFFIX.sub("", m.group(1))] += 1
    out = {}
    for k, e in meta.items():
        h = hist.get(k, collections.Counter())
        out[k] = ({short: int(e.get(key, -1)) for short, key in RES}, sum(h.values()), h)
    return out


def short_name(n):
    m = re.search(r"ncc_mfma_kernelI(.*?)EEv", n)
    if not m:
        return n[:90]
    v = re.findall(r"L[ib](n?\d+)E", m.group(1))
    return "ncc_mfma_kernel<" + ",".join(x.replace("n", "-") for x in v) + ">"


def main(argv):
    args = [a for a in argv[1:] if not a.startswith("--")]
    prefix = "mtm_mfma_"
    if "--units" in argv:
        prefix = argv[argv.index("--units") + 1]
        args.remove(prefix)
    if len(args) < 2:
        print(__doc__)
        return 2
    da, db = args[0], args[1]
    flt = args[2] if len(args) > 2 else "ncc_mfma_kernel"
    by_kernel = "--by-kernel" in argv
    listed = lambda d: sorted(f for f in os.listdir(d) if f.startswith(prefix) and f.endswith("-gfx950.s"))
    units = [f for f in listed(da) if os.path.exists(os.path.join(db, f))]
    n = bad = 0
    print("%-12s %-52s %s  %s  %s" % ("unit", "kernel", " ".join("%-8s" % s for s, _ in RES), "insns   ", "histogram delta (B - A)"))

    def merged(d):              # every kernel of every listing of `d`, and the unit that holds it
        out, where, twice = {}, {}, []
        for u in listed(d):
            for k, v in parse_listing(os.path.join(d, u)).items():
                if k in out:
                    twice.append(k)
                out[k], where[k] = v, u.split("-")[0].replace("mtm_", "").replace(".hip", "")
        return out, where, twice

    if by_kernel:
        (a_all, _, twice_a), (b_all, where_b, twice_b) = merged(da), merged(db)
        for k in twice_a + twice_b:
            bad += 1
            print("%-12s %-52s compiled into two units of %s" % ("", short_name(k), "A" if k in twice_a else "B"))
        pairs = [("", a_all, b_all)]
        units = listed(db)
    else:
        pairs = [(u.split("-")[0].replace("mtm_", ""), parse_listing(os.path.join(da, u)), parse_listing(os.path.join(db, u))) for u in units]
    for unit0, a, b in pairs:
        for k in sorted(set(a) | set(b)):
            unit = where_b.get(k, "-") if by_kernel else unit0
            if flt not in k:
                continue
            n += 1
            if k not in a or k not in b:
                bad += 1
                print("%-12s %-52s only in %s" % (unit, short_name(k), "A" if k in a else "B"))
                continue
            (ra, ca, ha), (rb, cb, hb) = a[k], b[k]
            cell = lambda x, y: "=%d" % x if x == y else "%d->%d" % (x, y)
            delta = {op: hb[op] - ha[op] for op in set(ha) | set(hb) if hb[op] != ha[op]}
            same = ra == rb and ca == cb and not delta
            bad += 0 if same else 1
            dtxt = "=" if not delta else " ".join("%s%+d" % (op, d) for op, d in sorted(delta.items()))
            print("%-12s %-52s %s  %-8s  %s" % (unit, short_name(k), " ".join("%-8s" % cell(ra[s], rb[s]) for s, _ in RES), cell(ca, cb), dtxt))
    print("%d kernels in %d units; %d differ" % (n, len(units), bad))
    return 1 if bad or not n else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
