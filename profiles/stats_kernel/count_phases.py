#!/usr/bin/env python3
"""Static instruction counts of a stats_u8_kernel instantiation by phase, from the device assembly the build keeps
(csrc/build/mtm_launch-hip-amdgcn-amd-amdhsa-gfx950.s):  count_phases.py <file.s> <mangled-name prefix>

The row loop is the loop that holds the kernel's two barriers.  Phases: everything ahead of it (layout conversion and the
column-sum prologue, whose 32-row batches are unrolled), the loop up to the first barrier (slide loads, thread totals, wave
scans), between the barriers (offsets, prefix writes), behind the second (window sums, float64 statistics, stores, block
records, tail boxes, slide).  Classes: f64 = v_*_f64, dpp, lds = ds_*, vmem = global_*, valu = other v_*, salu = s_*."""
import re
import sys


def cls(op):
    if op.endswith("_dpp") or "_dpp" in op:
        return "dpp"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    if op.startswith("v_"):
        return "f64" if "f64" in op else "valu"
    return "salu"


def main(path, prefix):
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(prefix) and ":" in l)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[start:end]
    is_ins = lambda l: re.match(r"^\s+[a-z]+_[a-z0-9_]+", l) is not None          # noqa: E731
    bars = [i for i, l in enumerate(body) if l.strip().startswith("s_barrier")]
    assert len(bars) == 2, bars
    head = max(i for i in range(bars[0]) if "Loop Header" in body[i])
    label = body[head].split(":")[0]
    marks = [i for i, l in enumerate(body) if "Header=" + label.lstrip(".L") + " " in l or l.rstrip().endswith("Header=" + label.lstrip(".L"))]
    back = next((i for i in range(max(marks) + 1, len(body)) if body[i].startswith(".LBB")), len(body)) - 1    # end of the loop's last block
    spans = {"ahead of the row loop": (0, head), "loop: loads + scans": (head, bars[0]), "loop: offsets + prefix writes": (bars[0], bars[1]),
             "loop: statistics + records + slide": (bars[1], back + 1)}
    print(lines[start].split(":")[0])
    for name, (a, b) in spans.items():
        n = {}
        for l in body[a:b]:
            if is_ins(l):
                op = l.split()[0]
                if op in ("s_nop", "s_waitcnt"):
                    continue
                n[cls(op)] = n.get(cls(op), 0) + 1
        print("  %-36s total %4d  %s" % (name, sum(n.values()), "  ".join("%s %d" % kv for kv in sorted(n.items()))))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
