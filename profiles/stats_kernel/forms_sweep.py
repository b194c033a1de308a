#!/usr/bin/env python3
"""Times stats_u8_kernel in every form on the statistics launches of the headline call (3840x2160, 64x64 window, tail split 42,
first band 68 units) and of cfg2 (1920x1080), through mtm_debug_window_stats: HIP events around the launch, 6 calls per
cell, the first dropped, min / median of the rest in microseconds.  Run from the repository root on the GPU:
    python profiles/stats_kernel/forms_sweep.py [first-band units]
One line per launch; a cell reads  f<form asked>(<form that ran>)=min/median  - f0 is the launcher's own choice, f1 = 8 rows
per work-group, f2 = 4 rows.  "conv": the launch converts the band's image rows on the way, as the banded upload has it do."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "multitemplatematching-python_amd"))
import numpy as np  # noqa: E402
from MTM import _lib  # noqa: E402

ctx = _lib.Context(0)
rng = np.random.default_rng(1)
img4k = rng.integers(0, 256, (2160, 3840), dtype=np.uint8)
imghd = rng.integers(0, 256, (1080, 1920), dtype=np.uint8)
b0 = int(sys.argv[1]) if len(sys.argv) > 1 else 68
launches = [("4k_band0_conv", img4k, (0, b0), (0, b0 * 8 + 63)), ("4k_band1_conv", img4k, (b0, 263), (b0 * 8 + 63, 2160)),
            ("4k_whole", img4k, None, None), ("hd_whole(cfg2)", imghd, None, None),
            ("4k_units_0_32", img4k, (0, 32), None), ("4k_units_0_64", img4k, (0, 64), None),
            ("4k_units_0_128", img4k, (0, 128), None), ("4k_units_0_160", img4k, (0, 160), None)]
for name, img, units, conv in launches:
    cells = []
    for form in range(0, len(_lib.STATS_FORMS) + 1):
        ts = []
        for rep in range(6):
            r = ctx.debug_window_stats(img, 64, 64, 1, form=form, planes=("t0", "sq", "blk"), tail_s=42, units=units, convert_rows=conv)
            ts.append(r["info"]["kernel_ns"] / 1000.0)
        ts = sorted(ts[1:])
        cells.append("f%d(%d)=%.1f/%.1f" % (form, r["info"]["form"], ts[0], ts[len(ts) // 2]))
    n_units = 263 if img is img4k else 128
    u = units if units else (0, n_units)
    print(name, "work-groups at 8 rows:", r["info"]["grid_x"] * (u[1] - u[0]), " us min/median:", "  ".join(cells), flush=True)
