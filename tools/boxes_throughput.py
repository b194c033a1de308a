#!/usr/bin/env python3
"""Milliseconds per call, from numpy arrays to hit lists, of four ways to search many small boxes of one image, one JSON
line per workload:
  loop       - [matchTemplates(subset_i, image, searchBox=box_i) for each box]: what a user writes without the new calls
  boxes      - matchTemplatesInBoxes(templates, image, searchBoxes)
  matcher    - TemplateMatcher(templates).match_boxes(image, searchBoxes): templates resident across calls
  full_image - one matchTemplates(distinct templates, image) over the whole image (searches everywhere; its hits outside
               the boxes would still have to be filtered out - not counted here)
The boxes' results are checked equal to the loop's (labels, boxes, float32 score bits).

Data from synth.py: a photograph-like image (smooth_u8; uint16 = 257 x that plus noise in the low byte) with the boxes
placed at random and each box's template cut from the image inside it, so every box holds an exact copy.  Each method is
warmed up first; the four calls are interleaved within a repetition; medians over the repetitions.

Usage: tools/boxes_throughput.py [--reps 5] [--warmup 2] [--only A|B|C|D]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multitemplatematching-python_amd"))

# name, (rows, cols), channels, dtype, boxes, box side, distinct templates, (template rows, cols), templates per box
WORKLOADS = [
    ("A", (1080, 1920), 1, "uint8", 256, 96, 256, (32, 32), 1),
    ("B", (2160, 3840), 3, "uint8", 64, 160, 4, (48, 48), 4),
    ("C", (2048, 2048), 1, "uint16", 512, 48, 1, (16, 16), 1),
    ("D", (2048, 2048), 1, "uint8", 1, 600, 1, (414, 400), 1),
]


def workload(spec, seed=0):
    import synth
    name, hw, chans, dtype, n_boxes, side, n_templ, ths, per_box = spec
    planes = [synth.smooth_u8(seed + c, hw) for c in range(chans)]
    img = planes[0] if chans == 1 else np.ascontiguousarray(np.stack(planes, axis=2))
    rng = np.random.default_rng(seed + 10)
    if dtype == "uint16":
        img = (img.astype(np.uint16) * 257 + rng.integers(0, 64, size=img.shape, dtype=np.uint16)).astype(np.uint16)
    boxes = [(int(rng.integers(0, hw[1] - side)), int(rng.integers(0, hw[0] - side)), side, side) for _ in range(n_boxes)]
    templs = []
    for i in range(n_templ):
        x, y, _, _ = boxes[i % n_boxes]
        ty, tx = y + int(rng.integers(0, side - ths[0] + 1)), x + int(rng.integers(0, side - ths[1] + 1))
        templs.append(("t%d" % i, np.ascontiguousarray(img[ty:ty + ths[0], tx:tx + ths[1]])))
    if per_box == n_templ:
        regions = boxes                                            # every template in every box
    else:
        regions = [(b, [i % n_templ]) for i, b in enumerate(boxes)]    # box i with its own template
    return img, templs, regions


def _key(hits):
    return [(h[0], tuple(int(v) for v in h[1]), np.float32(h[2]).tobytes()) for h in hits]


def run(MTM, spec, reps, warmup, thr=0.5):
    img, templs, regions = workload(spec)

    def loop():
        out = []
        for r in regions:
            box, idx = (r[0], r[1]) if len(r) == 2 else (r, None)
            sub = templs if idx is None else [templs[j] for j in idx]
            out.append(MTM.matchTemplates(sub, img, score_threshold=thr, searchBox=box))
        return out

    matcher = MTM.TemplateMatcher(templs, score_threshold=thr)
    methods = {
        "loop": loop,
        "boxes": lambda: MTM.matchTemplatesInBoxes(templs, img, regions, score_threshold=thr),
        "matcher": lambda: matcher.match_boxes(img, regions),
        "full_image": lambda: MTM.matchTemplates(templs, img, score_threshold=thr),
    }
    results = {}
    for k, fn in methods.items():
        for _ in range(warmup):
            results[k] = fn()
    ms = {k: [] for k in methods}
    for _ in range(reps):
        for k, fn in methods.items():
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    equal = all(_key(a) == _key(b) for a, b in zip(results["boxes"], results["loop"])) and \
        all(_key(a) == _key(b) for a, b in zip(results["matcher"], results["loop"]))
    name, hw, chans, dtype, n_boxes, side, n_templ, ths, per_box = spec
    return {
        "workload": name, "image": "%dx%dx%d %s" % (hw[0], hw[1], chans, dtype), "boxes": n_boxes, "box": side,
        "templates": n_templ, "template": "%dx%d" % ths, "templates_per_box": per_box,
        "ms": {k: round(v, 3) for k, v in med.items()},
        "ms_min": {k: round(min(v), 3) for k, v in ms.items()},
        "speedup_vs_loop": {k: round(med["loop"] / med[k], 2) for k in ("boxes", "matcher", "full_image")},
        "hits": {k: sum(len(h) for h in v) if k != "full_image" else len(v) for k, v in results.items()},
        "equal_to_loop": equal,
        "reps": reps,
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None, help="run the one workload of this name (profiling runs)")
    args = ap.parse_args()
    import build as mtm_build
    mtm_build.build()
    import MTM
    for spec in WORKLOADS:
        if args.only and spec[0] != args.only:
            continue
        print(json.dumps(run(MTM, spec, args.reps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
