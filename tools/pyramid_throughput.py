#!/usr/bin/env python3
"""Milliseconds per call of MTM.matchTemplatesPyramid against matchTemplates (exhaustive) and matchTemplatesDownscaled,
on the large shapes the coarse-to-fine search is for, one JSON line per shape: the coarse candidates the pyramid call
worked from and its recall - the fraction of matchTemplates' hits it reproduced exactly (label, box, float32 score).

Data from synth.py: a photograph-like image (smooth_u8) and templates cut from it (cut_templates), so every template
has an exact copy in the image.  Each shape is warmed up first (placement, buffers, code objects); the three calls are
interleaved within a repetition.

Usage: tools/pyramid_throughput.py [--reps 5] [--warmup 2] [--only NAME]
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

# name, (rows, cols), channels, templates, (template rows, cols), factor, N_object
SHAPES = [
    ("2160x3840_32t64_f2", (2160, 3840), 32, (64, 64), 2, float("inf")),
    ("2160x3840_32t64_f4", (2160, 3840), 32, (64, 64), 4, float("inf")),
    ("2048x2048_1t414x400_f4_n1", (2048, 2048), 1, (414, 400), 4, 1),
    ("4320x7680_16t128_f4", (4320, 7680), 16, (128, 128), 4, float("inf")),
]
MAX_CANDIDATES = 256


def workload(hw, n_templ, ths, seed=0):
    import synth
    img = synth.smooth_u8(seed, hw)
    rng = np.random.default_rng(seed + 1)
    units = []
    for i in range(n_templ):
        y, x = int(rng.integers(0, hw[0] - ths[0])), int(rng.integers(0, hw[1] - ths[1]))
        units.append(("t%d" % i, np.ascontiguousarray(img[y:y + ths[0], x:x + ths[1]])))
    return img, units


def _key(hits):
    return [(h[0], tuple(int(v) for v in h[1]), np.float32(h[2]).tobytes()) for h in hits]


def coarse_candidates(MTM, img, units, f, coarse_threshold):
    """What the pyramid call's coarse level proposes: per template the local maxima of its coarse map above the coarse
    threshold, at most MAX_CANDIDATES."""
    small = MTM.augment.downscale(img, f)
    su = [(n, MTM.augment.downscale(t, f)) for n, t in units]
    hits = MTM.findMatches(su, small, 5, score_threshold=coarse_threshold)
    per = {}
    for h in hits:
        per[h[0]] = per.get(h[0], 0) + 1
    return sum(min(MAX_CANDIDATES, v) for v in per.values())


def run_shape(MTM, spec, reps, warmup, thr=0.5):
    name, hw, n_templ, ths, f, n_obj = spec
    img, units = workload(hw, n_templ, ths)
    methods = {
        "pyramid": lambda: MTM.matchTemplatesPyramid(units, img, f, N_object=n_obj, score_threshold=thr,
                                                     max_candidates=MAX_CANDIDATES),
        "exhaustive": lambda: MTM.matchTemplates(units, img, N_object=n_obj, score_threshold=thr),
        "downscaled": lambda: MTM.augment.matchTemplatesDownscaled(units, img, f, N_object=n_obj, score_threshold=thr),
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
    exh = set(_key(results["exhaustive"]))
    pyr = set(_key(results["pyramid"]))
    return {
        "shape": name, "factor": f, "N_object": "inf" if n_obj == float("inf") else n_obj,
        "ms": {k: round(v, 3) for k, v in med.items()},
        "ms_min": {k: round(min(v), 3) for k, v in ms.items()},
        "pyramid_speedup_vs_exhaustive": round(med["exhaustive"] / med["pyramid"], 2),
        "coarse_candidates": coarse_candidates(MTM, img, units, f, thr - 0.1),
        "hits": {k: len(v) for k, v in results.items()},
        "recall": round(len(exh & pyr) / len(exh), 4) if exh else None,
        "pyramid_hits_not_exhaustive": len(pyr - exh),
        "reps": reps,
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None, help="run the one shape of this name (profiling runs)")
    args = ap.parse_args()
    import build as mtm_build
    mtm_build.build()
    import MTM
    for spec in SHAPES:
        if args.only and spec[0] != args.only:
            continue
        print(json.dumps(run_shape(MTM, spec, args.reps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
