#!/usr/bin/env python3
"""Milliseconds per call of three ways to get the 3 x 3 score neighbourhoods of a hit list and their sub-pixel positions,
one JSON line per workload:
  refine      - MTM.refineHits(templates, image, hits): one native call (mtm_hit_neighbourhoods) for every hit
  maps        - MTM.computeScoreMap per template the hits use, the neighbourhoods cut from the maps in numpy, then the fit
  crops       - MTM.computeScoreMap on each hit's (h + 2) x (w + 2) crop (clipped to the image), then the fit
The neighbourhood arrays of maps and crops are compared with refine's: equal bit for bit (uint8, uint16), or NaN in the
same places and the largest difference relative to max(1, |score|) (float32: computeScoreMap's float32 route is not the
oracle).

Workloads:
  S1  3840 x 2160 uint8, 32 templates 64 x 64, the hits of matchTemplates (about 2,000)
  S2  2048 x 2048 uint16, one 16 x 16 template, 20,000 random hits
  S3  1920 x 1080 float32, 8 templates 48 x 48, about 500 hits
Each method is warmed up first; medians over the repetitions.

Usage: tools/subpixel_throughput.py [--reps 3] [--warmup 1] [--only S1|S2|S3] [--skip-crops]
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multitemplatematching-python_amd"))


def _smooth(seed, hw):
    import synth
    return synth.smooth_u8(seed, hw)


def workload(name, seed=0):
    import MTM
    rng = np.random.default_rng(seed)
    if name == "S1":
        img = _smooth(seed + 1, (2160, 3840))
        templs = []
        for k in range(32):
            y, x = int(rng.integers(0, 2160 - 64)), int(rng.integers(0, 3840 - 64))
            templs.append(("t%d" % k, np.ascontiguousarray(img[y:y + 64, x:x + 64])))
        hits = MTM.matchTemplates(templs, img, score_threshold=0.45, maxOverlap=0.25)
        return templs, img, hits
    if name == "S2":
        img = (_smooth(seed + 2, (2048, 2048)).astype(np.uint16) * 257 +
               rng.integers(0, 256, size=(2048, 2048), dtype=np.uint16)).astype(np.uint16)
        t = np.ascontiguousarray(img[1000:1016, 700:716])
        n = 20000
        xs, ys = rng.integers(0, 2048 - 16 + 1, n), rng.integers(0, 2048 - 16 + 1, n)
        hits = [("a", (int(x), int(y), 16, 16), np.float32(0)) for x, y in zip(xs, ys)]
        return [("a", t)], img, hits
    img = _smooth(seed + 3, (1080, 1920)).astype(np.float32) / 255.0
    templs = []
    for k in range(8):
        y, x = int(rng.integers(0, 1080 - 48)), int(rng.integers(0, 1920 - 48))
        templs.append(("t%d" % k, np.ascontiguousarray(img[y:y + 48, x:x + 48])))
    hits = MTM.matchTemplates(templs, img, score_threshold=0.3, maxOverlap=0.1)
    return templs, img, hits


def _cut(smap, x, y):
    out = np.full((3, 3), np.nan, dtype=np.float32)
    y0, y1, x0, x1 = max(y - 1, 0), min(y + 2, smap.shape[0]), max(x - 1, 0), min(x + 2, smap.shape[1])
    out[y0 - y + 1:y1 - y + 1, x0 - x + 1:x1 - x + 1] = smap[y0:y1, x0:x1]
    return out


def by_maps(templs, img, hits):
    import MTM
    from MTM.subpixel import fit_offsets
    by = {t[0]: t[1] for t in templs}
    maps = {}
    nb = np.empty((len(hits), 3, 3), np.float32)
    for i, (label, (x, y, w, h), _) in enumerate(hits):
        if label not in maps:
            maps[label] = MTM.computeScoreMap(by[label], img, 5)
        nb[i] = _cut(maps[label], x, y)
    fit_offsets(nb, 5)
    return nb


def by_crops(templs, img, hits):
    import MTM
    from MTM.subpixel import fit_offsets
    by = {t[0]: t[1] for t in templs}
    H, W = img.shape[:2]
    nb = np.empty((len(hits), 3, 3), np.float32)
    for i, (label, (x, y, w, h), _) in enumerate(hits):
        y0, x0 = max(y - 1, 0), max(x - 1, 0)
        y1, x1 = min(y + h + 1, H), min(x + w + 1, W)
        m = MTM.computeScoreMap(by[label], img[y0:y1, x0:x1], 5)
        nb[i] = _cut(m, x - x0, y - y0)
    fit_offsets(nb, 5)
    return nb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default=None)
    ap.add_argument("--skip-crops", action="store_true")
    args = ap.parse_args()
    import MTM
    warnings.simplefilter("ignore")
    for name in ("S1", "S2", "S3"):
        if args.only and name != args.only:
            continue
        templs, img, hits = workload(name)
        methods = {"refine": lambda: MTM.hitNeighbourhoods(templs, img, hits, 5), "maps": lambda: by_maps(templs, img, hits)}
        if not args.skip_crops:
            methods["crops"] = lambda: by_crops(templs, img, hits)
        res = {}
        for k, fn in methods.items():
            for _ in range(args.warmup):
                res[k] = fn()
        refine_call = lambda: MTM.refineHits(templs, img, hits, 5)          # noqa: E731 (what the user calls)
        refine_call()
        times = {k: [] for k in methods}
        for _ in range(args.reps):
            for k, fn in methods.items():
                t0 = time.perf_counter()
                (refine_call if k == "refine" else fn)()
                times[k].append(1e3 * (time.perf_counter() - t0))
        nb = res["refine"]
        check = {}
        for k in methods:
            if k == "refine":
                continue
            if img.dtype == np.float32:
                ok = np.array_equal(np.isnan(nb), np.isnan(res[k]))
                fin = ~np.isnan(nb)
                err = float(np.max(np.abs(nb[fin].astype(np.float64) - res[k][fin]) /
                                   np.maximum(1.0, np.abs(res[k][fin].astype(np.float64))))) if fin.any() else 0.0
                check[k] = {"nan_equal": bool(ok), "max_rel_err": err}
            else:
                check[k] = bool(np.array_equal(nb, res[k], equal_nan=True))
        ms = {k: round(statistics.median(v), 3) for k, v in times.items()}
        line = {"workload": name, "image": list(img.shape), "dtype": str(img.dtype), "templates": len(templs),
                "hits": len(hits), "ms": ms, "speedup": {k: round(ms[k] / ms["refine"], 2) for k in ms if k != "refine"},
                "equal": check}
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
