#!/usr/bin/env python
"""The route record of fm_end (GPU box): a fixed list of small mtm_find_matches calls, one context per dtype, chosen so that
consecutive calls walk the synchronising half's routes - candidates verified on the host, the device's hash verification,
the overflow ladder's steps (maps, three products, map scan, float64 kernel, grown lists), the back-off routes of the calls
that follow an overflow, the global extremum with and without the fused route, a 1-D map next to 2-D ones, the NMS entry.

    python tools/fm_end_routes.py --record tests/golden/fm_end_routes.json     # on the commit whose behaviour is the record
    python tools/fm_end_routes.py                                              # print the calls' records, one JSON line each
    python tools/fm_end_routes.py --kernel-names <kernel_trace.csv>            # kernel names of a rocprofv3 kernel trace of
                                                                               # this script, in dispatch order

tests/test_gpu_fm_end_routes.py replays the calls and compares field by field.  Images and templates are integer formulas
(no random generator, no file): every build sees the same bytes.
"""
import argparse
import csv
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for _p in (os.path.join(ROOT, "multitemplatematching-python_amd"),):
    if _p not in sys.path:
        sys.path.insert(0, _p)

ROWS, COLS = 96, 128
TH, TW = 12, 16
FIELDS = ("kernel_used", "f32_route", "f32_pieces", "hits_only", "ncc_launches", "sq_launches", "n_hits")


def _images():
    yy, xx = np.mgrid[0:ROWS, 0:COLS].astype(np.uint64)
    h = (yy * np.uint64(73856093)) ^ (xx * np.uint64(19349663))
    h = (h * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    noise = ((h >> np.uint64(13)) & np.uint64(0xFF)).astype(np.uint8)
    yi, xi = np.mgrid[0:ROWS, 0:COLS].astype(np.int64)
    tri = lambda v, p: np.abs(v % (2 * p) - p)                                     # noqa: E731
    smooth = (tri(3 * yi + 2 * xi, 47) + tri(5 * yi - 3 * xi, 31) * 2 + tri(yi * xi // 16 + xi, 23) * 3).astype(np.uint8)
    tile = ((yi % 4) * 37 + (xi % 4) * 59 + (yi % 4) * (xi % 4) * 11).astype(np.uint8)      # period 4 x 4: many equal bests
    return {"noise": noise, "smooth": smooth, "tile": tile}


def _templates(img):
    """three TH x TW cuts (exact copies exist: score 1) and one full-height, 5-wide cut (a 1-D map)"""
    cuts = [np.ascontiguousarray(img[y:y + TH, x:x + TW]) for y, x in ((7, 11), (40, 97), (ROWS - TH, COLS - TW))]
    tall = np.ascontiguousarray(img[:, 60:65])
    return cuts, tall


def _f32(a):
    return a.astype(np.float32) * np.float32(1.5) + np.float32(3.0)


def calls():
    """[(context, name, dict)]: option changes ("opt": [(option name, value)], applied first) and one search each."""
    L, G = "local", "global"
    u8 = [
        ("host verified", dict(img="noise", thr=0.5)),
        ("host verified, minima", dict(img="noise", thr=0.3, method=1)),
        ("host verified, constant border", dict(img="noise", thr=0.5, opt=[("OPT_PEAK_BORDER", 0)])),
        ("1-D map next to 2-D maps", dict(img="noise", thr=0.5, tall=True, opt=[("OPT_PEAK_BORDER", 1)])),
        ("device hash verify", dict(img="smooth", thr=-1.0)),
        ("nms entry", dict(img="noise", thr=0.5, nms=(0.25, -1))),
        ("nms entry, N_object", dict(img="smooth", thr=0.3, nms=(0.4, 2))),
        ("global, fused", dict(img="noise", mode=G)),
        ("global, extremum kernel", dict(img="noise", mode=G, opt=[("OPT_HITS_ONLY", 0)])),
        ("maps: candidates overflow 64", dict(img="smooth", thr=0.2, opt=[("OPT_HITS_ONLY", 1), ("OPT_HIT_CAPACITY", 64)])),
        ("back-off route", dict(img="smooth", thr=0.2)),
        ("back-off route, list of 16", dict(img="smooth", thr=0.2, opt=[("OPT_HIT_CAPACITY", 16)])),
        ("back-off route, few hits", dict(img="noise", thr=0.5)),
        ("back-off, 1-D map: full scan grown", dict(img="smooth", thr=0.2, tall=True, opt=[("OPT_HIT_CAPACITY", 16)])),
        ("back-off, nms", dict(img="smooth", thr=0.2, nms=(0.25, -1))),
        ("maps: candidates overflow 16", dict(img="smooth", thr=0.2, opt=[("OPT_HITS_ONLY", 1), ("OPT_HIT_CAPACITY", 16)])),
        ("maps written, full scan", dict(img="smooth", thr=0.6, opt=[("OPT_HITS_ONLY", 0), ("OPT_HIT_CAPACITY", 1 << 18)])),
        ("host verified again", dict(img="noise", thr=0.5, opt=[("OPT_HITS_ONLY", 1)])),
    ]
    reset16 = [("OPT_HITS_ONLY", 1), ("OPT_HIT_CAPACITY", 16)]
    f32 = [
        ("refined, host verified", dict(img="noise", thr=0.5)),
        ("refined, device verify", dict(img="smooth", thr=-1.0)),
    ] + [
        ("refined ladder, list of 16, thr %g" % t, dict(img="smooth", thr=t, opt=reset16)) for t in (0.999, 0.99, 0.95, 0.8, 0.5, 0.2)
    ] + [
        ("refined, the call after an overflow", dict(img="smooth", thr=0.2)),
        ("refined ladder, list of 64", dict(img="smooth", thr=0.7, opt=[("OPT_HITS_ONLY", 1), ("OPT_HIT_CAPACITY", 64)])),
        ("refined, 1-D map", dict(img="noise", thr=0.5, tall=True, opt=[("OPT_HITS_ONLY", 1), ("OPT_HIT_CAPACITY", 1 << 18)])),
        ("refined global", dict(img="noise", mode=G)),
        ("refined global, list of 16 overflows", dict(img="tile", mode=G, opt=reset16)),
        ("refined global, three products first", dict(img="tile", mode=G)),
        ("global, float64 kernel", dict(img="noise", mode=G, opt=[("OPT_HITS_ONLY", 0), ("OPT_HIT_CAPACITY", 1 << 18)])),
        ("raw sums, list of 16", dict(img="tile", thr=1.0, method=0, opt=reset16)),
        ("raw sums, host verified", dict(img="noise", thr=1.0, method=0, opt=[("OPT_HITS_ONLY", 1), ("OPT_HIT_CAPACITY", 1 << 18)])),
        ("nms entry", dict(img="noise", thr=0.5, nms=(0.25, -1))),
    ]
    defaults = dict(mode=L, method=5, tall=False, thr=0.0, opt=[], nms=None)
    return [(which, n, {**defaults, **d}) for which, lst in (("u8", u8), ("f32", f32)) for n, d in lst]


def run():
    """The calls' records: {"ctx", "name", FIELDS..., "hit_capacity", "n_returned", "hits_hex" | "hits_sha256"}."""
    from MTM import _lib
    imgs = _images()
    ctxs = {"u8": _lib.Context(0), "f32": _lib.Context(0)}
    recs = []
    try:
        for which, name, d in calls():
            c = ctxs[which]
            for opt, value in d["opt"]:
                c.set_option(getattr(_lib, opt), value)
            img = imgs[d["img"]]
            cuts, tall = _templates(img)
            tl = cuts + ([tall] if d["tall"] else [])
            if which == "f32":
                img, tl = _f32(img), [_f32(t) for t in tl]
            units = [(t, None) for t in tl]
            if d.get("nms"):
                hits = c.search_nms(units, img, d["method"], d["thr"], d["nms"][0], d["nms"][1])
            else:
                hits = c.search(units, img, d["method"], _lib.PEAKS_GLOBAL if d["mode"] == "global" else _lib.PEAKS_LOCAL, d["thr"])
            t = c.timing()
            rec = {"ctx": which, "name": name}
            rec.update({f: int(t[f]) for f in FIELDS})
            rec["hit_capacity"] = c.get_option(_lib.OPT_HIT_CAPACITY)
            rec["n_returned"] = int(len(hits))
            raw = hits.tobytes()
            if len(raw) <= 10 * _lib.HIT_DTYPE.itemsize:
                rec["hits_hex"] = raw.hex()
            else:
                rec["hits_sha256"] = hashlib.sha256(raw).hexdigest()
            recs.append(rec)
    finally:
        for c in ctxs.values():
            c.close()
    return recs


def kernel_names(trace_csv):
    with open(trace_csv, newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    return [r["Kernel_Name"] for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", help="write the records to this JSON file")
    ap.add_argument("--kernel-names", help="a rocprofv3 kernel trace (csv) of this script: print its kernel names in dispatch order")
    a = ap.parse_args()
    if a.kernel_names:
        for k in kernel_names(a.kernel_names):
            print(k)
        return
    recs = run()
    for r in recs:
        print(json.dumps(r))
    if a.record:
        with open(a.record, "w") as f:
            json.dump(recs, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
