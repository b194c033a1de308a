"""
Differential fuzz of the host layer: the expected outcomes.  Run in the BUILD CONTAINER only, like make_golden.py:

    PYTHONDONTWRITEBYTECODE=1 /opt/conda/bin/python3.9 tests/golden/make_hostfuzz.py

Every case of tests/hostfuzz_cases.py goes through the UNMODIFIED reference package (imported from /root/reference with
tests/golden/cv2_standin on the path: the cv2 arithmetic is the oracle's, the orchestration, the peak finders of
scikit-image 0.18.3 / scipy and the NMS hand-off are the reference's own).  Recorded per case: the outcome kind (hits /
error / cv2_error - the stand-in refused what real cv2.matchTemplate rejects), the hit list, the Python types of a box and
a score, the exception, the warnings in order, and for computeScoreMap checksums and every k-th element of the map.
Local-extrema cases are recorded under scikit-image 0.18.3's border rule ("@constant") and under make_golden's
nearest_border() patch ("@nearest", the library's default).

The reference's thread pool is held to one worker (os.cpu_count patched in this process) so that its cross-template hit
order is template order.  Cases whose maps (other than exact ones: 8-bit, or integer sums) come within
g = 1e-5 * max(1, max|map|) of the threshold, have a border value within g of 0, or have a peak with a 3x3 neighbour within
g, are redrawn (case id + ".d<n>").  matchTemplates records its tie band g (0 for exact arithmetic) and, for
N_object == 1, the per-template extrema within g of the best (top_ties: rounding may pick any of them).  Where the
kept list depends on the order of tied scores within one template (scikit-image's unstable argsort; or, with rounding, of
any two scores within g) - such candidates overlapping by more than maxOverlap, or an N_object cut between two of them -
every pre-NMS candidate is stored too.
Writes tests/golden/hostfuzz.json.gz; the output is deterministic.
"""
import contextlib
import gzip
import io
import json
import os
import sys
import traceback
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "cv2_standin"))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, TESTS)
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import cv2  # the stand-in  # noqa: E402
import MTM  # the unmodified reference  # noqa: E402
import hostfuzz_cases as HC  # noqa: E402

from border_rules import nearest_border  # noqa: E402
from mtm_oracle import _rect_overlap  # noqa: E402  (cv2.dnn.NMSBoxes' overlap, as the stand-in runs it)

assert MTM.__file__.startswith("/root/reference"), MTM.__file__

os.cpu_count = lambda: 2        # the reference's pool: round(cpu_count * .5) = 1 worker -> hits in template order
warnings.simplefilter("always")

MAX_DRAWS = 12
MAP_SAMPLES = 64
_STANDIN_FILES = (os.path.basename(cv2.__file__), "mtm_oracle.py")

_maps = []                      # every map cv2.matchTemplate produced in the current call, with the image dtype
_real_match = cv2.matchTemplate


def _integral(a):
    a = np.asarray(a)
    return a.dtype.kind in "biu" or bool(np.all(a == np.round(a)))


def _recording_match(image, templ, method, result=None, mask=None):
    """cv2.matchTemplate, remembering the map and whether its arithmetic is exact: 8-bit, an all-zero mask (every sum
    is 0), or integer pixels under the unnormalised TM_SQDIFF / TM_CCORR without a mask with every value below 2^24 (the
    float32 sums are then integers)."""
    out = _real_match(image, templ, method, result, mask)
    exact = np.asarray(image).dtype == np.uint8 or (mask is not None and not np.any(mask)) or (
        method in (0, 2) and mask is None and _integral(image) and _integral(templ)
        and float(np.abs(out).max(initial=0)) < 2 ** 24)
    _maps.append((exact, out))
    return out


cv2.matchTemplate = _recording_match


def f32(x):
    return float(np.float32(x))


def hits_json(hits):
    return [[h[0], [int(v) for v in h[1]], f32(h[2])] for h in hits]


def _mtm_warnings(log):
    return [str(w.message) for w in log if os.path.basename(os.path.dirname(w.filename)) == "MTM"]


def run(fn, args, kwargs):
    """One reference call -> the recorded outcome."""
    del _maps[:]
    with warnings.catch_warnings(record=True) as log:
        warnings.simplefilter("always")
        try:
            res = getattr(MTM, fn)(*args, **kwargs)
        except Exception as e:  # noqa: BLE001
            files = [os.path.basename(f.filename) for f in traceback.extract_tb(e.__traceback__)]
            kind = "cv2_error" if any(f in _STANDIN_FILES for f in files) else "error"
            return {"kind": kind, "exc": [type(e).__name__, str(e)], "warnings": _mtm_warnings(log)}
    out = {"kind": "hits", "warnings": _mtm_warnings(log)}
    if fn == "computeScoreMap":
        out["map"] = map_record(res)
        return out
    out["hits"] = hits_json(res)
    if res:
        out["box_types"] = [type(v).__name__ for v in res[0][1]]
        out["score_type"] = type(res[0][2]).__name__
    return out


def map_record(m):
    m64 = m.astype(np.float64)
    fin = np.isfinite(m64)
    k = max(1, m.size // MAP_SAMPLES)
    return {"shape": list(m.shape), "dtype": m.dtype.name, "sum": float(m64[fin].sum()), "abs_sum": float(np.abs(m64[fin]).sum()),
            "n_nonfinite": int((~fin).sum()),
            "argmax": int(np.nanargmax(m64)) if fin.any() else -1, "argmin": int(np.nanargmin(m64)) if fin.any() else -1,
            "k": k, "every_k": [f32(v) for v in m.ravel()[::k]]}


def guard(kwargs):
    """A non-exact map with a value within g of the threshold, or a border value within g of 0 (scikit-image 0.18.3's
    zero padding is a neighbour of every border pixel): which side it falls on is decided by rounding."""
    thr = kwargs.get("score_threshold", 0.5)
    reject = False
    for exact, m in _maps:
        fin = m[np.isfinite(m)].astype(np.float64)
        if exact or fin.size == 0:
            continue
        g = 1e-5 * max(1.0, float(np.abs(fin).max()))
        if np.any(np.abs(fin - float(thr)) <= g):
            reject = True
        rim = np.concatenate([m[0], m[-1], m[:, 0], m[:, -1]]).astype(np.float64)
        if np.any(np.abs(rim[np.isfinite(rim)]) <= g):
            reject = True
    return reject


def neighbour_reject(maps, cands):
    """A non-8-bit peak with a 3x3 neighbour within g: its being a peak is decided by rounding."""
    for (exact, m), peaks in zip(maps, cands):
        if exact or not peaks:
            continue
        a = m.astype(np.float64)
        fin = a[np.isfinite(a)]
        g = 1e-5 * max(1.0, float(np.abs(fin).max())) if fin.size else 0.0
        for y, x in peaks:
            v = a[y, x]
            nb = a[max(0, y - 1):y + 2, max(0, x - 1):x + 2]
            if int((np.abs(nb - v) <= g).sum()) > 1:
                return True
    return False


def tie_band(scores, exact):
    """g for scores: two scores within it are ties (exact arithmetic: only equal scores are)."""
    return 0.0 if exact or not scores else 1e-5 * max(1.0, max(abs(v) for v in scores))


def order_ambiguous(cands, kept_all, n_kept, max_overlap, g):
    """Whether the kept list depends on an order the two sides need not share.  Equal scores of DIFFERENT templates keep
    template order in both (one worker here; the NMS sorts stably); equal scores of one template come in the order of
    scikit-image's unstable argsort, and with rounding (g > 0) any two scores within g may swap.  The order matters for
    two such candidates overlapping by more than max_overlap (which one is kept decides what else is), or for an N_object
    cut between two such kept hits (`kept_all`: the uncut NMS result, `n_kept`: what the cut left)."""
    def swappable(a, b):
        return abs(a[2] - b[2]) <= g and (g > 0 or (type(a[0]), repr(a[0])) == (type(b[0]), repr(b[0])))

    by_score = sorted(cands, key=lambda h: h[2])
    for i, a in enumerate(by_score):
        for b in by_score[i + 1:]:
            if b[2] - a[2] > g:
                break
            if swappable(a, b) and float(_rect_overlap(a[1], b[1])) > max_overlap:
                return True
    if 0 < n_kept < len(kept_all):
        edge = kept_all[n_kept - 1][2]
        before = [h for h in kept_all[:n_kept] if abs(h[2] - edge) <= g]
        after = [h for h in kept_all[n_kept:] if abs(h[2] - edge) <= g]
        return any(swappable(a, b) for a in before for b in after)
    return False


def search_case(kind, call):
    """Outcomes of a find / match call under both border rules, plus the guard decisions."""
    fn, args, kw = call["fn"], call["args"], call["kwargs"]
    rec = {}
    reject = False
    ambiguous = False
    n_obj = kw.get("N_object", float("inf"))
    local = not (n_obj == 1)
    pre_kw = {k: v for k, v in kw.items() if k != "maxOverlap"}
    for border in ("constant", "nearest"):
        with (nearest_border() if border == "nearest" else contextlib.nullcontext()):
            out = run(fn, args, kw)
            rec["@" + border] = out
            if out["kind"] != "hits":
                continue
            # pre-NMS candidates (what findMatches returns) and the maps behind them
            pre = run("findMatches", args, pre_kw)
            maps = list(_maps)
            if pre["kind"] != "hits":
                continue
            kept_all = run(fn, args, dict(kw, N_object=float("inf")))["hits"] if (kind == "match" and local) else None
        exact = all(e for e, _ in maps)
        del _maps[:]
        _maps.extend(maps)
        if local and guard(kw):
            reject = True
        # peaks per map: the candidates of each template, in map coordinates
        lt = args[0]
        sb = kw.get("searchBox")
        xo, yo = (int(sb[0]), int(sb[1])) if sb is not None else (0, 0)
        labels = [t[0] for t in lt]
        cands = [[] for _ in maps]
        if local and len(maps) == len(lt) and len(set(map(repr, labels))) == len(labels):
            for h in pre["hits"]:
                idx = [repr(x) for x in labels].index(repr(h[0]))
                cands[idx].append((h[1][1] - yo, h[1][0] - xo))
            if neighbour_reject(maps, cands):
                reject = True
        if kind != "match":
            continue
        g = tie_band([h[2] for h in pre["hits"]], exact)
        out["tie_band"] = g
        if not local:
            # N_object == 1: the first best of the per-template extrema (python max / min), the same rule in both; only
            # another extremum within rounding of the best could take its place: those are recorded
            best = out["hits"][0][2] if out["hits"] else None
            top = [h for h in pre["hits"] if best is not None and abs(h[2] - best) <= g]
            if g > 0 and len(top) > 1:
                out["top_ties"] = top
        elif order_ambiguous(pre["hits"], kept_all, len(out["hits"]), float(np.float32(kw.get("maxOverlap", 0.25))), g):
            out["candidates"] = pre["hits"]
            ambiguous = True
    return rec, reject, ambiguous


def seq_case(call):
    steps = []
    for s in call["steps"]:
        if s["before"] is not None:
            s["before"]()
        rec, _, _ = search_case("match" if s["fn"] == "matchTemplates" else "find", s)
        steps.append(rec)
    return steps


def main():
    cases = {}
    rejected = {s: 0 for s in HC.STRATA}
    kinds = {}
    for base in HC.case_ids():
        for draw in range(MAX_DRAWS):
            cid = base if draw == 0 else "%s.d%d" % (base, draw)
            kind, call, inputs = HC.build_case(cid)
            entry = {"stratum": base[0], "kind": kind, "digests": HC.digests(inputs), "call": HC.describe(call)}
            if kind == "seq":
                entry["steps"] = seq_case(call)
                break
            if kind == "map":
                entry["@any"] = run(call["fn"], call["args"], call["kwargs"])
                break
            rec, reject, ambiguous = search_case(kind, call)
            entry.update(rec)
            if not reject:
                break
            rejected[base[0]] += 1
        else:
            raise SystemExit("case %s: no acceptable draw in %d" % (base, MAX_DRAWS))
        cases[base] = dict(entry, id=cid)
        k = (entry.get("@nearest") or entry.get("@any") or entry["steps"][0]["@nearest"])["kind"]
        kinds[k] = kinds.get(k, 0) + 1
    doc = {"cases": cases, "versions": dict(numpy=np.__version__, skimage=__import__("skimage").__version__,
                                            scipy=__import__("scipy").__version__, MTM=MTM.__version__)}
    payload = json.dumps(doc, sort_keys=True, separators=(",", ":")).encode()
    buf = io.BytesIO()
    with gzip.GzipFile(filename="", mode="wb", fileobj=buf, mtime=0, compresslevel=9) as gz:
        gz.write(payload)
    path = os.path.join(HERE, "hostfuzz.json.gz")
    with open(path, "wb") as f:
        f.write(buf.getvalue())
    counts = {s: sum(1 for c in cases.values() if c["stratum"] == s) for s in HC.STRATA}
    n_steps = sum(len(c["steps"]) for c in cases.values() if c["kind"] == "seq")
    print("wrote %s: %d cases, %d bytes" % (path, len(cases), len(buf.getvalue())))
    for s, n in counts.items():
        print("  %s %-20s %4d cases  %3d rejected draws" % (s, HC.STRATUM_NAMES[s], n, rejected[s]))
    n_match = sum(1 for c in cases.values() if c["kind"] == "match" and c["@nearest"]["kind"] == "hits")
    n_amb = sum(1 for c in cases.values() if "candidates" in c.get("@nearest", {}))
    print("  memo sequence steps: %d;  outcome kinds: %s;  matchTemplates cases with hits: %d, of them tie-order "
          "ambiguous (compared as a valid NMS of the candidates): %d" % (n_steps, kinds, n_match, n_amb))


if __name__ == "__main__":
    main()
