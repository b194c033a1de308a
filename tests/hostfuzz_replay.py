"""
Replay of the host-layer differential fuzz (tests/golden/hostfuzz.json.gz, written by tests/golden/make_hostfuzz.py from
the unmodified reference) through this package, and the comparison rules; shared by the CPU replay (oracle engine stub)
and the GPU replay (the HIP kernels).

Rules: exception type and message equal (``cv2_error``: the reference's cv2 refused the input - a ValueError is enough);
warnings equal as a multiset; box and score types equal; findMatches as multisets; matchTemplates in order, hits of one
run of tied scores in any order among themselves, and where the order of tied scores changes what the reference kept, as
a valid greedy NMS of its recorded candidates with the same N_object cut; scores within 1e-6 (8-bit) / 1e-5 (otherwise)
relative to max(1, |score|).
"""
import gzip
import json
import math
import os
import warnings

import numpy as np

import hostfuzz_cases as HC
from helpers import GOLDEN_DIR

_FIXTURE = None


def load_fixture():
    global _FIXTURE
    if _FIXTURE is None:
        with gzip.open(os.path.join(GOLDEN_DIR, "hostfuzz.json.gz"), "rt") as f:
            _FIXTURE = json.load(f)
    return _FIXTURE


def _warnings_of(log):
    return [str(w.message) for w in log if os.path.basename(os.path.dirname(w.filename)) == "MTM"]


def outcome(fn, *a, **kw):
    """Run one package call -> the outcome in the fixture's form (hits are kept as returned)."""
    with warnings.catch_warnings(record=True) as log:
        warnings.simplefilter("always")
        try:
            res = fn(*a, **kw)
        except Exception as e:  # noqa: BLE001
            return {"kind": "error", "exc": [type(e).__name__, str(e)], "warnings": _warnings_of(log)}
    return {"kind": "hits", "res": res, "warnings": _warnings_of(log)}


def is_8bit(call):
    """Every array of the search is uint8 (exact arithmetic on both sides)."""
    lt, img = call["args"][0], call["args"][1]
    arrays = [img] + [t[1] for t in lt if isinstance(t, (tuple, list)) and len(t) >= 2]
    return all(isinstance(a, np.ndarray) and a.dtype == np.uint8 for a in arrays)


def _label_key(h):
    return (type(h[0]).__name__, repr(h[0]), tuple(int(v) for v in h[1]))


def _runs(want, g):
    """Split the reference's kept list (best first) into runs of tied scores: consecutive hits within g of each other."""
    runs = []
    for h in want:
        if runs and abs(h[2] - runs[-1][-1][2]) <= g:
            runs[-1].append(h)
        else:
            runs.append([h])
    return runs


def compare_hits(exp, got_res, call, *, ordered, tol):
    """Problems (strings) between the reference's recorded outcome `exp` and the package's returned hit list.
    matchTemplates (`ordered`): in order, where only hits of one run of tied scores (within the recorded tie band; for exact
    arithmetic equal scores of one template) may come in another order - the reference orders equal scores of a template
    by an unstable sort; where that order changes what is kept, the recorded candidates are the yardstick (valid_nms);
    N_object == 1 with other extrema within rounding of the best, any of those (top_ties).  findMatches: as multisets."""
    got = [[h[0], [int(v) for v in h[1]], float(np.float32(h[2]))] for h in got_res]
    want = exp["hits"]

    def same(g, w):
        return type(g[0]) is type(w[0]) and g[0] == w[0] and g[1] == w[1] and (
            g[2] == w[2] or (math.isnan(g[2]) and math.isnan(w[2])) or abs(g[2] - w[2]) <= tol * max(1.0, abs(w[2])))

    if "candidates" in exp:
        probs = valid_nms(got, exp, call, tol)
    elif "top_ties" in exp:         # N_object == 1, extrema of other templates within rounding of the best one
        probs = [] if len(got) == 1 and any(same(got[0], t) for t in exp["top_ties"]) else \
            ["%r is not one of the tied best hits %r" % (got, exp["top_ties"])]
    elif len(got) != len(want):
        probs = ["%d hits, reference %d" % (len(got), len(want))]
    else:
        probs = []
        band = exp.get("tie_band", 0.0)
        if ordered:
            segments, k = [], 0
            for run in _runs(want, band):
                segments.append((got[k:k + len(run)], run))
                k += len(run)
        else:
            segments = [(got, want)]
        for gs, ws in segments:
            # exact ties of different templates keep template order on both sides (the NMS sorts stably): only hits of one
            # template may swap places - with rounding (band > 0) any two of the run may
            if ordered and band == 0 and [_label_key(h)[:2] for h in gs] != [_label_key(h)[:2] for h in ws]:
                probs.append("labels %r, reference %r (at rank %d)" % ([h[0] for h in gs], [h[0] for h in ws], want.index(ws[0])))
                break
            gs, ws = sorted(gs, key=_label_key), sorted(ws, key=_label_key)
            bad = [(g, w) for g, w in zip(gs, ws) if not same(g, w)]
            if bad:
                probs.append("hit %r, reference %r (at rank %d)" % (bad[0][0], bad[0][1], want.index(ws[0]) if ordered else 0))
                break
    if got_res and "box_types" in exp:
        box_types = [type(v).__name__ for v in got_res[0][1]]
        want_types = list(exp["box_types"])
        # deliberate difference: the reference adds the searchBox offsets as given, so an ndarray searchBox makes x and y
        # numpy integers; this package always returns Python ints in boxes (MTM._to_hit_list)
        if isinstance(call["kwargs"].get("searchBox"), np.ndarray):
            want_types[:2] = ["int", "int"]
        if box_types != want_types:
            probs.append("box element types %s, reference %s" % (box_types, want_types))
        if type(got_res[0][2]).__name__ != exp["score_type"]:
            probs.append("score type %s, reference %s" % (type(got_res[0][2]).__name__, exp["score_type"]))
    return probs


def valid_nms(got, exp, call, tol):
    """The reference's kept list depends on the order of tied scores (overlapping ties, or an N_object cut inside a run
    of ties), so the package's list must be A greedy NMS of the same candidates, cut the same way: every hit a candidate
    with that score, best first, no two kept boxes overlapping by more than maxOverlap, as many hits as the reference
    (finite N_object: the cut), and every candidate passing the threshold that is better than the last kept hit (no cut:
    every one) either kept or overlapping a kept hit of at least its quality by more than maxOverlap."""
    from mtm_oracle import _rect_overlap
    candidates, want = exp["candidates"], exp["hits"]
    kw = call["kwargs"]
    method = int(kw.get("method", 5))
    max_overlap = float(np.float32(kw.get("maxOverlap", 0.25)))
    n_obj = kw.get("N_object", float("inf"))
    sign = -1.0 if method == 1 else 1.0
    if n_obj != float("inf") and len(got) != len(want):
        return ["%d hits, reference %d (N_object=%r)" % (len(got), len(want), n_obj)]
    pool = {}
    for h in candidates:
        pool.setdefault(_label_key(h), []).append(h[2])
    for h in got:
        if not any(abs(h[2] - s) <= tol * max(1.0, abs(s)) for s in pool.get(_label_key(h), [])):
            return ["hit %r is not a reference candidate with that score" % (h,)]
    q = [sign * h[2] for h in got]
    if any(a < b - tol for a, b in zip(q, q[1:])):
        return ["hits not best first"]
    for i, a in enumerate(got):
        for b in got[:i]:
            if float(_rect_overlap(a[1], b[1])) > max_overlap:
                return ["kept hits %r and %r overlap by more than %g" % (b, a, max_overlap)]
    thr = float(kw.get("score_threshold", 0.5))
    floor = -math.inf if (n_obj == float("inf") or not got) else q[-1] + tol
    kept = {_label_key(h) for h in got}
    for c in candidates:
        passes = (1 - c[2] > 1 - thr) if method == 1 else (c[2] > thr)
        if not passes or sign * c[2] <= floor or _label_key(c) in kept:
            continue
        if not any(sign * h[2] >= sign * c[2] - tol and float(_rect_overlap(c[1], h[1])) > max_overlap for h in got):
            return ["candidate %r passes the threshold, is not kept and no kept hit suppresses it" % (c,)]
    return []


def compare(exp, got, call, kind):
    if exp["kind"] in ("error", "cv2_error"):
        if got["kind"] != "error":
            return ["returned %d hits, reference raised %s" % (len(got["res"]), exp["exc"])]
        if exp["kind"] == "cv2_error":
            probs = [] if got["exc"][0] == "ValueError" else ["raised %s, reference's cv2 refused the input (ValueError wanted)" % got["exc"]]
        else:
            probs = [] if got["exc"] == exp["exc"] else ["raised %s, reference %s" % (got["exc"], exp["exc"])]
    elif got["kind"] != "hits":
        return ["raised %s, reference returned %d hits" % (got["exc"], len(exp.get("hits", [])))]
    elif kind == "map":
        probs = compare_map(exp["map"], got["res"], call)
    else:
        probs = compare_hits(exp, got["res"], call, ordered=(kind == "match"), tol=1e-6 if is_8bit(call) else 1e-5)
    if sorted(got["warnings"]) != sorted(exp["warnings"]):
        probs.append("warnings %s, reference %s" % (got["warnings"], exp["warnings"]))
    return probs


def compare_map(rec, m, call):
    probs = []
    if not isinstance(m, np.ndarray) or list(m.shape) != rec["shape"] or m.dtype.name != rec["dtype"]:
        return ["map %s, reference %s %s" % (HC._short(m), rec["dtype"], rec["shape"])]
    a = m.astype(np.float64)
    fin = np.isfinite(a)
    scale = max(1.0, float(np.abs(a[fin]).max(initial=0)))
    t = call["args"]
    tol = (1e-6 if all(x.dtype == np.uint8 for x in t) else 1e-5) * scale
    if int((~fin).sum()) != rec["n_nonfinite"]:
        probs.append("%d non-finite values, reference %d" % (int((~fin).sum()), rec["n_nonfinite"]))
    sub = a.ravel()[::rec["k"]]
    want = np.asarray(rec["every_k"], dtype=np.float64)
    bad = ~((sub == want) | (np.isnan(sub) & np.isnan(want)) | (np.abs(sub - want) <= tol))
    if sub.shape != want.shape or bad.any():
        probs.append("every %d-th value: %d differ beyond %.3g (first at %d)" % (rec["k"], int(bad.sum()), tol, int(np.argmax(bad))))
    if abs(float(a[fin].sum()) - rec["sum"]) > tol * max(1, a.size) or abs(float(np.abs(a[fin]).sum()) - rec["abs_sum"]) > tol * max(1, a.size):
        probs.append("sums %r / %r, reference %r / %r" % (float(a[fin].sum()), float(np.abs(a[fin]).sum()), rec["sum"], rec["abs_sum"]))
    for name, fn in (("argmax", np.nanargmax), ("argmin", np.nanargmin)):
        if rec[name] >= 0:      # the extreme VALUE must agree (the position may be another pixel of a near-tie)
            if abs(a.ravel()[rec[name]] - a.ravel()[int(fn(a))]) > tol:
                probs.append("%s at %d, reference %d" % (name, int(fn(a)), rec[name]))
    return probs


def check_digests(case_id, entry, inputs):
    got = HC.digests(inputs)
    assert got == entry["digests"], "case %s: the rebuilt inputs differ from the generator's (%s)" % (
        case_id, sorted(k for k in got if got[k] != entry["digests"].get(k)))


def replay_case(MTM, entry, border, via="direct", ctx=None, on_step=None):
    """Replay one case; returns a list of failure messages (empty: equal to the reference).  ``on_step(kind, outcome)``
    is called after every call."""
    case_id = entry["id"]
    kind, call, inputs = HC.build_case(case_id)
    check_digests(case_id, entry, inputs)
    out = []
    steps = call["steps"] if kind == "seq" else [dict(call, before=None)]
    recs = entry["steps"] if kind == "seq" else [entry]
    for n, (step, rec) in enumerate(zip(steps, recs)):
        if step.get("before") is not None:
            step["before"]()
        exp = rec["@any"] if "@any" in rec else rec["@" + border]
        skind = kind if kind != "seq" else ("match" if step["fn"] == "matchTemplates" else "find")
        if via == "matcher":
            got = _via_matcher(MTM, step, ctx)
        elif via == "sharded":
            got = _via_sharded(MTM, step)
        else:
            got = outcome(getattr(MTM, step["fn"]), *step["args"], **step["kwargs"])
        if on_step is not None:
            on_step(skind, got)
        if via == "matcher" and matcher_difference(step, got):
            continue
        probs = compare(exp, got, step, skind)
        if probs:
            out.append("case %s (stratum %s, %s, @%s, via %s%s): %s\n    reproduce: kind, call, inputs = "
                       "hostfuzz_cases.build_case(%r)  # %s" % (
                           case_id, entry["stratum"], HC.STRATUM_NAMES[entry["stratum"]], border, via,
                           ", step %d" % n if kind == "seq" else "", "; ".join(probs), case_id, HC.describe(step)))
    return out


_MATCHER_KW = ("method", "N_object", "score_threshold", "maxOverlap")


def _via_matcher(MTM, step, ctx):
    lt, img = step["args"]
    kw = step["kwargs"]
    ckw = {k: kw[k] for k in _MATCHER_KW if k in kw}

    def run():
        return MTM.TemplateMatcher(lt, context=ctx, **ckw).match(img, kw.get("searchBox"))
    return outcome(run)


def _via_sharded(MTM, step):
    from MTM.distributed import HitExchange, matchTemplates_sharded
    lt, img = step["args"]
    ex = HitExchange("custom", 0, 1, allgather_bytes=lambda payload: [payload])
    return outcome(matchTemplates_sharded, lt, img, ex, **step["kwargs"])


def matcher_difference(step, got):
    """TemplateMatcher's documented restriction (see its docstring): all templates of one pixel type.  A list that mixes
    them raises there and is matched by matchTemplates, so only that exact refusal of such a list is let through."""
    if got["kind"] != "error" or "needs templates of one pixel type" not in got["exc"][1]:
        return False
    lt, img = step["args"]
    kinds = {("u8" if (t[1].dtype == np.uint8 and img.dtype == np.uint8) else
              "u16" if (t[1].dtype == np.uint16 and img.dtype == np.uint16 and (len(t) < 3 or t[2] is None)) else "f32")
             for t in lt}
    return len(kinds) > 1
