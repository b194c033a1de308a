"""
The float32 screen (ncc_bf16_kernel + the float64 chain behind it) on scaled, huge, tiny and non-finite scenes (-m gpu).

What MTM_OPT_F32_MFMA = 1 returns is the float64 kernel's record, bit for bit - while every output's bf16 score is within
the bound M of the exact one AND every output that could pass is listed.  tests/test_gpu_f32_geometry.py checks that on
values between 1e-3 and 1e3.  Here: the same scenes times 2^40, 2^-20, 2^-40 (in range: the whole contract, maps included),
times 2^60 and 2^-60 (`huge`: the float32 accumulators overflow; `tiny`: cv2's absolute DBL_EPSILON rule makes every
template constant under TM_CCOEFF_NORMED) and `nonfinite`: exact copies of template 0 planted beside a NaN, a +inf and a
-inf (tests/f32_model.py::range_scene).  The project's standard outside the reference's own range is its float64 kernel.

Four mechanisms could lose an output whose own window and statistics are clean.  Before the rule below the first two lost
the copies of `nonfinite` on every cell and the third the records of `huge` on two of six (where a sum came out NaN, not
+inf); the fourth is harmless:

  1. padded taps: the taps w .. 32 nkb - 1 of a template row are zero pieces that multiply the pixels right of the window;
     0 * inf = NaN in the accumulator (copy b);
  2. the tile constant: one non-finite sample of the 8 x 8 grid makes every accumulator of the 128 x 4 tile NaN (copy a);
  3. float32 accumulation: near 2^60 the centred products exceed FLT_MAX (`huge`);
  4. bf16_rne on a NaN whose payload carries into the exponent (-0.0): harmless - the window that holds it has NaN
     statistics, which take it to the exact test (pixel d); pinned in tests/test_f32_model_cpu.py.

The rule ("float32 images"): an output whose accumulator or bound is not finite cannot be screened - in
threshold modes it is listed, in global-extremum and map mode it takes the call to the float64 kernel (route 3).

Per cell, scene and method 5, 3, 1 (signed scenes: 5, 3 - TM_SQDIFF_NORMED saturates on zero-mean noise):

  1. the default route's records (MTM_OPT_F32_MFMA = 1, set on the context) equal the float64 kernel's (bytes of the whole
     record) by local extrema hits-only, local extrema with maps in memory, local extrema by the map scan (a context whose
     candidate list has just overflowed: route 2, or 3 where the rule sends it on) and global extremum; thresholds 0.9
     (methods 5, 3) and 0.1 (method 1);
  2. `nonfinite`: the float64 kernel's records hold the copies a, b, c at window_scores' score - asserted first;
  3. in-range scenes: the kernel's maps (three piece products and one) against model_scores to accum_map and against the
     direct sums to bound_map, at least 99 % of every map compared;
  4. `huge`, `tiny`, `nonfinite`: the same comparison where the model applies (no float32 overflow possible, outside
     kernel_reach and clean statistics); a non-finite map value elsewhere than under kernel_reach, poisoned statistics or
     the `huge` / `tiny` scenes fails;
  5. raw sums (methods 0, 2, 4) with thresholds on either side of a true peak score, 12 x 20 cell, up40 and down20;
  6. hitNeighbourhoods on the scaled scenes against the float64 context's score maps.

Assertions about which route ran are skipped under the route switches of the environment; assertions about results never.
"""
import time
import warnings

import numpy as np
import pytest

import f32_model as F
import mtm_oracle as O
from test_gpu_f32_geometry import _Poison
from test_gpu_tilings import default_routes

pytestmark = pytest.mark.gpu

THRESHOLD = {5: 0.9, 3: 0.9, 1: 0.1}
SCENES = [("noise+", s) for s in ("up40", "down20", "down40", "huge", "tiny", "nonfinite")] + \
         [("signed", "up40"), ("signed", "down20")]
CASES = [(c, kind, scene) for c in F.RANGE_CELLS for kind, scene in SCENES]
_IDS = ["%s-%s-%s" % (c["name"], kind, scene) for c, kind, scene in CASES]


def methods_of(kind):
    return (5, 3, 1) if kind == "noise+" else (5, 3)


def map_picks(cell):
    """The templates whose whole maps are compared: all of a small list; of the list of 17 the first and last of each group
    of 16 and the first noisy one."""
    n = cell["n"]
    return list(range(n)) if n <= 4 else sorted({0, 1, 15, 16, n - 1})


def always_one(scene, method):
    """cv2: templ_norm < DBL_EPSILON under TM_CCOEFF_NORMED - an ABSOLUTE rule: sum of the channel variances, 1600 * 4^k."""
    return method == 5 and scene in ("down40", "tiny")


_SCENES, _REFS = {}, {}


def scene_of(cell, kind, scene):
    key = (cell["name"], kind, scene)
    if key not in _SCENES:
        _SCENES[key] = F.range_scene(cell, scene, kind)
    return _SCENES[key]


def refs_of(cell, kind, scene, method):
    """Per picked template (direct-sum map, {pieces: model map}, {pieces: (accum_map, bound_map, live)}, valid): computed
    once, shared, never written to.  `valid`: where the model restates the kernel - everywhere on a scaled scene whose
    accumulators cannot overflow, nowhere on one where they can; on `nonfinite` (model and sums of the image WITHOUT the
    bad pixels) outside kernel_reach and where window and engine statistics are clean."""
    key = (cell["name"], kind, scene, method)
    if key in _REFS:
        return _REFS[key]
    S = scene_of(cell, kind, scene)
    img, clean, h, w = S["img"], S["clean"], cell["h"], cell["w"]
    picks = map_picks(cell)
    tl = [S["templs"][i] for i in picks]
    with np.errstate(over="ignore", invalid="ignore"):
        model = {pc: dict(zip(picks, F.model_scores_many(clean, tl, method, pc))) for pc in (3, 1)}
    ok = np.ones(cell["out"], bool)
    if scene == "nonfinite":
        ok = ~(F.kernel_reach(img, h, w) | F.window_dirty(img, h, w) | F.engine_stats_dirty(img, h, w))
    out = {}
    for i in picks:
        t = S["templs"][i]
        with np.errstate(over="ignore", invalid="ignore"):
            exact = O.match_template(clean, t, method, corr="direct").astype(np.float64)
            tol = {pc: F.tolerances(clean, t, method, pc) for pc in (3, 1)}
        valid = ok & F.accumulators_surely_finite(clean, t)
        out[i] = (exact, {pc: model[pc][i].astype(np.float64) for pc in (3, 1)}, tol, valid)
    _REFS[key] = out
    return out


def compared(exact_copy, a, b, live, valid):
    """The outputs a comparison covers (|score| < 1 in both maps, window not flat, the model applies) and whether they are
    at least 99 % of the map, an exact copy's own position not counted."""
    with np.errstate(invalid="ignore"):
        unsat = live & valid & (np.abs(a) < 1.0) & (np.abs(b) < 1.0)
    return unsat, int(unsat.sum()) >= 0.99 * (unsat.size - (1 if exact_copy else 0))


# ---- the GPU side --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import build as mtm_build
    mtm_build.build()
    from MTM import _lib
    assert _lib.load().mtm_device_count() >= 1
    return _lib


_ROUTES = {}            # (cell, kind, scene) -> set of f32_route values the default route took
_WORST = {}             # (kind, scene) -> {(pieces, "accum" | "bound"): worst error / tolerance}
_RAN = {}


def _compare_map(name, what, scene, method, pieces, i, got, ref, on_cores):
    exact, model, tol, valid = ref
    got = got.astype(np.float64)
    if always_one(scene, method):
        # nothing else is claimed for it: the template is constant by cv2's rule, whatever the image
        assert np.array_equal(got, np.ones_like(got)), (name, what, "constant by the DBL_EPSILON rule: 1 everywhere")
        return
    # a non-finite value is allowed under kernel_reach / poisoned statistics (valid is False there) or on huge / tiny
    bad = ~np.isfinite(got) & valid & (scene not in ("huge", "tiny"))
    assert not bad.any(), (name, what, "non-finite where nothing non-finite reaches", np.argwhere(bad)[:4].tolist())
    if not on_cores:
        # the float64 kernel (a route switch of the environment): the direct sums at 1e-6 relative
        with np.errstate(invalid="ignore"):
            far = valid & ~(np.abs(got - exact) <= 1e-6 * np.maximum(1.0, np.abs(exact)))
        assert not far.any(), (name, what, int(far.sum()), np.argwhere(far)[:4].tolist())
        return
    A, M, live = tol[pieces]
    for versus, other, T in (("accum", model[pieces], A), ("bound", exact, M)):
        unsat, enough = compared(i % 3 != 1, got, other, live, valid)
        if scene in F.IN_RANGE:
            assert enough, (name, what, versus, "compared %d of %d outputs" % (int(unsat.sum()), unsat.size))
        elif scene in ("tiny", "nonfinite"):
            assert unsat.sum() >= 0.05 * unsat.size, (name, what, versus, int(unsat.sum()))
        d = np.abs(got - other)
        ratio = float((d[unsat] / T[unsat]).max()) if unsat.any() else 0.0
        mine = _WORST.setdefault((name.split("/")[1], scene), {})
        mine[(pieces, versus)] = max(ratio, mine.get((pieces, versus), 0.0))
        far = unsat & ~(d <= T)
        assert not far.any(), "%s %s: %d outputs beyond %s_map (worst %.3f of it), first at %s: %r / %r" % (
            name, what, int(far.sum()), versus, ratio, np.argwhere(far)[0].tolist(), got[tuple(np.argwhere(far)[0])],
            other[tuple(np.argwhere(far)[0])])


def _kernel_maps(lib, cell, name, scene, ctxs, poison, method, S, refs):
    """Checks 3 and 4: the maps of three and of one piece product, through a map-mode search and the single-template launch."""
    img, shape = S["img"], cell["out"]
    units = [(t, None) for t in S["templs"]]
    nothing = -1.0 if method == 1 else 2.0          # a threshold no score passes: the maps are what is checked
    for pieces in (3, 1):
        ctx = ctxs[pieces]
        poison(ctx)
        ctx.search(units, img, method, lib.PEAKS_LOCAL, nothing)
        tm = ctx.timing()
        if default_routes():
            assert (tm["kernel_used"], tm["f32_pieces"]) == (5, pieces), (name, tm)
        for i in sorted(refs):
            _compare_map(name, "m%d np%d search map %d" % (method, pieces, i), scene, method, pieces, i,
                         ctx.last_score_map(i, shape), refs[i], tm["kernel_used"] == 5)
        i = max(refs)
        ctx.set_image(img)
        ctx.set_templates(units, method)
        poison(ctx)
        got = ctx.score_map(i, shape)
        _compare_map(name, "m%d np%d score_map(%d)" % (method, pieces, i), scene, method, pieces, i, got, refs[i],
                     ctx.timing()["kernel_used"] == 5)


def _copies_found(name, cell, method, S, ref):
    """Check 2, on the reference alone: the float64 kernel's records hold every planted copy at window_scores' score."""
    want = F.window_scores(S["img"], S["templs"][0], method, list(S["copies"].values()))
    for (label, (y, x)), s in zip(S["copies"].items(), want):
        rec = ref[(ref["templ_idx"] == 0) & (ref["y"] == y) & (ref["x"] == x)]
        assert len(rec) == 1, (name, method, "copy", label, (y, x), "is not among the float64 kernel's %d records" % len(ref))
        assert abs(float(rec["score"][0]) - float(s)) <= 1e-6, (name, method, label, float(rec["score"][0]), float(s))


def _to_map_scan(lib, ctx, S):
    """A list of 64 records and a threshold every output passes: the kernel candidates overflow, the ladder runs down and
    the context's next 16 local-extrema calls start on the map scan."""
    ctx.set_option(lib.OPT_HITS_ONLY, 0)
    ctx.set_option(lib.OPT_HIT_CAPACITY, 64)
    ctx.search([(t, None) for t in S["templs"]], S["clean"], 3, lib.PEAKS_LOCAL, -0.5)
    ctx.set_option(lib.OPT_HIT_CAPACITY, 1 << 18)


def _records(lib, cell, name, key, scene, fast, scan, exact, poison, method, S):
    """Checks 1 and 2: the default route's records are the float64 kernel's."""
    img = S["img"]
    units = [(t, None) for t in S["templs"]]
    thr = THRESHOLD[method]
    both_halves = cell["chans"] in (1, 3)
    exact.set_option(lib.OPT_HITS_ONLY, 0)
    ref = exact.search(units, img, method, lib.PEAKS_LOCAL, thr).copy()
    assert exact.timing()["kernel_used"] == 0 or not default_routes()
    if scene == "nonfinite":
        _copies_found(name, cell, method, S, ref)
    elif not always_one(scene, method):
        assert len(ref) >= len(units), (name, method, "every template is cut from the image", len(ref))
    for honly in ((1, 0) if both_halves else (0,)):
        fast.set_option(lib.OPT_HITS_ONLY, honly)
        poison(fast)
        got = fast.search(units, img, method, lib.PEAKS_LOCAL, thr).copy()
        tm = fast.timing()
        assert got.tobytes() == ref.tobytes(), (name, "local", method, "hits-only" if honly else "maps", "route %d pieces %d" % (
            tm["f32_route"], tm["f32_pieces"]), len(got), len(ref),
            sorted(set(map(tuple, got[["templ_idx", "y", "x"]].tolist())) ^ set(map(tuple, ref[["templ_idx", "y", "x"]].tolist())))[:6])
        if default_routes():
            assert tm["f32_route"] in (1, 2, 3), (name, tm)
            _ROUTES.setdefault(key, set()).add(tm["f32_route"])
    # ... and by the map scan (route 2), which a context takes for the 16 calls after a candidate list overflowed
    poison(scan)
    got = scan.search(units, img, method, lib.PEAKS_LOCAL, thr).copy()
    tm = scan.timing()
    assert got.tobytes() == ref.tobytes(), (name, "local", method, "map scan", "route %d" % tm["f32_route"], len(got), len(ref))
    if default_routes():
        assert tm["f32_route"] in (2, 3), (name, tm)
        _ROUTES.setdefault(key, set()).add(tm["f32_route"])
    exact.set_option(lib.OPT_HITS_ONLY, 1)
    gref = exact.search(units, img, method, lib.PEAKS_GLOBAL, 0.0).copy()
    fast.set_option(lib.OPT_HITS_ONLY, 1)
    poison(fast)
    got = fast.search(units, img, method, lib.PEAKS_GLOBAL, 0.0).copy()
    tm = fast.timing()
    assert got.tobytes() == gref.tobytes(), (name, "global", method, "route %d" % tm["f32_route"], got.tolist()[:3], gref.tolist()[:3])
    if default_routes():
        _ROUTES.setdefault(key, set()).add(tm["f32_route"])


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_f32_range_case(lib, case):
    cell, kind, scene = case
    t_start = time.perf_counter()
    name = "%s/%s/%s" % (cell["name"], kind, scene)
    key = (cell["name"], kind, scene)
    S = scene_of(cell, kind, scene)
    for label, why in S["skipped"].items():
        print("%s: pixel (%s) left out: %s" % (name, label, why))
    ctxs = {3: lib.Context(0), 1: lib.Context(0)}
    fast, scan, exact = lib.Context(0), lib.Context(0), lib.Context(0)
    poison = _Poison()
    try:
        ctxs[3].set_option(lib.OPT_F32_MFMA, 2)         # the bf16 scores as they are, three piece products
        ctxs[1].set_option(lib.OPT_F32_MFMA, 4)         # ... one
        exact.set_option(lib.OPT_F32_MFMA, 0)
        for c in (fast, scan):
            c.set_option(lib.OPT_F32_MFMA, 1)           # the contract under test, whatever the environment's switch says
        for c in ctxs.values():
            c.set_option(lib.OPT_HITS_ONLY, 0)
        _to_map_scan(lib, scan, S)
        for method in methods_of(kind):
            _records(lib, cell, name, key, scene, fast, scan, exact, poison, method, S)
            _kernel_maps(lib, cell, name, scene, ctxs, poison, method, S, refs_of(cell, kind, scene, method))
    finally:
        for c in list(ctxs.values()) + [fast, scan, exact]:
            c.close()
    _RAN[name] = time.perf_counter() - t_start
    print("%s: %.2f s; routes %s; worst error / tolerance so far on %s %s: %s" % (
        name, _RAN[name], sorted(_ROUTES.get(key, ())), kind, scene, ", ".join(
            "np%d %s %.3f" % (pc, what, r) for (pc, what), r in sorted(_WORST.get((kind, scene), {}).items()))))


@pytest.mark.parametrize("scene", ["up40", "down20"])
def test_f32_range_raw_sums_with_thresholds(lib, scene):
    """Check 5: TM_SQDIFF, TM_CCORR, TM_CCOEFF with a threshold on either side of one true peak score of the float64 run."""
    cell = F.RANGE_CELLS[0]
    S = scene_of(cell, "noise+", scene)
    units = [(t, None) for t in S["templs"]]
    fast, exact = lib.Context(0), lib.Context(0)
    poison = _Poison()
    try:
        exact.set_option(lib.OPT_F32_MFMA, 0)
        fast.set_option(lib.OPT_F32_MFMA, 1)
        for method in (0, 2, 4):
            everything = 3.0e38 if method == 0 else -3.0e38
            ref0 = exact.search(units, S["img"], method, lib.PEAKS_LOCAL, everything)
            sc = np.sort(np.unique(ref0["score"].astype(np.float64)))
            assert len(sc) >= 3, (scene, method, len(sc))
            s = float(sc[len(sc) // 2])
            d = abs(s) * 2e-6
            assert d > 0.0
            for thr in (s - d, s + d):
                ref = exact.search(units, S["img"], method, lib.PEAKS_LOCAL, thr).copy()
                poison(fast)
                got = fast.search(units, S["img"], method, lib.PEAKS_LOCAL, thr).copy()
                tm = fast.timing()
                assert len(ref) > 0 and got.tobytes() == ref.tobytes(), (scene, method, thr, tm["f32_route"], len(got), len(ref))
                if default_routes():
                    assert tm["f32_route"] in (1, 3), tm
    finally:
        fast.close()
        exact.close()


def _cut(smap, x, y):
    out = np.full((3, 3), np.nan, dtype=np.float32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if 0 <= y + dy < smap.shape[0] and 0 <= x + dx < smap.shape[1]:
                out[1 + dy, 1 + dx] = smap[y + dy, x + dx]
    return out


@pytest.mark.parametrize("scene", sorted(F.SCALES))
@pytest.mark.parametrize("cell", [F.RANGE_CELLS[0], F.RANGE_CELLS[5]], ids=lambda c: c["name"])
def test_f32_range_neighbourhoods(lib, cell, scene):
    """Check 6: hitNeighbourhoods with hits at the maps' four corners and at the templates' own positions, against cuts of
    the float64 context's score maps - test_float_neighbourhoods_agree_with_the_oracle's tolerance, NaN meets NaN."""
    import MTM
    S = scene_of(cell, "noise+", scene)
    h, w, (oh, ow) = cell["h"], cell["w"], cell["out"]
    lt = [("t%d" % k, t) for k, t in enumerate(S["templs"])]
    exact = lib.Context(0)
    try:
        exact.set_option(lib.OPT_F32_MFMA, 0)
        for method in (5, 3, 1):
            exact.set_image(S["img"])
            exact.set_templates([(t, None) for t in S["templs"]], method)
            maps = [exact.score_map(k, (oh, ow)) for k in range(len(lt))]
            hits, exp = [], []
            for k in range(len(lt)):
                own = np.unravel_index(int(np.argmin(maps[k]) if method == 1 else np.argmax(maps[k])), (oh, ow))
                for x, y in [(0, 0), (ow - 1, 0), (0, oh - 1), (ow - 1, oh - 1), (int(own[1]), int(own[0]))]:
                    hits.append(("t%d" % k, (x, y, w, h), np.float32(0.0)))
                    exp.append(_cut(maps[k], x, y))
            exp = np.stack(exp)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                nb = MTM.hitNeighbourhoods(lt, S["img"], hits, method)
            assert np.array_equal(np.isnan(nb), np.isnan(exp)), (cell["name"], scene, method)
            ok = ~np.isnan(exp)
            with np.errstate(invalid="ignore", over="ignore"):
                err = np.abs(nb[ok].astype(np.float64) - exp[ok]) / np.maximum(1.0, np.abs(exp[ok].astype(np.float64)))
            assert err.max() <= 1e-6, (cell["name"], scene, method, float(err.max()))
    finally:
        exact.close()


def test_f32_range_routes_and_figures():
    """Over the file, the kernel-candidate route (1) and the map scan (2) both ran; the figures docs/HISTORY.md records."""
    if not _RAN:                # (the cases did not run in this session: nothing to report)
        return
    seen = set().union(*_ROUTES.values()) if _ROUTES else set()
    for (kind, scene), worst in sorted(_WORST.items()):
        print("f32 range: %s %s worst error / tolerance: %s" % (kind, scene, ", ".join(
            "np%d %s %.3f" % (pc, what, r) for (pc, what), r in sorted(worst.items()))))
    by_scene = {}
    for (cname, kind, scene), r in _ROUTES.items():
        by_scene.setdefault((kind, scene), set()).update(r)
    print("f32 range: routes by scene %s" % {k: sorted(v) for k, v in sorted(by_scene.items())})
    print("f32 range: %d cases in %.1f s, slowest %s %.2f s" % (len(_RAN), sum(_RAN.values()), max(_RAN, key=_RAN.get), max(_RAN.values())))
    if default_routes():
        assert {1, 2} <= seen, seen
