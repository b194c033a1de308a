"""
The masked float32 screen (csrc/mtm_maskf32.hip.h, launch_masked_bf16) output by output (-m gpu).

Context.debug_maskf32_screen (mtm_debug_maskf32_screen) runs the stages a search call runs - J and the window sums, the two
raw launches of ncc_bf16_kernel, the listing pass, the exact re-scoring - and hands back what each leaves behind.  Every cell
of tests/maskf32_model.py's table runs with one and three piece products, TM_CCORR_NORMED and TM_SQDIFF, against a threshold
and in global mode, from poisoned memory, on `noise+` and one other scene; a second context with MTM_OPT_F32_MFMA = 0 supplies
the float64 kernel's maps.  Checked at every output of every template:

  1. the tile constants equal f32_model.tile_mu's bit for bit;
  2. the raw sums against the model (the same pieces multiplied exactly): accum_eps sqrt(S centred_sum2) + 2^-23 |c|;
  3. the raw sums against the exact sums: E1 and E2 as the header defines them;
  4. the bounds are the header's formulas of the returned sums (1e-9 of the interval's larger end; infinities exactly);
  5. lb <= q <= ub for the exact quality and for the float64 kernel's float32 score, no tolerance;
  6. threshold mode: the listed set is {not (ub < thr)}, each member once, placeholders exactly on the complement;
  7. global mode: best[] is the largest rounded-down lb, at most the exact maximum, the listed set {not (ub^ < best)} holds
     every tie of the extremum;
  8. after re-scoring the listed outputs and the records are the float64 kernel's bit for bit, placeholders untouched;
  9. a list capacity below the count: counted past it, `cap` records written, the canary behind them intact - and, through
     a search call, the ladder one piece product -> three -> the float64 kernel.

tests/test_maskf32_model_cpu.py shows on the CPU that the screen is live on these cells (not everything listed) and that the
model's own bounds hold.  Scenes with pixels or squares that are not finite (`nonfinite`, `huge`): the engine's running window
sums carry a NaN further than the windows that hold the pixel, and f32_model's statistics further still; there an output
whose bound (or model) is NaN is required to be listed and the comparisons cover the rest.
"""
import numpy as np
import pytest

import f32_model as F
import maskf32_model as M
from test_gpu_tilings import default_routes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import build as mtm_build
    mtm_build.build()
    from MTM import _lib
    assert _lib.load().mtm_device_count() >= 1
    return _lib


class _Poison:
    def __init__(self):
        self.k = 0

    def __call__(self, ctx):
        self.k += 1
        ctx.debug_poison(0xFF if self.k % 2 else 0x7F, 7)


def _same_bits(a, b):
    """float32 arrays equal bit for bit, any NaN equal to any NaN."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def _where(bad):
    return int(bad.sum()), np.argwhere(bad)[:4].tolist()


def _listed_mask(tag, rec, n, shape, h, w):
    """The records as a boolean (n, oh, ow) mask; each output at most once, w and h the class's."""
    oh, ow = shape
    t, y, x = rec["templ_idx"].astype(np.int64), rec["y"].astype(np.int64), rec["x"].astype(np.int64)
    assert ((t >= 0) & (t < n) & (y >= 0) & (y < oh) & (x >= 0) & (x < ow)).all(), (tag, "a record outside the maps")
    assert (rec["w"] == w).all() and (rec["h"] == h).all(), (tag, "w, h of the records")
    flat = (t * oh + y) * ow + x
    assert len(np.unique(flat)) == len(flat), (tag, "an output listed twice")
    mask = np.zeros(n * oh * ow, bool)
    mask[flat] = True
    return mask.reshape(n, oh, ow)


def _check_sums_and_bounds(tag, cm, members, method, pieces, got, f64q, listed, dirty):
    """Assertions 2 .. 5 for every template.  f64q: the float64 kernel's float32 scores as qualities; listed: the mask the
    listing pass produced (for outputs whose bound does not exist); dirty: a scene with values that are not finite."""
    h, nkb = cm.h, cm.nkb
    acc = F.accum_eps(1, h, nkb, pieces)
    m1, m2 = cm.raw(pieces)
    worst = {"accum": 0.0, "exact": 0.0}
    for j, k in enumerate(members):             # j: the template's index in its class, k: in the cell
        c1, c2 = got["c1"][j].astype(np.float64), got["c2"][j].astype(np.float64)
        e1x, e2x, _ = cm.exact[k]
        cs2_u, cs2_v = cm.cs2[k]
        with np.errstate(invalid="ignore", over="ignore"):
            # 2. against the model
            for name, c, model, S, cs2 in (("c1", c1, m1[k], cm.px.s_i, cs2_u), ("c2", c2, m2[k], cm.px.s_j, cs2_v)):
                tol = acc * np.sqrt(S * cs2) + 2.0 ** -23 * np.abs(c)
                ok = np.isfinite(model) & np.isfinite(tol)
                assert dirty or ok.all(), (tag, k, name, "model not finite")
                d = np.abs(c - model)
                bad = ok & ~(d <= tol)
                if (ok & (tol > 0)).any():
                    worst["accum"] = max(worst["accum"], float((d[ok & (tol > 0)] / tol[ok & (tol > 0)]).max()))
                assert not bad.any(), (tag, k, name, "raw sum beyond the accumulation tolerance of the model") + _where(bad) + (
                    float(c[tuple(np.argwhere(bad)[0])]), float(model[tuple(np.argwhere(bad)[0])]), float(tol[tuple(np.argwhere(bad)[0])]))
            # 3. against the exact sums
            E1, E2 = M.error_terms(cm.px, cs2_u, cs2_v, cm.eps(pieces), c1, c2)
            for name, c, ex, E in (("c1", c1, e1x, E1), ("c2", c2, e2x, E2)):
                ok = np.isfinite(ex) & np.isfinite(E) & np.isfinite(c)
                assert dirty or ok.all(), (tag, k, name, "sums not finite")
                d = np.abs(c - ex)
                bad = ok & ~(d <= E)
                if ok.any():
                    worst["exact"] = max(worst["exact"], float((d[ok] / E[ok]).max()))
                assert not bad.any(), (tag, k, name, "raw sum beyond E of the exact sum") + _where(bad)
            # 4. the bounds are the header's formulas of these sums
            lbm, ubm = cm.bounds_from(method, pieces, k, c1, c2)
            for name, dev, mod in (("lb", got["lb"][j], lbm), ("ub", got["ub"][j], ubm)):
                nan = np.isnan(dev) | np.isnan(mod)
                assert dirty or not nan.any(), (tag, k, name, "NaN bound on finite data") + _where(nan)
                assert listed[j][nan].all(), (tag, k, name, "a bound that does not exist, not listed")
                inf = ~nan & (np.isinf(dev) | np.isinf(mod))
                assert np.array_equal(dev[inf], mod[inf]), (tag, k, name, "infinities differ")
                fin = ~nan & ~inf
                scale = np.maximum(np.abs(lbm), np.abs(ubm))
                scale = np.where(np.isfinite(scale), scale, np.abs(mod))
                bad = fin & ~(np.abs(dev - mod) <= 1e-9 * scale)
                assert not bad.any(), (tag, k, name, "bound differs from the header's formula") + _where(bad)
            # 5. containment, no tolerance
            lb, ub = got["lb"][j], got["ub"][j]
            for name, q in (("exact", cm.q(method, k)), ("f64 kernel", f64q[j].astype(np.float64))):
                fin = np.isfinite(q)
                bad = fin & ~M.contains(lb, ub, q)
                assert not bad.any(), (tag, k, name, "quality outside [lb, ub]") + _where(bad) + (
                    float(lb[tuple(np.argwhere(bad)[0])]), float(q[tuple(np.argwhere(bad)[0])]), float(ub[tuple(np.argwhere(bad)[0])]))
                none = ~fin
                assert ((ub[none] == np.inf) | listed[j][none]).all(), (tag, k, name, "no quality, yet neither ub = +inf nor listed")
    return worst


def _check_listing(tag, cm, members, method, mode, thr, got, f64, f64q, lib):
    """Assertions 6 .. 8; returns the listed mask."""
    n, (oh, ow) = len(members), cm.cell["out"]
    below = np.float32(np.inf if method == M.SQDIFF else -np.inf)
    info = got["info"]
    assert info["count"] <= info["cap"] and info["rescored"] == 1 and len(got["records"]) == info["count"], (tag, info)
    listed = _listed_mask(tag, got["records"], n, (oh, ow), cm.h, cm.w)
    lb, ub = got["lb"], got["ub"]
    if mode == lib.PEAKS_LOCAL:
        want = np.stack([M.listed_threshold(method, ub[k], thr) for k in range(n)])
        # every output whose float64-kernel score passes the threshold is listed
        with np.errstate(invalid="ignore"):
            passes = f64q >= np.float32(M.thr_quality(method, thr))
        assert listed[passes].all(), (tag, "a score that passes the threshold is not listed") + _where(passes & ~listed)
    else:
        want = np.stack([M.listed_global(lb[k], ub[k]) for k in range(n)])
        for j, k in enumerate(members):
            best = M.key_to_float(got["best"][j])
            assert best == M.best_lower(lb[j]), (tag, k, "best[] key", best, M.best_lower(lb[j]))
            for name, q in (("exact", cm.q(method, k)), ("f64 kernel", f64q[j].astype(np.float64))):
                fin = np.isfinite(q)
                if fin.any():
                    top = q[fin].max()
                    assert float(best) <= top, (tag, k, name, "best lower bound above the maximum quality", float(best), float(top))
                    ties = fin & (q == top)
                    assert listed[j][ties].all(), (tag, k, name, "a tie of the extremum is not listed") + _where(ties & ~listed[j])
    for (t, y, x) in cm.plants:
        if t in members:
            assert listed[members.index(t), y, x], (tag, "planted copy not listed", t, y, x)
    assert np.array_equal(listed, want), (tag, "listed set differs from the rule on the returned bounds") + _where(listed != want)
    # the map as the listing pass left it: the placeholder exactly on the complement (listed slots: not the placeholder,
    # unless the bound itself is parked there in global mode, which is never the placeholder's sign of infinity by the rule)
    ml, mr = got["map_listed"], got["map_rescored"]
    assert (ml[~listed] == below).all(), (tag, "no placeholder on an output that is not listed") + _where(~listed & (ml != below))
    if mode == lib.PEAKS_LOCAL:
        # (threshold mode never writes a listed slot: it still holds the poison pattern, NaN or a huge number)
        assert not (ml[listed] == below).any(), (tag, "placeholder on a listed output")
    # 8. after re-scoring
    assert (mr[~listed] == below).all(), (tag, "re-scoring touched a placeholder")
    assert _same_bits(mr[listed], f64[listed]), (tag, "re-scored outputs differ from the float64 kernel") + _where(
        listed & ~((mr == f64) | (np.isnan(mr) & np.isnan(f64))))
    rec = got["records"]
    assert _same_bits(rec["score"], f64[rec["templ_idx"], rec["y"], rec["x"]]), (tag, "record scores differ from the float64 kernel")
    assert (got["canary"] == 0xC5).all(), (tag, "the canary behind the list")
    return listed


_RAN = {}


@pytest.mark.parametrize("cell", [c for c in M.CELLS if c["on_route"]], ids=[c["name"] for c in M.CELLS if c["on_route"]])
def test_maskf32_screen_cell(lib, cell):
    import time
    t_start = time.perf_counter()
    name, shape = cell["name"], cell["out"]
    fast, exact = lib.Context(0), lib.Context(0)
    poison = _Poison()
    worst = {"accum": 0.0, "exact": 0.0}
    no_cap = []             # classes none of whose listings held two outputs: no capacity check
    shares = {}             # (scene, pieces) -> the listed share of every class, method and mode (constant masks aside)
    try:
        fast.set_option(lib.OPT_F32_MFMA, 1)
        exact.set_option(lib.OPT_F32_MFMA, 0)
        for scene in cell["scenes"]:
            cm = M.CellModel(cell, scene)
            dirty = scene in ("nonfinite", "huge")
            for method in M.METHODS:
                for g, (kind, members) in enumerate(cm.groups):         # one size class, one screen, per mask
                    units = [cm.units[k] for k in members]
                    n = len(units)
                    for c_ in (fast, exact):
                        c_.set_image(cm.img)
                        c_.set_templates(units, method)
                    f64 = np.stack([exact.score_map(j, shape) for j in range(n)])
                    f64q = -f64 if method == M.SQDIFF else f64
                    thr = cm.threshold(method, g)
                    for pieces in (1, 3):
                        for mode in (lib.PEAKS_LOCAL, lib.PEAKS_GLOBAL):
                            tag = (name, scene, kind, "m%d" % method, "np%d" % pieces, "global" if mode else "thr %r" % thr)
                            poison(fast)
                            got = fast.debug_maskf32_screen(n, shape, pieces, mode, thr)
                            info = got["info"]
                            assert (info["n_templ"], info["h"], info["w"], info["oh"], info["ow"]) == (n, cm.h, cm.w) + tuple(shape), (tag, info)
                            assert info["mb"] == (2 if n > 16 else 1) and info["cap"] == info["cap_production"], (tag, info)
                            # 1. the tile constants
                            for which, mu in (("mu_i", cm.px.mu_i), ("mu_j", cm.px.mu_j)):
                                assert _same_bits(got[which], mu), (tag, which, "tile constants differ from f32_model.tile_mu") + _where(
                                    ~((got[which] == mu) | (np.isnan(got[which]) & np.isnan(mu))))
                            listed = _check_listing(tag, cm, members, method, mode, thr, got, f64, f64q, lib)
                            w_ = _check_sums_and_bounds(tag, cm, members, method, pieces, got, f64q, listed, dirty)
                            worst = {k_: max(worst[k_], w_[k_]) for k_ in worst}
                            if kind not in ("zero", "one_tap"):
                                shares.setdefault((scene, pieces), []).append(float(listed.mean()))
                    # 9. a capacity below the count: the first of these listings that holds two outputs or more (a class whose
                    # exact cut is its only output above the threshold lists one with three products)
                    done = False
                    for pieces, mode in ((3, lib.PEAKS_LOCAL), (1, lib.PEAKS_LOCAL), (3, lib.PEAKS_GLOBAL), (1, lib.PEAKS_GLOBAL)):
                        poison(fast)
                        full = fast.debug_maskf32_screen(n, shape, pieces, mode, thr)
                        count = full["info"]["count"]
                        if count < 2:
                            continue
                        cap = count // 2
                        poison(fast)
                        got = fast.debug_maskf32_screen(n, shape, pieces, mode, thr, list_cap=cap)
                        info = got["info"]
                        what = (name, scene, kind, method, pieces, mode)
                        assert info["cap"] == cap and info["count"] == count > cap and info["rescored"] == 0, (what, info)
                        assert len(got["records"]) == cap and (got["canary"] == 0xC5).all(), (what, "records past the capacity")
                        part = _listed_mask(what + ("cap",), got["records"], n, shape, cm.h, cm.w)
                        assert not (part & ~_listed_mask(what, full["records"], n, shape, cm.h, cm.w)).any(), what
                        done = True
                        break
                    if not done:
                        no_cap.append("%s m%d %s" % (scene, method, kind))
                    # (the class of the planted copies lists them and the cut they were taken from: never skipped)
                    assert done or not any(t in members for t, _, _ in cm.plants), (name, scene, kind, method, "capacity check skipped")
    finally:
        fast.close()
        exact.close()
    _RAN[name] = time.perf_counter() - t_start
    print("%s: %.2f s; worst |raw - model| / tolerance %.3f, |raw - exact| / E %.3f; listed share (min .. max over classes): %s" % (
        name, _RAN[name], worst["accum"], worst["exact"],
        "; ".join("%s np%d %.3f .. %.3f" % (sc, pc, min(v), max(v)) for (sc, pc), v in sorted(shares.items()))))
    if no_cap:
        print("%s: no capacity check (fewer than two outputs listed in every listing): %s" % (name, "; ".join(no_cap)))


def test_off_route_class_is_refused_and_runs_the_float64_kernel(lib):
    """w = 257 > kBfMaxW: the entry refuses the class with a clean error, a search takes route 0 and equals the exact context.
    Also refused: templates of several classes (different masks), a class without masks, a context whose float32 option
    leaves the screen off."""
    cell = next(c for c in M.CELLS if not c["on_route"])
    cm = M.CellModel(cell, "noise+")
    shape = cell["out"]
    fast, exact = lib.Context(0), lib.Context(0)
    try:
        fast.set_option(lib.OPT_F32_MFMA, 1)
        exact.set_option(lib.OPT_F32_MFMA, 0)
        for method in M.METHODS:
            for g, (kind, members) in enumerate(cm.groups):
                units = [cm.units[k] for k in members]
                thr = cm.threshold(method, g)
                fast.debug_poison(0xFF, 7)
                a = fast.search(units, cm.img, method, lib.PEAKS_LOCAL, thr).copy()
                assert fast.timing()["f32_route"] == 0, (method, kind)
                b = exact.search(units, cm.img, method, lib.PEAKS_LOCAL, thr).copy()
                assert a.tobytes() == b.tobytes() and (len(a) >= 1 or kind in ("zero", "one_tap")), (method, kind, len(a), len(b))
                with pytest.raises(lib.MtmError, match="mtm_debug_maskf32_screen"):
                    fast.debug_maskf32_screen(len(units), shape, 3, lib.PEAKS_LOCAL, thr)
        small = next(c for c in M.CELLS if c["name"] == "taps-5x32")
        cs = M.CellModel(small, "noise+")
        one = [cs.units[k] for k in cs.groups[0][1]]
        for ctx, units in ((exact, one), (fast, cs.units), (fast, [(t, None) for t, _ in one])):
            ctx.set_image(cs.img)
            ctx.set_templates(units, M.CCORR_NORMED)
            with pytest.raises(lib.MtmError, match="mtm_debug_maskf32_screen"):
                ctx.debug_maskf32_screen(len(units), small["out"], 3, lib.PEAKS_LOCAL, 0.5)
        # ... and the same class on the screen's own context is taken
        fast.set_templates(one, M.CCORR_NORMED)
        assert fast.debug_maskf32_screen(len(one), small["out"], 3, lib.PEAKS_LOCAL, 0.5)["info"]["n_templ"] == len(one)
    finally:
        fast.close()
        exact.close()


def test_the_ladder_through_a_search_call(lib):
    """One piece product -> three -> the float64 kernel, through the production call: on maskf32_model.LADDER the one-product
    bound lists every output and the three-product bound less than a third of them (tests/test_maskf32_model_cpu.py prints
    the two counts), so a list capacity between the two makes the first screen overflow and the second fit; a capacity below
    both sends the class to the float64 kernel.  The records are the float64 kernel's every time."""
    name, scene, g = M.LADDER
    cell = next(c for c in M.CELLS if c["name"] == name)
    cm = M.CellModel(cell, scene)
    counts = M.ladder_counts(cm, g)
    assert counts[1] >= 3 * counts[3] and counts[3] >= 4, counts
    thr = cm.threshold(M.CCORR_NORMED, g)
    units = [cm.units[k] for k in cm.groups[g][1]]
    exact = lib.Context(0)
    exact.set_option(lib.OPT_F32_MFMA, 0)
    try:
        ref = exact.search(units, cm.img, M.CCORR_NORMED, lib.PEAKS_LOCAL, thr).copy()
        assert len(ref) >= 1
        # (a fresh context per rung: an overflow makes the next calls of a context start with three products)
        for cap, pieces, route in ((0, 1, 4), ((counts[1] + counts[3]) // 2, 3, 4), (counts[3] // 2, None, 0)):
            fast = lib.Context(0)
            try:
                fast.set_option(lib.OPT_F32_MFMA, 1)
                fast.debug_poison(0x7F, 7)
                fast.set_image(cm.img)
                fast.set_templates(units, M.CCORR_NORMED)
                fast.debug_maskf32_list_cap(cap)
                got = fast.search(units, cm.img, M.CCORR_NORMED, lib.PEAKS_LOCAL, thr).copy()
                tm = fast.timing()
                assert got.tobytes() == ref.tobytes(), (cap, len(got), len(ref))
                if default_routes():
                    assert tm["f32_route"] == route and pieces in (None, tm["f32_pieces"]), (cap, counts, tm["f32_pieces"], tm["f32_route"])
            finally:
                fast.close()
    finally:
        exact.close()
