"""
The tail screen's constants and bound, from the device's own data, against exact sums (-m gpu).

The two-row int8 score kernel leaves its K loop where acc_P + K_P + m S1 + (tau_Q - 128) S1_Q + sqrt(V_Q) g_Q rules out every
hit of a wave.  The tail-box records (tests/test_gpu_window_stats.py) and the accumulators (tests/test_gpu_tilings.py) are
held to exact sums elsewhere; this file takes the third input - TemplDev::tail_k / tail_d / tail_g, summed by
tail_consts_kernel out of the packed A operand and valid for ONE split - and the bound built from all three.

  cells        classes that really screen (asserted through Context.class_tilings() on the default routes), at the row-loop
               and segment edges of tail_consts_kernel, list positions >= 16, partly filled groups, every template kind that
               strains a term (tests/tail_model.py: CONST_CELLS, KINDS); one cell's templates are views built on the device.
  constants    Context.debug_tail_consts(split) for splits 6, 7, h - 2 and the rule's values, every template, both parities:
               the inequalities of tail_model.check_consts against exact integers and Fractions - and, since division and
               square root are correctly rounded on the device, the float64 restatement bit for bit (d, g, and k restated
               from the device's own g).
  the split    one context called at 0.5, 0.9, 0.7, 0.5, 0.7: after each call the device holds the constants of the split that
               call carried and says so; a re-derivation for a foreign split through the entry is followed by a search that
               returns a fresh context's records and leaves its own split's constants behind.
  the bound    constants from debug_tail_consts, block records from debug_window_stats(tail_s=split), accumulators and
               numerators as exact integers: Fraction(bound) >= numerator at every output of every block.  The smallest
               (bound - numerator) / (templ_norm sq) per cell is printed: how small a mistake the check can see.
"""
import ctypes
import time

import numpy as np
import pytest

import tail_model as M
from test_gpu_tilings import default_routes

pytestmark = pytest.mark.gpu

_SECONDS = {}            # cell -> seconds
_TIGHT = {}              # cell -> {split: tightness}
_BIT_EQUAL = {"d": True, "g": True, "k": True}
_SCENES = {}             # cell name -> (img, templates, kinds): made once, shared, read-only


@pytest.fixture(scope="module")
def lib():
    import build as mtm_build
    mtm_build.build()
    from MTM import _lib
    assert _lib.load().mtm_device_count() >= 1
    return _lib


@pytest.fixture(scope="module", autouse=True)
def _sweep_record():
    """What the cells of this session measured, in one place (profiles/tail_model/sweep.txt keeps a run's copy)."""
    yield
    if not _SECONDS:
        return
    print("\ntail_consts: %d cells, %.1f s; slowest %s" % (len(_SECONDS), sum(_SECONDS.values()),
                                                           max(_SECONDS.items(), key=lambda kv: kv[1])))
    print("tail_consts: bit-equal to the float64 restatement: d %s, g %s, k (from the device's g) %s" % (
        _BIT_EQUAL["d"], _BIT_EQUAL["g"], _BIT_EQUAL["k"]))
    for name, tight in sorted(_TIGHT.items()):
        if tight:
            print("tail_consts: %-22s smallest (bound - num) / (templ_norm sq) = %.3e" % (name, min(tight.values())))


def _ctx(monkeypatch, lib, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = lib.Context(0)
    for k in env:
        monkeypatch.delenv(k)
    c.set_option(lib.OPT_HITS_ONLY, 1)
    return c


def _scene(cell):
    if cell["name"] not in _SCENES:
        img, templates, kinds = M.scene(cell)
        for a in [img] + templates:
            a.setflags(write=False)
        _SCENES[cell["name"]] = (img, templates, kinds)
    return _SCENES[cell["name"]]


def _search(lib, ctx, cell, img, templates, thr):
    if cell.get("device"):
        bases, recs, _ = M.device_units(cell)
        ctx.set_templates_augmented(bases, recs, cell["method"])
        return ctx.find_matches_image(img, lib.PEAKS_LOCAL, thr).copy()
    return ctx.search([(t, None) for t in templates], img, cell["method"], lib.PEAKS_LOCAL, thr).copy()


def _screening_class(ctx, cell):
    rec, = ctx.class_tilings()
    assert (rec["h"], rec["w"], rec["n_templates"]) == (cell["h"], cell["w"], cell["n"]), rec
    if default_routes():
        assert rec["tail_ok"] and rec["r2"] == 2 and rec["kernel"] == 3 and not rec["kp_nseg"] and not rec["rm_nt"], rec
    return rec


def _check_table(got, templates, split, where):
    """got: debug_tail_consts' array for `split`.  The inequalities, then the restatement bit for bit."""
    assert got.shape == (len(templates), 7) and np.isfinite(got).all(), where
    assert (got[:, 6] == split).all(), (where, got[:, 6])
    bad = M.consts_violations(got, templates, split)
    assert not bad, (where, len(bad), bad[:4])
    for li, T in enumerate(templates):
        for r, q0 in enumerate((split, split - 1)):
            k, d, g = M.consts_f64(T, q0)
            k_dev_g = M.consts_f64(T, q0, g=got[li, 4 + r])[0]
            _BIT_EQUAL["d"] &= bool(got[li, 2 + r] == d)
            _BIT_EQUAL["g"] &= bool(got[li, 4 + r] == g)
            _BIT_EQUAL["k"] &= bool(got[li, r] == k_dev_g)
            # one IEEE division and subtraction; one division, square root and product; sums and products of those
            assert got[li, 2 + r] == d, (where, li, r, got[li, 2 + r], d)
            assert got[li, 4 + r] == g, (where, li, r, got[li, 4 + r], g)
            assert got[li, r] == k_dev_g == k, (where, li, r, got[li, r], k_dev_g, k)


@pytest.mark.parametrize("cell", M.CONST_CELLS, ids=[c["name"] for c in M.CONST_CELLS])
def test_cell(lib, monkeypatch, cell):
    """Constants at every split of the cell, then the bound from the device's constants and block records."""
    t0 = time.perf_counter()
    img, templates, kinds = _scene(cell)
    h, w, method = cell["h"], cell["w"], cell["method"]
    assert set(kinds) >= set(M.KINDS) and len(templates) == cell["n"]
    ctx = _ctx(monkeypatch, lib)
    try:
        ctx.debug_poison(0xFF, 7)
        _search(lib, ctx, cell, img, templates, 0.5)
        rec = _screening_class(ctx, cell)
        # what the search left behind: the constants of the split it carried (0.5: the split placement computed them for)
        held = ctx.debug_tail_consts(0)
        if not rec["tail_ok"]:                              # (a route switch took the class off the two-row tiling)
            assert not default_routes() and np.isnan(held[:, :6]).all() and (held[:, 6] == -1).all()
            return
        if default_routes():
            assert rec["tail_split"] == M.rule_split(lib, h, w, 0.5), rec
        if rec["tail_split"] > 0:
            _check_table(held, templates, rec["tail_split"], (cell["name"], "after the search"))
        tstats = M.templ_stats(lib, templates, method)
        nums = None
        tight = {}
        for split in M.cell_splits(lib, cell):
            ctx.debug_poison(0x7F if split & 1 else 0xFF, 7)
            got = ctx.debug_tail_consts(split)
            _check_table(got, templates, split, (cell["name"], split))
            again = ctx.debug_tail_consts(0)                  # launches nothing: the same bytes
            assert again.tobytes() == got.tobytes(), (cell["name"], split)
            # the bound: device constants, device block records, exact accumulators and numerators
            st = ctx.debug_window_stats(img, h, w, 1 if method == 5 else 0, planes=("t0", "sq", "blk"), tail_s=split)
            if nums is None:
                nums = M.numerators(img, templates, method, st)
            r = M.rigour(img, templates, method, 0.5, got, tstats, st, split, nums=nums)
            assert not r["violations"], (cell["name"], split, len(r["violations"]), r["violations"][:3])
            assert r["checked"] == cell["n"] * 13 * 19 and r["tightness"] >= 0.0
            tight[split] = r["tightness"]
        _TIGHT[cell["name"]] = tight
    finally:
        ctx.close()
        _SECONDS[cell["name"]] = time.perf_counter() - t0
        print("tail_consts %-22s %5.2f s  splits %s  min (bound - num) / (templ_norm sq): %s" % (
            cell["name"], _SECONDS[cell["name"]], M.cell_splits(lib, cell),
            " ".join("%d:%.2e" % kv for kv in sorted(_TIGHT.get(cell["name"], {}).items()))))


def test_constants_follow_the_split(lib, monkeypatch):
    cell = M.COUNTER_SCENES[0]                       # 64 x 64 x 32 on a 16 x 512 map
    img, templates, _ = _scene(cell)
    h, w, method = cell["h"], cell["w"], cell["method"]
    tl = [(t, None) for t in templates]
    thrs = (0.5, 0.9, 0.7, 0.5, 0.7)
    want = {t: M.rule_split(lib, h, w, t) for t in thrs}
    assert len(set(want.values())) == 3 and min(want.values()) >= 6, want
    fresh = _ctx(monkeypatch, lib)
    ctx = _ctx(monkeypatch, lib)
    try:
        fresh.debug_poison(0x7F, 7)
        ref = {}
        for t in sorted(set(thrs)):
            ref[t] = fresh.search(tl, img, method, lib.PEAKS_LOCAL, t).copy()
        assert len(ref[0.5]) >= 2 and {0, cell["n"] - 1} <= set(ref[0.9]["templ_idx"].tolist())      # the two exact copies
        ctx.debug_poison(0xFF, 7)
        for t in thrs:
            got = ctx.search(tl, img, method, lib.PEAKS_LOCAL, t).copy()
            assert got.tobytes() == ref[t].tobytes(), (t, len(got), len(ref[t]))
            if not default_routes():
                continue
            rec = _screening_class(ctx, cell)
            assert rec["tail_split"] == want[t], (t, rec)
            _check_table(ctx.debug_tail_consts(0), templates, want[t], ("after a search at", t))
        if default_routes():
            # a foreign split through the entry, then a search: it re-derives its own, and its records are a fresh context's
            # (far from the call's split, next to it on either side, and the call's own)
            for foreign, t in ((h - 2, 0.5), (6, 0.7), (want[0.9], 0.5), (want[0.5] + 3, 0.5), (want[0.7] - 7, 0.7),
                               (want[0.9] + 1, 0.9), (want[0.5], 0.5)):
                ctx.debug_poison(0x7F, 7)
                _check_table(ctx.debug_tail_consts(foreign), templates, foreign, ("foreign", foreign))
                got = ctx.search(tl, img, method, lib.PEAKS_LOCAL, t).copy()
                assert got.tobytes() == ref[t].tobytes(), (foreign, t, len(got), len(ref[t]))
                assert _screening_class(ctx, cell)["tail_split"] == want[t]
                _check_table(ctx.debug_tail_consts(0), templates, want[t], ("after foreign", foreign, t))
    finally:
        ctx.close()
        fresh.close()


def test_entry_refuses_and_marks_classes_without_a_screen(lib, monkeypatch):
    ctx = _ctx(monkeypatch, lib)
    try:
        with pytest.raises(lib.MtmError, match="no template set is placed"):
            ctx.debug_tail_consts(0)
        rng = np.random.default_rng(5)
        img = rng.integers(0, 256, (60, 200)).astype(np.uint8)
        narrow = [(rng.integers(0, 256, (20, 24)).astype(np.uint8), None) for _ in range(18)]        # packed K: no screen
        wide = [(rng.integers(0, 256, (24, 56)).astype(np.uint8), None) for _ in range(19)]          # two-row: screens
        ctx.debug_poison(0xFF, 7)
        ctx.search(narrow[:9] + wide + narrow[9:], img, 5, lib.PEAKS_LOCAL, 0.7)
        recs = ctx.class_tilings()
        assert sorted((r["h"], r["w"], r["n_templates"]) for r in recs) == [(20, 24, 18), (24, 56, 19)], recs
        for split in (0, 9):
            out = ctx.debug_tail_consts(split)
            assert out.shape == (37, 7)
            where = np.array([False] * 9 + [True] * 19 + [False] * 9)
            assert np.isnan(out[~where, :6]).all() and (out[~where, 6] == -1).all(), out[~where]
            if default_routes():
                assert np.isfinite(out[where]).all()
                assert (out[where, 6] == (9 if split else M.rule_split(lib, 24, 56, 0.7))).all(), out[where, 6]
                assert not M.consts_violations(out[where], [t for t, _ in wide], int(out[where][0, 6]))
        # too small an output, a negative split: refused, nothing written
        small = np.full(7 * 37 - 1, -7.0)
        p = small.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        assert lib.load().mtm_debug_tail_consts(ctx._h, 0, p, small.size) == lib.E_OVERFLOW and (small == -7.0).all()
        assert lib.load().mtm_debug_tail_consts(ctx._h, -1, p, small.size) == -1 and (small == -7.0).all()
        # a find in flight owns the context
        ctx.set_image(img)
        ctx.set_templates(wide, 5)
        ctx.find_matches(lib.PEAKS_LOCAL, 0.7)
        ctx.find_matches_async(lib.PEAKS_LOCAL, 0.7)
        try:
            with pytest.raises(lib.MtmError, match="in flight"):
                ctx.debug_tail_consts(0)
        finally:
            ctx.find_matches_wait()
        assert ctx.debug_tail_consts(0).shape == (19, 7)
    finally:
        ctx.close()
