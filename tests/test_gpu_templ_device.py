"""
Templates built on the device - views, area resizes, integer downscales, the A-operand packs gathered from them - against exact
sums (-m gpu).

mtm_set_templates_augmented keeps the bases in a device arena, makes the resized sources there (resize_area_kernel,
downscale_int_kernel), sums them (source_sums_kernel: every constant of a resized unit), reads every unit through six view
coefficients (View::fliplr / flipud / rot90 -> unit_px, unit_mask) and gathers the packs of every tiling from those views
(pack_units_kernel; gather_unit_kernel for the kernels with host-packed weights).  A wrong index there is right for square
templates and for w % 16 == 0 and gives plausible scores for one residue.  Every cell of tests/templ_device_model.py

  1. asserts through Context.class_tilings() which kernel and tiling every class entered (default routes);
  2. compares the whole score map of EVERY unit, from poisoned memory, with
       (a) the oracle's direct sums on the model's expansion - unmasked: bit for bit, NaN with NaN; masked classes:
           1e-6 max(1, |exp|), the tolerance tests/test_gpu_tilings.py holds masked maps to;
       (b) the same library given the host-expanded list through set_templates on a context created under
           MTM_TEMPL_ON_DEVICE=0 - the host packers - bit for bit, masked or not;
  3. on the unmasked single-class cells, compares the hits-only records at one threshold with map mode's byte for byte.

Next to the table: a readout of the packed pixels themselves (TM_CCORR against one set pixel), invalid resizes, a context that
goes through several template sets, and the image-side downscale read out through 1 x 1 templates.
"""
import os
import time

import numpy as np
import pytest

import mtm_oracle as O
import templ_device_model as M
from test_gpu_tilings import default_routes

pytestmark = pytest.mark.gpu

_CONFIRMED = {}           # cell name -> [(family, views of the class)] its tiling assertion passed on
_WORST = {}               # cell name -> worst |got - exp| / tolerance over its masked maps
_SECONDS = {}


@pytest.fixture(scope="module")
def lib():
    import build as mtm_build
    mtm_build.build()
    from MTM import _lib
    assert _lib.load().mtm_device_count() >= 1
    return _lib


@pytest.fixture(scope="module")
def pair(lib):
    """(the context under test, a context with the host packers): created once, every cell replaces their template sets."""
    old = os.environ.get("MTM_TEMPL_ON_DEVICE")
    os.environ["MTM_TEMPL_ON_DEVICE"] = "0"
    try:
        host = lib.Context(0)
    finally:
        if old is None:
            del os.environ["MTM_TEMPL_ON_DEVICE"]
        else:
            os.environ["MTM_TEMPL_ON_DEVICE"] = old
    dev = lib.Context(0)
    for c in (dev, host):
        c.set_option(lib.OPT_HITS_ONLY, 0)
        c.set_option(lib.OPT_EXACT_DIV, 1)
    yield dev, host
    dev.close()
    host.close()


_KERNELS = {"auto": None, "naive": 1, "dot4": 2}


def _set_kernel(lib, ctxs, name):
    from conftest import fresh_options
    for c in ctxs:
        c.set_option(lib.OPT_KERNEL, fresh_options()[lib.OPT_KERNEL] if _KERNELS[name] is None else _KERNELS[name])


def _map_shape(img, t):
    return (img.shape[0] - t.shape[0] + 1, img.shape[1] - t.shape[1] + 1)


def _first_bad(same):
    bad = np.argwhere(~same)
    return (len(bad), tuple(int(v) for v in bad[0])) if len(bad) else (0, None)


def _compare_maps(lib, dev, host, cell, bases, recs, units, img, method, oracle=True):
    """Sets the bases on `dev` and the expansion on `host`, searches in map mode and compares every unit's map three ways."""
    masked = bases[0][1] is not None
    thr = {0: -1.0, 1: -1.0, 2: 1e30, 3: 2.0, 4: 1e30, 5: 2.0}[method]                 # nothing listed: the maps are what is checked
    dev.debug_poison(0xFF, 7)
    host.debug_poison(0x7F, 4)
    dev.set_templates_augmented(bases, list(recs), method)
    dev.find_matches_image(img, lib.PEAKS_LOCAL, thr)
    host.set_templates(units, method)
    host.find_matches_image(img, lib.PEAKS_LOCAL, thr)
    worst = 0.0
    for i, (t, mask) in enumerate(units):
        where = (cell["name"], "method %d" % method, "unit %d" % i, "base %d" % (i // len(recs)), "record %r" % (recs[i % len(recs)],))
        shape = _map_shape(img, t)
        got, packed = dev.last_score_map(i, shape), host.last_score_map(i, shape)
        n_host, at_host = _first_bad((got == packed) | (np.isnan(got) & np.isnan(packed)))
        if not oracle:
            assert n_host == 0, where + ("host packers", n_host, at_host, got[at_host], packed[at_host])
            continue
        ref = O.match_template(img, t, method, mask=mask, corr="direct")
        both_nan = np.isnan(got) & np.isnan(ref)
        if masked:
            with np.errstate(invalid="ignore"):
                err = np.abs(got.astype(np.float64) - ref) / (1e-6 * np.maximum(1.0, np.abs(ref)))
            err[both_nan | (got == ref)] = 0.0
            err[np.isnan(err)] = np.inf
            worst = max(worst, float(err.max()))
            same = err <= 1.0
        else:
            same = (got == ref) | both_nan
        n_bad, at = _first_bad(same)
        assert n_bad == 0 and n_host == 0, where + (
            "outputs that differ from the oracle's: %d, first at %r: %r / %r" % (n_bad, at, at and got[at], at and ref[at]),
            "from the host packers': %d, first at %r: %r / %r" % (n_host, at_host, at_host and got[at_host], at_host and packed[at_host]))
    return worst


def _check_tilings(dev, cell, method):
    recs = dev.class_tilings()
    want = M.cell_classes(cell, method)
    assert [(r["h"], r["w"], r["n_templates"]) for r in recs] == [c[:3] for c in want], (cell["name"], method, recs)
    out = []
    for r, (h, w, n, exp, views) in zip(recs, want):
        assert M.family_of(r) == exp["family"], (cell["name"], method, exp, r)
        for f, v in exp.items():
            if f != "family":
                assert r[f] == v, (cell["name"], method, f, exp, r)
        out.append((exp["family"], frozenset(views)))
    return out


@pytest.mark.parametrize("name", M.NAMES)
def test_cell(lib, pair, name):
    dev, host = pair
    cell = M.BY_NAME[name]
    t0 = time.perf_counter()
    bases = M.cell_bases(cell)
    units = M.expand(bases, cell["recs"])
    img = M.cell_image(cell, units)
    _set_kernel(lib, pair, cell["kernel"])
    entered, worst = [], 0.0
    try:
        for method in cell["methods"]:
            worst = max(worst, _compare_maps(lib, dev, host, cell, bases, cell["recs"], units, img, method))
            if cell["tilings"] and default_routes():
                entered += _check_tilings(dev, cell, method)
            else:
                entered += [(M.family_of(r), frozenset()) for r in dev.class_tilings()]
        if entered and cell["tilings"] and default_routes():
            _CONFIRMED[name] = entered
        if cell["mask"]:
            _WORST[name] = worst
        # hits-only against map mode (just checked against exact sums), records byte for byte
        method = cell["methods"][-1]
        if not cell["mask"] and len(M.cell_classes(cell, method)) == 1 and method in (1, 3, 5):
            thr = 0.5
            dev.set_templates_augmented(bases, list(cell["recs"]), method)
            ref = dev.find_matches_image(img, lib.PEAKS_LOCAL, thr).copy()
            assert 0 in set(ref["templ_idx"].tolist()), (name, len(ref))          # the planted copy of unit 0 is listed
            dev.set_option(lib.OPT_HITS_ONLY, 1)
            try:
                dev.debug_poison(0x7F, 7)
                got = dev.find_matches_image(img, lib.PEAKS_LOCAL, thr).copy()
            finally:
                dev.set_option(lib.OPT_HITS_ONLY, 0)
            assert got.tobytes() == ref.tobytes(), (name, thr, len(got), len(ref))
    finally:
        _set_kernel(lib, pair, "auto")
        _SECONDS[name] = time.perf_counter() - t0
        print("templ_device %-24s %5.2f s  %s  worst/tol %s" % (
            name, _SECONDS[name], " ".join(sorted({f for f, _ in entered})) or "-",
            ("%.3g" % _WORST[name]) if name in _WORST else "-"))


@pytest.mark.parametrize("shape,chans", M.READOUT, ids=["%dx%dx%d" % (s + (c,)) for s, c in M.READOUT])
def test_readout_of_the_packed_pixels(lib, pair, shape, chans):
    """TM_CCORR against an image that is zero but for one pixel of value 1: the map, flipped in both axes, is the unit's pixels
    as the packs hold them - exact in float32, compared byte for byte with the model, one image per channel."""
    dev, _ = pair
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, shape + ((chans,) if chans > 1 else ())).astype(np.uint8)
    units = M.expand([(base, None)], M.RECORDS16)
    P = max(shape) - 1
    dev.set_templates_augmented([(base, None)], list(M.RECORDS16), 2)
    for c in range(chans):
        img = np.zeros((2 * P + 1, 2 * P + 1) + ((chans,) if chans > 1 else ()), np.uint8)
        img[(P, P) + ((c,) if chans > 1 else ())] = 1
        dev.debug_poison(0xFF, 7)
        dev.find_matches_image(img, lib.PEAKS_LOCAL, 1e30)
        for i, (t, _) in enumerate(units):
            m = dev.last_score_map(i, _map_shape(img, t))
            want = t[:, :, c] if chans > 1 else t
            ys, xs = np.indices(want.shape)
            got = m[P - ys, P - xs]
            n_bad, at = _first_bad(got == want.astype(np.float32))
            assert n_bad == 0, "unit %d record %r channel %d: %d pixels differ, first at (y, x) = %r: packed %r, model %r" % (
                i, M.RECORDS16[i], c, n_bad, at, got[at], want[at])
            rest = np.ones(m.shape, bool)
            rest[P - ys, P - xs] = False
            assert not m[rest].any(), (i, M.RECORDS16[i], c)


def test_a_resize_that_leaves_nothing_is_refused(lib, pair):
    """A factor larger than a base and a variant that names both a size and a factor are MTM_E_INVALID (-1), again on the same
    call repeated (the refused set is not remembered as the current one); the set the context had before is placed again
    afterwards and gives the maps it gave."""
    dev, host = pair
    cell = M.BY_NAME["rs-views"]
    bases = M.cell_bases(cell)
    recs = cell["recs"][::5]
    units = M.expand(bases, recs)
    img = M.cell_image(cell, units)
    _compare_maps(lib, dev, host, cell, bases, recs, units, img, 5, oracle=False)
    before = [dev.last_score_map(i, _map_shape(img, u[0])) for i, u in enumerate(units)]
    for bad in ([M.rec(), M.rec(down=18)], [M.rec(down=38)], [M.rec(1, rows=3, cols=3, down=2)], [M.rec(rows=4, cols=0)], [M.rec(4)]):
        for _ in range(2):
            with pytest.raises(lib.MtmError, match=r"\(-1\)"):
                dev.set_templates_augmented(bases, bad, 5)
    with pytest.raises(lib.MtmError):
        dev.set_templates_augmented(bases, [], 5)
    dev.debug_poison(0xFF, 7)
    dev.set_templates_augmented(bases, list(recs), 5)
    dev.find_matches_image(img, lib.PEAKS_LOCAL, 2.0)
    for i, u in enumerate(units):
        assert np.array_equal(dev.last_score_map(i, _map_shape(img, u[0])), before[i], equal_nan=True), i


def test_one_context_through_several_sets(lib, pair):
    """A large augmented set, a smaller one with other shapes, a plain set, the first again - on one context: every call's maps
    equal a fresh context's.  Sources of 1 x 1 and 3 x 5 ahead of the others put arena offsets off every multiple of 64; the
    staging copies, the unit table and the sums buffer are reused from set to set."""
    dev, host = pair
    rng = np.random.default_rng(23)
    mk = lambda *s: rng.integers(0, 256, s).astype(np.uint8)                                              # noqa: E731
    big = ([(mk(1, 1), None), (mk(3, 5), None), (mk(37, 41), None), (mk(64, 17), None), (mk(24, 49), None)],
           [M.rec(), M.rec(1), M.rec(2, 1, 0), M.rec(3, 0, 1, down=1), M.rec(rows=9, cols=11), M.rec(1, 1, 0, rows=2, cols=3)])
    small = ([(mk(3, 5), None), (mk(22, 16), None)], [M.rec(1, 0, 1), M.rec(0, 1, 0, down=2), M.rec(down=3)])
    plain = [(mk(21, 15), None), (mk(9, 81), None), (mk(2, 2), None)]
    img = (rng.integers(0, 256, (90, 120)) * (rng.random((90, 120)) < 0.35)).astype(np.uint8)

    def maps(ctx, what):
        ctx.debug_poison(0xFF, 7)
        if isinstance(what, tuple):
            ctx.set_templates_augmented(what[0], what[1], 5)
            units = M.expand(*what)
        else:
            ctx.set_templates(what, 5)
            units = what
        ctx.find_matches_image(img, lib.PEAKS_LOCAL, 2.0)
        return [ctx.last_score_map(i, _map_shape(img, u[0])) for i, u in enumerate(units)], units

    sequence = (big, small, plain, big, small)
    fresh = []
    for what in sequence[:3]:
        ctx = lib.Context(0)
        try:
            ctx.set_option(lib.OPT_HITS_ONLY, 0)
            ctx.set_option(lib.OPT_EXACT_DIV, 1)
            got, units = maps(ctx, what)
        finally:
            ctx.close()
        for m, (t, _) in zip(got, units):                                  # the fresh context's maps are right
            ref = O.match_template(img, t, 5, corr="direct")
            assert np.array_equal(m, ref, equal_nan=True)
        fresh.append(got)
    for step, what in enumerate(sequence):
        got, _ = maps(dev, what)
        want = fresh[(big, small, plain).index(what)]
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a, b, equal_nan=True), (step, i)


@pytest.mark.parametrize("dtype,chans", M.IMAGE_DOWN, ids=["%s-%dch" % d for d in M.IMAGE_DOWN])
def test_image_side_downscale(lib, pair, dtype, chans):
    """set_image(img, downscale=f), f = 2, 3, 5, 7 with remainders in both axes, read out byte for byte through TM_CCORR with
    1 x 1 templates (RGB: one per channel, one-hot): the planes equal the model's integer rule; float32 images through the naive
    kernel, whose map against a template of 1.0 is the image's float32 bits."""
    dev, _ = pair
    rng = np.random.default_rng(31)
    npdt = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}[dtype]
    H, W = M.IMAGE_DOWN_SHAPE
    full = (H, W) + ((chans,) if chans > 1 else ())
    if dtype == "f32":
        img = (rng.standard_normal(full) * 100.0).astype(np.float32)
    else:
        img = rng.integers(0, int(np.iinfo(npdt).max) + 1, full).astype(npdt)
        img[:6, :6] = np.iinfo(npdt).max                                   # saturated blocks under every factor ...
        img[6:12, :6] = 0
        img[12:14, 0:2] = np.array([[1, 0], [0, 1]], npdt).reshape((2, 2) + (1,) * (len(full) - 2))   # ... and a factor-2 tie
    units = []
    for c in range(chans):
        t = np.zeros((1, 1) + ((chans,) if chans > 1 else ()), npdt)
        t[(0, 0) + ((c,) if chans > 1 else ())] = 1
        units.append((t, None))
    _set_kernel(lib, (dev,), "naive" if dtype == "f32" else "auto")
    try:
        for f in M.FACTORS:
            want = M.downscale_int_exact(img, f)
            dev.debug_poison(0xFF, 7)
            dev.set_image(img, downscale=f)
            dev.set_templates(units, 2)
            dev.find_matches(lib.PEAKS_LOCAL, 1e30)
            if dtype == "f32" and default_routes():
                assert [r["kernel"] for r in dev.class_tilings()] == [1]
            for c in range(chans):
                got = dev.last_score_map(c, want.shape[:2])
                plane = want[:, :, c] if chans > 1 else want
                if dtype == "f32":
                    same = got.view(np.uint32) == np.ascontiguousarray(plane).view(np.uint32)
                else:
                    same = got == plane.astype(np.float32)
                n_bad, at = _first_bad(same)
                assert n_bad == 0, (dtype, chans, f, c, n_bad, at, got[at], plane[at])
    finally:
        _set_kernel(lib, (dev,), "auto")


def test_the_sweep_reached_every_family():
    """The table names every family (tests/test_templ_device_model_cpu.py holds it to that); every cell that ran on the default
    routes in this session passed its tiling assertion, and together they reached every family through a view that is not the
    identity."""
    assert {f for c in M.CELLS for m in c["methods"] for *_, e, _v in M.cell_classes(c, m) for f in [e["family"]]} == set(M.FAMILIES)
    if set(_CONFIRMED) != {c["name"] for c in M.CELLS if c["tilings"]}:
        return                                                             # a partial run (-k), or a route switch
    reached = {}
    for name, entered in _CONFIRMED.items():
        for fam, views in entered:
            reached.setdefault(fam, set()).update(views)
    for fam in M.FAMILIES:
        assert reached.get(fam, set()) - {M.IDENTITY}, fam
    for fam in M.VIEW_FAMILIES:
        assert len(reached[fam]) == 8, (fam, len(reached[fam]))
