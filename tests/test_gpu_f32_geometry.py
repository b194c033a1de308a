"""
ncc_bf16_kernel at the edges of its geometry rules, against float64 sums and against a model of its own arithmetic (-m gpu).

Everything MTM_OPT_F32_MFMA = 1 returns is the float64 kernel's record only while |bf16 score - exact score| <= M holds at
every output (Bf16Params::rig).  The kernel has as many geometry rules as the int8 kernel - 32-tap blocks (nkb = 1 .. 8, the
taps w .. 32 nkb - 1 padding), K chunks of 64 or 32 template rows, two differently pipelined K loops with their remainder
steps, one or two groups of 16 templates per wave, the single-template launch, 128 x 4 output tiles with their right and
bottom edges, a tile constant from a clamped sample grid, 1 .. kMaxChans channels - and "the bound holds" alone leaves a tenfold
margin on ordinary data: a dropped tap would pass it.  So every cell compares the kernel's maps

  * with tests/f32_model.py::model_scores - the same pieces multiplied exactly - to accum_map, the ACCUMULATION term of the
    bound alone (mtm_ctx.h::bf16_rig_eps: two roundings per MFMA, doubled; taken from there, not tuned), and
  * with the oracle's direct float64 sums to bound_map, the whole bound,

with three piece products (MTM_OPT_F32_MFMA = 2) and with one (= 4), through the single-template launch (score_map) and
through a map-mode search, from poisoned memory; and the records of the default route (= 1; local extrema hits-only and with
maps in memory, the global extremum of all six methods) bit for bit with the float64 kernel's (= 0) and with the oracle's
peak rule on the oracle's map.  tests/test_f32_model_cpu.py shows on the CPU that the model itself meets bound_map on every
cell's scenes and that at least 99 % of every map is compared.

Which outputs are compared: all where |score| < 1 in both maps (the saturation rules apply beyond) and the window is not
flat; at least 99 % of a map's outputs, an exact copy's own position (score 1) not counted - on the 2 x 2 .. 5 x 9 maps of the
output-geometry cells that one position alone is up to a quarter of the map.  A constant template under TM_CCOEFF_NORMED is 1
everywhere by rule: compared exactly.  Impulse templates (one non-zero tap) go with methods 5 and 3: under TM_SQDIFF_NORMED
they saturate at every output.  Scenes by method as measured on the oracle alone (test_f32_model_cpu.py): TM_SQDIFF_NORMED
saturates on zero-mean noise and on 29 - 44 % of a step image, so it takes `noise+` and `offset` only.

A cell with "n = 1" in the sense of the kernel - one group of at most 16 templates, MB = 1 - carries its 4 .. 16 templates in one
list; its first template also runs alone, as a list of one.
"""
import zlib

import numpy as np
import pytest

import f32_model as F
import mtm_oracle as O
from test_gpu_tilings import default_routes

pytestmark = pytest.mark.gpu

SCENE_METHODS = {"noise+": (5, 3, 1), "signed": (5, 3), "offset": (5, 3, 1), "step": (5, 3)}
# the scene x method pairs a cell takes besides noise+ x (5, 3, 1), in rotation over the table
_EXTRA = [("signed", 5), ("offset", 3), ("step", 5), ("offset", 1), ("signed", 3), ("step", 3), ("offset", 5)]
DEFAULT_MAP, SMALL_MAP = (9, 133), (5, 41)      # 133: the second 128-column segment holds 5 outputs; 9: the third row block one row


# ---- the table -----------------------------------------------------------------------------------------------------------
CELLS = []


def _cell(family, h, w, n=0, chans=1, out=None, kernel=5):
    """n = 0: the cell's own 4 .. 16 templates in one group (MB = 1); n > 0: a list of exactly n."""
    if out is None:
        out = DEFAULT_MAP if chans * h * w <= 20000 else SMALL_MAP     # (the oracle's and the model's direct sums: seconds)
    name = "%s-%dx%d" % (family, h, w) + ("-c%d" % chans if chans > 1 else "") + ("-n%d" % n if n else "") + \
           ("-o%dx%d" % out if family == "outputs" else "")
    extra = _EXTRA[len(CELLS) % len(_EXTRA)]
    CELLS.append(dict(name=name, family=family, h=h, w=w, n=n, chans=chans, out=out, kernel=kernel,
                      scenes=(("noise+", SCENE_METHODS["noise+"]), (extra[0], (extra[1],)))))


# tap blocks: nkb = 1 .. 8 on both sides of every block boundary
for _w in (7, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 224, 225, 255, 256):
    _cell("taps", 5, _w)
_cell("off_cores", 5, 257, kernel=0)                    # w > kBfMaxW: the float64 kernel
# chunks: chunk_h = 64 at nkb <= 2, 32 beyond
for _h in (63, 64, 65, 69, 128, 129):
    _cell("chunks", _h, 33)
for _h in (31, 32, 33, 64, 65, 97):
    _cell("chunks", _h, 97)
# step residues: nsteps = ch nkb; w = 20: nkb = 1, nsteps = h; w = 70: nkb = 3
for _h in range(1, 10):
    _cell("steps", _h, 20)
for _h in (3, 5):
    _cell("steps", _h, 70)
# (added: odd residues in a LAST chunk need an odd nkb and more than one chunk - w = 20, h = 64 + r: the last chunk has r steps)
for _h in range(65, 72):
    _cell("steps", _h, 20)
# template lists: MB = 1 up to 16 templates, 2 beyond; ntg = ceil(n / (16 MB))
for _n in (1, 15, 16, 17, 31, 32, 33, 49):
    _cell("lists", 24, 40, n=_n)
# channels (2 and kMaxChans: map mode only - the hits-only routes take 1 or 3 channels)
_cell("channels", 7, 40, chans=3)
_cell("channels", 33, 250, chans=3)
_cell("channels", 24, 40, chans=3, n=17)
_cell("channels", 7, 40, chans=2)
_cell("channels", 7, 40, chans=F.K_MAX_CHANS)
# output geometry: ow mod 4 = 0 .. 3, images narrower than the tile (the sample grid clamps), a third segment of one column
for _out in ((2, 2), (3, 7), (4, 8), (5, 9), (9, 127), (9, 128), (9, 129), (5, 257)):
    _cell("outputs", 5, 31, out=_out)

_NAMES = [c["name"] for c in CELLS]
assert len(set(_NAMES)) == len(_NAMES)


# ---- a cell's scenes and templates ---------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def scene_image(cell, scene):
    h, w, chans, (oh, ow) = cell["h"], cell["w"], cell["chans"], cell["out"]
    shape = (h + oh - 1, w + ow - 1) + ((chans,) if chans > 1 else ())
    rng = _rng(cell["name"], scene)
    if scene == "noise+":
        return rng.normal(100.0, 40.0, shape).astype(np.float32)
    if scene == "signed":
        return rng.normal(0.0, 40.0, shape).astype(np.float32)
    if scene == "offset":
        return rng.normal(1000.0, 5.0, shape).astype(np.float32)
    assert scene == "step"
    # test_gpu_parity.py::_step_image's geometry at this size: a 0 -> 1 step down the middle, texture of 2e-3 on both sides, one
    # patch of 0.2 on the dark side - windows beside the step are nearly flat while their tile constant sits half way up
    rows, cols = shape[:2]
    im = np.zeros(shape, np.float32)
    im[:, cols // 2:] = 1.0
    im += rng.normal(0.0, 2e-3, shape).astype(np.float32)
    r0, c0, pr, pc = rows // 8, cols // 16, max(2, rows // 3), max(2, cols // 5)
    im[r0:r0 + pr, c0:c0 + pc] += rng.normal(0.0, 0.2, im[r0:r0 + pr, c0:c0 + pc].shape).astype(np.float32)
    return im


_NOISE = {"noise+": 10.0, "signed": 10.0, "offset": 1.25, "step": 5e-4}
_CONST = {"noise+": 100.0, "signed": 7.0, "offset": 1000.0, "step": 0.5}


def impulse_taps(h, w):
    """(dy, dx) of the impulse templates: every column block edge x every chunk edge, at most 12."""
    ch = F.chunk_h_of(w)
    dxs = sorted({d for d in (0, 31, 32, w - 1) if 0 <= d < w})
    dys = sorted({d for d in (0, ch - 1, ch, h - 1) if 0 <= d < h})
    taps = [(i, j) for i in range(len(dys)) for j in range(len(dxs))]
    if len(taps) > 12:
        taps = [(i, j) for i, j in taps if not ((i + j) % 2 == 1 and i in (1, 2))]
    return [(dys[i], dxs[j]) for i, j in taps]


def template_kinds(cell, scene, method):
    imp = [("imp", t) for t in impulse_taps(cell["h"], cell["w"])] if method in (5, 3) else []
    kinds = [("noisy", None), ("exact", None), ("const", None), ("cut" if scene == "step" else "noisy", None)] + imp
    if cell["n"]:
        kinds = kinds[:cell["n"]]
        while len(kinds) < cell["n"]:
            kinds.append(("exact" if len(kinds) % 2 else "noisy", None))
    assert cell["n"] or 4 <= len(kinds) <= 16
    return kinds


def templates(cell, scene, method, img):
    """[(kind, template)] of a cell under a method: copies are cut at the same places whatever the method."""
    h, w, (oh, ow) = cell["h"], cell["w"], cell["out"]
    out = []
    for k, (kind, tap) in enumerate(template_kinds(cell, scene, method)):
        rng = _rng(cell["name"], scene, "t", k, kind)
        y, x = int(rng.integers(0, oh)), int(rng.integers(0, ow))
        if kind == "cut":
            x = img.shape[1] // 2 - w // 2
        t = np.array(img[y:y + h, x:x + w], np.float32)
        if kind == "noisy":
            t += rng.normal(0.0, _NOISE[scene], t.shape).astype(np.float32)
        elif kind == "const":
            t[:] = _CONST[scene]
        elif kind == "imp":
            t[:] = 0.0
            t[tap[0], tap[1]] = 64.0
        out.append((kind, np.ascontiguousarray(t)))
    return out


def map_picks(cell, kinds):
    """The templates whose whole maps are compared: all of a small cell; of a list the first and last of every group of 16
    and every special one."""
    n = len(kinds)
    if not cell["n"]:
        return list(range(n))
    picks = {i for g in range(0, n, 16) for i in (g, min(g + 15, n - 1))}
    return sorted(picks | {i for i, k in enumerate(kinds) if k in ("const", "imp", "cut")})


def single_picks(cell, kinds):
    """... and through the single-template launch, which recomputes tg0, n_list and only_li."""
    n = len(kinds)
    return sorted({0, n - 1} | ({i for i in (15, 16, 31, 32) if i < n} if cell["n"] else {1, 2}))


def oracle_map(img, t, method, memo):
    """O.match_template(img, t, method, corr="direct"); `memo` (one dict per image) keeps the direct float64 correlation of a
    template, which every method's epilogue starts from."""
    real, key = O.sliding_corr, zlib.crc32(t.tobytes())

    def once(img2d, ker2d, exact_int=False, force=None, cache=None, cache_key=None):
        if (key, cache_key) not in memo:
            memo[(key, cache_key)] = real(img2d, ker2d, exact_int=exact_int, force=force)
        return memo[(key, cache_key)]
    O.sliding_corr = once
    try:
        return O.match_template(img, t, method, corr="direct")
    finally:
        O.sliding_corr = real


def compared(kind, a, b, live):
    """The outputs a comparison covers and whether they are enough of the map (see the module's docstring)."""
    with np.errstate(invalid="ignore"):
        unsat = live & (np.abs(a) < 1.0) & (np.abs(b) < 1.0)
    need = unsat.size
    if kind in ("exact", "cut"):            # (the template cut across the step is an exact copy too)
        need -= 1
    return unsat, int(unsat.sum()) >= 0.99 * need


def always_one(kind, method):
    return kind == "const" and method == 5


# ---- the GPU side --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import build as mtm_build
    mtm_build.build()
    from MTM import _lib
    assert _lib.load().mtm_device_count() >= 1
    return _lib


_WORST = {}             # (pieces, "accum" | "bound") -> (worst error / tolerance, cell)
_CELL_WORST = {}        # cell name -> {(pieces, "accum" | "bound"): worst error / tolerance of that cell}
_RAN = {}               # cell name -> seconds


def _note(pieces, what, ratio, name):
    mine = _CELL_WORST.setdefault(name, {})
    mine[(pieces, what)] = max(ratio, mine.get((pieces, what), 0.0))
    if ratio > _WORST.get((pieces, what), (0.0, ""))[0]:
        _WORST[(pieces, what)] = (ratio, name)


class _Poison:
    def __init__(self):
        self.k = 0

    def __call__(self, ctx):
        self.k += 1
        ctx.debug_poison(0xFF if self.k % 2 else 0x7F, 7)


def _check_placement(ctx, cell, n):
    recs = ctx.class_tilings()
    assert len(recs) == 1, recs
    r = recs[0]
    assert (r["h"], r["w"], r["n_templates"], r["kernel"]) == (cell["h"], cell["w"], n, cell["kernel"]), (cell["name"], r)


def _refs(cell, scene, method, img, tl, picks, memo):
    """Per picked template: (oracle map, {pieces: model map}, {pieces: (accum_map, bound_map, live)})."""
    out = {}
    if cell["w"] > F.MAX_W:                     # off the matrix cores: nothing to model
        return {i: (oracle_map(img, tl[i][1], method, memo).astype(np.float64), None, None) for i in picks}
    model = {pc: dict(zip(picks, F.model_scores_many(img, [tl[i][1] for i in picks], method, pc))) for pc in (3, 1)}
    for i in picks:
        out[i] = (oracle_map(img, tl[i][1], method, memo).astype(np.float64),
                  {pc: model[pc][i].astype(np.float64) for pc in (3, 1)},
                  {pc: F.tolerances(img, tl[i][1], method, pc) for pc in (3, 1)})
    return out


def _compare_map(cell, what, kind, method, pieces, got, ref, on_cores):
    name = cell["name"]
    exact, model, tol = ref
    got = got.astype(np.float64)
    if always_one(kind, method):
        assert np.array_equal(got, np.ones_like(got)), (name, what, "a constant template under TM_CCOEFF_NORMED is 1")
        return
    if not on_cores:
        # the float64 kernel (the off-cores cell, or a route switch of the environment): the oracle at 1e-6 relative
        bad = np.abs(got - exact) > 1e-6 * np.maximum(1.0, np.abs(exact))
        assert not bad.any(), (name, what, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        return
    A, M, live = tol[pieces]
    for versus, other, T in (("accum", model[pieces], A), ("bound", exact, M)):
        unsat, enough = compared(kind, got, other, live)
        assert enough, (name, what, versus, "compared %d of %d outputs" % (int(unsat.sum()), unsat.size))
        d = np.abs(got - other)
        ratio = float((d[unsat] / T[unsat]).max()) if unsat.any() else 0.0
        _note(pieces, versus, ratio, name)
        bad = unsat & ~(d <= T)
        assert not bad.any(), "%s %s: %d outputs beyond %s_map (worst %.3f of it), rows %s columns %s, first %r / %r" % (
            name, what, int(bad.sum()), versus, ratio, sorted(set(np.argwhere(bad)[:, 0].tolist()))[:6],
            sorted(set(np.argwhere(bad)[:, 1].tolist()))[:12], got[tuple(np.argwhere(bad)[0])], other[tuple(np.argwhere(bad)[0])])


def _kernel_maps(lib, cell, ctxs, poison, scene, method, img, tl, refs):
    """Step 2: the maps of three and of one piece product, through score_map and through a map-mode search."""
    name, shape, on_cores = cell["name"], cell["out"], cell["kernel"] == 5
    units = [(t, None) for _, t in tl]
    kinds = [k for k, _ in tl]
    nothing = -1.0 if method == 1 else 2.0          # a threshold no score passes: the maps are what is checked
    for pieces in (3, 1):
        ctx = ctxs[pieces]
        want_pieces = pieces if on_cores else 0
        # the single-template launch
        ctx.set_image(img)
        ctx.set_templates(units, method)
        for i in single_picks(cell, kinds):
            poison(ctx)
            got = ctx.score_map(i, shape)
            tm = ctx.timing()
            if default_routes():
                assert (tm["kernel_used"], tm["f32_pieces"]) == (cell["kernel"], want_pieces), (name, tm)
            if i in refs:
                _compare_map(cell, "%s m%d np%d score_map(%d)" % (scene, method, pieces, i), kinds[i], method, pieces, got, refs[i],
                             tm["kernel_used"] == 5)
        # a map-mode search, then the maps it left
        poison(ctx)
        ctx.search(units, img, method, lib.PEAKS_LOCAL, nothing)
        tm = ctx.timing()
        if default_routes():
            assert (tm["kernel_used"], tm["f32_pieces"]) == (cell["kernel"], want_pieces), (name, tm)
            _check_placement(ctx, cell, len(tl))
        for i in sorted(refs):
            _compare_map(cell, "%s m%d np%d search map %d" % (scene, method, pieces, i), kinds[i], method, pieces,
                         ctx.last_score_map(i, shape), refs[i], tm["kernel_used"] == 5)
    if not cell["n"]:
        # the first template alone: a list of one
        ctx = ctxs[3]
        poison(ctx)
        ctx.search(units[:1], img, method, lib.PEAKS_LOCAL, nothing)
        if default_routes():
            _check_placement(ctx, cell, 1)
        _compare_map(cell, "%s m%d np3 alone" % (scene, method), kinds[0], method, 3, ctx.last_score_map(0, shape), refs[0],
                     ctx.timing()["kernel_used"] == 5)


def _oracle_records(maps, method, mode, thr, border):
    rows = []
    for i, m in enumerate(maps):
        if mode == 1:
            _, _, mn, mx = O.min_max_loc(m)
            peaks = [mn[::-1]] if method in (0, 1) else [mx[::-1]]
        elif method in (0, 1):
            peaks = O.find_local_min(m, thr, border=border)
        else:
            peaks = O.find_local_max(m, thr, border=border)
        rows += [(i, int(p[0]), int(p[1]), float(m[tuple(p)])) for p in peaks]
    return sorted(rows)


def _same_as_oracle(name, what, got, exp):
    rows = sorted((int(r["templ_idx"]), int(r["y"]), int(r["x"]), float(r["score"])) for r in got)
    assert [r[:3] for r in rows] == [e[:3] for e in exp], (name, what, len(rows), len(exp),
                                                          sorted(set(r[:3] for r in rows) ^ set(e[:3] for e in exp))[:6])
    for r, e in zip(rows, exp):
        assert abs(r[3] - e[3]) <= 1e-6 * max(1.0, abs(e[3])), (name, what, r, e)


def _thresholds(maps, kinds, method, border):
    """One threshold 4e-4 on the far side of the weakest non-constant template's best score, and four within 1e-5 on either
    side of two true peak scores (unsaturated ones no other peak's score comes within 3e-6 of the threshold of: the float64
    kernel and the oracle agree to ~1e-7, not to the bit)."""
    lower = method == 1
    best = [float(m.min() if lower else m.max()) for m, k in zip(maps, kinds) if k != "const"]
    thr_all = max(best) + 4e-4 if lower else min(best) - 4e-4
    peaks = np.array([r[3] for r in _oracle_records(maps, method, 0, thr_all, border)])
    inner = sorted(s for s in set(peaks.tolist()) if 1e-3 < s < 1.0 - 1e-3)
    thrs = [thr_all]
    for s in inner[len(inner) // 3::max(1, len(inner) // 3)]:
        cand = [s - 1e-5, s + 1e-5]
        if all(np.abs(peaks - t).min() > 3e-6 for t in cand) and len(thrs) < 5:
            thrs += cand
    return thrs


def _records(lib, cell, fast, exact, poison, img, lists, omaps):
    """Step 3: the default route's records are the float64 kernel's, and the oracle's."""
    name = cell["name"]
    both_halves = cell["chans"] in (1, 3)
    border = {0: "constant", 1: "nearest"}[fast.get_option(lib.OPT_PEAK_BORDER)]
    for method in (5, 3, 1):
        units = [(t, None) for _, t in lists[method]]
        kinds = [k for k, _ in lists[method]]
        for thr in _thresholds(omaps[method], kinds, method, border):
            exact.set_option(lib.OPT_HITS_ONLY, 0)
            ref = exact.search(units, img, method, lib.PEAKS_LOCAL, thr).copy()
            assert exact.timing()["kernel_used"] == 0 or not default_routes()
            _same_as_oracle(name, ("local", method, thr), ref, _oracle_records(omaps[method], method, 0, thr, border))
            for honly in ((1, 0) if both_halves else (0,)):
                fast.set_option(lib.OPT_HITS_ONLY, honly)
                poison(fast)
                got = fast.search(units, img, method, lib.PEAKS_LOCAL, thr).copy()
                tm = fast.timing()
                assert got.tobytes() == ref.tobytes(), (name, method, thr, honly, tm["f32_route"], tm["f32_pieces"], len(got), len(ref))
                if default_routes() and cell["kernel"] == 5:
                    # hits-only starts with one piece product (three after an overflow of its list); maps in memory are the
                    # three-product kernel's; route 3 is the float64 kernel behind an overflowed scan
                    assert tm["f32_route"] in (1, 2, 3) and (honly or tm["f32_pieces"] in (0, 3)), (name, tm)
                    assert tm["f32_route"] != 1 or tm["f32_pieces"] in ((1, 3) if honly else (3,)), (name, tm)
    if not both_halves:
        return
    for method in (5, 3, 1, 0, 2, 4):
        lm = method if method in (5, 3) else 1              # (the raw sums take the list without impulses, as TM_SQDIFF_NORMED)
        units = [(t, None) for _, t in lists[lm]]
        exact.set_option(lib.OPT_HITS_ONLY, 1)
        ref = exact.search(units, img, method, lib.PEAKS_GLOBAL, 0.0).copy()
        fast.set_option(lib.OPT_HITS_ONLY, 1)
        poison(fast)
        got = fast.search(units, img, method, lib.PEAKS_GLOBAL, 0.0).copy()
        assert got.tobytes() == ref.tobytes(), (name, "global", method, fast.timing()["f32_route"])
        # (a constant template's TM_CCOEFF map is 0 up to the rounding of two equal sums: its extremum is nowhere in particular)
        keep = [i for i, (k, _) in enumerate(lists[lm]) if not (method == 4 and k == "const")]
        exp = [r for r in _oracle_records(omaps[method], method, 1, 0.0, border) if r[0] in keep]
        _same_as_oracle(name, ("global", method), ref[np.isin(ref["templ_idx"], keep)], exp)


@pytest.mark.parametrize("cell", CELLS, ids=_NAMES)
def test_f32_geometry_cell(lib, cell):
    import time
    t_start = time.perf_counter()
    name = cell["name"]
    ctxs = {3: lib.Context(0), 1: lib.Context(0)}
    fast, exact = lib.Context(0), lib.Context(0)
    poison = _Poison()
    try:
        ctxs[3].set_option(lib.OPT_F32_MFMA, 2)         # the bf16 scores as they are, three piece products
        ctxs[1].set_option(lib.OPT_F32_MFMA, 4)         # ... one
        exact.set_option(lib.OPT_F32_MFMA, 0)
        for c in ctxs.values():
            c.set_option(lib.OPT_HITS_ONLY, 0)
        lists, omaps, memos = {}, {}, {}
        for scene, methods in cell["scenes"]:
            img = scene_image(cell, scene)
            memo = memos.setdefault(scene, {})
            for method in methods:
                tl = templates(cell, scene, method, img)
                picks = map_picks(cell, [k for k, _ in tl])
                refs = _refs(cell, scene, method, img, tl, picks, memo)
                _kernel_maps(lib, cell, ctxs, poison, scene, method, img, tl, refs)
                if scene == "noise+":
                    lists[method] = tl
        # the records, on noise+: the oracle's maps of every template (one correlation per template for all methods)
        img = scene_image(cell, "noise+")
        for lm, methods in ((5, (5,)), (3, (3,)), (1, (1, 0, 2, 4))):
            for m in methods:
                omaps[m] = [oracle_map(img, t, m, memos["noise+"]) for _, t in lists[lm]]
        _records(lib, cell, fast, exact, poison, img, lists, omaps)
    finally:
        for c in list(ctxs.values()) + [fast, exact]:
            c.close()
    _RAN[name] = time.perf_counter() - t_start
    print("%s: %.2f s; worst error / tolerance: %s" % (name, _RAN[name], ", ".join(
        "np%d %s %.3f" % (pc, what, r) for (pc, what), r in sorted(_CELL_WORST.get(name, {}).items()))))


def test_the_table_covers_every_edge():
    """A table edit cannot silently drop an edge: on the table itself."""
    on = [c for c in CELLS if c["kernel"] == 5]
    # 32-tap blocks: every nkb, and a full last block, a last block of one tap and of 31
    assert {F.nkb_of(c["w"]) for c in on} == set(range(1, 9))
    taps = {c["w"] for c in on if c["family"] == "taps"}
    assert taps >= {7, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 224, 225, 255, 256}
    assert [c for c in CELLS if c["kernel"] == 0] and all(c["w"] > F.MAX_W for c in CELLS if c["kernel"] == 0)
    assert max(c["w"] for c in on) == F.MAX_W
    # chunks: both regimes, one row below, at, and above each boundary, two full chunks and two full chunks + 1
    for w, ch in ((33, 64), (97, 32)):
        hs = {c["h"] for c in on if c["w"] == w and c["family"] == "chunks"}
        assert F.chunk_h_of(w) == ch and hs >= {ch - 1, ch, ch + 1, 2 * ch, 2 * ch + 1}, (w, sorted(hs))
    assert any(F.nkb_of(c["w"]) == 8 and c["h"] > 32 and c["chans"] == 3 for c in on)           # chunks per channel
    # step residues: nsteps mod 8 in a single chunk and in the last of several (the one-product loop: two stages of four
    # steps, guards left_ > 1 / 2 / 3); both parities for the three-product loop's remainder step
    single = {F.chunk_steps(c["h"], c["w"])[0] % 8 for c in on if len(F.chunk_steps(c["h"], c["w"])) == 1}
    last = {F.chunk_steps(c["h"], c["w"])[-1] % 8 for c in on if len(F.chunk_steps(c["h"], c["w"])) > 1}
    assert single == set(range(8)) and last == set(range(8)), (sorted(single), sorted(last))
    assert {F.chunk_steps(c["h"], c["w"])[0] for c in on} >= {1, 2, 3, 4, 5, 6, 7, 8, 9, 15}
    assert {s % 2 for c in on for s in F.chunk_steps(c["h"], c["w"])} == {0, 1}
    # lists: both sides of MB 1 -> 2 and of every group count; a second channel count with MB = 2
    assert {c["n"] for c in on if c["family"] == "lists"} >= {1, 15, 16, 17, 31, 32, 33, 49}
    assert any(c["n"] > 16 and c["chans"] == 3 for c in on)
    for c in on:
        for scene, methods in c["scenes"]:
            for m in methods:
                n = len(template_kinds(c, scene, m))
                assert (n == c["n"]) if c["n"] else (4 <= n <= 16), (c["name"], n)
    # channels
    assert {c["chans"] for c in on} == {1, 2, 3, F.K_MAX_CHANS}
    # outputs: ow mod 4, fewer columns than one sample-grid step, one and two full segments, one column in a last segment,
    # fewer rows than a row block, a last row block of one row
    outs = {c["out"] for c in on}
    assert outs >= {(2, 2), (3, 7), (4, 8), (5, 9), (9, 127), (9, 128), (9, 129), (5, 257), DEFAULT_MAP}
    assert {o[1] % 4 for o in outs} == {0, 1, 2, 3} and {o[0] % 4 for o in outs} == {0, 1, 2, 3}
    # scenes: every scene x method pair that leaves 99 % of a map compared occurs
    pairs = {(s, m) for c in on for s, ms in c["scenes"] for m in ms}
    assert pairs == {(s, m) for s, ms in SCENE_METHODS.items() for m in ms}
    # impulse taps: the block edges and the chunk edges where they exist
    assert set(impulse_taps(65, 33)) >= {(0, 0), (63, 31), (64, 32), (64, 0), (63, 0), (0, 32)} and len(impulse_taps(97, 97)) == 12
    assert {dx for _, dx in impulse_taps(97, 97)} == {0, 31, 32, 96} and {dy for dy, _ in impulse_taps(97, 97)} == {0, 31, 32, 96}
    if _RAN:
        slow = max(_RAN, key=_RAN.get)
        print("f32 geometry: %d cells in %.1f s, slowest %s %.2f s" % (len(_RAN), sum(_RAN.values()), slow, _RAN[slow]))
        for (pc, what), (ratio, name) in sorted(_WORST.items()):
            print("f32 geometry: %d piece product(s), worst error / %s_map = %.3f (%s)" % (pc, what, ratio, name))
