"""
The tilings of ncc_mfma_kernel at their geometry edges, against exact sums (-m gpu).

choose_tiling (csrc/mtm_placement.hip) sends a size class to one of a dozen forms of the score kernel purely by the class's
numbers - template count, h, w, channels, method, mask: row-multiplexed (packed K or not), plain (packed K or not, one to four
64-tap blocks), two-row (with the tail screen or without, in one K chunk or several), slabs, the uint16 byte-plane passes.  A
pack layout, a chunk boundary or a constant can be wrong for one residue of those numbers and right for every shape a
hand-picked test uses.  This is a table of cells at the edges of the rules; every cell

  1. asserts through Context.class_tilings() (mtm_debug_class_tilings) that the class really entered the tiling the cell is
     there for - the assertion that keeps the sweep honest when a rule moves;
  2. compares whole score maps (map mode, IEEE division: bit for bit; reciprocal mode and masked classes: 1e-6 max(1, |exp|))
     with the oracle's direct sums - exact integers, float64 epilogue in OpenCV's order - from poisoned memory;
  3. on the normalised methods, compares the hits-only records with map mode's byte for byte - on the cells whose class can
     screen its K loop at 0.5, 0.7 and just below the best score of a template with its structure in its last rows, where the
     call at 0.7 must really have carried a split.

The image is sparse noise (two thirds of the pixels 0): TM_CCORR_NORMED between unrelated windows of uniform noise is
E[I]^2 / E[I^2] = 0.75, every output of every template would pass 0.5 and 0.7, the candidate list would overflow and the
call would fall back to map mode - no screen.  Sparse noise puts that baseline at 0.2 (0.4 .. 0.5 for templates with flat
rows), and the zero pixels are the biased operands' -128.
"""
import os
import zlib

import numpy as np
import pytest

import mtm_oracle as O
from test_gpu_tail_screen import _OTHER_ROUTES

pytestmark = pytest.mark.gpu

# switches of tools/alt_modes.sh that move a class to another kernel, tiling or mode: the assertions about WHICH tiling a
# cell entered (and that a split was carried) only hold without them; the results are asserted always
_ROUTE_SWITCHES = tuple(sorted(set(_OTHER_ROUTES) | {"MTM_TEMPL_ON_DEVICE", "MTM_ROW_MUX", "MTM_SLAB_MFMA", "MTM_TAIL_SPLIT"}))


def default_routes():
    return not any(os.environ.get(k) for k in _ROUTE_SWITCHES)


@pytest.fixture(scope="module")
def lib():
    import build as mtm_build
    mtm_build.build()
    from MTM import _lib
    assert _lib.load().mtm_device_count() >= 1
    return _lib


# ---- the table -----------------------------------------------------------------------------------------------------------
# (name, dtype, chans, method, masked, n_templates, (h, w), expected tiling)
#   expected tiling: {"family", "kernel", "nz": the fields of (rm_nt, kp_nseg, r2, tail_ok, n_slabs) that are non-zero,
#                     further fields with their exact values, "kinds": the templates of a cell with fewer than eight}
_NZ_FIELDS = ("rm_nt", "kp_nseg", "r2", "tail_ok", "n_slabs")
CELLS = []


def _cell(family, shape, n, method, nz=(), dtype="u8", chans=1, masked=False, kernel=3, kinds=None, **exact):
    name = "%s-%dx%d-n%d-m%d" % (family, shape[0], shape[1], n, method)
    if kinds:
        name += "-" + "+".join(kinds)
    exp = dict(exact, family=family, kernel=kernel, nz=frozenset(nz), kinds=kinds)
    CELLS.append((name, dtype, chans, method, masked, n, shape, exp))


# two-row with the tail screen: w in 49 .. 64 (narrower normalised classes take packed K), 8 <= h <= 71 (one K chunk of 72)
for _shape in ((24, 49), (24, 56), (24, 63), (8, 64), (71, 64), (71, 49)):
    _cell("r2_screen", _shape, 20, 5, nz=("r2", "tail_ok"))
    _cell("r2_screen", _shape, 33, 3, nz=("r2", "tail_ok"))
_cell("r2_screen", (24, 63), 33, 5, nz=("r2", "tail_ok"))
_cell("r2_screen", (24, 49), 20, 3, nz=("r2", "tail_ok"))
# two-row without: h = 7 (below 8), h + 1 > 72 (several K chunks)
for _shape in ((7, 64), (72, 64), (73, 56), (129, 64)):
    for _m in (5, 3):
        _cell("r2_noscreen", _shape, 20, _m, nz=("r2",))
# two-row raw sums: any w <= 64.  (Placement marks 8 <= h <= 71 as able to screen whatever the method; a raw-sum call never
# carries a split - tail_split_for - and lists nothing here.)
for _m in (2, 4):
    for _shape in ((20, 3), (20, 17), (20, 48), (20, 64)):
        _cell("r2_raw", _shape, 20, _m, nz=("r2", "tail_ok"))
    _cell("r2_raw", (72, 33), 20, _m, nz=("r2",))
# plain, not packed: ceil(w / 16) a multiple of four and w > 64, or a method without a packed or two-row form
for _shape in ((5, 113), (64, 128), (65, 192), (20, 241), (20, 256)):
    for _m in (5, 3):
        _cell("plain", _shape, 20, _m)
_cell("plain", (20, 40), 20, 0)
# plain packed K: nseg = ceil(w / 16) in {1, 6, 7, 10, 11, 13, 14, 15}; h nseg % 4 = 1, 2, 3 (how full the last MFMA step
# is); w % 16 in {15, 0, 1}; h = 65: two chunks
for _shape, _nseg in (((21, 15), 1), ((22, 16), 1), ((9, 81), 6), ((9, 111), 7), ((7, 160), 10), ((7, 161), 11), ((7, 207), 13),
                      ((5, 224), 14), ((5, 225), 15), ((65, 40), 3)):
    assert (_shape[1] + 15) // 16 == _nseg and _shape[0] * _nseg % 4 != 0
    for _m in (5, 3):
        _cell("plain_kp", _shape, 20, _m, nz=("kp_nseg",), kp_nseg=_nseg)
assert {(s[0] * ((s[1] + 15) // 16)) % 4 for c in CELLS if c[7]["family"] == "plain_kp" for s in [c[6]]} == {1, 2, 3}
assert {c[6][1] % 16 for c in CELLS if c[7]["family"] == "plain_kp"} >= {0, 1, 15}
# row-multiplexed: rm_group_templates doubles nt while the LDS tile - min(h + 2R - 1, 64) + 6R rows (R = 16 / nt) of
# (16 + 4 nb + 1) 16 bytes - exceeds 72 KB = 73728 B.  One template, nt = 1, R = 16: min(h + 31, 64) + 96 rows.
#   3 blocks (464 B): h = 31: 158 rows = 73312 B fit; h = 32: 159 rows = 73776 B do not -> nt = 2
#   4 blocks (528 B): h = 12: 139 rows = 73392 B fit; h = 13: 140 rows = 73920 B do not -> nt = 2
#   70 x 250, n = 1: nt = 1: 160 rows = 84480 B; nt = 2 (R = 8): min(85, 64) + 48 = 112 rows = 59136 B -> nt = 2
#   70 x 250, n = 3: nt = 4 (R = 4): min(77, 64) + 24 = 88 rows = 46464 B -> nt = 4
# (w = 130: nseg = 9, packed K on the normalised methods; w = 192 and 250: nseg 12 and 16, not packed)
for _shape, _n, _nt, _kp in (((31, 130), 1, 1, 9), ((32, 130), 1, 2, 9), ((31, 192), 1, 1, 0), ((32, 192), 1, 2, 0),
                             ((12, 250), 1, 1, 0), ((13, 250), 1, 2, 0), ((70, 250), 1, 2, 0), ((70, 250), 3, 4, 0)):
    for _m in (5, 3):
        _cell("rm_doubling", _shape, _n, _m, nz=("rm_nt", "kp_nseg") if _kp else ("rm_nt",), rm_nt=_nt, rm_R=16 // _nt, kp_nseg=_kp)
# <= 16 templates off the row-multiplexed tiling: chans w h 65025 >= 2^32 (one channel: w h >= 66052; RGB: w h >= 22018)
for _n in (1, 5):
    for _m in (5, 3):
        _cell("few_plain", (259, 256), _n, _m)
for _m in (5, 3):
    _cell("few_rgb_rm", (148, 148), 3, _m, chans=3, nz=("rm_nt", "kp_nseg"), rm_nt=4, kp_nseg=10)     # 3 * 21904 * 65025 < 2^32
    _cell("few_plain", (149, 148), 3, _m, chans=3, nz=("kp_nseg",), kp_nseg=10)                       # 3 * 22052 * 65025 >= 2^32
    _cell("few_rgb_rm", (172, 128), 3, _m, chans=3, nz=("rm_nt",), rm_nt=4)                           # 22016
    _cell("few_plain", (173, 128), 3, _m, chans=3)                                                    # 22144
# the largest unslabbed area, chans w h = 130816 <= 131071: saturated operands over matching patches - an all-0 window
# against an all-0 template is 16384 w h = 2 143 289 344 in the int32 accumulator (2^31 - 1 = 2 147 483 647)
for _m in (5, 2, 0):
    for _k in ("zero", "sat"):
        _cell("largest_plain", (511, 256), 1, _m, kinds=(_k,))
_cell("largest_plain", (511, 256), 1, 5, kinds=("exact",))
_cell("largest_plain", (511, 256), 1, 3, kinds=("noisy",))
# slabs: by area (<= 16 templates: row-multiplexed raw launches, 512 x 128 or 512 x 64 slabs: one template per MFMA group) and
# by width (20 templates: a 256-wide slab and a ONE-column slab, plain raw launches)
for _m in (5, 3):
    _cell("slabs", (512, 256), 1, _m, nz=("n_slabs",), slab_nt=1)
    _cell("slabs", (20, 257), 20, _m, nz=("n_slabs",), n_slabs=2, slab_nt=0)
_cell("slabs", (512, 256), 1, 2, nz=("n_slabs",), slab_nt=1, kinds=("zero",))
# masked (disc mask), one channel, w h <= 66051: 258 x 256 = 66048 is in (row-multiplexed: n = 1; nt = 1 needs 160 rows of
# 528 B -> nt = 2), 259 x 256 is out: the float64 kernel (MTM_KERNEL_AUTO).  Packed K on methods 3 and 1 (w = 40: nseg 3),
# not at w = 64 / 128; 20 templates plain (a masked class has no two-row form), 3 row-multiplexed.
for _m in (3, 1):
    _cell("masked", (258, 256), 1, _m, masked=True, nz=("rm_nt",), rm_nt=2)
    _cell("masked_off_cores", (259, 256), 1, _m, masked=True, kernel=0)
    _cell("masked", (24, 40), 20, _m, masked=True, nz=("kp_nseg",), kp_nseg=3)
    _cell("masked", (24, 40), 3, _m, masked=True, nz=("rm_nt", "kp_nseg"), rm_nt=4, kp_nseg=3)
    _cell("masked", (24, 64), 20, _m, masked=True)
    _cell("masked", (9, 128), 3, _m, masked=True, nz=("rm_nt",), rm_nt=4)
# uint16 (MTM_KERNEL_MFMA16): packed K where ceil(w / 16) is no multiple of four.  The middle byte-plane correlations
# I_hi x T_lo + I_lo x T_hi share one int32 accumulator: 2 x 16384 w h where every byte is zero, which fits up to
# w h = 65535 (257 x 255) and not at 256 x 256.  This sweep found the limit at the uint8 path's 131071: 511 x 256 returned
# 0 over zero regions and 0.977 at an exact copy's own position.  Larger classes run the float64 kernel (MTM_KERNEL_AUTO).
for _m in (5, 3):
    for _shape, _kp in (((20, 49), 0), ((20, 64), 0), ((65, 33), 3), ((7, 250), 0), ((9, 81), 6)):
        _cell("u16", _shape, 20, _m, dtype="u16", kernel=4, nz=("kp_nseg",) if _kp else (), kp_nseg=_kp)
for _k in ("zero", "sat", "exact"):
    _cell("u16", (257, 255), 1, 5, dtype="u16", kernel=4, kinds=(_k,))
    _cell("u16_off_cores", (511, 256), 1, 5, dtype="u16", kernel=0, kinds=(_k,))
_cell("u16", (257, 255), 1, 3, dtype="u16", kernel=4, kinds=("zero",))
_cell("u16_off_cores", (256, 256), 1, 5, dtype="u16", kernel=0, kinds=("zero",))

_NAMES = [c[0] for c in CELLS]
assert len(set(_NAMES)) == len(_NAMES)
_CONFIRMED = {}          # cell name -> the record its tiling assertion passed on


# ---- a cell's scene --------------------------------------------------------------------------------------------------------
_KINDS_FEW = ("exact", "noisy", "tail", "const", "zero", "sat")


def _kinds(n, kinds):
    if kinds:
        assert len(kinds) == n
        return list(kinds)
    if n < 8:
        return list(_KINDS_FEW[:n])
    return ["exact", "noisy", "tail", "const", "zero", "sat"] + ["noisy" if i % 3 == 1 else "exact" for i in range(6, n)]


def _disc(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((yy - h / 2 + 0.5) / (h / 2)) ** 2 + ((xx - w / 2 + 0.5) / (w / 2)) ** 2) <= 1.0).astype(np.uint8) * 255


def _scene(name, dtype, chans, masked, n, shape, kinds):
    """The image and the templates of a cell.  Map size by the oracle's cost (taps x outputs): 45 x 269 (the last
    256-column segment holds 13 outputs; six 8-row blocks, the last with 5 rows), 13 x 263, or 9 x 41 for the largest."""
    h, w = shape
    taps = chans * h * w * (2 if masked else 1)
    oh, ow = (45, 269) if taps <= 9000 else (13, 263) if taps <= 40000 else (9, 41)
    H, W = h + oh - 1, w + ow - 1
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    top = 65535 if dtype == "u16" else 255
    npdt = np.uint16 if dtype == "u16" else np.uint8
    full = (H, W) + ((chans,) if chans > 1 else ())
    img = (rng.integers(0, top + 1, full) * (rng.random(full) < 0.35)).astype(npdt)
    kinds = _kinds(n, kinds)
    # the saturated patches, template-sized, each with one pixel of the other extreme at its centre
    spots = {"zero": (min(1, oh - 1), 2), "sat": (min(3, oh - 1), W - w - 1)}
    if "zero" in kinds and "sat" in kinds:
        assert spots["zero"][1] + w <= spots["sat"][1], (name, "the two patches overlap")
    for kind, (y, x) in spots.items():
        if kind in kinds:
            img[y:y + h, x:x + w] = 0 if kind == "zero" else top
            img[y + h // 2, x + w // 2] = top if kind == "zero" else 0
    units = []
    for kind in kinds:
        y, x = int(rng.integers(0, oh)), int(rng.integers(0, ow))
        if kind in spots:
            y, x = spots[kind]
        t = img[y:y + h, x:x + w].astype(np.int64)
        if kind == "noisy":
            t = t + rng.integers(-30 * (top // 255), 30 * (top // 255) + 1, t.shape)
        elif kind == "tail":
            t[: (2 * h) // 3] = (top + 1) // 2                 # structure only in the last third of the rows
        elif kind == "const":
            t[:] = 77 * (top // 255)
        units.append(np.ascontiguousarray(np.clip(t, 0, top).astype(npdt)))
    mask = _disc(h, w) if masked else None
    return img, [(t, mask) for t in units], kinds, (oh, ow)


def _picks(n, kinds):
    """First and last template, one in the last (partly filled) 16-template group, every special one."""
    out = {0, n - 1, 16 * ((n - 1) // 16), min(n - 1, 16 * ((n - 1) // 16) + 1)}
    out |= {i for i, k in enumerate(kinds[:6]) if k in ("tail", "const", "zero", "sat", "noisy")}
    return sorted(out)


def _reference(img, t, mask, method, dtype):
    if dtype == "u16":
        # (through float32, as the reference package turns uint16 into: sums of integer-valued float64 products below 2^53
        # are exact - test_uint16_whole_maps_on_partly_filled_last_segments)
        return O.match_template(img.astype(np.float32), t.astype(np.float32), method, corr="direct")
    return O.match_template(img, t, method, mask=mask, corr="direct")


def _check_tiling(ctx, name, masked, n, shape, exp):
    recs = ctx.class_tilings()
    assert len(recs) == 1, recs
    r = recs[0]
    assert (r["h"], r["w"], r["n_templates"]) == (shape[0], shape[1], n), r
    assert r["kernel"] == exp["kernel"], (name, r)
    if exp["kernel"] in (3, 4):
        assert frozenset(f for f in _NZ_FIELDS if r[f]) == exp["nz"], (name, sorted(exp["nz"]), r)
    for f, v in exp.items():
        if f not in ("family", "kernel", "nz", "kinds"):
            assert r[f] == v, (name, f, v, r)
    return r


@pytest.mark.parametrize("cell", CELLS, ids=_NAMES)
def test_tiling_cell(lib, cell):
    name, dtype, chans, method, masked, n, shape, exp = cell
    img, units, kinds, (oh, ow) = _scene(name, dtype, chans, masked, n, shape, exp["kinds"])
    normed = method in (1, 3, 5)
    lower = method in (0, 1)                                   # the squared differences: hits are minima below the threshold
    thr0 = 0.5 if normed else (-1.0 if method == 0 else 1e30)  # raw sums: nothing listed (their maps are what is checked)
    picks = _picks(n, kinds)
    refs = {i: _reference(img, units[i][0], units[i][1], method, dtype) for i in picks}
    ctx = lib.Context(0)
    try:
        ctx.set_option(lib.OPT_HITS_ONLY, 0)
        best = {}
        for exact, pattern in ((1, 0xFF), (1, 0x7F), (0, 0xFF)):
            ctx.set_option(lib.OPT_EXACT_DIV, exact)
            ctx.debug_poison(pattern, 7)
            ctx.search(units, img, method, lib.PEAKS_LOCAL, thr0)
            if default_routes() and name not in _CONFIRMED:
                _CONFIRMED[name] = _check_tiling(ctx, name, masked, n, shape, exp)
            for i in picks:
                got, ref = ctx.last_score_map(i, (oh, ow)), refs[i]
                both_nan = np.isnan(got) & np.isnan(ref)
                if exact and not masked:
                    same = (got == ref) | both_nan
                else:
                    with np.errstate(invalid="ignore"):
                        same = (np.abs(got.astype(np.float64) - ref) <= 1e-6 * np.maximum(1.0, np.abs(ref))) | both_nan | (got == ref)
                bad = np.argwhere(~same)
                assert len(bad) == 0, "%s exact_div %d pattern %#x template %d (%s): %d wrong pixels, columns %s rows %s, first %r / %r" % (
                    name, exact, pattern, i, kinds[i], len(bad), sorted(set(bad[:, 1].tolist()))[:12],
                    sorted(set(bad[:, 0].tolist()))[:6], got[tuple(bad[0])], ref[tuple(bad[0])])
            if exact and pattern == 0xFF and normed:
                for i in range(n):
                    m = ctx.last_score_map(i, (oh, ow))
                    best[i] = float(np.nanmin(m) if lower else np.nanmax(m))
        if not normed:
            return
        # hits-only against map mode (just checked against exact sums), IEEE division, records byte for byte
        ctx.set_option(lib.OPT_EXACT_DIV, 1)
        live = [i for i, k in enumerate(kinds) if k != "const"]
        thr_all = max(best[i] for i in live) + 4e-4 if lower else min(best[i] for i in live) - 4e-4
        thrs = [thr_all]
        screened = "tail_ok" in exp["nz"]
        if screened:
            thrs += [0.5, 0.7, best[kinds.index("tail")] - 4e-4]
        for thr in thrs:
            ctx.set_option(lib.OPT_HITS_ONLY, 0)
            ref = ctx.search(units, img, method, lib.PEAKS_LOCAL, thr).copy()
            ctx.set_option(lib.OPT_HITS_ONLY, 1)
            for pattern in (0xFF, 0x7F):
                ctx.debug_poison(pattern, 7)
                got = ctx.search(units, img, method, lib.PEAKS_LOCAL, thr).copy()
                assert got.tobytes() == ref.tobytes(), (name, thr, pattern, len(got), len(ref))
            if thr == thr_all:
                assert set(ref["templ_idx"].tolist()) >= set(live), (name, thr, sorted(set(live) - set(ref["templ_idx"].tolist())))
            if screened and thr == 0.7 and default_routes():
                r = ctx.class_tilings()[0]
                assert r["tail_ok"] and r["tail_split"] >= 6, (name, r)      # the call at 0.7 did carry a split
    finally:
        ctx.close()


def test_the_table_covers_every_tiling():
    """A table edit cannot silently drop a family: the expectations of the table (each asserted against class_tilings() by
    its own case above) cover every tiling the sweep is there for, and every case that ran on the default routes in this
    session did pass its tiling assertion."""
    fam = {}
    for name, dtype, chans, method, masked, n, (h, w), exp in CELLS:
        fam.setdefault(exp["family"], []).append((dtype, chans, method, masked, n, h, w, exp))
    nz = lambda *f: frozenset(f)                                                                            # noqa: E731
    have = lambda family, pred: any(pred(*c) for c in fam.get(family, []))                                  # noqa: E731
    # two-row with the screen: a partly padded last segment (w < 64) and a full one, the extremes of h, both group counts
    for pred in (lambda d, c, m, k, n, h, w, e: w < 64, lambda d, c, m, k, n, h, w, e: w == 64, lambda d, c, m, k, n, h, w, e: h == 8,
                 lambda d, c, m, k, n, h, w, e: h == 71, lambda d, c, m, k, n, h, w, e: n == 20, lambda d, c, m, k, n, h, w, e: n == 33,
                 lambda d, c, m, k, n, h, w, e: m == 3, lambda d, c, m, k, n, h, w, e: m == 5):
        assert have("r2_screen", lambda *c: c[7]["nz"] == nz("r2", "tail_ok") and pred(*c))
    for pred in (lambda h: h == 7, lambda h: h == 72, lambda h: h > 72):
        assert have("r2_noscreen", lambda *c: c[7]["nz"] == nz("r2") and pred(c[5]))
    assert {c[2] for c in fam["r2_raw"]} == {2, 4} and all("r2" in c[7]["nz"] for c in fam["r2_raw"])
    assert have("r2_raw", lambda *c: c[5] + 1 > 72) and have("r2_raw", lambda *c: c[6] < 16) and have("r2_raw", lambda *c: c[6] == 64)
    assert {(c[6] + 63) // 64 for c in fam["plain"] if c[7]["nz"] == nz()} == {1, 2, 3, 4}
    assert have("plain", lambda *c: c[5] > 64) and have("plain", lambda *c: c[2] == 0)
    assert {c[7]["kp_nseg"] for c in fam["plain_kp"] if c[7]["nz"] == nz("kp_nseg")} >= {1, 6, 7, 10, 11, 13, 14, 15}
    assert have("plain_kp", lambda *c: c[5] > 64)
    assert {(c[4], c[5], c[6], c[7]["rm_nt"]) for c in fam["rm_doubling"]} >= {
        (1, 31, 130, 1), (1, 32, 130, 2), (1, 12, 250, 1), (1, 13, 250, 2), (1, 70, 250, 2), (3, 70, 250, 4)}
    assert have("rm_doubling", lambda *c: c[7]["kp_nseg"] > 0) and have("rm_doubling", lambda *c: c[7]["kp_nseg"] == 0)
    assert have("few_plain", lambda *c: c[1] == 1 and c[4] == 1 and c[7]["nz"] == nz())
    assert have("few_plain", lambda *c: c[1] == 1 and c[4] == 5 and c[7]["nz"] == nz())
    assert have("few_plain", lambda *c: c[1] == 3 and "rm_nt" not in c[7]["nz"]) and have("few_rgb_rm", lambda *c: c[1] == 3 and "rm_nt" in c[7]["nz"])
    assert {(c[2], c[7]["kinds"]) for c in fam["largest_plain"]} >= {(m, (k,)) for m in (5, 2, 0) for k in ("zero", "sat")}
    assert all(c[5] * c[6] == 130816 and c[7]["nz"] == nz() for c in fam["largest_plain"])
    assert have("slabs", lambda *c: c[6] > 256 and c[7]["nz"] == nz("n_slabs")) and have("slabs", lambda *c: c[5] * c[6] > 131071 and c[6] <= 256)
    assert {c[2] for c in fam["masked"]} == {3, 1} and all(c[3] for c in fam["masked"] + fam["masked_off_cores"])
    assert have("masked", lambda *c: c[5] * c[6] == 66048 and c[7]["kernel"] == 3) and have("masked_off_cores", lambda *c: c[5] * c[6] == 66304 and c[7]["kernel"] == 0)
    assert have("masked", lambda *c: c[7]["nz"] == nz("kp_nseg") and c[4] == 20) and have("masked", lambda *c: c[7]["nz"] == nz() and c[4] == 20)
    assert have("masked", lambda *c: "rm_nt" in c[7]["nz"] and c[4] == 3)
    assert all(c[0] == "u16" and c[7]["kernel"] == 4 for c in fam["u16"])
    assert have("u16", lambda *c: c[7]["nz"] == nz("kp_nseg")) and have("u16", lambda *c: c[7]["nz"] == nz() and c[4] == 20)
    assert {c[7]["kinds"] for c in fam["u16"] if c[5] * c[6] == 65535} >= {("zero",), ("sat",), ("exact",)}
    assert all(c[0] == "u16" and c[7]["kernel"] == 0 for c in fam["u16_off_cores"])
    assert have("u16_off_cores", lambda *c: c[5] * c[6] == 65536) and have("u16_off_cores", lambda *c: c[5] * c[6] == 130816)
    # what ran in this session was confirmed (a case that fails its tiling assertion never gets here)
    for name, rec in _CONFIRMED.items():
        assert rec["n_templates"] >= 1, (name, rec)
