"""
The float64, dot4 and naive score kernels (csrc/mtm_k_score.hip.h) at their geometry edges, against exact sums (-m gpu).

Half of the suite takes these three kernels as its standard of truth: every float32 route must reproduce the float64 kernel's
records bit for bit, the peak-entry and hits-only tests compare with the dot4 kernel, test_dot4_variants_agree compares
everything with the naive kernel.  A tap dropped or counted twice for one residue of a width, a height or a list length in one
of them would be inherited by both sides of those comparisons.  This is a table of cells at the edges of their rules -

  ncc_f64_kernel<MASKED>   16 x 32 template chunks (the guard dx4 + s < cw of the last float4 of a chunk: cw % 4 = 0 .. 3),
                           128 x 8 output tiles of four outputs per thread, the accumulator hand-over between channels;
  ncc_dot4_kernel          64 x 64 chunks over w4 = round_up(w, 4), the pad rows of the PY-row blocking, the NT list tail
                           that repeats its last entry, the XCD work mapping (n_work no multiple of 8), the LDS transpose of
                           the epilogue, uint64 totals from chans w h 65025 >= 2^32 on, the MASKSQ instantiation (sum I^2 M);
  ncc_naive_kernel         the base of test_dot4_variants_agree

- and every cell compares WHOLE maps, every output, BIT FOR BIT (NaN meets NaN: the 0 / 0 of OpenCV's matchTemplateMask) with
mtm_oracle.match_template(..., corr="direct"): plain sliding sums, OpenCV's epilogue order, nothing of the code under test.

Why bit for bit holds: the data is exact.  Pixels are uint8, uint16 (through float32, as the reference package casts them),
or float32 values that are integers (`f32i`, 0 .. 4095) or quarters (`f32q`); masks are binary or weights k / 8 (uint16
masks, which the library reads as weights as the reference does: integers 0 .. 4).  Every product and every partial sum is
then a dyadic number below 2^53: the kernels' FMA chains, numpy's sums and Python's integers give the same float64, and the
epilogues - the same operations in the same order (mtm_device_util.hip.h, mtm_templ_stats.h) - the same float32.
tests/test_exact_kernels_cpu.py proves the precondition for every scene of the table, and that corr="direct" is a plain
triple loop's result.

ONE exception, the `general` family: float32 pixels normal(100, 40) clipped to positive values, float weight masks from
rng.random, TM_CCORR and TM_CCORR_NORMED only (no term cancels).  Both chains carry a relative error of at most N 2^-53
(N <= 2145 taps here: 2.4e-13), far below 2^-24: got is float32(ref) or its float32 neighbour.  The CPU companion shows the
oracle in float64 and in np.longdouble agreeing to better than 2^-40 relative on these scenes.

Scenes: noise with a tenth of the pixels zero (DENSITY) and the template kinds of test_gpu_tilings.py, exact / noisy / const /
zero / sat, with its saturated image patches where the map has room for them; masked cells carry `mzero` (a template that is
zero wherever its mask is not: templ2_mask2_sum = 0) and, with the same proviso, an image patch that is zero under the mask
(sum I^2 M = 0 there).  Masks are random with their border rows and columns set: a mask that happened to zero the last tap of a
row would hide a kernel that drops it.  Honest scenes (checked on the CPU from the
reference alone): of the normalised maps of the exact / noisy / sat templates at least half the outputs are finite and not
0, 1 or -1 - but for maps of fewer than 16 outputs, which carry noisy templates only and are required to hold one such
output at least, and 1 x 1 templates, whose normalised scores are 0 or 1 by arithmetic.  Most cells have sums beyond 2^24.

Every cell asserts the route it entered - Context.class_tilings()[0]["kernel"], timing()["kernel_used"] (0 float64, 1 naive,
2 dot4), the dot4 variant its launch took (class_tilings()[0]["dot_variant"], 7 = uint64 totals), for MASKSQ that the masked
class ran on the matrix cores without their sum I^2 M pass (sq_launches = 0: launch_masked_sumsq then takes the dot4 pass) -
unless a switch of tools/alt_modes.sh is set; the results are asserted always.  Every cell runs through the batched launch
(a map-mode search, last_score_map) and the single-template launch (score_map), from memory poisoned with 0xFF and with 0x7F,
in a context of its own.
"""
import zlib

import numpy as np
import pytest

import mtm_oracle as O
from test_gpu_tilings import default_routes

pytestmark = pytest.mark.gpu

# mirrored from csrc/mtm_score_params.h and kDotVariants of csrc/mtm_launch.hip (test_exact_kernels_cpu.py parses both)
F64_CHUNK_H, F64_CHUNK_W, F64_BX, F64_BY = 16, 32, 128, 8
DOT_CHUNK = 64
DOT_VARIANTS = ((4, 4, 4), (4, 4, 2), (8, 2, 4), (8, 4, 2), (4, 2, 4), (8, 2, 2), (4, 2, 8), (4, 2, 2))   # (PX, PY, NT); 7: wide
DOT_WIDE = 7
MASKSQ_VARIANT = (4, 4, 1)
K_MAX_CHANS = 4
KERNEL_F64, KERNEL_NAIVE, KERNEL_DOT4, KERNEL_MFMA = 0, 1, 2, 3

DEFAULT_MAP = (9, 133)          # a second 128-column tile of five outputs, a second 8-row tile of one row
DOT_MAP = (33, 133)             # ... of the dot4 tiles of 128 columns and 16 or 32 rows
DOT_MAP_WIDE = (33, 257)        # ... and of the 256-column tiles (PX = 8)
ALL, MASKED_METHODS = (0, 1, 2, 3, 4, 5), (0, 1, 2, 3)
TOP = {"u8": 255, "u16": 65535, "f32i": 4095, "f32q": 4095, "gen": None}
# Nine pixels of ten are non-zero.  (test_gpu_tilings.py keeps a third, for its K-loop screens; here TM_SQDIFF_NORMED must
# stay below its saturation at 1 between unrelated windows: 2 (1 - 0.75 p) < 1 needs a density p above 2 / 3.)
DENSITY = 0.9


def is_wide(chans, h, w):
    return chans * w * h * 65025 >= 2 ** 32


# ---- the table -----------------------------------------------------------------------------------------------------------
CELLS = []
_ROT = ("const", "zero", "sat")


def _cell(family, kernel, h, w, out=DEFAULT_MAP, n=3, dtype="f32i", chans=1, methods=ALL, mask=None, variant=None, kinds=None,
          env=(), tag=""):
    """kernel: "f64" | "dot4" | "naive" | "masksq".  kinds None: by n and the map size (see _kinds)."""
    if mask:
        methods = tuple(m for m in methods if m in MASKED_METHODS)
    name = "%s-%s%s-%dx%d-o%dx%d-n%d" % (family, dtype, "c%d" % chans if chans > 1 else "", h, w, out[0], out[1], n)
    name += ("-" + mask if mask else "") + ("-v%d" % variant if variant is not None else "") + ("-" + tag if tag else "")
    CELLS.append(dict(name=name, family=family, kernel=kernel, h=h, w=w, out=tuple(out), n=n, dtype=dtype, chans=chans,
                      methods=tuple(methods), mask=mask, variant=variant, kinds=kinds, env=tuple(env), rot=len(CELLS)))


F64_WIDTHS = (1, 2, 3, 4, 5, 31, 32, 33, 34, 35, 36, 37, 63, 64, 65, 97)      # (34: cw % 4 = 2 in a chunk behind a full one)
F64_HEIGHTS = (1, 15, 16, 17, 31, 32, 33, 49)
F64_OWS, F64_OHS = (1, 2, 3, 4, 5, 127, 128, 129, 130, 257), (1, 7, 8, 9, 17)       # (2, 130: ow % 4 = 2)
# ncc_f64_kernel<false> and <true>: template widths on both sides of every chunk and float4 boundary, heights likewise
for _i, _w in enumerate(F64_WIDTHS):
    _cell("f64_w", "f64", 5, _w, dtype=("f32i", "f32q")[_i % 2])
    _cell("f64_w", "f64", 5, _w, dtype=("f32q", "f32i")[_i % 2], mask=("wt", "bin")[_i % 2])
for _i, _h in enumerate(F64_HEIGHTS):
    _cell("f64_h", "f64", _h, 33, dtype=("f32q", "f32i")[_i % 2])
    _cell("f64_h", "f64", _h, 33, dtype=("f32i", "f32q")[_i % 2], mask=("wt", "bin")[_i % 2])
# output geometry at a small template: one-column and one-row maps, last tiles of one column or one row, ow % 4 = 0 .. 3
for _i, _ow in enumerate(F64_OWS):
    _cell("f64_out", "f64", 5, 33, out=(9, _ow), n=(1, 3)[_i % 2])
    _cell("f64_out", "f64", 5, 33, out=(9, _ow), n=(3, 1)[_i % 2], mask=("wt", "bin")[_i % 2])
for _i, _oh in enumerate(F64_OHS):
    _cell("f64_out", "f64", 5, 33, out=(_oh, 133), n=(3, 1)[_i % 2])
    _cell("f64_out", "f64", 5, 33, out=(_oh, 133), n=(1, 3)[_i % 2], mask=("bin", "wt")[_i % 2])
_cell("f64_out", "f64", 5, 33, out=(1, 1), n=1)
_cell("f64_out", "f64", 5, 33, out=(1, 1), n=3, mask="bin")
# channels 1 .. kMaxChans: the accumulators are handed over per channel; 17 x 35: two row chunks and two column chunks each
for _c in (2, 3, K_MAX_CHANS):
    _cell("f64_chans", "f64", 5, 33, chans=_c, dtype="f32q", n=1)
    _cell("f64_chans", "f64", 17, 35, chans=_c)
    _cell("f64_chans", "f64", 17, 35, chans=_c, mask=("wt", "bin")[_c % 2], n=1)
# the other classes whose production route this kernel is: uint16 RGB (mfma16_class_ok wants one channel), uint16 with masks,
# uint8 RGB with a mask, masked uint8 beyond 66051 pixels
for _shape in ((5, 33), (17, 37), (16, 64)):
    _cell("f64_u16rgb", "f64", _shape[0], _shape[1], dtype="u16", chans=3, methods=(3, 5))
for _shape, _mk in (((5, 33), "bin"), ((17, 36), "wt"), ((33, 5), "wt")):
    _cell("f64_u16mask", "f64", _shape[0], _shape[1], dtype="u16", mask=_mk)
for _shape in ((5, 33), (16, 32), (17, 65)):
    _cell("f64_u8rgbmask", "f64", _shape[0], _shape[1], dtype="u8", chans=3, mask="bin")
_cell("f64_u8large", "f64", 259, 256, dtype="u8", mask="bin", n=1, kinds=("exact",), methods=(3, 1))
# the `general` family: inexact data, TM_CCORR and TM_CCORR_NORMED, float32(ref) or its neighbour
for _shape, _c, _mk in (((5, 33), 1, None), ((17, 37), 1, None), ((33, 65), 1, None), ((5, 35), 3, None),
                        ((5, 33), 1, "wt"), ((17, 37), 1, "wt"), ((33, 65), 1, "wt")):
    _cell("general", "f64", _shape[0], _shape[1], dtype="gen", chans=_c, mask=_mk, methods=(2, 3), kinds=("exact", "noisy", "noisy"))

# ncc_dot4_kernel: every variant on a map that crosses all their tile edges (BX 128 | 256, BY 16 | 32), on one inside a
# tile, on a 1 x 1 map
for _v in range(7):
    _cell("dot_variants", "dot4", 9, 40, out=(33, 257), n=5, dtype="u8", variant=_v)
    _cell("dot_variants", "dot4", 9, 40, out=(7, 29), n=2, dtype="u8", variant=_v)
    _cell("dot_variants", "dot4", 9, 40, out=(1, 1), n=2, dtype="u8", variant=_v)
# chunk edges (64 x 64 over w4) at variant 0 and at a PX = 8 variant (3: PY = 4 as well)
DOT_WIDTHS = (1, 3, 4, 5, 61, 63, 64, 65, 68, 69, 127, 128, 129)
DOT_HEIGHTS = (1, 63, 64, 65, 127, 128, 129)
for _v, _map in ((0, DOT_MAP), (3, DOT_MAP_WIDE)):
    for _w in DOT_WIDTHS:
        _cell("dot_chunks", "dot4", 40, _w, out=_map, n=2, dtype="u8", variant=_v)
    for _h in DOT_HEIGHTS:
        _cell("dot_chunks", "dot4", _h, 40, out=_map, n=2, dtype="u8", variant=_v)
# list tails: n = 1, NT - 1, NT, NT + 1, 2 NT + 1 (every template's map is compared: a repeated last entry must not leak)
for _v in (1, 0, 6):
    _nt = DOT_VARIANTS[_v][2]
    for _n in sorted({1, _nt - 1, _nt, _nt + 1, 2 * _nt + 1}):
        _cell("dot_tails", "dot4", 24, 40, n=_n, dtype="u8", variant=_v, methods=(5, 3, 0))
# work counts (ntx nty nchunks; the grid is rounded up to 8): 1, 7 (26 templates on one tile), 9 (3 tiles x 3 chunks), 66
_cell("dot_work", "dot4", 9, 40, out=(5, 9), n=3, dtype="u8", variant=0, methods=(5, 1), tag="work1")
_cell("dot_work", "dot4", 9, 40, out=(5, 9), n=26, dtype="u8", variant=0, methods=(5, 1), tag="work7")
_cell("dot_work", "dot4", 9, 40, out=(9, 257), n=9, dtype="u8", variant=0, methods=(5, 1), tag="work9")
_cell("dot_work", "dot4", 9, 40, out=(33, 257), n=41, dtype="u8", variant=0, methods=(3, 0), tag="work66")
# RGB at chunk-edge shapes
_cell("dot_rgb", "dot4", 9, 65, out=DOT_MAP, n=3, dtype="u8", chans=3, variant=0)
_cell("dot_rgb", "dot4", 65, 9, out=DOT_MAP_WIDE, n=3, dtype="u8", chans=3, variant=3)
# the uint32 limit chans w h 65025 >= 2^32: 66049 and 3 x 21904 are not wide, 66304 and 3 x 22052 are; all 255 against all 255
for _shape, _c in (((257, 257), 1), ((259, 256), 1), ((148, 148), 3), ((149, 148), 3)):
    _cell("dot_limit", "dot4", _shape[0], _shape[1], out=(17, 129), n=3, dtype="u8", chans=_c, variant=0,
          kinds=("sat", "zero", "exact"), methods=(5, 3, 2))
# MASKSQ, ncc_dot4_kernel<4, 4, 1, false, true>: the sum I^2 M pass of masked uint8 classes on the matrix cores without the
# row-multiplexed tiling or without the fused statistics
for _env in (("MTM_ROW_MUX", "0"), ("MTM_FUSE_STATS", "0")):
    for _shape in ((9, 5), (9, 40), (9, 64), (9, 65), (64, 40), (65, 40), (65, 65)):
        _cell("masksq", "masksq", _shape[0], _shape[1], out=DOT_MAP, dtype="u8", mask="bin", methods=(3, 1), env=(_env,),
              tag=_env[0][4:].lower())
    _cell("masksq", "masksq", 258, 256, out=(9, 41), n=1, kinds=("exact",), dtype="u8", mask="bin", methods=(3, 1), env=(_env,),
          tag=_env[0][4:].lower())

# ncc_naive_kernel on a cross-section
for _shape in ((5, 33), (17, 65), (1, 1)):
    _cell("naive", "naive", _shape[0], _shape[1], dtype="u8")
    _cell("naive", "naive", _shape[0], _shape[1], dtype="u8", chans=3)
    _cell("naive", "naive", _shape[0], _shape[1], dtype="u16")
    _cell("naive", "naive", _shape[0], _shape[1], dtype="f32q")
    _cell("naive", "naive", _shape[0], _shape[1], dtype="f32q", mask="wt")

_NAMES = [c["name"] for c in CELLS]
assert len(set(_NAMES)) == len(_NAMES)


# ---- a cell's scene --------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def _kinds(cell):
    n, (oh, ow) = cell["n"], cell["out"]
    if cell["kinds"]:
        assert len(cell["kinds"]) == n
        return list(cell["kinds"])
    if oh * ow < 16:                                    # a map too small for "half of it": noisy templates only
        return ["noisy"] * n
    special = "mzero" if cell["mask"] else _ROT[cell["rot"] % 3]
    base = ["noisy"] if n == 1 else ["exact", "noisy", special, "const", "zero", "sat"][:n]
    return base + ["noisy" if i % 3 == 1 else "exact" for i in range(len(base), n)]


def _npdt(dtype):
    return {"u8": np.uint8, "u16": np.uint16}.get(dtype, np.float32)


def _mask(cell, rng):
    h, w, chans, dtype = cell["h"], cell["w"], cell["chans"], cell["dtype"]
    shape = (h, w) + ((chans,) if chans > 1 else ())
    if dtype == "gen":
        return rng.random(shape).astype(np.float32)
    if cell["mask"] == "bin":
        m = (rng.random(shape) < 0.7).astype(np.int64)
        one = 1
    else:
        m = rng.integers(0, 5 if dtype == "u16" else 9, shape)
        one = int(m.max()) or 1
    m[0], m[-1], m[:, 0], m[:, -1] = one, one, one, one     # the border taps count
    if dtype == "u8":
        return (m * 255).astype(np.uint8)
    if dtype == "u16":
        return m.astype(np.uint16)
    return (m / (1.0 if cell["mask"] == "bin" else 8.0)).astype(np.float32)


def scene(cell):
    """-> image, [(template, mask or None)], kinds.  Everything is drawn from the cell's name."""
    h, w, chans, dtype, (oh, ow) = cell["h"], cell["w"], cell["chans"], cell["dtype"], cell["out"]
    H, W = h + oh - 1, w + ow - 1
    rng = _rng(cell["name"])
    full = (H, W) + ((chans,) if chans > 1 else ())
    kinds = _kinds(cell)
    mask = _mask(cell, rng) if cell["mask"] else None
    if dtype == "gen":
        img = np.maximum(rng.normal(100.0, 40.0, full), 1.0).astype(np.float32)
        units = []
        for kind in kinds:
            y, x = int(rng.integers(0, oh)), int(rng.integers(0, ow))
            t = np.array(img[y:y + h, x:x + w], np.float32)
            if kind == "noisy":
                t = np.maximum(t + rng.normal(0.0, 10.0, t.shape), 1.0).astype(np.float32)
            units.append((np.ascontiguousarray(t), mask))
        return img, units, kinds
    top, q = TOP[dtype], (4 if dtype == "f32q" else 1)
    unit = top // 255
    img = rng.integers((top // 4) * q, (top + 1) * q, full) * (rng.random(full) < DENSITY)    # in units of 1 / q
    spots = {"zero": (min(1, oh - 1), min(2, ow - 1)), "sat": (min(3, oh - 1), max(ow - 2, 0))}
    # The patches go in where the map leaves columns between them for templates cut from plain noise (a template cut across a
    # patch is unlike every other window, and TM_SQDIFF_NORMED saturates), or where the cell names its kinds itself.
    lo, hi = spots["zero"][1] + w, spots["sat"][1] - w
    room = lo <= hi
    patches = [k for k in ("sat", "zero") if k in kinds and (room or cell["kinds"])]
    if len(patches) == 2 and not room:
        patches = ["sat"]                                                               # (they would overlap)
    for kind in patches:
        y, x = spots[kind]
        img[y:y + h, x:x + w] = 0 if kind == "zero" else top * q
        img[y + h // 2, x + w // 2] = top * q if kind == "zero" else 0
    if mask is not None and (room or cell["kinds"]):       # a region that is zero under the mask: sum I^2 M = 0
        y, x = spots["zero"]
        img[y:y + h, x:x + w][mask > 0] = 0
    temps = []
    for kind in kinds:
        y, x = int(rng.integers(0, oh)), int(rng.integers(lo, hi + 1) if room else rng.integers(0, ow))
        t = img[y:y + h, x:x + w].copy()
        if kind == "noisy":
            t = t + rng.integers(-30 * unit * q, 30 * unit * q + 1, t.shape)
        elif kind == "const":
            t[:] = 77 * unit * q
        elif kind in ("zero", "sat"):                      # constructed, whether or not the image carries the patch
            t[:] = 0 if kind == "zero" else top * q
            t[h // 2, w // 2] = top * q if kind == "zero" else 0
        elif kind == "mzero":
            t = t + rng.integers(0, 30 * unit * q + 1, t.shape)
            t[mask > 0] = 0
        temps.append(np.clip(t, 0, top * q))
    conv = (lambda a: np.ascontiguousarray((a / float(q)).astype(np.float32))) if dtype in ("f32i", "f32q") else \
           (lambda a: np.ascontiguousarray(a.astype(_npdt(dtype))))
    return conv(img), [(conv(t), mask) for t in temps], kinds


def oracle_inputs(cell, img, t, mask):
    """What mtm_oracle.match_template takes for a unit: uint16 through float32 (as the reference package turns it into; a
    uint16 mask is then a float32 weight image), everything else as it is."""
    if cell["dtype"] == "u16":
        return img.astype(np.float32), t.astype(np.float32), None if mask is None else mask.astype(np.float32)
    return img, t, mask


def reference_maps(cell, img, units):
    """{method: [O.match_template(..., corr="direct") per template]}, computed once per cell.  The sliding sums of a template
    (one pass per channel; masked: two) serve every method's epilogue."""
    real, memo, who = O.sliding_corr, {}, [0]

    def once(img2d, ker2d, exact_int=False, force=None, cache=None, cache_key=None):
        key = (who[0], cache_key)
        if key not in memo:
            memo[key] = real(img2d, ker2d, exact_int=exact_int, force=force)
        return memo[key]
    O.sliding_corr = once
    try:
        out = {m: [] for m in cell["methods"]}
        for i, (t, mask) in enumerate(units):
            who[0] = i
            a, b, mk = oracle_inputs(cell, img, t, mask)
            for m in cell["methods"]:
                ref = np.ascontiguousarray(O.match_template(a, b, m, mask=mk, corr="direct"), dtype=np.float32)
                assert ref.shape == cell["out"]
                ref.setflags(write=False)
                out[m].append(ref)
        return out
    finally:
        O.sliding_corr = real


_DATA = {}


def cell_data(cell):
    """(image, units, kinds, reference maps) of a cell, made once per session and left unchanged."""
    if cell["name"] not in _DATA:
        img, units, kinds = scene(cell)
        _DATA[cell["name"]] = (img, units, kinds, reference_maps(cell, img, units))
    return _DATA[cell["name"]]


def same_bits(cell, got, ref):
    """Per output: the same float32 (`general`: or its neighbour), NaN with NaN."""
    g, r = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(ref).view(np.uint32)
    both_nan = np.isnan(got) & np.isnan(ref)
    if cell["dtype"] == "gen":
        return (np.abs(g.astype(np.int64) - r.astype(np.int64)) <= 1) | both_nan
    return (g == r) | both_nan


def expected_route(cell):
    """(class kernel, timing kernel_used, dot_variant)"""
    k = cell["kernel"]
    if k == "f64":
        return KERNEL_F64, KERNEL_F64, -1
    if k == "naive":
        return KERNEL_NAIVE, KERNEL_NAIVE, -1
    if k == "masksq":
        return KERNEL_MFMA, KERNEL_MFMA, -1
    return KERNEL_DOT4, KERNEL_DOT4, DOT_WIDE if is_wide(cell["chans"], cell["h"], cell["w"]) else cell["variant"]


# ---- the GPU side --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import build as mtm_build
    mtm_build.build()
    from MTM import _lib
    assert _lib.load().mtm_device_count() >= 1
    return _lib


_RAN = {}


def _check_route(ctx, cell):
    recs = ctx.class_tilings()
    assert len(recs) == 1, (cell["name"], recs)
    r, tm = recs[0], ctx.timing()
    kernel, used, variant = expected_route(cell)
    assert (r["h"], r["w"], r["n_templates"]) == (cell["h"], cell["w"], cell["n"]), (cell["name"], r)
    assert (r["kernel"], tm["kernel_used"], r["dot_variant"]) == (kernel, used, variant), (cell["name"], r, tm)
    if cell["kernel"] == "masksq":
        assert tm["sq_launches"] == 0, (cell["name"], tm)          # no sum I^2 M pass on the matrix cores: the dot4 pass ran


def _compare(cell, what, kind, method, got, ref):
    if kind == "const" and method == 5 and not cell["mask"]:
        assert np.array_equal(got, np.ones_like(got)), (cell["name"], what, "a constant template under TM_CCOEFF_NORMED is 1")
    bad = np.argwhere(~same_bits(cell, got, ref))
    assert len(bad) == 0, "%s %s (%s, method %d): %d of %d outputs differ, columns %s rows %s, first %r / %r" % (
        cell["name"], what, kind, method, len(bad), got.size, sorted(set(bad[:, 1].tolist()))[:12],
        sorted(set(bad[:, 0].tolist()))[:6], got[tuple(bad[0])], ref[tuple(bad[0])])


@pytest.mark.parametrize("cell", CELLS, ids=_NAMES)
def test_exact_cell(lib, cell, monkeypatch):
    import time
    t_start = time.perf_counter()
    routes = default_routes()                   # (asked before the cell's own switches are set)
    for k, v in cell["env"]:
        monkeypatch.setenv(k, v)
    img, units, kinds, refs = cell_data(cell)
    n, out = cell["n"], cell["out"]
    singles = sorted({0, n // 2, n - 1})
    ctx = lib.Context(0)
    try:
        ctx.set_option(lib.OPT_HITS_ONLY, 0)
        ctx.set_option(lib.OPT_EXACT_DIV, 1)
        ctx.set_option(lib.OPT_F32_MFMA, 0)          # (no bf16 screen may answer for the float64 kernel)
        if cell["kernel"] == "dot4":
            ctx.set_option(lib.OPT_KERNEL, lib.KERNEL_DOT4)
            ctx.set_option(lib.OPT_DOT4_VARIANT, cell["variant"])
        elif cell["kernel"] == "naive":
            ctx.set_option(lib.OPT_KERNEL, lib.KERNEL_NAIVE)
        for method in cell["methods"]:
            nothing = -1.0 if method in (0, 1) else 1e30 if method in (2, 4) else 2.0      # the maps are what is checked
            for pattern in (0xFF, 0x7F):
                ctx.debug_poison(pattern, 7)
                ctx.search(units, img, method, lib.PEAKS_LOCAL, nothing)
                if routes:
                    _check_route(ctx, cell)
                for i in range(n):
                    _compare(cell, "search %#x map %d" % (pattern, i), kinds[i], method, ctx.last_score_map(i, out), refs[method][i])
                ctx.debug_poison(pattern, 7)
                for i in singles:
                    got = ctx.score_map(i, out)
                    if routes:
                        _check_route(ctx, cell)
                    _compare(cell, "score_map(%d) %#x" % (i, pattern), kinds[i], method, got, refs[method][i])
    finally:
        ctx.close()
    _RAN[cell["name"]] = time.perf_counter() - t_start


def test_the_sweep_ran_every_family():
    """On what ran in this session: a summary line (-s), and no family of the table without a cell - when the whole module
    ran."""
    if not _RAN:
        return
    slow = max(_RAN, key=_RAN.get)
    print("exact kernels: %d cells in %.1f s, slowest %s %.2f s" % (len(_RAN), sum(_RAN.values()), slow, _RAN[slow]))
    if len(_RAN) == len(CELLS):
        assert {c["family"] for c in CELLS} == {c["family"] for c in CELLS if c["name"] in _RAN}
