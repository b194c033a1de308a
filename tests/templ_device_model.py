"""Templates built on the device (csrc/mtm_templates.hip.h, set_templates_device of csrc/mtm_placement.hip) restated plainly -
numpy and Python integers only - and the table of cells tests/test_gpu_templ_device.py sweeps and
tests/test_templ_device_model_cpu.py checks without a GPU.

  area_resize_exact    the definition of the area resize in fractions.Fraction: the mean of the source over the output pixel's
                       footprint, rounded half up, clipped to 0 .. 255 (resize_area_kernel, MTM.augment.resize_area)
  downscale_int_exact  the integer-factor rule in literal loops (downscale_int_kernel, the image-side planarize kernels,
                       MTM.augment.downscale, mtm_oracle.downscale_area)
  apply_variant        resize, left-right flip, up-down flip, k quarter turns - index arithmetic, no np.rot90 / np.fliplr
  expand               base-major, as mtm_set_templates_augmented numbers its units
  expected_tiling      which kernel and tiling a size class enters, from the preconditions the tilings sweep documents
  CELLS                name, bases, mask kind, channels, variant records, methods, kernel option, the families it is there for
"""
import zlib
from fractions import Fraction

import numpy as np

# ---- the resizes ---------------------------------------------------------------------------------------------------------


def _overlaps(n_out, n_in):
    """[[(source index, overlap length as a Fraction of a source pixel)]] of the n_out output intervals
    [i n_in / n_out, (i + 1) n_in / n_out) with the unit source intervals [y, y + 1)."""
    out = []
    for i in range(n_out):
        lo, hi = Fraction(i * n_in, n_out), Fraction((i + 1) * n_in, n_out)
        row = []
        for y in range(int(lo), n_in):
            if y >= hi:
                break
            length = min(hi, Fraction(y + 1)) - max(lo, Fraction(y))
            if length > 0:
                row.append((y, length))
        assert sum(l for _, l in row) == hi - lo
        out.append(row)
    return out


def area_resize_exact(a, rows, cols):
    """Output (i, j) = the mean of the source over [i H / rows, (i + 1) H / rows) x [j W / cols, (j + 1) W / cols), rounded
    half up and clipped to 0 .. 255; per channel, and for mask bytes alike."""
    a = np.asarray(a)
    assert a.dtype == np.uint8 and rows >= 1 and cols >= 1
    H, W = a.shape[:2]
    planes = a.reshape(H, W, -1)
    wy, wx = _overlaps(rows, H), _overlaps(cols, W)
    area = Fraction(H, rows) * Fraction(W, cols)
    out = np.empty((rows, cols, planes.shape[2]), np.uint8)
    for c in range(planes.shape[2]):
        src = [[int(v) for v in row] for row in planes[:, :, c]]
        for i in range(rows):
            for j in range(cols):
                total = Fraction(0)
                for y, ly in wy[i]:
                    total += ly * sum(lx * src[y][x] for x, lx in wx[j])
                mean = total / area
                v = (2 * mean.numerator + mean.denominator) // (2 * mean.denominator)       # floor(mean + 1/2)
                out[i, j, c] = min(max(v, 0), 255)
    return out.reshape((rows, cols) + a.shape[2:])


def f32_scale(f):
    return np.float32(1.0) / np.float32(f * f)


def downscale_sum_rule(s, f, top=255):
    """The integer rule on one block sum: factor 2 -> (s + 2) >> 2; else the float32 product float32(s) float32(1 / f^2)
    rounded to nearest even; clipped to the type's top value."""
    if f == 2:
        return min((int(s) + 2) >> 2, top)
    prod = np.float32(np.float32(s) * f32_scale(f))
    return min(int(np.rint(prod)), top)


def downscale_int_exact(a, f):
    """rows // f x cols // f, remainder rows and columns dropped; uint8 / uint16: downscale_sum_rule of the block sum;
    float32: the row-major float32 block sum times float32(1 / f^2)."""
    a = np.asarray(a)
    f = int(f)
    if f == 1:
        return a
    H, W = a.shape[:2]
    r, c = H // f, W // f
    assert r >= 1 and c >= 1
    planes = a.reshape(H, W, -1)
    out = np.empty((r, c, planes.shape[2]), a.dtype)
    for ch in range(planes.shape[2]):
        for i in range(r):
            for j in range(c):
                if a.dtype == np.float32:
                    acc = np.float32(0.0)
                    for dy in range(f):
                        for dx in range(f):
                            acc = np.float32(acc + planes[i * f + dy, j * f + dx, ch])
                    out[i, j, ch] = np.float32(acc * f32_scale(f))
                else:
                    s = 0
                    for dy in range(f):
                        for dx in range(f):
                            s += int(planes[i * f + dy, j * f + dx, ch])
                    out[i, j, ch] = downscale_sum_rule(s, f, int(np.iinfo(a.dtype).max))
    return out.reshape((r, c) + a.shape[2:])


# ---- the variants ----------------------------------------------------------------------------------------------------------
def rec(k=0, lr=0, ud=0, rows=0, cols=0, down=0):
    return (k, lr, ud, rows, cols, down)


RECORDS16 = tuple(rec(k, lr, ud) for lr in (0, 1) for ud in (0, 1) for k in range(4))
EVEN_VIEWS = (rec(0), rec(0, 1, 0), rec(0, 0, 1), rec(2))                  # identity, lr, ud, half turn: the shape stays
ODD_VIEWS = (rec(1), rec(3), rec(1, 1, 0), rec(1, 0, 1))                   # the four with the axes exchanged
VIEWS8 = EVEN_VIEWS + ODD_VIEWS


def apply_variant(a, record):
    """resize, then left-right flip, then up-down flip, then k counter-clockwise quarter turns (np.rot90's sense):
    flip lr: new(y, x) = cur(y, W - 1 - x); flip ud: new(y, x) = cur(H - 1 - y, x); turn: new(i, j) = cur(j, W - 1 - i), W x H."""
    k, lr, ud, rows, cols, down = record
    a = np.asarray(a)
    if rows > 0:
        a = area_resize_exact(a, rows, cols)
    elif down > 1:
        a = downscale_int_exact(a, down)
    if lr:
        H, W = a.shape[:2]
        yy, xx = np.indices((H, W))
        a = a[yy, W - 1 - xx]
    if ud:
        H, W = a.shape[:2]
        yy, xx = np.indices((H, W))
        a = a[H - 1 - yy, xx]
    for _ in range(k):
        H, W = a.shape[:2]
        ii, jj = np.indices((W, H))
        a = a[jj, W - 1 - ii]
    return np.ascontiguousarray(a)


def expand(bases, recs):
    """[(pixels, mask or None)] of every base under every record, base-major: unit b * len(recs) + v."""
    return [tuple(None if a is None else apply_variant(a, r) for a in base) for base in bases for r in recs]


_PROBE = np.arange(6, dtype=np.uint8).reshape(2, 3)


def view_of(record):
    """A name for the view a record's (k, lr, ud) gives: the bytes of a 2 x 3 probe seen through it (8 distinct ones)."""
    v = apply_variant(_PROBE, rec(*record[:3]))
    return v.shape + tuple(v.ravel().tolist())


IDENTITY = view_of(rec())


def unit_shape(shape, record):
    k, _lr, _ud, rows, cols, down = record
    h, w = (rows, cols) if rows > 0 else ((shape[0] // down, shape[1] // down) if down > 1 else tuple(shape[:2]))
    return (w, h) if k % 2 else (h, w)


# ---- which tiling a class enters ---------------------------------------------------------------------------------------------
# The preconditions, as tests/test_gpu_tilings.py documents them next to its table: slabs beyond w = 256 or chans w h = 131071
# (the int32 accumulator); row-multiplexed for <= 16 templates whose fused window statistics exist (chans w h 255^2 < 2^32),
# one channel or unmasked RGB; packed K on the normalised methods where ceil(w / 16) is no multiple of four (not for a masked
# class on method 5); two-row for > 16 unmasked one-channel templates with w <= 64 on methods >= 2, with the tail screen for
# 8 <= h <= 71; a masked class on the matrix cores needs one channel, w h <= 66051 and a method <= 3.
FAMILIES = ("r2_screen", "r2_noscreen", "plain", "plain_kp", "rm", "rm_kp", "slab_rm", "slab_plain", "off_cores", "dot4", "naive")
VIEW_FAMILIES = FAMILIES[:6]


def rm_group_templates(n, h, w):
    """Templates per MFMA group of a row-multiplexed class: the next power of two, doubled while the LDS tile -
    min(h + 2R - 1, 64) + 6R rows (R = 16 / nt) of (16 + 4 nb + 1) 16 bytes - exceeds 72 KB."""
    nt = 1
    while nt < n:
        nt *= 2
    pitch = (16 + 4 * ((w + 63) // 64) + 1) * 16
    while nt < 16 and (min(h + 2 * (16 // nt) - 1, 64) + 6 * (16 // nt)) * pitch > 72 * 1024:
        nt *= 2
    return nt


def expected_tiling(n, h, w, chans, method, masked, kernel="auto"):
    """{"family", "kernel", and the exact fields that family fixes} of a uint8 class of n units h x w."""
    if kernel == "naive":
        return {"family": "naive", "kernel": 1}
    if kernel == "dot4":
        return {"family": "off_cores", "kernel": 0} if masked else {"family": "dot4", "kernel": 2}
    big = w > 256 or chans * w * h > 131071
    if masked and (big or chans != 1 or w * h > 66051 or method > 3):
        return {"family": "off_cores", "kernel": 0}
    if big:
        return {"family": "slab_rm" if n <= 16 else "slab_plain", "kernel": 3}
    one_pack = chans == 1 or (chans == 3 and not masked)
    fused = chans in (1, 3) and w <= 768 and chans * w * h * 255 * 255 < 2 ** 32
    nseg = (w + 15) // 16
    rm = n <= 16 and one_pack and fused
    kp = nseg % 4 != 0 and method in (1, 3, 5) and one_pack and not (masked and method == 5)
    out = {"kernel": 3, "kp_nseg": nseg if kp else 0, "rm_nt": rm_group_templates(n, h, w) if rm else 0, "r2": 0, "n_slabs": 0}
    if rm:
        out["family"] = "rm_kp" if kp else "rm"
    elif kp:
        out["family"] = "plain_kp"
    elif n > 16 and w <= 64 and chans == 1 and not masked and method >= 2:
        out["family"], out["r2"] = ("r2_screen" if 8 <= h <= 71 else "r2_noscreen"), 2
    else:
        out["family"] = "plain"
    out["tail_ok"] = int(out["family"] == "r2_screen")
    return out


def family_of(r):
    """The family of a Context.class_tilings() record."""
    if r["kernel"] != 3:
        return {0: "off_cores", 1: "naive", 2: "dot4"}[r["kernel"]]
    if r["n_slabs"]:
        return "slab_rm" if r["slab_nt"] else "slab_plain"
    if r["rm_nt"]:
        return "rm_kp" if r["kp_nseg"] else "rm"
    if r["r2"]:
        return "r2_screen" if r["tail_ok"] else "r2_noscreen"
    return "plain_kp" if r["kp_nseg"] else "plain"


# ---- the table -------------------------------------------------------------------------------------------------------------
CELLS = []


def _cell(name, group, bases, recs, methods=(5,), mask=None, chans=1, kernel="auto", want=(), tilings=True, content="noise",
          nt=None):
    """bases: shapes (h, w); content: how their pixels are made; mask: None or a kind of _mask; want: the families the cell is in
    the table for (checked against expected_tiling by the CPU file); nt: {(h, w): rm_nt} stated by hand where it is the point."""
    assert name not in {c["name"] for c in CELLS}
    CELLS.append(dict(name=name, group=group, bases=tuple(bases), recs=tuple(recs), methods=tuple(methods), mask=mask, chans=chans,
                      kernel=kernel, want=frozenset(want), tilings=tilings, content=content, nt=nt or {}))


def _both(shape, a=2, b=1):
    return [shape] * a + [shape[::-1]] * b


# views x tilings: bases S and S transposed under all 16 records - two classes of 8 (a + b) units, each holding all 8 views
_cell("v-r2screen-24x49", "views", _both((24, 49)), RECORDS16, (5,), want=("r2_screen", "plain_kp"))
_cell("v-r2screen-24x49-m3", "views", _both((24, 49), 1, 2), RECORDS16, (3,), want=("r2_screen", "plain_kp"))
_cell("v-r2no-7x64", "views", _both((7, 64)), RECORDS16, (3,), want=("r2_noscreen", "plain_kp"))
_cell("v-r2no-73x56", "views", _both((73, 56)), RECORDS16, (5,), want=("r2_noscreen", "plain_kp"))
_cell("v-plain1-24x49-m1", "views", _both((24, 49)), RECORDS16, (1,), want=("plain", "plain_kp"))       # below method 2: no two-row form
_cell("v-plain2-5x113", "views", _both((5, 113)), RECORDS16, (5,), want=("plain", "plain_kp"))
_cell("v-plain4-20x241", "views", _both((20, 241)), RECORDS16, (3,), want=("plain", "plain_kp"))
_cell("v-plain2-64x128", "views", _both((64, 128)), RECORDS16, (5,), want=("plain", "r2_noscreen"))
for _shape, _m in (((21, 15), 5), ((22, 16), 3), ((9, 81), 5), ((9, 111), 3), ((65, 40), 5)):
    _cell("v-kp-%dx%d" % _shape, "views", _both(_shape), RECORDS16, (_m,), want=("plain_kp",))
# row-multiplexed on both sides of an nt doubling: ONE unit per class (one base, one even and one odd view) and three (three
# transposed bases, so that the class of the edge holds the odd views); the turned classes are packed K
for _k, (_shape, _nt1) in enumerate((((31, 192), 1), ((32, 192), 2), ((12, 250), 1), ((13, 250), 2))):
    _cell("rm-%dx%d-n1" % _shape, "views", [_shape], (EVEN_VIEWS[_k], ODD_VIEWS[_k]), (5, 3)[_k % 2:][:1], want=("rm", "rm_kp"),
          nt={_shape: _nt1, _shape[::-1]: 1})
    _cell("rm-%dx%d-n3" % _shape, "views", [_shape[::-1]] * 3, (ODD_VIEWS[(_k + 1) % 4], EVEN_VIEWS[(_k + 1) % 4]), (3, 5)[_k % 2:][:1],
          want=("rm", "rm_kp"), nt={_shape: 4, _shape[::-1]: 4})
_cell("rm-kp-31x130-n1", "views", [(31, 130)], (rec(0, 1, 0), rec(3)), (5,), want=("rm_kp",), nt={(31, 130): 1})
_cell("rm-kp-32x130-n1", "views", [(32, 130)], (rec(2), rec(1, 1, 0)), (3,), want=("rm_kp",), nt={(32, 130): 2})
_cell("rm-kp-31x130-n3", "views", [(130, 31)] * 3, (rec(1, 0, 1), rec(0, 0, 1), rec(1), rec(0)), (5,), want=("rm_kp",))
# class sizes: bases x even views of one shape, so that the last group's tail lanes must be zero
for _n, _nb, _recs in ((1, 1, (rec(0, 1, 0),)), (15, 5, (rec(2), rec(0, 1, 0), rec(0, 0, 1))), (16, 4, EVEN_VIEWS), (17, 17, (rec(2),)),
                       (33, 11, (rec(0, 0, 1), rec(2), rec(0, 1, 0)))):
    _cell("n-%d-24x49" % _n, "sizes", [(24, 49)] * _nb, _recs, (5,), want=("rm",) if _n <= 16 else ("r2_screen",))
    _cell("n-%d-9x81" % _n, "sizes", [(9, 81)] * _nb, _recs, (3,), want=("rm_kp",) if _n <= 16 else ("plain_kp",))
# RGB: 3 x 148 x 148 x 255^2 < 2^32 row-multiplexed, 149 x 148 not
_cell("rgb-148x148", "views", [(148, 148)], (rec(1), rec(0, 1, 0), rec(2, 0, 1), rec(3, 1, 0)), (5,), chans=3, want=("rm_kp",),
      nt={(148, 148): 4})
_cell("rgb-149x148", "views", [(149, 148)], (rec(0, 1, 0), rec(2), rec(1), rec(3, 0, 1)), (3,), chans=3, want=("plain_kp",))
# slabs: by area with one unit (row-multiplexed raw launches), by width with 20 (plain raw launches)
_cell("slab-512x256", "views", [(512, 256)], (rec(2, 1, 0),), (5,), want=("slab_rm",))
_cell("slab-20x257", "views", [(20, 257)] * 5, EVEN_VIEWS, (3,), want=("slab_plain",))

# resizes
SIZES = ((23, 29), (50, 60), (1, 1), (37, 41), (64, 17), (50, 20), (24, 49), (9, 81))     # down, up, one pixel, each base's own
RS_BASES = ((37, 41), (64, 17))                                                           # size, up / down mixed, tiling edges
ALL_METHODS = (0, 1, 2, 3, 4, 5)
MASK_METHODS = (0, 3, 1)
_SIZE_RECS = tuple(rec(rows=r, cols=c) for r, c in SIZES)
_cell("rs-sizes", "resize", RS_BASES, _SIZE_RECS, ALL_METHODS)
_cell("rs-sizes-rgb", "resize", RS_BASES, _SIZE_RECS, ALL_METHODS, chans=3)
_cell("rs-sizes-rgb-mask", "resize", RS_BASES[:1], (rec(rows=23, cols=29), rec(rows=1, cols=1), rec(rows=50, cols=20)), MASK_METHODS,
      chans=3, mask="perchan", want=("off_cores",))
# factors 2, 3, 5, 7: seven bases whose rows and columns leave every remainder 0 .. f - 1
FACTORS = (2, 3, 5, 7)
FACTOR_BASES = tuple((42 + i, 49 + (3 * i) % 7) for i in range(7))
_FACTOR_RECS = tuple(rec(down=f) for f in FACTORS)
_cell("rs-factors", "resize", FACTOR_BASES, _FACTOR_RECS, ALL_METHODS)
_cell("rs-factors-rgb", "resize", FACTOR_BASES[:3], _FACTOR_RECS, ALL_METHODS, chans=3)
_cell("rs-factors-mask", "resize", FACTOR_BASES[2:5], _FACTOR_RECS, MASK_METHODS, mask="asym")
# ties, saturation, zero: constructed contents (tie_base), every base under every resize that can meet its ties
_cell("rs-ties", "resize", [(16, 24), (24, 36), (40, 60)], (rec(down=2), rec(down=3), rec(down=5), rec(rows=8, cols=12)), (3, 0),
      content="ties")
_cell("rs-sat-zero", "resize", [(37, 41), (37, 41)], (rec(down=2), rec(down=3), rec(down=5), rec(down=7), rec(rows=23, cols=29),
                                                    rec(rows=50, cols=60)), (3, 0), content="sat-zero")
# masks of 0 / 1 and of 0 / 255 bytes resized both ways (a 0 / 1 mask's area mean below one half is 0: no mask there)
_cell("rs-masks-01", "resize", RS_BASES, (rec(down=2), rec(down=3), rec(rows=23, cols=29), rec(rows=50, cols=60), rec(rows=9, cols=81)),
      MASK_METHODS, mask="asym01")
_cell("rs-masks-255", "resize", RS_BASES, (rec(down=2), rec(down=3), rec(rows=23, cols=29), rec(rows=50, cols=60), rec(rows=9, cols=81)),
      MASK_METHODS, mask="asym")
# resizes combined with views
_cell("rs-views", "resize", RS_BASES, tuple(rec(*v[:3], rows=r, cols=c, down=d) for r, c, d in ((24, 49, 0), (9, 81, 0), (0, 0, 3))
                                          for v in VIEWS8), (5,))
_cell("rs-views-mask", "resize", RS_BASES[:1], tuple(rec(*v[:3], rows=24, cols=40) for v in VIEWS8), (3,), mask="asym")

# masks: what decides which masked units share a class (mask_key) and so one mask pack
_cell("m-four-views", "masks", [(24, 40)], EVEN_VIEWS, MASK_METHODS, mask="asym", want=("rm_kp", "rm"))
_cell("m-square-turns", "masks", [(32, 32)], (rec(0), rec(1), rec(2), rec(3)), MASK_METHODS, mask="asym")
_cell("m-one-byte", "masks", [(24, 40)] * 2, (rec(0, 1, 0),), MASK_METHODS, mask="onebyte")
_cell("m-identical", "masks", [(24, 40)] * 2, (rec(2),), MASK_METHODS, mask="same", tilings=False)       # may share a class
_cell("m-plain-24x64", "masks", [(24, 64)] * 20, (rec(2), rec(0, 1, 0)), (3,), mask="same", want=("plain",))
_cell("m-kp-24x40", "masks", [(24, 40)] * 20, (rec(0, 0, 1), rec(2)), (1,), mask="same", want=("plain_kp",))
_cell("m-rm-9x128", "masks", [(9, 128)] * 3, (rec(0, 1, 0), rec(1)), (3,), mask="same", want=("rm", "rm_kp"), nt={(9, 128): 4})
_cell("m-off-259x256", "masks", [(259, 256)], (rec(2),), (3,), mask="asym", want=("off_cores",))
_cell("m-rgb-perchan", "masks", [(20, 33)], (rec(0, 1, 0), rec(1), rec(2), rec(3, 1, 0)), (3,), chans=3, mask="perchan", want=("off_cores",))

# the kernels that take host-packed weights: pixels and masks fetched back by gather_unit_kernel
_cell("fb-dot4-views", "fallback", [(21, 15)], RECORDS16, (5,), kernel="dot4", want=("dot4",))
_cell("fb-naive-views", "fallback", [(21, 15)], RECORDS16, (3,), kernel="naive", want=("naive",))
_cell("fb-dot4-resize", "fallback", RS_BASES[:1], (rec(1, rows=23, cols=29), rec(0, 1, 0, down=3), rec(3, 0, 1, rows=50, cols=60)), (5,),
      kernel="dot4", want=("dot4",))
_cell("fb-naive-resize-mask", "fallback", RS_BASES[:1], (rec(1, rows=23, cols=29), rec(2, 1, 0, down=2)), (3,), kernel="naive",
      mask="asym", want=("naive",))

NAMES = [c["name"] for c in CELLS]
BY_NAME = {c["name"]: c for c in CELLS}

# the readout family: two non-square shapes under all 16 records, TM_CCORR against one set pixel
READOUT = (((5, 17), 1), ((18, 7), 3))
# the image-side downscale: (dtype, channels), image shapes with remainders in both axes
IMAGE_DOWN = (("u8", 1), ("u8", 3), ("u16", 1), ("f32", 1))
IMAGE_DOWN_SHAPE = (45, 61)            # 45 = 2 22 + 1 = 3 15 = 5 9 = 7 6 + 3; 61 = 2 30 + 1 = 3 20 + 1 = 5 12 + 1 = 7 8 + 5


# ---- contents --------------------------------------------------------------------------------------------------------------
def tie_sums(f, top=255):
    """(sums on which the rule meets a tie, sums next to one): factor 2: s % 4 == 2 - the mean is k + 1/2 and (s + 2) >> 2
    rounds it up; otherwise the sums whose float32 product is exactly k + 1/2 (f odd: s / f^2 never is, so only a rounding
    of the product could make one) and the sums either side of every k + 1/2."""
    sums = range(top * f * f + 1)
    if f == 2:
        return [s for s in sums if s % 4 == 2], []
    ties, near = [], []
    for s in sums:
        prod = float(np.float32(np.float32(s) * f32_scale(f)))
        if prod - np.floor(prod) == 0.5:
            ties.append(s)
        if s % (f * f) in ((f * f - 1) // 2, (f * f + 1) // 2):
            near.append(s)
    return ties, near


def _block_with_sum(s, f, rng):
    """f x f bytes that add up to s."""
    q, r = divmod(s, f * f)
    b = np.full(f * f, q, np.int64)
    b[rng.permutation(f * f)[:r]] += 1
    assert b.sum() == s and b.max() <= 255
    return b.reshape(f, f)


def tie_base(shape, f, seed):
    """A base of f x f blocks whose sums are ties of the factor-f rule (where there are any) and sums next to a tie."""
    rng = np.random.default_rng(seed)
    ties, near = tie_sums(f)
    pool = ties + near
    a = np.zeros(shape, np.uint8)
    k = 0
    for i in range(shape[0] // f):
        for j in range(shape[1] // f):
            a[i * f:(i + 1) * f, j * f:(j + 1) * f] = _block_with_sum(pool[(k * 37) % len(pool)], f, rng)
            k += 1
    return a


def _mask(kind, shape, chans, rng, k):
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    # a wedge with holes: no symmetry under any flip or turn
    blob = ((xx * h * 10 >= yy * w * 6) & ((yy * 7 + xx * 3) % 11 != 0)) | ((yy < max(1, h // 5)) & (xx < max(1, w // 3)))
    if kind in ("asym", "same", "onebyte"):
        m = (blob * 255).astype(np.uint8)
        if kind == "asym":
            m[rng.random((h, w)) < 0.05] = 0
        if kind == "onebyte" and k == 1:
            m[h // 2, w // 3] ^= 255
    elif kind == "asym01":
        m = blob.astype(np.uint8)
        m[:, w // 2:] &= ((yy + xx) % 5 == 0)[:, w // 2:].astype(np.uint8)      # sparse ones: area means below one half
    else:
        raise ValueError(kind)
    if chans > 1:
        m = np.repeat(m[:, :, None], chans, axis=2)
    return np.ascontiguousarray(m)


def cell_bases(cell):
    """[(pixels, mask or None)] of a cell, from its name alone."""
    rng = np.random.default_rng(zlib.crc32(cell["name"].encode()))
    out = []
    for k, shape in enumerate(cell["bases"]):
        full = tuple(shape) + ((cell["chans"],) if cell["chans"] > 1 else ())
        if cell["content"] == "ties":
            px = tie_base(shape, (2, 3, 5)[k], k)
        elif cell["content"] == "sat-zero":
            px = np.full(full, 255 if k == 0 else 0, np.uint8)
        else:
            px = rng.integers(0, 256, full).astype(np.uint8)
        mask = None
        if cell["mask"] == "perchan":
            mask = np.stack([_mask("asym", shape, 1, rng, k) for _ in range(cell["chans"])], axis=2)
            assert not np.array_equal(mask[:, :, 0], mask[:, :, 1])
        elif cell["mask"] in ("same", "onebyte"):
            mask = _mask(cell["mask"], shape, cell["chans"], np.random.default_rng(7), k)
        elif cell["mask"]:
            mask = _mask(cell["mask"], shape, cell["chans"], rng, k)
        out.append((np.ascontiguousarray(px), mask))
    return out


def cell_units_shapes(cell):
    return [unit_shape(b, r) for b in cell["bases"] for r in cell["recs"]]


def cell_classes(cell, method):
    """[(h, w, n, expected_tiling, the views of its units)] of the classes of a cell, in order of first appearance.  Unmasked
    units share a class by shape; masked ones by shape, source mask (the base's bytes - every base has its own, but for the
    kinds "same" - and the resize made of them) and view: the least that keeps one mask pack per class right."""
    order, members = [], {}
    for k, b in enumerate(cell["bases"]):
        for r in cell["recs"]:
            s = unit_shape(b, r)
            key = (s, 0 if cell["mask"] == "same" else k, r[3:], view_of(r)) if cell["mask"] else s
            if key not in members:
                order.append(key)
                members[key] = []
            members[key].append(view_of(r))
    out = []
    for key in order:
        h, w = key[0] if cell["mask"] else key
        n = len(members[key])
        out.append((h, w, n, expected_tiling(n, h, w, cell["chans"], method, bool(cell["mask"]), cell["kernel"]), members[key]))
    return out


def cell_image(cell, units):
    """Sparse noise (two thirds of the pixels 0, see tests/test_gpu_tilings.py), the largest unit's shape plus (12, 37) - a map
    spans more than one 16- and 32-column tile and has a partial last one - with unit 0 planted, so that a threshold lists
    something."""
    rng = np.random.default_rng(zlib.crc32(("image " + cell["name"]).encode()))
    H = max(u[0].shape[0] for u in units) + 12
    W = max(u[0].shape[1] for u in units) + 37
    full = (H, W) + ((cell["chans"],) if cell["chans"] > 1 else ())
    img = (rng.integers(0, 256, full) * (rng.random(full) < 0.35)).astype(np.uint8)
    t = units[0][0]
    img[3:3 + t.shape[0], 5:5 + t.shape[1]] = t
    return np.ascontiguousarray(img)
