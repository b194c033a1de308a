"""The fused uint8 window statistics kernel (stats_u8_kernel) in every form - 8 or 4 output rows per work-group -
against tests/stats_model.py, byte for byte and with no tolerance: every output is an exact integer below 2^53 or a fixed
sequence of correctly rounded float64 operations on such integers, and a form only changes how the work is spread.
Context.debug_window_stats (mtm_debug_window_stats) launches the kernel through the function the search calls use, into
buffers that start out as a byte pattern: what a launch must not touch - rows outside its row units, planes rows it does
not convert, the header it is not asked to clear - has to keep it."""
import numpy as np
import pytest

import stats_model as M

pytestmark = pytest.mark.gpu

PATTERN = 0xA5
ALL_PLANES = ("t0", "sum2", "sq", "rsq", "blk")


@pytest.fixture(scope="module")
def ctx():
    from MTM import _lib
    return _lib.Context(0)


def _forms():
    from MTM import _lib
    return range(1, len(_lib.STATS_FORMS) + 1)


_MODELS = {}


def _model(image, h, w, num_type, tail_s):
    key = (image.tobytes(), image.shape, h, w, num_type, tail_s)
    if key not in _MODELS:
        _MODELS[key] = M.window_stats(image, h, w, num_type, tail_s)
    return _MODELS[key]


def check(ctx, image, h, w, num_type=1, form=0, tail_s=0, units=None, conv=None, planes=ALL_PLANES, zero_header=True):
    """One launch against the model: the wanted planes' rows of the launch's row units, the pattern everywhere else."""
    got = ctx.debug_window_stats(image, h, w, num_type, form=form, planes=planes, tail_s=tail_s, units=units, convert_rows=conv,
                                 zero_header=zero_header, pattern=PATTERN)
    exp = _model(image, h, w, num_type, tail_s)
    rows, cols = image.shape
    oh = rows - h + 1
    n_units = (oh + M.UNIT_ROWS - 1) // M.UNIT_ROWS
    u0, u1 = (0, n_units) if units is None else (units[0], min(units[1], n_units) if units[1] >= 0 else n_units)
    y0, y1 = u0 * M.UNIT_ROWS, min(u1 * M.UNIT_ROWS, oh)
    what = (form, h, w, image.shape, num_type, tail_s, units, conv)
    for name in tuple(planes) + (("blkq",) if tail_s else ()):
        g = got[name]
        assert g[y0:y1].tobytes() == exp[name][y0:y1].tobytes(), (name, what, np.argwhere(g[y0:y1] != exp[name][y0:y1])[:4])
        rest = np.concatenate([g[:y0].ravel(), g[y1:].ravel()]).view(np.uint8)
        assert (rest == PATTERN).all(), (name, "rows outside the launch's units were written", what)
    if conv is None:
        assert (got["u8"][:, :cols] == image).all() and (got["u8"][:, cols:] == 0).all(), what      # the source plane, untouched
        assert (got["u8b"] == PATTERN).all(), what
    else:
        u8, u8b = M.converted_planes(image, conv[0], conv[1], PATTERN)
        assert got["u8"].tobytes() == u8.tobytes() and got["u8b"].tobytes() == u8b.tobytes(), ("converted planes", what)
    # every work-group of the launch starts on an output row of its range: its prologue reads the h image rows from its first
    # row on, and the raw upload buffer of a search call ends with the image (oh % 8 in 1 .. 4 with 4 rows per work-group)
    from MTM import _lib
    rows_wg = _lib.STATS_FORMS[got["info"]["form"] - 1]
    assert got["info"]["grid_y"] == -(-(y1 - y0) // rows_wg) and y0 + (got["info"]["grid_y"] - 1) * rows_wg < y1, what
    header = 0 if zero_header else int.from_bytes(bytes([PATTERN]) * 8, "little")
    assert got["header"].tolist() == [header, header], what
    return got


def _random(rows, cols, seed=0):
    return np.random.default_rng(seed + rows * 7919 + cols).integers(0, 256, (rows, cols), dtype=np.uint8)


@pytest.mark.parametrize("h", [1, 2, 7, 8, 9, 64, 71, 85])
@pytest.mark.parametrize("w", [1, 3, 16, 63, 64, 65, 768])
def test_window_sizes(ctx, w, h):
    """Every window size of the table on a small image (one strip, two row units, a width that is no multiple of 4), random
    and saturated: 768 x 85 at 255 is just under the kernel's admission bound w h 255^2 < 2^32."""
    rows, cols = h + 10, w + 37
    tail_s = 6 if h >= 8 else 0
    for image in (_random(rows, cols), np.full((rows, cols), 255, np.uint8)):
        for form in _forms():
            check(ctx, image, h, w, form=form, tail_s=tail_s)


# w = 65 and w = 1 make strips of exactly 1024 image columns (owg + w - 1 = 1024: the E[1024] read)
@pytest.mark.parametrize("w,cols", [(65, 165), (65, 1024), (65, 1025), (65, 1026), (65, 1027), (65, 1028), (65, 1031), (65, 2000),
                                    (1, 1024), (1, 1025), (1, 1028), (64, 1024), (64, 1028), (768, 1030)])
def test_strips(ctx, w, cols):
    """One partial strip, a strip of exactly 1024 columns, two strips whose last holds 1 .. 4 output columns, widths that
    are and are not multiples of 4; with the conversion (cols % 4 == 0: the raw buffer's pitch is the image's width, so the
    last quad sits at the pitch's edge) and without."""
    h, rows = 8, 8 + 8
    image = _random(rows, cols)
    for form in _forms():
        check(ctx, image, h, w, form=form, tail_s=6)
        if cols % 4 == 0:
            check(ctx, image, h, w, form=form, tail_s=6, conv=(0, rows))


@pytest.mark.parametrize("oh", [1, 3, 4, 5, 7, 8, 9, 12, 13, 15, 16, 17, 33])
def test_output_heights_and_unit_ranges(ctx, oh):
    """Output heights around the row unit and around every form's rows per work-group (4, 8; a last unit of 1 .. 4 rows included), the whole range and the
    range split at every unit - each part a launch of its own, as the banded upload makes them -, with the rows that have
    'just arrived' converted on the way and without."""
    h, w, cols = 9, 16, 100
    rows = oh + h - 1
    image = _random(rows, cols)
    n_units = (oh + 7) // 8
    for form in _forms():
        check(ctx, image, h, w, form=form, tail_s=6)
        check(ctx, image, h, w, form=form, tail_s=6, conv=(0, rows))
        for k in range(1, n_units):
            # the band boundary of a banded upload: rows up to the window bottoms of unit k - 1 first, the rest behind
            r_split = min(rows, 8 * k + h - 1)
            check(ctx, image, h, w, form=form, tail_s=6, units=(0, k), conv=(0, r_split))
            check(ctx, image, h, w, form=form, tail_s=6, units=(k, n_units), conv=(r_split, rows), zero_header=False)
            check(ctx, image, h, w, form=form, tail_s=6, units=(k, k + 1))


@pytest.mark.parametrize("h,tail_s", [(64, 6), (64, 33), (64, 62), (9, 6), (9, 7), (85, 6), (85, 40), (85, 83)])
def test_tail_splits(ctx, h, tail_s):
    rows, cols, w = h + 18, 150, 24
    image = _random(rows, cols)
    for form in _forms():
        check(ctx, image, h, w, form=form, tail_s=tail_s)


@pytest.mark.parametrize("num_type", [0, 1, 2])
@pytest.mark.parametrize("planes", [ALL_PLANES, ("t0", "sum2", "sq", "blk"), ("sum2", "sq"), ("t0",), ("sq", "rsq")])
def test_num_types_and_planes(ctx, num_type, planes):
    """The three numerator types, the reciprocal plane on and off (instantiations of their own), planes left out."""
    image = _random(40, 300)
    for form in _forms():
        check(ctx, image, 16, 32, num_type=num_type, form=form, planes=planes, tail_s=8 if "blk" in planes else 0)


def _contents():
    rows, cols = 64 + 40, 2100              # three strips of 960 output columns, six row units
    step = np.zeros((rows, cols), np.uint8)
    step[:, cols // 2 + 3:] = 200
    step[rows // 2 + 1:] += 55
    bright = np.zeros((rows, cols), np.uint8)
    bright[70, 1000] = 255
    return {"random": _random(rows, cols), "zeros": np.zeros((rows, cols), np.uint8), "saturated": np.full((rows, cols), 255, np.uint8),
            "step": step, "bright_pixel": bright}


@pytest.mark.parametrize("content", ["random", "zeros", "saturated", "step", "bright_pixel"])
def test_contents(ctx, content):
    """The headline window (64 x 64, split 42) over three strips: flat windows (the guard of window_norm, sqrt 0, the
    reciprocal's zero), an edge, one pixel."""
    image = _contents()[content]
    for form in _forms():
        check(ctx, image, 64, 64, form=form, tail_s=42)
    check(ctx, image, 64, 64, form=0, tail_s=42, conv=(0, image.shape[0]))


def test_the_launchers_choice(ctx):
    """Form 0: 4 rows per work-group for a launch of at most 2 x n_cus work-groups of 8 rows (strips x units), 8 rows beyond -
    both sides of the crossover, one unit apart, on a 6-strip image; the model's bytes either way."""
    h, w, cols, strips = 2, 768, 2100, 6            # 256 output columns per strip
    n_cus = ctx.debug_window_stats(_random(8, 16), 2, 2, 1)["info"]["n_cus"]
    k = 2 * n_cus // strips                         # strips * k <= 2 n_cus < strips * (k + 1)
    image = _random((k + 1) * 8 + h - 1, cols)
    for units, form in ((k, 2), (k + 1, 1)):
        got = check(ctx, image, h, w, form=0, units=(0, units), planes=("sq",))
        assert (got["info"]["grid_x"], got["info"]["form"]) == (strips, form), (n_cus, units, got["info"])
    assert check(ctx, _random(30, 200), 8, 16, form=0, tail_s=6)["info"]["form"] == 2


def test_refusals(ctx):
    from MTM import _lib
    image = _random(100, 900)
    with pytest.raises(_lib.MtmError):
        ctx.debug_window_stats(image, 90, 769, 1)                       # w > 768
    with pytest.raises(_lib.MtmError):
        ctx.debug_window_stats(image, 100, 700, 1)                      # w h 255^2 >= 2^32
    with pytest.raises(_lib.MtmError):
        ctx.debug_window_stats(image, 8, 8, 1, form=len(_lib.STATS_FORMS) + 1)
    with pytest.raises(_lib.MtmError):
        ctx.debug_window_stats(image[:, :899], 8, 8, 1, convert_rows=(0, 100))     # the conversion needs cols % 4 == 0
    assert _lib.load().mtm_debug_window_stats(None, None) == -1
