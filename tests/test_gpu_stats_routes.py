"""The six window-statistics kernel chains next to the fused single-channel uint8 one - U8MC, U16, U8_2P, U8_2P_WIDE, F64_LDS,
F64 (csrc/mtm_stats_route.h) - against tests/stats_routes_model.py, byte for byte and with no tolerance: every plane is an
exact integer below 2^53 or a fixed sequence of correctly rounded float64 operations.  Context.debug_window_stats_route
(mtm_debug_window_stats_route) runs each chain through the launcher the search calls use, in a buffer that starts out as a
byte pattern: what a launch must not touch - planes it was not asked for, the pitch columns of a two-pass chain, rows outside
its units - has to keep it.  The shapes are the smallest at which each mechanism of the kernels turns over."""
import time

import numpy as np
import pytest

import stats_routes_model as R

pytestmark = pytest.mark.gpu

ALL = ("t", "sum2", "sq")
CELLS = {"n": 0, "slowest": (0.0, None), "ratio": (0.0, None)}


@pytest.fixture(scope="module")
def ctx():
    from MTM import _lib
    return _lib.Context(0)


@pytest.fixture(params=[0xA5, 0x7F])
def pattern(request):
    return request.param


_MODELS = {}


def _model(image, h, w, num_type, route):
    exact = image.dtype != np.float32 or bool(np.array_equal(image, np.floor(image)) and image.min() >= 0 and image.max() < 65536)
    key = (image.tobytes(), image.shape, image.dtype.str, h, w, num_type, route if exact else -1)
    if key not in _MODELS:
        if len(_MODELS) > 64:
            _MODELS.clear()
        _MODELS[key] = R.integer_stats(image, h, w, num_type, route) if exact else R.replay_stats(image, h, w, num_type)
    return _MODELS[key]


def check(ctx, image, h, w, num_type=1, route=0, want=ALL, units=None, rows_in=None, pattern=0xA5):
    """One launch against the model: the wanted planes where the route writes them, the pattern everywhere else."""
    t_start = time.perf_counter()
    got = ctx.debug_window_stats_route(image, h, w, num_type, route=route, want=want, units=units, rows_in=rows_in, pattern=pattern)
    rows, cols = image.shape[:2]
    chans = 1 if image.ndim == 2 else image.shape[2]
    ran = got["info"]["route"]
    if route == 0:
        assert ran == R.stats_route(image.dtype, chans, h, w, cols), (ran, image.dtype, chans, h, w, cols)
    else:
        assert ran == route
    exp = _model(image, h, w, num_type, ran)
    oh = rows - h + 1
    n_units = (oh + R.UNIT_ROWS - 1) // R.UNIT_ROWS
    u0, u1 = (0, n_units) if units is None else (units[0], min(units[1], n_units) if units[1] >= 0 else n_units)
    y0, y1 = u0 * R.UNIT_ROWS, min(u1 * R.UNIT_ROWS, oh)
    what = (R.ROUTES[ran], image.dtype.str, image.shape, h, w, num_type, want, units, rows_in, hex(pattern))
    written = np.zeros_like(exp["cover"])
    written[y0:y1] = exp["cover"][y0:y1]
    two_pass = ran not in R.FUSED

    def plane(g, e, wanted, name):
        assert g.dtype == np.float64 and g.shape == e.shape
        cells = written if wanted else np.zeros_like(written)
        assert g[cells].tobytes() == e[cells].tobytes(), (name, what, np.argwhere(cells & (g != e))[:4])
        assert (g[~cells].view(np.uint8) == pattern).all(), (name, "written where the launch has no business", what)

    for c in range(4):
        plane(got["t"][c], exp["t"][c] if c < chans else np.zeros_like(exp["sum2"]), "t" in want and c < chans, "t%d" % c)
    plane(got["sum2"], exp["sum2"], "sum2" in want or two_pass, "sum2")
    plane(got["sq"], exp["sq"], "sq" in want, "sq")
    if "blk" in want:
        assert got["blk"][y0:y1].tobytes() == exp["blk"][y0:y1].tobytes(), ("blk", what, np.argwhere(got["blk"][y0:y1] != exp["blk"][y0:y1])[:4])
        rest = np.concatenate([got["blk"][:y0].ravel(), got["blk"][y1:].ravel()]).view(np.uint8)
        assert (rest == pattern).all(), ("blk", "rows outside the launch's units were written", what)
    else:
        assert (got["blk"].view(np.uint8) == pattern).all(), ("blk", what)
    CELLS["n"] += 1
    dt = time.perf_counter() - t_start
    if dt > CELLS["slowest"][0]:
        CELLS["slowest"] = (dt, what)
    return got


def _rand(dtype, rows, cols, chans=1, seed=0):
    rng = np.random.default_rng(seed + rows * 7919 + cols * 31 + chans)
    shape = (rows, cols) if chans == 1 else (rows, cols, chans)
    if np.dtype(dtype) == np.float32:
        return rng.normal(0.0, 40.0, shape).astype(np.float32)
    return rng.integers(0, int(np.iinfo(dtype).max) + 1, shape).astype(dtype)


FUSED_KINDS = [(R.U8MC, np.uint8, 3), (R.U16, np.uint16, 1)]


def _owg(w):
    return (1025 - w) & ~15


# ---- strip geometry of the two fused kernels -------------------------------------------------------------------------------
@pytest.mark.parametrize("route,dtype,chans", FUSED_KINDS)
@pytest.mark.parametrize("w", [1, 64, 65, 768])
def test_strips(ctx, pattern, route, dtype, chans, w):
    """owg = (1025 - w) & ~15 output columns a strip: w = 1 and w = 65 make strips of exactly 1024 image columns (the E[1024]
    read), 768 the narrowest (256); one partial strip, one exact strip, a last strip of 1 .. 5 output columns - widths that
    are no multiple of 4 or 16 among them."""
    h, rows = 8, 8 + 8
    owg = _owg(w)
    assert owg == {1: 1024, 64: 960, 65: 960, 768: 256}[w]
    for ow in (owg // 2 + 3, owg, owg + 1, owg + 2, owg + 3, owg + 4, owg + 5):
        got = check(ctx, _rand(dtype, rows, ow + w - 1, chans), h, w, want=ALL + (("blk",) if route == R.U16 else ()), pattern=pattern)
        assert got["info"]["grid1_x"] == -(-ow // owg) and got["info"]["grid2_x"] == 0


@pytest.mark.parametrize("route,dtype,chans", FUSED_KINDS)
@pytest.mark.parametrize("h", [1, 2, 3, 4, 5, 8, 9])
def test_rows(ctx, route, dtype, chans, h):
    """The column-sum prologue's batches of four rows (min(r0 + i, h - 1)) and output heights around the 8-row unit."""
    w, cols = 5, 41
    for oh in (1, 7, 8, 9, 17):
        check(ctx, _rand(dtype, oh + h - 1, cols, chans), h, w, want=ALL + (("blk",) if route == R.U16 else ()))


def test_u16_unit_ranges(ctx, pattern):
    image = _rand(np.uint16, 17 + 8, 70)
    for units in ((1, 2), (1, 3), (0, 1), (2, 3)):
        got = check(ctx, image, 9, 6, units=units, want=ALL + ("blk",), pattern=pattern)
        assert got["info"]["grid1_y"] == units[1] - units[0]


# ---- value range -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(86, 256), (28, 768)])
def test_u8mc_saturated(ctx, h, w):
    """The largest admitted areas: the all-channel prefix of the squares wraps modulo 2^32 along the strip, the window sum
    (3 w h 255^2 < 2^32) does not."""
    assert 3 * h * w * 255 * 255 < 2 ** 32 <= 3 * (h + 1) * w * 255 * 255
    image = np.full((h + 3, w + 21, 3), 255, np.uint8)
    for num_type in (0, 1):
        check(ctx, image, h, w, num_type=num_type)


@pytest.mark.parametrize("h,w", [(256, 256), (255, 257)])
def test_u16_saturated(ctx, h, w):
    """S1 = 256 * 256 * 65535 = 4 294 901 760: 65 536 below the uint32 limit."""
    assert h * w * 65535 < 2 ** 32
    image = np.full((h + 2, w + 9), 65535, np.uint16)
    for num_type in (0, 1):
        check(ctx, image, h, w, num_type=num_type, want=ALL + ("blk",))


U16_EDGES = [0x0000, 0x007F, 0x0080, 0x00FF, 0x7FFF, 0x8000, 0x80FF, 0xFF00, 0xFFFF]


def test_u16_bias_edges(ctx):
    """Pixels on both sides of the bias in either byte plane, in runs and as single pixels in a field of another."""
    runs = np.repeat(np.array(U16_EDGES, np.uint16), 7)[None, :].repeat(20, axis=0)
    check(ctx, runs, 3, 4, want=ALL + ("blk",))
    check(ctx, np.ascontiguousarray(runs.T), 4, 3, want=ALL + ("blk",))
    for k, v in enumerate(U16_EDGES):
        single = np.full((12, 37), U16_EDGES[(k + 4) % len(U16_EDGES)], np.uint16)
        single[5, 17] = v
        check(ctx, single, 3, 5, want=ALL + ("blk",))


def test_u8mc_channels_apart(ctx):
    """Channels that cannot be confused with each other: a ramp, zeros, saturated - in every order."""
    rows, cols = 21, 75
    ramp = (np.arange(rows)[:, None] * 3 + np.arange(cols)[None, :]).astype(np.uint8)
    planes = [ramp, np.zeros((rows, cols), np.uint8), np.full((rows, cols), 255, np.uint8)]
    for order in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        image = np.ascontiguousarray(np.stack([planes[i] for i in order], axis=2))
        for num_type in (0, 1, 2):
            check(ctx, image, 6, 10, num_type=num_type)


@pytest.mark.parametrize("num_type", [0, 1, 2])
def test_u16_block_records(ctx, num_type):
    """A block whose smallest and largest window sum sit in its first and its last column (and the other way round), a
    block cut by ow, flat windows (sq = 0 is the block's minimum).  (A block wholly beyond ow cannot occur inside blk_pitch =
    ceil(round_up(ow, 4) / 16) blocks - 16 b >= ow and 16 b < round_up(ow, 4) have no common solution - so the
    lo = hi = 0, sm = +inf record the model and the kernel keep for it never comes into play on this route.)"""
    rows, cols = 10, 45                                  # h = w = 1: ow = 45 - blocks 0, 1 whole, block 2 cut at 13 columns
    image = np.full((rows, cols), 1000, np.uint16)
    image[:, 16], image[:, 31] = 3, 60000               # block 1: minimum first, maximum last
    image[:, 0], image[:, 15] = 65535, 0                # block 0: maximum first, minimum last
    image[:, 44] = 7                                    # the cut block's last column inside ow
    got = check(ctx, image, 1, 1, num_type=num_type, want=ALL + ("blk",))
    assert got["blk"][0, 1, :2].tolist() == [3.0, 60000.0] and got["blk"][0, 0, :2].tolist() == [0.0, 65535.0]
    assert got["blk"][0, 2, :2].tolist() == [7.0, 1000.0]
    wide = np.full((rows, 60), 500, np.uint16)          # w = 16: ow = 45 again; windows 16 .. 31 flat, the rest not
    wide[:, :8], wide[:, 50:] = 0, 9
    got = check(ctx, wide, 3, 16, num_type=num_type, want=ALL + ("blk",))
    if num_type == 1:
        assert got["blk"][0, 1, 2] == 0.0 and got["blk"][0, 0, 2] == 0.0 and got["blk"][0, 2, 2] == 0.0
    check(ctx, np.full((rows, 60), 77, np.uint16), 3, 16, num_type=num_type, want=ALL + ("blk",))


# ---- the uint8 two-pass chains ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [255, 256, 257, 513])
@pytest.mark.parametrize("chans", [1, 2, 4])
def test_u8_two_pass_scan_rounds(ctx, cols, chans):
    """hsum_u8_kernel's 256-column scan rounds and their carry: one round short by a column, exact, one column and one
    round more; 2 and 4 channels take the route by themselves, 1 is forced onto it."""
    image = _rand(np.uint8, 12, cols, chans)
    check(ctx, image, 4, 9, route=R.U8_2P if chans == 1 else 0)
    check(ctx, np.full_like(image, 255), 4, 9, route=R.U8_2P if chans == 1 else 0)


def test_u8_two_pass_8191_columns(ctx):
    """The widest image of the route: 65 536 B of dynamic LDS next to the kernel's static words."""
    for chans in (1, 2):
        got = check(ctx, _rand(np.uint8, 6, 8191, chans), 3, 40, route=R.U8_2P if chans == 1 else 0)
        assert got["info"]["lds_bytes"] == 65536 and got["info"]["grid1_x"] == 6


@pytest.mark.parametrize("w,cols", [(769, 800), (1100, 1130)])
def test_u8_two_pass_wide_windows(ctx, w, cols):
    for chans in (1, 3):
        check(ctx, _rand(np.uint8, 9, cols, chans), 5, w)


def test_u8_two_pass_large_sums(ctx):
    """260 x 260 on a saturated image: a window sum of squares of 4 395 690 000 >= 2^32 - why the route exists."""
    assert 260 * 260 * 255 * 255 >= 2 ** 32
    for num_type in (0, 1, 2):
        check(ctx, np.full((300, 300), 255, np.uint8), 260, 260, num_type=num_type)
    check(ctx, _rand(np.uint8, 300, 300), 260, 260)


@pytest.mark.parametrize("h", [1, 7, 8, 9, 17])
def test_u8_two_pass_heights(ctx, h):
    """vsum_stats_kernel's batches of eight rows, and its band restarts every 32 output rows."""
    for oh in (31, 32, 33, 65):
        check(ctx, _rand(np.uint8, oh + h - 1, 30, 2), h, 7)


@pytest.mark.parametrize("ow", [255, 256, 257])
def test_u8_two_pass_widths(ctx, ow):
    got = check(ctx, _rand(np.uint8, 10, ow + 10, 2), 3, 11)
    assert got["info"]["grid2_x"] == -(-ow // 256)


@pytest.mark.parametrize("cols,w", [(8200, 9), (8200, 8), (8192, 4097)])
def test_u8_two_pass_wide_images(ctx, cols, w):
    """ow = 8192 and 8193: two row-sum work-groups of 4096 columns exactly, then one column more; 1 and 3 channels are forced
    onto the route (they have fused kernels at these windows), 2 channels take it by themselves."""
    for chans, route in ((1, R.U8_2P_WIDE), (3, R.U8_2P_WIDE), (2, 0)):
        got = check(ctx, _rand(np.uint8, 12, cols, chans), 5, w, route=route)
        assert got["info"]["grid1_x"] == -(-(cols - w + 1) // 4096) and got["info"]["route"] == R.U8_2P_WIDE


# ---- the float64 chains ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ow", [15, 16, 17, 4095, 4096, 4097])
@pytest.mark.parametrize("w", [1, 16, 17])
def test_f64_widths(ctx, ow, w):
    for chans in ((1, 3) if ow < 100 else (1,)):
        check(ctx, R.float_data("normal_1000_5", 6, ow + w - 1, chans, seed=ow), 3, w)


@pytest.mark.parametrize("ow", [15, 17, 4097])
def test_f64_lds_against_generic_row_sums(ctx, ow):
    """w = 1024 runs on hsum_lds_kernel, w = 1025 on hsum_kernel<double>; at 1024 the same image through both (forced): the
    same bytes from either."""
    image = R.float_data("normal_0_40", 5, ow + 1024 - 1, 1, seed=ow)
    a = check(ctx, image, 3, 1024)
    b = check(ctx, image, 3, 1024, route=R.F64)
    assert (a["info"]["route"], b["info"]["route"]) == (R.F64_LDS, R.F64)
    for k in ("t", "sum2", "sq"):
        assert a[k].tobytes() == b[k].tobytes(), k
    wider = R.float_data("normal_0_40", 5, ow + 1025 - 1, 1, seed=ow)
    assert check(ctx, wider, 3, 1025)["info"]["route"] == R.F64


@pytest.mark.parametrize("chans", [1, 2, 3, 4])
def test_f64_channels(ctx, chans):
    for route in (0, R.F64):
        check(ctx, R.float_data("normal_1000_5", 40, 50, chans, seed=chans), 7, 19, route=route)
    check(ctx, _rand(np.uint16, 40, 50, chans), 7, 19, route=0 if chans > 1 else R.F64_LDS)       # multi-channel uint16: this route


@pytest.mark.parametrize("kind", R.FLOAT_KINDS)
def test_f64_contents(ctx, kind):
    """Every content against the replay of the kernels' additions (bytes), and the device's window sums against exact ones
    within the derived bound (stats_routes_model.exact_sums)."""
    for rows, cols, h, w, chans in ((70, 50, 5, 17, 1), (40, 40, 33, 3, 2)):
        image = R.float_data(kind, rows, cols, chans, seed=1)
        for route in (0, R.F64):
            got = check(ctx, image, h, w, num_type=1, route=route)
        s1, s2, b1, b2, _ = R.exact_sums(image, h, w)
        ow = cols - w + 1
        for c in range(chans):
            ratio, at = R.error_ratio(got["t"][c, :, :ow], s1[c], b1[c])
            print("float route, %s %dx%d window %dx%d channel %d: worst |S1 - exact| / bound = %.4f at %s" % (kind, rows, cols, h, w, c, ratio, at))
            assert ratio <= 1.0, (kind, c, ratio, at)
            if ratio > CELLS["ratio"][0]:
                CELLS["ratio"] = (ratio, (kind, "S1", (rows, cols, h, w), c, at))
        if chans == 1:
            ratio, at = R.error_ratio(got["sum2"][:, :ow], s2[0], b2[0])
            print("float route, %s %dx%d window %dx%d: worst |S2 - exact| / bound = %.4f at %s" % (kind, rows, cols, h, w, ratio, at))
            assert ratio <= 1.0, (kind, ratio, at)
            if ratio > CELLS["ratio"][0]:
                CELLS["ratio"] = (ratio, (kind, "S2", (rows, cols, h, w), 0, at))


def test_f64_lds_partial_launches(ctx, pattern):
    """The launch of a band of a banded upload: row sums of the image rows that have just arrived, then the windows they
    complete - the whole-image launch's bytes in those rows, nothing outside them."""
    h, w, rows, cols = 9, 12, 83, 61
    image = R.float_data("normal_1000_5", rows, cols, 1, seed=9)
    whole = check(ctx, image, h, w, pattern=pattern)
    oh = rows - h + 1
    for units, rows_in in (((4, 8), (20, 75)), ((4, 8), (32, 72)), ((8, -1), (64, 83)), ((0, 4), (0, 40)), ((4, -1), (1, rows))):
        part = check(ctx, image, h, w, units=units, rows_in=rows_in, pattern=pattern)
        y0, y1 = units[0] * 8, oh if units[1] < 0 else units[1] * 8
        for k in ("t", "sum2", "sq"):
            assert part[k][..., y0:y1, :].tobytes() == whole[k][..., y0:y1, :].tobytes(), (k, units)
        assert part["info"]["grid1_y"] == rows_in[1] - rows_in[0] and part["info"]["grid2_y"] == -(-(y1 - y0) // 32)


# ---- numerator types and planes, on every route ----------------------------------------------------------------------------
ROUTE_IMAGES = {R.U8MC: (np.uint8, 3, 0), R.U16: (np.uint16, 1, 0), R.U8_2P: (np.uint8, 2, 0), R.U8_2P_WIDE: (np.uint8, 2, R.U8_2P_WIDE),
                R.F64_LDS: (np.float32, 2, 0), R.F64: (np.float32, 1, R.F64)}
WANTS = [ALL, ("sum2", "sq"), ("t", "sum2"), ("sum2",), ("t", "sum2", "nulls"), ("sum2", "nulls"), ("sum2", "sq", "nulls")]
FUSED_WANTS = [("t",), ("sq",), (), ("t", "nulls"), ("sq", "nulls")]


@pytest.mark.parametrize("route", sorted(ROUTE_IMAGES))
@pytest.mark.parametrize("num_type", [0, 1, 2])
def test_num_types_and_planes(ctx, pattern, route, num_type):
    """num_type 0 / 1 / 2 crossed with the planes asked for; planes not asked for keep the pattern (the two-pass chains
    write sum2 whatever is asked); "nulls": the kernels get NULL for them, as the masked float32 path calls the F64_LDS chain."""
    dtype, chans, force = ROUTE_IMAGES[route]
    image = _rand(dtype, 21, 43, chans, seed=route)
    for want in WANTS + (FUSED_WANTS if route in R.FUSED else []):
        got = check(ctx, image, 6, 9, num_type=num_type, route=force, want=want, pattern=pattern)
        assert got["info"]["route"] == route
    if route == R.F64_LDS:      # launch_masked_bf16's call: one channel, sums only, t1 .. t3 and sq NULL
        check(ctx, _rand(np.float32, 21, 43, 1), 6, 9, num_type=0, want=("t", "sum2", "nulls"), pattern=pattern)


# ---- refusals: one per message ---------------------------------------------------------------------------------------------
def test_refusals(ctx):
    from MTM import _lib
    u8, u16, f32 = _rand(np.uint8, 40, 60), _rand(np.uint16, 40, 60), _rand(np.float32, 40, 60)
    rgb = _rand(np.uint8, 40, 60, 3)

    def refused(message, image, h, w, **kw):
        with pytest.raises(_lib.MtmError, match=message):
            ctx.debug_window_stats_route(image, h, w, kw.pop("num_type", 1), **kw)

    refused("a window inside it", u16, 41, 8)
    refused("1 .. 4 channels", _rand(np.uint8, 10, 10, 5), 2, 2)
    refused("num_type 0 .. 2", u16, 8, 8, num_type=3)
    refused("num_type 0 .. 2", u16, 8, 8, route=7)
    refused("mtm_debug_window_stats's", u8, 8, 8)
    refused("the fused RGB kernel takes", u8, 8, 8, route=R.U8MC)                                        # one channel
    refused("the fused RGB kernel takes", _rand(np.uint8, 4, 800, 3), 2, 769, route=R.U8MC)             # w > 768
    refused("the fused RGB kernel takes", _rand(np.uint8, 90, 260, 3), 87, 256, route=R.U8MC)           # 3 w h 255^2 >= 2^32
    refused("the fused uint16 kernel takes", u8, 8, 8, route=R.U16)
    refused("the fused uint16 kernel takes", _rand(np.uint16, 4, 800), 2, 769, route=R.U16)
    refused("the fused uint16 kernel takes", _rand(np.uint16, 260, 260), 256, 257, route=R.U16)         # w h 65535 >= 2^32
    refused("two-pass kernels take uint8", f32, 8, 8, route=R.U8_2P)
    refused("two-pass kernels take uint8", u16, 8, 8, route=R.U8_2P_WIDE)
    refused("cols <= 8191", _rand(np.uint8, 4, 8192), 2, 2, route=R.U8_2P)
    refused("w <= 1024", _rand(np.float32, 3, 1030), 2, 1025, route=R.F64_LDS)
    refused("empty range of row units", u16, 8, 8, units=(3, 3))
    refused("the F64_LDS route only", u16, 8, 8, rows_in=(0, 40))
    refused("a range of row units", rgb, 8, 8, units=(1, 2))
    refused("a range of row units", f32, 8, 8, units=(1, 2))                                            # F64_LDS, but no rows_in
    tall = _rand(np.float32, 83, 30)
    refused("a multiple of 32", tall, 9, 8, units=(1, 8), rows_in=(0, 83))
    refused("lay_r0 <= sb0", tall, 9, 8, units=(4, 8), rows_in=(33, 83))
    refused("lay_r0 <= sb0", tall, 9, 8, units=(4, 8), rows_in=(20, 84))
    refused("lay_r1 < min", tall, 9, 8, units=(4, 8), rows_in=(20, 71))
    refused("lay_r1 < min", tall, 9, 8, units=(4, -1), rows_in=(20, 82))
    refused("blk: the U16 route only", rgb, 8, 8, want=ALL + ("blk",))
    refused("it cannot be null", f32, 8, 8, want=("t", "nulls"))
    refused("more than 256 MB", np.zeros((1000, 16000, 4), np.uint8), 990, 15990)
    assert _lib.load().mtm_debug_window_stats_route(None, None) == -1


def test_zz_report():
    """What the sweep covered (run the file with -s to read it)."""
    print("stats routes sweep: %d cells; slowest %.3f s: %s; worst float-route error / bound %.4f at %s"
          % (CELLS["n"], CELLS["slowest"][0], CELLS["slowest"][1], CELLS["ratio"][0], CELLS["ratio"][1]))
