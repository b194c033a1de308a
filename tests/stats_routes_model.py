"""The six window-statistics kernel chains next to the fused single-channel uint8 one (csrc/mtm_stats_route.h, the launchers of
csrc/mtm_stats.hip, the kernels of csrc/mtm_k_stats.hip.h) restated in numpy, bit for bit - tests/stats_model.py does the same
for the seventh.

The library is built with -ffp-contract=off and the device's float64 sqrt is correctly rounded, so every plane is a fixed
sequence of IEEE operations and is compared with `==` on the bytes:
  integer routes (U8MC, U16, U8_2P, U8_2P_WIDE - and F64_LDS / F64 on integer-valued pixels): every window sum is an exact
    integer below 2^53, taken from int64 integral images (`integer_stats`);
  float route (F64_LDS / F64 on general float32 pixels): the kernels' float64 additions in the kernels' order (`replay_stats`),
    and next to it exact window sums with an error bound derived from the number of rounded operations (`exact_sums`).
What a fused route leaves in the pitch columns right of ow are the windows that run into the image's zero padding; the
two-pass routes leave them alone."""
from fractions import Fraction

import numpy as np

import stats_model as M

ROUTES = ("U8", "U8MC", "U16", "U8_2P", "U8_2P_WIDE", "F64_LDS", "F64")
U8, U8MC, U16, U8_2P, U8_2P_WIDE, F64_LDS, F64 = range(7)
FUSED = (U8, U8MC, U16)
HSUM_SEG = 16                   # kHsumSeg: output columns a thread of the row-sum kernels slides over
VSUM_BAND = 32                  # kVsumBand: output rows a thread of vsum_stats_kernel slides over
UNIT_ROWS = M.UNIT_ROWS


def stats_route(dtype, chans, h, w, cols, fuse_stats=True):
    """csrc/mtm_stats_route.h, restated from the kernels' preconditions (not from its text): the fused kernels hold a
    strip's prefix sums in uint32 - every window sum they form must stay below 2^32 - and >= 256 output columns of a
    1024-column strip; hsum_u8_kernel holds 2 (cols + 1) words in 64 KB; hsum_lds_kernel a row stretch of 4096 + w floats."""
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        for ch, route in ((1, U8), (3, U8MC)):
            if fuse_stats and chans == ch and w <= 768 and ch * w * h * 255 * 255 < 2 ** 32:
                return route
        return U8_2P if 2 * (cols + 1) * 4 <= 65536 else U8_2P_WIDE
    if dtype == np.uint16 and fuse_stats and chans == 1 and w <= 768 and w * h * 65535 < 2 ** 32:
        return U16
    return F64_LDS if w <= 1024 else F64


def _planes(image):
    image = np.asarray(image)
    return image[:, :, None] if image.ndim == 2 else image


def _blocks(v, ow, bp, fill, reduce):
    oh = v.shape[0]
    full = np.full((oh, bp * 16), fill, dtype=v.dtype)
    full[:, :ow] = v[:, :ow]
    return reduce(full.reshape(oh, bp, 16), axis=2)


def _finish(t, s2c, h, w, num_type):
    """The float64 statistics every route ends with, from the per-channel window sums t (chans, oh, n) and sums of squares
    s2c (chans, oh, n) as float64: mean2 = (sum_c t_c t_c) inv_area and sum2 = sum_c s2_c, each added up from 0.0 in channel
    order, then window_norm."""
    inv_area = 1.0 / (float(h) * float(w))
    mean2, sum2 = np.zeros_like(t[0]), np.zeros_like(t[0])
    for c in range(t.shape[0]):
        if num_type == 1:
            mean2 = mean2 + t[c] * t[c]
        sum2 = sum2 + s2c[c]
    mean2 = mean2 * inv_area
    return sum2, M.window_norm(sum2, mean2)


def integer_stats(image, h, w, num_type, route):
    """Integer-valued pixels ((rows, cols) or (rows, cols, chans), any dtype) -> dict(t (chans, oh, st_pitch), sum2, sq (oh,
    st_pitch) float64, blk (oh, blk_pitch, 4), cover (oh, st_pitch) bool: the cells the route writes)."""
    px = _planes(image)
    assert np.array_equal(px, np.floor(px)) and px.min(initial=0) >= 0
    rows, cols, chans = px.shape
    g = M.geometry(rows, cols, h, w)
    oh, ow, sp, bp = g["oh"], g["ow"], g["st_pitch"], g["blk_pitch"]
    a = np.zeros((chans, rows, sp + w), dtype=np.int64)
    a[:, :, :cols] = np.moveaxis(px, 2, 0).astype(np.int64)
    s1 = np.stack([M._box_sums(a[c], 0, h, w, sp) for c in range(chans)])
    s2 = np.stack([M._box_sums(a[c] * a[c], 0, h, w, sp) for c in range(chans)])
    assert s1.shape == (chans, oh, sp)
    # int64 holds every sum (256 x 256 windows of 65535: 2.8e14), float64 holds them exactly; t t is one rounded float64
    # product here as in the kernels
    assert int(s2.sum(axis=0).max(initial=0)) < 2 ** 53 and int(s1.max(initial=0)) < 2 ** 53
    if route in FUSED:          # what the uint32 prefixes must hold
        assert int(s1.max(initial=0)) < 2 ** 32
        assert route == U16 or int(s2.sum(axis=0).max(initial=0)) < 2 ** 32
    t = s1.astype(np.float64)
    if route in FUSED:          # the squares of all channels are added as integers
        s2c = s2.sum(axis=0, keepdims=True).astype(np.float64)
        sum2, sq = _finish(t, np.concatenate([s2c, np.zeros((chans - 1,) + s2c.shape[1:])]), h, w, num_type)
    else:
        sum2, sq = _finish(t, s2.astype(np.float64), h, w, num_type)
    cover = np.zeros((oh, sp), dtype=bool)
    cover[:, :sp if route in FUSED else ow] = True
    big = np.iinfo(np.int64).max
    lo = _blocks(s1[0], ow, bp, big, np.min)
    blk = np.zeros((oh, bp, 4), dtype=np.float64)
    blk[:, :, 0] = np.where(lo == big, 0, lo).astype(np.float64)
    blk[:, :, 1] = _blocks(s1[0], ow, bp, 0, np.max).astype(np.float64)
    blk[:, :, 2] = _blocks(sq, ow, bp, np.inf, np.min)
    return {"t": t, "sum2": sum2, "sq": sq, "blk": blk, "cover": cover}


def _hsum_replay(plane, w, ow):
    """hsum_kernel<double> / hsum_lds_kernel on one float32 plane (rows, cols): a thread owns HSUM_SEG output columns - the
    sequential sum of the first window's w taps, then slides s1 += vn - vo, s2 += vn vn - vo vo.  -> hs1, hs2 (rows, ow)
    float64 and the number of rounded additions behind each column."""
    rows, cols = plane.shape
    nseg = (ow + HSUM_SEG - 1) // HSUM_SEG
    v = np.zeros((rows, nseg * HSUM_SEG + w + 1), dtype=np.float64)
    v[:, :cols] = plane.astype(np.float64)
    x0 = np.arange(nseg) * HSUM_SEG
    s1, s2 = np.zeros((rows, nseg)), np.zeros((rows, nseg))
    for dx in range(w):
        t = v[:, x0 + dx]
        s1 = s1 + t
        s2 = s2 + t * t
    hs1, hs2 = np.zeros((rows, nseg * HSUM_SEG)), np.zeros((rows, nseg * HSUM_SEG))
    for k in range(HSUM_SEG):
        hs1[:, x0 + k], hs2[:, x0 + k] = s1, s2
        vn, vo = v[:, x0 + k + w], v[:, x0 + k]
        s1 = s1 + (vn - vo)
        s2 = s2 + (vn * vn - vo * vo)
    n_ops = w + 2 * (np.arange(ow) % HSUM_SEG)
    return hs1[:, :ow], hs2[:, :ow], n_ops


def _vsum_replay(hs, h, oh):
    """vsum_stats_kernel<double, double> on one plane of row sums: bands of VSUM_BAND output rows - the sequential sum of the
    first window's h rows, then slides s += n - o."""
    out = np.zeros((oh, hs.shape[1]))
    for y0 in range(0, oh, VSUM_BAND):
        s = np.zeros(hs.shape[1])
        for d in range(h):
            s = s + hs[y0 + d]
        for y in range(y0, min(y0 + VSUM_BAND, oh)):
            out[y] = s
            if y + 1 < min(y0 + VSUM_BAND, oh):
                s = s + (hs[y + h] - hs[y])
    return out


def replay_stats(image, h, w, num_type):
    """F64_LDS / F64 on float32 pixels -> dict as integer_stats (no blk), plus n_ops (oh, ow): rounded additions behind a
    channel's window sum."""
    px = _planes(image)
    assert px.dtype == np.float32
    rows, cols, chans = px.shape
    g = M.geometry(rows, cols, h, w)
    oh, ow, sp = g["oh"], g["ow"], g["st_pitch"]
    t, s2c = np.zeros((chans, oh, sp)), np.zeros((chans, oh, sp))
    for c in range(chans):
        hs1, hs2, n_h = _hsum_replay(px[:, :, c], w, ow)
        t[c, :, :ow], s2c[c, :, :ow] = _vsum_replay(hs1, h, oh), _vsum_replay(hs2, h, oh)
    sum2, sq = _finish(t, s2c, h, w, num_type)
    cover = np.zeros((oh, sp), dtype=bool)
    cover[:, :ow] = True
    n_ops = n_h[None, :] + (h + 2 * (np.arange(oh) % VSUM_BAND))[:, None]
    return {"t": t, "sum2": sum2, "sq": sq, "cover": cover, "n_ops": n_ops}


def exact_sums(image, h, w):
    """Exact window sums of float32 pixels (every float is an integer multiple of a common power of two: Python integers) and
    the bound on what replay_stats / the kernels may differ from them by.

    A window sum at output (y, x) is n_ops = w + 2 (x % 16) + h + 2 (y % 32) rounded float64 additions (the products v v of
    float32 values are exact in float64) over the pixels of image rows [y - y % 32, y + h) and columns [x - x % 16, x + w):
    the windows the thread slid over on its way.  Every partial result is at most T = the sum of |terms| over that region in
    magnitude (to first order), so the accumulated error is at most n_ops u T / (1 - n_ops u), u = 2^-53 (Higham, Accuracy and
    Stability of Numerical Algorithms, 4.2, with the intermediate sums bounded by T).
    -> s1, s2 (chans, oh, ow) object arrays of Fraction; bound1, bound2 (chans, oh, ow) float64; n_ops (oh, ow)."""
    px = _planes(image)
    assert px.dtype == np.float32
    rows, cols, chans = px.shape
    oh, ow = rows - h + 1, cols - w + 1
    mant, expo = np.frexp(px.astype(np.float64))
    nz = px != 0
    e_min = int(expo[nz].min()) - 24 if nz.any() else 0
    ints = np.vectorize(lambda m, e: int(m * 2 ** 24) << (int(e) - 24 - e_min) if m else 0, otypes=[object])(mant, expo)
    assert all(Fraction(int(i)) * Fraction(2) ** e_min == Fraction(float(p)) for i, p in zip(ints.ravel()[:64], px.ravel()[:64]))

    def ii(a):
        out = np.zeros((a.shape[0] + 1, a.shape[1] + 1), dtype=object)
        out[1:, 1:] = np.cumsum(np.cumsum(a, axis=0), axis=1)
        return out

    def box(i2, r0, r1, c0, c1):        # sums over rows [r0, r1) x columns [c0, c1), index arrays broadcast
        return i2[r1, c1] - i2[r0, c1] - i2[r1, c0] + i2[r0, c0]

    ys, xs = np.arange(oh)[:, None], np.arange(ow)[None, :]
    yb, xb = ys - ys % VSUM_BAND, xs - xs % HSUM_SEG
    n_ops = (w + 2 * (xs % HSUM_SEG)) + (h + 2 * (ys % VSUM_BAND))
    s1, s2 = np.zeros((chans, oh, ow), dtype=object), np.zeros((chans, oh, ow), dtype=object)
    b1, b2 = np.zeros((chans, oh, ow)), np.zeros((chans, oh, ow))
    scale1, scale2 = Fraction(2) ** e_min, Fraction(2) ** (2 * e_min)
    for c in range(chans):
        a = ints[:, :, c]
        i1, i2, ia = ii(a), ii(a * a), ii(np.abs(a))
        s1[c] = box(i1, ys, ys + h, xs, xs + w) * scale1
        s2[c] = box(i2, ys, ys + h, xs, xs + w) * scale2
        t1 = (box(ia, yb, ys + h, xb, xs + w) * scale1).astype(np.float64)
        t2 = (box(i2, yb, ys + h, xb, xs + w) * scale2).astype(np.float64)
        gamma = n_ops * 2.0 ** -53 / (1.0 - n_ops * 2.0 ** -53)
        b1[c], b2[c] = gamma * t1 * (1 + 2.0 ** -50), gamma * t2 * (1 + 2.0 ** -50)     # (T itself was rounded to float64 once)
    return s1, s2, b1, b2, n_ops


FLOAT_KINDS = ("u16_valued", "normal_0_40", "normal_1000_5", "nine_decades", "negative", "zeros", "constant", "huge_pixel")


def float_data(kind, rows, cols, chans=1, seed=0):
    """The float32 contents the float route is held to (tests/test_gpu_stats_routes.py and the CPU checks of the bound)."""
    rng = np.random.default_rng(seed * 1000 + FLOAT_KINDS.index(kind))
    shape = (rows, cols) if chans == 1 else (rows, cols, chans)
    if kind == "u16_valued":
        a = rng.integers(0, 65536, shape).astype(np.float64)
    elif kind == "normal_0_40":
        a = rng.normal(0.0, 40.0, shape)
    elif kind == "normal_1000_5":           # cancellation in the slides
        a = rng.normal(1000.0, 5.0, shape)
    elif kind == "nine_decades":
        a = 10.0 ** rng.uniform(-4.0, 5.0, shape) * rng.choice([-1.0, 1.0], shape)
    elif kind == "negative":
        a = -np.abs(rng.normal(300.0, 100.0, shape))
    elif kind == "zeros":
        a = np.zeros(shape)
    elif kind == "constant":                # the flat-window guard
        a = np.full(shape, 123.456)
    else:                                   # one huge pixel enters and leaves the slides
        a = rng.normal(0.0, 1.0, shape)
        a[(rows // 2, cols // 2) + ((0,) if chans > 1 else ())] = 3.0e9
    return a.astype(np.float32)


def error_ratio(got, exact, bound):
    """max over cells of |got - exact| / bound (0 / 0 = 0), and where: exact arithmetic."""
    worst, at = 0.0, None
    for idx in np.ndindex(got.shape):
        err = abs(Fraction(float(got[idx])) - exact[idx])
        if err == 0:
            continue
        r = float(err / Fraction(float(bound[idx]))) if bound[idx] > 0 else np.inf
        if r > worst:
            worst, at = r, idx
    return worst, at
