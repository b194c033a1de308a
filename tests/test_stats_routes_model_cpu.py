"""tests/stats_routes_model.py - the numpy restatement tests/test_gpu_stats_routes.py holds six window-statistics kernel chains
to - checked itself: each model against a literal loop on tiny shapes, the integer model against the oracle's window sums,
the replay of the float route against exact sums within the derived bound, and the binding's argument block against the
header."""
from fractions import Fraction

import numpy as np
import pytest

import mtm_oracle as O
import stats_model as M
import stats_routes_model as R


def _literal_integer(image, h, w, num_type, fused):
    px = R._planes(image)
    rows, cols, chans = px.shape
    g = M.geometry(rows, cols, h, w)
    oh, ow, sp, bp = g["oh"], g["ow"], g["st_pitch"], g["blk_pitch"]
    at = lambda y, x, c: int(px[y, x, c]) if x < cols else 0          # noqa: E731  (the zero padding right of the image)
    t, sum2, sq = np.zeros((chans, oh, sp)), np.zeros((oh, sp)), np.zeros((oh, sp))
    blk = np.zeros((oh, bp, 4))
    blk[:, :, 2] = np.inf
    for y in range(oh):
        for x in range(sp if fused else ow):
            mean2, s2 = 0.0, 0
            for c in range(chans):
                s1 = sum(at(y + dy, x + dx, c) for dy in range(h) for dx in range(w))
                s2 += sum(at(y + dy, x + dx, c) ** 2 for dy in range(h) for dx in range(w))
                t[c, y, x] = s1
                if num_type == 1:
                    mean2 += float(s1) * float(s1)
            mean2 *= 1.0 / (float(h) * float(w))
            d = max(float(s2) - mean2, 0.0)
            sum2[y, x] = s2
            sq[y, x] = 0.0 if d <= min(0.5, (10.0 * M.FLT_EPSILON) * float(s2)) else float(np.sqrt(np.float64(d)))
        for b in range(bp):
            xs = [x for x in range(16 * b, 16 * b + 16) if x < ow]
            if xs:
                blk[y, b] = (min(t[0, y, x] for x in xs), max(t[0, y, x] for x in xs), min(sq[y, x] for x in xs), 0.0)
    return {"t": t, "sum2": sum2, "sq": sq, "blk": blk}


@pytest.mark.parametrize("rows,cols,h,w", [(6, 9, 3, 2), (7, 21, 4, 5), (5, 40, 5, 3), (4, 4, 1, 1), (12, 33, 7, 16), (9, 18, 9, 18)])
@pytest.mark.parametrize("num_type", [0, 1, 2])
@pytest.mark.parametrize("route,dtype,chans", [(R.U8MC, np.uint8, 3), (R.U16, np.uint16, 1), (R.U8_2P, np.uint8, 1),
                                               (R.U8_2P, np.uint8, 2), (R.U8_2P_WIDE, np.uint8, 4), (R.F64_LDS, np.uint16, 3)])
def test_integer_model_is_the_literal_loop(rows, cols, h, w, num_type, route, dtype, chans):
    rng = np.random.default_rng(rows * 100 + cols + num_type + chans)
    top = int(np.iinfo(dtype).max)
    shape = (rows, cols) if chans == 1 else (rows, cols, chans)
    for image in (rng.integers(0, top + 1, shape).astype(dtype), np.full(shape, top, dtype), np.zeros(shape, dtype)):
        got, exp = R.integer_stats(image, h, w, num_type, route), _literal_integer(image, h, w, num_type, route in R.FUSED)
        cov = got["cover"]
        ow = cols - w + 1       # a fused route writes the pitch columns too, a two-pass chain leaves them alone
        assert cov[:, :ow].all() and (cov[:, ow:].all() if route in R.FUSED else not cov[:, ow:].any())
        for k in ("sum2", "sq"):
            assert got[k][cov].tobytes() == exp[k][cov].tobytes(), k
        assert got["t"][:, cov].tobytes() == exp["t"][:, cov].tobytes()
        if chans == 1:
            assert got["blk"].tobytes() == exp["blk"].tobytes()


@pytest.mark.parametrize("dtype,chans,h,w,route", [(np.uint16, 1, 256, 256, R.U16), (np.uint16, 1, 255, 257, R.U16),
                                                   (np.uint8, 3, 86, 256, R.U8MC), (np.uint8, 1, 260, 260, R.U8_2P)])
def test_integer_model_on_saturated_images(dtype, chans, h, w, route):
    """The largest sums of the GPU sweep, in closed form: every window inside the image holds h w pixels of the type's maximum."""
    top = int(np.iinfo(dtype).max)
    image = np.full((h + 2, w + 5) + ((chans,) if chans > 1 else ()), top, dtype)
    for num_type in (0, 1):
        m = R.integer_stats(image, h, w, num_type, route)
        assert (m["t"][:, :, :6] == float(top * h * w)).all() and (m["sum2"][:, :6] == float(chans * top * top * h * w)).all()
        assert (m["sq"][:, :6] == (0.0 if num_type == 1 else np.sqrt(np.float64(chans * top * top * h * w)))).all()


def _literal_replay(image, h, w, num_type):
    """hsum_kernel<double> and vsum_stats_kernel<double, double> (csrc/mtm_k_stats.hip.h), line for line, one scalar at a time."""
    px = R._planes(image)
    rows, cols, chans = px.shape
    oh, ow = rows - h + 1, cols - w + 1
    f = np.float64
    hs1, hs2 = np.zeros((chans, rows, ow)), np.zeros((chans, rows, ow))
    for c in range(chans):
        for y in range(rows):
            row = [f(px[y, x, c]) for x in range(cols)] + [f(0.0)] * 17
            for x0 in range(0, ow, R.HSUM_SEG):
                s1, s2 = f(0.0), f(0.0)
                for dx in range(w):
                    v = row[x0 + dx]
                    s1 = s1 + v
                    s2 = s2 + v * v
                for k in range(R.HSUM_SEG):
                    x = x0 + k
                    if x >= ow:
                        break
                    hs1[c, y, x], hs2[c, y, x] = s1, s2
                    vn, vo = row[x + w], row[x]
                    s1 = s1 + (vn - vo)
                    s2 = s2 + (vn * vn - vo * vo)
    t, sum2, sq = np.zeros((chans, oh, ow)), np.zeros((oh, ow)), np.zeros((oh, ow))
    inv_area = f(1.0) / (f(h) * f(w))
    for x in range(ow):
        for y0 in range(0, oh, R.VSUM_BAND):
            s1, s2 = [f(0.0)] * chans, [f(0.0)] * chans
            for c in range(chans):
                for d in range(h):
                    s1[c] = s1[c] + hs1[c, y0 + d, x]
                    s2[c] = s2[c] + hs2[c, y0 + d, x]
            y1 = min(y0 + R.VSUM_BAND, oh)
            for y in range(y0, y1):
                mean2, ws2 = f(0.0), f(0.0)
                for c in range(chans):
                    if num_type == 1:
                        mean2 = mean2 + s1[c] * s1[c]
                    t[c, y, x] = s1[c]
                    ws2 = ws2 + s2[c]
                mean2 = mean2 * inv_area
                sum2[y, x] = ws2
                sq[y, x] = M.window_norm(np.float64(ws2), np.float64(mean2))
                if y + 1 < y1:
                    for c in range(chans):
                        s1[c] = s1[c] + (hs1[c, y + h, x] - hs1[c, y, x])
                        s2[c] = s2[c] + (hs2[c, y + h, x] - hs2[c, y, x])
    return {"t": t, "sum2": sum2, "sq": sq}


@pytest.mark.parametrize("rows,cols,h,w,chans", [(6, 9, 3, 2, 1), (36, 21, 2, 5, 2), (5, 40, 5, 3, 3), (40, 35, 7, 17, 4), (4, 4, 1, 1, 1)])
@pytest.mark.parametrize("kind", ["normal_1000_5", "nine_decades", "huge_pixel", "constant"])
def test_replay_is_the_literal_loop(rows, cols, h, w, chans, kind):
    image = R.float_data(kind, rows, cols, chans, seed=rows + cols)
    for num_type in (0, 1):
        got, exp = R.replay_stats(image, h, w, num_type), _literal_replay(image, h, w, num_type)
        ow = cols - w + 1
        for k in ("sum2", "sq"):
            assert got[k][:, :ow].tobytes() == exp[k].tobytes(), k
        assert got["t"][:, :, :ow].tobytes() == exp["t"].tobytes()


def test_replay_on_integers_is_the_integer_model():
    """Where every partial sum is an exact integer the order of the additions cannot show."""
    image = R.float_data("u16_valued", 50, 60, 2, seed=3)
    got, exp = R.replay_stats(image, 9, 17, 1), R.integer_stats(image, 9, 17, 1, R.F64_LDS)
    for k in ("t", "sum2", "sq"):
        assert got[k][..., :44].tobytes() == exp[k][..., :44].tobytes(), k


@pytest.mark.parametrize("rows,cols,h,w", [(40, 70, 8, 16), (33, 129, 17, 64), (64, 64, 64, 64)])
def test_integer_model_against_the_oracle(rows, cols, h, w):
    """The oracle's window sums (float64 integral images: exact at these sizes), per channel and for the squares of all."""
    rng = np.random.default_rng(rows + cols)
    image = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    ow = cols - w + 1
    f = image.astype(np.float64)
    for route in (R.U8MC, R.U8_2P):
        m = R.integer_stats(image, h, w, 1, route)
        for c in range(3):
            assert np.array_equal(m["t"][c, :, :ow], O.window_sums(f[:, :, c], h, w))
        assert np.array_equal(m["sum2"][:, :ow], O.window_sums((f * f).sum(axis=2), h, w))
    u16 = rng.integers(0, 65536, (rows, cols)).astype(np.uint16)
    m = R.integer_stats(u16, h, w, 1, R.U16)
    assert np.array_equal(m["t"][0, :, :ow], O.window_sums(u16.astype(np.float64), h, w))
    assert np.array_equal(m["sum2"][:, :ow], O.window_sums(u16.astype(np.float64) ** 2, h, w))


@pytest.mark.parametrize("kind", R.FLOAT_KINDS)
@pytest.mark.parametrize("rows,cols,h,w,chans", [(70, 50, 5, 17, 1), (40, 40, 33, 3, 2)])
def test_replay_stays_inside_the_bound(kind, rows, cols, h, w, chans):
    """The kernels' order of additions against exact window sums: within n_ops u T / (1 - n_ops u) on every content the GPU
    sweep uses - the bound is derived (stats_routes_model.exact_sums), and the float route is held to the replay's bytes."""
    image = R.float_data(kind, rows, cols, chans, seed=1)
    rep = R.replay_stats(image, h, w, 0)
    s1, s2, b1, b2, n_ops = R.exact_sums(image, h, w)
    ow = cols - w + 1
    assert np.array_equal(n_ops, rep["n_ops"])
    for c in range(chans):
        r1, at1 = R.error_ratio(rep["t"][c, :, :ow], s1[c], b1[c])
        assert r1 <= 1.0, (kind, "S1", c, r1, at1)
    if chans == 1:          # (the sum2 plane of several channels is their sum: one more addition each, not part of this bound)
        r2, at2 = R.error_ratio(rep["sum2"][:, :ow], s2[0], b2[0])
        assert r2 <= 1.0, (kind, "S2", r2, at2)
    if kind in ("u16_valued", "zeros"):
        assert all(Fraction(float(v)) == e for v, e in zip(rep["t"][0, :, :ow].ravel(), s1[0].ravel()))


def test_route_rule():
    assert R.stats_route(np.uint8, 1, 86, 768, 900) == R.U8 and R.stats_route(np.uint8, 1, 87, 768, 900) == R.U8_2P
    assert R.stats_route(np.uint8, 3, 28, 768, 900) == R.U8MC and R.stats_route(np.uint8, 3, 29, 768, 900) == R.U8_2P
    assert R.stats_route(np.uint8, 3, 86, 256, 900) == R.U8MC and R.stats_route(np.uint8, 3, 87, 256, 900) == R.U8_2P
    assert R.stats_route(np.uint8, 3, 8, 769, 900) == R.U8_2P and R.stats_route(np.uint8, 2, 8, 8, 8191) == R.U8_2P
    assert R.stats_route(np.uint8, 2, 8, 8, 8192) == R.U8_2P_WIDE and R.stats_route(np.uint8, 1, 8, 8, 900, False) == R.U8_2P
    assert R.stats_route(np.uint16, 1, 256, 256, 900) == R.U16 and R.stats_route(np.uint16, 1, 255, 257, 900) == R.U16
    assert R.stats_route(np.uint16, 1, 256, 257, 900) == R.F64_LDS and R.stats_route(np.uint16, 2, 8, 8, 900) == R.F64_LDS
    assert R.stats_route(np.float32, 1, 8, 1024, 2000) == R.F64_LDS and R.stats_route(np.float32, 1, 8, 1025, 2000) == R.F64


def test_window_stats_route_block_matches_the_header():
    """mtm_debug_window_stats_route (test support): the binding's argument block has the header's fields in the header's
    order, the route numbers are the header's, and the entry point refuses null arguments without a GPU."""
    import ctypes
    import os
    import re
    import build as mtm_build
    mtm_build.build()
    from MTM import _lib
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "mtm_hip.h")).read()
    body = hdr[hdr.index("typedef struct mtm_window_stats_route {"):hdr.index("} mtm_window_stats_route;")]
    fields = [f for line in body.splitlines()[1:] for f in re.findall(r"\b([a-z_0-9]+)\s*[,;]", line)]
    assert fields == [f[0] for f in _lib.MtmWindowStatsRoute._fields_], fields
    assert ctypes.sizeof(_lib.MtmWindowStatsRoute) == 14 * 4 + 9 * 8
    routes = dict(re.findall(r"#define\s+MTM_STATS_ROUTE_([A-Z0-9_]+)\s+(\d+)", hdr))
    assert [int(routes[name]) for name in _lib.STATS_ROUTES] == list(range(7)) and _lib.STATS_ROUTES == R.ROUTES
    src = open(os.path.join(os.path.dirname(mtm_build.__file__), "csrc", "mtm_stats_route.h")).read()
    enum = re.findall(r"kStatsRoute(\w+) = (\d+)", src)
    assert [int(v) for _, v in enum] == list(range(8)) and enum[-1][0] == "Count"
    assert len(_lib.STATS_ROUTE_INFO_FIELDS) == 12 and "info[12]" in hdr
    assert "mtm_debug_window_stats_route" in hdr[hdr.index("Bumped when"):hdr.index("#define MTM_ABI_VERSION")]
    assert _lib.load().mtm_debug_window_stats_route(None, None) == -1
    assert b"mtm_debug_window_stats_route" in _lib.load().mtm_last_error()
