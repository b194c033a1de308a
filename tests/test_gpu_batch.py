"""TemplateMatcher.match_batch on the MI355X (mtm_find_matches_batch: the images stacked into one tall image, one chain of
launches, seam-aware peaks and per-image extrema) against a loop of match() on a context of the same configuration -
exact equality of hits, order and float32 scores."""
import zlib

import numpy as np
import pytest

import batch_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mtm():
    import build as mtm_build
    mtm_build.build()
    import MTM
    return MTM


@pytest.fixture(scope="module")
def ctxs(mtm):
    """(batch context, per-image context); every test sets the options it depends on and puts them back."""
    a, b = mtm._lib.Context(0), mtm._lib.Context(0)
    yield a, b
    a.close()
    b.close()


def _norm(hits):
    return [(h[0], tuple(int(v) for v in h[1]), np.float32(h[2]).tobytes()) for h in hits]


def _compare(mtm, ctxs, lt, ims, border=None, search_box=None, route="engine", **kw):
    ca, cb = ctxs
    bd = mtm._lib.BORDER_CONSTANT if border == "constant" else mtm._lib.BORDER_NEAREST
    for c in (ca, cb):
        c.set_option(mtm._lib.OPT_PEAK_BORDER, bd)
    try:
        bm = mtm.TemplateMatcher(lt, context=ca, **kw)
        pm = mtm.TemplateMatcher(lt, context=cb, **kw)
        got = bm.match_batch(ims, searchBox=search_box)
        if route:
            assert bm.last_batch_route == route
        if bm.last_batch_route == "engine":
            assert ca.timing()["f32_route"] == 0
        want = [pm.match(im, searchBox=search_box) for im in ims]
    finally:
        for c in (ca, cb):
            c.set_option(mtm._lib.OPT_PEAK_BORDER, mtm._lib.BORDER_NEAREST)
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert _norm(g) == _norm(w), b
    return got


def _stack(rng, n, shape, dtype=np.uint8, hi=256):
    return rng.randint(0, hi, size=(n,) + shape).astype(dtype)


def _plant(ims, t, rng):
    for im in ims:
        y = rng.randint(0, im.shape[0] - t.shape[0] + 1)
        x = rng.randint(0, im.shape[1] - t.shape[1] + 1)
        im[y:y + t.shape[0], x:x + t.shape[1]] = t


def _case(kind, n, rng):
    """(template list, images, matcher kwargs) of one pixel kind."""
    if kind == "u8_rgb":
        ims = _stack(rng, n, (56, 60, 3))
    elif kind == "u16_gray":
        ims = _stack(rng, n, (56, 60), np.uint16, 65536)
    elif kind == "slabs":
        ims = _stack(rng, n, (40, 300))
    else:
        ims = _stack(rng, n, (56, 60))
    if kind == "slabs":        # wider than one matrix-core launch takes: cut into slabs
        t0, t1 = ims[0, 2:14, 5:290].copy(), ims[n - 1, 20:30, 0:270].copy()
    else:
        t0, t1 = ims[0, 3:15, 5:16].copy(), ims[n - 1, 30:40, 40:52].copy()
    _plant(ims[1:], t0, rng)
    lt = [("a", t0), ("b", t1)]
    kw = dict(method=5, score_threshold=0.4)
    if kind in ("mask_m3", "mask_m0"):
        m = np.zeros(t0.shape, np.uint8)
        m[2:10, 1:9] = 1
        lt = [("a", t0, m), ("b", t1, np.ones(t1.shape, np.uint8))]
        kw = dict(method=3, score_threshold=0.4) if kind == "mask_m3" else dict(method=0, score_threshold=1e6)
    return lt, ims, kw


@pytest.mark.parametrize("kind", ["u8_gray", "u8_rgb", "u16_gray", "mask_m3", "slabs"])
@pytest.mark.parametrize("n_object", [float("inf"), 1, 3])
def test_batch_kinds(mtm, ctxs, kind, n_object):
    rng = np.random.RandomState(zlib.crc32(("%s %s" % (kind, n_object)).encode()))
    lt, ims, kw = _case(kind, 7, rng)
    _compare(mtm, ctxs, lt, ims, N_object=n_object, **kw)


@pytest.mark.parametrize("n_images", [1, 2, 7, 33])
@pytest.mark.parametrize("n_object", [float("inf"), 1, 3])
def test_batch_sizes(mtm, ctxs, n_images, n_object):
    rng = np.random.RandomState(100 + n_images)
    lt, ims, kw = _case("u8_gray", n_images, rng)
    _compare(mtm, ctxs, lt, ims, N_object=n_object, route="engine" if n_images > 1 else "per-image", **kw)


def test_batch_method0_raises_like_match(mtm, ctxs):
    rng = np.random.RandomState(8)
    lt, ims, kw = _case("mask_m0", 4, rng)
    with pytest.raises(ValueError, match="TM_SQDIFF is not supported"):
        mtm.TemplateMatcher(lt, context=ctxs[0], **kw).match_batch(ims)
    with pytest.raises(ValueError, match="TM_SQDIFF is not supported"):
        mtm.TemplateMatcher(lt, context=ctxs[1], **kw).match(ims[0])


@pytest.mark.parametrize("method", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("border", ["nearest", "constant"])
def test_batch_methods_borders(mtm, ctxs, method, border):
    rng = np.random.RandomState(method)
    lt, ims, _ = _case("u8_gray", 7, rng)
    thr = {1: 0.3, 2: 2.0e6, 3: 0.9, 4: 2.0e5, 5: 0.4}[method]
    _compare(mtm, ctxs, lt, ims, border=border, method=method, score_threshold=thr)


def test_batch_search_box(mtm, ctxs):
    rng = np.random.RandomState(21)
    lt, ims, kw = _case("u8_gray", 7, rng)
    got = _compare(mtm, ctxs, lt, ims, search_box=(3, 4, 50, 45), **kw)
    assert any(got)


@pytest.mark.parametrize("case", C.ADVERSARIAL, ids=[c[0] for c in C.ADVERSARIAL])
@pytest.mark.parametrize("border", ["nearest", "constant"])
def test_batch_seam_adversaries(mtm, ctxs, case, border):
    _, build, method, n_object, thr = case
    ims, t = build()
    _compare(mtm, ctxs, [("t", t)], ims, border=border, method=method, N_object=n_object, score_threshold=thr)
    # the engine's raw peaks (before the NMS of match) against the per-image truth of the oracle, by position
    lib = mtm._lib
    ca = ctxs[0]
    ca.set_option(lib.OPT_PEAK_BORDER, lib.BORDER_CONSTANT if border == "constant" else lib.BORDER_NEAREST)
    try:
        ca.set_templates([(t, None)], method)
        raws = ca.find_matches_batch(list(ims), lib.PEAKS_GLOBAL if n_object == 1 else lib.PEAKS_LOCAL, thr)
    finally:
        ca.set_option(lib.OPT_PEAK_BORDER, lib.BORDER_NEAREST)
    truth = C.per_image_raw(ims, t, method, n_object, thr, border)
    assert any(truth)
    for r, tr in zip(raws, truth):
        assert sorted((int(h["y"]), int(h["x"])) for h in r) == sorted((y, x) for y, x, _ in tr)


@pytest.mark.parametrize("n_object", [float("inf"), 1])
def test_batch_line_and_point_maps(mtm, ctxs, n_object):
    rng = np.random.RandomState(31)
    ims = _stack(rng, 5, (24, 40))
    lt = [("rows", ims[0, :, 3:11].copy()), ("cols", ims[1, 2:9, :].copy()), ("all", ims[2].copy()),
          ("2d", ims[3, 5:12, 6:15].copy())]
    _compare(mtm, ctxs, lt, ims, method=5, N_object=n_object, score_threshold=-0.5)
    _compare(mtm, ctxs, lt, ims, method=1, N_object=n_object, score_threshold=1.5)


def test_batch_dense_overflow(mtm, ctxs):
    """A dense stack at a low threshold: thousands of peaks; the hit list overflows its capacity and the peak pass runs
    again with a grown list."""
    rng = np.random.RandomState(71)
    ims = _stack(rng, 9, (96, 96))
    ca = ctxs[0]
    ca.set_option(mtm._lib.OPT_HIT_CAPACITY, 64)
    try:
        _compare(mtm, ctxs, [("t", ims[0, 10:18, 20:28].copy())], ims, score_threshold=-0.99)
        raw_peaks = ca.timing()["n_hits"]
    finally:
        ca.set_option(mtm._lib.OPT_HIT_CAPACITY, 1 << 18)
    assert raw_peaks > 1000


def test_batch_chunking(mtm, ctxs):
    lib = mtm._lib
    ca = ctxs[0]
    assert ca.get_option(lib.OPT_BATCH_MAX_ROWS) == lib.BATCH_MAX_ROWS < 2 ** 21
    rng = np.random.RandomState(41)
    lt, ims, kw = _case("u8_gray", 9, rng)
    for n_object in (float("inf"), 1):
        one = mtm.TemplateMatcher(lt, context=ca, N_object=n_object, **kw).match_batch(ims)
        for rows in (56, 2 * 56 + 1, 5 * 56):
            ca.set_option(lib.OPT_BATCH_MAX_ROWS, rows)
            try:
                chunked = mtm.TemplateMatcher(lt, context=ca, N_object=n_object, **kw).match_batch(ims)
            finally:
                ca.set_option(lib.OPT_BATCH_MAX_ROWS, lib.BATCH_MAX_ROWS)
            assert [_norm(g) for g in chunked] == [_norm(g) for g in one]
    with pytest.raises(lib.MtmError):
        ca.set_option(lib.OPT_BATCH_MAX_ROWS, 2 ** 21)


def test_batch_route_proof(mtm, ctxs):
    """One chain of launches: the score launches of a batch of 33 512x512 images are as many as those of 2 - a loop of
    per-image calls could not do that."""
    rng = np.random.RandomState(51)
    ims = _stack(rng, 33, (512, 512))
    t = ims[4, 100:132, 200:232].copy()
    _plant(ims, t, rng)
    ca = ctxs[0]
    m = mtm.TemplateMatcher([("t", t), ("u", ims[9, 10:42, 10:42].copy())], context=ca, score_threshold=0.6)
    m.match_batch(ims[:2])
    assert m.last_batch_route == "engine"
    two = ca.timing()["ncc_launches"]
    got = m.match_batch(ims)
    assert m.last_batch_route == "engine"
    tm = ca.timing()
    assert tm["ncc_launches"] == two > 0 and tm["f32_route"] == 0
    assert all(any(h[0] == "t" for h in g) for g in got)
    f = mtm.TemplateMatcher([("t", t.astype(np.float32))], context=ca, score_threshold=0.6)
    f.match_batch(ims[:3].astype(np.float32))
    assert f.last_batch_route == "per-image"


def test_batch_context_hygiene(mtm, ctxs):
    lib = mtm._lib
    ca = ctxs[0]
    rng = np.random.RandomState(61)
    lt, ims, kw = _case("u8_gray", 5, rng)
    m = mtm.TemplateMatcher(lt, context=ca, **kw)
    m.match_batch(ims)
    with pytest.raises(lib.MtmError, match="-4"):       # no current image after a batch
        ca.find_matches(lib.PEAKS_LOCAL, 0.4)
    after = m.match(ims[2])
    fresh = lib.Context(0)
    try:
        want = mtm.TemplateMatcher(lt, context=fresh, **kw).match(ims[2])
    finally:
        fresh.close()
    assert _norm(after) == _norm(want)


def test_batch_abi_direct(mtm, ctxs):
    lib = mtm._lib
    ca, cb = ctxs
    rng = np.random.RandomState(71)
    ims = _stack(rng, 3, (40, 48))
    t = ims[1, 5:15, 7:19].copy()
    for c in (ca, cb):
        c.set_templates([(t, None)], 5)
    one = ca.find_matches_batch([ims[1]], lib.PEAKS_LOCAL, 0.3)
    assert _raw(one[0]) == _raw(cb.find_matches_image(ims[1], lib.PEAKS_LOCAL, 0.3))
    # a cropped view per image (one row stride, no host copy), coordinates in each crop's frame
    views = [im[3:37, 2:44] for im in ims]
    got = ca.find_matches_batch(views, lib.PEAKS_LOCAL, 0.3)
    for v, g in zip(views, got):
        assert _raw(g) == _raw(cb.find_matches_image(v, lib.PEAKS_LOCAL, 0.3))
    with pytest.raises(lib.MtmError, match="uint8 and uint16"):
        ca.find_matches_batch([im.astype(np.float32) for im in ims], lib.PEAKS_LOCAL, 0.3)


def _raw(a):
    return [tuple(r) for r in a.tolist()]
