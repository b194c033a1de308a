"""TemplateMatcher.match_batch / MTM.matchTemplatesBatch on the host layer, no GPU: the engine is the oracle, run per
image behind the batch interface (mtm_find_matches_batch's contract).  Checks that a batch returns what a loop of
match() returns - hits, order, scores, warnings, exceptions - which route it takes, and that the adversarial stacks of
tests/batch_cases.py really break a batch that stacks the images and drops the seam rows afterwards."""
import os
import re
import warnings
import zlib

import numpy as np
import pytest

import batch_cases as C
from helpers import OracleContext

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def mtm():
    import build as mtm_build
    mtm_build.build()
    import MTM
    return MTM


class BatchOracleContext(OracleContext):
    """OracleContext with the batch entry point: the oracle per image.  Records the batch sizes it was given."""

    def __init__(self, hit_dtype, border=None):
        super().__init__(hit_dtype, border)
        self.batches = []

    def find_matches_batch(self, images, mode, thr):
        assert len({(im.shape, im.dtype) for im in images}) == 1
        assert images[0].dtype in (np.uint8, np.uint16)
        self.batches.append(len(images))
        return [self.find_matches_image(im, mode, thr) for im in images]


def _ctx(mtm, border=None):
    return BatchOracleContext(mtm._lib.HIT_DTYPE, border)


def _pair(mtm, lt, **kw):
    """A batch matcher and a per-image matcher, each on its own oracle context."""
    return mtm.TemplateMatcher(lt, context=_ctx(mtm), **kw), mtm.TemplateMatcher(lt, context=_ctx(mtm), **kw)


def _stack(rng, n, shape, dtype=np.uint8, hi=256):
    ims = rng.randint(0, hi, size=(n,) + shape).astype(dtype)
    return ims


def _plant(ims, t, rng):
    for im in ims:
        y = rng.randint(0, im.shape[0] - t.shape[0] + 1)
        x = rng.randint(0, im.shape[1] - t.shape[1] + 1)
        im[y:y + t.shape[0], x:x + t.shape[1]] = t


def _norm(hits):
    return [(h[0], tuple(int(v) for v in h[1]), np.float32(h[2]).tobytes()) for h in hits]


def _assert_same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert _norm(g) == _norm(w)
        assert all(type(h[2]) is np.float32 for h in g)


@pytest.mark.parametrize("kind", ["u8_gray", "u8_rgb", "u16_gray", "mask_m3"])
@pytest.mark.parametrize("n_object", [float("inf"), 1, 3])
def test_batch_equals_match_loop(mtm, kind, n_object):
    rng = np.random.RandomState(zlib.crc32(("%s %s" % (kind, n_object)).encode()))
    method = 3 if kind == "mask_m3" else 5
    if kind == "u8_rgb":
        ims = _stack(rng, 5, (40, 44, 3))
    elif kind == "u16_gray":
        ims = _stack(rng, 5, (40, 44), np.uint16, 65536)
    else:
        ims = _stack(rng, 5, (40, 44))
    t0 = ims[0, 3:13, 5:14].copy()
    t1 = ims[2, 20:28, 30:41].copy()
    _plant(ims[1:], t0, rng)
    lt = [("a", t0), ("b", t1)]
    if kind == "mask_m3":
        m = np.zeros(t0.shape, np.uint8)
        m[2:8, 1:7] = 1
        lt = [("a", t0, m), ("b", t1)]
    bm, pm = _pair(mtm, lt, method=method, N_object=n_object, score_threshold=0.4)
    got = bm.match_batch(ims)
    assert bm.last_batch_route == "engine" and bm._ctx.batches == [5]
    _assert_same(got, [pm.match(im) for im in ims])


def test_batch_methods_and_borders(mtm):
    rng = np.random.RandomState(7)
    ims = _stack(rng, 4, (36, 36))
    t = ims[1, 4:14, 6:15].copy()
    _plant(ims, t, rng)
    for method in (1, 2, 3, 4, 5):
        for border in ("nearest", "constant"):
            kw = dict(method=method, score_threshold=0.3 if method != 1 else 0.2)
            bm = mtm.TemplateMatcher([("t", t)], context=_ctx(mtm, border), **kw)
            pm = mtm.TemplateMatcher([("t", t)], context=_ctx(mtm, border), **kw)
            _assert_same(bm.match_batch(ims), [pm.match(im) for im in ims])
            assert bm.last_batch_route == "engine"


def test_ndarray_and_sequence_forms(mtm):
    rng = np.random.RandomState(3)
    ims = _stack(rng, 6, (32, 30))
    t = ims[0, 2:10, 3:12].copy()
    _plant(ims, t, rng)
    a, b = _pair(mtm, [("t", t)], score_threshold=0.3)
    got_arr = a.match_batch(ims)
    got_seq = b.match_batch([im for im in ims])
    _assert_same(got_arr, got_seq)
    got_gen = mtm.TemplateMatcher([("t", t)], context=_ctx(mtm), score_threshold=0.3).match_batch(im for im in ims)
    _assert_same(got_gen, got_arr)


def test_routes(mtm):
    rng = np.random.RandomState(5)
    ims = _stack(rng, 3, (30, 30))
    t = ims[0, 2:10, 3:12].copy()
    m, _ = _pair(mtm, [("t", t)])
    assert m.match_batch([]) == [] and m.last_batch_route is None
    assert m.match_batch(np.zeros((0, 30, 30), np.uint8)) == []
    m.match_batch(ims[:1])
    assert m.last_batch_route == "per-image" and m._ctx.batches == []      # one image: match's own route
    m.match_batch(ims)
    assert m.last_batch_route == "engine" and m._ctx.batches == [3]
    m.match_batch([ims[0], ims[1][:, :28], ims[2]])                        # mixed shapes
    assert m.last_batch_route == "per-image" and m._ctx.batches == [3]
    # float32 matching (float32 images, or uint16 with a mask) is never batched
    f = mtm.TemplateMatcher([("t", t.astype(np.float32))], context=_ctx(mtm), score_threshold=0.3)
    f.match_batch(ims.astype(np.float32))
    assert f.last_batch_route == "per-image" and f._ctx.batches == []
    u16 = ims.astype(np.uint16) * 200
    tm = mtm.TemplateMatcher([("t", u16[0, 2:10, 3:12].copy(), np.ones((8, 9), np.uint16))], method=3,
                             context=_ctx(mtm), score_threshold=0.3)
    tm.match_batch(u16)
    assert tm.last_batch_route == "per-image" and tm._ctx.batches == []
    tu = mtm.TemplateMatcher([("t", u16[0, 2:10, 3:12].copy())], context=_ctx(mtm), score_threshold=0.3)
    tu.match_batch(u16)
    assert tu.last_batch_route == "engine" and tu._ctx.batches == [3]


def test_large_maps_go_per_image(mtm, monkeypatch):
    """Images whose score maps exceed the batch's map budget run match per image (the batch writes every map)."""
    rng = np.random.RandomState(6)
    ims = _stack(rng, 3, (30, 30))
    t = ims[0, 2:10, 3:12].copy()
    floats = (30 - 8 + 1) * (30 - 9 + 1)
    monkeypatch.setattr(mtm, "_BATCH_MAP_FLOATS_MAX", floats - 1)
    m = mtm.TemplateMatcher([("t", t)], context=_ctx(mtm), score_threshold=0.3)
    m.match_batch(ims)
    assert m.last_batch_route == "per-image" and m._ctx.batches == []
    monkeypatch.setattr(mtm, "_BATCH_MAP_FLOATS_MAX", floats)
    m.match_batch(ims)
    assert m.last_batch_route == "engine" and m._ctx.batches == [3]


def test_search_box_offsets(mtm):
    rng = np.random.RandomState(11)
    ims = _stack(rng, 4, (50, 60))
    t = ims[0, 20:30, 25:36].copy()
    _plant(ims, t, rng)
    box = (7, 5, 45, 40)
    bm, pm = _pair(mtm, [("t", t)], score_threshold=0.3)
    got = bm.match_batch(ims, searchBox=box)
    assert bm.last_batch_route == "engine"
    want = [pm.match(im, searchBox=box) for im in ims]
    _assert_same(got, want)
    assert any(got) and all(h[1][0] >= 7 and h[1][1] >= 5 for hits in got for h in hits)
    # a box that crops the images to different shapes (images of different sizes): per image, same results
    mixed = [ims[0], ims[1][:42, :50], ims[2]]
    _assert_same(bm.match_batch(mixed, searchBox=box), [pm.match(im, searchBox=box) for im in mixed])
    assert bm.last_batch_route == "per-image"


def test_warnings_once(mtm):
    rng = np.random.RandomState(2)
    ims = _stack(rng, 4, (30, 30))
    t = ims[0, 2:10, 3:12].copy()
    lt = [("a", t, np.ones_like(t)), ("b", t, np.ones_like(t))]        # masks with method 5: ignored, one warning each
    bm, pm = _pair(mtm, lt, score_threshold=0.3)
    with warnings.catch_warnings(record=True) as wb:
        warnings.simplefilter("always")
        bm.match_batch(ims)
    with warnings.catch_warnings(record=True) as wp:
        warnings.simplefilter("always")
        for im in ims:
            pm.match(im)
    assert [str(w.message) for w in wb] == [str(w.message) for w in wp] and len(wb) == 2


def _same_exception(fn_batch, fn_loop):
    with pytest.raises(Exception) as eb:
        fn_batch()
    with pytest.raises(Exception) as el:
        fn_loop()
    assert type(eb.value) is type(el.value) and str(eb.value) == str(el.value)
    return eb.value


def test_exceptions_match_the_loop(mtm):
    rng = np.random.RandomState(4)
    ims = _stack(rng, 3, (30, 30))
    t = ims[0, 2:10, 3:12].copy()
    # TM_SQDIFF: matchTemplates' ValueError, after the search
    bm, pm = _pair(mtm, [("t", t)], method=0)
    e = _same_exception(lambda: bm.match_batch(ims), lambda: [pm.match(im) for im in ims])
    assert isinstance(e, ValueError) and "TM_SQDIFF" in str(e)
    # a template larger than an image / the searchBox
    bm, pm = _pair(mtm, [("big", np.zeros((31, 5), np.uint8))])
    e = _same_exception(lambda: bm.match_batch(ims), lambda: [pm.match(im) for im in ims])
    assert isinstance(e, ValueError) and "larger than image" in str(e)
    bm, pm = _pair(mtm, [("t", t)])
    e = _same_exception(lambda: bm.match_batch(ims, searchBox=(0, 0, 6, 30)),
                        lambda: [pm.match(im, searchBox=(0, 0, 6, 30)) for im in ims])
    assert "larger than searchBox" in str(e)
    # float64, a 64-bit image in the middle of the batch
    bm, pm = _pair(mtm, [("t", t)])
    bad = [ims[0], ims[1].astype(np.float64), ims[2]]
    _same_exception(lambda: bm.match_batch(bad), lambda: [pm.match(im) for im in bad])
    # pixel type that differs from the resident templates
    bm, pm = _pair(mtm, [("t", t)])
    bad = [ims[0], ims[1].astype(np.uint16)]
    _same_exception(lambda: bm.match_batch(bad), lambda: [pm.match(im) for im in bad])
    # N_object that is no integer, an empty image
    with pytest.raises(TypeError):
        mtm.TemplateMatcher([("t", t)], N_object=2.5, context=_ctx(mtm))
    bm, pm = _pair(mtm, [("t", t)])
    bad = [ims[0], ims[1][0:0]]
    _same_exception(lambda: bm.match_batch(bad), lambda: [pm.match(im) for im in bad])


def test_match_templates_batch(mtm):
    assert "matchTemplatesBatch" in mtm.__all__
    rng = np.random.RandomState(9)
    ims = _stack(rng, 4, (40, 40))
    t = ims[3, 10:22, 5:16].copy()
    _plant(ims, t, rng)
    lt = [("t", t)]
    for n_object in (float("inf"), 1, 2):
        ctx = _ctx(mtm)
        got = mtm.matchTemplatesBatch(lt, ims, method=5, N_object=n_object, score_threshold=0.3, context=ctx)
        assert ctx.batches == [4]
        want = [mtm.TemplateMatcher(lt, N_object=n_object, score_threshold=0.3, context=_ctx(mtm)).match(im) for im in ims]
        _assert_same(got, want)


@pytest.mark.parametrize("case", C.ADVERSARIAL, ids=[c[0] for c in C.ADVERSARIAL])
@pytest.mark.parametrize("border", ["nearest", "constant"])
def test_adversarial_stacks_break_the_naive_batch(case, border):
    """The GPU seam tests have teeth: stacking and dropping seam-row hits afterwards gets every one of these stacks wrong."""
    _, build, method, n_object, thr = case
    ims, t = build()
    truth = C.per_image_raw(ims, t, method, n_object, thr, border)
    naive = C.naive_batch_raw(ims, t, method, n_object, thr, border)
    assert truth != naive
    assert any(truth)


def test_abi_declares_the_batch_entry(mtm):
    lib = mtm._lib
    hdr = open(os.path.join(ROOT, "include", "mtm_hip.h")).read()
    assert re.search(r"int mtm_find_matches_batch\(", hdr) and "mtm_find_matches_batch" in lib.SYMBOLS
    assert re.search(r"#define MTM_OPT_BATCH_MAX_ROWS 8\b", hdr) and lib.OPT_BATCH_MAX_ROWS == 8
    assert lib.OPT_BATCH_MAX_ROWS in lib.ALL_OPTIONS
    # the chunk bound keeps every stacked map row inside the 21-bit row field of the candidate key and 16-bit grid rows
    assert 0 < lib.BATCH_MAX_ROWS < 2 ** 21 and lib.BATCH_MAX_ROWS <= 65535
    src = open(os.path.join(ROOT, "multitemplatematching-python_amd", "csrc", "mtm_ctx.h")).read()
    assert re.search(r"constexpr int kBatchMaxRows = %d;" % lib.BATCH_MAX_ROWS, src)
