"""MTM.hitNeighbourhoods / refineHits / TemplateMatcher.refine on the GPU (mtm_hit_neighbourhoods): uint8 and
uint16 neighbourhoods equal computeScoreMap's maps bit for bit, float32 ones the oracle's maps to rounding; the fit of
refineHits is the numpy fit of those neighbourhoods; hits of every search function pass straight in."""
import warnings

import numpy as np
import pytest

import MTM
import mtm_oracle as O
from MTM import _lib
from MTM.subpixel import fit_offsets

from test_subpixel_cpu import BLOB_SHIFTS, blob_case

pytestmark = pytest.mark.gpu


def _cut(smap, x, y):
    out = np.full((3, 3), np.nan, dtype=np.float32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if 0 <= y + dy < smap.shape[0] and 0 <= x + dx < smap.shape[1]:
                out[1 + dy, 1 + dx] = smap[y + dy, x + dx]
    return out


def _pixels(rng, shape, dtype):
    if dtype == np.uint8:
        return rng.randint(0, 256, size=shape).astype(np.uint8)
    if dtype == np.uint16:
        return rng.randint(0, 65536, size=shape).astype(np.uint16)
    return (rng.rand(*shape) * 255.0).astype(np.float32)


def _scene(seed, dtype, chans, sizes, hw=(70, 150), masked=False):
    """An image, templates cut from it (one per size, some with a mask), and hits at the maps' corners, edges and inside."""
    rng = np.random.RandomState(seed)
    shape = hw if chans == 1 else hw + (chans,)
    img = _pixels(rng, shape, dtype)
    lt, hits = [], []
    for k, (h, w) in enumerate(sizes):
        y0, x0 = rng.randint(0, hw[0] - h + 1), rng.randint(0, hw[1] - w + 1)
        t = img[y0:y0 + h, x0:x0 + w].copy()
        if masked:
            m = (rng.rand(*t.shape) > 0.3).astype(dtype)
            if dtype == np.float32:
                m = (rng.rand(*t.shape) * 2.0).astype(np.float32)
            lt.append(("t%d" % k, t, m))
        else:
            lt.append(("t%d" % k, t))
        oh, ow = hw[0] - h + 1, hw[1] - w + 1
        pts = [(0, 0), (ow - 1, 0), (0, oh - 1), (ow - 1, oh - 1), (ow // 2, 0), (0, oh // 2), (ow - 1, oh // 3),
               (ow // 3, oh - 1), (x0, y0)]
        pts += [(int(rng.randint(0, ow)), int(rng.randint(0, oh))) for _ in range(8)]
        hits += [("t%d" % k, (x, y, w, h), np.float32(0.0)) for x, y in pts]
    return lt, img, hits


def _score_map_cuts(lt, img, hits, method):
    by = {t[0]: t for t in lt}
    maps = {}
    out = []
    for label, (x, y, w, h), _ in hits:
        if label not in maps:
            t = by[label]
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                maps[label] = MTM.computeScoreMap(t[1], img, method, t[2] if len(t) > 2 else None)
        out.append(_cut(maps[label], x, y))
    return np.stack(out)


SIZES = [(7, 9), (16, 64), (20, 70), (3, 130)]      # (chunks: more than 16 rows, more than 64 columns)

EXACT = [("u8", np.uint8, 1, False, range(6)), ("u8 rgb", np.uint8, 3, False, range(6)),
         ("u16", np.uint16, 1, False, range(6)), ("u8 masked", np.uint8, 1, True, (0, 3)),
         ("u8 rgb masked", np.uint8, 3, True, (0, 3))]


@pytest.mark.parametrize("desc,dtype,chans,masked,methods", EXACT, ids=[e[0] for e in EXACT])
def test_integer_neighbourhoods_equal_the_score_maps_bit_for_bit(desc, dtype, chans, masked, methods):
    for method in methods:
        lt, img, hits = _scene(10 + method, dtype, chans, SIZES, masked=masked)
        nb = MTM.hitNeighbourhoods(lt, img, hits, method)
        exp = _score_map_cuts(lt, img, hits, method)
        assert nb.shape == (len(hits), 3, 3) and nb.dtype == np.float32
        bad = ~((nb == exp) | (np.isnan(nb) & np.isnan(exp)))
        assert not bad.any(), (desc, method, np.argwhere(bad)[:5], nb[bad][:5], exp[bad][:5])


FLOAT = [("f32", np.float32, 1, False, range(6), None), ("f32 rgb", np.float32, 3, False, range(6), None),
         ("f32 masked", np.float32, 1, True, (0, 3), None), ("f32 rgb masked", np.float32, 3, True, (0, 3), None),
         ("u16 masked", np.uint16, 1, True, (0, 3), None), ("u8 image, f32 templates", np.float32, 1, False, (3, 5), np.uint8)]


@pytest.mark.parametrize("desc,dtype,chans,masked,methods,img_dtype", FLOAT, ids=[f[0] for f in FLOAT])
def test_float_neighbourhoods_agree_with_the_oracle(desc, dtype, chans, masked, methods, img_dtype):
    for method in methods:
        lt, img, hits = _scene(20 + method, dtype, chans, SIZES, masked=masked)
        if img_dtype is not None:
            img = np.clip(img, 0, 255).astype(img_dtype)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            nb = MTM.hitNeighbourhoods(lt, img, hits, method)
        by = {t[0]: t for t in lt}
        maps = {k: O.compute_score_map(t[1], img, method, t[2] if len(t) > 2 else None) for k, t in by.items()}
        exp = np.stack([_cut(maps[h[0]], h[1][0], h[1][1]) for h in hits])
        assert np.array_equal(np.isnan(nb), np.isnan(exp))
        ok = ~np.isnan(exp)
        err = np.abs(nb[ok].astype(np.float64) - exp[ok]) / np.maximum(1.0, np.abs(exp[ok].astype(np.float64)))
        assert err.max() <= 1e-6, (desc, method, float(err.max()))


@pytest.mark.parametrize("dtype,chans,method", [(np.uint8, 1, 5), (np.uint8, 3, 1), (np.uint16, 1, 0), (np.float32, 1, 3)])
def test_refine_is_the_numpy_fit_of_the_neighbourhoods(dtype, chans, method):
    lt, img, hits = _scene(31, dtype, chans, SIZES)
    nb = MTM.hitNeighbourhoods(lt, img, hits, method)
    ref = MTM.refineHits(lt, img, hits, method)
    ox, oy = fit_offsets(nb, method)
    assert len(ref) == len(hits)
    for r, h, a, b in zip(ref, hits, ox, oy):
        assert r[0] == h[0] and r[2] is h[2]
        xf, yf, w, hh = r[1]
        assert type(xf) is float and type(yf) is float
        assert (xf, yf, w, hh) == (h[1][0] + float(a), h[1][1] + float(b), h[1][2], h[1][3])


def _plant(seed):
    from synth import make_workload
    return make_workload(seed=seed, image_hw=(400, 640), n_base=3, templ=24, rotations=2)


def _check_search_hits(lt, img, hits, method=5):
    assert hits, "the search found nothing to refine"
    nb = MTM.hitNeighbourhoods(lt, img, hits, method)
    exp = _score_map_cuts(lt, img, hits, method)
    assert np.array_equal(nb, exp, equal_nan=True)
    assert np.array_equal(nb[:, 1, 1], np.array([h[2] for h in hits], dtype=np.float32))
    ref = MTM.refineHits(lt, img, hits, method)
    assert all(abs(r[1][0] - h[1][0]) <= 0.5 and abs(r[1][1] - h[1][1]) <= 0.5 for r, h in zip(ref, hits))


def test_hits_of_every_search_function_pass_straight_in():
    img, lt, _ = _plant(3)
    _check_search_hits(lt, img, MTM.matchTemplates(lt, img, score_threshold=0.5, maxOverlap=0.25))
    box = (40, 30, 200, 150)
    _check_search_hits(lt, img, MTM.findMatches(lt, img, score_threshold=0.3, searchBox=box))
    boxes = [(0, 0, 160, 120), (100, 60, 220, 140), (30, 20, 90, 90)]
    per_box = MTM.findMatchesInBoxes(lt, img, boxes, score_threshold=0.3)
    _check_search_hits(lt, img, [h for r in per_box for h in r])
    _check_search_hits(lt, img, MTM.findMatchesPyramid(lt, img, 2, score_threshold=0.4))
    frames = [np.roll(img, (k, 2 * k), axis=(0, 1)) for k in range(3)]
    tracks = [((h[1][0] - 6, h[1][1] - 6, h[1][2] + 12, h[1][3] + 12), [e[0] for e in lt].index(h[0]))
              for h in MTM.matchTemplates(lt, img, score_threshold=0.5, maxOverlap=0.25)[:4]]
    tracks = [((max(0, x), max(0, y), w, h), j) for (x, y, w, h), j in tracks]
    for f, res in zip(frames, MTM.trackTemplates(lt, frames, tracks, margin=4)):
        _check_search_hits(lt, f, [r[0] for r in res])


def test_twenty_thousand_hits_duplicates_and_an_empty_list():
    rng = np.random.RandomState(5)
    img = rng.randint(0, 65536, size=(300, 400)).astype(np.uint16)
    t = img[100:116, 200:216].copy()
    lt = [("a", t)]
    oh, ow = 300 - 16 + 1, 400 - 16 + 1
    xs, ys = rng.randint(0, ow, 20000), rng.randint(0, oh, 20000)
    xs[:50], ys[:50] = 200, 100                     # duplicates
    hits = [("a", (int(x), int(y), 16, 16), np.float32(0)) for x, y in zip(xs, ys)]
    nb = MTM.hitNeighbourhoods(lt, img, hits, 3)
    smap = MTM.computeScoreMap(t, img, 3)
    pad = np.full((oh + 2, ow + 2), np.nan, dtype=np.float32)
    pad[1:-1, 1:-1] = smap
    exp = np.stack([pad[ys + dy, xs + dx] for dy in range(3) for dx in range(3)], axis=1).reshape(-1, 3, 3)
    assert np.array_equal(nb, exp, equal_nan=True)
    assert np.array_equal(nb[:50], np.repeat(nb[:1], 50, axis=0))
    assert MTM.hitNeighbourhoods(lt, img, []).shape == (0, 3, 3)
    assert MTM.refineHits(lt, img, []) == []


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
def test_matcher_refine_then_match_equals_match_templates(dtype):
    lt, img, hits = _scene(41, dtype, 1, [(12, 12), (9, 14), (20, 20)])
    m = MTM.TemplateMatcher(lt, method=5, score_threshold=0.5)
    try:
        assert m.refine(img, hits) == MTM.refineHits(lt, img, hits, 5)
        assert m._uploaded_for == (np.dtype(dtype).name, 1)
        assert m.match(img) == MTM.matchTemplates(lt, img, method=5, score_threshold=0.5)
        assert m.refine(img, []) == []
        assert m._uploaded_for == (np.dtype(dtype).name, 1)
        with pytest.raises(ValueError):
            m.refine(img, [("nope", (0, 0, 12, 12), 0.5)])
        assert m._uploaded_for is None                  # a call that raises clears the record: match() uploads again
        assert m.match(img) == MTM.matchTemplates(lt, img, method=5, score_threshold=0.5)
    finally:
        m._ctx.close()


@pytest.mark.parametrize("repeat", [0, 1])         # (consecutive tests: the fixture's two poison patterns)
def test_results_do_not_depend_on_poisoned_memory(repeat):
    for dtype, chans, method, masked in [(np.uint8, 3, 5, False), (np.uint16, 1, 1, False), (np.uint8, 1, 3, True),
                                         (np.float32, 1, 0, True)]:
        lt, img, hits = _scene(50, dtype, chans, SIZES, masked=masked)
        nb = MTM.hitNeighbourhoods(lt, img, hits, method)
        if dtype == np.float32:
            assert np.array_equal(nb, MTM.hitNeighbourhoods(lt, img, hits, method), equal_nan=True)
        else:
            assert np.array_equal(nb, _score_map_cuts(lt, img, hits, method), equal_nan=True)


def test_gaussian_blob_shifts_are_recovered_on_the_gpu():
    worst = 0.0
    for dx, dy in BLOB_SHIFTS:
        t, img, tx, ty = blob_case(dx, dy)
        hits = MTM.findMatches([("blob", t)], img, N_object=1)
        assert len(hits) == 1
        (_, (xf, yf, _, _), _), = MTM.refineHits([("blob", t)], img, hits)
        assert abs(xf - tx) <= 0.05 and abs(yf - ty) <= 0.05, (dx, dy, xf, yf)
        worst = max(worst, abs(hits[0][1][0] - tx), abs(hits[0][1][1] - ty))
    assert worst >= 0.4
