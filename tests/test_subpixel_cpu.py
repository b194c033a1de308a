"""MTM.hitNeighbourhoods / refineHits without a GPU: the parabola fit restated in plain Python on neighbourhoods cut from the
oracle's score maps, every scope and lookup error raised before anything reaches the library, and the fit's accuracy on
analytically rendered blobs."""
import math
import warnings

import numpy as np
import pytest

import MTM
import mtm_oracle as O
from MTM import _lib
from MTM.subpixel import fit_offsets


class _NativeCalled(Exception):
    pass


@pytest.fixture
def no_native(monkeypatch):
    """Any use of the library raises _NativeCalled: a ValueError that comes first was raised in the Python layer."""
    def boom(*a, **k):
        raise _NativeCalled()
    monkeypatch.setattr(_lib, "default_context", boom)
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_lib, "engine_for", boom)


def _img(h=64, w=80, chans=1, dtype=np.uint8, seed=0):
    rng = np.random.RandomState(seed)
    shape = (h, w) if chans == 1 else (h, w, chans)
    return rng.randint(0, 256, size=shape).astype(dtype)


def _fit_axis(a, b, c, minima):
    """The fit of one axis as the issue defines it, in Python floats."""
    a, b, c = float(a), float(b), float(c)
    if minima:
        a, b, c = -a, -b, -c
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return 0.0
    if not (b >= a and b >= c):
        return 0.0
    d = (a - 2 * b) + c
    if not d < 0:
        return 0.0
    return 0.5 * (a - c) / d


def _fit(n, method):
    m = method in (0, 1)
    return _fit_axis(n[1, 0], n[1, 1], n[1, 2], m), _fit_axis(n[0, 1], n[1, 1], n[2, 1], m)


def _cut(smap, x, y):
    """smap[y - 1:y + 2, x - 1:x + 2] with NaN outside the map."""
    out = np.full((3, 3), np.nan, dtype=np.float32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if 0 <= y + dy < smap.shape[0] and 0 <= x + dx < smap.shape[1]:
                out[1 + dy, 1 + dx] = smap[y + dy, x + dx]
    return out


@pytest.mark.parametrize("method", range(6))
def test_fit_matches_its_restatement_on_oracle_neighbourhoods(method):
    img = _img(48, 56, seed=method)
    img[10:20, 10:30] = 77                              # flat windows: NaN / saturated scores
    t = img[20:32, 24:40].copy()
    smap = O.match_template(img, t, method)
    oh, ow = smap.shape
    pts = [(0, 0), (ow - 1, 0), (0, oh - 1), (ow - 1, oh - 1), (ow // 2, 0), (0, oh // 2), (24, 20), (11, 11)]
    pts += [(x, y) for y in range(1, oh - 1, 5) for x in range(1, ow - 1, 7)]
    nb = np.stack([_cut(smap, x, y) for x, y in pts])
    ox, oy = fit_offsets(nb, method)
    for k in range(len(pts)):
        ex, ey = _fit(nb[k], method)
        assert (float(ox[k]), float(oy[k])) == (ex, ey)
        assert abs(ex) <= 0.5 and abs(ey) <= 0.5


def test_fit_special_cases():
    nan = float("nan")
    cases = [
        # (neighbourhood rows, method, expected (ox, oy))
        ([[0, 0, 0], [0.5, 1.0, 0.5], [0, 0, 0]], 5, (0.0, 0.0)),        # symmetric in x; y: a = c = 0, d < 0 -> 0
        ([[0, 0, 0], [1.0, 1.0, 0.0], [0, 0, 0]], 5, (-0.5, 0.0)),       # two equal maxima: the midpoint
        ([[0, 0, 0], [0.0, 1.0, 1.0], [0, 0, 0]], 5, (0.5, 0.0)),
        ([[0, 0, 0], [2.0, 1.0, 0.0], [0, 0, 0]], 5, (0.0, 0.0)),        # not a maximum along x
        ([[0, 0, 0], [nan, 1.0, 0.5], [0, 0, 0]], 5, (0.0, 0.0)),        # border
        ([[1, 1, 1], [1.0, 1.0, 1.0], [1, 1, 1]], 5, (0.0, 0.0)),        # plateau: d == 0
        ([[9, 0.2, 9], [0.6, 0.1, 0.2], [9, 0.4, 9]], 0, None),          # minima: the restatement's value, non-zero
        ([[9, 0.2, 9], [0.6, 0.1, 0.2], [9, 0.4, 9]], 5, (0.0, 0.0)),    # a minimum is no maximum
    ]
    for rows, method, exp in cases:
        nb = np.array([rows], dtype=np.float32)
        ox, oy = fit_offsets(nb, method)
        if exp is None:
            exp = _fit(nb[0], method)
            assert exp[0] != 0.0 and exp[1] != 0.0
        assert (float(ox[0]), float(oy[0])) == exp
    ox, _ = fit_offsets(np.array([[[0, 0, 0], [0.2, 1.0, 0.6], [0, 0, 0]]], dtype=np.float32), 5)
    assert 0.0 < ox[0] <= 0.5


def _blob(shape, cx, cy, sigma=4.0):
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    return np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * sigma * sigma))


def blob_case(dx, dy):
    """(template, image, true window x, true window y): a Gaussian blob (sigma 4) at the centre of a 25 x 25 template, and
    the same blob rendered in an 80 x 96 image at a known fractional shift."""
    t = (200.0 * _blob((25, 25), 12.0, 12.0) + 10.0).astype(np.float32)
    x0, y0 = 37, 29
    img = (200.0 * _blob((80, 96), x0 + 12.0 + dx, y0 + 12.0 + dy) + 10.0).astype(np.float32)
    return t, img, x0 + dx, y0 + dy


BLOB_SHIFTS = [(-0.5, 0.0), (-0.4, 0.3), (-0.25, -0.5), (0.0, 0.0), (0.1, -0.2), (0.33, 0.45), (0.5, 0.5), (0.2, -0.35)]


@pytest.mark.parametrize("method", [1, 3, 5])
def test_fit_recovers_known_shifts_of_a_gaussian_blob(method):
    worst_int = 0.0
    for dx, dy in BLOB_SHIFTS:
        t, img, tx, ty = blob_case(dx, dy)
        smap = O.match_template(img, t, method)
        y, x = np.unravel_index(np.argmin(smap) if method in (0, 1) else np.argmax(smap), smap.shape)
        ox, oy = fit_offsets(_cut(smap, x, y)[None], method)
        assert abs(x + ox[0] - tx) <= 0.05 and abs(y + oy[0] - ty) <= 0.05, (dx, dy, x + ox[0], y + oy[0])
        worst_int = max(worst_int, abs(x - tx), abs(y - ty))
    assert worst_int >= 0.4                     # whole-pixel positions miss by up to 0.5


# ---- scope and lookup errors, before any native call -------------------------------------------------------------------

def _hit(label="a", x=5, y=6, w=16, h=16, score=0.9):
    return (label, (x, y, w, h), np.float32(score))


BAD = [
    # (description, kwargs, fragment of the message)
    ("float64 image", dict(image=_img(dtype=np.float64)), "64-bit"),
    ("float64 template", dict(templ=_img(16, 16, dtype=np.float64)), "64-bit"),
    ("2-channel image", dict(image=_img(chans=2), templ=_img(16, 16, chans=2)), "1 or 3 channels"),
    ("4-channel image", dict(image=_img(chans=4), templ=_img(16, 16, chans=4)), "1 or 3 channels"),
    ("3-channel uint16", dict(image=_img(chans=3, dtype=np.uint16), templ=_img(16, 16, chans=3, dtype=np.uint16)),
     "uint16"),
    ("channel mismatch", dict(image=_img(chans=3), templ=_img(16, 16)), "channels"),
    ("1-D image", dict(image=np.zeros(64, np.uint8)), "2-D"),
    ("unknown label", dict(hits=[_hit(label="b")]), "hit 0: no template"),
    ("wrong shape", dict(hits=[_hit(), _hit(w=15)]), "hit 1: no template"),
    ("left of the map", dict(hits=[_hit(x=-1)]), "hit 0: window"),
    ("below the map", dict(hits=[_hit(), _hit(), _hit(y=64 - 16 + 1)]), "hit 2: window"),
    ("right of the map", dict(hits=[_hit(x=80 - 16 + 1)]), "hit 0: window"),
    ("float position", dict(hits=[("a", (5.5, 6, 16, 16), 0.9)]), "hit 0: the box"),
    ("not a hit", dict(hits=[("a", (5, 6, 16), 0.9)]), "hit 0 is not"),
    ("ambiguous", dict(extra=[("a", _img(16, 16, seed=3))]), "hit 0: templates 0 and 1"),
    ("ambiguous mask", dict(extra=[("a", _img(16, 16, seed=1), np.ones((16, 16), np.uint8))], method=3),
     "hit 0: templates 0 and 1"),
]


@pytest.mark.parametrize("desc,kw,msg", BAD, ids=[b[0] for b in BAD])
@pytest.mark.parametrize("api", ["nbhd", "refine"])
def test_scope_and_lookup_errors_before_any_native_call(no_native, api, desc, kw, msg):
    kw = dict(kw)
    image = kw.pop("image", _img())
    chans = 1 if image.ndim != 3 else image.shape[2]
    templ = kw.pop("templ", _img(16, 16, chans=chans, seed=1))
    hits = kw.pop("hits", [_hit()])
    lt = [("a", templ)] + kw.pop("extra", [])
    fn = MTM.hitNeighbourhoods if api == "nbhd" else MTM.refineHits
    with pytest.raises(ValueError, match=msg):
        fn(lt, image, hits, **kw)


def test_duplicate_entries_with_equal_pixels_are_one_template(no_native):
    t = _img(16, 16, seed=1)
    with pytest.raises(_NativeCalled):
        MTM.refineHits([("a", t), ("a", t.copy()), ("b", t)], _img(), [_hit(), _hit(label="b")])


def test_augmented_lists_pass_the_lookup(no_native):
    t = _img(16, 24, seed=1)
    lt = MTM.augment.flips(MTM.augment.rotations([("a", t)]))
    assert len({e[0] for e in lt}) == len(lt)
    hits = [(lab, (3, 4, tt.shape[1], tt.shape[0]), np.float32(0.5)) for lab, tt, *_ in lt]
    with pytest.raises(_NativeCalled):
        MTM.hitNeighbourhoods(lt, _img(), hits)


def test_empty_hit_lists_never_reach_the_library(no_native):
    t = _img(16, 16)
    nb = MTM.hitNeighbourhoods([("a", t)], _img(), [])
    assert nb.shape == (0, 3, 3) and nb.dtype == np.float32
    assert MTM.refineHits([("a", t)], _img(), []) == []


def test_masks_with_other_methods_are_dropped_with_the_score_map_warning(no_native):
    t = _img(16, 16, seed=1)
    with pytest.warns(UserWarning, match="not compatible with use of mask"):
        with pytest.raises(_NativeCalled):
            MTM.hitNeighbourhoods([("a", t, np.ones_like(t))], _img(), [_hit()], method=5)


@pytest.mark.parametrize("desc,image,templ,mask", [
    ("uint8", _img(), _img(16, 16, seed=1), None),
    ("uint8 rgb", _img(chans=3), _img(16, 16, chans=3, seed=1), None),
    ("uint8 masked", _img(), _img(16, 16, seed=1), np.ones((16, 16), np.uint8)),
    ("uint16", _img(dtype=np.uint16), _img(16, 16, dtype=np.uint16, seed=1), None),
    ("uint16 masked", _img(dtype=np.uint16), _img(16, 16, dtype=np.uint16, seed=1), np.ones((16, 16), np.uint16)),
    ("float32 rgb", _img(chans=3, dtype=np.float32), _img(16, 16, chans=3, dtype=np.float32, seed=1), None),
    ("mixed", _img(dtype=np.int16), _img(16, 16, seed=1), None),
])
def test_in_scope_inputs_reach_the_library(no_native, desc, image, templ, mask):
    lt = [("a", templ) if mask is None else ("a", templ, mask)]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(_NativeCalled):
            MTM.hitNeighbourhoods(lt, image, [_hit()], method=3)
