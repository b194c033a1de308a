"""MTM.findMatchesPyramid / matchTemplatesPyramid without a GPU: the scope checks (every exclusion is a ValueError raised
before anything reaches the library) and the numpy restatement of the semantics (tests/pyramid_cases.py) against the
exhaustive oracle."""
import warnings

import numpy as np
import pytest

import MTM
import mtm_oracle as O
import pyramid_cases as P
from MTM import _lib


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


BAD = [
    # (description, kwargs, fragment of the message)
    ("float32 image", dict(image=_img(dtype=np.float32)), "uint8"),
    ("uint16 template", dict(templ=_img(16, 16, dtype=np.uint16)), "uint8"),
    ("2-channel image", dict(image=_img(chans=2), templ=_img(16, 16, chans=2)), "3-channel"),
    ("method 0", dict(method=0), "TM_SQDIFF"),
    ("method 6", dict(method=6), "1..5"),
    ("method 2 without coarse_threshold", dict(method=2), "coarse_threshold"),
    ("method 4 without coarse_threshold", dict(method=4), "coarse_threshold"),
    ("factor 1", dict(factor=1), "factor"),
    ("factor 0", dict(factor=0), "factor"),
    ("factor 2.0", dict(factor=2.0), "factor"),
    ("factor True", dict(factor=True), "factor"),
    ("negative radius", dict(radius=-1), "radius"),
    ("max_candidates 0", dict(max_candidates=0), "max_candidates"),
    ("coarse template 1x1", dict(templ=_img(3, 3)), "at least 2x2"),
    ("coarse template 2x1", dict(templ=_img(16, 3)), "at least 2x2"),
    ("template larger than the image", dict(templ=_img(65, 16)), "larger"),
    ("coarse map 1-D (rows)", dict(image=_img(21, 80), templ=_img(20, 16), factor=4), "coarse score map"),
    ("coarse map 1-D (columns)", dict(image=_img(64, 41), templ=_img(16, 40), factor=4), "coarse score map"),
    ("full map 1-D", dict(image=_img(20, 80), templ=_img(20, 16), factor=4), "score map"),
    ("searchBox leaves a 1-D map", dict(templ=_img(16, 16), searchBox=(0, 0, 80, 16)), "score map"),
]


@pytest.mark.parametrize("desc,kw,msg", BAD, ids=[b[0] for b in BAD])
@pytest.mark.parametrize("api", ["find", "match"])
def test_scope_errors_before_any_native_call(no_native, api, desc, kw, msg):
    kw = dict(kw)
    image = kw.pop("image", _img())
    templ = kw.pop("templ", _img(16, 16, chans=1 if image.ndim == 2 else image.shape[2], dtype=np.uint8))
    factor = kw.pop("factor", 2)
    fn = MTM.findMatchesPyramid if api == "find" else MTM.matchTemplatesPyramid
    with pytest.raises(ValueError, match=msg):
        fn([("a", templ)], image, factor, **kw)


def test_mask_with_method_3_is_an_error(no_native):
    t = _img(16, 16)
    with pytest.raises(ValueError, match="mask"):
        MTM.findMatchesPyramid([("a", t, np.ones_like(t))], _img(), 2, method=3)


def test_mask_with_another_method_is_ignored_with_the_usual_warning(no_native):
    t = _img(16, 16)
    with pytest.warns(UserWarning, match="not supporting the use of Mask"):
        with pytest.raises(_NativeCalled):          # the checks passed: the call went on to the library
            MTM.findMatchesPyramid([("a", t, np.ones_like(t))], _img(), 2, method=5)


def test_valid_call_reaches_the_library(no_native):
    with pytest.raises(_NativeCalled):
        MTM.matchTemplatesPyramid([("a", _img(16, 16))], _img(), 2, method=2, coarse_threshold=1e6)


def test_max_overlap_range(no_native):
    with pytest.raises(ValueError, match="overlap"):
        MTM.matchTemplatesPyramid([("a", _img(16, 16))], _img(), 2, maxOverlap=1.5)


def test_exported():
    assert "findMatchesPyramid" in MTM.__all__ and "matchTemplatesPyramid" in MTM.__all__
    assert "mtm_find_matches_pyramid" in _lib.SYMBOLS


# ---- the restatement ---------------------------------------------------------------------------------------------------
def _key(hits):
    return [(h[0], tuple(h[1]), np.float32(h[2]).tobytes()) for h in hits]


@pytest.mark.parametrize("method", [1, 3, 5])
@pytest.mark.parametrize("border", ["nearest", "constant"])
def test_whole_map_windows_equal_the_exhaustive_search(method, border):
    img, units = P.planted(3, hw=(72, 90), side=16, n_templ=2)
    H, W = img.shape
    cthr = 2.0 if method == 1 else -2.0             # every coarse peak is a candidate
    for f in (2, 3):
        got = P.find_matches_pyramid(units, img, f, method, score_threshold=0.5 if method != 1 else 0.3,
                                     coarse_threshold=cthr, radius=max(H, W), border=border)
        exp = O.find_matches(units, img, method, score_threshold=0.5 if method != 1 else 0.3, border=border)
        assert _key(got) == _key(exp)
        for n_obj in (1, float("inf")):
            got = P.match_templates_pyramid(units, img, f, method, N_object=n_obj, coarse_threshold=cthr,
                                            radius=max(H, W), border=border)
            exp = O.match_templates(units, img, method, N_object=n_obj, border=border)
            assert _key(got) == _key(exp)


def test_windows_clip_at_every_edge():
    oh, ow = 20, 30
    assert P.windows([(0, 0)], 2, 3, oh, ow) == [(0, 3, 0, 3)]                 # top-left
    assert P.windows([(9, 14)], 2, 3, oh, ow) == [(15, 19, 25, 29)]            # bottom-right
    assert P.windows([(0, 14)], 3, 1, oh, ow) == []                            # right of the map: empty
    assert P.windows([(5, 7)], 2, 0, oh, ow) == [(10, 10, 14, 14)]             # radius 0: one position
    assert P.windows([(3, 3)], 4, 100, oh, ow) == [(0, 19, 0, 29)]             # the whole map


def test_overlapping_windows_count_a_position_once():
    img, units = P.random_with_flats(5)
    oh, ow = img.shape[0] - 11, img.shape[1] - 11
    wins = P.windows([(10, 10), (11, 11), (10, 11)], 2, 2, oh, ow)
    u = P.union_mask(wins, oh, ow)
    assert u.sum() == len({(y, x) for y0, y1, x0, x1 in wins for y in range(y0, y1 + 1) for x in range(x0, x1 + 1)})
    hits = P.find_matches_pyramid(units, img, 2, 5, score_threshold=0.1, coarse_threshold=-1.0, radius=2,
                                  max_candidates=8)
    boxes = [(h[0], h[1]) for h in hits]
    assert len(boxes) == len(set(boxes)) and len(boxes) > 0


def test_search_box_offsets():
    img, units = P.planted(7, hw=(96, 120), side=16, n_templ=2)
    box = (13, 9, 90, 80)
    got = P.find_matches_pyramid(units, img, 2, 5, searchBox=box, score_threshold=0.3, coarse_threshold=0.0)
    crop = img[9:89, 13:103]
    ref = P.find_matches_pyramid(units, crop, 2, 5, score_threshold=0.3, coarse_threshold=0.0)
    assert len(got) > 0
    assert [(h[0], (h[1][0] - 13, h[1][1] - 9) + tuple(h[1][2:]), h[2]) for h in got] == ref


def test_partial_windows_are_a_subset_of_the_exhaustive_hits():
    img, units = P.random_with_flats(11, chans=3)
    full = O.find_matches(units, img, 5, score_threshold=0.05)
    for mc in (1, 4):
        for r in (0, 1, 2):
            got = P.find_matches_pyramid(units, img, 2, 5, score_threshold=0.05, coarse_threshold=0.0, radius=r,
                                         max_candidates=mc)
            assert set(_key(got)) <= set(_key(full))
