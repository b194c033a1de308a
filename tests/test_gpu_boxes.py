"""MTM.findMatchesInBoxes / matchTemplatesInBoxes / TemplateMatcher.match_boxes on the GPU: every case equals the loop of
findMatches / matchTemplates with searchBox a user writes today (hits, order, labels, boxes, float32 score bits, exceptions),
and the scores equal computeScoreMap on the crop bit for bit."""
import warnings

import numpy as np
import pytest

import MTM
from MTM import _lib

pytestmark = pytest.mark.gpu

INF = float("inf")


def _key(hits):
    return [(h[0], tuple(int(v) for v in h[1]), np.float32(h[2]).tobytes()) for h in hits]


def _norm(regions):
    """searchBoxes -> [(box, indices or None)]"""
    out = []
    for el in regions:
        if len(el) == 2:
            out.append((tuple(el[0]), list(el[1])))
        else:
            out.append((tuple(el), None))
    return out


def _loop(fn, templs, img, regions, *args):
    res = []
    for box, idx in _norm(regions):
        sub = templs if idx is None else [templs[j] for j in idx]
        res.append(fn(sub, img, *args, searchBox=box))
    return res


def _outcome(call):
    """(result, None) or (None, (exception type, message))"""
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            r = call()
        return r, None, len(w)
    except Exception as e:  # noqa: BLE001 - compared with the loop's
        return None, (type(e), str(e)), 0


def _check_scores(templs, img, regions, method, got, n_regions=3):
    """Each hit's score bits are those of computeScoreMap on its region's crop."""
    for (box, idx), hits in list(zip(_norm(regions), got))[:n_regions]:
        x, y, w, h = box
        crop = img[y:y + h, x:x + w]
        by_label = {t[0]: t[1] for t in templs}
        maps = {}
        for lab, (hx, hy, _, _), sc in hits:
            if lab not in maps:
                maps[lab] = MTM.computeScoreMap(by_label[lab], crop, method)
            assert np.float32(sc).tobytes() == maps[lab][hy - y, hx - x].tobytes()


def _compare(templs, img, regions, method, n_obj, thr, overlap=None, check_scores=True):
    if overlap is None:
        exp = _outcome(lambda: _loop(MTM.findMatches, templs, img, regions, method, n_obj, thr))
        got = _outcome(lambda: MTM.findMatchesInBoxes(templs, img, regions, method, n_obj, thr))
    else:
        exp = _outcome(lambda: _loop(MTM.matchTemplates, templs, img, regions, method, n_obj, thr, overlap))
        got = _outcome(lambda: MTM.matchTemplatesInBoxes(templs, img, regions, method, n_obj, thr, overlap))
    assert got[1] == exp[1]
    assert got[2] == exp[2]                 # mask warnings
    if exp[1] is None:
        assert len(got[0]) == len(exp[0])
        for g, e in zip(got[0], exp[0]):
            assert _key(g) == _key(e)
        if check_scores:
            _check_scores(templs, img, regions, method, got[0])
    return exp


class _Opt:
    """An option of the default context for the duration of a block (put back afterwards)."""
    def __init__(self, opt, value):
        self.opt, self.value = opt, value

    def __enter__(self):
        self.ctx = _lib.default_context()
        self.old = self.ctx.get_option(self.opt)
        self.ctx.set_option(self.opt, self.value)
        return self

    def __exit__(self, *exc):
        self.ctx.set_option(self.opt, self.old)


def _image(rng, h, w, kind):
    if kind == "u16":
        img = rng.randint(0, 65536, size=(h, w)).astype(np.uint16)
    elif kind == "rgb":
        img = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    else:
        img = rng.randint(0, 256, size=(h, w)).astype(np.uint8)
    return img


def _templates(rng, img, n, hmax=16):
    out = []
    for i in range(n):
        th, tw = rng.randint(2, hmax + 1, 2)
        y, x = rng.randint(0, img.shape[0] - th), rng.randint(0, img.shape[1] - tw)
        out.append(("t%d" % i, img[y:y + th, x:x + tw].copy()))
    return out


_THR = {0: 1e13, 1: 0.3, 2: 0.0, 3: 0.7, 4: 0.0, 5: 0.3}


@pytest.mark.parametrize("kind", ["u8", "rgb", "u16"])
@pytest.mark.parametrize("method", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("n_obj", [INF, 1, 3])
def test_find_matches_in_boxes_equals_loop(kind, method, n_obj):
    rng = np.random.RandomState(7 * method + {"u8": 0, "rgb": 1, "u16": 2}[kind])
    img = _image(rng, 96, 110, kind)
    templs = _templates(rng, img, 3)
    regions = [(0, 0, 40, 40), (30, 20, 50, 45), ((60, 50, 60, 60), [2, 0]), ((5, 70, 30, 30), []),
               ((95, 80, 40, 40), [1, 1])]
    _compare(templs, img, regions, method, n_obj, _THR[method])


@pytest.mark.parametrize("kind", ["u8", "rgb", "u16"])
@pytest.mark.parametrize("method", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("n_obj", [INF, 1, 3])
@pytest.mark.parametrize("border", [0, 1])
def test_match_templates_in_boxes_equals_loop(kind, method, n_obj, border):
    rng = np.random.RandomState(11 * method + border)
    img = _image(rng, 90, 100, kind)
    templs = _templates(rng, img, 2, hmax=12)
    regions = [(0, 0, 45, 45), (20, 25, 60, 50), ((50, 40, 50, 50), [1]), (70, 60, 200, 200)]
    with _Opt(_lib.OPT_PEAK_BORDER, border):
        _compare(templs, img, regions, method, n_obj, _THR[method], overlap=0.25)


def test_clipped_boxes_at_every_edge_and_1d_maps():
    rng = np.random.RandomState(3)
    img = _image(rng, 64, 72, "u8")
    templs = [("a", img[10:18, 20:26].copy()), ("b", img[30:31, 5:15].copy())]
    regions = [
        (60, 10, 40, 20), (10, 50, 20, 40), (60, 50, 40, 40), (0, 0, 8, 30),      # right, bottom, corner, left edge
        ((20, 20, 6, 30), [0]),            # map 23 x 1 (N x 1)
        ((20, 20, 30, 8), [0]),            # map 1 x 25 (1 x N)
        ((20, 20, 6, 8), [0]),             # 1 x 1
        ((0, 30, 10, 1), [1]),             # 1 x 1 with a one-row template
        ((0, 29, 72, 1), [1]),             # 1 x 63
    ]
    for border in (0, 1):
        with _Opt(_lib.OPT_PEAK_BORDER, border):
            for method, thr in ((5, 0.2), (1, 0.6), (0, 1e9), (3, 0.5)):
                _compare(templs, img, regions, method, INF, thr)
                _compare(templs, img, regions, method, 1, thr)
                if method:
                    _compare(templs, img, regions, method, INF, thr, overlap=0.3)


def test_constant_patches_have_no_peaks():
    rng = np.random.RandomState(4)
    img = _image(rng, 80, 80, "u8")
    img[10:40, 10:40] = 77
    templs = [("flat", np.full((6, 6), 77, np.uint8)), ("tex", img[50:58, 50:58].copy())]
    regions = [(10, 10, 30, 30), (5, 5, 40, 40), (45, 45, 30, 30)]
    for method in (0, 1, 2, 3, 4, 5):
        exp = _compare(templs, img, regions, method, INF, -1e18 if method not in (0, 1) else 1e18)
        assert exp[0][0] == []                  # the flat map of the flat region: no peaks


def test_one_template_in_hundreds_of_overlapping_boxes():
    rng = np.random.RandomState(5)
    img = _image(rng, 256, 256, "u8")
    templs = [("t", img[100:110, 120:128].copy())]
    regions = [(int(x), int(y), 24, 24) for x, y in rng.randint(0, 240, size=(300, 2))]
    _compare(templs, img, regions, 5, INF, 0.2, check_scores=False)
    _compare(templs, img, regions, 5, 3, 0.2, overlap=0.25, check_scores=False)
    _compare(templs, img, regions[:40], 5, 1, 0.2, overlap=0.25)


def test_large_templates():
    rng = np.random.RandomState(6)
    img = _image(rng, 360, 340, "rgb")
    templs = [("big", img[20:320, 15:295].copy())]                    # 300 x 280 x 3
    regions = [(10, 12, 300, 296), (0, 0, 340, 360)]
    _compare(templs, img, regions, 5, INF, 0.1)
    _compare(templs, img, regions, 1, 1, 0.5, overlap=0.25)
    gray = _image(rng, 460, 450, "u8")
    templs = [("huge", gray[30:444, 20:420].copy())]                  # 414 x 400
    _compare(templs, gray, [(10, 20, 420, 430)], 5, INF, 0.1)
    _compare(templs, gray, [(10, 20, 420, 430)], 3, 1, 0.5, overlap=0.25)


def test_small_hit_capacity_and_output_overflow():
    rng = np.random.RandomState(8)
    img = _image(rng, 200, 200, "u8")
    templs = [("t", img[0:5, 0:5].copy())]
    regions = [(0, 0, 200, 200), (10, 10, 100, 100)]         # ~ 5000 local maxima over a zero threshold (> 4096 records)
    with _Opt(_lib.OPT_HIT_CAPACITY, 16):
        _compare(templs, img, regions, 2, INF, 0.0, check_scores=False)
    ctx = _lib.default_context()
    ctx.set_templates([(templs[0][1], None)], 2)
    units = np.zeros(2, dtype=_lib.BOX_UNIT_DTYPE)
    units["rows"], units["cols"] = 200, 200
    raw, counts = ctx.find_matches_boxes(img, units, _lib.PEAKS_LOCAL, 0.0)
    assert len(raw) == counts.sum() > 4096 and counts[0] == counts[1]


def test_small_box_budget_forces_chunks():
    rng = np.random.RandomState(9)
    img = _image(rng, 120, 120, "u16")
    templs = _templates(rng, img, 3, hmax=10)
    regions = [(int(x), int(y), 30, 30) for x, y in rng.randint(0, 100, size=(40, 2))]
    exp = _compare(templs, img, regions, 5, INF, 0.3, check_scores=False)
    with _Opt(_lib.OPT_BOXES_MAX_FLOATS, 300):
        got = MTM.findMatchesInBoxes(templs, img, regions, 5, INF, 0.3)
    assert [_key(g) for g in got] == [_key(e) for e in exp[0]]


def test_template_matcher_match_boxes_over_frames():
    rng = np.random.RandomState(10)
    templs = [("a", _image(rng, 12, 10, "u8")), ("b", _image(rng, 9, 14, "u8"))]
    matcher = MTM.TemplateMatcher(templs, 5, 3, 0.4, 0.25)
    for frame in range(4):
        img = _image(rng, 128, 128, "u8")
        img[40:52, 30:40] = templs[0][1]
        regions = [(int(x), int(y), 40, 40) for x, y in rng.randint(0, 100, size=(8, 2))] + [((25, 35, 30, 30), [0])]
        got = matcher.match_boxes(img, regions)
        exp = MTM.matchTemplatesInBoxes(templs, img, regions, 5, 3, 0.4, 0.25)
        assert [_key(g) for g in got] == [_key(e) for e in exp]
        assert [_key(g) for g in got] == [_key(e) for e in _loop(MTM.matchTemplates, templs, img, regions, 5, 3, 0.4, 0.25)]
    assert _key(matcher.match(img)) == _key(MTM.matchTemplates(templs, img, 5, 3, 0.4, 0.25))


@pytest.mark.parametrize("kind", ["u8", "u16"])
@pytest.mark.parametrize("method", [1, 5])
@pytest.mark.parametrize("n_obj", [0, -1, 2])
def test_finite_n_object_cuts_as_the_loop(kind, method, n_obj):
    """A finite N_object as the loop applies it: the uint8 route cuts every list (one hit too) to N_object, the uint16
    route returns a list of one hit as it is; boxes of the template's own size hold exactly one hit."""
    rng = np.random.RandomState(20 + method)
    img = _image(rng, 80, 90, kind)
    templs = [("a", img[10:19, 12:20].copy()), ("b", img[40:47, 50:60].copy())]
    regions = [((12, 10, 8, 9), [0]), ((50, 40, 10, 7), [1]), ((12, 10, 8, 9), [0, 0]), (0, 0, 60, 60), (30, 20, 60, 60)]
    exp = _compare(templs, img, regions, method, n_obj, 0.9 if method == 5 else 0.05, overlap=0.25)
    assert exp[1] is None
    single = [len(_loop(MTM.findMatches, templs, img, regions[:2], method, INF, 0.9 if method == 5 else 0.05)[k])
              for k in range(2)]
    assert single == [1, 1]                         # the one-hit lists the two routes treat differently for N_object = 0
    if n_obj == 0:
        assert [len(h) for h in exp[0][:2]] == ([0, 0] if kind == "u8" else [1, 1])


def test_match_boxes_without_units_keeps_match_working():
    """match_boxes with nothing to search sets no templates, and match() afterwards still uploads and matches."""
    rng = np.random.RandomState(12)
    img = _image(rng, 96, 96, "u8")
    templs = [("a", img[10:20, 10:22].copy()), ("b", img[50:58, 30:44].copy())]
    exp = _key(MTM.matchTemplates(templs, img, 5, INF, 0.5, 0.25))
    m = MTM.TemplateMatcher(templs, 5, INF, 0.5, 0.25)
    assert m.match_boxes(img, []) == []
    assert _key(m.match(img)) == exp
    m = MTM.TemplateMatcher(templs, 5, INF, 0.5, 0.25)
    assert m.match_boxes(img, [((0, 0, 40, 40), []), ((20, 20, 40, 40), [])]) == [[], []]
    assert _key(m.match(img)) == exp
    # a matcher whose resident set is float32 (match() on a float32 image) keeps it through a call that sets nothing
    f32 = img.astype(np.float32)
    exp32 = _key(MTM.matchTemplates(templs, f32, 5, INF, 0.5, 0.25))
    m = MTM.TemplateMatcher(templs, 5, INF, 0.5, 0.25)
    assert _key(m.match(f32)) == exp32
    assert m.match_boxes(img, [((0, 0, 40, 40), [])]) == [[]]
    assert _key(m.match(f32)) == exp32
    # and one that set the uint8 templates: match() on uint8 images runs on them
    got = m.match_boxes(img, [(0, 0, 40, 40)])
    assert [_key(g) for g in got] == [_key(e) for e in _loop(MTM.matchTemplates, templs, img, [(0, 0, 40, 40)], 5, INF,
                                                               0.5, 0.25)]
    assert _key(m.match(img)) == exp


def _random_case(rng):
    kind = ["u8", "rgb", "u16"][rng.randint(3)]
    H, W = rng.randint(24, 90, 2)
    img = _image(rng, H, W, kind)
    if rng.rand() < 0.3:                                   # a constant patch
        y, x = rng.randint(0, H // 2), rng.randint(0, W // 2)
        img[y:y + rng.randint(4, 30), x:x + rng.randint(4, 30)] = img[0, 0]
    templs = _templates(rng, img, rng.randint(1, 4), hmax=8)
    regions = []
    for _ in range(rng.randint(1, 6)):            # boxes of >= 10 x 10 pixels after clipping, some past the edges
        box = (int(rng.randint(0, W - 10)), int(rng.randint(0, H - 10)), int(rng.randint(10, 60)), int(rng.randint(10, 60)))
        if rng.rand() < 0.4:
            regions.append((box, [int(j) for j in rng.randint(0, len(templs), rng.randint(0, 3))]))
        else:
            regions.append(box)
    if rng.rand() < 0.1:                          # a box smaller than a template: the loop's error, at the loop's region
        regions.insert(int(rng.randint(0, len(regions) + 1)), (1, 1, 1, 1))
    return kind, img, templs, regions


def test_seeded_random_sweep():
    rng = np.random.RandomState(2024)
    n_ok = n_err = 0
    for case in range(220):
        kind, img, templs, regions = _random_case(rng)
        match = rng.rand() < 0.5
        method = int(rng.randint(1 if match else 0, 6))
        n_obj = [INF, 1, 3][rng.randint(3)]
        thr = {0: 1e12, 1: 0.4, 2: 0.0, 3: 0.8, 4: 0.0, 5: 0.2}[method]
        with _Opt(_lib.OPT_PEAK_BORDER, int(rng.randint(2))):
            exp = _compare(templs, img, regions, method, n_obj, thr, overlap=0.25 if match else None,
                           check_scores=case % 10 == 0)
        n_ok += exp[1] is None
        n_err += exp[1] is not None
    assert n_ok > 100 and n_err > 5                         # both outcomes are exercised
