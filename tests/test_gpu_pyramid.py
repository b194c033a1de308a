"""MTM.findMatchesPyramid / matchTemplatesPyramid on the GPU: equal to the exhaustive engine where the windows cover its
hits, equal to the restatement of tests/pyramid_cases.py evaluated on the engine's own score maps everywhere, scores bit
for bit those of computeScoreMap; the ABI entry's overflow protocol."""
import ctypes

import numpy as np
import pytest

import MTM
import pyramid_cases as P
from MTM import _lib, augment

pytestmark = pytest.mark.gpu


def _key(hits):
    return [(h[0], tuple(int(v) for v in h[1]), np.float32(h[2]).tobytes()) for h in hits]


def _engine_map(templ, image, method):
    return MTM.computeScoreMap(templ, image, method)


class _Border:
    """The default context's peak border option for the duration of a block (put back afterwards)."""
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.ctx = _lib.default_context()
        self.old = self.ctx.get_option(_lib.OPT_PEAK_BORDER)
        self.ctx.set_option(_lib.OPT_PEAK_BORDER, {"constant": 0, "nearest": 1}[self.name])
        return self

    def __exit__(self, *exc):
        self.ctx.set_option(_lib.OPT_PEAK_BORDER, self.old)


PLANTED = [
    # (chans, method, N_object, maxOverlap, factor, searchBox, border)
    (1, 5, float("inf"), 0.25, 2, None, "nearest"),
    (1, 5, 3, 0.0, 3, None, "constant"),
    (1, 5, 1, 0.25, 4, None, "nearest"),
    (1, 3, float("inf"), 0.0, 2, (7, 5, 180, 150), "nearest"),
    (1, 1, float("inf"), 0.25, 3, None, "nearest"),
    (1, 1, 1, 0.25, 2, (3, 11, 190, 140), "constant"),
    (3, 5, float("inf"), 0.25, 2, None, "constant"),
    (3, 5, 3, 0.25, 4, (9, 2, 185, 150), "nearest"),
    (3, 1, float("inf"), 0.0, 3, None, "nearest"),
    (3, 3, 1, 0.25, 2, None, "nearest"),
]


@pytest.mark.parametrize("chans,method,n_obj,overlap,f,box,border", PLANTED)
def test_planted_objects_equal_match_templates(chans, method, n_obj, overlap, f, box, border):
    img, units = P.planted(100 + chans * 10 + method, chans=chans)
    # thresholds that only the copies pass: the flat background scores ~0.15 (method 1) and ~0.98 (method 3, not centred)
    thr = {1: 0.05, 3: 0.995, 5: 0.6}[method]
    with _Border(border):
        exp = MTM.matchTemplates(units, img, method, N_object=n_obj, score_threshold=thr, maxOverlap=overlap,
                                 searchBox=box)
        got = MTM.matchTemplatesPyramid(units, img, f, method, N_object=n_obj, score_threshold=thr, maxOverlap=overlap,
                                        searchBox=box, radius=2 * f)
    assert len(exp) > 0
    assert _key(got) == _key(exp)


@pytest.mark.parametrize("chans", [1, 3])
@pytest.mark.parametrize("method", [1, 3, 5])
@pytest.mark.parametrize("border", ["nearest", "constant"])
def test_whole_map_windows_equal_find_matches(chans, method, border):
    img, units = P.random_with_flats(200 + chans + method, chans=chans)
    H, W = img.shape[:2]
    thr = 0.2 if method == 1 else 0.3
    cthr = 2.0 if method == 1 else -2.0
    with _Border(border):
        exp = MTM.findMatches(units, img, method, score_threshold=thr)
        for f in (2, 3):
            got = MTM.findMatchesPyramid(units, img, f, method, score_threshold=thr, coarse_threshold=cthr,
                                         radius=max(H, W))
            assert _key(got) == _key(exp)


@pytest.mark.parametrize("chans", [1, 3])
@pytest.mark.parametrize("method", [1, 3, 5])
@pytest.mark.parametrize("border", ["nearest", "constant"])
def test_partial_coverage_equals_the_restatement(chans, method, border):
    img, units = P.random_with_flats(300 + chans + method, chans=chans)
    thr = 0.5 if method == 1 else 0.1
    cthr = 0.8 if method == 1 else 0.0
    with _Border(border):
        for f in (2, 3):
            for mc in (1, 4):
                for r in (0, 1, f):
                    for n_obj in (float("inf"), 1):
                        got = MTM.findMatchesPyramid(units, img, f, method, N_object=n_obj, score_threshold=thr,
                                                     coarse_threshold=cthr, radius=r, max_candidates=mc)
                        exp = P.find_matches_pyramid(units, img, f, method, N_object=n_obj, score_threshold=thr,
                                                     coarse_threshold=cthr, radius=r, max_candidates=mc, border=border,
                                                     score_map=_engine_map)
                        assert _key(got) == _key(exp), (f, mc, r, n_obj)
                        maps = {u[0]: _engine_map(u[1], img, method) for u in units}
                        for label, (x, y, w, h), s in got:
                            assert np.float32(s).tobytes() == maps[label][y, x].tobytes()


def test_large_rgb_template_scores_equal_compute_score_map():
    rng = np.random.RandomState(5)
    img = rng.randint(0, 256, size=(1024, 1024, 3)).astype(np.uint8)
    t = np.ascontiguousarray(img[400:700, 300:580])                 # 300 x 280 x 3: 255^2 x taps > 2^32
    img[100:400, 650:930] = t                                       # and a second copy
    units = [("big", t)]
    m = _engine_map(t, img, 5)
    got = MTM.findMatchesPyramid(units, img, 4, 5, score_threshold=0.05, coarse_threshold=0.0, max_candidates=6)
    assert len(got) >= 2
    for _, (x, y, w, h), s in got:
        assert (w, h) == (280, 300)
        assert np.float32(s).tobytes() == m[y, x].tobytes()
    exp = P.find_matches_pyramid(units, img, 4, 5, score_threshold=0.05, coarse_threshold=0.0, max_candidates=6,
                                 score_map=lambda tt, ii, mm: m if tt.shape == t.shape and ii.shape == img.shape
                                 else _engine_map(tt, ii, mm))
    assert _key(got) == _key(exp)
    best = MTM.matchTemplatesPyramid(units, img, 4, 5, N_object=1)
    assert len(best) == 1 and _key(best) == _key(MTM.matchTemplates(units, img, 5, N_object=1))


@pytest.mark.parametrize("method", [2, 4])
@pytest.mark.parametrize("chans", [1, 3])
def test_raw_sum_methods_with_an_explicit_coarse_threshold(method, chans):
    img, units = P.planted(400 + method + chans, hw=(120, 150), side=20, chans=chans)
    small = augment.downscale(img, 2)
    cmaps = [_engine_map(augment.downscale(u[1], 2), small, method) for u in units]
    fmaps = [_engine_map(u[1], img, method) for u in units]
    cthr = float(np.quantile(np.concatenate([c.ravel() for c in cmaps]), 0.9))
    thr = float(np.quantile(np.concatenate([f.ravel() for f in fmaps]), 0.95))
    for n_obj in (float("inf"), 1):
        got = MTM.findMatchesPyramid(units, img, 2, method, N_object=n_obj, score_threshold=thr, coarse_threshold=cthr,
                                     max_candidates=16)
        exp = P.find_matches_pyramid(units, img, 2, method, N_object=n_obj, score_threshold=thr, coarse_threshold=cthr,
                                     max_candidates=16, score_map=_engine_map)
        assert len(exp) > 0
        assert _key(got) == _key(exp)


def test_abi_overflow_protocol_and_the_context_afterwards():
    img, units = P.random_with_flats(77)
    ctx = _lib.default_context()
    before = MTM.matchTemplates(units, img, 5, score_threshold=0.2)
    with ctx.lock:
        ctx.set_templates([(u[1], None) for u in units], 5)
        full = ctx.find_matches_pyramid(img, 2, _lib.PEAKS_LOCAL, 0.0, 0.1, 2, 8)
        assert len(full) > 2
        a, ptr, stride = _lib._pixel_rows(img)
        out = np.empty(1, dtype=_lib.HIT_DTYPE)
        n = ctypes.c_int64(0)
        rc = ctx._lib.mtm_find_matches_pyramid(ctx._h, ptr, img.shape[0], img.shape[1], 1, _lib.MTM_U8, stride, 2,
                                               _lib.PEAKS_LOCAL, 0.0, 0.1, 2, 8, out.ctypes.data, 1, ctypes.byref(n))
        assert rc == _lib.E_OVERFLOW and n.value == len(full)
        rest = np.empty(n.value, dtype=_lib.HIT_DTYPE)
        assert ctx._lib.mtm_last_hits(ctx._h, rest.ctypes.data, n.value, ctypes.byref(n)) == 0
        assert rest.tobytes() == full.tobytes()
        # a hit list smaller than the window pass's records: it runs once more with room for all of them, same result
        dense = ctx.find_matches_pyramid(img, 2, _lib.PEAKS_LOCAL, 0.0, -1.0, 4, 64)
        assert len(dense) > 16
        old_cap = ctx.get_option(_lib.OPT_HIT_CAPACITY)
        ctx.set_option(_lib.OPT_HIT_CAPACITY, 16)
        try:
            small = ctx.find_matches_pyramid(img, 2, _lib.PEAKS_LOCAL, 0.0, -1.0, 4, 64)
        finally:
            ctx.set_option(_lib.OPT_HIT_CAPACITY, old_cap)
        assert small.tobytes() == dense.tobytes()
    after = MTM.matchTemplates(units, img, 5, score_threshold=0.2)
    assert _key(after) == _key(before)
