"""MTM.trackTemplates / TemplateMatcher.track / MTM.tracking.next_box without a GPU: every argument error and frame-0 error
of the findMatchesInBoxes loop it replaces is raised (type, message, warnings) before anything reaches the library, the box
update rule at every edge and with min_score, what reaches the library, and the loop restated on the CPU oracle."""
import threading
import warnings

import numpy as np
import pytest

import MTM
import mtm_oracle as O
from MTM import _lib, tracking
from MTM.tracking import next_box


class _NativeCalled(Exception):
    pass


@pytest.fixture
def no_native(monkeypatch):
    """Any use of the library raises _NativeCalled: an error that comes first was raised in the Python layer."""
    def boom(*a, **k):
        raise _NativeCalled()
    monkeypatch.setattr(_lib, "default_context", boom)
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_lib, "engine_for", boom)


class _FakeCtx:
    """Records what would reach the library.  Boxes calls return no hits; track calls return one record per (frame, track)
    at the track's frame-0 box origin."""
    def __init__(self):
        self.lock = threading.RLock()
        self.calls = []

    def set_templates(self, templates, method):
        self.calls.append(("set_templates", [t[0].shape for t in templates], method))

    def find_matches_boxes(self, image, units, mode, thr):
        self.calls.append(("boxes", units.copy(), mode, thr))
        return np.zeros(0, dtype=_lib.HIT_DTYPE), np.zeros(len(units), np.int64)

    def track_boxes(self, frames, units, margin, min_score):
        self.calls.append(("track", len(frames), units.copy(), margin, min_score))
        out = np.zeros(len(frames) * len(units), dtype=_lib.HIT_DTYPE)
        for f in range(len(frames)):
            rec = out[f * len(units):(f + 1) * len(units)]
            rec["templ_idx"], rec["x"], rec["y"] = units["templ_idx"], units["x0"], units["y0"]
            rec["score"] = 0.25
        return out


class _NoNativeCtx:
    """A matcher's context that raises _NativeCalled on any use but its lock."""
    def __init__(self):
        self.lock = threading.RLock()

    def __getattr__(self, name):
        raise _NativeCalled()


@pytest.fixture
def fake_ctx(monkeypatch):
    ctx = _FakeCtx()
    monkeypatch.setattr(_lib, "default_context", lambda: ctx)
    return ctx


def _img(h=64, w=80, chans=1, dtype=np.uint8, seed=0):
    rng = np.random.RandomState(seed)
    shape = (h, w) if chans == 1 else (h, w, chans)
    return rng.randint(0, 256, size=shape).astype(dtype)


def _frames(n=3, **kw):
    return [_img(seed=s, **kw) for s in range(n)]


def _templs(img, n=2):
    return [("t%d" % i, np.ascontiguousarray(img[3 * i:3 * i + 6, 2 * i:2 * i + 5])) for i in range(n)]


def _loop(templs, frames, tracks, margin, method=5, min_score=None):
    """The loop trackTemplates replaces (MTM/tracking.py), on MTM.findMatchesInBoxes."""
    out, bxs = [], [b for b, _ in tracks]
    for f in frames:
        r = MTM.findMatchesInBoxes(templs, f, [(b, [j]) for b, (_, j) in zip(bxs, tracks)], method, N_object=1)
        out.append(r)
        bxs = [next_box(b, ri[0] if ri else None, margin, f.shape, method, min_score) for b, ri in zip(bxs, r)]
    return out


def _outcome(call):
    """(result, (exception type, message) or None, number of warnings)"""
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        try:
            r, e = call(), None
        except _NativeCalled:
            raise
        except Exception as ex:  # noqa: BLE001 - compared with the loop's
            r, e = None, (type(ex), str(ex))
    return r, e, len(w)


# ---- next_box --------------------------------------------------------------------------------------------------------
H, W = 50, 70


@pytest.mark.parametrize("hit_xy, margin, want", [
    ((30, 20), 5, (25, 15, 18, 16)),            # inside
    ((2, 20), 5, (0, 15, 15, 16)),              # left edge
    ((30, 1), 5, (25, 0, 18, 12)),              # top edge
    ((62, 20), 5, (57, 15, 13, 16)),            # right edge: x1 = W
    ((30, 44), 5, (25, 39, 18, 11)),            # bottom edge: y1 = H
    ((0, 0), 5, (0, 0, 13, 11)),                # top-left corner
    ((62, 44), 5, (57, 39, 13, 11)),            # bottom-right corner
    ((30, 20), 0, (30, 20, 8, 6)),              # margin 0: the hit's own box
    ((62, 44), 0, (62, 44, 8, 6)),
    ((30, 20), 1000, (0, 0, W, H)),             # a margin past the frame: the whole frame
])
def test_next_box_edges(hit_xy, margin, want):
    hit = ("t", (hit_xy[0], hit_xy[1], 8, 6), np.float32(0.9))
    got = next_box((1, 2, 3, 4), hit, margin, (H, W), 5)
    assert got == want
    x, y, w, h = got
    assert 0 <= x and 0 <= y and x + w <= W and y + h <= H
    assert w >= 8 and h >= 6                    # the template always fits


@pytest.mark.parametrize("method, score, min_score, moves", [
    (5, 0.9, 0.5, True), (5, 0.5, 0.5, False), (5, 0.4, 0.5, False), (2, 1e6, 1e5, True), (4, -1.0, 0.0, False),
    (3, 0.91, 0.9, True), (0, 10.0, 20.0, True), (0, 20.0, 20.0, False), (0, 30.0, 20.0, False),
    (1, 0.1, 0.2, True), (1, 0.3, 0.2, False),
    (5, float("nan"), 0.5, False), (1, float("nan"), 0.5, False), (5, float("nan"), None, True),
    (5, 0.9, float("nan"), False), (1, 0.1, float("nan"), False),
    (5, -5.0, None, True), (1, 5.0, None, True),
])
def test_next_box_min_score(method, score, min_score, moves):
    box = (3, 4, 20, 20)
    hit = ("t", (10, 12, 8, 6), np.float32(score))
    got = next_box(box, hit, 2, (H, W), method, min_score)
    assert got == ((8, 10, 12, 10) if moves else box)


def test_next_box_without_a_hit_keeps_the_box():
    assert next_box([3, 4, 20, 20], None, 2, (H, W), 5) == (3, 4, 20, 20)
    assert next_box((3, 4, 20, 20), None, 2, (H, W), 1, 0.5) == (3, 4, 20, 20)


def test_next_box_compares_min_score_as_python_floats():
    # a float32 score just above a threshold that rounds to it in float32 still passes
    s = np.float32(0.1)
    assert float(s) > 0.1 and np.float32(0.1) == s
    hit = ("t", (10, 12, 8, 6), s)
    assert next_box((0, 0, 30, 30), hit, 1, (H, W), 5, 0.1) == (9, 11, 10, 8)
    assert next_box((0, 0, 30, 30), hit, 1, (H, W), 1, 0.1) == (0, 0, 30, 30)


# ---- argument and scope errors before any native call --------------------------------------------------------------
def _errs():
    f = _frames()
    t = _templs(f[0])
    return [
        # (description, templates, frames, tracks, margin, method, min_score, exception, fragment)
        ("negative margin", t, f, [((0, 0, 30, 30), 0)], -1, 5, None, ValueError, "margin"),
        ("float margin", t, f, [((0, 0, 30, 30), 0)], 1.5, 5, None, ValueError, "margin"),
        ("bool margin", t, f, [((0, 0, 30, 30), 0)], True, 5, None, ValueError, "margin"),
        ("string margin", t, f, [((0, 0, 30, 30), 0)], "3", 5, None, ValueError, "margin"),
        ("frames of two shapes", t, [f[0], f[1][:60]], [((0, 0, 30, 30), 0)], 4, 5, None, ValueError, "shape"),
        ("frames of two dtypes", t, [f[0], f[1].astype(np.uint16)], [((0, 0, 30, 30), 0)], 4, 5, None, ValueError, "dtype"),
        ("a frame that is a list", t, [f[0], f[1].tolist()], [((0, 0, 30, 30), 0)], 4, 5, None, ValueError, "numpy"),
        ("a 2-D array as frames", t, f[0], [((0, 0, 30, 30), 0)], 4, 5, None, ValueError, "shape"),
        ("min_score text", t, f, [((0, 0, 30, 30), 0)], 4, 5, "0.5", ValueError, "min_score"),
    ]


@pytest.mark.parametrize("case", _errs(), ids=lambda c: c[0])
def test_argument_errors_before_native(no_native, case):
    _, templs, frames, tracks, margin, method, min_score, exc, frag = case
    with pytest.raises(exc, match=frag):
        MTM.trackTemplates(templs, frames, tracks, margin, method, min_score)
    m = MTM.TemplateMatcher(templs, method, context=_NoNativeCtx())
    with pytest.raises(exc, match=frag):
        m.track(frames, tracks, margin, min_score)


def _frame0_cases():
    f = _frames()
    t = _templs(f[0])
    f3 = _frames(chans=3)
    big = [("big", _img(40, 40))]
    return [
        # (description, templates, frames, tracks, method): the loop's first call raises
        ("float32 frames", t, [a.astype(np.float32) for a in f], [((0, 0, 30, 30), 0)], 5),
        ("2-channel frames", t, _frames(chans=2), [((0, 0, 30, 30), 0)], 5),
        ("3-channel uint16 frames", t, _frames(chans=3, dtype=np.uint16), [((0, 0, 30, 30), 0)], 5),
        ("template of another dtype", [("a", _img(8, 8, dtype=np.uint16))], f, [((0, 0, 30, 30), 0)], 5),
        ("channel mismatch", t, f3, [((0, 0, 30, 30), 0)], 5),
        ("method 6", t, f, [((0, 0, 30, 30), 0)], 6),
        ("method -1", t, f, [((0, 0, 30, 30), 0)], -1),
        ("mask with method 3", [("a", _img(8, 8), np.ones((8, 8), np.uint8))], f, [((0, 0, 30, 30), 0)], 3),
        ("mask with method 0", [("a", _img(8, 8), np.ones((8, 8), np.uint8))], f, [((0, 0, 30, 30), 0)], 0),
        ("negative x", t, f, [((0, 0, 30, 30), 0), ((-1, 0, 30, 30), 1)], 5),
        ("negative y", t, f, [((2, -5, 30, 30), 0)], 5),
        ("template larger than box", t, f, [((0, 0, 30, 30), 0), ((10, 10, 4, 30), 1)], 5),
        ("template larger than clipped box", big, f, [((50, 0, 40, 40), 0)], 5),
        ("box past the frame", t, f, [((90, 0, 30, 30), 0)], 5),
        ("template index out of range", t, f, [((0, 0, 30, 30), 0), ((0, 0, 30, 30), 2)], 5),
        ("negative template index out of range", t, f, [((0, 0, 30, 30), -3)], 5),
        ("template index not an integer", t, f, [((0, 0, 30, 30), 0.5)], 5),
        ("box of three values", t, f, [((0, 0, 30), 0)], 5),
        ("box values not integers", t, f, [((0, 0.5, 30, 30), 0)], 5),
        ("not a template tuple", [t[0], ["x", t[1][1]]], f, [((0, 0, 30, 30), 1)], 5),
        ("template of height 0", [("z", np.zeros((0, 4), np.uint8))], f, [((0, 0, 30, 30), 0)], 5),
        ("template of width 0", [("z", np.zeros((4, 0), np.uint8))], f, [((0, 0, 30, 30), 0)], 5),
        ("mask slot warnings, then a larger template", [("m", _img(6, 6), None), ("big", _img(40, 40))], f,
         [((0, 0, 30, 30), 0), ((0, 0, 30, 30), 1)], 5),
        ("frames of height 0", t, [np.zeros((0, 5), np.uint8)] * 2, [((0, 0, 30, 30), 0)], 5),
        ("a track that is not a pair", t, f, [((0, 0, 30, 30), 0, 1)], 5),
        ("a track that is a number", t, f, [5], 5),
    ]


@pytest.mark.parametrize("case", _frame0_cases(), ids=lambda c: c[0])
def test_frame0_errors_and_warnings_equal_the_loop(no_native, case):
    _, templs, frames, tracks, method = case
    exp = _outcome(lambda: _loop(templs, frames, tracks, 4, method))
    assert exp[1] is not None, "the loop raises before its first native call"
    got = _outcome(lambda: MTM.trackTemplates(templs, frames, tracks, 4, method))
    assert got[1:] == exp[1:]


def test_matcher_checks_every_resident_template(no_native):
    f = _frames()
    templs = _templs(f[0]) + [("u16", _img(5, 5, dtype=np.uint16))]
    m = MTM.TemplateMatcher(templs, 5, context=_NoNativeCtx())
    with pytest.raises(ValueError, match="dtype"):
        m.track(f, [((0, 0, 30, 30), 0)], 4)       # the unused uint16 template would be set on the context too


def test_matcher_refuses_while_streaming():
    m = MTM.TemplateMatcher(_templs(_img()), 5, context=_NoNativeCtx())
    m._streaming = True
    with pytest.raises(RuntimeError, match="match_stream"):
        m.track(_frames(), [((0, 0, 30, 30), 0)], 4)


# ---- what reaches the library ----------------------------------------------------------------------------------------
def test_empty_inputs(fake_ctx):
    f = _frames()
    t = _templs(f[0])
    assert MTM.trackTemplates(t, [], [((0, 0, 30, 30), 0)], 4) == []
    assert MTM.trackTemplates(t, np.zeros((0, 64, 80), np.uint8), [((0, 0, 30, 30), 0)], 4) == []
    assert MTM.trackTemplates(t, f, [], 4) == [[], [], []]
    assert fake_ctx.calls == []
    assert _loop(t, f, [], 4) == [[], [], []] and _loop(t, [], [((0, 0, 30, 30), 0)], 4) == []


def test_units_templates_and_clipping(fake_ctx):
    f = _frames(4)
    t = _templs(f[0], 3)
    tracks = [((70, 50, 30, 30), 2), ((0, 0, 12, 9), -1), ((5, 6, 20, 20), 0)]
    res = MTM.trackTemplates(t, np.stack(f), tracks, 3, 1, 0.5)
    (kind, n, units, margin, min_score), = [c for c in fake_ctx.calls if c[0] == "track"]
    assert (n, margin, min_score) == (4, 3, 0.5)
    assert fake_ctx.calls[0] == ("set_templates", [(6, 5), (6, 5)], 1)      # only the used templates, in list order
    assert units["templ_idx"].tolist() == [1, 1, 0]
    assert units[["y0", "x0", "rows", "cols"]].tolist() == [(50, 70, 14, 10), (0, 0, 9, 12), (6, 5, 20, 20)]
    assert len(res) == 4 and all(len(r) == 3 and all(len(e) == 1 for e in r) for r in res)
    assert res[2][0][0] == ("t2", (70, 50, 0, 0), np.float32(0.25))      # (the fake leaves w, h at 0)
    assert res[3][2][0][0] == "t0"
    assert isinstance(res[0][0][0][2], np.float32)


def test_huge_margin_reaches_the_library_clipped(fake_ctx):
    f = _frames(2)
    MTM.trackTemplates(_templs(f[0]), f, [((0, 0, 30, 30), 0)], 10 ** 12)
    assert [c for c in fake_ctx.calls if c[0] == "track"][0][3] == 80


def test_mask_warnings_per_frame_as_the_loop(fake_ctx):
    f = _frames(5)
    t = [("m", _img(6, 6), np.ones((6, 6), np.uint8)), ("p", _img(5, 7))]
    tracks = [((0, 0, 30, 30), 0), ((10, 10, 30, 30), 1), ((3, 3, 30, 30), 0)]
    exp = _outcome(lambda: _loop(t, f, tracks, 4, 5))
    got = _outcome(lambda: MTM.trackTemplates(t, f, tracks, 4, 5))
    assert exp[2] == got[2] == 2 * 5


def test_matcher_records_resident_templates_only_when_set(fake_ctx):
    f = _frames(2)
    m = MTM.TemplateMatcher(_templs(f[0], 3), 5, context=fake_ctx)
    m.track(f, [], 3)
    assert m._uploaded_for is None and fake_ctx.calls == []
    m.track(f, [((0, 0, 30, 30), 1)], 3)
    assert fake_ctx.calls[0] == ("set_templates", [(6, 5)] * 3, 5)     # the whole list, resident
    assert fake_ctx.calls[1][2]["templ_idx"].tolist() == [1]
    assert m._uploaded_for == ("uint8", 1)


# ---- the loop restated on the CPU oracle -----------------------------------------------------------------------------
def track_restated(templs, frames, tracks, margin, method, min_score=None):
    """The loop on the oracle: each track's frame crop, the oracle's find_matches with N_object=1 on it, next_box."""
    out, bxs = [], [tuple(b) for b, _ in tracks]
    for f in frames:
        r = [O.find_matches([templs[j]], f, method, 1, searchBox=b) for b, (_, j) in zip(bxs, tracks)]
        out.append(r)
        bxs = [next_box(b, ri[0] if ri else None, margin, f.shape, method, min_score) for b, ri in zip(bxs, r)]
    return out


def _scene(seed, n_frames, hw, templ_hw, n_tracks, margin, chans=1):
    """Noise frames with each track's template pasted at a position that moves up to margin / 2 pixels per frame."""
    rng = np.random.RandomState(seed)
    shape = hw if chans == 1 else hw + (chans,)
    th, tw = templ_hw
    templs = [("o%d" % k, rng.randint(0, 256, size=templ_hw if chans == 1 else templ_hw + (chans,)).astype(np.uint8))
              for k in range(n_tracks)]
    pos = [[int(rng.randint(0, hw[1] - tw + 1)), int(rng.randint(0, hw[0] - th + 1))] for _ in range(n_tracks)]
    frames, truth = [], []
    for _ in range(n_frames):
        fr = (rng.randint(0, 256, size=shape) // 4).astype(np.uint8)
        for k in range(n_tracks):
            x, y = pos[k]
            fr[y:y + th, x:x + tw] = templs[k][1]
        frames.append(fr)
        truth.append([tuple(p) for p in pos])
        for p in pos:
            p[0] = int(np.clip(p[0] + rng.randint(-(margin // 2), margin // 2 + 1), 0, hw[1] - tw))
            p[1] = int(np.clip(p[1] + rng.randint(-(margin // 2), margin // 2 + 1), 0, hw[0] - th))
    starts = [((max(0, x - margin), max(0, y - margin), tw + 2 * margin, th + 2 * margin), k)
              for k, (x, y) in enumerate(truth[0])]
    return templs, frames, starts, truth


@pytest.mark.parametrize("chans", [1, 3])
@pytest.mark.parametrize("method", range(6))
def test_restatement_follows_the_pasted_templates(chans, method):
    templs, frames, tracks, truth = _scene(7 + method, 6, (48, 64), (7, 9), 3, 4, chans)
    res = track_restated(templs, frames, tracks, 4, method)
    assert len(res) == 6
    if method in (1, 3, 5):             # the normalised methods find an exact copy of the template
        for r, tr in zip(res, truth):
            assert [h[0][1][:2] for h in r] == tr
    for f, r in enumerate(res):
        for (box, j), hits in zip(tracks, r):
            assert len(hits) == 1 and hits[0][0] == "o%d" % j


def test_restatement_equals_loop_of_crops():
    """The restatement's searchBox call is the crop search: its hits equal the oracle's find_matches on the crop, offset."""
    templs, frames, tracks, _ = _scene(3, 4, (40, 50), (6, 8), 2, 6)
    res = track_restated(templs, frames, tracks, 6, 5, min_score=0.5)
    bxs = [b for b, _ in tracks]
    for f, r in zip(frames, res):
        for (b, (_, j)), hits in zip(zip(bxs, tracks), r):
            x, y, w, h = b
            crop = f[y:y + h, x:x + w]
            e = O.find_matches([templs[j]], crop, 5, 1)
            assert [(hh[0], (hh[1][0] + x, hh[1][1] + y) + hh[1][2:], np.float32(hh[2]).tobytes()) for hh in e] == \
                [(hh[0], hh[1], np.float32(hh[2]).tobytes()) for hh in hits]
        bxs = [next_box(b, ri[0], 6, f.shape, 5, 0.5) for b, ri in zip(bxs, r)]


def test_restatement_min_score_keeps_the_box_while_the_object_is_gone():
    templs, frames, tracks, truth = _scene(11, 6, (40, 56), (6, 8), 1, 4)
    for f in (2, 3):
        frames[f] = frames[f].copy()
        x, y = truth[f][0]
        frames[f][y:y + 6, x:x + 8] = 7                 # the object is covered for two frames
    got = track_restated(templs, frames, tracks, 20, 5, min_score=0.95)
    assert got[1][0][0][1][:2] == truth[1][0] and float(got[1][0][0][2]) > 0.95
    assert all(float(got[f][0][0][2]) < 0.95 for f in (2, 3))
    assert got[4][0][0][1][:2] == truth[4][0]       # re-acquired from the kept box
