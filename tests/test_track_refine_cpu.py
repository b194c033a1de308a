"""MTM.trackTemplates(refine=...) / TemplateMatcher.track(refine=...) / MTM.tracking.positions without a GPU: the argument
check comes before any native call, what reaches the library with and without refinement, and the Python layer's result
from neighbourhoods that a fake context cuts out of the CPU oracle's score maps."""
import threading
import warnings

import numpy as np
import pytest

import MTM
import mtm_oracle as O
from MTM import _lib, subpixel, tracking
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


class _NoNativeCtx:
    """A matcher's context that raises _NativeCalled on any use but its lock."""
    def __init__(self):
        self.lock = threading.RLock()

    def __getattr__(self, name):
        raise _NativeCalled()


def _cut(smap, x, y):
    out = np.full((3, 3), np.nan, dtype=np.float32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if 0 <= y + dy < smap.shape[0] and 0 <= x + dx < smap.shape[1]:
                out[1 + dy, 1 + dx] = smap[y + dy, x + dx]
    return out


class _OracleCtx:
    """Tracks on the CPU oracle: the records of the loop restated on O.find_matches, and - for track_boxes_nbhd - each
    record's neighbourhood cut out of the oracle's score map of its frame.  Records what reaches it."""
    def __init__(self):
        self.lock = threading.RLock()
        self.calls = []
        self.templates, self.method = None, None

    def set_templates(self, templates, method):
        self.calls.append(("set_templates", len(templates), method))
        self.templates, self.method = [t[0] for t in templates], method

    def _run(self, frames, units, margin, min_score):
        n, t = len(frames), len(units)
        out = np.zeros(n * t, dtype=_lib.HIT_DTYPE)
        nbhd = np.empty((n * t, 3, 3), dtype=np.float32)
        bxs = [(int(u["x0"]), int(u["y0"]), int(u["cols"]), int(u["rows"])) for u in units]
        for f, fr in enumerate(frames):
            for k, u in enumerate(units):
                j = int(u["templ_idx"])
                (_, (x, y, w, h), s), = O.find_matches([("t", self.templates[j])], fr, self.method, 1, searchBox=bxs[k])
                out[f * t + k] = (j, x, y, w, h, s)
                nbhd[f * t + k] = _cut(O.compute_score_map(self.templates[j], fr, self.method), x, y)
                bxs[k] = next_box(bxs[k], ("t", (x, y, w, h), np.float32(s)), margin, fr.shape, self.method, min_score)
        return out, nbhd

    def track_boxes(self, frames, units, margin, min_score):
        self.calls.append(("track", len(frames), units.copy(), margin, min_score))
        return self._run(frames, units, margin, min_score)[0]

    def track_boxes_nbhd(self, frames, units, margin, min_score):
        self.calls.append(("track_nbhd", len(frames), units.copy(), margin, min_score))
        return self._run(frames, units, margin, min_score)


@pytest.fixture
def oracle_ctx(monkeypatch):
    ctx = _OracleCtx()
    monkeypatch.setattr(_lib, "default_context", lambda: ctx)
    return ctx


def _scene(seed, n_frames=4, hw=(32, 40), templ_hw=(5, 6), n_tracks=3, margin=3, chans=1, dtype=np.uint8):
    rng = np.random.RandomState(seed)
    shape = hw if chans == 1 else hw + (chans,)
    th, tw = templ_hw
    top = 256 if dtype == np.uint8 else 65536
    templs = [("o%d" % k, rng.randint(0, top, size=templ_hw if chans == 1 else templ_hw + (chans,)).astype(dtype))
              for k in range(n_tracks)]
    pos = [[int(rng.randint(0, hw[1] - tw + 1)), int(rng.randint(0, hw[0] - th + 1))] for _ in range(n_tracks)]
    frames = []
    for _ in range(n_frames):
        fr = (rng.randint(0, top, size=shape) // 4).astype(dtype)
        for k in range(n_tracks):
            x, y = pos[k]
            fr[y:y + th, x:x + tw] = templs[k][1]
        frames.append(fr)
        for p in pos:
            p[0] = int(np.clip(p[0] + rng.randint(-1, 2), 0, hw[1] - tw))
            p[1] = int(np.clip(p[1] + rng.randint(-1, 2), 0, hw[0] - th))
    starts = [((max(0, x - margin), max(0, y - margin), tw + 2 * margin, th + 2 * margin), k)
              for k, (x, y) in enumerate(pos)]
    return templs, frames, starts


# ---- the argument check ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [1, 0, None, "yes", 1.0, np.bool_(True), [True]], ids=repr)
def test_refine_must_be_a_bool_before_any_native_call(no_native, refine):
    templs, frames, tracks = _scene(1)
    with pytest.raises(ValueError, match="refine"):
        MTM.trackTemplates(templs, frames, tracks, 3, 5, refine=refine)
    m = MTM.TemplateMatcher(templs, 5, context=_NoNativeCtx())
    with pytest.raises(ValueError, match="refine"):
        m.track(frames, tracks, 3, refine=refine)
    with pytest.raises(ValueError, match="refine"):        # (also with nothing to track)
        MTM.trackTemplates(templs, frames, [], 3, 5, refine=refine)


def test_refine_is_keyword_only():
    templs, frames, tracks = _scene(1)
    with pytest.raises(TypeError):
        MTM.trackTemplates(templs, frames, tracks, 3, 5, None, True)
    with pytest.raises(TypeError):
        MTM.TemplateMatcher(templs, 5, context=_NoNativeCtx()).track(frames, tracks, 3, None, True)


def test_other_argument_errors_come_first_with_refine(no_native):
    templs, frames, tracks = _scene(1)
    with pytest.raises(ValueError, match="margin"):
        MTM.trackTemplates(templs, frames, tracks, -1, 5, refine=True)
    with pytest.raises(ValueError, match="min_score"):
        MTM.trackTemplates(templs, frames, tracks, 3, 5, "0.5", refine=True)


# ---- what reaches the library ------------------------------------------------------------------------------------------
def test_unrefined_call_reaches_track_boxes_with_four_arguments(oracle_ctx):
    templs, frames, tracks = _scene(2)
    seen = []
    oracle_ctx.track_boxes = lambda *a, **k: (seen.append((a, k)), _OracleCtx._run(oracle_ctx, *a))[1][0]
    oracle_ctx.track_boxes_nbhd = None          # (must not be touched)
    MTM.trackTemplates(templs, frames, tracks, 3, 5, 0.5)
    MTM.trackTemplates(templs, frames, tracks, 3, 5, 0.5, refine=False)
    assert len(seen) == 2
    for a, k in seen:
        assert len(a) == 4 and k == {}
        assert len(a[0]) == len(frames) and len(a[1]) == len(tracks) and a[2:] == (3, 0.5)


def test_refined_call_reaches_track_boxes_nbhd(oracle_ctx):
    templs, frames, tracks = _scene(2)
    MTM.trackTemplates(templs, frames, tracks, 3, 5, 0.5, refine=True)
    kinds = [c[0] for c in oracle_ctx.calls]
    assert kinds == ["set_templates", "track_nbhd"]
    _, n, units, margin, min_score = oracle_ctx.calls[1]
    assert (n, margin, min_score) == (len(frames), 3, 0.5) and len(units) == len(tracks)
    m = MTM.TemplateMatcher(templs, 5, context=oracle_ctx)
    del oracle_ctx.calls[:]
    m.track(frames, tracks, 3, refine=True)
    m.track(frames, tracks, 3)
    assert [c[0] for c in oracle_ctx.calls] == ["set_templates", "track_nbhd", "set_templates", "track"]
    assert m._uploaded_for == ("uint8", 1)


# ---- the Python layer's result -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("chans,dtype", [(1, np.uint8), (3, np.uint8), (1, np.uint16)])
@pytest.mark.parametrize("method", range(6))
def test_refined_result_is_the_fit_of_the_neighbourhoods(oracle_ctx, method, chans, dtype):
    templs, frames, tracks = _scene(10 + method, chans=chans, dtype=dtype)
    res = MTM.trackTemplates(templs, frames, tracks, 3, method)
    got = MTM.trackTemplates(templs, np.stack(frames), tracks, 3, method, refine=True)
    n, t = len(frames), len(tracks)
    assert len(got) == n and all(len(r) == t and all(len(c) == 1 for c in r) for r in got)
    # the fake's own neighbourhoods of the unrefined records, fitted as refineHits fits them
    flat = [res[f][k][0] for f in range(n) for k in range(t)]
    nbhd = np.stack([_cut(O.compute_score_map(templs[k][1], frames[f], method), *res[f][k][0][1][:2])
                     for f in range(n) for k in range(t)])
    exp = subpixel._refined(flat, nbhd, method)
    ox, oy = subpixel.fit_offsets(nbhd, method)
    moved = 0
    for f in range(n):
        for k in range(t):
            (label, (xf, yf, w, h), s), = got[f][k]
            e = exp[f * t + k]
            u = res[f][k][0]
            assert type(xf) is float and type(yf) is float and type(w) is int and type(h) is int
            assert isinstance(s, np.float32) and s.tobytes() == u[2].tobytes()
            assert (label, xf, yf, w, h) == (e[0],) + tuple(e[1])
            assert (label, w, h) == (u[0], u[1][2], u[1][3])
            assert xf == u[1][0] + float(ox[f * t + k]) and yf == u[1][1] + float(oy[f * t + k])
            assert abs(xf - u[1][0]) <= 0.5 and abs(yf - u[1][1]) <= 0.5      # the integer part is the unrefined call's
            moved += (xf != u[1][0]) or (yf != u[1][1])
    assert moved > 0


def test_refinement_does_not_feed_back_and_failed_hits_are_refined(oracle_ctx):
    templs, frames, tracks = _scene(21, n_frames=5)
    frames[2] = np.random.RandomState(99).randint(0, 64, size=frames[2].shape).astype(np.uint8)   # no objects: hits fail
    res = MTM.trackTemplates(templs, frames, tracks, 3, 5, 0.9)
    got = MTM.trackTemplates(templs, frames, tracks, 3, 5, 0.9, refine=True)
    assert any(float(c[0][2]) < 0.9 for c in res[2])
    for fr, gr in zip(res, got):
        for (u,), (g,) in zip(fr, gr):
            assert (g[0], g[1][2:], g[2].tobytes()) == (u[0], u[1][2:], u[2].tobytes())
            assert abs(g[1][0] - u[1][0]) <= 0.5 and abs(g[1][1] - u[1][1]) <= 0.5


def test_mask_warnings_with_and_without_refine(oracle_ctx):
    templs, frames, tracks = _scene(5, n_frames=4)
    masked = [(t[0], t[1], np.ones_like(t[1])) for t in templs[:2]] + templs[2:]

    def count(**kw):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            MTM.trackTemplates(masked, frames, tracks, 3, 5, **kw)
        return len(w)
    assert count() == count(refine=True) == 2 * 4


def test_duplicate_labels_are_no_error(oracle_ctx):
    templs, frames, tracks = _scene(6)
    same = [("x", t[1]) for t in templs]
    got = MTM.trackTemplates(same, frames, tracks, 3, 5, refine=True)
    exp = MTM.trackTemplates(templs, frames, tracks, 3, 5, refine=True)
    assert [[c[0][1:] for c in fr] for fr in got] == [[c[0][1:] for c in fr] for fr in exp]
    assert {c[0][0] for fr in got for c in fr} == {"x"}


def test_zero_frames_and_zero_tracks(oracle_ctx):
    templs, frames, tracks = _scene(7)
    assert MTM.trackTemplates(templs, [], tracks, 3, refine=True) == []
    assert MTM.trackTemplates(templs, np.zeros((0, 32, 40), np.uint8), tracks, 3, refine=True) == []
    assert MTM.trackTemplates(templs, frames, [], 3, refine=True) == [[] for _ in frames]
    m = MTM.TemplateMatcher(templs, 5, context=oracle_ctx)
    assert m.track(frames, [], 3, refine=True) == [[] for _ in frames] and m.track([], tracks, 3, refine=True) == []
    assert oracle_ctx.calls == []


# ---- positions ---------------------------------------------------------------------------------------------------------
def test_positions_of_hand_made_results():
    s = np.float32(0.5)
    res = [[[("a", (1, 2, 5, 6), s)], [("b", (3.25, 4.5, 5, 6), s)]],
           [[("a", (7, 8, 5, 6), s)], [("b", (9.0, 10.75, 5, 6), s)]],
           [[("a", (0, 0, 5, 6), s)], [("b", (-0.5, 0.5, 5, 6), s)]]]
    p = tracking.positions(res)
    assert p.shape == (3, 2, 2) and p.dtype == np.float64
    assert p.tolist() == [[[1.0, 2.0], [3.25, 4.5]], [[7.0, 8.0], [9.0, 10.75]], [[0.0, 0.0], [-0.5, 0.5]]]
    assert tracking.positions([]).shape == (0, 0, 2)
    assert tracking.positions([[], []]).shape == (2, 0, 2)
    assert "positions" in tracking.__all__


@pytest.mark.parametrize("bad", [
    [[[("a", (1, 2, 5, 6), 0.5)], []]],                                               # no hit
    [[[("a", (1, 2, 5, 6), 0.5), ("a", (2, 2, 5, 6), 0.4)]]],                         # two hits
    [[[("a", (1, 2, 5, 6), 0.5)]], [[("a", (1, 2, 5, 6), 0.5)], [("b", (1, 2, 5, 6), 0.5)]]],   # ragged frames
])
def test_positions_needs_one_hit_per_frame_and_track(bad):
    with pytest.raises(ValueError, match="positions"):
        tracking.positions(bad)


def test_positions_of_a_tracked_result(oracle_ctx):
    templs, frames, tracks = _scene(8)
    res = MTM.trackTemplates(templs, frames, tracks, 3, 5)
    got = MTM.trackTemplates(templs, frames, tracks, 3, 5, refine=True)
    assert tracking.positions(res).tolist() == [[list(map(float, c[0][1][:2])) for c in fr] for fr in res]
    assert tracking.positions(got).tolist() == [[list(c[0][1][:2]) for c in fr] for fr in got]


def test_context_has_the_native_entry_point():
    assert "mtm_track_boxes_nbhd" in _lib.SYMBOLS
    assert len(_lib.SYMBOLS["mtm_track_boxes_nbhd"][1]) == len(_lib.SYMBOLS["mtm_track_boxes"][1]) + 1
    assert callable(_lib.Context.track_boxes_nbhd)
