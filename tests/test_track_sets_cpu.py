"""Tracks that carry a set of templates in MTM.trackTemplates / TemplateMatcher.track without a GPU: the Python layer's
result from a stand-in context that runs the defining loop on the CPU oracle, the tie rule, the new argument errors -
before any native call and after the loop's own frame-0 errors -, all-integer tracks through the methods the call used
before, the mask warnings, the matcher's residency record, and the C header."""
import os
import threading
import warnings

import numpy as np
import pytest

import MTM
import mtm_oracle as O
from MTM import _lib, subpixel
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


def _passes(score, method, min_score):
    s, m = float(score), float(min_score)
    return s < m if method in (0, 1) else s > m


def _set(js):
    return [js] if isinstance(js, (int, np.integer)) else list(js)


def sets_loop_restated(templs, frames, tracks, margin, method, min_score=None, reacquire=False):
    """The loop of the issue and of MTM/tracking.py's docstring on the oracle: every variant of the set searched in the
    track's box, the first extreme hit the frame's record; with `reacquire` a record that does not pass is followed by the
    whole-frame search of the set, reduced the same way.  Returns (hits [f][k], the (frame, track) pairs searched twice)."""
    pick = min if method in (0, 1) else max
    box = [tuple(b) for b, _ in tracks]
    out, again = [], []
    for fi, f in enumerate(frames):
        H, W = f.shape[:2]
        row = []
        for k, (_, js) in enumerate(tracks):
            hits = [O.find_matches([templs[j]], f, method, 1, searchBox=box[k])[0] for j in _set(js)]
            hit = pick(hits, key=lambda h: h[2])
            if reacquire and not _passes(hit[2], method, min_score):
                hits = [O.find_matches([templs[j]], f, method, 1, searchBox=(0, 0, W, H))[0] for j in _set(js)]
                hit = pick(hits, key=lambda h: h[2])
                again.append((fi, k))
            row.append([hit])
            box[k] = next_box(box[k], hit, margin, f.shape, method, min_score)
        out.append(row)
    return out, again


class _SetsOracleCtx:
    """track_boxes_sets as the loop on the oracle, in the binding's terms (start units, offsets, indices, records)."""
    def __init__(self):
        self.lock = threading.RLock()
        self.calls = []

    def set_templates(self, templates, method):
        self.templates, self.method = [t[0] for t in templates], method

    def track_boxes_sets(self, frames, start, set_off, set_idx, margin, min_score=None, reacquire=False, with_nbhd=False):
        set_off, set_idx = np.asarray(set_off), np.asarray(set_idx)
        self.calls.append((len(frames), start.copy(), set_off.copy(), set_idx.copy(), margin, min_score, reacquire, with_nbhd))
        assert len(set_off) == len(start) + 1 and set_off[0] == 0 and set_off[-1] == len(set_idx)
        assert start["templ_idx"].tolist() == set_idx[set_off[:-1]].tolist()
        templs = [(i, t) for i, t in enumerate(self.templates)]             # (the label is the index the record names)
        tracks = [((int(u["x0"]), int(u["y0"]), int(u["cols"]), int(u["rows"])), set_idx[a:b].tolist())
                  for u, a, b in zip(start, set_off[:-1], set_off[1:])]
        res, _ = sets_loop_restated(templs, frames, tracks, margin, self.method, min_score, reacquire)
        out = np.zeros(len(frames) * len(start), dtype=_lib.HIT_DTYPE)
        for f, row in enumerate(res):
            for k, ((i, (x, y, w, h), s),) in enumerate(row):
                out[f * len(start) + k] = (i, x, y, w, h, s)
        self.nbhd = None
        if with_nbhd:           # (a made-up neighbourhood with a fractional peak: the fit is subpixel's business)
            self.nbhd = np.zeros((len(out), 3, 3), np.float32)
            self.nbhd[:, 1, 1] = out["score"]
            self.nbhd[:, 1, 2] = out["score"] * np.float32(0.75)
            self.nbhd[:, 1, 0] = out["score"] * np.float32(0.5)
        return out, self.nbhd


def _variants(t):
    """The template and its flips / 180 degree rotation: four appearances of one shape."""
    return [t, t[:, ::-1].copy(), t[::-1].copy(), t[::-1, ::-1].copy()]


def _scene(seed, chans=1, dtype=np.uint8, n_frames=5, hw=(32, 40), templ_hw=(5, 6), n_tracks=3, margin=2, jump=None,
           blank=()):
    """Dim noise frames; track k's object is variant (f + k) % 4 of its template, pasted at a position that drifts by at
    most one pixel per frame, so the winning label changes from frame to frame.  jump = (track, frame): before that frame
    the track's object moves half the map away.  Returns (templates: 4 variants per track, then one unused entry; frames;
    tracks with sets; the (x, y) and variant shown per frame and track)."""
    rng = np.random.RandomState(seed)
    th, tw = templ_hw
    top = 256 if dtype == np.uint8 else 65536
    shape = hw if chans == 1 else hw + (chans,)
    templs = []
    for k in range(n_tracks):
        base = rng.randint(0, top, size=templ_hw if chans == 1 else templ_hw + (chans,)).astype(dtype)
        templs += [("o%d.%d" % (k, v), a) for v, a in enumerate(_variants(base))]
    templs.append(("unused", templs[0][1][:3, :3].copy()))
    pos = [[int(rng.randint(0, hw[1] - tw + 1)), int(rng.randint(0, hw[0] - th + 1))] for _ in range(n_tracks)]
    tracks = [((max(0, x - margin), max(0, y - margin), tw + 2 * margin, th + 2 * margin), [4 * k + v for v in range(4)])
              for k, (x, y) in enumerate(pos)]
    frames, truth = [], []
    for f in range(n_frames):
        if jump and jump[1] == f:
            p = pos[jump[0]]
            p[0] = (p[0] + (hw[1] - tw + 1) // 2) % (hw[1] - tw + 1)
            p[1] = (p[1] + (hw[0] - th + 1) // 2) % (hw[0] - th + 1)
        fr = (rng.randint(0, top, size=shape) // 8).astype(dtype)
        for k in range(n_tracks):
            x, y = pos[k]
            if f not in blank:
                fr[y:y + th, x:x + tw] = templs[4 * k + (f + k) % 4][1]
        frames.append(fr)
        truth.append([(p[0], p[1], (f + k) % 4) for k, p in enumerate(pos)])
        for p in pos:
            p[0] = int(np.clip(p[0] + rng.randint(-1, 2), 0, hw[1] - tw))
            p[1] = int(np.clip(p[1] + rng.randint(-1, 2), 0, hw[0] - th))
    return templs, frames, tracks, truth


def _thr(method, templs):
    if method == 1:
        return 0.05
    if method in (3, 5):
        return 0.95
    if method == 0:
        return 1.0
    t = [np.asarray(t[1], np.float64).reshape(t[1].shape[0], t[1].shape[1], -1) for t in templs]
    if method == 2:
        return 0.9 * min(float((a * a).sum()) for a in t)
    return 0.9 * min(float(((a - a.mean(axis=(0, 1))) ** 2).sum()) for a in t)


def _same(got, exp):
    g, e = got[0], exp[0]
    assert g[0] == e[0]
    assert tuple(g[1]) == tuple(e[1]) and all(type(v) is int for v in g[1])
    assert isinstance(g[2], np.float32) and g[2].tobytes() == np.float32(e[2]).tobytes()


def _same_result(got, exp, n_frames, n_tracks):
    assert len(got) == n_frames and all(len(r) == n_tracks and all(len(c) == 1 for c in r) for r in got)
    for f in range(n_frames):
        for k in range(n_tracks):
            _same(got[f][k], exp[f][k])


# ---- the result is the loop's -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chans,dtype", [(1, np.uint8), (3, np.uint8), (1, np.uint16)])
@pytest.mark.parametrize("method", [0, 1, 2, 3, 4, 5])
def test_set_tracks_result_is_the_loops(monkeypatch, method, chans, dtype):
    templs, frames, tracks, truth = _scene(40 + method, chans=chans, dtype=dtype, jump=(1, 2))
    # mixed: track 0 a tuple with a negative index and a duplicate, track 1 an array, track 2 a plain integer
    tracks = [(tracks[0][0], (0, 1, -11, 3, 1)), (tracks[1][0], np.array([4, 5, 6, 7])), (tracks[2][0], 8 + 2)]
    thr = _thr(method, templs[:12])
    ctx = _SetsOracleCtx()
    monkeypatch.setattr(_lib, "default_context", lambda: ctx)
    for min_score, reacquire in [(None, False), (thr, False), (thr, True)]:
        exp, again = sets_loop_restated(templs, frames, tracks, 2, method, min_score, reacquire)
        got = MTM.trackTemplates(templs, np.stack(frames), tracks, 2, method, min_score, reacquire=reacquire)
        n, start, set_off, set_idx, margin, ms, rq, with_nbhd = ctx.calls[-1]
        assert (n, margin, ms, rq, with_nbhd) == (len(frames), 2, min_score, reacquire, False)
        assert set_off.tolist() == [0, 5, 9, 10]
        assert set_idx.tolist() == [0, 1, 2, 3, 1, 4, 5, 6, 7, 8]       # only the used templates are set, in list order
        _same_result(got, exp, len(frames), len(tracks))
        # the scene does what it is for (where an exact copy is the extremum whatever lies around it: the difference and
        # the normalised methods): the label follows the appearance ...
        if min_score is not None and method in (0, 1, 3, 5):
            for f in range(len(frames)):
                if reacquire or f < 2:
                    assert [got[f][k][0][0] for k in (0, 1)] == ["o%d.%d" % (k, truth[f][k][2]) for k in (0, 1)]
            assert all(row[2][0][0] == "o2.2" for row in got)           # ... and an integer track keeps its own
        if reacquire and method in (0, 1, 3, 5):                # ... and the jump is searched twice and found
            assert (2, 1) in again and tuple(got[2][1][0][1][:2]) == truth[2][1][:2]
    # refined: the fit of the final records' neighbourhoods, with the winner's label
    plain = MTM.trackTemplates(templs, frames, tracks, 2, method, thr, reacquire=True)
    ref = MTM.trackTemplates(templs, frames, tracks, 2, method, thr, reacquire=True, refine=True)
    assert ctx.calls[-1][7] is True
    flat = [plain[f][k][0] for f in range(len(frames)) for k in range(len(tracks))]
    assert [r[0] for row in ref for r in row] == subpixel._refined(flat, ctx.nbhd, method)
    assert all(type(r[0][1][0]) is float for row in ref for r in row)
    assert MTM.tracking.positions(ref).shape == (len(frames), 3, 2)
    assert MTM.tracking.lost(plain, method, thr).shape == (len(frames), 3)


@pytest.mark.parametrize("method", [1, 5])
@pytest.mark.parametrize("order", [(0, 1), (1, 0)], ids=["a first", "b first"])
def test_identical_variants_the_first_in_set_order_wins(monkeypatch, method, order):
    templs, frames, tracks, _ = _scene(7, n_tracks=1)
    twins = [("a", templs[0][1]), ("b", templs[0][1].copy())]
    ctx = _SetsOracleCtx()
    monkeypatch.setattr(_lib, "default_context", lambda: ctx)
    got = MTM.trackTemplates(twins, frames, [(tracks[0][0], list(order))], 2, method)
    assert all(row[0][0][0] == twins[order[0]][0] for row in got)
    exp, _ = sets_loop_restated(twins, frames, [(tracks[0][0], list(order))], 2, method)
    _same_result(got, exp, len(frames), 1)


# ---- the new errors: in the Python layer, after the loop's own ----------------------------------------------------------
def test_new_errors_are_raised_before_any_native_call(no_native):
    templs, frames, tracks, _ = _scene(1)
    other = templs + [("tall", np.zeros((6, 6), np.uint8))]
    b = tracks[0][0]
    m = MTM.TemplateMatcher(other, 5, context=_NoNativeCtx())
    cases = [([(b, [])], {}, "empty set"), ([tracks[0], (b, ())], {}, r"tracks\[1\]: an empty set"),
             ([(b, np.zeros(0, np.int64))], {}, "empty set"),
             ([(b, [0, 13])], {}, r"tracks\[0\]: the templates of a set must be of one \(h, w\)"),
             ([(b, np.zeros((2, 2), np.int64))], {}, "1-D"),
             (tracks, {"update": 0.5}, "set of templates"), (tracks, {"return_templates": True}, "set of templates"),
             ([tracks[0], (b, 1)], {"update": 0.5, "refine": True}, "set of templates")]
    for tr, kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            MTM.trackTemplates(other, frames, tr, 2, 5, **kw)
        with pytest.raises(ValueError, match=msg):
            m.track(frames, tr, 2, **kw)
    with pytest.raises(ValueError, match="set of templates"):          # (also with no frame to plan)
        MTM.trackTemplates(other, [], tracks, 2, 5, return_templates=True)
    # members that are not integers, or out of range: what the loop's findMatchesInBoxes call raises
    for js in ([0, 1.5], ["0"], np.array([0.0, 1.0]), [0, 99]):
        with pytest.raises(Exception) as want:
            MTM.findMatchesInBoxes(other, frames[0], [(b, list(js))], 5, N_object=1)
        assert not isinstance(want.value, _NativeCalled)
        with pytest.raises(type(want.value)) as got:
            MTM.trackTemplates(other, frames, [(b, js)], 2, 5)
        assert str(got.value) == str(want.value)


def test_the_loops_own_frame0_errors_come_first(no_native):
    templs, frames, tracks, _ = _scene(1)
    other = templs + [("tall", np.zeros((6, 6), np.uint8)), ("huge", np.zeros((30, 6), np.uint8))]
    b = tracks[0][0]
    # a template larger than its box, a negative offset, a mask with method 3: _plan's errors, whatever else is wrong
    with pytest.raises(ValueError, match="larger than searchBox"):
        MTM.trackTemplates(other, frames, [(b, [0, 14]), (b, [])], 2, 5, update=0.5)
    with pytest.raises(ValueError, match="negative box offsets"):
        MTM.trackTemplates(other, frames, [((-1, 0, 12, 12), [0, 13])], 2, 5)
    with pytest.raises(ValueError, match="negative box offsets"):       # (also ahead of the 1-D rule)
        MTM.trackTemplates(other, frames, [((-1, 0, 12, 12), np.zeros((2, 2), np.int64))], 2, 5)
    with pytest.raises(IndexError):
        MTM.trackTemplates(other, frames, [(b, np.full((2, 2), 99))], 2, 5)
    masked = [(t[0], t[1], np.ones_like(t[1])) for t in templs]
    with pytest.raises(ValueError, match="masks are not supported"):
        MTM.trackTemplates(masked, frames, [(b, [])] + tracks, 2, 3)
    with pytest.raises(ValueError, match="margin"):
        MTM.trackTemplates(templs, frames, [(b, [])], -1, 5)
    # the mask warnings of frame 0 are emitted before the new error
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with pytest.raises(ValueError, match="empty set"):
            MTM.trackTemplates(masked, frames, [(b, [0, 1]), (b, [])], 2, 5)
    assert len(w) == 2


# ---- integer tracks go where they went ---------------------------------------------------------------------------------
class _OldCtx:
    """Implements only what trackTemplates used before sets: records what reaches it, returns fixed records."""
    def __init__(self):
        self.lock = threading.RLock()
        self.calls = []

    def set_templates(self, templates, method):
        self.calls.append(("set_templates", len(templates), method))

    def _records(self, frames, units):
        out = np.zeros(len(frames) * len(units), dtype=_lib.HIT_DTYPE)
        for f in range(len(frames)):
            rec = out[f * len(units):(f + 1) * len(units)]
            rec["templ_idx"], rec["x"], rec["y"] = units["templ_idx"], units["x0"] + f, units["y0"]
            rec["w"], rec["h"], rec["score"] = 6, 5, 0.25
        return out

    def _nbhd(self, rec):
        nb = np.zeros((len(rec), 3, 3), np.float32)
        nb[:, 1, 1] = 0.25
        return nb

    def track_boxes(self, *a, **k):
        self.calls.append(("track", a[2:], k))
        return self._records(a[0], a[1])

    def track_boxes_nbhd(self, *a, **k):
        self.calls.append(("track_nbhd", a[2:], k))
        rec = self._records(a[0], a[1])
        return rec, self._nbhd(rec)

    def track_boxes_adapt(self, *a, **k):
        self.calls.append(("track_adapt", a[2:5] + a[6:], k))
        rec = self._records(a[0], a[1])
        return rec, (self._nbhd(rec) if a[6] else None), [np.array(a[5][j]) for j in a[1]["templ_idx"].tolist()], None

    def track_boxes_reacquire(self, *a, **k):
        self.calls.append(("track_reacquire", a[2:5] + a[6:], k))
        rec = self._records(a[0], a[1])
        return rec, (self._nbhd(rec) if a[6] else None), None, None


@pytest.mark.parametrize("kw,kind,args", [({}, "track", (3, 0.5)), ({"refine": True}, "track_nbhd", (3, 0.5)),
                                          ({"update": 0.5}, "track_adapt", (3, 0.5, 128, False)),
                                          ({"reacquire": True, "refine": True}, "track_reacquire", (3, 0.5, 0, True))],
                         ids=["plain", "refine", "update", "reacquire"])
def test_integer_tracks_use_the_old_methods_with_the_old_arguments(monkeypatch, kw, kind, args):
    templs, frames, tracks, _ = _scene(2)
    ints = [(b, js[0]) for b, js in tracks] + [(tracks[0][0], np.int64(5))]
    ctx = _OldCtx()
    monkeypatch.setattr(_lib, "default_context", lambda: ctx)
    MTM.trackTemplates(templs, frames, ints, 3, 5, 0.5, **kw)
    MTM.TemplateMatcher(templs, 5, context=ctx).track(frames, ints, 3, 0.5, **kw)
    assert [c[0] for c in ctx.calls] == ["set_templates", kind] * 2
    assert all(c[1:] == (args, {}) for c in ctx.calls if c[0] == kind)
    # the old context has no method for the new call: a set must not be served by the old ones
    with pytest.raises(AttributeError, match="track_boxes_sets"):
        MTM.trackTemplates(templs, frames, ints[:1] + [(ints[1][0], [4])], 3, 5, 0.5, **{k: v for k, v in kw.items()
                                                                                       if k != "update"})


# ---- mask warnings, the matcher ----------------------------------------------------------------------------------------
def test_mask_warnings_one_per_track_variant_with_a_mask_slot_and_frame(monkeypatch):
    templs, frames, tracks, _ = _scene(5)
    masked = [(t[0], t[1], None) if i in (0, 2, 5) else t for i, t in enumerate(templs)]
    tracks = [tracks[0], (tracks[1][0], [4, 5, 5]), (tracks[2][0], 8)]          # 2 + 2 + 0 units with a mask slot
    ctx = _SetsOracleCtx()
    monkeypatch.setattr(_lib, "default_context", lambda: ctx)
    for reacquire in (False, True):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            MTM.trackTemplates(masked, frames, tracks, 2, 5, 0.95, reacquire=reacquire)
        assert len(w) == 4 * len(frames)            # the second search adds none


def test_matcher_track_with_sets_keeps_or_clears_its_residency_record(monkeypatch):
    templs, frames, tracks, _ = _scene(31)
    ctx = _SetsOracleCtx()
    monkeypatch.setattr(_lib, "default_context", lambda: ctx)
    exp = MTM.trackTemplates(templs, frames, tracks, 2, 5, 0.95, reacquire=True)
    assert ctx.calls[-1][3].tolist() == list(range(12))
    m = MTM.TemplateMatcher(templs, 5, context=ctx)
    assert m._uploaded_for is None
    got = m.track(frames, tracks, 2, 0.95, reacquire=True)
    assert repr(got) == repr(exp)
    assert len(ctx.templates) == len(templs)                    # every template resident, in list order
    assert ctx.calls[-1][3].tolist() == list(range(12))
    assert m._uploaded_for == ("uint8", 1)                      # as track leaves it for integer tracks
    n = len(ctx.calls)
    with pytest.raises(ValueError, match="empty set"):          # an error before the native call: the record is cleared
        m.track(frames, [(tracks[0][0], [])], 2, 0.95)
    assert m._uploaded_for is None and len(ctx.calls) == n
    m.track(frames, tracks, 2)
    assert m._uploaded_for == ("uint8", 1)
    assert m.track([], tracks, 2) == [] and m._uploaded_for == ("uint8", 1)     # nothing to do: the record stays


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_point():
    import build as mtm_build
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "include", "mtm_hip.h")) as fh:
        header = fh.read()
    assert "int mtm_track_boxes_sets(mtm_ctx* ctx," in header
    assert "#define MTM_ABI_VERSION 9" in header
    assert "mtm_track_boxes_sets" in _lib.SYMBOLS and len(_lib.SYMBOLS["mtm_track_boxes_sets"][1]) == 18
    assert callable(_lib.Context.track_boxes_sets)
    mtm_build.build()
    lib = _lib.load()
    assert lib.mtm_track_boxes_sets is not None
    # refused before any device work: no context
    assert lib.mtm_track_boxes_sets(None, None, 0, 0, 0, 1, 0, 0, None, 0, None, None, 0, 1, 0.0, 0, None, None) < 0
