"""Lost tracks re-acquired by a whole-frame search in MTM.trackTemplates / TemplateMatcher.track (reacquire=True) without
a GPU: the argument errors before any native call, reacquire=False through the methods the call used before, the Python
layer's result from a fake context that runs the defining loop on the CPU oracle, tracking.lost, and the C header."""
import os
import threading
import warnings

import numpy as np
import pytest

import MTM
import mtm_oracle as O
from MTM import _lib, subpixel, tracking
from MTM.tracking import blend_template, next_box


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


def _scene(seed, n_frames=5, hw=(32, 40), templ_hw=(5, 6), n_tracks=3, margin=2, chans=1, dtype=np.uint8, jumps=((1, 2),)):
    """Dim noise frames with each track's template pasted at a position that drifts by at most one pixel per frame;
    `jumps`: (track, frame) pairs - before that frame the track's object moves half the map away, out of its box."""
    rng = np.random.RandomState(seed)
    shape = hw if chans == 1 else hw + (chans,)
    th, tw = templ_hw
    top = 256 if dtype == np.uint8 else 65536
    templs = [("o%d" % k, rng.randint(0, top, size=templ_hw if chans == 1 else templ_hw + (chans,)).astype(dtype))
              for k in range(n_tracks)]
    pos = [[int(rng.randint(0, hw[1] - tw + 1)), int(rng.randint(0, hw[0] - th + 1))] for _ in range(n_tracks)]
    starts = [((max(0, x - margin), max(0, y - margin), tw + 2 * margin, th + 2 * margin), k) for k, (x, y) in enumerate(pos)]
    frames, truth = [], []
    for f in range(n_frames):
        for k, jf in jumps:
            if jf == f:
                pos[k][0] = (pos[k][0] + (hw[1] - tw + 1) // 2) % (hw[1] - tw + 1)
                pos[k][1] = (pos[k][1] + (hw[0] - th + 1) // 2) % (hw[0] - th + 1)
        fr = (rng.randint(0, top, size=shape) // 8).astype(dtype)
        for k in range(n_tracks):
            x, y = pos[k]
            fr[y:y + th, x:x + tw] = templs[k][1]
        frames.append(fr)
        truth.append([tuple(p) for p in pos])
        for p in pos:
            p[0] = int(np.clip(p[0] + rng.randint(-1, 2), 0, hw[1] - tw))
            p[1] = int(np.clip(p[1] + rng.randint(-1, 2), 0, hw[0] - th))
    return templs, frames, starts, truth


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


# ---- argument errors before any native call --------------------------------------------------------------------------
@pytest.mark.parametrize("reacquire", [1, 0, "yes", None], ids=repr)
def test_reacquire_must_be_a_bool_before_any_native_call(no_native, reacquire):
    templs, frames, tracks, _ = _scene(1)
    with pytest.raises(ValueError, match="reacquire"):
        MTM.trackTemplates(templs, frames, tracks, 3, 5, 0.9, reacquire=reacquire)
    m = MTM.TemplateMatcher(templs, 5, context=_NoNativeCtx())
    with pytest.raises(ValueError, match="reacquire"):
        m.track(frames, tracks, 3, 0.9, reacquire=reacquire)
    with pytest.raises(ValueError, match="reacquire"):        # (also with nothing to track)
        MTM.trackTemplates(templs, frames, [], 3, 5, 0.9, reacquire=reacquire)


def test_reacquire_needs_min_score_before_any_native_call(no_native):
    templs, frames, tracks, _ = _scene(1)
    with pytest.raises(ValueError, match="min_score"):
        MTM.trackTemplates(templs, frames, tracks, 3, 5, reacquire=True)
    with pytest.raises(ValueError, match="min_score"):
        MTM.trackTemplates(templs, frames, tracks, 3, 5, None, reacquire=True, refine=True, update=0.5)
    m = MTM.TemplateMatcher(templs, 5, context=_NoNativeCtx())
    with pytest.raises(ValueError, match="min_score"):
        m.track(frames, tracks, 3, reacquire=True)
    with pytest.raises(ValueError, match="min_score"):
        m.track(frames, tracks, 3, None, reacquire=True)
    with pytest.raises(ValueError, match="margin"):           # the older checks still come
        MTM.trackTemplates(templs, frames, tracks, -1, 5, 0.9, reacquire=True)


def test_reacquire_is_keyword_only():
    templs, frames, tracks, _ = _scene(1)
    with pytest.raises(TypeError):
        MTM.trackTemplates(templs, frames, tracks, 3, 5, 0.9, False, None, False, True)


# ---- reacquire=False goes through the methods it went through before --------------------------------------------------
class _OldCtx:
    """Implements only what trackTemplates used before `reacquire`: records what reaches it, returns fixed records."""
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
        assert len(a) == 4 and not k
        return self._records(a[0], a[1])

    def track_boxes_nbhd(self, *a, **k):
        self.calls.append(("track_nbhd", a[2:], k))
        assert len(a) == 4 and not k
        rec = self._records(a[0], a[1])
        return rec, self._nbhd(rec)

    def track_boxes_adapt(self, *a, **k):
        self.calls.append(("track_adapt", a[2:5] + a[6:], k))
        assert len(a) == 7 and not k
        rec = self._records(a[0], a[1])
        return rec, (self._nbhd(rec) if a[6] else None), [np.array(a[5][j]) for j in a[1]["templ_idx"].tolist()], None


@pytest.mark.parametrize("refine,update,kind,args", [(False, None, "track", (3, 0.5)), (True, None, "track_nbhd", (3, 0.5)),
                                                     (False, 0.5, "track_adapt", (3, 0.5, 128, False)),
                                                     (True, 0.5, "track_adapt", (3, 0.5, 128, True))])
def test_reacquire_false_uses_the_old_methods_with_the_old_arguments(monkeypatch, refine, update, kind, args):
    templs, frames, tracks, _ = _scene(2)
    ctx = _OldCtx()
    monkeypatch.setattr(_lib, "default_context", lambda: ctx)
    old = MTM.trackTemplates(templs, frames, tracks, 3, 5, 0.5, refine=refine, update=update)
    new = MTM.trackTemplates(templs, frames, tracks, 3, 5, 0.5, refine=refine, update=update, reacquire=False)
    m = MTM.TemplateMatcher(templs, 5, context=ctx)
    third = m.track(frames, tracks, 3, 0.5, refine=refine, update=update, reacquire=False)
    assert repr(old) == repr(new) == repr(third)
    assert [c[0] for c in ctx.calls] == ["set_templates", kind] * 3
    assert all(c[1:] == (args, {}) for c in ctx.calls if c[0] == kind)
    # the old context has no method for the new call: reacquire=True must not be served by the old ones
    with pytest.raises(AttributeError, match="track_boxes_reacquire"):
        MTM.trackTemplates(templs, frames, tracks, 3, 5, 0.5, refine=refine, update=update, reacquire=True)


# ---- the Python layer on a context that runs the defining loop on the oracle ------------------------------------------
def _passes(score, method, min_score):
    s, m = float(score), float(min_score)
    return s < m if method in (0, 1) else s > m


def reacquire_loop_restated(templs, frames, tracks, margin, method, min_score, rate=None):
    """The loop of MTM/tracking.py's docstring on the oracle, with `update`'s adoption where rate is given: (hits [f][k],
    every track's last template, the (frame, track) pairs searched twice)."""
    cur = [templs[j][1] for _, j in tracks]
    box = [tuple(b) for b, _ in tracks]
    out, again = [], []
    for fi, f in enumerate(frames):
        H, W = f.shape[:2]
        row = []
        for k, (_, j) in enumerate(tracks):
            hit, = O.find_matches([(templs[j][0], cur[k])], f, method, 1, searchBox=box[k])
            if not _passes(hit[2], method, min_score):
                hit, = O.find_matches([(templs[j][0], cur[k])], f, method, 1, searchBox=(0, 0, W, H))
                again.append((fi, k))
            row.append([hit])
            if rate is not None and _passes(hit[2], method, min_score):
                x, y, w, h = hit[1]
                cur[k] = blend_template(cur[k], f[y:y + h, x:x + w], rate)
            box[k] = next_box(box[k], hit, margin, f.shape, method, min_score)
        out.append(row)
    return out, cur, again


class _ReacqOracleCtx:
    """track_boxes_reacquire as the loop on the oracle, in the binding's terms (units, weight in 256ths, records)."""
    def __init__(self):
        self.lock = threading.RLock()
        self.calls = []

    def set_templates(self, templates, method):
        self.templates, self.method = [t[0] for t in templates], method

    def track_boxes_reacquire(self, frames, units, margin, min_score, blend_a, templates, with_nbhd=False):
        self.calls.append((len(frames), units.copy(), margin, min_score, blend_a, with_nbhd))
        assert all(a is b for a, b in zip(templates, self.templates))
        templs = [("t", t) for t in self.templates]
        tracks = [((int(u["x0"]), int(u["y0"]), int(u["cols"]), int(u["rows"])), int(u["templ_idx"])) for u in units]
        res, cur, _ = reacquire_loop_restated(templs, frames, tracks, margin, self.method, min_score,
                                              blend_a / 256 if blend_a else None)
        out = np.zeros(len(frames) * len(units), dtype=_lib.HIT_DTYPE)
        for f, row in enumerate(res):
            for k, ((_, (x, y, w, h), s),) in enumerate(row):
                out[f * len(units) + k] = (tracks[k][1], x, y, w, h, s)
        self.nbhd = None
        if with_nbhd:           # (a made-up neighbourhood with a fractional peak: the fit is subpixel's business)
            self.nbhd = np.zeros((len(out), 3, 3), np.float32)
            self.nbhd[:, 1, 1] = out["score"]
            self.nbhd[:, 1, 2] = out["score"] * np.float32(0.75)
            self.nbhd[:, 1, 0] = out["score"] * np.float32(0.5)
        return out, self.nbhd, (cur if blend_a else None), (np.zeros((len(units), 7)) if blend_a else None)


def _same(got, exp):
    g, e = got[0], exp[0]
    assert g[0] == e[0]
    assert tuple(g[1]) == tuple(e[1]) and all(type(v) is int for v in g[1])
    assert isinstance(g[2], np.float32) and g[2].tobytes() == np.float32(e[2]).tobytes()


@pytest.mark.parametrize("chans,dtype", [(1, np.uint8), (3, np.uint8), (1, np.uint16)])
@pytest.mark.parametrize("method", [1, 2, 5])
@pytest.mark.parametrize("update", [None, 0.5])
def test_reacquiring_result_is_the_loops(monkeypatch, method, chans, dtype, update):
    templs, frames, tracks, truth = _scene(20 + method, chans=chans, dtype=dtype)
    tracks = tracks + [(tracks[0][0], 0)]               # two tracks of one list template, and an unused list entry
    templs = templs[:2] + [("unused", templs[0][1][:3, :3].copy())] + templs[2:]
    tracks = [(b, j if j < 2 else j + 1) for b, j in tracks]
    thr = _thr(method, [templs[j] for _, j in tracks])
    ctx = _ReacqOracleCtx()
    monkeypatch.setattr(_lib, "default_context", lambda: ctx)
    exp, exp_last, again = reacquire_loop_restated(templs, frames, tracks, 2, method, thr, update)
    assert (2, 1) in again                              # the jump is searched twice ...
    assert exp[2][1][0][1][:2] == truth[2][1]           # ... and found
    got, last = MTM.trackTemplates(templs, np.stack(frames), tracks, 2, method, thr, update=update, reacquire=True,
                                   return_templates=True)
    (n, units, margin, min_score, a, with_nbhd), = ctx.calls
    assert (n, margin, min_score, a, with_nbhd) == (len(frames), 2, thr, 128 if update else 0, False)
    assert units["templ_idx"].tolist() == [0, 1, 2, 0]         # only the used templates are set, in list order
    assert len(got) == len(frames) and all(len(r) == len(tracks) and all(len(c) == 1 for c in r) for r in got)
    for f in range(len(frames)):
        for k, (_, j) in enumerate(tracks):
            _same(got[f][k], exp[f][k])
            assert got[f][k][0][0] == templs[j][0]             # the list's label, mapped back from the used subset
    assert len(last) == len(tracks)
    for t, e, (_, j) in zip(last, exp_last, tracks):
        assert t.shape == templs[j][1].shape and t.dtype == templs[j][1].dtype and np.array_equal(t, e)
        assert t is not templs[j][1]
    # refined: the fit of the final records' neighbourhoods
    ref = MTM.trackTemplates(templs, frames, tracks, 2, method, thr, update=update, reacquire=True, refine=True)
    assert ctx.calls[-1][5] is True
    flat = [got[f][k][0] for f in range(len(frames)) for k in range(len(tracks))]
    want = subpixel._refined(flat, ctx.nbhd, method)
    assert [r[0] for row in ref for r in row] == want
    assert all(type(r[0][1][0]) is float for row in ref for r in row)


def test_matcher_track_reacquires_and_keeps_the_residency_record(monkeypatch):
    templs, frames, tracks, _ = _scene(31)
    templs = templs + [("unused", templs[0][1][:3, :3].copy())]
    ctx = _ReacqOracleCtx()
    monkeypatch.setattr(_lib, "default_context", lambda: ctx)
    exp = MTM.trackTemplates(templs, frames, tracks, 2, 5, 0.95, reacquire=True)
    m = MTM.TemplateMatcher(templs, 5, context=ctx)
    assert m._uploaded_for is None
    got = m.track(frames, tracks, 2, 0.95, reacquire=True)
    assert repr(got) == repr(exp)
    assert len(ctx.templates) == len(templs)                    # every template resident, in list order
    assert ctx.calls[-1][1]["templ_idx"].tolist() == [0, 1, 2]
    assert m._uploaded_for == ("uint8", 1)                      # as track leaves it today
    r2, l2 = m.track(frames, tracks, 2, 0.95, reacquire=True, return_templates=True)
    assert repr(r2) == repr(exp) and all(np.array_equal(a, templs[j][1]) for a, (_, j) in zip(l2, tracks))
    # nothing to do: no native call, the record stays
    assert m.track([], tracks, 2, 0.95, reacquire=True) == [] and m._uploaded_for == ("uint8", 1)
    assert MTM.trackTemplates(templs, frames, [], 2, 5, 0.95, reacquire=True) == [[] for _ in frames]


def test_mask_warnings_are_those_of_the_call_without_reacquire(monkeypatch):
    templs, frames, tracks, _ = _scene(5)
    masked = [(t[0], t[1], np.ones_like(t[1])) for t in templs[:2]] + templs[2:]
    ctx = _ReacqOracleCtx()
    monkeypatch.setattr(_lib, "default_context", lambda: ctx)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        MTM.trackTemplates(masked, frames, tracks, 2, 5, 0.95, reacquire=True)
    assert len(w) == 2 * len(frames)            # one per masked track and frame: the second search adds none
    with pytest.raises(ValueError):             # masks with method 3: out of scope, as without reacquire
        MTM.trackTemplates(masked, frames, tracks, 2, 3, 0.95, reacquire=True)
    assert len(ctx.calls) == 1


# ---- tracking.lost ---------------------------------------------------------------------------------------------------
def test_lost_marks_the_hits_that_do_not_pass():
    f32 = np.float32
    res = [[[("a", (1, 2, 5, 6), f32(0.5))], [("b", (3, 4, 5, 6), f32(0.96))]],
           [[("a", (7, 8, 5, 6), f32(np.nan))], [("b", (9, 10, 5, 6), f32(0.95))]]]
    refined = [[[(h[0], (h[1][0] + 0.25, h[1][1] - 0.5) + h[1][2:], h[2])] for (h,) in row] for row in res]
    for r in (res, refined):
        for method in (2, 3, 4, 5):             # maxima: pass above min_score; equal does not pass; NaN never passes
            got = tracking.lost(r, method, 0.95)
            assert got.dtype == bool and got.shape == (2, 2)
            assert got.tolist() == [[True, float(f32(0.96)) <= 0.95], [True, True]]
        for method in (0, 1):                   # minima: pass below min_score
            assert tracking.lost(r, method, 0.6).tolist() == [[False, True], [True, True]]
            assert tracking.lost(r, method, 0.5).tolist() == [[True, True], [True, True]]
    assert tracking.lost([], 5, 0.5).shape == (0, 0)
    assert tracking.lost([[], []], 5, 0.5).shape == (2, 0)
    assert "lost" in tracking.__all__


@pytest.mark.parametrize("bad", [[[[]]], [[[("a", (0, 0, 1, 1), 0.5)] * 2]],
                                 [[[("a", (0, 0, 1, 1), 0.5)]], []]], ids=["no hit", "two hits", "ragged"])
def test_lost_needs_one_hit_per_frame_and_track(bad):
    with pytest.raises(ValueError, match="lost"):
        tracking.lost(bad, 5, 0.5)


@pytest.mark.parametrize("min_score", [None, True, "x"], ids=repr)
def test_lost_needs_a_number(min_score):
    with pytest.raises(ValueError, match="min_score"):
        tracking.lost([], 5, min_score)


def test_lost_of_a_tracked_result(monkeypatch):
    templs, frames, tracks, _ = _scene(12, n_frames=6, jumps=())
    for f in (2, 3):                    # nothing anywhere in two frames: both searches fail
        frames[f] = (np.random.RandomState(f).randint(0, 256, size=frames[f].shape) // 8).astype(np.uint8)
    ctx = _ReacqOracleCtx()
    monkeypatch.setattr(_lib, "default_context", lambda: ctx)
    for refine in (False, True):
        res = MTM.trackTemplates(templs, frames, tracks, 2, 5, 0.95, reacquire=True, refine=refine)
        want = np.zeros((6, 3), bool)
        want[2:4] = True
        assert np.array_equal(tracking.lost(res, 5, 0.95), want)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_point():
    import build as mtm_build
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "include", "mtm_hip.h")) as fh:
        header = fh.read()
    assert "int mtm_track_boxes_reacquire(mtm_ctx* ctx," in header
    assert "#define MTM_ABI_VERSION 9" in header
    assert "mtm_track_boxes_reacquire" in _lib.SYMBOLS
    assert _lib.SYMBOLS["mtm_track_boxes_reacquire"] == _lib.SYMBOLS["mtm_track_boxes_adapt"]
    assert callable(_lib.Context.track_boxes_reacquire)
    mtm_build.build()
    lib = _lib.load()
    assert lib.mtm_track_boxes_reacquire is not None
    # refused before any device work: no context
    assert lib.mtm_track_boxes_reacquire(None, None, 0, 0, 0, 1, 0, 0, None, 0, 0, 1, 0.0, None, None, 0, None, None) < 0
    assert lib.mtm_track_boxes_reacquire(None, None, 0, 0, 0, 1, 0, 0, None, 0, 0, 1, 0.0, None, None, 300, None, None) < 0
