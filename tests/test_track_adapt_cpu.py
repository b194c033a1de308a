"""Adaptive templates in MTM.trackTemplates / TemplateMatcher.track (update=..., return_templates=...) without a GPU:
blend_template's integer arithmetic, the argument errors before any native call, update=None through the methods the
call used before, the Python layer's result from a fake context that runs the defining loop on the CPU oracle, and the
host's template constants (mtm_debug_templ_stats) against a numpy restatement in the same operation order."""
import threading

import numpy as np
import pytest

import MTM
import mtm_oracle as O
from MTM import _lib, tracking
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


def _scene(seed, n_frames=4, hw=(32, 40), templ_hw=(5, 6), n_tracks=3, margin=3, chans=1, dtype=np.uint8):
    """Dim noise frames with each track's template pasted at a drifting position, brighter from frame to frame."""
    rng = np.random.RandomState(seed)
    shape = hw if chans == 1 else hw + (chans,)
    th, tw = templ_hw
    top = 256 if dtype == np.uint8 else 65536
    templs = [("o%d" % k, rng.randint(0, top // 2, size=templ_hw if chans == 1 else templ_hw + (chans,)).astype(dtype))
              for k in range(n_tracks)]
    pos = [[int(rng.randint(0, hw[1] - tw + 1)), int(rng.randint(0, hw[0] - th + 1))] for _ in range(n_tracks)]
    starts = [((max(0, x - margin), max(0, y - margin), tw + 2 * margin, th + 2 * margin), k) for k, (x, y) in enumerate(pos)]
    frames = []
    for f in range(n_frames):
        fr = (rng.randint(0, top, size=shape) // 8).astype(dtype)
        for k in range(n_tracks):
            x, y = pos[k]
            fr[y:y + th, x:x + tw] = templs[k][1] + (templs[k][1] // 8) * f
        frames.append(fr)
        for p in pos:
            p[0] = int(np.clip(p[0] + rng.randint(-1, 2), 0, hw[1] - tw))
            p[1] = int(np.clip(p[1] + rng.randint(-1, 2), 0, hw[0] - th))
    return templs, frames, starts


# ---- blend_template ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("a", [1, 77, 128, 255, 256])
def test_blend_template_is_the_rounded_blend_in_integers(dtype, a):
    rng = np.random.RandomState(a)
    top = int(np.iinfo(dtype).max)
    T = rng.randint(0, top + 1, size=(9, 11, 3)).astype(dtype)
    W = rng.randint(0, top + 1, size=(9, 11, 3)).astype(dtype)
    T[0, 0], W[0, 0] = (0, top, top), (top, 0, top)         # the extremes
    got = blend_template(T, W, a / 256)
    assert got.dtype == T.dtype and got.shape == T.shape
    # floor((T (256 - a) + W a) / 256 + 1 / 2) in Python integers
    exp = [(2 * (int(t) * (256 - a) + int(w) * a) + 256) // 512 for t, w in zip(T.ravel().tolist(), W.ravel().tolist())]
    assert got.ravel().tolist() == exp
    assert got is not T and got is not W


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_blend_template_rate_one_is_the_window(dtype):
    rng = np.random.RandomState(3)
    T = rng.randint(0, 200, size=(4, 7)).astype(dtype)
    W = rng.randint(0, 200, size=(4, 7)).astype(dtype)
    assert np.array_equal(blend_template(T, W, 1.0), W) and np.array_equal(blend_template(T, W, 1), W)
    assert np.array_equal(blend_template(T, T, 0.3), T)        # blending with itself changes nothing


@pytest.mark.parametrize("rate", [0, -0.1, 1.5, True, "x", 1e-4, None, float("nan")], ids=repr)
def test_blend_template_rate_errors(rate):
    T = np.zeros((3, 3), np.uint8)
    with pytest.raises(ValueError, match="rate"):
        blend_template(T, T, rate)


def test_blend_template_shape_and_dtype_errors():
    T = np.zeros((3, 4), np.uint8)
    with pytest.raises(ValueError, match="shape"):
        blend_template(T, np.zeros((4, 3), np.uint8), 0.5)
    with pytest.raises(ValueError, match="uint8"):
        blend_template(T, np.zeros((3, 4), np.uint16), 0.5)
    with pytest.raises(ValueError, match="uint8"):
        blend_template(T.astype(np.float32), T.astype(np.float32), 0.5)


def test_blend_template_is_public():
    assert "blend_template" in tracking.__all__


# ---- argument errors before any native call --------------------------------------------------------------------------
@pytest.mark.parametrize("update", [0, -0.1, 1.5, True, "x", 1e-4], ids=repr)
def test_update_errors_before_any_native_call(no_native, update):
    templs, frames, tracks = _scene(1)
    with pytest.raises(ValueError, match="update"):
        MTM.trackTemplates(templs, frames, tracks, 3, 5, update=update)
    m = MTM.TemplateMatcher(templs, 5, context=_NoNativeCtx())
    with pytest.raises(ValueError, match="update"):
        m.track(frames, tracks, 3, update=update)
    with pytest.raises(ValueError, match="update"):        # (also with nothing to track)
        MTM.trackTemplates(templs, frames, [], 3, 5, update=update)


@pytest.mark.parametrize("update", [None, 0.5])
def test_return_templates_must_be_a_bool(no_native, update):
    templs, frames, tracks = _scene(1)
    with pytest.raises(ValueError, match="return_templates"):
        MTM.trackTemplates(templs, frames, tracks, 3, 5, update=update, return_templates=1)
    m = MTM.TemplateMatcher(templs, 5, context=_NoNativeCtx())
    with pytest.raises(ValueError, match="return_templates"):
        m.track(frames, tracks, 3, update=update, return_templates=1)


def test_new_arguments_are_keyword_only():
    templs, frames, tracks = _scene(1)
    with pytest.raises(TypeError):
        MTM.trackTemplates(templs, frames, tracks, 3, 5, None, False, 0.5)


# ---- update=None goes through the methods it went through before ------------------------------------------------------
class _OldCtx:
    """Implements only what trackTemplates used before `update`: records what reaches it, returns a fixed record."""
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

    def track_boxes(self, *a, **k):
        self.calls.append(("track", a[2:], k))
        assert len(a) == 4 and not k
        return self._records(a[0], a[1])

    def track_boxes_nbhd(self, *a, **k):
        self.calls.append(("track_nbhd", a[2:], k))
        assert len(a) == 4 and not k
        rec = self._records(a[0], a[1])
        nb = np.zeros((len(rec), 3, 3), np.float32)
        nb[:, 1, 1] = 0.25
        return rec, nb


@pytest.mark.parametrize("refine", [False, True])
def test_update_none_uses_the_old_methods_and_gives_the_old_result(monkeypatch, refine):
    templs, frames, tracks = _scene(2)
    ctx = _OldCtx()
    monkeypatch.setattr(_lib, "default_context", lambda: ctx)
    old = MTM.trackTemplates(templs, frames, tracks, 3, 5, 0.5, refine=refine)
    new = MTM.trackTemplates(templs, frames, tracks, 3, 5, 0.5, refine=refine, update=None)
    res, last = MTM.trackTemplates(templs, frames, tracks, 3, 5, 0.5, refine=refine, update=None, return_templates=True)
    assert repr(old) == repr(new) == repr(res)
    assert isinstance(old, list) and len(old) == len(frames) and old[1][2][0][0] == "o2"
    kind = "track_nbhd" if refine else "track"
    assert [c[0] for c in ctx.calls] == ["set_templates", kind] * 3
    assert all(c[1:] == ((3, 0.5), {}) for c in ctx.calls if c[0] == kind)
    # without update, the returned templates are copies of the originals
    assert len(last) == len(tracks)
    for t, (_, j) in zip(last, tracks):
        assert np.array_equal(t, templs[j][1]) and t.dtype == templs[j][1].dtype and t is not templs[j][1]
    m = MTM.TemplateMatcher(templs, 5, context=ctx)
    assert repr(m.track(frames, tracks, 3, 0.5, refine=refine)) == repr(old)
    r2, l2 = m.track(frames, tracks, 3, 0.5, refine=refine, return_templates=True)
    assert repr(r2) == repr(old) and all(np.array_equal(a, b) for a, b in zip(l2, last))


def test_return_templates_with_nothing_to_do(no_native):
    templs, frames, tracks = _scene(2)
    for update in (None, 0.5):
        res, last = MTM.trackTemplates(templs, [], tracks, 3, 5, update=update, return_templates=True)
        assert res == [] and [t.tolist() for t in last] == [templs[j][1].tolist() for _, j in tracks]
        res, last = MTM.trackTemplates(templs, frames, [], 3, 5, update=update, return_templates=True)
        assert res == [[] for _ in frames] and last == []


# ---- the Python layer on a context that runs the defining loop on the oracle ------------------------------------------
def _passes(score, method, min_score):
    if min_score is None:
        return True
    s, m = float(score), float(min_score)
    return s < m if method in (0, 1) else s > m


def adaptive_loop_restated(templs, frames, tracks, margin, method, min_score, rate):
    """The loop of MTM/tracking.py's docstring on the oracle: (hits [f][k], every track's last template)."""
    cur = [templs[j][1] for _, j in tracks]
    box = [tuple(b) for b, _ in tracks]
    out = []
    for f in frames:
        row = []
        for k, (_, j) in enumerate(tracks):
            hit, = O.find_matches([(templs[j][0], cur[k])], f, method, 1, searchBox=box[k])
            row.append([hit])
            if _passes(hit[2], method, min_score):
                x, y, w, h = hit[1]
                cur[k] = blend_template(cur[k], f[y:y + h, x:x + w], rate)
            box[k] = next_box(box[k], hit, margin, f.shape, method, min_score)
        out.append(row)
    return out, cur


class _AdaptOracleCtx:
    """track_boxes_adapt as the loop on the oracle, in the binding's terms (units, weight in 256ths, records)."""
    def __init__(self):
        self.lock = threading.RLock()
        self.calls = []

    def set_templates(self, templates, method):
        self.templates, self.method = [t[0] for t in templates], method

    def track_boxes_adapt(self, frames, units, margin, min_score, blend_a, templates, with_nbhd=False):
        self.calls.append((len(frames), units.copy(), margin, min_score, blend_a, with_nbhd))
        assert all(a is b for a, b in zip(templates, self.templates))
        templs = [("t", t) for t in self.templates]
        tracks = [((int(u["x0"]), int(u["y0"]), int(u["cols"]), int(u["rows"])), int(u["templ_idx"])) for u in units]
        res, cur = adaptive_loop_restated(templs, frames, tracks, margin, self.method, min_score, blend_a / 256)
        out = np.zeros(len(frames) * len(units), dtype=_lib.HIT_DTYPE)
        for f, row in enumerate(res):
            for k, ((_, (x, y, w, h), s),) in enumerate(row):
                out[f * len(units) + k] = (tracks[k][1], x, y, w, h, s)
        nbhd = None
        if with_nbhd:
            nbhd = np.zeros((len(out), 3, 3), np.float32)
            nbhd[:, 1, 1] = out["score"]
        return out, nbhd, cur, np.zeros((len(units), 7))


@pytest.mark.parametrize("chans,dtype", [(1, np.uint8), (3, np.uint8), (1, np.uint16)])
@pytest.mark.parametrize("method", [1, 3, 5])
def test_adaptive_result_is_the_loops(monkeypatch, method, chans, dtype):
    templs, frames, tracks = _scene(20 + method, chans=chans, dtype=dtype)
    tracks = tracks + [(tracks[0][0], 0)]               # two tracks of one list template, and an unused list entry
    templs = templs + [("unused", templs[0][1][:3, :3].copy())]
    ctx = _AdaptOracleCtx()
    monkeypatch.setattr(_lib, "default_context", lambda: ctx)
    exp, exp_last = adaptive_loop_restated(templs, frames, tracks, 3, method, None, 0.5)
    got, last = MTM.trackTemplates(templs, np.stack(frames), tracks, 3, method, update=0.5, return_templates=True)
    (n, units, margin, min_score, a, with_nbhd), = ctx.calls
    assert (n, margin, min_score, a, with_nbhd) == (len(frames), 3, None, 128, False)
    assert units["templ_idx"].tolist() == [0, 1, 2, 0]         # only the used templates are set, in list order
    # labels, nesting, boxes, score bits
    assert len(got) == len(frames) and all(len(r) == len(tracks) and all(len(c) == 1 for c in r) for r in got)
    for f in range(len(frames)):
        for k, (_, j) in enumerate(tracks):
            g, e = got[f][k][0], exp[f][k][0]
            assert g[0] == e[0] == templs[j][0]
            assert tuple(g[1]) == tuple(e[1]) and all(type(v) is int for v in g[1])
            assert isinstance(g[2], np.float32) and g[2].tobytes() == np.float32(e[2]).tobytes()
    # the templates: one per track, shapes and dtypes of the list's, the loop's pixels; the objects changed, so they differ
    assert len(last) == len(tracks)
    for t, e, (_, j) in zip(last, exp_last, tracks):
        assert t.shape == templs[j][1].shape and t.dtype == templs[j][1].dtype and np.array_equal(t, e)
    assert any(not np.array_equal(t, templs[j][1]) for t, (_, j) in zip(last, tracks))
    # without return_templates: the result alone; on a matcher: the same, every template resident
    assert repr(MTM.trackTemplates(templs, frames, tracks, 3, method, update=0.5)) == repr(got)
    m = MTM.TemplateMatcher(templs, method, context=ctx)
    r2, l2 = m.track(frames, tracks, 3, update=0.5, return_templates=True)
    assert repr(r2) == repr(got) and all(np.array_equal(a, b) for a, b in zip(l2, last))
    assert ctx.calls[-1][1]["templ_idx"].tolist() == [0, 1, 2, 0] and len(ctx.templates) == len(templs)


def test_adaptive_refined_call_asks_for_neighbourhoods_and_quantises_the_rate(monkeypatch):
    templs, frames, tracks = _scene(5)
    ctx = _AdaptOracleCtx()
    monkeypatch.setattr(_lib, "default_context", lambda: ctx)
    res = MTM.trackTemplates(templs, frames, tracks, 3, 5, 0.2, refine=True, update=1 / 256)
    assert ctx.calls[0][3:] == (0.2, 1, True)
    assert all(type(r[0][1][0]) is float for row in res for r in row)
    MTM.trackTemplates(templs, frames, tracks, 3, 5, update=1)
    MTM.trackTemplates(templs, frames, tracks, 3, 5, update=0.3)
    assert [c[4] for c in ctx.calls[1:]] == [256, 77]


# ---- the host's template constants -----------------------------------------------------------------------------------
def _stats_np(t, method):
    """templ_stats_from_sums (csrc/mtm_templ_stats.h) restated: float64 operations in the same order, exact sums."""
    t = t.reshape(t.shape[0], t.shape[1], -1)
    rows, cols, chans = t.shape
    f = np.float64
    n = f(rows) * f(cols)
    inv_area = f(1.0) / (f(rows) * f(cols))
    mean, sdv = [f(0)] * 4, [f(0)] * 4
    for c in range(chans):
        v = [int(x) for x in t[:, :, c].ravel().tolist()]
        s, sq = f(sum(v)), f(sum(x * x for x in v))
        mean[c] = s / n
        var = sq / n - mean[c] * mean[c]
        sdv[c] = np.sqrt(max(var, f(0)))
    out = [f(0)] * 7
    if method == 2:
        return out
    num_type = 0 if method == 3 else 1 if method in (4, 5) else 2
    out[:4] = mean
    if method != 4:
        templ_norm = f(0)
        for c in range(chans):
            templ_norm = templ_norm + sdv[c] * sdv[c]
        if templ_norm < np.finfo(f).eps and method == 5:
            out[6] = f(1)
            return out
        msum = f(0)
        for c in range(chans):
            msum = msum + mean[c] * mean[c]
        templ_sum2 = templ_norm + msum
        if num_type != 1:
            out[:4] = [f(0)] * 4
            templ_norm = templ_sum2
        templ_sum2 = templ_sum2 / inv_area
        templ_norm = np.sqrt(templ_norm)
        templ_norm = templ_norm / np.sqrt(inv_area)
        out[4], out[5] = templ_norm, templ_sum2
    return out


def _stat_templates():
    rng = np.random.RandomState(0)
    out = []
    for hw in ((1, 1), (5, 7), (17, 65)):
        out.append(("u8 %dx%d" % hw, rng.randint(0, 256, size=hw).astype(np.uint8)))
        out.append(("rgb %dx%d" % hw, rng.randint(0, 256, size=hw + (3,)).astype(np.uint8)))
        out.append(("u16 %dx%d" % hw, rng.randint(0, 65536, size=hw).astype(np.uint16)))
    out.append(("u8 constant", np.full((5, 7), 93, np.uint8)))
    out.append(("rgb constant", np.full((5, 7, 3), 200, np.uint8)))
    out.append(("u16 constant", np.full((17, 65), 40000, np.uint16)))
    out.append(("u16 white", np.full((17, 65), 65535, np.uint16)))
    return out


@pytest.mark.parametrize("method", range(6))
def test_debug_templ_stats_equals_the_restatement(method):
    import build as mtm_build
    mtm_build.build()
    n_ones = 0
    for name, t in _stat_templates():
        got = _lib.debug_templ_stats(t, method)
        exp = _stats_np(t, method)
        assert got.dtype == np.float64 and got.shape == (7,)
        assert [float(v).hex() for v in got] == [float(v).hex() for v in exp], (name, method)
        if "constant" in name or "white" in name or t.shape[:2] == (1, 1):
            assert got[6] == (1.0 if method == 5 else 0.0), (name, method)
            n_ones += int(got[6])
    assert n_ones == (7 if method == 5 else 0)
    assert len(_lib.TEMPL_STATS_FIELDS) == 7


def test_debug_templ_stats_refuses_bad_arguments():
    import build as mtm_build
    mtm_build.build()
    lib = _lib.load()
    out = (np.zeros(7) - 7.0)
    px = np.zeros((4, 4), np.uint8)
    for args in ((None, 4, 4, 1, 0, 5), (px.ctypes.data, 0, 4, 1, 0, 5), (px.ctypes.data, 4, 4, 5, 0, 5),
                 (px.ctypes.data, 4, 4, 1, 7, 5), (px.ctypes.data, 4, 4, 1, 0, 6)):
        assert lib.mtm_debug_templ_stats(*args, out.ctypes.data_as(_lib._P(_lib.ctypes.c_double))) < 0
    assert (out == -7.0).all()
