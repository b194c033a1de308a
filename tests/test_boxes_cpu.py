"""MTM.findMatchesInBoxes / matchTemplatesInBoxes without a GPU: every scope error and every error of the loop it replaces
is raised before anything reaches the library (the loop's type, message and warnings), the parsing and clipping of both
box forms, the per-region suppression, and a numpy restatement of the region semantics on the oracle checked against a
loop of the oracle's findMatches on the crops."""
import threading
import warnings

import numpy as np
import pytest

import MTM
import mtm_oracle as O
from MTM import _lib, boxes

INF = float("inf")


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
    """Records what would reach the library; returns no hits."""
    def __init__(self):
        self.lock = threading.RLock()
        self.calls = []

    def set_templates(self, templates, method):
        self.calls.append(("set_templates", [t[0].shape for t in templates], method))

    def find_matches_boxes(self, image, units, mode, thr):
        self.calls.append(("boxes", units.copy(), mode, thr))
        return np.zeros(0, dtype=_lib.HIT_DTYPE), np.zeros(len(units), np.int64)


@pytest.fixture
def fake_ctx(monkeypatch):
    ctx = _FakeCtx()
    monkeypatch.setattr(_lib, "default_context", lambda: ctx)
    return ctx


def _img(h=64, w=80, chans=1, dtype=np.uint8, seed=0):
    rng = np.random.RandomState(seed)
    shape = (h, w) if chans == 1 else (h, w, chans)
    return rng.randint(0, 256, size=shape).astype(dtype)


def _templs(img, n=2):
    return [("t%d" % i, np.ascontiguousarray(img[3 * i:3 * i + 6, 2 * i:2 * i + 5])) for i in range(n)]


# ---- scope ---------------------------------------------------------------------------------------------------------
SCOPE = [
    # (description, image, templates-from-image, regions, method, fragment)
    ("float32 image", _img(dtype=np.float32), None, [(0, 0, 30, 30)], 5, "uint8 images"),
    ("2-channel image", _img(chans=2), None, [(0, 0, 30, 30)], 5, "uint8 images"),
    ("3-channel uint16", _img(chans=3, dtype=np.uint16), None, [(0, 0, 30, 30)], 5, "uint8 images"),
    ("mixed dtypes", _img(), [("a", _img(8, 8, dtype=np.uint16))], [(0, 0, 30, 30)], 5, "dtype"),
    ("channel mismatch", _img(chans=3), [("a", _img(8, 8))], [(0, 0, 30, 30)], 5, "channels"),
    ("method 6", _img(), None, [(0, 0, 30, 30)], 6, "methods"),
    ("mask with method 3", _img(), [("a", _img(8, 8), np.ones((8, 8), np.uint8))], [(0, 0, 30, 30)], 3, "masks"),
    ("mask with method 0", _img(), [("a", _img(8, 8), np.ones((8, 8), np.uint8))], [(0, 0, 30, 30)], 0, "masks"),
    ("negative x", _img(), None, [(0, 0, 30, 30), (-1, 0, 30, 30)], 5, "negative"),
    ("negative y", _img(), None, [((2, -5, 30, 30), [0])], 5, "negative"),
    ("uint16 template over 2^21 pixels", _img(1460, 1460, dtype=np.uint16),
     [("big", np.zeros((1449, 1449), np.uint16))], [(0, 0, 1460, 1460)], 5, "2\\^21"),
]


@pytest.mark.parametrize("desc,image,templs,regions,method,frag", SCOPE, ids=[s[0] for s in SCOPE])
@pytest.mark.parametrize("fn", ["find", "match"])
def test_scope_errors_before_native(no_native, desc, image, templs, regions, method, frag, fn):
    templs = templs if templs is not None else _templs(image)
    call = MTM.findMatchesInBoxes if fn == "find" else MTM.matchTemplatesInBoxes
    with pytest.raises(ValueError, match=frag):
        call(templs, image, regions, method)


# ---- the loop's own errors, in the loop's order ---------------------------------------------------------------------
def _loop_outcome(fn, templs, image, regions, method, n_obj, overlap):
    """What the loop does before its first native call: (exception type, message, warnings emitted before it)."""
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        for i, el in enumerate(regions):
            box, idx = (el[0], el[1]) if len(el) == 2 else (el, None)
            try:
                sub = templs if idx is None else [templs[j] for j in idx]
                if fn == "find":
                    MTM.findMatches(sub, image, method, n_obj, 0.5, searchBox=box)
                else:
                    MTM.matchTemplates(sub, image, method, n_obj, 0.5, overlap, searchBox=box)
            except _NativeCalled:
                if fn == "match" and method == 0:       # (the loop raises this once the first search ran)
                    return ValueError, "The method TM_SQDIFF is not supported. Use TM_SQDIFF_NORMED instead.", len(w)
                continue
            except Exception as e:  # noqa: BLE001
                return type(e), str(e), len(w)
    return None, None, len(w)


def _boxes_outcome(fn, templs, image, regions, method, n_obj, overlap):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        try:
            if fn == "find":
                MTM.findMatchesInBoxes(templs, image, regions, method, n_obj, 0.5)
            else:
                MTM.matchTemplatesInBoxes(templs, image, regions, method, n_obj, 0.5, overlap)
        except _NativeCalled:
            return None, None, len(w)
        except Exception as e:  # noqa: BLE001
            return type(e), str(e), len(w)
    return None, None, len(w)


_IMG = _img(40, 50)
_T = [("a", _IMG[0:8, 0:8].copy(), None), ("b", _IMG[5:20, 3:9].copy()), ("c", _IMG[1:4, 1:30].copy(), None)]
LOOP_ERRORS = [
    # (description, templates, image, regions, method, N_object, maxOverlap)
    ("larger than the 3rd box", _T, _IMG, [(0, 0, 40, 40), ((0, 0, 30, 30), [0]), (0, 0, 10, 40)], 5, INF, 0.25),
    ("larger at index 1 of a subset", _T, _IMG, [((0, 0, 12, 12), [0, 1])], 5, INF, 0.25),
    ("crop of height 0", _T, _IMG, [((0, 0, 30, 30), [0]), ((0, 40, 30, 30), [0])], 5, INF, 0.25),
    ("crop of width 0", _T, _IMG, [((50, 0, 30, 30), [0])], 1, 3, 0.25),
    ("N_object float", _T, _IMG, [(0, 0, 40, 40)], 5, 2.5, 0.25),
    ("maxOverlap", _T, _IMG, [(0, 0, 40, 40)], 5, INF, 1.5),
    ("bad index in region 2", _T, _IMG, [((0, 0, 30, 30), [0]), ((0, 0, 30, 30), [1, 3])], 5, INF, 0.25),
    ("template height 0", [("z", np.zeros((0, 4), np.uint8))] + _T, _IMG, [((0, 0, 30, 30), [1]), (0, 0, 40, 40)], 5,
     INF, 0.25),
    ("tuple form", _T + [["x", _IMG[:3, :3]]], _IMG, [((0, 0, 30, 30), [0]), ((0, 0, 30, 30), [3])], 5, INF, 0.25),
    ("image height 0", _T, _IMG[:0], [(0, 0, 10, 10)], 5, INF, 0.25),
    ("TM_SQDIFF", _T[:1], _IMG, [(0, 0, 30, 30), (0, 0, 4, 4)], 0, INF, 0.25),
    ("TM_SQDIFF after region 0's error", _T[:1], _IMG, [(0, 0, 4, 4), (0, 0, 30, 30)], 0, INF, 0.25),
    ("mask warnings of the completed regions", _T, _IMG, [(0, 0, 40, 40), (0, 0, 40, 40), (0, 0, 20, 5)], 5, INF,
     0.25),
    ("no error, mask warnings", _T, _IMG, [(0, 0, 40, 40), ((0, 0, 40, 40), [2, 0, 2]), ((0, 0, 40, 40), [])], 2, 1,
     0.25),
    ("empty searchBoxes", _T, _IMG, [], 5, 2.5, 7.0),
]


@pytest.mark.parametrize("desc,templs,image,regions,method,n_obj,overlap", LOOP_ERRORS, ids=[c[0] for c in LOOP_ERRORS])
@pytest.mark.parametrize("fn", ["find", "match"])
def test_loop_errors_and_warnings_in_loop_order(no_native, desc, templs, image, regions, method, n_obj, overlap, fn):
    exp = _loop_outcome(fn, templs, image, regions, method, n_obj, overlap)
    got = _boxes_outcome(fn, templs, image, regions, method, n_obj, overlap)
    assert got == exp


# ---- parsing, clipping, what reaches the library ---------------------------------------------------------------------
def test_both_box_forms_and_clipping(fake_ctx):
    img = _img(40, 50)
    templs = _templs(img, 3)
    regions = [(0, 0, 20, 20), ((45, 30, 20, 20), [2]), ((10, 33, 100, 100), [1, 1]), ((5, 5, 10, 10), []),
               np.array([30, 0, 20, 40])]
    res = MTM.findMatchesInBoxes(templs, img, regions, 5)
    assert res == [[], [], [], [], []]
    (_, shapes, method), (_, units, mode, thr) = fake_ctx.calls
    assert shapes == [(6, 5), (6, 5), (6, 5)] and method == 5 and mode == _lib.PEAKS_LOCAL and thr == 0.5
    # every template of a plain box, the listed ones of a pair (duplicates kept), crops clipped at the image's edges
    assert [tuple(int(v) for v in u) for u in units] == [
        (0, 0, 0, 20, 20), (1, 0, 0, 20, 20), (2, 0, 0, 20, 20),
        (2, 30, 45, 10, 5),
        (1, 33, 10, 7, 40), (1, 33, 10, 7, 40),
        (0, 0, 30, 40, 20), (1, 0, 30, 40, 20), (2, 0, 30, 40, 20)]


def test_match_boxes_records_resident_templates_only_when_set(fake_ctx):
    """TemplateMatcher.match_boxes claims the list resident (what match() then relies on) only after a call that set the
    templates: not for an empty searchBoxes, nor when every box lists no template."""
    img = _img(40, 50)
    m = MTM.TemplateMatcher(_templs(img, 2), 5, context=fake_ctx)
    assert m.match_boxes(img, []) == [] and m._uploaded_for is None
    assert m.match_boxes(img, [((0, 0, 30, 30), []), ((5, 5, 30, 30), [])]) == [[], []] and m._uploaded_for is None
    assert fake_ctx.calls == []
    m.match_boxes(img, [(0, 0, 30, 30)])
    assert m._uploaded_for == ("uint8", 1) and [c[0] for c in fake_ctx.calls] == ["set_templates", "boxes"]
    m._uploaded_for = ("float32", 1)                 # (as after match() on a float32 image)
    assert m.match_boxes(img, [((0, 0, 30, 30), [])]) == [[]] and m._uploaded_for == ("float32", 1)
    with pytest.raises(ValueError):                   # raised before the native call: match() will upload again
        m.match_boxes(img, [(0, 0, 2, 2)])
    assert m._uploaded_for is None


def test_only_used_templates_are_set(fake_ctx):
    img = _img(40, 50)
    templs = _templs(img, 3) + [("huge", _img(90, 90))]         # never searched: the loop never looks at it
    MTM.matchTemplatesInBoxes(templs, img, [((0, 0, 30, 30), [2]), ((1, 1, 30, 30), [0])], 1, 1)
    (_, shapes, _), (_, units, mode, _) = fake_ctx.calls
    assert len(shapes) == 2 and list(units["templ_idx"]) == [1, 0] and mode == _lib.PEAKS_GLOBAL


def test_slice_len_is_numpy_slicing():
    rng = np.random.RandomState(1)
    for _ in range(500):
        size, start, length = int(rng.randint(0, 30)), int(rng.randint(0, 40)), int(rng.randint(-45, 45))
        got = int(boxes._slice_len(np.array([start]), np.array([length]), size)[0])
        assert got == len(range(size)[start:start + length])


def test_mask_warning_count(fake_ctx):
    img = _img(40, 50)
    templs = [("a", img[:5, :5].copy(), None), ("b", img[:6, :6].copy()), ("c", img[:4, :4].copy(), np.ones((4, 4)))]
    regions = [(0, 0, 30, 30), ((0, 0, 30, 30), [2, 2, 1]), ((0, 0, 30, 30), [])]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        MTM.findMatchesInBoxes(templs, img, regions, 5)
    assert len(w) == 2 + 2 and all(str(x.message) == MTM._MSG_MASK_UNSUPPORTED for x in w)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        MTM.findMatchesInBoxes(templs[:2], img, regions[:1], 3)      # methods 0 / 3 use the (absent) masks: no warning
    assert len(w) == 0


# ---- the suppression per region ---------------------------------------------------------------------------------------
def _random_raw(rng, counts, ascending):
    raw = np.zeros(int(sum(counts)), dtype=_lib.HIT_DTYPE)
    raw["x"] = rng.randint(0, 60, len(raw))
    raw["y"] = rng.randint(0, 60, len(raw))
    raw["w"] = raw["h"] = 12
    raw["templ_idx"] = rng.randint(0, 2, len(raw))
    raw["score"] = np.round(rng.rand(len(raw)), 2).astype(np.float32)       # ties included
    off = 0
    for n in counts:        # each region's list in findMatches' order: template, quality, row-major
        seg = raw[off:off + n]
        q = seg["score"] if not ascending else -seg["score"]
        raw[off:off + n] = seg[np.lexsort((seg["x"], seg["y"], -q, seg["templ_idx"]))]
        off += n
    return raw


@pytest.mark.parametrize("n_obj", [INF, 1, 3, 0, -2])
@pytest.mark.parametrize("method", [1, 5])
@pytest.mark.parametrize("fused", [False, True])
def test_nms_per_region_equals_nms_of_each_region(n_obj, method, fused):
    rng = np.random.RandomState(int(method + (n_obj if n_obj != INF else 9) * 3 + 5))
    counts = np.array([0, 1, 2, 7, 30, 1, 0, 12])
    raw = _random_raw(rng, counts, method == 1)
    kept, kc = boxes._nms_regions(raw, counts, 0.3, method, n_obj, 0.25, fused_cut=fused)
    off = 0
    exp = []
    for n in counts:
        seg = raw[off:off + n]
        off += n
        k = MTM._nms_raw(seg, 0.3, method == 1, n_obj, 0.25)
        if fused and n_obj not in (INF, 1) and n_obj >= 0:       # mtm_find_matches_image_nms cuts a list of one hit too
            k = k[:n_obj]
        exp.append(k)
    assert list(kc) == [len(e) for e in exp]
    assert kept.tobytes() == (np.concatenate(exp) if exp else kept[:0]).tobytes()


# ---- the region semantics restated on the oracle -------------------------------------------------------------------
def find_matches_in_boxes_restated(listTemplates, image, regions, method, N_object, thr, border):
    """findMatchesInBoxes restated: a unit's map is the full image's map of its template, cut to the outputs whose windows
    lie inside the region (a window sum over the crop is a window sum over the image); its own edges are the map border
    for the 3x3 peak test (padded by the border rule), the "no non-maximum pixel, no peaks" rule and the 1-D / 1x1 rules
    apply per unit; N_object == 1 takes the unit's extremum, first in row-major order."""
    H, W = image.shape[:2]
    full = {}
    out = []
    for el in regions:
        box, idx = (el[0], el[1]) if len(el) == 2 else (el, range(len(listTemplates)))
        x, y, w, h = box
        rows, cols = len(range(H)[y:y + h]), len(range(W)[x:x + w])
        hits = []
        for j in idx:
            label, templ = listTemplates[j][:2]
            th, tw = templ.shape[:2]
            if j not in full:
                full[j] = O.compute_score_map(templ, image, method)
            m = full[j][y:y + rows - th + 1, x:x + cols - tw + 1]
            q = -m.astype(np.float64) if method in (0, 1) else m.astype(np.float64)
            thr_q = -thr if method in (0, 1) else thr
            if N_object == 1:
                k = int(np.argmax(q.ravel()))
                peaks = [(k // m.shape[1], k % m.shape[1])]
            elif m.shape == (1, 1):
                peaks = [(0, 0)] if q[0, 0] >= thr_q else []
            elif m.shape[0] == 1 or m.shape[1] == 1:
                line = q.ravel()
                pk = O.find_peaks_1d(line, thr_q)
                peaks = [(0, p) if m.shape[0] == 1 else (p, 0) for p in pk]
            else:
                pad = np.pad(q, 1, mode="edge") if border == "nearest" else np.pad(q, 1, constant_values=0.0)
                mx = q.copy()
                for dy in range(3):
                    for dx in range(3):
                        mx = np.maximum(mx, pad[dy:dy + q.shape[0], dx:dx + q.shape[1]])
                is_max = q == mx
                if is_max.all():
                    is_max[:] = False
                is_max &= q > thr_q
                ys, xs = np.nonzero(is_max)
                order = np.argsort(-q[ys, xs], kind="stable")
                peaks = [(int(ys[i]), int(xs[i])) for i in order]
            hits += [(label, (int(px) + x, int(py) + y, tw, th), m[py, px]) for py, px in peaks]
        out.append(hits)
    return out


def _key(hits):
    return [(h[0], tuple(int(v) for v in h[1]), np.float32(h[2]).tobytes()) for h in hits]


@pytest.mark.parametrize("border", ["constant", "nearest"])
@pytest.mark.parametrize("chans", [1, 3])
def test_restatement_equals_oracle_loop(border, chans):
    rng = np.random.RandomState(40 + chans)
    for case in range(12):
        img = _img(36, 44, chans, seed=case)
        img[4:20, 6:26] = 90                                       # a flat patch
        templs = [("a", img[2:8, 3:10].copy()), ("b", img[10:11, 0:12].copy()), ("flat", img[6:10, 8:14].copy())]
        regions = [(6, 4, 20, 16), (0, 0, 44, 36), (30, 20, 30, 30), ((3, 2, 7, 20), [0]), ((3, 2, 30, 6), [0]),
                   ((3, 2, 7, 6), [0]), ((0, 10, 44, 1), [1]), ((5, 10, 12, 1), [1]),
                   (int(rng.randint(0, 20)), int(rng.randint(0, 20)), int(rng.randint(14, 40)), int(rng.randint(14, 40)))]
        for method in range(6):
            thr = {0: 1e7, 1: 0.5, 2: 0.0, 3: 0.9, 4: 0.0, 5: 0.3}[method]
            for n_obj in (INF, 1):
                exp = []
                for el in regions:
                    box, idx = (el[0], el[1]) if len(el) == 2 else (el, range(3))
                    exp.append(O.find_matches([templs[j] for j in idx], img, method, n_obj, thr, searchBox=box,
                                              border=border))
                got = find_matches_in_boxes_restated(templs, img, regions, method, n_obj, thr, border)
                assert [_key(g) for g in got] == [_key(e) for e in exp]
                if n_obj == INF and border == "nearest":
                    assert got[0] == []              # the flat region's maps hold no non-maximum pixel: no peaks
