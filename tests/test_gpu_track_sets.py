"""Tracks that carry a set of templates in MTM.trackTemplates / TemplateMatcher.track on the GPU: every case
equals the loop that defines it (MTM/tracking.py) written with MTM.findMatchesInBoxes and next_box - every variant of the
set searched in the track's box, the first extreme hit the frame's record - in labels, boxes, float32 score bits,
exceptions and warning counts.  The scenes show a different variant of each object in every frame, and the tests assert
that the reference's labels change, so that no comparison passes with one variant winning throughout."""
import warnings

import numpy as np
import pytest

import MTM
from MTM import _lib
from MTM.tracking import next_box

pytestmark = pytest.mark.gpu

KINDS = ["u8", "rgb", "u16"]
NV = 4                  # templates per work-group (kTrackNV, csrc/mtm_track.hip)
GRID = 2048             # work-groups of one track_reacquire_sets_kernel launch (kTrackReacquireGrid)
SIZES = (1, 2, NV, NV + 1, 2 * NV + 1)


def _key(hits):
    return [(h[0], tuple(int(v) for v in h[1]), np.float32(h[2]).tobytes()) for h in hits]


def _key3(res):
    return [[_key(r) for r in fr] for fr in res]


def _top(kind):
    return 65536 if kind == "u16" else 256


def _pixels(rng, shape, kind, hi=None):
    if kind == "u16":
        return rng.randint(0, hi or 65536, size=shape).astype(np.uint16)
    shape = tuple(shape) if kind == "u8" else tuple(shape) + (3,)
    return rng.randint(0, hi or 256, size=shape).astype(np.uint8)


def _pool(rng, hw, kind, n):
    """n appearances of one shape: a template, its flips and its 180 degree rotation, then unrelated ones."""
    t = _pixels(rng, hw, kind)
    pool = [t, t[:, ::-1].copy(), t[::-1].copy(), t[::-1, ::-1].copy()]
    return (pool + [_pixels(rng, hw, kind) for _ in range(max(0, n - 4))])[:n]


def _scene(seed, kind, set_sizes, n_frames=6, hw=(60, 76), thw=(7, 9), pad=3, step=1, jumps=None, blank=(), absent=None,
           at=None):
    """Dim noise frames (below a quarter of the range); track k's object is variant (f + k) % len(set k) of its set,
    pasted at a position that moves up to `step` pixels per frame.  jumps[(f, k)] = (dx, dy): after frame f track k's
    object also moves by that much, modulo its map's size.  `blank`: frames that show no object; absent[k] = f: track k's
    object is gone from frame f on.  `at`: the objects' (x, y) in frame 0 (default: random, so objects may cover each
    other).  Returns (templates, frames, tracks with sets, (x, y, label) per frame and track)."""
    rng = np.random.RandomState(seed)
    th, tw = thw
    templs, sets = [], []
    for k, n in enumerate(set_sizes):
        sets.append(list(range(len(templs), len(templs) + n)))
        templs += [("o%d.%d" % (k, v), a) for v, a in enumerate(_pool(rng, thw, kind, n))]
    pos = [[int(rng.randint(0, hw[1] - tw + 1)), int(rng.randint(0, hw[0] - th + 1))] for _ in set_sizes]
    if at is not None:
        pos = [list(p) for p in at]
    tracks = [((max(0, x - pad), max(0, y - pad), tw + 2 * pad, th + 2 * pad), js) for (x, y), js in zip(pos, sets)]
    frames, truth = [], []
    for f in range(n_frames):
        fr = _pixels(rng, hw, kind, hi=_top(kind) // 4)
        row = []
        for k, js in enumerate(sets):
            x, y = pos[k]
            j = js[(f + k) % len(js)]
            if f not in blank and not (absent and k in absent and f >= absent[k]):
                fr[y:y + th, x:x + tw] = templs[j][1]
            row.append((x, y, templs[j][0]))
        frames.append(fr)
        truth.append(row)
        for k, p in enumerate(pos):
            p[0] = int(np.clip(p[0] + rng.randint(-step, step + 1), 0, hw[1] - tw))
            p[1] = int(np.clip(p[1] + rng.randint(-step, step + 1), 0, hw[0] - th))
            if jumps and (f, k) in jumps:
                p[0] = (p[0] + jumps[(f, k)][0]) % (hw[1] - tw + 1)
                p[1] = (p[1] + jumps[(f, k)][1]) % (hw[0] - th + 1)
    return templs, frames, tracks, truth


def _thr(method, templs):
    """Thresholds far from both an exact copy's score and a noise window's."""
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


def _passes(score, method, min_score):
    s, m = float(score), float(min_score)
    return s < m if method in (0, 1) else s > m


def _set(js):
    return [js] if isinstance(js, (int, np.integer)) else list(js)


def _loop(templs, frames, tracks, margin, method, min_score=None, reacquire=False, refine=False):
    """The defining loop on the public functions.  Returns (result [f][k], [(f, k, recovered)] per second search).  The
    second search is silent: the call emits the mask warnings of the call without reacquire."""
    pick = min if method in (0, 1) else max
    box = [b for b, _ in tracks]
    out, again = [], []
    for fi, f in enumerate(frames):
        H, W = f.shape[:2]
        row = []
        for k, (_, js) in enumerate(tracks):
            hits = MTM.findMatchesInBoxes(templs, f, [(box[k], _set(js))], method, N_object=1)[0]
            hit = pick(hits, key=lambda h: h[2])
            if reacquire and not _passes(hit[2], method, min_score):
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    hits = MTM.findMatchesInBoxes(templs, f, [((0, 0, W, H), _set(js))], method, N_object=1)[0]
                hit = pick(hits, key=lambda h: h[2])
                again.append((fi, k, _passes(hit[2], method, min_score)))
            row.append(MTM.refineHits(templs, f, [hit], method) if refine else [hit])
            box[k] = next_box(box[k], hit, margin, f.shape, method, min_score)
        out.append(row)
    return out, again


def _outcome(call):
    """(result, (exception type, message) or None, number of warnings)"""
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        try:
            r, e = call(), None
        except Exception as ex:  # noqa: BLE001 - compared with the loop's
            r, e = None, (type(ex), str(ex))
    return r, e, len(w)


def _compare(templs, frames, tracks, margin, method, min_score=None, reacquire=False, matcher=None):
    """trackTemplates against the loop: result, exception, warning count.  Returns (the loop's result, second searches)."""
    exp = _outcome(lambda: _loop(templs, list(frames), tracks, margin, method, min_score, reacquire))
    if matcher is None:
        got = _outcome(lambda: MTM.trackTemplates(templs, frames, tracks, margin, method, min_score, reacquire=reacquire))
    else:
        got = _outcome(lambda: matcher.track(frames, tracks, margin, min_score, reacquire=reacquire))
    assert got[1] == exp[1]
    assert got[2] == exp[2]
    if exp[1] is not None:
        return None, None
    assert _key3(got[0]) == _key3(exp[0][0])
    return exp[0]


def _labels(res, k):
    return [row[k][0][0] for row in res]


# ---- every set size, kind and method ------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("kind", KINDS)
def test_sets_of_every_group_filling_equal_the_loop(kind, method):
    templs, frames, tracks, truth = _scene(100 + method, kind, SIZES)
    tracks = tracks[:4] + [(tracks[4][0], np.array(tracks[4][1]))]              # (a 1-D array is a set too)
    thr = _thr(method, templs)
    exp, _ = _compare(templs, frames, tracks, 3, method, thr)
    for k, n in enumerate(SIZES):           # the winner is the appearance shown: the label changes across the frames
        assert _labels(exp, k) == [row[k][2] for row in truth]
        assert len(set(_labels(exp, k))) == min(n, len(frames))
    exp2, _ = _compare(templs, frames, tracks, 3, method)                       # (no min_score)
    assert _key3(exp2) == _key3(exp)


@pytest.mark.parametrize("method", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("kind", KINDS)
def test_a_template_over_one_chunk_in_both_directions(kind, method):
    templs, frames, tracks, truth = _scene(200 + method, kind, (NV + 1,), n_frames=5, hw=(40, 100), thw=(17, 65), pad=2)
    exp, _ = _compare(templs, frames, tracks, 2, method, _thr(method, templs))
    assert _labels(exp, 0) == [row[0][2] for row in truth] and len(set(_labels(exp, 0))) == 5


# ---- box geometry --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("margin", [0, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_boxes_at_every_frame_edge_and_a_map_of_one_output(kind, margin):
    rng = np.random.RandomState(5)
    hw, (th, tw) = (60, 76), (7, 9)
    pools = [_pool(rng, (th, tw), kind, n) for n in (NV + 1, 2, NV, 3, 2 * NV + 1)]
    templs = [("o%d.%d" % (k, v), a) for k, p in enumerate(pools) for v, a in enumerate(p)]
    first = np.cumsum([0] + [len(p) for p in pools])
    sets = [list(range(first[k], first[k + 1])) for k in range(5)]
    # objects in the four corners and one in the middle; the corner boxes reach past the frame and are clipped by the
    # call, the middle one is exactly the template's size (one output)
    at = [(0, 0), (hw[1] - tw, 0), (0, hw[0] - th), (hw[1] - tw, hw[0] - th), (30, 25)]
    boxes = [(0, 0, tw + 3, th + 3), (hw[1] - tw - 3, 0, tw + 30, th + 3), (0, hw[0] - th - 3, tw + 3, th + 30),
             (hw[1] - tw - 3, hw[0] - th - 3, tw + 30, th + 30), (30, 25, tw, th)]
    frames = []
    for f in range(5):
        fr = _pixels(rng, hw, kind, hi=_top(kind) // 4)
        for k, (x, y) in enumerate(at):
            fr[y:y + th, x:x + tw] = templs[sets[k][(f + k) % len(sets[k])]][1]
        frames.append(fr)
    tracks = list(zip(boxes, sets))
    for method in (1, 4, 5):
        exp, _ = _compare(templs, frames, tracks, margin, method)
        for k in range(5):
            assert [tuple(row[k][0][1][:2]) for row in exp] == [at[k]] * 5
            assert len(set(_labels(exp, k))) == min(len(sets[k]), 5)


# ---- ties ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("kind", KINDS)
def test_flat_frames_flat_templates_and_ties(kind, method):
    rng = np.random.RandomState(9)
    hw, thw = (40, 50), (7, 9)
    t = _pixels(rng, thw, kind)
    flat = np.full_like(t, 77)
    # identical pixels under different labels, in both orders, around a flat template and a different one
    templs = [("a", t), ("b", t.copy()), ("flat", flat), ("c", t[::-1].copy()), ("b2", t.copy()), ("flat2", flat.copy())]
    frames = [np.full_like(_pixels(rng, hw, kind), 77) for _ in range(2)]
    for _ in range(3):
        fr = _pixels(rng, hw, kind, hi=_top(kind) // 4)
        fr[10:17, 12:21] = t
        fr[10:17, 24:33] = t            # the same pixels twice in one box: equal scores at two positions of one variant
        frames.append(fr)
    frames.append(np.zeros_like(frames[0]))
    box = (8, 6, 30, 16)
    tracks = [(box, [0, 1, 4]), (box, [4, 1, 0]), (box, [2, 5]), (box, [5, 2, 3, 0, 1]), (box, [3, 2, 1, 0, 4, 5, 3, 2, 1]),
              ((0, 0, 50, 40), [1, 0])]
    exp, _ = _compare(templs, frames, tracks, 40, method)
    assert [_labels(exp, k)[2] for k in (0, 1, 5)] == ["a", "b2", "b"]           # the first in set order
    assert tuple(exp[2][0][0][1][:2]) == (12, 10)                               # the first in row-major order
    _compare(templs, frames, tracks, 2, method, _thr(method, templs[:1]), reacquire=True)


# ---- reacquire -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("kind", KINDS)
def test_reacquire_jump_never_found_and_lost_in_frame_0(kind, method):
    templs, frames, tracks, truth = _scene(300 + method, kind, (NV + 1, 2, 2 * NV + 1, 3), n_frames=7,
                                           jumps={(1, 0): (30, 22), (3, 2): (31, 20)}, absent={1: 3},
                                           at=[(8, 6), (60, 6), (8, 40), (58, 44)])     # (far apart, jumps included)
    tracks[3] = ((20, 20, 15, 13), tracks[3][1])                # track 3 starts away from its object
    thr = _thr(method, templs)
    exp, again = _compare(templs, frames, tracks, 3, method, thr, reacquire=True)
    assert len(again) >= 4
    if method in (2, 4):        # (without a normalisation a window over another object can pass: no facts to assert)
        return
    assert (2, 0, True) in again and (4, 2, True) in again and (0, 3, True) in again
    assert [a for a in again if a[1] == 1] == [(f, 1, False) for f in range(3, 7)]     # never found again
    for k in (0, 2, 3):
        assert _labels(exp, k) == [row[k][2] for row in truth]
    assert np.array_equal(MTM.tracking.lost(exp, method, thr)[:, 1], np.arange(7) >= 3)


@pytest.mark.parametrize("kind", KINDS)
def test_all_tracks_lost_at_once_with_more_items_than_the_grid(kind):
    n = 40
    templs, frames, tracks, truth = _scene(17, kind, (2 * NV + 1,) * n, n_frames=3, blank=(1,))
    items = n * 3 * (-(-(60 - 7 + 1) // 16) * -(-(76 - 9 + 1) // 16))
    assert items > GRID
    exp, again = _compare(templs, frames, tracks, 3, 5, 0.95, reacquire=True)
    assert sorted(a for a in again if a[0] == 1) == [(1, k, False) for k in range(n)]
    # a copy that a later track's copy covers is not the shown one: the label is asserted where the window is intact,
    # which the last track's always is
    shown = [k for k in range(n) if np.array_equal(
        frames[2][truth[2][k][1]:truth[2][k][1] + 7, truth[2][k][0]:truth[2][k][0] + 9], dict(templs)[truth[2][k][2]])]
    assert n - 1 in shown
    assert all(exp[2][k][0][0] == truth[2][k][2] for k in shown)


# ---- compositions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reacquire", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_refine_is_refinehits_of_the_unrefined_result(kind, reacquire):
    templs, frames, tracks, _ = _scene(23, kind, (NV + 1, 1, 2), jumps={(1, 0): (30, 22)})
    tracks[1] = (tracks[1][0], tracks[1][1][0])                 # (an integer track among the sets)
    for method in (1, 5):
        thr = _thr(method, templs)
        plain = MTM.trackTemplates(templs, frames, tracks, 3, method, thr, reacquire=reacquire)
        got = MTM.trackTemplates(templs, frames, tracks, 3, method, thr, reacquire=reacquire, refine=True)
        want = [[MTM.refineHits(templs, f, hits, method) for hits in row] for f, row in zip(frames, plain)]
        assert got == want
        assert all(type(h[0][1][0]) is float for row in got for h in row)
        assert got == _loop(templs, frames, tracks, 3, method, thr, reacquire, refine=True)[0]
        assert MTM.tracking.positions(got).shape == (len(frames), 3, 2)


@pytest.mark.parametrize("kind", KINDS)
def test_one_frame_per_chunk_gives_the_unforced_result(kind):
    templs, frames, tracks, _ = _scene(13, kind, (NV + 1, 2, NV), n_frames=7, jumps={(1, 1): (35, 25)}, blank=(5,))
    ctx = _lib.default_context()
    old = ctx.get_option(_lib.OPT_BATCH_MAX_ROWS)
    ref = MTM.trackTemplates(templs, frames, tracks, 4, 5, 0.95, reacquire=True)
    ctx.set_option(_lib.OPT_BATCH_MAX_ROWS, frames[0].shape[0])
    try:
        exp, again = _compare(templs, frames, tracks, 4, 5, 0.95, reacquire=True)
    finally:
        ctx.set_option(_lib.OPT_BATCH_MAX_ROWS, old)
    assert _key3(ref) == _key3(exp)
    assert (2, 1, True) in again and (5, 0, False) in again


def test_the_same_call_twice_gives_identical_keys():
    n = 12
    jumps = {(f, k): (20 + k, 15 + k) for f in (0, 2) for k in range(n)}
    templs, frames, tracks, _ = _scene(29, "u8", (NV + 1, 2, 2 * NV + 1) * 4, jumps=jumps)
    a = MTM.trackTemplates(templs, frames, tracks, 3, 5, 0.95, reacquire=True)
    b = MTM.trackTemplates(templs, frames, tracks, 3, 5, 0.95, reacquire=True)
    assert _key3(a) == _key3(b)


def test_matcher_track_equals_the_function_and_match_works_afterwards():
    templs, frames, tracks, _ = _scene(31, "u8", (NV + 1, 2, 1), jumps={(1, 0): (30, 22)})
    m = MTM.TemplateMatcher(templs, 5, N_object=1)
    exp, again = _compare(templs, frames, tracks, 4, 5, 0.95, reacquire=True, matcher=m)
    assert (2, 0, True) in again
    got = m.track(np.stack(frames), tracks, 4, 0.95, reacquire=True, refine=True)
    assert got == MTM.trackTemplates(templs, frames, tracks, 4, 5, 0.95, reacquire=True, refine=True)
    for f in frames[:2]:                            # match() on the same matcher afterwards
        assert _key(m.match(f)) == _key(MTM.matchTemplates(templs, f, 5, 1))


def test_frame_0_errors_and_warnings_are_the_loops():
    templs, frames, tracks, _ = _scene(37, "u8", (2, 3, 1))
    masked = [(t[0], t[1], None) if i in (0, 3) else t for i, t in enumerate(templs)]
    exp, _ = _compare(masked, frames, tracks, 3, 5, 0.95, reacquire=True)        # warnings: one per unit with a slot and frame
    assert exp is not None
    big = templs + [("big", np.zeros((30, 9), np.uint8))]
    assert _compare(big, frames, [tracks[0], (tracks[1][0], [2, 6])], 3, 5) == (None, None)
    assert _compare(templs, frames, [tracks[0], (tracks[1][0], [2, 60])], 3, 5) == (None, None)
    # an empty set: the loop's max() of no hit and the call's own check are both ValueError (the messages differ)
    with pytest.raises(ValueError):
        _loop(templs, frames, [tracks[0], (tracks[1][0], [])], 3, 5)
    with pytest.raises(ValueError, match="empty set"):
        MTM.trackTemplates(templs, frames, [tracks[0], (tracks[1][0], [])], 3, 5)


# ---- a seeded sweep ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(60))
def test_random_small_cases_equal_the_loop(seed):
    rng = np.random.RandomState(1000 + seed)
    kind = KINDS[rng.randint(3)]
    method = int(rng.randint(6))
    n_tracks = int(rng.randint(1, 4))
    set_sizes = [int(rng.choice([1, 2, 3, NV, NV + 1, 2 * NV, 2 * NV + 1])) for _ in range(n_tracks)]
    thw = (int(rng.randint(1, 20)), int(rng.randint(1, 70)))
    hw = (thw[0] + int(rng.randint(4, 30)), thw[1] + int(rng.randint(4, 40)))
    margin = int(rng.choice([0, 1, 3, 100]))
    reacquire = bool(rng.randint(2))
    jumps = {(1, 0): (hw[1] // 2, hw[0] // 2)} if rng.randint(2) else None
    templs, frames, tracks, _ = _scene(seed, kind, set_sizes, n_frames=int(rng.randint(2, 5)), hw=hw, thw=thw,
                                       pad=int(rng.randint(0, 4)), step=int(rng.randint(0, 3)), jumps=jumps,
                                       blank=(2,) if rng.randint(3) == 0 else ())
    tracks = [(b, js[0]) if len(js) == 1 and rng.randint(2) else (b, js) for b, js in tracks]
    if n_tracks > 1 and rng.randint(2):             # a set that borrows another track's variants, with a duplicate
        tracks[0] = (tracks[0][0], _set(tracks[0][1]) + _set(tracks[1][1])[:2] + _set(tracks[0][1])[:1])
    min_score = _thr(method, templs) if reacquire or rng.randint(2) else None
    _compare(templs, frames, tracks, margin, method, min_score, reacquire=reacquire)
    if rng.randint(4) == 0:
        got = MTM.trackTemplates(templs, frames, tracks, margin, method, min_score, reacquire=reacquire, refine=True)
        assert got == _loop(templs, frames, tracks, margin, method, min_score, reacquire, refine=True)[0]
