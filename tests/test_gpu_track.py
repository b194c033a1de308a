"""MTM.trackTemplates / TemplateMatcher.track on the GPU: every case equals the loop of findMatchesInBoxes calls with
N_object=1 and next_box that a user writes today (hits, labels, boxes, float32 score bits, exceptions, warnings), for
every pixel type and method of the scope, across chunks of frames."""
import warnings

import numpy as np
import pytest

import MTM
from MTM import _lib
from MTM.tracking import next_box

pytestmark = pytest.mark.gpu


def _key(hits):
    return [(h[0], tuple(int(v) for v in h[1]), np.float32(h[2]).tobytes()) for h in hits]


def _key3(res):
    return [[_key(r) for r in fr] for fr in res]


def _loop(templs, frames, tracks, margin, method, min_score=None):
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
        except Exception as ex:  # noqa: BLE001 - compared with the loop's
            r, e = None, (type(ex), str(ex))
    return r, e, len(w)


def _compare(templs, frames, tracks, margin, method, min_score=None, matcher=None):
    exp = _outcome(lambda: _loop(templs, list(frames), tracks, margin, method, min_score))
    got = _outcome(lambda: MTM.trackTemplates(templs, frames, tracks, margin, method, min_score))
    assert got[1] == exp[1]
    assert got[2] == exp[2]
    if exp[1] is None:
        assert _key3(got[0]) == _key3(exp[0])
    if matcher is not None:
        got = _outcome(lambda: matcher.track(frames, tracks, margin, min_score))
        assert got[1] == exp[1]
        if exp[1] is None:
            assert _key3(got[0]) == _key3(exp[0])
    return exp[0]


def _pixels(rng, shape, kind, hi=None):
    if kind == "u16":
        return rng.randint(0, hi or 65536, size=shape).astype(np.uint16)
    shape = shape if kind == "u8" else shape + (3,)
    return rng.randint(0, hi or 256, size=shape).astype(np.uint8)


def _scene(seed, kind, n_frames=6, hw=(60, 76), templ_hw=(7, 9), n_tracks=4, step=3, corner=None, flat=False):
    """Dim noise frames with each track's template pasted at a position that moves up to `step` pixels per frame (or
    `step` pixels per frame towards `corner`, where it stays)."""
    rng = np.random.RandomState(seed)
    th, tw = templ_hw
    top = 65536 if kind == "u16" else 256
    templs = [("o%d" % k, _pixels(rng, templ_hw, kind)) for k in range(n_tracks)]
    if flat:
        templs[0] = ("flat", np.full_like(templs[0][1], top // 2))
    pos = [[int(rng.randint(0, hw[1] - tw + 1)), int(rng.randint(0, hw[0] - th + 1))] for _ in range(n_tracks)]
    frames, truth = [], []
    for _ in range(n_frames):
        fr = _pixels(rng, hw, kind, hi=top // 4)
        if flat:
            fr[: hw[0] // 2, : hw[1] // 2] = top // 3              # a constant patch: flat windows, tied scores
        for k in range(n_tracks):
            x, y = pos[k]
            fr[y:y + th, x:x + tw] = templs[k][1]
        frames.append(fr)
        truth.append([tuple(p) for p in pos])
        for p in pos:
            if corner is None:
                dx, dy = rng.randint(-step, step + 1), rng.randint(-step, step + 1)
            else:
                dx, dy = step * corner[0], step * corner[1]
            p[0] = int(np.clip(p[0] + dx, 0, hw[1] - tw))
            p[1] = int(np.clip(p[1] + dy, 0, hw[0] - th))
    return templs, frames, truth


def _starts(truth0, templ_hw, pad):
    th, tw = templ_hw
    return [((max(0, x - pad), max(0, y - pad), tw + 2 * pad, th + 2 * pad), k) for k, (x, y) in enumerate(truth0)]


KINDS = ["u8", "rgb", "u16"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", range(6))
@pytest.mark.parametrize("margin", [0, 1, 16])
def test_track_equals_loop(kind, method, margin):
    templs, frames, truth = _scene(100 * method + margin, kind, step=max(1, margin // 2))
    tracks = _starts(truth[0], (7, 9), 5)
    res = _compare(templs, frames, tracks, margin, method)
    if method in (1, 3, 5) and margin >= 2:        # the normalised methods follow the exact copy pasted last
        assert [fr[-1][0][1][:2] for fr in res] == [t[-1] for t in truth]


@pytest.mark.parametrize("kind", KINDS)
def test_matcher_track_equals_loop_and_match_after(kind):
    templs, frames, truth = _scene(7, kind, n_frames=5)
    m = MTM.TemplateMatcher(templs, 5, N_object=1)
    _compare(templs, frames, _starts(truth[0], (7, 9), 6), 8, 5, matcher=m)
    _compare(templs, np.stack(frames), _starts(truth[0], (7, 9), 3), 4, 5, min_score=0.9, matcher=m)
    for f in frames[:2]:                            # match() on the same matcher afterwards
        assert _key(m.match(f)) == _key(MTM.matchTemplates(templs, f, 5, 1))


@pytest.mark.parametrize("corner", [(-1, -1), (1, -1), (-1, 1), (1, 1)])
@pytest.mark.parametrize("kind", KINDS)
def test_tracks_driven_into_corners_and_clipped_at_edges(corner, kind):
    templs, frames, truth = _scene(31, kind, n_frames=10, step=4, corner=corner)
    tracks = _starts(truth[0], (7, 9), 6)
    # boxes that reach past every edge of the frame (clipped as numpy slicing clips them)
    tracks += [((0, 0, 200, 12), 0), ((60, 0, 40, 40), 1), ((0, 50, 30, 30), 2), ((64, 52, 30, 30), 3)]
    for method in (1, 2, 5):
        res = _compare(templs, frames, tracks, 6, method)
        if method in (1, 5):
            assert res[-1][3][0][1][:2] == truth[-1][3]


@pytest.mark.parametrize("kind", KINDS)
def test_constant_patches_and_ties(kind):
    templs, frames, truth = _scene(5, kind, n_frames=6, flat=True)
    top = 65536 if kind == "u16" else 256
    # a flat template and a track whose box lies in the constant patch: every window ties (first in row-major order)
    tracks = _starts(truth[0], (7, 9), 4) + [((2, 2, 26, 20), 0), ((3, 1, 30, 25), 1)]
    flat_frames = [f.copy() for f in frames]
    for f in flat_frames:
        f[...] = top // 5
    for method in range(6):
        _compare(templs, frames, tracks, 3, method)
        _compare(templs, flat_frames, tracks, 2, method, min_score=0.5)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", [1, 3, 5])
def test_min_score_loss_and_reacquisition(kind, method):
    templs, frames, truth = _scene(13, kind, n_frames=8, n_tracks=2, step=1)
    for f in (3, 4):                                # track 1's object is covered for two frames
        x, y = truth[f][1]
        frames[f][y:y + 7, x:x + 9] = 3
    thr = 0.05 if method == 1 else 0.95
    res = _compare(templs, frames, _starts(truth[0], (7, 9), 3), 6, method, min_score=thr)
    assert res[-1][1][0][1][:2] == truth[-1][1]     # re-acquired from the kept box
    for f in (3, 4):
        s = float(res[f][1][0][2])
        assert (s > thr) if method == 1 else (s < thr)


@pytest.mark.parametrize("kind", KINDS)
def test_frame0_boxes_larger_than_the_margin_box(kind):
    templs, frames, truth = _scene(17, kind, n_frames=5)
    tracks = [((0, 0, 76, 60), k) for k in range(4)] + [((5, 5, 70, 30), 1)]
    for method in (0, 4, 5):
        _compare(templs, frames, tracks, 2, method)


@pytest.mark.parametrize("rows_per_chunk", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_forced_chunks_carry_the_tracks(rows_per_chunk, kind):
    templs, frames, truth = _scene(23, kind, n_frames=8)
    ctx = _lib.default_context()
    old = ctx.get_option(_lib.OPT_BATCH_MAX_ROWS)
    ref = MTM.trackTemplates(templs, frames, _starts(truth[0], (7, 9), 4), 5, 5, 0.6)
    ctx.set_option(_lib.OPT_BATCH_MAX_ROWS, rows_per_chunk * frames[0].shape[0])
    try:
        res = _compare(templs, frames, _starts(truth[0], (7, 9), 4), 5, 5, min_score=0.6)
        res1 = _compare(templs, frames, _starts(truth[0], (7, 9), 2), 16, 1)
    finally:
        ctx.set_option(_lib.OPT_BATCH_MAX_ROWS, old)
    assert _key3(res) == _key3(ref)
    assert [fr[-1][0][1][:2] for fr in res1] == [t[-1] for t in truth]


def test_no_frames_and_no_tracks():
    templs, frames, truth = _scene(3, "u8", n_frames=3)
    assert MTM.trackTemplates(templs, [], _starts(truth[0], (7, 9), 3), 4) == []
    assert MTM.trackTemplates(templs, np.zeros((0, 60, 76), np.uint8), _starts(truth[0], (7, 9), 3), 4) == []
    assert MTM.trackTemplates(templs, frames, [], 4) == [[], [], []]
    m = MTM.TemplateMatcher(templs, 5)
    assert m.track(frames, [], 4) == [[], [], []] and m.track([], [((0, 0, 9, 9), 0)], 4) == []
    _compare(templs, frames, [], 4, 5, matcher=m)
    f = frames[0]
    assert _key(m.match(f)) == _key(MTM.matchTemplates(templs, f, 5))


@pytest.mark.parametrize("kind", KINDS)
def test_line_and_single_output_maps(kind):
    templs, frames, truth = _scene(29, kind, n_frames=6, step=1)
    (x0, y0), (x1, y1), (x2, y2) = truth[0][:3]
    tracks = [((x0, y0, 9, 7), 0),              # 1 x 1 map in frame 0
              ((x1, max(0, y1 - 3), 9, 14), 1),  # a column map
              ((max(0, x2 - 4), y2, 18, 7), 2)]  # a row map
    for method in range(6):
        _compare(templs, frames, tracks, 0, method)      # margin 0: every later map is 1 x 1
        _compare(templs, frames, tracks, 1, method)


def test_error_of_frame0_as_the_loop():
    templs, frames, truth = _scene(3, "u8", n_frames=3)
    _compare(templs, frames, [((0, 0, 5, 30), 0)], 4, 5)                 # template larger than its box
    _compare(templs, [f.astype(np.float32) for f in frames], _starts(truth[0], (7, 9), 3), 4, 5)
    masked = [(t[0], t[1], np.ones_like(t[1])) for t in templs]
    _compare(masked, frames, _starts(truth[0], (7, 9), 3), 4, 5)         # mask warnings, every frame
    _compare(masked, frames, _starts(truth[0], (7, 9), 3), 4, 3)         # masks with method 3: out of scope


def test_seeded_random_sweep():
    rng = np.random.RandomState(2026)
    for case in range(120):
        kind = KINDS[case % 3]
        hw = (int(rng.randint(20, 90)), int(rng.randint(20, 90)))
        th, tw = int(rng.randint(1, min(20, hw[0]))), int(rng.randint(1, min(20, hw[1])))
        n_tracks = int(rng.randint(1, 6))
        templs, frames, truth = _scene(1000 + case, kind, n_frames=int(rng.randint(1, 7)), hw=hw, templ_hw=(th, tw),
                                       n_tracks=n_tracks, step=int(rng.randint(0, 4)), flat=bool(rng.randint(0, 4) == 0))
        tracks = []
        for k in range(n_tracks):
            x, y = truth[0][k]
            if rng.randint(0, 3) == 0:          # a random box that may reach past the frame
                bx, by = int(rng.randint(0, hw[1] - tw + 1)), int(rng.randint(0, hw[0] - th + 1))
                tracks.append(((bx, by, tw + int(rng.randint(0, 40)), th + int(rng.randint(0, 40))), k))
            else:
                pad = int(rng.randint(0, 8))
                tracks.append(((max(0, x - pad), max(0, y - pad), tw + 2 * pad, th + 2 * pad), k))
        method = int(rng.randint(0, 6))
        margin = int(rng.choice([0, 1, 2, 3, 5, 8, 16, 40]))
        min_score = None
        if rng.randint(0, 3) == 0:
            min_score = float(rng.choice([0.2, 0.5, 0.9])) if method in (1, 3, 5) else float(rng.uniform(-1e6, 1e9))
        _compare(templs, frames, tracks, margin, method, min_score)
