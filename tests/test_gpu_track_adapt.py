"""MTM.trackTemplates(update=...) / TemplateMatcher.track(update=...) / Context.track_boxes_adapt on the GPU:
every case equals the loop that defines it - findMatchesInBoxes with the track's own template, next_box, blend_template
of the hit's window where the hit passes - run through the public functions: hits, labels, boxes, float32 score bits, the
templates after the last frame, and the constants the device recomputed for them (equal to the host's for the returned
template).  Every comparison is equality."""
import numpy as np
import pytest

import MTM
from MTM import _lib
from MTM.tracking import blend_template, next_box

pytestmark = pytest.mark.gpu

KINDS = ["u8", "rgb", "u16"]
BIG, SMALL = (72, 96), (40, 48)


def _key(hits):
    return [(h[0], tuple(int(v) for v in h[1]), np.float32(h[2]).tobytes()) for h in hits]


def _key3(res):
    return [[_key(r) for r in fr] for fr in res]


def _top(kind):
    return 65536 if kind == "u16" else 256


def _pixels(rng, shape, kind, lo, hi):
    shape = tuple(shape) + ((3,) if kind == "rgb" else ())
    return rng.randint(lo, hi, size=shape).astype(np.uint16 if kind == "u16" else np.uint8)


def _scene(seed, kind, n_frames=8, hw=BIG, templ_hw=(7, 9), n_tracks=3, step=2, targets=None, start=None):
    """Dim noise frames.  Track k's object - a textured patch, first at start[k] (default: anywhere) - moves up to `step`
    pixels per frame (or `step` pixels per frame towards targets[k], where it stays), grows brighter with every frame (a
    ramp of 1 / 10 of its texture per frame), carries fresh noise of a few levels and one saturated pixel that wanders:
    its appearance drifts away from the template it started with.  Returns (templates: the objects as frame 0 shows them,
    frames, the objects' positions per frame)."""
    rng = np.random.RandomState(seed)
    th, tw = templ_hw
    top = _top(kind)
    base = [_pixels(rng, templ_hw, kind, top // 8, top // 2).astype(np.int64) for _ in range(n_tracks)]
    pos = [[int(rng.randint(0, hw[1] - tw + 1)), int(rng.randint(0, hw[0] - th + 1))] for _ in range(n_tracks)]
    if start is not None:
        pos = [list(p) for p in start]
    frames, truth, templs = [], [], None
    for f in range(n_frames):
        fr = _pixels(rng, hw, kind, 0, top // 16)
        looks = []
        for k in range(n_tracks):
            x, y = pos[k]
            look = base[k] + (base[k] * f) // 10 + rng.randint(0, top // 64, size=base[k].shape)
            if f > 0 and th * tw > 1:
                look[rng.randint(0, th), rng.randint(0, tw)] = top - 1
            look = np.clip(look, 0, top - 1).astype(fr.dtype)
            fr[y:y + th, x:x + tw] = look
            looks.append(look)
        if templs is None:
            templs = [("o%d" % k, looks[k].copy()) for k in range(n_tracks)]
        frames.append(fr)
        truth.append([tuple(p) for p in pos])
        for k, p in enumerate(pos):
            if targets is None or targets[k] is None:
                dx, dy = rng.randint(-step, step + 1), rng.randint(-step, step + 1)
            else:
                dx = int(np.clip(targets[k][0] - p[0], -step, step))
                dy = int(np.clip(targets[k][1] - p[1], -step, step))
            p[0] = int(np.clip(p[0] + dx, 0, hw[1] - tw))
            p[1] = int(np.clip(p[1] + dy, 0, hw[0] - th))
    return templs, frames, truth


def _starts(truth0, templ_hw, pad, idx=None):
    th, tw = templ_hw
    return [((max(0, x - pad), max(0, y - pad), tw + 2 * pad, th + 2 * pad), k if idx is None else idx[k])
            for k, (x, y) in enumerate(truth0)]


def _passes(score, method, min_score):
    if min_score is None:
        return True
    s, m = float(score), float(min_score)
    return s < m if method in (0, 1) else s > m


def _loop(templs, frames, tracks, margin, method, min_score, rate, refine=False):
    """The defining loop (MTM/tracking.py) on the public functions: (result [f][k], every track's last template)."""
    cur = [templs[j][1] for _, j in tracks]
    box = [b for b, _ in tracks]
    out = []
    for f in frames:
        row = []
        for k, (_, j) in enumerate(tracks):
            one = [(templs[j][0], cur[k])]
            r = MTM.findMatchesInBoxes(one, f, [box[k]], method, N_object=1)[0]
            hit = r[0]
            row.append(MTM.refineHits(one, f, [hit], method) if refine else r)      # (the template frame f was searched with)
            if _passes(hit[2], method, min_score):
                x, y, w, h = hit[1]
                cur[k] = blend_template(cur[k], f[y:y + h, x:x + w], rate)
            box[k] = next_box(box[k], hit, margin, f.shape, method, min_score)
        out.append(row)
    return out, cur


def _native_stats(templs, frames, tracks, margin, method, min_score, rate):
    """Context.track_boxes_adapt on the default context: (records, last templates, stats_out)."""
    fh, fw = frames[0].shape[:2]
    units = np.zeros(len(tracks), dtype=_lib.BOX_UNIT_DTYPE)
    for i, ((x, y, w, h), j) in enumerate(tracks):
        units[i] = (j, y, x, min(fh, y + h) - y, min(fw, x + w) - x)
    ctx = _lib.default_context()
    with ctx.lock:
        ctx.set_templates([(t[1], None) for t in templs], method)
        rec, nb, last, stats = ctx.track_boxes_adapt(list(frames), units, margin, min_score, int(round(rate * 256)),
                                                     [t[1] for t in templs])
    assert nb is None and stats.shape == (len(tracks), 7)
    return rec, last, stats


def _compare(templs, frames, tracks, margin, method, min_score=None, rate=0.5, must_differ=False):
    """trackTemplates(update=rate) against the loop: result and templates; the device's constants of the last templates
    against the host's.  Returns (result, templates)."""
    exp, exp_last = _loop(templs, list(frames), tracks, margin, method, min_score, rate)
    got, last = MTM.trackTemplates(templs, frames, tracks, margin, method, min_score, update=rate, return_templates=True)
    assert _key3(got) == _key3(exp)
    assert len(last) == len(tracks)
    for k, (t, e, (_, j)) in enumerate(zip(last, exp_last, tracks)):
        assert t.dtype == templs[j][1].dtype and t.shape == templs[j][1].shape, k
        assert np.array_equal(t, e), (k, method)
    rec, last2, stats = _native_stats(templs, frames, tracks, margin, method, min_score, rate)
    assert [(int(r["x"]), int(r["y"]), r["score"].tobytes()) for r in rec] == \
        [(h[0][1][0], h[0][1][1], h[0][2].tobytes()) for fr in got for h in fr]
    assert rec["templ_idx"].tolist() == [j for _, j in tracks] * len(frames)        # the list index, not the track
    for k, t in enumerate(last2):
        assert np.array_equal(t, last[k])
        host = _lib.debug_templ_stats(t, method)
        assert [float(v).hex() for v in stats[k]] == [float(v).hex() for v in host], (k, method)
    if must_differ:         # the objects drift: a call that ignored `update` would score otherwise
        plain = MTM.trackTemplates(templs, frames, tracks, margin, method, min_score)
        assert [h[0][2].tobytes() for fr in got for h in fr] != [h[0][2].tobytes() for fr in plain for h in fr]
    return got, last


# ---- pixel types, methods, rates -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", range(6))
def test_adaptive_equals_loop(kind, method):
    templs, frames, truth = _scene(100 + method, kind)
    tracks = _starts(truth[0], (7, 9), 3)
    got, _ = _compare(templs, frames, tracks, 3, method, must_differ=True)
    if method in (1, 3, 5):             # the normalised methods follow the objects
        assert [tuple(h[0][1][:2]) for h in got[-1]] == truth[-1]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rate", [1.0, 0.5, 1 / 256])
def test_rates(kind, rate):
    templs, frames, truth = _scene(7, kind, hw=SMALL, n_tracks=2)
    _, last = _compare(templs, frames, _starts(truth[0], (7, 9), 3), 3, 5, rate=rate, must_differ=True)
    if rate == 1.0:                     # the last template is the last hit's window
        for k, (x, y) in enumerate(truth[-1]):
            assert np.array_equal(last[k], frames[-1][y:y + 7, x:x + 9])


# ---- template sizes at the chunk edges of the window kernels (16 rows x 64 columns, quads of 4), frame corners -------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("templ_hw", [(1, 1), (5, 7), (16, 64), (17, 65), (33, 6)])
def test_template_sizes_and_frame_corners(kind, templ_hw):
    th, tw = templ_hw
    hw = SMALL if th * tw < 100 else BIG
    # object 0 is driven to frame position (0, 0), object 1 to (W - w, H - h): the adopted windows touch the first and the
    # last row and column of the frame
    corners = [(0, 0), (hw[1] - tw, hw[0] - th)]
    dx, dy, step, pad = (1, 1, 1, 1) if templ_hw == (1, 1) else (12, 9, 3, 3)
    start = [(dx, dy), (hw[1] - tw - dx, hw[0] - th - dy)]
    templs, frames, truth = _scene(th * 100 + tw, kind, hw=hw, templ_hw=templ_hw, n_tracks=2, step=step, targets=corners,
                                   start=start)
    assert truth[-1] == corners
    tracks = _starts(truth[0], templ_hw, pad)
    for method in (1, 5):
        # (a 1 x 1 template is constant: under method 5 its map is all ones, and nothing tells one pixel from another)
        got, _ = _compare(templs, frames, tracks, pad, method, must_differ=templ_hw != (1, 1))
        if method == 1 or templ_hw != (1, 1):
            assert [tuple(h[0][1][:2]) for h in got[-1]] == corners


# ---- min_score: no adoption while the object is gone -------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", [1, 5])
def test_min_score_holds_box_and_template_while_the_object_is_gone(kind, method):
    templs, frames, truth = _scene(13, kind, n_tracks=2, step=1, start=[(10, 10), (60, 40)])
    rng = np.random.RandomState(99)
    for f in (3, 4):                                # track 1's object is replaced by noise for two frames
        x, y = truth[f][1]
        frames[f][y:y + 7, x:x + 9] = _pixels(rng, (7, 9), kind, 0, _top(kind) // 16)
    thr = 0.25 if method == 1 else 0.55
    tracks = _starts(truth[0], (7, 9), 3)
    got, last = _compare(templs, frames, tracks, 6, method, min_score=thr, must_differ=True)
    for f in range(len(frames)):
        gone = [False, f in (3, 4)]
        for k in range(2):
            s = float(got[f][k][0][2])
            assert ((s > thr) if method == 1 else (s < thr)) == gone[k], (f, k, s)
    assert [tuple(h[0][1][:2]) for h in got[-1]] == truth[-1]      # re-acquired from the held box, with the held template
    # held: track 1's template after frame 4 is its template after frame 2; it adapts again afterwards
    _, last2 = MTM.trackTemplates(templs, frames[:3], tracks, 6, method, thr, update=0.5, return_templates=True)
    _, last4 = MTM.trackTemplates(templs, frames[:5], tracks, 6, method, thr, update=0.5, return_templates=True)
    assert np.array_equal(last2[1], last4[1]) and not np.array_equal(last2[0], last4[0])
    assert not np.array_equal(last[1], last4[1])


# ---- tracks and list templates -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_tracks_of_one_list_template_diverge_and_a_duplicate_track_repeats(kind):
    templs, frames, truth = _scene(17, kind, n_tracks=3)
    # tracks 0 and 1 both start from list template 0 (object 1 begins as a copy of object 0's look, then drifts on its own);
    # track 3 repeats track 2
    x, y = truth[0][1]
    frames[0][y:y + 7, x:x + 9] = templs[0][1]
    tracks = _starts(truth[0], (7, 9), 3, idx=[0, 0, 2])
    tracks.append(tracks[2])
    got, last = _compare(templs, frames, tracks, 3, 5, must_differ=True)
    assert not np.array_equal(last[0], last[1])
    assert np.array_equal(last[2], last[3])
    assert [_key(fr[2]) for fr in got] == [_key(fr[3]) for fr in got]
    assert all(fr[0][0][0] == fr[1][0][0] == "o0" for fr in got)


@pytest.mark.parametrize("kind", KINDS)
def test_flat_regions_with_ccoeff_normed(kind):
    """Method 5 and constant pixels: a track that starts inside a constant region (its template turns constant at the
    first adoption: all_ones, a map of ones) and one that drifts onto it."""
    top = _top(kind)
    templs, frames, truth = _scene(19, kind, n_tracks=2, step=3, targets=[None, (8, 8)])
    for fr in frames:
        fr[:30, :40] = top // 3
    tracks = [((4, 4, 20, 18), 0), _starts(truth[0], (7, 9), 3)[1]]
    for rate in (1.0, 0.5):
        _, last = _compare(templs, frames, tracks, 3, 5, rate=rate)
    rec, last, stats = _native_stats(templs, frames, tracks, 3, 5, None, 1.0)
    assert stats[0][6] == 1.0 and np.all(last[0] == top // 3)


# ---- chunks of frames --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_forced_chunks_carry_the_templates(kind):
    templs, frames, truth = _scene(23, kind, hw=SMALL)
    tracks = _starts(truth[0], (7, 9), 3)
    ctx = _lib.default_context()
    old = ctx.get_option(_lib.OPT_BATCH_MAX_ROWS)
    ref, ref_last = MTM.trackTemplates(templs, frames, tracks, 3, 5, 0.3, update=0.5, return_templates=True)
    ref_r = MTM.trackTemplates(templs, frames, tracks, 3, 5, 0.3, update=0.5, refine=True)
    ctx.set_option(_lib.OPT_BATCH_MAX_ROWS, 2 * frames[0].shape[0])         # two frames per chunk
    try:
        got, last = _compare(templs, frames, tracks, 3, 5, min_score=0.3, must_differ=True)
        got_r = MTM.trackTemplates(templs, frames, tracks, 3, 5, 0.3, update=0.5, refine=True)
    finally:
        ctx.set_option(_lib.OPT_BATCH_MAX_ROWS, old)
    assert _key3(got) == _key3(ref)
    assert all(np.array_equal(a, b) for a, b in zip(last, ref_last))
    assert repr(got_r) == repr(ref_r)


# ---- refine=True -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", [1, 4, 5])
def test_refined_adaptive_equals_refine_hits_with_the_template_of_the_search(kind, method):
    templs, frames, truth = _scene(29 + method, kind, hw=SMALL, n_tracks=2)
    tracks = _starts(truth[0], (7, 9), 3)
    exp, exp_last = _loop(templs, frames, tracks, 3, method, None, 0.5, refine=True)
    got, last = MTM.trackTemplates(templs, frames, tracks, 3, method, update=0.5, refine=True, return_templates=True)
    plain = MTM.trackTemplates(templs, frames, tracks, 3, method, update=0.5)
    n_moved = 0
    for f in range(len(frames)):
        for k in range(len(tracks)):
            (gl, (gx, gy, gw, gh), gs), = got[f][k]
            (el, (ex, ey, ew, eh), es), = exp[f][k]
            assert type(gx) is float and type(gy) is float
            assert (gl, gx, gy, gw, gh, gs.tobytes()) == (el, ex, ey, ew, eh, np.float32(es).tobytes())     # floats with ==
            p = plain[f][k][0]
            assert abs(gx - p[1][0]) <= 0.5 and abs(gy - p[1][1]) <= 0.5 and gs.tobytes() == p[2].tobytes()
            n_moved += gx != p[1][0] or gy != p[1][1]
    assert n_moved > 0
    assert all(np.array_equal(a, b) for a, b in zip(last, exp_last))


# ---- TemplateMatcher: the resident templates stay as they are ---------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_matcher_keeps_its_templates(kind):
    templs, frames, truth = _scene(31, kind, hw=SMALL, n_tracks=3)
    tracks = _starts(truth[0], (7, 9), 3)
    m = MTM.TemplateMatcher(templs, 5, N_object=2)
    before = [_key(m.match(f)) for f in frames[:2]]
    plain_before = _key3(m.track(frames, tracks, 3))
    exp, exp_last = _loop(templs, frames, tracks, 3, 5, None, 0.5)
    got, last = m.track(frames, tracks, 3, update=0.5, return_templates=True)
    assert _key3(got) == _key3(exp) and all(np.array_equal(a, b) for a, b in zip(last, exp_last))
    assert _key3(got) != plain_before
    assert [_key(m.match(f)) for f in frames[:2]] == before
    assert _key3(m.track(frames, tracks, 3)) == plain_before == _key3(MTM.trackTemplates(templs, frames, tracks, 3, 5))
    # in pieces: the second half carries on from the first half's templates
    half, mid = m.track(frames[:4], tracks, 3, update=0.5, return_templates=True)
    boxes = [next_box(b, h[0], 3, frames[0].shape, 5) for (b, _), h in zip(tracks, half[-1])]
    rest = MTM.trackTemplates([(templs[j][0], t) for t, (_, j) in zip(mid, tracks)], frames[4:],
                              [(b, k) for k, b in enumerate(boxes)], 3, 5, update=0.5)
    assert _key3(half) + _key3(rest) == _key3(got)
