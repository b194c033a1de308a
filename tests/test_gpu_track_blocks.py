"""More tracks than one 256-lane block of the update kernels (track_update_kernel / track_reupdate_kernel),
through Context directly: 257 tracks, of which the last lane of the first block and the first lane of the second pass and
fail min_score in different frames.  Every entry point equals the loop that defines it (MTM/tracking.py) written with
MTM.findMatchesInBoxes and next_box - one call per frame over every track's region, which is what a call per track
returns - byte for byte in the records; plain tracks equal singleton sets, and a call repeated gives identical bytes."""
import functools

import numpy as np
import pytest

import MTM
from MTM import _lib
from MTM.tracking import blend_template, next_box

pytestmark = pytest.mark.gpu

KINDS = ["u8", "rgb", "u16"]
N_TRACKS, N_FRAMES, HW, SIDE, MARGIN = 257, 4, (48, 64), 5, 2
METHOD, MIN_SCORE, RATE = 5, 0.9, 0.5
N_TEMPL, SPOTS_PER_ROW, N_SPOTS = 7, 7, 35      # spot s: row s // 7, column s % 7, shows template s % 7
EDGE = (254, 255, 256)                          # the 255th, 256th and 257th track: the end of block 0, the start of block 1


def _pixels(rng, shape, kind, hi=None):
    if kind == "u16":
        return rng.randint(0, hi or 65536, size=shape).astype(np.uint16)
    shape = tuple(shape) if kind == "u8" else tuple(shape) + (3,)
    return rng.randint(0, hi or 256, size=shape).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _scene(kind):
    """Dim noise frames with a 5 x 7 grid of spots, 9 pixels apart, that move by one pixel between frames; spot s shows
    template s % 7, except in the frames f with (s + f) % 4 == 0 and - column 6 - in frame 2, where it shows nothing: the
    track loses it there, and finds another spot of its column over the whole frame, or - column 6, frame 2 - none.  Track k
    follows spot k % 35 from a box 1 to 3 pixels wider than the template.  Returns (templates, frames, tracks as
    ((x, y, w, h), template))."""
    rng = np.random.RandomState({"u8": 1, "rgb": 2, "u16": 3}[kind])
    templs = [("t%d" % j, _pixels(rng, (SIDE, SIDE), kind)) for j in range(N_TEMPL)]
    at = [(4 + 9 * (s % SPOTS_PER_ROW), 4 + 9 * (s // SPOTS_PER_ROW)) for s in range(N_SPOTS)]
    frames = []
    for f in range(N_FRAMES):
        fr = _pixels(rng, HW, kind, hi=(65536 if kind == "u16" else 256) // 4)
        for s, (x, y) in enumerate(at):
            if (s + f) % 4 == 0 or (f == 2 and s % SPOTS_PER_ROW == 6):
                continue
            x, y = x + f % 2, y + (f // 2) % 2
            fr[y:y + SIDE, x:x + SIDE] = templs[s % N_TEMPL][1]
        frames.append(fr)
    tracks = []
    for k in range(N_TRACKS):
        (x, y), pad = at[k % N_SPOTS], 1 + k % 3
        tracks.append(((x - pad, y - pad, SIDE + 2 * pad, SIDE + 2 * pad), (k % N_SPOTS) % N_TEMPL))
    return templs, frames, tracks


def _passes(score):
    return float(score) > MIN_SCORE


def _set_of(j, n):
    return [(j + i) % N_TEMPL for i in range(n)]


@functools.lru_cache(maxsize=None)
def _loop(kind, reacquire=False, rate=None, set_size=1):
    """The defining loop, one findMatchesInBoxes call per frame (and one per frame for the second searches): the records
    as HIT_DTYPE, frame-major, and [(f, k, the box search passed, the frame's record passed)] per frame and track.
    `rate`: every track searches and blends a template of its own; the record names the list template it started from."""
    templs, frames, tracks = _scene(kind)
    idx = {t[0]: j for j, t in enumerate(templs)}
    cur = [templs[j][1] for _, j in tracks]
    box = [b for b, _ in tracks]
    rec = np.zeros(N_FRAMES * N_TRACKS, dtype=_lib.HIT_DTYPE)
    passed = []
    for fi, f in enumerate(frames):
        if rate is None:
            tl, sets = templs, [_set_of(j, set_size) for _, j in tracks]
        else:
            tl, sets = [("k%d" % k, c) for k, c in enumerate(cur)], [[k] for k in range(N_TRACKS)]
        found = MTM.findMatchesInBoxes(tl, f, list(zip(box, sets)), METHOD, N_object=1)
        hits = [max(h, key=lambda r: r[2]) for h in found]
        first = [_passes(h[2]) for h in hits]
        lost = [k for k, ok in enumerate(first) if not ok]
        if reacquire and lost:
            whole = (0, 0, HW[1], HW[0])
            again = MTM.findMatchesInBoxes(tl, f, [(whole, sets[k]) for k in lost], METHOD, N_object=1)
            for k, h in zip(lost, again):
                hits[k] = max(h, key=lambda r: r[2])
        for k, hit in enumerate(hits):
            (x, y, w, h), ok = hit[1], _passes(hit[2])
            rec[fi * N_TRACKS + k] = (idx[hit[0]] if rate is None else tracks[k][1], x, y, w, h, hit[2])
            passed.append((fi, k, first[k], ok))
            if rate is not None and ok:
                cur[k] = blend_template(cur[k], f[y:y + h, x:x + w], rate)
            box[k] = next_box(box[k], hit, MARGIN, f.shape, METHOD, MIN_SCORE)
    return rec, passed


def _units(tracks):
    units = np.zeros(len(tracks), dtype=_lib.BOX_UNIT_DTYPE)
    for i, ((x, y, w, h), j) in enumerate(tracks):
        units[i] = (j, y, x, min(HW[0], y + h) - y, min(HW[1], x + w) - x)
    return units


def _twice(call):
    a, b = call(), call()
    assert a.tobytes() == b.tobytes()
    return a


@pytest.mark.parametrize("kind", KINDS)
def test_257_tracks_equal_the_loop_in_every_entry_point(kind):
    templs, frames, tracks = _scene(kind)
    # the loop alone shows both outcomes at the block boundary and elsewhere: of the box search in each of the last two
    # edge tracks, and of the second search (column 6 finds nothing in frame 2) in other tracks
    for reacquire in (False, True):
        _, passed = _loop(kind, reacquire=reacquire)
        for k in EDGE[1:]:
            assert {p[2] for p in passed if p[1] == k} == {False, True}
        assert {p[2] for p in passed if p[1] < EDGE[0]} == {False, True}
        assert {p[3] for p in passed if not p[2]} == ({False, True} if reacquire else {False})
    assert all(p[3] for p in _loop(kind, reacquire=True)[1] if p[1] in EDGE)       # (the edge tracks are found again)

    units = _units(tracks)
    arrays = [t[1] for t in templs]
    one_off = np.arange(N_TRACKS + 1, dtype=np.int32)
    five_idx = np.array([_set_of(j, 5) for _, j in tracks], dtype=np.int32).ravel()
    ctx = _lib.default_context()
    with ctx.lock:
        ctx.set_templates([(a, None) for a in arrays], METHOD)
        plain = _twice(lambda: ctx.track_boxes(frames, units, MARGIN, MIN_SCORE))
        reacq = _twice(lambda: ctx.track_boxes_reacquire(frames, units, MARGIN, MIN_SCORE, 0, arrays)[0])
        reacq_a = _twice(lambda: ctx.track_boxes_reacquire(frames, units, MARGIN, MIN_SCORE, 128, arrays)[0])
        adapt = _twice(lambda: ctx.track_boxes_adapt(frames, units, MARGIN, MIN_SCORE, 128, arrays)[0])
        one = _twice(lambda: ctx.track_boxes_sets(frames, units, one_off, units["templ_idx"], MARGIN, MIN_SCORE)[0])
        one_r = _twice(lambda: ctx.track_boxes_sets(frames, units, one_off, units["templ_idx"], MARGIN, MIN_SCORE, True)[0])
        five = _twice(lambda: ctx.track_boxes_sets(frames, units, 5 * one_off, five_idx, MARGIN, MIN_SCORE)[0])
        five_r = _twice(lambda: ctx.track_boxes_sets(frames, units, 5 * one_off, five_idx, MARGIN, MIN_SCORE, True)[0])
    # plain tracks are singleton sets
    assert plain.tobytes() == one.tobytes()
    assert reacq.tobytes() == one_r.tobytes()
    # every call is its loop
    assert plain.tobytes() == _loop(kind)[0].tobytes()
    assert reacq.tobytes() == _loop(kind, reacquire=True)[0].tobytes()
    assert adapt.tobytes() == _loop(kind, rate=RATE)[0].tobytes()
    assert reacq_a.tobytes() == _loop(kind, reacquire=True, rate=RATE)[0].tobytes()
    assert five.tobytes() == _loop(kind, set_size=5)[0].tobytes()
    assert five_r.tobytes() == _loop(kind, reacquire=True, set_size=5)[0].tobytes()
