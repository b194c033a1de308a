"""MTM.trackTemplates(reacquire=True) / TemplateMatcher.track(reacquire=True) on the GPU: every case equals
the loop that defines it (MTM/tracking.py) written with MTM.findMatchesInBoxes and next_box - a track whose hit in its box
does not pass min_score is searched again over the whole frame - in hits, labels, boxes, float32 score bits, exceptions
and warning counts.  The loop also reports which (frame, track) pairs it searched twice and whether that recovered the
track, and the tests assert those facts about the reference, so that no comparison passes with nothing re-acquired."""
import warnings

import numpy as np
import pytest

import MTM
from MTM import _lib, tracking
from MTM.tracking import blend_template, next_box

pytestmark = pytest.mark.gpu

KINDS = ["u8", "rgb", "u16"]
GRID = 2048             # work-groups of one track_reacquire_kernel launch (kTrackReacquireGrid, csrc/mtm_track.hip)


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


def _scene(seed, kind, n_frames=7, hw=(60, 76), sizes=((7, 9),) * 3, step=1, jumps=None, blank=(), absent=None):
    """tests/test_gpu_track.py's recipe: dim noise frames (below a quarter of the range) with each track's template pasted
    at a position that moves up to `step` pixels per frame.  jumps[(f, k)] = (dx, dy): after frame f track k's object also
    moves by that much, modulo the size of its map (out of any box around it).  `blank`: frames that show no object.
    absent[k] = f: track k's object is gone from frame f on.  Returns (templates, frames, positions per frame)."""
    rng = np.random.RandomState(seed)
    top = _top(kind)
    n = len(sizes)
    templs = [("o%d" % k, _pixels(rng, sizes[k], kind)) for k in range(n)]
    pos = [[int(rng.randint(0, hw[1] - tw + 1)), int(rng.randint(0, hw[0] - th + 1))] for th, tw in sizes]
    frames, truth = [], []
    for f in range(n_frames):
        fr = _pixels(rng, hw, kind, hi=top // 4)
        for k, (th, tw) in enumerate(sizes):
            x, y = pos[k]
            if f not in blank and not (absent and k in absent and f >= absent[k]):
                fr[y:y + th, x:x + tw] = templs[k][1]
        frames.append(fr)
        truth.append([tuple(p) for p in pos])
        for k, p in enumerate(pos):
            th, tw = sizes[k]
            dx, dy = rng.randint(-step, step + 1), rng.randint(-step, step + 1)
            p[0] = int(np.clip(p[0] + dx, 0, hw[1] - tw))
            p[1] = int(np.clip(p[1] + dy, 0, hw[0] - th))
            if jumps and (f, k) in jumps:
                p[0] = (p[0] + jumps[(f, k)][0]) % (hw[1] - tw + 1)
                p[1] = (p[1] + jumps[(f, k)][1]) % (hw[0] - th + 1)
    return templs, frames, truth


def _starts(truth0, sizes, pad):
    return [((max(0, x - pad), max(0, y - pad), tw + 2 * pad, th + 2 * pad), k)
            for k, ((x, y), (th, tw)) in enumerate(zip(truth0, sizes))]


def _thr(method, templs):
    """The thresholds of the jump scene: far from both an exact copy's score and a noise window's."""
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


def _loop(templs, frames, tracks, margin, method, min_score, refine=False, rate=None):
    """The defining loop on the public functions.  Returns (result [f][k], [(f, k, recovered)] for every second search,
    every track's last template).  With `rate` the track's own template is searched (update's loop); with `refine` the
    frame's final record is refined with the template the frame was searched with.  The second search is silent: the
    call emits the mask warnings of the call without reacquire."""
    cur = [templs[j][1] for _, j in tracks]
    box = [b for b, _ in tracks]
    out, again = [], []
    for fi, f in enumerate(frames):
        H, W = f.shape[:2]
        row = []
        for k, (_, j) in enumerate(tracks):
            tl, idx = (templs, j) if rate is None else ([(templs[j][0], cur[k])], 0)
            hit = MTM.findMatchesInBoxes(tl, f, [(box[k], [idx])], method, N_object=1)[0][0]
            if not _passes(hit[2], method, min_score):
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    hit = MTM.findMatchesInBoxes(tl, f, [((0, 0, W, H), [idx])], method, N_object=1)[0][0]
                again.append((fi, k, _passes(hit[2], method, min_score)))
            row.append(MTM.refineHits(tl, f, [hit], method) if refine else [hit])
            if rate is not None and _passes(hit[2], method, min_score):
                x, y, w, h = hit[1]
                cur[k] = blend_template(cur[k], f[y:y + h, x:x + w], rate)
            box[k] = next_box(box[k], hit, margin, f.shape, method, min_score)
        out.append(row)
    return out, again, cur


def _outcome(call):
    """(result, (exception type, message) or None, number of warnings)"""
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        try:
            r, e = call(), None
        except Exception as ex:  # noqa: BLE001 - compared with the loop's
            r, e = None, (type(ex), str(ex))
    return r, e, len(w)


def _compare(templs, frames, tracks, margin, method, min_score, matcher=None):
    """trackTemplates(reacquire=True) against the loop: result, exception, warning count.  Returns (the loop's result,
    its second searches)."""
    exp = _outcome(lambda: _loop(templs, list(frames), tracks, margin, method, min_score))
    got = _outcome(lambda: MTM.trackTemplates(templs, frames, tracks, margin, method, min_score, reacquire=True))
    assert got[1] == exp[1]
    assert got[2] == exp[2]
    if exp[1] is not None:
        return None, None
    assert _key3(got[0]) == _key3(exp[0][0])
    if matcher is not None:
        got = _outcome(lambda: matcher.track(frames, tracks, margin, min_score, reacquire=True))
        assert got[1] is None and _key3(got[0]) == _key3(exp[0][0])
    return exp[0][0], exp[0][1]


# ---- the jump scene ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", range(6))
def test_jump_scene_is_recovered_as_the_loop_recovers_it(kind, method):
    sizes = ((7, 9),) * 3
    templs, frames, truth = _scene(13, kind, jumps={(1, 1): (35, 25), (3, 1): (35, 25)})
    tracks = _starts(truth[0], sizes, 3)
    thr = _thr(method, templs)
    exp, again = _compare(templs, frames, tracks, 4, method, thr)
    # the reference loop re-searches exactly twice, recovers both times, and every record is at the pasted position
    assert again == [(2, 1, True), (4, 1, True)]
    assert [[r[0][1][:2] for r in fr] for fr in exp] == truth
    # without reacquire the track stays lost
    plain = MTM.trackTemplates(templs, frames, tracks, 4, method, thr)
    assert tracking.lost(plain, method, thr)[2:4, 1].all() and not tracking.lost(exp, method, thr).any()


# ---- the geometry of the whole-frame search ----------------------------------------------------------------------------
GEOMETRY = {
    # name: (frame, template sizes, jumps)
    "two lds chunks each way": ((40, 150), ((17, 70),), {(1, 0): (40, 12)}),
    "map 16 x 16": ((22, 24), ((7, 9),), {(1, 0): (8, 8)}),
    "map 17 x 17": ((23, 25), ((7, 9),), {(1, 0): (8, 8)}),
    "map 1 x 1": ((12, 14), ((12, 14),), {}),
    "map 1 x n": ((12, 40), ((12, 9),), {(1, 0): (16, 0)}),
    "two sizes lost together": ((50, 64), ((7, 9), (11, 5)), {(1, 0): (25, 20), (1, 1): (30, 18)}),
}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(GEOMETRY))
def test_geometry_of_the_whole_frame_search(name, kind):
    hw, sizes, jumps = GEOMETRY[name]
    templs, frames, truth = _scene(41, kind, n_frames=5, hw=hw, sizes=sizes, jumps=jumps, blank=(3,))
    tracks = _starts(truth[0], sizes, 2)
    for method in (1, 4, 5):
        exp, again = _compare(templs, frames, tracks, 2, method, _thr(method, templs))
        # the blank frame is searched twice in vain by every track; a jump is searched twice and recovered
        assert [a for a in again if a[0] == 3] == [(3, k, False) for k in range(len(sizes))]
        for (f, k) in jumps:
            assert (f + 1, k, True) in again
            assert exp[f + 1][k][0][1][:2] == truth[f + 1][k]


# ---- every track lost at once: the grid-stride loop --------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_all_tracks_lost_at_once_and_more_items_than_work_groups(kind):
    n, hw, sizes = 12, (200, 300), ((7, 9),) * 12
    tiles = -(-(hw[0] - 7 + 1) // 16) * -(-(hw[1] - 9 + 1) // 16)
    assert n * tiles == 2964 and n * tiles > GRID           # some work-group walks more than one item
    jumps = {(2, k): (100 + 7 * k, 60 + 5 * k) for k in range(n)}
    templs, frames, truth = _scene(77, kind, n_frames=5, hw=hw, sizes=sizes, jumps=jumps, blank=(2,))
    tracks = _starts(truth[0], sizes, 3)
    exp, again = _compare(templs, frames, tracks, 3, 5, 0.95)
    assert [a for a in again if a[0] == 2] == [(2, k, False) for k in range(n)]        # nothing anywhere: boxes kept
    assert [a for a in again if a[0] == 3] == [(3, k, True) for k in range(n)]         # the objects return elsewhere
    assert [r[0][1][:2] for r in exp[3]] == truth[3] and [r[0][1][:2] for r in exp[4]] == truth[4]
    assert tracking.lost(exp, 5, 0.95).tolist() == [[f == 2] * n for f in range(5)]


# ---- lost in frame 0, never found --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_lost_in_frame_0(kind):
    sizes = ((7, 9),) * 3
    templs, frames, truth = _scene(19, kind, n_frames=4)
    tracks = [(((x + 30) % 60, (y + 25) % 40, 15, 13), k) for k, (x, y) in enumerate(truth[0])]    # the boxes miss
    for method in range(6):
        exp, again = _compare(templs, frames, tracks, 4, method, _thr(method, templs))
        assert [a for a in again if a[0] == 0] == [(0, k, True) for k in range(3)]
        assert [r[0][1][:2] for r in exp[0]] == truth[0]


@pytest.mark.parametrize("kind", KINDS)
def test_never_found_again(kind):
    sizes = ((7, 9),) * 3
    templs, frames, truth = _scene(24, kind, n_frames=6, absent={1: 2})
    tracks = _starts(truth[0], sizes, 3)
    for method in (0, 1, 2, 3, 4, 5):
        thr = _thr(method, templs)
        exp, again = _compare(templs, frames, tracks, 4, method, thr)
        assert again == [(f, 1, False) for f in range(2, 6)]          # every frame tries again, in vain
        want = np.zeros((6, 3), bool)
        want[2:, 1] = True
        assert np.array_equal(tracking.lost(exp, method, thr), want)
        # the records are whole-frame extrema: what a search of the whole frame returns
        for f in range(2, 6):
            H, W = frames[f].shape[:2]
            whole = MTM.findMatchesInBoxes(templs, frames[f], [((0, 0, W, H), [1])], method, N_object=1)[0]
            assert _key(exp[f][1]) == _key(whole)


# ---- ties --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_ties_in_flat_frames_and_a_flat_template(kind):
    sizes = ((7, 9),) * 3
    templs, frames, truth = _scene(5, kind, n_frames=4)
    top = _top(kind)
    templs[0] = ("flat", np.full_like(templs[0][1], top // 2))           # all_ones under method 5
    flat = [np.full_like(f, top // 5) for f in frames]
    half = [f.copy() for f in frames]
    for f in half:
        f[:30, :40] = top // 3                      # a constant patch: tied scores, first in row-major order
    tracks = _starts(truth[0], sizes, 4) + [((30, 20, 30, 25), 0), ((45, 30, 25, 20), 1)]
    n_again = 0
    for method in range(6):
        for fr in (flat, half, frames):
            _, again = _compare(templs, fr, tracks, 2, method, _thr(method, templs[1:]))
            n_again += len(again)
    assert n_again > 0


# ---- chunks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_one_frame_per_chunk_gives_the_unforced_result(kind):
    sizes = ((7, 9),) * 3
    templs, frames, truth = _scene(13, kind, jumps={(1, 1): (35, 25), (3, 1): (35, 25)}, blank=(5,))
    tracks = _starts(truth[0], sizes, 3)
    ctx = _lib.default_context()
    old = ctx.get_option(_lib.OPT_BATCH_MAX_ROWS)
    ref = MTM.trackTemplates(templs, frames, tracks, 4, 5, 0.95, reacquire=True)
    ctx.set_option(_lib.OPT_BATCH_MAX_ROWS, frames[0].shape[0])
    try:
        exp, again = _compare(templs, frames, tracks, 4, 5, 0.95)
    finally:
        ctx.set_option(_lib.OPT_BATCH_MAX_ROWS, old)
    assert _key3(ref) == _key3(exp)
    assert (2, 1, True) in again and (5, 0, False) in again


# ---- compositions ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("refine,rate", [(True, None), (False, 0.5), (True, 0.5)])
def test_compositions_equal_their_loops(kind, refine, rate):
    sizes = ((7, 9),) * 3
    templs, frames, truth = _scene(13, kind, jumps={(1, 1): (35, 25), (3, 1): (35, 25)}, blank=(5,))
    tracks = _starts(truth[0], sizes, 3) + [(_starts(truth[0], sizes, 3)[1][0], 1)]        # two tracks of one template
    for method in (1, 5):
        thr = _thr(method, templs)
        exp, again, exp_last = _loop(templs, frames, tracks, 4, method, thr, refine=refine, rate=rate)
        assert (2, 1, True) in again and (4, 1, True) in again and (5, 0, False) in again
        got, last = MTM.trackTemplates(templs, frames, tracks, 4, method, thr, refine=refine, update=rate, reacquire=True,
                                       return_templates=True)
        for f in range(len(frames)):
            for k in range(len(tracks)):
                (g,), (e,) = got[f][k], exp[f][k]
                assert g[0] == e[0] and g[1] == e[1] and np.float32(g[2]).tobytes() == np.float32(e[2]).tobytes(), (f, k)
                assert all(type(v) is (float if refine else int) for v in g[1][:2])
        assert len(last) == len(tracks)
        for t, e in zip(last, exp_last):
            assert t.dtype == e.dtype and np.array_equal(t, e)


# ---- TemplateMatcher ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_matcher_track_equals_the_function_and_match_after(kind):
    sizes = ((7, 9),) * 3
    templs, frames, truth = _scene(13, kind, jumps={(1, 1): (35, 25), (3, 1): (35, 25)})
    m = MTM.TemplateMatcher(templs, 5, N_object=1)
    exp, again = _compare(templs, frames, _starts(truth[0], sizes, 3), 4, 5, 0.95, matcher=m)
    assert len(again) == 2
    got = m.track(np.stack(frames), _starts(truth[0], sizes, 3), 4, 0.95, reacquire=True, refine=True)
    assert got == MTM.trackTemplates(templs, frames, _starts(truth[0], sizes, 3), 4, 5, 0.95, reacquire=True, refine=True)
    for f in frames[:2]:                            # match() on the same matcher afterwards
        assert _key(m.match(f)) == _key(MTM.matchTemplates(templs, f, 5, 1))


# ---- determinism, frame 0's errors and warnings ------------------------------------------------------------------------
def test_the_same_call_twice_gives_identical_keys():
    n, sizes = 12, ((7, 9),) * 12
    jumps = {(f, k): (20 + k, 15 + k) for f in (0, 2) for k in range(n)}
    templs, frames, truth = _scene(3, "u8", n_frames=5, hw=(90, 120), sizes=sizes, jumps=jumps)
    tracks = _starts(truth[0], sizes, 3)
    a = MTM.trackTemplates(templs, frames, tracks, 3, 5, 0.95, reacquire=True)
    b = MTM.trackTemplates(templs, frames, tracks, 3, 5, 0.95, reacquire=True)
    assert _key3(a) == _key3(b)
    assert not tracking.lost(a, 5, 0.95)[[0, 1, 3]].all()


def test_frame0_errors_and_mask_warnings_as_the_loop():
    sizes = ((7, 9),) * 3
    templs, frames, truth = _scene(13, "u8", jumps={(1, 1): (35, 25)})
    tracks = _starts(truth[0], sizes, 3)
    _compare(templs, frames, [((0, 0, 5, 30), 0)], 4, 5, 0.95)                  # template larger than its box
    _compare(templs, [f.astype(np.float32) for f in frames], tracks, 4, 5, 0.95)
    masked = [(t[0], t[1], np.ones_like(t[1])) for t in templs]
    _, again = _compare(masked, frames, tracks, 4, 5, 0.95)                     # mask warnings: one per track and frame
    assert again == [(2, 1, True)]
    _compare(masked, frames, tracks, 4, 3, 0.95)                                # masks with method 3: out of scope
    with pytest.raises(_lib.MtmError):                                          # the native call needs use_min
        ctx = _lib.default_context()
        with ctx.lock:
            ctx.set_templates([(t[1], None) for t in templs], 5)
            units = np.zeros(1, dtype=_lib.BOX_UNIT_DTYPE)
            units[0] = (0, 0, 0, 20, 20)
            ctx.track_boxes_reacquire(frames, units, 4, None, 0, [t[1] for t in templs])


# ---- seeded sweep ------------------------------------------------------------------------------------------------------
def test_seeded_random_sweep():
    rng = np.random.RandomState(2027)
    recovered = vain = 0
    for case in range(40):
        kind = KINDS[case % 3]
        method = int(rng.randint(0, 6))
        hw = (int(rng.randint(24, 80)), int(rng.randint(24, 80)))
        n = int(rng.randint(1, 5))
        sizes = tuple((int(rng.randint(1, min(18, hw[0] // 2))), int(rng.randint(1, min(18, hw[1] // 2)))) for _ in range(n))
        n_frames = int(rng.randint(2, 7))
        jumps = {(int(rng.randint(0, n_frames)), int(rng.randint(0, n))): (int(rng.randint(10, 40)), int(rng.randint(10, 40)))
                 for _ in range(int(rng.randint(0, 4)))}
        absent = {int(rng.randint(0, n)): int(rng.randint(0, n_frames))} if rng.randint(0, 3) == 0 else None
        blank = (int(rng.randint(0, n_frames)),) if rng.randint(0, 4) == 0 else ()
        templs, frames, truth = _scene(3000 + case, kind, n_frames=n_frames, hw=hw, sizes=sizes,
                                       step=int(rng.randint(0, 3)), jumps=jumps, absent=absent, blank=blank)
        tracks = _starts(truth[0], sizes, int(rng.randint(0, 5)))
        margin = int(rng.choice([0, 1, 2, 4, 8, 30]))
        exp, again = _compare(templs, frames, tracks, margin, method, _thr(method, templs))
        recovered += any(a[2] for a in again)
        vain += any(not a[2] for a in again)
    # the reference loop: cases with a second search that recovers, cases with one in vain
    assert recovered >= 10 and vain >= 5, (recovered, vain)
