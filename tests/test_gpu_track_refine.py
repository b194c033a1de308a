"""MTM.trackTemplates(refine=True) / TemplateMatcher.track(refine=True) / Context.track_boxes_nbhd on the GPU:
the neighbourhoods scored inside the track call equal MTM.hitNeighbourhoods of each frame's records bit for bit - at frame
borders inside a stack of frames, for every template size around the kernel's chunk, for uint16 extremes - and the refined
result equals the loop of refineHits calls it replaces, floats compared with ==."""
import warnings

import numpy as np
import pytest

import MTM
from MTM import _lib, tracking
from MTM.subpixel import fit_offsets

pytestmark = pytest.mark.gpu

H, W = 60, 76
KINDS = ["u8", "rgb", "u16"]


# ---- scenes (as tests/test_gpu_track.py builds them) ---------------------------------------------------------------------
def _pixels(rng, shape, kind, hi=None):
    if kind == "u16":
        return rng.randint(0, hi or 65536, size=shape).astype(np.uint16)
    shape = shape if kind == "u8" else shape + (3,)
    return rng.randint(0, hi or 256, size=shape).astype(np.uint8)


def _scene(seed, kind, n_frames=6, hw=(H, W), templ_hw=(7, 9), n_tracks=4, step=3, corner=None, flat=False):
    """Dim noise frames (new noise in every frame) with each track's template pasted at a position that moves up to `step`
    pixels per frame (or `step` pixels per frame towards `corner`, where it stays)."""
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


# ---- the native call against hitNeighbourhoods -----------------------------------------------------------------------
def _native(templs, frames, tracks, margin, method, min_score=None):
    """(track_boxes' records, track_boxes_nbhd's records, its neighbourhoods) on the default context; boxes clipped to the
    frame as trackTemplates clips them."""
    fh, fw = frames[0].shape[:2]
    units = np.zeros(len(tracks), dtype=_lib.BOX_UNIT_DTYPE)
    for i, ((x, y, w, h), j) in enumerate(tracks):
        units[i] = (j, y, x, min(fh, y + h) - y, min(fw, x + w) - x)
    ctx = _lib.default_context()
    with ctx.lock:
        ctx.set_templates([(t[1], None) for t in templs], method)
        plain = ctx.track_boxes(frames, units, margin, min_score)
        rec, nb = ctx.track_boxes_nbhd(frames, units, margin, min_score)
    return plain, rec, nb


def _hits(templs, rec):
    return [(templs[int(r["templ_idx"])][0], (int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"])), r["score"]) for r in rec]


def _check_native(templs, frames, tracks, margin, method, min_score=None):
    """The contract of Context.track_boxes_nbhd; returns (records, neighbourhoods) shaped (F, T) and (F, T, 3, 3)."""
    frames = list(frames)
    plain, rec, nb = _native(templs, frames, tracks, margin, method, min_score)
    n, t = len(frames), len(tracks)
    assert rec.tobytes() == plain.tobytes()
    assert nb.shape == (n * t, 3, 3) and nb.dtype == np.float32
    for f in range(n):
        exp = MTM.hitNeighbourhoods(templs, frames[f], _hits(templs, rec[f * t:(f + 1) * t]), method)
        got = nb[f * t:(f + 1) * t]
        assert np.array_equal(got, exp, equal_nan=True), (f, method, np.argwhere(~((got == exp) | (np.isnan(got) & np.isnan(exp))))[:4])
    return rec.reshape(n, t), nb.reshape(n, t, 3, 3)


# ---- the public functions against the loop of refineHits calls -----------------------------------------------------------
def _outcome(call):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = call()
    return r, len(w)


def _rkey(res):
    out = []
    for fr in res:
        row = []
        for hits in fr:
            cell = []
            for label, (x, y, w, h), s in hits:
                assert type(x) is float and type(y) is float and type(w) is int and type(h) is int
                assert isinstance(s, np.float32)
                cell.append((label, x, y, w, h, s.tobytes()))
            row.append(cell)
        out.append(row)
    return out


def _refine_loop(templs, frames, res, method):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")     # (refineHits' own mask warnings are not the refined call's)
        return [[MTM.refineHits(templs, frames[f], res[f][k], method) for k in range(len(res[f]))] for f in range(len(res))]


def _compare(templs, frames, tracks, margin, method, min_score=None, matcher=None):
    res, n_warn = _outcome(lambda: MTM.trackTemplates(templs, frames, tracks, margin, method, min_score))
    exp = _refine_loop(templs, list(frames), res, method)
    got, n_got = _outcome(lambda: MTM.trackTemplates(templs, frames, tracks, margin, method, min_score, refine=True))
    assert n_got == n_warn
    assert _rkey(got) == _rkey(exp)         # (floats compared with ==)
    # the integer part is the unrefined call's
    assert [[[(h[0], h[1][2:], h[2].tobytes()) for h in c] for c in fr] for fr in got] == \
        [[[(h[0], h[1][2:], h[2].tobytes()) for h in c] for c in fr] for fr in res]
    if matcher is not None:
        got, n_got = _outcome(lambda: matcher.track(frames, tracks, margin, min_score, refine=True))
        assert n_got == n_warn
        assert _rkey(got) == _rkey(exp)
    return res, got


# ---- 1: neighbourhoods, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", range(6))
@pytest.mark.parametrize("margin", [0, 1, 16])
def test_neighbourhoods_equal_hit_neighbourhoods(kind, method, margin):
    templs, frames, truth = _scene(100 * method + margin, kind, step=max(1, margin // 2))
    _check_native(templs, frames, _starts(truth[0], (7, 9), 5), margin, method)


# ---- 2: the public contract --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_refined_tracks_equal_the_refine_loop_and_match_after(kind):
    templs, frames, truth = _scene(7, kind, n_frames=5)
    m = MTM.TemplateMatcher(templs, 5, N_object=1)
    _compare(templs, frames, _starts(truth[0], (7, 9), 6), 8, 5, matcher=m)
    # min_score set so that some hits fail it: they are refined and returned all the same
    for f in (2, 3):
        x, y = truth[f][1]
        frames[f][y:y + 7, x:x + 9] = 3
    res, got = _compare(templs, np.stack(frames), _starts(truth[0], (7, 9), 3), 4, 5, min_score=0.9, matcher=m)
    scores = [float(c[0][2]) for fr in res for c in fr]
    assert min(scores) < 0.9 < max(scores)
    assert all(len(c) == 1 for fr in got for c in fr)
    for method in (0, 1, 2, 3, 4):
        _compare(templs, frames, _starts(truth[0], (7, 9), 3), 4, method)
    for f in frames[:2]:                            # match() on the same matcher afterwards
        key = lambda hits: [(h[0], tuple(int(v) for v in h[1]), np.float32(h[2]).tobytes()) for h in hits]  # noqa: E731
        assert key(m.match(f)) == key(MTM.matchTemplates(templs, f, 5, 1))


def test_refined_call_adds_no_mask_warning():
    templs, frames, truth = _scene(3, "u8", n_frames=3)
    masked = [(t[0], t[1], np.ones_like(t[1])) for t in templs]
    tracks = _starts(truth[0], (7, 9), 3)
    res, n_warn = _outcome(lambda: MTM.trackTemplates(masked, frames, tracks, 4, 5))
    assert n_warn == len(tracks) * len(frames)
    _compare(masked, frames, tracks, 4, 5)


def test_duplicate_labels_follow_the_track_template():
    templs, frames, truth = _scene(9, "u8", n_frames=3)
    same = [("x", t[1]) for t in templs]            # refineHits would refuse the label lookup; the track knows its template
    tracks = _starts(truth[0], (7, 9), 3)
    got = MTM.trackTemplates(same, frames, tracks, 4, 5, refine=True)
    exp = MTM.trackTemplates(templs, frames, tracks, 4, 5, refine=True)
    assert [[[h[1:] for h in c] for c in fr] for fr in _rkey(got)] == [[[h[1:] for h in c] for c in fr] for fr in _rkey(exp)]


# ---- 3: frame borders inside a stack -----------------------------------------------------------------------------------
@pytest.mark.parametrize("frames_per_chunk", [1, 3, None])
@pytest.mark.parametrize("kind", KINDS)
def test_frame_borders_inside_a_stack(frames_per_chunk, kind):
    ctx = _lib.default_context()
    old = ctx.get_option(_lib.OPT_BATCH_MAX_ROWS)
    n_frames = 8
    per = frames_per_chunk or n_frames
    inner = [f for f in range(n_frames) if f % per not in (0, per - 1) and f != n_frames - 1]
    seen = set()
    if frames_per_chunk:
        ctx.set_option(_lib.OPT_BATCH_MAX_ROWS, frames_per_chunk * H)
    try:
        for corner in [(-1, -1), (1, -1), (-1, 1), (1, 1)]:
            # 20 pixels per frame: every track is in its corner from frame 4 on
            templs, frames, truth = _scene(31, kind, n_frames=n_frames, step=20, corner=corner)
            tracks = _starts(truth[0], (7, 9), 6)
            tracks += [((0, 0, 200, 12), 0), ((60, 0, 40, 40), 1), ((0, 50, 30, 30), 2), ((64, 52, 30, 30), 3)]
            for method in (1, 5):
                rec, nb = _check_native(templs, frames, tracks, 20, method)
                for f in inner:
                    for k in range(len(tracks)):
                        r, n = rec[f, k], nb[f, k]
                        assert np.isfinite(n[1, 1])
                        if r["y"] == 0:
                            seen.add("top")
                            assert np.isnan(n[0]).all()
                        if r["y"] == H - 7:
                            seen.add("bottom")
                            assert np.isnan(n[2]).all()
                        if r["x"] == 0:
                            seen.add("left")
                            assert np.isnan(n[:, 0]).all()
                        if r["x"] == W - 9:
                            seen.add("right")
                            assert np.isnan(n[:, 2]).all()
            _compare(templs, frames, tracks, 20, 5)
    finally:
        ctx.set_option(_lib.OPT_BATCH_MAX_ROWS, old)
    if inner:           # refined records on every border of a frame that is neither first nor last of its chunk
        assert seen == {"top", "bottom", "left", "right"}


# ---- 4: template sizes around the chunk --------------------------------------------------------------------------------
SIZES = [(1, 1), (3, 5), (16, 64), (17, 65), (7, 66), (40, 90), (40, 5), (3, 90)]   # the frame, 1-row and 1-column maps


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_template_sizes_around_the_chunk(kind, size):
    templs, frames, truth = _scene(41, kind, n_frames=3, hw=(40, 90), templ_hw=size, n_tracks=2, step=1)
    tracks = _starts(truth[0], size, 3) + [((0, 0, 90, 40), 1)]
    for method in range(6):
        rec, nb = _check_native(templs, frames, tracks, 2, method)
        if size == (40, 90):                # a 1 x 1 map: eight NaNs around the only window
            assert np.isnan(nb).sum() == 8 * nb.shape[0] * nb.shape[1] and not np.isnan(nb[:, :, 1, 1]).any()
        if size[0] == 40:
            assert np.isnan(nb[:, :, 0]).all() and np.isnan(nb[:, :, 2]).all()
        if size[1] == 90:
            assert np.isnan(nb[:, :, :, 0]).all() and np.isnan(nb[:, :, :, 2]).all()
    _compare(templs, frames, tracks, 2, 5)


# ---- 5: uint16 extremes ------------------------------------------------------------------------------------------------
def test_uint16_extremes():
    rng = np.random.RandomState(5)
    frames = []
    for _ in range(4):
        fr = rng.choice(np.array([0, 65535], dtype=np.uint16), size=(H, W))
        fr[4:58, 10:70] = 65535                      # a bright patch larger than the 48 x 48 template
        fr[rng.randint(0, H, 40), rng.randint(0, W, 40)] = 0
        frames.append(fr)
    templs = [("ones", np.full((48, 48), 65535, dtype=np.uint16)),
              ("bits", rng.choice(np.array([0, 65535], dtype=np.uint16), size=(7, 9))),
              ("cut", frames[0][1:20, 2:40].copy())]
    tracks = [((8, 2, 60, 56), 0), ((0, 0, W, H), 0), ((20, 20, 30, 30), 1), ((0, 0, 50, 30), 2)]
    for method in range(6):
        _check_native(templs, frames, tracks, 3, method)
        _compare(templs, frames, tracks, 3, method)


# ---- 6: more tracks than one update block ------------------------------------------------------------------------------
def test_more_tracks_than_one_update_block():
    templs, frames, truth = _scene(61, "u8", n_frames=3, templ_hw=(3, 3), n_tracks=2)
    rng = np.random.RandomState(6)
    tracks = []
    for k in range(300):
        x, y = int(rng.randint(0, W - 12)), int(rng.randint(0, H - 12))
        tracks.append(((x, y, int(rng.randint(3, 13)), int(rng.randint(3, 13))), k % 2))
    rec, nb = _check_native(templs, frames, tracks, 2, 5)
    assert nb.shape == (3, 300, 3, 3)
    _check_native(templs, frames, tracks, 1, 0)


# ---- 7: flat frames and constant patches -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_flat_frames_and_constant_patches(kind):
    templs, frames, truth = _scene(5, kind, n_frames=4, flat=True)
    top = 65536 if kind == "u16" else 256
    tracks = _starts(truth[0], (7, 9), 4) + [((2, 2, 26, 20), 0), ((3, 1, 30, 25), 1)]
    flat_frames = [f.copy() for f in frames]
    for f in flat_frames:
        f[...] = top // 5
    for method in range(6):
        _check_native(templs, frames, tracks, 3, method)
        _compare(templs, frames, tracks, 3, method)
        rec, nb = _check_native(templs, flat_frames, tracks, 2, method)
        ox, oy = fit_offsets(nb.reshape(-1, 3, 3), method)
        assert not ox.any() and not oy.any()        # every window of a constant frame ties (or is NaN): no offset
        res, got = _compare(templs, flat_frames, tracks, 2, method, min_score=0.5)
        assert [[c[0][1][:2] for c in fr] for fr in got] == [[tuple(float(v) for v in c[0][1][:2]) for c in fr] for fr in res]


# ---- 8: poison independence --------------------------------------------------------------------------------------------
def _cut(smap, x, y):
    out = np.full((3, 3), np.nan, dtype=np.float32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if 0 <= y + dy < smap.shape[0] and 0 <= x + dx < smap.shape[1]:
                out[1 + dy, 1 + dx] = smap[y + dy, x + dx]
    return out


@pytest.mark.parametrize("repeat", [0, 1])         # (consecutive tests: the fixture's two poison patterns)
def test_results_do_not_depend_on_poisoned_memory(repeat):
    for kind, method in [("u8", 5), ("rgb", 3), ("u16", 1)]:
        templs, frames, truth = _scene(50, kind, n_frames=5, templ_hw=(17, 65), n_tracks=3, step=2, hw=(H, 100))
        tracks = _starts(truth[0], (17, 65), 4)
        plain, rec, nb = _native(templs, frames, tracks, 4, method)
        assert rec.tobytes() == plain.tobytes()
        for f, fr in enumerate(frames):
            for k in range(3):
                r = rec[f * 3 + k]
                smap = MTM.computeScoreMap(templs[int(r["templ_idx"])][1], fr, method)
                assert np.array_equal(nb[f * 3 + k], _cut(smap, int(r["x"]), int(r["y"])), equal_nan=True), (kind, f, k)


# ---- 9: seeded sweep ---------------------------------------------------------------------------------------------------
def test_seeded_random_sweep():
    rng = np.random.RandomState(2027)
    for case in range(60):
        kind = KINDS[case % 3]
        hw = (int(rng.randint(20, 90)), int(rng.randint(20, 90)))
        th, tw = int(rng.randint(1, min(20, hw[0]))), int(rng.randint(1, min(20, hw[1])))
        n_tracks = int(rng.randint(1, 6))
        templs, frames, truth = _scene(3000 + case, kind, n_frames=int(rng.randint(1, 7)), hw=hw, templ_hw=(th, tw),
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


# ---- 10: positions -----------------------------------------------------------------------------------------------------
def test_positions_of_refined_and_unrefined_results():
    templs, frames, truth = _scene(11, "u8", n_frames=6, step=2)
    tracks = _starts(truth[0], (7, 9), 5)
    res = MTM.trackTemplates(templs, frames, tracks, 5, 5)
    got = MTM.trackTemplates(templs, frames, tracks, 5, 5, refine=True)
    exp = _refine_loop(templs, frames, res, 5)
    p = tracking.positions(got)
    assert p.shape == (6, 4, 2) and p.dtype == np.float64
    assert np.array_equal(p, np.array([[c[0][1][:2] for c in fr] for fr in exp], dtype=np.float64))
    assert np.array_equal(tracking.positions(res), np.array([[c[0][1][:2] for c in fr] for fr in res], dtype=np.float64))
    assert np.abs(p - tracking.positions(res)).max() <= 0.5
    assert np.array_equal(tracking.positions(res)[:, -1], np.array([t[-1] for t in truth], dtype=np.float64))


def test_no_frames_and_no_tracks():
    templs, frames, truth = _scene(3, "u8", n_frames=3)
    tracks = _starts(truth[0], (7, 9), 3)
    assert MTM.trackTemplates(templs, [], tracks, 4, refine=True) == []
    assert MTM.trackTemplates(templs, frames, [], 4, refine=True) == [[], [], []]
    m = MTM.TemplateMatcher(templs, 5)
    assert m.track(frames, [], 4, refine=True) == [[], [], []] and m.track([], tracks, 4, refine=True) == []
    ctx = _lib.default_context()
    units = np.zeros(0, dtype=_lib.BOX_UNIT_DTYPE)
    rec, nb = ctx.track_boxes_nbhd(frames, units, 4, None)
    assert len(rec) == 0 and nb.shape == (0, 3, 3) and nb.dtype == np.float32
