"""MTM.matchBlocksStack(offsets=) and MTM.matchBlocksStackMultipass on the GPU.  blocks_plane_peak_kernel on constructed
sums (mtm_debug_plane_peaks with a context) against the cell-by-cell restatement and numpy plane_peaks, planes and records
bit for bit; matchBlocksStack(offsets=) per pair against the loop of matchBlocks(offsets=) and its ensemble planes against a
restatement from MTM.computeScoreMap of host-cut blocks on host-cut crops (tests/blocks_stack_passes_model.py);
matchBlocksStackMultipass per pair against the loop of matchBlocksMultipass and on ensemble planes against the by-hand loop
its docstring writes out; frame chunks change no byte; the context's templates and options are left alone."""
import warnings

import numpy as np
import pytest

import MTM
import blocks_stack_passes_model as M
from MTM import _lib
from MTM import blocks as B
from test_blocks_stack_passes_cpu import PASSES_2, PASSES_3, check_plane_peaks

pytestmark = pytest.mark.gpu


class _Opt:
    """An option of the default context for the duration of a block (put back afterwards)."""
    def __init__(self, opt, value):
        self.opt, self.value = opt, value

    def __enter__(self):
        self.ctx = _lib.default_context()
        self.old = self.ctx.get_option(self.opt)
        self.ctx.set_option(self.opt, self.value)
        return self

    def __exit__(self, *exc):
        self.ctx.set_option(self.opt, self.old)


def _movie(seed, n, kind, hw, step=(1, -1), noise=3):
    """n frames: a random image moved by `step` = (dx, dy) from frame to frame (wrapping around), with a little noise."""
    rng = np.random.RandomState(seed)
    top = 65536 if kind == "u16" else 256
    shape = hw + (3,) if kind == "rgb" else hw
    base = rng.randint(0, top, size=shape)
    out = []
    for f in range(n):
        a = np.roll(base, (f * step[1], f * step[0]), axis=(0, 1)) + rng.randint(-noise, noise + 1, size=shape)
        out.append(np.clip(a, 0, top - 1).astype(np.uint16 if kind == "u16" else np.uint8))
    return out


def _quiet(f, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("error")              # no warnings are emitted
        return f(*a, **kw)


def _same(got, exp):
    assert len(got) == len(exp)
    for k, (a, b) in enumerate(zip(got, exp)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            same = (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else a == b
            bad = np.argwhere(~same)
            assert len(bad) == 0 and a.dtype.kind == "f", (k, bad[:5], [(a[tuple(i)], b[tuple(i)]) for i in bad[:5]])
            # (equal as numbers: then equal in every bit but a NaN's payload)
            num = ~np.isnan(a)
            assert a[num].tobytes() == b[num].tobytes(), k


# ---- blocks_plane_peak_kernel on constructed sums ----------------------------------------------------------------------------
@pytest.mark.parametrize("pairs", [1, 7])
@pytest.mark.parametrize("method", [0, 5])
@pytest.mark.parametrize("side", [1, 3, 17, 33])
def test_plane_peak_kernel_on_constructed_sums(side, method, pairs):
    """Sides of 1, 9, 289 and 1 089 cells: below one wave, above one, above the work-group's 256 lanes, above 1 024.  Means,
    NaN borders from clips on every side, ties at the first, middle and last cell, zeros of both signs, a single valid cell,
    +-inf and the largest float32, a plane without a number: planes and records bit for bit, and the same bits as the
    host's restatement of the rule."""
    ctx = _lib.default_context()
    planes, recs = check_plane_peaks(ctx, side, pairs, method)
    h_planes, h_recs = check_plane_peaks(None, side, pairs, method)
    num = ~np.isnan(h_planes)
    assert (np.isnan(planes) == ~num).all() and planes[num].tobytes() == h_planes[num].tobytes()
    for f in ("templ_idx", "x", "y", "w", "h"):
        assert (recs[f] == h_recs[f]).all(), f
    some = ~np.isnan(h_recs["score"])
    assert recs["score"][some].tobytes() == h_recs["score"][some].tobytes() and np.isnan(recs["score"][~some]).all()
    with pytest.raises(_lib.MtmError, match="mtm_debug_plane_peaks: bad arguments"):
        ctx.debug_plane_peaks(np.zeros((1, 4, 4)), [(0, 0)], [1], [1], 1, 5)            # (an even side)


# ---- matchBlocksStack(offsets=) ------------------------------------------------------------------------------------------------
_KIND_METHODS = [(k, m) for k in ("u8", "rgb", "u16") for m in (1, 3, 5)] + [("u8", 0)]


def _at_cases(hw, shapes):
    """Blocks of every (h, w) of `shapes` at the four corners and one interior place, with offsets that push them over every
    border, along it, and inwards: (blocks, offsets)."""
    H, W = hw
    blocks, offs = [], []
    for h, w in shapes:
        for (x, y), (dx, dy) in (((0, 0), (-7, -3)), ((W - w, 0), (9, 2)), ((0, H - h), (3, 11)), ((W - w, H - h), (200, 300)),
                                 (((W - w) // 2, (H - h) // 2), (2, -1)), ((0, 0), (4, 5)), ((W - w, H - h), (-3, -6)),
                                 (((W - w) // 2, 0), (0, -2 ** 31)), ((0, (H - h) // 2), (2 ** 31 - 1, 0))):
            blocks.append((x, y, w, h))
            offs.append((dx, dy))
    return blocks, offs


@pytest.mark.parametrize("kind, method", _KIND_METHODS)
def test_stack_offsets_equal_the_loop_and_the_planes_restatement(kind, method):
    reference = "first" if method in (1, 5) else "previous"
    mode = M.FIRST if reference == "first" else M.PREVIOUS
    for hw, n_frames, shapes, margins in (((40, 52), 3, [(8, 8)], (0, 1, 8)), ((70, 90), 4, [(8, 8), (17, 65)], (1, 8))):
        frames = _movie(400 + method, n_frames, kind, hw)
        blocks, offs = _at_cases(hw, shapes)
        moved = B.moved_blocks(blocks, offs, hw)
        assert (moved == M.moved_brute(blocks, offs, hw)).all() and (moved[:, :2] != np.array(blocks)[:, :2]).any(axis=1).sum() >= 6
        for margin in margins:
            for refine in (False, True):
                got = _quiet(MTM.matchBlocksStack, frames, blocks, margin, method, reference=reference, refine=refine, offsets=offs)
                exp = [MTM.matchBlocks(frames[r], frames[s], blocks, margin, method, refine=refine, offsets=offs)
                       for r, s in M.S.pair_frames(n_frames, mode)]
                assert got[0].shape == (n_frames - 1, len(blocks), 2)
                _same(got, (np.stack([e[0] for e in exp]), np.stack([e[1] for e in exp])))
            planes = M.planes_at(MTM.computeScoreMap, frames, blocks, offs, margin, method, mode)
            for refine in (False, True):
                pos, sc, pl = _quiet(MTM.matchBlocksStack, frames, blocks, margin, method, reference=reference, refine=refine,
                                     ensemble=True, offsets=offs)
                _same((pl,), (planes,))
                _same((pos, sc), B.plane_peaks(planes, moved, method, refine))
            # the device's own peak records are plane_peaks' integer peaks
            _, recs = _lib.default_context().match_blocks_stack_at(frames, _lib.block_records(blocks),
                                                                   (moved[:, :2] - np.array(blocks)[:, :2]).astype(np.int32), margin,
                                                                   method, mode, planes=True)
            ipos, isc = B.plane_peaks(planes, moved, method)
            assert (np.stack((recs["x"], recs["y"]), axis=1) == ipos).all() and recs["score"].astype(np.float32).tobytes() == isc.tobytes()
            assert (recs["w"] == moved[:, 2]).all() and (recs["h"] == moved[:, 3]).all()
            if margin == 8:     # clipped on every side somewhere, and an interior block not at all
                nan = np.isnan(planes)
                assert nan[0, :, 0].all() and nan[0, 0].all() and nan[3, -1].all() and nan[3, :, -1].all() and not nan[4].any()
        # zero offsets are the call without them
        zero = np.zeros((len(blocks), 2), np.int64)
        for kw in ({}, {"refine": True}, {"ensemble": True}, {"ensemble": True, "refine": True}):
            _same(_quiet(MTM.matchBlocksStack, frames, blocks, 8, method, reference=reference, offsets=zero, **kw),
                  _quiet(MTM.matchBlocksStack, frames, blocks, 8, method, reference=reference, **kw))


# ---- matchBlocksStackMultipass -------------------------------------------------------------------------------------------------
def _multi(frames, passes, method=5, **kw):
    return _quiet(MTM.matchBlocksStackMultipass, frames, passes, method, **kw)


@pytest.mark.parametrize("refine", [False, True])
@pytest.mark.parametrize("reference", ["previous", "first"])
@pytest.mark.parametrize("passes", [PASSES_2, PASSES_3], ids=["two", "three"])
def test_multipass_per_pair_equals_the_loop_of_matchBlocksMultipass(passes, reference, refine):
    for kind, hw, n_frames, method in (("u8", (70, 90), 4, 5), ("rgb", (40, 52), 3, 3), ("u16", (40, 52), 3, 1), ("u8", (40, 52), 3, 0)):
        frames = _movie(500, n_frames, kind, hw, step=(3, -2))
        got = _multi(frames, passes, method, reference=reference, refine=refine)
        exp = M.loop_pairs(MTM.matchBlocksMultipass, frames, passes, method, reference, refine)
        assert len(got) == len(passes)
        for g, e in zip(got, exp):
            assert len(g) == 3 and g[1].shape == (n_frames - 1, len(g[0]), 2) and g[1].dtype == (np.float64 if refine else np.int64)
            _same(g, e)


@pytest.mark.parametrize("refine", [False, True])
@pytest.mark.parametrize("reference", ["previous", "first"])
@pytest.mark.parametrize("passes", [PASSES_2, PASSES_3], ids=["two", "three"])
def test_multipass_ensemble_equals_the_by_hand_loop(passes, reference, refine):
    for kind, hw, n_frames, method in (("u8", (70, 90), 4, 5), ("rgb", (40, 52), 3, 3), ("u16", (40, 52), 3, 1), ("u8", (40, 52), 3, 0)):
        frames = _movie(510, n_frames, kind, hw, step=(3, -2))
        got = _multi(frames, passes, method, reference=reference, refine=refine, ensemble=True)
        exp = M.loop_ensemble(MTM.matchBlocksStack, frames, passes, method, reference, refine)
        for g, e, (_, _, margin) in zip(got, exp, passes):
            assert len(g) == 4 and g[3].shape == (len(g[0]), 2 * margin + 1, 2 * margin + 1)
            _same(g, e)


def test_multipass_finds_a_shift_beyond_the_fine_margin():
    """A movie that moves by (5, 3) a frame under noise: the single-pass ensemble at the fine margin of 1 cannot hold the
    displacement in its planes, the ensemble multipass - a coarse pass at margin 6, then margin 1 - finds it."""
    rng = np.random.RandomState(520)
    H, W = 72, 96
    base = rng.randint(0, 256, size=(H, W)).astype(np.float64)
    frames = [np.clip(128 + 0.3 * (np.roll(base, (3 * f, 5 * f), axis=(0, 1)) - 128) + rng.normal(0, 15, size=(H, W)), 0, 255)
              .astype(np.uint8) for f in range(6)]
    passes = [(16, 16, 6), (16, 8, 1)]
    blocks = B.grid((H, W), 16, 8)
    inner = (blocks[:, 0] >= 16) & (blocks[:, 1] >= 16) & (blocks[:, 0] + 32 <= W) & (blocks[:, 1] + 32 <= H)
    single, _, _ = _quiet(MTM.matchBlocksStack, frames, blocks, 1, 5, ensemble=True)
    multi = _multi(frames, passes, ensemble=True)
    assert (multi[1][0] == blocks).all()
    found = lambda pos: (B.displacements(blocks, pos) == (5, 3)).all(axis=1)[inner].mean()      # noqa: E731
    assert inner.sum() >= 8 and found(single) == 0.0 and found(multi[1][1]) >= 0.9, (found(single), found(multi[1][1]))
    # ... and so does every pair's own multipass on this movie's first pairs, one call for all of them
    pairs = _multi(frames, passes)
    assert np.mean([found(p) for p in pairs[1][1]]) >= 0.9


def test_a_one_pair_stack_is_one_multipass_call():
    for kind in ("u8", "rgb", "u16"):
        frames = _movie(530, 2, kind, (40, 52), step=(3, -2))
        for refine in (False, True):
            got = _multi(np.stack(frames), PASSES_3, refine=refine)
            exp = MTM.matchBlocksMultipass(frames[0], frames[1], PASSES_3, 5, refine=refine)
            for g, e in zip(got, exp):
                _same(g, (e[0], e[1][None], e[2][None]))
            if not refine:      # one pair: the mean of one plane is the plane, its integer peak the pair's match (a refined
                #                 peak is fitted inside the plane, a pair's in the whole image's map: not the same at a border)
                for g, e in zip(_multi(frames, PASSES_3, ensemble=True), exp):
                    _same(g[:3], e)
        one = _multi(frames[:1], PASSES_2)
        assert [r[1].shape for r in one] == [(0, len(r[0]), 2) for r in one]
        with pytest.raises(ValueError, match="two frames at least"):
            _multi(frames[:1], PASSES_2, ensemble=True)


@pytest.mark.parametrize("reference", ["previous", "first"])
def test_frame_chunks_change_no_byte(reference):
    H, W = 40, 52
    for kind in ("u8", "u16"):
        frames = _movie(540, 5, kind, (H, W), step=(3, -2))
        blocks, offs = _at_cases((H, W), [(8, 8)])
        calls = [lambda: _multi(frames, PASSES_3, reference=reference, refine=True),
                 lambda: _multi(frames, PASSES_3, reference=reference, refine=True, ensemble=True),
                 lambda: _quiet(MTM.matchBlocksStack, frames, blocks, 3, 5, reference=reference, refine=True, offsets=offs),
                 lambda: _quiet(MTM.matchBlocksStack, frames, blocks, 3, 5, reference=reference, ensemble=True, offsets=offs)]
        whole = [c() for c in calls]
        # 2 frames per stack, 3, and a row bound below two frames (a stack never holds fewer than two)
        for max_rows in (2 * H, 3 * H, H + 12):
            with _Opt(_lib.OPT_BATCH_MAX_ROWS, max_rows):
                for c, w in zip(calls, whole):
                    got = c()
                    if isinstance(w, list):
                        for g, e in zip(got, w):
                            _same(g, e)
                    else:
                        _same(got, w)
        with _Opt(_lib.OPT_BATCH_MAX_ROWS, 2 * H):
            with _Opt(_lib.OPT_BOXES_MAX_FLOATS, 1500):     # several block chunks per pass as well (4 bytes a float)
                for g, e in zip(calls[0](), whole[0]):
                    _same(g, e)
    cells = sum(len(B.grid((H, W), b, s)) * (2 * m + 1) ** 2 for b, s, m in PASSES_3)
    with _Opt(_lib.OPT_BOXES_MAX_FLOATS, cells - 1):        # one float short: refused, by the Python layer and by the library
        with pytest.raises(ValueError, match="OPT_BOXES_MAX_FLOATS = %d" % (cells - 1)):
            _multi(frames, PASSES_3, ensemble=True)
        rec = _lib.block_pass_records([(b, b, s, s, m) for b, s, m in PASSES_3])
        with pytest.raises(_lib.MtmError, match="MTM_OPT_BOXES_MAX_FLOATS = %d" % (cells - 1)):
            _lib.default_context().match_blocks_stack_passes(frames, rec, [len(B.grid((H, W), b, s)) for b, s, _ in PASSES_3], 5,
                                                             M.PREVIOUS, planes=True)


def _keys(res):
    return [[(h[0], tuple(int(v) for v in h[1]), np.float32(h[2]).tobytes()) for h in r] for r in res]


def test_repeats_and_the_contexts_state():
    rng = np.random.RandomState(29)
    H, W = 70, 90
    frames = _movie(550, 4, "u8", (H, W), step=(3, -2))
    templs = [("t%d" % k, rng.randint(0, 256, size=(7 + k, 9)).astype(np.uint8)) for k in range(3)]
    templs[0] = ("t0", frames[1][20:27, 30:39].copy())
    regions = [((10, 10, 60, 50), [0, 1]), ((0, 0, W, H), [2])]
    blocks, offs = _at_cases((H, W), [(8, 8)])
    ctx = _lib.default_context()
    options = ctx.options()
    before = MTM.findMatchesInBoxes(templs, frames[1], regions, 5, N_object=1)
    runs = [lambda **kw: _multi(frames, PASSES_3, 3, refine=True, **kw), lambda **kw: _multi(frames, PASSES_2, 3, ensemble=True, **kw),
            lambda **kw: [_quiet(MTM.matchBlocksStack, frames, blocks, 4, 3, ensemble=True, offsets=offs, **kw)]]
    first = [r() for r in runs]
    assert _keys(before) == _keys(MTM.findMatchesInBoxes(templs, frames[1], regions, 5, N_object=1))
    assert ctx.options() == options
    for r, f in zip(runs, first):
        for g, e in zip(r(), f):
            _same(g, e)
    # a resident template set on a context of its own stays as it is
    own = _lib.Context()
    m = MTM.TemplateMatcher(templs, 5, N_object=1, score_threshold=0.2, context=own)
    boxes = [r[0] for r in regions]
    hits = m.match_boxes(frames[1], boxes)
    resident = m._uploaded_for
    assert resident is not None
    for r, f in zip(runs, first):
        for g, e in zip(r(context=own), f):
            _same(g, e)
    assert m._uploaded_for == resident and _keys(hits) == _keys(m.match_boxes(frames[1], boxes))
    own.close()
