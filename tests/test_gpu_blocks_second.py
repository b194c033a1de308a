"""The second correlation peak on the GPU.  blocks_second_kernel on constructed maps (mtm_debug_second_peaks with a context)
and MTM.matchBlocks(second=) / MTM.matchBlocksMultipass(second=) against the brute-force rule of tests/blocks_second_model.py
applied to MTM.computeScoreMap of every block over its search box: positions with ``==``, float32 score bits, NaN exactly
where the model has no second peak; positions, scores and flags equal the calls without ``second`` bit for bit."""
import warnings

import numpy as np
import pytest

import MTM
import blocks_second_model as S
from MTM import _lib
from MTM import blocks as B

pytestmark = pytest.mark.gpu

_H, _W = 96, 120
_SHIFT = (11, -7)
_KINDS = ("u8", "rgb", "u16")
_EDGE_SHAPES = ((15, 17), (16, 16), (33, 33))       # 255 and 256 cells (17 x 17, 289, is swept anyway): the 256-lane walk's edges


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


def _pair(seed, h, w, kind, shift=_SHIFT, noise=3):
    """A reference and an image: the reference moved by `shift` = (dx, dy) (wrapping around) with a little noise."""
    rng = np.random.RandomState(seed)
    top = 65536 if kind == "u16" else 256
    shape = (h, w, 3) if kind == "rgb" else (h, w)
    ref = rng.randint(0, top, size=shape).astype(np.uint16 if kind == "u16" else np.uint8)
    img = np.roll(ref, (shift[1], shift[0]), axis=(0, 1)).astype(np.int64) + rng.randint(-noise, noise + 1, size=shape)
    return ref, np.clip(img, 0, top - 1).astype(ref.dtype)


_PAIRS = {}


def _images(kind):
    """One pair per pixel kind for the whole module (never written to); a flat patch in the reference, one in the image."""
    if kind not in _PAIRS:
        ref, img = _pair(60 + _KINDS.index(kind), _H, _W, kind)
        ref[40:62, 28:62] = 77
        img[8:52, 66:118] = 50
        ref.setflags(write=False)
        img.setflags(write=False)
        _PAIRS[kind] = (ref, img)
    return _PAIRS[kind]


def _placed(H, W, shapes):
    """Every (w, h) of `shapes` at the four corners, the middles of the four edges and one interior place."""
    out = []
    for w, h in shapes:
        xs, ys = (0, (W - w) // 2, W - w), (0, (H - h) // 2, H - h)
        out += [(x, y, w, h) for y in ys for x in xs]
    return out


# 5 x 7, 16 x 16, 17 x 33 and 70 x 20 touching every border; two flat blocks; a block whose box (margin <= 8) is flat
_BLOCKS = _placed(_H, _W, [(5, 7), (16, 16), (17, 33), (70, 20)]) + [(30, 42, 20, 10), (36, 44, 16, 16), (86, 24, 12, 10)]
_FLAT_BLOCKS, _FLAT_BOX = (len(_BLOCKS) - 3, len(_BLOCKS) - 2), len(_BLOCKS) - 1
_MARGINS = (0, 1, 2, 3, 7, 8, 20)


def _offsets(n, seed):
    """Zeros, the true shift, offsets that push the box past each border, and small random ones, in turn; none for the block
    whose box is flat."""
    rng = np.random.RandomState(seed)
    fixed = [(0, 0), _SHIFT, (1000, 1000), (-1000, -1000), (1000, 0), (0, -1000), (-_W, 3), (4, _H), (10 ** 9, -10 ** 9)]
    off = np.array([fixed[k % (len(fixed) + 2)] if k % (len(fixed) + 2) < len(fixed) else tuple(rng.randint(-12, 13, 2))
                    for k in range(n)], dtype=np.int64)
    off[_FLAT_BOX] = 0
    return off


def _call(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("error")              # no warnings are emitted
        return fn(*a, **kw)


def _bytes(arrays):
    return [(a.dtype, a.shape, a.tobytes()) for a in arrays]


# ---- blocks_second_kernel on constructed maps ---------------------------------------------------------------------------
_EXPECTED = {}


def _constructed(r, mode_min):
    """The maps of one (r, mode_min) and the model's second peaks, computed once."""
    if (r, mode_min) not in _EXPECTED:
        maps = S.maps(r, mode_min, 100 * r + mode_min, extra=_EDGE_SHAPES)
        _EXPECTED[r, mode_min] = (maps, [S.second_peak(m, 1 if mode_min else 5, r)[0] for m in maps])
    return _EXPECTED[r, mode_min]


@pytest.mark.parametrize("mode_min", [0, 1])
@pytest.mark.parametrize("r", S.RADII)
def test_kernel_on_constructed_maps(r, mode_min):
    ctx = _lib.default_context()
    maps, exp = _constructed(r, mode_min)
    S.same_seconds(*ctx.debug_second_peaks(maps, mode_min, r), exp)
    host = _lib.debug_second_peaks(maps, mode_min, r)
    assert _bytes(ctx.debug_second_peaks(maps, mode_min, r)) == _bytes(host)
    # a first peak that is given: the host path (pinned to the model on the CPU) says what the kernel says
    firsts = [(7 * k) % m.size for k, m in enumerate(maps)]
    assert _bytes(ctx.debug_second_peaks(maps, mode_min, r, firsts=firsts)) == \
        _bytes(_lib.debug_second_peaks(maps, mode_min, r, firsts=firsts))


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_kernel_over_n_maps(n):
    ctx = _lib.default_context()
    maps, exp = _constructed(2, 0)
    pick = [(5 * k + 3) % len(maps) for k in range(n)]
    S.same_seconds(*ctx.debug_second_peaks([maps[i] for i in pick], 0, 2), [exp[i] for i in pick])


def test_kernel_reads_only_its_map():
    # maps back to back, every neighbour full of values that would win: a read past a map's end would pick one up
    ctx = _lib.default_context()
    maps, exp = _constructed(1, 0)
    inter = [m for smap in maps for m in (smap, np.full((3, 7), 9.0, np.float32))]
    pos, sc = ctx.debug_second_peaks(inter, 0, 1)
    S.same_seconds(pos[0::2], sc[0::2], exp)


def test_bad_arguments_on_a_context():
    ctx = _lib.default_context()
    ref, img = _images("u8")
    with pytest.raises(RuntimeError, match="mtm_debug_second_peaks: bad arguments"):
        ctx.debug_second_peaks([np.zeros((3, 3), np.float32)], 0, -1)
    with pytest.raises(RuntimeError, match="mtm_match_blocks_second: bad arguments"):
        ctx.match_blocks_at(ref, img, _lib.block_records(np.array(_BLOCKS[:2])), None, 2, 5, second=-1)
    rec = np.array([(16, 16, 16, 16, 2)], dtype=_lib.BLOCK_PASS_DTYPE)
    with pytest.raises(RuntimeError, match="mtm_match_blocks_passes_second: bad arguments"):
        ctx.match_blocks_passes(ref, img, rec, [len(B.grid(img.shape, 16))], 5, second=-1)


# ---- the calls against the model -----------------------------------------------------------------------------------------
def _check_call(ref, img, blocks, margin, method, offsets, radii=(0, 2)):
    """matchBlocks(second=r) for every r: the call without second bit for bit, the first peak that of the block's map, the
    second peak the model's."""
    plain = _call(MTM.matchBlocks, ref, img, blocks, margin, method, offsets=offsets)
    exp = {}
    for r in radii:
        got = _call(MTM.matchBlocks, ref, img, blocks, margin, method, offsets=offsets, second=r)
        assert len(got) == 4 and _bytes(got[:2]) == _bytes(plain)
        if not exp:     # (the maps once for every radius)
            smaps = [S.block_map(ref, img, b, (0, 0) if offsets is None else offsets[k], margin, method, MTM.computeScoreMap)
                     for k, b in enumerate(blocks)]
        exp[r] = []
        for k, (smap, (x0, y0)) in enumerate(smaps):
            ((sx, sy), s), (fx, fy) = S.second_peak(smap, method, r)
            assert (fx + x0, fy + y0) == tuple(got[0][k]), (k, blocks[k])           # the first peak is the call's record
            assert np.float32(smap[fy, fx] + np.float32(0.0)).tobytes() == got[1][k].tobytes()
            exp[r].append(((sx + x0, sy + y0) if sx >= 0 else (-1, -1), s))
        S.same_seconds(got[2], got[3], exp[r])
    return plain, exp, smaps


@pytest.mark.parametrize("method", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("kind", _KINDS)
def test_calls_equal_the_model(kind, method):
    ref, img = _images(kind)
    for margin in _MARGINS:
        off = _offsets(len(_BLOCKS), 7 * margin + method)
        plain, exp, smaps = _check_call(ref, img, _BLOCKS, margin, method, off)
        if margin == 0:         # 1 x 1 maps: no second peak
            assert all(np.isnan(s) for _, s in exp[0] + exp[2])
        if margin == 2:         # 5 x 5 maps at most: the ones inside the exclusion of their peak have none, others have one
            none = [np.isnan(s) for _, s in exp[2]]
            assert any(none) and not all(none) and not any(np.isnan(s) for _, s in exp[0])
        if margin in (3, 8):    # all-equal maps (a flat block under the centred methods, a flat box): the tie rule
            flat = [k for k, (m, _) in enumerate(smaps) if m.size > 1 and (m == m.flat[0]).all()]
            assert _FLAT_BOX in flat and (method < 4 or set(_FLAT_BLOCKS) <= set(flat))
            for k in flat:
                x0, y0 = B.search_box_at(_BLOCKS[k], off[k], margin, img.shape)[:2]
                assert tuple(plain[0][k]) == (x0, y0) and exp[0][k][0] == (x0 + 1, y0) and exp[2][k][0] == (x0 + 3, y0)
    # without offsets: mtm_match_blocks' boxes, the zero-offset call
    zero = np.zeros((len(_BLOCKS), 2), np.int64)
    for refine in (False, True):
        a = _call(MTM.matchBlocks, ref, img, _BLOCKS, 7, method, second=True, refine=refine)
        assert _bytes(a) == _bytes(_call(MTM.matchBlocks, ref, img, _BLOCKS, 7, method, second=2, offsets=zero, refine=refine))
        assert _bytes(a[:2]) == _bytes(_call(MTM.matchBlocks, ref, img, _BLOCKS, 7, method, refine=refine))
        assert a[2].dtype == np.int64           # (refine moves the first positions only)
    S.same_seconds(a[2], a[3], S.expected_seconds(ref, img, _BLOCKS, None, 7, method, 2, MTM.computeScoreMap))


def test_a_periodic_image():
    rng = np.random.RandomState(9)
    cell = rng.randint(0, 256, size=(8, 8)).astype(np.uint8)
    ref = np.tile(cell, (9, 12))                # 72 x 96, period 8 both ways
    blocks = [(40, 32, 12, 12), (0, 0, 16, 9), (80, 60, 16, 12)]
    for method in (1, 5):
        plain, exp, _ = _check_call(ref, ref, blocks, 12, method, None, radii=(0, 2, 8))
        # every period repeats the match exactly: the second peak scores what the first does, one period away at most
        (p2, s2) = exp[2][0]
        assert s2.tobytes() == plain[1][0].tobytes() and max(abs(p2[0] - plain[0][0][0]), abs(p2[1] - plain[0][0][1])) == 8
        ratio = B.peak_ratio(plain[1], np.array([s for _, s in exp[2]], np.float32), method)
        assert ratio[0] == 1.0 or (method == 1 and ratio[0] == np.inf)      # (sqdiff 0 / 0: no signal either way)


# ---- matchBlocksMultipass ------------------------------------------------------------------------------------------------
_PASS_SETS = ([(32, 16, 8), (16, 8, 2)], [(24, 12, 6), (12, 6, 3), (8, 4, 0)])


@pytest.mark.parametrize("kind", _KINDS)
@pytest.mark.parametrize("passes", _PASS_SETS, ids=["two", "three"])
def test_multipass_equals_the_by_hand_loop(passes, kind):
    ref, img = _images(kind)
    for method, validate, refine in ((5, None, False), (1, (2.0, 0.5), True), (2, True, False), (4, None, True)):
        got = _call(MTM.matchBlocksMultipass, ref, img, passes, method, refine=refine, validate=validate, second=2)
        plain = _call(MTM.matchBlocksMultipass, ref, img, passes, method, refine=refine, validate=validate)
        steer = None
        for p, (g, q) in enumerate(zip(got, plain)):
            assert len(g) == len(q) + 2 and _bytes(g[:-2]) == _bytes(q)         # positions, scores and flags: untouched
            block, step, margin = passes[p]
            off = None if p == 0 else B.predict_offsets(img.shape, passes[p - 1][:2], steer, passes[p][:2])
            pos, sc, pos2, sc2 = _call(MTM.matchBlocks, ref, img, g[0], margin, method, offsets=off, second=2)
            assert _bytes(g[-2:]) == _bytes((pos2, sc2))
            steer = pos
            if validate:
                _, rep = B.validate(B.grid_shape(img.shape, block, step), B.displacements(g[0], pos), 2.0, 0.5)
                steer = g[0][:, :2] + rep


# ---- chunks, sub-ranges, the plane buffer ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "u16"])
def test_one_block_per_chunk_and_per_plane_sub_range(kind):
    ref, img = _images(kind)
    floats = 200        # 800 bytes of templates per chunk: at most one 24 x 24 uint8 block; planes of 13 x 13 = 169 floats:
    passes = [(24, 12, 6), (12, 6, 3), (8, 4, 7)]   # one per sub-range, 7 x 7: four, 15 x 15 = 225: one, past the budget
    rec = [(b, b, s, s, m) for b, s, m in passes]
    counts, _, chunk_of = _lib.debug_plan_blocks_passes(img.shape, 1, ref.dtype, rec, 4 * floats)
    assert chunk_of[:counts[0]].max() == counts[0] - 1 and chunk_of[-counts[2]:].max() >= 2
    off = _offsets(len(_BLOCKS), 5)
    for refine in (False, True):
        whole = _call(MTM.matchBlocksMultipass, ref, img, passes, 5, refine=refine, second=2, validate=True)
        at = _call(MTM.matchBlocks, ref, img, _BLOCKS, 8, 1, offsets=off, refine=refine, second=1)
        with _Opt(_lib.OPT_BOXES_MAX_FLOATS, floats):
            again = _call(MTM.matchBlocksMultipass, ref, img, passes, 5, refine=refine, second=2, validate=True)
            assert [_bytes(t) for t in again] == [_bytes(t) for t in whole]
            assert _bytes(_call(MTM.matchBlocks, ref, img, _BLOCKS, 8, 1, offsets=off, refine=refine, second=1)) == _bytes(at)
        with _Opt(_lib.OPT_BOXES_MAX_FLOATS, 1):        # a budget below every block: one block at a time throughout
            assert _bytes(_call(MTM.matchBlocks, ref, img, _BLOCKS, 8, 1, offsets=off, refine=refine, second=1)) == _bytes(at)
    assert _lib.default_context().get_option(_lib.OPT_BOXES_MAX_FLOATS) not in (floats, 1)


def test_a_poisoned_plane_buffer_changes_nothing():
    ref, img = _images("u8")
    ctx = _lib.Context()
    off = _offsets(len(_BLOCKS), 3)
    first = _call(MTM.matchBlocks, ref, img, _BLOCKS, 20, 5, offsets=off, second=2, context=ctx)
    assert _bytes(first) == _bytes(_call(MTM.matchBlocks, ref, img, _BLOCKS, 20, 5, offsets=off, second=2))
    for pattern in (0x7F, 0xFF, 0x00):          # a huge number in every cell, NaN, zero
        ctx.debug_poison(pattern, _lib.POISON_ARENAS)
        assert _bytes(_call(MTM.matchBlocks, ref, img, _BLOCKS, 7, 5, offsets=off, second=2, context=ctx)) == \
            _bytes(_call(MTM.matchBlocks, ref, img, _BLOCKS, 7, 5, offsets=off, second=2))
        assert _bytes(_call(MTM.matchBlocks, ref, img, _BLOCKS, 20, 5, offsets=off, second=2, context=ctx)) == _bytes(first)
    assert _bytes(_call(MTM.matchBlocks, ref, img, _BLOCKS, 20, 5, offsets=off, second=2, context=ctx)) == _bytes(first)
    ctx.close()


# ---- the context's state -------------------------------------------------------------------------------------------------
def _keys(res):
    return [[(h[0], tuple(int(v) for v in h[1]), np.float32(h[2]).tobytes()) for h in r] for r in res]


def test_context_state_is_left_alone():
    ref, img = _images("u8")
    rng = np.random.RandomState(29)
    templs = [("t%d" % k, rng.randint(0, 256, size=(7 + k, 9)).astype(np.uint8)) for k in range(3)]
    templs[0] = ("t0", img[20:27, 30:39].copy())
    regions = [((10, 10, 60, 50), [0, 1]), ((0, 0, 100, 80), [2])]
    blocks = B.grid(ref.shape, 16)
    before = MTM.findMatchesInBoxes(templs, img, regions, 5, N_object=1)
    got = _call(MTM.matchBlocks, ref, img, blocks, 4, 3, second=True)
    after = MTM.findMatchesInBoxes(templs, img, regions, 5, N_object=1)
    assert _keys(before) == _keys(after)
    for method in (5, 1, 4, 0):     # different methods back to back: the gathered constants depend on the method
        _call(MTM.matchBlocks, ref, img, blocks, 4, method, second=True)
    assert _bytes(_call(MTM.matchBlocks, ref, img, blocks, 4, 3, second=True)) == _bytes(got)

    ctx = _lib.Context()
    m = MTM.TemplateMatcher(templs, 5, N_object=1, score_threshold=0.2, context=ctx)
    boxes = [r[0] for r in regions]
    first = m.match_boxes(img, boxes)
    resident = m._uploaded_for
    assert resident is not None
    assert _bytes(_call(MTM.matchBlocks, ref, img, blocks, 4, 3, second=True, context=ctx)) == _bytes(got)
    on_ctx = _call(MTM.matchBlocksMultipass, ref, img, _PASS_SETS[0], 3, refine=True, second=1, validate=True, context=ctx)
    assert [_bytes(t) for t in on_ctx] == \
        [_bytes(t) for t in _call(MTM.matchBlocksMultipass, ref, img, _PASS_SETS[0], 3, refine=True, second=1, validate=True)]
    assert m._uploaded_for == resident
    again = m.match_boxes(img, boxes)
    assert _keys(first) == _keys(again) and m._uploaded_for == resident
    ctx.close()


# ---- what it is for ---------------------------------------------------------------------------------------------------------
def test_a_pasted_copy_is_the_second_peak_and_lowers_the_ratio():
    rng = np.random.RandomState(17)
    ref = rng.randint(0, 256, size=(72, 96)).astype(np.uint8)
    img = np.roll(ref, (-2, 3), axis=(0, 1)).astype(np.int64) + rng.randint(-3, 4, size=ref.shape)
    x, y, w, h = 40, 30, 12, 12
    copy = ref[y:y + h, x:x + w].astype(np.int64) + rng.randint(-40, 41, size=(h, w))
    img[y + 9:y + 9 + h, x - 8:x - 8 + w] = copy                # a noisy copy of the block at displacement (-8, 9)
    img = np.clip(img, 0, 255).astype(np.uint8)
    blocks = np.array([(x, y, w, h), (70, 44, 12, 12)])         # the second block's box holds no pixel of the copy
    pos, sc, pos2, sc2 = _call(MTM.matchBlocks, ref, img, blocks, 12, 5, second=2)
    d1, d2 = B.displacements(blocks, pos), B.displacements(blocks, pos2)
    assert tuple(d1[0]) == (3, -2) and tuple(d2[0]) == (-8, 9) and tuple(d1[1]) == (3, -2)
    ratio = B.peak_ratio(sc, sc2, 5)
    print("scores %s, second %s, ratios %s" % (sc, sc2, ratio))
    assert 1.0 <= ratio[0] < ratio[1]
