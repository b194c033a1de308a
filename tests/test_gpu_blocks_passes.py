"""MTM.matchBlocks(offsets=) and MTM.matchBlocksMultipass on the GPU.  matchBlocks(offsets=) equals the loop a user writes
through findMatchesInBoxes with every block's box from search_box_at (and refineHits) in positions (``==``) and float32 score
bits; matchBlocksMultipass equals, pass by pass, the loop of matchBlocks(offsets=) and predict_offsets it documents."""
import warnings

import numpy as np
import pytest

import MTM
from MTM import _lib
from MTM import blocks as B

pytestmark = pytest.mark.gpu

_H, _W = 96, 120
_SHIFT = (11, -7)           # (dx, dy) of the image against the reference: out of reach of a zero-offset box of margin <= 8
_KINDS = ("u8", "rgb", "u16")


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
    """One pair per pixel kind for the whole module (never written to); a flat patch in the reference."""
    if kind not in _PAIRS:
        ref, img = _pair(40 + _KINDS.index(kind), _H, _W, kind)
        ref[40:62, 28:62] = 77
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


# 5 x 7, 16 x 16, 17 x 33 and 70 x 20 (wider than one 16 x 64 template chunk), touching every border; two flat blocks
_BLOCKS = _placed(_H, _W, [(5, 7), (16, 16), (17, 33), (70, 20)]) + [(30, 42, 20, 10), (36, 44, 16, 16)]


def _offsets(n, seed):
    """Zeros, the true shift, +-1000, offsets that push the box past each border, and small random ones, in turn."""
    rng = np.random.RandomState(seed)
    fixed = [(0, 0), _SHIFT, (1000, 1000), (-1000, -1000), (1000, 0), (0, -1000), (-_W, 3), (4, _H), (_W - 1, -_H + 1),
             (-13, 9), (10 ** 9, -10 ** 9)]
    return np.array([fixed[k % (len(fixed) + 2)] if k % (len(fixed) + 2) < len(fixed) else tuple(rng.randint(-12, 13, 2))
                     for k in range(n)], dtype=np.int64)


def _loop(reference, image, blocks, offsets, margin, method, refine):
    """The loop through findMatchesInBoxes (and refineHits): (positions, scores, refined positions or None)."""
    blocks = [tuple(int(v) for v in b) for b in blocks]
    templs = [("b%d" % k, np.ascontiguousarray(reference[y:y + h, x:x + w])) for k, (x, y, w, h) in enumerate(blocks)]
    regions = [(B.search_box_at(b, offsets[k], margin, image.shape), [k]) for k, b in enumerate(blocks)]
    res = MTM.findMatchesInBoxes(templs, image, regions, method, N_object=1)
    assert all(len(r) == 1 for r in res)
    hits = [r[0] for r in res]
    pos = np.array([[h[1][0], h[1][1]] for h in hits], dtype=np.int64).reshape(-1, 2)
    sc = np.array([h[2] for h in hits], dtype=np.float32)
    fine = None
    if refine:
        out = MTM.refineHits(templs, image, hits, method)
        fine = np.array([[h[1][0], h[1][1]] for h in out], dtype=np.float64).reshape(-1, 2)
    return pos, sc, fine


def _call(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("error")              # no warnings are emitted
        return fn(*a, **kw)


def _same(got, exp_pos, exp_sc):
    pos, sc = got
    assert pos.dtype == exp_pos.dtype and pos.shape == exp_pos.shape
    bad = np.flatnonzero((pos != exp_pos).any(axis=1) | (sc.view(np.uint32) != exp_sc.view(np.uint32)))
    assert sc.dtype == np.float32 and len(bad) == 0, (bad[:5], pos[bad[:5]], exp_pos[bad[:5]], sc[bad[:5]], exp_sc[bad[:5]])


# ---- matchBlocks(offsets=) against the findMatchesInBoxes loop -----------------------------------------------------------
# margins: a 1 x 1 map; exactly one tile (3 and 15 per side); the 17-wide map's second, partly filled tile; several tiles
# with clipped boxes whose trailing tiles of the fixed table leave early
@pytest.mark.parametrize("method", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("kind", _KINDS)
def test_offsets_equal_the_boxes_loop(kind, method):
    ref, img = _images(kind)
    for margin in (0, 1, 7, 8, 20):
        off = _offsets(len(_BLOCKS), 7 * margin + method)
        exp_pos, exp_sc, fine = _loop(ref, img, _BLOCKS, off, margin, method, True)
        _same(_call(MTM.matchBlocks, ref, img, _BLOCKS, margin, method, offsets=off), exp_pos, exp_sc)
        _same(_call(MTM.matchBlocks, ref, img, _BLOCKS, margin, method, offsets=off, refine=True), fine, exp_sc)
        if method == 5:         # a flat block scores 1.0 everywhere: the first output of ITS box
            k = len(_BLOCKS) - 2
            assert exp_sc[k] == np.float32(1.0)
            assert tuple(exp_pos[k]) == B.search_box_at(_BLOCKS[k], off[k], margin, img.shape)[:2]


@pytest.mark.parametrize("kind", _KINDS)
def test_zero_offsets_are_the_call_without_and_true_offsets_are_not(kind):
    ref, img = _images(kind)
    n = len(_BLOCKS)
    for margin in (0, 1, 7, 8, 20):
        for method in (1, 5):
            plain = _call(MTM.matchBlocks, ref, img, _BLOCKS, margin, method)
            _same(_call(MTM.matchBlocks, ref, img, _BLOCKS, margin, method, offsets=np.zeros((n, 2), np.int32)), *plain)
            for refine in (False, True):
                zero = _call(MTM.matchBlocks, ref, img, _BLOCKS, margin, method, offsets=[(0, 0)] * n, refine=refine)
                _same(zero, *_call(MTM.matchBlocks, ref, img, _BLOCKS, margin, method, refine=refine))
    # a kernel that ignored its offsets would return the zero-offset hits: with the true shift out of a margin-7 box's reach
    # the interior blocks' hits differ, and the offset ones sit at the shift (blocks that hold a part of the reference's flat
    # patch, which the image does not have, are left out)
    inner = np.array([k for k, (x, y, w, h) in enumerate(_BLOCKS[:-2])
                      if x + _SHIFT[0] >= 0 and y + _SHIFT[1] >= 0 and x + w + _SHIFT[0] <= _W and y + h + _SHIFT[1] <= _H
                      and (x >= 62 or x + w <= 28 or y >= 62 or y + h <= 40)])
    assert len(inner) >= 6
    blocks = np.array(_BLOCKS)
    plain, _ = _call(MTM.matchBlocks, ref, img, _BLOCKS, 7, 5)
    moved, _ = _call(MTM.matchBlocks, ref, img, _BLOCKS, 7, 5, offsets=[_SHIFT] * n)
    assert (B.displacements(blocks, moved)[inner] == _SHIFT).all()
    assert (B.displacements(blocks, plain)[inner] != _SHIFT).any(axis=1).all()


# ---- matchBlocksMultipass against the by-hand loop ------------------------------------------------------------------------
def _by_hand(ref, img, passes, method, refine):
    out, off, steer = [], None, None
    for p, (block, step, margin) in enumerate(passes):
        b = B.grid(img.shape, block, step)
        if p:
            off = B.predict_offsets(img.shape, passes[p - 1][:2], steer, passes[p][:2])
        steer, _ = MTM.matchBlocks(ref, img, b, margin, method, offsets=off)
        pos, sc = MTM.matchBlocks(ref, img, b, margin, method, offsets=off, refine=refine)
        out.append((b, pos, sc))
    return out


def _same_passes(got, exp):
    assert len(got) == len(exp)
    for (gb, gp, gs), (eb, ep, es) in zip(got, exp):        # every pass, the non-final ones included
        assert gb.dtype == eb.dtype and (gb == eb).all()
        _same((gp, gs), ep, es)


_PASS_SETS = ([(32, 16, 8), (16, 8, 2)], [(24, 12, 6), (12, 6, 3), (8, 4, 0)], [((20, 12), (17, 19), 6)])


@pytest.mark.parametrize("method", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("kind", _KINDS)
@pytest.mark.parametrize("passes", _PASS_SETS, ids=["two", "three", "single"])
def test_multipass_equals_the_by_hand_loop(passes, kind, method):
    ref, img = _images(kind)
    for refine in (False, True):
        got = _call(MTM.matchBlocksMultipass, ref, img, passes, method, refine=refine)
        _same_passes(got, _by_hand(ref, img, passes, method, refine))
        if len(passes) == 1:        # a single pass is matchBlocks
            (block, step, margin), = passes
            _same(got[0][1:], *_call(MTM.matchBlocks, ref, img, B.grid(img.shape, block, step), margin, method, refine=refine))


@pytest.mark.parametrize("kind", ["u8", "u16"])
def test_multipass_in_several_chunks_per_pass(kind):
    ref, img = _images(kind)
    passes = _PASS_SETS[1]
    floats = 200        # 800 bytes of templates per chunk: at most one 24 x 24, five 12 x 12 and twelve 8 x 8 uint8 blocks
    rec = [(b, b, s, s, m) for b, s, m in passes]
    counts, _, chunk_of = _lib.debug_plan_blocks_passes(img.shape, 1, ref.dtype, rec, 4 * floats)
    at = 0
    for c in counts:
        assert chunk_of[at:at + c].max() >= 2
        at += c
    for refine in (False, True):
        whole = _call(MTM.matchBlocksMultipass, ref, img, passes, 5, refine=refine)
        with _Opt(_lib.OPT_BOXES_MAX_FLOATS, floats):
            _same_passes(_call(MTM.matchBlocksMultipass, ref, img, passes, 5, refine=refine), whole)
    assert _lib.default_context().get_option(_lib.OPT_BOXES_MAX_FLOATS) != floats


def test_a_shift_beyond_the_fine_margin_is_found_coarse_to_fine():
    H, W = 160, 192
    rng = np.random.RandomState(5)
    ref = rng.randint(0, 256, size=(H, W)).astype(np.uint8)
    img = np.roll(ref, (_SHIFT[1], _SHIFT[0]), axis=(0, 1))
    fine = B.grid(ref.shape, 16, 16)
    # interior: the nearest 32 x 32 block is not on the border, so its own shifted copy lies inside the image
    inner = (fine[:, 0] >= 32) & (fine[:, 1] >= 32) & (fine[:, 0] + 16 <= W - 32) & (fine[:, 1] + 16 <= H - 32)
    assert inner.sum() == 8 * 6
    alone, _ = _call(MTM.matchBlocks, ref, img, fine, 4, 5)
    assert (B.displacements(fine, alone)[inner] != _SHIFT).any(axis=1).all()        # margin 4 alone misses it
    passes = [(32, 32, 12), (16, 16, 4)]
    got = _call(MTM.matchBlocksMultipass, ref, img, passes, 5)
    _same_passes(got, _by_hand(ref, img, passes, 5, False))
    blocks, pos, sc = got[1]
    assert (blocks == fine).all()
    assert (B.displacements(blocks, pos)[inner] == _SHIFT).all() and (sc[inner] == np.float32(1.0)).all()


# ---- the context's state -------------------------------------------------------------------------------------------------
def _keys(res):
    return [[(h[0], tuple(int(v) for v in h[1]), np.float32(h[2]).tobytes()) for h in r] for r in res]


def test_resident_templates_survive_the_new_calls():
    ref, img = _images("u8")
    rng = np.random.RandomState(29)
    templs = [("t%d" % k, rng.randint(0, 256, size=(7 + k, 9)).astype(np.uint8)) for k in range(3)]
    templs[0] = ("t0", img[20:27, 30:39].copy())
    boxes = [(10, 10, 60, 50), (0, 0, 100, 80)]
    ctx = _lib.Context()
    m = MTM.TemplateMatcher(templs, 5, N_object=1, score_threshold=0.2, context=ctx)
    first = m.match_boxes(img, boxes)
    resident = m._uploaded_for
    assert resident is not None
    blocks = B.grid(ref.shape, 16)
    off = np.tile(_SHIFT, (len(blocks), 1))
    on_ctx = _call(MTM.matchBlocks, ref, img, blocks, 4, 1, offsets=off, context=ctx)
    _same(on_ctx, *_call(MTM.matchBlocks, ref, img, blocks, 4, 1, offsets=off))
    B.predict_offsets(ref.shape, (16, None), on_ctx[0], (8, None))
    _same_passes(_call(MTM.matchBlocksMultipass, ref, img, _PASS_SETS[0], 3, refine=True, context=ctx),
                 _call(MTM.matchBlocksMultipass, ref, img, _PASS_SETS[0], 3, refine=True))
    assert m._uploaded_for == resident
    again = m.match_boxes(img, boxes)
    assert _keys(first) == _keys(again) and m._uploaded_for == resident
    ctx.close()
