"""MTM.matchBlocks(mask=) on the GPU: every case equals the loop a user writes today - findMatches with the
block and its mask cut out on the host as a masked template and the block's search box as searchBox, N_object=1, then
refineHits - in positions (``==``) and float32 score bits, and equals the model on the CPU oracle
(tests/blocks_mask_model.py), so that the loop and the new call cannot be wrong together.  Images of the loop comparisons
hold pixels in 1..255: no output is NaN and the loop itself is well defined; the none rule is checked against the model."""
import warnings

import numpy as np
import pytest

import MTM
import blocks_mask_model as MM
from MTM import _lib
from MTM import blocks as B

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


def _pair(rng, h, w, rgb=False, shift=(2, -1), noise=3):
    """A reference and an image with pixels in 1..255: the reference moved by `shift` = (dx, dy) with a little noise."""
    shape = (h, w, 3) if rgb else (h, w)
    ref = rng.randint(1, 256, size=shape).astype(np.uint8)
    img = np.roll(ref, (shift[1], shift[0]), axis=(0, 1)).astype(np.int64) + rng.randint(-noise, noise + 1, size=shape)
    return ref, np.clip(img, 1, 255).astype(np.uint8)


def _placed(H, W, shapes):
    """Every (h, w) of `shapes` at the four corners, the middles of the four edges and one interior place."""
    out = []
    for h, w in shapes:
        xs, ys = (0, (W - w) // 2, W - w), (0, (H - h) // 2, H - h)
        out += [(x, y, w, h) for y in ys for x in xs]
    return out


def _call(reference, image, blocks, margin, method, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("error")              # no warnings are emitted
        return MTM.matchBlocks(reference, image, blocks, margin, method, **kw)


def _loop(reference, image, mask, blocks, margin, method, offsets=None, refine=False):
    """The loop through findMatches(searchBox=) with masked tuples (and refineHits): (positions, scores, refined or None)."""
    pos, sc, fine = [], [], []
    for k, b in enumerate(blocks):
        tup = MM.block_tuple(reference, mask, b)
        box = MM.box_of(b, None if offsets is None else offsets[k], margin, image.shape)
        hit, = MTM.findMatches([tup], image, method, N_object=1, searchBox=box)
        pos.append(hit[1][:2])
        sc.append(hit[2])
        if refine:
            out, = MTM.refineHits([tup], image, [hit], method)
            fine.append(out[1][:2])
    return (np.array(pos, dtype=np.int64).reshape(-1, 2), np.array(sc, dtype=np.float32),
            np.array(fine, dtype=np.float64).reshape(-1, 2) if refine else None)


def _check(reference, image, mask, blocks, margin, method, refine=False, **kw):
    """matchBlocks(mask=) against the loop and against the model; returns the call's result."""
    blocks = [tuple(int(v) for v in b) for b in blocks]
    got = _call(reference, image, blocks, margin, method, mask=mask, **kw)
    assert got[0].dtype == np.int64
    l_pos, l_sc, fine = _loop(reference, image, mask, blocks, margin, method, kw.get("offsets"), refine)
    MM.same(got[0], got[1], l_pos, l_sc)
    m_pos, m_sc = MM.match_blocks(reference, image, mask, blocks, margin, method, offsets=kw.get("offsets"))
    MM.same(got[0], got[1], m_pos, m_sc)
    if refine:
        fpos, fsc = _call(reference, image, blocks, margin, method, mask=mask, refine=True, **kw)[:2]
        assert fpos.dtype == np.float64
        MM.same(fpos, fsc, fine, l_sc)
    return got


def _keep_one(mask, blocks):
    """Every block keeps at least its first pixel (the loop comparisons need a score that is a number)."""
    for x, y, w, h in blocks:
        mask[y, x] = True
    return mask


# ---- chunk and quad edges: the 16 x 64 template chunk's and the 4-byte quad's edges, maps of 1, 3, 17 and 33 per side -------
_HS, _WS = (1, 15, 16, 17, 33), (1, 3, 4, 5, 63, 64, 65, 130)


@pytest.mark.parametrize("method", [0, 3])
@pytest.mark.parametrize("margin", [0, 1, 8, 16])
def test_chunk_and_quad_edges_uint8(margin, method):
    rng = np.random.RandomState(100 + margin)
    ref, img = _pair(rng, 200, 240)
    blocks = _placed(200, 240, [(h, w) for h in _HS for w in _WS])
    mask = _keep_one(rng.rand(200, 240) > 0.5, blocks)
    _check(ref, img, mask, blocks, margin, method)


@pytest.mark.parametrize("method", [0, 3])
@pytest.mark.parametrize("margin", [0, 1, 8, 16])
def test_chunk_and_quad_edges_rgb(margin, method):
    rng = np.random.RandomState(200 + margin)
    ref, img = _pair(rng, 120, 150, rgb=True)
    blocks = _placed(120, 150, [(h, w) for h in _HS for w in _WS])
    mask = _keep_one(rng.rand(120, 150) > 0.5, blocks)
    _check(ref, img, mask.astype(np.uint8) * 3, blocks, margin, method, refine=(margin == 8))


# ---- mask shapes ---------------------------------------------------------------------------------------------------------------
_SHAPE_BLOCKS = [(3, 2, 130, 17), (140, 1, 65, 33), (10, 30, 64, 16), (90, 32, 5, 17), (100, 60, 63, 15), (2, 76, 130, 33),
                 (180, 50, 1, 17), (150, 90, 33, 20)]


def _shape_mask(kind, rng, H, W):
    if kind == "all":
        return np.ones((H, W), bool)
    if kind == "random":
        return _keep_one(rng.rand(H, W) > 0.5, _SHAPE_BLOCKS)
    if kind == "disc":
        yy, xx = np.mgrid[0:H, 0:W]
        return _keep_one((yy - 45) ** 2 + (xx - 100) ** 2 <= 60 ** 2, _SHAPE_BLOCKS)
    mask = np.zeros((H, W), bool)
    for x, y, w, h in _SHAPE_BLOCKS:
        if kind == "one_pixel":
            mask[y + h // 2, x + (2 * w) // 3] = True
        elif kind == "last_column":
            mask[y:y + h, x + w - 1] = True
        elif kind == "third_chunk":                 # columns 128-129 of a 130-wide block; else the last two columns
            mask[y:y + h, x + max(0, w - 2):x + w] = True
        elif kind == "row_16":                      # row 16 of a block at least 17 high; else the last row
            mask[y + min(16, h - 1), x:x + w] = True
    return mask


@pytest.mark.parametrize("rgb", [False, True], ids=["u8", "rgb"])
@pytest.mark.parametrize("kind", ["random", "disc", "one_pixel", "last_column", "third_chunk", "row_16", "all"])
def test_mask_shapes(kind, rgb):
    rng = np.random.RandomState(300)
    ref, img = _pair(rng, 120, 240, rgb=rgb)
    mask = _shape_mask(kind, rng, 120, 240)
    assert (B.mask_fraction(mask, _SHAPE_BLOCKS) > 0).all()
    for method in (0, 3):
        _check(ref, img, mask, _SHAPE_BLOCKS, 8, method, refine=True)


def test_largest_sums():
    """An all-255 33 x 130 block with an all-set mask on an all-255 region."""
    rng = np.random.RandomState(7)
    for rgb in (False, True):
        ref, img = _pair(rng, 120, 200, rgb=rgb)
        ref[20:53, 30:160] = 255
        img[10:63, 20:170] = 255
        mask = np.ones((120, 200), np.uint8)
        for method in (0, 3):
            _check(ref, img, mask, [(30, 20, 130, 33), (31, 21, 40, 20), (0, 0, 130, 33)], 8, method, refine=True)


# ---- the other keywords ----------------------------------------------------------------------------------------------------------
def test_offsets_clamped_ones_too():
    rng = np.random.RandomState(11)
    ref, img = _pair(rng, 150, 200, shift=(9, -7))
    blocks = B.grid(ref.shape, (24, 18), (29, 31))
    mask = _keep_one(rng.rand(150, 200) > 0.4, blocks)
    off = np.tile(np.array([[9, -7]]), (len(blocks), 1))
    off[::5] = [400, -400]                          # clamped into the image
    off[1::7] = [-3, 10 ** 6]
    for method in (0, 3):
        _check(ref, img, mask, blocks, 3, method, refine=True, offsets=off)
        zero = _call(ref, img, blocks, 3, method, mask=mask, offsets=np.zeros_like(off))
        MM.same(*zero, *_call(ref, img, blocks, 3, method, mask=mask))


@pytest.mark.parametrize("second", [True, 0])
def test_second_peaks(second):
    rng = np.random.RandomState(13)
    ref, img = _pair(rng, 120, 150, rgb=(second is True))
    blocks = _placed(120, 150, [(16, 16), (17, 65), (5, 130)])
    mask = _keep_one(rng.rand(120, 150) > 0.5, blocks)
    off = rng.randint(-6, 7, size=(len(blocks), 2))
    for method, margin, o in ((3, 8, None), (0, 1, None), (3, 0, None), (0, 8, off)):
        kw = {} if o is None else {"offsets": o}
        pos, sc, pos2, sc2 = _call(ref, img, blocks, margin, method, mask=mask, second=second, **kw)
        exp = MM.match_blocks(ref, img, mask, blocks, margin, method, offsets=o, second=second)
        MM.same(pos, sc, exp[0], exp[1])
        MM.same(pos2, sc2, exp[2], exp[3])
        MM.same(pos, sc, *_call(ref, img, blocks, margin, method, mask=mask, **kw))
        assert margin > 0 or np.isnan(sc2).all()


def test_none_rule_and_its_neighbours():
    """Against the model only: an empty mask under both methods, a box in an all-zero patch under method 3, NaN cells next to
    numbers - and the other blocks of the same call come out as they do alone."""
    rng = np.random.RandomState(17)
    ref, img = _pair(rng, 120, 150)
    img[30:90, 20:100] = 0
    mask = rng.rand(120, 150) > 0.3
    mask[0:16, 0:16] = False                        # block 0 keeps no pixel
    blocks = [(0, 0, 16, 16), (50, 50, 16, 16), (16, 0, 16, 16), (18, 40, 16, 16), (110, 90, 33, 20), (0, 100, 65, 17)]
    _keep_one(mask, blocks[1:])
    for method in (0, 3):
        for kw in ({}, {"offsets": np.array([[0, 0], [2, 2], [1, 0], [0, 3], [-2, 1], [0, 0]])}):
            pos, sc, pos2, sc2 = _call(ref, img, blocks, 6, method, mask=mask, second=1, **kw)
            exp = MM.match_blocks(ref, img, mask, blocks, 6, method, second=1, **kw)
            MM.same(pos, sc, exp[0], exp[1])
            MM.same(pos2, sc2, exp[2], exp[3])
            none = [0, 1] if method == 3 else [0]
            assert (pos[none] == -1).all() and np.isnan(sc[none]).all() and np.isnan(sc2[none]).all()
            rest = [k for k in range(len(blocks)) if k not in none]
            assert (pos[rest] >= 0).all() and not np.isnan(sc[rest]).any()
            fpos, fsc = _call(ref, img, blocks, 6, method, mask=mask, refine=True, **kw)
            assert fpos.dtype == np.float64 and (fpos[none] == -1.0).all() and np.isnan(fsc[none]).all()
            alone = _call(ref, img, [blocks[k] for k in rest], 6, method, mask=mask,
                          **{k: v[rest] for k, v in kw.items()})
            MM.same(pos[rest], sc[rest], *alone)


def test_several_chunks():
    """30 blocks of 16 x 16 take 2 * 256 template bytes each; a budget of 1280 floats = 5120 bytes holds ten: three chunks.
    The planner's debug entry keeps its unmasked meaning (256 bytes a block), so the split is asserted at half the budget,
    where the unmasked plan is the masked one's; that the masked call really plans 2 * chans bytes per pixel shows in its
    results, which a chunk of twice the planned bytes would overwrite."""
    rng = np.random.RandomState(19)
    ref, img = _pair(rng, 120, 150)
    blocks = B.grid(ref.shape, 16, (23, 21))[:30]
    assert len(blocks) == 30
    _, chunk_of, _, _ = _lib.debug_plan_blocks(ref.shape, 1, ref.dtype, blocks, 6, 4 * 1280 // 2)
    assert chunk_of.tolist() == [k // 10 for k in range(30)]
    mask = _keep_one(rng.rand(120, 150) > 0.5, blocks)
    mask[blocks[7][1]:blocks[7][1] + 16, blocks[7][0]:blocks[7][0] + 16] = False
    ctx = _lib.default_context()
    before = ctx.get_option(_lib.OPT_BOXES_MAX_FLOATS)
    whole = {m: _call(ref, img, blocks, 6, m, mask=mask, second=True) for m in (0, 3)}
    fine = _call(ref, img, blocks, 6, 3, mask=mask, refine=True)
    with _Opt(_lib.OPT_BOXES_MAX_FLOATS, 1280):
        for m in (0, 3):
            got = _call(ref, img, blocks, 6, m, mask=mask, second=True)
            MM.same(got[0], got[1], whole[m][0], whole[m][1])
            MM.same(got[2], got[3], whole[m][2], whole[m][3])
            MM.same(*_call(ref, img, blocks, 6, m, mask=mask), whole[m][0], whole[m][1])
        MM.same(*_call(ref, img, blocks, 6, 3, mask=mask, refine=True), *fine)
    assert ctx.get_option(_lib.OPT_BOXES_MAX_FLOATS) == before
    exp = MM.match_blocks(ref, img, mask, blocks, 6, 3, second=True)
    MM.same(whole[3][0], whole[3][1], exp[0], exp[1])
    MM.same(whole[3][2], whole[3][3], exp[2], exp[3])
    assert np.isnan(whole[3][1][7]) and np.isnan(whole[0][1][7])


def test_second_is_required_with_an_exclusion():
    """The entry itself, on a live context: exclusion >= 0 without a place for the second records is refused, and the same
    call with exclusion < 0 runs."""
    ctx = _lib.default_context()
    rng = np.random.RandomState(37)
    ref, img = _pair(rng, 40, 48)
    mask = np.ones((40, 48), np.uint8)
    blk = _lib.block_records([(4, 4, 8, 8)])
    out = np.zeros(1, dtype=_lib.HIT_DTYPE)

    def call(exclusion, second):
        with ctx.lock:
            return ctx._lib.mtm_match_blocks_masked(ctx._h, ref.ctypes.data, 48, img.ctypes.data, 48, mask.ctypes.data, 48, 40, 48,
                                                    1, _lib.MTM_U8, blk.ctypes.data, 1, None, 2, 3, exclusion, out.ctypes.data,
                                                    None, second)

    assert call(2, None) == -1 and b"mtm_match_blocks_masked: bad arguments" in ctx._lib.mtm_last_error()
    assert out["w"][0] == 0
    assert call(-1, None) == 0 and out["w"][0] == 8
    out2 = np.zeros(1, dtype=_lib.HIT_DTYPE)
    assert call(2, out2.ctypes.data) == 0 and out2["w"][0] == 8


# ---- the context's state ---------------------------------------------------------------------------------------------------------
def _keys(res):
    return [[(h[0], tuple(int(v) for v in h[1]), np.float32(h[2]).tobytes()) for h in r] for r in res]


def test_context_state_is_left_alone():
    rng = np.random.RandomState(29)
    ref, img = _pair(rng, 80, 100)
    mask = rng.rand(80, 100) > 0.3
    blocks = B.grid(ref.shape, 16)
    _keep_one(mask, blocks)
    templs = [("t%d" % k, rng.randint(0, 256, size=(7 + k, 9)).astype(np.uint8)) for k in range(3)]
    templs[0] = ("t0", img[20:27, 30:39].copy())
    boxes = [(10, 10, 60, 50), (0, 0, 100, 80)]
    default = _lib.default_context()
    options = {o: default.get_option(o) for o in _lib.ALL_OPTIONS}
    exp = MM.match_blocks(ref, img, mask, blocks, 4, 3)
    MM.same(*_call(ref, img, blocks, 4, 3, mask=mask), *exp)
    assert {o: default.get_option(o) for o in _lib.ALL_OPTIONS} == options

    ctx = _lib.Context()
    m = MTM.TemplateMatcher(templs, 5, N_object=1, score_threshold=0.2, context=ctx)
    first = m.match_boxes(img, boxes)
    resident = m._uploaded_for
    assert resident is not None
    MM.same(*_call(ref, img, blocks, 4, 3, mask=mask, context=ctx), *exp)
    MM.same(*_call(ref, img, blocks, 4, 0, mask=mask, context=ctx, second=True)[:2], *MM.match_blocks(ref, img, mask, blocks, 4, 0))
    assert m._uploaded_for == resident
    again = m.match_boxes(img, boxes)
    assert _keys(first) == _keys(again) and m._uploaded_for == resident
    ctx.close()


def test_mask_none_is_the_unmasked_call():
    """A sanity check (it passes without the feature's kernels): mask=None returns the arrays of the call without it, and an
    all-set mask changes the scores' rule but, for a moved copy, not where the blocks are found."""
    rng = np.random.RandomState(31)
    ref, img = _pair(rng, 100, 120, noise=0)
    blocks = B.grid(ref.shape, 16, 12)
    for method in (0, 3, 5):
        a = _call(ref, img, blocks, 4, method)
        b = _call(ref, img, blocks, 4, method, mask=None)
        assert all(np.array_equal(u, v) and u.dtype == v.dtype for u, v in zip(a, b))
    inner = [k for k, (x, y, w, h) in enumerate(blocks) if x + 2 + w <= 120 and y - 1 >= 0]
    pos, _ = _call(ref, img, blocks, 4, 3, mask=np.ones((100, 120), bool))
    assert (B.displacements(blocks, pos)[inner] == (2, -1)).all()
