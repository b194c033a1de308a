"""MTM.matchBlocks on the GPU: every case equals the loop a user writes today - findMatchesInBoxes with the blocks cut out
of the reference on the host as templates and each block's search box as its region, N_object=1, then refineHits - in
positions (``==``) and float32 score bits; a dozen cases also equal the CPU oracle, so that the loop and the new call cannot
be wrong together."""
import warnings

import numpy as np
import pytest

import MTM
import mtm_oracle as O
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


def _cut(reference, blocks):
    return [("b%d" % k, np.ascontiguousarray(reference[y:y + h, x:x + w])) for k, (x, y, w, h) in enumerate(blocks)]


def _loop(reference, image, blocks, margin, method, refine=False, context=None):
    """The loop through findMatchesInBoxes (and refineHits): (positions, scores, refined positions or None)."""
    blocks = [tuple(int(v) for v in b) for b in blocks]
    templs = _cut(reference, blocks)
    regions = [(B.search_box(b, margin, image.shape), [k]) for k, b in enumerate(blocks)]
    res = MTM.findMatchesInBoxes(templs, image, regions, method, N_object=1, context=context)
    assert all(len(r) == 1 for r in res)
    hits = [r[0] for r in res]
    pos = np.array([[h[1][0], h[1][1]] for h in hits], dtype=np.int64).reshape(-1, 2)
    sc = np.array([h[2] for h in hits], dtype=np.float32)
    fine = None
    if refine:
        out = MTM.refineHits(templs, image, hits, method, context=context)
        fine = np.array([[h[1][0], h[1][1]] for h in out], dtype=np.float64).reshape(-1, 2)
    return pos, sc, fine


def _call(reference, image, blocks, margin, method, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("error")              # no warnings are emitted
        return MTM.matchBlocks(reference, image, blocks, margin, method, **kw)


def _same(got, exp_pos, exp_sc):
    pos, sc = got
    assert pos.dtype == exp_pos.dtype and pos.shape == exp_pos.shape
    bad = np.flatnonzero((pos != exp_pos).any(axis=1) | (sc.view(np.uint32) != exp_sc.view(np.uint32)))
    assert sc.dtype == np.float32 and len(bad) == 0, (bad[:5], pos[bad[:5]], exp_pos[bad[:5]], sc[bad[:5]], exp_sc[bad[:5]])


def _compare(reference, image, blocks, margin, method, refine=None, **kw):
    """matchBlocks against the loop, unrefined and (refine None: both; else as given) refined."""
    exp_pos, exp_sc, fine = _loop(reference, image, blocks, margin, method, refine is not False, kw.get("context"))
    if not refine:
        _same(_call(reference, image, blocks, margin, method, **kw), exp_pos, exp_sc)
    if refine is not False:
        _same(_call(reference, image, blocks, margin, method, refine=True, **kw), fine, exp_sc)
    return exp_pos, exp_sc


def _pair(rng, h, w, kind, shift=(2, -1), noise=3):
    """A reference and an image: the reference moved by `shift` = (dx, dy) (wrapping around) with a little noise."""
    top = 65536 if kind == "u16" else 256
    shape = (h, w, 3) if kind == "rgb" else (h, w)
    ref = rng.randint(0, top, size=shape).astype(np.uint16 if kind == "u16" else np.uint8)
    img = np.roll(ref, (shift[1], shift[0]), axis=(0, 1)).astype(np.int64) + rng.randint(-noise, noise + 1, size=shape)
    return ref, np.clip(img, 0, top - 1).astype(ref.dtype)


def _placed(H, W, shapes):
    """Every (h, w) of `shapes` at the four corners, the middles of the four edges and one interior place."""
    out = []
    for h, w in shapes:
        xs, ys = (0, (W - w) // 2, W - w), (0, (H - h) // 2, H - h)
        out += [(x, y, w, h) for y in ys for x in xs]
    return out


# ---- chunk and tile edges: the 16 x 64 template chunk's and the 4-byte quad's edges, maps of 1, 3, 15, 17 and 33 per side ---
_HS, _WS = (1, 15, 16, 17, 33), (1, 3, 4, 5, 63, 64, 65, 130)


@pytest.mark.parametrize("method", [5, 1])
@pytest.mark.parametrize("margin", [0, 1, 7, 8, 16])
def test_chunk_and_tile_edges_uint8(margin, method):
    rng = np.random.RandomState(100 + margin)
    ref, img = _pair(rng, 200, 240, "u8")
    blocks = _placed(200, 240, [(h, w) for h in _HS for w in _WS])
    _compare(ref, img, blocks, margin, method, refine=False)


@pytest.mark.parametrize("kind", ["rgb", "u16"])
@pytest.mark.parametrize("margin", [0, 8])
def test_chunk_and_tile_edges_rgb_and_uint16(margin, kind):
    rng = np.random.RandomState(200 + margin)
    ref, img = _pair(rng, 120, 150, kind)
    blocks = _placed(120, 150, [(h, w) for h in (1, 16, 17) for w in (4, 5, 64, 65)])
    _compare(ref, img, blocks, margin, 5)
    _compare(ref, img, blocks[::5], margin, 0, refine=False)


def test_largest_sums():
    """A 33 x 65 uint16 block of all 65535 in a region of all 65535, and a uint8 block of all 255."""
    rng = np.random.RandomState(7)
    for kind, top in (("u16", 65535), ("u8", 255)):
        ref, img = _pair(rng, 90, 120, kind)
        ref[20:20 + 33, 30:30 + 65] = top
        img[10:10 + 53, 20:20 + 85] = top
        for method in (0, 1, 2, 3, 4, 5):
            _compare(ref, img, [(30, 20, 65, 33), (31, 21, 40, 20), (0, 0, 65, 33)], 8, method)


# ---- degenerate content --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "rgb", "u16"])
def test_flat_block_and_flat_box(kind):
    rng = np.random.RandomState(11)
    ref, img = _pair(rng, 64, 80, kind)
    ref[10:30, 10:40] = 77                      # a flat block
    img[30:64, 40:80] = 5                       # a flat search box
    blocks = [(12, 12, 20, 10), (50, 40, 12, 9), (0, 0, 9, 9)]
    for method in (0, 1, 2, 3, 4, 5):
        exp_pos, exp_sc = _compare(ref, img, blocks, 6, method)
        if method == 5:                         # 1.0 everywhere: the box's first output
            assert tuple(exp_pos[0]) == (6, 6) and exp_sc[0] == np.float32(1.0)


def test_periodic_image_first_occurrence_wins():
    rng = np.random.RandomState(13)
    cell = rng.randint(0, 256, size=(6, 8)).astype(np.uint8)
    img = np.tile(cell, (10, 10))               # period 8 in x, 6 in y
    ref = img.copy()
    blocks = [(24, 18, 8, 6), (33, 25, 11, 7)]
    for method in (1, 3, 5):
        pos, sc = _call(ref, img, blocks, 9, method)
        exp_pos, exp_sc = _compare(ref, img, blocks, 9, method)
        # the box of block 0 starts at (15, 9): the first exact occurrence in row-major order is at (16, 12)
        assert tuple(pos[0]) == (16, 12) and tuple(exp_pos[0]) == (16, 12)
        # ... and of block 1, whose box starts at (24, 16), at (25, 19)
        assert tuple(pos[1]) == (25, 19)


def test_strides_and_fortran_order():
    rng = np.random.RandomState(17)
    for kind in ("u8", "rgb", "u16"):
        ref, img = _pair(rng, 70, 90, kind)
        big_r = np.zeros((140,) + ref.shape[1:], ref.dtype)
        big_i = np.zeros((215,) + ref.shape[1:], ref.dtype)
        big_r[::2] = ref
        big_i[5::3] = img
        rv, iv = big_r[::2], big_i[5::3]
        assert rv.strides[0] != iv.strides[0] and not rv.flags.c_contiguous
        blocks = B.grid(ref.shape, (13, 9), (11, 10))
        got = _call(rv, iv, blocks, 5, 5)
        _same(got, *_loop(ref, img, blocks, 5, 5)[:2])
        _same(_call(np.asfortranarray(ref), np.asfortranarray(img), blocks, 5, 5), got[0], got[1])


# ---- the seeded sweep ----------------------------------------------------------------------------------------------------
def _sweep_case(seed):
    rng = np.random.RandomState(1000 + seed)
    kind = ("u8", "rgb", "u16")[rng.randint(3)]
    method = int(rng.randint(6))
    H, W = (int(v) for v in rng.randint(24, 161, 2))
    ref, img = _pair(rng, H, W, kind, shift=(int(rng.randint(-3, 4)), int(rng.randint(-3, 4))))
    blocks = []
    for _ in range(int(rng.randint(1, 41))):
        w, h = int(rng.randint(1, min(W, 70) + 1)), int(rng.randint(1, min(H, 40) + 1))
        edge = rng.randint(4)                   # a good share of blocks touches the image's edge: NaN neighbours
        x = 0 if edge == 0 else W - w if edge == 1 else int(rng.randint(0, W - w + 1))
        y = 0 if edge == 2 else H - h if edge == 3 else int(rng.randint(0, H - h + 1))
        blocks.append((x, y, w, h))
    return ref, img, blocks, int(rng.randint(0, 13)), method


@pytest.mark.parametrize("seed", range(60))
def test_seeded_sweep(seed):
    ref, img, blocks, margin, method = _sweep_case(seed)
    exp_pos, exp_sc = _compare(ref, img, blocks, margin, method, refine=seed % 2 == 1)
    if seed % 5 == 0:       # the independent check: the CPU oracle's searchBox call per block
        for k, (x, y, w, h) in enumerate(blocks):
            (_, box, s), = O.find_matches([("b", ref[y:y + h, x:x + w])], img, method, 1,
                                          searchBox=B.search_box(blocks[k], margin, img.shape))
            assert tuple(box[:2]) == tuple(exp_pos[k]), (k, box, exp_pos[k])
            assert np.float32(s).tobytes() == exp_sc[k].tobytes(), (k, s, exp_sc[k])


# ---- chunking ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "u16"])
def test_one_block_per_chunk(kind):
    rng = np.random.RandomState(23)
    ref, img = _pair(rng, 96, 128, kind)
    blocks = B.grid(ref.shape, (20, 12), (17, 19))
    whole = _call(ref, img, blocks, 6, 5, refine=True)
    plain = _call(ref, img, blocks, 6, 5)
    with _Opt(_lib.OPT_BOXES_MAX_FLOATS, 1):        # 4 bytes of templates: every block is a chunk of its own
        _same(_call(ref, img, blocks, 6, 5, refine=True), *whole)
        _same(_call(ref, img, blocks, 6, 5), *plain)
    _same(plain, *_loop(ref, img, blocks, 6, 5)[:2])


# ---- the context's state -------------------------------------------------------------------------------------------------
def _keys(res):
    return [[(h[0], tuple(int(v) for v in h[1]), np.float32(h[2]).tobytes()) for h in r] for r in res]


def test_context_state_is_left_alone():
    rng = np.random.RandomState(29)
    ref, img = _pair(rng, 80, 100, "u8")
    templs = [("t%d" % k, rng.randint(0, 256, size=(7 + k, 9)).astype(np.uint8)) for k in range(3)]
    templs[0] = ("t0", img[20:27, 30:39].copy())
    regions = [((10, 10, 60, 50), [0, 1]), ((0, 0, 100, 80), [2])]
    blocks = B.grid(ref.shape, 16)
    before = MTM.findMatchesInBoxes(templs, img, regions, 5, N_object=1)
    got = _call(ref, img, blocks, 4, 3)
    after = MTM.findMatchesInBoxes(templs, img, regions, 5, N_object=1)
    assert _keys(before) == _keys(after)
    # two calls with different methods back to back: the gathered constants depend on the method
    for method in (5, 1, 4, 0):
        _same(_call(ref, img, blocks, 4, method), *_loop(ref, img, blocks, 4, method)[:2])
    _same(got, *_loop(ref, img, blocks, 4, 3)[:2])

    ctx = _lib.Context()
    m = MTM.TemplateMatcher(templs, 5, N_object=1, score_threshold=0.2, context=ctx)
    boxes = [r[0] for r in regions]
    first = m.match_boxes(img, boxes)
    resident = m._uploaded_for
    assert resident is not None
    _same(_call(ref, img, blocks, 4, 1, context=ctx), *_loop(ref, img, blocks, 4, 1)[:2])
    assert m._uploaded_for == resident
    again = m.match_boxes(img, boxes)
    assert _keys(first) == _keys(again) and m._uploaded_for == resident
    assert _keys(first) == _keys(MTM.matchTemplatesInBoxes(templs, img, boxes, 5, 1, 0.2))
    ctx.close()


# ---- a displacement field --------------------------------------------------------------------------------------------------
def test_field_of_overlapping_blocks_recovers_the_shift():
    rng = np.random.RandomState(31)
    ref = rng.randint(0, 256, size=(512, 640)).astype(np.uint8)
    dx, dy = 3, -2
    img = np.roll(ref, (dy, dx), axis=(0, 1))
    blocks = B.grid(ref.shape, 16, 8)
    assert len(blocks) == 63 * 79
    pos, sc = _call(ref, img, blocks, 4, 5)
    _same((pos, sc), *_loop(ref, img, blocks, 4, 5)[:2])
    d = B.displacements(blocks, pos)
    inner = (blocks[:, 0] >= 8) & (blocks[:, 1] >= 8) & (blocks[:, 0] + 16 <= 632) & (blocks[:, 1] + 16 <= 504)
    assert inner.sum() > 4000 and (d[inner] == (dx, dy)).all() and (sc[inner] == np.float32(1.0)).all()
