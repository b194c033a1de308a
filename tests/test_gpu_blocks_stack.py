"""MTM.matchBlocksStack on the GPU.  Per pair every case equals the loop of MTM.matchBlocks over the pairs (itself pinned
against findMatchesInBoxes and the oracle by test_gpu_blocks.py) in positions (``==``) and float32 score bits, and - the two
calls share their chain of launches - one test pins the stack call itself against the findMatchesInBoxes loop; the ensemble
planes equal, bit for bit, a restatement from MTM.computeScoreMap of host-cut blocks on host-cut search-box crops
(tests/blocks_stack_model.py), and their peaks the restated peak rule; frame and block chunking change no byte."""
import warnings

import numpy as np
import pytest

import MTM
import blocks_stack_model as M
from MTM import _lib
from MTM import blocks as B
from test_gpu_blocks import _loop as _boxes_loop

pytestmark = pytest.mark.gpu

H, W = 72, 96


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


def _movie(seed, n, kind, step=(1, -1), noise=3, hw=(H, W)):
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


def _placed(shapes):
    """Every (h, w) of `shapes` at the four corners, the middles of the four edges and one interior place."""
    out = []
    for h, w in shapes:
        xs, ys = (0, (W - w) // 2, W - w), (0, (H - h) // 2, H - h)
        out += [(x, y, w, h) for y in ys for x in xs]
    return out


_EDGE_BLOCKS = _placed([(h, w) for h in (1, 16, 17) for w in (1, 4, 5, 64, 65)])
_MARGINS = (0, 1, 7, 8, 16)         # maps of 1, 3, 15, 17 and 33 per side, clipped differently on all four sides


def _call(frames, blocks, margin, method, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("error")              # no warnings are emitted
        return MTM.matchBlocksStack(frames, blocks, margin, method, **kw)


def _loop(frames, blocks, margin, method, reference, refine):
    """The loop of matchBlocks over the pairs: (positions (P, N, 2), scores (P, N))."""
    mode = M.FIRST if reference == "first" else M.PREVIOUS
    res = [MTM.matchBlocks(frames[r], frames[s], blocks, margin, method, refine=refine)
           for r, s in M.pair_frames(len(frames), mode)]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def _same(got, exp):
    (pos, sc), (exp_pos, exp_sc) = got[:2], exp[:2]
    assert pos.dtype == exp_pos.dtype and pos.shape == exp_pos.shape and sc.dtype == np.float32 and sc.shape == exp_sc.shape
    bad = np.argwhere((pos != exp_pos).any(axis=-1) | (sc.view(np.uint32) != exp_sc.view(np.uint32)))
    assert len(bad) == 0, (bad[:5], [(pos[tuple(i)], exp_pos[tuple(i)], sc[tuple(i)], exp_sc[tuple(i)]) for i in bad[:5]])


def _same_planes(got, exp):
    assert got.dtype == np.float32 and got.shape == exp.shape
    assert (np.isnan(got) == np.isnan(exp)).all(), np.argwhere(np.isnan(got) != np.isnan(exp))[:5]
    bad = np.argwhere(got.view(np.uint32) != exp.view(np.uint32))
    assert len(bad) == 0, (bad[:5], [(got[tuple(i)], exp[tuple(i)]) for i in bad[:5]])


# ---- per pair: the loop of matchBlocks -----------------------------------------------------------------------------------
_KIND_METHODS = [(k, m) for k in ("u8", "rgb", "u16") for m in (1, 3, 5)] + [("u8", m) for m in (0, 2, 4)]


@pytest.mark.parametrize("refine", [False, True])
@pytest.mark.parametrize("reference", ["previous", "first"])
@pytest.mark.parametrize("kind, method", _KIND_METHODS)
def test_pairs_equal_the_loop(kind, method, reference, refine):
    frames = _movie(300 + method, 4, kind)
    for margin in _MARGINS:
        got = _call(frames, _EDGE_BLOCKS, margin, method, reference=reference, refine=refine)
        assert got[0].shape == (3, len(_EDGE_BLOCKS), 2) and got[0].dtype == (np.float64 if refine else np.int64)
        _same(got, _loop(frames, _EDGE_BLOCKS, margin, method, reference, refine))


# ---- per pair: the loop of findMatchesInBoxes on host-cut templates, another kernel family and host path -------------------
# 3 frames of 48 x 96; margin 9: an interior block's 19 x 19 map has four tiles, three of them partial
_ANCHOR_HW, _ANCHOR_MARGIN = (48, 96), 9
_ANCHOR_BLOCKS = [(10, 20, 70, 5),      # 5 x 70: crosses the 64-column template chunk
                  (50, 12, 4, 17),      # 17 x 4: crosses the 16-row template chunk
                  (90, 44, 6, 4),       # the bottom right corner: its box is clipped on two sides
                  (40, 30, 1, 1)]       # (x, y, w, h)


@pytest.mark.parametrize("method", [1, 5])
@pytest.mark.parametrize("refine", [False, True])
@pytest.mark.parametrize("reference", ["previous", "first"])
@pytest.mark.parametrize("kind", ["u8", "rgb", "u16"])
def test_pairs_equal_the_boxes_loop(kind, reference, refine, method):
    """matchBlocksStack against findMatchesInBoxes (and refineHits) per pair, bit for bit: test_pairs_equal_the_loop
    compares two calls that run one chain of launches, this one does not.  Once with every block in one chunk ("first"
    gathers once), once with a chunk per block."""
    frames = _movie(390 + method, 3, kind, hw=_ANCHOR_HW)
    blocks, margin, n = _ANCHOR_BLOCKS, _ANCHOR_MARGIN, len(_ANCHOR_BLOCKS)
    chans, dtype = (3 if kind == "rgb" else 1), frames[0].dtype
    budget = 4 * int(_lib.default_context().get_option(_lib.OPT_BOXES_MAX_FLOATS))
    tiles, chunk_of, _, maps = _lib.debug_plan_blocks(_ANCHOR_HW, chans, dtype, blocks, margin, budget)
    assert (chunk_of == 0).all() and maps[0].tolist() == [1, 11, 19, 19] and maps[2, 2:].tolist() == [10, 10]
    assert tiles[tiles[:, 0] == 0, 1:].tolist() == [[0, 0], [0, 16], [16, 0], [16, 16]]
    assert (_lib.debug_plan_blocks(_ANCHOR_HW, chans, dtype, blocks, margin, 4)[1] == np.arange(n)).all()
    mode = M.FIRST if reference == "first" else M.PREVIOUS
    per_pair = [_boxes_loop(frames[r], frames[s], blocks, margin, method, refine) for r, s in M.pair_frames(3, mode)]
    exp = np.stack([fine if refine else pos for pos, _, fine in per_pair]), np.stack([sc for _, sc, _ in per_pair])
    _same(_call(frames, blocks, margin, method, reference=reference, refine=refine), exp)
    with _Opt(_lib.OPT_BOXES_MAX_FLOATS, 1):            # 4 bytes of templates: every block is a chunk of its own
        _same(_call(frames, blocks, margin, method, reference=reference, refine=refine), exp)


@pytest.mark.parametrize("kind", ["u8", "rgb", "u16"])
def test_two_frames_are_one_matchBlocks_call_and_one_frame_is_none(kind):
    frames = _movie(310, 2, kind, step=(2, -1))
    for reference in ("previous", "first"):
        for refine in (False, True):
            pos, sc = _call(np.stack(frames), _EDGE_BLOCKS, 7, 5, reference=reference, refine=refine)
            e_pos, e_sc = MTM.matchBlocks(frames[0], frames[1], _EDGE_BLOCKS, 7, 5, refine=refine)
            _same((pos, sc), (e_pos[None], e_sc[None]))
            pos, sc = _call(frames[:1], _EDGE_BLOCKS, 7, 5, reference=reference, refine=refine)
            assert pos.shape == (0, len(_EDGE_BLOCKS), 2) and pos.dtype == e_pos.dtype and sc.shape == (0, len(_EDGE_BLOCKS))
    # the movie's step is found by the blocks that hold enough pixels, away from the border
    d = B.displacements(_EDGE_BLOCKS, _call(frames, _EDGE_BLOCKS, 7, 5)[0][0])
    inner = [k for k, (x, y, w, h) in enumerate(_EDGE_BLOCKS) if w * h >= 64 and 2 <= x <= W - w - 2 and 2 <= y <= H - h - 2]
    assert len(inner) >= 4 and (d[inner] == (2, -1)).all()


def test_views_and_frames_of_different_strides():
    for kind in ("u8", "rgb", "u16"):
        frames = _movie(320, 4, kind)
        big = np.zeros((4, 2 * H) + frames[0].shape[1:], frames[0].dtype)
        big[:, ::2] = np.stack(frames)
        wide = np.zeros((H, W + 9) + frames[0].shape[2:], frames[0].dtype)
        wide[:, 4:W + 4] = frames[2]
        views = [big[0, ::2], big[1, ::2], wide[:, 4:W + 4], np.asfortranarray(frames[3])]
        assert len({v.strides[0] for v in views}) > 1 and not views[0].flags.c_contiguous
        blocks = B.grid((H, W), (13, 9), (11, 10))
        for kw in ({"refine": True}, {"reference": "first"}):
            _same(_call(views, blocks, 5, 5, **kw), _call(frames, blocks, 5, 5, **kw))
        _same_planes(_call(views, blocks, 5, 5, ensemble=True)[2], _call(frames, blocks, 5, 5, ensemble=True)[2])
        _same(_call(big[:, ::2], blocks, 5, 5), _call(frames, blocks, 5, 5))


# ---- chunk seams -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reference", ["previous", "first"])
@pytest.mark.parametrize("kind", ["u8", "rgb", "u16"])
def test_frame_and_block_chunks_change_no_byte(kind, reference):
    frames = _movie(330, 5, kind)
    blocks = B.grid((H, W), (32, 24), 16)
    n = len(blocks)
    kw = {"reference": reference}
    plain = _call(frames, blocks, 6, 5, **kw)
    fine = _call(frames, blocks, 6, 5, refine=True, **kw)
    # the planes' own bound (N (2 margin + 1)^2 floats) admits no budget of 1: the smallest budget that passes it, 9 n floats
    # = 36 n bytes of templates at margin 1, still gives every one of these blocks a chunk of its own
    ens = _call(frames, blocks, 1, 5, ensemble=True, refine=True, **kw)
    chans, dtype = (3 if kind == "rgb" else 1), frames[0].dtype
    assert n >= 12 and 36 * n < 2 * 32 * 24
    assert (_lib.debug_plan_blocks((H, W), chans, dtype, blocks, 1, 36 * n)[1] == np.arange(n)).all()

    def check():
        _same(_call(frames, blocks, 6, 5, **kw), plain)
        _same(_call(frames, blocks, 6, 5, refine=True, **kw), fine)

    def check_ensemble():
        got = _call(frames, blocks, 1, 5, ensemble=True, refine=True, **kw)
        _same_planes(got[2], ens[2])
        _same(got, ens)

    # 2 frames per stack, 3, and a row bound below two frames (a stack never holds fewer than two)
    for max_rows in (2 * H, 3 * H, H + 28):
        with _Opt(_lib.OPT_BATCH_MAX_ROWS, max_rows):
            check()
            check_ensemble()
    with _Opt(_lib.OPT_BOXES_MAX_FLOATS, 1):            # 4 bytes of templates: every block is a chunk of its own
        check()
    with _Opt(_lib.OPT_BOXES_MAX_FLOATS, 9 * n):
        check_ensemble()
    for max_rows in (2 * H, 3 * H):
        with _Opt(_lib.OPT_BATCH_MAX_ROWS, max_rows):
            with _Opt(_lib.OPT_BOXES_MAX_FLOATS, 1):
                check()
            with _Opt(_lib.OPT_BOXES_MAX_FLOATS, 9 * n):
                check_ensemble()
    _same(plain, _loop(frames, blocks, 6, 5, reference, False))
    with _Opt(_lib.OPT_BOXES_MAX_FLOATS, 9 * n - 1):    # one float short: refused, by the Python layer and by the library
        with pytest.raises(ValueError, match="OPT_BOXES_MAX_FLOATS = %d" % (9 * n - 1)):
            _call(frames, blocks, 1, 5, ensemble=True, **kw)
        with pytest.raises(_lib.MtmError, match="MTM_OPT_BOXES_MAX_FLOATS = %d" % (9 * n - 1)):
            _lib.default_context().match_blocks_stack(frames, blocks, 1, 5, M.PREVIOUS, planes=True)


# ---- ensemble planes -------------------------------------------------------------------------------------------------------
# the four corners sit closer to the border than the margin, by another distance on every side: (ox, oy) differ per block
_PLANE_MARGIN = 6
_PLANE_BLOCKS = [(2, 3, 10, 8), (W - 10 - 1, 2, 10, 8), (3, H - 8 - 2, 10, 8), (W - 10 - 4, H - 8 - 1, 10, 8),
                 (0, 0, 5, 5), (W - 5, H - 5, 5, 5), (40, 0, 9, 7), (0, 30, 4, 17), (40, 30, 16, 16), (20, 20, 1, 1),
                 (10, 50, 65, 4), (0, 10, W, 3), (5, 0, 7, H)]


@pytest.mark.parametrize("reference", ["previous", "first"])
@pytest.mark.parametrize("method", [1, 5])
@pytest.mark.parametrize("kind", ["u8", "rgb", "u16"])
def test_ensemble_planes_equal_the_restatement(kind, method, reference):
    frames = _movie(340 + method, 4, kind)
    mode = M.FIRST if reference == "first" else M.PREVIOUS
    exp = M.planes(MTM.computeScoreMap, frames, _PLANE_BLOCKS, _PLANE_MARGIN, method, mode)
    offs = M.clip((H, W), _PLANE_BLOCKS, _PLANE_MARGIN)
    assert offs[:4].tolist() == [[4, 3], [0, 4], [3, 0], [0, 0]] and np.isnan(exp[3, 8:]).all() and np.isnan(exp[3, :, 11:]).all()
    pos, sc, planes = _call(frames, _PLANE_BLOCKS, _PLANE_MARGIN, method, reference=reference, ensemble=True)
    side = 2 * _PLANE_MARGIN + 1
    assert planes.shape == (len(_PLANE_BLOCKS), side, side)
    _same_planes(planes, exp)
    e_pos, e_sc, cells = M.peaks(exp, _PLANE_BLOCKS, method)
    assert pos.dtype == np.int64 and sc.dtype == np.float32
    _same((pos, sc), (e_pos, e_sc))
    fpos, fsc, fplanes = _call(frames, _PLANE_BLOCKS, _PLANE_MARGIN, method, reference=reference, ensemble=True, refine=True)
    ox, oy = MTM.subpixel.fit_offsets(M.peak_neighbourhoods(exp, cells), method)
    assert fpos.dtype == np.float64 and (ox != 0).any()
    _same((fpos, fsc), (e_pos.astype(np.float64) + np.stack((ox, oy), axis=1), e_sc))
    _same_planes(fplanes, exp)
    p2, s2 = B.plane_peaks(planes, _PLANE_BLOCKS, method)          # public: the planes peak again
    _same((p2, s2), (pos, sc))


def test_ensemble_of_one_pair_is_matchBlocks():
    for kind in ("u8", "rgb", "u16"):
        frames = _movie(350, 2, kind, step=(2, -1))
        for method in ((0, 1, 2, 3, 4, 5) if kind == "u8" else (1, 3, 5)):
            for margin in (0, 7, 16):
                pos, sc, _ = _call(frames, _EDGE_BLOCKS[::2], margin, method, ensemble=True)
                _same((pos, sc), MTM.matchBlocks(frames[0], frames[1], _EDGE_BLOCKS[::2], margin, method))
        # a flat block (method 5: 1.0 everywhere, the box's first output) and a flat search box
        ref, img = frames[0].copy(), frames[1].copy()
        ref[10:30, 10:40] = 77
        img[30:64, 40:80] = 5
        blocks = [(12, 12, 20, 10), (50, 40, 12, 9), (0, 0, 9, 9)]
        for method in (0, 1, 2, 3, 4, 5):
            pos, sc, _ = _call([ref, img], blocks, 6, method, ensemble=True)
            _same((pos, sc), MTM.matchBlocks(ref, img, blocks, 6, method))
            if method == 5:
                assert tuple(pos[0]) == (6, 6) and sc[0] == np.float32(1.0)
    # a periodic image: the first exact occurrence in row-major order of the box's map wins
    rng = np.random.RandomState(13)
    img = np.tile(rng.randint(0, 256, size=(6, 8)).astype(np.uint8), (10, 10))
    blocks = [(24, 18, 8, 6), (33, 25, 11, 7)]
    for method in (1, 3, 5):
        pos, sc, _ = _call([img, img.copy()], blocks, 9, method, ensemble=True)
        _same((pos, sc), MTM.matchBlocks(img, img, blocks, 9, method))
        assert tuple(pos[0]) == (16, 12) and tuple(pos[1]) == (25, 19)


def test_ensemble_finds_a_shift_that_single_pairs_miss():
    """Frames of noise (sigma 22) around a weak common pattern (sigma about 9) that moves by (2, 1) a frame: two frames'
    matching 16 x 16 blocks correlate with about 0.14, 2.2 times the 1 / 16 scatter of unrelated blocks' correlation, so a
    pair's own plane often peaks elsewhere among its 81 cells; the mean of 8 planes stands sqrt(8) times higher, 6 such
    deviations, and peaks at the step.  (The CPU oracle's planes of this movie: 38 % of the blocks from the pairs' peaks,
    all of them from the mean.)"""
    rng = np.random.RandomState(360)
    base = rng.randint(0, 256, size=(H, W)).astype(np.float64)
    frames = [np.clip(128 + 0.12 * (np.roll(base, (f, 2 * f), axis=(0, 1)) - 128) + rng.normal(0, 22, size=(H, W)), 0, 255)
              .astype(np.uint8) for f in range(9)]
    blocks = B.grid((H, W), 16, 8)
    blocks = blocks[(blocks[:, 0] >= 8) & (blocks[:, 1] >= 8) & (blocks[:, 0] + 24 <= W) & (blocks[:, 1] + 24 <= H)]
    pos, _ = _call(frames, blocks, 4, 5)
    epos, _, _ = _call(frames, blocks, 4, 5, ensemble=True)
    single = np.mean([(B.displacements(blocks, p) == (2, 1)).all(axis=1).mean() for p in pos])
    ens = (B.displacements(blocks, epos) == (2, 1)).all(axis=1).mean()
    assert ens > single and ens >= 0.9, (single, ens)


# ---- hygiene ---------------------------------------------------------------------------------------------------------------
def _keys(res):
    return [[(h[0], tuple(int(v) for v in h[1]), np.float32(h[2]).tobytes()) for h in r] for r in res]


def test_repeats_and_the_contexts_state():
    rng = np.random.RandomState(29)
    frames = _movie(370, 4, "u8")
    templs = [("t%d" % k, rng.randint(0, 256, size=(7 + k, 9)).astype(np.uint8)) for k in range(3)]
    templs[0] = ("t0", frames[1][20:27, 30:39].copy())
    regions = [((10, 10, 60, 50), [0, 1]), ((0, 0, W, H), [2])]
    blocks = B.grid((H, W), 16)
    before = MTM.findMatchesInBoxes(templs, frames[1], regions, 5, N_object=1)
    first = _call(frames, blocks, 4, 3, refine=True)
    ens = _call(frames, blocks, 4, 3, ensemble=True, reference="first")
    after = MTM.findMatchesInBoxes(templs, frames[1], regions, 5, N_object=1)
    assert _keys(before) == _keys(after)
    again = _call(frames, blocks, 4, 3, refine=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    again = _call(frames, blocks, 4, 3, ensemble=True, reference="first")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ens, again))
    # a resident template set on a context of its own stays as it is
    ctx = _lib.Context()
    m = MTM.TemplateMatcher(templs, 5, N_object=1, score_threshold=0.2, context=ctx)
    boxes = [r[0] for r in regions]
    hits = m.match_boxes(frames[1], boxes)
    resident = m._uploaded_for
    assert resident is not None
    _same(_call(frames, blocks, 4, 1, context=ctx), _loop(frames, blocks, 4, 1, "previous", False))
    _same_planes(_call(frames, blocks, 4, 3, ensemble=True, reference="first", context=ctx)[2], ens[2])
    assert m._uploaded_for == resident and _keys(hits) == _keys(m.match_boxes(frames[1], boxes))
    ctx.close()


def test_planes_hold_nothing_of_the_call_before():
    a, b = _movie(380, 4, "u16"), _movie(381, 3, "u16")
    blocks = _PLANE_BLOCKS
    ctx = _lib.default_context()
    want = _call(b, blocks, 5, 5, ensemble=True)[2]
    other = _call(a, blocks, 5, 5, ensemble=True)[2]            # leaves its sums in the context's buffer
    got = _call(b, blocks, 5, 5, ensemble=True)[2]
    _same_planes(got, want)
    assert other.tobytes() != want.tobytes()
    ctx.debug_poison(0x7F, _lib.POISON_ARENAS)                  # ... and so does a buffer full of a huge number
    _same_planes(_call(b, blocks, 5, 5, ensemble=True)[2], want)
    ctx.debug_poison(0xFF, _lib.POISON_ARENAS)                  # ... or of NaN
    _same_planes(_call(b, blocks, 5, 5, ensemble=True)[2], want)
    _same_planes(want, M.planes(MTM.computeScoreMap, b, blocks, 5, 5, M.PREVIOUS))
