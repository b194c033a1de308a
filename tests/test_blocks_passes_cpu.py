"""MTM.matchBlocks(offsets=), MTM.blocks.search_box_at / predict_offsets and MTM.matchBlocksMultipass without a GPU: the
helpers, every argument error before any native call, the nearest-block rule against a brute-force search and against the
host C that the kernel shares (mtm_debug_plan_blocks_passes), the fixed tile table and the chunk split against a numpy
restatement (tests/blocks_passes_model.py), the Python layer's composition on the CPU oracle, and the C ABI's declarations."""
import os
import re

import numpy as np
import pytest

import MTM
import blocks_passes_model as M
from MTM import _lib
from MTM import blocks as B

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


class _NativeCalled(Exception):
    pass


@pytest.fixture
def no_native(monkeypatch):
    """Any use of the library raises _NativeCalled: an error that comes first was raised in the Python layer."""
    def boom(*a, **k):
        raise _NativeCalled()
    monkeypatch.setattr(_lib, "default_context", boom)
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_lib, "engine_for", boom)


def _pair(seed, hw=(40, 52), kind="u8", shift=(5, -3)):
    rng = np.random.RandomState(seed)
    top = 65536 if kind == "u16" else 256
    shape = hw + (3,) if kind == "rgb" else hw
    ref = rng.randint(0, top, size=shape).astype(np.uint16 if kind == "u16" else np.uint8)
    img = np.roll(ref, (shift[1], shift[0]), axis=(0, 1)).astype(np.int64) + rng.randint(-2, 3, size=shape)
    return ref, np.clip(img, 0, top - 1).astype(ref.dtype)


# ---- search_box_at --------------------------------------------------------------------------------------------------------
def test_search_box_at():
    shape = (50, 60)
    rng = np.random.RandomState(1)
    for _ in range(200):
        w, h = int(rng.randint(1, 61)), int(rng.randint(1, 51))
        blk = (int(rng.randint(0, 60 - w + 1)), int(rng.randint(0, 50 - h + 1)), w, h)
        m = int(rng.randint(0, 9))
        assert B.search_box_at(blk, (0, 0), m, shape) == B.search_box(blk, m, shape)
        dx, dy = (int(v) for v in rng.randint(-70, 71, 2))
        x0, y0, bw, bh = B.search_box_at(blk, (dx, dy), m, shape)
        cx, cy = min(max(blk[0] + dx, 0), 60 - w), min(max(blk[1] + dy, 0), 50 - h)
        assert (x0, y0, bw, bh) == B.search_box((cx, cy, w, h), m, shape)
        assert x0 >= 0 and y0 >= 0 and x0 + bw <= 60 and y0 + bh <= 50 and bw >= w and bh >= h      # the map is never empty
    blk = (20, 15, 8, 6)
    # the four borders: the moved block stops at the border, the box is clipped there
    assert B.search_box_at(blk, (-25, 0), 3, shape) == (0, 12, 11, 12)
    assert B.search_box_at(blk, (45, 0), 3, shape) == (49, 12, 11, 12)
    assert B.search_box_at(blk, (0, -20), 3, shape) == (17, 0, 14, 9)
    assert B.search_box_at(blk, (0, 40), 3, shape) == (17, 41, 14, 9)
    # any magnitude
    assert B.search_box_at(blk, (10 ** 9, -10 ** 9), 3, shape) == (49, 0, 11, 9)
    assert B.search_box_at(blk, (-10 ** 9, 10 ** 9), 3, shape) == (0, 41, 11, 9)
    assert B.search_box_at(blk, (10 ** 30, 0), 0, shape) == (52, 15, 8, 6)
    # margin 0: the moved block itself, a 1 x 1 map
    assert B.search_box_at(blk, (4, -2), 0, shape) == (24, 13, 8, 6)
    assert B.search_box_at(blk, (100, 100), 0, shape) == (52, 44, 8, 6)


# ---- predict_offsets ------------------------------------------------------------------------------------------------------
def _random_grid_pair(rng):
    H, W = (int(v) for v in rng.randint(8, 90, 2))
    kind = rng.randint(5)
    wc, hc = int(rng.randint(1, W + 1)), int(rng.randint(1, H + 1))
    sx, sy = int(rng.randint(1, 25)), int(rng.randint(1, 25))
    if kind == 0:       # one column of coarse blocks
        wc = int(rng.randint(W // 2 + 1, W + 1))
        sx = W
    elif kind == 1:     # one row
        hc = int(rng.randint(H // 2 + 1, H + 1))
        sy = H
    elif kind == 2:     # overlapping coarse blocks much larger than the stride: wf < wc - s
        wc, hc = int(rng.randint(W // 2, W + 1)), int(rng.randint(H // 2, H + 1))
        sx, sy = int(rng.randint(1, 4)), int(rng.randint(1, 4))
    wf, hf = int(rng.randint(1, W + 1)), int(rng.randint(1, H + 1))
    if kind in (2, 3):
        wf, hf = int(rng.randint(1, max(2, wc // 4))), int(rng.randint(1, max(2, hc // 4)))
    fx, fy = int(rng.randint(1, 13)), int(rng.randint(1, 13))
    return (H, W), ((wc, hc), (sx, sy)), ((wf, hf), (fx, fy))


def test_predict_offsets_against_brute_force_and_host_c():
    rng = np.random.RandomState(2)
    seen = {"small_fine": 0, "one_row": 0, "one_col": 0, "tie": 0}
    for _ in range(200):
        shape, coarse, fine = _random_grid_pair(rng)
        cg, fg = B.grid(shape, *coarse), B.grid(shape, *fine)
        pos = cg[:, :2] + rng.randint(-20, 21, size=(len(cg), 2))
        near = M.nearest_brute(shape, coarse, fine)
        exp = pos[near] - cg[near, :2]
        got = B.predict_offsets(shape, coarse, pos, fine)
        assert got.dtype == np.int64 and got.shape == (len(fg), 2) and (got == exp).all(), (shape, coarse, fine)
        (wc, hc), (sx, sy) = coarse
        seen["small_fine"] += fine[0][0] < wc - sx
        seen["one_row"] += len(np.unique(cg[:, 1])) == 1 and len(cg) > 1
        seen["one_col"] += len(np.unique(cg[:, 0])) == 1 and len(cg) > 1
        seen["tie"] += bool(((2 * fg[:, 0] + fg[:, 2] - wc + sx) % (2 * sx) == 0).any())
        # the host C that blocks_unit_kernel shares: the same offsets, and search_box_at's units
        margin = int(rng.randint(0, 7))
        rec = [(wc, hc, sx, sy, 3), fine[0] + fine[1] + (margin,)]
        counts, _, _, pred, maps = _lib.debug_plan_blocks_passes(shape, 1, np.uint8, rec, 1 << 30, coarse=pos, at_pass=1)
        assert list(counts) == [len(cg), len(fg)] and (pred == exp).all()
        boxes = np.array([B.search_box_at(fg[k], exp[k], margin, shape) for k in range(len(fg))])
        assert (maps[:, 0] == boxes[:, 0]).all() and (maps[:, 1] == boxes[:, 1]).all()
        assert (maps[:, 2] == boxes[:, 2] - fg[:, 2] + 1).all() and (maps[:, 3] == boxes[:, 3] - fg[:, 3] + 1).all()
    assert min(seen.values()) >= 10, seen


def test_predict_offsets_ties_go_to_the_higher_index():
    # coarse 8-wide blocks at stride 8 (doubled centres 8, 24, 40, 56), fine 4-wide blocks at stride 2: the fine block at x = 6
    # (doubled centre 16) lies exactly between coarse 0 and 1, the one at x = 14 between 1 and 2
    shape = (8, 32)
    pos = B.grid(shape, 8)[:, :2] + np.array([[1, 0], [2, 0], [3, 0], [4, 0]])
    got = B.predict_offsets(shape, (8, None), pos, ((4, 8), (2, 8)))
    fx = B.grid(shape, (4, 8), (2, 8))[:, 0]
    assert list(got[fx == 4, 0]) == [1] and list(got[fx == 6, 0]) == [2] and list(got[fx == 8, 0]) == [2]
    assert list(got[fx == 14, 0]) == [3] and list(got[fx == 22, 0]) == [4] and list(got[fx == 28, 0]) == [4]
    assert (got[:, 1] == 0).all()


def test_predict_offsets_errors(no_native):
    shape = (40, 52)
    pos = B.grid(shape, 16)[:, :2]
    with pytest.raises(ValueError, match=r"positions of shape \(5, 2\) for a coarse grid of 6 blocks"):
        B.predict_offsets(shape, (16, None), pos[:5], (8, None))
    with pytest.raises(ValueError, match="positions of shape"):
        B.predict_offsets(shape, (16, None), pos.reshape(-1), (8, None))
    with pytest.raises(TypeError, match="positions must be integers"):
        B.predict_offsets(shape, (16, None), pos.astype(np.float64), (8, None))
    with pytest.raises(ValueError, match="predict_offsets: block must be a positive integer"):
        B.predict_offsets(shape, (0, None), pos, (8, None))
    with pytest.raises(ValueError, match="predict_offsets: step must be a positive integer"):
        B.predict_offsets(shape, (16, -1), pos, (8, None))
    with pytest.raises(ValueError, match=r"\(block, step\) pairs"):
        B.predict_offsets(shape, 16, pos, (8, None))
    with pytest.raises(ValueError, match="the coarse grid is empty"):
        B.predict_offsets(shape, (64, None), np.zeros((0, 2), np.int64), (8, None))
    assert B.predict_offsets(shape, (16, None), pos, (64, None)).shape == (0, 2)


# ---- the host plan --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chans, dtype", [(1, np.uint8), (3, np.uint8), (1, np.uint16)])
def test_plan_tiles_and_chunks(chans, dtype):
    shape = (96, 120)
    passes = [(32, 32, 16, 16, 8), (17, 9, 8, 11, 20), (16, 16, 8, 8, 2), (8, 8, 4, 4, 0), (5, 7, 9, 9, 7)]
    for budget in (1 << 30, 3000, 1):
        counts, tiles, chunk_of = _lib.debug_plan_blocks_passes(shape, chans, dtype, passes, budget)
        e_counts, e_tiles, e_chunk = M.plan(shape, chans, dtype, passes, budget)
        assert (counts == e_counts).all() and tiles.shape == e_tiles.shape and (tiles == e_tiles).all()
        assert (chunk_of == e_chunk).all()
        for p, a in enumerate(passes):      # ceil((2 m + 1) / 16)^2 tiles per block, whatever its clipped map
            per_block = np.bincount(tiles[tiles[:, 0] == p, 1], minlength=counts[p])
            assert (per_block == (-(-(2 * a[4] + 1) // 16)) ** 2).all()
    _, _, chunk_of = _lib.debug_plan_blocks_passes(shape, chans, dtype, passes, 1)
    assert (chunk_of[:counts[0]] == np.arange(counts[0])).all()          # a chunk holds at least one block


def test_plan_errors():
    shape = (40, 52)
    with pytest.raises(RuntimeError, match=r"pass 1.*empty grid"):
        _lib.debug_plan_blocks_passes(shape, 1, np.uint8, [(8, 8, 8, 8, 2), (53, 8, 8, 8, 2)], 1 << 20)
    for bad in ((0, 8, 8, 8, 2), (8, 8, 0, 8, 2), (8, 8, 8, 8, -1)):
        with pytest.raises(RuntimeError, match="pass 1: block and step must be >= 1"):
            _lib.debug_plan_blocks_passes(shape, 1, np.uint8, [(8, 8, 8, 8, 2), bad], 1 << 20)
    # a margin past the image: per axis the tiles of the block's map over the whole image (33 x 45 outputs), no more
    counts, tiles, _ = _lib.debug_plan_blocks_passes(shape, 1, np.uint8, [(8, 8, 8, 8, 10 ** 6)], 1 << 20)
    e_counts, e_tiles, _ = M.plan(shape, 1, np.uint8, [(8, 8, 8, 8, 10 ** 6)], 1 << 20)
    assert (counts == e_counts).all() and (tiles == e_tiles).all() and len(tiles) == 9 * counts[0]
    with pytest.raises(RuntimeError, match="uint16 block of more than 2\\^21 pixels"):
        _lib.debug_plan_blocks_passes((2049, 1025), 1, np.uint16, [(1025, 2047, 1, 1, 0)], 1 << 30)


# ---- errors, all before any native call ----------------------------------------------------------------------------------
def test_offsets_errors_come_before_any_native_call(no_native):
    u8 = np.zeros((20, 30), np.uint8)
    blk = [(0, 0, 4, 4), (5, 5, 4, 4)]
    for bad in ([(0, 0)], [(0, 0), (1, 1), (2, 2)], [(0, 0, 0), (1, 1, 1)], np.zeros((2, 2, 2), np.int32), 3, [0, 0, 0, 0]):
        with pytest.raises(ValueError, match=r"offsets must be an \(N, 2\).*got shape .* for blocks of shape \(2, 4\)"):
            MTM.matchBlocks(u8, u8, blk, 2, offsets=bad)
    for bad in ([(0, 0), (1.0, 1)], np.zeros((2, 2), np.float32), np.zeros((2, 2), bool), [(0, 0), (None, 1)]):
        with pytest.raises(TypeError, match=r"offsets\[\d\]: \(dx, dy\) of block \d must be integers"):
            MTM.matchBlocks(u8, u8, blk, 2, offsets=bad)
    with pytest.raises(TypeError, match=r"offsets\[1\]"):
        MTM.matchBlocks(u8, u8, blk, 2, offsets=[(0, 0), (1, 2.5)])
    # the call's other errors still come first, and any magnitude passes the checks (the native call is the next thing)
    with pytest.raises(ValueError, match=r"blocks\[1\].*not inside"):
        MTM.matchBlocks(u8, u8, [(0, 0, 4, 4), (28, 0, 4, 4)], 2, offsets=[(0, 0)])
    for big in ([(10 ** 9, -10 ** 9), (0, 0)], [(10 ** 30, 0), (0, -10 ** 30)], np.array([[2 ** 63 - 1, 0], [0, -2 ** 63]]),
                np.array([[2 ** 64 - 1, 0], [0, 1]], dtype=np.uint64)):
        with pytest.raises(_NativeCalled):
            MTM.matchBlocks(u8, u8, blk, 2, offsets=big)
    assert MTM.matchBlocks(u8, u8, [], 2, offsets=[])[0].shape == (0, 2)


def test_multipass_errors_come_before_any_native_call(no_native):
    u8 = np.zeros((20, 30), np.uint8)
    ok = [(8, 4, 2)]
    with pytest.raises(ValueError, match="differ in shape, dtype or channel count"):
        MTM.matchBlocksMultipass(u8, np.zeros((20, 31), np.uint8), ok)
    with pytest.raises(ValueError, match="uint8 images with 1 or 3 channels"):
        MTM.matchBlocksMultipass(u8.astype(np.float32), u8.astype(np.float32), ok)
    with pytest.raises(TypeError, match="reference must be a numpy array"):
        MTM.matchBlocksMultipass(None, u8, ok)
    with pytest.raises(ValueError, match="methods 0..5"):
        MTM.matchBlocksMultipass(u8, u8, ok, 6)
    with pytest.raises(ValueError, match="refine must be True or False"):
        MTM.matchBlocksMultipass(u8, u8, ok, refine=1)
    with pytest.raises(ValueError, match="passes is empty"):
        MTM.matchBlocksMultipass(u8, u8, [])
    with pytest.raises(TypeError, match="passes must be a sequence"):
        MTM.matchBlocksMultipass(u8, u8, 7)
    for bad in ((8, 4), 8, (8, 4, 2, 1)):
        with pytest.raises(ValueError, match=r"passes\[1\] must be \(block, step, margin\)"):
            MTM.matchBlocksMultipass(u8, u8, ok + [bad])
    with pytest.raises(ValueError, match=r"passes\[1\]: block must be a positive integer"):
        MTM.matchBlocksMultipass(u8, u8, ok + [(0, 4, 2)])
    with pytest.raises(ValueError, match=r"passes\[1\]: step must be a positive integer"):
        MTM.matchBlocksMultipass(u8, u8, ok + [(8, (4, 0), 2)])
    for bad in (-1, 1.0, None, True):
        with pytest.raises(ValueError, match=r"passes\[1\]: margin must be an integer >= 0"):
            MTM.matchBlocksMultipass(u8, u8, ok + [(8, 4, bad)])
    with pytest.raises(ValueError, match=r"passes\[1\]: no 31 x 8 block fits the 20 x 30 images \(empty grid\)"):
        MTM.matchBlocksMultipass(u8, u8, ok + [((31, 8), None, 2)])
    big = np.zeros((2049, 1025), np.uint16)
    with pytest.raises(ValueError, match=r"passes\[0\]: uint16 blocks of more than 2\^21 pixels"):
        MTM.matchBlocksMultipass(big, big, [((1025, 2047), None, 0)])
    with pytest.raises(_NativeCalled):
        MTM.matchBlocksMultipass(u8, u8, ok + [(4, None, 10 ** 12)])


# ---- the Python layer on the CPU oracle ----------------------------------------------------------------------------------
def _by_hand(ref, img, passes, method, refine, ctx):
    out, off, steer = [], None, None
    for p, (block, step, margin) in enumerate(passes):
        b = B.grid(img.shape, block, step)
        if p:
            off = B.predict_offsets(img.shape, passes[p - 1][:2], steer, passes[p][:2])
        steer, _ = MTM.matchBlocks(ref, img, b, margin, method, offsets=off, context=ctx)
        pos, sc = MTM.matchBlocks(ref, img, b, margin, method, offsets=off, refine=refine, context=ctx)
        out.append((b, pos, sc))
    return out


@pytest.mark.parametrize("kind, method", [("u8", 5), ("u8", 1), ("rgb", 3), ("u16", 5), ("u16", 0)])
def test_multipass_composition_on_the_oracle(kind, method):
    ref, img = _pair(3, kind=kind)
    passes = [(16, 8, 6), ((8, 6), (5, 7), 2), (4, None, 0)]
    for refine in (False, True):
        ctx = M.OracleCtx()
        got = MTM.matchBlocksMultipass(ref, img, passes, method, refine=refine, context=ctx)
        (tag, rec, counts, m, with_nbhd), = ctx.calls
        assert tag == "passes" and m == method and with_nbhd is refine
        assert rec.tolist() == [(16, 16, 8, 8, 6), (8, 6, 5, 7, 2), (4, 4, 4, 4, 0)]
        exp = _by_hand(ref, img, passes, method, refine, M.OracleCtx())
        assert len(got) == len(exp) == 3
        for (gb, gp, gs), (eb, ep, es) in zip(got, exp):
            assert gb.dtype == np.int64 and (gb == eb).all()
            assert gp.dtype == ep.dtype == (np.float64 if refine else np.int64) and (gp == ep).all()
            assert gs.dtype == np.float32 and gs.tobytes() == es.tobytes()
    # the coarse pass found the shift on its interior block, and the fine passes follow it beyond their own margins
    d = B.displacements(got[1][0], np.round(got[1][1]).astype(np.int64))
    assert (d == (5, -3)).all(axis=1).sum() >= len(d) // 3


def test_offsets_reach_the_context_clamped():
    ref, img = _pair(4)
    blocks = [(0, 0, 8, 8), (44, 32, 8, 8), (10, 10, 6, 5)]
    ctx = M.OracleCtx()
    pos, sc = MTM.matchBlocks(ref, img, blocks, 3, 5, offsets=[(-10 ** 12, 7), (10 ** 30, 10 ** 9), (5, -3)], context=ctx)
    (tag, _, off, margin, method, with_nbhd), = ctx.calls
    assert tag == "at" and off.dtype == np.int32 and off.tolist() == [[0, 7], [0, 0], [5, -3]]
    assert tuple(pos[2]) == (15, 7) and sc.dtype == np.float32
    # a margin past the images' larger side is that side's; offsets=None is the call as it was
    MTM.matchBlocks(ref, img, blocks, 10 ** 9, 5, offsets=[(0, 0)] * 3, context=ctx)
    MTM.matchBlocks(ref, img, blocks, 3, 5, context=ctx)
    assert ctx.calls[1][3] == 52 and ctx.calls[2][0] == "plain"


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_abi_and_exports():
    hdr = open(os.path.join(ROOT, "include", "mtm_hip.h")).read()
    assert re.search(r"#define MTM_ABI_VERSION 9\b", hdr) and _lib.load().mtm_abi_version() == 9
    since = re.search(r"Entry points added since 9 - (.*?) - are new symbols only", hdr, re.S).group(1)
    for name, n_args in (("mtm_match_blocks_at", 16), ("mtm_match_blocks_passes", 14), ("mtm_debug_plan_blocks_passes", 16)):
        assert name in _lib.SYMBOLS and name in since
        decl = re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[name][1]) == n_args
    assert _lib.BLOCK_PASS_DTYPE.itemsize == 20
    for name in ("matchBlocksMultipass",):
        assert name in MTM.__all__ and getattr(MTM, name) is getattr(B, name)
    for name in ("matchBlocksMultipass", "search_box_at", "predict_offsets"):
        assert name in B.__all__
