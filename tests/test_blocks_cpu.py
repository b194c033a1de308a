"""MTM.matchBlocks / MTM.blocks without a GPU: every argument error comes before any native call, the helpers (grid,
search_box, displacements), the Python layer's result from a fake context that restates the call on the CPU oracle, what
reaches the context, the C ABI's declaration, and the host planner against a numpy restatement (tests/blocks_model.py)."""
import os
import re
import threading
import warnings

import numpy as np
import pytest

import MTM
import mtm_oracle as O
import blocks_model
from MTM import _lib
from MTM import blocks as B
from MTM.tracking import next_box

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


def _cut(smap, x, y):
    out = np.full((3, 3), np.nan, dtype=np.float32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if 0 <= y + dy < smap.shape[0] and 0 <= x + dx < smap.shape[1]:
                out[1 + dy, 1 + dx] = smap[y + dy, x + dx]
    return out


class _OracleCtx:
    """match_blocks on the CPU oracle: per block O.find_matches(..., N_object=1, searchBox=) of the block cut out of the
    reference, and its neighbourhood cut out of the oracle's whole-image score map.  Records what reaches it."""
    def __init__(self):
        self.lock = threading.RLock()
        self.calls = []

    def match_blocks(self, reference, image, blocks, margin, method, with_nbhd=False):
        self.calls.append((reference, image, blocks.copy(), margin, method, with_nbhd))
        n = len(blocks)
        out = np.zeros(n, dtype=_lib.HIT_DTYPE)
        nbhd = np.empty((n, 3, 3), dtype=np.float32) if with_nbhd else None
        ref, img = np.ascontiguousarray(reference), np.ascontiguousarray(image)
        for k, b in enumerate(blocks):
            x, y, w, h = (int(b[f]) for f in "xywh")
            t = ref[y:y + h, x:x + w]
            (_, (hx, hy, hw, hh), s), = O.find_matches([("b", t)], img, method, 1,
                                                       searchBox=B.search_box((x, y, w, h), margin, img.shape))
            out[k] = (k, hx, hy, hw, hh, s)
            if with_nbhd:
                nbhd[k] = _cut(O.compute_score_map(t, img, method), hx, hy)
        return out, nbhd

    def __getattr__(self, name):            # (anything else - set_templates above all - is not the call's business)
        raise AssertionError("matchBlocks used the context's %s" % name)


def _pair(seed, hw=(40, 52), kind="u8", shift=(2, -1)):
    rng = np.random.RandomState(seed)
    top = 65536 if kind == "u16" else 256
    shape = hw + (3,) if kind == "rgb" else hw
    ref = rng.randint(0, top, size=shape).astype(np.uint16 if kind == "u16" else np.uint8)
    img = np.roll(ref, (shift[1], shift[0]), axis=(0, 1)).astype(np.int64) + rng.randint(-2, 3, size=shape)
    return ref, np.clip(img, 0, top - 1).astype(ref.dtype)


# ---- errors, all before any native call ----------------------------------------------------------------------------------
def test_image_errors_come_before_any_native_call(no_native):
    u8 = np.zeros((20, 30), np.uint8)
    blk = [(0, 0, 4, 4)]
    bad_pairs = [
        (u8, np.zeros((20, 31), np.uint8)),                          # shape
        (u8, np.zeros((20, 30), np.uint16)),                         # dtype
        (u8, np.zeros((20, 30, 3), np.uint8)),                       # channels
        (np.zeros((20, 30, 1), np.uint8), u8),                       # (2-D against 3-D: shapes differ)
    ]
    for r, i in bad_pairs:
        with pytest.raises(ValueError, match="differ in shape, dtype or channel count"):
            MTM.matchBlocks(r, i, blk, 2)
    out_of_scope = [np.zeros((20, 30), np.float32), np.zeros((20, 30, 2), np.uint8), np.zeros((20, 30, 4), np.uint8),
                    np.zeros((20, 30, 3), np.uint16), np.zeros((20, 30), np.float64), np.zeros((20, 30), np.int8),
                    np.zeros((20,), np.uint8), np.zeros((2, 20, 30, 3), np.uint8)]
    for a in out_of_scope:
        with pytest.raises(ValueError, match="uint8 images with 1 or 3 channels and single-channel uint16"):
            MTM.matchBlocks(a, a.copy(), blk, 2)
    with pytest.raises(TypeError, match="reference must be a numpy array"):
        MTM.matchBlocks([[1, 2], [3, 4]], u8, blk, 2)
    with pytest.raises(TypeError, match="image must be a numpy array"):
        MTM.matchBlocks(u8, None, blk, 2)
    with pytest.raises(ValueError, match="at most 32767 rows"):
        tall = np.zeros((32768, 4), np.uint8)
        MTM.matchBlocks(tall, tall, blk, 2)


@pytest.mark.parametrize("blocks, exc, msg", [
    ([(0, 0, 4)], ValueError, r"\(N, 4\)"),
    (np.zeros((2, 5), np.int32), ValueError, r"\(N, 4\)"),
    (np.zeros((2, 2, 4), np.int32), ValueError, r"\(N, 4\)"),
    (7, ValueError, r"\(N, 4\)"),
    (np.zeros((2, 4), np.float32), TypeError, "integers"),
    (np.zeros((2, 4), bool), TypeError, "integers"),
    ([(0, 0, 4, 4), (1, 1, 4.0, 4)], TypeError, r"blocks\[1\]"),
    ([(0, 0, 4, 4), (1, 1, 0, 4), (50, 0, 4, 4)], ValueError, r"blocks\[1\].*w >= 1 and h >= 1"),
    ([(0, 0, 4, 4), (1, 1, 4, -2)], ValueError, r"blocks\[1\].*w >= 1 and h >= 1"),
    ([(0, 0, 4, 4), (0, 0, 30, 20), (27, 0, 4, 4), (0, 17, 4, 4)], ValueError, r"blocks\[2\].*not inside the 20 x 30"),
    ([(0, 17, 4, 4)], ValueError, r"blocks\[0\].*not inside"),
    ([(-1, 0, 4, 4)], ValueError, r"blocks\[0\].*not inside"),
    ([(0, -1, 4, 4)], ValueError, r"blocks\[0\].*not inside"),
    ([(0, 0, 31, 4)], ValueError, r"blocks\[0\].*not inside"),
    ([(2 ** 40, 0, 4, 4)], ValueError, r"blocks\[0\].*not inside"),
], ids=lambda v: None)
def test_block_errors_name_the_first_bad_block(no_native, blocks, exc, msg):
    ref, img = _pair(1, (20, 30))
    with pytest.raises(exc, match=msg):
        MTM.matchBlocks(ref, img, blocks, 2)
    with pytest.raises(exc, match=msg):
        MTM.matchBlocks(ref, img, blocks, 2, refine=True)


def test_uint16_block_of_more_than_2_21_pixels(no_native):
    a = np.zeros((2049, 1025), np.uint16)
    with pytest.raises(ValueError, match=r"blocks\[1\]: uint16 blocks of more than 2\^21 pixels"):
        MTM.matchBlocks(a, a, [(0, 0, 1024, 2048), (0, 0, 1025, 2047)], 0)
    b = np.zeros((2049, 1025), np.uint8)                # (uint8 has no such bound)
    with pytest.raises(_NativeCalled):
        MTM.matchBlocks(b, b, [(0, 0, 1025, 2047)], 0)


@pytest.mark.parametrize("margin", [-1, 1.0, "2", None, True, np.bool_(False), [1]], ids=repr)
def test_margin_must_be_a_non_negative_integer(no_native, margin):
    ref, img = _pair(1)
    with pytest.raises(ValueError, match="margin"):
        MTM.matchBlocks(ref, img, [(0, 0, 4, 4)], margin)
    with pytest.raises(ValueError, match="margin"):        # (also with nothing to match)
        MTM.matchBlocks(ref, img, [], margin)


@pytest.mark.parametrize("method", [-1, 6, 5.0, "5", None, True], ids=repr)
def test_method_outside_0_5(no_native, method):
    ref, img = _pair(1)
    with pytest.raises(ValueError, match="methods 0..5"):
        MTM.matchBlocks(ref, img, [(0, 0, 4, 4)], 2, method)


@pytest.mark.parametrize("refine", [1, 0, None, "yes", np.bool_(True)], ids=repr)
def test_refine_must_be_a_bool(no_native, refine):
    ref, img = _pair(1)
    with pytest.raises(ValueError, match="refine"):
        MTM.matchBlocks(ref, img, [(0, 0, 4, 4)], 2, refine=refine)
    with pytest.raises(TypeError):                          # (keyword-only)
        MTM.matchBlocks(ref, img, [(0, 0, 4, 4)], 2, 5, True)


def test_valid_arguments_reach_the_library(no_native):
    ref, img = _pair(1)
    with pytest.raises(_NativeCalled):
        MTM.matchBlocks(ref, img, [(0, 0, 4, 4)], np.int64(2), np.int32(3))


@pytest.mark.parametrize("blocks", [[], (), np.zeros((0, 4), np.int64), np.zeros((0, 4), np.float32), np.zeros(0)], ids=repr)
def test_empty_blocks_return_empty_arrays_without_the_library(no_native, blocks):
    ref, img = _pair(1)
    pos, sc = MTM.matchBlocks(ref, img, blocks, 3)
    assert pos.shape == (0, 2) and pos.dtype == np.int64 and sc.shape == (0,) and sc.dtype == np.float32
    pos, sc = MTM.matchBlocks(ref, img, blocks, 3, refine=True)
    assert pos.shape == (0, 2) and pos.dtype == np.float64 and sc.shape == (0,) and sc.dtype == np.float32


# ---- the helpers -----------------------------------------------------------------------------------------------------------
def test_search_box_is_next_box_of_the_block():
    rng = np.random.RandomState(3)
    H, W = 60, 75
    cases = []
    for k in range(200):
        w, h = int(rng.randint(1, 30)), int(rng.randint(1, 30))
        x, y = int(rng.randint(0, W - w + 1)), int(rng.randint(0, H - h + 1))
        if k % 8 == 0:
            x = 0
        elif k % 8 == 1:
            x = W - w
        elif k % 8 == 2:
            y = 0
        elif k % 8 == 3:
            y = H - h
        cases.append(((x, y, w, h), int(rng.randint(0, 40))))
    cases += [((0, 0, W, H), 5), ((0, 0, 1, 1), 0), ((W - 1, H - 1, 1, 1), 100)]
    for shape in ((H, W), (H, W, 3)):
        for block, margin in cases:
            for method in (1, 5):
                exp = next_box(None, (None, block, 0), margin, shape, method)
                got = B.search_box(block, margin, shape)
                assert got == exp and all(type(v) is int for v in got)
                x0, y0, bw, bh = got
                assert 0 <= x0 <= block[0] and 0 <= y0 <= block[1] and x0 + bw <= W and y0 + bh <= H
                assert bw >= block[2] and bh >= block[3]


def test_grid():
    g = B.grid((64, 96), 32)
    assert g.dtype == np.int64 and g.shape == (6, 4)
    assert g.tolist() == [[0, 0, 32, 32], [32, 0, 32, 32], [64, 0, 32, 32], [0, 32, 32, 32], [32, 32, 32, 32], [64, 32, 32, 32]]
    g = B.grid((70, 100, 3), 32)                        # sizes that do not divide the shape: the remainder is left out
    assert len(g) == 2 * 3 and g[-1].tolist() == [64, 32, 32, 32]
    g = B.grid((70, 100), (30, 20), 8)                  # (w, h) blocks at stride 8, overlapping
    assert len(g) == ((70 - 20) // 8 + 1) * ((100 - 30) // 8 + 1) and g[-1].tolist() == [64, 48, 30, 20]
    assert ((g[:, 0] + g[:, 2] <= 100) & (g[:, 1] + g[:, 3] <= 70)).all()
    g = B.grid((70, 100), (30, 20), (50, 25))
    assert g.tolist() == [[0, 0, 30, 20], [50, 0, 30, 20], [0, 25, 30, 20], [50, 25, 30, 20], [0, 50, 30, 20], [50, 50, 30, 20]]
    assert B.grid((70, 100), (100, 70)).tolist() == [[0, 0, 100, 70]]
    assert B.grid((70, 100), 101).shape == (0, 4) and B.grid((70, 100), (5, 71)).shape == (0, 4)
    for bad in (0, -3, (4, 0), (1, 2, 3), 2.5, True):
        with pytest.raises(ValueError, match="grid"):
            B.grid((70, 100), bad)
        with pytest.raises(ValueError, match="grid"):
            B.grid((70, 100), 8, bad)


def test_displacements():
    blocks = np.array([[10, 20, 8, 8], [0, 5, 4, 6]])
    d = B.displacements(blocks, np.array([[12, 19], [0, 5]], dtype=np.int64))
    assert d.dtype == np.int64 and d.tolist() == [[2, -1], [0, 0]]
    d = B.displacements(blocks.tolist(), np.array([[12.25, 19.5], [0.0, 4.75]]))
    assert d.dtype == np.float64 and d.tolist() == [[2.25, -0.5], [0.0, -0.25]]
    assert B.displacements([], np.zeros((0, 2))).shape == (0, 2)
    with pytest.raises(ValueError, match="displacements"):
        B.displacements(blocks, np.zeros((3, 2)))


# ---- the Python layer against the oracle -----------------------------------------------------------------------------------
def _oracle_loop(ref, img, blocks, margin, method):
    pos, sc, nb = [], [], []
    for x, y, w, h in blocks:
        t = ref[y:y + h, x:x + w]
        (_, box, s), = O.find_matches([("b", t)], img, method, 1, searchBox=B.search_box((x, y, w, h), margin, img.shape))
        pos.append(box[:2])
        sc.append(s)
        nb.append(_cut(O.compute_score_map(t, img, method), box[0], box[1]))
    return np.array(pos, dtype=np.int64), np.array(sc, dtype=np.float32), np.array(nb, dtype=np.float32)


@pytest.mark.parametrize("kind", ["u8", "rgb", "u16"])
@pytest.mark.parametrize("method", [1, 3, 5])
def test_python_layer_returns_the_loops_results(monkeypatch, kind, method):
    ref, img = _pair(5, kind=kind)
    # (the last block is the whole image: its hit is the map's only output, every neighbour outside the map)
    blocks = [(0, 0, 7, 5), (10, 8, 6, 6), (52 - 9, 40 - 4, 9, 4), (20, 0, 12, 3), (0, 30, 5, 10), (17, 11, 1, 1),
              (0, 0, 52, 40)]
    ctx = _OracleCtx()
    monkeypatch.setattr(_lib, "default_context", lambda: ctx)
    exp_pos, exp_sc, exp_nb = _oracle_loop(ref, img, blocks, 3, method)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pos, sc = MTM.matchBlocks(ref, img, blocks, 3, method)
        fpos, fsc = MTM.matchBlocks(ref, img, np.array(blocks), 3, method, refine=True, context=ctx)
    assert pos.dtype == np.int64 and sc.dtype == np.float32 and (pos == exp_pos).all()
    assert sc.tobytes() == exp_sc.tobytes() and fsc.tobytes() == exp_sc.tobytes()
    assert (B.displacements(blocks, pos)[1] == (2, -1)).all()       # the interior block follows the shift
    # refineHits' arithmetic: int(x) + offset as Python floats, the offsets of one fit_offsets call
    ox, oy = MTM.subpixel.fit_offsets(exp_nb, method)
    exp_f = np.array([[int(p[0]) + float(a), int(p[1]) + float(b)] for p, a, b in zip(exp_pos, ox, oy)])
    assert fpos.dtype == np.float64 and (fpos == exp_f).all()
    assert np.isnan(exp_nb[-1]).sum() == 8 and (ox != 0).any()      # (NaN neighbours at the map's edge; something was fitted)
    # what reached the context: the arrays as passed, int32 block records, the margin and method, refine as a flag
    (r0, i0, b0, m0, me0, nb0), (r1, i1, b1, m1, me1, nb1) = ctx.calls
    assert r0 is ref and i0 is img and r1 is ref and i1 is img
    for b in (b0, b1):
        assert b.dtype == _lib.BLOCK_DTYPE and b.dtype.itemsize == 16
        assert np.stack([b[f] for f in "xywh"], axis=1).tolist() == [list(v) for v in blocks]
    assert (m0, me0, nb0) == (3, method, False) and (m1, me1, nb1) == (3, method, True)


def test_views_reach_the_context_with_their_strides(monkeypatch):
    ref, img = _pair(7, (30, 40))
    big_r, big_i = np.zeros((60, 40), np.uint8), np.zeros((95, 40), np.uint8)
    big_r[::2], big_i[5::3] = ref, img
    rv, iv = big_r[::2], big_i[5::3]
    ctx = _OracleCtx()
    blocks = B.grid(ref.shape, (9, 7), (10, 11))
    pos, sc = MTM.matchBlocks(rv, iv, blocks, 40 * 10, 5, context=ctx)      # (a margin past the image: the whole image)
    (r, i, b, m, _, _), = ctx.calls
    assert r is rv and i is iv and r.strides[0] == 80 and i.strides[0] == 120 and m == 40
    exp_pos, exp_sc, _ = _oracle_loop(ref, img, blocks.tolist(), 400, 5)
    assert (pos == exp_pos).all() and sc.tobytes() == exp_sc.tobytes()
    a, ptr, stride = _lib._pixel_rows(rv)
    assert a is rv and stride == 80                                   # the binding passes the view's own rows


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import build as mtm_build
    mtm_build.build()
    return _lib.load()


def test_header_declares_the_entry_point(lib):
    hdr = open(os.path.join(ROOT, "include", "mtm_hip.h")).read()
    assert "#define MTM_ABI_VERSION 9" in hdr and _lib.ABI_VERSION == 9 and lib.mtm_abi_version() == 9
    decl = re.search(r"int mtm_match_blocks\(([^;]*)\);", hdr).group(1)
    assert len(decl.split(",")) == len(_lib.SYMBOLS["mtm_match_blocks"][1]) == 15
    assert "typedef struct mtm_block {" in hdr and re.search(r"int32_t x, y, w, h;\s*} mtm_block;", hdr)
    assert "mtm_debug_plan_blocks" in _lib.SYMBOLS and "matchBlocks" in MTM.__all__
    assert hasattr(_lib.Context, "match_blocks")
    import build as mtm_build
    assert "mtm_blocks.hip" in mtm_build.SOURCES


def test_null_context_is_refused_without_a_gpu(lib):
    out = np.zeros(1, dtype=_lib.HIT_DTYPE)
    px = np.zeros((8, 8), np.uint8)
    blk = _lib.block_records([(0, 0, 4, 4)])
    rc = lib.mtm_match_blocks(None, px.ctypes.data, 8, px.ctypes.data, 8, 8, 8, 1, _lib.MTM_U8, blk.ctypes.data, 1, 2, 5,
                              out.ctypes.data, None)
    assert rc == -1 and b"mtm_match_blocks" in lib.mtm_last_error()
    assert out["w"][0] == 0


# ---- the host planner ----------------------------------------------------------------------------------------------------------
def _same_plan(shape, chans, dtype, blocks, margin, budget):
    got = _lib.debug_plan_blocks(shape, chans, dtype, blocks, margin, budget)
    exp = blocks_model.plan(shape, chans, dtype, blocks, margin, budget)
    for g, e in zip(got, exp):
        assert g.dtype == e.dtype and g.shape == e.shape and (g == e).all(), (g, e)
    return got


def test_planner_tile_tables(lib):
    # maps of 1, 17 and 33 outputs per side: margins 0, 8 and 16 around an interior block
    shape = (120, 140)
    for margin, side in ((0, 1), (8, 17), (16, 33)):
        tiles, chunk_of, toff, maps = _same_plan(shape, 1, np.uint8, [(50, 40, 12, 10)], margin, 1 << 30)
        assert maps.tolist() == [[50 - margin, 40 - margin, side, side]]
        n = (side + 15) // 16
        assert tiles.tolist() == [[0, ty * 16, tx * 16] for ty in range(n) for tx in range(n)]
    # a margin of 15 clipped on two sides: 17 per side one pixel off the corner, 16 per side (one full tile) in the corner
    tiles, _, _, maps = _same_plan(shape, 1, np.uint8, [(1, 1, 12, 10)], 15, 1 << 30)
    assert maps.tolist() == [[0, 0, 17, 17]] and len(tiles) == 4
    tiles, _, _, maps = _same_plan(shape, 1, np.uint8, [(0, 0, 12, 10)], 15, 1 << 30)
    assert maps.tolist() == [[0, 0, 16, 16]] and tiles.tolist() == [[0, 0, 0]]
    # blocks on every edge, several kinds, against the model
    rng = np.random.RandomState(9)
    for chans, dtype in ((1, np.uint8), (3, np.uint8), (1, np.uint16)):
        blocks = []
        for _ in range(60):
            w, h = int(rng.randint(1, 50)), int(rng.randint(1, 40))
            blocks.append((int(rng.randint(0, 140 - w + 1)), int(rng.randint(0, 120 - h + 1)), w, h))
        blocks += [(0, 0, 140, 120), (139, 119, 1, 1), (0, 119, 140, 1)]
        for margin, budget in ((0, 1 << 30), (5, 4000), (20, 1), (300, 20000)):
            _same_plan(shape, chans, dtype, blocks, margin, budget)


def test_planner_chunk_split(lib):
    blocks = B.grid((64, 64), 16)                       # 16 blocks of 256 bytes (uint8), 512 (uint16), 768 (RGB)
    _, chunk_of, toff, _ = _same_plan((64, 64), 1, np.uint8, blocks, 2, 1024)
    assert chunk_of.tolist() == [k // 4 for k in range(16)] and toff.tolist() == [256 * (k % 4) for k in range(16)]
    _, chunk_of, toff, _ = _same_plan((64, 64), 1, np.uint16, blocks, 2, 1024)
    assert chunk_of.tolist() == [k // 2 for k in range(16)] and toff.tolist() == [512 * (k % 2) for k in range(16)]
    _, chunk_of, toff, _ = _same_plan((64, 64), 3, np.uint8, blocks, 2, 1024)
    assert chunk_of.tolist() == list(range(16)) and not toff.any()
    # a budget below every block: one block per chunk
    _, chunk_of, toff, _ = _same_plan((64, 64), 1, np.uint8, blocks, 2, 4)
    assert chunk_of.tolist() == list(range(16)) and not toff.any()
    _, chunk_of, _, _ = _same_plan((64, 64), 1, np.uint8, blocks, 2, 1 << 28)
    assert not chunk_of.any()


def test_planner_refuses_what_the_python_layer_refuses(lib):
    for blocks, msg in (([(0, 0, 4, 4), (27, 0, 4, 4)], b"block 1: block outside the reference"),
                        ([(0, 0, 0, 4)], b"block 0: empty block"),
                        ([(0, 0, 4, 4), (0, 0, 4, 4), (-1, 0, 4, 4)], b"block 2: block outside the reference")):
        with pytest.raises(_lib.MtmError):
            _lib.debug_plan_blocks((20, 30), 1, np.uint8, blocks, 2, 1 << 20)
        assert msg in lib.mtm_last_error()
    with pytest.raises(_lib.MtmError):
        _lib.debug_plan_blocks((2049, 1025), 1, np.uint16, [(0, 0, 1025, 2047)], 0, 1 << 30)
    assert b"block 0: uint16 block of more than 2^21 pixels" in lib.mtm_last_error()
    _lib.debug_plan_blocks((2049, 1025), 1, np.uint16, [(0, 0, 1024, 2048)], 0, 1 << 30)      # (exactly 2^21 passes)
