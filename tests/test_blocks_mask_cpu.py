"""MTM.matchBlocks(mask=) without a GPU: the argument errors come before any native call, ``mask=None`` is the call as it
was, ``mask_fraction`` against a brute-force loop, the model (tests/blocks_mask_model.py) against the oracle's loop and on
its none rule, and the C ABI's entry refusing bad arguments."""
import os
import re
import threading

import numpy as np
import pytest

import MTM
import mtm_oracle as O
import blocks_mask_model as MM
import blocks_second_model as S2
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


class _FakeCtx:
    """Records what reaches the context; returns records at the blocks' own positions."""
    def __init__(self):
        self.lock = threading.RLock()
        self.calls = []

    def _out(self, blocks, with_nbhd):
        out = np.zeros(len(blocks), dtype=_lib.HIT_DTYPE)
        out["x"], out["y"], out["w"], out["h"] = blocks["x"], blocks["y"], blocks["w"], blocks["h"]
        return out, (np.zeros((len(blocks), 3, 3), np.float32) if with_nbhd else None)

    def match_blocks(self, *args, **kw):
        self.calls.append(("match_blocks", args, kw))
        return self._out(args[2], args[5])

    def match_blocks_at(self, *args, **kw):
        self.calls.append(("match_blocks_at", args, kw))
        res = self._out(args[2], args[6])
        return res + (res[0].copy(),) if "second" in kw else res

    def match_blocks_masked(self, *args, **kw):
        self.calls.append(("match_blocks_masked", args, kw))
        res = self._out(args[3], args[7])
        return res + (res[0].copy(),) if kw.get("second") is not None else res


def _pair(seed, hw=(40, 52), rgb=False, lo=1):
    rng = np.random.RandomState(seed)
    shape = hw + (3,) if rgb else hw
    ref = rng.randint(lo, 256, size=shape).astype(np.uint8)
    img = np.roll(ref, (-1, 2), axis=(0, 1)).astype(np.int64) + rng.randint(-2, 3, size=shape)
    return ref, np.clip(img, lo, 255).astype(np.uint8)


# ---- errors, all before any native call ----------------------------------------------------------------------------------
def test_mask_errors_come_before_any_native_call(no_native):
    ref, img = _pair(1)
    blk = [(3, 4, 8, 6)]
    ok = np.ones((40, 52), np.uint8)
    for bad, exc, frag in [
            (np.ones((40, 51), np.uint8), ValueError, "mask of shape"),
            (np.ones((52, 40), bool), ValueError, "mask of shape"),
            (np.ones((40, 52, 1), np.uint8), ValueError, "2-D"),
            (np.ones((40, 52, 3), bool), ValueError, "2-D"),
            (np.ones((40 * 52,), np.uint8), ValueError, "2-D"),
            (np.ones((40, 52), np.float32), TypeError, "bool or uint8"),
            (np.ones((40, 52), np.int32), TypeError, "bool or uint8"),
            (np.ones((40, 52), np.uint16), TypeError, "bool or uint8"),
            (ok.tolist(), TypeError, "numpy array"),
    ]:
        with pytest.raises(exc, match=frag):
            MTM.matchBlocks(ref, img, blk, 2, 3, mask=bad)
    for method in (1, 2, 4, 5):
        with pytest.raises(ValueError, match="methods 0 .* and 3"):
            MTM.matchBlocks(ref, img, blk, 2, method, mask=ok)
    with pytest.raises(ValueError, match="methods 0 .* and 3"):
        MTM.matchBlocks(ref, img, blk, 2, mask=ok)                      # (the default method is 5)
    r16 = ref.astype(np.uint16)
    with pytest.raises(ValueError, match="uint8 images"):
        MTM.matchBlocks(r16, r16.copy(), blk, 2, 0, mask=ok)
    with pytest.raises(ValueError, match="not inside"):                 # (the other checks still run)
        MTM.matchBlocks(ref, img, [(50, 0, 8, 6)], 2, 0, mask=ok)
    with pytest.raises(_NativeCalled):                                  # (and a good call does reach the library)
        MTM.matchBlocks(ref, img, blk, 2, 0, mask=ok)


def test_multipass_and_stack_take_no_mask():
    ref, img = _pair(2)
    with pytest.raises(TypeError):
        MTM.matchBlocksMultipass(ref, img, [(8, 8, 2)], 0, mask=np.ones((40, 52), bool))
    with pytest.raises(TypeError):
        MTM.matchBlocksStack([ref, img], [(0, 0, 8, 8)], 2, 0, mask=np.ones((40, 52), bool))


# ---- what reaches the context ------------------------------------------------------------------------------------------------
def test_mask_none_is_the_call_as_it_was():
    ref, img = _pair(3)
    blk = [(3, 4, 8, 6), (20, 10, 5, 5)]
    off = np.array([[1, -1], [0, 2]])
    for kw, name in [({}, "match_blocks"), ({"offsets": off}, "match_blocks_at"), ({"second": True}, "match_blocks_at"),
                     ({"refine": True}, "match_blocks"), ({"offsets": off, "second": 1, "refine": True}, "match_blocks_at")]:
        a, b = _FakeCtx(), _FakeCtx()
        MTM.matchBlocks(ref, img, blk, 2, 3, context=a, **kw)
        MTM.matchBlocks(ref, img, blk, 2, 3, context=b, mask=None, **kw)
        (na, aa, ka), = a.calls
        (nb, ab, kb), = b.calls
        assert na == nb == name and ka == kb and len(aa) == len(ab)
        for u, v in zip(aa, ab):
            assert type(u) is type(v) and (np.array_equal(u, v) if isinstance(u, np.ndarray) else u == v)


def test_a_mask_reaches_the_masked_entry_as_uint8():
    ref, img = _pair(4)
    blk = [(3, 4, 8, 6), (20, 10, 5, 5)]
    mask = np.random.RandomState(4).rand(40, 52) > 0.4
    for m in (mask, mask.astype(np.uint8) * 7, np.asfortranarray(mask), (mask.astype(np.uint8) * 255)[:, ::1]):
        ctx = _FakeCtx()
        pos, sc, pos2, sc2 = MTM.matchBlocks(ref, img, blk, 2, 0, context=ctx, mask=m, second=3, offsets=[[1, 0], [0, -1]])
        (name, args, kw), = ctx.calls
        assert name == "match_blocks_masked" and kw == {"second": 3}
        assert args[0] is ref and args[1] is img and args[5:] == (2, 0, False)
        assert args[2].dtype == np.uint8 and args[2].shape == (40, 52) and args[2].flags.c_contiguous
        assert np.array_equal(args[2] != 0, mask)
        assert args[4].dtype == np.int32 and args[4].tolist() == [[1, 0], [0, -1]]
        assert pos.tolist() == [[3, 4], [20, 10]] and pos2.dtype == np.int64 and sc2.dtype == np.float32
    ctx = _FakeCtx()
    pos, sc = MTM.matchBlocks(ref, img, blk, 2, 3, context=ctx, mask=mask, refine=True)
    (name, args, kw), = ctx.calls
    assert name == "match_blocks_masked" and args[4] is None and args[7] is True and kw == {"second": None}
    assert pos.dtype == np.float64
    ctx = _FakeCtx()
    res = MTM.matchBlocks(ref, img, [], 2, 3, context=ctx, mask=mask, second=True)
    assert not ctx.calls and [len(a) for a in res] == [0, 0, 0, 0]


# ---- mask_fraction ---------------------------------------------------------------------------------------------------------
def test_mask_fraction_against_a_loop():
    rng = np.random.RandomState(5)
    for H, W in ((1, 1), (7, 13), (40, 52)):
        for mask in (rng.rand(H, W) > 0.3, (rng.rand(H, W) > 0.7).astype(np.uint8) * 200, np.ones((H, W), bool),
                     np.zeros((H, W), np.uint8)):
            blocks = []
            for _ in range(40):
                w, h = rng.randint(1, W + 1), rng.randint(1, H + 1)
                blocks.append((rng.randint(0, W - w + 1), rng.randint(0, H - h + 1), w, h))
            blocks += [(0, 0, W, H), (W - 1, H - 1, 1, 1)]
            got = B.mask_fraction(mask, blocks)
            exp = np.array([np.count_nonzero(mask[y:y + h, x:x + w]) / float(w * h) for x, y, w, h in blocks])
            assert got.dtype == np.float64 and got.shape == (len(blocks),) and np.array_equal(got, exp)
            assert np.array_equal(B.mask_fraction(mask, np.array(blocks)), exp)
    assert B.mask_fraction(np.ones((4, 4), bool), []).shape == (0,)
    assert B.mask_fraction(np.ones((4, 4), bool), np.zeros((0, 4), int)).dtype == np.float64
    with pytest.raises(ValueError, match="not inside"):
        B.mask_fraction(np.ones((4, 4), bool), [(2, 2, 3, 3)])
    with pytest.raises(TypeError):
        B.mask_fraction(np.ones((4, 4), np.float32), [(0, 0, 1, 1)])
    with pytest.raises(ValueError):
        B.mask_fraction(np.ones((4, 4, 1), bool), [(0, 0, 1, 1)])


# ---- the model ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rgb", [False, True])
@pytest.mark.parametrize("method", [0, 3])
def test_model_equals_the_oracle_loop(method, rgb):
    """NaN-free inputs (pixels in 1..255, every block keeps a pixel): the model is the loop of the oracle's find_matches with
    masked tuples, and its second peaks are blocks_second_model's plain loops over the same maps."""
    ref, img = _pair(10 + method, rgb=rgb)
    mask = np.random.RandomState(6).rand(40, 52) > 0.5
    blocks = [(0, 0, 7, 5), (45, 35, 7, 5), (20, 12, 9, 9), (3, 30, 17, 4), (30, 0, 1, 1), (10, 10, 1, 6)]
    mask[0, 30] = mask[10, 10] = True
    assert (B.mask_fraction(mask, blocks) > 0).all()
    offsets = np.array([[0, 0], [5, 5], [-3, 2], [1, -40], [2, 2], [0, 0]])
    for margin in (0, 1, 4):
        for off in (None, offsets):
            pos, sc, pos2, sc2 = MM.match_blocks(ref, img, mask, blocks, margin, method, offsets=off, second=1)
            for k, b in enumerate(blocks):
                box = MM.box_of(b, None if off is None else off[k], margin, img.shape)
                (_, (x, y, w, h), s), = O.find_matches([MM.block_tuple(ref, mask, b)], img, method, 1, searchBox=box)
                assert (x, y) == tuple(pos[k]) and (w, h) == b[2:] and np.float32(s).tobytes() == sc[k].tobytes()
                smap, (x0, y0) = MM.block_map(ref, img, mask, b, None if off is None else off[k], margin, method)
                assert not np.isnan(smap).any()
                ((sx, sy), s2), (fx, fy) = S2.second_peak(smap, method, 1)
                assert (fx + x0, fy + y0) == tuple(pos[k])
                assert ((sx + x0, sy + y0) if sx >= 0 else (-1, -1)) == tuple(pos2[k])
                assert (np.isnan(s2) and np.isnan(sc2[k])) or np.float32(s2).tobytes() == sc2[k].tobytes()
            assert MM.match_blocks(ref, img, mask, blocks, margin, method, offsets=off)[0].tolist() == pos.tolist()


def test_model_none_rule():
    ref, img = _pair(20, lo=1)
    img[10:34, 8:44] = 0                                    # an all-zero patch
    mask = np.ones((40, 52), bool)
    mask[0:8, 0:8] = False                                  # block 0 keeps no pixel
    blocks = [(0, 0, 8, 8), (20, 18, 6, 6), (0, 30, 8, 8), (6, 15, 6, 6)]
    # method 3: block 1's box (margin 4) lies in the patch - every output NaN; block 3's box reaches out of it
    pos, sc, pos2, sc2 = MM.match_blocks(ref, img, mask, blocks, 4, 3, second=True)
    assert pos[0].tolist() == pos[1].tolist() == [-1, -1] and np.isnan(sc[:2]).all()
    assert pos2[0].tolist() == pos2[1].tolist() == [-1, -1] and np.isnan(sc2[:2]).all()
    assert (pos[2:] >= 0).all() and not np.isnan(sc[2:]).any()
    smap, _ = MM.block_map(ref, img, mask, blocks[3], None, 4, 3)
    assert np.isnan(smap).any() and not np.isnan(smap).all()          # (NaN cells are skipped, not chosen)
    assert pos[3, 0] < 8 and not np.isnan(sc2[3])
    # method 0 has no NaN: only the empty mask gives none
    pos, sc = MM.match_blocks(ref, img, mask, blocks, 4, 0)
    assert pos[0].tolist() == [-1, -1] and np.isnan(sc[0]) and (pos[1:] >= 0).all() and not np.isnan(sc[1:]).any()
    # a map of NaNs and no map at all, directly
    nan = np.full((3, 4), np.nan, np.float32)
    assert MM.peaks(nan, 3)[0] is None and MM.peaks(None, 0, 2)[1][0] is None
    one = nan.copy()
    one[2, 1] = -0.0
    first, second = MM.peaks(one, 3, 0)
    assert first[0] == (2, 1) and first[1].tobytes() == np.float32(0.0).tobytes() and second[0] is None


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import build as mtm_build
    mtm_build.build()
    return _lib.load()


def test_header_declares_the_entry_point(lib):
    hdr = open(os.path.join(ROOT, "include", "mtm_hip.h")).read()
    assert "#define MTM_ABI_VERSION 9" in hdr and _lib.ABI_VERSION == 9 and lib.mtm_abi_version() == 9
    decl = re.search(r"int mtm_match_blocks_masked\(([^;]*)\);", hdr).group(1)
    assert len(decl.split(",")) == len(_lib.SYMBOLS["mtm_match_blocks_masked"][1]) == 20
    assert hasattr(_lib.Context, "match_blocks_masked") and "mask_fraction" in B.__all__


def test_bad_arguments_are_refused_without_a_gpu(lib):
    out = np.zeros(1, dtype=_lib.HIT_DTYPE)
    px = np.ones((8, 8), np.uint8)
    blk = _lib.block_records([(0, 0, 4, 4)])

    def call(ctx=None, mask=px.ctypes.data, stride=8, dtype=_lib.MTM_U8, method=3, exclusion=-1, second=None):
        return lib.mtm_match_blocks_masked(ctx, px.ctypes.data, 8, px.ctypes.data, 8, mask, stride, 8, 8, 1, dtype,
                                           blk.ctypes.data, 1, None, 2, method, exclusion, out.ctypes.data, None, second)

    assert call() == -1 and b"mtm_match_blocks_masked: bad arguments" in lib.mtm_last_error()      # (a NULL context)
    assert call(mask=None) == -1 and b"mask" in lib.mtm_last_error()
    assert call(dtype=_lib.MTM_U16) == -1 and b"dtype" in lib.mtm_last_error()
    for method in (1, 2, 4, 5, 6, -1):
        assert call(method=method) == -1 and b"method" in lib.mtm_last_error()
    assert call(stride=7) == -1 and b"mask_stride_bytes" in lib.mtm_last_error()
    # (that `second` is required with exclusion >= 0 is tested behind the context test, so only on a live context:
    #  tests/test_gpu_blocks_mask.py::test_second_is_required_with_an_exclusion)
    assert out["w"][0] == 0
