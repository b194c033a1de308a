"""The second correlation peak without a GPU: MTM.blocks.second_peaks and the host C the kernel shares
(mtm_debug_second_peaks without a context) against the brute-force rule of tests/blocks_second_model.py on constructed
maps, key_float_order against key_order_float through the host path, peak_ratio's branches, every argument error before any
native call, the Python layer's composition on the CPU oracle, and the C ABI's declarations."""
import os
import re

import numpy as np
import pytest

import MTM
import blocks_second_model as S
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


# ---- the rule on constructed maps ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_min", [0, 1])
@pytest.mark.parametrize("r", S.RADII)
def test_host_c_equals_the_brute_force(r, mode_min):
    maps = S.maps(r, mode_min, 100 * r + mode_min)
    method = 1 if mode_min else 5
    exp = [S.second_peak(m, method, r)[0] for m in maps]
    S.same_seconds(*_lib.debug_second_peaks(maps, mode_min, r), exp)
    assert any(np.isnan(s) for _, s in exp) and not all(np.isnan(s) for _, s in exp)
    # a first peak that is given, not found: the exclusion lies around it
    firsts = [(7 * k) % m.size for k, m in enumerate(maps)]
    exp = [S.second_peak(m, method, r, first=divmod(f, m.shape[1]))[0] for m, f in zip(maps, firsts)]
    S.same_seconds(*_lib.debug_second_peaks(maps, mode_min, r, firsts=firsts), exp)


@pytest.mark.parametrize("method", [1, 5])
@pytest.mark.parametrize("r", S.RADII)
def test_second_peaks_equals_the_brute_force_on_nan_padded_planes(r, method, no_native):
    mode_min = int(method in (0, 1))
    for smap in S.maps(r, mode_min, 7 + 100 * r + mode_min):
        plane, (oy, ox) = S.padded(smap)
        m = plane.shape[0] // 2
        block = (40, 30, 6, 5)
        ((sx, sy), s), (fx, fy) = S.second_peak(smap, method, r)
        # the model on the padded plane itself says the same: NaN cells are absent
        assert S.second_peak(plane, method, r)[0][0] == ((sx + ox, sy + oy) if sx >= 0 else (-1, -1))
        pos, sc = B.second_peaks(plane[None], [block], method, r)
        e_pos = (block[0] + sx + ox - m, block[1] + sy + oy - m) if sx >= 0 else (-1, -1)
        S.same_seconds(pos, sc, [(e_pos, s)])
        first, _ = B.plane_peaks(plane[None], np.array([block]), method)       # the first peak is plane_peaks' cell
        assert tuple(first[0]) == (block[0] + fx + ox - m, block[1] + fy + oy - m)


def test_all_equal_maps_take_the_first_cell_outside_the_exclusion():
    for mode_min in (0, 1):
        flat = np.full((5, 5), 0.5, dtype=np.float32)
        for r, exp in ((0, (1, 0)), (1, (2, 0)), (3, (4, 0)), (4, (-1, -1))):       # the first peak is cell (0, 0)
            pos, sc = _lib.debug_second_peaks([flat], mode_min, r)
            assert tuple(pos[0]) == exp and (np.isnan(sc[0]) if exp == (-1, -1) else sc[0] == np.float32(0.5))
        # the first peak at the centre: r = 1 leaves the border, whose first cell is (0, 0)
        pos, _ = _lib.debug_second_peaks([flat], mode_min, 1, firsts=[12])
        assert tuple(pos[0]) == (0, 0)
    pos, sc = B.second_peaks(np.full((1, 5, 5), 0.5), [(10, 20, 3, 3)], 5, 1)
    assert tuple(pos[0]) == (10 - 2 + 2, 20 - 2) and sc[0] == np.float32(0.5)


def test_zeros_of_either_sign_are_equal_and_come_back_as_plus_zero():
    z = np.array([[-0.0, 0.0, -0.0, 0.0, -0.0]], dtype=np.float32)
    for mode_min in (0, 1):
        pos, sc = _lib.debug_second_peaks([z], mode_min, 1)
        assert tuple(pos[0]) == (2, 0) and sc.view(np.uint32)[0] == 0              # +0, whatever the cell holds
    pos, sc = B.second_peaks(z.repeat(5, axis=0)[None], [(0, 0, 1, 1)], 1, 1)
    assert tuple(pos[0]) == (0, -2) and sc.view(np.uint32)[0] == 0


def test_order_word_round_trip():
    # key_order_float(key_float_order(v)) == v over a sweep of bit patterns, -0 -> +0: a 1 x 2 map whose second peak is its
    # cell 1 carries v through second_cell_key and back through quality_key_record
    rng = np.random.RandomState(3)
    bits = np.concatenate([np.array([0, 0x80000000, 1, 0x80000001, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x00800000,
                                     0x807FFFFF, 0x3F800000, 0xBF800000], dtype=np.uint32),
                           rng.randint(0, 2 ** 32, size=4000, dtype=np.uint64).astype(np.uint32)])
    v = bits.view(np.float32)
    v = v[~np.isnan(v)]
    maps = [np.array([[0.0, x]], dtype=np.float32) for x in v]
    exp = (v + np.float32(0.0)).view(np.uint32)
    for mode_min in (0, 1):
        pos, sc = _lib.debug_second_peaks(maps, mode_min, 0, firsts=[0] * len(maps))
        assert (pos == (1, 0)).all() and (sc.view(np.uint32) == exp).all()
    # and the order is the floats' order: of three cells the better of the two outside the exclusion wins
    a, b = v[:-1], v[1:]
    maps = [np.array([[0.0, x, y]], dtype=np.float32) for x, y in zip(a, b)]
    pos, _ = _lib.debug_second_peaks(maps, 0, 0, firsts=[0] * len(maps))
    assert (pos[:, 0] == np.where(b > a, 2, 1)).all()
    pos, _ = _lib.debug_second_peaks(maps, 1, 0, firsts=[0] * len(maps))
    assert (pos[:, 0] == np.where(b < a, 2, 1)).all()


def test_host_c_errors():
    one = [np.zeros((3, 3), np.float32)]
    for kw in (dict(mode_min=2, exclusion=0), dict(mode_min=0, exclusion=-1), dict(mode_min=0, exclusion=0, firsts=[9]),
               dict(mode_min=0, exclusion=0, firsts=[-1])):
        with pytest.raises(RuntimeError, match="mtm_debug_second_peaks: bad arguments"):
            _lib.debug_second_peaks(one, **kw)
    with pytest.raises(RuntimeError, match="mtm_debug_second_peaks: bad arguments"):
        _lib.debug_second_peaks([], 0, 0)
    lib = _lib.load()
    pair = (None, None, 0, None, 0, 8, 8, 1, 0)
    rec = np.zeros(1, dtype=_lib.HIT_DTYPE)
    for args in ((*pair, None, None, 0, 1, 5, None, None, -1, rec.ctypes.data), (*pair, None, None, 0, 1, 5, None, None, 2, None)):
        with pytest.raises(RuntimeError, match="mtm_match_blocks_second: bad arguments"):
            _lib.check(lib.mtm_match_blocks_second(*args), "second")
    for args in ((*pair, None, 1, 5, 2.0, 0.5, None, None, None, -1, rec.ctypes.data),
                 (*pair, None, 1, 5, 2.0, 0.5, None, None, None, 2, None)):
        with pytest.raises(RuntimeError, match="mtm_match_blocks_passes_second: bad arguments"):
            _lib.check(lib.mtm_match_blocks_passes_second(*args), "second")
    # threshold and epsilon are read only when there are flags to write
    flags = np.zeros(1, np.uint8)
    with pytest.raises(RuntimeError, match="mtm_match_blocks_passes_second: threshold must be finite and >= 0"):
        _lib.check(lib.mtm_match_blocks_passes_second(*pair, None, 1, 5, -1.0, 0.5, None, None, flags.ctypes.data, 2, None), "s")
    with pytest.raises(RuntimeError, match="mtm_match_blocks_passes_second: bad arguments"):
        _lib.check(lib.mtm_match_blocks_passes_second(*pair, None, 1, 5, -1.0, 0.5, None, None, None, 2, None), "s")


# ---- peak_ratio -------------------------------------------------------------------------------------------------------------
def test_peak_ratio_branches(no_native):
    nan, inf = np.nan, np.inf
    for method in (2, 3, 4, 5):
        got = B.peak_ratio(np.array([1.0, 0.5, 0.9, 0.9, 0.9, -0.5], np.float32),
                           np.array([0.5, 0.5, 0.0, -0.25, nan, 0.25], np.float32), method)
        assert got.dtype == np.float64 and got.shape == (6,)
        assert got[:2].tolist() == [2.0, 1.0] and got[2] == inf and got[3] == inf and np.isnan(got[4]) and got[5] == -2.0
    for method in (0, 1):
        got = B.peak_ratio(np.array([0.25, 0.5, 0.0, 0.0, 0.5], np.float32), np.array([0.5, 0.5, 0.75, nan, nan], np.float32),
                           method)
        assert got.dtype == np.float64
        assert got[:2].tolist() == [2.0, 1.0] and got[2] == inf and np.isnan(got[3]) and np.isnan(got[4])
    assert B.peak_ratio(np.zeros((2, 0)), np.zeros((2, 0)), 5).shape == (2, 0)
    assert B.peak_ratio(np.float32(0.75), np.float32(0.25), 5) == 3.0
    with pytest.raises(ValueError, match="peak_ratio: scores of shape"):
        B.peak_ratio(np.zeros(3), np.zeros(4), 5)
    with pytest.raises(ValueError, match="peak_ratio takes methods 0..5"):
        B.peak_ratio(np.zeros(3), np.zeros(3), 6)
    assert "normalised methods" in B.peak_ratio.__doc__
    for name in ("second_peaks", "peak_ratio"):
        assert name in B.__all__


# ---- argument errors come before any native call ----------------------------------------------------------------------------
def test_second_errors_come_before_any_native_call(no_native):
    u8 = np.zeros((40, 52), np.uint8)
    blocks = [(0, 0, 8, 8)]
    calls = (lambda **kw: MTM.matchBlocks(u8, u8, blocks, 2, **kw), lambda **kw: MTM.matchBlocksMultipass(u8, u8, [(16, 8, 2)], **kw))
    for call in calls:
        for bad in (False, np.True_, np.False_, 2.0, "2", (2,), [2], np.float32(1)):
            with pytest.raises(TypeError, match="second must be None, True or an integer exclusion radius"):
                call(second=bad)
        for bad in (-1, np.int64(-3)):
            with pytest.raises(ValueError, match="second: the exclusion radius must be >= 0"):
                call(second=bad)
        for good in (True, 0, 2, np.int32(5), 10 ** 12):
            with pytest.raises(_NativeCalled):
                call(second=good)
    # the calls' other errors stay what they are
    with pytest.raises(ValueError, match="margin must be an integer >= 0"):
        MTM.matchBlocks(u8, u8, blocks, -1, second=True)
    with pytest.raises(ValueError, match="is not inside"):
        MTM.matchBlocks(u8, u8, [(50, 0, 8, 8)], 2, second=True)
    # empty block lists: empty arrays of the right dtypes, the library untouched
    for refine in (False, True):
        pos, sc, pos2, sc2 = MTM.matchBlocks(u8, u8, [], 2, refine=refine, second=3)
        assert pos.shape == (0, 2) and pos.dtype == (np.float64 if refine else np.int64) and sc.dtype == np.float32
        assert pos2.shape == (0, 2) and pos2.dtype == np.int64 and sc2.shape == (0,) and sc2.dtype == np.float32
    assert len(MTM.matchBlocks(u8, u8, [], 2)) == 2
    pos2, sc2 = B.second_peaks(np.zeros((0, 5, 5), np.float32), [], 5)
    assert pos2.shape == (0, 2) and pos2.dtype == np.int64 and sc2.shape == (0,) and sc2.dtype == np.float32
    # second_peaks' own checks
    p = np.zeros((1, 5, 5), np.float32)
    for bad in (2.0, True, None, "1"):
        with pytest.raises(TypeError, match="second_peaks: exclusion must be an integer >= 0"):
            B.second_peaks(p, [(0, 0, 1, 1)], 5, bad)
    with pytest.raises(ValueError, match="second_peaks: exclusion must be an integer >= 0"):
        B.second_peaks(p, [(0, 0, 1, 1)], 5, -1)
    for bad in (np.zeros((1, 4, 4), np.float32), np.zeros((5, 5), np.float32), np.zeros((1, 5, 5), np.int32)):
        with pytest.raises(ValueError, match="planes must be an"):
            B.second_peaks(bad, [(0, 0, 1, 1)], 5)
    with pytest.raises(ValueError, match="one block per plane"):
        B.second_peaks(p, [(0, 0, 1, 1)] * 2, 5)
    with pytest.raises(ValueError, match=r"planes\[0\] holds no number"):
        B.second_peaks(np.full((1, 3, 3), np.nan, np.float32), [(0, 0, 1, 1)], 5)


# ---- the Python layer on the CPU oracle ---------------------------------------------------------------------------------
def _pair(seed, kind, hw=(40, 52), shift=(5, -3)):
    rng = np.random.RandomState(seed)
    top = 65536 if kind == "u16" else 256
    shape = hw + (3,) if kind == "rgb" else hw
    ref = rng.randint(0, top, size=shape).astype(np.uint16 if kind == "u16" else np.uint8)
    img = np.roll(ref, (shift[1], shift[0]), axis=(0, 1)).astype(np.int64) + rng.randint(-2, 3, size=shape)
    ref[8:24, 16:32] = 77
    return ref, np.clip(img, 0, top - 1).astype(ref.dtype)


_BLOCKS = [(0, 0, 8, 8), (44, 32, 8, 8), (20, 14, 9, 7), (16, 8, 16, 16), (30, 0, 12, 5)]
_OFFSETS = np.array([(0, 0), (5, -3), (100, 100), (-100, 2), (5, -3)])
_ORACLE_PASSES = [(16, 8, 4), ((8, 6), (9, 7), 2), (4, (12, 9), 0)]


@pytest.mark.parametrize("method", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("kind", ["u8", "rgb", "u16"])
def test_match_blocks_second_on_the_oracle(kind, method):
    import mtm_oracle as O
    ref, img = _pair(11, kind)
    for offsets, margin, r, refine in ((None, 3, True, False), (_OFFSETS, 4, 1, True), (_OFFSETS, 0, 0, False)):
        ctx = S.OracleCtx()
        got = MTM.matchBlocks(ref, img, _BLOCKS, margin, method, offsets=offsets, refine=refine, second=r, context=ctx)
        (tag, rec, off, m, meth, with_nbhd, radius), = ctx.calls            # one native call
        assert tag == "second" and m == margin and meth == method and with_nbhd is refine and radius == (2 if r is True else r)
        assert (off is None) == (offsets is None)
        plain = MTM.matchBlocks(ref, img, _BLOCKS, margin, method, offsets=offsets, refine=refine, context=S.OracleCtx())
        assert len(got) == 4 and len(plain) == 2
        assert got[0].dtype == plain[0].dtype and (got[0] == plain[0]).all() and got[1].tobytes() == plain[1].tobytes()
        first = MTM.matchBlocks(ref, img, _BLOCKS, margin, method, offsets=offsets, context=S.OracleCtx())[0]
        exp = S.expected_seconds(ref, img, _BLOCKS, offsets, margin, method, radius, O.compute_score_map, firsts=first)
        S.same_seconds(got[2], got[3], exp)             # (integers, with refine too)
        assert np.isnan(got[3]).all() == (margin == 0)


@pytest.mark.parametrize("method", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("kind", ["u8", "rgb", "u16"])
def test_multipass_second_on_the_oracle(kind, method):
    ref, img = _pair(12, kind)
    for validate, refine in ((None, False), ((2.0, 0.5), True)):
        ctx = S.OracleCtx()
        got = MTM.matchBlocksMultipass(ref, img, _ORACLE_PASSES, method, refine=refine, validate=validate, second=1, context=ctx)
        (tag, rec, counts, meth, with_nbhd, params, radius), = ctx.calls            # one native call
        assert tag == "passes_second" and meth == method and with_nbhd is refine and params == validate and radius == 1
        plain = MTM.matchBlocksMultipass(ref, img, _ORACLE_PASSES, method, refine=refine, validate=validate, context=S.OracleCtx())
        exp = S.V.by_hand(ref, img, _ORACLE_PASSES, method, *(validate or (None, None)), refine=refine, context=S.OracleCtx())
        assert len(got) == len(plain) == 3
        steer = None
        for p, (g, q, e) in enumerate(zip(got, plain, exp)):
            assert len(g) == len(q) + 2 == (6 if validate else 5)
            for a, b, c in zip(g[:-2], q, e):           # blocks, positions, scores and flags: the call without second
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes() == c.tobytes()
            # the second peaks: matchBlocks(offsets=, second=) of the by-hand loop
            block, step, margin = _ORACLE_PASSES[p]
            off = None if p == 0 else B.predict_offsets(img.shape, _ORACLE_PASSES[p - 1][:2], steer, _ORACLE_PASSES[p][:2])
            pos, _, pos2, sc2 = MTM.matchBlocks(ref, img, g[0], margin, method, offsets=off, second=1, context=S.OracleCtx())
            assert (g[-2] == pos2).all() and g[-2].dtype == np.int64 and g[-1].dtype == np.float32
            assert g[-1].tobytes() == sc2.tobytes()
            steer = pos
            if validate:
                _, rep = B.validate(B.grid_shape(img.shape, block, step), B.displacements(g[0], pos), *validate)
                steer = g[0][:, :2] + rep
        assert np.isnan(got[2][-1]).all() and not np.isnan(got[0][-1]).any()        # margin 0: no second peak; margin 4: one


def test_second_none_is_the_call_as_it_was():
    ref, img = _pair(4, "u8")
    ctx = S.M.OracleCtx()       # (the contexts as they were: their calls take no `second`)
    got = MTM.matchBlocks(ref, img, _BLOCKS, 3, 5, offsets=_OFFSETS, second=None, context=ctx)
    plain = MTM.matchBlocks(ref, img, _BLOCKS, 3, 5, second=None, context=ctx)
    assert [c[0] for c in ctx.calls] == ["at", "plain"] and len(got) == 2 and len(plain) == 2
    got = MTM.matchBlocksMultipass(ref, img, _ORACLE_PASSES, 5, second=None, context=ctx)
    assert ctx.calls[-1][0] == "passes" and all(len(t) == 3 for t in got)
    vctx = S.V.OracleCtx()
    got = MTM.matchBlocksMultipass(ref, img, _ORACLE_PASSES, 5, validate=True, second=None, context=vctx)
    assert vctx.calls[-1][0] == "validated" and all(len(t) == 4 for t in got)


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_abi_symbols():
    hdr = open(os.path.join(ROOT, "include", "mtm_hip.h")).read()
    assert re.search(r"#define MTM_ABI_VERSION 9\b", hdr) and _lib.load().mtm_abi_version() == 9
    since = re.search(r"Entry points added since 9 - (.*?) - are new symbols only", hdr, re.S).group(1)
    for name, n_args in (("mtm_match_blocks_second", 18), ("mtm_match_blocks_passes_second", 19), ("mtm_debug_second_peaks", 9),
                         ("mtm_match_blocks_at", 16), ("mtm_match_blocks_passes_validated", 17)):
        assert name in _lib.SYMBOLS and name in since
        decl = re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[name][1]) == n_args
        assert getattr(_lib.load(), name) is not None
