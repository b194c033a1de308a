"""MTM.blocks.validate / grid_shape and MTM.matchBlocksMultipass(validate=) without a GPU: the numpy rule against a
brute-force restatement in Python integers (tests/blocks_validate_model.py), the host C that the kernel shares
(mtm_debug_validate_blocks without a context) against the numpy rule, the Python layer's composition on the CPU oracle
against the by-hand loop it documents, the scene with one flat coarse block that validation repairs, every argument error
before any native call, and the C ABI's declarations."""
import os
import re

import numpy as np
import pytest

import MTM
import blocks_validate_model as V
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


# ---- the rule -------------------------------------------------------------------------------------------------------------
def test_grid_shape():
    for shape, block, step in (((166, 230), 32, 64), ((166, 230), 16, 16), ((40, 52), (8, 6), (5, 7)), ((40, 52), 16, None),
                               ((10, 10), 11, None)):
        ny, nx = B.grid_shape(shape, block, step)
        g = B.grid(shape, block, step)
        assert ny * nx == len(g)
        if len(g):
            assert (ny, nx) == (len(np.unique(g[:, 1])), len(np.unique(g[:, 0])))
    assert B.grid_shape((166, 230), 32, 64) == (3, 4)


@pytest.mark.parametrize("grid_shape", V.GRIDS, ids=lambda g: "%dx%d" % g)
def test_validate_against_brute_force(grid_shape, no_native):
    ny, nx = grid_shape
    seen = {"flagged": 0, "kept": 0}
    for f, field in enumerate(V.fields(grid_shape, 11 * ny + nx)):
        for threshold, epsilon in V.PARAMS:
            valid, rep = B.validate(grid_shape, field, threshold, epsilon)
            e_valid, e_rep = V.validate_brute(grid_shape, field, threshold, epsilon)
            assert valid.dtype == bool and valid.shape == (ny * nx,) and rep.dtype == np.int64 and rep.shape == (ny * nx, 2)
            assert valid.tolist() == e_valid and [tuple(r) for r in rep.tolist()] == e_rep, (f, threshold, epsilon)
            assert (rep[valid] == field[valid]).all()
            seen["flagged"] += int((~valid).sum())
            seen["kept"] += int(valid.sum())
    if min(ny, nx) == 1 or ny * nx < 4:         # fewer than 3 neighbours everywhere: nothing is ever flagged
        assert seen["flagged"] == 0
    else:
        assert seen["flagged"] > 0 and seen["kept"] > 0
    # the default parameters
    field = V.fields(grid_shape, 3)[-3]
    assert B.validate(grid_shape, field)[0].tolist() == V.validate_brute(grid_shape, field, 2.0, 0.5)[0]


def test_validate_defaults_on_a_uniform_neighbourhood():
    # rm4 = 0: a deviation of 1 px passes (4 > 4 is false), 2 px is flagged and replaced by the median
    for dev, ok in ((1, True), (-1, True), (2, False), (-2, False)):
        f = np.zeros((9, 2), np.int64)
        f[4] = (dev, 0)
        valid, rep = B.validate((3, 3), f)
        assert valid[4] == ok and valid.sum() == 8 + ok and tuple(rep[4]) == ((dev, 0) if ok else (0, 0))
    # a sub-pixel epsilon flags every 1-px step
    f = np.zeros((9, 2), np.int64)
    f[4] = (0, 1)
    assert not B.validate((3, 3), f, 2.0, 0.1)[0][4]
    # a 1 x n grid: nobody has three neighbours
    valid, rep = B.validate((1, 4), np.array([[0, 0], [50, 50], [0, 0], [0, 0]]))
    assert valid.all() and tuple(rep[1]) == (50, 50)
    # 2 x 2: block 0 has the three neighbours (0, -1), (1, 0), (0, 0): medians 0 and 0
    valid, rep = B.validate((2, 2), np.array([[9, 9], [0, -1], [1, 0], [0, 0]]))
    assert not valid[0] and tuple(rep[0]) == (0, 0)
    # an even count rounds half towards +infinity: eight neighbours with dx 0 0 0 0 1 1 1 1 (doubled median 1 -> 1) and
    # dy -1 -1 -1 -1 0 0 0 0 (doubled median -1 -> 0)
    f = np.array([[0, -1], [0, -1], [0, -1], [0, -1], [9, 9], [1, 0], [1, 0], [1, 0], [1, 0]])
    valid, rep = B.validate((3, 3), f)
    assert not valid[4] and tuple(rep[4]) == (1, 0)
    # five neighbours, an odd count: block 1 of a 2 x 3 grid - dx 0 0 1 5 1 (median 1), dy -1 -1 0 -7 0 (median -1)
    valid, rep = B.validate((2, 3), np.array([[0, -1], [9, 9], [0, -1], [1, 0], [5, -7], [1, 0]]))
    assert not valid[1] and tuple(rep[1]) == (1, -1)


def test_validate_errors(no_native):
    z = np.zeros((6, 2), np.int64)
    with pytest.raises(TypeError, match="displacements must be integers"):
        B.validate((2, 3), z.astype(np.float64))
    with pytest.raises(TypeError, match="displacements must be integers"):
        B.validate((2, 3), z.astype(bool))
    for bad in (z[:5], z.reshape(-1), z.reshape(2, 3, 2), np.zeros((6, 3), np.int64)):
        with pytest.raises(ValueError, match="displacements of shape"):
            B.validate((2, 3), bad)
    for bad in ((2,), 6, (2, 3, 1), (2.0, 3), (-2, -3), None):
        with pytest.raises(ValueError, match="grid_shape must be"):
            B.validate(bad, z)
    for bad in (-1, float("nan"), float("inf"), -0.5, None, "2", True):
        with pytest.raises(ValueError, match="threshold must be a finite number >= 0"):
            B.validate((2, 3), z, bad)
        with pytest.raises(ValueError, match="epsilon must be a finite number >= 0"):
            B.validate((2, 3), z, 2.0, bad)
    valid, rep = B.validate((0, 0), np.zeros((0, 2), np.int32))
    assert valid.shape == (0,) and rep.shape == (0, 2) and rep.dtype == np.int64
    assert B.validate((2, 3), z.astype(np.uint8))[1].dtype == np.int64
    for name in ("grid_shape", "validate"):
        assert name in B.__all__


# ---- the host C the kernel shares -------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid_shape", V.GRIDS, ids=lambda g: "%dx%d" % g)
def test_host_c_equals_validate(grid_shape):
    ny, nx = grid_shape
    g = np.stack((np.tile(np.arange(nx), ny), np.repeat(np.arange(ny), nx)), axis=1).astype(np.int64)
    for f, field in enumerate(V.fields(grid_shape, 11 * ny + nx)):
        step = ((16, 16), (5, 7), (1, 3))[f % 3]
        at = g * np.array(step)
        for threshold, epsilon in V.PARAMS:
            e_valid, e_rep = B.validate(grid_shape, field, threshold, epsilon)
            valid, steer = _lib.debug_validate_blocks(at + field, grid_shape, step, threshold, epsilon)
            assert valid.dtype == bool and np.array_equal(valid, e_valid), (f, threshold, epsilon)
            assert steer.dtype == np.int64 and np.array_equal(steer, at + e_rep), (f, threshold, epsilon)


def test_host_c_errors():
    pos = np.zeros((6, 2), np.int64)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="mtm_debug_validate_blocks: threshold must be finite and >= 0"):
            _lib.debug_validate_blocks(pos, (2, 3), (4, 4), bad, 0.5)
        with pytest.raises(RuntimeError, match="mtm_debug_validate_blocks: epsilon must be finite and >= 0"):
            _lib.debug_validate_blocks(pos, (2, 3), (4, 4), 2.0, bad)
    with pytest.raises(RuntimeError, match="bad arguments"):
        _lib.debug_validate_blocks(pos, (2, 3), (0, 4))
    with pytest.raises(ValueError, match="5 positions for a grid of 2 x 3"):
        _lib.debug_validate_blocks(pos[:5], (2, 3), (4, 4))


def test_validated_call_names_a_bad_threshold_or_epsilon():
    lib = _lib.load()
    none = (None, None, 0, None, 0, 8, 8, 1, 0, None, 1, 5)
    for thr, eps, name in ((-1.0, 0.5, "threshold"), (float("nan"), 0.5, "threshold"), (2.0, float("inf"), "epsilon"),
                           (2.0, -0.25, "epsilon")):
        with pytest.raises(RuntimeError, match="mtm_match_blocks_passes_validated: %s must be finite and >= 0" % name):
            _lib.check(lib.mtm_match_blocks_passes_validated(*none, thr, eps, None, None, None), "validated")
    with pytest.raises(RuntimeError, match="mtm_match_blocks_passes_validated: bad arguments"):
        _lib.check(lib.mtm_match_blocks_passes_validated(*none, 2.0, 0.5, None, None, None), "validated")


# ---- the Python layer on the CPU oracle ---------------------------------------------------------------------------------
def _pair(seed, kind, hw=(40, 52), shift=(5, -3)):
    """A reference and an image moved by `shift` with a little noise; a flat patch over coarse block (1, 2) of the 16 / 8 grid."""
    rng = np.random.RandomState(seed)
    top = 65536 if kind == "u16" else 256
    shape = hw + (3,) if kind == "rgb" else hw
    ref = rng.randint(0, top, size=shape).astype(np.uint16 if kind == "u16" else np.uint8)
    img = np.roll(ref, (shift[1], shift[0]), axis=(0, 1)).astype(np.int64) + rng.randint(-2, 3, size=shape)
    ref[8:24, 16:32] = 77
    return ref, np.clip(img, 0, top - 1).astype(ref.dtype)


_ORACLE_PASSES = [(16, 8, 6), ((8, 6), (5, 7), 2), (4, None, 0)]


@pytest.mark.parametrize("method", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("kind", ["u8", "rgb", "u16"])
def test_validated_composition_on_the_oracle(kind, method):
    ref, img = _pair(3, kind)
    for refine in (False, True):
        ctx = V.OracleCtx()
        got = MTM.matchBlocksMultipass(ref, img, _ORACLE_PASSES, method, refine=refine, context=ctx, validate=(2.0, 0.5))
        (tag, rec, counts, m, with_nbhd, params), = ctx.calls            # one native call
        assert tag == "validated" and m == method and with_nbhd is refine and params == (2.0, 0.5)
        assert rec.tolist() == [(16, 16, 8, 8, 6), (8, 6, 5, 7, 2), (4, 4, 4, 4, 0)]
        exp = V.by_hand(ref, img, _ORACLE_PASSES, method, 2.0, 0.5, refine, V.OracleCtx())
        assert len(got) == len(exp) == 3
        for (gb, gp, gs, gv), (eb, ep, es, ev) in zip(got, exp):
            assert gb.dtype == np.int64 and (gb == eb).all()
            assert gp.dtype == ep.dtype == (np.float64 if refine else np.int64) and (gp == ep).all()
            assert gs.dtype == np.float32 and gs.tobytes() == es.tobytes()
            assert gv.dtype == bool and gv.shape == (len(gb),) and (gv == ev).all()
    if method == 5:     # the flat coarse block lands on its box's first output and is flagged: validation is at work
        assert not got[0][3][1 * 5 + 2] and not got[0][3].all()
    # validate=True is (2.0, 0.5)
    ctx = V.OracleCtx()
    MTM.matchBlocksMultipass(ref, img, _ORACLE_PASSES[:1], method, context=ctx, validate=True)
    assert ctx.calls[0][0] == "validated" and ctx.calls[0][5] == (2.0, 0.5)


def test_validation_repairs_the_flat_coarse_block():
    ref, img = V.scene()
    val = MTM.matchBlocksMultipass(ref, img, V.SCENE_PASSES, 5, context=V.OracleCtx(), validate=True)
    raw = MTM.matchBlocksMultipass(ref, img, V.SCENE_PASSES, 5, context=V.OracleCtx())
    blocks0, pos0, _, valid0 = val[0]
    assert B.grid_shape(img.shape, 32, 64) == (3, 4) and tuple(blocks0[5]) == (64, 64, 32, 32)
    assert tuple(B.displacements(blocks0, pos0)[5]) == (-16, -16)          # the flat block: its box's first output
    assert valid0.tolist() == [k != 5 for k in range(12)]                   # pass 0 flags exactly the flat block
    assert (pos0 == raw[0][1]).all()                                        # the returned positions stay the raw ones
    blocks1, pos1, _, valid1 = val[1]
    out = V.outside_patch(blocks1)
    assert len(blocks1) == 140 and out.sum() == 136 and valid1.shape == (140,)
    found_val = int((B.displacements(blocks1, pos1)[out] == V.SCENE_SHIFT).all(axis=1).sum())
    found_raw = int((B.displacements(raw[1][0], raw[1][1])[out] == V.SCENE_SHIFT).all(axis=1).sum())
    print("found validated %d, unvalidated %d of %d" % (found_val, found_raw, out.sum()))
    assert found_val == 136 and found_raw < found_val


def test_validate_none_is_the_call_as_it_was():
    ref, img = _pair(4, "u8")
    ctx = V.M.OracleCtx()       # (the context as it was: its match_blocks_passes takes no `validate`)
    got = MTM.matchBlocksMultipass(ref, img, _ORACLE_PASSES, 5, context=ctx, validate=None)
    again = MTM.matchBlocksMultipass(ref, img, _ORACLE_PASSES, 5, context=V.M.OracleCtx())
    (tag, _, counts, m, with_nbhd), = ctx.calls
    assert tag == "passes" and m == 5 and with_nbhd is False
    assert all(len(t) == 3 for t in got) and len(got) == 3
    for (gb, gp, gs), (eb, ep, es) in zip(got, again):
        assert (gb == eb).all() and (gp == ep).all() and gs.tobytes() == es.tobytes()


def test_validate_errors_come_before_any_native_call(no_native):
    u8 = np.zeros((40, 52), np.uint8)
    ok = [(16, 8, 2)]
    for bad in (False, 2.0, (2.0,), (2.0, 0.5, 1.0), "ab", [], 0, np.True_):
        with pytest.raises(ValueError, match=r"validate must be None, True or \(threshold, epsilon\)"):
            MTM.matchBlocksMultipass(u8, u8, ok, validate=bad)
    for bad in (-1, float("nan"), float("inf"), None, "2", True):
        with pytest.raises(ValueError, match="validate: threshold must be a finite number >= 0"):
            MTM.matchBlocksMultipass(u8, u8, ok, validate=(bad, 0.5))
        with pytest.raises(ValueError, match="validate: epsilon must be a finite number >= 0"):
            MTM.matchBlocksMultipass(u8, u8, ok, validate=(2.0, bad))
    # the call's other errors still come first or after, never a native call
    with pytest.raises(ValueError, match="uint8 images with 1 or 3 channels"):
        MTM.matchBlocksMultipass(u8.astype(np.float32), u8.astype(np.float32), ok, validate=True)
    with pytest.raises(ValueError, match=r"passes\[0\]: margin must be an integer >= 0"):
        MTM.matchBlocksMultipass(u8, u8, [(16, 8, -1)], validate=True)
    for good in (True, (2.0, 0.5), [0, 0], (np.float32(1.5), np.int64(2))):
        with pytest.raises(_NativeCalled):
            MTM.matchBlocksMultipass(u8, u8, ok, validate=good)


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_abi_symbols():
    hdr = open(os.path.join(ROOT, "include", "mtm_hip.h")).read()
    assert re.search(r"#define MTM_ABI_VERSION 9\b", hdr) and _lib.load().mtm_abi_version() == 9
    since = re.search(r"Entry points added since 9 - (.*?) - are new symbols only", hdr, re.S).group(1)
    for name, n_args in (("mtm_match_blocks_passes_validated", 17), ("mtm_debug_validate_blocks", 10),
                         ("mtm_match_blocks_passes", 14)):
        assert name in _lib.SYMBOLS and name in since
        decl = re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[name][1]) == n_args
        assert getattr(_lib.load(), name) is not None
