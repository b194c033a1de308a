"""MTM.blocks.displacement_field / field_at / deform and MTM.matchBlocksMultipass(deform=True) without a GPU: the numpy rule
against a brute-force restatement in Python integers (tests/blocks_deform_model.py), the host C that the kernel shares
(mtm_deform_image without a context) against the numpy rule, the Python layer's composition on the CPU oracle against the
by-hand loop it documents, the sheared pair that deformation exists for, every argument error before any native call, and
the C ABI's declarations."""
import os
import re

import numpy as np
import pytest

import MTM
import blocks_deform_model as D
from MTM import _lib
from MTM import blocks as B

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_IDS = ["1x1", "1xn", "nx1", "3x4", "5x7"]


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
def test_the_grids_are_the_ones_named():
    assert tuple(D.grid_counts(s, c) for s, c in D.GRIDS) == D.GRID_COUNTS
    for (shape, coarse), (nx, ny) in zip(D.GRIDS, D.GRID_COUNTS):
        assert B.grid_shape(shape, *coarse) == (ny, nx)


@pytest.mark.parametrize("shape, coarse", D.GRIDS, ids=_IDS)
def test_field_and_warp_against_brute_force(shape, coarse, no_native):
    fine = B.grid(shape, (5, 4), (3, 6))
    assert len(fine) > 1
    imgs = {k: D.image(shape, k, 7) for k in ("u8", "rgb", "u16")}
    assert imgs["u16"].max() == 65535 and imgs["u16"].min() == 0
    for f, disp in enumerate(D.fields(shape, coarse, 5)):
        field = B.displacement_field(shape, coarse, disp)
        assert field.dtype == np.int64 and field.shape == tuple(shape) + (2,)
        assert np.array_equal(field, D.field_brute(shape, coarse, disp)), f
        at = B.field_at(shape, coarse, disp, fine)
        assert at.dtype == np.int64 and np.array_equal(at, D.field_at_brute(shape, coarse, disp, fine)), f
        for kind, img in imgs.items():
            out = B.deform(img, field)
            assert out.dtype == img.dtype and out.shape == img.shape
            if f != 1 or kind == "u8":          # (the brute-force warp of one constant field per kind is enough)
                assert np.array_equal(out, D.deform_brute(img, field)), (f, kind)
            if f == 0:                          # a zero field: the image
                assert np.array_equal(out, img)
            if f in (1, 2):                     # an integer constant field: the shifted image, edges replicated
                dx, dy = (int(v) for v in disp[0])
                H, W = shape
                ys = np.clip(np.arange(H) + dy, 0, H - 1)
                xs = np.clip(np.arange(W) + dx, 0, W - 1)
                assert (field == 256 * disp[0]).all() and np.array_equal(out, img[ys][:, xs]), (f, kind)


def test_the_floor_shift_and_the_clamps():
    shape, coarse = D.GRIDS[3]
    neg = D.fields(shape, coarse, 5)[3]
    field = B.displacement_field(shape, coarse, neg)
    assert (neg < 0).all() and (field < 0).all() and (field % 256 != 0).any()       # fractional and negative: a floor
    # one node at -1, the others 0: -1 px at the node, and between the nodes every value of (-1, 0] px
    one = np.zeros_like(neg)
    one[0] = (-1, -1)
    f = B.displacement_field(shape, coarse, one)
    assert f.min() == -256 and set(np.unique(f)) <= set(range(-256, 1)) and len(np.unique(f)) > 20
    # every sample clamps: the far corner's pixel everywhere
    img = D.image(shape, "rgb", 2)
    out = B.deform(img, B.displacement_field(shape, coarse, np.full_like(neg, 10 ** 4)))
    assert (out == img[-1, -1]).all()
    out = B.deform(img, B.displacement_field(shape, coarse, np.full_like(neg, -10 ** 4)))
    assert (out == img[0, 0]).all()


def test_field_errors(no_native):
    shape, coarse = D.GRIDS[3]
    n = 12
    ok = np.zeros((n, 2), np.int64)
    for fn in (lambda d, c=coarse: B.displacement_field(shape, c, d), lambda d, c=coarse: B.field_at(shape, c, d, B.grid(shape, 4)),
               lambda d, c=coarse: MTM.deformImage(np.zeros(shape, np.uint8), c, d)):
        with pytest.raises(TypeError, match="displacements must be integers"):
            fn(ok.astype(np.float64))
        for bad in (ok[:-1], ok.reshape(-1), np.zeros((n, 3), np.int64)):
            with pytest.raises(ValueError, match="displacements of shape"):
                fn(bad)
        with pytest.raises(ValueError, match="beyond 2\\^22"):
            fn(ok + (1 << 22) + 1)
        with pytest.raises(ValueError, match="coarse is a \\(block, step\\) pair"):
            fn(ok, 5)
    with pytest.raises(ValueError, match="the coarse grid is empty"):
        B.displacement_field(shape, (64, 64), np.zeros((0, 2), np.int64))
    with pytest.raises(ValueError, match="a field of shape"):
        B.deform(np.zeros(shape, np.uint8), np.zeros(shape + (3,), np.int64))
    with pytest.raises(TypeError, match="the field must be integers"):
        B.deform(np.zeros(shape, np.uint8), np.zeros(shape + (2,), np.float64))
    with pytest.raises(ValueError, match="uint8 or uint16"):
        B.deform(np.zeros(shape, np.float32), np.zeros(shape + (2,), np.int64))
    with pytest.raises(TypeError, match="image must be a numpy array"):
        MTM.deformImage([[1]], coarse, ok)
    with pytest.raises(ValueError, match="deformImage takes uint8 images"):
        MTM.deformImage(np.zeros(shape, np.float32), coarse, ok)
    with pytest.raises(_NativeCalled):
        MTM.deformImage(np.zeros(shape, np.uint8), coarse, ok)


# ---- the host C the kernel shares -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, coarse", D.GRIDS, ids=_IDS)
def test_host_c_equals_numpy(shape, coarse):
    (bw, bh), (sx, sy) = coarse
    for kind in ("u8", "rgb", "u16"):
        img = D.image(shape, kind, 9)
        for f, disp in enumerate(D.fields(shape, coarse, 6)):
            out = _lib.deform_image(img, (bw, bh, sx, sy), disp)
            assert out.dtype == img.dtype and np.array_equal(out, B.deform(img, B.displacement_field(shape, coarse, disp))), (kind, f)
    # a strided image (rows of a wider array) and the largest displacements
    wide = D.image((shape[0], shape[1] + 5), "u8", 1)
    view = wide[:, 2:2 + shape[1]]
    nx, ny = D.grid_counts(shape, coarse)
    disp = np.full((nx * ny, 2), 1 << 22, np.int64)
    disp[::2] = -(1 << 22)
    assert np.array_equal(_lib.deform_image(view, (bw, bh, sx, sy), disp),
                          B.deform(view, B.displacement_field(shape, coarse, disp)))


def test_host_c_errors():
    img = np.zeros((20, 30), np.uint8)
    ok = np.zeros((6, 2), np.int32)             # 3 x 2 blocks of 10 x 10
    with pytest.raises(_lib.MtmError, match="displacement beyond 2\\^22"):
        _lib.deform_image(img, (10, 10, 10, 10), ok + (1 << 22) + 1)
    with pytest.raises(_lib.MtmError, match="a block must fit the image"):
        _lib.deform_image(img, (40, 10, 10, 10), ok)
    with pytest.raises(_lib.MtmError, match="block and step must be >= 1"):
        _lib.deform_image(img, (10, 10, 0, 10), ok)
    with pytest.raises(_lib.MtmError, match="uint8 images with 1 or 3 channels"):
        _lib.deform_image(np.zeros((20, 30, 2), np.uint8), (10, 10, 10, 10), ok)
    with pytest.raises(_lib.MtmError, match="bad arguments"):
        _lib.check(_lib.load().mtm_deform_image(None, img.ctypes.data, 30, 20, 30, 1, _lib.MTM_U8, 10, 10, 10, 10, None,
                                                img.ctypes.data, 30))


# ---- the Python layer on the oracle ---------------------------------------------------------------------------------------
def _pair(seed, kind, shift=(2, -1), hw=(40, 52)):
    """A smooth reference and the same texture moved by `shift` with a little noise."""
    rng = np.random.RandomState(seed)
    top = 65535 if kind == "u16" else 255
    ref = D.smooth_texture(hw, seed, kind)
    img = np.roll(ref, (shift[1], shift[0]), axis=(0, 1)).astype(np.int64) + rng.randint(-2, 3, size=ref.shape)
    return ref, np.clip(img, 0, top).astype(ref.dtype)


_ORACLE_PASSES = [(16, 8, 4), ((8, 6), (5, 7), 2)]


def _same(got, exp, refine, n):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert len(g) == len(e) == n
        assert g[0].dtype == np.int64 and (g[0] == e[0]).all()
        assert g[1].dtype == e[1].dtype == (np.float64 if refine else np.int64) and (g[1] == e[1]).all()
        assert g[2].dtype == np.float32 and g[2].tobytes() == e[2].tobytes()
        if n == 5:
            assert g[3].dtype == bool and g[3].shape == (len(g[0]),) and (g[3] == e[3]).all()
        assert g[-1].dtype == np.float64 and g[-1].shape == (len(g[0]), 2) and (g[-1] == e[-1]).all()


@pytest.mark.parametrize("method", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("kind", ["u8", "rgb", "u16"])
def test_deformed_composition_on_the_oracle(kind, method):
    ref, img = _pair(3, kind)
    for refine in (False, True):
        for validate in (None, (1.0, 0.0)):
            ctx = D.OracleCtx()
            got = MTM.matchBlocksMultipass(ref, img, _ORACLE_PASSES, method, refine=refine, context=ctx, validate=validate,
                                           deform=True)
            (tag, rec, counts, m, with_nbhd, params), = ctx.calls            # one native call
            assert tag == "deformed" and m == method and with_nbhd is refine and params == validate
            assert rec.tolist() == [(16, 16, 8, 8, 4), (8, 6, 5, 7, 2)]
            # the loop of the docstring: numpy field and warp, matchBlocks on the plain oracle
            exp = D.by_hand(ref, img, _ORACLE_PASSES, method, validate, refine, D.V.M.OracleCtx())
            _same(got, exp, refine, 4 if validate is None else 5)
            assert (got[0][-1] == 0).all()
    assert (got[1][-1] != 0).any()              # the second pass did carry a field


def test_deform_false_is_the_call_as_it_was():
    ref, img = _pair(4, "u8")
    ctx = D.V.M.OracleCtx()         # (the context as it was: its match_blocks_passes takes no `deform`)
    got = MTM.matchBlocksMultipass(ref, img, _ORACLE_PASSES, 5, context=ctx, deform=False)
    again = MTM.matchBlocksMultipass(ref, img, _ORACLE_PASSES, 5, context=D.V.M.OracleCtx())
    (tag, _, counts, m, with_nbhd), = ctx.calls
    assert tag == "passes" and m == 5 and with_nbhd is False
    assert all(len(t) == 3 for t in got) and len(got) == 2
    for (gb, gp, gs), (eb, ep, es) in zip(got, again):
        assert (gb == eb).all() and gp.dtype == ep.dtype and (gp == ep).all() and gs.tobytes() == es.tobytes()
    vctx = D.V.OracleCtx()          # (... and with validate: no `deform` reaches the context either)
    val = MTM.matchBlocksMultipass(ref, img, _ORACLE_PASSES, 5, context=vctx, validate=True, deform=False)
    assert vctx.calls[0][0] == "validated" and all(len(t) == 4 for t in val)


def test_a_single_deformed_pass_is_the_plain_call():
    ref, img = _pair(5, "rgb")
    for refine in (False, True):
        got, = MTM.matchBlocksMultipass(ref, img, _ORACLE_PASSES[:1], 3, refine=refine, context=D.OracleCtx(), deform=True)
        pos, sc = MTM.matchBlocks(ref, img, B.grid(img.shape, 16, 8), 4, 3, refine=refine, context=D.V.M.OracleCtx())
        assert len(got) == 4 and got[1].dtype == pos.dtype and (got[1] == pos).all() and got[2].tobytes() == sc.tobytes()
        assert (got[3] == 0).all() and got[3].shape == (len(pos), 2)


def test_deformation_sharpens_the_peak_under_shear():
    """The prototype's pair: 160 x 192, sheared by 0.12 px per row, 32 x 32 blocks, coarse stride 32, fine stride 16."""
    ref, img = D.sheared_pair()
    passes = [(32, 32, 12), (32, 16, 2)]
    plain = MTM.matchBlocksMultipass(ref, img, passes, 5, context=D.OracleCtx())
    bent = MTM.matchBlocksMultipass(ref, img, passes, 5, context=D.OracleCtx(), deform=True)
    inner = D.interior(plain[1][0], img.shape, 16)
    assert inner.sum() >= 20
    s_plain, s_bent = float(plain[1][2][inner].mean()), float(bent[1][2][inner].mean())
    print("mean last-pass score over %d interior blocks: rigid %.4f, deformed %.4f" % (inner.sum(), s_plain, s_bent))
    assert s_bent > s_plain
    # the field the coarse pass measured is the shear: dx = 0.12 (y - H / 2) at the fine blocks' centres, to a pixel - away
    # from the coarse blocks of the first and last column, which cannot follow a displacement that leaves the image
    b, pred = bent[1][0], bent[1][3]
    mid = D.interior(b, img.shape, 32)
    want = 0.12 * (b[:, 1] + 15.5 - 80.0)
    assert mid.sum() >= 20 and np.abs(pred[mid, 0] - want[mid]).max() <= 1.0 and np.abs(pred[mid, 1]).max() <= 1.0


# ---- the argument errors --------------------------------------------------------------------------------------------------
def test_deform_errors_come_before_any_native_call(no_native):
    u8 = np.zeros((40, 52), np.uint8)
    ok = [(16, 8, 2), (8, 8, 1)]
    for bad in (1, 0, None, "yes", np.True_):
        with pytest.raises(ValueError, match="deform must be True or False"):
            MTM.matchBlocksMultipass(u8, u8, ok, deform=bad)
    for second in (True, 0, 3):
        with pytest.raises(ValueError, match="deform=True does not go with second="):
            MTM.matchBlocksMultipass(u8, u8, ok, deform=True, second=second)
    with pytest.raises(ValueError, match=r"len\(passes\) \* max\(H, W\) of at most 2\^22"):
        wide = np.zeros((4, 1 << 21), np.uint8)
        MTM.matchBlocksMultipass(wide, wide, [(4, 4, 0)] * 3, deform=True)
    with pytest.raises(ValueError, match="uint8 images with 1 or 3 channels"):
        MTM.matchBlocksMultipass(u8.astype(np.float32), u8.astype(np.float32), ok, deform=True)
    with pytest.raises(ValueError, match=r"passes\[1\]: margin must be an integer >= 0"):
        MTM.matchBlocksMultipass(u8, u8, [(16, 8, 1), (8, 8, -1)], deform=True)
    with pytest.raises(ValueError, match="validate must be None, True or"):
        MTM.matchBlocksMultipass(u8, u8, ok, deform=True, validate=2.0)
    for kw in ({}, {"validate": True}, {"refine": True}):
        with pytest.raises(_NativeCalled):
            MTM.matchBlocksMultipass(u8, u8, ok, deform=True, **kw)


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_abi_symbols():
    hdr = open(os.path.join(ROOT, "include", "mtm_hip.h")).read()
    assert re.search(r"#define MTM_ABI_VERSION 9\b", hdr) and _lib.load().mtm_abi_version() == 9
    since = re.search(r"Entry points added since 9 - (.*?) - are new symbols only", hdr, re.S).group(1)
    for name, n_args in (("mtm_match_blocks_passes_deformed", 18), ("mtm_deform_image", 14)):
        assert name in _lib.SYMBOLS and name in since
        decl = re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[name][1]) == n_args
        assert getattr(_lib.load(), name) is not None
    assert "deformImage" in MTM.__all__ and MTM.deformImage is B.deformImage
    assert {"displacement_field", "field_at", "deform", "deformImage"} <= set(B.__all__)
