"""MTM.blocks.to_q8 / smooth_displacements, the Q8 field and MTM.matchBlocksMultipass(deform=True, steer="refined") without a
GPU: the numpy rule against brute force in Python numbers (tests/blocks_steer_model.py), the host C that the kernels share
(mtm_deform_image_q8 and mtm_debug_steer_q8 without a context) against numpy and brute force, the Python layer's
composition on the CPU oracle against the by-hand loop it documents, every argument error before any native call, the C
ABI's declarations, and the accuracy claim steering exists for - on the particle pair, iterated on the final grid, the
steered call beats both the rigid and the integer-steered one."""
import os
import re

import numpy as np
import pytest

import MTM
import blocks_deform_model as D
import blocks_steer_model as S
from MTM import _lib, subpixel
from MTM import blocks as B

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_IDS = ["1x1", "1xn", "nx1", "3x4", "5x7"]
_SMOOTH_GRIDS = [(1, 1), (1, 6), (6, 1), (2, 2), (3, 4), (5, 7)]


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


# ---- to_q8 and the filter --------------------------------------------------------------------------------------------------
def test_to_q8_against_python_numbers(no_native):
    rng = np.random.RandomState(1)
    p = np.concatenate((rng.uniform(-300, 300, 500), [0.0, -0.0, 0.5 / 256, -0.5 / 256, 1.5 / 256, -1.5 / 256, -1.0 / 512,
                                                       7.001953125, -7.001953125, -3.998046875, float(1 << 22), -float(1 << 22),
                                                       (1 << 22) - 1 / 256.0, 1e-300, -1e-300]))
    got = B.to_q8(p.reshape(-1, 1))
    assert got.dtype == np.int64 and got.shape == (len(p), 1)
    assert got.reshape(-1).tolist() == [S.q8_of(v) for v in p]
    # the floor: half a step rounds towards +infinity on both sides of zero
    assert B.to_q8(np.array([0.5 / 256, -0.5 / 256, -1.5 / 256, -0.75 / 256])).tolist() == [1, 0, -1, -1]
    assert B.to_q8(np.array([[3, -4]])).tolist() == [[768, -1024]] and B.to_q8(np.array([1 << 22])).tolist() == [1 << 30]
    assert B.to_q8(np.zeros((0, 2))).shape == (0, 2)
    for bad in (np.array([np.nan]), np.array([np.inf]), np.array([float((1 << 22) + 1)]), np.array([(1 << 22) + 1])):
        with pytest.raises(ValueError, match="2\\^22"):
            B.to_q8(bad)
    with pytest.raises(TypeError, match="must be numbers"):
        B.to_q8(np.array(["a"]))


@pytest.mark.parametrize("shape", _SMOOTH_GRIDS, ids=lambda s: "%dx%d" % s)
def test_smooth_displacements_against_brute_force(shape, no_native):
    ny, nx = shape
    n = nx * ny
    rng = np.random.RandomState(ny * 10 + nx)
    top = 1 << 30
    sets = [rng.randint(-2000, 2001, size=(n, 2)),                      # signs mixed: fractional results of both signs
            -rng.randint(1, 17, size=(n, 2)),                           # small negatives: sums that are no multiple of 16
            np.where(rng.randint(0, 2, size=(n, 2)) == 1, top, -top),   # the limits
            np.full((n, 2), -top), np.tile(np.array([[-1237, 5]]), (n, 1))]
    for k, d in enumerate(sets):
        got = B.smooth_displacements(shape, d.astype(np.int64))
        assert got.dtype == np.int64 and got.shape == (n, 2)
        assert np.array_equal(got, S.smooth_brute(shape, d)), k
        if k >= 3 or n == 1:
            assert np.array_equal(got, d), k                            # a constant field (and a 1 x 1 grid): unchanged
        assert np.array_equal(B.smooth_displacements(shape, d.astype(np.int32)), got)
    if n > 1:
        assert (S.smooth_brute(shape, sets[1]) * 16 != sum_of(shape, sets[1])).any()      # the floor was exercised


def sum_of(shape, d):
    """16 S without the rounding: the weighted sums themselves."""
    ny, nx = shape
    g = np.asarray(d, dtype=np.int64).reshape(ny, nx, 2)
    out = np.zeros_like(g)
    for j in range(ny):
        for i in range(nx):
            for dv, kv in ((-1, 1), (0, 2), (1, 1)):
                for du, ku in ((-1, 1), (0, 2), (1, 1)):
                    out[j, i] += ku * kv * g[min(max(j + dv, 0), ny - 1), min(max(i + du, 0), nx - 1)]
    return out.reshape(-1, 2)


def test_smooth_displacements_errors(no_native):
    ok = np.zeros((12, 2), np.int64)
    with pytest.raises(TypeError, match="displacements must be integers"):
        B.smooth_displacements((3, 4), ok.astype(np.float64))
    for bad in (ok[:-1], ok.reshape(-1), np.zeros((12, 3), np.int64)):
        with pytest.raises(ValueError, match="displacements of shape"):
            B.smooth_displacements((3, 4), bad)
    for shape in (5, (3,), (3.0, 4), (-1, 4)):
        with pytest.raises(ValueError, match="grid_shape must be"):
            B.smooth_displacements(shape, ok)
    with pytest.raises(ValueError, match="beyond 2\\^30"):
        B.smooth_displacements((3, 4), ok + (1 << 30) + 1)
    assert B.smooth_displacements((0, 4), np.zeros((0, 2), np.int64)).shape == (0, 2)


# ---- the Q8 field ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, coarse", D.GRIDS, ids=_IDS)
def test_q8_field_of_whole_pixels_is_the_integer_field(shape, coarse, no_native):
    """For S = 256 d the Q8 field is today's, bit for bit - over every grid and field of the existing sweep."""
    fine = B.grid(shape, (5, 4), (3, 6))
    for f, disp in enumerate(D.fields(shape, coarse, 5)):
        assert np.array_equal(B.displacement_field(shape, coarse, 256 * disp, q8=True), B.displacement_field(shape, coarse, disp)), f
        assert np.array_equal(B.field_at(shape, coarse, 256 * disp, fine, q8=True), B.field_at(shape, coarse, disp, fine)), f
    nx, ny = D.grid_counts(shape, coarse)
    big = np.full((nx * ny, 2), 1 << 22, np.int64)
    big[::2] = -(1 << 22)
    assert np.array_equal(B.displacement_field(shape, coarse, 256 * big, q8=True), B.displacement_field(shape, coarse, big))


@pytest.mark.parametrize("shape, coarse", D.GRIDS, ids=_IDS)
def test_q8_field_against_brute_force(shape, coarse, no_native):
    fine = B.grid(shape, (5, 4), (3, 6))
    for f, nodes in enumerate(S.q8_fields(shape, coarse, 4)):
        field = B.displacement_field(shape, coarse, nodes, q8=True)
        assert field.dtype == np.int64 and np.array_equal(field, S.field_brute_q8(shape, coarse, nodes)), f
        assert np.array_equal(B.field_at(shape, coarse, nodes, fine, q8=True), S.field_at_brute_q8(shape, coarse, nodes, fine)), f
    assert (S.q8_fields(shape, coarse, 4)[2] % 256 != 0).any()


def test_q8_field_errors(no_native):
    shape, coarse = D.GRIDS[3]
    ok = np.zeros((12, 2), np.int64)
    for fn in (lambda d: B.displacement_field(shape, coarse, d, q8=True), lambda d: B.field_at(shape, coarse, d, B.grid(shape, 4), q8=True),
               lambda d: MTM.deformImage(np.zeros(shape, np.uint8), coarse, d, q8=True)):
        with pytest.raises(TypeError, match="displacements must be integers"):
            fn(ok.astype(np.float64))
        with pytest.raises(ValueError, match="beyond 2\\^22"):
            fn(ok + (1 << 30) + 1)
    assert (B.displacement_field(shape, coarse, ok + (1 << 30), q8=True) == 1 << 30).all()
    with pytest.raises(ValueError, match="q8 must be True or False"):
        B.displacement_field(shape, coarse, ok, q8=1)
    with pytest.raises(_NativeCalled):
        MTM.deformImage(np.zeros(shape, np.uint8), coarse, ok, q8=True)


# ---- the host C the kernels share -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, coarse", D.GRIDS, ids=_IDS)
def test_host_deform_image_q8_equals_numpy(shape, coarse):
    (bw, bh), (sx, sy) = coarse
    for kind in ("u8", "rgb", "u16"):
        img = D.image(shape, kind, 9)
        for f, nodes in enumerate(S.q8_fields(shape, coarse, 6)):
            out = _lib.deform_image(img, (bw, bh, sx, sy), nodes, q8=True)
            exp = B.deform(img, B.displacement_field(shape, coarse, nodes, q8=True))
            assert out.dtype == img.dtype and np.array_equal(out, exp), (kind, f)
    img = D.image(shape, "u8", 1)
    nx, ny = D.grid_counts(shape, coarse)
    for disp in D.fields(shape, coarse, 6)[:4]:                        # 256 d: mtm_deform_image's pixels of d
        assert np.array_equal(_lib.deform_image(img, (bw, bh, sx, sy), 256 * disp, q8=True),
                              _lib.deform_image(img, (bw, bh, sx, sy), disp))
    top = np.full((nx * ny, 2), 1 << 30, np.int64)
    top[::2] = -(1 << 30)
    assert np.array_equal(_lib.deform_image(img, (bw, bh, sx, sy), top, q8=True),
                          B.deform(img, B.displacement_field(shape, coarse, top, q8=True)))
    with pytest.raises(_lib.MtmError, match="mtm_deform_image_q8: block 0: displacement beyond 2\\^22"):
        _lib.deform_image(img, (bw, bh, sx, sy), top + np.where(top > 0, 1, -1), q8=True)


_STEER_GRIDS = [((1, 1), (8, 8)), ((1, 9), (5, 7)), ((9, 1), (6, 4)), ((3, 4), (16, 8)), ((17, 17), (3, 5))]


def test_the_constructed_neighbourhoods_cover_what_they_name():
    nb = S.neighbourhoods(40, 3)
    ox, oy = subpixel.fit_offsets(nb, 5)
    assert (ox == 0.5).any() and (oy == -0.5).any() and ((np.abs(ox) > 0) & (np.abs(ox) < 0.5)).any()
    assert (ox == 0).any() and np.isnan(nb).any() and np.isinf(nb).any() and (np.abs(nb) == S._BIG).any()
    assert (np.abs(ox) <= 0.5).all() and (np.abs(oy) <= 0.5).all()


@pytest.mark.parametrize("method", [1, 5])
@pytest.mark.parametrize("grid_shape, step", _STEER_GRIDS, ids=lambda v: "%dx%d" % v if isinstance(v[0], int) else None)
def test_host_steer_q8_equals_numpy_and_brute_force(grid_shape, step, method):
    ny, nx = grid_shape
    blocks = np.stack((np.tile(np.arange(nx) * step[0], ny), np.repeat(np.arange(ny) * step[1], nx)), axis=1)
    for with_flags in (False, True):
        pos, nb, pred, valid, steer = S.steer_inputs(grid_shape, step, 5 + nx, method, with_flags)
        # numpy: the public helpers, as the docstring's loop uses them
        ox, oy = subpixel.fit_offsets(nb, method)
        fine_w = (pos - ((pred + 128) >> 8)).astype(np.float64) + np.stack((ox, oy), axis=1)
        d8 = B.to_q8(fine_w) - 256 * blocks + pred
        if with_flags:
            d8[~valid] = 256 * (steer - blocks)[~valid]
        for smooth in (0, 1):
            got = _lib.debug_steer_q8(pos, nb, pred, grid_shape, step, method in (0, 1), smooth, valid, steer)
            assert got.dtype == np.int32 and got.shape == (nx * ny, 2)
            exp = B.smooth_displacements(grid_shape, d8) if smooth else d8
            assert np.array_equal(got, exp), (with_flags, smooth)
            assert np.array_equal(got, S.steer_brute(grid_shape, step, method, smooth, pos, nb, pred, valid, steer))


def test_host_steer_q8_errors():
    pos, nb, pred, valid, steer = S.steer_inputs((3, 4), (8, 8), 1, 5, True)
    with pytest.raises(ValueError, match="one position, neighbourhood and field per block"):
        _lib.debug_steer_q8(pos[:-1], nb, pred, (3, 4), (8, 8), 0, 1)
    with pytest.raises(ValueError, match="one position, neighbourhood and field per block"):
        _lib.debug_steer_q8(pos, nb, pred, (3, 4), (8, 8), 0, 1, valid, None)
    with pytest.raises(_lib.MtmError, match="mtm_debug_steer_q8: bad arguments"):
        _lib.debug_steer_q8(pos, nb, pred, (3, 4), (0, 8), 0, 1)


# ---- the Python layer on the oracle ---------------------------------------------------------------------------------------
def _pair(seed, kind, shift=(2, -1), hw=(40, 52)):
    """A smooth reference and the same texture moved by `shift` with a little noise."""
    rng = np.random.RandomState(seed)
    top = 65535 if kind == "u16" else 255
    ref = D.smooth_texture(hw, seed, kind)
    img = np.roll(ref, (shift[1], shift[0]), axis=(0, 1)).astype(np.int64) + rng.randint(-2, 3, size=ref.shape)
    return ref, np.clip(img, 0, top).astype(ref.dtype)


_ORACLE_PASSES = [(16, 8, 4), ((8, 6), (5, 7), 2)]
_REPEATED = [(16, 8, 4), (8, 8, 2), (8, 8, 2)]             # the final grid repeated: what steering is for


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
def test_steered_composition_on_the_oracle(kind, method):
    ref, img = _pair(3, kind)
    fractional = False
    for passes in (_ORACLE_PASSES, _REPEATED) if method in (1, 5) else (_ORACLE_PASSES,):
        for refine in (False, True):
            for validate in (None, (1.0, 0.0)):
                ctx = S.OracleCtx()
                got = MTM.matchBlocksMultipass(ref, img, passes, method, refine=refine, context=ctx, validate=validate,
                                               deform=True, steer="refined")
                (tag, rec, counts, m, with_nbhd, params), = ctx.calls            # one native call
                assert tag == "steered" and m == method and with_nbhd is refine and params == validate
                assert len(rec) == len(passes) and counts == [len(t[0]) for t in got]
                # the loop of the docstring: numpy helpers, matchBlocks on the plain oracle
                exp = S.by_hand(ref, img, passes, method, validate, refine, D.V.M.OracleCtx())
                _same(got, exp, refine, 4 if validate is None else 5)
                assert (got[0][-1] == 0).all()
                fractional |= bool((got[-1][-1] % 1 != 0).any())
    assert fractional                           # a later pass did carry a sub-pixel field


def test_steer_integer_is_the_call_as_it_was():
    ref, img = _pair(4, "u8")
    for validate in (None, True):
        ctx = D.OracleCtx()          # (the context as it was: its match_blocks_passes knows no `steer`)
        got = MTM.matchBlocksMultipass(ref, img, _ORACLE_PASSES, 5, context=ctx, deform=True, steer="integer", validate=validate)
        again = MTM.matchBlocksMultipass(ref, img, _ORACLE_PASSES, 5, context=D.OracleCtx(), deform=True, validate=validate)
        assert ctx.calls[0][0] == "deformed" and len(ctx.calls) == 1
        _same(got, again, False, 4 if validate is None else 5)
    # ... and the keyword that reaches a context: none but deform (and validate)
    seen = []

    class Spy(D.OracleCtx):
        def match_blocks_passes(self, *a, **kw):
            seen.append(sorted(kw))
            return super().match_blocks_passes(*a, **kw)
    MTM.matchBlocksMultipass(ref, img, _ORACLE_PASSES, 5, context=Spy(), deform=True, steer="integer")
    MTM.matchBlocksMultipass(ref, img, _ORACLE_PASSES, 5, context=Spy(), steer="integer")
    assert seen == [["deform"], []]


def test_a_single_steered_pass_is_the_plain_call():
    ref, img = _pair(5, "rgb")
    for refine in (False, True):
        got, = MTM.matchBlocksMultipass(ref, img, _ORACLE_PASSES[:1], 3, refine=refine, context=S.OracleCtx(), deform=True,
                                        steer="refined")
        pos, sc = MTM.matchBlocks(ref, img, B.grid(img.shape, 16, 8), 4, 3, refine=refine, context=D.V.M.OracleCtx())
        assert len(got) == 4 and got[1].dtype == pos.dtype and (got[1] == pos).all() and got[2].tobytes() == sc.tobytes()
        assert (got[3] == 0).all() and got[3].shape == (len(pos), 2)


# ---- the argument errors --------------------------------------------------------------------------------------------------
def test_steer_errors_come_before_any_native_call(no_native):
    u8 = np.zeros((40, 52), np.uint8)
    ok = [(16, 8, 2), (8, 8, 1)]
    for bad in (1, 0, None, True, "Refined", "subpixel", b"refined"):
        with pytest.raises(ValueError, match='steer must be "integer" or "refined"'):
            MTM.matchBlocksMultipass(u8, u8, ok, deform=True, steer=bad)
    for kw in ({}, {"deform": False}, {"validate": True}, {"second": True}):
        with pytest.raises(ValueError, match="steer='refined' needs deform=True"):
            MTM.matchBlocksMultipass(u8, u8, ok, steer="refined", **kw)
    with pytest.raises(ValueError, match="deform=True does not go with second="):
        MTM.matchBlocksMultipass(u8, u8, ok, deform=True, steer="refined", second=True)
    with pytest.raises(ValueError, match=r"len\(passes\) \* max\(H, W\) of at most 2\^22"):
        wide = np.zeros((4, 1 << 21), np.uint8)
        MTM.matchBlocksMultipass(wide, wide, [(4, 4, 0)] * 3, deform=True, steer="refined")
    with pytest.raises(ValueError, match=r"passes\[1\]: margin must be an integer >= 0"):
        MTM.matchBlocksMultipass(u8, u8, [(16, 8, 1), (8, 8, -1)], deform=True, steer="refined")
    with pytest.raises(ValueError, match="refine must be True or False"):
        MTM.matchBlocksMultipass(u8, u8, ok, deform=True, steer="refined", refine=1)
    for kw in ({}, {"validate": True}, {"refine": True}):
        with pytest.raises(_NativeCalled):
            MTM.matchBlocksMultipass(u8, u8, ok, deform=True, steer="refined", **kw)


def test_native_steer_argument_is_checked_first():
    lib = _lib.load()
    code = lib.mtm_match_blocks_passes_steered(None, None, 0, None, 0, 0, 0, 0, 0, None, 0, 0, 0.0, 0.0, None, None, None, None, 2)
    with pytest.raises(_lib.MtmError, match="mtm_match_blocks_passes_steered: steer must be 0 .* or 1 .*got 2"):
        _lib.check(code, "mtm_match_blocks_passes_steered")
    for steer, who in ((0, "mtm_match_blocks_passes_deformed"), (1, "mtm_match_blocks_passes_steered")):
        code = lib.mtm_match_blocks_passes_steered(None, None, 0, None, 0, 0, 0, 0, 0, None, 0, 0, 0.0, 0.0, None, None, None, None,
                                                   steer)
        with pytest.raises(_lib.MtmError, match=who + ": bad arguments"):       # (no context: steer = 0 is the deformed call)
            _lib.check(code, who)


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_abi_symbols():
    hdr = open(os.path.join(ROOT, "include", "mtm_hip.h")).read()
    assert re.search(r"#define MTM_ABI_VERSION 9\b", hdr) and _lib.load().mtm_abi_version() == 9
    since = re.search(r"Entry points added since 9 - (.*?) - are new symbols only", hdr, re.S).group(1)
    for name, n_args in (("mtm_match_blocks_passes_steered", 19), ("mtm_deform_image_q8", 14), ("mtm_debug_steer_q8", 13)):
        assert name in _lib.SYMBOLS and name in since
        decl = re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[name][1]) == n_args
        assert getattr(_lib.load(), name) is not None
    assert {"to_q8", "smooth_displacements"} <= set(B.__all__)


# ---- the claim --------------------------------------------------------------------------------------------------------------
def test_steering_beats_rigid_and_integer_steering_on_the_particle_pair():
    """160 x 192, 2 500 Gaussian particles (sigma 0.9 px) rotated by 0.02 rad; passes [(32, 32, 12), (32, 16, 2), (32, 16,
    2)], TM_CCOEFF_NORMED; the RMS error of the last pass's refined displacements over the 35 blocks at least 32 px from
    every edge, on the CPU oracle."""
    ref, img = S.particle_pair()
    rigid, integer, steered = S.three_rms(ref, img, contexts=S.OracleCtx)
    print("rms error (px) over 35 interior blocks: rigid %.4f, deform=True %.4f, steer='refined' %.4f" % (rigid, integer, steered))
    assert steered < rigid and steered < integer
    assert (round(rigid, 4), round(integer, 4), round(steered, 4)) == S.PARTICLE_RMS_ORACLE      # (what the GPU test expects)
