"""MTM.matchBlocksMultipass(validate=) and blocks_validate_kernel on the GPU.  The kernel (mtm_debug_validate_blocks with a
context) equals MTM.blocks.validate flag for flag and position for position, over grids of more than one work-group too; the
validated call equals, pass by pass, the by-hand loop of matchBlocks(offsets=), validate and predict_offsets it documents, in
positions (``==``), float32 score bits and flags; on the scene with one flat coarse block it finds every block the
unvalidated call loses."""
import warnings

import numpy as np
import pytest

import MTM
import blocks_validate_model as V
from MTM import _lib
from MTM import blocks as B

pytestmark = pytest.mark.gpu

_SCENES = {}


def _scene(kind):
    """One pair per pixel kind for the whole module (never written to)."""
    if kind not in _SCENES:
        ref, img = V.scene(kind)
        ref.setflags(write=False)
        img.setflags(write=False)
        _SCENES[kind] = (ref, img)
    return _SCENES[kind]


def _call(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("error")              # no warnings are emitted
        return fn(*a, **kw)


def _same_passes(got, exp):
    assert len(got) == len(exp)
    for p, (g, e) in enumerate(zip(got, exp)):              # every pass, the non-final ones included
        assert len(g) == len(e)
        assert g[0].dtype == e[0].dtype and (g[0] == e[0]).all()
        assert g[1].dtype == e[1].dtype and g[1].shape == e[1].shape
        bad = np.flatnonzero((g[1] != e[1]).any(axis=1) | (g[2].view(np.uint32) != e[2].view(np.uint32)))
        assert g[2].dtype == np.float32 and len(bad) == 0, (p, bad[:5], g[1][bad[:5]], e[1][bad[:5]])
        if len(e) == 4:
            assert g[3].dtype == bool and g[3].shape == e[3].shape and (g[3] == e[3]).all(), (p, np.flatnonzero(g[3] != e[3]))


# ---- the kernel against the numpy rule ----------------------------------------------------------------------------------
# 1 x 257 and 17 x 16 (272 blocks): two 256-lane work-groups, the last one partly filled
@pytest.mark.parametrize("grid_shape", V.GRIDS + ((1, 257), (17, 16)), ids=lambda g: "%dx%d" % g)
def test_kernel_equals_validate(grid_shape):
    ny, nx = grid_shape
    ctx = _lib.default_context()
    g = np.stack((np.tile(np.arange(nx), ny), np.repeat(np.arange(ny), nx)), axis=1).astype(np.int64)
    flagged = 0
    for f, field in enumerate(V.fields(grid_shape, 11 * ny + nx, every=1 if ny * nx <= 64 else 15)):
        step = ((16, 16), (5, 7), (1, 3))[f % 3]
        at = g * np.array(step)
        for threshold, epsilon in V.PARAMS:
            e_valid, e_rep = B.validate(grid_shape, field, threshold, epsilon)
            with ctx.lock:
                valid, steer = ctx.debug_validate_blocks(at + field, grid_shape, step, threshold, epsilon)
            assert valid.dtype == bool and np.array_equal(valid, e_valid), (f, threshold, epsilon)
            assert np.array_equal(steer, at + e_rep), (f, threshold, epsilon)
            flagged += int((~valid).sum())
    assert (flagged == 0) == (min(ny, nx) == 1 or ny * nx < 4)


# ---- the validated call against the by-hand loop -----------------------------------------------------------------------
@pytest.mark.parametrize("kind, method", [("u8", 5), ("u8", 1), ("rgb", 5), ("rgb", 3), ("u16", 5), ("u16", 0)])
def test_validated_multipass_equals_the_by_hand_loop(kind, method):
    ref, img = _scene(kind)
    got = _call(MTM.matchBlocksMultipass, ref, img, V.SCENE_PASSES, method, validate=True)
    assert all(len(t) == 4 for t in got)
    _same_passes(got, V.by_hand(ref, img, V.SCENE_PASSES, method, 2.0, 0.5))
    if method != 5:
        return
    raw = _call(MTM.matchBlocksMultipass, ref, img, V.SCENE_PASSES, 5)
    _same_passes(raw, V.by_hand(ref, img, V.SCENE_PASSES, 5, None, None))
    blocks0, pos0, _, valid0 = got[0]
    assert tuple(B.displacements(blocks0, pos0)[5]) == (-16, -16)          # the flat block: its box's first output
    assert valid0.tolist() == [k != 5 for k in range(12)]                   # pass 0 flags exactly the flat block
    assert (pos0 == raw[0][1]).all()                                        # the returned positions stay the raw ones
    blocks1, pos1 = got[1][:2]
    out = V.outside_patch(blocks1)
    assert len(blocks1) == 140 and out.sum() == 136
    found_val = int((B.displacements(blocks1, pos1)[out] == V.SCENE_SHIFT).all(axis=1).sum())
    found_raw = int((B.displacements(raw[1][0], raw[1][1])[out] == V.SCENE_SHIFT).all(axis=1).sum())
    print("found validated %d, unvalidated %d of %d" % (found_val, found_raw, out.sum()))
    assert found_val == 136 and found_raw < found_val


@pytest.mark.parametrize("kind", ["u8", "rgb", "u16"])
def test_refined_positions_are_those_of_the_loop(kind):
    ref, img = _scene(kind)
    got = _call(MTM.matchBlocksMultipass, ref, img, V.SCENE_PASSES, 5, refine=True, validate=(2.0, 0.5))
    exp = V.by_hand(ref, img, V.SCENE_PASSES, 5, 2.0, 0.5, refine=True)
    assert got[1][1].dtype == np.float64
    _same_passes(got, exp)
    # three passes, other parameters: the second pass's flags steer the third
    passes = [(32, 32, 16), (16, 16, 3), ((8, 6), (7, 5), 1)]
    _same_passes(_call(MTM.matchBlocksMultipass, ref, img, passes, 3, refine=True, validate=(1.0, 0.0)),
                 V.by_hand(ref, img, passes, 3, 1.0, 0.0, refine=True))


def test_a_one_row_coarse_grid_is_the_unvalidated_call():
    rng = np.random.RandomState(9)
    ref = rng.randint(0, 256, size=(40, 200)).astype(np.uint8)
    img = np.roll(ref, (1, -6), axis=(0, 1))
    ref[0:32, 64:96] = 31              # coarse block 2 is flat: a grid with more rows would flag it
    passes = [(32, 32, 8), ((16, 40), (8, 40), 2)]
    assert B.grid_shape(ref.shape, 32, 32) == (1, 6) and B.grid_shape(ref.shape, (16, 40), (8, 40)) == (1, 24)
    for refine in (False, True):
        val = _call(MTM.matchBlocksMultipass, ref, img, passes, 5, refine=refine, validate=True)
        raw = _call(MTM.matchBlocksMultipass, ref, img, passes, 5, refine=refine)
        for (vb, vp, vs, vv), (rb, rp, rs) in zip(val, raw):
            assert (vb == rb).all() and vp.dtype == rp.dtype and vp.tobytes() == rp.tobytes() and vs.tobytes() == rs.tobytes()
            assert vv.dtype == bool and vv.all() and vv.shape == (len(vb),)
    assert (B.displacements(raw[0][0], raw[0][1])[2] != (-6, 1)).any()          # the flat block did match wrongly
