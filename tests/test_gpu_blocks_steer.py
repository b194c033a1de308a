"""The steer and filter kernels, MTM.deformImage(q8=True) and MTM.matchBlocksMultipass(deform=True, steer="refined") on the
GPU.  The two small kernels equal their host path record for record over partial and several work-groups; the warp with Q8
nodes equals MTM.blocks.deform(displacement_field(q8=True)) pixel for pixel; the steered call equals, pass by pass, the
by-hand loop of matchBlocks and the numpy helpers it documents, in positions (``==``), float32 score bits, flags and
predicted fields; steer="integer" stays the deformed call it was; on the particle pair the three RMS errors are the CPU
oracle's."""
import warnings

import numpy as np
import pytest

import MTM
import blocks_deform_model as D
import blocks_steer_model as S
from MTM import _lib
from MTM import blocks as B

pytestmark = pytest.mark.gpu

_PAIRS = {}
_PASS_SETS = ([(32, 32, 8), (16, 16, 2)], [(32, 64, 12), (32, 16, 3), (32, 16, 3), (16, 8, 1)])
_SHAPES = ((96, 120), (67, 131))


def _pair(kind, shape):
    """One sheared pair per pixel kind and shape for the whole module (never written to)."""
    if (kind, shape) not in _PAIRS:
        ref, img = D.sheared_pair(shape=shape, kind=kind)
        ref.setflags(write=False)
        img.setflags(write=False)
        _PAIRS[kind, shape] = (ref, img)
    return _PAIRS[kind, shape]


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
        for k in range(3, len(e)):
            assert g[k].dtype == e[k].dtype and g[k].shape == e[k].shape and (g[k] == e[k]).all(), (p, k)


# ---- the two small kernels against their host path ---------------------------------------------------------------------------
# 1, 255, 256, 257 and 1 000 records (partial and several work-groups) as 1 x n grids; 1 x 1, 1 x 9, 9 x 1, 3 x 4 and 17 x 17
# nodes (the last: more than one work-group of nodes)
_KERNEL_GRIDS = [((1, 1), (8, 8)), ((1, 255), (3, 4)), ((1, 256), (3, 4)), ((257, 1), (5, 2)), ((25, 40), (4, 4)),
                 ((1, 9), (5, 7)), ((9, 1), (6, 4)), ((3, 4), (16, 8)), ((17, 17), (3, 5))]


@pytest.mark.parametrize("method", [1, 5])
def test_steer_kernels_equal_the_host_path(method):
    ctx = _lib.Context()
    for g, (grid_shape, step) in enumerate(_KERNEL_GRIDS):
        for with_flags in (False, True):
            pos, nb, pred, valid, steer = S.steer_inputs(grid_shape, step, 40 + g, method, with_flags)
            for smooth in (0, 1):
                host = _lib.debug_steer_q8(pos, nb, pred, grid_shape, step, method in (0, 1), smooth, valid, steer)
                dev = _call(ctx.debug_steer_q8, pos, nb, pred, grid_shape, step, method in (0, 1), smooth, valid, steer)
                assert dev.dtype == np.int32 and np.array_equal(dev, host), (grid_shape, with_flags, smooth)
    ctx.close()


# ---- the warp with Q8 nodes against the numpy rule -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "rgb", "u16"])
@pytest.mark.parametrize("shape", sorted(D.GPU_GRIDS), ids=lambda s: "%dx%d" % s)
def test_q8_warp_equals_numpy(shape, kind):
    img = D.image(shape, kind, 13)
    img.setflags(write=False)
    for g, coarse in enumerate(D.GPU_GRIDS[shape]):
        for f, nodes in enumerate(S.q8_fields(shape, coarse, 3 + g)):
            out = _call(MTM.deformImage, img, coarse, nodes, q8=True)
            exp = B.deform(img, B.displacement_field(shape, coarse, nodes, q8=True))
            assert out.dtype == img.dtype and out.shape == img.shape and np.array_equal(out, exp), (g, f)
            if f == 0:
                assert np.array_equal(out, img)
        # q8=False: the pixels it gave before, against numpy - and 256 d in Q8 gives the same
        disp = D.fields(shape, coarse, 3 + g)[4]
        plain = _call(MTM.deformImage, img, coarse, disp)
        assert np.array_equal(plain, B.deform(img, B.displacement_field(shape, coarse, disp))), g
        assert np.array_equal(_call(MTM.deformImage, img, coarse, 256 * disp, q8=True), plain), g


# ---- the steered call against the by-hand loop ---------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", _PASS_SETS, ids=["two", "four"])
@pytest.mark.parametrize("kind, method, shape", [("u8", 5, _SHAPES[0]), ("rgb", 3, _SHAPES[1]), ("u16", 1, _SHAPES[0]),
                                                 ("u8", 5, _SHAPES[1])])
def test_steered_multipass_equals_the_by_hand_loop(kind, method, shape, passes):
    ref, img = _pair(kind, shape)
    assert all(p[0] <= min(shape) for p in passes)
    fractional = False
    for refine in (False, True):
        for validate in (None, (2.0, 0.5)):
            got = _call(MTM.matchBlocksMultipass, ref, img, passes, method, refine=refine, validate=validate, deform=True,
                        steer="refined")
            assert all(len(t) == (4 if validate is None else 5) for t in got)
            _same_passes(got, S.by_hand(ref, img, passes, method, validate, refine))
            assert got[0][-1].dtype == np.float64 and (got[0][-1] == 0).all() and (got[-1][-1] != 0).any()
            fractional |= bool((got[-1][-1] % 1 != 0).any())
    assert fractional


def test_steer_integer_is_the_deformed_call():
    ref, img = _pair("u8", _SHAPES[0])
    for passes in _PASS_SETS:
        for refine in (False, True):
            for validate in (None, (2.0, 0.5)):
                got = _call(MTM.matchBlocksMultipass, ref, img, passes, 5, refine=refine, validate=validate, deform=True,
                            steer="integer")
                _same_passes(got, D.by_hand(ref, img, passes, 5, validate, refine))
    # the native entry with steer = 0 is the deformed entry
    ctx = _lib.default_context()
    rec = _lib.block_pass_records([(32, 32, 32, 32, 8), (16, 16, 16, 16, 2)])
    counts = [len(B.grid(img.shape, 32, 32)), len(B.grid(img.shape, 16, 16))]
    with ctx.lock:
        a = ctx.match_blocks_passes(ref, img, rec, counts, 5, True, deform=True)
        b = ctx.match_blocks_passes(ref, img, rec, counts, 5, True, deform=True, steer=0)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    # a single pass with steer="refined" is the plain call with zero fields
    one, = _call(MTM.matchBlocksMultipass, ref, img, _PASS_SETS[0][:1], 5, deform=True, steer="refined")
    pos, sc = _call(MTM.matchBlocks, ref, img, one[0], 8, 5)
    assert (one[1] == pos).all() and one[2].tobytes() == sc.tobytes() and (one[3] == 0).all()


def _keys(res):
    return [[(h[0], tuple(int(v) for v in h[1]), np.float32(h[2]).tobytes()) for h in r] for r in res]


def test_resident_templates_survive_the_steered_calls():
    ref, img = _pair("u8", _SHAPES[0])
    rng = np.random.RandomState(29)
    templs = [("t%d" % k, rng.randint(0, 256, size=(7 + k, 9)).astype(np.uint8)) for k in range(3)]
    templs[0] = ("t0", img[20:27, 30:39].copy())
    boxes = [(10, 10, 60, 50), (0, 0, 100, 80)]
    ctx = _lib.Context()
    m = MTM.TemplateMatcher(templs, 5, N_object=1, score_threshold=0.2, context=ctx)
    first = m.match_boxes(img, boxes)
    resident = m._uploaded_for
    assert resident is not None
    kw = dict(refine=True, deform=True, steer="refined", validate=True)
    _same_passes(_call(MTM.matchBlocksMultipass, ref, img, _PASS_SETS[0], 3, context=ctx, **kw),
                 _call(MTM.matchBlocksMultipass, ref, img, _PASS_SETS[0], 3, **kw))
    coarse = ((32, 32), (32, 32))
    nodes = S.q8_fields(img.shape, coarse, 4)[3]
    assert np.array_equal(_call(MTM.deformImage, img, coarse, nodes, context=ctx, q8=True),
                          _call(MTM.deformImage, img, coarse, nodes, q8=True))
    assert m._uploaded_for == resident
    again = m.match_boxes(img, boxes)
    assert _keys(first) == _keys(again) and m._uploaded_for == resident
    ctx.close()


# ---- the claim -----------------------------------------------------------------------------------------------------------------
# the CPU oracle's figures for the particle pair (tests/test_blocks_steer_cpu.py prints them): the scores are bit-exact, so the
# device's records, neighbourhoods and hence errors are the same numbers
def test_particle_pair_rms_errors():
    ref, img = S.particle_pair()
    rigid, integer, steered = S.three_rms(ref, img)
    print("rms error (px) over 35 interior blocks: rigid %.4f, deform=True %.4f, steer='refined' %.4f" % (rigid, integer, steered))
    assert steered < rigid and steered < integer
    assert (round(rigid, 4), round(integer, 4), round(steered, 4)) == S.PARTICLE_RMS_ORACLE
