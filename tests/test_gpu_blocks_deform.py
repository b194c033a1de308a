"""MTM.deformImage, deform_image_kernel and MTM.matchBlocksMultipass(deform=True) on the GPU.  The kernel equals
MTM.blocks.deform(displacement_field(...)) pixel for pixel over image sizes that leave partial work-groups at both edges,
every grid kind and field of the CPU sweep and the three pixel kinds; the deformed call equals, pass by pass, the by-hand
loop of matchBlocks, displacement_field, deform and field_at it documents, in positions (``==``), float32 score bits, flags
and predicted fields; deform=False stays the call it was; on a sheared pair the deformed call's last pass scores higher."""
import warnings

import numpy as np
import pytest

import MTM
import blocks_deform_model as D
from MTM import _lib
from MTM import blocks as B

pytestmark = pytest.mark.gpu

_PAIRS = {}
_PASS_SETS = ([(32, 32, 8), (16, 16, 2)], [(32, 64, 12), (32, 16, 3), (16, 8, 1)])


def _pair(kind):
    """One sheared pair per pixel kind for the whole module (never written to)."""
    if kind not in _PAIRS:
        ref, img = D.sheared_pair(kind=kind)
        ref.setflags(write=False)
        img.setflags(write=False)
        _PAIRS[kind] = (ref, img)
    return _PAIRS[kind]


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


# ---- the kernel against the numpy rule ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "rgb", "u16"])
@pytest.mark.parametrize("shape", sorted(D.GPU_GRIDS), ids=lambda s: "%dx%d" % s)
def test_kernel_equals_numpy(shape, kind):
    assert tuple(D.grid_counts(shape, c) for c in D.GPU_GRIDS[shape]) == D.GRID_COUNTS
    img = D.image(shape, kind, 13)
    img.setflags(write=False)
    for g, coarse in enumerate(D.GPU_GRIDS[shape]):
        for f, disp in enumerate(D.fields(shape, coarse, 3 + g)):
            out = _call(MTM.deformImage, img, coarse, disp)
            exp = B.deform(img, B.displacement_field(shape, coarse, disp))
            assert out.dtype == img.dtype and out.shape == img.shape and np.array_equal(out, exp), (g, f)
            if f == 0:
                assert np.array_equal(out, img)


@pytest.mark.parametrize("kind", ["u8", "rgb", "u16"])
def test_kernel_over_several_work_groups_along_a_row(kind):
    shape, coarse = D.WIDE
    assert D.grid_counts(shape, coarse) == (4, 3)
    img = D.image(shape, kind, 17)
    view = np.concatenate((img, img), axis=1)[:, 3:3 + shape[1]]             # rows of a wider array: a stride of its own
    for disp in D.fields(shape, coarse, 8)[3:]:
        exp = B.deform(view, B.displacement_field(shape, coarse, disp))
        assert np.array_equal(_call(MTM.deformImage, view, coarse, disp), exp)


# ---- the deformed call against the by-hand loop -------------------------------------------------------------------------
@pytest.mark.parametrize("passes", _PASS_SETS, ids=["two", "three"])
@pytest.mark.parametrize("kind, method", [("u8", 5), ("rgb", 3), ("u16", 1)])
def test_deformed_multipass_equals_the_by_hand_loop(kind, method, passes):
    ref, img = _pair(kind)
    passes = D.clip_passes(passes, img.shape)
    assert len(passes) >= 2
    for refine in (False, True):
        for validate in (None, (2.0, 0.5)):
            got = _call(MTM.matchBlocksMultipass, ref, img, passes, method, refine=refine, validate=validate, deform=True)
            assert all(len(t) == (4 if validate is None else 5) for t in got)
            _same_passes(got, D.by_hand(ref, img, passes, method, validate, refine))
            assert got[0][-1].dtype == np.float64 and (got[0][-1] == 0).all() and (got[-1][-1] != 0).any()


def test_deform_false_is_the_parent_call():
    ref, img = _pair("u8")
    for passes in _PASS_SETS:
        for refine in (False, True):
            got = _call(MTM.matchBlocksMultipass, ref, img, passes, 5, refine=refine, deform=False)
            assert all(len(t) == 3 for t in got)
            _same_passes(got, D.V.by_hand(ref, img, passes, 5, None, None, refine))
    val = _call(MTM.matchBlocksMultipass, ref, img, _PASS_SETS[0], 5, validate=True, deform=False)
    _same_passes(val, D.V.by_hand(ref, img, _PASS_SETS[0], 5, 2.0, 0.5))
    # a single pass with deform=True is the plain call with zero fields
    one, = _call(MTM.matchBlocksMultipass, ref, img, _PASS_SETS[0][:1], 5, deform=True)
    pos, sc = _call(MTM.matchBlocks, ref, img, one[0], 8, 5)
    assert (one[1] == pos).all() and one[2].tobytes() == sc.tobytes() and (one[3] == 0).all()


def test_deformation_sharpens_the_peak_under_shear():
    ref, img = _pair("u8")
    passes = [(32, 32, 12), (32, 16, 2)]
    plain = _call(MTM.matchBlocksMultipass, ref, img, passes, 5)
    bent = _call(MTM.matchBlocksMultipass, ref, img, passes, 5, deform=True)
    inner = D.interior(plain[1][0], img.shape, 16)
    s_plain, s_bent = float(plain[1][2][inner].mean()), float(bent[1][2][inner].mean())
    print("mean last-pass score over %d interior blocks: rigid %.4f, deformed %.4f" % (inner.sum(), s_plain, s_bent))
    assert inner.sum() >= 20 and s_bent > s_plain


def _keys(res):
    return [[(h[0], tuple(int(v) for v in h[1]), np.float32(h[2]).tobytes()) for h in r] for r in res]


def test_resident_templates_survive_the_new_calls():
    ref, img = _pair("u8")
    rng = np.random.RandomState(29)
    templs = [("t%d" % k, rng.randint(0, 256, size=(7 + k, 9)).astype(np.uint8)) for k in range(3)]
    templs[0] = ("t0", img[20:27, 30:39].copy())
    boxes = [(10, 10, 60, 50), (0, 0, 100, 80)]
    ctx = _lib.Context()
    m = MTM.TemplateMatcher(templs, 5, N_object=1, score_threshold=0.2, context=ctx)
    first = m.match_boxes(img, boxes)
    resident = m._uploaded_for
    assert resident is not None
    _same_passes(_call(MTM.matchBlocksMultipass, ref, img, _PASS_SETS[0], 3, refine=True, deform=True, context=ctx),
                 _call(MTM.matchBlocksMultipass, ref, img, _PASS_SETS[0], 3, refine=True, deform=True))
    coarse = ((32, 32), (32, 32))
    disp = D.fields(img.shape, coarse, 4)[4]
    assert np.array_equal(_call(MTM.deformImage, img, coarse, disp, context=ctx), _call(MTM.deformImage, img, coarse, disp))
    assert m._uploaded_for == resident
    again = m.match_boxes(img, boxes)
    assert _keys(first) == _keys(again) and m._uploaded_for == resident
    ctx.close()
