"""Every multipass entry fills one options record and runs one staged chain on the context's shared blk_* buffers, so what a
shared record can newly break is buffer sizing and state left behind by a differently-shaped call.  All 16 legal combinations
of validate x {plain, second, deform, deform + steer="refined"} x refine run in sequence on ONE context, forwards and
backwards, and again behind three-pass calls that make every buffer grow first; MTM.matchBlocks(offsets=, second=) runs
before and after.  Every result equals, bit for bit (NaNs by position), the same call on a fresh context."""
import itertools

import numpy as np
import pytest

import MTM
import blocks_deform_model as D
from MTM import _lib
from MTM import blocks as B

pytestmark = pytest.mark.gpu

_SHAPE = (67, 131)                                  # the smallest pair of test_gpu_blocks_steer.py, and its two-pass set
_TWO = [(32, 32, 8), (16, 16, 2)]
_THREE = [(32, 32, 8), (16, 16, 3), (8, 4, 1)]      # 8 + 32 + 465 blocks: more passes, more blocks, two work-groups of lanes
_METHOD = 5
_KINDS = {"plain": {}, "second": {"second": 2}, "deform": {"deform": True}, "steered": {"deform": True, "steer": "refined"}}
_COMBOS = list(itertools.product((None, (2.0, 0.5)), _KINDS, (False, True)))
_FRESH = {}


def _pair():
    if "pair" not in _FRESH:
        ref, img = D.sheared_pair(shape=_SHAPE, kind="u8")
        ref.setflags(write=False)
        img.setflags(write=False)
        _FRESH["pair"] = (ref, img)
    return _FRESH["pair"]


def _multipass(ctx, passes, combo):
    validate, kind, refine = combo
    ref, img = _pair()
    return MTM.matchBlocksMultipass(ref, img, passes, _METHOD, refine=refine, validate=validate, context=ctx, **_KINDS[kind])


def _single(ctx):
    ref, img = _pair()
    blocks = B.grid(_SHAPE, 16, 16)
    offsets = np.random.RandomState(5).randint(-4, 5, size=(len(blocks), 2))
    return [MTM.matchBlocks(ref, img, blocks, 3, _METHOD, refine=True, context=ctx, offsets=offsets, second=2)]


def _fresh(key, call):
    """The call's result on a context of its own, computed once per module and never written to."""
    if key not in _FRESH:
        ctx = _lib.Context()
        _FRESH[key] = call(ctx)
        ctx.close()
    return _FRESH[key]


def _same(got, exp, what):
    assert len(got) == len(exp), what
    for p, (g, e) in enumerate(zip(got, exp)):
        assert len(g) == len(e), (what, p)
        for k, (a, b) in enumerate(zip(g, e)):
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
            assert a.dtype == b.dtype and a.shape == b.shape, (what, p, k)
            if a.dtype.kind == "f":
                bits = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
                nan = np.isnan(a)
                assert (nan == np.isnan(b)).all() and (a.view(bits)[~nan] == b.view(bits)[~nan]).all(), (what, p, k)
            else:
                assert (a == b).all(), (what, p, k)


def _check_two_pass(ctx, combos, what):
    for combo in combos:
        _same(_multipass(ctx, _TWO, combo), _fresh(("two", combo), lambda c: _multipass(c, _TWO, combo)), (what, combo))


def test_sixteen_combinations_in_sequence_on_one_context():
    assert len(_COMBOS) == 16
    ctx = _lib.Context()
    _same(_single(ctx), _fresh("single", _single), "single before")
    _check_two_pass(ctx, _COMBOS, "forwards")
    _check_two_pass(ctx, _COMBOS[::-1], "backwards")
    _same(_single(ctx), _fresh("single", _single), "single after")
    ctx.close()


def test_buffers_grow_and_are_reused():
    ctx = _lib.Context()
    _same(_single(ctx), _fresh("single", _single), "single before")
    for kind in _KINDS:                 # every feature's buffers grow: validated and refined, so every row is written
        combo = ((2.0, 0.5), kind, True)
        _same(_multipass(ctx, _THREE, combo), _fresh(("three", combo), lambda c: _multipass(c, _THREE, combo)), ("three", combo))
    _check_two_pass(ctx, _COMBOS, "behind three passes")
    _same(_single(ctx), _fresh("single", _single), "single after")
    ctx.close()
