"""MTM.matchBlocksStack(offsets=), MTM.matchBlocksStackMultipass and MTM.blocks.moved_blocks without a GPU: moved_blocks
against a search over every position, every argument error before any native call, offsets=None reaching the old context
call with the old arguments, the Python layer of both modes against the by-hand loops on a context that restates the native
calls on the CPU oracle (tests/blocks_stack_passes_model.py), the float budget, the C ABI's declarations, the host side of
the new entries refusing bad arguments, and the plane-peak rule's host restatement (mtm_debug_plane_peaks without a context)
on constructed sums."""
import ctypes
import os
import re

import numpy as np
import pytest

import MTM
import mtm_oracle as O
import blocks_stack_passes_model as M
from MTM import _lib
from MTM import blocks as B

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HW = (40, 52)
PASSES_2 = [(8, 16, 4), (8, 8, 1)]
PASSES_3 = [(16, 16, 8), (16, 8, 2), (8, 8, 0)]


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


def _movie(seed, n, hw=HW, kind="u8", shift=(2, -1), noise=2):
    """n frames: a random image moved by `shift` = (dx, dy) from frame to frame (wrapping around), with a little noise."""
    rng = np.random.RandomState(seed)
    top = 65536 if kind == "u16" else 256
    shape = hw + (3,) if kind == "rgb" else hw
    base = rng.randint(0, top, size=shape)
    out = []
    for f in range(n):
        a = np.roll(base, (f * shift[1], f * shift[0]), axis=(0, 1)) + rng.randint(-noise, noise + 1, size=shape)
        out.append(np.clip(a, 0, top - 1).astype(np.uint16 if kind == "u16" else np.uint8))
    return out


def _same(got, exp):
    assert len(got) == len(exp)
    for a, b in zip(got, exp):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes()


# ---- moved_blocks ----------------------------------------------------------------------------------------------------------
def test_moved_blocks_against_a_search_over_every_position():
    rng = np.random.RandomState(5)
    shape = (23, 31)
    blocks = [(x, y, w, h) for w, h in ((1, 1), (5, 7), (31, 23), (30, 1), (4, 22)) for x in (0, (31 - w) // 2, 31 - w)
              for y in (0, 23 - h)]
    offs = rng.randint(-40, 41, size=(len(blocks), 2))
    offs[:4] = [(0, 0), (-1, 1), (10 ** 6, -10 ** 6), (-2 ** 31, 2 ** 31 - 1)]
    got = B.moved_blocks(blocks, offs, shape)
    assert got.dtype == np.int64 and got.shape == (len(blocks), 4)
    assert (got == M.moved_brute(blocks, offs, shape)).all()
    for b, o, g in zip(blocks, offs.tolist(), got.tolist()):
        assert B.search_box_at(b, o, 3, shape) == B.search_box(g, 3, shape)
    assert (B.moved_blocks(blocks, np.zeros((len(blocks), 2), np.int64), shape) == np.array(blocks)).all()
    assert B.moved_blocks([], [], shape).shape == (0, 4)
    assert (B.moved_blocks([(3, 3, 4, 4)], [(2 ** 70, -2 ** 70)], shape) == [[27, 0, 4, 4]]).all()      # (any integer)
    with pytest.raises(ValueError, match="offsets must be an"):
        B.moved_blocks(blocks, offs[:-1], shape)
    with pytest.raises(TypeError, match=r"offsets\[1\]"):
        B.moved_blocks(blocks[:2], [(0, 0), (1.5, 0)], shape)
    with pytest.raises(ValueError, match="not inside"):
        B.moved_blocks([(30, 0, 4, 4)], [(0, 0)], shape)


# ---- errors, all before any native call ------------------------------------------------------------------------------------
def test_offsets_errors_come_before_any_native_call(no_native):
    frames = _movie(1, 3)
    blk = [(0, 0, 4, 4), (8, 8, 4, 4)]
    for ensemble in (False, True):
        with pytest.raises(ValueError, match=r"offsets must be an \(N, 2\) integer array"):
            MTM.matchBlocksStack(frames, blk, 2, ensemble=ensemble, offsets=[(0, 0)])
        with pytest.raises(ValueError, match=r"offsets must be an \(N, 2\) integer array"):
            MTM.matchBlocksStack(frames, blk, 2, ensemble=ensemble, offsets=[(0, 0, 0), (1, 1, 1)])
        with pytest.raises(TypeError, match=r"offsets\[1\]: \(dx, dy\) of block 1 must be integers"):
            MTM.matchBlocksStack(frames, blk, 2, ensemble=ensemble, offsets=[(0, 0), (0.5, 1)])
        with pytest.raises(_NativeCalled):
            MTM.matchBlocksStack(frames, blk, 2, ensemble=ensemble, offsets=[(0, 0), (2 ** 40, -3)])
    with pytest.raises(TypeError):
        MTM.matchBlocksStack(frames, blk, 2, 5, [(0, 0), (0, 0)])           # (keyword only)
    with pytest.raises(ValueError, match="needs two frames"):
        MTM.matchBlocksStack(frames[:1], blk, 2, ensemble=True, offsets=[(0, 0), (1, 1)])
    pos, sc = MTM.matchBlocksStack(frames[:1], blk, 2, offsets=[(0, 0), (1, 1)])      # one frame: nothing to do
    assert pos.shape == (0, 2, 2) and sc.shape == (0, 2)
    pos, sc = MTM.matchBlocksStack(frames, [], 2, offsets=[])
    assert pos.shape == (2, 0, 2) and sc.shape == (2, 0)


@pytest.mark.parametrize("kw, exc, msg", [
    ({"frames": 7}, TypeError, "frames must be a sequence"),
    ({"frames": []}, ValueError, "frames is empty"),
    ({"frames": [np.zeros(HW, np.uint8), np.zeros((40, 53), np.uint8)]}, ValueError, r"frames\[1\] differs from frames\[0\]"),
    ({"frames": [np.zeros(HW, np.float32)] * 2}, ValueError, "uint8 frames with 1 or 3 channels"),
    ({"passes": 7}, TypeError, "passes must be a sequence"),
    ({"passes": []}, ValueError, "passes is empty"),
    ({"passes": [(8, 8)]}, ValueError, r"passes\[0\] must be \(block, step, margin\)"),
    ({"passes": [(8, 8, 2), (0, 8, 1)]}, ValueError, r"passes\[1\]: block must be a positive integer"),
    ({"passes": [(8, 8, -1)]}, ValueError, r"passes\[0\]: margin must be an integer >= 0"),
    ({"passes": [(8, 8, 1), (64, 8, 1)]}, ValueError, r"passes\[1\]: no 64 x 64 block fits the 40 x 52 images \(empty grid\)"),
    ({"method": 6}, ValueError, "matchBlocksStackMultipass takes methods 0..5"),
    ({"method": True}, ValueError, "methods 0..5"),
    ({"reference": "last"}, ValueError, 'reference must be "previous" or "first"'),
    ({"refine": 1}, ValueError, "refine must be True or False"),
    ({"ensemble": "yes"}, ValueError, "ensemble must be True or False"),
    ({"frames": [np.zeros(HW, np.uint8)], "ensemble": True}, ValueError, "ensemble=True needs two frames at least"),
    ({"validate": True}, TypeError, "validate"), ({"second": 2}, TypeError, "second"), ({"deform": True}, TypeError, "deform"),
    ({"steer": "refined"}, TypeError, "steer"), ({"mask": np.ones(HW, bool)}, TypeError, "mask"),
], ids=lambda v: None)
def test_multipass_argument_errors_come_before_any_native_call(no_native, kw, exc, msg):
    args = {"frames": _movie(1, 3), "passes": PASSES_2, "method": 5}
    args.update(kw)
    frames, passes, method = args.pop("frames"), args.pop("passes"), args.pop("method")
    with pytest.raises(exc, match=msg):
        MTM.matchBlocksStackMultipass(frames, passes, method, **args)


def test_multipass_options_are_keyword_only_and_valid_arguments_reach_the_library(no_native):
    frames = _movie(1, 3)
    with pytest.raises(TypeError):
        MTM.matchBlocksStackMultipass(frames, PASSES_2, 5, "first")
    for kw in ({}, {"reference": "first", "refine": True}, {"ensemble": True}):
        with pytest.raises(_NativeCalled):
            MTM.matchBlocksStackMultipass(np.stack(frames), PASSES_2, np.int32(3), **kw)
    a = np.zeros((2, 2049, 1025), np.uint16)
    with pytest.raises(ValueError, match=r"passes\[1\]: uint16 blocks of more than 2\^21 pixels"):
        MTM.matchBlocksStackMultipass(a, [((1024, 2048), None, 0), ((1025, 2047), None, 0)])
    # one frame: arrays with a leading 0, no native call
    for refine in (False, True):
        res = MTM.matchBlocksStackMultipass(frames[:1], PASSES_2, refine=refine)
        assert [len(r) for r in res] == [3, 3]
        for (g, pos, sc), (block, step, _) in zip(res, PASSES_2):
            assert (g == B.grid(HW, block, step)).all()
            assert pos.shape == (0, len(g), 2) and pos.dtype == (np.float64 if refine else np.int64)
            assert sc.shape == (0, len(g)) and sc.dtype == np.float32


def test_the_float_budget_covers_the_planes_of_all_passes(no_native):
    frames = _movie(1, 3)
    n0, n1 = len(B.grid(HW, 8, 16)), len(B.grid(HW, 8, 8))
    cells = n0 * 81 + n1 * 9
    ctx = M.StackOracleCtx(max_floats=cells - 1)
    with pytest.raises(ValueError, match="the planes of 2 passes hold %d floats, more than the context's OPT_BOXES_MAX_FLOATS = %d"
                       % (cells, cells - 1)):
        MTM.matchBlocksStackMultipass(frames, PASSES_2, ensemble=True, context=ctx)
    assert ctx.kinds == [] and ctx.calls == []
    ctx = M.StackOracleCtx(max_floats=cells)
    MTM.matchBlocksStackMultipass(frames, PASSES_2, ensemble=True, context=ctx)
    assert [k[0] for k in ctx.kinds] == ["stack_passes"]
    MTM.matchBlocksStackMultipass(frames, PASSES_2, context=M.StackOracleCtx(max_floats=1))       # (no planes, no budget)


# ---- offsets=None is the call as it was ------------------------------------------------------------------------------------
class _Recorder:
    """A context that knows match_blocks_stack only, with the signature it had before offsets= existed."""
    def __init__(self):
        import threading
        self.lock = threading.RLock()
        self.seen = []
        self.inner = M.StackOracleCtx()

    def get_option(self, opt):
        return self.inner.get_option(opt)

    def match_blocks_stack(self, *args, **kw):
        self.seen.append((args, kw))
        return self.inner.match_blocks_stack(*args, **kw)

    def __getattr__(self, name):
        raise AssertionError("matchBlocksStack without offsets used the context's %s" % name)


def test_no_offsets_reach_match_blocks_stack_with_the_old_arguments():
    frames = _movie(2, 3)
    blocks = B.grid(HW, 12, 10)
    rec = _lib.block_records(blocks)
    for kw, want in (({}, {"with_nbhd": False}), ({"refine": True}, {"with_nbhd": True}),
                     ({"ensemble": True, "reference": "first"}, {"planes": True}), ({"offsets": None}, {"with_nbhd": False})):
        ctx = _Recorder()
        MTM.matchBlocksStack(frames, blocks, 3, 5, context=ctx, **kw)
        (args, got), = ctx.seen
        assert got == want and len(args) == 5
        assert all(a is b for a, b in zip(args[0], frames)) and (args[1] == rec).all()
        assert args[2:] == (3, 5, M.FIRST if kw.get("reference") == "first" else M.PREVIOUS)


# ---- matchBlocksStack(offsets=) on the oracle context ----------------------------------------------------------------------
_AT_BLOCKS = [(0, 0, 8, 8), (44, 0, 8, 8), (0, 32, 8, 8), (44, 32, 8, 8), (20, 14, 9, 7), (3, 20, 17, 5), (30, 2, 1, 1)]
_AT_OFFSETS = [(-5, -5), (9, 3), (-2, 30), (100, 100), (2, -1), (0, 0), (-40, 50)]


@pytest.mark.parametrize("reference", ["previous", "first"])
@pytest.mark.parametrize("kind, method", [("u8", 5), ("rgb", 3), ("u16", 1), ("u8", 0)])
def test_stack_offsets_equal_the_loop_and_the_planes_model(kind, method, reference):
    frames = _movie(10 + method, 3, kind=kind)
    mode = M.FIRST if reference == "first" else M.PREVIOUS
    ctx = M.StackOracleCtx()
    for margin in (0, 3):
        for refine in (False, True):
            got = MTM.matchBlocksStack(frames, _AT_BLOCKS, margin, method, reference=reference, refine=refine, offsets=_AT_OFFSETS,
                                       context=ctx)
            exp = [MTM.matchBlocks(frames[r], frames[s], _AT_BLOCKS, margin, method, refine=refine, offsets=_AT_OFFSETS,
                                   context=ctx) for r, s in M.S.pair_frames(3, mode)]
            _same(got, (np.stack([e[0] for e in exp]), np.stack([e[1] for e in exp])))
        planes = M.planes_at(O.compute_score_map, frames, _AT_BLOCKS, _AT_OFFSETS, margin, method, mode)
        moved = B.moved_blocks(_AT_BLOCKS, _AT_OFFSETS, HW)
        for refine in (False, True):
            pos, sc, pl = MTM.matchBlocksStack(frames, _AT_BLOCKS, margin, method, reference=reference, refine=refine,
                                               ensemble=True, offsets=_AT_OFFSETS, context=ctx)
            _same((pl,), (planes,))
            _same((pos, sc), B.plane_peaks(planes, moved, method, refine))
        if margin:
            assert np.isnan(planes[0, 0, 0]) and np.isnan(planes[3, -1, -1]) and not np.isnan(planes[4]).any()
    kinds = [k[0] for k in ctx.kinds]
    assert set(kinds) == {"stack_at"}
    # the offsets reach the context clamped, as int32, and zero offsets give the planes of the call without them
    assert ctx.kinds[0][1][2].tolist() == (B.moved_blocks(_AT_BLOCKS, _AT_OFFSETS, HW)[:, :2] - np.array(_AT_BLOCKS)[:, :2]).tolist()
    zero = MTM.matchBlocksStack(frames, _AT_BLOCKS, 3, method, ensemble=True, offsets=np.zeros((7, 2), np.int8), context=ctx)
    _same(zero, MTM.matchBlocksStack(frames, _AT_BLOCKS, 3, method, ensemble=True, context=ctx))


# ---- matchBlocksStackMultipass on the oracle context -----------------------------------------------------------------------
@pytest.mark.parametrize("refine", [False, True])
@pytest.mark.parametrize("reference", ["previous", "first"])
@pytest.mark.parametrize("passes", [PASSES_2, PASSES_3], ids=["two", "three"])
def test_multipass_per_pair_equals_the_loop_of_matchBlocksMultipass(passes, reference, refine):
    frames = _movie(20, 3, shift=(3, -2))
    ctx = M.StackOracleCtx()
    got = MTM.matchBlocksStackMultipass(frames, passes, 5, reference=reference, refine=refine, context=ctx)
    (kind, args, kw), = ctx.kinds
    assert kind == "stack_passes" and kw == {"with_nbhd": refine, "planes": False}
    assert args[2] == [len(B.grid(HW, b, s)) for b, s, _ in passes] and args[3:] == (5, M.FIRST if reference == "first" else 0)
    exp = M.loop_pairs(lambda *a, **k: MTM.matchBlocksMultipass(*a, context=ctx, **k), frames, passes, 5, reference, refine)
    assert len(got) == len(exp) == len(passes)
    for g, e in zip(got, exp):
        assert len(g) == 3 and g[1].shape == (2, len(g[0]), 2) and g[2].shape == (2, len(g[0]))
        _same(g, e)
    if passes is PASSES_2:          # the movie's step is what the last pass finds away from the border
        g = got[-1][0]
        d = got[-1][1][0] - g[:, :2]
        inner = (g[:, 0] >= 8) & (g[:, 1] >= 8) & (g[:, 0] <= 52 - 16) & (g[:, 1] <= 40 - 16)
        assert inner.sum() >= 4 and (np.round(d[inner]) == (3, -2)).all()


@pytest.mark.parametrize("refine", [False, True])
@pytest.mark.parametrize("reference", ["previous", "first"])
@pytest.mark.parametrize("passes", [PASSES_2, PASSES_3], ids=["two", "three"])
def test_multipass_ensemble_equals_the_by_hand_loop(passes, reference, refine):
    frames = _movie(21, 4, shift=(3, -2))
    ctx = M.StackOracleCtx()
    got = MTM.matchBlocksStackMultipass(frames, passes, 5, reference=reference, refine=refine, ensemble=True, context=ctx)
    (kind, _, kw), = ctx.kinds
    assert kind == "stack_passes" and kw == {"with_nbhd": False, "planes": True}
    exp = M.loop_ensemble(lambda *a, **k: MTM.matchBlocksStack(*a, context=ctx, **k), frames, passes, 5, reference, refine)
    for g, e, (_, _, margin) in zip(got, exp, passes):
        assert len(g) == 4 and g[3].shape == (len(g[0]), 2 * margin + 1, 2 * margin + 1) and g[3].dtype == np.float32
        assert g[1].dtype == (np.float64 if refine else np.int64)
        _same(g, e)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_abi_declarations_and_exports():
    hdr = open(os.path.join(ROOT, "include", "mtm_hip.h")).read()
    for name, n_args in (("mtm_match_blocks_stack_at", 17), ("mtm_match_blocks_stack_passes", 15), ("mtm_debug_plane_peaks", 11)):
        decl = re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[name][1]) == n_args, name
    decl = re.search(r"int mtm_match_blocks_stack\(([^;]*)\);", hdr).group(1)
    assert len(decl.split(",")) == len(_lib.SYMBOLS["mtm_match_blocks_stack"][1]) == 16        # (as it was)
    assert int(re.search(r"#define\s+MTM_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION == 9
    for name in ("match_blocks_stack_at", "match_blocks_stack_passes", "debug_plane_peaks"):
        assert hasattr(_lib.Context, name)
    assert "matchBlocksStackMultipass" in MTM.__all__ and MTM.matchBlocksStackMultipass is B.matchBlocksStackMultipass
    assert {"matchBlocksStackMultipass", "moved_blocks"} <= set(B.__all__)


def test_the_new_entries_refuse_bad_arguments_on_the_host():
    lib = _lib.load()
    frames = [np.zeros((8, 8), np.uint8) for _ in range(3)]
    ptrs = (ctypes.c_void_p * 3)(*[f.ctypes.data for f in frames])
    blk = _lib.block_records([(0, 0, 4, 4)])
    off = np.zeros((1, 2), np.int32)
    out = np.zeros(2, dtype=_lib.HIT_DTYPE)
    ps = _lib.block_pass_records([(4, 4, 4, 4, 1)])
    # no context: refused ahead of everything else, the entry named
    rc = lib.mtm_match_blocks_stack_at(None, ptrs, 3, 8, 8, 1, _lib.MTM_U8, 8, blk.ctypes.data, off.ctypes.data, 1, 2, 5, 0,
                                       out.ctypes.data, None, None)
    assert rc == -1 and b"mtm_match_blocks_stack_at: bad arguments" in lib.mtm_last_error()
    rc = lib.mtm_match_blocks_stack_passes(None, ptrs, 3, 8, 8, 1, _lib.MTM_U8, 8, ps.ctypes.data, 1, 5, 0, out.ctypes.data, None,
                                           None)
    assert rc == -1 and b"mtm_match_blocks_stack_passes: bad arguments" in lib.mtm_last_error()
    # the plane-peak entry checks its arguments with or without a context
    acc = np.zeros((1, 3, 3), np.float64)
    one = np.ones(1, np.int32)
    pl = np.zeros((1, 3, 3), np.float32)
    rec = np.zeros(1, dtype=_lib.HIT_DTYPE)
    ok = (acc.ctypes.data, 1, 3, np.zeros(2, np.int32).ctypes.data, one.ctypes.data, one.ctypes.data, 1, 5, pl.ctypes.data,
          rec.ctypes.data)
    assert lib.mtm_debug_plane_peaks(None, *ok) == 0
    for at, bad in ((0, None), (1, 0), (2, 4), (2, 0), (3, None), (4, None), (5, None), (6, 0), (7, 6), (7, -1), (8, None),
                    (9, None)):
        args = list(ok)
        args[at] = bad
        assert lib.mtm_debug_plane_peaks(None, *args) == -1, (at, bad)
        assert b"mtm_debug_plane_peaks: bad arguments" in lib.mtm_last_error()
    four = np.array([4], np.int32)
    assert lib.mtm_debug_plane_peaks(None, *ok[:4], four.ctypes.data, *ok[5:]) == -1           # (a box taller than the plane)


# ---- the plane-peak rule, on the host ---------------------------------------------------------------------------------------
def check_plane_peaks(context, side, pairs, method):
    """mtm_debug_plane_peaks (a context: blocks_plane_peak_kernel) on the model's constructed sums: planes and records bit for
    bit against the cell-by-cell restatement and, where a plane holds a number, against plane_peaks.  Shared with the GPU
    test."""
    acc, clip, oh, ow = M.plane_cases(side, pairs, 7 * side + pairs)
    planes, recs = _lib.debug_plane_peaks(acc, clip, oh, ow, pairs, method, context=context)
    exp = M.mean_planes(acc, clip, oh, ow, pairs)
    assert planes.dtype == np.float32 and planes.shape == exp.shape
    assert planes.view(np.uint32).tolist() == exp.view(np.uint32).tolist() or (
        (np.isnan(planes) == np.isnan(exp)).all() and (planes[~np.isnan(exp)].view(np.uint32) == exp[~np.isnan(exp)].view(np.uint32)).all())
    want = M.peak_records(exp, method)
    for k, (dx, dy, s) in enumerate(want):
        r = recs[k]
        assert (int(r["x"]), int(r["y"])) == (dx, dy), (k, r, want[k])
        assert np.float32(r["score"]).tobytes() == s.tobytes() or (np.isnan(s) and np.isnan(r["score"])), (k, r, want[k])
        assert int(r["templ_idx"]) == k
    some = ~np.isnan(exp).all(axis=(1, 2))
    assert some.sum() == len(exp) - 1
    pos, sc = B.plane_peaks(planes[some], np.zeros((int(some.sum()), 4), np.int64), method)
    assert (pos == np.stack((recs["x"], recs["y"]), axis=1)[some]).all()
    assert sc.tobytes() == recs["score"][some].astype(np.float32).tobytes()
    return planes, recs


@pytest.mark.parametrize("pairs", [1, 7])
@pytest.mark.parametrize("method", [0, 5])
@pytest.mark.parametrize("side", [1, 3, 17, 33])
def test_plane_peak_rule_on_the_host(side, method, pairs):
    planes, recs = check_plane_peaks(None, side, pairs, method)
    acc, clip, oh, ow = M.plane_cases(side, pairs, 7 * side + pairs)
    n_rand = 6
    if side > 1:
        # the ties: first, middle and last cell tied - the first wins; without the first - the middle; the last alone
        m = side // 2
        # (per tie set a raised and a lowered variant: the raised ones peak under method 5, the lowered ones under method 0)
        tied = [(int(r["x"]), int(r["y"])) for r in recs[n_rand + (1 if method == 0 else 0):n_rand + 6:2]]
        assert tied == [(-m, -m), (0, 0), (m, m)]
        # zeros of both signs are one value: the first cell, and its own sign
        z = recs[n_rand + 6:n_rand + 8]
        assert [(int(r["x"]), int(r["y"])) for r in z] == [(-m, -m)] * 2
        assert np.signbit(z[0]["score"]) and not np.signbit(z[1]["score"])
