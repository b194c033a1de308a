"""MTM.matchBlocksStack / MTM.blocks.plane_peaks without a GPU: every argument error comes before any native call, the empty
cases, the Python layer's results from a fake context that restates the native call on the CPU oracle, plane_peaks on
constructed planes, the C ABI's declaration, and the host planner - frame chunks and clip offsets - against a plain
restatement (tests/blocks_stack_model.py)."""
import os
import re
import threading
import warnings

import numpy as np
import pytest

import MTM
import mtm_oracle as O
import blocks_stack_model as M
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


def _cut(smap, x, y):
    out = np.full((3, 3), np.nan, dtype=np.float32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if 0 <= y + dy < smap.shape[0] and 0 <= x + dx < smap.shape[1]:
                out[1 + dy, 1 + dx] = smap[y + dy, x + dx]
    return out


class _OracleCtx:
    """match_blocks (the loop's call) and match_blocks_stack on the CPU oracle; records what reaches match_blocks_stack."""
    def __init__(self, max_floats=1 << 26):
        self.lock = threading.RLock()
        self.calls = []
        self.max_floats = max_floats

    def get_option(self, opt):
        assert opt == _lib.OPT_BOXES_MAX_FLOATS
        return self.max_floats

    def match_blocks(self, reference, image, blocks, margin, method, with_nbhd=False):
        n = len(blocks)
        out = np.zeros(n, dtype=_lib.HIT_DTYPE)
        nbhd = np.empty((n, 3, 3), dtype=np.float32) if with_nbhd else None
        ref, img = np.ascontiguousarray(reference), np.ascontiguousarray(image)
        for k, b in enumerate(blocks):
            x, y, w, h = (int(b[f]) for f in "xywh")
            t = ref[y:y + h, x:x + w]
            (_, (hx, hy, hw, hh), s), = O.find_matches([("b", t)], img, method, 1,
                                                       searchBox=B.search_box((x, y, w, h), margin, img.shape))
            out[k] = (k, hx, hy, hw, hh, s)
            if with_nbhd:
                nbhd[k] = _cut(O.compute_score_map(t, img, method), hx, hy)
        return out, nbhd

    def match_blocks_stack(self, frames, blocks, margin, method, mode, with_nbhd=False, planes=False):
        self.calls.append((frames, blocks.copy(), margin, method, mode, with_nbhd, planes))
        if planes:
            b = np.stack([blocks[f] for f in "xywh"], axis=1)
            return M.planes(O.compute_score_map, [np.ascontiguousarray(f) for f in frames], b, margin, method, mode)
        res = [self.match_blocks(frames[r], frames[s], blocks, margin, method, with_nbhd)
               for r, s in M.pair_frames(len(frames), mode)]
        return (np.concatenate([r[0] for r in res]),
                np.concatenate([r[1] for r in res]) if with_nbhd else None)

    def __getattr__(self, name):
        raise AssertionError("matchBlocksStack used the context's %s" % name)


def _movie(seed, n, hw=(40, 52), kind="u8", shift=(2, -1), noise=2):
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


# ---- errors, all before any native call ----------------------------------------------------------------------------------
def test_frame_errors_come_before_any_native_call(no_native):
    u8 = np.zeros((20, 30), np.uint8)
    blk = [(0, 0, 4, 4)]
    for bad, i in (([u8, np.zeros((20, 31), np.uint8)], 1), ([u8, u8, np.zeros((20, 30), np.uint16)], 2),
                   ([u8, np.zeros((20, 30, 3), np.uint8), u8], 1), ([np.zeros((20, 30, 1), np.uint8), u8], 1)):
        with pytest.raises(ValueError, match=r"frames\[%d\] differs from frames\[0\]" % i):
            MTM.matchBlocksStack(bad, blk, 2)
    for a in (np.zeros((20, 30), np.float32), np.zeros((20, 30, 2), np.uint8), np.zeros((20, 30, 4), np.uint8),
              np.zeros((20, 30, 3), np.uint16), np.zeros((20, 30), np.float64), np.zeros((20,), np.uint8)):
        with pytest.raises(ValueError, match="uint8 frames with 1 or 3 channels and single-channel uint16"):
            MTM.matchBlocksStack([a, a.copy()], blk, 2)
    with pytest.raises(TypeError, match=r"frames\[1\] must be a numpy array"):
        MTM.matchBlocksStack([u8, [[1, 2], [3, 4]]], blk, 2)
    with pytest.raises(TypeError, match="frames must be a sequence"):
        MTM.matchBlocksStack(7, blk, 2)
    with pytest.raises(ValueError, match=r"\(F, H, W\) or \(F, H, W, C\)"):
        MTM.matchBlocksStack(u8, blk, 2)                              # (one image is not a stack)
    with pytest.raises(ValueError, match="frames is empty"):
        MTM.matchBlocksStack([], blk, 2)
    with pytest.raises(ValueError, match="at most 32767 rows"):
        MTM.matchBlocksStack(np.zeros((2, 32768, 4), np.uint8), blk, 2)
    with pytest.raises(ValueError, match="frames are empty"):
        MTM.matchBlocksStack(np.zeros((2, 0, 4), np.uint8), [], 2)


@pytest.mark.parametrize("blocks, exc, msg", [
    ([(0, 0, 4)], ValueError, r"\(N, 4\)"),
    (np.zeros((2, 4), np.float32), TypeError, "integers"),
    ([(0, 0, 4, 4), (1, 1, 4.0, 4)], TypeError, r"blocks\[1\]"),
    ([(0, 0, 4, 4), (1, 1, 0, 4), (50, 0, 4, 4)], ValueError, r"blocks\[1\].*w >= 1 and h >= 1"),
    ([(0, 0, 4, 4), (0, 0, 30, 20), (27, 0, 4, 4)], ValueError, r"blocks\[2\].*not inside the 20 x 30"),
    ([(0, -1, 4, 4)], ValueError, r"blocks\[0\].*not inside"),
], ids=lambda v: None)
@pytest.mark.parametrize("ensemble", [False, True])
def test_block_errors_name_the_first_bad_block(no_native, blocks, exc, msg, ensemble):
    with pytest.raises(exc, match=msg):
        MTM.matchBlocksStack(_movie(1, 3, (20, 30)), blocks, 2, ensemble=ensemble)


def test_uint16_block_of_more_than_2_21_pixels(no_native):
    a = np.zeros((2, 2049, 1025), np.uint16)
    with pytest.raises(ValueError, match=r"blocks\[1\]: uint16 blocks of more than 2\^21 pixels"):
        MTM.matchBlocksStack(a, [(0, 0, 1024, 2048), (0, 0, 1025, 2047)], 0)


@pytest.mark.parametrize("what, value, msg", [
    ("margin", -1, "margin"), ("margin", 1.0, "margin"), ("margin", True, "margin"), ("margin", None, "margin"),
    ("method", 6, "methods 0..5"), ("method", -1, "methods 0..5"), ("method", 5.0, "methods 0..5"), ("method", True, "methods 0..5"),
    ("reference", "last", "reference"), ("reference", 0, "reference"), ("reference", None, "reference"),
    ("reference", "Previous", "reference"), ("reference", ["first"], "reference"),
    ("refine", 1, "refine"), ("refine", None, "refine"), ("refine", np.bool_(True), "refine"),
    ("ensemble", 1, "ensemble"), ("ensemble", "yes", "ensemble"), ("ensemble", np.bool_(False), "ensemble"),
], ids=repr)
def test_argument_errors_come_before_any_native_call(no_native, what, value, msg):
    frames = _movie(1, 3)
    kw = {"margin": 2, "method": 5}
    kw[what] = value
    margin, method = kw.pop("margin"), kw.pop("method")
    for blocks in ([(0, 0, 4, 4)], []):                         # (also with nothing to match)
        with pytest.raises(ValueError, match=msg):
            MTM.matchBlocksStack(frames, blocks, margin, method, **kw)


def test_options_are_keyword_only_and_valid_arguments_reach_the_library(no_native):
    frames = _movie(1, 3)
    with pytest.raises(TypeError):
        MTM.matchBlocksStack(frames, [(0, 0, 4, 4)], 2, 5, "first")
    for kw in ({}, {"reference": "first", "refine": True}, {"ensemble": True}):
        with pytest.raises(_NativeCalled):
            MTM.matchBlocksStack(frames, [(0, 0, 4, 4)], np.int64(2), np.int32(3), **kw)
        with pytest.raises(_NativeCalled):
            MTM.matchBlocksStack(np.stack(frames), np.array([(0, 0, 4, 4)]), 2, **kw)


def test_ensemble_planes_past_the_float_budget(no_native):
    frames = _movie(1, 3)
    ctx = _OracleCtx(max_floats=3 * 25 - 1)
    blocks = [(0, 0, 4, 4), (5, 5, 4, 4), (9, 9, 4, 4)]
    with pytest.raises(ValueError, match=r"3 blocks at margin 2 hold 75 floats.*OPT_BOXES_MAX_FLOATS = 74"):
        MTM.matchBlocksStack(frames, blocks, 2, ensemble=True, context=ctx)
    assert ctx.calls == []
    ctx.max_floats = 75
    MTM.matchBlocksStack(frames, blocks, 2, ensemble=True, context=ctx)
    MTM.matchBlocksStack(frames, blocks, 9, context=_OracleCtx(max_floats=1))       # (no planes: no bound)


# ---- the empty cases -----------------------------------------------------------------------------------------------------
def test_one_frame_and_empty_blocks(no_native):
    frames = _movie(1, 4)
    for refine, ptype in ((False, np.int64), (True, np.float64)):
        pos, sc = MTM.matchBlocksStack(frames[:1], [(0, 0, 4, 4), (3, 3, 5, 5)], 3, refine=refine)
        assert pos.shape == (0, 2, 2) and pos.dtype == ptype and sc.shape == (0, 2) and sc.dtype == np.float32
        pos, sc = MTM.matchBlocksStack(np.stack(frames), np.zeros((0, 4), np.int64), 3, refine=refine, reference="first")
        assert pos.shape == (3, 0, 2) and pos.dtype == ptype and sc.shape == (3, 0) and sc.dtype == np.float32
        pos, sc, pl = MTM.matchBlocksStack(frames, [], 3, refine=refine, ensemble=True)
        assert pos.shape == (0, 2) and pos.dtype == ptype and sc.shape == (0,) and sc.dtype == np.float32
        assert pl.shape == (0, 7, 7) and pl.dtype == np.float32
    for blocks in ([(0, 0, 4, 4)], []):
        with pytest.raises(ValueError, match="no pair to average"):
            MTM.matchBlocksStack(frames[:1], blocks, 3, ensemble=True)


# ---- the Python layer against the oracle -----------------------------------------------------------------------------------
_BLOCKS = [(0, 0, 7, 5), (10, 8, 6, 6), (52 - 9, 40 - 4, 9, 4), (20, 0, 12, 3), (0, 30, 5, 10), (17, 11, 1, 1), (2, 1, 48, 37)]


@pytest.mark.parametrize("kind", ["u8", "rgb", "u16"])
@pytest.mark.parametrize("reference", ["previous", "first"])
def test_python_layer_returns_the_loops_results(monkeypatch, kind, reference):
    frames = _movie(5, 4, kind=kind, shift=(1, -1))
    method = {"u8": 5, "rgb": 3, "u16": 1}[kind]
    ctx = _OracleCtx()
    monkeypatch.setattr(_lib, "default_context", lambda: ctx)
    mode = M.FIRST if reference == "first" else M.PREVIOUS
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pos, sc = MTM.matchBlocksStack(frames, _BLOCKS, 3, method, reference=reference)
        fpos, fsc = MTM.matchBlocksStack(np.stack(frames), np.array(_BLOCKS), 3, method, reference=reference, refine=True,
                                         context=ctx)
    assert pos.shape == (3, 7, 2) and pos.dtype == np.int64 and sc.shape == (3, 7) and sc.dtype == np.float32
    assert fpos.shape == (3, 7, 2) and fpos.dtype == np.float64 and fsc.dtype == np.float32
    for p, (r, s) in enumerate(M.pair_frames(4, mode)):
        e_pos, e_sc = MTM.matchBlocks(frames[r], frames[s], _BLOCKS, 3, method, context=ctx)
        e_fpos, _ = MTM.matchBlocks(frames[r], frames[s], _BLOCKS, 3, method, refine=True, context=ctx)
        assert (pos[p] == e_pos).all() and sc[p].tobytes() == e_sc.tobytes() and fsc[p].tobytes() == e_sc.tobytes()
        assert (fpos[p] == e_fpos).all()
    assert (fpos != pos).any()                                  # (something was fitted)
    step = (1, -1) if reference == "previous" else (3, -3)
    assert tuple(B.displacements(_BLOCKS, pos[2])[1]) == step   # the interior block follows the movie's shift
    # what reached the context: the frames as passed, int32 block records, margin, method, mode, the two flags
    (f0, b0, m0, me0, mo0, nb0, pl0), (f1, b1, m1, me1, mo1, nb1, pl1) = ctx.calls
    assert all(a is b for a, b in zip(f0, frames)) and len(f1) == 4
    for b in (b0, b1):
        assert b.dtype == _lib.BLOCK_DTYPE and np.stack([b[f] for f in "xywh"], axis=1).tolist() == [list(v) for v in _BLOCKS]
    assert (m0, me0, mo0, nb0, pl0) == (3, method, mode, False, False) and (m1, me1, mo1, nb1, pl1) == (3, method, mode, True, False)


@pytest.mark.parametrize("kind", ["u8", "rgb", "u16"])
@pytest.mark.parametrize("method", [1, 5])
def test_python_layer_returns_the_restated_ensemble(kind, method):
    frames = _movie(6, 4, kind=kind, shift=(1, 0))
    ctx = _OracleCtx()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pos, sc, pl = MTM.matchBlocksStack(frames, _BLOCKS, 3, method, ensemble=True, reference="first", context=ctx)
        fpos, fsc, fpl = MTM.matchBlocksStack(frames, _BLOCKS, 3, method, ensemble=True, reference="first", refine=True,
                                              context=ctx)
    exp = M.planes(O.compute_score_map, frames, _BLOCKS, 3, method, M.FIRST)
    assert pl.dtype == np.float32 and pl.shape == (7, 7, 7) and pl.tobytes() == exp.tobytes() == fpl.tobytes()
    assert np.isnan(pl[0, :3]).all() and np.isnan(pl[0, :, :3]).all() and not np.isnan(pl[0, 3:, 3:]).any()
    assert not np.isnan(pl[1]).any()
    e_pos, e_sc, cells = M.peaks(exp, _BLOCKS, method)
    assert pos.dtype == np.int64 and (pos == e_pos).all() and sc.dtype == np.float32 and sc.tobytes() == e_sc.tobytes()
    ox, oy = MTM.subpixel.fit_offsets(M.peak_neighbourhoods(exp, cells), method)
    assert fpos.dtype == np.float64 and (fpos == e_pos.astype(np.float64) + np.stack((ox, oy), axis=1)).all()
    assert fsc.tobytes() == e_sc.tobytes() and (ox != 0).any()
    assert [c[4:] for c in ctx.calls] == [(M.FIRST, False, True)] * 2
    # a margin past the frames: the planes of the frames' larger side
    pos, sc, pl = MTM.matchBlocksStack(frames, _BLOCKS[:2], 10 ** 6, method, ensemble=True, context=ctx)
    assert pl.shape == (2, 105, 105) and ctx.calls[-1][2] == 52


# ---- plane_peaks -------------------------------------------------------------------------------------------------------------
def test_plane_peaks_on_constructed_planes():
    nan = np.nan
    blocks = np.array([(10, 20, 4, 4), (0, 0, 3, 3), (7, 7, 2, 2), (30, 5, 6, 6)])
    pl = np.zeros((4, 5, 5), np.float32)
    pl[0, 1, 3] = pl[0, 3, 0] = pl[0, 1, 4] = 0.75              # a tie: the first cell in row-major order
    pl[1, :2] = nan                                             # NaN borders (a box clipped at the top and the left) ...
    pl[1, :, :2] = nan
    pl[1, 2:, 2:] = [[0.5, 0.25, 0.0], [0.25, 0.0, 0.0], [0.0, 0.0, 0.0]]      # ... with the peak next to them
    pl[2] = 0.5
    pl[2, 4, 4] = 0.875                                         # a peak in the plane's last cell
    pl[2, 4, 3], pl[2, 3, 4] = 0.625, 0.75
    pl[3] = -1.0
    pl[3, 2, 1], pl[3, 2, 2], pl[3, 2, 3], pl[3, 1, 2], pl[3, 3, 2] = 0.25, 0.5, 0.375, 0.125, 0.25
    pos, sc = B.plane_peaks(pl, blocks, 5)
    assert pos.dtype == np.int64 and pos.tolist() == [[11, 19], [0, 0], [9, 9], [30, 5]]
    assert sc.dtype == np.float32 and sc.tolist() == [0.75, 0.5, 0.875, 0.5]
    e_pos, e_sc, cells = M.peaks(pl, blocks, 5)
    assert (pos == e_pos).all() and sc.tobytes() == e_sc.tobytes()
    fpos, fsc = B.plane_peaks(pl, blocks, 5, refine=True)
    ox, oy = MTM.subpixel.fit_offsets(M.peak_neighbourhoods(pl, cells), 5)
    assert fpos.dtype == np.float64 and (fpos == pos + np.stack((ox, oy), axis=1)).all() and fsc.tobytes() == sc.tobytes()
    # a NaN (or the plane's edge) in an axis' three cells: no offset on that axis; plane 3 is fitted on both
    assert (fpos[1] == pos[1]).all() and (fpos[2] == pos[2]).all()
    assert fpos[3, 0] == 30 + 0.5 * (0.25 - 0.375) / ((0.25 - 1.0) + 0.375) and fpos[3, 1] == 5 + 0.5 * (0.125 - 0.25) / ((0.125 - 1.0) + 0.25)
    # the minimum for methods 0 and 1, its first cell on ties, NaN cells never
    lo = np.full((2, 3, 3), 9.0, np.float32)
    lo[0, 0, 0] = nan
    lo[0, 1, 2] = lo[0, 2, 0] = 2.0
    lo[1, 2, 1] = -np.inf
    for method in (0, 1):
        pos, sc = B.plane_peaks(lo, blocks[:2], method)
        assert pos.tolist() == [[11, 20], [0, 1]] and sc.tolist() == [2.0, -np.inf]
    pos, sc = B.plane_peaks(lo, blocks[:2], 3)
    assert pos.tolist() == [[10, 19], [-1, -1]] and sc.tolist() == [9.0, 9.0]
    # float64 planes (several calls' planes averaged on the host) are taken as their float32 rounding
    pos64, sc64 = B.plane_peaks(pl.astype(np.float64), blocks.tolist(), 5)
    assert (pos64 == e_pos).all() and sc64.dtype == np.float32 and sc64.tobytes() == e_sc.tobytes()
    pos, sc = B.plane_peaks(np.zeros((0, 3, 3), np.float32), [], 5, refine=True)
    assert pos.shape == (0, 2) and pos.dtype == np.float64 and sc.shape == (0,)


def test_plane_peaks_argument_errors():
    pl = np.zeros((2, 3, 3), np.float32)
    blocks = [(0, 0, 2, 2), (1, 1, 2, 2)]
    for bad in (np.zeros((2, 3, 4), np.float32), np.zeros((2, 4, 4), np.float32), np.zeros((3, 3), np.float32),
                np.zeros((2, 3, 3), np.int32)):
        with pytest.raises(ValueError, match="planes must be"):
            B.plane_peaks(bad, blocks, 5)
    for bad in (blocks[:1], [(0, 0, 2)], np.zeros((2, 4), np.float32)):
        with pytest.raises(ValueError, match="blocks must be"):
            B.plane_peaks(pl, bad, 5)
    with pytest.raises(ValueError, match="methods 0..5"):
        B.plane_peaks(pl, blocks, 6)
    with pytest.raises(ValueError, match="refine"):
        B.plane_peaks(pl, blocks, 5, refine=1)
    pl[1] = np.nan
    with pytest.raises(ValueError, match=r"planes\[1\] holds no number"):
        B.plane_peaks(pl, blocks, 5)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import build as mtm_build
    mtm_build.build()
    return _lib.load()


def test_header_declares_the_entry_point(lib):
    hdr = open(os.path.join(ROOT, "include", "mtm_hip.h")).read()
    assert "#define MTM_ABI_VERSION 9" in hdr and _lib.ABI_VERSION == 9 and lib.mtm_abi_version() == 9
    decl = re.search(r"int mtm_match_blocks_stack\(([^;]*)\);", hdr).group(1)
    assert len(decl.split(",")) == len(_lib.SYMBOLS["mtm_match_blocks_stack"][1]) == 16
    decl = re.search(r"int mtm_debug_plan_blocks_stack\(([^;]*)\);", hdr).group(1)
    assert len(decl.split(",")) == len(_lib.SYMBOLS["mtm_debug_plan_blocks_stack"][1]) == 14
    assert "#define MTM_BLOCKS_REF_PREVIOUS 0" in hdr and "#define MTM_BLOCKS_REF_FIRST 1" in hdr
    assert (_lib.BLOCKS_REF_PREVIOUS, _lib.BLOCKS_REF_FIRST) == (0, 1) == (M.PREVIOUS, M.FIRST)
    assert hasattr(lib, "mtm_match_blocks_stack") and hasattr(_lib.Context, "match_blocks_stack")
    assert "matchBlocksStack" in MTM.__all__ and MTM.matchBlocksStack is B.matchBlocksStack and "plane_peaks" in B.__all__


def test_null_context_is_refused_without_a_gpu(lib):
    out = np.zeros(2, dtype=_lib.HIT_DTYPE)
    px = np.zeros((8, 8), np.uint8)
    ptrs = (_lib.ctypes.c_void_p * 3)(px.ctypes.data, px.ctypes.data, px.ctypes.data)
    blk = _lib.block_records([(0, 0, 4, 4)])
    rc = lib.mtm_match_blocks_stack(None, ptrs, 3, 8, 8, 1, _lib.MTM_U8, 8, blk.ctypes.data, 1, 2, 5, 0, out.ctypes.data,
                                    None, None)
    assert rc == -1 and b"mtm_match_blocks_stack" in lib.mtm_last_error()
    assert not out["w"].any()


# ---- the host planner ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [M.PREVIOUS, M.FIRST])
def test_frame_chunks(lib, mode):
    for n_frames in range(2, 10):
        for per in range(2, 6):
            got, none = _lib.debug_plan_blocks_stack(n_frames, per, mode)
            exp = M.chunks(n_frames, per, mode)
            assert none is None and got.dtype == exp.dtype and got.shape == exp.shape and (got == exp).all(), (n_frames, per)
            pairs, uploads = [], []
            for f0, nf, carried, p0 in got.tolist():
                assert 1 <= nf and nf + 1 <= per                # the stack holds the carried frame and nf more
                stack = [carried] + list(range(f0, f0 + nf))
                uploads += stack[1:]
                for p in range(p0, p0 + nf):                    # both frames of every pair lie in its chunk's stack
                    r, s = M.pair_frames(n_frames, mode)[p]
                    assert r in stack and s in stack and stack.index(r) < stack.index(s)
                    if mode == M.PREVIOUS:
                        assert stack.index(s) == stack.index(r) + 1
                    pairs.append(p)
                assert carried == (0 if mode == M.FIRST else f0 - 1)
            assert pairs == list(range(n_frames - 1))           # every pair exactly once, in order
            assert uploads == list(range(1, n_frames))          # every frame once (frame 0 as the first carried frame)
            assert len(got) == -(-(n_frames - 1) // (per - 1))
    for bad in ((1, 2, mode), (3, 1, mode), (3, 2, 2), (3, 2, -1)):
        with pytest.raises(_lib.MtmError):
            _lib.debug_plan_blocks_stack(*bad)


def test_clip_offsets(lib):
    rng = np.random.RandomState(4)
    shape = (60, 75)
    blocks = [(0, 0, 5, 5), (70, 55, 5, 5), (3, 2, 8, 6), (64, 51, 8, 6), (30, 0, 4, 4), (0, 30, 4, 4), (20, 20, 9, 9),
              (0, 0, 75, 60)]
    for _ in range(40):
        w, h = int(rng.randint(1, 30)), int(rng.randint(1, 30))
        blocks.append((int(rng.randint(0, 75 - w + 1)), int(rng.randint(0, 60 - h + 1)), w, h))
    for chans, dtype in ((1, np.uint8), (3, np.uint8), (1, np.uint16)):
        for margin in (0, 1, 4, 7, 16, 100):
            _, got = _lib.debug_plan_blocks_stack(2, 2, 0, shape, chans, dtype, blocks, margin)
            exp = M.clip(shape, blocks, margin)
            assert got.dtype == exp.dtype and got.shape == exp.shape and (got == exp).all()
            # every output of a block's map has a cell in its plane
            _, _, _, maps = _lib.debug_plan_blocks(shape, chans, dtype, blocks, margin, 1 << 30)
            assert (got >= 0).all() and (got[:, 0] + maps[:, 2] <= 2 * margin + 1).all()
            assert (got[:, 1] + maps[:, 3] <= 2 * margin + 1).all()
    _, got = _lib.debug_plan_blocks_stack(2, 2, 0, shape, 1, np.uint8, blocks[:4], 4)
    assert got.tolist() == [[4, 4], [0, 0], [1, 2], [0, 0]]
    with pytest.raises(_lib.MtmError):
        _lib.debug_plan_blocks_stack(2, 2, 0, shape, 1, np.uint8, [(0, 0, 4, 4), (73, 0, 4, 4)], 4)
    assert b"block 1: block outside the reference" in lib.mtm_last_error()
