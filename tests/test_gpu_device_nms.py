"""
The device's share of the non-maxima suppression - nms_count_kernel, nms_offsets_kernel, nms_scatter_kernel,
nms_champion_kernel, nms_prune_kernel (csrc/mtm_k_nms.hip.h) - on constructed hit lists, against a plain greedy reference in
exact rational arithmetic (-m gpu).

Through a search the kernels only ever see the peaks a smooth image produces, on one grid of 276 cells of side 32.
Context.debug_device_nms (mtm_debug_device_nms) hands the very chain the search call queues a list of the test's choosing:
the table of tests/nms_model.py (validated on the CPU by tests/test_nms_model_cpu.py) - grids of 276, 1024, 1025 and 3000
cells (one, two and three cells per thread of the prefix kernel), cells of 33, 100 and 257 (a template's side, not the floor
of 32), 3-wide grids, hits at the image's corners and on both sides of cell borders, 1 .. 300 hits in one cell, candidate
counts on both sides of the 8-per-wave and 32-per-block turns, n_max = 256 (several turns of the grid-stride loops), the gate
[n_min, n_max], chains, hits that are no candidates, ties at every level of the order, overlap limits that pairs hit exactly,
a few hundred random clustered lists.

No tolerance anywhere: the champions and the undecided hits the device returns are compared with the reference's sets as
sorted records (the order inside each part depends on atomics), and greedy NMS over the returned list, the champions taken
as kept, must give the reference's greedy records byte for byte.  One context runs the whole table, its work buffers
poisoned before each geometry.
"""
import collections
import ctypes

import numpy as np
import pytest

import nms_model as M

pytestmark = pytest.mark.gpu

_SENTINEL = 0xA5


@pytest.fixture(scope="module")
def lib():
    import build as mtm_build
    mtm_build.build()
    from MTM import _lib
    assert _lib.load().mtm_device_count() >= 1
    assert _lib.HIT_DTYPE == M.HIT_DTYPE
    return _lib


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


GROUPS = collections.OrderedDict()
for _c in M.CASES:
    GROUPS.setdefault((_c.rows, _c.cols, _c.max_side), []).append(_c)


def _records(a):
    return sorted(r.tobytes() for r in a)


def run_case(ctx, c):
    """one call of the device chain on the case's list; every assertion of the sweep"""
    ref = M.case_reference(c.name)
    out = np.frombuffer(bytes([_SENTINEL]) * (M.HIT_DTYPE.itemsize * (len(c.hits) + 3)), dtype=M.HIT_DTYPE).copy()
    untouched = out.tobytes()
    champions, undecided = ctx.debug_device_nms(c.hits, c.rows, c.cols, c.max_side, c.score_threshold, c.max_overlap,
                                                ascending=c.ascending, n_min=c.n_min, n_max=c.n_max, out=out)
    if not c.runs:                  # outside [n_min, n_max]: the kernels do nothing
        assert (len(champions), len(undecided)) == (0, 0), c.name
        assert out.tobytes() == untouched, c.name
        return
    assert (len(champions), len(undecided)) == (len(ref.champions), len(ref.undecided)), c.name
    got_c, got_u = _records(champions), _records(undecided)
    assert len(set(got_c + got_u)) == len(got_c) + len(got_u), c.name               # nothing twice
    assert got_c == _records(ref.champions), c.name
    assert got_u == _records(ref.undecided), c.name
    assert out[len(champions) + len(undecided):].tobytes() == untouched[:M.HIT_DTYPE.itemsize * (len(out) - len(got_c) - len(got_u))], c.name
    kept = M.greedy(undecided, c.score_threshold, c.ascending, c.max_overlap, sure=champions)
    assert kept.tobytes() == ref.greedy.tobytes(), c.name


@pytest.mark.parametrize("k", range(len(GROUPS)), ids=["%dx%d-side%d" % g for g in GROUPS])
def test_device_nms_table(ctx, k):
    geom = list(GROUPS)[k]
    ctx.debug_poison(0xFF if k % 2 else 0x7F, 4)
    for c in GROUPS[geom]:
        run_case(ctx, c)


def test_every_case_of_the_table_is_run():
    assert sum(len(g) for g in GROUPS.values()) == len(M.CASES) >= 300
    assert {(c.rows, c.cols, c.max_side) for c in M.CASES if c.name.startswith("geo-")} <= set(GROUPS)


def test_each_call_returns_its_own_result(ctx):
    """a 3000-cell grid, a 276-cell one, the 3000-cell one again with another list, short launches in between: nothing of
    an earlier call's cell counts, ranks, sorted records or status words may show in a later one"""
    for name in ("random-long", "geo-cells276-ov0", "geo-cells3000-ov0", "turns-nmax256-1", "turns-nmax256-2", "cellrun-300-ov0.6",
                 "geo-cells3000-ov0.3", "gate-below-nmin", "random-long", "all-below-threshold", "geo-cells276-ov0.3"):
        run_case(ctx, M.CASE_BY_NAME[name])


def test_empty_list_and_refused_arguments(lib, ctx):
    """(all of these are refused or do nothing before a kernel could go wrong)"""
    empty = np.zeros(0, dtype=M.HIT_DTYPE)
    for n_min in (0, 1):
        champions, undecided = ctx.debug_device_nms(empty, 300, 640, 32, 0.5, 0.3, n_min=n_min, n_max=256)
        assert (len(champions), len(undecided)) == (0, 0)
    fn = lib.load().mtm_debug_device_nms
    c = M.CASE_BY_NAME["count-9"]
    n = len(c.hits)
    out = np.zeros(n, dtype=M.HIT_DTYPE)
    nc, nu = ctypes.c_int64(-7), ctypes.c_int64(-7)

    def call(handle=ctx._h, hits=c.hits.ctypes.data, n=n, rows=300, cols=640, side=32, ov=0.3, n_min=1, n_max=4096, out=out.ctypes.data, cap=n):
        return fn(handle, hits, n, rows, cols, side, 0.5, 0, ov, n_min, n_max, out, cap, ctypes.byref(nc), ctypes.byref(nu))

    assert call() == 0 and nc.value + nu.value > 0
    nc.value = nu.value = -7
    for bad in (dict(handle=None), dict(n=-1), dict(rows=0), dict(cols=-5), dict(side=-1), dict(ov=-0.1), dict(ov=float("nan")),
                dict(n_min=-1), dict(n_max=0), dict(n_max=(1 << 18) + 1), dict(cap=n - 1), dict(cap=-1), dict(hits=None),
                dict(out=None)):
        assert call(**bad) == -1, bad                   # MTM_E_INVALID
        assert (nc.value, nu.value) == (-7, -7), bad
    assert call(n_min=n + 1, cap=0, out=None) == 0 and (nc.value, nu.value) == (0, 0)      # outside the gate: no capacity needed
