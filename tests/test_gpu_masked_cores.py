"""
Masked uint8 classes on ncc_mfma_kernel: masks, range and geometry of the sum I^2 M pass against exact sums (-m gpu).

The table, the scenes and the references are tests/masked_cores_cases.py (read its docstring first);
tests/test_masked_cores_cpu.py proves their preconditions without a GPU.  Here every cell runs in a context of its own, from
memory poisoned with 0xFF and with 0x7F:

  read-out cells   TM_SQDIFF under an all-zero template is float32(sum I^2 M): last_score_map of a map-mode search and
                   score_map (the single-template launch) equal the integer sums, every output, bit for bit;
  range cells      ... and again with MTM_MASKSQ_FUSED=0 (two raw launches + masksq_combine_kernel), MTM_ROW_MUX=0 and
                   MTM_FUSE_STATS=0 (the dot4 MASKSQ pass): every route gives the same integers;
  full scores      all four masked methods, whole maps of every template against mtm_oracle.match_template(..., mask=...,
                   corr="direct") by the rule test_gpu_tilings.py has for masked classes - |got - ref| <= 1e-6 max(1, |ref|),
                   NaN meets NaN, no output skipped - in IEEE and in reciprocal division mode; on methods 1 and 3 the
                   hits-only records equal map mode's byte for byte at the threshold that lists every live template
                   (best -+ 4e-4), the `black` scenes with their blocks of sum I^2 M = 0 included.

Route, under default routes: class_tilings()[0]["kernel"] is the matrix-core kernel (the float64 kernel for the two range rows
off the cores, as the masked_off_cores cells of the tilings sweep), and timing()["sq_launches"] == 1: the counter counts the
sum I^2 M PASSES of a call, one per masked class on the cores, in either form (launch_masked_sumsq brackets the fused launch,
or the two raw launches and the combine kernel, with ONE event pair); 0 off the cores.  Under the switches only results are
asserted.

What the sweep found.  The fused pass accumulates 256 a_h + a_l in int32, which reaches -32896 n under a mask of n set taps:
beyond n = 65280 dark windows cannot be held, while masked classes are admitted up to 66051 taps.  At the commit before
kMasksqFusedMaxOnes, on an MI355X, the range cells of 65536 and 66048 set taps returned sum I^2 M + 2^32 for every output of
the `dark` and `black` scenes ("range-256x256-o9x41-ones-dark search 0xff: 369 of 369 outputs differ ... first 4299546600.0 /
4579485.0"), the cell of 65281 set taps for the one window over the zero patch (4294967300.0 / 0.0), and the cells at 65280
and below passed; the full-score cells at 256 x 256 and 258 x 256 had TM_SQDIFF 4298250000 for 3282781, TM_SQDIFF_NORMED
297.5 for 4.33, and TM_CCORR_NORMED 0 where the oracle has 0 / 0.  Masks of more than 65280 set taps now take the unfused
form, which combines in float64; the other three routes (MTM_MASKSQ_FUSED=0, MTM_ROW_MUX=0, MTM_FUSE_STATS=0) were right
before and after.
"""
import time

import numpy as np
import pytest

import masked_cores_cases as C
from test_gpu_tilings import default_routes, lib          # noqa: F401  (lib: the module-scoped fixture that builds and loads)

pytestmark = pytest.mark.gpu

_RAN = {}
_SWITCHES = ("MTM_MASKSQ_FUSED", "MTM_ROW_MUX", "MTM_FUSE_STATS")


def _check_route(ctx, cell, d):
    recs = ctx.class_tilings()
    assert len(recs) == 1, (cell["name"], recs)
    r, tm = recs[0], ctx.timing()
    kernel, sq, _ = C.expected_route(cell, d["n_set"])
    assert (r["h"], r["w"], r["n_templates"]) == (cell["h"], cell["w"], cell["n"]), (cell["name"], r)
    assert (r["kernel"], tm["sq_launches"]) == (kernel, sq), (cell["name"], r, tm)


def _wrong(cell, what, got, ref, same):
    bad = np.argwhere(~same)
    assert len(bad) == 0, "%s %s: %d of %d outputs differ, columns %s rows %s, first %r / %r" % (
        cell["name"], what, len(bad), got.size, sorted(set(bad[:, 1].tolist()))[:12], sorted(set(bad[:, 0].tolist()))[:6],
        got[tuple(bad[0])], ref[tuple(bad[0])])


def _read_out(lib, cell, routes):
    t0 = time.perf_counter()
    d = C.cell_data(cell)
    ref, out = d["refs"][0][0], cell["out"]
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)                                                  # noqa: E731
    ctx = lib.Context(0)
    try:
        ctx.set_option(lib.OPT_HITS_ONLY, 0)
        ctx.set_option(lib.OPT_EXACT_DIV, 1)
        for pattern in (0xFF, 0x7F):
            ctx.debug_poison(pattern, 7)
            ctx.search(d["units"], d["img"], 0, lib.PEAKS_LOCAL, -1.0)          # nothing listed: the map is what is checked
            if routes:
                _check_route(ctx, cell, d)
            got = ctx.last_score_map(0, out)
            _wrong(cell, "search %#x" % pattern, got, ref, bits(got) == bits(ref))
            ctx.debug_poison(pattern, 7)
            got = ctx.score_map(0, out)
            if routes:
                _check_route(ctx, cell, d)
            _wrong(cell, "score_map %#x" % pattern, got, ref, bits(got) == bits(ref))
    finally:
        ctx.close()
    return time.perf_counter() - t0


@pytest.mark.parametrize("cell", C.READOUT, ids=[c["name"] for c in C.READOUT])
def test_read_out_cell(lib, cell):
    _RAN[cell["name"]] = _read_out(lib, cell, default_routes())


@pytest.mark.parametrize("switch", _SWITCHES)
@pytest.mark.parametrize("cell", C.RANGE, ids=[c["name"] for c in C.RANGE])
def test_range_cell_on_the_other_routes(lib, cell, switch, monkeypatch):
    monkeypatch.setenv(switch, "0")                      # (read when the context is created)
    _read_out(lib, cell, False)


@pytest.mark.parametrize("cell", C.SCORE, ids=[c["name"] for c in C.SCORE])
def test_full_score_cell(lib, cell):
    t0 = time.perf_counter()
    routes = default_routes()
    d = C.cell_data(cell)
    n, out, units, img, kinds = cell["n"], cell["out"], d["units"], d["img"], d["kinds"]
    live = [i for i, k in enumerate(kinds) if k != "mzero"]
    ctx = lib.Context(0)
    try:
        for method in cell["methods"]:
            normed, lower = method in (1, 3), method in (0, 1)
            thr0 = 0.5 if normed else (-1.0 if method == 0 else 1e30)
            ctx.set_option(lib.OPT_HITS_ONLY, 0)
            best = {}
            for exact, pattern in ((1, 0xFF), (1, 0x7F), (0, 0xFF)):
                ctx.set_option(lib.OPT_EXACT_DIV, exact)
                ctx.debug_poison(pattern, 7)
                ctx.search(units, img, method, lib.PEAKS_LOCAL, thr0)
                if routes:
                    _check_route(ctx, cell, d)
                for i in range(n):
                    got, ref = ctx.last_score_map(i, out), d["refs"][method][i]
                    with np.errstate(invalid="ignore"):
                        same = (np.abs(got.astype(np.float64) - ref) <= 1e-6 * np.maximum(1.0, np.abs(ref))) | \
                               (np.isnan(got) & np.isnan(ref)) | (got == ref)
                    _wrong(cell, "method %d exact_div %d pattern %#x template %d (%s)" % (method, exact, pattern, i, kinds[i]), got, ref, same)
                    if exact and pattern == 0xFF and normed and i in live:
                        best[i] = float(np.nanmin(got) if lower else np.nanmax(got))
            if not normed:
                continue
            # hits-only against map mode (just checked against exact sums), IEEE division, records byte for byte
            ctx.set_option(lib.OPT_EXACT_DIV, 1)
            thr = max(best.values()) + 4e-4 if lower else min(best.values()) - 4e-4
            ctx.set_option(lib.OPT_HITS_ONLY, 0)
            ref = ctx.search(units, img, method, lib.PEAKS_LOCAL, thr).copy()
            ctx.set_option(lib.OPT_HITS_ONLY, 1)
            for pattern in (0xFF, 0x7F):
                ctx.debug_poison(pattern, 7)
                got = ctx.search(units, img, method, lib.PEAKS_LOCAL, thr).copy()
                assert got.tobytes() == ref.tobytes(), (cell["name"], method, thr, pattern, len(got), len(ref))
            assert set(ref["templ_idx"].tolist()) >= set(live), (cell["name"], method, thr, sorted(set(live) - set(ref["templ_idx"].tolist())))
    finally:
        ctx.close()
    _RAN[cell["name"]] = time.perf_counter() - t0


def test_the_sweep_ran_every_family():
    """On what ran in this session: a summary line (-s), and no family of the table without a cell - when the whole module
    ran."""
    if not _RAN:
        return
    slow = max(_RAN, key=_RAN.get)
    print("masked cores: %d cells in %.1f s, slowest %s %.2f s" % (len(_RAN), sum(_RAN.values()), slow, _RAN[slow]))
    if len(_RAN) == len(C.CELLS):
        assert {c["family"] for c in C.CELLS} == {c["family"] for c in C.CELLS if c["name"] in _RAN}
