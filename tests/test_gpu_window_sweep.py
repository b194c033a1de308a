"""
The exact-integer window kernels at their chunk and tile edges, against exact sums (-m gpu).

Five features stand on one family of device code - win_score_tile<CH, U16> (csrc/mtm_k_window.hip.h: boxes_score_kernel,
track_score_kernel, track_reacquire_kernel, the blocks_* kernels, phase 1 of pyr_window_kernel), its fused copies
win_tile_sums_u8_set / win_tile_sums_u16_set (the set kernels of tracking, kTrackNV = 4) and the split-K copy sub_nbhd_int
with the float kinds of sub_nbhd_kernel (csrc/mtm_k_nbhd.hip.h, csrc/mtm_subpixel.hip) - and the rest of the suite mostly
holds the family's members to each other.  Here every cell of tests/window_cases.py goes through a public entry point and is
compared with mtm_oracle.match_template(..., corr="direct") alone: whole planes (P), every record (B, T), all nine values of
every point (N), every hit (Y), float32 bit for bit, NaN with NaN, no tolerance, nothing excluded.  What the cells are and why
bit for bit holds: tests/window_cases.py; that the table is honest: tests/test_window_cases_cpu.py.

Every cell runs twice in consecutive tests, so that both poison patterns of the suite's fixture (0xFF, 0x7F) precede it.
Measured on an MI355X: docs/HISTORY.md and profiles/window_sweep/sweep.txt; what each cell is sensitive to:
profiles/window_sweep/mutants.txt.
"""
import time

import numpy as np
import pytest

import window_cases as C

pytestmark = pytest.mark.gpu

_RAN = {}
TWICE = (0, 1)


def _cells(f):
    return [pytest.param(c, id=c["name"][2:]) for c in C.family(f)]


@pytest.fixture(scope="module")
def MTM():
    import build as mtm_build
    mtm_build.build()
    import MTM as pkg
    assert pkg._lib.load().mtm_device_count() >= 1
    return pkg


def _ran(cell, run, t_start):
    _RAN[(cell["name"], run)] = time.perf_counter() - t_start


def _differs(name, what, got, ref):
    bad = np.argwhere(~C.same_bits(got, ref))
    assert len(bad) == 0, "%s %s: %d of %d values differ, first at %s: %r / %r" % (
        name, what, len(bad), ref.size, tuple(bad[0]), got[tuple(bad[0])], ref[tuple(bad[0])])


# ---- P: whole planes -----------------------------------------------------------------------------------------------------
def _p_data(cell):
    key = ("P", cell["name"])
    if key not in C._DATA:
        img, calls, blocks, temps, kinds = C.p_scene(cell)
        C._DATA[key] = (img, calls, blocks, kinds, C.p_expected(cell, img, blocks, temps)[0])
    return C._DATA[key]


@pytest.mark.parametrize("run", TWICE)
@pytest.mark.parametrize("cell", _cells("P"))
def test_block_planes(MTM, cell, run):
    t_start = time.perf_counter()
    img, calls, blocks, kinds, planes = _p_data(cell)
    m = cell["margin"]
    for method in cell["methods"]:
        for ref, group in calls:
            _, _, got = MTM.matchBlocksStack([ref, img], [blocks[k] for k in group], m, method, ensemble=True)
            assert got.dtype == np.float32 and got.shape == (len(group), 2 * m + 1, 2 * m + 1)
            for i, k in enumerate(group):
                _differs(cell["name"], "block %d at %r (%s), method %d" % (k, blocks[k][:2], kinds[k], method), got[i],
                         planes[method][k])
    _ran(cell, run, t_start)


# ---- B: records of findMatchesInBoxes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", TWICE)
@pytest.mark.parametrize("cell", _cells("B"))
def test_box_records(MTM, cell, run):
    t_start = time.perf_counter()
    img, temps, regions, _ = C.b_scene(cell)
    lib = MTM._lib
    ctx = lib.Context(0) if cell["mode"] == "local" else None       # (the border option: a context of the test's own)
    try:
        if ctx is not None:
            ctx.set_option(lib.OPT_PEAK_BORDER, {"constant": 0, "nearest": 1}[cell["border"]])
        for method in cell["methods"]:
            exp = C.b_expected(cell, method)
            if cell["mode"] == "global":
                got = MTM.findMatchesInBoxes(temps, img, regions, method, N_object=1)
            else:
                got = MTM.findMatchesInBoxes(temps, img, regions, method, score_threshold=C.local_threshold(method), context=ctx)
            assert len(got) == len(exp)
            bad = [i for i, (g, e) in enumerate(zip(got, exp)) if C.records(g) != e]
            assert not bad, "%s method %d: %d of %d units differ, first unit %d (template %r): %r / %r" % (
                cell["name"], method, len(bad), len(exp), bad[0], temps[bad[0]][1].shape[:2], C.records(got[bad[0]])[:3],
                exp[bad[0]][:3])
    finally:
        if ctx is not None:
            ctx.close()
    _ran(cell, run, t_start)


# ---- T: records of trackTemplates ------------------------------------------------------------------------------------------
T_MARGIN = 4


@pytest.mark.parametrize("run", TWICE)
@pytest.mark.parametrize("cell", _cells("T"))
def test_track_records(MTM, cell, run):
    t_start = time.perf_counter()
    frames, temps, tracks, _, min_score, reacquire = C.t_scene(cell)
    for method in cell["methods"]:
        exp = C.t_expected(cell, method, T_MARGIN)
        got = MTM.trackTemplates(temps, frames, tracks, T_MARGIN, method,
                                 min_score=C.never_passes(method) if min_score else None, reacquire=reacquire)
        assert len(got) == len(frames)
        for f, (grow, erow) in enumerate(zip(got, exp)):
            grow = [C.records(g)[0] if len(g) == 1 else tuple(g) for g in grow]
            bad = [k for k, (g, e) in enumerate(zip(grow, erow)) if g != e]
            assert len(grow) == len(erow), (cell["name"], method, f, len(grow), len(erow))
            assert not bad, "%s method %d frame %d: %d of %d tracks differ, first track %d (set %r): %r / %r" % (
                cell["name"], method, f, len(bad), len(erow), bad[0], tracks[bad[0]][1], grow[bad[0]], erow[bad[0]])
    _ran(cell, run, t_start)


# ---- N: whole maps of the neighbourhood kernel ------------------------------------------------------------------------------
def _n_data(cell):
    key = ("N", cell["name"])
    if key not in C._DATA:
        img, temps, kinds = C.n_scene(cell)
        C._DATA[key] = (img, temps, kinds, [C.n_expected(cell, img, e)[0] for e in temps])
    return C._DATA[key]


@pytest.mark.parametrize("run", TWICE)
@pytest.mark.parametrize("cell", _cells("N"))
def test_neighbourhood_maps(MTM, cell, run):
    t_start = time.perf_counter()
    img, temps, kinds, exp = _n_data(cell)
    hits = [h for e in temps for h in C.n_hits(cell, e[0])]
    n = C.N_MAP[0] * C.N_MAP[1]
    for method in cell["methods"]:
        got = MTM.hitNeighbourhoods(temps, img, hits, method)
        assert got.dtype == np.float32 and got.shape == (len(temps) * n, 3, 3)
        for i, kind in enumerate(kinds):
            _differs(cell["name"], "template %d (%s), method %d, (point, dy, dx)" % (i, kind, method), got[i * n:(i + 1) * n],
                     exp[i][method])
    _ran(cell, run, t_start)


# ---- Y: hits of findMatchesPyramid ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", TWICE)
@pytest.mark.parametrize("cell", _cells("Y"))
def test_pyramid_hits(MTM, cell, run):
    t_start = time.perf_counter()
    img, temps, places = C.y_scene(cell)
    key = ("Y", cell["name"])
    if key not in C._DATA:
        C._DATA[key] = [C.direct_maps(img, t, cell["methods"]) for _, t in temps]
    maps = C._DATA[key]
    label_of = {lab: i for i, (lab, _) in enumerate(temps)}
    for method in cell["methods"]:
        thr, coarse = C.y_thresholds(method)
        hits = MTM.findMatchesPyramid(temps, img, cell["factor"], method, score_threshold=thr, coarse_threshold=coarse,
                                      radius=cell["radius"])
        found = {(lab, y, x) for lab, (x, y, _, _), _ in hits}
        missing = [("t%d" % i, y, x) for i, (y, x) in enumerate(places) if ("t%d" % i, y, x) not in found]
        assert not missing, (cell["name"], method, missing, len(hits))      # (every planted window is scored and is a hit)
        for lab, (x, y, w, h), s in hits:
            assert (h, w) == (cell["h"], cell["w"])
            assert C.bits(s) == C.bits(maps[label_of[lab]][method][y, x]), (cell["name"], method, lab, x, y, s)
    _ran(cell, run, t_start)


def test_the_sweep_ran_every_family():
    """On what ran in this session: a summary line and the per-cell record (-s), and no family of the table without a
    cell - when the whole module ran."""
    if not _RAN:
        return
    slow = max(_RAN, key=_RAN.get)
    print("window sweep: %d cell runs in %.1f s, slowest %s (run %d) %.2f s" % (len(_RAN), sum(_RAN.values()), slow[0], slow[1],
                                                                             _RAN[slow]))
    for fam in "PBTNY":
        t = [v for (name, _), v in _RAN.items() if name.startswith(fam + "-")]
        print("  family %s: %d cell runs, %.1f s" % (fam, len(t), sum(t)))
    for (name, run), v in sorted(_RAN.items()):
        print("  %-40s run %d %.3f s" % (name, run, v))
    if len(_RAN) == 2 * len(C.CELLS):
        assert {c["family"] for c in C.CELLS} == {name[0] for name, _ in _RAN}
