"""
The two callers of the peak launchers (csrc/mtm_peaks.hip) against each other (-m gpu): a search call - queue_peak_pass,
the extremum pass - and the test entry mtm_debug_peak_pass on the search's own score maps.

tests/test_gpu_peaks.py sweeps the launchers through the test entry alone; here a search whose maps stay in memory takes the
same launcher (peaks_kernel for local extrema, extremum_kernel for the global one), its maps are fetched with
mtm_last_score_map and handed to the entry, and the two record sets must be equal.  The image is the integer hash formula
of tools/fm_end_routes.py at 150 x 300 (no random generator); the three templates' maps are 139 x 285, 111 x 293 and
146 x 271: two strip columns of 256, two strip rows of 128, the largest height and the largest width on different maps.
MTM_KERNEL_DOT4 keeps every class off the MFMA kernel, so nothing is fused and the maps are in memory (asserted through
timing()["kernel_used"]).

No tolerance: both sides run the same kernel on the same floats.  Records are compared as sets, byte for byte.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS, COLS = 150, 300
CUTS = (((12, 16), (7, 11)), ((40, 8), (60, 200)), ((5, 30), (100, 100)))       # ((h, w), (y, x))
TM_SQDIFF_NORMED, TM_CCOEFF_NORMED = 1, 5


def _noise():
    yy, xx = np.mgrid[0:ROWS, 0:COLS].astype(np.uint64)
    h = (yy * np.uint64(73856093)) ^ (xx * np.uint64(19349663))
    h = (h * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    return ((h >> np.uint64(13)) & np.uint64(0xFF)).astype(np.uint8)


@pytest.fixture(scope="module")
def lib():
    import build as mtm_build
    mtm_build.build()
    from MTM import _lib
    assert _lib.load().mtm_device_count() >= 1
    return _lib


@pytest.fixture(scope="module")
def scene():
    img = _noise()
    templ = [np.ascontiguousarray(img[y:y + h, x:x + w]) for (h, w), (y, x) in CUTS]
    hw = [s for s, _ in CUTS]
    shapes = [(ROWS - h + 1, COLS - w + 1) for h, w in hw]
    assert shapes == [(139, 285), (111, 293), (146, 271)]
    return img, [(t, None) for t in templ], hw, shapes


def _search(lib, scene, method, mode, thr, border):
    """one search on the dot4 kernel (maps in memory) -> its hits, its maps, the context"""
    img, units, hw, shapes = scene
    c = lib.Context(0)
    c.set_option(lib.OPT_KERNEL, lib.KERNEL_DOT4)
    c.set_option(lib.OPT_PEAK_BORDER, border)
    hits = c.search(units, img, method, mode, thr)
    assert c.timing()["kernel_used"] == lib.KERNEL_DOT4
    maps = [c.last_score_map(t, shapes[t]) for t in range(len(units))]
    return hits, maps, c


def _sorted(a):
    return sorted(r.tobytes() for r in a)


@pytest.mark.parametrize("border", [0, 1], ids=["constant", "nearest"])
@pytest.mark.parametrize("method,thr", [(TM_CCOEFF_NORMED, 0.5), (TM_SQDIFF_NORMED, 0.3)], ids=["ccoeff_normed", "sqdiff_normed"])
def test_local_extrema_of_a_search_equal_the_entrys_scan(lib, scene, method, thr, border):
    mode_min = method == TM_SQDIFF_NORMED
    hits, maps, c = _search(lib, scene, method, lib.PEAKS_LOCAL, thr, border)
    try:
        res = c.debug_peak_pass(maps, lib.PEAK_SCAN, thr, mode_min=mode_min, border=border, templ_hw=scene[2],
                                hit_cap=len(hits) + 64)
    finally:
        c.close()
    print("method %d border %d: search %d hits, entry count %d, trivial %s" % (method, border, len(hits), res["count"],
                                                                             res["trivial"].tolist()))
    assert len(hits) > 0                                    # (the exact cuts at least)
    assert res["count"] == len(hits)
    assert not res["trivial"].any()
    rec = res["records"][:res["count"]]
    rec = rec[~res["trivial"].astype(bool)[rec["templ_idx"]]]       # as drop_trivial_maps: a trivial map's records go
    assert _sorted(rec) == _sorted(hits)


@pytest.mark.parametrize("method", [TM_CCOEFF_NORMED, TM_SQDIFF_NORMED], ids=["ccoeff_normed", "sqdiff_normed"])
def test_global_extremum_of_a_search_equals_the_entrys(lib, scene, method):
    minima = method == TM_SQDIFF_NORMED
    hits, maps, c = _search(lib, scene, method, lib.PEAKS_GLOBAL, 0.0, 1)
    try:
        res = c.debug_peak_pass(maps, lib.PEAK_EXTREMUM, 0.0, mode_min=minima, templ_hw=scene[2])
    finally:
        c.close()
    assert len(hits) == len(maps)
    for t in range(len(maps)):
        assert hits[t].tobytes() == res["ext_hits"][t][1 if minima else 0].tobytes(), t
