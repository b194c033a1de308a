"""
The masked float32 screen's model (tests/maskf32_model.py) on the CPU: on every cell and scene of the table the bounds
computed from the MODEL's raw sums contain the exact quality wherever that is finite, and the conditions that keep
tests/test_gpu_maskf32_screen.py from passing vacuously hold for the reference alone:

  * threshold mode, the class's threshold (maskf32_model.threshold_for: midway between the 0.9 quantile and the maximum of the
    exact qualities of the class's first template; templates share a class, one screen, where their masks are equal): at least one output is listed and at least half of the map gets a placeholder;
  * global mode: fewer than half of the outputs are listed;
  * every planted exact copy is listed, in both modes.

The first two apply to the scenes meant to have a live screen (noise+, signed, offset, step), per class, for both methods
and for one and three piece products, except where exempt() says the bound's own arithmetic rules them out, and on maps of
at least 16 outputs.  For
`huge`, `nonfinite` and the all-zero mask this file shows their stated expectation instead: everything affected is listed.
Every cell prints the share of its outputs that the model bounds list, for one and for three piece products.
"""
import numpy as np
import pytest

import f32_model as F
import maskf32_model as M


def exempt(scene, method, kind, pieces):
    """Where the liveness conditions cannot hold, by the bound's own arithmetic - everything else is asserted.
      * the all-zero mask: the map is one value by rule (NaN under TM_CCORR_NORMED, 0 under TM_SQDIFF) and listed entirely;
      * one live tap under TM_CCORR_NORMED: c1 / sqrt(tms c2) = +-1 at every output, no threshold splits the map;
      * ONE piece product on `offset` and `step`: the bound is 2^-7 of the norms' product.  On `offset` (sd / mean = 0.005) the
        qualities of a map spread over (sd / mean)^2 = 2.5e-5 while the bound is 2^-7 * 0.005 = 4e-5 wide; on `step` the windows
        beside the step are nearly flat on a tile constant half way up.  The one-product screen lists everything there and
        three products are what screens these scenes (launch_masked_bf16's ladder);
      * one live tap under TM_SQDIFF, with one piece product, and with three on `offset` and `step`: E1 and E2 are
        Cauchy-Schwarz over the WHOLE window - sum (I - mu)^2 over h w pixels against a single live weight u - so the
        interval is about 2 eps sqrt(h w) sd |u| wide while the map itself spreads over about sd |u| times the one pixel's
        difference: with eps = 2^-7 and h w = 35 .. 3201 that is 0.1 .. 0.9 of the spread (40 - 90 % of a `noise+` map listed,
        printed); with three products the class is live on `noise+` and `signed` (4 - 26 % listed) and asserted there, while on
        the two scenes whose windows vary least against their tile constant half a map can still be listed (26 - 68 %)."""
    if kind == "zero" or (kind == "one_tap" and method == M.CCORR_NORMED):
        return True
    if kind == "one_tap" and pieces == 1:
        return True
    if scene in ("offset", "step"):
        return pieces == 1 or kind == "one_tap"
    return False


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(cell, scene):
        key = (cell["name"], scene)
        if key not in cache:
            cache[key] = M.CellModel(cell, scene)
        return cache[key]
    return get


@pytest.mark.parametrize("cell", [c for c in M.CELLS if c["on_route"]], ids=[c["name"] for c in M.CELLS if c["on_route"]])
def test_model_bounds_contain_the_exact_quality_and_the_screen_is_live(models, cell):
    for scene in cell["scenes"]:
        cm = models(cell, scene)
        for method in M.METHODS:
            for g, (kind, members) in enumerate(cm.groups):
                thr = cm.threshold(method, g)
                line = []
                for pieces in (1, 3):
                    n_thr = n_glob = n_all = 0
                    for k in members:
                        lb, ub = cm.model_bounds(method, pieces, k)
                        q = cm.q(method, k)
                        lt, lg = M.listed_threshold(method, ub, thr), M.listed_global(lb, ub)
                        tag = (cell["name"], scene, method, pieces, kind, k)
                        fin = np.isfinite(q)
                        inside = M.contains(lb, ub, q)
                        # (a bound that is NaN does not exist - the raw sums of J = inf: such an output is listed)
                        assert lt[np.isnan(ub)].all() and lg[np.isnan(ub)].all(), tag
                        assert inside[fin].all(), tag + (int((fin & ~inside).sum()), np.argwhere(fin & ~inside)[:3].tolist())
                        # where the exact quality does not exist the output is listed
                        assert lt[~fin].all() and lg[~fin].all(), tag
                        if kind == "zero" and method == M.CCORR_NORMED:
                            assert lt.all() and lg.all() and np.isnan(q).all(), tag
                        elif kind == "zero" and scene not in ("nonfinite", "huge"):
                            assert np.array_equal(q, np.zeros_like(q)), tag
                        n_all += lt.size
                        n_thr += int(lt.sum())
                        n_glob += int(lg.sum())
                        for (t, y, x) in cm.plants:
                            if t == k:
                                assert lt[y, x] and lg[y, x], tag + ("planted copy not listed", y, x)
                    line.append("np%d thr %.4f global %.4f" % (pieces, n_thr / n_all, n_glob / n_all))
                    live = scene in M.SCENES_LIVE and not exempt(scene, method, kind, pieces)
                    # (maps of fewer than 16 outputs: "half of the map" is a handful of outputs either way - printed only)
                    if live and n_all >= 16 * len(members):
                        assert 1 <= n_thr <= n_all // 2, (cell["name"], scene, method, pieces, kind, "threshold", thr, n_thr, n_all)
                        assert n_glob < n_all / 2, (cell["name"], scene, method, pieces, kind, "global", n_glob, n_all)
                print("%s %s m%d %s thr=%.6g listed share: %s" % (cell["name"], scene, method, kind, thr, "; ".join(line)))


def test_nonfinite_and_huge_scenes_list_what_they_touch(models):
    """`nonfinite`: a window that holds the NaN or the +inf pixel is listed (its bound does not exist); `huge`: J = I^2
    overflows float32, an output whose window holds such a pixel is listed.  One exception, by the header's own rule: under
    TM_CCORR_NORMED an output whose c1 + E1 <= 0 (I itself is finite) has ub = 0 whatever c2 is - the quality's sign is
    settled; such an output may get a placeholder, and its exact quality is indeed below that bound."""
    seen = set()
    for cell in M.CELLS:
        for scene in cell["scenes"]:
            if scene not in ("nonfinite", "huge") or not cell["on_route"]:
                continue
            seen.add(scene)
            cm = models(cell, scene)
            J = M.square_f32(cm.img).astype(np.float64)
            with np.errstate(invalid="ignore", over="ignore"):
                bad = ~np.isfinite(M.window_sum(J, cm.h, cm.w))
            assert bad.any(), (cell["name"], scene)
            for method in M.METHODS:
                for g, (kind, members) in enumerate(cm.groups):
                    thr = cm.threshold(method, g)
                    for pieces in (1, 3):
                        for k in members:
                            lb, ub = cm.model_bounds(method, pieces, k)
                            q = cm.q(method, k)
                            for listed in (M.listed_threshold(method, ub, thr), M.listed_global(lb, ub)):
                                out = bad & ~listed
                                with np.errstate(invalid="ignore"):
                                    settled = (method == M.CCORR_NORMED) & (ub <= 4e-7) & (q <= ub)
                                assert not (out & ~settled).any(), (cell["name"], scene, method, pieces, k, int((out & ~settled).sum()))
    assert seen == {"nonfinite", "huge"}


def test_the_ladder_scene_lists_several_times_more_with_one_piece(models):
    """The capacity test's class (maskf32_model.LADDER): under TM_CCORR_NORMED the one-product bound lists several times more
    outputs than the three-product bound, so a capacity between the two counts shows the ladder."""
    name, scene, g = M.LADDER
    cm = models(next(c for c in M.CELLS if c["name"] == name), scene)
    counts = M.ladder_counts(cm, g)
    print("ladder class %s / %s / %s: listed with one piece product %d, with three %d" % (name, scene, cm.groups[g][0], counts[1], counts[3]))
    assert counts[1] >= 3 * counts[3] and counts[3] >= 4, counts


def test_the_table_covers_every_rule():
    on = [c for c in M.CELLS if c["on_route"]]
    assert {c["w"] for c in on if c["family"] == "taps"} == {7, 32, 33, 64, 65, 129, 255, 256}
    assert [c for c in M.CELLS if not c["on_route"]] and all(c["w"] > F.MAX_W for c in M.CELLS if not c["on_route"])
    assert {(c["h"], c["w"]) for c in on if c["family"] == "chunks"} == {(64, 33), (65, 33), (32, 97), (33, 97)}
    assert {c["h"] for c in on if c["family"] == "steps"} == {1, 2, 3, 67}
    assert {c["n"] for c in on if c["family"] == "lists"} == {1, 16, 17, 33}
    assert {c["out"] for c in on if c["family"] == "outputs"} == {(2, 2), (3, 7), (5, 9), (9, 127), (9, 128), (9, 129), (5, 257)}
    scenes = {s for c in on for s in c["scenes"]}
    assert scenes == {"noise+", "signed", "offset", "step", "tiny", "huge", "nonfinite"}
    # every mask occurs in every cell that is no list, and every mask under some list
    assert all([k for k, _ in M.mask_groups(c, s)] == list(M.MASKS) for c in on if not c["n"] for s in c["scenes"])
    assert {M.mask_groups(c, s)[0][0] for c in on if c["n"] for s in c["scenes"]} >= {"disc", "uniform", "signed", "large"}


def test_the_restated_constants_are_the_sources():
    """The constants this model restates are the ones in the sources (a changed constant must change the model)."""
    import os
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "multitemplatematching-python_amd", "csrc")
    src = open(os.path.join(root, "mtm_maskf32.hip.h")).read()
    for text in ("* 1.000002 + 3e-7 * fabs(c1) + 1e-30", "* 1.000002 + 6e-7 * fabs(c2) + 1e-30",
                 "4e-7 * (2.0 * fabs(c1) + fabs(c2) + fabs(tms))", "4e-7 * fmax(1.0, fabs(*ub))", "4e-7 * fmax(1.0, fabs(*lb))",
                 "* 1.000001 + 1e-12 * (fabs(s2i) + area * mi * mi)", "(size_t)(y / kBfRows) * p.nseg + x / kBfSeg"):
        assert text in src, text
