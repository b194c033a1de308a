"""
tests/f32_model.py on the CPU: the model of ncc_bf16_kernel's arithmetic against the oracle's direct float64 sums, on the
scenes of every cell of tests/test_gpu_f32_geometry.py - the conditions the GPU sweep relies on, shown without a GPU:

  * the model stays within bound_map of O.match_template(..., corr="direct"), with three piece products and with one;
  * at least 99 % of every map is compared (|score| < 1 in both maps, window not flat; an exact copy's own position, where the
    score IS 1, not counted), so a cell cannot pass by comparing nothing;
  * which scenes a method cannot use, and why.
"""
import numpy as np
import pytest

import f32_model as F
import mtm_oracle as O
import test_gpu_f32_geometry as G


def _lanes_shuffle_sum(v):
    """The kernel's loop on 64 lanes, lane by lane: __shfl_down(v, off) of lane l is lane l + off's value, its own beyond 63."""
    v = [np.float32(x) for x in v]
    off = 32
    while off:
        v = [np.float32(v[l] + (v[l + off] if l + off < 64 else v[l])) for l in range(64)]
        off >>= 1
    return v[0]


def test_tree_sum_is_the_shuffle_trees_order():
    rng = np.random.default_rng(1)
    differs = 0
    for k in range(200):
        v = (rng.normal(100.0, 40.0, 64) * 10.0 ** rng.integers(-3, 4)).astype(np.float32)
        assert F.tree_sum(v).tobytes() == _lanes_shuffle_sum(v).tobytes()
        differs += F.tree_sum(v) != np.float32(np.cumsum(v)[-1])
    assert differs > 0                  # (a sequential sum is another order on random data too)
    # constructed: lanes 0 and 32 cancel in the tree's first step; any order that adds a small lane to 2^24 first loses it
    v = np.zeros(64, np.float32)
    v[0], v[32], v[1:32] = 2.0 ** 24, -2.0 ** 24, 1.0
    assert F.tree_sum(v) == _lanes_shuffle_sum(v) == 31.0
    assert np.float32(np.cumsum(v)[-1]) != 31.0
    # ... and mu moves with it: every piece of the tile would round differently
    plane = np.tile(v.reshape(8, 8), (1, 1))
    assert F.tile_mu(plane, 0, 0, 6, 8) == np.float32(31.0 / 64.0)


def test_pieces_are_bfloat16_round_to_nearest_even():
    v = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.1415927, 1e-30, 65504.0], np.float32)
    v0, v1 = F.pieces_of(v)
    assert v0[0] == 1.0 and v0[1] == 1.0 and v0[2] == np.float32(1.0 + 2.0 ** -6) and v0[3] == np.float32(1.0 + 2.0 ** -7)
    assert ((v0.view(np.uint32) | v1.view(np.uint32)) & 0xFFFF == 0).all()
    assert (np.abs(v.astype(np.float64) - v0 - v1) <= 2.0 ** -16 * np.abs(v)).all()


def test_rig_eps_restates_the_headers_constants():
    # mtm_ctx.h::bf16_rig_eps at three points, computed by hand from its two return statements
    assert F.rig_eps(1, 64, 2, 3) == float(np.float32(2.0 * (3.0518e-5 + 2.0 * 3.0 * 1 * 64 * 2 * 5.97e-8)))
    assert F.rig_eps(3, 33, 8, 1) == float(np.float32(0.0078125 * 1.002 + 2.0 * (2.0 * 1.0 * 3 * 33 * 8 * 5.97e-8)))
    assert F.accum_eps(3, 33, 8, 3) == 2.0 * (2.0 * 3 * 3 * 33 * 8 * 5.97e-8)
    assert F.rig_eps(1, 24, 1, 3, doubled=False) == 3.0518e-5 + 2.0 * 3.0 * 24 * 1 * 5.97e-8
    for pc in (3, 1):
        assert F.accum_eps(2, 9, 3, pc) < F.rig_eps(2, 9, 3, pc)


@pytest.mark.parametrize("cell", G.CELLS, ids=G._NAMES)
def test_model_meets_the_bound_on_the_cells_scenes(cell):
    worst = {3: 0.0, 1: 0.0}
    for scene, methods in cell["scenes"]:
        img = G.scene_image(cell, scene)
        memo = {}
        for method in methods:
            tl = G.templates(cell, scene, method, img)
            kinds = [k for k, _ in tl]
            picks = G.map_picks(cell, kinds)
            assert set(G.single_picks(cell, kinds)) <= set(range(len(tl)))
            refs = G._refs(cell, scene, method, img, tl, picks, memo)
            for i in picks:
                exact, model, tol = refs[i]
                if model is None:                   # the off-cores cell: nothing to model
                    assert cell["kernel"] == 0
                    continue
                for pc in (3, 1):
                    m = model[pc]
                    if G.always_one(kinds[i], method):
                        assert np.array_equal(m, np.ones_like(m)) and np.array_equal(exact, np.ones_like(m))
                        continue
                    A, M, live = tol[pc]
                    unsat, enough = G.compared(kinds[i], m, exact, live)
                    assert enough, (cell["name"], scene, method, i, kinds[i], int(unsat.sum()), unsat.size)
                    d = np.abs(m - exact)
                    assert (d[unsat] <= M[unsat]).all(), (cell["name"], scene, method, i, kinds[i], pc, float((d[unsat] / M[unsat]).max()))
                    assert (A[unsat] <= M[unsat]).all() and (A[unsat] > 0.0).all()
                    worst[pc] = max(worst[pc], float((d[unsat] / M[unsat]).max()))
    print("%s: worst |model - exact| / bound_map: three products %.3f, one %.3f" % (cell["name"], worst[3], worst[1]))


def test_the_table_covers_every_edge_cpu():
    G.test_the_table_covers_every_edge()


def _fraction_compared(img, t, method):
    m = F.model_scores(img, t, method).astype(np.float64)
    ref = O.match_template(img, t, method, corr="direct").astype(np.float64)
    _, live = F.bound_map(img, t, method)
    return float((live & (np.abs(m) < 1.0) & (np.abs(ref) < 1.0)).mean())


def test_which_scenes_a_method_can_use():
    """TM_SQDIFF_NORMED = sum (I - T)^2 / sqrt(sum I^2 sum T^2) is ~2 between unrelated zero-mean windows - saturated - and
    on a step image wherever window and template lie on different sides; on N(100, 40) it is ~0.27.  Methods 5 and 3 leave
    only the exact copy's own position out on all four scenes."""
    cell = next(c for c in G.CELLS if c["name"] == "chunks-65x33")
    frac = {}
    for scene in ("noise+", "signed", "offset", "step"):
        img = G.scene_image(cell, scene)
        for kind, t in G.templates(cell, scene, 1, img)[:2]:
            for method in (5, 3, 1):
                frac[(scene, kind, method)] = _fraction_compared(img, t, method)
    n_out = cell["out"][0] * cell["out"][1]
    for (scene, kind, method), f in frac.items():
        if method in G.SCENE_METHODS[scene]:
            assert f >= (n_out - 1.0) / n_out, (scene, kind, method, f)
    assert frac[("noise+", "noisy", 1)] == 1.0
    assert frac[("signed", "noisy", 1)] < 0.01 and frac[("signed", "exact", 1)] < 0.01
    assert frac[("step", "noisy", 1)] < 0.99 and frac[("step", "exact", 1)] < 0.99


@pytest.mark.parametrize("shape", [(5, 31), (65, 33), (33, 97)])
def test_impulse_templates_pick_the_shifted_normalised_image(shape):
    """One non-zero tap at (dy, dx), TM_CCORR_NORMED: the map is I(y + dy, x + dx) / sqrt(window sum of I^2), whatever the
    tap's value - a tap the model (or the kernel) dropped or misplaced shows at every output."""
    h, w = shape
    cell = next(c for c in G.CELLS if (c["h"], c["w"], c["chans"], c["n"]) == (h, w, 1, 0))
    for scene in ("noise+", "step"):
        img = G.scene_image(cell, scene)
        oh, ow = cell["out"]
        S2 = O.window_sums(img.astype(np.float64) ** 2, h, w)
        for dy, dx in G.impulse_taps(h, w):
            t = np.zeros((h, w), np.float32)
            t[dy, dx] = 64.0
            want = img[dy:dy + oh, dx:dx + ow].astype(np.float64) / np.sqrt(S2)
            for pc in (3, 1):
                got = F.model_scores(img, t, 3, pc).astype(np.float64)
                M, live = F.bound_map(img, t, 3, pc)
                ok = live & (np.abs(want) < 1.0) & (np.abs(got) < 1.0)
                assert ok.mean() >= 0.99
                assert (np.abs(got - want)[ok] <= M[ok]).all(), (shape, scene, dy, dx, pc)
            # the tap's place matters: the neighbouring tap's map is another one
            if dx + 1 < w and scene == "noise+":
                t2 = np.zeros((h, w), np.float32)
                t2[dy, dx + 1] = 64.0
                other = F.model_scores(img, t2, 3, 3).astype(np.float64)
                A, _, _ = F.tolerances(img, t, 3, 3)
                assert (np.abs(other - want)[ok] > A[ok]).mean() > 0.9


# ---- the scenes of tests/test_gpu_f32_range.py: every cell exercises what it is there for, shown on the reference alone ----
import test_gpu_f32_range as R     # noqa: E402


def _range_id(case):
    return "%s-%s-%s" % (case[0]["name"], case[1], case[2])


@pytest.mark.parametrize("case", [c for c in R.CASES if c[2] in F.IN_RANGE], ids=_range_id)
def test_range_model_meets_the_bound_on_in_range_scenes(case):
    cell, kind, scene = case
    worst = 0.0
    for method in R.methods_of(kind):
        for i, (exact, model, tol, valid) in R.refs_of(cell, kind, scene, method).items():
            assert valid.all()
            for pc in (3, 1):
                m = model[pc]
                if R.always_one(scene, method):
                    # cv2's absolute DBL_EPSILON rule: the template is constant, the score 1 everywhere - and nothing else
                    # is claimed for this pair
                    assert np.array_equal(m, np.ones_like(m)) and np.array_equal(exact, np.ones_like(m))
                    continue
                assert not (m == 1.0).all()
                A, M, live = tol[pc]
                unsat, enough = R.compared(i % 3 != 1, m, exact, live, valid)
                assert enough, (cell["name"], kind, scene, method, i, int(unsat.sum()), unsat.size)
                d = np.abs(m - exact)
                assert (d[unsat] <= M[unsat]).all(), (cell["name"], kind, scene, method, i, pc, float((d[unsat] / M[unsat]).max()))
                assert (A[unsat] <= M[unsat]).all() and (A[unsat] > 0.0).all()
                worst = max(worst, float((d[unsat] / M[unsat]).max()))
    print("%s: worst |model - exact| / bound_map %.3f" % (_range_id(case), worst))


def test_range_scaled_scenes_are_the_base_scene_exactly():
    cell = F.RANGE_CELLS[0]
    a, b = F.range_scene(cell, "up40"), F.range_scene(cell, "tiny")
    assert np.array_equal(a["img"] * np.float32(2.0 ** -100), b["img"]) and a["cuts"] == b["cuts"]
    for ta, tb in zip(a["templs"], b["templs"]):
        assert np.array_equal(ta * np.float32(2.0 ** -100), tb)
    assert np.array_equal(a["img"][a["cuts"][0][0]:, a["cuts"][0][1]:][:cell["h"], :cell["w"]], a["templs"][0])
    assert not np.array_equal(a["img"][a["cuts"][1][0]:, a["cuts"][1][1]:][:cell["h"], :cell["w"]], a["templs"][1])   # (noisy)


@pytest.mark.parametrize("cell", F.RANGE_CELLS, ids=lambda c: c["name"])
def test_range_huge_and_tiny_provoke_what_they_are_there_for(cell):
    h, w = cell["h"], cell["w"]
    for scene in ("huge", "tiny"):
        S = F.range_scene(cell, scene)
        for method in (5, 3, 1):
            for i, (exact, model, tol, valid) in R.refs_of(cell, "noise+", scene, method).items():
                assert valid.all() == (scene == "tiny")         # huge: a float32 accumulator may overflow anywhere
                for pc in (3, 1):
                    m = model[pc]
                    if R.always_one(scene, method):
                        assert scene == "tiny" and np.array_equal(m, np.ones_like(m)) and np.array_equal(exact, np.ones_like(m))
                        continue
                    # the float64 restatement still meets the bound
                    A, M, live = tol[pc]
                    unsat, enough = R.compared(i % 3 != 1, m, exact, live, np.ones_like(valid))
                    assert enough and (np.abs(m - exact)[unsat] <= M[unsat]).all(), (cell["name"], scene, method, i, pc)
    # huge: the float32 sum of the exact copy's centred leading-piece products is not finite
    S = F.range_scene(cell, "huge")
    y, x = S["cuts"][0]
    img3, t3 = F._as3d(S["img"]), F._as3d(S["templs"][0])
    _, planes = F.templ_centred(t3)
    total = np.float32(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(cell["chans"]):
            mu = F.tile_mu(img3[:, :, c], y - y % F.ROWS, x - x % F.SEG, h, F.SEG + 32 * F.nkb_of(w))
            a0 = F.bf16_rne(img3[y:y + h, x:x + w, c] - mu)
            total = total + (a0 * F.bf16_rne(planes[c])).sum(dtype=np.float32)
    assert not np.isfinite(total)
    assert F.window_scores(S["img"], S["templs"][0], 3, [(y, x)])[0] == 1.0     # ... while the float64 sums give 1


@pytest.mark.parametrize("cell", F.RANGE_CELLS, ids=lambda c: c["name"])
def test_range_nonfinite_scene_is_live(cell):
    h, w = cell["h"], cell["w"]
    S = F.range_scene(cell, "nonfinite")
    img = S["img"]
    assert set(S["copies"]) | set(S["skipped"]) >= {"a", "b", "c"} and set(S["bad"]) | set(S["skipped"]) == {"a", "b", "c", "d"}
    assert "a" in S["copies"]                       # every cell has room for (a)
    assert ("b" in S["copies"]) == (cell["name"] in ("12x20", "5x33", "24x40-n17", "7x40-c3"))
    assert "d" in S["bad"]
    reach, dirty, inside = F.kernel_reach(img, h, w), F.engine_stats_dirty(img, h, w), F.window_dirty(img, h, w)
    samples = F.tile_samples(img.shape[0], img.shape[1], cell["out"][0], cell["out"][1], h, w)
    for label, (y, x) in S["copies"].items():
        assert np.array_equal(F._as3d(img)[y:y + h, x:x + w], F._as3d(S["templs"][0])), label       # an exact copy, intact
        assert not inside[y, x] and not dirty[y, x], label
        assert reach[y, x] == (label in ("a", "b")), label
        for method, want in ((5, 1.0), (3, 1.0)):
            assert F.window_scores(img, S["templs"][0], method, [(y, x)])[0] == want, (label, method)
        # TM_SQDIFF_NORMED: cv2 takes sum T^2 from meanStdDev, (variance + mean^2) * area - a few float64 ulp from the direct
        # sum, so the exact copy scores 0 up to ~1e-16
        assert 0.0 <= F.window_scores(img, S["templs"][0], 1, [(y, x)])[0] <= 1e-12, label
    r, c, ch, bits = S["bad"]["a"]
    assert (r, c) == (0, 0) and (0, 0) in samples and S["copies"]["a"] == (1, 40)
    for label in ("b", "c", "d"):
        if label in S["bad"]:
            assert S["bad"][label][:2] not in samples, label
    if "b" in S["copies"]:
        (y, x), (r, c, ch, bits) = S["copies"]["b"], S["bad"]["b"]
        assert y <= r <= y + h - 1 and 1 <= c - (x + w - 1) <= 32 * F.nkb_of(w) - w and y >= F.ROWS
        assert np.isposinf(F._as3d(img)[r, c, ch])
    if "c" in S["copies"]:
        (y, x), (r, c, ch, bits) = S["copies"]["c"], S["bad"]["c"]
        assert r == y + h and x <= c < x + w and np.isneginf(F._as3d(img)[r, c, ch])
        # the windows under the copy meet the pixel with positive taps: -inf there, never the +inf that TM_SQDIFF_NORMED's
        # fmax(.., 0) turns into a score of 0 beside the copy
        assert (F._as3d(S["templs"][0])[h - 1, c - x - 1:c - x + 2, ch] > 0).all()
    # (d): a NaN whose payload carries - in no copy's window, and the model is compared somewhere
    r, c, ch, bits = S["bad"]["d"]
    assert F._as3d(img).view(np.uint32)[r, c, ch] == F.NAN_PAYLOAD
    assert not any(y <= r < y + h and x <= c < x + w for y, x in S["copies"].values())
    assert (~(reach | dirty | inside)).mean() >= 0.1
    assert np.isfinite(S["clean"]).all()


def test_bf16_rne_on_nan():
    """bf16_rne is stated for finite floats and infinities.  A NaN keeps being one while its payload does not carry into the
    exponent; 0x7FFFFFFF + 0x8000 wraps to -0.0.  Harmless: the windows that hold the pixel have NaN statistics."""
    v = np.array([np.nan, np.inf, -np.inf], np.float32)
    out = F.bf16_rne(v)
    assert np.isnan(out[0]) and out[1] == np.inf and out[2] == -np.inf
    p = np.array([F.NAN_PAYLOAD], np.uint32).view(np.float32)
    assert np.isnan(p[0]) and F.bf16_rne(p).view(np.uint32)[0] == 0x80000000
