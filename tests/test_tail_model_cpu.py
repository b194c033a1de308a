"""The tail screen's model (tests/tail_model.py) held to itself, without a GPU: the float64 restatement of tail_consts_kernel
obeys against exact integers and Fractions what tests/test_gpu_tail_consts.py asks of the device's constants; the bound built
from them is never below the exact numerator - on the sweep's scenes and on adversarial windows, both methods, both row
parities, splits 6, 7, the rule's values and h - 2; one mistake at a time in the constants IS seen by one of those two checks;
and the scenes of tools/tail_wave_count.py are ones on which some waves leave and some stay."""
import numpy as np
import pytest

import tail_model as M


@pytest.fixture(scope="module")
def lib():
    import build as mtm_build
    mtm_build.build()
    from MTM import _lib
    return _lib


_IDS = [c["name"] for c in M.CONST_CELLS]


@pytest.mark.parametrize("cell", M.CONST_CELLS, ids=_IDS)
def test_restated_constants_obey_the_inequalities(lib, cell):
    _, templates, kinds = M.scene(cell)
    assert set(kinds) >= set(M.KINDS)
    splits = M.cell_splits(lib, cell)
    assert splits[0] == 6 and splits[-1] == cell["h"] - 2
    for split in splits:
        bad = M.consts_violations(M.table_f64(templates, split), templates, split)
        assert not bad, (cell["name"], split, bad[:3])


def test_exact_constants_against_a_pixel_loop():
    rng = np.random.default_rng(3)
    for kind, (h, w), q0s in (("noise", (8, 64), (5, 6)), ("noise", (9, 49), (6, 7)), ("flat_top", (24, 49), (16, 17, 22)),
                              ("last_pixel", (11, 50), (9,)), ("checker", (10, 63), (6, 8)), ("const77", (8, 56), (6,))):
        T = M.make_template(kind, h, w, rng)
        for q0 in q0s:
            assert M.consts_exact(T, q0) == M.consts_brute(T, q0), (kind, h, w, q0)


# ---- rigour ----------------------------------------------------------------------------------------------------------------
def _adversarial(h, w, rng):
    """(name, window I, template T): pairs built to strain one term of the bound each."""
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.clip(128 + 100 * np.sin(yy / 7.0) * np.cos(xx / 5.0), 0, 255).astype(np.uint8)
    noise = rng.integers(0, 256, (h, w)).astype(np.uint8)
    binary = (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
    one = np.zeros((h, w), np.uint8)
    one[h - 1, w // 3] = 200
    full = lambda v: np.full((h, w), v, np.uint8)                                                       # noqa: E731
    return [("copy_noise", noise, noise), ("copy_smooth", smooth, smooth), ("anti", smooth, 255 - smooth),
            ("anti_noise", noise, 255 - noise), ("flat_vs_noise", full(255), noise), ("noise_vs_flat", noise, full(77)),
            ("near_flat_vs_binary", rng.integers(254, 256, (h, w)).astype(np.uint8), binary), ("binary_copy", binary, binary),
            ("sat_sat", full(255), full(255)), ("zero_zero", full(0), full(0)), ("sat_zero", full(255), full(0)),
            ("tail_pixel_copy", one, one), ("tail_pixel_vs_noise", noise, one), ("tail_pixel_vs_sat", full(255), one)]


def _pair_images(I, rng):
    """The window at an even and at an odd output row: one more image row below / above it."""
    extra = rng.integers(0, 256, (1, I.shape[1])).astype(np.uint8)
    return {"even": np.vstack([I, extra]), "odd": np.vstack([extra, I])}


def _rigour(lib, img, templates, method, thr, split, table, nums=None, tstats=None):
    h, w = templates[0].shape
    st = M.model_stats(img, h, w, method, split)
    tstats = M.templ_stats(lib, templates, method) if tstats is None else tstats
    return M.rigour(img, templates, method, thr, table, tstats, st, split, nums=nums)


@pytest.mark.parametrize("method", [5, 3])
@pytest.mark.parametrize("cell", M.CONST_CELLS, ids=_IDS)
def test_bound_is_never_below_the_numerator_on_the_scenes(lib, cell, method):
    cell = dict(cell, method=method)
    img, templates, _ = M.scene(cell)
    h, w = cell["h"], cell["w"]
    tstats = M.templ_stats(lib, templates, method)
    nums = M.numerators(img, templates, method, M.model_stats(img, h, w, method, 6))
    checked = 0
    for split in M.cell_splits(lib, cell):
        r = _rigour(lib, img, templates, method, 0.5, split, M.table_f64(templates, split), nums=nums, tstats=tstats)
        assert not r["violations"], (cell["name"], method, split, r["violations"][:3])
        assert 0.0 <= r["tightness"] < 1.0, (cell["name"], method, split, r["tightness"])
        checked += r["checked"]
        print("tail_model %-22s method %d split %2d  min (bound - num) / (templ_norm sq) = %.3e" % (
            cell["name"], method, split, r["tightness"]))
    assert checked >= 13 * 19 * cell["n"]              # every row (both parities), every block, every template


@pytest.mark.parametrize("method", [5, 3])
@pytest.mark.parametrize("h,w", [(8, 64), (24, 49), (71, 64)])
def test_bound_is_never_below_the_numerator_on_adversarial_pairs(lib, h, w, method):
    rng = np.random.default_rng(100 * h + w + method)
    splits = sorted({6, min(7, h - 2), h - 2} | {s for s in (M.rule_split(lib, h, w, t) for t in M.RULE_THRESHOLDS) if s})
    n_checked = 0
    for name, I, T in _adversarial(h, w, rng):
        for parity, img in _pair_images(I, rng).items():
            for split in splits:
                r = _rigour(lib, img, [T], method, 0.5, split, M.table_f64([T], split))
                assert not r["violations"], (name, parity, h, w, method, split, r["violations"])
                n_checked += r["checked"]
    assert n_checked == 14 * 2 * len(splits) * 2


# ---- the checks can see mistakes -------------------------------------------------------------------------------------------
def _seen_by(lib, mistake):
    """Where one wrong derivation of the constants shows: {(cell, split): "consts" / "rigour" / both}, over small cells of the
    table and the adversarial pairs."""
    seen = {}
    for cell in (M.CONST_CELLS[1], M.CONST_CELLS[3]):
        for method in (5, 3):
            c = dict(cell, method=method)
            img, templates, _ = M.scene(c)
            for split in M.cell_splits(lib, c):
                if mistake == "stale" and split + 7 > c["h"] - 2:
                    continue
                table = M.table_f64(templates, split, mistake)
                how = []
                if M.consts_violations(table, templates, split):
                    how.append("consts")
                if _rigour(lib, img, templates, method, 0.5, split, table)["violations"]:
                    how.append("rigour")
                if how:
                    seen[(c["name"], method, split)] = "+".join(how)
    rng = np.random.default_rng(7)
    h, w = 24, 49
    for name, I, T in _adversarial(h, w, rng):
        for parity, img in _pair_images(I, rng).items():
            for split in (6, 12, h - 2):
                if mistake == "stale" and split + 7 > h - 2:
                    continue
                if mistake == "neighbour":
                    continue                                   # (one template: it has no neighbour)
                table = M.table_f64([T], split, mistake)
                if _rigour(lib, img, [T], 5, 0.5, split, table)["violations"]:
                    seen[(name + "-" + parity, 5, split)] = "rigour"
    return seen


@pytest.mark.parametrize("mistake", M.MISTAKES)
def test_one_mistake_in_the_constants_is_seen(lib, mistake):
    seen = _seen_by(lib, mistake)
    by_rigour = sorted(k for k, v in seen.items() if "rigour" in v)
    by_consts = sorted(k for k, v in seen.items() if "consts" in v)
    print("tail_model mistake %-10s seen on %d cells: constants comparison %d, rigour %d (first: %s)" % (
        mistake, len(seen), len(by_consts), len(by_rigour), by_rigour[:2]))
    assert seen, mistake
    # the decisions it would have cost: leaving waves of a counter scene with the wrong constants against the right ones
    cell = M.COUNTER_SCENES[2]
    _, templates, _ = M.scene(cell)
    for thr in M.COUNTER_THRESHOLDS:
        split = M.rule_split(lib, cell["h"], cell["w"], thr)
        if mistake == "stale" and split + 7 > cell["h"] - 2:
            continue
        right = M.predict(lib, cell, thr)
        wrong = M.predict(lib, cell, thr, consts=M.table_f64(templates, split, mistake))
        print("tail_model mistake %-10s %s thr %.1f: leaving %d -> %d of %d, %d waves decide otherwise" % (
            mistake, cell["name"], thr, right["leaving"], wrong["leaving"], right["waves"], int((right["stay"] != wrong["stay"]).sum())))


def test_the_unmistaken_constants_pass_both_checks(lib):
    """The control of the test above: the same cells with the right constants trip nothing."""
    assert _seen_by(lib, None) == {}


# ---- the counter scenes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", M.COUNTER_SCENES, ids=[c["name"] for c in M.COUNTER_SCENES])
def test_counter_scenes_have_waves_that_leave_and_waves_that_stay(lib, cell):
    for thr in M.COUNTER_THRESHOLDS:
        p = M.predict(lib, cell, thr)
        g = M.geometry(cell["map"][0], cell["map"][1], cell["n"])
        assert p["waves"] == g["waves"] and p["stay"].shape == (g["nyb"], g["nseg"], g["ntg"], M.WAVES)
        print("tail_model counter scene %-20s thr %.1f split %2d: %d of %d waves leave; per group %s" % (
            cell["name"], thr, p["split"], p["leaving"], p["waves"],
            [int((~p["stay"][:, :, tg]).sum()) for tg in range(g["ntg"])]))
        if cell["method"] == 3 and not cell.get("force_split"):
            continue                # (sparse noise under TM_CCORR_NORMED at the rule's split: the model's figure is printed)
        assert p["split"] >= 6
        assert 0 < p["leaving"] < p["waves"], (cell["name"], thr, p["leaving"])
        if cell["method"] == 5:
            # the flat-topped template (list position 1) keeps its whole group in; the other group leaves but around the
            # plant of the last template: row min(4, oh - 1), column (ow - 1) / 2
            assert p["stay"][:, :, 0].all(), (cell["name"], thr)
            y, x = min(4, cell["map"][0] - 1), (cell["map"][1] - 1) // 2
            assert p["stay"][y // M.ITEM_ROWS, x // M.ITEM_COLS, 1, (y % M.ITEM_ROWS) // M.WAVE_ROWS]
            assert p["stay"][:, :, 1].sum() <= 3, (cell["name"], thr, int(p["stay"][:, :, 1].sum()))
