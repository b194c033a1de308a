"""
The conditions tests/test_gpu_window_sweep.py relies on, shown without a GPU and from the reference alone:

  * the constants tests/window_cases.py mirrors are the kernels' (parsed out of the headers);
  * the table covers the edges it is there for - every w % 4 against every lx & 3, every lane of a tile as a family-B
    winner per instantiation, every variant index of every group size nv of the fused set sums, every w % 4 against every
    d = 0 .. 2 of the neighbourhood kernel - so that a table edit cannot silently drop one;
  * every scene is exact data: no partial sum of a window reaches 2^53;
  * mtm_oracle's corr="direct" sums are what a triple loop over Python integers gives;
  * the scenes are honest: most of every normalised map of an exact, noisy or saturated template is finite and not 0 or
    +-1, every planted winner is its map's strict extremum (the tie cells tie exactly as intended), no float cell carries
    a flat window, and the border rows and columns of the templates and masks whose taps must count are non-zero.
"""
import os
import re

import numpy as np
import pytest

import mtm_oracle as O
import window_cases as C

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "multitemplatematching-python_amd", "csrc")
BIG = C.P_FLUSH_U16["h"]


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_mirrored_constants_are_the_kernels():
    win, nbhd = _src("mtm_k_window.hip.h"), _src("mtm_k_nbhd.hip.h")
    const = lambda text, name: int(re.search(r"\b%s\s*=\s*(\d+)" % name, text).group(1))                       # noqa: E731
    assert (const(win, "kWinTile"), const(win, "kWinKR"), const(win, "kWinKC")) == (C.WIN_TILE, C.WIN_KR, C.WIN_KC)
    assert re.search(r"kWinIW\s*=\s*kWinTile \+ kWinKC \+ 4;", win) and C.WIN_IW == C.WIN_TILE + C.WIN_KC + 4
    assert re.search(r"kSubR\s*=\s*kWinKR,\s*kSubC\s*=\s*kWinKC;", nbhd) and (C.SUB_R, C.SUB_C) == (C.WIN_KR, C.WIN_KC)
    assert const(_src("mtm_internal.h"), "kTrackNV") == C.TRACK_NV
    assert re.search(r"_U16_MAX_PIXELS = 1 << 21", open(os.path.join(CSRC, "..", "MTM", "blocks.py")).read())
    assert C.U16_MAX_PIXELS == 1 << 21 and "t.rows * t.cols > (1ll << 21)" in _src("mtm_host.cpp")
    assert BIG * BIG <= C.U16_MAX_PIXELS < (BIG + 1) * (BIG + 1)


def _chunk(w):
    return (w - 1) // C.WIN_KC


def test_the_table_covers_every_edge():
    # ---- P: per instantiation, every w % 4 of a first, second and third chunk against every lx & 3, at margin 16 at least
    for dt in C.INT_DTYPES:
        cells = [c for c in C.family("P") if c["dtype"] == dt]
        ws = {c["w"] for c in cells if c["group"] == "w"}
        assert ws == set(C.P_WIDTHS)
        for k in (0, 1):                                        # the column tail of 1 .. 3 bytes (or none) of the last chunk
            assert {w % 4 for w in ws if _chunk(w) == k} == {0, 1, 2, 3}, (dt, k)
        assert {w - 2 * C.WIN_KC for w in ws if _chunk(w) == 2} == {1}          # ... and a third chunk of one column
        pairs = {(c["w"] % 4, lx & 3) for c in cells for lx in range(min(2 * c["margin"] + 1, C.WIN_TILE))}
        assert len(pairs) == 16
        # lanes 13 .. 15 and a second tile's first lane against a full 64-column chunk
        assert any(c["w"] >= C.WIN_KC and c["margin"] >= 7 for c in cells)             # a map of 15 or more: lanes 13 .. 15
        assert any(c["w"] >= C.WIN_KC and 2 * c["margin"] + 1 > C.WIN_TILE for c in cells)
        for g, w in (("h", 5), ("h", 65)):
            assert {c["h"] for c in cells if c["group"] == g and c["w"] == w} == set(C.P_HEIGHTS)
        assert {(17, 65), (33, 129)} <= {(c["h"], c["w"]) for c in cells if c["group"] == "hw"}
        assert {c["margin"] for c in cells if c["group"] == "m"} == set(C.P_MARGINS)
        assert {2 * m + 1 for m in C.P_MARGINS} == {1, 3, 15, 17, 33, 49}
        place = [c for c in cells if c["group"] == "place"]
        assert {c["frame"][1] % 4 for c in place} == {0, 1, 2, 3} and all(len(c["places"]) == 9 for c in place)
        assert all(c["methods"] == C.ALL for c in cells)
    assert all(c["margin"] == 16 for c in C.family("P") if c["group"] == "w" and c["dtype"] == "u8")     # every width meets 16
    flush = [c for c in C.family("P") if c["group"] == "flush"]
    assert {(c["dtype"], c["h"], c["w"]) for c in flush} == {("rgb", 300, 280), ("u16", BIG, BIG)}
    assert 300 * 280 * 255 * 255 > 2 ** 32
    # ---- B: the geometry of P on maps of 17 x 33; every lane per instantiation (below, from the maps)
    assert {w for h, w in C.B_GEOMS if h == 3} == set(C.P_WIDTHS) and C.B_MAP == (17, 33)
    assert {h for h, w in C.B_GEOMS if w == 5} >= set(C.P_HEIGHTS) <= {h for h, w in C.B_GEOMS if w == 65}
    assert {(17, 65), (33, 129)} <= set(C.B_GEOMS)
    assert {(c["dtype"], c["mode"], c.get("border")) for c in C.family("B")} == {
        (dt, mode, b) for dt in C.INT_DTYPES for mode, b in (("global", None), ("local", "constant"), ("local", "nearest"))}
    # ---- T: every (group size nv, index in the group) in a full group, a last group and a single group
    slots = {C.set_slots(n, v) for n, v in C.T_COMBOS}
    assert {(nv, i) for nv, i, role in slots if role == "single"} == {(nv, i) for nv in (1, 2, 3, 4) for i in range(nv)}
    assert {(nv, i) for nv, i, role in slots if role == "last"} == {(nv, i) for nv in (1, 4) for i in range(nv)}
    assert {(nv, i) for nv, i, role in slots if role == "full"} == {(4, i) for i in range(4)}
    assert {w for _, w in C.T_SHAPES} == set(C.T_WIDTHS) and {h for h, _ in C.T_SHAPES} == set(C.T_HEIGHTS)
    assert C.TRACK_NV == 4 and set(C.T_SETS) == {1, 2, 3, 4, 5, 8, 9}
    for pair in C.T_TIES:
        assert sorted(pair) == list(pair)                       # (the first in row-major order comes first)
    (a, b), (c, d) = C.T_TIES
    assert a[1] // C.WIN_TILE != b[1] // C.WIN_TILE             # two tiles
    assert (c[0], d[0]) == (3, 4) and c[1] < C.WIN_TILE and d[1] < c[1]     # waves 0 and 1 of one tile, the later lane first
    for dt in C.INT_DTYPES:
        cells = [x for x in C.family("T") if x["dtype"] == dt]
        # a call without a set runs track_score_kernel / track_reacquire_kernel, a call with one the fused set kernels
        assert {(x["mode"], x.get("plain", False)) for x in cells} == {("sets", False), ("ties", False), ("reacquire", False),
                                                                       ("sets", True), ("reacquire", True)}
        assert {x["frame"] for x in cells if x["mode"] == "reacquire" and not x.get("plain")} == set(C.T_REACQ_FRAMES)
    # ---- N: per kind, every w % 4 in a first and in a second chunk (d = 0 .. 2: every interior point has all nine windows)
    for kind in C.N_KINDS:
        cells = [c for c in C.family("N") if c["kind"] == kind]
        for k in (0, 1):
            assert {c["w"] % 4 for c in cells if _chunk(c["w"]) == k} == {0, 1, 2, 3}, (kind, k)
        assert {c["w"] for c in cells} == set(C.N_WIDTHS)
        assert {c["h"] for c in cells} == set(C.N_HEIGHTS) | {3}
        assert all(c["methods"] == ((0, 3) if c["masked"] else C.ALL) for c in cells)
    assert C.N_MAP[0] >= 3 and C.N_MAP[1] >= 3
    # ---- Y
    assert {(c["h"], c["w"]) for c in C.family("Y")} == {(17, 65), (5, 129)}
    assert all(2 * c["radius"] + 1 > C.WIN_TILE for c in C.family("Y"))


# ---- exact data ------------------------------------------------------------------------------------------------------------
def _exact(image, templ, mask=None):
    """The largest partial sum any chain over a window can form stays below 2^53: taps x max I x max (T, I), and the
    integral image of I^2 over the whole image the oracle is given."""
    vi, vt = float(image.max()), float(templ.max())
    taps = templ.size
    assert float(np.abs(image).min()) >= 0 and np.array_equal(image, np.rint(image)) and np.array_equal(templ, np.rint(templ))
    assert taps * max(vi, vt) ** 2 < 2.0 ** 53
    assert float((image.astype(np.float64) ** 2).sum()) < 2.0 ** 53
    if mask is not None:
        assert set(np.unique(mask).tolist()) <= {0, 1, 255}


@pytest.mark.parametrize("fam", "PBTNY")
def test_every_scene_is_exact_data(fam):
    for cell in C.family(fam):
        if fam == "P":
            img, calls, blocks, temps, kinds = C.p_scene(cell)
            for b, t in zip(blocks, temps):
                x0, y0, bw, bh = C.search_box(b, cell["margin"], img.shape)
                box = img[y0:y0 + bh, x0:x0 + bw]
                if cell["h"] == BIG:
                    # the one scene whose integral image passes 2^53 (by 0.3 %): the windows' own sums, which are what the
                    # kernels form, stay below it - 1448^2 pixels of 65535^2 - and the oracle's maps are those of the exact sums
                    # all the same (test_the_limit_block_in_integers)
                    assert t.size * 65535.0 ** 2 < 2.0 ** 53 < float((box.astype(np.float64) ** 2).sum())
                    continue
                _exact(box, t)
            for ref, group in calls:
                for k in group:
                    x, y, w, h = blocks[k]
                    assert np.array_equal(ref[y:y + h, x:x + w], temps[k])
        elif fam == "B":
            img, temps, regions, _ = C.b_scene(cell)
            for (x, y, bw, bh), (j,) in regions:
                _exact(img[y:y + bh, x:x + bw], temps[j][1])
        elif fam == "T":
            frames, temps, tracks, _, _, reacquire = C.t_scene(cell)
            for (x, y, bw, bh), js in tracks:
                for j in C.track_set(js):
                    _exact(frames[0] if reacquire else frames[0][y:y + bh, x:x + bw], temps[j][1])
        elif fam == "Y":
            img, temps, _ = C.y_scene(cell)
            for _, t in temps:
                _exact(img, t)
        else:
            img, temps, kinds = C.n_scene(cell)
            assert img.dtype == C.NPDT[cell["dtype"]] and float(img.max()) <= C.TOP[cell["dtype"]]
            for e in temps:
                _exact(img, e[1], e[2] if len(e) > 2 else None)


def test_the_limit_block_in_integers():
    """The 1448 x 1448 uint16 block: every window sum in int64 (exact, below 2^63) against the oracle's float64 integral-image
    lookup and its direct correlation.  The integral image of I^2 over the 1450 x 1450 box passes 2^53 by 0.3 %, so the
    oracle's lookup is a unit or two off at two outputs; its float32 maps are those of the exact sums nevertheless."""
    cell = next(c for c in C.family("P") if c["h"] == BIG)
    img, calls, blocks, temps, kinds = C.p_scene(cell)
    assert kinds == ["flush"] and img.shape == (BIG + 2, BIG + 2) and len(blocks) == 1
    a, t = img.astype(np.int64), temps[0].astype(np.int64)
    assert int((t != 65535).sum()) == 4 and int((a != 65535).sum()) == 0
    h = w = BIG
    exact = {}
    for power in (1, 2):
        ii = np.zeros((BIG + 3, BIG + 3), np.int64)
        ii[1:, 1:] = np.cumsum(np.cumsum(a ** power, axis=1), axis=0)
        exact[power] = ii[:3, :3] - ii[:3, w:] - ii[h:, :3] + ii[h:, w:]
        assert int(exact[power].max()) < 2 ** 53
        # the oracle's float64 integral of I^2 rounds once past 2^53 (entry 1449 x 1449 is odd): two outputs are 1 and 2 units
        # of 9.0e15 off
        off = np.abs(O.window_sums(img.astype(np.float64) ** power, h, w) - exact[power].astype(np.float64))
        assert float(off.max()) <= (0.0 if power == 1 else 2.0)
    corr = np.array([[int((a[y:y + h, x:x + w] * t).sum()) for x in range(3)] for y in range(3)])
    assert int(corr.max()) < 2 ** 53
    planes, maps = _p_data(cell)
    assert np.array_equal(maps[0][2], corr.astype(np.float64).astype(np.float32))            # TM_CCORR: the sums themselves
    # ... and its six maps are, bit for bit, what its own formulas give from the exact integer sums: the standard stands
    real = O.window_sums, O.sliding_corr
    O.window_sums = lambda x, hh, ww: exact[1 if float(x.max()) <= 65535.0 else 2].astype(np.float64)
    O.sliding_corr = lambda *args, **kw: corr.astype(np.float64)
    try:
        for m in C.ALL:
            again = O.match_template(img.astype(np.float32), temps[0].astype(np.float32), m, corr="direct")
            assert C.same_bits(again, maps[0][m]).all(), m
    finally:
        O.window_sums, O.sliding_corr = real


def _triple_loop(img2d, ker2d):
    a = [[int(v) for v in row] for row in np.asarray(img2d)]
    k = [[int(v) for v in row] for row in np.asarray(ker2d)]
    H, W, h, w = len(a), len(a[0]), len(k), len(k[0])
    out = np.empty((H - h + 1, W - w + 1), np.float64)
    for y in range(H - h + 1):
        for x in range(W - w + 1):
            s = 0
            for dy in range(h):
                ar, kr = a[y + dy], k[dy]
                for dx in range(w):
                    s += ar[x + dx] * kr[dx]
            assert s < 2 ** 53
            out[y, x] = float(s)
    return out


_SMALL = {"P-u8": "P-w-u8-3x5-m16", "P-u16": "P-m-u16-3x5-m7", "N-rgbmask": "N-rgbmask-3x4", "N-f32mask": "N-f32mask-3x5"}


@pytest.mark.parametrize("which", sorted(_SMALL))
def test_direct_sums_are_a_plain_triple_loop(which):
    """O.sliding_corr(..., force="direct") - the sums every epilogue of O.match_template(..., corr="direct") starts from -
    against Python-integer loops, operand by operand as the oracle forms them (masked: I x T M^2 and I^2 x M^2)."""
    cell = next(c for c in C.CELLS if c["name"] == _SMALL[which])
    if cell["family"] == "P":
        img, calls, blocks, temps, kinds = C.p_scene(cell)
        x0, y0, bw, bh = C.search_box(blocks[0], cell["margin"], img.shape)
        image, templ, mask = img[y0:y0 + bh, x0:x0 + bw], temps[0], None
    else:
        image, temps, kinds = C.n_scene(cell)
        templ, mask = temps[0][1], temps[0][2]
    integer = image.dtype == np.uint8
    a3, b3 = O._as3d(image).astype(np.float64), O._as3d(templ).astype(np.float64)
    for c in range(a3.shape[2]):
        if mask is None:
            pairs = [(a3[:, :, c], b3[:, :, c])]
        else:
            m = (O._as3d(mask)[:, :, c] > 0).astype(np.float64)
            pairs = [(a3[:, :, c], b3[:, :, c] * m * m), (a3[:, :, c] ** 2, m * m)]
        for x, k in pairs:
            got = O.sliding_corr(x, k, exact_int=integer, force="direct")
            assert got.dtype == np.float64 and np.array_equal(got, _triple_loop(x, k)), (cell["name"], c)


# ---- honest scenes ---------------------------------------------------------------------------------------------------------
_LIVE = ("exact", "noisy", "sat")


def _live_map(name, r, what):
    ok = np.isfinite(r) & ~np.isin(r, (0.0, 1.0, -1.0))
    assert ok.any() if r.size < 16 else 2 * int(ok.sum()) >= ok.size, (name, what, int(ok.sum()), ok.size)


def _border_counts(name, a):
    a3 = O._as3d(a)
    for c in range(a3.shape[2]):
        ch = a3[:, :, c]
        assert ch[0].all() and ch[-1].all() and ch[:, 0].all() and ch[:, -1].all(), name


def _p_data(cell):
    key = ("Pcpu", cell["name"])
    if key not in C._DATA:
        img, calls, blocks, temps, kinds = C.p_scene(cell)
        C._DATA[key] = C.p_expected(cell, img, blocks, temps)
    return C._DATA[key]


def test_the_plane_scenes_are_honest():
    flat = nan_cells = 0
    for cell in C.family("P"):
        img, calls, blocks, temps, kinds = C.p_scene(cell)
        planes, maps = _p_data(cell)
        for k, kind in enumerate(kinds):
            if kind in ("exact", "noisy", "noise", "isat", "iconst"):
                _border_counts(cell["name"], temps[k])
            for m in (1, 3, 5):
                if kind in _LIVE and cell["h"] * cell["w"] > 1:
                    _live_map(cell["name"], maps[k][m], (k, kind, m))
            if kind in ("isat", "iconst") and cell["margin"] >= 1:
                flat += bool((maps[k][5] == 0).any())           # a flat window under TM_CCOEFF_NORMED: 0
            if kind == "const":
                assert np.array_equal(maps[k][5], np.ones_like(maps[k][5])), cell["name"]
        nan_cells += bool(np.isnan(planes[5]).any())
        side = 2 * cell["margin"] + 1
        assert planes[5].shape == (len(blocks), side, side)
    assert flat >= 20 and nan_cells >= 12           # flat windows, and clipped boxes (NaN outside them), are well represented
    # the flush cells: their totals pass one uint32 and the correlation differs from output to output only where it should
    for cell in C.family("P"):
        if cell["group"] == "flush":
            _, maps = _p_data(cell)
            assert float(maps[0][2].max()) > 2.0 ** 32 and len(np.unique(maps[0][0])) >= 1


def test_every_box_winner_is_planted_and_every_lane_is_visited():
    for dt in C.INT_DTYPES:
        cell = next(c for c in C.family("B") if c["dtype"] == dt and c["mode"] == "global")
        img, temps, regions, winners = C.b_scene(cell)
        maps = C.b_maps(dt)
        assert len(maps) == len(winners) >= 2 * C.WIN_TILE ** 2
        for _, t in temps:
            _border_counts(cell["name"], t)
        for method in C.PLANTED:
            # a unit counts where the planted output is its map's strict extremum, neither tied nor clamped (among unrelated
            # windows of a handful of pixels one may match a template of that size as well: such units are compared with the
            # oracle's extremum like the others, they just do not count here)
            lanes, second, planted = set(), set(), 0
            for ref, (wy, wx), (_, t) in zip(maps, winners, temps):
                cmap = ref[method]
                assert cmap.shape == C.B_MAP
                y, x, s = C.extremum(cmap, method)
                if (y, x) != (wy, wx) or int((cmap == s).sum()) != 1 or not np.isfinite(s):
                    assert t.shape[0] * t.shape[1] <= 16, (dt, method, t.shape, (wy, wx), (y, x))
                    continue
                if method != 0 and not 0.0 < abs(float(s)) < 1.0:
                    continue
                planted += 1
                lanes.add((y % C.WIN_TILE, x % C.WIN_TILE))
                if x >= C.WIN_TILE or y >= C.WIN_TILE:
                    second.add((y % C.WIN_TILE, x % C.WIN_TILE))
            assert len(lanes) == C.WIN_TILE ** 2 and len(second) >= C.WIN_TILE ** 2 - 32, (dt, method, len(lanes), len(second))
            assert 10 * planted >= 9 * len(maps), (dt, method, planted)
            assert {(y, x) for y, x in winners if y == 16 or x == 32}                   # the one-lane tiles
        for method in (3, 5):
            for ref in maps[:C.B_LOCAL_UNITS]:
                _live_map(cell["name"], ref[method], method)
        for border in ("constant", "nearest"):
            local = next(c for c in C.family("B") if c["dtype"] == dt and c.get("border") == border)
            for method in C.ALL:
                exp = C.b_expected(local, method)
                assert len(exp) == C.B_LOCAL_UNITS and min(len(e) for e in exp) >= 1 and sum(len(e) for e in exp) > 20 * len(exp)


def test_every_track_winner_is_planted():
    for cell in C.family("T"):
        frames, temps, tracks, planted, min_score, reacquire = C.t_scene(cell)
        for _, t in temps:
            _border_counts(cell["name"], t)
        by_label = {lab: j for j, (lab, _) in enumerate(temps)}
        seen = set()
        for method in C.PLANTED:
            exp = C.t_expected(cell, method)
            for f, row in enumerate(exp):
                for k, (rec, (v, places), ((bx, by, _, _), js)) in enumerate(zip(row, planted, tracks)):
                    js = C.track_set(js)
                    assert cell.get("plain", False) == isinstance(tracks[k][1], int)
                    lab, (x, y, w, h), sbits = rec
                    assert by_label[lab] == js[v], (cell["name"], method, k)
                    if reacquire:
                        assert (y, x) == (places[0][0] + f, places[0][1] + f), (cell["name"], method, f, k)
                    else:
                        assert (y - by, x - bx) == places[0], (cell["name"], method, k)       # (ties: the first in row-major order)
                    seen.add((len(js),) + C.set_slots(len(js), v))
                    if cell["mode"] == "ties":
                        # exactly the two planted outputs tie for the extremum, under the exact variant(s)
                        frame = frames[0][by:by + h + C.T_MAP[0] - 1, bx:bx + w + C.T_MAP[1] - 1]
                        cmap = C.direct_maps(np.ascontiguousarray(frame), temps[js[v]][1], (method,))[method]
                        _, _, s = C.extremum(cmap, method)
                        assert sorted(map(tuple, np.argwhere(cmap == s).tolist())) == places, (cell["name"], method, k)
        if cell["mode"] == "sets":
            assert len(tracks) >= 96
            assert {(n,) + C.set_slots(n, v) for n, v in ([(1, 0)] if cell.get("plain") else C.T_COMBOS)} == seen
            assert {t.shape[:2] for _, t in temps} == set(C.T_SHAPES)
        if reacquire:
            # min_score is above every in-box score: no record of the plain call would pass it
            for method in C.ALL:
                m = C.never_passes(method)
                for row in C.t_expected(dict(cell), method):
                    for rec in row:
                        s = float(np.uint32(rec[2]).view(np.float32))
                        assert not (s < m if method in (0, 1) else s > m)


def test_the_neighbourhood_scenes_are_honest():
    masks = []
    for cell in C.family("N"):
        img, temps, kinds = C.n_scene(cell)
        h, w = cell["h"], cell["w"]
        flt = cell["dtype"].startswith("f32")
        i3 = O._as3d(img).astype(np.float64)
        var = sum(O.window_sums(i3[:, :, c] ** 2, h, w) * (h * w) - O.window_sums(i3[:, :, c], h, w) ** 2 for c in range(i3.shape[2]))
        assert (var.min() > 0) if flt else (var == 0).sum() >= 4, cell["name"]              # float: no flat window
        assert not flt or img.min() > 0
        for e, kind in zip(temps, kinds):
            exp, ref = C.n_expected(cell, img, e)
            if kind in ("exact", "noisy", "noise"):
                _border_counts(cell["name"], e[1])
            if len(e) > 2:
                _border_counts(cell["name"], e[2])
                if max(h - 2, 0) * max(w - 2, 0) >= 8:
                    masks.append(bool((e[2] == 0).any()))
            for m in cell["methods"]:
                assert exp[m].shape == (C.N_MAP[0] * C.N_MAP[1], 3, 3)
                assert np.isnan(exp[m][0, 0]).all() and np.isnan(exp[m][0, :, 0]).all() and np.isnan(exp[m][-1, 2]).all()
                assert np.array_equal(exp[m][:, 1, 1].reshape(C.N_MAP), ref[m], equal_nan=True)
                if flt:
                    assert np.isfinite(ref[m]).all(), (cell["name"], m)
                if m in (1, 3, 5) and kind in _LIVE and h * w > 1:
                    _live_map(cell["name"], ref[m], (kind, m))
    assert all(masks) and len(masks) > 60               # (a 3 x 2 mask is all border; one with an interior drops pixels)


def test_the_pyramid_scenes_are_honest():
    for cell in C.family("Y"):
        img, temps, places = C.y_scene(cell)
        assert all(y % cell["factor"] == 0 and x % cell["factor"] == 0 for y, x in places)
        for (lab, t), (y, x) in zip(temps, places):
            _border_counts(cell["name"], t)
            for m, cmap in C.direct_maps(img, t, cell["methods"]).items():
                assert C.extremum(cmap, m)[:2] == (y, x) and 0.0 < abs(float(cmap[y, x])) < 1.0
                thr, coarse = C.y_thresholds(m)
                assert (cmap[y, x] < coarse < thr) if m == 1 else (cmap[y, x] > coarse > thr)     # the planted hit passes both
