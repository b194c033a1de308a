"""
The conditions tests/test_gpu_exact_kernels.py relies on, shown without a GPU:

  * its table covers the edges it is there for (a table edit cannot silently drop one), against the kernels' constants as
    csrc/mtm_score_params.h and csrc/mtm_launch.hip state them;
  * every scene of the table is exact data: pixels, templates and weights are dyadic, and no partial sum of any chain - the
    kernels' FMA chains, the window statistics, the oracle's integral images - can reach 2^53, so every order of summation
    gives the same float64;
  * mtm_oracle's direct sums are what a triple loop over Python integers gives;
  * the scenes are honest: most of every normalised map is neither saturated nor NaN, most cells have sums a float32
    accumulator could not hold, the masked cells do meet 0 / 0; and the `general` family's float64 oracle is within 2^-40
    relative of the same formulas in np.longdouble.
"""
import os
import re

import numpy as np
import pytest

import mtm_oracle as O
import test_gpu_exact_kernels as G

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "multitemplatematching-python_amd", "csrc")
EXACT = [c for c in G.CELLS if c["dtype"] != "gen"]
GENERAL = [c for c in G.CELLS if c["dtype"] == "gen"]


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_mirrored_constants_are_the_kernels():
    hdr = _src("mtm_score_params.h")
    const = lambda name: int(re.search(r"\b%s\s*=\s*(\d+)" % name, hdr).group(1))                             # noqa: E731
    assert (const("kF64ChunkH"), const("kF64ChunkW"), const("kF64BX"), const("kF64BY")) == (G.F64_CHUNK_H, G.F64_CHUNK_W, G.F64_BX, G.F64_BY)
    assert const("kDotChunk") == G.DOT_CHUNK
    assert int(re.search(r"\bkMaxChans\s*=\s*(\d+)", _src("mtm_kernels.h")).group(1)) == G.K_MAX_CHANS
    launch = _src("mtm_launch.hip")
    variants = re.findall(r"^\s*DOTV\((\d+), (\d+), (\d+), (false|true)\)", launch, re.M)
    assert tuple(tuple(int(v) for v in r[:3]) for r in variants) == G.DOT_VARIANTS
    assert [r[3] for r in variants] == ["false"] * 7 + ["true"] and "kDotWideVariant = %d" % G.DOT_WIDE in launch
    assert "ncc_dot4_kernel<%d, %d, %d, false, true>" % G.MASKSQ_VARIANT in launch
    assert "c->chans * sc.w * sc.h * 65025.0 >= 4294967296.0" in launch and G.is_wide(1, 259, 256) and not G.is_wide(1, 257, 257)


def _fam(*names):
    return [c for c in G.CELLS if c["family"] in names]


def _sides(values, edge):
    """one below, at and one above a multiple of a chunk or tile constant"""
    return {edge - 1, edge, edge + 1} <= set(values)


def test_the_table_covers_every_edge():
    # ---- the float64 kernel, both instantiations
    for masked in (False, True):
        cells = [c for c in _fam("f64_w", "f64_h", "f64_out", "f64_chans") if bool(c["mask"]) == masked]
        ws = {c["w"] for c in cells if c["family"] == "f64_w"}
        hs = {c["h"] for c in cells if c["family"] == "f64_h"}
        assert ws == set(G.F64_WIDTHS) and hs == set(G.F64_HEIGHTS)
        last = lambda w: (w - 1) % G.F64_CHUNK_W + 1                                                          # noqa: E731
        assert {last(w) % 4 for w in ws} == {0, 1, 2, 3}                                   # cw % 4 of the last chunk
        assert {last(w) % 4 for w in ws if w > G.F64_CHUNK_W} == {0, 1, 2, 3}              # ... behind a full chunk
        assert all(_sides(ws, k * G.F64_CHUNK_W) for k in (1, 2)) and 3 * G.F64_CHUNK_W + 1 in ws
        assert all(_sides(ws, k) for k in (4, 36)) and {1, 2, 3} <= ws                     # float4 boundaries
        assert all(_sides(hs, k * G.F64_CHUNK_H) for k in (1, 2)) and {1, 3 * G.F64_CHUNK_H + 1} <= hs
        assert {c["n"] for c in cells} >= {1, 3}                                           # grid.y
        outs = {c["out"] for c in cells}
        assert {o[1] % 4 for o in outs} == {0, 1, 2, 3} and {o for o in outs if 1 in o}
    outs = {c["out"] for c in _fam("f64_out")}
    assert {o[1] for o in outs} >= set(G.F64_OWS) and {o[0] for o in outs} >= set(G.F64_OHS) and (1, 1) in outs
    assert _sides({o[1] for o in outs}, G.F64_BX) and 2 * G.F64_BX + 1 in {o[1] for o in outs}
    assert _sides({o[0] for o in outs}, G.F64_BY) and 2 * G.F64_BY + 1 in {o[0] for o in outs}
    assert G.DEFAULT_MAP[1] > G.F64_BX and G.DEFAULT_MAP[0] > G.F64_BY                     # every other cell crosses both edges
    for masked in (False, True):
        ch = [c for c in _fam("f64_chans", "f64_w") if bool(c["mask"]) == masked]
        assert {c["chans"] for c in ch} == {1, 2, 3, G.K_MAX_CHANS}
        assert any(c["chans"] == G.K_MAX_CHANS and c["h"] > G.F64_CHUNK_H and c["w"] > G.F64_CHUNK_W for c in ch)
    f64 = [c for c in G.CELLS if c["kernel"] == "f64" and c["dtype"] != "gen"]
    assert {m for c in f64 if not c["mask"] and c["dtype"] in ("f32i", "f32q") for m in c["methods"]} == set(range(6))
    assert {m for c in _fam("f64_u16rgb") for m in c["methods"]} == {3, 5} and all(c["chans"] == 3 for c in _fam("f64_u16rgb"))
    for dt, fam in (("f32i", "f64_w"), ("f32q", "f64_w"), ("u16", "f64_u16mask"), ("u8", "f64_u8rgbmask"), ("u8", "f64_u8large")):
        got = [c for c in _fam(fam) if c["dtype"] == dt and c["mask"]]
        assert got and {m for c in got for m in c["methods"]} >= ({3, 1} if fam == "f64_u8large" else set(G.MASKED_METHODS)), (dt, fam)
    assert {c["mask"] for c in f64 if c["mask"] and c["dtype"] in ("f32i", "f32q")} == {"bin", "wt"}
    assert {c["mask"] for c in _fam("f64_u16mask")} == {"bin", "wt"}
    assert all(c["chans"] == 3 for c in _fam("f64_u8rgbmask"))
    assert [c for c in _fam("f64_u8large") if c["h"] * c["w"] > 66051 and c["chans"] == 1 and c["out"][1] > G.F64_BX]
    # ---- the dot4 kernel
    dot = [c for c in G.CELLS if c["kernel"] == "dot4"]
    crossing = {c["variant"] for c in _fam("dot_variants") if c["out"] == (33, 257)}
    assert crossing == set(range(7))
    for px, py, _ in G.DOT_VARIANTS[:7]:
        assert 257 > 32 * px and 257 % (32 * px) == 1 and 33 % (8 * py) == 1               # last tiles of one column, one row
    assert {c["variant"] for c in _fam("dot_variants") if c["out"] == (1, 1)} == set(range(7))
    assert {c["variant"] for c in _fam("dot_variants") if c["out"][0] < 16 and 1 < c["out"][1] < 128} == set(range(7))
    for v in {c["variant"] for c in _fam("dot_chunks")}:
        ws = {c["w"] for c in _fam("dot_chunks") if c["variant"] == v and c["h"] == 40}
        hs = {c["h"] for c in _fam("dot_chunks") if c["variant"] == v and c["w"] == 40}
        assert ws == set(G.DOT_WIDTHS) and hs == set(G.DOT_HEIGHTS)
        assert all(_sides(ws, k * G.DOT_CHUNK) for k in (1, 2)) and all(_sides(hs, k * G.DOT_CHUNK) for k in (1, 2))
        assert {w % 4 for w in ws} == {0, 1, 3} and {61, 65, 68, 69} <= ws                 # w4 = 64 | 68 | 72: a chunk of 1, 2 dwords
        px, py, _ = G.DOT_VARIANTS[v]
        for c in _fam("dot_chunks"):
            if c["variant"] == v:
                assert c["out"][1] > 32 * px and c["out"][0] > 8 * py, c["name"]           # the map crosses both tile edges
    assert {G.DOT_VARIANTS[v][0] for v in {c["variant"] for c in _fam("dot_chunks")}} == {4, 8} and 0 in {c["variant"] for c in _fam("dot_chunks")}
    for v, nt in ((1, 2), (0, 4), (6, 8)):
        assert G.DOT_VARIANTS[v][2] == nt
        assert {c["n"] for c in _fam("dot_tails") if c["variant"] == v} == {1, nt - 1, nt, nt + 1, 2 * nt + 1}
    works = set()
    for c in _fam("dot_work"):
        px, py, nt = G.DOT_VARIANTS[c["variant"]]
        works.add(-(-c["out"][1] // (32 * px)) * -(-c["out"][0] // (8 * py)) * -(-c["n"] // nt))
    assert works >= {1, 7, 9} and max(works) > 64 and max(works) % 8 != 0
    assert any(c["chans"] == 3 and (c["w"] - 1) % G.DOT_CHUNK == 0 for c in _fam("dot_rgb"))
    limit = {(c["chans"], c["h"], c["w"]): c for c in _fam("dot_limit")}
    assert set(limit) == {(1, 257, 257), (1, 259, 256), (3, 148, 148), (3, 149, 148)}
    assert [G.is_wide(*k) for k in sorted(limit)] == [False, True, False, True]
    assert all(set(c["kinds"]) == {"zero", "sat", "exact"} for c in limit.values())
    assert all(G.expected_route(c)[2] == (G.DOT_WIDE if G.is_wide(c["chans"], c["h"], c["w"]) else c["variant"]) for c in dot)
    # ---- MASKSQ
    for env in (("MTM_ROW_MUX", "0"), ("MTM_FUSE_STATS", "0")):
        cells = [c for c in _fam("masksq") if c["env"] == (env,)]
        assert {c["w"] for c in cells} >= {5, 40, 64, 65} and {c["h"] for c in cells} >= {9, 64, 65}
        assert any(c["h"] * c["w"] == 66048 for c in cells)
        assert all(c["methods"] == (3, 1) and c["mask"] == "bin" and c["dtype"] == "u8" and c["chans"] == 1 for c in cells)
        assert all(c["out"][1] > 32 * G.MASKSQ_VARIANT[0] and c["out"][0] > 8 * G.MASKSQ_VARIANT[1] for c in cells if c["h"] < 258)
    # ---- the naive kernel
    naive = _fam("naive")
    assert {(c["h"], c["w"]) for c in naive} == {(5, 33), (17, 65), (1, 1)}
    for shape in ((5, 33), (17, 65), (1, 1)):
        combos = {(c["dtype"], c["chans"], bool(c["mask"])): c["methods"] for c in naive if (c["h"], c["w"]) == shape}
        assert set(combos) == {("u8", 1, False), ("u8", 3, False), ("u16", 1, False), ("f32q", 1, False), ("f32q", 1, True)}
        assert all(m == (G.MASKED_METHODS if k[2] else G.ALL) for k, m in combos.items())
    # ---- every masked method, every kernel's route expectation
    assert {m for c in G.CELLS if c["mask"] for m in c["methods"]} == set(G.MASKED_METHODS)
    assert {G.expected_route(c)[:2] for c in G.CELLS} == {(0, 0), (1, 1), (2, 2), (3, 3)}
    assert all(set(c["methods"]) == {2, 3} for c in GENERAL) and {bool(c["mask"]) for c in GENERAL} == {False, True}


def _frac_bits(a):
    a = np.asarray(a, np.float64)
    for f in range(0, 40):
        s = a * 2.0 ** f
        if np.array_equal(s, np.rint(s)):
            return f
    return None


@pytest.mark.parametrize("cell", EXACT, ids=[c["name"] for c in EXACT])
def test_every_scene_is_exact_data(cell):
    """Dyadic operands, and the largest partial sum any chain can form - taps x max |I| x max |T M^2| of the score kernels,
    pixels x max I^2 of an integral image over the whole frame - times 2^(fractional bits) stays below 2^53."""
    img, units, kinds, _ = G.cell_data(cell)
    fi, vi = _frac_bits(img), float(np.abs(img).max())
    assert fi is not None and fi <= 2
    taps = cell["chans"] * cell["h"] * cell["w"]
    assert 2.0 ** (2 * fi) * vi * vi * img.size < 2.0 ** 53
    for t, mask in units:
        a, b, mk = G.oracle_inputs(cell, img, t, mask)
        m = np.ones_like(b, np.float64) if mk is None else (mk > 0).astype(np.float64) if mk.dtype == np.uint8 else mk.astype(np.float64)
        k1, k2 = b.astype(np.float64) * m * m, m * m
        f1, f2 = _frac_bits(k1), _frac_bits(k2)
        assert f1 is not None and f2 is not None and _frac_bits(b) <= 2 and _frac_bits(m) <= 3
        assert 2.0 ** (fi + f1) * taps * vi * float(np.abs(k1).max()) < 2.0 ** 53
        assert 2.0 ** (2 * fi + f2) * taps * vi * vi * float(k2.max()) < 2.0 ** 53
        assert 2.0 ** (2 * _frac_bits(b * m)) * taps * float(np.abs(b * m).max()) ** 2 < 2.0 ** 53       # sum T^2, templ2_mask2_sum


def _triple_loop(img2d, ker2d):
    """sum over (dy, dx) of img[y + dy, x + dx] ker[dy, dx] in Python integers (both operands scaled to integers by powers of
    two, the result scaled back: exact), as a float64 map."""
    fi, fk = _frac_bits(img2d), _frac_bits(ker2d)
    a = [[int(v) for v in row] for row in (np.asarray(img2d, np.float64) * 2.0 ** fi)]
    k = [[int(v) for v in row] for row in (np.asarray(ker2d, np.float64) * 2.0 ** fk)]
    H, W, h, w = len(a), len(a[0]), len(k), len(k[0])
    out = np.empty((H - h + 1, W - w + 1), np.float64)
    for y in range(H - h + 1):
        for x in range(W - w + 1):
            s = 0
            for dy in range(h):
                ar, kr = a[y + dy], k[dy]
                for dx in range(w):
                    s += ar[x + dx] * kr[dx]
            assert abs(s) < 2 ** (53 + fi + fk)
            out[y, x] = s / 2.0 ** (fi + fk)            # (exact: an integer below 2^53 times a power of two)
    return out


_SMALL = {"f32-weights": lambda c: c["family"] == "f64_w" and c["w"] <= 5 and c["mask"] == "wt" and c["dtype"] == "f32q",
          "u8-rgb": lambda c: c["family"] == "naive" and c["dtype"] == "u8" and c["chans"] == 3 and c["w"] == 33,
          "u16-mask": lambda c: c["family"] == "f64_u16mask" and c["w"] == 33}


@pytest.mark.parametrize("which", sorted(_SMALL))
def test_direct_sums_are_a_plain_triple_loop(which):
    """The reference does not lean on numpy's summation either: O.sliding_corr(..., force="direct") - the sums every
    epilogue of O.match_template(..., corr="direct") starts from - against Python-integer loops, operand by operand as the
    oracle forms them (masked: I x T M^2 and I^2 x M^2)."""
    cell = next(c for c in G.CELLS if _SMALL[which](c))
    name = cell["name"]
    img, units, kinds, _ = G.cell_data(cell)
    t, mask = units[1]
    a, b, mk = G.oracle_inputs(cell, img, t, mask)
    a3, b3 = O._as3d(a).astype(np.float64), O._as3d(b).astype(np.float64)
    integer = a.dtype == np.uint8
    for c in range(a3.shape[2]):
        if mk is None:
            pairs = [(a3[:, :, c], b3[:, :, c])]
        else:
            m = O._as3d(mk)[:, :, c]
            m = (m > 0).astype(np.float64) if m.dtype == np.uint8 else m.astype(np.float64)
            pairs = [(a3[:, :, c], b3[:, :, c] * m * m), (a3[:, :, c] ** 2, m * m)]
        for x, k in pairs:
            got = O.sliding_corr(x, k, exact_int=integer, force="direct")
            assert got.dtype == np.float64 and np.array_equal(got, _triple_loop(x, k)), (name, c)


def test_the_scenes_are_honest():
    big = 0
    for cell in G.CELLS:
        img, units, kinds, refs = G.cell_data(cell)
        tiny_map, one_tap = cell["out"][0] * cell["out"][1] < 16, cell["h"] * cell["w"] == 1
        live = [i for i, k in enumerate(kinds) if k in ("exact", "noisy", "sat")]
        assert live, cell["name"]
        for m in cell["methods"]:
            for i, kind in enumerate(kinds):
                r = refs[m][i]
                if kind == "const" and m == 5:
                    assert np.array_equal(r, np.ones_like(r)), cell["name"]
                if m not in (1, 3, 5) or i not in live or one_tap:
                    continue
                ok = np.isfinite(r) & ~np.isin(r, (0.0, 1.0, -1.0))
                assert ok.any() if tiny_map else 2 * int(ok.sum()) >= ok.size, (cell["name"], m, kind, int(ok.sum()), ok.size)
        if cell["mask"] and cell["dtype"] != "gen" and "mzero" in kinds and 3 in cell["methods"]:
            # the template that is zero under its mask: 0 / 0 everywhere; the region that is zero under the mask: NaN for all
            assert np.isnan(refs[3][kinds.index("mzero")]).all(), cell["name"]
            if cell["out"] == G.DEFAULT_MAP and cell["w"] <= 37:
                assert np.isnan(refs[3][0]).any() and not np.isnan(refs[3][0]).all(), cell["name"]
        # an exact copy's sum at its own position, sum (T M)^2, is one of the sums the kernel forms
        own = 0.0
        for (t, mask), kind in zip(units, kinds):
            if kind == "exact":
                _, b, mk = G.oracle_inputs(cell, img, t, mask)
                m = 1.0 if mk is None else (mk > 0).astype(np.float64) if mk.dtype == np.uint8 else mk.astype(np.float64)
                own = max(own, float(((b.astype(np.float64) * m) ** 2).sum()))
        big += own > 2.0 ** 24
    assert 2 * big > len(G.CELLS), (big, len(G.CELLS))          # a float32 accumulator could not pass most cells


@pytest.mark.parametrize("cell", GENERAL, ids=[c["name"] for c in GENERAL])
def test_the_general_family_in_longdouble(cell):
    """TM_CCORR and TM_CCORR_NORMED of the inexact scenes: the oracle's formulas over float64 direct sums against the same over
    np.longdouble direct sums agree to 2^-40 relative - and the float64 ones round to the oracle's float32 maps."""
    if np.finfo(np.longdouble).nmant <= 52:
        pytest.skip("np.longdouble is float64 on this platform")
    img, units, kinds, refs = G.cell_data(cell)
    i3 = O._as3d(img)
    for idx, (t, mask) in enumerate(units):
        t3 = O._as3d(t)
        m3 = None if mask is None else O._as3d(mask)
        vals = {}
        for dt in (np.float64, np.longdouble):
            c1 = c2 = 0
            tms = dt(0)
            for c in range(i3.shape[2]):
                a, b = i3[:, :, c].astype(dt), t3[:, :, c].astype(dt)
                m2 = np.ones_like(b) if m3 is None else m3[:, :, c].astype(dt) ** 2
                c1 = c1 + O.corr_direct(a, b * m2, dt)
                c2 = c2 + O.corr_direct(a * a, m2, dt)
                tms = tms + (b * b * m2).sum()
            vals[dt] = (c1, c1 / np.sqrt(tms * c2))
        for k, method in enumerate((2, 3)):
            lo, hi = vals[np.float64][k], vals[np.longdouble][k]
            rel = np.abs(lo.astype(np.longdouble) - hi) / np.abs(hi)
            assert float(rel.max()) < 2.0 ** -40, (cell["name"], idx, method, float(rel.max()))
            ref = refs[method][idx]
            plain = ref < 1.0 if method == 3 else np.ones(ref.shape, bool)     # (an exact copy's own position saturates at 1)
            near = np.abs(lo.astype(np.float32).view(np.int32).astype(np.int64) - ref.view(np.int32)) <= 1
            assert near[plain].all() and plain.sum() >= plain.size - 1, (cell["name"], idx, method)
