"""
The conditions tests/test_gpu_masked_cores.py relies on, shown without a GPU from tests/masked_cores_cases.py and the sources:

  * the constants the table mirrors are the sources' - 66051 of mfma_class_ok, kMfmaMaxW, kMfSeg, kMfRows, kMfChunkH, R = 16 and
    nt = 1 of the sum I^2 M pass, kMasksqFusedMaxOnes and the launcher's condition on it;
  * the read-out is exact: every `dark`, `black` and `sparse` read-out cell has its largest sum I^2 M below 2^24, and
    c2_exact is a plain triple loop's result;
  * the range family stands where it claims to: the fused accumulator 256 a_h + a_l = c2 - 32896 n would leave the int32 range
    for at least half the outputs of every `dark` range cell of n >= 65536 set taps, for at least one output at n = 65281
    (c2 < 128: the zero patch of the `black` scene), for none at n <= 65280, and never at the positive end (`sat`);
  * the full-score scenes are honest (the rule of test_exact_kernels_cpu.py): of the normalised maps of exact and noisy
    templates at least half the outputs are finite and not 0, 1 or -1 (one at least in a map of fewer than 16) - but under a
    mask of ONE set tap TM_CCORR_NORMED is I T / sqrt(T^2 I^2) = 1 or 0 / 0 by arithmetic, which is asserted instead; the
    `black` scenes do hold windows of sum I^2 M = 0; `mzero` templates are 0 / 0 everywhere;
  * the table covers every mask kind, every listed width, height, map size and range row, and its names are unique.
"""
import os
import re

import numpy as np
import pytest

import masked_cores_cases as C

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "multitemplatematching-python_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_mirrored_constants_are_the_sources():
    const = lambda text, name: int(re.search(r"\b%s\s*=\s*(\d+)" % name, text).group(1))                     # noqa: E731
    ctx, params, place, launch = _src("mtm_ctx.h"), _src("mtm_mfma_params.h"), _src("mtm_placement.hip"), _src("mtm_launch.hip")
    assert const(ctx, "kMfmaMaxW") == C.MFMA_MAX_W
    assert (const(params, "kMfSeg"), const(params, "kMfRows"), const(params, "kMfChunkH")) == (C.MF_SEG, C.MF_ROWS, C.MF_CHUNK_H)
    assert "if (sc.masked) return c->chans == 1 && (long long)sc.w * sc.h <= %d;" % C.MASKED_MAX_AREA in place
    assert C.MASKED_MAX_AREA * 65025 < 2 ** 32 <= (C.MASKED_MAX_AREA + 1) * 65025
    # the pass: R = 16, nt = 1, whatever the class's tiling; its row block; its K chunks
    assert "mfma_row_mux(p, %d, 1)" % C.SQ_R in launch
    assert re.search(r"void pack_mask_rm\([^)]*\) \{\s*const int h = sc.h, w = sc.w, nb = \(w \+ 63\) / 64, R = %d;" % C.SQ_R, place)
    assert "p.rm_steps = p.h + 2 * R - 1;" in launch and "p.nyb = (p.oh + 8 * R - 1) / (8 * R);" in launch
    assert C.ROW_BLOCK == 8 * C.SQ_R == 128
    assert "static constexpr int kChunk = R2 ? kMfChunkR2 : kMfChunkH;" in _src("mtm_mfma.hip.h")
    assert "return std::min(h + 2 * R - 1, kMfChunkH) + (kMfRows - 1) * 2 * R; }" in ctx
    # the bound of the fused form, and that the launcher applies it (and sizes the raw planes of the unfused form)
    assert const(ctx, "kMasksqFusedMaxOnes") == C.FUSED_MAX_ONES
    assert "257.0 * 128.0 * sc.mask_ones" in launch and C.ACC_PER_BLACK_TAP == 257 * 128
    assert C.ACC_PER_BLACK_TAP * C.FUSED_MAX_ONES <= 2 ** 31 < C.ACC_PER_BLACK_TAP * (C.FUSED_MAX_ONES + 1)
    assert "const bool fused_sq = c->masksq_fused != 0 && sc.mask_ones <= (double)kMasksqFusedMaxOnes;" in launch
    assert "if (!fused_sq) MTMC(c->raw16.ensure(sizeof(int) * (size_t)(2 * raw_map)));" in launch
    assert re.search(r"static_assert\(32896 \* kMasksqFusedMaxOnes <= 2147483648LL", ctx)


def test_names_are_unique_and_the_table_covers_every_edge():
    assert len(set(C.NAMES)) == len(C.NAMES)
    fam = {}
    for c in C.CELLS:
        fam.setdefault(c["family"], []).append(c)
    have = lambda family, pred: any(pred(c) for c in fam.get(family, []))                                     # noqa: E731
    assert all(c["methods"] == (0,) and c["n"] == 1 for c in C.READOUT)
    # every mask kind, at a shape with several 64-tap blocks and at one with two K chunks, on dark and on sparse scenes
    for kind in C.MASK_KINDS:
        cells = [c for c in fam["mask"] if c["mask"] == kind]
        assert {c["scene"] for c in cells} == {"dark", "sparse"}, kind
        assert any(c["w"] > 128 for c in cells) and any(c["h"] + 2 * C.SQ_R - 1 > C.MF_CHUNK_H for c in cells), kind
        if kind != "none":
            assert all(C.mask_set(kind, c["h"], c["w"], np.random.default_rng(0)).any() for c in cells), kind
    # widths: both sides of every 16-tap segment and 64-tap block up to kMfmaMaxW, in one K chunk and in two
    for k in range(64, C.MFMA_MAX_W + 1, 64):
        for w in (k - 1, k, k + 1):
            if w <= C.MFMA_MAX_W:
                assert w in C.W_EDGES, w
    assert {1, 15, 16, 17} <= set(C.W_EDGES) and max(C.W_EDGES) == C.MFMA_MAX_W
    for w in C.W_EDGES:
        assert have("w", lambda c: c["w"] == w and c["h"] + 31 <= C.MF_CHUNK_H) and have("w", lambda c: c["w"] == w and c["h"] + 31 > C.MF_CHUNK_H), w
    assert {c["mask"] for c in fam["w"]} >= {"rand", "lastcol", "ones"}
    # heights: the listed ones and both sides of every K chunk boundary a template of up to 258 rows can cross
    edges = [h for h in range(1, 258) if -(-(h + 31) // C.MF_CHUNK_H) != -(-(h + 32) // C.MF_CHUNK_H)]
    assert sorted(set(edges) | {h + 1 for h in edges}) == sorted(C.H_CHUNK_EDGES)
    for h in C.H_EDGES + C.H_CHUNK_EDGES:
        assert have("h", lambda c: c["h"] == h and c["mask"] == "rand" and c["scene"] == "dark"), h
        assert have("h", lambda c: c["h"] == h and c["scene"] == "sparse"), h
    assert {c["h"] for c in fam["h"] if c["w"] > 128} >= set(C.H_CHUNK_EDGES[:4])
    assert have("h", lambda c: (c["h"], c["w"]) == (258, 256) and c["out"] == C.LARGE_MAP)
    # output geometry at 9 x 40 and 9 x 65
    for shape in ((9, 40), (9, 65)):
        outs = {c["out"] for c in fam["out"] if (c["h"], c["w"]) == shape}
        assert {o[0] for o in outs} >= set(C.OUT_OHS) and {o[1] for o in outs} >= set(C.OUT_OWS), shape
    assert {k * C.SQ_R + d for k in (1, 2, 8) for d in (-1, 0, 1)} <= set(C.OUT_OHS) and 1 in C.OUT_OHS
    assert {C.MF_SEG - 1, C.MF_SEG, C.MF_SEG + 1, C.MF_SEG + 3, 1, 2, 3, 4} <= set(C.OUT_OWS)
    assert {ow % 4 for ow in C.OUT_OWS} == {0, 1, 2, 3} and {ow % 4 for ow in C.OUT_OWS if ow > C.MF_SEG} >= {1, 3}
    assert have("out", lambda c: c["out"] == (1, 1))
    assert have("out", lambda c: c["out"][0] > C.ROW_BLOCK and c["out"][1] > C.MF_SEG)          # a second row block AND segment
    assert all(c["out"] in (C.DEFAULT_MAP, C.LARGE_MAP) for c in C.CELLS if c["family"] in ("mask", "w", "h", "range", "hits"))
    assert all(c["out"] == C.LARGE_MAP for c in C.CELLS if c["h"] * c["w"] > 40000)
    assert C.DEFAULT_MAP[0] > 2 * C.SQ_R                                                       # both MFMA groups, a second wave
    # the range family: every row on both scenes, with the set taps the table states
    for h, w, kind, n in C.RANGE_ROWS:
        for s in ("dark", "black"):
            assert have("range", lambda c: (c["h"], c["w"], c["mask"], c["scene"]) == (h, w, kind, s)), (h, w, kind, s)
        assert int(C.mask_set(kind, h, w, np.random.default_rng(0)).sum()) == n
    assert [n for _, _, _, n in C.RANGE_ROWS] == [65280, 65536, 65280, 65281, 66048, 66049, 66304]
    assert [C.on_cores(h, w) for h, w, _, _ in C.RANGE_ROWS] == [True] * 5 + [False] * 2
    assert have("range", lambda c: c["scene"] == "sat" and c["h"] * c["w"] == 66048 and c["mask"] == "ones")
    # full scores: the mask kinds, scenes, methods and template counts asked for; both forms of the pass; hits-only on black
    score = fam["score"]
    assert {c["mask"] for c in score} >= {"ones", "corners", "last", "col63", "rand"}
    assert {c["scene"] for c in score} == {"dark", "noise"} and {c["n"] for c in score} == {1, 3, 20}
    assert all(c["methods"] == C.METHODS for c in score)
    assert {k for c in score for k in C.kinds_of(c)} == {"exact", "noisy", "mzero"}
    assert {C.expected_route(c, C.cell_data(c)["n_set"])[2] for c in score} == {"fused", "unfused"}
    assert have("score", lambda c: c["out"][0] > C.ROW_BLOCK and c["out"][1] > C.MF_SEG)
    assert all(c["scene"] == "black" and c["methods"] == (1, 3) for c in fam["hits"])
    assert {C.expected_route(c, C.cell_data(c)["n_set"])[2] for c in fam["hits"]} == {"fused", "unfused"}


def test_c2_exact_is_a_plain_triple_loop():
    cell = next(c for c in C.CELLS if c["family"] == "mask" and c["mask"] == "rand" and c["h"] == 9)
    d = C.cell_data(cell)
    img, mask = [[int(v) for v in row] for row in d["img"]], [[int(v) for v in row] for row in d["mask"]]
    oh, ow = cell["out"]
    for y in range(0, oh, 7):
        for x in range(0, ow, 5):
            s = 0
            for dy in range(cell["h"]):
                for dx in range(cell["w"]):
                    if mask[dy][dx] > 0:
                        s += img[y + dy][x + dx] ** 2
            assert s == int(d["c2"][y, x]), (y, x)


@pytest.mark.parametrize("cell", C.READOUT, ids=[c["name"] for c in C.READOUT])
def test_the_read_out_is_exact(cell):
    d = C.cell_data(cell)
    assert set(np.unique(d["mask"]).tolist()) <= {0, 1, 128, 255}
    assert all(not t.any() for t, _ in d["units"])                                             # the all-zero template: c1 = 0
    if cell["scene"] == "sat":
        assert int(d["c2"].min()) == 65025 * d["n_set"] > 2 ** 24                                # (read through float32 rounding)
        assert (126 * 256 - 127) * d["n_set"] < 2 ** 31                                          # the positive end fits
        return
    assert 0 <= int(d["c2"].min()) and int(d["c2"].max()) < 2 ** 24, (cell["name"], int(d["c2"].max()))
    assert np.array_equal(d["refs"][0][0].astype(np.int64), d["c2"])
    if cell["scene"] in ("dark", "black"):
        assert int(d["img"].max()) <= 15                                                       # J_h = 0: its biased plane is -128
    if cell["scene"] == "black":
        assert int(d["c2"][C.zero_patch(*cell["out"])]) == 0
    if cell["scene"] == "sparse" and d["n_set"] >= 9:
        assert int(d["img"].max()) >= 16 and int(d["c2"].max()) >= 256                         # both byte planes are met
    if cell["mask"] != "none":
        assert d["n_set"] > 0 and (cell["scene"] != "dark" or int(d["c2"].max()) > 0)


@pytest.mark.parametrize("cell", C.RANGE, ids=[c["name"] for c in C.RANGE])
def test_the_range_family_stands_at_the_bound(cell):
    d = C.cell_data(cell)
    n, wraps = d["n_set"], C.would_wrap(d["c2"], d["n_set"])
    assert n == next(r[3] for r in C.RANGE_ROWS if r[:3] == (cell["h"], cell["w"], cell["mask"]))
    if cell["scene"] == "sat" or n <= C.FUSED_MAX_ONES:
        assert not wraps.any(), cell["name"]
    elif n >= 65536 and cell["scene"] == "dark":
        assert 2 * int(wraps.sum()) >= wraps.size, (cell["name"], int(wraps.sum()))
    if n == 65281 and cell["scene"] == "black":
        assert wraps.any() and wraps[C.zero_patch(*cell["out"])] and int(d["c2"].min()) < 128
    if n > C.FUSED_MAX_ONES and cell["scene"] == "black":
        assert wraps.any(), cell["name"]          # every `black` cell above the bound holds an output the fused form cannot


@pytest.mark.parametrize("cell", C.SCORE, ids=[c["name"] for c in C.SCORE])
def test_the_full_score_scenes_are_honest(cell):
    d = C.cell_data(cell)
    tiny = cell["out"][0] * cell["out"][1] < 16
    live = [i for i, k in enumerate(d["kinds"]) if k in ("exact", "noisy")]
    assert live
    for m in cell["methods"]:
        for i, kind in enumerate(d["kinds"]):
            r = d["refs"][m][i]
            if kind == "mzero":
                assert float(((d["units"][i][0].astype(np.float64) * (d["mask"] > 0)) ** 2).sum()) == 0.0
                if m in (1, 3):
                    assert not np.isfinite(r).any(), (cell["name"], m)
                continue
            if m not in (1, 3):
                assert np.isfinite(r).all(), (cell["name"], m, kind)
                continue
            if d["n_set"] == 1 and m == 3:
                assert (np.isnan(r) | (r == 1.0)).all() and (r == 1.0).any(), (cell["name"], kind)   # I T / sqrt(T^2 I^2)
                continue
            ok = np.isfinite(r) & ~np.isin(r, (0.0, 1.0, -1.0))
            assert ok.any() if tiny else 2 * int(ok.sum()) >= ok.size, (cell["name"], m, kind, int(ok.sum()), ok.size)
    if cell["scene"] == "black":
        assert int(d["c2"].min()) == 0 and np.isnan(d["refs"][3][live[0]][C.zero_patch(*cell["out"])])
