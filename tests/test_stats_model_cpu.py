"""tests/stats_model.py - the numpy restatement tests/test_gpu_window_stats.py holds the fused statistics kernel to - checked
itself: against a literal double loop on tiny cases, against the tail-box quantities of tests/test_tail_bound_cpu.py's
restatement, and against the oracle's window sums and normalisation where it has them."""
import numpy as np
import pytest

import mtm_oracle as O
import stats_model as M
from test_tail_bound_cpu import _bound_and_num


def _literal(image, h, w, num_type, tail_s):
    rows, cols = image.shape
    g = M.geometry(rows, cols, h, w)
    oh, ow, sp, bp = g["oh"], g["ow"], g["st_pitch"], g["blk_pitch"]
    px = lambda y, x: int(image[y, x]) if x < cols else 0          # noqa: E731  (the zero padding right of the image)
    out = {k: np.zeros((oh, sp)) for k in ("t0", "sum2", "sq", "rsq")}
    out["blk"], out["blkq"] = np.zeros((oh, bp, 4)), np.zeros((oh, bp, 4))
    for y in range(oh):
        rq = range(y + tail_s - (y & 1), y + h)                      # the tail box's image rows
        rec = {}
        for x in range(sp):
            s1 = sum(px(y + dy, x + dx) for dy in range(h) for dx in range(w))
            s2 = sum(px(y + dy, x + dx) ** 2 for dy in range(h) for dx in range(w))
            mean2 = (float(s1) * float(s1)) * (1.0 / (float(h) * float(w))) if num_type == 1 else 0.0
            d = max(float(s2) - mean2, 0.0)
            sq = 0.0 if d <= min(0.5, (10.0 * M.FLT_EPSILON) * float(s2)) else float(np.sqrt(np.float64(d)))
            out["t0"][y, x], out["sum2"][y, x], out["sq"][y, x] = s1, s2, sq
            out["rsq"][y, x] = 1.0 / sq if sq > 0.0 else 0.0
            if x < ow:
                rq = rq if tail_s else ()
                q1 = sum(px(r, x + dx) for r in rq for dx in range(w))
                q2 = sum(px(r, x + dx) ** 2 for r in rq for dx in range(w))
                rec.setdefault(x // 16, []).append((s1, sq, q1, len(rq) * w * q2 - q1 * q1))
        for b in range(bp):
            r = rec.get(b)
            if r is None:
                out["blk"][y, b] = (0.0, 0.0, np.inf, 0.0)
                continue
            out["blk"][y, b] = (min(v[0] for v in r), max(v[0] for v in r), min(v[1] for v in r), 0.0)
            if not tail_s:
                continue
            nq = float(len(rq) * w)
            vm = float(np.sqrt(np.float64(max(v[3] for v in r)) * (1.0 / nq)) * (1.0 + 2.0 ** -49))
            out["blkq"][y, b] = (min(v[2] for v in r), max(v[2] for v in r), vm, 0.0)
    return out


@pytest.mark.parametrize("rows,cols,h,w,tail_s", [(6, 9, 3, 2, 1), (7, 21, 4, 5, 2), (5, 40, 5, 3, 4), (9, 18, 2, 1, 1),
                                                  (4, 4, 1, 1, 0), (12, 33, 7, 16, 5)])
@pytest.mark.parametrize("num_type", [0, 1, 2])
def test_model_is_the_literal_double_loop(rows, cols, h, w, tail_s, num_type):
    rng = np.random.default_rng(rows * 100 + cols + num_type)
    for image in (rng.integers(0, 256, (rows, cols), dtype=np.uint8), np.full((rows, cols), 255, np.uint8),
                  np.zeros((rows, cols), np.uint8)):
        got, exp = M.window_stats(image, h, w, num_type, tail_s), _literal(image, h, w, num_type, tail_s)
        for k in got:
            assert got[k].tobytes() == exp[k].tobytes(), k


@pytest.mark.parametrize("h,w,split", [(64, 64, 42), (20, 24, 12), (8, 16, 6)])
def test_tail_boxes_are_those_of_the_bound(h, w, split):
    """test_tail_bound_cpu restates the bound the score kernel builds from the records: its window sum, S1_Q and sqrt(V_Q) for
    the wave's first row (q0 = split, even output row) and second (q0 = split - 1, odd) are the model's - so with a zero
    template prefix, unit tail and one window per block the bound's terms can be read off."""
    rng = np.random.default_rng(h + w)
    image = rng.integers(0, 256, (h + 1, w), dtype=np.uint8)         # output rows 0 (even) and 1 (odd), one column
    m = M.window_stats(image, h, w, 1, split)
    for y, q0 in ((0, split), (1, split - 1)):
        I = image[y:y + h].astype(np.int64)
        Q = I[q0:]
        nq = Q.size
        s1q, s2q = int(Q.sum()), int((Q ** 2).sum())
        vq = np.sqrt((nq * s2q - s1q * s1q) * (1.0 / nq)) * (1.0 + 2.0 ** -49)          # _bound_and_num's line, verbatim
        assert m["blkq"][y, 0].tolist() == [float(s1q), float(s1q), float(vq), 0.0]
        assert m["blk"][y, 0, 0] == m["blk"][y, 0, 1] == float(I.sum()) == m["t0"][y, 0]
        T = rng.integers(0, 256, (h, w))
        bound, num = _bound_and_num(I, T, q0, 5)
        assert bound >= num


@pytest.mark.parametrize("rows,cols,h,w", [(40, 70, 8, 16), (33, 129, 17, 64), (64, 64, 64, 64)])
def test_model_against_the_oracle(rows, cols, h, w):
    """The oracle's window sums (float64 integral images: exact at these sizes) and its TM_CCOEFF_NORMED normalisation."""
    rng = np.random.default_rng(rows + cols)
    image = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    m = M.window_stats(image, h, w, 1)
    ow = cols - w + 1
    f = image.astype(np.float64)
    assert np.array_equal(m["t0"][:, :ow], O.window_sums(f, h, w))
    assert np.array_equal(m["sum2"][:, :ow], O.window_sums(f * f, h, w))
    var = m["sum2"][:, :ow] - m["t0"][:, :ow] ** 2 / (h * w)
    assert np.allclose(m["sq"][:, :ow], np.sqrt(np.maximum(var, 0.0)), rtol=1e-12, atol=1e-3)
    assert np.array_equal(m["rsq"] > 0, m["sq"] > 0)


def test_converted_planes():
    image = np.arange(12 * 8, dtype=np.uint8).reshape(12, 8)
    u8, u8b = M.converted_planes(image, 3, 7, 0xA5)
    assert u8.shape == (12, 576) and (u8[3:7, :8] == image[3:7]).all() and (u8b[3:7, :8] == image[3:7] ^ 0x80).all()
    assert (u8[:3] == 0xA5).all() and (u8[7:] == 0xA5).all() and (u8b[3:7, 8:] == 0xA5).all()


def test_window_stats_block_matches_the_header():
    """mtm_debug_window_stats (test support): the binding's argument block has the header's fields in the header's order, as
    many forms as the header says, and the entry point refuses null arguments without a GPU."""
    import ctypes
    import os
    import re
    import build as mtm_build
    mtm_build.build()
    from MTM import _lib
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "mtm_hip.h")).read()
    body = hdr[hdr.index("typedef struct mtm_window_stats {"):hdr.index("} mtm_window_stats;")]
    fields = [f for line in body.splitlines()[1:] for f in re.findall(r"\b([a-z_0-9]+)\s*[,;]", line)]
    assert fields == [f[0] for f in _lib.MtmWindowStats._fields_], fields
    assert ctypes.sizeof(_lib.MtmWindowStats) == 14 * 4 + 11 * 8
    assert int(re.search(r"#define\s+MTM_STATS_FORMS\s+(\d+)", hdr).group(1)) == len(_lib.STATS_FORMS)
    assert len(_lib.STATS_INFO_FIELDS) == 8 and "info[8]" in hdr
    assert _lib.load().mtm_debug_window_stats(None, None) == -1
    assert b"mtm_debug_window_stats" in _lib.load().mtm_last_error()
