"""
A plain reference of MTM's non-maxima suppression and the table of hit lists the device's NMS kernels are swept with
(tests/test_nms_model_cpu.py validates both on the CPU, tests/test_gpu_device_nms.py runs the table on the device).

Pure Python / numpy: nothing here calls the library.  The definitions are those of csrc/mtm_nms_core.h:

  order       the transformed score in float32 - 1 - s for the difference methods ("ascending"), then + 0.0 so that -0 is +0 -
              descending; ties by templ_idx, then by the raw score (ascending lists: the smaller one first), then y, then x
  candidate   a hit whose transformed score is > float32(threshold), the threshold transformed in double (1 - t for
              ascending lists) and narrowed; NaN is never a candidate
  overlap     the exact IoU of two boxes, a fraction of integer areas, compared with Fraction(float32(max_overlap))

and, by brute force over all pairs of candidates, with no grid:

  champions   candidates that no earlier candidate overlaps beyond the limit
  undecided   candidates that are not champions and that no champion overlaps beyond the limit
  greedy      walk the candidates in order, keep one iff no kept one overlaps it beyond the limit

The kernels compute 1.0f - (float)(1.0 - i / u) where this file compares fractions: the two can only disagree on an IoU
within float32 rounding (1.2e-7) of the limit.  `margin_violations` lists the pairs of a case whose IoU is neither the limit
itself nor more than 1e-6 away from it; the CPU test asserts there is none in the whole table.
"""
import collections
import functools
from fractions import Fraction

import numpy as np

HIT_DTYPE = np.dtype([("templ_idx", "<i4"), ("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4"), ("score", "<f4")])


# ---- the grid rule, as the header comment of nms_grid (csrc/mtm_nms_core.h) states it ------------------------------------
def grid(rows, cols, max_side):
    """-> (cell, gw, gh): cell = max(32, max_side), gw = cols / cell + 3, gh = rows / cell + 3 (integer divisions)"""
    cell = max(32, max_side)
    return cell, cols // cell + 3, rows // cell + 3


def cell_of(x, y, rows, cols, max_side):
    """the cell index a hit at (x, y) is filed under"""
    cell, gw, gh = grid(rows, cols, max_side)
    return (min(max(y // cell, 0), gh - 3) + 1) * gw + min(max(x // cell, 0), gw - 3) + 1


def cells_per_thread(n_cells):
    """the prefix kernel's 1024 threads own this many consecutive cells each"""
    return (n_cells + 1023) // 1024


# ---- order and candidates ------------------------------------------------------------------------------------------------
def transformed_scores(hits, ascending):
    s = hits["score"].astype(np.float32)
    with np.errstate(invalid="ignore"):
        return ((np.float32(1.0) - s) if ascending else s) + np.float32(0.0)


def transformed_threshold(score_threshold, ascending):
    return np.float32(1.0 - float(score_threshold)) if ascending else np.float32(score_threshold)


def candidate_order(hits, score_threshold, ascending):
    """indices of the candidates of `hits`, earliest first"""
    ts = transformed_scores(hits, ascending)
    with np.errstate(invalid="ignore"):
        cand = np.nonzero(ts > transformed_threshold(score_threshold, ascending))[0]
    h = hits[cand]
    raw = h["score"].astype(np.float64)
    key = np.lexsort((h["x"], h["y"], raw if ascending else -raw, h["templ_idx"], -ts[cand].astype(np.float64)))
    return cand[key]


def find_order(hits, ascending):
    """`hits` in the order mtm_find_matches returns a list: template, descending quality (score, or -score), row-major
    position.  NMSBoxes' stable sort by the transformed score resolves ties in the order the list arrives in: this one."""
    raw = hits["score"].astype(np.float64)
    q = np.where(np.isnan(raw), np.inf, raw if ascending else -raw)          # (NaN last; never a candidate)
    return hits[np.lexsort((hits["x"], hits["y"], q, hits["templ_idx"]))]


# ---- exact overlap -------------------------------------------------------------------------------------------------------
def limit_fraction(max_overlap):
    return Fraction(float(np.float32(max_overlap)))


def iou(a, b):
    """the exact IoU of two records as a Fraction"""
    iw = min(int(a["x"]) + int(a["w"]), int(b["x"]) + int(b["w"])) - max(int(a["x"]), int(b["x"]))
    ih = min(int(a["y"]) + int(a["h"]), int(b["y"]) + int(b["h"])) - max(int(a["y"]), int(b["y"]))
    i = iw * ih if iw > 0 and ih > 0 else 0
    return Fraction(i, int(a["w"]) * int(a["h"]) + int(b["w"]) * int(b["h"]) - i)


def _areas(h):
    """pairwise intersection and union areas (int64 matrices)"""
    x0, y0 = h["x"].astype(np.int64), h["y"].astype(np.int64)
    x1, y1 = x0 + h["w"], y0 + h["h"]
    iw = np.minimum(x1[:, None], x1[None, :]) - np.maximum(x0[:, None], x0[None, :])
    ih = np.minimum(y1[:, None], y1[None, :]) - np.maximum(y0[:, None], y0[None, :])
    inter = np.where((iw > 0) & (ih > 0), iw * ih, 0)
    area = (x1 - x0) * (y1 - y0)
    return inter, area[:, None] + area[None, :] - inter


def _cross(h, max_overlap):
    """i * q - p * u for every pair, p / q = Fraction(float32(max_overlap)): the sign of IoU - limit, in exact integers"""
    lim = limit_fraction(max_overlap)
    p, q = lim.numerator, lim.denominator
    inter, union = _areas(h)
    assert len(h) == 0 or (int(inter.max()) * q < 2 ** 62 and int(union.max()) * max(p, 1) < 2 ** 62)
    return inter * q - union * p, union * q


def beyond(h, max_overlap):
    """bool matrix: IoU(h[i], h[j]) > the limit (the Fraction comparison, cross-multiplied)"""
    return _cross(h, max_overlap)[0] > 0


def margin_violations(hits, max_overlap):
    """pairs (i, j, IoU) whose IoU is neither exactly the limit nor more than 1e-6 away from it"""
    num, den = _cross(hits, max_overlap)
    bad = (num != 0) & (np.abs(num).astype(np.float64) <= 1.000001e-6 * den.astype(np.float64))
    return [(int(i), int(j), iou(hits[i], hits[j])) for i, j in zip(*np.nonzero(np.triu(bad, 1)))]


# ---- the three sets ------------------------------------------------------------------------------------------------------
Reference = collections.namedtuple("Reference", "champions undecided greedy n_candidates")


def reference(hits, score_threshold, ascending, max_overlap):
    """-> Reference: record arrays, each in NMS order"""
    order = candidate_order(hits, score_threshold, ascending)
    h = hits[order]
    over = beyond(h, max_overlap)
    np.fill_diagonal(over, False)
    beaten = np.tril(over, -1).any(axis=1)              # an EARLIER candidate overlaps it
    champ = ~beaten
    doomed = over[:, champ].any(axis=1)                 # a champion overlaps it (never true of a champion: it would be earlier)
    assert not (doomed & champ).any()
    return Reference(h[champ], h[beaten & ~doomed], h[_greedy_walk(over, 0)], len(h))


def _greedy_walk(over, n_sure):
    kept = []
    for k in range(over.shape[0]):
        if k < n_sure or not over[k, kept].any():
            kept.append(k)
    return np.asarray(kept, dtype=np.int64)


def greedy(hits, score_threshold, ascending, max_overlap, sure=None):
    """Plain greedy NMS of `hits` -> the kept records in order.  `sure`: records to take as kept without testing them
    (the champions of a pruned list), whatever their place in the order."""
    if sure is not None and len(sure):
        hits = np.concatenate([sure, hits])
    order = candidate_order(hits, score_threshold, ascending)
    h = hits[order]
    over = beyond(h, max_overlap)
    np.fill_diagonal(over, False)
    if sure is None or not len(sure):
        return h[_greedy_walk(over, 0)]
    is_sure = order < len(sure)
    kept = []
    for k in range(len(h)):
        if is_sure[k] or not over[k, kept].any():
            kept.append(k)
    return h[np.asarray(kept, dtype=np.int64)]


# ---- the table -----------------------------------------------------------------------------------------------------------
# expect: for the geometry cases, the (n_cells, cell, cells per prefix thread) the case is named for
Case = collections.namedtuple("Case", "name hits rows cols max_side score_threshold ascending max_overlap n_min n_max runs expect")
CASES = []
_NAMES = set()


def mk(records):
    return np.array([tuple(r) for r in records], dtype=HIT_DTYPE).reshape(-1)


def _case(name, hits, geom, max_overlap, score_threshold=0.5, ascending=False, n_min=1, n_max=1 << 18, runs=True, expect=None,
          shuffle=True):
    hits = mk(hits) if not isinstance(hits, np.ndarray) else hits
    if shuffle and len(hits) > 1:                       # the device takes the list in any order
        hits = hits[np.random.default_rng(len(CASES) + 17).permutation(len(hits))]
    assert name not in _NAMES
    _NAMES.add(name)
    rows, cols, max_side = geom
    CASES.append(Case(name, np.ascontiguousarray(hits), rows, cols, max_side, score_threshold, ascending, max_overlap, n_min, n_max,
                      runs, expect))


def _scores(n, rng):
    """n distinct float32 scores in (0.5, 1), in random order"""
    assert n < 2048
    return (np.float32(0.5) + rng.permutation(np.arange(1, n + 1)).astype(np.float32) / np.float32(4096.0)).astype(np.float32)


# (rows, cols, max_side) -> (n_cells, cell, cells per prefix thread)
G276 = (300, 640, 32)             # 23 x 12 cells: the geometry of test_fused_nms_call_equals_find_then_nms
GEOMETRIES = collections.OrderedDict([
    ("cells276", (G276, (276, 32, 1))),
    ("cells1024", ((945, 933, 32), (1024, 32, 1))),                 # 32 x 32: the last thread's single cell is the last cell
    ("cells1025-side33", ((1261, 736, 33), (1025, 33, 2))),         # 25 x 41: thread 512 owns cell 1024 alone, 513 .. idle
    ("cells3000", ((1825, 1535, 32), (3000, 32, 3))),               # 50 x 60: three cells per thread, threads 1000 .. idle
    ("side100", ((1000, 1530, 100), (234, 100, 1))),                # 18 x 13, neither side a multiple of the cell
    ("side257", ((2000, 3000, 257), (140, 257, 1))),                # 14 x 10
    ("thin-cols", ((200, 30, 32), (27, 32, 1))),                    # cols < cell: 3 x 9
    ("thin-rows", ((20, 500, 32), (54, 32, 1))),                    # rows < cell: 18 x 3
    ("thin-both", ((31, 31, 31), (9, 32, 1))),                      # 3 x 3
])


def _cluster(recs, seen, rng, x0, y0, k, sizes, rows, cols, spread, templ0=0, exact=True):
    """k hits around (x0, y0), inside the image, one record per (templ, x, y) (exact=False: fewer where a tiny image has
    no k distinct places)"""
    tries = 0
    while k > 0:
        tries += 1
        if tries > 4000:
            assert not exact
            return
        t = int(rng.integers(len(sizes)))
        w, h = sizes[t]
        x = int(min(max(x0 + rng.integers(-spread, spread + 1), 0), cols - w))
        y = int(min(max(y0 + rng.integers(-spread, spread + 1), 0), rows - h))
        if (templ0 + t, x, y) in seen:
            continue
        seen.add((templ0 + t, x, y))
        recs.append([templ0 + t, x, y, w, h, 0.0])
        k -= 1


def _geometry_records(geom, rng):
    rows, cols, max_side = geom
    cell, gw, gh = grid(*geom)
    n_cells = gw * gh
    per = cells_per_thread(n_cells)
    big = (min(max_side, cols), min(max_side, rows))
    small = (min(8, cols), min(8, rows))
    sizes = [big, small, (min(max(max_side // 2, 5), cols), min(max_side, rows))]
    recs, seen = [], set()

    def put(t, x, y, w, h):
        assert 0 <= x and x + w <= cols and 0 <= y and y + h <= rows and w <= max_side and h <= max_side, (t, x, y, w, h, geom)
        if (t, x, y) not in seen:
            seen.add((t, x, y))
            recs.append([t, x, y, w, h, 0.0])

    # the corners: x = 0, y = 0, x = cols - w, y = rows - h (the clamp of nms_cell_of), with a partner one pixel inside
    for t, (w, h) in enumerate((big, small)):
        for x in (0, cols - w):
            for y in (0, rows - h):
                put(t, x, y, w, h)
                put(t, min(max(x + (1 if x == 0 else -1), 0), cols - w), min(max(y + (1 if y == 0 else -1), 0), rows - h), w, h)
    # ... and the last cell any box can be filed in: a 1 x 1 box in the last pixel, a 2 x 2 one around it
    put(2, cols - 1, rows - 1, 1, 1)
    put(2, cols - 2, rows - 2, 2, 2)
    # pairs straddling a cell border: x / y = k cell - 1 and k cell, horizontally, vertically and on both diagonals
    w, h = min(12, cols), min(10, rows)
    kxs = [k for k in sorted({1, 2, (gw - 3) // 2, gw - 4, gw - 3}) if k >= 1 and k * cell + w <= cols]
    kys = [k for k in sorted({1, 2, (gh - 3) // 2, gh - 4, gh - 3}) if k >= 1 and k * cell + h <= rows]
    mid_x, mid_y = min(cell // 2, cols - w), min(cell // 2, rows - h)
    for n, kx in enumerate(kxs):
        y = min(mid_y + (n * 3 % max(gh - 2, 1)) * cell, rows - h)
        put(3, kx * cell - 1, y, w, h)
        put(3, kx * cell, y, w, h)
    for n, ky in enumerate(kys):
        x = min(mid_x + (n * 5 % max(gw - 2, 1)) * cell, cols - w)
        put(4, x, ky * cell - 1, w, h)
        put(4, x, ky * cell, w, h)
    for kx in kxs:
        for ky in kys[::2]:
            put(5, kx * cell - 1, ky * cell - 1, w, h)          # main diagonal
            put(5, kx * cell, ky * cell, w, h)
            put(6, kx * cell, ky * cell - 1, w, h)              # the other one
            put(6, kx * cell - 1, ky * cell, w, h)
    # two boxes of width (height) exactly `cell` in neighbouring cells, sharing one column (row)
    if max_side == cell:
        for kx in kxs:
            if kx * cell + cell <= cols:
                y = min(3 * cell + 5, rows - small[1])
                put(7, (kx - 1) * cell + 1, y, cell, small[1])
                put(7, kx * cell, y, cell, small[1])
        for ky in kys:
            if ky * cell + cell <= rows:
                x = min(4 * cell + 3, cols - small[0])
                put(8, x, (ky - 1) * cell + 1, small[0], cell)
                put(8, x, ky * cell, small[0], cell)
    # clusters in the first and the last cell in use and, where a prefix thread owns several cells, on both sides of a
    # thread boundary (cells c - 1, c with c a multiple of the span) at the start, the middle and the end of the grid
    targets = [gw + 1, cell_of(cols - 1, rows - 1, *geom)]
    if per > 1:
        for c in (gw + per, n_cells // 2, n_cells - gw - per):
            c -= c % per
            targets += [c - 1, c, c + per - 1, c + per]
    for c in targets:
        cx, cy = min(max(c % gw, 1), gw - 2), min(max(c // gw, 1), gh - 2)
        _cluster(recs, seen, rng, (cx - 1) * cell + cell // 2, (cy - 1) * cell + cell // 2, 5, sizes, rows, cols, cell // 2 - 1, 9, exact=False)
    return recs


def _settle(hits, max_overlap):
    """drops the later record of every pair `margin_violations` lists (random lists only)"""
    while True:
        bad = margin_violations(hits, max_overlap)
        if not bad:
            return hits
        hits = np.delete(hits, sorted({j for _, j, _ in bad}))


def _random_records(seed, geom, n, sizes, tie_step=0, n_clusters=None):
    """n hits (or as many as the image has room for) in clusters (dense cells), scores in (0.3, 1): most above the threshold 0.5, a few below it or NaN"""
    rng = np.random.default_rng(seed)
    rows, cols, max_side = geom
    cell = grid(*geom)[0]
    sizes = [(min(w, cols), min(h, rows)) for w, h in sizes]
    recs, seen = [], set()
    n_clusters = n_clusters or max(1, n // 20)
    left = n
    for c in range(n_clusters):
        k = left if c == n_clusters - 1 else min(left, max(1, n // n_clusters))
        _cluster(recs, seen, rng, int(rng.integers(cols)), int(rng.integers(rows)), k, sizes, rows, cols, max(cell // 3, 6), exact=False)
        left -= k
    hits = mk(recs)
    n = len(hits)                   # (fewer in an image too small for n distinct places)
    s = rng.uniform(0.3, 1.0, n).astype(np.float32)
    if tie_step:
        s = (np.round(s * tie_step) / np.float32(tie_step)).astype(np.float32)
    s[rng.uniform(size=n) < 0.03] = np.nan
    hits["score"] = s
    return hits


def _with_scores(recs, rng):
    hits = mk(recs)
    hits["score"] = _scores(len(hits), rng)
    return hits


def _build():
    rng = np.random.default_rng(20240611)

    # ---- grid geometry: every intersection counts (limit 0), then 0.3 ----
    for name, (geom, expect) in GEOMETRIES.items():
        hits = _with_scores(_geometry_records(geom, rng), rng)
        _case("geo-%s-ov0" % name, hits, geom, 0.0, expect=expect)
        _case("geo-%s-ov0.3" % name, _settle(hits, 0.3), geom, 0.3, expect=expect)

    # ---- one cell holding k mutually intersecting hits (the stride-8 lane split) ----
    for k in (1, 7, 8, 9, 63, 64, 65, 300):
        for ov in (0.0, 0.6):
            recs, seen = [], set()
            _cluster(recs, seen, rng, 3 * 32 + 11, 4 * 32 + 11, 2 * k, [(24, 32), (30, 26)], 300, 640, 11)
            hits = _settle(_with_scores(recs, rng), ov)[:k]             # (twice as many, so that k are left)
            assert len(hits) == k and len({cell_of(r["x"], r["y"], *G276) for r in hits}) == 1
            assert (_areas(hits)[0] > 0).all()
            _case("cellrun-%d-ov%g" % (k, ov), hits, G276, ov)
    # a target with ONE beating partner in its cell, behind j = 0 .. 8 unrelated hits of the cell to the left: the partner
    # sits at every sub-lane position of the grid row's run
    for j in range(9):
        recs = [[0, 5 * 32 + 4, 3 * 32 + 4, 20, 20, 0.6], [0, 5 * 32 + 8, 3 * 32 + 6, 20, 20, 0.9]]
        recs += [[1, 4 * 32 + 4 * f, 3 * 32, 3, 3, 0.95 - 0.01 * f] for f in range(j)]       # disjoint 3 x 3 boxes, all earlier
        _case("sublane-%d" % j, recs, G276, 0.3)

    # ---- candidate counts at the tails of the 8-per-wave and 32-per-block turns (plus two hits that are no candidates) ----
    sizes = [(24, 32), (30, 20), (8, 8)]
    for n in (1, 7, 8, 9, 31, 32, 33, 255, 256, 257):
        hits = _random_records(1000 + n, G276, n, sizes, n_clusters=max(1, n // 6))
        hits["score"] = _scores(n, rng)
        hits = _settle(hits, 0.3)
        if len(hits) < n:                       # keep the count the case is named for: isolated small boxes
            extra = [[7, 600 + 9 * (e % 4), 250 + 9 * (e // 4), 8, 8, 0.99] for e in range(n - len(hits))]
            hits = np.concatenate([hits, mk(extra)])
            hits["score"] = _scores(n, rng)
            assert not margin_violations(hits, 0.3)
        low = mk([[0, 1, 1, 24, 32, 0.25], [1, 2, 2, 30, 20, np.nan]])
        _case("count-%d" % n, np.concatenate([hits, low]), G276, 0.3)

    # ---- n_max = 256 with ~200 candidates: several turns of both grid-stride loops, the LDS counters reused ----
    for seed, geom in ((1, G276), (2, GEOMETRIES["cells3000"][0])):
        hits = _settle(_random_records(2000 + seed, geom, 236, sizes, n_clusters=12), 0.3)
        _case("turns-nmax256-%d" % seed, hits, geom, 0.3, n_max=256)
    # ---- the gate ----
    hits = _settle(_random_records(2100, G276, 40, sizes, n_clusters=4), 0.3)
    n = len(hits)
    _case("gate-n-eq-nmin", hits, G276, 0.3, n_min=n, n_max=4096)
    _case("gate-n-eq-nmax", hits, G276, 0.3, n_min=1, n_max=n)
    _case("gate-n-eq-both", hits, G276, 0.3, n_min=n, n_max=n)
    _case("gate-below-nmin", hits, G276, 0.3, n_min=n + 1, n_max=4096, runs=False)
    _case("gate-above-nmax", hits, G276, 0.3, n_min=1, n_max=n - 1, runs=False)

    # ---- chains a > b > c: a dooms b, only b overlaps c: c comes back undecided ----
    recs = []
    for k, (x, y) in enumerate(((40, 40), (31, 100), (200, 63), (500, 200))):       # 20 x 20, 6 columns apart: 7/13, 12: 1/4
        recs += [[0, x, y, 20, 20, 0.9 - 0.01 * k], [0, x + 6, y, 20, 20, 0.8 - 0.01 * k], [0, x + 12, y, 20, 20, 0.7 - 0.01 * k]]
    recs += [[1, 300 + 6 * k, 128 + 6 * k, 20, 20, 0.95 - 0.05 * k] for k in range(7)]       # a longer one, down a diagonal
    _case("chains", recs, G276, 0.3)

    # ---- hits that are no candidates, on top of candidates: they suppress nothing and are not returned ----
    recs = [[0, 100, 100, 24, 32, 0.8], [1, 100, 100, 24, 32, np.nan], [2, 100, 100, 24, 32, 0.5], [3, 100, 100, 24, 32, 0.49999997],
            [0, 104, 100, 24, 32, np.nan], [0, 200, 50, 24, 32, 0.6], [1, 201, 50, 24, 32, -np.inf], [1, 202, 51, 24, 32, np.nan],
            [2, 200, 50, 24, 32, np.inf], [0, 400, 200, 24, 32, 0.50000006]]
    _case("non-candidates", recs, G276, 0.3)
    _case("score-equals-threshold", [[0, 10, 10, 24, 32, 0.5], [1, 12, 10, 24, 32, 0.5], [0, 300, 10, 24, 32, 0.50000006],
                                     [1, 302, 10, 24, 32, 0.5]], G276, 0.3)
    _case("all-below-threshold", [[0, 10, 10, 24, 32, 0.1], [1, 12, 10, 24, 32, np.nan]], G276, 0.3)

    # ---- ties: one score everywhere, so templ_idx, y and x decide; identical rectangles from different templates ----
    recs, seen = [], set()
    for k, (x0, y0) in enumerate(((50, 50), (128, 64), (400, 150), (606, 262))):
        _cluster(recs, seen, rng, x0, y0, 14, [(24, 32), (24, 32), (30, 20)], 300, 640, 12)
    recs += [[t, 250, 250, 24, 32, 0.0] for t in range(3)] + [[2, 250, 250 - 1, 24, 32, 0.0]]
    hits = mk(recs)
    hits["score"] = 0.75
    for ov in (0.0, 0.5, 1.0):
        _case("ties-all-equal-ov%g" % ov, _settle(hits, ov), G276, ov)
    # ascending lists whose distinct raw scores collapse to one float32 1 - s: the raw score decides
    recs, seen = [], set()
    for x0, y0 in ((60, 60), (300, 128)):
        _cluster(recs, seen, rng, x0, y0, 16, [(24, 32)], 300, 640, 10)
    hits = mk(recs)
    hits["score"] = (np.float32(0.25) + rng.permutation(32).astype(np.float32) * np.float32(2.0 ** -25)).astype(np.float32)
    assert len(np.unique(hits["score"])) == 32 and len(np.unique(transformed_scores(hits, True))) < 32
    _case("ascending-collapse", _settle(hits, 0.3), G276, 0.3, ascending=True)
    tiny = mk(recs[:12])
    tiny["score"] = (np.arange(12) * 1e-9).astype(np.float32)               # 1 - s = 1 for all of them
    tiny["score"][3] = -0.0
    _case("ascending-collapse-at-1", _settle(tiny, 0.3), G276, 0.3, ascending=True)
    # -0.0 and +0.0 are one score
    zeros = mk(recs[:10])
    zeros["score"] = np.where(np.arange(10) % 2, np.float32(-0.0), np.float32(0.0))
    _case("signed-zeros", _settle(zeros, 0.3), G276, 0.3, score_threshold=-0.5)
    _case("signed-zeros-ascending", _settle(zeros, 0.3), G276, 0.3, score_threshold=0.5, ascending=True)

    # ---- mixed box sizes: the cell comes from the largest ----
    geom = (600, 900, 100)
    hits = _settle(_random_records(2200, geom, 120, [(8, 8), (100, 40), (40, 100)], n_clusters=8), 0.3)
    _case("mixed-8x8-100x40", hits, geom, 0.3)

    # ---- the overlap limits; pairs whose IoU IS the limit (not suppressed) next to pairs just beyond it ----
    base = _random_records(2300, G276, 150, sizes, n_clusters=10)
    for ov in (0.0, 0.3, 0.6, 1.0):
        _case("limit-%g" % ov, _settle(base, ov), G276, ov)
    recs = []
    for k in range(6):          # w x h = 20 x 20, 12 rows apart: 160 / 640 = 1/4; 11 rows: 180 / 620
        recs += [[0, 30 + 70 * k, 20, 20, 20, 0.9], [0, 30 + 70 * k, 32, 20, 20, 0.8 - 0.01 * k],
                 [1, 30 + 70 * k, 120, 20, 20, 0.9], [1, 30 + 70 * k, 131, 20, 20, 0.8 - 0.01 * k],
                 [2, 30 + 70 * k, 220 + k, 20, 20, 0.9], [2, 42 + 70 * k, 220 + k, 20, 20, 0.8]]        # 12 columns: 1/4 as well
    assert iou(mk(recs)[0], mk(recs)[1]) == Fraction(1, 4)
    _case("limit-0.25-exact", recs, G276, 0.25)
    recs = []
    for k in range(6):          # w x h = 32 x 24, 8 rows apart: 512 / 1024 = 1/2; 7 rows: 544 / 992
        recs += [[0, 30 + 70 * k, 20, 32, 24, 0.9], [0, 30 + 70 * k, 28, 32, 24, 0.8 - 0.01 * k],
                 [1, 30 + 70 * k, 120, 32, 24, 0.9], [1, 30 + 70 * k, 127, 32, 24, 0.8 - 0.01 * k]]
    assert iou(mk(recs)[0], mk(recs)[1]) == Fraction(1, 2)
    _case("limit-0.5-exact", recs, (300, 640, 32), 0.5)

    # ---- seeded random lists, clustered, spread over the geometries ----
    geoms = [g for g, _ in GEOMETRIES.values()]
    limits = (0.3, 0.0, 0.6, 0.5, 0.25, 1.0, 0.3, 0.45)
    for seed in range(240):
        geom = geoms[seed % len(geoms)]
        ms = geom[2]
        szs = [(ms, ms), (max(ms * 3 // 4, 5), max(ms // 2, 5)), (max(ms // 3, 4), ms), (8, 8)]
        n = (20, 45, 70, 110)[seed % 4] if seed % 40 else 700
        ov = limits[(seed // 3) % len(limits)]
        asc = seed % 5 == 3
        hits = _random_records(3000 + seed, geom, n, szs, tie_step=(0, 16, 0, 64)[(seed // 2) % 4])
        if asc:
            hits["score"] = np.float32(1.0) - hits["score"]
        hits = _settle(hits, ov)
        _case("random-%03d" % seed, hits, geom, ov, ascending=asc, score_threshold=0.5,
              n_max=(256 if n <= 110 and seed % 7 == 0 else 1 << 18))


    # ... and one long list on the largest grid
    geom = GEOMETRIES["cells3000"][0]
    _case("random-long", _settle(_random_records(4000, geom, 2000, [(32, 32), (24, 32), (30, 20), (8, 8)], n_clusters=60), 0.3), geom, 0.3)


_build()
CASE_BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """the reference's sets for a case of the table, computed once per process"""
    c = CASE_BY_NAME[name]
    return reference(c.hits, c.score_threshold, c.ascending, c.max_overlap)
