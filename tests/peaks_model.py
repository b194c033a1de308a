"""
A plain reference of the peak pass (csrc/mtm_k_peaks.hip.h) and the table of constructed score maps that
tests/test_gpu_peaks.py runs through Context.debug_peak_pass; tests/test_peaks_model_cpu.py validates both on the CPU.

The model is numpy on float32 arrays, without tiling.  Its rules:
  quality   q = -map for minima (mode_min), else map
  peak      q == max(q over the 3x3 neighbourhood; outside the map 0 under the constant border, -inf under the nearest one)
            and q > thr_q (strict); thr_q = -thr for minima
  record    (map index, x, y, w, h, the map's own value - bits and all, the sign of a zero included)
  NaN       never a peak; ignored as a neighbour; makes its map nontrivial
  trivial   every pixel equals its local maximum
  batch     image b of a stack owns map rows b * img_rows .. b * img_rows + img_rows - h; the rows between belong to no image
            and lie outside every image's map
  segments  only pixels of flagged (row, 256-column) segments are examined; under `holes` an unflagged segment reads as
            "below everything" (-inf in quality) for its neighbours
  extremum  first index in row-major order of the maximum and of the minimum over the non-NaN pixels, -0 == +0

Every case is built in QUALITY space (what is placed where is the same for maxima and minima) and negated exactly for
minima.  The table is built once at import from a fixed seed; expectations are computed on demand and cached.
"""
import collections
import functools

import numpy as np

HIT_DTYPE = np.dtype([("templ_idx", "<i4"), ("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4"), ("score", "<f4")])
SCAN, SCAN_BATCH, SEGMENTS, VERIFY_MAPS, VERIFY_HASH, EXTREMUM, EXTREMUM_BATCH = range(7)
ROUTE_NAMES = ("scan", "batch", "segments", "verify-maps", "verify-hash", "extremum", "extremum-batch")
BORDER_CONSTANT, BORDER_NEAREST = 0, 1
STRIP_COLS = 256            # a (row, strip column) segment: the unit of the flags
F32 = np.float32
NINF = F32(-np.inf)


# ---- the model ---------------------------------------------------------------------------------------------------------------
def quality(m, mode_min):
    m = np.asarray(m, dtype=F32)
    return -m if mode_min else m


def local_max(q, border):
    """max over the 3x3 neighbourhood of every pixel, NaN ignored (NaN only where all nine are NaN)"""
    H, W = q.shape
    p = np.full((H + 2, W + 2), F32(0.0) if border == BORDER_CONSTANT else NINF, dtype=F32)
    p[1:-1, 1:-1] = q
    out = p[1:-1, 1:-1].copy()
    for dy in range(3):
        for dx in range(3):
            out = np.fmax(out, p[dy:dy + H, dx:dx + W])
    return out


def is_local_max(q, border):
    with np.errstate(invalid="ignore"):
        return q == local_max(q, border)


def records(t, ys, xs, m, hw):
    r = np.zeros(len(ys), dtype=HIT_DTYPE)
    r["templ_idx"], r["x"], r["y"], r["w"], r["h"] = t, xs, ys, hw[1], hw[0]
    r["score"] = np.asarray(m, dtype=F32)[ys, xs]
    return r


def map_peaks(m, thr_q, mode_min, border, t=0, hw=(1, 1), y_off=0, whole=None):
    """-> (records, nontrivial) of one map (`whole`: the stack the map is a slice of; y_off its first row there)"""
    q = quality(m, mode_min)
    eq = is_local_max(q, border)
    with np.errstate(invalid="ignore"):
        ys, xs = np.nonzero(eq & (q > F32(thr_q)))
    r = records(t, ys, xs, m, hw)
    r["y"] += y_off
    return r, bool((~eq).any())


def batch_peaks(m, img_rows, thr_q, mode_min, border, t, hw):
    """-> (records in stack rows, [nontrivial per image])"""
    h = hw[0]
    n_img = (m.shape[0] + h - 1) // img_rows
    recs, nontriv = [], []
    for b in range(n_img):
        r, nt = map_peaks(m[b * img_rows:b * img_rows + img_rows - h + 1], thr_q, mode_min, border, t, hw, y_off=b * img_rows)
        recs.append(r)
        nontriv.append(nt)
    return np.concatenate(recs), nontriv


def n_strip_cols(ow):
    return (ow + STRIP_COLS - 1) // STRIP_COLS


def pixel_flags(flags_t, oh, ow):
    """the (row, strip column) flags of one map as a boolean per pixel"""
    return np.repeat(np.asarray(flags_t[:oh, :n_strip_cols(ow)]) != 0, STRIP_COLS, axis=1)[:, :ow]


def segment_peaks(m, flags_t, holes, thr_q, mode_min, border, t=0, hw=(1, 1)):
    """-> (records, (byte 0, byte 1, byte 2))"""
    q = quality(m, mode_min).copy()
    oh, ow = q.shape
    on = pixel_flags(flags_t, oh, ow)
    if holes:
        q[~on] = NINF
    eq = is_local_max(q, border)
    with np.errstate(invalid="ignore"):
        ys, xs = np.nonzero(on & eq & (q > F32(thr_q)))
    seg = np.asarray(flags_t[:oh, :n_strip_cols(ow)]) != 0
    return records(t, ys, xs, m, hw), (int((on & ~eq).any()), int(seg.any()), int((~seg).any()))


def necessary_flags(q, thr_q):
    """the segments that hold a pixel above the threshold"""
    oh, ow = q.shape
    with np.errstate(invalid="ignore"):
        above = q > F32(thr_q)
    pad = np.zeros((oh, n_strip_cols(ow) * STRIP_COLS), dtype=bool)
    pad[:, :ow] = above
    return pad.reshape(oh, -1, STRIP_COLS).any(axis=2).astype(np.uint8)


def verify_peaks(maps, cands, n_judged, by_hash, thr_q, mode_min, border):
    """the first n_judged records of the list, judged against the maps (by_hash: against the list alone - a neighbour that
    is not among the judged records is below everything) -> (the records kept, in list order; peaks per map)"""
    keep = np.zeros(n_judged, dtype=bool)
    tcount = np.zeros(len(maps), dtype=np.int64)
    c = cands[:n_judged]
    for t, m in enumerate(maps):
        sel = np.nonzero(c["templ_idx"] == t)[0]
        if not len(sel):
            continue
        q = quality(m, mode_min)
        if by_hash:
            ql = np.full(q.shape, NINF, dtype=F32)
            ql[c["y"][sel], c["x"][sel]] = quality(c["score"][sel], mode_min)
            q = ql
        own = quality(c["score"][sel], mode_min)
        lm = np.fmax(local_max(q, border)[c["y"][sel], c["x"][sel]], own)
        with np.errstate(invalid="ignore"):
            ok = (own == lm) & (own > F32(thr_q))
        keep[sel] = ok
        tcount[t] = int(ok.sum())
    return c[keep], tcount


def float_order(v):
    """the order-preserving image of a float32 as the extremum keys carry it (-0 folded to +0)"""
    b = int(np.array(v + F32(0.0) if v == 0 else v, dtype=F32).view(np.uint32))
    return (~b) & 0xFFFFFFFF if b & 0x80000000 else b | 0x80000000


def extremum(m):
    """-> ((index, value) of the maximum, (index, value) of the minimum), None where every pixel is NaN"""
    flat = np.asarray(m, dtype=F32).ravel()
    ok = ~np.isnan(flat)
    if not ok.any():
        return None, None
    hi, lo = flat[ok].max(), flat[ok].min()
    with np.errstate(invalid="ignore"):
        return (int(np.nonzero(flat == hi)[0][0]), flat[np.nonzero(flat == hi)[0][0]]), \
               (int(np.nonzero(flat == lo)[0][0]), flat[np.nonzero(flat == lo)[0][0]])


def extremum_keys(m):
    """the (max, min) key pair: order(v) << 32 | ~index, the minimum's order complemented; 0 = no pixel"""
    a, b = extremum(m)
    if a is None:
        return 0, 0
    return (float_order(a[1]) << 32) | (0xFFFFFFFF - a[0]), ((~float_order(b[1]) & 0xFFFFFFFF) << 32) | (0xFFFFFFFF - b[0])


# the candidate table's hash, restated: used ONLY to choose candidate positions that collide, never for an expectation
def cand_key(t, y, x):
    return ((np.asarray(t, dtype=np.uint64) + np.uint64(1)) << np.uint64(42)) | (np.asarray(y, dtype=np.uint64) << np.uint64(21)) | \
        np.asarray(x, dtype=np.uint64)


def cand_slot(k, mask):
    with np.errstate(over="ignore"):
        return ((np.asarray(k, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(32)) & np.uint64(mask)


def hash_slots(cand_cap):
    n = 1024
    while n < 2 * cand_cap:
        n <<= 1
    return n


def probe_lengths(cands, n_slots):
    """linear probing of the records' keys into a table of n_slots -> (longest run of probes of an insertion, insertions
    that wrapped past the table's end, keys whose first slot is one of the last three)"""
    keys = cand_key(cands["templ_idx"], cands["y"], cands["x"])
    start = cand_slot(keys, n_slots - 1).astype(np.int64)
    table = {}
    longest = wrapped = 0
    for k, s in zip(keys.tolist(), start.tolist()):
        n, s0 = 1, s
        while s in table and table[s] != k:
            s = (s + 1) % n_slots
            n += 1
        table[s] = k
        longest = max(longest, n)
        wrapped += s < s0
    return longest, wrapped, int((start >= n_slots - 3).sum())


# ---- the table ---------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name route qmaps hw thr_q mode_min border hit_cap img_rows flags holes cands cand_count "
                                      "cand_cap tags group")
CASES = []
_rng = np.random.default_rng(20261018)

OWS = [2, 3, 4, 5, 7, 8, 252, 253, 254, 255, 256, 257, 258, 259, 260, 511, 512, 513]
OHS = [2, 3, 7, 8, 9, 31, 32, 33, 127, 128, 129, 130]
# a sparse product: every width and every height, the largest map 513 x 130
SIZES = [(OHS[(5 * i) % len(OHS)], ow) for i, ow in enumerate(OWS)] + [(oh, OWS[(7 * i + 3) % len(OWS)]) for i, oh in enumerate(OHS)] + \
        [(130, 513), (2, 2), (128, 512), (33, 257)]
MODES = [(mm, bd) for mm in (False, True) for bd in (BORDER_NEAREST, BORDER_CONSTANT)]


def _bg(oh, ow, lo=0.0, hi=0.375):
    """a background below 0.5 in steps of 1/64: local maxima and ties everywhere, none above the usual threshold"""
    return (_rng.integers(int(lo * 64), int(hi * 64) + 1, size=(oh, ow)) / 64.0).astype(F32)


def _flat(oh, ow, v=0.25):
    return np.full((oh, ow), v, dtype=F32)


def maps_of(c):
    """the maps as the device gets them (the quality negated exactly for minima)"""
    return [(-q if c.mode_min else q) for q in c.qmaps]


def thr_of(c):
    return F32(-c.thr_q) if c.mode_min else F32(c.thr_q)


def _all_candidates(qmaps, thr_list, mode_min, hws):
    """every pixel whose quality exceeds thr_list, shuffled"""
    parts = []
    for t, q in enumerate(qmaps):
        with np.errstate(invalid="ignore"):
            ys, xs = np.nonzero(q > F32(thr_list))
        parts.append(records(t, ys, xs, -q if mode_min else q, hws[t]))
    c = np.concatenate(parts) if parts else np.zeros(0, dtype=HIT_DTYPE)
    return c[_rng.permutation(len(c))]


def _flag_sets(qmaps, thr_q):
    """necessary flags, all flags, necessary + random extra ones - [n][max oh][max strip columns]"""
    n, moh, msx = len(qmaps), max(q.shape[0] for q in qmaps), max(n_strip_cols(q.shape[1]) for q in qmaps)
    need = np.zeros((n, moh, msx), dtype=np.uint8)
    for t, q in enumerate(qmaps):
        f = necessary_flags(q, thr_q)
        need[t, :f.shape[0], :f.shape[1]] = f
    extra = need | (_rng.random(need.shape) < 0.3).astype(np.uint8)
    return (("need", need), ("all", np.ones_like(need)), ("extra", extra))


def add(name, route, qmaps, thr_q, mode_min, border, hw=None, hit_cap=None, img_rows=0, flags=None, holes=False, cands=None,
        cand_count=None, cand_cap=None, tags=(), group=None):
    qmaps = [np.ascontiguousarray(q, dtype=F32) for q in qmaps]
    hw = [(1, 1)] * len(qmaps) if hw is None else list(hw)
    if hit_cap is None:
        hit_cap = 2048
    CASES.append(Case("%s-%s-%s-%s" % (name, ROUTE_NAMES[route], "min" if mode_min else "max", "const" if border == 0 else "near"),
                      route, qmaps, hw, F32(thr_q), bool(mode_min), border, int(hit_cap), int(img_rows), flags, bool(holes), cands,
                      cand_count, cand_cap, tuple(tags), group or name))


def add_content(name, qmaps, thr_q, modes=MODES, routes=(SCAN, SEGMENTS, VERIFY_MAPS, VERIFY_HASH), hit_cap=None, list_margin=0.0,
                flag_sets=("need", "all", "extra"), tags=()):
    """one placed content through the scan, the flagged-segment scan (both hole settings, three flag sets) and the two
    verifiers (the candidate list: every pixel above the threshold, shuffled), maxima and minima, both borders"""
    hws = [(3 + t % 5, 2 + t % 7) for t in range(len(qmaps))]
    with np.errstate(invalid="ignore"):
        above = [int((q > F32(thr_q) - F32(list_margin)).sum()) for q in qmaps]
    cap = hit_cap if hit_cap is not None else max(2048, sum(above) + 8)
    for mode_min, border in modes:
        if SCAN in routes:
            add(name, SCAN, qmaps, thr_q, mode_min, border, hw=hws, hit_cap=cap, tags=tags, group=name)
        if SEGMENTS in routes:
            for fname, fl in _flag_sets(qmaps, thr_q):
                if fname not in flag_sets:
                    continue
                for holes in (False, True):
                    # (8 x the largest list: no region overflows unless the case is about that)
                    add("%s-%s-holes%d" % (name, fname, holes), SEGMENTS, qmaps, thr_q, mode_min, border, hw=hws,
                        hit_cap=max(cap, 8 * max(above)), flags=fl, holes=holes, tags=tags, group=name)
        for route in (VERIFY_MAPS, VERIFY_HASH):
            if route in routes:
                cands = _all_candidates(qmaps, F32(thr_q) - F32(list_margin), mode_min, hws)
                add(name, route, qmaps, thr_q, mode_min, border, hw=hws, hit_cap=cap, cands=cands, cand_count=len(cands),
                    cand_cap=max(len(cands), 1), tags=tags, group=name)


def _put(q, y, x, v):
    q[y, x] = F32(v)
    return q


# -- geometry: random quantised maps with peaks in the corners, the last row and the last column, lists of 1, 2 and 33 maps of
#    mixed sizes (the smaller maps leave whole waves idle beside the largest)
def _geo_map(oh, ow):
    q = _bg(oh, ow)
    for y, x in ((0, 0), (0, ow - 1), (oh - 1, 0), (oh - 1, ow - 1), (oh - 1, ow // 2), (oh // 2, ow - 1)):
        q[y, x] = F32(0.625 + _rng.integers(0, 16) / 64.0)
    for _ in range(max(1, oh * ow // 600)):
        q[_rng.integers(0, oh), _rng.integers(0, ow)] = F32(0.5 + _rng.integers(1, 32) / 64.0)
    return q


_geo = [_geo_map(oh, ow) for oh, ow in SIZES]
add_content("geo-33maps", _geo[:33], 0.5, tags=("idle-waves",))
add_content("geo-2maps", [_geo[30], _geo[3]], 0.5, tags=("idle-waves",))
for _i in (0, 11, 17, 29, 30, 32, 33):
    add_content("geo-1map-%d-%dx%d" % ((_i,) + SIZES[_i][::-1]), [_geo[_i]], 0.5, flag_sets=("need", "extra"))

# -- single peaks on the seams of the strips (columns 255 | 256, 511 | 512; rows 31 | 32, 127 | 128, and 7 | 8 for the 8-row
#    strips of the flagged-segment scan), then a second pixel - equal, then greater - in each of the 8 neighbour positions
SEAM_POINTS_SMALL = [(31, 255), (32, 256), (33, 257), (7, 255), (8, 256), (32, 255), (31, 256)]        # in 260 x 40 maps
SEAM_POINTS_LARGE = [(127, 511), (128, 512), (127, 512), (128, 255), (127, 256)]                     # in 513 x 130 maps
NEIGHBOURS = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]
for _pts, (_oh, _ow), _nm in ((SEAM_POINTS_SMALL, (40, 260), "small"), (SEAM_POINTS_LARGE, (130, 513), "large")):
    _single = [_put(_bg(_oh, _ow), y, x, 0.75) for y, x in _pts]
    add_content("seam-single-" + _nm, _single + [_geo[3]], 0.5, flag_sets=("need", "extra"), tags=("idle-waves",))
    for _k, (y, x) in enumerate(_pts):
        _pair = []
        for dy, dx in NEIGHBOURS:
            if not (0 <= y + dy < _oh and 0 <= x + dx < _ow):
                continue
            for v2 in (0.75, 0.875):
                _pair.append(_put(_put(_bg(_oh, _ow), y, x, 0.75), y + dy, x + dx, v2))
        add_content("seam-pair-%s-%d_%d" % (_nm, y, x), _pair, 0.5, flag_sets=("need",))

# -- plateaus of 2 x 2, 1 x 5 and 5 x 1 across a column seam, a row seam and both; one greater pixel touching from each side
_plateaus = []
for (py, px) in ((10, 255), (31, 100), (31, 255), (7, 254)):
    for ph, pw in ((2, 2), (1, 5), (5, 1)):
        y0, x0 = py - (ph - 1) // 2, px - (pw - 1) // 2
        for touch in (None, (y0 - 1, x0), (y0 + ph, x0 + pw - 1), (y0, x0 - 1), (y0 + ph - 1, x0 + pw)):
            q = _bg(40, 260)
            q[y0:y0 + ph, x0:x0 + pw] = F32(0.75)
            if touch is not None:
                q[touch] = F32(0.8125)
            _plateaus.append(q)
add_content("plateau-a", _plateaus[:30], 0.5, flag_sets=("need",))
add_content("plateau-b", _plateaus[30:], 0.5, flag_sets=("need", "extra"))

# -- qualities below zero at the border: no peaks under the constant border (the pad is 0), peaks under the nearest one
_neg = []
for oh, ow in ((2, 2), (3, 5), (9, 257), (33, 8), (8, 256)):
    q = (-0.5 - _bg(oh, ow)).astype(F32)
    for y, x in ((0, 0), (0, ow - 1), (oh - 1, 0), (oh - 1, ow - 1), (oh // 2, ow - 1), (oh - 1, ow // 2), (oh // 2, ow // 2)):
        q[y, x] = F32(-0.125)
    _neg.append(q)
add_content("negative-border", _neg, -1.0)

# -- thresholds exactly at a pixel's value (no hit) and one float32 below it (a hit); a negative threshold: every pixel passes
_thr_map = _put(_put(_bg(34, 258), 32, 255, 0.75), 5, 5, 0.625)
for _nm, _thr in (("at", F32(0.75)), ("below", np.nextafter(F32(0.75), F32(0))), ("at-lower", F32(0.625)),
                  ("below-lower", np.nextafter(F32(0.625), F32(0)))):
    add_content("threshold-" + _nm, [_thr_map, _geo[2]], _thr, flag_sets=("need", "all"))
add_content("threshold-negative", [_bg(9, 258, -0.5, 0.5), _bg(33, 7, -0.5, 0.5), _bg(2, 3, -0.5, 0.5)], -1.0, flag_sets=("need",))

# -- trivial and nearly trivial maps
_triv = [_flat(8, 257, 0.75), _flat(2, 2, 0.75), _flat(33, 256, 0.25),
         _put(_flat(9, 258, 0.75), 4, 255, 0.5),              # every pixel equals its local maximum except one
         _put(_flat(32, 255, 0.75), 31, 254, 0.875),          # exactly one pixel differs (its neighbours are below it)
         _put(_flat(3, 4, 0.75), 0, 0, 0.5), _put(_flat(130, 5, 0.25), 129, 4, 0.75)]
add_content("trivial", _triv, 0.5, tags=("trivial",))
add_content("trivial-all-pass", _triv[:6], -1.0, tags=("trivial", "every-pixel-a-peak"))

# -- NaN alone, next to a peak, a NaN row, an all-NaN map; +inf and -inf; -0 / +0 plateaus at the constant border's 0
_nan = [_put(_flat(8, 257, 0.75), 3, 255, np.nan),
        _put(_put(_bg(33, 258), 31, 256, 0.75), 31, 255, np.nan),
        _put(_put(_put(_bg(9, 260), 4, 256, 0.75), 3, 255, np.nan), 5, 257, np.nan),
        np.full((7, 5), np.nan, dtype=F32), _geo[1].copy(), _bg(40, 257)]
_nan[4][1, :] = np.nan
_nan[5][7, :] = np.nan
_nan[5][8, 100] = F32(0.875)
_nan[5][6, 256] = F32(0.875)
add_content("nan", _nan, 0.5, tags=("nan",))
add_content("nan-all-pass", _nan, -1.0, flag_sets=("need",), tags=("nan",))
_inf = [_put(_put(_bg(9, 258), 4, 255, np.inf), 4, 256, np.inf), _put(_bg(33, 7), 32, 6, -np.inf), np.full((3, 4), -np.inf, dtype=F32),
        _put(_put(np.full((8, 256), -np.inf, dtype=F32), 0, 0, 0.75), 7, 255, -0.25), np.full((2, 5), np.inf, dtype=F32)]
add_content("inf", _inf, 0.5)
add_content("inf-all-pass", _inf, -1.0, flag_sets=("need",))
_zero = []
for oh, ow in ((3, 5), (9, 257), (8, 256)):
    q = _flat(oh, ow, -0.5)
    q[0, :3] = [0.0, -0.0, 0.0]
    q[oh - 1, ow - 2:] = [-0.0, 0.0]
    q[oh // 2, 0] = -0.0
    q[oh // 2, ow - 1] = -0.0
    _zero.append(q)
add_content("signed-zero", _zero, -0.25)

# -- hit_cap below the number of peaks: the count stays exact, the records kept are peaks, none twice
_many = [_geo[30].copy(), _geo[3].copy()]
_many[0][::2, ::2] = F32(0.75)
add_content("hit-cap-below", _many, 0.5, routes=(SCAN, VERIFY_MAPS, VERIFY_HASH), hit_cap=100, modes=MODES[:2], tags=("hit-cap-below",))

# -- the flagged-segment scan: flags around a strip-column seam with a peak at column 255 and at 256
for _x in (255, 256):
    q = _put(_put(_put(_bg(24, 300, 0.0, 0.25), 10, _x, 0.75), 10, 511 - _x, 0.4375), 9 if _x == 255 else 11, 511 - _x, 0.46875)
    need = necessary_flags(q, 0.5)
    _other = 1 - _x // 256
    for nb_strip in (0, 1):
        for rows_on in (0, 1):
            fl = need.copy()
            fl[10, _other] = nb_strip
            fl[9, :] |= rows_on
            fl[11, :] |= rows_on
            fl[9, _other] = fl[11, _other] = nb_strip & rows_on
            for holes in (False, True):
                for mode_min, border in MODES:
                    add("seam-flags-x%d-nb%d-rows%d-holes%d" % (_x, nb_strip, rows_on, holes), SEGMENTS, [q], 0.5, mode_min, border,
                        hw=[(4, 6)], hit_cap=65536, flags=fl[None], holes=holes, group="seam-flags-x%d" % _x)
# ... and a peak below zero beside an unflagged segment: "below", not the pad value
_qn = _flat(16, 513, -2.0)
_qn[4, 250:256] = F32(-0.5)
_qn[4, 255] = F32(-0.25)
_qn[12, 256] = F32(-0.25)
_qn[12, 511] = F32(-0.25)
for holes in (False, True):
    for mode_min, border in MODES:
        add("negative-beside-hole-holes%d" % holes, SEGMENTS, [_qn], -1.0, mode_min, border, hw=[(2, 2)], hit_cap=65536,
            flags=necessary_flags(_qn, -1.0)[None], holes=holes, group="negative-beside-hole")

# -- the staging buffer: rows with 1, 63, 64, 65, 128 and 256 peaks; row sums of exactly 64 and of 65 before a flush; a direct
#    row (more than 64 peaks) behind a partly filled stage.  One 8-row strip per sequence, the rows two apart.
STAGE_SEQUENCES = [[1], [63], [64], [65], [128], [256], [63, 1, 1], [64, 1], [32, 32, 1], [30, 128, 5], [20, 65, 3], [1, 256, 64], [33, 32, 2], [40, 24, 1, 63]]


def _stage_map():
    q = _flat(8 * len(STAGE_SEQUENCES), 260, 0.25)
    for s, seq in enumerate(STAGE_SEQUENCES):
        for k, cnt in enumerate(seq):
            y = 8 * s + 2 * k
            if cnt == 256:
                q[y, :256] = F32(0.75)                        # a one-row plateau
            else:
                xs = np.sort(_rng.permutation(128)[:cnt]) * 2 if cnt < 128 else np.arange(128) * 2
                q[y, xs] = (0.625 + _rng.integers(0, 8, size=cnt) / 64.0).astype(F32)
        q[8 * s + 1, 257 + s % 3] = F32(0.75)                 # (the second strip column: a short list)
    return q


_stage = _stage_map()
for holes in (False, True):
    for mode_min, border in MODES:
        for fname, fl in _flag_sets([_stage, _geo[5]], 0.5)[:2]:
            add("stage-%s-holes%d" % (fname, holes), SEGMENTS, [_stage, _geo[5]], 0.5, mode_min, border, hw=[(3, 3), (2, 9)],
                hit_cap=65536, flags=fl, holes=holes, tags=("stage",), group="stage")
add("stage", SCAN, [_stage, _geo[5]], 0.5, False, BORDER_NEAREST, hw=[(3, 3), (2, 9)], hit_cap=65536)

# -- region overflow: more peaks in one (map, strip column) list than it holds, short lists beside it
_over = [_flat(130, 260, 0.25), _geo[8].copy()]
_over[0][::2, 0:256:2] = (0.625 + _rng.integers(0, 8, size=(65, 128)) / 64.0).astype(F32)
_over[0][5, 258] = F32(0.75)
for holes in (False, True):
    for mode_min, border in MODES[:2]:
        add("region-overflow-holes%d" % holes, SEGMENTS, _over, 0.5, mode_min, border, hw=[(3, 3), (5, 4)], hit_cap=2048,
            flags=_flag_sets(_over, 0.5)[0][1], holes=holes, tags=("region-overflow",), group="region-overflow")
        add("region-overflow-holes%d" % holes, SCAN, _over, 0.5, mode_min, border, hw=[(3, 3), (5, 4)], hit_cap=16384,
            tags=("region-overflow-scan",), group="region-overflow")

# -- the verifiers: list lengths around the work-group size and the capacity, a count beyond the capacity, a list with a margin
VERIFY_CAP = 300


def _verify_len_case(n_list):
    q = _bg(40, 70)
    pos = _rng.permutation(q.size)[:n_list]
    q.ravel()[pos] = (0.5 + _rng.integers(1, 32, size=n_list) / 64.0).astype(F32)
    return q


for _n in (0, 1, 255, 256, 257, VERIFY_CAP - 1, VERIFY_CAP, VERIFY_CAP + 5):
    for route in (VERIFY_MAPS, VERIFY_HASH):
        for mode_min, border in MODES[:2] if _n not in (0, VERIFY_CAP + 5) else MODES:
            q = _verify_len_case(_n)
            cands = _all_candidates([q], 0.5, mode_min, [(2, 3)])
            add("verify-len%d" % _n, route, [q], 0.5, mode_min, border, hw=[(2, 3)], hit_cap=4096, cands=cands, cand_count=_n,
                cand_cap=VERIFY_CAP, tags=("beyond-cand-cap",) if _n > VERIFY_CAP else ("list-at-cap",) if _n == VERIFY_CAP else (), group="verify-len")
add_content("verify-margin", [_geo[30], _geo[9], _plateaus[7]], 0.5, routes=(VERIFY_MAPS, VERIFY_HASH), list_margin=0.1875, tags=("margin",))

# -- the hash table: 40 + keys whose probing starts in the table's last three slots (it wraps), one probe chain longer than 64,
#    map indices 0 and 32, positions up to (512, 129)
HASH_CAND_CAP = 512


def _hash_case():
    n_slots = hash_slots(HASH_CAND_CAP)
    qmaps = [_flat(130, 513, 0.25) if t in (0, 32) else _flat(2 + t % 3, 2 + t % 5, 0.25) for t in range(33)]
    yy, xx = np.mgrid[0:130, 0:512]                     # (x + 1 <= 512 stays inside the map)
    chosen = []
    for t, want_slots, count in ((0, (n_slots - 1, n_slots - 2, n_slots - 3), 24), (32, (n_slots - 1, n_slots - 2, n_slots - 3), 24),
                                 (32, (517,), 40), (0, (517,), 35)):
        s = cand_slot(cand_key(t, yy, xx), n_slots - 1)
        ys, xs = np.nonzero(np.isin(s, np.array(want_slots, dtype=np.uint64)))
        pick = _rng.permutation(len(ys))[:count]
        chosen += [(t, int(ys[i]), int(xs[i])) for i in pick]
    for t, y, x in chosen:
        qmaps[t][y, x] = F32(0.625 + _rng.integers(0, 16) / 64.0)
        if qmaps[t][y, x + 1] == F32(0.25):             # a listed right neighbour, below, equal or above
            qmaps[t][y, x + 1] = F32(0.5625 + _rng.integers(0, 24) / 64.0)
    qmaps[32][129, 512] = F32(0.9375)
    qmaps[0][129, 511] = F32(0.9375)
    return qmaps


_hash_maps = _hash_case()
for route in (VERIFY_HASH, VERIFY_MAPS):
    for mode_min, border in MODES:
        hws = [(2, 2)] * 33
        cands = _all_candidates(_hash_maps, 0.5, mode_min, hws)
        add("hash-collisions", route, _hash_maps, 0.5, mode_min, border, hw=hws, hit_cap=HASH_CAND_CAP, cands=cands,
            cand_count=len(cands), cand_cap=HASH_CAND_CAP, tags=("hash-wrap",))

# -- every pixel a peak: tcount == oh * ow reads as trivial
for route in (VERIFY_MAPS, VERIFY_HASH):
    for mode_min, border in MODES:
        qm = [_flat(9, 33, 0.75), _put(_flat(8, 31, 0.75), 7, 30, 0.5)]
        cands = _all_candidates(qm, 0.5, mode_min, [(1, 1), (1, 1)])
        add("verify-trivial", route, qm, 0.5, mode_min, border, hit_cap=1024, cands=cands, cand_count=len(cands),
            cand_cap=max(1, len(cands)), tags=("every-pixel-a-peak",))

# -- stacks of images: seams inside a strip (img_rows 5, 31, 33), on a strip boundary (32) and on a work-group boundary (64: one
#    work-group is 128 rows); h = 2, 3 and img_rows - 1
BATCH_IMG_ROWS = [5, 31, 32, 33, 64]


def _batch_map(img_rows, h, n_img, ow, trivial_image=None):
    oh = n_img * img_rows - h + 1
    q = _bg(oh, ow)
    oh_b = img_rows - h + 1
    for b in range(n_img):
        y0, y1 = b * img_rows, b * img_rows + oh_b - 1
        if b == trivial_image:
            q[y0:y1 + 1] = F32(0.75)
        else:
            # peaks on the first and the last owned row, greater values on the seam rows above and below them
            xa, xb = 1 + (7 * b) % (ow - 2), 1 + (11 * b + 3) % (ow - 2)
            q[y0, xa] = F32(0.75)
            q[y1, xb] = F32(0.75)
            if y0 > 0:
                q[y0 - 1, max(xa - 1, 0):xa + 2] = F32(0.9375)
            if y1 + 1 < oh:
                q[y1 + 1, max(xb - 1, 0):xb + 2] = F32(0.9375)
        # the seam rows: greater than everything, never reported, never read as neighbours
        q[y1 + 1:y0 + img_rows] = np.maximum(q[y1 + 1:y0 + img_rows], F32(0.875))
    return q


for _ir in BATCH_IMG_ROWS:
    for _h in (2, 3, _ir - 1):
        n_img = 9 if _ir == 5 else 5
        qm = [_batch_map(_ir, _h, n_img, 258, trivial_image=2), _batch_map(_ir, _h, n_img, 7)]
        for mode_min, border in MODES:
            add("batch-rows%d-h%d" % (_ir, _h), SCAN_BATCH, qm, 0.5, mode_min, border, hw=[(_h, 4), (_h, 2)], hit_cap=16384,
                img_rows=_ir, tags=("batch",) + (("strip-spans-images",) if _ir == 5 else ()), group="batch-rows%d" % _ir)
            add("batch-rows%d-h%d" % (_ir, _h), EXTREMUM_BATCH, qm, 0.5, mode_min, border, hw=[(_h, 4), (_h, 2)], img_rows=_ir, group="batch-rows%d" % _ir)

# -- the global extremum: ties in different work-groups and waves of the launch, -0 against +0, NaN at the would-be extremum,
#    an all-NaN map, infinities, a difference in the last pixel only
_ext = []
q = _bg(130, 513, -0.375, 0.375)
for idx in (70, 300, 256 * 7 + 3, 256 * 256 + 5, 66000):           # (256 work-groups of 256 pixels per turn of the loop)
    q.ravel()[idx] = F32(0.75)
    q.ravel()[idx + 64] = F32(-0.75)
_ext.append(q)
_ext.append(_put(_flat(9, 258, 0.0), 0, 100, -0.0))            # zeros of both signs: index 0 wins both, whichever zero it is
_ext.append(_put(_flat(9, 258, -0.0), 3, 3, 0.0))
_ext.append(_put(_put(_put(_bg(33, 257), 5, 5, np.nan), 20, 256, 0.75), 20, 255, np.nan))
_ext.append(np.full((7, 5), np.nan, dtype=F32))
_ext.append(_put(_put(_bg(8, 256), 7, 255, np.inf), 0, 0, -np.inf))
_ext.append(_put(_flat(128, 512, 0.25), 127, 511, 0.25 + 2.0 ** -20))
_ext.append(_put(_flat(130, 513, 0.25), 129, 512, 0.25 - 2.0 ** -20))
_ext.append(_put(np.full((3, 4), np.nan, dtype=F32), 2, 3, -0.0))
add("extremum", EXTREMUM, _ext, 0.5, False, BORDER_NEAREST, tags=("extremum",))
add("extremum-1map", EXTREMUM, [_ext[0]], 0.5, False, BORDER_NEAREST)
add("extremum-geo", EXTREMUM, _geo[:33], 0.5, False, BORDER_NEAREST)
# stacks: the same tie in two images, the seam rows hold more extreme values
for _ir in BATCH_IMG_ROWS:
    _h = 3
    oh = 4 * _ir - _h + 1
    q = _bg(oh, 258, -0.375, 0.375)
    for b in range(4):
        y0 = b * _ir
        q[y0 + _ir - _h + 1:y0 + _ir] = F32(2.0) if b % 2 else F32(-2.0)
        if b in (1, 3):
            q[y0 + 1, [5, 200]] = F32(0.75)
            q[y0, [257, 100]] = F32(-0.75)
    add("extremum-stack-rows%d" % _ir, EXTREMUM_BATCH, [q, _batch_map(_ir, _h, 4, 5)], 0.5, False, BORDER_NEAREST,
        hw=[(_h, 2), (_h, 9)], img_rows=_ir, tags=("extremum-stack",), group="extremum-stack")

CASE_BY_NAME = {c.name: c for c in CASES}
GROUPS = collections.OrderedDict()
for _c in CASES:
    GROUPS.setdefault("%s-%s" % ("-".join(_c.group.split("-")[:2]), ROUTE_NAMES[_c.route]), []).append(_c)
assert len(CASE_BY_NAME) == len(CASES), [n for n, k in collections.Counter(c.name for c in CASES).items() if k > 1]


# ---- expectations ------------------------------------------------------------------------------------------------------------
Expect = collections.namedtuple("Expect", "records nontrivial bytes3 tcount keys ext")


@functools.lru_cache(maxsize=None)
def expect(name):
    """the model's answer for a case: every true peak (whatever the capacities), per-map / per-image nontrivial, the
    flagged scan's three bytes, the verifiers' counts, the extremum keys"""
    c = CASE_BY_NAME[name]
    maps = maps_of(c)
    if c.route == SCAN:
        out = [map_peaks(m, c.thr_q, c.mode_min, c.border, t, c.hw[t]) for t, m in enumerate(maps)]
        return Expect(np.concatenate([r for r, _ in out]), [nt for _, nt in out], None, None, None, None)
    if c.route == SCAN_BATCH:
        out = [batch_peaks(m, c.img_rows, c.thr_q, c.mode_min, c.border, t, c.hw[t]) for t, m in enumerate(maps)]
        return Expect(np.concatenate([r for r, _ in out]), np.array([nt for _, nt in out]).T, None, None, None, None)
    if c.route == SEGMENTS:
        out = [segment_peaks(m, c.flags[t], c.holes, c.thr_q, c.mode_min, c.border, t, c.hw[t]) for t, m in enumerate(maps)]
        return Expect(np.concatenate([r for r, _ in out]), None, [b for _, b in out], None, None, None)
    if c.route in (VERIFY_MAPS, VERIFY_HASH):
        n_judged = min(c.cand_count, c.cand_cap)
        kept, tcount = verify_peaks(maps, c.cands, n_judged, c.route == VERIFY_HASH, c.thr_q, c.mode_min, c.border)
        return Expect(kept, None, None, tcount, None, None)
    if c.route == EXTREMUM:
        return Expect(None, None, None, None, [extremum_keys(m) for m in maps], [extremum(m) for m in maps])
    n_img = (maps[0].shape[0] + c.hw[0][0] - 1) // c.img_rows
    sub = [[m[b * c.img_rows:b * c.img_rows + c.img_rows - c.hw[t][0] + 1] for t, m in enumerate(maps)] for b in range(n_img)]
    return Expect(None, None, None, None, [[extremum_keys(m) for m in row] for row in sub], [[extremum(m) for m in row] for row in sub])
