"""The tail screen of the two-row int8 score kernel as a plain model: the templates' tail constants (tail_consts_kernel,
TemplDev::tail_k / tail_d / tail_g), the bound a wave holds against the threshold after `split` K steps, and the wave's
decision to leave the K loop (csrc/mtm_mfma.hip.h).

Claims about exactness are made with Python integers and Fractions:

  consts_exact   K_P = 128 sum(T_P) - 16384 |P| (int), d = sum(T_Q) / |Q| - 128 and g^2 = sum_Q (T - mean(T_Q))^2 (Fractions);
                 P = template rows 0 .. q0 - 1 (accumulated), Q = rows q0 .. h - 1 (the tail); q0 = split for the wave's first
                 (even) output row, split - 1 for its second (odd) one.
  consts_f64     the kernel's float64 expressions in the kernel's order (Python floats are IEEE doubles, int -> float and
                 math.sqrt are correctly rounded): what the device must hold bit for bit if its operations are.
  check_consts   the inequalities any (k, d, g) has to obey against the exact values for the rigour argument to stand.
  rigour         Fraction(bound) >= exact numerator at every output of every 16-column block, from whatever constants and
                 block records it is handed (the model's or the device's); accumulators and numerators are exact integers.
  wave_pass      the decision as the kernel takes it.  Work item: 8 output rows x 256 columns x one group of 16 list
                 positions; wave: 2 rows; lane: one 16-column block (x four templates).  Row mb of a wave reads the block
                 records of row min(y, oh - 1), block min(b, blk_pitch - 1); the accumulators are those of the image as the
                 device planes hold it - zero pixels right of and below the image.  A wave leaves when nothing in it passes.

Template constants (mean, templ_norm, all_ones) come from _lib.debug_templ_stats (host code, no GPU), the block records from
stats_model.window_stats - or, in the GPU tests, from the device."""
import math
import zlib
from fractions import Fraction

import numpy as np

import stats_model

ITEM_ROWS, ITEM_COLS, GROUP, WAVE_ROWS, BLOCK = 8, 256, 16, 2, 16
WAVES = ITEM_ROWS // WAVE_ROWS
SLACK = 2.0 ** -46              # tail_consts_kernel: k = K_P + mag * 2^-46
ROUND_UP = 1.0 + 2.0 ** -49     # ... and g = sqrt(.) * (1 + 2^-49); stats_u8_kernel's sqrt(V_Q) likewise


# ---- the launch's numbers (csrc/mtm_launch.hip: wire_mfma_candidates, tail_split_for) -------------------------------------
def thr_lo(thr):
    t = float(np.float32(thr))
    return t - 1e-6 * max(1.0, abs(t))


def screen_hi(thr):
    return min(thr_lo(thr), 0.999999) - 1e-6


def sq_floor(h, w):
    return 0.99 / math.sqrt(float(w) * float(h))


def clamp_split(split, h):
    return max(6, min(int(split), h - 2))


def rule_split(lib, h, w, thr):
    """The split a call at `thr` carries (tail_split_rule through mtm_debug_tail_split; 0 = unscreened)."""
    return lib.debug_tail_split(h, w, thr_lo(thr))


def geometry(oh, ow, n):
    nyb, nseg, ntg = -(-oh // ITEM_ROWS), -(-ow // ITEM_COLS), -(-n // GROUP)
    return {"nyb": nyb, "nseg": nseg, "ntg": ntg, "oh_pad": nyb * ITEM_ROWS, "ow_pad": nseg * ITEM_COLS, "n_pad": ntg * GROUP,
            "waves": nyb * nseg * ntg * WAVES}


# ---- constants -------------------------------------------------------------------------------------------------------------
def _sums(T, q0):
    T = np.asarray(T)
    h, w = T.shape
    assert 1 <= q0 <= h - 1, (q0, h)
    t = T.astype(np.int64)                      # (sums of at most 2^13 bytes and their squares: far inside int64)
    return h, w, int(t.sum()), int(t[q0:].sum()), int((t[q0:] * t[q0:]).sum())


def consts_exact(T, q0):
    """-> (K_P int, d Fraction, g^2 Fraction)."""
    h, w, sall, sq, s2q = _sums(T, q0)
    nq = (h - q0) * w
    return 128 * (sall - sq) - 16384 * q0 * w, Fraction(sq, nq) - 128, Fraction(nq * s2q - sq * sq, nq)


def consts_brute(T, q0):
    """consts_exact by the definitions, pixel by pixel (the mean of Q first, then the squared distances from it)."""
    T = np.asarray(T)
    h, w = T.shape
    kp = 0
    for y in range(q0):
        for x in range(w):
            kp += 128 * int(T[y, x]) - 16384
    tail = [int(T[y, x]) for y in range(q0, h) for x in range(w)]
    tau = Fraction(sum(tail), len(tail))
    return kp, tau - 128, sum((v - tau) ** 2 for v in tail)


def consts_f64(T, q0, g=None):
    """(k, d, g) by tail_consts_kernel's expressions, in its order; g given: the slack restated from that g."""
    h, w, sall, sq, s2q = _sums(T, q0)
    nq, np_, n = (h - q0) * w, q0 * w, h * w
    kp = 128.0 * float(sall - sq) - 16384.0 * float(np_)
    d = float(sq) / float(nq) - 128.0
    gg = math.sqrt(float(nq * s2q - sq * sq) / float(nq)) * ROUND_UP if g is None else float(g)
    mag = 4294967296.0 + abs(kp) + 2.0 * 128.0 * 255.0 * float(n) + gg * 128.0 * math.sqrt(float(nq))
    return kp + mag * SLACK, d, gg


def mag_exact(T, q0):
    """The magnitude the slack is a 2^-46 of, from the exact values (a float: it is only held to a factor of two)."""
    h, w = np.asarray(T).shape
    kp, _, g2 = consts_exact(T, q0)
    return 2.0 ** 32 + abs(kp) + 65280.0 * h * w + 128.0 * math.sqrt(float(g2) * (h - q0) * w)


def check_consts(k, d, g, T, q0):
    """What is wrong with (k, d, g) as the constants of template T at first tail row q0: a list of strings, empty if nothing.
    k - K_P positive and within a factor of two of 2^-46 mag; d within the two roundings of its expression (2^-46 + 2^-47);
    g^2 >= the exact g^2 and g <= exact (1 + 2^-47), as Fractions."""
    kp, dx, g2 = consts_exact(T, q0)
    bad = []
    if not all(math.isfinite(v) for v in (k, d, g)):
        return ["not finite: %r" % ((k, d, g),)]
    slack, want = Fraction(k) - kp, Fraction(mag_exact(T, q0)) * Fraction(SLACK)
    if not slack > 0:
        bad.append("k - K_P = %.6g is not positive" % float(slack))
    elif not want / 2 <= slack <= want * 2:
        bad.append("k - K_P = %.6g, not within a factor of two of 2^-46 mag = %.6g" % (float(slack), float(want)))
    if abs(Fraction(d) - dx) > Fraction(3, 2 ** 47):
        bad.append("d = %r, exact %.17g" % (d, float(dx)))
    gf = Fraction(g)
    if g < 0 or gf * gf < g2:
        bad.append("g^2 below the exact one: g = %r, exact g = %.17g" % (g, math.sqrt(float(g2))))
    if gf * gf > g2 * Fraction(2 ** 47 + 1, 2 ** 47) ** 2:
        bad.append("g above exact (1 + 2^-47): g = %r, exact g = %.17g" % (g, math.sqrt(float(g2))))
    return bad


def table_f64(templates, split, mistake=None):
    """(n, 6) float64: k0, k1, d0, d1, g0, g1 per template at `split` by consts_f64 - or, with `mistake`, by one of the
    wrong derivations the checks have to be able to see."""
    n = len(templates)
    out = np.zeros((n, 6), dtype=np.float64)
    for li, T in enumerate(templates):
        h, w = np.asarray(T).shape
        for r, q0 in enumerate((split, split - 1)):
            if mistake is None:
                k, d, g = consts_f64(T, q0)
            elif mistake == "same_q0":              # both parities given q0 = split
                k, d, g = consts_f64(T, split)
            elif mistake == "q_short":              # |Q| short by one row (sums over Q as they are)
                _, _, sall, sq, s2q = _sums(T, q0)
                nq = (h - q0 - 1) * w
                kp = 128.0 * float(sall - sq) - 16384.0 * float(q0 * w)
                d = float(sq) / float(nq) - 128.0
                g = math.sqrt(max(float(nq * s2q - sq * sq), 0.0) / float(nq)) * ROUND_UP
                mag = 4294967296.0 + abs(kp) + 2.0 * 128.0 * 255.0 * float(h * w) + g * 128.0 * math.sqrt(float(nq))
                k = kp + mag * SLACK
            elif mistake == "no_slack":
                k, d, g = consts_f64(T, q0)
                k = float(consts_exact(T, q0)[0])
            elif mistake == "g_down":               # no round-up factor, g^2 rounded down
                _, _, g2 = consts_exact(T, q0)
                g2f = float(g2)
                if Fraction(g2f) > g2:
                    g2f = math.nextafter(g2f, -math.inf)
                g = math.sqrt(g2f)
                if Fraction(g) ** 2 > Fraction(g2f):
                    g = math.nextafter(g, -math.inf)
                k, d, _ = consts_f64(T, q0, g=g)
            elif mistake == "neighbour":            # K_P of the neighbouring list position
                k, d, g = consts_f64(T, q0)
                k = consts_f64(templates[(li + 1) % n], q0)[0]
            elif mistake == "stale":                # the constants of split + 7, left behind by another call
                k, d, g = consts_f64(T, q0 + 7)
            else:
                raise ValueError(mistake)
            out[li, r], out[li, 2 + r], out[li, 4 + r] = k, d, g
    return out


MISTAKES = ("same_q0", "q_short", "no_slack", "g_down", "neighbour", "stale")


def consts_violations(table, templates, split):
    """check_consts over a whole table -> [(list position, parity, what)]."""
    out = []
    for li, T in enumerate(templates):
        for r, q0 in enumerate((split, split - 1)):
            for what in check_consts(float(table[li, r]), float(table[li, 2 + r]), float(table[li, 4 + r]), T, q0):
                out.append((li, r, what))
    return out


# ---- exact sums ------------------------------------------------------------------------------------------------------------
def device_image(img, rows, cols):
    """The image as the device planes hold it: zero pixels right of and below it (0x80 in the int8 view)."""
    img = np.asarray(img)
    out = np.zeros((max(rows, img.shape[0]), max(cols, img.shape[1])), dtype=np.int64)
    out[:img.shape[0], :img.shape[1]] = img
    return out


def _row_products(a, y, nrows, ncols, w, tm):
    """sum over dy < nrows, dx < w of a[y + dy][x + dx] * tm[dy * w + dx][t] for x < ncols -> (ncols, n) exact integers.
    float64 matrix product of integers: every partial sum is an integer below 2^53, so any summation order is exact."""
    win = np.lib.stride_tricks.sliding_window_view(a[y:y + nrows, :ncols + w - 1], w, axis=1)        # (nrows, ncols, w)
    m = np.ascontiguousarray(win.transpose(1, 0, 2)).reshape(ncols, nrows * w).astype(np.float64)
    return np.rint(m @ tm[:nrows * w]).astype(np.int64)


def accumulators(img, templates, split, oh, ow):
    """The biased int8 accumulators after `split` K steps, (n, oh_pad, ow_pad) int64: output row y holds template rows
    0 .. split - 1 (y even) or 0 .. split - 2 (y odd) of sum (I - 128)(T - 128), over the padded image."""
    n = len(templates)
    h, w = np.asarray(templates[0]).shape
    g = geometry(oh, ow, n)
    a = device_image(img, g["oh_pad"] + h, g["ow_pad"] + w) - 128
    tm = np.stack([np.asarray(t, dtype=np.int64).reshape(-1) - 128 for t in templates], axis=1).astype(np.float64)
    acc = np.zeros((n, g["oh_pad"], g["ow_pad"]), dtype=np.int64)
    for y in range(g["oh_pad"]):
        acc[:, y, :] = _row_products(a, y, split - (y & 1), g["ow_pad"], w, tm).T
    assert int(np.abs(acc).max(initial=0)) < 2 ** 31
    return acc


def numerators(img, templates, method, stats):
    """-> (num_scaled (n, oh, ow) int64, scale (n,) int): the exact numerator times `scale` - TM_CCORR_NORMED (3): sum I T,
    scale 1; TM_CCOEFF_NORMED (5): sum I T - mean(T) S1 times w h."""
    n = len(templates)
    h, w = np.asarray(templates[0]).shape
    img = np.asarray(img)
    oh, ow = img.shape[0] - h + 1, img.shape[1] - w + 1
    a = img.astype(np.int64)
    tm = np.stack([np.asarray(t, dtype=np.int64).reshape(-1) for t in templates], axis=1).astype(np.float64)
    corr = np.zeros((n, oh, ow), dtype=np.int64)
    for y in range(oh):
        corr[:, y, :] = _row_products(a, y, h, ow, w, tm).T
    if method == 3:
        return corr, [1] * n
    s1 = stats["t0"][:, :ow].astype(np.int64)
    tsum = np.array([int(np.asarray(t, dtype=np.int64).sum()) for t in templates], dtype=np.int64)
    return corr * (h * w) - tsum[:, None, None] * s1[None], [h * w] * n


# ---- the bound and the decision --------------------------------------------------------------------------------------------
def templ_stats(lib, templates, method):
    """(n, 7) float64 of _lib.TEMPL_STATS_FIELDS (mean0 .. mean3, templ_norm, templ_sum2, all_ones): host code, no GPU."""
    return np.stack([lib.debug_templ_stats(np.ascontiguousarray(t, dtype=np.uint8), method) for t in templates])


def bounds(acc, consts, tstats, blk, blkq, method, thr, h, w, oh, ow):
    """Per (padded output row, 16-column block, padded list position): the kernel's bound, its right-hand side and its
    verdict.  -> dict(bound, rhs, lane_pass: (oh_pad, blocks, n_pad); amax likewise, int64)."""
    n = acc.shape[0]
    g = geometry(oh, ow, n)
    nb = g["ow_pad"] // BLOCK
    amax = acc.reshape(n, g["oh_pad"], nb, BLOCK).max(axis=3).transpose(1, 2, 0)                     # (oh_pad, nb, n)
    yr = np.minimum(np.arange(g["oh_pad"]), oh - 1)
    bj = np.minimum(np.arange(nb), blk.shape[1] - 1)
    rec, recq = blk[yr][:, bj], blkq[yr][:, bj]                                                       # (oh_pad, nb, 4)
    par = np.arange(g["oh_pad"]) & 1
    k, d, gq = consts[:, 0:2].T[par], consts[:, 2:4].T[par], consts[:, 4:6].T[par]                    # (oh_pad, n)
    m = (128.0 - tstats[:, 0]) if method == 5 else np.full(n, 128.0)
    s1lo, s1hi, sqmin = rec[..., 0, None], rec[..., 1, None], rec[..., 2, None]
    qlo, qhi, vq = recq[..., 0, None], recq[..., 1, None], recq[..., 2, None]
    with np.errstate(invalid="ignore", over="ignore"):
        bound = (((amax.astype(np.float64) + k[:, None, :]) + np.maximum(m * s1lo, m * s1hi)) +
                 np.maximum(d[:, None, :] * qlo, d[:, None, :] * qhi)) + vq * gq[:, None, :]
        rhs = (screen_hi(thr) * tstats[:, 4]) * np.maximum(sqmin, sq_floor(h, w))
        lane = (tstats[:, 6] != 0.0) | (bound > rhs)
    pad = g["n_pad"] - n                                # positions past the list never pass
    if pad:
        z = (g["oh_pad"], nb, pad)
        bound = np.concatenate([bound, np.full(z, -1e300)], axis=2)
        rhs = np.concatenate([rhs, np.full(z, np.inf)], axis=2)
        lane = np.concatenate([lane, np.zeros(z, dtype=bool)], axis=2)
        amax = np.concatenate([amax, np.zeros(z, dtype=np.int64)], axis=2)
    return {"bound": bound, "rhs": rhs, "lane_pass": lane, "amax": amax}


def wave_pass(acc, consts, tstats, blk, blkq, method, thr, h, w, oh, ow):
    """-> dict(stay: (nyb, nseg, ntg, 4 waves) bool - the wave goes on with its K loop -, waves, leaving)."""
    n = acc.shape[0]
    g = geometry(oh, ow, n)
    lane = bounds(acc, consts, tstats, blk, blkq, method, thr, h, w, oh, ow)["lane_pass"]
    v = lane.reshape(g["nyb"], WAVES, WAVE_ROWS, g["nseg"], ITEM_COLS // BLOCK, g["ntg"], GROUP)
    stay = v.any(axis=(2, 4, 6)).transpose(0, 2, 3, 1)                                                # (nyb, nseg, ntg, wave)
    return {"stay": stay, "waves": int(stay.size), "leaving": int(stay.size - stay.sum())}


def rigour(img, templates, method, thr, consts, tstats, stats, split, acc=None, nums=None):
    """Fraction(bound) >= exact numerator at every output of every block.  -> dict(violations: [(li, y, block, bound,
    numerator)], tightness: the smallest (bound - numerator) / (templ_norm sq) over outputs with templ_norm sq > 0, checked:
    the number of (row, block, template) bounds compared)."""
    n = len(templates)
    h, w = np.asarray(templates[0]).shape
    oh, ow = np.asarray(img).shape[0] - h + 1, np.asarray(img).shape[1] - w + 1
    acc = accumulators(img, templates, split, oh, ow) if acc is None else acc
    num, scale = numerators(img, templates, method, stats) if nums is None else nums
    b = bounds(acc, consts, tstats, stats["blk"], stats["blkq"], method, thr, h, w, oh, ow)["bound"]
    nb = -(-ow // BLOCK)
    full = np.full((n, oh, nb * BLOCK), np.iinfo(np.int64).min, dtype=np.int64)
    full[:, :, :ow] = num
    nmax = full.reshape(n, oh, nb, BLOCK).max(axis=3)
    viol, checked = [], 0
    for li in range(n):
        for y in range(oh):
            for blk_i in range(nb):
                p, q = float(b[y, blk_i, li]).as_integer_ratio() if math.isfinite(b[y, blk_i, li]) else (-1, 0)
                checked += 1
                if q == 0 or p * scale[li] < int(nmax[li, y, blk_i]) * q:
                    viol.append((li, y, blk_i, float(b[y, blk_i, li]), int(nmax[li, y, blk_i]) / scale[li]))
    sq = stats["sq"][:, :ow]
    tight = math.inf
    for li in range(n):
        den = tstats[li, 4] * sq
        bx = np.repeat(b[:oh, :nb, li], BLOCK, axis=1)[:, :ow]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (bx - num[li] / float(scale[li])) / den
        t = t[den > 0]
        if t.size:
            tight = min(tight, float(t.min()))
    return {"violations": viol, "tightness": tight, "checked": checked}


# ---- scenes ----------------------------------------------------------------------------------------------------------------
KINDS = ("noise", "zero", "sat", "const77", "flat_top", "checker", "last_pixel")


def make_template(kind, h, w, rng, sparse=False):
    t = rng.integers(0, 256, (h, w))
    if sparse:
        t = t * (rng.random((h, w)) < 1.0 / 3.0)
    if kind == "zero":
        t[:] = 0
    elif kind == "sat":
        t[:] = 255
    elif kind == "const77":
        t[:] = 77
    elif kind == "flat_top":
        t[:(2 * h) // 3] = 128                      # structure only in the last third of the rows
    elif kind == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        t = ((yy + xx) & 1) * 255
    elif kind == "last_pixel":
        t[:] = 0
        t[h - 1, int(rng.integers(0, w))] = int(rng.integers(1, 256))
    else:
        assert kind == "noise", kind
    return np.ascontiguousarray(t.astype(np.uint8))


def cell_kinds(n, which):
    """"counter": noise, but for one flat-topped template at list position 1 (the first group);  "all": every kind of KINDS in
    turn, rotated so that the positions past 16 start with another kind than position 0."""
    if which == "counter":
        return ["flat_top" if i == 1 else "noise" for i in range(n)]
    return [KINDS[(i + 3 * (i // GROUP)) % len(KINDS)] for i in range(n)]


def scene(cell):
    """cell: dict(h, w, n, method, map=(oh, ow), kinds="counter" | "all"[, seed, device]).  -> (image uint8, templates
    [uint8], kinds); a "device" cell's templates are the views of device_units.
    A noise image (TM_CCORR_NORMED: sparse noise, two thirds of the pixels zero - between windows of dense noise that score
    is 0.75 everywhere and the candidate list overflows), templates drawn independently of it, and three plants in disjoint
    columns: an exact copy of template 0, an exact copy of the last template, and the last third of the rows of the first
    flat-topped template (whose first two thirds are flat 128)."""
    h, w, n, method = cell["h"], cell["w"], cell["n"], cell["method"]
    oh, ow = cell["map"]
    rng = np.random.default_rng(zlib.crc32(("%d-%d-%d-%d-%d-%d-%d" % (cell.get("seed", 0), h, w, n, method, oh, ow)).encode()))
    sparse = method == 3
    H, W = h + oh - 1, w + ow - 1
    img = rng.integers(0, 256, (H, W))
    if sparse:
        img = img * (rng.random((H, W)) < 1.0 / 3.0)
    if cell.get("device"):
        kinds = [k for k in KINDS + ("noise",) for _ in range(4)]
        templates = [u[0] for u in device_units(cell)[2]]
    else:
        kinds = cell_kinds(n, cell.get("kinds", "all"))
        templates = [make_template(k, h, w, rng, sparse) for k in kinds]
    assert len(templates) == n and all(t.shape == (h, w) for t in templates)
    assert ow - 1 >= 2 * w, "the three plants need disjoint columns"
    xs = (0, (ow - 1) // 2, ow - 1)
    ys = (min(1, oh - 1), min(4, oh - 1), max(oh - 2, 0))
    tail = kinds.index("flat_top")
    img[ys[0]:ys[0] + h, xs[0]:xs[0] + w] = templates[0]
    img[ys[1]:ys[1] + h, xs[1]:xs[1] + w] = templates[n - 1]
    img[ys[2] + (2 * h) // 3:ys[2] + h, xs[2]:xs[2] + w] = templates[tail][(2 * h) // 3:]
    return np.ascontiguousarray(img.astype(np.uint8)), templates, kinds


def model_stats(img, h, w, method, split):
    return stats_model.window_stats(img, h, w, 1 if method == 5 else 0, tail_s=split)


def predict(lib, cell, thr, split=None, consts=None):
    """The model's decisions for scene(cell) at `thr`: dict(split, waves, leaving, stay)."""
    img, templates, _ = scene(cell)
    h, w, method = cell["h"], cell["w"], cell["method"]
    oh, ow = cell["map"]
    if split is None:
        split = clamp_split(cell["force_split"], h) if cell.get("force_split") else rule_split(lib, h, w, thr)
    g = geometry(oh, ow, len(templates))
    if split <= 0:
        return {"split": 0, "waves": g["waves"], "leaving": 0, "stay": np.ones((g["nyb"], g["nseg"], g["ntg"], WAVES), bool)}
    st = model_stats(img, h, w, method, split)
    consts = table_f64(templates, split) if consts is None else consts
    acc = accumulators(img, templates, split, oh, ow)
    out = wave_pass(acc, consts, templ_stats(lib, templates, method), st["blk"], st["blkq"], method, thr, h, w, oh, ow)
    out["split"] = split
    return out


# The cells of the constants sweep (tests/test_gpu_tail_consts.py, tests/test_tail_model_cpu.py): classes that screen - w in
# 49 .. 64, 8 <= h <= 71, more than 16 templates.  tail_consts_kernel's row loop strides by 64 (h = 64, 65, 71); w % 16 = 1, 8,
# 15, 0; list lengths 17, 20, 32, 33, 49: positions >= 16, partly filled last groups.  "device": the templates are views
# built on the device (mtm_set_templates_augmented: 8 bases x identity / lr / ud / half turn), the other packer.
CONST_CELLS = tuple(
    {"name": "%dx%d-n%d-m%d%s" % (h, w, n, m, "-device" if dev else ""), "h": h, "w": w, "n": n, "method": m, "map": (13, 300),
     "kinds": "all", "device": dev}
    for h, w, n, m, dev in ((8, 64, 17, 5, False), (9, 49, 20, 3, False), (24, 49, 32, 5, False), (24, 56, 33, 3, False),
                            (24, 63, 49, 5, False), (64, 64, 32, 5, True), (65, 56, 17, 3, False), (71, 49, 20, 5, False),
                            (71, 64, 33, 3, False)))
RULE_THRESHOLDS = (0.5, 0.7, 0.9)


def cell_splits(lib, cell):
    """6, 7, h - 2 and the rule's value at 0.5, 0.7 and 0.9, inside [6, h - 2]."""
    h, w = cell["h"], cell["w"]
    s = {6, 7, h - 2} | {rule_split(lib, h, w, t) for t in RULE_THRESHOLDS}
    return sorted(v for v in s if 6 <= v <= h - 2)


def device_units(cell):
    """A "device" cell's templates as (bases, variant records, expanded units): 8 bases of the kinds of KINDS plus one more
    noise template, each in four views that keep its shape."""
    import templ_device_model as D
    assert cell["device"] and cell["n"] == 32
    rng = np.random.default_rng(zlib.crc32(cell["name"].encode()))
    bases = [(make_template(k, cell["h"], cell["w"], rng, cell["method"] == 3), None) for k in KINDS + ("noise",)]
    return bases, list(D.EVEN_VIEWS), D.expand(bases, D.EVEN_VIEWS)


# the scenes whose leaving waves the MFMA counter is held to (tools/tail_wave_count.py): whole items and groups, and one
# with a partial row block, a partial 256-column segment and a partly filled group.  TM_CCORR_NORMED: between windows of
# sparse noise the bound at the rule's split stays above the right-hand side in some lane of every wave (the model: no wave
# leaves at 0.5) - that scene runs a second time with the split forced to h - 2 (MTM_TAIL_SPLIT), where waves do leave.
COUNTER_SCENES = (
    {"name": "64x64-n32", "h": 64, "w": 64, "n": 32, "method": 5, "map": (16, 512), "kinds": "counter"},
    {"name": "24x49-n32", "h": 24, "w": 49, "n": 32, "method": 5, "map": (16, 512), "kinds": "counter"},
    {"name": "24x56-n20", "h": 24, "w": 56, "n": 20, "method": 5, "map": (13, 300), "kinds": "counter"},
    {"name": "24x56-n20-ccorr", "h": 24, "w": 56, "n": 20, "method": 3, "map": (13, 300), "kinds": "counter"},
    {"name": "24x56-n20-ccorr-s22", "h": 24, "w": 56, "n": 20, "method": 3, "map": (13, 300), "kinds": "counter", "force_split": 22},
)
COUNTER_THRESHOLDS = (0.5, 0.7)
