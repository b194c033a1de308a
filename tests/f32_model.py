"""
numpy model of ncc_bf16_kernel<MB, NP> (csrc/mtm_bf16.hip.h) and of the error bound its listing decisions rest on.

model_scores   what the kernel computes, restated: per work item (128 columns x 4 rows of outputs) and channel the tile
               constant mu (8 x 8 sample grid, summed in float32 in the order of the kernel's __shfl_down tree), the image
               pieces a0 + a1 ~ float32(I - mu) and the template pieces T0 + T1 ~ float32(T - mean) (bfloat16, round to
               nearest even), acc = sum a0 T0 (+ a0 T1 + a1 T0) - every product exact in float64, summed in float64 - and
               bf_finish's epilogue on exact float64 window statistics.  The model and the kernel multiply the same
               pieces: they differ by the kernel's float32 accumulation alone.
bound_map      Bf16Params::rig's bound M(x, y) of |bf16 score - exact score|, for 1 .. kMaxChans channels.
accum_map      the accumulation term of that bound alone: the tolerance of kernel against model.

The constants are those of mtm_ctx.h::bf16_rig_eps (two roundings of 2^-24 per MFMA, the whole doubled).
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import mtm_oracle as O

K_MAX_CHANS = 4             # kMaxChans (mtm_kernels.h)
SEG, ROWS = 128, 4          # kBfSeg, kBfRows: outputs of one work item
MAX_W = 256                 # kBfMaxW
ROUNDING = 5.97e-8          # 2^-24 as bf16_rig_eps writes it
PIECE_EPS = {3: 3.0518e-5, 1: 0.0078125 * 1.002}
NORMED = (1, 3, 5)


def nkb_of(w):
    return (w + 31) // 32


def chunk_h_of(w):
    return 64 if nkb_of(w) <= 2 else 32


def chunk_steps(h, w):
    """nsteps = ch * nkb of every K-loop chunk of a channel, in order."""
    ch, nkb = chunk_h_of(w), nkb_of(w)
    return [min(ch, h - cy0) * nkb for cy0 in range(0, h, ch)]


def accum_eps(chans, h, nkb, pieces):
    """The accumulation term of bf16_rig_eps: NP MFMAs per 32-tap block, two roundings each, doubled."""
    return 2.0 * (2.0 * pieces * chans * h * nkb * ROUNDING)


def rig_eps(chans, h, nkb, pieces=3, doubled=True):
    """bf16_rig_eps(chans, h, nkb, np) as the kernel receives it (a float).  doubled=False: the bound as it was before the
    whole was doubled - what test_float32_error_bound_holds has asserted since round 5."""
    if not doubled:
        return (3.0518e-5 if pieces == 3 else 2.0 ** -7 * (1.0 + 2.0 ** -9)) + 2.0 * pieces * chans * h * nkb * ROUNDING
    if pieces == 1:
        return float(np.float32(PIECE_EPS[1] + accum_eps(chans, h, nkb, 1)))
    return float(np.float32(2.0 * (PIECE_EPS[3] + 2.0 * 3.0 * chans * h * nkb * ROUNDING)))


# ---- the tile constant ---------------------------------------------------------------------------------------------------
def tree_sum(v):
    """Lane 0 of  for (off = 32; off > 0; off >>= 1) v += __shfl_down(v, off)  over 64 float32 lanes."""
    v = np.asarray(v, np.float32)
    assert v.shape == (64,)
    n = 32
    while n:
        v = (v[:n] + v[n:2 * n]).astype(np.float32)
        n >>= 1
    return v[0]


def tile_mu(plane, y0, x0, h, lds_cols):
    """s_mu of the work item at (y0, x0): lane 8 i + k holds the sample (i, k), clamped into the image."""
    rows, cols = plane.shape
    sr = np.minimum(y0 + (np.arange(8) * (h + ROWS - 2)) // 7, rows - 1)
    sc = np.minimum(x0 + (np.arange(8) * (lds_cols - 1)) // 7, cols - 1)
    return np.float32(tree_sum(plane[np.ix_(sr, sc)].reshape(64)) * np.float32(1.0 / 64.0))


def mu_planes(img3, h, w):
    """mu of every output's work item, one (oh, ow) float32 plane per channel."""
    rows, cols, chans = img3.shape
    oh, ow = rows - h + 1, cols - w + 1
    lds_cols = SEG + 32 * nkb_of(w)
    out = np.zeros((chans, oh, ow), np.float32)
    for c in range(chans):
        plane = img3[:, :, c]
        for y0 in range(0, oh, ROWS):
            for x0 in range(0, ow, SEG):
                out[c, y0:y0 + ROWS, x0:x0 + SEG] = tile_mu(plane, y0, x0, h, lds_cols)
    return out


# ---- bfloat16 pieces -----------------------------------------------------------------------------------------------------
def bf16_rne(v):
    """float32 -> the bfloat16 nearest to it (ties to even), as a float32 (bf16_rne of the kernel and of the packer)."""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32)
    r = ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)) << np.uint32(16)
    return r.astype(np.uint32).view(np.float32)


def pieces_of(v):
    v = np.ascontiguousarray(v, np.float32)
    v0 = bf16_rne(v)
    return v0, bf16_rne(v - v0)


def _as3d(a):
    a = np.asarray(a)
    return a[:, :, None] if a.ndim == 2 else a


def templ_centred(t3):
    """pack_class_bf16: per channel the mean as a sequential float64 sum over the plane, Tc = float32(T - mean)."""
    h, w, chans = t3.shape
    means, planes = [], []
    for c in range(chans):
        p = t3[:, :, c].astype(np.float64)
        mean = float(np.cumsum(p.reshape(-1))[-1]) / float(h * w)
        means.append(mean)
        planes.append((p - mean).astype(np.float32))
    return means, planes


# ---- statistics and epilogue ---------------------------------------------------------------------------------------------
def window_stats(img3, h, w):
    """Exact float64 window sums per channel and the window sum of squares over all channels."""
    S1 = [O.window_sums(img3[:, :, c].astype(np.float64), h, w) for c in range(img3.shape[2])]
    S2 = sum(O.window_sums(img3[:, :, c].astype(np.float64) ** 2, h, w) for c in range(img3.shape[2]))
    return S1, S2


def _templ_consts(t3, method):
    """templ_mean, templ_norm, templ_sum2 in cv2.matchTemplate's order (oracle/mtm_oracle.py::match_template)."""
    h, w, chans = t3.shape
    area = float(h) * float(w)
    mean, sdv = O._templ_mean_sdv(t3, False)
    norm = sum(s * s for s in sdv)
    all_ones = norm < O.DBL_EPSILON and method == 5
    sum2 = norm + sum(m * m for m in mean)
    if method not in (4, 5):
        mean = [0.0] * chans
        norm = sum2
    return mean, np.sqrt(norm) * np.sqrt(area), sum2 * area, all_ones


def _denominators(img3, t3, method, S1, S2):
    """(sq, templ_norm, ratio num / (sq templ_norm) is taken of), sq = 0 on flat windows."""
    h, w, chans = t3.shape
    area = float(h) * float(w)
    mean2 = sum(s * s for s in S1) / area if method == 5 else 0.0
    diff2 = np.maximum(S2 - mean2, 0.0)
    flat = diff2 <= np.minimum(0.5, 10.0 * O.FLT_EPSILON * S2)
    return np.where(flat, 0.0, np.sqrt(diff2))


def finish(corr, img3, t3, method, S1, S2):
    """bf_finish on a float64 correlation map: the score (float32) and the ratio before the saturation rules."""
    mean, tn, tsum2, all_ones = _templ_consts(t3, method)
    if all_ones:
        return np.ones(corr.shape, np.float32), np.ones(corr.shape)
    if method == 2:
        return corr.astype(np.float32), corr
    num = corr.copy()
    if method in (4, 5):
        for c in range(t3.shape[2]):
            num -= S1[c] * mean[c]
    elif method in (0, 1):
        num = np.maximum(S2 - 2.0 * num + tsum2, 0.0)
    if method not in NORMED:
        return num.astype(np.float32), num
    tt = _denominators(img3, t3, method, S1, S2) * tn
    an = np.abs(num)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = num / tt
    out = np.where(an < tt, r, np.where(an < tt * 1.125, np.where(num > 0, 1.0, -1.0), 1.0 if method == 1 else 0.0))
    return out.astype(np.float32), np.where(tt > 0.0, r, 0.0)


# ---- the model -----------------------------------------------------------------------------------------------------------
def model_acc(img, templs, pieces=3):
    """acc + centre * S1 of the kernel - the correlation map sum I T as it enters bf_finish - for templates of one size:
    a list of float64 (oh, ow) maps."""
    assert pieces in (1, 3)
    img3 = _as3d(img)
    t3s = [_as3d(t) for t in templs]
    # (float64 templates: the masked screen's U = T M^2 and V = M^2, which pack_class_bf16 centres in float64 as well)
    assert img3.dtype == np.float32 and all(t.dtype in (np.float32, np.float64) and t.shape == t3s[0].shape for t in t3s)
    rows, cols, chans = img3.shape
    h, w, _ = t3s[0].shape
    assert 1 <= chans <= K_MAX_CHANS and chans == t3s[0].shape[2] and w <= MAX_W
    oh, ow = rows - h + 1, cols - w + 1
    lds_cols = SEG + 32 * nkb_of(w)
    S1, _ = window_stats(img3, h, w)
    centred = [templ_centred(t) for t in t3s]
    acc = np.zeros((oh, ow, len(t3s)))
    for c in range(chans):
        # (h, w, n): what multiplies a0 and what multiplies a1
        p = [pieces_of(planes[c]) for _, planes in centred]
        with_a0 = np.stack([(t0.astype(np.float64) + t1) if pieces == 3 else t0.astype(np.float64) for t0, t1 in p], axis=2)
        with_a1 = np.stack([t0.astype(np.float64) for t0, _ in p], axis=2)
        plane = img3[:, :, c]
        for y0 in range(0, oh, ROWS):
            nr = min(ROWS, oh - y0)
            for x0 in range(0, ow, SEG):
                nc = min(SEG, ow - x0)
                mu = tile_mu(plane, y0, x0, h, lds_cols)
                a0, a1 = pieces_of(plane[y0:y0 + nr + h - 1, x0:x0 + nc + w - 1] - mu)
                a0, a1 = a0.astype(np.float64), a1.astype(np.float64)
                part = np.zeros((nr, nc, len(t3s)))
                for dy in range(h):
                    part += sliding_window_view(a0[dy:dy + nr], w, axis=1) @ with_a0[dy]
                    if pieces == 3:
                        part += sliding_window_view(a1[dy:dy + nr], w, axis=1) @ with_a1[dy]
                acc[y0:y0 + nr, x0:x0 + nc] += part
        for k, (means, _) in enumerate(centred):
            acc[:, :, k] += means[c] * S1[c]
    return [acc[:, :, k] for k in range(len(t3s))]


def model_scores_many(img, templs, method, pieces=3):
    img3 = _as3d(img)
    h, w = templs[0].shape[:2]
    S1, S2 = window_stats(img3, h, w)
    return [finish(corr, img3, _as3d(t), method, S1, S2)[0] for corr, t in zip(model_acc(img, templs, pieces), templs)]


def model_scores(img, templ, method, pieces=3):
    """The float32 score map ncc_bf16_kernel<MB, pieces> + bf_finish compute, up to the kernel's float32 accumulation."""
    return model_scores_many(img, [templ], method, pieces)[0]


# ---- the bound -----------------------------------------------------------------------------------------------------------
def _bound_factor(img, templ, method):
    """sqrt(sum (I - mu)^2) / sq * (escale sqrt(t2c) / templ_norm) per output, and where it applies (sq > 0, a template that
    is not constant under the method's own norm)."""
    assert method in NORMED
    img3, t3 = _as3d(img), _as3d(templ)
    h, w, chans = t3.shape
    area = float(h * w)
    S1, S2 = window_stats(img3, h, w)
    mu = mu_planes(img3, h, w).astype(np.float64)
    s2c = S2.copy()
    mu2 = np.zeros_like(S2)
    for c in range(chans):
        s2c += mu[c] * (area * mu[c] - 2.0 * S1[c])
        mu2 += mu[c] * mu[c]
    s2c = np.maximum(s2c, 0.0) * 1.000001 + 1e-12 * (np.abs(S2) + area * mu2)
    T = t3.astype(np.float64)
    t2c = float(sum(((T[:, :, c] - T[:, :, c].mean()) ** 2).sum() for c in range(chans)))
    tn = np.sqrt(t2c) if method == 5 else np.sqrt((T * T).sum())
    esc = 2.0 if method == 1 else 1.0
    sq = _denominators(img3, t3, method, S1, S2)
    live = (sq > 0.0) & (tn > 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.sqrt(s2c) / sq * (esc * np.sqrt(t2c) / tn)
    return np.where(live, f, 0.0), live


def bound_map(img, templ, method, pieces=3, doubled=True, r=None):
    """M(x, y) = rig_eps * sqrt(sum (I - mu)^2) / sq * (escale sqrt(t2c) / templ_norm) + 3e-7 max(1, |r|), and where it
    applies.  mu per channel, sum (I - mu)^2 and t2c summed over the channels.  r: the ratio before the saturation rules
    (None: |r| <= 1, the compared outputs)."""
    t3 = _as3d(templ)
    f, live = _bound_factor(img, templ, method)
    eps = rig_eps(t3.shape[2], t3.shape[0], nkb_of(t3.shape[1]), pieces, doubled)
    tail = 3e-7 * (1.0 if r is None else np.maximum(1.0, np.abs(r)))
    return np.where(live, eps * f + tail, 0.0), live


def accum_map(img, templ, method, pieces=3, r=None):
    """What is left of bound_map without the piece term: 2 (2 NP chans h nkb 5.97e-8) * the same factor + 3e-7 max(1, |r|)."""
    t3 = _as3d(templ)
    f, live = _bound_factor(img, templ, method)
    tail = 3e-7 * (1.0 if r is None else np.maximum(1.0, np.abs(r)))
    return np.where(live, accum_eps(t3.shape[2], t3.shape[0], nkb_of(t3.shape[1]), pieces) * f + tail, 0.0), live


def tolerances(img, templ, method, pieces=3):
    """(accum_map, bound_map, where they apply) of the compared outputs (|r| < 1), on one evaluation of the common factor."""
    t3 = _as3d(templ)
    f, live = _bound_factor(img, templ, method)
    chans, h, nkb = t3.shape[2], t3.shape[0], nkb_of(t3.shape[1])
    return (np.where(live, accum_eps(chans, h, nkb, pieces) * f + 3e-7, 0.0),
            np.where(live, rig_eps(chans, h, nkb, pieces) * f + 3e-7, 0.0), live)


# ---- scenes beyond the range the geometry sweep covers -------------------------------------------------------------------
# The cells of tests/test_gpu_f32_range.py: the smallest ones that still reach each code form of the kernel.
RANGE_CELLS = [
    dict(name="12x20", h=12, w=20, n=4, chans=1, out=(9, 133)),         # nkb 1, 12 padded taps
    dict(name="5x33", h=5, w=33, n=4, chans=1, out=(9, 133)),           # nkb 2, 31 padded taps: the widest reach
    dict(name="5x64", h=5, w=64, n=4, chans=1, out=(9, 133)),           # no padded tap: the control
    dict(name="33x97", h=33, w=97, n=4, chans=1, out=(5, 41)),          # nkb 4, two K chunks of 32 rows
    dict(name="24x40-n17", h=24, w=40, n=17, chans=1, out=(9, 133)),    # MB = 2, two template groups
    dict(name="7x40-c3", h=7, w=40, n=4, chans=3, out=(9, 133)),        # channels
]
# power-of-two factors: every scaled scene is the base scene exactly (float32 scaling by 2^k neither rounds nor leaves the
# normal range at these magnitudes)
SCALES = {"up40": 40, "down20": -20, "down40": -40, "huge": 60, "tiny": -60}
IN_RANGE = ("up40", "down20", "down40")
BASE_NOISE = 10.0           # the noisy templates' noise in base units (the geometry sweep's, noise+ and signed)
NAN_PAYLOAD = 0x7FFFFFFF    # bad pixel (d): a NaN whose payload carries into the exponent under bf16_rne's rounding add
FLT_MAX = float(np.finfo(np.float32).max)


def _range_rng(*key):
    import zlib
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def tile_samples(rows, cols, oh, ow, h, w):
    """{(row, column)} of every work item's 8 x 8 sample grid (tile_mu's addresses)."""
    lds_cols = SEG + 32 * nkb_of(w)
    out = set()
    for y0 in range(0, oh, ROWS):
        for x0 in range(0, ow, SEG):
            sr = np.minimum(y0 + (np.arange(8) * (h + ROWS - 2)) // 7, rows - 1)
            sc = np.minimum(x0 + (np.arange(8) * (lds_cols - 1)) // 7, cols - 1)
            out |= {(int(r), int(c)) for r in sr for c in sc}
    return out


def _not_finite(img):
    return ~np.isfinite(_as3d(img)).all(axis=2)


def kernel_reach(img, h, w):
    """The outputs whose accumulators see a non-finite operand: the work item's sample grid holds one (s_mu, subtracted from
    every pixel of the tile), or one lies in rows y .. y + h - 1 and columns x .. x + 32 nkb - 1 - the taps w .. 32 nkb - 1
    carry zero template pieces and still multiply the pixels right of the window (0 * NaN = NaN).  The staging loop of
    ncc_bf16_kernel fills lds_cols = 128 + 32 nkb columns from the tile's first column; an output at column x reads columns
    x - x0 .. x - x0 + 32 nkb - 1 of it.  Beyond the image the staged pixels are the zero padding."""
    nf = _not_finite(img)
    rows, cols = nf.shape
    oh, ow = rows - h + 1, cols - w + 1
    span = 32 * nkb_of(w)
    lds_cols = SEG + span
    out = np.zeros((oh, ow), bool)
    for y0 in range(0, oh, ROWS):
        for x0 in range(0, ow, SEG):
            sr = np.minimum(y0 + (np.arange(8) * (h + ROWS - 2)) // 7, rows - 1)
            sc = np.minimum(x0 + (np.arange(8) * (lds_cols - 1)) // 7, cols - 1)
            tile_bad = bool(nf[np.ix_(sr, sc)].any())
            for y in range(y0, min(y0 + ROWS, oh)):
                for x in range(x0, min(x0 + SEG, ow)):
                    out[y, x] = tile_bad or bool(nf[y:y + h, x:x + span].any())
    return out


def window_dirty(img, h, w):
    """The outputs whose own window holds a non-finite pixel."""
    nf = _not_finite(img)
    oh, ow = nf.shape[0] - h + 1, nf.shape[1] - w + 1
    return np.array([[bool(nf[y:y + h, x:x + w].any()) for x in range(ow)] for y in range(oh)])


def engine_stats_dirty(img, h, w):
    """The outputs whose window statistics the engine's running sums poison.  hsum_kernel / hsum_lds_kernel: a thread sums
    columns x0 .. x0 + w - 1 of a row (x0 a multiple of 16), stores, and slides 16 times (s += I[x + w] - I[x]); once a
    non-finite pixel has entered the sum it stays (inf - inf = NaN).  vsum_stats_kernel: the same down a column of those
    sums, restarting every 32 output rows.  So a bad pixel reaches right and downward, to the end of its segment."""
    nf = _not_finite(img)
    rows, cols = nf.shape
    oh, ow = rows - h + 1, cols - w + 1
    hs = np.zeros((rows, ow), bool)
    for r in range(rows):
        for x0 in range(0, ow, 16):
            dirty = False
            for dx in range(w):
                dirty = dirty or bool(nf[r, x0 + dx])
            for k in range(16):
                x = x0 + k
                if x >= ow:
                    break
                hs[r, x] = dirty
                if x + w < cols:                        # (the zero padding beyond the row is finite)
                    dirty = dirty or bool(nf[r, x + w])
    out = np.zeros((oh, ow), bool)
    for x in range(ow):
        for y0 in range(0, oh, 32):
            dirty = False
            for dy in range(h):
                dirty = dirty or bool(hs[y0 + dy, x])
            for y in range(y0, min(y0 + 32, oh)):
                out[y, x] = dirty
                if y + 1 < min(y0 + 32, oh):
                    dirty = dirty or bool(hs[y + h, x])
    return out


def window_scores(img, templ, method, points):
    """cv2.matchTemplate's epilogue on sums taken window by window in float64 - no cumulative sums, so a non-finite pixel
    touches the windows that hold it and no other: float32 scores at `points` [(y, x)]."""
    img3, t3 = _as3d(img), _as3d(templ)
    h, w, chans = t3.shape
    T = t3.astype(np.float64)
    corr = np.zeros(len(points))
    S1 = [np.zeros(len(points)) for _ in range(chans)]
    S2 = np.zeros(len(points))
    for i, (y, x) in enumerate(points):
        W = img3[y:y + h, x:x + w].astype(np.float64)
        for c in range(chans):
            corr[i] += float((W[:, :, c] * T[:, :, c]).sum())
            S1[c][i] = float(W[:, :, c].sum())
            S2[i] += float((W[:, :, c] * W[:, :, c]).sum())
    with np.errstate(invalid="ignore", over="ignore"):
        return finish(corr, img3, t3, method, S1, S2)[0]


def accumulators_surely_finite(img, templ):
    """True when no float32 partial sum of the kernel's accumulators can leave the finite range: every centred operand is at
    most twice the largest magnitude of its array, the pieces add up to (1 + 2^-7) of it, three products per tap."""
    img3, t3 = _as3d(img), _as3d(templ)
    h, w, chans = t3.shape
    fin = np.abs(img3[np.isfinite(img3)].astype(np.float64))
    amax = 2.0 * float(fin.max()) if fin.size else 0.0
    tmax = 2.0 * float(np.abs(t3.astype(np.float64)).max())
    return 3.0 * 1.02 * chans * h * 32 * nkb_of(w) * amax * tmax < FLT_MAX


def _place_nonfinite(shape, h, w, oh, ow, chans, t0):
    """Where the copies of template 0 and the bad pixels go: ({label: (y, x)}, {label: (row, column, channel, bits)},
    {label: why it is left out}).  Copies in the order a, c, b from the left, their windows apart; (b) and (c) outside the
    work item (0, 0) whose sample grid holds pixel (a)."""
    rows, cols = shape[:2]
    nkb = nkb_of(w)
    pad = 32 * nkb - w
    samples = tile_samples(rows, cols, oh, ow, h, w)
    copies, bad, skipped = {}, {}, {}
    nan_bits = int(np.array([np.nan], np.float32).view(np.uint32)[0])
    inf_bits = int(np.array([np.inf], np.float32).view(np.uint32)[0])
    # (a) a default NaN at pixel (0, 0), a sample of tile (0, 0); its copy at output (1, 40): inside that tile, right of
    # columns 0 .. 15 whose statistics the NaN poisons
    if oh > 1 and ow > 40:
        copies["a"], bad["a"] = (1, 40), (0, 0, 0, nan_bits)
    else:
        skipped["a"] = "no output (1, 40) in a %d x %d map" % (oh, ow)
    x_next = 40 + w
    # (c) -inf one row under a copy's last row
    yc, xc = min(4, oh - 2), x_next
    if oh >= 6 and xc + w <= ow - 1 + w and xc <= ow - 1 and xc + w <= cols:
        # (the three windows under the copy multiply the pixel by taps of template 0's last row: positive ones, or the
        # float64 kernel's TM_SQDIFF_NORMED there is fmax(S2 - 2 (+inf) + T2, 0) = 0 and the copy is no local minimum)
        last = _as3d(t0)[h - 1, :, 2 % chans]
        cc = next((c for c in range(xc + w // 2, xc + w - 1) if (yc + h, c) not in samples and
                   (last[c - xc - 1:c - xc + 2] > 0).all()), None)
        if cc is not None and yc >= ROWS:
            copies["c"], bad["c"] = (yc, xc), (yc + h, cc, 2 % chans, inf_bits | 0x80000000)
            x_next = xc + w
    if "c" not in copies:
        skipped["c"] = "no room for a third copy outside work item (0, 0) with a row under it in a %d x %d map" % (oh, ow)
    # (b) +inf d columns right of a copy's last column, in a row the copy covers (below copy (a)'s rows)
    yb, xb = min(4, oh - 1), x_next
    if pad == 0:
        skipped["b"] = "w = %d is a multiple of 32: no padded tap" % w
    elif yb < ROWS or xb > ow - 1:
        skipped["b"] = "no room for a copy beside copy (a) outside work item (0, 0) in a %d x %d map" % (oh, ow)
    else:
        spot = next(((r, xb + w - 1 + d, d) for d in range(pad, 0, -1) for r in range(yb + h - 1, max(yb, h + 1) - 1, -1)
                     if xb + w - 1 + d <= cols - 1 and (r, xb + w - 1 + d) not in samples), None)
        if spot is None:
            skipped["b"] = "no pixel right of the copy inside the image"
        else:
            copies["b"], bad["b"] = (yb, xb), (spot[0], spot[1], 1 % chans, inf_bits)
    # (d) a NaN with payload 0x7FFFFFFF in a region no copy touches: the image's last row, under the columns 0 .. 15 whose
    # statistics pixel (a) poisons already (a small map keeps outputs the model is compared on)
    rd = rows - 1
    cd = next((c for c in range(4, 16) if (rd, c) not in samples), None)
    if cd is not None and rd > h:
        bad["d"] = (rd, cd, 0, NAN_PAYLOAD)
    else:
        skipped["d"] = "no free pixel in the last row"
    return copies, bad, skipped


def range_scene(cell, name, kind="noise+"):
    """A scene of tests/test_gpu_f32_range.py: dict(img, clean, templs, cuts, copies, bad, skipped).  `name`: a key of SCALES - the
    base scene of `kind` ("noise+": N(100, 40), "signed": N(0, 40)) times 2^k, templates included - or "nonfinite": noise+
    with exact copies of template 0 planted beside bad pixels (clean: the image without them).  Templates are cut from the
    image; every third one (1, 4, 7 ..) carries noise in the scene's own units."""
    h, w, chans, (oh, ow) = cell["h"], cell["w"], cell["chans"], cell["out"]
    shape = (h + oh - 1, w + ow - 1) + ((chans,) if chans > 1 else ())
    assert kind in ("noise+", "signed") and (name in SCALES or (name == "nonfinite" and kind == "noise+"))
    rng = _range_rng("range", cell["name"], kind)               # (one base scene per cell and kind, whatever the factor)
    img = rng.normal(100.0 if kind == "noise+" else 0.0, 40.0, shape).astype(np.float32)
    templs, cuts = [], []
    for k in range(cell["n"]):
        r = _range_rng("range", cell["name"], kind, "t", k)
        y, x = int(r.integers(0, oh)), int(r.integers(0, ow))
        cuts.append((y, x))
        t = img[y:y + h, x:x + w].copy()
        if k % 3 == 1:
            t = (t + r.normal(0.0, BASE_NOISE, t.shape)).astype(np.float32)
        templs.append(np.ascontiguousarray(t))
    copies, bad, skipped = {}, {}, {}
    clean = img
    if name == "nonfinite":
        copies, bad, skipped = _place_nonfinite(shape, h, w, oh, ow, chans, templs[0])
        for y, x in copies.values():
            img[y:y + h, x:x + w] = templs[0]
        clean = img.copy()
        flat = _as3d(img).view(np.uint32)
        for r, c, ch, bits in bad.values():
            flat[r, c, ch] = bits
    else:
        f = np.float32(2.0 ** SCALES[name])
        img = img * f
        templs = [np.ascontiguousarray(t * f) for t in templs]
        assert np.isfinite(img).all() and img.dtype == np.float32
        clean = img
    return dict(img=img, clean=clean, templs=templs, cuts=cuts, copies=copies, bad=bad, skipped=skipped)
