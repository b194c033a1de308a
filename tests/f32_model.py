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
