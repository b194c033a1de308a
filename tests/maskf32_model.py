"""
numpy model of the masked float32 screen (csrc/mtm_maskf32.hip.h, launch_masked_bf16 in csrc/mtm_launch.hip) and the table of
cells, scenes and masks tests/test_maskf32_model_cpu.py and tests/test_gpu_maskf32_screen.py walk.

exact_sums     c1 = sum I (T M^2), c2 = sum I^2 M^2 and tms = sum (T M)^2 in float64 from the float32 inputs, the weights
               formed as the engine forms them (double(t) * (double(m) * double(m)): pack_class_bf16 and the float64
               kernel's weight arena), and the exact quality (the score; minima: minus the score).
raw_model      what the two raw launches compute up to their float32 accumulation: f32_model.model_acc (the unmasked
               kernel's model, reused as it is) of I against U = T M^2 and of J = float32(I I) against V = M^2.
pixel_terms,   maskf32_pixel and maskf32_bounds restated in float64, branch by branch; eps is f32_model.rig_eps(1, h, nkb,
bounds         pieces), centred_sum2 of U and V as pack_class_bf16 sums them.
listed_*       the listing rules of maskf32_combine_kernel and of maskf32_best_kernel + maskf32_list_best_kernel.
"""
import zlib

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import f32_model as F

SQDIFF, CCORR_NORMED = 0, 3
METHODS = (CCORR_NORMED, SQDIFF)
DEFAULT_MAP = (9, 133)      # 133: the second 128-column segment holds 5 outputs; 9: the third row block one row


# ---- weights and exact sums ----------------------------------------------------------------------------------------------
def weights(t, m):
    """U = T M^2 and V = M^2 in float64 as place_templates forms them: m2 = m * m (exact for float32 m), u = t * m2."""
    T, M = np.asarray(t, np.float32).astype(np.float64), np.asarray(m, np.float32).astype(np.float64)
    m2 = M * M
    return T * m2, m2


def seq_sum(v):
    """A float64 sum in index order (the host loops of compute_templ_stats and pack_class_bf16)."""
    return float(np.cumsum(np.asarray(v, np.float64).reshape(-1))[-1])


def templ_tms(t, m):
    v = np.asarray(t, np.float32).astype(np.float64) * np.asarray(m, np.float32).astype(np.float64)
    return seq_sum(v * v)


def centred_sum2(x):
    """pack_class_bf16 (which = 1, 2): mean = (sequential sum) / plane, then the sequential sum of (x - mean)^2."""
    mean = seq_sum(x) / float(x.size)
    return seq_sum((x - mean) * (x - mean))


def window_sum(plane, h, w):
    """Direct float64 window sums (no running sums: a pixel that is not finite reaches the windows that hold it only)."""
    win = sliding_window_view(np.asarray(plane, np.float64), (h, w))
    return win.reshape(win.shape[0], win.shape[1], h * w).sum(axis=2)


def exact_sums(img, units):
    """Per template (c1, c2, tms): float64 sums over the float64 products of the float32 inputs."""
    I = np.asarray(img, np.float32).astype(np.float64)
    h, w = units[0][0].shape
    with np.errstate(over="ignore", invalid="ignore"):
        w1 = sliding_window_view(I, (h, w))
        w2 = sliding_window_view(I * I, (h, w))
        oh, ow = w1.shape[:2]
        U = np.stack([weights(t, m)[0].reshape(-1) for t, m in units], axis=1)
        V = np.stack([weights(t, m)[1].reshape(-1) for t, m in units], axis=1)
        c1 = (w1.reshape(oh * ow, h * w) @ U).reshape(oh, ow, len(units))
        c2 = (w2.reshape(oh * ow, h * w) @ V).reshape(oh, ow, len(units))
    return [(c1[:, :, k], c2[:, :, k], templ_tms(*units[k])) for k in range(len(units))]


def quality(method, c1, c2, tms):
    """The exact quality: TM_CCORR_NORMED c1 / sqrt(tms c2) (0 / 0 is NaN, as in OpenCV), TM_SQDIFF -(-2 c1 + c2 + tms)."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if method == SQDIFF:
            return -(-2.0 * c1 + c2 + tms)
        return c1 / np.sqrt(tms * c2)


# ---- the raw launches ----------------------------------------------------------------------------------------------------
def square_f32(img):
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return (np.asarray(img, np.float32) * np.asarray(img, np.float32)).astype(np.float32)


def raw_model(img, units, pieces):
    """([c1 model per template], [c2 model per template]): f32_model.model_acc of I x U and of J x V."""
    Us, Vs = zip(*(weights(t, m) for t, m in units))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return (F.model_acc(np.asarray(img, np.float32), list(Us), pieces), F.model_acc(square_f32(img), list(Vs), pieces))


def tile_mu_plane(plane, h, w):
    """Bf16Params::mu_out: the tile constant of every work item, [yb][seg]."""
    rows, cols = plane.shape
    oh, ow = rows - h + 1, cols - w + 1
    lds_cols = F.SEG + 32 * F.nkb_of(w)
    out = np.zeros(((oh + F.ROWS - 1) // F.ROWS, (ow + F.SEG - 1) // F.SEG), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for yb in range(out.shape[0]):
            for seg in range(out.shape[1]):
                out[yb, seg] = F.tile_mu(plane, yb * F.ROWS, seg * F.SEG, h, lds_cols)
    return out


def per_output(mu, oh, ow):
    return np.repeat(np.repeat(mu, F.ROWS, axis=0), F.SEG, axis=1)[:oh, :ow]


# ---- maskf32_pixel and maskf32_bounds ------------------------------------------------------------------------------------
class Pixel:
    """What the bounds need of the image: exact window sums of I, I^2, J, J^2, the tile constants per output, and
    maskf32_pixel's si, sj.  s_i, s_j: sum (I - mu)^2 and sum (J - mu_J)^2 without the allowances (the pixel term of the
    accumulation tolerance)."""

    def __init__(self, img, h, w):
        I = np.asarray(img, np.float32)
        J = square_f32(I)
        oh, ow = I.shape[0] - h + 1, I.shape[1] - w + 1
        area = float(h) * float(w)
        self.mu_i, self.mu_j = tile_mu_plane(I, h, w), tile_mu_plane(J, h, w)
        with np.errstate(over="ignore", invalid="ignore"):
            I64, J64 = I.astype(np.float64), J.astype(np.float64)
            s1i, s2i = window_sum(I64, h, w), window_sum(I64 * I64, h, w)
            s1j, s2j = window_sum(J64, h, w), window_sum(J64 * J64, h, w)
            mi, mj = per_output(self.mu_i, oh, ow).astype(np.float64), per_output(self.mu_j, oh, ow).astype(np.float64)
            si = s2i + mi * (area * mi - 2.0 * s1i)
            sj = s2j + mj * (area * mj - 2.0 * s1j)
            self.s_i, self.s_j = np.fmax(si, 0.0), np.fmax(sj, 0.0)
            self.si = np.fmax(si, 0.0) * 1.000001 + 1e-12 * (np.abs(s2i) + area * mi * mi)
            self.sj = np.fmax(sj, 0.0) * 1.000001 + 1e-12 * (np.abs(s2j) + area * mj * mj)


def error_terms(px, cs2_u, cs2_v, eps, c1, c2):
    """E1 and E2 as maskf32_bounds states them (c1, c2: the approximate sums, float32 values as float64)."""
    with np.errstate(over="ignore", invalid="ignore"):
        e1 = eps * np.sqrt(px.si * cs2_u) * 1.000002 + 3e-7 * np.abs(c1) + 1e-30
        e2 = eps * np.sqrt(px.sj * cs2_v) * 1.000002 + 6e-7 * np.abs(c2) + 1e-30
    return e1, e2


def bounds(method, px, cs2_u, cs2_v, tms, eps, c1, c2):
    """(lb, ub) of the quality, float64 - maskf32_bounds, every branch."""
    c1, c2 = np.asarray(c1, np.float64), np.asarray(c2, np.float64)
    e1, e2 = error_terms(px, cs2_u, cs2_v, eps, c1, c2)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if method == SQDIFF:
            s = -2.0 * c1 + c2 + tms
            slack = (2.0 * e1 + e2) + 4e-7 * (2.0 * np.abs(c1) + np.abs(c2) + abs(tms))
            return -(s + slack), -(s - slack)
        if not tms > 0.0:
            return np.full(c1.shape, -np.inf), np.full(c1.shape, np.inf)
        num_hi, num_lo = c1 + e1, c1 - e1
        c2_lo, c2_hi = c2 - e2, c2 + e2
        # (comparisons with NaN are false: the else branches, as in the kernel)
        ub = np.where(num_hi <= 0.0, np.where(c2_hi > 0.0, num_hi / np.sqrt(tms * c2_hi), 0.0),
                      np.where(c2_lo > 0.0, num_hi / np.sqrt(tms * c2_lo), np.inf))
        lb = np.where(num_lo >= 0.0, np.where(c2_hi > 0.0, num_lo / np.sqrt(tms * c2_hi), 0.0),
                      np.where(c2_lo > 0.0, num_lo / np.sqrt(tms * c2_lo), -np.inf))
        ub = ub + 4e-7 * np.fmax(1.0, np.abs(ub))
        lb = lb - 4e-7 * np.fmax(1.0, np.abs(lb))
    return lb, ub


def contains(lb, ub, q):
    """lb <= q <= ub, no tolerance; a bound that is NaN does not exist (the output is listed instead)."""
    with np.errstate(invalid="ignore"):
        return ((lb <= q) | np.isnan(lb)) & ((q <= ub) | np.isnan(ub))


# ---- the listing rules ---------------------------------------------------------------------------------------------------
def thr_quality(method, thr):
    """maskf32_combine_kernel's thr_q: the float32 score threshold, negated for minima."""
    t = float(np.float32(thr))
    return -t if method == SQDIFF else t


def listed_threshold(method, ub, thr):
    with np.errstate(invalid="ignore"):
        return ~(ub < thr_quality(method, thr))


def round_up_f32(v):
    """maskf32_best_kernel's ubf: float32(ub) moved up where the conversion went below; NaN -> +inf."""
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.asarray(v, np.float64).astype(np.float32)
        f = np.where(f.astype(np.float64) < v, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)
    return np.where(np.isnan(v), np.float32(np.inf), f).astype(np.float32)


def round_down_f32(v):
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.asarray(v, np.float64).astype(np.float32)
        return np.where(f.astype(np.float64) > v, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


def best_lower(lb):
    """best[t] decoded: the largest rounded-down lb that is not NaN; -inf where there is none."""
    f = round_down_f32(lb)
    f = f[~np.isnan(f)]
    return np.float32(f.max()) if f.size else np.float32(-np.inf)


def listed_global(lb, ub):
    with np.errstate(invalid="ignore"):
        return ~(round_up_f32(ub) < best_lower(lb))


def key_to_float(key):
    """mf_order_float; 0: no key was published (-inf)."""
    key = int(key)
    if key == 0:
        return np.float32(-np.inf)
    b = (key ^ 0x80000000) if key & 0x80000000 else (~key & 0xFFFFFFFF)
    return np.array([b], np.uint32).view(np.float32)[0]


# ---- the table -----------------------------------------------------------------------------------------------------------
SCENES_LIVE = ("noise+", "signed", "offset", "step")            # a live screen is required on these
_EXTRA = ["signed", "offset", "step", "tiny", "huge", "nonfinite"]
MASKS = ("disc", "uniform", "signed", "large", "one_tap", "zero_rows", "zero")
CELLS = []


PER_MASK = 2                # templates per mask of a cell that is no list: an exact cut and a noisy one


def _cell(family, h, w, n=0, out=DEFAULT_MAP, on_route=True):
    """Templates share a size class - one screen - only where their masks are EQUAL (size_classes): a cell is one class
    per mask.  n = 0: every mask of MASKS with PER_MASK templates; n > 0 (lists): ONE class of n templates under one mask,
    which rotates over the list cells and their scenes."""
    name = "%s-%dx%d" % (family, h, w) + ("-n%d" % n if n else "") + ("-o%dx%d" % out if family == "outputs" else "")
    CELLS.append(dict(name=name, family=family, h=h, w=w, n=n, out=out, on_route=on_route, index=len(CELLS),
                      scenes=("noise+", _EXTRA[len(CELLS) % len(_EXTRA)])))


for _w in (7, 32, 33, 64, 65, 129, 255, 256):
    _cell("taps", 5, _w)
_cell("off-route", 5, 257, on_route=False)
for _h, _w in ((64, 33), (65, 33), (32, 97), (33, 97)):
    _cell("chunks", _h, _w)
for _h in (1, 2, 3, 67):
    _cell("steps", _h, 20)
for _n in (1, 16, 17, 33):
    _cell("lists", 24, 40, n=_n)
for _out in ((2, 2), (3, 7), (5, 9), (9, 127), (9, 128), (9, 129), (5, 257)):
    _cell("outputs", 5, 31, out=_out)
NAMES = [c["name"] for c in CELLS]
assert len(set(NAMES)) == len(NAMES)


def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def _step_image(rng, shape):
    """tests/test_gpu_f32_geometry.py::scene_image's step image."""
    rows, cols = shape
    im = np.zeros(shape, np.float32)
    im[:, cols // 2:] = 1.0
    im += rng.normal(0.0, 2e-3, shape).astype(np.float32)
    r0, c0, pr, pc = rows // 8, cols // 16, max(2, rows // 3), max(2, cols // 5)
    im[r0:r0 + pr, c0:c0 + pc] += rng.normal(0.0, 0.2, im[r0:r0 + pr, c0:c0 + pc].shape).astype(np.float32)
    return im


_NOISE = {"noise+": 10.0, "signed": 10.0, "offset": 1.25, "step": 5e-4, "tiny": 10.0e-18, "huge": 10.0e18, "nonfinite": 10.0}


def mask_of(kind, h, w, rng):
    if kind == "disc":
        yy, xx = np.mgrid[0:h, 0:w]
        m = ((((yy - h / 2 + 0.5) / (h / 2)) ** 2 + ((xx - w / 2 + 0.5) / (w / 2)) ** 2) <= 1.0).astype(np.float32)
        if not m.any():
            m[h // 2, w // 2] = 1.0
        return m
    if kind == "uniform":
        return rng.random((h, w)).astype(np.float32)
    if kind == "signed":
        return (2.0 * rng.random((h, w)) - 1.0).astype(np.float32)
    if kind == "large":
        return (1000.0 * rng.random((h, w))).astype(np.float32)
    if kind == "one_tap":
        m = np.zeros((h, w), np.float32)
        m[int(rng.integers(0, h)), int(rng.integers(0, w))] = 1.0
        return m
    if kind == "zero_rows":
        # zero rows across the K-chunk boundary where the template has one, else across its middle
        # (h = 2: one of the two rows; h = 1: columns across the template's middle instead)
        m = (0.25 + rng.random((h, w))).astype(np.float32)
        ch = F.chunk_h_of(w)
        mid = ch if h > ch else h // 2
        if h >= 3:
            m[mid - 1:mid + 1] = 0.0
        elif h == 2:
            m[1] = 0.0
        else:
            m[:, max(0, w // 2 - 1):w // 2 + 1] = 0.0
        return m
    assert kind == "zero"
    return np.zeros((h, w), np.float32)


_LIST_MASKS = (("disc", "uniform"), ("uniform", "signed"), ("signed", "large"), ("large", "zero_rows"))


def mask_groups(cell, name):
    """[(mask kind, [template indices])]: the size classes of a cell's scene."""
    if cell["n"]:
        kind = _LIST_MASKS[(1, 16, 17, 33).index(cell["n"])][cell["scenes"].index(name)]
        return [(kind, list(range(cell["n"])))]
    return [(kind, list(range(g * PER_MASK, (g + 1) * PER_MASK))) for g, kind in enumerate(MASKS)]


def scene(cell, name):
    """(image, [(template, mask)], groups, [(template index, y, x)] of the exact copies planted - the first template, twice:
    global mode's ties).  Within a class the templates 1, 4, 7 .. carry noise, the others are exact cuts."""
    h, w, (oh, ow) = cell["h"], cell["w"], cell["out"]
    shape = (h + oh - 1, w + ow - 1)
    rng = _rng(cell["name"], name)
    if name in ("noise+", "nonfinite"):
        img = rng.normal(100.0, 40.0, shape).astype(np.float32)
    elif name in ("signed", "tiny", "huge"):
        img = rng.normal(0.0, 40.0, shape).astype(np.float32)
    elif name == "offset":
        img = rng.normal(1000.0, 5.0, shape).astype(np.float32)
    else:
        assert name == "step"
        img = _step_image(rng, shape)
    if name == "tiny":
        img = (img * np.float32(1e-18)).astype(np.float32)
    if name == "huge":
        img = (img * np.float32(1e18)).astype(np.float32)
    groups = mask_groups(cell, name)
    units = [None] * sum(len(m) for _, m in groups)
    for g, (kind, members) in enumerate(groups):
        mask = mask_of(kind, h, w, _rng(cell["name"], name, "m", g))
        for j, k in enumerate(members):
            r = _rng(cell["name"], name, "t", k)
            y, x = int(r.integers(0, oh)), int(r.integers(0, ow))
            t = img[y:y + h, x:x + w].copy()
            if j % 3 == 1:
                t = (t + r.normal(0.0, _NOISE[name], t.shape)).astype(np.float32)
            units[k] = (np.ascontiguousarray(t), mask)
    # exact copies of the first template, planted twice where the image has room for two that do not overlap
    plants = []
    t0 = units[0][0]
    # (columns 1 .. w and cols - w - 1 .. cols - 2: apart once cols >= 2 w + 2, i.e. ow >= w + 3)
    if ow >= w + 3 and oh > 1:
        for (y, x) in ((1, 1), (1, shape[1] - w - 1)):
            img[y:y + h, x:x + w] = t0
            plants.append((0, y, x))
    if name == "nonfinite":
        r = _rng(cell["name"], name, "bad")
        for v in (np.nan, np.inf):
            y, x = int(r.integers(0, shape[0])), int(r.integers(0, shape[1]))
            if not any(py <= y < py + h and px_ <= x < px_ + w for _, py, px_ in plants):
                img[y, x] = v
    return img, units, groups, plants


def threshold_for(method, q):
    """A cell's threshold from its exact map, one rule for all: midway between the 0.9 quantile of the finite qualities and
    their maximum, as a score (minima: negated back), rounded to float32 as the engine takes it."""
    f = q[np.isfinite(q)]
    if f.size == 0:
        return 0.0
    tq = 0.5 * (float(np.quantile(f, 0.9)) + float(f.max()))
    with np.errstate(over="ignore"):            # (`huge`: beyond float32 - the threshold is +-inf)
        return float(np.float32(-tq if method == SQDIFF else tq))


class CellModel:
    """Everything the two test files need of one (cell, scene): exact sums, the pixel terms, per template cs2 and tms; the
    raw model and the model bounds per `pieces` on demand."""

    def __init__(self, cell, scene_name):
        self.cell, self.scene = cell, scene_name
        self.img, self.units, self.groups, self.plants = scene(cell, scene_name)
        self.kinds = [kind for kind, members in self.groups for _ in members]
        self.h, self.w = cell["h"], cell["w"]
        self.nkb = F.nkb_of(self.w)
        self.exact = exact_sums(self.img, self.units)
        self.px = Pixel(self.img, self.h, self.w) if cell["on_route"] else None
        self.cs2 = [(centred_sum2(U), centred_sum2(V)) for U, V in (weights(t, m) for t, m in self.units)]
        self._raw = {}

    def eps(self, pieces):
        return F.rig_eps(1, self.h, self.nkb, pieces)

    def raw(self, pieces):
        if pieces not in self._raw:
            self._raw[pieces] = raw_model(self.img, self.units, pieces)
        return self._raw[pieces]

    def q(self, method, k):
        c1, c2, tms = self.exact[k]
        return quality(method, c1, c2, tms)

    def bounds_from(self, method, pieces, k, c1, c2):
        return bounds(method, self.px, self.cs2[k][0], self.cs2[k][1], self.exact[k][2], self.eps(pieces), c1, c2)

    def model_bounds(self, method, pieces, k):
        m1, m2 = self.raw(pieces)
        with np.errstate(over="ignore", invalid="ignore"):
            c1 = m1[k].astype(np.float32).astype(np.float64)
            c2 = m2[k].astype(np.float32).astype(np.float64)
        return self.bounds_from(method, pieces, k, c1, c2)

    def threshold(self, method, g):
        """The threshold of class g: the rule on the exact map of the class's first template."""
        return threshold_for(method, self.q(method, self.groups[g][1][0]))


# the capacity test's cell, scene and class: on `offset` the one-product bound lists every output (see
# test_maskf32_model_cpu.py), the three-product bound the exact copies and a handful more
LADDER = ("taps-5x32", "offset", 0)


def ladder_counts(cm, g):
    """{pieces: outputs of class g listed under TM_CCORR_NORMED at the class's threshold by the model bounds}."""
    thr = cm.threshold(CCORR_NORMED, g)
    return {pieces: sum(int(listed_threshold(CCORR_NORMED, cm.model_bounds(CCORR_NORMED, pieces, k)[1], thr).sum())
                        for k in cm.groups[g][1]) for pieces in (1, 3)}
