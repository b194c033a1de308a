"""
Sub-pixel hit positions from 3 x 3 score neighbourhoods.

``hitNeighbourhoods`` returns, for every hit of any search function, the scores of the hit's template at the nine windows
around the hit, computed by one native call (mtm_hit_neighbourhoods) instead of one whole score map per template:

    computeScoreMap(template, image, method, mask)[y - 1:y + 2, x - 1:x + 2]        (NaN outside the map)

``refineHits`` fits a parabola through each axis of that neighbourhood (``fit_offsets``) and returns the hits at
fractional positions.  A hit ``(label, (x, y, w, h), score)`` is in image coordinates, as every search function returns
it (searchBox offsets included); its template is the entry of ``listTemplates`` with that label and that (h, w).

Scope: ``computeScoreMap``'s pixel policy (``_apply_pixel_policy``) - uint8 with 1 or 3 channels, uint16 with 1 channel,
and everything the policy matches in float32 with 1 or 3 channels; masks with methods 0 and 3 (other methods drop them with
computeScoreMap's warning); float64 raises.  uint8 and uint16 neighbourhoods equal computeScoreMap's values bit for bit;
float32 ones agree with them to rounding (1e-6 relative), except on flat windows.  Anything out of scope, a hit without
its template, and a hit whose window is outside the map raise ValueError before any native call.
"""
import numbers
from typing import List

import numpy as np

from . import _lib
from . import TM_CCOEFF_NORMED, _apply_pixel_policy, _check_opencv_preconditions

__all__ = ["hitNeighbourhoods", "refineHits", "fit_offsets"]


def fit_offsets(nbhd, method):
    """The sub-pixel offsets (ox, oy) of the centres of (n, 3, 3) neighbourhoods, as two float64 arrays of n.

    Per axis, the three scores along it as doubles a, b, c (neighbour at -1, centre, neighbour at +1), negated for methods 0
    and 1 (minima): the offset is ``0.5 * (a - c) / d`` with ``d = (a - 2*b) + c`` when a, b and c are finite, b >= a,
    b >= c and d < 0 (then |offset| <= 0.5; two equal maxima give +-0.5), and 0.0 otherwise - the map's border, flat
    (NaN) windows, a hit that is not an extremum of its neighbourhood."""
    n = np.asarray(nbhd, dtype=np.float32).reshape(-1, 3, 3).astype(np.float64)
    if method in (0, 1):
        n = -n

    def axis(a, b, c):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            d = (a - 2.0 * b) + c
            ok = np.isfinite(a) & np.isfinite(b) & np.isfinite(c) & (b >= a) & (b >= c) & (d < 0)
            return np.where(ok, 0.5 * (a - c) / np.where(ok, d, -1.0), 0.0)

    return axis(n[:, 1, 0], n[:, 1, 1], n[:, 1, 2]), axis(n[:, 0, 1], n[:, 1, 1], n[:, 2, 1])


def _integer(v):
    return isinstance(v, (numbers.Integral, np.integer)) and not isinstance(v, bool)


def _parse_hits(hits):
    """hits -> (labels list, (n, 4) int64 array of x, y, w, h); a malformed hit raises ValueError naming its index."""
    try:
        labels, boxes, _ = zip(*hits)
        b = np.array(boxes)
        if b.shape == (len(hits), 4) and b.dtype.kind in "iu":
            return list(labels), b.astype(np.int64)
    except (TypeError, ValueError, OverflowError):
        pass
    for i, hit in enumerate(hits):          # (the slow path finds the offending hit)
        try:
            label, box, _ = hit
            x, y, w, h = box
        except (TypeError, ValueError):
            raise ValueError("hit %d is not (label, (x, y, w, h), score)" % i) from None
        if not all(_integer(v) for v in (x, y, w, h)):
            raise ValueError("hit %d: the box (x, y, w, h) must hold integers (got %r)" % (i, (x, y, w, h)))
    raise ValueError("hits: the boxes (x, y, w, h) must hold integers")


def _same_entry(a, b):
    """Two entries of listTemplates with the same pixels and the same mask (or both none)."""
    ta, tb = a[1], b[1]
    if ta.dtype != tb.dtype or ta.shape != tb.shape or not np.array_equal(ta, tb):
        return False
    ma = a[2] if len(a) >= 3 else None
    mb = b[2] if len(b) >= 3 else None
    if (ma is None) != (mb is None):
        return False
    return ma is None or (ma.dtype == mb.dtype and ma.shape == mb.shape and np.array_equal(ma, mb))


def _lookup(listTemplates, labels, b):
    """Index into listTemplates of each hit's template: the entry with the hit's label and (h, w)."""
    by_key = {}
    for j, t in enumerate(listTemplates):
        if not isinstance(t, tuple) or len(t) < 2:
            raise ValueError("listTemplates should be a list of tuples as ('name','array') or ('name', 'array', 'mask')")
        try:
            key = (t[0], int(t[1].shape[0]), int(t[1].shape[1]))
            by_key.setdefault(key, []).append(j)
        except TypeError:               # an unhashable label: found by the linear scan below
            pass
    idx = []
    known = {}                              # key -> template index, once its entries were checked
    for i, (label, h, w) in enumerate(zip(labels, b[:, 3].tolist(), b[:, 2].tolist())):
        try:
            idx.append(known[(label, h, w)])
            continue
        except (KeyError, TypeError):
            pass
        try:
            cand = by_key.get((label, h, w), [])
        except TypeError:
            cand = [j for j, t in enumerate(listTemplates) if t[0] == label and t[1].shape[:2] == (h, w)]
        if not cand:
            raise ValueError("hit %d: no template labelled %r of %d x %d (h x w) in listTemplates" % (i, label, h, w))
        for j in cand[1:]:
            if not _same_entry(listTemplates[cand[0]], listTemplates[j]):
                raise ValueError("hit %d: templates %d and %d are both labelled %r with shape %d x %d but differ" % (
                    i, cand[0], j, label, h, w))
        try:
            known[(label, h, w)] = cand[0]
        except TypeError:
            pass
        idx.append(cand[0])
    return np.array(idx, dtype=np.int64)


def _prepare(listTemplates, image, method, used):
    """The pixel policy of computeScoreMap for the templates `used` (indices): {j: (template, mask, policy image)}."""
    if not isinstance(image, np.ndarray) or image.ndim not in (2, 3):
        raise ValueError("image must be a 2-D (grayscale) or 3-D (rows, cols, channels) numpy array")
    ichans = 1 if image.ndim == 2 else image.shape[2]
    if ichans not in (1, 3):
        raise ValueError("hitNeighbourhoods takes images with 1 or 3 channels (got %d)" % ichans)
    prepared = {}
    images = {}
    for j in used:
        t = listTemplates[j]
        mask = t[2] if len(t) >= 3 else None
        tt, im, m = _apply_pixel_policy(t[1], image, method, mask)
        _check_opencv_preconditions(tt, im)
        if im.dtype not in (np.uint8, np.uint16, np.float32):
            raise ValueError("hitNeighbourhoods: pixel type %s is not supported" % im.dtype)
        if im.dtype == np.uint16 and ichans != 1:
            raise ValueError("hitNeighbourhoods takes single-channel uint16 images (got %d channels)" % ichans)
        key = str(im.dtype)
        im = images.setdefault(key, im)         # (one policy image per pixel type)
        prepared[j] = (tt, m, im)
    return prepared


def _neighbourhoods(listTemplates, image, hits, method, ctx, resident):
    """hitNeighbourhoods on `ctx`.  `resident` (TemplateMatcher): every template of the list is set, in list order, as
    TemplateMatcher.match would set them for this image.  Returns (array, the resident kind (pixel type name, channels) when
    templates were set in that way, else None)."""
    hits = list(hits)
    if not hits:
        return np.zeros((0, 3, 3), dtype=np.float32), None
    labels, b = _parse_hits(hits)
    idx = _lookup(listTemplates, labels, b)
    used = range(len(listTemplates)) if resident else np.unique(idx).tolist()
    prepared = _prepare(listTemplates, image, method, used)
    H, W = image.shape[0], image.shape[1]
    x, y, w, h = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    outside = np.flatnonzero((x < 0) | (y < 0) | (x > W - w) | (y > H - h))
    if len(outside):
        i = int(outside[0])
        raise ValueError("hit %d: window (%d, %d) of a %d x %d template is outside the %d x %d image's score map" % (
            i, x[i], y[i], h[i], w[i], H, W))
    kinds = sorted({str(p[2].dtype) for p in prepared.values()})
    if resident and len(kinds) > 1:
        raise ValueError("TemplateMatcher needs templates of one pixel type (all uint8, all uint16, or neither)")
    out = np.empty((len(hits), 3, 3), dtype=np.float32)
    ctx = ctx or _lib.default_context()         # (only now: every argument error comes before "no GPU")
    ichans = 1 if image.ndim == 2 else image.shape[2]
    with ctx.lock:
        for kind in kinds:
            group = [j for j in used if str(prepared[j][2].dtype) == kind]
            slot = np.full(len(listTemplates), -1, dtype=np.int64)
            slot[group] = np.arange(len(group))
            sel = np.flatnonzero(slot[idx] >= 0)
            pts = np.empty(len(sel), dtype=_lib.POINT_DTYPE)
            pts["templ_idx"] = slot[idx[sel]]
            pts["x"] = x[sel]
            pts["y"] = y[sel]
            ctx.set_templates([(prepared[j][0], prepared[j][1]) for j in group], method)
            out[sel] = ctx.hit_neighbourhoods(prepared[group[0]][2], pts)
    return out, ((kinds[0], ichans) if resident else None)


def hitNeighbourhoods(listTemplates, image: np.ndarray, hits, method: int = TM_CCOEFF_NORMED, *, context=None) -> np.ndarray:
    """
    The 3 x 3 score neighbourhoods of ``hits`` (any search function's output, in image coordinates): a float32 array of
    shape (len(hits), 3, 3) whose element ``[i, 1 + dy, 1 + dx]`` is the score of hit i's template at window
    ``(x + dx, y + dy)`` of the whole image's score map - ``computeScoreMap(template, image, method, mask)[y + dy, x + dx]``
    - and NaN for a window outside the map.  Hit i's template is the entry of listTemplates with the hit's label and
    (h, w).  ``context``: the _lib.Context to run on (default: the process's).
    """
    return _neighbourhoods(listTemplates, image, hits, method, context, False)[0]


def _refined(hits, nbhd, method):
    ox, oy = fit_offsets(nbhd, method)
    return [(label, (int(x) + a, int(y) + b, w, h), score)
            for (label, (x, y, w, h), score), a, b in zip(hits, ox.tolist(), oy.tolist())]


def refineHits(listTemplates, image: np.ndarray, hits, method: int = TM_CCOEFF_NORMED, *, context=None) -> List[tuple]:
    """
    ``hits`` at sub-pixel positions: one ``(label, (xf, yf, w, h), score)`` per hit, in input order, with
    ``xf = x + ox`` and ``yf = y + oy`` Python floats - ``fit_offsets`` of the hit's ``hitNeighbourhoods`` - and the hit's
    own score unchanged.  The fractional boxes are positions, not drawing boxes: they are not meant for drawBoxesOnRGB /
    drawBoxesOnGray, which take whole pixels.
    """
    hits = list(hits)
    nb = hitNeighbourhoods(listTemplates, image, hits, method, context=context)
    return _refined(hits, nb, method)
