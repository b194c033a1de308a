"""
Many searchBoxes of one image in one engine call: the loop a user writes today,

    [findMatches([listTemplates[j] for j in indices_i], image, method, N_object, score_threshold, searchBox=box_i)
     for box_i, indices_i in regions]

(or the same with ``matchTemplates`` and ``maxOverlap``), with the same hits, order, labels, full-image boxes, float32
score bits, exceptions and warnings, computed by one native call (mtm_find_matches_boxes): the image is
uploaded once, and every (region, template) pair - a unit - gets the score map of its crop from one tiled kernel launch.

An element of ``searchBoxes`` is a box ``(x, y, w, h)``, which searches every template, or a pair
``((x, y, w, h), indices)``, which searches ``[listTemplates[j] for j in indices]``.  A box that extends past the image is
clipped as numpy slicing clips it (what ``searchBox`` does); a region with an empty index list returns ``[]``.

Scope (anything else raises ValueError before any native call): uint8 images and templates with 1 or 3 channels, or
single-channel uint16 ones (templates of at most 2^21 pixels), every template of the image's dtype and channel count;
methods 0..5 (``findMatchesInBoxes``) or 1..5 (``matchTemplatesInBoxes``; 0 raises the loop's TM_SQDIFF error); no
masks for methods 0 and 3; box offsets ``x, y >= 0``.
"""
import numbers
import warnings
from typing import List, Sequence

import numpy as np

from . import _lib
from . import _MSG_MASK_UNSUPPORTED, _MSG_SQDIFF, Hit, TemplateTuple, TM_CCOEFF_NORMED

__all__ = ["findMatchesInBoxes", "matchTemplatesInBoxes"]

_MSG_TUPLES = "listTemplates should be a list of tuples as ('name','array') or ('name', 'array', 'mask')"
_I64 = np.dtype(np.int64)
_SCOPE_METHODS = (0, 1, 2, 3, 4, 5)
_U16_MAX_PIXELS = 1 << 21       # mtm_find_matches_boxes: uint16 correlations stay below 2^53, exact in float64


def _is_int(v):
    return isinstance(v, numbers.Integral)


class _Regions:
    """searchBoxes parsed: boxes (R x 4: x, y, w, h), the units (region, template index) in loop order, and the first
    region whose index list would raise in the user's list comprehension (IndexError), or None."""
    __slots__ = ("boxes", "u_region", "u_templ", "bad_index")

    def __init__(self, searchBoxes, n_templ):
        self.bad_index = None
        boxes = None
        try:
            arr = np.asarray(searchBoxes)
            if arr.ndim == 2 and arr.shape[1] == 4 and arr.dtype.kind in "iu":
                boxes = arr.astype(_I64)
        except (ValueError, TypeError):       # ragged: pairs with index lists
            pass
        if boxes is not None:                 # plain boxes: every template in every region
            R = len(boxes)
            self.boxes = boxes
            self.u_region = np.repeat(np.arange(R, dtype=_I64), n_templ)
            self.u_templ = np.tile(np.arange(n_templ, dtype=_I64), R)
            return
        # pairs: one pass that only splits the elements, then the boxes and the index lists as two numpy arrays
        blist, lens, flat = [], [], []
        for i, el in enumerate(searchBoxes):
            if len(el) == 2:
                box, idx = el
                n0 = len(flat)
                flat.extend(idx)
                lens.append(len(flat) - n0)
            elif len(el) == 4:
                box = el
                lens.append(-1)                                  # every template
            else:
                raise ValueError("searchBoxes[%d]: expected (x, y, w, h) or ((x, y, w, h), indices)" % i)
            if len(box) != 4:
                raise ValueError("searchBoxes[%d]: a box is (x, y, w, h)" % i)
            blist.append(box)
        R = len(blist)
        lens = np.asarray(lens, dtype=_I64)
        self.boxes = _int_array(blist, "box values", lambda k: k // 4).reshape(R, 4) if R else np.zeros((0, 4), _I64)
        listed = lens >= 0
        ix = _int_array(flat, "template indices", lambda k: int(np.searchsorted(np.cumsum(np.maximum(lens, 0)), k,
                                                                                   side="right")))
        counts = np.where(listed, lens, n_templ)
        self.u_region = np.repeat(np.arange(R, dtype=_I64), counts)
        u_listed = np.repeat(listed, counts)
        u_templ = np.empty(len(self.u_region), _I64)
        u_templ[~u_listed] = np.tile(np.arange(n_templ, dtype=_I64), int(np.count_nonzero(~listed)))
        u_templ[u_listed] = ix
        bad = u_listed & ((u_templ < -n_templ) | (u_templ >= n_templ))
        if bad.any():          # [listTemplates[j] for j in indices] raises before this region's call; its units do not run
            self.bad_index = int(self.u_region[int(np.argmax(bad))])
            self.u_region, u_templ = self.u_region[~bad], u_templ[~bad]
        self.u_templ = np.where(u_templ < 0, u_templ + n_templ, u_templ)      # Python's negative list indices


def _int_array(values, what, region_of):
    """`values` as an int64 array; TypeError naming the region of the first value that is not an integer."""
    a = np.asarray(values) if len(values) else np.zeros(0, _I64)
    if a.dtype.kind in "iub":
        return a.astype(_I64).reshape(-1)
    for k, v in enumerate(np.asarray(values, dtype=object).reshape(-1)):
        if not _is_int(v):
            raise TypeError("searchBoxes[%d]: %s must be integers" % (region_of(k), what))
    return a.astype(_I64).reshape(-1)


def _slice_len(start, length, size):
    """len(range(size)[start:start + length]) for start >= 0: numpy's clipping of a searchBox crop."""
    stop = start + length
    stop = np.where(stop < 0, stop + size, stop)
    stop = np.clip(stop, 0, size)
    return np.maximum(stop - np.minimum(start, size), 0)


def _templ_info(listTemplates, used):
    """Per template: the first loop error its own checks raise (MTM._validate_search: tuple form, height 0, width 0) as
    (type, message) or None, and its height / width / whether the tuple has a mask slot.  Only `used` ones are looked at."""
    n = len(listTemplates)
    err = [None] * n
    h = np.zeros(n, _I64)
    w = np.zeros(n, _I64)
    slot = np.zeros(n, bool)
    for j in used:
        t = listTemplates[j]
        if not isinstance(t, tuple) or len(t) < 2:
            err[j] = (ValueError, _MSG_TUPLES)
            continue
        shp = t[1].shape
        slot[j] = len(t) >= 3
        if shp[0] == 0:
            err[j] = (ValueError, f"Template '{t[0]}' has a height of 0.")
        elif shp[1] == 0:
            err[j] = (ValueError, f"Template '{t[0]}' has a width of 0.")
        h[j], w[j] = shp[0], shp[1]
    return err, h, w, slot


def _check_scope(listTemplates, image, used, method, methods):
    if not _is_int(method) or method not in methods:
        raise ValueError("the searchBox calls take methods %d..5 (got %r)" % (methods[0], method))
    ok_img = (image.dtype == np.uint8 and (image.ndim == 2 or (image.ndim == 3 and image.shape[2] in (1, 3)))) or \
        (image.dtype == np.uint16 and (image.ndim == 2 or (image.ndim == 3 and image.shape[2] == 1)))
    if not ok_img:
        raise ValueError("the searchBox calls take uint8 images with 1 or 3 channels and single-channel uint16 images "
                         "(got a %s image of shape %s)" % (image.dtype, image.shape))
    for j in used:
        t = listTemplates[j]
        if not isinstance(t, tuple) or len(t) < 2:
            continue                          # (the loop's own error, raised in loop order)
        a = t[1]
        if a.dtype != image.dtype:
            raise ValueError("the searchBox calls take templates of the image's dtype (template '{}' is {}, the image "
                             "{})".format(t[0], a.dtype, image.dtype))
        if a.ndim != image.ndim or (a.ndim == 3 and a.shape[2] != image.shape[2]):
            raise ValueError("Template '{}' and the image differ in their channels".format(t[0]))
        if method in (0, 3) and len(t) >= 3 and t[2] is not None:
            raise ValueError("Template '{}': masks are not supported by the searchBox calls".format(t[0]))
        if a.dtype == np.uint16 and a.shape[0] * a.shape[1] > _U16_MAX_PIXELS:
            raise ValueError("Template '{}': uint16 templates of more than 2^21 pixels are not supported by the searchBox "
                             "calls (their exact correlations would pass 2^53)".format(t[0]))


def _plan(listTemplates, image, searchBoxes, method, N_object, methods, maxOverlap=None, first_region_only=False):
    """Every check of the loop, in the loop's order, and the scope checks - before anything reaches the library.
    Emits the loop's mask warnings.  `first_region_only`: the loop stops after its first region (matchTemplates with
    TM_SQDIFF raises once that region's search ran), so only that region's errors count.  Returns (regions, BOX_UNIT_DTYPE units with templ_idx = list index), or None when
    there is no region."""
    n_templ = len(listTemplates)
    reg = _Regions(searchBoxes, n_templ)
    R = len(reg.boxes)
    if R == 0:
        return None
    # what the first iteration of the loop checks before any template (MTM.matchTemplates, MTM._validate_search)
    if maxOverlap is not None and (maxOverlap < 0 or maxOverlap > 1):
        raise ValueError("Maximal overlap between bounding box is in range [0-1]")
    if N_object != float("inf") and not isinstance(N_object, int):
        raise TypeError("N_object must be an integer")
    if image.shape[0] == 0:
        raise ValueError("Image has a height of 0.")
    if image.shape[1] == 0:
        raise ValueError("Image has a width of 0.")
    used = np.unique(reg.u_templ).tolist()
    _check_scope(listTemplates, image, used, method, methods)
    if (reg.boxes[:, :2] < 0).any():
        i = int(np.argmax((reg.boxes[:, :2] < 0).any(axis=1)))
        raise ValueError("searchBoxes[%d]: negative box offsets are not supported (numpy slicing would wrap around)" % i)
    H, W = image.shape[:2]
    crop_h = _slice_len(reg.boxes[:, 1], reg.boxes[:, 3], H)
    crop_w = _slice_len(reg.boxes[:, 0], reg.boxes[:, 2], W)
    err, th, tw, slot = _templ_info(listTemplates, used)
    # the first unit, in loop order, whose template check fails (own error, or larger than its crop)
    ur, ut = reg.u_region, reg.u_templ
    own = np.fromiter((err[j] is not None for j in ut), bool, len(ut)) if any(e is not None for e in err) else \
        np.zeros(len(ut), bool)
    larger = (th[ut] > crop_h[ur]) | (tw[ut] > crop_w[ur])
    bad = own | larger
    first = int(np.argmax(bad)) if bad.any() else -1
    bad_region = int(ur[first]) if first >= 0 else None
    if reg.bad_index is not None and (bad_region is None or reg.bad_index <= bad_region):
        bad_region, first = reg.bad_index, -1
    if first_region_only and bad_region is not None and bad_region > 0:
        bad_region, first = None, -1
    # mask warnings: one per (region, template tuple with a mask slot) of the regions the loop completes
    n_warn = 0
    if method not in (0, 3) and slot.any():
        done = ur < bad_region if bad_region is not None else np.ones(len(ur), bool)
        n_warn = int(np.count_nonzero(slot[ut] & done))
    if first >= 0 or bad_region is not None:
        for _ in range(n_warn):
            warnings.warn(_MSG_MASK_UNSUPPORTED)
        if first < 0:
            raise IndexError("list index out of range")
        j = int(ut[first])
        if err[j] is not None:
            raise err[j][0](err[j][1])
        pos = first - int(np.searchsorted(ur, ur[first]))          # the template's index in its region's list
        raise ValueError("Template '{}' at index {} in the list of templates is larger than searchBox.".format(
            listTemplates[j][0], pos))
    for _ in range(n_warn):
        warnings.warn(_MSG_MASK_UNSUPPORTED)
    units = np.empty(len(ut), dtype=_lib.BOX_UNIT_DTYPE)
    units["templ_idx"] = ut
    units["y0"] = reg.boxes[ur, 1]
    units["x0"] = reg.boxes[ur, 0]
    units["rows"] = crop_h[ur]
    units["cols"] = crop_w[ur]
    return reg, units


def _labels(listTemplates):
    labels = np.empty(len(listTemplates), dtype=object)
    for i, t in enumerate(listTemplates):          # element-wise: a label may be any object (even a tuple)
        labels[i] = t[0]
    return labels


def _split_hits(raw, counts, listTemplates):
    """Structured hits (templ_idx = index into listTemplates, full-image boxes) -> one list of Hit per region, counts[r]
    each: the columns converted at once, as MTM._to_hit_list does."""
    labels = _labels(listTemplates)
    boxes = zip(raw["x"].tolist(), raw["y"].tolist(), raw["w"].tolist(), raw["h"].tolist())
    hits = list(zip(labels[raw["templ_idx"]].tolist(), boxes, list(raw["score"])))
    ends = np.cumsum(counts).tolist()
    starts = [0] + ends[:-1]
    return [hits[a:b] for a, b in zip(starts, ends)]


def _search(listTemplates, image, reg, units, method, N_object, score_threshold, ctx, resident):
    """The native call.  `resident`: the context holds every template of listTemplates in list order (TemplateMatcher);
    otherwise the templates the units use are set now.  Returns (raw hits, templ_idx = list index; records per region;
    whether templates were set on the context - not when no unit is left to search)."""
    mode = _lib.PEAKS_GLOBAL if N_object == 1 else _lib.PEAKS_LOCAL
    R = len(reg.boxes)
    if len(units) == 0:
        return np.zeros(0, dtype=_lib.HIT_DTYPE), np.zeros(R, _I64), False
    if resident:
        used = None
        templates = [(t[1], None) for t in listTemplates]
    else:
        used = np.unique(units["templ_idx"])
        units = units.copy()
        units["templ_idx"] = np.searchsorted(used, units["templ_idx"])
        templates = [(listTemplates[j][1], None) for j in used.tolist()]
    ctx = ctx or _lib.default_context()         # (only now: every argument error comes before "no GPU")
    with ctx.lock:
        ctx.set_templates(templates, method)
        raw, ucounts = ctx.find_matches_boxes(image, units, mode, score_threshold)
    if used is not None and len(raw):
        raw = raw.copy()
        raw["templ_idx"] = used[raw["templ_idx"]]
    rcounts = np.bincount(reg.u_region, weights=ucounts, minlength=R).astype(_I64)
    return raw, rcounts, True


def _nms_regions(raw, rcounts, score_threshold, method, N_object, maxOverlap, fused_cut):
    """MTM.matchTemplates' suppression (MTM._nms_raw, or the engine's fused one) on each region's hits, without a Python
    loop over the regions.  `fused_cut`: the loop's uint8 calls with 0 <= N_object < inf cut every list to N_object
    (mtm_find_matches_image_nms), a list of one hit included; elsewhere a list of at most one hit stays as it is."""
    R = len(rcounts)
    starts = np.concatenate(([0], np.cumsum(rcounts)[:-1])).astype(_I64)
    if N_object == 1:
        # python max() / min() per region as MTM._nms_raw: the first best hit; a list of <= 1 hit as it is
        keep_r = rcounts > 0
        if not keep_r.any():
            return raw[:0], np.zeros(R, _I64)
        seg = np.repeat(np.arange(R), rcounts)
        sc = raw["score"].astype(np.float64)
        q = -sc if method == 1 else sc
        best = np.full(R, -np.inf)
        np.maximum.at(best, seg, q)
        idx = np.arange(len(raw))
        cand = np.where(q == best[seg], idx, len(raw))
        first = np.full(R, len(raw))
        np.minimum.at(first, seg, cand)
        sel = first[keep_r]
        return raw[sel], keep_r.astype(_I64)
    keep, kcounts = _lib.nms_segments(raw, rcounts, score_threshold, maxOverlap, ascending=(method == 1))
    if N_object != float("inf"):
        N = int(N_object)
        if fused_cut and N >= 0:
            limit = np.minimum(kcounts, N)
        else:           # MTM._nms_raw: indexes[:N_object], after a list of <= 1 hit was returned as it is
            limit = np.minimum(kcounts, N) if N >= 0 else np.maximum(kcounts + N, 0)
            limit = np.where(rcounts <= 1, kcounts, limit)
        kstarts = np.concatenate(([0], np.cumsum(kcounts)[:-1])).astype(_I64)
        rank = np.arange(len(keep)) - np.repeat(kstarts, kcounts)
        keep = keep[rank < np.repeat(limit, kcounts)]
        kcounts = limit.astype(_I64)
    return raw[keep], kcounts


def findMatchesInBoxes(listTemplates: Sequence[TemplateTuple], image: np.ndarray, searchBoxes, method: int = TM_CCOEFF_NORMED,
                       N_object=float("inf"), score_threshold: float = 0.5, *, context=None) -> List[List[Hit]]:
    """
    ``[findMatches(subset_i, image, method, N_object, score_threshold, searchBox=box_i) for each region i]`` in one
    engine call.  ``searchBoxes``: boxes ``(x, y, w, h)`` (every template) or pairs ``((x, y, w, h), indices)`` (the
    templates ``listTemplates[j]`` for j in indices).  ``context``: the _lib.Context to run on (default: the process's).
    uint8 (1 or 3 channels) or single-channel uint16, methods 0..5, no masks for methods 0 and 3.
    """
    plan = _plan(listTemplates, image, searchBoxes, method, N_object, _SCOPE_METHODS)
    if plan is None:
        return []
    reg, units = plan
    raw, rcounts, _ = _search(listTemplates, image, reg, units, method, N_object, score_threshold, context, False)
    return _split_hits(raw, rcounts, listTemplates)


def _match_boxes(listTemplates, image, searchBoxes, method, N_object, score_threshold, maxOverlap, ctx, resident):
    """matchTemplatesInBoxes on `ctx`.  Returns (hits per region, whether templates were set on the context)."""
    plan = _plan(listTemplates, image, searchBoxes, method, N_object, _SCOPE_METHODS, maxOverlap=maxOverlap,
                 first_region_only=method == 0)
    if plan is None:
        return [], False
    if method == 0:     # as the loop: after the first region's checks and search (MTM/__init__.py:291)
        raise ValueError(_MSG_SQDIFF)
    reg, units = plan
    raw, rcounts, uploaded = _search(listTemplates, image, reg, units, method, N_object, score_threshold, ctx, resident)
    kept, kcounts = _nms_regions(raw, rcounts, score_threshold, method, N_object, maxOverlap,
                                 fused_cut=image.dtype == np.uint8)
    return _split_hits(kept, kcounts, listTemplates), uploaded


def matchTemplatesInBoxes(listTemplates: Sequence[TemplateTuple], image: np.ndarray, searchBoxes,
                          method: int = TM_CCOEFF_NORMED, N_object=float("inf"), score_threshold: float = 0.5,
                          maxOverlap: float = 0.25, *, context=None) -> List[List[Hit]]:
    """
    ``[matchTemplates(subset_i, image, method, N_object, score_threshold, maxOverlap, searchBox=box_i) for each region
    i]`` in one engine call: findMatchesInBoxes' hits, then matchTemplates' non-maxima suppression on each region's hits
    separately.  Methods 1..5 (0 raises the loop's TM_SQDIFF error).
    """
    return _match_boxes(listTemplates, image, searchBoxes, method, N_object, score_threshold, maxOverlap, context,
                        False)[0]
