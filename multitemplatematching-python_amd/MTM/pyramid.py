"""
Coarse-to-fine search: the reference's two speed-ups of Tutorial 3 (``tutorials/Tutorial3-SpeedingUp.ipynb``: a
searchBox, and matching a downscaled image and template) combined.

A downscaled search proposes candidates; full-resolution scores are computed only in small windows around them, with
the arithmetic of the exhaustive search.  Hits keep full-resolution positions, sizes and bit-exact scores.  Where the
windows cover every hit the exhaustive search reports, the result is exactly that of ``findMatches`` /
``matchTemplates``; elsewhere a hit the coarse level did not propose is missed.

Semantics, with ``I`` the uint8 image after the searchBox crop and ``f`` the factor:

1. Coarse level: ``augment.downscale(I, f)`` against ``augment.downscale(T, f)``; a template's candidates are the local
   extrema of its coarse map (findMatches' 3x3 rule and border option) that pass ``coarse_threshold``, the best
   ``max_candidates`` of them (ties in row-major order).  This gating applies for ``N_object == 1`` too: such a call
   can return ``[]``, where ``matchTemplates`` always returns a hit.
2. Windows: a candidate at coarse output ``(cy, cx)`` covers full-resolution rows ``[cy f - r, cy f + r]`` and columns
   ``[cx f - r, cx f + r]`` of the score map (clipped), ``r = radius`` (default ``f``).
3. Fine level: the positions of the windows' union that are local extrema of the full-resolution score map (the
   exhaustive rule; neighbours outside the windows count) and pass ``score_threshold``; with ``N_object == 1`` the
   extremum over the union.
"""
import numbers
import warnings
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from . import _MSG_MASK_UNSUPPORTED, _MSG_SQDIFF, _nms_raw, _to_hit_list, _validate_search, BBox, Hit, TemplateTuple
from . import TM_CCOEFF_NORMED

__all__ = ["findMatchesPyramid", "matchTemplatesPyramid"]



def _is_int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def _check_pyramid(listTemplates, image, method, factor, score_threshold, coarse_threshold, radius, max_candidates):
    """The scope of the coarse-to-fine search, checked before anything reaches the library.  `image` is already cropped
    to the searchBox.  Returns (units, coarse_threshold, radius)."""
    if method == 0:
        raise ValueError(_MSG_SQDIFF)
    if method not in (1, 2, 3, 4, 5):
        raise ValueError("method must be one of 1..5 (TM_SQDIFF_NORMED .. TM_CCOEFF_NORMED)")
    if not _is_int(factor) or factor < 2:
        raise ValueError("factor must be an integer >= 2")
    if radius is None:
        radius = int(factor)
    if not _is_int(radius) or radius < 0:
        raise ValueError("radius must be an integer >= 0")
    if not _is_int(max_candidates) or max_candidates < 1:
        raise ValueError("max_candidates must be an integer >= 1")
    if coarse_threshold is None:
        if method in (2, 4):
            raise ValueError("methods 2 (TM_CCORR) and 4 (TM_CCOEFF) need an explicit coarse_threshold: raw sums differ "
                             "between scales")
        coarse_threshold = score_threshold + 0.1 if method == 1 else score_threshold - 0.1
    if image.dtype != np.uint8:
        raise ValueError("the pyramid search takes uint8 images and templates (got a %s image)" % image.dtype)
    if image.ndim not in (2, 3) or (image.ndim == 3 and image.shape[2] not in (1, 3)):
        raise ValueError("the pyramid search takes grayscale or 3-channel images")
    H, W = image.shape[:2]
    Hc, Wc = H // factor, W // factor
    units = []
    n_ignored = 0
    for index, tempTuple in enumerate(listTemplates):
        t = tempTuple[1]
        label = tempTuple[0]
        if len(tempTuple) >= 3:
            if method == 3:
                if tempTuple[2] is not None:
                    raise ValueError("Template '{}': masks are not supported by the pyramid search".format(label))
            else:
                n_ignored += 1
        if t.dtype != np.uint8:
            raise ValueError("the pyramid search takes uint8 images and templates (template '{}' is {})".format(
                label, t.dtype))
        if t.ndim != image.ndim or (t.ndim == 3 and t.shape[2] != image.shape[2]):
            raise ValueError("Template '{}' and the image differ in their channels".format(label))
        h, w = t.shape[:2]
        hc, wc = h // factor, w // factor
        if hc < 2 or wc < 2:
            raise ValueError("Template '{}' downscaled by {} is {}x{}: the coarse template must be at least 2x2".format(
                label, factor, hc, wc))
        if hc > Hc or wc > Wc:
            raise ValueError("Template '{}' downscaled by {} is larger than the downscaled image".format(label, factor))
        if Hc - hc + 1 < 2 or Wc - wc + 1 < 2:
            raise ValueError("Template '{}': the coarse score map is {}x{}; the pyramid search needs 2-D maps of at "
                             "least 2x2".format(label, Hc - hc + 1, Wc - wc + 1))
        if H - h + 1 < 2 or W - w + 1 < 2:
            raise ValueError("Template '{}': the score map is {}x{}; the pyramid search needs 2-D maps of at least "
                             "2x2".format(label, H - h + 1, W - w + 1))
        units.append((t, None))
    for _ in range(n_ignored):      # as findMatches warns: one per template tuple with a mask slot
        warnings.warn(_MSG_MASK_UNSUPPORTED)
    return units, coarse_threshold, radius


def _raw_pyramid(listTemplates, image, factor, method, N_object, score_threshold, searchBox, coarse_threshold, radius,
                 max_candidates, context):
    image, xOffset, yOffset = _validate_search(listTemplates, image, N_object, searchBox)
    units, coarse_threshold, radius = _check_pyramid(listTemplates, image, method, factor, score_threshold,
                                                     coarse_threshold, radius, max_candidates)
    mode = _lib.PEAKS_GLOBAL if N_object == 1 else _lib.PEAKS_LOCAL
    if not units:
        return np.zeros(0, dtype=_lib.HIT_DTYPE), xOffset, yOffset
    engine = context or _lib.default_context()
    with engine.lock:
        engine.set_templates(units, method)
        raw = engine.find_matches_pyramid(image, factor, mode, coarse_threshold, score_threshold, radius, max_candidates)
    return raw, xOffset, yOffset


def findMatchesPyramid(listTemplates: Sequence[TemplateTuple], image: np.ndarray, factor: int,
                       method: int = TM_CCOEFF_NORMED, N_object=float("inf"), score_threshold: float = 0.5,
                       searchBox: Optional[BBox] = None, coarse_threshold: Optional[float] = None,
                       radius: Optional[int] = None, max_candidates: int = 256, context=None) -> List[Hit]:
    """
    Coarse-to-fine findMatches (pre-NMS hits, in findMatches' order).

    - factor           : integer >= 2, the downscale of the coarse level
    - coarse_threshold : what a coarse candidate must pass (default: score_threshold - 0.1 for methods 3 / 5,
                         + 0.1 for method 1; required for the raw-sum methods 2 and 4)
    - radius           : half-size of the full-resolution window around a candidate (default: factor)
    - max_candidates   : coarse candidates kept per template, best first
    - context          : an MTM._lib.Context to run on (default: the process's default context)
    Other arguments as in findMatches.  uint8 images and templates with 1 or 3 channels, methods 1..5, no masks.
    """
    raw, xOffset, yOffset = _raw_pyramid(listTemplates, image, factor, method, N_object, score_threshold, searchBox,
                                         coarse_threshold, radius, max_candidates, context)
    return _to_hit_list(raw, listTemplates, xOffset, yOffset)


def matchTemplatesPyramid(listTemplates: Sequence[TemplateTuple], image: np.ndarray, factor: int,
                          method: int = TM_CCOEFF_NORMED, N_object=float("inf"), score_threshold: float = 0.5,
                          maxOverlap: float = 0.25, searchBox: Optional[BBox] = None,
                          coarse_threshold: Optional[float] = None, radius: Optional[int] = None,
                          max_candidates: int = 256, context=None) -> List[Hit]:
    """
    Coarse-to-fine matchTemplates: findMatchesPyramid's hits through matchTemplates' non-maxima suppression.
    Arguments as in findMatchesPyramid and matchTemplates.  With N_object == 1 the best hit over the candidate windows -
    or no hit, when no template has a coarse candidate.
    """
    if maxOverlap < 0 or maxOverlap > 1:
        raise ValueError("Maximal overlap between bounding box is in range [0-1]")
    raw, xOffset, yOffset = _raw_pyramid(listTemplates, image, factor, method, N_object, score_threshold, searchBox,
                                         coarse_threshold, radius, max_candidates, context)
    kept = _nms_raw(raw, score_threshold, method == 1, N_object, maxOverlap)
    return _to_hit_list(kept, listTemplates, xOffset, yOffset)
