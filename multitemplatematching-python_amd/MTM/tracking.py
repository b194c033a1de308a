"""
Templates tracked through a stack of frames in one engine call: the loop a user writes today,

    out, boxes = [], [b for b, _ in tracks]
    for f in frames:
        r = findMatchesInBoxes(listTemplates, f, [(b, [j]) for b, (_, j) in zip(boxes, tracks)], method, N_object=1)
        out.append(r)
        boxes = [next_box(b, ri[0] if ri else None, margin, f.shape, method, min_score) for b, ri in zip(boxes, r)]

with the same hits, labels, boxes, float32 score bits, exceptions and warnings, computed by one native call
(mtm_track_boxes): the frames go up in chunks, and the next frame's search boxes are computed on the GPU from
this frame's hits, so the host waits once per call instead of twice per frame.

``refine=True`` returns every hit at its sub-pixel position, element ``[f][k]`` being exactly

    refineHits(listTemplates, frames[f], trackTemplates(..., refine=False)[f][k], method)

- ``[(label, (x + ox, y + oy, w, h), score)]`` with float ``x + ox``, ``y + oy`` - from the same native call
(mtm_track_boxes_nbhd): each frame's 3 x 3 score neighbourhoods are computed while the frame is on the device, and one
``subpixel.fit_offsets`` call fits them all.  The hit's template is the track's own ``listTemplates[j]``.  The refined
positions do not steer the tracks (the next box is ``next_box`` of the integer hit), a hit that fails ``min_score`` is
refined like any other, and the exceptions and warnings are those of the unrefined call.  ``positions`` turns either kind
of result into an (F, T, 2) array of trajectories.

``update=rate`` (0 < rate <= 1) gives every track a template of its own that follows its object's appearance: after each
frame whose hit passes (``next_box``' own rule), the track's template becomes ``blend_template(template, window, rate)``
of the hit's window in that frame.  Element ``[f][k]`` is exactly what this loop returns,

    cur, box = [listTemplates[j][1] for _, j in tracks], [b for b, _ in tracks]
    for f in frames:
        for k, (_, j) in enumerate(tracks):
            r = findMatchesInBoxes([(listTemplates[j][0], cur[k])], f, [box[k]], method, N_object=1)[0]
            hit = r[0]
            if <the hit passes: no min_score, or next_box' comparison of the score with it; NaN never passes>:
                x, y, w, h = hit[1]
                cur[k] = blend_template(cur[k], f[y:y + h, x:x + w], rate)
            box[k] = next_box(box[k], hit, margin, f.shape, method, min_score)

from one native call (mtm_track_boxes_adapt): the blend and the new template's statistics are computed on the device
between two frames' searches, in buffers of the call - the templates set on the context, a TemplateMatcher's resident
ones included, are never touched.  Two tracks of one ``listTemplates[j]`` diverge.  With ``refine=True`` frame f's hit is
refined with the template frame f was searched with.  ``return_templates=True`` returns ``(result, templates)``,
``templates[k]`` being track k's template after the last frame (copies of the originals without ``update``): a video
tracked in pieces carries on from them.

``reacquire=True`` (needs ``min_score``) recovers a track whose object left its box - a stage jump, a dropped frame, drift
during an occlusion: a hit that does not pass ``min_score`` is followed, in the same frame, by a search of the whole
frame for that track's template, and that search's hit is the frame's record.  Element ``[f][k]`` is exactly what this
loop returns,

    box = [b for b, _ in tracks]
    for f in frames:
        H, W = f.shape[:2]
        for k, (_, j) in enumerate(tracks):
            hit = findMatchesInBoxes(listTemplates, f, [(box[k], [j])], method, N_object=1)[0][0]
            if not <the hit passes min_score: next_box' comparison; NaN never passes>:
                hit = findMatchesInBoxes(listTemplates, f, [((0, 0, W, H), [j])], method, N_object=1)[0][0]
            out[f][k] = [hit]
            box[k] = next_box(box[k], hit, margin, f.shape, method, min_score)

from one native call (mtm_track_boxes_reacquire): the second search runs on the device for exactly the tracks that
failed, and the host never learns which they are.  The whole-frame map contains the box's map with the same score bits,
so a failed frame's record is the frame's global extremum for that template, the first in row-major order of the
whole-frame map on ties; if it fails too, the box stays where it was and the next frame tries again (``lost`` marks
those frames).  Frame 0 is a frame like any other: its errors and warnings are those of the loop's first call, the
whole-frame box always holds the template, so the second search raises nothing, and it emits no mask warning of its own
- the call warns as often as the call without ``reacquire``.  With ``refine=True`` the frame's final record is refined;
with ``update=rate`` the whole frame is searched with the track's own adapted template, and the track adopts the window
of its final record when that record passes.

A track is a pair ``((x, y, w, h), j)``: template ``listTemplates[j]``, searched in that box in frame 0 and around its
last hit afterwards (``next_box``).

A track may carry a *set* of templates instead - ``((x, y, w, h), js)`` with ``js`` a list, a tuple or a 1-D integer array
of indices into ``listTemplates`` (negative ones count from the end, duplicates are allowed): the appearances of one
object - rotations, flips, focus states -, all of one ``(h, w)``.  Every frame searches the whole set in the track's box,
and the frame's record is the best variant's, so its label says which appearance the object had.  Element ``[f][k]`` is
exactly what this loop returns,

    box = [b for b, _ in tracks]
    for f in frames:
        for k, (_, js) in enumerate(tracks):
            hits = findMatchesInBoxes(listTemplates, f, [(box[k], list(js))], method, N_object=1)[0]   # one per variant
            hit = (min if method in (0, 1) else max)(hits, key=lambda h: h[2])        # the first extreme one on ties
            out[f][k] = [hit]
            box[k] = next_box(box[k], hit, margin, f.shape, method, min_score)

from one native call (mtm_track_boxes_sets): the variants of a set share the box, so the kernel stages each tile's image
rows and forms the window sums once per group of variants.  An integer ``j`` is the set ``(j,)``, and both kinds of
track may be mixed in one call; a call without a set takes the code paths it took before sets existed.  With
``reacquire=True`` a winner that does not pass ``min_score`` is followed by the whole-frame search of the whole set,
reduced the same way; with ``refine=True`` the frame's final record is refined with the winner's template.  An empty
set, a set whose templates differ in ``(h, w)`` (the next box is derived from the winner's size) and ``update`` or
``return_templates=True`` together with a set raise ValueError after frame 0's own checks: adaptive sets are not built.

Scope (anything else raises before any native call): findMatchesInBoxes' scope with N_object=1 - uint8 frames with 1 or 3
channels or single-channel uint16 ones, methods 0..5, no masks for methods 0 and 3 - and frames of one shape and dtype,
``margin`` an integer >= 0.  Frame 0's boxes raise what the loop's first call raises; later boxes always hold their
template, so later frames raise nothing.
"""
import numbers
import warnings
from typing import List

import numpy as np

from . import _lib, boxes, subpixel
from . import _MSG_MASK_UNSUPPORTED, Hit, TM_CCOEFF_NORMED

__all__ = ["trackTemplates", "next_box", "blend_template", "positions", "lost"]


def next_box(box, hit, margin, image_shape, method, min_score=None):
    """The search box of the next frame from this frame's ``hit`` (a Hit, or None when the search returned none) in
    box ``box`` of an image of shape ``image_shape``: the hit's box widened by ``margin`` pixels on every side and clipped
    to the image, ``(x0, y0, x1 - x0, y1 - y0)`` with x0 = max(0, x - margin), y0 = max(0, y - margin),
    x1 = min(W, x + w + margin), y1 = min(H, y + h + margin).  ``box`` itself is returned when there is no hit, or when
    ``min_score`` is set and the hit's score does not pass it: methods 0 and 1 (minima) pass with score < min_score, the
    others with score > min_score, compared as Python floats; a NaN score never passes."""
    if hit is None:
        return tuple(box)
    if min_score is not None:
        s, m = float(hit[2]), float(min_score)
        if not (s < m if method in (0, 1) else s > m):
            return tuple(box)
    x, y, w, h = (int(v) for v in hit[1])
    H, W = int(image_shape[0]), int(image_shape[1])
    x0, y0 = max(0, x - margin), max(0, y - margin)
    x1, y1 = min(W, x + w + margin), min(H, y + h + margin)
    return (x0, y0, x1 - x0, y1 - y0)


def _blend_weight(rate, name="update"):
    """The window's weight in 256ths, a = round(256 rate), of a blend rate 0 < rate <= 1."""
    if not isinstance(rate, numbers.Real) or isinstance(rate, bool) or not 0 < rate <= 1:
        raise ValueError("%s must be a number in (0, 1] or None (got %r)" % (name, rate))
    a = int(round(rate * 256))
    if a == 0:
        raise ValueError("%s = %r is below the smallest step, 1 / 256 (it rounds to a weight of 0)" % (name, rate))
    return a


def blend_template(template, window, rate):
    """The template an adaptive track carries on with after a hit at ``window`` (the frame's pixels under the hit, of the
    template's shape and dtype, uint8 or uint16): with a = round(256 rate), 0 < rate <= 1,

        ((template * (256 - a) + window * a + 128) >> 8)

    in integers per pixel - the rounded blend, ``rate=1`` the window itself.  This is the definition of what
    ``trackTemplates(..., update=rate)`` computes on the device."""
    template, window = np.asarray(template), np.asarray(window)
    if template.dtype != window.dtype or template.dtype not in (np.uint8, np.uint16):
        raise ValueError("blend_template: template and window must both be uint8 or both uint16 (got %s and %s)" % (
            template.dtype, window.dtype))
    if template.shape != window.shape:
        raise ValueError("blend_template: template and window differ in shape (%s and %s)" % (template.shape, window.shape))
    a = _blend_weight(rate, "rate")
    return ((template.astype(np.int64) * (256 - a) + window.astype(np.int64) * a + 128) >> 8).astype(template.dtype)


def _frames(frames):
    """frames -> a list of arrays of one shape and dtype (an (F, H, W[, C]) array is split along its first axis)."""
    if isinstance(frames, np.ndarray):
        if frames.ndim not in (3, 4):
            raise ValueError("frames: an array of frames has the shape (F, H, W) or (F, H, W, C) (got %s)" % (frames.shape,))
        return list(frames)
    fl = list(frames)
    for i, f in enumerate(fl):
        if not isinstance(f, np.ndarray):
            raise ValueError("frames[%d] is not a numpy array" % i)
        if f.shape != fl[0].shape or f.dtype != fl[0].dtype:
            raise ValueError("frames[%d] differs from frames[0] in shape or dtype (%s %s, frames[0] %s %s)" % (
                i, f.shape, f.dtype, fl[0].shape, fl[0].dtype))
    return fl


def _check_args(margin, min_score, refine=False, update=None, return_templates=False, reacquire=False):
    if not isinstance(margin, numbers.Integral) or isinstance(margin, bool) or margin < 0:
        raise ValueError("margin must be an integer >= 0 (got %r)" % (margin,))
    if min_score is not None and (not isinstance(min_score, numbers.Real) or isinstance(min_score, bool)):
        raise ValueError("min_score must be a number or None (got %r)" % (min_score,))
    if not isinstance(refine, bool):
        raise ValueError("refine must be True or False (got %r)" % (refine,))
    if not isinstance(return_templates, bool):
        raise ValueError("return_templates must be True or False (got %r)" % (return_templates,))
    if not isinstance(reacquire, bool):
        raise ValueError("reacquire must be True or False (got %r)" % (reacquire,))
    if reacquire and min_score is None:
        raise ValueError("reacquire=True needs min_score: a track is searched again where its hit does not pass it")
    return None if update is None else _blend_weight(update)


def _originals(listTemplates, tracks):
    return [np.array(listTemplates[j][1]) for _, j in tracks]


_MSG_ADAPTIVE_SETS = "update and return_templates are not supported for tracks that carry a set of templates"


def _regions(tracks):
    """tracks -> (the regions the loop's findMatchesInBoxes calls take, whether some track carries a set, the first
    track whose set is an array that is not 1-D or None: its members reach the loop's checks flattened, and the track
    raises after them)."""
    regions, any_set, not_1d = [], False, None
    for b, j in tracks:                 # (the loop's unpacking of the pairs, and its errors)
        if isinstance(j, (list, tuple)) or (isinstance(j, np.ndarray) and j.ndim > 0):
            if isinstance(j, np.ndarray) and j.ndim != 1:
                if not_1d is None:
                    not_1d = len(regions)
                j = j.reshape(-1)
            regions.append((b, list(j)))
            any_set = True
        else:
            regions.append((b, [j]))
    return regions, any_set, not_1d


def _check_sets(listTemplates, tracks, reg, units, n_tracks, adaptive, not_1d):
    """The rules of set tracks, after the loop's own checks: (n_tracks + 1 offsets of the tracks' units) or ValueError."""
    if not_1d is not None:
        raise ValueError("tracks[%d]: a set of templates is a list, a tuple or a 1-D array of indices (got an array of "
                         "shape %s)" % (not_1d, tracks[not_1d][1].shape))
    counts = np.bincount(reg.u_region, minlength=n_tracks)
    if (counts == 0).any():
        raise ValueError("tracks[%d]: an empty set of templates" % int(np.argmax(counts == 0)))
    set_off = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    shp = np.array([listTemplates[j][1].shape[:2] for j in units["templ_idx"].tolist()], dtype=np.int64)
    differs = (shp != shp[np.repeat(set_off[:-1], counts)]).any(axis=1)
    if differs.any():
        u = int(np.argmax(differs))
        raise ValueError("tracks[%d]: the templates of a set must be of one (h, w) (template '%s' is %s, the set's first %s)"
                         % (int(reg.u_region[u]), listTemplates[int(units["templ_idx"][u])][0], tuple(shp[u].tolist()),
                            tuple(shp[set_off[reg.u_region[u]]].tolist())))
    if adaptive:
        raise ValueError(_MSG_ADAPTIVE_SETS)
    return set_off


def _track(listTemplates, frames, tracks, margin, method, min_score, ctx, resident, refine=False, update=None,
           return_templates=False, reacquire=False):
    """trackTemplates on `ctx`.  `resident`: the context holds every template of listTemplates in list order
    (TemplateMatcher); otherwise the templates the tracks use are set now.  Returns (hits per frame and track, the first
    frame or None, whether templates were set on the context, every track's last template or None)."""
    fl = _frames(frames)
    a = _check_args(margin, min_score, refine, update, return_templates, reacquire)
    regions, any_set, not_1d = _regions(tracks)
    if not fl:
        if any_set and (a is not None or return_templates):
            raise ValueError(_MSG_ADAPTIVE_SETS)
        return [], None, False, (_originals(listTemplates, tracks) if return_templates else None)
    if not regions:
        return [[] for _ in fl], fl[0], False, ([] if return_templates else None)
    f0 = fl[0]
    if resident and method in boxes._SCOPE_METHODS:       # every resident template is in scope
        boxes._check_scope(listTemplates, f0, range(len(listTemplates)), method, boxes._SCOPE_METHODS)
    # frame 0's errors and warnings, as the loop's first call raises and emits them
    reg, units = boxes._plan(listTemplates, f0, regions, method, 1, boxes._SCOPE_METHODS)
    set_off = None
    if any_set:
        set_off = _check_sets(listTemplates, tracks, reg, units, len(regions), a is not None or return_templates,
                              not_1d)
    if method not in (0, 3) and len(fl) > 1:        # the mask warnings of the loop's later calls
        n_warn = sum(1 for j in units["templ_idx"].tolist() if len(listTemplates[j]) >= 3)
        for _ in range(n_warn * (len(fl) - 1)):
            warnings.warn(_MSG_MASK_UNSUPPORTED)
    if resident:
        used = None
        templates = [(t[1], None) for t in listTemplates]
    else:
        used = np.unique(units["templ_idx"])
        units = units.copy()
        units["templ_idx"] = np.searchsorted(used, units["templ_idx"])
        templates = [(listTemplates[j][1], None) for j in used.tolist()]
    # (a margin past the frame's larger side clips to the whole frame, as a margin of that side does)
    m = int(min(margin, max(f0.shape[0], f0.shape[1])))
    ctx = ctx or _lib.default_context()         # (only now: every argument error comes before "no GPU")
    with ctx.lock:
        ctx.set_templates(templates, method)
        last = None
        if any_set:         # (one unit per track and variant; the record names the variant that won its frame)
            raw, nbhd = ctx.track_boxes_sets(fl, units[set_off[:-1]], set_off, units["templ_idx"], m, min_score, reacquire,
                                             refine)
        elif reacquire:       # (one binding method for every composition: a weight of 0 is no adaptation)
            raw, nbhd, last, _ = ctx.track_boxes_reacquire(fl, units, m, min_score, a or 0, [t[0] for t in templates],
                                                           refine)
        elif a is not None:
            raw, nbhd, last, _ = ctx.track_boxes_adapt(fl, units, m, min_score, a, [t[0] for t in templates], refine)
        elif refine:
            raw, nbhd = ctx.track_boxes_nbhd(fl, units, m, min_score)
        else:
            raw = ctx.track_boxes(fl, units, m, min_score)
    tidx = raw["templ_idx"] if used is None else used[raw["templ_idx"]]
    labels = boxes._labels(listTemplates)
    xywh = zip(raw["x"].tolist(), raw["y"].tolist(), raw["w"].tolist(), raw["h"].tolist())
    hits = list(zip(labels[tidx].tolist(), xywh, list(raw["score"])))
    if refine:          # (one fit over every record: refineHits' numbers by construction)
        hits = subpixel._refined(hits, nbhd, method)
    T = len(regions)
    if return_templates and last is None:
        last = _originals(listTemplates, tracks)
    return [[[hits[f * T + k]] for k in range(T)] for f in range(len(fl))], f0, True, (last if return_templates else None)


def trackTemplates(listTemplates, frames, tracks, margin: int, method: int = TM_CCOEFF_NORMED, min_score=None, *,
                   refine: bool = False, update=None, return_templates: bool = False, reacquire: bool = False,
                   context=None):
    """
    Follow each track through ``frames`` (a sequence of arrays of one shape and dtype, or one ``(F, H, W[, C])`` array):
    element ``[f][k]`` is what ``findMatchesInBoxes(listTemplates, frames[f], ..., method, N_object=1)`` returns for track
    k - ``[hit]`` - in the loop of this module's docstring, where each frame's search box is ``next_box`` of the previous
    frame's hit.  ``tracks``: pairs ``((x, y, w, h), j)``, template ``listTemplates[j]`` starting from that box in frame
    0, or ``((x, y, w, h), js)`` with a set of same-shape templates ``[listTemplates[j] for j in js]``, of which each frame's
    best one gives the record and its label (the module's docstring).  ``min_score``: a hit that does not pass it (``next_box``) leaves its track's box where it was.  ``refine``
    (True / False): every hit at its sub-pixel position, ``refineHits(listTemplates, frames[f], [hit], method)`` of the
    unrefined call's hit, from the same native call (the module's docstring).  ``update`` (None, or a rate in (0, 1]):
    every track adapts a template of its own, ``blend_template(template, hit's window, update)`` after each frame whose
    hit passes (the module's docstring); ``return_templates=True`` returns ``(result, templates)`` with every track's
    template after the last frame.  ``reacquire`` (True / False; True needs ``min_score``): a track whose hit does not
    pass ``min_score`` is searched again in the same frame over the whole frame, and that search's hit is the frame's
    record - and the track's new position when it passes (the module's docstring).  ``context``: the _lib.Context to run
    on (default: the process's).
    """
    r = _track(listTemplates, frames, tracks, margin, method, min_score, context, False, refine, update, return_templates,
               reacquire)
    return (r[0], r[3]) if return_templates else r[0]


def positions(result) -> np.ndarray:
    """The trajectories of a trackTemplates / TemplateMatcher.track result, refined or not: an (F, T, 2) float64 array,
    element ``[f, k]`` the ``(x, y)`` of track k's hit in frame f.  ValueError when some ``[f][k]`` does not hold exactly
    one hit, or when the frames differ in their number of tracks."""
    result = list(result)
    n_tracks = len(result[0]) if result else 0
    out = np.empty((len(result), n_tracks, 2), dtype=np.float64)
    for f, row in enumerate(result):
        if len(row) != n_tracks:
            raise ValueError("positions: frame %d holds %d tracks, frame 0 holds %d" % (f, len(row), n_tracks))
        for k, hits in enumerate(row):
            if len(hits) != 1:
                raise ValueError("positions: frame %d, track %d holds %d hits, not one" % (f, k, len(hits)))
            out[f, k, 0], out[f, k, 1] = hits[0][1][0], hits[0][1][1]
    return out


def lost(result, method, min_score) -> np.ndarray:
    """Where a trackTemplates / TemplateMatcher.track result, refined or not, lost its object: an (F, T) bool array,
    element ``[f, k]`` true where track k's hit in frame f does not pass ``min_score`` by ``next_box``' rule (methods 0
    and 1 pass with score < min_score, the others with score > min_score, as Python floats; a NaN score never passes).
    Without ``reacquire`` these are the frames whose box was kept; with ``reacquire=True`` they are the frames in which
    the object was found nowhere in the frame.  ValueError as ``positions`` raises it."""
    if not isinstance(min_score, numbers.Real) or isinstance(min_score, bool):
        raise ValueError("min_score must be a number (got %r)" % (min_score,))
    result = list(result)
    n_tracks = len(result[0]) if result else 0
    out = np.empty((len(result), n_tracks), dtype=bool)
    m = float(min_score)
    for f, row in enumerate(result):
        if len(row) != n_tracks:
            raise ValueError("lost: frame %d holds %d tracks, frame 0 holds %d" % (f, len(row), n_tracks))
        for k, hits in enumerate(row):
            if len(hits) != 1:
                raise ValueError("lost: frame %d, track %d holds %d hits, not one" % (f, k, len(hits)))
            s = float(hits[0][2])
            out[f, k] = not (s < m if method in (0, 1) else s > m)
    return out
