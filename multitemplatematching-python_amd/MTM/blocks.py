"""
Block matching between two images in one engine call: the displacement of every block of ``reference`` in ``image`` -
drift and stage-shift estimation, registration of stitching overlaps, PIV-style displacement fields, "where did every
patch of frame n go in frame n + 1".  The loop a user writes today,

    for k, (x, y, w, h) in enumerate(blocks):
        hit, = findMatchesInBoxes([("b", reference[y:y + h, x:x + w])], image, [search_box((x, y, w, h), margin, image.shape)],
                                  method, N_object=1)[0]
        positions[k], scores[k] = hit[1][:2], hit[2]

with the same positions and float32 score bits, computed by one native call (mtm_match_blocks): both images
are uploaded once, and the templates never exist on the host - a kernel cuts every block out of the uploaded reference
and computes its constants on the device.  The search box of a block is the block's own box widened by ``margin`` pixels
on every side and clipped to the image (``search_box``; ``MTM.tracking.next_box`` of the block taken as a hit).  Ties go
to the first output in row-major order of the box's map; a flat block under TM_CCOEFF_NORMED scores 1.0 everywhere and
lands on the box's first output; ``margin=0`` gives a 1 x 1 map.

``refine=True`` returns float64 positions, element k being exactly

    refineHits([("b", reference[y:y + h, x:x + w])], image, [hit_k], method)[0][1][:2]

from the same native call: the 3 x 3 neighbourhood of every hit in the whole image's score map (NaN outside it), fitted
by one ``subpixel.fit_offsets`` call for all blocks.  The scores stay the unrefined ones.

Results are numpy arrays, not hit tuples.  The call leaves the templates set on its context - a TemplateMatcher's resident
ones included - exactly as it found them.

Scope (anything else raises ValueError / TypeError before any native call): two images of one shape, dtype and channel
count - uint8 with 1 or 3 channels or single-channel uint16, at most 32767 rows -, methods 0..5, blocks wholly inside the
reference, uint16 blocks of at most 2^21 pixels, ``margin`` an integer >= 0.

``matchBlocks(..., offsets=)`` centres every block's box on a predicted displacement (``search_box_at``), and
``matchBlocksMultipass`` is the coarse-to-fine scheme built on it (mtm_match_blocks_passes): a sparse pass
with a wide margin finds the large motion, every later pass searches a small margin around what the nearest block of the
pass before found (``predict_offsets``) - one native call, the boxes of the later passes computed on the device.
``validate=`` runs the normalised median test (``validate``) over every pass's displacements on the device before they
steer the next pass: a coarse block that matched wrongly - a flat, periodic or occluded patch - is steered by its
neighbours' median instead of misleading every fine block nearest to it.

``second=`` (``matchBlocks``, ``matchBlocksMultipass``) adds every block's second correlation peak - the best output of the
block's map outside a small exclusion window around the first - from the same native call (mtm_match_blocks_second, DESIGN
5.6.3); ``peak_ratio`` of the two is the vector's signal-to-noise, which tells a unique match from a periodic texture, a
flat patch or an occluded block.  ``second_peaks`` states the rule in numpy, for ensemble planes.

``matchBlocksMultipass(deform=True)`` adds window deformation between the passes (mtm_match_blocks_passes_deformed, DESIGN
5.6.4): a later pass does not just move every block's box, it warps the whole original image back by the displacement
field interpolated from the pass before (``displacement_field``: bilinear between the coarse blocks' centres, Q8 integers;
``deform``: the bilinear warp, integers again) and searches the blocks in the warped image, so that a block under shear,
rotation or strain still meets a window shaped like itself; ``field_at`` is the field at the blocks' centres, which the
pass adds to what it finds.  All on the device, one native call; the three helpers state the rule in numpy, bit for bit.
``deformImage`` is the warp by itself on the device (mtm_deform_image): how a frame is registered once its drift field
is known.  ``steer="refined"`` steers every deformed pass by the pass before's SUB-PIXEL positions (``to_q8``), filtered by
a 3 x 3 binomial kernel over the grid (``smooth_displacements``), instead of by its integer records: what makes deformation
worth iterating on the final grid.

``matchBlocks(..., mask=)`` takes a static mask over the reference - channel walls, a solid body in the flow, a reticle, a
timestamp, a dead sensor region: an (H, W) bool or uint8 array, non-zero = the pixel takes part (mtm_match_blocks_masked,
DESIGN 5.6.5).  Every block is then matched as the masked template ``(reference[y:y + h, x:x + w], mask[y:y + h, x:x + w])``
- uint8 images, methods 0 and 3, the package's masked methods -, the block and its mask cut on the device; a block whose
mask keeps no pixel, or whose map holds no number, comes back as position ``(-1, -1)`` and score NaN.  ``mask_fraction``
gives the share of every block the mask keeps, to drop blocks that are mostly masked.  Not built: ``mask=`` in
``matchBlocksMultipass`` and ``matchBlocksStack`` (a masked multipass can be written by hand with ``matchBlocks(mask=,
offsets=)`` and ``predict_offsets``), masks with uint16 or float32 images, masked methods other than 0 and 3.

``matchBlocksStack`` is the movie form: the pairs of a stack of frames - each frame against the previous or against the
first - in one native call (mtm_match_blocks_stack), every frame uploaded once; per pair the very results of
``matchBlocks``, or (``ensemble=True``) every block's correlation plane averaged over the pairs and its peak
(``plane_peaks``): ensemble correlation, for movies whose single pairs are too noisy to peak.  ``offsets=`` centres every
block's box on a predicted displacement shared by the pairs (mtm_match_blocks_stack_at), the planes then lying around the
moved blocks (``moved_blocks``), and ``matchBlocksStackMultipass`` is the coarse-to-fine scheme over a movie
(mtm_match_blocks_stack_passes): per pair the passes of ``matchBlocksMultipass``, or - ``ensemble=True`` -
passes whose ensemble peaks steer the next, what micro-PIV runs on movies whose single pairs are too noisy to peak.
"""
import numbers

import numpy as np

from . import _lib, subpixel
from . import TM_CCOEFF_NORMED

__all__ = ["matchBlocks", "matchBlocksStack", "matchBlocksMultipass", "matchBlocksStackMultipass", "moved_blocks", "plane_peaks", "grid", "search_box", "search_box_at",
           "predict_offsets", "displacements", "grid_shape", "validate", "second_peaks", "peak_ratio", "displacement_field",
           "field_at", "deform", "deformImage", "to_q8", "smooth_displacements", "mask_fraction"]

_I64 = np.dtype(np.int64)
_U16_MAX_PIXELS = 1 << 21       # mtm_match_blocks: uint16 correlations stay below 2^53, exact in float64
_MAX_ROWS = 32767               # the two images are uploaded as one stack of at most 65535 rows


def _is_int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, (bool, np.bool_))


def search_box(block, margin, shape):
    """The search box ``(x0, y0, bw, bh)`` of ``block = (x, y, w, h)`` in an image of shape ``shape``: the block's box
    widened by ``margin`` pixels on every side and clipped to the image -
    ``MTM.tracking.next_box(None, (None, block, 0), margin, shape, method)``."""
    x, y, w, h = (int(v) for v in block)
    H, W = int(shape[0]), int(shape[1])
    x0, y0 = max(0, x - margin), max(0, y - margin)
    x1, y1 = min(W, x + w + margin), min(H, y + h + margin)
    return (x0, y0, x1 - x0, y1 - y0)


def search_box_at(block, offset, margin, shape):
    """``search_box`` of ``block = (x, y, w, h)`` moved by ``offset = (dx, dy)``: the position is moved and clamped so
    that the block still lies inside the image - ``cx = min(max(x + dx, 0), W - w)``, ``cy`` likewise -, and the result
    is ``search_box((cx, cy, w, h), margin, shape)``.  A zero offset gives ``search_box(block, ...)``; the box's map is
    never empty, whatever the offset."""
    x, y, w, h = (int(v) for v in block)
    dx, dy = (int(v) for v in offset)
    H, W = int(shape[0]), int(shape[1])
    cx, cy = min(max(x + dx, 0), W - w), min(max(y + dy, 0), H - h)
    return search_box((cx, cy, w, h), margin, shape)


def moved_blocks(blocks, offsets, shape):
    """Where ``offsets`` move ``blocks`` in an image of shape ``shape``: an (N, 4) int64 array of ``(cx, cy, w, h)``, the
    position of every block moved by its ``(dx, dy)`` and clamped so that the block still lies inside the image, ``cx =
    min(max(x + dx, 0), W - w)`` and ``cy`` likewise - the block ``search_box_at`` widens, and the block the planes of
    ``matchBlocksStack(ensemble=True, offsets=)`` lie around.  ``blocks`` and ``offsets`` as ``matchBlocks`` takes them."""
    b = _check_blocks(blocks, np.empty((int(shape[0]), int(shape[1])), np.uint8))
    out = b.copy()
    out[:, :2] += _check_offsets(offsets, b, shape)
    return out


def _pair(v, what, who="grid"):
    try:
        p = (v, v) if _is_int(v) else tuple(v)
    except TypeError:
        p = ()
    if len(p) != 2 or not all(_is_int(q) for q in p) or min(p) < 1:
        raise ValueError("%s: %s must be a positive integer or a pair of them (got %r)" % (who, what, v))
    return int(p[0]), int(p[1])


def _grid_axes(shape, block, step, who="grid"):
    """(w, h, sx, sy, nx, ny) of ``grid(shape, block, step)``."""
    w, h = _pair(block, "block", who)
    sx, sy = (w, h) if step is None else _pair(step, "step", who)
    H, W = int(shape[0]), int(shape[1])
    return w, h, sx, sy, ((W - w) // sx + 1 if W >= w else 0), ((H - h) // sy + 1 if H >= h else 0)


def grid(shape, block, step=None):
    """Every block of size ``block`` (an int, or ``(w, h)``) at stride ``step`` (an int or ``(sx, sy)``; default: the
    block size) that lies wholly inside an image of shape ``shape``, in row-major order: an (N, 4) int64 array of
    ``(x, y, w, h)``."""
    w, h, sx, sy, nx, ny = _grid_axes(shape, block, step)
    out = np.empty((ny * nx, 4), dtype=_I64)
    out[:, 0] = np.tile(np.arange(0, nx * sx, sx, dtype=_I64), ny)
    out[:, 1] = np.repeat(np.arange(0, ny * sy, sy, dtype=_I64), nx)
    out[:, 2] = w
    out[:, 3] = h
    return out


def grid_shape(shape, block, step=None):
    """``(ny, nx)``: the rows and columns of blocks of ``grid(shape, block, step)`` (block ``iy * nx + ix`` is in row iy
    and column ix)."""
    _, _, _, _, nx, ny = _grid_axes(shape, block, step, "grid_shape")
    return ny, nx


def _check_validate_params(threshold, epsilon, who):
    for name, v in (("threshold", threshold), ("epsilon", epsilon)):
        if not isinstance(v, numbers.Real) or isinstance(v, (bool, np.bool_)) or not np.isfinite(v) or v < 0:
            raise ValueError("%s: %s must be a finite number >= 0 (got %r)" % (who, name, v))
    return float(threshold), float(epsilon)


_NEIGHBOURS = tuple((oy, ox) for oy in (-1, 0, 1) for ox in (-1, 0, 1) if (oy, ox) != (0, 0))


def _doubled_median(values, present, n):
    """Along axis 0: s[(n - 1) // 2] + s[n // 2] of the sorted ``values`` that are ``present`` (n >= 1 of them)."""
    s = np.sort(np.where(present, values, np.iinfo(np.int64).max), axis=0)
    return (np.take_along_axis(s, ((n - 1) // 2)[None], axis=0) + np.take_along_axis(s, (n // 2)[None], axis=0))[0]


def validate(grid_shape, displacements, threshold=2.0, epsilon=0.5):
    """The normalised median test (Westerweel & Scarano) over a displacement field, in plain numpy - the rule
    ``matchBlocksMultipass(validate=)`` runs on the device between its passes (mtm_blocks_validate.h).
    ``grid_shape``: ``(ny, nx)``; ``displacements``: the integer (ny * nx, 2) ``(dx, dy)`` of the grid's blocks in
    row-major order.  Returns ``(valid, replaced)``: ``valid`` bool (N,), and ``replaced`` int64 (N, 2), the input with
    every outlier's row substituted.

    The neighbours of a block are the blocks of its 3 x 3 grid neighbourhood that exist, without the block itself; a
    block with fewer than 3 of them is valid (every block of a 1 x n or n x 1 grid).  Per component u over the n >= 3
    neighbour values, in integers: ``m2 = dmed(u_i)`` with ``dmed(s) = s[(n - 1) // 2] + s[n // 2]`` of the sorted
    values (the doubled median), ``r_i = |2 u_i - m2|``, ``rm4 = dmed(r_i)``; the block is an outlier in the component iff
    ``float64(2 |2 u_0 - m2|) > threshold * (float64(rm4) + 4.0 * epsilon)``.  A block is invalid if either component is
    an outlier, and its row becomes ``((m2x + 1) >> 1, (m2y + 1) >> 1)``: the neighbours' median, rounded half towards
    +infinity.  Only the input is read - neighbours that are outliers themselves count as they are, nothing is iterated.

    The defaults are for integer fields: in a uniform neighbourhood (rm4 = 0) a deviation of 1 px passes (4 > 4 is
    false) and 2 px is flagged; a sub-pixel epsilon such as 0.1 would flag every 1-px step.  Float displacements raise
    TypeError (refined positions never steer a pass); bad shapes and a negative or non-finite threshold or epsilon raise
    ValueError.
    """
    try:
        ny, nx = grid_shape
    except (TypeError, ValueError):
        raise ValueError("validate: grid_shape must be (ny, nx) (got %r)" % (grid_shape,)) from None
    if not _is_int(ny) or not _is_int(nx) or ny < 0 or nx < 0:
        raise ValueError("validate: grid_shape must be two integers >= 0 (got %r)" % (grid_shape,))
    ny, nx = int(ny), int(nx)
    threshold, epsilon = _check_validate_params(threshold, epsilon, "validate")
    d = np.asarray(displacements)
    if d.ndim != 2 or d.shape[1] != 2 or len(d) != ny * nx:
        raise ValueError("validate: displacements of shape %s for a grid of %d x %d blocks (expected (%d, 2))" % (
            d.shape, ny, nx, ny * nx))
    if d.dtype.kind not in "iu":
        raise TypeError("validate: displacements must be integers (got %s): refined positions never steer a pass" % d.dtype)
    d = d.astype(_I64)
    if ny * nx == 0:
        return np.zeros(0, bool), d
    u0 = d.reshape(ny, nx, 2)
    values = np.zeros((8, ny, nx, 2), _I64)
    present = np.zeros((8, ny, nx, 1), bool)
    for j, (oy, ox) in enumerate(_NEIGHBOURS):
        ys, xs = slice(max(0, -oy), ny - max(0, oy)), slice(max(0, -ox), nx - max(0, ox))
        yn, xn = slice(max(0, oy), ny - max(0, -oy)), slice(max(0, ox), nx - max(0, -ox))
        values[j, ys, xs] = u0[yn, xn]
        present[j, ys, xs] = True
    n = present.sum(axis=0)
    tested = n >= 3
    n = np.maximum(n, 1)
    m2 = np.where(tested, _doubled_median(values, present, n), 0)
    rm4 = np.where(tested, _doubled_median(np.abs(2 * values - m2), present, n), 0)
    lhs = (2 * np.abs(2 * u0 - m2)).astype(np.float64)
    with np.errstate(over="ignore"):
        rhs = np.float64(threshold) * (rm4.astype(np.float64) + np.float64(4.0 * epsilon))
    valid = ~(tested & (lhs > rhs)).any(axis=2)
    replaced = np.where(valid[:, :, None], u0, (m2 + 1) >> 1)
    return valid.reshape(-1), replaced.reshape(-1, 2)


def _nearest(n, s, wc, x, wf):
    """Per axis: the index of the coarse block (size wc, stride s, n of them) whose centre is nearest to that of every
    fine block of size wf at x, on doubled centres; an exact tie goes to the higher index (blocks_nearest_inl,
    mtm_blocks_predict.h)."""
    return np.minimum(n - 1, np.maximum(0, 2 * x + wf - wc + s) // (2 * s))


def predict_offsets(shape, coarse, positions, fine):
    """The displacements a coarse pass predicts for the blocks of a finer one.  ``coarse`` and ``fine``: ``(block, step)``
    as ``grid`` takes them; ``positions``: the integer (Nc, 2) positions found for ``grid(shape, *coarse)``.  Returns an
    (Nf, 2) int64 array: for every block of ``grid(shape, *fine)`` the displacement ``positions - blocks[:, :2]`` of the
    coarse block whose centre is nearest - per axis ``i = min(n - 1, max(0, 2 x + wf - wc + s) // (2 s))`` for a coarse
    axis of n blocks of size wc at stride s and a fine block of size wf at x; an exact tie goes to the higher index."""
    try:
        (cb, cs), (fb, fs) = coarse, fine
    except (TypeError, ValueError):
        raise ValueError("predict_offsets: coarse and fine are (block, step) pairs (got %r and %r)" % (coarse, fine)) from None
    wc, hc, sx, sy, nx, ny = _grid_axes(shape, cb, cs, "predict_offsets")
    fg = grid(shape, fb, fs)
    pos = np.asarray(positions)
    if pos.ndim != 2 or pos.shape[1] != 2 or len(pos) != nx * ny:
        raise ValueError("predict_offsets: positions of shape %s for a coarse grid of %d blocks (expected (%d, 2))" % (
            pos.shape, nx * ny, nx * ny))
    if pos.dtype.kind not in "iu":
        raise TypeError("predict_offsets: positions must be integers (got %s): refined positions never steer a pass" % pos.dtype)
    if len(fg) == 0:
        return np.zeros((0, 2), _I64)
    if nx * ny == 0:
        raise ValueError("predict_offsets: the coarse grid is empty")
    pos = pos.astype(_I64)
    ix = _nearest(nx, sx, wc, fg[:, 0], fg[:, 2])
    iy = _nearest(ny, sy, hc, fg[:, 1], fg[:, 3])
    return pos[iy * nx + ix] - np.stack((ix * sx, iy * sy), axis=1)


_DEFORM_MAX = 1 << 22           # mtm_blocks_deform.h: the largest |displacement| the field takes


def _deform_axis(n, s, wc, X2):
    """Per axis of n coarse blocks of size wc at stride s: (i, a8) at the doubled coordinates X2 - the lower node and the
    weight (0 .. 256) of node min(i + 1, n - 1) (deform_axis_inl, mtm_blocks_deform.h)."""
    X2 = np.asarray(X2, dtype=_I64)
    if n <= 1:
        return np.zeros(X2.shape, _I64), np.zeros(X2.shape, _I64)
    i = np.clip((X2 - (wc - 1)) // (2 * s), 0, n - 2)
    a = np.clip(X2 - (2 * i * s + wc - 1), 0, 2 * s)
    return i, (256 * a + s) // (2 * s)


def _deform_args(shape, coarse, displacements, who, q8=False):
    """(wc, hc, sx, sy, nx, ny, d): the coarse grid's axes and its displacements as an (ny, nx, 2) int64 array.  ``q8``: the
    displacements are in Q8 (the same limit of 2^22 pixels)."""
    _check_flag(q8, "q8")
    top = _DEFORM_MAX << 8 if q8 else _DEFORM_MAX
    try:
        cb, cs = coarse
    except (TypeError, ValueError):
        raise ValueError("%s: coarse is a (block, step) pair (got %r)" % (who, coarse)) from None
    wc, hc, sx, sy, nx, ny = _grid_axes(shape, cb, cs, who)
    d = np.asarray(displacements)
    if d.ndim != 2 or d.shape[1] != 2 or len(d) != nx * ny:
        raise ValueError("%s: displacements of shape %s for a coarse grid of %d blocks (expected (%d, 2))" % (
            who, d.shape, nx * ny, nx * ny))
    if d.dtype.kind not in "iu":
        raise TypeError("%s: displacements must be integers (got %s): refined positions never steer a pass" % (who, d.dtype))
    if nx * ny == 0:
        raise ValueError("%s: the coarse grid is empty" % who)
    if d.dtype.kind == "u":
        d = np.minimum(d, np.uint64(top + 1))
    d = d.astype(_I64)
    if np.abs(d).max() > top:
        raise ValueError("%s: displacements beyond 2^22 pixels are not supported" % who)
    return wc, hc, sx, sy, nx, ny, d.reshape(ny, nx, 2)


def _field(d, ix, ax, iy, ay, q8=False):
    """The Q8 field from the nodes d (ny, nx, 2) at lower nodes (iy, ix) with weights (ay, ax), broadcast together; ``q8``:
    the nodes are in Q8 themselves."""
    ny, nx = d.shape[:2]
    ix1, iy1 = np.minimum(ix + 1, nx - 1), np.minimum(iy + 1, ny - 1)
    ax, ay = ax[..., None], ay[..., None]
    acc = (d[iy, ix] * (256 - ax) * (256 - ay) + d[iy, ix1] * ax * (256 - ay) + d[iy1, ix] * (256 - ax) * ay
           + d[iy1, ix1] * ax * ay)
    return (acc + 32768) >> 16 if q8 else (acc + 128) >> 8


def displacement_field(shape, coarse, displacements, q8=False):
    """The per-pixel displacement field a coarse grid's displacements give, (H, W, 2) int64 of (Fx, Fy) in Q8 (1/256 px) -
    the field ``matchBlocksMultipass(deform=True)`` warps by, in plain numpy.  ``coarse``: ``(block, step)`` as ``grid``
    takes them; ``displacements``: the integer (Nc, 2) ``(dx, dy)`` of ``grid(shape, *coarse)`` in row-major order.

    The rule (mtm_blocks_deform.h), in integers on DOUBLED coordinates - pixel x is ``X2 = 2 x``, the centre of a block at
    x of width w is ``2 x + w - 1``, the centre of coarse column i is ``Cx_i = 2 i sx + wc - 1``.  Per axis (nx == 1: ``i =
    0, ax = 0``): ``i = clamp((X2 - (wc - 1)) // (2 sx), 0, nx - 2)``, ``a = clamp(X2 - Cx_i, 0, 2 sx)``, ``ax = (256 a +
    sx) // (2 sx)`` in 0..256 - constant extrapolation outside the centres' hull -, ``i1 = min(i + 1, nx - 1)``; ``j, ay,
    j1`` likewise.  Per component, in int64, the shift a floor:

        F = (d[j,i] (256-ax)(256-ay) + d[j,i1] ax (256-ay) + d[j1,i] (256-ax) ay + d[j1,i1] ax ay + 128) >> 8

    ``q8=True``: the integer displacements are themselves in Q8 (sub-pixel nodes ``S``, ``|S| <= 2^30``), and

        F = (S[j,i] (256-ax)(256-ay) + S[j,i1] ax (256-ay) + S[j1,i] (256-ax) ay + S[j1,i1] ax ay + 32768) >> 16

    which for ``S = 256 d`` is the field of ``d``, bit for bit.

    Float displacements raise TypeError, a wrong length (or one beyond 2^22 pixels) ValueError."""
    wc, hc, sx, sy, nx, ny, d = _deform_args(shape, coarse, displacements, "displacement_field", q8)
    H, W = int(shape[0]), int(shape[1])
    ix, ax = _deform_axis(nx, sx, wc, 2 * np.arange(W, dtype=_I64))
    iy, ay = _deform_axis(ny, sy, hc, 2 * np.arange(H, dtype=_I64))
    return _field(d, ix[None, :], ax[None, :], iy[:, None], ay[:, None], q8)


def field_at(shape, coarse, displacements, blocks, q8=False):
    """``displacement_field``'s rule at the doubled centres ``(2 x + w - 1, 2 y + h - 1)`` of ``blocks`` ((N, 4) integers
    of ``(x, y, w, h)``): (N, 2) int64 in Q8 - what a deformed pass adds to what it finds in the warped image.  ``q8``:
    as ``displacement_field``'s."""
    wc, hc, sx, sy, nx, ny, d = _deform_args(shape, coarse, displacements, "field_at", q8)
    b = np.asarray(blocks)
    if b.size == 0:
        return np.zeros((0, 2), _I64)
    if b.ndim != 2 or b.shape[1] != 4 or b.dtype.kind not in "iu":
        raise ValueError("field_at: blocks must be an (N, 4) integer array of (x, y, w, h)")
    b = b.astype(_I64)
    ix, ax = _deform_axis(nx, sx, wc, 2 * b[:, 0] + b[:, 2] - 1)
    iy, ay = _deform_axis(ny, sy, hc, 2 * b[:, 1] + b[:, 3] - 1)
    return _field(d, ix, ax, iy, ay, q8)


def to_q8(positions):
    """Positions (or displacements) in pixels as int64 in Q8 (1/256 px): ``floor(256.0 * p + 0.5)`` in float64 - how a
    steered call (``matchBlocksMultipass(steer="refined")``) takes the refined positions of ``matchBlocks(refine=True)``.
    Integers give ``256 * p`` exactly; values that are not finite or beyond 2^22 pixels raise ValueError."""
    p = np.asarray(positions)
    if p.dtype.kind in "iu":
        p = p.astype(_I64)
        if p.size and np.abs(p).max() > _DEFORM_MAX:
            raise ValueError("to_q8: positions beyond 2^22 pixels are not supported")
        return 256 * p
    if p.dtype.kind != "f":
        raise TypeError("to_q8: positions must be numbers (got %s)" % p.dtype)
    p = p.astype(np.float64)
    if p.size and not (np.abs(p) <= _DEFORM_MAX).all():
        raise ValueError("to_q8: positions must be finite and within 2^22 pixels")
    return np.floor(256.0 * p + 0.5).astype(_I64)


def smooth_displacements(grid_shape, d):
    """The predictor filter of a steered call, in plain numpy: the (ny * nx, 2) integer displacements ``d`` of a
    ``grid_shape`` = ``(ny, nx)`` grid in row-major order filtered by the 3 x 3 binomial kernel, per component in int64:

        S[j,i] = (sum over u, v in {-1, 0, 1} of k[u] k[v] d[clamp(j + u, 0, ny - 1), clamp(i + v, 0, nx - 1)] + 8) >> 4

    with ``k = (1, 2, 1)`` and an arithmetic shift (a floor).  Only the input is read.  A constant field comes back
    unchanged, a 1 x 1 grid is the identity.  Returns (N, 2) int64.  Float displacements raise TypeError; values beyond
    2^30 (2^22 pixels in Q8) and bad shapes ValueError."""
    try:
        ny, nx = grid_shape
    except (TypeError, ValueError):
        raise ValueError("smooth_displacements: grid_shape must be (ny, nx) (got %r)" % (grid_shape,)) from None
    if not _is_int(ny) or not _is_int(nx) or ny < 0 or nx < 0:
        raise ValueError("smooth_displacements: grid_shape must be two integers >= 0 (got %r)" % (grid_shape,))
    ny, nx = int(ny), int(nx)
    a = np.asarray(d)
    if a.ndim != 2 or a.shape[1] != 2 or len(a) != ny * nx:
        raise ValueError("smooth_displacements: displacements of shape %s for a grid of %d x %d blocks (expected (%d, 2))" % (
            a.shape, ny, nx, ny * nx))
    if a.dtype.kind not in "iu":
        raise TypeError("smooth_displacements: displacements must be integers (got %s): to_q8 makes them" % a.dtype)
    if a.dtype.kind == "u":
        a = np.minimum(a, np.uint64((_DEFORM_MAX << 8) + 1))
    a = a.astype(_I64)
    if ny * nx == 0:
        return a
    if np.abs(a).max() > _DEFORM_MAX << 8:
        raise ValueError("smooth_displacements: displacements beyond 2^30 are not supported")
    g = a.reshape(ny, nx, 2)
    rows = np.clip(np.arange(-1, ny + 1), 0, ny - 1)
    cols = np.clip(np.arange(-1, nx + 1), 0, nx - 1)
    g = g[rows][:, cols]
    v = g[:-2] + 2 * g[1:-1] + g[2:]
    h = v[:, :-2] + 2 * v[:, 1:-1] + v[:, 2:]
    return ((h + 8) >> 4).reshape(-1, 2)


def deform(image, field):
    """``image`` (H, W[, C], uint8 or uint16) warped by ``field`` ((H, W, 2) integers, Q8): output pixel (x, y) samples
    ``X = clamp(256 x + Fx, 0, 256 (W - 1))``, ``Y`` likewise with H; ``x0 = X >> 8, fx = X & 255, x1 = min(x0 + 1, W -
    1)``, ``y0, fy, y1`` likewise; per channel

        out = (I[y0,x0] (256-fx)(256-fy) + I[y0,x1] fx (256-fy) + I[y1,x0] (256-fx) fy + I[y1,x1] fx fy + 32768) >> 16

    A zero field returns the image, an integer constant field the shifted image with replicated edges - both exactly."""
    img = np.asarray(image)
    f = np.asarray(field)
    if img.dtype not in (np.uint8, np.uint16) or img.ndim not in (2, 3) or img.size == 0:
        raise ValueError("deform takes a non-empty uint8 or uint16 image (got %s of shape %s)" % (img.dtype, img.shape))
    if f.shape != img.shape[:2] + (2,):
        raise ValueError("deform: a field of shape %s for an image of shape %s" % (f.shape, img.shape))
    if f.dtype.kind not in "iu":
        raise TypeError("deform: the field must be integers in Q8 (got %s)" % f.dtype)
    H, W = img.shape[:2]
    f = f.astype(_I64)
    X = np.clip(256 * np.arange(W, dtype=_I64)[None, :] + f[:, :, 0], 0, 256 * (W - 1))
    Y = np.clip(256 * np.arange(H, dtype=_I64)[:, None] + f[:, :, 1], 0, 256 * (H - 1))
    x0, fx, y0, fy = X >> 8, X & 255, Y >> 8, Y & 255
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    v = img.astype(_I64)
    if img.ndim == 3:
        fx, fy = fx[:, :, None], fy[:, :, None]
    out = (v[y0, x0] * (256 - fx) * (256 - fy) + v[y0, x1] * fx * (256 - fy) + v[y1, x0] * (256 - fx) * fy
           + v[y1, x1] * fx * fy + 32768) >> 16
    return out.astype(img.dtype)


def deformImage(image: np.ndarray, coarse, displacements, context=None, q8=False):
    """``image`` warped by the field of a coarse grid's displacements, on the device: ``deform(image,
    displacement_field(image.shape, coarse, displacements))`` bit for bit, in one native call (mtm_deform_image: the
    image and the displacements go up, one kernel interpolates the field and resamples, the warped image comes back) - how
    a frame is registered once its drift field is known.  ``image``: uint8 with 1 or 3 channels or single-channel uint16;
    ``coarse`` and ``displacements`` as ``displacement_field`` takes them; ``context``: the _lib.Context to run on.
    ``q8=True``: the integer displacements are in Q8 (``to_q8`` of a drift field known to sub-pixel precision), the result
    ``deform(image, displacement_field(image.shape, coarse, displacements, q8=True))`` (mtm_deform_image_q8)."""
    if not isinstance(image, np.ndarray):
        raise TypeError("image must be a numpy array (got %s)" % type(image).__name__)
    _check_pixels(image, "deformImage", "images", "%s images")
    wc, hc, sx, sy, nx, ny, d = _deform_args(image.shape, coarse, displacements, "deformImage", q8)
    ctx = context or _lib.default_context()     # (only now: every argument error comes before "no GPU")
    kw = {"q8": True} if q8 else {}             # (the default reaches the context as it always did)
    with ctx.lock:
        return ctx.deform_image(image, (wc, hc, sx, sy), d.reshape(-1, 2), **kw).reshape(image.shape)


def displacements(blocks, positions):
    """``positions - blocks[:, :2]``: where every block of ``blocks`` moved to, as (dx, dy) - int64 for matchBlocks'
    integer positions, float64 for refined ones."""
    b = np.asarray(blocks).reshape(-1, 4)
    p = np.asarray(positions).reshape(-1, 2)
    if len(b) != len(p):
        raise ValueError("displacements: %d blocks and %d positions" % (len(b), len(p)))
    return p - b[:, :2]


def _check_method(method, who):
    if not _is_int(method) or method not in (0, 1, 2, 3, 4, 5):
        raise ValueError("%s takes methods 0..5 (got %r)" % (who, method))


def _check_margin(margin, prefix=""):
    if not _is_int(margin) or margin < 0:
        raise ValueError("%smargin must be an integer >= 0 (got %r)" % (prefix, margin))


def _check_flag(value, name):
    if not isinstance(value, bool):
        raise ValueError("%s must be True or False (got %r)" % (name, value))


def _check_second(second):
    """second -> None or the exclusion radius: True is 2, an integer r >= 0 is r."""
    if second is None:
        return None
    if second is True:
        return 2
    if not _is_int(second):
        raise TypeError("second must be None, True or an integer exclusion radius >= 0 (got %r)" % (second,))
    if second < 0:
        raise ValueError("second: the exclusion radius must be >= 0 (got %r)" % (second,))
    return int(min(second, 2 ** 31 - 1))        # (no map is that large: everything is excluded either way)


def _second_arrays(raw2):
    """The second peaks' records as ``(second_positions, second_scores)``."""
    return np.stack((raw2["x"], raw2["y"]), axis=1).astype(_I64), raw2["score"].astype(np.float32)


def _check_pixels(a, who, noun, got):
    """What ``who`` asks of its ``noun`` ("images" / "frames"), all shaped and typed as ``a``: the pixel kind (``got``: how
    the message names ``a``, a format for its dtype), not empty, the row limit."""
    ok = (a.dtype == np.uint8 and (a.ndim == 2 or (a.ndim == 3 and a.shape[2] in (1, 3)))) or \
        (a.dtype == np.uint16 and (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 1)))
    if not ok:
        raise ValueError("%s takes uint8 %s with 1 or 3 channels and single-channel uint16 %s (got %s of shape %s)" % (
            who, noun, noun, got % a.dtype, a.shape))
    if a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError("%s: the %s are empty (shape %s)" % (who, noun, a.shape))
    if a.shape[0] > _MAX_ROWS:
        raise ValueError("%s takes %s of at most %d rows (got %d)" % (who, noun, _MAX_ROWS, a.shape[0]))


def _clip_margin(margin, shape):
    """A margin past the images' larger side clips to the whole image, as a margin of that side does."""
    return int(min(margin, max(shape[0], shape[1])))


def _block_records(b):
    rec = np.empty(len(b), dtype=_lib.BLOCK_DTYPE)
    rec["x"], rec["y"], rec["w"], rec["h"] = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    return rec


def _positions_scores(raw, nbhd, method, refine, shape=None):
    """The records of a call as ``(positions, scores)`` of leading shape ``shape`` (default: one axis); ``refine``: one
    fit over every record's neighbourhood - refineHits' numbers by construction."""
    positions = np.stack((raw["x"], raw["y"]), axis=1).astype(_I64)
    scores = raw["score"].astype(np.float32)
    if refine:
        ox, oy = subpixel.fit_offsets(nbhd, method)
        positions = positions.astype(np.float64) + np.stack((ox, oy), axis=1)
    if shape is None:
        return positions, scores
    return positions.reshape(shape + (2,)), scores.reshape(shape)


def _check_images(reference, image):
    for name, a in (("reference", reference), ("image", image)):
        if not isinstance(a, np.ndarray):
            raise TypeError("%s must be a numpy array (got %s)" % (name, type(a).__name__))
    if reference.shape != image.shape or reference.dtype != image.dtype:
        raise ValueError("reference and image differ in shape, dtype or channel count (%s %s and %s %s)" % (
            reference.shape, reference.dtype, image.shape, image.dtype))
    _check_pixels(image, "matchBlocks", "images", "%s images")


def _check_blocks(blocks, reference):
    """blocks -> (N, 4) int64 array; TypeError / ValueError naming the first offending block."""
    try:
        b = np.asarray(blocks)
    except (ValueError, TypeError):
        b = None
    if b is not None and b.size == 0 and b.ndim <= 2 and (b.ndim < 2 or b.shape[1] in (0, 4)):
        return np.zeros((0, 4), _I64)
    if b is None or b.ndim != 2 or b.shape[1] != 4:
        raise ValueError("blocks must be a sequence or an (N, 4) array of (x, y, w, h)")
    if b.dtype.kind not in "iu":
        for k, v in enumerate(np.asarray(blocks, dtype=object).reshape(-1)):
            if not _is_int(v):
                raise TypeError("blocks[%d]: (x, y, w, h) must be integers (got %r)" % (k // 4, v))
        b = np.array(b.tolist(), dtype=_I64)       # (an object array of Python integers)
    b = b.astype(_I64)
    H, W = reference.shape[0], reference.shape[1]
    x, y, w, h = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    empty = (w < 1) | (h < 1)
    outside = (x < 0) | (y < 0) | (w > W - x) | (h > H - y)
    large = (w * h > _U16_MAX_PIXELS) if reference.dtype == np.uint16 else np.zeros(len(b), bool)
    bad = empty | outside | large
    if bad.any():
        k = int(np.argmax(bad))
        blk = tuple(int(v) for v in b[k])
        if empty[k]:
            raise ValueError("blocks[%d]: a block needs w >= 1 and h >= 1 (got %r)" % (k, blk))
        if outside[k]:
            raise ValueError("blocks[%d]: block %r is not inside the %d x %d reference" % (k, blk, H, W))
        raise ValueError("blocks[%d]: uint16 blocks of more than 2^21 pixels are not supported (their exact correlations "
                         "would pass 2^53)" % k)
    return b


_OFF_LIMIT = 1 << 62            # offsets beyond it are clamped to it first: int64 sums below stay exact


def _check_offsets(offsets, b, shape):
    """offsets -> the (N, 2) int32 offsets that move every block of ``b`` to its clamped position (any integer magnitude
    is taken: the clamp makes it harmless, and it is applied here, in int64, before anything is narrowed)."""
    try:
        o = np.asarray(offsets)
    except (ValueError, TypeError):
        o = None
    if o is not None and o.size == 0 and len(b) == 0:
        return np.zeros((0, 2), np.int32)
    if o is None or o.ndim != 2 or o.shape[1] != 2 or len(o) != len(b):
        raise ValueError("offsets must be an (N, 2) integer array of (dx, dy), one per block (got shape %s for blocks of shape %s)"
                         % (None if o is None else o.shape, b.shape))
    if o.dtype.kind not in "iu":
        flat = np.asarray(offsets, dtype=object).reshape(-1)
        for k, v in enumerate(flat):
            if not _is_int(v):
                raise TypeError("offsets[%d]: (dx, dy) of block %d must be integers (got %r)" % (k // 2, k // 2, v))
        o = np.array([min(max(int(v), -_OFF_LIMIT), _OFF_LIMIT) for v in flat], dtype=_I64).reshape(-1, 2)
    elif o.dtype.kind == "u":
        o = np.minimum(o, np.uint64(_OFF_LIMIT)).astype(_I64)
    o = np.clip(o.astype(_I64), -_OFF_LIMIT, _OFF_LIMIT)
    H, W = int(shape[0]), int(shape[1])
    cx = np.clip(b[:, 0] + o[:, 0], 0, W - b[:, 2])
    cy = np.clip(b[:, 1] + o[:, 1], 0, H - b[:, 3])
    return np.stack((cx - b[:, 0], cy - b[:, 1]), axis=1).astype(np.int32)


_MASK_METHODS = (0, 3)          # TM_SQDIFF and TM_CCORR_NORMED: the package's masked methods


def _check_mask(mask, reference, method):
    """mask -> an (H, W) uint8 array, non-zero where a pixel takes part; and what a masked call asks of the images and
    the method."""
    if not isinstance(mask, np.ndarray):
        raise TypeError("mask must be a numpy array (got %s)" % type(mask).__name__)
    if mask.dtype != np.bool_ and mask.dtype != np.uint8:
        raise TypeError("mask must be of dtype bool or uint8 (got %s)" % mask.dtype)
    if mask.ndim != 2:
        raise ValueError("mask must be a 2-D (H, W) array, one value per pixel for every channel (got shape %s)" % (mask.shape,))
    if mask.shape != reference.shape[:2]:
        raise ValueError("mask of shape %s for a reference of %d x %d pixels" % (mask.shape, reference.shape[0],
                                                                                reference.shape[1]))
    if reference.dtype != np.uint8:
        raise ValueError("matchBlocks: a mask goes with uint8 images (got %s: the package matches masked %s templates in "
                         "float32, which block matching does not take)" % (reference.dtype, reference.dtype))
    if method not in _MASK_METHODS:
        raise ValueError("matchBlocks: a mask goes with methods 0 (TM_SQDIFF) and 3 (TM_CCORR_NORMED), the package's masked "
                         "methods (got %r)" % (method,))
    return np.ascontiguousarray(mask.view(np.uint8) if mask.dtype == np.bool_ else mask)


def mask_fraction(mask, blocks):
    """The share of each block's pixels that ``mask`` keeps: an (N,) float64 array, ``count_nonzero(mask[y:y + h, x:x + w])
    / (w * h)`` for every ``(x, y, w, h)`` of ``blocks`` - from one summed-area table, in plain numpy, so that a caller can
    drop the blocks that are mostly masked before ``matchBlocks(mask=)``.  ``mask``: an (H, W) bool or uint8 array,
    non-zero = the pixel takes part; ``blocks``: as ``matchBlocks`` takes them, each inside the mask."""
    if not isinstance(mask, np.ndarray):
        raise TypeError("mask must be a numpy array (got %s)" % type(mask).__name__)
    if mask.dtype != np.bool_ and mask.dtype != np.uint8:
        raise TypeError("mask must be of dtype bool or uint8 (got %s)" % mask.dtype)
    if mask.ndim != 2:
        raise ValueError("mask must be a 2-D (H, W) array (got shape %s)" % (mask.shape,))
    b = _check_blocks(blocks, mask)
    if len(b) == 0:
        return np.zeros(0, np.float64)
    sat = np.zeros((mask.shape[0] + 1, mask.shape[1] + 1), _I64)
    sat[1:, 1:] = (mask != 0).cumsum(axis=0, dtype=_I64).cumsum(axis=1, dtype=_I64)
    x, y, w, h = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    kept = sat[y + h, x + w] - sat[y, x + w] - sat[y + h, x] + sat[y, x]
    return kept / (w * h).astype(np.float64)


def matchBlocks(reference: np.ndarray, image: np.ndarray, blocks, margin: int, method: int = TM_CCOEFF_NORMED, *,
                refine: bool = False, context=None, offsets=None, second=None, mask=None):
    """
    Where every block of ``reference`` is in ``image``: ``(positions, scores)``, ``positions[k]`` the int64 ``[x, y]``
    (image coordinates) and ``scores[k]`` the float32 score of the single hit of

        findMatchesInBoxes([("b", reference[y:y + h, x:x + w])], image, [search_box(blocks[k], margin, image.shape)],
                           method, N_object=1)[0]

    in one native call.  ``blocks``: a sequence or an (N, 4) integer array of ``(x, y, w, h)``, each inside the reference
    (``grid`` makes regular ones).  ``refine=True``: float64 positions, ``refineHits``' of each hit (the module's
    docstring).  ``context``: the _lib.Context to run on (default: the process's); its templates are not touched.
    ``displacements(blocks, positions)`` gives the displacement field.

    ``offsets``: an (N, 2) integer array of predicted displacements ``(dx, dy)``; block k is then searched in
    ``search_box_at(blocks[k], offsets[k], margin, image.shape)`` - the box of the block moved by its offset and clamped
    into the image - instead (mtm_match_blocks_at: the boxes are computed on the device).  Zero offsets give the call
    without them, bit for bit.

    ``second``: ``None`` (the call above), ``True`` (exclusion radius 2) or an integer radius ``r >= 0``: the call returns
    ``(positions, scores, second_positions, second_scores)``, the last two every block's second correlation peak - the best
    output of the block's map (``computeScoreMap`` of the block over its search box, the map ``positions`` is the best
    output of) among the cells more than ``r`` cells away from the first peak, ``max(|dy|, |dx|) > r``, in the order the
    first peak is chosen by: the larger score (the smaller for methods 0 and 1), ties to the first cell in row-major
    order.  ``second_positions`` is (N, 2) int64 in image coordinates, always integers (``refine`` moves only
    ``positions``), ``second_scores`` float32; a map with no cell outside the exclusion - ``margin=0``, or a map within
    ``r`` cells of its peak - gives ``(-1, -1)`` and NaN.  Computed on the device inside the same native call
    (mtm_match_blocks_second); ``positions`` and ``scores`` are those of the call without ``second``, bit for bit.
    ``peak_ratio(scores, second_scores, method)`` is the signal-to-noise PIV packages report.

    ``mask``: ``None`` (the call above: the same native entry, kernels and launches) or an (H, W) array of dtype bool or
    uint8 over the reference, non-zero = the pixel takes part, in every channel (mtm_match_blocks_masked, DESIGN 5.6.5:
    the mask goes up once and a kernel cuts every block together with its mask).  Block k is then matched as a masked
    template: the result is what this loop returns, positions equal and float32 score bits equal -

        m = (mask[y:y + h, x:x + w] != 0).astype(np.uint8)
        m = m if reference.ndim == 2 else np.repeat(m[:, :, None], reference.shape[2], 2)
        hit, = findMatches([("b", reference[y:y + h, x:x + w], m)], image, method, N_object=1,
                           searchBox=search_box(blocks[k], margin, image.shape))

    - with ties to the first output in row-major order of the box's map.  Scope: uint8 images, methods 0 (TM_SQDIFF) and 3
    (TM_CCORR_NORMED), the package's masked methods; any other method, uint16 images and a mask of another shape raise
    ValueError, one of another dtype TypeError.  With M the block's binary mask, ``TM = T M`` and every sum taken over all
    channels - ``tms = sum TM^2``, per output ``c1 = sum I TM`` and ``c2 = sum (I M)^2`` -, method 3 scores
    ``float32(c1 / sqrt(tms c2))`` in float64 and method 0 ``float32(-2 c1 + c2 + tms)``.  The none rule: an output whose
    score is NaN (``c2 == 0`` or ``tms == 0`` under method 3) is never the peak; a block whose mask has no set pixel is not
    searched, under either method; such a block, and a block all of whose outputs are NaN, returns position ``(-1, -1)``
    (``(-1.0, -1.0)`` with ``refine=True``) and score NaN, and its second peak is ``(-1, -1)`` / NaN.  ``mask`` composes
    with the other keywords: ``offsets`` only moves the boxes, ``refine=True`` gives ``refineHits``' positions of the same
    masked tuple, ``second`` uses the same maps and exclusion rule, NaN cells never chosen.  ``mask_fraction(mask,
    blocks)`` tells how much of every block is kept.  ``matchBlocksMultipass`` and ``matchBlocksStack`` take no mask in
    this version: a masked multipass is this call with ``offsets=predict_offsets(...)`` per pass.
    """
    _check_images(reference, image)
    _check_method(method, "matchBlocks")
    _check_margin(margin)
    _check_flag(refine, "refine")
    r = _check_second(second)
    mk = None if mask is None else _check_mask(mask, reference, method)
    b = _check_blocks(blocks, reference)
    off = None if offsets is None else _check_offsets(offsets, b, image.shape)
    if len(b) == 0:
        none = (np.zeros((0, 2), dtype=np.float64 if refine else _I64), np.zeros(0, dtype=np.float32))
        return none if r is None else none + (np.zeros((0, 2), dtype=_I64), np.zeros(0, dtype=np.float32))
    rec, m = _block_records(b), _clip_margin(margin, image.shape)
    ctx = context or _lib.default_context()     # (only now: every argument error comes before "no GPU")
    with ctx.lock:
        if mk is not None:
            raw, nbhd, *got = ctx.match_blocks_masked(reference, image, mk, rec, off, m, int(method), refine, second=r)
            raw2 = got[0] if got else None
        elif r is not None:
            raw, nbhd, raw2 = ctx.match_blocks_at(reference, image, rec, off, m, int(method), refine, second=r)
        elif off is None:
            raw, nbhd = ctx.match_blocks(reference, image, rec, m, int(method), refine)
        else:
            raw, nbhd = ctx.match_blocks_at(reference, image, rec, off, m, int(method), refine)
    res = _positions_scores(raw, nbhd, method, refine)
    return res if r is None else res + _second_arrays(raw2)


def _check_passes(passes, image):
    """passes -> (the list, its BLOCK_PASS_DTYPE records for images shaped and typed as ``image``, every pass's grid)."""
    try:
        pl = list(passes)
    except TypeError:
        raise TypeError("passes must be a sequence of (block, step, margin) (got %s)" % type(passes).__name__) from None
    if not pl:
        raise ValueError("passes is empty")
    rec = np.empty(len(pl), dtype=_lib.BLOCK_PASS_DTYPE)
    grids = []
    for p, item in enumerate(pl):
        who = "passes[%d]" % p
        try:
            block, step, margin = item
        except (TypeError, ValueError):
            raise ValueError("%s must be (block, step, margin) (got %r)" % (who, item)) from None
        w, h, sx, sy, nx, ny = _grid_axes(image.shape, block, step, who)
        _check_margin(margin, who + ": ")
        if nx * ny == 0:
            raise ValueError("%s: no %d x %d block fits the %d x %d images (empty grid)" % (
                who, w, h, image.shape[0], image.shape[1]))
        if image.dtype == np.uint16 and w * h > _U16_MAX_PIXELS:
            raise ValueError("%s: uint16 blocks of more than 2^21 pixels are not supported (their exact correlations would "
                             "pass 2^53)" % who)
        rec[p] = (w, h, sx, sy, _clip_margin(margin, image.shape))
        grids.append(grid(image.shape, block, step))
    return pl, rec, grids


def matchBlocksMultipass(reference: np.ndarray, image: np.ndarray, passes, method: int = TM_CCOEFF_NORMED, *,
                         refine: bool = False, context=None, validate=None, second=None, deform: bool = False,
                         steer: str = "integer"):
    """
    Coarse-to-fine block matching in one native call.  ``passes``: a non-empty sequence of ``(block, step, margin)``,
    ``block`` and ``step`` as ``grid`` takes them (``step=None``: the block size).  Pass 0 is ``matchBlocks`` over its
    grid; every later pass searches each block of its own grid in the box centred on what the nearest block of the pass
    before found.  Returns a list with one ``(blocks_p, positions_p, scores_p)`` per pass, exactly what this loop gives:

        off = None
        for p, (block, step, margin) in enumerate(passes):
            b = grid(image.shape, block, step)
            if p: off = predict_offsets(image.shape, passes[p - 1][:2], steer, passes[p][:2])
            steer, _ = matchBlocks(reference, image, b, margin, method, offsets=off)
            pos, sc = matchBlocks(reference, image, b, margin, method, offsets=off, refine=refine)

    The integer positions steer the next pass, never the refined ones.  Scope and checks as ``matchBlocks``'; a pass whose
    grid is empty raises ValueError.  The templates set on the context are left alone.

    ``validate``: ``None`` (the call above, in every respect), ``True`` (threshold 2.0, epsilon 0.5) or ``(threshold,
    epsilon)``: the normalised median test of ``validate`` runs on the device over every pass's displacements, and an
    outlier steers the next pass by its neighbours' median instead of by what it found (mtm_match_blocks_passes_validated:
    still one native call, one small launch per pass more).  Every pass's tuple is then ``(blocks_p, positions_p,
    scores_p, valid_p)``, ``valid_p`` the bool flags of the pass - the last pass is tested too.  ``positions_p`` and
    ``scores_p`` stay the raw matches (refined positions with ``refine=True``): validation only changes what steers the
    next pass.  This equals the loop

        steer = None
        for p, (block, step, margin) in enumerate(passes):
            b = grid(image.shape, block, step)
            off = None if p == 0 else predict_offsets(image.shape, passes[p - 1][:2], steer, passes[p][:2])
            pos, sc = matchBlocks(reference, image, b, margin, method, offsets=off)
            valid, rep = validate(grid_shape(image.shape, block, step), displacements(b, pos), threshold, epsilon)
            steer = b[:, :2] + rep

    (and ``matchBlocks(..., offsets=off, refine=True)`` for the refined positions).

    ``second``: as ``matchBlocks``' - every pass's tuple gets ``second_positions_p, second_scores_p`` appended at its end
    (after ``valid_p`` when ``validate`` is given), those of ``matchBlocks(reference, image, b, margin, method,
    offsets=off, second=second)`` in the loops above (mtm_match_blocks_passes_second, still one native call).  The second
    peaks steer nothing: positions, scores and flags are those of the call without ``second``, bit for bit.

    ``deform``: ``False`` (the call above, in every respect) or ``True``: window deformation between the passes
    (mtm_match_blocks_passes_deformed, DESIGN 5.6.4: still one native call and one host wait).  Instead of moving every
    block's box by the nearest coarse block's displacement, a pass p >= 1 warps the whole ORIGINAL image back by the field
    interpolated from the displacements that steer it (``displacement_field``, ``deform``; never a warp of a warp, so blur
    does not compound), searches every block in the warped image in its own box, and adds the field at the block's centre
    (``field_at``) to what it found - under shear, rotation or strain the block then matches a window deformed like
    itself.  Every pass's tuple gets ``predicted_p`` appended (after ``valid_p`` when ``validate`` is given): float64 (N,
    2), the field at the blocks' centres in pixels, zeros for pass 0.  The call equals, bit for bit, the loop

        steer = None
        for p, (block, step, margin) in enumerate(passes):
            b = grid(image.shape, block, step)
            if p == 0:
                searched, c = image, np.zeros((len(b), 2), np.int64)
            else:
                prev = passes[p - 1][:2]
                d = steer - grid(image.shape, *prev)[:, :2]
                searched = deform(image, displacement_field(image.shape, prev, d))
                c = field_at(image.shape, prev, d, b)
            pos_w, sc = matchBlocks(reference, searched, b, margin, method)
            pos = pos_w + ((c + 128) >> 8)
            steer = pos     # with validate: b[:, :2] + validate(grid_shape(...), pos - b[:, :2], thr, eps)[1]
            # refine=True: matchBlocks(..., refine=True)[0] + c / 256.0

    with ``positions_p = pos`` (refined: the fit in the warped image plus ``c / 256.0``), ``scores_p = sc``, ``valid_p``
    the flags of ``validate`` over ``pos - b[:, :2]`` and ``predicted_p = c / 256.0``.  An integer position of a deformed
    pass carries a displacement and is NOT clamped: it may lie outside ``[0, W - w]`` x ``[0, H - h]``.  ``deform=True``
    with ``second`` raises ValueError; ``len(passes) * max(H, W)`` must stay within 2^22.

    ``steer``: ``"integer"`` (the call above, in every respect) or ``"refined"`` (needs ``deform=True``;
    mtm_match_blocks_passes_steered, still one native call and one host wait): the displacement that steers pass p + 1 is
    pass p's SUB-PIXEL position in Q8 (``to_q8`` of the fit in the searched image, plus the field that steered pass p), an
    outlier's its neighbours' integer median as before, filtered by the 3 x 3 binomial kernel over the grid
    (``smooth_displacements``) - an integer record carries up to half a pixel of rounding into every node of the next field,
    which is why integer steering cannot be iterated, and the filter is what keeps the iteration from diverging.  The
    tuples keep ``deform=True``'s layout and meaning; only what steers the next pass changes.  The call equals, bit for bit,

        S8 = None
        for p, (block, step, margin) in enumerate(passes):
            b = grid(image.shape, block, step)
            if p == 0:
                searched, c = image, np.zeros((len(b), 2), np.int64)
            else:
                searched = deform(image, displacement_field(image.shape, prev, S8, q8=True))
                c = field_at(image.shape, prev, S8, b, q8=True)
            pos_w, sc = matchBlocks(reference, searched, b, margin, method)
            fine_w, _ = matchBlocks(reference, searched, b, margin, method, refine=True)
            pos = pos_w + ((c + 128) >> 8)              # the record; positions_p (refine=True: fine_w + c / 256.0)
            D8 = to_q8(fine_w) - 256 * b[:, :2] + c     # with validate: D8[~valid] = 256 * rep[~valid], (valid, rep) =
            #                                             validate(grid_shape(image.shape, block, step), pos - b[:, :2], ...)
            S8 = smooth_displacements(grid_shape(image.shape, block, step), D8); prev = (block, step)
    """
    _check_images(reference, image)
    _check_method(method, "matchBlocksMultipass")
    _check_flag(refine, "refine")
    _check_flag(deform, "deform")
    if not isinstance(steer, str) or steer not in ("integer", "refined"):
        raise ValueError('steer must be "integer" or "refined" (got %r)' % (steer,))
    if steer == "refined" and not deform:
        raise ValueError("steer='refined' needs deform=True")
    r = _check_second(second)
    if deform and r is not None:
        raise ValueError("matchBlocksMultipass: deform=True does not go with second= in this version")
    if validate is not None:
        if validate is True:
            validate = (2.0, 0.5)
        else:
            if isinstance(validate, (bool, np.bool_, str)) or not hasattr(validate, "__len__") or len(validate) != 2:
                raise ValueError("validate must be None, True or (threshold, epsilon) (got %r)" % (validate,))
            validate = _check_validate_params(validate[0], validate[1], "validate")
    pl, rec, grids = _check_passes(passes, image)
    counts = [len(g) for g in grids]
    if deform and len(pl) * max(image.shape[0], image.shape[1]) > _DEFORM_MAX:
        raise ValueError("matchBlocksMultipass: deform=True takes len(passes) * max(H, W) of at most 2^22 (got %d passes "
                         "over %d x %d images)" % (len(pl), image.shape[0], image.shape[1]))
    ctx = context or _lib.default_context()     # (only now: every argument error comes before "no GPU")
    pred = None
    with ctx.lock:
        if deform:
            kw = {} if validate is None else {"validate": validate}
            if steer == "refined":              # (the default passes nothing new: a context that knows no steer serves it)
                kw["steer"] = 1
            raw, nbhd, *got = ctx.match_blocks_passes(reference, image, rec, counts, int(method), refine, deform=True, **kw)
            flags = got[0] if validate is not None else None
            pred = np.asarray(got[-1], dtype=_I64).reshape(-1, 2) / 256.0
        elif r is not None:
            kw = {} if validate is None else {"validate": validate}
            *got, raw2 = ctx.match_blocks_passes(reference, image, rec, counts, int(method), refine, second=r, **kw)
            raw, nbhd = got[:2]
            flags = got[2] if validate is not None else None
        elif validate is None:
            raw, nbhd = ctx.match_blocks_passes(reference, image, rec, counts, int(method), refine)
        else:
            raw, nbhd, flags = ctx.match_blocks_passes(reference, image, rec, counts, int(method), refine, validate=validate)
    if deform and refine:
        # the record holds the warped position plus the field's integer part: the fit starts from the position in the
        # warped image, in integers, and the whole field is added to it
        positions, scores = _positions_scores(raw, None, method, False)
        ox, oy = subpixel.fit_offsets(nbhd, method)
        shift = (np.asarray(got[-1], dtype=_I64).reshape(-1, 2) + 128) >> 8
        positions = ((positions - shift).astype(np.float64) + np.stack((ox, oy), axis=1)) + pred
    else:
        positions, scores = _positions_scores(raw, nbhd, method, refine)       # (one fit over every pass and block)
    if r is not None:
        positions2, scores2 = _second_arrays(raw2)
    out, at = [], 0
    for g in grids:
        res = (g, positions[at:at + len(g)], scores[at:at + len(g)])
        if validate is not None:
            res += (np.asarray(flags[at:at + len(g)], dtype=bool),)
        if r is not None:
            res += (positions2[at:at + len(g)], scores2[at:at + len(g)])
        if deform:
            res += (pred[at:at + len(g)],)
        out.append(res)
        at += len(g)
    return out


_REFERENCE_MODES = {"previous": _lib.BLOCKS_REF_PREVIOUS, "first": _lib.BLOCKS_REF_FIRST}


def _check_frames(frames):
    """frames -> a list of arrays of one shape and dtype in matchBlocks' scope (an (F, H, W[, C]) array is split along
    its first axis); TypeError / ValueError naming the first offending frame."""
    if isinstance(frames, np.ndarray):
        if frames.ndim not in (3, 4):
            raise ValueError("frames: an array of frames has the shape (F, H, W) or (F, H, W, C) (got %s)" % (frames.shape,))
        fl = list(frames)
    else:
        try:
            fl = list(frames)
        except TypeError:
            raise TypeError("frames must be a sequence of numpy arrays or one array with a leading frame axis (got %s)"
                            % type(frames).__name__) from None
    if not fl:
        raise ValueError("frames is empty")
    for i, f in enumerate(fl):
        if not isinstance(f, np.ndarray):
            raise TypeError("frames[%d] must be a numpy array (got %s)" % (i, type(f).__name__))
        if f.shape != fl[0].shape or f.dtype != fl[0].dtype:
            raise ValueError("frames[%d] differs from frames[0] in shape, dtype or channel count (%s %s, frames[0] %s %s)" % (
                i, f.shape, f.dtype, fl[0].shape, fl[0].dtype))
    _check_pixels(fl[0], "matchBlocksStack", "frames", "frames[0] %s")
    return fl


def plane_peaks(planes, blocks, method, refine=False):
    """
    The peak of every block's score plane: ``(positions, scores)``.  ``planes``: an (N, 2m+1, 2m+1) float array,
    ``planes[k, m + dy, m + dx]`` block k's score at displacement (dx, dy), NaN where there is none (``matchBlocksStack``'s
    ensemble planes, or a combination of the planes of several calls).  Per plane the maximum over the cells that are not
    NaN - the minimum for methods 0 and 1 -, the first such cell in row-major order on ties: ``positions[k]`` is the int64
    ``(x_k + dx, y_k + dy)``, ``scores[k]`` the plane's value as float32.  ``refine=True``: float64 positions, the peak plus
    ``subpixel.fit_offsets`` of the plane's 3 x 3 cells around it (cells outside the plane count as NaN: no offset along
    an axis whose three cells are not all numbers).  Host numpy; a plane without a number raises ValueError.
    """
    _check_method(method, "plane_peaks")
    _check_flag(refine, "refine")
    p = np.asarray(planes)
    if p.ndim != 3 or p.shape[1] != p.shape[2] or p.shape[1] % 2 != 1 or p.dtype.kind != "f":
        raise ValueError("planes must be an (N, 2m+1, 2m+1) float array (got %s %s)" % (p.dtype, p.shape))
    p = p.astype(np.float32, copy=False)
    b = np.asarray(blocks)
    if b.size == 0 and len(p) == 0:
        b = np.zeros((0, 4), _I64)
    if b.ndim != 2 or b.shape[1] != 4 or b.dtype.kind not in "iu" or len(b) != len(p):
        raise ValueError("blocks must be an (N, 4) integer array of (x, y, w, h), one block per plane (got %s for %d planes)"
                         % (b.shape, len(p)))
    n, side = len(p), p.shape[1]
    m = side // 2
    flat = p.reshape(n, side * side)
    nan = np.isnan(flat)
    if nan.all(axis=1).any():
        raise ValueError("planes[%d] holds no number" % int(np.argmax(nan.all(axis=1))))
    if method in (0, 1):
        at = np.argmin(np.where(nan, np.float32(np.inf), flat), axis=1)
    else:
        at = np.argmax(np.where(nan, np.float32(-np.inf), flat), axis=1)
    stray = nan[np.arange(n), at]           # (every number of the plane is the infinity that stood in for NaN)
    at[stray] = np.argmin(nan[stray], axis=1)
    cy, cx = at // side, at % side
    scores = flat[np.arange(n), at].astype(np.float32)
    positions = b[:, :2].astype(_I64) + np.stack((cx - m, cy - m), axis=1).astype(_I64)
    if refine:
        padded = np.full((n, side + 2, side + 2), np.nan, dtype=np.float32)
        padded[:, 1:-1, 1:-1] = p
        rows = (cy[:, None] + np.arange(3)[None, :])[:, :, None]
        cols = (cx[:, None] + np.arange(3)[None, :])[:, None, :]
        nbhd = padded[np.arange(n)[:, None, None], rows, cols]
        ox, oy = subpixel.fit_offsets(nbhd, method)
        positions = positions.astype(np.float64) + np.stack((ox, oy), axis=1)
    return positions, scores


def second_peaks(planes, blocks, method, exclusion=2):
    """
    The second peak of every block's score plane, ``(second_positions, second_scores)`` - ``matchBlocks(second=)``'s rule
    in host numpy, in the shape of ``plane_peaks``: how ``matchBlocksStack(ensemble=True)`` users get the second peak of
    the ensemble planes.  ``planes``: an (N, 2m+1, 2m+1) float array as ``plane_peaks`` takes it, NaN cells counting as
    absent.  Per plane the cells are ordered by score - larger first, smaller first for methods 0 and 1, -0 equal to +0,
    ties to the first cell in row-major order -; the first peak is the first cell of that order (``plane_peaks``' cell),
    the second peak the first among the cells with ``max(|dy|, |dx|) > exclusion`` from it.  ``second_positions[k]`` is the
    int64 ``(x_k + dx, y_k + dy)``, ``second_scores[k]`` the plane's value as float32 (+0 for a zero of either sign);
    ``(-1, -1)`` and NaN where no cell that holds a number lies outside the exclusion.  A plane without a number raises
    ValueError.
    """
    _check_method(method, "second_peaks")
    if not _is_int(exclusion):
        raise TypeError("second_peaks: exclusion must be an integer >= 0 (got %r)" % (exclusion,))
    if exclusion < 0:
        raise ValueError("second_peaks: exclusion must be an integer >= 0 (got %r)" % (exclusion,))
    p = np.asarray(planes)
    if p.ndim != 3 or p.shape[1] != p.shape[2] or p.shape[1] % 2 != 1 or p.dtype.kind != "f":
        raise ValueError("planes must be an (N, 2m+1, 2m+1) float array (got %s %s)" % (p.dtype, p.shape))
    p = p.astype(np.float32, copy=False)
    b = np.asarray(blocks)
    if b.size == 0 and len(p) == 0:
        b = np.zeros((0, 4), _I64)
    if b.ndim != 2 or b.shape[1] != 4 or b.dtype.kind not in "iu" or len(b) != len(p):
        raise ValueError("blocks must be an (N, 4) integer array of (x, y, w, h), one block per plane (got %s for %d planes)"
                         % (b.shape, len(p)))
    n, side = len(p), p.shape[1]
    m = side // 2
    flat = np.ascontiguousarray(p.reshape(n, side * side))
    nan = np.isnan(flat)
    if nan.all(axis=1).any():
        raise ValueError("planes[%d] holds no number" % int(np.argmax(nan.all(axis=1))))
    if n == 0:
        return np.zeros((0, 2), _I64), np.zeros(0, np.float32)
    # the 64-bit quality key of every cell (mtm_quality_key.h): order(q) << 32 | ~index, 0 for a NaN cell
    q = (-flat if method in (0, 1) else flat) + np.float32(0.0)            # (-0 -> +0)
    bits = q.view(np.uint32).astype(np.uint64)
    order = np.where(bits >> np.uint64(31), bits ^ np.uint64(0xFFFFFFFF), bits | np.uint64(0x80000000))
    keys = (order << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(side * side, dtype=np.uint64))[None, :]
    keys[nan] = 0
    rows = np.arange(n)
    first = np.argmax(keys, axis=1)
    cy, cx = np.divmod(np.arange(side * side), side)
    away = np.maximum(np.abs(cy[None, :] - (first // side)[:, None]), np.abs(cx[None, :] - (first % side)[:, None])) > exclusion
    keys[~away] = 0
    at = np.argmax(keys, axis=1)
    some = keys[rows, at] != 0
    positions = np.where(some[:, None], b[:, :2].astype(_I64) + np.stack((at % side - m, at // side - m), axis=1), -1)
    scores = np.where(some, flat[rows, at] + np.float32(0.0), np.float32(np.nan)).astype(np.float32)
    return positions.astype(_I64), scores


def peak_ratio(scores, second_scores, method):
    """
    The peak-to-peak ratio of ``matchBlocks(second=)``'s two scores, float64 and >= 1 for a first peak that beats the
    second: the signal-to-noise PIV packages report per vector.  Methods 2..5 (a larger score is better): ``scores /
    second_scores`` where the second score is > 0, ``inf`` where it is <= 0.  Methods 0 and 1 (smaller is better):
    ``second_scores / scores`` where the first score is > 0, ``inf`` where it is 0.  NaN where there is no second peak
    (a NaN second score).  Meant for the normalised methods (1, 3, 5), whose scores have a fixed scale; the raw sums of
    methods 0, 2 and 4 grow with the block's brightness, and TM_CCOEFF's can be negative.
    """
    _check_method(method, "peak_ratio")
    s1 = np.asarray(scores, dtype=np.float64)
    s2 = np.asarray(second_scores, dtype=np.float64)
    if s1.shape != s2.shape:
        raise ValueError("peak_ratio: scores of shape %s and second_scores of shape %s" % (s1.shape, s2.shape))
    num, den = (s2, s1) if method in (0, 1) else (s1, s2)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(den > 0, num / np.where(den > 0, den, 1.0), np.inf)
    return np.where(np.isnan(s2), np.nan, ratio).astype(np.float64)


def matchBlocksStack(frames, blocks, margin: int, method: int = TM_CCOEFF_NORMED, *, reference: str = "previous",
                     refine: bool = False, ensemble: bool = False, context=None, offsets=None):
    """
    ``matchBlocks`` over a stack of F frames in one native call.  ``frames``: a sequence of F arrays of one shape and dtype
    or one array with a leading frame axis.  Pair p (0 .. F - 2) searches ``frames[p + 1]``; its reference is ``frames[p]``
    (``reference="previous"``) or ``frames[0]`` (``"first"``).

    ``ensemble=False``: ``(positions, scores)`` of shapes (F - 1, N, 2) and (F - 1, N), ``positions[p], scores[p]`` being
    exactly ``matchBlocks(ref_p, frames[p + 1], blocks, margin, method, refine=refine)``.  One frame gives empty arrays.

    ``ensemble=True``: ``(positions, scores, planes)``; ``planes`` is an (N, 2m+1, 2m+1) float32 array (m: the margin,
    clipped to the frames' larger side), ``planes[k, m + dy, m + dx]`` the mean over the pairs of block k's score at
    displacement (dx, dy) - the float32 rounding of the pairs' float32 scores summed in float64 in pair order and divided
    by their number -, NaN where the block's clipped search box has no such displacement.  ``positions`` (N, 2) and
    ``scores`` (N,) are ``plane_peaks(planes, blocks, method, refine)``.  Needs two frames at least, and planes of at
    most OPT_BOXES_MAX_FLOATS cells in all.

    ``offsets``: ``None`` (the call above: the same native entry with the same arguments) or an (N, 2) integer array of
    predicted displacements ``(dx, dy)``, shared by every pair and checked as ``matchBlocks``' (mtm_match_blocks_stack_at):
    block k of every pair is searched in ``search_box_at(blocks[k], offsets[k], margin, shape)``.  ``ensemble=False``:
    ``positions[p], scores[p]`` are exactly ``matchBlocks(ref_p, frames[p + 1], blocks, margin, method, refine=refine,
    offsets=offsets)``.  ``ensemble=True``: with ``moved = moved_blocks(blocks, offsets, shape)``, ``planes[k, m + dy, m +
    dx]`` is the mean over the pairs - the arithmetic above - of block k's score at position ``(moved[k, 0] + dx, moved[k,
    1] + dy)``, NaN where the clipped box has no such output, and ``positions, scores`` are ``plane_peaks(planes, moved,
    method, refine)``; the means and the NaN fill are computed on the device.  Zero offsets give the call without them.
    """
    fl = _check_frames(frames)
    _check_method(method, "matchBlocksStack")
    _check_margin(margin)
    if not isinstance(reference, str) or reference not in _REFERENCE_MODES:
        raise ValueError('reference must be "previous" or "first" (got %r)' % (reference,))
    _check_flag(refine, "refine")
    _check_flag(ensemble, "ensemble")
    b = _check_blocks(blocks, fl[0])
    off = None if offsets is None else _check_offsets(offsets, b, fl[0].shape)
    n, pairs = len(b), len(fl) - 1
    if ensemble and pairs < 1:
        raise ValueError("ensemble=True needs two frames at least: there is no pair to average")
    m = _clip_margin(margin, fl[0].shape)
    side = 2 * m + 1
    ptype = np.float64 if refine else _I64
    if ensemble and n == 0:
        return np.zeros((0, 2), dtype=ptype), np.zeros(0, dtype=np.float32), np.zeros((0, side, side), dtype=np.float32)
    if not ensemble and (n == 0 or pairs == 0):
        return np.zeros((pairs, n, 2), dtype=ptype), np.zeros((pairs, n), dtype=np.float32)
    rec = _block_records(b)
    ctx = context or _lib.default_context()     # (only now: every argument error above comes before "no GPU")
    mode = _REFERENCE_MODES[reference]
    with ctx.lock:
        if ensemble:
            budget = int(ctx.get_option(_lib.OPT_BOXES_MAX_FLOATS))
            if n * side * side > budget:
                raise ValueError("ensemble=True: the planes of %d blocks at margin %d hold %d floats, more than the "
                                 "context's OPT_BOXES_MAX_FLOATS = %d" % (n, m, n * side * side, budget))
            if off is None:
                planes = ctx.match_blocks_stack(fl, rec, m, int(method), mode, planes=True)
            else:
                planes, _ = ctx.match_blocks_stack_at(fl, rec, off, m, int(method), mode, planes=True)
        elif off is None:
            raw, nbhd = ctx.match_blocks_stack(fl, rec, m, int(method), mode, with_nbhd=refine)
        else:
            raw, nbhd = ctx.match_blocks_stack_at(fl, rec, off, m, int(method), mode, with_nbhd=refine)
    if ensemble:
        moved = b if off is None else b + np.concatenate((off.astype(_I64), np.zeros((n, 2), _I64)), axis=1)
        positions, scores = plane_peaks(planes, moved, int(method), refine)
        return positions, scores, planes
    return _positions_scores(raw, nbhd, method, refine, (pairs, n))     # (one fit over every pair and block)


def matchBlocksStackMultipass(frames, passes, method: int = TM_CCOEFF_NORMED, *, reference: str = "previous",
                              refine: bool = False, ensemble: bool = False, context=None):
    """
    Coarse-to-fine block matching over a stack of F frames in one native call with one host wait
    (mtm_match_blocks_stack_passes).  ``frames`` and ``reference`` as ``matchBlocksStack`` takes them,
    ``passes`` as ``matchBlocksMultipass`` does.  Returns a list with one tuple per pass.

    ``ensemble=False``: every pass gives ``(blocks_p, positions_p (F - 1, N_p, 2), scores_p (F - 1, N_p))``, slice ``[q]``
    being pass p of ``matchBlocksMultipass(ref_q, frames[q + 1], passes, method, refine=refine)``, bit for bit.  Every pair
    runs its own chain of passes on the device - records, the next pass's boxes, the next pass -, every frame goes up
    once, in ``matchBlocksStack``'s frame chunks, and all passes of a chunk's pairs run before the next upload.  One frame
    gives arrays with a leading 0.

    ``ensemble=True``: every pass gives ``(blocks_p, positions_p (N_p, 2), scores_p (N_p,), planes_p (N_p, 2 m_p + 1, 2 m_p
    + 1))``: the passes run on ensemble planes, each centred on what the ensemble peak of the pass before found - the
    integer peak steers, never the refined one.  The call equals, bit for bit, the loop

        steer = None
        for p, (block, step, margin) in enumerate(passes):
            b = grid(shape, block, step)
            off = None if p == 0 else predict_offsets(shape, passes[p - 1][:2], steer, passes[p][:2])
            steer, _, _ = matchBlocksStack(frames, b, margin, method, reference=reference, ensemble=True, offsets=off)
            pos, sc, planes = matchBlocksStack(frames, b, margin, method, reference=reference, ensemble=True, offsets=off,
                                               refine=refine)

    Every pass needs every pair: a stack that fits one frame chunk (OPT_BATCH_MAX_ROWS) goes up once, any other once per
    pass.  Needs two frames at least; the planes of all passes together hold at most OPT_BOXES_MAX_FLOATS floats
    (ValueError before any native call otherwise).

    Not in this version: ``validate``, ``second``, ``deform``, ``steer`` and ``mask``.  Scope and checks as the two
    functions'; the templates set on the context are left alone.
    """
    fl = _check_frames(frames)
    _check_method(method, "matchBlocksStackMultipass")
    if not isinstance(reference, str) or reference not in _REFERENCE_MODES:
        raise ValueError('reference must be "previous" or "first" (got %r)' % (reference,))
    _check_flag(refine, "refine")
    _check_flag(ensemble, "ensemble")
    pl, rec, grids = _check_passes(passes, fl[0])
    pairs, shape = len(fl) - 1, fl[0].shape
    if ensemble and pairs < 1:
        raise ValueError("ensemble=True needs two frames at least: there is no pair to average")
    counts = [len(g) for g in grids]
    sides = [2 * int(a["margin"]) + 1 for a in rec]
    ptype = np.float64 if refine else _I64
    if pairs == 0:
        return [(g, np.zeros((0, len(g), 2), dtype=ptype), np.zeros((0, len(g)), dtype=np.float32)) for g in grids]
    ctx = context or _lib.default_context()     # (only now: every argument error above comes before "no GPU")
    mode = _REFERENCE_MODES[reference]
    with ctx.lock:
        if ensemble:
            budget, cells = int(ctx.get_option(_lib.OPT_BOXES_MAX_FLOATS)), sum(k * sd * sd for k, sd in zip(counts, sides))
            if cells > budget:
                raise ValueError("ensemble=True: the planes of %d passes hold %d floats, more than the context's "
                                 "OPT_BOXES_MAX_FLOATS = %d" % (len(pl), cells, budget))
            flat, raw = ctx.match_blocks_stack_passes(fl, rec, counts, int(method), mode, planes=True)
        else:
            raw, nbhd = ctx.match_blocks_stack_passes(fl, rec, counts, int(method), mode, with_nbhd=refine)
    out, at = [], 0
    if not ensemble:
        positions, scores = _positions_scores(raw, nbhd, method, refine, (pairs, sum(counts)))    # (one fit over everything)
        for g in grids:
            out.append((g, positions[:, at:at + len(g)], scores[:, at:at + len(g)]))
            at += len(g)
        return out
    steer, cell = None, 0
    for p, g in enumerate(grids):
        planes = flat[cell:cell + len(g) * sides[p] ** 2].reshape(len(g), sides[p], sides[p])
        # the blocks the pass's planes lie around: the grid moved by what the peaks of the pass before predict
        moved = g if p == 0 else moved_blocks(g, predict_offsets(shape, pl[p - 1][:2], steer, pl[p][:2]), shape)
        steer, scores = _positions_scores(raw[at:at + len(g)], None, method, False)         # (the device's peak records)
        positions = plane_peaks(planes, moved, int(method), True)[0] if refine else steer
        out.append((g, positions, scores, planes))
        at += len(g)
        cell += len(g) * sides[p] ** 2
    return out
