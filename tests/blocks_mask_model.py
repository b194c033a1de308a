"""MTM.matchBlocks(mask=) restated on the CPU oracle: per block the oracle's masked score map of the block
over its search box, the first extremum in row-major order among the cells that hold a number, the none rule, and the
second peak by matchBlocks(second=)'s rule with NaN cells skipped.  Shares no code with the call."""
import numpy as np

import mtm_oracle as O
from MTM import blocks as B

NONE_POS = (-1, -1)


def block_mask(reference, mask, block):
    """The mask tuple element of `block` = (x, y, w, h): (mask != 0) as uint8, repeated over the reference's channels."""
    x, y, w, h = (int(v) for v in block)
    m = (np.asarray(mask)[y:y + h, x:x + w] != 0).astype(np.uint8)
    return m if reference.ndim == 2 else np.repeat(m[:, :, None], reference.shape[2], 2)


def block_tuple(reference, mask, block, name="b"):
    """The masked template tuple the loop through findMatches sets for `block`."""
    x, y, w, h = (int(v) for v in block)
    return (name, np.ascontiguousarray(reference[y:y + h, x:x + w]), block_mask(reference, mask, block))


def box_of(block, offset, margin, shape):
    block = tuple(int(v) for v in block)
    return B.search_box(block, margin, shape) if offset is None else B.search_box_at(block, offset, margin, shape)


def block_map(reference, image, mask, block, offset, margin, method):
    """The oracle's masked float32 map of `block` over its box, and the box's origin (x0, y0); None for an empty mask."""
    _, t, m = block_tuple(reference, mask, block)
    x0, y0, bw, bh = box_of(block, offset, margin, image.shape)
    if not m.any():
        return None, (x0, y0)
    crop = np.ascontiguousarray(image[y0:y0 + bh, x0:x0 + bw])
    return np.asarray(O.match_template(crop, t, method, mask=m), dtype=np.float32), (x0, y0)


def _ordered(smap, method):
    """The cells of the map that hold a number, best first: larger score first (smaller for methods 0 and 1), -0 equal to
    +0, ties to the smaller row-major index."""
    flat = smap.reshape(-1).astype(np.float64)
    idx = np.flatnonzero(~np.isnan(flat))
    q = flat[idx] if method in (0, 1) else -flat[idx]           # ascending sort key; -0.0 == 0.0 in the comparison
    return idx[np.lexsort((idx, q + 0.0))]


def peaks(smap, method, exclusion=None):
    """((y, x) or None, score) of the first peak of the map, and - exclusion given - of the second peak: the first cell of
    the order more than `exclusion` cells (Chebyshev) away from the first peak.  None / NaN where there is none."""
    nan = np.float32(np.nan)
    none = (None, nan)
    if smap is None:
        return (none, none) if exclusion is not None else none
    order = _ordered(smap, method)
    if len(order) == 0:
        return (none, none) if exclusion is not None else none
    ow = smap.shape[1]
    fy, fx = divmod(int(order[0]), ow)
    first = ((fy, fx), np.float32(smap[fy, fx] + np.float32(0.0)))
    if exclusion is None:
        return first
    ys, xs = np.divmod(order, ow)
    away = np.maximum(np.abs(ys - fy), np.abs(xs - fx)) > exclusion
    if not away.any():
        return first, none
    k = int(np.argmax(away))
    sy, sx = int(ys[k]), int(xs[k])
    return first, ((sy, sx), np.float32(smap[sy, sx] + np.float32(0.0)))


def match_blocks(reference, image, mask, blocks, margin, method, offsets=None, second=None):
    """(positions (N, 2) int64, scores (N,) float32[, second_positions, second_scores]) of matchBlocks(mask=) by the rule:
    a block whose mask has no set pixel, or whose map holds no number, gives (-1, -1) and NaN."""
    r = None if second is None else (2 if second is True else int(second))
    n = len(blocks)
    pos, sc = np.full((n, 2), -1, np.int64), np.full(n, np.nan, np.float32)
    pos2, sc2 = pos.copy(), sc.copy()
    for k, b in enumerate(blocks):
        smap, (x0, y0) = block_map(reference, image, mask, b, None if offsets is None else offsets[k], margin, method)
        res = peaks(smap, method, r)
        first, sec = res if r is not None else (res, (None, None))
        if first[0] is not None:
            pos[k], sc[k] = (x0 + first[0][1], y0 + first[0][0]), first[1]
        if sec[0] is not None:
            pos2[k], sc2[k] = (x0 + sec[0][1], y0 + sec[0][0]), sec[1]
    return (pos, sc) if r is None else (pos, sc, pos2, sc2)


def same(got_pos, got_sc, exp_pos, exp_sc):
    """Positions with ==, scores as bit patterns, NaN exactly where the expectation has none."""
    assert got_pos.shape == exp_pos.shape and got_sc.dtype == np.float32 and got_sc.shape == exp_sc.shape
    none = np.isnan(exp_sc)
    bad = np.flatnonzero((got_pos != exp_pos).any(axis=1) | (np.isnan(got_sc) != none) |
                         (~none & (got_sc.view(np.uint32) != exp_sc.view(np.uint32))))
    assert len(bad) == 0, (bad[:5], got_pos[bad[:5]], exp_pos[bad[:5]], got_sc[bad[:5]], exp_sc[bad[:5]])
