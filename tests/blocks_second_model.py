"""Restatements for the second correlation peak (MTM.matchBlocks(second=), MTM.blocks.second_peaks, mtm_debug_second_peaks)
that share no code with them: the rule in plain Python loops over a float32 map, the constructed maps its tests sweep, and
blocks_validate_model's oracle context extended with the second-peak calls."""
import numpy as np

import blocks_passes_model as M
import blocks_validate_model as V
import mtm_oracle as O
from MTM import _lib
from MTM import blocks as B

NONE = ((-1, -1), np.float32(np.nan))
RADII = (0, 1, 2, 5)


def _better(qa, ia, qb, ib):
    """Cell a (quality qa, row-major index ia) comes before cell b: the larger quality, -0 equal to +0 (a float compare),
    ties to the smaller index."""
    return qa > qb or (qa == qb and ia < ib)


def _best(smap, mode_min, allowed):
    """The first cell, in the rule's order, of the float32 map among those `allowed(y, x)` that hold a number: (y, x) or
    None."""
    best = None
    oh, ow = smap.shape
    for y in range(oh):
        for x in range(ow):
            s = smap[y, x]
            if s != s or not allowed(y, x):
                continue
            q = -s if mode_min else s
            if best is None or _better(q, y * ow + x, best[0], best[1]):
                best = (q, y * ow + x)
    return None if best is None else divmod(best[1], ow)


def second_peak(smap, method, r, first=None):
    """((x, y), score) of the second peak of the 2-D float32 map under `method` with exclusion radius r, in the map's own
    coordinates - NONE where no cell lies outside the exclusion -, and the first peak's (x, y) (None: a map of NaNs).
    `first`: the first peak's (y, x) if it is given instead of found."""
    smap = np.asarray(smap, dtype=np.float32)
    mode_min = method in (0, 1)
    if first is None:
        first = _best(smap, mode_min, lambda y, x: True)
    if first is None:
        return NONE, None
    py, px = first
    at = _best(smap, mode_min, lambda y, x: max(abs(y - py), abs(x - px)) > r)
    if at is None:
        return NONE, (px, py)
    s = smap[at]
    q = -s if mode_min else s
    return ((at[1], at[0]), np.float32((-q if mode_min else q) + np.float32(0.0))), (px, py)


def same_seconds(positions, scores, expected):
    """positions (N, 2) int64 and scores (N,) float32 equal the model's [((x, y), score)]: positions with ==, scores as bit
    patterns, NaN exactly where the model has none."""
    assert positions.dtype == np.int64 and positions.shape == (len(expected), 2)
    assert scores.dtype == np.float32 and scores.shape == (len(expected),)
    e_pos = np.array([p for p, _ in expected], dtype=np.int64).reshape(-1, 2)
    e_sc = np.array([s for _, s in expected], dtype=np.float32)
    none = np.isnan(e_sc)
    bad = np.flatnonzero((positions != e_pos).any(axis=1) | (np.isnan(scores) != none) |
                         (~none & (scores.view(np.uint32) != e_sc.view(np.uint32))))
    assert len(bad) == 0, (bad[:5], positions[bad[:5]], e_pos[bad[:5]], scores[bad[:5]], e_sc[bad[:5]])
    assert ((positions[none] == -1).all() and (positions[~none] >= 0).all())


# ---- constructed maps ---------------------------------------------------------------------------------------------------
def _places(oh, ow):
    """The four corners, the middles of the four edges and the centre of an oh x ow map, without repeats."""
    return sorted({(y, x) for y in (0, oh // 2, oh - 1) for x in (0, ow // 2, ow - 1)})


def shapes(r, extra=()):
    """1 x 1, 1 x n and n x 1, sides 3, 5, 2r + 1, 2r + 2 and 17, and `extra`."""
    return [(1, 1), (1, 9), (9, 1), (3, 3), (5, 5), (2 * r + 1, 2 * r + 1), (2 * r + 2, 2 * r + 2), (17, 17)] + list(extra)


def maps(r, mode_min, seed, extra=()):
    """The float32 maps of one (r, mode_min): per shape a coarse random map (eight levels: many ties) with the best value
    planted at every corner, on every edge and inside; an all-equal map; a map of +0, -0 and a few small values of both
    signs."""
    rng = np.random.RandomState(seed)
    out = []
    for oh, ow in shapes(r, extra):
        for (y, x) in _places(oh, ow):
            q = (rng.randint(0, 8, size=(oh, ow)) / np.float32(8.0)).astype(np.float32)
            q[y, x] = 2.0
            out.append(-q if mode_min else q)
        out.append(np.full((oh, ow), 0.25, dtype=np.float32))
        z = rng.choice(np.array([0.0, -0.0, 0.0, -0.0, -0.5, 0.5, -1.0], dtype=np.float32), size=(oh, ow))
        out.append(z.astype(np.float32))
    return out


def padded(smap):
    """An ensemble-style plane: the map inside the smallest odd square that holds it with a NaN border at least one cell wide
    on the right and at the bottom, at an offset that varies with its shape; ((N=1) plane, (oy, ox))."""
    oh, ow = smap.shape
    side = max(oh, ow) + 2
    side += 1 - side % 2
    oy, ox = (side - oh) // 2, (side - ow) - (side - ow) // 3 - 1
    plane = np.full((side, side), np.nan, dtype=np.float32)
    plane[oy:oy + oh, ox:ox + ow] = smap
    return plane, (oy, ox)


# ---- the calls on the CPU oracle ------------------------------------------------------------------------------------------
def block_map(reference, image, block, offset, margin, method, score_map):
    """The map of `block` = (x, y, w, h) of the reference moved by `offset`: score_map(block's pixels, the image cropped to
    search_box_at(...), method), and the box's origin (x0, y0)."""
    x, y, w, h = (int(v) for v in block)
    x0, y0, bw, bh = B.search_box_at((x, y, w, h), offset, margin, image.shape)
    t = np.ascontiguousarray(reference[y:y + h, x:x + w])
    return np.asarray(score_map(t, np.ascontiguousarray(image[y0:y0 + bh, x0:x0 + bw]), method), dtype=np.float32), (x0, y0)


def expected_seconds(reference, image, blocks, offsets, margin, method, r, score_map, firsts=None):
    """[((x, y), score)] in image coordinates for every block, by second_peak over block_map; `firsts` (N, 2): the first
    peaks a call returned, asserted to be those of the maps."""
    out = []
    for k, b in enumerate(blocks):
        smap, (x0, y0) = block_map(reference, image, b, (0, 0) if offsets is None else offsets[k], margin, method, score_map)
        ((sx, sy), s), (fx, fy) = second_peak(smap, method, r)
        if firsts is not None:
            assert (fx + x0, fy + y0) == tuple(int(v) for v in firsts[k]), (k, b, (fx + x0, fy + y0), firsts[k])
        out.append(((sx + x0, sy + y0) if sx >= 0 else (-1, -1), s))
    return out


class OracleCtx(V.OracleCtx):
    """blocks_validate_model.OracleCtx with the second-peak calls: match_blocks_at(second=) and match_blocks_passes(second=)
    run the calls without it and add the brute-force second peak of the oracle's map of every block."""
    def _seconds(self, reference, image, blocks, offsets, margin, method, r, out):
        tuples = [tuple(int(b[f]) for f in "xywh") for b in blocks]
        exp = expected_seconds(np.ascontiguousarray(reference), np.ascontiguousarray(image), tuples, offsets, margin, method, r,
                               O.compute_score_map, firsts=np.stack((out["x"], out["y"]), axis=1))
        out2 = out.copy()
        out2["x"], out2["y"] = [p[0] for p, _ in exp], [p[1] for p, _ in exp]
        out2["score"] = [s for _, s in exp]
        return out2

    def match_blocks_at(self, reference, image, blocks, offsets, margin, method, with_nbhd=False, **kw):
        if "second" not in kw:
            return super().match_blocks_at(reference, image, blocks, offsets, margin, method, with_nbhd)
        r = kw.pop("second")
        assert not kw and isinstance(r, int) and r >= 0
        self.calls.append(("second", blocks.copy(), None if offsets is None else offsets.copy(), margin, method, with_nbhd, r))
        off = np.zeros((len(blocks), 2), np.int64) if offsets is None else offsets
        out, nbhd = self._run(reference, image, blocks, off, margin, method, with_nbhd)
        return out, nbhd, self._seconds(reference, image, blocks, off, margin, method, r, out)

    def match_blocks_passes(self, reference, image, passes, counts, method, with_nbhd=False, **kw):
        if "second" not in kw:
            return super().match_blocks_passes(reference, image, passes, counts, method, with_nbhd, **kw)
        r = kw.pop("second")
        validate = kw.pop("validate", None)
        assert not kw and isinstance(r, int) and r >= 0 and passes.dtype == _lib.BLOCK_PASS_DTYPE
        self.calls.append(("passes_second", passes.copy(), list(counts), method, with_nbhd, validate, r))
        outs, nbs, flags, seconds, prev = [], [], [], [], None
        for p, a in enumerate(passes):
            spec = ((int(a["bw"]), int(a["bh"])), (int(a["sx"]), int(a["sy"])))
            g = B.grid(image.shape, *spec)
            assert len(g) == counts[p]
            off = np.zeros((len(g), 2), np.int64)
            if p:
                cg = B.grid(image.shape, *prev[0])
                near = M.nearest_brute(image.shape, prev[0], spec)
                off = prev[1][near] - cg[near, :2]
            rec = _lib.block_records(g)
            out, nb = self._run(reference, image, rec, off, int(a["margin"]), method, with_nbhd)
            pos = np.stack((out["x"], out["y"]), axis=1).astype(np.int64)
            if validate is not None:
                ny, nx = len(np.unique(g[:, 1])), len(np.unique(g[:, 0]))
                valid, rep = V.validate_brute((ny, nx), pos - g[:, :2], *validate)
                flags.append(np.array(valid, dtype=bool))
                pos = g[:, :2] + np.array(rep, dtype=np.int64).reshape(-1, 2)
            prev = (spec, pos)
            outs.append(out)
            nbs.append(nb)
            seconds.append(self._seconds(reference, image, rec, off, int(a["margin"]), method, r, out))
        res = (np.concatenate(outs), (np.concatenate(nbs) if with_nbhd else None))
        if validate is not None:
            res += (np.concatenate(flags),)
        return res + (np.concatenate(seconds),)
