"""Plain restatements for MTM.matchBlocksStack(offsets=) and MTM.matchBlocksStackMultipass (mtm_match_blocks_stack_at,
mtm_match_blocks_stack_passes) for their tests: where an offset moves a block, by search over every position
the block can have; the ensemble planes around moved blocks from per-block score maps of host-cut crops; the peak rule of
the device's plane kernel, cell by cell; the two by-hand loops the new function is documented to equal; and a context that
runs the three stack calls on the CPU oracle.  Loops over cells and blocks, nothing shared with the code under test."""
import numpy as np

import mtm_oracle as O
import blocks_passes_model as P
import blocks_stack_model as S
from MTM import _lib
from MTM import blocks as B

PREVIOUS, FIRST = S.PREVIOUS, S.FIRST


def moved_brute(blocks, offsets, shape):
    """(N, 4) int64 of (cx, cy, w, h): of every position at which the block lies inside the image, the one nearest to
    (x + dx, y + dy), per axis."""
    out = []
    for (x, y, w, h), (dx, dy) in zip(np.asarray(blocks).reshape(-1, 4).tolist(), np.asarray(offsets).reshape(-1, 2).tolist()):
        cx = min(range(0, int(shape[1]) - w + 1), key=lambda c: abs(c - (x + dx)))
        cy = min(range(0, int(shape[0]) - h + 1), key=lambda c: abs(c - (y + dy)))
        out.append((cx, cy, w, h))
    return np.array(out, dtype=np.int64).reshape(-1, 4)


def planes_at(score_map, frames, blocks, offsets, margin, method, mode):
    """The ensemble planes around moved blocks: per pair and block score_map(the block cut out of the reference where it
    is, the searched frame's crop to the moved block's search box, method), cell (m + dy, m + dx) holding the score at
    position (cx + dx, cy + dy); summed in float64 in pair order starting from the first pair's own value, divided by the
    number of pairs, rounded to float32; NaN where the clipped box has no output."""
    side = 2 * margin + 1
    blocks = np.asarray(blocks, dtype=np.int64).reshape(-1, 4).tolist()
    moved = moved_brute(blocks, offsets, frames[0].shape).tolist()
    pairs = S.pair_frames(len(frames), mode)
    total = None
    for r, s in pairs:
        one = np.full((len(blocks), side, side), np.nan, dtype=np.float64)
        for k, ((x, y, w, h), (cx, cy, _, _)) in enumerate(zip(blocks, moved)):
            x0, y0, bw, bh = S.search_box((cx, cy, w, h), margin, frames[0].shape)
            m = np.asarray(score_map(np.ascontiguousarray(frames[r][y:y + h, x:x + w]),
                                     np.ascontiguousarray(frames[s][y0:y0 + bh, x0:x0 + bw]), method))
            assert m.dtype == np.float32 and m.shape == (bh - h + 1, bw - w + 1)
            ox, oy = x0 - (cx - margin), y0 - (cy - margin)
            assert ox >= 0 and oy >= 0
            one[k, oy:oy + m.shape[0], ox:ox + m.shape[1]] = m.astype(np.float64)
        total = one if total is None else total + one
    return (total / float(len(pairs))).astype(np.float32)


def mean_planes(acc, clip, oh, ow, pairs):
    """(N, side, side) float32: float32(acc / pairs) in the cells oy <= cy < oy + oh, ox <= cx < ox + ow, NaN elsewhere."""
    out = np.full(acc.shape, np.nan, dtype=np.float32)
    for k in range(len(acc)):
        (ox, oy), h, w = clip[k], oh[k], ow[k]
        box = acc[k, oy:oy + h, ox:ox + w]
        with np.errstate(over="ignore"):           # (a mean past the largest float32 is +-inf)
            out[k, oy:oy + box.shape[0], ox:ox + box.shape[1]] = (box / np.float64(pairs)).astype(np.float32)
    return out


def peak_records(planes, method):
    """Per plane (dx, dy, score): the first cell in row-major order holding the maximum (methods 0 and 1: the minimum)
    over the cells that are not NaN, -0 comparing equal to +0, the score the cell's own float32; (-1, -1, NaN) for a plane
    without a number (which sits at displacement (-1, -1) only by that convention)."""
    side = planes.shape[1]
    m = side // 2
    out = []
    for pl in planes:
        best = None
        for cy in range(side):
            for cx in range(side):
                v = pl[cy, cx]
                if np.isnan(v):
                    continue
                if best is None or (v < best[0] if method in (0, 1) else v > best[0]):
                    best = (v, cx, cy)
        out.append((-1, -1, np.float32(np.nan)) if best is None else (best[1] - m, best[2] - m, np.float32(best[0])))
    return out


def loop_pairs(multipass, frames, passes, method, reference, refine):
    """matchBlocksStackMultipass(ensemble=False) by hand: `multipass` (MTM.matchBlocksMultipass) over the pairs."""
    mode = FIRST if reference == "first" else PREVIOUS
    per_pair = [multipass(frames[r], frames[s], passes, method, refine=refine) for r, s in S.pair_frames(len(frames), mode)]
    return [(per_pair[0][p][0], np.stack([q[p][1] for q in per_pair]), np.stack([q[p][2] for q in per_pair]))
            for p in range(len(passes))]


def loop_ensemble(stack, frames, passes, method, reference, refine):
    """matchBlocksStackMultipass(ensemble=True) by hand, as its docstring writes it: `stack` (MTM.matchBlocksStack) pass after
    pass, the integer ensemble peaks steering the next."""
    shape = frames[0].shape
    out, steer = [], None
    for p, (block, step, margin) in enumerate(passes):
        b = B.grid(shape, block, step)
        off = None if p == 0 else B.predict_offsets(shape, passes[p - 1][:2], steer, passes[p][:2])
        steer, _, _ = stack(frames, b, margin, method, reference=reference, ensemble=True, offsets=off)
        pos, sc, planes = stack(frames, b, margin, method, reference=reference, ensemble=True, offsets=off, refine=refine)
        out.append((b, pos, sc, planes))
    return out


class StackOracleCtx(P.OracleCtx):
    """blocks_passes_model's context with the three stack calls on the CPU oracle.  `kinds`: what reached it, in order."""
    def __init__(self, max_floats=1 << 26):
        super().__init__()
        self.max_floats = max_floats
        self.kinds = []

    def get_option(self, opt):
        assert opt == _lib.OPT_BOXES_MAX_FLOATS
        return self.max_floats

    def _records(self, planes, moved, method):
        out = np.zeros(len(planes), dtype=_lib.HIT_DTYPE)
        for k, (dx, dy, s) in enumerate(peak_records(planes, method)):
            out[k] = (k, moved[k][0] + dx, moved[k][1] + dy, moved[k][2], moved[k][3], s)
        return out

    def match_blocks_stack(self, frames, blocks, margin, method, mode, with_nbhd=False, planes=False):
        self.kinds.append(("stack", (frames, blocks.copy(), margin, method, mode), {"with_nbhd": with_nbhd, "planes": planes}))
        frames = [np.ascontiguousarray(f) for f in frames]
        if planes:
            b = np.stack([blocks[f] for f in "xywh"], axis=1)
            return S.planes(O.compute_score_map, frames, b, margin, method, mode)
        res = [self.match_blocks(frames[r], frames[s], blocks, margin, method, with_nbhd)
               for r, s in S.pair_frames(len(frames), mode)]
        return np.concatenate([r[0] for r in res]), (np.concatenate([r[1] for r in res]) if with_nbhd else None)

    def match_blocks_stack_at(self, frames, blocks, offsets, margin, method, mode, with_nbhd=False, planes=False):
        assert offsets.dtype == np.int32 and offsets.shape == (len(blocks), 2)
        self.kinds.append(("stack_at", (frames, blocks.copy(), offsets.copy(), margin, method, mode),
                           {"with_nbhd": with_nbhd, "planes": planes}))
        frames = [np.ascontiguousarray(f) for f in frames]
        if planes:
            b = np.stack([blocks[f] for f in "xywh"], axis=1)
            pl = planes_at(O.compute_score_map, frames, b, offsets, margin, method, mode)
            return pl, self._records(pl, moved_brute(b, offsets, frames[0].shape).tolist(), method)
        res = [self._run(frames[r], frames[s], blocks, offsets, margin, method, with_nbhd)
               for r, s in S.pair_frames(len(frames), mode)]
        return np.concatenate([r[0] for r in res]), (np.concatenate([r[1] for r in res]) if with_nbhd else None)

    def match_blocks_stack_passes(self, frames, passes, counts, method, mode, with_nbhd=False, planes=False):
        assert passes.dtype == _lib.BLOCK_PASS_DTYPE
        self.kinds.append(("stack_passes", (frames, passes.copy(), list(counts), method, mode),
                           {"with_nbhd": with_nbhd, "planes": planes}))
        frames = [np.ascontiguousarray(f) for f in frames]
        shape = frames[0].shape
        if not planes:
            res = [self.match_blocks_passes(frames[r], frames[s], passes, counts, method, with_nbhd)
                   for r, s in S.pair_frames(len(frames), mode)]
            return np.concatenate([r[0] for r in res]), (np.concatenate([r[1] for r in res]) if with_nbhd else None)
        flat, recs, prev = [], [], None
        for p, a in enumerate(passes):
            spec = ((int(a["bw"]), int(a["bh"])), (int(a["sx"]), int(a["sy"])))
            g = B.grid(shape, *spec)
            assert len(g) == counts[p]
            off = np.zeros((len(g), 2), np.int64)
            if p:
                cg = B.grid(shape, *prev[0])
                near = P.nearest_brute(shape, prev[0], spec)
                off = prev[1][near] - cg[near, :2]
            pl = planes_at(O.compute_score_map, frames, g, off, int(a["margin"]), method, mode)
            rec = self._records(pl, moved_brute(g, off, shape).tolist(), method)
            prev = (spec, np.stack((rec["x"], rec["y"]), axis=1).astype(np.int64))
            flat.append(pl.reshape(-1))
            recs.append(rec)
        return np.concatenate(flat), np.concatenate(recs)


F32_MAX = float(np.finfo(np.float32).max)


def plane_cases(side, pairs, seed):
    """Constructed planes of sums for the plane-peak kernel: (acc (N, side, side) float64, clip (N, 2) int32 of (ox, oy),
    oh (N,), ow (N,)).  Random sums in boxes clipped on each side in turn and on all; a flat plane whose extremum - for
    either direction - is tied at the first, the middle and the last cell, at the middle and the last, at the last alone;
    zeros of both signs (a -0 first, a +0 first); a single valid cell at every corner and in the middle; +-inf, the
    largest float32 and values that round to infinity; a box without a cell."""
    rng = np.random.RandomState(seed)
    last = side - 1
    mid = side // 2
    acc, clip, oh, ow = [], [], [], []

    def add(a, ox=0, oy=0, h=side, w=side):
        acc.append(np.asarray(a, dtype=np.float64).reshape(side, side))
        clip.append((ox, oy))
        oh.append(h)
        ow.append(w)

    cut = min(2, last)
    for ox, oy, h, w in ((0, 0, side, side), (cut, 0, side, side - cut), (0, cut, side - cut, side), (0, 0, side, side - cut),
                         (0, 0, side - cut, side), (cut, cut, side - 2 * cut if side > 2 * cut else 1, side - 2 * cut if side > 2 * cut else 1)):
        add(rng.uniform(-1, 1, size=(side, side)) * pairs, ox, oy, max(h, 1), max(w, 1))
    cells = [(0, 0), (mid, mid), (last, last)]
    for keep in (cells, cells[1:], cells[2:]):
        for sign in (1.0, -1.0):                    # a tied maximum, and a tied minimum
            a = np.full((side, side), 0.25 * pairs)
            for cy, cx in keep:
                a[cy, cx] += sign * 0.5 * pairs
            add(a)
    a = np.full((side, side), -0.0)
    a[mid, mid] = 0.0
    add(a)                                          # -0 first: the peak is cell 0 and its score stays -0
    a = np.full((side, side), 0.0)
    a[last, last] = -0.0
    add(a)
    for cy, cx in ((0, 0), (0, last), (last, 0), (last, last), (mid, mid)):
        add(rng.uniform(-1, 1, size=(side, side)) * pairs, cx, cy, 1, 1)
    a = rng.uniform(-1, 1, size=(side, side)) * pairs
    a[mid, last] = np.inf
    a[last, mid] = -np.inf
    add(a)
    a = rng.uniform(-1, 1, size=(side, side)) * pairs
    a[0, last] = F32_MAX * pairs
    a[last, 0] = -F32_MAX * pairs
    a[mid, mid] = 2.0 * F32_MAX * pairs             # (rounds to +inf as a float32)
    add(a)
    add(np.full((side, side), -np.inf))             # every number is the infinity that loses (or wins)
    add(rng.uniform(-1, 1, size=(side, side)), 0, 0, 0, 0)      # no cell: a plane without a number
    return (np.stack(acc), np.array(clip, dtype=np.int32), np.array(oh, dtype=np.int32), np.array(ow, dtype=np.int32))
