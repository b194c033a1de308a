"""Numpy restatements for MTM.matchBlocks(offsets=) / MTM.matchBlocksMultipass without a GPU: the nearest coarse block by
brute force, the host plan of a mtm_match_blocks_passes call (its fixed tile table and chunk split), and a context that runs
the three native block calls on the CPU oracle."""
import threading

import numpy as np

import mtm_oracle as O
from MTM import _lib
from MTM import blocks as B

TILE = 16


def nearest_brute(shape, coarse, fine):
    """For every block of grid(shape, *fine) the index of the block of grid(shape, *coarse) whose centre is nearest, per
    axis, by search over every coarse block on doubled integer centres; of equally near ones the highest index."""
    cg, fg = B.grid(shape, *coarse), B.grid(shape, *fine)
    xs, ys = np.unique(cg[:, 0]), np.unique(cg[:, 1])
    wc, hc = int(cg[0, 2]), int(cg[0, 3])
    out = np.empty(len(fg), dtype=np.int64)
    for k, (x, y, w, h) in enumerate(fg.tolist()):
        dx = np.abs(2 * xs + wc - (2 * x + w))
        dy = np.abs(2 * ys + hc - (2 * y + h))
        ix = len(xs) - 1 - int(np.argmin(dx[::-1]))         # (the last of the minima)
        iy = len(ys) - 1 - int(np.argmin(dy[::-1]))
        out[k] = iy * len(xs) + ix
    return out


def plan(shape, chans, dtype, passes, budget_bytes):
    """(counts (P,); tiles (n, 4) of (pass, block, ty0, tx0); chunk_of, pass-major) of `passes` = (bw, bh, sx, sy, margin)
    records for images of `shape`: ceil((2 margin + 1) / 16)^2 tiles per block whatever its map (per axis never more than
    the block's map over the whole image has), chunks of whole blocks by template bytes within each pass."""
    per_pixel = 2 if np.dtype(dtype) == np.uint16 else int(chans)
    counts, tiles, chunk_of = [], [], []
    for p, (bw, bh, sx, sy, margin) in enumerate(passes):
        g = B.grid(shape, (bw, bh), (sx, sy))
        counts.append(len(g))
        th, tw = min(2 * margin + 1, shape[0] - bh + 1), min(2 * margin + 1, shape[1] - bw + 1)
        chunk, used = 0, 0
        for k in range(len(g)):
            nbytes = bw * bh * per_pixel
            if k and used + nbytes > budget_bytes:
                chunk, used = chunk + 1, 0
            used += nbytes
            chunk_of.append(chunk)
            tiles += [(p, k, ty, tx) for ty in range(0, th, TILE) for tx in range(0, tw, TILE)]
    return (np.array(counts, dtype=np.int64), np.array(tiles, dtype=np.int32).reshape(-1, 4),
            np.array(chunk_of, dtype=np.int32))


def _cut(smap, x, y):
    out = np.full((3, 3), np.nan, dtype=np.float32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if 0 <= y + dy < smap.shape[0] and 0 <= x + dx < smap.shape[1]:
                out[1 + dy, 1 + dx] = smap[y + dy, x + dx]
    return out


class OracleCtx:
    """match_blocks, match_blocks_at and match_blocks_passes on the CPU oracle: per block O.find_matches(..., N_object=1,
    searchBox=search_box_at(...)) of the block cut out of the reference, and its neighbourhood cut out of the oracle's
    whole-image score map; the passes composed as the native call documents them.  Records what reaches it."""
    def __init__(self):
        self.lock = threading.RLock()
        self.calls = []

    def _run(self, reference, image, blocks, offsets, margin, method, with_nbhd):
        n = len(blocks)
        out = np.zeros(n, dtype=_lib.HIT_DTYPE)
        nbhd = np.empty((n, 3, 3), dtype=np.float32) if with_nbhd else None
        ref, img = np.ascontiguousarray(reference), np.ascontiguousarray(image)
        for k, b in enumerate(blocks):
            x, y, w, h = (int(b[f]) for f in "xywh")
            t = ref[y:y + h, x:x + w]
            box = B.search_box_at((x, y, w, h), offsets[k], margin, img.shape)
            (_, (hx, hy, hw, hh), s), = O.find_matches([("b", t)], img, method, 1, searchBox=box)
            out[k] = (k, hx, hy, hw, hh, s)
            if with_nbhd:
                nbhd[k] = _cut(O.compute_score_map(t, img, method), hx, hy)
        return out, nbhd

    def match_blocks(self, reference, image, blocks, margin, method, with_nbhd=False):
        self.calls.append(("plain", blocks.copy(), None, margin, method, with_nbhd))
        return self._run(reference, image, blocks, np.zeros((len(blocks), 2), np.int64), margin, method, with_nbhd)

    def match_blocks_at(self, reference, image, blocks, offsets, margin, method, with_nbhd=False):
        assert offsets.dtype == np.int32 and offsets.shape == (len(blocks), 2)
        self.calls.append(("at", blocks.copy(), offsets.copy(), margin, method, with_nbhd))
        return self._run(reference, image, blocks, offsets, margin, method, with_nbhd)

    def match_blocks_passes(self, reference, image, passes, counts, method, with_nbhd=False):
        assert passes.dtype == _lib.BLOCK_PASS_DTYPE
        self.calls.append(("passes", passes.copy(), list(counts), method, with_nbhd))
        outs, nbs, prev = [], [], None
        for p, a in enumerate(passes):
            spec = ((int(a["bw"]), int(a["bh"])), (int(a["sx"]), int(a["sy"])))
            g = B.grid(image.shape, *spec)
            assert len(g) == counts[p]
            off = np.zeros((len(g), 2), np.int64)
            if p:
                cg = B.grid(image.shape, *prev[0])
                near = nearest_brute(image.shape, prev[0], spec)
                off = prev[1][near] - cg[near, :2]
            out, nb = self._run(reference, image, _lib.block_records(g), off, int(a["margin"]), method, with_nbhd)
            prev = (spec, np.stack((out["x"], out["y"]), axis=1).astype(np.int64))
            outs.append(out)
            nbs.append(nb)
        return np.concatenate(outs), (np.concatenate(nbs) if with_nbhd else None)

    def __getattr__(self, name):            # (anything else - set_templates above all - is not the call's business)
        raise AssertionError("the block calls used the context's %s" % name)
