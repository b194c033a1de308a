"""A plain restatement of MTM.matchBlocksStack (mtm_match_blocks_stack) for its tests: the frame chunks of the
host plan (plan_blocks_stack, mtm_host.cpp), every block's clip offsets, the ensemble planes from per-block score maps of
host-cut crops, and the peak rule of MTM.blocks.plane_peaks - loops over cells, nothing shared with the code under test."""
import numpy as np

PREVIOUS, FIRST = 0, 1


def chunks(n_frames, frames_per_chunk, mode):
    """(n, 4) int32 of (f0, nf, carried, p0): a chunk uploads [frame carried, frames f0 .. f0 + nf - 1] and runs the pairs
    p0 .. p0 + nf - 1 (pair p searches frame p + 1; its reference is frame p, or frame 0 in mode FIRST)."""
    new = max(2, frames_per_chunk) - 1
    out = []
    f0 = 1
    while f0 < n_frames:
        nf = min(new, n_frames - f0)
        out.append((f0, nf, 0 if mode == FIRST else f0 - 1, f0 - 1))
        f0 += nf
    return np.array(out, dtype=np.int32).reshape(-1, 4)


def search_box(block, margin, shape):
    x, y, w, h = (int(v) for v in block)
    x0, y0 = max(0, x - margin), max(0, y - margin)
    x1, y1 = min(int(shape[1]), x + w + margin), min(int(shape[0]), y + h + margin)
    return x0, y0, x1 - x0, y1 - y0


def clip(shape, blocks, margin):
    """(N, 2) int32 of (ox, oy): how many columns / rows of the margin the frame cut off at the left / top of each box."""
    out = []
    for b in np.asarray(blocks, dtype=np.int64).reshape(-1, 4).tolist():
        x0, y0, _, _ = search_box(b, margin, shape)
        out.append((margin - (b[0] - x0), margin - (b[1] - y0)))
    return np.array(out, dtype=np.int32).reshape(-1, 2)


def pair_frames(n_frames, mode):
    """[(reference frame, searched frame)] of the pairs in order."""
    return [(0 if mode == FIRST else p, p + 1) for p in range(n_frames - 1)]


def planes(score_map, frames, blocks, margin, method, mode):
    """The ensemble planes: per pair and block score_map(host-cut block, host-cut search-box crop, method) placed at the
    clip offsets, summed in float64 in pair order starting from the first pair's own value, divided by the number of
    pairs and rounded to float32; NaN where no pair has an output (the same cells for every pair)."""
    side = 2 * margin + 1
    blocks = np.asarray(blocks, dtype=np.int64).reshape(-1, 4).tolist()
    offs = clip(frames[0].shape, blocks, margin)
    total = None
    pairs = pair_frames(len(frames), mode)
    for r, s in pairs:
        one = np.full((len(blocks), side, side), np.nan, dtype=np.float64)
        for k, (x, y, w, h) in enumerate(blocks):
            x0, y0, bw, bh = search_box((x, y, w, h), margin, frames[0].shape)
            m = score_map(np.ascontiguousarray(frames[r][y:y + h, x:x + w]),
                          np.ascontiguousarray(frames[s][y0:y0 + bh, x0:x0 + bw]), method)
            m = np.asarray(m)
            assert m.dtype == np.float32 and m.shape == (bh - h + 1, bw - w + 1)
            ox, oy = offs[k]
            one[k, oy:oy + m.shape[0], ox:ox + m.shape[1]] = m.astype(np.float64)
        total = one if total is None else total + one
    return (total / float(len(pairs))).astype(np.float32)


def peaks(pl, blocks, method):
    """(positions int64 (N, 2), scores float32 (N,), cells [(cy, cx)]): per plane the first cell in row-major order that
    holds the maximum (methods 0 and 1: the minimum) over the cells that are not NaN."""
    blocks = np.asarray(blocks, dtype=np.int64).reshape(-1, 4)
    side = pl.shape[1]
    m = side // 2
    pos, sc, cells = [], [], []
    for k in range(len(pl)):
        best = None
        for cy in range(side):
            for cx in range(side):
                v = pl[k, cy, cx]
                if np.isnan(v):
                    continue
                if best is None or (v < best[0] if method in (0, 1) else v > best[0]):
                    best = (v, cy, cx)
        pos.append((blocks[k, 0] + best[2] - m, blocks[k, 1] + best[1] - m))
        sc.append(best[0])
        cells.append((best[1], best[2]))
    return np.array(pos, dtype=np.int64).reshape(-1, 2), np.array(sc, dtype=np.float32), cells


def peak_neighbourhoods(pl, cells):
    """(N, 3, 3) float32: the plane's cells around each peak, NaN outside the plane."""
    side = pl.shape[1]
    out = np.full((len(pl), 3, 3), np.nan, dtype=np.float32)
    for k, (cy, cx) in enumerate(cells):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if 0 <= cy + dy < side and 0 <= cx + dx < side:
                    out[k, 1 + dy, 1 + dx] = pl[k, cy + dy, cx + dx]
    return out
