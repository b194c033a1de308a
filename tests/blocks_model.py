"""A numpy restatement of the host plan of a mtm_match_blocks call (plan_blocks, mtm_host.cpp): every block's search box and
map, the 16 x 16 tiles over the maps, and the split into chunks of whole blocks by a template-byte budget."""
import numpy as np

TILE = 16


def plan(shape, chans, dtype, blocks, margin, budget_bytes):
    """(tiles (n, 3) of (block, ty0, tx0); chunk_of (N,); toff (N,); maps (N, 4) of (x0, y0, ow, oh)) for images of
    `shape` = (rows, cols)."""
    H, W = int(shape[0]), int(shape[1])
    per_pixel = 2 if np.dtype(dtype) == np.uint16 else int(chans)
    tiles, chunk_of, toff, maps = [], [], [], []
    chunk, used, first = 0, 0, True
    for k, (x, y, w, h) in enumerate(np.asarray(blocks, dtype=np.int64).reshape(-1, 4).tolist()):
        x0, y0 = max(0, x - margin), max(0, y - margin)
        x1, y1 = min(W, x + w + margin), min(H, y + h + margin)
        ow, oh = x1 - x0 - w + 1, y1 - y0 - h + 1
        nbytes = w * h * per_pixel
        if not first and used + nbytes > budget_bytes:      # (a chunk holds at least one block)
            chunk, used = chunk + 1, 0
        first = False
        chunk_of.append(chunk)
        toff.append(used)
        used += nbytes
        maps.append((x0, y0, ow, oh))
        tiles += [(k, ty, tx) for ty in range(0, oh, TILE) for tx in range(0, ow, TILE)]
    return (np.array(tiles, dtype=np.int32).reshape(-1, 3), np.array(chunk_of, dtype=np.int32),
            np.array(toff, dtype=np.int64), np.array(maps, dtype=np.int32).reshape(-1, 4))
