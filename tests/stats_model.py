"""The fused uint8 window statistics kernel (csrc/mtm_k_stats.hip.h, stats_u8_kernel) restated in numpy, bit for bit.

Every output is an exact integer below 2^53 or a fixed sequence of correctly rounded float64 operations on such integers, so
the model is compared with `==` on the bytes: window sums from int64 integral images, window_norm in the kernel's operation
order, the records per 16-pixel column block and the tail boxes of even and odd output rows as the kernel's comments define
them.  What the model leaves out is how the kernel spreads the work (its forms): that must not show."""
import numpy as np

UNIT_ROWS = 8                   # kStatBand4
FLT_EPSILON = float(np.finfo(np.float32).eps)


def geometry(rows, cols, h, w):
    oh, ow = rows - h + 1, cols - w + 1
    st_pitch = (ow + 3) // 4 * 4
    return {"oh": oh, "ow": ow, "st_pitch": st_pitch, "blk_pitch": (st_pitch + 15) // 16,
            "pitch": (cols + 512 + 63) // 64 * 64, "units": (oh + UNIT_ROWS - 1) // UNIT_ROWS}


def _box_sums(a, r0, nrows, w, ncols):
    """int64 sums of a[y + r0 : y + r0 + nrows(y), x : x + w] for every row y the box fits and x < ncols: through an
    integral image (a is already padded on the right)."""
    ii = np.zeros((a.shape[0] + 1, a.shape[1] + 1), dtype=np.int64)
    ii[1:, 1:] = np.cumsum(np.cumsum(a, axis=0), axis=1)
    n = a.shape[0] - r0 - nrows + 1
    top, bot = ii[r0:r0 + n], ii[r0 + nrows:r0 + nrows + n]
    return bot[:, w:w + ncols] - bot[:, :ncols] - top[:, w:w + ncols] + top[:, :ncols]


def window_norm(sum2, mean2):
    """csrc/mtm_device_util.hip.h: sqrt(sum2 - mean2), zero where the window is flat to float32 precision."""
    diff2 = np.maximum(sum2 - mean2, 0.0)
    small = diff2 <= np.minimum(0.5, (10.0 * FLT_EPSILON) * sum2)
    return np.where(small, 0.0, np.sqrt(diff2))


def window_stats(image, h, w, num_type, tail_s=0):
    """-> dict(t0, sum2, sq, rsq: (oh, st_pitch) float64 - the pitch columns right of ow hold the windows that run into the
    image's zero padding, as the kernel writes them; blk (oh, blk_pitch, 4); blkq likewise when tail_s > 0)."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 2
    rows, cols = image.shape
    g = geometry(rows, cols, h, w)
    oh, ow, sp, bp = g["oh"], g["ow"], g["st_pitch"], g["blk_pitch"]
    a = np.zeros((rows, sp + w), dtype=np.int64)
    a[:, :cols] = image
    s1, s2 = _box_sums(a, 0, h, w, sp), _box_sums(a * a, 0, h, w, sp)
    assert s1.shape == (oh, sp) and int(s2.max(initial=0)) < 2 ** 32
    t0, sum2 = s1.astype(np.float64), s2.astype(np.float64)
    inv_area = 1.0 / (float(h) * float(w))
    mean2 = (t0 * t0) * inv_area if num_type == 1 else np.zeros_like(t0)
    sq = window_norm(sum2, mean2)
    with np.errstate(divide="ignore"):
        rsq = np.where(sq > 0.0, 1.0 / sq, 0.0)
    out = {"t0": t0, "sum2": sum2, "sq": sq, "rsq": rsq}

    def blocks(v, fill, reduce):
        """v (oh, sp) -> (oh, bp): `reduce` over the output columns x < ow of every 16-column block, `fill` for a block without."""
        full = np.full((oh, bp * 16), fill, dtype=v.dtype)
        full[:, :ow] = v[:, :ow]
        return reduce(full.reshape(oh, bp, 16), axis=2)

    big = np.iinfo(np.int64).max
    lo = blocks(s1, big, np.min)
    blk = np.zeros((oh, bp, 4), dtype=np.float64)
    blk[:, :, 0] = np.where(lo == big, 0, lo).astype(np.float64)
    blk[:, :, 1] = blocks(s1, 0, np.max).astype(np.float64)
    blk[:, :, 2] = blocks(sq, np.inf, np.min)
    out["blk"] = blk
    if tail_s:
        # even output row y: image rows y + s .. y + h - 1; odd y: those of its pair's even row plus one, y + s - 1 .. y + h - 1
        assert 1 <= tail_s <= h - 1
        q1, q2 = np.zeros((oh, sp), dtype=np.int64), np.zeros((oh, sp), dtype=np.int64)
        ev1, ev2 = _box_sums(a, tail_s, h - tail_s, w, sp), _box_sums(a * a, tail_s, h - tail_s, w, sp)
        od1, od2 = _box_sums(a, tail_s - 1, h - tail_s + 1, w, sp), _box_sums(a * a, tail_s - 1, h - tail_s + 1, w, sp)
        q1[0::2], q2[0::2] = ev1[0:oh:2], ev2[0:oh:2]
        q1[1::2], q2[1::2] = od1[1:oh:2], od2[1:oh:2]
        nq = np.where(np.arange(oh) % 2 == 1, (h - tail_s + 1) * w, (h - tail_s) * w).astype(np.float64)[:, None]
        a1 = q1.astype(np.float64)
        v = nq * q2.astype(np.float64) - a1 * a1                        # |Q| S2_Q - S1_Q^2: exact
        vm = blocks(v, 0.0, np.max)
        loq = blocks(q1, big, np.min)
        blkq = np.zeros((oh, bp, 4), dtype=np.float64)
        blkq[:, :, 0] = np.where(loq == big, 0, loq).astype(np.float64)
        blkq[:, :, 1] = blocks(q1, 0, np.max).astype(np.float64)
        blkq[:, :, 2] = np.sqrt(vm * (1.0 / nq)) * (1.0 + 2.0 ** -49)
        out["blkq"] = blkq
    return out


def converted_planes(image, r0, r1, pattern):
    """The two planes of a launch that converts image rows r0 .. r1 - 1 on the way (pitch as the context lays them out):
    the uint8 plane and its int8 view (byte ^ 0x80); every other byte keeps `pattern`."""
    rows, cols = image.shape
    pitch = (cols + 512 + 63) // 64 * 64
    u8 = np.full((rows, pitch), pattern, dtype=np.uint8)
    u8b = np.full((rows, pitch), pattern, dtype=np.uint8)
    u8[r0:r1, :cols] = image[r0:r1]
    u8b[r0:r1, :cols] = image[r0:r1] ^ 0x80
    return u8, u8b
