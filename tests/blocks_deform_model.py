"""Restatements for MTM.blocks.displacement_field / field_at / deform and MTM.matchBlocksMultipass(deform=True) that share no
code with them: the field and the warp pixel by pixel in Python integers, the grids, fields and images their tests sweep,
the sheared pair, the by-hand loop the deformed call documents, and blocks_validate_model's oracle context extended with the
deformed passes call."""
import numpy as np

import blocks_validate_model as V
from MTM import _lib
from MTM import blocks as B


def _axes(shape, coarse):
    (bw, bh), (sx, sy) = coarse
    H, W = shape[:2]
    return bw, bh, sx, sy, (W - bw) // sx + 1, (H - bh) // sy + 1


def _axis(n, s, wc, X2):
    if n == 1:
        return 0, 0
    i = min(max((X2 - (wc - 1)) // (2 * s), 0), n - 2)
    a = min(max(X2 - (2 * i * s + wc - 1), 0), 2 * s)
    return i, (256 * a + s) // (2 * s)


def field_point(shape, coarse, disp, X2, Y2):
    """(Fx, Fy) in Q8 at the doubled point (X2, Y2), by the rule as the issue states it, in Python integers."""
    wc, hc, sx, sy, nx, ny = _axes(shape, coarse)
    d = [(int(a), int(b)) for a, b in np.asarray(disp).tolist()]
    assert len(d) == nx * ny
    i, ax = _axis(nx, sx, wc, X2)
    j, ay = _axis(ny, sy, hc, Y2)
    i1, j1 = min(i + 1, nx - 1), min(j + 1, ny - 1)
    out = []
    for c in (0, 1):
        s = (d[j * nx + i][c] * (256 - ax) * (256 - ay) + d[j * nx + i1][c] * ax * (256 - ay)
             + d[j1 * nx + i][c] * (256 - ax) * ay + d[j1 * nx + i1][c] * ax * ay + 128)
        out.append(s >> 8)              # (Python's >> on a negative integer is a floor)
    return tuple(out)


def field_brute(shape, coarse, disp):
    H, W = shape[:2]
    out = np.zeros((H, W, 2), dtype=np.int64)
    for y in range(H):
        for x in range(W):
            out[y, x] = field_point(shape, coarse, disp, 2 * x, 2 * y)
    return out


def field_at_brute(shape, coarse, disp, blocks):
    return np.array([field_point(shape, coarse, disp, 2 * x + w - 1, 2 * y + h - 1) for x, y, w, h in
                     np.asarray(blocks).tolist()], dtype=np.int64).reshape(-1, 2)


def deform_brute(image, field):
    img = np.asarray(image)
    H, W = img.shape[:2]
    px = img.reshape(H, W, -1).tolist()
    f = np.asarray(field).tolist()
    out = np.zeros((H, W, len(px[0][0])), dtype=img.dtype)
    for y in range(H):
        for x in range(W):
            X = min(max(256 * x + f[y][x][0], 0), 256 * (W - 1))
            Y = min(max(256 * y + f[y][x][1], 0), 256 * (H - 1))
            x0, fx, y0, fy = X >> 8, X & 255, Y >> 8, Y & 255
            x1, y1 = min(x0 + 1, W - 1), min(y0 + 1, H - 1)
            for c in range(out.shape[2]):
                out[y, x, c] = (px[y0][x0][c] * (256 - fx) * (256 - fy) + px[y0][x1][c] * fx * (256 - fy)
                                + px[y1][x0][c] * (256 - fx) * fy + px[y1][x1][c] * fx * fy + 32768) >> 16
    return out.reshape(img.shape)


# (shape, coarse = ((bw, bh), (sx, sy))): coarse grids of 1 x 1, 1 x n, n x 1, 3 x 4 and 5 x 7 blocks; odd and even
# block sizes, steps that differ from the block
GRIDS = (
    ((23, 29), ((29, 23), (29, 23))),           # 1 x 1
    ((20, 41), ((9, 20), (8, 5))),              # 1 row of 5
    ((37, 12), ((12, 8), (3, 7))),              # 1 column of 5
    ((29, 41), ((8, 9), (11, 7))),              # 3 rows of 4
    ((33, 53), ((10, 7), (7, 6))),              # 5 rows of 7
)
GRID_COUNTS = ((1, 1), (5, 1), (1, 5), (4, 3), (7, 5))      # (nx, ny) of each


# the same five grid kinds over the two image sizes of the GPU tests: 67 x 131 (partial work-groups at both edges, pitch
# padding) and 96 x 120
GPU_GRIDS = {
    (67, 131): (((131, 67), (131, 67)), ((31, 67), (25, 9)), ((131, 11), (7, 14)), ((32, 20), (33, 23)), ((17, 12), (19, 13))),
    (96, 120): (((120, 96), (120, 96)), ((24, 96), (24, 8)), ((120, 16), (7, 20)), ((32, 32), (29, 32)), ((16, 16), (17, 20))),
}
WIDE = ((40, 600), ((100, 16), (160, 11)))      # three work-groups along a row, the last one partly filled; 3 rows of 4


def grid_counts(shape, coarse):
    _, _, _, _, nx, ny = _axes(shape, coarse)
    return nx, ny


def fields(shape, coarse, seed):
    """The displacement sets of one grid: zero; integer constants; negative with fractional weights; random in [-5, 5];
    +-10^4 (every sample clamps)."""
    nx, ny = grid_counts(shape, coarse)
    n = nx * ny
    rng = np.random.RandomState(seed)
    out = [np.zeros((n, 2), np.int64), np.tile(np.array([[3, -2]], np.int64), (n, 1)),
           np.tile(np.array([[-4, 5]], np.int64), (n, 1))]
    neg = -(np.arange(2 * n, dtype=np.int64).reshape(n, 2) % 7) - 1
    out.append(neg)
    out += [rng.randint(-5, 6, size=(n, 2)).astype(np.int64) for _ in range(2)]
    out.append(np.where(rng.randint(0, 2, size=(n, 2)) == 1, 10 ** 4, -10 ** 4).astype(np.int64))
    return out


def image(shape, kind, seed):
    """Random pixels of one of the three kinds, the extreme values 0 and 255 / 65535 planted."""
    rng = np.random.RandomState(seed)
    top = 65536 if kind == "u16" else 256
    full = tuple(shape[:2]) + ((3,) if kind == "rgb" else ())
    a = rng.randint(0, top, full).astype(np.uint16 if kind == "u16" else np.uint8)
    a[0, 0], a[-1, -1], a[0, -1], a[shape[0] // 2, shape[1] // 2] = 0, top - 1, top - 1, top - 1
    a[shape[0] // 2, shape[1] // 2 + 1] = 0
    return a


def smooth_texture(shape, seed, kind="u8"):
    """A smooth random texture: white noise box-filtered twice (integers), stretched to the pixel range."""
    rng = np.random.RandomState(seed)
    H, W = shape
    a = rng.randint(0, 256, (H + 12, W + 12)).astype(np.int64)
    for _ in range(2):
        a = a[:-3] + a[1:-2] + a[2:-1] + a[3:]
        a = a[:, :-3] + a[:, 1:-2] + a[:, 2:-1] + a[:, 3:]
    a = a[:H, :W].astype(np.float64)
    a = (a - a.min()) / (a.max() - a.min())
    if kind == "u16":
        return np.round(a * 65535).astype(np.uint16)
    g = np.round(a * 255).astype(np.uint8)
    return np.stack((g, 255 - g, g // 2 + 60), axis=2) if kind == "rgb" else g


def sheared_pair(shape=(160, 192), g=0.12, seed=3, kind="u8"):
    """(reference, image): a smooth texture and the same texture sheared by dx = g (y - H / 2), resampled linearly along
    x in float64 from a wider texture so that no edge enters."""
    H, W = shape
    pad = int(np.ceil(abs(g) * H / 2)) + 2
    wide = smooth_texture((H, W + 2 * pad), seed, kind).astype(np.float64)
    ref = wide[:, pad:pad + W]
    img = np.empty_like(ref)
    for y in range(H):
        # image(x) = reference(x - dx): the content of row y moved by dx to the right
        src = np.arange(W) + pad - g * (y - H / 2)
        x0 = np.floor(src).astype(int)
        t = (src - x0).reshape((W,) + (1,) * (wide.ndim - 2))
        img[y] = wide[y, x0] * (1 - t) + wide[y, x0 + 1] * t
    dt = np.uint16 if kind == "u16" else np.uint8
    return np.round(ref).astype(dt), np.round(img).astype(dt)


def interior(blocks, shape, border):
    """The blocks at least `border` pixels from every edge of the image."""
    x, y, w, h = (blocks[:, i] for i in range(4))
    return (x >= border) & (y >= border) & (x + w <= shape[1] - border) & (y + h <= shape[0] - border)


def clip_passes(passes, shape):
    """The passes whose block fits the image."""
    return [p for p in passes if p[0] <= min(shape[0], shape[1])]


def by_hand(ref, img, passes, method, validate=None, refine=False, context=None, deform=B.deform,
            displacement_field=B.displacement_field, field_at=B.field_at):
    """The loop matchBlocksMultipass(deform=True) documents, through matchBlocks: one (blocks, positions, scores[, valid],
    predicted) per pass."""
    out, steer = [], None
    for p, (block, step, margin) in enumerate(passes):
        b = B.grid(img.shape, block, step)
        if p == 0:
            searched, c = img, np.zeros((len(b), 2), np.int64)
        else:
            prev = passes[p - 1][:2]
            d = steer - B.grid(img.shape, *prev)[:, :2]
            searched = deform(img, displacement_field(img.shape, prev, d))
            c = field_at(img.shape, prev, d, b)
        pos_w, sc = B.matchBlocks(ref, searched, b, margin, method, context=context)
        pos = pos_w + ((c + 128) >> 8)
        fine = pos
        if refine:
            fine = B.matchBlocks(ref, searched, b, margin, method, refine=True, context=context)[0] + c / 256.0
        res = (b, fine, sc)
        if validate is None:
            steer = pos
        else:
            valid, rep = B.validate(B.grid_shape(img.shape, block, step), pos - b[:, :2], *validate)
            steer = b[:, :2] + rep
            res += (valid,)
        out.append(res + (c / 256.0,))
    return out


class OracleCtx(V.OracleCtx):
    """blocks_validate_model.OracleCtx with the deformed passes call composed as the native call documents it, on the
    brute-force field and warp above: every pass p >= 1 searches the original image warped by the field of the records
    that steer it, with zero offsets, and its records are moved by the field at the blocks' centres."""
    def match_blocks_passes(self, reference, image, passes, counts, method, with_nbhd=False, **kw):
        if not kw.get("deform"):
            kw.pop("deform", None)
            return super().match_blocks_passes(reference, image, passes, counts, method, with_nbhd, **kw)
        kw.pop("deform")
        validate = kw.pop("validate", None)
        assert not kw and passes.dtype == _lib.BLOCK_PASS_DTYPE
        self.calls.append(("deformed", passes.copy(), list(counts), method, with_nbhd, validate))
        outs, nbs, flags, preds, prev = [], [], [], [], None
        for p, a in enumerate(passes):
            spec = ((int(a["bw"]), int(a["bh"])), (int(a["sx"]), int(a["sy"])))
            g = B.grid(image.shape, *spec)
            assert len(g) == counts[p]
            searched, c = image, np.zeros((len(g), 2), np.int64)
            if p:
                d = prev[1] - B.grid(image.shape, *prev[0])[:, :2]
                searched = deform_brute(image, field_brute(image.shape, prev[0], d))
                c = field_at_brute(image.shape, prev[0], d, g)
            out, nb = self._run(reference, searched, _lib.block_records(g), np.zeros((len(g), 2), np.int64), int(a["margin"]),
                                method, with_nbhd)
            out["x"] += ((c[:, 0] + 128) >> 8).astype(np.int32)
            out["y"] += ((c[:, 1] + 128) >> 8).astype(np.int32)
            pos = np.stack((out["x"], out["y"]), axis=1).astype(np.int64)
            steer = pos
            if validate is not None:
                ny, nx = len(np.unique(g[:, 1])), len(np.unique(g[:, 0]))
                valid, rep = V.validate_brute((ny, nx), pos - g[:, :2], *validate)
                steer = g[:, :2] + np.array(rep, dtype=np.int64).reshape(-1, 2)
                flags.append(np.array(valid, dtype=bool))
            prev = (spec, steer)
            outs.append(out)
            nbs.append(nb)
            preds.append(c.astype(np.int32))
        res = (np.concatenate(outs), (np.concatenate(nbs) if with_nbhd else None))
        if validate is not None:
            res += (np.concatenate(flags),)
        return res + (np.concatenate(preds),)
