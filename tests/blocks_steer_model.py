"""Restatements for MTM.blocks.to_q8 / smooth_displacements, the Q8 field and MTM.matchBlocksMultipass(deform=True,
steer="refined") that share no code with them: the fit, the Q8 position, the predictor filter and the field of Q8 nodes in
plain Python numbers, the constructed neighbourhoods the steer kernel's tests sweep, the particle pair the accuracy claim is
made on, the by-hand loop the steered call documents, and blocks_deform_model's oracle context extended with the steered
call."""
import math

import numpy as np

import blocks_deform_model as D
from MTM import _lib
from MTM import blocks as B

V = D.V


# ---- the rule in Python numbers --------------------------------------------------------------------------------------------
def fit_axis(a, b, c, method):
    """subpixel.fit_offsets along one axis, on three float32 scores, in Python floats (IEEE float64)."""
    a, b, c = float(np.float32(a)), float(np.float32(b)), float(np.float32(c))
    if method in (0, 1):
        a, b, c = -a, -b, -c
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return 0.0
    d = (a - 2.0 * b) + c
    if not (math.isfinite(d) and b >= a and b >= c and d < 0):
        return 0.0
    return 0.5 * (a - c) / d


def q8_of(p):
    return int(math.floor(256.0 * float(p) + 0.5))


def smooth_brute(grid_shape, d):
    ny, nx = grid_shape
    v = [[(int(a), int(b)) for a, b in row] for row in np.asarray(d).reshape(ny, nx, 2).tolist()]
    out = []
    for j in range(ny):
        for i in range(nx):
            acc = [0, 0]
            for dv, kv in ((-1, 1), (0, 2), (1, 1)):
                for du, ku in ((-1, 1), (0, 2), (1, 1)):
                    node = v[min(max(j + dv, 0), ny - 1)][min(max(i + du, 0), nx - 1)]
                    acc[0] += ku * kv * node[0]
                    acc[1] += ku * kv * node[1]
            out.append(((acc[0] + 8) >> 4, (acc[1] + 8) >> 4))      # (Python's >> on a negative integer is a floor)
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def field_point_q8(shape, coarse, nodes, X2, Y2):
    """(Fx, Fy) in Q8 at the doubled point (X2, Y2) from Q8 nodes, in Python integers."""
    wc, hc, sx, sy, nx, ny = D._axes(shape, coarse)
    s = [(int(a), int(b)) for a, b in np.asarray(nodes).tolist()]
    assert len(s) == nx * ny
    i, ax = D._axis(nx, sx, wc, X2)
    j, ay = D._axis(ny, sy, hc, Y2)
    i1, j1 = min(i + 1, nx - 1), min(j + 1, ny - 1)
    return tuple((s[j * nx + i][c] * (256 - ax) * (256 - ay) + s[j * nx + i1][c] * ax * (256 - ay)
                  + s[j1 * nx + i][c] * (256 - ax) * ay + s[j1 * nx + i1][c] * ax * ay + 32768) >> 16 for c in (0, 1))


def field_brute_q8(shape, coarse, nodes):
    H, W = shape[:2]
    out = np.zeros((H, W, 2), dtype=np.int64)
    for y in range(H):
        for x in range(W):
            out[y, x] = field_point_q8(shape, coarse, nodes, 2 * x, 2 * y)
    return out


def field_at_brute_q8(shape, coarse, nodes, blocks):
    return np.array([field_point_q8(shape, coarse, nodes, 2 * x + w - 1, 2 * y + h - 1) for x, y, w, h in
                     np.asarray(blocks).tolist()], dtype=np.int64).reshape(-1, 2)


def q8_fields(shape, coarse, seed):
    """The Q8 node sets of one grid: zero; 256 times integer constants; fractional negatives; random within +-5 px;
    +-10^4 px (every sample clamps)."""
    nx, ny = D.grid_counts(shape, coarse)
    n = nx * ny
    rng = np.random.RandomState(seed)
    out = [np.zeros((n, 2), np.int64), np.tile(np.array([[3 * 256, -2 * 256]], np.int64), (n, 1))]
    out.append(-(np.arange(2 * n, dtype=np.int64).reshape(n, 2) * 37 % 1789) - 1)
    out += [rng.randint(-5 * 256, 5 * 256 + 1, size=(n, 2)).astype(np.int64) for _ in range(2)]
    out.append(np.where(rng.randint(0, 2, size=(n, 2)) == 1, 256 * 10 ** 4, -256 * 10 ** 4).astype(np.int64) + 77)
    return out


# ---- the steer kernel's constructed inputs ---------------------------------------------------------------------------------
_BIG = float(np.finfo(np.float32).max)
_TINY = float(np.finfo(np.float32).tiny)


def neighbourhoods(n, seed):
    """n constructed 3 x 3 neighbourhoods (as scores of a maximum: negate them for methods 0 and 1), cycling through:
    interior maxima; two equal maxima (an offset of +-0.5); NaN cells (the map's border); flat windows; d >= 0; a centre
    that is not the extremum; float32 extremes; infinities."""
    rng = np.random.RandomState(seed)
    out = np.empty((n, 3, 3), dtype=np.float32)
    for k in range(n):
        kind = k % 10
        nb = (rng.rand(3, 3) * 0.5).astype(np.float32)
        nb[1, 1] = np.float32(0.6 + 0.4 * rng.rand())                   # 0: an interior maximum
        if kind == 1:
            nb[1, 2] = nb[1, 1]                                         # two equal maxima along x: +0.5
        elif kind == 2:
            nb[0, 1] = nb[1, 1]                                         # ... along y: -0.5
        elif kind == 3:
            nb[rng.randint(0, 3), :] = np.nan                           # a border row (the centre's row: no fit at all)
        elif kind == 4:
            nb[:, 0 if k % 20 < 10 else 2] = np.nan                     # a border column
        elif kind == 5:
            nb[:] = np.float32(1.0) if k % 20 < 10 else np.float32(np.nan)      # a flat window (score 1 everywhere / NaN)
        elif kind == 6:
            nb[1, 0] = nb[1, 2] = nb[1, 1]                              # d == 0 along x
            nb[0, 1], nb[2, 1] = nb[1, 1] + np.float32(0.25), nb[1, 1] + np.float32(0.5)       # d > 0 along y
        elif kind == 7:
            nb[1, 2] = nb[1, 1] + np.float32(0.125)                     # the centre is not the extremum
        elif kind == 8:
            nb[1] = (-_BIG, _BIG, _BIG * 0.5) if k % 20 < 10 else (0.0, _TINY, -_TINY)      # float32 extremes
            nb[0, 1], nb[2, 1] = -_BIG, -_BIG
        elif kind == 9:
            nb[1, 0] = -np.inf                                          # not finite: no fit along x
            nb[2, 1] = np.inf
        out[k] = nb
    return out


def steer_inputs(grid_shape, step, seed, method, with_flags):
    """Constructed inputs of mtm_debug_steer_q8 for one grid: (positions, nbhd, predicted, valid, steer_positions)."""
    ny, nx = grid_shape
    n = nx * ny
    rng = np.random.RandomState(seed)
    nb = neighbourhoods(n, seed)
    if method in (0, 1):
        nb = -nb
    blocks = np.stack((np.tile(np.arange(nx) * step[0], ny), np.repeat(np.arange(ny) * step[1], nx)), axis=1).astype(np.int64)
    pred = rng.randint(-2000, 2001, size=(n, 2)).astype(np.int64)
    pred[::7] = (-128, 127)                                             # the record's shift at its rounding edges
    pos = blocks + rng.randint(-9, 10, size=(n, 2)) + ((pred + 128) >> 8)
    valid = steer = None
    if with_flags:
        valid = rng.rand(n) < 0.7
        steer = np.where(valid[:, None], pos, blocks + rng.randint(-6, 7, size=(n, 2)))
    return pos, nb, pred, valid, steer


def steer_brute(grid_shape, step, method, smooth, pos, nb, pred, valid=None, steer=None):
    """What mtm_debug_steer_q8 returns, record by record in Python numbers."""
    ny, nx = grid_shape
    out = []
    for k in range(nx * ny):
        b = ((k % nx) * step[0], (k // nx) * step[1])
        if valid is not None and not valid[k]:
            out.append(tuple(256 * (int(steer[k][c]) - b[c]) for c in (0, 1)))
            continue
        o = (fit_axis(nb[k][1][0], nb[k][1][1], nb[k][1][2], method), fit_axis(nb[k][0][1], nb[k][1][1], nb[k][2][1], method))
        row = []
        for c in (0, 1):
            p = int(pred[k][c])
            pos_w = int(pos[k][c]) - ((p + 128) >> 8)
            row.append(q8_of(float(pos_w) + o[c]) - 256 * b[c] + p)
        out.append(tuple(row))
    d8 = np.array(out, dtype=np.int64).reshape(-1, 2)
    return smooth_brute(grid_shape, d8) if smooth else d8


# ---- the particle pair -----------------------------------------------------------------------------------------------------
PARTICLE_SHAPE = (160, 192)
PARTICLE_PASSES = [(32, 32, 12), (32, 16, 2), (32, 16, 2)]
PARTICLE_ANGLE = 0.02
# (rigid, deform=True, steer="refined") RMS errors of the pair on the CPU oracle, to 4 places (test_blocks_steer_cpu.py pins them)
PARTICLE_RMS_ORACLE = (0.0582, 0.3153, 0.0216)
_PARTICLES = {}


def _render(shape, x, y, amp, sigma):
    H, W = shape
    gx = np.exp(-0.5 * ((np.arange(W)[None, :] - x[:, None]) / sigma) ** 2)
    gy = np.exp(-0.5 * ((np.arange(H)[None, :] - y[:, None]) / sigma) ** 2)
    return np.clip(np.round(200.0 * (gy.T @ (amp[:, None] * gx))), 0, 255).astype(np.uint8)


def particle_pair(angle=PARTICLE_ANGLE, shape=PARTICLE_SHAPE, count=2500, sigma=0.9, seed=11, border=20):
    """(reference, image): `count` Gaussian particles of width sigma rendered at exact positions - uniform over the frame
    plus a border, amplitudes uniform in [0.4, 1], the sum scaled by 200 and clipped to uint8 -, and the same particles
    rotated by `angle` about the frame's centre.  One read-only pair per argument set for the whole session."""
    key = (angle, shape, count, sigma, seed, border)
    if key not in _PARTICLES:
        H, W = shape
        rng = np.random.RandomState(seed)
        x = rng.uniform(-border, W + border, count)
        y = rng.uniform(-border, H + border, count)
        amp = rng.uniform(0.4, 1.0, count)
        cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
        ca, sa = math.cos(angle), math.sin(angle)
        x2 = cx + ca * (x - cx) - sa * (y - cy)
        y2 = cy + sa * (x - cx) + ca * (y - cy)
        pair = (_render(shape, x, y, amp, sigma), _render(shape, x2, y2, amp, sigma))
        for a in pair:
            a.setflags(write=False)
        _PARTICLES[key] = pair
    return _PARTICLES[key]


def rotation_truth(blocks, shape=PARTICLE_SHAPE, angle=PARTICLE_ANGLE):
    """The displacement of every block's centre under the rotation, (N, 2) float64."""
    H, W = shape
    b = np.asarray(blocks, dtype=np.float64)
    rx = b[:, 0] + (b[:, 2] - 1) / 2.0 - (W - 1) / 2.0
    ry = b[:, 1] + (b[:, 3] - 1) / 2.0 - (H - 1) / 2.0
    ca, sa = math.cos(angle), math.sin(angle)
    return np.stack((ca * rx - sa * ry - rx, sa * rx + ca * ry - ry), axis=1)


def rms_error(last, shape=PARTICLE_SHAPE, angle=PARTICLE_ANGLE, border=32):
    """The RMS error (px) of a call's last pass - refined positions - over the blocks at least `border` px from every
    edge, and how many blocks those are."""
    blocks, pos = last[0], last[1]
    inner = D.interior(blocks, shape, border)
    err = (pos - blocks[:, :2])[inner] - rotation_truth(blocks, shape, angle)[inner]
    return float(np.sqrt((err ** 2).sum(axis=1).mean())), int(inner.sum())


def three_rms(ref, img, passes=PARTICLE_PASSES, method=5, context=None, contexts=None):
    """(rigid, deform=True, steered) RMS errors of the three calls, refined; `contexts`: a factory of a fresh context per
    call (the oracle stubs), else `context`."""
    import MTM
    out = []
    for kw in ({}, {"deform": True}, {"deform": True, "steer": "refined"}):
        ctx = contexts() if contexts else context
        res = MTM.matchBlocksMultipass(ref, img, passes, method, refine=True, context=ctx, **kw)
        rms, n = rms_error(res[-1], img.shape)
        assert n == 35
        out.append(rms)
    return tuple(out)


# ---- the by-hand loop and the oracle stub -----------------------------------------------------------------------------------
def by_hand(ref, img, passes, method, validate=None, refine=False, context=None):
    """The loop matchBlocksMultipass(deform=True, steer="refined") documents, through matchBlocks and the numpy helpers: one
    (blocks, positions, scores[, valid], predicted) per pass."""
    out, S8, prev = [], None, None
    for p, (block, step, margin) in enumerate(passes):
        b = B.grid(img.shape, block, step)
        if p == 0:
            searched, c = img, np.zeros((len(b), 2), np.int64)
        else:
            searched = B.deform(img, B.displacement_field(img.shape, prev, S8, q8=True))
            c = B.field_at(img.shape, prev, S8, b, q8=True)
        pos_w, sc = B.matchBlocks(ref, searched, b, margin, method, context=context)
        fine_w, _ = B.matchBlocks(ref, searched, b, margin, method, refine=True, context=context)
        pos = pos_w + ((c + 128) >> 8)
        res = (b, fine_w + c / 256.0 if refine else pos, sc)
        D8 = B.to_q8(fine_w) - 256 * b[:, :2] + c
        if validate is not None:
            valid, rep = B.validate(B.grid_shape(img.shape, block, step), pos - b[:, :2], *validate)
            D8[~valid] = 256 * rep[~valid]
            res += (valid,)
        S8 = B.smooth_displacements(B.grid_shape(img.shape, block, step), D8)
        prev = (block, step)
        out.append(res + (c / 256.0,))
    return out


class OracleCtx(D.OracleCtx):
    """blocks_deform_model.OracleCtx with the steered call composed as the native call documents it, on brute force: the
    fit, the Q8 position and the filter in Python numbers, the field of Q8 nodes and the warp pixel by pixel."""
    def match_blocks_passes(self, reference, image, passes, counts, method, with_nbhd=False, **kw):
        if not kw.get("steer"):
            kw.pop("steer", None)
            return super().match_blocks_passes(reference, image, passes, counts, method, with_nbhd, **kw)
        assert kw.pop("steer") == 1 and kw.pop("deform") is True
        validate = kw.pop("validate", None)
        assert not kw and passes.dtype == _lib.BLOCK_PASS_DTYPE
        self.calls.append(("steered", passes.copy(), list(counts), method, with_nbhd, validate))
        outs, nbs, flags, preds, prev = [], [], [], [], None
        for p, a in enumerate(passes):
            spec = ((int(a["bw"]), int(a["bh"])), (int(a["sx"]), int(a["sy"])))
            g = B.grid(image.shape, *spec)
            assert len(g) == counts[p]
            ny, nx = len(np.unique(g[:, 1])), len(np.unique(g[:, 0]))
            searched, c = image, np.zeros((len(g), 2), np.int64)
            if p:
                searched = D.deform_brute(image, field_brute_q8(image.shape, prev[0], prev[1]))
                c = field_at_brute_q8(image.shape, prev[0], prev[1], g)
            out, nb = self._run(reference, searched, _lib.block_records(g), np.zeros((len(g), 2), np.int64), int(a["margin"]),
                                method, True)
            pos_w = np.stack((out["x"], out["y"]), axis=1).astype(np.int64)
            out["x"] += ((c[:, 0] + 128) >> 8).astype(np.int32)
            out["y"] += ((c[:, 1] + 128) >> 8).astype(np.int32)
            pos = np.stack((out["x"], out["y"]), axis=1).astype(np.int64)
            d8 = []
            for k in range(len(g)):
                o = (fit_axis(nb[k][1][0], nb[k][1][1], nb[k][1][2], method), fit_axis(nb[k][0][1], nb[k][1][1], nb[k][2][1], method))
                d8.append([q8_of(float(pos_w[k][i]) + o[i]) - 256 * int(g[k][i]) + int(c[k][i]) for i in (0, 1)])
            d8 = np.array(d8, dtype=np.int64).reshape(-1, 2)
            if validate is not None:
                valid, rep = V.validate_brute((ny, nx), pos - g[:, :2], *validate)
                valid = np.array(valid, dtype=bool)
                d8[~valid] = 256 * np.array(rep, dtype=np.int64).reshape(-1, 2)[~valid]
                flags.append(valid)
            prev = (spec, smooth_brute((ny, nx), d8))
            outs.append(out)
            nbs.append(nb)
            preds.append(c.astype(np.int32))
        res = (np.concatenate(outs), (np.concatenate(nbs) if with_nbhd else None))
        if validate is not None:
            res += (np.concatenate(flags),)
        return res + (np.concatenate(preds),)
