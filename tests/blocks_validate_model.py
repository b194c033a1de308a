"""Restatements for MTM.blocks.validate and MTM.matchBlocksMultipass(validate=) that share no code with them: the normalised
median test in Python integers and ``sorted``, the grids and fields its tests sweep, the scene with one flat coarse block,
the by-hand loop the validated call documents, and blocks_passes_model's oracle context extended with the validated passes
call."""
import numpy as np

import blocks_passes_model as M
from MTM import _lib
from MTM import blocks as B

GRIDS = ((1, 1), (1, 2), (1, 5), (2, 2), (2, 3), (3, 3), (3, 4), (5, 7))
PARAMS = ((2, 0.5), (1, 0), (0, 0), (3.5, 0.1))


def validate_brute(grid_shape, disp, threshold, epsilon):
    """(valid list of bool, replaced list of (dx, dy)) by the rule as the issue states it, block by block."""
    ny, nx = grid_shape
    d = [(int(a), int(b)) for a, b in np.asarray(disp).tolist()]
    valid, replaced = [], []
    for iy in range(ny):
        for ix in range(nx):
            nb = [d[jy * nx + jx] for jy in range(iy - 1, iy + 2) for jx in range(ix - 1, ix + 2)
                  if (jy, jx) != (iy, ix) and 0 <= jy < ny and 0 <= jx < nx]
            own = d[iy * nx + ix]
            out, med = False, []
            if len(nb) >= 3:
                n = len(nb)
                for c in (0, 1):
                    s = sorted(v[c] for v in nb)
                    m2 = s[(n - 1) // 2] + s[n // 2]
                    r = sorted(abs(2 * v[c] - m2) for v in nb)
                    rm4 = r[(n - 1) // 2] + r[n // 2]
                    # Python floats are float64: one rounded addition, one rounded multiplication
                    out = out or float(2 * abs(2 * own[c] - m2)) > float(threshold) * (float(rm4) + 4.0 * float(epsilon))
                    med.append((m2 + 1) // 2)           # (floor((m2 + 1) / 2): half goes towards +infinity)
            valid.append(not out)
            replaced.append(tuple(med) if out else own)
    return valid, replaced


def fields(grid_shape, seed, every=1):
    """The displacement fields of one grid: constant; constant with one outlier at every position (at every `every`-th
    one); random in [-3, 3] (many ties, even-count medians); random of magnitude up to 2^30."""
    ny, nx = grid_shape
    n = ny * nx
    rng = np.random.RandomState(seed)
    out = [np.tile(np.array([[4, -2]], dtype=np.int64), (n, 1))]
    for k in range(0, n, every):
        f = out[0].copy()
        f[k] = (4 + (7 if k % 2 else -2), -2 + (0 if k % 3 else 5))
        out.append(f)
    out += [rng.randint(-3, 4, size=(n, 2)).astype(np.int64) for _ in range(4)]
    out += [rng.randint(-2 ** 30, 2 ** 30 + 1, size=(n, 2)).astype(np.int64) for _ in range(2)]
    return out


def scene(kind="u8"):
    """The 166 x 230 pair with one flat coarse block: random pixels moved by (dx, dy) = (5, 3) with a little noise, then
    a flat 32 x 32 patch planted in the reference over block 5 of the 32 / 64 coarse grid."""
    rng = np.random.RandomState(5)
    top = 65536 if kind == "u16" else 256
    shape = (166, 230, 3) if kind == "rgb" else (166, 230)
    dt = np.uint16 if kind == "u16" else np.uint8
    ref = rng.randint(0, top, shape)
    img = np.clip(np.roll(ref, (3, 5), (0, 1)) + rng.randint(-3, 4, shape), 0, top - 1).astype(dt)
    ref = ref.astype(dt)
    ref[64:96, 64:96] = 77
    return ref, img


SCENE_PASSES = [(32, 64, 16), (16, 16, 2)]
SCENE_SHIFT = (5, 3)


def outside_patch(blocks):
    """The blocks that hold no pixel of the scene's flat patch."""
    x, y, w, h = (blocks[:, i] for i in range(4))
    return (x >= 96) | (x + w <= 64) | (y >= 96) | (y + h <= 64)


def by_hand(ref, img, passes, method, threshold, epsilon, refine=False, context=None):
    """The loop matchBlocksMultipass(validate=(threshold, epsilon)) documents, through matchBlocks(offsets=): one (blocks,
    positions, scores, valid) per pass; validate=None (threshold None): the unvalidated loop, 3-tuples."""
    out, steer = [], None
    for p, (block, step, margin) in enumerate(passes):
        b = B.grid(img.shape, block, step)
        off = None if p == 0 else B.predict_offsets(img.shape, passes[p - 1][:2], steer, passes[p][:2])
        pos, sc = B.matchBlocks(ref, img, b, margin, method, offsets=off, context=context)
        fine = B.matchBlocks(ref, img, b, margin, method, offsets=off, refine=True, context=context)[0] if refine else pos
        if threshold is None:
            steer = pos
            out.append((b, fine, sc))
        else:
            valid, rep = B.validate(B.grid_shape(img.shape, block, step), B.displacements(b, pos), threshold, epsilon)
            steer = b[:, :2] + rep
            out.append((b, fine, sc, valid))
    return out


class OracleCtx(M.OracleCtx):
    """blocks_passes_model.OracleCtx with the validated passes call composed as the native call documents it: every pass's
    records go through the median test (validate_brute), and the next pass is predicted from the replaced positions."""
    def match_blocks_passes(self, reference, image, passes, counts, method, with_nbhd=False, **kw):
        if "validate" not in kw:
            return super().match_blocks_passes(reference, image, passes, counts, method, with_nbhd)
        threshold, epsilon = kw.pop("validate")
        assert not kw and passes.dtype == _lib.BLOCK_PASS_DTYPE
        self.calls.append(("validated", passes.copy(), list(counts), method, with_nbhd, (threshold, epsilon)))
        outs, nbs, flags, prev = [], [], [], None
        for p, a in enumerate(passes):
            spec = ((int(a["bw"]), int(a["bh"])), (int(a["sx"]), int(a["sy"])))
            g = B.grid(image.shape, *spec)
            assert len(g) == counts[p]
            off = np.zeros((len(g), 2), np.int64)
            if p:
                cg = B.grid(image.shape, *prev[0])
                near = M.nearest_brute(image.shape, prev[0], spec)
                off = prev[1][near] - cg[near, :2]
            out, nb = self._run(reference, image, _lib.block_records(g), off, int(a["margin"]), method, with_nbhd)
            pos = np.stack((out["x"], out["y"]), axis=1).astype(np.int64)
            ny, nx = len(np.unique(g[:, 1])), len(np.unique(g[:, 0]))
            valid, rep = validate_brute((ny, nx), pos - g[:, :2], threshold, epsilon)
            prev = (spec, g[:, :2] + np.array(rep, dtype=np.int64).reshape(-1, 2))
            outs.append(out)
            nbs.append(nb)
            flags.append(np.array(valid, dtype=bool))
        return np.concatenate(outs), (np.concatenate(nbs) if with_nbhd else None), np.concatenate(flags)
