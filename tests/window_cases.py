"""
The cells of tests/test_gpu_window_sweep.py: the exact-integer window kernels (csrc/mtm_k_window.hip.h, csrc/mtm_k_nbhd.hip.h,
the float kinds of sub_nbhd_kernel in csrc/mtm_subpixel.hip) at their chunk and tile edges.  This file holds the table, the
scene builder and the expectations; it imports nothing of the library and runs without a GPU (tests/test_window_cases_cpu.py
shows that the table is honest).

Standard of truth: mtm_oracle.match_template(image, templ, method, mask=..., corr="direct") - plain sliding sums - and, for
records, the oracle's own min_max_loc and find_local_max / find_local_min on that map.  Pixels are uint8, uint16 (through
float32, as the reference package casts them) or float32 integers 0 .. 4095, masks are binary: every partial sum is an integer
below 2^53, and the kernels claim the exhaustive map's value bit for bit.  Every comparison is equality of float32 bits, NaN
meeting NaN.

Families
  P  whole maps of win_score_tile through blocks_plane_kernel: matchBlocksStack([ref, img], blocks, margin, method,
     ensemble=True) returns every block's score at every displacement; with one pair the mean is the score itself.
  B  records of boxes_score_kernel: findMatchesInBoxes on host-packed templates, N_object = 1 (planted winners that visit
     every lane of a tile) and N_object = inf (every peak of the map).
  T  records of track_score_kernel, of the fused set sums (win_tile_sums_u8_set / _u16_set) and of re-acquisition.
  N  whole maps of the neighbourhood kernel: hitNeighbourhoods with a hit at every output.
  Y  pyr_window_kernel (phase 1 calls win_tile_sums_u8 itself): every hit of findMatchesPyramid carries the direct map's bits.

Scenes: noise with a tenth of the pixels zero (float kinds: none, they carry no flat windows) and the template kinds of
test_gpu_tilings.py - `noise`, `exact`, `noisy` (a tenth of the pixels moved by 1 to 3: the score is neither clamped nor
tied), `const`, `zero`, `sat` - plus `isat` / `iconst` (a noise template over a saturated / constant image patch: flat windows,
the epilogue's 0 / NaN rules) and `flush` (a saturated template on a saturated box: sums across more than one uint32 flush).
The border rows and columns of the noise, exact and noisy templates and of every mask are non-zero: a dropped last tap
would otherwise multiply a zero.
"""
import zlib

import numpy as np

import mtm_oracle as O

# mirrored from csrc/mtm_k_window.hip.h, csrc/mtm_k_nbhd.hip.h and csrc/mtm_internal.h (test_window_cases_cpu.py parses them)
WIN_TILE = 16
WIN_KR, WIN_KC = 16, 64
WIN_IW = WIN_TILE + WIN_KC + 4
SUB_R, SUB_C = 16, 64
TRACK_NV = 4
U16_MAX_PIXELS = 1 << 21

ALL = (0, 1, 2, 3, 4, 5)
PLANTED = (0, 1, 3, 5)              # the methods under which a noisy copy is its map's extremum
DENSITY = 0.9
TOP = {"u8": 255, "rgb": 255, "u16": 65535, "f32": 4095, "f32rgb": 4095}
CHANS = {"u8": 1, "rgb": 3, "u16": 1, "f32": 1, "f32rgb": 3}
NPDT = {"u8": np.uint8, "rgb": np.uint8, "u16": np.uint16, "f32": np.float32, "f32rgb": np.float32}
INT_DTYPES = ("u8", "rgb", "u16")

P_WIDTHS = (1, 2, 3, 4, 5, 7, 8, 60, 61, 62, 63, 64, 65, 66, 67, 68, 127, 128, 129)
P_HEIGHTS = (1, 2, 15, 16, 17, 31, 32, 33, 49)
P_MARGINS = (0, 1, 7, 8, 16, 24)
T_WIDTHS = (3, 61, 62, 63, 64, 65, 66, 67, 68)
T_HEIGHTS = (15, 16, 17, 33)
T_SETS = (1, 2, 3, 4, 5, 8, 9)
N_WIDTHS = (1, 2, 3, 4, 5, 61, 62, 63, 64, 65, 66, 67, 68, 129)
N_HEIGHTS = (1, 15, 16, 17, 33)


def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def _shape(h, w, dtype):
    return (h, w, 3) if CHANS[dtype] == 3 else (h, w)


def _noise(rng, shape, top, density=DENSITY):
    return rng.integers(top // 4, top + 1, shape) * (rng.random(shape) < density)


def _fix_border(a, top):
    """The zero pixels of the first and last row and column become top / 2 (in place)."""
    for edge in (a[0], a[-1], a[:, 0], a[:, -1]):
        edge[edge == 0] = top // 2


def _noisy(rng, patch, top, share=0.1, lo=1, hi=3):
    """`patch` with `share` of its pixels (one at least) moved by lo .. hi 255ths of `top`, up or down, inside 0 .. top."""
    sel = rng.random(patch.shape) < share
    sel.flat[int(rng.integers(0, patch.size))] = True
    step = rng.integers(lo, hi + 1, patch.shape) * rng.choice((-1, 1), patch.shape) * (top // 255)
    moved = patch + step
    moved = np.where((moved < 0) | (moved > top), patch - step, moved)       # (a move that would clip goes the other way)
    return np.where(sel, moved, patch)


def _template(kind, rng, patch, top):
    h, w = patch.shape[:2]
    if kind == "exact":
        return patch.copy()
    if kind == "noisy":
        return _noisy(rng, patch, top)
    if kind in ("noise", "isat", "iconst"):
        t = _noise(rng, patch.shape, top)
        _fix_border(t, top)
        return t
    t = np.empty_like(patch)
    if kind == "const":
        t[:] = 77 * (top // 255)
    elif kind == "zero":
        t[:] = 0
        t[h // 2, w // 2] = top
    elif kind in ("sat", "flush"):
        t[:] = top
        t[h // 2, w // 2] = 0
        if kind == "flush":                 # a few pixels more: both bytes of a uint16 pixel, the first and the last tap
            t[0, 0], t[-1, -1], t[h // 3, (2 * w) // 3] = top - 1, top // 2 + 1, 1
    else:
        raise ValueError(kind)
    return t


def direct_maps(image, templ, methods, mask=None):
    """{method: mtm_oracle.match_template(image, templ, method, mask, corr="direct")} as read-only float32 maps; the sliding
    sums of the template (one pass per channel; masked: two) are formed once and serve every method's epilogue.  uint16 goes
    through float32, as the reference package casts it."""
    if image.dtype == np.uint16:
        image, templ = image.astype(np.float32), templ.astype(np.float32)
    real, memo = O.sliding_corr, {}

    def once(img2d, ker2d, exact_int=False, force=None, cache=None, cache_key=None):
        assert cache_key is not None            # (one memo slot per operand pair of this template)
        if cache_key not in memo:
            memo[cache_key] = real(img2d, ker2d, exact_int=exact_int, force=force)
        return memo[cache_key]
    O.sliding_corr = once
    try:
        out = {}
        for m in methods:
            ref = np.ascontiguousarray(O.match_template(image, templ, m, mask=mask, corr="direct"), dtype=np.float32)
            ref.setflags(write=False)
            out[m] = ref
        return out
    finally:
        O.sliding_corr = real


def same_bits(got, ref):
    """Per element: the same float32, NaN with NaN."""
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    return (got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))


def bits(v):
    return int(np.float32(v).view(np.uint32))


def extremum(cmap, method):
    """(y, x, score) of the map's minimum (methods 0 and 1) or maximum, the first in row-major order (cv2.minMaxLoc)."""
    _, _, lo, hi = O.min_max_loc(cmap)
    x, y = lo if method in (0, 1) else hi
    return int(y), int(x), cmap[y, x]


def search_box(block, margin, shape):
    """The block's box widened by `margin` on every side and clipped to the image: (x0, y0, bw, bh)."""
    x, y, w, h = block
    x0, y0 = max(0, x - margin), max(0, y - margin)
    return x0, y0, min(shape[1], x + w + margin) - x0, min(shape[0], y + h + margin) - y0


CELLS = []
_DATA = {}


def _add(family, name, **kw):
    CELLS.append(dict(kw, family=family, name="%s-%s" % (family, name), rot=len(CELLS)))


# ---- family P ------------------------------------------------------------------------------------------------------------
_P_KINDS = ("noisy", "exact", "noise", "const", "zero", "sat", "isat", "iconst")
_P_SPARSE = (16, 7, 24, 8)


def _p_cell(group, dtype, h, w, margin, frame=None, places=None, kinds=None, methods=ALL):
    """places None: three blocks side by side, their boxes unclipped.  Otherwise the names of the nine places of a frame."""
    _add("P", "%s-%s-%dx%d-m%d%s" % (group, dtype, h, w, margin, "-f%dx%d" % frame if frame else ""), group=group, dtype=dtype,
         h=h, w=w, margin=margin, frame=frame, places=places, kinds=kinds, methods=tuple(methods))


for _d, _dt in enumerate(INT_DTYPES):
    for _i, _w in enumerate(P_WIDTHS):          # uint8 meets margin 16 at every width; the others cross sparsely
        _p_cell("w", _dt, 3, _w, 16 if _d == 0 else _P_SPARSE[(_i + _d) % 4])
    for _i, _h in enumerate(P_HEIGHTS):
        _p_cell("h", _dt, _h, 5, _P_SPARSE[(_i + _d) % 4])
        _p_cell("h", _dt, _h, 65, _P_SPARSE[(_i + _d + 1) % 4])
    for _m in (16, 24):
        _p_cell("hw", _dt, 17, 65, _m)
        _p_cell("hw", _dt, 33, 129, _m)
    for _m in P_MARGINS:
        _p_cell("m", _dt, 3, 5, _m)
        _p_cell("m", _dt, 16, 67, _m)
    # the nine places of a frame, whose width is 0 .. 3 mod 4: the box is clipped differently on each side
    for _i, _fw in enumerate((200, 201, 202, 203)):
        _p_cell("place", _dt, (17, 3, 16, 5)[_i], (65, 5, 62, 67)[_i], (7, 16, 8, 16)[(_i + _d) % 4], frame=(131, _fw),
                places=("tl", "tc", "tr", "ml", "in", "mr", "bl", "bc", "br"))
# saturated across the uint32 flushes: RGB 300 x 280 (a channel's total passes 2^32)
_p_cell("flush", "rgb", 300, 280, 8, kinds=("flush",))
P_FLUSH_U16 = dict(h=1448, w=1448, margin=1)       # (1448^2 pixels: just under the 2^21 the host admits)
_p_cell("flush", "u16", P_FLUSH_U16["h"], P_FLUSH_U16["w"], P_FLUSH_U16["margin"], frame=(1450, 1450), places=("in",),
        kinds=("flush",))


def _p_blocks(cell):
    """[(x, y, kind)] and the frame's shape."""
    h, w, m = cell["h"], cell["w"], cell["margin"]
    if cell["places"] is None:
        kinds = cell["kinds"] or tuple(_P_KINDS[(cell["rot"] * 3 + i) % len(_P_KINDS)] for i in range(3))
        if (2 * m + 1) ** 2 < 16:           # (an exact copy on a map of one output scores 1 and nothing else)
            kinds = tuple("noisy" if k == "exact" else k for k in kinds)
        n = len(kinds)
        H, W = h + 2 * m + 5, n * (w + 2 * m) + 7
        return [(m + 2 + i * (w + 2 * m), m + 3, k) for i, k in enumerate(kinds)], (H, W)
    H, W = cell["frame"]
    xs = {"l": 0, "c": ((W - w) // 2) | 1, "r": W - w, "n": ((W - w) // 3) | 1}
    ys = {"t": 0, "m": ((H - h) // 2) | 1, "b": H - h, "i": ((H - h) // 3) | 1}
    kinds = cell["kinds"] or tuple(_P_KINDS[(cell["rot"] + i) % len(_P_KINDS)] for i in range(len(cell["places"])))
    if len(kinds) < len(cell["places"]):
        kinds = tuple(kinds) * len(cell["places"])
    return [(xs[p[1]], ys[p[0]], k) for p, k in zip(cell["places"], kinds)], (H, W)


def _overlap(a, b):
    return a[0] < b[0] + b[2] and b[0] < a[0] + a[2] and a[1] < b[1] + b[3] and b[1] < a[1] + a[3]


def p_scene(cell):
    """-> image, [(reference frame, [block index])], [(x, y, w, h)], [template], kinds.  A reference frame holds the
    templates of its blocks at the blocks' places (blocks whose rectangles overlap go to different frames, that is calls)."""
    dtype, h, w, m = cell["dtype"], cell["h"], cell["w"], cell["margin"]
    top, rng = TOP[dtype], _rng(cell["name"])
    placed, (H, W) = _p_blocks(cell)
    img = _noise(rng, _shape(H, W, dtype), top)
    for x, y, kind in placed:
        if kind in ("isat", "iconst"):                  # (h + 2) x (w + 2) around the block: up to 3 x 3 flat windows
            img[max(0, y - 1):y + h + 1, max(0, x - 1):x + w + 1] = top if kind == "isat" else 77 * (top // 255)
        elif kind == "flush":                           # the whole search box
            x0, y0, bw, bh = search_box((x, y, w, h), m, (H, W))
            img[y0:y0 + bh, x0:x0 + bw] = top
    for x, y, kind in placed:
        if kind in ("exact", "noisy"):
            _fix_border(img[y:y + h, x:x + w], top)
    temps = [_template(kind, rng, img[y:y + h, x:x + w], top) for x, y, kind in placed]
    blocks = [(x, y, w, h) for x, y, _ in placed]
    groups = []
    for k, b in enumerate(blocks):
        for g in groups:
            if not any(_overlap(b, blocks[j]) for j in g):
                g.append(k)
                break
        else:
            groups.append([k])
    calls = []
    for g in groups:
        ref = _noise(rng, img.shape, top) if max(H, W) < 1000 else np.zeros_like(img)
        for k in g:
            x, y = blocks[k][:2]
            ref[y:y + h, x:x + w] = temps[k]
        calls.append((ref.astype(NPDT[dtype]), g))
    return img.astype(NPDT[dtype]), calls, blocks, [t.astype(NPDT[dtype]) for t in temps], [k for _, _, k in placed]


def p_expected(cell, img, blocks, temps):
    """{method: (n, 2m+1, 2m+1) planes}: the direct map of the host-cut block on the host-cut box, placed by the clip
    offsets, NaN elsewhere; and the maps themselves, [block][method]."""
    m = cell["margin"]
    side = 2 * m + 1
    planes = {mt: np.full((len(blocks), side, side), np.nan, np.float32) for mt in cell["methods"]}
    maps = []
    for k, (b, t) in enumerate(zip(blocks, temps)):
        x0, y0, bw, bh = search_box(b, m, img.shape)
        ref = direct_maps(np.ascontiguousarray(img[y0:y0 + bh, x0:x0 + bw]), t, cell["methods"])
        maps.append(ref)
        py, px = m - (b[1] - y0), m - (b[0] - x0)
        for mt in cell["methods"]:
            oh, ow = ref[mt].shape
            assert (oh, ow) == (bh - b[3] + 1, bw - b[2] + 1)
            planes[mt][k, py:py + oh, px:px + ow] = ref[mt]
    return planes, maps


# ---- family B ------------------------------------------------------------------------------------------------------------
B_MAP = (17, 33)
B_GEOMS = tuple((3, w) for w in P_WIDTHS) + tuple((h, w) for w in (5, 65) for h in P_HEIGHTS) + ((17, 65), (33, 129))
B_LOCAL_UNITS = len(B_GEOMS)            # the units of the N_object = inf cells: every geometry once


def _b_winners():
    """Planted outputs: every lane (ly, lx) in the first and in the second tile of a row of tiles, then the one-lane tiles."""
    out = [((i // 16) % 16, i % 16 + 16 * (i // 256)) for i in range(512)]
    out += [(16, x) for x in (0, 5, 15, 16, 31, 32)] + [(y, 32) for y in (0, 3, 4, 15)]
    return out


for _dt in INT_DTYPES:
    _add("B", "global-%s" % _dt, dtype=_dt, mode="global", methods=ALL)
    for _border in ("constant", "nearest"):
        _add("B", "local-%s-%s" % (_dt, _border), dtype=_dt, mode="local", border=_border, methods=ALL)


def b_scene(cell):
    """-> image, templates [(label, array)], regions [((x, y, w, h), [j])], winners [(y, x)] (outputs of each unit's map).
    The global and the local cells of a pixel type share one image; the local ones search its first units only."""
    dtype = cell["dtype"]
    key = ("B", dtype)
    if key not in _DATA:
        top, rng = TOP[dtype], _rng("B", dtype)
        winners = _b_winners()
        geoms = [B_GEOMS[(i * 5 + INT_DTYPES.index(dtype)) % len(B_GEOMS)] for i in range(len(winners))]
        boxes, x, y, shelf, width = [], 0, 0, 0, 1600
        for h, w in geoms:
            bh, bw = h + B_MAP[0] - 1, w + B_MAP[1] - 1
            if x + bw > width:
                x, y, shelf = 0, y + shelf, 0
            boxes.append((x, y, bw, bh))
            x, shelf = x + bw, max(shelf, bh)
        img = _noise(rng, _shape(y + shelf, width, dtype), top)
        wins = []
        for (bx, by, _, _), (h, w), (wy, wx) in zip(boxes, geoms, winners):
            wins.append(img[by + wy:by + wy + h, bx + wx:bx + wx + w])
            _fix_border(wins[-1], top)
        temps = [("t%d" % i, _noisy(rng, p, top).astype(NPDT[dtype])) for i, p in enumerate(wins)]
        regions = [(b, [i]) for i, b in enumerate(boxes)]
        _DATA[key] = (img.astype(NPDT[dtype]), temps, regions, winners)
    img, temps, regions, winners = _DATA[key]
    n = len(regions) if cell["mode"] == "global" else B_LOCAL_UNITS
    return img, temps[:n], regions[:n], winners[:n]


def b_maps(dtype):
    """[unit][method]: the direct map of every unit's crop, made once per pixel type."""
    key = ("Bmaps", dtype)
    if key not in _DATA:
        img, temps, regions, _ = b_scene(dict(dtype=dtype, mode="global"))
        _DATA[key] = [direct_maps(np.ascontiguousarray(img[y:y + bh, x:x + bw]), temps[j[0]][1], ALL)
                      for (x, y, bw, bh), j in regions]
    return _DATA[key]


def local_threshold(method):
    """Below every score (above, for the minima of methods 0 and 1): every peak of the map is a record."""
    return 1e30 if method in (0, 1) else -1e30


def b_expected(cell, method):
    """Per region the records [(label, (x, y, w, h), score bits)]: global - the extremum; local - the oracle's peak rule
    (find_local_max / find_local_min at local_threshold) as a sorted list."""
    img, temps, regions, _ = b_scene(cell)
    maps = b_maps(cell["dtype"])
    out = []
    for ((bx, by, _, _), (j,)), ref in zip(regions, maps):
        label, t = temps[j]
        cmap = ref[method]
        if cell["mode"] == "global":
            y, x, s = extremum(cmap, method)
            peaks = [(y, x)]
        elif method in (0, 1):
            peaks = O.find_local_min(cmap, local_threshold(method), cell["border"])
        else:
            peaks = O.find_local_max(cmap, local_threshold(method), cell["border"])
        out.append(sorted((label, (bx + int(x), by + int(y), t.shape[1], t.shape[0]), bits(cmap[y, x])) for y, x in peaks))
    return out


def records(hits):
    """A region's hits as b_expected states them."""
    return sorted((lab, tuple(int(v) for v in box), bits(s)) for lab, box, s in hits)


# ---- family T ------------------------------------------------------------------------------------------------------------
T_MAP = (17, 20)                         # a second tile of one row, of four columns
T_SHAPES = tuple((16, w) for w in T_WIDTHS) + tuple((h, w) for h in (15, 17, 33) for w in (3, 65))
T_COMBOS = tuple((n, v) for n in T_SETS for v in range(n))          # (set size, the variant that wins)
T_ROUNDS = 6
# two exact copies in one box (16 x 3 templates: the windows do not overlap): across the tile seam, across the wave boundary
# inside a tile (rows 3 and 4 of the 16 x 16 tile: lanes 48 .. 63 | 64 .. 79), the first in row-major order in the later lane
T_TIES = (((2, 17), (9, 3)), ((3, 10), (4, 2)))
T_REACQ_FRAMES = ((40, 50), (55, 71), (70, 88), (70, 89), (70, 90))
T_REACQ_WIDE = ((16, 61), (16, 64), (15, 65), (17, 65), (16, 68), (33, 65))

for _dt in INT_DTYPES:
    # plain: every track names one template by its index - a call without a set runs track_score_kernel and
    # track_reacquire_kernel (win_score_tile); a call with a set, of one template too, runs the fused set kernels
    _add("T", "plain-%s" % _dt, dtype=_dt, mode="sets", plain=True, methods=ALL)
    _add("T", "plain-reacquire-%s" % _dt, dtype=_dt, mode="reacquire", plain=True, frame=T_REACQ_FRAMES[-1 - INT_DTYPES.index(_dt)],
         methods=ALL)
    _add("T", "sets-%s" % _dt, dtype=_dt, mode="sets", methods=ALL)
    _add("T", "ties-%s" % _dt, dtype=_dt, mode="ties", methods=ALL)
    for _f in T_REACQ_FRAMES:
        _add("T", "reacquire-%s-%dx%d" % ((_dt,) + _f), dtype=_dt, mode="reacquire", frame=_f, methods=ALL)


def set_slots(n, v):
    """Variant v of a set of n: (the size nv of its group of TRACK_NV, its index in the group, the group's role)."""
    g = v // TRACK_NV
    nv = min(TRACK_NV, n - g * TRACK_NV)
    role = "single" if n <= TRACK_NV else "last" if (g + 1) * TRACK_NV >= n else "full"
    return nv, v % TRACK_NV, role


def _pack(sizes, width):
    """Shelf packing of (bw, bh) boxes: [(x, y, bw, bh)], the canvas height."""
    boxes, x, y, shelf = [], 0, 0, 0
    for bw, bh in sizes:
        if x + bw > width:
            x, y, shelf = 0, y + shelf, 0
        boxes.append((x, y, bw, bh))
        x, shelf = x + bw, max(shelf, bh)
    return boxes, y + shelf


def t_scene(cell):
    """-> frames, templates [(label, array)], tracks [((x, y, w, h), [j])], planted [(variant or None, [(y, x)])], min_score,
    reacquire."""
    dtype, mode, plain = cell["dtype"], cell["mode"], cell.get("plain", False)
    top, rng, npdt = TOP[dtype], _rng(cell["name"]), NPDT[dtype]
    temps, tracks, planted = [], [], []
    if mode == "sets":
        specs = []
        for i in range(T_ROUNDS * len(T_COMBOS)):
            n, v = (1, 0) if plain else T_COMBOS[i % len(T_COMBOS)]
            h, w = T_SHAPES[(i * 7 + INT_DTYPES.index(dtype)) % len(T_SHAPES)]
            specs.append((n, v, h, w, ((i * 5) % T_MAP[0], (i * 7) % T_MAP[1])))
        boxes, height = _pack([(w + T_MAP[1] - 1, h + T_MAP[0] - 1) for _, _, h, w, _ in specs], 1200)
        img = _noise(rng, _shape(height, 1200, dtype), top)
        for (n, v, h, w, (wy, wx)), (bx, by, _, _) in zip(specs, boxes):
            _fix_border(img[by + wy:by + wy + h, bx + wx:bx + wx + w], top)
        for (n, v, h, w, (wy, wx)), box in zip(specs, boxes):
            patch = img[box[1] + wy:box[1] + wy + h, box[0] + wx:box[0] + wx + w]
            js = []
            for k in range(n):       # the winner: a tenth of the pixels moved by 1 .. 3; the others: a third by 4 .. 12
                t = _noisy(rng, patch, top) if k == v else _noisy(rng, patch, top, 0.34, 4, 12)
                js.append(len(temps))
                temps.append(("t%d" % len(temps), t.astype(npdt)))
            tracks.append((box, js[0] if plain else js))
            planted.append((v, [(wy, wx)]))
        return [img.astype(npdt)], temps, tracks, planted, None, False
    if mode == "ties":
        h, w = 16, 3
        specs = [(n, dup, pair) for pair in T_TIES for n, dup in ((1, None), (2, None), (5, None), (3, (1, 2)), (9, (3, 4)))]
        boxes, height = _pack([(w + T_MAP[1] - 1, h + T_MAP[0] - 1)] * len(specs), 400)
        img = _noise(rng, _shape(height, 400, dtype), top)
        for (n, dup, pair), (bx, by, _, _) in zip(specs, boxes):
            patch = _noise(rng, _shape(h, w, dtype), top)
            _fix_border(patch, top)
            for y, x in pair:
                img[by + y:by + y + h, bx + x:bx + x + w] = patch
            js = []
            for k in range(n):
                # the exact copy is variant 0; or two identical exact copies at `dup`: the first in set order wins
                exact = k == 0 if dup is None else k in dup
                js.append(len(temps))
                temps.append(("t%d" % len(temps), (patch if exact else _noisy(rng, patch, top, 0.34, 4, 12)).astype(npdt)))
            tracks.append(((bx, by, w + T_MAP[1] - 1, h + T_MAP[0] - 1), js))
            planted.append((0 if dup is None else dup[0], sorted(pair)))
        return [img.astype(npdt)], temps, tracks, planted, None, False
    # reacquire: small frames, every track's box (the upper left corner) away from its object, min_score above every in-box
    # score.  The narrow objects stand side by side at the frame's lower right, one wide one (where the frame holds it) at
    # its lower left; from frame 0 to frame 1 every object moves by (1, 1).
    H, W = cell["frame"]
    fi, di = T_REACQ_FRAMES.index(cell["frame"]), INT_DTYPES.index(dtype)
    shapes = [(s, W - 5 - 4 * i) for i, s in enumerate(((16, 3), (15, 3), (17, 3), (33, 3))) if s[0] + 20 <= H]
    if W >= 88:
        shapes.append((T_REACQ_WIDE[(fi * 2 + di) % len(T_REACQ_WIDE)], 1))
    frames = [_noise(_rng(cell["name"], f), _shape(H, W, dtype), top) for f in range(2)]
    for i, ((h, w), ox) in enumerate(shapes):
        n = 1 if plain else (1, 3, 5, 2, 9, 4, 8)[(i + fi + di) % 7]
        v = (i * 3 + fi) % n
        oy = H - h - 2 - i % 2
        patch = _noise(rng, _shape(h, w, dtype), top)
        _fix_border(patch, top)
        for f, frame in enumerate(frames):
            frame[oy + f:oy + f + h, ox + f:ox + f + w] = patch
        js = []
        for k in range(n):
            t = _noisy(rng, patch, top) if k == v else _noisy(rng, patch, top, 0.34, 4, 12)
            js.append(len(temps))
            temps.append(("t%d" % len(temps), t.astype(npdt)))
        tracks.append(((0, 0, w + 9, h + 8), js[0] if plain else js))
        planted.append((v, [(oy, ox)]))
    return [f.astype(npdt) for f in frames], temps, tracks, planted, "never", True


def track_set(js):
    """A track's templates as a list (a plain track names one by its index)."""
    return [js] if isinstance(js, int) else list(js)


def never_passes(method):
    """A min_score no score passes (next_box: minima pass below it, maxima above it)."""
    return -1.0 if method in (0, 1) else 1e30


def t_expected(cell, method, margin=4):
    """[frame][track] -> (label, (x, y, w, h), score bits): the extremum of the box's map per variant, the best variant
    first in set order on ties; with re-acquisition (min_score never passes) the whole frame's."""
    frames, temps, tracks, _, min_score, reacquire = t_scene(cell)
    memo = _DATA.setdefault(("Tmaps", cell["name"]), {})
    boxes = [b for b, _ in tracks]
    out = []
    for f, frame in enumerate(frames):
        row = []
        for k, (_, js) in enumerate(tracks):
            x0, y0, bw, bh = (0, 0, frame.shape[1], frame.shape[0]) if reacquire else boxes[k]
            best = None
            for j in track_set(js):
                key = (f, j, x0, y0, bw, bh)
                if key not in memo:
                    memo[key] = direct_maps(np.ascontiguousarray(frame[y0:y0 + bh, x0:x0 + bw]), temps[j][1], ALL)
                y, x, s = extremum(memo[key][method], method)
                q = -float(s) if method in (0, 1) else float(s)
                if best is None or q > best[0]:
                    t = temps[j][1]
                    best = (q, (temps[j][0], (x0 + x, y0 + y, t.shape[1], t.shape[0]), bits(s)))
            row.append(best[1])
            if not reacquire:               # (no min_score: every hit moves its box)
                boxes[k] = search_box(best[1][1], margin, frame.shape)
        out.append(row)
    return out


# ---- family N ------------------------------------------------------------------------------------------------------------
N_MAP = (20, 23)
N_KINDS = ("u8", "rgb", "u8mask", "rgbmask", "u16", "f32", "f32rgb", "f32mask", "f32rgbmask")
_N_ROT = ("exact", "noise", "const", "zero", "sat")


def _n_cell(kind, h, w):
    masked = kind.endswith("mask")
    _add("N", "%s-%dx%d" % (kind, h, w), kind=kind, dtype=kind[:-4] if masked else kind, masked=masked, h=h, w=w,
         methods=(0, 3) if masked else ALL)


for _k, _kind in enumerate(N_KINDS):
    for _w in N_WIDTHS:
        _n_cell(_kind, 3, _w)
    for _i, _h in enumerate(N_HEIGHTS):
        _n_cell(_kind, _h, 65)
        if "rgb" not in _kind:
            _n_cell(_kind, _h, 5)


def n_scene(cell):
    """-> image, listTemplates [(label, template[, mask])], kinds.  The image's map is N_MAP; the hits are every output."""
    dtype, h, w = cell["dtype"], cell["h"], cell["w"]
    top, rng, npdt = TOP[dtype], _rng(cell["name"]), NPDT[dtype]
    flt = dtype.startswith("f32")
    H, W = h + N_MAP[0] - 1, w + N_MAP[1] - 1
    img = _noise(rng, _shape(H, W, dtype), top, 1.0 if flt else DENSITY)
    kinds = ["noisy", "exact" if flt else _N_ROT[cell["rot"] % len(_N_ROT)]]
    if not flt:                                         # flat windows: 2 x 2 of them saturated, 2 x 2 constant
        img[2:3 + h, 3:4 + w] = top
        img[10:11 + h, 15:16 + w] = 77 * (top // 255)
    places = [(int(rng.integers(5, 9)), int(rng.integers(6, 13))), (int(rng.integers(13, N_MAP[0])), int(rng.integers(0, 11)))]
    for y, x in places:
        _fix_border(img[y:y + h, x:x + w], top)
    temps = []
    for i, ((y, x), kind) in enumerate(zip(places, kinds)):
        t = _template(kind, rng, img[y:y + h, x:x + w], top).astype(npdt)
        if cell["masked"]:
            mk = (rng.random(t.shape) < 0.7)
            mk[0], mk[-1], mk[:, 0], mk[:, -1] = True, True, True, True
            temps.append(("t%d" % i, t, (mk * (1.0 if flt else 255)).astype(npdt)))
        else:
            temps.append(("t%d" % i, t))
    return img.astype(npdt), temps, kinds


def n_hits(cell, label):
    return [(label, (x, y, cell["w"], cell["h"]), 0.0) for y in range(N_MAP[0]) for x in range(N_MAP[1])]


def n_expected(cell, img, entry):
    """{method: (outputs, 3, 3)}: the direct map around every output, NaN outside the map."""
    ref = direct_maps(img, entry[1], cell["methods"], mask=entry[2] if len(entry) > 2 else None)
    out = {}
    for m, cmap in ref.items():
        assert cmap.shape == N_MAP
        pad = np.full((N_MAP[0] + 2, N_MAP[1] + 2), np.nan, np.float32)
        pad[1:-1, 1:-1] = cmap
        out[m] = np.stack([pad[y:y + 3, x:x + 3] for y in range(N_MAP[0]) for x in range(N_MAP[1])])
    return out, ref


# ---- family Y ------------------------------------------------------------------------------------------------------------
Y_SHAPES = ((17, 65), (5, 129))
for _h, _w in Y_SHAPES:
    _add("Y", "u8-%dx%d" % (_h, _w), dtype="u8", h=_h, w=_w, factor=2, radius=9, methods=(5, 3, 1))


def y_scene(cell):
    """-> image, listTemplates, places: noisy copies of three windows of a noise image (findMatchesPyramid, uint8).  The
    windows stand at multiples of the factor, so that the coarse level sees them as well."""
    h, w = cell["h"], cell["w"]
    rng = _rng(cell["name"])
    img = _noise(rng, (96 + h, 150 + w), 255)
    places = [(8, 12), (40, 92), (76, 34)]
    for y, x in places:
        _fix_border(img[y:y + h, x:x + w], 255)
    temps = [("t%d" % i, _noisy(rng, img[y:y + h, x:x + w], 255).astype(np.uint8)) for i, (y, x) in enumerate(places)]
    return img.astype(np.uint8), temps, places


def y_thresholds(method):
    """(score_threshold, coarse_threshold): every extremum of the scored windows is a hit; the coarse level proposes the
    planted windows at least."""
    return (2.0, 0.8) if method == 1 else (0.0, 0.3)


_NAMES = [c["name"] for c in CELLS]
assert len(set(_NAMES)) == len(_NAMES)


def family(f):
    return [c for c in CELLS if c["family"] == f]
