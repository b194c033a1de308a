"""
The cells of tests/test_gpu_masked_cores.py: masked uint8 classes on ncc_mfma_kernel - the table, the scenes and the exact
references.  No GPU and no library here; tests/test_masked_cores_cpu.py proves from this file alone what the GPU side relies on.

A masked uint8 class on the matrix cores is two launches.  The score launch forms c1 = sum I T M.  The sum I^2 M pass
(launch_masked_sumsq, csrc/mtm_launch.hip) is a launch of its own: row-multiplexed raw mode of ncc_mfma_kernel over the two
byte planes J_h, J_l of I^2 (square_planes_kernel, biased by -128) against the mask pack of pack_mask_rm (int8 0 / 1, not
biased), always R = 16 output rows per MFMA group and nt = 1 "template" - whatever tiling the class's score launch has.  Fused
(MfmaParams::sq_fused, the default), one launch accumulates A = 256 a_h + a_l, a_x = sum (J_x - 128) M, and its epilogue writes
c2 = A + 257 * 128 * n (n = the mask's set taps) into the sum2 plane, and the block minima the masked hits-only screen reads.
Unfused (MTM_MASKSQ_FUSED=0), two raw launches write a_h and a_l and masksq_combine_kernel combines them in float64.

READ-OUT.  TM_SQDIFF with a template that is zero everywhere: c1 = 0 and sum (T M)^2 = 0, so the score map is float32(c2).
With pixels 0 .. 15, c2 <= 225 * 66051 < 2^24: every output is an exact integer in float32, compared bit for bit with
sum I^2 (M > 0) in numpy int64 (c2_exact below: one shifted addition per set tap, nothing of the code under test).  Dark pixels
make the test sharp: J_h is 0 everywhere, its biased plane is constant at -128, and a tap dropped or counted twice moves c2 by
256 * 128 = 32768 - wherever the tap lies and whatever the pixel under it is.  The `sparse` scene (isolated pixels 1 .. 255, so
few that c2 stays below 2^24) exercises both byte planes.  The `sat` scene (all 255) is the positive end of the accumulator,
A = (126 * 256 - 127) n = 32129 n; its c2 = 65025 n is beyond 2^24 and is read THROUGH float32 rounding: the expected map is
float32(float64(c2)), one rounding of an exact integer, as the epilogue's cast.

THE RANGE.  A reaches down to -(256 + 1) 128 n = -32896 n over black pixels.  That fits an int32 up to n = 65280
(32896 * 65280 = 2 147 450 880; 32896 * 65281 = 2 147 483 776 > 2^31), while mfma_class_ok admits masked classes up to
w h = 66051 (the bound of the uint32 dot4 pass).  A window under a mask of n > 65280 set taps with c2 < 32896 n - 2^31 cannot
be held: at n = 65536 (256 x 256, full mask) that is c2 < 8 388 608, grey levels up to about 11; at n = 66048, mean I^2 < 382.
Before kMasksqFusedMaxOnes (csrc/mtm_ctx.h) the fused launch ran for every n; since, masks of more than 65280 set taps take the
unfused form.  The range family walks the bound: 65280 (255 x 256 full; 258 x 256 with 768 taps cleared), 65281, 65536, 66048,
and off the cores 66049 (257 x 257: wider than kMfmaMaxW) and 66304 (259 x 256), on `dark` and `black` scenes.

GEOMETRY of the R = 16, nt = 1 pass (all of it independent of the class's own tiling):
  * columns: 16-tap segments, 64-tap blocks (nb = ceil(w / 64) <= 4, kMfmaMaxW = 256): W_EDGES, both sides of each;
  * rows: a wave walks rm_steps = h + 2 R - 1 = h + 31 image rows (mfma_row_mux) in K chunks of Cfg::kChunk = kMfChunkH = 64
    rows (rm_tile_rows(h, 16) = min(h + 31, 64) + 96 tile rows): ceil((h + 31) / 64) chunks, so the chunk count steps up between
    h = 33 and 34, 97 and 98, 161 and 162, 225 and 226 (H_CHUNK_EDGES) - and h = 258 walks 289 rows in five chunks;
  * outputs: an MFMA group holds R = 16 rows, a wave two groups (32 rows), a work-group kMfRows = 4 waves: 8 R = 128 rows per
    row block (p.nyb); kMfSeg = 256 columns per segment, stored four at a time (the float4 / double2 tail).
Maps are 37 x 41 (both MFMA groups of wave 0 and the first rows of wave 1) where the output geometry is not the subject, and
9 x 41 for templates of more than 40000 taps, as in the tilings sweep (the costliest reference is 369 outputs x 66048 taps).

FULL SCORES.  A cross-section of the shapes with real templates (exact copies, noisy copies, `mzero`: zero under the mask, so
sum (T M)^2 = 0 and every normalised output is 0 / 0), 1, 3 and 20 templates (row-multiplexed and plain masked classes), all
four masked methods, against mtm_oracle.match_template(..., mask=..., corr="direct").

Everything is drawn from the cell's name with zlib.crc32.
"""
import zlib

import numpy as np

# mirrored from the sources (test_masked_cores_cpu.py parses them out of csrc/)
MASKED_MAX_AREA = 66051         # mfma_class_ok: w h 255^2 < 2^32
MFMA_MAX_W = 256                # kMfmaMaxW
MF_SEG = 256                    # kMfSeg: output columns per wave
MF_ROWS = 4                     # kMfRows: waves per work-group
MF_CHUNK_H = 64                 # kMfChunkH: image rows per K chunk
SQ_R = 16                       # R of the sum I^2 M pass (pack_mask_rm, mfma_row_mux(p, 16, 1))
ROW_BLOCK = 2 * MF_ROWS * SQ_R  # 128 output rows per work-group
FUSED_MAX_ONES = 65280          # kMasksqFusedMaxOnes
ACC_PER_BLACK_TAP = 257 * 128   # -A per set tap over a black pixel: 32896

KERNEL_F64, KERNEL_MFMA = 0, 3
METHODS = (0, 1, 2, 3)          # TM_SQDIFF, TM_SQDIFF_NORMED, TM_CCORR, TM_CCORR_NORMED: what a masked class takes

MASK_KINDS = ("ones", "disc", "ring", "corners", "first", "last", "lastrow", "lastcol", "col15", "col63", "checker", "rand", "none")
W_EDGES = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
H_EDGES = (1, 2, 15, 16, 17, 32, 33, 34, 64, 65)
H_CHUNK_EDGES = (33, 34, 97, 98, 161, 162, 225, 226)        # ceil((h + 31) / 64) = 1 | 2, 2 | 3, 3 | 4, 4 | 5
assert all(-(-(a + 2 * SQ_R - 1) // MF_CHUNK_H) + 1 == -(-(b + 2 * SQ_R - 1) // MF_CHUNK_H) and b == a + 1
           for a, b in zip(H_CHUNK_EDGES[::2], H_CHUNK_EDGES[1::2]))
OUT_OHS = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129)
OUT_OWS = (1, 2, 3, 4, 255, 256, 257, 259)
DEFAULT_MAP, LARGE_MAP = (37, 41), (9, 41)
# (h, w, mask kind, set taps) of the range family, the table of the module docstring
RANGE_ROWS = ((255, 256, "ones", 65280), (256, 256, "ones", 65536), (258, 256, "ones65280", 65280), (258, 256, "ones65281", 65281),
              (258, 256, "ones", 66048), (257, 257, "ones", 66049), (259, 256, "ones", 66304))


def on_cores(h, w):
    """mfma_class_ok for a masked single-channel uint8 class"""
    return w <= MFMA_MAX_W and h * w <= MASKED_MAX_AREA


# ---- the table -----------------------------------------------------------------------------------------------------------
CELLS = []


def _cell(family, h, w, mask, scene, out=None, n=1, methods=(0,), kinds=None):
    """family: mask | w | h | out | range (read-out cells: one all-zero template, TM_SQDIFF) or score | hits (full scores)."""
    out = tuple(out or (DEFAULT_MAP if h * w <= 40000 else LARGE_MAP))
    name = "%s-%dx%d-o%dx%d-%s-%s" % (family, h, w, out[0], out[1], mask, scene)
    readout = family not in ("score", "hits")
    if not readout:
        name += "-n%d" % n
    CELLS.append(dict(name=name, family=family, h=h, w=w, out=out, mask=mask, scene=scene, n=n, methods=tuple(methods),
                      kinds=kinds, readout=readout))


# every mask kind at two shapes: 9 x 130 (three blocks, the last of two taps; columns 15 .. 127 and 63, 127 exist) and
# 34 x 65 (two K chunks; a second block of ONE tap)
for _i, _k in enumerate(MASK_KINDS):
    _cell("mask", 9, 130, _k, ("dark", "sparse")[_i % 2])
    _cell("mask", 34, 65, _k, ("sparse", "dark")[_i % 2])
# template widths at one K chunk (h = 9) and at two (h = 34); heights at a partly filled block (w = 40) and, at the chunk
# edges, at three blocks as well (w = 129: the pack step is (sp * nb + b))
for _i, _w in enumerate(W_EDGES):
    _cell("w", 9, _w, "rand", "dark")
    _cell("w", 34, _w, ("lastcol", "rand", "ones")[_i % 3], ("sparse", "dark")[_i % 2])
for _i, _h in enumerate(sorted(set(H_EDGES + H_CHUNK_EDGES))):
    _cell("h", _h, 40, "rand", "dark")
    _cell("h", _h, 40, ("lastrow", "ones", "ring")[_i % 3], "sparse")
for _h in H_CHUNK_EDGES[:4]:
    _cell("h", _h, 129, "rand", "dark")
_cell("h", 258, 256, "rand", "dark")             # about 0.7 * 66048 set taps: the fused launch at the largest class
_cell("h", 258, 256, "disc", "sparse")
# output geometry at two small templates
for _i, _oh in enumerate(OUT_OHS):
    _cell("out", 9, 40, "rand", ("dark", "sparse")[_i % 2], out=(_oh, 37))
    _cell("out", 9, 65, "rand", ("sparse", "dark")[_i % 2], out=(_oh, 259))
for _i, _ow in enumerate(OUT_OWS):
    _cell("out", 9, 40, "rand", ("dark", "sparse")[_i % 2], out=(33, _ow))
    _cell("out", 9, 65, "rand", ("sparse", "dark")[_i % 2], out=(9, _ow))
_cell("out", 9, 40, "rand", "dark", out=(1, 1))
_cell("out", 9, 65, "ones", "black", out=(129, 257))
# the range family
for _h, _w, _k, _n in RANGE_ROWS:
    for _s in ("dark", "black"):
        _cell("range", _h, _w, _k, _s)
_cell("range", 258, 256, "ones", "sat")
RANGE = [c for c in CELLS if c["family"] == "range"]
# full scores: (h, w), n, mask, scene[, map]
for _shape, _n, _k, _s, _out in (((24, 40), 20, "rand", "noise", None), ((24, 40), 3, "last", "dark", None),
                                 ((24, 64), 20, "col63", "dark", None), ((9, 128), 3, "col63", "noise", None),
                                 ((34, 65), 3, "corners", "dark", None), ((34, 65), 1, "ones", "dark", None),
                                 ((65, 129), 1, "rand", "dark", None), ((17, 256), 3, "last", "dark", None),
                                 ((9, 40), 3, "rand", "dark", (129, 259)), ((9, 65), 1, "corners", "dark", (129, 41)),
                                 ((255, 256), 1, "ones", "dark", None), ((256, 256), 1, "ones", "dark", None),
                                 ((258, 256), 1, "rand", "noise", None), ((258, 256), 1, "ones", "dark", None)):
    _cell("score", _shape[0], _shape[1], _k, _s, out=_out, n=_n, methods=METHODS)
# ... and the scenes with blocks of c2 = 0, for the hits-only screen
for _shape, _n, _k in (((24, 40), 3, "rand"), ((9, 128), 3, "ones"), ((256, 256), 1, "ones"), ((258, 256), 1, "ones65281")):
    _cell("hits", _shape[0], _shape[1], _k, "black", n=_n, methods=(1, 3))

READOUT = [c for c in CELLS if c["readout"]]
SCORE = [c for c in CELLS if not c["readout"]]
NAMES = [c["name"] for c in CELLS]


# ---- masks, scenes, templates ----------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def mask_set(kind, h, w, rng):
    """The set taps of a mask kind, as a bool array."""
    yy, xx = np.mgrid[0:h, 0:w]
    s = np.zeros((h, w), bool)
    if kind == "ones":
        s[:] = True
    elif kind.startswith("ones"):                   # onesN: all but h w - N taps, the first and the last tap kept
        s[:] = True
        s.flat[rng.choice(np.arange(1, h * w - 1), size=h * w - int(kind[4:]), replace=False)] = False
    elif kind == "disc":                            # (the mask of test_gpu_tilings.py)
        s = (((yy - h / 2 + 0.5) / (h / 2)) ** 2 + ((xx - w / 2 + 0.5) / (w / 2)) ** 2) <= 1.0
    elif kind == "ring":
        s[0], s[-1], s[:, 0], s[:, -1] = True, True, True, True
    elif kind == "corners":
        s[0, 0] = s[0, -1] = s[-1, 0] = s[-1, -1] = True
    elif kind == "first":
        s[0, 0] = True
    elif kind == "last":
        s[-1, -1] = True
    elif kind == "lastrow":
        s[-1] = True
    elif kind == "lastcol":
        s[:, -1] = True
    elif kind in ("col15", "col63"):
        s = xx % (16 if kind == "col15" else 64) == (15 if kind == "col15" else 63)
    elif kind == "checker":
        s = (yy + xx) % 2 == 0
    elif kind == "rand":                            # (test_gpu_exact_kernels._mask: p = 0.7, the border taps count)
        s = rng.random((h, w)) < 0.7
        s[0], s[-1], s[:, 0], s[:, -1] = True, True, True, True
    else:
        assert kind == "none", kind
    return s


def make_mask(kind, h, w, rng):
    """uint8; a tap is set where the byte is non-zero: set bytes are a mix of 1, 128 and 255."""
    s = mask_set(kind, h, w, rng)
    vals = rng.choice(np.array([1, 128, 255], np.uint8), size=(h, w))
    return np.where(s, vals, 0).astype(np.uint8)


def zero_patch(oh, ow):
    """where the `black` scene's template-sized all-zero patch lies (an output position)"""
    return min(1, oh - 1), min(2, ow - 1)


def make_image(scene, h, w, oh, ow, n_set, rng):
    H, W = h + oh - 1, w + ow - 1
    if scene == "dark":
        img = rng.integers(0, 16, (H, W)) * (rng.random((H, W)) < 0.9)
    elif scene == "black":
        img = rng.integers(0, 4, (H, W))
        y, x = zero_patch(oh, ow)
        img[y:y + h, x:x + w] = 0
    elif scene == "sparse":                         # about 400 pixels of mean square 21760 under the mask at the most: ~ 2^23
        img = rng.integers(1, 256, (H, W)) * (rng.random((H, W)) < min(0.35, 400.0 / max(n_set, 1)))
    elif scene == "noise":                          # (the scene of test_gpu_tilings.py)
        img = rng.integers(0, 256, (H, W)) * (rng.random((H, W)) < 0.35)
    else:
        assert scene == "sat", scene
        img = np.full((H, W), 255)
    return np.ascontiguousarray(img.astype(np.uint8))


def kinds_of(cell):
    if cell["readout"]:
        return ["allzero"]
    if cell["kinds"]:
        return list(cell["kinds"])
    n = cell["n"]
    if n == 1:
        return ["noisy"]
    return ["exact", "noisy", "mzero"] + ["noisy" if i % 3 == 1 else "exact" for i in range(3, n)]


def scene(cell):
    """-> image, mask, [(template, mask)], kinds"""
    h, w, (oh, ow) = cell["h"], cell["w"], cell["out"]
    rng = _rng(cell["name"])
    mask = make_mask(cell["mask"], h, w, rng)
    n_set = int((mask > 0).sum())
    img = make_image(cell["scene"], h, w, oh, ow, n_set, rng)
    amp = {"noise": 30, "dark": 3, "black": 1}.get(cell["scene"], 0)
    kinds, units = kinds_of(cell), []
    for kind in kinds:
        if kind == "allzero":
            t = np.zeros((h, w), np.int64)
        else:
            y, x = int(rng.integers(0, oh)), int(rng.integers(0, ow))
            t = img[y:y + h, x:x + w].astype(np.int64)
            if kind == "noisy":
                t = t + rng.integers(-amp, amp + 1, t.shape)
            elif kind == "mzero":
                t = t + rng.integers(0, amp + 1, t.shape)
                t[mask > 0] = 0
            if kind != "mzero" and 0 < n_set <= 4:  # a template that is zero under a mask of a few taps would be one more `mzero`
                t[mask > 0] = np.maximum(t[mask > 0], 1)
        units.append((np.ascontiguousarray(np.clip(t, 0, 255).astype(np.uint8)), mask))
    return img, mask, units, kinds


# ---- the references --------------------------------------------------------------------------------------------------------
def c2_exact(img, mask):
    """sum I^2 (M > 0) over every window, int64: one shifted addition of the squared image per set tap."""
    h, w = mask.shape
    oh, ow = img.shape[0] - h + 1, img.shape[1] - w + 1
    sq = img.astype(np.int64) ** 2
    out = np.zeros((oh, ow), np.int64)
    for dy, dx in zip(*np.nonzero(mask)):
        out += sq[dy:dy + oh, dx:dx + ow]
    return out


def would_wrap(c2, n_set):
    """the outputs whose fused accumulator 256 a_h + a_l = c2 - 32896 n lies below -2^31"""
    return c2 < ACC_PER_BLACK_TAP * n_set - 2 ** 31


def reference_maps(cell, img, units):
    """{method: [mtm_oracle.match_template(image, template, method, mask=mask, corr="direct") per template]}.  The sliding
    sums serve every method's epilogue, and sum I^2 M every template's (a cell has one mask)."""
    import mtm_oracle as O
    real, memo, who = O.sliding_corr, {}, [0]

    def once(img2d, ker2d, exact_int=False, force=None, cache=None, cache_key=None):
        key = cache_key if cache_key[0] == "I2" else (who[0], cache_key)
        if key not in memo:
            memo[key] = real(img2d, ker2d, exact_int=exact_int, force=force)
        return memo[key]
    O.sliding_corr = once
    try:
        out = {m: [] for m in cell["methods"]}
        for i, (t, mask) in enumerate(units):
            who[0] = i
            for m in cell["methods"]:
                ref = np.ascontiguousarray(O.match_template(img, t, m, mask=mask, corr="direct"), dtype=np.float32)
                assert ref.shape == cell["out"]
                ref.setflags(write=False)
                out[m].append(ref)
        return out
    finally:
        O.sliding_corr = real


_DATA = {}


def cell_data(cell):
    """dict(img, mask, units, kinds, n_set, c2: int64 map, refs: {method: [float32 maps]}) of a cell, made once per session
    and left unchanged.  Read-out cells: refs[0][0] = float32(c2), from the integers alone."""
    d = _DATA.get(cell["name"])
    if d is None:
        img, mask, units, kinds = scene(cell)
        c2 = c2_exact(img, mask)
        if cell["readout"]:
            ref = c2.astype(np.float64).astype(np.float32)
            if cell["scene"] != "sat":
                assert np.array_equal(ref.astype(np.int64), c2), cell["name"]      # below 2^24: exact
            refs = {0: [ref]}
        else:
            refs = reference_maps(cell, img, units)
        for a in (img, mask, c2) + tuple(r for v in refs.values() for r in v):
            a.setflags(write=False)
        d = _DATA[cell["name"]] = dict(img=img, mask=mask, units=units, kinds=kinds, n_set=int((mask > 0).sum()), c2=c2, refs=refs)
    return d


def expected_route(cell, n_set):
    """(class kernel, timing()["sq_launches"], form of the pass).  sq_launches counts PASSES, not launches: launch_masked_sumsq
    brackets either form - the fused launch, or the two raw launches and masksq_combine_kernel - with one event pair and adds
    one; off the cores (the float64 kernel forms sum I^2 M itself) it stays 0.  Which form ran is therefore not visible in
    timing(): it is what the launcher's condition says (test_masked_cores_cpu.py holds the source to it), and above the bound
    only the unfused form can give the range cells' sums."""
    if not on_cores(cell["h"], cell["w"]):
        return KERNEL_F64, 0, "f64"
    return KERNEL_MFMA, 1, "fused" if n_set <= FUSED_MAX_ONES else "unfused"
