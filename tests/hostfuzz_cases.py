"""
Cases of the host-layer differential fuzz (tests/golden/hostfuzz.json.gz): every input array of a case is rebuilt from
its id, so the fixture holds only ids, digests and the reference's outcomes.

Pure numpy, ``np.random.RandomState`` only (its stream is frozen across numpy releases: the generator and the tests run
under different ones).  Imported by tests/golden/make_hostfuzz.py and by the replays; never imports the reference.

A case id is ``<stratum><index>`` with an optional ``.d<draw>`` suffix (the generator's redraw of a case whose scores lie
too close to the threshold).  ``build_case(case_id) -> (kind, call, inputs)``:

- kind   "find" | "match" | "map" | "seq"
- call   for find / match / map: ``{"fn", "args", "kwargs"}`` with live objects (``fn`` names the MTM function);
         for seq: ``{"steps": [{"fn", "args", "kwargs", "before"}]}`` - ``before`` (None or a callable) changes the
         case's arrays in place before its step runs; the steps run in order on the same objects
- inputs {name: ndarray} of every array the call reaches (digested before anything runs)
"""
import hashlib
import zlib

import numpy as np

STRATA = {"A": 132, "B": 126, "C": 84, "D": 32, "E": 10, "F": 66}
STRATUM_NAMES = {"A": "arguments", "B": "pixel policy", "C": "degenerate geometry", "D": "routes",
                 "E": "memo sequences", "F": "computeScoreMap"}
DTYPES = ("uint8", "uint16", "int16", "int32", "bool", "float16", "float32")


def case_ids():
    return ["%s%03d" % (s, i) for s, n in STRATA.items() for i in range(n)]


def digest(a):
    """sha256 of an input array: its bytes (logical order), dtype, shape and strides."""
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(a).tobytes())
    h.update(("|%s|%r|%r" % (a.dtype.str, tuple(a.shape), tuple(a.strides))).encode())
    return h.hexdigest()


def digests(inputs):
    return {k: digest(v) for k, v in sorted(inputs.items())}


def _rs(case_id):
    return np.random.RandomState(zlib.crc32(case_id.encode()) & 0x7FFFFFFF)


def _pixels(rs, shape, dtype):
    """Random pixels of `dtype` over its usual range, with some low-frequency structure so that planted copies stand out."""
    base = rs.rand(*shape)
    if len(shape) >= 2 and shape[0] > 3 and shape[1] > 3:
        k = np.ones(3) / 3
        smooth = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 0, base)
        base = 0.5 * base + 0.5 * np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 1, smooth)
    dtype = np.dtype(dtype)
    if dtype == np.bool_:
        return base > 0.5
    if dtype.kind == "f":
        return base.astype(dtype)
    lo, hi = {"uint8": (0, 255), "uint16": (0, 65535), "int16": (-3000, 3000), "int32": (-100000, 100000)}[dtype.name]
    return np.floor(lo + base * (hi - lo + 1)).clip(lo, hi).astype(dtype)


def _recast(a, dtype):
    """`a` in another pixel type, its values mapped range to range (no overflow, no wrap-around)."""
    dtype = np.dtype(dtype)
    if a.dtype == dtype:
        return a.copy()
    a64 = a.astype(np.float64)
    lo, hi = float(a64.min(initial=0)), float(a64.max(initial=1))
    u = (a64 - lo) / (hi - lo) if hi > lo else np.zeros_like(a64)
    if dtype == np.bool_:
        return u > 0.5
    if dtype.kind == "f":
        return u.astype(dtype)
    tlo, thi = {"uint8": (0, 255), "uint16": (0, 65535), "int16": (-3000, 3000), "int32": (-100000, 100000)}[dtype.name]
    return np.round(tlo + u * (thi - tlo)).astype(dtype)


def _scene(rs, H, W, dtype="uint8", C=1, sizes=((9, 11), (7, 6)), plant=2):
    """An image and templates cut out of it (each also planted `plant` more times, copy k with k + 1 pixels changed), so
    that every template has hits."""
    shape = (H, W) if C == 1 else (H, W, C)
    img = _pixels(rs, shape, dtype)
    templs = []
    placed = []                                     # (y, x, h, w): copies go where they overlap nothing placed before

    def free(y, x, h, w):
        return all(y + h <= py or py + ph <= y or x + w <= px or px + pw <= x for py, px, ph, pw in placed)

    for h, w in sizes:
        y, x = rs.randint(0, H - h + 1), rs.randint(0, W - w + 1)
        t = img[y:y + h, x:x + w].copy()
        placed.append((y, x, h, w))
        for k in range(plant):
            for _ in range(20):
                y2, x2 = rs.randint(0, H - h + 1), rs.randint(0, W - w + 1)
                if free(y2, x2, h, w):
                    break
            img[y2:y2 + h, x2:x2 + w] = t
            # copy k differs from the template in k + 1 pixels: distinct scores, so that the order of hits is decided
            flat = img[y2:y2 + h, x2:x2 + w].reshape(h * w, -1)
            flat[rs.randint(0, h * w, k + 1)] = _pixels(rs, (k + 1, flat.shape[1]), img.dtype)
            img[y2:y2 + h, x2:x2 + w] = flat.reshape(img[y2:y2 + h, x2:x2 + w].shape)
            placed.append((y2, x2, h, w))
        templs.append(t)
    return img, [np.ascontiguousarray(t) for t in templs]


def _thr(rs, method, t, dtype="uint8"):
    """A threshold for `method` of the order of the scores a template `t` produces."""
    if method in (3, 5):
        return float(np.round(rs.uniform(0.45, 0.9), 3))
    if method == 1:
        return float(np.round(rs.uniform(0.05, 0.3), 3))
    vmax = {"uint8": 255.0, "uint16": 65535.0, "int16": 3000.0, "int32": 1e5}.get(np.dtype(dtype).name, 1.0)
    scale = t.size * vmax * vmax
    if method == 0:
        return float(np.round(rs.uniform(0.02, 0.08) * scale, 1))
    if method == 2:
        return float(np.round(rs.uniform(0.3, 0.4) * scale, 1))
    return float(np.round(rs.uniform(0.02, 0.06) * scale, 1))          # method 4


def _named(inputs, lt):
    for i, tup in enumerate(lt):
        if isinstance(tup, (tuple, list)) and len(tup) >= 2:
            inputs["t%d" % i] = tup[1]
            if len(tup) >= 3 and isinstance(tup[2], np.ndarray):
                inputs["m%d" % i] = tup[2]
    return inputs


def _search(fn, lt, img, **kw):
    kind = "match" if fn == "matchTemplates" else "find"
    inputs = _named({"image": img}, lt if isinstance(lt, (list, tuple)) else [])
    return kind, {"fn": fn, "args": (lt, img), "kwargs": kw}, inputs


# ---- A: arguments ---------------------------------------------------------------------------------------------------
_NOBJ = [-3, -1, 0, 1, 2, 3, True, False, float("inf"), 2.0, np.int64(2), float("nan")]


def _case_A(i, rs):
    fn = "matchTemplates" if i % 2 == 0 else "findMatches"
    j = i // 2                                      # 66 variants x both functions (maxOverlap: matchTemplates)
    img, (t0, t1) = _scene(rs, rs.randint(40, 70), rs.randint(50, 90))
    lt = [("a", t0), ("b", t1)]
    kw = {"method": 5, "score_threshold": _thr(rs, 5, t0)}
    if j < 12:
        kw["N_object"] = _NOBJ[j]
        if j % 3 == 1:
            kw["method"], kw["score_threshold"] = 1, _thr(rs, 1, t0)
    elif j < 24:                                    # tuple shapes
        m = (rs.rand(*t0.shape) > 0.3).astype(np.uint8) * 255
        method = (3, 0, 5)[j % 3] if fn == "findMatches" else (3, 5, 1)[j % 3]
        kw["method"], kw["score_threshold"] = method, _thr(rs, method, t0)
        v = (j - 12) // 3 if j < 21 else 3 + (j - 21)
        if v == 0:
            lt = [("a", t0, m), ("b", t1)]
        elif v == 1:
            lt = [("a", t0, None), ("b", t1, None)]
        elif v == 2:
            lt = [("a", t0, m[:-1]), ("b", t1, m.astype(np.float32)[:t1.shape[0], :t1.shape[1]])]
        elif v == 3:
            lt = [("a", t0, m, "extra"), ("b", t1, None, None)]
        elif v == 4:
            lt = [["a", t0], ("b", t1)]
        else:
            lt = [("a", t0, m.astype(bool))]
    elif j < 30:                                    # containers and labels
        v = j - 24
        if v == 0:
            lt = (("a", t0), ("b", t1))
        elif v == 1:
            lt = []
        elif v == 2:
            lt = [(7, t0), (-1, t1)]
        elif v == 3:
            lt = [("a",), ("b", t1)]
        elif v == 4:
            lt = [(0, t0), ("0", t0.copy())]
        else:
            lt = ()
    elif j < 36:                                    # score_threshold types and range
        v = j - 30
        kw["score_threshold"] = [0.55, 1, np.float32(0.6), np.float64(0.65), -0.25, 1.5][v]
        if v == 1:
            kw["score_threshold"] = 0
    elif j < 42:                                    # maxOverlap: a matchTemplates argument only (12 values)
        fn = "matchTemplates"
        kw["maxOverlap"] = ([0, 0.25, 1, np.float32(0.3), -0.01, 1.01] if i % 2 == 0 else
                            [0.5, 0.75, np.float64(0.1), 0.99, 0.0, 1.0])[j - 36]
        kw["score_threshold"] = 0.3
        if i % 2 and j - 36 in (4, 5):
            kw["N_object"] = 3 if j - 36 == 4 else 2
            kw["method"], kw["score_threshold"] = 1, _thr(rs, 1, t0)
    elif j < 49:                                    # method 0-5 and a numpy integer
        kw["method"] = [0, 1, 2, 3, 4, 5, np.int64(3)][j - 42]
        kw["score_threshold"] = _thr(rs, int(kw["method"]), t0)
    elif j < 57:                                    # searchBox
        H, W = img.shape
        v = j - 49
        sb = [(5, 4, W - 10, H - 8), [3, 2, W - 20, H - 6], np.array([2, 6, W - 12, H - 10]), (-6, 3, 30, H - 3),
              (4, -5, W - 5, 30), (W - 25, H - 20, 60, 60), (10, 12, t0.shape[1], t0.shape[0]),
              (0, 0, t0.shape[1] - 1, t0.shape[0])][v]
        kw["searchBox"] = sb
        if v == 6:
            lt = [("a", t0)]
    else:                                           # empty and 64-bit inputs
        v = j - 57
        if v == 0:
            img = img[0:0]
        elif v == 1:
            img = img[:, 0:0]
        elif v == 2:
            lt = [("a", t0[0:0]), ("b", t1)]
        elif v == 3:
            lt = [("a", t0), ("b", t1[:, 0:0])]
        elif v == 4:
            img = img.astype(np.float64)
        elif v == 5:
            lt = [("a", t0.astype(np.float64))]
        elif v == 6:
            lt = [("a", t0.astype(np.float64))]
            img = img.astype(np.float64)
        elif v == 7:
            lt = [("a", np.ascontiguousarray(np.pad(t0, ((0, img.shape[0]), (0, 0)))))]
        else:
            kw["N_object"] = 2.5
    return _search(fn, lt, img, **kw)


# ---- B: pixel policy ------------------------------------------------------------------------------------------------
def _noncontig(a, v):
    if v == 0:
        return a[::-1]
    if v == 1:
        return a[:, ::-1]
    if v == 2:
        return np.asfortranarray(a)
    return a


def _case_B(i, rs):
    fn = "findMatches" if i % 3 else "matchTemplates"
    H, W = rs.randint(36, 64), rs.randint(40, 80)
    if i < 49:                                      # every image x template dtype pair
        idt, tdt = DTYPES[i // 7], DTYPES[i % 7]
        img, (t0,) = _scene(rs, H, W, idt, sizes=((8, 10),))
        t0 = _recast(t0, tdt)
        method = (5, 3, 1, 4, 2, 0)[i % 6] if fn == "findMatches" else (5, 3, 1)[i % 3]
        if "bool" in (idt, tdt):                    # 0/1 pixels: plateaus everywhere; integer sums keep them exact
            method = (2, 0)[i % 2] if fn == "findMatches" else 2
        lt = [("t", t0), ("u", t0[1:-1, 2:].copy())]
        return _search(fn, lt, img, method=method, score_threshold=_thr(rs, method, t0, tdt))
    if i < 77:                                      # masks of every dtype, all-zero and single-pixel masks
        k = i - 49
        idt = ("uint8", "float32", "uint16", "uint8")[k % 4]
        img, (t0,) = _scene(rs, H, W, idt, sizes=((9, 8),))
        mdt = DTYPES[k % 7]
        kind = k // 7                               # 0 random, 1 all-zero, 2 single pixel, 3 ones
        m = np.zeros(t0.shape, dtype=mdt)
        if kind == 0:
            m = _pixels(rs, t0.shape, mdt)
        elif kind == 2:
            m[rs.randint(t0.shape[0]), rs.randint(t0.shape[1])] = 1
        elif kind == 3:
            m = np.ones(t0.shape, dtype=mdt)
        if mdt == "uint8" and kind == 0:
            m = (m > 100).astype(np.uint8) * 255
        method = 3 if (k % 2 == 0 or kind == 2) else 0     # (one-pixel TM_SQDIFF: border values near 0 everywhere)
        fn = "findMatches" if (method == 0 or kind == 1) else fn
        lt = [("m", t0, m), ("p", t0)]
        thr = _thr(rs, method, t0, idt)
        if method == 0:                             # TM_SQDIFF weighs the squares by mask^2
            thr *= max(1.0, float(m.astype(np.float64).max())) ** 2
        return _search(fn, lt, img, method=method, score_threshold=thr)
    if i < 101:                                     # channels
        k = i - 77
        C = (1, 3, 4)[k % 3]
        idt = ("uint8", "float32")[(k // 3) % 2]
        img, (t0, t1) = _scene(rs, H, W, idt, C=C)
        method = (5, 3, 1, 2)[(k // 6) % 4]
        lt = [("a", t0), ("b", t1)]
        if k >= 12:                                 # channel mismatches: a gray template on colour and the reverse
            if C == 1:
                lt = [("a", np.stack([t0] * 3, axis=2))]
            elif k % 2:
                lt = [("a", np.ascontiguousarray(t0[..., 0]))]
            else:
                lt = [("a", np.ascontiguousarray(t0[..., :2]))] if C == 3 else [("a", t0[..., :3].copy())]
        return _search(fn, lt, img, method=method, score_threshold=_thr(rs, method, t0, idt))
    k = i - 101                                     # non-contiguous inputs
    idt = ("uint8", "float32", "uint16", "int16", "uint8")[k % 5]
    C = 3 if k % 4 == 3 else 1
    img, (t0, t1) = _scene(rs, H, W, idt, C=C)
    v = k % 5
    if v == 3:
        img, t0, t1 = img.transpose(1, 0, 2) if C == 3 else img.T, (t0.transpose(1, 0, 2) if C == 3 else t0.T), t1
    elif v == 4:
        img = np.repeat(img, 2, axis=1)[:, ::2]
        t0 = np.repeat(t0, 2, axis=0)[::2]
    else:
        img, t0 = _noncontig(img, v), _noncontig(t0, (v + 1) % 3)
    method = (5, 1, 3)[k % 3]
    lt = [("a", t0), ("b", t1)]
    return _search(fn, lt, img, method=method, score_threshold=_thr(rs, method, t0, idt))


# ---- C: degenerate geometry -----------------------------------------------------------------------------------------
def _case_C(i, rs):
    fn = "findMatches" if i % 2 else "matchTemplates"
    method = (5, 1, 3, 0, 2, 4)[(i // 2) % 6]
    if fn == "matchTemplates" and method == 0:
        method = 1
    H, W = rs.randint(20, 48), rs.randint(24, 60)
    img = _pixels(rs, (H, W), "uint8")
    v = i // 12
    if v == 0:                                      # 1x1 templates
        lt = [("p", img[3:4, 5:6].copy()), ("q", np.array([[200]], np.uint8))]
    elif v == 1:                                    # template == image: a 1x1 map
        lt = [("all", img.copy()), ("all2", (255 - img).copy())]
    elif v == 2:                                    # h == H: 1-D map along x, with constant stretches
        img[:, 10:22] = 90
        lt = [("tall", img[:, 12:17].copy()), ("tall2", img[:, 3:9].copy())]
    elif v == 3:                                    # w == W: 1-D map along y, with constant stretches
        img[8:20, :] = 150
        img[8:20:2, 3] = 151
        lt = [("wide", img[9:13, :].copy()), ("wide2", img[0:5, :].copy())]
    elif v == 4:                                    # constant templates (the templNorm < DBL_EPSILON shortcut)
        img[5:15, 5:25] = 77
        lt = [("c", np.full((6, 7), 77, np.uint8)), ("z", np.zeros((4, 4), np.uint8))]
    elif v == 5:                                    # exact copies in flat regions
        img[:, : W // 2] = 40
        t = img[2:8, W // 2 - 3:W // 2 + 4].copy()
        img[H - 7:H - 1, W - 8:W - 1] = t
        lt = [("edge", t), ("flat", img[0:5, 0:5].copy())]
    else:                                           # extrema on the map border, both border rules
        h, w = rs.randint(4, 9), rs.randint(4, 9)
        corners = [(0, 0), (0, W - w), (H - h, 0), (H - h, W - w), (0, rs.randint(1, W - w)), (rs.randint(1, H - h), W - w)]
        y, x = corners[i % 6]
        t = img[y:y + h, x:x + w].copy()
        lt = [("b", t), ("n", _pixels(rs, (h + 1, w), "uint8"))]
    t0 = lt[0][1]
    thr = _thr(rs, method, t0)
    if v in (1, 2, 3) and method in (3, 5):
        thr = float(np.round(rs.uniform(-0.2, 0.6), 3))
    return _search(fn, lt, img, method=method, score_threshold=thr)


# ---- D: routes ------------------------------------------------------------------------------------------------------
def _case_D(i, rs):
    if i < 10:                                      # float32 lists mixing masked and unmasked templates (method 3)
        img, (t0, t1) = _scene(rs, 60, 80, "float32", sizes=((10, 9), (8, 12)))
        m = (rs.rand(*t0.shape) > 0.25).astype(np.float32)
        lt = [("masked", t0, m), ("plain", t1)] if i % 2 else [("plain", t1), ("masked", t0, m), ("p2", t0)]
        nobj = (1, float("inf"), 2, float("inf"), 1)[i % 5]
        return _search("matchTemplates", lt, img, method=3, N_object=nobj, score_threshold=float(np.round(rs.uniform(0.8, 0.97), 3)),
                       maxOverlap=0.2)
    if i < 14:                                      # >= 4096 pre-NMS peaks: device NMS
        img = rs.randint(0, 256, (200, 300)).astype(np.uint8)
        lt = [("n%d" % k, img[k * 11:k * 11 + 6, k * 17:k * 17 + 7].copy()) for k in range(1 + i % 2)]
        fn = "matchTemplates" if i != 13 else "findMatches"
        method = 1 if i == 11 else 5
        return _search(fn, lt, img, method=method, score_threshold=(0.9 if method == 1 else -0.3), maxOverlap=0.3) \
            if fn == "matchTemplates" else _search(fn, lt, img, method=method, score_threshold=-0.3)
    if i < 31:                                      # uint8 lists: one size class, many sizes
        k = i - 14
        img, _ = _scene(rs, 120, 160, "uint8", C=(1, 3)[k % 2], sizes=())
        if k < 8:
            lt = [("s%d" % n, img[n * 9:n * 9 + 12, n * 13:n * 13 + 12].copy()) for n in range(6 + k)]
        else:
            lt = [("v%d" % n, img[n * 7:n * 7 + 5 + n, n * 5:n * 5 + 14 - n].copy()) for n in range(k)]
        method = (5, 3, 1)[k % 3]
        fn = "matchTemplates" if k % 4 else "findMatches"
        thr = float(np.round(rs.uniform(*{5: (0.8, 0.9), 3: (0.985, 0.995), 1: (0.01, 0.03)}[method]), 3))
        kw = {"maxOverlap": 0.25} if fn == "matchTemplates" else {}
        return _search(fn, lt, img, method=method, score_threshold=thr, **kw)
    img, (t0, t1) = _scene(rs, 1024, 1100, "uint8", sizes=((24, 20), (16, 30)), plant=6)       # >= 1 Mpx (banded uploads)
    return _search("matchTemplates", [("big0", t0), ("big1", t1)], img, method=5, score_threshold=0.6, maxOverlap=0.1)


# ---- E: memo sequences ----------------------------------------------------------------------------------------------
def _case_E(i, rs):
    img, (t0, t1) = _scene(rs, 64, 90, "uint8", sizes=((10, 12), (8, 9)))
    m = (rs.rand(*t0.shape) > 0.3).astype(np.uint8) * 255
    lt = [("a", t0, m), ("b", t1)] if i % 2 else [("a", t0), ("b", t1)]
    other = np.ascontiguousarray(img[::-1])
    inputs = _named({"image": img, "other": other}, lt)
    st = lambda fn, im, before=None, **kw: {"fn": fn, "args": (lt, im), "kwargs": kw, "before": before}  # noqa: E731
    v = i % 5
    if v == 0:                                      # the image shape changes
        steps = [st("matchTemplates", img, score_threshold=0.6), st("matchTemplates", img[5:50, 3:80], score_threshold=0.6),
                 st("findMatches", other, score_threshold=0.6)]
    elif v == 1:                                    # searchBox and method change
        steps = [st("findMatches", img, method=3, score_threshold=0.8), st("findMatches", img, method=5, score_threshold=0.6,
                                                                            searchBox=(4, 4, 60, 50)),
                 st("matchTemplates", img, method=3, score_threshold=0.85, searchBox=(0, 2, 80, 60)),
                 st("findMatches", img, method=0, score_threshold=_thr(rs, 0, t0))]
    elif v == 2:                                    # template pixels changed in place
        def poke():
            t0[2:5, 3:6] = 255 - t0[2:5, 3:6]
        steps = [st("matchTemplates", img, score_threshold=0.5), st("matchTemplates", img, before=poke, score_threshold=0.5),
                 st("findMatches", img, score_threshold=0.5)]
    elif v == 3:                                    # `arr.shape = ...`: same pixels, another geometry
        def reshape():
            t0.shape = (t0.shape[1], t0.shape[0])
            if len(lt[0]) > 2:
                m.shape = (m.shape[1], m.shape[0])
        steps = [st("findMatches", img, method=3, score_threshold=0.7), st("findMatches", img, before=reshape, method=3,
                                                                            score_threshold=0.5),
                 st("matchTemplates", img, method=3, score_threshold=0.5)]
    else:                                           # a mask changed in place, then an image of another dtype
        def unmask():
            m[:] = 255
        steps = [st("findMatches", img, method=3, score_threshold=0.75), st("findMatches", img, before=unmask, method=3,
                                                                             score_threshold=0.75),
                 st("matchTemplates", img.astype(np.float32), method=3, score_threshold=0.75)]
    return "seq", {"steps": steps}, inputs


# ---- F: computeScoreMap ---------------------------------------------------------------------------------------------
def _case_F(i, rs):
    method = i % 6
    idt = DTYPES[(i // 6) % 7] if i < 42 else ("uint8", "float32", "uint16")[i % 3]
    tdt = idt if i % 4 else ("uint8", "float32")[(i // 4) % 2]
    C = 3 if i in (17, 29, 47, 53) else 1
    img, (t0,) = _scene(rs, rs.randint(24, 48), rs.randint(30, 60), idt, C=C, sizes=((7, 9),))
    t0 = _recast(t0, tdt)
    mask = None
    if i >= 42:
        k = i - 42                                  # masks: every dtype, all-zero, single pixel, wrong shape (warning)
        mdt = DTYPES[k % 7]
        mask = _pixels(rs, t0.shape, mdt) if k % 3 == 0 else np.zeros(t0.shape, mdt)
        if k % 3 == 1:
            mask[3, 4] = 1
        if k % 8 == 5:
            mask = mask[:-1]
        if k % 5 == 4:
            mask = _recast(mask, t0.dtype)
    inputs = {"image": img, "template": t0}
    if mask is not None:
        inputs["mask"] = mask
    return "map", {"fn": "computeScoreMap", "args": (t0, img), "kwargs": {"method": method, "mask": mask}}, inputs


_BUILDERS = {"A": _case_A, "B": _case_B, "C": _case_C, "D": _case_D, "E": _case_E, "F": _case_F}


def build_case(case_id):
    base = case_id.split(".")[0]
    kind, call, inputs = _BUILDERS[base[0]](int(base[1:]), _rs(case_id))
    return kind, call, inputs


def _short(v):
    if isinstance(v, np.ndarray):
        return "%s%s" % (v.dtype.name, list(v.shape))
    if isinstance(v, (list, tuple)):
        inner = ", ".join(_short(x) for x in v)
        return "[%s]" % inner if isinstance(v, list) else "(%s%s)" % (inner, "," if len(v) == 1 else "")
    if isinstance(v, np.generic):
        return "np.%s(%r)" % (type(v).__name__, v.item())
    return repr(v)


def describe(call):
    """One line naming the call (arrays by dtype and shape)."""
    steps = call["steps"] if "steps" in call else [call]
    return " ; ".join("%sMTM.%s(%s%s)" % ("<in-place change> " if s.get("before") else "", s["fn"],
                                          ", ".join(_short(a) for a in s["args"]),
                                          "".join(", %s=%s" % (k, _short(v)) for k, v in s["kwargs"].items()))
                      for s in steps)
