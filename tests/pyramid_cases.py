"""The coarse-to-fine search (MTM.findMatchesPyramid / matchTemplatesPyramid) restated in numpy on the oracle's functions,
and the planted images its tests use.  tests/test_pyramid_cpu.py checks the restatement against the exhaustive oracle;
tests/test_gpu_pyramid.py checks the GPU's pyramid search against it and against the exhaustive engine."""
import numpy as np

import mtm_oracle as O


def windows(cands, factor, radius, oh, ow):
    """The full-resolution windows of coarse candidates [(cy, cx), ...]: inclusive (y0, y1, x0, x1), clipped to an oh x ow
    score map; empty windows are dropped."""
    out = []
    for cy, cx in cands:
        y0, y1 = max(0, cy * factor - radius), min(oh - 1, cy * factor + radius)
        x0, x1 = max(0, cx * factor - radius), min(ow - 1, cx * factor + radius)
        if y0 <= y1 and x0 <= x1:
            out.append((y0, y1, x0, x1))
    return out


def union_mask(wins, oh, ow):
    u = np.zeros((oh, ow), dtype=bool)
    for y0, y1, x0, x1 in wins:
        u[y0:y1 + 1, x0:x1 + 1] = True
    return u


def default_coarse_threshold(method, score_threshold):
    return score_threshold + 0.1 if method == 1 else score_threshold - 0.1


def find_matches_pyramid(listTemplates, image, factor, method=5, N_object=float("inf"), score_threshold=0.5,
                         searchBox=None, coarse_threshold=None, radius=None, max_candidates=256, border=None,
                         score_map=None):
    """MTM.findMatchesPyramid restated.  `score_map(template, image, method)` computes a score map (default: the oracle's
    compute_score_map; the GPU tests pass MTM.computeScoreMap, whose maps are the engine's own)."""
    score_map = score_map or O.compute_score_map
    if coarse_threshold is None:
        coarse_threshold = default_coarse_threshold(method, score_threshold)
    radius = factor if radius is None else radius
    if searchBox is not None:
        x_off, y_off, sw, sh = searchBox
        image = image[y_off:y_off + sh, x_off:x_off + sw]
    else:
        x_off = y_off = 0
    small = O.downscale_area(image, factor)
    hits = []
    for tup in listTemplates:
        label, templ = tup[:2]
        th, tw = templ.shape[:2]
        cmap = score_map(O.downscale_area(templ, factor), small, method)
        if method == 1:
            cands = O.find_local_min(cmap, coarse_threshold, border)
        else:
            cands = O.peak_local_max_2d(cmap, coarse_threshold, border)
        cands = cands[:max_candidates]             # descending quality, ties row-major
        fmap = score_map(templ, image, method)
        oh, ow = fmap.shape
        u = union_mask(windows(cands, factor, radius, oh, ow), oh, ow)
        q = -fmap if method == 1 else fmap          # quality: larger is better
        if not u.any():
            continue
        if N_object == 1:
            ys, xs = np.nonzero(u)                  # row-major
            i = int(np.argmax(q[ys, xs]))           # first best
            peaks = [(int(ys[i]), int(xs[i]))]
        else:
            # the exhaustive peak test on the whole map (neighbours outside the windows count), every position of it
            is_max = np.zeros((oh, ow), dtype=bool)
            for y, x in O.peak_local_max_2d(q, -np.inf, border):
                is_max[y, x] = True
            if is_max[u].all():                     # no position of the windows differs from its neighbourhood's max
                continue
            thr = np.float32(-score_threshold if method == 1 else score_threshold)
            sel = is_max & u & (q > thr)
            ys, xs = np.nonzero(sel)
            order = np.argsort(-q[ys, xs].astype(np.float64), kind="stable")
            peaks = [(int(ys[i]), int(xs[i])) for i in order]
        hits.extend((label, (x + x_off, y + y_off, tw, th), fmap[y, x]) for y, x in peaks)
    return hits


def match_templates_pyramid(listTemplates, image, factor, method=5, N_object=float("inf"), score_threshold=0.5,
                            maxOverlap=0.25, searchBox=None, coarse_threshold=None, radius=None, max_candidates=256,
                            border=None, score_map=None):
    hits = find_matches_pyramid(listTemplates, image, factor, method, N_object, score_threshold, searchBox,
                                coarse_threshold, radius, max_candidates, border, score_map)
    return O.NMS(hits, score_threshold, method == 1, N_object, maxOverlap)


# ---- planted images --------------------------------------------------------------------------------------------------
def blob_template(rng, side, chans=1):
    """A template with structure at several scales (survives an area downscale): a few Gaussian blobs and mild noise."""
    y, x = np.mgrid[0:side, 0:side].astype(np.float64)
    planes = []
    for _ in range(chans):
        t = np.full((side, side), 60.0)
        for _ in range(4):
            cy, cx = rng.uniform(0, side, size=2)
            s = rng.uniform(side / 8.0, side / 4.0)
            t += rng.uniform(-60, 150) * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s))
        t += rng.uniform(-6, 6, size=t.shape)
        planes.append(t)
    t = np.stack(planes, axis=-1) if chans > 1 else planes[0]
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


def planted(seed, hw=(160, 200), side=24, n_templ=3, copies=2, chans=1):
    """(image, listTemplates): a low-contrast noise background with `copies` exact copies of every template at
    non-overlapping places."""
    rng = np.random.RandomState(seed)
    H, W = hw
    shape = (H, W) if chans == 1 else (H, W, chans)
    img = rng.randint(100, 124, size=shape).astype(np.uint8)
    units = [("t%d" % i, blob_template(rng, side, chans)) for i in range(n_templ)]
    taken = []
    for label, t in units:
        for _ in range(copies):
            for _attempt in range(200):
                y, x = int(rng.randint(0, H - side + 1)), int(rng.randint(0, W - side + 1))
                if all(abs(y - y2) > side + 2 or abs(x - x2) > side + 2 for y2, x2 in taken):
                    break
            taken.append((y, x))
            img[y:y + side, x:x + side] = t
    return img, units


def random_with_flats(seed, hw=(72, 90), side=12, n_templ=3, chans=1):
    """Random images with flat regions and exact copies of the templates (one of them cut from a flat region)."""
    rng = np.random.RandomState(seed)
    H, W = hw
    shape = (H, W) if chans == 1 else (H, W, chans)
    img = rng.randint(0, 256, size=shape).astype(np.uint8)
    img[5:30, 40:75] = 77
    img[H - 20:, :25] = 200
    units = []
    for i in range(n_templ):
        y, x = int(rng.randint(0, H - side)), int(rng.randint(0, W - side))
        units.append(("r%d" % i, np.ascontiguousarray(img[y:y + side, x:x + side])))
    return img, units
