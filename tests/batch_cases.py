"""Image stacks for the batch tests (TemplateMatcher.match_batch / mtm_find_matches_batch): adversarial seams, and the
"naive" batch - stack the images, search the tall image, drop the hits in seam rows afterwards - that the seam-aware
route must NOT be.  tests/test_batch_cpu.py checks on the oracle that every adversarial stack breaks the naive batch;
tests/test_gpu_batch.py checks the GPU's batch against per-image matching on the same stacks."""
import numpy as np

import mtm_oracle as O

H = W = 48          # image size of the adversarial stacks
TH = TW = 12        # template size


def blob_template():
    """A smooth template: a one-row shift of it still correlates highly (so windows next to a copy score high too)."""
    y, x = np.mgrid[0:TH, 0:TW].astype(np.float64)
    t = 40 + 180 * np.exp(-((y - 5.0) ** 2 + (x - 6.5) ** 2) / 18.0) + 3 * x
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


def background(rng, n):
    return rng.randint(100, 116, size=(n, H, W)).astype(np.uint8)


def split_template_stack(seed=1):
    """Image 0 ends with the top half of the template, image 1 starts with its bottom half: the straddling window is a
    perfect copy and must not be found; the partial windows beside it are what each image holds."""
    rng = np.random.RandomState(seed)
    t = blob_template()
    ims = background(rng, 3)
    ims[0, H - TH // 2:, 10:10 + TW] = t[:TH // 2]
    ims[1, :TH - TH // 2, 10:10 + TW] = t[TH // 2:]
    return ims, t


def last_row_stack(seed=2):
    """True peaks on the last valid map row of image 0 and on the first map row of image 1, each beside straddling
    windows that score higher (an exact copy of the template across the seam)."""
    rng = np.random.RandomState(seed)
    t = blob_template()
    ims = background(rng, 3)
    # straddling window at stack row H - TH + 2: image 0 rows H-TH+2 .. H-1 = template rows 0 .. TH-3, image 1 rows 0, 1
    ims[0, H - TH + 2:, 20:20 + TW] = t[:TH - 2]
    ims[1, :2, 20:20 + TW] = t[TH - 2:]
    # and one the other way round lower in the stack, for the first map row of image 2
    ims[1, H - 2:, 5:5 + TW] = t[:2]
    ims[2, :TH - 2, 5:5 + TW] = t[2:]
    return ims, t


def seam_minima_stack(seed=3):
    """Method 1 (TM_SQDIFF_NORMED, local minima): dark bands across the seams make low-difference windows straddle them,
    next to border windows of each image."""
    rng = np.random.RandomState(seed)
    t = blob_template()
    ims = background(rng, 4)
    for b in range(3):
        ims[b, H - 5:, 14:14 + TW] = t[:5]
        ims[b + 1, :TH - 5, 14:14 + TW] = t[5:]
    ims[3, H - TH:, 30:30 + TW] = t          # an exact copy on the last valid row of the last image
    return ims, t


def global_straddle_stack(seed=4):
    """N_object == 1: the best window of the tall map straddles a seam; every image has its own, weaker best."""
    rng = np.random.RandomState(seed)
    t = blob_template()
    ims = background(rng, 3)
    ims[0, H - 7:, 8:8 + TW] = t[:7]
    ims[1, :TH - 7, 8:8 + TW] = t[7:]
    noisy = np.clip(t.astype(np.int32) + rng.randint(-25, 26, size=t.shape), 0, 255).astype(np.uint8)
    for b in range(3):
        ims[b, 15:15 + TH, 3 + 9 * b:3 + 9 * b + TW] = noisy
    return ims, t


# (name, builder, method, N_object, threshold): the stacks the GPU tests run and the naive batch gets wrong
ADVERSARIAL = [
    ("split_template", split_template_stack, 5, float("inf"), 0.1),
    ("last_row", last_row_stack, 5, float("inf"), 0.5),
    ("seam_minima", seam_minima_stack, 1, float("inf"), 0.2),
    ("global_straddle", global_straddle_stack, 5, 1, 0.5),
]


def per_image_raw(images, template, method, n_object, thr, border):
    """Per-image truth on the oracle: [(y, x, score), ...] per image, the peaks (or the extremum) of the template."""
    out = []
    for im in images:
        cmap = O.match_template(im, template, method)
        out.append(_peaks(cmap, method, n_object, thr, border))
    return out


def naive_batch_raw(images, template, method, n_object, thr, border):
    """Stack, search the tall image as ONE image, then drop hits in seam rows and split by image."""
    n, h = len(images), template.shape[0]
    rows = images.shape[1]
    cmap = O.match_template(np.concatenate(list(images), axis=0), template, method)
    out = [[] for _ in range(n)]
    for y, x, s in _peaks(cmap, method, n_object, thr, border):
        b, yl = divmod(y, rows)
        if yl <= rows - h:
            out[b].append((yl, x, s))
    return out


def _peaks(cmap, method, n_object, thr, border):
    if n_object == 1:
        mn, mx, lmin, lmax = O.min_max_loc(cmap)
        x, y = lmin if method in (0, 1) else lmax
        return [(int(y), int(x), float(cmap[y, x]))]
    find = O.find_local_min if method in (0, 1) else O.find_local_max
    return sorted((int(p[0]), int(p[1]), float(cmap[tuple(p)])) for p in find(cmap, thr, border=border))
