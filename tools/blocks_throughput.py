#!/usr/bin/env python3
"""Milliseconds per call, from numpy arrays to numpy arrays, of three ways to get the displacement of every block of a
grid between two images, one JSON line per workload:
  blocks        - matchBlocks(reference, image, grid, margin)
  blocks_refine - matchBlocks(..., refine=True): the same with sub-pixel positions
  loop          - what a user writes without the call: the blocks cut out of the reference on the host as templates, each
                  with its search box as a region, through one findMatchesInBoxes(..., N_object=1) - template cutting,
                  region building and the conversion of the hit lists to arrays included
The call's positions and float32 score bits are checked equal to the loop's (``equal_to_loop``), the refined positions
equal to refineHits' of the loop's hits (``refine_equal``, outside the timed part).

Data from synth.py: a photograph-like reference (smooth_u8; uint16 = 257 x that plus noise in the low byte) and, as the
image, the reference moved by a few pixels (wrapping around) with a little noise.  Each method is warmed up first; the
three calls are interleaved within a repetition; medians over the repetitions.

--stack F: the movie form instead - F frames of the same shapes and block grids (frame f = the reference moved by f times
the shift, with noise), milliseconds per PAIR of
  stack_previous / stack_first - matchBlocksStack(frames, grid, margin, reference=...)
  stack_ensemble               - matchBlocksStack(..., ensemble=True): the averaged planes and their peaks
  loop                         - matchBlocks over the F - 1 pairs ("previous"), what a user writes without the call
with ``equal_to_loop`` (both reference modes against their loops, positions and score bits) and, on a movie of at most 8
frames of noise around a weak pattern that moves by (2, 1) a frame (``noisy_movie``: a single pair's peak about 2.5 standard
deviations above the correlation noise of a block), the fraction of blocks found at that step by the pairs' own peaks
(``noisy_found_pairs``, mean over the pairs) and by the ensemble peak (``noisy_found_ensemble``).

--stack F --passes: coarse to fine over the movie - the two passes of --passes below, milliseconds per PAIR of
  stack_passes   - matchBlocksStackMultipass(frames, passes): one native call, every frame uploaded once
  loop_multipass - matchBlocksMultipass over the F - 1 pairs, what a user writes without the call
  stack_wide     - matchBlocksStack(frames, grid, margin): the single pass at the workload's (wide) margin
with ``equal_to_loop`` (stack_passes against loop_multipass, every pass and pair, positions and score bits).
--stack F --passes --ensemble: the passes on ensemble planes - milliseconds per PAIR of
  stack_passes_ensemble - matchBlocksStackMultipass(frames, passes, ensemble=True)
  by_hand               - the loop of matchBlocksStack(ensemble=True, offsets=) and predict_offsets the call documents
with ``equal_to_loop`` (every pass: positions, score bits and planes) and, on ``noisy_movie`` moved by more than the dense
margin a frame (at most 8 frames), the share of the dense grid's blocks clear of the border found at the step by the pairs'
own multipass (``noisy_found_pairs_multipass``, mean over the pairs), by the single-pass ensemble at the dense margin
(``noisy_found_ensemble_single``) and by the ensemble multipass (``noisy_found_ensemble_multipass``).
Both forms append their lines to profiles/blocks/stack_passes_throughput.jsonl (``--out`` names another file).

--passes: coarse to fine instead - milliseconds per call of
  single    - matchBlocks(reference, image, grid, margin): today's single pass at the workload's margin
  multipass - matchBlocksMultipass with a sparse wide pass (the workload's block at stride 2 x the block, the workload's
              margin) and a dense pass (the workload's grid, a quarter of the margin)
  by_hand   - the same two passes as the loop of matchBlocks(offsets=) and predict_offsets a user writes
with ``equal_to_loop`` (multipass against by_hand, every pass, positions and score bits) and, on a pair whose four quadrants
moved by four different known shifts within the workload's margin, with noise (``quadrant_pair``), the share of the blocks
that lie clear of the quadrants' seams found at their true displacement by the single pass and by the dense pass of
multipass (``found_single``, ``found_multipass``).  One further line (workload "K1 far") moves the whole image by more than
the dense margin: the dense grid alone at the dense margin against the two passes.

--passes --validate: the same two passes with the median test between them - milliseconds per call of
  validated   - matchBlocksMultipass(..., validate=True)
  unvalidated - matchBlocksMultipass(...) of the same build
  by_hand     - the loop of matchBlocks(offsets=), validate and predict_offsets the validated call documents
with ``equal_to_loop`` (validated against by_hand, every pass, positions, score bits and flags), the difference between
the validated and the unvalidated call (``validate_cost_ms``, medians of the same run) and, on the workload's pair with one
flat patch planted in the reference over a coarse block (``flat_block_pair``), the share of the dense blocks outside the
patch and clear of the border found at the true shift with and without validation (``found_validated``,
``found_unvalidated``).

--second [r] (alone or with --passes): the second correlation peak - milliseconds per call of
  plain  - matchBlocks(reference, image, grid, margin), or with --passes matchBlocksMultipass of the two passes above
  second - the same call with second=r (default 2), interleaved with it in one run
with their difference (``second_cost_ms``, medians of the same run), ``equal_to_model`` (every block's second position and
float32 score bits against the brute-force rule of tests/blocks_second_model.py over MTM.computeScoreMap of the block and its
box, NaN exactly where the model has no second peak), ``first_peaks_unchanged`` (positions and score bits of the call
without ``second``), the blocks without a second peak and the median peak ratio of every pass.

--passes --deform: the same two passes with window deformation between them - milliseconds per call of
  deformed   - matchBlocksMultipass(..., deform=True)
  undeformed - matchBlocksMultipass(...) of the same build
  by_hand    - the loop of matchBlocks, displacement_field, deform and field_at the deformed call documents
with ``equal_to_loop`` (deformed against by_hand, every pass: positions, score bits, predicted fields), their difference
(``deform_cost_ms``), the warp kernel alone (``warp_kernel_ms``: device events around deformImage's launch) against a
device-to-device copy of the image's bytes timed in the same run (``device_copy_ms``, ``warp_vs_copy``), and, on the
workload's reference under a known shear and a known rotation (``warped_pair``), the mean last-pass score and the RMS error
of the refined displacements against the known field over the blocks clear of the border, with and without ``deform``.

--passes --deform --steer refined: a third pass, the dense one repeated - milliseconds per call of
  undeformed - matchBlocksMultipass(...)
  deformed   - matchBlocksMultipass(..., deform=True): integer records steer
  steered    - matchBlocksMultipass(..., deform=True, steer="refined"): sub-pixel positions, filtered, steer
with ``equal_to_loop`` (steered against the loop it documents), ``steer_cost_ms`` (steered - deformed) and, on the sheared
and the rotated pair with 2 and 3 passes and (K1's row) on the tests' particle pair, ``rms_error_px`` of all three.

--mask: a static mask over the reference (the uint8 workloads K1 and K3, TM_CCORR_NORMED, pixels in 1..255 so that no
score is NaN) - milliseconds per call of
  masked   - matchBlocks(reference, image, grid, margin, 3, mask=mask)
  unmasked - matchBlocks(reference, image, grid, margin, 3) on the same pair
  loop     - what a user writes without the keyword: per block findMatches([(name, block, block's mask)], image, 3,
             N_object=1, searchBox=search_box(block, margin, shape))
  masked_at / unmasked_at - both calls with ``offsets=`` of zeros: the same results through the same native chain
             (mtm_match_blocks_at's: units on the device, the fixed tile table, a record kernel), which the masked call
             always takes a form of and the plain unmasked call does not
interleaved in one run, with ``equal_to_loop`` (positions and score bits of masked against loop) and the device time
between each call's events (``device_ms``: the call's table uploads and every launch of its chain - gather, score, and
for the pass chain the unit and record kernels; the images' and the mask's uploads lie ahead of the first event and are
not in it).  ``masked_vs_unmasked_device`` compares two different chains (the plain unmasked call decodes its keys on the
host); ``masked_at_vs_unmasked_at_device`` compares like with like.  The score launch alone is a kernel-trace row:
``--no-loop`` leaves the loop out so that a profiler run holds the calls' kernels only.  The mask keeps about 70 % of the
pixels: a few discs and a band cut out, generated and seeded (``static_mask``).  The lines also go to
profiles/blocks/mask_throughput.jsonl (``--out`` names another file).

Usage: tools/blocks_throughput.py [--reps 5] [--warmup 2] [--only K1|K2|K3] [--stack F [--passes [--ensemble]]]
       [--passes [--validate | --deform [--steer refined]]]
       [--second [r]] [--mask [--no-loop] [--out FILE]]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multitemplatematching-python_amd"))

# name, (rows, cols), channels, dtype, block side (= step), margin
WORKLOADS = [
    ("K1", (1080, 1920), 1, "uint8", 32, 8),
    ("K2", (2048, 2048), 1, "uint16", 48, 12),
    ("K3", (2160, 3840), 3, "uint8", 64, 16),
]


def workload(spec, seed=0, shift=(3, -2)):
    import synth
    name, hw, chans, dtype, side, margin = spec
    planes = [synth.smooth_u8(seed + c, hw) for c in range(chans)]
    ref = planes[0] if chans == 1 else np.ascontiguousarray(np.stack(planes, axis=2))
    rng = np.random.default_rng(seed + 10)
    top = 255
    if dtype == "uint16":
        ref = (ref.astype(np.uint16) * 257 + rng.integers(0, 64, size=ref.shape, dtype=np.uint16)).astype(np.uint16)
        top = 65535
    img = np.roll(ref, (shift[1], shift[0]), axis=(0, 1)).astype(np.int64) + rng.integers(-2, 3, size=ref.shape)
    return ref, np.clip(img, 0, top).astype(ref.dtype)


def run(MTM, spec, reps, warmup):
    from MTM import blocks as B
    name, hw, chans, dtype, side, margin = spec
    ref, img = workload(spec)
    grid = B.grid(ref.shape, side)
    method = MTM.TM_CCOEFF_NORMED

    def loop(keep=None):
        templs = [("b%d" % k, ref[y:y + h, x:x + w]) for k, (x, y, w, h) in enumerate(grid.tolist())]
        regions = [(B.search_box(b, margin, img.shape), [k]) for k, b in enumerate(grid.tolist())]
        res = MTM.findMatchesInBoxes(templs, img, regions, method, N_object=1)
        if keep is not None:
            keep.extend([templs, [r[0] for r in res]])
        pos = np.array([r[0][1][:2] for r in res], dtype=np.int64)
        return pos, np.array([r[0][2] for r in res], dtype=np.float32)

    methods = {
        "blocks": lambda: MTM.matchBlocks(ref, img, grid, margin, method),
        "blocks_refine": lambda: MTM.matchBlocks(ref, img, grid, margin, method, refine=True),
        "loop": loop,
    }
    results = {}
    for k, fn in methods.items():
        for _ in range(warmup):
            results[k] = fn()
    ms = {k: [] for k in methods}
    for _ in range(reps):
        for k, fn in methods.items():
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    (pos, sc), (lpos, lsc) = results["blocks"], results["loop"]
    equal = bool((pos == lpos).all() and sc.tobytes() == lsc.tobytes() and
                 results["blocks_refine"][1].tobytes() == lsc.tobytes())
    keep = []
    loop(keep)
    fine = np.array([h[1][:2] for h in MTM.refineHits(keep[0], img, keep[1], method)], dtype=np.float64)
    d = B.displacements(grid, pos)
    return {
        "workload": name, "image": "%dx%dx%d %s" % (hw[0], hw[1], chans, dtype), "blocks": int(len(grid)), "block": side,
        "margin": margin, "map": "%dx%d" % (2 * margin + 1, 2 * margin + 1),
        "ms": {k: round(v, 3) for k, v in med.items()},
        "ms_min": {k: round(min(v), 3) for k, v in ms.items()},
        "speedup_vs_loop": {k: round(med["loop"] / med[k], 2) for k in ("blocks", "blocks_refine")},
        "equal_to_loop": equal,
        "refine_equal": bool((results["blocks_refine"][0] == fine).all()),
        "found_shift": float(np.mean((d == (3, -2)).all(axis=1))),
        "reps": reps,
    }


def movie(spec, n, seed=0, shift=(3, -2)):
    ref, _ = workload(spec, seed, shift)
    rng = np.random.default_rng(seed + 20)
    top = 65535 if ref.dtype == np.uint16 else 255
    frames = [ref]
    for f in range(1, n):
        a = np.roll(ref, (f * shift[1], f * shift[0]), axis=(0, 1)).astype(np.int32)
        a += rng.integers(-2, 3, size=ref.shape, dtype=np.int32)
        frames.append(np.clip(a, 0, top).astype(ref.dtype))
    return frames


def noisy_movie(spec, n, seed=0, step=(2, 1), sigma=22.0, z=2.5):
    """n frames of noise (standard deviation `sigma` grey levels) around a weak random pattern that moves by `step` a
    frame.  The pattern's amplitude is set from the block size: two frames' matching blocks correlate with rho = the
    pattern's share of a frame's variance, the correlation of unrelated blocks of n_pix values scatters by about
    1 / sqrt(n_pix), and rho is chosen `z` such standard deviations high - a single pair's peak is marginal at any block
    size, the mean of P planes stands sqrt(P) times higher."""
    name, hw, chans, dtype, side, margin = spec
    ref, _ = workload(spec, seed)
    rng = np.random.default_rng(seed + 30)
    scale = 257.0 if ref.dtype == np.uint16 else 1.0
    base = rng.integers(0, 256, size=ref.shape).astype(np.float32) - 127.5
    rho = z / np.sqrt(side * side * chans)
    amp = np.sqrt(rho / (1.0 - rho)) * sigma / float(base.std())
    frames = []
    for f in range(n):
        a = 128 + amp * np.roll(base, (f * step[1], f * step[0]), axis=(0, 1))
        a += sigma * rng.standard_normal(size=ref.shape, dtype=np.float32)
        frames.append((np.clip(a, 0, 255) * scale).astype(ref.dtype))
    return frames


def run_stack(MTM, spec, n_frames, reps, warmup):
    from MTM import blocks as B
    name, hw, chans, dtype, side, margin = spec
    frames = movie(spec, n_frames)
    grid = B.grid(frames[0].shape, side)
    method = MTM.TM_CCOEFF_NORMED
    pairs = n_frames - 1

    def loop(first=False):
        res = [MTM.matchBlocks(frames[0 if first else p], frames[p + 1], grid, margin, method) for p in range(pairs)]
        return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])

    methods = {
        "stack_previous": lambda: MTM.matchBlocksStack(frames, grid, margin, method),
        "stack_first": lambda: MTM.matchBlocksStack(frames, grid, margin, method, reference="first"),
        "stack_ensemble": lambda: MTM.matchBlocksStack(frames, grid, margin, method, ensemble=True),
        "loop": loop,
    }
    results = {}
    for k, fn in methods.items():
        for _ in range(warmup):
            results[k] = fn()
    ms = {k: [] for k in methods}
    for _ in range(reps):
        for k, fn in methods.items():
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3 / pairs)
    med = {k: statistics.median(v) for k, v in ms.items()}

    def same(a, b):
        return bool((a[0] == b[0]).all() and a[1].tobytes() == b[1].tobytes())

    equal = same(results["stack_previous"], results["loop"]) and same(results["stack_first"], loop(first=True))
    noisy = noisy_movie(spec, min(n_frames, 8))
    step = (2, 1)
    ppos, _ = MTM.matchBlocksStack(noisy, grid, margin, method)
    epos, _, _ = MTM.matchBlocksStack(noisy, grid, margin, method, ensemble=True)
    found = lambda pos: float(np.mean((B.displacements(grid, pos) == step).all(axis=1)))     # noqa: E731
    return {
        "workload": name, "image": "%dx%dx%d %s" % (hw[0], hw[1], chans, dtype), "frames": n_frames, "pairs": pairs,
        "blocks": int(len(grid)), "block": side, "margin": margin, "map": "%dx%d" % (2 * margin + 1, 2 * margin + 1),
        "ms_per_pair": {k: round(v, 3) for k, v in med.items()},
        "ms_per_pair_min": {k: round(min(v), 3) for k, v in ms.items()},
        "speedup_vs_loop": {k: round(med["loop"] / med[k], 2) for k in ("stack_previous", "stack_first", "stack_ensemble")},
        "equal_to_loop": equal,
        "found_shift": float(np.mean((B.displacements(grid, results["stack_previous"][0][0]) == (3, -2)).all(axis=1))),
        "noisy_frames": len(noisy),
        "noisy_found_pairs": round(float(np.mean([found(p) for p in ppos])), 4),
        "noisy_found_ensemble": round(found(epos), 4),
        "reps": reps,
    }


def run_stack_passes(MTM, spec, n_frames, reps, warmup, ensemble):
    from MTM import blocks as B
    name, hw, chans, dtype, side, margin = spec
    frames = movie(spec, n_frames)
    method = MTM.TM_CCOEFF_NORMED
    pairs = n_frames - 1
    fine_margin = max(1, margin // 4)
    passes = [(side, 2 * side, margin), (side, side, fine_margin)]
    grid = B.grid(frames[0].shape, side)

    def loop_multipass(fr=frames):
        return [MTM.matchBlocksMultipass(fr[p], fr[p + 1], passes, method) for p in range(len(fr) - 1)]

    def by_hand(fr=frames):
        out, off, steer = [], None, None
        for p, (block, step, m) in enumerate(passes):
            b = B.grid(fr[0].shape, block, step)
            if p:
                off = B.predict_offsets(fr[0].shape, passes[p - 1][:2], steer, passes[p][:2])
            steer, sc, planes = MTM.matchBlocksStack(fr, b, m, method, ensemble=True, offsets=off)
            out.append((b, steer, sc, planes))
        return out

    if ensemble:
        methods = {"stack_passes_ensemble": lambda: MTM.matchBlocksStackMultipass(frames, passes, method, ensemble=True),
                   "by_hand": by_hand}
    else:
        methods = {"stack_passes": lambda: MTM.matchBlocksStackMultipass(frames, passes, method),
                   "loop_multipass": loop_multipass,
                   "stack_wide": lambda: MTM.matchBlocksStack(frames, grid, margin, method)}
    results = {}
    for k, fn in methods.items():
        for _ in range(warmup):
            results[k] = fn()
    ms = {k: [] for k in methods}
    for _ in range(reps):
        for k, fn in methods.items():
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3 / pairs)
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {
        "workload": name, "image": "%dx%dx%d %s" % (hw[0], hw[1], chans, dtype), "frames": n_frames, "pairs": pairs,
        "blocks": int(len(grid)), "block": side, "passes": [[b, st, m] for b, st, m in passes], "ensemble": ensemble,
        "ms_per_pair": {k: round(v, 3) for k, v in med.items()},
        "ms_per_pair_min": {k: round(min(v), 3) for k, v in ms.items()},
        "reps": reps,
    }
    if ensemble:
        out["equal_to_loop"] = all(bool((a[1] == b[1]).all() and a[2].tobytes() == b[2].tobytes() and
                                        np.array_equal(a[3], b[3], equal_nan=True))
                                   for a, b in zip(results["stack_passes_ensemble"], results["by_hand"]))
        out["vs_by_hand"] = round(med["by_hand"] / med["stack_passes_ensemble"], 2)
        step = (fine_margin + 2, -(fine_margin + 1))
        noisy = noisy_movie(spec, min(n_frames, 8), step=step)
        inner = (grid[:, 0] >= 2 * side) & (grid[:, 1] >= 2 * side) & (grid[:, 0] + 3 * side <= hw[1]) & \
            (grid[:, 1] + 3 * side <= hw[0])
        found = lambda pos: float(np.mean((B.displacements(grid, pos)[inner] == step).all(axis=1)))      # noqa: E731
        out.update({
            "noisy_frames": len(noisy), "noisy_step": list(step), "blocks_counted": int(inner.sum()),
            "noisy_found_pairs_multipass": round(float(np.mean(
                [found(p) for p in MTM.matchBlocksStackMultipass(noisy, passes, method)[1][1]])), 4),
            "noisy_found_ensemble_single": round(found(MTM.matchBlocksStack(noisy, grid, fine_margin, method, ensemble=True)[0]), 4),
            "noisy_found_ensemble_multipass": round(found(
                MTM.matchBlocksStackMultipass(noisy, passes, method, ensemble=True)[1][1]), 4)})
    else:
        loop = results["loop_multipass"]
        out["equal_to_loop"] = all(bool((g[1][q] == loop[q][p][1]).all() and g[2][q].tobytes() == loop[q][p][2].tobytes())
                                   for p, g in enumerate(results["stack_passes"]) for q in range(pairs))
        out["vs_loop_multipass"] = round(med["loop_multipass"] / med["stack_passes"], 2)
        out["vs_stack_wide"] = round(med["stack_wide"] / med["stack_passes"], 2)
        out["found_shift"] = float(np.mean((B.displacements(grid, results["stack_passes"][1][1][0]) == (3, -2)).all(axis=1)))
    return out


def quadrant_pair(spec, seed=0):
    """A reference and an image whose four quadrants are the reference's moved by four different shifts (dx, dy) within the
    workload's margin, with a little noise: (ref, img, shifts (2, 2, 2) by quadrant row and column)."""
    name, hw, chans, dtype, side, margin = spec
    ref, _ = workload(spec, seed)
    m = margin
    shifts = np.array([[(m - 1, -(m // 2)), (-(m - 2), 3)], [(2, m - 1), (-(m // 2 + 1), -(m - 1))]])
    rng = np.random.default_rng(seed + 40)
    top = 65535 if ref.dtype == np.uint16 else 255
    H, W = hw
    img = np.empty_like(ref)
    for qy, (y0, y1) in enumerate(((0, H // 2), (H // 2, H))):
        for qx, (x0, x1) in enumerate(((0, W // 2), (W // 2, W))):
            dx, dy = (int(v) for v in shifts[qy, qx])
            img[y0:y1, x0:x1] = np.roll(ref, (dy, dx), axis=(0, 1))[y0:y1, x0:x1]
    img = img.astype(np.int64) + rng.integers(-2, 3, size=ref.shape)
    return ref, np.clip(img, 0, top).astype(ref.dtype), shifts


def found_share(B, grid, pos, shape, shifts, margin):
    """The share of the blocks clear of the image's border and of the quadrants' seams (by a block and the margin) whose
    displacement is their quadrant's shift."""
    H, W = shape[0], shape[1]
    x, y, w, h = grid[:, 0], grid[:, 1], grid[:, 2], grid[:, 3]
    qx, qy = (x >= W // 2).astype(int), (y >= H // 2).astype(int)
    pad = margin + 1
    clear = (x >= pad) & (x + w <= W - pad) & (y >= pad) & (y + h <= H - pad)
    clear &= np.where(qx == 0, x + w + pad <= W // 2, x - pad >= W // 2)
    clear &= np.where(qy == 0, y + h + pad <= H // 2, y - pad >= H // 2)
    d = B.displacements(grid, pos)
    return float(np.mean((d[clear] == shifts[qy[clear], qx[clear]]).all(axis=1))), int(clear.sum())


def run_passes(MTM, spec, reps, warmup, far=False):
    from MTM import blocks as B
    name, hw, chans, dtype, side, margin = spec
    ref, img = workload(spec, shift=(margin - 1, -(margin - 2))) if far else workload(spec)
    method = MTM.TM_CCOEFF_NORMED
    fine_margin = max(1, margin // 4)
    passes = [(side, 2 * side, margin), (side, side, fine_margin)]
    grid = B.grid(ref.shape, side)
    single_margin = fine_margin if far else margin

    def by_hand(r=ref, i=img):
        out, off, steer = [], None, None
        for p, (block, step, m) in enumerate(passes):
            b = B.grid(i.shape, block, step)
            if p:
                off = B.predict_offsets(i.shape, passes[p - 1][:2], steer, passes[p][:2])
            steer, sc = MTM.matchBlocks(r, i, b, m, method, offsets=off)
            out.append((b, steer, sc))
        return out

    methods = {
        "single": lambda: MTM.matchBlocks(ref, img, grid, single_margin, method),
        "multipass": lambda: MTM.matchBlocksMultipass(ref, img, passes, method),
        "by_hand": by_hand,
    }
    results = {}
    for k, fn in methods.items():
        for _ in range(warmup):
            results[k] = fn()
    ms = {k: [] for k in methods}
    for _ in range(reps):
        for k, fn in methods.items():
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    equal = all(bool((a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2].tobytes() == b[2].tobytes())
                for a, b in zip(results["multipass"], results["by_hand"]))
    tiles = lambda n, m: n * (-(-(2 * m + 1) // 16)) ** 2      # noqa: E731
    out = {
        "workload": name + (" far" if far else ""), "image": "%dx%dx%d %s" % (hw[0], hw[1], chans, dtype),
        "blocks": int(len(grid)), "block": side, "single_margin": single_margin,
        "passes": [[b, st, m] for b, st, m in passes], "pass_blocks": [int(len(r[0])) for r in results["multipass"]],
        "tile_ratio": round(sum(tiles(len(r[0]), p[2]) for r, p in zip(results["multipass"], passes)) /
                            tiles(len(grid), margin), 3),
        "ms": {k: round(v, 3) for k, v in med.items()},
        "ms_min": {k: round(min(v), 3) for k, v in ms.items()},
        "multipass_vs_single": round(med["single"] / med["multipass"], 2),
        "multipass_vs_by_hand": round(med["by_hand"] / med["multipass"], 2),
        "equal_to_loop": equal, "reps": reps,
    }
    if far:
        shift = (margin - 1, -(margin - 2))
        inner = (grid[:, 0] >= 2 * side) & (grid[:, 1] >= 2 * side) & (grid[:, 0] + 3 * side <= hw[1]) & \
            (grid[:, 1] + 3 * side <= hw[0])
        share = lambda pos: round(float(np.mean((B.displacements(grid, pos)[inner] == shift).all(axis=1))), 4)  # noqa: E731
        out.update({"shift": list(shift), "found_single": share(results["single"][0]),
                    "found_multipass": share(results["multipass"][1][1]), "blocks_counted": int(inner.sum())})
    else:
        qref, qimg, shifts = quadrant_pair(spec)
        f_single, n_clear = found_share(B, grid, MTM.matchBlocks(qref, qimg, grid, margin, method)[0], hw, shifts, margin)
        f_multi, _ = found_share(B, grid, MTM.matchBlocksMultipass(qref, qimg, passes, method)[1][1], hw, shifts, margin)
        out.update({"quadrant_shifts": shifts.reshape(4, 2).tolist(), "found_single": round(f_single, 4),
                    "found_multipass": round(f_multi, 4), "blocks_counted": n_clear})
    return out


def flat_block_pair(spec, passes, seed=0):
    """The workload's pair with a flat patch planted in the reference over the middle block of the coarse pass's grid:
    (ref, img, (x, y, w, h) of the patch).  Under TM_CCOEFF_NORMED the flat block scores 1.0 everywhere and lands on its
    box's first output, a displacement of minus the coarse margin."""
    from MTM import blocks as B
    ref, img = workload(spec, seed)
    block, step, _ = passes[0]
    ny, nx = B.grid_shape(ref.shape, block, step)
    x, y = (nx // 2) * step, (ny // 2) * step
    ref = ref.copy()
    ref[y:y + block, x:x + block] = 77
    return ref, img, (x, y, block, block)


def run_passes_validate(MTM, spec, reps, warmup):
    from MTM import blocks as B
    name, hw, chans, dtype, side, margin = spec
    ref, img = workload(spec)
    method = MTM.TM_CCOEFF_NORMED
    fine_margin = max(1, margin // 4)
    passes = [(side, 2 * side, margin), (side, side, fine_margin)]
    threshold, epsilon = 2.0, 0.5

    def by_hand(r=ref, i=img):
        out, steer = [], None
        for p, (block, step, m) in enumerate(passes):
            b = B.grid(i.shape, block, step)
            off = None if p == 0 else B.predict_offsets(i.shape, passes[p - 1][:2], steer, passes[p][:2])
            pos, sc = MTM.matchBlocks(r, i, b, m, method, offsets=off)
            valid, repl = B.validate(B.grid_shape(i.shape, block, step), B.displacements(b, pos), threshold, epsilon)
            steer = b[:, :2] + repl
            out.append((b, pos, sc, valid))
        return out

    methods = {
        "validated": lambda: MTM.matchBlocksMultipass(ref, img, passes, method, validate=(threshold, epsilon)),
        "unvalidated": lambda: MTM.matchBlocksMultipass(ref, img, passes, method),
        "by_hand": by_hand,
    }
    results = {}
    for k, fn in methods.items():
        for _ in range(warmup):
            results[k] = fn()
    ms = {k: [] for k in methods}
    for _ in range(reps):
        for k, fn in methods.items():
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}

    def same(x, y):
        return all(bool((a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2].tobytes() == b[2].tobytes() and
                        (a[3] == b[3]).all()) for a, b in zip(x, y))

    fref, fimg, (px, py, pw, ph) = flat_block_pair(spec, passes)
    fval = MTM.matchBlocksMultipass(fref, fimg, passes, method, validate=(threshold, epsilon))
    fraw = MTM.matchBlocksMultipass(fref, fimg, passes, method)
    grid = fval[1][0]
    x, y, w, h = grid[:, 0], grid[:, 1], grid[:, 2], grid[:, 3]
    counted = ((x >= px + pw) | (x + w <= px) | (y >= py + ph) | (y + h <= py)) & (x >= 2 * side) & (y >= 2 * side) & \
        (x + 3 * side <= hw[1]) & (y + 3 * side <= hw[0])
    share = lambda pos: round(float(np.mean((B.displacements(grid, pos)[counted] == (3, -2)).all(axis=1))), 4)   # noqa: E731
    return {
        "workload": name, "image": "%dx%dx%d %s" % (hw[0], hw[1], chans, dtype),
        "passes": [[b, st, m] for b, st, m in passes], "pass_blocks": [int(len(r[0])) for r in results["validated"]],
        "threshold": threshold, "epsilon": epsilon,
        "ms": {k: round(v, 3) for k, v in med.items()},
        "ms_min": {k: round(min(v), 3) for k, v in ms.items()},
        "validate_cost_ms": round(med["validated"] - med["unvalidated"], 3),
        "validated_vs_by_hand": round(med["by_hand"] / med["validated"], 2),
        "flagged": [int((~r[3]).sum()) for r in results["validated"]],
        "equal_to_loop": same(results["validated"], results["by_hand"]) and same(fval, by_hand(fref, fimg)),
        "flat_patch": [int(px), int(py), int(pw), int(ph)], "flat_flagged": [int((~r[3]).sum()) for r in fval],
        "found_validated": share(fval[1][1]), "found_unvalidated": share(fraw[1][1]), "blocks_counted": int(counted.sum()),
        "reps": reps,
    }


def warped_pair(spec, kind, seed=0):
    """The workload's reference and the same content under a known smooth motion, resampled bilinearly in float64:
    (ref, img, field) with field(x, y) -> (dx, dy), where the block centred on (x, y) of the reference is found in the
    image.  "shear": dx = g (y - H / 2); "rotation": a rotation about the image centre.  Either way the largest
    displacement is 0.6 of the workload's margin."""
    name, hw, chans, dtype, side, margin = spec
    ref, _ = workload(spec, seed)
    H, W = hw
    cy, cx = (H - 1) / 2.0, (W - 1) / 2.0
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    if kind == "shear":
        g = 0.6 * margin / (H / 2.0)
        field = lambda x, y: (g * (y - cy), 0.0 * x)                    # noqa: E731
        sx, sy = xx - g * (yy - cy), yy
    else:
        th = 0.6 * margin / np.hypot(cy, cx)
        c, s = np.cos(th), np.sin(th)
        field = lambda x, y: (c * (x - cx) - s * (y - cy) - (x - cx), s * (x - cx) + c * (y - cy) - (y - cy))   # noqa: E731
        sx, sy = c * (xx - cx) + s * (yy - cy) + cx, -s * (xx - cx) + c * (yy - cy) + cy
    sx, sy = np.clip(sx, 0, W - 1), np.clip(sy, 0, H - 1)
    x0, y0 = np.minimum(np.floor(sx).astype(np.int64), W - 2), np.minimum(np.floor(sy).astype(np.int64), H - 2)
    tx, ty = sx - x0, sy - y0
    if ref.ndim == 3:
        tx, ty = tx[:, :, None], ty[:, :, None]
    v = ref.astype(np.float64)
    img = (v[y0, x0] * (1 - tx) + v[y0, x0 + 1] * tx) * (1 - ty) + (v[y0 + 1, x0] * (1 - tx) + v[y0 + 1, x0 + 1] * tx) * ty
    return ref, np.round(img).astype(ref.dtype), field


def device_copy_ms(nbytes, reps):
    """Milliseconds (device events, the median of `reps`) of one device-to-device copy of nbytes."""
    import ctypes
    with open("/proc/self/maps") as maps:       # (the runtime the library itself runs on, already in the process)
        hip = ctypes.CDLL(next((ln.split()[-1] for ln in maps if "libamdhip64" in ln), "libamdhip64.so"))

    def ok(rc):
        if rc != 0:
            raise RuntimeError("HIP call failed (%d)" % rc)
    src, dst, a, b = (ctypes.c_void_p() for _ in range(4))
    ok(hip.hipMalloc(ctypes.byref(src), ctypes.c_size_t(nbytes)))
    ok(hip.hipMalloc(ctypes.byref(dst), ctypes.c_size_t(nbytes)))
    ok(hip.hipMemset(src, 0, ctypes.c_size_t(nbytes)))
    ok(hip.hipEventCreate(ctypes.byref(a)))
    ok(hip.hipEventCreate(ctypes.byref(b)))
    out, ms = [], ctypes.c_float(0.0)
    for i in range(reps + 2):
        ok(hip.hipEventRecord(a, None))
        ok(hip.hipMemcpyAsync(dst, src, ctypes.c_size_t(nbytes), 3, None))      # 3: hipMemcpyDeviceToDevice
        ok(hip.hipEventRecord(b, None))
        ok(hip.hipEventSynchronize(b))
        ok(hip.hipEventElapsedTime(ctypes.byref(ms), a, b))
        if i >= 2:
            out.append(ms.value)
    for e in (a, b):
        ok(hip.hipEventDestroy(e))
    for p in (src, dst):
        ok(hip.hipFree(p))
    return statistics.median(out)


def run_passes_deform(MTM, spec, reps, warmup):
    """--passes --deform: the two passes with and without window deformation and the loop the deformed call documents,
    interleaved; the warp kernel against a device-to-device copy of the image's bytes; what deformation buys on a
    sheared and on a rotated pair."""
    from MTM import _lib
    from MTM import blocks as B
    name, hw, chans, dtype, side, margin = spec
    ref, img = workload(spec)
    method = MTM.TM_CCOEFF_NORMED
    passes = [(side, 2 * side, margin), (side, side, max(1, margin // 4))]

    def by_hand(r=ref, i=img):
        out, steer = [], None
        for p, (block, step, m) in enumerate(passes):
            b = B.grid(i.shape, block, step)
            if p == 0:
                searched, c = i, np.zeros((len(b), 2), np.int64)
            else:
                prev = passes[p - 1][:2]
                d = steer - B.grid(i.shape, *prev)[:, :2]
                searched = B.deform(i, B.displacement_field(i.shape, prev, d))
                c = B.field_at(i.shape, prev, d, b)
            pos_w, sc = MTM.matchBlocks(r, searched, b, m, method)
            steer = pos_w + ((c + 128) >> 8)
            out.append((b, steer, sc, c / 256.0))
        return out

    methods = {
        "deformed": lambda: MTM.matchBlocksMultipass(ref, img, passes, method, deform=True),
        "undeformed": lambda: MTM.matchBlocksMultipass(ref, img, passes, method),
        "by_hand": by_hand,
    }
    results = {}
    for k, fn in methods.items():
        for _ in range(warmup):
            results[k] = fn()
    ms = {k: [] for k in methods}
    for _ in range(reps):
        for k, fn in methods.items():
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}

    def same(x, y):
        return all(bool((a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2].tobytes() == b[2].tobytes() and
                        (a[3] == b[3]).all()) for a, b in zip(x, y))

    # the warp kernel alone (device events around its launch: the context's timing) against a copy of the same bytes
    ctx = _lib.default_context()
    coarse = passes[0][:2]
    d = B.displacements(results["deformed"][0][0], results["deformed"][0][1])
    warp = []
    for i in range(reps + 2):
        out = MTM.deformImage(img, coarse, d)
        if i >= 2:
            warp.append(ctx.timing()["total_ms"])
    warp_equal = bool(np.array_equal(out, B.deform(img, B.displacement_field(img.shape, coarse, d))))
    warp_ms, copy_ms = statistics.median(warp), device_copy_ms(img.nbytes, reps)

    motion = {}
    for kind in ("shear", "rotation"):
        r, i, field = warped_pair(spec, kind)
        row = {"equal_to_loop": same(MTM.matchBlocksMultipass(r, i, passes, method, deform=True), by_hand(r, i))}
        for key, flag in (("rigid", False), ("deformed", True)):
            b, pos, sc = MTM.matchBlocksMultipass(r, i, passes, method, refine=True, deform=flag)[-1][:3]
            x, y, w, h = (b[:, j] for j in range(4))
            inner = (x >= 2 * side) & (y >= 2 * side) & (x + 3 * side <= hw[1]) & (y + 3 * side <= hw[0])
            fx, fy = field(x + (w - 1) / 2.0, y + (h - 1) / 2.0)
            err = (pos - b[:, :2]) - np.stack((fx, fy), axis=1)
            row[key] = {"mean_score": round(float(sc[inner].mean()), 4),
                        "rms_error_px": round(float(np.sqrt((err[inner] ** 2).sum(axis=1).mean())), 4)}
        row["blocks_counted"] = int(inner.sum())
        motion[kind] = row
    return {
        "workload": name, "image": "%dx%dx%d %s" % (hw[0], hw[1], chans, dtype),
        "passes": [[b, st, m] for b, st, m in passes], "pass_blocks": [int(len(r[0])) for r in results["deformed"]],
        "ms": {k: round(v, 3) for k, v in med.items()},
        "ms_min": {k: round(min(v), 3) for k, v in ms.items()},
        "ms_max": {k: round(max(v), 3) for k, v in ms.items()},
        "deform_cost_ms": round(med["deformed"] - med["undeformed"], 3),
        "deformed_vs_by_hand": round(med["by_hand"] / med["deformed"], 2),
        "equal_to_loop": same(results["deformed"], results["by_hand"]),
        "warp_kernel_ms": round(warp_ms, 4), "device_copy_ms": round(copy_ms, 4), "image_bytes": int(img.nbytes),
        "warp_vs_copy": round(warp_ms / copy_ms, 2), "warp_equal_to_numpy": warp_equal,
        "motion": motion, "reps": reps,
    }


def run_passes_steer(MTM, spec, reps, warmup):
    """--passes --deform --steer refined: three passes - the dense pass repeated - undeformed, with deform=True and steered
    by refined positions (and steered with validation: the median test's kernel next to the two new ones in a kernel
    trace), interleaved; the steered call against the loop it documents; the RMS error of the refined displacements of
    all three on the sheared and the rotated pair with 2 and 3 passes, and (K1's row) on the tests' particle pair."""
    from MTM import blocks as B
    name, hw, chans, dtype, side, margin = spec
    ref, img = workload(spec)
    method = MTM.TM_CCOEFF_NORMED
    dense = (side, side, max(1, margin // 4))
    passes = [(side, 2 * side, margin), dense, dense]

    def by_hand(r, i, pl):
        out, S8, prev = [], None, None
        for p, (block, step, m) in enumerate(pl):
            b = B.grid(i.shape, block, step)
            if p == 0:
                searched, c = i, np.zeros((len(b), 2), np.int64)
            else:
                searched = B.deform(i, B.displacement_field(i.shape, prev, S8, q8=True))
                c = B.field_at(i.shape, prev, S8, b, q8=True)
            pos_w, sc = MTM.matchBlocks(r, searched, b, m, method)
            fine_w, _ = MTM.matchBlocks(r, searched, b, m, method, refine=True)
            D8 = B.to_q8(fine_w) - 256 * b[:, :2] + c
            S8, prev = B.smooth_displacements(B.grid_shape(i.shape, block, step), D8), (block, step)
            out.append((b, pos_w + ((c + 128) >> 8), sc, c / 256.0))
        return out

    methods = {
        "undeformed": lambda: MTM.matchBlocksMultipass(ref, img, passes, method),
        "deformed": lambda: MTM.matchBlocksMultipass(ref, img, passes, method, deform=True),
        "steered": lambda: MTM.matchBlocksMultipass(ref, img, passes, method, deform=True, steer="refined"),
        "steered_validated": lambda: MTM.matchBlocksMultipass(ref, img, passes, method, deform=True, steer="refined",
                                                              validate=True),
    }
    results = {}
    for k, fn in methods.items():
        for _ in range(warmup):
            results[k] = fn()
    ms = {k: [] for k in methods}
    for _ in range(reps):
        for k, fn in methods.items():
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}

    def same(x, y):
        return len(x) == len(y) and all(bool((a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2].tobytes() == b[2].tobytes()
                                             and (a[-1] == b[-1]).all()) for a, b in zip(x, y))

    calls = (("rigid", {}), ("deformed", {"deform": True}), ("steered", {"deform": True, "steer": "refined"}))
    motion = {}
    for kind in ("shear", "rotation"):
        r, i, field = warped_pair(spec, kind)
        for n_passes in (2, 3):
            pl = passes[:n_passes]
            row = {"equal_to_loop": same(MTM.matchBlocksMultipass(r, i, pl, method, deform=True, steer="refined"), by_hand(r, i, pl))}
            for key, kw in calls:
                b, pos, sc = MTM.matchBlocksMultipass(r, i, pl, method, refine=True, **kw)[-1][:3]
                x, y, w, h = (b[:, j] for j in range(4))
                inner = (x >= 2 * side) & (y >= 2 * side) & (x + 3 * side <= hw[1]) & (y + 3 * side <= hw[0])
                fx, fy = field(x + (w - 1) / 2.0, y + (h - 1) / 2.0)
                err = (pos - b[:, :2]) - np.stack((fx, fy), axis=1)
                row[key] = {"mean_score": round(float(sc[inner].mean()), 4),
                            "rms_error_px": round(float(np.sqrt((err[inner] ** 2).sum(axis=1).mean())), 4)}
            row["blocks_counted"] = int(inner.sum())
            motion["%s_%d_passes" % (kind, n_passes)] = row
    out = {
        "workload": name, "image": "%dx%dx%d %s" % (hw[0], hw[1], chans, dtype),
        "passes": [[b, st, m] for b, st, m in passes], "pass_blocks": [int(len(r[0])) for r in results["steered"]],
        "ms": {k: round(v, 3) for k, v in med.items()},
        "ms_min": {k: round(min(v), 3) for k, v in ms.items()},
        "ms_max": {k: round(max(v), 3) for k, v in ms.items()},
        "deform_cost_ms": round(med["deformed"] - med["undeformed"], 3),
        "steer_cost_ms": round(med["steered"] - med["deformed"], 3),
        "equal_to_loop": same(results["steered"], by_hand(ref, img, passes)),
        "motion": motion, "reps": reps,
    }
    if name == "K1":
        for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
            if p not in sys.path:
                sys.path.insert(0, p)
        import blocks_steer_model as S
        pr, pi = S.particle_pair()
        out["particle_pair"] = {}
        for n_passes in (2, 3, 6):
            pl = S.PARTICLE_PASSES[:2] + S.PARTICLE_PASSES[1:2] * (n_passes - 2)
            rms = S.three_rms(pr, pi, passes=pl)
            out["particle_pair"]["%d_passes" % n_passes] = dict(zip(("rigid", "deformed", "steered"), (round(v, 4) for v in rms)))
    return out


def run_second(MTM, spec, reps, warmup, radius, passes_form):
    """--second: the call with and without the second peak, interleaved; the second peaks against the brute-force model of
    tests/blocks_second_model.py over MTM.computeScoreMap of every block and its box."""
    for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import blocks_second_model as S
    from MTM import blocks as B
    name, hw, chans, dtype, side, margin = spec
    ref, img = workload(spec)
    method = MTM.TM_CCOEFF_NORMED
    if passes_form:
        passes = [(side, 2 * side, margin), (side, side, max(1, margin // 4))]
        methods = {"plain": lambda: MTM.matchBlocksMultipass(ref, img, passes, method),
                   "second": lambda: MTM.matchBlocksMultipass(ref, img, passes, method, second=radius)}
    else:
        grid = B.grid(ref.shape, side)
        methods = {"plain": lambda: [(grid,) + MTM.matchBlocks(ref, img, grid, margin, method)],
                   "second": lambda: [(grid,) + MTM.matchBlocks(ref, img, grid, margin, method, second=radius)]}
    results = {}
    for k, fn in methods.items():
        for _ in range(warmup):
            results[k] = fn()
    ms = {k: [] for k in methods}
    for _ in range(reps):
        for k, fn in methods.items():
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    equal, unchanged, steer, n_none, ratios = True, True, None, 0, []
    for p, (got, plain) in enumerate(zip(results["second"], results["plain"])):
        b, pos, sc, pos2, sc2 = got
        unchanged = unchanged and bool((pos == plain[1]).all() and sc.tobytes() == plain[2].tobytes())
        off = None if p == 0 else B.predict_offsets(img.shape, passes[p - 1][:2], steer, passes[p][:2])
        m = passes[p][2] if passes_form else margin
        exp = S.expected_seconds(ref, img, b.tolist(), off, m, method, radius, MTM.computeScoreMap, firsts=pos)
        try:
            S.same_seconds(pos2, sc2, exp)
        except AssertionError:
            equal = False
        steer = pos
        n_none += int(np.isnan(sc2).sum())
        ratio = B.peak_ratio(sc, sc2, method)
        ratios.append(round(float(np.median(ratio[~np.isnan(ratio)])), 3) if not np.isnan(ratio).all() else None)
    return {
        "workload": name, "image": "%dx%dx%d %s" % (hw[0], hw[1], chans, dtype), "form": "passes" if passes_form else "pair",
        "blocks": [int(len(r[0])) for r in results["second"]], "margin": [p[2] for p in passes] if passes_form else margin,
        "exclusion": radius, "ms": {k: round(v, 3) for k, v in med.items()}, "ms_min": {k: round(min(v), 3) for k, v in ms.items()},
        "second_cost_ms": round(med["second"] - med["plain"], 3), "equal_to_model": equal, "first_peaks_unchanged": unchanged,
        "without_second_peak": n_none, "median_peak_ratio": ratios, "reps": reps,
    }


def static_mask(hw, seed=0):
    """An (H, W) bool mask that keeps about 70 % of the pixels: a horizontal band (a channel wall) and discs (bodies in
    the flow) cut out, the discs added from a seeded generator until 30 % are gone."""
    H, W = hw
    rng = np.random.default_rng(seed + 50)
    mask = np.ones((H, W), bool)
    mask[int(0.46 * H):int(0.54 * H), :] = False
    yy, xx = np.mgrid[0:H, 0:W]
    while mask.mean() > 0.70:
        r = int(rng.integers(min(H, W) // 16, min(H, W) // 6))
        cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
        mask[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = False
    return mask


def run_mask(MTM, spec, reps, warmup, with_loop=True):
    """--mask: the masked call, the unmasked call on the same pair, both again through the offsets chain, and the by-hand
    loop through findMatches, interleaved."""
    from MTM import _lib
    from MTM import blocks as B
    name, hw, chans, dtype, side, margin = spec
    ref, img = (np.maximum(a, 1) for a in workload(spec))
    grid = B.grid(ref.shape, side)
    method = MTM.TM_CCORR_NORMED
    mask = static_mask(hw)
    kept = B.mask_fraction(mask, grid)
    grid = grid[kept > 0]           # (the loop has no answer for a block the mask removes entirely)
    ctx = _lib.default_context()

    def loop():
        pos, sc = [], []
        for x, y, w, h in grid.tolist():
            m = mask[y:y + h, x:x + w].astype(np.uint8)
            m = m if chans == 1 else np.repeat(m[:, :, None], chans, 2)
            hit, = MTM.findMatches([("b", ref[y:y + h, x:x + w], m)], img, method, N_object=1,
                                   searchBox=B.search_box((x, y, w, h), margin, img.shape))
            pos.append(hit[1][:2])
            sc.append(hit[2])
        return np.array(pos, dtype=np.int64), np.array(sc, dtype=np.float32)

    zeros = np.zeros((len(grid), 2), np.int32)
    methods = {
        "masked": lambda: MTM.matchBlocks(ref, img, grid, margin, method, mask=mask),
        "unmasked": lambda: MTM.matchBlocks(ref, img, grid, margin, method),
        "masked_at": lambda: MTM.matchBlocks(ref, img, grid, margin, method, mask=mask, offsets=zeros),
        "unmasked_at": lambda: MTM.matchBlocks(ref, img, grid, margin, method, offsets=zeros),
    }
    if with_loop:
        methods["loop"] = loop
    results = {}
    for k, fn in methods.items():
        for _ in range(warmup if k != "loop" else 1):
            results[k] = fn()
    ms = {k: [] for k in methods}
    dev = {k: [] for k in methods if k != "loop"}
    for _ in range(reps):
        for k, fn in methods.items():
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
            if k in dev:
                dev[k].append(ctx.timing()["total_ms"])
    med = {k: statistics.median(v) for k, v in ms.items()}
    dmed = {k: statistics.median(v) for k, v in dev.items()}
    (pos, sc), (lpos, lsc) = results["masked"], results.get("loop", (None, None))
    same = lambda a, b: bool((a[0] == b[0]).all() and a[1].tobytes() == b[1].tobytes())     # noqa: E731
    d = B.displacements(grid, pos)
    return {
        "workload": name, "image": "%dx%dx%d %s" % (hw[0], hw[1], chans, dtype), "blocks": int(len(grid)), "block": side,
        "margin": margin, "method": int(method), "mask_kept": round(float(mask.mean()), 4),
        "blocks_dropped_empty": int((kept == 0).sum()), "blocks_partly_masked": int(((kept > 0) & (kept < 1)).sum()),
        "ms": {k: round(v, 3) for k, v in med.items()},
        "ms_min": {k: round(min(v), 3) for k, v in ms.items()},
        "ms_max": {k: round(max(v), 3) for k, v in ms.items()},
        "device_ms": {k: round(v, 4) for k, v in dmed.items()},
        "device_ms_all": {k: [round(x, 4) for x in v] for k, v in dev.items()},
        "masked_vs_unmasked_device": round(dmed["masked"] / dmed["unmasked"], 3),
        "masked_at_vs_unmasked_at_device": round(dmed["masked_at"] / dmed["unmasked_at"], 3),
        "masked_vs_unmasked": round(med["masked"] / med["unmasked"], 3),
        "speedup_vs_loop": round(med["loop"] / med["masked"], 2) if with_loop else None,
        "equal_to_loop": same((pos, sc), (lpos, lsc)) if with_loop else None,
        "at_equal": same(results["masked_at"], results["masked"]) and same(results["unmasked_at"], results["unmasked"]),
        "found_shift": float(np.mean((d == (3, -2)).all(axis=1))),
        "reps": reps,
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None, help="run the one workload of this name (profiling runs)")
    ap.add_argument("--stack", type=int, default=0, metavar="F", help="the movie form: matchBlocksStack over F frames")
    ap.add_argument("--passes", action="store_true", help="coarse to fine: matchBlocksMultipass against the single pass")
    ap.add_argument("--validate", action="store_true", help="with --passes: the median test between the passes")
    ap.add_argument("--second", type=int, nargs="?", const=2, default=None, metavar="r",
                    help="the second peak with exclusion radius r (default 2): the pair call, or with --passes the passes")
    ap.add_argument("--deform", action="store_true", help="with --passes: window deformation between the passes")
    ap.add_argument("--steer", choices=["integer", "refined"], default="integer",
                    help="with --passes --deform: refined = the deformed passes steered by sub-pixel positions, three passes")
    ap.add_argument("--mask", action="store_true", help="a static mask over the reference: masked, unmasked and the loop (K1, K3)")
    ap.add_argument("--no-loop", action="store_true", help="with --mask: leave the by-hand loop out (profiler runs)")
    ap.add_argument("--ensemble", action="store_true", help="with --stack F --passes: the passes on ensemble planes")
    ap.add_argument("--out", default=None,
                    help="with --mask: the file the lines are written to (default profiles/blocks/mask_throughput.jsonl); with "
                         "--stack F --passes: appended to (default profiles/blocks/stack_passes_throughput.jsonl)")
    args = ap.parse_args()
    if args.mask and (args.passes or args.stack or args.second is not None):
        ap.error("--mask goes alone")
    if args.steer == "refined" and not args.deform:
        ap.error("--steer refined goes with --passes --deform")
    stack_passes = bool(args.stack and args.passes)
    if args.ensemble and not stack_passes:
        ap.error("--ensemble goes with --stack F --passes")
    if stack_passes and (args.stack < 2 or args.validate or args.deform or args.second is not None):
        ap.error("--stack F --passes takes two frames at least and goes with --ensemble only")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "blocks", "stack_passes_throughput.jsonl" if stack_passes
                                else "mask_throughput.jsonl")
    if args.validate and not args.passes:
        ap.error("--validate goes with --passes")
    if args.deform and (not args.passes or args.validate or args.second is not None):
        ap.error("--deform goes with --passes alone")
    if args.second is not None and (args.second < 0 or args.validate or args.stack):
        ap.error("--second takes a radius >= 0 and goes alone or with --passes")
    import build as mtm_build
    mtm_build.build()
    import MTM
    lines = []
    for spec in WORKLOADS:
        if args.only and spec[0] != args.only:
            continue
        if args.mask:
            if spec[3] == "uint8":
                lines.append(json.dumps(run_mask(MTM, spec, args.reps, args.warmup, not args.no_loop)))
                print(lines[-1], flush=True)
        elif stack_passes:
            lines.append(json.dumps(run_stack_passes(MTM, spec, args.stack, args.reps, args.warmup, args.ensemble)))
            print(lines[-1], flush=True)
        elif args.second is not None:
            print(json.dumps(run_second(MTM, spec, args.reps, args.warmup, args.second, args.passes)), flush=True)
        elif args.passes and args.deform and args.steer == "refined":
            print(json.dumps(run_passes_steer(MTM, spec, args.reps, args.warmup)), flush=True)
        elif args.passes and args.deform:
            print(json.dumps(run_passes_deform(MTM, spec, args.reps, args.warmup)), flush=True)
        elif args.passes and args.validate:
            print(json.dumps(run_passes_validate(MTM, spec, args.reps, args.warmup)), flush=True)
        elif args.passes:
            print(json.dumps(run_passes(MTM, spec, args.reps, args.warmup)), flush=True)
            if spec[0] == "K1":
                print(json.dumps(run_passes(MTM, spec, args.reps, args.warmup, far=True)), flush=True)
        elif args.stack:
            if args.stack < 2:
                ap.error("--stack needs two frames at least")
            print(json.dumps(run_stack(MTM, spec, args.stack, args.reps, args.warmup)), flush=True)
        else:
            print(json.dumps(run(MTM, spec, args.reps, args.warmup)), flush=True)
    if args.mask and lines and not args.no_loop:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if stack_passes and lines:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
