#!/usr/bin/env python3
"""Milliseconds per frame, from numpy arrays to hit lists, of four ways to track templates through a stack of frames, one
JSON line per workload:
  track        - MTM.trackTemplates(templates, frames, tracks, margin): one native call for the whole stack
  matcher      - TemplateMatcher(templates).track(frames, tracks, margin): the same with the templates resident
  loop_boxes   - the loop of findMatchesInBoxes(..., N_object=1) calls and next_box a user writes without trackTemplates
  loop_matcher - the same loop with TemplateMatcher(templates, N_object=1).match_boxes
The results of track and matcher are checked equal to loop_boxes' (labels, boxes, float32 score bits), and the fraction
of (frame, track) hits at the true position is reported.

--refine times sub-pixel tracking instead, one JSON line per workload:
  track_refine   - MTM.trackTemplates(..., refine=True): the neighbourhoods scored inside the one native call
  matcher_refine - TemplateMatcher(templates).track(..., refine=True)
  track_then_refine - today's way: MTM.trackTemplates(...) followed by one MTM.refineHits call per frame
  track, matcher - the unrefined calls, for the refined call's overhead per frame
The results of track_refine and matcher_refine are checked equal to track_then_refine's (labels, float positions with ==,
sizes, float32 score bits).

--update RATE times adaptive templates (update=RATE) instead, one JSON line per workload:
  track_update - MTM.trackTemplates(..., update=RATE): every track's template blended with its hit's window on the device
  track        - the same call with update=None, for the adaptive call's overhead per frame
  loop_update  - the loop the adaptive call replaces: per frame and track one findMatchesInBoxes call with the track's
                 own template (a fresh mtm_set_templates each), next_box and MTM.tracking.blend_template
The result of track_update is checked equal to loop_update's (labels, boxes, float32 score bits, last templates).

--reacquire times the re-acquisition of lost tracks (reacquire=True, min_score 0.9) instead, one JSON line per workload,
on a variant of the workload in which one track in eight jumps to a random place, outside its box, after every 10th
frame:
  track_reacquire - MTM.trackTemplates(..., min_score, reacquire=True): lost tracks searched over the whole frame on the
                    device
  track           - the same call with reacquire=False (the jumped tracks stay lost), for the cost of the second searches
  loop_reacquire  - the loop the call replaces: findMatchesInBoxes per frame, a whole-frame findMatchesInBoxes for every
                    hit that fails, next_box
  match_whole     - for comparison, per jump frame one exhaustive matchTemplates(N_object=1) over the jumped tracks'
                    templates (milliseconds per such frame)
and on the unmodified workload with min_score -1, which every hit passes, so that nothing is ever lost (at 0.9 the
unmodified T1 and T2 lose tracks too: their pasted copies overlap at times):
  idle_reacquire, idle_track - reacquire=True and reacquire=False: the cost of the option when it has nothing to do
The result of track_reacquire is checked equal to loop_reacquire's (labels, boxes, float32 score bits).

--sets V (1 <= V <= 4) times tracks that carry a set of V same-shape variants - the template, its two flips and its 180
degree rotation - instead, one JSON line per workload, on a variant of the workload in which each object shows variant
(frame + track) % V of its set:
  track_sets     - MTM.trackTemplates(...) with tracks ((x, y, w, h), [j0 .. jV-1]): one unit per track and variant, the
                   variants of a set scored by one work-group per tile
  track_separate - the same variants as V separate single-template tracks each (V times the tracks; every one follows its
                   own maximum, so this is the cost of the search alone, not the set's result)
  loop_sets      - the loop the set call replaces: per frame one findMatchesInBoxes call over (box, set) regions, the best
                   hit of each region on the host, next_box
The result of track_sets is checked equal to loop_sets' (labels, boxes, float32 score bits).

Data: each frame is one of 8 synth.smooth_u8 backgrounds (uint16: 257 x that plus noise in the low byte) with each
track's template - a crop of another smooth_u8 image - pasted at a position that moves up to margin / 2 pixels per frame
in each direction.  Each method is warmed up first; the four are interleaved within a repetition; medians over the
repetitions.

Usage: tools/track_throughput.py [--reps 3] [--warmup 1] [--only T1|T2|T3] [--refine | --update RATE | --reacquire | --sets V]
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

# name, frames, (rows, cols), channels, dtype, tracks, template side, margin
WORKLOADS = [
    ("T1", 200, (1080, 1920), 1, "uint8", 64, 32, 16),
    ("T2", 100, (2048, 2048), 1, "uint16", 16, 48, 24),
    ("T3", 50, (2160, 3840), 3, "uint8", 8, 64, 32),
]
N_BACKGROUNDS = 8


def _image(seed, hw, chans, dtype, rng):
    import synth
    planes = [synth.smooth_u8(seed + 101 * c, hw) for c in range(chans)]
    img = planes[0] if chans == 1 else np.ascontiguousarray(np.stack(planes, axis=2))
    if dtype == "uint16":
        img = (img.astype(np.uint16) * 257 + rng.integers(0, 64, size=img.shape, dtype=np.uint16)).astype(np.uint16)
    return img


def workload(spec, seed=0, jumps=False):
    name, n_frames, hw, chans, dtype, n_tracks, side, margin = spec
    rng = np.random.default_rng(seed)
    backs = [_image(seed + 1 + b, hw, chans, dtype, rng) for b in range(N_BACKGROUNDS)]
    src = _image(seed + 99, hw, chans, dtype, rng)
    templs = []
    for k in range(n_tracks):
        y, x = int(rng.integers(0, hw[0] - side)), int(rng.integers(0, hw[1] - side))
        templs.append(("t%d" % k, np.ascontiguousarray(src[y:y + side, x:x + side])))
    pos = np.stack([rng.integers(0, hw[1] - side, n_tracks), rng.integers(0, hw[0] - side, n_tracks)], axis=1)
    frames = np.empty((n_frames,) + backs[0].shape, backs[0].dtype)
    truth = np.empty((n_frames, n_tracks, 2), np.int64)
    for f in range(n_frames):
        frames[f] = backs[f % N_BACKGROUNDS]
        for k in range(n_tracks):
            x, y = pos[k]
            frames[f, y:y + side, x:x + side] = templs[k][1]
        truth[f] = pos
        step = rng.integers(-(margin // 2), margin // 2 + 1, size=pos.shape)
        pos = np.clip(pos + step, 0, [hw[1] - side, hw[0] - side])
        if jumps and f % 10 == 9:           # one track in eight jumps to a random place (from a generator of its own)
            jr = np.random.default_rng(seed + 7919 * f)
            for k in range(0, n_tracks, 8):
                pos[k] = (int(jr.integers(0, hw[1] - side)), int(jr.integers(0, hw[0] - side)))
    tracks = [((max(0, int(x) - margin), max(0, int(y) - margin), side + 2 * margin, side + 2 * margin), k)
              for k, (x, y) in enumerate(truth[0])]
    return templs, frames, tracks, truth


def _key(res):
    return [[(h[0][0], tuple(int(v) for v in h[0][1]), np.float32(h[0][2]).tobytes()) for h in fr] for fr in res]


def _time(methods, reps, warmup):
    """Each method warmed up, then the methods interleaved within a repetition: (last results, milliseconds per method)."""
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
    return results, ms


def _rkey(res):
    return [[(h[0][0], tuple(h[0][1]), np.float32(h[0][2]).tobytes()) for h in fr] for fr in res]


def run_refine(MTM, spec, reps, warmup):
    name, n_frames, hw, chans, dtype, n_tracks, side, margin = spec
    templs, frames, tracks, truth = workload(spec)
    frame_list = list(frames)
    method = MTM.TM_CCOEFF_NORMED
    matcher = MTM.TemplateMatcher(templs, method)

    def then_refine():
        res = MTM.trackTemplates(templs, frames, tracks, margin, method)
        return [[[h] for h in MTM.refineHits(templs, f, [c[0] for c in fr], method)] for f, fr in zip(frame_list, res)]

    methods = {
        "track_refine": lambda: MTM.trackTemplates(templs, frames, tracks, margin, method, refine=True),
        "matcher_refine": lambda: matcher.track(frames, tracks, margin, refine=True),
        "track_then_refine": then_refine,
        "track": lambda: MTM.trackTemplates(templs, frames, tracks, margin, method),
        "matcher": lambda: matcher.track(frames, tracks, margin),
    }
    results, ms = _time(methods, reps, max(1, warmup))
    med = {k: statistics.median(v) for k, v in ms.items()}
    ref = _rkey(results["track_then_refine"])
    pos = MTM.tracking.positions(results["track_refine"])
    methods["track_refine"]()                       # (the default context's timing: this call's, upload to last launch)
    t = MTM._lib.default_context().timing()
    return {
        "workload": name, "mode": "refine", "frames": n_frames, "frame": "%dx%dx%d %s" % (hw[0], hw[1], chans, dtype),
        "tracks": n_tracks, "template": "%dx%d" % (side, side), "margin": margin,
        "ms_per_frame": {k: round(v / n_frames, 4) for k, v in med.items()},
        "ms_per_frame_min": {k: round(min(v) / n_frames, 4) for k, v in ms.items()},
        "ms_per_frame_max": {k: round(max(v) / n_frames, 4) for k, v in ms.items()},
        "speedup_vs_track_then_refine": {k: round(med["track_then_refine"] / med[k], 2)
                                         for k in ("track_refine", "matcher_refine")},
        "refine_overhead_us_per_frame": {"track": round((med["track_refine"] - med["track"]) / n_frames * 1e3, 1),
                                         "matcher": round((med["matcher_refine"] - med["matcher"]) / n_frames * 1e3, 1)},
        "track_refine_device_ms": round(float(t["total_ms"]), 3),
        "equal_to_track_then_refine": {k: _rkey(results[k]) == ref for k in ("track_refine", "matcher_refine")},
        "mean_abs_offset": round(float(np.mean(np.abs(pos - np.round(pos)))), 4),
        "reps": reps,
    }


def run_update(MTM, spec, reps, warmup, rate):
    from MTM.tracking import blend_template, next_box
    name, n_frames, hw, chans, dtype, n_tracks, side, margin = spec
    templs, frames, tracks, truth = workload(spec)
    frame_list = list(frames)
    method = MTM.TM_CCOEFF_NORMED

    def loop():
        cur, box, out = [templs[j][1] for _, j in tracks], [b for b, _ in tracks], []
        for f in frame_list:
            row = []
            for k, (_, j) in enumerate(tracks):
                r = MTM.findMatchesInBoxes([(templs[j][0], cur[k])], f, [box[k]], method, N_object=1)[0]
                x, y, w, h = r[0][1]
                cur[k] = blend_template(cur[k], f[y:y + h, x:x + w], rate)
                box[k] = next_box(box[k], r[0], margin, f.shape, method)
                row.append(r)
            out.append(row)
        return out, cur

    methods = {
        "track_update": lambda: MTM.trackTemplates(templs, frames, tracks, margin, method, update=rate, return_templates=True),
        "track": lambda: MTM.trackTemplates(templs, frames, tracks, margin, method),
        "loop_update": loop,
    }
    results, ms = _time(methods, reps, max(1, warmup))
    med = {k: statistics.median(v) for k, v in ms.items()}
    (got, last), (ref, ref_last) = results["track_update"], results["loop_update"]
    equal = _key(got) == _key(ref) and all(np.array_equal(a, b) for a, b in zip(last, ref_last))
    pos = np.array([[h[0][1][:2] for h in fr] for fr in got])
    methods["track_update"]()                       # (the default context's timing: this call's, upload to last launch)
    t = MTM._lib.default_context().timing()
    return {
        "workload": name, "mode": "update", "rate": rate, "frames": n_frames,
        "frame": "%dx%dx%d %s" % (hw[0], hw[1], chans, dtype), "tracks": n_tracks, "template": "%dx%d" % (side, side),
        "margin": margin,
        "ms_per_frame": {k: round(v / n_frames, 4) for k, v in med.items()},
        "ms_per_frame_min": {k: round(min(v) / n_frames, 4) for k, v in ms.items()},
        "ms_per_frame_max": {k: round(max(v) / n_frames, 4) for k, v in ms.items()},
        "speedup_vs_loop_update": round(med["loop_update"] / med["track_update"], 2),
        "update_overhead_us_per_frame": round((med["track_update"] - med["track"]) / n_frames * 1e3, 1),
        "track_update_device_ms": round(float(t["total_ms"]), 3),
        "equal_to_loop_update": bool(equal),
        "recovered": round(float(np.mean(np.all(pos == truth, axis=2))), 4),
        "reps": reps,
    }


def run_reacquire(MTM, spec, reps, warmup, min_score=0.9):
    from MTM.tracking import lost, next_box
    name, n_frames, hw, chans, dtype, n_tracks, side, margin = spec
    templs, frames, tracks, truth = workload(spec, jumps=True)
    _, idle_frames, idle_tracks, _ = workload(spec)
    frame_list = list(frames)
    method = MTM.TM_CCOEFF_NORMED
    whole = (0, 0, hw[1], hw[0])

    def loop():
        out, box, n_again = [], [b for b, _ in tracks], 0
        for f in frame_list:
            r = MTM.findMatchesInBoxes(templs, f, [(b, [j]) for b, (_, j) in zip(box, tracks)], method, N_object=1)
            again = [k for k, ri in enumerate(r) if not float(ri[0][2]) > min_score]
            if again:       # (one call for the frame's failed hits: kinder to the loop than one call per track)
                r2 = MTM.findMatchesInBoxes(templs, f, [(whole, [tracks[k][1]]) for k in again], method, N_object=1)
                for k, ri in zip(again, r2):
                    r[k] = ri
                n_again += len(again)
            out.append(r)
            box = [next_box(b, ri[0], margin, f.shape, method, min_score) for b, ri in zip(box, r)]
        return out, n_again

    jumped = [templs[j] for (_, j) in tracks[::8]]
    jump_frames = [f for i, f in enumerate(frame_list) if i % 10 == 0 and i > 0]

    def match_whole():
        return [MTM.matchTemplates(jumped, f, method, 1) for f in jump_frames]

    methods = {
        "track_reacquire": lambda: MTM.trackTemplates(templs, frames, tracks, margin, method, min_score, reacquire=True),
        "track": lambda: MTM.trackTemplates(templs, frames, tracks, margin, method, min_score),
        "loop_reacquire": loop,
        "idle_reacquire": lambda: MTM.trackTemplates(templs, idle_frames, idle_tracks, margin, method, -1.0,
                                                     reacquire=True),
        "idle_track": lambda: MTM.trackTemplates(templs, idle_frames, idle_tracks, margin, method, -1.0),
        "match_whole": match_whole,
    }
    results, ms = _time(methods, reps, max(1, warmup))
    med = {k: statistics.median(v) for k, v in ms.items()}
    got, (ref, n_again) = results["track_reacquire"], results["loop_reacquire"]

    def recovered(res):
        return round(float(np.mean(np.all(np.array([[h[0][1][:2] for h in fr] for fr in res]) == truth, axis=2))), 4)

    per = {k: v / n_frames for k, v in med.items() if k != "match_whole"}
    methods["track_reacquire"]()                    # (the default context's timing: this call's, upload to last launch)
    t_re = float(MTM._lib.default_context().timing()["total_ms"])
    methods["track"]()
    t_plain = float(MTM._lib.default_context().timing()["total_ms"])
    methods["idle_reacquire"]()
    t_idle_re = float(MTM._lib.default_context().timing()["total_ms"])
    methods["idle_track"]()
    t_idle = float(MTM._lib.default_context().timing()["total_ms"])
    return {
        "workload": name, "mode": "reacquire", "min_score": min_score, "frames": n_frames,
        "frame": "%dx%dx%d %s" % (hw[0], hw[1], chans, dtype), "tracks": n_tracks, "template": "%dx%d" % (side, side),
        "margin": margin, "second_searches": n_again,
        "ms_per_frame": {k: round(v, 4) for k, v in per.items()},
        "ms_per_frame_min": {k: round(min(v) / n_frames, 4) for k, v in ms.items() if k != "match_whole"},
        "ms_per_frame_max": {k: round(max(v) / n_frames, 4) for k, v in ms.items() if k != "match_whole"},
        "speedup_vs_loop_reacquire": round(med["loop_reacquire"] / med["track_reacquire"], 2),
        "ms_per_second_search": round((med["track_reacquire"] - med["track"]) / max(1, n_again), 4),
        "device_ms_per_second_search": round((t_re - t_plain) / max(1, n_again), 4),
        "match_whole_ms_per_jump_frame": round(med["match_whole"] / max(1, len(jump_frames)), 4),
        "idle_overhead_us_per_frame": round((per["idle_reacquire"] - per["idle_track"]) * 1e3, 1),
        "idle_device_overhead_us_per_frame": round((t_idle_re - t_idle) / n_frames * 1e3, 1),
        "idle_still_lost": int(lost(results["idle_reacquire"], method, -1.0).sum()),
        "track_reacquire_device_ms": round(t_re, 3), "track_device_ms": round(t_plain, 3),
        "equal_to_loop_reacquire": _key(got) == _key(ref),
        "idle_equal": _key(results["idle_reacquire"]) == _key(results["idle_track"]),
        "recovered": {"track_reacquire": recovered(got), "track": recovered(results["track"])},
        "still_lost": int(lost(got, method, min_score).sum()),
        "reps": reps,
    }


def run_sets(MTM, spec, reps, warmup, n_var):
    from MTM.tracking import next_box
    name, n_frames, hw, chans, dtype, n_tracks, side, margin = spec
    base, frames, tracks, truth = workload(spec)
    templs, sets = [], []
    for k, (label, t) in enumerate(base):
        variants = [t, t[:, ::-1], t[::-1], t[::-1, ::-1]][:n_var]
        sets.append(list(range(len(templs), len(templs) + n_var)))
        templs += [("%s.%d" % (label, v), np.ascontiguousarray(a)) for v, a in enumerate(variants)]
    shown = np.empty((n_frames, n_tracks), np.int64)
    for f in range(n_frames):               # (in track order, as workload pasted the originals)
        for k in range(n_tracks):
            x, y = truth[f, k]
            shown[f, k] = sets[k][(f + k) % n_var]
            frames[f, y:y + side, x:x + side] = templs[shown[f, k]][1]
    frame_list = list(frames)
    method = MTM.TM_CCOEFF_NORMED
    set_tracks = [(b, sets[k]) for k, (b, _) in enumerate(tracks)]
    separate = [(b, j) for k, (b, _) in enumerate(tracks) for j in sets[k]]

    def loop():
        out, box = [], [b for b, _ in set_tracks]
        for f in frame_list:
            r = MTM.findMatchesInBoxes(templs, f, [(b, js) for b, (_, js) in zip(box, set_tracks)], method, N_object=1)
            row = [[max(hits, key=lambda h: h[2])] for hits in r]
            out.append(row)
            box = [next_box(b, ri[0], margin, f.shape, method) for b, ri in zip(box, row)]
        return out

    methods = {
        "track_sets": lambda: MTM.trackTemplates(templs, frames, set_tracks, margin, method),
        "track_separate": lambda: MTM.trackTemplates(templs, frames, separate, margin, method),
        "loop_sets": loop,
    }
    results, ms = _time(methods, reps, max(1, warmup))
    med = {k: statistics.median(v) for k, v in ms.items()}
    got = results["track_sets"]
    pos = np.array([[h[0][1][:2] for h in fr] for fr in got])
    labels = np.array([[h[0][0] for h in fr] for fr in got])
    want = np.array([[templs[j][0] for j in row] for row in shown])
    methods["track_sets"]()                         # (the default context's timing: this call's, upload to last launch)
    t_sets = float(MTM._lib.default_context().timing()["total_ms"])
    methods["track_separate"]()
    t_sep = float(MTM._lib.default_context().timing()["total_ms"])
    return {
        "workload": name, "mode": "sets", "variants": n_var, "frames": n_frames,
        "frame": "%dx%dx%d %s" % (hw[0], hw[1], chans, dtype), "tracks": n_tracks, "template": "%dx%d" % (side, side),
        "margin": margin,
        "ms_per_frame": {k: round(v / n_frames, 4) for k, v in med.items()},
        "ms_per_frame_min": {k: round(min(v) / n_frames, 4) for k, v in ms.items()},
        "ms_per_frame_max": {k: round(max(v) / n_frames, 4) for k, v in ms.items()},
        "speedup_vs_loop_sets": round(med["loop_sets"] / med["track_sets"], 2),
        "speedup_vs_track_separate": round(med["track_separate"] / med["track_sets"], 2),
        "track_sets_device_ms": round(t_sets, 3), "track_separate_device_ms": round(t_sep, 3),
        "equal_to_loop_sets": _key(got) == _key(results["loop_sets"]),
        "recovered": round(float(np.mean(np.all(pos == truth, axis=2))), 4),
        "variant_named": round(float(np.mean(labels == want)), 4),
        "reps": reps,
    }


def run(MTM, spec, reps, warmup):
    from MTM.tracking import next_box
    name, n_frames, hw, chans, dtype, n_tracks, side, margin = spec
    templs, frames, tracks, truth = workload(spec)
    frame_list = list(frames)
    method = MTM.TM_CCOEFF_NORMED

    def loop(search):
        out, bxs = [], [b for b, _ in tracks]
        for f in frame_list:
            r = search(f, [(b, [j]) for b, (_, j) in zip(bxs, tracks)])
            out.append(r)
            bxs = [next_box(b, ri[0] if ri else None, margin, f.shape, method) for b, ri in zip(bxs, r)]
        return out

    matcher = MTM.TemplateMatcher(templs, method)
    matcher1 = MTM.TemplateMatcher(templs, method, N_object=1)
    methods = {
        "track": lambda: MTM.trackTemplates(templs, frames, tracks, margin, method),
        "matcher": lambda: matcher.track(frames, tracks, margin),
        "loop_boxes": lambda: loop(lambda f, reg: MTM.findMatchesInBoxes(templs, f, reg, method, N_object=1)),
        "loop_matcher": lambda: loop(matcher1.match_boxes),
    }
    results, ms = _time(methods, reps, warmup)
    med = {k: statistics.median(v) for k, v in ms.items()}
    ref = _key(results["loop_boxes"])
    equal = {k: _key(results[k]) == ref for k in ("track", "matcher", "loop_matcher")}
    got = np.array([[h[0][1][:2] for h in fr] for fr in results["track"]])
    recovered = float(np.mean(np.all(got == truth, axis=2)))
    methods["track"]()                              # (the default context's timing: this call's, upload to last launch)
    t = MTM._lib.default_context().timing()
    return {
        "workload": name, "frames": n_frames, "frame": "%dx%dx%d %s" % (hw[0], hw[1], chans, dtype), "tracks": n_tracks,
        "template": "%dx%d" % (side, side), "margin": margin,
        "ms_per_frame": {k: round(v / n_frames, 4) for k, v in med.items()},
        "ms_per_frame_min": {k: round(min(v) / n_frames, 4) for k, v in ms.items()},
        "ms_per_frame_max": {k: round(max(v) / n_frames, 4) for k, v in ms.items()},
        "speedup_vs_loop_boxes": {k: round(med["loop_boxes"] / med[k], 2) for k in ("track", "matcher", "loop_matcher")},
        "track_device_ms": round(float(t["total_ms"]), 3),
        "equal_to_loop_boxes": equal,
        "recovered": round(recovered, 4),
        "reps": reps,
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default=None, help="run the one workload of this name (profiling runs)")
    ap.add_argument("--refine", action="store_true", help="time sub-pixel tracking (refine=True) against today's way")
    ap.add_argument("--update", type=float, default=None, metavar="RATE",
                    help="time adaptive templates (update=RATE) against the plain call and the loop they replace")
    ap.add_argument("--reacquire", action="store_true",
                    help="time the re-acquisition of lost tracks (reacquire=True) against the plain call and the loop")
    ap.add_argument("--sets", type=int, default=None, metavar="V",
                    help="time tracks that carry V same-shape variants (1..4) against separate tracks and the loop")
    args = ap.parse_args()
    if args.refine + (args.update is not None) + args.reacquire + (args.sets is not None) > 1:
        ap.error("--refine, --update, --reacquire and --sets are separate measurements")
    if args.sets is not None and not 1 <= args.sets <= 4:
        ap.error("--sets takes 1 to 4 variants (the template, its flips and its 180 degree rotation)")
    import build as mtm_build
    mtm_build.build()
    import MTM
    for spec in WORKLOADS:
        if args.only and spec[0] != args.only:
            continue
        if args.sets is not None:
            rec = run_sets(MTM, spec, args.reps, args.warmup, args.sets)
        elif args.reacquire:
            rec = run_reacquire(MTM, spec, args.reps, args.warmup)
        elif args.update is not None:
            rec = run_update(MTM, spec, args.reps, args.warmup, args.update)
        else:
            rec = (run_refine if args.refine else run)(MTM, spec, args.reps, args.warmup)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
