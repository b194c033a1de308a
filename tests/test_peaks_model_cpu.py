"""
tests/peaks_model.py on the CPU: the plain reference of the peak pass against the oracle's peak_local_max_2d / min_max_loc on
every NaN-free map of the table, against a literal loop on small random maps with NaN, infinities and signed zeros, and the
premises the table of tests/test_gpu_peaks.py rests on - asserted, not assumed.
"""
import math

import numpy as np

import mtm_oracle as O
import peaks_model as M

F32 = np.float32
BORDER_NAME = {M.BORDER_CONSTANT: "constant", M.BORDER_NEAREST: "nearest"}


def _unique_maps():
    seen, out = set(), []
    for c in M.CASES:
        for q in c.qmaps:
            if id(q) not in seen:
                seen.add(id(q))
                out.append((q, float(c.thr_q)))
    return out


def test_model_equals_the_oracle_on_every_nan_free_map_of_the_table():
    maps = [(q, thr) for q, thr in _unique_maps() if not np.isnan(q).any()]
    assert len(maps) >= 150
    for q, thr in maps:
        for mode_min in (False, True):
            m = -q if mode_min else q               # the map a minima call would see; its quality is q again
            for border in (M.BORDER_CONSTANT, M.BORDER_NEAREST):
                rec, nontrivial = M.map_peaks(m, thr, mode_min, border)
                got = sorted(zip(rec["y"].tolist(), rec["x"].tolist())) if nontrivial else []
                ref = sorted(tuple(p) for p in O.peak_local_max_2d(M.quality(m, mode_min), F32(thr), BORDER_NAME[border]))
                assert got == ref, (q.shape, mode_min, border)
                assert rec["score"].tobytes() == m[rec["y"], rec["x"]].tobytes()
            lo, hi, (lx, ly), (hx, hy) = O.min_max_loc(m)
            a, b = M.extremum(m)
            assert (a[0], b[0]) == (hy * m.shape[1] + hx, ly * m.shape[1] + lx), q.shape
            assert (float(a[1]), float(b[1])) == (hi, lo)


def _literal(m, thr_q, mode_min, border):
    """the rules of the model's header, pixel by pixel"""
    oh, ow = m.shape
    pad = 0.0 if border == M.BORDER_CONSTANT else -math.inf
    peaks, nontrivial = [], False
    for y in range(oh):
        for x in range(ow):
            v = -float(m[y, x]) if mode_min else float(m[y, x])
            best = -math.inf
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    yy, xx = y + dy, x + dx
                    n = pad
                    if 0 <= yy < oh and 0 <= xx < ow:
                        n = -float(m[yy, xx]) if mode_min else float(m[yy, xx])
                    if not math.isnan(n) and n > best:
                        best = n
            if math.isnan(v) or v != best:
                nontrivial = True
            elif v > thr_q:
                peaks.append((y, x))
    return peaks, nontrivial


def _literal_extremum(m):
    best_hi = best_lo = None
    for i, v in enumerate(m.ravel().tolist()):
        if math.isnan(v):
            continue
        if best_hi is None or v > best_hi[1]:
            best_hi = (i, v)
        if best_lo is None or v < best_lo[1]:
            best_lo = (i, v)
    return best_hi, best_lo


def test_model_equals_a_literal_loop_on_small_maps_with_nan_inf_and_signed_zeros():
    rng = np.random.default_rng(7)
    pool = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 0.25, -0.25, 0.5, 0.75, -0.5], dtype=F32)
    for k in range(200):
        oh, ow = int(rng.integers(1, 8)), int(rng.integers(1, 9))
        m = pool[rng.integers(0, len(pool) if k % 3 else 5, size=(oh, ow))]
        if k % 5 == 0:
            m = np.where(rng.random((oh, ow)) < 0.8, F32(0.25), m).astype(F32)
        for mode_min in (False, True):
            for border in (M.BORDER_CONSTANT, M.BORDER_NEAREST):
                for thr_q in (-1.0, 0.0, 0.3):
                    rec, nontrivial = M.map_peaks(m, thr_q, mode_min, border, t=3, hw=(4, 5))
                    ref, ref_nt = _literal(m, thr_q, mode_min, border)
                    assert sorted(zip(rec["y"].tolist(), rec["x"].tolist())) == ref and nontrivial == ref_nt, (k, m)
                    assert rec["score"].tobytes() == m[rec["y"], rec["x"]].tobytes()          # the sign of a zero too
                    assert set(rec["templ_idx"]) <= {3} and set(rec["w"]) <= {5} and set(rec["h"]) <= {4}
                    # all flags set: the flagged scan is the scan
                    fl = np.ones((oh, M.n_strip_cols(ow)), dtype=np.uint8)
                    for holes in (False, True):
                        srec, bytes3 = M.segment_peaks(m, fl, holes, thr_q, mode_min, border, t=3, hw=(4, 5))
                        assert srec.tobytes() == rec.tobytes() and bytes3 == (int(nontrivial), 1, 0)
        hi, lo = _literal_extremum(m)
        a, b = M.extremum(m)
        if hi is None:
            assert a is None and b is None and M.extremum_keys(m) == (0, 0)
        else:
            assert (a[0], float(a[1])) == hi and (b[0], float(b[1])) == lo, m
            kmax, kmin = M.extremum_keys(m)
            assert 0xFFFFFFFF - (kmax & 0xFFFFFFFF) == hi[0] and 0xFFFFFFFF - (kmin & 0xFFFFFFFF) == lo[0]


def test_float_order_is_monotonic_and_folds_the_zeros():
    v = np.array([-np.inf, -3.0, -1e-30, -0.0, 0.0, 1e-30, 0.5, np.inf], dtype=F32)
    o = [M.float_order(x) for x in v]
    assert o == sorted(o) and o[3] == o[4] and len(set(o)) == len(o) - 1


def test_flags_cover_everything_above_the_threshold():
    """every SEGMENTS case flags each segment that holds a pixel above the threshold; with all of a case's flags the model's
    flagged scan finds the full scan's peaks, holes or not (an unflagged neighbour is below every peak either way)"""
    n = 0
    for c in M.CASES:
        if c.route != M.SEGMENTS:
            continue
        n += 1
        assert c.flags.shape == (len(c.qmaps), max(q.shape[0] for q in c.qmaps), max(M.n_strip_cols(q.shape[1]) for q in c.qmaps))
        for t, q in enumerate(c.qmaps):
            need = M.necessary_flags(q, c.thr_q)
            have = c.flags[t, :q.shape[0], :need.shape[1]]
            assert (have[need != 0] != 0).all(), c.name
            if c.holes:         # what the device never gets holds nothing above the threshold
                with np.errstate(invalid="ignore"):
                    assert not (q[~M.pixel_flags(c.flags[t], *q.shape)] > c.thr_q).any(), c.name
        m = M.maps_of(c)
        full = np.concatenate([M.map_peaks(mm, c.thr_q, c.mode_min, c.border, t, c.hw[t])[0] for t, mm in enumerate(m)])
        assert sorted(r.tobytes() for r in M.expect(c.name).records) == sorted(r.tobytes() for r in full), c.name
    assert n >= 300


def test_candidate_lists_hold_every_pixel_above_their_threshold_once():
    n = 0
    for c in M.CASES:
        if c.route not in (M.VERIFY_MAPS, M.VERIFY_HASH):
            continue
        n += 1
        pos = list(zip(c.cands["templ_idx"].tolist(), c.cands["y"].tolist(), c.cands["x"].tolist()))
        assert len(set(pos)) == len(pos), c.name
        margin = F32(0.1875) if "margin" in c.tags else F32(0.0)
        with np.errstate(invalid="ignore"):
            above = sum(int((q > c.thr_q - margin).sum()) for q in c.qmaps)
        assert above == len(pos), c.name
        for t, m in enumerate(M.maps_of(c)):
            sel = c.cands["templ_idx"] == t
            assert c.cands["score"][sel].tobytes() == m[c.cands["y"][sel], c.cands["x"][sel]].tobytes(), c.name
        if "margin" in c.tags:
            with np.errstate(invalid="ignore"):
                assert sum(int(((q > c.thr_q - margin) & ~(q > c.thr_q)).sum()) for q in c.qmaps) > 50
        if "beyond-cand-cap" in c.tags:
            assert c.cand_count == len(pos) == c.cand_cap + 5
        else:
            assert c.cand_count == len(pos) <= c.cand_cap, c.name
            # a complete list: judged against the maps or against the list alone, the peaks are the full scan's
            full = np.concatenate([M.map_peaks(m, c.thr_q, c.mode_min, c.border, t, c.hw[t])[0] for t, m in enumerate(M.maps_of(c))])
            assert sorted(r.tobytes() for r in M.expect(c.name).records) == sorted(r.tobytes() for r in full), c.name
    assert n >= 300
    lens = {c.cand_count for c in M.CASES if c.name.startswith("verify-len")}
    assert lens == {0, 1, 255, 256, 257, M.VERIFY_CAP - 1, M.VERIFY_CAP, M.VERIFY_CAP + 5}


def test_cases_meant_to_reach_a_structure_reach_it():
    by_tag = lambda tag: [c for c in M.CASES if tag in c.tags]            # noqa: E731
    # region overflow: by the model's own count, more peaks in one (map, strip column) than a list of hit_cap / 8 holds - and
    # than the floor of 256 -, the other lists short; the reported count will exceed hit_cap
    over = [c for c in by_tag("region-overflow")]
    assert len(over) >= 4
    for c in over:
        rec = M.expect(c.name).records
        per_list = np.bincount(rec["templ_idx"] * 2 + rec["x"] // M.STRIP_COLS, minlength=4)
        cap_t = max(256, c.hit_cap // 8)
        assert per_list[0] > cap_t and per_list[0] > c.hit_cap and (per_list[1:] < cap_t).all() and per_list[1] > 0, per_list
        scan = M.CASE_BY_NAME[c.name.replace("-segments-", "-scan-")]
        assert len(M.expect(scan.name).records) == len(rec) <= scan.hit_cap
    # the staging buffer: rows of 1, 63, 64, 65, 128 and 256 peaks, strips whose rows sum to exactly 64 / to 65 before a
    # further row, a row of more than 64 behind a partly filled stage
    stage = by_tag("stage")
    assert len(stage) >= 16
    for c in stage:
        rec = M.expect(c.name).records
        rec = rec[(rec["templ_idx"] == 0) & (rec["x"] < M.STRIP_COLS)]
        rows = np.bincount(rec["y"], minlength=8 * len(M.STAGE_SEQUENCES))
        seqs = [[int(v) for v in rows[8 * s:8 * s + 8] if v] for s in range(len(M.STAGE_SEQUENCES))]
        assert seqs == M.STAGE_SEQUENCES, seqs
    flat = [v for s in M.STAGE_SEQUENCES for v in s]
    assert {1, 63, 64, 65, 128, 256} <= set(flat)
    assert any(sum(s[:k]) == 64 and len(s) > k for s in M.STAGE_SEQUENCES for k in (1, 2))          # a flush with a full stage
    assert any(sum(s[:2]) == 65 and s[0] < 64 for s in M.STAGE_SEQUENCES if len(s) > 1)              # ... one record too many
    assert any(0 < s[0] < 64 < s[1] for s in M.STAGE_SEQUENCES if len(s) > 1)                        # direct behind a stage
    # the hash table: 40 + keys start in the last three slots, an insertion wraps, one chain is longer than 64
    wrap = [c for c in by_tag("hash-wrap") if c.route == M.VERIFY_HASH]
    assert len(wrap) == 4
    for c in wrap:
        longest, wrapped, at_end = M.probe_lengths(c.cands[:min(c.cand_count, c.cand_cap)], M.hash_slots(c.cand_cap))
        assert at_end >= 40 and wrapped >= 30 and longest > 64, (longest, wrapped, at_end)
        assert {0, 32} <= set(c.cands["templ_idx"].tolist()) and len(c.qmaps) == 33
        assert ((c.cands["x"] == 512) & (c.cands["y"] == 129) & (c.cands["templ_idx"] == 32)).any()
        assert len(c.cands) <= c.cand_cap
    # hit_cap below the number of peaks
    for c in by_tag("hit-cap-below"):
        assert len(M.expect(c.name).records) > c.hit_cap
    # every pixel a peak / trivial maps
    for c in by_tag("every-pixel-a-peak"):
        if c.route in (M.VERIFY_MAPS, M.VERIFY_HASH):
            assert int(M.expect(c.name).tcount[0]) == c.qmaps[0].size
    assert any(any(M.expect(c.name).nontrivial) and not all(M.expect(c.name).nontrivial)
               for c in by_tag("trivial") if c.route == M.SCAN)           # trivial maps beside nontrivial ones in one launch
    # stacks: a strip of 32 rows spans more than 4 images, a trivial image among nontrivial ones, seams inside a strip, on a
    # strip boundary and on a work-group boundary
    batch = by_tag("batch")
    assert {c.img_rows for c in batch} == set(M.BATCH_IMG_ROWS) == {5, 31, 32, 33, 64}
    assert any(c.img_rows * 5 <= 32 for c in by_tag("strip-spans-images"))
    for c in batch:
        nt = np.asarray(M.expect(c.name).nontrivial)
        assert not nt[2, 0] and nt[:, 0].sum() == nt.shape[0] - 1, c.name
        assert {c.hw[0][0] for c in batch if c.img_rows == 31} == {2, 3, 30}
        # peaks on the first and the last owned row of the images, none on a seam row
        rec = M.expect(c.name).records
        yl = rec["y"] % c.img_rows
        assert (yl <= c.img_rows - c.hw[0][0]).all() and (yl == 0).any() and (yl == c.img_rows - c.hw[0][0]).any(), c.name
    # lists of 1, 2 and 33 maps; launches in which smaller maps leave whole waves idle
    assert {len(c.qmaps) for c in M.CASES} >= {1, 2, 33}
    assert any(min(q.shape[0] for q in c.qmaps) + 32 <= max(q.shape[0] for q in c.qmaps) for c in by_tag("idle-waves"))
    # the sizes of the sweep
    ows = {q.shape[1] for c in M.CASES for q in c.qmaps}
    ohs = {q.shape[0] for c in M.CASES for q in c.qmaps}
    assert set(M.OWS) <= ows and set(M.OHS) <= ohs and max(ows) == 513
    assert max(q.shape[0] for c in M.CASES if c.route not in (M.SCAN_BATCH, M.EXTREMUM_BATCH) for q in c.qmaps) == 130


def test_extremum_cases_tie_across_work_groups_and_images():
    c = M.CASE_BY_NAME["extremum-extremum-max-near"]
    q = c.qmaps[0].ravel()
    ties = np.nonzero(q == q.max())[0]
    assert len(ties) >= 5 and len({int(i) // 256 for i in ties}) >= 4 and len({(int(i) // 64) % 4 for i in ties}) >= 2
    assert len({int(i) // 65536 for i in ties}) >= 2            # ... and in different turns of the grid-stride loop
    e = M.expect(c.name)
    assert e.keys[3] != (0, 0) and e.keys[4] == (0, 0)
    assert e.ext[1][0][0] == 0 and e.ext[1][1][0] == 0 and e.ext[2][0][0] == 0          # the earlier zero wins, whichever it is
    for c in [c for c in M.CASES if "extremum-stack" in c.tags]:
        e = M.expect(c.name)
        per_img = [e.ext[b][0] for b in range(4)]
        assert per_img[1][0][0] == per_img[3][0][0] == 258 + 5 and float(per_img[1][0][1]) == 0.75, c.name
        assert per_img[1][1][0] == per_img[3][1][0] == 100 and float(per_img[1][1][1]) == -0.75, c.name
        assert np.abs(c.qmaps[0]).max() == 2.0 and all(abs(float(v[k][1])) < 2.0 for v in per_img for k in (0, 1))
