"""
The peak kernels - peaks_kernel, peaks_batch_kernel, peaks_sparse_kernel + compact_hits_kernel, verify_peaks_kernel,
cand_hash_insert_kernel + verify_hash_kernel, extremum_kernel, extremum_batch_kernel (csrc/mtm_k_peaks.hip.h) - on constructed
score maps, against the plain 3x3 reference of tests/peaks_model.py (-m gpu).

Through a search the kernels only see what the score kernel produced from an image: nobody chooses where a plateau, a tie or
a NaN falls.  Context.debug_peak_pass (mtm_debug_peak_pass) hands the very kernels, through the launchers a search call goes
through (csrc/mtm_peaks.hip; grids and capacities from csrc/mtm_peak_sizing.h), maps of the test's choosing: the table of tests/peaks_model.py (validated on the CPU
by tests/test_peaks_model_cpu.py) - map widths 2 .. 8, 252 .. 260, 511 .. 513 and heights 2 .. 130 in lists of 1, 2 and 33
maps of mixed sizes; single peaks, equal and greater pairs, plateaus on and across the seams of the 256-column by 32-row (8-row)
strips; negative qualities at the border under both border rules; thresholds at a pixel's value and one float32 below; trivial
maps; NaN, infinities and signed zeros; stacks of images with seams inside a strip, on a strip and on a work-group boundary;
flag sets with and without holes; rows of 1 .. 256 peaks through the 64-record staging buffer; a region that overflows;
candidate lists of 0 .. cand_cap + 5 records, a hash table whose probing wraps and chains 75 keys; extremum ties across
work-groups, waves and images.  Every content runs for maxima and minima and both borders, once over a map arena filled with
0xFF and once with 0x7F; the flagged-segment scan a third time over 0xFE.

No tolerance anywhere: every comparison in these kernels is an equality or an order of float32 values.  Records are compared
as sets, byte for byte (the order inside a list depends on atomics), counts exactly, and what lies beyond the count in the
record buffer must be what the test put there.
"""
import numpy as np
import pytest

import peaks_model as M

pytestmark = pytest.mark.gpu

_SENTINEL = 0xA5
_GUARD = 3                  # records behind hit_cap that no kernel may touch
_REACHED = set()            # structural features the cells that ran did reach (the last test of the file)


@pytest.fixture(scope="module")
def lib():
    import build as mtm_build
    mtm_build.build()
    from MTM import _lib
    assert _lib.load().mtm_device_count() >= 1
    assert _lib.HIT_DTYPE == M.HIT_DTYPE
    assert (_lib.PEAK_SCAN, _lib.PEAK_SCAN_BATCH, _lib.PEAK_SEGMENTS, _lib.PEAK_VERIFY_MAPS, _lib.PEAK_VERIFY_HASH, _lib.PEAK_EXTREMUM,
            _lib.PEAK_EXTREMUM_BATCH) == (M.SCAN, M.SCAN_BATCH, M.SEGMENTS, M.VERIFY_MAPS, M.VERIFY_HASH, M.EXTREMUM, M.EXTREMUM_BATCH)
    return _lib


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


def _sorted(a):
    return sorted(r.tobytes() for r in a)


def _call(ctx, c, pattern):
    records = np.frombuffer(bytes([_SENTINEL]) * (M.HIT_DTYPE.itemsize * (c.hit_cap + _GUARD)), dtype=M.HIT_DTYPE).copy()
    res = ctx.debug_peak_pass(M.maps_of(c), c.route, M.thr_of(c), mode_min=c.mode_min, border=c.border, hit_cap=c.hit_cap,
                              templ_hw=c.hw, img_rows=c.img_rows, flags=c.flags, holes=c.holes, cands=c.cands,
                              cand_count=c.cand_count, cand_cap=c.cand_cap, thr_q=c.thr_q, pattern=pattern, records=records)
    return res


def _check_list(c, res, want, n_written):
    """the first n_written records of the buffer against the true peaks `want`; everything behind them untouched"""
    got = res["records"][:n_written]
    g = _sorted(got)
    assert len(set(g)) == len(g), c.name                                # nothing twice
    if n_written == len(want):
        assert g == _sorted(want), c.name
    else:                                                               # a list that overflowed: a subset of the true peaks
        assert n_written < len(want) and set(g) <= set(_sorted(want)), c.name
    rest = res["records"][n_written:]
    assert rest.tobytes() == bytes([_SENTINEL]) * rest.nbytes, c.name


def run_case(ctx, c, pattern):
    """one call of the entry on the case's maps; every assertion of the sweep"""
    e = M.expect(c.name)
    res = _call(ctx, c, pattern)
    info = res["info"]
    n = len(c.qmaps)
    if c.route in (M.EXTREMUM, M.EXTREMUM_BATCH):
        keys, ext = (e.keys, e.ext) if c.route == M.EXTREMUM_BATCH else ([e.keys], [e.ext])
        assert res["keys"].reshape(len(keys), n, 2).tolist() == [[list(k) for k in row] for row in keys], c.name
        hits = res["ext_hits"].reshape(len(keys), n, 2)
        for b, row in enumerate(ext):
            for t, pair in enumerate(row):
                ow = c.qmaps[t].shape[1]
                m = M.maps_of(c)[t]
                for k in (0, 1):
                    h = hits[b, t, k]
                    assert (h["templ_idx"], h["w"], h["h"]) == (t, c.hw[t][1], c.hw[t][0]), c.name
                    if pair[k] is None:
                        assert (h["x"], h["y"]) == (0, 0) and np.isnan(h["score"]), c.name
                    else:
                        idx, v = pair[k]
                        assert (h["x"], h["y"]) == (idx % ow, idx // ow), (c.name, b, t, k)
                        # the record carries the map's value, a zero as +0 (the key folds the two)
                        y_img = idx // ow + (b * c.img_rows if c.route == M.EXTREMUM_BATCH else 0)
                        assert np.float32(h["score"]).tobytes() == (m[y_img, idx % ow] + np.float32(0.0)).tobytes(), c.name
        if c.route == M.EXTREMUM and max(q.size for q in c.qmaps) > 256 * 256:
            _REACHED.add("extremum-second-turn")
        return
    true = e.records
    count = res["count"]
    if c.route in (M.SCAN, M.SCAN_BATCH):
        assert count == len(true), c.name
        _check_list(c, res, true, min(count, c.hit_cap))
        nontrivial = np.asarray(e.nontrivial)
        assert res["raw"].tolist() == nontrivial.astype(int).tolist(), c.name
        assert res["trivial"].tolist() == (~nontrivial).astype(int).tolist(), c.name
        oh = [q.shape[0] for q in c.qmaps]
        if c.route == M.SCAN and (min(oh) + 31) // 32 + 4 <= info["grid_y"] * 4:
            _REACHED.add("idle-waves")
        if c.route == M.SCAN_BATCH and 5 * c.img_rows <= 32 and count:
            _REACHED.add("strip-spans-images")
    elif c.route == M.SEGMENTS:
        assert info["grid_x"] == max(M.n_strip_cols(q.shape[1]) for q in c.qmaps) and info["n_lists"] == n * info["grid_x"], c.name
        per_list = np.bincount(true["templ_idx"] * info["grid_x"] + true["x"] // M.STRIP_COLS, minlength=info["n_lists"])
        assert res["list_counts"][:info["n_lists"]].tolist() == per_list.tolist(), c.name
        cap_t = info["list_cap"]
        assert cap_t == max(256, min(c.hit_cap // 8, (64 << 20) // 24 // info["n_lists"])), c.name
        kept = np.minimum(per_list, cap_t)
        if (per_list <= cap_t).all():
            assert count == len(true), c.name
            _check_list(c, res, true, min(count, c.hit_cap))
        else:
            # an overflowed list counts 8 times, and the count exceeds the capacity whatever the sum
            assert count == max(int(np.where(per_list > cap_t, 8 * per_list, per_list).sum()), c.hit_cap + 1) > c.hit_cap, c.name
            n_written = min(int(kept.sum()), c.hit_cap)
            _check_list(c, res, true, n_written)
            off = np.concatenate([[0], np.cumsum(kept)])
            for k in range(info["n_lists"]):                # every region's records are peaks of that region; short ones complete
                part = res["records"][min(off[k], n_written):min(off[k + 1], n_written)]
                assert (part["templ_idx"] * info["grid_x"] + part["x"] // M.STRIP_COLS == k).all(), (c.name, k)
                if per_list[k] <= cap_t and off[k + 1] <= n_written:
                    mine = true[true["templ_idx"] * info["grid_x"] + true["x"] // M.STRIP_COLS == k]
                    assert _sorted(part) == _sorted(mine), (c.name, k)
            _REACHED.add("region-overflow")
        raw = res["raw"]
        got3 = [(int(r) & 0xFF, (int(r) >> 8) & 0xFF, (int(r) >> 16) & 0xFF) for r in raw]
        assert got3 == [tuple(b) for b in e.bytes3] and all(int(r) >> 24 == 0 for r in raw), c.name
        assert res["trivial"].tolist() == [int(not (b0 or (b1 and b2))) for b0, b1, b2 in e.bytes3], c.name
        rows = np.bincount((true["templ_idx"] * info["grid_x"] + true["x"] // M.STRIP_COLS) * 65536 + true["y"]) if len(true) else np.zeros(1)
        if rows.max() > 64:
            _REACHED.add("direct-path")
        # a flush with a full stage: in some 8-row strip of a list the model's row counts (the entry's counter agrees with
        # their sum) reach exactly 64 staged records with a further row of peaks behind them
        for k in np.nonzero(per_list)[0]:
            mine = true[true["templ_idx"] * info["grid_x"] + true["x"] // M.STRIP_COLS == k]
            per_row = np.bincount(mine["y"], minlength=8 * ((int(mine["y"].max()) + 8) // 8)).reshape(-1, 8)
            for strip in per_row:
                staged = 0
                for cnt in strip[strip > 0]:
                    if cnt > 64 or staged + cnt > 64:
                        if staged == 64:
                            _REACHED.add("full-stage-flush")
                        staged = 0
                    staged += cnt if cnt <= 64 else 0
        if min(q.shape[0] for q in c.qmaps) + 32 <= max(q.shape[0] for q in c.qmaps):
            _REACHED.add("idle-waves-segments")
    else:
        assert count == len(true), c.name
        _check_list(c, res, true, min(count, c.hit_cap))
        assert res["raw"].tolist() == e.tcount.tolist(), c.name
        assert res["trivial"].tolist() == [int(int(k) == q.size) for k, q in zip(e.tcount, c.qmaps)], c.name
        assert info["verify_blocks"] * 256 >= c.cand_cap, c.name
        if c.route == M.VERIFY_HASH:
            assert info["hash_slots"] == M.hash_slots(c.cand_cap) >= 2 * c.cand_cap, c.name
            if "hash-wrap" in c.tags:
                longest, wrapped, _ = M.probe_lengths(c.cands[:min(c.cand_count, c.cand_cap)], info["hash_slots"])
                if wrapped and longest > 64:
                    _REACHED.add("probe-wraps")
        # a list at its cap / beyond it: by the model's count of the pixels above the list's threshold, every one of which the
        # entry judged (its peak count is the model's)
        with np.errstate(invalid="ignore"):
            n_above = sum(int((q > c.thr_q).sum()) for q in c.qmaps)
        if n_above == c.cand_cap == c.cand_count and "margin" not in c.tags:
            _REACHED.add("list-at-cap")
        if n_above == c.cand_count > c.cand_cap:
            _REACHED.add("count-beyond-cap")


# 0xFF (NaN) and 0x7F (3.4e38); the flagged-segment scan also over 0xFE (-1.7e38): under `holes` a read of a segment that was
# never written shows for maxima over 0x7F and for minima over 0xFE only (fmaxf ignores the NaN of 0xFF)
_CELLS = [(g, pattern) for g in M.GROUPS for pattern in (0xFF, 0x7F) + ((0xFE,) if g.endswith("-segments") else ())]


@pytest.mark.parametrize("group,pattern", _CELLS, ids=["%s-%02x" % c for c in _CELLS])
def test_peak_pass_table(ctx, group, pattern):
    ctx.debug_poison(pattern, 4)
    failed = []
    for c in M.GROUPS[group]:               # (every case of the group runs: one failure does not hide the others)
        try:
            run_case(ctx, c, pattern)
        except AssertionError as err:
            failed.append((c.name, str(err)[:300]))
    assert not failed, ("%d of %d cases" % (len(failed), len(M.GROUPS[group])), [n for n, _ in failed], failed[:3])


def test_each_call_returns_its_own_result(ctx):
    """large and small launches of every route in turn: nothing of an earlier call's flags, counters, table or keys may show
    in a later one"""
    names = ["geo-33maps-scan-max-near", "hash-collisions-verify-hash-min-const", "geo-2maps-extra-holes1-segments-min-near",
             "region-overflow-holes1-segments-max-near", "verify-len1-verify-hash-max-near", "stage-need-holes0-segments-max-const",
             "extremum-extremum-max-near", "batch-rows5-h2-batch-min-const", "geo-2maps-scan-min-const",
             "verify-len300-verify-maps-max-const", "extremum-stack-rows32-extremum-batch-max-near", "hash-collisions-verify-hash-max-near",
             "trivial-all-pass-all-holes0-segments-max-near", "extremum-1map-extremum-max-near"]
    for k, name in enumerate(names + names[::-1]):
        run_case(ctx, M.CASE_BY_NAME[name], 0x7F if k % 2 else 0xFF)


def test_a_placed_set_and_the_options_survive_the_entry(lib):
    """the entry needs no image and no templates, and leaves a placed template set and the options as they were"""
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(90, 120), dtype=np.uint8)
    templs = [(img[10:22, 30:44].copy(), None), (img[50:70, 60:75].copy(), None)]
    c = lib.Context(0)
    try:
        c.set_templates(templs, 5)
        c.set_image(img)
        before = c.find_matches(lib.PEAKS_LOCAL, 0.6)
        opts = c.options()
        for name in ("geo-2maps-scan-max-near", "geo-2maps-need-holes1-segments-max-const", "verify-len257-verify-hash-max-near",
                     "extremum-1map-extremum-max-near"):
            run_case(c, M.CASE_BY_NAME[name], 0xFF)
        assert c.options() == opts
        after = c.find_matches(lib.PEAKS_LOCAL, 0.6)
        assert len(before) >= 2 and np.asarray(before).tobytes() == np.asarray(after).tobytes()
    finally:
        c.close()


def test_refused_arguments(lib, ctx):
    """(all of these are refused before anything is launched)"""
    q = np.zeros((4, 6), dtype=np.float32)
    with pytest.raises(lib.MtmError):
        ctx.debug_peak_pass([q], 7, 0.5)                                            # no such route
    with pytest.raises(lib.MtmError):
        ctx.debug_peak_pass([q], lib.PEAK_SCAN, 0.5, border=2)
    with pytest.raises(lib.MtmError):
        ctx.debug_peak_pass([q], lib.PEAK_SCAN, 0.5, hit_cap=0)
    with pytest.raises(lib.MtmError):
        ctx.debug_peak_pass([q[:1]], lib.PEAK_SCAN, 0.5)                            # a line map: the host's
    with pytest.raises(lib.MtmError):
        ctx.debug_peak_pass([q], lib.PEAK_SCAN, 0.5, hit_cap=8, records=np.zeros(7, dtype=M.HIT_DTYPE))
    with pytest.raises(lib.MtmError):
        ctx.debug_peak_pass([q], lib.PEAK_SCAN_BATCH, 0.5, templ_hw=[(2, 2)], img_rows=4)      # 4 + 2 - 1 rows: no whole images
    with pytest.raises(lib.MtmError):
        ctx.debug_peak_pass([q], lib.PEAK_SEGMENTS, 0.5)                            # no flags
    bad = np.zeros(1, dtype=M.HIT_DTYPE)
    bad["x"] = 6
    with pytest.raises(lib.MtmError):
        ctx.debug_peak_pass([q], lib.PEAK_VERIFY_MAPS, 0.5, cands=bad)              # a candidate outside its map
    with pytest.raises(lib.MtmError):
        ctx.debug_peak_pass([q], lib.PEAK_VERIFY_HASH, 0.5, cands=bad[:0], cand_count=3, cand_cap=8)   # records missing
    assert lib.load().mtm_debug_peak_pass(None, None) == -1


def test_refused_while_a_call_is_in_flight(lib):
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, size=(90, 120), dtype=np.uint8)
    c = lib.Context(0)
    try:
        c.set_templates([(img[10:22, 30:44].copy(), None)], 5)
        c.set_image(img)
        c.find_matches_async(lib.PEAKS_LOCAL, 0.6)
        try:
            with pytest.raises(lib.MtmError, match="in flight"):
                c.debug_peak_pass([np.zeros((4, 6), dtype=np.float32)], lib.PEAK_SCAN, 0.5)
        finally:
            hits = c.find_matches_wait()
        assert len(hits) >= 1
        run_case(c, M.CASE_BY_NAME["geo-2maps-scan-max-near"], 0xFF)
    finally:
        c.close()


def test_every_structure_of_the_kernels_is_reached(ctx):
    """one cell per structural feature, run here (whatever ran before, in whatever order): each passes every assertion of the
    sweep and is seen to reach its feature - from the entry's own counters and sizes and the model's counts"""
    assert sum(len(g) for g in M.GROUPS.values()) == len(M.CASES) >= 1000
    for name in ("stage-need-holes1-segments-min-near", "region-overflow-holes0-segments-max-near", "hash-collisions-verify-hash-max-const",
                 "verify-len300-verify-hash-max-near", "verify-len305-verify-maps-min-near", "batch-rows5-h2-batch-max-near",
                 "geo-33maps-scan-min-const", "geo-33maps-need-holes0-segments-max-near", "extremum-extremum-max-near"):
        run_case(ctx, M.CASE_BY_NAME[name], 0xFF)
    want = {"direct-path", "full-stage-flush", "region-overflow", "probe-wraps", "list-at-cap", "count-beyond-cap",
            "strip-spans-images", "idle-waves", "idle-waves-segments", "extremum-second-turn"}
    assert want <= _REACHED, want - _REACHED
