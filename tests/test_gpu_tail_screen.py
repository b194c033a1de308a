"""The two-row MFMA kernel's tail screen (MfmaParams::tail_split: the K loop of a hits-only uint8 call stops after a split
where a Cauchy-Schwarz bound on the template rows still missing rules out every candidate of a wave) only skips work: the
hit records with it are identical to those of MTM_TAIL_SCREEN=0 - templates whose structure lies only in the rows after
the split, noisy copies, flat tail boxes, constant templates, thresholds within 1e-3 of the best scores of those templates
on both sides, partial row blocks and column segments, banded image uploads against single-band calls.  And on the
default routes it does skip work: the score kernel of a screened call takes clearly less time.

The screen only exists in the two-row tiling, which a normalised-method class takes at ceil(w / 16) % 4 == 0 alone: w in
49 .. 64.  The 64 x 40 and 20 x 24 cases are packed-K classes (nseg 3 and 2): no screen is compiled into the launch they
run, both contexts do the same thing - they stay as unscreened controls.  The cases where the screen runs say so through
Context.class_tilings() (tail_ok), among them widths that leave the last 16-tap segment partly padded (56, 49)."""
import os

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

# switches of tools/alt_modes.sh that move the work to another kernel, tiling or mode (where the screen does not run)
_OTHER_ROUTES = ("MTM_KERNEL", "MTM_HITS_ONLY", "MTM_F32_MFMA", "MTM_FUSE_STATS", "MTM_MFMA_R2", "MTM_SCREEN_L1",
                 "MTM_TAIL_SCREEN")


def _contexts(monkeypatch):
    from MTM import _lib
    monkeypatch.setenv("MTM_TAIL_SCREEN", "0")
    plain = _lib.Context()
    monkeypatch.delenv("MTM_TAIL_SCREEN")
    screened = _lib.Context()
    for c_ in (plain, screened):
        c_.set_option(_lib.OPT_HITS_ONLY, 1)
    return _lib, plain, screened


def _templates(rng, img, h, w, n):
    """n templates cut from the image; kind = i % 5: 0 exact, 1 structure only in the last third of the rows (flat top),
    2 noisy copy, 3 constant (the first two of that kind), 4 exact."""
    H, W = img.shape
    ts, kinds = [], []
    for i in range(n):
        y, x = int(rng.integers(0, H - h)), int(rng.integers(0, W - w))
        t = img[y:y + h, x:x + w].astype(np.int64)
        kind = i % 5
        if kind == 1:
            t[: (2 * h) // 3] = 128
        elif kind == 2:
            t = t + np.rint(rng.normal(0, 30, t.shape)).astype(np.int64)
        elif kind == 3 and i < 10:
            t[:] = 77
        ts.append(np.clip(t, 0, 255).astype(np.uint8))
        kinds.append(kind)
    return ts, kinds


def _screen_runs(h, w):
    """The class is one whose hits-only launches can screen their K loop (choose_tiling): two-row tiling, one K chunk."""
    return 49 <= w <= 64 and 8 <= h <= 71


@pytest.mark.parametrize("shape,h,w", [((300, 700), 64, 64), ((203, 517), 64, 40), ((150, 333), 32, 64), ((97, 290), 20, 24),
                                       ((203, 517), 64, 56), ((97, 290), 24, 49), ((150, 333), 71, 64)])
def test_tail_screen_changes_nothing(monkeypatch, shape, h, w):
    """Screened against MTM_TAIL_SCREEN=0.  The screen runs at 64 x 64, 32 x 64, 64 x 56, 24 x 49 and 71 x 64 (asserted:
    tail_ok, and - where the candidate list cannot overflow - a split carried by the TM_CCOEFF_NORMED call at 0.7); 64 x 40
    and 20 x 24 are packed-K classes, kept as unscreened controls (asserted too: no tail_ok there)."""
    _lib, plain, screened = _contexts(monkeypatch)
    default = not any(os.environ.get(k) for k in _OTHER_ROUTES)
    rng = np.random.default_rng(20261016 + h * 7 + w)
    try:
        img = rng.integers(0, 256, shape).astype(np.uint8)
        img[10:10 + h, 30:30 + w + 40] = 200                           # a flat patch: flat tail boxes
        img[shape[0] - h - 5:shape[0] - 5, 5:5 + w] = np.linspace(0, 255, w)[None, :].astype(np.uint8)
        ts, kinds = _templates(rng, img, h, w, 24)
        # a copy with only its tail rows planted into the image: a partial score that the tail must lift or not
        y, x = shape[0] // 2 - h // 2, shape[1] // 3
        img[y + h // 2:y + h, x:x + w] = ts[0][h // 2:]
        tl = [(t, None) for t in ts]
        n_rec = n_near = 0
        for method in (5, 3):
            # each template's best score (the screen is off at this threshold); thresholds 4e-4 on either side of those of
            # the tail-structured templates and the noisy copies, where a bound a little too low would lose a hit
            probe = plain.search(tl, img, method, _lib.PEAKS_LOCAL, 0.05)
            best = {}
            for r in probe:
                best[int(r["templ_idx"])] = max(best.get(int(r["templ_idx"]), -1.0), float(r["score"]))
            near = sorted(s for i, s in best.items() if kinds[i] in (1, 2) and 0.45 < s < 0.999)
            assert near, (shape, h, w, method, sorted(best.values())[-5:])
            thrs = [0.5, 0.7, 0.9]
            for s in near[:3] + near[-3:]:
                thrs += [s - 4e-4, s + 4e-4]
            for thr in thrs:
                a = screened.search(tl, img, method, _lib.PEAKS_LOCAL, thr)
                if default:
                    rec, = screened.class_tilings()
                    assert bool(rec["tail_ok"]) == _screen_runs(h, w) and (rec["kp_nseg"] > 0) == (not _screen_runs(h, w)), rec
                    # (a constant template scores 1 everywhere: at 300 x 700 the two of them alone put 2 x 237 x 637 outputs
                    # into a candidate list of 2^18 records - every call there overflows and is repeated in map mode, the
                    # comparison covers that fallback, not the screen)
                    if _screen_runs(h, w) and method == 5 and thr == 0.7 and 2 * (shape[0] - h + 1) * (shape[1] - w + 1) < 1 << 18:
                        assert rec["tail_split"] >= 6, rec
                b = plain.search(tl, img, method, _lib.PEAKS_LOCAL, thr)
                assert np.array_equal(a, b), (shape, h, w, method, thr, len(a), len(b))
                n_rec += len(a)
            n_near += len(near)
        assert n_rec > 0 and n_near >= 2
    finally:
        plain.close()
        screened.close()


@pytest.mark.parametrize("bands", ["0.25,1", "0.16,0.44,0.72,1"])
def test_tail_screen_banded_equals_single_band(monkeypatch, bands):
    """The banded image upload (statistics and score launch per row band: the headline's route), screened, against the
    same call with MTM_TAIL_SCREEN=0 and against the single-band call (set_image + find_matches), on 64 x 64 templates at
    thresholds where the screen runs; the banded call really ran in bands."""
    monkeypatch.setenv("MTM_UPLOAD_BANDS", bands)
    monkeypatch.setenv("MTM_BAND_MIN_FILL", "0")      # band this image too (by default a band must fill the chip)
    _lib, plain, screened = _contexts(monkeypatch)
    single = _lib.Context()
    single.set_option(_lib.OPT_HITS_ONLY, 1)
    try:
        img, units, _ = synth.make_workload(seed=7, image_hw=(1080, 1920), n_base=5, templ=64, rotations=4)
        tl = [(u[1], None) for u in units]
        n_rec = 0
        for thr in (0.5, 0.6, 0.95):
            a = screened.search(tl, img, 5, _lib.PEAKS_LOCAL, thr)
            t = screened.timing()
            b = plain.search(tl, img, 5, _lib.PEAKS_LOCAL, thr)
            single.set_image(img)
            single.set_templates(tl, 5)
            c = single.find_matches(_lib.PEAKS_LOCAL, thr)
            assert np.array_equal(a, b), (bands, thr, len(a), len(b))
            assert np.array_equal(a, c), (bands, thr, len(a), len(c))
            n_rec += len(a)
            if not any(os.environ.get(k) for k in _OTHER_ROUTES):
                assert 2 <= t["ncc_launches"] <= len(bands.split(",")), (bands, t["ncc_launches"])
                assert single.timing()["ncc_launches"] == 1
        assert n_rec >= len(tl)
    finally:
        plain.close()
        screened.close()
        single.close()


def test_tail_screen_skips_work(monkeypatch):
    """The screen does engage: on noise-like images with planted copies (the headline's kind of workload) the score kernel
    of the screened call runs well below the unscreened one (about 0.7 of it where waves leave after 42 of 65 steps), with
    the same records.  Minimum of several resident calls each, alternating."""
    _lib, plain, screened = _contexts(monkeypatch)
    try:
        img, units, _ = synth.make_workload(seed=3, image_hw=(1080, 1920), n_base=20, templ=64, noisy_per_unit=1)
        tl = [(u[1], None) for u in units]
        for c_ in (plain, screened):
            c_.set_image(img)
            c_.set_templates(tl, 5)
        ms = {"plain": [], "screened": []}
        for _ in range(6):
            for name, c_ in (("plain", plain), ("screened", screened)):
                c_.find_matches(_lib.PEAKS_LOCAL, 0.5)
                ms[name].append(c_.timing()["ncc_kernel_ms"])
        a = screened.find_matches(_lib.PEAKS_LOCAL, 0.5)
        b = plain.find_matches(_lib.PEAKS_LOCAL, 0.5)
        assert np.array_equal(a, b) and len(a) >= len(tl)
        if not any(os.environ.get(k) for k in _OTHER_ROUTES):
            assert min(ms["screened"]) < 0.85 * min(ms["plain"]), ms
    finally:
        plain.close()
        screened.close()
