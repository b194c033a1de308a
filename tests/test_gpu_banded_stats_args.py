"""
The band arguments of launch_stats (csrc/mtm_stats.hip: StatBand - the stream of a banded call's statistics launches, its row
units, the image rows that have just arrived) where the banded images of test_gpu_parity.py do not reach.  Every banded
image there has cols % 4 == 0, so every band converts its layout inside its statistics launch: a band stream WITH layout
rows.  Here the columns are 1027: the bands' statistics launches go to the band stream with NO layout rows (the uint8 image:
the fused kernel reads the planes a kernel of the upload made; the uint16 image made from it: the byte-plane kernel over a
range of row units), and the first of them still clears the candidate header.  Two bands (0.3, 1) of an image just above the
2^20 pixels a banded call needs.

What is asserted is what test_fused_image_call_equals_two_calls asserts: the one-call search equals set_image +
set_templates + find_matches byte for byte, and the maps bit for bit - the two-call path takes the default arguments (the
whole image on the context's stream), so a band argument that went astray shows as a difference.
"""
import os

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

METHOD, THR = 5, 0.5


@pytest.fixture(scope="module")
def mtm():
    import build as mtm_build
    mtm_build.build()
    import MTM
    assert MTM._lib.load().mtm_device_count() >= 1, "no GPU visible to libmtm_hip"
    return MTM


@pytest.fixture(scope="module")
def scenes():
    img, units, _ = synth.make_workload(seed=31, image_hw=(1030, 1027), n_base=20, templ=32)
    assert img.shape == (1030, 1027) and img.dtype == np.uint8 and img.size == 1057810 and len(units) == 20
    assert all(u[1].shape == (32, 32) for u in units)
    img16 = img.astype(np.uint16) * 200 + 7
    small, small_units, _ = synth.make_workload(seed=32, image_hw=(300, 400), n_base=3, templ=32)
    return {"u8": (img, [(u[1], None) for u in units]),
            "u16": (img16, [(u[1].astype(np.uint16) * 200 + 7, None) for u in units[:4]]),
            "small": (small, [(u[1], None) for u in small_units])}


def test_banded_statistics_launches_without_layout_rows(mtm, scenes, monkeypatch):
    from MTM import _lib
    monkeypatch.setenv("MTM_UPLOAD_BANDS", "0.3,1")
    monkeypatch.setenv("MTM_BAND_MIN_FILL", "0")
    fused, plain, fresh = _lib.Context(0), _lib.Context(0), _lib.Context(0)
    try:
        for honly in (1, 0):
            fused.set_option(_lib.OPT_HITS_ONLY, honly)
            plain.set_option(_lib.OPT_HITS_ONLY, honly)
            for mode in (_lib.PEAKS_LOCAL, _lib.PEAKS_GLOBAL):
                for name in ("u8", "u16"):
                    im, tl = scenes[name]
                    a = fused.search(tl, im, METHOD, mode, THR)
                    plain.set_image(im)
                    plain.set_templates(tl, METHOD)
                    b = plain.find_matches(mode, THR)
                    assert len(a) == len(b) and len(a) >= len(tl), (name, honly, mode, len(a), len(b))
                    assert np.array_equal(a, b), (name, honly, mode)
                    if honly == 0 and mode == _lib.PEAKS_LOCAL:            # the last template's map, bit for bit
                        shape = (im.shape[0] - tl[-1][0].shape[0] + 1, im.shape[1] - tl[-1][0].shape[1] + 1)
                        assert np.array_equal(fused.last_score_map(len(tl) - 1, shape), plain.last_score_map(len(tl) - 1, shape)), name
        # the calls really ran in two bands: one score launch behind each band's statistics launch
        fused.set_option(_lib.OPT_HITS_ONLY, 1)
        for name in ("u8", "u16"):
            im, tl = scenes[name]
            fused.search(tl, im, METHOD, _lib.PEAKS_LOCAL, THR)
            if not any(os.environ.get(k) for k in ("MTM_FUSE_STATS", "MTM_KERNEL")):       # (tools/alt_modes.sh)
                assert fused.timing()["ncc_launches"] == 2, (name, fused.timing())
        # an image too small to band, through the same context: nothing of the bands' arguments survives the call
        im, tl = scenes["small"]
        assert im.shape == (300, 400)
        a = fused.search(tl, im, METHOD, _lib.PEAKS_LOCAL, THR)
        b = fresh.search(tl, im, METHOD, _lib.PEAKS_LOCAL, THR)
        plain.set_option(_lib.OPT_HITS_ONLY, 1)
        plain.set_image(im)
        plain.set_templates(tl, METHOD)
        assert len(a) >= len(tl) and np.array_equal(a, b) and np.array_equal(a, plain.find_matches(_lib.PEAKS_LOCAL, THR))
    finally:
        fused.close()
        plain.close()
        fresh.close()
