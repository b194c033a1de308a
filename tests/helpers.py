"""Shared helpers for the tests (fixtures loading, canonical hit ordering, engine stand-ins backed by the oracle)."""
import json
import os
import threading

import numpy as np

import mtm_oracle as O

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden():
    with open(os.path.join(GOLDEN_DIR, "golden.json")) as f:
        return json.load(f)


def load_coins():
    img = np.load(os.path.join(GOLDEN_DIR, "coins.npz"))["image"]
    assert img.shape == (303, 384) and img.dtype == np.uint8 and int(img.sum()) == 11269333
    return img


def coin_templates(image):
    small = image[37:37 + 38, 80:80 + 41]
    big = image[14:14 + 59, 302:302 + 65]
    return small, big


def hits_json(hits):
    return [[h[0], [int(v) for v in h[1]], float(np.float32(h[2]))] for h in hits]


def canon(hits):
    """Order-free canonical form (the reference's cross-template / tie order is thread timing)."""
    return sorted(hits_json(hits), key=lambda h: (-h[2], h[0], h[1]))


def assert_hits_equal(got, expected, tol=1e-4, ordered=True):
    got = hits_json(got) if got and not isinstance(got[0], list) else got
    if not ordered:
        got = sorted(got, key=lambda h: (h[0], h[1]))
        expected = sorted(expected, key=lambda h: (h[0], h[1]))
    assert len(got) == len(expected), (len(got), len(expected))
    for g, e in zip(got, expected):
        assert g[0] == e[0] and list(g[1]) == list(e[1]), (g, e)
        assert abs(g[2] - e[2]) <= tol * max(1.0, abs(e[2])), (g, e)


class OracleContext:
    """Implements the _lib.Context surface the host layer uses, on the oracle."""

    def __init__(self, hit_dtype, border=None):
        self.lock = threading.RLock()
        self.hit_dtype = hit_dtype
        self.border = border        # peak_local_max's border rule (None: the oracle's DEFAULT_PEAK_BORDER, "nearest")

    @staticmethod
    def _as_cv2_sees_it(a):
        # MTM_U16: the library takes uint16 pixels as they are; the reference casts them to float32
        # (exactly) before cv2.matchTemplate (MTM/__init__.py:71-74)
        return a.astype(np.float32) if a is not None and a.dtype == np.uint16 else a

    def set_image(self, image, downscale=1):
        self.image = self._as_cv2_sees_it(O.downscale_area(image, downscale))       # mtm_set_image_downscaled

    def set_templates(self, templates, method):
        self.templates, self.method = [(self._as_cv2_sees_it(t), self._as_cv2_sees_it(m)) for t, m in templates], method

    def score_map(self, idx, shape):
        t, m = self.templates[idx]
        out = O.match_template(self.image, t, self.method, mask=m)
        assert out.shape == tuple(shape)
        return out

    def search(self, templates, image, method, mode, thr):          # the engine interface (Context / Group)
        self.set_templates(templates, method)
        return self.find_matches_image(image, mode, thr)

    def find_matches_image(self, image, mode, thr):                 # mtm_find_matches_image
        self.set_image(image)
        return self._find(mode, thr)

    def find_matches(self, mode, thr, next_image=None):
        try:
            return self._find(mode, thr)
        finally:
            if next_image is not None:      # mtm_find_matches_next: the next image becomes current
                self.image = next_image

    def _find(self, mode, thr):
        rows = []
        for i, (t, m) in enumerate(self.templates):
            cmap = O.match_template(self.image, t, self.method, mask=m)
            if mode == 1:
                _, _, mn, mx = O.min_max_loc(cmap)
                peaks = [mn[::-1]] if self.method in (0, 1) else [mx[::-1]]
            elif self.method in (0, 1):
                peaks = O.find_local_min(cmap, thr, border=self.border)
            else:
                peaks = O.find_local_max(cmap, thr, border=self.border)
            rows += [(i, int(p[1]), int(p[0]), t.shape[1], t.shape[0], cmap[tuple(p)]) for p in peaks]
        return np.array(rows, dtype=self.hit_dtype) if rows else np.zeros(0, dtype=self.hit_dtype)



class FusedContext(OracleContext):
    """OracleContext with the fused search + NMS entry (mtm_find_matches_image_nms) and its native semantics:
    n_object < 0 means no limit.  The stand-in's search_nms is search + the library's host NMS (mtm_nms).
    Every call is recorded as (method, n_object) in `calls`."""

    def __init__(self, hit_dtype, border=None):
        super().__init__(hit_dtype, border)
        self.calls = []

    def search_nms(self, templates, image, method, thr, max_overlap, n_object=-1):
        from MTM import _lib
        self.calls.append((method, n_object))
        raw = self.search(templates, image, method, 0, thr)
        if len(raw) <= 1:                                   # MTM/NMS.py:53-55
            return raw
        idx = _lib.nms_hits(raw, thr, max_overlap, ascending=(method == 1))
        return raw[idx] if n_object < 0 else raw[idx][:n_object]
