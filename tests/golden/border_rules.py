"""
The border rule of skimage.feature.peak_local_max, for the generators in this directory (build container only).

scikit-image 0.18.3 (the only release importable there) runs its 3x3 maximum filter with mode='constant'; releases
>= 0.19 pass mode='nearest', the library's default.  ``nearest_border()`` runs the same 0.18.3 code with that one
argument replaced: the "@nearest" fixtures.
"""
import contextlib

import skimage.feature.peak as _pk


class _NdiNearest:
    """scipy.ndimage with maximum_filter(..., mode='nearest'), every other attribute untouched."""

    def __init__(self, ndi):
        self._ndi = ndi

    def __getattr__(self, name):
        return getattr(self._ndi, name)

    def maximum_filter(self, *a, **kw):
        kw["mode"] = "nearest"
        return self._ndi.maximum_filter(*a, **kw)


@contextlib.contextmanager
def nearest_border():
    saved = _pk.ndi
    _pk.ndi = _NdiNearest(saved)
    try:
        yield
    finally:
        _pk.ndi = saved
