"""The tail screen's split as a function of the call's threshold (tail_split_rule in mtm_host.cpp, exported as
mtm_debug_tail_split): the smallest s in [6, h - 2] with thr - (h - s + 1) / h >= z sqrt(s / h) / sqrt(w h), 0 where none
exists or where s / h is above the fraction beyond which a screened call no longer beats an unscreened one - restated in
numpy on a grid; the bound of test_tail_bound_cpu.py at EVERY split the kernel can now be given, both row parities; and
the screen still rules out noise at the split the rule picks for the headline."""
import ctypes

import numpy as np
import pytest

from test_tail_bound_cpu import _bound_and_num, _cases

# the measured constants of tail_split_rule (kTailSplitZ, kTailSplitMaxFrac; DESIGN 4.1 "Tail screen")
Z = 6.5
MAX_FRAC = 0.94


@pytest.fixture(scope="module")
def rule():
    import build as mtm_build   # multitemplatematching-python_amd/build.py
    so = ctypes.CDLL(mtm_build.build())
    fn = so.mtm_debug_tail_split
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_double]
    return fn


def _rule_np(h, w, thr):
    if not thr >= 0.0:
        return 0
    for s in range(6, h - 1):
        if thr - (h - s + 1) / h >= Z * np.sqrt(s / h) / np.sqrt(float(w * h)):
            return s if s / h <= MAX_FRAC else 0
    return 0


def test_rule_equals_its_restatement_on_a_grid(rule):
    n_on = 0
    for h in (8, 20, 32, 48, 64):
        for w in (16, 24, 40, 64):
            prev = None
            for k in range(5, 100):
                thr = k / 100.0
                s = rule(h, w, thr)
                assert s == _rule_np(h, w, thr), (h, w, thr, s, _rule_np(h, w, thr))
                assert s == 0 or 6 <= s <= h - 2, (h, w, thr, s)
                if s and prev:
                    assert s <= prev, (h, w, thr, s, prev)       # non-increasing in thr wherever it is non-zero
                if prev:
                    assert s, (h, w, thr)                        # (and once a split exists, every higher threshold has one)
                prev = s or prev
                n_on += s > 0
            for thr in (-1e-9, -0.3, -1.0, float("nan")):
                assert rule(h, w, thr) == 0
    assert n_on > 500
    # the headline's class, and the reference's other usual threshold
    assert 36 <= rule(64, 64, 0.5 - 1e-6) <= 42
    assert 22 <= rule(64, 64, 0.7 - 1e-6) <= 28


@pytest.mark.parametrize("h,w", [(64, 64), (32, 64), (20, 24)])
@pytest.mark.parametrize("method", [5, 3])
def test_tail_bound_is_an_upper_bound_at_every_split(h, w, method):
    rng = np.random.default_rng(h * 1000 + w + method)
    cases = list(_cases(rng, h, w))
    for _ in range(6):                                    # random templates against windows made from them
        T = rng.integers(0, 256, (h, w))
        cases.append((np.clip(T + rng.integers(-40, 41, (h, w)), 0, 255), T))
    n_case = 0
    for split in range(6, h - 1):
        for I, T in cases:
            for q0 in (split, split - 1):                 # the wave's first row, its second
                bound, num = _bound_and_num(I, T, q0, method)
                assert bound >= num, (h, w, q0, method, bound, num)
                n_case += 1
    assert n_case == (h - 7) * len(cases) * 2


def test_tail_bound_rules_out_noise_at_the_rules_split(rule):
    """test_tail_bound_cpu.py's seeded noise, 64 x 64, threshold 0.5: the per-window bound stays below the right-hand side
    for at least 48 of 50 windows at the rule's split (the wave's first row) and one row earlier (its second)."""
    h = w = 64
    s = rule(h, w, 0.5 * (1 - 1e-6))
    assert 6 <= s <= h - 2
    for q0 in (s, s - 1):
        rng = np.random.default_rng(5)
        T = rng.integers(0, 256, (h, w))
        tn = np.sqrt(((T - T.mean()) ** 2).sum())
        below = 0
        for _ in range(50):
            I = rng.integers(0, 256, (h, w))
            sq = np.sqrt(((I - I.mean()) ** 2).sum())
            bound, num = _bound_and_num(I, T, q0, 5)
            below += bound < 0.5 * (1 - 2e-6) * tn * sq
        assert below >= 48, (s, q0, below)
