"""The two-row MFMA kernel's tail screen restated in numpy (ncc_mfma_kernel, tail_consts_kernel, stats_u8_kernel's tail
boxes): after s K steps the wave's first row holds template rows 0 .. s - 1, its second 0 .. s - 2, as the biased int8
accumulator.  The bound acc_P + K_P + m S1 + (tau_Q - 128) S1_Q + sqrt(V_Q) g_Q must never be below the exact numerator
of TM_CCOEFF_NORMED / TM_CCORR_NORMED - on random, smooth and adversarial windows, for both row parities."""
import numpy as np
import pytest


def _bound_and_num(I, T, q0, method):
    h, w = T.shape
    I = I.astype(np.int64)
    T = T.astype(np.int64)
    P, Q = slice(0, q0), slice(q0, h)
    acc = int(((I[P] - 128) * (T[P] - 128)).sum())                     # the biased accumulator after rows 0 .. q0 - 1
    nq, npp, n = (h - q0) * w, q0 * w, h * w
    kp = 128.0 * T[P].sum() - 16384.0 * npp
    d = T[Q].sum() / nq - 128.0
    g = np.sqrt((nq * (T[Q] ** 2).sum() - T[Q].sum() ** 2) / nq) * (1.0 + 2.0 ** -49)
    mag = 2.0 ** 32 + abs(kp) + 2.0 * 128 * 255 * n + g * 128 * np.sqrt(nq)
    kp_slack = kp + mag * 2.0 ** -46
    s1 = float(I.sum())
    s1q, s2q = int(I[Q].sum()), int((I[Q] ** 2).sum())
    vq = np.sqrt((nq * s2q - s1q * s1q) * (1.0 / nq)) * (1.0 + 2.0 ** -49)     # V' = |Q| V_Q exact, as the kernel
    m = 128.0 - T.sum() / n if method == 5 else 128.0
    bound = acc + kp_slack + m * s1 + d * s1q + vq * g
    corr = int((I * T).sum())
    num = corr - s1 * T.sum() / n if method == 5 else float(corr)
    return bound, num


def _cases(rng, h, w):
    yield rng.integers(0, 256, (h, w)), rng.integers(0, 256, (h, w))                         # noise
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.clip(128 + 100 * np.sin(yy / 7.0) * np.cos(xx / 5.0), 0, 255).astype(np.int64)
    yield smooth, smooth                                                                      # exact copy (score 1)
    yield smooth, 255 - smooth                                                                # anti-correlated
    t = rng.integers(0, 256, (h, w))
    t[: h // 2] = 128                                                                         # structure in the tail only
    i = t.copy()
    yield i, t
    yield np.full((h, w), 255), rng.integers(0, 256, (h, w))                                  # flat window
    yield rng.integers(254, 256, (h, w)), rng.integers(0, 2, (h, w)) * 255                    # near-flat vs binary
    yield rng.integers(0, 256, (h, w)), np.full((h, w), 77)                                   # constant template


@pytest.mark.parametrize("h,w,split", [(64, 64, 42), (64, 40, 42), (32, 64, 24), (20, 24, 12), (8, 16, 6)])
@pytest.mark.parametrize("method", [5, 3])
def test_tail_bound_is_an_upper_bound(h, w, split, method):
    rng = np.random.default_rng(h * 1000 + w + split + method)
    n_case = 0
    for I, T in _cases(rng, h, w):
        for q0 in (split, split - 1):                     # the wave's first row, its second
            bound, num = _bound_and_num(I, T, q0, method)
            assert bound >= num, (h, w, q0, method, bound, num)
            n_case += 1
    for _ in range(40):                                   # random templates against windows made from them
        T = rng.integers(0, 256, (h, w))
        I = np.clip(T + rng.integers(-40, 41, (h, w)), 0, 255)
        for q0 in (split, split - 1):
            bound, num = _bound_and_num(I, T, q0, method)
            assert bound >= num
            n_case += 1
    assert n_case > 80


def test_tail_bound_rules_out_noise():
    """On noise against noise the bound at the headline's split stays far below the 0.5 threshold's right-hand side for
    almost every window: what the screen is for."""
    rng = np.random.default_rng(5)
    h = w = 64
    T = rng.integers(0, 256, (h, w))
    tn = np.sqrt(((T - T.mean()) ** 2).sum())
    below = 0
    for _ in range(50):
        I = rng.integers(0, 256, (h, w))
        sq = np.sqrt(((I - I.mean()) ** 2).sum())
        bound, num = _bound_and_num(I, T, 41, 5)
        below += bound < 0.5 * (1 - 2e-6) * tn * sq
    assert below >= 48
