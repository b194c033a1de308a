"""Differential fuzz of the host layer on the MI355X: every case of tests/golden/hostfuzz.json.gz (outcomes of the
unmodified reference, tests/golden/make_hostfuzz.py) replayed through the HIP kernels with the rules of
tests/hostfuzz_replay.py - the shipped default context ("nearest" border, "@nearest" outcomes), then the same context with
MTM_OPT_PEAK_BORDER = constant ("@constant" outcomes), then through TemplateMatcher and (a subset) through
MTM.distributed.matchTemplates_sharded.  Fixture only: the reference is never imported.

matchTemplates compares in order (only hits of one run of tied scores - equal scores for 8-bit - may swap places: the
reference orders them by an unstable sort), 8-bit scores to 1e-6; the uint8 epilogue is documented as bit-identical to the
oracle."""
import collections
import os

import pytest

import hostfuzz_replay as R

pytestmark = pytest.mark.gpu

FIX = R.load_fixture()["cases"]
IDS = sorted(FIX)
MATCH_IDS = [c for c in IDS if FIX[c]["kind"] == "match"]
SHARDED_IDS = MATCH_IDS[::max(1, len(MATCH_IDS) // 40)][:40]
ROUTES = collections.Counter()          # (kernel_used, f32_route) after every search of the default-context replays


@pytest.fixture(scope="module")
def mtm():
    import build as mtm_build
    mtm_build.build()
    import MTM
    return MTM


def _replay(mtm, border, ids, via="direct"):
    ctx = mtm._lib.default_context()
    mtm._list_memo = None

    def on_step(kind, got):
        if kind in ("find", "match") and got["kind"] == "hits":
            t = ctx.timing()
            ROUTES[(t["kernel_used"], t["f32_route"])] += 1
    fails = []
    for cid in ids:
        fails += R.replay_case(mtm, FIX[cid], border, via=via, ctx=ctx, on_step=on_step if via == "direct" else None)
    assert not fails, "%d of %d cases differ from the reference:\n%s" % (len(fails), len(ids), "\n".join(fails[:25]))


def test_replay_default_context(mtm):
    ctx = mtm._lib.default_context()
    assert ctx.get_option(mtm._lib.OPT_PEAK_BORDER) == 1            # the shipped default: "nearest"
    _replay(mtm, "nearest", IDS)


def test_replay_constant_border(mtm):
    ctx = mtm._lib.default_context()
    saved = ctx.get_option(mtm._lib.OPT_PEAK_BORDER)
    ctx.set_option(mtm._lib.OPT_PEAK_BORDER, 0)
    try:
        _replay(mtm, "constant", IDS)
    finally:
        ctx.set_option(mtm._lib.OPT_PEAK_BORDER, saved)


def test_replay_template_matcher(mtm):
    _replay(mtm, "nearest", MATCH_IDS, via="matcher")


def test_replay_sharded_world_size_one(mtm):
    _replay(mtm, "nearest", SHARDED_IDS, via="sharded")


def test_replay_took_every_route(mtm):
    """The replays above ran the int8 matrix-core kernel (kernel_used 3), the float64 kernel for float32 images
    (kernel_used 0: the exact route, e.g. lists mixing masked and unmasked float32 templates) and the bf16 screen with
    exact re-scoring (f32_route 1, 2 or 4)."""
    if not ROUTES:
        _replay(mtm, "nearest", IDS)
    print("hostfuzz: %d cases, routes (kernel_used, f32_route): %s" % (len(IDS), dict(sorted(ROUTES.items()))))
    if os.environ.get("MTM_KERNEL") or os.environ.get("MTM_F32_MFMA"):
        pytest.skip("a route is forced by MTM_KERNEL / MTM_F32_MFMA")
    k = {r[0] for r in ROUTES}
    f = {r[1] for r in ROUTES}
    assert 3 in k and 0 in k and f & {1, 2, 4}, dict(ROUTES)
