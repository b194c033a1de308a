"""Differential fuzz of the host layer on CPU: every case of tests/golden/hostfuzz.json.gz (outcomes of the unmodified
reference, see tests/golden/make_hostfuzz.py) replayed through MTM with the oracle standing in for the kernels - under both
border rules, through the two-step engine and the fused search + NMS engine, through TemplateMatcher and (a subset)
through MTM.distributed.matchTemplates_sharded.  Rules: tests/hostfuzz_replay.py.

Bugs this fixture found (fixed in the same change):
- A030, A031, A033, A042, A043: ("label", template, None) raised AttributeError on the 8-bit path (methods 0 and 3); the
  reference's TemplateTuple allows a None mask.
- A000 (N_object=-3), A002 (N_object=-1) on the fused engine: a finite negative N_object reached search_nms, which reads
  every negative value as "no limit", instead of cutting the kept list with indexes[:N_object].
"""
import numpy as np
import pytest

import hostfuzz_cases as HC
import hostfuzz_replay as R
from helpers import FusedContext, OracleContext

FIX = R.load_fixture()["cases"]
IDS = sorted(FIX)
MATCH_IDS = [c for c in IDS if FIX[c]["kind"] == "match"]
SHARDED_IDS = MATCH_IDS[::max(1, len(MATCH_IDS) // 40)][:40]


@pytest.fixture(scope="module")
def mtm():
    import build as mtm_build
    mtm_build.build()
    import MTM
    return MTM


def _replay(mtm, monkeypatch, engine, border, ids, via="direct"):
    ctx = engine(mtm._lib.HIT_DTYPE, border=border)
    monkeypatch.setattr(mtm._lib, "_default_ctx", ctx)
    monkeypatch.setattr(mtm, "_list_memo", None)
    fails = []
    for cid in ids:
        fails += R.replay_case(mtm, FIX[cid], border, via=via, ctx=ctx)
    assert not fails, "%d of %d cases differ from the reference:\n%s" % (len(fails), len(ids), "\n".join(fails[:25]))
    return ctx


def test_fixture_covers_the_strata():
    counts = {s: sum(1 for c in FIX.values() if c["stratum"] == s) for s in HC.STRATA}
    assert len(FIX) >= 400 and counts["A"] >= 120 and counts["B"] >= 120 and counts["C"] >= 80 and counts["D"] >= 30 \
        and counts["F"] >= 60, counts
    assert sum(len(c["steps"]) for c in FIX.values() if c["kind"] == "seq") >= 20
    kinds = {c.get("@nearest", c.get("@any", {})).get("kind") for c in FIX.values()}
    assert {"hits", "error", "cv2_error"} <= kinds


@pytest.mark.parametrize("border", ["nearest", "constant"])
def test_replay_two_step_engine(mtm, monkeypatch, border):
    _replay(mtm, monkeypatch, OracleContext, border, IDS)


@pytest.mark.parametrize("border", ["nearest", "constant"])
def test_replay_fused_engine(mtm, monkeypatch, border):
    assert _replay(mtm, monkeypatch, FusedContext, border, IDS).calls


def test_negative_n_object_stays_off_the_fused_call(mtm, monkeypatch):
    """A000 (N_object=-3) and A002 (-1) take the two-step route - search_nms reads every negative value as "no limit";
    A004 (0) and A016 (inf) take the fused call, once each."""
    for cid, n_calls in (("A000", 0), ("A002", 0), ("A004", 1), ("A016", 1)):
        assert FIX[cid]["kind"] == "match"
        ctx = _replay(mtm, monkeypatch, FusedContext, "nearest", [cid])
        assert len(ctx.calls) == n_calls, (cid, ctx.calls)


def test_sharded_rccl_route_keeps_negative_n_object_off_the_fused_call(mtm, monkeypatch):
    """MTM.distributed.matchTemplates_sharded over an "rccl" exchange hands 8-bit calls to the context's fused native
    entry (search_sharded_nms, where n_object < 0 means no limit) - except for a finite negative N_object, which must cut
    the kept list like indexes[:N_object]: the step-by-step route.  The stand-in context is the oracle + mtm_nms."""
    from MTM.distributed import HitExchange, matchTemplates_sharded

    class RcclStub(OracleContext):
        def __init__(self, hit_dtype):
            super().__init__(hit_dtype)
            self.calls = []

        def search_sharded_nms(self, templates, image, method, thr, max_overlap, n_object, global_idx):
            self.calls.append(n_object)
            raw = self.search(templates, image, method, 0, thr).copy()
            raw["templ_idx"] = np.asarray(global_idx, dtype=np.int32)[raw["templ_idx"]]
            if len(raw) <= 1:
                return raw
            idx = mtm._lib.nms_hits(raw, thr, max_overlap, ascending=(method == 1))
            return raw[idx] if n_object < 0 else raw[idx][:n_object]

    monkeypatch.setattr(mtm._lib, "_default_ctx", OracleContext(mtm._lib.HIT_DTYPE))
    stub = RcclStub(mtm._lib.HIT_DTYPE)
    ex = HitExchange("rccl", 0, 1, context=stub)
    _, call, _ = HC.build_case("A000")
    lt, img = call["args"]
    lengths = {}
    for n in (-3, -1, 2, float("inf")):
        kw = dict(method=5, N_object=n, score_threshold=0.5, maxOverlap=0.25)
        got = matchTemplates_sharded(lt, img, ex, **kw)
        assert got == mtm.matchTemplates(lt, img, **kw), n
        lengths[n] = len(got)
    assert stub.calls == [2, -1]
    assert lengths[-1] == lengths[float("inf")] - 1 and lengths[-3] == lengths[float("inf")] - 3 and lengths[2] == 2, lengths


def test_replay_template_matcher(mtm, monkeypatch):
    _replay(mtm, monkeypatch, OracleContext, "nearest", MATCH_IDS, via="matcher")


def test_replay_sharded_world_size_one(mtm, monkeypatch):
    assert len(SHARDED_IDS) == 40
    _replay(mtm, monkeypatch, OracleContext, "nearest", SHARDED_IDS, via="sharded")


def test_u8_units_none_mask(mtm):
    """MTM.distributed._u8_units: a None mask is no mask (the sharded form of A030's bug)."""
    from MTM.distributed import _u8_units
    img = np.zeros((20, 20), np.uint8)
    t = np.ones((4, 5), np.uint8)
    m = np.full((4, 5), 255, np.uint8)
    for method in (0, 3):
        units = _u8_units([("a", t, None), ("b", t, m), ("c", t)], img, method)
        assert units is not None and [u[1] is None for u in units] == [True, False, True]
        assert units[0][0] is t
    assert _u8_units([("a", t, None)], img, 5) is None          # an ignored mask: the general route warns
    assert _u8_units([("a", t, m[:-1])], img, 3) is None
