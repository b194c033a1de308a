"""The routes of fm_end (the synchronising half of every search call) against a record taken before it was split into
stages: tools/fm_end_routes.py makes three dozen small calls on one context per dtype - candidates verified on the host,
the device's hash verification, every step of the overflow ladder the shapes reach (maps, three products, map scan, float64
kernel, grown lists), the back-off routes of the calls that follow, the global extremum with and without the fused route,
a 1-D map next to 2-D ones, the NMS entry - and tests/golden/fm_end_routes.json holds what each call reported and returned
(`python tools/fm_end_routes.py --record ...` on the commit whose behaviour is the record).  Not reached by these shapes:
leaving the flagged segments for the full scan (more than 256 peaks in one strip:
test_gpu_parity.py::test_sparse_maps_route_equals_the_full_maps_route), a bound too wide for the map scan (low-contrast
windows beside a brightness step: test_gpu_parity.py::test_float32_adversarial_lists_equal_the_float64_kernels with the
maps in memory) and the device's share of the suppression (test_gpu_parity.py::test_fused_nms_call_equals_find_then_nms)."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.gpu
def test_fm_end_routes_replay_the_record():
    spec = importlib.util.spec_from_file_location("fm_end_routes", os.path.join(ROOT, "tools", "fm_end_routes.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(ROOT, "tests", "golden", "fm_end_routes.json")) as f:
        want = json.load(f)
    if any(os.environ.get(v) for v in ("MTM_KERNEL", "MTM_HITS_ONLY", "MTM_SPARSE_MAPS", "MTM_F32_MFMA", "MTM_FUSE_PEAKS",
                                       "MTM_CAND_PINNED", "MTM_PEAK_BORDER")):
        pytest.skip("a route switch is set: the record is of the default routes")
    got = tool.run()
    assert [(r["ctx"], r["name"]) for r in got] == [(r["ctx"], r["name"]) for r in want]
    for g, w in zip(got, want):
        for field in sorted(set(g) | set(w)):
            assert g.get(field) == w.get(field), (w["ctx"], w["name"], field, g.get(field), w.get(field))
