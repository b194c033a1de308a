#!/usr/bin/env python3
"""The tail screen's leave-or-stay decisions per wave, counted by the MFMA instruction counter and held to the model.

SQ_INSTS_MFMA of a score launch is exact and repeatable (profiles/tail_split/mfma_counts.txt): a wave of the two-row int8
kernel issues c = 32 MFMAs per K step, h + 1 steps if it stays, `split` steps if the tail screen sends it away.  So

    MTM_TAIL_SCREEN=0:  N_full = c W (h + 1)                 W = waves of the launch
    screened:           N      = N_full - c L (h + 1 - split)   L = waves that left

and L follows from two counter values.  tests/tail_model.py predicts W and L per scene (wave_pass) from exact integers.

  --predict            no GPU: the model's split, W and L per scene and threshold (tail_model.COUNTER_SCENES)
  --run [--out DIR]    one search per scene, threshold and context - screened, then MTM_TAIL_SCREEN=0 - one score launch per
                       call (MTM_UPLOAD_BANDS=1), contexts created the way tests/test_gpu_tail_split.py creates them; prints
                       class_tilings() for each call and writes the call list to DIR/calls.json.  Run it under the counter:
                         rocprofv3 --pmc SQ_INSTS_MFMA --output-format csv -d DIR -o counts -- python tools/tail_wave_count.py --run --out DIR
  --counts CSV [--calls DIR/calls.json]
                       no GPU: the ncc_mfma_kernel dispatches of the counter file, in dispatch order, against the call list:
                       N_full, N, L from the counter and L from the model per scene; exit status 1 on a mismatch.
"""
import csv
import glob
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (os.path.join(ROOT, "multitemplatematching-python_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

MFMA_PER_WAVE_STEP = 32         # 16 column phases x 2 output rows


def _lib():
    import build as mtm_build
    mtm_build.build()
    from MTM import _lib
    return _lib


def _cases(M):
    return [(cell, thr) for cell in M.COUNTER_SCENES for thr in M.COUNTER_THRESHOLDS]


def predict():
    import tail_model as M
    lib = _lib()
    for cell, thr in _cases(M):
        p = M.predict(lib, cell, thr)
        n_full = MFMA_PER_WAVE_STEP * p["waves"] * (cell["h"] + 1)
        n = n_full - MFMA_PER_WAVE_STEP * p["leaving"] * (cell["h"] + 1 - p["split"]) if p["split"] else n_full
        print("%-22s method %d thr %.1f split %2d  W %3d  L %3d  (SQ_INSTS_MFMA %d unscreened, %d screened)" % (
            cell["name"], cell["method"], thr, p["split"], p["waves"], p["leaving"], n_full, n))
    return 0


def _context(lib, **env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c = lib.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    c.set_option(lib.OPT_HITS_ONLY, 1)
    return c


def run(out_dir):
    import tail_model as M
    os.environ["MTM_UPLOAD_BANDS"] = "1"
    lib = _lib()
    calls = []
    for cell, thr in _cases(M):
        img, templates, _ = M.scene(cell)
        tl = [(t, None) for t in templates]
        p = M.predict(lib, cell, thr)
        env = {"MTM_TAIL_SPLIT": str(cell["force_split"])} if cell.get("force_split") else {}
        records = {}
        for screened, ctx in ((True, _context(lib, **env)), (False, _context(lib, MTM_TAIL_SCREEN="0"))):
            try:
                hits = ctx.search(tl, img, cell["method"], lib.PEAKS_LOCAL, thr)
                records[screened] = hits.tobytes()
                tilings = ctx.class_tilings()
                launches = int(ctx.timing()["ncc_launches"])
            finally:
                ctx.close()
            print("%-22s thr %.1f %-10s hits %4d ncc_launches %d class_tilings %s" % (
                cell["name"], thr, "screened" if screened else "unscreened", len(hits), launches, tilings), flush=True)
            calls.append({"scene": cell["name"], "thr": thr, "screened": screened, "h": cell["h"], "launches": launches,
                          "split": int(tilings[0]["tail_split"]), "n_hits": int(len(hits)), "model_split": int(p["split"]),
                          "model_waves": int(p["waves"]), "model_leaving": int(p["leaving"])})
        assert records[True] == records[False], (cell["name"], thr, "the screened records differ from the unscreened ones")
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "calls.json"), "w") as f:
            json.dump(calls, f, indent=1)
    return 0


def _dispatches(path):
    """[(dispatch id, value)] of SQ_INSTS_MFMA over the ncc_mfma_kernel dispatches of a rocprofv3 counter csv, in dispatch
    order (a dispatch's rows - one per counter dimension, where the tool splits them - are summed)."""
    if os.path.isdir(path):
        found = sorted(glob.glob(os.path.join(path, "**", "*counter_collection.csv"), recursive=True))
        assert found, "no *counter_collection.csv under " + path
        path = found[-1]
    per = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if row["Counter_Name"] != "SQ_INSTS_MFMA" or "ncc_mfma_kernel" not in row["Kernel_Name"]:
                continue
            k = int(row["Dispatch_Id"])
            per[k] = per.get(k, 0.0) + float(row["Counter_Value"])
    return sorted(per.items())


def counts(csv_path, calls_path):
    with open(calls_path) as f:
        calls = json.load(f)
    disp = _dispatches(csv_path)
    need = sum(c["launches"] for c in calls)
    print("# %d ncc_mfma_kernel dispatches with SQ_INSTS_MFMA, %d score launches in the call list" % (len(disp), need))
    if len(disp) != need or any(c["launches"] != 1 for c in calls):
        print("# the dispatches do not pair with the calls one to one: nothing derived")
        return 1
    bad = 0
    by = {}
    for c, (did, value) in zip(calls, disp):
        by[(c["scene"], c["thr"], c["screened"])] = (c, did, int(round(value)))
    for (scene, thr, screened), (c, did, n) in sorted(by.items()):
        if not screened:
            continue
        cu, did_u, n_full = by[(scene, thr, False)]
        h, split, waves = c["h"], c["split"], c["model_waves"]
        full_ok = n_full == MFMA_PER_WAVE_STEP * waves * (h + 1)
        line = "%-22s thr %.1f  N_full %8d (dispatch %d; 32 W (h + 1) with W = %d: %s)  N %8d (dispatch %d) split %2d" % (
            scene, thr, n_full, did_u, waves, "yes" if full_ok else "NO", n, did, split)
        if split != c["model_split"]:
            line += "  SPLIT differs from the model's %d" % c["model_split"]
            bad += 1
        elif split == 0:
            left, ok = 0, n == n_full
            line += "  unscreened: N == N_full %s" % ("yes" if ok else "NO")
            bad += 0 if ok and c["model_leaving"] == 0 else 1
        else:
            per_wave = MFMA_PER_WAVE_STEP * (h + 1 - split)
            left, rem = divmod(n_full - n, per_wave)
            ok = rem == 0 and left == c["model_leaving"]
            line += "  L counter %3d%s  L model %3d  %s" % (left, "" if rem == 0 else " (+ %d MFMAs over)" % rem,
                                                        c["model_leaving"], "match" if ok else "MISMATCH")
            bad += 0 if ok else 1
        bad += 0 if full_ok else 1
        print(line)
    print("# %d scenes x thresholds, %d do not match" % (sum(1 for k in by if k[2]), bad))
    return 1 if bad else 0


def main(argv):
    def opt(name, default=None):
        return argv[argv.index(name) + 1] if name in argv else default
    if "--predict" in argv:
        return predict()
    if "--run" in argv:
        return run(opt("--out"))
    if "--counts" in argv:
        src = opt("--counts")
        return counts(src, opt("--calls", os.path.join(src if os.path.isdir(src) else os.path.dirname(src), "calls.json")))
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv))
