#!/bin/bash
# GPU parity suite under every alternative compute route of the library (GPU box).  Round 6: 20 MTM_* variables are left in
# the native code (39 in round 5); the ones that select a route are all here, the rest is tuning / diagnostics
# (MTM_CLASS_LANES, MTM_UPLOAD_BANDS, MTM_BAND_MIN_FILL, MTM_GROUP_SPIN_US, MTM_COMM_TIMEOUT_S, MTM_HOST_TRACE).
# Known, not among the default modes: MTM_TAIL_SPLIT=<s> (the tail screen's split forced, e.g. ALT_MODES="MTM_TAIL_SPLIT=37";
# any split gives the same records - tests/test_gpu_tail_split.py covers every residue of the K loop's rotation).
# Exit status: 0 if every switch passed, 1 if some had failures; a run that timed out or died of a signal (abort,
# segmentation fault, kill: 124, 134, 137, 139, ...) ends the script at once with its status - nothing more is started on
# a GPU that may be in a bad state.
DEFAULT_MODES="X=0 MTM_FUSE_LAYOUT=0 MTM_CAND_PINNED=0 MTM_SEG_SKIP=0 MTM_ROW_MUX=0 MTM_HITS_ONLY=0 MTM_EXACT_DIV=0 MTM_EXACT_DIV=2 MTM_FUSE_STATS=0 MTM_KERNEL=dot4 MTM_MFMA_R2=0 MTM_SCREEN_L1=0 MTM_TAIL_SCREEN=0 MTM_F32_MFMA=2 MTM_F32_MFMA=3 MTM_F32_MFMA=0 MTM_TEMPL_ON_DEVICE=0 MTM_UPLOAD_BANDS=1 MTM_CLASS_LANES=1 MTM_CLASS_LANES=4 MTM_BAND_MIN_FILL=0 MTM_MASKSQ_FUSED=0 MTM_SPARSE_MAPS=0 MTM_NMS_DEVICE_MIN=-1"
status=0
# ALT_MODES: a subset of the switches (space separated) instead of all of them
for e in ${ALT_MODES:-$DEFAULT_MODES}; do
  # ALT_K: optional pytest -k expression for a quick pass (e.g. ALT_K="not cfg" tools/alt_modes.sh)
  echo "== $e"
  env $e timeout -k 10 900 python -m pytest tests -m gpu -q ${ALT_K:+-k "$ALT_K"} 2>&1 | grep -E "passed|failed|error" | tail -2
  rc=${PIPESTATUS[0]}
  if [ "$rc" -eq 124 ] || [ "$rc" -gt 128 ]; then
    echo "== stopped: $e exited with status $rc"
    exit "$rc"
  fi
  [ "$rc" -ne 0 ] && status=1
done
exit $status
