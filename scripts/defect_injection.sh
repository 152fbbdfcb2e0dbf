#!/bin/bash
# Prove that the gradient tests bite: build a lab copy of the library with a defect injected (scripts/lab_build.sh, selected by
# CIRKIT_HIP_LIB) and run the tests that must see it: they must FAIL.  Exit 0 when every defect was caught.
#   bash scripts/defect_injection.sh [defect]   VERDICT r5 #8: a sum job's epilogue scales <W, dW> by (1 + defect) (default 1e-3);
#                                               the job-form gradient tests (tests/test_training_jobs.py) and the sum job's
#                                               kernel test (tests/test_gpu_jobs.py -k sum64_bwd): both runs must fail
#   bash scripts/defect_injection.sh layer      the layer backward kernels (CK_BWD_LAB_DEFECT of cirkit_amd/csrc/ck_backward.hip)
#                                               against tests/test_gpu_layer_backward.py: 1 the tile32 kernel treats the rows beyond B
#                                               of a ragged tile as live, 2 it stops after a wave's first tile, 3 the register
#                                               mixing kernel scales dmw by 1 + 1e-3
# The lab libraries need the objects of a finished build under cirkit_amd/lib/; LAYER_LABS=keep (layer) / JOBS_LAB=keep (default
# path) runs libraries that are already under build/lab/ (built where the objects are).
set -u
cd "$(dirname "$0")/.."
if [ "${1:-}" = "layer" ]; then
  missed=0
  for d in 1 2 3; do
    if [ "${LAYER_LABS:-}" != "keep" ]; then
      bash scripts/lab_build.sh bwd_defect$d cirkit_amd/csrc/ck_backward.hip -DCK_BWD_LAB_DEFECT=$d > /dev/null || exit 2
    fi
    case $d in
      1) what="tile32: rows beyond B live"; pick="test_sum_tile or test_sum_value_families" ;;
      2) what="tile32: tiles after a wave's first skipped"; pick="test_sum_tile_many_folds" ;;
      3) what="mixing register kernel: dmw scaled by 1 + 1e-3"; pick="test_mixing_register_kernels or test_mixing_many_folds" ;;
    esac
    CIRKIT_HIP_LIB=$PWD/build/lab/lib_bwd_defect$d.so timeout -k 10 600 python -m pytest tests/test_gpu_layer_backward.py -q -m gpu -x -k "$pick" \
      -p no:cacheprovider > build/lab/bwd_defect$d.log 2>&1
    rc=$?
    grep -E "^E  .*(assert|Error)" build/lab/bwd_defect$d.log | head -3 | cut -c1-220
    tail -1 build/lab/bwd_defect$d.log
    if [ $rc -eq 1 ]; then echo "layer defect $d ($what): CAUGHT"; else echo "layer defect $d ($what): NOT caught (pytest rc $rc)"; missed=1; fi
    if [ $rc -gt 1 ]; then exit 2; fi  # (not a test failure: nothing more is started)
  done
  exit $missed
fi
DEFECT=${1:-1e-3f}
if [ "${JOBS_LAB:-}" != "keep" ]; then
  bash scripts/lab_build.sh defect cirkit_amd/csrc/ck_jobs.hip -DCK_JOBS_LAB_DEFECT=$DEFECT > /dev/null || exit 2
fi
missed=0
run_must_fail() {  # <log name> <what> <pytest arguments...>
  local log=build/lab/$1.log what=$2
  shift 2
  CIRKIT_HIP_LIB=$PWD/build/lab/lib_defect.so timeout -k 10 600 python -m pytest "$@" -q -m gpu -x -p no:cacheprovider > "$log" 2>&1
  local rc=$?
  grep -E "^E  .*(assert|Error)" "$log" | head -6 | cut -c1-220
  tail -3 "$log"
  if [ $rc -eq 1 ]; then echo "defect $DEFECT in <W, dW>, $what: CAUGHT"; else echo "defect $DEFECT in <W, dW>, $what: NOT caught (pytest rc $rc)"; missed=1; fi
  if [ $rc -gt 1 ]; then exit 2; fi  # (not a test failure: nothing more is started)
}
run_must_fail defect "circuit-level tests" tests/test_training_jobs.py -k "shallow_circuit or gradients_match_the_layerwise"
run_must_fail defect_kernel "kernel test" tests/test_gpu_jobs.py -k sum64_bwd
exit $missed
