#!/bin/bash
# Quick GPU iteration: the GPU tests matching $1 (pytest -k), then the bench.
# Usage: [OUT=dir] bash tools/gpu_quick.sh "icp" [bench args...]
set -o pipefail
cd "${GRAFT_REPO_ROOT:-.}"
export TMPDIR=/tmp
K="$1"; shift
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread -k "$K" > "$OUT/quick_tests.log" 2>&1
rc=$?
tail -3 "$OUT/quick_tests.log"
[ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python bench.py --full --no-cpu "$@" > "$OUT/quick_bench.json" 2> "$OUT/quick_bench.err"
