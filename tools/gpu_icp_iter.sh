export TMPDIR=/tmp; OUT=${OUT:-bench_out}; mkdir -p "$OUT"
timeout -k 10 500 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread -k "icp or registration" > "$OUT/q_tests.log" 2>&1; rc=$?; tail -3 "$OUT/q_tests.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 200 rocprofv3 --kernel-trace -d "$OUT/prof_icp" -o run --output-format csv -- python tools/prof_kernels.py icp_loop > "$OUT/picp.log" 2>&1 || exit 1
timeout -k 10 300 python bench.py --full --no-cpu > "$OUT/qb.json" 2>"$OUT/qb.err"; grep -o "\"icp\": {[^}]*}" "$OUT/qb.json"; grep -o "\"icp_30\": [0-9.]*" "$OUT/qb.json"
