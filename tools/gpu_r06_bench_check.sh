#!/bin/bash
set -o pipefail
cd "${GRAFT_REPO_ROOT:-.}"
export TMPDIR=/tmp
export OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 600 python bench.py --full > "$OUT/r06_bench_check.json" 2> "$OUT/r06_bench_check.err" || { tail -20 "$OUT/r06_bench_check.err"; exit 1; }
python -c "import json,os;d=json.loads(open(os.path.join(os.environ['OUT'],'r06_bench_check.json')).read().strip().splitlines()[-1]);print(d['value'],d['ms_per_step'],d['scaling'],d['roofline']['frac'],d['cpu_baseline']['value'])"
