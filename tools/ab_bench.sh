#!/bin/bash
# A/B of a library variant (tools/build_variant.sh) on the bench's headline
# step and kernel timers: the in-tree build, then _lib/var/libo3dx_$1.so.
# Usage: [OUT=dir] bash tools/ab_bench.sh NAME[,NAME...] [bench args...]
set -o pipefail
cd "${GRAFT_REPO_ROOT:-.}"
export TMPDIR=/tmp
V=$1; shift
export OUT=${OUT:-bench_out}
mkdir -p "$OUT"
for lib in base ${V//,/ }; do
  if [ "$lib" = base ]; then unset O3DX_LIB; else export O3DX_LIB=$PWD/open3d-py-extension_amd/open3dpypro/_lib/var/libo3dx_$lib.so; fi
  timeout -k 10 300 python bench.py --full --no-cpu "$@" > "$OUT/ab_$lib.json" 2> "$OUT/ab_$lib.err" || exit 1
  python - "$lib" <<'PY'
import json, os, sys
d = json.loads(open(os.path.join(os.environ["OUT"], f"ab_{sys.argv[1]}.json")).read().strip().splitlines()[-1])
e = d["extra"]
print(sys.argv[1], "ms", d["ms_per_step"], "kernels", {k: v["avg_ms"] for k, v in e["kernels"].items()},
      "raw_c3", (e.get("normals_raw_c3") or {}).get("ms"), "icp", (e.get("icp") or {}).get("iters_per_s"))
PY
done
