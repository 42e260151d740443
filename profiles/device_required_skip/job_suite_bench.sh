#!/bin/bash
# the whole GPU suite, smoke(), then bench.py with the parent's library and this tree's, interleaved
set -u -o pipefail
mkdir -p bench_out
timeout -k 10 840 python -m pytest tests -m gpu -q -p no:cacheprovider 2>&1 | tee bench_out/gpu_suite.log | tail -6 &&
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tee bench_out/smoke.log | tail -3 &&
for i in 1 2 3; do
  TSG_LIB=$PWD/trivy_amd/_variants/parent/libtsg.so timeout -k 10 150 python bench.py --gpus 1 --steps 20 --warmup 5 2>/dev/null | tail -1 > bench_out/c2_bench_parent_$i.json || exit 1
  timeout -k 10 150 python bench.py --gpus 1 --steps 20 --warmup 5 2>/dev/null | tail -1 > bench_out/c2_bench_new_$i.json || exit 1
done
python - <<'PY'
import json, glob
for f in sorted(glob.glob("bench_out/c2_bench_*.json")):
    d = json.loads(open(f).read())
    print(f, {k: d[k] for k in d if k in ("value", "gbps", "throughput_gbps", "metric", "unit")} or list(d)[:8])
PY
