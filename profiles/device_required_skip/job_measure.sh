#!/bin/bash
# the index and the whole step with skip options, the switch off and on interleaved in one job
set -u -o pipefail
mkdir -p bench_out
SK='--skip-dirs **/node_modules,usr/share/doc --skip-files **/*.pem --required-skip both --steps 20 --warmup 5'
timeout -k 10 420 python tools/device_only_bench.py --layer --walk gpu --required gpu --index-only $SK --out bench_out/index_ustar.jsonl > /dev/null 2> bench_out/index_ustar.err &&
timeout -k 10 420 python tools/device_only_bench.py --layers 5 --layer-gb 5 --required gpu --index-only $SK --out bench_out/index_c4x5.jsonl > /dev/null 2> bench_out/index_c4x5.err &&
timeout -k 10 600 python tools/device_only_bench.py --layer --walk gpu --required gpu $SK --out bench_out/step_ustar.jsonl > /dev/null 2> bench_out/step_ustar.err
echo "rc $?"
python - <<'PY'
import json, glob
for f in sorted(glob.glob("bench_out/*_ustar.jsonl") + glob.glob("bench_out/index_c4x5.jsonl")):
    for line in open(f):
        d = json.loads(line)
        print(f, d["mode"], "ms %.1f (%.1f-%.1f)" % (d["ms_per_step"], d["min_ms"], d["max_ms"]), "cpus %.1f" % d["host_cpus"],
              d.get("skip"), {k: d["index"][k] for k in ("ms_total", "ms_total_min", "ms_total_max", "files")} if "index" in d else "",
              d.get("required_skip"), {k: v for k, v in (d.get("required") or {}).items() if k.startswith(("ms_", "skip", "under", "reason", "on_gpu"))},
              d.get("findings"))
PY
