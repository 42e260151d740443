#!/bin/bash
set -u -o pipefail
mkdir -p bench_out
timeout -k 10 300 python -m pytest tests/test_gpu_tar_required_skip_kernel.py tests/test_gpu_tar_required_skip.py tests/test_gpu_tar_required.py -q -p no:cacheprovider 2>&1 | tail -4 &&
timeout -k 10 300 python profiles/device_required_skip/job_dirs.py bench_out/index_dirs.jsonl &&
for i in 1 2 3; do
  TSG_LIB=$PWD/trivy_amd/_variants/parent/libtsg.so timeout -k 10 200 python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs bench_out/dump_parent_$i 2>/dev/null | tail -1 > bench_out/c2_bench_parent_$i.json || exit 1
  timeout -k 10 200 python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs bench_out/dump_new_$i 2>/dev/null | tail -1 > bench_out/c2_bench_new_$i.json || exit 1
done
(cd bench_out && sha256sum dump_*/findings.npy dump_*/findings_count.npy) | tee bench_out/dump_sha256.txt
python -c "
import json,glob
for f in sorted(glob.glob('bench_out/c2_bench_*.json')): print(f, json.load(open(f))['value'])"
