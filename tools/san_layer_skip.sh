#!/bin/bash
# LayerTar's skipDirs / skipFiles in the layer walks (tsg_analyzer_set_tar_skip) under ASan + UBSan, as a
# stand-alone program (tools/san_layer_skip.cpp: its own main, no interpreter, no GPU): the product's host
# C++ and the oracle hooks are compiled with the sanitizers and linked with the program; the gfx950 device
# objects are linked as built (nothing of them runs here).  The layers and what is expected of each are the
# tests' (tests/tar_skip_model.py), written to files first.
# Usage: bash tools/san_layer_skip.sh   (log -> profiles/layer_skip/san_layer_skip.log)
set -u -o pipefail
cd "$(dirname "$0")/.."
python -c "import __graft_entry__ as g; g.build()" || exit 1
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
COMMON="-O1 -g -march=x86-64-v3 -fPIC -std=c++17 -fno-omit-frame-pointer -I trivy_amd/csrc -I include -I oracle/native -D__HIP_PLATFORM_AMD__ -I ${ROCM_PATH:-/opt/rocm}/include"
out=oracle/build/san_layer_skip
mkdir -p $out/layers profiles/layer_skip
python - "$out/layers" <<'PY' || exit 1
import sys
from pathlib import Path
sys.path.insert(0, ".")
from oracle import analyzer as oan
from tests import tar_skip_model as sm
d = Path(sys.argv[1])
for f in list(d.glob("*.tar")) + list(d.glob("*.opts")):
    f.unlink()
oracle = oan.SecretAnalyzer("")
cases = dict(sm.cases())
cases["order"] = (sm.order_layer(), ["**/skipme"], ["**/7.conf"])
cases["windows"] = (sm.window_layer(), ["**/skipme"], ["**/2.log"])
for name, (layer, sd, sf) in cases.items():
    m = sm.walk(layer, sd, sf)
    kept = sum(1 for fp, size, _ in m["kept"] if oracle.required(fp, size))
    lines = ["d " + p for p in sd] + ["f " + p for p in sf]
    lines += ["k %d" % kept, "s %d %d %d" % (len(m["skipped_dirs"]), m["skipped_files"], m["under_skipped_dir"])]
    name = name.replace("-", "_")
    (d / (name + ".tar")).write_bytes(layer)
    (d / (name + ".opts")).write_text("\n".join(lines) + "\n")
PY
objs=""
pids=""
for src in trivy_amd/csrc/*.cpp oracle/native/*.cpp tools/san_layer_skip.cpp; do
  o=$out/$(basename ${src%.cpp}).o
  objs="$objs $o"
  g++ $COMMON $SAN -c $src -o $o &
  pids="$pids $!"
done
for p in $pids; do wait $p || exit 1; done
g++ $SAN -o $out/san_layer_skip $objs trivy_amd/_obj/*.hip.o -L${ROCM_PATH:-/opt/rocm}/lib -lamdhip64 -lpthread \
  -Wl,-rpath,${ROCM_PATH:-/opt/rocm}/lib || exit 1
ASAN_OPTIONS=detect_leaks=1:halt_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
  $out/san_layer_skip $out/layers/*.tar 2>&1 | tee profiles/layer_skip/san_layer_skip.log
