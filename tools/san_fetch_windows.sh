#!/bin/bash
# The host half of the windows fetch (plan, bounded regex search, sparse exact
# pass) under ASan + UBSan, as a stand-alone program (tools/san_fetch_windows.cpp:
# its own main, no interpreter, no GPU): the product's host C++ and the oracle
# hooks are compiled with the sanitizers and linked with the program; the gfx950
# device objects are linked as built (nothing of them runs here).
# Usage: bash tools/san_fetch_windows.sh   (log -> profiles/fetch_windows/san_fetch_windows.log)
set -u -o pipefail
cd "$(dirname "$0")/.."
python -c "import __graft_entry__ as g; g.build()" || exit 1
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
COMMON="-O1 -g -march=x86-64-v3 -fPIC -std=c++17 -fno-omit-frame-pointer -I trivy_amd/csrc -I include -I oracle/native -D__HIP_PLATFORM_AMD__ -I ${ROCM_PATH:-/opt/rocm}/include"
out=oracle/build/san_fetch_windows
mkdir -p $out
objs=""
pids=""
for src in trivy_amd/csrc/*.cpp oracle/native/*.cpp tools/san_fetch_windows.cpp; do
  o=$out/$(basename ${src%.cpp}).o
  objs="$objs $o"
  g++ $COMMON $SAN -c $src -o $o &
  pids="$pids $!"
done
for p in $pids; do wait $p || exit 1; done
g++ $SAN -o $out/san_fetch_windows $objs trivy_amd/_obj/*.hip.o -L${ROCM_PATH:-/opt/rocm}/lib -lamdhip64 -lpthread \
  -Wl,-rpath,${ROCM_PATH:-/opt/rocm}/lib || exit 1
mkdir -p profiles/fetch_windows
ASAN_OPTIONS=detect_leaks=1:halt_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
  $out/san_fetch_windows 2>&1 | tee profiles/fetch_windows/san_fetch_windows.log
