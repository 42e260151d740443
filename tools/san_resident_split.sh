#!/bin/bash
# The host half of the split scan (trivy_amd/csrc/split_host.h: the sub-batch plan,
# the candidate remapping, the merge of the exact pass's views) under ASan + UBSan,
# as a stand-alone program (tools/san_resident_split.cpp: its own main, no
# interpreter, no GPU, no HIP: the header is plain C++).
# Usage: bash tools/san_resident_split.sh   (log -> profiles/resident_split/san_resident_split.log)
set -u -o pipefail
cd "$(dirname "$0")/.."
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
out=oracle/build/san_resident_split
mkdir -p $out profiles/resident_split
g++ -O1 -g -std=c++17 -fno-omit-frame-pointer -Wall -I trivy_amd/csrc $SAN tools/san_resident_split.cpp \
  -o $out/san_resident_split || exit 1
ASAN_OPTIONS=detect_leaks=1:halt_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
  $out/san_resident_split 2>&1 | tee profiles/resident_split/san_resident_split.log
