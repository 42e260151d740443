#!/bin/bash
# The host half of a tar layer resident in HBM (trivy_amd/csrc/tar_index_host.h: the
# chain walk over candidate records, the index, the plan and kinds of a batch whose
# arena is the layer) under ASan + UBSan, as a stand-alone program
# (tools/san_device_layer.cpp: its own main, no interpreter, no GPU, no HIP: the
# header is plain C++).  The layers are the tests' (tests/tar_index_model.py), written
# to files first; the candidate records come from the program's own model of the kernel.
# Usage: bash tools/san_device_layer.sh   (log -> profiles/device_layer/san_device_layer.log)
set -u -o pipefail
cd "$(dirname "$0")/.."
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
out=oracle/build/san_device_layer
mkdir -p $out/layers profiles/device_layer
python - "$out/layers" <<'PY' || exit 1
import sys, tarfile
from pathlib import Path
sys.path.insert(0, ".")
from tests import tar_index_model as tm
from tests.layers import make_layer
d = Path(sys.argv[1])
for f in d.glob("*.tar"):
    f.unlink()
good = {"gnu": make_layer(100 + tarfile.GNU_FORMAT, 150, tarfile.GNU_FORMAT),
        "pax": make_layer(100 + tarfile.PAX_FORMAT, 150, tarfile.PAX_FORMAT),
        "ustar_prefix": tm.ustar_prefix_layer(), "nested": tm.nested_layer(), "pax_size": tm.pax_size_layer(),
        "no_trailer": tm.no_trailer_layer(), "empty": bytes(1024), "l3": make_layer(3, 60)}
bad = bytearray(good["l3"])
bad[148] ^= 1                                   # the first header's checksum
good["bad_checksum"] = bytes(bad)
good["bad_truncated"] = good["l3"].rstrip(b"\0")[:-700]
junk = bytearray(good["l3"])
hdr = tm.candidates(good["l3"])[5][0]             # garbage where the sixth header was
junk[512 * hdr:512 * hdr + 512] = bytes((37 * i + 1) % 255 + 1 for i in range(512))
good["bad_junk_header"] = bytes(junk)
for name, data in good.items():
    (d / (name + ".tar")).write_bytes(data)
PY
g++ -O1 -g -std=c++17 -mavx2 -fno-omit-frame-pointer -Wall -I trivy_amd/csrc -I include $SAN tools/san_device_layer.cpp \
  -o $out/san_device_layer || exit 1
ASAN_OPTIONS=detect_leaks=1:halt_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
  $out/san_device_layer $out/layers/*.tar 2>&1 | tee profiles/device_layer/san_device_layer.log
