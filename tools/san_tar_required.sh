#!/bin/bash
# The host half behind the GPU's path classify and Required of a resident tar layer
# (trivy_amd/csrc/tar_required_host.h: IndexTarFiles over the file records of
# trivy_amd/csrc/tarrequired.h) under ASan + UBSan, as a stand-alone program
# (tools/san_tar_required.cpp: its own main, no interpreter, no GPU, no HIP: the headers are
# plain C++).  The layers are the tests' (tests/test_tar_required_host.py), written to files
# first, each with what the device stage hands over for it, made by the tests' model.
# Usage: bash tools/san_tar_required.sh   (log -> profiles/device_required/san_tar_required.log)
set -u -o pipefail
cd "$(dirname "$0")/.."
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
out=oracle/build/san_tar_required
mkdir -p $out/layers profiles/device_required
python - "$out/layers" <<'PY' || exit 1
import sys
from pathlib import Path
sys.path.insert(0, ".")
from tests import tar_chain_model as cm
from tests import tar_required_model as rm
from tests.test_tar_required_host import LAYERS
d = Path(sys.argv[1])
for f in d.glob("*.*"):
    f.unlink()
layers = {k.replace("-", "_"): v() for k, v in LAYERS.items()}
layers.update({"boundaries_64": cm.boundary_layer(64), "empty": bytes(1024), "nothing": b""})
for name, data in layers.items():
    entries, stop, _ = cm.chain(data)
    assert stop[0] == cm.END, name
    recs, names = cm.pack(entries)
    # no allow-path tables: every file that reaches the allow paths is asked about
    _, frecs, blob, counts = rm.stage(recs, len(entries), bytes(names), [0, len(entries)], [0, len(names)], b".", None,
                                      None)
    (d / (name + ".tar")).write_bytes(data)
    (d / (name + ".frecs")).write_bytes(frecs)
    (d / (name + ".blob")).write_bytes(blob)
    (d / (name + ".counts")).write_bytes(counts[0].tobytes())
PY
g++ -O1 -g -std=c++17 -mavx2 -pthread -fno-omit-frame-pointer -Wall -I trivy_amd/csrc -I include $SAN \
  tools/san_tar_required.cpp -o $out/san_tar_required || exit 1
ASAN_OPTIONS=detect_leaks=1:halt_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
  $out/san_tar_required $out/layers/*.tar 2>&1 | tee profiles/device_required/san_tar_required.log
