#!/bin/bash
# The host half of the forest pass over all layers of an image (trivy_amd/csrc/tarforest.h: the
# virtual block space, the cut into passes, the bases of the layers in the two shared buffers;
# trivy_amd/csrc/tar_index_host.h: IndexTarEntries per layer) under ASan + UBSan, as a stand-alone
# program (tools/san_tar_forest.cpp: its own main, no interpreter, no GPU, no HIP: the headers are
# plain C++).  The layers are the tests' (tests/tar_index_model.py, tests/tar_chain_model.py),
# written to files first; together they are one image.
# Usage: bash tools/san_tar_forest.sh   (log -> profiles/device_layers/san_tar_forest.log)
set -u -o pipefail
cd "$(dirname "$0")/.."
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
out=oracle/build/san_tar_forest
mkdir -p $out/layers profiles/device_layers
python - "$out/layers" <<'PY' || exit 1
import sys, tarfile
from pathlib import Path
sys.path.insert(0, ".")
from tests import tar_chain_model as cm
from tests import tar_index_model as tm
from tests.layers import make_layer
d = Path(sys.argv[1])
for f in d.glob("*.tar"):
    f.unlink()
good = {"gnu3": make_layer(3, 60, tarfile.GNU_FORMAT), "pax7": make_layer(7, 60, tarfile.PAX_FORMAT),
        "ustar": cm.ustar_layer(), "odd_names": cm.odd_names_layer(), "nested": tm.nested_layer(),
        "pax_size": tm.pax_size_layer(), "no_trailer": tm.no_trailer_layer(), "empty": bytes(1024), "nothing": b"",
        "boundaries_64": cm.boundary_layer(64)}
good.update({"l20_%02d" % s: make_layer(s, 20, tarfile.PAX_FORMAT if s % 2 else tarfile.GNU_FORMAT) for s in range(8)})
good.update({"case_" + k.replace("-", "_"): v for k, v in cm.complete_cases().items()})
for k, (v, reason, _) in cm.punt_cases().items():
    malformed = reason not in (cm.CAP, cm.PAX_SIZE_FORM)
    good[("bad_" if malformed else "left_to_host_") + k.replace("-", "_").replace("+", "p")] = v
# (sorted by name the malformed layers come first: every later layer's slice starts after layers that hand nothing over)
for name, data in good.items():
    (d / (name + ".tar")).write_bytes(data)
PY
g++ -O1 -g -std=c++17 -mavx2 -pthread -fno-omit-frame-pointer -Wall -I trivy_amd/csrc -I include $SAN tools/san_tar_forest.cpp \
  -o $out/san_tar_forest || exit 1
ASAN_OPTIONS=detect_leaks=1:halt_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
  $out/san_tar_forest $out/layers/*.tar 2>&1 | tee profiles/device_layers/san_tar_forest.log
