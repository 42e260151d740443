#!/bin/bash
# The host side of LayerTar's skip options in the GPU's Required stage of a resident tar layer
# (tsg_analyzer_set_tar_required_skip): the pattern classifier and the matcher of
# trivy_amd/csrc/tar_skip_dev.h and the extended IndexTarFiles of
# trivy_amd/csrc/tar_required_host.h, under ASan + UBSan, as a stand-alone program
# (tools/san_tar_required_skip.cpp: its own main, no interpreter, no GPU, no HIP: the headers
# are plain C++).  The layers and patterns are the tests' (tests/test_tar_required_skip_host.py),
# written to files first, each layer with its options and with what the device stage hands over
# for it, made by the tests' model.
# Usage: bash tools/san_tar_required_skip.sh   (log -> profiles/device_required_skip/san_tar_required_skip.log)
set -u -o pipefail
cd "$(dirname "$0")/.."
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
out=oracle/build/san_tar_required_skip
mkdir -p $out/layers profiles/device_required_skip
python - "$out/layers" <<'PY' || exit 1
import sys
from pathlib import Path
sys.path.insert(0, ".")
from tests import tar_chain_model as cm
from tests import tar_required_skip_model as km
from tests.test_tar_required_skip_host import LAYERS, PATTERNS
d = Path(sys.argv[1])
for f in d.glob("*.*"):
    f.unlink()
(d / "patterns.txt").write_text("".join("%s%s\n" % ("-" if form is None else "+", p) for p, form in PATTERNS if p),
                                encoding="utf-8")
for name, (make, skip_dirs, skip_files, falls_back) in LAYERS.items():
    name, data = name.replace("-", "_"), make()
    entries, stop, _ = cm.chain(data)
    assert stop[0] == cm.END, name
    recs, names = cm.pack(entries)
    # no allow-path tables: every file that reaches the allow paths is asked about
    _, frecs, blob, counts = km.stage(recs, len(entries), bytes(names), [0, len(entries)], [0, len(names)], b".", None,
                                      None, [p.encode() for p in skip_dirs], [p.encode() for p in skip_files])
    (d / (name + ".tar")).write_bytes(data)
    (d / (name + ".dirs")).write_text("".join(p + "\n" for p in skip_dirs))
    (d / (name + ".files")).write_text("".join(p + "\n" for p in skip_files))
    (d / (name + ".frecs")).write_bytes(frecs)
    (d / (name + ".blob")).write_bytes(blob)
    (d / (name + ".counts")).write_bytes(counts[0].tobytes())
    if falls_back:
        (d / (name + ".fallback")).write_text("")
PY
g++ -O1 -g -std=c++17 -mavx2 -pthread -fno-omit-frame-pointer -Wall -I trivy_amd/csrc -I include $SAN \
  tools/san_tar_required_skip.cpp -o $out/san_tar_required_skip || exit 1
ASAN_OPTIONS=detect_leaks=1:halt_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
  $out/san_tar_required_skip $out/layers/patterns.txt $out/layers/*.tar 2>&1 | tee profiles/device_required_skip/san_tar_required_skip.log
