"""The skip stage on a layer that records directories: 12,000 directories u<j>/skipme, each with eight files
below it (four before its entry, four after) and eight beside it, 204,000 entries in all; IndexDevice with
--skip-dirs "**/skipme" --skip-files "**/*.pem", the switch off and on interleaved, 20 steps after 5.
Run from the repository root: python profiles/device_required_skip/job_dirs.py OUT.jsonl"""
import json
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from tests import tar_chain_model as cm  # noqa: E402
from trivy_amd.analyzer import AnalyzerOptions, SecretAnalyzer  # noqa: E402
from trivy_amd.walker import NewLayerTar, Option  # noqa: E402

UNITS = 12000
parts = []
for j in range(UNITS):
    parts += [cm.member(b"u%d/skipme/f%d.conf" % (j, k), cm.TEXT) for k in range(4)]
    parts.append(cm.member(b"u%d/skipme/" % j, b"", b"5"))
    parts += [cm.member(b"u%d/skipme/f%d.conf" % (j, k), cm.TEXT) for k in range(4, 8)]
    parts += [cm.member(b"u%d/keep/f%d.conf" % (j, k), cm.TEXT) for k in range(8)]
layer = b"".join(parts) + cm.TRAILER
dev = torch.from_numpy(np.frombuffer(layer + bytes(64), dtype=np.uint8).copy()).to("cuda:0")
an = SecretAnalyzer(device=0)
an.Init(AnalyzerOptions())
an.set_tar_walk("gpu")
an.set_tar_required("gpu")
an.set_layer_walker(NewLayerTar(Option(SkipFiles=["**/*.pem"], SkipDirs=["**/skipme"])))
res = {"host": [], "gpu": []}
for step in range(25):
    for mode in ("host", "gpu"):
        an.set_tar_required_skip(mode)
        st = {}
        ix = an.IndexDevice(dev, len(layer), stats=st)
        if step >= 5:
            res[mode].append((st["ms_total"], ix.required_skip_stats, ix.required_stats, ix.n, ix.skip_stats))
assert res["host"][-1][3] == res["gpu"][-1][3] and res["host"][-1][4] == res["gpu"][-1][4]
with open(sys.argv[1], "w") as f:
    for mode in ("host", "gpu"):
        ms = [r[0] for r in res[mode]]
        ss, rs = res[mode][-1][1], res[mode][-1][2]
        line = json.dumps({"tool": "job_dirs", "switch": mode, "gb": len(layer) / 1e9, "entries": 17 * UNITS,
                           "files": res[mode][-1][3], "skip": res[mode][-1][4], "index_ms_total": statistics.median(ms),
                           "min_ms": min(ms), "max_ms": max(ms), "required_reason": rs["reason"],
                           "required_ms_kernel": statistics.median(r[2]["ms_kernel"] for r in res[mode]),
                           "skip_reason": ss["reason"], "table_slots": ss["table_slots"],
                           "skip_ms_kernel": statistics.median(r[1]["ms_kernel"] for r in res[mode])})
        print(line)
        f.write(line + "\n")
