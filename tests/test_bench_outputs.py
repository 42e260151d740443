"""bench.py's --dump-outputs and --full plumbing (CPU).

dump_outputs writes the last timed step's result as float64 .npy files; here the result is a
ScanResult of the exact host pass over a small corpus (no GPU), and the files must give the
result's records back exactly -- the 64-bit digest included, which float64 cannot hold whole --
and identically on a second call.  The option parsing is checked on --dry-run (no GPU)."""
import json
import os
import subprocess
import sys

import numpy as np

from tests.corpus import make_corpus
from tests.test_host_tail import host_tail_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_findings_roundtrip(tmp_path):
    import bench
    files = [(p, b.replace(b"\r", b"")) for p, b in make_corpus(21, 150)]
    res = host_tail_scan(None, files, raw=True)
    rec = res.records()
    assert len(rec) > 5
    bench.dump_outputs(str(tmp_path / "a"), 0, 1, res, None)
    bench.dump_outputs(str(tmp_path / "b"), 0, 1, res, None)
    assert sorted(os.listdir(tmp_path / "a")) == ["findings.npy", "findings_count.npy"]
    assert np.load(tmp_path / "a" / "findings_count.npy").tolist() == [float(len(rec))]
    a = np.load(tmp_path / "a" / "findings.npy")
    assert a.dtype == np.float64 and a.shape == (len(rec), 6)
    assert np.array_equal(a, np.load(tmp_path / "b" / "findings.npy"))
    assert np.array_equal(a[:, 0].astype(np.uint32), rec["file"])
    assert np.array_equal(a[:, 1].astype(np.uint32), rec["rule"])
    assert np.array_equal(a[:, 2].astype(np.int64), rec["start_line"])
    assert np.array_equal(a[:, 3].astype(np.int64), rec["end_line"])
    digest = (a[:, 4].astype(np.uint64) << np.uint64(32)) | a[:, 5].astype(np.uint64)
    assert np.array_equal(digest, rec["digest"])
    assert len(set(rec["digest"] >> np.uint64(32))) > 1  # (the high half is in use)


def test_dump_outputs_samples_past_the_row_cap(tmp_path, monkeypatch):
    """Past DUMP_MAX_ROWS the rows are a fixed sample in the result's order: the same rows on
    every call, each one a row of the full dump, the full count beside them."""
    import bench
    files = [(p, b.replace(b"\r", b"")) for p, b in make_corpus(22, 150)]
    res = host_tail_scan(None, files, raw=True)
    n = len(res.records())
    bench.dump_outputs(str(tmp_path / "all"), 0, 1, res, None)
    monkeypatch.setattr(bench, "DUMP_MAX_ROWS", n // 2)
    bench.dump_outputs(str(tmp_path / "a"), 0, 1, res, None)
    bench.dump_outputs(str(tmp_path / "b"), 0, 1, res, None)
    full, a = np.load(tmp_path / "all" / "findings.npy"), np.load(tmp_path / "a" / "findings.npy")
    assert a.shape == (n // 2, 6) and np.array_equal(a, np.load(tmp_path / "b" / "findings.npy"))
    assert np.load(tmp_path / "a" / "findings_count.npy").tolist() == [float(n)]
    rows = [tuple(r) for r in full]
    picks = [rows.index(tuple(r)) for r in a]
    assert picks == sorted(picks) and len(set(picks)) == len(picks)


def test_dump_outputs_analyzer_counts_and_rank_suffix(tmp_path):
    import bench
    st = {"added": 12, "input_bytes": 3456, "scan_findings": 7, "walk_s": 0.5}
    bench.dump_outputs(str(tmp_path), 1, 2, None, st)
    assert os.listdir(tmp_path) == ["analysis_counts_rank1.npy"]
    a = np.load(tmp_path / "analysis_counts_rank1.npy")
    assert a.dtype == np.float64 and a.tolist() == [12.0, 3456.0, 7.0]


def test_bench_accepts_full_and_dump_outputs():
    """--full and --dump-outputs parse beside the plain arguments, and --steps sets the timed steps
    (the dry run: no GPU, nothing dumped)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                            "MASTER_PORT", "LOCAL_WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                        "--full", "--dump-outputs", os.devnull, "--dry-run"],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["steps"] == 4 and d["n_gpus"] == 1 and d["ms_per_step"] >= 0
