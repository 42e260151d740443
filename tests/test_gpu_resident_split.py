"""Resident batches with a transform in split mode (Scanner.set_resident_transform("split"),
DESIGN.md 4.12): the files the transform leaves as read are scanned where they lie, as an
untransformed resident batch that skips the others; the files it changes are gathered from the arena,
rewritten and scanned as a second batch.  In every case the split result's JSON and records equal the
chunked mode's byte for byte, and the per-file secrets equal the oracle's on the transformed contents.
"""
import numpy as np
import pytest

from oracle import analyzer as oan
from oracle import secret_scanner as osc

pytestmark = pytest.mark.gpu

AWS = b"AKIA" + b"Q" * 16
GH = b"ghp_" + b"a1B2" * 9
TILE = 4096
SPLIT_ZERO = {"mode_used": 0, "files_in_place": 0, "bytes_in_place": 0, "files_changed": 0, "bytes_changed": 0,
              "files_dropped": 0, "bytes_dropped": 0, "ms_census": 0.0, "ms_sub": 0.0}


@pytest.fixture(scope="module")
def scanner():
    import trivy_amd.secret as secret
    s = secret.NewScanner(None)
    assert s.resident_transform() == "chunked"
    return s


@pytest.fixture(scope="module")
def oracle():
    return osc.new_scanner(None)


def _resident(files):
    import torch
    contents = [b for _, b, _ in files]
    offs = np.zeros(len(files) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in contents])
    arena = np.frombuffer(b"".join(contents) + b"\0" * 64, dtype=np.uint8).copy()
    d_arena = torch.from_numpy(arena).to("cuda:0")
    d_offs = torch.from_numpy(offs.view(np.int64)).to("cuda:0")
    return arena, offs, d_arena, d_offs


def _transformed(b, k):
    return b if k == 0 else b.replace(b"\r", b"") if k == 1 else oan.extract_printable_bytes(b) if k == 2 else b""


def _model(files):
    """What the census marks say: (in place, changed, dropped) as (files, bytes) pairs."""
    cnt = {"in_place": [0, 0], "changed": [0, 0], "dropped": [0, 0]}
    for _, b, k in files:
        key = "dropped" if k == 3 else "changed" if k == 2 or (k == 1 and b"\r" in b) else "in_place"
        cnt[key][0] += 1
        cnt[key][1] += len(b)
    return cnt


def _check_stats(ss, files):
    m = _model(files)
    assert ss["mode_used"] == 1
    for key in ("in_place", "changed", "dropped"):
        assert (ss["files_" + key], ss["bytes_" + key]) == tuple(m[key]), key


def _both(s, files, oracle=None, mirrored=False, text=True):
    """Chunked and split scans of `files` ((path, bytes, kind) triples) on scanner s -> (chunked, split)."""
    import torch
    arena, offs, d_arena, d_offs = _resident(files)
    paths = [p for p, _, _ in files]
    kinds = np.array([k for _, _, k in files], dtype=np.uint8)
    binary = np.array([1 if k == 2 else 0 for _, _, k in files], dtype=np.uint8)
    n = len(files)

    def scan():
        if mirrored:
            return s.scan_arena(arena, offs, paths, binary=binary, dev_arena=d_arena.data_ptr(),
                                dev_offsets=d_offs.data_ptr(), transform=kinds)
        return s.scan_device(d_arena, offs, paths, binary=binary, transform=kinds, dev_offsets=d_offs)

    assert s.resident_transform() == "chunked"
    chunked = scan()
    assert chunked.split_stats() == SPLIT_ZERO
    s.set_resident_transform("split")
    try:
        split = scan()
    finally:
        s.set_resident_transform("chunked")
    if n and text:
        assert split.raw_text(0, n) == chunked.raw_text(0, n)
    assert split.records().tobytes() == chunked.records().tobytes()
    if n and int(offs[-1]):
        _check_stats(split.split_stats(), files)
    if oracle is not None:
        raw = split.raw()
        for (p, b, k), g, r in zip(files, split.secrets(paths), raw):
            if k == 3:
                assert r["kind"] == 0, p
            else:
                assert g.to_dict() == oracle.scan(p, _transformed(b, k), k == 2), p
    torch.cuda.synchronize()
    return chunked, split


def _lines(n, eol=b"\n"):
    return b"".join(b"line %04d of filler text" % i + eol for i in range(n))


def _main_batch():
    files = []

    def cur():
        return sum(len(b) for _, b, _ in files)

    crlf_split = b"[main]\r\nkey = " + AWS[:8] + b"\r" + AWS[8:] + b"\r\nend\r\n"
    files.append(("a/crlf_split.txt", crlf_split, 1))    # matches only once the '\r' is gone
    files.append(("a/same_bytes.txt", crlf_split, 0))    # the same bytes as they are: no match
    files.append(("lib/mod.pyc", b"\x03\xf3\r\n\x00\x00\x00\x00abcd\x00hello world k=" + AWS + b"\x00" + b"y" * 40 +
                  b"\x01tail", 2))
    files.append(("b/lf_only.txt", b"plain\nt = " + GH + b"\nno carriage returns here\n", 1))  # in place
    # a dropped file with a token between two kept files, the three inside one tile; the kept
    # files' tokens end 1 byte before / start 2 bytes behind it
    files.append(("c/left.cfg", b"# left\n" + _lines(3) + b"key = " + AWS + b"\n", 0))
    files.append(("c/dropped.bin", b"x = " + AWS + b"\nt = " + GH + b"\n", 3))
    files.append(("c/right.cfg", b"t=" + GH + b"\n" + _lines(3), 0))
    assert cur() < TILE
    # a changed file with tokens within 16 B of its start and of its end
    files.append(("d/edges.ini", b"k=" + AWS + b"\r\n" + _lines(40, b"\r\n") + b"t=" + GH, 1))
    # dropped tiles, then an in-place file whose token straddles a tile edge, the tiles behind it dropped too
    files.append(("e/before.bin", (b"k = " + AWS + b"\n") * 40 + b"z" * (3 * TILE), 3))
    start = cur()
    edge = (start // TILE + 2) * TILE
    lead = edge - 10 - start - 5
    straddle = _lines(lead // 20 + 2)[:lead] + b"\nk = " + AWS + b"\nrest\n"
    files.append(("e/straddle.txt", straddle, 0))
    assert start + straddle.index(AWS) == edge - 10
    files.append(("e/behind.bin", (b"t = " + GH + b"\r\n") * 30 + b"w" * (3 * TILE), 3))
    files.append(("f/empty.txt", b"", 1))
    files.append(("f/last.txt", b"the last file\nk = " + AWS + b"\n", 0))
    return files


@pytest.fixture(scope="module")
def main_batch():
    files = _main_batch()
    m = _model(files)
    assert m["changed"][0] == 3 and m["dropped"][0] == 3 and m["in_place"][0] == len(files) - 6
    return files


def _found(result, files):
    return {p for (p, _, _), r in zip(files, result.raw()) if r["kind"] == 2}


EXPECT_FOUND = {"a/crlf_split.txt", "lib/mod.pyc", "b/lf_only.txt", "c/left.cfg", "c/right.cfg", "d/edges.ini",
                "e/straddle.txt", "f/last.txt"}


# ---- 1. chunked against split --------------------------------------------------------
def test_split_equals_chunked(scanner, oracle, main_batch):
    files = main_batch
    chunked, split = _both(scanner, files, oracle)
    assert _found(split, files) == EXPECT_FOUND  # not same_bytes.txt, no dropped file
    paths = [p for p, _, _ in files]
    sec = dict(zip(paths, split.secrets(paths)))
    assert len(sec["d/edges.ini"].Findings) == 2
    assert all(f.Code.Lines is None for f in sec["lib/mod.pyc"].Findings)  # Binary: Code without lines
    # fetched: in-place files only -- never a dropped or a changed one
    fs = split.fetch_stats()
    in_place_found = {p for p, b, k in files if p in EXPECT_FOUND and not (k == 2 or (k == 1 and b"\r" in b))}
    in_place_tokens = [p for p, b, k in files if k in (0, 1) and b"\r" not in b and (b"AKIA" in b or b"ghp_" in b)]
    assert len(in_place_found) <= fs["files"] <= len(in_place_tokens) + 1  # (+ same_bytes.txt, if a candidate)
    ss = split.split_stats()
    assert ss["ms_census"] > 0 and ss["ms_sub"] > 0


def test_ragged_tile_candidate_is_dropped(scanner, oracle):
    """The only tokens lie in a dropped file that shares its tile with two kept files: its tile is
    streamed, its candidates must reach neither the fetch nor the exact pass."""
    files = [("k/left.txt", _lines(5), 0),
             ("k/dropped.bin", b"x = " + AWS + b"\nt = " + GH + b"\n", 3),
             ("k/right.txt", _lines(5), 1)]
    _, split = _both(scanner, files, oracle)
    assert _found(split, files) == set()
    assert split.fetch_stats()["files"] == 0 and split.fetch_stats()["bytes"] == 0


# ---- 2. fetch modes ------------------------------------------------------------------
def _windows_case(s, oracle, files):
    by_files_chunked, by_files = _both(s, files)
    s.set_fetch_mode("windows")
    try:
        chunked, split = _both(s, files, oracle)
    finally:
        s.set_fetch_mode("files")
    n = len(files)
    assert split.raw_text(0, n) == by_files.raw_text(0, n) == by_files_chunked.raw_text(0, n)
    assert chunked.fetch_window_stats()["mode_used"] == 0  # a transformed batch in chunks keeps the files fetch
    ws = split.fetch_window_stats()
    assert ws["mode_used"] == 1 and ws["window_bytes"] == 256 * ws["granules"] and ws["granules"] > 0
    # the changed files' findings carry their lines: made by the host from the transformed bytes
    paths = [p for p, _, _ in files]
    sec = dict(zip(paths, split.secrets(paths)))
    for p in ("a/crlf_split.txt", "d/edges.ini"):
        for f in sec[p].Findings:
            assert f.Code.Lines and all(b"\r" not in l.Content.encode() for l in f.Code.Lines), p
    return split


def test_windows_mode(scanner, oracle, main_batch):
    split = _windows_case(scanner, oracle, main_batch)
    assert _found(split, main_batch) == EXPECT_FOUND


def test_windows_mode_gpu_findings(oracle, main_batch, monkeypatch):
    import trivy_amd.secret as secret
    monkeypatch.setenv("TSG_GPU_FINDINGS", "1")
    s = secret.NewScanner(None)
    split = _windows_case(s, oracle, main_batch)
    assert _found(split, main_batch) == EXPECT_FOUND


# ---- 3. degenerate splits --------------------------------------------------------------
def test_no_file_changed(scanner, oracle):
    files = [("n/%d.txt" % i, _lines(i) + b"k = " + AWS + b"\n" + _lines(7 - i), 1) for i in range(6)]
    _, split = _both(scanner, files, oracle)
    ss = split.split_stats()
    assert ss["files_changed"] == 0 and ss["ms_sub"] == 0 and ss["files_in_place"] == 6
    assert len(_found(split, files)) == 6


def test_every_file_changed(scanner, oracle):
    files = [("c/%d.ini" % i, _lines(i, b"\r\n") + b"k = " + AWS + b"\r\n" + _lines(200 * i, b"\r\n"), 1)
             for i in range(1, 6)]
    _, split = _both(scanner, files, oracle)
    ss = split.split_stats()
    assert ss["files_in_place"] == 0 and ss["files_changed"] == 5
    assert len(_found(split, files)) == 5 and split.fetch_stats()["files"] == 0


def test_every_file_dropped(scanner, oracle):
    files = [("d/%d.bin" % i, b"k = " + AWS + b"\n" + _lines(50 * i), 3) for i in range(5)]
    _, split = _both(scanner, files, oracle)
    ss = split.split_stats()
    assert ss["files_dropped"] == 5 and ss["files_changed"] == 0 and ss["files_in_place"] == 0
    assert _found(split, files) == set() and split.fetch_stats()["files"] == 0


@pytest.mark.parametrize("kind,eol", [(0, b"\n"), (1, b"\n"), (1, b"\r\n"), (2, b"\n"), (3, b"\n")])
def test_one_file(scanner, oracle, kind, eol):
    files = [("one/f.pyc" if kind == 2 else "one/f.txt", b"a = 1" + eol + b"k = " + AWS + eol, kind)]
    _, split = _both(scanner, files, oracle)
    assert len(_found(split, files)) == (0 if kind == 3 else 1)


def test_empty_batches(scanner):
    _, split = _both(scanner, [])
    assert split.split_stats() == SPLIT_ZERO
    _, split = _both(scanner, [("e/a.txt", b"", 1), ("e/b.txt", b"", 3)])  # files, no bytes
    assert split.split_stats() == SPLIT_ZERO and [r["kind"] for r in split.raw()] == [0, 0]


# ---- 4. a mirrored batch ---------------------------------------------------------------
def test_mirrored_batch(scanner, oracle, main_batch):
    chunked, split = _both(scanner, main_batch, oracle, mirrored=True)
    assert _found(split, main_batch) == EXPECT_FOUND
    assert split.fetch_stats()["files"] == 0 and split.fetch_stats()["bytes"] == 0
    assert split.fetch_window_stats()["mode_used"] == 0


# ---- 5. the analyzer -------------------------------------------------------------------
def _analyze_files():
    body = b"# settings\nname = demo\n"
    late_nul = b"k = " + AWS + b"\n" + b"x" * 300 + b"\x00 and more text\n"
    return [("etc/plain.conf", body + b"key = " + AWS + b"\nend\n"),
            ("etc/crlf.ini", b"[main]\r\ntoken = " + GH + b"\r\nmore = 1\r\n" * 4),
            ("lib/mod.pyc", b"\x03\xf3\r\n\x00\x00\x00\x00abcd\x00hello world k=" + AWS + b"\x00" + b"y" * 40 +
             b"\x01tail"),
            ("bin/blob.dat", b"heads\x00\x01 key = " + AWS + b"\n" + b"z" * 60),
            ("var/late_nul.txt", late_nul),
            ("node_modules/x.js", b"var t = '" + GH + b"';\n"),
            ("img/a.png", b"not really a png: " + AWS + b"\n"),
            ("go.sum", b"example.com/m v1.0.0 h1:" + AWS + b"=\n"),
            ("tiny.txt", b"123456789"),
            ("etc/clean.txt", b"nothing to see here\n" * 5)]


@pytest.mark.parametrize("dir_", ["", "/src"])
def test_analyze_device_in_split_mode(dir_):
    import torch
    from trivy_amd.analyzer import AnalyzerOptions, SecretAnalyzer
    a = SecretAnalyzer()  # a scanner and analyzer of this test's own: no other module sees the mode
    a.Init(AnalyzerOptions())
    ref = oan.SecretAnalyzer("")
    files = _analyze_files()
    contents = [b for _, b in files]
    offs = np.zeros(len(files) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in contents])
    d_arena = torch.from_numpy(np.frombuffer(b"".join(contents) + b"\0" * 64, dtype=np.uint8).copy()).to("cuda:0")
    paths = [p for p, _ in files]
    want = [ref.analyze(p, dir_, b) if ref.required(p, len(b)) else None for p, b in files]

    def same(got):
        assert len(got) == len(want)
        for p, g, w in zip(paths, got, want):
            if w is None:
                assert g is None, p
            else:
                assert g is not None and [s.to_dict() for s in g.Secrets] == w["Secrets"], p

    chunked = a.AnalyzeDeviceAsync(d_arena, offs, paths, dir_)
    got_chunked = chunked.wait()
    same(got_chunked)
    assert chunked.result.split_stats() == SPLIT_ZERO
    a.scanner.set_resident_transform("split")
    p1 = a.AnalyzeDeviceAsync(d_arena, offs, paths, dir_)  # two submits in flight,
    p2 = a.AnalyzeDeviceAsync(d_arena, offs, paths, dir_)
    got2 = p2.wait()                                       # waited for in reverse order
    got1 = p1.wait()
    same(got1)
    same(got2)
    n = len(files)
    assert p1.result.raw_text(0, n) == p2.result.raw_text(0, n) == chunked.result.raw_text(0, n)
    ss = p1.result.split_stats()
    assert ss["mode_used"] == 1 and ss["files_changed"] == 2 and ss["files_in_place"] + ss["files_dropped"] == n - 2
    assert {p for p, g in zip(paths, got1) if g is not None} == \
        {"etc/plain.conf", "etc/crlf.ini", "lib/mod.pyc", "var/late_nul.txt"}
    torch.cuda.synchronize()


# ---- 6. candidate overflow ---------------------------------------------------------------
def test_candidate_overflow_reruns_with_the_marks():
    """More candidates than the engine's first candidate buffer holds (64 Ki records): the in-place
    scan is rerun synchronously with the skip list and drop_marked, and a dropped file full of
    tokens in the middle still yields nothing."""
    import trivy_amd.secret as secret
    s = secret.NewScanner(None)  # fresh buffers
    dense = (b"k = " + AWS + b"\n") * 36000
    files = [("o/dense_a.txt", dense, 1),
             ("o/dropped.bin", (b"k = " + AWS + b"\n") * 2000, 3),
             ("o/crlf.ini", (b"k = " + AWS + b"\r\n") * 50, 1),
             ("o/dense_b.txt", dense, 0)]
    assert sum(len(b) for _, b, _ in files) < 2 << 20
    chunked, split = _both(s, files, text=False)  # (the records carry a digest of every finding's text)
    rec = split.records()
    assert len(rec) == 2 * 36000 + 50 > 1 << 16
    assert set(np.unique(rec["file"]).tolist()) == {0, 2, 3}
    assert split.stats()["candidates"] >= len(rec)


# ---- 7. mode off ---------------------------------------------------------------------------
def test_mode_off_reports_nothing(scanner, main_batch):
    files = main_batch
    _, offs, d_arena, d_offs = _resident(files)
    kinds = np.array([k for _, _, k in files], dtype=np.uint8)
    r = scanner.scan_device(d_arena, offs, [p for p, _, _ in files], transform=kinds, dev_offsets=d_offs)
    assert scanner.resident_transform() == "chunked"
    ss = r.split_stats()
    assert ss == SPLIT_ZERO and ss["mode_used"] == 0


def test_env_sets_the_initial_mode(monkeypatch):
    import trivy_amd.secret as secret
    monkeypatch.setenv("TSG_RESIDENT_TRANSFORM", "split")
    s = secret.NewScanner(None)
    assert s.resident_transform() == "split"
    monkeypatch.setenv("TSG_RESIDENT_TRANSFORM", "chunked")
    assert secret.NewScanner(None).resident_transform() == "chunked"
    s.set_resident_transform("chunked")
    assert s.resident_transform() == "chunked"
    with pytest.raises(ValueError):
        s.set_resident_transform("both")
