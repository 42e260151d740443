"""Analyze for files whose bytes exist only in HBM (SecretAnalyzer.ClassifyDevice / AnalyzeDevice,
tsg_analyzer_classify_device / _submit_device): the binary gate runs on the GPU over the resident
arena (trivy_amd/csrc/classify.hip), a skipped file is dropped where it lies by the pre-transform
(kind 3, trivy_amd/csrc/xform.hip), and the results are what Analyze returns.  Everything is
compared with oracle/analyzer.py.
"""
import ctypes as c
import random

import numpy as np
import pytest

from oracle import analyzer as oan

pytestmark = pytest.mark.gpu

AWS = b"AKIA" + b"Q" * 16
GH = b"ghp_" + b"a1B2" * 9

LENGTHS = [0, 1, 9, 10, 15, 16, 17, 31, 299, 300, 301, 316, 1000]
BAD = [0x00, 0x06, 0x0B, 0x0E, 0x1A, 0x1C, 0x1F, 0x7F]
CONTROLS = [0x07, 0x09, 0x0A, 0x0C, 0x0D, 0x1B, 0x20, 0x7E, 0x80, 0xFF]
WHERE = ["first", "last", "299", "300", "prev_last", "next_first", "middle"]


def _offsets(contents):
    offs = np.zeros(len(contents) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in contents])
    return offs


# ---- 1. the heads ----------------------------------------------------------
def _head_files():
    """~3,000 files of b"a" with one byte planted per case.  A case is (length, start phase, where the
    byte goes); a filler file before each case brings the case's start to its phase, and carries the
    bytes planted just outside the case (its last byte, the next filler's first)."""
    values = BAD + CONTROLS
    files, cases, cur, k = [], [], 0, 0
    for ln in LENGTHS:
        for phase in range(16):
            for where in WHERE:
                if files:
                    pad = (phase - cur) % 16 or 16
                    files.append(bytearray(b"a" * pad))
                    cur += pad
                assert cur % 16 == phase
                files.append(bytearray(b"a" * ln))
                cases.append((len(files) - 1, where, values[k % len(values)], cur % 16, ln))
                cur += ln
                k += 1
    # the arena's last file: its head reaches the arena's end in the middle of a 16-B block
    pad = (5 - 17 - cur) % 16 or 16
    files += [bytearray(b"a" * pad), bytearray(b"a" * 17)]
    for i, where, v, _, ln in cases:
        f = files[i]
        if where == "first" and ln:
            f[0] = v
        elif where == "last" and ln:
            f[-1] = v
        elif where == "299" and ln > 299:
            f[299] = v
        elif where == "300" and ln > 300:
            f[300] = v
        elif where == "prev_last" and i > 0:
            files[i - 1][-1] = v
        elif where == "next_first":
            files[i + 1][0] = v
        elif where == "middle" and ln > 2:
            f[ln // 2] = v
    return [bytes(f) for f in files], cases


def test_heads_vs_is_binary():
    from trivy_amd import _lib
    L = _lib.lib()
    L.tsg_debug_classify.argtypes = [c.c_int, c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint32, c.c_void_p]
    assert oan.is_binary(b"a" * 300 + b"\0", 301) is False  # byte 300 is past the head
    assert [b for b in range(256) if oan.is_binary(bytes([b]), 1)] == \
        [b for b in range(256) if b == 0x7F or (b < 0x20 and (0xF7FFC87F >> b) & 1)]
    files, cases = _head_files()
    assert 2900 <= len(files) <= 3100
    assert {(ph, ln) for _, _, _, ph, ln in cases} == {(ph, ln) for ph in range(16) for ln in LENGTHS}
    offs = _offsets(files)
    assert offs[0] == 0 and int(offs[-1]) % 16 == 5
    raw = np.frombuffer(b"".join(files), dtype=np.uint8)  # (the hook appends the 64 pad bytes, 0x00)
    flags = np.full(len(files), 0x55, dtype=np.uint8)
    rc = L.tsg_debug_classify(0, raw.ctypes.data, int(offs[-1]), offs.ctypes.data, len(files), flags.ctypes.data)
    assert rc == 0, _lib.last_error(L)
    want = np.array([1 if oan.is_binary(b, len(b)) else 0 for b in files], dtype=np.uint8)
    assert 200 < int(want.sum()) < len(files) - 200  # both answers are well represented
    wrong = np.nonzero(flags != want)[0]
    assert len(wrong) == 0, [(int(i), int(offs[i]) % 16, len(files[i]), int(flags[i]), int(want[i]))
                             for i in wrong[:10]]


# ---- 2. kind 3 -------------------------------------------------------------
def _text(rng, n, alphabet=b"abcdefghij =:/\n"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _drop_files():
    rng = random.Random(21)
    fk = [(b"drop-first" * 3, 3),  # first in the batch
          (_text(rng, 100), 0),
          (b"", 3),
          (b"x", 3),
          (b"a\r\nb\r\n" * 8, 1),
          (_text(rng, 5000), 3),  # spans tiles
          (_text(rng, 70), 0)]
    cur = sum(len(b) for b, _ in fk)
    fk.append((_text(rng, (-cur) % 1024 or 1024), 0))
    fk += [(b"q" * 300, 3),  # starts exactly at a 1-KiB tile's first byte
           (_text(rng, 3 * 1024 + 500), 0),  # identity tiles, then mid-tile:
           (b"d" * 40, 3),  # alone inside an otherwise identity tile
           (_text(rng, 2 * 1024 + 100), 0),
           (b"\x00\x01printable-to-the-end", 2),  # its run touches the dropped file's first byte
           (b"DROPPED-but-printable" * 2, 3),
           (b"printable-from-the-start\x00\x02tail5", 2),
           (b"\x00abcd", 2),  # 4 + 4 + 4 printable bytes across the three files: no run of 5 in any
           (b"efgh", 3),
           (b"ijkl\x00", 2),
           (b"a\r\nb\r\n" * 10, 3),  # CRs in a dropped file
           (_text(rng, 33), 1)]
    alpha = [b"a", b"Z", b" ", b"\x00", b"\x07", b"\r", b"\n", b"\xa0", b"\xa1", b"\x7f", b"pqrst", b"uvwxyz12"]
    for _ in range(1500):
        n = rng.choice([0, 0, 1, 5, 16, 17, 100, 1000, 1023, 1024, 1025, 3000])
        b = b"".join(rng.choice(alpha) for _ in range(n))[:n]
        fk.append((b, rng.choice([0, 1, 2, 3, 3])))
    fk.append((b"last-drop" * 7, 3))  # last in the batch
    return [b for b, _ in fk], [k for _, k in fk]


@pytest.fixture(scope="module")
def drop_case():
    files, kinds = _drop_files()
    want = [b if k == 0 else b.replace(b"\r", b"") if k == 1 else oan.extract_printable_bytes(b) if k == 2 else b""
            for b, k in zip(files, kinds)]
    return files, kinds, want


@pytest.mark.parametrize("mode", ["narrow", "wide", "onepass"])
def test_kind3_drops_the_file(drop_case, mode, monkeypatch):
    """Kinds 0-3 mixed: a kind-3 file's output is empty, every other file's equals the oracle's
    transform.  wide: the 64-bit-position kernels (TSG_XFORM_WIDE=1); onepass: xf_onepass_kernel."""
    from trivy_amd import _lib
    if mode == "wide":
        monkeypatch.setenv("TSG_XFORM_WIDE", "1")
    elif mode == "onepass":
        monkeypatch.setenv("TSG_XFORM_ONEPASS", "1")
    files, kinds, want = drop_case
    assert kinds[0] == 3 and kinds[-1] == 3
    L = _lib.lib()
    L.tsg_debug_xform.argtypes = [c.c_int, c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint32, c.c_void_p, c.c_void_p,
                                  c.c_uint64, c.c_void_p]
    offs = _offsets(files)
    assert any(k == 3 and int(o) % 1024 == 0 and o > 0 for k, o in zip(kinds, offs))
    raw = np.frombuffer(b"".join(files) + b"\0" * 64, dtype=np.uint8)
    kd = np.array(kinds, dtype=np.uint8)
    out = np.zeros(int(offs[-1]) * 2 + 64, dtype=np.uint8)
    xoff = np.zeros(len(files) + 1, dtype=np.uint64)
    rc = L.tsg_debug_xform(0, raw.ctypes.data, int(offs[-1]), offs.ctypes.data, len(files), kd.ctypes.data,
                           out.ctypes.data, len(out), xoff.ctypes.data)
    assert rc == 0, _lib.last_error(L)
    for i, w in enumerate(want):
        got = out[int(xoff[i]):int(xoff[i + 1])].tobytes()
        assert got == w, (i, kinds[i], files[i][:60])
    assert int(xoff[-1]) == sum(map(len, want))
    assert not out[int(xoff[-1]):].any()  # nothing written past the end


# ---- 3-6. the analyzer -----------------------------------------------------
@pytest.fixture(scope="module")
def analyzer():
    from trivy_amd.analyzer import AnalyzerOptions, SecretAnalyzer
    a = SecretAnalyzer()
    a.Init(AnalyzerOptions())
    return a


@pytest.fixture(scope="module")
def oracle():
    return oan.SecretAnalyzer("")


def _resident(files):
    import torch
    contents = [b for _, b in files]
    offs = _offsets(contents)
    arena = np.frombuffer(b"".join(contents) + b"\0" * 64, dtype=np.uint8).copy()
    return torch.from_numpy(arena).to("cuda:0"), offs, [p for p, _ in files]


def _reference(oracle, files, dir_):
    """Per file what AnalyzeFile gives: None when Required refuses it, else the oracle's analyze."""
    return [oracle.analyze(p, dir_, b) if oracle.required(p, len(b)) else None for p, b in files]


def _same(got, want, files):
    assert len(got) == len(want) == len(files)
    for (p, _), g, w in zip(files, got, want):
        if w is None:
            assert g is None, p
        else:
            assert g is not None and [s.to_dict() for s in g.Secrets] == w["Secrets"], p


def _analyze_files():
    body = b"# settings\nname = demo\n"
    late_nul = b"k = " + AWS + b"\n" + b"x" * 300 + b"\x00 and more text\n"
    assert late_nul.index(b"\x00") >= 300
    return [("etc/plain.conf", body + b"key = " + AWS + b"\nend\n"),
            ("etc/crlf.ini", b"[main]\r\ntoken = " + GH + b"\r\nmore = 1\r\n" * 4),
            ("lib/mod.pyc", b"\x03\xf3\r\n\x00\x00\x00\x00abcd\x00hello world k=" + AWS + b"\x00" + b"y" * 40 +
             b"\x01tail"),
            ("bin/blob.dat", b"heads\x00\x01 key = " + AWS + b"\n" + b"z" * 60),  # NUL at byte 5: binary, not .pyc
            ("var/late_nul.txt", late_nul),
            ("node_modules/x.js", b"var t = '" + GH + b"';\n"),
            ("img/a.png", b"not really a png: " + AWS + b"\n"),
            ("go.sum", b"example.com/m v1.0.0 h1:" + AWS + b"=\n"),
            ("tiny.txt", b"123456789"),
            ("etc/clean.txt", b"nothing to see here\n" * 5)]


@pytest.mark.parametrize("dir_", ["", "/src"])
def test_analyze_device_end_to_end(analyzer, oracle, dir_):
    from trivy_amd.analyzer import AnalysisInput, FileInfo
    files = _analyze_files()
    assert files[3][1][5] == 0 and len(files[8][1]) == 9
    d_arena, offs, paths = _resident(files)
    pend = analyzer.AnalyzeDeviceAsync(d_arena, offs, paths, dir_)
    got = pend.wait()
    want = _reference(oracle, files, dir_)
    _same(got, want, files)
    # the same bytes held on the host, through the collector (Required applied first, as AnalyzeFile does)
    req = [i for i, (p, b) in enumerate(files) if analyzer.Required(p, FileInfo(len(b)))]
    batch = analyzer.AnalyzeBatch([AnalysisInput(dir_, files[i][0], FileInfo(len(files[i][1])), files[i][1])
                                   for i in req])
    host = [None] * len(files)
    for i, r in zip(req, batch):
        host[i] = r
    for (p, _), g, h in zip(files, got, host):
        assert (g is None) == (h is None), p
        if g is not None:
            assert [s.to_dict() for s in g.Secrets] == [s.to_dict() for s in h.Secrets], p
    found = {p for (p, _), g in zip(files, got) if g is not None}
    assert found == {"etc/plain.conf", "etc/crlf.ini", "lib/mod.pyc", "var/late_nul.txt"}
    prefix = "/" if dir_ == "" else ""
    assert got[0].Secrets[0].FilePath == prefix + "etc/plain.conf"
    pyc = got[2].Secrets[0]
    assert pyc.Findings and all(f.Code.Lines is None for f in pyc.Findings)  # Binary: Code without lines
    # fetched for the exact pass: the two candidate files the transform left as read -- not the
    # dropped blob (its token never became a candidate), not the transformed ones (gathered)
    fs = pend.result.fetch_stats()
    assert fs["files"] == 2 and fs["bytes"] == len(files[0][1]) + len(files[4][1])
    assert all(r["kind"] == 0 for r, g in zip(pend.result.raw(), got) if g is None)


def test_nothing_survives(analyzer, oracle):
    files = [("a.png", b"png " + AWS + b"\n"),
             ("bin/tool", b"\x7fELF\x00\x01 " + AWS + b"\n" + b"q" * 2000),
             ("x/node_modules/y/z.js", b"t = '" + GH + b"'\n"),
             ("short", b"k=" + b"1" * 5),
             ("go.sum", b"h1:" + AWS + b"\n"),
             ("empty.txt", b"")]
    d_arena, offs, paths = _resident(files)
    kinds, binary = analyzer.ClassifyDevice(d_arena, offs, paths)
    assert kinds.tolist() == [3] * len(files) and binary.tolist() == [0] * len(files)
    pend = analyzer.AnalyzeDeviceAsync(d_arena, offs, paths)
    got = pend.wait()
    assert got == [None] * len(files)
    assert _reference(oracle, files, "") == [None] * len(files)
    fs = pend.result.fetch_stats()
    assert fs["files"] == 0 and fs["bytes"] == 0
    assert pend.result.stats()["candidates"] == 0


def test_two_in_flight_waited_in_reverse(analyzer, oracle):
    rng = random.Random(9)
    a = _analyze_files()
    b = [("srv/%02d.env" % i, b"n = %d\n" % i + (b"pw = " + GH + b"\r\n" if i % 3 else b"\x00\x00") +
          bytes(rng.choice(b"xyz =\n") for _ in range(rng.randint(20, 3000)))) for i in range(40)]
    ra, rb = _resident(a), _resident(b)
    sync_a = analyzer.AnalyzeDevice(*ra)
    sync_b = analyzer.AnalyzeDevice(*rb, dir_="/srv")
    pa = analyzer.AnalyzeDeviceAsync(*ra)
    pb = analyzer.AnalyzeDeviceAsync(*rb, dir_="/srv")
    got_b = pb.wait()
    got_a = pa.wait()
    assert got_a == sync_a and got_b == sync_b
    _same(got_a, _reference(oracle, a, ""), a)
    _same(got_b, _reference(oracle, b, "/srv"), b)
    assert any(g is None for g in got_b) and sum(g is not None for g in got_b) >= 10


def test_classify_device_vs_collector(analyzer):
    """The kinds and binary flags equal what a Collector(gpu_transform=True) records for the same
    files added from host bytes (kind 2 and Binary for a binary .pyc, else kind 1); a file the
    collector skips, or that Required refuses, is kind 3."""
    from tests.corpus import make_corpus
    from trivy_amd.analyzer import Collector, FileInfo
    from trivy_amd.analyzer.secret import TSG_SKIPPED
    rng = random.Random(13)
    files = []
    for i, (p, b) in enumerate(make_corpus(77, 160)):
        r = i % 8
        if r == 0:
            b = b[:rng.randint(0, 299)] + b"\x00" + b  # a bad byte somewhere in the head
        elif r == 1:
            p, b = p + ".pyc", b"\x01\x02" + b
        elif r == 2:
            p = p + ".pyc"  # a .pyc that is text
        elif r == 3:
            b = b"t" * 300 + b"\x00" + b  # the first bad byte is byte 300
        elif r == 4:
            p = "node_modules/" + p
        elif r == 5:
            b = b[:9]
        files.append((p, b))
    files += _analyze_files()
    d_arena, offs, paths = _resident(files)
    st = {}
    kinds, binary = analyzer.ClassifyDevice(d_arena, offs, paths, stats=st)
    coll = Collector(analyzer, gpu_transform=True)
    want_k, want_b = [], []
    for p, b in files:
        r = coll.add(p, "", b)
        assert r >= 0 or r == TSG_SKIPPED
        if r >= 0:
            bn = coll.file(r)[2]
        if r == TSG_SKIPPED or not analyzer.Required(p, FileInfo(len(b))):
            want_k.append(3)
            want_b.append(0)
        else:
            want_k.append(2 if bn else 1)
            want_b.append(1 if bn else 0)
    assert kinds.tolist() == want_k and binary.tolist() == want_b
    assert {1, 2, 3} <= set(want_k)
    assert st["files"] == len(files) and st["pyc"] == want_k.count(2)
    assert st["required"] == sum(1 for p, b in files if analyzer.Required(p, FileInfo(len(b))))
    assert st["required"] - st["skipped_binary"] == len(files) - want_k.count(3)
    assert st["ms_kernel"] >= 0 and st["ms_total"] > 0 and st["ms_total"] >= st["ms_kernel"]
