"""Device-only batches (tsg_batch.host_arena NULL), the parts that need no GPU.

* tsg_fetch_stats is laid out as the C compiler lays it out, and the ctypes mirror agrees;
* tsg_result_fetch_stats refuses a struct_size it does not know;
* the argument errors of a batch come back as <0 with a text before anything else is looked
  at -- from a scanner without a GPU engine (the oracle's library holds the product's host
  objects), whose valid batches fail with "no GPU engine" instead.
"""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import hostlib
from trivy_amd import _lib

ROOT = Path(__file__).resolve().parent.parent


def test_fetch_stats_layout(tmp_path):
    from trivy_amd.secret.scanner import _CFetchStats, FETCH_STATS_SIZE_V1
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "tsg_scanner.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %u\\n",'
                   ' sizeof(tsg_fetch_stats), offsetof(tsg_fetch_stats, struct_size), offsetof(tsg_fetch_stats, rounds),'
                   ' offsetof(tsg_fetch_stats, files), offsetof(tsg_fetch_stats, bytes),'
                   ' offsetof(tsg_fetch_stats, direct_files), offsetof(tsg_fetch_stats, ms_fetch),'
                   ' (unsigned)TSG_FETCH_STATS_SIZE_V1); return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    size, o_ss, o_r, o_f, o_b, o_d, o_ms, v1 = [
        int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert size == ctypes.sizeof(_CFetchStats) == 40 == v1 == FETCH_STATS_SIZE_V1
    assert (o_ss, o_r, o_f, o_b, o_d, o_ms) == (0, 4, 8, 16, 24, 32)
    for name, off in (("struct_size", o_ss), ("rounds", o_r), ("files", o_f), ("bytes", o_b),
                      ("direct_files", o_d), ("ms_fetch", o_ms)):
        assert getattr(_CFetchStats, name).offset == off, name


def test_fetch_stats_refuses_unknown_struct_size():
    """The size check comes before the result is read: no scan (and no GPU) is needed."""
    from trivy_amd.secret.scanner import _CFetchStats, _declare, FETCH_STATS_SIZE_V1
    L = _lib.lib()
    _declare(L)
    dummy = ctypes.create_string_buffer(4096)  # (never read: every size below is refused)
    for bogus in (0, 8, FETCH_STATS_SIZE_V1 - 8, FETCH_STATS_SIZE_V1 + 8, 0xFFFFFFFF):
        s = _CFetchStats()
        s.struct_size = bogus
        s.files = 7
        assert L.tsg_result_fetch_stats(ctypes.cast(dummy, ctypes.c_void_p), ctypes.byref(s)) < 0
        assert "struct_size %d" % bogus in _lib.last_error(L)
        assert s.files == 7  # nothing written
    s = _CFetchStats()
    s.struct_size = FETCH_STATS_SIZE_V1
    assert L.tsg_result_fetch_stats(None, ctypes.byref(s)) < 0


@pytest.fixture(scope="module")
def host_scanner():
    from trivy_amd.secret import NewScanner
    return NewScanner(None, lib=hostlib.lib(), host_only=True)


def _batch(host_arena, dev_arena, n=2):
    from trivy_amd.secret.scanner import _CBatch
    offs = np.array([0, 8, 16][:n + 1], dtype=np.uint64)
    paths = (ctypes.c_char_p * n)(*[b"a.txt", b"b.txt"][:n])
    b = _CBatch(n, host_arena, offs.ctypes.data, dev_arena, None, ctypes.cast(paths, ctypes.c_void_p).value,
                None, None, None, None, None)
    return b, (offs, paths)


def test_argument_errors_come_before_the_engine(host_scanner):
    from trivy_amd.secret.scanner import _CBatchExt, BATCH_EXT_SIZE_V2
    L = host_scanner._L
    arena = np.zeros(64, np.uint8)
    kinds = np.zeros(2, np.uint8)
    gsrc = np.zeros(2, np.uint64)
    FAKE_DEV = 0x7000_0000_0000  # never dereferenced: a scanner without an engine stops first

    def scan(b):
        h = ctypes.c_void_p()
        rc = L.tsg_scan(host_scanner._h, ctypes.byref(b), ctypes.byref(h))
        assert not h.value
        return rc, _lib.last_error(L)

    def scan_ext(e):
        h = ctypes.c_void_p()
        rc = L.tsg_scan_ext(host_scanner._h, ctypes.byref(e), ctypes.byref(h))
        assert not h.value
        return rc, _lib.last_error(L)

    # host_arena NULL with no dev_arena and no gather_base
    b, keep = _batch(None, None)
    rc, text = scan(b)
    assert rc < 0 and "host_arena is NULL" in text and "engine" not in text
    e = _CBatchExt(BATCH_EXT_SIZE_V2, b, None, None, None, None)
    rc, text = scan_ext(e)
    assert rc < 0 and "host_arena is NULL" in text
    h = ctypes.c_void_p()
    assert L.tsg_scan_submit(host_scanner._h, ctypes.byref(b), ctypes.byref(h)) < 0 and not h.value
    assert "host_arena is NULL" in _lib.last_error(L)
    assert L.tsg_scan_submit_ext(host_scanner._h, ctypes.byref(e), ctypes.byref(h)) < 0 and not h.value
    assert "host_arena is NULL" in _lib.last_error(L)

    # gather_base together with dev_arena
    b, keep2 = _batch(None, FAKE_DEV)
    b.transform = kinds.ctypes.data
    e = _CBatchExt(BATCH_EXT_SIZE_V2, b, None, None, arena.ctypes.data, gsrc.ctypes.data)
    rc, text = scan_ext(e)
    assert rc < 0 and "gathered batch" in text and "no dev_arena" in text

    # host_offsets missing
    b, keep3 = _batch(arena.ctypes.data, None)
    b.host_offsets = None
    rc, text = scan(b)
    assert rc < 0 and "host_offsets is required" in text

    # valid batches pass the checks and stop at the missing engine: mirrored, device-only,
    # device-only with a transform (no longer "must be host-resident")
    for host, dev, xf in ((arena.ctypes.data, None, None), (arena.ctypes.data, FAKE_DEV, None),
                          (None, FAKE_DEV, None), (None, FAKE_DEV, kinds.ctypes.data)):
        b, keep4 = _batch(host, dev)
        b.transform = xf
        rc, text = scan(b)
        assert rc < 0 and "no GPU engine" in text, text
