"""The split scan's C-ABI (tsg_scanner_set_resident_transform, tsg_result_split_stats), the parts
that need no GPU.

* tsg_split_stats is laid out as the C compiler lays it out, and the ctypes mirror agrees;
* tsg_result_split_stats refuses a struct_size it does not know before it reads the result;
* a mode that does not exist is refused with a text, the getter round-trips, and
  TSG_RESIDENT_TRANSFORM=split sets the initial mode -- on a scanner without a GPU engine (the
  oracle's library holds the product's host objects).
"""
import ctypes
import subprocess
from pathlib import Path

import pytest

from oracle import hostlib
from trivy_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
FIELDS = ("struct_size", "mode_used", "files_in_place", "bytes_in_place", "files_changed", "bytes_changed",
          "files_dropped", "bytes_dropped", "ms_census", "ms_sub")


def test_split_stats_layout(tmp_path):
    from trivy_amd.secret.scanner import _CSplitStats, SPLIT_STATS_SIZE_V1
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "tsg_scanner.h"\nint main(void){printf("%zu %u %u %u", '
                   'sizeof(tsg_split_stats), (unsigned)TSG_SPLIT_STATS_SIZE_V1, (unsigned)TSG_RESIDENT_CHUNKED, '
                   '(unsigned)TSG_RESIDENT_SPLIT);' +
                   "".join('printf(" %%zu", offsetof(tsg_split_stats, %s));' % f for f in FIELDS) +
                   'printf("\\n"); return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    size, v1, chunked, split = out[:4]
    assert size == ctypes.sizeof(_CSplitStats) == 72 == v1 == SPLIT_STATS_SIZE_V1
    assert (chunked, split) == (0, 1)
    assert out[4:] == [0, 4, 8, 16, 24, 32, 40, 48, 56, 64]
    assert [n for n, _ in _CSplitStats._fields_] == list(FIELDS)
    for name, off in zip(FIELDS, out[4:]):
        assert getattr(_CSplitStats, name).offset == off, name


def test_split_stats_refuses_unknown_struct_size():
    """The size check comes before the result is read: no scan (and no GPU) is needed."""
    from trivy_amd.secret.scanner import _CSplitStats, _declare, SPLIT_STATS_SIZE_V1
    L = _lib.lib()
    _declare(L)
    dummy = ctypes.create_string_buffer(4096)  # (never read: every size below is refused)
    for bogus in (0, 8, SPLIT_STATS_SIZE_V1 - 8, SPLIT_STATS_SIZE_V1 + 8, 0xFFFFFFFF):
        s = _CSplitStats()
        s.struct_size = bogus
        s.files_changed = 7
        assert L.tsg_result_split_stats(ctypes.cast(dummy, ctypes.c_void_p), ctypes.byref(s)) < 0
        assert "struct_size %d" % bogus in _lib.last_error(L)
        assert s.files_changed == 7 and s.mode_used == 0  # nothing written
    s = _CSplitStats()
    s.struct_size = SPLIT_STATS_SIZE_V1
    assert L.tsg_result_split_stats(None, ctypes.byref(s)) < 0
    assert L.tsg_result_split_stats(ctypes.cast(dummy, ctypes.c_void_p), None) < 0


@pytest.fixture()
def host_scanner():
    from trivy_amd.secret import NewScanner
    return NewScanner(None, lib=hostlib.lib(), host_only=True)


def test_mode_round_trips_and_a_bad_mode_is_refused(host_scanner):
    s, L = host_scanner, host_scanner._L
    assert s.resident_transform() == "chunked"  # the default
    s.set_resident_transform("split")
    assert s.resident_transform() == "split"
    for bad in (2, 3, 0xFFFFFFFF):
        assert L.tsg_scanner_set_resident_transform(s._h, bad) < 0
        assert "mode %d" % bad in _lib.last_error(L) and "chunked" in _lib.last_error(L)
        assert s.resident_transform() == "split"  # unchanged
    s.set_resident_transform("chunked")
    assert s.resident_transform() == "chunked"
    with pytest.raises(ValueError):
        s.set_resident_transform("windows")
    m = ctypes.c_uint32(9)
    assert L.tsg_scanner_set_resident_transform(None, 1) < 0
    assert L.tsg_scanner_get_resident_transform(None, ctypes.byref(m)) < 0 and m.value == 9
    assert L.tsg_scanner_get_resident_transform(s._h, None) < 0


def test_env_sets_the_initial_mode(monkeypatch):
    from trivy_amd.secret import NewScanner
    monkeypatch.setenv("TSG_RESIDENT_TRANSFORM", "split")
    assert NewScanner(None, lib=hostlib.lib(), host_only=True).resident_transform() == "split"
    monkeypatch.setenv("TSG_RESIDENT_TRANSFORM", "chunked")
    assert NewScanner(None, lib=hostlib.lib(), host_only=True).resident_transform() == "chunked"
    monkeypatch.delenv("TSG_RESIDENT_TRANSFORM")
    assert NewScanner(None, lib=hostlib.lib(), host_only=True).resident_transform() == "chunked"
