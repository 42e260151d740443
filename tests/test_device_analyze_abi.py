"""Analyze for HBM-resident files (tsg_analyzer_classify_device / tsg_analyzer_submit_device), the
parts that need no GPU.

* tsg_device_files and tsg_device_classify_stats are laid out as the C compiler lays them out, and
  the ctypes mirrors agree;
* the symbols exist in the library;
* every argument error comes back as <0 with a text before anything else is looked at -- from an
  analyzer whose scanner has no GPU engine (the oracle's library holds the product's host objects),
  where valid arguments stop at "no GPU engine" instead.
"""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import hostlib
from trivy_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
FAKE_DEV = 0x7000_0000_0000  # 16-B aligned, never dereferenced: an analyzer without an engine stops first


def _probe(tmp_path, body):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "tsg_analyzer.h"\nint main(void){' + body + ' return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    return [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]


def test_device_files_layout(tmp_path):
    from trivy_amd.analyzer.secret import _CDeviceFiles, DEVICE_FILES_SIZE_V1
    names = ["struct_size", "n_files", "dev_arena", "host_offsets", "dev_offsets", "paths", "path_lens", "dir"]
    got = _probe(tmp_path, 'printf("%zu %u", sizeof(tsg_device_files), (unsigned)TSG_DEVICE_FILES_SIZE_V1);'
                 + "".join('printf(" %%zu", offsetof(tsg_device_files, %s));' % n for n in names))
    assert got[0] == ctypes.sizeof(_CDeviceFiles) == 56 == got[1] == DEVICE_FILES_SIZE_V1
    assert got[2:] == [0, 4, 8, 16, 24, 32, 40, 48]
    for name, off in zip(names, got[2:]):
        assert getattr(_CDeviceFiles, name).offset == off, name


def test_classify_stats_layout(tmp_path):
    from trivy_amd.analyzer.secret import _CDeviceClassifyStats, DEVICE_CLASSIFY_STATS_SIZE_V1
    names = ["struct_size", "reserved", "files", "required", "skipped_binary", "pyc", "ms_kernel", "ms_total"]
    got = _probe(tmp_path, 'printf("%zu %u", sizeof(tsg_device_classify_stats),'
                 ' (unsigned)TSG_DEVICE_CLASSIFY_STATS_SIZE_V1);'
                 + "".join('printf(" %%zu", offsetof(tsg_device_classify_stats, %s));' % n for n in names))
    assert got[0] == ctypes.sizeof(_CDeviceClassifyStats) == 56 == got[1] == DEVICE_CLASSIFY_STATS_SIZE_V1
    assert got[2:] == [0, 4, 8, 16, 24, 32, 40, 48]
    for name, off in zip(names, got[2:]):
        assert getattr(_CDeviceClassifyStats, name).offset == off, name


def test_symbols_exist():
    L = _lib.lib()
    for name in ("tsg_analyzer_classify_device", "tsg_analyzer_submit_device", "tsg_debug_classify",
                 "tsg_debug_engine_stages", "tsg_debug_rule_gate_implied"):
        assert hasattr(L, name), name
    from trivy_amd import analyzer
    for name in ("ClassifyDevice", "AnalyzeDevice", "AnalyzeDeviceAsync"):
        assert callable(getattr(analyzer.SecretAnalyzer, name)), name
    assert analyzer.XFORM_DROP == 3 and analyzer.PendingDeviceAnalyze


@pytest.fixture(scope="module")
def host_analyzer():
    from trivy_amd.analyzer import SecretAnalyzer
    from trivy_amd.secret import NewScanner
    L = hostlib.lib()
    return SecretAnalyzer(NewScanner(None, lib=L, host_only=True), lib=L, host_only=True)


def _files(n=2, **over):
    from trivy_amd.analyzer.secret import _CDeviceFiles, DEVICE_FILES_SIZE_V1
    offs = np.array([0, 20, 40][:n + 1], dtype=np.uint64)
    paths = (ctypes.c_char_p * n)(*[b"a.txt", b"b.txt"][:n])
    vals = dict(struct_size=DEVICE_FILES_SIZE_V1, n_files=n, dev_arena=FAKE_DEV, host_offsets=offs.ctypes.data,
                dev_offsets=None, paths=ctypes.cast(paths, ctypes.c_void_p).value, path_lens=None, dir=b"")
    vals.update(over)
    return _CDeviceFiles(**vals), (offs, paths)


def test_argument_errors_come_before_the_gpu(host_analyzer):
    from trivy_amd.analyzer.secret import (_CDeviceClassifyStats, DEVICE_CLASSIFY_STATS_SIZE_V1,
                                           DEVICE_FILES_SIZE_V1)
    L, a = host_analyzer._L, host_analyzer._h
    kinds = np.full(2, 0xAA, np.uint8)
    binary = np.full(2, 0xAA, np.uint8)

    def both(f):
        """(rc, text) of the two entry points on f; they must agree on the error."""
        rc1 = L.tsg_analyzer_classify_device(a, ctypes.byref(f), kinds.ctypes.data, binary.ctypes.data, None)
        t1 = _lib.last_error(L)
        h = ctypes.c_void_p()
        rc2 = L.tsg_analyzer_submit_device(a, ctypes.byref(f), ctypes.byref(h))
        t2 = _lib.last_error(L)
        assert not h.value  # no pending object on an error
        assert (kinds == 0xAA).all() and (binary == 0xAA).all()  # nothing written
        return (rc1, t1), (rc2, t2)

    for bogus in (0, 8, DEVICE_FILES_SIZE_V1 - 8, DEVICE_FILES_SIZE_V1 + 8, 0xFFFFFFFF):
        f, keep = _files(struct_size=bogus)
        for rc, text in both(f):
            assert rc < 0 and "struct_size %d" % bogus in text and "engine" not in text

    for field, what in (("dev_arena", "dev_arena is NULL"), ("host_offsets", "host_offsets is required"),
                        ("paths", "paths is NULL")):
        f, keep = _files(**{field: None})
        for rc, text in both(f):
            assert rc < 0 and what in text and "engine" not in text, (field, text)

    for ptr in (FAKE_DEV + 1, FAKE_DEV + 8, FAKE_DEV + 15):
        f, keep = _files(dev_arena=ptr)
        for rc, text in both(f):
            assert rc < 0 and "16-B aligned" in text and "engine" not in text

    for bad in ([1, 20, 40], [0, 30, 20], [0, 20, 19]):
        offs = np.array(bad, dtype=np.uint64)
        f, keep = _files(host_offsets=offs.ctypes.data)
        for rc, text in both(f):
            assert rc < 0 and "ascend from 0" in text and "engine" not in text, (bad, text)

    # a stats struct of an unknown size is refused too
    f, keep = _files()
    st = _CDeviceClassifyStats()
    st.struct_size = DEVICE_CLASSIFY_STATS_SIZE_V1 + 8
    st.files = 7
    assert L.tsg_analyzer_classify_device(a, ctypes.byref(f), kinds.ctypes.data, binary.ctypes.data,
                                          ctypes.byref(st)) < 0
    assert "tsg_device_classify_stats.struct_size" in _lib.last_error(L) and st.files == 7

    # valid arguments pass the checks and stop at the missing engine
    for rc, text in both(f):
        assert rc < 0 and "no GPU engine" in text, text
    # an empty batch reads nothing: no GPU work, no error
    f, keep = _files(n=0)
    assert L.tsg_analyzer_classify_device(a, ctypes.byref(f), None, None, None) == 0


def test_python_checks_come_first(host_analyzer):
    """The arena contract is checked by Scanner._device_batch before the library is called."""
    offs = np.array([0, 20, 40], dtype=np.uint64)
    with pytest.raises(ValueError, match="16-B aligned"):
        host_analyzer.ClassifyDevice(FAKE_DEV + 4, offs, ["a", "b"], nbytes=1 << 20)
    with pytest.raises(ValueError, match="nbytes"):
        host_analyzer.AnalyzeDevice(FAKE_DEV, offs, ["a", "b"])
    with pytest.raises(ValueError, match=r"offsets\[-1\] \+ 64"):
        host_analyzer.AnalyzeDevice(FAKE_DEV, offs, ["a", "b"], nbytes=100)
    with pytest.raises(ValueError, match="ascending"):
        host_analyzer.AnalyzeDevice(FAKE_DEV, offs[::-1].copy(), ["a", "b"], nbytes=1 << 20)
    with pytest.raises(ValueError, match="1 paths for 2 files"):
        host_analyzer.AnalyzeDevice(FAKE_DEV, offs, ["a"], nbytes=1 << 20, dev_offsets=FAKE_DEV)
