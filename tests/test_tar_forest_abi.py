"""All layers of an image resident in HBM, the part that needs no GPU (include/tsg_analyzer.h:
tsg_analyzer_index_device_tars; trivy_amd/analyzer/secret.py: layer_groups).

* every argument error comes back before any GPU work (-1, its own text, a layer's with the layer's number),
  on an analyzer whose scanner has no GPU engine, and leaves out[] all NULL;
* the versioned structs are laid out as the C compiler lays them out;
* the grouping of AnalyzeLayersDevice is a pure function: order kept, base layers left out, an oversized
  layer alone, group_bytes respected;
* the virtual block space of the model (tests/tar_forest_model.py).
"""
import ctypes as c
import subprocess
from pathlib import Path

import pytest

from oracle import hostlib
from tests import tar_forest_model as fm

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def an():
    from trivy_amd.analyzer import AnalyzerOptions, SecretAnalyzer
    from trivy_amd.analyzer.secret import _declare
    a = SecretAnalyzer(lib=hostlib.lib(), host_only=True)
    a.Init(AnalyzerOptions())
    _declare(a._L)
    return a


def _err(a):
    from trivy_amd import _lib
    return _lib.last_error(a._L)


def test_struct_layouts(tmp_path):
    from trivy_amd.analyzer.secret import (DEVICE_TARS_MAX_LAYERS, DEVICE_TARS_SIZE_V1, TAR_FOREST_STATS_SIZE_V1,
                                           _CDeviceTars, _CTarForestStats)
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "tsg_analyzer.h"\nint main(void){printf("%zu %u %zu %zu %zu %u %zu %zu %zu %zu %u\\n",'
                   ' sizeof(tsg_device_tars), (unsigned)TSG_DEVICE_TARS_SIZE_V1, offsetof(tsg_device_tars, n_layers),'
                   ' offsetof(tsg_device_tars, layers), sizeof(tsg_tar_forest_stats),'
                   ' (unsigned)TSG_TAR_FOREST_STATS_SIZE_V1, offsetof(tsg_tar_forest_stats, layers),'
                   ' offsetof(tsg_tar_forest_stats, device_bytes), offsetof(tsg_tar_forest_stats, ms_candidates),'
                   ' offsetof(tsg_tar_forest_stats, ms_total), (unsigned)TSG_DEVICE_TARS_MAX_LAYERS); return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    (size_t, v1_t, off_n, off_l, size_f, v1_f, off_layers, off_dev, off_ms0, off_ms1, max_layers) = \
        [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert size_t == v1_t == c.sizeof(_CDeviceTars) == DEVICE_TARS_SIZE_V1 == 16
    assert off_n == _CDeviceTars.n_layers.offset == 4 and off_l == _CDeviceTars.layers.offset == 8
    assert size_f == v1_f == c.sizeof(_CTarForestStats) == TAR_FOREST_STATS_SIZE_V1 == 8 + 7 * 8 + 7 * 8
    assert off_layers == _CTarForestStats.layers.offset == 8 and off_dev == _CTarForestStats.device_bytes.offset == 56
    assert off_ms0 == _CTarForestStats.ms_candidates.offset == 64 and off_ms1 == _CTarForestStats.ms_total.offset == 112
    assert max_layers == DEVICE_TARS_MAX_LAYERS == 65536


def test_argument_errors_come_before_any_gpu_work(an):
    from trivy_amd.analyzer.secret import (DEVICE_TAR_SIZE_V1, DEVICE_TAR_STATS_SIZE_V1, DEVICE_TARS_SIZE_V1,
                                           TAR_FOREST_STATS_SIZE_V1, _CDeviceTar, _CDeviceTars, _CDeviceTarStats,
                                           _CTarForestStats)
    L = an._L
    fake = 0x700000000000  # never dereferenced
    who = "tsg_analyzer_index_device_tars"

    def good():
        return [_CDeviceTar(DEVICE_TAR_SIZE_V1, 0, fake + 4096 * k, 4096) for k in range(3)]

    def index(layers, n=None, size=DEVICE_TARS_SIZE_V1, st=None, fs=None, out=True, a=an._h, null_t=False):
        arr = (_CDeviceTar * max(1, len(layers)))(*layers) if layers is not None else None
        t = _CDeviceTars(size, len(layers) if n is None else n, arr)
        slots = 16  # (more than any n_layers that passes the checks here)
        hs = (c.c_void_p * slots)(*([1] * slots))
        bad = c.c_uint32(77)
        rc = L.tsg_analyzer_index_device_tars(a, None if null_t else c.byref(t), hs if out else None, st,
                                              c.byref(fs) if fs is not None else None, c.byref(bad))
        text = _err(an)
        if out and a is not None and not null_t and size == DEVICE_TARS_SIZE_V1 and 0 < t.n_layers <= slots:
            assert not any(hs[:t.n_layers])  # out[] is all NULL after any error past the header checks
        return rc, text

    # NULLs
    for kw in ({"a": None}, {"null_t": True}, {"out": False}):
        rc, text = index(good(), **kw)
        assert rc == -1 and text.startswith(who + ": NULL")
    rc, text = index(None, n=2)
    assert rc == -1 and "layers is NULL" in text
    # the struct sizes
    for bogus in (0, 8, DEVICE_TARS_SIZE_V1 - 8, DEVICE_TARS_SIZE_V1 + 8, 0xFFFFFFFF):
        rc, text = index(good(), size=bogus)
        assert rc == -1 and "tsg_device_tars.struct_size %d" % bogus in text
    fs = _CTarForestStats()
    fs.struct_size = TAR_FOREST_STATS_SIZE_V1 - 8
    rc, text = index(good(), fs=fs)
    assert rc == -1 and "tsg_tar_forest_stats.struct_size" in text
    # the layer count
    for n in (0, 65537, 0xFFFFFFFF):
        rc, text = index(good(), n=n)
        assert rc == -1 and "n_layers %d" % n in text
    # per layer: the single-layer call's texts, the layer's number first
    for k in range(3):
        pre = "%s: layer %d: " % (who, k)
        for bogus in (0, DEVICE_TAR_SIZE_V1 + 8):
            ly = good()
            ly[k].struct_size = bogus
            rc, text = index(ly)
            assert rc == -1 and text.startswith(pre + "tsg_device_tar.struct_size %d" % bogus)
        ly = good()
        ly[k].dev_tar = None
        rc, text = index(ly)
        assert rc == -1 and text.startswith(pre + "dev_tar is NULL")
        for mis in (1, 8, 15):
            ly = good()
            ly[k].dev_tar = fake + mis
            rc, text = index(ly)
            assert rc == -1 and text == pre + "dev_tar must be 16-B aligned"
        ly = good()
        ly[k].n_bytes = 512 << 32
        rc, text = index(ly)
        assert rc == -1 and text.startswith(pre) and "2^32" in text
        st = (_CDeviceTarStats * 3)()
        for x in st:
            x.struct_size = DEVICE_TAR_STATS_SIZE_V1
        st[k].struct_size += 8
        rc, text = index(good(), st=st)
        assert rc == -1 and text.startswith(pre + "tsg_device_tar_stats.struct_size")
    # the lowest layer's error is the one reported
    ly = good()
    ly[1].dev_tar = fake + 8
    ly[2].dev_tar = None
    assert index(ly)[1].startswith(who + ": layer 1: ")
    # valid arguments stop at the scanner's missing engine, in both walk modes
    fs.struct_size = TAR_FOREST_STATS_SIZE_V1
    for mode in ("host", "gpu"):
        an.set_tar_walk(mode)
        try:
            rc, text = index(good(), fs=fs)
        finally:
            an.set_tar_walk("host")
        assert rc == -2 and "no GPU engine" in text, mode


def test_layer_groups():
    from trivy_amd.analyzer.secret import layer_groups
    assert layer_groups([], None, 100) == []
    assert layer_groups([10, 20, 30], None, 100) == [[0, 1, 2]]
    assert layer_groups([10, 20, 30], None, 30) == [[0, 1], [2]]          # respected: 60 > 30, 30 == 30 fits
    assert layer_groups([10, 20, 30], None, 29) == [[0], [1], [2]]         # 30 > 29 goes alone
    assert layer_groups([50, 500, 50, 50], None, 100) == [[0], [1], [2, 3]]  # an oversized layer alone
    assert layer_groups([500], None, 100) == [[0]]
    assert layer_groups([0, 0, 0], None, 0) == [[0, 1, 2]]
    base = [True, False, False, True, False, True]
    assert layer_groups([40] * 6, base, 80) == [[1, 2], [4]]               # base layers left out, order kept
    assert layer_groups([40] * 6, [True] * 6, 80) == []
    sizes = [(7 * k * k + 3) % 97 for k in range(200)]
    for gb in (1, 50, 96, 97, 400):
        groups = layer_groups(sizes, None, gb)
        assert [k for g in groups for k in g] == list(range(200))
        for g in groups:
            assert len(g) == 1 or sum(sizes[k] for k in g) <= gb
        for g, nxt in zip(groups, groups[1:]):  # greedy: the next layer did not fit
            assert sum(sizes[k] for k in g) + sizes[nxt[0]] > gb


def _layout(L, sizes, seg):
    import numpy as np
    L.tsg_debug_tar_forest_layout.argtypes = [c.c_void_p, c.c_uint32, c.c_uint32, c.c_void_p, c.POINTER(c.c_uint64),
                                              c.POINTER(c.c_uint32)]
    s = np.array(sizes, dtype=np.uint64)
    v0 = np.zeros(len(sizes), dtype=np.uint64)
    total, first = c.c_uint64(), c.c_uint32()
    assert L.tsg_debug_tar_forest_layout(s.ctypes.data, len(sizes), seg, v0.ctypes.data, c.byref(total), c.byref(first)) == 0
    return v0.tolist(), total.value, first.value


def test_virtual_block_space(an):
    """The library's layout (tarforest.h: TarForestSpan, TarForestCut) is the model's: V_k is a multiple of S,
    a layer without a complete block takes one segment, the total is the sum; a pass stays below 2^31 blocks."""
    for seg in (8, 64, 0):
        S = seg or 8192
        sizes = [0, 100, 512, 512 * S, 512 * S + 511, 512 * (S + 1), 3 * 512 * S - 1]
        v, total, first = _layout(an._L, sizes, seg)
        assert (v, total) == fm.virtual_blocks(sizes, S)
        assert v == [0, S, 2 * S, 3 * S, 4 * S, 5 * S, 7 * S] and total == 10 * S and first == len(sizes)
        sizes = [(7 * k * k + 3) % 97 * 4099 for k in range(300)]
        v, total, first = _layout(an._L, sizes, seg)
        assert (v, total) == fm.virtual_blocks(sizes, S) and first == 300
        big = [512 << 27] * 20  # 2^27 blocks each: the sixteenth does not fit beside fifteen
        assert _layout(an._L, big, seg)[2] == 15
        assert _layout(an._L, [100] + big, seg)[2] == 16
        assert _layout(an._L, [512 << 31, 4096], seg)[2] == 0 and _layout(an._L, [(512 << 31) - 1024, 4096], seg)[2] == 0
        assert _layout(an._L, [(512 << 31) - 512 * (S + 3), 4096], seg)[2] == 1
    bad = (c.c_uint64 * 1)(4096)
    for seg in (1, 4, 12, 100):
        assert an._L.tsg_debug_tar_forest_layout(bad, 1, seg, bad, c.byref(c.c_uint64()), c.byref(c.c_uint32())) == -1
