"""Layers resident in HBM, the part that needs no GPU (include/tsg_analyzer.h: tsg_analyzer_index_device_tar,
tsg_analyzer_submit_device_tar; trivy_amd/csrc/tar_index_host.h).

* the argument errors come back before any GPU work, on an analyzer whose scanner has no GPU engine;
* the versioned structs are laid out as the C compiler lays them out;
* the host half -- the chain walk over the candidate records, the index, the plan of a batch whose arena
  is the layer itself, the kinds -- driven with the records of the pure-Python kernel model
  (tests/tar_index_model.py) instead of the GPU's (tsg_debug_index_tar_records), reproduces
  oracle/analyzer.py's walk_layer_tar.
"""
import ctypes as c
import io
import random
import subprocess
import tarfile
from pathlib import Path

import numpy as np
import pytest

from oracle import analyzer as oan
from oracle import hostlib
from tests import tar_index_model as tm
from tests.layers import make_layer

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def an():
    from trivy_amd.analyzer import AnalyzerOptions, SecretAnalyzer
    a = SecretAnalyzer(lib=hostlib.lib(), host_only=True)
    a.Init(AnalyzerOptions())
    L = a._L
    L.tsg_debug_index_tar_records.argtypes = [c.c_void_p, c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint64,
                                              c.POINTER(c.c_void_p), c.c_void_p]
    L.tsg_debug_tar_batch_plan.argtypes = [c.c_void_p, c.c_uint32, c.c_uint32, c.c_void_p, c.POINTER(c.c_uint64),
                                           c.c_void_p, c.c_void_p, c.c_void_p]
    return a


@pytest.fixture(scope="module")
def oracle():
    return oan.SecretAnalyzer("")


def _err(a):
    from trivy_amd import _lib
    return _lib.last_error(a._L)


def _index(a, layer: bytes, shuffle_seed=1):
    """The index and stats of the host half over the model's records (shuffled: the order is unspecified)."""
    from trivy_amd.analyzer.secret import DEVICE_TAR_STATS_SIZE_V1, DeviceTarIndex, _CDeviceTarStats
    cands = tm.candidates(layer)
    order = list(range(len(cands)))
    random.Random(shuffle_seed).shuffle(order)
    recs = tm.records(cands, order)
    buf = np.frombuffer(layer or b"\0", dtype=np.uint8)
    st = _CDeviceTarStats()
    st.struct_size = DEVICE_TAR_STATS_SIZE_V1
    h = c.c_void_p()
    rc = a._L.tsg_debug_index_tar_records(a._h, buf.ctypes.data, len(layer), recs.ctypes.data if len(recs) else None,
                                          len(cands), c.byref(h), c.byref(st))
    if rc != 0:
        assert not h.value
        raise ValueError(_err(a))
    return DeviceTarIndex(a, h, None, st.to_dict()), cands


LAYERS = {
    "gnu": lambda: make_layer(100 + tarfile.GNU_FORMAT, 150, tarfile.GNU_FORMAT),
    "pax": lambda: make_layer(100 + tarfile.PAX_FORMAT, 150, tarfile.PAX_FORMAT),
    "ustar-prefix": tm.ustar_prefix_layer,
    "nested": tm.nested_layer,
    "pax-size": tm.pax_size_layer,
    "no-trailer": tm.no_trailer_layer,
    "empty": lambda: bytes(1024),
}
# candidates that are file data, not headers on the chain (the model's counts)
OFF_CHAIN = {"nested": 53, "pax-size": 1}


def test_model_counts():
    """The figures the cases rest on: make_layer(3, 60) has 220 blocks and 76 candidates, all on the chain;
    the nested layer has 81,920 bytes, 55 candidates and 2 regular entries on the chain."""
    l3 = make_layer(3, 60)
    assert len(l3) // 512 == 220 and len(tm.candidates(l3)) == 76
    n = tm.nested_layer()
    files, _, _ = oan.walk_layer_tar(n)
    assert len(n) == 81920 and len(tm.candidates(n)) == 55 and len(files) == 2
    assert [f[:2] for f in oan.walk_layer_tar(tm.pax_size_layer())[0]] == [("etc/pax.conf", 700), ("etc/second.conf", 30)]
    t = tm.no_trailer_layer()
    assert len(t) == 2560 and oan.walk_layer_tar(t)[0][-1][1] == 1024
    tm.kernel_blocks()


@pytest.mark.parametrize("name", list(LAYERS))
def test_host_half_vs_walk_layer_tar(an, oracle, name):
    layer = LAYERS[name]()
    ix, cands = _index(an, layer)
    files, wh, opq = oan.walk_layer_tar(layer)
    want = [(fp, size, content) for fp, size, content in files if oracle.required(fp, size)]
    got = ix.files()
    assert [(p, s) for p, _, s in got] == [(fp, size) for fp, size, _ in want]
    for (_, off, size), (_, _, content) in zip(got, want):
        assert layer[off:off + size] == content
    st = ix.stats
    with tarfile.open(fileobj=io.BytesIO(layer), mode="r:") as tf:
        n_members = len(tf.getmembers()) if any(layer) else 0
    assert st["entries"] == n_members
    assert st["whiteouts"] == wh and st["opaque_dirs"] == opq
    assert st["regular"] == len(files) and st["required"] == len(want)
    assert st["blocks"] == len(layer) // 512 and st["candidates"] == len(cands) and st["kernel_runs"] == 0
    assert st["off_chain"] == OFF_CHAIN.get(name, 0)
    # a chain block that is no candidate: the end-of-archive zero block, where the layer has one
    assert st["block_fetches"] == (0 if name == "no-trailer" else 1)
    if name in ("gnu", "pax", "pax-size"):
        assert st["ext_bytes"] > 0  # long names / PAX records came through range copies
    if name in ("ustar-prefix", "nested", "no-trailer", "empty"):
        assert st["ext_bytes"] == 0
    if name != "empty":
        assert len(want) >= (1 if name == "nested" else 2)  # (Required refuses inner.tar by its extension)
    if name in ("gnu", "pax"):
        assert wh > 0 and opq > 0 and len(want) < len(files)


@pytest.mark.parametrize("name", ["gnu", "pax", "nested", "pax-size", "no-trailer"])
def test_batch_plan(an, name):
    """The pseudo-files of a sub-range: gap, file, gap, ..., file, gap over the layer from a 512-B boundary
    at or before the first file's header; kinds from the IsBinary flags by DeviceKinds' rule."""
    layer = LAYERS[name]()
    ix, _ = _index(an, layer)
    files = ix.files()
    n = len(files)
    rng = random.Random(3)
    ranges = {(0, n), (0, 1), (n - 1, 1), (n // 2, n - n // 2), (min(1, n - 1), max(1, n // 3)), (0, 0)}
    for first, count in sorted(ranges):
        m = 2 * count + 1
        flags = np.array([rng.randint(0, 1) for _ in range(m)], dtype=np.uint8)
        for j in range(count):
            _, off, size = files[first + j]
            flags[2 * j + 1] = 1 if oan.is_binary(layer[off:off + size], size) else 0
        base = c.c_uint64(123)
        offs = np.zeros(m + 1, dtype=np.uint64)
        kinds = np.full(m, 9, dtype=np.uint8)
        binary = np.full(m, 9, dtype=np.uint8)
        assert an._L.tsg_debug_tar_batch_plan(ix._h, first, count, flags.ctypes.data, c.byref(base), offs.ctypes.data,
                                              kinds.ctypes.data, binary.ctypes.data) == 0, _err(an)
        b = base.value
        want_offs = [0]
        for j in range(count):
            _, off, size = files[first + j]
            want_offs += [off - b, off + size - b]
        want_offs.append(want_offs[-1])
        assert offs.tolist() == want_offs
        if count:
            assert b == int(ix.start[first])  # what DeviceTarIndex.batches measures a batch's span from
            assert b % 512 == 0 and b <= files[first][1] - 512
            prev_end = 0 if first == 0 else files[first - 1][1] + files[first - 1][2]
            assert b >= prev_end
            assert want_offs[-1] + b + 64 <= len(layer) + 64  # the 64 bytes after the batch are the layer's own
        want_kinds = [3] * m
        for j in range(count):
            p = files[first + j][0]
            want_kinds[2 * j + 1] = 1 if not flags[2 * j + 1] else 2 if p.endswith(".pyc") else 3
        assert kinds.tolist() == want_kinds
        assert binary.tolist() == [1 if k == 2 else 0 for k in want_kinds]
    if name in ("gnu", "pax", "pax-size"):  # long names / PAX records: the chain starts before the entry's header
        assert any(int(ix.start[i]) < files[i][1] - 512 for i in range(n))
        assert all(int(ix.start[i]) <= files[i][1] - 512 and int(ix.start[i]) % 512 == 0 for i in range(n))
    if name == "gnu":
        ks = []
        for j, (p, off, size) in enumerate(files):
            ks.append(1 if not oan.is_binary(layer[off:off + size], size) else 2 if p.endswith(".pyc") else 3)
        assert {1, 2, 3} <= set(ks)
    h = c.c_uint64()
    assert an._L.tsg_debug_tar_batch_plan(ix._h, n, 1, flags.ctypes.data, c.byref(h), offs.ctypes.data,
                                          kinds.ctypes.data, binary.ctypes.data) < 0


def _host_walk_error(an, layer: bytes) -> str:
    from trivy_amd.analyzer.secret import Collector, _CTarStats
    with pytest.raises(ValueError) as e:
        coll = Collector(an, 1 << 20)
        cursor = 0
        while True:
            rc, cursor = coll.add_tar(layer, cursor, _CTarStats())
            coll.reset()
            if rc == 0:
                break
    return str(e.value).replace("tar layer: ", "")


def test_malformed_layers_give_the_host_walks_error(an):
    layer = bytearray(make_layer(3, 60))
    ix, _ = _index(an, bytes(layer))
    # the header of a regular entry in the middle of the layer: its checksum field off by one
    _, off, _ = ix.files()[5]
    layer[off - 512 + 150] ^= 0x01
    assert not tm.is_candidate(bytes(layer[off - 512:off]))
    with pytest.raises(ValueError) as e:
        _index(an, bytes(layer))
    assert str(e.value) == "tar: invalid header checksum at offset %d" % (off - 512)
    assert str(e.value) == _host_walk_error(an, bytes(layer))
    # a truncated last entry
    good = make_layer(4, 20)
    ix, _ = _index(an, good)
    _, off, size = ix.files()[-1]
    trunc = good[:off + size - 3]
    with pytest.raises(ValueError) as e:
        _index(an, trunc)
    assert str(e.value) == "tar: truncated entry data" == _host_walk_error(an, trunc)
    # garbage where a header should be
    junk = bytearray(good)
    junk[off - 512:off] = bytes(random.Random(1).randrange(1, 256) for _ in range(512))
    with pytest.raises(ValueError) as e:
        _index(an, bytes(junk))
    assert str(e.value) == _host_walk_error(an, bytes(junk))


# ---- the C ABI ---------------------------------------------------------------
def test_struct_layouts(tmp_path):
    from trivy_amd.analyzer.secret import (DEVICE_TAR_SIZE_V1, DEVICE_TAR_STATS_SIZE_V1, _CDeviceTar,
                                           _CDeviceTarStats, _CTarStats)
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "tsg_analyzer.h"\nint main(void){printf("%zu %u %zu %zu %zu %u %zu %zu %zu %zu\\n",'
                   ' sizeof(tsg_device_tar), (unsigned)TSG_DEVICE_TAR_SIZE_V1, offsetof(tsg_device_tar, dev_tar),'
                   ' offsetof(tsg_device_tar, n_bytes), sizeof(tsg_device_tar_stats),'
                   ' (unsigned)TSG_DEVICE_TAR_STATS_SIZE_V1, offsetof(tsg_device_tar_stats, tar),'
                   ' offsetof(tsg_device_tar_stats, blocks), offsetof(tsg_device_tar_stats, ms_kernel),'
                   ' sizeof(tsg_tar_stats)); return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    (size_t, v1_t, off_dev, off_n, size_s, v1_s, off_tar, off_blocks, off_ms, size_ts) = \
        [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert size_t == v1_t == c.sizeof(_CDeviceTar) == DEVICE_TAR_SIZE_V1 == 24
    assert off_dev == _CDeviceTar.dev_tar.offset == 8 and off_n == _CDeviceTar.n_bytes.offset == 16
    assert size_ts == c.sizeof(_CTarStats) == 64
    assert size_s == v1_s == c.sizeof(_CDeviceTarStats) == DEVICE_TAR_STATS_SIZE_V1 == 8 + 64 + 6 * 8 + 16
    assert off_tar == _CDeviceTarStats.tar.offset == 8
    assert off_blocks == _CDeviceTarStats.blocks.offset and off_ms == _CDeviceTarStats.ms_kernel.offset


def test_argument_errors_come_before_any_gpu_work(an):
    """On an analyzer whose scanner has no GPU engine every argument error comes back first (-1, its own
    text); valid arguments stop at the missing engine (-2)."""
    from trivy_amd.analyzer.secret import (DEVICE_TAR_SIZE_V1, DEVICE_TAR_STATS_SIZE_V1, _CDeviceTar,
                                           _CDeviceTarStats, _declare)
    L = an._L
    _declare(L)
    fake = 0x700000000000  # never dereferenced

    def index(t, st=None, out=True, a=an._h):
        h = c.c_void_p(1)
        rc = L.tsg_analyzer_index_device_tar(a, c.byref(t) if t is not None else None, c.byref(h) if out else None,
                                             c.byref(st) if st is not None else None)
        if out:
            assert not h.value
        return rc, _err(an)

    for bogus in (0, 8, DEVICE_TAR_SIZE_V1 - 8, DEVICE_TAR_SIZE_V1 + 8, 0xFFFFFFFF):
        rc, text = index(_CDeviceTar(bogus, 0, fake, 4096))
        assert rc == -1 and "struct_size %d" % bogus in text
    st = _CDeviceTarStats()
    st.struct_size = DEVICE_TAR_STATS_SIZE_V1 + 8
    rc, text = index(_CDeviceTar(DEVICE_TAR_SIZE_V1, 0, fake, 4096), st)
    assert rc == -1 and "tsg_device_tar_stats.struct_size" in text
    rc, text = index(_CDeviceTar(DEVICE_TAR_SIZE_V1, 0, None, 4096))
    assert rc == -1 and "dev_tar is NULL" in text
    for mis in (1, 4, 8, 15):
        rc, text = index(_CDeviceTar(DEVICE_TAR_SIZE_V1, 0, fake + mis, 4096))
        assert rc == -1 and "16-B aligned" in text
    rc, text = index(_CDeviceTar(DEVICE_TAR_SIZE_V1, 0, fake, 512 << 32))
    assert rc == -1 and "2^32" in text
    assert index(_CDeviceTar(DEVICE_TAR_SIZE_V1, 0, fake, 4096), out=False)[0] == -1
    assert index(None)[0] == -1
    assert index(_CDeviceTar(DEVICE_TAR_SIZE_V1, 0, fake, 4096), a=None)[0] == -1
    # valid: the largest layer the index takes; it stops at the scanner's missing engine, not at an argument
    st.struct_size = DEVICE_TAR_STATS_SIZE_V1
    rc, text = index(_CDeviceTar(DEVICE_TAR_SIZE_V1, 0, fake, (512 << 32) - 1), st)
    assert rc == -2 and "no GPU engine" in text

    ix, _ = _index(an, make_layer(3, 60))
    n = ix.n
    assert n > 10

    def submit(first, count, index=ix._h, out=True):
        h = c.c_void_p(1)
        rc = L.tsg_analyzer_submit_device_tar(an._h, index, first, count, c.byref(h) if out else None)
        if out:
            assert not h.value
        return rc, _err(an)

    for first, count in [(0, n + 1), (n, 1), (n + 1, 0), (1, n), (0xFFFFFFFF, 1), (0xFFFFFFFF, 0xFFFFFFFF)]:
        rc, text = submit(first, count)
        assert rc == -1 and "outside the index" in text, (first, count)
    assert submit(0, 1, index=None)[0] == -1
    assert submit(0, 1, out=False)[0] == -1
    rc, text = submit(0, n)  # in range: refused only because this index was made without a device layer
    assert rc == -1 and "no device layer" in text
    pp, pl, off, size = c.c_void_p(), c.c_uint64(), c.c_uint64(), c.c_uint64()
    assert L.tsg_tar_index_file(ix._h, n, c.byref(pp), c.byref(pl), c.byref(off), c.byref(size)) == -1
    assert L.tsg_tar_index_file(ix._h, n - 1, c.byref(pp), c.byref(pl), c.byref(off), c.byref(size)) == 0
    assert (c.string_at(pp, pl.value).decode(), off.value, size.value) == ix.files()[-1]
