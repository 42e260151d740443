"""The GPU half of the tar chain walk (trivy_amd/csrc/tarchain.hip) through tsg_debug_tar_chain: the entry
records, the names, the stop and the candidate count equal the pure-Python model's (tests/tar_chain_model.py)
at every segment size and with one workgroup striding over everything.  The model itself is checked against
oracle/analyzer.py's walk in tests/test_tar_walk_host.py.
"""
import ctypes as c
import tarfile

import numpy as np
import pytest

from tests import tar_chain_model as cm
from tests import tar_index_model as tm
from tests.layers import make_layer

pytestmark = pytest.mark.gpu

SEGMENTS = (8, 64, 0)  # 0: the default


@pytest.fixture(scope="module")
def L():
    from trivy_amd import _lib
    lib = _lib.lib()
    lib.tsg_debug_tar_chain.argtypes = [c.c_int, c.c_void_p, c.c_uint64, c.c_uint32, c.c_uint32, c.c_void_p, c.c_uint64,
                                        c.POINTER(c.c_uint64), c.c_void_p, c.c_uint64, c.POINTER(c.c_uint64),
                                        c.c_void_p, c.POINTER(c.c_uint64)]
    return lib


class Dev:
    """A layer on the device: all of `data` is there, so the bytes past n_bytes are there to be read by a
    kernel that goes too far."""

    def __init__(self, data: bytes):
        import torch
        self.t = torch.from_numpy(np.frombuffer(data + bytes(16), dtype=np.uint8).copy()).to("cuda:0")
        assert self.t.data_ptr() % 16 == 0


def _run(L, dev, n, want_entries, want_names, segment=0, grid_cap=0):
    from trivy_amd import _lib
    rec_cap, name_cap = want_entries + 8, want_names + 64
    recs = np.full(64 * rec_cap, 0xA5, dtype=np.uint8)
    names = np.full(name_cap, 0xA5, dtype=np.uint8)
    stop = np.zeros(4, dtype=np.uint64)
    n_rec, n_names, n_cand = c.c_uint64(1 << 40), c.c_uint64(1 << 40), c.c_uint64(1 << 40)
    rc = L.tsg_debug_tar_chain(0, dev.t.data_ptr(), n, segment, grid_cap, recs.ctypes.data, rec_cap, c.byref(n_rec),
                               names.ctypes.data, name_cap, c.byref(n_names), stop.ctypes.data, c.byref(n_cand))
    assert rc == 0, _lib.last_error(L)
    assert (recs[64 * n_rec.value:] == 0xA5).all() and (names[n_names.value:] == 0xA5).all()
    return cm.unpack(recs, n_rec.value, names[:n_names.value]), tuple(int(x) for x in stop), n_cand.value


def _check(L, data, n_bytes=None, segments=SEGMENTS, grid_caps=(0,)):
    """The model's result, after the kernels gave the same at every segment size."""
    n = len(data) if n_bytes is None else n_bytes
    entries, stop, n_cand = cm.chain(data, n)
    want = cm.strip_next(entries) if stop[0] == cm.END else []  # nothing is handed over for an INCOMPLETE stop
    name_bytes = sum(len(e["name"]) for e in want)
    dev = Dev(data)
    for seg in segments:
        for cap in grid_caps:
            got, got_stop, got_cand = _run(L, dev, n, len(want), name_bytes, seg, cap)
            assert got_cand == n_cand, (seg, cap)
            if stop[0] == cm.END:
                assert got_stop == stop, (seg, cap)
            else:  # (the hopped-header count of an INCOMPLETE entry is not part of the contract)
                assert got_stop[:3] == stop[:3], (seg, cap)
            assert got == want, (seg, cap)
    return entries, stop


LAYERS = {
    "gnu3": lambda: make_layer(3, 60, tarfile.GNU_FORMAT),
    "gnu7": lambda: make_layer(7, 60, tarfile.GNU_FORMAT),
    "pax3": lambda: make_layer(3, 60, tarfile.PAX_FORMAT),
    "pax7": lambda: make_layer(7, 60, tarfile.PAX_FORMAT),
    "ustar": cm.ustar_layer,
    "ustar-prefix": tm.ustar_prefix_layer,
    "odd-names": cm.odd_names_layer,
    "nested": tm.nested_layer,
    "pax-size": tm.pax_size_layer,
    "no-trailer": tm.no_trailer_layer,
}


@pytest.mark.parametrize("name", list(LAYERS))
def test_layers_vs_model(L, name):
    entries, stop = _check(L, LAYERS[name](), grid_caps=(0, 1))
    assert stop[0] == cm.END and len(entries) >= 2
    if name == "nested":
        assert len(entries) == 2
    if name == "no-trailer":
        assert stop[2] == 2560  # the data ends exactly at n: END past the last block, no zero block read


@pytest.mark.parametrize("S", [8, 64])
def test_segment_boundaries(L, S):
    """cm.boundary_layer: a full segment of zero-size entries, a file ending exactly on a boundary, one
    spanning more than three segments, x / L headers straddling a boundary, and a tar inside a file's data
    whose off-chain candidates change nothing."""
    data = cm.boundary_layer(S)
    entries, stop = _check(L, data, grid_caps=(0, 1))
    assert stop[0] == cm.END and [e["name"] for e in entries[-2:]] == [b"outer.bin", b"after.conf"]
    assert all(e["start"] == 512 * i and e["size"] == 0 for i, e in enumerate(entries[:S + 3]))
    assert any(e["n_ext"] == 2 and e["start"] // 512 % S == S - 2 and e["flags"] == cm.NAME_LONG for e in entries)
    assert any(e["start"] // 512 % S == 0 and e["size"] == 512 * (3 * S + 5) for e in entries)


def test_default_segment_has_several_segments(L):
    """29 MB: seven segments of the default 8,192 blocks, with the same boundary cases at that size."""
    data = cm.boundary_layer(8192)
    assert len(data) // 512 > 6 * 8192
    entries, stop = _check(L, data, segments=(0, 64))
    assert stop[0] == cm.END and len(entries) > 8192


@pytest.mark.parametrize("name", list(cm.complete_cases()))
def test_cases_the_device_completes(L, name):
    data = cm.complete_cases()[name]
    entries, stop = _check(L, data, grid_caps=(0, 1))
    assert stop[0] == cm.END
    by_name = {e["name"]: e for e in entries}
    if name == "pax-size-override":
        assert by_name[b"sparse/file"]["size"] == 1000 and by_name[b"sparse/link"]["size"] == 0
        assert by_name[b"after"]["start"] == by_name[b"sparse/link"]["hdr"] + 512
    if name == "two-x-headers":
        assert [(e["name"], e["size"], e["n_ext"]) for e in entries] == [(b"second/name", 3, 2), (b"after", len(cm.TEXT), 0)]
    if name == "K-and-g":
        assert [(e["typeflag"], e["n_ext"]) for e in entries] == [(ord("g"), 0), (ord("2"), 2), (ord("0"), 0)]
        assert entries[1]["name"] == b"n" * 130
    if name == "base-256-size":
        assert entries[0]["size"] == 1300
    if name == "symlink-with-size":
        assert entries[0]["size"] == 0 and entries[1]["start"] == 512
    if name in ("x-then-zero-block", "x-then-end"):
        assert len(entries) == 1 and stop == (cm.END, cm.OK, 1024, 1)
    if name == "16-extension-headers":
        assert entries[0]["n_ext"] == 16 and entries[0]["name"] == b"p/15"
    if name == "pax-data-64KiB":
        assert entries[0]["name"] == b"exactly/64KiB"
    if name == "long-name-with-NULs":
        assert entries[0]["name"] == b"dir/name"
    if name in ("only-zero-blocks", "one-zero-block"):
        assert entries == [] and stop == (cm.END, cm.OK, 0, 0)


def test_empty_and_short_layers(L):
    """No complete block: END for no bytes at all, a truncated header otherwise (decided without a kernel)."""
    dev = Dev(bytes(tm.header(b"poison", 5)))
    assert _run(L, dev, 0, 0, 0) == ([], (cm.END, cm.OK, 0, 0), 0)
    for n in (1, 511):
        assert _run(L, dev, n, 0, 0) == ([], (cm.INCOMPLETE, cm.TRUNCATED, 0, 0), 0)


@pytest.mark.parametrize("extra", [1, 300, 511])
def test_partial_last_block_is_never_read(L, extra):
    """n is no multiple of 512.  The partial block and the bytes after it are a valid header, in memory in
    full.  After a trailer the chain has ended before it; without one the walk stops there, truncated."""
    layer = make_layer(3, 20)
    poison = bytes(tm.header(b"poison/after-the-end.txt", 5))
    entries, stop = _check(L, layer + poison, len(layer) + extra)
    assert stop[0] == cm.END and len(entries) > 20
    bare = tm.no_trailer_layer()
    entries, stop = _check(L, bare + poison, len(bare) + extra)
    assert stop == (cm.INCOMPLETE, cm.TRUNCATED, len(bare), 0)


@pytest.mark.parametrize("name", list(cm.punt_cases()))
def test_punts_stop_incomplete_where_the_model_stops(L, name):
    data, reason, at = cm.punt_cases()[name]
    entries, stop = _check(L, data)
    assert stop[:3] == (cm.INCOMPLETE, reason, at) and len(entries) == 2


def test_segment_argument(L):
    dev = Dev(make_layer(3, 20))
    n_rec, n_names, n_cand = c.c_uint64(), c.c_uint64(), c.c_uint64()
    stop = np.zeros(4, dtype=np.uint64)
    for bad in (1, 4, 12, 100, 16384, 1 << 20):
        assert L.tsg_debug_tar_chain(0, dev.t.data_ptr(), 4096, bad, 0, None, 0, c.byref(n_rec), None, 0, c.byref(n_names),
                                     stop.ctypes.data, c.byref(n_cand)) == -2
    # buffers too small: -3, with what is needed
    assert L.tsg_debug_tar_chain(0, dev.t.data_ptr(), dev.t.numel() - 16, 0, 0, None, 0, c.byref(n_rec), None, 0,
                                 c.byref(n_names), stop.ctypes.data, c.byref(n_cand)) == -3
    entries, _, _ = cm.chain(make_layer(3, 20))
    assert n_rec.value == len(entries) and n_names.value == sum(len(e["name"]) for e in entries)
