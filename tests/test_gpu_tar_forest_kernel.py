"""The forest pass over all layers of an image (trivy_amd/csrc/tarforest.hip) through tsg_debug_tar_forest: per
layer the head, the entry records and the names equal the pure-Python model's (tests/tar_forest_model.py: the
single-layer model applied per layer), each layer's slice of the two shared buffers is what the single-layer pass
writes for it, and nothing is written past the totals -- at every segment size and with one workgroup striding
over everything.
"""
import ctypes as c
import tarfile

import numpy as np
import pytest

from tests import tar_chain_model as cm
from tests import tar_forest_model as fm
from tests import tar_index_model as tm
from tests.layers import make_layer
from tests.test_gpu_tar_chain_kernel import LAYERS

pytestmark = pytest.mark.gpu

SEGMENTS = (8, 64, 0)  # 0: the default
DEFAULT_S = 8192
CAPS = (0, 1)


@pytest.fixture(scope="module")
def L():
    from trivy_amd import _lib
    lib = _lib.lib()
    u64p = c.POINTER(c.c_uint64)
    lib.tsg_debug_tar_forest.argtypes = [c.c_int, c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_uint32, c.c_void_p,
                                         c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint64, u64p, c.c_void_p, c.c_uint64,
                                         u64p]
    lib.tsg_debug_tar_chain.argtypes = [c.c_int, c.c_void_p, c.c_uint64, c.c_uint32, c.c_uint32, c.c_void_p, c.c_uint64,
                                        u64p, c.c_void_p, c.c_uint64, u64p, c.c_void_p, u64p]
    return lib


_dev, _model = {}, {}


def dev(data: bytes):
    """The device copy of `data` (made once): all of it is there, with 16 more bytes."""
    import torch
    if id(data) not in _dev:
        t = torch.from_numpy(np.frombuffer(data + bytes(16), dtype=np.uint8).copy()).to("cuda:0")
        assert t.data_ptr() % 16 == 0
        _dev[id(data)] = (t, data)  # (data kept: its id stays its own)
    return _dev[id(data)][0].data_ptr()


def part(data: bytes, n: int, off: int = 0):
    """The model's verdict on the layer data[off:off + n] (computed once)."""
    key = (id(data), off, n)
    if key not in _model:
        _model[key] = (fm.layer(data[off:], n), data)
    return _model[key][0]


def own(data: bytes, n=None):
    """A layer in an allocation of its own: (device pointer, the model's part)."""
    n = len(data) if n is None else n
    return dev(data), n, part(data, n)


def _run(L, ptrs, sizes, rec_cap, name_cap, segment, grid_cap):
    from trivy_amd import _lib
    n = len(ptrs)
    heads = np.full(8 * n, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    rb, nb = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    recs = np.full(64 * rec_cap, 0xA5, dtype=np.uint8)
    names = np.full(name_cap, 0xA5, dtype=np.uint8)
    n_rec, n_names = c.c_uint64(1 << 40), c.c_uint64(1 << 40)
    p = np.array(ptrs, dtype=np.uint64)
    s = np.array(sizes, dtype=np.uint64)
    rc = L.tsg_debug_tar_forest(0, p.ctypes.data, s.ctypes.data, n, segment, grid_cap, heads.ctypes.data, rb.ctypes.data,
                                nb.ctypes.data, recs.ctypes.data, rec_cap, c.byref(n_rec), names.ctypes.data, name_cap,
                                c.byref(n_names))
    assert rc == 0, _lib.last_error(L)
    assert (recs[64 * n_rec.value:] == 0xA5).all() and (names[n_names.value:] == 0xA5).all()  # nothing past the totals
    hs = [fm.HEAD.unpack(heads[8 * k:8 * k + 8].tobytes()) for k in range(n)]
    return hs, rb.tolist(), nb.tolist(), recs, names, n_rec.value, n_names.value


def _check(L, items, segments=SEGMENTS, caps=CAPS):
    """items: (device pointer, n_bytes, the model's part) per layer.  The forest equals the model at every
    segment size and grid; returns the model's heads."""
    parts = [it[2] for it in items]
    heads, rec_base, name_base, n_rec, n_names = fm.forest(parts)
    for seg in segments:
        S = seg or DEFAULT_S
        for cap in caps:
            hs, rb, nb, recs, names, got_rec, got_names = _run(L, [it[0] for it in items], [it[1] for it in items],
                                                               n_rec + 8, n_names + 64, seg, cap)
            assert (got_rec, got_names) == (n_rec, n_names), (seg, cap)
            assert rb == rec_base and nb == name_base, (seg, cap)
            for k, (want, stop, n_cand) in enumerate(parts):
                kind, reason, offset, ext, steps, entries, name_bytes, cands, pad = hs[k]
                why = (seg, cap, k)
                assert pad == 0 and cands == n_cand, why
                if stop[0] == cm.END:
                    assert (kind, reason, offset, ext) == stop, why
                else:  # (the hopped-header count of an INCOMPLETE entry is not part of the contract)
                    assert (kind, reason, offset) == stop[:3], why
                assert (entries, name_bytes) == heads[k][4:6], why
                assert steps <= items[k][1] // 512 // S + 1, why  # at most one dependent load per segment entered
                got = cm.unpack(recs[64 * rb[k]:], entries, names[nb[k]:nb[k] + name_bytes])
                assert got == want, why
    return heads


def test_every_chain_kernel_layer_in_one_forest(L):
    """Every layer of the single-layer kernel test, and boundary_layer(S) three times in a row."""
    base = [own(_layer(name)) for name in LAYERS]
    for seg in (8, 64):
        b = own(_boundary(seg))
        heads = _check(L, base + [b, b, b], segments=(seg,))
        assert all(h[0] == cm.END and h[4] >= 2 for h in heads)
    b = own(_boundary(64))
    _check(L, [b] + base + [b, b], segments=(0,))


_named = {}


def _layer(name):
    if name not in _named:
        _named[name] = LAYERS[name]()
    return _named[name]


def _boundary(S):
    return _named.setdefault(("boundary", S), cm.boundary_layer(S))


def test_default_segment_boundaries_three_times(L):
    """29 MB each: seven segments of the default 8,192 blocks per layer, the boundary cases at that size."""
    b = own(_boundary(DEFAULT_S))
    heads = _check(L, [b, b, b], segments=(0,))  # whole grid, and one workgroup striding over all 21 segments
    assert all(h[0] == cm.END and h[4] > DEFAULT_S for h in heads)


@pytest.mark.parametrize("name", ["gnu3", "pax7", "nested", "no-trailer", "boundary"])
def test_one_layer_forest_equals_the_chain_pass(L, name):
    """A forest of one layer and tsg_debug_tar_chain: the same bytes."""
    data = _boundary(64) if name == "boundary" else _layer(name)
    ptr, n, (want, stop, n_cand) = own(data)
    rec_cap, name_cap = len(want) + 8, sum(len(e["name"]) for e in want) + 64
    for seg in SEGMENTS:
        for cap in CAPS:
            hs, rb, nb, recs, names, n_rec, n_names = _run(L, [ptr], [n], rec_cap, name_cap, seg, cap)
            recs1 = np.full(64 * rec_cap, 0xA5, dtype=np.uint8)
            names1 = np.full(name_cap, 0xA5, dtype=np.uint8)
            stop1 = np.zeros(4, dtype=np.uint64)
            r1, b1, c1 = c.c_uint64(), c.c_uint64(), c.c_uint64()
            assert L.tsg_debug_tar_chain(0, ptr, n, seg, cap, recs1.ctypes.data, rec_cap, c.byref(r1), names1.ctypes.data,
                                         name_cap, c.byref(b1), stop1.ctypes.data, c.byref(c1)) == 0
            assert (n_rec, n_names) == (r1.value, b1.value) and rb == [0] and nb == [0]
            assert recs.tobytes() == recs1.tobytes() and names.tobytes() == names1.tobytes()
            assert hs[0][:4] == tuple(int(x) for x in stop1) and hs[0][5:8] == (r1.value, b1.value, c1.value)


def test_complete_and_punted_layers_mixed(L):
    """All complete cases and all punt cases, interleaved: the complete layers' records and names are the
    model's; a punted layer's head is INCOMPLETE with the model's reason and offset and it takes no record."""
    good, punts = cm.complete_cases(), cm.punt_cases()
    _named.setdefault("cases", (good, punts))
    items, kinds = [], []
    gi, pi = list(good), list(punts)
    for j in range(max(len(gi), len(pi))):
        if j < len(pi):
            data, reason, at = punts[pi[j]]
            items.append(own(data))
            kinds.append((cm.INCOMPLETE, reason, at))
        if j < len(gi):
            items.append(own(good[gi[j]]))
            kinds.append(None)
    heads = _check(L, items)
    for h, kind in zip(heads, kinds):
        if kind is None:
            assert h[0] == cm.END
        else:
            assert h[:3] == kind and h[4:6] == (0, 0)
    assert sum(h[4] for h in heads) >= len(good)


def _blocks_layer(blocks: int) -> bytes:
    """A well-formed layer of exactly `blocks` blocks: one file, its data, the two trailer blocks."""
    return cm.sized(b"fill/%d.txt" % blocks, blocks - 3) + cm.TRAILER


@pytest.mark.parametrize("seg", SEGMENTS)
def test_tiny_and_segment_sized_layers_in_every_position(L, seg):
    """Layers of 0 bytes, 100 bytes, exactly 512 bytes, S blocks and S + 1 blocks, each as first, middle and
    last layer of a forest.  (A layer without a complete block gets its head without a read: the 100 bytes
    lie at the start of a valid header.)"""
    S = seg or DEFAULT_S
    hdr = _named.setdefault("one-header", bytes(tm.header(b"lonely", 0)))
    normal = own(_layer("gnu3"))
    full, more = _named.setdefault(("blocks", S), (_blocks_layer(S), _blocks_layer(S + 1)))
    special = [own(hdr, 0), own(hdr, 100), own(hdr, 512), own(full), own(more)]
    assert special[0][2][1] == (cm.END, cm.OK, 0, 0) and special[1][2][1] == (cm.INCOMPLETE, cm.TRUNCATED, 0, 0)
    assert special[2][2][1] == (cm.END, cm.OK, 512, 0) and len(special[2][2][0]) == 1
    assert len(full) == 512 * S and len(more) == 512 * (S + 1)
    for r in range(5):
        rot = special[r:] + special[:r]
        heads = _check(L, [rot[0], normal, rot[1], rot[2], rot[3], normal, rot[4]], segments=(seg,))
        assert heads[1] == heads[5] and heads[1][4] > 20


def test_adjacent_slices_of_one_buffer(L):
    """Layers as 512-B-aligned ranges of one buffer.  (a) a layer without a trailer directly followed by
    another layer's first header: it ENDs at its own end and the second is unaffected.  (b) a layer cut so that
    its last entry's data runs past its end, into the next layer's bytes: truncated, the neighbour unaffected."""
    bare, nxt = tm.no_trailer_layer(), _layer("gnu3")
    assert len(bare) % 512 == 0
    buf = _named.setdefault("slices-a", bare + nxt)
    p = dev(buf)
    items = [(p, len(bare), part(buf, len(bare))), (p + len(bare), len(nxt), part(buf, len(nxt), len(bare)))]
    heads = _check(L, items)
    assert heads[0][:3] == (cm.END, cm.OK, len(bare)) and heads[0][4] >= 2
    assert heads[1] == fm.forest([own(nxt)[2]])[0][0]
    # (b)
    first = _layer("gnu7")
    entries, _, _ = cm.chain(first)
    big = [e for e in entries if e["size"] > 1024][-1]
    cut = big["data"] + 512  # inside the entry's data, on a block boundary
    buf = _named.setdefault("slices-b", first[:cut] + nxt)
    p = dev(buf)
    items = [(p, cut, part(buf, cut)), (p + cut, len(nxt), part(buf, len(nxt), cut)), own(nxt)]
    heads = _check(L, items)
    assert heads[0][:3] == (cm.INCOMPLETE, cm.TRUNCATED, big["start"]) and heads[0][4:6] == (0, 0)
    assert heads[1] == heads[2] and heads[1][0] == cm.END


def test_64_layers_of_alternating_formats(L):
    items = [own(_named.setdefault(("l20", s), make_layer(s, 20, tarfile.PAX_FORMAT if s % 2 else tarfile.GNU_FORMAT)))
             for s in range(64)]
    heads = _check(L, items)
    assert all(h[0] == cm.END and h[4] >= 20 for h in heads)


def test_arguments(L):
    ptr, n, _ = own(_layer("gnu3"))
    p = np.array([ptr, ptr], dtype=np.uint64)
    s = np.array([n, n], dtype=np.uint64)
    heads, rb, nb = np.zeros(16, dtype=np.uint64), np.zeros(2, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    n_rec, n_names = c.c_uint64(), c.c_uint64()

    def call(ptrs, n_layers, seg):
        return L.tsg_debug_tar_forest(0, ptrs.ctypes.data, s.ctypes.data, n_layers, seg, 0, heads.ctypes.data,
                                      rb.ctypes.data, nb.ctypes.data, None, 0, c.byref(n_rec), None, 0, c.byref(n_names))
    for bad in (1, 4, 12, 100, 16384, 1 << 20):
        assert call(p, 2, bad) == -2
    assert call(p, 0, 0) == -2 and call(p, 65537, 0) == -2
    assert call(np.array([ptr, ptr + 8], dtype=np.uint64), 2, 0) == -2  # misaligned
    # buffers too small: -3, with what is needed
    assert call(p, 2, 0) == -3
    want = own(_layer("gnu3"))[2][0]
    assert n_rec.value == 2 * len(want) and n_names.value == 2 * sum(len(e["name"]) for e in want)
