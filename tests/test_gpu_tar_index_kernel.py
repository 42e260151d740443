"""tar_headers_kernel (trivy_amd/csrc/tarindex.hip) through tsg_debug_tar_headers: the records, as the set
of (block, 512 bytes), and the count equal the pure-Python model's (tests/tar_index_model.py) on every
input; nothing is read past the complete blocks and nothing is written past the capacity.
"""
import ctypes as c
import random
import tarfile

import numpy as np
import pytest

from tests import tar_index_model as tm
from tests.layers import make_layer

pytestmark = pytest.mark.gpu

GUARD = 4096


@pytest.fixture(scope="module")
def L():
    from trivy_amd import _lib
    lib = _lib.lib()
    lib.tsg_debug_tar_headers.argtypes = [c.c_int, c.c_void_p, c.c_uint64, c.c_uint64, c.c_uint32, c.c_void_p,
                                          c.POINTER(c.c_uint64), c.POINTER(c.c_double)]
    return lib


def _run(L, data: bytes, n_bytes=None, capacity=None, grid_cap=0):
    """(count, records buffer with its guard) of one kernel run over data[:n_bytes]; the tensor holds all
    of `data`, so bytes past n_bytes are there to be read by a kernel that goes too far."""
    import torch
    from trivy_amd import _lib
    n = len(data) if n_bytes is None else n_bytes
    host = np.frombuffer(data + bytes(16), dtype=np.uint8).copy()
    dev = torch.from_numpy(host).to("cuda:0")
    want = len(tm.candidates(data, n))
    cap = want if capacity is None else capacity
    rec = torch.full((cap * tm.RECORD + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert dev.data_ptr() % 16 == 0 and rec.data_ptr() % 16 == 0
    count, ms = c.c_uint64(1 << 40), c.c_double(-1)
    rc = L.tsg_debug_tar_headers(0, dev.data_ptr(), n, cap, grid_cap, rec.data_ptr(), c.byref(count), c.byref(ms))
    assert rc == 0, _lib.last_error(L)
    if n >= 512:
        assert ms.value >= 0
    out = rec.cpu().numpy()
    assert (out[cap * tm.RECORD:] == 0xA5).all()  # nothing written past the capacity
    return count.value, out


def _check(L, data, n_bytes=None, grid_cap=0):
    want = tm.candidates(data, n_bytes)
    count, out = _run(L, data, n_bytes, grid_cap=grid_cap)
    assert count == len(want)
    assert tm.parse_records(out, count) == set(want)
    return want


LAYERS = {
    "l3": lambda: make_layer(3, 60),
    "gnu": lambda: make_layer(100 + tarfile.GNU_FORMAT, 150, tarfile.GNU_FORMAT),
    "pax": lambda: make_layer(100 + tarfile.PAX_FORMAT, 150, tarfile.PAX_FORMAT),
    "ustar-prefix": tm.ustar_prefix_layer,
    "nested": tm.nested_layer,
    "pax-size": tm.pax_size_layer,
    "no-trailer": tm.no_trailer_layer,
    "empty": lambda: bytes(1024),
}


@pytest.mark.parametrize("name", list(LAYERS))
def test_layers_vs_model(L, name):
    want = _check(L, LAYERS[name]())
    if name == "l3":
        assert len(want) == 76
    if name == "nested":
        assert len(want) == 55
    if name == "empty":
        assert want == []


def test_single_block_cases(L):
    """Right only as a signed sum; right sum, field not octal; right only if the field's own bytes are not
    read as spaces; base-256 and space-padded fields; the zero block -- each alone, at every position of a
    tile, and all together among text blocks."""
    blocks = tm.kernel_blocks()
    assert {n for n, _, _ in blocks} >= {"signed-only", "non-octal", "own-bytes-not-spaces"}
    filler = (b"plain text, no header here\n" * 20)[:512]
    for name, blk, cand in blocks:
        for pos in range(8):
            data = filler * pos + blk + filler * (8 - pos)
            want = _check(L, data)
            assert [b for b, _ in want] == ([pos] if cand else []), name
    data = b"".join(blk + filler for _, blk, _ in blocks)
    want = _check(L, data)
    assert [b // 2 for b, _ in want] == [i for i, (_, _, cand) in enumerate(blocks) if cand]


def test_random_bytes_with_planted_headers(L):
    data, at = tm.planted_random()
    want = _check(L, data)
    assert [b for b, _ in want] == at and len(at) == 200


@pytest.mark.parametrize("n_blocks", [0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 127, 129])
def test_cut_layers_ignore_the_partial_block(L, n_blocks):
    """n_bytes is no multiple of 512: the partial block is ignored.  It and the bytes after it are a valid
    header, in memory in full, which a kernel reading past n_bytes / 512 blocks would report."""
    layer = make_layer(3, 60)
    poison = bytes(tm.header(b"poison/after-the-end.txt", 5))
    assert tm.is_candidate(poison)
    data = layer[:512 * n_blocks] + poison
    for extra in (1, 300, 511):
        want = _check(L, data, 512 * n_blocks + extra)
        assert all(b < n_blocks for b, _ in want)
    if n_blocks >= 3:
        assert len(want) > 0


def test_one_workgroup_strides_over_everything(L):
    data, at = tm.planted_random(seed=8, n_blocks=5000, n_planted=200)
    want = _check(L, data, grid_cap=1)
    assert [b for b, _ in want] == at
    _check(L, make_layer(3, 60) + bytes(300), 220 * 512 + 300, grid_cap=1)


def test_capacity_below_the_count(L):
    """The count is exact whatever the capacity; exactly the first `capacity` slots hold valid candidates;
    the 0xA5 guard after them is untouched (_run checks it)."""
    data = make_layer(3, 60)
    want = set(tm.candidates(data))
    assert len(want) == 76
    for cap in (0, 1, 75):
        for grid_cap in (0, 1):
            count, out = _run(L, data, capacity=cap, grid_cap=grid_cap)
            assert count == 76
            got = tm.parse_records(out, cap)
            assert len(got) == cap and got <= want


def test_set_does_not_depend_on_grid_or_capacity(L):
    rng = random.Random(2)
    data = tm.nested_layer()
    want = set(tm.candidates(data))
    for grid_cap in (1, 2, 3, 7, 0):
        cap = rng.choice([len(want), len(want) + 9])
        count, out = _run(L, data, capacity=cap, grid_cap=grid_cap)
        assert count == len(want) and tm.parse_records(out, count) == want
