"""The two gathers of trivy_amd/csrc/xform.hip through their debug hooks, byte for byte against numpy
(tests/byte_movers_model.py): gather_kernel / copy_shifted (tsg_debug_gather_files) and
gather_host_kernel (tsg_debug_gather_host, the source in mapped host memory).  Sources and the output's
guard bytes are random, a guard of 1..16 bytes lies before every destination, and the whole output is
compared: a wrong word of the byte shift, a byte of a neighbour, a short tail or a touched guard shows."""
import numpy as np
import pytest

from tests import byte_movers_model as bm
from trivy_amd import _lib

pytestmark = pytest.mark.gpu

PIECE = bm.GATHER_PIECE


def _compare(got, want, starts, lens, dsts):
    got = np.frombuffer(got, dtype=np.uint8)
    assert len(got) == len(want)
    bad = np.nonzero(got != want)[0]
    if not len(bad):
        return
    at = int(bad[0])
    own = [i for i, (d, n) in enumerate(zip(dsts, lens)) if d - 16 <= at < d + n + 16]
    pytest.fail("%d bytes differ, first at output offsets %s (got %s want %s); files near the first: %s" % (
        len(bad), bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist(),
        [dict(i=i, src=starts[i], dst=dsts[i], length=lens[i], shift=(starts[i] - dsts[i]) & 15, phase=dsts[i] & 15,
              inside=dsts[i] <= at < dsts[i] + lens[i]) for i in own[:4]]))


def _before(dst_bytes, seed):
    return np.random.default_rng(seed).integers(0, 256, size=dst_bytes + 64, dtype=np.uint8).tobytes()


def _gather_files(case, order, tail):
    before = _before(case.dst_bytes, len(order))
    files = [case.files[i] for i in order]
    starts, lens, dsts = ([x[i] for i in order] for x in (case.starts, case.lens, case.dsts))
    got = _lib.gather_files(case.src, case.xoff, files, dsts, before, tail=tail)
    _compare(got, bm.gather_out(case.src, starts, lens, dsts, before), starts, lens, dsts)


def _gather_host(src, starts, lens, dsts, dst_bytes):
    before = _before(dst_bytes, len(starts))
    got = _lib.gather_host(src, starts, lens, dsts, before)
    _compare(got, bm.gather_out(src, starts, lens, dsts, before), starts, lens, dsts)


# ---- gather_kernel ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    case = bm.gather_table()
    bm.gather_kernel_coverage(case)  # (the asserts tests/test_byte_movers_model.py runs without a GPU)
    return case


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_gather_pairs_and_lengths(table, order):
    """All 256 ((s - d) & 15, d & 15) pairs x GATHER_LENS, the arena's first file and its last (a tail of
    the caller's behind it: the kernel may read 16 bytes of it and must store none)."""
    idx = list(range(len(table.files)))
    if order == "descending":
        idx.reverse()
    elif order == "shuffled":
        np.random.default_rng(1).shuffle(idx)
    _gather_files(table, idx, tail=b"\x5A" * 64)


def test_gather_grid_stride():
    """16,384 + 37 files of 1..3 bytes: more files than the grid has waves."""
    rng = np.random.default_rng(2)
    n = 16384 + 37
    lens = [int(x) for x in rng.integers(1, 4, size=n)]
    xoff = np.zeros(n + 1, dtype=np.uint64)
    xoff[1:] = np.cumsum(lens)
    src = rng.integers(0, 256, size=int(xoff[-1]), dtype=np.uint8).tobytes()
    order = [int(i) for i in rng.permutation(n)]
    dsts, cur = [0] * n, 0
    for pos, i in enumerate(order):  # destinations in another order than the sources, a guard byte now and then
        cur += pos % 3 == 0
        dsts[i] = cur
        cur += lens[i]
    case = bm.GatherCase(src, xoff, list(range(n)), [int(x) for x in xoff[:-1]], lens, dsts, cur + 5, None)
    _gather_files(case, list(range(n)), tail=b"\xEE" * 64)


def test_gather_nothing_listed(table):
    _gather_files(table, [], tail=b"")


# ---- gather_host_kernel -------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_tables():
    cases = [bm.host_table(0), bm.host_table(1)]
    bm.host_gather_coverage(cases)
    return cases


@pytest.mark.parametrize("part", [0, 1])
def test_host_gather_pairs_and_lengths(host_tables, part):
    """All 256 pairs x the short lengths, the lengths around 4 KiB (lane 63's extra load at the end of an
    iteration) and around the 16-KiB piece spread over them (byte_movers_model.host_table)."""
    c = host_tables[part]
    _gather_host(c.src, c.starts, c.lens, c.dsts, c.dst_bytes)


def test_host_gather_grid_stride():
    """300 small files: more items than the 128 waves of the grid."""
    rng = np.random.default_rng(3)
    cases = [(int(k), int(dp), int(ln)) for k, dp, ln in zip(rng.integers(0, 16, 300), rng.integers(0, 16, 300),
                                                               rng.integers(1, 200, 300))]
    starts, dsts, src_end, dst_end = bm.place(rng, cases, 32, 0)
    src = rng.integers(0, 256, size=src_end + 32, dtype=np.uint8).tobytes()
    _gather_host(src, starts, [c[2] for c in cases], dsts, dst_end + 3)


@pytest.mark.parametrize("length", [1, 16, 4097, PIECE + 1])
@pytest.mark.parametrize("dst", [0, 1, 15])
def test_host_gather_exact_margins(length, dst):
    """One file with exactly the 32 readable bytes the hook asks for before and after it."""
    src = np.random.default_rng(length + dst).integers(0, 256, size=32 + length + 32, dtype=np.uint8).tobytes()
    _gather_host(src, [32], [length], [dst], dst + length)
    _gather_host(src, [32], [length], [dst], dst + length + 40)


def test_host_gather_contiguous_as_the_engine_lays_out():
    """Destinations back to back from 0, as a host batch's offsets are: every file's end is the next
    one's start, the sources in tar order with a 512-B header between."""
    rng = np.random.default_rng(9)
    lens = [0, 5, 512, 1, 0, 4096, 17, PIECE + 3, 33, 0]
    starts, cur = [], 512
    for n in lens:
        starts.append(cur)
        cur += (n + 511) // 512 * 512 + 512
    src = rng.integers(0, 256, size=cur, dtype=np.uint8).tobytes()
    dsts = [int(x) for x in np.cumsum([0] + lens[:-1])]
    _gather_host(src, starts, lens, dsts, sum(lens))
