"""The two kernels of trivy_amd/csrc/census.hip through their debug hooks.

transform_census (tsg_debug_transform_census): one mark per file, compared with an exact model,
`kind >= 2 or (kind == 1 and b"\\r" in data)`: a false positive counts as a failure like a miss.
gather_device (tsg_debug_gather_device): files scattered in a resident arena packed into a buffer,
compared with numpy, the bytes no file owns included; the cases hold files at source offsets below
16 with unaligned destinations, whose first aligned source block would lie before the arena.
"""
import random

import numpy as np
import pytest

from trivy_amd import _lib

pytestmark = pytest.mark.gpu

TILE = 4096
PIECE = 16384  # kGatherPiece (trivy_amd/csrc/xform.h)
CR_TAIL = b"\r" * 64


def _offsets(contents):
    offs = np.zeros(len(contents) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in contents])
    return offs


def _model(files, kinds):
    return bytes(1 if k >= 2 or (k == 1 and b"\r" in b) else 0 for b, k in zip(files, kinds))


def _census(files, kinds, tail=CR_TAIL):
    return _lib.transform_census(b"".join(files), _offsets(files), kinds, tail=tail)


def _check(files, kinds, tail=CR_TAIL):
    got, want = _census(files, kinds, tail), _model(files, kinds)
    offs = _offsets(files)
    wrong = [i for i in range(len(files)) if got[i] != want[i]]
    assert not wrong, [(i, kinds[i], int(offs[i]), len(files[i]), got[i], want[i]) for i in wrong[:10]]


# ---- 1. a hand-built batch ---------------------------------------------------
def _hand_built():
    fk = []

    def cur():
        return sum(len(b) for b, _ in fk)

    def fill_to(phase, mod, kind=1):  # a CR-free file that brings the next one to `phase` mod `mod`
        n = (phase - cur()) % mod or mod
        fk.append((b"f" * n, kind))

    named = {}
    fk.append((b"\rfirst byte", 1))
    named["cr_first"] = len(fk) - 1
    fk.append((b"last byte\r", 1))
    named["cr_last"] = len(fk) - 1
    # 1-byte b"\r" files of the four kinds inside one 16-B block, empty files between them
    fill_to(2, 16)
    named["one_block"] = len(fk)
    for k in (0, 1, 2, 3):
        fk.append((b"\r", k))
        fk.append((b"", 1))
        fk.append((b"", 0))
    assert cur() % 16 == 6
    # a CR-free kind-1 file between a kind-0 and a kind-3 file with '\r', the three in one block
    fill_to(0, 16)
    fk.append((b"ab\r", 0))
    fk.append((b"cdef", 1))
    named["squeezed"] = len(fk) - 1
    fk.append((b"\rgh\r", 3))
    assert cur() % 16 == 11
    # a kind-1 file over three 4-KiB tiles, its only '\r' the last byte
    fill_to(3000, TILE)
    start = cur()
    fk.append((b"s" * 5999 + b"\r", 1))
    named["three_tiles"] = len(fk) - 1
    assert (start + 5999) // TILE - start // TILE == 2
    # the same without the '\r' (a kind-0 neighbour with one right behind it)
    fill_to(3000, TILE)
    fk.append((b"t" * 6000, 1))
    named["three_tiles_clean"] = len(fk) - 1
    fk.append((b"\r", 0))
    # a file that starts exactly on a tile boundary; the filler before it ends there, CR-free
    fill_to(0, TILE)
    named["before_boundary"] = len(fk) - 1
    assert cur() % TILE == 0
    fk.append((b"x" * 50 + b"\r" + b"y" * 10, 1))
    named["on_boundary"] = len(fk) - 1
    # the arena's last byte
    fill_to(5, 16, kind=0)
    fk.append((b"the arena ends with\r", 1))
    named["arena_last"] = len(fk) - 1
    assert cur() % 16 != 0
    return [b for b, _ in fk], [k for _, k in fk], named


def test_census_hand_built():
    files, kinds, named = _hand_built()
    got, want = _census(files, kinds), _model(files, kinds)
    assert got == want, [(i, kinds[i], got[i], want[i]) for i in range(len(files)) if got[i] != want[i]]
    i = named["one_block"]
    assert list(got[i:i + 12:3]) == [0, 1, 1, 1] and not any(got[i + 1:i + 12:3]) and not any(got[i + 2:i + 12:3])
    for name, w in [("cr_first", 1), ("cr_last", 1), ("squeezed", 0), ("three_tiles", 1), ("three_tiles_clean", 0),
                    ("before_boundary", 0), ("on_boundary", 1), ("arena_last", 1)]:
        assert got[named[name]] == w, name
    # '\r' in the 64 bytes past n_bytes must not mark the last file
    files.append(b"no cr here")
    kinds.append(1)
    assert len(b"".join(files)) % 16 != 0
    got = _census(files, kinds, tail=CR_TAIL)
    assert got == _model(files, kinds) and got[-1] == 0


# ---- 2. random files -----------------------------------------------------------
def _random_files():
    rng = random.Random(22)
    alpha = [b"a", b"Z", b" ", b"\x00", b"\x07", b"\r", b"\n", b"\xa0", b"\x0c", b"\x0e", b"\x8d", b"pqrst",
             b"uvwxyz12"]
    files, kinds = [], []
    for _ in range(1500):
        n = rng.choice([0, 0, 1, 5, 16, 17, 100, 1000, 1023, 1024, 1025, 3000])
        # (longer files draw '\r' rarely, so that both answers stay well represented)
        pool = alpha if n <= 17 or rng.random() < 0.3 else [a for a in alpha if a != b"\r"]
        files.append(b"".join(rng.choice(pool) for _ in range(n))[:n])
        kinds.append(rng.randrange(4))
    return files, kinds


@pytest.fixture(scope="module")
def random_case():
    return _random_files()


def test_census_random_files(random_case):
    files, kinds = random_case
    want = _model(files, kinds)
    k1 = [w for w, k in zip(want, kinds) if k == 1]
    assert 100 < sum(k1) < len(k1) - 100  # both answers are well represented among the kind-1 files
    assert any(b"\r" in b and k == 0 for b, k in zip(files, kinds))
    _check(files, kinds)


# ---- 3. arena sizes --------------------------------------------------------------
@pytest.mark.parametrize("total", [1, 15, 16, 4095, 4096, 4097, (1 << 20) + 13])
def test_census_arena_sizes(total):
    rng = random.Random(total)
    # one kind-1 file: no '\r'; only the last byte; only the first byte
    _check([b"a" * total], [1])
    _check([b"a" * (total - 1) + b"\r"], [1])
    _check([b"\r" + b"a" * (total - 1)], [1])
    _check([b"\r" * total], [0])
    # cut into files at random places (the tile and block edges among them), a '\r' in about half
    for _ in range(3):
        cuts = sorted({0, total} | {rng.randrange(total + 1) for _ in range(min(total, 40))} |
                      {c for c in (15, 16, 17, 4095, 4096, 4097) if c < total})
        data = bytearray(np.random.default_rng(total).choice(np.frombuffer(b"abc \n\x0c\x0e", dtype=np.uint8),
                                                             size=total).tobytes())
        files, kinds = [], []
        for a, z in zip(cuts, cuts[1:]):
            if z > a and rng.random() < 0.5:
                data[rng.choice([a, z - 1, rng.randrange(a, z)])] = 0x0D
            files.append(bytes(data[a:z]))
            kinds.append(rng.randrange(4))
            if rng.random() < 0.2:
                files.append(b"")
                kinds.append(rng.randrange(4))
        _check(files, kinds)


def test_census_empty_batches():
    assert _lib.transform_census(b"", [0], [], tail=CR_TAIL) == b""
    assert _lib.transform_census(b"", [0, 0, 0, 0, 0], [0, 1, 2, 3], tail=CR_TAIL) == bytes([0, 0, 1, 1])


# ---- 4. the gather ---------------------------------------------------------------
def _gather(raw, src_off, lens, dst_start, tail=b"\xEE" * 64):
    """Runs the hook and compares every byte of the output with numpy."""
    dst_off = np.zeros(len(lens) + 1, dtype=np.uint64)
    dst_off[0] = dst_start
    dst_off[1:] = dst_start + np.cumsum(lens, dtype=np.uint64)
    rng = np.random.default_rng(len(raw) + 7 * dst_start + len(lens))
    before = rng.integers(0, 256, size=int(dst_off[-1]) + 64, dtype=np.uint8)
    want = before.copy()
    src = np.frombuffer(raw, dtype=np.uint8)
    for s, ln, d in zip(src_off, lens, dst_off[:-1]):
        want[int(d):int(d) + ln] = src[s:s + ln]
    got = np.frombuffer(_lib.gather_device(raw, src_off, dst_off, before.tobytes(), tail=tail), dtype=np.uint8)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (list(src_off[:4]), list(lens[:4]), dst_start, bad[:8].tolist())
    assert np.array_equal(got[int(dst_off[-1]):], before[int(dst_off[-1]):])  # past the last file: unchanged
    assert np.array_equal(got[:dst_start], before[:dst_start])


GATHER_LENS = [0, 1, 15, 16, 17, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE + 5]


@pytest.mark.parametrize("dst_start", [0, 7, 9])
def test_gather_near_the_arena_start(dst_start):
    """Files at source offsets 0, 1, 3 and 15: with destination 7 or 9 the first destination block's
    source lies before the arena (the case gather_host_kernel's `a_lo` does not allow)."""
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 256, size=15 + 2 * PIECE + 5, dtype=np.uint8).tobytes()
    for src in (0, 1, 3, 15):
        for ln in GATHER_LENS:
            _gather(raw, [src], [ln], dst_start)
        # all lengths in one call: every later file meets another destination phase
        _gather(raw, [src] * len(GATHER_LENS), GATHER_LENS, dst_start)


def test_gather_every_third_file(random_case):
    files, _ = random_case
    offs = _offsets(files)
    raw = b"".join(files)
    sel = list(range(0, len(files), 3))
    _gather(raw, [int(offs[i]) for i in sel], [len(files[i]) for i in sel], 0)
    sel = list(range(1, len(files), 3))[::-1]  # (any order of the sources)
    _gather(raw, [int(offs[i]) for i in sel], [len(files[i]) for i in sel], 9)


# ---- 5. the arena's last file -------------------------------------------------------
@pytest.mark.parametrize("n_bytes", [16 * 40, 16 * 40 + 1, 16 * 40 + 15, 2 * PIECE + 3])
def test_gather_last_file(n_bytes):
    """The selection's file ends at n_bytes, the 64 readable bytes (0xEE here) behind it."""
    rng = np.random.default_rng(n_bytes)
    raw = rng.integers(0, 256, size=n_bytes, dtype=np.uint8).tobytes()
    for ln in (1, 15, 16, 17, 33, 600):
        for dst_start in (0, 7, 9):
            _gather(raw, [n_bytes - ln], [ln], dst_start)
    _gather(raw, [0, n_bytes - 100, n_bytes - 17], [50, 100, 17], 3)
    _gather(raw, [0], [n_bytes], 5)  # the whole arena as one file
