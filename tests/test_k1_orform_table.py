"""K1's OR-form table (trivy_amd/csrc/k1_orform.h) without a GPU.

The filter kernel's default form evaluates a window as an OR of slot masks read
from a re-laid copy of the reach table.  tsg_debug_filter_orform returns the
256 x 4 row that every replica of the kernel's LDS image holds:

  m_s[b]  bit j = bit 4 s + j % 4 of reach[b][j // 4]   (16 buckets, slot s "not allowed")
  W_k[b]  = m_{2k+1}[b] << 16 | m_{2k}[b]               (k = 0..2; slots 6-7 dropped)
  W_3[b]  = 1 for b == '\\n' only (the newline bucket's slot-0 bit is 0)

Checked bit for bit against a Python re-layout of FilterModel's reach table for
the builtin rules, a calibrated compile and the class-run rule set; and the OR
form itself -- H_p = W_0[b_{p-4}] | W_1[b_{p-2}] | W_2[b_p], fire word
hi(H_p) | lo(H_{p-1}), a zero bit among buckets 0..14 fires -- is evaluated on
64 KiB of seeded bytes with planted windows against the model's flagged blocks
and newline counts.
"""
import ctypes as c
import random

import numpy as np
import pytest

from tests import stage_cases as sc
from tests.filter_model import FilterModel
from tests.stage_model import Batch, StageModel
from trivy_amd import _lib
from trivy_amd.secret import builtin_rules


def relayout(reach):
    """The issue's formulas on a [256, 4] u32 reach table -> [256, 4] u32."""
    reach = np.asarray(reach, dtype=np.uint64)
    m = np.zeros((8, 256), dtype=np.uint64)
    for s in range(8):
        for r in range(4):
            m[s] |= ((reach[:, r] >> np.uint64(4 * s)) & np.uint64(0xF)) << np.uint64(4 * r)
    out = np.zeros((256, 4), dtype=np.uint32)
    for k in range(3):
        out[:, k] = (m[2 * k + 1] << np.uint64(16) | m[2 * k]).astype(np.uint32)
    out[:, 3] = ((~reach[:, 3] >> np.uint64(3)) & np.uint64(1)).astype(np.uint32)
    return out


def orform_table(fm):
    L = _lib.lib()
    L.tsg_debug_filter_orform.argtypes = [c.c_void_p, c.c_void_p]
    out = np.zeros((256, 4), dtype=np.uint32)
    assert L.tsg_debug_filter_orform(fm.h, out.ctypes.data) == 0
    return out


def orform_eval(W, a):
    """(fire word per position [n] u16, newlines [n] u8) of byte stream `a`, zero bytes before it."""
    a = np.concatenate([np.zeros(5, dtype=np.uint8), np.asarray(a, dtype=np.uint8)])
    n = len(a) - 5
    p = np.arange(4, n + 5)                                 # H_{-1} .. H_{n-1}
    H = W[a[p - 4], 0] | W[a[p - 2], 1] | W[a[p], 2]
    F = (H[1:] >> 16) | (H[:-1] & 0xFFFF)
    return F.astype(np.uint16), W[a[5:], 3].astype(np.uint8)


_FMS = {}


def _fm(kind):
    if kind not in _FMS:
        if kind == "builtin":
            _FMS[kind] = FilterModel(builtin_rules())
        elif kind == "calibrated":
            from tests.test_filter_model import _calibration_sample
            _FMS[kind] = FilterModel(builtin_rules(), calibration=_calibration_sample(0))
            assert _FMS[kind].n_calibrated >= 1
        else:
            _FMS[kind] = FilterModel(sc.class_run_rules())
    return _FMS[kind]


@pytest.mark.parametrize("kind", ["builtin", "calibrated", "class-runs"])
def test_table_is_the_relayout_of_reach(kind):
    fm = _fm(kind)
    assert (fm.n_buckets, fm.n_words) == (16, 4) and fm.window <= 6
    W = orform_table(fm)
    assert np.array_equal(W, relayout(fm.reach))
    # the shape the kernel relies on: only '\n' counts, and the newline bucket (bit 15 of a fire word)
    # can never fire -- its slots 4-5 allow nothing
    assert W[:, 3].sum() == 1 and W[ord("\n"), 3] == 1
    assert ((W[:, 2] >> 15) & 1).all() and ((W[:, 2] >> 31) & 1).all()
    # slot s of bucket j, bit for bit, against FilterModel.allowed
    for j in range(16):
        for s in range(6):
            bit = (W[:, s // 2] >> np.uint32(16 * (s % 2) + j)) & 1
            assert np.array_equal(bit == 0, fm.allowed(j, s)), (j, s)


def _planted(seed, n):
    rng = random.Random(seed)
    p = sc.Planter(n)
    k = 0
    while k < 160:
        if p.put(rng.randrange(0, n - 64), sc.TOKENS[k % 4](rng)):
            k += 1
    a = bytearray(p.buf)
    for _ in range(64):  # arbitrary bytes too, 0x00 and 0xFF among them
        at = rng.randrange(0, n - 16)
        a[at:at + 16] = bytes(rng.choice([0, 255, 10, rng.randrange(256)]) for _ in range(16))
    return bytes(a)


@pytest.mark.parametrize("kind", ["builtin", "calibrated", "class-runs"])
def test_orform_fires_equal_the_model(kind):
    fm = _fm(kind)
    W = orform_table(fm)
    a = np.frombuffer(_planted(11, 64 * 1024), dtype=np.uint8)
    F, nl = orform_eval(W, a)
    fires = fm.fires(a)  # [bucket, position], zero bytes before the stream
    got = ((F[None, :] >> np.arange(16, dtype=np.uint16)[:, None]) & 1) == 0
    assert np.array_equal(got, fires)
    assert not got[15].any()
    blocks = np.unique(np.nonzero(got[:15].any(axis=0))[0] >> 4)
    assert len(blocks) >= 150  # the planted windows fire
    # a block is flagged iff the AND of its 16 fire words is not all ones: the kernel's test
    acc = np.bitwise_and.reduce(F.reshape(-1, 16), axis=1)
    assert np.array_equal(np.nonzero(acc != 0xFFFF)[0], blocks)
    assert np.array_equal(nl, (a == 10).astype(np.uint8))


def test_orform_blocks_equal_the_stage_model():
    """... and StageModel.flagged_blocks / nl_counts, the expectation of the GPU stage tests, on an arena
    that ends inside a tile (the kernel zeroes the rest of the tile)."""
    model = StageModel(builtin_rules())
    body = _planted(12, 64 * 1024 - 1234)
    b = Batch([body])
    W = orform_table(model.fm)
    pad = (-b.n_bytes) % 4096
    F, nl = orform_eval(W, np.concatenate([b.a, np.zeros(pad, dtype=np.uint8)]))
    acc = np.bitwise_and.reduce(F.reshape(-1, 16), axis=1)
    assert np.array_equal(np.nonzero(acc != 0xFFFF)[0].astype(np.uint32), model.flagged_blocks(b))
    want_nl = model.nl_counts(b)  # one per 1-KiB chunk that holds arena bytes; the zeroed rest holds no newline
    per_kib = nl.reshape(-1, 1024).sum(axis=1).astype(np.uint16)
    assert np.array_equal(per_kib[:len(want_nl)], want_nl) and not per_kib[len(want_nl):].any()
