"""The windows fetch's kernels (trivy_amd/csrc/fetch_windows.hip) on the GPU, through
tsg_debug_fetch_windows_device: the counters equal the host plan's and the brute-force
bitmap's, and the packed bytes equal the arena's marked granules, byte for byte --
over several staging rounds, an overflowed candidate list, and an arena whose last
granule is partial, in an allocation of exactly n_bytes + 64.
"""
import random

import numpy as np
import pytest

from tests import fetch_windows_model as fw

pytestmark = pytest.mark.gpu
NO = fw.NO_MAX_LEN


def _offsets(lens):
    o = np.zeros(len(lens) + 1, dtype=np.uint64)
    o[1:] = np.cumsum(lens)
    return o


def _arena(n, seed):
    return np.random.default_rng(seed).integers(1, 255, n, dtype=np.uint8).tobytes()


def _check(lens, recs, ml, opts=None, stage=1 << 20, cap=None, seed=0):
    offs = _offsets(lens)
    arena = _arena(int(offs[-1]), seed)
    cands = fw.cands_of(recs)
    seen = cands if cap is None else cands[:cap]  # an overflowed list: only the records written count
    bits, whole = fw.model(offs, seen, ml, opts)
    runs, views, tot = fw.model_plan(offs, bits, whole)
    assert fw.native_plan(offs, seen, ml, opts)[2] == tot
    got, ctr = fw.device_pack(arena, offs, cands, ml, opts, stage_bytes=stage, cand_cap=cap)
    assert ctr[:3] == tot[:3], (ctr, tot)
    assert ctr[3] == (tot[3] + stage // 256 * 256 - 1) // (stage // 256 * 256)
    want = fw.model_packed(arena, bits)
    assert len(got) == len(want) == tot[3]
    assert np.array_equal(got, want)
    # and every file's view reads its own bytes out of the packed buffer
    for f, lo, hi, p in views:
        fs = int(offs[f])
        assert got[p:p + hi - lo].tobytes() == arena[fs + lo:fs + hi]
    return tot


def test_edges_partial_last_granule():
    """A span across a granule boundary (arena 250-270), one at arena offset 0, one ending at the last
    byte of an arena of length 1 mod 256, file lengths that are no multiple of 16 or 256, an empty
    file between two marked ones, two 40-byte files in one granule, a marked file beside an unmarked one."""
    lens = [300, 0, 40, 40, 1000, 777, 4096 + 1 - (300 + 80 + 1000 + 777) % 256]
    assert sum(lens) % 256 == 1
    ml = [20, NO]
    recs = [(0, 0, 0, 0, 0), (0, 0, 250, 250, 0), (2, 0, 5, 5, 0), (3, 0, 20, 20, 0), (5, 0, 400, 410, 0),
            (6, 0, lens[6] - 21, lens[6] - 21, 0)]
    tot = _check(lens, recs, ml, seed=1)
    assert tot[0] >= 4 and tot[2] >= 1
    # the last file alone, marked whole: the partial granule's blocks past the arena stay unread
    _check(lens, [(6, 1, 0, lens[6], 0)], ml, opts=dict(max_span=16), seed=2)


def test_rounds_and_overflowed_list():
    rng = random.Random(5)
    lens = [rng.randint(0, 9000) for _ in range(60)]
    ml = [20, 200, NO]
    recs = []
    for _ in range(400):
        f = rng.randrange(len(lens))
        lo = rng.randint(0, lens[f])
        recs.append((f, rng.randrange(3), lo, min(lens[f], lo + rng.choice([0, 3, 40])),
                     fw.CAND_DROP if rng.random() < 0.1 else 0))
    tot = _check(lens, recs, ml, stage=4096, seed=3)
    assert tot[3] > 8 * 4096  # several rounds
    _check(lens, recs, ml, stage=256, cap=150, seed=4)  # a 1-granule stage; the list counts past its capacity


def test_nothing_everything_and_whole_marks():
    lens = [5000, 70000, 300, 0, 2500]
    ml = [20, NO]
    assert _check(lens, [], ml, seed=6)[:3] == (0, 0, 0)
    assert _check(lens, [(0, 0, 10, 20, fw.CAND_DROP)], ml, seed=6)[:3] == (0, 0, 0)
    every = [(f, 1, 0, lens[f], 0) for f in range(len(lens))]  # every file, whole (the 70000-B one by max_span)
    tot = _check(lens, every, ml, seed=7)
    assert tot[1] == 1 and tot[0] == (sum(lens) + 255) // 256
    # a whole-file mark of a file of many bitmap words beside small spans: interior words and edge words
    tot = _check([100, 1 << 20, 100], [(1, 1, 0, 1 << 20, 0), (0, 0, 50, 50, 0), (2, 0, 50, 50, 0)], ml, seed=8)
    assert tot[2] == 3  # (each 100-B file lies in one granule: its span is all of it)
