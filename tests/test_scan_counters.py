"""What the engine grows after a scan that overflowed a list (scan_layout.h GrowOverflowed), without a GPU.

GpuEngine::Run rescans after an overflow with one list grown; which list, and to what, is a pure
function of the scan counters, the full-scan list counters and the current capacities
(tsg_debug_scan_grow).  The expected numbers below restate the rules one by one:

  records            min(n + n/4 + 4096, 0xFFFFFFF0 / 4)
  fold sites         min(n + n/4 + 1024, 0xFFFFFFF0 / 16)
  hits               min(n + n/4 + 1024, 0xFFFFFFF0 / 12)
  candidates         min(n + n/4 + 1024, 0xFFFFFFF0)
  full-scan pairs    max(cap, p + p/4 + 1024)                       (32-bit arithmetic)
  full-scan tasks    want = m + m/4 + 1024, m the largest of the four task counters;
                     cap = min(max(cap, want), kMaxTasks), kMaxTasks = 0x7FFFFFFF / 8 / 4;
                     want > kMaxTasks: the lane task size doubles while it is below 2^26 and
                     want * size_before / size > kMaxTasks

in the order records, full-scan lists, fold sites, hits, candidates, one list per call.
"""
import ctypes as c

import pytest

from tests.stage_model import (CT_CAND_OVF, CT_CANDS, CT_FOLD_OVF, CT_FOLDS, CT_FS_OVF, CT_HIT_OVF, CT_HITS,
                               CT_REC_OVF, CT_RECS, CTR_WORDS)
from trivy_amd import _lib

HIT, CAND, REC, FOLD, FS_PAIR, FS_TASK, FS_TASK_BYTES = range(7)   # tsg_debug_scan_grow's caps
NONE, RECS, FULLSCAN, FOLDS, HITS, CANDS = range(6)                # ... and its return value
FS_TASKS = 1                                                       # kFsTasks (fs: pairs, 4 x tasks, wave pairs)
MAX_TASKS = 0x7FFFFFFF // 8 // 4
CAPS0 = [1 << 16, 1 << 16, 1 << 17, 1 << 16, 1 << 14, 1 << 16, 4096]
# (flag slot, count slot, capacity, slack, bytes per record, return value)
LISTS = [(CT_REC_OVF, CT_RECS, REC, 4096, 4, RECS), (CT_FOLD_OVF, CT_FOLDS, FOLD, 1024, 16, FOLDS),
         (CT_HIT_OVF, CT_HITS, HIT, 1024, 12, HITS), (CT_CAND_OVF, CT_CANDS, CAND, 1024, 1, CANDS)]


def grow(counters, fs=None, caps=None):
    L = _lib.lib()
    L.tsg_debug_scan_grow.restype = c.c_int
    L.tsg_debug_scan_grow.argtypes = [c.POINTER(c.c_uint32)] * 3
    assert len(counters) == CTR_WORDS
    cnt = (c.c_uint32 * CTR_WORDS)(*counters)
    fc = (c.c_uint32 * 6)(*(fs or [0] * 6))
    cp = (c.c_uint32 * 7)(*(caps or CAPS0))
    which = L.tsg_debug_scan_grow(cnt, fc, cp)
    assert list(cnt) == list(counters)  # inputs
    return which, list(cp)


def counts(slots):
    cnt = [0] * CTR_WORDS
    for k, v in slots.items():
        cnt[k] = v
    return cnt


def with_cap(i, v, caps=CAPS0):
    return [v if k == i else x for k, x in enumerate(caps)]


def test_no_flag_nothing_grows():
    cnt = [0xFFFFFFFF] * CTR_WORDS  # counts (and the unused slots) alone do not grow anything
    for flag in (CT_HIT_OVF, CT_CAND_OVF, CT_FS_OVF, CT_REC_OVF, CT_FOLD_OVF):
        cnt[flag] = 0
    assert grow(cnt, fs=[0xFFFFFFFF] * 6) == (NONE, CAPS0)
    assert grow([0] * CTR_WORDS) == (NONE, CAPS0)


@pytest.mark.parametrize("flag,count,cap,slack,rec_bytes,code", LISTS)
def test_each_flag_grows_its_own_list(flag, count, cap, slack, rec_bytes, code):
    clamp = 0xFFFFFFF0 // rec_bytes
    below = 1000003
    at = clamp - clamp // 5  # n + n/4 passes the clamp: the list cannot hold a quarter more
    for n, want in ((below, below + below // 4 + slack), (at, clamp), (clamp, clamp), (0xFFFFFFFF, clamp),
                    (0, slack)):  # (to the count seen: a larger capacity than needed shrinks)
        assert n + n // 4 + slack >= want
        cnt = [0] * CTR_WORDS
        cnt[flag], cnt[count] = 1, n
        assert grow(cnt) == (code, with_cap(cap, want)), n


def test_fullscan_flag_grows_the_fullscan_lists():
    cnt = counts({CT_FS_OVF: 1})
    p, m = 300001, 200003
    which, caps = grow(cnt, fs=[p, m, 5, 0, 7, 99])
    assert which == FULLSCAN
    assert caps == with_cap(FS_PAIR, p + p // 4 + 1024, with_cap(FS_TASK, m + m // 4 + 1024))
    # counts below the capacities: they stay (max with the current capacity), wave pairs do not count
    assert grow(cnt, fs=[10, 10, 10, 10, 10, 0xFFFFFFFF]) == (FULLSCAN, CAPS0)
    # the pair capacity is computed in 32 bits
    p = 0xFFFFFFFF
    assert grow(cnt, fs=[p, 0, 0, 0, 0, 0])[1][FS_PAIR] == max(CAPS0[FS_PAIR], (p + p // 4 + 1024) & 0xFFFFFFFF)


@pytest.mark.parametrize("w", range(4))
def test_fullscan_takes_the_largest_task_counter(w):
    fs = [0, 70001, 70002, 70003, 70004, 0]
    fs[FS_TASKS + w] = 900001
    which, caps = grow(counts({CT_FS_OVF: 1}), fs=fs)
    assert which == FULLSCAN and caps[FS_TASK] == 900001 + 900001 // 4 + 1024
    assert caps[FS_TASK_BYTES] == CAPS0[FS_TASK_BYTES]


def test_several_flags_one_list_per_call_in_order():
    cnt = counts({CT_HITS: 500000, CT_CANDS: 400000, CT_RECS: 3000000, CT_FOLDS: 600000, CT_HIT_OVF: 1, CT_CAND_OVF: 1,
                  CT_FS_OVF: 1, CT_REC_OVF: 1, CT_FOLD_OVF: 1})
    fs = [300000, 1, 2, 800000, 3, 0]
    caps = list(CAPS0)
    order = [(RECS, CT_REC_OVF, {REC: 3000000 + 750000 + 4096}),
             (FULLSCAN, CT_FS_OVF, {FS_PAIR: 300000 + 75000 + 1024, FS_TASK: 800000 + 200000 + 1024}),
             (FOLDS, CT_FOLD_OVF, {FOLD: 600000 + 150000 + 1024}),
             (HITS, CT_HIT_OVF, {HIT: 500000 + 125000 + 1024}),
             (CANDS, CT_CAND_OVF, {CAND: 400000 + 100000 + 1024})]
    for code, flag, changed in order:
        which, new = grow(cnt, fs=fs, caps=caps)
        assert which == code
        assert new == [changed.get(i, x) for i, x in enumerate(caps)]  # this list and no other
        caps = new
        cnt[flag] = 0  # the rescan with the grown list
    assert grow(cnt, fs=fs, caps=caps) == (NONE, caps)


def _task_bytes(m, tb0):
    want = m + m // 4 + 1024
    tb = tb0
    if want > MAX_TASKS:
        while tb < (1 << 26) and want * tb0 // tb > MAX_TASKS:
            tb *= 2
    return tb


@pytest.mark.parametrize("m,tb0,tb", [
    (MAX_TASKS - MAX_TASKS // 5 - 1024, 4096, 4096),  # want <= kMaxTasks: the lists grow, the size stays
    (MAX_TASKS, 4096, 8192),                          # want = 1.25 x kMaxTasks: one doubling
    (0xFFFFFFFF, 4096, 4096 * 128),                   # want = 80.0 x kMaxTasks
    (0xFFFFFFFF, 1 << 25, 1 << 26),                   # stops at 2^26
    (0xFFFFFFFF, 1 << 26, 1 << 26),
    (0xFFFFFFFF, 100 << 20, 100 << 20),               # (a configured size above it stays)
])
def test_fullscan_coarser_tasks_when_the_lists_cannot_grow(m, tb0, tb):
    assert _task_bytes(m, tb0) == tb
    want = m + m // 4 + 1024
    which, caps = grow(counts({CT_FS_OVF: 1}), fs=[0, 0, m, 0, 0, 0], caps=with_cap(FS_TASK_BYTES, tb0))
    assert which == FULLSCAN
    assert caps == with_cap(FS_TASK_BYTES, tb, with_cap(FS_TASK, min(max(CAPS0[FS_TASK], want), MAX_TASKS)))
