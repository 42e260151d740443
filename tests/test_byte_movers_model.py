"""The byte movers' CPU models against bytes written out by hand, the coverage of the GPU tests' case
tables (tests/byte_movers_model.py), and the debug hooks' refusals, which precede every HIP call."""
import numpy as np
import pytest

from tests import byte_movers_model as bm
from trivy_amd import _lib

SEG = bm.FETCH_SEG
PIECE = bm.GATHER_PIECE
P = b"\xA5"  # the staging buffer's fill


# ---- 1. the models on layouts written out literally ---------------------------------------
def test_fetch_model_hand_written():
    arena = b"AAA" + b"bbbbb" + b"CCCCCCCCCCCCCCCCD" + b"" + b"EE" + b"ff"
    offsets = [0, 3, 8, 25, 25, 27, 29]
    marked = [1, 0, 1, 1, 1, 0]
    plan = bm.fetch_plan(offsets, marked, 1 << 62)
    assert plan == dict(list=[0, 2, 3, 4], lpoff=[0, 16, 48, 48, 64], packed_bytes=64, n_packed=4, n_direct=0,
                        n_files=4, file_bytes=22)
    want = b"AAA" + P * 13 + b"CCCCCCCCCCCCCCCCD" + P * 15 + b"EE" + P * 14
    assert bm.fetch_packed(arena, offsets, plan).tobytes() == want
    assert bm.fetch_packed(arena, offsets, plan, 32).tobytes() == want[:32]
    assert bm.fetch_packed(arena, offsets, plan, 96).tobytes() == want + P * 32
    # the 17-byte file at the direct threshold: counted, not packed
    plan = bm.fetch_plan(offsets, marked, 17)
    assert plan == dict(list=[0, 3, 4], lpoff=[0, 16, 16, 32], packed_bytes=32, n_packed=3, n_direct=1, n_files=4,
                        file_bytes=22)
    assert bm.fetch_packed(arena, offsets, plan).tobytes() == b"AAA" + P * 13 + b"EE" + P * 14
    plan = bm.fetch_plan(offsets, marked, 18)
    assert plan["list"] == [0, 2, 3, 4] and plan["n_direct"] == 0


def test_candidate_marks_hand_written():
    recs = [(2, 0), (2, 0), (1, bm.CAND_DROP), (9, 0), (0, 1), (3, 0)]
    assert bm.marked_by_candidates(recs, 4) == [1, 0, 1, 1]
    assert bm.marked_by_candidates(recs, 4, n_cands=6, cand_cap=4) == [0, 0, 1, 0]  # only the records written
    raw = bm.candidate_records(recs)
    assert len(raw) == 64 * len(recs)
    assert raw[64 * 2:64 * 2 + 4] == b"\x01\0\0\0" and raw[64 * 2 + 32:64 * 2 + 36] == b"\x08\0\0\0"


def test_gather_model_hand_written():
    src = b"0123456789abcdefghij"
    before = b"." * 20
    got = bm.gather_out(src, [2, 10], [3, 5], [1, 9], before).tobytes()
    assert got == b".234.....abcde......"
    # any order, an empty file, two files that touch
    got = bm.gather_out(src, [15, 0, 7], [5, 2, 0], [2, 0, 11], before).tobytes()
    assert got == b"01fghij............."
    assert before == b"." * 20  # (the input is left alone)


def test_branch_helpers_hand_checked():
    assert bm.fetch_branch_of(0, 16, 0, 0) == "aligned"
    assert bm.fetch_branch_of(32, 17, 0, 1) == "tail"
    # a file at arena offset 5: block 0's aligned pair starts before it, block 5's ends past it
    assert [bm.fetch_branch_of(5, 100, 0, b) for b in range(7)] == \
        ["bytes", "shift_q1", "shift_q1", "shift_q1", "shift_q1", "bytes", "tail"]
    # the same file over a segment edge: the second item is a call of its own with the same phase
    assert bm.fetch_branch_of(5, 100, SEG - 32, 2) == "shift_q1"
    assert bm.fetch_branch_of(14, 64, 0, 1) == "shift_q3"
    assert [bm.shifted_branch_of(3, 40, 5, b) for b in range(3)] == ["ragged", "shift_q3", "ragged"]
    assert bm.shifted_branch_of(16, 16, 32, 0) == "shift_q0"
    assert bm.host_branch_of(33, 8192, 32, 0, 255) == bm.HostBranch("full", "q0r1", "ex")
    assert bm.host_branch_of(32, 8192, 32, 0, 63) == bm.HostBranch("full", "aligned", "readlane")
    assert bm.host_branch_of(39, PIECE + 3, 34, 1, 0) == bm.HostBranch("ragged", "q1r1", "shfl")
    assert bm.blocks_of(15, 2) == 2 and bm.blocks_of(16, 16) == 1 and bm.blocks_of(3, 0) == 0


# ---- 2. the GPU tests' case tables reach what they are for -----------------------------------
def test_fetch_table_coverage():
    case = bm.fetch_table()
    assert len(case.arena) <= 2 << 20
    seen = bm.fetch_table_coverage(case)
    assert len(seen) == 2 + 15 * 3
    # every (phase, length) is a marked file with an unmarked neighbour before it
    assert {case.tags[f] for f in case.tags} >= {(ph, ln) for ph in range(16) for ln in bm.FETCH_LENS}
    for f, (ph, ln) in case.tags.items():
        assert case.marked[f] and int(case.offsets[f]) & 15 == ph
        assert int(case.offsets[f + 1]) - int(case.offsets[f]) == ln
        assert f == 0 or not case.marked[f - 1]


def test_gather_table_coverage():
    case = bm.gather_table()
    assert len(case.src) + case.dst_bytes <= 3 << 20
    bm.gather_kernel_coverage(case)
    assert case.starts[0] == 0 and case.starts[-1] + case.lens[-1] == len(case.src)  # the arena's first and last


def test_host_table_coverage():
    cases = [bm.host_table(0), bm.host_table(1)]
    for c in cases:
        assert len(c.src) <= 2 << 20
        assert min(c.starts) >= 32 and max(s + n for s, n in zip(c.starts, c.lens)) + 32 <= len(c.src)
    bm.host_gather_coverage(cases)


def test_coverage_asserts_notice_a_gap():
    case = bm.fetch_table()
    unmarked = [0 if case.tags.get(f) == (7, 48) else m for f, m in enumerate(case.marked)]
    with pytest.raises(AssertionError):
        bm.fetch_table_coverage(case._replace(marked=unmarked))
    g = bm.gather_table()
    keep = [i for i, t in enumerate(g.tags) if t != (9, 4)]
    with pytest.raises(AssertionError):
        bm.gather_kernel_coverage(g._replace(starts=[g.starts[i] for i in keep], lens=[g.lens[i] for i in keep],
                                             dsts=[g.dsts[i] for i in keep], tags=[g.tags[i] for i in keep]))
    with pytest.raises(AssertionError):
        bm.host_gather_coverage([bm.host_table(0)])


# ---- 3. the hooks refuse before they touch HIP --------------------------------------------
def test_fetch_hook_refusals():
    arena = bytes(range(64))
    for offsets, kw, why in (([1, 64], {}, "start at 0"),
                             ([0, 40, 30, 64], {}, "ascend"),
                             ([0, 63], {}, "end at n_bytes"),
                             ([0, 64], {"copy_bytes": 24}, "multiple of 16")):
        with pytest.raises(_lib.HookRefused, match=why):
            _lib.fetch_files_device(arena, offsets, flags=[1] * (len(offsets) - 1), **kw)
    with pytest.raises(_lib.HookRefused, match="more candidates"):
        _lib.fetch_files_device(arena, [0, 64], cands=bm.candidate_records([(0, 0)]), n_cands=1 << 32, cand_cap=1)


def test_gather_files_hook_refusals():
    src, out = bytes(range(100)), bytes(40 + 64)
    xoff = [0, 10, 30, 100]
    for xo, files, dst, why in ((xoff, [3], [0], "no such file"),
                                ([0, 30, 10, 100], [0], [0], "ascend"),
                                ([0, 10, 30, 101], [0], [0], "leaves the arena"),
                                (xoff, [1], [21], "leaves the output"),
                                (xoff, [0, 1], [5, 14], "overlap")):
        with pytest.raises(_lib.HookRefused, match=why):
            _lib.gather_files(src, xo, files, dst, out)


def test_gather_host_hook_refusals():
    src, out = bytes(200), bytes(100 + 64)
    for so, ln, dst, why in (([31], [10], [0], "32 readable bytes"),
                             ([32], [137], [0], "32 readable bytes"),   # 32 + 137 + 32 > 200
                             ([168], [1], [0], "32 readable bytes"),
                             ([0], [0], [0], "32 readable bytes"),      # an empty file is held to it too
                             ([40], [50], [51], "leaves the output"),
                             ([40, 100], [20, 20], [0, 19], "overlap")):
        with pytest.raises(_lib.HookRefused, match=why):
            _lib.gather_host(src, so, ln, dst, out)
