"""The files fetch of device-only batches (trivy_amd/csrc/fetch.hip) through tsg_debug_fetch_files_device,
byte for byte against tests/byte_movers_model.py: the packed layout with its padding (the staging
buffer's 0xA5 fill must survive there), the compacted list, its offsets and the counters.  Every arena is
random bytes with unmarked files between the marked ones, so a byte taken from a neighbour, a skipped
block or a short tail shows.  The hook itself fails (-4) when a round writes past its bytes."""
from bisect import bisect_right

import numpy as np
import pytest

from tests import byte_movers_model as bm
from trivy_amd import _lib

pytestmark = pytest.mark.gpu

SEG = bm.FETCH_SEG
NO_DIRECT = 1 << 62
COUNTERS = ("packed_bytes", "n_packed", "n_direct", "n_files", "file_bytes")


def _explain(got, want, plan, offsets):
    bad = np.nonzero(got != want)[0]
    at = int(bad[0])
    i = max(bisect_right(plan["lpoff"], at) - 1, 0)
    f = plan["list"][min(i, len(plan["list"]) - 1)] if plan["list"] else -1
    fs, fe = (int(offsets[f]), int(offsets[f + 1])) if f >= 0 else (0, 0)
    return ("file %d (arena phase %d, length %d, packed offset %d): %d bytes differ, first at packed offsets %s; "
            "got %s want %s" % (f, fs & 15, fe - fs, plan["lpoff"][i] if plan["list"] else 0, len(bad),
                                bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist()))


def _check(arena, offsets, marked, direct=NO_DIRECT, stage=1 << 22, copy=0, **route):
    """One hook call against the model; `route` replaces the flags by candidate records."""
    plan = bm.fetch_plan(offsets, marked, direct)
    got = _lib.fetch_files_device(arena, offsets, direct_bytes=direct, stage_bytes=stage, copy_bytes=copy,
                                  **(route or {"flags": marked}))
    assert {k: got[k] for k in COUNTERS} == {k: plan[k] for k in COUNTERS}
    assert got["list"] == plan["list"]
    assert got["lpoff"] == plan["lpoff"]
    want = bm.fetch_packed(arena, offsets, plan, copy)
    have = np.frombuffer(got["packed"], dtype=np.uint8)
    assert len(have) == len(want)
    assert np.array_equal(have, want), _explain(have, want, plan, offsets)
    size = copy or plan["packed_bytes"]
    stage = max(stage // SEG, 1) * SEG
    assert got["rounds"] == (size + stage - 1) // stage
    return got


def _batch(seed, n_files=120, big=3):
    """Random files of 0..600 bytes, about half of them marked, and a few marked ones of 16..40 KiB."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 600, size=n_files)
    lens[rng.choice(n_files, size=n_files // 8, replace=False)] = 0
    lens[rng.choice(n_files, size=big, replace=False)] = rng.integers(SEG, 40 << 10, size=big)
    offsets = np.zeros(n_files + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    arena = rng.integers(0, 256, size=int(offsets[-1]), dtype=np.uint8).tobytes()
    marked = [int(x) for x in rng.integers(0, 2, size=n_files)]
    for f in np.nonzero(lens >= SEG)[0]:
        marked[f] = 1
    return arena, offsets, marked


@pytest.fixture(scope="module")
def table():
    case = bm.fetch_table()
    bm.fetch_table_coverage(case)  # (the asserts tests/test_byte_movers_model.py runs without a GPU)
    return case


@pytest.fixture(scope="module")
def table_one_round(table):
    return _check(table.arena, table.offsets, table.marked)


# ---- every start phase x every length ------------------------------------------------------
def test_phase_length_table(table, table_one_round):
    """16 phases x FETCH_LENS, a marked file first in the arena and one last, ending at n_bytes in
    mid-block with the 0xEE tail behind it; the padding after every file is still the fill."""
    got = np.frombuffer(table_one_round["packed"], dtype=np.uint8)
    plan = bm.fetch_plan(table.offsets, table.marked, NO_DIRECT)
    assert plan["list"][0] == 0 and plan["list"][-1] == len(table.marked) - 1
    for f, p in zip(plan["list"], plan["lpoff"]):
        ln = int(table.offsets[f + 1]) - int(table.offsets[f])
        pad = got[p + ln:p + ((ln + 15) & ~15)]
        assert (pad == bm.STAGE_FILL).all(), (f, table.tags[f], pad.tolist())
    assert int(table.offsets[-1]) % 16 and len(got) == plan["lpoff"][-2] + 32  # the last file: 21 bytes, 11 of fill


def test_segment_rounds_equal_one_round(table, table_one_round):
    got = _check(table.arena, table.offsets, table.marked, stage=SEG)
    assert got["rounds"] == (got["packed_bytes"] + SEG - 1) // SEG > 80
    assert got["packed"] == table_one_round["packed"]


def test_table_with_every_file_marked(table):
    """The neighbours marked too: other packed offsets, so other segment edges inside the files."""
    _check(table.arena, table.offsets, [1] * len(table.marked), stage=4 * SEG)


# ---- copy_bytes against packed_bytes -------------------------------------------------------
@pytest.mark.parametrize("stage", [SEG, 1 << 22])
def test_copy_bytes_above_and_below(stage):
    arena, offsets, marked = _batch(3)
    size = bm.fetch_plan(offsets, marked, NO_DIRECT)["packed_bytes"]
    assert size > 3 * SEG
    # above: the extra rounds (three whole ones and a part) write nothing
    _check(arena, offsets, marked, stage=stage, copy=size + 3 * SEG + 48)
    # below: a prefix, ending inside a segment, at a segment edge, after one block
    for copy in (SEG + 4096 + 16, 2 * SEG, 16):
        _check(arena, offsets, marked, stage=stage, copy=copy)


# ---- the list search ----------------------------------------------------------------------
def test_many_tiny_files_in_one_segment():
    rng = np.random.default_rng(4)
    lens = [int(x) for x in rng.integers(1, 41, size=300)]
    offsets = np.zeros(301, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    arena = rng.integers(0, 256, size=int(offsets[-1]), dtype=np.uint8).tobytes()
    marked = [0 if i % 3 == 1 else 1 for i in range(300)]  # 200 marked: more than 64 in the first segment
    plan = bm.fetch_plan(offsets, marked, NO_DIRECT)
    assert sum(1 for p in plan["lpoff"][:-1] if p < SEG) > 64 and plan["packed_bytes"] < SEG
    _check(arena, offsets, marked)
    _check(arena, offsets, [1] * 300)


@pytest.mark.parametrize("stage", [SEG, 1 << 22])
def test_zero_length_files_at_a_segment_edge(stage):
    """Marked empty files whose packed offset is exactly a segment edge, several in a row, before the
    file that starts there; also as the list's first and last entries."""
    rng = np.random.default_rng(5)
    lens = [0, 0, SEG, 0, 0, 0, 100, 7, 0, SEG - 112, 0, 0, 2 * SEG + 5, 0]
    marked = [1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1]
    offsets = np.zeros(len(lens) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    arena = rng.integers(0, 256, size=int(offsets[-1]), dtype=np.uint8).tobytes()
    plan = bm.fetch_plan(offsets, marked, NO_DIRECT)
    assert plan["lpoff"][3:7] == [SEG] * 4 and plan["lpoff"][9:12] == [2 * SEG] * 3
    _check(arena, offsets, marked, stage=stage)


def test_nothing_everything_and_no_files():
    arena, offsets, marked = _batch(6, n_files=40, big=1)
    got = _check(arena, offsets, [0] * 40)
    assert got["packed"] == b"" and got["rounds"] == 0
    _check(arena, offsets, [0] * 40, copy=2 * SEG, stage=SEG)  # rounds over an empty layout write nothing
    _check(arena, offsets, [1] * 40)
    _check(b"", [0], [])
    _check(b"", [0], [], copy=64)
    _check(b"", [0, 0, 0], [1, 1])  # marked, all empty


# ---- the direct threshold -----------------------------------------------------------------
def test_direct_threshold():
    arena, offsets, marked = _batch(7)
    f, ln = next((i, int(offsets[i + 1]) - int(offsets[i])) for i in range(len(marked))
                 if marked[i] and 100 <= int(offsets[i + 1]) - int(offsets[i]) < SEG)
    for direct, packed in ((ln - 1, False), (ln, False), (ln + 1, True)):
        got = _check(arena, offsets, marked, direct=direct)
        assert (f in got["list"]) == packed
    small = 17  # files of 17 bytes or more go direct: most of them
    got = _check(arena, offsets, marked, direct=small)
    assert got["n_direct"] > 20 and got["n_packed"] > 0
    got = _check(arena, offsets, marked, direct=0)  # every marked file, the empty ones too
    assert got["n_packed"] == 0 and got["n_direct"] == got["n_files"] == sum(marked)


# ---- the candidate route ------------------------------------------------------------------
def test_candidate_route_equals_flags_route():
    arena, offsets, marked = _batch(8)
    n = len(marked)
    rng = np.random.default_rng(8)
    want = [f for f in range(n) if marked[f]]
    recs = [(f, int(fl)) for f in want for fl in rng.choice([0, 1, 2, 4], size=int(rng.integers(1, 4)))]  # duplicates
    recs += [(f, bm.CAND_DROP | int(rng.integers(0, 8))) for f in range(n) if not marked[f]]  # dropped: no mark
    recs += [(f, bm.CAND_DROP) for f in want[:5]]  # dropped beside a live record of the same file
    recs += [(n, 0), (n + 1, 0), (0xFFFFFFFF, 0)]  # no such file
    rng.shuffle(recs)
    recs = [(int(f), int(fl)) for f, fl in recs]
    assert bm.marked_by_candidates(recs, n) == marked
    by_flags = _check(arena, offsets, marked)
    by_cands = _check(arena, offsets, marked, cands=bm.candidate_records(recs))
    assert by_cands == by_flags
    # an overflowed list: the count says all of them, the buffer holds the first 40
    cut = bm.marked_by_candidates(recs, n, n_cands=len(recs), cand_cap=40)
    assert cut != marked and any(cut)
    by_cands = _check(arena, offsets, cut, cands=bm.candidate_records(recs), n_cands=len(recs), cand_cap=40)
    assert by_cands == _check(arena, offsets, cut)
    _check(arena, offsets, [0] * n, cands=b"")


# ---- the plan's grid strides -----------------------------------------------------------------
def test_plan_grid_strides():
    """More files than fetch_len / fetch_compact have threads (1024 x 256), and more candidate records
    than mark_files has (256 x 256): the strided passes of all three."""
    rng = np.random.default_rng(10)
    n = 1024 * 256 + 300
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(rng.integers(0, 3, size=n))
    arena = rng.integers(0, 256, size=int(offsets[-1]), dtype=np.uint8).tobytes()
    marked = [int(x) for x in rng.integers(0, 4, size=n) == 0]
    marked[-1] = marked[-2] = 1  # (files only the strided pass reaches)
    _check(arena, offsets, marked)
    few = [0] * n
    recs = [(int(f), 0) for f in rng.integers(0, 2000, size=256 * 256 + 500)]
    recs[-1] = (n - 1, 0)  # a record only the strided pass reaches marks a file nothing else does
    for f, _ in recs:
        few[f] = 1
    _check(arena, offsets, few, cands=bm.candidate_records(recs))
