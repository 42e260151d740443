"""CPU models of the three kernels that only move file bytes, and the case tables of their GPU tests.

  files fetch   fetch.hip   mark_files / fetch_len / fetch_compact / fetch_files_kernel (FetchPlan, FetchPack)
  gather        xform.hip   gather_kernel / copy_shifted (GatherFiles)
  host gather   xform.hip   gather_host_kernel (GatherHostFiles)

The models (numpy only) say what the bytes must be: plain slices, no alignment logic.  The *_branch_of
helpers restate which path of the kernel's copy a 16-B block takes -- they are not used to compute any
expected byte, only to assert that a case table reaches every path (tests/test_byte_movers_model.py runs
the same asserts without a GPU).
"""
import struct
from collections import namedtuple

import numpy as np

FETCH_SEG = 16384     # trivy_amd/csrc/fetch.h kFetchSeg
GATHER_PIECE = 16384  # trivy_amd/csrc/xform.h kGatherPiece
STAGE_FILL = 0xA5     # what tsg_debug_fetch_files_device fills the staging buffer with
CAND_DROP = 8         # trivy_amd/csrc/engine.h kCandDrop


# ---- models -------------------------------------------------------------------------
def candidate_records(recs):
    """64-B Candidate records (engine.h) of (file, flags) pairs; the other fields are arbitrary."""
    return b"".join(struct.pack("<IIqqqI3I3II", f, 7, 1, 2, 3, fl, 4, 5, 6, 7, 8, 9, 0) for f, fl in recs)


def marked_by_candidates(recs, n_files, n_cands=None, cand_cap=None):
    """The files mark_files_kernel marks: those of the records written (an overflowed list counts past
    its capacity) that are not kCandDrop and name a file of the batch."""
    n = len(recs) if n_cands is None else n_cands
    if cand_cap is not None:
        n = min(n, cand_cap)
    marked = [0] * n_files
    for f, fl in recs[:n]:
        if f < n_files and not fl & CAND_DROP:
            marked[f] = 1
    return marked


def fetch_plan(offsets, marked, direct_bytes):
    """What FetchPlan leaves: the compacted list, its packed offsets and the FetchCounters fields."""
    lst, lpoff, p = [], [], 0
    r = dict(n_direct=0, n_files=0, file_bytes=0)
    for f, m in enumerate(marked):
        if not m:
            continue
        ln = int(offsets[f + 1]) - int(offsets[f])
        r["n_files"] += 1
        r["file_bytes"] += ln
        if ln >= direct_bytes:
            r["n_direct"] += 1
            continue
        lst.append(f)
        lpoff.append(p)
        p += (ln + 15) & ~15
    lpoff.append(p)
    r.update(list=lst, lpoff=lpoff, packed_bytes=p, n_packed=len(lst))
    return r


def fetch_packed(arena, offsets, plan, copy_bytes=0):
    """Bytes [0, copy_bytes or packed_bytes) of the packed layout; padding and everything past
    packed_bytes is the staging buffer's fill."""
    src = np.frombuffer(arena, dtype=np.uint8)
    full = np.full(plan["packed_bytes"], STAGE_FILL, dtype=np.uint8)
    for f, p in zip(plan["list"], plan["lpoff"]):
        a, z = int(offsets[f]), int(offsets[f + 1])
        full[p:p + z - a] = src[a:z]
    if not copy_bytes:
        return full
    out = np.full(copy_bytes, STAGE_FILL, dtype=np.uint8)
    n = min(copy_bytes, len(full))
    out[:n] = full[:n]
    return out


def gather_out(src, starts, lens, dsts, before):
    """`before` with src[starts[i] .. + lens[i]) written at dsts[i] (either gather)."""
    s = np.frombuffer(src, dtype=np.uint8)
    want = np.array(np.frombuffer(before, dtype=np.uint8))
    for a, n, d in zip(starts, lens, dsts):
        want[d:d + n] = s[a:a + n]
    return want


# ---- which path a block takes -----------------------------------------------------------
def fetch_branch_of(fs, length, p0, block):
    """fetch_copy's path for the 16-B block `block` of a file that starts at arena offset fs and packed
    offset p0: 'aligned' (one load), 'shift_q0'..'shift_q3' (two loads and the byte shift), 'bytes' (the
    aligned pair would leave the file) or 'tail' (the ragged last block)."""
    fe = fs + length
    pos = p0 + 16 * block                      # the block's packed offset
    lo = pos // FETCH_SEG * FETCH_SEG          # its segment: a wave's work item
    a, z = max(lo, p0), min(lo + FETCH_SEG, p0 + length)
    s, n, j = fs + (a - p0), z - a, pos - a    # fetch_copy(src, s, fs, fe, dst, a - w0, n), block at j
    assert 0 <= j < n
    if j + 16 > n:
        return "tail"
    k = s & 15
    if k == 0:
        return "aligned"
    sa = (s + j) & ~15
    return "shift_q%d" % (k >> 2) if sa >= fs and sa + 32 <= fe else "bytes"


def fetch_paths_of_phase(k):
    """The paths a file that starts at phase k can take."""
    return {"aligned", "tail"} if k == 0 else {"shift_q%d" % (k >> 2), "bytes", "tail"}


def shifted_branch_of(s, length, d, block):
    """copy_shifted's path for destination block `block` (counted from d & ~15) of a file copied from
    source offset s to destination d: 'shift_q0'..'shift_q3' (a whole block: two loads and the byte
    shift, by (s - d) & 15) or 'ragged' (the first / last block: byte by byte)."""
    e, y0 = d + length, (d & ~15) + 16 * block
    assert length and y0 < e
    return "shift_q%d" % (((s - d) & 15) >> 2) if y0 >= d and y0 + 16 <= e else "ragged"


HostBranch = namedtuple("HostBranch", "store shift nxt")


def host_branch_of(s, length, d, piece, block):
    """gather_host_kernel's path for destination block `block` (counted from d0 & ~15) of item `piece`:
    store 'full' or 'ragged'; shift 'aligned' ((s - d) & 15 == 0: the low words alone) or 'q<n>r<m>';
    nxt, where the block's upper source words come from: 'shfl' (the next lane), 'readlane' (lane 63:
    lane 0 of the next group of 64) or 'ex' (lane 63 of the last group: the extra load)."""
    d0 = d + piece * GATHER_PIECE
    d1 = min(d + length, d0 + GATHER_PIECE)
    B = (d0 & ~15) + 16 * block
    assert d0 < d1 and B < d1
    r = (s - d) & 15
    jj = block % 256
    nxt = "shfl" if jj % 64 != 63 else ("readlane" if jj != 255 else "ex")
    return HostBranch("full" if B >= d0 and B + 16 <= d1 else "ragged",
                      "aligned" if r == 0 else "q%dr%d" % (r >> 2, r & 3), nxt)


def blocks_of(d, length):
    """How many 16-B destination blocks [d, d + length) touches."""
    return 0 if not length else ((d + length + 15) >> 4) - (d >> 4)


# ---- case tables ------------------------------------------------------------------------
FETCH_LENS = [0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 1023, 1024, 1025, FETCH_SEG - 1, FETCH_SEG, FETCH_SEG + 1,
              2 * FETCH_SEG + 5]
GATHER_LENS = [0, 1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 2049]
HOST_SHORT = [0, 1, 15, 16, 17]
HOST_MID = [4095, 4096, 4097, 4111, 4112]
HOST_BIG = [GATHER_PIECE - 1, GATHER_PIECE, GATHER_PIECE + 1, 2 * GATHER_PIECE + 5]
HOST_LENS = HOST_SHORT + HOST_MID + HOST_BIG

FetchCase = namedtuple("FetchCase", "arena offsets marked tags")


def fetch_table(seed=11):
    """Every start phase x every length of FETCH_LENS as a marked file, an unmarked file of 1..16 random
    bytes before each (it sets the phase, and a byte of it that leaked would show); a marked file is the
    arena's first, and the last ends at n_bytes in mid-block.  tags[f]: (phase, length) of a marked file."""
    rng = np.random.default_rng(seed)
    lens, marked, tags = [33], [1], {0: (0, 33)}
    cur = 33
    order = [(ph, ln) for ln in FETCH_LENS for ph in range(16)]
    rng.shuffle(order)  # the long files spread over the layout, so every phase meets segment edges
    for ph, ln in order + [(5, 21)]:
        gap = (ph - cur) % 16 or 16
        lens += [gap, ln]
        marked += [0, 1]
        tags[len(lens) - 1] = (int(ph), int(ln))
        cur += gap + ln
    offsets = np.zeros(len(lens) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    assert int(offsets[-1]) % 16 != 0 and marked[-1]
    arena = rng.integers(0, 256, size=int(offsets[-1]), dtype=np.uint8).tobytes()
    return FetchCase(arena, offsets, marked, tags)


def fetch_table_coverage(case, direct_bytes=1 << 62):
    """Asserts that the table reaches what it is for; returns the (phase, path) pairs seen."""
    plan = fetch_plan(case.offsets, case.marked, direct_bytes)
    seen, lens_at, edges = set(), set(), {}
    for f, p0 in zip(plan["list"], plan["lpoff"]):
        fs, ln = int(case.offsets[f]), int(case.offsets[f + 1]) - int(case.offsets[f])
        ph = fs & 15
        lens_at.add((ph, ln))
        if ln:
            edges.setdefault(ph, set()).add((p0 + ln - 1) // FETCH_SEG - p0 // FETCH_SEG)
        for b in range(blocks_of(0, ln)):
            seen.add((ph, fetch_branch_of(fs, ln, p0, b)))
    for ph in range(16):
        missing = {(ph, x) for x in fetch_paths_of_phase(ph)} - seen
        assert not missing, "fetch table: paths not reached: %s" % sorted(missing)
        absent = [ln for ln in FETCH_LENS if (ph, ln) not in lens_at]
        assert not absent, "fetch table: phase %d lacks lengths %s" % (ph, absent)
        assert {1, 2} <= edges[ph], "fetch table: phase %d straddles %s edges" % (ph, edges[ph])
    return seen


GatherCase = namedtuple("GatherCase", "src xoff files starts lens dsts dst_bytes tags")


def place(rng, pairs_lens, src_cur, dst_cur):
    """Source starts and destinations for (k, dp, length) cases: (s - d) & 15 == k and d & 15 == dp, a
    source gap of 0..15 bytes and a destination guard of 1..16 bytes before each file."""
    starts, dsts = [], []
    for k, dp, ln in pairs_lens:
        dst_cur += (dp - dst_cur - 1) % 16 + 1
        src_cur += (k + dp - src_cur) % 16
        starts.append(src_cur)
        dsts.append(dst_cur)
        src_cur += ln
        dst_cur += ln
    return starts, dsts, src_cur, dst_cur


def gather_table(seed=12):
    """gather_kernel: all 256 ((s - d) & 15, d & 15) pairs x GATHER_LENS.  The sources are files of one
    arena (the gaps are files of it too, not listed); its first file and its last are listed."""
    rng = np.random.default_rng(seed)
    cases = [(k, dp, ln) for ln in GATHER_LENS for k in range(16) for dp in range(16)]
    rng.shuffle(cases)
    cases = [(0, 0, 40)] + [tuple(int(x) for x in c) for c in cases] + [(3, 6, 23)]
    starts, dsts, src_end, dst_end = place(rng, cases, 0, 0)
    cuts, files = [0], []
    for s, (_, _, ln) in zip(starts, cases):
        if s != cuts[-1]:
            cuts.append(s)  # the gap before it: a file nobody lists
        files.append(len(cuts) - 1)
        cuts.append(s + ln)
    assert starts[0] == 0 and cuts[-1] == src_end
    src = rng.integers(0, 256, size=src_end, dtype=np.uint8).tobytes()
    lens = [c[2] for c in cases]
    return GatherCase(src, np.array(cuts, dtype=np.uint64), files, starts, lens, dsts, dst_end + 19,
                      [(c[0], c[1]) for c in cases])


def host_table(part, seed=13):
    """gather_host_kernel: all 256 pairs x HOST_SHORT, and the long lengths spread over the pairs: pair
    (k, dp) gets HOST_BIG[(k + dp) % 4] for dp < 4 and HOST_MID[(k + dp) % 5] otherwise, so every pair has
    a length of 4095 or more and every length meets all 16 shifts k.  part 0 / 1: the pairs with even /
    odd dp (the whole table is above the size one test may move).  The source keeps 32 bytes before its
    first file and after its last."""
    rng = np.random.default_rng(seed + part)
    cases = []
    for k in range(16):
        for dp in range(part, 16, 2):
            cases += [(k, dp, ln) for ln in HOST_SHORT]
            cases.append((k, dp, HOST_BIG[(k + dp) % 4] if dp < 4 else HOST_MID[(k + dp) % 5]))
    rng.shuffle(cases)
    cases = [tuple(int(x) for x in c) for c in cases]
    starts, dsts, src_end, dst_end = place(rng, cases, 32, 0)
    # (the first file may start past 32: a case of its own has the exact margins)
    src = rng.integers(0, 256, size=src_end + 32, dtype=np.uint8).tobytes()
    return GatherCase(src, None, None, starts, [c[2] for c in cases], dsts, dst_end + 19,
                      [(c[0], c[1]) for c in cases])


def gather_table_coverage(cases, branch_of_block, want_paths):
    """Asserts over one or more GatherCase that every ((s - d) & 15, d & 15) pair occurs and every shift
    meets the paths `want_paths(k)`; branch_of_block(s, length, d) yields the paths of a file's blocks.
    Returns the pairs, the (shift, length) and the (destination phase, length) combinations seen."""
    pairs, by_k, by_dp, paths = set(), set(), set(), {}
    for c in cases:
        for s, ln, d, tag in zip(c.starts, c.lens, c.dsts, c.tags):
            k, dp = (s - d) & 15, d & 15
            assert (k, dp) == tag
            pairs.add((k, dp))
            by_k.add((k, ln))
            by_dp.add((dp, ln))
            paths.setdefault(k, set()).update(branch_of_block(s, ln, d))
    assert len(pairs) == 256, "pairs missing: %d of 256" % len(pairs)
    for k in range(16):
        assert not want_paths(k) - paths[k], "shift %d lacks %s" % (k, want_paths(k) - paths[k])
    return pairs, by_k, by_dp


def shifted_blocks(s, ln, d):
    return {shifted_branch_of(s, ln, d, b) for b in range(blocks_of(d, ln))}


def host_blocks(s, ln, d):
    out = set()
    for p in range((ln + GATHER_PIECE - 1) // GATHER_PIECE):
        d0 = d + p * GATHER_PIECE
        for b in range(blocks_of(d0, min(ln - p * GATHER_PIECE, GATHER_PIECE))):
            out.add(host_branch_of(s, ln, d, p, b))
    return out


def gather_kernel_coverage(case):
    pairs, by_k, by_dp = gather_table_coverage([case], shifted_blocks, lambda k: {"shift_q%d" % (k >> 2), "ragged"})
    for x in range(16):
        assert not [ln for ln in GATHER_LENS if (x, ln) not in by_k], "gather table: shift %d lacks a length" % x
        assert not [ln for ln in GATHER_LENS if (x, ln) not in by_dp], "gather table: phase %d lacks a length" % x


def host_gather_coverage(cases):
    def want(k):
        sh = "aligned" if k == 0 else "q%dr%d" % (k >> 2, k & 3)
        return {HostBranch("full", sh, nx) for nx in ("shfl", "readlane", "ex")} | {HostBranch("ragged", sh, "shfl")}

    pairs, by_k, by_dp = gather_table_coverage(cases, host_blocks, want)
    long_of = {}
    for c in cases:
        for s, ln, d in zip(c.starts, c.lens, c.dsts):
            if ln >= 4095:
                long_of.setdefault(((s - d) & 15, d & 15), []).append(ln)
    assert len(long_of) == 256, "host table: pairs without a length of 4095 or more"
    for k in range(16):
        assert not [ln for ln in HOST_LENS if (k, ln) not in by_k], "host table: shift %d lacks a length" % k
    for dp in range(16):
        assert not [ln for ln in HOST_SHORT if (dp, ln) not in by_dp], "host table: phase %d lacks a length" % dp
