"""What path_filter_kernel (trivy_amd/csrc/pathfilter.hip) reports, stated without tables, and the tables, paths
and batches of tests/test_gpu_path_filter_kernel.py.

  rules(p)  the OR of the rule bits of the prefilter literals contained in the ASCII-lowered path
  sure(p)   p is ASCII, 1 <= len(p) <= 4096, and some exact literal matches position by position at some i,
            with i == 0 for a `begin` literal and i + k == len(p) for an `end` one
  record    (i | kPathNonAscii, rules 0) for a path holding a byte >= 0x80, else (i, rules) iff rules != 0
  skip      one byte per path: 1 iff sure(p)
The shift-and classes of tests/tar_required_model.py read the raw tables as a second opinion.
"""
from collections import namedtuple

NON_ASCII = 0x80000000
SURE_MAX_PATH = 4096

Tables = namedtuple("Tables", "name lits sure")  # lits: [(lowercased bytes, rule)]; sure: [(positions, begin, end)]


def lower(p: bytes) -> bytes:
    return bytes(b + 32 if 0x41 <= b <= 0x5A else b for b in p)


def exact(lit: bytes, begin=False, end=False, fold=False):
    """An exact literal: per position the two bytes it accepts (both cases of a letter with fold)."""
    pos = []
    for b in lit:
        other = b ^ 0x20 if fold and (0x41 <= b <= 0x5A or 0x61 <= b <= 0x7A) else b
        pos.append((b, other))
    return (pos, begin, end)


def rules(t: Tables, p: bytes) -> int:
    lp, out = lower(p), 0
    for lit, r in t.lits:
        if lit in lp:
            out |= 1 << r
    return out


def sure(t: Tables, p: bytes) -> bool:
    if not t.sure or not 1 <= len(p) <= SURE_MAX_PATH or any(b >= 0x80 for b in p):
        return False
    for pos, begin, end in t.sure:
        k = len(pos)
        starts = [0] if begin else ([len(p) - k] if end else range(len(p) - k + 1))
        for i in starts:
            if 0 <= i <= len(p) - k and (not end or i + k == len(p)) and all(p[i + j] in pos[j] for j in range(k)):
                return True
    return False


def batch_model(t: Tables, paths, memo=None):
    """(records, skip): the set of (file, pad, rules) records of a batch and its skip bytes."""
    memo = {} if memo is None else memo
    recs, skip = set(), bytearray()
    for i, p in enumerate(paths):
        if p not in memo:
            high = any(b >= 0x80 for b in p)
            memo[p] = (high, 0 if high else rules(t, p), sure(t, p))
        high, r, s = memo[p]
        skip.append(1 if s else 0)
        if high:
            recs.add((i | NON_ASCII, 0, 0))
        elif r:
            recs.add((i, 0, r))
    return recs, bytes(skip)


def counts(t: Tables, paths, memo=None):
    """(hits, non-ASCII paths, sure paths, paths with rules != 0 that are not sure)."""
    recs, skip = batch_model(t, paths, memo)
    flagged = {f for f, _, r in recs if r}
    return (len(recs), sum(1 for f, _, _ in recs if f & NON_ASCII), sum(skip),
            sum(1 for f in flagged if not skip[f]))


# ---- tables -------------------------------------------------------------------------------
def four_word_tables():
    """Both tables fill all four words.  Prefilter: word 0 is one 64-byte literal (its last position is bit 63),
    so the next literal starts at bit 0 of word 1; 2-byte literals; rule ids 0 and 63; a literal that does not
    fit the rest of a word and moves to the next.  Exact: begin-only, end-only, both, neither, case-folded
    positions, a 64-position literal; an end literal packed right before a begin literal."""
    long64 = b"/" + b"abcdefghijklmnopqrstuvwxyz0123456789_-." * 2
    long64 = long64[:63] + b"/"
    assert len(long64) == 64
    lits = [(long64, 63), (b"ab", 0), (b"zz", 1), (b"/test", 2), (b"vendor/", 3), (b".md", 4), (b"node_modules", 5),
            (b"q" * 30, 6),                                   # word 1: 2 + 2 + 5 + 7 + 3 + 12 + 30 = 61 positions
            (b"r1r2r3r4r5r6r7r8r9r0r1r2r3r4r5", 7),           # 30 more do not fit: word 2
            (b"/locale/", 8), (b"0123456789" * 6, 9),         # 30 + 8, then 60 do not fit: word 3
            (b"t.", 62)]
    sure = [exact(long64, begin=True), exact(b".lock", end=True, fold=True), exact(b"build/", begin=True),
            exact(b"/Vendor/"), exact(b"exact-name", begin=True, end=True), exact(b"/locale/"), exact(b"/locales/"),
            exact(b"a"), exact(b"Q" * 40, fold=True), exact(b"y" * 20 + b"/", begin=True),
            exact(b"w" * 50, end=True), exact(b"md", end=True)]
    return Tables("four_words", lits, sure)


def small_tables():
    return Tables("small", [(b"test", 0), (b"st/", 63), (b"ab", 5), (b"ba", 6)],
                  [exact(b".md", end=True, fold=True), exact(b"test/", begin=True), exact(b"/t")])


def no_sure_tables():
    return Tables("no_sure", small_tables().lits, [])


# ---- paths --------------------------------------------------------------------------------
def case_paths(t: Tables):
    """The edge paths of the issue for the given tables, every prefilter and exact literal at offset 0, in
    the middle and at the end, in both cases."""
    out = [b"", b"a", b"b", b"/", b"@", b"A", b"Z", b"[", b"`", b"{", b"\x80", b"\xff", b"\x80ab", b"ab\x80", b"a\xc5b",
           b"@b", b"Ab", b"aB", b"AB", b"[b", b"a[", b"`b", b"a@", b"zZ", b"Zz", b"z[", b"zZz", b"aba", b"bab", b"abab",
           b"x/none/of/them", b"t", b"t.", b"T.", b"xt.x"]
    for lit, _ in t.lits:
        for v in (lit, lit.upper(), lit[:-1], lit[1:], lit[:-1] + b"\x80"):
            out += [v, b"x" + v, v + b"y", b"dir/" + v + b"/f", v + v]
    for pos, begin, end in t.sure:
        a, b = bytes(p[0] for p in pos), bytes(p[1] for p in pos)
        mixed = bytes(p[j % 2] for j, p in enumerate(pos))
        for v in (a, b, mixed, a[:-1], a[1:], lower(a), a.upper()):
            out += [v, b"x" + v, v + b"y", b"x" + v + b"y", b"\x80" + v, v + b"\xfe"]
    # the exact literal last at lengths 4095 / 4096 / 4097; a begin literal at offset 1; an end literal + 1 byte
    for pos, begin, end in t.sure:
        a = bytes(p[0] for p in pos)
        for n in (4095, 4096, 4097):
            if len(a) < 60:
                out.append(b"p" * (n - len(a)) + a)
    # one exact literal right after the one packed before it: a carry out of a literal's last position into the
    # next one's first would start a begin literal past offset 0, or go on from an end literal's last position
    for (pa, _, _), (pb, _, _) in zip(t.sure, t.sure[1:]):
        a, b = bytes(p[0] for p in pa), bytes(p[0] for p in pb)
        if len(a) + len(b) < 80:
            out += [a + b, b"x" + a + b]
    # two literals overlapping in the path
    out += [b"/testst/", b"vendor/test", b"abzz", b"abb", b"/test.md", b"x/locale/locales/", b"/Vendor/locale/"]
    return out


def big_batch(t: Tables, n):
    """n paths repeating the distinct case paths shorter than 200 bytes in a fixed shuffled order."""
    import numpy as np
    pool = sorted({p for p in case_paths(t) if len(p) < 200})
    pick = np.random.default_rng(12).integers(0, len(pool), size=n)
    return [pool[int(i)] for i in pick]
