"""path_filter_kernel (trivy_amd/csrc/pathfilter.hip, both instantiations) and the host code around it through
tsg_debug_path_filter, against the substring semantics of tests/path_filter_model.py: the PathHit records as a
set with each path at most once and pad == 0, the skip bytes exactly.  All batches of a call run one after
another on one PathFilter, so the slot's two counters used in turn, the guessed read-back with its second copy
and the count carried from call to call are part of what is compared."""
import pytest

from tests import path_filter_model as pm
from trivy_amd import _lib

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257]


@pytest.fixture(scope="module")
def raw():
    out = {}
    for make in (pm.four_word_tables, pm.small_tables, pm.no_sure_tables):
        t = make()
        out[t.name] = (t,) + _lib.path_tables(t.lits, t.sure)
    return out


def _check(t, pt, st, batches, host_packed, want_skip=True, memo=None):
    """Runs the batches, compares each with the model; -> the model's counts per batch."""
    memo = {} if memo is None else memo
    got = _lib.path_filter(pt, st, batches, host_packed=host_packed, want_skip=want_skip)
    out = []
    for b, (paths, (recs, skip)) in enumerate(zip(batches, got)):
        want_recs, want_skip_bytes = pm.batch_model(t, paths, memo)
        where = "batch %d of %s (%d paths, %s route)" % (b, [len(x) for x in batches], len(paths),
                                                        "host-packed" if host_packed else "device")
        files = [f & ~pm.NON_ASCII for f, _, _ in recs]
        twice = sorted({f for f in files if files.count(f) > 1}) if len(set(files)) != len(files) else []
        assert not twice, "%s: paths reported twice: %s" % (where, [(f, paths[f] if f < len(paths) else None)
                                                                  for f in twice[:4]])
        for f, pad, r in recs:
            i = f & ~pm.NON_ASCII
            assert i < len(paths), "%s: a record of path %d, which the batch does not have (stale?)" % (where, i)
            assert pad == 0, "%s: path %d %r: pad %#x" % (where, i, paths[i][:80], pad)
        extra, missing = set(recs) - want_recs, want_recs - set(recs)
        if extra or missing:
            i = min(f & ~pm.NON_ASCII for f, _, _ in (extra | missing))
            g = [x for x in recs if x[0] & ~pm.NON_ASCII == i]
            w = [x for x in want_recs if x[0] & ~pm.NON_ASCII == i]
            pytest.fail("%s: path %d %r (%d bytes): record (file, pad, rules) got %s want %s; %d extra, %d missing" % (
                where, i, paths[i][:80], len(paths[i]), [(hex(a), b_, hex(c)) for a, b_, c in g],
                [(hex(a), b_, hex(c)) for a, b_, c in w], len(extra), len(missing)))
        if want_skip and st is not None and paths:
            assert skip is not None, where + ": no skip bytes"
            if skip != want_skip_bytes:
                i = next(k for k in range(len(paths)) if skip[k] != want_skip_bytes[k])
                pytest.fail("%s: path %d %r (%d bytes): skip byte got %#x want %d" % (
                    where, i, paths[i][:80], len(paths[i]), skip[i], want_skip_bytes[i]))
        else:
            assert skip is None, where + ": skip bytes without want_skip and a sure table"
        out.append(pm.counts(t, paths, memo))
    return out


def _nontrivial(counts, sure=True):
    hits, high, n_sure, flagged_not_sure = (sum(c[k] for c in counts) for k in range(4))
    assert hits > 0 and high > 0 and flagged_not_sure > 0 and (n_sure > 0 or not sure), (hits, high, n_sure,
                                                                                         flagged_not_sure)


@pytest.mark.parametrize("host_packed", [False, True])
@pytest.mark.parametrize("tables", ["four_words", "small", "no_sure"])
def test_case_paths_and_batch_sizes(raw, tables, host_packed):
    """Every case path (the fold's neighbours @ A Z [, bytes >= 0x80 first, last and alone, the empty path, literals
    at offset 0 and at the end, 4095 / 4096 / 4097 bytes with the exact literal last, begin / end literals one byte
    off, overlapping literals) in one batch, then the same paths cut into batches of 1, 63, 64, 65, 255, 256 and
    257 on the same filter."""
    t, pt, st = raw[tables]
    paths = pm.case_paths(t)
    pool = paths[5:] * (sum(SIZES) // (len(paths) - 5) + 1)  # (repeated where the tables have few case paths)
    batches, at = [paths], 0
    for n in SIZES:
        batches.append(pool[at:at + n])
        at += n
    assert all(len(b) == n for b, n in zip(batches[1:], SIZES))
    counts = _check(t, pt, st, batches, host_packed)
    _nontrivial(counts[:1], sure=st is not None)
    _nontrivial(counts[1:], sure=st is not None)
    hits, high, n_sure, fns = counts[0]
    assert hits > 50 and high > 10 and fns > 10 and (n_sure > 20 or st is None)


def test_without_want_skip(raw):
    """path_filter_kernel<false> with a sure table present: no skip bytes, the same records."""
    t, pt, st = raw["four_words"]
    paths = pm.case_paths(t)
    _nontrivial(_check(t, pt, st, [paths[:300], paths[300:]], False, want_skip=False))


@pytest.mark.parametrize("host_packed", [False, True])
def test_more_paths_than_threads(raw, host_packed):
    """1,048,576 + 300 paths, more than the grid's 4096 x 256 threads: the grid-stride loop with whole waves, a
    last wave that is part empty.  The batch repeats a few hundred distinct paths."""
    t, pt, st = raw["four_words"]
    paths = pm.big_batch(t, 1048576 + 300)
    counts = _check(t, pt, st, [paths], host_packed)
    _nontrivial(counts)
    assert counts[0][0] > 100000


@pytest.mark.parametrize("host_packed", [False, True])
def test_sequences_on_one_filter(raw, host_packed):
    """The host code around the kernel: a batch with 0 hits; then one with more than 1,024 + 9/8 of the last count
    (the guessed read-back is short: the second copy); then a small one (no stale record of the batch before may
    appear, the counter this launch uses was cleared by the launch before); an odd number of launches, and the
    count is still exact."""
    t, pt, st = raw["small"]
    memo = {}
    none = [b"x%d/nothing" % i for i in range(500)]
    hot = [(b"\xc3\xa9%d" % i, b"dir%d/test/" % i, b"d%dtest" % i)[i % 3] for i in range(3000)]
    small = [b"test/a", b"plain", b"\x80", b"x/t", b"A.MD", b"xtest"]
    # thirteen launches (the empty batch launches nothing), both counters in turn; then one more
    batches = [none, hot, small, none[:70], hot[:1500], small, hot, small[:1], [], small, hot[:65], none, small, small]
    counts = _check(t, pt, st, batches, host_packed, memo=memo)
    assert counts[0][0] == 0 and counts[1][0] == 3000 > 1024 + 9 * counts[0][0] // 8
    assert counts[2][0] == 3 and counts[4][0] == 1500 > 1024 + 9 * counts[3][0] // 8
    assert counts[6][0] == 3000 > 1024 + 9 * counts[5][0] // 8 and counts[-1] == counts[2]
    assert counts[7][0] == 1 and counts[8][0] == 0 and counts[10][0] == 65
    _nontrivial(counts)


def test_builtin_rules_tables():
    """The builtin rules' own tables (the scanner's, as the resident layers' Required stage reads them)."""
    import random

    from tests import tar_required_model as trm
    from tests.test_gpu_parity import _allow_paths_batch
    from trivy_amd.analyzer import AnalyzerOptions, SecretAnalyzer
    a = SecretAnalyzer()
    a.Init(AnalyzerOptions())
    P, S = trm.tables_of(a)
    assert P is not None and S is not None
    paths = [p.encode() for p in _allow_paths_batch(random.Random(7))][:3000]
    paths += [p.upper() for p in paths[:300]] + [p + b"\xc3\xa9" for p in paths[:50]] + [b""]
    L = a._L
    import ctypes as c
    pt, st = c.create_string_buffer(trm.PATH_TABLE_BYTES), c.create_string_buffer(trm.SURE_TABLE_BYTES)
    have = c.c_uint32()
    assert L.tsg_debug_tar_required_tables(a._h, pt, len(pt), st, len(st), c.byref(have)) == 0 and have.value == 3
    (recs, skip), = _lib.path_filter(pt.raw, st.raw, [paths])
    want = set()
    for i, p in enumerate(paths):
        if any(b >= 0x80 for b in p):
            want.add((i | pm.NON_ASCII, 0, 0))
        elif P.rules(p):
            want.add((i, 0, P.rules(p)))
    assert set(recs) == want and len(recs) == len(want)
    want_skip = bytes(1 if (p and len(p) <= 4096 and max(p) < 0x80 and S.completes(p)) else 0 for p in paths)
    assert skip == want_skip
    assert len(want) > 500 and sum(want_skip) > 300 and len(want) < len(paths)
