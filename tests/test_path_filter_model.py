"""The path filter's table builders (BuildPathTable / BuildSureTable through tsg_debug_path_tables) and the host
model of the exact shift-and (tsg_debug_sure_allow) against the substring semantics of tests/path_filter_model.py,
without a GPU: the raw tables, run through the shift-and classes of tests/tar_required_model.py, must give the
rules and the decisions the semantics give on every case path."""
import numpy as np
import pytest

from tests import path_filter_model as pm
from tests import tar_required_model as trm
from tests.test_sure_allow import _sure
from trivy_amd import _lib


def _raw(t):
    pt, st = _lib.path_tables(t.lits, t.sure)
    assert pt is not None and (st is not None) == bool(t.sure)
    return pt, st


@pytest.mark.parametrize("make", [pm.four_word_tables, pm.small_tables, pm.no_sure_tables])
def test_built_tables_vs_semantics(make):
    """Pins BuildPathTable's rule_of and word packing and BuildSureTable's S0 / EZ."""
    t = make()
    pt, st = _raw(t)
    P, S = trm.PathTable(pt), (trm.SureTable(st) if st else None)
    paths = pm.case_paths(t)
    n_rules = n_sure = 0
    for p in paths:
        want = pm.rules(t, p)
        assert P.rules(p) == want, (p, hex(want))
        n_rules += want != 0
        if S is not None:
            want = pm.sure(t, p)
            got = bool(p) and len(p) <= pm.SURE_MAX_PATH and max(p) < 0x80 and S.completes(p)
            assert got == want, p
            n_sure += want
    assert n_rules > 50 and (S is None or n_sure > 20)
    hits, high, sure, flagged_not_sure = pm.counts(t, paths)
    assert hits > 50 and high > 10 and flagged_not_sure > 10 and (sure > 20 or S is None)


def test_four_word_tables_fill_four_words():
    t = pm.four_word_tables()
    pt, st = _raw(t)
    P, S = trm.PathTable(pt), trm.SureTable(st)
    assert all(P.S) and all(P.E) and P.S[0] == 1 and P.E[0] == 1 << 63 and P.S[1] & 1  # bit 63, then bit 0
    assert P.rule_of[63] == 63 and P.rule_of[64 + 1] == 0
    assert np.frombuffer(pt[8512:8516], dtype=np.uint32)[0] == 4
    assert all(a | b for a, b in zip(S.S, S.S0)) and all(a | b for a, b in zip(S.E, S.EZ))
    assert S.S0[0] == 1 and S.E[0] == 1 << 63
    assert {r for _, r in t.lits} >= {0, 63} and any(len(l) == 2 for l, _ in t.lits)
    kinds = {(b, e) for _, b, e in t.sure}
    assert kinds == {(False, False), (True, False), (False, True), (True, True)}
    assert any(a != b for pos, _, _ in t.sure for a, b in pos)


def test_case_paths_hold_the_listed_edges():
    t = pm.four_word_tables()
    paths = set(pm.case_paths(t))
    assert {b"", b"a", b"@", b"A", b"Z", b"[", b"\x80"} <= paths
    assert {len(p) for p in paths} >= {0, 1, 4095, 4096, 4097}
    assert any(p[0] >= 0x80 and max(p[1:]) < 0x80 for p in paths if len(p) > 1)
    assert any(p[-1] >= 0x80 and max(p[:-1]) < 0x80 for p in paths if len(p) > 1)
    assert b"xbuild/" in paths and not pm.sure(t, b"xbuild/x")             # a begin literal at offset 1
    assert b"x.locky" in paths and not pm.sure(t, b"q.locky") and pm.sure(t, b"q.LoCk")  # an end literal + 1 byte
    assert pm.sure(t, b"p" * 4091 + b".lock") and not pm.sure(t, b"p" * 4092 + b".lock")
    assert pm.rules(t, b"/testst/") == 1 << 2 and pm.rules(t, b"abzz") == 3


def test_sure_allow_host_model_on_real_patterns():
    """tsg_debug_sure_allow (SureTableOf + SureAllowHost) on patterns whose exact literals are written out here by
    hand agrees with the semantics on every case path."""
    patterns = [r"(?i)\.lock$", r"^build/", r"/Vendor/", r"/locales?/", r"^exact-name$"]
    t = pm.Tables("real", [], [pm.exact(b".lock", end=True, fold=True), pm.exact(b"build/", begin=True),
                               pm.exact(b"/Vendor/"), pm.exact(b"/locale/"), pm.exact(b"/locales/"),
                               pm.exact(b"exact-name", begin=True, end=True)])
    paths = pm.case_paths(pm.four_word_tables()) + pm.case_paths(t)
    assert b".lockbuild/" in paths and not pm.sure(t, b".lockbuild/")  # (no start after an end literal's last position)
    sure, form = _sure(patterns, paths)
    assert form.all()
    want = [pm.sure(t, p) for p in paths]
    for p, got, w in zip(paths, sure, want):
        assert bool(got) == w, "path %r: sure got %s want %s" % (p[:80], bool(got), w)
    assert sum(want) > 30


def test_builders_refuse():
    ok = [(b"ab", 0)]
    assert _lib.path_tables(ok, [])[0] is not None
    for lits in ([(b"ab", 64)], [(b"a", 0)], [(b"x" * 65, 0)], [(b"aB", 0)], [(b"x" * 64, i) for i in range(5)], []):
        assert _lib.path_tables(lits, [])[0] is None, lits
    assert _lib.path_tables([(b"x" * 64, i) for i in range(4)], [])[0] is not None
    # the exact builder: a fifth word is refused; an empty list builds nothing
    assert _lib.path_tables(ok, [pm.exact(b"y" * 64)] * 4)[1] is not None
    assert _lib.path_tables(ok, [pm.exact(b"y" * 64)] * 4 + [pm.exact(b"z")])[1] is None
    assert _lib.path_tables(ok, [])[1] is None
