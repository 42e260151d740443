"""The findings kernels' CPU model (tests/findings_model.py) against the oracle's scan, the coverage of the GPU
tests' case tables (tests/findings_cases.py), and tsg_debug_materialize's refusals, which precede every HIP call."""
import numpy as np
import pytest

from oracle import secret_scanner as osc
from oracle.gosort import sort_slice
from tests import findings_cases as fc
from tests import findings_model as fm
from tests.test_gpu_findings import _edge_files
from trivy_amd import _lib


# ---- 1. the model's layout gives the oracle's findings -------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_model_layout_vs_oracle_scan(seed, monkeypatch):
    """For the edge files of tests/test_gpu_findings.py: the locations the oracle's scan hands to toFinding, laid
    out by the model as the kernels lay them out (spans, shared cause text, file-relative offsets), give back the
    scan's own findings."""
    o = osc.new_scanner(None)
    rule_index = {id(r): i for i, r in enumerate(o.rules)}
    seen = []
    real = osc.to_finding

    def recording(rule, loc, content):
        seen.append((rule_index[id(rule)], loc[0], loc[1]))
        return real(rule, loc, content)

    monkeypatch.setattr(osc, "to_finding", recording)
    n = lines = 0
    for path, content in _edge_files(seed):
        del seen[:]
        want = o.scan(path, content)
        if not seen:
            assert not want["Findings"]
            continue
        fo = fm.file_model(content, list(seen))
        got = fm.findings_of(o.rules, fo)

        def less(x, y):  # scanner.go:452-457
            if x["RuleID"] != y["RuleID"]:
                return osc._b(x["RuleID"]) < osc._b(y["RuleID"])
            return osc._b(x["Match"]) < osc._b(y["Match"])

        sort_slice(got, less)
        assert got == want["Findings"], path
        assert len(fo.text) <= sum(fm.text_bound(s, e) for _, s, e in seen), path
        n += len(got)
        lines += len(fo.lines)
    assert n > 80 and lines > 2 * n


def test_spans_and_anchor_helpers_hand_written():
    c = b"ab\ncd\n\nefgh\nij"
    assert fm.merged_spans(c, [(8, 11), (1, 4), (3, 7), (5, 5), (11, 13)]) == [(1, 7, 0), (8, 13, 3),
                                                                              (fm.SENTINEL, fm.SENTINEL, 4)]
    assert fm.merged_spans(c, [(4, 4)]) == [(fm.SENTINEL, fm.SENTINEL, 0)]
    assert fm.censor(c, fm.merged_spans(c, [(1, 4)])) == b"a***d\n\nefgh\nij"
    assert fm.choose_anchor(c, 8, [0, 3, 7, 9]) == (7, 3)
    assert fm.choose_anchor(c, 2, [3, 7]) == (0, 0)
    # one finding written out by hand: the cause line shares the match text, the others follow it
    fo = fm.file_model(c, [(5, 8, 10)])
    assert fo.text == b"e**h" + b"cd" + b"" + b"ij"
    assert fo.findings.tolist() == [(5, 4, 4, 0, 4, 0, 4)]
    assert fo.lines.tolist() == [(2, 4, 2, 0, 0, 0), (3, 6, 0, 0, 0, 0), (4, 0, 4, 1, 1, 1), (5, 6, 2, 0, 0, 0)]
    call = fm.call_model([fo, fo])
    assert call.pref.tolist() == [0, 8 << 32 | 4, 16 << 32 | 8] and call.text == fo.text * 2
    assert fm.diff(call, call) is None
    other = call._replace(text=call.text[:9] + b"X" + call.text[10:])
    assert "location 1" in fm.diff(other, call) and "text byte 9" in fm.diff(other, call)
    longer = call.findings.copy()
    longer["match_len"][0] = 5
    d = fm.diff(call._replace(findings=longer, pref=call.pref + np.array([0, 1 << 32, 1 << 32], dtype=np.uint64)), call)
    assert "location 0" in d and "FindingOut.match_len got 5 want 4" in d


# ---- 2. the GPU tests' case tables reach what they are for -----------------------------------
@pytest.mark.parametrize("table", sorted(fc.TABLES))
def test_case_table_coverage(table):
    cases = fc.TABLES[table]()
    assert len({c.name for c in cases}) == len(cases)
    fc.coverage(table, cases)
    fc.minimum_counts(table, cases)
    for c in cases:  # the records the hook will take: every location inside its file, anchors at or below s
        F, M, S = fc.records_of(c, fc.arena_of(c.content))
        assert len(F) == 17 and (M["a_wlo"] <= M["s"]).all() and (M["e"] <= len(c.content)).all()


def test_coverage_asserts_notice_a_gap():
    back = [c for c in fc.backward_cases() if c.tags.get("back", (0, 0, 0))[2] != 1025]
    with pytest.raises(AssertionError):
        fc.coverage("backward", back)
    with pytest.raises(AssertionError):
        fc.coverage("forward", [c for c in fc.forward_cases() if c.tags.get("fwd_edge") != "fwd_empty_line_below"])
    with pytest.raises(AssertionError):
        fc.coverage("counting", [c for c in fc.counting_cases() if c.tags["count"] != (4112, "sparse", 37)])


# ---- 3. the hook refuses before it touches HIP ------------------------------------------------
def _call(content=b"ab\ncd\nefgh\nij\n", F=None, M=None, S=None, offsets=None):
    F0, M0, S0 = fm.records([1], [content], [[(1, 6, 9), (2, 11, 13)]])
    pick = lambda x, d: d if x is None else x
    arena = b"\n\n" + content + b"\n" * 64
    return _lib.materialize(arena, pick(offsets, [0, 2, 2 + len(content)]), pick(F, F0), pick(M, M0), pick(S, S0))


def _edited(arr, i, **kw):
    a = arr.copy()
    for k, v in kw.items():
        a[k][i] = v
    return a


def test_materialize_hook_refusals():
    F, M, S = fm.records([1], [b"ab\ncd\nefgh\nij\n"], [[(1, 6, 9), (2, 11, 13)]])
    assert S.tolist() == [(6, 9, 0), (11, 13, 0), (fm.SENTINEL, fm.SENTINEL, 0)]
    two = np.concatenate([F, F])
    two["m0"][1], two["s0"][1] = 2, 3
    cases = [
        (dict(M=_edited(M, 1, e=15)), "location 1: outside its file"),
        (dict(M=_edited(M, 0, s=-1, a_wlo=-1)), "location 0: outside its file|negative anchor"),
        (dict(M=_edited(M, 0, e=5)), "location 0: e < s"),
        (dict(M=_edited(M, 0, a_wlo=7)), "location 0: a_wlo > s"),
        (dict(M=_edited(M, 1, s=10)), "location 1: no span covers it"),
        (dict(S=S[[1, 0, 2]]), "span 1 is unsorted"),
        (dict(S=_edited(S, 0, e=11)), "span 1 is unsorted, touches"),
        (dict(S=_edited(S, 0, e=12)), "span 1 is unsorted, touches or overlaps"),
        (dict(S=_edited(S, 1, e=15)), "span 1 is empty or outside its file"),
        (dict(S=_edited(S, 2, e=14, s=13)), "lack the sentinel"),
        (dict(S=S[:2], F=_edited(F, 0, ns=2)), "lack the sentinel"),
        (dict(M=_edited(M, 1, fidx=1)), "location 1: fidx contradicts"),
        (dict(F=_edited(F, 0, m0=1)), "file record 0: m0 contradicts"),
        (dict(F=_edited(F, 0, s0=1)), "file record 0: s0 contradicts"),
        (dict(F=_edited(F, 0, nm=1)), "no file record holds"),
        (dict(F=_edited(F, 0, nm=3)), "leave the arrays"),
        (dict(F=two), "file record 1: its locations or spans leave the arrays"),
        (dict(F=_edited(F, 0, file=2)), "no such file"),
        (dict(offsets=[0, 2, 15]), "end at n_bytes"),
        (dict(offsets=[1, 2, 16]), "start at 0"),
        (dict(offsets=[0, 17, 16]), "ascend"),
    ]
    for kw, why in cases:
        with pytest.raises(_lib.HookRefused, match=why):
            _call(**kw)
