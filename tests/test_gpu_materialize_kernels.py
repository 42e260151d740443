"""mat_locate_kernel and mat_write_kernel (trivy_amd/csrc/materialize.hip) through tsg_debug_materialize, field
for field against the plain model of tests/findings_model.py (the reference's findLocation on the censored
content).  Every case of tests/findings_cases.py runs as seventeen files of one call -- the arena's first
file, the start phases 1..15, the arena's last file ending in mid-block before a tail of '\\n' -- between
neighbours full of '\\n', with the materializer's guard bytes on: every FindingOut and LineOut field, the text,
pref, the totals and the bytes past them are compared, and a difference names the case, the file's phase,
the location and the field."""
import numpy as np
import pytest

from tests import findings_cases as fc
from tests import findings_model as fm
from trivy_amd import _lib

pytestmark = pytest.mark.gpu


def _got(r) -> fm.Call:
    return fm.Call(np.frombuffer(r["findings"], dtype=fm.FINDING), np.array(r["pref"], dtype=np.uint64),
                   np.frombuffer(r["lines"], dtype=fm.LINE), r["text"], r["n_lines"], r["n_text"])


def _run_case(case, order=None):
    ar = fc.arena_of(case.content)
    F, M, S = fc.records_of(case, ar, order)
    want = fc.expected_of(case, len(F))
    got = _got(_lib.materialize(ar.arena, ar.offsets, F, M, S, guard=True))

    def describe(m):
        i = int(M["fidx"][m])
        start = int(ar.offsets[int(F["file"][i])])
        return "case %s, file at arena offset %d (phase %d%s), location %d [%d, %d) anchor %d" % (
            case.name, start, start % 16, ", the last file" if int(F["file"][i]) == ar.file_ids[-1] else "",
            m - int(F["m0"][i]), int(M["s"][m]), int(M["e"][m]), int(M["a_wlo"][m]))

    d = fm.diff(got, want, describe)
    assert d is None, d


PARTS = dict(backward=3, forward=2, counting=2, spans=1, cuts=1, empty=1)  # (a table's cases dealt out over its parts)


@pytest.mark.parametrize("table,part", [(t, p) for t in ["backward", "forward", "counting", "spans", "cuts", "empty"]
                                        for p in range(PARTS[t])])
def test_case_table(table, part):
    """backward: the last three visible '\\n' before s over the 1-KiB windows walked downwards; forward: the first
    two at or after s; counting: the raw '\\n' between the anchor and s in 4-KiB steps; spans: the per-block censor
    masks; cuts: the 100-B line cut and the start-30 / end+20 match cut; empty: s == e."""
    cases = fc.TABLES[table]()
    fc.coverage(table, cases)  # (the asserts tests/test_findings_model.py runs without a GPU)
    for case in cases[part::PARTS[table]]:
        _run_case(case)


def test_layout_file_order_and_empty_files():
    """MatFile.file descending and shuffled (m0 / s0 stay the running sums), an empty file with an empty location
    between files with findings, several locations per file."""
    case = next(c for c in fc.span_cases() if c.name == "span_nl_around_code")
    ar = fc.arena_of(case.content)
    _run_case(case, ar.file_ids[::-1])
    _run_case(case, [int(i) for i in np.random.default_rng(4).permutation(ar.file_ids)])
    # three files: findings, an empty file, findings; then the same with the empty file holding a location
    a, b = fc.cut_cases()[0], fc.backward_cases()[5]
    contents = [a.content, b"", b.content]
    offsets = np.cumsum([0, 7] + [x for c in contents for x in (len(c), 5)]).astype(np.uint64)
    arena = b"\n" * 7 + b"".join(c + b"\n" * 5 for c in contents) + b"\n" * 64
    for ids, locs in (([1, 5], [a.locs, b.locs]), ([5, 3, 1], [b.locs, [(7, 0, 0)], a.locs])):
        cs = [arena[int(offsets[i]):int(offsets[i + 1])] for i in ids]
        F, M, S = fm.records(ids, cs, locs)
        want = fm.call_model([fm.file_model(c, l) for c, l in zip(cs, locs)])
        d = fm.diff(_got(_lib.materialize(arena, offsets, F, M, S)), want)
        assert d is None, d
        assert want.n_lines >= 6 and int(F["m0"][-1]) > 0 and int(F["s0"][-1]) > 0


def test_more_locations_than_waves():
    """65,536 + 77 locations (the grid's 16,384 workgroups x 4 waves hold 65,536) over one small file: the
    grid-stride loop, pref over many records.  The locations repeat a few distinct ones, so the model runs once
    per distinct location."""
    case = next(c for c in fc.span_cases() if c.name == "span_merged_middle")
    distinct = case.locs + [(9, 5, 5), (9, 210, 210)]
    n = 65536 + 77
    pick = np.random.default_rng(6).integers(0, len(distinct), size=n)
    locs = [distinct[int(i)] for i in pick]
    arena = b"\n" * 21 + case.content + b"\n" * 64
    offsets = [0, 21, 21 + len(case.content)]
    spans = fm.merged_spans(case.content, [(s, e) for _, s, e in case.locs])
    F, M, S = fm.records([1], [case.content], [locs], [case.anchors], [spans])
    want = fm.call_model([fm.file_model(case.content, locs, spans)])
    d = fm.diff(_got(_lib.materialize(arena, offsets, F, M, S)), want)
    assert d is None, d
    assert want.n_lines > 3 * n


def test_caps_and_totals():
    """-3 when a cap is below its total; the totals come back in any case."""
    case = fc.cut_cases()[0]
    ar = fc.arena_of(case.content)
    F, M, S = fc.records_of(case, ar)
    want = fc.expected_of(case, 17)
    for kw in (dict(lines_cap=want.n_lines - 1), dict(text_cap=want.n_text - 1)):
        with pytest.raises(_lib.HookStatus) as ei:
            _lib.materialize(ar.arena, ar.offsets, F, M, S, **kw)
        assert ei.value.rc == -3 and (ei.value.n_lines, ei.value.n_text) == (want.n_lines, want.n_text)
    r = _lib.materialize(ar.arena, ar.offsets, F, M, S, lines_cap=want.n_lines, text_cap=want.n_text, guard=False)
    assert fm.diff(_got(r), want) is None


def test_kernel_self_check_fires():
    """The kernel's own consistency check (the error word): a location on line 1 whose a_nl is one too large
    makes the line count 2 while the search finds one '\\n' before s; Run reports it (-5)."""
    content = b"first line\nk = " + fc.SECRET + b" \nthird\n"
    s = content.index(fc.SECRET)
    F, M, S = fm.records([1], [content], [[(1, s, s + len(fc.SECRET))]], [(12,)])
    assert M["a_wlo"][0] == 12 and M["a_nl"][0] == 1
    arena = b"\n" * 9 + content + b"\n" * 64
    offsets = [0, 9, 9 + len(content)]
    assert _got(_lib.materialize(arena, offsets, F, M, S)).findings["start_line"][0] == 2
    M["a_nl"][0] = 2
    with pytest.raises(_lib.HookStatus, match="line search and line count disagree") as ei:
        _lib.materialize(arena, offsets, F, M, S)
    assert ei.value.rc == -5
