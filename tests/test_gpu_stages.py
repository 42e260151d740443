"""Every stage of the GPU candidate engine against its CPU model.

tsg_debug_engine_stages runs one synchronous scan (GpuEngine::Run) and returns what the
kernels left behind: the chunk map (K0), the per-chunk newline counts and flagged blocks
(K1), the anchor hits, keyword bits and file flags (K2, fold, kwfold), all candidates with
their line hints and gate flags (verify, full scan, finalize).  Every case asserts, after
the overflow guard, the six invariants of tests/stage_model.py check_all:

  1. chunk map and newline counts equal the model;
  2. the flagged blocks equal the model's, each recorded once.  K1 is exact: a block is
     flagged iff a bucket fires at one of its 16 window ends (the fire slots are sampled so
     that every end is seen once), over the arena zero-padded to the last 4-KiB tile;
  3. files without fold runes: required hits <= GPU hits <= allowed hits (the two differ only
     by hits whose literal ends with the arena's last byte, which K2 keeps untested);
  4. keyword bits (ASCII containment; Go ToLower containment after kwfold) and file flags;
  5. candidates of anchored rules in files without fold runes as a multiset, and nl_before,
     nl_back, nl_fwd, flags of every candidate;
  6. every true match start of every rule in every file lies in a live candidate's window.

All comparisons are exact; the cases (tests/stage_cases.py) are the smallest shapes at which
the kernels can go wrong, and each asserts non-trivial counts.
"""
import pytest

from tests import stage_cases as sc
from tests import stage_model as sm

pytestmark = pytest.mark.gpu

_PREPARED = {}


def _prepared(key, build, monkeypatch):
    """(case, model, expectation, true matches) of a case, computed once."""
    if key not in _PREPARED:
        case = build()
        model = sc.model_of(case, monkeypatch)
        b = case["batch"]
        _PREPARED[key] = (case, model, model.expect(b), model.true_matches(b))
    return _PREPARED[key]


def _run(name, prepared, monkeypatch, env=None):
    case, model, e, matches = prepared
    b = case["batch"]
    with monkeypatch.context() as m:
        for k, v in {**(case.get("env") or {}), **(env or {})}.items():
            m.setenv(k, v)
        d = sm.run_engine(model, b)
    sm.check_overflow(d)  # first: nothing below may pass on a truncated list
    n = sm.check_all(d, e, model, b, matches)
    sc.check_case(case, d, e, model)
    lo = case["min"]
    print("stage-case %s %s: files %d bytes %d blocks %d hits %d candidates %d matches %d"
          % (name, env or {}, b.n_files, b.n_bytes, len(d.recs), len(d.hits), len(d.cands), n))
    assert len(d.hits) >= lo[0] and len(d.cands) >= lo[1] and n >= lo[2], (len(d.hits), len(d.cands), n, lo)
    return d


VARIANTS = {
    "default": {},
    "k1-grid-1": {"TSG_DIAG_K1_GRID": "1"},
    "global-tables": {"TSG_LDS_TABS_MAX": "0"},
    "global-tables-unstaged-classes": {"TSG_LDS_TABS_MAX": "0", "TSG_CONFIRM_STAGE_CLASSES": "0"},
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_boundaries(monkeypatch, variant):
    """Match starts and literal ends at every offset around 16-B block, 64-B lane chunk, 1-KiB chunk,
    4-KiB tile and workgroup boundaries, under the engine's table variants."""
    _run("boundaries", _prepared("boundaries", sc.case_boundaries, monkeypatch), monkeypatch, VARIANTS[variant])


def test_boundaries_calibrated(monkeypatch):
    """The same batch with tables from a calibrated compile (anchors moved to class runs)."""
    from tests.test_filter_model import _calibration_sample
    sample = _calibration_sample(0)
    p = _prepared("boundaries-calibrated", lambda: sc.case_boundaries(sample), monkeypatch)
    assert p[1].fm.n_calibrated >= 1
    _run("boundaries-calibrated", p, monkeypatch)


@pytest.mark.parametrize("variant", ["default", "global-tables"])
def test_boundaries_class_run_rules(monkeypatch, variant):
    _run("class-runs", _prepared("class-runs", sc.case_class_runs, monkeypatch), monkeypatch, VARIANTS[variant])


@pytest.mark.parametrize("grid", ["uncapped", "1"])
def test_arena_edges(monkeypatch, grid):
    """Tokens at arena offsets 0..7 (K1 sees zero bytes before the arena) and 0..7 bytes before its end."""
    for k in range(8):
        p = _prepared("arena-edges-%d" % k, lambda: sc.case_arena_edges(k), monkeypatch)
        _run("arena-edges-%d" % k, p, monkeypatch, {} if grid == "uncapped" else {"TSG_DIAG_K1_GRID": "1"})


def test_files(monkeypatch):
    """File lengths 0..1025, empty files at a chunk start, tokens and keywords cut between files,
    a token and keywords completed only by the 64 bytes behind the arena."""
    _run("files", _prepared("files", sc.case_files, monkeypatch), monkeypatch)


@pytest.mark.parametrize("fill", ["newlines", "rune"])
def test_tail_bytes_reach_no_stage(monkeypatch, fill):
    """The bytes behind the arena full of '\\n' / U+0130: no count, hint or flag comes from them."""
    byts = b"\n" if fill == "newlines" else sm.RUNE_I
    d = _run("tail-" + fill, _prepared("tail-" + fill, lambda: sc.case_tail(byts), monkeypatch), monkeypatch)
    assert not d.flags.any()


def test_dense_blocks(monkeypatch):
    p = _prepared("dense", sc.case_dense, monkeypatch)
    sc.check_case_shape("dense", p[0], p[2], p[1])  # blocks with >= 5 firing window ends
    _run("dense", p, monkeypatch)
    _run("dense", p, monkeypatch, VARIANTS["global-tables"])


def test_follow_requirements(monkeypatch):
    p = _prepared("follow", sc.case_follow, monkeypatch)
    sc.check_case_shape("follow", p[0], p[2], p[1])
    _run("follow", p, monkeypatch)


@pytest.mark.parametrize("variant", ["default", "global-tables"])
def test_fold_files(monkeypatch, variant):
    """Fold runes: exact flags, keyword bits by Go's ToLower (kwfold on), coverage in every file."""
    p = _prepared("fold", sc.case_fold, monkeypatch)
    assert p[1].kw_fold
    d = _run("fold", p, monkeypatch, VARIANTS[variant])
    assert d.counters[sm.CT_FOLDS] > 30 and d.counters[sm.CT_SPECIAL] > 20  # fold sites, special files


def test_fold_files_without_kwfold(monkeypatch):
    """TSG_KWFOLD=0: the keyword bits of files with U+0130 / U+212A are inexact, their candidates
    carry kCandFoldFile and none is dropped or skipped on a closed gate."""
    case, model, _, matches = _prepared("fold", sc.case_fold, monkeypatch)
    if "fold-inexact" not in _PREPARED:
        _PREPARED["fold-inexact"] = (case, model, model.expect(case["batch"], kw_fold=False), matches)
    d = _run("fold", _PREPARED["fold-inexact"], monkeypatch, {"TSG_KWFOLD": "0"})
    marked = [x for x in d.cands if int(x["flags"]) & sm.FOLD_FILE]
    assert len(marked) >= 5 and all(int(d.flags[int(x["file"])]) & 4 and not int(x["flags"]) & sm.DROP for x in marked)


def test_fullscan_rules(monkeypatch):
    p = _prepared("fullscan", sc.case_fullscan, monkeypatch)
    sc.check_case_shape("fullscan", p[0], p[2], p[1])
    d = _run("fullscan", p, monkeypatch)
    assert d.counters[sm.CT_OPEN_PAIRS] >= 8  # open (file, rule) pairs


def test_gates(monkeypatch):
    p = _prepared("gates", sc.case_gates, monkeypatch)
    sc.check_case_shape("gates", p[0], p[2], p[1])
    d = _run("gates", p, monkeypatch)
    aws = [r.ID for r in p[1].rules].index("aws-access-key-id")
    live = {int(x["file"]) for x in d.cands if int(x["rule"]) == aws and not int(x["flags"]) & sm.DROP}
    assert live == {1, 2, 3, 6}, live  # closed without the keyword (0) and with the runes alone (4)


def test_finalize_edges(monkeypatch):
    """Line hints over a 2.3-MiB single line: distances up to and past the 1-MiB reach, the
    file's edges, newline-only neighbours.

    Found by this test at its introduction: nl_fwd of a newline exactly kNlReach bytes after a
    16-B aligned window start came back kNlUnknown (the forward walk stopped at `lo - wabs <
    kNlReach` with the newline in the next, unread block); finalize_kernel now walks while
    `lo - wabs <= kNlReach`."""
    p = _prepared("finalize", sc.case_finalize, monkeypatch)
    sc.check_case_shape("finalize", p[0], p[2], p[1])
    _run("finalize", p, monkeypatch)
