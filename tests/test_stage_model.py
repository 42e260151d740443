"""The CPU models of the engine's stages (tests/stage_model.py) and their checkers, without a GPU.

  * The relaxed NFAs the verify kernel runs accept every true match: executed here by a
    big-int restatement of nfa_run_abs, from the match start alone and from the verify window
    of every anchor hit that covers it, for the builtin rules, the golden configs' custom
    rules and rules of every NFA width (1-4 words).
  * Every case of tests/stage_cases.py holds what it promises, and a dump made from the models
    alone passes every comparison the GPU test makes.
  * Every comparison can fail: one corruption at a time is rejected.
"""
import copy
import random
from pathlib import Path

import numpy as np
import pytest
import yaml

from tests import stage_cases as sc
from tests import stage_model as sm
from tests.test_filter_model import _planted_texts
from trivy_amd import _lib
from trivy_amd.secret import ParseConfig, builtin_rules
from trivy_amd.secret.config import Rule

ROOT = Path(__file__).resolve().parent.parent
WIDE = [Rule(ID="wide%d" % n, Category="C", Title="t", Severity="LOW", Regex="wide%d_[a-f]{%d}" % (n, n))
        for n in (70, 150, 200)]  # 2, 3 and 4 NFA words


def _rule_sets():
    out = [("builtin+wide", builtin_rules() + WIDE)]
    for f in sorted((ROOT / "tests/golden/scanner").glob("*.yaml")):
        d = yaml.safe_load(f.read_text()) or {}
        if not d.get("rules"):
            continue
        try:
            cfg = ParseConfig(str(f))
        except ValueError:
            continue
        out.append((f.name, builtin_rules() + list(cfg.CustomRules or [])))
    return out


def _soundness(model, contents, widths):
    """Every non-empty match start s: the NFA accepts with wlo = whi = s, and with the window of
    every anchor hit of the rule that covers s.  Returns (matches, windows) checked."""
    b = sm.Batch(contents)
    e = model.expect(b)
    wins = {}
    for f, end, aid in e.hits_required:
        if int(e.flags[f]) & 1:
            continue
        r, lit_len, off_lo, off_hi = model.anchors[aid]
        lit = end - lit_len
        if lit - off_lo >= 0:
            wins.setdefault((f, r), set()).add((max(0, lit - off_hi), lit - off_lo))
    n_m = n_w = 0
    for f, x in enumerate(contents):
        for r, rule in enumerate(model.rules):
            if not rule.Regex:
                continue
            nfa = model.info[r]["nfa"]
            for m in _lib.regex_find_all(rule.Regex, x, submatch=False):
                if m[1] == m[0]:
                    continue
                assert nfa.accepts(x, m[0], m[0]), (rule.ID, x[m[0]:m[1]])
                widths.add(nfa.words)
                n_m += 1
                for lo, hi in wins.get((f, r), ()):
                    if lo <= m[0] <= hi:
                        assert nfa.accepts(x, lo, hi), (rule.ID, lo, hi, x[m[0]:m[1]])
                        n_w += 1
    return n_m, n_w


def test_relaxed_nfa_accepts_every_match():
    widths = set()
    n_m = n_w = 0
    for k, (name, rules) in enumerate(_rule_sets()):
        model = sm.StageModel(rules)
        rng = random.Random(700 + k)
        custom = [r for r in rules[len(builtin_rules()):] if r.Regex]
        texts = _planted_texts(rng, rules if k == 0 else custom, 60 if k == 0 else 12)
        # files of multi-byte runes around the samples (the NFA stays on continuation bytes)
        texts += ["é日本 ".encode() + t + " ü€\U0001F600".encode() for t in texts[:20]]
        if k == 0:
            texts += [b"wide%d_" % n + b"abcdef" * 40 for n in (70, 150, 200)]
        a, w = _soundness(model, texts, widths)
        n_m, n_w = n_m + a, n_w + w
    assert widths == {1, 2, 3, 4}, widths
    assert n_m > 300 and n_w > 200, (n_m, n_w)


def test_nfa_model_rejects():
    """The model is no accept-all: windows that hold no match are rejected, and the injection
    stops at whi."""
    rules = builtin_rules()
    model = sm.StageModel(rules)
    r = [x.ID for x in rules].index("github-pat")
    nfa = model.info[r]["nfa"]
    tok = b" ghp_" + b"A1b2" * 9 + b" "
    x = b"0123456789" + tok + b"0123456789" * 5
    assert nfa.accepts(x, 10, 10) and nfa.accepts(x, 0, 10) and nfa.accepts(x, 7, 14)
    assert not nfa.accepts(x, 0, 8)                      # the injection ends before the match start
    assert not nfa.accepts(x, 12, 60)                    # starts behind it
    assert not nfa.accepts(x[:30], 10, 10)               # the file ends inside the token
    assert not nfa.accepts(x.replace(b"A1b2" * 9, b"A1b2" * 4 + b"-" + b"A1b2" * 4), 10, 10)


def test_keyword_model_is_the_tables():
    """ASCII case-insensitive containment = the keyword items of the compiled tables, run exactly."""
    rules = builtin_rules()
    model = sm.StageModel(rules)
    rng = random.Random(5)
    contents = _planted_texts(rng, rules, 40)
    contents += [k.upper() + b" x" for k in model.keywords] + [b"a" + k + b"b" for k in model.keywords]
    contents = [x for x in contents if not any(r in x for r in (sm.RUNE_I, sm.RUNE_K, sm.RUNE_S))]
    b = sm.Batch(contents)
    got = set()
    model.fm.run(b.a, b.offs, got)
    bits, exact = model.keyword_bits(b, model.file_flags(b), True)
    assert exact == list(range(len(contents))) and bits == got and len(bits) > 30


CASES = {
    "boundaries": sc.case_boundaries, "arena-edges-0": lambda: sc.case_arena_edges(0),
    "arena-edges-5": lambda: sc.case_arena_edges(5), "files": sc.case_files,
    "tail-newlines": lambda: sc.case_tail(b"\n"), "tail-rune": lambda: sc.case_tail(sm.RUNE_I),
    "dense": sc.case_dense, "follow": sc.case_follow, "class-runs": sc.case_class_runs, "fold": sc.case_fold,
    "fullscan": sc.case_fullscan, "gates": sc.case_gates, "finalize": sc.case_finalize,
}
MODEL_ONLY = {"fold", "fullscan", "gates"}  # cases whose candidates the models do not derive (coverage needs the engine)


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_hold_on_the_models(name, monkeypatch):
    case = CASES[name]()
    model = sc.model_of(case, monkeypatch)
    b = case["batch"]
    e = model.expect(b)
    d = model.synth_dump(b, e)
    matches = model.true_matches(b)
    if name in MODEL_ONLY:
        for check in (sm.check_overflow, lambda x: sm.check_chunks(x, e), lambda x: sm.check_blocks(x, e),
                      lambda x: sm.check_hits(x, e, b), lambda x: sm.check_keywords(x, e, model),
                      lambda x: sm.check_flags(x, e, b), lambda x: sm.check_candidates(x, e, model),
                      lambda x: sm.check_fields(x, e, model, b)):
            check(d)
        n = sum(len(v) for v in matches.values())
    else:
        n = sm.check_all(d, e, model, b, matches)
        sc.check_case(case, d, e, model)
    lo = case["min"]
    assert len(e.hits_required) >= lo[0] and n >= lo[2], (len(e.hits_required), n, lo)
    if name not in MODEL_ONLY:
        assert len(d.cands) >= lo[1]
    sc.check_case_shape(name, case, e, model)


def _small():
    rng = random.Random(3)
    files = [sc.filler(100) + sc.tok_aws(rng) + sc.filler(100), sc.filler(200) + sc.tok_ghp(rng) + b"\n" + sc.filler(30),
             sc.filler(50) + sc.tok_hook(rng) + sc.filler(70), sc.filler(40)]
    model = sm.StageModel(builtin_rules())
    b = sm.Batch(files)
    e = model.expect(b)
    return model, b, e, model.synth_dump(b, e)


def _cand_of(d, model, rule_id):
    r = [x.ID for x in model.rules].index(rule_id)
    return int(np.nonzero(d.cands["rule"] == r)[0][0])


def _drop_hit(d, model):
    d.hits.pop(1)
    d.counters[sm.CT_HITS] -= 1


def _move_hit(d, model):
    f, end, aid = d.hits[0]
    d.hits[0] = (f + 1, end, aid)


def _clear_kw(d, model):
    k = model.keywords.index(b"akia")
    assert d.kw_bit(0, k)
    d.kw[0, k >> 5] &= ~np.uint32(1 << (k & 31))


def _leak_kw(d, model):
    k = model.keywords.index(b"akia")
    assert not d.kw_bit(1, k)
    d.kw[1, k >> 5] |= np.uint32(1 << (k & 31))


def _field(name, index, delta=None, value=None):
    def f(d, model):
        i = _cand_of(d, model, "github-pat")
        x = d.cands[name]
        if index is None:
            x[i] = x[i] + delta
        else:
            assert x[i][index] not in (sm.NL_NONE, sm.NL_UNKNOWN)
            x[i][index] = np.uint32(int(x[i][index]) + delta if value is None else value)
    return f


def _remove_cand(d, model):
    d.cands = np.delete(d.cands, _cand_of(d, model, "slack-web-hook"))
    d.counters[sm.CT_CANDS] -= 1


def _narrow(d, model):
    d.cands["wlo"][_cand_of(d, model, "github-pat")] += 1


def _narrow_hi(d, model):
    d.cands["whi"][_cand_of(d, model, "github-pat")] -= 1


def _drop_open(d, model):
    i = _cand_of(d, model, "aws-access-key-id")
    assert d.cands["flags"][i] & sm.GATE_OPEN
    d.cands["flags"][i] |= sm.DROP


def _bump(attr, index, delta):
    def f(d, model):
        getattr(d, attr)[index] += delta
    return f


def _drop_block(d, model):
    d.recs = d.recs[1:]
    d.counters[sm.CT_RECS] -= 1


def _dup_block(d, model):
    d.recs = np.concatenate([d.recs, d.recs[:1]])
    d.counters[sm.CT_RECS] += 1


def _overflow(d, model):
    d.counters[sm.CT_HIT_OVF] = 1


CORRUPTIONS = {
    "drop one hit": (_drop_hit, "check_hits"),
    "move one hit to the neighbouring file": (_move_hit, "check_hits"),
    "clear one keyword bit": (_clear_kw, "check_keywords"),
    "set a keyword bit in the next file": (_leak_kw, "check_keywords"),
    "nl_before + 1": (_field("nl_before", None, 1), "check_fields"),
    "nl_before - 1": (_field("nl_before", None, -1), "check_fields"),
    "nl_back off by one": (_field("nl_back", 1, 1), "check_fields"),
    "nl_fwd off by one": (_field("nl_fwd", 0, -1), "check_fields"),
    "kNlUnknown where the distance is short": (_field("nl_back", 0, value=sm.NL_UNKNOWN), "check_fields"),
    "kNlUnknown forwards where the distance is short": (_field("nl_fwd", 0, value=sm.NL_UNKNOWN), "check_fields"),
    "kNlNone where a newline exists": (_field("nl_fwd", 0, value=sm.NL_NONE), "check_fields"),
    "remove one candidate": (_remove_cand, "check_candidates"),
    "narrow one window by one": (_narrow, "check_candidates"),
    "narrow one window from above": (_narrow_hi, "check_candidates"),
    "kCandDrop on a candidate whose gate is open": (_drop_open, "check_fields"),
    "a newline count + 1": (_bump("nl", 0, 1), "check_chunks"),
    "a chunk of the neighbouring file": (_bump("chunk_file", 0, 1), "check_chunks"),
    "a flag on a plain file": (_bump("flags", 1, 1), "check_flags"),
    "drop one flagged block": (_drop_block, "check_blocks"),
    "a flagged block twice": (_dup_block, "check_blocks"),
    "an overflow counter": (_overflow, "check_overflow"),
}


@pytest.fixture(scope="module")
def small():
    return _small()


def _run(check, d, e, model, b):
    args = {"check_overflow": (d,), "check_chunks": (d, e), "check_blocks": (d, e), "check_hits": (d, e, b),
            "check_keywords": (d, e, model), "check_flags": (d, e, b), "check_candidates": (d, e, model),
            "check_fields": (d, e, model, b)}[check]
    getattr(sm, check)(*args)


def test_the_clean_dump_passes(small):
    model, b, e, d = small
    assert sm.check_all(d, e, model, b) == 3 and len(d.hits) >= 3 and len(d.cands) == 3


@pytest.mark.parametrize("name", sorted(CORRUPTIONS))
def test_checkers_reject(small, name):
    model, b, e, clean = small
    corrupt, check = CORRUPTIONS[name]
    d = copy.deepcopy(clean)
    corrupt(d, model)
    with pytest.raises(AssertionError):
        _run(check, d, e, model, b)
    with pytest.raises(AssertionError):
        sm.check_all(d, e, model, b)
    for other in ("check_overflow", "check_chunks", "check_blocks", "check_hits", "check_keywords", "check_flags",
                  "check_candidates", "check_fields"):
        _run(other, clean, e, model, b)  # (the clean dump was not touched)


def test_coverage_check_rejects(small):
    """Invariant 6 fails when a true match loses its candidate, or keeps only a dropped one."""
    model, b, e, clean = small
    for how in ("remove", "drop", "shift"):
        d = copy.deepcopy(clean)
        i = _cand_of(d, model, "github-pat")
        if how == "remove":
            d.cands = np.delete(d.cands, i)
        elif how == "drop":
            d.cands["flags"][i] |= sm.DROP
        else:
            d.cands["wlo"][i] += 5
            d.cands["whi"][i] += 5
        with pytest.raises(AssertionError):
            sm.check_coverage(d, model, b)


def test_stage_dump_layout_and_argument_errors(tmp_path):
    """tsg_debug_stage_dump as the C compiler lays it out; argument errors come before the GPU."""
    import ctypes
    import subprocess
    names = [n for n, _ in sm._CStageDump._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tsg_debug.h"\nint main(void){'
                   'printf("%zu", sizeof(tsg_debug_stage_dump));'
                   + "".join('printf(" %%zu", offsetof(tsg_debug_stage_dump, %s));' % n for n in names)
                   + " return 0;}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == ctypes.sizeof(sm._CStageDump)
    for name, off in zip(names, got[1:]):
        assert getattr(sm._CStageDump, name).offset == off, name
    L = _lib.lib()
    model = sm.StageModel(builtin_rules())
    L.tsg_debug_engine_stages.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
                                          ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    d = sm._CStageDump()
    off = np.array([0, 4], dtype=np.uint64)
    tail = (ctypes.c_uint8 * 64)()
    assert L.tsg_debug_engine_stages(model.fm.h, 0, b"abcd", 4, off.ctypes.data, 1, tail, ctypes.byref(d)) == -2
    assert "struct_size" in _lib.last_error()
    d.struct_size = ctypes.sizeof(sm._CStageDump)
    assert L.tsg_debug_engine_stages(model.fm.h, 0, b"abcd", 5, off.ctypes.data, 1, tail, ctypes.byref(d)) == -2
    assert "n_bytes" in _lib.last_error()
    assert L.tsg_debug_engine_stages(model.fm.h, 0, b"abcd", 4, off.ctypes.data, 1, None, ctypes.byref(d)) == -2
