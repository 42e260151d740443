"""Prefilter windows and buckets chosen by measurement on a calibration sample.

With a sample the rule compiler clusters the item windows by the fires it counts on a prefix of
the sample instead of the static byte prior's estimate (filter.cpp MeasuredBuckets).  Checked here
on the CPU model (tests/filter_model.py): the flagged-block rate on held-out bytes against the
prior's clustering (TSG_CALIB_BUCKETS=0: the same calibrated anchor choice, the static prior's
windows and buckets), the rate on foreign data, coverage of every true match, the tables'
structure, their independence of the thread count, and -- without a sample -- tables byte for
byte those of the build before this method existed.
"""
import ctypes as c
import hashlib
import os
import random
from pathlib import Path

import numpy as np
import pytest
import yaml

from tests.corpus import make_corpus
from tests.filter_model import FilterModel
from tests.test_filter_model import _calibration_sample, _check, _planted_texts
from trivy_amd import _lib, corpus
from trivy_amd.secret import ParseConfig, builtin_rules

ROOT = Path(__file__).resolve().parent.parent
SAMPLE_BYTES = 16_000_000

_CACHE = {}


def _c2():
    """24 MB of the C2 generator's corpus as bench.py builds it: (first 16 MB, held-out 8 MB)."""
    if "c2" not in _CACHE:
        C = corpus.generate(24e6, crlf_share=0.05).stripped()
        a = np.asarray(C.arena[:C.n_bytes], dtype=np.uint8).copy()
        _CACHE["c2"] = (a[:SAMPLE_BYTES], a[SAMPLE_BYTES:])
    return _CACHE["c2"]


def _model(key, env=None, calibration=None, rules=None):
    """A FilterModel compiled under env (cached by key)."""
    if key not in _CACHE:
        old = {k: os.environ.get(k) for k in (env or {})}
        os.environ.update(env or {})
        try:
            _CACHE[key] = FilterModel(rules if rules is not None else builtin_rules(), calibration=calibration)
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
    return _CACHE[key]


def _new():
    return _model("new", calibration=_c2()[0])


def _parent():
    return _model("parent", {"TSG_CALIB_BUCKETS": "0"}, calibration=_c2()[0])


def _flagged_blocks(m, a):
    """16-B blocks of `a` holding a window end at which an item bucket fires (what K1 hands K2)."""
    a = np.concatenate([np.zeros(8, dtype=np.uint8), np.asarray(a, dtype=np.uint8)])
    n = len(a)
    any_ = np.zeros(n, dtype=bool)
    for j in range(m.n_buckets - 1):
        if m.bucket_off[j + 1] == m.bucket_off[j]:
            continue
        ok = np.ones(n, dtype=bool)
        for s in range(m.window):
            sh = m.window - 1 - s
            col = m.allowed(j, s)[a]
            ok[sh:] &= col[:n - sh] if sh else col
            ok[:sh] = False
        any_ |= ok
    any_ = any_[8:]
    k = len(any_) // 16 * 16
    return int(any_[:k].reshape(-1, 16).any(axis=1).sum())


def _tables_digest(m):
    h = hashlib.sha256()
    for x in (np.array([m.n_buckets, m.window, m.n_words], dtype=np.uint32), m.reach, m.bucket_off, m.bucket_items,
              m.item_cls, m.classes.astype(np.uint8), m.item_ids, np.array([m.fp_est], dtype=np.float64)):
        h.update(np.ascontiguousarray(x).tobytes())
    for it in m.items:
        h.update(repr(sorted(it.items())).encode())
    return h.hexdigest()


def test_held_out_rate():
    """Sample: the first 16 MB; rate on the 8 MB behind it.  At most 0.86 x the prior's clustering
    (the -14 % a crude greedy reached; measured at the introduction: 0.61 here and on 30 MB of C2)."""
    held = _c2()[1]
    new, old = _flagged_blocks(_new(), held), _flagged_blocks(_parent(), held)
    print("held-out flagged blocks: measured %d, prior %d, ratio %.3f" % (new, old, new / old))
    assert _new().n_calibrated == _parent().n_calibrated >= 1
    assert old > 1000
    assert new <= 0.86 * old


def test_foreign_data_not_worse():
    """Calibrated on C2, evaluated on other bytes: the rate must not exceed the prior's tables'."""
    files = make_corpus(7, 400)
    mc = np.frombuffer(b"".join(b for _, b in files), dtype=np.uint8)
    layer = corpus.generate_layer(4e6)  # a tar layer: headers and padding between the files
    for name, a in (("make_corpus", mc), ("generate_layer", layer)):
        new, old = _flagged_blocks(_new(), a), _flagged_blocks(_parent(), a)
        print("%s (%d bytes): measured %d, prior %d, ratio %.3f" % (name, len(a), new, old, new / max(old, 1)))
        assert new <= old, name


@pytest.mark.parametrize("seed", range(2))
def test_builtin_planted_matches_covered(seed):
    rules = builtin_rules()
    rng = random.Random(700 + seed)
    texts = _planted_texts(rng, rules, 120)
    texts += [b"color: linear-gradient(" + t for t in texts[:20]]
    n, _ = _check(rules, texts, calibration=_calibration_sample(seed))
    assert n > 50


def test_builtin_planted_matches_covered_c2_sample():
    rules = builtin_rules()
    n, _ = _check(rules, _planted_texts(random.Random(710), rules, 120), calibration=_c2()[0][:4 << 20])
    assert n > 50


def test_custom_rules_covered():
    rng = random.Random(19)
    seen = 0
    for f in sorted((ROOT / "tests/golden/scanner").glob("*.yaml")):
        d = yaml.safe_load(f.read_text()) or {}
        if not d.get("rules"):
            continue
        try:
            cfg = ParseConfig(str(f))
        except ValueError:
            continue
        rules = builtin_rules() + list(cfg.CustomRules or [])
        custom = [r for r in rules if r.Regex]
        _check(rules, _planted_texts(rng, custom, 25), calibration=_calibration_sample(1)[:1 << 20])
        seen += 1
        if seen == 3:  # (a compile each)
            break
    assert seen


def _slot_sets(m, it):
    """The item's window: (slot, bool[256]) for the positions ending at `back`."""
    wl = min(it["n"], m.window)
    cls = m.item_cls[it["cls_off"]:it["cls_off"] + it["n"]]
    return [(m.window - wl + q, m.classes[cls[it["back"] - wl + q]]) for q in range(wl)]


def test_structure():
    m = _new()
    nb = m.n_buckets - 1
    assert m.bucket_off[0] == 0 and m.bucket_off[nb] == m.bucket_off[nb + 1] == len(m.bucket_items)
    assert sorted(int(x) for x in m.bucket_items) == list(range(len(m.items)))  # each item in exactly one bucket
    moved = 0
    prior = _parent()
    for j in range(nb):
        for x in m.bucket_items[m.bucket_off[j]:m.bucket_off[j + 1]]:
            it = m.items[int(x)]
            assert min(it["n"], m.window) <= it["back"] <= it["n"]
            for s, allowed in _slot_sets(m, it):  # the window's sets lie inside the bucket's slot unions
                assert not (allowed & ~m.allowed(j, s)).any(), (j, int(x), s)
            moved += it["back"] != prior.items[int(x)]["back"]
    assert [(i["n"], i["kind"], i["lit_end"], i["n_ids"]) for i in m.items] == \
           [(i["n"], i["kind"], i["lit_end"], i["n_ids"]) for i in prior.items]
    print("windows that differ from the prior's choice: %d of %d" % (moved, len(m.items)))
    assert moved >= 1


def _core(m):
    L = _lib.lib()
    L.tsg_debug_filter_core.argtypes = [c.c_void_p, c.POINTER(c.c_uint32)]
    out = (c.c_uint32 * 4)()
    assert L.tsg_debug_filter_core(m.h, out) == 0
    return list(out)


def test_core_tables_stay_lds_sized():
    """The confirm kernel stages the class-compressed core tables (groups x classes x 8 B) in LDS
    when they fit beside its fixed 40-odd KB under the 80-KB limit of four workgroups per CU
    (engine.hip lds_tabs_).  The prior's builtin tables take 12.8 KB of it; the measured ones must
    stay under 16 KB, and no bucket may need more than two core groups per fire."""
    groups, classes, most, hashed = _core(_new())
    pg, pc, pm, _ = _core(_parent())
    print("core groups %d (prior %d), byte classes %d (%d), most groups in a bucket %d (%d)"
          % (groups, pg, classes, pc, most, pm))
    assert hashed == 0
    assert groups * classes * 8 <= 16 * 1024
    assert most <= 2


def test_tables_independent_of_threads_and_runs():
    sample = _c2()[0][:1 << 20]
    short = {"TSG_CALIB_PREFIX_KB": "512"}  # columns over 512 KiB: one thread works through them alone
    want = _tables_digest(_model("short", short, calibration=sample))
    for threads in ("1", "16"):
        got = _tables_digest(_model("threads" + threads, dict(short, TSG_COMPILE_THREADS=threads), calibration=sample))
        assert got == want, threads
    assert _tables_digest(_model("again", short, calibration=sample)) == want
    assert want != _tables_digest(_model("plain"))


# sha256 of the tables (the fields of _tables_digest) from the build before the measured method
PARENT_DIGESTS = {
    "builtin": "caca6ce242c53bdf25875169184e6f96c8700aee34501e2f21f60d4f25406ce3",
    "builtin-calib-prior": "922b6db1e109cad6cf0cb49647b47e8d5206b12730c8b1cce256826974e9f502",
    "class-runs": "d7ee8a754c7ce0a6c8ec58e371a86234d63fb9b9e5c79c8009fddb28b9440030",
}


def _class_run_rules():
    from tests.stage_cases import class_run_rules
    return class_run_rules()


def test_no_sample_tables_unchanged():
    assert _tables_digest(_model("plain")) == PARENT_DIGESTS["builtin"]
    assert _tables_digest(_model("plain-cr", rules=_class_run_rules())) == PARENT_DIGESTS["class-runs"]


def test_calib_prior_tables_unchanged():
    """TSG_CALIB_PRIOR=1: the sample's byte frequencies as the prior, no measurement."""
    m = _model("calib-prior", {"TSG_CALIB_PRIOR": "1"}, calibration=_calibration_sample(0))
    assert _tables_digest(m) == PARENT_DIGESTS["builtin-calib-prior"]
