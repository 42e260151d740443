"""The GPU's "surely allowed" path decision (pathfilter.h SureTable) vs the oracle.

A scan leaves out the bytes of the files whose path the path kernel finds
surely allow-listed, so the decision must never say yes where the reference's
AllowPath (scanner.go:57-59, 205-212) says no.  The host model of the kernel's
exact shift-and (tsg_debug_sure_allow: the same table builder, the same step)
is checked here over the parity suite's allow-path batch, a few thousand
mutations of it, and custom rules:

* sure => allowed, for every path;
* sure == allowed-by-a-rule-with-an-exact-form, for every ASCII path of at
  most 4096 bytes (so a classifier that never says yes does not pass).
"""
import ctypes as c
import json
import random
from pathlib import Path

import numpy as np
import pytest

from oracle import goregexp
from tests.test_gpu_parity import _allow_paths_batch
from trivy_amd import _lib

MAX_PATH = 4096  # pathfilter.h kSureMaxPath
BUILTIN = json.loads((Path(_lib.__file__).resolve().parent / "secret" / "builtin_rules.json").read_text())
BUILTIN_PATHS = [(a["id"], a["path"]) for a in BUILTIN["allow_rules"] if a["path"]]
# the builtin rules with an exact literal form; node.js and python have a repeat of a class
BUILTIN_FORMS = {"tests", "examples", "vendor", "usr-dirs", "locale-dir", "markdown", "golang", "rubygems",
                 "wordpress", "anaconda-log"}
CUSTOM = [("lock", r"(?i)\.lock$", True), ("build", r"^build/", True), ("Vendor", r"/Vendor/", True),
          ("locales", r"/locales?/", True), ("yarn", r"^opt/yarn-v[\d.]+/", False), ("ab", r"a|b", True)]


def _sure(patterns, paths):
    L = _lib.lib()
    L.tsg_debug_sure_allow.restype = c.c_int
    L.tsg_debug_sure_allow.argtypes = [c.POINTER(c.c_char_p), c.c_uint32, c.c_void_p, c.c_void_p, c.c_uint32,
                                       c.c_void_p, c.c_void_p]
    pats = (c.c_char_p * len(patterns))(*[p.encode() for p in patterns])
    off = np.zeros(len(paths) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in paths])
    blob = np.frombuffer(b"".join(paths) + b"\0", dtype=np.uint8).copy()
    sure = np.zeros(len(paths), dtype=np.uint8)
    form = np.zeros(len(patterns), dtype=np.uint8)
    rc = L.tsg_debug_sure_allow(pats, len(patterns), blob.ctypes.data, off.ctypes.data, len(paths),
                                sure.ctypes.data, form.ctypes.data)
    assert rc == 0, _lib.last_error()
    return sure.astype(bool), form.astype(bool)


@pytest.fixture(scope="module")
def path_sets():
    rng = random.Random(11)
    base = [p.encode() for p in _allow_paths_batch(random.Random(7))]
    edge = [b"", b"a", b"b", b"x.lock", b"x.LOCK", b"x.lock/y", b"build/x", b"a/build/x", b"Build/x", b"a/Vendor/b",
            b"a/vendor/b", b"a/VENDOR/b", b"opt/yarn-v1.2.3/a", b"test", b"atest", b"tes", b"md", b".md", b"x.md",
            b"x.mdx", b"x.md/", b"/locale/", b"/locales/", b"/localess/", b"usr/lib/", b"usr/lib", b"ausr/lib/x",
            "ſrc/test".encode(), "x/teſt".encode(), "a/Kendor/".encode(), b"z" * 4093 + b".md",
            b"z" * 4094 + b".md", b"test" + b"z" * 5000, b"\xff/test", b"a/test\xfe"]
    mut = []
    ends = b"/._-aAtTmMdDkKsSbx \x80\xc5"
    for _ in range(4000):
        p = bytearray(rng.choice(base))
        r = rng.random()
        if r < 0.4 and p:  # case flips
            for _ in range(rng.randint(1, 3)):
                i = rng.randrange(len(p))
                if chr(p[i]).isalpha() and p[i] < 0x80:
                    p[i] ^= 0x20
        elif r < 0.6:
            p.insert(0, rng.choice(ends))
        elif r < 0.8:
            p.append(rng.choice(ends))
        elif r < 0.9 and p:
            del p[0]
        elif p:
            del p[-1]
        mut.append(bytes(p))
    return base + edge + mut


def _check(rules, want_form, paths):
    """rules: (id, pattern); want_form: the ids that must have an exact form."""
    sure, form = _sure([r[1] for r in rules], paths)
    assert {r[0] for r, f in zip(rules, form) if f} == set(want_form)
    res = [goregexp.compile(r[1]) for r in rules]
    n_sure = 0
    for p, s in zip(paths, sure):
        hit = [re.match_string(p) for re in res]  # the reference alone, per rule
        allowed = any(hit)
        assert not s or allowed, p
        if all(b < 0x80 for b in p) and len(p) <= MAX_PATH:
            assert bool(s) == any(h for h, f in zip(hit, form) if f), p
        else:
            assert not s, p
        n_sure += int(s)
    return n_sure


def test_builtin_rules(path_sets):
    n = _check(BUILTIN_PATHS, BUILTIN_FORMS, path_sets)
    assert n > 1000  # the batch is built around the rules' literals


def test_custom_rules(path_sets):
    n = _check([(i, p) for i, p, _ in CUSTOM], {i for i, _, f in CUSTOM if f}, path_sets)
    assert n > 1000


def test_builtin_and_custom_rules_together(path_sets):
    """150 + 38 positions: the literals reach into the fourth shift-and word."""
    rules = BUILTIN_PATHS + [(i, p) for i, p, _ in CUSTOM]
    _check(rules, BUILTIN_FORMS | {i for i, _, f in CUSTOM if f}, path_sets)


def test_no_form_and_odd_shapes():
    paths = [b"", b"a", b"ab", b"abc", b"xabcx", b"ABC", b"abd", b"a\nb", b"b"]
    for pat, form in [(r"a.c", False), (r"[ab]c", False), (r"ab+", False), (r"(?m)^ab", False), (r"ab\b", False),
                      (r"", False), (r"a?", False), (r"(?i)ab?c", True), (r"^(?:a|b)$", True), (r"(a(b|c))d?", True),
                      (r"a{2}", False), (r"^abc$|^b$", True)]:
        sure, f = _sure([pat], paths)
        assert bool(f[0]) == form, pat
        re = goregexp.compile(pat)
        for p, s in zip(paths, sure):
            assert bool(s) == (form and re.match_string(p)), (pat, p)
