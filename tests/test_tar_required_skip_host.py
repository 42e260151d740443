"""LayerTar's skip options in the Required stage of a resident tar layer (tsg_analyzer_set_tar_required_skip),
the parts that need no GPU.

* the pattern classifier (trivy_amd/csrc/tar_skip_dev.h) against a table of accepted and refused patterns;
* the device's matcher -- the model's and the native one -- against doublestar.Match (tsg_doublestar_match,
  which is skip_path.h's DoubleStarMatch) and oracle.analyzer.skip_path, for every accepted pattern over a table
  of names;
* the three-case under rule against tar.go's underSkippedDir as tests/tar_skip_model.py restates it;
* the model's output (tests/tar_required_skip_model.py) through the host half (tsg_debug_index_tar_files)
  against the host half of walk mode 1 with the same options (tsg_debug_index_tar_entries) and against
  tests/tar_skip_model.walk;
* the setter, TSG_TAR_REQUIRED_SKIP, the new struct's layout, argument errors.
"""
import ctypes as c
import itertools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import analyzer as oan
from oracle import hostlib
from tests import tar_chain_model as cm
from tests import tar_required_model as rm
from tests import tar_required_skip_model as km
from tests import tar_skip_model as sm

ROOT = Path(__file__).resolve().parent.parent
TEXT = cm.TEXT

# (pattern, the form the device takes it in, or None)
PATTERNS = [
    ("vendor", km.EXACT), ("usr/share/doc", km.EXACT), ("a b/c", km.EXACT), ("..foo/x", km.EXACT),
    ("**/node_modules", km.ANY_DIR), ("**/a/b", km.ANY_DIR), ("**/.cache", km.ANY_DIR),
    ("vendor/**", km.BELOW), ("usr/share/**", km.BELOW),
    ("**/*.pem", km.SUFFIX), ("**/*_test.go", km.SUFFIX), ("**/*x", km.SUFFIX), ("**/*...", km.SUFFIX),
    ("a" * 255, km.EXACT), ("**/" + "a" * 255, km.ANY_DIR),
    ("a/*/b", None), ("{a,b}", None), ("[ab]", None), ("a?", None), ("a\\b", None), ("**", None), ("**/", None),
    ("**/*", None), ("**/**", None), ("*", None), ("*.pem", None), ("**/*.p*m", None), ("**/*a/b", None),
    ("café", None), ("**/*.é", None), ("..", None), ("a/../b", None), ("**/..", None), ("./a", None),
    ("a/./b", None), ("/a", None), ("a/", None), ("a//b", None), ("", None), ("a/**/b", None), ("**/a/**", None),
    ("**/*.", None), ("**/*..", None), ("a" * 256, None), ("**/*" + "a" * 256, None), ("/**", None),
]
ACCEPTED = [p for p, f in PATTERNS if f is not None]

# cleaned paths (bytes): component-boundary near misses, a base name equal to S, non-ASCII and invalid UTF-8
# before S, "..foo" elements
NAMES = [b"vendor", b"xvendor", b"vendor2", b"a/vendor/b", b"a/vendor", b"vendor/a", b"vendor/a/b", b"a/xvendor",
         b"usr/share/doc", b"usr/share/docs", b"usr/share/doc/x", b"usr/share", b"usr", b"x/usr/share/doc",
         b"node_modules", b"a/node_modules", b"a/node_modules/b", b"a/xnode_modules", b"node_modules2",
         b"a/b", b"x/a/b", b"xa/b", b"a/b/c", b"a", b"b", b".cache", b"h/.cache", b"h/x.cache",
         b".pem", b"a.pem", b"d/.pem", b"d/a.pem", b"a.pem/x", b"a.pemx", b"pem", b"d.pem/k",
         b"caf\xc3\xa9.pem", b"\xc3.pem", b"\xff\xfe.pem", b"d/\xe2\x82.pem", b"\xc3\xa9x", b"d/\xf0\x9f\x98x",
         b"m_test.go", b"_test.go", b"d/_test.go", b"x", b"xx", b"d/x", b"...", b"a...", b"d/....",
         b"..foo/x", b"..foo", b"..foo/x/y", b"a/..foo/x", b"a b/c", b"a b", b"a" * 255, b"d/" + b"a" * 255,
         b"a" * 254, b"a" * 256, b"usr/share/" + b"a" * 255]


def _analyzer(skip_switch=None):
    from trivy_amd.analyzer import AnalyzerOptions, SecretAnalyzer
    a = SecretAnalyzer(lib=hostlib.lib(), host_only=True)
    a.Init(AnalyzerOptions())
    L = a._L
    L.tsg_debug_index_tar_entries.argtypes = [c.c_void_p, c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint64, c.c_void_p,
                                              c.c_uint64, c.c_uint64, c.POINTER(c.c_void_p), c.c_void_p]
    L.tsg_debug_index_tar_files.argtypes = [c.c_void_p, c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint64, c.c_void_p,
                                            c.c_void_p, c.c_uint64, c.c_uint64, c.POINTER(c.c_void_p), c.c_void_p]
    L.tsg_debug_tar_skip_classify.argtypes = [c.POINTER(c.c_char_p), c.c_uint32, c.POINTER(c.c_char_p), c.c_uint32,
                                              c.c_void_p]
    L.tsg_debug_tar_skip_match.argtypes = [c.c_char_p, c.c_char_p, c.c_uint32]
    L.tsg_doublestar_match.argtypes = [c.c_char_p, c.c_char_p]
    if skip_switch:
        a.set_tar_required_skip(skip_switch)
    return a


@pytest.fixture(scope="module")
def an():
    return _analyzer()


def _err(a):
    from trivy_amd import _lib
    return _lib.last_error(a._L)


def _classify(a, dirs, files):
    """tsg_debug_tar_skip_classify: the forms, or None when the device does not take the set."""
    d = (c.c_char_p * max(1, len(dirs)))(*[p.encode() for p in dirs])
    f = (c.c_char_p * max(1, len(files)))(*[p.encode() for p in files])
    forms = np.full(len(dirs) + len(files), 255, dtype=np.uint8)
    rc = a._L.tsg_debug_tar_skip_classify(d, len(dirs), f, len(files), forms.ctypes.data if len(forms) else None)
    assert rc in (0, 1), _err(a)
    return forms.tolist() if rc == 1 else None


def test_pattern_classifier(an):
    for p, form in PATTERNS:
        got = km.form_of(p.encode())
        assert (got[0] if got else None) == form, p[:40]
        if p == "":
            continue  # (CleanSkipPaths never hands an empty pattern on; the C array cannot tell it from none)
        for as_dir in (True, False):
            native = _classify(an, [p] if as_dir else [], [] if as_dir else [p])
            assert native == (None if form is None else [form]), p[:40]
    # one refused pattern refuses the set; the caps: 32 of a kind, 2 KiB of literals
    assert _classify(an, ["vendor", "a/*/b"], ["**/*.pem"]) is None
    assert _classify(an, ["vendor"], ["**/*.pem", "{a,b}"]) is None
    assert _classify(an, ["vendor", "**/x", "y/**"], ["**/*.pem"]) == [km.EXACT, km.ANY_DIR, km.BELOW, km.SUFFIX]
    many = ["d%d" % i for i in range(33)]
    assert _classify(an, many[:32], many[:32]) == [km.EXACT] * 64
    assert _classify(an, many, []) is None and _classify(an, [], many) is None
    assert km.classify([p.encode() for p in many], []) is None
    big = [("%02d" % i) + "a" * 253 for i in range(9)]  # 255 bytes each: eight fit 2 KiB, nine do not
    assert _classify(an, big[:8], []) == [km.EXACT] * 8 and _classify(an, big[:4], big[4:8]) == [km.EXACT] * 8
    assert _classify(an, big[:8], ["x"] * 8) == [km.EXACT] * 16  # 2,048 bytes exactly
    assert _classify(an, big, []) is None and _classify(an, big[:8], ["x"] * 9) is None
    assert km.classify([p.encode() for p in big], []) is None
    assert km.classify([p.encode() for p in big[:8]], [b"x"] * 8) is not None
    assert _classify(an, [], []) == []


def test_matcher_is_doublestar_match_for_the_accepted_forms(an):
    L = an._L
    for p in ACCEPTED:
        form, lit = km.form_of(p.encode())
        for fp in NAMES:
            want = L.tsg_doublestar_match(p.encode(), fp)
            assert want in (0, 1), (p[:40], fp[:40])
            assert km.match_one(form, lit, fp) == bool(want), (p[:40], fp[:40])
            assert L.tsg_debug_tar_skip_match(p.encode(), fp, len(fp)) == want, (p[:40], fp[:40])
            assert oan.skip_path(fp.decode("utf-8", "surrogateescape"), [p]) == bool(want), (p[:40], fp[:40])
    assert L.tsg_debug_tar_skip_match(b"a/*/b", b"a/x/b", 5) == -1
    # every form matches something and refuses something in the table
    for p in ACCEPTED:
        form, lit = km.form_of(p.encode())
        hits = [km.match_one(form, lit, fp) for fp in NAMES]
        assert any(hits) and not all(hits), p[:40]


def test_three_case_under_rule_is_under_skipped_dir():
    """On clean, non-empty names without a ".." element -- "..foo" elements included -- for every recorded list
    of up to three directories from the table, in order."""
    names = [n.decode("utf-8", "surrogateescape") for n in NAMES if len(n) < 64]
    dirs = ["vendor", "a/vendor", "usr/share/doc", "a/b", "a", "..foo/x", "..foo", "a/..foo/x", "x/a/b", "usr/share",
            "a b/c", "d/.pem"]
    n_checked = 0
    for k in (1, 2, 3):
        for rec in itertools.permutations(dirs, k):
            first, parent_first = {}, {}
            for rank, d in enumerate(rec):
                km.record(first, parent_first, d.encode(), 512 * rank)
            for upto in range(k + 1):  # the file's rank: after `upto` of the directories
                rank = 512 * upto - 256
                for fp in names:
                    want = sm.under_skipped_dir(fp, list(rec[:upto]))
                    assert km.under(fp.encode("utf-8", "surrogateescape"), rank, first, parent_first) == want, \
                        (fp, rec, upto)
                    n_checked += 1
    assert n_checked > 100000


# ---- the host half -------------------------------------------------------------
def _layer(entries) -> bytes:
    """(kind, raw name): "f" a regular file with TEXT, "d" a directory (typeflag '5'), "0d" a '\\0' entry."""
    out = b""
    for kind, name in entries:
        out += cm.member(name, TEXT, b"0") if kind == "f" else cm.member(name, b"", b"5" if kind == "d" else b"\0")
    return out + cm.TRAILER


LAYERS = {
    # name: (layer, skip_dirs, skip_files, falls back)
    "ustar": (cm.ustar_layer, ["srv/dir", "**/etc"], ["**/*-3.txt", "etc/short-4.conf"], False),
    "odd-names": (cm.odd_names_layer, ["old/regadir", "**/abs"], ["**/up.conf", "tail.conf", "**/*c.conf"], False),
    "dir-after-files-and-twice": (lambda: _layer([
        ("f", b"app/skipme/early.conf"), ("f", b"app/keep.conf"), ("d", b"app/skipme/"), ("f", b"app/skipme/a.conf"),
        ("d", b"app/skipme"), ("f", b"app/skipme/deep/b.conf"), ("f", b"app/skipmez.conf"), ("0d", b"./app/skipme/"),
        ("f", b"/app/skipme/c.conf"), ("f", b"app/other.conf")]), ["**/skipme"], [], False),
    "file-equals-dir": (lambda: _layer([("f", b"x/y"), ("d", b"x/y"), ("f", b"x/y"), ("f", b"x/yz"), ("f", b"x")]),
                        ["x/y"], [], False),
    "file-is-direct-parent": (lambda: _layer([("f", b"c/d"), ("d", b"c/d/e"), ("f", b"c"), ("f", b"c/d"),
                                              ("f", b"c/d/e2"), ("f", b"c/dx"), ("d", b"top"), ("f", b"top2")]),
                              ["c/d/e", "top"], [], False),
    "asked-names": (lambda: _layer([
        ("f", b"w/./skipme/before.conf"), ("d", b"w/skipme"), ("f", b"w/./skipme/x.conf"), ("f", b"w//keep.conf"),
        ("f", b"w/./k.pem"), ("f", b"w/skipme/../out.conf"), ("f", b"../w/skipme/up.conf"), ("d", b"w/./other/"),
        ("f", b"w/other/y.conf"), ("f", b"w/z.pem")]), ["**/skipme"], ["**/*.pem"], False),
    "asked-dir-matches": (lambda: _layer([("f", b"z/a.conf"), ("d", b"z/./skipme/"), ("f", b"z/skipme/x.conf"),
                                          ("f", b"z/b.conf")]), ["**/skipme"], [], True),
}


def _stats():
    from trivy_amd.analyzer.secret import DEVICE_TAR_STATS_SIZE_V1, _CDeviceTarStats
    st = _CDeviceTarStats()
    st.struct_size = DEVICE_TAR_STATS_SIZE_V1
    return st


def _ptr(a):
    return a.ctypes.data if len(a) else None


def _set(a, skip_dirs, skip_files):
    from trivy_amd.walker import NewLayerTar, Option
    w = NewLayerTar(Option(SkipFiles=list(skip_files), SkipDirs=list(skip_dirs)))
    assert (w.skipDirs, w.skipFiles) == (list(skip_dirs), list(skip_files))  # the patterns are clean
    a.set_layer_walker(w)


def _index_entries(a, entries, stop, n_cand, n_bytes):
    from trivy_amd.analyzer.secret import DeviceTarIndex
    recs, names = cm.pack(entries)
    stop_a = np.array(stop, dtype=np.uint64)
    st, h = _stats(), c.c_void_p()
    rc = a._L.tsg_debug_index_tar_entries(a._h, _ptr(recs), len(entries), _ptr(names), len(names), stop_a.ctypes.data,
                                          n_bytes, n_cand, c.byref(h), c.byref(st))
    assert rc == 0, _err(a)
    return DeviceTarIndex(a, h, None, st.to_dict())


def _index_files(a, frecs: bytes, blob: bytes, counts, stop, n_cand, n_bytes, want_rc=0):
    from trivy_amd.analyzer.secret import DeviceTarIndex
    fr = np.frombuffer(frecs or b"\0", dtype=np.uint8)
    bl = np.frombuffer(blob or b"\0", dtype=np.uint8)
    cnt = np.ascontiguousarray(counts, dtype=np.uint64)
    stop_a = np.array(stop, dtype=np.uint64)
    st, h = _stats(), c.c_void_p()
    rc = a._L.tsg_debug_index_tar_files(a._h, fr.ctypes.data if frecs else None, len(frecs) // 48,
                                        bl.ctypes.data if blob else None, len(blob), cnt.ctypes.data, stop_a.ctypes.data,
                                        n_bytes, n_cand, c.byref(h), c.byref(st))
    assert rc == want_rc, (rc, _err(a))
    return DeviceTarIndex(a, h, None, st.to_dict()) if rc == 0 else None


def _pool(ix):
    if ix.n == 0:
        return b""
    pp, pl = c.c_void_p(), c.c_uint64()
    assert ix._an._L.tsg_tar_index_file(ix._h, 0, c.byref(pp), c.byref(pl), None, None) == 0
    total = sum(len(p.encode("utf-8", "surrogateescape")) + 1 for p, _, _ in ix.files())
    return c.string_at(pp, total)


@pytest.mark.parametrize("name", list(LAYERS))
def test_model_through_the_host_half_equals_the_host_half_and_the_walk(name):
    make, skip_dirs, skip_files, falls_back = LAYERS[name]
    layer = make()
    an = _analyzer("gpu")
    pt, st = rm.tables_of(an)
    oracle = oan.SecretAnalyzer("")
    entries, stop, n_cand = cm.chain(layer)
    assert stop[0] == cm.END, stop
    recs, names = cm.pack(entries)
    verdicts, frecs, blob, counts = km.stage(recs, len(entries), bytes(names), [0, len(entries)], [0, len(names)], b".",
                                             pt, st, [p.encode() for p in skip_dirs], [p.encode() for p in skip_files])
    _set(an, skip_dirs, skip_files)
    want = _index_entries(an, entries, stop, n_cand, len(layer))  # the host half of walk mode 1, same options
    assert want.required_stats["reason"] == 1 and want.required_skip_stats["reason"] == 4
    m = sm.walk(layer, skip_dirs, skip_files)
    walk_skip = {"skipped_dirs": len(m["skipped_dirs"]), "skipped_files": m["skipped_files"],
                 "under_skipped_dir": m["under_skipped_dir"]}
    assert want.skip_stats == walk_skip
    assert [(p, s) for p, _, s in want.files()] == [(fp, size) for fp, size, _ in m["kept"] if oracle.required(fp, size)]
    assert sum(walk_skip.values()) > 0  # the options bite in every layer
    if falls_back:
        assert _index_files(an, frecs, blob, counts[0], stop, n_cand, len(layer), want_rc=1) is None
        assert "skipped directory" in _err(an)
        return
    got = _index_files(an, frecs, blob, counts[0], stop, n_cand, len(layer))
    assert got.files() == want.files() and _pool(got) == _pool(want)
    assert got.start.tolist() == want.start.tolist() and got.data_off.tolist() == want.data_off.tolist()
    assert got.size.tolist() == want.size.tolist()
    for k in ("entries", "regular", "required", "whiteouts", "opaque_dirs", "blocks", "candidates", "off_chain",
              "block_fetches", "ext_bytes", "kernel_runs"):
        assert got.stats[k] == want.stats[k], k
    assert got.skip_stats == want.skip_stats
    assert got.stats["regular"] == m["regular"] and got.stats["whiteouts"] == m["whiteouts"]
    rs, ss = got.required_stats, got.required_skip_stats
    assert rs["mode"] == "gpu" and rs["reason"] == 0 and rs["entries"] == len(entries)
    assert (rs["kept"], rs["dropped"], rs["ask_allow"], rs["ask_name"]) == tuple(
        int((verdicts == v).sum()) for v in (rm.KEEP, rm.DROP, rm.ASK_ALLOW, rm.ASK_NAME))
    assert rs["kept"] + rs["ask_allow"] + rs["ask_name"] - rs["ask_dropped"] == got.n
    assert ss["mode"] == "gpu" and ss["reason"] == 0
    assert (ss["dir_patterns"], ss["file_patterns"]) == (len(skip_dirs), len(skip_files))
    assert {k: ss[k] for k in walk_skip} == walk_skip
    # the device's share of the counts is the model's
    assert int((verdicts == km.SKIP_DIR).sum()) == walk_skip["skipped_dirs"]
    assert int((verdicts == km.SKIP_FILE).sum()) <= walk_skip["skipped_files"]
    assert int((verdicts == km.SKIP_UNDER).sum()) <= walk_skip["under_skipped_dir"]
    # the switch off: the same records are refused (their counts name skipped entries), as without the feature
    an.set_tar_required_skip("host")
    if int(counts[0][14]) or int(counts[0][15]):
        assert _index_files(an, frecs, blob, counts[0], stop, n_cand, len(layer), want_rc=-1) is None


def test_asked_names_are_decided_by_the_host_in_its_order():
    """The asked-names layer: an asked file under a recorded directory, one before it, one a file pattern matches,
    one whose cleaned path leaves the directory."""
    make, skip_dirs, skip_files, _ = LAYERS["asked-names"]
    m = sm.walk(make(), skip_dirs, skip_files)
    assert [fp for fp, _, _ in m["kept"]] == ["w/skipme/before.conf", "w/keep.conf", "w/out.conf",
                                              "../w/skipme/up.conf", "w/other/y.conf"]
    assert sorted(m["dropped"]) == ["w/k.pem", "w/skipme/x.conf", "w/z.pem"]


# ---- plumbing ------------------------------------------------------------------
def test_setter_and_getter():
    an = _analyzer()
    L = an._L
    assert an.tar_required_skip() == "host"  # the default
    an.set_tar_required_skip("gpu")
    assert an.tar_required_skip() == "gpu" and an.tar_required() == "host"  # a switch of its own
    for bad in (2, 3, -1, 1 << 20):
        assert L.tsg_analyzer_set_tar_required_skip(an._h, bad) == -1
        assert "mode %d" % bad in _err(an)
        assert an.tar_required_skip() == "gpu"  # unchanged
    an.set_tar_required_skip("host")
    assert an.tar_required_skip() == "host"
    with pytest.raises(ValueError):
        an.set_tar_required_skip("device")
    m = c.c_int(9)
    assert L.tsg_analyzer_set_tar_required_skip(None, 1) == -1
    assert L.tsg_analyzer_get_tar_required_skip(None, c.byref(m)) == -1 and m.value == 9
    assert L.tsg_analyzer_get_tar_required_skip(an._h, None) == -1
    # the Required setter still refuses what is not one of its modes
    assert L.tsg_analyzer_set_tar_required(an._h, 2) == -1 and "mode 2" in _err(an)


def test_skip_stats_reasons_and_argument_errors():
    from trivy_amd.analyzer.secret import TAR_REQUIRED_SKIP_STATS_SIZE_V1, _CTarRequiredSkipStats
    an = _analyzer()
    entries, stop, n_cand = cm.chain(cm.ustar_layer())
    ix = _index_entries(an, entries, stop, n_cand, 1 << 20)
    assert ix.required_skip_stats["reason"] == 1 and ix.required_skip_stats["mode"] == "host"  # the switch is off
    an.set_tar_required_skip("gpu")
    assert _index_entries(an, entries, stop, n_cand, 1 << 20).required_skip_stats["reason"] == 2  # no options
    _set(an, ["a/*/b"], [])
    ss = _index_entries(an, entries, stop, n_cand, 1 << 20).required_skip_stats
    assert ss["reason"] == 3 and ss["dir_patterns"] == 1 and ss["mode"] == "gpu"  # patterns unsupported
    _set(an, ["srv/dir"], [])
    assert _index_entries(an, entries, stop, n_cand, 1 << 20).required_skip_stats["reason"] == 4  # (a host half)
    st = _CTarRequiredSkipStats()
    for bogus in (0, 8, TAR_REQUIRED_SKIP_STATS_SIZE_V1 - 8, TAR_REQUIRED_SKIP_STATS_SIZE_V1 + 8):
        st.struct_size = bogus
        assert an._L.tsg_tar_index_required_skip_stats(ix._h, c.byref(st)) == -1
        assert "struct_size %d" % bogus in _err(an)
    st.struct_size = TAR_REQUIRED_SKIP_STATS_SIZE_V1
    assert an._L.tsg_tar_index_required_skip_stats(None, c.byref(st)) == -1
    assert an._L.tsg_tar_index_required_skip_stats(ix._h, None) == -1
    assert an._L.tsg_tar_index_required_skip_stats(ix._h, c.byref(st)) == 0 and st.reason == 1


def test_env_sets_the_initial_mode():
    """TSG_TAR_REQUIRED_SKIP is read when an analyzer is made: in a child process, so this one's environment stays."""
    code = ("from oracle import hostlib\n"
            "from trivy_amd.analyzer import AnalyzerOptions, SecretAnalyzer\n"
            "a = SecretAnalyzer(lib=hostlib.lib(), host_only=True)\n"
            "a.Init(AnalyzerOptions())\n"
            "print(a.tar_required_skip(), a.tar_required())\n")
    for value, want in (("gpu", "gpu"), ("host", "host"), ("GPU", "host"), (None, "host")):
        env = dict(os.environ)
        for k in ("TSG_TAR_REQUIRED_SKIP", "TSG_TAR_REQUIRED", "TSG_TAR_WALK"):
            env.pop(k, None)
        if value is not None:
            env["TSG_TAR_REQUIRED_SKIP"] = value
        out = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), env=env, check=True, capture_output=True,
                             text=True).stdout.split()
        assert out[-2:] == [want, "host"], (value, out)


def test_struct_layout(tmp_path):
    from trivy_amd.analyzer.secret import (TAR_REQUIRED_SKIP_STATS_SIZE_V1, TAR_REQUIRED_STATS_SIZE_V1,
                                           _CTarRequiredSkipStats)
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "tsg_analyzer.h"\nint main(void){printf("%zu %u %zu %zu %zu %zu %zu %u\\n",'
                   ' sizeof(tsg_tar_required_skip_stats), (unsigned)TSG_TAR_REQUIRED_SKIP_STATS_SIZE_V1,'
                   ' offsetof(tsg_tar_required_skip_stats, reason), offsetof(tsg_tar_required_skip_stats, file_patterns),'
                   ' offsetof(tsg_tar_required_skip_stats, skipped_dirs), offsetof(tsg_tar_required_skip_stats, table_slots),'
                   ' offsetof(tsg_tar_required_skip_stats, ms_kernel), (unsigned)TSG_TAR_REQUIRED_STATS_SIZE_V1);'
                   ' return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    size, v1, o_reason, o_fp, o_dirs, o_slots, o_ms, req_v1 = \
        [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _CTarRequiredSkipStats
    assert size == v1 == c.sizeof(S) == TAR_REQUIRED_SKIP_STATS_SIZE_V1 == 24 + 4 * 8 + 8
    assert o_reason == S.reason.offset == 12 and o_fp == S.file_patterns.offset == 20
    assert o_dirs == S.skipped_dirs.offset == 24 and o_slots == S.table_slots.offset == 48
    assert o_ms == S.ms_kernel.offset == 56
    assert req_v1 == TAR_REQUIRED_STATS_SIZE_V1 == 16 + 7 * 8 + 3 * 8  # tsg_tar_required_stats keeps its V1 size
