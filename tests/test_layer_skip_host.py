"""LayerTar's skipDirs / skipFiles in every layer walk (tsg_analyzer_set_tar_skip), the parts that need no GPU.

Through the host-only library: the host walk (tsg_collector_add_tar, copy and gather mode) and both host
halves of a resident layer's index -- the chain walk over candidate records (tsg_debug_index_tar_records,
walk mode 0) and the index from the GPU walk's entry records (tsg_debug_index_tar_entries, walk mode 1), fed
the models' records -- against tests/tar_skip_model.py, a restatement of walker/tar.go:35-116 over tarfile.
"""
import ctypes as c
import json
import os
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import analyzer as oan
from oracle import hostlib
from tests import tar_chain_model as cm
from tests import tar_index_model as tm
from tests import tar_skip_model as sm

ROOT = Path(__file__).resolve().parent.parent
CASES = sm.cases()
SKIP_KEYS = ("skipped_dirs", "skipped_files", "under_skipped_dir")


def _new_analyzer():
    from trivy_amd.analyzer import AnalyzerOptions, SecretAnalyzer
    a = SecretAnalyzer(lib=hostlib.lib(), host_only=True)
    a.Init(AnalyzerOptions())
    L = a._L
    L.tsg_debug_index_tar_records.argtypes = [c.c_void_p, c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint64,
                                              c.POINTER(c.c_void_p), c.c_void_p]
    L.tsg_debug_index_tar_entries.argtypes = [c.c_void_p, c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint64, c.c_void_p,
                                              c.c_uint64, c.c_uint64, c.POINTER(c.c_void_p), c.c_void_p]
    return a


@pytest.fixture(scope="module")
def an():
    return _new_analyzer()


@pytest.fixture(scope="module")
def oracle():
    return oan.SecretAnalyzer("")


def _err(a):
    from trivy_amd import _lib
    return _lib.last_error(a._L)


def _set(a, skip_dirs, skip_files):
    from trivy_amd.walker import NewLayerTar, Option
    w = NewLayerTar(Option(SkipFiles=list(skip_files), SkipDirs=list(skip_dirs)))
    assert (w.skipDirs, w.skipFiles) == (list(skip_dirs), list(skip_files))  # the cases' patterns are clean
    a.set_layer_walker(w)


def _want(oracle, layer, skip_dirs, skip_files):
    """The model's outcome: (the walk dict, the index [(filePath, size)] -- kept and Required)."""
    m = sm.walk(layer, skip_dirs, skip_files)
    return m, [(fp, size) for fp, size, _ in m["kept"] if oracle.required(fp, size)]


def _model_skip(m):
    return {"skipped_dirs": len(m["skipped_dirs"]), "skipped_files": m["skipped_files"],
            "under_skipped_dir": m["under_skipped_dir"]}


def _host_walk(a, layer, arena_bytes=1 << 20, gpu_transform=True, gather=False, colls=None):
    """The whole layer through tsg_collector_add_tar: (the scan paths, tsg_tar_stats, the skip counts of this
    walk, add_tar calls).  colls: collectors to fill in turn."""
    from trivy_amd.analyzer.secret import Collector, _CTarStats
    colls = colls or [Collector(a, arena_bytes, gpu_transform, gather)]
    buf = np.frombuffer(layer, dtype=np.uint8)
    before = a.tar_skip_stats()
    st, cur, files, calls = _CTarStats(), 0, [], 0
    while True:
        coll = colls[calls % len(colls)]
        rc, cur = coll.add_tar(buf, cur, st)
        calls += 1
        files += coll.paths()
        coll.reset()
        if rc == 0:
            break
    a.WalkEnd()
    after = a.tar_skip_stats()
    return files, {n: getattr(st, n) for n, _ in st._fields_}, {k: after[k] - before[k] for k in SKIP_KEYS}, calls


def _stats():
    from trivy_amd.analyzer.secret import DEVICE_TAR_STATS_SIZE_V1, _CDeviceTarStats
    st = _CDeviceTarStats()
    st.struct_size = DEVICE_TAR_STATS_SIZE_V1
    return st


def _index_records(a, layer):
    """Walk mode 0's host half over the model's candidate records."""
    from trivy_amd.analyzer.secret import DeviceTarIndex
    cands = tm.candidates(layer)
    recs = tm.records(cands)
    buf = np.frombuffer(layer, dtype=np.uint8)
    st, h = _stats(), c.c_void_p()
    rc = a._L.tsg_debug_index_tar_records(a._h, buf.ctypes.data, len(layer), recs.ctypes.data, len(cands), c.byref(h),
                                          c.byref(st))
    assert rc == 0, _err(a)
    return DeviceTarIndex(a, h, None, st.to_dict())


def _index_entries(a, layer):
    """Walk mode 1's host half over the model's entry records."""
    from trivy_amd.analyzer.secret import DeviceTarIndex
    entries, stop, n_cand = cm.chain(layer)
    assert stop[0] == cm.END, stop
    recs, names = cm.pack(entries)
    stop_a = np.array(stop, dtype=np.uint64)
    st, h = _stats(), c.c_void_p()
    rc = a._L.tsg_debug_index_tar_entries(a._h, recs.ctypes.data, len(entries), names.ctypes.data, len(names),
                                          stop_a.ctypes.data, len(layer), n_cand, c.byref(h), c.byref(st))
    assert rc == 0, _err(a)
    return DeviceTarIndex(a, h, None, st.to_dict())


def _check_all_walks(a, oracle, layer, skip_dirs, skip_files):
    """Host walk (copy, gather, host transform) and both index halves against the model; returns the model."""
    m, index = _want(oracle, layer, skip_dirs, skip_files)
    _set(a, skip_dirs, skip_files)
    try:
        for kw in ({}, {"gather": True}, {"gpu_transform": False}):
            files, st, sk, _ = _host_walk(a, layer, **kw)
            assert files == ["/" + fp for fp, _ in index], kw
            assert (st["regular"], st["whiteouts"], st["opaque_dirs"]) == (m["regular"], m["whiteouts"], m["opaque_dirs"])
            assert st["required"] == st["added"] == len(index)
            assert sk == _model_skip(m), kw
        for ix in (_index_records(a, layer), _index_entries(a, layer)):
            assert [(p, s) for p, _, s in ix.files()] == index
            for (_, off, size), (_, _, data) in zip(ix.files(), [k for k in m["kept"] if oracle.required(k[0], k[1])]):
                assert layer[off:off + size] == data
            assert ix.skip_stats == _model_skip(m)
            assert (ix.stats["regular"], ix.stats["whiteouts"], ix.stats["opaque_dirs"]) == \
                (m["regular"], m["whiteouts"], m["opaque_dirs"])
            assert ix.stats["required"] == len(index)
    finally:
        a.set_layer_walker(None)
    return m, index


# ---- the model is checked by itself first ---------------------------------------
def test_model_rel_table():
    """What follows from filepath.Rel for underSkippedDir, on the model's own Rel."""
    rel, under = sm.go_rel, sm.under_skipped_dir
    assert rel("a/b", "a/b/c") == "c" and under("a/b/c", ["a/b"])
    assert rel("a/b", "a/b") == "." and under("a/b", ["a/b"])
    assert rel("a/b", "a/bc") == "../bc" and not under("a/bc", ["a/b"])
    assert rel("a/b", "a") == ".." and under("a", ["a/b"])  # the direct parent is dropped
    assert rel("a/b/c", "a") == "../.." and not under("a", ["a/b/c"])
    assert rel(".", "x/y") == "x/y" and under("x/y", ["."]) and not under("../x", ["."])
    assert rel("../a", "b") is None and not under("b", ["../a", "b"])  # the failure ends the test
    assert under("b", ["b", "../a"])
    assert rel("", "x") == "x" and rel("/a", "b") is None


def test_fixture_layers_plant_a_finding_in_every_file(oracle):
    for name, (layer, sd, sf) in CASES.items():
        sm.check_planted(oracle, layer)
        m = sm.walk(layer, sd, sf)
        assert m["kept"] and m["dropped"], name
    sm.check_planted(oracle, sm.order_layer())


# ---- every case, every walk ------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_case_vs_model(an, oracle, name):
    layer, sd, sf = CASES[name]
    m, index = _check_all_walks(an, oracle, layer, sd, sf)
    kept = {fp for fp, _ in index}
    assert kept and m["dropped"] and not kept & set(m["dropped"])
    unfiltered = sm.walk(layer)
    assert (m["whiteouts"], m["opaque_dirs"]) == (unfiltered["whiteouts"], unfiltered["opaque_dirs"])
    if name == "before":
        assert "app/skipme/early.conf" in kept and "app/skipme/late.conf" in m["dropped"]
    if name == "sibling":
        assert "app/modules2/y.conf" in kept and "app/modulesz.conf" in kept and m["dropped"] == ["app/modules/x.conf"]
    if name == "skip-files":
        assert kept == {"srv/secret.env", "etc/app/secret.env.d/x.conf"} and m["skipped_files"] == 2
    if name == "markers":
        assert (m["whiteouts"], m["opaque_dirs"], len(m["skipped_dirs"])) == (2, 1, 1)
    if name == "malformed":
        assert m["skipped_dirs"] == ["a/skipme"] and kept == {"a/b.conf", "a/other[/c.conf"}
    if name == "parent":
        assert set(m["dropped"]) == {"a", "c/d", "a/b/x"} and kept == {"a2", "c", "a/bc"}
    if name == "rel-failure":
        assert m["skipped_dirs"] == ["../up", "b"] and m["dropped"] == ["../up/y.conf"] and "b/x.conf" in kept
    if name == "dot":
        assert kept == {"first.conf", "../out.conf"} and m["under_skipped_dir"] == 2


def test_no_options_and_clearing(an, oracle):
    """Without options nothing is dropped, and clearing them restores that."""
    layer, sd, sf = CASES["after"]
    plain = _host_walk(an, layer)
    assert plain[2] == dict.fromkeys(SKIP_KEYS, 0) and len(plain[0]) == len(sm.walk(layer)["kept"])
    _set(an, sd, sf)
    assert len(_host_walk(an, layer)[0]) < len(plain[0])
    assert an.layer_walker() is not None
    _set(an, [], [])
    assert an.layer_walker() is None
    assert _host_walk(an, layer)[:3] == plain[:3]
    ix = _index_entries(an, layer)
    assert len(ix.files()) == len(plain[0]) and ix.skip_stats == dict.fromkeys(SKIP_KEYS, 0)


# ---- order dependence across the units the walks index in parallel ---------------
def test_dir_and_files_in_different_chunks(an, oracle):
    """About 200 tiny entries: the skipped directory's entry and its later files lie in different 64-entry
    chunks of the entry-record half, and one of its files precedes it."""
    layer = sm.order_layer()
    entries, _, _ = cm.chain(layer)
    names = [e["name"].decode() for e in entries]
    at = names.index("z/skipme/")
    late = [i for i, n in enumerate(names) if n.startswith("z/skipme/late-")]
    assert 180 <= len(entries) <= 220 and at // 64 == 0 and {i // 64 for i in late} == {1, 2, 3}
    m, index = _check_all_walks(an, oracle, layer, ["**/skipme"], [])
    assert ("z/skipme/early.conf", len(sm.content("z/skipme/early.conf"))) in index
    assert m["under_skipped_dir"] == len(late) == 22 and len(index) == len(entries) - 1 - len(late)


def test_resumed_across_add_tar_calls_with_a_tiny_arena(an, oracle):
    """One file a batch: the list of skipped directories goes on from call to call."""
    layer = sm.order_layer()
    m, index = _want(oracle, layer, ["**/skipme"], [])
    _set(an, ["**/skipme"], [])
    try:
        for kw in ({}, {"gather": True}):
            files, st, sk, calls = _host_walk(an, layer, arena_bytes=64, **kw)
            assert calls >= len(index) and files == ["/" + fp for fp, _ in index]
            assert sk == _model_skip(m) and st["required"] == len(index) and st["regular"] == m["regular"]
    finally:
        an.set_layer_walker(None)


def test_resumed_inside_a_window_by_another_kind_of_collector(an, oracle):
    """Two collectors of one analyzer that do not share cached entries (one packs transformed bytes, one the
    bytes as read) fill in turn: every call indexes again from a cursor inside what the walk has read, and
    the list is cut back to what was recorded before that cursor."""
    from trivy_amd.analyzer.secret import Collector
    layer = sm.order_layer()
    m, index = _want(oracle, layer, ["**/skipme"], [])
    _set(an, ["**/skipme"], [])
    try:
        colls = [Collector(an, 2048, True), Collector(an, 2048, False)]
        files, st, sk, calls = _host_walk(an, layer, colls=colls)
        assert calls >= 6 and files == ["/" + fp for fp, _ in index]
        assert sk == _model_skip(m) and st["required"] == len(index)
    finally:
        an.set_layer_walker(None)


def test_setter_ends_the_walk_and_a_foreign_cursor_starts_an_empty_list(an, oracle):
    from trivy_amd.analyzer.secret import Collector, _CTarStats
    layer = sm.order_layer()
    buf = np.frombuffer(layer, dtype=np.uint8)
    entries, _, _ = cm.chain(layer)
    names = [e["name"].decode() for e in entries]
    after_dir = entries[names.index("z/skipme/") + 3]["start"]  # a cursor past the directory's entry
    _set(an, ["**/skipme"], [])
    try:
        coll = Collector(an, 64, True)
        st, cur, got = _CTarStats(), 0, []
        while cur < after_dir:
            rc, cur = coll.add_tar(buf, cur, st)
            assert rc == 1
            got += coll.paths()
            coll.reset()
        assert an.tar_skip_stats()["skipped_dirs"] == 1
        _set(an, ["**/skipme"], [])  # the same options again: the walk in progress ends, the counts restart
        assert an.tar_skip_stats() == dict.fromkeys(SKIP_KEYS, 0)
        big = Collector(an, 1 << 20, True)
        rc, end = big.add_tar(buf, cur, st)  # the cursor continues no walk: the directory is not on the list
        assert rc == 0
        rest = big.paths()
        late = [p for p in rest if p.startswith("/z/skipme/late-")]
        assert len(late) == 22 and an.tar_skip_stats() == dict.fromkeys(SKIP_KEYS, 0)
        an.WalkEnd()
        big.reset()
        # the same without the setter in between: the cursor continues the walk, the files stay dropped
        st, cur = _CTarStats(), 0
        while cur < after_dir:
            rc, cur = coll.add_tar(buf, cur, st)
            coll.reset()
        rc, end = big.add_tar(buf, cur, st)
        assert rc == 0 and not [p for p in big.paths() if p.startswith("/z/skipme/late-")]
        assert an.tar_skip_stats() == {"skipped_dirs": 1, "skipped_files": 0, "under_skipped_dir": 22}
        # and walk_end in between ends it as the setter does
        big.reset()
        st, cur = _CTarStats(), 0
        while cur < after_dir:
            rc, cur = coll.add_tar(buf, cur, st)
            coll.reset()
        an.WalkEnd()
        rc, end = big.add_tar(buf, cur, st)
        assert rc == 0 and len([p for p in big.paths() if p.startswith("/z/skipme/late-")]) == 22
    finally:
        an.WalkEnd()
        an.set_layer_walker(None)


_WINDOW_SCRIPT = r"""
import json, sys
sys.path.insert(0, %(root)r)
from tests import test_layer_skip_host as t
from tests import tar_skip_model as sm
a = t._new_analyzer()
layer = sm.window_layer()
out = {}
for ahead in (1, 0):
    assert a._L.tsg_analyzer_set_walk_ahead(a._h, ahead) == 0
    t._set(a, ["**/skipme"], ["**/2.log"])
    for arena in (1 << 20, 300 << 10):
        files, st, sk, calls = t._host_walk(a, layer, arena_bytes=arena)
        out["%%d-%%d" %% (ahead, arena)] = [files, st, sk, calls]
    a.set_layer_walker(None)
print(json.dumps(out))
"""


def test_dir_and_files_in_different_windows_and_walk_ahead(oracle):
    """A 1-MiB window (TSG_WALK_AHEAD=0, read once per process: a child) over a 1.6-MB layer: the directory's
    entry and its later files are indexed in different windows, with the next window indexed on the
    background thread (walk-ahead on) and without."""
    layer = sm.window_layer()
    m, index = _want(oracle, layer, ["**/skipme"], ["**/2.log"])
    assert m["under_skipped_dir"] == 3 and m["skipped_files"] == 1 and len(index) == 5
    env = dict(os.environ, TSG_WALK_AHEAD="0", TSG_WALK_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", _WINDOW_SCRIPT % {"root": str(ROOT)}], cwd=str(ROOT), env=env, check=True,
                       capture_output=True, text=True)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    windows = sum(1 for ln in r.stderr.splitlines() if ln.startswith("index: segs"))
    assert windows >= 2 * 4  # two windows or more per walk
    assert len(out) == 4
    for key, (files, st, sk, calls) in out.items():
        assert files == ["/" + fp for fp, _ in index], key
        assert sk == _model_skip(m) and st["required"] == len(index) and st["regular"] == m["regular"], key


def test_random_layers_vs_model(an, oracle):
    """Small random layers over a few path elements, "." and ".." among them, with random patterns: the three
    walks against the model (the index alone: these files carry no secret)."""
    rng = random.Random(20241220)
    elems = ["a", "b", "c", "ab", "..", "."]
    pats = ["a", "b", "a/b", "**/b", "*/c", "..", "../a", ".", "**", "a/**", "[", "{a,b}/c", "**/ab", "c"]
    totals = dict.fromkeys(SKIP_KEYS, 0)
    for _ in range(150):
        entries = []
        for _ in range(rng.randint(5, 20)):
            name = "/".join(rng.choice(elems) for _ in range(rng.randint(1, 4)))
            kind = rng.choice(["d", "d", "f", "f", "f", "l"])
            if oan.go_path_clean(name).lstrip("/") in ("", ".") and kind != "d":
                continue  # (the corner the reference leaves open: "." against another directory)
            entries.append((kind, name))
        layer = sm.build(entries)
        sd = [rng.choice(pats) for _ in range(rng.randint(1, 3))]
        sf = [rng.choice(pats) for _ in range(rng.randint(0, 2))]
        m, _ = _check_all_walks(an, oracle, layer, sd, sf)
        for k, v in _model_skip(m).items():
            totals[k] += v
    assert min(totals.values()) >= 50, totals  # (the model's counts: the layers do exercise every rule)


# ---- the interface ----------------------------------------------------------------
def test_argument_errors(an):
    from trivy_amd.analyzer.secret import TAR_SKIP_STATS_SIZE_V1, _CTarSkipStats
    L = an._L
    one = (c.c_char_p * 1)(b"a")
    null = (c.c_char_p * 1)(None)
    assert L.tsg_analyzer_set_tar_skip(None, one, 1, one, 1) == -1 and "NULL analyzer" in _err(an)
    assert L.tsg_analyzer_set_tar_skip(an._h, None, 1, one, 1) == -1 and "non-zero count" in _err(an)
    assert L.tsg_analyzer_set_tar_skip(an._h, one, 1, None, 2) == -1 and "non-zero count" in _err(an)
    assert L.tsg_analyzer_set_tar_skip(an._h, null, 1, one, 1) == -1 and "skip_dirs[0]" in _err(an)
    assert L.tsg_analyzer_set_tar_skip(an._h, one, 1, null, 1) == -1 and "skip_files[0]" in _err(an)
    nd, nf = c.c_uint32(9), c.c_uint32(9)
    assert L.tsg_analyzer_get_tar_skip(an._h, c.byref(nd), c.byref(nf)) == 0 and (nd.value, nf.value) == (0, 0)
    assert L.tsg_analyzer_set_tar_skip(an._h, one, 1, None, 0) == 0
    assert L.tsg_analyzer_get_tar_skip(an._h, c.byref(nd), c.byref(nf)) == 0 and (nd.value, nf.value) == (1, 0)
    assert L.tsg_analyzer_set_tar_skip(an._h, None, 0, None, 0) == 0
    assert L.tsg_analyzer_get_tar_skip(an._h, c.byref(nd), c.byref(nf)) == 0 and (nd.value, nf.value) == (0, 0)
    assert L.tsg_analyzer_get_tar_skip(None, c.byref(nd), c.byref(nf)) == -1
    assert L.tsg_analyzer_get_tar_skip(an._h, None, c.byref(nf)) == -1
    ix = _index_records(an, CASES["after"][0])
    st = _CTarSkipStats()
    for bogus in (0, 8, TAR_SKIP_STATS_SIZE_V1 - 8, TAR_SKIP_STATS_SIZE_V1 + 8):
        st.struct_size = bogus
        assert L.tsg_analyzer_tar_skip_stats(an._h, c.byref(st)) == -1 and "struct_size %d" % bogus in _err(an)
        assert L.tsg_tar_index_skip_stats(ix._h, c.byref(st)) == -1 and "struct_size %d" % bogus in _err(an)
    st.struct_size = TAR_SKIP_STATS_SIZE_V1
    assert L.tsg_analyzer_tar_skip_stats(None, c.byref(st)) == -1
    assert L.tsg_analyzer_tar_skip_stats(an._h, None) == -1
    assert L.tsg_tar_index_skip_stats(None, c.byref(st)) == -1
    assert L.tsg_tar_index_skip_stats(ix._h, None) == -1
    assert L.tsg_analyzer_tar_skip_stats(an._h, c.byref(st)) == 0
    assert L.tsg_tar_index_skip_stats(ix._h, c.byref(st)) == 0


def test_python_mirror(an):
    from trivy_amd.walker import LayerTar, NewLayerTar, Option
    w = NewLayerTar(Option(SkipFiles=["/etc//passwd", "./a/../b.txt"], SkipDirs=["usr/lib/", "", "/"]))
    assert w == LayerTar(skipFiles=["etc/passwd", "b.txt"], skipDirs=["usr/lib", ".", ""])
    an.set_layer_walker(w)
    try:
        nd, nf = c.c_uint32(), c.c_uint32()
        workers = an.LayerWorkers(parallel=2, arena_bytes=1 << 20)
        for sub, _ in workers:  # the workers' analyzers inherit the options
            assert sub.layer_walker() == w
            assert an._L.tsg_analyzer_get_tar_skip(sub._h, c.byref(nd), c.byref(nf)) == 0
            assert (nd.value, nf.value) == (3, 2)
    finally:
        an.set_layer_walker(None)
    assert an.layer_walker() is None


def test_struct_layout(tmp_path):
    from trivy_amd.analyzer.secret import TAR_SKIP_STATS_SIZE_V1, _CTarSkipStats
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "tsg_analyzer.h"\nint main(void){printf("%zu %u %zu %zu %zu\\n",'
                   ' sizeof(tsg_tar_skip_stats), (unsigned)TSG_TAR_SKIP_STATS_SIZE_V1,'
                   ' offsetof(tsg_tar_skip_stats, skipped_dirs), offsetof(tsg_tar_skip_stats, skipped_files),'
                   ' offsetof(tsg_tar_skip_stats, under_skipped_dir)); return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    size, v1, o_d, o_f, o_u = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True,
                                                              text=True).stdout.split()]
    assert size == v1 == c.sizeof(_CTarSkipStats) == TAR_SKIP_STATS_SIZE_V1 == 32
    assert o_d == _CTarSkipStats.skipped_dirs.offset == 8 and o_f == _CTarSkipStats.skipped_files.offset == 16
    assert o_u == _CTarSkipStats.under_skipped_dir.offset == 24
    # the structs that were there keep their layouts
    from trivy_amd.analyzer.secret import DEVICE_TAR_STATS_SIZE_V1, _CTarStats
    assert c.sizeof(_CTarStats) == 64 and DEVICE_TAR_STATS_SIZE_V1 == 8 + 64 + 6 * 8 + 16
