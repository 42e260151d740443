"""The GPU chain walk of a resident tar layer (tsg_analyzer_set_tar_walk), the parts that need no GPU.

* the pure-Python model of the GPU half (tests/tar_chain_model.py) gives, on every well-formed layer, the
  entries oracle/analyzer.py's walk_layer_tar walks -- the model is not its own yardstick;
* the host half (tsg_debug_index_tar_entries: clean, classify, Required and the index over the entry
  records, on the host pool) fed the model's records builds the index today's host half builds from the
  candidate records (tsg_debug_index_tar_records): files, spans, the five tar stats, off_chain;
* the setter's argument errors, TSG_TAR_WALK, the new struct's layout.
"""
import ctypes as c
import os
import subprocess
import sys
import tarfile
from pathlib import Path

import numpy as np
import pytest

from oracle import analyzer as oan
from oracle import hostlib
from tests import tar_chain_model as cm
from tests import tar_index_model as tm
from tests.layers import make_layer

ROOT = Path(__file__).resolve().parent.parent

LAYERS = {
    "gnu3": lambda: make_layer(3, 60, tarfile.GNU_FORMAT),
    "gnu7": lambda: make_layer(7, 60, tarfile.GNU_FORMAT),
    "pax3": lambda: make_layer(3, 60, tarfile.PAX_FORMAT),
    "pax7": lambda: make_layer(7, 60, tarfile.PAX_FORMAT),
    "ustar": cm.ustar_layer,
    "ustar-prefix": tm.ustar_prefix_layer,
    "odd-names": cm.odd_names_layer,
    "nested": tm.nested_layer,
    "pax-size": tm.pax_size_layer,
    "no-trailer": tm.no_trailer_layer,
    "empty": lambda: bytes(1024),
    "nothing": lambda: b"",
    "boundaries-8": lambda: cm.boundary_layer(8),
    "boundaries-64": lambda: cm.boundary_layer(64),
}
LAYERS.update({"case-" + k: (lambda v=v: v) for k, v in cm.complete_cases().items()})


@pytest.fixture(scope="module")
def an():
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
def oracle():
    return oan.SecretAnalyzer("")


def _err(a):
    from trivy_amd import _lib
    return _lib.last_error(a._L)


def _stats():
    from trivy_amd.analyzer.secret import DEVICE_TAR_STATS_SIZE_V1, _CDeviceTarStats
    st = _CDeviceTarStats()
    st.struct_size = DEVICE_TAR_STATS_SIZE_V1
    return st


def _index_records(a, layer: bytes):
    """Today's host half over the model's candidate records."""
    from trivy_amd.analyzer.secret import DeviceTarIndex
    cands = tm.candidates(layer)
    recs = tm.records(cands)
    buf = np.frombuffer(layer or b"\0", dtype=np.uint8)
    st, h = _stats(), c.c_void_p()
    rc = a._L.tsg_debug_index_tar_records(a._h, buf.ctypes.data, len(layer), recs.ctypes.data if len(recs) else None,
                                          len(cands), c.byref(h), c.byref(st))
    assert rc == 0, _err(a)
    return DeviceTarIndex(a, h, None, st.to_dict())


def _index_entries(a, layer: bytes):
    """The new host half over the model's entry records."""
    from trivy_amd.analyzer.secret import DeviceTarIndex
    entries, stop, n_cand = cm.chain(layer)
    assert stop[0] == cm.END, stop
    recs, names = cm.pack(entries)
    stop_a = np.array(stop, dtype=np.uint64)
    st, h = _stats(), c.c_void_p()
    rc = a._L.tsg_debug_index_tar_entries(a._h, recs.ctypes.data if len(recs) else None, len(entries),
                                          names.ctypes.data if len(names) else None, len(names), stop_a.ctypes.data,
                                          len(layer), n_cand, c.byref(h), c.byref(st))
    assert rc == 0, _err(a)
    return DeviceTarIndex(a, h, None, st.to_dict()), entries


def _model_walk(layer: bytes):
    """walk_layer_tar's result from the model's entries: the host half's rules, restated in Python."""
    entries, stop, _ = cm.chain(layer)
    assert stop[0] == cm.END
    files, wh, opq = [], 0, 0
    for e in entries:
        raw = e["name"].decode("utf-8", "surrogateescape")
        fp = oan.go_path_clean(raw).lstrip("/")
        fname = fp.rsplit("/", 1)[-1]
        if fname == ".wh..wh..opq":
            opq += 1
        elif fname.startswith(".wh."):
            wh += 1
        elif e["typeflag"] == 0x30 or (e["typeflag"] == 0 and not raw.endswith("/")):
            files.append((fp, e["size"], layer[e["data"]:e["data"] + e["size"]]))
    return files, wh, opq


# Python's tarfile, which the oracle walks with, reads some hand-built combinations differently from
# Go's archive/tar (several x headers before one entry, an x header before the end of the archive): for the
# "case-" layers the yardstick is today's host half alone.
@pytest.mark.parametrize("name", [n for n in LAYERS if n != "nothing" and not n.startswith("case-")])
def test_model_vs_oracle_walk(name):
    layer = LAYERS[name]()
    files, wh, opq = oan.walk_layer_tar(layer)
    assert _model_walk(layer) == (files, wh, opq)
    entries, stop, n_cand = cm.chain(layer)
    with tarfile.open(fileobj=__import__("io").BytesIO(layer), mode="r:") as tf:
        assert len(entries) == (len(tf.getmembers()) if any(layer) else 0)
    if name in ("gnu3", "gnu7"):
        assert 6 <= sum(e["flags"] == cm.NAME_LONG for e in entries) <= 43
    if name in ("pax3", "pax7"):
        assert 6 <= sum(e["flags"] == cm.NAME_PAX for e in entries) <= 43
    if name in ("ustar", "ustar-prefix"):
        assert any(b"/" in e["name"] and len(e["name"]) > 100 for e in entries) and all(e["n_ext"] == 0 for e in entries)


@pytest.mark.parametrize("name", list(LAYERS))
def test_host_half_vs_records_walk_and_oracle(an, oracle, name):
    layer = LAYERS[name]()
    want = _index_records(an, layer)
    got, entries = _index_entries(an, layer)
    assert got.files() == want.files()
    assert got.start.tolist() == want.start.tolist() and got.data_off.tolist() == want.data_off.tolist()
    assert got.size.tolist() == want.size.tolist()
    for k in ("entries", "regular", "required", "whiteouts", "opaque_dirs", "blocks", "candidates", "off_chain"):
        assert got.stats[k] == want.stats[k], k
    assert got.stats["block_fetches"] == 0 and got.stats["ext_bytes"] == 0 and got.stats["kernel_runs"] == 0
    ws = got.walk_stats
    assert ws["walk"] == "gpu" and ws["fallback"] == 0 and ws["chain_entries"] == len(entries)
    assert want.walk_stats["walk"] == "host" and want.walk_stats["chain_entries"] == 0
    if layer and not name.startswith("case-"):
        files, wh, opq = oan.walk_layer_tar(layer)
        req = [(fp, size, content) for fp, size, content in files if oracle.required(fp, size)]
        assert [(p, s) for p, _, s in got.files()] == [(fp, size) for fp, size, _ in req]
        for (_, off, size), (_, _, content) in zip(got.files(), req):
            assert layer[off:off + size] == content
        assert (got.stats["whiteouts"], got.stats["opaque_dirs"], got.stats["regular"]) == (wh, opq, len(files))
    if name == "odd-names":
        assert got.stats["whiteouts"] == 2 and got.stats["opaque_dirs"] == 1
        assert [p for p, _, _ in got.files()] == ["a/c.conf", "abs/path.conf", "two/slashes.conf", "../up.conf", "a/b",
                                                  "old/rega.conf", "tail.conf"]


@pytest.mark.parametrize("name", list(cm.punt_cases()))
def test_punts_are_what_the_host_walk_rejects_or_the_device_leaves_to_it(an, name):
    """The model stops INCOMPLETE; today's host half, which such a layer falls back to, fails on the
    malformed ones with its own message and indexes the ones only the device does not decide."""
    layer, reason, at = cm.punt_cases()[name]
    entries, stop, _ = cm.chain(layer)
    assert stop[:3] == (cm.INCOMPLETE, reason, at)
    cands = tm.candidates(layer)
    recs = tm.records(cands)
    buf = np.frombuffer(layer, dtype=np.uint8)
    h = c.c_void_p()
    rc = an._L.tsg_debug_index_tar_records(an._h, buf.ctypes.data, len(layer), recs.ctypes.data, len(cands), c.byref(h),
                                           None)
    if reason in (cm.CAP, cm.PAX_SIZE_FORM):
        assert rc == 0, _err(an)
        from trivy_amd.analyzer.secret import DeviceTarIndex
        ix = DeviceTarIndex(an, h, None, {})
        assert [p for p, _, _ in ix.files()][:2] == ["first", "second"] and ix.n >= 3
    else:
        assert rc == -3 and _err(an).startswith("tar: ")


def test_host_half_refuses_what_is_not_a_finished_walk(an):
    entries, stop, n_cand = cm.chain(make_layer(3, 20))
    recs, names = cm.pack(entries)
    h = c.c_void_p()

    def call(recs_a, n, names_n, stop_t, st=None):
        stop_a = np.array(stop_t, dtype=np.uint64)
        return an._L.tsg_debug_index_tar_entries(an._h, recs_a.ctypes.data, n, names.ctypes.data, names_n,
                                                 stop_a.ctypes.data, 1 << 20, n_cand, c.byref(h), st)

    assert call(recs, len(entries), len(names), (cm.INCOMPLETE, cm.BAD_PAX, 512, 0)) == -1 and "END" in _err(an)
    assert call(recs, len(entries), len(names) - 1, stop) == -1 and "outside the name blob" in _err(an)
    assert not h.value
    from trivy_amd.analyzer.secret import _CDeviceTarStats
    st = _CDeviceTarStats()
    st.struct_size = 8
    assert call(recs, len(entries), len(names), stop, c.byref(st)) == -1 and "struct_size" in _err(an)
    assert an._L.tsg_debug_index_tar_entries(None, None, 0, None, 0, None, 0, 0, c.byref(h), None) == -1


def test_setter_and_getter(an):
    L = an._L
    assert an.tar_walk() == "host"  # the default
    an.set_tar_walk("gpu")
    assert an.tar_walk() == "gpu"
    for bad in (2, 3, -1, 1 << 20):
        assert L.tsg_analyzer_set_tar_walk(an._h, bad) == -1
        assert "mode %d" % bad in _err(an)
        assert an.tar_walk() == "gpu"  # unchanged
    an.set_tar_walk("host")
    assert an.tar_walk() == "host"
    with pytest.raises(ValueError):
        an.set_tar_walk("device")
    m = c.c_int(9)
    assert L.tsg_analyzer_set_tar_walk(None, 1) == -1
    assert L.tsg_analyzer_get_tar_walk(None, c.byref(m)) == -1 and m.value == 9
    assert L.tsg_analyzer_get_tar_walk(an._h, None) == -1


def test_walk_stats_argument_errors(an):
    from trivy_amd.analyzer.secret import TAR_WALK_STATS_SIZE_V1, _CTarWalkStats
    ix = _index_records(an, make_layer(3, 20))
    ws = _CTarWalkStats()
    for bogus in (0, 8, TAR_WALK_STATS_SIZE_V1 - 8, TAR_WALK_STATS_SIZE_V1 + 8):
        ws.struct_size = bogus
        assert an._L.tsg_tar_index_walk_stats(ix._h, c.byref(ws)) == -1 and "struct_size %d" % bogus in _err(an)
    ws.struct_size = TAR_WALK_STATS_SIZE_V1
    assert an._L.tsg_tar_index_walk_stats(None, c.byref(ws)) == -1
    assert an._L.tsg_tar_index_walk_stats(ix._h, None) == -1
    assert an._L.tsg_tar_index_walk_stats(ix._h, c.byref(ws)) == 0 and ws.walk == 0 and ws.fallback == 0


def test_env_sets_the_initial_mode():
    """TSG_TAR_WALK is read when an analyzer is made: in a child process, so this one's environment stays."""
    code = ("from oracle import hostlib\n"
            "from trivy_amd.analyzer import AnalyzerOptions, SecretAnalyzer\n"
            "a = SecretAnalyzer(lib=hostlib.lib(), host_only=True)\n"
            "a.Init(AnalyzerOptions())\n"
            "print(a.tar_walk())\n")
    for value, want in (("gpu", "gpu"), ("host", "host"), ("GPU", "host"), ("", "host"), (None, "host")):
        env = dict(os.environ)
        env.pop("TSG_TAR_WALK", None)
        if value is not None:
            env["TSG_TAR_WALK"] = value
        out = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), env=env, check=True, capture_output=True,
                             text=True).stdout.split()
        assert out[-1] == want, (value, out)


def test_struct_layout(tmp_path):
    from trivy_amd.analyzer.secret import TAR_WALK_STATS_SIZE_V1, _CTarWalkStats
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "tsg_analyzer.h"\nint main(void){printf("%zu %u %zu %zu %zu %zu %zu\\n",'
                   ' sizeof(tsg_tar_walk_stats), (unsigned)TSG_TAR_WALK_STATS_SIZE_V1, offsetof(tsg_tar_walk_stats, walk),'
                   ' offsetof(tsg_tar_walk_stats, fallback), offsetof(tsg_tar_walk_stats, chain_entries),'
                   ' offsetof(tsg_tar_walk_stats, device_bytes), offsetof(tsg_tar_walk_stats, ms_candidates));'
                   ' return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    size, v1, o_walk, o_fb, o_ce, o_db, o_ms = \
        [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert size == v1 == c.sizeof(_CTarWalkStats) == TAR_WALK_STATS_SIZE_V1 == 16 + 4 * 8 + 6 * 8
    assert o_walk == _CTarWalkStats.walk.offset == 8 and o_fb == _CTarWalkStats.fallback.offset == 12
    assert o_ce == _CTarWalkStats.chain_entries.offset == 16 and o_db == _CTarWalkStats.device_bytes.offset == 40
    assert o_ms == _CTarWalkStats.ms_candidates.offset == 48
