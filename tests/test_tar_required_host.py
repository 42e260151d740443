"""Path classify and Required of a resident tar layer on the GPU (tsg_analyzer_set_tar_required), the parts
that need no GPU.

* the pure-Python model of the device stage (tests/tar_required_model.py) gives, for a table of names, the
  verdict written beside each name -- the model is not its own yardstick;
* the host half behind the stage (tsg_debug_index_tar_files) fed the model's output builds the index and the
  stats mode 1's host half (tsg_debug_index_tar_entries) builds from the entry records, and what
  oracle/analyzer.py walks and requires, with the builtin rules and with an allow rule that has no literal;
* the setter, TSG_TAR_REQUIRED, the new struct's layout, argument errors.
"""
import ctypes as c
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

ROOT = Path(__file__).resolve().parent.parent
TEXT = cm.TEXT  # 61 bytes
CONFIG_BASE = "trivy-secret.yaml"

# (raw name, typeflag, content size or None for TEXT, the verdict with the builtin rules, the indexed path or
# None when the file is not in the index).  With the no-literal config every KEEP is ASK_ALLOW for all rules.
K, D, A, N, O, W, Q = rm.KEEP, rm.DROP, rm.ASK_ALLOW, rm.ASK_NAME, rm.OTHER, rm.WHITEOUT, rm.OPAQUE
SURE_4096 = b"example/" + b"a/" * 2043 + b"ab"
SURE_4097 = b"example/" + b"a/" * 2043 + b"abc"
NAME_TABLE = [
    # skip dirs
    (b".git/config", b"0", None, D, None), (b"a/.git/x", b"0", None, D, None), (b".gitx/y", b"0", None, K, ".gitx/y"),
    (b"x.git/y", b"0", None, K, "x.git/y"), (b"a/node_modules/b", b"0", None, D, None),
    (b"node_modules", b"0", None, K, "node_modules"), (b"a/.git", b"0", None, K, "a/.git"),
    (b"node_modules/x", b"0", None, D, None), (b"a/node_modulesx/b", b"0", None, K, "a/node_modulesx/b"),
    # skip files
    (b"go.mod", b"0", None, D, None), (b"a/go.mod", b"0", None, D, None), (b"go.modx", b"0", None, K, "go.modx"),
    (b"xgo.mod", b"0", None, K, "xgo.mod"), (b"package-lock.json", b"0", None, D, None),
    (b"d/Gemfile.lock", b"0", None, D, None), (b"go.mod/x", b"0", None, K, "go.mod/x"),
    # extensions
    (b"a.jpg", b"0", None, D, None), (b"a.JPG", b"0", None, K, "a.JPG"), (b"a.socket", b"0", None, D, None),
    (b"a.sockets", b"0", None, K, "a.sockets"), (b".gz", b"0", None, D, None), (b"a.tar.gz", b"0", None, D, None),
    (b"a.", b"0", None, K, "a."), (b"a.b/c", b"0", None, K, "a.b/c"), (b"a.jpg/c", b"0", None, K, "a.jpg/c"),
    (b"a.tar", b"0", None, D, None), (b"a.gzip", b"0", None, D, None), (b"a.jpgx", b"0", None, K, "a.jpgx"),
    # sizes
    (b"size9", b"0", 9, D, None), (b"size10", b"0", 10, K, "size10"), (b"size0", b"0", 0, D, None),
    # markers
    (b".wh.x", b"0", None, W, None), (b"d/.wh.x", b"0", None, W, None), (b".wh.", b"0", None, W, None),
    (b"x.wh.y", b"0", None, K, "x.wh.y"), (b".wh..wh..opq", b"0", None, Q, None),
    (b"d/.wh..wh..opq", b"0", None, Q, None), (b"l/.wh.x", b"2", 0, W, None), (b"e/.wh.x", b"5", 0, W, None),
    (b".wh.x/", b"5", 0, W, None), (b".wh./f", b"0", None, K, ".wh./f"), (b".wh..wh..opqx", b"0", None, W, None),
    # decided forms
    (b"./a", b"0", None, K, "a"), (b"/a", b"0", None, K, "a"), (b"a/", b"0", None, K, "a"), (b"./a/", b"0", None, K, "a"),
    (b"./a/b//", b"0", None, K, "a/b"), (b"/.a", b"0", None, K, ".a"), (b"...", b"0", None, K, "..."),
    (b"..a/b..", b"0", None, K, "..a/b.."),
    # typeflags
    (b"rega", b"\0", None, K, "rega"), (b"regadir/", b"\0", 0, O, None), (b"reg0/", b"0", None, K, "reg0"),
    (b"dir5", b"5", 0, O, None), (b"dir5/", b"5", 0, O, None), (b"link", b"2", 0, O, None),
    (b"hard", b"1", 0, O, None), (b"seven", b"7", None, O, None),
    # names the device does not clean
    (b"", b"0", None, N, "."), (b".", b"0", None, N, "."), (b"./", b"5", 0, N, None), (b"/", b"5", 0, N, None),
    (b"//a", b"0", None, N, "a"), (b".//a", b"0", None, N, "a"), (b"a//b", b"0", None, N, "a/b"),
    (b"a/./b", b"0", None, N, "a/b"), (b"a/../b", b"0", None, N, "b"), (b"../a", b"0", None, N, "../a"),
    (b"/../a", b"0", None, N, "a"), (b"a/..", b"0", None, N, "."), (b"a/.", b"0", None, N, "a"),
    (b"..", b"0", None, N, ".."), (b"././a", b"0", None, N, "a"), (b"d/../.wh.x", b"0", None, N, None),
    (b"x/../a.jpg", b"0", None, N, None), (b"a/./", b"\0", 0, N, None),
    # the allow paths
    (b"docs/example/cfg", b"0", None, D, None), (SURE_4096, b"0", None, D, None), (SURE_4097, b"0", None, A, None),
    (b"a/README.md", b"0", None, D, None), (b"a/README.md5", b"0", None, A, "a/README.md5"),
    (b"x/opt/yarn-v1/f.conf", b"0", None, A, "x/opt/yarn-v1/f.conf"), (b"usr/share/f", b"0", None, D, None),
    (b"a/usr/share/f", b"0", None, A, "a/usr/share/f"), (b"EXAMPLE.conf", b"0", None, A, "EXAMPLE.conf"),
    (b"caf\xc3\xa9/conf", b"0", None, A, "caf\u00e9/conf"), (b"\xff\xfe.md", b"0", None, A, None),
    # the config base: the whole path, as the host compares it
    (CONFIG_BASE.encode(), b"0", None, D, None), (b"etc/" + CONFIG_BASE.encode(), b"0", None, K, "etc/" + CONFIG_BASE),
    (b"./" + CONFIG_BASE.encode() + b"/", b"0", None, D, None),
]


def table_layer() -> bytes:
    out = b""
    for name, typeflag, size, _, _ in NAME_TABLE:
        body = TEXT if size is None else (TEXT * 2)[:size]
        if len(name) > 100 or name in (b"", b"."):  # (tarfile-free: a PAX path carries what the name field cannot)
            out += cm.xhdr(b"path=" + name) + cm.member(b"pax-name", body, typeflag)
        else:
            out += cm.member(name, body, typeflag, magic=bytes(8))
    return out + cm.TRAILER


LAYERS = {
    "ustar": cm.ustar_layer,
    "odd-names": cm.odd_names_layer,
    "boundaries-8": lambda: cm.boundary_layer(8),
    "table": table_layer,
}
LAYERS.update({"case-" + k: (lambda v=v: v) for k, v in cm.complete_cases().items()})


def _declare(L):
    L.tsg_debug_index_tar_entries.argtypes = [c.c_void_p, c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint64, c.c_void_p,
                                              c.c_uint64, c.c_uint64, c.POINTER(c.c_void_p), c.c_void_p]
    L.tsg_debug_index_tar_files.argtypes = [c.c_void_p, c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint64, c.c_void_p,
                                            c.c_void_p, c.c_uint64, c.c_uint64, c.POINTER(c.c_void_p), c.c_void_p]


def _analyzer(config_path=""):
    from trivy_amd.analyzer import AnalyzerOptions, SecretAnalyzer, SecretScannerOption
    a = SecretAnalyzer(lib=hostlib.lib(), host_only=True)
    a.Init(AnalyzerOptions(SecretScannerOption(ConfigPath=config_path)))
    _declare(a._L)
    return a


@pytest.fixture(scope="module")
def cfg_dir(tmp_path_factory):
    """Two configs named CONFIG_BASE: one without rules of its own, one whose allow rule has no literal."""
    d = tmp_path_factory.mktemp("cfg")
    (d / "builtin").mkdir()
    (d / "noliteral").mkdir()
    (d / "builtin" / CONFIG_BASE).write_text("disable-rules: []\n")
    (d / "noliteral" / CONFIG_BASE).write_text(
        "allow-rules:\n  - id: no-literal\n    description: d\n    path: '^[a-c]+/[0-9]'\n")
    return d


@pytest.fixture(scope="module", params=["builtin", "noliteral"])
def setup(request, cfg_dir):
    path = str(cfg_dir / request.param / CONFIG_BASE)
    an = _analyzer(path)
    pt, st = rm.tables_of(an)
    assert (pt is not None) == (request.param == "builtin") and (st is not None) == (request.param == "builtin")
    return request.param, an, oan.SecretAnalyzer(path), pt, st


def _err(a):
    from trivy_amd import _lib
    return _lib.last_error(a._L)


def _stats():
    from trivy_amd.analyzer.secret import DEVICE_TAR_STATS_SIZE_V1, _CDeviceTarStats
    st = _CDeviceTarStats()
    st.struct_size = DEVICE_TAR_STATS_SIZE_V1
    return st


def _ptr(a):
    return a.ctypes.data if len(a) else None


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
    assert rc == want_rc, _err(a)
    return DeviceTarIndex(a, h, None, st.to_dict()) if rc == 0 else None


def _model(entries, cfg: bytes, pt, st):
    recs, names = cm.pack(entries)
    return rm.stage(recs, len(entries), bytes(names), [0, len(entries)], [0, len(names)], cfg, pt, st)


def _pool(ix):
    """The index's path pool, read through the first file's pointer: every path and its NUL, in order."""
    if ix.n == 0:
        return b""
    pp, pl = c.c_void_p(), c.c_uint64()
    assert ix._an._L.tsg_tar_index_file(ix._h, 0, c.byref(pp), c.byref(pl), None, None) == 0
    total = sum(len(p.encode("utf-8", "surrogateescape")) + 1 for p, _, _ in ix.files())
    return c.string_at(pp, total)


def test_the_table_has_the_verdict_beside_each_name(setup):
    kind, an, oracle, pt, st = setup
    for name, typeflag, size, want, path in NAME_TABLE:
        size = len(TEXT) if size is None else size
        v, skip, out_len, rules, all_rules = rm.decide(name, typeflag[0], size, CONFIG_BASE.encode(), pt, st)
        if kind == "noliteral" and want in (K, A):
            assert (v, all_rules) == (A, 1), name[:40]
        elif kind == "noliteral" and want == D and v == A:  # dropped by a builtin allow path: this config has none
            assert all_rules == 1
        else:
            assert v == want, (name[:40], v, want)
        if v in (K, A):
            assert name[skip:skip + out_len] == oan.go_path_clean(name.decode("utf-8", "surrogateescape")).lstrip(
                "/").encode("utf-8", "surrogateescape"), name[:40]
        if v == A and not all_rules:
            assert rules != 0
        # the verdict against the oracle, entry by entry
        raw = name.decode("utf-8", "surrogateescape")
        fp = oan.go_path_clean(raw).lstrip("/")
        base = fp.rsplit("/", 1)[-1]
        marker = base.startswith(".wh.")
        regular = not marker and (typeflag == b"0" or (typeflag == b"\0" and not raw.endswith("/")))
        indexed = regular and oracle.required(fp, size)
        if kind == "builtin":
            assert indexed == (path is not None), name[:40]
            if indexed:
                assert fp == path
        if v == K:
            assert indexed
        if v in (D, O, W, Q):
            assert not indexed
        if v == W:
            assert marker and base != ".wh..wh..opq"
        if v == Q:
            assert base == ".wh..wh..opq"


@pytest.mark.parametrize("name", list(LAYERS))
def test_model_through_the_host_half_equals_mode_1_and_the_oracle(setup, name):
    kind, an, oracle, pt, st = setup
    layer = LAYERS[name]()
    entries, stop, n_cand = cm.chain(layer)
    assert stop[0] == cm.END, stop
    if name == "table":
        assert [e["name"] for e in entries] == [t[0] for t in NAME_TABLE]
    want = _index_entries(an, entries, stop, n_cand, len(layer))
    verdicts, frecs, blob, counts = _model(entries, CONFIG_BASE.encode(), pt, st)
    got = _index_files(an, frecs, blob, counts[0], stop, n_cand, len(layer))
    assert got.files() == want.files() and _pool(got) == _pool(want)
    assert got.start.tolist() == want.start.tolist() and got.data_off.tolist() == want.data_off.tolist()
    assert got.size.tolist() == want.size.tolist()
    for k in ("entries", "regular", "required", "whiteouts", "opaque_dirs", "blocks", "candidates", "off_chain",
              "block_fetches", "ext_bytes", "kernel_runs"):
        assert got.stats[k] == want.stats[k], k
    rs = got.required_stats
    assert rs["mode"] == "gpu" and rs["reason"] == 0 and rs["entries"] == len(entries)
    assert (rs["kept"], rs["dropped"], rs["ask_allow"], rs["ask_name"]) == tuple(
        int((verdicts == v).sum()) for v in (K, D, A, N))
    assert rs["kept"] + rs["ask_allow"] + rs["ask_name"] - rs["ask_dropped"] == got.n
    assert rs["path_bytes"] == len(blob)
    assert want.required_stats["mode"] == "host" and want.required_stats["reason"] == 1
    if rs["ask_name"] == 0 and rs["ask_dropped"] == 0:  # the blob is the pool as it stands
        assert _pool(got) == blob
    # the oracle: its walk where Python's tarfile reads the layer as Go does, else its path rules over the entries
    if name.startswith("case-"):
        return
    if name == "table":
        files = []
        for e in entries:
            raw = e["name"].decode("utf-8", "surrogateescape")
            fp = oan.go_path_clean(raw).lstrip("/")
            if not fp.rsplit("/", 1)[-1].startswith(".wh.") and (
                    e["typeflag"] == 0x30 or (e["typeflag"] == 0 and not raw.endswith("/"))):
                files.append((fp, e["size"]))
    else:
        files = [(fp, size) for fp, size, _ in oan.walk_layer_tar(layer)[0]]
    assert [(p, s) for p, _, s in got.files()] == [(fp, size) for fp, size in files if oracle.required(fp, size)]
    assert got.stats["regular"] == len(files)
    if name == "table" and kind == "builtin":
        assert [p for p, _, _ in got.files()] == [t[4] for t in NAME_TABLE if t[4] is not None]


def test_ustar_layer_asks_about_no_name():
    an = _analyzer()
    pt, st = rm.tables_of(an)
    assert pt is not None and st is not None
    entries, stop, _ = cm.chain(cm.ustar_layer())
    verdicts, frecs, blob, counts = _model(entries, b".", pt, st)
    assert int(counts[0][rm.COUNTS.index("ask_name")]) == 0 and not (verdicts == N).any()
    assert int(counts[0][rm.COUNTS.index("kept")]) == 12


def test_host_half_refuses_records_that_contradict_the_blob_or_the_counts():
    an = _analyzer()
    pt, st = rm.tables_of(an)
    layer = cm.odd_names_layer()
    entries, stop, n_cand = cm.chain(layer)
    verdicts, frecs, blob, counts = _model(entries, b".", pt, st)
    assert _index_files(an, frecs, blob, counts[0], stop, n_cand, len(layer)) is not None
    assert _index_files(an, frecs, blob[:-1], counts[0], stop, n_cand, len(layer), want_rc=-1) is None
    assert "counts" in _err(an)
    short = counts[0].copy()
    short[rm.COUNTS.index("path_bytes")] -= 1  # the last record's NUL is now outside the blob
    assert _index_files(an, frecs, blob[:-1], short, stop, n_cand, len(layer), want_rc=-1) is None
    assert "outside the path blob" in _err(an)
    bad = bytearray(frecs)
    bad[37] = rm.DROP  # a verdict that has no record
    assert _index_files(an, bytes(bad), blob, counts[0], stop, n_cand, len(layer), want_rc=-1) is None
    flagged = counts[0].copy()
    flagged[rm.COUNTS.index("bad")] = 1
    assert _index_files(an, frecs, blob, flagged, stop, n_cand, len(layer), want_rc=-1) is None
    assert _index_files(an, frecs, blob, counts[0], (cm.INCOMPLETE, cm.BAD_PAX, 512, 0), n_cand, len(layer),
                        want_rc=-1) is None and "END" in _err(an)
    h = c.c_void_p()
    assert an._L.tsg_debug_index_tar_files(None, None, 0, None, 0, None, None, 0, 0, c.byref(h), None) == -1


def test_setter_and_getter():
    an = _analyzer()
    L = an._L
    assert an.tar_required() == "host"  # the default
    an.set_tar_required("gpu")
    assert an.tar_required() == "gpu"
    for bad in (2, 3, -1, 1 << 20):
        assert L.tsg_analyzer_set_tar_required(an._h, bad) == -1
        assert "mode %d" % bad in _err(an)
        assert an.tar_required() == "gpu"  # unchanged
    an.set_tar_required("host")
    assert an.tar_required() == "host"
    with pytest.raises(ValueError):
        an.set_tar_required("device")
    m = c.c_int(9)
    assert L.tsg_analyzer_set_tar_required(None, 1) == -1
    assert L.tsg_analyzer_get_tar_required(None, c.byref(m)) == -1 and m.value == 9
    assert L.tsg_analyzer_get_tar_required(an._h, None) == -1
    # the walk setter still refuses what is not a walk mode
    assert L.tsg_analyzer_set_tar_walk(an._h, 2) == -1


def test_required_stats_argument_errors():
    from trivy_amd.analyzer.secret import TAR_REQUIRED_STATS_SIZE_V1, _CTarRequiredStats
    an = _analyzer()
    entries, stop, n_cand = cm.chain(cm.ustar_layer())
    ix = _index_entries(an, entries, stop, n_cand, 1 << 20)
    rs = _CTarRequiredStats()
    for bogus in (0, 8, TAR_REQUIRED_STATS_SIZE_V1 - 8, TAR_REQUIRED_STATS_SIZE_V1 + 8):
        rs.struct_size = bogus
        assert an._L.tsg_tar_index_required_stats(ix._h, c.byref(rs)) == -1 and "struct_size %d" % bogus in _err(an)
    rs.struct_size = TAR_REQUIRED_STATS_SIZE_V1
    assert an._L.tsg_tar_index_required_stats(None, c.byref(rs)) == -1
    assert an._L.tsg_tar_index_required_stats(ix._h, None) == -1
    assert an._L.tsg_tar_index_required_stats(ix._h, c.byref(rs)) == 0 and rs.mode == 0 and rs.reason == 1


def test_env_sets_the_initial_mode():
    """TSG_TAR_REQUIRED is read when an analyzer is made: in a child process, so this one's environment stays."""
    code = ("from oracle import hostlib\n"
            "from trivy_amd.analyzer import AnalyzerOptions, SecretAnalyzer\n"
            "a = SecretAnalyzer(lib=hostlib.lib(), host_only=True)\n"
            "a.Init(AnalyzerOptions())\n"
            "print(a.tar_required(), a.tar_walk())\n")
    for value, want in (("gpu", "gpu"), ("host", "host"), ("GPU", "host"), ("", "host"), (None, "host")):
        env = dict(os.environ)
        env.pop("TSG_TAR_REQUIRED", None)
        env.pop("TSG_TAR_WALK", None)
        if value is not None:
            env["TSG_TAR_REQUIRED"] = value
        out = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), env=env, check=True, capture_output=True,
                             text=True).stdout.split()
        assert out[-2:] == [want, "host"], (value, out)


def test_struct_layout(tmp_path):
    from trivy_amd.analyzer.secret import TAR_REQUIRED_STATS_SIZE_V1, _CTarRequiredStats
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "tsg_analyzer.h"\nint main(void){printf("%zu %u %zu %zu %zu %zu %zu\\n",'
                   ' sizeof(tsg_tar_required_stats), (unsigned)TSG_TAR_REQUIRED_STATS_SIZE_V1,'
                   ' offsetof(tsg_tar_required_stats, mode), offsetof(tsg_tar_required_stats, reason),'
                   ' offsetof(tsg_tar_required_stats, entries), offsetof(tsg_tar_required_stats, path_bytes),'
                   ' offsetof(tsg_tar_required_stats, ms_kernel)); return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    size, v1, o_mode, o_reason, o_entries, o_pb, o_ms = \
        [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert size == v1 == c.sizeof(_CTarRequiredStats) == TAR_REQUIRED_STATS_SIZE_V1 == 16 + 7 * 8 + 3 * 8
    assert o_mode == _CTarRequiredStats.mode.offset == 8 and o_reason == _CTarRequiredStats.reason.offset == 12
    assert o_entries == _CTarRequiredStats.entries.offset == 16 and o_pb == _CTarRequiredStats.path_bytes.offset == 64
    assert o_ms == _CTarRequiredStats.ms_kernel.offset == 72
    assert rm.FREC.size == 48 and len(rm.COUNTS) == 16
