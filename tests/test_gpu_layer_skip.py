"""LayerTar's skipDirs / skipFiles end to end on the GPU (SecretAnalyzer.set_layer_walker,
tsg_analyzer_set_tar_skip): AnalyzeLayer in copy and in gather mode and AnalyzeLayerDevice in both tar-walk
modes return what tests/tar_skip_model.py -- walker/tar.go:35-116 restated over tarfile, with the oracle's
analyzer -- returns for the same layer and options.  Every regular file of these layers carries a secret, so a
file wrongly kept or wrongly dropped is a finding too many or too few.
"""
import numpy as np
import pytest

from oracle import analyzer as oan
from tests import tar_skip_model as sm

pytestmark = pytest.mark.gpu

CASES = sm.cases()
CASES["order"] = (sm.order_layer(), ["**/skipme"], ["**/7.conf"])
_cache = {}


@pytest.fixture(scope="module")
def analyzer():
    from trivy_amd.analyzer import AnalyzerOptions, SecretAnalyzer
    a = SecretAnalyzer()
    a.Init(AnalyzerOptions())
    yield a
    a.set_tar_walk("host")
    a.set_layer_walker(None)


@pytest.fixture(scope="module")
def oracle():
    return oan.SecretAnalyzer("")


def _walker(sd, sf):
    from trivy_amd.walker import NewLayerTar, Option
    return NewLayerTar(Option(SkipFiles=list(sf), SkipDirs=list(sd)))


def _case(name, oracle):
    """(layer, numpy copy, resident tensor of len + 64, the model's walk, its secrets in walk order, the
    unfiltered secrets), computed once per layer."""
    if name not in _cache:
        import torch
        layer, sd, sf = CASES[name]
        assert len(layer) < 300 << 10
        host = np.frombuffer(layer, dtype=np.uint8).copy()
        dev = torch.from_numpy(np.frombuffer(layer + b"\xee" * 64, dtype=np.uint8).copy()).to("cuda:0")
        m = sm.walk(layer, sd, sf)
        want = sm.analyze(oracle, layer, sd, sf)
        plain = sm.analyze(oracle, layer)
        # every kept file has its finding, every dropped one would have had one
        assert [s["FilePath"] for s in want] == ["/" + fp for fp, _, _ in m["kept"]] and m["kept"] and m["dropped"]
        assert {s["FilePath"] for s in plain} == {s["FilePath"] for s in want} | {"/" + fp for fp in m["dropped"]}
        _cache[name] = (layer, host, dev, m, want, plain)
    return _cache[name]


def _secrets(result):
    return [s.to_dict() for s in result.Secrets]


def _skip_counts(m):
    return {"skipped_dirs": len(m["skipped_dirs"]), "skipped_files": m["skipped_files"],
            "under_skipped_dir": m["under_skipped_dir"]}


@pytest.mark.parametrize("name", list(CASES))
def test_every_layer_path_vs_model(analyzer, oracle, name):
    layer, host, dev, m, want, plain = _case(name, oracle)
    analyzer.set_layer_walker(_walker(*CASES[name][1:]))
    try:
        for kw in ({}, {"gpu_transform": True}, {"gather": True}):
            st = {}
            assert _secrets(analyzer.AnalyzeLayer(host, stats=st, **kw)) == want, kw
            assert {k: st[k] for k in _skip_counts(m)} == _skip_counts(m), kw
            assert (st["regular"], st["whiteouts"], st["opaque_dirs"]) == (m["regular"], m["whiteouts"], m["opaque_dirs"])
            assert st["required"] == len(m["kept"])
        for mode in ("host", "gpu"):
            analyzer.set_tar_walk(mode)
            st = {}
            assert _secrets(analyzer.AnalyzeLayerDevice(dev, stats=st)) == want, mode
            assert {k: st[k] for k in _skip_counts(m)} == _skip_counts(m), mode
            assert (st["regular"], st["whiteouts"], st["opaque_dirs"]) == (m["regular"], m["whiteouts"], m["opaque_dirs"])
            assert st["required"] == st["files"] == len(m["kept"])
            assert st["walk"]["walk"] == mode and st["walk"]["fallback"] == 0
            if mode == "gpu":  # the GPU walk completed the layer: nothing was left to the host walk
                assert analyzer.last_tar_fallback() == 0 and st["walk"]["chain_entries"] > 0
                assert st["block_fetches"] == 0
            files, ist = analyzer.IndexLayerDevice(dev)
            assert [p for p, _, _ in files] == [fp for fp, _, _ in m["kept"]]
            assert {k: ist[k] for k in _skip_counts(m)} == _skip_counts(m)
    finally:
        analyzer.set_tar_walk("host")
        analyzer.set_layer_walker(None)


def test_batches_cut_between_the_dir_and_its_files(analyzer, oracle):
    """The skipped directory's entry is in the first batch, its files in later ones."""
    layer, host, dev, m, want, plain = _case("order", oracle)
    analyzer.set_layer_walker(_walker(*CASES["order"][1:]))
    try:
        for kw in ({}, {"gather": True}):
            st = {}
            assert _secrets(analyzer.AnalyzeLayer(host, arena_bytes=2048, stats=st, **kw)) == want, kw
            assert st["input_bytes"] > 3 * 2048  # (a batch holds at most 2,048 bytes of these small files: 4 or more)
            assert {k: st[k] for k in _skip_counts(m)} == _skip_counts(m)
        for mode in ("host", "gpu"):
            analyzer.set_tar_walk(mode)
            ix = analyzer.IndexDevice(dev)
            batches = ix.batches(48 << 10)
            assert len(batches) >= 3 and ix.walk_stats["fallback"] == 0
            # the directory's entry lies in the first batch's span, its later files after that span
            second = int(ix.start[batches[1][0]])
            assert layer.find(b"z/skipme/\0") < second <= layer.find(b"z/skipme/late-0.conf\0")
            for depth in (1, 2):
                assert _secrets(analyzer.AnalyzeLayerDevice(dev, arena_bytes=48 << 10, depth=depth)) == want
    finally:
        analyzer.set_tar_walk("host")
        analyzer.set_layer_walker(None)


def test_analyze_layers_workers_inherit_the_option(analyzer, oracle):
    names = ["order", "after", "before", "parent"]
    cs = [_case(n, oracle) for n in names]
    analyzer.set_layer_walker(_walker(["**/skipme", "a/b", "c/d/e"], ["**/7.conf"]))
    try:
        want = [sm.sort_secrets(sm.analyze(oracle, c[0], ["**/skipme", "a/b", "c/d/e"], ["**/7.conf"])) for c in cs]
        for kw in ({}, {"gather": True}):
            st = []
            got = analyzer.AnalyzeLayers([c[1] for c in cs], parallel=2, arena_bytes=4096, stats=st, **kw)
            assert [_secrets(r) for r in got] == want, kw
            assert [s["under_skipped_dir"] for s in st] == \
                [sm.walk(c[0], ["**/skipme", "a/b", "c/d/e"], ["**/7.conf"])["under_skipped_dir"] for c in cs]
        # workers made before the option changes take the new one
        workers = analyzer.LayerWorkers(parallel=2, arena_bytes=4096)
        analyzer.set_layer_walker(None)
        got = analyzer.AnalyzeLayers([c[1] for c in cs], workers=workers)
        assert [_secrets(r) for r in got] == [sm.sort_secrets(list(c[5])) for c in cs]
    finally:
        analyzer.set_layer_walker(None)


def test_clearing_the_option_restores_the_unfiltered_result(analyzer, oracle):
    layer, host, dev, m, want, plain = _case("order", oracle)
    assert len(plain) > len(want)
    analyzer.set_layer_walker(_walker(*CASES["order"][1:]))
    try:
        assert _secrets(analyzer.AnalyzeLayer(host)) == want
        analyzer.set_tar_walk("gpu")
        assert _secrets(analyzer.AnalyzeLayerDevice(dev)) == want
        analyzer.set_layer_walker(None)
        st = {}
        assert _secrets(analyzer.AnalyzeLayerDevice(dev, stats=st)) == plain
        assert st["skipped_dirs"] == st["skipped_files"] == st["under_skipped_dir"] == 0
        analyzer.set_tar_walk("host")
        assert _secrets(analyzer.AnalyzeLayerDevice(dev)) == plain
        for kw in ({}, {"gather": True}):
            st = {}
            assert _secrets(analyzer.AnalyzeLayer(host, stats=st, **kw)) == plain
            assert st["skipped_dirs"] == st["skipped_files"] == st["under_skipped_dir"] == 0
    finally:
        analyzer.set_tar_walk("host")
        analyzer.set_layer_walker(None)
