"""A tar layer resident in HBM end to end (SecretAnalyzer.AnalyzeLayerDevice / IndexLayerDevice,
tsg_analyzer_index_device_tar / _submit_device_tar): the GPU finds the headers, the host
follows the chain, each batch is scanned with the layer itself as its arena.  The result equals
oracle/analyzer.py's analyze_layer and AnalyzeLayer of the same bytes held on the host.
"""
import ctypes as c
import tarfile
import threading

import numpy as np
import pytest

from oracle import analyzer as oan
from tests import tar_index_model as tm
from tests.layers import make_layer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def analyzer():
    from trivy_amd.analyzer import AnalyzerOptions, SecretAnalyzer
    a = SecretAnalyzer()
    a.Init(AnalyzerOptions())
    a._L.tsg_debug_set_tar_capacity.argtypes = [c.c_uint64]
    return a


@pytest.fixture(scope="module")
def oracle():
    return oan.SecretAnalyzer("")


LAYERS = {
    "gnu": lambda: make_layer(100 + tarfile.GNU_FORMAT, 150, tarfile.GNU_FORMAT),
    "pax": lambda: make_layer(100 + tarfile.PAX_FORMAT, 150, tarfile.PAX_FORMAT),
    "nested": tm.nested_layer,
    "pax-size": tm.pax_size_layer,
    "no-trailer": tm.no_trailer_layer,  # the last file's data ends exactly at n_bytes: only the 64-B pad follows
}
_cache = {}


def _case(name, analyzer, oracle):
    """(layer bytes, resident tensor of len + 64, the oracle's result sorted, AnalyzeLayer's of the host copy),
    computed once per layer."""
    if name not in _cache:
        import torch
        layer = LAYERS[name]()
        want = oan.analyze_layer(oracle, layer)
        want.sort(key=lambda s: s["FilePath"].encode("utf-8", "surrogateescape"))
        for s in want:  # AnalysisResult.Sort (analyzer.go:225-234)
            s["Findings"].sort(key=lambda f: (f["RuleID"].encode(), f["StartLine"]))
        host = analyzer.AnalyzeLayer(layer, gpu_transform=True)
        dev = torch.from_numpy(np.frombuffer(layer + b"\xee" * 64, dtype=np.uint8).copy()).to("cuda:0")
        _cache[name] = (layer, dev, want, [s.to_dict() for s in host.Secrets])
    return _cache[name]


def _same(got, want, host):
    assert [s.to_dict() for s in got.Secrets] == host  # the same files in the same (walk) order
    got.Sort()
    assert [s.to_dict() for s in got.Secrets] == want


@pytest.mark.parametrize("name", list(LAYERS))
def test_layer_vs_oracle_and_host(analyzer, oracle, name):
    layer, dev, want, host = _case(name, analyzer, oracle)
    st = {}
    got = analyzer.AnalyzeLayerDevice(dev, stats=st)
    _same(got, want, host)
    assert len(want) >= (1 if name == "nested" else 2)  # (Required refuses inner.tar by its extension)
    # the stats against the oracle's counts and the model's
    files, wh, opq = oan.walk_layer_tar(layer)
    cands = tm.candidates(layer)
    assert st["regular"] == len(files) and st["whiteouts"] == wh and st["opaque_dirs"] == opq
    assert st["required"] == sum(1 for fp, size, _ in files if oracle.required(fp, size)) == st["files"]
    assert st["blocks"] == len(layer) // 512 and st["candidates"] == len(cands) and st["kernel_runs"] == 1
    on_chain = {"nested": 2, "pax-size": 3}.get(name, len(cands))
    assert st["off_chain"] == len(cands) - on_chain
    if name in ("nested", "pax-size"):
        assert st["off_chain"] > 0
    assert st["block_fetches"] == (0 if name == "no-trailer" else 1)
    assert st["ms_kernel"] > 0 and st["ms_total"] >= st["ms_kernel"]


def test_index_layer_device(analyzer, oracle):
    layer, dev, _, _ = _case("gnu", analyzer, oracle)
    st = {}
    files, stats = analyzer.IndexLayerDevice(dev, stats=st)
    assert stats == st
    want = [(fp, size, content) for fp, size, content in oan.walk_layer_tar(layer)[0] if oracle.required(fp, size)]
    assert [(p, s) for p, _, s in files] == [(fp, size) for fp, size, _ in want]
    assert all(layer[off:off + size] == content for (_, off, size), (_, _, content) in zip(files, want))
    # an explicit nbytes; a tensor that is too short is refused
    files2, _ = analyzer.IndexLayerDevice(dev, nbytes=len(layer))
    assert files2 == files
    with pytest.raises(ValueError):
        analyzer.IndexLayerDevice(dev, nbytes=len(layer) + 1)
    with pytest.raises(ValueError):
        analyzer.AnalyzeLayerDevice(dev[:len(layer) + 63], nbytes=len(layer))
    with pytest.raises(ValueError):
        analyzer.AnalyzeLayerDevice(dev[1:])  # not 16-B aligned


@pytest.mark.parametrize("depth", [1, 3])
def test_many_batches(analyzer, oracle, depth):
    layer, dev, want, host = _case("gnu", analyzer, oracle)
    ix = analyzer.IndexDevice(dev)
    batches = ix.batches(32 << 10)
    assert len(batches) >= 5 and sum(n for _, n in batches) == ix.n
    assert [f for f, _ in batches] == [sum(n for _, n in batches[:k]) for k in range(len(batches))]
    ends = ix.data_off[:ix.n] + ix.size[:ix.n]
    for first, n in batches:  # at most 32 KiB from where the batch's arena begins, unless a single file is larger
        base = int(ix.start[first])  # (equal to the plan's base: tests/test_device_layer_abi.py)
        assert base % 512 == 0 and base <= int(ix.data_off[first]) - 512
        assert base >= (int(ends[first - 1]) if first else 0)
        assert int(ends[first + n - 1]) - base <= 32 << 10 or n == 1
        if first + n < ix.n:  # and no batch stops early: the next file would not have fitted
            assert int(ends[first + n]) - base > 32 << 10
    # entries with a GNU long name: the chain starts at the 'L' header, two or more blocks before the entry's own
    assert any(int(ix.start[i]) < int(ix.data_off[i]) - 512 for i in range(ix.n))
    _same(analyzer.AnalyzeLayerDevice(dev, arena_bytes=32 << 10, depth=depth), want, host)


@pytest.mark.parametrize("fetch", ["files", "windows"])
@pytest.mark.parametrize("resident", ["chunked", "split"])
def test_fetch_and_resident_modes(analyzer, oracle, fetch, resident):
    s = analyzer.scanner
    s.set_fetch_mode(fetch)
    s.set_resident_transform(resident)
    try:
        for name in ("gnu", "nested"):
            layer, dev, want, host = _case(name, analyzer, oracle)
            _same(analyzer.AnalyzeLayerDevice(dev, arena_bytes=64 << 10), want, host)
        # the modes did apply to a layer batch.  The windows fetch applies to the files scanned where they
        # lie, that is in split mode (a transformed batch in chunks keeps the files fetch)
        ix = analyzer.IndexDevice(_case("gnu", analyzer, oracle)[1])
        p = ix.submit(0, ix.n)
        p.wait()
        ws = p.result.fetch_window_stats()
        assert p.result.split_stats()["mode_used"] == (1 if resident == "split" else 0)
        assert ws["mode_used"] == (1 if (fetch, resident) == ("windows", "split") else 0)
        if ws["mode_used"]:
            assert ws["window_bytes"] > 0 and ws["granules"] > 0
        else:
            assert p.result.fetch_stats()["files"] > 0 and ws["window_bytes"] == 0
    finally:
        s.set_fetch_mode("files")
        s.set_resident_transform("chunked")


def test_overflow_runs_the_kernel_again(analyzer, oracle):
    layer, dev, want, host = _case("gnu", analyzer, oracle)
    n_cands = len(tm.candidates(layer))
    analyzer._L.tsg_debug_set_tar_capacity(n_cands // 3)
    try:
        st = {}
        got = analyzer.AnalyzeLayerDevice(dev, stats=st)
    finally:
        analyzer._L.tsg_debug_set_tar_capacity(0)
    assert st["kernel_runs"] == 2 and st["candidates"] == n_cands
    _same(got, want, host)
    st = {}
    analyzer.IndexLayerDevice(dev, stats=st)
    assert st["kernel_runs"] == 1


def test_two_layers_in_flight_from_two_threads(analyzer, oracle):
    cases = [_case("gnu", analyzer, oracle), _case("pax", analyzer, oracle)]
    out, errors = [None, None], []

    def work(k):
        try:
            out[k] = [analyzer.AnalyzeLayerDevice(cases[k][1], arena_bytes=48 << 10, depth=2) for _ in range(2)]
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(2):
        for got in out[k]:
            _same(got, cases[k][2], cases[k][3])


def test_result_indexing(analyzer, oracle):
    """Result file 2 j + 1 is index file first + j; the even results are gaps, kind 0."""
    layer, dev, _, _ = _case("gnu", analyzer, oracle)
    ix = analyzer.IndexDevice(dev)
    first, n = 3, ix.n - 5
    p = ix.submit(first, n)
    got = p.wait()
    raw = p.result.raw()
    assert len(raw) == 2 * n + 1 and len(got) == n
    assert all(r["kind"] == 0 for r in raw[0::2])
    found = {ix.path(first + j) for j, g in enumerate(got) if g is not None}
    want = {s["FilePath"][1:] for s in oan.analyze_layer(oracle, layer)}
    assert found == want & {ix.path(i) for i in range(first, first + n)} and len(found) > 5
    assert all(g is None or g.FilePath == "/" + ix.path(first + j) for j, g in enumerate(got))


def test_malformed_layer(analyzer):
    import torch
    layer = bytearray(make_layer(3, 60))
    layer[148] ^= 0x01
    dev = torch.from_numpy(np.frombuffer(bytes(layer) + bytes(64), dtype=np.uint8).copy()).to("cuda:0")
    with pytest.raises(ValueError) as e:
        analyzer.AnalyzeLayerDevice(dev)
    assert "tar: invalid header checksum at offset 0" in str(e.value)
