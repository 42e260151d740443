"""A resident tar layer with the header chain walked on the GPU (SecretAnalyzer.set_tar_walk("gpu"),
tsg_analyzer_set_tar_walk) end to end: the index, its stats and AnalyzeLayerDevice's result equal
host mode's, AnalyzeLayer's of the same bytes on the host and oracle/analyzer.py's; a layer the GPU walk does not
complete falls back to the host walk and gives its error text; the fallback never hides a broken kernel: every
well-formed layer indexes with fallback == 0.
"""
import random
import tarfile
import threading

import numpy as np
import pytest

from oracle import analyzer as oan
from tests import tar_chain_model as cm
from tests import tar_index_model as tm
from tests.layers import make_layer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def analyzer():
    from trivy_amd.analyzer import AnalyzerOptions, SecretAnalyzer
    a = SecretAnalyzer()
    a.Init(AnalyzerOptions())
    assert a.tar_walk() == "host"
    return a


@pytest.fixture(scope="module")
def oracle():
    return oan.SecretAnalyzer("")


@pytest.fixture()
def gpu_walk(analyzer):
    analyzer.set_tar_walk("gpu")
    yield analyzer
    analyzer.set_tar_walk("host")


LAYERS = {
    "gnu": lambda: make_layer(100 + tarfile.GNU_FORMAT, 150, tarfile.GNU_FORMAT),
    "pax": lambda: make_layer(100 + tarfile.PAX_FORMAT, 150, tarfile.PAX_FORMAT),
    "ustar": cm.ustar_layer,
    "odd-names": cm.odd_names_layer,
    "nested": tm.nested_layer,
    "pax-size": tm.pax_size_layer,
    "no-trailer": tm.no_trailer_layer,
    "boundaries": lambda: cm.boundary_layer(64),
}
_cache = {}


def _dev(layer: bytes):
    import torch
    return torch.from_numpy(np.frombuffer(layer + b"\xee" * 64, dtype=np.uint8).copy()).to("cuda:0")


def _case(name, analyzer, oracle):
    """(layer, resident tensor, the oracle's result sorted, AnalyzeLayer's of the host copy, host mode's index
    files / spans / stats), computed once per layer, in host mode (whatever mode is in force)."""
    if name not in _cache:
        mode = analyzer.tar_walk()
        analyzer.set_tar_walk("host")
        try:
            layer = LAYERS[name]()
            want = oan.analyze_layer(oracle, layer)
            want.sort(key=lambda s: s["FilePath"].encode("utf-8", "surrogateescape"))
            for s in want:
                s["Findings"].sort(key=lambda f: (f["RuleID"].encode(), f["StartLine"]))
            host = analyzer.AnalyzeLayer(layer, gpu_transform=True)
            dev = _dev(layer)
            ix = analyzer.IndexDevice(dev)
            assert ix.walk_stats["walk"] == "host"
            _cache[name] = (layer, dev, want, [s.to_dict() for s in host.Secrets],
                            (ix.files(), ix.start.tolist(), ix.stats))
        finally:
            analyzer.set_tar_walk(mode)
    return _cache[name]


def _same(got, want, host):
    assert [s.to_dict() for s in got.Secrets] == host  # the same files in the same (walk) order
    got.Sort()
    assert [s.to_dict() for s in got.Secrets] == want


def _check_index(ix, layer, host_index):
    files, start, hst = host_index
    assert ix.files() == files and ix.start.tolist() == start
    for k in ("entries", "regular", "required", "whiteouts", "opaque_dirs", "blocks", "candidates", "off_chain"):
        assert ix.stats[k] == hst[k], k
    ws = ix.walk_stats
    assert ws["walk"] == "gpu" and ws["fallback"] == 0
    assert ix.stats["kernel_runs"] == 1 and ix.stats["block_fetches"] == 0 and ix.stats["ext_bytes"] == 0
    entries, stop, _ = cm.chain(layer)
    assert ws["chain_entries"] == len(entries) == hst["entries"]
    assert ws["name_bytes"] == sum(len(e["name"]) for e in entries)
    assert ws["segments"] == (len(layer) // 512 + 8191) // 8192 and ws["device_bytes"] >= 20 * (len(layer) // 512)
    assert ix.stats["ms_kernel"] > 0 and ix.stats["ms_total"] >= ix.stats["ms_kernel"]
    assert min(ws[k] for k in ("ms_candidates", "ms_entries", "ms_mark", "ms_compact")) > 0


@pytest.mark.parametrize("name", list(LAYERS))
def test_layer_vs_host_mode_oracle_and_host(analyzer, oracle, name):
    layer, dev, want, host, host_index = _case(name, analyzer, oracle)
    analyzer.set_tar_walk("gpu")
    try:
        _check_index(analyzer.IndexDevice(dev), layer, host_index)
        files, stats = analyzer.IndexLayerDevice(dev)
        assert files == host_index[0]
        _same(analyzer.AnalyzeLayerDevice(dev), want, host)
    finally:
        analyzer.set_tar_walk("host")
    req = [(fp, size) for fp, size, _ in oan.walk_layer_tar(layer)[0] if oracle.required(fp, size)]
    assert [(p, s) for p, _, s in files] == req and len(req) >= 1


def test_many_batches_and_another_mode_pair(analyzer, oracle, gpu_walk):
    """Small arenas (many batches), and the windows fetch with the split scan instead of the defaults."""
    layer, dev, want, host, host_index = _case("gnu", analyzer, oracle)
    ix = analyzer.IndexDevice(dev)
    _check_index(ix, layer, host_index)
    assert len(ix.batches(32 << 10)) >= 5
    for depth in (1, 3):
        _same(analyzer.AnalyzeLayerDevice(dev, arena_bytes=32 << 10, depth=depth), want, host)
    s = analyzer.scanner
    s.set_fetch_mode("windows")
    s.set_resident_transform("split")
    try:
        for name in ("gnu", "pax"):
            layer, dev, want, host, _ = _case(name, analyzer, oracle)
            _same(analyzer.AnalyzeLayerDevice(dev, arena_bytes=64 << 10), want, host)
    finally:
        s.set_fetch_mode("files")
        s.set_resident_transform("chunked")


def _malformed():
    """tests/test_device_layer_abi.py's malformed layers, rebuilt: (bytes, the host walk's message or None)."""
    out = []
    good = make_layer(3, 60)
    entries, _, _ = cm.chain(good)
    reg = [e for e in entries if e["typeflag"] == 0x30 and e["n_ext"] == 0]
    layer = bytearray(good)
    off = reg[5]["hdr"]
    layer[off + 150] ^= 0x01  # a header in mid-layer: its checksum field off by one
    out.append((bytes(layer), "tar: invalid header checksum at offset %d" % off))
    good = make_layer(4, 20)
    last = cm.chain(good)[0][-1]
    out.append((good[:last["data"] + last["size"] - 3], "tar: truncated entry data"))
    junk = bytearray(good)
    junk[last["hdr"]:last["hdr"] + 512] = bytes(random.Random(1).randrange(1, 256) for _ in range(512))
    out.append((bytes(junk), None))
    out.append((cm.punt_cases()["bad-pax-record"][0], "tar: invalid PAX record"))
    out.append((cm.punt_cases()["negative-size"][0], "tar: invalid size field"))
    out.append((good[:300], "tar: truncated header"))
    return out


@pytest.mark.parametrize("k", range(6))
def test_malformed_layers_give_the_host_walks_error(analyzer, k):
    layer, text = _malformed()[k]
    dev = _dev(layer)
    assert analyzer.tar_walk() == "host"
    with pytest.raises(ValueError) as e_host:
        analyzer.IndexDevice(dev, nbytes=len(layer))
    analyzer.set_tar_walk("gpu")
    try:
        with pytest.raises(ValueError) as e_gpu:
            analyzer.IndexDevice(dev, nbytes=len(layer))
        fallback = analyzer.last_tar_fallback()
    finally:
        analyzer.set_tar_walk("host")
    assert str(e_gpu.value) == str(e_host.value)
    assert fallback != 0 and fallback == cm.chain(layer)[1][1]  # the GPU walk stopped, for the model's reason
    if text is not None:
        assert str(e_gpu.value) == "tar layer: " + text


@pytest.mark.parametrize("name", ["pax-size-with-sign", "pax-data-64KiB+1", "17-extension-headers", "long-name-64KiB+1"])
def test_what_the_device_leaves_to_the_host_is_indexed_by_it(analyzer, name):
    """A layer the device does not decide but the host walk accepts: the index is host mode's, and
    fallback says why the GPU walk's result was not used."""
    layer, reason, _ = cm.punt_cases()[name]
    dev = _dev(layer)
    want = analyzer.IndexDevice(dev)
    analyzer.set_tar_walk("gpu")
    try:
        got = analyzer.IndexDevice(dev)
    finally:
        analyzer.set_tar_walk("host")
    assert got.files() == want.files() and got.start.tolist() == want.start.tolist() and got.stats["entries"] >= 3
    assert {k: v for k, v in got.stats.items() if not k.startswith("ms_")} == \
        {k: v for k, v in want.stats.items() if not k.startswith("ms_")}
    ws = got.walk_stats
    assert ws["walk"] == "gpu" and ws["fallback"] == reason != 0 and ws["chain_entries"] == 0
    assert want.walk_stats["fallback"] == 0


def test_two_layers_in_flight_from_two_threads(analyzer, oracle, gpu_walk):
    cases = [_case(n, analyzer, oracle) for n in ("gnu", "pax")]
    out, errors = [None, None], []

    def work(k):
        try:
            res = []
            for _ in range(2):
                ix = analyzer.IndexDevice(cases[k][1])
                res.append((ix, analyzer.AnalyzeLayerDevice(cases[k][1], arena_bytes=48 << 10, depth=2)))
            out[k] = res
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(2):
        for ix, got in out[k]:
            _check_index(ix, cases[k][0], cases[k][4])
            _same(got, cases[k][2], cases[k][3])


def test_empty_layers(analyzer, gpu_walk):
    for n in (0, 512, 4096):
        ix = analyzer.IndexDevice(_dev(bytes(n)), nbytes=n)
        assert ix.n == 0 and ix.stats["entries"] == 0 and ix.walk_stats["fallback"] == 0
