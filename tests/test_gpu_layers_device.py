"""All layers of an image resident in HBM, end to end (SecretAnalyzer.AnalyzeLayersDevice, IndexLayersDevice;
tsg_analyzer_index_device_tars): per layer the result equals AnalyzeLayers' of the host copies,
AnalyzeLayerDevice's of that layer alone and oracle/analyzer.py's, in both tar-walk modes, with the layers held
as separate tensors and as adjacent slices of one buffer.  The per-layer fallback never hides a broken kernel:
on every well-formed image no layer falls back in "gpu" mode.
"""
import tarfile
import threading

import numpy as np
import pytest

from oracle import analyzer as oan
from tests import tar_chain_model as cm
from tests import tar_index_model as tm
from tests.layers import make_layer

pytestmark = pytest.mark.gpu

MODES = ("host", "gpu")


@pytest.fixture(scope="module")
def analyzer():
    from trivy_amd.analyzer import AnalyzerOptions, SecretAnalyzer
    a = SecretAnalyzer()
    a.Init(AnalyzerOptions())
    assert a.tar_walk() == "host"
    return a


def _sorted_oracle(oracle, layer):
    want = oan.analyze_layer(oracle, layer)
    want.sort(key=lambda s: s["FilePath"].encode("utf-8", "surrogateescape"))
    for s in want:
        s["Findings"].sort(key=lambda f: (f["RuleID"].encode(), f["StartLine"]))
    return want


def _dicts(result):
    return [s.to_dict() for s in result.Secrets]


def _resident(layers):
    """(separate tensors, slices of one buffer as (view, nbytes)): every layer is a multiple of 512 bytes."""
    import torch
    sep = [torch.from_numpy(np.frombuffer(ly + b"\xee" * 64, dtype=np.uint8).copy()).to("cuda:0") for ly in layers]
    assert all(len(ly) % 512 == 0 for ly in layers)
    buf = torch.from_numpy(np.frombuffer(b"".join(layers) + b"\xee" * 64, dtype=np.uint8).copy()).to("cuda:0")
    slices, at = [], 0
    for ly in layers:
        slices.append((buf[at:at + len(ly) + 64], len(ly)))
        at += len(ly)
    return sep, slices


class Image:
    """The six-layer fixture and its references, computed once, in "host" mode: per layer the oracle's sorted
    result, AnalyzeLayers' of the host copies, AnalyzeLayerDevice's (sorted) and the single-layer index."""

    def __init__(self, analyzer, layers):
        self.layers = layers
        self.sep, self.slices = _resident(layers)
        oracle = oan.SecretAnalyzer("")
        self.oracle = [_sorted_oracle(oracle, ly) for ly in layers]
        self.host = [_dicts(r) for r in analyzer.AnalyzeLayers(layers, gpu_transform=True)]
        self.single, self.index = [], []
        for t in self.sep:
            r = analyzer.AnalyzeLayerDevice(t)
            r.Sort()
            self.single.append(_dicts(r))
            ix = analyzer.IndexDevice(t)
            self.index.append((ix.files(), ix.start.tolist(), {k: v for k, v in ix.stats.items() if not k.startswith("ms_")}))
        assert self.host == self.oracle == self.single

    def check(self, results, base=None):
        assert len(results) == len(self.layers)
        for k, r in enumerate(results):
            assert _dicts(r) == ([] if base and base[k] else self.oracle[k]), k


@pytest.fixture(scope="module")
def image(analyzer):
    layers = [make_layer(100 + tarfile.GNU_FORMAT, 150, tarfile.GNU_FORMAT),
              make_layer(100 + tarfile.PAX_FORMAT, 150, tarfile.PAX_FORMAT), tm.nested_layer(), tm.no_trailer_layer(),
              tm.pax_size_layer(), bytes(1024)]
    img = Image(analyzer, layers)
    assert sum(len(r) for r in img.oracle) >= 20 and img.oracle[5] == []
    return img


@pytest.fixture()
def mode(request, analyzer):
    analyzer.set_tar_walk(request.param)
    yield request.param
    analyzer.set_tar_walk("host")


def _check_stats(img, stats, mode, base=None, groups=1):
    per, forest = stats[:-1], stats[-1]
    live = [k for k in range(len(img.layers)) if not (base and base[k])]
    assert len(per) == len(img.layers) and forest["layers"] == len(live)
    assert forest["fallbacks"] == 0
    assert forest["batched"] == (len(live) if mode == "gpu" else 0)
    assert forest["passes"] == (groups if mode == "gpu" else 0)
    assert min(forest[k] for k in ("index_s", "scan_s", "wall_s")) >= 0
    for k, st in enumerate(per):
        if k not in live:
            assert st is None  # a base layer: no index, no scan
            continue
        files, _, single = img.index[k]
        assert st["files"] == len(files)
        for key, v in single.items():  # (the single-layer index was made in "host" mode, which fetches blocks)
            if mode == "host" or key not in ("kernel_runs", "block_fetches", "ext_bytes"):
                assert st[key] == v, (k, key)
        ws = st["walk"]
        assert ws["walk"] == mode and ws["fallback"] == 0
        if mode == "gpu":
            entries, _, _ = cm.chain(img.layers[k])
            assert ws["chain_entries"] == len(entries) and ws["name_bytes"] == sum(len(e["name"]) for e in entries)
            assert ws["segments"] == (len(img.layers[k]) // 512 + 8191) // 8192
            assert st["block_fetches"] == 0 and st["ext_bytes"] == 0
    if mode == "gpu":
        assert forest["virtual_blocks"] == 8192 * sum(max(1, (len(img.layers[k]) // 512 + 8191) // 8192) for k in live)
        assert forest["segments"] == forest["virtual_blocks"] // 8192
        assert forest["device_bytes"] >= 20 * forest["virtual_blocks"] // groups


@pytest.mark.parametrize("held", ["separate", "slices"])
@pytest.mark.parametrize("mode", MODES, indirect=True)
def test_image_vs_host_single_layer_and_oracle(analyzer, image, mode, held):
    layers = image.sep if held == "separate" else image.slices
    stats = []
    image.check(analyzer.AnalyzeLayersDevice(layers, stats=stats))
    _check_stats(image, stats, mode)
    st = []
    ixs = analyzer.IndexLayersDevice(layers, stats=st)
    assert len(st) == len(layers) + 1 and st[-1]["fallbacks"] == 0
    for ix, (files, start, _) in zip(ixs, image.index):
        assert ix.files() == files and ix.start.tolist() == start
        assert ix.walk_stats["walk"] == mode and ix.walk_stats["fallback"] == 0


@pytest.mark.parametrize("held", ["separate", "slices"])
@pytest.mark.parametrize("fetch", ["files", "windows"])
@pytest.mark.parametrize("xform", ["chunked", "split"])
@pytest.mark.parametrize("mode", MODES, indirect=True)
def test_fetch_and_resident_transform_modes(analyzer, image, mode, fetch, xform, held):
    """Both walk modes x the four fetch x resident-transform modes: the batched result equals the oracle's and
    AnalyzeLayerDevice's of every layer alone, made in the same modes."""
    layers = image.sep if held == "separate" else image.slices
    s = analyzer.scanner
    s.set_fetch_mode(fetch)
    s.set_resident_transform(xform)
    try:
        stats = []
        got = analyzer.AnalyzeLayersDevice(layers, arena_bytes=64 << 10, stats=stats)
        single = []
        for ly in layers:
            r = analyzer.AnalyzeLayerDevice(*ly, arena_bytes=64 << 10) if isinstance(ly, tuple) else \
                analyzer.AnalyzeLayerDevice(ly, arena_bytes=64 << 10)
            r.Sort()
            single.append(_dicts(r))
    finally:
        s.set_fetch_mode("files")
        s.set_resident_transform("chunked")
    image.check(got)
    assert [_dicts(r) for r in got] == single
    assert stats[-1]["fallbacks"] == 0 and stats[-1]["batched"] == (6 if mode == "gpu" else 0)


@pytest.mark.parametrize("mode", MODES, indirect=True)
def test_base_layers_are_neither_indexed_nor_scanned(analyzer, image, mode):
    base = [True, False, True, False, False, True]
    stats = []
    image.check(analyzer.AnalyzeLayersDevice(image.sep, base=base, stats=stats), base)
    _check_stats(image, stats, mode, base)
    stats = []
    image.check(analyzer.AnalyzeLayersDevice(image.slices, base=[True] * 6, stats=stats), [True] * 6)
    assert stats[:-1] == [None] * 6 and stats[-1]["index_s"] == 0
    with pytest.raises(ValueError):
        analyzer.AnalyzeLayersDevice(image.sep, base=[True])


@pytest.mark.parametrize("mode", MODES, indirect=True)
def test_small_groups_and_depths(analyzer, image, mode):
    from trivy_amd.analyzer.secret import layer_groups
    group_bytes = 160 << 10
    groups = layer_groups([len(ly) for ly in image.layers], None, group_bytes)
    assert len(groups) >= 3
    for depth in (1, 3):
        stats = []
        image.check(analyzer.AnalyzeLayersDevice(image.slices, group_bytes=group_bytes, arena_bytes=32 << 10, depth=depth,
                                                 stats=stats))
        _check_stats(image, stats, mode, groups=len(groups))
    stats = []
    analyzer.AnalyzeLayersDevice(image.sep, group_bytes=group_bytes, materialize=False, stats=stats)
    assert any(k.startswith("scan_") for k in stats[0]) and stats[-1]["layers"] == 6


@pytest.mark.parametrize("mode", MODES, indirect=True)
def test_layer_walker_skip_options(analyzer, image, mode):
    """LayerTar's skip-dirs and skip-files: the stats and the result equal the per-layer path's."""
    from trivy_amd.walker import NewLayerTar, Option
    analyzer.set_layer_walker(NewLayerTar(Option(SkipFiles=["**/README.md"], SkipDirs=["etc/app", "**/conf"])))
    try:
        want, want_stats = [], []
        for t in image.sep:
            st = {}
            r = analyzer.AnalyzeLayerDevice(t, stats=st)
            r.Sort()
            want.append(_dicts(r))
            want_stats.append(st)
        stats = []
        got = analyzer.AnalyzeLayersDevice(image.slices, stats=stats)
    finally:
        analyzer.set_layer_walker(None)
    assert [_dicts(r) for r in got] == want and want != image.oracle
    assert sum(st["skipped_dirs"] + st["skipped_files"] for st in want_stats) > 0
    for st, ws in zip(stats[:-1], want_stats):
        for key in ("entries", "regular", "required", "whiteouts", "opaque_dirs", "skipped_dirs", "skipped_files",
                    "under_skipped_dir", "files", "candidates", "off_chain"):
            assert st[key] == ws[key], key
    assert stats[-1]["fallbacks"] == 0


def test_a_layer_the_device_leaves_to_the_host_falls_back_alone(analyzer, image):
    """A PAX size the GPU does not decide, in the middle of the image: that layer is indexed by the host walk,
    the others keep their batched index, and every result is the per-layer path's."""
    import torch
    punt, reason, _ = cm.punt_cases()["pax-size-with-sign"]
    t = torch.from_numpy(np.frombuffer(punt + b"\xee" * 64, dtype=np.uint8).copy()).to("cuda:0")
    layers = image.sep[:3] + [t] + image.sep[3:]
    want = analyzer.AnalyzeLayerDevice(t)
    want.Sort()
    analyzer.set_tar_walk("gpu")
    try:
        stats = []
        got = analyzer.AnalyzeLayersDevice(layers, stats=stats)
    finally:
        analyzer.set_tar_walk("host")
    forest = stats[-1]
    assert forest["layers"] == 7 and forest["fallbacks"] == 1 and forest["batched"] == 6
    assert [st["walk"]["fallback"] for st in stats[:-1]] == [0, 0, 0, reason, 0, 0, 0]
    assert stats[3]["walk"]["walk"] == "gpu" and stats[3]["walk"]["chain_entries"] == 0
    assert _dicts(got[3]) == _dicts(want) and stats[3]["entries"] >= 3
    image.check(got[:3] + got[4:])


@pytest.mark.parametrize("mode", MODES, indirect=True)
def test_a_malformed_layer_in_the_middle(analyzer, image, mode):
    """The ValueError carries the text AnalyzeLayerDevice gives for that layer, with the layer's number;
    nothing is left in flight, and the analyzer works afterwards."""
    import torch
    good = make_layer(3, 60)
    entries, _, _ = cm.chain(good)
    off = [e for e in entries if e["typeflag"] == 0x30 and e["n_ext"] == 0][5]["hdr"]
    bad = bytearray(good)
    bad[off + 150] ^= 0x01  # a header in mid-layer: its checksum field off by one
    t = torch.from_numpy(np.frombuffer(bytes(bad) + b"\xee" * 64, dtype=np.uint8).copy()).to("cuda:0")
    with pytest.raises(ValueError) as single:
        analyzer.AnalyzeLayerDevice(t)
    assert str(single.value) == "tar layer: tar: invalid header checksum at offset %d" % off
    layers = image.sep[:4] + [t] + image.sep[4:]
    n_threads = threading.active_count()
    for kw in ({}, {"group_bytes": 160 << 10, "arena_bytes": 32 << 10}):
        with pytest.raises(ValueError) as e:
            analyzer.AnalyzeLayersDevice(layers, **kw)
        assert str(e.value) == "tar layer 4: tar: invalid header checksum at offset %d" % off
        assert threading.active_count() == n_threads  # the index thread was joined
    with pytest.raises(ValueError) as e:
        analyzer.IndexLayersDevice(layers)
    assert str(e.value) == "tar layer 4: tar: invalid header checksum at offset %d" % off
    with pytest.raises(ValueError):
        analyzer.AnalyzeLayersDevice([image.sep[0], image.sep[0][::2]])  # not contiguous
    image.check(analyzer.AnalyzeLayersDevice(image.slices))


def test_two_threads_at_once(analyzer, image):
    analyzer.set_tar_walk("gpu")
    out, errors = [None, None], []

    def work(k):
        try:
            res = []
            for _ in range(2):
                stats = []
                r = analyzer.AnalyzeLayersDevice(image.slices if k else image.sep, arena_bytes=48 << 10, stats=stats)
                res.append((r, stats))
            out[k] = res
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
    try:
        threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    finally:
        analyzer.set_tar_walk("host")
    assert not errors, errors
    for k in range(2):
        for r, stats in out[k]:
            image.check(r)
            _check_stats(image, stats, "gpu")
