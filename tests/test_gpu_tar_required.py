"""A resident tar layer whose path classify and Required run on the GPU (SecretAnalyzer.set_tar_required("gpu"),
tsg_analyzer_set_tar_required) end to end: under both required modes the index, its stats and
AnalyzeLayerDevice's result equal each other, AnalyzeLayer's of the same bytes on the host and
oracle/analyzer.py's; the stage is in force on every well-formed layer (reason 0) and gives way, with the
reason, to walk mode host, to skip options and to a layer the GPU walk does not complete.
"""
import threading

import numpy as np
import pytest

from oracle import analyzer as oan
from tests import tar_chain_model as cm
from tests import tar_required_model as rm
from tests.test_tar_required_host import CONFIG_BASE, LAYERS as HOST_LAYERS, NAME_TABLE

pytestmark = pytest.mark.gpu

LAYERS = {k: v for k, v in HOST_LAYERS.items() if not k.startswith("case-")}
CASES = {k: v for k, v in HOST_LAYERS.items() if k.startswith("case-")}
STAT_KEYS = ("entries", "regular", "required", "whiteouts", "opaque_dirs", "blocks", "candidates", "off_chain",
             "block_fetches", "ext_bytes", "kernel_runs")


@pytest.fixture(scope="module")
def cfg_path(tmp_path_factory):
    p = tmp_path_factory.mktemp("cfg") / CONFIG_BASE
    p.write_text("disable-rules: []\n")
    return str(p)


@pytest.fixture(scope="module")
def analyzer(cfg_path):
    from trivy_amd.analyzer import AnalyzerOptions, SecretAnalyzer, SecretScannerOption
    a = SecretAnalyzer()
    a.Init(AnalyzerOptions(SecretScannerOption(ConfigPath=cfg_path)))
    assert a.tar_walk() == "host" and a.tar_required() == "host"
    a.set_tar_walk("gpu")
    yield a
    a.set_tar_walk("host")
    a.set_tar_required("host")


@pytest.fixture(scope="module")
def oracle(cfg_path):
    return oan.SecretAnalyzer(cfg_path)


def _dev(layer: bytes):
    import torch
    return torch.from_numpy(np.frombuffer(layer + b"\xee" * 64, dtype=np.uint8).copy()).to("cuda:0")


def _secrets(res):
    return [s.to_dict() for s in res.Secrets]


def _both(analyzer, fn):
    """fn() under required host, then gpu."""
    out = []
    for mode in ("host", "gpu"):
        analyzer.set_tar_required(mode)
        try:
            out.append(fn())
        finally:
            analyzer.set_tar_required("host")
    return out


def _same_index(got, want):
    assert got.files() == want.files() and got.start.tolist() == want.start.tolist()
    assert got.data_off.tolist() == want.data_off.tolist() and got.size.tolist() == want.size.tolist()
    for k in STAT_KEYS:
        assert got.stats[k] == want.stats[k], k
    gw, ww = got.walk_stats, want.walk_stats
    for k in ("walk", "fallback", "chain_entries", "name_bytes", "segments"):
        assert gw[k] == ww[k], k


@pytest.mark.parametrize("name", list(LAYERS))
def test_layer_under_both_modes_vs_host_and_oracle(analyzer, oracle, name):
    layer = LAYERS[name]()
    assert len(layer) < 400 << 10
    dev = _dev(layer)
    (ix_h, res_h), (ix_g, res_g) = _both(analyzer, lambda: (analyzer.IndexDevice(dev), analyzer.AnalyzeLayerDevice(dev)))
    _same_index(ix_g, ix_h)
    rh, rg = ix_h.required_stats, ix_g.required_stats
    assert (rh["mode"], rh["reason"]) == ("host", 1) and (rg["mode"], rg["reason"]) == ("gpu", 0)
    assert ix_g.walk_stats["fallback"] == 0
    entries, _, _ = cm.chain(layer)
    recs, names = cm.pack(entries)
    verdicts = rm.stage(recs, len(entries), bytes(names), [0, len(entries)], [0, len(names)], CONFIG_BASE.encode(),
                        *rm.tables_of(analyzer))[0]
    assert rg["entries"] == len(entries)
    assert (rg["kept"], rg["dropped"], rg["ask_allow"], rg["ask_name"]) == tuple(
        int((verdicts == v).sum()) for v in (rm.KEEP, rm.DROP, rm.ASK_ALLOW, rm.ASK_NAME))
    assert rg["kept"] + rg["ask_allow"] + rg["ask_name"] - rg["ask_dropped"] == ix_g.n
    assert rg["ms_kernel"] > 0
    assert _secrets(res_g) == _secrets(res_h)
    host = analyzer.AnalyzeLayer(layer, gpu_transform=True)
    assert _secrets(res_g) == _secrets(host)
    if name == "table":  # (Python's tarfile, which the oracle walks with, does not read its odd names as Go does)
        assert [p for p, _, _ in ix_g.files()] == [t[4] for t in NAME_TABLE if t[4] is not None]
        return
    want = oan.analyze_layer(oracle, layer)
    want.sort(key=lambda s: s["FilePath"].encode("utf-8", "surrogateescape"))
    for s in want:
        s["Findings"].sort(key=lambda f: (f["RuleID"].encode(), f["StartLine"]))
    res_g.Sort()
    assert _secrets(res_g) == want
    req = [(fp, size) for fp, size, _ in oan.walk_layer_tar(layer)[0] if oracle.required(fp, size)]
    assert [(p, s) for p, _, s in ix_g.files()] == req and len(req) >= 1


@pytest.mark.parametrize("name", list(CASES))
def test_complete_cases_under_both_modes(analyzer, name):
    dev = _dev(CASES[name]())
    ix_h, ix_g = _both(analyzer, lambda: analyzer.IndexDevice(dev))
    _same_index(ix_g, ix_h)
    assert ix_g.required_stats["reason"] == 0 and ix_g.required_stats["mode"] == "gpu"


def test_walk_mode_host_is_reason_2(analyzer):
    layer = LAYERS["odd-names"]()
    dev = _dev(layer)
    want = analyzer.AnalyzeLayerDevice(dev)
    analyzer.set_tar_walk("host")
    analyzer.set_tar_required("gpu")
    try:
        ix = analyzer.IndexDevice(dev)
        got = analyzer.AnalyzeLayerDevice(dev)
    finally:
        analyzer.set_tar_required("host")
        analyzer.set_tar_walk("gpu")
    assert (ix.required_stats["mode"], ix.required_stats["reason"]) == ("host", 2)
    assert ix.walk_stats["walk"] == "host" and _secrets(got) == _secrets(want)


def test_skip_options_are_reason_3(analyzer):
    from trivy_amd.walker import NewLayerTar, Option
    layer = LAYERS["ustar"]()
    dev = _dev(layer)
    analyzer.set_layer_walker(NewLayerTar(Option(SkipFiles=["etc/short-2.conf"], SkipDirs=["srv/dir"])))
    try:
        (ix_h, res_h), (ix_g, res_g) = _both(
            analyzer, lambda: (analyzer.IndexDevice(dev), analyzer.AnalyzeLayerDevice(dev)))
    finally:
        analyzer.set_layer_walker(None)
    _same_index(ix_g, ix_h)
    assert (ix_g.required_stats["mode"], ix_g.required_stats["reason"]) == ("host", 3)
    assert ix_g.skip_stats["skipped_files"] == 1 and _secrets(res_g) == _secrets(res_h)
    analyzer.set_tar_required("gpu")
    try:
        assert analyzer.IndexDevice(dev).required_stats["reason"] == 0  # the options are gone: the stage is back
    finally:
        analyzer.set_tar_required("host")


def test_a_layer_the_walk_does_not_complete_is_reason_4(analyzer):
    layer, reason, _ = cm.punt_cases()["17-extension-headers"]
    dev = _dev(layer)
    (ix_h, res_h), (ix_g, res_g) = _both(analyzer, lambda: (analyzer.IndexDevice(dev), analyzer.AnalyzeLayerDevice(dev)))
    _same_index(ix_g, ix_h)
    assert ix_g.walk_stats["fallback"] == reason != 0
    assert (ix_g.required_stats["mode"], ix_g.required_stats["reason"]) == ("host", 4)
    assert ix_h.required_stats["reason"] == 1 and _secrets(res_g) == _secrets(res_h)


def test_three_layers_and_one_that_falls_back_alone(analyzer, oracle):
    punt = cm.punt_cases()["17-extension-headers"][0]
    layers = [LAYERS["ustar"](), LAYERS["table"](), punt, LAYERS["odd-names"]()]
    devs = [_dev(x) for x in layers]
    (ixs_h, res_h), (ixs_g, res_g) = _both(
        analyzer, lambda: (analyzer.IndexLayersDevice(devs), analyzer.AnalyzeLayersDevice(devs)))
    for k in range(4):
        _same_index(ixs_g[k], ixs_h[k])
        assert ixs_g[k].required_stats["reason"] == (4 if k == 2 else 0)
        assert ixs_h[k].required_stats["reason"] == 1
        assert _secrets(res_g[k]) == _secrets(res_h[k])
        alone = analyzer.AnalyzeLayerDevice(devs[k])
        alone.Sort()
        assert _secrets(res_g[k]) == _secrets(alone)
    assert sum(len(r.Secrets) for r in res_g) >= 3
    # as slices of one resident buffer, an empty layer among them
    import torch
    parts, spans, at = [], [], 0
    for x in (layers[0], bytes(1024), layers[3]):
        parts.append(x)
        spans.append((at, len(x)))
        at += len(x)
    buf = torch.from_numpy(np.frombuffer(b"".join(parts) + b"\xee" * 64, dtype=np.uint8).copy()).to("cuda:0")
    slices = [(buf[o:], n) for o, n in spans]
    ixs_h, ixs_g = _both(analyzer, lambda: analyzer.IndexLayersDevice(slices))
    for g, h in zip(ixs_g, ixs_h):
        _same_index(g, h)
        assert g.required_stats["reason"] == 0
    assert ixs_g[1].n == 0 and ixs_g[1].required_stats["entries"] == 0


def test_two_threads_indexing_at_once(analyzer):
    devs = [_dev(LAYERS["table"]()), _dev(LAYERS["boundaries-8"]())]
    want = [analyzer.IndexDevice(d) for d in devs]
    out, errors = [[], []], []
    analyzer.set_tar_required("gpu")

    def work(k):
        try:
            for _ in range(3):
                out[k].append(analyzer.IndexDevice(devs[k]))
                out[k].extend(analyzer.IndexLayersDevice([devs[k], devs[1 - k]])[:1])
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
    try:
        threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    finally:
        analyzer.set_tar_required("host")
    assert not errors, errors
    for k in range(2):
        assert len(out[k]) == 6
        for ix in out[k]:
            _same_index(ix, want[k])
            assert ix.required_stats["reason"] == 0


def test_empty_layers(analyzer):
    analyzer.set_tar_required("gpu")
    try:
        for n in (0, 512, 4096):
            ix = analyzer.IndexDevice(_dev(bytes(n)), nbytes=n)
            assert ix.n == 0 and ix.stats["entries"] == 0 and ix.required_stats["reason"] == 0
    finally:
        analyzer.set_tar_required("host")
