"""A resident tar layer whose skip options are honoured by the GPU's Required stage
(SecretAnalyzer.set_tar_required_skip("gpu"), tsg_analyzer_set_tar_required_skip) end to end: with
the switch on and off the index, its stats and AnalyzeLayerDevice's result equal each other, AnalyzeLayer's of the
same bytes under the same NewLayerTar(Option(...)) and tests/tar_skip_model.py's walk with oracle/analyzer.py's
Required; the stage is in force with patterns it takes (reason 0) and gives way, with the reason, to a pattern
it does not take, to a layer whose asked names hold a skipped directory, and to a layer the GPU walk does not
complete.
"""
import threading

import numpy as np
import pytest

from oracle import analyzer as oan
from tests import tar_chain_model as cm
from tests import tar_skip_model as sm
from tests.test_tar_required_skip_host import LAYERS

pytestmark = pytest.mark.gpu

STAT_KEYS = ("entries", "regular", "required", "whiteouts", "opaque_dirs", "blocks", "candidates", "off_chain",
             "block_fetches", "ext_bytes", "kernel_runs")


@pytest.fixture(scope="module")
def analyzer():
    from trivy_amd.analyzer import AnalyzerOptions, SecretAnalyzer
    a = SecretAnalyzer()
    a.Init(AnalyzerOptions())
    assert a.tar_required_skip() == "host"
    a.set_tar_walk("gpu")
    a.set_tar_required("gpu")
    yield a
    a.set_layer_walker(None)
    a.set_tar_required_skip("host")
    a.set_tar_required("host")
    a.set_tar_walk("host")


@pytest.fixture(scope="module")
def oracle():
    return oan.SecretAnalyzer("")


def _dev(layer: bytes):
    import torch
    return torch.from_numpy(np.frombuffer(layer + b"\xee" * 64, dtype=np.uint8).copy()).to("cuda:0")


def _secrets(res):
    return [s.to_dict() for s in res.Secrets]


def _walker(skip_dirs, skip_files):
    from trivy_amd.walker import NewLayerTar, Option
    return NewLayerTar(Option(SkipFiles=list(skip_files), SkipDirs=list(skip_dirs)))


def _both(analyzer, fn):
    """fn() with the switch off, then on."""
    out = []
    for mode in ("host", "gpu"):
        analyzer.set_tar_required_skip(mode)
        try:
            out.append(fn())
        finally:
            analyzer.set_tar_required_skip("host")
    return out


def _same_index(got, want):
    assert got.files() == want.files() and got.start.tolist() == want.start.tolist()
    assert got.data_off.tolist() == want.data_off.tolist() and got.size.tolist() == want.size.tolist()
    for k in STAT_KEYS:
        assert got.stats[k] == want.stats[k], k
    assert got.skip_stats == want.skip_stats
    gw, ww = got.walk_stats, want.walk_stats
    for k in ("walk", "fallback", "chain_entries", "name_bytes", "segments"):
        assert gw[k] == ww[k], k


def _model_skip(m):
    return {"skipped_dirs": len(m["skipped_dirs"]), "skipped_files": m["skipped_files"],
            "under_skipped_dir": m["under_skipped_dir"]}


@pytest.mark.parametrize("name", list(LAYERS))
def test_layer_with_the_switch_off_and_on_vs_host_and_oracle(analyzer, oracle, name):
    make, skip_dirs, skip_files, falls_back = LAYERS[name]
    layer = make()
    assert len(layer) < 400 << 10
    dev = _dev(layer)
    analyzer.set_layer_walker(_walker(skip_dirs, skip_files))
    try:
        (ix_h, res_h), (ix_g, res_g) = _both(
            analyzer, lambda: (analyzer.IndexDevice(dev), analyzer.AnalyzeLayerDevice(dev)))
        host = analyzer.AnalyzeLayer(layer, gpu_transform=True)
    finally:
        analyzer.set_layer_walker(None)
    _same_index(ix_g, ix_h)
    rh, rg, sh, sg = ix_h.required_stats, ix_g.required_stats, ix_h.required_skip_stats, ix_g.required_skip_stats
    # the switch off is the behaviour before it existed: reason 3, the host half
    assert (rh["mode"], rh["reason"]) == ("host", 3) and (sh["mode"], sh["reason"]) == ("host", 1)
    if falls_back:
        assert (rg["mode"], rg["reason"]) == ("host", 5) and (sg["mode"], sg["reason"]) == ("gpu", 5)
    else:
        assert (rg["mode"], rg["reason"]) == ("gpu", 0) and (sg["mode"], sg["reason"]) == ("gpu", 0)
        assert rg["entries"] == len(cm.chain(layer)[0]) and sg["ms_kernel"] > 0
        assert rg["kept"] + rg["ask_allow"] + rg["ask_name"] - rg["ask_dropped"] == ix_g.n
        assert (sg["table_slots"] > 0) == (sg["skipped_dirs"] > 0)
    assert (sg["dir_patterns"], sg["file_patterns"]) == (len(skip_dirs), len(skip_files))
    m = sm.walk(layer, skip_dirs, skip_files)
    assert ix_g.skip_stats == _model_skip(m) == {k: sg[k] for k in _model_skip(m)}
    assert [(p, s) for p, _, s in ix_g.files()] == [(fp, size) for fp, size, _ in m["kept"] if oracle.required(fp, size)]
    assert ix_g.stats["regular"] == m["regular"]
    assert _secrets(res_g) == _secrets(res_h) == _secrets(host)
    want = sm.sort_secrets(sm.analyze(oracle, layer, skip_dirs, skip_files))
    res_g.Sort()
    assert _secrets(res_g) == want


def test_one_refused_pattern_is_reason_3_and_removing_the_options_restores_the_stage(analyzer):
    make, skip_dirs, skip_files, _ = LAYERS["dir-after-files-and-twice"]
    dev = _dev(make())
    analyzer.set_layer_walker(_walker(skip_dirs + ["app/*/nothing"], skip_files))
    try:
        (ix_h, res_h), (ix_g, res_g) = _both(
            analyzer, lambda: (analyzer.IndexDevice(dev), analyzer.AnalyzeLayerDevice(dev)))
        _same_index(ix_g, ix_h)
        assert (ix_g.required_stats["mode"], ix_g.required_stats["reason"]) == ("host", 3)
        assert (ix_g.required_skip_stats["mode"], ix_g.required_skip_stats["reason"]) == ("gpu", 3)
        assert ix_g.skip_stats["under_skipped_dir"] >= 2 and _secrets(res_g) == _secrets(res_h)
        analyzer.set_layer_walker(_walker(skip_dirs, skip_files))  # the accepted ones alone: the stage runs
        analyzer.set_tar_required_skip("gpu")
        ix = analyzer.IndexDevice(dev)
        assert ix.required_stats["reason"] == 0 and ix.required_skip_stats["reason"] == 0
        _same_index(ix, ix_h)
        analyzer.set_layer_walker(None)  # no options: the switch has no effect, the stage runs as it always did
        ix_on = analyzer.IndexDevice(dev)
        analyzer.set_tar_required_skip("host")
        ix_off = analyzer.IndexDevice(dev)
        _same_index(ix_on, ix_off)
        for ix in (ix_on, ix_off):
            assert (ix.required_stats["mode"], ix.required_stats["reason"]) == ("gpu", 0)
            assert ix.skip_stats == {"skipped_dirs": 0, "skipped_files": 0, "under_skipped_dir": 0}
        assert ix_on.required_skip_stats["reason"] == 2 and ix_off.required_skip_stats["reason"] == 1
        assert ix_on.n > ix_h.n
    finally:
        analyzer.set_tar_required_skip("host")
        analyzer.set_layer_walker(None)


def test_required_off_or_walk_host_is_skip_reason_4(analyzer):
    make, skip_dirs, skip_files, _ = LAYERS["file-is-direct-parent"]
    dev = _dev(make())
    analyzer.set_layer_walker(_walker(skip_dirs, skip_files))
    analyzer.set_tar_required_skip("gpu")
    try:
        want = analyzer.IndexDevice(dev)
        assert want.required_skip_stats["reason"] == 0
        analyzer.set_tar_required("host")
        ix = analyzer.IndexDevice(dev)
        assert ix.required_stats["reason"] == 1 and ix.required_skip_stats["reason"] == 4
        _same_index(ix, want)
        analyzer.set_tar_required("gpu")
        analyzer.set_tar_walk("host")
        ix = analyzer.IndexDevice(dev)
        assert ix.required_stats["reason"] == 2 and ix.required_skip_stats["reason"] == 4
        assert ix.files() == want.files() and ix.skip_stats == want.skip_stats
    finally:
        analyzer.set_tar_walk("gpu")
        analyzer.set_tar_required("gpu")
        analyzer.set_tar_required_skip("host")
        analyzer.set_layer_walker(None)


def test_layers_in_one_pass_with_one_falling_back_alone(analyzer, oracle):
    """Three layers with the same names of which only the middle one records the directory, the layer whose asked
    name is a skipped directory (reason 5, alone), and a layer the GPU walk does not complete (reason 4, alone)."""
    skip_dirs, skip_files = ["**/skipme"], ["**/*.pem"]
    same = LAYERS["dir-after-files-and-twice"][0]()
    no_dir = same.replace(cm.member(b"app/skipme/", b"", b"5"), cm.member(b"app/skipme/", b"", b"2")).replace(
        cm.member(b"app/skipme", b"", b"5"), cm.member(b"app/skipme", b"", b"2")).replace(
        cm.member(b"./app/skipme/", b"", b"\0"), cm.member(b"./app/skipme/", b"", b"2"))
    assert len(no_dir) == len(same) and no_dir != same
    punt = cm.punt_cases()["17-extension-headers"][0]
    layers = [no_dir, same, no_dir, LAYERS["asked-dir-matches"][0](), punt, LAYERS["asked-names"][0]()]
    devs = [_dev(x) for x in layers]
    analyzer.set_layer_walker(_walker(skip_dirs, skip_files))
    try:
        (ixs_h, res_h), (ixs_g, res_g) = _both(
            analyzer, lambda: (analyzer.IndexLayersDevice(devs), analyzer.AnalyzeLayersDevice(devs)))
        analyzer.set_tar_required_skip("gpu")
        alone = [analyzer.AnalyzeLayerDevice(d) for d in devs]
        # as slices of one resident buffer, an empty layer among them
        import torch
        parts, spans, at = [], [], 0
        for x in (layers[1], bytes(1024), layers[5], layers[0]):
            parts.append(x)
            spans.append((at, len(x)))
            at += len(x)
        buf = torch.from_numpy(np.frombuffer(b"".join(parts) + b"\xee" * 64, dtype=np.uint8).copy()).to("cuda:0")
        sliced = analyzer.IndexLayersDevice([(buf[o:], n) for o, n in spans])
    finally:
        analyzer.set_tar_required_skip("host")
        analyzer.set_layer_walker(None)
    for k in range(len(layers)):
        _same_index(ixs_g[k], ixs_h[k])
        assert ixs_h[k].required_stats["reason"] == 3  # (the options come before the walk's outcome, as ever)
        assert ixs_g[k].required_stats["reason"] == {3: 5, 4: 4}.get(k, 0)
        assert ixs_g[k].required_skip_stats["reason"] == {3: 5, 4: 4}.get(k, 0)
        assert _secrets(res_g[k]) == _secrets(res_h[k])
        alone[k].Sort()
        assert _secrets(res_g[k]) == _secrets(alone[k])
        if k == 4:  # (Python's tarfile, which the model walks with, does not read that layer)
            continue
        m = sm.walk(layers[k], skip_dirs, skip_files)
        assert ixs_g[k].skip_stats == _model_skip(m)
        assert [(p, s) for p, _, s in ixs_g[k].files()] == [(fp, size) for fp, size, _ in m["kept"]
                                                             if oracle.required(fp, size)]
    assert ixs_g[0].skip_stats["under_skipped_dir"] == 0 and ixs_g[1].skip_stats["under_skipped_dir"] >= 3
    assert ixs_g[0].files() == ixs_g[2].files() and ixs_g[0].n > ixs_g[1].n
    for g, k in zip(sliced, (1, None, 5, 0)):
        assert g.required_stats["reason"] == 0 and g.required_skip_stats["reason"] == 0
        if k is None:
            assert g.n == 0 and g.required_stats["entries"] == 0
        else:
            assert g.files() == ixs_g[k].files() and g.skip_stats == ixs_g[k].skip_stats


def test_two_threads_indexing_at_once(analyzer):
    names = ["dir-after-files-and-twice", "asked-names"]
    devs = [_dev(LAYERS[n][0]()) for n in names]
    analyzer.set_layer_walker(_walker(["**/skipme"], ["**/*.pem"]))
    out, errors = [[], []], []
    try:
        want = [analyzer.IndexDevice(d) for d in devs]  # the switch off: the host half
        analyzer.set_tar_required_skip("gpu")

        def work(k):
            try:
                for _ in range(3):
                    out[k].append(analyzer.IndexDevice(devs[k]))
                    out[k].extend(analyzer.IndexLayersDevice([devs[k], devs[1 - k]])[:1])
            except BaseException as e:  # noqa: BLE001
                errors.append(e)
        threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    finally:
        analyzer.set_tar_required_skip("host")
        analyzer.set_layer_walker(None)
    assert not errors, errors
    for k in range(2):
        assert len(out[k]) == 6 and want[k].required_stats["reason"] == 3
        for ix in out[k]:
            _same_index(ix, want[k])
            assert ix.required_stats["reason"] == 0 and ix.required_skip_stats["reason"] == 0
