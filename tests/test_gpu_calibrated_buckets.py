"""The GPU stages on tables whose windows and buckets a calibration sample chose.

One 1-MiB batch of tests/stage_cases.py (tokens around every kind of boundary), scanned by an
engine compiled with a 1-MiB sample.  The smallest shape that can go wrong is a bucket of more
than 8 items (two core groups per fire in K2's phase B) together with an item whose window is
not the prior's choice (another `back`): the sample is picked so that both occur, and the test
asserts that they do.  Then invariants 2 (flagged blocks), 3 (hits) and 6 (coverage) of
tests/stage_model.py, the tables staged in LDS, and the scanner's findings against the oracle.
"""
import random

import numpy as np
import pytest

from tests import stage_cases as sc
from tests import stage_model as sm
from tests.filter_model import FilterModel
from tests.test_filter_model import _calibration_sample

pytestmark = pytest.mark.gpu

_STATE = {}


def _sample():
    return _calibration_sample(0)[:1 << 20]


def _case():
    if "case" not in _STATE:
        body, n = sc.boundary_file(n_bytes=(1 << 20) - 4096)
        small = [b"", sc.filler(100) + sc.tok_ghp(random.Random(2)) + b"\n", b"x",
                 b"heroku_key = '0A1B2C3D-1111-2222-3333-0A1B2C3D4E5F'\n"]
        case = {"rules": sc.builtin_rules(), "batch": sm.Batch([body] + small), "calibration": _sample(), "n": n}
        assert (1 << 20) - 4096 < case["batch"].n_bytes <= 1 << 20
        _STATE["case"] = case
    return _STATE["case"]


def test_stages_with_measured_buckets(monkeypatch, capfd):
    case = _case()
    b = case["batch"]
    model = sc.model_of(case, monkeypatch)
    fm = model.fm
    with monkeypatch.context() as m:
        m.setenv("TSG_CALIB_BUCKETS", "0")
        prior = FilterModel(case["rules"], calibration=case["calibration"])
    sizes = np.diff(fm.bucket_off)
    moved = [i for i, (x, y) in enumerate(zip(fm.items, prior.items)) if x["back"] != y["back"]]
    print("bucket sizes %s, windows that differ from the prior's: items %s" % (list(map(int, sizes)), moved))
    assert sizes.max() > 8 and moved
    e = model.expect(b)
    matches = model.true_matches(b)
    with monkeypatch.context() as m:
        m.setenv("TSG_ENGINE_DEBUG", "1")
        d = sm.run_engine(model, b)
    err = capfd.readouterr().err
    assert "LDS tables" in err, err[-400:]  # confirm_kernel<true>: the item tables fit its LDS variant
    sm.check_overflow(d)
    sm.check_blocks(d, e)
    sm.check_hits(d, e, b)
    n = sm.check_coverage(d, model, b, matches)
    big = {j for j in range(fm.n_buckets - 1) if sizes[j] > 8}
    fired = fm.fires(b.a)
    print("blocks %d hits %d candidates %d matches %d, fires in buckets of two groups %d"
          % (len(d.recs), len(d.hits), len(d.cands), n, int(fired[sorted(big)].sum())))
    assert len(d.hits) >= case["n"] and n >= case["n"]
    assert fired[sorted(big)].any()  # phase B walked a second core group


def test_findings_equal_oracle():
    from oracle import secret_scanner as osc
    import trivy_amd.secret as secret
    b = _case()["batch"]
    args = [secret.ScanArgs(FilePath="dir/f%d.txt" % i, Content=x) for i, x in enumerate(b.contents)]
    scn = secret.NewScanner(None, device=0, calibration=_sample())
    got = scn.ScanBatch(args)
    ref = osc.new_scanner(None)
    n = 0
    for a, g in zip(args, got):
        want = ref.scan(a.FilePath, a.Content)
        assert g.to_dict() == want, a.FilePath
        n += len(want["Findings"] or [])
    print("findings %d" % n)
    assert n >= 100
