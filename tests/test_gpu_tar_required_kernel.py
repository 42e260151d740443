"""The device stage that classifies the paths of a resident layer's entries and runs Required
(trivy_amd/csrc/tarrequired.hip) alone, through tsg_debug_tar_required, against the pure-Python model
(tests/tar_required_model.py): every byte of every output -- the verdict per entry, the 48-B file records, the
path blob, the counts per layer.  The model itself is checked against a table of expected verdicts, the host
half and the oracle in tests/test_tar_required_host.py.
"""
import ctypes as c
import random

import numpy as np
import pytest

from tests import tar_chain_model as cm
from tests import tar_required_model as rm
from tests.test_tar_required_host import CONFIG_BASE, NAME_TABLE, TEXT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from trivy_amd.analyzer import AnalyzerOptions, SecretAnalyzer, SecretScannerOption
    cfg = tmp_path_factory.mktemp("cfg") / CONFIG_BASE
    cfg.write_text("disable-rules: []\n")
    a = SecretAnalyzer()
    a.Init(AnalyzerOptions(SecretScannerOption(ConfigPath=str(cfg))))
    a._L.tsg_debug_tar_required.argtypes = [c.c_void_p, c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint64, c.c_void_p,
                                            c.c_void_p, c.c_uint32, c.c_uint32, c.c_void_p, c.c_void_p, c.c_uint64,
                                            c.POINTER(c.c_uint64), c.c_void_p, c.c_uint64, c.POINTER(c.c_uint64),
                                            c.c_void_p]
    pt, st = rm.tables_of(a)
    assert pt is not None and st is not None
    return a, pt, st


def _entries(names, seed=0):
    """Entry records as the chain walk writes them, for (name, typeflag, size) triples."""
    rng = random.Random(seed)
    out, at = [], 0
    for name, typeflag, size in names:
        n_ext = rng.randrange(3)
        out.append(dict(start=at, hdr=at + 1024 * n_ext, data=at + 1024 * n_ext + 512, size=size, name=name,
                        typeflag=typeflag, flags=0, n_ext=n_ext))
        at += 1024 * n_ext + 512 + (size + 511) // 512 * 512
    return out


def _from_table(n, seed):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        name, typeflag, size, _, _ = rng.choice(NAME_TABLE)
        out.append((name, typeflag[0], len(TEXT) if size is None else size))
    return out


def _run(a, recs, n, names, rec_base, name_base, grid_cap):
    """The hook's (rc, verdicts, file records, blob, counts); the outputs sit in buffers pre-filled with 0xA5
    and sized exactly, so a byte written past the counted sizes is seen."""
    n_layers = len(rec_base) - 1
    rb, nb = np.array(rec_base, dtype=np.uint64), np.array(name_base, dtype=np.uint64)
    verdicts = np.full(max(n, 1), 0xA5, dtype=np.uint8)
    frecs = np.full(48 * n + 64, 0xA5, dtype=np.uint8)
    blob = np.full(len(names) + n + 64, 0xA5, dtype=np.uint8)
    counts = np.zeros((n_layers, 16), dtype=np.uint64)
    n_f, n_b = c.c_uint64(), c.c_uint64()
    nm = np.frombuffer(bytes(names) or b"\0", dtype=np.uint8)
    rc = a._L.tsg_debug_tar_required(a._h, recs.ctypes.data if n else None, n, nm.ctypes.data if len(names) else None,
                                     len(names), rb.ctypes.data, nb.ctypes.data, n_layers, grid_cap, verdicts.ctypes.data,
                                     frecs.ctypes.data, n, c.byref(n_f), blob.ctypes.data, len(names) + n, c.byref(n_b),
                                     counts.ctypes.data)
    assert (frecs[48 * n_f.value:] == 0xA5).all() and (blob[n_b.value:] == 0xA5).all()
    return rc, verdicts[:n], bytes(frecs[:48 * n_f.value]), bytes(blob[:n_b.value]), counts


_model_cache = {}


def _check(setup, layers, grid_cap, want_rc=0):
    """layers: lists of entries; one stage over all of them against the model."""
    a, pt, st = setup
    recs_l, names_l, rec_base, name_base = [], [], [0], [0]
    for entries in layers:
        r, nm = cm.pack(entries)
        recs_l.append(bytes(r))
        names_l.append(bytes(nm))
        rec_base.append(rec_base[-1] + len(entries))
        name_base.append(name_base[-1] + len(nm))
    recs = np.frombuffer(b"".join(recs_l) or b"\0", dtype=np.uint8).copy()
    names = b"".join(names_l)
    n = rec_base[-1]
    key = (bytes(recs[:64 * n]), names, tuple(rec_base))
    if key not in _model_cache:  # (the model runs once per input, whatever the grid)
        _model_cache[key] = rm.stage(recs, n, names, rec_base, name_base, CONFIG_BASE.encode(), pt, st)
    want = _model_cache[key]
    rc, verdicts, frecs, blob, counts = _run(a, recs, n, names, rec_base, name_base, grid_cap)
    assert rc == want_rc
    assert verdicts.tolist() == want[0].tolist()
    assert counts.tolist() == want[3].tolist()
    assert frecs == want[1] and blob == want[2]
    return want


@pytest.mark.parametrize("grid_cap", [1, 0])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 5000])
def test_names_drawn_from_the_table(setup, n, grid_cap):
    want = _check(setup, [_entries(_from_table(n, n), n)], grid_cap)
    if n >= 257:
        assert len(set(want[0].tolist())) == 7  # every verdict but the bad one


@pytest.mark.parametrize("grid_cap", [1, 0])
def test_the_whole_table_in_order(setup, grid_cap):
    names = [(name, typeflag[0], len(TEXT) if size is None else size) for name, typeflag, size, _, _ in NAME_TABLE]
    want = _check(setup, [_entries(names)], grid_cap)
    assert want[0].tolist() == [t[3] for t in NAME_TABLE]


@pytest.mark.parametrize("grid_cap", [1, 0])
def test_name_lengths(setup, grid_cap):
    names = []
    for ln in (1, 15, 16, 17, 255, 256, 65536):
        body = (b"dir/" * (ln // 4 + 1))[:ln - 1] + b"f" if ln > 1 else b"f"
        assert len(body) == ln
        names += [(body, 0x30, 61), (b"./" + body[2:], 0x30, 61) if ln > 2 else (body, 0, 61),
                  (body[:-1] + b"/", 0x30, 61) if ln > 1 else (b"/", 0x35, 0),
                  ((b"a//" + body)[:ln], 0x30, 61), ((b"example/" + body)[:ln], 0x30, 61),
                  ((b"vendor-" * (ln // 7 + 1))[:ln - 1] + b"\xc3", 0x30, 61) if ln > 1 else (b"\xc3", 0x30, 61)]
    want = _check(setup, [_entries(names)], grid_cap)
    assert {rm.KEEP, rm.DROP, rm.ASK_ALLOW, rm.ASK_NAME} <= set(want[0].tolist())


@pytest.mark.parametrize("grid_cap", [1, 0])
def test_three_layers_with_an_empty_one_in_the_middle(setup, grid_cap):
    first, last = _entries(_from_table(70, 1), 1), _entries(_from_table(130, 2), 2)
    want = _check(setup, [first, [], last], grid_cap)
    cnt = {k: want[3][:, i].tolist() for i, k in enumerate(rm.COUNTS)}
    assert cnt["entries"] == [70, 0, 130] and cnt["records"][1] == 0 and cnt["path_bytes"][1] == 0
    assert cnt["rec_first"] == [0, cnt["records"][0], cnt["records"][0]]
    # each layer's slice is what the stage gives for that layer alone
    for k, entries in ((0, first), (2, last)):
        alone = _check(setup, [entries], grid_cap)
        r0, p0 = cnt["rec_first"][k], cnt["path_first"][k]
        assert want[1][48 * r0:48 * (r0 + cnt["records"][k])] == alone[1]
        assert want[2][p0:p0 + cnt["path_bytes"][k]] == alone[2]
    _check(setup, [[], first, []], grid_cap)
    _check(setup, [[], []], grid_cap)


@pytest.mark.parametrize("grid_cap", [1, 0])
def test_a_record_outside_its_blob_is_reported_and_not_read(setup, grid_cap):
    """The name of layer 0's last record runs one byte into layer 1's names, another starts past its layer's
    end, a third has a length of 2^32 - 1: verdict 7 each, the call says so, the rest is decided as usual."""
    a, pt, st = setup
    first, last = _entries(_from_table(40, 3), 3), _entries(_from_table(40, 4), 4)
    layers = [first, last]
    recs_l, names_l, rec_base, name_base = [], [], [0], [0]
    for entries in layers:
        r, nm = cm.pack(entries)
        recs_l.append(bytearray(bytes(r)))
        names_l.append(bytes(nm))
        rec_base.append(rec_base[-1] + len(entries))
        name_base.append(name_base[-1] + len(nm))
    off, ln = cm.REC.unpack(bytes(recs_l[0][64 * 39:64 * 40]))[4:6]
    recs_l[0][64 * 39 + 40:64 * 39 + 44] = int(ln + (len(names_l[0]) - off - ln) + 1).to_bytes(4, "little")
    recs_l[1][64 * 5 + 32:64 * 5 + 40] = int(len(names_l[1]) + 1).to_bytes(8, "little")
    recs_l[1][64 * 9 + 40:64 * 9 + 44] = (0xFFFFFFFF).to_bytes(4, "little")
    recs = np.frombuffer(bytes(recs_l[0] + recs_l[1]), dtype=np.uint8).copy()
    names = b"".join(names_l)
    want = rm.stage(recs, 80, names, rec_base, name_base, CONFIG_BASE.encode(), pt, st)
    assert [i for i, v in enumerate(want[0]) if v == rm.BAD] == [39, 45, 49]
    rc, verdicts, frecs, blob, counts = _run(a, recs, 80, names, rec_base, name_base, grid_cap)
    from trivy_amd import _lib
    assert rc == -4 and "outside" in _lib.last_error(a._L)
    assert verdicts.tolist() == want[0].tolist() and counts.tolist() == want[3].tolist()
    assert frecs == want[1] and blob == want[2]
    assert counts[:, rm.COUNTS.index("bad")].tolist() == [1, 2]


def test_argument_errors(setup):
    a, _, _ = setup
    L = a._L
    z = np.zeros(4, dtype=np.uint64)
    n_f, n_b = c.c_uint64(), c.c_uint64()
    assert L.tsg_debug_tar_required(None, None, 0, None, 0, z.ctypes.data, z.ctypes.data, 1, 0, None, None, 0,
                                    c.byref(n_f), None, 0, c.byref(n_b), z.ctypes.data) == -2
    assert L.tsg_debug_tar_required(a._h, None, 0, None, 0, z.ctypes.data, z.ctypes.data, 0, 0, None, None, 0,
                                    c.byref(n_f), None, 0, c.byref(n_b), z.ctypes.data) == -2
    bad = np.array([0, 5], dtype=np.uint64)  # the table does not end at n_records
    assert L.tsg_debug_tar_required(a._h, None, 0, None, 0, bad.ctypes.data, z.ctypes.data, 1, 0, None, None, 0,
                                    c.byref(n_f), None, 0, c.byref(n_b), z.ctypes.data) == -2
