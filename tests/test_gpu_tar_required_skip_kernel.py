"""The Required stage of a resident layer with its skip stage (trivy_amd/csrc/tarrequired.hip: the match, build
and under kernels between the decisions and the sums) alone, through tsg_debug_tar_required_skip, against the
pure-Python model (tests/tar_required_skip_model.py): every byte of every output -- the verdict per entry, the
48-B file records, the path blob, the counts per layer.  The model's matcher and under rule are checked against
doublestar.Match and tar.go's underSkippedDir in tests/test_tar_required_skip_host.py.
"""
import ctypes as c
import random

import numpy as np
import pytest

from tests import tar_chain_model as cm
from tests import tar_required_model as rm
from tests import tar_required_skip_model as km
from tests.test_tar_required_host import CONFIG_BASE, NAME_TABLE, TEXT

pytestmark = pytest.mark.gpu

SKIP_DIRS = ["**/skipme", "t3/**", "t5/s2", "old/regadir", "**/a/b"]
SKIP_FILES = ["**/*.pem", "t0/s0/f7.conf", "**/x.wh.y", "size10", "etc/**"]


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from trivy_amd.analyzer import AnalyzerOptions, SecretAnalyzer, SecretScannerOption
    cfg = tmp_path_factory.mktemp("cfg") / CONFIG_BASE
    cfg.write_text("disable-rules: []\n")
    a = SecretAnalyzer()
    a.Init(AnalyzerOptions(SecretScannerOption(ConfigPath=str(cfg))))
    a._L.tsg_debug_tar_required_skip.argtypes = [
        c.c_void_p, c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint64, c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32,
        c.POINTER(c.c_char_p), c.c_uint32, c.POINTER(c.c_char_p), c.c_uint32, c.c_uint64,
        c.c_void_p, c.c_void_p, c.c_uint64, c.POINTER(c.c_uint64), c.c_void_p, c.c_uint64, c.POINTER(c.c_uint64),
        c.c_void_p, c.POINTER(c.c_uint64)]
    pt, st = rm.tables_of(a)
    assert pt is not None and st is not None
    return a, pt, st


def _entries(names, seed=0):
    """Entry records as the chain walk writes them, for (name, typeflag, size) triples: the starts ascend."""
    rng = random.Random(seed)
    out, at = [], 0
    for name, typeflag, size in names:
        n_ext = rng.randrange(3)
        out.append(dict(start=at, hdr=at + 1024 * n_ext, data=at + 1024 * n_ext + 512, size=size, name=name,
                        typeflag=typeflag, flags=0, n_ext=n_ext))
        at += 1024 * n_ext + 512 + (size + 511) // 512 * 512
    return out


def _tree(n, seed, n_units=8):
    """n names: files and directories of a small tree that the patterns cut in every way, names of the
    Required table (markers, names the device does not clean), in random order -- a directory's entry comes
    before some of its files and after others."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        t, s, f = rng.randrange(n_units), rng.randrange(4), rng.randrange(12)
        k = rng.randrange(12)
        if k == 0:
            name, typeflag, size, _, _ = rng.choice(NAME_TABLE)
            out.append((name, typeflag[0], len(TEXT) if size is None else size))
        elif k == 1:
            out.append((b"t%d/s%d" % (t, s) + rng.choice((b"", b"/", b"//")), 0x35, 0))
        elif k == 2:
            out.append((rng.choice((b"", b"./", b"/")) + b"t%d/s%d/skipme" % (t, s) + rng.choice((b"", b"/")),
                        rng.choice((0x35, 0x35, 0x32)), 0))
        elif k == 3:
            out.append((b"t%d/skipme/" % t, 0, 0))  # a '\0' entry whose name ends in '/'
        elif k == 4:
            out.append((b"t%d/s%d/k%d.pem" % (t, s, f), 0x30, 61))
        elif k == 5:
            out.append((b"t%d/s%d/skipme/f%d.conf" % (t, s, f), 0x30, rng.choice((61, 5))))
        elif k == 6:
            out.append((b"t%d/skipme/deep/er/f%d.conf" % (t, f), 0x30, 61))
        elif k == 7:
            out.append((rng.choice((b"t%d/s%d" % (t, s), b"t%d" % t, b"t%d/skipme" % t, b"t%d/s%d/skipme" % (t, s))),
                        0x30, 61))  # a file named as a directory, or as the parent of one
        elif k == 8:
            out.append((b"t%d/./s%d/skipme/asked%d.conf" % (t, s, f), 0x30, 61))
        else:
            out.append((b"t%d/s%d/f%d.conf" % (t, s, f), 0x30, 61))
    return out


def _run(a, recs, n, names, rec_base, name_base, grid_cap, dirs, files, slots=0):
    """The hook's (rc, verdicts, file records, blob, counts, slots); the outputs sit in buffers pre-filled with
    0xA5 and sized exactly, so a byte written past the counted sizes is seen."""
    n_layers = len(rec_base) - 1
    rb, nb = np.array(rec_base, dtype=np.uint64), np.array(name_base, dtype=np.uint64)
    verdicts = np.full(max(n, 1), 0xA5, dtype=np.uint8)
    frecs = np.full(48 * n + 64, 0xA5, dtype=np.uint8)
    blob = np.full(len(names) + n + 64, 0xA5, dtype=np.uint8)
    counts = np.zeros((n_layers, 16), dtype=np.uint64)
    n_f, n_b, n_s = c.c_uint64(), c.c_uint64(), c.c_uint64(77)
    nm = np.frombuffer(bytes(names) or b"\0", dtype=np.uint8)
    d = (c.c_char_p * max(1, len(dirs)))(*[p.encode() for p in dirs])
    f = (c.c_char_p * max(1, len(files)))(*[p.encode() for p in files])
    rc = a._L.tsg_debug_tar_required_skip(
        a._h, recs.ctypes.data if n else None, n, nm.ctypes.data if len(names) else None, len(names), rb.ctypes.data,
        nb.ctypes.data, n_layers, grid_cap, d, len(dirs), f, len(files), slots, verdicts.ctypes.data, frecs.ctypes.data, n,
        c.byref(n_f), blob.ctypes.data, len(names) + n, c.byref(n_b), counts.ctypes.data, c.byref(n_s))
    assert (frecs[48 * n_f.value:] == 0xA5).all() and (blob[n_b.value:] == 0xA5).all()
    return rc, verdicts[:n], bytes(frecs[:48 * n_f.value]), bytes(blob[:n_b.value]), counts, n_s.value


_model_cache = {}


def _pack(layers):
    recs_l, names_l, rec_base, name_base = [], [], [0], [0]
    for entries in layers:
        r, nm = cm.pack(entries)
        recs_l.append(bytes(r))
        names_l.append(bytes(nm))
        rec_base.append(rec_base[-1] + len(entries))
        name_base.append(name_base[-1] + len(nm))
    return np.frombuffer(b"".join(recs_l) or b"\0", dtype=np.uint8).copy(), b"".join(names_l), rec_base, name_base


def _check(setup, layers, grid_cap, dirs=SKIP_DIRS, files=SKIP_FILES, slots=0):
    """layers: lists of entries; one stage over all of them against the model.  slots: "min" forces the smallest
    table the hook takes.  Returns (the model's outputs, the slots used)."""
    a, pt, st = setup
    recs, names, rec_base, name_base = _pack(layers)
    n = rec_base[-1]
    key = (bytes(recs[:64 * n]), names, tuple(rec_base), tuple(dirs), tuple(files))
    if key not in _model_cache:  # (the model runs once per input, whatever the grid and the table)
        _model_cache[key] = km.stage(recs, n, names, rec_base, name_base, CONFIG_BASE.encode(), pt, st,
                                     [p.encode() for p in dirs], [p.encode() for p in files])
    want = _model_cache[key]
    n_dirs = int((want[0] == km.SKIP_DIR).sum())
    if slots == "min":
        slots = 1
        while slots < 4 * n_dirs:
            slots *= 2
    rc, verdicts, frecs, blob, counts, used = _run(a, recs, n, names, rec_base, name_base, grid_cap, dirs, files, slots)
    from trivy_amd import _lib
    assert rc == 0, _lib.last_error(a._L)
    assert verdicts.tolist() == want[0].tolist()
    assert counts.tolist() == want[3].tolist()
    assert frecs == want[1] and blob == want[2]
    if n_dirs == 0:
        assert used == 0  # the build and under kernels did not run
    else:
        assert used == (slots or used) and used >= 4 * n_dirs and used & (used - 1) == 0
        if not slots:
            assert used < 16 * n_dirs or used == 8
    return want, used


@pytest.mark.parametrize("grid_cap", [1, 0])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 5000])
def test_names_drawn_from_the_tree(setup, n, grid_cap):
    want, _ = _check(setup, [_entries(_tree(n, n), n)], grid_cap)
    if n >= 257:
        assert {km.SKIP_DIR, km.SKIP_FILE, km.SKIP_UNDER, rm.ASK_NAME, rm.KEEP, rm.DROP} <= set(want[0].tolist())
    if n == 5000:
        assert set(want[0].tolist()) == set(range(11)) - {rm.BAD}  # every verdict but the bad one
        _check(setup, [_entries(_tree(n, n), n)], grid_cap, slots="min")


@pytest.mark.parametrize("grid_cap", [1, 0])
@pytest.mark.parametrize("n_dirs", [0, 1, 1000])
def test_recorded_directories(setup, n_dirs, grid_cap):
    """n_dirs directories u<j>/skipme, each with a file before it, one under it, one beside it and one that is its
    direct parent's name sake; with the smallest table too, where the probe sequences are longest."""
    rng = random.Random(n_dirs)
    names = []
    for j in range(max(n_dirs, 3)):
        if j < n_dirs:
            names.append((b"u%d/skipme" % j, 0x35, 0))
        names += [(b"u%d/skipme/in.conf" % j, 0x30, 61), (b"u%d/beside.conf" % j, 0x30, 61), (b"u%d" % j, 0x30, 61),
                  (b"u%d/skipme" % j, 0x30, 61)]
    rng.shuffle(names)
    for slots in (0, "min"):
        want, used = _check(setup, [_entries(names, n_dirs)], grid_cap, dirs=["**/skipme"], files=["**/*.pem"], slots=slots)
        assert int((want[0] == km.SKIP_DIR).sum()) == n_dirs
        if n_dirs == 1000:
            assert used == (4096 if slots else 8192)
            assert 500 < int((want[0] == km.SKIP_UNDER).sum()) < 3000
    if n_dirs == 0:
        assert not (want[0] == km.SKIP_UNDER).any()


def test_forced_table_sizes_the_hook_refuses(setup):
    a, pt, st = setup
    names = [(b"u%d/skipme" % j, 0x35, 0) for j in range(5)] + [(b"u1/skipme/f.conf", 0x30, 61)]
    recs, blob, rec_base, name_base = _pack([_entries(names)])
    from trivy_amd import _lib
    for slots in (3, 16, 24, 1 << 32):  # no power of two; below 4 x 5; no power of two; above 2^31
        rc = _run(a, recs, 6, blob, rec_base, name_base, 0, ["**/skipme"], [], slots)[0]
        assert rc == -1 and "table_slots %d" % slots in _lib.last_error(a._L)
    assert _run(a, recs, 6, blob, rec_base, name_base, 0, ["**/skipme"], [], 32)[0] == 0
    # patterns the device does not take, and none at all
    assert _run(a, recs, 6, blob, rec_base, name_base, 0, ["a/*/b"], [], 0)[0] == -1
    assert _run(a, recs, 6, blob, rec_base, name_base, 0, [], [], 0)[0] == -1


@pytest.mark.parametrize("grid_cap", [1, 0])
def test_a_path_with_100_ancestors(setup, grid_cap):
    deep = b"/".join(b"a%d" % k for k in range(100))
    for at in (1, 50, 100, None):  # which ancestor is the recorded directory
        names = [(deep + b"/early.conf", 0x30, 61)]
        if at is not None:
            names.append((b"/".join(b"a%d" % k for k in range(at)) + b"/", 0x35, 0))
        names += [(deep + b"/f.conf", 0x30, 61), (deep, 0x30, 61), (b"a0x/f.conf", 0x30, 61)]
        pat = "a0/**" if at == 1 else "**/a49" if at == 50 else "**/a98/a99"
        want, _ = _check(setup, [_entries(names)], grid_cap, dirs=[pat], files=[])
        v = want[0].tolist()
        if at is None:
            assert km.SKIP_UNDER not in v and km.SKIP_DIR not in v
        else:
            assert v[0] != km.SKIP_UNDER and v[1] == km.SKIP_DIR and v[2] == km.SKIP_UNDER and v[4] != km.SKIP_UNDER
            assert v[3] == km.SKIP_UNDER  # (below the directory, or at 100 the file named as the directory itself)
    names = [(b"/".join(b"a%d" % k for k in range(99)) + b"/a98x", 0x35, 0), (b"/".join(b"a%d" % k for k in range(99)), 0x30, 61)]
    want, _ = _check(setup, [_entries(names)], grid_cap, dirs=["**/a98x"], files=[])
    assert want[0].tolist() == [km.SKIP_DIR, km.SKIP_UNDER]  # the direct parent of a recorded directory


@pytest.mark.parametrize("grid_cap", [1, 0])
def test_name_lengths(setup, grid_cap):
    names = []
    for ln in (255, 256, 65536):
        d = (b"q/" + b"dir/" * (ln // 4))[:ln - 2 - len(b"x/skipme")] + b"x/skipme"
        assert len(d) == ln - 2 and b"//" not in d
        names += [(d + b"/f", 0x30, 61), (d, 0x35, 0), (d + b"/f", 0x30, 61), (d[:-1] + b"/f", 0x30, 61),
                  (d[:-7] + b"k.pem", 0x30, 61), (d + b"/", 0, 0)]
        assert len(names[-4][0]) == ln
    for dirs in (["**/skipme"], ["q/**"], ["q/dir/dir/**", "**/dir/x/skipme"]):
        want, _ = _check(setup, [_entries(names)], grid_cap, dirs=dirs, files=["**/*k.pem"])
        v = want[0].tolist()
        for k in range(3):
            assert v[6 * k + 1] == km.SKIP_DIR and v[6 * k + 5] == km.SKIP_DIR and v[6 * k + 4] == km.SKIP_FILE
            assert v[6 * k] != km.SKIP_UNDER and v[6 * k + 2] == km.SKIP_UNDER


@pytest.mark.parametrize("grid_cap", [1, 0])
def test_three_layers_with_the_same_names_and_only_the_middle_one_records(setup, grid_cap):
    files = [(b"app/skipme/a.conf", 0x30, 61), (b"app/skipme", 0x32, 0), (b"app/skipme/b.conf", 0x30, 61),
             (b"app", 0x30, 61), (b"app/skipme/deep/c.conf", 0x30, 61)]
    middle = list(files)
    middle[1] = (b"app/skipme", 0x35, 0)
    outer, mid = _entries(files, 1), _entries(middle, 1)
    assert [e["start"] for e in outer] == [e["start"] for e in mid]  # the same ranks too
    for slots in (0, "min"):
        want, _ = _check(setup, [outer, mid, outer], grid_cap, dirs=["**/skipme"], files=[], slots=slots)
        v = want[0].tolist()
        assert km.SKIP_UNDER not in v[:5] + v[10:] and km.SKIP_DIR not in v[:5] + v[10:]
        assert v[5:10] == [rm.KEEP, km.SKIP_DIR, km.SKIP_UNDER, km.SKIP_UNDER, km.SKIP_UNDER]  # ("app": the parent)
    want, _ = _check(setup, [mid, outer, mid], grid_cap, dirs=["**/skipme"], files=[])
    assert want[0].tolist()[5:10] == [rm.KEEP, rm.OTHER, rm.KEEP, rm.KEEP, rm.KEEP]


@pytest.mark.parametrize("grid_cap", [1, 0])
def test_an_empty_layer_in_any_position(setup, grid_cap):
    first, last = _entries(_tree(70, 1), 1), _entries(_tree(130, 2), 2)
    want, _ = _check(setup, [first, [], last], grid_cap)
    cnt = {k: want[3][:, i].tolist() for i, k in enumerate(rm.COUNTS)}
    assert cnt["entries"] == [70, 0, 130] and cnt["records"][1] == 0 and cnt["pad0"][1] == 0 and cnt["pad1"][1] == 0
    for k, entries in ((0, first), (2, last)):  # each layer's slice is what the stage gives for that layer alone
        alone, _ = _check(setup, [entries], grid_cap)
        r0, p0 = cnt["rec_first"][k], cnt["path_first"][k]
        assert want[1][48 * r0:48 * (r0 + cnt["records"][k])] == alone[1]
        assert want[2][p0:p0 + cnt["path_bytes"][k]] == alone[2]
        assert (cnt["pad0"][k], cnt["pad1"][k]) == (int(alone[3][0][14]), int(alone[3][0][15]))
    _check(setup, [[], first, []], grid_cap)
    _check(setup, [[], first], grid_cap)
    _check(setup, [first, []], grid_cap, slots="min")
    _check(setup, [[], []], grid_cap)
