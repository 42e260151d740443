"""ctypes binding of trivy_amd/libtsg.so (the C-ABI declared in include/*.h).

The library is built in-tree by trivy_amd/_build.py (``__graft_entry__.build()``).
There is no fallback: if the shared object is missing, importing the product
fails loudly.
"""
import ctypes
import os
from pathlib import Path

# TSG_LIB: an alternative build of the same library (tools/build_variant.py, tuning runs)
_PATH = Path(os.environ.get("TSG_LIB") or Path(__file__).resolve().parent / "libtsg.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not _PATH.exists():
            raise ImportError("trivy_amd native library %s is missing: run __graft_entry__.build()" % _PATH)
        _lib = ctypes.CDLL(str(_PATH), mode=os.RTLD_NOW | ctypes.RTLD_GLOBAL)
        _declare(_lib)
    return _lib


def _declare(L):
    c = ctypes
    L.tsg_last_error.restype = c.c_char_p
    L.tsg_regex_find_all.restype = c.c_int
    L.tsg_regex_find_all.argtypes = [c.c_char_p, c.c_char_p, c.c_uint64, c.c_int,
                                     c.POINTER(c.c_int64), c.c_uint32, c.POINTER(c.c_int64),
                                     c.c_uint64, c.POINTER(c.c_uint64), c.POINTER(c.c_int32)]
    L.tsg_regex_match.restype = c.c_int
    L.tsg_regex_match.argtypes = [c.c_char_p, c.c_char_p, c.c_uint64]
    L.tsg_go_bytes_to_lower.restype = c.c_int64
    L.tsg_go_bytes_to_lower.argtypes = [c.c_char_p, c.c_uint64, c.c_char_p, c.c_uint64]


def last_error(L=None):
    """Thread-local error text of library L (default libtsg.so)."""
    L = L if L is not None else lib()
    L.tsg_last_error.restype = ctypes.c_char_p
    e = L.tsg_last_error()
    return e.decode("utf-8", "replace") if e else ""


def regex_find_all(pattern: str, text: bytes, submatch=True, windows=None):
    """Go FindAll[Submatch]Index through the native engine -> list of index lists."""
    L = lib()
    pat = pattern.encode("utf-8", "surrogateescape")
    wbuf, nw = None, 0
    if windows is not None:
        flat = [x for w in windows for x in w]
        wbuf = (ctypes.c_int64 * max(1, len(flat)))(*flat)
        nw = len(windows)
    cap = 1 << 12
    while True:
        out = (ctypes.c_int64 * cap)()
        n = ctypes.c_uint64()
        ncap = ctypes.c_int32()
        rc = L.tsg_regex_find_all(pat, text, len(text), 1 if submatch else 0, wbuf, nw, out, cap,
                                  ctypes.byref(n), ctypes.byref(ncap))
        if rc != 0:
            raise ValueError(last_error())
        if n.value <= cap:
            break
        cap = n.value
    k = 2 * (ncap.value + 1) if submatch else 2
    flat = list(out[:n.value])
    return [flat[i:i + k] for i in range(0, len(flat), k)]


def regex_match(pattern: str, text: bytes) -> bool:
    rc = lib().tsg_regex_match(pattern.encode("utf-8", "surrogateescape"), text, len(text))
    if rc < 0:
        raise ValueError(last_error())
    return rc == 1


GATHER_PIECE = 16384  # csrc/xform.h kGatherPiece


def transform_census(raw: bytes, offsets, kinds, tail: bytes = b"", device=0) -> bytes:
    """tsg_debug_transform_census: one mark byte per file (1: the transform of its kind changes it).
    offsets: n_files + 1 from 0 to len(raw); tail: up to 64 bytes placed behind the arena (0x00 after)."""
    L = lib()
    c = ctypes
    n_files = len(offsets) - 1
    if len(kinds) != n_files or len(tail) > 64:
        raise ValueError("transform_census: one kind per file, a tail of at most 64 bytes")
    buf = c.create_string_buffer(bytes(raw) + bytes(tail).ljust(64, b"\0"), len(raw) + 64)
    off = (c.c_uint64 * (n_files + 1))(*[int(x) for x in offsets])
    kd = (c.c_uint8 * max(1, n_files))(*[int(k) for k in kinds])
    mark = (c.c_uint8 * max(1, n_files))()
    L.tsg_debug_transform_census.restype = c.c_int
    L.tsg_debug_transform_census.argtypes = [c.c_int, c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint32, c.c_void_p,
                                             c.c_void_p]
    if L.tsg_debug_transform_census(int(device), buf, len(raw), off, n_files, kd, mark) != 0:
        raise RuntimeError(last_error(L))
    return bytes(mark[:n_files])


def gather_device(raw: bytes, src_off, dst_off, out: bytes, tail: bytes = b"", device=0) -> bytes:
    """tsg_debug_gather_device: `out` (dst_off[-1] + 64 bytes) with file i, raw[src_off[i] ..) of length
    dst_off[i + 1] - dst_off[i], written at dst_off[i]; every other byte of it as given."""
    L = lib()
    c = ctypes
    n_files = len(src_off)
    if len(dst_off) != n_files + 1 or len(out) != int(dst_off[-1]) + 64 or len(tail) > 64:
        raise ValueError("gather_device: n + 1 destination offsets, an output of dst_off[-1] + 64 bytes")
    buf = c.create_string_buffer(bytes(raw) + bytes(tail).ljust(64, b"\0"), len(raw) + 64)
    so = (c.c_uint64 * max(1, n_files))(*[int(x) for x in src_off])
    do = (c.c_uint64 * (n_files + 1))(*[int(x) for x in dst_off])
    ob = c.create_string_buffer(bytes(out), len(out))
    L.tsg_debug_gather_device.restype = c.c_int
    L.tsg_debug_gather_device.argtypes = [c.c_int, c.c_void_p, c.c_uint64, c.c_void_p, c.c_void_p, c.c_uint32,
                                          c.c_void_p]
    if L.tsg_debug_gather_device(int(device), buf, len(raw), so, do, n_files, ob) != 0:
        raise RuntimeError(last_error(L))
    return ob.raw


FETCH_SEG = 16384  # csrc/fetch.h kFetchSeg


class HookRefused(ValueError):
    """A debug hook's argument check refused the call (-2) before any HIP call."""


def _hook_rc(L, rc):
    if rc == -2:
        raise HookRefused(last_error(L))
    if rc != 0:
        raise RuntimeError("rc %d: %s" % (rc, last_error(L)))


def _u64s(xs, at_least=1):
    xs = [int(x) for x in xs]
    return (ctypes.c_uint64 * max(at_least, len(xs)))(*xs)


def gather_files(src: bytes, xoff, files, dst_off, out: bytes, tail: bytes = b"", device=0) -> bytes:
    """tsg_debug_gather_files: `out` (dst_bytes + 64) with file files[i], src[xoff[f] .. xoff[f + 1]), written at
    dst_off[i]; every other byte of it as given.  tail: up to 64 bytes placed behind src (0x00 after)."""
    L = lib()
    c = ctypes
    n_files, n = len(xoff) - 1, len(files)
    if len(dst_off) != n or len(out) < 64 or len(tail) > 64:
        raise ValueError("gather_files: one destination per listed file, an output of dst_bytes + 64 bytes")
    buf = c.create_string_buffer(bytes(src) + bytes(tail).ljust(64, b"\0"), len(src) + 64)
    fl = (c.c_uint32 * max(1, n))(*[int(x) for x in files])
    ob = c.create_string_buffer(bytes(out), len(out))
    L.tsg_debug_gather_files.restype = c.c_int
    L.tsg_debug_gather_files.argtypes = [c.c_int, c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint32, c.c_void_p,
                                         c.c_void_p, c.c_uint32, c.c_void_p, c.c_uint64]
    _hook_rc(L, L.tsg_debug_gather_files(int(device), buf, len(src), _u64s(xoff), n_files, fl, _u64s(dst_off), n, ob,
                                         len(out) - 64))
    return ob.raw


def gather_host(src: bytes, src_off, lens, dst_off, out: bytes, device=0) -> bytes:
    """tsg_debug_gather_host: `out` (dst_bytes + 64) with file i, src[src_off[i] .. + lens[i]) read from mapped host
    memory, written at dst_off[i]; every other byte of it as given."""
    L = lib()
    c = ctypes
    n = len(src_off)
    if len(lens) != n or len(dst_off) != n or len(out) < 64:
        raise ValueError("gather_host: a source, a length and a destination per file, an output of dst_bytes + 64")
    buf = c.create_string_buffer(bytes(src), max(1, len(src)))
    ob = c.create_string_buffer(bytes(out), len(out))
    L.tsg_debug_gather_host.restype = c.c_int
    L.tsg_debug_gather_host.argtypes = [c.c_int, c.c_void_p, c.c_uint64, c.c_void_p, c.c_void_p, c.c_void_p,
                                        c.c_uint32, c.c_void_p, c.c_uint64]
    _hook_rc(L, L.tsg_debug_gather_host(int(device), buf, len(src), _u64s(src_off), _u64s(lens), _u64s(dst_off), n, ob,
                                        len(out) - 64))
    return ob.raw


def fetch_files_device(arena: bytes, offsets, flags=None, cands=None, n_cands=None, cand_cap=None, direct_bytes=1 << 62,
                       stage_bytes=1 << 22, copy_bytes=0, device=0):
    """tsg_debug_fetch_files_device.  The marked files: `flags` (one per file, nonzero: fetch) or `cands` (64-B
    Candidate records as bytes; n_cands, default the records given, is what the device count says; cand_cap, default
    the same, bounds the records uploaded).  -> dict: packed (bytes: copy_bytes, or packed_bytes when 0), list,
    lpoff, and the counters packed_bytes, n_packed, n_direct, n_files, file_bytes, rounds."""
    L = lib()
    c = ctypes
    n_files = len(offsets) - 1
    if flags is not None:
        if len(flags) != n_files:
            raise ValueError("fetch_files_device: one flag per file")
        fl = (c.c_uint32 * max(1, n_files))(*[int(x) for x in flags])
        cb, nc, cap = None, 0, 0
    else:
        fl = None
        cands = bytes(cands or b"")
        nc = len(cands) // 64 if n_cands is None else int(n_cands)
        cap = nc if cand_cap is None else int(cand_cap)
        cb = c.create_string_buffer(cands, max(1, len(cands)))
    off = _u64s(offsets)
    # every file rounded up to 16 bounds the plan's packed_bytes
    packed_cap = int(copy_bytes) if copy_bytes else len(arena) + 16 * n_files + 16
    packed = c.create_string_buffer(max(1, packed_cap))
    lst = (c.c_uint32 * (n_files + 1))()
    lpoff = (c.c_uint64 * (n_files + 2))()
    ctr = (c.c_uint64 * 6)()
    ab = c.create_string_buffer(bytes(arena), max(1, len(arena)))
    L.tsg_debug_fetch_files_device.restype = c.c_int
    L.tsg_debug_fetch_files_device.argtypes = [c.c_int, c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint32, c.c_void_p,
                                               c.c_uint64, c.c_uint32, c.c_void_p, c.c_uint64, c.c_uint64, c.c_uint64,
                                               c.c_void_p, c.c_uint64, c.c_void_p, c.c_void_p, c.c_void_p]
    _hook_rc(L, L.tsg_debug_fetch_files_device(int(device), ab, len(arena), off, n_files, cb, nc, cap, fl,
                                               int(direct_bytes), int(stage_bytes), int(copy_bytes), packed,
                                               packed_cap, lst, lpoff, ctr))
    names = ("packed_bytes", "n_packed", "n_direct", "n_files", "file_bytes", "rounds")
    r = dict(zip(names, (int(x) for x in ctr)))
    n_packed = r["n_packed"]
    r["packed"] = packed.raw[:int(copy_bytes) if copy_bytes else r["packed_bytes"]]
    r["list"] = list(lst[:n_packed])
    r["lpoff"] = list(lpoff[:n_packed + 1])
    return r


class HookStatus(RuntimeError):
    """A debug hook came back with a status of its own (neither 0 nor the -2 of a refusal)."""

    def __init__(self, rc, text):
        RuntimeError.__init__(self, "rc %d: %s" % (rc, text))
        self.rc = rc


def materialize(arena: bytes, offsets, files, matches, spans, guard=True, lines_cap=None, text_cap=None, device=0):
    """tsg_debug_materialize.  arena: the n_bytes + 64 bytes to upload (offsets end at n_bytes); files, matches,
    spans: the raw MatFile / MatMatch / MatSpan records (bytes, or numpy arrays of 24 / 40 / 24-B items).
    -> dict: findings (40-B records), pref (u64 list), lines (24-B records), text, n_lines, n_text, all bytes
    but pref.  HookRefused for -2, HookStatus (its rc: -3 a cap too small, -4 a guard byte, -5 the kernel's
    own check, -6 totals past their bounds) otherwise."""
    L = lib()
    c = ctypes
    n_files = len(offsets) - 1
    n_bytes = len(arena) - 64
    fb, mb, sb = (x if isinstance(x, bytes) else x.tobytes() for x in (files, matches, spans))
    if n_bytes < 0 or len(fb) % 24 or len(mb) % 40 or len(sb) % 24:
        raise ValueError("materialize: an arena with its 64-B tail, records of 24 / 40 / 24 bytes")
    nf, nm, ns = len(fb) // 24, len(mb) // 40, len(sb) // 24
    lines_cap = 4 * nm if lines_cap is None else int(lines_cap)
    if text_cap is None:  # the scanner's own bound
        import numpy as np
        m = np.frombuffer(mb, dtype=np.int64).reshape(-1, 5)
        text_cap = int((np.maximum(100, m[:, 2] - m[:, 1] + 50) + 400).sum()) if nm else 0
    ab = c.create_string_buffer(bytes(arena), len(arena))
    fo = c.create_string_buffer(max(1, 40 * nm))
    pref = (c.c_uint64 * (nm + 1))()
    lo = c.create_string_buffer(max(1, 24 * lines_cap))
    tx = c.create_string_buffer(max(1, text_cap))
    tot = (c.c_uint64 * 2)()
    L.tsg_debug_materialize.restype = c.c_int
    L.tsg_debug_materialize.argtypes = [c.c_int, c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint32, c.c_char_p, c.c_uint32,
                                        c.c_char_p, c.c_uint32, c.c_char_p, c.c_uint32, c.c_int, c.c_void_p, c.c_void_p,
                                        c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint64, c.c_void_p]
    rc = L.tsg_debug_materialize(int(device), ab, n_bytes, _u64s(offsets), n_files, fb, nf, mb, nm, sb, ns,
                                 1 if guard else 0, fo, pref, lo, lines_cap, tx, text_cap, tot)
    if rc == -2:
        raise HookRefused(last_error(L))
    n_lines, n_text = int(tot[0]), int(tot[1])
    if rc != 0:
        e = HookStatus(rc, last_error(L))
        e.n_lines, e.n_text = n_lines, n_text
        raise e
    return dict(findings=fo.raw[:40 * nm], pref=list(pref), lines=lo.raw[:24 * n_lines], text=tx.raw[:n_text],
                n_lines=n_lines, n_text=n_text)


PATH_TABLE_BYTES = 8520  # sizeof(PathTable), csrc/pathfilter.h
SURE_TABLE_BYTES = 8328  # sizeof(SureTable)
PATH_NON_ASCII = 0x80000000  # kPathNonAscii


def path_tables(lits, sure_lits):
    """tsg_debug_path_tables (no GPU).  lits: [(lowercased literal bytes, rule id)]; sure_lits: [(positions,
    begin, end)] with positions a list of (byte, byte) pairs.  -> (raw PathTable or None, raw SureTable or
    None): None where the builder refused."""
    L = lib()
    c = ctypes
    lb = b"".join(bytes(x) for x, _ in lits)
    lo, at = [0], 0
    for x, _ in lits:
        at += len(x)
        lo.append(at)
    rules = (c.c_uint32 * max(1, len(lits)))(*[int(r) for _, r in lits])
    pairs = bytes(b for pos, _, _ in sure_lits for pr in pos for b in pr)
    so, at = [0], 0
    for pos, _, _ in sure_lits:
        at += len(pos)
        so.append(at)
    fl = bytes((1 if b else 0) | (2 if e else 0) for _, b, e in sure_lits)
    pt, st = c.create_string_buffer(PATH_TABLE_BYTES), c.create_string_buffer(SURE_TABLE_BYTES)
    L.tsg_debug_path_tables.restype = c.c_int
    L.tsg_debug_path_tables.argtypes = [c.c_char_p, c.c_void_p, c.c_void_p, c.c_uint32, c.c_char_p, c.c_void_p,
                                        c.c_char_p, c.c_uint32, c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint64]
    rc = L.tsg_debug_path_tables(lb or b"\0", _u64s(lo), rules, len(lits), pairs or b"\0", _u64s(so), fl or b"\0",
                                 len(sure_lits), pt, PATH_TABLE_BYTES, st, SURE_TABLE_BYTES)
    if rc < 0:
        raise ValueError(last_error(L))
    return (pt.raw if rc & 1 else None, st.raw if rc & 2 else None)


def path_filter(path_table: bytes, sure_table, batches, host_packed=False, want_skip=True, device=0):
    """tsg_debug_path_filter: `batches` (lists of path bytes) one after another on one PathFilter.  -> one
    (hits, skip) per batch: hits a list of (file, pad, rules) records as the filter returned them, skip the
    batch's skip bytes or None when it had none."""
    L = lib()
    c = ctypes
    paths = [p for b in batches for p in b]
    first, at = [0], 0
    for b in batches:
        at += len(b)
        first.append(at)
    blob = b"".join(paths)
    off, at = [0], 0
    for p in paths:
        at += len(p)
        off.append(at)
    n = len(paths)
    import numpy as np
    off = np.array(off, dtype=np.uint64)
    hits = np.zeros((max(1, n), 2), dtype=np.uint64)
    skip = np.full(max(1, n), 0x77, dtype=np.uint8)
    n_hits = (c.c_uint32 * max(1, len(batches)))()
    have = (c.c_uint8 * max(1, len(batches)))()
    bf = (c.c_uint32 * len(first))(*first)
    L.tsg_debug_path_filter.restype = c.c_int
    L.tsg_debug_path_filter.argtypes = [c.c_int, c.c_char_p, c.c_char_p, c.c_char_p, c.c_void_p, c.c_void_p, c.c_uint32,
                                        c.c_uint32, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    _hook_rc(L, L.tsg_debug_path_filter(int(device), path_table, sure_table, blob or b"\0", off.ctypes.data, bf,
                                        len(batches), (1 if host_packed else 0) | (2 if want_skip else 0),
                                        hits.ctypes.data, n_hits, skip.ctypes.data, have))
    out = []
    for b in range(len(batches)):
        h = hits[first[b]:first[b] + int(n_hits[b])]
        recs = [(int(x) & 0xFFFFFFFF, int(x) >> 32, int(r)) for x, r in h]
        out.append((recs, skip[first[b]:first[b + 1]].tobytes() if have[b] else None))
    return out


def go_bytes_to_lower(b: bytes) -> bytes:
    out = ctypes.create_string_buffer(len(b) * 3 + 4)
    n = lib().tsg_go_bytes_to_lower(b, len(b), out, len(out))
    return out.raw[:n]
