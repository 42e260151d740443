"""Brute-force model of the windows fetch's layout (trivy_amd/csrc/fetch_layout.h)
and ctypes wrappers of its test hooks (include/tsg_debug.h).  Restated here from
the layout's description, not from the C++: a numpy bitmap, one bit per 256-B
granule of the arena.
"""
import ctypes as c

import numpy as np

from trivy_amd import _lib

GRANULE = 256
NO_MAX_LEN = 0xFFFFFFFF
CAND_DROP = 8
DEFAULTS = dict(back=16, fwd=1024, fwd_cap=4096, max_span=65536)

CAND = np.dtype([("file", "<u4"), ("rule", "<u4"), ("wlo", "<i8"), ("whi", "<i8"), ("nl_before", "<i8"),
                 ("flags", "<u4"), ("nl_back", "<u4", (3,)), ("nl_fwd", "<u4", (3,)), ("pad", "<u4")])
assert CAND.itemsize == 64


def cands_of(recs):
    """[(file, rule, wlo, whi, flags)] -> Candidate records"""
    a = np.zeros(len(recs), dtype=CAND)
    for k, (f, r, lo, hi, fl) in enumerate(recs):
        a[k] = (f, r, lo, hi, 0, fl, [0xFFFFFFFF] * 3, [0xFFFFFFFF] * 3, 0)
    return a


def _opts(o):
    o = dict(o or {})
    return np.array([o.get("back", 0), o.get("fwd", 0), o.get("fwd_cap", 0), o.get("max_span", 0)], dtype=np.uint32)


def model(offsets, cands, max_len, opts=None):
    """-> (bitmap of granules, set of files marked whole)"""
    o = dict(DEFAULTS)
    o.update({k: v for k, v in (opts or {}).items() if v})
    n_bytes = int(offsets[-1])
    bits = np.zeros((n_bytes + GRANULE - 1) // GRANULE, dtype=bool)
    whole = set()
    for rec in cands:
        f = int(rec["file"])
        if int(rec["flags"]) & CAND_DROP:
            continue
        fs, fe = int(offsets[f]), int(offsets[f + 1])
        ln = fe - fs
        if ln == 0:
            continue
        wlo, whi = int(rec["wlo"]), int(rec["whi"])
        file_gran = (fs // GRANULE, (fe + GRANULE - 1) // GRANULE)
        ml = int(max_len[int(rec["rule"])])
        fwd = ml + 4 if ml != NO_MAX_LEN and ml <= o["fwd_cap"] else o["fwd"]
        a, b = max(0, wlo - o["back"]), min(ln, whi + 1 + fwd)
        if a >= b:  # a window at the file's very end: its last byte
            a = b - 1
        g = ((fs + a) // GRANULE, (fs + b + GRANULE - 1) // GRANULE)
        if whi - wlo + 1 > o["max_span"] or g == file_gran:
            g = file_gran
            whole.add(f)
        bits[g[0]:g[1]] = True
    return bits, whole


def model_plan(offsets, bits, whole):
    """-> runs [(g0, g1, packed)], views [(file, lo, hi, packed)], totals (granules, runs, whole, bytes)"""
    d = np.diff(np.concatenate(([0], bits.astype(np.int8), [0])))
    starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    rank = np.concatenate(([0], np.cumsum(bits)))  # packed index of each granule
    runs = [(int(a), int(b), int(rank[a]) * GRANULE) for a, b in zip(starts, ends)]
    views = []
    for f in range(len(offsets) - 1):
        fs, fe = int(offsets[f]), int(offsets[f + 1])
        for g0, g1, p in runs:
            a, b = max(fs, g0 * GRANULE), min(fe, g1 * GRANULE)
            if a < b:
                views.append((f, a - fs, b - fs, p + a - g0 * GRANULE))
    n = int(bits.sum())
    return runs, views, (n, len(runs), len(whole), n * GRANULE)


def model_packed(arena, bits, tail=0xEE):
    """The packed layout's bytes as the device hook returns them: the arena followed
    by 64 tail bytes; a 16-B block that begins at or past the arena's end reads as 0."""
    n = len(arena)
    padded = np.concatenate((np.frombuffer(bytes(arena), dtype=np.uint8), np.full(64, tail, dtype=np.uint8),
                             np.zeros(GRANULE, dtype=np.uint8)))
    out = []
    for g in np.flatnonzero(bits):
        blk = padded[g * GRANULE:(g + 1) * GRANULE].copy()
        for b in range(0, GRANULE, 16):
            if g * GRANULE + b >= n:
                blk[b:] = 0
                break
        out.append(blk)
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint8)


def _declare(L):
    L.tsg_debug_fetch_windows_plan.restype = c.c_int
    L.tsg_debug_fetch_windows_plan.argtypes = [c.c_void_p, c.c_uint32, c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint32,
                                               c.c_void_p, c.c_void_p, c.c_uint64, c.POINTER(c.c_uint64), c.c_void_p,
                                               c.c_uint64, c.POINTER(c.c_uint64), c.c_void_p]
    L.tsg_debug_fetch_windows_device.restype = c.c_int
    L.tsg_debug_fetch_windows_device.argtypes = [c.c_int, c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint32, c.c_void_p,
                                                 c.c_uint64, c.c_uint32, c.c_void_p, c.c_uint32, c.c_void_p,
                                                 c.c_uint64, c.c_void_p, c.c_uint64, c.c_void_p]
    L.tsg_regex_find_all_bounded.restype = c.c_int
    L.tsg_regex_find_all_bounded.argtypes = [c.c_char_p, c.c_char_p, c.c_uint64, c.c_uint64, c.c_uint64, c.c_int,
                                             c.POINTER(c.c_int64), c.c_uint32, c.POINTER(c.c_int64), c.c_uint64,
                                             c.POINTER(c.c_uint64), c.POINTER(c.c_int32), c.POINTER(c.c_int32)]
    return L


def native_plan(offsets, cands, max_len, opts=None, raw_opts=None):
    L = _declare(_lib.lib())
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    cands = np.ascontiguousarray(cands)
    ml = np.ascontiguousarray(max_len, dtype=np.uint32)
    o = raw_opts if raw_opts is not None else _opts(opts)
    n_files = len(offsets) - 1
    n_gran = (int(offsets[-1]) + GRANULE - 1) // GRANULE
    runs = np.zeros((n_gran + 1, 3), dtype=np.uint64)
    views = np.zeros((n_gran + n_files + 1, 4), dtype=np.uint64)
    nr, nv = c.c_uint64(), c.c_uint64()
    tot = np.zeros(4, dtype=np.uint64)
    rc = L.tsg_debug_fetch_windows_plan(offsets.ctypes.data, n_files, cands.ctypes.data, len(cands), ml.ctypes.data,
                                        len(ml), o.ctypes.data, runs.ctypes.data, len(runs), c.byref(nr),
                                        views.ctypes.data, len(views), c.byref(nv), tot.ctypes.data)
    if rc != 0:
        raise ValueError(_lib.last_error())
    assert nr.value <= len(runs) and nv.value <= len(views)
    return ([tuple(int(x) for x in r) for r in runs[:nr.value]], [tuple(int(x) for x in v) for v in views[:nv.value]],
            tuple(int(x) for x in tot))


def device_pack(arena, offsets, cands, max_len, opts=None, stage_bytes=1 << 20, cand_cap=None, device=0):
    """-> (packed bytes, (granules, runs, whole files, rounds))"""
    L = _declare(_lib.lib())
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    cands = np.ascontiguousarray(cands)
    ml = np.ascontiguousarray(max_len, dtype=np.uint32)
    o = _opts(opts)
    a = np.frombuffer(bytes(arena), dtype=np.uint8) if len(arena) else np.zeros(1, dtype=np.uint8)
    n_bytes = len(arena)
    out = np.zeros(((n_bytes + GRANULE - 1) // GRANULE + 1) * GRANULE, dtype=np.uint8)
    ctr = np.zeros(4, dtype=np.uint64)
    rc = L.tsg_debug_fetch_windows_device(device, a.ctypes.data, n_bytes, offsets.ctypes.data, len(offsets) - 1,
                                          cands.ctypes.data, len(cands), len(cands) if cand_cap is None else cand_cap,
                                          ml.ctypes.data, len(ml), o.ctypes.data, stage_bytes, out.ctypes.data,
                                          len(out), ctr.ctypes.data)
    if rc != 0:
        raise RuntimeError(_lib.last_error())
    return out[:int(ctr[0]) * GRANULE], tuple(int(x) for x in ctr)


def find_all_bounded(pattern, text, lo, hi, submatch=True, windows=None):
    """-> (matches, hit_limit)"""
    L = _declare(_lib.lib())
    pat = pattern.encode("utf-8", "surrogateescape")
    wbuf, nw = None, 0
    if windows is not None:
        flat = [x for w in windows for x in w]
        wbuf = (c.c_int64 * max(1, len(flat)))(*flat)
        nw = len(windows)
    cap = 1 << 12
    while True:
        out = (c.c_int64 * cap)()
        n, ncap, hit = c.c_uint64(), c.c_int32(), c.c_int32()
        rc = L.tsg_regex_find_all_bounded(pat, text, len(text), lo, hi, 1 if submatch else 0, wbuf, nw, out, cap,
                                          c.byref(n), c.byref(ncap), c.byref(hit))
        if rc != 0:
            raise ValueError(_lib.last_error())
        if n.value <= cap:
            break
        cap = n.value
    k = 2 * (ncap.value + 1) if submatch else 2
    flat = list(out[:n.value])
    return [flat[i:i + k] for i in range(0, len(flat), k)], bool(hit.value)
