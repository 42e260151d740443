"""A pure-Python model of the device stage that classifies the paths of a resident tar layer's entries and
runs Required on them (trivy_amd/csrc/tarrequired.h, tarrequired.hip; tsg_analyzer_set_tar_required mode 1).

In: the 64-B entry records and the name blob of tests/tar_chain_model.py, a layer table of record and name
bases, the analyzer's config base and the scanner's two allow-path tables (raw bytes of PathTable / SureTable,
trivy_amd/csrc/pathfilter.h, or None).  Out: a verdict per entry, the 48-B file records, the path blob and 16
words of counts per layer -- every byte the stage writes.
"""
import struct

import numpy as np

from tests import tar_chain_model as cm

OTHER, WHITEOUT, OPAQUE, DROP, KEEP, ASK_ALLOW, ASK_NAME, BAD = range(8)
FREC = struct.Struct("<QQQQIBBBBQ")  # tsg_tar_file_rec
assert FREC.size == 48
COUNTS = ("entries", "regular", "whiteouts", "opaque_dirs", "records", "path_bytes", "kept", "dropped", "ask_allow",
          "ask_name", "bad", "ext_headers", "rec_first", "path_first", "pad0", "pad1")
SURE_MAX_PATH = 4096
SKIP_DIRS = (b".git", b"node_modules")
SKIP_FILES = (b"go.mod", b"go.sum", b"package-lock.json", b"yarn.lock", b"pnpm-lock.yaml", b"Pipfile.lock",
              b"Gemfile.lock")
SKIP_EXTS = (b".jpg", b".png", b".gif", b".doc", b".pdf", b".bin", b".svg", b".socket", b".deb", b".rpm", b".zip",
             b".gz", b".gzip", b".tar")
PATH_TABLE_BYTES = 8520  # sizeof(PathTable): B[256][4], S[4], E[4], rule_of[256], words, padding
SURE_TABLE_BYTES = 8328  # sizeof(SureTable): B[256][4], S[4], S0[4], E[4], EZ[4], words, padding
M64 = (1 << 64) - 1


class PathTable:
    def __init__(self, raw: bytes):
        assert len(raw) == PATH_TABLE_BYTES
        w = np.frombuffer(raw[:8256], dtype=np.uint64)
        self.B = [[int(x) for x in w[4 * c:4 * c + 4]] for c in range(256)]
        self.S = [int(x) for x in w[1024:1028]]
        self.E = [int(x) for x in w[1028:1032]]
        self.rule_of = raw[8256:8512]

    def rules(self, p: bytes) -> int:
        """The allow rules with a literal in the ASCII-lowered path."""
        D, H = [0] * 4, [0] * 4
        for c in p:
            lc = c + 32 if 0x41 <= c <= 0x5A else c
            for w in range(4):
                D[w] = ((D[w] << 1) | self.S[w]) & self.B[lc][w] & M64
                H[w] |= D[w] & self.E[w]
        out = 0
        for w in range(4):
            for bit in range(64):
                if H[w] >> bit & 1:
                    out |= 1 << self.rule_of[64 * w + bit]
        return out


class SureTable:
    def __init__(self, raw: bytes):
        assert len(raw) == SURE_TABLE_BYTES
        w = np.frombuffer(raw[:8320], dtype=np.uint64)
        self.B = [[int(x) for x in w[4 * c:4 * c + 4]] for c in range(256)]
        self.S, self.S0, self.E, self.EZ = ([int(x) for x in w[1024 + 4 * k:1028 + 4 * k]] for k in range(4))

    def completes(self, p: bytes) -> bool:
        D, hit = [0] * 4, 0
        for i, c in enumerate(p):
            for w in range(4):
                D[w] = ((((D[w] & ~(self.E[w] | self.EZ[w])) << 1) | self.S[w] | (self.S0[w] if i == 0 else 0))
                        & self.B[c][w] & M64)
                hit |= D[w] & (self.E[w] | (self.EZ[w] if i + 1 == len(p) else 0))
        return hit != 0


def tables_of(analyzer):
    """(PathTable or None, SureTable or None) of an analyzer's scanner (tsg_debug_tar_required_tables)."""
    import ctypes as c
    L = analyzer._L
    L.tsg_debug_tar_required_tables.argtypes = [c.c_void_p, c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint64,
                                                c.POINTER(c.c_uint32)]
    pt, st, have = c.create_string_buffer(PATH_TABLE_BYTES), c.create_string_buffer(SURE_TABLE_BYTES), c.c_uint32()
    assert L.tsg_debug_tar_required_tables(analyzer._h, pt, PATH_TABLE_BYTES, st, SURE_TABLE_BYTES, c.byref(have)) == 0
    return (PathTable(pt.raw) if have.value & 1 else None, SureTable(st.raw) if have.value & 2 else None)


def decide(name: bytes, typeflag: int, size: int, cfg: bytes, pt, st):
    """(verdict, where the blob's bytes begin in the name, their length, rules mask, all-rules flag)."""
    p0 = 2 if name.startswith(b"./") else 1 if name.startswith(b"/") else 0
    rest = name[p0:]
    m = rest.rstrip(b"/")
    elems = m.split(b"/")
    if not m or any(e in (b"", b".", b"..") for e in elems):  # (a leading '/' of M is an empty first element)
        return ASK_NAME, 0, len(name), 0, 0
    base = elems[-1]

    def out(v, rules=0, all_rules=0):
        return v, p0, len(m), rules, all_rules

    if base == b".wh..wh..opq":
        return out(OPAQUE)
    if base.startswith(b".wh."):
        return out(WHITEOUT)
    if not (typeflag == 0x30 or (typeflag == 0 and len(m) == len(rest))):
        return out(OTHER)
    if size >= 1 << 63:
        size -= 1 << 64
    dot = base.rfind(b".")
    if (size < 10 or any(e in SKIP_DIRS for e in elems[:-1]) or base in SKIP_FILES or m == cfg or
            (dot >= 0 and len(base) - dot <= 7 and base[dot:] in SKIP_EXTS)):
        return out(DROP)
    if pt is None or max(m) >= 0x80:
        return out(ASK_ALLOW, 0, 1)
    if st is not None and len(m) <= SURE_MAX_PATH and st.completes(m):
        return out(DROP)
    rules = pt.rules(m)
    return out(ASK_ALLOW, rules) if rules else out(KEEP)


def stage(recs, n: int, names: bytes, rec_base, name_base, cfg: bytes, pt, st):
    """(verdicts, file records, blob, counts): a uint8 array of n verdicts, the bytes of the 48-B records, the
    path blob, and an (n_layers, 16) uint64 array of counts.  rec_base / name_base: n_layers + 1 each."""
    raw, names = bytes(recs[:64 * n]), bytes(names)
    n_layers = len(rec_base) - 1
    verdicts = np.zeros(n, dtype=np.uint8)
    frecs, blob = bytearray(), bytearray()
    counts = np.zeros((n_layers, 16), dtype=np.uint64)
    memo = {}  # (the decision is a function of the name, the typeflag and the size)
    for k in range(n_layers):
        cnt = dict.fromkeys(COUNTS, 0)
        cnt["rec_first"], cnt["path_first"] = len(frecs) // 48, len(blob)
        lb, le = int(name_base[k]), int(name_base[k + 1])
        for i in range(int(rec_base[k]), int(rec_base[k + 1])):
            start, _hdr, data, size, off, ln, typeflag, _flags, n_ext, _pad = cm.REC.unpack(raw[64 * i:64 * i + 64])
            cnt["entries"] += 1
            cnt["ext_headers"] += n_ext
            if off > le - lb or ln > le - lb - off:
                verdicts[i] = BAD
                cnt["bad"] += 1
                continue
            name = names[lb + off:lb + off + ln]
            key = (name, typeflag, size)
            if key not in memo:
                memo[key] = decide(name, typeflag, size, cfg, pt, st)
            v, skip, out_len, rules, all_rules = memo[key]
            verdicts[i] = v
            cnt[{OTHER: "pad0", WHITEOUT: "whiteouts", OPAQUE: "opaque_dirs", DROP: "dropped", KEEP: "kept",
                 ASK_ALLOW: "ask_allow", ASK_NAME: "ask_name"}[v]] += 1
            if v in (KEEP, ASK_ALLOW, ASK_NAME):
                frecs += FREC.pack(start, data, size, len(blob) - cnt["path_first"], out_len, typeflag, v, all_rules, 0,
                                   rules)
                blob += name[skip:skip + out_len] + b"\0"
        cnt["pad0"] = 0
        cnt["regular"] = cnt["dropped"] + cnt["kept"] + cnt["ask_allow"]
        cnt["records"] = len(frecs) // 48 - cnt["rec_first"]
        cnt["path_bytes"] = len(blob) - cnt["path_first"]
        counts[k] = [cnt[c] for c in COUNTS]
    return verdicts, bytes(frecs), bytes(blob), counts
