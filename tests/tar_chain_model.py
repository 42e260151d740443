"""A pure-Python model of the GPU half of the tar chain walk (trivy_amd/csrc/tarchain.h, tarchain.hip;
tsg_analyzer_set_tar_walk mode 1) and the layers its tests share.

The contract: layer bytes -> the candidate bitmap (tests/tar_index_model.is_candidate), and from block 0 the
entries of the header chain, each read as trivy_amd/csrc/tar_index_host.h's ChainEntryT / ResolveT read it,
up to the stop -- the first entry start that is not completed:

  END          the offset is at or past the layer's end, the block there is all zero, or the entry's
               extension headers run into either;
  INCOMPLETE   with a reason: what the device does not decide (a cap, a PAX size that is not 1..18 digits)
               or what is malformed (size field, PAX record, a chain block that is no candidate, truncation).

Per entry: start, hdr, data, size, the raw name (PAX path, else GNU 'L' data up to its NUL, else ustar
prefix + '/' + name, else name), the typeflag byte, where the name came from, the extension headers hopped.
"""
import io
import struct
import tarfile

import numpy as np

from tests import tar_index_model as tm

END, INCOMPLETE = 0, 1
OK, BAD_SIZE, BAD_PAX, PAX_SIZE_FORM, CAP, NOT_CANDIDATE, TRUNCATED, TOO_LARGE = range(8)
NAME_PAX, NAME_LONG = 1, 2
MAX_EXT = 16
MAX_PAX_DATA = 64 << 10
MAX_NAME_SRC = 64 << 10
MAX_PAX_SIZE_DIGITS = 18
REC = struct.Struct("<QQQQQIBBBB16x")  # tsg_tar_entry_rec
assert REC.size == 64


def _cstr(b: bytes) -> bytes:
    return b.split(b"\0", 1)[0]


def _parse_pax(d: bytes, st: dict):
    """ParsePax with the device's rule for size; updates st; returns a reason."""
    p, n = 0, len(d)
    while p < n:
        sp = d.find(b" ", p)
        if sp < 0:
            return BAD_PAX
        digits = d[p:sp]
        if any(not 0x30 <= c <= 0x39 for c in digits):
            return BAD_PAX
        ln = int(digits) if digits else 0
        if ln < sp - p + 2 or p + ln > n or d[p + ln - 1] != 0x0A:
            return BAD_PAX
        rec = d[sp + 1:p + ln - 1]
        eq = rec.find(b"=")
        if eq < 0:
            return BAD_PAX
        k, v = rec[:eq], rec[eq + 1:]
        if k == b"path":
            st["path"] = v
        elif k == b"size":
            if not 1 <= len(v) <= MAX_PAX_SIZE_DIGITS or any(not 0x30 <= c <= 0x39 for c in v):
                return PAX_SIZE_FORM
            st["size"] = int(v)
        p += ln
    return OK


def entry(data: bytes, n: int, cand: set, c: int):
    """The entry that starts at candidate block c: ("ok", fields), ("end", n_ext) or ("inc", reason, n_ext)."""
    p = 512 * c
    st = {}
    n_ext = 0
    long_name = None
    while True:
        if p + 512 > n:
            return ("end", n_ext) if p >= n else ("inc", TRUNCATED, n_ext)
        h = data[p:p + 512]
        if p != 512 * c and p // 512 not in cand:
            return ("end", n_ext) if not any(h) else ("inc", NOT_CANDIDATE, n_ext)
        typ = h[156:157]
        size = tm.parse_numeric(h[124:136])
        if size is None or size < 0:
            return ("inc", BAD_SIZE, n_ext)
        dsz = 0 if typ in b"123456" and typ else size
        dat = p + 512
        if dat + dsz > n:
            return ("inc", TRUNCATED, n_ext)
        if typ not in (b"x", b"L", b"K"):
            break
        if n_ext == MAX_EXT:
            return ("inc", CAP, n_ext)
        n_ext += 1
        if typ == b"x":
            if dsz > MAX_PAX_DATA:
                return ("inc", CAP, n_ext)
            r = _parse_pax(data[dat:dat + dsz], st)
            if r != OK:
                return ("inc", r, n_ext)
        if typ == b"L":
            if dsz > MAX_NAME_SRC:
                return ("inc", CAP, n_ext)
            long_name = data[dat:dat + dsz]
        p = dat + (dsz + 511) // 512 * 512
    if "size" in st:
        size = st["size"]
    dsz = 0 if typ in b"123456" and typ else size
    if p + 512 + dsz > n:
        return ("inc", TRUNCATED, n_ext)
    if "path" in st:
        name, flags = st["path"], NAME_PAX
    elif long_name is not None:
        name, flags = _cstr(long_name), NAME_LONG
    else:
        name, flags = _cstr(h[:100]), 0
        if h[257:263] == b"ustar\0" and h[263:265] == b"00":
            pfx = _cstr(h[345:500])
            if pfx:
                name = pfx + b"/" + name
    return ("ok", dict(start=512 * c, hdr=p, data=p + 512, size=dsz, name=name, typeflag=h[156], flags=flags,
                       n_ext=n_ext, next=p + 512 + (dsz + 511) // 512 * 512))


def candidate_blocks(data: bytes, n: int) -> set:
    """tm.candidates' block indices; numpy first drops the blocks that cannot be one (all zero, or a
    checksum field with a byte that is neither an octal digit, a space or a NUL, nor base-256)."""
    nb = n // 512
    if nb == 0:
        return set()
    a = np.frombuffer(data, dtype=np.uint8, count=512 * nb).reshape(nb, 512)
    f = a[:, 148:156]
    plain = (((f >= 0x30) & (f <= 0x37)) | (f == 0x20) | (f == 0)).all(axis=1)
    maybe = a.any(axis=1) & (plain | (f[:, 0] >= 0x80))
    return {int(b) for b in np.nonzero(maybe)[0] if tm.is_candidate(bytes(a[b]))}


def chain(data: bytes, n_bytes=None):
    """(entries, stop, n_candidates): the entries on the chain from block 0 up to the stop
    (kind, reason, offset, extension headers hopped before an END inside an entry)."""
    n = len(data) if n_bytes is None else n_bytes
    cand = candidate_blocks(data, n)
    out = []
    p = 0
    while True:
        if p + 512 > n:
            stop = (END, OK, p, 0) if p >= n else (INCOMPLETE, TRUNCATED, p, 0)
            break
        b = p // 512
        if b not in cand:
            stop = (END, OK, p, 0) if not any(data[p:p + 512]) else (INCOMPLETE, NOT_CANDIDATE, p, 0)
            break
        r = entry(data, n, cand, b)
        if r[0] == "end":
            stop = (END, OK, p, r[1])
            break
        if r[0] == "inc":
            stop = (INCOMPLETE, r[1], p, r[2])
            break
        out.append(r[1])
        p = r[1]["next"]
    return out, stop, len(cand)


def pack(entries):
    """(records as a uint8 array of 64-B tsg_tar_entry_rec, the name blob) in walk order."""
    recs, names = bytearray(), bytearray()
    for e in entries:
        recs += REC.pack(e["start"], e["hdr"], e["data"], e["size"], len(names), len(e["name"]), e["typeflag"],
                         e["flags"], e["n_ext"], 0)
        names += e["name"]
    return (np.frombuffer(bytes(recs) or b"\0", dtype=np.uint8).copy()[:len(recs)],
            np.frombuffer(bytes(names) or b"\0", dtype=np.uint8).copy()[:len(names)])


def unpack(recs, n, names):
    """The entries of n records and their name blob, as chain() gives them (without "next")."""
    raw, blob = bytes(recs[:64 * n]), bytes(names)
    out = []
    for i in range(n):
        start, hdr, data, size, off, ln, typeflag, flags, n_ext, pad = REC.unpack(raw[64 * i:64 * i + 64])
        assert pad == 0 and raw[64 * i + 48:64 * i + 64] == bytes(16) and off + ln <= len(blob)
        out.append(dict(start=start, hdr=hdr, data=data, size=size, name=blob[off:off + ln], typeflag=typeflag,
                        flags=flags, n_ext=n_ext))
    return out


def strip_next(entries):
    return [{k: v for k, v in e.items() if k != "next"} for e in entries]


# ---- builders ------------------------------------------------------------------
def hdr(name: bytes, size: int, typeflag=b"0", prefix=b"", size_field=None, magic=b"ustar\x0000") -> bytes:
    h = bytearray(512)
    h[:len(name)] = name
    h[100:108] = b"0000644\x00"
    h[108:116] = b"0000000\x00"
    h[116:124] = b"0000000\x00"
    h[124:136] = size_field if size_field is not None else b"%011o\x00" % size
    h[136:148] = b"00000000000\x00"
    h[156:157] = typeflag
    h[257:265] = magic
    h[345:345 + len(prefix)] = prefix
    return bytes(tm.set_checksum(h))


def member(name: bytes, content: bytes = b"", typeflag=b"0", **kw) -> bytes:
    return hdr(name, len(content), typeflag, **kw) + tm.pad512(content)


def pax_records(*kvs) -> bytes:
    out = b""
    for kv in kvs:
        n = len(kv) + 3
        while len(b"%d %s\n" % (n, kv)) != n:
            n = len(b"%d %s\n" % (n, kv))
        out += b"%d %s\n" % (n, kv)
    return out


def pax_of_len(total: int, *kvs) -> bytes:
    """The records of kvs after a comment record that brings the data to exactly `total` bytes."""
    tail = pax_records(*kvs)
    for k in range(total - len(tail) - 20, total - len(tail)):
        head = pax_records(b"comment=" + b"c" * k)
        if len(head) + len(tail) == total:
            return head + tail
    raise AssertionError("no comment record of that length")


def xhdr(*kvs, raw=None) -> bytes:
    return member(b"PaxHeaders/x", pax_records(*kvs) if raw is None else raw, b"x")


def lhdr(name: bytes) -> bytes:
    return member(b"././@LongLink", name + b"\0", b"L")


TRAILER = bytes(1024)
TEXT = b"aws_access_key_id = " + tm.AWS + b"\n"


def ustar_layer() -> bytes:
    """USTAR with prefixes (tarfile splits long names), short names, a directory, a symlink."""
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w", format=tarfile.USTAR_FORMAT) as tf:
        for i in range(12):
            name = ("srv/%s/deep/%d/conf-%d.txt" % ("p" * 90, i, i)) if i % 2 else "etc/short-%d.conf" % i
            body = b"n = %d\n" % i + TEXT
            ti = tarfile.TarInfo(name)
            ti.size = len(body)
            tf.addfile(ti, io.BytesIO(body))
        d = tarfile.TarInfo("srv/dir")
        d.type = tarfile.DIRTYPE
        tf.addfile(d)
        s = tarfile.TarInfo("srv/link")
        s.type = tarfile.SYMTYPE
        s.linkname = "dir"
        tf.addfile(s)
    return buf.getvalue()


def odd_names_layer() -> bytes:
    """Unclean and absolute names, TypeRegA files, TypeRegA names ending in '/', whiteouts of non-regular
    type, an opaque-dir marker."""
    out = b""
    for name in (b"a/./b/../c.conf", b"/abs/path.conf", b"//two//slashes.conf", b"../up.conf", b"a/b/"):
        out += member(name, TEXT)
    out += member(b"old/rega.conf", TEXT, b"\0", magic=bytes(8))
    out += member(b"old/regadir/", b"", b"\0", magic=bytes(8))
    out += member(b"d/.wh.gone", b"", b"5")
    out += member(b"d/.wh..wh..opq", b"", b"2")
    out += member(b"d/.wh.file", b"", b"0")
    out += member(b"./", b"", b"5")
    out += member(b"tail.conf", TEXT)
    return out + TRAILER


FILL = (b"plain text, no header here\n" * 20)[:512]


def sized(name: bytes, blocks: int) -> bytes:
    """A regular file of `blocks` data blocks of text."""
    return hdr(name, 512 * blocks) + FILL * blocks


def boundary_layer(S: int) -> bytes:
    """Everything the marking pass can get wrong at the boundaries of segments of S blocks: S + 3 zero-size
    files back to back (every block of a segment is an entry), a file whose data ends exactly on a segment
    boundary, a file at a segment's first block that spans more than three segments, an entry whose x and L
    headers straddle a boundary, and a tar inside a file's data -- off-chain candidates: one at the first
    block of a segment whose successor is exactly the next real header, an x header with garbage data, one
    whose size points past the layer."""
    out = []

    def at():
        return sum(len(b) for b in out) // 512

    for i in range(S + 3):
        out.append(hdr(b"z/%d" % i, 0))
    out.append(sized(b"ends/on-boundary.txt", S - 1 - at() % S if at() % S != S - 1 else 2 * S - 1))
    assert at() % S == 0
    out.append(sized(b"spans/three-segments.txt", 3 * S + 5))
    pad = (S - 2 - (at() + 1)) % S or S
    out.append(sized(b"pad/to-straddle.txt", pad))
    assert at() % S == S - 2
    long_name = b"straddle/" + b"n" * 150 + b".conf"
    out.append(xhdr(b"mtime=1.5"))            # blocks S - 2, S - 1
    out.append(lhdr(long_name))               # blocks S, S + 1 of the next segment
    out.append(member(b"straddle/short", TEXT))
    # the tar inside outer.bin: inner block j is layer block q + 1 + j
    q = at()
    first = -(q + 1) % S                      # inner index of a segment's first block
    while first < 4:
        first += S
    inner = [hdr(b"inner/first", 0), hdr(b"inner/x", 512, b"x"), (b"garbage, no PAX records " * 30)[:512],
             hdr(b"inner/past-the-end", 0, size_field=b"%011o\x00" % (1 << 32))]
    inner += [FILL] * (first - len(inner))
    assert len(inner) == first and (q + 1 + first) % S == 0
    inner.append(hdr(b"inner/at-segment-start", 512 * 6))  # its successor: the header after outer.bin
    inner += [FILL] * 6
    out.append(hdr(b"outer.bin", 512 * len(inner)) + b"".join(inner))
    out.append(member(b"after.conf", TEXT))
    return b"".join(out) + TRAILER


def complete_cases():
    """Small layers the device completes: name -> bytes."""
    T, out = TEXT, {}
    body = (b"k = v\n" * 200)[:1000]
    # the PAX size replaces the header's (a sparse stand-in: header size 0), on a regular file and on a symlink,
    # where it is then ignored (header-only): the symlink's successor is the block after it
    out["pax-size-override"] = (xhdr(b"size=1000") + hdr(b"sparse/file", 0) + tm.pad512(body) +
                                xhdr(b"size=1000") + hdr(b"sparse/link", 0, b"2") + member(b"after", T) +
                                TRAILER)
    out["two-x-headers"] = (xhdr(b"path=first/name", b"size=3") + xhdr(b"path=second/name", b"mtime=1.5") +
                            hdr(b"short", 700) + tm.pad512(b"abc") + member(b"after", T) + TRAILER)
    out["K-and-g"] = (member(b"pax_global_header", pax_records(b"comment=global"), b"g") +
                      member(b"././@LongLink", b"l" * 120 + b"\0", b"K") + lhdr(b"n" * 130) +
                      hdr(b"short", 0, b"2") + member(b"after", T) + TRAILER)
    out["base-256-size"] = (hdr(b"big/base256", 0, size_field=b"\x80" + (1300).to_bytes(11, "big")) +
                            tm.pad512(b"x" * 1300) + member(b"after", T) + TRAILER)
    out["symlink-with-size"] = hdr(b"link", 1234, b"2") + member(b"after", T) + TRAILER
    out["x-then-zero-block"] = member(b"first", T) + xhdr(b"path=never/seen") + TRAILER
    out["x-then-end"] = member(b"first", T) + xhdr(b"path=never/seen")
    out["16-extension-headers"] = (b"".join(xhdr(b"path=p/%d" % i) for i in range(16)) + member(b"short", T) +
                                   TRAILER)
    rec = pax_of_len(64 << 10, b"path=exactly/64KiB")
    out["pax-data-64KiB"] = xhdr(raw=rec) + member(b"short", T) + TRAILER
    out["long-name-with-NULs"] = member(b"././@LongLink", b"dir/name\0tail\0\0", b"L") + member(b"s", T) + TRAILER
    out["only-zero-blocks"] = bytes(8 * 512)
    out["one-zero-block"] = bytes(512)
    return out


def punt_cases():
    """Layers the device walk stops on, INCOMPLETE: name -> (bytes, reason, the stop's offset)."""
    T, out = TEXT, {}
    good = member(b"first", T) + member(b"second", T)
    at = len(good)
    out["pax-size-with-sign"] = (good + xhdr(b"size=+12") + hdr(b"f", 0) + tm.pad512(b"x" * 12) + TRAILER,
                                 PAX_SIZE_FORM, at)
    out["pax-size-19-digits"] = (good + xhdr(b"size=0000000000000000012") + member(b"f", b"x" * 12) + TRAILER,
                                 PAX_SIZE_FORM, at)
    rec = pax_of_len((64 << 10) + 1, b"path=one/too/many")
    out["pax-data-64KiB+1"] = (good + xhdr(raw=rec) + member(b"f", T) + TRAILER, CAP, at)
    out["long-name-64KiB+1"] = (good + member(b"././@LongLink", b"n" * (64 << 10) + b"\0", b"L") + member(b"f", T) +
                                TRAILER, CAP, at)
    out["17-extension-headers"] = (good + b"".join(xhdr(b"path=p/%d" % i) for i in range(17)) + member(b"f", T) +
                                   TRAILER, CAP, at)
    bad = bytearray(good + member(b"third", T) + member(b"fourth", T) + TRAILER)
    bad[at + 150] ^= 0x01
    out["bad-checksum-mid-chain"] = (bytes(bad), NOT_CANDIDATE, at)
    bad = bytearray(good + xhdr(b"path=p") + member(b"f", T) + TRAILER)
    bad[at + 1024 + 150] ^= 0x01  # the header an x header hops to
    out["bad-checksum-after-x"] = (bytes(bad), NOT_CANDIDATE, at)
    out["truncated-last-entry"] = ((good + member(b"third", b"y" * 2000))[:at + 512 + 1500], TRUNCATED, at)
    out["truncated-x-data"] = ((good + xhdr(b"path=" + b"p" * 900))[:at + 512 + 600], TRUNCATED, at)
    out["bad-size-field"] = (good + hdr(b"f", 0, size_field=b"0000000009\x00\x00") + TRAILER, BAD_SIZE, at)
    out["negative-size"] = (good + hdr(b"f", 0, size_field=b"\xff" * 12) + TRAILER, BAD_SIZE, at)
    out["bad-pax-record"] = (good + xhdr(raw=b"12 path=abcX") + member(b"f", T) + TRAILER, BAD_PAX, at)
    out["pax-record-without-equals"] = (good + xhdr(raw=b"8 pathx\n") + member(b"f", T) + TRAILER, BAD_PAX, at)
    return out
