"""A pure-Python model of tar_headers_kernel (trivy_amd/csrc/tarindex.hip) and the layers its tests share.

A 512-B block is a header candidate exactly when the host walk's ChecksumOK(block) && !AllZero(block)
holds (trivy_amd/csrc/tar_index_host.h, Go's archive/tar): the checksum field, bytes 148..155, parsed
as parseNumeric parses it (base-256 when the first byte has bit 7, else octal trimmed of spaces and
NULs), equals the sum of the 512 bytes with the field counted as eight spaces -- the unsigned sum, or
the signed one old writers made.
"""
import io
import random
import struct
import tarfile

import numpy as np

from tests.layers import make_layer

RECORD = 528  # u64 block index, 8 B of padding, the 512 header bytes


def parse_numeric(b: bytes):
    """archive/tar parseNumeric; None when the field does not parse."""
    if b and b[0] & 0x80:
        neg = bool(b[0] & 0x40)
        v = 0
        for i, c in enumerate(b):
            if i == 0:
                c &= 0x7F
            if neg:
                c ^= 0xFF
            if i == 0 and neg:
                c &= 0x7F
            if v >> 56:
                return None
            v = (v << 8) | c
        if v >> 63:
            return None
        return -v - 1 if neg else v
    t = b.strip(b" \x00")
    v = 0
    for c in t:
        if not 0x30 <= c <= 0x37:
            return None
        if v >> 60:
            return None
        v = v * 8 + (c - 0x30)
    return v


def is_candidate(block: bytes) -> bool:
    assert len(block) == 512
    if not any(block):
        return False
    want = parse_numeric(block[148:156])
    if want is None:
        return False
    body = block[:148] + b" " * 8 + block[156:]
    unsigned = sum(body)
    signed = sum(c - 256 if c >= 0x80 else c for c in body)
    return want == unsigned or want == signed


def candidates(data: bytes, n_bytes=None):
    """[(block index, 512 bytes)] of the complete blocks below n_bytes, ascending."""
    n = len(data) if n_bytes is None else n_bytes
    return [(b, bytes(data[512 * b:512 * b + 512])) for b in range(n // 512) if is_candidate(data[512 * b:512 * b + 512])]


def records(cands, order=None) -> np.ndarray:
    """The candidates as the kernel's 528-B records (a flat uint8 array), in `order` when given."""
    cands = list(cands)
    if order is not None:
        cands = [cands[i] for i in order]
    out = bytearray()
    for b, blk in cands:
        out += struct.pack("<QQ", b, 0) + blk
    return np.frombuffer(bytes(out) or b"\0", dtype=np.uint8).copy()[:len(out)]


def parse_records(buf, n):
    """The set of (block index, 512 bytes) of the first n records of a byte buffer."""
    raw = bytes(buf[:n * RECORD])
    out = set()
    for i in range(n):
        r = raw[i * RECORD:(i + 1) * RECORD]
        b, pad = struct.unpack("<QQ", r[:16])
        assert pad == 0
        out.add((b, r[16:]))
    assert len(out) == n  # no candidate twice
    return out


def set_checksum(block: bytearray, signed=False):
    """Writes the header's checksum field as tar writers do (six octal digits, NUL, space)."""
    block[148:156] = b" " * 8
    s = sum(c - 256 if (signed and c >= 0x80) else c for c in block)
    block[148:156] = b"%06o\x00 " % s
    return block


def header(name: bytes, size: int, typeflag=b"0") -> bytearray:
    h = bytearray(512)
    h[:len(name)] = name
    h[100:108] = b"0000644\x00"
    h[108:116] = b"0000000\x00"
    h[116:124] = b"0000000\x00"
    h[124:136] = b"%011o\x00" % size
    h[136:148] = b"00000000000\x00"
    h[156:157] = typeflag
    h[257:265] = b"ustar\x0000"
    return set_checksum(h)


def pad512(b: bytes) -> bytes:
    return b + b"\0" * (-len(b) % 512)


# ---- the layers the tests share ---------------------------------------------
AWS = b"AKIA" + b"Q" * 16
GH = b"ghp_" + b"a1B2" * 9


def nested_layer() -> bytes:
    """make_layer(7, 40) as one member, opt/service/conf/inner.tar, and a text file after it: the inner
    archive's headers are candidates that are not on the chain."""
    inner = make_layer(7, 40)
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w", format=tarfile.GNU_FORMAT) as tf:
        ti = tarfile.TarInfo("opt/service/conf/inner.tar")
        ti.size = len(inner)
        tf.addfile(ti, io.BytesIO(inner))
        text = b"# after the inner archive\naws_access_key_id = " + AWS + b"\n"
        ti = tarfile.TarInfo("opt/service/conf/after.conf")
        ti.size = len(text)
        tf.addfile(ti, io.BytesIO(text))
    return buf.getvalue()


def pax_size_layer() -> bytes:
    """A hand-built PAX 'x' header whose size= record (700) differs from the entry header's size field
    (100): the chain must follow the PAX size.  Where the header's own size would put the next header
    (512 bytes into the data) lies a valid header, a decoy that is file content and not on the chain."""
    text = (b"line one\ntoken = " + GH + b"\n").ljust(511, b"x") + b"\n"
    data = text + bytes(header(b"etc/decoy.conf", 0))  # 1,024 bytes, of which 700 are the file
    recs = b""
    for kv in (b"path=etc/pax.conf", b"size=700"):
        n = len(kv) + 3
        while len(b"%d %s\n" % (n, kv)) != n:
            n = len(b"%d %s\n" % (n, kv))
        recs += b"%d %s\n" % (n, kv)
    out = bytes(header(b"PaxHeaders/pax.conf", len(recs), b"x")) + pad512(recs)
    out += bytes(header(b"etc/short-name", 100)) + data
    tail = b"second = " + AWS + b"\n"
    out += bytes(header(b"etc/second.conf", len(tail))) + pad512(tail)
    return out + b"\0" * 1024


def no_trailer_layer() -> bytes:
    """A layer without end-of-archive blocks whose last file's data ends exactly at its last byte."""
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w", format=tarfile.GNU_FORMAT) as tf:
        for i, text in enumerate([b"first = " + GH + b"\n", (b"k = v\n" * 80 + b"id = " + AWS + b"\n").ljust(1024, b"#")]):
            ti = tarfile.TarInfo("srv/app/%d.conf" % i)
            ti.size = len(text)
            tf.addfile(ti, io.BytesIO(text))
    data = buf.getvalue()
    end = 512 + 512 + 512 + 1024  # header, data (padded), header, 1024 bytes of data
    assert len(data) >= end and not any(data[end:])
    return data[:end]


def ustar_prefix_layer() -> bytes:
    """USTAR cannot hold names over 255 bytes: one with prefix-split names (tests/test_analyzer.py's)."""
    from tests.corpus import make_corpus
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w", format=tarfile.USTAR_FORMAT) as tf:
        for i, (p, b) in enumerate(make_corpus(77, 80)):
            ti = tarfile.TarInfo("opt/data/some/long/prefix/dir/%s/%d/%s" % ("q" * 60, i, p))
            ti.size = len(b)
            tf.addfile(ti, io.BytesIO(b))
    return buf.getvalue()


def kernel_blocks():
    """Single blocks for the kernel's edge cases: (name, 512 bytes, candidate?)."""
    out = []
    h = header(b"caf\xc3\xa9/\xff\xfe\x80name.txt", 10)
    set_checksum(h, signed=True)  # right only as a signed sum: the name has bytes >= 0x80
    assert sum(h[:148]) + sum(h[156:]) + 256 != parse_numeric(bytes(h[148:156]))
    out.append(("signed-only", bytes(h), True))
    h = header(b"etc/octal.conf", 10)
    h[153:154] = b"8"  # the sum does not depend on the field: right sum, a field that is not octal
    out.append(("non-octal", bytes(h), False))
    for k in range(1000):  # the field holds the sum of the block as it is, its own bytes included
        h = header(b"etc/self-%d.conf" % k, 10)
        rest = sum(h[:148]) + sum(h[156:])
        fixed = [s for s in range(rest + 320, rest + 363) if rest + sum(b"%06o\x00 " % s) == s]
        if fixed:
            h[148:156] = b"%06o\x00 " % fixed[0]
            assert sum(h) == parse_numeric(bytes(h[148:156]))
            out.append(("own-bytes-not-spaces", bytes(h), False))
            break
    else:
        raise AssertionError("no self-summing header found")
    h = header(b"etc/base256.conf", 10)
    h[148:156] = bytes([0x80]) + parse_numeric(bytes(h[148:156])).to_bytes(7, "big")
    out.append(("base-256", bytes(h), True))
    h = header(b"etc/spaces.conf", 10)
    h[148:156] = b" %05o \x00" % parse_numeric(bytes(h[148:156]))
    out.append(("padded-octal", bytes(h), True))
    out.append(("zero", bytes(512), False))
    for name, blk, want in out:
        assert is_candidate(blk) == want, name
    return out


def planted_random(seed=5, n_blocks=3000, n_planted=200):
    """Random bytes with valid headers planted at random blocks."""
    rng = random.Random(seed)
    data = bytearray(np.random.RandomState(seed).randint(0, 256, 512 * n_blocks, dtype=np.uint8).tobytes())
    at = sorted(rng.sample(range(n_blocks), n_planted))
    for k, b in enumerate(at):
        data[512 * b:512 * b + 512] = header(b"planted/%d.txt" % k, rng.randint(0, 1 << 20))
    return bytes(data), at
