"""A pure-Python model of the Required stage of a resident tar layer with its skip stage
(trivy_amd/csrc/tarrequired.h, tar_skip_dev.h; tsg_analyzer_set_tar_required_skip mode 1):
tests/tar_required_model.py's decisions, then the pattern matcher of the four device forms, then the
three-case under rule, then the same outputs -- a verdict per entry, the 48-B file records, the path blob
and 16 words of counts per layer, every byte the stage writes.

The forms (cleaned patterns): L | **/L | L/** | **/*S, with L a non-empty ASCII literal of at most 255 bytes
without * ? [ ] { } \\ whose elements are neither empty nor "." nor "..", S such a literal without '/'.
"""
import numpy as np

from tests import tar_chain_model as cm
from tests import tar_required_model as rm

SKIP_DIR, SKIP_FILE, SKIP_UNDER = 8, 9, 10
EXACT, ANY_DIR, BELOW, SUFFIX = range(4)
MAX_PATTERNS, MAX_LITERAL, MAX_BYTES = 32, 255, 2048
SPECIAL = b"*?[]{}\\"


def literal_ok(lit: bytes, slashes: bool) -> bool:
    if not lit or len(lit) > MAX_LITERAL or any(c >= 0x80 or c in SPECIAL for c in lit):
        return False
    if not slashes and b"/" in lit:
        return False
    return all(e not in (b"", b".", b"..") for e in lit.split(b"/"))


def form_of(p: bytes):
    """(form, literal) of one cleaned pattern, or None when the device does not take it."""
    if p.startswith(b"**/*"):
        return (SUFFIX, p[4:]) if literal_ok(p[4:], False) else None
    if p.startswith(b"**/"):
        f, lit = ANY_DIR, p[3:]
    elif len(p) > 3 and p.endswith(b"/**"):
        f, lit = BELOW, p[:-3]
    else:
        f, lit = EXACT, p
    return (f, lit) if literal_ok(lit, True) else None


def classify(dirs, files):
    """The forms of an option set ([(form, literal)] for dirs, the same for files), or None when a pattern or
    the set is outside what the device takes."""
    if len(dirs) > MAX_PATTERNS or len(files) > MAX_PATTERNS:
        return None
    out = [[form_of(p) for p in ps] for ps in (dirs, files)]
    if any(f is None for fs in out for f in fs):
        return None
    if sum(len(f[1]) for fs in out for f in fs) > MAX_BYTES:
        return None
    return out


def match_one(form, lit: bytes, fp: bytes) -> bool:
    if form == EXACT:
        return fp == lit
    if form == ANY_DIR:
        return fp == lit or fp.endswith(b"/" + lit)
    if form == BELOW:
        return fp == lit or fp.startswith(lit + b"/")
    return fp.rsplit(b"/", 1)[-1].endswith(lit)


def match(forms, fp: bytes) -> bool:
    return any(match_one(f, lit, fp) for f, lit in forms)


def under(fp: bytes, rank: int, first: dict, parent_first: dict) -> bool:
    """The three-case rule: fp is a recorded directory, lies below one, or is the direct parent of one -- recorded
    at a rank below `rank`.  first: path -> lowest rank; parent_first: direct parent -> lowest rank."""
    if first.get(fp, rank) < rank or parent_first.get(fp, rank) < rank:
        return True
    at = fp.find(b"/")
    while at >= 0:
        if first.get(fp[:at], rank) < rank:
            return True
        at = fp.find(b"/", at + 1)
    return False


def record(first: dict, parent_first: dict, fp: bytes, rank: int):
    first[fp] = min(first.get(fp, rank), rank)
    sl = fp.rfind(b"/")
    if sl > 0:
        parent_first[fp[:sl]] = min(parent_first.get(fp[:sl], rank), rank)


def stage(recs, n: int, names: bytes, rec_base, name_base, cfg: bytes, pt, st, skip_dirs, skip_files):
    """(verdicts, file records, blob, counts) as tar_required_model.stage gives them, with the skip stage.
    skip_dirs / skip_files: cleaned patterns (bytes) the device takes."""
    forms = classify(list(skip_dirs), list(skip_files))
    assert forms is not None
    dir_forms, file_forms = forms
    raw, names = bytes(recs[:64 * n]), bytes(names)
    n_layers = len(rec_base) - 1
    verdicts = np.zeros(n, dtype=np.uint8)
    frecs, blob = bytearray(), bytearray()
    counts = np.zeros((n_layers, 16), dtype=np.uint64)
    memo = {}
    for k in range(n_layers):
        lb, le = int(name_base[k]), int(name_base[k + 1])
        ents = []  # [verdict, start, data, size, typeflag, fp or raw name, rules, all_rules, n_ext]
        for i in range(int(rec_base[k]), int(rec_base[k + 1])):
            start, _hdr, data, size, off, ln, typeflag, _flags, n_ext, _pad = cm.REC.unpack(raw[64 * i:64 * i + 64])
            if off > le - lb or ln > le - lb - off:
                ents.append([rm.BAD, start, data, size, typeflag, b"", 0, 0, n_ext])
                continue
            name = names[lb + off:lb + off + ln]
            key = (name, typeflag, size)
            if key not in memo:
                memo[key] = rm.decide(name, typeflag, size, cfg, pt, st)
            v, skip, out_len, rules, all_rules = memo[key]
            fp = name[skip:skip + out_len]
            if v == rm.OTHER and (typeflag == 0x35 or (typeflag == 0 and name.endswith(b"/"))) and match(dir_forms, fp):
                v = SKIP_DIR
            elif v in (rm.DROP, rm.KEEP, rm.ASK_ALLOW) and match(file_forms, fp):
                v = SKIP_FILE
            ents.append([v, start, data, size, typeflag, fp, rules, all_rules, n_ext])
        first, parent_first = {}, {}
        for e in ents:
            if e[0] == SKIP_DIR:
                record(first, parent_first, e[5], e[1])
        for e in ents:
            if e[0] in (rm.DROP, rm.KEEP, rm.ASK_ALLOW) and under(e[5], e[1], first, parent_first):
                e[0] = SKIP_UNDER
        cnt = dict.fromkeys(rm.COUNTS, 0)
        cnt["rec_first"], cnt["path_first"] = len(frecs) // 48, len(blob)
        tot = [0] * 11
        for i, e in zip(range(int(rec_base[k]), int(rec_base[k + 1])), ents):
            v, start, data, size, typeflag, fp, rules, all_rules, n_ext = e
            verdicts[i] = v
            tot[v] += 1
            cnt["ext_headers"] += n_ext
            if v in (rm.KEEP, rm.ASK_ALLOW, rm.ASK_NAME, SKIP_DIR):
                frecs += rm.FREC.pack(start, data, size, len(blob) - cnt["path_first"], len(fp), typeflag, v, all_rules,
                                      0, rules)
                blob += fp + b"\0"
        cnt.update(entries=len(ents), whiteouts=tot[rm.WHITEOUT], opaque_dirs=tot[rm.OPAQUE], dropped=tot[rm.DROP],
                   kept=tot[rm.KEEP], ask_allow=tot[rm.ASK_ALLOW], ask_name=tot[rm.ASK_NAME], bad=tot[rm.BAD],
                   regular=tot[rm.DROP] + tot[rm.KEEP] + tot[rm.ASK_ALLOW] + tot[SKIP_FILE] + tot[SKIP_UNDER],
                   records=len(frecs) // 48 - cnt["rec_first"], path_bytes=len(blob) - cnt["path_first"],
                   pad0=tot[SKIP_DIR], pad1=tot[SKIP_FILE] | (tot[SKIP_UNDER] << 32))
        counts[k] = [cnt[c] for c in rm.COUNTS]
    return verdicts, bytes(frecs), bytes(blob), counts
