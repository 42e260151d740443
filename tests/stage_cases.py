"""The batches of the engine stage tests (test helper): the smallest shapes at which the
kernels of trivy_amd/csrc/engine.hip can go wrong.  tests/test_stage_model.py checks on the
CPU that each case holds what its name promises (with the models alone);
tests/test_gpu_stages.py runs them through the engine.

A case is a dict: rules, batch (stage_model.Batch), env (the engine's variant switches),
and `min`: lower bounds on (hits, candidates, true matches) that keep a comparison from
passing on nothing.
"""
import random

import numpy as np

from tests.stage_model import DROP, NL_REACH, RUNE_I, RUNE_K, RUNE_S, Batch, StageModel
from trivy_amd.secret import builtin_rules
from trivy_amd.secret.config import Rule

ALNUM = b"ABCDEFGHJKLMNPQRSTUVWXYZabcdefghjkmnpqrstuvwxyz23456789"
LINE = b"lorem ipsum dolor sit amet, consectetur elit sed do eiusmod\n"  # 60 bytes, no keyword, no anchor


def _rs(rng, alphabet, n):
    return bytes(rng.choice(alphabet) for _ in range(n))


def tok_ghp(rng):      # github-pat: one follow run
    return b" ghp_" + _rs(rng, ALNUM, 36) + b" "


def tok_aws(rng):      # aws-access-key-id: gated by its own literal, not implied
    return b" AKIA" + _rs(rng, b"ABCDEFGHIJKLMNOPQRSTUVWXYZ234567", 16) + b" "


def tok_a3t(rng):      # aws-access-key-id through the alternative that holds no keyword
    return b" A3TX" + _rs(rng, b"BCDEFGHJLMNOPQRSTUVWXYZ234567", 16) + b" "


def tok_hook(rng):     # slack-web-hook: two follow runs, gated by a keyword its literal holds
    return b" https://hooks.slack.com/services/" + _rs(rng, ALNUM, 46) + b" "


def tok_stripe(rng):   # stripe-secret-token: (?i), literal at offset 3..7
    return b" sk_live_" + _rs(rng, b"0123456789abcdefghijklmnopqrstuvwxyz", 24) + b" "


TOKENS = (tok_ghp, tok_aws, tok_hook, tok_stripe)


def filler(n):
    return (LINE * (n // len(LINE) + 1))[:n]


class Planter:
    """Overwrites filler with tokens, never two in the same place."""

    def __init__(self, n):
        self.buf = bytearray(filler(n))
        self.used = []

    def put(self, at, tok):
        if at < 0 or at + len(tok) > len(self.buf):
            return False
        if any(at < e + 2 and s < at + len(tok) + 2 for s, e in self.used):
            return False
        self.buf[at:at + len(tok)] = tok
        self.used.append((at, at + len(tok)))
        return True


def boundary_file(n_bytes=208 * 1024, seed=1):
    """One file at arena offset 0 (so file and arena positions agree) with tokens whose match start
    lies at -16 .. +7 and whose anchor literal ends at about -11 .. +12 around boundaries of every
    kind: 24 boundaries per kind, one offset each; every 4-KiB tile boundary (offset k mod 24), which
    are the wave boundaries of a capped K1 grid (16 KiB) and, uncapped, the boundaries between
    workgroups' tiles (64 KiB: three in this file, with match starts 1 and 9 bytes before and 7 bytes behind)."""
    rng = random.Random(seed)
    p = Planter(n_bytes)
    n = 0
    kinds = {
        16: [4096 + 176 + 192 * j for j in range(80)],                # multiples of 16, not of 64
        64: [20480 + 64 + 256 * j for j in range(80)],                # multiples of 64, not of 1024
        1024: [32768 + 1024 * j for j in range(1, 40) if j % 4],      # multiples of 1 KiB, not of 4 KiB
    }
    for kind, cands in kinds.items():
        k = 0
        for B in cands:
            if k == 24:
                break
            if kind < 1024 and not 300 < B % 4096 < 3700:
                continue
            assert B % kind == 0
            if p.put(B - 16 + k, TOKENS[n % 4](rng)):
                k += 1
                n += 1
        assert k == 24, kind
    for k, B in enumerate(range(4096, n_bytes - 200, 4096)):
        assert p.put(B - 16 + k % 24, TOKENS[n % 4](rng)), B
        n += 1
    return bytes(p.buf), n


def case_boundaries(calibration=None):
    """calibration: a sample for the compiler's anchor choice (the tables differ, the batch does not)."""
    body, n = boundary_file()
    small = [b"", filler(100) + tok_ghp(random.Random(2)) + b"\n", b"x",
             b"heroku_key = '0A1B2C3D-1111-2222-3333-0A1B2C3D4E5F'\n"]
    return {"rules": builtin_rules(), "batch": Batch([body] + small), "min": (n, n, n), "calibration": calibration}


def case_arena_edges(k):
    """Tokens at arena offset k (zero bytes before the arena in K1's window) and ending k bytes before
    the arena's end; a last file ending in a bare anchor literal (its follow span is the file's end)."""
    rng = random.Random(30 + k)
    first = filler(k)[:k] + tok_ghp(rng)[1:] + filler(300) + tok_aws(rng) + b"\n"
    mid = filler(700) + tok_hook(rng) + filler(40)
    last = filler(500) + tok_stripe(rng) + b"\n" + tok_ghp(rng)[:-1] + filler(k)[:k]
    files = [first, mid, last]
    if k % 2:
        files.append(filler(33) + b" ghp_")  # the literal ends with the arena
    return {"rules": builtin_rules(), "batch": Batch(files), "min": (4, 4, 4)}


def case_files():
    """File lengths 0, 1, 5, 15, 16, 17, 1023, 1024, 1025; runs of empty files at a chunk start; a
    token cut between two files at every position; a keyword cut between two files; a last file
    ending in an anchor literal and half a token whose other half is the arena's tail."""
    rng = random.Random(5)
    files = []
    for n in (0, 1, 5, 15, 16, 17, 1023, 1024, 1025):
        files.append(filler(n))
        files.append((tok_ghp(rng)[1:] + filler(n))[:n] if n >= 41 else filler(n)[::-1])
    pad = (-sum(len(x) for x in files)) % 1024
    files.append(filler(pad))            # the next files start a 1-KiB chunk
    files += [b"", b"", b"", tok_aws(rng) + filler(100), b"", b""]
    cut_from = len(files)
    tok = tok_ghp(rng)
    for cut in range(2, len(tok) - 1):   # halves of a token in adjacent files: no candidate
        files += [filler(7) + tok[:cut], tok[cut:] + filler(9)]
    cut_to = len(files)
    lit_to = cut_from + 2 * 7            # cuts inside ' ghp_' and the four bytes of its follow run: no hit either
    kw_from = len(files)
    for cut in range(1, 15):             # a keyword cut over two files: no bit
        files += [filler(20) + b"hooks.slack.com"[:cut], b"hooks.slack.com"[cut:] + filler(20)]
    kw_to = len(files)
    files.append(filler(300) + tok_stripe(rng) + filler(50) + b" ghp_Ab")
    # the tail completes the follow run and the token, and holds keywords
    tail = (b"3Ab3" + b"Cd5" * 11 + b" hooks.slack.com AKIA ")[:64].ljust(64, b"z")
    return {"rules": builtin_rules(), "batch": Batch(files, tail), "min": (3, 3, 3),
            "no_cands": range(cut_from, cut_to), "no_hits": range(cut_from, lit_to), "no_kw": range(kw_from, kw_to), "tail_file": len(files) - 1}


def case_tail(fill):
    """The same batch with the 64 bytes behind the arena full of newlines, or of a fold rune: no
    newline count, no hint and no flag may come from them."""
    c = case_files()
    b = c["batch"]
    c["batch"] = Batch(b.contents[:-1] + [b.contents[-1] + b"\n" + filler(10)], (fill * 64)[:64])
    return c


def case_dense():
    """Back-to-back anchor literals: 16-B blocks with five and more window ends that fire (K2's
    register queue overflows into its in-place path)."""
    rng = random.Random(8)
    runs = [b"ghp_" * 60, b"AKIAAKIA" * 30, b"sk_live_" * 30, b"ghp_AKIAxoxb-ghp_" * 20, b"xoxb-xoxp-" * 30]
    body = b"".join(filler(50 + 13 * i) + r + tok_ghp(rng) for i, r in enumerate(runs))
    return {"rules": builtin_rules(), "batch": Batch([body, runs[0], filler(64) + runs[3]]), "min": (20, 5, 5)}


def case_follow():
    """Follow requirements: spans that cross the file's end, that hold a byte >= 0x80, that fail at
    exactly the first / last allowed offset, anchors with two requirement runs."""
    rng = random.Random(9)
    files = []
    ghp = tok_ghp(rng)
    for cut in range(5, 12):                      # ' ghp_' + 0..6 bytes: the run does not fit the file
        files.append(filler(30) + ghp[:cut])
    files.append(filler(30) + b" ghp_\xc3\xa9" + ghp[5:])       # a two-byte rune right behind the literal
    files.append(filler(30) + b" ghp_Ab\xe2\x82\xac" + ghp[5:])
    files.append(filler(30) + b" ghp_A-bc" + ghp[5:])           # the run fails in its second byte
    files.append(filler(30) + b" ghp_Abc-" + ghp[5:])           # ... in its last byte
    files.append(filler(30) + ghp)
    hook = tok_hook(rng)                          # slack-web-hook: runs at fixed offsets 2 and 7 of the literal end
    for k in range(1, 14):
        broken = bytearray(hook)
        broken[len(b" https://hooks.slack.com") + k - 1] = ord("!")
        files.append(filler(20) + bytes(broken))
        files.append(filler(20) + hook[:len(b" https://hooks.slack.com") + k])
    # heroku / facebook: two runs with offset ranges; the separator at the first and the last offset
    for pad in (0, 1, 24, 25, 26):
        files.append(b"facebook" + b"_" * pad + b" = '" + _rs(rng, b"abcdef0123456789", 32) + b"'\n")
        files.append(b"heroku" + b" " * pad + b": \"" + b"0A1B2C3D-1111-2222-3333-0A1B2C3D4E5F" + b"\"\n")
        files.append(b"facebook" + b"_" * pad + b" # " + _rs(rng, b"abcdef0123456789", 32) + b"'\n")
    # the span crosses the file's end behind the item's own lookahead: run starts are cut to the file
    files.append(b"facebook_" + b"a" * 20)
    files.append(b"facebook = 'abcdef0123456789")
    files.append(b"twitter" + b" " * 22 + b"= '")
    # a rune inside the span: the offsets are not fixed, the hit is left to the NFA
    files.append(b"facebook_" + b"a" * 17 + b"\xc3\xa9 # no separator, no secret\n")
    files.append(b"heroku " + b"b" * 18 + b"\xe2\x82\xac # nothing\n")
    files.append(b"facebook_" + b"a" * 17 + b"e # no separator, no secret, no rune\n")
    return {"rules": builtin_rules(), "batch": Batch(files), "min": (10, 4, 4)}


CLASS_RUN_SRCS = [r"(?i)\b[g-z]{3}[0-9]{3}[._-][a-z0-9]{12}\b", r"[a-f]{2}[0-9]{2}_[a-z]+_end[0-9]",
                  r"[0-9]{3}-[0-9]{4}-[0-9]{3}", r"(?i)(?:^|\s)[k-s]{2}[0-9]{4}[:=][A-Z0-9]{8}",
                  r"x?[0-9]{2}\.[0-9]{2}\.[0-9]{4}-[a-z]{2}"]  # tests/test_filter_model.py


def class_run_rules():
    return builtin_rules() + [Rule(ID="cr%d" % i, Category="C", Title="t", Severity="LOW", Regex=s)
                              for i, s in enumerate(CLASS_RUN_SRCS)]


def case_class_runs():
    """The boundary sweep with tokens of rules anchored on runs of one-byte classes."""
    body, n = boundary_file()
    rng = random.Random(12)
    p = Planter(len(body))
    p.buf[:] = body
    extra = 0
    toks = [lambda: b" pqr777.abcdef123456 ", lambda: b" ab12_" + _rs(rng, b"qrstuv", 20) + b"_end7 ",
            lambda: b" 555-1234-999 ", lambda: b" kq1234=ABCD1234 ", lambda: b" 12.34.5678-ab "]
    for k, B in enumerate(range(4096 + 2048, len(body) - 200, 4096)):
        if p.put(B - 16 + k % 24, toks[k % 5]()):
            extra += 1
    for k in range(24):
        if p.put(70000 + 320 * k + 16 * (k % 4) - 16 + k, toks[k % 5]()):
            extra += 1
    assert extra > 60
    return {"rules": class_run_rules(), "batch": Batch([bytes(p.buf), b" 555-1234-999", b""]),
            "min": (n + 40, n + 40, n + 40)}


def case_fold():
    """Files holding each fold rune, runes straddling 16-B / 1-KiB / 4-KiB boundaries, truncated rune
    prefixes, keywords spelled through U+0130 / U+212A, tokens beside the runes."""
    rng = random.Random(14)
    files = [filler(100) + r + filler(50) + t(rng) for r in (RUNE_I, RUNE_K, RUNE_S) for t in (tok_ghp, tok_a3t)]
    for B in (16, 1024, 4096):
        for r in (RUNE_I, RUNE_K, RUNE_S):
            for back in range(1, len(r)):        # the rune starts `back` bytes before arena boundary B
                pre = (-sum(len(x) for x in files)) % 4096
                files.append(filler(pre + B - back) + r + filler(30) + tok_stripe(rng))
    files += [filler(10) + r[:n] for r in (RUNE_I, RUNE_K, RUNE_S) for n in range(1, len(r))]  # prefixes: no flag
    files += [filler(10) + r[:n] + b"x" + r[n:] for r in (RUNE_I, RUNE_K, RUNE_S) for n in range(1, len(r))]
    K, I = RUNE_K, RUNE_I
    for kw in (b"a" + K + I + b"a", b"A" + K + b"ia", b"hoo" + K + b"s.slac" + K + b".com", b"hooks.slack.com",
               b"a" + K + K + b"a", b"ak" + I + I + b"a"):
        files.append(filler(200) + kw + filler(100) + tok_a3t(rng) + tok_hook(rng).replace(b"hooks.slack.com", kw))
    files.append(filler(64) + RUNE_S + b" sk_live_" + _rs(rng, b"0123456789abcdef", 24) + b" ")
    return {"rules": builtin_rules(), "batch": Batch(files), "min": (5, 5, 10)}


FULLSCAN_RULES = [
    Rule(ID="tok", Category="Custom", Title="Token", Severity="HIGH",
         Regex=r"(?i)\b[g-z]{3}[0-9]{3}[._-][a-z0-9]{12}\b", Keywords=["gatekw"]),
    Rule(ID="digits", Category="Custom", Title="Digits", Severity="LOW", Regex=r"[0-9]{3}-[0-9]{4}-[0-9]{3}",
         Keywords=["call"]),
    Rule(ID="long", Category="Custom", Title="Long run", Severity="LOW", Regex=r"[a-f]{2}[0-9]{2}_[a-z]+_end[0-9]"),
]


def case_fullscan():
    """Unanchored rules (TSG_CLASS_RUNS=0 at compile time) at TSG_FULLSCAN_CHUNK=4096: tokens at
    and across the 4-KiB lane chunks, files whose gate is closed."""
    rng = random.Random(16)
    files = []
    for i in range(6):
        p = Planter(9000 + 4096 * i)
        for k in range(1, 2 + i):
            p.put(4096 * k - 10 + 3 * i, b" pqr%03d.abcdef123456 " % rng.randrange(1000))
            p.put(4096 * k - 2000, b" %03d-4567-%03d " % (rng.randrange(1000), rng.randrange(1000)))
        body = bytes(p.buf)
        if i % 2 == 0:
            body = b"gatekw\n" + body
        if i % 3 == 0:
            body += b"CALL me\n"
        files.append(body)
    files.append(filler(5000) + b" ab12_" + b"q" * 9000 + b"_end7 " + filler(100))
    files += [b"", b" 123-4567-890"]
    return {"rules": builtin_rules() + FULLSCAN_RULES, "batch": Batch(files), "min": (0, 8, 8),
            "env": {"TSG_FULLSCAN_CHUNK": "4096"}, "compile_env": {"TSG_CLASS_RUNS": "0"}}


def case_gates():
    """A gated rule whose regex matches in a file without the keyword; with the keyword in the
    other case only; with the keyword only through U+212A / U+0130."""
    rng = random.Random(18)
    a3t = tok_a3t(rng)
    files = [filler(300) + a3t + filler(100),                                  # no keyword: closed
             filler(300) + a3t + filler(100) + b" akia " + filler(20),         # lower case only
             filler(300) + a3t + filler(100) + b" AKIA " + filler(20),
             filler(300) + a3t + filler(100) + b" a" + RUNE_K + RUNE_I + b"a " + filler(20),   # through runes
             filler(300) + a3t + filler(100) + b" " + RUNE_K + RUNE_I + b" " + filler(20),     # runes, no keyword
             filler(100) + tok_hook(rng).replace(b"hooks", b"HOOKS") + filler(10),
             filler(100) + tok_aws(rng) + filler(10)]
    return {"rules": builtin_rules(), "batch": Batch(files), "min": (5, 4, 4), "closed": [(0, "aws-access-key-id")]}


def case_finalize():
    """One ~2.3-MiB file that is a single line except for newlines at chosen distances from the
    window starts of planted tokens (a candidate carries its three nearest newlines each way, so
    each token gets three distances per side):
      at the file's start      after: 1023, 1024
      near the start (odd)     before: 1, 15, 16; after: the token's end + 1, 15, 16
      16-B aligned             before: 17, 1023, 1024; after: the token's end + 17, then 1023, 1024
      two in the middle, 61 B apart, the first 1-KiB aligned in the arena: 2^20 - 1, 2^20 and 2^20 + 1025 before
      and after each (the first sees 2^20 forwards, the second backwards, among its nearest three)
      the file's last bytes    before: 17, 1023, 1024; after: none
    Around it files of newlines only (a hint that leaks over a file boundary shows), a file
    without a newline, and tokens with exactly 0..3 newlines before and after them."""
    rng = random.Random(20)
    M = 1 << 20
    n = 2 * M + 300 * 1024
    big = bytearray(b"x" * n)

    def put(wlo, tok=None):     # ' ghp_...' with its window start (literal start - 4) at wlo
        t = tok_ghp(rng) if tok is None else tok
        big[wlo + 3:wlo + 3 + len(t)] = t
        return wlo + 3 + len(t)  # the token's end

    def nls(*at):
        for p in at:
            assert 0 <= p < n and big[p] == ord("x"), p
            big[p] = 10

    first = tok_ghp(rng)[1:]
    big[0:len(first)] = first
    nls(1023, 1024)
    w = 6001
    e = put(w)
    nls(w - 1, w - 15, w - 16, e + 1, e + 15, e + 16)
    w = 20 * 1024 + 16
    e = put(w)
    nls(w - 17, w - 1023, w - 1024, e + 17, w + 1023, w + 1024)
    a = M + 150 * 1024
    for w in (a, a + 61):
        put(w)
        nls(w - (M - 1), w - M, w - (M + 1025), w + (M - 1), w + M, w + (M + 1025))
    last = tok_ghp(rng)[:-1]
    w = n - len(last) - 3
    assert put(w, last) == n
    nls(w - 17, w - 1023, w - 1024)
    files = [b"\n" * 1024, bytes(big), b"\n" * 1030, filler(59)[:-1] + tok_ghp(rng) + filler(59)[:-1], b"\n" * 5]
    for before in range(4):
        for after in range(4):
            files.append(b"a\n" * before + b"bb" + tok_ghp(rng) + b"cc" + b"\nd" * after)
    return {"rules": builtin_rules(), "batch": Batch(files), "min": (20, 20, 20)}


_MODELS = {}


def model_of(case, monkeypatch):
    """The StageModel of a case's rules, compiled under the case's compile-time switches (cached)."""
    cenv = case.get("compile_env") or {}
    calib = case.get("calibration")
    key = (tuple(r.ID for r in case["rules"]), tuple(sorted(cenv.items())), hash(calib))
    if key not in _MODELS:
        with monkeypatch.context() as m:
            for k, v in cenv.items():
                m.setenv(k, v)
            _MODELS[key] = StageModel(case["rules"], calibration=calib)
    if calib is not None:
        assert _MODELS[key].fm.n_calibrated >= 1
    return _MODELS[key]


def _rule(model, rule_id):
    return [r.ID for r in model.rules].index(rule_id)


def check_case(case, d, e, model):
    """What a case asserts of a dump beyond the invariants every case shares."""
    b = case["batch"]
    hit_files = {h[0] for h in d.hits}
    cand_files = {int(x["file"]) for x in d.cands}
    for f in case.get("no_cands", ()):       # the halves of a token cut between two files
        assert f not in cand_files, f
    for f in case.get("no_hits", ()):        # ... cut inside the anchor literal or its follow run
        assert f not in hit_files, f
    for f in case.get("no_kw", ()):          # the halves of a keyword
        assert not d.kw[f].any(), f
    if "tail_file" in case:                  # nothing from the 64 bytes behind the arena
        f, r = case["tail_file"], _rule(model, "github-pat")
        assert not any(h[0] == f and model.anchors[h[2]][0] == r for h in d.hits)
        assert not any(int(x["file"]) == f and int(x["rule"]) == r for x in d.cands)
        for kw in (b"hooks.slack.com", b"akia"):
            assert not d.kw_bit(f, model.keywords.index(kw))
        assert int(d.nl[-1]) == b.arena[len(d.nl) * 1024 - 1024:].count(b"\n")
    for f, rule_id in case.get("closed", ()):
        r = _rule(model, rule_id)
        assert not any(int(x["file"]) == f and int(x["rule"]) == r and not int(x["flags"]) & DROP for x in d.cands)
    # no candidate survives for a (file, rule) whose gate the oracle says is closed
    closed = {}
    for x in d.cands:
        key = (int(x["file"]), int(x["rule"]))
        if key not in closed:
            closed[key] = not model.match_keywords(key[1], b.contents[key[0]])
        info = model.info[key[1]]
        inexact = int(d.flags[key[0]]) & 4 and not e.kw_fold  # (the host re-checks those files' gates)
        if closed[key] and info["gate"] == 1 and not info["implied"] and not inexact:
            assert int(x["flags"]) & DROP, key


def check_case_shape(name, case, e, model):
    """The case holds what its name promises (by the models alone)."""
    b = case["batch"]
    if name == "dense":       # as tests/test_gpu_parity.py test_blocks_with_many_fires
        fr = model.fm.fires(b.a)[:model.fm.n_buckets - 1].any(axis=0)
        per_block = np.bincount(np.nonzero(fr)[0] >> 4)
        assert (per_block >= 5).sum() >= 10, per_block.max()
    if name == "follow":
        dropped = set(e.all_hits) - set(e.hits_required)
        assert len(dropped) >= 8 and len(e.hits_required) >= 10
        runs = {len(model.reqs[h[2]]) for h in e.all_hits}
        assert runs >= {1, 2}
        spans = [(h, max(hi + len(s) for lo, hi, s in model.reqs[h[2]])) for h in e.hits_required]
        assert any(any(c >= 0x80 for c in b.contents[h[0]][h[1]:h[1] + n]) for h, n in spans)   # kept by a rune
        assert any(h[1] + n > len(b.contents[h[0]]) for h, n in [(h, max(
            hi + len(s) for lo, hi, s in model.reqs[h[2]])) for h in e.all_hits])               # spans past the end
    if name.startswith("arena-edges"):
        assert any(int(b.offs[h[0]]) + h[1] <= 12 for h in e.hits_required)
        assert any(int(b.offs[h[0]]) + h[1] >= b.n_bytes - 100 for h in e.hits_allowed)
    if name in ("files", "tail-newlines", "tail-rune"):
        lens = {len(x) for x in b.contents}
        assert lens >= {0, 1, 5, 15, 16, 17, 1023, 1024, 1025}
        starts = [int(b.offs[f]) for f in range(b.n_files) if not b.contents[f]]
        assert sum(1 for s in starts if s % 1024 == 0 and s) >= 3
    if name == "fold":
        assert {int(x) for x in e.flags} >= {0, 3, 5}
        k = model.keywords.index(b"akia")
        through = [f for f in range(b.n_files) if (f, k) in e.kw_bits and b"akia" not in b.contents[f].lower()]
        assert len(through) >= 2
    if name == "gates":
        k = model.keywords.index(b"akia")
        assert [(f, k) in e.kw_bits for f in range(5)] == [False, True, True, True, False]
    if name == "fullscan":
        assert sum(1 for i in model.info if not i["anchored"]) >= 3
    if name == "finalize":
        seen_b, seen_f, none, aligned = set(), set(), 0, set()
        for (f, r, wlo, whi) in e.cands_required:
            _, back, fwd = model.hints(b.contents[f], wlo)
            if NL_REACH in fwd:     # the window start's alignment in the arena decides where the walk's steps fall
                aligned.add((int(b.offs[f]) + wlo) % 1024 == 0)
            if NL_REACH in back:
                aligned.add(2 + (int(b.offs[f]) + wlo) % 2)
            seen_b.update(x for x in back if x is not None)
            seen_f.update(x for x in fwd if x is not None)
            none += back.count(None) + fwd.count(None)
        M = NL_REACH
        assert seen_b >= {1, 15, 16, 17, 1023, 1024, M - 1, M}, sorted(seen_b)
        assert seen_f >= {1023, 1024, M - 1, M} and any(x > M for x in seen_f | seen_b), sorted(seen_f)
        assert none >= 20 and aligned >= {True, 3}, aligned
