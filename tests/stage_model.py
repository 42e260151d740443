"""CPU models of the candidate engine's stages (test helper, not product code).

One synchronous scan of trivy_amd/csrc/engine.hip leaves behind a chunk map
(K0), per-chunk newline counts and flagged 16-B blocks (K1), anchor hits,
keyword bits and file flags (K2, the fold kernels), candidates (verify / full
scan) and their line hints and gate flags (finalize).  tsg_debug_engine_stages
(include/tsg_debug.h) brings them back; this file restates each stage plainly,
on top of FilterModel (the compiled prefilter tables) and the oracle, and holds
the comparison functions tests/test_stage_model.py (CPU: the models and the
checkers themselves) and tests/test_gpu_stages.py (the kernels) share.  Every
check is an exact set or integer comparison and raises AssertionError.
"""
import ctypes as c
import os
from collections import Counter

import numpy as np

from oracle.gostd import bytes_to_lower, strings_to_lower
from tests.filter_model import KIND_ANCHOR, KIND_FOLD, KIND_KEYWORD, FilterModel, RuleInfo
from trivy_amd import _lib

CHUNK = 1024          # engine.h kChunk
TILE = 4096           # engine.hip kFTile
NL_NONE, NL_UNKNOWN = 0xFFFFFFFE, 0xFFFFFFFF
NL_REACH = 1 << 20    # engine.h kNlReach
GATE_OPEN, FOLD_FILE, GATE_VALID, DROP = 1, 2, 4, 8  # engine.h kCand*
# The scan counters' slots (trivy_amd/csrc/scan_layout.h kCt*; tsg_debug_stage_dump.counters).
CTR_WORDS = 16
CT_HITS, CT_CANDS, CT_SPECIAL, CT_HIT_OVF, CT_CAND_OVF = 0, 1, 2, 3, 4
CT_FS_OVF, CT_RECS, CT_REC_OVF, CT_FOLDS, CT_FOLD_OVF = 6, 7, 8, 9, 10
CT_ANCHOR_HITS, CT_OPEN_PAIRS = 11, 13
RUNE_I, RUNE_K, RUNE_S = b"\xc4\xb0", b"\xe2\x84\xaa", b"\xc5\xbf"  # U+0130, U+212A, U+017F

CAND = np.dtype([("file", "<u4"), ("rule", "<u4"), ("wlo", "<i8"), ("whi", "<i8"), ("nl_before", "<i8"),
                 ("flags", "<u4"), ("nl_back", "<u4", (3,)), ("nl_fwd", "<u4", (3,)), ("pad", "<u4")])
assert CAND.itemsize == 64  # engine.h Candidate


class Batch:
    """Files packed back to back, as the scanner packs them; `tail`: the 64 bytes behind the arena."""

    def __init__(self, contents, tail=None):
        self.contents = [bytes(x) for x in contents]
        self.arena = b"".join(self.contents)
        self.a = np.frombuffer(self.arena, dtype=np.uint8)
        self.offs = np.zeros(len(self.contents) + 1, dtype=np.int64)
        self.offs[1:] = np.cumsum([len(x) for x in self.contents])
        self.tail = bytes(tail) if tail is not None else bytes(64)
        assert len(self.tail) == 64
        self.n_files, self.n_bytes = len(self.contents), len(self.arena)


class Dump:
    """The stages of one scan: what tsg_debug_engine_stages returns, or what the models expect."""

    def __init__(self, counters, kw_words, hits, kw, flags, nl, recs, chunk_file, cands):
        self.counters = [int(x) for x in counters]
        self.kw_words = int(kw_words)
        self.hits = [tuple(int(x) for x in h) for h in hits]   # (file, literal end in the file, anchor id)
        self.flags = np.array(flags, dtype=np.uint32)
        self.kw = np.array(kw, dtype=np.uint32).reshape(-1, self.kw_words) if self.kw_words else \
            np.zeros((len(self.flags), 1), dtype=np.uint32)  # [file, word]
        self.nl = np.array(nl, dtype=np.uint16)
        self.recs = np.array(recs, dtype=np.uint32)
        self.chunk_file = np.array(chunk_file, dtype=np.uint32)
        self.cands = np.array(cands, dtype=CAND)

    def kw_bit(self, f, k):
        return bool((int(self.kw[f, k >> 5]) >> (k & 31)) & 1)


class _CStageDump(c.Structure):  # tsg_debug_stage_dump (include/tsg_debug.h)
    _fields_ = [("struct_size", c.c_uint32), ("kw_words", c.c_uint32), ("counters", c.c_uint32 * CTR_WORDS),
                ("caps", c.c_uint32 * 3), ("reserved_", c.c_uint32)] + \
               [(n, t) for name in ("hits", "kw", "flags", "nl", "chunk_file", "recs", "cands")
                for n, t in ((name, c.c_void_p), (name + "_cap", c.c_uint64), ("n_" + name, c.c_uint64))]


class Nfa:
    """A rule's relaxed NFA (rules.h: O L F B[256], W words each; word 0 least significant) as big ints."""

    def __init__(self, words, ptr):
        self.words = words
        if words == 0:
            return
        raw = np.ctypeslib.as_array((c.c_uint64 * ((3 + 256) * words)).from_address(ptr)).copy()

        def big(i):
            return sum(int(raw[i * words + w]) << (64 * w) for w in range(words))

        self.O, self.L, self.F = big(0), big(1), big(2)
        self.B = [big(3 + b) for b in range(256)]
        self.mask = (1 << (64 * words)) - 1

    def accepts(self, content, wlo, whi):
        """engine.hip nfa_run_abs: start at wlo, inject while pos <= whi, the optional-state closure
        by the add-carry trick, stay on UTF-8 continuation bytes, accept on D & F, reject when dead
        past whi or at the file end."""
        if self.words == 0:
            return True
        D, O, L, F, B, mask = 0, self.O, self.L, self.F, self.B, self.mask
        for pos in range(wlo, len(content)):
            b = content[pos]
            T = ((D << 1) | (1 if pos <= whi else 0) | (D & L)) & mask
            T |= (((T & O) + O) & mask) ^ O
            D = (T & B[b]) | (D if (b & 0xC0) == 0x80 else 0)
            if D & F:
                return True
            if D == 0 and pos >= whi:
                return False
        return False


class StageModel:
    def __init__(self, rules, calibration=None):
        self.rules = list(rules)
        self.fm = FilterModel(self.rules, calibration=calibration)
        L, h = _lib.lib(), self.fm.h
        L.tsg_debug_anchor.argtypes = [c.c_void_p, c.c_uint32] + [c.c_void_p] * 4
        self.anchors = []  # (rule, lit_len, off_lo, off_hi)
        while True:
            r, ln, lo, hi = c.c_uint32(), c.c_uint32(), c.c_int32(), c.c_int32()
            if L.tsg_debug_anchor(h, len(self.anchors), c.byref(r), c.byref(ln), c.byref(lo), c.byref(hi)) != 0:
                break
            self.anchors.append((r.value, ln.value, lo.value, hi.value))
        self.reqs = self.fm.anchor_reqs()
        L.tsg_debug_rule.argtypes = [c.c_void_p, c.c_uint32, c.c_void_p]
        L.tsg_debug_rule_gate_implied.argtypes = [c.c_void_p, c.c_uint32]
        self.info = []  # per rule: dict(nfa, gate, anchored, has_regex, kw, implied)
        for i in range(len(self.rules)):
            ri = RuleInfo()
            assert L.tsg_debug_rule(h, i, c.byref(ri)) == 0
            kw = [int(x) for x in np.ctypeslib.as_array((c.c_uint32 * ri.n_kw).from_address(ri.kw_ids))] \
                if ri.n_kw else []
            self.info.append({"nfa": Nfa(ri.nfa_words, ri.nfa), "gate": ri.gate, "anchored": ri.anchored,
                              "has_regex": ri.has_regex, "kw": kw,
                              "implied": L.tsg_debug_rule_gate_implied(h, i) == 1})
        L.tsg_debug_keyword.restype = c.c_char_p
        L.tsg_debug_keyword.argtypes = [c.c_void_p, c.c_uint32]
        self.keywords = []
        while True:
            k = L.tsg_debug_keyword(h, len(self.keywords))
            if k is None:
                break
            self.keywords.append(k)
        self.kw_words = (len(self.keywords) + 31) // 32
        kw_items = [it for it in self.fm.items if it["kind"] == KIND_KEYWORD]
        self.kw_with_item = sorted({int(self.fm.item_ids[it["ids_off"]]) for it in kw_items})
        # engine.hip GpuEngine(): kwfold_kernel covers keyword items of <= 48 positions (TSG_KWFOLD=0: off)
        self.kw_fold = all(it["n"] <= 48 for it in kw_items) and os.environ.get("TSG_KWFOLD", "1") != "0"

    # ---- K0 / K1 ----------------------------------------------------------------------------------
    @staticmethod
    def chunk_map(b):
        """chunk_file[c]: the last file f with off[f] <= 1024 c, capped at n_files - 1."""
        n = (b.n_bytes + CHUNK - 1) // CHUNK
        out = np.zeros(n, dtype=np.uint32)
        for ck in range(n):
            f = int(np.searchsorted(b.offs[:b.n_files], ck * CHUNK, side="right")) - 1
            out[ck] = min(max(f, 0), b.n_files - 1)
        return out

    @staticmethod
    def nl_counts(b):
        n = (b.n_bytes + CHUNK - 1) // CHUNK
        return np.array([b.arena[CHUNK * k:CHUNK * (k + 1)].count(b"\n") for k in range(n)], dtype=np.uint16)

    def flagged_blocks(self, b):
        """{t >> 4} over every window end t at which a non-newline bucket fires.  K1 streams whole
        4-KiB tiles and zeroes the last tile's bytes past n_bytes (engine.hip filter_kernel, kTail),
        so the model's stream is the arena zero-padded to the tile end: a bucket whose sets admit
        0x00 may fire there, and does in the kernel."""
        pad = (-b.n_bytes) % TILE
        fr = self.fm.fires(np.concatenate([b.a, np.zeros(pad, dtype=np.uint8)]))
        t = np.nonzero(fr[:self.fm.n_buckets - 1].any(axis=0))[0]
        return np.unique(t >> 4).astype(np.uint32)

    # ---- K2 ---------------------------------------------------------------------------------------
    def confirm(self, b):
        """FilterModel.run, keeping the multiplicity of the anchor hits: a list of (file, end, anchor)."""
        fm, a, offs = self.fm, b.a, b.offs
        hits = []
        fr = fm.fires(a)
        for j in range(fm.n_buckets):
            for t in np.nonzero(fr[j])[0]:
                for x in fm.bucket_items[fm.bucket_off[j]:fm.bucket_off[j + 1]]:
                    it = fm.items[int(x)]
                    if it["kind"] != KIND_ANCHOR:
                        continue
                    start = int(t) + 1 - it["back"]
                    if not fm.item_match(a, it, start):
                        continue
                    f = int(np.searchsorted(offs, start, side="right")) - 1
                    fs, fe = int(offs[f]), int(offs[f + 1])
                    if start < fs or start + it["n"] > fe:
                        continue
                    for aid in fm.item_ids[it["ids_off"]:it["ids_off"] + it["n_ids"]]:
                        hits.append((f, start - fs + it["lit_end"], int(aid)))
        return hits

    def file_flags(self, b):
        """bit 0: any of U+0130 / U+212A / U+017F occurs; bit 1: U+017F; bit 2: U+0130 / U+212A."""
        out = np.zeros(b.n_files, dtype=np.uint32)
        for f, x in enumerate(b.contents):
            s, ik = RUNE_S in x, RUNE_I in x or RUNE_K in x
            out[f] = (1 if s or ik else 0) | (2 if s else 0) | (4 if ik else 0)
        return out

    def keyword_bits(self, b, flags, kw_fold):
        """{(file, keyword id)} for keywords with an item, and the files whose bits are exact:
        ASCII case-insensitive containment; in a file with U+0130 / U+212A, after kwfold_kernel,
        containment in Go's bytes.ToLower of the content."""
        bits, exact = set(), []
        for f, x in enumerate(b.contents):
            if int(flags[f]) & 4:
                if not kw_fold:
                    continue
                low = _lib.go_bytes_to_lower(x)
            else:
                low = x.lower()
            exact.append(f)
            bits.update((f, k) for k in self.kw_with_item if self.keywords[k] in low)
        return bits, exact

    def gate_skipped(self, r, f, flags, kw_fold, bit):
        """verify_hits_kernel / fs_pairs_kernel / finalize_kernel: the rule's ASCII keyword gate is
        closed in a file whose bits are exact (bit(f, k) reads them)."""
        ri = self.info[r]
        if ri["gate"] != 1 or ri["implied"]:
            return False
        if (int(flags[f]) & 4) and not kw_fold:
            return False
        return not any(bit(f, k) for k in ri["kw"])

    def candidates(self, b, hits, flags, kw_fold, bits):
        """verify_hits_kernel over `hits`, files without fold runes: Counter of (file, rule, wlo, whi)."""
        out = Counter()
        memo = {}
        for f, end, aid in hits:
            if int(flags[f]) & 1:
                continue
            r, lit_len, off_lo, off_hi = self.anchors[aid]
            if self.gate_skipped(r, f, flags, kw_fold, lambda ff, k: (ff, k) in bits):
                continue
            lit = end - lit_len
            whi = lit - off_lo
            if whi < 0:
                continue
            wlo = max(0, lit - off_hi)
            key = (f, r, wlo, whi)
            if key not in memo:
                memo[key] = self.info[r]["nfa"].accepts(b.contents[f], wlo, whi)
            if memo[key]:
                out[key] += 1
        return out

    def expect(self, b, kw_fold=None):
        """Everything the models say about batch b."""
        kw_fold = self.kw_fold if kw_fold is None else kw_fold
        e = type("Expect", (), {})()
        e.kw_fold = kw_fold
        e.chunk_file, e.nl, e.blocks = self.chunk_map(b), self.nl_counts(b), self.flagged_blocks(b)
        e.flags = self.file_flags(b)
        e.kw_bits, e.kw_exact = self.keyword_bits(b, e.flags, kw_fold)
        e.all_hits = self.confirm(b)
        # The confirm kernel tests an anchor's follow requirements only while the literal ends
        # before the arena's end (engine.hip check_item: `lut.n[0] && e < P.n_bytes`): a hit whose
        # literal ends with the arena's last byte is kept untested.  `required` is what no scan may
        # miss, `allowed` adds those hits; the kernel must lie between the two.
        req, alw = [], []
        for h in e.all_hits:
            f, end, aid = h
            ok = self.fm.follow_possible(self.reqs[aid], b.contents[f], end)
            if ok:
                req.append(h)
            if ok or int(b.offs[f]) + end == b.n_bytes:
                alw.append(h)
        e.hits_required, e.hits_allowed = req, alw
        e.cands_required = self.candidates(b, req, e.flags, kw_fold, e.kw_bits)
        e.cands_allowed = self.candidates(b, alw, e.flags, kw_fold, e.kw_bits)
        return e

    # ---- finalize ---------------------------------------------------------------------------------
    @staticmethod
    def hints(content, wlo):
        """(nl_before, [(distance or None) x 3] backwards, the same forwards) of a window start."""
        back, p = [], wlo
        while len(back) < 3:
            p = content.rfind(b"\n", 0, p)
            if p < 0:
                break
            back.append(wlo - p)
        fwd, p = [], wlo
        while len(fwd) < 3:
            p = content.find(b"\n", p)
            if p < 0:
                break
            fwd.append(p - wlo)
            p += 1
        return content.count(b"\n", 0, wlo), back + [None] * (3 - len(back)), fwd + [None] * (3 - len(fwd))

    def cand_flags(self, r, f, flags, kw_fold, bit):
        """finalize_kernel / gate_flags: the flags of a candidate of rule r in file f."""
        ri = self.info[r]
        inexact = bool(int(flags[f]) & 4) and not kw_fold
        fl = GATE_VALID | (FOLD_FILE if inexact else 0)
        gated = ri["gate"] == 1 and not ri["implied"]
        if gated and any(bit(f, k) for k in ri["kw"]):
            fl |= GATE_OPEN
        if gated and not inexact and not fl & GATE_OPEN:
            fl |= DROP
        return fl

    def synth_dump(self, b, e):
        """A dump made from the models alone (what a correct engine would return)."""
        kw = np.zeros((b.n_files, max(1, self.kw_words)), dtype=np.uint32)
        for f, k in e.kw_bits:
            kw[f, k >> 5] |= np.uint32(1 << (k & 31))
        cands = []
        for (f, r, wlo, whi), n in sorted(e.cands_required.items()):
            nlb, back, fwd = self.hints(b.contents[f], wlo)
            fl = self.cand_flags(r, f, e.flags, e.kw_fold, lambda ff, k: (ff, k) in e.kw_bits)
            enc = lambda v: [NL_NONE if x is None else x for x in v]  # noqa: E731
            cands += [(f, r, wlo, whi, nlb, fl, enc(back), enc(fwd), 0)] * n
        counters = [0] * CTR_WORDS
        counters[CT_HITS], counters[CT_CANDS], counters[CT_RECS] = len(e.hits_required), len(cands), len(e.blocks)
        counters[CT_SPECIAL] = int(np.count_nonzero(e.flags))
        return Dump(counters, self.kw_words, e.hits_required, kw, e.flags, e.nl, e.blocks, e.chunk_file, cands)

    # ---- the oracle -------------------------------------------------------------------------------
    def match_keywords(self, r, content, low=None):
        """scanner.go:174-186 (oracle/secret_scanner.py Rule.match_keywords); low: the lowered content."""
        kws = self.rules[r].Keywords or []
        if not kws:
            return True
        low = bytes_to_lower(content) if low is None else low
        return any(strings_to_lower(k.encode("utf-8", "surrogateescape")) in low for k in kws)

    def true_matches(self, b):
        """{(file, rule): [non-empty match starts]} where the oracle's MatchKeywords holds."""
        out = {}
        for f, x in enumerate(b.contents):
            if not x:
                continue
            low = bytes_to_lower(x)
            for r, rule in enumerate(self.rules):
                if not rule.Regex or not self.match_keywords(r, x, low):
                    continue
                starts = [m[0] for m in _lib.regex_find_all(rule.Regex, x, submatch=False) if m[1] > m[0]]
                if starts:
                    out[(f, r)] = starts
        return out


def run_engine(model, b, device=0):
    """tsg_debug_engine_stages on batch b -> Dump."""
    L = _lib.lib()
    d = _CStageDump()
    d.struct_size = c.sizeof(_CStageDump)
    off = np.ascontiguousarray(b.offs, dtype=np.uint64)
    arena = np.frombuffer(b.arena + b"\0", dtype=np.uint8)  # (never empty)
    tail = (c.c_uint8 * 64).from_buffer_copy(b.tail)
    L.tsg_debug_engine_stages.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint32,
                                          c.c_void_p, c.c_void_p]
    keep = {}
    for attempt in range(2):  # sizes first, then the records
        rc = L.tsg_debug_engine_stages(model.fm.h, device, arena.ctypes.data, b.n_bytes, off.ctypes.data, b.n_files,
                                       tail, c.byref(d))
        if rc != 0:
            raise RuntimeError(_lib.last_error())
        if attempt == 0:
            for name, dt in (("hits", np.dtype((np.uint64, 3))), ("kw", np.uint32), ("flags", np.uint32),
                             ("nl", np.uint16), ("chunk_file", np.uint32), ("recs", np.uint32), ("cands", CAND)):
                n = int(getattr(d, "n_" + name))
                keep[name] = np.zeros(n + 1, dtype=dt)
                setattr(d, name, keep[name].ctypes.data)
                setattr(d, name + "_cap", n)
    for name, buf in keep.items():
        assert int(getattr(d, "n_" + name)) == len(buf) - 1, name  # (the scan is deterministic in its counts)
        keep[name] = buf[:-1]
    return Dump(list(d.counters), d.kw_words, keep["hits"], keep["kw"], keep["flags"], keep["nl"], keep["recs"],
                keep["chunk_file"], keep["cands"])


# ---- the comparisons (shared by the CPU and the GPU tests) -------------------------------------------

def _fail(what, *detail):
    raise AssertionError(what + ": " + " ".join(repr(x)[:400] for x in detail))


def check_overflow(d):
    """No list overflowed: a comparison must not pass on truncated lists."""
    if any(d.counters[i] for i in (CT_HIT_OVF, CT_CAND_OVF, CT_REC_OVF, CT_FOLD_OVF)):
        _fail("overflow counters set", d.counters)
    if d.counters[CT_HITS] != len(d.hits) or d.counters[CT_CANDS] != len(d.cands) or \
            d.counters[CT_RECS] != len(d.recs):
        _fail("list lengths differ from the counters", d.counters, len(d.hits), len(d.cands), len(d.recs))


def check_chunks(d, e):
    """Invariant 1: the chunk map and the per-chunk newline counts."""
    if not np.array_equal(d.chunk_file, e.chunk_file):
        _fail("chunk map", np.nonzero(d.chunk_file != e.chunk_file)[0][:8] if len(d.chunk_file) == len(e.chunk_file)
              else (len(d.chunk_file), len(e.chunk_file)))
    if not np.array_equal(d.nl, e.nl):
        _fail("newline counts", np.nonzero(d.nl != e.nl)[0][:8] if len(d.nl) == len(e.nl) else (len(d.nl), len(e.nl)))


def check_blocks(d, e):
    """Invariant 2: the flagged blocks, each once.  K1 is exact (StageModel.flagged_blocks)."""
    got = np.sort(d.recs)
    if not np.array_equal(got, e.blocks):
        _fail("flagged blocks", "missing", sorted(set(e.blocks.tolist()) - set(got.tolist()))[:8], "excess",
              sorted(set(got.tolist()) - set(e.blocks.tolist()))[:8], "records", len(got), "model", len(e.blocks))


def check_hits(d, e, b):
    """Invariant 3, files without fold runes: required <= hits <= allowed, as multisets."""
    plain = lambda hs: Counter(h for h in hs if not int(e.flags[h[0]]) & 1)  # noqa: E731
    got, req, alw = plain(d.hits), plain(e.hits_required), plain(e.hits_allowed)
    for h in d.hits:
        if not (0 <= h[0] < b.n_files and 0 < h[1] <= len(b.contents[h[0]])):
            _fail("hit outside its file", h)
    if req - got:
        _fail("missed hits", sorted((req - got).elements())[:8])
    if got - alw:
        _fail("hits the tables do not justify", sorted((got - alw).elements())[:8])


def check_keywords(d, e, model):
    """Invariant 4: keyword bits, in the files where they are exact; none in an empty file."""
    for f in e.kw_exact:
        for k in range(len(model.keywords)):
            want = (f, k) in e.kw_bits
            if d.kw_bit(f, k) != want:
                _fail("keyword bit", "file", f, "keyword", model.keywords[k], "want", want)


def check_flags(d, e, b):
    """Invariant 4: the per-file fold flags and their count."""
    if not np.array_equal(d.flags, e.flags):
        _fail("file flags", [(f, int(d.flags[f]), int(e.flags[f])) for f in np.nonzero(d.flags != e.flags)[0][:8]])
    if d.counters[CT_SPECIAL] != int(np.count_nonzero(e.flags)):
        _fail("special-file count", d.counters[CT_SPECIAL], int(np.count_nonzero(e.flags)))
    for f, x in enumerate(b.contents):
        if not x and (int(d.flags[f]) or d.kw[f].any()):
            _fail("an empty file has a flag or a keyword bit", f)


def check_candidates(d, e, model):
    """Invariant 5: candidates of anchored rules in files without fold runes, as a multiset."""
    got = Counter((int(x["file"]), int(x["rule"]), int(x["wlo"]), int(x["whi"])) for x in d.cands
                  if model.info[int(x["rule"])]["anchored"] and not int(e.flags[int(x["file"])]) & 1)
    if e.cands_required - got:
        _fail("missed candidates", sorted((e.cands_required - got).elements())[:8])
    if got - e.cands_allowed:
        _fail("candidates the hits do not justify", sorted((got - e.cands_allowed).elements())[:8])


def check_fields(d, e, model, b):
    """Invariant 5: nl_before, the newline hints and the gate flags of every candidate."""
    bit = d.kw_bit
    for i, x in enumerate(d.cands):
        f, r, wlo, whi = int(x["file"]), int(x["rule"]), int(x["wlo"]), int(x["whi"])
        if not (f < b.n_files and r < len(model.rules) and 0 <= wlo <= whi and wlo <= len(b.contents[f])):
            _fail("candidate out of range", i, f, r, wlo, whi)
        content = b.contents[f]
        nlb, back, fwd = model.hints(content, wlo)
        if int(x["nl_before"]) != nlb:
            _fail("nl_before", i, (f, r, wlo), int(x["nl_before"]), nlb)
        fl = int(x["flags"])
        want = model.cand_flags(r, f, d.flags, e.kw_fold, bit)
        if fl != want:
            _fail("candidate flags", i, (f, r, wlo), fl, want)
        if fl & DROP and model.match_keywords(r, content):
            _fail("kCandDrop where MatchKeywords holds", i, (f, r, wlo))
        for name, true, edge in (("nl_back", back, wlo), ("nl_fwd", fwd, len(content) - wlo)):
            for k in range(3):
                got = int(x[name][k])
                if fl & DROP:  # the hints are left as put_candidate wrote them
                    ok = got == NL_UNKNOWN
                elif true[k] is None:  # no such newline: known once the search reached the file's edge
                    ok = got == NL_NONE or (edge > NL_REACH and got == NL_UNKNOWN)
                else:
                    ok = got == true[k] or (true[k] > NL_REACH and got == NL_UNKNOWN)
                if not ok:
                    _fail(name, i, (f, r, wlo), "rank", k, "got", got, "true", true[k])


def check_coverage(d, model, b, matches=None):
    """Invariant 6: every non-empty true match start of every rule, in every file, lies in the
    window of a candidate of that (file, rule) that is not dropped (where MatchKeywords holds)."""
    wins = {}
    for x in d.cands:
        if not int(x["flags"]) & DROP:
            wins.setdefault((int(x["file"]), int(x["rule"])), []).append((int(x["wlo"]), int(x["whi"])))
    matches = model.true_matches(b) if matches is None else matches
    n = 0
    for key, starts in matches.items():
        ws = wins.get(key, [])
        for s in starts:
            if not any(lo <= s <= hi for lo, hi in ws):
                _fail("true match without a candidate", "file", key[0], "rule", model.rules[key[1]].ID, "start", s)
            n += 1
    return n


def check_all(d, e, model, b, matches=None):
    """Invariants 1-6 on one dump; returns the number of true matches covered."""
    check_overflow(d)
    check_chunks(d, e)
    check_blocks(d, e)
    check_hits(d, e, b)
    check_keywords(d, e, model)
    check_flags(d, e, b)
    check_candidates(d, e, model)
    check_fields(d, e, model, b)
    return check_coverage(d, model, b, matches)
