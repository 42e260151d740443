"""A plain model of the findings kernels (trivy_amd/csrc/materialize.hip: mat_locate_kernel, mat_write_kernel)
behind tsg_debug_materialize: everything the two kernels write, from the reference's own text.

The censored content is built by replacing every span with '*', oracle.secret_scanner.find_location (the
restatement of scanner.go:495-558) runs per location on it -- no windows, no blocks, no anchors -- and the
result is laid out as the kernels do: per location, in order, the match text, then the lines that are not
the cause line (the cause line shares the match text).  FindingOut fields are file-relative, pref is global
to the call.
"""
from collections import namedtuple

import numpy as np

from oracle import secret_scanner as osc

MATFILE = np.dtype([("file", "<u4"), ("m0", "<u4"), ("nm", "<u4"), ("s0", "<u4"), ("ns", "<u4"), ("pad", "<u4")])
MATMATCH = np.dtype([("rule", "<u4"), ("fidx", "<u4"), ("s", "<i8"), ("e", "<i8"), ("a_wlo", "<i8"), ("a_nl", "<i8")])
MATSPAN = np.dtype([("s", "<i8"), ("e", "<i8"), ("nl_before", "<i8")])
FINDING = np.dtype({"names": ["rule", "start_line", "end_line", "match_off", "match_len", "line_lo", "line_hi"],
                    "formats": ["<u4", "<i8", "<i8", "<u4", "<u4", "<u4", "<u4"],
                    "offsets": [0, 8, 16, 24, 28, 32, 36], "itemsize": 40})
LINE = np.dtype({"names": ["number", "off", "len", "is_cause", "first_cause", "last_cause"],
                 "formats": ["<i8", "<u4", "<u4", "u1", "u1", "u1"], "offsets": [0, 8, 12, 16, 17, 18], "itemsize": 24})
assert (MATFILE.itemsize, MATMATCH.itemsize, MATSPAN.itemsize) == (24, 40, 24)
SENTINEL = (1 << 63) - 1
LINE_CUT = 100


def text_bound(s, e):
    """The scanner's bound of one location's text bytes (materialize.h MatTextBound)."""
    return max(100, e - s + 50) + 400


def merged_spans(content: bytes, locs):
    """The censor spans of raw locations [(s, e)] as the scanner hands them over: sorted, merged where they
    overlap or touch, empty ones left out, each with the '\\n' inside the spans before it, the sentinel last."""
    out, nl = [], 0
    for s, e in sorted((s, e) for s, e in locs if e > s):
        if out and s <= out[-1][1]:
            if e > out[-1][1]:
                out[-1][1] = e
            continue
        out.append([s, e, 0])
    for sp in out:
        sp[2] = nl
        nl += content.count(b"\n", sp[0], sp[1])
    return [tuple(sp) for sp in out] + [(SENTINEL, SENTINEL, nl)]


def censor(content: bytes, spans) -> bytes:
    c = bytearray(content)
    for s, e, _ in spans:
        if s != SENTINEL:
            c[s:e] = b"*" * (e - s)
    return bytes(c)


def choose_anchor(content: bytes, s: int, positions):
    """(a_wlo, a_nl) for a location starting at s: the greatest of `positions` at or below s (0 when there is
    none) and the raw '\\n' count before it."""
    at = max([p for p in positions if p <= s], default=0)
    return at, content.count(b"\n", 0, at)


FileOut = namedtuple("FileOut", "findings lines text counts")  # file-relative; counts: (lines, text) per location


def file_model(content: bytes, locs, spans=None) -> FileOut:
    """One file's records: locs = [(rule, s, e)] in order; spans default to merged_spans of the locations."""
    spans = merged_spans(content, [(s, e) for _, s, e in locs]) if spans is None else spans
    cen = censor(content, spans)
    findings, lines, text, counts, memo = [], [], bytearray(), [], {}
    for rule, s, e in locs:
        if (s, e) not in memo:
            memo[(s, e)] = osc.find_location(s, e, cen)
        start_line, end_line, code, match = memo[(s, e)]
        t0, l0 = len(text), len(lines)
        text += match
        causes = [ln for ln in code["Lines"] if ln["IsCause"]]
        assert len(causes) == 1 and end_line == start_line, "a location is censored whole: one cause line"
        assert osc._b(causes[0]["Content"]) == match, "the cause line shares the match text"
        for ln in code["Lines"]:
            body = osc._b(ln["Content"])
            if ln["IsCause"]:
                off, n = t0, len(match)
            else:
                off, n = len(text), len(body)
                text += body
            lines.append((ln["Number"], off, n, ln["IsCause"], ln["FirstCause"], ln["LastCause"]))
        findings.append((rule, start_line, end_line, t0, len(match), l0, len(lines)))
        counts.append((len(lines) - l0, len(text) - t0))
    return FileOut(np.array(findings, dtype=FINDING).reshape(-1), np.array(lines, dtype=LINE).reshape(-1), bytes(text),
                   counts)


Call = namedtuple("Call", "findings pref lines text n_lines n_text")


def call_model(file_outs) -> Call:
    """The outputs of one call whose MatFile records have the given FileOut each, in MatFile order."""
    pref, t, l = [], 0, 0
    for fo in file_outs:
        for nl, nt in fo.counts:
            pref.append(t << 32 | l)
            t += nt
            l += nl
    pref.append(t << 32 | l)
    cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dtype=dt)
    return Call(cat([fo.findings for fo in file_outs], FINDING), np.array(pref, dtype=np.uint64),
                cat([fo.lines for fo in file_outs], LINE), b"".join(fo.text for fo in file_outs), l, t)


def records(file_ids, contents, locs_per_file, anchors_per_file=None, spans_per_file=None):
    """The upload records of a call: MatFile i is arena file file_ids[i] with content contents[i] and locations
    locs_per_file[i] = [(rule, s, e)].  anchors_per_file[i]: positions choose_anchor picks from (default: 0
    only).  -> (MATFILE, MATMATCH, MATSPAN arrays)."""
    F, M, S = [], [], []
    for i, (fid, content, locs) in enumerate(zip(file_ids, contents, locs_per_file)):
        spans = (merged_spans(content, [(s, e) for _, s, e in locs]) if spans_per_file is None
                 else spans_per_file[i])
        F.append((fid, len(M), len(locs), len(S), len(spans), 0))
        pos = anchors_per_file[i] if anchors_per_file is not None else (0,)
        for rule, s, e in locs:
            M.append((rule, i, s, e) + choose_anchor(content, s, pos))
        S += spans
    return (np.array(F, dtype=MATFILE).reshape(-1), np.array(M, dtype=MATMATCH).reshape(-1),
            np.array(S, dtype=MATSPAN).reshape(-1))


def findings_of(rules, fo: FileOut):
    """The reference's Finding dicts (unsorted) rebuilt from one file's records; rules[i]: the oracle's Rule."""
    out = []
    for f in fo.findings:
        rule = rules[int(f["rule"])]
        lines = []
        for ln in fo.lines[int(f["line_lo"]):int(f["line_hi"])]:
            s = osc._s(fo.text[int(ln["off"]):int(ln["off"]) + int(ln["len"])])
            lines.append({"Number": int(ln["number"]), "Content": s, "IsCause": bool(ln["is_cause"]), "Annotation": "",
                          "Truncated": False, "Highlighted": s, "FirstCause": bool(ln["first_cause"]),
                          "LastCause": bool(ln["last_cause"])})
        out.append({"RuleID": rule.id, "Category": rule.category,
                    "Severity": "UNKNOWN" if rule.severity == "" else rule.severity, "Title": rule.title,
                    "StartLine": int(f["start_line"]), "EndLine": int(f["end_line"]), "Code": {"Lines": lines},
                    "Match": osc._s(fo.text[int(f["match_off"]):int(f["match_off"]) + int(f["match_len"])])})
    return out


def diff(got: Call, want: Call, describe=lambda m: "location %d" % m):
    """The first difference between two calls' outputs, naming the location and the field; None when equal."""
    if (got.n_lines, got.n_text) != (want.n_lines, want.n_text):
        # (fall through to the per-location fields: they say where the totals went apart)
        head = "totals (lines, text) got %s want %s; " % ((got.n_lines, got.n_text), (want.n_lines, want.n_text))
    else:
        head = ""
    nm = len(want.findings)
    if len(got.findings) != nm or len(got.pref) != nm + 1:
        return head + "record counts differ"
    bad = np.nonzero(got.pref != want.pref)[0]
    if len(bad):  # pref[m + 1] - pref[m] is location m's (text bytes, lines): the first wrong entry blames m
        m = int(bad[0])
        c = max(m - 1, 0)
        fields = ["FindingOut.%s got %d want %d" % (n, int(got.findings[n][c]), int(want.findings[n][c]))
                  for n in FINDING.names if got.findings[n][c] != want.findings[n][c]]
        l0, l1 = int(want.pref[c]) & 0xFFFFFFFF, int(want.pref[c + 1]) & 0xFFFFFFFF
        if l1 <= len(got.lines):
            fields += ["line %d LineOut.len got %d want %d" % (i - l0, int(got.lines["len"][i]), int(want.lines["len"][i]))
                       for i in range(l0, l1) if got.lines["len"][i] != want.lines["len"][i]]
        return head + "%s: pref[%d] (the sizes up to and with this location) got (text %d, line %d) want (text %d, line %d)%s" % (
            describe(c), m, int(got.pref[m]) >> 32, int(got.pref[m]) & 0xFFFFFFFF,
            int(want.pref[m]) >> 32, int(want.pref[m]) & 0xFFFFFFFF, "; " + "; ".join(fields) if fields else "")
    for name in FINDING.names:
        bad = np.nonzero(got.findings[name] != want.findings[name])[0]
        if len(bad):
            m = int(bad[0])
            return head + "%s: FindingOut.%s got %d want %d (%d locations differ)" % (
                describe(m), name, int(got.findings[name][m]), int(want.findings[name][m]), len(bad))
    line_owner = np.searchsorted(want.pref & np.uint64(0xFFFFFFFF), np.arange(want.n_lines), side="right") - 1
    for name in LINE.names:
        bad = np.nonzero(got.lines[name] != want.lines[name])[0]
        if len(bad):
            i = int(bad[0])
            m = int(line_owner[i])
            return head + "%s: line %d LineOut.%s got %d want %d" % (
                describe(m), i - (int(want.pref[m]) & 0xFFFFFFFF), name, int(got.lines[name][i]),
                int(want.lines[name][i]))
    if got.text != want.text:
        g, w = np.frombuffer(got.text, dtype=np.uint8), np.frombuffer(want.text, dtype=np.uint8)
        i = int(np.nonzero(g != w)[0][0])
        m = int(np.searchsorted(want.pref >> np.uint64(32), i, side="right") - 1)
        return head + "%s: text byte %d (%d of its text) got %r want %r" % (
            describe(m), i, i - (int(want.pref[m]) >> 32), got.text[i:i + 1], want.text[i:i + 1])
    return head or None
