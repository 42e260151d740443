"""A pure-Python model of LayerTar.Walk with its skipFiles / skipDirs options (pkg/fanal/walker/tar.go:35-89,
underSkippedDir :105-116) and the layers the skip tests share.

Per entry of the archive, in order, on filePath = path.Clean(name) without leading '/':

1. opaque markers and whiteouts are counted, whatever the options say;
2. TypeDir (typeflag '5', or '\\0' with a name that ends in '/'): when SkipPath(filePath, skipDirs) holds the
   path is appended to skippedDirs and the entry dropped;
3. TypeReg: dropped when SkipPath(filePath, skipFiles) holds;
4. every other type is dropped;
5. a survivor is dropped when under_skipped_dir(filePath, skippedDirs) holds.

Headers are read with CPython's tarfile (independent of the native walks); path.Clean, SkipPath and the
analyzer are oracle/analyzer.py's.  go_rel restates Go's filepath.Rel on Unix.
"""
import io
import tarfile

from oracle import analyzer as oan
from tests import tar_index_model as tm

TOKEN = b"ghp_" + b"a1B2" * 9  # a builtin rule (github-pat) finds it


def go_rel(base: str, targ: str):
    """filepath.Rel(base, targ) for two path.Clean-ed inputs ("" cleans to "."); None when it fails."""
    base = base or "."
    targ = targ or "."
    if base == targ:
        return "."
    if base == ".":
        base = ""
    if base.startswith("/") != targ.startswith("/"):
        return None
    bl, tl = len(base), len(targ)
    b0 = bi = t0 = ti = 0
    while bi < bl and ti < tl:
        while bi < bl and base[bi] != "/":
            bi += 1
        while ti < tl and targ[ti] != "/":
            ti += 1
        if targ[t0:ti] != base[b0:bi]:
            break
        if bi < bl:
            bi += 1
        if ti < tl:
            ti += 1
        b0, t0 = bi, ti
    if base[b0:bi] == "..":
        return None
    if b0 != bl:
        out = ".." + "/.." * base[b0:bl].count("/")
        if t0 != tl:
            out += "/" + targ[t0:]
        return out
    return targ[t0:]


def under_skipped_dir(file_path: str, skipped_dirs) -> bool:  # tar.go:105-116
    for d in skipped_dirs:
        rel = go_rel(d, file_path)
        if rel is None:
            return False
        if not rel.startswith("../"):
            return True
    return False


def walk(layer: bytes, skip_dirs=(), skip_files=()):
    """The walk's outcome as a dict: kept [(filePath, size, content)] -- the regular files analyzeFn sees --
    dropped [filePath] of the regular files the options dropped, whiteouts, opaque_dirs, regular (every
    regular entry that is no marker), skipped_dirs (the recorded list), skipped_files, under_skipped_dir
    (regular files only)."""
    skip_dirs, skip_files = list(skip_dirs), list(skip_files)
    out = dict(kept=[], dropped=[], whiteouts=0, opaque_dirs=0, regular=0, skipped_dirs=[], skipped_files=0,
               under_skipped_dir=0)
    with tarfile.open(fileobj=io.BytesIO(layer), mode="r:") as tf:
        for m in tf:
            fp = oan.go_path_clean(m.name).lstrip("/")
            fname = fp.rsplit("/", 1)[-1]
            if fname == ".wh..wh..opq":
                out["opaque_dirs"] += 1
                continue
            if fname.startswith(".wh."):
                out["whiteouts"] += 1
                continue
            if m.type == tarfile.DIRTYPE:  # (tarfile, like Go, makes a '\0' entry with a trailing slash one)
                if oan.skip_path(fp, skip_dirs):
                    out["skipped_dirs"].append(fp)
                    continue
            elif m.type in (tarfile.REGTYPE, tarfile.AREGTYPE):
                out["regular"] += 1
                if oan.skip_path(fp, skip_files):
                    out["skipped_files"] += 1
                    out["dropped"].append(fp)
                    continue
            else:
                continue
            if under_skipped_dir(fp, out["skipped_dirs"]):
                if m.type != tarfile.DIRTYPE:
                    out["under_skipped_dir"] += 1
                    out["dropped"].append(fp)
                continue
            if m.type != tarfile.DIRTYPE:
                out["kept"].append((fp, m.size, tf.extractfile(m).read()))
    return out


def sort_secrets(secrets):
    """AnalysisResult.Sort (analyzer.go:225-234) over secret dicts."""
    secrets.sort(key=lambda s: s["FilePath"].encode("utf-8", "surrogateescape"))
    for s in secrets:
        s["Findings"].sort(key=lambda f: (f["RuleID"].encode(), f["StartLine"]))
    return secrets


def analyze(analyzer: oan.SecretAnalyzer, layer: bytes, skip_dirs=(), skip_files=()):
    """oracle.analyzer.analyze_layer with the options: the secret dicts of the kept files with findings,
    in walk order."""
    out = []
    for fp, size, content in walk(layer, skip_dirs, skip_files)["kept"]:
        if not analyzer.required(fp, size):
            continue
        r = analyzer.analyze(fp, "", content)
        if r is not None:
            out.append(r["Secrets"][0])
    return out


# ---- the layers ----------------------------------------------------------------
def content(name: str, size: int = 0) -> bytes:
    """A regular file's bytes: ten bytes or more, with a planted secret."""
    b = b"# " + name.encode("utf-8", "surrogateescape") + b"\ntoken = " + TOKEN + b"\n"
    while len(b) < size:
        b += b"# filler line %d of a larger file\n" % len(b)
    return b


def build(entries, fmt=tarfile.GNU_FORMAT) -> bytes:
    """One layer from (kind, name[, size]) tuples: "d" a directory (typeflag '5'), "f" a regular file with
    content(name, size), "m" an empty marker entry (a whiteout, an opaque marker), "l" a symlink, "0d" / "0f"
    hand-built ustar headers with typeflag '\\0' (the directory's name ends in '/')."""
    buf = io.BytesIO()
    tf = tarfile.open(fileobj=buf, mode="w", format=fmt)
    for e in entries:
        kind, name = e[0], e[1]
        if kind == "d":
            ti = tarfile.TarInfo(name + "/")
            ti.type = tarfile.DIRTYPE
            tf.addfile(ti)
        elif kind == "f":
            data = content(name, e[2] if len(e) > 2 else 0)
            ti = tarfile.TarInfo(name)
            ti.size = len(data)
            ti.mode = 0o644
            tf.addfile(ti, io.BytesIO(data))
        elif kind == "m":
            tf.addfile(tarfile.TarInfo(name))
        elif kind == "l":
            ti = tarfile.TarInfo(name)
            ti.type = tarfile.SYMTYPE
            ti.linkname = "target"
            tf.addfile(ti)
        elif kind == "0d":
            assert name.endswith("/") and len(name) <= 100
            tf.fileobj.write(bytes(tm.header(name.encode(), 0, b"\0")))
            tf.offset += 512
        elif kind == "0f":
            data = content(name)
            tf.fileobj.write(bytes(tm.header(name.encode(), len(data), b"\0")) + tm.pad512(data))
            tf.offset += 512 + len(tm.pad512(data))
        else:
            raise ValueError(kind)
    tf.close()
    return buf.getvalue()


LONG = "p" * 120
LONG_DIR = "long/" + "d" * 130


def cases():
    """{name: (layer, skip_dirs, skip_files)}; the patterns are clean already."""
    c = {}
    c["after"] = (build([("f", "app/keep.conf"), ("d", "app/skipme"), ("f", "app/skipme/a.conf"),
                         ("f", "app/skipme/deep/b.conf"), ("d", "app/skipme/deep"), ("f", "app/skipme/deep/c.conf"),
                         ("f", "app/other.conf")]), ["**/skipme"], [])
    c["before"] = (build([("f", "app/skipme/early.conf"), ("d", "app"), ("d", "app/skipme"),
                          ("f", "app/skipme/late.conf"), ("f", "srv/skipme/never-recorded.conf")]), ["**/skipme"], [])
    # (the reference case is node_modules / node_modules2; Required itself refuses node_modules, so a file
    # there would show nothing -- the same shape under another name)
    c["sibling"] = (build([("d", "app/modules"), ("d", "app/modules2"), ("f", "app/modules/x.conf"),
                           ("f", "app/modules2/y.conf"), ("f", "app/modulesz.conf")]), ["app/modules"], [])
    c["skip-files"] = (build([("f", "secret.env"), ("f", "etc/app/secret.env"), ("f", "srv/secret.env"),
                              ("d", "etc/app/secret.env.d"), ("f", "etc/app/secret.env.d/x.conf"),
                              ("l", "etc/app/link.env")]),
                       [], ["secret.env", "etc/*/secret.env", "**/link.env"])
    c["pax-long-path"] = (build([("d", "data/skipme"), ("f", "data/skipme/" + LONG + ".conf"),
                                 ("f", "data/other/" + LONG + ".conf")], tarfile.PAX_FORMAT), ["data/skipme"], [])
    c["gnu-long-dir"] = (build([("d", LONG_DIR), ("f", LONG_DIR + "/in.conf"), ("f", "long/" + "d" * 129 + "/out.conf"),
                                ("d", "long/" + "e" * 130), ("f", "long/" + "e" * 130 + "/kept.conf")]),
                         ["long/d*"], [])
    c["rega-dir"] = (build([("0d", "old/skipme/"), ("f", "old/skipme/f.conf"), ("0f", "old/skipme/rega.conf"),
                            ("0f", "old/rega.conf"), ("f", "old/keep.conf")]), ["old/skipme"], [])
    c["markers"] = (build([("d", "w/skipme"), ("m", "w/skipme/.wh.gone"), ("m", "w/skipme/.wh..wh..opq"),
                           ("f", "w/skipme/x.conf"), ("m", "w/.wh.skipme"), ("f", "w/y.conf")]),
                    ["w/skipme", "**/.wh.*"], ["**/.wh.*"])
    c["malformed"] = (build([("d", "a/skipme"), ("f", "a/skipme/x.conf"), ("d", "a/other["), ("f", "a/b.conf"),
                             ("f", "a/other[/c.conf")]), ["**/skipme", "[", "a/other\\["], ["[", "**/b.conf"])
    c["parent"] = (build([("d", "a/b"), ("d", "c/d/e"), ("f", "a"), ("f", "a2"), ("f", "c"), ("f", "c/d"),
                          ("f", "a/bc"), ("f", "a/b/x")]), ["a/b", "c/d/e"], [])
    c["rel-failure"] = (build([("d", "../up"), ("d", "b"), ("f", "b/x.conf"), ("f", "../up/y.conf"),
                               ("f", "z.conf")]), ["../up", "b"], [])
    c["dot"] = (build([("f", "first.conf"), ("d", "."), ("f", "x.conf"), ("f", "deep/er/y.conf"),
                       ("f", "../out.conf")]), ["."], [])
    return c


def order_layer(n_before=10, n_between=80, n_after=110) -> bytes:
    """About 200 tiny entries: one file of z/skipme early, the directory's entry after n_before + 1 files,
    n_between other files, then the directory's files among n_after more -- more than a 64-entry chunk apart."""
    e = [("f", "z/skipme/early.conf")] + [("f", "pre/%d.conf" % i) for i in range(n_before)]
    e += [("d", "z/skipme")] + [("f", "mid/%d.conf" % i) for i in range(n_between)]
    for i in range(n_after):
        e.append(("f", ("z/skipme/late-%d.conf" if i % 5 == 0 else "post/%d.conf") % i))
    return build(e)


def window_layer(file_bytes=400 << 10, n=4) -> bytes:
    """The skipped directory's entry, then n files of file_bytes each, then files of the directory: in another
    window of the host walk when a window is shorter than n * file_bytes."""
    e = [("f", "w/skipme/early.conf"), ("d", "w/skipme")]
    e += [("f", "big/%d.log" % i, file_bytes) for i in range(n)]
    e += [("f", "w/skipme/late-%d.conf" % i) for i in range(3)] + [("f", "w/kept.conf")]
    return build(e)


def check_planted(analyzer: oan.SecretAnalyzer, layer: bytes):
    """Every regular file of the layer gives a finding without options (so a file wrongly kept or wrongly
    dropped shows in the findings)."""
    files = walk(layer)["kept"]
    got = {s["FilePath"] for s in analyze(analyzer, layer)}
    assert files and got == {"/" + fp for fp, _, _ in files}, sorted({"/" + fp for fp, _, _ in files} - got)
