"""SecretAnalyzer: pkg/fanal/analyzer/secret/secret.go over the MI355X engine.

Same names and behaviour as the Go analyzer (undistro/trivy @ 2024-12-20):

* ``SecretAnalyzer.Init(opt)``      -- secret.go:86-101 (ParseConfig + NewScanner)
* ``SecretAnalyzer.Required(p, fi)`` -- secret.go:152-190 (tsg_analyzer_required)
* ``SecretAnalyzer.Analyze(input)`` -- secret.go:103-150: binary gate, CR strip or
  printable extraction, "/" prefix for image files, Scan, nil without findings
* ``Type()`` = "secret" (analyzer/const.go:140), ``Version()`` = 1 (secret.go:26)

and the batched forms the engine is built for (the analyzer group's goroutine
per file, analyzer.go:403-455, becomes a batch collector feeding one arena):

* ``AnalyzeBatch(inputs)``  -- Analyze for many files, one GPU submission per arena
* ``AnalyzeLayer(tar)``     -- LayerTar.Walk (walker/tar.go:35-103) + AnalyzeFile's
  Required gate + Analyze for every regular file of an uncompressed layer,
  parsed natively into double-buffered pinned arenas (tsg_collector_add_tar)
* ``AnalyzeLayers(tars, base)`` -- the image artifact's layer pipeline
  (artifact/image/image.go:202-235): `parallel` layer walks at once into one
  engine, base layers with the secret analyzer disabled

Every transform runs in libtsg.so (include/tsg_analyzer.h); there is no CPU
fallback for the scan itself.
"""
import ctypes
import collections
import time
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from .. import _lib
from ..secret import NewScanner, ParseConfig, Secret
from ..secret.scanner import ScanResult

c = ctypes
TypeSecret = "secret"  # pkg/fanal/analyzer/const.go:140
version = 1            # secret.go:26
TSG_SKIPPED, TSG_FULL = -1, -2


class _CTarStats(c.Structure):
    _fields_ = [(n, c.c_uint64) for n in ("entries", "regular", "required", "added", "skipped_binary",
                                          "whiteouts", "opaque_dirs", "input_bytes")]


class _CDeviceFiles(c.Structure):  # tsg_device_files (versioned: struct_size first)
    _fields_ = [("struct_size", c.c_uint32), ("n_files", c.c_uint32), ("dev_arena", c.c_void_p),
                ("host_offsets", c.c_void_p), ("dev_offsets", c.c_void_p), ("paths", c.c_void_p),
                ("path_lens", c.c_void_p), ("dir", c.c_char_p)]


DEVICE_FILES_SIZE_V1 = _CDeviceFiles.dir.offset + c.sizeof(c.c_char_p)


class _CDeviceClassifyStats(c.Structure):  # tsg_device_classify_stats (versioned)
    _fields_ = [("struct_size", c.c_uint32), ("reserved", c.c_uint32), ("files", c.c_uint64),
                ("required", c.c_uint64), ("skipped_binary", c.c_uint64), ("pyc", c.c_uint64),
                ("ms_kernel", c.c_double), ("ms_total", c.c_double)]


DEVICE_CLASSIFY_STATS_SIZE_V1 = _CDeviceClassifyStats.ms_total.offset + c.sizeof(c.c_double)
XFORM_DROP = 3  # tsg_batch.transform: a file the analyzer skips, dropped from the scan


class _CDeviceTar(c.Structure):  # tsg_device_tar (versioned)
    _fields_ = [("struct_size", c.c_uint32), ("reserved", c.c_uint32), ("dev_tar", c.c_void_p),
                ("n_bytes", c.c_uint64)]


DEVICE_TAR_SIZE_V1 = _CDeviceTar.n_bytes.offset + c.sizeof(c.c_uint64)


class _CDeviceTarStats(c.Structure):  # tsg_device_tar_stats (versioned)
    _fields_ = [("struct_size", c.c_uint32), ("reserved", c.c_uint32), ("tar", _CTarStats)] + \
               [(n, c.c_uint64) for n in ("blocks", "candidates", "off_chain", "block_fetches", "ext_bytes",
                                          "kernel_runs")] + [("ms_kernel", c.c_double), ("ms_total", c.c_double)]

    def to_dict(self):
        d = {n: getattr(self.tar, n) for n in ("entries", "regular", "required", "whiteouts", "opaque_dirs")}
        d.update({n: getattr(self, n) for n, _ in self._fields_ if n not in ("struct_size", "reserved", "tar")})
        return d


DEVICE_TAR_STATS_SIZE_V1 = _CDeviceTarStats.ms_total.offset + c.sizeof(c.c_double)


class _CTarWalkStats(c.Structure):  # tsg_tar_walk_stats (versioned)
    _fields_ = [("struct_size", c.c_uint32), ("reserved", c.c_uint32), ("walk", c.c_uint32), ("fallback", c.c_uint32)] + \
               [(n, c.c_uint64) for n in ("chain_entries", "name_bytes", "segments", "device_bytes")] + \
               [(n, c.c_double) for n in ("ms_candidates", "ms_entries", "ms_mark", "ms_compact", "ms_copy", "ms_host")]

    def to_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n not in ("struct_size", "reserved", "walk")}
        d["walk"] = TAR_WALK_MODES[self.walk] if self.walk < len(TAR_WALK_MODES) else self.walk
        return d


TAR_WALK_STATS_SIZE_V1 = _CTarWalkStats.ms_host.offset + c.sizeof(c.c_double)
TAR_WALK_MODES = ("host", "gpu")  # tsg_analyzer_set_tar_walk
# tsg_tar_walk_stats.fallback: why the GPU walk's result was discarded and the host walk ran
TAR_WALK_FALLBACKS = ("", "size field", "PAX record", "PAX size form", "cap", "non-candidate header", "truncation",
                      "too many blocks")


class _CTarRequiredStats(c.Structure):  # tsg_tar_required_stats (versioned)
    _fields_ = [("struct_size", c.c_uint32), ("reserved", c.c_uint32), ("mode", c.c_uint32), ("reason", c.c_uint32)] + \
               [(n, c.c_uint64) for n in ("entries", "kept", "dropped", "ask_allow", "ask_name", "ask_dropped",
                                          "path_bytes")] + \
               [(n, c.c_double) for n in ("ms_kernel", "ms_copy", "ms_host")]

    def to_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n not in ("struct_size", "reserved", "mode")}
        d["mode"] = TAR_REQUIRED_MODES[self.mode] if self.mode < len(TAR_REQUIRED_MODES) else self.mode
        return d


TAR_REQUIRED_STATS_SIZE_V1 = _CTarRequiredStats.ms_host.offset + c.sizeof(c.c_double)
TAR_REQUIRED_MODES = ("host", "gpu")  # tsg_analyzer_set_tar_required
# tsg_tar_required_stats.reason: why Required ran on the host
TAR_REQUIRED_REASONS = ("", "setter off", "walk mode host", "skip options", "layer fell back to the host walk",
                        "an asked name was a skipped directory")


class _CTarRequiredSkipStats(c.Structure):  # tsg_tar_required_skip_stats (versioned)
    _fields_ = [("struct_size", c.c_uint32), ("reserved", c.c_uint32), ("mode", c.c_uint32), ("reason", c.c_uint32),
                ("dir_patterns", c.c_uint32), ("file_patterns", c.c_uint32)] + \
               [(n, c.c_uint64) for n in ("skipped_dirs", "skipped_files", "under_skipped_dir", "table_slots")] + \
               [("ms_kernel", c.c_double)]

    def to_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n not in ("struct_size", "reserved", "mode")}
        d["mode"] = TAR_REQUIRED_MODES[self.mode] if self.mode < len(TAR_REQUIRED_MODES) else self.mode
        return d


TAR_REQUIRED_SKIP_STATS_SIZE_V1 = _CTarRequiredSkipStats.ms_kernel.offset + c.sizeof(c.c_double)
# tsg_tar_required_skip_stats.reason: why the device stage did not honour the skip options
TAR_REQUIRED_SKIP_REASONS = ("", "setter off", "no skip options", "patterns unsupported",
                             "the required stage did not run", "an asked name was a skipped directory")


class _CDeviceTars(c.Structure):  # tsg_device_tars (versioned)
    _fields_ = [("struct_size", c.c_uint32), ("n_layers", c.c_uint32), ("layers", c.POINTER(_CDeviceTar))]


DEVICE_TARS_SIZE_V1 = _CDeviceTars.layers.offset + c.sizeof(c.c_void_p)
DEVICE_TARS_MAX_LAYERS = 65536


class _CTarForestStats(c.Structure):  # tsg_tar_forest_stats (versioned)
    _fields_ = [("struct_size", c.c_uint32), ("reserved", c.c_uint32)] + \
               [(n, c.c_uint64) for n in ("layers", "batched", "fallbacks", "passes", "virtual_blocks", "segments",
                                          "device_bytes")] + \
               [(n, c.c_double) for n in ("ms_candidates", "ms_entries", "ms_mark", "ms_compact", "ms_copy", "ms_host",
                                          "ms_total")]

    def to_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n not in ("struct_size", "reserved")}


TAR_FOREST_STATS_SIZE_V1 = _CTarForestStats.ms_total.offset + c.sizeof(c.c_double)


def layer_groups(nbytes: Sequence[int], base: Optional[Sequence[bool]] = None, group_bytes: int = 1 << 30):
    """How AnalyzeLayersDevice groups the layers of an image for its index calls: the layers that are no
    base layer, in order, in runs of at most group_bytes of layer bytes; a larger layer goes alone.
    Returns lists of layer numbers."""
    out, cur, tot = [], [], 0
    for k, n in enumerate(nbytes):
        if base is not None and base[k]:
            continue
        if cur and tot + int(n) > group_bytes:
            out.append(cur)
            cur, tot = [], 0
        cur.append(k)
        tot += int(n)
    if cur:
        out.append(cur)
    return out


class _CTarSkipStats(c.Structure):  # tsg_tar_skip_stats (versioned)
    _fields_ = [("struct_size", c.c_uint32), ("reserved", c.c_uint32)] + \
               [(n, c.c_uint64) for n in ("skipped_dirs", "skipped_files", "under_skipped_dir")]

    def to_dict(self):
        return {n: getattr(self, n) for n in TAR_SKIP_KEYS}


TAR_SKIP_KEYS = ("skipped_dirs", "skipped_files", "under_skipped_dir")
TAR_SKIP_STATS_SIZE_V1 = _CTarSkipStats.under_skipped_dir.offset + c.sizeof(c.c_uint64)


def _declare(L):
    if getattr(L, "_tsg_analyzer_declared", False):
        return
    if hasattr(L, "tsg_analyzer_set_tar_skip"):  # (absent from an older build of the library: TSG_LIB)
        L.tsg_analyzer_set_tar_skip.argtypes = [c.c_void_p, c.POINTER(c.c_char_p), c.c_uint32, c.POINTER(c.c_char_p),
                                                c.c_uint32]
        L.tsg_analyzer_get_tar_skip.argtypes = [c.c_void_p, c.POINTER(c.c_uint32), c.POINTER(c.c_uint32)]
        L.tsg_analyzer_tar_skip_stats.argtypes = [c.c_void_p, c.POINTER(_CTarSkipStats)]
        L.tsg_tar_index_skip_stats.argtypes = [c.c_void_p, c.POINTER(_CTarSkipStats)]
    if hasattr(L, "tsg_analyzer_set_tar_walk"):  # (absent from an older build of the library: TSG_LIB)
        L.tsg_analyzer_set_tar_walk.argtypes = [c.c_void_p, c.c_int]
        L.tsg_analyzer_get_tar_walk.argtypes = [c.c_void_p, c.POINTER(c.c_int)]
        L.tsg_tar_index_walk_stats.argtypes = [c.c_void_p, c.POINTER(_CTarWalkStats)]
        L.tsg_debug_tar_walk_last_fallback.argtypes = [c.c_void_p]
    if hasattr(L, "tsg_analyzer_set_tar_required"):  # (absent from an older build of the library: TSG_LIB)
        L.tsg_analyzer_set_tar_required.argtypes = [c.c_void_p, c.c_int]
        L.tsg_analyzer_get_tar_required.argtypes = [c.c_void_p, c.POINTER(c.c_int)]
        L.tsg_tar_index_required_stats.argtypes = [c.c_void_p, c.POINTER(_CTarRequiredStats)]
    if hasattr(L, "tsg_analyzer_set_tar_required_skip"):  # (absent from an older build of the library: TSG_LIB)
        L.tsg_analyzer_set_tar_required_skip.argtypes = [c.c_void_p, c.c_int]
        L.tsg_analyzer_get_tar_required_skip.argtypes = [c.c_void_p, c.POINTER(c.c_int)]
        L.tsg_tar_index_required_skip_stats.argtypes = [c.c_void_p, c.POINTER(_CTarRequiredSkipStats)]
    if hasattr(L, "tsg_analyzer_index_device_tars"):  # (absent from an older build of the library: TSG_LIB)
        L.tsg_analyzer_index_device_tars.argtypes = [c.c_void_p, c.POINTER(_CDeviceTars), c.POINTER(c.c_void_p),
                                                     c.POINTER(_CDeviceTarStats), c.POINTER(_CTarForestStats),
                                                     c.POINTER(c.c_uint32)]
    L.tsg_analyzer_classify_device.argtypes = [c.c_void_p, c.POINTER(_CDeviceFiles), c.c_void_p, c.c_void_p,
                                               c.POINTER(_CDeviceClassifyStats)]
    L.tsg_analyzer_submit_device.argtypes = [c.c_void_p, c.POINTER(_CDeviceFiles), c.POINTER(c.c_void_p)]
    L.tsg_analyzer_index_device_tar.argtypes = [c.c_void_p, c.POINTER(_CDeviceTar), c.POINTER(c.c_void_p),
                                                c.POINTER(_CDeviceTarStats)]
    L.tsg_tar_index_files.argtypes = [c.c_void_p]
    L.tsg_tar_index_files.restype = c.c_uint32
    L.tsg_tar_index_file.argtypes = [c.c_void_p, c.c_uint32, c.POINTER(c.c_void_p), c.POINTER(c.c_uint64),
                                     c.POINTER(c.c_uint64), c.POINTER(c.c_uint64)]
    L.tsg_tar_index_spans.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    L.tsg_analyzer_submit_device_tar.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32,
                                                 c.POINTER(c.c_void_p)]
    L.tsg_tar_index_free.argtypes = [c.c_void_p]
    L.tsg_is_binary.argtypes = [c.c_char_p, c.c_uint64]
    L.tsg_extract_printable.argtypes = [c.c_char_p, c.c_uint64, c.c_char_p]
    L.tsg_extract_printable.restype = c.c_uint64
    L.tsg_strip_cr.argtypes = [c.c_char_p, c.c_uint64, c.c_char_p]
    L.tsg_strip_cr.restype = c.c_uint64
    L.tsg_analyzer_new.argtypes = [c.c_void_p, c.c_char_p, c.POINTER(c.c_void_p)]
    L.tsg_analyzer_free.argtypes = [c.c_void_p]
    L.tsg_analyzer_walk_end.argtypes = [c.c_void_p]
    L.tsg_analyzer_set_walk_ahead.argtypes = [c.c_void_p, c.c_int]
    L.tsg_analyzer_required.argtypes = [c.c_void_p, c.c_char_p, c.c_uint64, c.c_int64]
    L.tsg_collector_new.argtypes = [c.c_void_p, c.c_uint64, c.POINTER(c.c_void_p)]
    L.tsg_collector_free.argtypes = [c.c_void_p]
    L.tsg_collector_add.argtypes = [c.c_void_p, c.c_char_p, c.c_uint64, c.c_char_p, c.c_char_p, c.c_uint64]
    L.tsg_collector_add.restype = c.c_int64
    L.tsg_collector_add_tar.argtypes = [c.c_void_p, c.c_void_p, c.c_uint64, c.POINTER(c.c_uint64),
                                        c.POINTER(_CTarStats)]
    L.tsg_collector_files.argtypes = [c.c_void_p]
    L.tsg_collector_files.restype = c.c_uint32
    L.tsg_collector_bytes.argtypes = [c.c_void_p]
    L.tsg_collector_bytes.restype = c.c_uint64
    L.tsg_collector_input_bytes.argtypes = [c.c_void_p]
    L.tsg_collector_input_bytes.restype = c.c_uint64
    L.tsg_collector_file.argtypes = [c.c_void_p, c.c_uint32, c.POINTER(c.c_void_p), c.POINTER(c.c_uint64),
                                     c.POINTER(c.c_void_p), c.POINTER(c.c_uint64), c.POINTER(c.c_int)]
    L.tsg_collector_submit.argtypes = [c.c_void_p, c.POINTER(c.c_void_p)]
    L.tsg_collector_reset.argtypes = [c.c_void_p]
    L.tsg_collector_set_gpu_transform.argtypes = [c.c_void_p, c.c_int]
    L.tsg_collector_set_gather.argtypes = [c.c_void_p, c.c_int]
    L.tsg_scan_wait.argtypes = [c.c_void_p, c.POINTER(c.c_void_p)]
    L._tsg_analyzer_declared = True


def _b(s) -> bytes:
    return s if isinstance(s, bytes) else str(s).encode("utf-8", "surrogateescape")


# ---- utils (pkg/fanal/utils/utils.go) -------------------------------------
def IsBinary(content: bytes, fileSize: int) -> bool:  # utils.go:85-103
    L = _lib.lib()
    _declare(L)
    return L.tsg_is_binary(content, min(int(fileSize), len(content))) == 1


def ExtractPrintableBytes(content: bytes) -> bytes:  # utils.go:128-160
    L = _lib.lib()
    _declare(L)
    out = c.create_string_buffer(len(content) + len(content) // 5 + 2)
    n = L.tsg_extract_printable(content, len(content), out)
    return out.raw[:n]


def StripCR(content: bytes) -> bytes:  # bytes.ReplaceAll(content, "\r", ""), secret.go:121
    L = _lib.lib()
    _declare(L)
    out = c.create_string_buffer(max(1, len(content)))
    n = L.tsg_strip_cr(content, len(content), out)
    return out.raw[:n]


# ---- analyzer types (pkg/fanal/analyzer/analyzer.go) -----------------------
@dataclass
class SecretScannerOption:  # analyzer.go:56-58
    ConfigPath: str = ""


@dataclass
class AnalyzerOptions:  # analyzer.go:44-54 (the secret analyzer's part)
    SecretScannerOption: SecretScannerOption = field(default_factory=SecretScannerOption)


@dataclass
class FileInfo:  # the os.FileInfo facts the analyzer reads
    size: int

    def Size(self) -> int:
        return self.size


@dataclass
class AnalysisInput:  # analyzer.go:81-88
    Dir: str
    FilePath: str
    Info: FileInfo
    Content: bytes  # or a readable binary file object


@dataclass
class AnalysisResult:  # analyzer.go:99-136 (the Secrets part)
    Secrets: List[Secret] = field(default_factory=list)

    def Merge(self, other: Optional["AnalysisResult"]):  # analyzer.go:251-301
        if other is not None:
            self.Secrets.extend(other.Secrets)

    def Sort(self):  # analyzer.go:225-234
        self.Secrets.sort(key=lambda s: _b(s.FilePath))
        for sec in self.Secrets:
            if sec.Findings:
                sec.Findings.sort(key=lambda f: (_b(f.RuleID), f.StartLine))


def _read(content) -> bytes:
    if isinstance(content, (bytes, bytearray, memoryview)):
        return bytes(content)
    data = content.read()
    if hasattr(content, "seek"):
        content.seek(0)
    return data


class Collector:
    """A batch arena (tsg_collector): Analyze's pre-scan half for many files."""

    def __init__(self, analyzer: "SecretAnalyzer", arena_bytes: int = 256 << 20, gpu_transform: bool = False,
                 gather: bool = False):
        """gpu_transform: files enter the arena as read and the CR strip / printable
        extraction runs on the GPU at scan time (tsg_collector_set_gpu_transform).
        gather (needs gpu_transform; tar walks): the walk copies nothing -- the GPU gathers
        the batch's files from the layer buffer, which the caller registers with
        HostRegister(buf, mapped=True) and keeps until the batch is waited on; one batch
        holds one layer's files (tsg_collector_set_gather)."""
        self._L = analyzer._L
        self._an = analyzer  # the C collector borrows the analyzer (and its walk state)
        if not analyzer._h:
            raise RuntimeError("Collector: the analyzer has no scanner (Init first)")
        h = c.c_void_p()
        if self._L.tsg_collector_new(analyzer._h, int(arena_bytes), c.byref(h)) != 0:
            raise RuntimeError("tsg_collector_new failed: %s" % _lib.last_error(self._L))
        self._h = h
        if gpu_transform and self._L.tsg_collector_set_gpu_transform(h, 1) != 0:
            raise RuntimeError("tsg_collector_set_gpu_transform failed: %s" % _lib.last_error(self._L))
        if gather and self._L.tsg_collector_set_gather(h, 1) != 0:
            raise RuntimeError("tsg_collector_set_gather failed: %s" % _lib.last_error(self._L))
        self.gather = bool(gather)
        self._keep = []

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.tsg_collector_free(self._h)
            self._h = None

    def add(self, path: str, dir_: str, content: bytes) -> int:
        p = _b(path)
        return self._L.tsg_collector_add(self._h, p, len(p), _b(dir_), content, len(content))

    def add_tar(self, buf, cursor: int, stats: _CTarStats):
        """Walk the layer from ``cursor``: (1 when full / 0 at the end, next cursor).
        With the analyzer's walk-ahead on, the next window of the layer is indexed on a
        background thread after a return of 1, so the analyzer keeps ``buf`` alive until
        the walk ends (0, an error, or SecretAnalyzer.WalkEnd) -- tsg_analyzer.h."""
        cur = c.c_uint64(cursor)
        addr = buf.ctypes.data if hasattr(buf, "ctypes") else c.cast(c.c_char_p(buf), c.c_void_p).value
        self._an._walk_buf = buf
        rc = self._L.tsg_collector_add_tar(self._h, addr, len(buf), c.byref(cur), c.byref(stats))
        if rc != 1:  # the walk ended (the C side joined any background index)
            self._an._walk_buf = None
        if rc < 0:
            raise ValueError("tar layer: %s" % _lib.last_error(self._L))
        return rc, cur.value

    def files(self) -> int:
        return self._L.tsg_collector_files(self._h)

    def nbytes(self) -> int:
        return self._L.tsg_collector_bytes(self._h)

    def input_bytes(self) -> int:
        return self._L.tsg_collector_input_bytes(self._h)

    def file(self, i: int):
        """(scan path, transformed content, binary) of batch file i."""
        pp, pl, cp, cl, bn = c.c_void_p(), c.c_uint64(), c.c_void_p(), c.c_uint64(), c.c_int()
        if self._L.tsg_collector_file(self._h, i, c.byref(pp), c.byref(pl), c.byref(cp), c.byref(cl),
                                      c.byref(bn)) != 0:
            raise IndexError(i)
        path = c.string_at(pp, pl.value).decode("utf-8", "surrogateescape")
        data = c.string_at(cp, cl.value) if cl.value else b""
        return path, data, bool(bn.value)

    def paths(self) -> List[str]:
        return [self.file(i)[0] for i in range(self.files())]

    def submit(self) -> "PendingBatch":
        h = c.c_void_p()
        if self._L.tsg_collector_submit(self._h, c.byref(h)) != 0:
            raise RuntimeError("tsg_collector_submit failed: %s" % _lib.last_error(self._L))
        return PendingBatch(self, h)

    def reset(self):
        self._L.tsg_collector_reset(self._h)


class PendingBatch:
    def __init__(self, coll: Collector, h):
        self.coll, self._h = coll, h

    def __del__(self):
        # dropped without wait() (e.g. an exception in the caller's loop): the
        # scan thread still reads the collector's arena, so join it first
        h = getattr(self, "_h", None)
        if h:
            r = c.c_void_p()
            self.coll._L.tsg_scan_wait(h, c.byref(r))
            self._h = None
            if r:
                self.coll._L.tsg_result_free(r)
            self.coll.reset()

    def wait(self, materialize: bool = True):
        """Per batch file: the Secret when it has findings (Analyze's result), else None.
        materialize=False: only the batch's tsg_stats (dict), no per-file objects."""
        r = c.c_void_p()
        rc = self.coll._L.tsg_scan_wait(self._h, c.byref(r))
        self._h = None
        if rc != 0:
            raise RuntimeError("tsg_scan failed: %s" % _lib.last_error(self.coll._L))
        res = ScanResult(_ScannerRef(self.coll._L), r)
        out = ([s if s.Findings else None for s in res.secrets(self.coll.paths())] if materialize
               else res.stats())
        del res
        self.coll.reset()
        return out


class _ScannerRef:  # what ScanResult needs of its scanner
    def __init__(self, L):
        self._L = L


class PendingDeviceAnalyze:
    """AnalyzeDeviceAsync in flight (tsg_analyzer_submit_device).  Keeps the arena tensor, the
    offsets and the paths referenced until wait(): the native thread borrows them."""

    def __init__(self, analyzer, h, paths, image, keep):
        self._an, self._h, self._paths, self._image, self._keep = analyzer, h, paths, image, keep
        self.result = None  # the ScanResult, after wait() (fetch_stats(), stats())

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:  # dropped without wait(): join the native thread before the buffers go
            r = c.c_void_p()
            self._an._L.tsg_scan_wait(h, c.byref(r))
            self._h = None
            if r:
                self._an._L.tsg_result_free(r)

    def wait(self, materialize: bool = True):
        """Per file what Analyze returns: an AnalysisResult when it has findings, else None.
        materialize=False (bench): the ScanResult alone, no per-file objects."""
        L = self._an._L
        r = c.c_void_p()
        rc = L.tsg_scan_wait(self._h, c.byref(r))
        self._h = None
        self._keep = None
        if rc != 0:
            raise RuntimeError("AnalyzeDevice failed: %s" % _lib.last_error(L))
        self.result = ScanResult(_ScannerRef(L), r)
        if not materialize:
            return self.result
        paths = self._paths
        if isinstance(paths, np.ndarray):  # a char* table
            paths = [c.string_at(int(p)).decode("utf-8", "surrogateescape") for p in paths]
        if self._image:  # the scan paths: "/" + FilePath for image files (secret.go:130-135)
            paths = ["/" + p if isinstance(p, str) else b"/" + p for p in paths]
        return [AnalysisResult(Secrets=[s]) if s.Findings else None for s in self.result.secrets(paths)]


class DeviceTarIndex:
    """The index of a tar layer resident in HBM (tsg_tar_index): its Required-accepted regular files in
    walk order.  Keeps the layer tensor referenced; the layer must stay unchanged while it lives."""

    def __init__(self, analyzer, h, keep, stats):
        self._an, self._h, self._keep, self.stats = analyzer, h, keep, stats
        L = analyzer._L
        self.n = L.tsg_tar_index_files(h)
        self.start = np.zeros(max(1, self.n), dtype=np.uint64)  # where each entry's header chain begins
        self.data_off = np.zeros(max(1, self.n), dtype=np.uint64)
        self.size = np.zeros(max(1, self.n), dtype=np.uint64)
        L.tsg_tar_index_spans(h, self.start.ctypes.data, self.data_off.ctypes.data, self.size.ctypes.data)

    def __del__(self):
        if getattr(self, "_h", None):
            self._an._L.tsg_tar_index_free(self._h)
            self._h = None

    @property
    def walk_stats(self) -> dict:
        """How the index was made (tsg_tar_index_walk_stats): the walk mode, the fallback reason (0: none),
        what the GPU walk handed over and its stage times."""
        ws = _CTarWalkStats()
        ws.struct_size = TAR_WALK_STATS_SIZE_V1
        if not hasattr(self._an._L, "tsg_tar_index_walk_stats"):  # an older build: the host walk, nothing to report
            return ws.to_dict()
        if self._an._L.tsg_tar_index_walk_stats(self._h, c.byref(ws)) != 0:
            raise RuntimeError("tsg_tar_index_walk_stats failed: %s" % _lib.last_error(self._an._L))
        return ws.to_dict()

    @property
    def required_stats(self) -> dict:
        """Where this index's Required ran (tsg_tar_index_required_stats): the mode in force, the reason
        when it was the host (TAR_REQUIRED_REASONS), what the device decided and asked, the stage's times."""
        rs = _CTarRequiredStats()
        rs.struct_size = TAR_REQUIRED_STATS_SIZE_V1
        if not hasattr(self._an._L, "tsg_tar_index_required_stats"):  # an older build: the host, setter absent
            rs.reason = 1
            return rs.to_dict()
        if self._an._L.tsg_tar_index_required_stats(self._h, c.byref(rs)) != 0:
            raise RuntimeError("tsg_tar_index_required_stats failed: %s" % _lib.last_error(self._an._L))
        return rs.to_dict()

    @property
    def required_skip_stats(self) -> dict:
        """How this index's skip options were honoured (tsg_tar_index_required_skip_stats): the switch, the
        reason when it was not the device stage (TAR_REQUIRED_SKIP_REASONS), the patterns, the three counts,
        the table's slots and the stage's kernel time."""
        ss = _CTarRequiredSkipStats()
        ss.struct_size = TAR_REQUIRED_SKIP_STATS_SIZE_V1
        if not hasattr(self._an._L, "tsg_tar_index_required_skip_stats"):  # an older build: the switch is absent
            ss.reason = 1
            return ss.to_dict()
        if self._an._L.tsg_tar_index_required_skip_stats(self._h, c.byref(ss)) != 0:
            raise RuntimeError("tsg_tar_index_required_skip_stats failed: %s" % _lib.last_error(self._an._L))
        return ss.to_dict()

    @property
    def skip_stats(self) -> dict:
        """What the layer walker's skip options dropped from this index (tsg_tar_index_skip_stats)."""
        st = _CTarSkipStats()
        st.struct_size = TAR_SKIP_STATS_SIZE_V1
        if not hasattr(self._an._L, "tsg_tar_index_skip_stats"):  # an older build: no options, nothing dropped
            return st.to_dict()
        if self._an._L.tsg_tar_index_skip_stats(self._h, c.byref(st)) != 0:
            raise RuntimeError("tsg_tar_index_skip_stats failed: %s" % _lib.last_error(self._an._L))
        return st.to_dict()

    def path(self, i: int) -> str:
        pp, pl = c.c_void_p(), c.c_uint64()
        if self._an._L.tsg_tar_index_file(self._h, i, c.byref(pp), c.byref(pl), None, None) != 0:
            raise IndexError(i)
        return c.string_at(pp, pl.value).decode("utf-8", "surrogateescape")

    def files(self):
        """[(path, data_off, size)]"""
        return [(self.path(i), int(self.data_off[i]), int(self.size[i])) for i in range(self.n)]

    def batches(self, arena_bytes: int):
        """[(first, count)]: runs of files spanning at most arena_bytes of the layer, cut at entry
        boundaries; a larger single file goes alone."""
        out, i = [], 0
        end = self.data_off[:self.n] + self.size[:self.n]
        while i < self.n:
            start = int(self.start[i])  # the batch's arena begins where file i's header chain does
            j = int(np.searchsorted(end, start + int(arena_bytes), side="right"))
            j = min(self.n, max(j, i + 1))
            out.append((i, j - i))
            i = j
        return out

    def submit(self, first: int, count: int) -> "PendingDeviceLayer":
        h = c.c_void_p()
        if self._an._L.tsg_analyzer_submit_device_tar(self._an._h, self._h, first, count, c.byref(h)) != 0:
            raise RuntimeError("tsg_analyzer_submit_device_tar failed: %s" % _lib.last_error(self._an._L))
        return PendingDeviceLayer(self, h, first, count)


class PendingDeviceLayer:
    """A batch of a resident layer in flight (tsg_analyzer_submit_device_tar).  The batch's result has
    2 count + 1 pseudo-files, gap, file, gap, ...: wait() hides that and gives one entry per index file."""

    def __init__(self, index: DeviceTarIndex, h, first, count):
        self._ix, self._h, self.first, self.count = index, h, first, count
        self.result = None  # the ScanResult, after wait()

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:  # dropped without wait(): join the native thread before the index and the layer go
            r = c.c_void_p()
            self._ix._an._L.tsg_scan_wait(h, c.byref(r))
            self._h = None
            if r:
                self._ix._an._L.tsg_result_free(r)

    def wait(self, materialize: bool = True):
        """Per index file of the batch the Secret when it has findings, else None (materialize=False:
        the batch's tsg_stats dict)."""
        L = self._ix._an._L
        r = c.c_void_p()
        rc = L.tsg_scan_wait(self._h, c.byref(r))
        self._h = None
        if rc != 0:
            raise RuntimeError("AnalyzeLayerDevice failed: %s" % _lib.last_error(L))
        self.result = ScanResult(_ScannerRef(L), r)
        if not materialize:  # the scan counters, with what came back from HBM and the census's time
            d = self.result.stats()
            fs, ws, ss = self.result.fetch_stats(), self.result.fetch_window_stats(), self.result.split_stats()
            d.update({"fetch_files": fs["files"], "fetch_bytes": fs["bytes"], "window_bytes": ws["window_bytes"],
                      "ms_census": ss["ms_census"]})
            return d
        paths = [""] * (2 * self.count + 1)
        for j in range(self.count):
            paths[2 * j + 1] = "/" + self._ix.path(self.first + j)  # image files (secret.go:130-135)
        return [s if s.Findings else None for s in self.result.secrets(paths)[1::2]]


def _pipeline(colls, fill, take):
    """Fill the collectors in turn (fill(coll) -> True at the end of the input) and submit
    each batch; with n collectors, n - 1 scans stay in flight while the next batch is
    filled (a collector is refilled only after its scan was taken).  Returns the seconds
    spent filling and waiting."""
    inflight = collections.deque()
    k, done = 0, False
    t_walk = t_wait = 0.0
    try:
        while not done:
            coll = colls[k]
            t0 = time.perf_counter()
            done = fill(coll)
            t_walk += time.perf_counter() - t0
            if coll.files():
                inflight.append(coll.submit())
            t0 = time.perf_counter()
            while len(inflight) > len(colls) - 1:
                take(inflight.popleft())
            t_wait += time.perf_counter() - t0
            k = (k + 1) % len(colls)
        t0 = time.perf_counter()
        while inflight:
            take(inflight.popleft())
        t_wait += time.perf_counter() - t0
    finally:
        while inflight:  # an error left batches in flight: join them before the arenas go
            inflight.popleft().__del__()
    return t_walk, t_wait


class SecretAnalyzer:
    """analyzer/secret.SecretAnalyzer bound to the MI355X engine."""

    def __init__(self, scanner=None, configPath: str = "", device: int = 0, lib=None, host_only: bool = False):
        """lib / host_only: as trivy_amd.secret.Scanner (tests drive the host logic on CPU)."""
        self._L = lib if lib is not None else _lib.lib()
        _declare(self._L)
        self.device = device
        self._host_only = host_only
        self._h = None
        self._walk_buf = None  # the layer buffer of a walk in progress (Collector.add_tar)
        self._layer_walker = None  # walker.LayerTar (set_layer_walker)
        self.scanner = None
        self.configPath = configPath
        if scanner is not None:
            self._bind(scanner, configPath)

    def _bind(self, scanner, configPath):
        if self._h:
            self._L.tsg_analyzer_free(self._h)
            self._h = None
            self._walk_buf = None
        self.scanner = scanner
        self.configPath = configPath
        h = c.c_void_p()
        if self._L.tsg_analyzer_new(scanner._h, _b(configPath), c.byref(h)) != 0:
            raise RuntimeError("tsg_analyzer_new failed: %s" % _lib.last_error(self._L))
        self._h = h
        # walk-ahead: this object keeps the layer buffer alive until the walk ends
        self._L.tsg_analyzer_set_walk_ahead(h, 1)
        if self._layer_walker is not None:  # a new native analyzer: the options go with this object
            self.set_layer_walker(self._layer_walker)

    def WalkEnd(self):
        """Ends a tar walk (joins its background index): the layer buffer may go after this."""
        if self._h:
            self._L.tsg_analyzer_walk_end(self._h)
        self._walk_buf = None

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.tsg_analyzer_free(self._h)  # joins a walk's background index
            self._h = None
        self._walk_buf = None

    # --- reference API ------------------------------------------------------
    def Init(self, opt: AnalyzerOptions):  # secret.go:86-101
        path = opt.SecretScannerOption.ConfigPath
        if self.scanner is not None and path == self.configPath:
            return None
        try:
            cfg = ParseConfig(path)
        except Exception as e:  # xerrors.Errorf("secret config error: %w", err)
            raise RuntimeError("secret config error: %s" % e)
        self._bind(NewScanner(cfg, device=self.device, lib=self._L, host_only=self._host_only), path)
        return None

    def Type(self) -> str:
        return TypeSecret

    def Version(self) -> int:
        return version

    def Required(self, filePath: str, fi) -> bool:  # secret.go:152-190
        p = _b(filePath)
        size = fi.Size() if hasattr(fi, "Size") else int(fi)
        return self._L.tsg_analyzer_required(self._h, p, len(p), int(size)) == 1

    def Analyze(self, input: AnalysisInput) -> Optional[AnalysisResult]:  # secret.go:103-150
        return self.AnalyzeBatch([input])[0]

    # --- batched forms ------------------------------------------------------
    def AnalyzeBatch(self, inputs: Sequence[AnalysisInput], arena_bytes: int = 256 << 20,
                     gpu_transform: bool = False) -> List[Optional[AnalysisResult]]:
        out: List[Optional[AnalysisResult]] = [None] * len(inputs)
        coll = Collector(self, arena_bytes, gpu_transform)
        idx: List[int] = []

        def flush():
            if not idx:
                return
            for k, sec in zip(idx, coll.submit().wait()):
                if sec is not None:
                    out[k] = AnalysisResult(Secrets=[sec])
            idx.clear()

        for k, inp in enumerate(inputs):
            data = _read(inp.Content)
            for _ in range(2):
                r = coll.add(inp.FilePath, inp.Dir, data)
                if r == TSG_FULL:
                    flush()
                    continue
                if r >= 0:
                    idx.append(k)
                elif r != TSG_SKIPPED:
                    raise RuntimeError("tsg_collector_add failed: %s" % _lib.last_error(self._L))
                break
        flush()
        return out

    # --- files resident in HBM (no host copy of the bytes) --------------------
    def _device_files(self, dev_arena, offsets, paths, dir_, dev_offsets, nbytes):
        """tsg_device_files over a resident arena, checked by Scanner._device_batch (tensor or integer
        pointer, device, alignment, the 64-byte tail); returns (struct, references to keep)."""
        if self.scanner is None:
            raise RuntimeError("the analyzer has no scanner (Init first)")
        ptr, d_offs, offs, keep = self.scanner._device_batch(dev_arena, offsets, nbytes, dev_offsets)
        n = len(offs) - 1
        if len(paths) != n:
            raise ValueError("AnalyzeDevice: %d paths for %d files" % (len(paths), n))
        d = _b(dir_ or "")
        if isinstance(paths, np.ndarray) and paths.dtype == np.uint64:  # a char* table (NUL-terminated strings
            f = _CDeviceFiles(DEVICE_FILES_SIZE_V1, n, ptr, offs.ctypes.data, d_offs,  # the caller keeps alive)
                              paths.ctypes.data, None, d)
            return f, (keep, offs, paths, d)
        pb = [_b(p) for p in paths]
        parr = (c.c_char_p * max(1, n))(*pb)
        plen = np.array([len(p) for p in pb], dtype=np.uint64) if n else np.zeros(1, np.uint64)
        f = _CDeviceFiles(DEVICE_FILES_SIZE_V1, n, ptr, offs.ctypes.data, d_offs, c.cast(parr, c.c_void_p).value,
                          plen.ctypes.data, d)
        return f, (keep, offs, pb, parr, plen, d)

    def ClassifyDevice(self, dev_arena, offsets, paths, dir_="", dev_offsets=None, nbytes=None, stats=None):
        """What Analyze decides per file before Scan, for files resident in HBM: (kinds, binary) as
        numpy u8 arrays -- kinds[i] the tsg_batch.transform value (3 dropped: Required false, or binary
        and not .pyc; 2 a binary .pyc; 1 text), binary[i] ScanArgs.Binary.  The binary gate runs on
        the GPU over the arena (tsg_analyzer_classify_device); stats (a dict) gets the call's counters."""
        f, keep = self._device_files(dev_arena, offsets, paths, dir_, dev_offsets, nbytes)
        kinds = np.zeros(max(1, f.n_files), dtype=np.uint8)
        binary = np.zeros(max(1, f.n_files), dtype=np.uint8)
        st = _CDeviceClassifyStats()
        st.struct_size = DEVICE_CLASSIFY_STATS_SIZE_V1
        if self._L.tsg_analyzer_classify_device(self._h, c.byref(f), kinds.ctypes.data, binary.ctypes.data,
                                                c.byref(st)) != 0:
            raise RuntimeError("tsg_analyzer_classify_device failed: %s" % _lib.last_error(self._L))
        if stats is not None:
            stats.update({k: getattr(st, k) for k, _ in st._fields_ if k not in ("struct_size", "reserved")})
        del keep
        return kinds[:f.n_files], binary[:f.n_files]

    def AnalyzeDeviceAsync(self, dev_arena, offsets, paths, dir_="", dev_offsets=None,
                           nbytes=None) -> PendingDeviceAnalyze:
        """AnalyzeDevice, pipelined (tsg_analyzer_submit_device): several may be in flight; .wait()
        gives the results.  The pending object keeps the tensors and arrays referenced."""
        f, keep = self._device_files(dev_arena, offsets, paths, dir_, dev_offsets, nbytes)
        h = c.c_void_p()
        if self._L.tsg_analyzer_submit_device(self._h, c.byref(f), c.byref(h)) != 0:
            raise RuntimeError("tsg_analyzer_submit_device failed: %s" % _lib.last_error(self._L))
        return PendingDeviceAnalyze(self, h, paths, not dir_, (keep, f, dev_arena, dev_offsets))

    def AnalyzeDevice(self, dev_arena, offsets, paths, dir_="", dev_offsets=None,
                      nbytes=None) -> List[Optional[AnalysisResult]]:
        """Analyze (secret.go:103-150) for files whose bytes exist only in HBM: dev_arena holds them as
        read, back to back (a torch.uint8 tensor on the scanner's device or an integer pointer with
        nbytes; 16-B aligned, 64 readable bytes past offsets[-1]), offsets / paths are on the host.
        Required runs on the host, IsBinary over the heads on the GPU; skipped files are dropped from
        the scan where they lie, .pyc binaries and CRLF text are transformed on the GPU, and only the
        files that got candidates come back for the exact pass.  Shaped like AnalyzeBatch."""
        return self.AnalyzeDeviceAsync(dev_arena, offsets, paths, dir_, dev_offsets, nbytes).wait()

    # --- a tar layer resident in HBM -------------------------------------------
    def _device_layer(self, dev_layer, nbytes):
        """Checks a resident layer (a torch.uint8 tensor, or an integer device pointer with nbytes) against
        the contract: on the scanner's device, contiguous, 16-B aligned, nbytes + 64 readable bytes."""
        if self.scanner is None:
            raise RuntimeError("the analyzer has no scanner (Init first)")
        if isinstance(dev_layer, int):
            if nbytes is None:
                raise ValueError("AnalyzeLayerDevice: an integer device pointer needs nbytes")
            return dev_layer, int(nbytes), None
        import torch
        t = dev_layer
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
            raise ValueError("AnalyzeLayerDevice: the layer must be a torch.uint8 tensor or an integer device pointer")
        if t.device.type != "cuda" or (self.device is not None and t.device.index != self.device):
            raise ValueError("AnalyzeLayerDevice: the layer is on %s, the scanner on device %s" % (t.device, self.device))
        if not t.is_contiguous():
            raise ValueError("AnalyzeLayerDevice: the layer must be contiguous")
        n = t.numel() - 64 if nbytes is None else int(nbytes)
        if n < 0 or t.numel() < n + 64:
            raise ValueError("AnalyzeLayerDevice: the tensor holds %d bytes; nbytes + 64 = %d are read"
                             % (t.numel(), n + 64))
        return t.data_ptr(), n, t

    def set_layer_walker(self, walker=None):
        """The layer walker's options (walker.LayerTar, from walker.NewLayerTar(Option(SkipFiles, SkipDirs)):
        tar.go:23-33) for every layer walk of this analyzer -- AnalyzeLayer in copy and gather mode,
        AnalyzeLayers and LayerWorkers (the workers' analyzers inherit them), IndexDevice, IndexLayerDevice
        and AnalyzeLayerDevice in both tar-walk modes (tsg_analyzer_set_tar_skip).  None, or a walker without
        patterns, restores the walk without options.  Ends a tar walk in progress."""
        sd = [_b(p) for p in (walker.skipDirs if walker is not None else [])]
        sf = [_b(p) for p in (walker.skipFiles if walker is not None else [])]
        if not hasattr(self._L, "tsg_analyzer_set_tar_skip"):
            if sd or sf:
                raise RuntimeError("set_layer_walker: this build of the library has no tsg_analyzer_set_tar_skip")
            self._layer_walker = None
            return
        if self._h:
            ad = (c.c_char_p * max(1, len(sd)))(*sd)
            af = (c.c_char_p * max(1, len(sf)))(*sf)
            if self._L.tsg_analyzer_set_tar_skip(self._h, ad, len(sd), af, len(sf)) != 0:
                raise ValueError("tsg_analyzer_set_tar_skip failed: %s" % _lib.last_error(self._L))
            self._walk_buf = None
        self._layer_walker = walker if (sd or sf) else None

    def layer_walker(self):
        return self._layer_walker

    def tar_skip_stats(self) -> dict:
        """What the options dropped in this analyzer's host walks (AnalyzeLayer), summed since
        set_layer_walker (tsg_analyzer_tar_skip_stats)."""
        st = _CTarSkipStats()
        st.struct_size = TAR_SKIP_STATS_SIZE_V1
        if self._h and hasattr(self._L, "tsg_analyzer_tar_skip_stats"):
            if self._L.tsg_analyzer_tar_skip_stats(self._h, c.byref(st)) != 0:
                raise RuntimeError("tsg_analyzer_tar_skip_stats failed: %s" % _lib.last_error(self._L))
        return st.to_dict()

    def set_tar_walk(self, mode):
        """Where IndexDevice / IndexLayerDevice / AnalyzeLayerDevice walk the header chain
        (tsg_analyzer_set_tar_walk): "host" (the default: the GPU finds the header candidates, the host walks
        the chain over their records) or "gpu" (the GPU walks the chain and hands over one record and the
        name per entry; the same index, and a layer it does not complete is indexed by "host")."""
        if mode not in TAR_WALK_MODES:
            raise ValueError("set_tar_walk: mode must be one of %s" % (TAR_WALK_MODES,))
        if self._L.tsg_analyzer_set_tar_walk(self._h, TAR_WALK_MODES.index(mode)) != 0:
            raise ValueError("tsg_analyzer_set_tar_walk failed: %s" % _lib.last_error(self._L))

    def tar_walk(self) -> str:
        m = c.c_int(0)
        if self._L.tsg_analyzer_get_tar_walk(self._h, c.byref(m)) != 0:
            raise RuntimeError("tsg_analyzer_get_tar_walk failed: %s" % _lib.last_error(self._L))
        return TAR_WALK_MODES[m.value]

    def set_tar_required(self, mode):
        """Where the path work and Required of a resident layer's index run (tsg_analyzer_set_tar_required):
        "host" (the default) or "gpu" (a device stage behind the GPU walk hands over only the files Required
        keeps and what it leaves to the host; the same index).  In force only with set_tar_walk("gpu"), without
        skip options, on a layer the GPU walk completes: DeviceTarIndex.required_stats says which ran and why."""
        if mode not in TAR_REQUIRED_MODES:
            raise ValueError("set_tar_required: mode must be one of %s" % (TAR_REQUIRED_MODES,))
        if self._L.tsg_analyzer_set_tar_required(self._h, TAR_REQUIRED_MODES.index(mode)) != 0:
            raise ValueError("tsg_analyzer_set_tar_required failed: %s" % _lib.last_error(self._L))

    def tar_required(self) -> str:
        m = c.c_int(0)
        if self._L.tsg_analyzer_get_tar_required(self._h, c.byref(m)) != 0:
            raise RuntimeError("tsg_analyzer_get_tar_required failed: %s" % _lib.last_error(self._L))
        return TAR_REQUIRED_MODES[m.value]

    def set_tar_required_skip(self, mode):
        """Whether that device stage honours the layer walker's skip options itself
        (tsg_analyzer_set_tar_required_skip): "host" (the default: with options set the host half runs) or "gpu"
        (patterns of the forms L, **/L, L/** and **/*S are matched on the GPU, and files under a directory
        skipped earlier in the layer are dropped there; any other pattern sends the whole option set to the host
        half).  DeviceTarIndex.required_skip_stats says which ran and why; the index is the same."""
        if mode not in TAR_REQUIRED_MODES:
            raise ValueError("set_tar_required_skip: mode must be one of %s" % (TAR_REQUIRED_MODES,))
        if self._L.tsg_analyzer_set_tar_required_skip(self._h, TAR_REQUIRED_MODES.index(mode)) != 0:
            raise ValueError("tsg_analyzer_set_tar_required_skip failed: %s" % _lib.last_error(self._L))

    def tar_required_skip(self) -> str:
        m = c.c_int(0)
        if self._L.tsg_analyzer_get_tar_required_skip(self._h, c.byref(m)) != 0:
            raise RuntimeError("tsg_analyzer_get_tar_required_skip failed: %s" % _lib.last_error(self._L))
        return TAR_REQUIRED_MODES[m.value]

    def last_tar_fallback(self) -> int:
        """tsg_tar_walk_stats.fallback of the last "gpu"-mode index call, also of one that raised."""
        return int(self._L.tsg_debug_tar_walk_last_fallback(self._h))

    def IndexDevice(self, dev_layer, nbytes=None, stats=None) -> DeviceTarIndex:
        """The DeviceTarIndex of a layer resident in HBM (tsg_analyzer_index_device_tar)."""
        ptr, n, keep = self._device_layer(dev_layer, nbytes)
        if ptr % 16 != 0:
            raise ValueError("AnalyzeLayerDevice: the layer must be 16-B aligned")
        t = _CDeviceTar(DEVICE_TAR_SIZE_V1, 0, ptr, n)
        st = _CDeviceTarStats()
        st.struct_size = DEVICE_TAR_STATS_SIZE_V1
        h = c.c_void_p()
        rc = self._L.tsg_analyzer_index_device_tar(self._h, c.byref(t), c.byref(h), c.byref(st))
        if rc == -3:  # a malformed archive (-2: a HIP error, also one in a copy the walk asked for)
            raise ValueError("tar layer: %s" % _lib.last_error(self._L))
        if rc != 0:
            raise RuntimeError("tsg_analyzer_index_device_tar failed: %s" % _lib.last_error(self._L))
        d = st.to_dict()
        ix = DeviceTarIndex(self, h, keep, d)
        d.update(ix.skip_stats)
        if stats is not None:
            stats.update(d)
        return ix

    def IndexLayerDevice(self, dev_layer, nbytes=None, stats=None):
        """Where the files of an uncompressed tar layer resident in HBM are: ([(path, data_off, size)] of
        the regular files Required accepts, in walk order; the stats dict).  The GPU finds the blocks that
        parse as headers, the host follows the chain over them (tsg_analyzer_index_device_tar)."""
        ix = self.IndexDevice(dev_layer, nbytes, stats)
        return ix.files(), ix.stats

    def AnalyzeLayerDevice(self, dev_layer, nbytes=None, arena_bytes: int = 1 << 30, depth: int = 2,
                           stats: Optional[dict] = None, materialize: bool = True) -> AnalysisResult:
        """AnalyzeLayer for a layer whose bytes exist only in HBM (a torch.uint8 tensor holding nbytes + 64
        bytes, nbytes = numel - 64 by default; or an integer pointer with nbytes): exactly what AnalyzeLayer
        returns for the same bytes on the host.  The layer is indexed on the GPU, cut into batches of at
        most arena_bytes of layer span at entry boundaries (a larger single file goes alone), and each
        batch is scanned in place -- the layer itself is the arena -- with up to `depth` in flight."""
        ix = self.IndexDevice(dev_layer, nbytes)
        result = AnalysisResult()
        scan_tot: dict = {}
        inflight = collections.deque()

        def take(p):
            out = p.wait(materialize)
            if materialize:
                result.Secrets.extend(sec for sec in out if sec is not None)
            else:
                for k2, v in out.items():
                    scan_tot[k2] = scan_tot.get(k2, 0) + v
        t0 = time.perf_counter()
        try:
            for first, count in ix.batches(arena_bytes):
                while len(inflight) >= max(1, depth):
                    take(inflight.popleft())
                inflight.append(ix.submit(first, count))
            while inflight:
                take(inflight.popleft())
        finally:
            while inflight:  # an error left batches in flight: join them before the index goes
                inflight.popleft().__del__()
        if stats is not None:
            stats.update(ix.stats)
            stats["walk"] = ix.walk_stats
            stats.update({"scan_" + k2: v for k2, v in scan_tot.items()})
            stats.update({"files": ix.n, "scan_s": time.perf_counter() - t0})
        return result

    # --- all layers of an image resident in HBM --------------------------------
    def _device_layers(self, layers):
        """[(ptr, nbytes, keep)] of the layers of an image: each a torch.uint8 tensor (nbytes = numel - 64), a
        (tensor, nbytes) pair or a (ptr, nbytes) pair, checked as _device_layer checks one.  Slices of one
        resident buffer are layers like any other."""
        out = []
        for k, ly in enumerate(layers):
            try:
                r = self._device_layer(*ly) if isinstance(ly, (tuple, list)) else self._device_layer(ly, None)
                if r[0] % 16 != 0:
                    raise ValueError("AnalyzeLayerDevice: the layer must be 16-B aligned")
            except ValueError as e:
                raise ValueError("layer %d: %s" % (k, e)) from None
            out.append(r)
        return out

    def _index_device_layers(self, resolved, which):
        """One tsg_analyzer_index_device_tars call over the layers `which` of `resolved`:
        ([DeviceTarIndex], the forest stats dict)."""
        if not hasattr(self._L, "tsg_analyzer_index_device_tars"):
            raise RuntimeError("this build of the library has no tsg_analyzer_index_device_tars")
        n = len(which)
        arr = (_CDeviceTar * n)(*[_CDeviceTar(DEVICE_TAR_SIZE_V1, 0, resolved[k][0], resolved[k][1]) for k in which])
        t = _CDeviceTars(DEVICE_TARS_SIZE_V1, n, arr)
        st = (_CDeviceTarStats * n)()
        for x in st:
            x.struct_size = DEVICE_TAR_STATS_SIZE_V1
        fs = _CTarForestStats()
        fs.struct_size = TAR_FOREST_STATS_SIZE_V1
        hs = (c.c_void_p * n)()
        bad = c.c_uint32(0)
        rc = self._L.tsg_analyzer_index_device_tars(self._h, c.byref(t), hs, st, c.byref(fs), c.byref(bad))
        if rc == -3:  # a malformed archive: "layer j: " + the host walk's message, j counted in this call
            msg = _lib.last_error(self._L)
            pre = "layer %d: " % bad.value
            raise ValueError("tar layer %d: %s" % (which[bad.value], msg[len(pre):] if msg.startswith(pre) else msg))
        if rc != 0:
            raise RuntimeError("tsg_analyzer_index_device_tars failed: %s" % _lib.last_error(self._L))
        out = []
        for j, k in enumerate(which):
            d = st[j].to_dict()
            ix = DeviceTarIndex(self, c.c_void_p(hs[j]), resolved[k][2], d)
            d.update(ix.skip_stats)
            out.append(ix)
        return out, fs.to_dict()

    def IndexLayersDevice(self, layers, stats: Optional[list] = None) -> List[DeviceTarIndex]:
        """The DeviceTarIndex of every layer of an image resident in HBM, made by one call
        (tsg_analyzer_index_device_tars): in tar-walk mode "gpu" one GPU pass walks the header chains of all
        layers.  Each layer is a torch.uint8 tensor (nbytes = numel - 64), a (tensor, nbytes) pair or a
        (ptr, nbytes) pair; slices of one resident buffer are allowed (a slice's 64 readable bytes past its
        end are whatever follows it in the buffer).  Each index is what IndexDevice gives for that layer alone
        and keeps its tensor alive.  stats (a list): the per-layer stats dicts, then the forest stats."""
        resolved = self._device_layers(layers)
        ixs, fs = self._index_device_layers(resolved, list(range(len(resolved))))
        if stats is not None:
            stats[:] = [ix.stats for ix in ixs] + [fs]
        return ixs

    def AnalyzeLayersDevice(self, layers, base: Optional[Sequence[bool]] = None, arena_bytes: int = 1 << 30,
                            depth: int = 2, group_bytes: int = 1 << 30, materialize: bool = True,
                            stats: Optional[list] = None) -> List[AnalysisResult]:
        """AnalyzeLayers for an image whose layers exist only in HBM (layers as IndexLayersDevice takes them):
        per layer exactly what AnalyzeLayerDevice returns, sorted as AnalyzeLayers sorts.  A base layer is
        neither indexed nor scanned and yields an empty result.  The other layers are taken in order in groups
        of at most group_bytes of layer bytes (layer_groups); a background thread indexes group g + 1 with one
        tsg_analyzer_index_device_tars call while this thread submits and collects the batches of group g.  All
        batches of all layers share one window of `depth` in flight, which is not drained at a layer or group
        boundary.  stats (a list): per layer the dict AnalyzeLayerDevice fills (None for base layers), then one
        dict of the forest stats summed over the groups with index_s, scan_s and wall_s.  An error stops the
        pipeline, joins every batch in flight and the index thread, and is raised: ValueError("tar layer k:
        ...") for a malformed layer, RuntimeError otherwise."""
        import queue
        import threading
        t_wall = time.perf_counter()
        resolved = self._device_layers(layers)
        n = len(resolved)
        base = list(base) if base is not None else [False] * n
        if len(base) != n:
            raise ValueError("AnalyzeLayersDevice: base flags must match the layers")
        groups = layer_groups([r[1] for r in resolved], base, group_bytes)
        results = [AnalysisResult() for _ in range(n)]
        per: List[Optional[dict]] = [None] * n
        scan_tot: List[dict] = [{} for _ in range(n)]
        span = [[None, None] for _ in range(n)]  # first submit, last collect
        forest: dict = {}
        index_s = [0.0]
        q: "queue.Queue" = queue.Queue()
        go = threading.Semaphore(0)  # one release per group the indexer may start on
        stop = threading.Event()

        def indexer():
            for gi, g in enumerate(groups):
                go.acquire()
                if stop.is_set():
                    return
                t0 = time.perf_counter()
                try:
                    item = self._index_device_layers(resolved, g)
                except BaseException as e:
                    q.put(e)
                    return
                index_s[0] += time.perf_counter() - t0
                q.put(item)

        inflight = collections.deque()

        def take():
            k, p = inflight.popleft()
            out = p.wait(materialize)
            span[k][1] = time.perf_counter()
            if materialize:
                results[k].Secrets.extend(sec for sec in out if sec is not None)
            else:
                for k2, v in out.items():
                    scan_tot[k][k2] = scan_tot[k].get(k2, 0) + v
        th = threading.Thread(target=indexer, name="tsg-layers-index")
        th.start()
        scan_s = 0.0
        try:
            go.release()  # group 0
            for g in groups:
                item = q.get()
                if isinstance(item, BaseException):
                    raise item
                go.release()  # the next group is indexed while this one's batches are submitted and collected
                ixs, fs = item
                for k2, v in fs.items():
                    forest[k2] = max(forest.get(k2, 0), v) if k2 == "device_bytes" else forest.get(k2, 0) + v
                t0 = time.perf_counter()
                for k, ix in zip(g, ixs):
                    per[k] = dict(ix.stats)
                    per[k]["walk"] = ix.walk_stats
                    per[k]["files"] = ix.n
                    span[k][0] = time.perf_counter()
                    for first, count in ix.batches(arena_bytes):
                        while len(inflight) >= max(1, depth):
                            take()
                        inflight.append((k, ix.submit(first, count)))
                scan_s += time.perf_counter() - t0
            t0 = time.perf_counter()
            while inflight:
                take()
            scan_s += time.perf_counter() - t0
        finally:
            while inflight:  # an error left batches in flight: join them before the indexes go
                inflight.popleft()[1].__del__()
            stop.set()
            go.release()
            th.join()
        for k in range(n):
            results[k].Sort()
            if per[k] is not None:
                per[k].update({"scan_" + k2: v for k2, v in scan_tot[k].items()})
                per[k]["scan_s"] = (span[k][1] - span[k][0]) if span[k][1] is not None else 0.0
        if stats is not None:
            forest.update({"index_s": index_s[0], "scan_s": scan_s, "wall_s": time.perf_counter() - t_wall})
            stats[:] = per + [forest]
        return results

    def AnalyzeFS(self, root: str, opt=None, arena_bytes: int = 256 << 20, stats: Optional[dict] = None,
                  materialize: bool = True, colls: Optional[List["Collector"]] = None,
                  gpu_transform: bool = False) -> AnalysisResult:
        """`trivy fs` for this analyzer: FS.Walk (walker/fs.go:25-78) + AnalyzeFile's Required +
        Analyze for every regular file under root, read natively into double-buffered pinned
        arenas (tsg_collector_add_fs); one collector fills while the others' batches scan.
        FilePath is the path relative to root (Dir = root, no '/' prefix: secret.go:130-135)."""
        from ..walker import FS, Option, _CFsAddStats
        w = FS().Walk(root, opt or Option(), lib=self._L)
        result = AnalysisResult()
        scan_tot: dict = {}
        st = _CFsAddStats()

        def take(p):
            out = p.wait(materialize)
            if materialize:
                result.Secrets.extend(sec for sec in out if sec is not None)
            else:
                for k2, v in out.items():
                    scan_tot[k2] = scan_tot.get(k2, 0) + v
        colls = colls or [Collector(self, arena_bytes, gpu_transform), Collector(self, arena_bytes, gpu_transform)]
        def fill(coll):
            rc = self._L.tsg_collector_add_fs(coll._h, w._h, c.byref(st))
            if rc < 0:
                raise RuntimeError("fs walk: %s" % _lib.last_error(self._L))
            return rc == 0
        t_walk, t_wait = _pipeline(colls, fill, take)
        if stats is not None:
            stats.update({n: getattr(st, n) for n, _ in st._fields_})
            stats.update(w.stats())
            stats.update({"scan_" + k2: v for k2, v in scan_tot.items()})
            stats.update({"walk_s": t_walk, "wait_s": t_wait})
        result.Sort()
        return result

    def AnalyzeLayer(self, layer, arena_bytes: int = 256 << 20, stats: Optional[dict] = None,
                     materialize: bool = True, colls: Optional[List[Collector]] = None,
                     gpu_transform: bool = False, gather: bool = False,
                     registered: bool = False) -> AnalysisResult:
        """Every regular file of an uncompressed tar layer (bytes or a uint8 numpy array),
        as the image artifact's AnalyzeFile(dir="") would run it.  The collectors (two by
        default) are filled in turn while the others' batches are on the GPU.  materialize=False
        (bench): findings stay in the engine; stats gets the summed scan counters.
        gather (with gpu_transform; or collectors made with gather=True): the GPU reads the files
        in the layer itself (no arena copy); the layer, a uint8 numpy array, is registered
        page-locked and mapped for the call unless `registered` says the caller holds it so
        (HostRegister(layer, mapped=True): a pinned layer-buffer pool registers once)."""
        result = AnalysisResult()
        scan_tot: dict = {}

        def take(p):
            out = p.wait(materialize)
            if materialize:
                result.Secrets.extend(sec for sec in out if sec is not None)
            else:
                for k2, v in out.items():
                    scan_tot[k2] = scan_tot.get(k2, 0) + v
        st = _CTarStats()
        skip0 = self.tar_skip_stats()
        colls = colls or [Collector(self, arena_bytes, gpu_transform or gather, gather) for _ in range(2)]
        cursor = 0
        unregister = None
        if any(cl.gather for cl in colls) and not registered:
            from ..secret.scanner import HostRegister
            if not hasattr(layer, "ctypes"):
                raise TypeError("AnalyzeLayer(gather): the layer must be a numpy uint8 array")
            unregister = HostRegister(layer, self._L, mapped=True)

        def fill(coll):
            nonlocal cursor
            rc, cursor = coll.add_tar(layer, cursor, st)
            if rc == 1 and coll.files() == 0:
                raise RuntimeError("tar layer: an entry does not fit an empty collector")
            return rc == 0
        try:
            t_walk, t_wait = _pipeline(colls, fill, take)
        finally:  # the layer buffer may go away after this call (tsg_analyzer.h buffer lifetime)
            self.WalkEnd()
            if unregister is not None:  # every batch read from it was waited on (_pipeline)
                unregister()
        if stats is not None:
            stats.update({n: getattr(st, n) for n, _ in st._fields_})
            stats.update({k2: v - skip0[k2] for k2, v in self.tar_skip_stats().items()})  # this layer's
            stats.update({"scan_" + k2: v for k2, v in scan_tot.items()})
            stats.update({"walk_s": t_walk, "wait_s": t_wait})
        return result


    def LayerWorkers(self, parallel: int = 2, arena_bytes: int = 256 << 20, collectors: int = 2,
                     gpu_transform: bool = False, gather: bool = False) -> list:
        """AnalyzeLayers' workers, for reuse across calls: per worker an analyzer bound to this scanner
        (its own tar-walk state) and its collectors (pinned arenas: allocating them per call would
        cost a hipHostMalloc each, and freeing them waits for the device)."""
        out = []
        for _ in range(max(1, parallel)):
            sub = SecretAnalyzer(self.scanner, self.configPath, device=self.device, lib=self._L,
                                 host_only=self._host_only)
            sub.set_layer_walker(self._layer_walker)
            out.append((sub, [Collector(sub, arena_bytes, gpu_transform or gather, gather)
                              for _ in range(max(1, collectors))]))
        return out

    def AnalyzeLayers(self, layers: Sequence, base: Optional[Sequence[bool]] = None, parallel: int = 2,
                      arena_bytes: int = 256 << 20, collectors: int = 2, gpu_transform: bool = False,
                      materialize: bool = True, stats: Optional[list] = None,
                      workers: Optional[list] = None, gather: bool = False,
                      registered: bool = False) -> List[AnalysisResult]:
        """The image artifact's layer inspection for this analyzer (pkg/fanal/artifact/image/image.go:
        202-235): a pipeline of `parallel` workers over the layers, each running inspectLayer's walk
        (AnalyzeLayer) of one layer at a time; a base layer (base[i] true, the image's base diff IDs)
        has the secret analyzer disabled (image.go:208-211) and yields an empty result without a walk.
        Each worker owns an analyzer (its own tar-walk state) and collectors bound to this scanner, so
        the walks of several layers feed the one engine -- its staging ring interleaves their batches'
        copies and kernels.  Returns one AnalysisResult per layer, in the order given, each sorted as
        inspectLayer sorts its result (analyzer.go:225-234).  stats (a list): per layer, the
        AnalyzeLayer stats dict (None for base layers).  workers: from LayerWorkers (then `parallel`,
        `arena_bytes`, `collectors`, `gpu_transform` and `gather` are theirs).  gather / registered:
        as AnalyzeLayer (the layers are then uint8 numpy arrays)."""
        import threading
        if self.scanner is None:
            raise RuntimeError("AnalyzeLayers: the analyzer has no scanner (Init first)")
        n = len(layers)
        base = list(base) if base is not None else [False] * n
        if len(base) != n:
            raise ValueError("AnalyzeLayers: base flags must match the layers")
        results: List[Optional[AnalysisResult]] = [None] * n
        per: List[Optional[dict]] = [None] * n
        todo = collections.deque(i for i in range(n) if not base[i])
        for i in range(n):
            if base[i]:
                results[i] = AnalysisResult()
        lock = threading.Lock()
        errors: List[BaseException] = []

        if workers is None:
            workers = self.LayerWorkers(min(parallel, max(1, len(todo))), arena_bytes, collectors, gpu_transform,
                                        gather)

        for sub, _ in workers:  # (workers made before the options were set: they inherit them now)
            if sub._layer_walker != self._layer_walker:
                sub.set_layer_walker(self._layer_walker)

        def worker(sub, colls):
            while True:
                with lock:
                    if errors or not todo:
                        return
                    i = todo.popleft()
                st: dict = {}
                try:
                    r = sub.AnalyzeLayer(layers[i], stats=st, materialize=materialize, colls=colls,
                                         registered=registered)
                except BaseException as e:  # the pipeline stops at the first error (parallel.Pipeline)
                    with lock:
                        errors.append(e)
                    return
                r.Sort()
                results[i], per[i] = r, st

        threads = [threading.Thread(target=worker, args=w, name="tsg-layer-%d" % k)
                   for k, w in enumerate(workers[:max(1, len(todo))])]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errors:
            raise errors[0]
        if stats is not None:
            stats[:] = per
        return results  # type: ignore[return-value]


def NewSecretAnalyzer(s=None, configPath: str = "") -> SecretAnalyzer:  # secret.go:79-84
    return SecretAnalyzer(s, configPath)
