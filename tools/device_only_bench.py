"""Mirrored vs device-only scans of an HBM-resident C2-generator corpus (measured, not gated).

The corpus (trivy_amd.corpus.generate, CR-stripped, a few GB) is resident in HBM.  After a warm-up,
blocks of `--block` mirrored scans (host arena + device arena: the exact pass reads the host
copy) alternate with blocks of device-only scans (host_arena NULL: the candidate files are
fetched from HBM), `--steps` scans of each in all, in one process on one scanner, pipelined
`--depth` deep as bench.py's C2 steps are.  Printed, and written as one JSON line:

  ms per step of both modes (wall time of a block / its scans),
  the fetched files and bytes per step, ms_fetch (plan + pack + copies, HIP events),
  the rounds and direct files,
  overlap_ms: how much of the fetch ran beside other work of the pipeline --
      ms_gpu_total + ms_fetch - the device-only ms per step, clamped to [0, ms_fetch]
      (0: every fetch extended its step by its whole length; ms_fetch: it was hidden).

--analyze: the analyzer on the same generator's corpus as read (CRLF files not stripped) resident
in HBM -- blocks of scan_device with caller-supplied kinds and binary flags (computed once, by
ClassifyDevice) alternate with blocks of AnalyzeDevice, which classifies every step.  Printed:
ms of classify_heads_kernel (HIP events) and of the whole classify call (offsets, kernel,
read-back, the host's Required pass), ms per step of both modes, and the kernel's traffic bound
(320 B per file plus the offsets).

--fetch windows: three modes interleaved in the same way -- mirrored, device-only with the files
fetch, device-only with the windows fetch (Scanner.set_fetch_mode, --fwd / --fwd-cap / --back) --
and, for the windows mode, the window stats per step (granules, runs, window bytes, sparse / whole /
fallback files and the fallback's share of the files with candidates, ms_fallback) beside the fetch
stats of both device-only modes.

--analyze --resident split: AnalyzeDevice alone, blocks in chunked mode alternating with blocks in
split mode (Scanner.set_resident_transform) on one scanner, with the files fetch or, with --fetch
windows, the windows fetch in force for both.  Printed: ms per step of both modes with every
block's figure (the claim to check: the split's slowest block is below the chunked mode's fastest),
the split stats (ms_census against the arena's size among them), the fetch and window stats and
ms_gpu_total of both.

--layer [--layer-gb G]: one uncompressed tar layer as bench.py's C4 generator makes it
(trivy_amd.corpus.generate_layer), put in HBM once.  Blocks of AnalyzeLayerDevice -- the GPU indexes
the resident layer's headers, the host follows the chain, every batch is scanned where it lies --
alternate with blocks of AnalyzeLayer(gather=True) on the page-locked, mapped host copy (the fastest
host layer path), in one process on one scanner, with --fetch / --resident in force for both.  One
JSON line per mode: ms per step with every block's figure, the index's ms_kernel / ms_total and
counters, the bytes fetched per step and the host CPUs busy (process CPU time / wall time).

--layers N [--layer-mb M | --layer-gb G]: an image of N layers resident in HBM as slices of one buffer
(N = 5: bench.py's five-layer C4 image of G GB; otherwise N layers of M MB).  Blocks of
AnalyzeLayersDevice -- one index call per group of layers, one window for all batches -- alternate
with blocks of the loop of AnalyzeLayerDevice it replaces and of AnalyzeLayers(gather=True) on the
host copies, all in tar-walk mode "gpu"; with --index-only, one tsg_analyzer_index_device_tars call
against the loop of single-layer index calls.  One JSON line per mode: ms per step (median, min,
max of the blocks), the host CPUs, the findings (equal in every mode), the forest stats and the
share of the index time that ran beside scans.

--required host|gpu|both (with --layer --walk gpu|both, and with --layers): where the path work and
Required of a GPU-walked layer run (SecretAnalyzer.set_tar_required).  gpu and both add the modes
ending in "-req", in the same interleaved blocks; with --index-only their lines carry the stage's
counts and times ("required").

--required-skip host|gpu|both (with --skip-dirs / --skip-files and --required gpu|both): whether the
GPU's Required stage honours the skip options itself (SecretAnalyzer.set_tar_required_skip).  gpu
and both add the modes "...-req+skip@gpu" (--layer) or "...-req@gpu" (--layers, where the options
then hold for every mode), in the same interleaved blocks; with --index-only their lines carry the
skip stage's counts, its table size and its kernel time ("required_skip").

Usage: python tools/device_only_bench.py [--gb 4] [--steps 20] [--warmup 5] [--depth 3]
                                         [--analyze [--resident split]] [--layer [--layer-gb 4]]
                                         [--layers N [--layer-mb 2] [--group-mb 1024] [--index-only]]
                                         [--fetch windows [--fwd N] [--fwd-cap N] [--back N]] [--out FILE]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=4.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--block", type=int, default=5, help="scans of one mode before the other takes its turn")
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--analyze", action="store_true", help="the AnalyzeDevice leg instead of mirrored / device-only")
    ap.add_argument("--fetch", choices=["files", "windows"], default="files",
                    help="windows: the three-mode leg (mirrored / files fetch / windows fetch)")
    ap.add_argument("--resident", choices=["chunked", "split"], default="chunked",
                    help="with --analyze; split: chunked and split blocks of AnalyzeDevice interleaved")
    ap.add_argument("--layer", action="store_true", help="the resident tar layer leg")
    ap.add_argument("--layer-gb", type=float, default=4.0)
    ap.add_argument("--layers", type=int, default=0,
                    help="the resident image leg: an image of this many layers, all in HBM as slices of one buffer; 5: "
                         "bench.py's five-layer C4 image of --layer-gb in all (34/26/20/12/8 %%); otherwise equal layers "
                         "of --layer-mb each.  AnalyzeLayersDevice (one index call per group, one window for all batches) "
                         "against the loop of AnalyzeLayerDevice in gpu walk mode and against AnalyzeLayers(gather=True); "
                         "with --index-only one tsg_analyzer_index_device_tars call against the loop of single-layer "
                         "index calls")
    ap.add_argument("--layer-mb", type=float, default=2.0, help="--layers: the size of each of the equal layers")
    ap.add_argument("--group-mb", type=int, default=1024, help="--layers: AnalyzeLayersDevice's group_bytes")
    ap.add_argument("--arena-mb", type=int, default=256, help="--layer: batch size of both modes")
    ap.add_argument("--collectors", type=int, default=6, help="--layer: the host mode's collectors")
    ap.add_argument("--walk", choices=("host", "gpu", "both"), default="host",
                    help="--layer: where the resident layer's header chain is walked (SecretAnalyzer.set_tar_walk); "
                         "both: a block of each per round, interleaved")
    ap.add_argument("--layer-format", choices=("ustar", "pax"), default="ustar",
                    help="--layer: pax rewrites the generated layer with a PAX x header (path, mtime) before every entry")
    ap.add_argument("--required", choices=("host", "gpu", "both"), default="host",
                    help="--layer / --layers: where a GPU-walked layer's path work and Required run "
                         "(SecretAnalyzer.set_tar_required); gpu and both need the GPU walk (--layer: --walk gpu or both) "
                         "and add the modes ending in -req, interleaved with the others")
    ap.add_argument("--index-only", action="store_true", help="--layer: time IndexDevice alone, no scans, no host leg")
    ap.add_argument("--skip-dirs", default="", help="--layer: LayerTar skipDirs patterns, comma-separated; every mode "
                    "then also runs with the options set (mode name + \"+skip\"), in the same interleaved blocks")
    ap.add_argument("--skip-files", default="", help="--layer: LayerTar skipFiles patterns, comma-separated")
    ap.add_argument("--required-skip", choices=("host", "gpu", "both"), default="host",
                    help="with skip options and --required gpu|both: whether the GPU's Required stage honours them "
                         "(SecretAnalyzer.set_tar_required_skip); gpu and both add the modes ...-req+skip@gpu, and "
                         "--layers (where the options then hold for every mode) ...-req@gpu")
    ap.add_argument("--fwd", type=int, default=None)
    ap.add_argument("--fwd-cap", type=int, default=None)
    ap.add_argument("--back", type=int, default=None)
    args = ap.parse_args()
    if args.layers:
        return layers_leg(args)
    if args.layer:
        return layer_leg(args)
    if args.analyze and args.resident == "split":
        return resident_leg(args)
    if args.analyze:
        return analyze_leg(args)
    if args.fetch == "windows":
        return windows_leg(args)

    import torch
    import trivy_amd.secret as secret
    from trivy_amd import corpus

    R = corpus.generate(int(args.gb * 1e9), seed=corpus.SEED, crlf_share=0.05)
    C = R.stripped()
    del R
    dev = torch.device("cuda", 0)
    d_arena = torch.from_numpy(C.arena).to(dev)  # (the generator's arena carries the 64 bytes of slack)
    d_offs = torch.from_numpy(C.offsets.view(np.int64)).to(dev)
    torch.cuda.synchronize()
    sc = secret.NewScanner(None, device=0, calibration=C.arena[:min(C.n_bytes, 16_000_000)])

    def submit(device_only):
        if device_only:
            return sc.scan_device_async(d_arena, C.offsets, C.path_ptrs, dev_offsets=d_offs)
        return sc.scan_arena_async(C.arena, C.offsets, C.path_ptrs, dev_arena=d_arena.data_ptr(),
                                   dev_offsets=d_offs.data_ptr())

    def block(device_only, n):
        """n pipelined scans of one mode: (seconds, their results' stats, fetch stats)."""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        inflight, st, fs = [], [], []
        for _ in range(n):
            inflight.append(submit(device_only))
            if len(inflight) >= args.depth:
                r = inflight.pop(0).wait()
                st.append(r.stats())
                fs.append(r.fetch_stats())
        while inflight:
            r = inflight.pop(0).wait()
            st.append(r.stats())
            fs.append(r.fetch_stats())
        return time.perf_counter() - t0, st, fs

    for mode in (False, True):
        block(mode, args.warmup)
    per = {False: [], True: []}
    stats = {False: [], True: []}
    fetch = []
    done = 0
    while done < args.steps:
        n = min(args.block, args.steps - done)
        for mode in (False, True):
            s, st, fs = block(mode, n)
            per[mode].append(1e3 * s / n)
            stats[mode] += st
            if mode:
                fetch += fs
        done += n
    findings = {m: stats[m][-1]["findings"] for m in (False, True)}
    assert findings[False] == findings[True], findings

    def med(xs):
        return float(statistics.median(xs))

    ms_m, ms_d = med(per[False]), med(per[True])
    ms_gpu = med([s["ms_gpu_total"] for s in stats[True]])
    ms_fetch = med([f["ms_fetch"] for f in fetch])
    out = {
        "tool": "device_only_bench", "gb": C.n_bytes / 1e9, "files": int(C.n_files), "steps": args.steps,
        "block": args.block, "depth": args.depth,
        "mirrored_ms_per_step": ms_m, "device_only_ms_per_step": ms_d,
        "mirrored_blocks_ms": per[False], "device_only_blocks_ms": per[True],
        "mirrored_gbps": C.n_bytes / 1e6 / ms_m, "device_only_gbps": C.n_bytes / 1e6 / ms_d,
        "ms_gpu_total": ms_gpu,
        "mirrored_ms_gpu_total": med([s["ms_gpu_total"] for s in stats[False]]),
        "fetch_files_per_step": med([f["files"] for f in fetch]),
        "fetch_bytes_per_step": med([f["bytes"] for f in fetch]),
        "fetch_rounds": med([f["rounds"] for f in fetch]),
        "fetch_direct_files": med([f["direct_files"] for f in fetch]),
        "ms_fetch": ms_fetch,
        "fetch_gbps": med([f["bytes"] for f in fetch]) / 1e6 / ms_fetch if ms_fetch > 0 else 0.0,
        "overlap_ms": max(0.0, min(ms_fetch, ms_gpu + ms_fetch - ms_d)),
        "candidates": int(stats[True][-1]["candidates"]), "findings": int(findings[True]),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


def windows_leg(args):
    import torch
    import trivy_amd.secret as secret
    from trivy_amd import corpus

    R = corpus.generate(int(args.gb * 1e9), seed=corpus.SEED, crlf_share=0.05)
    C = R.stripped()
    del R
    dev = torch.device("cuda", 0)
    d_arena = torch.from_numpy(C.arena).to(dev)
    d_offs = torch.from_numpy(C.offsets.view(np.int64)).to(dev)
    torch.cuda.synchronize()
    sc = secret.NewScanner(None, device=0, calibration=C.arena[:min(C.n_bytes, 16_000_000)])
    MODES = ("mirrored", "files", "windows")

    def submit(mode):
        if mode == "mirrored":
            return sc.scan_arena_async(C.arena, C.offsets, C.path_ptrs, dev_arena=d_arena.data_ptr(),
                                       dev_offsets=d_offs.data_ptr())
        if mode == "windows":  # (the options hold for the scans submitted from here on)
            sc.set_fetch_mode("windows", back=args.back, fwd=args.fwd, fwd_cap=args.fwd_cap)
        else:
            sc.set_fetch_mode("files")
        return sc.scan_device_async(d_arena, C.offsets, C.path_ptrs, dev_offsets=d_offs)

    def block(mode, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        inflight, res = [], []
        for _ in range(n):
            inflight.append(submit(mode))
            if len(inflight) >= args.depth:
                res.append(inflight.pop(0).wait())
        while inflight:
            res.append(inflight.pop(0).wait())
        s = time.perf_counter() - t0
        return s, [(r.stats(), r.fetch_stats(), r.fetch_window_stats()) for r in res]

    for mode in MODES:
        block(mode, args.warmup)
    per = {m: [] for m in MODES}
    rec = {m: [] for m in MODES}
    done = 0
    while done < args.steps:
        n = min(args.block, args.steps - done)
        for mode in MODES:
            s, r = block(mode, n)
            per[mode].append(1e3 * s / n)
            rec[mode] += r
        done += n
    sc.set_fetch_mode("windows", back=args.back, fwd=args.fwd, fwd_cap=args.fwd_cap)
    options = sc.fetch_options()  # (the effective values of the windows steps)
    sc.set_fetch_mode("files")
    findings = {m: rec[m][-1][0]["findings"] for m in MODES}
    assert len(set(findings.values())) == 1, findings

    def med(xs):
        return float(statistics.median(xs))

    out = {"tool": "device_only_bench --fetch windows", "gb": C.n_bytes / 1e9, "files": int(C.n_files),
           "steps": args.steps, "block": args.block, "depth": args.depth, "options": options,
           "candidates": int(rec["windows"][-1][0]["candidates"]), "findings": int(findings["windows"])}
    for m in MODES:
        out[m + "_ms_per_step"] = med(per[m])
        out[m + "_blocks_ms"] = per[m]
        out[m + "_ms_gpu_total"] = med([r[0]["ms_gpu_total"] for r in rec[m]])
        out[m + "_ms_host_exact"] = med([r[0]["ms_host_exact"] for r in rec[m]])
    for m in ("files", "windows"):
        for k in ("files", "bytes", "rounds", "direct_files", "ms_fetch"):
            out["%s_fetch_%s" % (m, k)] = med([r[1][k] for r in rec[m]])
    for k in ("granules", "runs", "window_bytes", "sparse_files", "whole_files", "fallback_files", "fallback_bytes",
              "ms_fallback"):
        out["windows_" + k] = med([r[2][k] for r in rec["windows"]])
    with_cands = out["windows_sparse_files"] + out["windows_whole_files"] + out["windows_fallback_files"]
    out["windows_fallback_share"] = out["windows_fallback_files"] / with_cands if with_cands else 0.0
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


def analyze_leg(args):
    import torch
    import trivy_amd.secret as secret
    from trivy_amd import corpus
    from trivy_amd.analyzer import SecretAnalyzer

    R = corpus.generate(int(args.gb * 1e9), seed=corpus.SEED, crlf_share=0.05)  # the bytes as read
    dev = torch.device("cuda", 0)
    d_arena = torch.from_numpy(R.arena).to(dev)
    d_offs = torch.from_numpy(R.offsets.view(np.int64)).to(dev)
    torch.cuda.synchronize()
    sc = secret.NewScanner(None, device=0, calibration=R.arena[:min(R.n_bytes, 16_000_000)])
    an = SecretAnalyzer(sc)
    classify = []
    for _ in range(args.warmup + 5):
        st = {}
        kinds, binary = an.ClassifyDevice(d_arena, R.offsets, R.path_ptrs, "/corpus", dev_offsets=d_offs, stats=st)
        classify.append(st)
    classify = classify[args.warmup:]

    def submit(analyze):
        if analyze:
            return an.AnalyzeDeviceAsync(d_arena, R.offsets, R.path_ptrs, "/corpus", dev_offsets=d_offs)
        return sc.scan_device_async(d_arena, R.offsets, R.path_ptrs, binary=binary, transform=kinds, dev_offsets=d_offs)

    def block(analyze, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        inflight, st, fs = [], [], []

        def take(p):
            r = p.wait(False) if analyze else p.wait()
            st.append(r.stats())
            fs.append(r.fetch_stats())
        for _ in range(n):
            inflight.append(submit(analyze))
            if len(inflight) >= args.depth:
                take(inflight.pop(0))
        while inflight:
            take(inflight.pop(0))
        return time.perf_counter() - t0, st, fs

    for mode in (False, True):
        block(mode, args.warmup)
    per = {False: [], True: []}
    stats = {False: [], True: []}
    fetch = {False: [], True: []}
    done = 0
    while done < args.steps:
        n = min(args.block, args.steps - done)
        for mode in (False, True):
            s, st, fs = block(mode, n)
            per[mode].append(1e3 * s / n)
            stats[mode] += st
            fetch[mode] += fs
        done += n
    findings = {m: stats[m][-1]["findings"] for m in (False, True)}
    assert findings[False] == findings[True], findings

    def med(xs):
        return float(statistics.median(xs))

    n_files = int(R.n_files)
    bound = 320 * n_files + 8 * (n_files + 1)
    ms_k = med([c["ms_kernel"] for c in classify])
    out = {
        "tool": "device_only_bench --analyze", "gb": R.n_bytes / 1e9, "files": n_files, "steps": args.steps,
        "block": args.block, "depth": args.depth,
        "classify_kernel_ms": ms_k, "classify_call_ms": med([c["ms_total"] for c in classify]),
        "classify_traffic_bound_bytes": bound, "classify_bound_gbps": bound / 1e6 / ms_k if ms_k > 0 else 0.0,
        "kinds": [int((kinds == k).sum()) for k in range(4)], "binary": int(binary.sum()),
        "required": int(classify[-1]["required"]), "skipped_binary": int(classify[-1]["skipped_binary"]),
        "scan_device_ms_per_step": med(per[False]), "analyze_device_ms_per_step": med(per[True]),
        "scan_device_blocks_ms": per[False], "analyze_device_blocks_ms": per[True],
        "ms_gpu_total": med([s["ms_gpu_total"] for s in stats[True]]),
        "ms_xform_kernel": med([s["ms_xform_kernel"] for s in stats[True]]),
        "fetch_files_per_step": med([f["files"] for f in fetch[True]]),
        "fetch_bytes_per_step": med([f["bytes"] for f in fetch[True]]),
        "ms_fetch": med([f["ms_fetch"] for f in fetch[True]]),
        "candidates": int(stats[True][-1]["candidates"]), "findings": int(findings[True]),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


def resident_leg(args):
    import torch
    import trivy_amd.secret as secret
    from trivy_amd import corpus
    from trivy_amd.analyzer import SecretAnalyzer

    R = corpus.generate(int(args.gb * 1e9), seed=corpus.SEED, crlf_share=0.05)  # the bytes as read
    dev = torch.device("cuda", 0)
    d_arena = torch.from_numpy(R.arena).to(dev)
    d_offs = torch.from_numpy(R.offsets.view(np.int64)).to(dev)
    torch.cuda.synchronize()
    sc = secret.NewScanner(None, device=0, calibration=R.arena[:min(R.n_bytes, 16_000_000)])
    an = SecretAnalyzer(sc)
    if args.fetch == "windows":
        sc.set_fetch_mode("windows", back=args.back, fwd=args.fwd, fwd_cap=args.fwd_cap)
    modes = ("chunked", "split")

    def block(mode, n):
        sc.set_resident_transform(mode)  # (in force for the scans submitted from here on)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        inflight, res = [], []

        def take(p):
            r = p.wait(False)
            res.append({"stats": r.stats(), "fetch": r.fetch_stats(), "win": r.fetch_window_stats(),
                        "split": r.split_stats()})
        for _ in range(n):
            inflight.append(an.AnalyzeDeviceAsync(d_arena, R.offsets, R.path_ptrs, "/corpus", dev_offsets=d_offs))
            if len(inflight) >= args.depth:
                take(inflight.pop(0))
        while inflight:
            take(inflight.pop(0))
        return time.perf_counter() - t0, res

    for mode in modes:
        block(mode, args.warmup)
    per = {m: [] for m in modes}
    res = {m: [] for m in modes}
    done = 0
    while done < args.steps:
        n = min(args.block, args.steps - done)
        for mode in modes:
            s, r = block(mode, n)
            per[mode].append(1e3 * s / n)
            res[mode] += r
        done += n
    sc.set_resident_transform("chunked")
    findings = {m: res[m][-1]["stats"]["findings"] for m in modes}
    assert findings["chunked"] == findings["split"], findings
    assert all(r["split"]["mode_used"] == (m == "split") for m in modes for r in res[m])

    def med(xs):
        return float(statistics.median(xs))

    def of(m, group, key):
        return med([r[group][key] for r in res[m]])

    ms_census = of("split", "split", "ms_census")
    out = {
        "tool": "device_only_bench --analyze --resident split", "fetch": args.fetch, "gb": R.n_bytes / 1e9,
        "files": int(R.n_files), "steps": args.steps, "block": args.block, "depth": args.depth,
        "chunked_ms_per_step": med(per["chunked"]), "split_ms_per_step": med(per["split"]),
        "chunked_blocks_ms": per["chunked"], "split_blocks_ms": per["split"],
        "split_slowest_below_chunked_fastest": max(per["split"]) < min(per["chunked"]),
        "split_stats": {k: of("split", "split", k) for k in res["split"][-1]["split"]},
        "census_gbps": R.n_bytes / 1e6 / ms_census if ms_census > 0 else 0.0,
        "findings": int(findings["split"]),
    }
    for m in modes:
        out[m] = {
            "ms_gpu_total": of(m, "stats", "ms_gpu_total"), "ms_xform_kernel": of(m, "stats", "ms_xform_kernel"),
            "ms_host_exact": of(m, "stats", "ms_host_exact"), "candidates": int(res[m][-1]["stats"]["candidates"]),
            "fetch": {k: of(m, "fetch", k) for k in res[m][-1]["fetch"]},
            "window": {k: of(m, "win", k) for k in res[m][-1]["win"]},
        }
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


def pax_layer(layer):
    """The ustar layer rewritten as BuildKit writes layers: a PAX x header with path and mtime records
    before every entry.  One pass over the header chain (names without prefix, octal sizes)."""
    import numpy as np
    src = layer.tobytes()
    n = len(src)
    xh = bytearray(512)
    xh[:13] = b"PaxHeaders/x\0"
    xh[100:124] = b"0000644\x000000000\x000000000\x00"
    xh[136:148] = b"00000000000\x00"
    xh[156:157] = b"x"
    xh[257:265] = b"ustar\x0000"
    xh[148:156] = b" " * 8
    base = sum(xh)
    parts, p = [], 0
    while p + 512 <= n and src[p] != 0:
        size = int(src[p + 124:p + 135], 8)
        name = src[p:p + 100].split(b"\0", 1)[0]
        k = len(name) + 7  # " path=" + name + newline, and the digits of the length itself
        k += len(str(k + len(str(k))))
        rec = b"%d path=%s\n30 mtime=1700000000.123456789\n" % (k, name)
        f = b"%011o\x00" % len(rec)
        xh[124:136] = f
        xh[148:156] = b"%06o\x00 " % (base + sum(f))
        end = p + 512 + (size + 511) // 512 * 512
        parts += [bytes(xh), rec.ljust(512, b"\0"), src[p:end]]
        p = end
    parts.append(src[p:])
    return np.frombuffer(b"".join(parts), dtype=np.uint8)


def layer_leg(args):
    import torch
    import trivy_amd.secret as secret
    from trivy_amd import corpus
    from trivy_amd.analyzer import AnalyzerOptions, SecretAnalyzer
    from trivy_amd.analyzer.secret import Collector

    layer = corpus.generate_layer(int(args.layer_gb * 1e9), seed=corpus.SEED)
    if args.layer_format == "pax":
        layer = pax_layer(layer)
    n_bytes = int(layer.nbytes)
    dev = torch.device("cuda", 0)
    d_layer = torch.empty(n_bytes + 64, dtype=torch.uint8, device=dev)  # the 64 readable bytes after the layer
    d_layer[:n_bytes].copy_(torch.from_numpy(layer))
    d_layer[n_bytes:].zero_()
    torch.cuda.synchronize()
    an = SecretAnalyzer(device=0)
    an.Init(AnalyzerOptions())
    sc = an.scanner
    sc.set_resident_transform(args.resident)
    if args.fetch == "windows":
        sc.set_fetch_mode("windows", back=args.back, fwd=args.fwd, fwd_cap=args.fwd_cap)
    colls = [Collector(an, args.arena_mb << 20, True, gather=True) for _ in range(args.collectors)]
    unregister = secret.HostRegister(layer, mapped=True)  # registered once, outside the timed region
    walks = ("host", "gpu") if args.walk == "both" else (args.walk,)
    reqs = ("host", "gpu") if args.required == "both" else (args.required,)
    dev_modes = tuple(("device" if w == "host" else "device-gpu-walk") + ("-req" if r == "gpu" else "")
                      for w in walks for r in reqs if r == "host" or w == "gpu")
    if not dev_modes:
        raise SystemExit("--required gpu needs --walk gpu or both")
    modes = dev_modes if args.index_only else dev_modes + ("host",)
    walker = None
    if args.skip_dirs or args.skip_files:
        from trivy_amd.walker import NewLayerTar, Option
        walker = NewLayerTar(Option(SkipFiles=[p for p in args.skip_files.split(",") if p],
                                    SkipDirs=[p for p in args.skip_dirs.split(",") if p]))
        modes = tuple(m + v for m in modes for v in ("", "+skip"))
        if args.required_skip != "host":  # the switch on, beside (both) or instead of (gpu) the switch off
            modes = tuple(x for m in modes for x in (
                ((m, m + "@gpu") if args.required_skip == "both" else (m + "@gpu",))
                if m.endswith("-req+skip") else (m,)))

    def step(mode):
        skip_gpu = mode.endswith("@gpu")
        mode = mode[:-4] if skip_gpu else mode
        if skip_gpu or hasattr(an._L, "tsg_analyzer_set_tar_required_skip"):
            an.set_tar_required_skip("gpu" if skip_gpu else "host")
        if walker is not None:
            an.set_layer_walker(walker if mode.endswith("+skip") else None)
            mode = mode.split("+")[0]
        st = {}
        req = mode.endswith("-req")
        mode = mode[:-4] if req else mode
        if req or hasattr(an._L, "tsg_analyzer_set_tar_required"):
            an.set_tar_required("gpu" if req else "host")
        if mode != "host" and (mode == "device-gpu-walk" or hasattr(an._L, "tsg_analyzer_set_tar_walk")):
            an.set_tar_walk("gpu" if mode == "device-gpu-walk" else "host")
        if mode != "host" and args.index_only:
            ix = an.IndexDevice(d_layer, n_bytes, stats=st)
            st["walk"] = ix.walk_stats
            st["required_stats"] = ix.required_stats
            st["required_skip_stats"] = ix.required_skip_stats
            st["files"] = ix.n
        elif mode != "host":
            an.AnalyzeLayerDevice(d_layer, n_bytes, arena_bytes=args.arena_mb << 20, depth=args.depth, stats=st,
                                  materialize=False)
        else:
            an.AnalyzeLayer(layer, stats=st, materialize=False, colls=colls, registered=True)
        return st

    def block(mode, n):
        torch.cuda.synchronize()
        t0, c0 = time.perf_counter(), time.process_time()
        sts = [step(mode) for _ in range(n)]
        wall = time.perf_counter() - t0
        return wall, (time.process_time() - c0) / wall, sts

    try:
        for mode in modes:
            block(mode, args.warmup)
        per = {m: [] for m in modes}
        cpus = {m: [] for m in modes}
        res = {m: [] for m in modes}
        done = 0
        while done < args.steps:
            n = min(args.block, args.steps - done)
            for mode in modes:
                s, cpu, sts = block(mode, n)
                per[mode].append(1e3 * s / n)
                cpus[mode].append(cpu)
                res[mode] += sts
            done += n
    finally:
        unregister()
    if not args.index_only:
        findings = {m: res[m][-1]["scan_findings"] for m in modes}
        for v in ("", "+skip"):  # every mode finds the same, with the options and without
            assert len({f for m, f in findings.items() if ("+skip" in m) == bool(v)}) <= 1, findings

    def med(xs):
        return float(statistics.median(xs))

    claim = {m: max(per[m]) < min(per["host"]) for m in dev_modes} if not args.index_only else {}
    skip_keys = ("skipped_dirs", "skipped_files", "under_skipped_dir")
    for m in modes:
        last = res[m][-1]
        out = {"tool": "device_only_bench --layer", "mode": m, "fetch": args.fetch, "resident": args.resident,
               "format": args.layer_format, "index_only": args.index_only,
               "gb": n_bytes / 1e9, "steps": args.steps, "block": args.block, "depth": args.depth,
               "arena_mb": args.arena_mb, "ms_per_step": med(per[m]), "blocks_ms": per[m], "min_ms": min(per[m]),
               "max_ms": max(per[m]), "gbps": n_bytes / 1e6 / med(per[m]), "host_cpus": med(cpus[m])}
        if not args.index_only:
            out["findings"] = int(findings[m])
        if walker is not None:
            out["skip"] = {k: int(last.get(k, 0)) for k in skip_keys}
        if m.split("+")[0] != "host":
            if not args.index_only and m in claim:
                out["device_slowest_below_host_fastest"] = claim[m]
            keys = ("ms_kernel", "ms_total", "blocks", "candidates", "off_chain", "block_fetches", "ext_bytes",
                    "kernel_runs", "entries", "regular", "required", "files")
            out["index"] = {k: med([r[k] for r in res[m]]) for k in keys}
            out["index"]["ms_total_min"] = min(r["ms_total"] for r in res[m])
            out["index"]["ms_total_max"] = max(r["ms_total"] for r in res[m])
            out["index_kernel_gbps"] = n_bytes / 1e6 / out["index"]["ms_kernel"]
            out["walk"] = {k: med([r["walk"][k] for r in res[m]]) for k in last["walk"] if k != "walk"}
            if "required_stats" in last:
                out["required"] = {k: med([r["required_stats"][k] for r in res[m]]) for k in last["required_stats"]
                                   if k != "mode"}
                out["required"]["mode"] = last["required_stats"]["mode"]
            if "required_skip_stats" in last:
                out["required_skip"] = {k: med([r["required_skip_stats"][k] for r in res[m]])
                                        for k in last["required_skip_stats"] if k != "mode"}
                out["required_skip"]["mode"] = last["required_skip_stats"]["mode"]
        else:
            out["walk_s"] = med([r["walk_s"] for r in res[m]])
            out["wait_s"] = med([r["wait_s"] for r in res[m]])
            out["added"] = int(last["added"])
        out["scan"] = {k[5:]: med([r[k] for r in res[m]]) for k in last if k.startswith("scan_")}
        line = json.dumps(out)
        print(line)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


def layers_leg(args):
    """--layers: interleaved blocks of the batched calls and the loops they replace, on one image in one process."""
    import torch
    import trivy_amd.secret as secret
    from trivy_amd import corpus
    from trivy_amd.analyzer import AnalyzerOptions, SecretAnalyzer

    if args.layers == 5:
        w = [0.34, 0.26, 0.20, 0.12, 0.08]
        layers = [corpus.generate_layer(int(args.layer_gb * 1e9 * x), seed=corpus.SEED + 1000 * k) for k, x in enumerate(w)]
    else:
        layers = [corpus.generate_layer(int(args.layer_mb * 1e6), seed=corpus.SEED + 1000 * k) for k in range(args.layers)]
    sizes = [int(ly.nbytes) for ly in layers]
    assert all(n % 512 == 0 for n in sizes)
    total = sum(sizes)
    dev = torch.device("cuda", 0)
    d_image = torch.empty(total + 64, dtype=torch.uint8, device=dev)  # the layers back to back, as in a saved image
    at, slices = 0, []
    for ly, n in zip(layers, sizes):
        d_image[at:at + n].copy_(torch.from_numpy(ly))
        slices.append((d_image[at:at + n + 64], n))
        at += n
    d_image[total:].zero_()
    torch.cuda.synchronize()
    an = SecretAnalyzer(device=0)
    an.Init(AnalyzerOptions())
    sc = an.scanner
    sc.set_resident_transform(args.resident)
    if args.fetch == "windows":
        sc.set_fetch_mode("windows", back=args.back, fwd=args.fwd, fwd_cap=args.fwd_cap)
    an.set_tar_walk("gpu")
    reqs = ("", "-req") if args.required == "both" else ("-req",) if args.required == "gpu" else ("",)
    modes = tuple(m + r for m in ("batched", "loop") for r in reqs) + (() if args.index_only else ("host",))
    if args.skip_dirs or args.skip_files:  # the options hold for every mode of this leg
        from trivy_amd.walker import NewLayerTar, Option
        an.set_layer_walker(NewLayerTar(Option(SkipFiles=[p for p in args.skip_files.split(",") if p],
                                               SkipDirs=[p for p in args.skip_dirs.split(",") if p])))
        if args.required_skip != "host":
            modes = tuple(x for m in modes for x in (
                ((m, m + "@gpu") if args.required_skip == "both" else (m + "@gpu",)) if m.endswith("-req") else (m,)))
    unregister = []
    workers = None
    if "host" in modes:
        unregister = [secret.HostRegister(ly, mapped=True) for ly in layers]  # once, outside the timed region
        workers = an.LayerWorkers(3, args.arena_mb << 20, args.collectors, gather=True)
    arena = args.arena_mb << 20

    def step(mode):
        st = {"findings": 0}
        skip_gpu = mode.endswith("@gpu")
        mode = mode[:-4] if skip_gpu else mode
        if skip_gpu or hasattr(an._L, "tsg_analyzer_set_tar_required_skip"):
            an.set_tar_required_skip("gpu" if skip_gpu else "host")
        req = mode.endswith("-req")
        mode = mode[:-4] if req else mode
        if req or hasattr(an._L, "tsg_analyzer_set_tar_required"):
            an.set_tar_required("gpu" if req else "host")

        def required_of(ixs):  # the layers' counts summed; the stage and its copies are one per pass
            rs = [ix.required_stats for ix in ixs]
            out = {k: sum(r[k] for r in rs) for k in ("entries", "kept", "dropped", "ask_allow", "ask_name",
                                                      "ask_dropped", "path_bytes")}
            shared = mode == "batched"
            for k in ("ms_kernel", "ms_copy"):
                out[k] = max(r[k] for r in rs) if shared else sum(r[k] for r in rs)
            out["ms_host_sum"] = sum(r["ms_host"] for r in rs)
            out["on_gpu_layers"] = sum(r["mode"] == "gpu" for r in rs)
            ss = [ix.required_skip_stats for ix in ixs]
            for k in ("skipped_dirs", "skipped_files", "under_skipped_dir"):
                out[k] = sum(x[k] for x in ss)
            out["skip_on_gpu_layers"] = sum(x["reason"] == 0 for x in ss)
            out["skip_table_slots"] = max(x["table_slots"] for x in ss)
            out["skip_ms_kernel"] = max(x["ms_kernel"] for x in ss) if shared else sum(x["ms_kernel"] for x in ss)
            return out
        if mode == "batched" and args.index_only:
            stats = []
            st["required"] = required_of(an.IndexLayersDevice(slices, stats=stats))
            st["forest"] = stats[-1]
        elif mode == "loop" and args.index_only:
            per, ixs = [], []
            for t, n in slices:
                ix = an.IndexDevice(t, n)
                per.append(ix.walk_stats)
                ixs.append(ix)
            st["required"] = required_of(ixs)
            st["stages"] = {k: sum(w[k] for w in per) for k in per[0] if k.startswith("ms_")}
            st["device_bytes"] = sum(w["device_bytes"] for w in per)  # allocated and freed over the image
        elif mode == "batched":
            stats = []
            an.AnalyzeLayersDevice(slices, arena_bytes=arena, depth=args.depth, group_bytes=args.group_mb << 20,
                                   materialize=False, stats=stats)
            st["forest"] = stats[-1]
            st["findings"] = sum(d.get("scan_findings", 0) for d in stats[:-1])
        elif mode == "loop":
            for t, n in slices:
                d = {}
                an.AnalyzeLayerDevice(t, n, arena_bytes=arena, depth=args.depth, stats=d, materialize=False)
                st["findings"] += d.get("scan_findings", 0)
        else:
            stats = []
            an.AnalyzeLayers(layers, materialize=False, stats=stats, workers=workers, registered=True)
            st["findings"] = sum(d.get("scan_findings", 0) for d in stats)
        return st

    def block(mode, n):
        torch.cuda.synchronize()
        t0, c0 = time.perf_counter(), time.process_time()
        sts = [step(mode) for _ in range(n)]
        wall = time.perf_counter() - t0
        return wall, (time.process_time() - c0) / wall, sts

    try:
        for mode in modes:
            block(mode, args.warmup)
        per = {m: [] for m in modes}
        cpus = {m: [] for m in modes}
        res = {m: [] for m in modes}
        done = 0
        while done < args.steps:
            n = min(args.block, args.steps - done)
            for mode in modes:
                s, cpu, sts = block(mode, n)
                per[mode].append(1e3 * s / n)
                cpus[mode].append(cpu)
                res[mode] += sts
            done += n
    finally:
        for u in unregister:
            u()

    def med(xs):
        return float(statistics.median(xs))
    findings = {m: int(res[m][-1]["findings"]) for m in modes}
    if not args.index_only:
        assert len(set(findings.values())) == 1, findings
    for m in modes:
        out = {"tool": "device_only_bench --layers", "mode": m, "index_only": args.index_only, "layers": len(layers),
               "gb": total / 1e9, "layer_bytes": sizes if len(sizes) <= 8 else [sizes[0], "...", sizes[-1]],
               "steps": args.steps, "block": args.block, "depth": args.depth, "arena_mb": args.arena_mb,
               "group_mb": args.group_mb, "fetch": args.fetch, "resident": args.resident,
               "ms_per_step": med(per[m]), "blocks_ms": per[m], "min_ms": min(per[m]), "max_ms": max(per[m]),
               "gbps": total / 1e6 / med(per[m]), "host_cpus": med(cpus[m]), "findings": findings[m]}
        if "required" in res[m][-1]:
            out["required"] = {k: med([r["required"][k] for r in res[m]]) for k in res[m][-1]["required"]}
        if m.startswith("batched"):
            loop = "loop" + m[len("batched"):]
            out["batched_slowest_below_loop_fastest"] = max(per[m]) < min(per[loop])
            out["forest"] = {k: med([r["forest"][k] for r in res[m]]) for k in res[m][-1]["forest"]}
            if not args.index_only:  # the share of the index time that ran beside scans
                f = out["forest"]
                hidden = f["index_s"] + f["scan_s"] - f["wall_s"]
                out["index_hidden_share"] = max(0.0, min(1.0, hidden / f["index_s"])) if f["index_s"] > 0 else 0.0
        if m.startswith("loop") and args.index_only:
            out["stages"] = {k: med([r["stages"][k] for r in res[m]]) for k in res[m][-1]["stages"]}
            out["device_bytes_allocated"] = med([r["device_bytes"] for r in res[m]])
        line = json.dumps(out)
        print(line)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
