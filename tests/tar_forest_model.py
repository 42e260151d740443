"""A pure-Python model of the forest pass over all layers of an image (trivy_amd/csrc/tarforest.h,
tarforest.hip; tsg_analyzer_index_device_tars in tar-walk mode "gpu"): tests/tar_chain_model.chain applied to
every layer on its own, plus what the pass adds -- a head per layer and where each layer's records and names
begin in the two shared buffers.

A layer is (data, n): the pass may read the complete 512-B blocks below n; `data` may be longer (a slice of
one buffer: what follows the layer in memory), and the model, like the pass, decides from the bytes below n.
"""
import struct

from tests import tar_chain_model as cm

HEAD = struct.Struct("<IIQQQQQQQ")  # TarChainHead: kind, reason, offset, ext, steps, entries, name_bytes, candidates, 0
assert HEAD.size == 64


def layer(data: bytes, n=None):
    """One layer's part: (the entries handed over, the stop, the candidate count)."""
    n = len(data) if n is None else n
    entries, stop, n_cand = cm.chain(data, n)
    want = cm.strip_next(entries) if stop[0] == cm.END else []  # nothing is handed over for an INCOMPLETE stop
    return want, stop, n_cand


def forest(parts):
    """parts: layer() results, in order.  -> (heads as (kind, reason, offset, ext, entries, name_bytes,
    candidates), record bases, name bases, total records, total name bytes)."""
    heads, rec_base, name_base = [], [], []
    r = nb = 0
    for want, stop, n_cand in parts:
        names = sum(len(e["name"]) for e in want)
        heads.append((stop[0], stop[1], stop[2], stop[3], len(want), names, n_cand))
        rec_base.append(r)
        name_base.append(nb)
        r += len(want)
        nb += names
    return heads, rec_base, name_base, r, nb


def virtual_blocks(sizes, S):
    """The virtual block space: V_k per layer and the total (tarforest.h)."""
    v, out = 0, []
    for n in sizes:
        out.append(v)
        v += (max(n // 512, 1) + S - 1) // S * S
    return out, v
