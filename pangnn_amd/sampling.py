"""A fresh random subset of the similarity edges per step: sub_sample_graph_edges of the reference (src/helper.py:16-68, an
older copy at src/dataset.py:398-446), which pangnn.py:190 means to call on the whole training graph at every step,

    batch = sub_sample_graph_edges(dataset.train, device, fraction = 0.8) if not args.union_edge_weights else dataset.train

and which is commented out there because the function cannot run: it hands `random.sample` a list of 0-d tensors, needs
`graph.union_edge_index` in the mode that has none, and goes through the CPU.  So the semantics are BUILD-DEFINED here
(DESIGN.md §2), after the function's evident intent — negative down-sampling that leaves the homolog structure intact:

  * exactly  k = int(E * (1 - fraction))  edges are removed, E' = E - k stay, in the caller's order;
  * sample_pos_edges=False (the default): the k edges are drawn uniformly without replacement from the negatives
    (y == 0) and every positive stays.  The reference's assertion is a ValueError here: when the positive share exceeds
    `fraction`, and when there are fewer than k negatives;
  * sample_pos_edges=True: the k edges are drawn uniformly without replacement from all edges;
  * the draw is made on the graph's device from `generator` (the device's default generator without one): the same seed
    gives the same subset;
  * x and neighbour_edge_index are shared with the parent; edge_index, edge_attr and y are compacted; `kept_edge_id`
    (int64 [E'], ascending) names the parent edge of every child edge, so per-edge results map back: out[kept_edge_id];
  * a graph with `union_edge_index` raises ValueError (the call site excludes --union_edge_weights).

On the device the child's `EdgeStructure` — both CSR orders the decoder and the propagates read — is DERIVED from the
parent's by an order-preserving compaction (EdgeStructure.filtered, csrc/edge_filter.hip) instead of two radix sorts of
the new edge list, and is placed where the model looks for it; the parent's positional-neighbour structure is carried
over.  The first call on a parent builds both of the parent's orders (its only sorts) and reads its negative count; after
that a call makes no device -> host synchronisation and the step on the child sorts nothing.
CPU tensors take a plain-torch path with the same definition and no structure.

Lifetime: the child's tables live in the child's structure, which the identity-keyed caches (graph._CACHE, the native
registry of csrc/graph_ops.cpp) also hold.  `release(child)` drops those entries; it also runs when the child `Data` is
garbage-collected, so `batch = sub_sample_graph_edges(...)` in a loop does not accumulate memory.
"""
from __future__ import annotations

import os
import weakref
from typing import Optional

import torch

from . import _lib
from . import graph as _G
from .data import Data

# the device draw marks the k smallest keys with a selection kernel (mask_k_smallest); False: torch.topk, for A/B
MASK_KERNEL = os.environ.get("PANGNN_MASK_KERNEL", "1") != "0"


def _num_nodes(graph) -> int:
    x = getattr(graph, "x", None)
    return int(x.shape[0]) if x is not None else int(graph.num_nodes)


def _check_graph(graph):
    if getattr(graph, "union_edge_index", None) is not None:
        raise ValueError("a graph with union_edge_index (--union_edge_weights) is not sub-sampled: pangnn.py:190 trains "
                         "on the whole union graph")
    ei = graph.edge_index
    if ei.dim() != 2 or ei.shape[0] != 2:
        raise ValueError(f"edge_index must be [2, E], got {tuple(ei.shape)}")
    return ei


def _drop(key, edge_index):
    _G.forget(key, edge_index)


def release(child) -> None:
    """Drop what the caches hold of a graph made by filter_edges / sub_sample_graph_edges (its structure's entry in the
    identity cache and in the native registry), so that its tables are freed with the last reference to the graph.
    Idempotent; also runs when the graph is garbage-collected."""
    fin = child.__dict__.get("_pangnn_release")
    if fin is not None:
        fin()
    child.__dict__.pop("_pangnn_structs", None)


def _per_edge_f32(t: Optional[torch.Tensor], e: int):
    """edge_attr / y as the kernel compacts them alongside (a float32 [E] vector), None for an absent one, False for
    anything else (gathered by kept_edge_id in plain torch)"""
    if t is None:
        return None
    if t.dtype != torch.float32 or t.dim() != 1 or t.shape[0] != e:
        return False
    return t.detach().contiguous()


def filter_edges(graph, keep: torch.Tensor, num_kept: Optional[int] = None) -> Data:
    """The graph of the edges with keep[e] != 0: a `Data` whose x and neighbour_edge_index are the parent's tensors, whose
    edge_index / edge_attr / y hold the kept edges in the caller's order, plus `kept_edge_id` (int64 [E']).  The parent is
    not modified.  Device tensors: the child's structure is derived from the parent's (module docstring) and found by
    `structure_of(child.edge_index, N, holder=child, name="sim")` and, by identity, by the dispatcher ops; `num_kept`
    (the number of kept edges, where the caller knows it) spares the one device -> host read of the count; a wrong one
    writes nothing out of bounds and is reported by the structure's `check_filter()` (one read) when the caller asks."""
    ei = _check_graph(graph)
    e, n = ei.shape[1], _num_nodes(graph)
    keep = keep.detach().reshape(-1)
    if keep.numel() != e:
        raise ValueError(f"{keep.numel()} keep entries for {e} edges")
    child = Data(x=getattr(graph, "x", None))
    for k, v in graph.__dict__.items():                       # everything that is not per similarity edge is shared
        if not k.startswith("_") and k not in ("x", "edge_index", "edge_attr", "y", "kept_edge_id"):
            child.__dict__[k] = v
    attr, y = getattr(graph, "edge_attr", None), getattr(graph, "y", None)
    if not ei.is_cuda:
        idx = torch.nonzero(keep != 0).view(-1)
        child.edge_index = ei[:, idx].contiguous()
        child.edge_attr = None if attr is None else attr[idx]
        child.y = None if y is None else y[idx]
        child.kept_edge_id = idx
        return child
    parent = _G.structure_of(ei, n, holder=graph, name="sim")
    # filtered() derives the orders its parent holds: ask for both once per parent (a graph that is only ever sub-sampled,
    # like dataset.train in the reference's loop, is never stepped on itself and would otherwise never get its by-source
    # order, leaving every child to sort for it)
    parent.by_dst, parent.by_src
    a32, y32 = _per_edge_f32(attr, e), _per_edge_f32(y, e)
    fused = [t for t in (a32, y32) if t is not None and t is not False]
    st, kept_id, outs = _G.EdgeStructure.filtered(parent, keep, num_kept, fused)
    outs = list(outs)
    child.edge_index = st.edge_index
    child.kept_edge_id = kept_id.long()
    for name, src, t32 in (("edge_attr", attr, a32), ("y", y, y32)):
        if src is None:
            val = None
        elif t32 is False:                                    # not a float32 [E] vector: a plain gather
            val = src[child.kept_edge_id]
        else:
            val = outs.pop(0)
        setattr(child, name, val)
    key = _G.structure_key(st.edge_index, n)
    structs = {"sim": (key, st)}
    nb = getattr(graph, "neighbour_edge_index", None)
    if nb is not None:
        nb_st = _G.structure_of(nb, n, holder=graph, name="nb")      # the parent's band structure: shared, not rebuilt
        structs["nb"] = (_G.structure_key(nb, n), nb_st)
    child._pangnn_structs = structs
    _G.register(st, key)
    child._pangnn_release = weakref.finalize(child, _drop, key, st.edge_index)
    return child


def _negatives(graph, y: torch.Tensor) -> int:
    """number of negatives (y == 0) of the parent, counted once per graph and label tensor (one device -> host read) and
    cached on it"""
    key = (y.data_ptr(), y._version, tuple(y.shape))
    hit = graph.__dict__.get("_pangnn_negatives") if hasattr(graph, "__dict__") else None
    if hit is None or hit[0] != key:
        hit = (key, int((y.reshape(-1) == 0).sum()), y)       # (keeps y alive: the key is its address)
        try:
            graph._pangnn_negatives = hit
        except Exception:
            pass
    return hit[1]


def mask_k_smallest(keys: torch.Tensor, k: int) -> torch.Tensor:
    """keep bool [n] for device keys int64 [n], 0 <= key < 2^63: False for exactly the k entries that come first in
    (key, index) order, True elsewhere (pangnn_mask_k_smallest_i64, csrc/mask_select.hip: a radix select, no sort, nothing
    read back; `keys` is only read).  With distinct keys: the complement of torch.topk(keys, k, largest=False)."""
    _lib.require_device(keys)
    if keys.dtype != torch.int64 or keys.dim() != 1:
        raise ValueError(f"keys must be int64 [n], got {keys.dtype} {tuple(keys.shape)}")
    n, k = keys.shape[0], int(k)
    if not 0 <= k <= n:
        raise ValueError(f"k = {k} of {n} keys")
    keys = keys if keys.is_contiguous() and keys.data_ptr() % 16 == 0 else keys.clone(memory_format=torch.contiguous_format)
    lib = _lib.load()
    keep = torch.empty(n, dtype=torch.uint8, device=keys.device)
    if n:
        with _lib.device_guard(keys.device):
            ws_bytes = lib.pangnn_mask_k_smallest_workspace_bytes(n)
            if ws_bytes == 0:
                raise _lib.PangnnHipError("pangnn_mask_k_smallest_workspace_bytes failed")
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=keys.device)
            _lib.check(lib.pangnn_mask_k_smallest_i64(keys.data_ptr(), n, k, keep.data_ptr(), ws.data_ptr(), ws_bytes,
                                                      _lib.stream_ptr()), "pangnn_mask_k_smallest_i64")
    return keep.view(torch.bool)


def draw_keep_mask(graph, fraction: float = 0.8, sample_pos_edges: bool = False, generator=None):
    """(keep bool [E], E') of sub_sample_graph_edges: exactly int(E * (1 - fraction)) entries False, drawn uniformly without
    replacement from the negatives (or from all edges) on the graph's device.  One 62-bit random key per edge, a
    positive's key replaced by a larger constant, the k smallest keys lose (ties between keys are 2^-62 events, so the
    subset is a function of the seed; nothing of size E is kept between calls).  On the device the k smallest are marked
    by a selection kernel (mask_k_smallest; MASK_KERNEL = False: torch.topk and an indexed store, the same mask); CPU
    tensors take the torch route."""
    ei = _check_graph(graph)
    e, dev = ei.shape[1], ei.device
    if not 0.0 <= fraction <= 1.0:
        raise ValueError(f"fraction = {fraction}")
    k = int(e * (1 - fraction))
    y = None
    if not sample_pos_edges:
        y = getattr(graph, "y", None)
        if y is None or y.reshape(-1).shape[0] != e:
            raise ValueError("sample_pos_edges=False needs the labels graph.y [E]")
        pool = _negatives(graph, y)
        if e and (e - pool) / e > fraction:
            raise ValueError(f"cannot keep {fraction} of the edges with every positive: {(e - pool) / e:.4f} of them are "
                             f"positive — lower the positive share, lower `fraction`, or pass sample_pos_edges=True")
        if pool < k:
            raise ValueError(f"{k} edges to remove but only {pool} negatives")
    if k == 0:
        return torch.ones(e, dtype=torch.bool, device=dev), e
    keys = torch.empty(e, dtype=torch.int64, device=dev).random_(0, 1 << 62, generator=generator)
    if y is not None:
        keys.masked_fill_(y.reshape(-1) != 0, 1 << 62)        # k <= the number of negatives: never among the k smallest
    if MASK_KERNEL and keys.is_cuda:
        return mask_k_smallest(keys, k), e - k
    keep = torch.ones(e, dtype=torch.bool, device=dev)
    keep[torch.topk(keys, k, largest=False, sorted=False).indices] = False
    return keep, e - k


def sub_sample_graph_edges(graph, device=None, fraction: float = 0.8, sample_pos_edges: bool = False, generator=None) -> Data:
    """The reference's sub_sample_graph_edges(graph, device, fraction, sample_pos_edges) (module docstring for the
    semantics): a `Data` with E - int(E * (1 - fraction)) of the similarity edges.  The draw and the compaction run where
    `graph` lives; `device`, if given and another one, moves the result there (`Data.to`: the derived structure stays
    behind, as for any moved graph)."""
    keep, kept = draw_keep_mask(graph, fraction, sample_pos_edges, generator)
    child = filter_edges(graph, keep, num_kept=kept)
    want, have = (None if device is None else torch.device(device)), child.edge_index.device
    if want is not None and (want.type != have.type or (want.index is not None and want.index != have.index)):
        moved = child.to(want)
        release(child)
        return moved
    return child
