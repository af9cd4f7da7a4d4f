"""Max-candidate labelling: the "best hit per genome" baselines of predict_homolog_genes (src/predict.py:83-90).

The reference computes them as Python dict loops over every edge: calculate_baseline_labels (src/helper.py:437-485, called
at src/dataset.py:390) over the Q-scores and the raw scores, calculate_logit_baseline_labels (src/helper.py:494-576) over the
logits.  For a relation of edges e = (src[e], dst[e]) with values v[e]:

    candidates(e) = { e' : src[e'] == src[e] and genome_of[dst[e']] == genome_of[dst[e]] }     (e itself included)
    label[e]      = 1  iff  no e' in candidates(e) has v[e] < v[e']

i.e. label = isnan(v) | (v >= max of the segment's non-NaN values): ties are all 1, a NaN value is 1, a NaN candidate beats
nobody.  The segments are the (source, candidate genome) groups of construct.normalize_sim_scores, key = src * G +
genome_of[dst].  `genome_of` is exact genome equality where the reference tests `startswith(genome prefix)`; on the bundled
data every prefix has 8 letters and simulated ids have equal length, so the two agree there.

Device tensors run on one HIP pass (pangnn_best_candidate_f32 / _f64, csrc/candidates.hip) over a segment structure that is
built once per (edge_index, genome_of) and cached; CPU tensors run the same definition in plain torch (scatter_reduce amax).
"""
from __future__ import annotations

import weakref
from types import SimpleNamespace
from typing import Optional

import torch

from . import _lib


def _num_genomes(genome_of: torch.Tensor) -> int:
    return int(genome_of.max().item()) + 1 if genome_of.numel() else 1


def _key(edge_index: torch.Tensor, genome_of: torch.Tensor) -> torch.Tensor:
    src, dst = edge_index[0].to(torch.int64), edge_index[1].to(torch.int64)
    genome_of = genome_of.to(src.device)
    return src * _num_genomes(genome_of) + genome_of[dst].to(torch.int64)


def build_segments(edge_index: torch.Tensor, genome_of: torch.Tensor) -> SimpleNamespace:
    """(seg_rowptr int64 [S+1], seg_edge int32 [E] or None, num_segments) of the (source, candidate genome) groups.
    When the key is already non-decreasing (simulated graphs in canonical order) the edge order IS the segment order and
    seg_edge is None; otherwise the edges are sorted by key (stable).  The structure lives on the device of edge_index;
    genome_of may live anywhere."""
    key = _key(edge_index, genome_of)
    e = key.numel()
    seg_edge = None
    if e > 1 and not bool((key[1:] >= key[:-1]).all()):
        order = torch.argsort(key, stable=True)
        key = key[order]
        seg_edge = order.to(torch.int32)
    if e:
        first = torch.ones(e, dtype=torch.bool, device=key.device)
        first[1:] = key[1:] != key[:-1]
        seg_rowptr = torch.cat([torch.nonzero(first).view(-1),
                                torch.full((1,), e, dtype=torch.int64, device=key.device)])
    else:
        seg_rowptr = torch.zeros(1, dtype=torch.int64, device=key.device)
    return SimpleNamespace(seg_rowptr=seg_rowptr, seg_edge=seg_edge, num_segments=seg_rowptr.numel() - 1, num_edges=e)


class _SegmentCache:
    """the last few segment structures, keyed on the identity and version of the caller's (edge_index, genome_of) — so a
    host genome_of keeps hitting the same entry; an entry goes when either tensor is gone"""

    def __init__(self, size: int = 4):
        self.size, self.entries = size, []

    def get(self, edge_index, genome_of):
        self.entries = [x for x in self.entries if x[0]() is not None and x[1]() is not None]     # the graph is gone
        for i, (ei, go, ver, seg) in enumerate(self.entries):
            if ei() is edge_index and go() is genome_of and ver == (edge_index._version, genome_of._version):
                self.entries.insert(0, self.entries.pop(i))
                return seg
        seg = build_segments(edge_index, genome_of)
        self.entries.insert(0, (weakref.ref(edge_index), weakref.ref(genome_of),
                                (edge_index._version, genome_of._version), seg))
        del self.entries[self.size:]
        return seg

    def clear(self):
        self.entries = []


SEGMENTS = _SegmentCache()


def _values(values: torch.Tensor) -> torch.Tensor:
    v = values.detach().reshape(-1)
    if v.dtype in (torch.float16, torch.bfloat16):
        v = v.to(torch.float32)                         # exact: every f16 / bf16 value is an f32 value
    elif v.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"best_candidate: values must be float32 / float64 (float16 / bfloat16 are upcast), got {v.dtype}")
    return v.contiguous()


def _label_on_device(v, seg, y, counts) -> torch.Tensor:
    lib = _lib.load()
    label = torch.empty(v.numel(), dtype=torch.uint8, device=v.device)
    yv = None
    if y is not None:
        yv = y.detach().reshape(-1).to(torch.float32).contiguous()
        if yv.numel() != v.numel():
            raise ValueError(f"{yv.numel()} labels for {v.numel()} values")
        if counts.dtype != torch.int64 or counts.numel() != 4 or not counts.is_contiguous():
            raise ValueError("counts must be a contiguous int64 [4] device tensor")
    name = "pangnn_best_candidate_f64" if v.dtype == torch.float64 else "pangnn_best_candidate_f32"
    with _lib.device_guard(v.device):
        _lib.check(getattr(lib, name)(seg.seg_rowptr.data_ptr(), _lib.ptr(seg.seg_edge), seg.num_segments, seg.num_edges,
                                      v.data_ptr(), _lib.ptr(yv), _lib.ptr(counts), label.data_ptr(), _lib.stream_ptr()),
                   name)
    return label.view(torch.bool)


def _best_candidate_cpu(v, edge_index, genome_of):
    key = _key(edge_index, genome_of)
    _, inv = torch.unique(key, return_inverse=True)
    nseg = int(inv.max().item()) + 1 if inv.numel() else 0
    finite = torch.where(torch.isnan(v), torch.full_like(v, -float("inf")), v)
    mx = torch.full((nseg,), -float("inf"), dtype=v.dtype).scatter_reduce(0, inv, finite, reduce="amax",
                                                                        include_self=True)
    return torch.isnan(v) | (v >= mx[inv])


def best_candidate(values: torch.Tensor, edge_index: torch.Tensor, genome_of: torch.Tensor,
                   y: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bool[E]: edge e is a best candidate of its (source, genome(target)) segment (module docstring).

    values: [E] float32 / float64 (float16 / bfloat16 are upcast to float32, other dtypes refused); edge_index [2, E];
    genome_of [N] (integer genome id of every node, on any device).  On the GPU, `y` [E] (0 / 1) with `counts` (int64 [4] on the device, [tn, fp, fn, tp] as
    metrics.BinaryConfusionMatrix keeps them) adds the confusion counts of the labels against y in the same pass."""
    v = _values(values)
    if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.shape[1] != v.numel():
        raise ValueError(f"edge_index {tuple(edge_index.shape)} does not match {v.numel()} values")
    if (y is None) != (counts is None):
        raise ValueError("y and counts go together")
    if not v.is_cuda:
        if y is not None:
            raise ValueError("fused confusion counts need device tensors")
        return _best_candidate_cpu(v, edge_index, genome_of)
    _lib.require_device(edge_index, y, counts)
    return _label_on_device(v, SEGMENTS.get(edge_index, genome_of), y, counts)


def candidate_baselines(edge_index: torch.Tensor, edge_attr: torch.Tensor, genome_of: torch.Tensor,
                        raw_src: Optional[torch.Tensor] = None, raw_dst: Optional[torch.Tensor] = None,
                        raw_score: Optional[torch.Tensor] = None):
    """(q_labels, raw_labels): dataset.base_labels, dataset.base_labels_raw of the reference (src/dataset.py:390).

    q_labels: max-candidate labels of the graph's own edges over their normalised weights `edge_attr`.
    raw_labels: labels of the RAW relation (raw_src, raw_dst, raw_score) — self hits included, so a within-genome paralog
    edge competes with its source's self hit — read back at the graph's edges by their (src, dst) key; None when no raw
    relation is given.  Trivial-case removal drops whole single-candidate segments, so the raw relation may be passed
    before or after it: the labels at the graph's edges are the same.  Raw pairs with a negative node id (a gene absent
    from the annotations) are ignored.  Every graph edge must be a pair of the raw relation."""
    q = best_candidate(edge_attr, edge_index, genome_of)
    if raw_src is None:
        return q, None
    s, d = raw_src.to(torch.int64), raw_dst.to(torch.int64)
    ok = (s >= 0) & (d >= 0)
    s, d, sc = s[ok], d[ok], raw_score[ok]
    raw_ei = torch.stack([s, d])
    if sc.is_cuda:                                      # a one-off relation: not cached
        _lib.require_device(raw_ei)
        raw = _label_on_device(_values(sc), build_segments(raw_ei, genome_of), None, None)
    else:
        raw = best_candidate(sc, raw_ei, genome_of)
    n = max(int(genome_of.numel()), 1)
    rk = s * n + d
    rk, order = torch.sort(rk)
    gk = edge_index[0].to(torch.int64) * n + edge_index[1].to(torch.int64)
    pos = torch.searchsorted(rk, gk).clamp_(max=max(rk.numel() - 1, 0))
    if gk.numel() and (rk.numel() == 0 or not bool((rk[pos] == gk).all())):
        raise ValueError("an edge of the graph is not a pair of the raw relation")
    return q, raw[order[pos]]
