"""Graph construction on integer COO arrays (runs on the device of its inputs: sort / unique / searchsorted programs
plus, on the GPU, the segmented softmax -> Q-score HIP kernel of csrc/edge_ops.hip).

Restates the host pipeline the reference runs as nested Python dict loops
(/root/reference/src/preprocessing.py:73-156,264-325,370-385,454-548; src/dataset.py:325-384) as
sort + segment reductions, so the 50k x 20 and larger simulated graphs — which the reference cannot
construct in practical time — build in seconds.  Checked against fixtures generated
by the reference's own code: edge_index / neighbour_edge_index / labels bit-exact, weights to fp32
rounding (tests/test_construct.py).

Relation encoding: the reference's {gene: {gene: score}} dict is a COO triple (src, dst, score);
`genome_of[node]` replaces the `id.split('_')[0]` genome prefix; `group_of[node]` (ortholog group
id, -1 = none) replaces the RIBAP dictionaries.  Edge order: the reference's order is an accident of
CPython set iteration (helper.py:428-431); the canonical order here is (src, dst) lexicographic.
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Optional

import torch


def _segments(key: torch.Tensor):
    """ids of equal-key runs (any order of `key`), and the run count per id"""
    uniq, inv, cnt = torch.unique(key, return_inverse=True, return_counts=True)
    return inv, cnt


def remove_trivial_cases(src, dst, score, genome_of):
    """preprocessing.py:370-385: per source gene keep only candidates whose genome holds more than
    one candidate of that source (self hits count)."""
    g = int(genome_of.max().item()) + 1 if genome_of.numel() else 1
    key = src * g + genome_of[dst].to(src.dtype)
    inv, cnt = _segments(key)
    keep = cnt[inv] > 1
    return src[keep], dst[keep], score[keep]


def normalize_sim_scores(src, dst, score, genome_of, t: float = 0.8, epsilon: float = 1e-8,
                         pseudo_count: float = 1.0):
    """preprocessing.py:454-548: per (source, candidate genome) group without self hits,
    p = softmax(score / t) (single candidate: p = 1), w = -10 log10(clip(1-p, eps, 1-eps)) + pseudo.
    float64 like the reference's numpy; returns (src, dst, w float64)."""
    ns = src != dst
    src, dst, score = src[ns], dst[ns], score[ns]
    g = int(genome_of.max().item()) + 1 if genome_of.numel() else 1
    key = src * g + genome_of[dst].to(src.dtype)
    if src.is_cuda:
        # device tensors: one segmented HIP pass over the key-sorted relation (pangnn_softmax_qscore_f64)
        from . import _lib
        lib = _lib.load()
        order = torch.argsort(key, stable=True)
        src, dst, key = src[order], dst[order], key[order]
        sc = score[order].to(torch.float64).contiguous()
        _, cnt = torch.unique_consecutive(key, return_counts=True)
        rowptr = torch.zeros(cnt.numel() + 1, dtype=torch.int64, device=src.device)
        torch.cumsum(cnt, 0, out=rowptr[1:])
        q = torch.empty_like(sc)
        with torch.cuda.device(src.device):
            _lib.check(lib.pangnn_softmax_qscore_f64(rowptr.data_ptr(), sc.data_ptr(), int(cnt.numel()), int(sc.numel()),
                                                     float(t), float(epsilon), float(pseudo_count), q.data_ptr(),
                                                     _lib.stream_ptr()), "pangnn_softmax_qscore_f64")
        return src, dst, q
    inv, cnt = _segments(key)
    x = score.to(torch.float64) / t
    nseg = cnt.numel()
    mx = torch.full((nseg,), -float("inf"), dtype=torch.float64, device=x.device)
    mx = mx.scatter_reduce(0, inv, x, reduce="amax", include_self=True)
    ex = torch.exp(x - mx[inv])
    sm = torch.zeros(nseg, dtype=torch.float64, device=x.device).scatter_add_(0, inv, ex)
    lse = torch.log(sm) + mx                                   # scipy.special.logsumexp
    p = torch.exp(x - lse[inv])
    p = torch.where(cnt[inv] > 1, p, torch.ones_like(p))
    q = -10.0 * torch.log10(torch.clamp(1.0 - p, epsilon, 1.0 - epsilon))
    q = torch.where(torch.isnan(p), torch.full_like(q, -10.0 * math.log10(1.0 - epsilon)), q)
    return src, dst, q + pseudo_count


def canonical_order(src, dst, num_nodes: int):
    return torch.argsort(src * int(num_nodes) + dst, stable=True)


def neighbour_edges(num_nodes: int, neighbours: int = 1, device=None) -> torch.Tensor:
    """dataset.py:356-366: (i, j) for j in [i-n, i+n] ∩ [0, N), j == i INCLUDED, nested-loop order
    (ignores genome ends, ignores synteny shuffling — exactly like the reference)."""
    i = torch.arange(num_nodes, dtype=torch.int64, device=device).repeat_interleave(2 * neighbours + 1)
    j = i + torch.arange(-neighbours, neighbours + 1, dtype=torch.int64, device=device).repeat(num_nodes)
    keep = (j >= 0) & (j < num_nodes)
    return torch.stack([i[keep], j[keep]])


def _graph_edges(num_nodes: int, src, dst, value):
    """the relation's entries that become edges (no self loops, ids in [0, N): preprocessing.py:98-109), canonical order"""
    ok = (src != dst) & (src >= 0) & (dst >= 0) & (src < num_nodes) & (dst < num_nodes)
    s, d, v = src[ok], dst[ok], value[ok]
    o = canonical_order(s, d, num_nodes)
    return s[o], d[o], v[o]


def whole_graph(num_nodes: int, src, dst, weight, group_of: Optional[torch.Tensor], neighbours: int = 1,
                pair_src=None, pair_dst=None, keep_raw: bool = False, raw=None, genome_of=None):
    """dataset.py:325-384: one Data-like object for the whole graph.

    (src, dst, weight): normalised relation.  Self loops and ids outside [0, N) are skipped
    (preprocessing.py:98-109).  Labels: 1 iff the two genes are in the same ortholog group —
    given either as `group_of[node]` or as explicit directed pairs (pair_src, pair_dst) which are
    matched in both directions (preprocessing.py:145-148).

    keep_raw: the object also carries `raw_score` — the bit score of every edge, in the graph's edge order, dtype as
    given — and `genome_of`, the inputs of pangnn_amd.weights (a learnable normalisation of the same scores).  `raw` is the
    relation (src, dst, score) that was normalised: one score per ordered pair, any order."""
    dev = src.device
    s, d, w = _graph_edges(num_nodes, src, dst, weight)
    if group_of is not None:
        gs, gd = group_of[s], group_of[d]
        y = ((gs == gd) & (gs >= 0)).to(torch.float32)
    else:
        k = torch.cat([pair_src * num_nodes + pair_dst, pair_dst * num_nodes + pair_src]).unique()
        e = s * num_nodes + d
        pos = torch.searchsorted(k, e).clamp_(max=max(k.numel() - 1, 0))
        y = (k[pos] == e).to(torch.float32) if k.numel() else torch.zeros_like(e, dtype=torch.float32)
    g = SimpleNamespace(
        x=torch.ones(num_nodes, 1, dtype=torch.float32, device=dev),
        edge_index=torch.stack([s, d]),
        edge_attr=w.to(torch.float32),
        y=y,
        neighbour_edge_index=neighbour_edges(num_nodes, neighbours, dev),
        num_nodes=num_nodes,
    )
    if keep_raw:
        if raw is None or genome_of is None:
            raise ValueError("whole_graph: keep_raw needs `raw` = (src, dst, score) and `genome_of`")
        rs, rd, rsc = _graph_edges(num_nodes, *raw)
        if not (torch.equal(rs, s) and torch.equal(rd, d)):
            raise ValueError("whole_graph: `raw` does not hold exactly the normalised relation's pairs")
        g.raw_score, g.genome_of = rsc.contiguous(), genome_of
    return g


def build_from_raw(num_nodes, raw_src, raw_dst, raw_score, genome_of, group_of=None, pair_src=None,
                   pair_dst=None, neighbours: int = 1, t: float = 0.8, include_trivial: bool = False,
                   keep_raw: bool = False):
    """raw relation -> remove_trivial_cases -> normalize_sim_scores -> whole-graph tensors
    (dataset.py:70,103,111-112 then generate_graphs).  keep_raw: see whole_graph."""
    s, d, sc = raw_src, raw_dst, raw_score
    if not include_trivial:
        s, d, sc = remove_trivial_cases(s, d, sc, genome_of)
    raw = (s, d, sc) if keep_raw else None
    s, d, w = normalize_sim_scores(s, d, sc, genome_of, t=t)
    return whole_graph(num_nodes, s, d, w, group_of, neighbours, pair_src, pair_dst, keep_raw, raw, genome_of)
