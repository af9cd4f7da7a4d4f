"""The Q-score edge weights as a differentiable function of the bit scores and of the softmax temperature.

construct.normalize_sim_scores turns bit scores into edge weights once, with the temperature (`--normalization_temp`, 0.8 in
the reference) baked in as a host constant.  GCNConv / AlternateGCN fill `edge_weight.grad` (DESIGN.md "Edge-weight
gradients"); this module is the producer that carries that gradient one step further, to the only trainable quantities in how
the model builds its input: the temperature and the scores.

  score_segments   the (source gene, candidate genome) groups over a graph's OWN edge list (built once per graph)
  qscore_weights   scores -> weights over such a plan, differentiable in `score` and in a tensor `t`
  QScoreWeights    the module: parameter log_t, `graph.raw_score` -> `edge_attr`

Device tensors run the two kernels of csrc/qscore.hip (pangnn_qscore_fwd / pangnn_qscore_bwd) behind one autograd.Function;
CPU tensors run the same definition in plain torch under autograd — the formula of normalize_sim_scores' CPU leg over the
plan, which is what the device is tested against (tests/test_qscore_weights.py).  The route is eager ctypes, like
functional.propagate_w: no dispatcher op, no torch.compile.
"""
from __future__ import annotations

import copy
import math
from typing import Optional

import torch
from torch import nn

from . import _lib
from . import functional as PF

SUM_PARTS = 1024                 # PANGNN_QSCORE_SUM_PARTS of include/pangnn_hip.h
DTYPE_F64 = 3                    # PANGNN_DTYPE_F64


class ScoreSegments:
    """The segment plan of one edge list: segment k holds the positions [rowptr[k], rowptr[k + 1]) of the (source, candidate
    genome) order, `item[pos]` (int32) is the edge at that position.  Per-edge arrays stay in the graph's edge order."""

    def __init__(self, rowptr: torch.Tensor, item: torch.Tensor):
        self.rowptr, self.item = rowptr, item
        self.num_segments, self.num_edges = int(rowptr.shape[0]) - 1, int(item.shape[0])
        self._of_edge = None

    @property
    def device(self):
        return self.item.device

    @property
    def counts(self) -> torch.Tensor:
        return self.rowptr[1:] - self.rowptr[:-1]

    @property
    def segment_of_edge(self) -> torch.Tensor:
        """int64 [E]: the segment of every edge (what the plain-torch formulation scatters by); built on first use"""
        if self._of_edge is None:
            ids = torch.repeat_interleave(torch.arange(self.num_segments, device=self.device), self.counts,
                                          output_size=self.num_edges)
            self._of_edge = torch.empty_like(ids).scatter_(0, self.item.long(), ids)
        return self._of_edge


def score_segments(edge_index: torch.Tensor, genome_of: torch.Tensor, holder=None) -> ScoreSegments:
    """The plan of `edge_index` [2, E] (row 0 = source gene, row 1 = candidate): key = src * G + genome_of[dst], positions by
    stable argsort of the key.  CPU or device tensors.  With `holder` (the graph object) the plan is built once and kept on it
    (`holder._pangnn_score_segments`), the way graph.structure_of keeps structures."""
    key_of = (edge_index.data_ptr(), edge_index._version, tuple(edge_index.shape), edge_index.device,
              genome_of.data_ptr(), genome_of._version)
    if holder is not None:
        hit = getattr(holder, "_pangnn_score_segments", None)
        if hit is not None and hit[0] == key_of:
            return hit[1]
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError(f"score_segments: edge_index must be [2, E], got {tuple(edge_index.shape)}")
    e = int(edge_index.shape[1])
    if e >= 2 ** 31:
        raise ValueError("score_segments: the int32 plan cannot address 2^31 edges or more")
    src, dst = edge_index[0].long(), edge_index[1].long()
    genome_of = genome_of.to(edge_index.device).long()
    if e:
        g = genome_of.max() + 1                                   # (a tensor: nothing is read back for it)
        key = src * g + genome_of[dst]
        order = torch.argsort(key, stable=True)
        _, cnt = torch.unique_consecutive(key[order], return_counts=True)
    else:
        order = torch.zeros(0, dtype=torch.int64, device=edge_index.device)
        cnt = torch.zeros(0, dtype=torch.int64, device=edge_index.device)
    rowptr = torch.zeros(cnt.numel() + 1, dtype=torch.int64, device=edge_index.device)
    torch.cumsum(cnt, 0, out=rowptr[1:])
    seg = ScoreSegments(rowptr, order.to(torch.int32).contiguous())
    if holder is not None:
        try:
            setattr(holder, "_pangnn_score_segments", (key_of, seg))
        except Exception:
            pass
    return seg


def wants_qscore_grad(score, t) -> bool:
    """`score` or a tensor `t` is a differentiable input of this call.  The device route is ctypes only, so where a tracer or a
    dispatch / function mode is watching it raises instead of dropping the gradient (functional.wants_weight_grad)."""
    if not torch.is_grad_enabled() or not (score.requires_grad or (torch.is_tensor(t) and t.requires_grad)):
        return False
    if PF.observed():
        raise NotImplementedError("pangnn_amd: the gradient with respect to the score / temperature of qscore_weights has no "
                                  "dispatcher op yet — it cannot be traced, compiled or run under a dispatch / function mode; "
                                  "detach the inputs or run eagerly")
    return True


def _code(dtype) -> int:
    return DTYPE_F64 if dtype == torch.float64 else 0


class _QScore(torch.autograd.Function):
    """weights [E] from scores [E] (float32 / float64, contiguous) and t (float64 [1]) on the device: pangnn_qscore_fwd, with
    lse kept for pangnn_qscore_bwd, which computes only the gradients asked for"""

    @staticmethod
    def forward(ctx, score, t, seg: ScoreSegments, eps: float, pseudo: float, out_dtype):
        w = torch.empty(seg.num_edges, dtype=out_dtype, device=score.device)
        lse = torch.empty(2 * seg.num_segments, dtype=torch.float64, device=score.device)     # lse, then its rounding residual
        PF._launch(score.device, "pangnn_qscore_fwd", seg.rowptr.data_ptr(), seg.item.data_ptr(), score.data_ptr(),
                   _code(score.dtype), seg.num_segments, seg.num_edges, t.data_ptr(), eps, pseudo, w.data_ptr(),
                   _code(out_dtype), lse.data_ptr())
        ctx.save_for_backward(score, t, lse)
        ctx.seg, ctx.eps = seg, eps
        return w

    @staticmethod
    def backward(ctx, g):
        score, t, lse = ctx.saved_tensors
        seg = ctx.seg
        want_s, want_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_s or want_t):
            return None, None, None, None, None, None
        if g.dtype not in (torch.float32, torch.float64):
            g = g.float()
        g = g.contiguous()
        gs = torch.empty_like(score) if want_s else None
        gt = parts = None
        if want_t:
            gt = torch.empty(1, dtype=torch.float64, device=score.device)
            parts = torch.empty(seg.num_segments + SUM_PARTS, dtype=torch.float64, device=score.device)
        PF._launch(score.device, "pangnn_qscore_bwd", seg.rowptr.data_ptr(), seg.item.data_ptr(), score.data_ptr(),
                   _code(score.dtype), g.data_ptr(), _code(g.dtype), lse.data_ptr(), seg.num_segments, seg.num_edges,
                   t.data_ptr(), ctx.eps, _lib.ptr(gs), _lib.ptr(gt), _lib.ptr(parts))
        return gs, gt, None, None, None, None


def _qscore_torch(score, t, seg: ScoreSegments, eps: float, pseudo: float, out_dtype):
    """the definition: normalize_sim_scores' CPU leg over the plan, in plain torch (differentiable by autograd)"""
    inv, cnt = seg.segment_of_edge, seg.counts
    x = score.to(torch.float64) / t
    n = seg.num_segments
    mx = torch.full((n,), -float("inf"), dtype=torch.float64, device=x.device)
    # (lse does not depend on the shift: no gradient through the maximum)
    mx = mx.scatter_reduce(0, inv, x.detach(), reduce="amax", include_self=True)
    ex = torch.exp(x - mx[inv])
    sm = torch.zeros(n, dtype=torch.float64, device=x.device).scatter_add(0, inv, ex)
    lse = torch.log(sm) + mx                                   # scipy.special.logsumexp
    p = torch.exp(x - lse[inv])
    p = torch.where(cnt[inv] > 1, p, torch.ones_like(p))
    q = -10.0 * torch.log10(torch.clamp(1.0 - p, eps, 1.0 - eps))
    q = torch.where(torch.isnan(p), torch.full_like(q, -10.0 * math.log10(1.0 - eps)), q)
    return (q + pseudo).to(out_dtype)


def qscore_weights(score: torch.Tensor, seg: ScoreSegments, t=0.8, epsilon: float = 1e-8, pseudo_count: float = 1.0,
                   out_dtype=torch.float32) -> torch.Tensor:
    """Edge weights [E] (`out_dtype`: float32 or float64, the graph's edge order) from bit scores [E] over the plan `seg`: per
    segment p = softmax(score / t) (one candidate: p = 1), w = -10 log10(clip(1 - p, epsilon, 1 - epsilon)) + pseudo_count, in
    float64 — construct.normalize_sim_scores over the graph's own edges.  Differentiable in `score` and, when `t` is a tensor
    (0-dim or one element), in `t`; the gradients come back in the inputs' dtypes.  On the device `t` is never read on the
    host, and a warm call reads nothing back.

    The plan covers the edges the graph kept, so the weights are those of the construction whenever construct.whole_graph
    dropped nothing after normalisation; ids outside [0, N) in the raw relation (whose edges it drops, while they still count
    as candidates in normalize_sim_scores' groups) would make the two differ."""
    if score.dim() != 1 or score.shape[0] != seg.num_edges:
        raise ValueError(f"qscore_weights: score must be [{seg.num_edges}], got {tuple(score.shape)}")
    if out_dtype not in (torch.float32, torch.float64):
        raise ValueError(f"qscore_weights: out_dtype must be float32 or float64, got {out_dtype}")
    if not 0.0 < epsilon < 0.5:
        raise ValueError(f"qscore_weights: epsilon must lie in (0, 0.5), got {epsilon}")
    if torch.is_tensor(t):
        if t.numel() != 1:
            raise ValueError(f"qscore_weights: t must hold one element, got {tuple(t.shape)}")
        if t.device != score.device:
            raise ValueError(f"qscore_weights: t lives on {t.device}, score on {score.device}")
    if not score.is_cuda:
        t64 = t.to(torch.float64).reshape(()) if torch.is_tensor(t) else float(t)
        return _qscore_torch(score, t64, seg, float(epsilon), float(pseudo_count), out_dtype)
    _lib.require_device(seg.item, seg.rowptr)
    wants_qscore_grad(score, t)                   # (raises where a tracer / dispatch mode is watching: no dispatcher op)
    if score.dtype not in (torch.float32, torch.float64):
        score = score.to(torch.float64)
    if torch.is_tensor(t):
        t64 = t.to(torch.float64).reshape(1)
    else:
        t64 = torch.full((1,), float(t), dtype=torch.float64, device=score.device)     # (a fill: no copy from the host)
    if seg.num_edges == 0:
        return torch.empty(0, dtype=out_dtype, device=score.device)
    return _QScore.apply(score.contiguous(), t64, seg, float(epsilon), float(pseudo_count), out_dtype)


class QScoreWeights(nn.Module):
    """Edge weights of a graph from its bit scores with a learnable softmax temperature: t = exp(log_t), so the temperature
    stays positive under any optimiser.  `forward(graph)` reads `graph.raw_score`, `graph.edge_index` and `graph.genome_of`
    (construct.build_from_raw / simulate.simulate_graph with keep_raw=True) and returns [E] float32 weights in edge order;
    `apply_to(graph)` returns a shallow copy of the graph with them as `edge_attr`, ready for `model(...)` /
    `model.loss_and_logits(...)`, whose backward then reaches `log_t` (and `raw_score`, where that requires grad)."""

    def __init__(self, t: float = 0.8, learn_t: bool = True, epsilon: float = 1e-8, pseudo_count: float = 1.0):
        super().__init__()
        if not t > 0.0:
            raise ValueError(f"QScoreWeights: t must be positive, got {t}")
        self.log_t = nn.Parameter(torch.tensor(math.log(t), dtype=torch.float64), requires_grad=bool(learn_t))
        # t = t_init * exp(log_t - log_t_init): exactly the given temperature until log_t moves (exp(log(0.8)) is not 0.8)
        self.register_buffer("t_init", torch.tensor(float(t), dtype=torch.float64))
        self.register_buffer("log_t_init", self.log_t.detach().clone())
        self.epsilon, self.pseudo_count = float(epsilon), float(pseudo_count)

    def temperature(self) -> torch.Tensor:
        return self.t_init * torch.exp((self.log_t - self.log_t_init).to(torch.float64))

    def forward(self, graph) -> torch.Tensor:
        seg = score_segments(graph.edge_index, graph.genome_of, holder=graph)
        return qscore_weights(graph.raw_score, seg, self.temperature(), self.epsilon, self.pseudo_count, torch.float32)

    def apply_to(self, graph, weights: Optional[torch.Tensor] = None):
        """a shallow copy of `graph` whose `edge_attr` is `weights` (default: this module's weights of the graph)"""
        out = copy.copy(graph)
        out.edge_attr = self(graph) if weights is None else weights
        return out
