"""`AlternateGCN` — drop-in for /root/reference/src/gnn.py:84-207 on MI355X.

Same constructor signature (`device, dataset, categorical_nodes, dims=[node_dim, hidden_dim]`), same
`forward(graph) -> logits [E]`, same `state_dict` keys and shapes:

  embedding.{weight[D,1],bias[D]}   conv_in.{bias[H],lin.weight[H,D]}   conv_hidden.{bias[H],lin.weight[H,H]}
  conv_out.{bias[D],lin.weight[D,H]}   linear_out.{weight[D,H],bias[D]}
  mlp.0.{weight[D,2D(+1)],bias[D]}   mlp.2.{weight[D,D],bias[D]}   mlp.4.{weight[1,D],bias[1]}

The reference reads its topology flags from a module-global argparse namespace
(gnn.py:5,111,128,132,143,171-180); here they are constructor kwargs, and `args=` accepts that same
namespace (anything with the attributes) so the reference's call site works unchanged.

Decoder: `mlp.0` applied to cat(z[src], z[dst] [, w]) is computed in the re-associated form
P[src] + Q[dst] (+ w*c) with P = z W_a^T, Q = z W_b^T + b — identical algebra, E*2D*D fewer
multiply-adds and no [E, 2D] intermediate (pangnn_edge_pair_add_f32).  `fused_decoder=False`
selects the literal gather-concat-Linear form (pangnn_edge_gather_concat_f32).

First layer: `conv_in(embedding(x))` with the scalar node feature is one operator evaluated by linearity
(functional._EmbedConvIn): A_hat (x w^T + 1 b^T) W^T + b_in = r a^T + s c^T + b_in with the node vectors
r = A_hat x, s = A_hat 1 computed once per graph by the propagate kernel and a = W w, c = W b per step — one
[N, H] write forward, three weighted column sums of dL/dout backward, no per-step propagate or dense product.
`fuse_embedding="propagate"` = round 2's form (per-step propagate of h0, embedding gradients by linearity),
`fuse_embedding=False` the layer-by-layer form (what the reference executes); all three are tested against
each other and the oracle.

Activations: every `h = ELU(layer(...))` of the encoder is consumed by exactly one dense layer, so the ELU runs
inside that layer's kernels (`functional.linear(..., in_act=1)`); `fold_activation=False` applies it as its own
op.  `encode()` always returns activated embeddings.
"""
from __future__ import annotations

import os
from types import SimpleNamespace
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from . import functional as PF
from .convolution import GCNConv
from .graph import structure_of

_FLAG_DEFAULTS = dict(union_edge_weights=False, base_model=False, skip_connections=False,
                      decoder="mlp", neighbours=1)


class AlternateGCN(nn.Module):
    def __init__(self, device=None, dataset=None, categorical_nodes: bool = False, dims=(64, 128),
                 args=None, num_nodes: Optional[int] = None, fused_decoder: bool = True,
                 fuse_embedding: bool = True, fold_activation: bool = True, fuse_first_dense: Optional[bool] = None,
                 deferred_logits: Optional[bool] = None, **flags):
        super().__init__()
        self.device = device
        cfg = dict(_FLAG_DEFAULTS)
        if args is not None:
            for k in cfg:
                if hasattr(args, k):
                    cfg[k] = getattr(args, k)
        unknown = set(flags) - set(cfg)
        if unknown:
            raise TypeError(f"unknown flags: {sorted(unknown)}")
        cfg.update(flags)
        self.flags = SimpleNamespace(**cfg)
        self.fused_decoder = fused_decoder
        self.fuse_embedding = fuse_embedding
        self.fold_activation = fold_activation
        # None: on unless PANGNN_FUSE_FIRST_DENSE=0 (same-box A/B of bench.py)
        self.fuse_first_dense = (os.environ.get("PANGNN_FUSE_FIRST_DENSE", "1") != "0") if fuse_first_dense is None \
            else bool(fuse_first_dense)
        # None: on unless PANGNN_DEFERRED_LOGITS=0 — training-mode forward() returns a DeferredLogits handle (deferred.py)
        self.deferred_logits = (os.environ.get("PANGNN_DEFERRED_LOGITS", "1") != "0") if deferred_logits is None \
            else bool(deferred_logits)
        node_embedding_dim, hidden_dim = dims

        if categorical_nodes:
            # The reference's categorical path cannot run (gnn.py:93 takes len() of a list of graphs,
            # and x is float ones, dataset.py:369).  Build-defined semantics:
            # x holds integer gene positions, one embedding row per node.
            if num_nodes is None:
                num_nodes = len(dataset.x) if hasattr(dataset, "x") else None
            if num_nodes is None:
                raise ValueError("categorical_nodes=True needs num_nodes=")
            self.embedding = nn.Embedding(int(num_nodes), node_embedding_dim)
        else:
            self.embedding = nn.Linear(1, node_embedding_dim)
        self.categorical_nodes = categorical_nodes

        self.conv_in = GCNConv(node_embedding_dim, hidden_dim, add_self_loops=False)
        self.conv_hidden = GCNConv(hidden_dim, hidden_dim, add_self_loops=False)
        self.conv_out = GCNConv(hidden_dim, node_embedding_dim, add_self_loops=False)
        self.linear_out = nn.Linear(hidden_dim, node_embedding_dim)
        self.activation_fct = nn.ELU()
        d = node_embedding_dim
        self.mlp = nn.Sequential(
            nn.Linear(2 * d + (1 if self.flags.skip_connections else 0), d), nn.ReLU(),
            nn.Linear(d, d), nn.ReLU(), nn.Linear(d, 1))
        self.epoch = 0
        if device is not None:
            self.to(device)

    # ---------------------------------------------------------------------------------
    # The wiring of the model (`_encode_pre`, the decoder's first layer) is written once, against the primitives below;
    # dist.DistAlternateGCN evaluates the same wiring on a shard by overriding them.
    @staticmethod
    def _edge_index(graph, name):
        """edge list of the graph `name`: "sim" (similarity), "nb" (positional neighbours), "union" (both)"""
        return getattr(graph, {"sim": "edge_index", "nb": "neighbour_edge_index", "union": "union_edge_index"}[name])

    def _edge_weight(self, graph, name, conv=None):
        """edge weights a layer on the graph `name` uses: `edge_attr` on "sim" and on "union" (dataset.py:380 stores the
        union weights there), none on "nb" (gnn.py:165) and for conv_out (gnn.py:138,165)"""
        return None if (name == "nb" or conv is self.conv_out) else graph.edge_attr

    def _weight_grad(self, graph) -> bool:
        """`graph.edge_attr` is a differentiable input of this call (it requires grad and grad is on).  Then the operators
        that rest on per-graph cached A_hat x, A_hat 1 do not apply (a cached vector cannot carry a gradient): the first layer
        takes the layer-by-layer route, every weighted GCN layer goes through GCNConv's PF.propagate_w route, and with
        `--skip_connections`, where the weights are also the decoder's per-edge input, the decoder is the literal
        gather-concat form.  Raises NotImplementedError where a tracer / dispatch mode is watching (PF.wants_weight_grad)."""
        return PF.wants_weight_grad(getattr(graph, "edge_attr", None))

    def _linear(self, x, w, b, in_act: int = 0, out_dtype=None):
        """one node-level dense layer"""
        return PF.linear(x, w, b, in_act, out_dtype)

    def _conv(self, conv, h, graph, name, in_elu: bool = False, dense_done: bool = False):
        """one GCN layer on the graph `name` (GCNConv.forward: in_elu, dense_done)"""
        return conv(h, self._edge_index(graph, name), self._edge_weight(graph, name, conv), graph=graph, name=name,
                    in_elu=in_elu, dense_done=dense_done)

    def _embed_conv_in(self, graph, name):
        """act-less `conv_in(embedding(x))` (gnn.py:125-131,143-146,156-158)"""
        x, conv = graph.x, self.conv_in
        _lib.require_device(x)
        if self.categorical_nodes:
            return self._conv(conv, self.embedding(x.long().view(-1)), graph, name)
        if self.fuse_embedding and (self.fuse_embedding != "propagate" or conv.in_channels < conv.out_channels) \
                and not self._weight_grad(graph):
            st, norm = self._first_layer_graph(graph, name)
            out_dtype = PF.autocast_rows_dtype(x)          # the autocast Linear's output type (bf16 / fp16 mixed precision)
            if self.fuse_embedding != "propagate":
                # the whole layer by linearity: r a^T + s c^T + b_in, r = A_hat x and s = A_hat 1 cached per graph
                # (functional._EmbedConvIn) — one [N, H] write per step, one pass over its gradient in backward
                return PF.embed_conv_in(x, self.embedding.weight, self.embedding.bias, conv.lin.weight, conv.bias, st,
                                        norm, out_dtype)
            # round 2's form: embedding + propagate as one operator whose backward yields the embedding's two parameter
            # gradients without the transposed propagate (functional._EmbedPropagate), then the dense layer
            agg = PF.embed_propagate(x, self.embedding.weight, self.embedding.bias, st, norm, tag=name)
            return PF.linear(agg, conv.lin.weight, conv.bias, 0, out_dtype)
        # Linear(1, D) on a [N,1] column is an outer product; as a GEMM its weight gradient is a
        # 64 x 1 x N problem that the BLAS library runs at < 0.1 TB/s
        h = x.float().view(-1, 1) * self.embedding.weight.view(1, -1) + self.embedding.bias
        return self._conv(conv, h, graph, name)

    def _first_layer_graph(self, graph, name):
        """(structure, normalisation) of the graph `name` for the first layer's fused operators"""
        st = structure_of(self._edge_index(graph, name), graph.x.shape[0], holder=graph, name=name)
        w = self._edge_weight(graph, name)
        if w is not None and w.shape[0] != st.num_edges:
            raise ValueError(f"edge_weight has {w.shape[0]} entries for {st.num_edges} edges")
        return st, st.gcn_norm(w)

    def _embed_conv_in_then_dense(self, graph, name, w_out, bias_out):
        """linear(ELU(conv_in(embedding(x))), w_out, bias_out) with the [N, H] rows of the first layer generated inside the
        dense layer's kernels (functional._EmbedConvInLinear) — or None where that operator does not apply: categorical
        nodes, fuse_embedding / fuse_first_dense / fold_activation off, widths its kernels do not cover, bf16 / fp16 autocast
        (the reference's autocast stores those rows in the autocast type; the generated rows are fp32)."""
        x, conv = graph.x, self.conv_in
        if self.categorical_nodes or not self.fuse_first_dense or not self._fold_elu() or not self.fuse_embedding \
                or self.fuse_embedding == "propagate" or self._weight_grad(graph):
            return None
        if w_out.shape[1] != conv.out_channels or not PF.embed_linear_supported(conv.out_channels, w_out.shape[0]):
            return None
        _lib.require_device(x)
        if PF.autocast_rows_dtype(x) is not None:
            return None
        st, norm = self._first_layer_graph(graph, name)
        return PF.embed_conv_in_linear(x, self.embedding.weight, self.embedding.bias, conv.lin.weight, conv.bias, w_out,
                                       bias_out, st, norm)

    def _fold_elu(self) -> bool:
        """the encoder's activation (gnn.py:108: ELU) can be folded into the dense layer that follows it"""
        a = self.activation_fct
        return self.fold_activation and isinstance(a, nn.ELU) and float(a.alpha) == 1.0

    def _encode_pre(self, graph):
        """(z or its pre-activation, pending): every `h = act(layer(...))` of gnn.py:125-166 is consumed by exactly
        one dense layer (GCNConv.lin of the next conv, linear_out, or the decoder's first layer), so with ELU the
        activation runs inside that layer's kernels (`in_elu` / `in_act`) and only the LAST one can be left pending for
        the caller.  `graph` is whatever the primitives above take: a Data / Batch here, a shard in dist.py."""
        fl, fold = self.flags, self._fold_elu()
        self._weight_grad(graph)         # (differentiable edge weights under a tracer / dispatch mode: raises before any launch)
        pre = (lambda h: h) if fold else self.activation_fct      # an ELU that is not folded runs as its own op
        if fl.union_edge_weights:                                              # gnn.py:128-139
            hid = self.conv_hidden
            y = self._embed_conv_in_then_dense(graph, "union", hid.lin.weight, None) \
                if hid.in_channels >= hid.out_channels else None
            h = self._embed_conv_in(graph, "union") if y is None else None
            for k in range(max(fl.neighbours - 2, 1)):
                if k == 0 and y is not None:           # the first hidden layer's dense part came fused with conv_in
                    h = self._conv(hid, y, graph, "union", dense_done=True)
                else:
                    h = self._conv(hid, pre(h), graph, "union", in_elu=fold)
            h = self._conv(self.conv_out, pre(h), graph, "union", in_elu=fold)
        elif fl.base_model:                                                    # gnn.py:143-150
            h = self._embed_conv_in_then_dense(graph, "sim", self.linear_out.weight, self.linear_out.bias)
            if h is None:
                h = self._embed_conv_in(graph, "sim")
                h = self._linear(pre(h), self.linear_out.weight, self.linear_out.bias, 1 if fold else 0)
        else:                                                                  # gnn.py:153-166
            out = self.conv_out
            y = self._embed_conv_in_then_dense(graph, "sim", out.lin.weight, None) \
                if out.in_channels >= out.out_channels else None
            if y is not None:                          # conv_out's dense part came fused with conv_in: propagate + bias left
                h = self._conv(out, y, graph, "nb", dense_done=True)
            else:
                h = self._conv(out, pre(self._embed_conv_in(graph, "sim")), graph, "nb", in_elu=fold)
        return h, True

    def encode(self, graph) -> torch.Tensor:
        h, pending = self._encode_pre(graph)
        return self.activation_fct(h) if pending else h

    def _fused_width(self) -> bool:
        """node_dim is a width the fused per-edge MLP kernels are built for: 64 (csrc/decoder.hip, decoder16.hip) or one of
        PF.DECODER_ND_WIDTHS (the width template of csrc/decoder.hip in both precision modes: f32 matrix pipe, float32 P | Q rows,
        no DeferredLogits)"""
        d = self.mlp[2].in_features
        return d == 64 or d in PF.DECODER_ND_WIDTHS

    def _decoder16(self) -> bool:
        """the fused kernels run in their default precision mode at node_dim 64: the one-pass training decoder is
        functional._decoder_train16 and P | Q rows are read as stored, so under bf16 / fp16 autocast they may be stored in the
        autocast type"""
        return self.mlp[2].in_features == 64 and PF.DECODER_PRECISION == 1

    def _skip_feature(self, graph):
        """the per-edge input of `--skip_connections` (gnn.py:173), else None"""
        return graph.edge_attr[: graph.edge_index.shape[1]] if self.flags.skip_connections else None

    def _literal_decoder(self, graph) -> bool:
        """the decoder's per-edge input needs a gradient (`--skip_connections` with differentiable edge weights): the literal
        gather-concat decoder, whose backward hands dL/dextra on — no fused kernels, no DeferredLogits"""
        return bool(self.flags.skip_connections) and self._weight_grad(graph)

    def _pq_operands(self, z):
        """(w_pq, b_pq, cvec) of the re-associated first decoder layer"""
        lin0 = self.mlp[0]
        return PF.pq_operands(lin0.weight, lin0.bias, z.shape[1], bool(self.flags.skip_connections))

    def _decoder_pq(self, z, graph, in_act: int = 0, rows16: bool = True, operands=None):
        """(P | Q [N, 2D], extra, cvec) of the re-associated first decoder layer: ONE node-level product
        z [W_a ; W_b]^T + [0 ; b1].  bf16 / fp16 mixed precision: mlp[0] is an autocast Linear, its node-level halves are
        stored (and gathered) in that type where the decoder kernel reads them so (`rows16`: the caller's decoder does)"""
        w_pq, b_pq, cvec = self._pq_operands(z) if operands is None else operands
        pq_dtype = PF.autocast_rows_dtype(z) if (rows16 and self._decoder16()) else None
        return self._linear(z, w_pq, b_pq, in_act, pq_dtype), self._skip_feature(graph), cvec

    def _fused_decoder_operands(self, graph):
        """(pq, structure, extra, cvec, layer) of the one-pass training decoder, or None where that kernel does not apply
        (another decoder, a node_dim it is not built for, no gradient wanted): the encoder (gnn.py:125-166) with its last ELU
        folded into the node-level half of `mlp[0]` (gnn.py:110,173-175).  Where PF.decoder_loss_z applies (see
        PF.fused_pq_backward_applies) the P | Q product is left to that operator: pq is None and layer = (z, w_pq, b_pq,
        in_act)."""
        z, pending = self._encode_pre(graph)
        fused = "mlp" in self.flags.decoder and self.fused_decoder is True and self._fused_width() and torch.is_grad_enabled() \
            and not self._literal_decoder(graph)
        if not (fused and pending and self._fold_elu()):
            z, pending = (self.activation_fct(z) if pending else z), False
        if not fused:
            return None, z
        st = structure_of(graph.edge_index, z.shape[0], holder=graph, name="sim")
        in_act = 1 if pending else 0
        operands = self._pq_operands(z)
        if type(self)._linear is AlternateGCN._linear and self._decoder16() and PF.fused_pq_backward_applies(
                z, operands[0], operands[1], st, getattr(graph, "live_edges", None)):
            return (None, st, self._skip_feature(graph), operands[2], (z, operands[0], operands[1], in_act)), z
        pq, extra, cvec = self._decoder_pq(z, graph, in_act, operands=operands)
        return (pq, st, extra, cvec, None), z

    def loss_and_logits(self, graph, labels, pos_weight=None):
        """`criterion(model(graph), labels)` (pangnn.py:200-203) as ONE decoder pass when the fused kernel
        applies (mlp decoder, node_dim 64, 32 or 128): returns (loss, detached logits).  Falls back to forward +
        criterion otherwise.  `model(graph)` followed by torch's / this package's BCEWithLogitsLoss reaches the same pass
        through the handle `forward` returns in training mode (deferred.DeferredLogits)."""
        from .train import criterion
        ops, z = self._fused_decoder_operands(graph)
        # a padded fixed-shape batch (SubGraphDataset.padded_buffers) carries the number of its real edges on the device; every
        # fused loss kernel reads it there (decoder16.hip's S / T pair, decoder.hip's one-pass backward, edge_score.hip)
        live = getattr(graph, "live_edges", None)
        if ops is not None:
            pq, st, extra, cvec, layer = ops
            if layer is not None:
                return PF.decoder_loss_z(*layer, st, extra, cvec, self.mlp[2].weight, self.mlp[2].bias,
                                         self.mlp[4].weight.view(-1), self.mlp[4].bias, labels, pos_weight, labels.shape[0])
            return PF.decoder_loss_pq(pq, st, extra, cvec, self.mlp[2].weight, self.mlp[2].bias,
                                      self.mlp[4].weight.view(-1), self.mlp[4].bias, labels, pos_weight,
                                      labels.shape[0], live=live)
        mode = self._score_mode()
        if mode is not None and self._scores_fused(z):
            # cosine / dot: logits, loss and dL/dlogit in one edge pass, dL/dz in one node pass (csrc/edge_score.hip)
            st = structure_of(graph.edge_index, z.shape[0], holder=graph, name="sim")
            return PF.edge_score_loss(z, st, mode, labels, pos_weight, labels.shape[0], live=live)
        if live is not None:
            # what is left takes the literal per-edge route, whose kernels and criterion count the padding as edges
            raise NotImplementedError(
                "a padded fixed-shape batch needs a fused training decoder (fused_decoder=True): the mlp decoder at node_dim "
                "32, 64 or 128, or cosine / dot at a width of 16, 32, 64, 128 or 256 — and, with skip_connections, edge "
                "weights that need no gradient")
        out = self._decode(z, graph)
        return criterion(out, labels, pos_weight), out.detach()

    def _score_mode(self):
        """"dot" / "cosine" when `_decode` picks a weightless decoder ("dot" wins over "cosine", which wins over "mlp"), else None"""
        dec = self.flags.decoder
        return "dot" if "dot" in dec else "cosine" if "cosine" in dec else None

    def _scores_fused(self, z) -> bool:
        """the weightless decoders run on csrc/edge_score.hip (D in {16, 32, 64, 128, 256}); `fused_decoder=False` keeps the
        literal gather-concat route"""
        return bool(self.fused_decoder) and z.dim() == 2 and PF.edge_score_supported(z.shape[1])

    def _defers(self) -> bool:
        """training-mode `forward` hands out a DeferredLogits handle instead of launching the inference decoder: only where the
        one-pass training decoder could resolve it, and never while a tracer / dispatch mode watches (a traced program
        wants plain tensors: `loss_and_logits` is the traceable training entry)"""
        fl = self.flags
        return (self.deferred_logits and self.training and torch.is_grad_enabled() and fl.decoder == "mlp"
                and self.fused_decoder is True and self._decoder16()
                and not torch.compiler.is_compiling() and not PF.observed())

    def _decode(self, nodes, graph):
        fl = self.flags
        out = None
        if "mlp" in fl.decoder:
            out = self.decode_mlp(nodes, graph)
        if "cosine" in fl.decoder:
            out = self.cosine_sim(nodes, graph.edge_index, graph)
        if "dot" in fl.decoder:
            out = self.decode(nodes, graph.edge_index, graph)
        return out

    def decode_mlp(self, z, graph) -> torch.Tensor:
        st = structure_of(graph.edge_index, z.shape[0], holder=graph, name="sim")
        d = z.shape[1]
        if self.fused_decoder and d % 4 == 0 and not self._literal_decoder(graph):
            # `fused_decoder="pair_add"` keeps the layer-by-layer form behind the P | Q rows, which reads them as fp32
            fused = self._fused_width() and self.fused_decoder != "pair_add"
            pq, extra, cvec = self._decoder_pq(z, graph, rows16=fused)
            if fused:
                # whole per-edge MLP in one HIP kernel (f32 MFMA), no [E, D] tensor in HBM on the way
                return PF.decoder_mlp_pq(pq, st, extra, cvec, self.mlp[2].weight, self.mlp[2].bias,
                                         self.mlp[4].weight.view(-1), self.mlp[4].bias)
            h = PF.edge_pair_add(pq[:, :d].contiguous(), pq[:, d:].contiguous(), st, extra, cvec)
        else:
            h = self.mlp[0](PF.edge_gather_concat(z, st, self._skip_feature(graph)))
        for layer in list(self.mlp)[1:]:
            # [E, D] intermediates are the largest tensors of the step: rectify them in place
            h = torch.relu_(h) if isinstance(layer, nn.ReLU) else layer(h)
        return h.squeeze(-1)

    def forward(self, graph) -> torch.Tensor:
        """logits [E] (gnn.py:121-200).  In training mode with the mlp decoder the result is a `DeferredLogits` handle: the
        encoder and the node-level half of `mlp[0]` run here (inside accelerate's autocast wrapper of `forward`), the per-edge
        decoder when the handle is used — as ONE pass with the loss and every gradient if that use is
        `BCEWithLogitsLoss(pos_weight)(output, labels)` (pangnn.py:98,203), through the inference kernel on any other use."""
        if self._defers() and not self._literal_decoder(graph):
            ops, z = self._fused_decoder_operands(graph)
            if ops is not None:
                return self._deferred(graph, *ops)
            return self._decode(z, graph)
        return self._decode(self.encode(graph), graph)

    def _deferred(self, graph, pq, st, extra, cvec, layer=None):
        from .deferred import DeferredLogits
        w2, b2, w3, b3 = self.mlp[2].weight, self.mlp[2].bias, self.mlp[4].weight.view(-1), self.mlp[4].bias
        live = getattr(graph, "live_edges", None)

        def materialize():
            if live is not None:
                raise NotImplementedError("a padded fixed-shape batch needs the fused training decoder: call "
                                          "BCEWithLogitsLoss(pos_weight)(output, labels) on the model's output first")
            # (the fused loss forms P | Q itself: a use that needs the inference kernel computes the rows here)
            rows = pq if layer is None else self._linear(layer[0], layer[1], layer[2], layer[3])
            return PF.decoder_mlp_pq(rows, st, extra, cvec, w2, b2, w3, b3)

        def fused_loss(labels, pos_weight):
            if layer is not None:
                return PF.decoder_loss_z(*layer, st, extra, cvec, w2, b2, w3, b3, labels, pos_weight, labels.shape[0])
            return PF.decoder_loss_pq(pq, st, extra, cvec, w2, b2, w3, b3, labels, pos_weight, labels.shape[0], live=live)

        return DeferredLogits(st.num_edges, (pq if layer is None else layer[0]).device, materialize, fused_loss)

    def _pairs(self, z, edge_index, graph=None):
        st = structure_of(edge_index, z.shape[0], holder=graph, name="sim")
        both = PF.edge_gather_concat(z, st)
        d = z.shape[1]
        return both[:, :d], both[:, d:]

    def decode(self, z, edge_index, graph=None):
        # gnn.py:202-204 is `z[src] @ z[dst]`, a shape error unless E == D (broken in the
        # reference); build-defined semantics: per-edge dot product.
        if self._scores_fused(z):
            return PF.edge_score(z, structure_of(edge_index, z.shape[0], holder=graph, name="sim"), "dot")
        a, b = self._pairs(z, edge_index, graph)
        return (a * b).sum(dim=1)

    def cosine_sim(self, z, edge_index, graph=None):
        if self._scores_fused(z):
            return PF.edge_score(z, structure_of(edge_index, z.shape[0], holder=graph, name="sim"), "cosine")
        a, b = self._pairs(z, edge_index, graph)
        return F.cosine_similarity(a, b, dim=1)
