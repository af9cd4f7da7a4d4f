"""The link-prediction train step around the model (pangnn.py:88-98,194-216): zero_grad ->
forward -> BCEWithLogits(pos_weight) -> backward -> Adam.  Host side is plain PyTorch; every
gather/scatter inside `model` runs in libpangnn_hip.so."""
from __future__ import annotations

import torch

from . import functional as PF


def criterion(logits, labels, pos_weight):
    """torch.nn.BCEWithLogitsLoss(pos_weight=class_balance) (pangnn.py:98) — loss and dL/dlogits from one
    HIP pass (device tensors only: there is no CPU path)"""
    from .deferred import DeferredLogits
    if isinstance(logits, DeferredLogits):     # training-mode model(graph): resolved by the one-pass decoder when it still can be
        loss = logits.fused_bce(labels, pos_weight)
        if loss is not None:
            return loss
        logits = logits.materialize()
    return PF.bce_with_logits(logits, labels, pos_weight)


def make_optimizer(model, lr: float = 1e-3, capturable: bool = False, fused: bool = True):
    """torch.optim.Adam(lr) of pangnn.py:88.  `fused=True`: PyTorch's single-launch Adam over all parameter tensors
    (the same update rule; ~8 launches fewer per step than the default foreach form, which is what a launch-bound
    mini-batch step notices)."""
    params = list(model.parameters())
    fused = bool(fused) and all(p.is_cuda and p.dtype == torch.float32 for p in params)
    return torch.optim.Adam(params, lr=lr, capturable=capturable, fused=fused)


def train_step(model, optimizer, graph, labels, pos_weight):
    """One step; returns (loss, logits) as device tensors without synchronising."""
    for group in optimizer.param_groups:              # optimizer.zero_grad(set_to_none=True) without its dynamo-disable
        for p in group["params"]:                     # wrapper (~20 us of a launch-bound mini-batch step)
            p.grad = None
    if hasattr(model, "loss_and_logits"):
        loss, out = model.loss_and_logits(graph, labels, pos_weight)                # fused forward + criterion
    else:
        out = model(graph)
        loss = criterion(out, labels, pos_weight)                                   # pangnn.py:98,203
    loss.backward(PF.unit_grad(loss.device))                                        # = loss.backward(), see unit_grad
    optimizer.step()
    return loss.detach(), out.detach()


@torch.no_grad()
def eval_step(model, graph, labels, pos_weight):
    out = model(graph)
    return criterion(out, labels, pos_weight), out


@torch.no_grad()
def evaluate(model, batches, pos_weight, threshold: float = 0.5) -> dict:
    """The validation pass of pangnn.py:241-290: mean loss over the batches, confusion counts at
    `threshold`, precision / recall / f1 / accuracy, ROC-AUC and PR-AUC.  Everything accumulates on the
    GPU; the only host synchronisation is the final read-out."""
    from .metrics import BinaryAUROC, BinaryAveragePrecision, BinaryConfusionMatrix, summary_from_confusion
    conf, auroc = None, BinaryAUROC()
    ap = BinaryAveragePrecision(share_curve_with=auroc)      # fed the same tensors: one sort serves both
    loss_sum, n_batches = None, 0
    was_training = model.training
    model.eval()
    for batch in batches:
        out = model(batch)
        loss = criterion(out, batch.y, pos_weight)
        loss_sum = loss if loss_sum is None else loss_sum + loss
        n_batches += 1
        if conf is None:
            conf = BinaryConfusionMatrix(threshold, device=out.device)
        conf.update_from_logits(out, batch.y)
        prob = torch.sigmoid(out)
        auroc.update(prob, batch.y)
        ap.update(prob, batch.y)
    model.train(was_training)
    if conf is None:
        raise ValueError("evaluate() needs at least one batch")
    res = summary_from_confusion(conf.compute())
    res.update(loss=float(loss_sum) / n_batches, roc_auc=float(auroc.compute()), pr_auc=float(ap.compute()))
    return res


class GraphedTrainStep:
    """The whole train step (zero_grad -> forward -> loss -> backward -> Adam) of ONE fixed batch captured
    into a HIP graph and replayed.  For the reference's regime (32 small sub-graphs per batch,
    pangnn.py:152-216) a step is ~70 launches of a few microseconds of GPU work each, i.e. bound by the
    host launch path; replaying a captured graph removes it.  One instance per distinct batch (shapes are
    baked in); parameters and optimizer state are shared, so instances for different batches can be
    replayed in any order, exactly like iterating a DataLoader.

    The batch's structures / normalisations are built (and cached on the batch) by the warm-up steps
    that precede capture, so the captured region contains kernel launches only."""

    def __init__(self, model, optimizer, graph, labels, pos_weight, warmup: int = 2):
        for g in optimizer.param_groups:
            if not g.get("capturable", False):
                raise ValueError("GraphedTrainStep needs torch.optim.Adam(..., capturable=True)")
        self.model, self.optimizer = model, optimizer
        self.graph, self.labels, self.pos_weight = graph, labels, pos_weight
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(warmup):
                self._step()
        torch.cuda.current_stream().wait_stream(s)
        self.cuda_graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.cuda_graph):
            self.loss, self.logits = self._step()

    def _step(self):
        self.optimizer.zero_grad(set_to_none=True)
        if hasattr(self.model, "loss_and_logits"):
            loss, out = self.model.loss_and_logits(self.graph, self.labels, self.pos_weight)
        else:
            out = self.model(self.graph)
            loss = criterion(out, self.labels, self.pos_weight)
        loss.backward(PF.unit_grad(loss.device))
        self.optimizer.step()
        return loss.detach(), out.detach()

    def __call__(self):
        self.cuda_graph.replay()
        return self.loss, self.logits


class _PaddedReplay:
    """What train.ReplayedFreshStep and train.ReplayedFreshEval share: fixed-shape buffers sized by `SubGraphDataset.padded_spec`
    (everyday ones of `slack` x the mean batch, worst-case ones built on first use), the step `self._step(buf)` captured into
    one HIP graph per set of buffers, and the choice of the set a batch fits.  A subclass states `_step(buf)` (one padded
    step, no host read-back; returns a tuple of tensors) and `_kept()`: the tensors a step changes that building a slot must
    leave as they were (the warm-up steps before capture run for real).  It sets `self.model` before `_init_slots`: the model's
    `union_edge_weights` flag selects the layout of the buffers (`SubGraphDataset.padded_buffers(union=)`)."""

    def _init_slots(self, ds, batch_size, graphs, capture, warmup, slack):
        self.ds, self.capture, self.warmup = ds, bool(capture), int(warmup)
        # a --union_edge_weights model reads `union_edge_index` and its weights: the buffers are collated in that layout
        self.union = bool(getattr(getattr(self.model, "flags", None), "union_edge_weights", False))
        self._first = list(range(min(batch_size, ds.num_graphs))) if graphs is None else [int(i) for i in list(graphs)[:batch_size]]
        worst = ds.padded_spec(batch_size, graphs)
        tight = worst if slack is None else ds.padded_spec(batch_size, graphs, slack)
        self.spec, self.spec_worst = tight, worst
        self._slots = {}                                   # spec -> (buffers, captured graph | None, the step's outputs | None)
        self._slot(tight)

    def _kept(self):
        return []

    def _restore(self, saved):
        with torch.no_grad():
            for t, v in zip(self._kept(), saved):
                t.copy_(v)

    def _slot(self, spec):
        """the buffers (and, with capture, the captured graph) of the padded shapes `spec`, built on first use"""
        hit = self._slots.get(spec)
        if hit is not None:
            return hit
        ds = self.ds
        buf = ds.padded_buffers(spec, union=self.union)
        first = [i for i in self._first]
        while len(first) > 1 and not ds.fits(spec, first):
            first.pop()
        ds.set_graph_ids(buf, first)
        if not self.capture:
            self._slots[spec] = (buf, None, None)
            return self._slots[spec]
        # the warm-up steps run on a side stream and are real steps on `first`: what they change is restored afterwards
        # (values copied back into the very tensors the captured graph updates), so that building a slot is not a step
        saved = self._save()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(max(self.warmup, 1)):
                self._step(buf)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = self._step(buf)
        torch.cuda.synchronize()
        self._restore(saved)
        self._slots[spec] = (buf, graph, outs)
        return self._slots[spec]

    def _save(self):
        return [t.detach().clone() for t in self._kept()]

    def _run(self, graph_ids):
        """(the step's outputs on the disjoint union of the sub-graphs `graph_ids`, its number of real edges)"""
        spec = self.spec if self.ds.fits(self.spec, graph_ids) else self.spec_worst
        buf, graph, outs = self._slot(spec)
        edges = self.ds.set_graph_ids(buf, graph_ids)[1]
        if graph is not None:
            graph.replay()
            return outs, edges
        return self._step(buf), edges


class ReplayedFreshStep(_PaddedReplay):
    """The reference's real regime — `DataLoader(batch_size=32, shuffle=True)`: every step sees a NEW batch
    (pangnn.py:152-153,180-216) — as ONE captured HIP graph that serves every mini-batch of a `SubGraphDataset`.

    What a fresh batch needs (collation, both CSR orders and run-sum plans of both edge lists, the degree normalisations, the
    first layer's node vectors r / s, then forward / loss / backward / Adam) is ~65 launches of a few microseconds each and
    therefore bound by the host's launch path (0.7-0.86 ms per step).  Here all of it is captured once:
      * the batch lives in buffers of FIXED shapes sized to the data set's maxima (`SubGraphDataset.padded_spec`), collated
        on the device from a device-resident list of sub-graph ids by `pangnn_collate_subgraphs_padded`, with an inert padded
        tail (self loops spread over the padded nodes, which are never real; the decoder kernels take the number of real edges from device memory:
        padded edges get dL/dlogit = 0 and the loss is the mean over the real ones);
      * so every kernel of the step runs on one shape, none of them needs a host-known size of the batch, and nothing reads
        back: the step is capturable, and a replay collates and trains on whatever ids the list holds at that moment.
    Per step the host does two things: one tiny launch that writes the next batch's ids (`pangnn_set_i64`, values carried in
    the kernel arguments) and one graph launch.  `capture=False` runs the very same padded step eagerly (the reference
    point of the bit-equality test).  Results equal the unpadded fresh step (`train_step` on `ds.batch(...)`) up to fp32
    re-association: padded rows are zero rows of every sum, but the per-workgroup partial sums of the node-level kernels are
    grouped by the padded row count.
    Served: every decoder whose fused loss kernel reads the real-edge count on the device — the mlp decoder at node_dim 64
    (decoder16.hip's S / T pair; csrc/decoder.hip's one-pass backward under PANGNN_DECODER_PRECISION=0) and at node_dim 32 /
    128 (csrc/decoder.hip), with or without `skip_connections`, and `cosine` / `dot` at a width of 16, 32, 64, 128 or 256
    (csrc/edge_score.hip).  Refused (NotImplementedError from `loss_and_logits`): a non-fused route (`fused_decoder=False` /
    "pair_add", any other width), differentiable edge weights with `skip_connections`.
    `--union_edge_weights` models are served with the same decoders: their buffers carry `union_edge_index` [2, spec.edges +
    spec.nb_edges] and its weights [real | ones] in place of the neighbour list, both CSR orders of the union list written by
    the same collation launch (`pangnn_collate_subgraphs_padded_union`); the decoder reads `edge_index`, `live_edges` and the
    similarity list's plans exactly as for any other model, and `skip_connections` reads `edge_attr[:spec.edges]`, the
    weights of `edge_index`.
    `stats`: a `metrics.EpochStats` (typically `capacity=0`) that the captured step ends with — the running training loss and
    the training confusion matrix of pangnn.py:218-222 with no host work per step; None: nothing changes."""

    def __init__(self, model, optimizer, ds, pos_weight, batch_size: int = 32, graphs=None, capture: bool = True,
                 warmup: int = 2, slack: float = 1.4, stats=None):
        """`slack`: the everyday buffers hold `slack` x the mean batch (SubGraphDataset.padded_spec); a batch that exceeds them
        runs through a second, worst-case set of buffers (and its own captured graph), built on first use.  None: worst-case
        buffers only."""
        if capture:
            for g in optimizer.param_groups:
                if not g.get("capturable", False):
                    raise ValueError("ReplayedFreshStep(capture=True) needs torch.optim.Adam(..., capturable=True)")
        if not hasattr(model, "loss_and_logits"):
            raise ValueError("ReplayedFreshStep needs a model with the fused loss_and_logits path")
        self.model, self.optimizer, self.pos_weight, self.stats = model, optimizer, pos_weight, stats
        self._init_slots(ds, batch_size, graphs, capture, warmup, slack)

    def _kept(self):
        return list(self.model.parameters()) + ([] if self.stats is None else [self.stats.state])

    def _save(self):
        import copy
        return super()._save(), copy.deepcopy(self.optimizer.state_dict())

    def _restore(self, saved):
        tensors, opt_state = saved
        super()._restore(tensors)
        with torch.no_grad():
            new_state = self.optimizer.state_dict()["state"]
            for k, st_ in new_state.items():
                old = opt_state["state"].get(k)
                for name, v in st_.items():
                    if torch.is_tensor(v):
                        if old is not None and torch.is_tensor(old.get(name)):
                            v.copy_(old[name])
                        else:
                            v.zero_()                      # a fresh optimizer: forget what the warm-up accumulated

    def _step(self, buf):
        """one padded fresh step: everything a new batch needs, no host read-back"""
        self.ds.collate_padded(buf)       # (also replaces / drops the structures cached on the buffers' addresses)
        self.optimizer.zero_grad(set_to_none=True)
        loss, out = self.model.loss_and_logits(buf, buf.y, self.pos_weight)
        loss.backward(PF.unit_grad(loss.device))
        self.optimizer.step()
        loss, out = loss.detach(), out.detach()
        if self.stats is not None:
            self.stats.update(out, buf.y, live=buf.live_edges, loss=loss)
        return loss, out

    def __call__(self, graph_ids):
        """train on the disjoint union of the sub-graphs `graph_ids` (host ints, any order, at most batch_size);
        returns (loss, logits of the batch's real edges) as device tensors without synchronising.  With capture the two
        are VIEWS of the captured graph's static outputs: the next call overwrites them — clone what must outlive it."""
        (loss, out), edges = self._run(graph_ids)
        return loss, out[:edges]


class ReplayedFreshEval(_PaddedReplay):
    """The validation loop of pangnn.py:241-289 over a `SubGraphDataset` as ONE captured HIP graph: the fixed-shape buffers and
    slot logic of `ReplayedFreshStep`, and a step that runs under `torch.no_grad()` with the model in eval mode:
        ds.collate_padded(buf);  out = model(buf);  stats.update(out, buf.y, live=buf.live_edges, pos_weight=pos_weight)
    `out` are plain logits of all max_edges entries; those of the padded tail are whatever the decoder computes for the inert
    self loops and are never read (`metrics.EpochStats` takes the number of real edges from device memory).  So every decoder
    and width `model(buf)` supports in eval mode is served — `mlp` at any node_dim, `cosine`, `dot`, with or without
    `skip_connections` / `base_model` / `union_edge_weights` (buffers in the union layout, as for the training replay) — wider
    than the training replay.  Per batch the host does one id write and one graph launch; loss, confusion counts and the scores the
    ranking metrics need accumulate in `self.stats`, read out once by `compute()`.
    `ranking`: keep scores and labels for ROC-AUC / PR-AUC; the capacity is the edge total of `graphs` (default: all), i.e. one
    pass over that validation set between two `reset()`s.  `capture=False` runs the very same padded step eagerly.
    The model's `training` flag is as before after construction and after every call; parameters are never touched and no
    autograd graph is kept."""

    def __init__(self, model, ds, pos_weight, batch_size: int = 32, graphs=None, capture: bool = True, warmup: int = 1,
                 slack: float = 1.4, threshold: float = 0.5, ranking: bool = True):
        from .metrics import EpochStats
        dev = ds.edge_index.device
        if pos_weight is not None:       # the device scalar the captured launch reads: made once, never inside the capture
            pos_weight = torch.as_tensor(pos_weight).detach().to(device=dev, dtype=torch.float32).reshape(-1)[:1]
        self.model, self.pos_weight = model, pos_weight
        h = ds._host()
        idx = range(ds.num_graphs) if graphs is None else [int(i) for i in graphs]
        capacity = sum(h.edge[i + 1] - h.edge[i] for i in idx) if ranking else 0
        self.stats = EpochStats(capacity, threshold, device=ds.edge_index.device)
        self._init_slots(ds, batch_size, graphs, capture, warmup, slack)

    def _kept(self):
        return [self.stats.state]

    @torch.no_grad()
    def _step(self, buf):
        was_training = self.model.training
        self.model.eval()
        try:
            self.ds.collate_padded(buf)
            out = self.model(buf)
            self.stats.update(out, buf.y, live=buf.live_edges, pos_weight=self.pos_weight)
        finally:
            self.model.train(was_training)
        return (out,)

    def __call__(self, graph_ids):
        """evaluate the disjoint union of the sub-graphs `graph_ids` (host ints, any order, at most batch_size) and fold it into
        `self.stats`; returns the logits of the batch's real edges without synchronising — with capture a VIEW of the captured
        graph's static output, which the next call overwrites"""
        (out,), edges = self._run(graph_ids)
        return out[:edges]

    def compute(self) -> dict:
        return self.stats.compute()

    def reset(self):
        self.stats.reset()


def run_epoch(step, evaluator, train_ids, val_ids, batch_size: int = 32, generator=None) -> dict:
    """One epoch of the reference's loop (pangnn.py:180-322) over the two replayed objects: shuffle `train_ids`, replay the
    training batches (`step`: a ReplayedFreshStep built with `stats=`), replay the validation batches (`evaluator`: a
    ReplayedFreshEval), read out once.  Returns the reference's epoch scalars (pangnn.py:296-322):
    train_loss / train_acc / train_f1 and val_loss / val_acc / val_precision / val_recall / val_f1 / val_roc_auc / val_pr_auc."""
    if step.stats is None:
        raise ValueError("run_epoch needs ReplayedFreshStep(..., stats=EpochStats(...))")
    train_ids, val_ids = [int(i) for i in train_ids], [int(i) for i in val_ids]
    order = torch.randperm(len(train_ids), generator=generator).tolist()
    step.stats.reset()
    evaluator.reset()
    for k in range(0, len(order), batch_size):
        step([train_ids[j] for j in order[k:k + batch_size]])
    for k in range(0, len(val_ids), batch_size):
        evaluator(val_ids[k:k + batch_size])
    tr, va = step.stats.compute(), evaluator.compute()
    res = dict(train_loss=tr["loss"], train_acc=tr["accuracy"], train_f1=tr["f1"])
    res.update(val_loss=va["loss"], val_acc=va["accuracy"], val_precision=va["precision"], val_recall=va["recall"],
               val_f1=va["f1"])
    for k in ("roc_auc", "pr_auc"):
        if k in va:
            res["val_" + k] = va[k]
    return res
