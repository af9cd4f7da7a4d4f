"""Evaluation metrics of the link predictor, accumulated on the GPU.

The reference keeps three torchmetrics objects (pangnn.py:104-108,218-222,255-262,268-285):
`BinaryConfusionMatrix` (thresholded predictions), `BinaryAUROC` and `BinaryAveragePrecision` (exact,
`thresholds=None`: every distinct score is a threshold).  torchmetrics is a third-party package that is
not in the reference tree; the classes here keep its `update / compute / reset` protocol and the
definitions it documents, and tests pin them against scikit-learn (`confusion_matrix`, `roc_auc_score`,
`average_precision_score`), which implements the same definitions.

  * confusion counts: one HIP pass over the logits (sigmoid + threshold + 4 integer counters,
    `pangnn_confusion_update_f32`), no [E] probability / prediction tensors, no host sync per batch.
  * AUROC / average precision: scores and labels of all batches stay on the device; `compute()` is one
    descending sort + prefix sums in int64/float64 (ties share one threshold, as in both libraries).
"""
from __future__ import annotations

import weakref
from typing import Optional

import torch

from . import _lib


class BinaryConfusionMatrix:
    """[[tn, fp], [fn, tp]] (row = true label, column = prediction), int64 on the device."""

    def __init__(self, threshold: float = 0.5, device=None):
        self.threshold = float(threshold)
        self.counts = torch.zeros(4, dtype=torch.int64, device=device if device is not None else "cuda")

    def _launch(self, scores, target, threshold, apply_sigmoid):
        lib = _lib.load()
        _lib.require_device(scores, target)
        s = scores.detach().reshape(-1).to(torch.float32).contiguous()
        t = target.detach().reshape(-1).to(torch.float32).contiguous()
        if s.shape != t.shape:
            raise ValueError(f"{s.shape[0]} scores for {t.shape[0]} labels")
        if self.counts.device != s.device:
            self.counts = self.counts.to(s.device)
        with torch.cuda.device(s.device):
            _lib.check(lib.pangnn_confusion_update_f32(s.data_ptr(), t.data_ptr(), s.shape[0], float(threshold),
                                                       int(apply_sigmoid), self.counts.data_ptr(),
                                                       _lib.stream_ptr()), "pangnn_confusion_update_f32")

    def update_from_logits(self, logits, target, threshold: Optional[float] = None):
        """sigmoid(logits) >= threshold, counted in one pass (pangnn.py:219-222 without the temporaries)"""
        self._launch(logits, target, self.threshold if threshold is None else threshold, True)

    def update(self, preds, target):
        """torchmetrics signature: `preds` are 0/1 predictions (what pangnn.py:221 passes) or probabilities
        (thresholded at `self.threshold`)"""
        if preds.dtype.is_floating_point:
            self._launch(preds, target, self.threshold, False)
        else:
            self._launch(preds.to(torch.float32), target, 0.5, False)

    def compute(self) -> torch.Tensor:
        return self.counts.view(2, 2).clone()

    def reset(self):
        self.counts.zero_()


def summary_from_confusion(conf) -> dict:
    """pangnn.py:268-285: precision / recall / f1 / accuracy with the reference's 1e-10 guards"""
    tn, fp, fn, tp = (float(v) for v in conf.reshape(-1).tolist())
    precision = tp / (tp + fp + 1e-10)
    recall = tp / (tp + fn + 1e-10)
    f1 = 2 * (precision * recall) / (precision + recall + 1e-10)
    total = tp + tn + fp + fn
    return dict(tn=int(tn), fp=int(fp), fn=int(fn), tp=int(tp), precision=precision, recall=recall, f1=f1,
                accuracy=(tp + tn) / total if total else 0.0)


class _RankingMetric:
    """keeps (score, label) of every update on the device, like torchmetrics with thresholds=None.
    `share_curve_with=other`: the two metrics are going to be fed the same tensors (ROC-AUC and PR-AUC of one validation pass,
    pangnn.py:255-285) — whichever computes second reuses the sorted curve of the first instead of sorting the 7.5e7 scores of
    config 4 again (the sort is most of the pass).  The curve lives on the metric objects and goes with them."""

    def __init__(self, share_curve_with=None):
        self.scores, self.labels, self._src, self._curve_kept = [], [], [], None
        self._partner = None if share_curve_with is None else weakref.ref(share_curve_with)     # weak both ways: no cycle
        if share_curve_with is not None:
            share_curve_with._partner = weakref.ref(self)

    def update(self, preds, target):
        self.scores.append(preds.detach().reshape(-1).to(torch.float32))
        self.labels.append((target.detach().reshape(-1) > 0.5))
        self._src.append((preds, target, preds._version, target._version))
        self._curve_kept = None

    def reset(self):
        self.scores, self.labels, self._src, self._curve_kept = [], [], [], None

    def _same_data(self, other) -> bool:
        return len(self._src) == len(other._src) and all(
            a[0] is b[0] and a[1] is b[1] and a[2] == b[2] and a[3] == b[3] for a, b in zip(self._src, other._src))

    def _curve(self):
        """(tps, fps, thresholds) at every distinct threshold, scores descending; tps / fps int64, thresholds the scores"""
        if self._curve_kept is None:
            p = None if self._partner is None else self._partner()
            if p is not None and p._curve_kept is not None and self._same_data(p):
                self._curve_kept = p._curve_kept
            else:
                self._curve_kept = self._curve_of(torch.cat(self.scores), torch.cat(self.labels))
        return self._curve_kept

    @staticmethod
    def _curve_of(s, y):
        s, order = torch.sort(s, descending=True, stable=True)
        y = y[order].to(torch.int64)
        n = s.shape[0]
        last = torch.ones(n, dtype=torch.bool, device=s.device)
        last[:-1] = s[1:] != s[:-1]                       # last element of each run of equal scores
        idx = torch.nonzero(last).view(-1)
        tps = torch.cumsum(y, 0)[idx]
        fps = idx + 1 - tps
        return tps, fps, s[idx]


class BinaryAUROC(_RankingMetric):
    """area under the ROC curve by the trapezoidal rule over all distinct thresholds; 0 if one class is absent
    (torchmetrics returns 0 with a warning there)"""

    def compute(self) -> torch.Tensor:
        if not self.scores or sum(t.numel() for t in self.scores) == 0:
            return torch.zeros((), dtype=torch.float32)
        tps, fps, _ = self._curve()
        p, n = tps[-1], fps[-1]
        if int(p) == 0 or int(n) == 0:
            return torch.zeros((), dtype=torch.float32, device=tps.device)
        z = torch.zeros(1, dtype=torch.float64, device=tps.device)
        tpr = torch.cat([z, tps.double() / p.double()])
        fpr = torch.cat([z, fps.double() / n.double()])
        return torch.trapezoid(tpr, fpr).to(torch.float32)

    def optimal_threshold(self) -> torch.Tensor:
        """Youden threshold of the kept curve (no second sort): see `youden_threshold`"""
        if not self.scores or sum(t.numel() for t in self.scores) == 0:
            return torch.full((), float("inf"), dtype=torch.float32)
        return _youden(*self._curve())


class BinaryAveragePrecision(_RankingMetric):
    """AP = sum_k (R_k - R_{k-1}) P_k over distinct thresholds (no interpolation)"""

    def compute(self) -> torch.Tensor:
        if not self.scores or sum(t.numel() for t in self.scores) == 0:
            return torch.zeros((), dtype=torch.float32)
        tps, fps, _ = self._curve()
        p = tps[-1]
        if int(p) == 0:
            return torch.zeros((), dtype=torch.float32, device=tps.device)
        precision = tps.double() / (tps + fps).double()
        recall = tps.double() / p.double()
        prev = torch.cat([torch.zeros(1, dtype=torch.float64, device=tps.device), recall[:-1]])
        return ((recall - prev) * precision).sum().to(torch.float32)


def _youden(tps, fps, thr) -> torch.Tensor:
    dev = tps.device
    m = tps.numel()
    # sklearn's drop_intermediate: of the curve's points keep the first, the last and every point where the second difference
    # of fps or tps is non-zero.  The dropped points are not argmax candidates: in exact arithmetic they never hold the first
    # maximum, but in float64 a point inside a flat collinear run can round one ulp above the run's first point.
    keep = torch.ones(m, dtype=torch.bool, device=dev)
    if m > 2:
        keep[1:-1] = ((tps[2:] - 2 * tps[1:-1] + tps[:-2]) != 0) | ((fps[2:] - 2 * fps[1:-1] + fps[:-2]) != 0)
    p, n = tps[-1].double(), fps[-1].double()
    z = torch.zeros(1, dtype=torch.float64, device=dev)
    j = torch.cat([z, tps.double() / p - fps.double() / n])               # leading point (0, 0) at threshold inf
    j = torch.where(torch.cat([keep.new_ones(1), keep]), j, torch.full_like(j, -float("inf")))
    # one class absent: sklearn's tpr or fpr is 0/0 = NaN and numpy's argmax takes the first NaN, the leading point
    k = torch.where(torch.isnan(j).any(), torch.zeros((), dtype=torch.int64, device=dev), torch.argmax(j))
    t = torch.cat([torch.full((1,), float("inf"), dtype=thr.dtype, device=dev), thr])
    return t[k]


def youden_threshold(scores, target) -> torch.Tensor:
    """thresholds[argmax(tpr - fpr)] of sklearn.metrics.roc_curve(target, scores) (src/plot.py:103-105, what plot_roc
    returns as stats['optimatl_threshold'] and --dynamic_binary_threshold sets): the FIRST maximum, on a curve whose leading
    point is (0, 0) at threshold inf — so inf when no score gives tpr - fpr > 0 or one class is absent.  The argmax runs over
    the points sklearn keeps (its default drop_intermediate rule), so float64 rounding inside a collinear run picks what
    sklearn picks.
    A 0-d float32 tensor on the device of `scores` (float32 scores, as the ranking metrics keep them)."""
    m = BinaryAUROC()
    m.update(scores, target)
    return m.optimal_threshold()


class EpochStats:
    """What an epoch keeps of its batches' logits, as device state that ONE capturable launch per batch adds to
    (`pangnn_batch_stats_f32`, csrc/batch_stats.hip): the confusion counts at a device-resident threshold, the sum of the
    batches' mean BCEWithLogits(pos_weight) losses and their number, and — `capacity > 0` — the raw logits and labels of every
    real edge, from which ROC-AUC, PR-AUC and the Youden threshold are computed once at the end (pangnn.py:218-222: the
    running training loss and confusion matrix; pangnn.py:241-289: the validation loop).  The batch may be a padded
    fixed-shape one (`live`: the device count of its real edges), and `update` reads nothing back, so it can end the
    captured step of `train.ReplayedFreshStep` / `train.ReplayedFreshEval`.

    State: `state`, int64[16] — counts[4] (index 2*label + prediction), batches, cursor, overflow, loss_sum (float64),
    last_loss (float32) and the threshold (float32), all in one allocation with the kernel's partials behind them — plus the
    two ranking buffers `scores` float32[capacity] / `labels` uint8[capacity].  Logits are stored, not probabilities: the
    appended data is an exact copy of what the model returned, and the sigmoid is applied once in `compute()`.
    A batch without a real edge adds nothing and is not counted (torch's mean over no element is NaN).  A batch that does not
    fit the ranking buffers is not appended and sets `overflow` (its counts and loss are still taken): `compute()` raises.

    CPU tensors run the same definition in plain torch (prediction `torch.sigmoid(x) >= threshold`, loss the float64
    `binary_cross_entropy_with_logits` of the real entries)."""

    WORDS = 16                 # PANGNN_BATCH_STATS_WORDS
    _ZEROED = 9                # words reset() clears: everything but the threshold

    def __init__(self, capacity: int = 0, threshold: float = 0.5, device=None):
        dev = torch.device("cuda" if device is None else device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.capacity = int(capacity)
        if self.capacity < 0:
            raise ValueError("capacity must be >= 0")
        self._ws_bytes = int(_lib.load().pangnn_batch_stats_workspace_bytes(1 << 30)) if dev.type == "cuda" else 0
        whole = torch.zeros(self.WORDS + self._ws_bytes // 8, dtype=torch.int64, device=dev)
        self.state, self._workspace = whole[:self.WORDS], whole[self.WORDS:]
        self.counts = self.state[:4]
        f32 = self.state[8:10].view(torch.float32)
        self._loss_sum, self._last_loss, self._threshold = self.state[7:8].view(torch.float64), f32[0:1], f32[2:3]
        self.scores = torch.zeros(self.capacity, dtype=torch.float32, device=dev)
        self.labels = torch.zeros(self.capacity, dtype=torch.uint8, device=dev)
        self.set_threshold(threshold)

    # 0-d views of the state: reading one of them on the host is a synchronisation
    batches = property(lambda self: self.state[4])
    cursor = property(lambda self: self.state[5])
    overflow = property(lambda self: self.state[6])
    loss_sum = property(lambda self: self._loss_sum[0])
    last_loss = property(lambda self: self._last_loss[0])
    device = property(lambda self: self.state.device)

    def set_threshold(self, t: float):
        """writes the device scalar the next update reads (pangnn.py's --dynamic_binary_threshold): one fill on the current
        stream, no re-capture"""
        self.threshold = float(t)
        self._threshold.fill_(self.threshold)

    def reset(self):
        self.state[:self._ZEROED].zero_()

    def _scalar(self, v, dtype):
        """a 1-element tensor of `dtype` on the state's device, or None"""
        if v is None:
            return None
        if not torch.is_tensor(v):
            return torch.tensor([v], dtype=dtype, device=self.device)
        v = v.detach().reshape(-1)[:1]
        return v if (v.dtype == dtype and v.device == self.device) else v.to(device=self.device, dtype=dtype)

    def update(self, logits, labels, live=None, pos_weight=None, loss=None):
        """fold one batch in: `logits` / `labels` [n_max], of which the first `live[0]` are real (a device int64 tensor, as a
        padded batch carries it; None: all).  `pos_weight`: the loss's positive weight; `loss`: the batch's loss where the
        caller already has it (then none is computed).  One launch on the current stream; nothing is read back."""
        x, y = logits.detach().reshape(-1), labels.detach().reshape(-1)
        if x.shape != y.shape:
            raise ValueError(f"{x.shape[0]} logits for {y.shape[0]} labels")
        if x.device != self.device or y.device != self.device:
            raise ValueError(f"EpochStats on {self.device} got a batch on {x.device}")
        x, y = x.to(torch.float32).contiguous(), y.to(torch.float32).contiguous()
        live, pw, loss = self._scalar(live, torch.int64), self._scalar(pos_weight, torch.float32), self._scalar(loss, torch.float32)
        if not x.is_cuda:
            return self._update_host(x, y, live, pw, loss)
        with _lib.device_guard(x.device):
            _lib.check(_lib.load().pangnn_batch_stats_f32(
                x.data_ptr(), y.data_ptr(), x.shape[0], _lib.ptr(live), _lib.ptr(pw), self._threshold.data_ptr(), _lib.ptr(loss),
                self.state.data_ptr(), _lib.ptr(self.scores) if self.capacity else None,
                _lib.ptr(self.labels) if self.capacity else None, self.capacity, self._workspace.data_ptr(), self._ws_bytes,
                _lib.stream_ptr()), "pangnn_batch_stats_f32")

    def _update_host(self, x, y, live, pw, loss):
        n = x.shape[0]
        m = n if live is None else int(live[0])
        m = n if (m < 0 or m > n) else m
        if m == 0:
            return
        xs, lab = x[:m], y[:m] > 0.5
        pred = torch.sigmoid(xs) >= self._threshold
        self.counts += torch.bincount(2 * lab.to(torch.int64) + pred.to(torch.int64), minlength=4)
        if loss is None:
            one = torch.nn.functional.binary_cross_entropy_with_logits(
                xs.double(), y[:m].double(), pos_weight=None if pw is None else pw.double())
        else:
            one = loss[0].double()
        self._loss_sum += one
        self._last_loss.copy_(one.float() if loss is None else loss[:1])
        self.state[4] += 1
        if self.capacity:
            c = int(self.state[5])
            if 0 <= c and c + m <= self.capacity:
                self.scores[c:c + m] = xs
                self.labels[c:c + m] = lab.to(torch.uint8)
                self.state[5] = c + m
            else:
                self.state[6] = 1

    def confusion(self) -> torch.Tensor:
        """[[tn, fp], [fn, tp]] int64, as BinaryConfusionMatrix.compute"""
        return self.counts.view(2, 2).clone()

    def _ranking(self, cursor: int):
        """(BinaryAUROC, BinaryAveragePrecision) fed ONCE with the collected probabilities: one sort serves both"""
        auroc = BinaryAUROC()
        ap = BinaryAveragePrecision(share_curve_with=auroc)
        prob, lab = torch.sigmoid(self.scores[:cursor]), self.labels[:cursor]
        auroc.update(prob, lab)
        ap.update(prob, lab)
        return auroc, ap

    def compute(self) -> dict:
        """the keys of `train.evaluate`: the confusion summary, `loss` = loss_sum / batches and — with ranking data —
        `roc_auc` / `pr_auc`.  The only host read-out."""
        import struct
        st = self.state.tolist()
        if st[6]:
            raise RuntimeError(f"EpochStats: a batch did not fit the {self.capacity} ranking entries (overflow); size the "
                               f"capacity to the pass and reset()")
        if st[4] == 0:
            raise ValueError("EpochStats.compute() needs at least one counted batch")
        res = summary_from_confusion(torch.tensor(st[:4], dtype=torch.int64))
        res["loss"] = struct.unpack("<d", struct.pack("<q", st[7]))[0] / st[4]
        if self.capacity:
            auroc, ap = self._ranking(st[5])
            res.update(roc_auc=float(auroc.compute()), pr_auc=float(ap.compute()))
        return res

    def optimal_threshold(self) -> torch.Tensor:
        """Youden threshold of the collected scores (`youden_threshold` of their probabilities): what
        --dynamic_binary_threshold feeds back into `set_threshold`"""
        if not self.capacity:
            raise ValueError("EpochStats(capacity=0) keeps no scores")
        if int(self.state[6]):
            raise RuntimeError("EpochStats: overflow")
        return self._ranking(int(self.state[5]))[0].optimal_threshold()
