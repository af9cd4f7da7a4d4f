"""predict_homolog_genes (src/predict.py:12-130): the inference pass that produces the tool's answer, with its metrics.

The reference runs the model under no_grad, copies the probabilities to the host and computes the statistics with
sklearn, the max-logit-candidate baseline with Python dict loops in a multiprocessing.Pool, and draws plots.  Here every
statistic is computed on the device — confusion counts, ROC-AUC, average precision and the Youden threshold from one
sorted curve, the max-candidate labelling in one HIP pass with its confusion counts fused (csrc/candidates.hip) — and the
results are read back to the host in one copy at the end.  That is not the only synchronisation: the ranking metrics
check their class counts on the host, the curve's run boundaries come from torch.nonzero, and building a segment
structure (first call per graph) syncs too.  No plots, no files.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from .candidates import best_candidate
from .metrics import BinaryAUROC, BinaryAveragePrecision, BinaryConfusionMatrix


def _div(a: float, b: float) -> float:
    return a / b if b else math.nan          # numpy's 0 / 0 of the reference: NaN (with a warning there)


def _graphs(ds):
    if ds is None:
        return []
    return list(ds) if isinstance(ds, (list, tuple)) else [ds]


def _as_device_labels(lab, device) -> torch.Tensor:
    t = lab if isinstance(lab, torch.Tensor) else torch.as_tensor(lab)
    return t.to(device=device).reshape(-1)


def _counts_of(pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """int64 [tn, fp, fn, tp] of 0/1 predictions against 0/1 labels, on the device"""
    return torch.bincount(2 * (y > 0.5).to(torch.int64) + (pred > 0.5).to(torch.int64), minlength=4)


def _candidate_summary(c) -> dict:
    """precision / recall / f1 of one max-candidate labelling, as sklearn's precision_score / recall_score / f1_score
    report them in plot_pr_curve (src/plot.py:148-170): 0 where a denominator is 0 (sklearn's zero_division default)"""
    tn, fp, fn, tp = c
    precision = tp / (tp + fp) if tp + fp else 0.0
    recall = tp / (tp + fn) if tp + fn else 0.0
    f1 = 2 * tp / (2 * tp + fp + fn) if tp else 0.0
    return dict(precision=precision, recall=recall, f1=f1)


def predict_homolog_genes(model, train_dataset=None, test_dataset=None, binary_th: float = 0.72, base_labels=None,
                          refined_base_labels=None, dataset=None):
    """Infer the model on `test_dataset` and compute the reference's statistics (src/predict.py:12-130).

    Returns (binary_prediction, edge_scores, stats) like the reference: binary_prediction = int32 (sigmoid(logits) >=
    binary_th) and the logits, both on the model's device.  When the test graph has labels `y`, `stats` holds the
    reference's keys (typos included): auc_test, optimatl_threshold (the Youden threshold of sklearn's roc_curve), tn, fp,
    fn, tp, average_precision, acc_test, acc_train (0 without a train set), precision, recall, specifity, f1 — plain
    Python numbers; a zero denominator gives NaN, and so does auc_test with one class absent, as in the reference.

    When the test graph or `dataset` carries `genome_of` (the node -> genome map of a whole graph), the reference's
    `not args.train or args.simulate_dataset` branch: stats['max_logit_candidate'] holds the precision / recall / f1 of
    the max-logit-candidate labels (candidates.best_candidate over the logits) and, when `base_labels` = (q_labels,
    raw_labels) is passed (tensors or lists, e.g. from candidates.candidate_baselines), stats['max_q_score_candidate'] /
    stats['max_raw_score_candidate'] those of the two given labelings (a None member is skipped).  `genome_of` may live on
    the host: the segment structure is cached on the caller's tensors.  Without `genome_of` (mini-batches of sub-graphs,
    whose nodes do not map back to genes) these keys are left out, as in the reference's sub-graph branch.

    `train_dataset`: a graph or a list of graphs; its accuracy at binary_th is stats['acc_train'].  `refined_base_labels`
    is accepted for signature compatibility and not used (the reference only plots it)."""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            edge_scores = model(test_dataset)
            graph = test_dataset[0] if isinstance(test_dataset, tuple) else test_dataset
            logits = edge_scores.detach().reshape(-1).float()
            prob = torch.sigmoid(logits)
            binary_prediction = (prob >= binary_th).int()
            stats = {}
            if not hasattr(graph, "y") or graph.y is None:
                return binary_prediction, edge_scores, stats
            dev = logits.device
            y = graph.y.reshape(-1)

            # train accuracy: correct predictions and edges over every train graph, on the device
            train_correct = torch.zeros((), dtype=torch.int64, device=dev)
            train_total = 0
            for g in _graphs(train_dataset):
                out = model(g).detach().reshape(-1).float()
                pred_tr = (torch.sigmoid(out) >= binary_th).int()
                train_correct += (pred_tr == g.y.reshape(-1).to(dev)).sum()
                train_total += pred_tr.numel()

            conf = BinaryConfusionMatrix(binary_th, device=dev)
            conf.update(binary_prediction, y)                       # counts the predictions returned, bit for bit
            auroc = BinaryAUROC()
            ap = BinaryAveragePrecision(share_curve_with=auroc)
            auroc.update(prob, y)
            ap.update(prob, y)
            parts = [conf.counts.double(), auroc.compute().double().reshape(1).to(dev),
                     ap.compute().double().reshape(1).to(dev), auroc.optimal_threshold().double().reshape(1).to(dev),
                     train_correct.double().reshape(1)]

            genome_of = getattr(graph, "genome_of", None)
            if genome_of is None and dataset is not None:
                genome_of = getattr(dataset, "genome_of", None)
            cand = []
            if genome_of is not None:
                counts = torch.zeros(4, dtype=torch.int64, device=dev)
                best_candidate(logits, graph.edge_index, genome_of, y=y, counts=counts)
                cand.append(("max_logit_candidate", counts))
                if base_labels is not None:
                    q_lab, raw_lab = base_labels
                    for name, lab in (("max_q_score_candidate", q_lab), ("max_raw_score_candidate", raw_lab)):
                        if lab is not None:                 # (q, None): candidate_baselines without a raw relation
                            cand.append((name, _counts_of(_as_device_labels(lab, dev), y)))
            parts += [c.double() for _, c in cand]
            host = torch.cat(parts).tolist()                        # the one read-out of the results

        tn, fp, fn, tp = (int(v) for v in host[0:4])
        auc, average_precision, opt_th, correct_train = host[4:8]
        total = tn + fp + fn + tp
        precision, recall = _div(tp, tp + fp), _div(tp, tp + fn)
        stats["auc_test"] = auc if (tp + fn) and (tn + fp) else math.nan
        stats["optimatl_threshold"] = opt_th
        stats["tn"], stats["fp"], stats["fn"], stats["tp"] = tn, fp, fn, tp
        stats["average_precision"] = average_precision
        stats["acc_test"] = _div(tp + tn, total)
        stats["acc_train"] = correct_train / train_total if train_total else 0
        stats["precision"] = precision
        stats["recall"] = recall
        stats["specifity"] = _div(tn, fp + tn)
        stats["f1"] = 2 * _div(precision * recall, precision + recall)
        for k, (name, _) in enumerate(cand):
            stats[name] = _candidate_summary([int(v) for v in host[8 + 4 * k:12 + 4 * k]])
        return binary_prediction, edge_scores, stats
    finally:
        model.train(was_training)
