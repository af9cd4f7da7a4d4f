"""Max-candidate labelling on the MI355X (csrc/candidates.hip) and predict_homolog_genes (src/predict.py:12-130).

The HIP labels are held to the reference's own labels (tests/golden/candidates_*.npz) bit for bit, and to the CPU path on
stress relations (many / few genomes, segments around the wave width and longer than 20 000 edges, +-inf, NaN, all-NaN
segments, duplicates, f32 / f64, the sorted fast path and the permuted general path), run twice for reproducibility.
predict_homolog_genes is held to sklearn on the same probabilities."""
import math
import warnings

import numpy as np
import pytest
import torch
from sklearn.metrics import average_precision_score, confusion_matrix, roc_auc_score, roc_curve

from conftest import load_golden

pytestmark = pytest.mark.gpu

CONFIGS = ["cfg1_2genomes", "cfg2_sim_1000x5", "cfg3_5genomes", "sim_200x4"]
KEYS = {"auc_test", "optimatl_threshold", "tn", "fp", "fn", "tp", "average_precision", "acc_test", "acc_train",
        "precision", "recall", "specifity", "f1"}
DEV = "cuda"


def _pc():
    from pangnn_amd import candidates
    return candidates


@pytest.mark.parametrize("name", CONFIGS)
def test_hip_labels_equal_reference_fixtures(name):
    pc = _pc()
    f, k = load_golden(name), load_golden(f"candidates_{name}")
    ei = torch.from_numpy(f["whole_edge_index"]).to(DEV)
    go = torch.from_numpy(f["genome_of"]).long().to(DEV)
    logit = pc.best_candidate(torch.from_numpy(k["logits"]).to(DEV), ei, go)
    q, raw = pc.candidate_baselines(ei, torch.from_numpy(f["whole_edge_attr"]).to(DEV), go,
                                    *(torch.from_numpy(f[x]).to(DEV) for x in ("raw_src", "raw_dst", "raw_score")))
    for got, want in ((logit, "labels_logit"), (q, "labels_q"), (raw, "labels_raw")):
        assert got.is_cuda and got.dtype == torch.bool
        np.testing.assert_array_equal(got.cpu().numpy().astype(np.uint8), k[want], err_msg=want)


def _relation(genomes, seg_lens, seed, dtype):
    """a relation sorted by (source, candidate genome) whose segments have the given lengths, with +-inf, NaN, all-NaN
    segments and duplicate values; returns (edge_index, genome_of, values) — canonical (fast path) order"""
    g = torch.Generator().manual_seed(seed)
    n_src = len(seg_lens)
    per = max(max(seg_lens), 1)
    nodes_per_genome = per + 1
    n = max(n_src, genomes * nodes_per_genome)
    genome_of = torch.arange(n) // nodes_per_genome
    genome_of = torch.where(genome_of < genomes, genome_of, genome_of % genomes)
    src, dst = [], []
    for s, ln in enumerate(seg_lens):
        tg = (s * 7) % genomes
        src.append(torch.full((ln,), s, dtype=torch.int64))
        dst.append(tg * nodes_per_genome + torch.arange(ln))
    src, dst = torch.cat(src), torch.cat(dst)
    e = src.numel()
    v = torch.round(torch.randn(e, generator=g, dtype=torch.float64) * 4) / 4          # duplicates
    r = torch.rand(e, generator=g)
    v[r < 0.01] = float("inf")
    v[(r >= 0.01) & (r < 0.02)] = -float("inf")
    v[(r >= 0.02) & (r < 0.05)] = float("nan")
    bounds = torch.cumsum(torch.tensor([0] + list(seg_lens)), 0)
    for k in range(0, len(seg_lens), 9):                                               # all-NaN segments
        v[bounds[k]:bounds[k + 1]] = float("nan")
    ei = torch.stack([src, dst])
    order = torch.argsort(src * (int(genome_of.max()) + 1) + genome_of[dst], stable=True)
    return ei[:, order], genome_of, v[order].to(dtype)


STRESS = [
    (1, [1, 63, 64, 65, 1, 2, 3, 128, 129]),
    (3, [5, 64, 63, 65, 1] * 40),
    (257, [2, 3, 4, 7, 31, 64, 65, 100] * 70),
    (5000, [1, 2, 3, 4, 5, 6, 7, 8] * 700),
    (3, [20_001, 3, 64, 25_000, 1]),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("case", range(len(STRESS)))
def test_hip_equals_cpu_and_repeats_on_stress_relations(case, dtype):
    pc = _pc()
    genomes, lens = STRESS[case]
    ei, go, v = _relation(genomes, lens, seed=case, dtype=dtype)
    want = pc.best_candidate(v, ei, go)
    p = torch.randperm(v.numel(), generator=torch.Generator().manual_seed(case))
    for e_i, vals, ref in ((ei, v, want), (ei[:, p].contiguous(), v[p].contiguous(), want[p])):     # fast, general path
        e_d, g_d, v_d = e_i.to(DEV), go.to(DEV), vals.to(DEV)
        seg = pc.build_segments(e_d, g_d)
        assert (seg.seg_edge is None) == (e_i is ei)
        a = pc.best_candidate(v_d, e_d, g_d)
        b = pc.best_candidate(v_d, e_d, g_d)
        assert torch.equal(a.cpu(), ref)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_relabelled_node_ids_take_the_general_path():
    """the same graph with node ids permuted: same labels edge for edge"""
    pc = _pc()
    ei, go, v = _relation(257, [2, 3, 64, 65, 7] * 50, seed=11, dtype=torch.float32)
    n = go.numel()
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3))
    ei2, go2 = perm[ei], torch.empty_like(go)
    go2[perm] = go
    a = pc.best_candidate(v.to(DEV), ei.to(DEV), go.to(DEV))
    assert pc.build_segments(ei2.to(DEV), go2.to(DEV)).seg_edge is not None
    b = pc.best_candidate(v.to(DEV), ei2.to(DEV), go2.to(DEV))
    assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
def test_fused_confusion_counts_equal_torch_and_accumulate(dtype):
    pc = _pc()
    ei, go, v = _relation(3, [5, 64, 63, 65, 1, 200] * 60, seed=5, dtype=dtype)
    y = (torch.rand(v.numel(), generator=torch.Generator().manual_seed(1)) < 0.3).float()
    p = torch.randperm(v.numel(), generator=torch.Generator().manual_seed(2))
    for e_i, vals, yy in ((ei, v, y), (ei[:, p], v[p], y[p])):
        e_d, g_d, v_d, y_d = e_i.to(DEV), go.to(DEV), vals.to(DEV), yy.to(DEV)
        counts = torch.zeros(4, dtype=torch.int64, device=DEV)
        lab = pc.best_candidate(v_d, e_d, g_d, y=y_d, counts=counts)
        want = torch.bincount(2 * y_d.long() + lab.long(), minlength=4)
        assert torch.equal(counts, want)
        assert torch.equal(lab, pc.best_candidate(v_d, e_d, g_d))
        pc.best_candidate(v_d, e_d, g_d, y=y_d, counts=counts)
        assert torch.equal(counts, 2 * want)


def _model_and_graph(train_steps=0):
    import pangnn_amd
    from pangnn_amd.simulate import simulate_graph
    from pangnn_amd.train import make_optimizer, train_step
    g = simulate_graph(2000, 10, 0.2, 10, 2, seed=0, device=DEV)
    torch.manual_seed(0)
    model = pangnn_amd.AlternateGCN(torch.device(DEV), None, False, dims=[64, 128])
    if train_steps:
        opt = make_optimizer(model)
        for _ in range(train_steps):
            train_step(model, opt, g, g.y, g.class_balance)
    return model, g


def test_predict_returns_the_reference_keys_with_and_without_genome_of():
    from pangnn_amd import predict_homolog_genes
    model, g = _model_and_graph()
    model.train()
    b, s, stats = predict_homolog_genes(model, None, g)
    assert model.training                                       # mode restored
    assert set(stats) == KEYS | {"max_logit_candidate"}
    assert set(stats["max_logit_candidate"]) == {"precision", "recall", "f1"}
    assert b.dtype == torch.int32 and b.shape == s.shape == g.y.shape
    q, _ = _pc().candidate_baselines(g.edge_index, g.edge_attr, g.genome_of)
    _, _, stats = predict_homolog_genes(model, g, g, base_labels=(q, q.cpu().tolist()))
    assert set(stats) == KEYS | {"max_logit_candidate", "max_q_score_candidate", "max_raw_score_candidate"}
    assert stats["acc_train"] == stats["acc_test"]
    gen = g.genome_of
    del g.genome_of
    _, _, stats = predict_homolog_genes(model, None, g, base_labels=(q, q))
    assert set(stats) == KEYS
    g.genome_of = gen


def test_predict_equals_sklearn_on_the_same_logits():
    from pangnn_amd import predict_homolog_genes
    pc = _pc()
    model, g = _model_and_graph(train_steps=20)
    model.eval()
    with torch.no_grad():
        p0 = torch.sigmoid(model(g).float()).cpu().numpy()
    th = float(np.float32(np.quantile(p0, 0.7)))            # both predictions occur; exact in float32 and float64
    b, scores, stats = predict_homolog_genes(model, None, g, binary_th=th)
    prob = torch.sigmoid(scores.float()).cpu().numpy()
    y = g.y.cpu().numpy()
    assert 0 < y.sum() < y.size and 0 < (prob >= th).sum() < y.size
    assert abs(stats["auc_test"] - roc_auc_score(y, prob)) < 1e-6                  # tests/test_metrics.py's tolerance
    assert abs(stats["average_precision"] - average_precision_score(y, prob)) < 1e-6
    pred = (prob >= th).astype(np.int32)
    np.testing.assert_array_equal(b.cpu().numpy(), pred)
    tn, fp, fn, tp = confusion_matrix(y, pred, labels=[0, 1]).ravel()
    assert (stats["tn"], stats["fp"], stats["fn"], stats["tp"]) == (tn, fp, fn, tp)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fpr, tpr, thr = roc_curve(y, prob)
    assert stats["optimatl_threshold"] == thr[np.argmax(tpr - fpr)]
    assert stats["acc_test"] == (tp + tn) / y.size
    assert stats["precision"] == tp / (tp + fp) and stats["recall"] == tp / (tp + fn)
    assert stats["specifity"] == tn / (fp + tn)
    p, r = tp / (tp + fp), tp / (tp + fn)
    assert math.isclose(stats["f1"], 2 * (p * r) / (p + r), rel_tol=1e-15)
    lab = pc.best_candidate(scores.float().cpu(), g.edge_index.cpu(), g.genome_of.cpu()).numpy()
    ltn, lfp, lfn, ltp = confusion_matrix(y, lab.astype(np.int32), labels=[0, 1]).ravel()
    mc = stats["max_logit_candidate"]
    assert mc["precision"] == ltp / (ltp + lfp) and mc["recall"] == ltp / (ltp + lfn)
    assert math.isclose(mc["f1"], 2 * ltp / (2 * ltp + lfp + lfn), rel_tol=1e-15)
    assert torch.equal(pc.best_candidate(scores, g.edge_index, g.genome_of).cpu(), torch.from_numpy(lab))   # HIP = CPU


def test_predict_zero_denominators_give_nan():
    from pangnn_amd import predict_homolog_genes
    model, g = _model_and_graph()
    _, _, stats = predict_homolog_genes(model, None, g, binary_th=2.0)           # nothing predicted positive
    assert stats["tp"] == stats["fp"] == 0
    assert math.isnan(stats["precision"]) and math.isnan(stats["f1"])
    with torch.no_grad():
        model.eval()
        prob = torch.sigmoid(model(g).float()).cpu().numpy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fpr, tpr, thr = roc_curve(g.y.cpu().numpy(), prob)
    assert stats["optimatl_threshold"] == thr[np.argmax(tpr - fpr)]


def test_predict_host_genome_of_reuses_one_segment_structure_and_skips_missing_raw_labels(monkeypatch):
    """genome_of kept on the host: the segment structure is built once for the caller's tensors, not once per call; the
    raw relation of candidate_baselines is not cached; base_labels = (q, None) leaves the raw-score key out"""
    from pangnn_amd import predict_homolog_genes
    pc = _pc()
    model, g = _model_and_graph()
    g.genome_of = g.genome_of.cpu()
    builds = []
    real = pc.build_segments
    monkeypatch.setattr(pc, "build_segments", lambda ei, go: (builds.append(1), real(ei, go))[1])
    pc.SEGMENTS.clear()
    _, _, a = predict_homolog_genes(model, None, g)
    _, _, b = predict_homolog_genes(model, None, g)
    assert len(builds) == 1 and a["max_logit_candidate"] == b["max_logit_candidate"]
    n_cached = len(pc.SEGMENTS.entries)
    src, dst = g.edge_index
    q, raw = pc.candidate_baselines(g.edge_index, g.edge_attr, g.genome_of, src, dst, g.edge_attr.double())
    assert len(pc.SEGMENTS.entries) == n_cached and len(builds) == 2                    # Q labels hit; raw built, not kept
    assert torch.equal(q, raw)                                                          # same relation, same labels
    q2, none = pc.candidate_baselines(g.edge_index, g.edge_attr, g.genome_of)
    assert none is None and torch.equal(q2, q)
    _, _, stats = predict_homolog_genes(model, None, g, base_labels=(q2, none))
    assert set(stats) == KEYS | {"max_logit_candidate", "max_q_score_candidate"}
