"""Max-candidate labelling and the Youden threshold on the CPU: the plain-torch path against labels computed by the
reference's own calculate_baseline_labels / find_max_logit (tests/golden/make_candidate_fixtures.py), the threshold
against sklearn, and the argument checks of the new C entry points (fake pointers, nothing launched)."""
import warnings

import numpy as np
import pytest
import torch
from sklearn.metrics import roc_curve

from conftest import load_golden
from pangnn_amd import _lib
from pangnn_amd.candidates import best_candidate, build_segments, candidate_baselines
from pangnn_amd.metrics import BinaryAUROC, youden_threshold

CONFIGS = ["cfg1_2genomes", "cfg2_sim_1000x5", "cfg3_5genomes", "sim_200x4"]


def _fixture(name):
    f, k = load_golden(name), load_golden(f"candidates_{name}")
    return f, k, torch.from_numpy(f["whole_edge_index"]), torch.from_numpy(f["genome_of"]).long()


@pytest.mark.parametrize("name", CONFIGS)
def test_cpu_logit_labels_match_reference(name):
    f, k, ei, go = _fixture(name)
    logits = torch.from_numpy(k["logits"])
    assert torch.isnan(logits).sum() == 1 and torch.isinf(logits).sum() == 6
    got = best_candidate(logits, ei, go).numpy().astype(np.uint8)
    np.testing.assert_array_equal(got, k["labels_logit"])


@pytest.mark.parametrize("raw", ["raw", "flt"])
@pytest.mark.parametrize("name", CONFIGS)
def test_cpu_q_and_raw_labels_match_reference(name, raw):
    """Q-score labels from the fp32 edge_attr (an fp32 tie the fp64 reference does not have would show here); raw-score
    labels from the raw relation before ("raw") and after ("flt") trivial-case removal, self hits included"""
    f, k, ei, go = _fixture(name)
    q, r = candidate_baselines(ei, torch.from_numpy(f["whole_edge_attr"]), go, torch.from_numpy(f[f"{raw}_src"]),
                               torch.from_numpy(f[f"{raw}_dst"]), torch.from_numpy(f[f"{raw}_score"]))
    np.testing.assert_array_equal(q.numpy().astype(np.uint8), k["labels_q"])
    np.testing.assert_array_equal(r.numpy().astype(np.uint8), k["labels_raw"])
    q_only, none = candidate_baselines(ei, torch.from_numpy(f["whole_edge_attr"]), go)
    assert none is None and torch.equal(q_only, q)


def test_cpu_semantics_on_a_hand_made_relation():
    nan, inf = float("nan"), float("inf")
    # node 0 -> genome 0; nodes 1..4 genome 1; nodes 5, 6 genome 2
    go = torch.tensor([0, 1, 1, 1, 1, 2, 2])
    src = torch.tensor([0, 0, 0, 0, 0, 0, 1, 1, 2, 3, 3])
    dst = torch.tensor([1, 2, 3, 4, 5, 6, 5, 6, 0, 5, 6])
    v = torch.tensor([1.0, 3.0, 3.0, nan, nan, nan, -inf, -inf, 2.0, 5.0, inf])
    want = torch.tensor([0, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1], dtype=torch.bool)   # ties 1, NaN 1, all-NaN 1, -inf tie 1
    for dtype in (torch.float32, torch.float64, torch.float16, torch.bfloat16):
        assert torch.equal(best_candidate(v.to(dtype), torch.stack([src, dst]), go), want)
    with pytest.raises(TypeError):
        best_candidate(torch.arange(src.numel()), torch.stack([src, dst]), go)      # integers: not silently rounded
    p = torch.randperm(src.numel(), generator=torch.Generator().manual_seed(0))
    assert torch.equal(best_candidate(v[p], torch.stack([src[p], dst[p]]), go), want[p])


def test_segment_structure_fast_and_general_path():
    go = torch.arange(12) // 4
    src = torch.tensor([0, 0, 0, 1, 1, 5, 5, 5, 5])
    dst = torch.tensor([4, 5, 9, 2, 3, 0, 1, 8, 10])
    s = build_segments(torch.stack([src, dst]), go)
    assert s.seg_edge is None and s.seg_rowptr.tolist() == [0, 2, 3, 5, 7, 9]
    p = torch.tensor([8, 3, 0, 5, 1, 7, 2, 6, 4])
    s = build_segments(torch.stack([src[p], dst[p]]), go)
    assert s.seg_rowptr.tolist() == [0, 2, 3, 5, 7, 9]
    assert s.seg_edge.dtype == torch.int32
    key = (src[p] * 3 + go[dst[p]])[s.seg_edge.long()]
    assert bool((key[1:] >= key[:-1]).all())


def _sk_youden(y, p):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fpr, tpr, th = roc_curve(y, p)
        return th[np.argmax(tpr - fpr)]


@pytest.mark.parametrize("seed", range(6))
def test_youden_threshold_matches_sklearn_with_heavy_ties(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(50, 3000))
    p = (rng.integers(0, int(rng.integers(2, 12)), n) / 11).astype(np.float32)
    y = (rng.random(n) < rng.uniform(0.05, 0.9)).astype(np.float32)
    y[0], y[1] = 0, 1
    got = float(youden_threshold(torch.from_numpy(p), torch.from_numpy(y)))
    assert got == _sk_youden(y, p)
    m = BinaryAUROC()                       # the method on a metric fed in two batches: same curve, same answer
    m.update(torch.from_numpy(p[: n // 2]), torch.from_numpy(y[: n // 2]))
    m.update(torch.from_numpy(p[n // 2:]), torch.from_numpy(y[n // 2:]))
    assert float(m.optimal_threshold()) == got


def test_youden_threshold_edge_cases_match_sklearn():
    rng = np.random.default_rng(7)
    y = (rng.random(500) < 0.3).astype(np.float32)
    same = np.full(500, 0.25, dtype=np.float32)
    assert float(youden_threshold(torch.from_numpy(same), torch.from_numpy(y))) == _sk_youden(y, same) == np.inf
    p = rng.random(500).astype(np.float32)
    for one_class in (np.zeros(500, np.float32), np.ones(500, np.float32)):
        assert float(youden_threshold(torch.from_numpy(p), torch.from_numpy(one_class))) == _sk_youden(one_class, p) == np.inf
    inverse = (1.0 - y).astype(np.float32) * 0.5 + 0.25          # every positive scores below every negative
    assert float(youden_threshold(torch.from_numpy(inverse), torch.from_numpy(y))) == _sk_youden(y, inverse) == np.inf
    assert float(BinaryAUROC().optimal_threshold()) == np.inf


def _collinear_case(top, runs, bottom_pos, bottom_neg):
    """`top` positives at 1.0, then `runs` thresholds holding one positive and one negative each, then a bottom tie"""
    p = [1.0] * top + [x for r in range(runs) for x in (0.9 - 0.1 * r,) * 2] + [0.05] * (bottom_pos + bottom_neg)
    y = [1] * top + [1, 0] * runs + [1] * bottom_pos + [0] * bottom_neg
    return np.array(p, dtype=np.float32), np.array(y, dtype=np.float32)


def test_youden_threshold_follows_sklearns_dropped_points():
    """inside a flat collinear run tpr - fpr can round one ulp above the run's first point in float64 (4/10 - 1/10 >
    3/10): sklearn's roc_curve has dropped those points, so its argmax stays on the first one"""
    p, y = _collinear_case(3, 4, 3, 6)
    assert float(youden_threshold(torch.from_numpy(p), torch.from_numpy(y))) == _sk_youden(y, p) == 1.0
    for top in range(1, 8):
        for runs in range(2, 8):
            for bp, bn in ((0, 3), (2, 5), (top, top + runs), (5, 2)):
                p, y = _collinear_case(top, runs, bp, bn)
                assert float(youden_threshold(torch.from_numpy(p), torch.from_numpy(y))) == _sk_youden(y, p), (top, runs, bp, bn)


F = 0x7f0000100000
E_BADARG, E_TOOLARGE = -1, -2


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: only where a missing check cannot reach a GPU")
@pytest.mark.parametrize("name", ["pangnn_best_candidate_f32", "pangnn_best_candidate_f64"])
def test_best_candidate_entry_points_refuse_bad_arguments(name):
    fn = getattr(_lib.load(), name)
    S, E = 1000, 5000
    assert fn(None, None, S, E, F, None, None, F, None) == E_BADARG            # null rowptr
    assert fn(F, None, S, E, None, None, None, F, None) == E_BADARG            # null values
    assert fn(F, None, S, E, F, None, None, None, None) == E_BADARG            # null labels
    assert fn(F, None, -1, E, F, None, None, F, None) == E_BADARG              # negative sizes
    assert fn(F, None, S, -1, F, None, None, F, None) == E_BADARG
    assert fn(F, None, S, E, F, None, F, F, None) == E_BADARG                  # counts without y
    assert fn(F, None, S, E, F, F, None, F, None) == E_BADARG                  # y without counts
    assert fn(F, None, 0, E, F, None, None, F, None) == E_BADARG               # edges in no segment
    assert fn(F, None, E + 1, E, F, None, None, F, None) == E_BADARG           # more segments than edges
    assert fn(F, F, S, 1 << 31, F, None, None, F, None) == E_TOOLARGE          # int32 seg_edge cannot address it
    assert name in _lib.load().pangnn_last_error().decode()
    assert fn(None, None, 0, 0, None, None, None, None, None) == 0             # empty relation: nothing to do
