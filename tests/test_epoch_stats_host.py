"""metrics.EpochStats and pangnn_batch_stats_f32 (csrc/batch_stats.hip), the part that needs no GPU: the entry point's argument
checks (fake pointers, nothing launched) and the CPU definition of EpochStats — what the kernel is held to in
tests/test_replayed_eval.py — against scikit-learn and torch's float64 loss.

`stats_inputs` (seeded logits kept away from the threshold's logit, labels, a poisoned tail) is defined here and imported by the
GPU file."""
import math

import pytest
import sklearn.metrics as sk
import torch
import torch.nn.functional as F

from pangnn_amd import _lib
from pangnn_amd.metrics import EpochStats, youden_threshold

FAKE = 0x7f0000100000          # a fake device pointer, 16-byte aligned
E_BADARG, E_WORKSPACE = -1, -3
N_MAX = (1, 65, 257, 5000)


def lives(n_max):
    return sorted({None, 0, 1, n_max // 2, n_max}, key=lambda v: -1 if v is None else v)


GRID = [(n, lv) for n in N_MAX for lv in lives(n)]


def grid_id(v):
    return f"n{v[0]}-live{v[1]}"


def stats_inputs(n_max, live, threshold=0.5, seed=0):
    """(logits, labels, m): a seeded 3 randn with every entry closer than 1e-3 to the threshold's logit moved away (no
    comparison rests on an ulp of the sigmoid); the tail behind `live` holds label 1 and logit +30, so that reading it shows"""
    gen = torch.Generator().manual_seed(1000 * n_max + 7 * (0 if live is None else live + 1) + seed)
    x = 3 * torch.randn(n_max, generator=gen)
    y = (torch.rand(n_max, generator=gen) < 0.3).float()
    cut = math.log(threshold / (1 - threshold))
    near = (x - cut).abs() < 1e-3
    x = torch.where(near, torch.full_like(x, cut + 0.01), x)
    m = n_max if live is None else live
    x[m:], y[m:] = 30.0, 1.0
    return x, y, m


def reference(x, y, m, threshold, pw):
    """(confusion counts [tn, fp, fn, tp] by scikit-learn, float64 loss) of the first m entries"""
    xs, ys = x[:m], y[:m]
    pred = (torch.sigmoid(xs) >= threshold).long()
    conf = sk.confusion_matrix(ys.long().numpy(), pred.numpy(), labels=[0, 1]).reshape(-1).tolist()
    # (pos_weight is a float32 scalar, as every loss kernel here takes it: the float64 loss is that of its float32 value)
    loss = F.binary_cross_entropy_with_logits(xs.double(), ys.double(),
                                              pos_weight=None if pw is None else torch.tensor(pw, dtype=torch.float32).double())
    return conf, float(loss)


# ------------------------------------------------------------------------------------------------------------------
# (a) the host half of the entry point
# ------------------------------------------------------------------------------------------------------------------
def _call(lib, **kw):
    a = dict(logits=FAKE, labels=FAKE, n_max=1000, live=FAKE, pw=None, th=FAKE, loss_in=None, state=FAKE, scores=FAKE,
             slabels=FAKE, cap=4000, ws=None, ws_bytes=0)
    a.update(kw)
    return lib.pangnn_batch_stats_f32(a["logits"], a["labels"], a["n_max"], a["live"], a["pw"], a["th"], a["loss_in"], a["state"],
                                      a["scores"], a["slabels"], a["cap"], a["ws"], a["ws_bytes"], None)


def test_abi_version_is_unchanged():
    assert _lib.load().pangnn_abi_version() == 3 == _lib.ABI_VERSION


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: only where a missing check cannot reach a GPU")
def test_entry_point_refuses_bad_arguments():
    """every call fails a check, so nothing is launched"""
    lib = _lib.load()
    for k in ("logits", "labels", "state", "th"):
        assert _call(lib, **{k: None}) == E_BADARG, k
    assert b"pangnn_batch_stats_f32" in lib.pangnn_last_error()
    assert _call(lib, n_max=-1) == E_BADARG
    assert _call(lib, cap=-1) == E_BADARG
    assert _call(lib, cap=-1, scores=None, slabels=None) == E_BADARG
    assert _call(lib, scores=None) == E_BADARG and _call(lib, slabels=None) == E_BADARG     # a capacity without its buffers
    assert _call(lib, logits=None, n_max=0) == E_BADARG                                     # the empty batch is checked too
    assert _call(lib, n_max=-1, state=None) == E_BADARG
    # above the one-workgroup limit the partials need their workspace: refused before the launch as well
    limit = 16384
    assert lib.pangnn_batch_stats_workspace_bytes(limit) == 0
    need = lib.pangnn_batch_stats_workspace_bytes(limit + 1)
    assert need > 0 and need == lib.pangnn_batch_stats_workspace_bytes(1 << 30)
    assert _call(lib, n_max=limit + 1) == E_WORKSPACE
    assert _call(lib, n_max=limit + 1, ws=FAKE, ws_bytes=need - 1) == E_WORKSPACE
    assert _call(lib, n_max=limit + 1, ws=FAKE, ws_bytes=-1) == E_WORKSPACE
    assert _call(lib, n_max=limit + 1, ws=FAKE, ws_bytes=need, logits=None) == E_BADARG     # null pointers first
    assert _call(lib, n_max=1 << 40, ws=FAKE, ws_bytes=need) == -2
    assert _call(lib, n_max=0) == 0                                                        # nothing to do, nothing launched


# ------------------------------------------------------------------------------------------------------------------
# (b) the CPU definition
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GRID, ids=grid_id)
@pytest.mark.parametrize("pw", [None, 4.3])
def test_cpu_definition_against_sklearn_and_float64_loss(case, pw):
    n_max, live = case
    th = 0.5 if pw is None else 0.72
    x, y, m = stats_inputs(n_max, live, th)
    s = EpochStats(capacity=2 * n_max + 3, threshold=th, device="cpu")
    s.scores.fill_(-7.0)
    s.labels.fill_(9)
    lv = None if live is None else torch.tensor([live])
    s.update(x, y, live=lv, pos_weight=pw)
    if m == 0:                                                          # skipped: nothing added, not counted
        assert s.state[:9].tolist() == [0] * 9 and bool((s.scores == -7).all()) and bool((s.labels == 9).all())
        with pytest.raises(ValueError):
            s.compute()
        return
    conf, loss = reference(x, y, m, th, pw)
    assert s.counts.tolist() == conf and s.confusion().tolist() == [conf[:2], conf[2:]]
    assert abs(float(s.loss_sum) - loss) <= 1e-12 * max(1.0, abs(loss)) and int(s.batches) == 1
    assert float(s.last_loss) == float(torch.tensor(loss).float())
    assert int(s.cursor) == m and int(s.overflow) == 0
    assert torch.equal(s.scores[:m], x[:m]) and torch.equal(s.labels[:m], (y[:m] > 0.5).to(torch.uint8))
    assert bool((s.scores[m:] == -7).all()) and bool((s.labels[m:] == 9).all())              # behind the cursor: untouched

    # a second update accumulates behind the first
    x2, y2, _ = stats_inputs(n_max, live, th, seed=1)
    s.update(x2, y2, live=lv, pos_weight=pw)
    conf2, loss2 = reference(x2, y2, m, th, pw)
    assert s.counts.tolist() == [a + b for a, b in zip(conf, conf2)]
    assert abs(float(s.loss_sum) - (loss + loss2)) <= 1e-12 * max(1.0, loss + loss2) and int(s.batches) == 2
    assert int(s.cursor) == 2 * m and torch.equal(s.scores[m:2 * m], x2[:m])
    res = s.compute()
    assert abs(res["loss"] - (loss + loss2) / 2) <= 1e-12 * max(1.0, loss)
    assert (res["tn"], res["fp"], res["fn"], res["tp"]) == tuple(s.counts.tolist())
    allx, ally = torch.cat([x[:m], x2[:m]]), torch.cat([y[:m], y2[:m]])
    prob = torch.sigmoid(allx)
    if 0 < int(ally.sum()) < ally.numel():
        assert abs(res["roc_auc"] - sk.roc_auc_score(ally.numpy(), prob.numpy())) <= 1e-6
        assert abs(res["pr_auc"] - sk.average_precision_score(ally.numpy(), prob.numpy())) <= 1e-6
    assert torch.equal(s.optimal_threshold(), youden_threshold(prob, ally))

    # reset() clears everything but the threshold
    s.reset()
    assert s.state[:9].tolist() == [0] * 9 and float(s._threshold) == float(torch.tensor(th).float())
    s.update(x, y, live=lv, pos_weight=pw)
    assert s.counts.tolist() == conf and int(s.cursor) == m


def test_given_loss_is_taken_verbatim():
    x, y, m = stats_inputs(257, 100)
    s = EpochStats(capacity=0, device="cpu")
    given = [torch.tensor(0.1234567), torch.tensor(3.25), torch.tensor(1e-3)]
    for g in given:
        s.update(x, y, live=torch.tensor([100]), loss=g)
    assert float(s.loss_sum) == sum(float(g) for g in given) and int(s.batches) == 3       # f64 sum of the f32 values: exact
    assert float(s.last_loss) == float(given[-1])
    assert s.counts.tolist() == [3 * c for c in reference(x, y, m, 0.5, None)[0]]
    res = s.compute()
    assert "roc_auc" not in res and "pr_auc" not in res                                      # capacity 0: no ranking data
    with pytest.raises(ValueError):
        s.optimal_threshold()
    s.update(x, y, live=torch.tensor([0]), loss=torch.tensor(5.0))                            # an empty batch: its loss is not counted
    assert int(s.batches) == 3 and float(s.last_loss) == float(given[-1])


def test_live_outside_the_batch_means_all_of_it():
    x, y, _ = stats_inputs(65, None)
    for lv in (-1, 66, 1 << 40):
        s = EpochStats(capacity=65, device="cpu")
        s.update(x, y, live=torch.tensor([lv]))
        assert int(s.cursor) == 65 and s.counts.tolist() == reference(x, y, 65, 0.5, None)[0]


def test_overflow_appends_nothing_and_compute_raises():
    x, y, m = stats_inputs(257, 200)
    s = EpochStats(capacity=300, device="cpu")
    s.scores.fill_(-7.0)
    s.update(x, y, live=torch.tensor([200]))
    assert int(s.cursor) == 200 and int(s.overflow) == 0
    kept = s.scores.clone()
    s.update(x, y, live=torch.tensor([200]))                                                 # 400 > 300
    assert int(s.cursor) == 200 and int(s.overflow) == 1 and torch.equal(s.scores, kept)
    conf, loss = reference(x, y, m, 0.5, None)
    assert s.counts.tolist() == [2 * c for c in conf] and int(s.batches) == 2               # counts and loss are still taken
    assert abs(float(s.loss_sum) - 2 * loss) <= 1e-12
    with pytest.raises(RuntimeError):
        s.compute()
    with pytest.raises(RuntimeError):
        s.optimal_threshold()
    s.reset()
    s.update(x, y, live=torch.tensor([200]))
    assert int(s.overflow) == 0 and s.compute()["tp"] == conf[3]


def test_set_threshold_changes_the_next_update():
    x, y, m = stats_inputs(5000, None, 0.72)
    s = EpochStats(threshold=0.5, device="cpu")
    s.update(x, y)
    a = s.counts.clone()
    assert a.tolist() == reference(x, y, m, 0.5, None)[0]
    s.set_threshold(0.72)
    s.update(x, y)
    assert (s.counts - a).tolist() == reference(x, y, m, 0.72, None)[0] and s.threshold == 0.72


def test_mismatched_operands_are_refused():
    s = EpochStats(device="cpu")
    with pytest.raises(ValueError):
        s.update(torch.zeros(3), torch.zeros(4))
    with pytest.raises(ValueError):
        EpochStats(capacity=-1, device="cpu")
