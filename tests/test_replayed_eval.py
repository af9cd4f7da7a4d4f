"""GPU suite of the epoch statistics: pangnn_batch_stats_f32 (csrc/batch_stats.hip) behind metrics.EpochStats against the
existing primitives on given logits, train.ReplayedFreshEval (the validation loop from one captured HIP graph) against its eager
run and against the unpadded model, the optional training statistics of train.ReplayedFreshStep, and train.run_epoch.

Loss bound (every computed loss here): 2^-21 (1 + pw) max(1, max|x|) — every rounding of the per-edge term
(1-y) x + (1 + (pw-1) y) (log1p(exp(-|x|)) + max(-x, 0)) is of a quantity no larger than max(1, |x|) (1 + pw), the two library
calls are good to a few ulp, and the float64 sum adds nothing; one padded element counted in (logit 30, label 1: a term of 0 at
weight pw but a divisor off by one) or a wrong divisor misses it by orders of magnitude."""
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from test_epoch_stats_host import lives, stats_inputs

pytestmark = pytest.mark.gpu

N_MAX = (1, 65, 257, 5000, 20000)            # 20000: past the one-workgroup limit (partials + finish kernel)
GRID = [(n, lv) for n in N_MAX for lv in lives(n)]


def dev():
    return torch.device("cuda:0")


def loss_bound(x, pw):
    top = float(x.abs().max()) if x.numel() else 0.0
    return 2.0 ** -21 * (1.0 + (1.0 if pw is None else float(pw))) * max(1.0, top)


def loss64(x, y, pw):
    """float64 BCEWithLogits(pos_weight) on the host; pos_weight is the float32 scalar the kernels take"""
    pw64 = None if pw is None else torch.as_tensor(pw, dtype=torch.float32).cpu().double()
    return float(F.binary_cross_entropy_with_logits(x.detach().cpu().double(), y.detach().cpu().double(), pos_weight=pw64))


def confusion_of(logits, y, threshold=0.5):
    from pangnn_amd.metrics import BinaryConfusionMatrix
    cm = BinaryConfusionMatrix(threshold, device=dev())
    cm.update_from_logits(logits, y)
    return cm.counts.clone()


# ------------------------------------------------------------------------------------------------------------------
# 1. the kernel against the existing primitives on given logits
# ------------------------------------------------------------------------------------------------------------------
def _sequence(n_max, live, pw, check):
    """update at threshold 0.5 -> device threshold 0.72 -> update -> update with a given loss; returns the final state"""
    from pangnn_amd import functional as PF
    from pangnn_amd.metrics import EpochStats
    x1, y1, m = stats_inputs(n_max, live, 0.5)
    x2, y2, _ = stats_inputs(n_max, live, 0.72, seed=1)
    x1, y1, x2, y2 = (t.to(dev()) for t in (x1, y1, x2, y2))
    lv = None if live is None else torch.tensor([live], device=dev())
    pwt = None if pw is None else torch.tensor(pw, device=dev())
    cap = 3 * m + 3
    s = EpochStats(capacity=cap, threshold=0.5, device=dev())
    s.scores.fill_(-7.0)
    s.labels.fill_(9)
    given = torch.tensor(0.8125331, device=dev())

    s.update(x1, y1, live=lv, pos_weight=pwt)
    if check and m > 0:
        assert torch.equal(s.counts, confusion_of(x1[:m], y1[:m], 0.5))
        l1 = float(s.loss_sum)
        print(f"n_max={n_max} m={m} pw={pw}: loss {l1!r} f64 {loss64(x1[:m], y1[:m], pw)!r} bound {loss_bound(x1[:m], pw):.3e}")
        assert abs(l1 - loss64(x1[:m], y1[:m], pw)) <= loss_bound(x1[:m], pw)
        assert abs(l1 - float(PF.bce_with_logits(x1[:m].contiguous(), y1[:m].contiguous(), pwt))) <= loss_bound(x1[:m], pw)
        assert float(s.last_loss) == float(torch.tensor(l1, dtype=torch.float64).float()) and int(s.batches) == 1
        assert int(s.cursor) == m and torch.equal(s.scores[:m], x1[:m])
        assert torch.equal(s.labels[:m], (y1[:m] > 0.5).to(torch.uint8))
    before = s.state.clone()

    s.set_threshold(0.72)                          # the device scalar: the next update counts at it with no other call
    s.update(x2, y2, live=lv, pos_weight=pwt)
    if check and m > 0:
        assert torch.equal(s.counts - before[:4], confusion_of(x2[:m], y2[:m], 0.72))
        assert int(s.cursor) == 2 * m and torch.equal(s.scores[m:2 * m], x2[:m])
    before = s.state.clone()

    s.update(x1, y1, live=lv, pos_weight=pwt, loss=given)
    if check and m > 0:
        assert float(s.loss_sum) == float(before[7:8].view(torch.float64)) + float(given)          # f64 + f32 value: exact
        assert float(s.last_loss) == float(given) and int(s.batches) == 3
        assert torch.equal(s.counts - before[:4], confusion_of(x1[:m], y1[:m], 0.72))
        assert int(s.cursor) == 3 * m and torch.equal(s.scores[2 * m:3 * m], x1[:m]) and int(s.overflow) == 0
    if check:
        if m == 0:                                 # empty batches: nothing added, none counted
            assert s.state[:9].tolist() == [0] * 9
        # behind the cursor: untouched — also by the poisoned tail of the inputs
        assert bool((s.scores[3 * m:] == -7).all()) and bool((s.labels[3 * m:] == 9).all())
    return s.state.clone(), s.scores.clone(), s.labels.clone()


@pytest.mark.parametrize("case", GRID, ids=lambda v: f"n{v[0]}-live{v[1]}")
@pytest.mark.parametrize("pw", [None, 4.3])
def test_kernel_against_the_existing_primitives(case, pw):
    n_max, live = case
    a = _sequence(n_max, live, pw, check=True)
    b = _sequence(n_max, live, pw, check=False)
    for u, v in zip(a, b):                          # the same sequence twice: the same bits
        assert torch.equal(u, v)


@pytest.mark.parametrize("n_max", [257, 20000])
def test_kernel_overflow_and_live_outside_the_batch(n_max):
    from pangnn_amd.metrics import EpochStats
    x, y, m = stats_inputs(n_max, n_max - 50)
    x, y = x.to(dev()), y.to(dev())
    lv = torch.tensor([m], device=dev())
    s = EpochStats(capacity=m + 10, device=dev())
    s.scores.fill_(-7.0)
    s.update(x, y, live=lv)
    kept = s.scores.clone()
    s.update(x, y, live=lv)                                                   # does not fit: nothing appended
    assert int(s.cursor) == m and int(s.overflow) == 1 and torch.equal(s.scores, kept)
    assert torch.equal(s.counts, 2 * confusion_of(x[:m], y[:m])) and int(s.batches) == 2   # counts and loss are still taken
    with pytest.raises(RuntimeError):
        s.compute()
    for bad in (-1, n_max + 1, 1 << 40):                                      # no count of this batch: all n_max entries
        t = EpochStats(capacity=n_max, device=dev())
        t.update(x, y, live=torch.tensor([bad], device=dev()))
        assert int(t.cursor) == n_max and torch.equal(t.counts, confusion_of(x, y)) and torch.equal(t.scores, x)


# ------------------------------------------------------------------------------------------------------------------
# the data set, schedule and models of tests 2-6
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def dataset():
    from pangnn_amd import simulate
    ds = simulate.simulate_subgraph_dataset(300, 4, 0.3, 10, 2, seed=5, device=dev())
    h = ds._host()
    perm = torch.randperm(ds.num_graphs, generator=torch.Generator().manual_seed(3)).tolist()
    schedule = [perm[i:i + 32] for i in range(0, len(perm), 32)]
    big = sorted(range(ds.num_graphs), key=lambda i: h.edge[i] - h.edge[i + 1])[:32]      # the 32 largest sub-graphs
    schedule = schedule[:4] + [big] + schedule[4:7] + [perm[:5]]
    return ds, ds.class_balance(), schedule, big, perm


def make_model(**kw):
    import pangnn_amd
    torch.manual_seed(0)
    return pangnn_amd.AlternateGCN(dev(), None, False, **dict(dict(dims=[64, 128]), **kw))


def reference_batch(ds, ids):
    """the disjoint union of the sub-graphs `ids` built with torch index ops (what Batch.from_data_list does), unpadded"""
    h = ds._host()
    ei, nb, w, y, n = [], [], [], [], 0
    for i in ids:
        n0, e0, e1, b0, b1 = h.node[i], h.edge[i], h.edge[i + 1], h.nb[i], h.nb[i + 1]
        ei.append(ds.edge_index[:, e0:e1] - n0 + n)
        nb.append(ds.neighbour_edge_index[:, b0:b1] - n0 + n)
        w.append(ds.edge_attr[e0:e1]); y.append(ds.y[e0:e1])
        n += h.node[i + 1] - n0
    return SimpleNamespace(x=torch.ones(n, 1, device=dev()), edge_index=torch.cat(ei, 1).contiguous(),
                           edge_attr=torch.cat(w).contiguous(), y=torch.cat(y).contiguous(),
                           neighbour_edge_index=torch.cat(nb, 1).contiguous())


def same_stats(a, b):
    c = int(a.cursor)
    return torch.equal(a.state, b.state) and torch.equal(a.scores[:c], b.scores[:c]) and torch.equal(a.labels[:c], b.labels[:c])


def close(a, b, tol=1e-5):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    ok = a.shape == b.shape and torch.allclose(a, b, atol=tol, rtol=tol)
    if not ok:
        print("max abs err", (a - b).abs().max().item() if a.shape == b.shape else (a.shape, b.shape))
    return ok


# ------------------------------------------------------------------------------------------------------------------
# 2. replay == eager     3. padded == unpadded
# ------------------------------------------------------------------------------------------------------------------
def test_replayed_eval_equals_its_eager_run_and_the_unpadded_model():
    from pangnn_amd.metrics import BinaryAUROC, BinaryAveragePrecision
    from pangnn_amd.train import ReplayedFreshEval
    ds, pw, schedule, big, _ = dataset()
    model = make_model()
    model.train()
    before = [p.detach().clone() for p in model.parameters()]
    ea = ReplayedFreshEval(model, ds, pw, 32, capture=True, slack=1.2)
    eb = ReplayedFreshEval(model, ds, pw, 32, capture=False, slack=1.2)
    assert model.training and same_stats(ea.stats, eb.stats) and ea.stats.state[:9].tolist() == [0] * 9
    assert not ds.fits(ea.spec, big) and ds.fits(ea.spec_worst, big)        # the schedule does exercise the second slot
    h = ds._host()
    assert ea.stats.capacity == h.edge[-1]
    for k, ids in enumerate(schedule):
        xa, xb = ea(ids), eb(ids)
        assert xa.shape == xb.shape == (sum(h.edge[i + 1] - h.edge[i] for i in ids),)
        assert torch.equal(xa, xb) and same_stats(ea.stats, eb.stats), k
        assert model.training and not xa.requires_grad
    assert len(ea._slots) == 2 and len(eb._slots) == 2
    # the schedule repeats sub-graphs, so it may hold more edges than the one pass the ranking buffers are sized for: a batch
    # that does not fit is not appended and flags the overflow, on both routes (host arithmetic on the offset table)
    cursor, overflow = 0, 0
    for ids in schedule:
        e = sum(h.edge[i + 1] - h.edge[i] for i in ids)
        if cursor + e <= ea.stats.capacity:
            cursor += e
        else:
            overflow = 1
    assert int(ea.stats.overflow) == overflow and int(ea.stats.cursor) == cursor and int(ea.stats.batches) == len(schedule)
    if overflow:
        with pytest.raises(RuntimeError):
            ea.compute()
    for p, q in zip(model.parameters(), before):
        assert torch.equal(p, q) and p.grad is None

    # 3. two batches against model.eval()(batch) on the unpadded union; the stats are exact functions of the returned logits
    ea.reset()
    outs, ys, losses = [], [], []
    model.eval()
    for ids in (schedule[0], schedule[-1]):
        out = ea(ids).clone()
        batch = reference_batch(ds, ids)
        with torch.no_grad():
            ref = model(batch)
        assert close(out, ref)
        outs.append(out); ys.append(batch.y); losses.append(loss64(out, batch.y, pw))
    assert not model.training
    model.train()
    allx, ally = torch.cat(outs), torch.cat(ys)
    assert torch.equal(ea.stats.counts, confusion_of(allx, ally)) and int(ea.stats.cursor) == allx.shape[0]
    res = ea.compute()
    auroc = BinaryAUROC()
    ap = BinaryAveragePrecision(share_curve_with=auroc)
    prob = torch.sigmoid(allx)
    auroc.update(prob, ally); ap.update(prob, ally)
    assert res["roc_auc"] == float(auroc.compute()) and res["pr_auc"] == float(ap.compute())
    print("loss", res["loss"], "f64 mean", sum(losses) / 2, "bound", loss_bound(allx, pw))
    assert abs(res["loss"] - sum(losses) / 2) <= loss_bound(allx, pw)
    assert torch.equal(ea.stats.optimal_threshold(), auroc.optimal_threshold())


# ------------------------------------------------------------------------------------------------------------------
# 4. the decoders and widths the training replay does not serve
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(decoder="cosine"), dict(dims=[32, 64]), dict(skip_connections=True)],
                         ids=["cosine", "d32", "skip"])
def test_replayed_eval_serves_other_decoders(kw):
    from pangnn_amd.train import ReplayedFreshEval
    ds, pw, schedule, _, perm = dataset()
    model = make_model(**kw)
    model.eval()
    ea = ReplayedFreshEval(model, ds, pw, 32, capture=True, slack=1.2)
    eb = ReplayedFreshEval(model, ds, pw, 32, capture=False, slack=1.2)
    for ids in (schedule[0], schedule[1], perm[:5]):
        xa, xb = ea(ids), eb(ids)
        assert torch.equal(xa, xb) and same_stats(ea.stats, eb.stats)
        with torch.no_grad():
            ref = model(reference_batch(ds, ids))
        assert close(xa, ref)
        assert not model.training
    assert int(ea.stats.batches) == 3 and int(ea.stats.overflow) == 0
    assert 0.0 <= ea.compute()["roc_auc"] <= 1.0


# ------------------------------------------------------------------------------------------------------------------
# 5. training statistics of the replayed step
# ------------------------------------------------------------------------------------------------------------------
def test_training_statistics_do_not_perturb_the_replayed_step():
    from pangnn_amd.metrics import EpochStats
    from pangnn_amd.train import ReplayedFreshStep, make_optimizer
    ds, pw, schedule, _, _ = dataset()
    schedule = schedule[:3] + [schedule[4], schedule[-1]]                    # everyday slot, worst-case slot, short batch

    def make(stats):
        model = make_model()
        opt = make_optimizer(model, capturable=True)
        return model, ReplayedFreshStep(model, opt, ds, pw, 32, capture=True, warmup=1, slack=1.2, stats=stats)

    s = EpochStats(capacity=0, device=dev())
    ma, sa = make(s)
    mb, sb = make(None)
    assert s.state[:9].tolist() == [0] * 9                                   # building a slot is not a step
    total, outs, ys = 0.0, [], []
    for k, ids in enumerate(schedule):
        la, xa = sa(ids)
        lb, xb = sb(ids)
        assert torch.equal(la, lb) and torch.equal(xa, xb), k
        for p, q in zip(ma.parameters(), mb.parameters()):
            assert torch.equal(p, q), k
        total += float(la)                                                   # float64 sum of the float32 losses, in order
        outs.append(xa.clone()); ys.append(reference_batch(ds, ids).y)
        assert float(s.last_loss) == float(la)
    assert float(s.loss_sum) == total and int(s.batches) == len(schedule)
    assert torch.equal(s.counts, confusion_of(torch.cat(outs), torch.cat(ys)))
    assert torch.equal(s.confusion().view(-1), s.counts) and len(sa._slots) == 2


# ------------------------------------------------------------------------------------------------------------------
# 6. run_epoch
# ------------------------------------------------------------------------------------------------------------------
def test_run_epoch_is_the_two_objects_called_in_order():
    from pangnn_amd.metrics import BinaryAUROC, BinaryAveragePrecision, EpochStats, summary_from_confusion
    from pangnn_amd.train import ReplayedFreshEval, ReplayedFreshStep, make_optimizer, run_epoch
    ds, pw, _, _, _ = dataset()
    n_train, n_val = int(0.7 * ds.num_graphs), int(0.15 * ds.num_graphs)
    train_ids, val_ids = list(range(n_train)), list(range(n_train, n_train + n_val))

    def make():
        model = make_model()
        opt = make_optimizer(model, capturable=True)
        step = ReplayedFreshStep(model, opt, ds, pw, 32, graphs=train_ids, warmup=1, stats=EpochStats(0, device=dev()))
        return step, ReplayedFreshEval(model, ds, pw, 32, graphs=val_ids)

    step, ev = make()
    res = run_epoch(step, ev, train_ids, val_ids, 32, generator=torch.Generator().manual_seed(7))

    # by hand, in the same order, from the same seed
    step2, ev2 = make()
    order = torch.randperm(n_train, generator=torch.Generator().manual_seed(7)).tolist()
    total, steps, outs, ys = 0.0, 0, [], []
    for k in range(0, n_train, 32):
        ids = [train_ids[j] for j in order[k:k + 32]]
        loss, out = step2(ids)
        total, steps = total + float(loss), steps + 1
        outs.append(out.clone()); ys.append(reference_batch(ds, ids).y)
    tr = summary_from_confusion(confusion_of(torch.cat(outs), torch.cat(ys)))
    assert res["train_loss"] == total / steps and res["train_acc"] == tr["accuracy"] and res["train_f1"] == tr["f1"]
    outs, ys, losses = [], [], []
    for k in range(0, n_val, 32):
        ids = val_ids[k:k + 32]
        out = ev2(ids).clone()
        outs.append(out); ys.append(reference_batch(ds, ids).y); losses.append(loss64(out, ys[-1], pw))
    allx, ally = torch.cat(outs), torch.cat(ys)
    va = summary_from_confusion(confusion_of(allx, ally))
    for k in ("precision", "recall", "f1"):
        assert res["val_" + k] == va[k], k
    assert res["val_acc"] == va["accuracy"]
    auroc = BinaryAUROC()
    ap = BinaryAveragePrecision(share_curve_with=auroc)
    auroc.update(torch.sigmoid(allx), ally); ap.update(torch.sigmoid(allx), ally)
    assert res["val_roc_auc"] == float(auroc.compute()) and res["val_pr_auc"] == float(ap.compute())
    assert res["val_loss"] == ev2.compute()["loss"]                           # the same launches on the same logits
    assert abs(res["val_loss"] - sum(losses) / len(losses)) <= loss_bound(allx, pw)
    assert set(res) == {"train_loss", "train_acc", "train_f1", "val_loss", "val_acc", "val_precision", "val_recall", "val_f1",
                        "val_roc_auc", "val_pr_auc"}
