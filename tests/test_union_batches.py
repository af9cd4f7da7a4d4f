"""GPU suite of --union_edge_weights mini-batches: the two union collations of csrc/graph_build.hip
(pangnn_collate_subgraphs_padded_union with its collation-written CSR orders, pangnn_collate_subgraphs_union) against the
host restatement of tests/test_union_batches_host.py and against the structures graph.EdgeStructure builds from the collated
list, a union model on a union batch against the oracle in float64, and train.ReplayedFreshStep / ReplayedFreshEval /
run_epoch with a union model.

Tolerances.  Model parity: those of tests/test_hip_parity.py's whole-graph union cases, restated here — logits 1e-4 (north
star), loss 1e-5, parameter gradients 2e-5 of the tensor's scale from the float64 oracle.  Padded step against the unpadded
step: tests/test_padded_decoders.py's (loss 1e-6, logits 1e-5, gradients 1e-5 of their scale); a quantity beyond one of them
is adjudicated by the float64 oracle on that batch: the padded step may be no further from it than the unpadded step is, plus
1e-6 of the quantity's scale.  Validation logits: tests/test_replayed_eval.py's 1e-5; its loss bound 2^-21 (1 + pw) max(1,
max|x|)."""
import copy
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from conftest import sub_graphs_from_golden
from oracle import gcn_oracle as go
from test_union_batches_host import expected_padded_union, hand_made, union_layout

pytestmark = pytest.mark.gpu

ATOL = RTOL = 1e-4              # north star: link-prediction logits
FP64_DIRECT = 2e-5              # HIP gradient vs the fp64 oracle, of the tensor's scale (tests/test_hip_parity.py)


def dev():
    return torch.device("cuda:0")


def close(a, b, atol=ATOL, rtol=RTOL):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    ok = a.shape == b.shape and torch.allclose(a, b, atol=atol, rtol=rtol)
    if not ok:
        print("max abs err", (a - b).abs().max().item() if a.shape == b.shape else (a.shape, b.shape), "atol", atol)
    return ok


def loss_bound(x, pw):
    top = float(x.abs().max()) if x.numel() else 0.0
    return 2.0 ** -21 * (1.0 + float(pw)) * max(1.0, top)


def loss64(x, y, pw):
    pw64 = torch.as_tensor(pw, dtype=torch.float32).cpu().double()
    return float(F.binary_cross_entropy_with_logits(x.detach().cpu().double(), y.detach().cpu().double(), pos_weight=pw64))


@functools.lru_cache(maxsize=None)
def gpu_dataset(name):
    from pangnn_amd import simulate
    from pangnn_amd.subgraphs import SubGraphDataset
    if name == "cfg1":
        return SubGraphDataset.from_data_list(sub_graphs_from_golden("cfg1_2genomes"), device=dev())
    if name == "hand":
        return SubGraphDataset.from_data_list(hand_made(), device=dev())
    if name == "sim1000":
        return simulate.simulate_subgraph_dataset(1000, 5, 0.3, 10, 2, seed=0, device=dev())
    assert name == "sim300"
    return simulate.simulate_subgraph_dataset(300, 4, 0.3, 10, 2, seed=5, device=dev())


def largest(ds, count=32):
    h = ds._host()
    return sorted(range(ds.num_graphs), key=lambda i: h.edge[i] - h.edge[i + 1])[:count]


@functools.lru_cache(maxsize=1)
def schedule():
    """data set and schedule of tests/test_padded_decoders.py: shuffled batches of 32, the batch of the 32 largest sub-graphs
    (overflows the everyday buffers), a short last batch"""
    ds = gpu_dataset("sim300")
    perm = torch.randperm(ds.num_graphs, generator=torch.Generator().manual_seed(3)).tolist()
    sched = [perm[i:i + 32] for i in range(0, len(perm), 32)]
    big = largest(ds)
    return ds, ds.class_balance(), sched[:4] + [big] + sched[4:7] + [perm[:5]], big, perm


def reference_union_batch(ds, ids):
    """the disjoint union of the sub-graphs `ids` in the union layout, built with torch index ops, unpadded"""
    h = ds._host()
    ei, nb, w, y, n = [], [], [], [], 0
    for i in ids:
        n0, e0, e1, b0, b1 = h.node[i], h.edge[i], h.edge[i + 1], h.nb[i], h.nb[i + 1]
        ei.append(ds.edge_index[:, e0:e1] - n0 + n)
        nb.append(ds.neighbour_edge_index[:, b0:b1] - n0 + n)
        w.append(ds.edge_attr[e0:e1]); y.append(ds.y[e0:e1])
        n += h.node[i + 1] - n0
    ei, nb = torch.cat(ei, 1).contiguous(), torch.cat(nb, 1)
    return SimpleNamespace(x=torch.ones(n, 1, device=dev()), edge_index=ei, y=torch.cat(y).contiguous(),
                           edge_attr=torch.cat(w + [torch.ones(nb.shape[1], device=dev())]).contiguous(),
                           union_edge_index=torch.cat([ei, nb], 1).contiguous())


def to_cpu(g):
    return SimpleNamespace(**{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in g.__dict__.items()})


# ------------------------------------------------------------------------------------------------------------------
# 5. the padded union collation and its orders
# ------------------------------------------------------------------------------------------------------------------
def _collation_case(case):
    from pangnn_amd.subgraphs import PaddedSpec
    if case == "hand":
        ds = gpu_dataset("hand")
        return ds, [2, 0, 1], ds.padded_spec(3), True
    if case == "big":                       # the 1000 x 5 set's worst case: U_max beyond the one-workgroup sort's 16384
        ds = gpu_dataset("sim1000")
        spec = ds.padded_spec(32)
        assert spec.edges + spec.nb_edges > 16384
        return ds, largest(ds), spec, True
    ds, _, sched, big, perm = schedule()
    if case == "shuffled32":
        return ds, sched[0], ds.padded_spec(32), True
    if case == "one":
        return ds, [perm[7]], ds.padded_spec(32), True
    if case == "exact":                     # no padded edge at all: the guarded division, one padded node
        n, e, b = ds._counts(sched[1])
        return ds, sched[1], PaddedSpec(32, n + 1, e, b), True
    assert case == "nofit"
    spec = ds.padded_spec(32, slack=1.2)
    assert not ds.fits(spec, big)
    return ds, big, spec, False


def _fill(ds, buf, ids):
    """write the ids without set_graph_ids' host-side refusal of a batch that does not fit, then collate"""
    g = buf.spec.graphs
    buf.graph_ids.copy_(torch.tensor(list(ids) + [-1] * (g - len(ids)), dtype=torch.int64))
    return ds.collate_padded(buf)


@pytest.mark.parametrize("case", ["shuffled32", "one", "exact", "nofit", "hand", "big"])
def test_padded_union_collation(case):
    from pangnn_amd.graph import EdgeStructure, structure_of
    ds, ids, spec, fits = _collation_case(case)
    g, n, e, b = spec
    u = e + b
    buf = ds.padded_buffers(spec, union=True)
    plain = ds.padded_buffers(spec)
    assert buf.orders is not None and buf.union and not hasattr(buf, "neighbour_edge_index")
    assert buf.union_edge_index.shape == (2, u) and buf.edge_attr.shape == (u,) and buf.edge_index.shape == (2, e)
    _fill(ds, buf, ids)
    _fill(ds, plain, ids)
    exp = expected_padded_union(ds, ids, spec)
    assert int(exp.live[4]) == (0 if fits else 1)
    for k in ("edge_index", "union_edge_index", "edge_attr", "y", "ptr", "batch", "x"):
        assert torch.equal(getattr(buf, k).cpu(), getattr(exp, k)), k
    assert torch.equal(buf.live[:5].cpu(), exp.live)
    # the default-layout fields: the bits the default collation of the same ids writes
    for k in ("edge_index", "y", "ptr", "batch", "x"):
        assert torch.equal(getattr(buf, k), getattr(plain, k)), k
    assert torch.equal(buf.live[:5], plain.live[:5]) and torch.equal(buf.edge_attr[:e], plain.edge_attr)
    assert bool((buf.edge_attr[int(exp.live[0]):] == 1).all())
    # the similarity list's orders and plans: those of the default collation, entry for entry
    for name in ("sim_dst", "sim_src"):
        ta, tb = buf.orders.tables[name], plain.orders.tables[name]
        assert set(ta) == set(tb) == {"other", "perm", "keys", "rowptr", "part_off", "part_rowptr", "last_part"}
        for f in ta:
            assert torch.equal(ta[f], tb[f]), (name, f)
    # the union list's orders: the tables EdgeStructure builds from the collated list (one launch up to 16384 edges, the
    # general sort beyond)
    un = buf.union_edge_index.clone()
    built = EdgeStructure(un, n, hints={"valid_ids": True})
    assert bool(_lib().pangnn_structure_small_supported(u, n)) == (case != "big")
    for order, csr, row in (("union_dst", built.by_dst, 1), ("union_src", built.by_src, 0)):
        t = buf.orders.tables[order]
        assert set(t) == {"other", "perm", "keys", "rowptr"}
        assert torch.equal(t["rowptr"], csr.rowptr) and t["rowptr"].dtype == csr.rowptr.dtype, order
        assert torch.equal(t["perm"].long(), csr.perm.long()), order
        assert torch.equal(t["other"].long(), csr.other.long()), order
        assert torch.equal(t["keys"].long(), un[row][csr.perm.long()]), order
        assert int(t["rowptr"][0]) == 0 and int(t["rowptr"][-1]) == u and bool((t["rowptr"][1:] >= t["rowptr"][:-1]).all())
    # ... adopted under the name the model asks for, with the hints of a producer-vouched list
    st = structure_of(buf.union_edge_index, n, holder=buf, name="union")
    assert st is buf._pangnn_structs["union"][1] and st._small_built and st.hints == {"valid_ids": True, "band_width": 0}
    assert st.by_dst.rowptr.data_ptr() == buf.orders.tables["union_dst"]["rowptr"].data_ptr()
    assert structure_of(buf.union_edge_index, n) is st and set(buf._pangnn_structs) == {"sim", "union"}
    if case == "shuffled32":                 # a second collation replaces the structures (same addresses, new content)
        _fill(ds, buf, ids[:3])
        st2 = structure_of(buf.union_edge_index, n, holder=buf, name="union")
        assert st2 is not st and structure_of(buf.union_edge_index, n) is st2
        exp2 = expected_padded_union(ds, ids[:3], spec)
        assert torch.equal(buf.union_edge_index.cpu(), exp2.union_edge_index) and torch.equal(buf.edge_attr.cpu(), exp2.edge_attr)
        assert torch.equal(st2.by_src.perm.long().cpu(), torch.argsort(exp2.union_edge_index[0], stable=True))


def _lib():
    from pangnn_amd import _lib as L
    return L.load()


def test_union_orders_beyond_the_limit_are_built_per_batch():
    from pangnn_amd.subgraphs import PaddedSpec
    ds = gpu_dataset("hand")
    buf = ds.padded_buffers(PaddedSpec(3, 64, 16384, 16385), union=True)
    assert buf.orders is None and buf.union_edge_index.shape == (2, 32769)
    _fill(ds, buf, [0, 1, 2])
    exp = expected_padded_union(ds, [0, 1, 2], buf.spec)
    assert torch.equal(buf.union_edge_index.cpu(), exp.union_edge_index) and torch.equal(buf.edge_attr.cpu(), exp.edge_attr)
    assert "_pangnn_structs" not in buf.__dict__


# ------------------------------------------------------------------------------------------------------------------
# 6. batch(union=True) on the device
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rng", [("sim300", (0, 32)), ("sim300", (33, 34)), ("sim300", (90, 10 ** 6)), ("hand", (0, 3)),
                                      ("hand", (1, 2)), ("cfg1", (0, 32))])
def test_union_batch_on_the_device_equals_the_index_ops(name, rng):
    from pangnn_amd.subgraphs import SubGraphDataset
    ds = gpu_dataset(name)
    host = SubGraphDataset(**{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in ds.__dict__.items()
                              if not k.startswith("_")})
    got, want = ds.batch(*rng, union=True), host.batch(*rng, union=True)
    assert set(got.__dict__) == set(want.__dict__) and got.num_graphs == want.num_graphs
    assert got._pangnn_hints == want._pangnn_hints
    for k in ("x", "edge_index", "edge_attr", "y", "union_edge_index", "ptr", "batch"):
        a, b = getattr(got, k), getattr(want, k)
        assert a.is_cuda and a.dtype == b.dtype and torch.equal(a.cpu(), b), k


# ------------------------------------------------------------------------------------------------------------------
# 7. a union model on a union batch against the oracle in float64
# ------------------------------------------------------------------------------------------------------------------
def _oracle64(flags, dims, state, g, pw):
    """(loss, logits, {parameter: gradient}) of the oracle evaluated in float64 on the CPU graph `g`"""
    oracle = go.AlternateGCNOracle(dims=tuple(dims), flags=go.default_flags(**flags))
    oracle.load_state_dict({k: v.detach().cpu() for k, v in state.items()})
    o64 = oracle.double()
    g64 = copy.copy(g)
    g64.x, g64.edge_attr = g.x.double(), g.edge_attr.double()
    out = o64(g64)
    loss = F.binary_cross_entropy_with_logits(out, g.y.double(), pos_weight=torch.as_tensor(pw).detach().cpu().double())
    loss.backward()
    return loss.detach(), out.detach(), {k: p.grad for k, p in o64.named_parameters()}


PARITY = [(dict(union_edge_weights=True), (64, 128)), (dict(union_edge_weights=True, neighbours=4), (64, 64)),
          (dict(union_edge_weights=True, skip_connections=True), (64, 128))]


@pytest.mark.parametrize("flags,dims", PARITY, ids=["union", "union-nb4", "union-skip"])
def test_union_model_on_a_union_batch_against_the_fp64_oracle(flags, dims):
    import pangnn_amd
    subs = sub_graphs_from_golden("cfg1_2genomes")
    ds = gpu_dataset("cfg1")
    batch = ds.batch(0, 32, union=True)
    # without skip_connections the model is the same function of the reference's own layout ([neighbour | similarity] per
    # sub-graph); with them the reference reads misaligned weights and the aligned layout is this build's definition
    g = to_cpu(batch) if flags.get("skip_connections") else go.collate(union_layout(subs[:32]))
    torch.manual_seed(0)
    oracle = go.AlternateGCNOracle(dims=dims, flags=go.default_flags(**flags))
    with torch.no_grad():
        for k, p in oracle.named_parameters():
            if k.endswith("bias"):
                p.uniform_(-0.5, 0.5)         # PyG initialises conv biases to 0; make them count
    model = pangnn_amd.AlternateGCN(dev(), None, False, dims=list(dims), **flags)
    model.load_state_dict(oracle.state_dict())
    pw = (g.y == 0).sum() / g.y.sum()
    l64, ref, g64 = _oracle64(flags, dims, oracle.state_dict(), g, pw)
    out = model(batch)
    assert out.shape == ref.shape == (batch.edge_index.shape[1],)
    print("max |logit - fp64|", float((out.detach().cpu().double() - ref).abs().max()))
    assert close(out, ref)
    lo = F.binary_cross_entropy_with_logits(out, batch.y, pos_weight=pw.to(dev()))
    assert close(lo, l64, atol=1e-5, rtol=1e-5)
    lo.backward()
    worst = {}
    for k, p in model.named_parameters():
        if g64[k] is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        scale = float(g64[k].abs().max()) + 1e-12
        worst[k] = float((p.grad.detach().cpu().double() - g64[k]).abs().max()) / scale
    print("gradient distance to the fp64 oracle, of the tensor's scale:", {k: f"{v:.1e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= FP64_DIRECT, (k, v)


# ------------------------------------------------------------------------------------------------------------------
# 8. train.ReplayedFreshStep with a union model
# ------------------------------------------------------------------------------------------------------------------
STEP_CASES = {
    "union": dict(dims=[64, 128], union_edge_weights=True),
    "union-nb4": dict(dims=[64, 64], union_edge_weights=True, neighbours=4),
    "union-skip": dict(dims=[64, 128], union_edge_weights=True, skip_connections=True),
    "union-cosine": dict(dims=[64, 128], union_edge_weights=True, decoder="cosine"),
}


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_replayed_fresh_step_serves_a_union_model(case):
    """tests/test_padded_decoders.py::test_replayed_fresh_step_serves_these_decoders for --union_edge_weights:
      (i)  the captured replay == the same padded step run eagerly, bit for bit (loss, logits, every parameter after every
           step) over the shuffled schedule, the batch that overflows the everyday buffers and the short last batch included;
      (ii) the padded step against train_step on the unpadded union batch from the same parameters: loss 1e-6, logits 1e-5,
           gradients 1e-5 of their scale — a quantity beyond its bound must be no further from the float64 oracle on that
           batch than the unpadded step's is, plus 1e-6 of its scale (both distances are printed)."""
    import pangnn_amd
    from pangnn_amd.train import ReplayedFreshStep, make_optimizer, train_step
    kw = STEP_CASES[case]
    flags = {k: v for k, v in kw.items() if k != "dims"}
    ds, pw, sched, big, _ = schedule()
    h = ds._host()

    def make(capture):
        torch.manual_seed(0)
        model = pangnn_amd.AlternateGCN(dev(), None, False, **kw)
        opt = make_optimizer(model, capturable=True)
        return model, opt, ReplayedFreshStep(model, opt, ds, pw, 32, capture=capture, warmup=1, slack=1.2)

    ma, oa, sa = make(True)
    mb, ob, sb = make(False)
    assert sa.union and not ds.fits(sa.spec, big) and ds.fits(sa.spec_worst, big)
    for k, ids in enumerate(sched):
        la, xa = sa(ids)
        lb, xb = sb(ids)
        assert xa.shape == xb.shape == (sum(h.edge[i + 1] - h.edge[i] for i in ids),)
        assert torch.equal(la, lb) and torch.equal(xa, xb), (k, float(la), float(lb))
        assert bool(torch.isfinite(la))
        for p, q in zip(ma.parameters(), mb.parameters()):
            assert torch.equal(p, q), k
    assert len(sa._slots) == 2
    for buf, _, _ in sa._slots.values():
        assert buf.union and buf.orders is not None              # both sets of buffers: collation-written orders

    torch.manual_seed(0)
    mc = pangnn_amd.AlternateGCN(dev(), None, False, **kw)
    oc = make_optimizer(mc, capturable=True)
    for ids in (sched[0], sched[-1]):
        state = {k: v.detach().clone() for k, v in mb.state_dict().items()}
        mc.load_state_dict(state)
        batch = reference_union_batch(ds, ids)
        lc, xc = train_step(mc, oc, batch, batch.y, pw)
        lb, xb = sb(ids)
        pairs = [("loss", lb, lc, 1e-6, 1e-6), ("logits", xb, xc, 1e-5, 1e-5)]
        for (k, p), (_, q) in zip(mb.named_parameters(), mc.named_parameters()):
            if q.grad is None:                           # a layer this topology does not use
                assert p.grad is None, k
                continue
            pairs.append((k, p.grad, q.grad, 1e-5 * (float(q.grad.abs().max()) + 1e-12) + 1e-9, 1e-4))
        print(f"{case}: padded loss {float(lb)!r} unpadded {float(lc)!r} max|dlogit| {float((xb - xc).abs().max()):.3e}")
        beyond = [(k, a, b) for k, a, b, atol, rtol in pairs if not close(a, b, atol=atol, rtol=rtol)]
        if beyond:
            l64, x64, g64 = _oracle64(flags, kw["dims"], state, to_cpu(batch), pw)
            ref = dict(g64, loss=l64, logits=x64)
            for k, a, b in beyond:
                scale = float(ref[k].abs().max()) + 1e-12
                d_pad = float((a.detach().cpu().double() - ref[k]).abs().max())
                d_unp = float((b.detach().cpu().double() - ref[k]).abs().max())
                print(f"{case}: {k}: distance to the fp64 oracle, padded {d_pad:.3e} unpadded {d_unp:.3e} scale {scale:.3e}")
                assert d_pad <= d_unp + 1e-6 * scale, (k, d_pad, d_unp, scale)


# ------------------------------------------------------------------------------------------------------------------
# 9. train.ReplayedFreshEval with a union model
# ------------------------------------------------------------------------------------------------------------------
def same_stats(a, b):
    c = int(a.cursor)
    return torch.equal(a.state, b.state) and torch.equal(a.scores[:c], b.scores[:c]) and torch.equal(a.labels[:c], b.labels[:c])


@pytest.mark.parametrize("kw", [dict(), dict(neighbours=4, dims=[64, 64]), dict(skip_connections=True)],
                         ids=["union", "union-nb4", "union-skip"])
def test_replayed_eval_serves_a_union_model(kw):
    import pangnn_amd
    from pangnn_amd.metrics import BinaryAUROC, BinaryAveragePrecision, BinaryConfusionMatrix
    from pangnn_amd.train import ReplayedFreshEval
    ds, pw, sched, big, perm = schedule()
    torch.manual_seed(0)
    model = pangnn_amd.AlternateGCN(dev(), None, False, **dict(dict(dims=[64, 128], union_edge_weights=True), **kw))
    model.train()
    before = [p.detach().clone() for p in model.parameters()]
    ea = ReplayedFreshEval(model, ds, pw, 32, capture=True, slack=1.2)
    eb = ReplayedFreshEval(model, ds, pw, 32, capture=False, slack=1.2)
    assert ea.union and model.training and same_stats(ea.stats, eb.stats) and ea.stats.state[:9].tolist() == [0] * 9
    h = ds._host()
    for k, ids in enumerate(sched[:2] + [big, perm[:5]]):              # everyday slot, worst-case slot, a short batch
        xa, xb = ea(ids), eb(ids)
        assert xa.shape == xb.shape == (sum(h.edge[i + 1] - h.edge[i] for i in ids),)
        assert torch.equal(xa, xb) and same_stats(ea.stats, eb.stats), k
        assert model.training and not xa.requires_grad
    assert len(ea._slots) == 2 and len(eb._slots) == 2
    for p, q in zip(model.parameters(), before):
        assert torch.equal(p, q) and p.grad is None

    # two batches against model.eval()(batch) on the unpadded union batch; the stats are exact functions of the returned logits
    ea.reset()
    outs, ys, losses = [], [], []
    model.eval()
    for ids in (sched[0], sched[-1]):
        out = ea(ids).clone()
        batch = reference_union_batch(ds, ids)
        with torch.no_grad():
            ref = model(batch)
        assert close(out, ref, atol=1e-5, rtol=1e-5)
        outs.append(out); ys.append(batch.y); losses.append(loss64(out, batch.y, pw))
    assert not model.training
    model.train()
    allx, ally = torch.cat(outs), torch.cat(ys)
    cm = BinaryConfusionMatrix(0.5, device=dev())
    cm.update_from_logits(allx, ally)
    assert torch.equal(ea.stats.counts, cm.counts) and int(ea.stats.cursor) == allx.shape[0]
    res = ea.compute()
    auroc = BinaryAUROC()
    ap = BinaryAveragePrecision(share_curve_with=auroc)
    prob = torch.sigmoid(allx)
    auroc.update(prob, ally); ap.update(prob, ally)
    assert res["roc_auc"] == float(auroc.compute()) and res["pr_auc"] == float(ap.compute())
    assert abs(res["loss"] - sum(losses) / 2) <= loss_bound(allx, pw)


# ------------------------------------------------------------------------------------------------------------------
# 10. run_epoch
# ------------------------------------------------------------------------------------------------------------------
def test_run_epoch_with_a_union_pair():
    import math
    import pangnn_amd
    from pangnn_amd.metrics import EpochStats
    from pangnn_amd.train import ReplayedFreshEval, ReplayedFreshStep, make_optimizer, run_epoch
    ds, pw, _, _, _ = schedule()
    n_train, n_val = int(0.7 * ds.num_graphs), int(0.15 * ds.num_graphs)
    train_ids, val_ids = list(range(n_train)), list(range(n_train, n_train + n_val))
    torch.manual_seed(0)
    model = pangnn_amd.AlternateGCN(dev(), None, False, dims=[64, 128], union_edge_weights=True)
    opt = make_optimizer(model, capturable=True)
    step = ReplayedFreshStep(model, opt, ds, pw, 32, graphs=train_ids, warmup=1, stats=EpochStats(0, device=dev()))
    ev = ReplayedFreshEval(model, ds, pw, 32, graphs=val_ids)
    before = [p.detach().clone() for p in model.parameters() if p.requires_grad]
    res = run_epoch(step, ev, train_ids, val_ids, 32, generator=torch.Generator().manual_seed(7))
    assert set(res) == {"train_loss", "train_acc", "train_f1", "val_loss", "val_acc", "val_precision", "val_recall", "val_f1",
                        "val_roc_auc", "val_pr_auc"}
    assert all(math.isfinite(float(v)) for v in res.values()), res
    assert int(step.stats.batches) == -(-n_train // 32) and int(ev.stats.batches) == -(-n_val // 32)
    assert any(not torch.equal(p, q) for p, q in zip((p for p in model.parameters() if p.requires_grad), before))
