"""GPU suite of the live-aware fused-loss passes: a padded fixed-shape batch whose real-edge count the kernels read from device
memory (include/pangnn_hip.h, live_edges), for every decoder outside decoder16.hip —
  1. cosine / dot (pangnn_edge_score_loss_live_mixed behind pangnn::edge_score_loss_live) against PF.edge_score_loss on the list
     cut to its live edges,
  2. the strict-fp32 mlp decoder at node_dim 32, 64, 128 (pangnn_decoder_nd_loss_live_f32 / pangnn_decoder_mlp_loss_live_f32)
     against functional._decoder_grads on the cut list,
  3. train.ReplayedFreshStep on these decoders: captured replay == eager padded step, padded step ~ unpadded train_step,
  4. what a padded batch still refuses.

Loss bound (every computed loss here): 2^-21 (1 + pw) max(1, max|x|), as tests/test_replayed_eval.py derives it — every rounding
of the per-edge term is of a quantity no larger than max(1, |x|) (1 + pw), the library calls are good to a few ulp; one padded
edge counted in, or a divisor off by one, misses it by orders of magnitude.
Gradient bound of the padded-versus-cut comparisons of the mlp decoder: 1e-5 of the tensor's scale + 1e-9 (slab and chunk
grouping follow the padded count, so the sums are re-associated; tests/test_hip_parity.py's padded-versus-unpadded bound)."""
import contextlib
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PW = 2.5


def dev():
    return torch.device("cuda:0")


def loss_bound(x, pw):
    top = float(x.abs().max()) if x.numel() else 0.0
    return 2.0 ** -21 * (1.0 + float(pw)) * max(1.0, top)


def loss64(x, y, pw):
    pw64 = torch.as_tensor(pw, dtype=torch.float32).double()
    return float(F.binary_cross_entropy_with_logits(x.detach().cpu().double(), y.detach().cpu().double(), pos_weight=pw64))


def close(a, b, atol, rtol=0.0):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    ok = torch.allclose(a, b, atol=atol, rtol=rtol)
    if not ok:
        print("max abs err", (a - b).abs().max().item(), "max |ref|", b.abs().max().item(), "atol", atol)
    return ok


@contextlib.contextmanager
def strict_fp32(on=True):
    """PF.DECODER_PRECISION = 0 for the duration (node_dim 64 then runs csrc/decoder.hip's instance), restored afterwards"""
    from pangnn_amd import functional as PF
    old = PF.DECODER_PRECISION
    if on:
        PF.DECODER_PRECISION = 0
    try:
        yield
    finally:
        PF.DECODER_PRECISION = old


# ------------------------------------------------------------------------------------------------------------------
# 1. kernel level, scores
# ------------------------------------------------------------------------------------------------------------------
N_NODES, N_REAL, E_ALL, E_REAL = 200, 150, 1000, 700
SCORE_LIVES = (0, 1, 63, 64, 65, 700, 1000, 1005)


@functools.lru_cache(maxsize=None)
def _score_list():
    """E_ALL edges on N_NODES nodes in the padding convention: E_REAL edges among the real nodes [0, N_REAL), then self loops
    spread over the padded nodes with non-decreasing ids; labels 0 and weight-free on the tail"""
    gen = torch.Generator().manual_seed(17)
    real = torch.randint(0, N_REAL, (2, E_REAL), generator=gen)
    pad = (N_REAL + torch.arange(E_ALL - E_REAL) * (N_NODES - N_REAL) // (E_ALL - E_REAL)).repeat(2, 1)
    y = torch.cat([(torch.rand(E_REAL, generator=gen) < 0.3).float(), torch.zeros(E_ALL - E_REAL)])
    return torch.cat([real, pad], 1).contiguous(), y


def _score_rows(d, dtype):
    gen = torch.Generator().manual_seed(d)
    z = torch.randn(N_NODES, d, generator=gen) / d ** 0.5
    # the padded nodes' rows: large and finite, so an edge that escapes the mask shows in the loss and in every sum it enters
    z[N_REAL:] = (32.0 + 32.0 * torch.rand(N_NODES - N_REAL, d, generator=gen)) * (1 - 2 * (torch.rand(N_NODES - N_REAL, d, generator=gen) < 0.5).float())
    return z.to(dev(), dtype)


def _score_run(z, st, mode, y, pw, live=None):
    """(loss, logits, dL/dlogit, dL/dz) of the registered op on `st`: the live form when `live` is given"""
    from pangnn_amd import functional as PF
    from pangnn_amd import graph as G
    from pangnn_amd import torch_ops as T
    T._ready(st, G.NEED_BY_DST | G.NEED_BY_SRC)
    zz = z.clone().requires_grad_(True)
    m = PF.SCORE_MODES[mode]
    if live is None:
        loss, logits, g_l, _ = torch.ops.pangnn.edge_score_loss(zz, st._key_tensor, m, y, pw, st.num_edges)
    else:
        loss, logits, g_l, _ = torch.ops.pangnn.edge_score_loss_live(zz, st._key_tensor, m, y, pw, live)
    loss.backward()
    return loss.detach(), logits, g_l, zz.grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", ["dot", "cosine"])
@pytest.mark.parametrize("d", [16, 64, 256])
def test_scores_live_equals_the_list_cut_to_its_live_edges(d, mode, dtype):
    from pangnn_amd import functional as PF
    from pangnn_amd.graph import structure_of
    ei_cpu, y_cpu = _score_list()
    ei, y = ei_cpu.to(dev()), y_cpu.to(dev())
    z = _score_rows(d, dtype)
    pw = torch.tensor(PW, device=dev())
    st = structure_of(ei, N_NODES)
    for lv in SCORE_LIVES:
        m = min(max(lv, 0), E_ALL)
        live = torch.tensor([lv], dtype=torch.int64, device=dev())
        loss, logits, g_l, gz = _score_run(z, st, mode, y, pw, live)
        tag = (d, mode, lv)
        assert logits.shape == g_l.shape == (E_ALL,) and gz.shape == z.shape and gz.dtype == dtype, tag
        assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(gz.float()).all()) and bool(torch.isfinite(loss)), tag
        assert not bool(g_l[m:].any()), tag                                # exactly 0 on the padding
        if m == 0:
            assert float(loss) == 0.0 and not bool(g_l.any()) and not bool(gz.any()), tag
            continue
        cut = structure_of(ei[:, :m].contiguous(), N_NODES)
        rloss, rlogits, rg_l, rgz = _score_run(z, cut, mode, y[:m].contiguous(), pw)
        assert torch.equal(logits[:m], rlogits) and torch.equal(g_l[:m], rg_l), tag
        real_rows = N_REAL if m <= E_REAL else N_NODES                     # m > E_REAL: the tail's self loops are live edges
        assert torch.equal(gz[:real_rows], rgz[:real_rows]), tag           # same entries in the same order: the same bits
        assert not bool(gz[real_rows:].any()), tag                         # padded nodes: zero rows, cosine's diagonal term too
        ref64, bound = loss64(logits[:m], y[:m], PW), loss_bound(logits[:m], PW)
        print(f"d={d} {mode} live={lv}: loss {float(loss)!r} f64 {ref64!r} cut list {float(rloss)!r} bound {bound:.3e}")
        assert abs(float(loss) - ref64) <= bound, tag
    # the functional route hands out the same loss and logits, and the same gradient through autograd
    live = torch.tensor([E_REAL], dtype=torch.int64, device=dev())
    zz = z.clone().requires_grad_(True)
    l2, x2 = PF.edge_score_loss(zz, st, mode, y, pw, E_ALL, live=live)
    l2.backward()
    loss, logits, _, gz = _score_run(z, st, mode, y, pw, live)
    assert torch.equal(l2.detach(), loss) and torch.equal(x2, logits) and torch.equal(zz.grad, gz)


# ------------------------------------------------------------------------------------------------------------------
# 2. kernel level, mlp
# ------------------------------------------------------------------------------------------------------------------
E_MLP = 32 * 9 + 11
MLP_LIVES = (0, 1, 31, 32, 33, 150, E_MLP - 1, E_MLP, E_MLP + 5)
GRAD_NAMES = ("gp", "gq", "g_cv", "g_w2", "g_b2", "g_w3", "g_b3")


def _mlp_inputs(d, skip, sorted_list):
    gen = torch.Generator().manual_seed(1000 * d + 10 * skip + sorted_list)
    n = 40
    src = torch.randint(0, n, (E_MLP,), generator=gen)
    if sorted_list:
        src = src.sort().values
    ei = torch.stack([src, torch.randint(0, n, (E_MLP,), generator=gen)]).contiguous()
    r = lambda *s: torch.randn(*s, generator=gen)                          # noqa: E731
    t = dict(p=r(n, d) / d ** 0.5, q=r(n, d) / d ** 0.5, w2=r(d, d) / d ** 0.5, b2=0.1 * r(d), w3=r(d) / d ** 0.5, b3=0.1 * r(1),
             ex=torch.rand(E_MLP, generator=gen) if skip else None, cv=0.5 * r(d) if skip else None,
             y=(torch.rand(E_MLP, generator=gen) < 0.3).float())
    return n, ei.to(dev()), {k: None if v is None else v.to(dev()).contiguous() for k, v in t.items()}


def _mlp_run(n, ei, t, m=None, live=None):
    """functional._decoder_grads on the whole list with `live`, or on the list cut to m edges with denom = m"""
    from pangnn_amd import functional as PF
    from pangnn_amd.graph import EdgeStructure
    cut = slice(None) if m is None else slice(0, m)
    st = EdgeStructure(ei[:, cut].contiguous(), n)
    ex = None if t["ex"] is None else t["ex"][cut].contiguous()
    y = t["y"][cut].contiguous()
    pw = torch.tensor([PW], device=dev())
    r = PF._decoder_grads(t["p"], t["q"], st, ex, t["cv"], t["w2"], t["b2"], t["w3"], t["b3"], False, y=y, pw=pw,
                          denom=st.num_edges, live=live)
    torch.cuda.synchronize()
    return st, r[0], r[1], dict(zip(GRAD_NAMES, r[2:]))


@pytest.mark.parametrize("sorted_list", [True, False], ids=["sorted", "unsorted"])
@pytest.mark.parametrize("skip", [False, True], ids=["plain", "skip"])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_mlp_live_equals_the_list_cut_to_its_live_edges(d, skip, sorted_list):
    with strict_fp32(d == 64):
        n, ei, t = _mlp_inputs(d, skip, sorted_list)
        for lv in MLP_LIVES:
            m = min(max(lv, 0), E_MLP)
            live = torch.tensor([lv], dtype=torch.int64, device=dev())
            st, loss, logits, g = _mlp_run(n, ei, t, live=live)
            tag = (d, skip, sorted_list, lv)
            assert (st.runsum_plan() is not None) == sorted_list, tag      # run parts / segment sums
            assert logits.shape == (E_MLP,) and bool(torch.isfinite(logits).all()) and bool(torch.isfinite(loss).all()), tag
            for k, v in g.items():
                assert (v is None) == (k == "g_cv" and not skip), (tag, k)
                assert v is None or bool(torch.isfinite(v).all()), (tag, k)
            if m == 0:
                assert float(loss) == 0.0, tag
                assert all(v is None or not bool(v.any()) for v in g.values()), tag
                continue
            _, rloss, rlogits, rg = _mlp_run(n, ei, t, m=m)
            assert torch.equal(logits[:m], rlogits), tag
            ref64, bound = loss64(logits[:m], t["y"][:m], PW), loss_bound(logits[:m], PW)
            print(f"d={d} skip={skip} sorted={sorted_list} live={lv}: loss {float(loss)!r} f64 {ref64!r} cut {float(rloss)!r} "
                  f"bound {bound:.3e}")
            assert abs(float(loss) - ref64) <= bound, tag
            for k, v in g.items():
                if v is None:
                    continue
                scale = float(rg[k].abs().max())
                assert close(v, rg[k], atol=1e-5 * scale + 1e-9), (tag, k)


def test_the_given_gradient_backward_has_no_live_form():
    from pangnn_amd import functional as PF
    from pangnn_amd.graph import EdgeStructure
    n, ei, t = _mlp_inputs(32, False, True)
    live = torch.tensor([5], dtype=torch.int64, device=dev())
    with pytest.raises(ValueError, match="fused loss"):
        PF._decoder_f32(t["p"], t["q"], EdgeStructure(ei, n), None, None, t["w2"], t["b2"], t["w3"], t["b3"],
                        g_logits=torch.zeros(E_MLP, device=dev()), live=live)


# ------------------------------------------------------------------------------------------------------------------
# 3. end to end: train.ReplayedFreshStep on every decoder it now serves
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def dataset():
    """data set and schedule of tests/test_hip_parity.py::test_replayed_fresh_step_serves_every_batch"""
    from pangnn_amd import simulate
    ds = simulate.simulate_subgraph_dataset(300, 4, 0.3, 10, 2, seed=5, device=dev())
    h = ds._host()
    perm = torch.randperm(ds.num_graphs, generator=torch.Generator().manual_seed(3)).tolist()
    schedule = [perm[i:i + 32] for i in range(0, len(perm), 32)]
    big = sorted(range(ds.num_graphs), key=lambda i: h.edge[i] - h.edge[i + 1])[:32]      # the 32 largest sub-graphs
    schedule = schedule[:4] + [big] + schedule[4:7] + [perm[:5]]
    return ds, ds.class_balance(), schedule, big


def _reference_batch(ds, ids):
    """the disjoint union of the sub-graphs `ids` built with torch index ops (what Batch.from_data_list does)"""
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


CASES = {
    "cosine": dict(dims=[64, 128], decoder="cosine"),
    "dot": dict(dims=[64, 128], decoder="dot"),
    "d32": dict(dims=[32, 64]),
    "d128": dict(dims=[128, 128]),
    "d32-skip": dict(dims=[32, 64], skip_connections=True),
    "strict64": dict(dims=[64, 128]),
}


@pytest.mark.parametrize("case", list(CASES))
def test_replayed_fresh_step_serves_these_decoders(case):
    """test_replayed_fresh_step_serves_every_batch restated for the decoders and widths outside decoder16.hip:
      (i)  replaying the captured graph over the shuffled schedule == the same padded step run eagerly, bit for bit (loss,
           logits, every parameter after every step), including the batch that overflows the everyday buffers and the short last
           batch;
      (ii) the padded step == the unpadded fresh step (train_step on the index-op union): loss 1e-6, logits 1e-5, parameter
           gradients 1e-5 of their scale."""
    import pangnn_amd
    from pangnn_amd.train import ReplayedFreshStep, make_optimizer, train_step
    kw = CASES[case]
    ds, pw, schedule, big = dataset()
    h = ds._host()
    with strict_fp32(case == "strict64"):
        def make(capture):
            torch.manual_seed(0)
            model = pangnn_amd.AlternateGCN(dev(), None, False, **kw)
            opt = make_optimizer(model, capturable=True)
            return model, opt, ReplayedFreshStep(model, opt, ds, pw, 32, capture=capture, warmup=1, slack=1.2)

        ma, oa, sa = make(True)
        mb, ob, sb = make(False)
        assert not ds.fits(sa.spec, big) and ds.fits(sa.spec_worst, big)        # the schedule does exercise the second slot
        for k, ids in enumerate(schedule):
            la, xa = sa(ids)
            lb, xb = sb(ids)
            assert xa.shape == xb.shape == (sum(h.edge[i + 1] - h.edge[i] for i in ids),)
            assert torch.equal(la, lb) and torch.equal(xa, xb), (k, float(la), float(lb))
            assert bool(torch.isfinite(la))
            for p, q in zip(ma.parameters(), mb.parameters()):
                assert torch.equal(p, q), k
        assert len(sa._slots) == 2

        # (ii) against the unpadded step on the same union, from the same parameters (one step each, gradients compared)
        torch.manual_seed(0)
        mc = pangnn_amd.AlternateGCN(dev(), None, False, **kw)
        oc = make_optimizer(mc, capturable=True)
        for ids in (schedule[0], schedule[-1]):
            mc.load_state_dict(mb.state_dict())
            batch = _reference_batch(ds, ids)
            lc, xc = train_step(mc, oc, batch, batch.y, pw)
            lb, xb = sb(ids)
            print(f"{case}: padded loss {float(lb)!r} unpadded {float(lc)!r} max|dlogit| {float((xb - xc).abs().max()):.3e}")
            assert close(lb, lc, atol=1e-6, rtol=1e-6) and close(xb, xc, atol=1e-5, rtol=1e-5)
            for (k, p), (_, q) in zip(mb.named_parameters(), mc.named_parameters()):
                if q.grad is None:                           # a layer this topology does not use
                    assert p.grad is None, k
                    continue
                scale = float(q.grad.abs().max()) + 1e-12
                assert close(p.grad, q.grad, atol=1e-5 * scale + 1e-9, rtol=1e-4), k


# ------------------------------------------------------------------------------------------------------------------
# 4. what a padded batch still refuses
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(fused_decoder=False), dict(fused_decoder=False, decoder="cosine"),
                                dict(fused_decoder="pair_add")], ids=["literal-mlp", "literal-cosine", "pair-add"])
def test_a_non_fused_route_still_refuses_a_padded_batch(kw):
    import pangnn_amd
    ds, pw, schedule, _ = dataset()
    torch.manual_seed(0)
    model = pangnn_amd.AlternateGCN(dev(), None, False, dims=[64, 128], **kw)
    buf = ds.padded_buffers(ds.padded_spec(32))
    ds.set_graph_ids(buf, schedule[0])
    ds.collate_padded(buf)
    with pytest.raises(NotImplementedError, match="needs a fused training decoder"):
        model.loss_and_logits(buf, buf.y, pw)
