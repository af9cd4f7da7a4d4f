"""The width template of the strict-fp32 MLP link decoder on the GPU (csrc/decoder.hip through pangnn_amd.functional and
AlternateGCN): bit for bit against a float64 evaluation on the exact grid of tests/test_decoder_run_sums.py (whose exactness at
these widths tests/test_decoder_widths_host.py proves on the CPU) and the fused loss on the same grids at node_dim 32, 64
(the strict-fp32 mode) and 128; at 32 and 128 the whole model against the oracle, the route a model takes, non-finite values,
and bf16 autocast."""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

from test_decoder_run_sums import SUMS, decoder_reference
from test_decoder_widths_host import EXACT_SETS, EXACT_WIDTHS, WIDTHS, exact_inputs, set_id
from test_hip_parity import _check_logits_loss_grads_against_oracle, _pair, close

pytestmark = pytest.mark.gpu
NAN = float("nan")


def dev():
    return torch.device("cuda:0")


@contextlib.contextmanager
def _strict_fp32():
    """PF.DECODER_PRECISION = 0 for the duration: node_dim 64 then runs the template's instance (32 and 128 do in any mode)"""
    from pangnn_amd import functional as PF
    old, PF.DECODER_PRECISION = PF.DECODER_PRECISION, 0
    try:
        yield
    finally:
        PF.DECODER_PRECISION = old


def _f32(x):
    """the float64 reference as the float32 it must be matched against (exact: asserted by the CPU tests)"""
    y = x.float()
    assert torch.equal(y.double(), x)
    return y


def _on_device(inp, order, w3_scale=1.0):
    """(tables, edge_index, g, extra) on the device with the edges taken in `order` (None: as drawn, i.e. unsorted)"""
    td = {k: v.to(dev()).contiguous() for k, v in inp.t.items()}
    td["w3"] = td["w3"] * w3_scale
    idx = torch.arange(inp.e) if order is None else order
    ei = torch.stack([inp.src[idx], inp.dst[idx]]).to(dev()).contiguous()
    extra = None if inp.extra is None else inp.extra[idx].to(dev())
    return td, ei, inp.g[idx].to(dev()), extra


def _leaves(td):
    return {k: td[k].clone().requires_grad_(True) for k in ("P", "Q", "cvec", "W2", "b2", "w3", "b3")}


def _grads(lv, skip):
    got = dict(gP=lv["P"].grad, gQ=lv["Q"].grad, gW2=lv["W2"].grad, gb2=lv["b2"].grad, gw3=lv["w3"].grad, gb3=lv["b3"].grad)
    if skip:
        got["gcvec"] = lv["cvec"].grad
    return got


def _decoder_mlp(td, st, extra, g):
    from pangnn_amd import functional as PF
    lv = _leaves(td)
    out = PF.decoder_mlp(lv["P"], lv["Q"], st, extra, lv["cvec"] if extra is not None else None, lv["W2"], lv["b2"], lv["w3"],
                         lv["b3"])
    out.backward(g)
    return out.detach(), _grads(lv, extra is not None)


# ------------------------------------------------------------------------------------------------------------------
# 1. bit for bit on the exact grid
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", EXACT_SETS, ids=set_id)
@_strict_fp32()
def test_logits_and_gradients_bit_for_bit_on_the_exact_grid(s):
    """PF.decoder_mlp and its backward under a given dL/dlogit: torch.equal against the float64 reference, no tolerance.  The
    list sorted by source (run-sum parts inside the kernel) and as drawn (segment sums by source and by target); "one-source"
    and "own-source" are sorted lists with one part per tile and one part per edge.  The same call twice: the same bits."""
    from pangnn_amd.graph import EdgeStructure
    inp = exact_inputs(*s)
    orders = {"sorted": inp.by_src} if s[2] != "list" else {"sorted": inp.by_src, "unsorted": None}
    for name, order in orders.items():
        td, ei, g, extra = _on_device(inp, order)
        ref = decoder_reference({k: v.double() for k, v in td.items()}, ei[0], ei[1], g.double(), extra)
        st = EdgeStructure(ei, inp.n)
        assert (st.runsum_plan() is not None) == (name == "sorted" or inp.e == 1)
        out, got = _decoder_mlp(td, st, extra, g)
        bad = out != _f32(ref["logits"])
        assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {inp.e} logits differ, first {int(bad.nonzero()[0])}"
        for k in SUMS:
            if k == "gcvec" and extra is None:
                continue
            bad = got[k] != _f32(ref[k])
            assert not bool(bad.any()), f"{name} {k}: {int(bad.sum())} entries differ, first {bad.nonzero()[0].tolist()}"
        out2, got2 = _decoder_mlp(td, st, extra, g)
        assert torch.equal(out, out2) and all(torch.equal(got[k], got2[k]) for k in got), name


@pytest.mark.parametrize("d", EXACT_WIDTHS)
@_strict_fp32()
def test_empty_list(d):
    """num_edges == 0: no logits, every gradient zero (the reduction runs over a zeroed workspace)"""
    from pangnn_amd.graph import EdgeStructure
    inp = exact_inputs(d, True, "list", 33)
    td, _, _, _ = _on_device(inp, None)
    st = EdgeStructure(torch.zeros(2, 0, dtype=torch.int64, device=dev()), inp.n)
    out, got = _decoder_mlp(td, st, torch.zeros(0, device=dev()), torch.zeros(0, device=dev()))
    assert out.shape == (0,)
    for k, v in got.items():
        assert v is not None and not bool(v.any()), k


# ------------------------------------------------------------------------------------------------------------------
# 2. the fused loss on the same grids
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", EXACT_SETS, ids=set_id)
@_strict_fp32()
def test_fused_loss_on_the_exact_grid(s):
    """PF.decoder_loss with w3 / 64 (still exact; |logit| stays where the sigmoid is not saturated), y ~ Bernoulli(0.3),
    pos_weight 2.5, denom = E.  Logits: the float64 reference's and the forward kernel's, bit for bit.  Loss: 1e-6 + 1e-5 |ref|.
    Gradients: the float64 dL/dlogit of torch's BCE through the reference; on this grid only dL/dlogit is inexact and no relu
    mask can differ, so the error is summation error alone: <= 64 * 2^-24 * (largest sum of absolute terms of the tensor)."""
    from pangnn_amd import functional as PF
    from pangnn_amd.graph import EdgeStructure
    inp = exact_inputs(*s)
    skip = inp.extra is not None
    y_cpu = (torch.rand(inp.e, generator=torch.Generator().manual_seed(inp.e + inp.d)) < 0.3).float()
    pw = torch.tensor(2.5, device=dev())
    orders = {"sorted": inp.by_src} if s[2] != "list" else {"sorted": inp.by_src, "unsorted": None}
    for name, order in orders.items():
        td, ei, _, extra = _on_device(inp, order, w3_scale=1.0 / 64)
        y = (y_cpu if order is None else y_cpu[order]).to(dev())
        t64 = {k: v.double() for k, v in td.items()}
        x = decoder_reference(t64, ei[0], ei[1], torch.zeros(inp.e, device=dev()), extra)["logits"].requires_grad_(True)
        assert float(x.detach().abs().max()) < 40.0
        lref = F.binary_cross_entropy_with_logits(x, y.double(), pos_weight=pw.double())
        lref.backward()
        ref = decoder_reference(t64, ei[0], ei[1], x.grad, extra, magnitudes=True)
        st = EdgeStructure(ei, inp.n)
        lv = _leaves(td)
        loss, logits = PF.decoder_loss(lv["P"], lv["Q"], st, extra, lv["cvec"] if skip else None, lv["W2"], lv["b2"], lv["w3"],
                                       lv["b3"], y, pw, inp.e)
        loss.backward()
        got = _grads(lv, skip)
        with torch.no_grad():
            fwd = PF.decoder_mlp(td["P"], td["Q"], st, extra, td["cvec"] if skip else None, td["W2"], td["b2"], td["w3"], td["b3"])
        assert torch.equal(logits, _f32(ref["logits"])) and torch.equal(logits, fwd), name
        got_loss, want_loss = float(loss.detach()), float(lref.detach())
        err = abs(got_loss - want_loss)
        print(f"{set_id(s)} {name}: loss {got_loss:.9g} ref {want_loss:.9g} err {err:.2e}")
        assert err <= 1e-6 + 1e-5 * abs(want_loss), (name, got_loss, want_loss)
        for k in SUMS:
            if k == "gcvec" and not skip:
                continue
            unit = 2.0 ** -24 * float(ref["mag"][k].max())
            worst = float((got[k].double() - ref[k]).abs().max())
            print(f"    {k}: {worst / unit if unit else 0.0:.2f} units of 2^-24 max|terms|")
            assert worst <= 64 * unit, (name, k, worst / unit if unit else worst)


# ------------------------------------------------------------------------------------------------------------------
# 3. the whole model against the oracle
# ------------------------------------------------------------------------------------------------------------------
MODEL_FLAGS = [dict(), dict(skip_connections=True)]
flag_id = lambda f: "skip" if f else "default"            # noqa: E731


@pytest.mark.parametrize("flags", MODEL_FLAGS, ids=flag_id)
@pytest.mark.parametrize("dims", [(32, 64), (128, 128)], ids=lambda d: f"{d[0]}x{d[1]}")
@pytest.mark.parametrize("name", ["sim_200x4", "cfg1_2genomes", "cfg3_5genomes"])
def test_model_matches_the_oracle_at_both_widths(name, dims, flags):
    """logits within 1e-4 of the oracle, loss within 1e-5, every parameter gradient within FP64_DIRECT = 2e-5 of its scale of
    the float64 oracle (no flip band: flips=()); then loss_and_logits on the same inputs: logits bit-equal to the eval-mode
    forward, gradients within 1e-5 of their scale of the model(g) + criterion route"""
    g, gd, oracle, model = _pair(name, dims, dict(flags))
    out, _, _ = _check_logits_loss_grads_against_oracle(g, gd, oracle, model, tag=f"{name}/{dims[0]}/{flag_id(flags)}", flips=())
    assert type(out) is torch.Tensor                        # training-mode forward at these widths: a plain tensor
    first = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    model.zero_grad()
    pw = torch.tensor(float((g.y == 0).sum() / g.y.sum()), device=dev())
    loss, logits = model.loss_and_logits(gd, gd.y, pw)
    loss.backward()
    model.eval()
    with torch.no_grad():
        assert torch.equal(logits, model(gd))
    assert close(loss, F.binary_cross_entropy_with_logits(out.detach(), gd.y, pos_weight=pw), atol=1e-5, rtol=1e-5)
    for k, p in model.named_parameters():
        if k in first:
            scale = float(first[k].abs().max()) + 1e-30
            assert float((p.grad - first[k]).abs().max()) <= 1e-5 * scale, k


# ------------------------------------------------------------------------------------------------------------------
# 4. the route
# ------------------------------------------------------------------------------------------------------------------
def _count(monkeypatch, names):
    from pangnn_amd import functional as PF
    calls = {k: 0 for k in names}
    for k in names:
        def wrapped(*a, _f=getattr(PF, k), _k=k, **kw):
            calls[_k] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(PF, k, wrapped)
    return calls


def _forbid_literal_route(monkeypatch):
    from pangnn_amd import functional as PF

    def refuse(*a, **kw):
        raise AssertionError("the layer-by-layer decoder route was taken")
    monkeypatch.setattr(PF, "edge_pair_add", refuse)
    monkeypatch.setattr(PF, "edge_gather_concat", refuse)


@pytest.mark.parametrize("flags", MODEL_FLAGS, ids=flag_id)
@pytest.mark.parametrize("dims", [(32, 64), (128, 128)], ids=lambda d: f"{d[0]}x{d[1]}")
def test_models_at_both_widths_take_the_fused_route(dims, flags, monkeypatch):
    import pangnn_amd
    from pangnn_amd import train
    g, gd, oracle, model = _pair("sim_200x4", dims, dict(flags))
    pw = torch.tensor(float((g.y == 0).sum() / g.y.sum()), device=dev())
    literal = pangnn_amd.AlternateGCN(dev(), None, False, dims=list(dims), num_nodes=g.x.shape[0], fused_decoder=False, **flags)
    literal.load_state_dict(oracle.state_dict())
    literal.eval()
    calls = _count(monkeypatch, ("edge_gather_concat",))
    with torch.no_grad():
        want = literal(gd)
    assert calls["edge_gather_concat"] == 1                 # fused_decoder=False: the literal route, today's
    _forbid_literal_route(monkeypatch)
    with pytest.raises(AssertionError, match="layer-by-layer"):
        with torch.no_grad():
            literal(gd)
    calls = _count(monkeypatch, ("decoder_mlp_pq", "decoder_loss_pq"))
    model.eval()
    with torch.no_grad():
        out = model(gd)
    assert calls == dict(decoder_mlp_pq=1, decoder_loss_pq=0)
    assert float((out - want).abs().max()) <= 1e-5
    model.train()
    out = model(gd)
    assert type(out) is torch.Tensor and out.requires_grad
    torch.nn.BCEWithLogitsLoss(pos_weight=pw)(out, gd.y).backward()
    assert calls == dict(decoder_mlp_pq=2, decoder_loss_pq=0)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.mlp.parameters())
    model.zero_grad()
    loss, logits = model.loss_and_logits(gd, gd.y, pw)
    loss.backward()
    assert calls == dict(decoder_mlp_pq=2, decoder_loss_pq=1) and logits.shape == out.shape
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    loss2, _ = train.train_step(model, opt, gd, gd.y, pw)
    assert calls == dict(decoder_mlp_pq=2, decoder_loss_pq=2)
    first, second = float(loss.detach()), float(loss2)
    assert second == second and abs(second - first) <= 1e-6 + 1e-5 * abs(first)      # the same parameters: the same loss


# ------------------------------------------------------------------------------------------------------------------
# 5. non-finite values
# ------------------------------------------------------------------------------------------------------------------
NF_N = 97
NF_CASES = [(d, skip, e, inj) for d in WIDTHS for skip in (False, True) for e in (33, 1000) for inj in ("nan_p", "nan_unused")]


@functools.lru_cache(maxsize=None)
def nonfinite_case(d, skip, e, inject):
    """tests/test_nonfinite.py's decoder case at width d: a source-sorted list over nodes 1 .. 95 (nodes 0 and 96 are referenced
    by no edge; node 0 is the row the lanes past the end of the last tile gather), and torch's float64 results"""
    gen = torch.Generator().manual_seed(1000 * d + 2 * e + skip)
    rn = lambda *s: torch.randn(*s, generator=gen)            # noqa: E731
    src, dst = (torch.randint(1, NF_N - 1, (e,), generator=gen) for _ in range(2))
    order = torch.argsort(src * NF_N + dst)
    ei = torch.stack([src[order], dst[order]])
    P, Q, W2, b2, w3, b3, cv = rn(NF_N, d), rn(NF_N, d), rn(d, d) / 8 * (64 / d) ** 0.5, rn(d), rn(d), rn(1), rn(d)
    extra = torch.rand(e, generator=gen) if skip else None
    y = (torch.rand(e, generator=gen) < 0.3).float()
    zeroed = None
    if inject == "nan_p":
        P[int(ei[0, 0])] = NAN
    else:
        zeroed = (P.clone(), Q.clone())
        for t in zeroed:
            t[0], t[NF_N - 1] = 0.0, 0.0
        P[0], P[NF_N - 1], Q[0], Q[NF_N - 1] = NAN, NAN, NAN, -float("inf")
    lv = [t.clone().double().requires_grad_(True) for t in (P, Q, W2, b2, w3, b3, cv)]
    h1 = lv[0][ei[0]] + lv[1][ei[1]]
    if skip:
        h1 = h1 + extra.double().unsqueeze(1) * lv[6]
    ref = torch.relu(torch.relu(h1) @ lv[2].t() + lv[3]) @ lv[4] + lv[5]
    lref = F.binary_cross_entropy_with_logits(ref, y.double(), pos_weight=torch.tensor(2.5, dtype=torch.float64))
    lref.backward()
    grads = [None if (k == 6 and not skip) else lv[k].grad for k in range(7)]
    return dict(ei=ei, tensors=(P, Q, W2, b2, w3, b3, cv), extra=extra, y=y, zeroed=zeroed, logits=ref.detach(),
                loss=lref.detach(), grads=grads)


def _run_nonfinite(c, skip, e, tables=None):
    from pangnn_amd import functional as PF
    from pangnn_amd.graph import EdgeStructure
    P, Q = tables if tables is not None else c["tensors"][:2]
    st = EdgeStructure(c["ei"].to(dev()), NF_N)
    ex = c["extra"].to(dev()) if skip else None
    y, pw = c["y"].to(dev()), torch.tensor(2.5, device=dev())
    out = {}
    gl = [t.clone().to(dev()).requires_grad_(True) for t in (P, Q) + c["tensors"][2:]]
    loss, logits = PF.decoder_loss(gl[0], gl[1], st, ex, gl[6] if skip else None, gl[2], gl[3], gl[4], gl[5], y, pw, e)
    loss.backward()
    out["fused"] = (logits.detach(), loss.detach(), [None if (k == 6 and not skip) else gl[k].grad for k in range(7)])
    gl2 = [t.clone().to(dev()).requires_grad_(True) for t in (P, Q) + c["tensors"][2:]]
    out2 = PF.decoder_mlp(gl2[0], gl2[1], st, ex, gl2[6] if skip else None, gl2[2], gl2[3], gl2[4], gl2[5])
    l2 = F.binary_cross_entropy_with_logits(out2, y, pos_weight=pw)
    l2.backward()
    out["mlp"] = (out2.detach(), l2.detach(), [None if (k == 6 and not skip) else gl2[k].grad for k in range(7)])
    return out


@pytest.mark.parametrize("d,skip,e,inject", NF_CASES)
def test_nonfinite_values_pass_like_torch(d, skip, e, inject):
    """a NaN row of P that one source's edges reference: those logits, the loss and every gradient tensor non-finite exactly
    where torch's float64 evaluation is (logits position by position, gradients tensor by tensor: the bounds and helpers of
    tests/test_nonfinite.py); NaN / -inf rows no edge references (node 0 among them, which the padded lanes of the last tile
    of E = 33 gather): bit-equal to the same rows zeroed"""
    from test_nonfinite import allclose_bound, assert_same_nonfinite, assert_same_nonfinite_tensorwise, scaled_bound
    c = nonfinite_case(d, skip, e, inject)
    bad = int((~torch.isfinite(c["logits"])).sum())
    assert (1 <= bad <= e // 2 and not torch.isfinite(c["loss"])) if inject == "nan_p" else (bad == 0 and torch.isfinite(c["loss"]))
    res = _run_nonfinite(c, skip, e)
    for route, (logits, loss, grads) in res.items():
        tag = f"{route} d={d} E={e} skip={skip} {inject}"
        assert_same_nonfinite(logits, c["logits"], finite_bound=allclose_bound(1.6e-5, 2e-6), what=tag + " logits")
        assert_same_nonfinite(loss, c["loss"], finite_bound=allclose_bound(1e-6, 1e-5), what=tag + " loss")
        for k, want in enumerate(c["grads"]):
            if want is not None:
                assert_same_nonfinite_tensorwise(grads[k], want, finite_bound=scaled_bound(1e-6 if e >= 1000 else 8e-6),
                                                 what=f"{tag} gradient {k}")
    if inject == "nan_unused":
        zero = _run_nonfinite(c, skip, e, tables=c["zeroed"])
        for route in res:
            (lg, ls, gr), (lg0, ls0, gr0) = res[route], zero[route]
            assert torch.equal(lg, lg0) and torch.equal(ls, ls0), route
            for k in range(7):
                if gr[k] is not None:
                    assert torch.equal(gr[k], gr0[k]), (route, k)


# ------------------------------------------------------------------------------------------------------------------
# 6. bf16 autocast
# ------------------------------------------------------------------------------------------------------------------
def test_training_step_under_bf16_autocast_takes_the_fused_route(monkeypatch):
    g, gd, _, model = _pair("sim_200x4", (32, 64), {})
    pw = torch.tensor(float((g.y == 0).sum() / g.y.sum()), device=dev())
    _forbid_literal_route(monkeypatch)
    calls = _count(monkeypatch, ("decoder_mlp_pq", "decoder_loss_pq"))
    with torch.autocast("cuda", torch.bfloat16):
        out = model(gd)
        loss = torch.nn.BCEWithLogitsLoss(pos_weight=pw)(out.float(), gd.y)
    loss.backward()
    assert type(out) is torch.Tensor and out.dtype == torch.float32 and bool(torch.isfinite(loss))
    model.zero_grad()
    with torch.autocast("cuda", torch.bfloat16):
        loss, logits = model.loss_and_logits(gd, gd.y, pw)
    loss.backward()
    assert logits.dtype == torch.float32 and bool(torch.isfinite(loss)) and calls == dict(decoder_mlp_pq=1, decoder_loss_pq=1)
