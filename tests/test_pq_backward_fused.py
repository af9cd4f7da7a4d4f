"""The backward of the decoder's P | Q layer taken straight from the run parts of the S and T kernels
(pangnn_linear_act_backward_parts_f32, pangnn::decoder_loss_z) against the unfused sequence on the same inputs: two
pangnn_spmm_csr_f32 part sums into one [N, 128] matrix, then pangnn_linear_dgrad_mixed and pangnn_linear_act_wgrad_mixed.
Every comparison is torch.equal: the fused kernel forms the same row sums in the same order and runs the same products in the
same tile-to-wave assignment, so no tolerance is involved anywhere."""
import os
from contextlib import contextmanager
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENV = "PANGNN_FUSED_PQ_BWD"


# ------------------------------------------------------------------------------------------------------ 1. the kernel
def _part_table(n, gen, long_row):
    """(parts [n_parts, 64], rowptr int64 [n + 1]): counts from {0, 1, 2, 3}, first and last row empty, one row of 40 parts,
    some -0.0 entries, one row whose parts are all +0 and one whose single part is all -0"""
    cnt = torch.randint(0, 4, (n,), generator=gen)
    cnt[0] = 0
    cnt[-1] = 0
    if n >= 3:
        cnt[long_row] = 40
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(cnt, 0)
    n_parts = int(rowptr[-1])
    parts = torch.randn(max(n_parts, 1), 64, generator=gen)
    parts[torch.rand(parts.shape, generator=gen) < 0.05] = -0.0
    filled = [r for r in range(n) if cnt[r] > 0 and r != long_row]
    if filled:
        r = filled[len(filled) // 2]
        parts[rowptr[r]:rowptr[r + 1]] = 0.0                       # an all-zero row
    single = [r for r in range(n) if cnt[r] == 1]
    if single:
        parts[rowptr[single[-1]]] = -0.0                          # -0 + (+0) = +0, as the part sum gives it
    return parts[:n_parts].contiguous(), rowptr


def _kernel_case(n, in_act, seed):
    gen = torch.Generator().manual_seed(seed)
    ps, rs = _part_table(n, gen, n // 2)
    pt, rt = _part_table(n, gen, n // 3 + 1 if n >= 3 else 0)
    x = torch.randn(n, 64, generator=gen)                          # both signs: ELU and ELU' take both branches
    w = torch.randn(128, 64, generator=gen) * 0.2
    return [t.to(DEV) for t in (ps, rs, pt, rt, x, w)]


def _unfused(ps, rs, pt, rt, x, w, in_act):
    from pangnn_amd import _lib
    from pangnn_amd import functional as PF
    lib, n = _lib.load(), x.shape[0]
    g = torch.empty(n, 128, device=DEV)
    for parts, rowptr, out in ((ps, rs, g[:, :64]), (pt, rt, g[:, 64:])):
        if parts.shape[0] == 0:                                   # (a table without parts: the sum of nothing)
            parts = torch.zeros(1, 64, device=DEV)
        PF._sum_parts(SimpleNamespace(part_rowptr=rowptr), parts, n, out)
    gx, gw, gb = torch.empty(n, 64, device=DEV), torch.empty(128, 64, device=DEV), torch.empty(128, device=DEV)
    ws_bytes = lib.pangnn_linear_wgrad_workspace_bytes(64, 128)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    with _lib.device_guard(x.device):
        _lib.check(lib.pangnn_linear_dgrad_mixed(g.data_ptr(), 0, 128, w.data_ptr(), gx.data_ptr(), 0, 64, n, 64, 128,
                                                 x.data_ptr() if in_act else None, 0, 64 if in_act else 0, _lib.stream_ptr()),
                   "pangnn_linear_dgrad_mixed")
        _lib.check(lib.pangnn_linear_act_wgrad_mixed(g.data_ptr(), 0, 128, x.data_ptr(), 0, 64, n, 64, 128, in_act,
                                                     gw.data_ptr(), gb.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr()),
                   "pangnn_linear_act_wgrad_mixed")
    return gx, gw, gb


def _fused(ps, rs, pt, rt, x, w, in_act):
    from pangnn_amd import _lib
    lib, n = _lib.load(), x.shape[0]
    gx = torch.full((n, 64), float("nan"), device=DEV)
    gw, gb = torch.full((128, 64), float("nan"), device=DEV), torch.full((128,), float("nan"), device=DEV)
    ws_bytes = lib.pangnn_linear_wgrad_workspace_bytes(64, 128)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    with _lib.device_guard(x.device):
        _lib.check(lib.pangnn_linear_act_backward_parts_f32(
            ps.data_ptr() if ps.shape[0] else None, rs.data_ptr(), ps.shape[0], pt.data_ptr() if pt.shape[0] else None,
            rt.data_ptr(), pt.shape[0], x.data_ptr(), 64, w.data_ptr(), n, 64, 128, in_act, gx.data_ptr(), 64, gw.data_ptr(),
            gb.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr()), "pangnn_linear_act_backward_parts_f32")
    return gx, gw, gb


def _sizes():
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    # the last: every wave of a full grid gets a second tile (accumulators carried) and the last tile is partial
    return [1, 31, 32, 33, 129, 4 * 32 * cus + 37]


@pytest.mark.parametrize("in_act", [0, 1])
@pytest.mark.parametrize("n", _sizes())
def test_kernel_equals_the_four_launches(n, in_act):
    case = _kernel_case(n, in_act, seed=n + in_act)
    ref = _unfused(*case, in_act)
    got = _fused(*case, in_act)
    for name, a, b in zip(("gx", "gw", "gb"), got, ref):
        assert torch.equal(a, b), (name, n, in_act, float((a - b).abs().max()))
        # bit for bit, the sign of zero included (torch.equal takes -0 == +0)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, "bits")


# ------------------------------------------------------------------------------------------------------ 2. - 5. the model
@contextmanager
def _env(value):
    old = os.environ.get(ENV)
    if value is None:
        os.environ.pop(ENV, None)
    else:
        os.environ[ENV] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = old


@contextmanager
def _ctypes_route():
    """what bench.py's timed loop sets: a KERNEL_TIMER holding the decoder tags sends the decoder over ctypes"""
    from pangnn_amd import functional as PF
    old, PF.KERNEL_TIMER = PF.KERNEL_TIMER, {"dec.bwd": [], "dec.dgrad": [], "dec.fwd": []}
    try:
        yield PF.KERNEL_TIMER
    finally:
        PF.KERNEL_TIMER = old


_GRAPH = {}


def _sim_graph():
    """a few hundred nodes, computed once and left unchanged; every user takes a fresh holder of the same tensors"""
    if "g" not in _GRAPH:
        from pangnn_amd import simulate
        _GRAPH["g"] = simulate.simulate_graph(100, 4, 0.3, 10, 2, seed=11, device=DEV)
    g = _GRAPH["g"]
    return SimpleNamespace(x=g.x, edge_index=g.edge_index, edge_attr=g.edge_attr, y=g.y,
                           neighbour_edge_index=g.neighbour_edge_index, class_balance=g.class_balance)


def _model(**flags):
    import pangnn_amd
    torch.manual_seed(0)
    return pangnn_amd.AlternateGCN(DEV, None, False, dims=[64, 128], **flags)


def _grads(model):
    return {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def _train_step(model, g, env, timer=False):
    """one train.train_step from the model's CURRENT parameters (the caller restores them); (loss, logits, grads)"""
    from pangnn_amd.train import train_step
    opt = torch.optim.SGD(model.parameters(), lr=0.0)            # the step leaves the parameters where they are
    with _env(env):
        if timer:
            with _ctypes_route():
                loss, logits = train_step(model, opt, g, g.y, g.class_balance)
        else:
            loss, logits = train_step(model, opt, g, g.y, g.class_balance)
    return loss.clone(), logits.clone(), _grads(model)


def _assert_same(a, b, what):
    assert torch.equal(a[0], b[0]), (what, "loss")
    assert torch.equal(a[1], b[1]), (what, "logits")
    assert a[2].keys() == b[2].keys() and len(a[2]) >= 8, (what, sorted(a[2]))
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), (what, k, float((a[2][k] - b[2][k]).abs().max()))


def _fused_calls():
    """counts the calls of the fused entry point on either route (the library's own counter does not exist: a dispatch spy
    would switch the route off, so the two Python entry points are wrapped)"""
    from pangnn_amd import functional as PF
    calls = []
    orig = PF.decoder_loss_z

    def spy(*a, **k):
        calls.append(1)
        return orig(*a, **k)
    return calls, orig, spy


@pytest.mark.parametrize("skip", [False, True], ids=["default", "skip"])
def test_train_step_is_bit_identical_on_both_routes(skip, monkeypatch):
    from pangnn_amd import functional as PF
    g, model = _sim_graph(), _model(skip_connections=skip)
    calls, _, spy = _fused_calls()
    monkeypatch.setattr(PF, "decoder_loss_z", spy)
    res = {}
    for route in ("ops", "ctypes"):
        fused = _train_step(model, g, None, timer=route == "ctypes")
        assert len(calls) == 1, "the fused operator did not take the step"
        calls.clear()
        plain = _train_step(model, g, "0", timer=route == "ctypes")
        assert not calls, "PANGNN_FUSED_PQ_BWD=0 must keep the unfused route"
        _assert_same(fused, plain, route)
        res[route] = fused
    _assert_same(res["ops"], res["ctypes"], "ops vs ctypes")


@pytest.mark.parametrize("route", ["ops", "ctypes"])
def test_upstream_gradient_of_two(route):
    """a power of two commutes with every rounding: scaling gz, gw_pq, gb_pq after the fused kernel equals scaling the
    [N, 128] gradient before the unfused products"""
    g, model = _sim_graph(), _model()
    outs = []
    for env in (None, "0"):
        model.zero_grad(set_to_none=True)
        with _env(env):
            if route == "ctypes":
                with _ctypes_route():
                    loss, logits = model.loss_and_logits(g, g.y, g.class_balance)
                    loss.backward(torch.tensor(2.0, device=DEV))
            else:
                loss, logits = model.loss_and_logits(g, g.y, g.class_balance)
                loss.backward(torch.tensor(2.0, device=DEV))
        outs.append((loss.detach().clone(), logits.clone(), _grads(model)))
    _assert_same(outs[0], outs[1], route)


def test_compiled_step_is_one_graph_with_the_fused_operator():
    g, model = _sim_graph(), _model()

    def step(fn):
        model.zero_grad(set_to_none=True)
        loss, logits = fn(g, g.y, g.class_balance)
        loss.backward()
        return loss.detach().clone(), logits.detach().clone(), _grads(model)

    eager = step(model.loss_and_logits)
    graphs = []

    def backend(gm, example_inputs):
        from torch._dynamo.backends.debugging import aot_eager
        graphs.append([str(n.target) for n in gm.graph.nodes if n.op == "call_function"])
        return aot_eager(gm, example_inputs)

    torch._dynamo.reset()
    try:
        compiled = torch.compile(model.loss_and_logits, backend=backend, fullgraph=True)
        _assert_same(eager, step(compiled), "compiled")
        assert len(graphs) == 1, f"{len(graphs)} graphs"
        assert any("decoder_loss_z" in t for t in graphs[0]), graphs[0]
    finally:
        torch._dynamo.reset()


def _run(model, g, env, autocast=False):
    model.zero_grad(set_to_none=True)
    with _env(env), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        loss, logits = model.loss_and_logits(g, g.y, getattr(g, "class_balance", None))
    loss.backward()
    return loss.detach().clone(), logits.detach().clone(), _grads(model)


def _assert_routed_away(model, g, monkeypatch, **kw):
    from pangnn_amd import functional as PF
    calls, _, spy = _fused_calls()
    monkeypatch.setattr(PF, "decoder_loss_z", spy)
    default = _run(model, g, None, **kw)
    assert not calls, "the guard conditions must route this call away from the fused operator"
    _assert_same(default, _run(model, g, "0", **kw), "fallback")


def test_fallback_padded_batch(monkeypatch):
    from pangnn_amd import simulate
    ds = simulate.simulate_subgraph_dataset(300, 4, 0.3, 10, 2, seed=5, device=DEV)
    buf = ds.padded_buffers(ds.padded_spec(32))
    ds.set_graph_ids(buf, list(range(7)))
    ds.collate_padded(buf)
    assert getattr(buf, "live_edges", None) is not None
    _assert_routed_away(_model(), buf, monkeypatch)


def test_fallback_bf16_autocast_rows(monkeypatch):
    _assert_routed_away(_model(), _sim_graph(), monkeypatch, autocast=True)


def test_fallback_unsorted_edge_list(monkeypatch):
    g = _sim_graph()
    perm = torch.randperm(g.edge_index.shape[1], generator=torch.Generator().manual_seed(3)).to(DEV)
    g.edge_index, g.edge_attr, g.y = g.edge_index[:, perm].contiguous(), g.edge_attr[perm].contiguous(), g.y[perm].contiguous()
    assert not bool((g.edge_index[0][1:] >= g.edge_index[0][:-1]).all())
    _assert_routed_away(_model(), g, monkeypatch)


def test_deferred_handle_reaches_the_fused_operator_and_still_materialises(monkeypatch):
    """training-mode forward() hands out a DeferredLogits: torch's criterion on it is the fused pass (the new operator where it
    applies), any other use computes P | Q and runs the inference kernel; both bit-equal to PANGNN_FUSED_PQ_BWD=0"""
    from pangnn_amd import functional as PF
    g, model = _sim_graph(), _model()
    model.train()
    calls, _, spy = _fused_calls()
    monkeypatch.setattr(PF, "decoder_loss_z", spy)
    outs = []
    for env in (None, "0"):
        model.zero_grad(set_to_none=True)
        with _env(env):
            out = model(g)
            assert out.device.type == "cuda"
            loss = torch.nn.BCEWithLogitsLoss(pos_weight=g.class_balance)(out, g.y)
            loss.backward()
            with torch.no_grad():
                probs = torch.sigmoid(model(g))                   # a use that is not the criterion: inference kernel
        outs.append((loss.detach().clone(), probs.clone(), _grads(model)))
        assert len(calls) == (1 if env is None else 0)
        calls.clear()
    _assert_same(outs[0], outs[1], "deferred")
    direct = _run(model, g, None)
    assert torch.equal(direct[0], outs[0][0])
    for k in direct[2]:
        assert torch.equal(direct[2][k], outs[0][2][k]), k
