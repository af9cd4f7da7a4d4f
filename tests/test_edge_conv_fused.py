"""The fused EdgeConv (csrc/edge_conv.hip, functional.edge_conv, torch.ops.pangnn.edge_conv, EdgeConv.forward) against
oracle.gcn_oracle.EdgeConvOracle evaluated in fp64 on the CPU with the same state_dict.

The arg-max is discontinuous, so nothing is excluded and nothing compared edge by edge: the forward value is compared as is
(max is 1-Lipschitz), the kernel's `arg` is checked for VALIDITY (the fp64 message it names is the fp64 row maximum to 1e-4)
and the backward is compared with fp64 autograd through the fp64 messages selected at the kernel's own `arg`."""
import functools

import pytest
import torch

from conftest import random_graph
from oracle import gcn_oracle as go

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-4                       # atol = rtol: the project's north-star tolerance
GRAD_ATOL, GRAD_RTOL = 1e-4, 1e-3    # the existing EdgeConv test's bounds


def dev():
    return torch.device("cuda:0")


def degree_graph():
    """target degrees 1, 31, 32, 33, 64, 65 in consecutive rows: rows start and end on, before and after the 32-entry tile
    boundaries of the by-target CSR; E = 226 is no multiple of 32.  Edge order shuffled."""
    gen = torch.Generator().manual_seed(11)
    n = 12
    dst = torch.cat([torch.full((d,), r, dtype=torch.int64) for r, d in enumerate((1, 31, 32, 33, 64, 65))])
    src = torch.randint(0, n, (dst.shape[0],), generator=gen)
    order = torch.randperm(dst.shape[0], generator=gen)
    return n, torch.stack([src[order], dst[order]])


@functools.lru_cache(maxsize=None)
def graph(name):
    """(num_nodes, edge_index int64 [2, E]) on the CPU"""
    if name == "rand300":
        return 300, random_graph(300, 2500, seed=9)[0]
    if name == "hub":
        return 40, random_graph(40, 9500, seed=4, hub=9000)[0]          # one row past the 8192 hub threshold
    if name == "degrees":
        return degree_graph()
    n, e = {"n1e0": (1, 0), "n7e1": (7, 1), "n33e5000": (33, 5000)}[name]
    return n, random_graph(n, e, seed=n)[0]


GRAPHS = ("rand300", "hub", "n1e0", "n7e1", "n33e5000", "degrees")


@functools.lru_cache(maxsize=None)
def case(name, c, out, neg=False):
    """oracle (fp32 parameters), x, upstream gradient and the fp64 reference (output, messages [E, out]); computed once"""
    n, ei = graph(name)
    torch.manual_seed(1000 * c + out + len(name))
    ref_m = go.EdgeConvOracle(c, out)
    if neg:                          # every message negative: small weights, b2 = -5
        with torch.no_grad():
            for p in ref_m.parameters():
                p.mul_(0.05)
            ref_m.mlp[2].bias.fill_(-5.0)
    x = torch.randn(n, c)
    gsel = torch.randn(n, out)
    m64 = go.EdgeConvOracle(c, out).double()
    m64.load_state_dict({k: v.double() for k, v in ref_m.state_dict().items()})
    with torch.no_grad():
        x64 = x.double()
        msg64 = m64.mlp(torch.cat([x64[ei[1]], x64[ei[0]] - x64[ei[1]]], dim=1))
        ref64 = m64(x64, ei)
    return ref_m, x, gsel, ref64, msg64


def fused_module(ref_m, c, out):
    import pangnn_amd
    m = pangnn_amd.EdgeConv(c, out).to(dev())
    m.load_state_dict(ref_m.state_dict())
    return m


def run_fused(name, c, out, neg=False):
    """one forward + backward through PF.edge_conv; returns (out, arg, x.grad, {param: grad}) on the CPU"""
    from pangnn_amd import functional as PF
    from pangnn_amd.graph import structure_of
    n, ei = graph(name)
    ref_m, x, gsel, _, _ = case(name, c, out, neg)
    m = fused_module(ref_m, c, out)
    xg = x.to(dev()).requires_grad_(True)
    st = structure_of(ei.to(dev()), n)
    y, arg = PF.edge_conv(xg, m.mlp[0].weight, m.mlp[0].bias, m.mlp[2].weight, m.mlp[2].bias, st, return_arg=True)
    assert not arg.requires_grad and arg.dtype == torch.int32 and y.shape == arg.shape == (n, out)
    y.backward(gsel.to(dev()))
    torch.cuda.synchronize()
    return y.detach().cpu(), arg.cpu(), xg.grad.cpu(), {k: p.grad.cpu() for k, p in m.named_parameters()}


def reference_grads(name, c, out, arg, neg=False):
    """fp64 autograd through the fp64 messages selected at the kernel's own arg"""
    n, ei = graph(name)
    ref_m, x, gsel, _, _ = case(name, c, out, neg)
    m64 = go.EdgeConvOracle(c, out).double()
    m64.load_state_dict({k: v.double() for k, v in ref_m.state_dict().items()})
    x64 = x.double().requires_grad_(True)
    msg = m64.mlp(torch.cat([x64[ei[1]], x64[ei[0]] - x64[ei[1]]], dim=1))
    a = arg.long()
    if msg.shape[0] == 0:
        sel = torch.zeros(n, out, dtype=torch.float64) + 0.0 * x64.sum() + sum(0.0 * p.sum() for p in m64.parameters())
    else:
        sel = torch.where(a >= 0, msg.gather(0, a.clamp(min=0)), torch.zeros((), dtype=torch.float64))
    sel.backward(gsel.double())
    return x64.grad, {k: p.grad for k, p in m64.named_parameters()}


def check_forward_and_arg(name, c, out, y, arg, neg=False):
    n, ei = graph(name)
    _, _, _, ref64, msg64 = case(name, c, out, neg)
    err = (y.double() - ref64).abs()
    print(f"{name} C={c} out={out}: max |out - fp64| = {err.max().item() if err.numel() else 0.0:.3e}")
    assert torch.allclose(y.double(), ref64, atol=FWD_TOL, rtol=FWD_TOL)
    has = torch.zeros(n, dtype=torch.bool)
    has[ei[1]] = True
    assert (arg[~has] == -1).all() and (arg[has] >= 0).all() and (arg < ei.shape[1]).all()
    if has.any():
        a = arg[has].long()
        rows = torch.nonzero(has).squeeze(1)
        assert (ei[1][a] == rows[:, None]).all(), "arg names an edge of another target row"
        row_max = ref64[has]                                  # fp64 maxima of the rows with in-edges
        gap = (row_max - msg64.gather(0, a)).abs().max().item()
        print(f"{name} C={c} out={out}: max (fp64 row max - fp64 message at arg) = {gap:.3e}")
        assert gap <= 1e-4


@pytest.mark.parametrize("name", GRAPHS)
@pytest.mark.parametrize("out", [64, 128])
@pytest.mark.parametrize("c", [8, 64])
def test_fused_edge_conv_matches_fp64_oracle(name, c, out):
    y, arg, gx, gp = run_fused(name, c, out)
    check_forward_and_arg(name, c, out, y, arg)
    rx, rp = reference_grads(name, c, out, arg)
    print(f"{name} C={c} out={out}: max |x.grad - fp64| = {(gx.double() - rx).abs().max().item():.3e}")
    assert torch.allclose(gx.double(), rx, atol=GRAD_ATOL, rtol=GRAD_RTOL)
    for k in ("mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias"):
        print(f"  {k}: max |grad - fp64| = {(gp[k].double() - rp[k]).abs().max().item():.3e}")
        assert torch.allclose(gp[k].double(), rp[k], atol=GRAD_ATOL, rtol=GRAD_RTOL), k


def test_all_negative_rows_keep_their_negative_maximum():
    """the running maximum starts from the first edge, not from 0; rows without in-edges are exactly 0"""
    n, ei = graph("rand300")
    y, arg, gx, gp = run_fused("rand300", 64, 64, neg=True)
    check_forward_and_arg("rand300", 64, 64, y, arg, neg=True)
    has = torch.zeros(n, dtype=torch.bool)
    has[ei[1]] = True
    assert (~has).any() and (y[has] < -1.0).all() and (y[~has] == 0).all()
    rx, rp = reference_grads("rand300", 64, 64, arg, neg=True)
    assert torch.allclose(gx.double(), rx, atol=GRAD_ATOL, rtol=GRAD_RTOL)
    assert torch.allclose(gp["mlp.2.bias"].double(), rp["mlp.2.bias"], atol=GRAD_ATOL, rtol=GRAD_RTOL)


def test_rows_without_in_edges_get_no_gradient_from_gu():
    from pangnn_amd import torch_ops
    from pangnn_amd.graph import structure_of
    n, ei = graph("rand300")
    torch.manual_seed(5)
    st = structure_of(ei.to(dev()), n)
    u = torch.randn(n, 64, device=dev(), requires_grad=True)
    v = torch.randn(n, 64, device=dev(), requires_grad=True)
    w2, b2 = torch.randn(64, 64, device=dev()) / 8, torch.randn(64, device=dev())
    y, arg = torch_ops.edge_conv(u, v, w2, b2, st)
    y.backward(torch.randn(n, 64, device=dev()))
    has = torch.zeros(n, dtype=torch.bool)
    has[ei[1]] = True
    assert (u.grad.cpu()[~has] == 0).all() and (u.grad.cpu()[has] != 0).any()
    is_src = torch.zeros(n, dtype=torch.bool)
    is_src[ei[0]] = True
    assert (v.grad.cpu()[~is_src] == 0).all()


def test_duplicate_edges_resolve_to_the_lower_id():
    """edges 1 and 3 of random_graph duplicate edges 0 and 2: equal messages, the first maximum in ascending id wins"""
    n, ei = graph("rand300")
    assert torch.equal(ei[:, 0], ei[:, 1]) and torch.equal(ei[:, 2], ei[:, 3])
    for c, out in ((8, 64), (64, 128)):
        _, arg, _, _ = run_fused("rand300", c, out)
        assert not (arg == 1).any() and not (arg == 3).any()


@pytest.mark.parametrize("name", ["hub", "rand300"])
def test_two_runs_are_bit_equal(name):
    a, b = run_fused(name, 64, 64), run_fused(name, 64, 64)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


def _forward_with_switch(m, x, ei, flag):
    from pangnn_amd import functional as PF
    old, PF.FUSE_EDGE_CONV = PF.FUSE_EDGE_CONV, flag
    try:
        return m(x, ei)
    finally:
        PF.FUSE_EDGE_CONV = old


def test_fused_and_literal_routes_agree():
    n, ei = graph("rand300")
    ref_m, x, _, ref64, _ = case("rand300", 64, 64)
    m = fused_module(ref_m, 64, 64)
    xd, eid = x.to(dev()), ei.to(dev())
    with torch.no_grad():
        fused, literal = _forward_with_switch(m, xd, eid, True), _forward_with_switch(m, xd, eid, False)
    assert torch.allclose(fused, literal, atol=FWD_TOL, rtol=FWD_TOL)
    assert torch.allclose(fused.cpu().double(), ref64, atol=FWD_TOL, rtol=FWD_TOL)


def test_a_subclass_that_overrides_message_keeps_its_own_definition():
    import pangnn_amd

    class PlainCat(pangnn_amd.EdgeConv):
        def message(self, x_i, x_j):
            return self.mlp(torch.cat([x_i, x_j], dim=1))

    n, ei = graph("rand300")
    ref_m, x, _, _, _ = case("rand300", 64, 64)
    m = PlainCat(64, 64).to(dev())
    m.load_state_dict(ref_m.state_dict())
    with torch.no_grad():
        y = m(x.to(dev()), ei.to(dev())).cpu()
        m64 = go.EdgeConvOracle(64, 64).double()
        m64.load_state_dict({k: v.double() for k, v in ref_m.state_dict().items()})
        x64 = x.double()
        ref = go.segment_max(m64.mlp(torch.cat([x64[ei[1]], x64[ei[0]]], dim=1)), ei[1], n)
    assert torch.allclose(y.double(), ref, atol=FWD_TOL, rtol=FWD_TOL)


def test_no_edge_sized_allocation():
    """N = 2 000, E = 200 000, out = C = 64: one fused forward + backward stays below E * out * 4 bytes above the level before
    the call; the literal route does not (so the bound bites)"""
    import pangnn_amd
    n, e = 2000, 200_000
    ei = random_graph(n, e, seed=3)[0].to(dev())
    torch.manual_seed(0)
    m = pangnn_amd.EdgeConv(64, 64).to(dev())
    x = torch.randn(n, 64, device=dev())
    g = torch.randn(n, 64, device=dev())
    bound = e * 64 * 4

    def rise(flag):
        def step():
            xg = x.clone().requires_grad_(True)
            _forward_with_switch(m, xg, ei, flag).backward(g)
            m.zero_grad(set_to_none=True)
        step()                                               # warm-up: structure, caches
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    fused, literal = rise(True), rise(False)
    print(f"peak rise: fused {fused / 1e6:.1f} MB, literal {literal / 1e6:.1f} MB, bound {bound / 1e6:.1f} MB")
    assert fused < bound
    assert literal > bound


def test_dispatcher_op_schema_fake_and_cpu_refusal():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from pangnn_amd import torch_ops  # noqa: F401
    ops = torch.ops.pangnn
    assert str(ops.edge_conv.default._schema) == \
        "pangnn::edge_conv(Tensor u, Tensor v, Tensor w2, Tensor b2, Tensor edge_index) -> (Tensor, Tensor)"
    assert str(ops.edge_conv_backward.default._schema) == (
        "pangnn::edge_conv_backward(Tensor g, Tensor arg, Tensor u, Tensor v, Tensor w2, Tensor edge_index) -> "
        "(Tensor, Tensor, Tensor, Tensor)")
    with pytest.raises((RuntimeError, NotImplementedError)):
        ops.edge_conv(torch.randn(3, 64), torch.randn(3, 64), torch.randn(64, 64), torch.randn(64),
                      torch.tensor([[0, 1], [1, 2]]))
    with FakeTensorMode():
        f = lambda *s: torch.empty(*s, device="cuda")                  # noqa: E731
        ei = torch.empty(2, 50, dtype=torch.int64, device="cuda")
        for out in (64, 128):
            y, arg = ops.edge_conv(f(20, out), f(20, out), f(out, out), f(out), ei)
            assert y.shape == arg.shape == (20, out) and y.dtype == torch.float32 and arg.dtype == torch.int32
            gu, gv, gw2, gb2 = ops.edge_conv_backward(y, arg, f(20, out), f(20, out), f(out, out), ei)
            assert gu.shape == gv.shape == (20, out) and gw2.shape == (out, out) and gb2.shape == (out,)
            assert {t.dtype for t in (gu, gv, gw2, gb2)} == {torch.float32}


def test_edge_conv_compiles_to_the_eager_result():
    from pangnn_amd import functional as PF
    if PF.USE_DISPATCHER_OPS is not True:
        pytest.skip("route forced by the environment")
    n, ei = graph("rand300")
    ref_m, x, gsel, _, _ = case("rand300", 64, 64)
    m = fused_module(ref_m, 64, 64)
    eid, gd = ei.to(dev()), gsel.to(dev())
    xe = x.to(dev()).requires_grad_(True)
    eager = m(xe, eid)
    eager.backward(gd)
    grads = {k: p.grad.clone() for k, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    torch._dynamo.reset()
    xc = x.to(dev()).requires_grad_(True)
    out = torch.compile(m, backend="aot_eager")(xc, eid)
    out.backward(gd)
    assert torch.equal(out, eager) and torch.equal(xc.grad, xe.grad)
    for k, p in m.named_parameters():
        assert torch.equal(p.grad, grads[k]), k


def test_c_abi_refuses_bad_arguments_on_the_host():
    """host-side checks only: nothing is launched"""
    from pangnn_amd import _lib
    lib = _lib.load()
    n, e = 4, 6
    f = lambda *s: torch.zeros(*s, device=dev())                       # noqa: E731
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev())  # noqa: E731
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=dev())
    ei = torch.zeros(2, e, dtype=torch.int64, device=dev())
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev())

    def call(out, rp):
        u, v, w2, b2, y, arg = f(n, out), f(n, out), f(out, out), f(out), f(n, out), i32(n, out)
        return lib.pangnn_edge_conv_fwd_f32(u.data_ptr(), out, v.data_ptr(), out, n, w2.data_ptr(), b2.data_ptr(), out,
                                            None if rp is None else rp.data_ptr(), i32(e).data_ptr(), i32(e).data_ptr(),
                                            ei.data_ptr(), e, e, y.data_ptr(), arg.data_ptr(), out, ws.data_ptr(), ws.numel(),
                                            _lib.stream_ptr())

    assert call(12, rowptr) == -1 and b"64 or 128" in lib.pangnn_last_error()           # PANGNN_E_BADARG
    assert call(64, None) == -1 and b"null" in lib.pangnn_last_error()
    assert lib.pangnn_edge_conv_scratch_bytes(e, 12, 0) == 0
    assert 0 < lib.pangnn_edge_conv_scratch_bytes(10 ** 8, 128, 0) < 64 << 20           # bounded in E
