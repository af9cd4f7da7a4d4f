"""GPU suite of the edge-weight gradient: GCNConv(x, edge_index, edge_weight) differentiated with respect to `edge_weight`
(csrc/edge_weight_grad.hip, functional.propagate_w) against the torch oracle, which differentiates gcn_norm and propagate_add
with respect to the weights by itself.

Three graphs, all with weights in [1, 81] as Q-scores are:
  T  a 12-node hand graph: an isolated node (11), a node with out-edges only (10), a duplicate edge, a self loop, and one edge
     of weight exactly 0 into a target that has other in-edges;
  R  random, N = 300, E = 5000;
  H  N = 64: 500 random edges, 9000 edges into node 5 and 9000 out of node 3, so that both CSR orders have a row past
     LONG_ROW = 8192 (segment tables in the norm backward, a row shared by several waves in the edge dot).
Gradient bound against the fp64 oracle: FP64_DIRECT = 2e-5 of each tensor's max-abs (tests/test_hip_parity.py)."""
import copy
import functools

import pytest
import torch

from conftest import copy_graph, random_graph
from oracle import gcn_oracle as go
from test_hip_parity import FP64_DIRECT, OBSERVED_FLIPS, _pair, close, dev

pytestmark = pytest.mark.gpu

ROWS = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


@functools.lru_cache(maxsize=None)
def graph(name):
    """(edge_index [2, E] int64, weights [E] float32, N) on the CPU"""
    if name == "T":
        edges = [(0, 1), (0, 1), (1, 2), (2, 3), (3, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8), (8, 9), (9, 0), (10, 0), (10, 5),
                 (2, 0), (4, 0), (6, 2), (8, 2), (1, 7), (5, 9), (7, 4), (9, 6), (2, 8), (0, 4)]
        ei = torch.tensor(edges, dtype=torch.int64).t().contiguous()
        w = torch.rand(ei.shape[1], generator=torch.Generator().manual_seed(3)) * 80 + 1
        w[-1] = 0.0                                   # (0, 4): node 4 also has the in-edges (3, 4) and (7, 4)
        return ei, w, 12
    if name == "R":
        ei, w = random_graph(300, 5000, seed=11)
        return ei, w, 300
    gen = torch.Generator().manual_seed(5)
    n = 64
    src = torch.cat([torch.randint(0, n, (500,), generator=gen), torch.randint(0, n, (9000,), generator=gen),
                     torch.full((9000,), 3, dtype=torch.int64)])
    dst = torch.cat([torch.randint(0, n, (500,), generator=gen), torch.full((9000,), 5, dtype=torch.int64),
                     torch.randint(0, n, (9000,), generator=gen)])
    order = torch.randperm(src.shape[0], generator=gen)          # the hub's edges are spread over the caller's order
    ei = torch.stack([src[order], dst[order]])
    return ei, torch.rand(ei.shape[1], generator=gen) * 80 + 1, n


@functools.lru_cache(maxsize=None)
def structure(name):
    from pangnn_amd.graph import EdgeStructure
    ei, _, n = graph(name)
    return EdgeStructure(ei.to(dev()), n)


def test_the_hub_graph_has_long_rows_in_both_orders():
    from pangnn_amd.graph import LONG_ROW
    st = structure("H")
    assert LONG_ROW == 8192 and st.by_dst.long_rows() is not None and st.by_src.long_rows() is not None
    assert structure("R").by_dst.long_rows() is None


# ------------------------------------------------------------------------------------------------------------------
# 1. the edge dot on an exact grid
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid(name, f):
    """integer tables in [-4, 4] and the float64 dot products per edge in the caller's order: every partial sum is an integer
    of magnitude <= 16 f <= 4096 < 2^24, exact in float32 in any order, and every entry is a bfloat16 / float16 value"""
    ei, _, n = graph(name)
    gen = torch.Generator().manual_seed(100 + f)
    g = torch.randint(-4, 5, (n, f), generator=gen).double()
    x = torch.randint(-4, 5, (n, f), generator=gen).double()
    return g, x, (g[ei[1]] * x[ei[0]]).sum(dim=1)


@pytest.mark.parametrize("name", ["R", "H"])
@pytest.mark.parametrize("f", [16, 32, 64, 128, 256])
@pytest.mark.parametrize("g_rows,x_rows", [("f32", "f32"), ("bf16", "bf16"), ("f16", "f16"), ("f32", "bf16"), ("f16", "f32")])
def test_edge_dot_is_exact_on_the_integer_grid(name, f, g_rows, x_rows):
    from pangnn_amd import _lib, functional as PF
    g, x, ref = grid(name, f)
    st = structure(name)
    csr = st.by_dst
    gd, xd = g.to(dev(), ROWS[g_rows]), x.to(dev(), ROWS[x_rows])
    if f == 16 and (g_rows, x_rows) != ("f32", "f32"):
        # width 16 is gathered as float32 only, like the propagate: the entry point refuses 2-byte rows there ...
        lib = _lib.load()
        out = torch.empty(csr.other.shape[0], device=dev())
        rc = lib.pangnn_edge_dot_mixed(csr.rowptr.data_ptr(), csr.other.data_ptr(), csr.perm.data_ptr(), gd.data_ptr(),
                                       PF.dtype_code(gd.dtype), f, gd.shape[0], xd.data_ptr(), PF.dtype_code(xd.dtype), f,
                                       xd.shape[0], gd.shape[0], csr.other.shape[0], f, out.data_ptr(), None, None)
        assert rc == -1
        # ... and the Python operator up-converts such rows: the float32 result
    out_sorted, out_orig = PF.edge_dot(csr, gd, xd)
    assert out_sorted.dtype == out_orig.dtype == torch.float32
    assert torch.equal(out_orig.cpu().double(), ref)
    assert torch.equal(out_sorted.cpu().double(), ref[csr.perm.cpu().long()])
    only_sorted, none = PF.edge_dot(csr, gd, xd, want_orig=False)
    assert none is None and torch.equal(only_sorted, out_sorted)


@pytest.mark.parametrize("f,rows", [(16, "f32"), (64, "f16"), (256, "f32")])
def test_edge_dot_at_the_corners_of_the_row_search(f, rows):
    """A wave owns 64 entries of a list this short, and each of its 64 / (f / 4) sub-groups finds the row of its first entry
    by the binary search of csrc/common.h (row_of_entry), then steps the row pointer: the row pointers of
    test_csr_plan.search_corners, the row of entry k being searchsorted(rowptr, k, right=True) - 1 on the CPU, on the
    integer grid of the test above (|sum| <= 16 f <= 4096: exact in any order)."""
    from pangnn_amd import functional as PF
    from pangnn_amd.graph import CSR
    from test_csr_plan import SEARCH_ROWS, row_of_entries, search_corners
    n_x = 37
    gen = torch.Generator().manual_seed(200 + f)
    g = torch.randint(-4, 5, (max(SEARCH_ROWS), f), generator=gen).double()
    x = torch.randint(-4, 5, (n_x, f), generator=gen).double()
    gd, xd = g.to(dev(), ROWS[rows]), x.to(dev(), ROWS[rows])
    for name, rowptr in search_corners():
        e, n = int(rowptr[-1]), rowptr.numel() - 1
        other = torch.randint(0, n_x, (e,), generator=gen, dtype=torch.int32)
        perm = torch.randperm(e, generator=gen).to(torch.int32)
        ref = (g[row_of_entries(rowptr)] * x[other.long()]).sum(dim=1)
        csr = CSR(rowptr.to(dev()), other.to(dev()), perm.to(dev()))
        out_sorted, out_orig = PF.edge_dot(csr, gd[:n], xd)
        assert torch.equal(out_sorted.cpu().double(), ref), (name, f, rows)
        assert torch.equal(out_orig.cpu().double()[perm.long()], ref), (name, f, rows)


# ------------------------------------------------------------------------------------------------------------------
# 2.-5. GCNConv against the oracle
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conv_case(name, cin, cout):
    """parameters, input, cotangent (CPU float32) and the float64 oracle's gradients of sum(out * r)"""
    ei, w, n = graph(name)
    gen = torch.Generator().manual_seed(7 * cin + cout)
    x = torch.randn(n, cin, generator=gen)
    a = (6.0 / (cin + cout)) ** 0.5
    W = (torch.rand(cout, cin, generator=gen) * 2 - 1) * a
    b = torch.rand(cout, generator=gen) * 2 - 1
    r = torch.randn(n, cout, generator=gen)
    return dict(x=x, W=W, b=b, r=r, ref=oracle_grads(ei, w, x, W, b, r, torch.float64))


def oracle_grads(ei, w, x, W, b, r, dtype, weight_of=None):
    """gradients of sum(gcn_conv(...) * r) in `dtype`; `weight_of`: the weights are weight_of(m) and `w` is m"""
    leaves = [t.detach().to(dtype).requires_grad_() for t in (w, x, W, b)]
    wl, xl, Wl, bl = leaves
    out = go.gcn_conv(xl, ei, wl if weight_of is None else weight_of(wl), Wl, bl)
    (out * r.to(dtype)).sum().backward()
    return dict(out=out.detach(), w=wl.grad, x=xl.grad, W=Wl.grad, b=bl.grad)


def hip_grads(name, cin, cout, requires_grad=True, weight_of=None, w=None, x=None, autocast=None):
    import pangnn_amd
    ei, w0, n = graph(name)
    c = conv_case(name, cin, cout)
    conv = pangnn_amd.GCNConv(cin, cout).to(dev())
    with torch.no_grad():
        conv.lin.weight.copy_(c["W"])
        conv.bias.copy_(c["b"])
    wl = (w0 if w is None else w).to(dev()).requires_grad_(requires_grad)
    xl = (c["x"] if x is None else x).to(dev()).requires_grad_()
    eid = ei.to(dev())
    if autocast is None:
        out = conv(xl, eid, wl if weight_of is None else weight_of(wl))
    else:
        with torch.autocast("cuda", dtype=autocast):
            out = conv(xl, eid, wl)
    (out.float() * c["r"].to(dev())).sum().backward()
    return dict(out=out.detach(), w=wl.grad, x=xl.grad, W=conv.lin.weight.grad, b=conv.bias.grad, conv=conv, ei=eid, wl=wl)


def assert_within(got, ref, tag):
    for k in ("w", "x", "W", "b"):
        scale = float(ref[k].abs().max()) + 1e-30
        err = float((got[k].detach().cpu().double() - ref[k].double()).abs().max()) / scale
        print(f"{tag} {k}: {err:.2e} of max-abs")
        assert err <= FP64_DIRECT, (tag, k, err)


@pytest.mark.parametrize("name", ["T", "R", "H"])
@pytest.mark.parametrize("cin,cout", [(64, 128), (128, 64)])
def test_gcnconv_gradients_match_the_fp64_oracle(name, cin, cout):
    got = hip_grads(name, cin, cout)
    ref = conv_case(name, cin, cout)["ref"]
    assert got["w"] is not None and got["w"].shape == ref["w"].shape and got["w"].dtype == torch.float32
    assert close(got["out"], ref["out"])
    assert_within(got, ref, f"{name} {cin}->{cout}")


@pytest.mark.parametrize("cin,cout", [(64, 128), (128, 64)])
def test_non_leaf_weights(cin, cout):
    """w = a * sigmoid(m): the gradient arrives in m"""
    ei, w, n = graph("R")
    a = (w * 2).clone()
    m = torch.randn(w.shape[0], generator=torch.Generator().manual_seed(2))
    c = conv_case("R", cin, cout)
    ref = oracle_grads(ei, m, c["x"], c["W"], c["b"], c["r"], torch.float64, weight_of=lambda t: a.double() * torch.sigmoid(t))
    ad = a.to(dev())
    got = hip_grads("R", cin, cout, w=m, weight_of=lambda t: ad * torch.sigmoid(t))
    assert_within(got, ref, f"non-leaf {cin}->{cout}")


@pytest.mark.parametrize("name", ["T", "R", "H"])
@pytest.mark.parametrize("cin,cout", [(64, 128), (128, 64)])
def test_nothing_else_moved(name, cin, cout):
    """the output and the other three gradients have the bits of the same call with the weights detached"""
    a, b = hip_grads(name, cin, cout), hip_grads(name, cin, cout, requires_grad=False)
    assert b["w"] is None and a["w"] is not None
    for k in ("out", "x", "W", "b"):
        assert torch.equal(a[k], b[k]), k


def test_weight_gradient_is_reproducible_on_the_hub_graph():
    a, b = hip_grads("H", 64, 128), hip_grads("H", 64, 128)
    assert torch.equal(a["w"], b["w"])
    a, b = hip_grads("H", 128, 64), hip_grads("H", 128, 64)
    assert torch.equal(a["w"], b["w"])


@pytest.mark.parametrize("cin,cout", [(64, 128), (128, 64)])
def test_nan_in_a_source_row_reaches_the_same_edges_as_in_torch(cin, cout):
    ei, w, n = graph("R")
    c = conv_case("R", cin, cout)
    x = c["x"].clone()
    s = int(ei[0, 0])
    x[s, 3] = float("nan")
    ref = oracle_grads(ei, w, x, c["W"], c["b"], c["r"], torch.float32)
    got = hip_grads("R", cin, cout, x=x)
    mask = torch.isnan(ref["w"])
    assert 0 < int(mask.sum()) < mask.numel() and bool(mask[ei[0] == s].all())
    assert torch.equal(torch.isnan(got["w"]).cpu(), mask)


# ------------------------------------------------------------------------------------------------------------------
# 6. autocast: the gradient is the two entry points on the stored 16-bit rows
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("cin,cout", [(64, 128), (128, 64)])
def test_autocast_gradient_is_the_entry_points_on_the_stored_rows(rows, cin, cout):
    from pangnn_amd import functional as PF
    from pangnn_amd.graph import structure_of
    got = hip_grads("R", cin, cout, autocast=rows)
    conv, eid, wl = got["conv"], got["ei"], got["wl"]
    c = conv_case("R", cin, cout)
    n = c["x"].shape[0]
    st = structure_of(eid, n)
    norm = st.gcn_norm(wl.detach())
    x, r = c["x"].to(dev()), c["r"].to(dev())
    W, b = conv.lin.weight.detach(), conv.bias.detach()
    with torch.autocast("cuda", dtype=rows):
        if cin < cout:       # propagate first: 16-bit input rows; the upstream gradient is the 16-bit dL/d(agg) of the autocast Linear
            x16 = x.to(rows)
            agg = PF.propagate(x16, None, st, norm, out_dtype=rows).detach().requires_grad_()
            out = PF.linear(agg, W, b, 0, rows)
            out.backward(r.to(rows))
            g, gathered = agg.grad, x16
            assert g.dtype == rows
        else:                # dense first: the Linear's 16-bit output rows are gathered; the upstream gradient is float32
            gathered = PF.linear(x, W, None, 0, rows).detach()
            g = r
            assert gathered.dtype == rows
    by_hand = PF.gcn_norm_backward(st, norm, PF.edge_dot(st.by_dst, g, gathered)[1])
    assert got["w"].dtype == torch.float32 and torch.equal(got["w"], by_hand)
    # and the stored rows are what counts: the same call on the up-converted rows gives the same bits
    up = PF.gcn_norm_backward(st, norm, PF.edge_dot(st.by_dst, g.float(), gathered.float())[1])
    assert torch.equal(up, by_hand)


# ------------------------------------------------------------------------------------------------------------------
# 7. the model
# ------------------------------------------------------------------------------------------------------------------
MODEL_GRAPH, MODEL_DIMS = "sim_200x4", (64, 128)
MODEL_FLAGS = [dict(), dict(union_edge_weights=True), dict(base_model=True), dict(skip_connections=True)]


def flags_id(f):
    return "-".join(f"{k}={v}" for k, v in f.items()) or "default"


def _bce(out, y, pw):
    return torch.nn.functional.binary_cross_entropy_with_logits(out, y, pos_weight=pw)


@pytest.mark.parametrize("route", ["loss_and_logits", "forward"])
@pytest.mark.parametrize("flags", MODEL_FLAGS, ids=flags_id)
def test_model_gradients_in_edge_attr_match_the_fp64_oracle(flags, route):
    """edge_attr.grad and every parameter gradient against the fp64 oracle model, by the acceptance rule of
    test_alternate_gcn_logits_and_grads_match_oracle: the direct FP64_DIRECT bound, and the flip band max(4 e_o32 + 2e-5, 5e-4)
    only for the (graph, flags) case that test lists as flipping"""
    g, gd, oracle, model = _pair(MODEL_GRAPH, MODEL_DIMS, flags)
    fid = flags_id(flags)
    flips = {k for (n_, f_, k) in OBSERVED_FLIPS if (n_, f_) == (MODEL_GRAPH, fid)}
    if flips:
        flips.add("edge_attr")
    pw = torch.tensor(float((g.y == 0).sum() / g.y.sum()))

    def oracle_run(dtype):
        o = copy.deepcopy(oracle).to(dtype)
        o.zero_grad()
        gg = copy.copy(g)
        gg.x = g.x.to(dtype)
        gg.edge_attr = g.edge_attr.detach().to(dtype).requires_grad_()
        out = o(gg)
        _bce(out, g.y.to(dtype), pw.to(dtype)).backward()
        grads = {k: p.grad for k, p in o.named_parameters()}
        grads["edge_attr"] = gg.edge_attr.grad
        return out.detach(), grads

    out32, g32 = oracle_run(torch.float32)
    _, g64 = oracle_run(torch.float64)
    gd.edge_attr = gd.edge_attr.detach().clone().requires_grad_()
    if route == "forward":
        out = model(gd)
        loss = _bce(out, gd.y, pw.to(dev()))
    else:
        loss, out = model.loss_and_logits(gd, gd.y, pw.to(dev()))
    assert close(out, out32)
    loss.backward()
    got = {k: p.grad for k, p in model.named_parameters()}
    got["edge_attr"] = gd.edge_attr.grad
    assert got["edge_attr"] is not None and got["edge_attr"].shape == g.edge_attr.shape
    for k, ref in g64.items():
        if ref is None:
            assert got[k] is None or float(got[k].abs().max()) == 0.0, k
            continue
        scale = float(g32[k].abs().max()) + 1e-12
        e_hip = float((got[k].detach().cpu().double() - ref).abs().max()) / scale
        e_o32 = float((g32[k].double() - ref).abs().max()) / scale
        print(f"{fid} {route} {k}: HIP {e_hip:.2e}, fp32 oracle {e_o32:.2e}")
        if k in flips:
            assert e_hip <= max(4.0 * e_o32 + 2e-5, 5e-4), (k, e_hip, e_o32)
        else:
            assert e_hip <= FP64_DIRECT, (k, e_hip, e_o32)


@pytest.mark.parametrize("flags", [f for f in MODEL_FLAGS if not f.get("skip_connections")], ids=flags_id)
def test_model_logits_equal_the_constant_weight_call(flags):
    """without skip connections the decoder route is the one of a constant-weight call, and the encoder is the layer-by-layer
    form: the logits have the bits of a `fuse_embedding=False` model on detached weights"""
    import pangnn_amd
    g, gd, oracle, model = _pair(MODEL_GRAPH, MODEL_DIMS, flags)
    plain = pangnn_amd.AlternateGCN(dev(), None, False, dims=list(MODEL_DIMS), num_nodes=g.x.shape[0], fuse_embedding=False,
                                    **flags)
    plain.load_state_dict(model.state_dict())
    gw = copy_graph(g, dev())
    gw.edge_attr = gw.edge_attr.detach().clone().requires_grad_()
    for m in (model, plain):
        m.eval()
    assert torch.equal(model(gw).detach(), plain(gd).detach())
    pw = torch.tensor(float((g.y == 0).sum() / g.y.sum()), device=dev())
    for m in (model, plain):
        m.train()
    (la, outa), (lb, outb) = model.loss_and_logits(gw, gw.y, pw), plain.loss_and_logits(gd, gd.y, pw)
    assert torch.equal(outa, outb) and torch.equal(la.detach(), lb.detach())


@pytest.mark.parametrize("flags", MODEL_FLAGS, ids=flags_id)
def test_model_raises_where_a_mode_is_watching(flags):
    from torch._subclasses.fake_tensor import FakeTensorMode
    g, gd, oracle, model = _pair(MODEL_GRAPH, MODEL_DIMS, flags)
    gd.edge_attr = gd.edge_attr.detach().clone().requires_grad_()

    class Watch(torch.utils._python_dispatch.TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            return func(*args, **(kwargs or {}))

    for mode in (FakeTensorMode(allow_non_fake_inputs=True), Watch()):
        with mode:
            with pytest.raises(NotImplementedError, match="edge_weight"):
                model(gd)
            with pytest.raises(NotImplementedError, match="edge_weight"):
                model.loss_and_logits(gd, gd.y, None)
    out = model(gd)                                   # and works again once nobody watches
    assert out.shape == (g.edge_index.shape[1],)
