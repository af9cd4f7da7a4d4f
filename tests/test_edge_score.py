"""The weightless link decoders (`--decoder cosine` / `dotproduct`, /root/reference/src/gnn.py:171-180,202-207) on
csrc/edge_score.hip: kernel level against torch in fp64, the fused BCE form, determinism, 2-byte rows, the dispatcher route,
the model, the reference's accelerate loop and the memory claim (no [E, 2D] edge tensor)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from conftest import copy_graph, random_graph, whole_graph_from_golden

WIDTHS = (16, 32, 64, 128, 256)
MODES = ("dot", "cosine")


# ---------------------------------------------------------------------------------------------- CPU: ops, fakes, C ABI checks
def test_ops_are_registered_with_their_schemas():
    from pangnn_amd import torch_ops  # noqa: F401
    ops = torch.ops.pangnn
    assert str(ops.edge_score.default._schema) == "pangnn::edge_score(Tensor z, Tensor edge_index, int mode) -> (Tensor, Tensor)"
    assert str(ops.edge_score_backward.default._schema) == (
        "pangnn::edge_score_backward(Tensor g, Tensor z, Tensor edge_index, Tensor logits, Tensor norms, Tensor? g_scale, "
        "int mode) -> Tensor")
    assert str(ops.edge_score_loss.default._schema) == (
        "pangnn::edge_score_loss(Tensor z, Tensor edge_index, int mode, Tensor y, Tensor? pos_weight, int denom) -> "
        "(Tensor, Tensor, Tensor, Tensor)")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fake_kernels_trace_with_shapes_and_dtypes(dtype):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from pangnn_amd import torch_ops  # noqa: F401
    ops = torch.ops.pangnn
    with FakeTensorMode():
        z = torch.empty(7, 32, dtype=dtype)
        ei = torch.empty(2, 11, dtype=torch.int64)
        y = torch.empty(11)
        for mode in (0, 1):
            logits, norms = ops.edge_score(z, ei, mode)
            assert logits.shape == (11,) and logits.dtype == torch.float32
            assert norms.shape == ((7, 2) if mode else (0, 2)) and norms.dtype == torch.float32
            gz = ops.edge_score_backward(logits, z, ei, logits, norms, None, mode)
            assert gz.shape == z.shape and gz.dtype == dtype
            loss, lg, g_l, nm = ops.edge_score_loss(z, ei, mode, y, None, 11)
            assert loss.shape == () and lg.shape == g_l.shape == (11,) and nm.shape == norms.shape
            assert loss.dtype == lg.dtype == g_l.dtype == torch.float32


_F = 0x7f0000100000          # a 16-byte aligned address that is never dereferenced


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: only where a missing check cannot reach a GPU")
def test_host_argument_checks_refuse_before_any_launch():
    from pangnn_amd import _lib
    L = _lib.load()
    BAD = -1
    n, e = 1000, 5000
    for d in WIDTHS:
        assert L.pangnn_edge_score_supported(d) == 1
    for d in (0, 8, 48, 63, 512):
        assert L.pangnn_edge_score_supported(d) == 0
        assert L.pangnn_edge_score_mixed(_F, 0, 64, n, _F, e, e, d, 1, _F, _F, None) == BAD
    fwd = lambda *a: L.pangnn_edge_score_mixed(*a, None)                                      # noqa: E731
    assert fwd(None, 0, 64, n, _F, e, e, 64, 1, _F, _F) == BAD                                # null z
    assert fwd(_F, 0, 64, n, None, e, e, 64, 1, _F, _F) == BAD                                # null edge list
    assert fwd(_F, 0, 64, n, _F, e, e, 64, 1, None, _F) == BAD                                # cosine without norms
    assert fwd(_F, 0, 64, -1, _F, e, e, 64, 1, _F, _F) == BAD                                 # negative sizes
    assert fwd(_F, 0, 64, n, _F, e, -1, 64, 1, _F, _F) == BAD
    assert fwd(_F, 0, 64, n, _F, e, e, 64, 2, _F, _F) == BAD                                  # unknown mode
    assert fwd(_F, 3, 64, n, _F, e, e, 64, 1, _F, _F) == BAD                                  # unknown storage type
    assert fwd(_F + 4, 0, 64, n, _F, e, e, 64, 0, None, _F) == -4                             # misaligned f32 rows
    loss = lambda *a: L.pangnn_edge_score_loss_mixed(*a, None)                                # noqa: E731
    assert loss(_F, 0, 64, n, _F, e, e, 64, 1, None, None, e, _F, _F, _F, _F, _F) == BAD       # null y
    assert loss(_F, 0, 64, n, _F, e, e, 64, 1, _F, None, 0, _F, _F, _F, _F, _F) == BAD         # denom 0
    assert loss(_F, 0, 64, n, _F, e, e, 64, 1, _F, None, e, _F, _F, _F, _F, None) == BAD       # no loss scratch
    assert loss(_F, 0, 64, n, _F, e, e, 48, 1, _F, None, e, _F, _F, _F, _F, _F) == BAD         # D
    order = [_F, _F, _F, None, None, 0, None]

    def bwd(*head, src=order, dst=order, g=_F, logits=_F, norms=_F, gz=_F, ldg=64):
        return L.pangnn_edge_score_bwd_mixed(*head, *src, *dst, g, logits, norms, None, gz, ldg, None)
    assert bwd(_F, 0, 64, n, e, 64, 1, gz=None) == BAD                                         # null gz
    assert bwd(_F, 0, 64, n, e, 64, 1, g=None) == BAD                                          # null g
    assert bwd(_F, 0, 64, n, e, 64, 1, norms=None) == BAD                                      # cosine without norms
    assert bwd(_F, 0, 64, n, e, 64, 0, ldg=60) == BAD                                          # ldg
    assert bwd(_F, 0, 64, n, -5, 64, 0) == BAD                                                 # negative sizes
    assert bwd(_F, 0, 64, n, e, 96, 0) == BAD                                                  # D
    assert bwd(_F, 0, 64, n, e, 64, 0, src=[_F, _F, _F, _F, None, 4, _F]) == BAD               # segments half given
    assert bwd(_F, 0, 64, n, e, 64, 0, src=[_F, _F, _F, _F, _F, 4, None]) == BAD               # segments without parts
    assert bwd(_F, 0, 64, n, e, 64, 0, src=[None, _F, _F, None, None, 0, None]) == BAD         # null row pointer
    assert b"pangnn_edge_score_bwd_mixed" in L.pangnn_last_error()


def test_a_rectangular_structure_is_refused_on_the_host():
    """edge_score / edge_score_loss go through ops that find a graph by (edge_index, target rows): a shard's structure with
    other source rows raises before anything is launched"""
    from pangnn_amd import functional as PF
    from pangnn_amd.graph import EdgeStructure
    st = EdgeStructure(torch.tensor([[0, 6, 3], [1, 2, 4]]), 5, num_src=7)
    z = torch.randn(7, 16)
    for mode in MODES:
        with pytest.raises(ValueError, match="edge_score: "):
            PF.edge_score(z, st, mode)
        with pytest.raises(ValueError, match="edge_score_loss: "):
            PF.edge_score_loss(z, st, mode, torch.zeros(3))


# ---------------------------------------------------------------------------------------------- GPU: kernel level
def _dev():
    return torch.device("cuda:0")


def _torch_scores(z, ei, mode):
    a, b = z[ei[0]], z[ei[1]]
    return F.cosine_similarity(a, b, dim=1) if mode == "cosine" else (a * b).sum(1)


def _reference(z, ei, mode, g):
    """(logits, dL/dz) of torch on CPU in fp64 and of today's literal fp32 route (torch on the same device in fp32)"""
    out = {}
    for tag, dt, dev in (("f64", torch.float64, "cpu"), ("lit", torch.float32, z.device)):
        zz = z.detach().to(dev, dt).requires_grad_(True)
        s = _torch_scores(zz, ei.to(dev), mode)
        s.backward(g.to(dev, dt))
        out[tag] = (s.detach().cpu().double(), zz.grad.cpu().double())
    return out


def _st(ei, n):
    from pangnn_amd.graph import structure_of
    return structure_of(ei, n)


def _graph_cases():
    cases = []
    for n, e, hub, seed in ((50, 333, None, 0), (300, 4099, None, 1), (1000, 1, None, 2), (64, 0, None, 3),
                            (3000, 30000, 20000, 4)):
        ei, _ = random_graph(n, e, seed=seed, hub=hub)
        cases.append((f"n{n}_e{e}" + ("_star" if hub else ""), n, ei))
    return cases


def _scaled_rows(n, d, seed, zero_rows=True):
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(n, d, generator=gen) / d ** 0.5
    if zero_rows and n > 8:
        z[1] = 0.0                                   # a zero row: torch's gradient of size ~1/eps
        z[2] *= 1e-10                                # norm below eps
    return z


def _check_against_f64(got_logits, got_grad, ref, tag):
    l64, g64 = ref["f64"]
    _, glit = ref["lit"]
    lscale = max(1.0, float(l64.abs().max())) if l64.numel() else 1.0
    if l64.numel():
        assert float((got_logits.cpu().double() - l64).abs().max()) <= 1e-6 * lscale, tag
    scale = float(g64.abs().max()) + 1e-30
    e_lit = float((glit - g64).abs().max()) / scale
    e_hip = float((got_grad.cpu().double() - g64).abs().max()) / scale
    assert e_hip <= max(2e-6, 2 * e_lit), (tag, e_hip, e_lit)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d", WIDTHS)
def test_kernels_match_torch_fp64(d, mode):
    from pangnn_amd import functional as PF
    for tag, n, ei in _graph_cases():
        eid = ei.to(_dev())
        z = _scaled_rows(n, d, seed=d + n)
        gen = torch.Generator().manual_seed(7)
        g = torch.randn(ei.shape[1], generator=gen)
        ref = _reference(z, ei, mode, g)
        zd = z.to(_dev()).requires_grad_(True)
        out = PF.edge_score(zd, _st(eid, n), mode)
        out.backward(g.to(_dev()))
        _check_against_f64(out.detach(), zd.grad, ref, f"{tag}/{d}/{mode}")
        # the same call twice: bitwise equal
        zd2 = z.to(_dev()).requires_grad_(True)
        out2 = PF.edge_score(zd2, _st(eid, n), mode)
        out2.backward(g.to(_dev()))
        assert torch.equal(out.detach(), out2.detach()) and torch.equal(zd.grad, zd2.grad), tag


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_tiny_and_zero_rows_follow_torch(mode):
    """rows of norm 0 and below eps: torch's gradient (size ~1/eps) to the same relative bound"""
    from pangnn_amd import functional as PF
    n, d = 40, 64
    gen = torch.Generator().manual_seed(3)
    z = torch.randn(n, d, generator=gen) * 1e-10                    # every row below eps
    z[0] = 0.0
    z[5:] = torch.randn(n - 5, d, generator=gen)
    ei = torch.tensor([[0, 1, 2, 3, 0, 7, 1, 9, 3], [1, 2, 3, 3, 9, 0, 1, 2, 0]])
    g = torch.randn(ei.shape[1], generator=gen)
    ref = _reference(z, ei, mode, g)
    zd = z.to(_dev()).requires_grad_(True)
    out = PF.edge_score(zd, _st(ei.to(_dev()), n), mode)
    out.backward(g.to(_dev()))
    _check_against_f64(out.detach(), zd.grad, ref, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d", (16, 64, 256))
def test_fused_loss_matches_torch_bce(d, mode):
    from pangnn_amd import functional as PF
    for tag, n, ei in _graph_cases():
        e = ei.shape[1]
        if e == 0:
            continue
        z = _scaled_rows(n, d, seed=d)
        gen = torch.Generator().manual_seed(11)
        y = (torch.rand(e, generator=gen) < 0.3).float()
        pw = torch.tensor(2.5)
        eid = ei.to(_dev())
        # torch in fp64 on the same logits the kernel produced
        zd = z.to(_dev()).requires_grad_(True)
        loss, logits = PF.edge_score_loss(zd, _st(eid, n), mode, y.to(_dev()), pw.to(_dev()), e)
        x = logits.cpu().double().requires_grad_(True)
        lr = F.binary_cross_entropy_with_logits(x, y.double(), pos_weight=pw.double())
        lr.backward()
        assert abs(loss.item() - lr.item()) <= 1e-6 * abs(lr.item()), tag
        # dL/dz = the plain call's backward with dL/dlogit, which must be torch's to 1e-7
        zd2 = z.to(_dev()).requires_grad_(True)
        PF.edge_score(zd2, _st(eid, n), mode).backward(x.grad.float().to(_dev()))
        loss.backward()
        scale = float(zd2.grad.abs().max()) + 1e-30
        assert float((zd.grad - zd2.grad).abs().max()) <= 1e-6 * scale + 1e-7 * scale, tag
        from pangnn_amd import torch_ops  # noqa: F401
        _, _, g_l, _ = torch.ops.pangnn.edge_score_loss(z.to(_dev()), eid, PF.SCORE_MODES[mode], y.to(_dev()), pw.to(_dev()), e)
        # 1e-7 absolute; where |dL/dlogit| itself exceeds 0.4 (a mean over a handful of edges) that is below fp32's
        # resolution, and the bound is two units in the last place of the largest element instead
        gmax = float(x.grad.abs().max())
        assert float((g_l.cpu().double() - x.grad).abs().max()) <= max(1e-7, 2.0 ** -22 * gmax), tag
        # an upstream gradient other than 1 is applied on the device
        zd3 = z.to(_dev()).requires_grad_(True)
        l3, _ = PF.edge_score_loss(zd3, _st(eid, n), mode, y.to(_dev()), pw.to(_dev()), e)
        (3.0 * l3).backward()
        assert torch.allclose(zd3.grad, 3.0 * zd.grad, rtol=1e-6, atol=0), tag


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_two_byte_rows_are_bit_identical_to_f32_on_the_up_converted_rows(dtype, mode):
    from pangnn_amd import functional as PF
    for tag, n, ei in _graph_cases():
        eid = ei.to(_dev())
        for d in (32, 128):
            z16 = _scaled_rows(n, d, seed=5, zero_rows=False).to(_dev(), dtype).requires_grad_(True)
            z32 = z16.detach().float().requires_grad_(True)
            g = torch.randn(ei.shape[1], device=_dev())
            o16 = PF.edge_score(z16, _st(eid, n), mode)
            o32 = PF.edge_score(z32, _st(eid, n), mode)
            o16.backward(g)
            o32.backward(g)
            assert torch.equal(o16, o32), tag
            assert z16.grad.dtype == dtype and torch.equal(z16.grad, z32.grad.to(dtype)), tag


def _raw_kernels(z, st, mode, y=None, pw=None, g=None, g_scale=None):
    """the C entry points on the structure's own tables: (logits, dL/dz) of pangnn_edge_score_mixed with the upstream gradient
    `g`, or with `y` (loss, logits, dL/dz) of pangnn_edge_score_loss_mixed — dL/dz from pangnn_edge_score_bwd_mixed either way,
    hub rows passed as the segments of CSR.long_rows"""
    from pangnn_amd import _lib
    L = _lib.load()
    m = {"dot": 0, "cosine": 1}[mode]
    n, d, e = z.shape[0], z.shape[1], st.num_edges
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=z.device)                      # noqa: E731
    logits, norms, loss, gz = f(e), f(n if m else 0, 2), f(1), f(n, d)
    nrm = norms.data_ptr() if m else None
    head = (z.data_ptr(), 0, z.stride(0), n, st.edge_index.data_ptr(), e, e, d, m)
    with _lib.device_guard(z.device):
        if y is None:
            _lib.check(L.pangnn_edge_score_mixed(*head, nrm, logits.data_ptr(), _lib.stream_ptr()), "pangnn_edge_score_mixed")
        else:
            g, parts = f(e), f(4096)                                                          # PANGNN_EDGE_SCORE_LOSS_PARTS
            _lib.check(L.pangnn_edge_score_loss_mixed(*head, y.data_ptr(), pw.data_ptr(), e, nrm, logits.data_ptr(),
                                                      loss.data_ptr(), g.data_ptr(), parts.data_ptr(), _lib.stream_ptr()),
                       "pangnn_edge_score_loss_mixed")
        orders, keep = [], []
        for csr in (st.by_src, st.by_dst):
            orders += [csr.rowptr.data_ptr(), csr.other.data_ptr(), csr.perm.data_ptr()]
            long = csr.long_rows()
            if long is None:
                orders += [None, None, 0, None]
            else:
                nseg = long[0].shape[0] - 1
                keep.append(f(nseg * (d + 1)))                                                # partial rows of the segments
                orders += [long[0].data_ptr(), long[1].data_ptr(), nseg, keep[-1].data_ptr()]
        _lib.check(L.pangnn_edge_score_bwd_mixed(z.data_ptr(), 0, z.stride(0), n, e, d, m, *orders, g.data_ptr(),
                                                 logits.data_ptr() if m else None, nrm, _lib.ptr(g_scale), gz.data_ptr(), d,
                                                 _lib.stream_ptr()), "pangnn_edge_score_bwd_mixed")
    return (logits, gz) if y is None else (loss.view(()), logits, gz)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_registered_ops_return_exactly_what_the_kernels_return(mode):
    """functional.edge_score / edge_score_loss have one route, the registered ops: their results and gradients are, bit for
    bit, those of the C entry points called here with the structure's tables"""
    from pangnn_amd import functional as PF
    tag, n, ei = _graph_cases()[-1]                          # the star: hub rows as segments
    eid = ei.to(_dev())
    st = _st(eid, n)
    assert st.by_dst.long_rows() is not None or st.by_src.long_rows() is not None
    z = _scaled_rows(n, 64, seed=9)
    y = (torch.rand(ei.shape[1]) < 0.4).float().to(_dev())
    pw = torch.tensor(1.7, device=_dev())
    g = torch.linspace(-1, 1, ei.shape[1], device=_dev())
    za = z.to(_dev()).requires_grad_(True)
    out = PF.edge_score(za, st, mode)
    out.backward(g)
    zb = z.to(_dev()).requires_grad_(True)
    loss, logits = PF.edge_score_loss(zb, st, mode, y, pw, ei.shape[1])
    loss.backward()
    zr = z.to(_dev())
    one = torch.ones(1, device=_dev())                       # loss.backward(): the upstream gradient the op hands the kernel
    raw = _raw_kernels(zr, st, mode, g=g) + _raw_kernels(zr, st, mode, y=y, pw=pw.reshape(1), g_scale=one)
    for a, b in zip((out.detach(), za.grad, loss.detach(), logits, zb.grad), raw):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- GPU: model level
def _model_pair(name, decoder, fused=True):
    import pangnn_amd
    from oracle import gcn_oracle as go
    g = whole_graph_from_golden(name)
    n = g.x.shape[0]
    torch.manual_seed(0)
    oracle = go.AlternateGCNOracle(dims=(64, 128), flags=go.default_flags(decoder=decoder), num_nodes=n)
    model = pangnn_amd.AlternateGCN(_dev(), None, False, dims=[64, 128], num_nodes=n, decoder=decoder, fused_decoder=fused)
    model.load_state_dict(oracle.state_dict())
    return g, copy_graph(g, _dev()), oracle, model


@pytest.mark.gpu
@pytest.mark.parametrize("decoder", ["cosine", "dot"])
@pytest.mark.parametrize("name", ["sim_200x4", "cfg1_2genomes", "cfg2_sim_1000x5", "cfg3_5genomes"])
def test_model_matches_oracle_and_literal_route(name, decoder):
    from test_hip_parity import _check_logits_loss_grads_against_oracle
    from pangnn_amd.train import criterion
    g, gd, oracle, model = _model_pair(name, decoder)
    out, ref, _ = _check_logits_loss_grads_against_oracle(g, gd, oracle, model, tag=f"{name}/{decoder}/fused")
    # fused_decoder=False: today's literal route, within the same bounds
    _, _, _, lit = _model_pair(name, decoder, fused=False)
    with torch.no_grad():
        z = lit.encode(gd)
        a, b = z[gd.edge_index[0]], z[gd.edge_index[1]]
        today = F.cosine_similarity(a, b, dim=1) if decoder == "cosine" else (a * b).sum(1)
        assert torch.allclose(lit(gd), today, atol=1e-6, rtol=1e-6)
        assert torch.allclose(lit(gd), out, atol=1e-4, rtol=1e-4)
    # loss_and_logits = criterion(model(g), y) + backward
    pw = torch.tensor(float((g.y == 0).sum() / g.y.sum()), device=_dev())
    model.zero_grad()
    loss_a = criterion(model(gd), gd.y, pw)
    loss_a.backward()
    ga = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    model.zero_grad()
    loss_b, logits_b = model.loss_and_logits(gd, gd.y, pw)
    loss_b.backward()
    assert torch.allclose(logits_b, out.detach(), atol=0, rtol=0)
    assert abs(loss_a.item() - loss_b.item()) <= 1e-6 * abs(loss_a.item())
    for k, p in model.named_parameters():
        if k in ga:
            scale = float(ga[k].abs().max()) + 1e-30
            assert float((p.grad - ga[k]).abs().max()) <= 1e-5 * scale, k


@pytest.mark.gpu
@pytest.mark.parametrize("decoder", ["cosine", "dot"])
def test_compiled_loss_and_logits_is_one_graph(decoder):
    _, gd, _, model = _model_pair("cfg1_2genomes", decoder)
    pw = torch.tensor(2.0, device=_dev())
    model.zero_grad()
    loss_e, logits_e = model.loss_and_logits(gd, gd.y, pw)
    loss_e.backward()
    ge = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    graphs = []

    def backend(gm, example_inputs):
        from torch._dynamo.backends.debugging import aot_eager
        graphs.append([n.target for n in gm.graph.nodes if n.op == "call_function"])
        return aot_eager(gm, example_inputs)

    torch._dynamo.reset()
    compiled = torch.compile(model.loss_and_logits, backend=backend, fullgraph=True)
    model.zero_grad()
    loss_c, logits_c = compiled(gd, gd.y, pw)
    loss_c.backward()
    assert len(graphs) == 1
    assert torch.ops.pangnn.edge_score_loss in graphs[0]
    assert torch.equal(loss_c.detach(), loss_e.detach()) and torch.equal(logits_c, logits_e)
    for k, p in model.named_parameters():
        if k in ge:
            assert torch.equal(p.grad, ge[k]), k
    torch._dynamo.reset()


@pytest.mark.gpu
@pytest.mark.parametrize("mixed", ["no", "bf16"])
def test_reference_loop_under_accelerate_with_cosine_decoder(mixed):
    """pangnn.py:25-216 literally, `--decoder cosine`, three whole-graph steps against the oracle's loop"""
    from accelerate import Accelerator
    from accelerate.state import AcceleratorState
    import pangnn_amd
    from oracle import gcn_oracle as go
    g = whole_graph_from_golden("cfg2_sim_1000x5")
    n = g.x.shape[0]
    cb = float((g.y == 0).sum() / g.y.sum())
    torch.manual_seed(0)
    oracle = go.AlternateGCNOracle(dims=(64, 64), flags=go.default_flags(decoder="cosine"), num_nodes=n)
    init = {k: v.clone() for k, v in oracle.state_dict().items()}
    opt_o = torch.optim.Adam(oracle.parameters(), lr=0.001)
    ref = []
    for _ in range(3):
        opt_o.zero_grad()
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=mixed == "bf16"):
            out = oracle(g)
        loss = F.binary_cross_entropy_with_logits(out.float(), g.y, pos_weight=torch.tensor(cb))
        loss.backward()
        opt_o.step()
        ref.append((loss.item(), out.detach().float()))
    AcceleratorState._reset_state(True)
    accelerator = Accelerator(mixed_precision=mixed)
    model = pangnn_amd.AlternateGCN(device=accelerator.device, dataset=None, categorical_nodes=False, dims=[64, 64],
                                    num_nodes=n, decoder="cosine")
    model.load_state_dict(init)
    optimizer = torch.optim.Adam(model.parameters(), lr=0.001)
    criterion = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor(cb))
    model, optimizer = accelerator.prepare(model, optimizer)
    whole = copy_graph(g, accelerator.device)
    got = []
    for _ in range(3):
        model.train()
        optimizer.zero_grad()
        output = model(whole)
        assert type(output) is torch.Tensor
        loss = criterion(output, whole.y)
        accelerator.backward(loss)
        optimizer.step()
        got.append((loss.item(), output.detach().float().cpu()))
    AcceleratorState._reset_state(True)
    for step, ((lm, om), (lo, oo)) in enumerate(zip(got, ref)):
        if mixed == "no":
            tol = 1e-4 if step == 0 else 5e-4
            assert torch.allclose(om, oo, atol=tol, rtol=tol), (step, float((om - oo).abs().max()))
            assert abs(lm - lo) <= (1e-5 if step == 0 else 1e-4) * max(1.0, abs(lo)), (step, lm, lo)
        else:
            scale = float(oo.abs().max())
            assert float((om - oo).abs().max()) < (5e-2 if step == 0 else 2e-1) * scale, step
            assert abs(lm - lo) < 5e-2 * abs(ref[0][0]), (step, lm, lo)


# ---------------------------------------------------------------------------------------------- GPU: the memory claim
@pytest.mark.gpu
def test_cosine_step_allocates_less_than_one_edge_by_d_tensor():
    """config 4's edge law (E ~ 1.5e6, D = 64): one cosine training step (forward, BCE, backward) peaks below E * D * 4 bytes
    above the pre-step level — the literal route's first op alone allocates E * 2D * 4"""
    import pangnn_amd
    from pangnn_amd import simulate
    from pangnn_amd.graph import structure_of
    dev = _dev()
    g = simulate.simulate_graph(1000, 20, 0.2, 100, 20, seed=3, device="cpu")
    gd = copy_graph(g, dev)
    e, d = g.edge_index.shape[1], 64
    model = pangnn_amd.AlternateGCN(dev, None, False, dims=[d, 128], num_nodes=g.num_nodes, decoder="cosine")
    pw = torch.tensor(float((g.y == 0).sum() / g.y.sum()), device=dev)
    loss, _ = model.loss_and_logits(gd, gd.y, pw)          # warm-up: structures, norms and caches are built once per graph
    loss.backward()
    del loss
    model.zero_grad(set_to_none=False)
    structure_of(gd.edge_index, g.num_nodes, holder=gd, name="sim")
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss, logits = model.loss_and_logits(gd, gd.y, pw)
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < e * d * 4, (peak, e * d * 4)
