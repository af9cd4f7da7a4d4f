"""Non-finite values on the training path ("Non-finite values"): a GradScaler protects `--mixed_precision fp16`
only if every kernel between an overflow and the parameter gradients hands inf / NaN on the way torch does, and raises no
alarm for values that no edge references.

Each operation is compared with the same operation in torch float64 on the CPU:
  1. forward outputs and the loss are non-finite exactly where the reference's are (inf and NaN are not told apart), and the
     elements that are finite in the reference meet the bound of that kernel's existing test;
  2. a gradient TENSOR that is non-finite anywhere in the reference is non-finite somewhere in ours, one that is finite in
     the reference is finite in ours and within the existing bound;
  3. non-finite values in rows that nothing references change nothing: bit-equal to the same call with those rows zeroed;
  4. operations with a NaN rule of their own keep it (fused EdgeConv = the literal route, normalize_sim_scores on the device
     = its CPU leg = oracle/construct_oracle.py).
The CPU tests (not marked gpu) test the two helpers and run every float64 reference on the chosen inputs: each case's reference
holds at least one non-finite output element and at least half of its elements are finite (rule-3 cases: none non-finite)."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import random_graph

NAN, INF = float("nan"), float("inf")
TABLES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _dev():
    return torch.device("cuda:0")


# ================================================================================================ the two helpers
def allclose_bound(atol, rtol):
    """|got - ref| <= atol + rtol |ref| element by element"""
    def bound(got, ref):
        return bool(((got - ref).abs() <= atol + rtol * ref.abs()).all())
    return bound


def scaled_bound(rel, floor=1e-30):
    """max |got - ref| <= rel * max |ref| (the gradient bound of the decoder / edge_score tests)"""
    def bound(got, ref):
        if ref.numel() == 0:
            return True
        return float((got - ref).abs().max()) <= rel * (float(ref.abs().max()) + floor)
    return bound


def _f64(t):
    return t.detach().cpu().double()


def assert_same_nonfinite(got, ref, *, finite_bound, what=""):
    """rule 1: `got` is non-finite exactly where `ref` is; where `ref` is finite, finite_bound(got, ref) holds"""
    got, ref = _f64(got), _f64(ref)
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    bad_got, bad_ref = ~torch.isfinite(got), ~torch.isfinite(ref)
    swallowed = bad_ref & ~bad_got
    leaked = bad_got & ~bad_ref
    assert not swallowed.any(), (f"{what}: {int(swallowed.sum())} element(s) finite here, non-finite in the reference; first at "
                                 f"{torch.nonzero(swallowed)[0].tolist()}")
    assert not leaked.any(), (f"{what}: {int(leaked.sum())} element(s) non-finite here, finite in the reference; first at "
                              f"{torch.nonzero(leaked)[0].tolist()}")
    ok = ~bad_ref
    if ok.any():
        g, r = got[ok], ref[ok]
        assert finite_bound(g, r), f"{what}: finite elements off by up to {float((g - r).abs().max()):.3e}"


def assert_same_nonfinite_tensorwise(got, ref, *, finite_bound, what=""):
    """rule 2 (what a GradScaler asks): `ref` non-finite anywhere -> `got` non-finite somewhere; `ref` all finite -> `got` all
    finite and finite_bound(got, ref)"""
    got, ref = _f64(got), _f64(ref)
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    if not torch.isfinite(ref).all():
        assert not torch.isfinite(got).all(), f"{what}: all finite here, non-finite in the reference (a swallowed overflow)"
        return
    assert torch.isfinite(got).all(), f"{what}: non-finite here, all finite in the reference (a false alarm)"
    assert finite_bound(got, ref), f"{what}: off by up to {float((got - ref).abs().max()):.3e}"


def as_stored(ref, table):
    """the reference of a result that comes back in a 2-byte type: a value past float16's range IS inf there (torch float32,
    then .half()); the rounding itself is left to the bound"""
    if table == "f32":
        return ref
    r32 = ref.detach().float()
    return torch.where(torch.isfinite(r32.to(TABLES[table])), ref.detach(), r32.to(TABLES[table]).double())


def informative(ref, *, expect_nonfinite=True):
    """the non-vacuity condition on a reference output"""
    ref = _f64(ref)
    bad = int((~torch.isfinite(ref)).sum())
    if not expect_nonfinite:
        return bad == 0
    return bad >= 1 and 2 * bad <= ref.numel()


def test_position_helper_fails_on_swallowed_leaked_and_finite_mismatch():
    ref = torch.tensor([1.0, NAN, -2.0, INF])
    b = allclose_bound(1e-6, 0.0)
    assert_same_nonfinite(torch.tensor([1.0, INF, -2.0, NAN]), ref, finite_bound=b)          # inf / NaN not told apart
    with pytest.raises(AssertionError, match="finite here, non-finite in the reference"):
        assert_same_nonfinite(torch.tensor([1.0, 0.0, -2.0, INF]), ref, finite_bound=b)     # swallowed
    with pytest.raises(AssertionError, match="non-finite here, finite in the reference"):
        assert_same_nonfinite(torch.tensor([1.0, NAN, NAN, INF]), ref, finite_bound=b)      # leaked
    with pytest.raises(AssertionError, match="finite elements off"):
        assert_same_nonfinite(torch.tensor([1.0, NAN, -2.1, INF]), ref, finite_bound=b)     # finite mismatch
    with pytest.raises(AssertionError):
        assert_same_nonfinite(torch.zeros(3), ref, finite_bound=b)                          # shape


def test_tensor_helper_fails_on_swallowed_leaked_and_finite_mismatch():
    b = scaled_bound(1e-6)
    ref_bad, ref_ok = torch.tensor([1.0, NAN, 3.0]), torch.tensor([1.0, 2.0, 3.0])
    assert_same_nonfinite_tensorwise(torch.tensor([INF, 2.0, 3.0]), ref_bad, finite_bound=b)    # the NaN may sit elsewhere
    assert_same_nonfinite_tensorwise(ref_ok.clone(), ref_ok, finite_bound=b)
    with pytest.raises(AssertionError, match="swallowed"):
        assert_same_nonfinite_tensorwise(ref_ok, ref_bad, finite_bound=b)
    with pytest.raises(AssertionError, match="false alarm"):
        assert_same_nonfinite_tensorwise(ref_bad, ref_ok, finite_bound=b)
    with pytest.raises(AssertionError, match="off by"):
        assert_same_nonfinite_tensorwise(torch.tensor([1.0, 2.0, 3.1]), ref_ok, finite_bound=b)


def test_informative_is_the_stated_condition():
    assert informative(torch.tensor([NAN, 1.0])) and not informative(torch.tensor([NAN, NAN, 1.0]))
    assert not informative(torch.tensor([1.0, 2.0])) and informative(torch.tensor([1.0, 2.0]), expect_nonfinite=False)
    assert not informative(torch.tensor([1.0, INF]), expect_nonfinite=False)


def test_torch_relu_keeps_nan_in_float64():
    """the premise of every reference below"""
    x = torch.tensor([NAN, -1.0, 2.0], dtype=torch.float64, requires_grad=True)
    y = torch.relu(x)
    assert torch.isnan(y[0]) and y[1] == 0 and y[2] == 2
    y.backward(torch.ones(3, dtype=torch.float64))
    assert x.grad.tolist()[1:] == [0.0, 1.0] and x.grad[0] == 1.0          # threshold_backward passes the gradient at a NaN


def set_negative_nan(t, row):
    """row `row` of `t` := NaN with the sign bit set, written as a bit pattern (a conversion to bfloat16 would drop the sign)"""
    pat = {torch.float32: (torch.int32, -4194304), torch.float16: (torch.int16, -512), torch.bfloat16: (torch.int16, -64)}
    it, v = pat[t.dtype]
    t.view(it)[row] = v
    assert torch.isnan(t[row]).all() and torch.signbit(t[row].float()).all()


# ================================================================================================ MLP decoder
DEC_N, DEC_D = 97, 64
DEC_E = (33, 1000, 1002)       # odd: sorted by source (run sums inside S), even: unsorted (both sums in T); 33 = one tile + 1
DEC_INJECT = ("nan_p", "inf_q", "ninf_q", "nan_unused", "negnan_p", "inf_w2", "inf_extra")
DEC_ALL_FINITE = ("nan_unused", "ninf_q")      # references without a non-finite element: rule 3, and the -inf a relu removes
DEC_NAMES = ("P", "Q", "W2", "b2", "w3", "b3", "cvec")
DEC_CASES = [(e, skip, inj, tab) for e in DEC_E for skip in (False, True) for inj in DEC_INJECT for tab in TABLES
             if skip or inj != "inf_extra"]          # `extra` only exists with skip connections


@functools.lru_cache(maxsize=None)
def decoder_case(e, skip, inject, table):
    """inputs (CPU, as stored) and the float64 reference of test_decoder_training_kernels_vs_fp64's formula; nodes 0 and 96
    are referenced by no edge (node 0 is the row a lane past the end of the list gathers in the strict-fp32 kernels)"""
    n, d, dt = DEC_N, DEC_D, TABLES[table]
    torch.manual_seed(e + skip)
    ei, w = random_graph(n - 2, e, seed=e, isolated=0.0)
    ei = ei + 1
    ei = ei[:, torch.argsort(ei[0] * n + ei[1])] if e % 2 else ei
    P, Q = torch.randn(n, d).to(dt), torch.randn(n, d).to(dt)
    W2, b2, w3, b3, cv = torch.randn(d, d) / 8, torch.randn(d), torch.randn(d), torch.randn(1), torch.randn(d)
    extra = (w / 40) if skip else None
    y = (torch.rand(e) < 0.3).float()
    pw = torch.tensor(2.5)
    s0, d0 = int(ei[0, 0]), int(ei[1, 2])
    zeroed = None
    if inject == "nan_p":
        P[s0] = NAN
    elif inject == "negnan_p":
        set_negative_nan(P, s0)
    elif inject == "inf_q":
        Q[d0] = INF
    elif inject == "ninf_q":
        Q[d0] = -INF                                  # h1 = -inf in every column: relu gives 0, the edge's logit is finite
    elif inject == "nan_unused":
        assert not ((ei == 0) | (ei == n - 1)).any()
        zeroed = (P.clone(), Q.clone())
        for t in zeroed:
            t[0], t[n - 1] = 0.0, 0.0
        P[0], P[n - 1], Q[0], Q[n - 1] = NAN, NAN, NAN, -INF
    elif inject == "inf_w2":
        W2[3, 5] = INF
    elif inject == "inf_extra":
        extra[4] = INF
    lv = [t.clone().double().requires_grad_(True) for t in (P, Q, W2, b2, w3, b3, cv)]
    h1 = lv[0][ei[0]] + lv[1][ei[1]]
    if skip:
        h1 = h1 + extra.double().unsqueeze(1) * lv[6]
    ref = torch.relu(torch.relu(h1) @ lv[2].t() + lv[3]) @ lv[4] + lv[5]
    lref = F.binary_cross_entropy_with_logits(ref, y.double(), pos_weight=pw.double())
    lref.backward()
    grads = [None if (k == 6 and not skip) else lv[k].grad for k in range(7)]
    return dict(e=e, skip=skip, inject=inject, ei=ei, d0=d0, P=P, Q=Q, W2=W2, b2=b2, w3=w3, b3=b3, cv=cv, extra=extra, y=y, pw=pw,
                zeroed=zeroed, logits=ref.detach(), loss=lref.detach(), grads=grads)


@pytest.mark.parametrize("e,skip,inject,table", DEC_CASES)
def test_decoder_references_are_informative(e, skip, inject, table):
    c = decoder_case(e, skip, inject, table)
    if inject in DEC_ALL_FINITE:
        assert informative(c["logits"], expect_nonfinite=False) and torch.isfinite(c["loss"])
        assert all(g is None or torch.isfinite(g).all() for g in c["grads"])
        return
    if inject == "inf_w2":
        # one inf in W2 meets a zero of relu(h1) in every edge's row (0 * inf): no logit is finite, in torch as here — the one
        # case whose reference cannot keep half of its elements finite
        assert not torch.isfinite(c["logits"]).any()
    else:
        assert informative(c["logits"]), int((~torch.isfinite(c["logits"])).sum())
    assert not torch.isfinite(c["loss"])
    assert all(g is None or not torch.isfinite(g).all() for g in c["grads"])     # every gradient tensor must raise the alarm


class _precision:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from pangnn_amd import functional as PF
        self.old, PF.DECODER_PRECISION = PF.DECODER_PRECISION, self.mode

    def __exit__(self, *a):
        from pangnn_amd import functional as PF
        PF.DECODER_PRECISION = self.old


def _run_decoder(c, mode, tables=None):
    """(logits, loss, grads) of decoder_loss and (logits, grads) of decoder_mlp + torch's BCE, on the device"""
    from pangnn_amd import functional as PF
    from pangnn_amd.graph import EdgeStructure
    P, Q = tables if tables is not None else (c["P"], c["Q"])
    skip, e = c["skip"], c["e"]
    st = EdgeStructure(c["ei"].to(_dev()), DEC_N)
    ex = c["extra"].to(_dev()) if skip else None
    y, pw = c["y"].to(_dev()), c["pw"].to(_dev())
    out = {}
    with _precision(mode):
        gl = [t.clone().to(_dev()).requires_grad_(True) for t in (P, Q, c["W2"], c["b2"], c["w3"], c["b3"], c["cv"])]
        loss, logits = PF.decoder_loss(gl[0], gl[1], st, ex, gl[6] if skip else None, gl[2], gl[3], gl[4], gl[5], y, pw, e)
        loss.backward()
        out["fused"] = (logits.detach(), loss.detach(), [None if (k == 6 and not skip) else gl[k].grad for k in range(7)])
        gl2 = [t.clone().to(_dev()).requires_grad_(True) for t in (P, Q, c["W2"], c["b2"], c["w3"], c["b3"], c["cv"])]
        out2 = PF.decoder_mlp(gl2[0], gl2[1], st, ex, gl2[6] if skip else None, gl2[2], gl2[3], gl2[4], gl2[5])
        l2 = F.binary_cross_entropy_with_logits(out2, y, pos_weight=pw)
        l2.backward()
        out["mlp"] = (out2.detach(), l2.detach(), [None if (k == 6 and not skip) else gl2[k].grad for k in range(7)])
    torch.cuda.synchronize()
    return out


def _decoder_grad_bound(c, k, table):
    """test_decoder_training_kernels_vs_fp64's bound; a gradient of a 2-byte table comes back in that type: one rounding
    (2^-9 bf16, 2^-12 f16 of the element, 2^-25 absolute in float16's subnormal range) on top"""
    tol = 1e-6 if c["e"] >= 1000 else 8e-6
    store = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}[table] if k < 2 else 0.0

    def bound(got, ref):
        scale = float(ref.abs().max()) + 1e-30
        return bool(((got - ref).abs() <= tol * scale + store * ref.abs() + (2.0 ** -24 if store else 0.0)).all())
    return bound


DEC_GPU_CASES = [pytest.param(*c, mode, id="-".join(map(str, c)) + ("-bf16x3" if mode else "-f32mfma"))
                 for mode in (1, 0) for c in DEC_CASES]


def _expected_of_mode(c, mode):
    """(logits, loss, grads) the decoder of `mode` is held to: torch's float64 results — except the ONE stated difference of
    the default decoder (mode 1), whose relu is x + |x| (decoder16.hip, relu2x: the one-instruction form that keeps a NaN;
    the exact compare + select costs 1.2 % of the headline step, profiles/nonfinite.md): relu2x(-inf) = NaN
    where relu(-inf) = 0.  In the `ninf_q` case exactly the edges INTO the -inf row of Q come out NaN there (h1 = -inf in every
    column), with them the loss and — their dL/dlogit being NaN — every gradient tensor; every other logit is torch's, to the
    usual bound.  The strict-fp32 decoder (mode 0) is held to torch without exception."""
    if not (mode == 1 and c["inject"] == "ninf_q"):
        return c["logits"], c["loss"], c["grads"]
    hit = c["ei"][1] == c["d0"]
    assert 1 <= int(hit.sum()) <= c["e"] // 2
    logits = torch.where(hit, torch.full_like(c["logits"], NAN), c["logits"])
    grads = [None if g is None else torch.full_like(g, NAN) for g in c["grads"]]
    return logits, torch.full_like(c["loss"], NAN), grads


@pytest.mark.gpu
@pytest.mark.parametrize("e,skip,inject,table,mode", DEC_GPU_CASES)
def test_decoder_passes_nonfinite_values_like_torch(e, skip, inject, table, mode):
    c = decoder_case(e, skip, inject, table)
    res = _run_decoder(c, mode)
    want_logits, want_loss, want_grads = _expected_of_mode(c, mode)
    for route, (logits, loss, grads) in res.items():
        tag = f"{route} E={e} skip={skip} {inject} {table} mode={mode}"
        assert_same_nonfinite(logits, want_logits, finite_bound=allclose_bound(1.6e-5, 2e-6), what=tag + " logits")
        assert_same_nonfinite(loss, want_loss, finite_bound=allclose_bound(1e-6, 1e-5), what=tag + " loss")
        for k, name in enumerate(DEC_NAMES):
            if want_grads[k] is None:
                continue
            assert_same_nonfinite_tensorwise(grads[k], as_stored(want_grads[k], table if k < 2 else "f32"),
                                             finite_bound=_decoder_grad_bound(c, k, table),
                                             what=f"{tag} dL/d{name}")
    if inject == "nan_unused":                           # rule 3: bit-equal to the call with those rows zeroed
        zero = _run_decoder(c, mode, tables=c["zeroed"])
        for route in res:
            (lg, ls, gr), (lg0, ls0, gr0) = res[route], zero[route]
            assert torch.equal(lg, lg0) and torch.equal(ls, ls0), route
            for k, name in enumerate(DEC_NAMES):
                if gr[k] is not None:
                    assert torch.equal(gr[k], gr0[k]), (route, name)


# ================================================================================================ edge_score / edge_score_loss
SCORE_GRAPHS = {"n50_e333": (50, 333, None, 0), "n3000_e30000_star": (3000, 30000, 20000, 4)}     # test_edge_score._graph_cases
SCORE_INJECT = ("nan", "inf", "nan_unused")
SCORE_CASES = [(g, d, tab, inj) for g in SCORE_GRAPHS for d in (16, 256) for tab in TABLES for inj in SCORE_INJECT]


@functools.lru_cache(maxsize=None)
def score_case(graph, d, table, inject):
    """the graph with two more nodes that no edge touches; rows as stored; z[1] = 0 and |z[2]| < eps stay in as finite controls"""
    n0, e, hub, seed = SCORE_GRAPHS[graph]
    ei, _ = random_graph(n0, e, seed=seed, hub=hub)
    n = n0 + 2
    gen = torch.Generator().manual_seed(d + n0)
    z = torch.randn(n, d, generator=gen) / d ** 0.5
    z[1] = 0.0
    z[2] *= 1e-10
    z = z.to(TABLES[table])
    node = int(ei[0, 7])
    assert node not in (1, 2)
    zeroed = None
    if inject == "nan":
        z[node] = NAN
    elif inject == "inf":
        z[node] = INF
    else:
        zeroed = z.clone()
        zeroed[n0:] = 0.0
        z[n0], z[n0 + 1] = NAN, INF
    g = torch.randn(e, generator=gen)
    y = (torch.rand(e, generator=gen) < 0.3).float()
    pw = torch.tensor(2.5)
    ref = {}
    for mode in ("dot", "cosine"):
        zz = z.double().requires_grad_(True)
        a, b = zz[ei[0]], zz[ei[1]]
        s = F.cosine_similarity(a, b, dim=1) if mode == "cosine" else (a * b).sum(1)
        s.backward(g.double())
        zl = z.double().requires_grad_(True)
        a, b = zl[ei[0]], zl[ei[1]]
        sl = F.cosine_similarity(a, b, dim=1) if mode == "cosine" else (a * b).sum(1)
        loss = F.binary_cross_entropy_with_logits(sl, y.double(), pos_weight=pw.double())
        loss.backward()
        ref[mode] = (s.detach(), zz.grad, loss.detach(), zl.grad)
    return dict(n=n, ei=ei, z=z, zeroed=zeroed, g=g, y=y, pw=pw, ref=ref)


@pytest.mark.parametrize("graph,d,table,inject", SCORE_CASES)
def test_edge_score_references_are_informative(graph, d, table, inject):
    c = score_case(graph, d, table, inject)
    for mode, (s, gz, loss, gzl) in c["ref"].items():
        if inject == "nan_unused":
            assert informative(s, expect_nonfinite=False) and torch.isfinite(gz).all() and torch.isfinite(loss)
            assert torch.isfinite(gzl).all()
        else:
            assert informative(s), (mode, int((~torch.isfinite(s)).sum()))
            assert not torch.isfinite(gz).all() and not torch.isfinite(loss) and not torch.isfinite(gzl).all()


def _run_score(c, mode, z):
    from pangnn_amd import functional as PF
    from pangnn_amd.graph import structure_of
    eid = c["ei"].to(_dev())
    st = structure_of(eid, c["n"])
    zd = z.to(_dev()).requires_grad_(True)
    out = PF.edge_score(zd, st, mode)
    out.backward(c["g"].to(_dev()))
    zl = z.to(_dev()).requires_grad_(True)
    loss, logits = PF.edge_score_loss(zl, st, mode, c["y"].to(_dev()), c["pw"].to(_dev()), c["ei"].shape[1])
    loss.backward()
    torch.cuda.synchronize()
    return out.detach(), zd.grad, loss.detach(), logits.detach(), zl.grad


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["dot", "cosine"])
@pytest.mark.parametrize("graph,d,table,inject", SCORE_CASES)
def test_edge_score_passes_nonfinite_values_like_torch(graph, d, table, inject, mode):
    c = score_case(graph, d, table, inject)
    s64, gz64, loss64, gzl64 = c["ref"][mode]
    out, gz, loss, logits, gzl = _run_score(c, mode, c["z"])
    tag = f"{graph} D={d} {table} {inject} {mode}"
    fin = s64[torch.isfinite(s64)]
    lscale = max(1.0, float(fin.abs().max())) if fin.numel() else 1.0
    logit_bound = allclose_bound(1e-6 * lscale, 0.0)                      # test_edge_score._check_against_f64
    assert_same_nonfinite(out, s64, finite_bound=logit_bound, what=tag + " logits")
    assert_same_nonfinite(logits, s64, finite_bound=logit_bound, what=tag + " logits of the loss form")
    assert_same_nonfinite(loss, loss64, finite_bound=allclose_bound(1e-6, 1e-5), what=tag + " loss")
    # gradient rows come back in z's type: one rounding of that type on top of the kernel test's 2e-6 of the tensor's scale
    store = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}[table]

    def grad_bound(got, ref):
        scale = float(ref.abs().max()) + 1e-30
        return bool(((got - ref).abs() <= 2e-6 * scale + store * ref.abs() + (2.0 ** -24 if store else 0.0)).all())
    # (a zero row's cosine gradient is ~1/eps = 1e8: inf once stored as float16, in torch as here)
    assert_same_nonfinite_tensorwise(gz, as_stored(gz64, table), finite_bound=grad_bound, what=tag + " dL/dz")
    assert_same_nonfinite_tensorwise(gzl, as_stored(gzl64, table), finite_bound=grad_bound, what=tag + " dL/dz of the loss form")
    if inject == "nan_unused":
        got0 = _run_score(c, mode, c["zeroed"])
        for a, b, name in zip((out, gz, loss, logits, gzl), got0, ("logits", "dL/dz", "loss", "loss logits", "loss dL/dz")):
            assert torch.equal(a, b), (tag, name)


# ================================================================================================ BCEWithLogits
BCE_LOGITS = (0.0, 1e-8, -1e-8, 17.0, -17.0, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0, 1e4, -1e4)
BCE_PW = (None, 4.7, 0.0)


def _bce64(x, y, pw, denom=None):
    """(loss, dL/dx) of torch in float64; `denom`: mean over that many elements"""
    xr = x.double().clone().requires_grad_(True)
    l = F.binary_cross_entropy_with_logits(xr, y.double(), pos_weight=None if pw is None else torch.tensor(pw).double(),
                                           reduction="sum") / (x.numel() if denom is None else denom)
    l.backward()
    return l.detach(), xr.grad


def test_bce_range_ends_are_finite_in_float64():
    for pw in BCE_PW:
        for x in BCE_LOGITS:
            for y in (0.0, 1.0):
                l, g = _bce64(torch.tensor([x]), torch.tensor([y]), pw)
                assert torch.isfinite(l) and torch.isfinite(g).all()


@pytest.mark.gpu
@pytest.mark.parametrize("pw", BCE_PW, ids=["none", "4.7", "0"])
def test_bce_range_ends_one_element_at_a_time(pw):
    """every logit of the list with label 0 and 1 as a call of its own (the loss IS that element's term): the tails where
    1 + t == 1 (|x| >= 17) and where t = exp(-|x|) underflows (|x| >= 88, 104) are held to torch float64"""
    from pangnn_amd import functional as PF
    pwt = None if pw is None else torch.tensor(pw, device=_dev())
    for x in BCE_LOGITS:
        for y in (0.0, 1.0):
            xt, yt = torch.tensor([x]), torch.tensor([y])
            l64, g64 = _bce64(xt, yt, pw)
            xg = xt.to(_dev()).requires_grad_(True)
            out = PF.bce_with_logits(xg, yt.to(_dev()), pwt, denom=1)
            out.backward()
            assert torch.isfinite(out) and torch.isfinite(xg.grad).all(), (x, y, pw)
            assert_same_nonfinite(out, l64, finite_bound=allclose_bound(1e-6, 1e-5), what=f"loss x={x} y={y} pw={pw}")
            assert_same_nonfinite(xg.grad, g64, finite_bound=allclose_bound(1e-9, 1e-4), what=f"grad x={x} y={y} pw={pw}")


@pytest.mark.gpu
@pytest.mark.parametrize("pw", BCE_PW, ids=["none", "4.7", "0"])
def test_bce_range_ends_inside_edge_score_loss(pw):
    """the same arithmetic inside edge_score_loss: D = 16 rows (x, 0, ..) and (1, 0, ..) give the dot-product logit x exactly"""
    from pangnn_amd import functional as PF
    from pangnn_amd import torch_ops  # noqa: F401
    pwt = None if pw is None else torch.tensor(pw, device=_dev())
    z = torch.zeros(2, 16)
    z[1, 0] = 1.0
    ei = torch.tensor([[0], [1]], device=_dev())
    for x in BCE_LOGITS:
        for y in (0.0, 1.0):
            z[0, 0] = x
            l64, g64 = _bce64(torch.tensor([x]), torch.tensor([y]), pw)
            loss, logits, g_l, _ = torch.ops.pangnn.edge_score_loss(z.to(_dev()), ei, PF.SCORE_MODES["dot"],
                                                                    torch.tensor([y], device=_dev()), pwt, 1)
            assert float(logits[0]) == float(torch.tensor(x, dtype=torch.float32))
            assert_same_nonfinite(loss, l64, finite_bound=allclose_bound(1e-6, 1e-5), what=f"loss x={x} y={y} pw={pw}")
            assert_same_nonfinite(g_l, g64, finite_bound=allclose_bound(1e-9, 1e-4), what=f"grad x={x} y={y} pw={pw}")


DEC_LOGIT_SCALES = (1e-8, 1.0, 30.0, 2000.0)       # of w3 and b3: |logit| from ~1e-8 to ~1e4


@functools.lru_cache(maxsize=None)
def scaled_decoder_case(scale):
    c = dict(decoder_case(1000, False, "nan_unused", "f32"))
    c["P"], c["Q"] = c["zeroed"]
    c["w3"], c["b3"] = c["w3"] * scale, c["b3"] * scale
    with torch.no_grad():
        h1 = c["P"].double()[c["ei"][0]] + c["Q"].double()[c["ei"][1]]
        c["logits"] = torch.relu(torch.relu(h1) @ c["W2"].double().t() + c["b2"].double()) @ c["w3"].double() + c["b3"].double()
    return c


def test_scaled_decoder_logits_reach_both_range_ends():
    lo, hi = scaled_decoder_case(1e-8)["logits"].abs(), scaled_decoder_case(2000.0)["logits"]
    assert float(lo.max()) < 1e-6 and float(hi.max()) > 1e3 and float(hi.min()) < -1e3
    mid = scaled_decoder_case(30.0)["logits"].abs()
    assert ((mid > 17) & (mid < 88)).any() and (mid > 104).any()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 0], ids=["bf16x3", "f32mfma"])
@pytest.mark.parametrize("scale", DEC_LOGIT_SCALES)
def test_bce_range_ends_inside_the_decoders_fused_loss(scale, mode):
    """both decoders' fused loss against float64 BCE evaluated on the kernel's own logits (as test_fused_loss_matches_torch_bce
    does), with w3 / b3 scaled so that the logits reach 1e-8 .. 1e4"""
    c = scaled_decoder_case(scale)
    logits, loss, grads = _run_decoder(c, mode)["fused"]
    assert torch.isfinite(logits).all() and torch.isfinite(loss) and all(g is None or torch.isfinite(g).all() for g in grads)
    l64, g64 = _bce64(logits.cpu(), c["y"], float(c["pw"]))
    assert_same_nonfinite(loss, l64, finite_bound=allclose_bound(1e-6, 1e-5), what=f"loss scale={scale} mode={mode}")
    # dL/db3 = the sum of dL/dlogit: pins the decoders' own form of the BCE gradient at these logits, to the bound
    # test_decoder_training_kernels_vs_fp64 holds dL/db3 to at E = 1000 (1e-6 of its size)
    gb3, want = grads[5].cpu().double().reshape(()), g64.sum()
    print(f"scale={scale} mode={mode}: dL/db3 {float(gb3):.9e} vs {float(want):.9e}, rel {abs(float(gb3 - want)) / abs(float(want)):.2e}")
    assert abs(float(gb3 - want)) <= 1e-6 * (abs(float(want)) + 1e-30)


BCE_BAD = torch.tensor([0.5, NAN, -2.0, INF, 3.0, -INF, 1.0, -1.0, INF, -INF])
BCE_BAD_Y = torch.tensor([0.0, 1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 1.0, 0.0])


def test_bce_nonfinite_reference_is_informative():
    l, g = _bce64(BCE_BAD, BCE_BAD_Y, 4.7)
    assert not torch.isfinite(l) and informative(g)
    assert torch.isnan(g[1]) and torch.isfinite(g[[3, 5, 8, 9]]).all()      # the sigmoid saturates: +-inf logits give finite gradients


@pytest.mark.gpu
@pytest.mark.parametrize("pw", BCE_PW, ids=["none", "4.7", "0"])
def test_bce_passes_nonfinite_logits_like_torch(pw):
    from pangnn_amd import functional as PF
    l64, g64 = _bce64(BCE_BAD, BCE_BAD_Y, pw)
    xg = BCE_BAD.to(_dev()).requires_grad_(True)
    out = PF.bce_with_logits(xg, BCE_BAD_Y.to(_dev()), None if pw is None else torch.tensor(pw, device=_dev()))
    out.backward()
    assert_same_nonfinite(out, l64, finite_bound=allclose_bound(1e-6, 1e-5), what=f"loss pw={pw}")
    assert_same_nonfinite(xg.grad, g64, finite_bound=allclose_bound(1e-9, 1e-4), what=f"dL/dlogit pw={pw}")


# ================================================================================================ normalize_sim_scores
SIM_LENGTHS = (1, 2, 63, 64, 65, 129, 500)


@functools.lru_cache(maxsize=None)
def sim_case():
    """two genomes; source gene s (genome 0) has SIM_LENGTHS[s % 7] candidates in genome 1: three rounds of the lengths — plain,
    one NaN per segment, one +inf per segment; equal values and +-1e4 in every round"""
    gen = torch.Generator().manual_seed(5)
    n_src = 3 * len(SIM_LENGTHS)
    n_dst = max(SIM_LENGTHS)
    src, dst, score = [], [], []
    for s in range(n_src):
        ln = SIM_LENGTHS[s % len(SIM_LENGTHS)]
        sc = torch.rand(ln, generator=gen, dtype=torch.float64) * 300
        if ln >= 2:
            sc[1] = sc[0]                                     # equal values
        if ln >= 63:
            sc[5], sc[6] = 1e4, -1e4
        if s // len(SIM_LENGTHS) == 1:
            sc[ln // 2] = NAN
        if s // len(SIM_LENGTHS) == 2:
            sc[ln - 1] = INF
        src.append(torch.full((ln,), s, dtype=torch.int64))
        dst.append(n_src + torch.randperm(n_dst, generator=gen)[:ln])
        score.append(sc)
    src, dst, score = torch.cat(src), torch.cat(dst), torch.cat(score)
    order = torch.randperm(src.numel(), generator=gen)        # the relation arrives unsorted
    genome_of = torch.cat([torch.zeros(n_src, dtype=torch.int64), torch.ones(n_dst, dtype=torch.int64)])
    return src[order], dst[order], score[order], genome_of


def test_normalize_sim_scores_cpu_leg_equals_the_oracle_with_nonfinite_scores():
    from oracle import construct_oracle as co
    from pangnn_amd import construct
    src, dst, score, genome_of = sim_case()
    s, d, w = construct.normalize_sim_scores(src, dst, score, genome_of)
    with np.errstate(all="ignore"):                                            # inf - inf inside scipy's logsumexp: intended
        so, do, wo = co.normalize_sim_scores(src.numpy(), dst.numpy(), score.numpy(), genome_of.numpy())
    assert np.array_equal(s.numpy(), so) and np.array_equal(d.numpy(), do)
    assert np.isfinite(wo).all() and torch.isfinite(w).all()                   # the nan_to_num branch: q is finite everywhere
    assert np.allclose(w.numpy(), wo, rtol=1e-12, atol=1e-12)
    nan_seg = torch.isnan(score)
    seg_of_nan = set(s[nan_seg].tolist())
    hit = torch.tensor([int(v) in seg_of_nan for v in s.tolist()]) & (torch.bincount(s)[s] > 1)
    assert hit.sum() > nan_seg.sum()                                           # the NaN marks its whole segment ...
    assert (w[hit] == -10.0 * math.log10(1.0 - 1e-8) + 1.0).all()              # ... with the isnan branch's value


@pytest.mark.gpu
def test_normalize_sim_scores_device_leg_equals_its_cpu_leg_with_nonfinite_scores():
    from pangnn_amd import construct
    src, dst, score, genome_of = sim_case()
    s, d, w = construct.normalize_sim_scores(src, dst, score, genome_of)
    sd, dd, wd = construct.normalize_sim_scores(src.to(_dev()), dst.to(_dev()), score.to(_dev()), genome_of.to(_dev()))
    key = lambda a, b: torch.argsort(a * 10000 + b, stable=True)               # noqa: E731  (the device leg returns key order)
    o, od = key(s, d), key(sd.cpu(), dd.cpu())
    assert torch.equal(s[o], sd.cpu()[od]) and torch.equal(d[o], dd.cpu()[od])
    assert_same_nonfinite(wd.cpu()[od], w[o], finite_bound=allclose_bound(5e-7, 5e-7), what="q scores")


# ================================================================================================ fused EdgeConv
CONV_CASES = [(out, inj) for out in (64, 128) for inj in ("nan", "nan_unused")]


@functools.lru_cache(maxsize=None)
def conv_case(out, inject):
    from oracle import gcn_oracle as go
    n, c = 300, 8
    ei = random_graph(n - 2, 2500, seed=9)[0] + 1               # nodes 0 and 299: no edge
    torch.manual_seed(out)
    ref_m = go.EdgeConvOracle(c, out)
    x = torch.randn(n, c)
    zeroed = None
    if inject == "nan":
        x[int(ei[0, 7])] = NAN
    else:
        zeroed = x.clone()
        zeroed[0], zeroed[n - 1] = 0.0, 0.0
        x[0], x[n - 1] = NAN, INF
    m64 = go.EdgeConvOracle(c, out).double()
    m64.load_state_dict({k: v.double() for k, v in ref_m.state_dict().items()})
    with torch.no_grad():
        ref64 = m64((zeroed if zeroed is not None else x).double(), ei)
    return n, ei, ref_m, x, zeroed, ref64


@pytest.mark.parametrize("out,inject", CONV_CASES)
def test_edge_conv_references_are_informative(out, inject):
    n, ei, ref_m, x, zeroed, ref64 = conv_case(out, inject)
    if inject == "nan_unused":
        assert not ((ei == 0) | (ei == n - 1)).any() and torch.isfinite(ref64).all()
        return
    # the literal route's definition is position-wise (rule 4); the rows the NaN node feeds are the non-finite ones
    node = int(torch.nonzero(torch.isnan(x).any(1))[0])
    fed = torch.unique(ei[1][(ei[0] == node) | (ei[1] == node)])
    assert 1 <= fed.numel() <= n // 2
    assert informative(ref64)                                  # the float64 oracle (scatter amax keeps a NaN) on the same input
    assert torch.nonzero(~torch.isfinite(ref64).all(1)).flatten().tolist() == sorted(fed.tolist())


def _conv_forward(m, x, ei, flag):
    from pangnn_amd import functional as PF
    old, PF.FUSE_EDGE_CONV = PF.FUSE_EDGE_CONV, flag
    try:
        with torch.no_grad():
            return m(x, ei)
    finally:
        PF.FUSE_EDGE_CONV = old


@pytest.mark.gpu
@pytest.mark.parametrize("out,inject", CONV_CASES)
def test_fused_edge_conv_is_the_literal_route_position_by_position(out, inject):
    """forward only.  The backward is not held to the literal route here: the fused form takes the first Linear at node level
    (u = x (Wa - Wb)^T for EVERY node), so its weight gradient g_u^T x meets an unreferenced NaN row of x as 0 * NaN where the
    literal route, which gathers x per edge, never reads it (measured: dL/d mlp.0.weight non-finite against finite) — the
    same holds for any node-level Linear in torch itself."""
    import pangnn_amd
    n, ei, ref_m, x, zeroed, ref64 = conv_case(out, inject)
    m = pangnn_amd.EdgeConv(8, out).to(_dev())
    m.load_state_dict(ref_m.state_dict())
    xd, eid = x.to(_dev()), ei.to(_dev())
    fused, literal = _conv_forward(m, xd, eid, True), _conv_forward(m, xd, eid, False)
    assert_same_nonfinite(fused, literal, finite_bound=allclose_bound(1e-4, 1e-4), what=f"EdgeConv out={out} {inject}")
    if inject == "nan_unused":
        assert torch.equal(fused, _conv_forward(m, zeroed.to(_dev()), eid, True))
        assert_same_nonfinite(fused, ref64, finite_bound=allclose_bound(1e-4, 1e-4), what="EdgeConv vs float64")


# ================================================================================================ pangnn_scale_unless_one_f32
@pytest.mark.gpu
@pytest.mark.parametrize("scale", [INF, -INF, NAN])
def test_scale_unless_one_with_a_nonfinite_scale_is_torchs_product(scale):
    """a GradScaler's scale times an overflowed loss gradient: every buffer equals t * scale in torch, 0 * inf = NaN included"""
    import ctypes as C
    from pangnn_amd import _lib
    lib = _lib.load()
    torch.manual_seed(0)
    bufs = [torch.randn(1003, device=_dev()), torch.randn(64, 128, device=_dev()), torch.randn(1, device=_dev())]
    bufs[0][5], bufs[0][6], bufs[0][7], bufs[1][3, 3] = 0.0, -0.0, INF, NAN
    work = [b.clone() for b in bufs]
    ptrs = (C.c_void_p * len(work))(*[w.data_ptr() for w in work])
    counts = (C.c_int64 * len(work))(*[w.numel() for w in work])
    sc = torch.tensor(scale, device=_dev())
    _lib.check(lib.pangnn_scale_unless_one_f32(ptrs, counts, len(work), sc.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    for w, b in zip(work, bufs):
        want = b * sc
        assert not torch.isfinite(want).any()
        assert torch.equal(torch.isnan(w), torch.isnan(want)) and torch.equal(w[~torch.isnan(w)], want[~torch.isnan(want)])


# ================================================================================================ functional.linear forward
LIN_N = 33                                            # one full 32-row tile + one row
LIN_INJECT = ("nan_x", "pinf_x", "ninf_x", "inf_w", "nan_bias")
LIN_CASES = [(k, m, in_act, xt, yt, inj) for (k, m) in ((64, 128), (128, 64)) for in_act in (0, 1)
             for xt, yt in (("f32", "f32"), ("f32", "bf16"), ("f32", "f16"), ("f16", "f32"), ("f16", "f16"))
             for inj in LIN_INJECT]


@functools.lru_cache(maxsize=None)
def linear_case(k, m, in_act, xt, inject):
    torch.manual_seed(k + 2 * m + in_act)
    x = torch.randn(LIN_N, k).to(TABLES[xt])
    w, b = torch.randn(m, k) / k ** 0.5, torch.randn(m)
    if inject == "nan_x":
        x[3] = NAN
    elif inject == "pinf_x":
        x[17, 5] = INF
    elif inject == "ninf_x":
        x[32] = -INF                                  # in_act = 1: elu(-inf) = -1, a finite row
    elif inject == "inf_w":
        w[7, 11] = INF
    elif inject == "nan_bias":
        b[9] = NAN
    xa = F.elu(x.double()) if in_act else x.double()
    ref = F.linear(xa, w.double(), b.double())
    return x, w, b, ref


@pytest.mark.parametrize("k,m,in_act,xt,inject", sorted({(k, m, a, xt, inj) for k, m, a, xt, _, inj in LIN_CASES}))
def test_linear_references_are_informative(k, m, in_act, xt, inject):
    x, w, b, ref = linear_case(k, m, in_act, xt, inject)
    if inject == "ninf_x" and in_act == 1:
        assert informative(ref, expect_nonfinite=False)          # elu(-inf) = -1: torch's row is finite, so must ours be
    else:
        assert informative(ref), int((~torch.isfinite(ref)).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("k,m,in_act,xt,yt,inject", LIN_CASES)
def test_linear_forward_passes_nonfinite_values_like_torch(k, m, in_act, xt, yt, inject):
    from pangnn_amd import functional as PF
    x, w, b, ref = linear_case(k, m, in_act, xt, inject)
    out = PF.linear(x.to(_dev()), w.to(_dev()), b.to(_dev()), in_act=in_act, out_dtype=TABLES[yt])
    assert out.dtype == TABLES[yt]
    # test_linear_kernels_match_torch's bound, plus one rounding of the stored type (2^-9 bf16, 2^-12 f16; 2^-25 absolute in
    # float16's subnormal range)
    store = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}[yt]

    def bound(got, r):
        return bool(((got - r).abs() <= 1e-4 + 1e-5 * r.abs() + store * r.abs() + (2.0 ** -24 if store else 0.0)).all())
    assert_same_nonfinite(out, as_stored(ref, yt), finite_bound=bound, what=f"linear {k}->{m} act={in_act} x={xt} y={yt} {inject}")


@functools.lru_cache(maxsize=None)
def f16_store_case(k, m):
    """rows whose products are 1e5 (inf in float16), 3e4 (finite) and in float16's subnormal range (stored exactly): x row r is
    v_r in column 0 and 0 elsewhere, w[:, 0] = 1, so out[r, j] = v_r exactly in fp32"""
    x = torch.zeros(LIN_N, k)
    vals = {0: 1e5, 1: 3e4, 2: -1e5, 3: -3e4, 4: 2.0 ** -24, 5: 3 * 2.0 ** -24, 6: 2.0 ** -15, 7: 1000 * 2.0 ** -24, 32: 6e4}
    for r, v in vals.items():
        x[r, 0] = v
    w = torch.zeros(m, k)
    w[:, 0] = 1.0
    ref32 = F.linear(x, w)                            # the float16-overflow reference: torch float32, then .half()
    return x, w, vals, ref32.half()


@pytest.mark.parametrize("k,m", [(64, 128), (128, 64)])
def test_f16_store_reference_is_informative(k, m):
    x, w, vals, ref = f16_store_case(k, m)
    assert informative(ref) and torch.isinf(ref[0]).all() and torch.isinf(ref[2]).all() and torch.isfinite(ref[1]).all()
    for r in (4, 5, 6, 7):
        assert 2.0 ** -24 <= vals[r] < 2.0 ** -14 and (ref[r].float() == vals[r]).all()      # float16 subnormals (6e-8 .. 6e-5), exact


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(64, 128), (128, 64)])
def test_linear_float16_store_overflows_and_keeps_subnormals_like_half(k, m):
    from pangnn_amd import functional as PF
    x, w, vals, ref = f16_store_case(k, m)
    out = PF.linear(x.to(_dev()), w.to(_dev()), None, out_dtype=torch.float16)
    assert out.dtype == torch.float16 and torch.equal(out.cpu().view(torch.int16), ref.view(torch.int16))
    back = PF.linear(out, torch.eye(m, device=_dev()), None)                          # float16 rows read as stored
    rows = [1, 3, 4, 5, 6, 7]
    assert torch.equal(back.cpu()[rows], ref.float()[rows])                           # subnormals intact


# ================================================================================================ linear: wgrad and dgrad
LIN_GRAD_CASES = [(k, m, in_act, tab) for (k, m) in ((64, 128), (128, 64)) for in_act in (0, 1) for tab in TABLES]


@functools.lru_cache(maxsize=None)
def linear_grad_case(k, m, in_act, table):
    """one inf in one row of the upstream gradient: a float16 gradient row after the GradScaler's 65 536 x"""
    torch.manual_seed(3 * k + m + in_act)
    dt = TABLES[table]
    x = torch.randn(LIN_N, k).to(dt)
    w, b = torch.randn(m, k) / k ** 0.5, torch.randn(m)
    g = torch.randn(LIN_N, m).to(dt)
    g[20, 7] = INF
    lv = [x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)]
    F.linear(F.elu(lv[0]) if in_act else lv[0], lv[1], lv[2]).backward(g.double())
    return x, w, b, g, [t.grad for t in lv]


@pytest.mark.parametrize("k,m,in_act,table", LIN_GRAD_CASES)
def test_linear_grad_references_are_informative(k, m, in_act, table):
    gx, gw, gb = linear_grad_case(k, m, in_act, table)[4]
    assert informative(gx) and informative(gw) and informative(gb)       # row 20 of dL/dx, row 7 of dL/dw, entry 7 of dL/db


@pytest.mark.gpu
@pytest.mark.parametrize("k,m,in_act,table", LIN_GRAD_CASES)
def test_linear_wgrad_and_dgrad_pass_an_overflowed_gradient_row(k, m, in_act, table):
    """the gated (in_act = 1: dL/dx comes out multiplied by ELU') and the bf16 / f16 variants of the backward kernels"""
    from pangnn_amd import functional as PF
    x, w, b, g, ref = linear_grad_case(k, m, in_act, table)
    lv = [t.to(_dev()).requires_grad_(True) for t in (x, w, b)]
    out = PF.linear(lv[0], lv[1], lv[2], in_act=in_act, out_dtype=TABLES[table])
    out.backward(g.to(_dev()))
    # position by position: the inf reaches row 20 of dL/dx, row 7 of dL/dw and entry 7 of dL/db, everything else stays finite and
    # within test_linear_kernels_match_torch's bound (atol = rtol = 1e-4; dL/dx comes back in x's type: one rounding of it on top)
    store = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}[table]
    for got, r, name, st_ in zip((t.grad for t in lv), ref, ("dL/dx", "dL/dw", "dL/db"), (store, 0.0, 0.0)):
        assert_same_nonfinite(got, r, finite_bound=allclose_bound(1e-4, 1e-4 + st_),
                              what=f"linear {k}->{m} act={in_act} {table} {name}")


# ================================================================================================ propagate
PROP_N, PROP_F = 300, 64
# in-degrees of target rows 0 .. 6.  Row 6 is a hub past graph.LONG_ROW = 8192 and is walked as segments: the threshold is read when
# a structure is built, but a list of <= 16 384 edges is built by the one-launch path that rules long rows out, so the hub row (and
# 34 edges into each other row: 16 916 edges) it is
PROP_DEG = (0, 1, 63, 64, 65, 200, 8193)
PROP_A, PROP_B, PROP_C = 290, 291, 292               # sources: of one edge into row 4 / only of the hub row 6 / of nothing
PROP_INJECT = ("nan_ordinary", "nan_hub_only", "nan_unused", "inf_weight", "nan_grad_row")
PROP_CASES = [(tab, inj) for tab in TABLES for inj in PROP_INJECT]


@functools.lru_cache(maxsize=None)
def prop_graph():
    gen = torch.Generator().manual_seed(21)
    src, dst = [], []
    for row, deg in enumerate(PROP_DEG):
        src.append(torch.randint(6, 290, (deg,), generator=gen))
        dst.append(torch.full((deg,), row, dtype=torch.int64))
    src[4][0] = PROP_A
    src[6][3] = PROP_B
    rest = torch.arange(7, 250).repeat_interleave(34)
    src.append(torch.randint(6, 290, (rest.numel(),), generator=gen))
    dst.append(rest)
    ei = torch.stack([torch.cat(src), torch.cat(dst)])
    ei = ei[:, torch.randperm(ei.shape[1], generator=gen)]
    w = torch.rand(ei.shape[1], generator=gen) * 80 + 1
    return ei, w


@functools.lru_cache(maxsize=None)
def prop_case(table, inject):
    """x (as stored), per-edge weights, upstream gradient rows (as stored) and the float64 results of out = A x and
    gx = A^T g with A[dst, src] = w"""
    ei, w = prop_graph()
    gen = torch.Generator().manual_seed(len(inject))
    x = torch.randn(PROP_N, PROP_F, generator=gen).to(TABLES[table])
    g = torch.randn(PROP_N, PROP_F, generator=gen).to(TABLES[table])
    w = w.clone()
    zeroed = None
    if inject == "nan_ordinary":
        x[PROP_A] = NAN
    elif inject == "nan_hub_only":
        x[PROP_B] = NAN
    elif inject == "nan_unused":
        zeroed = x.clone()
        zeroed[PROP_C] = 0.0
        x[PROP_C] = NAN
    elif inject == "inf_weight":
        w[int(torch.nonzero(ei[1] == 3)[0])] = INF
    elif inject == "nan_grad_row":
        g[4] = NAN
    out = torch.zeros(PROP_N, PROP_F, dtype=torch.float64).index_add_(0, ei[1], w.double()[:, None] * x.double()[ei[0]])
    gx = torch.zeros(PROP_N, PROP_F, dtype=torch.float64).index_add_(0, ei[0], w.double()[:, None] * g.double()[ei[1]])
    return ei, w, x, g, zeroed, out, gx


@pytest.mark.parametrize("table,inject", PROP_CASES)
def test_propagate_references_are_informative(table, inject):
    ei, w, x, g, zeroed, out, gx = prop_case(table, inject)
    deg = torch.bincount(ei[1], minlength=PROP_N)
    assert deg[:7].tolist() == list(PROP_DEG) and ei.shape[1] > 16384
    assert (ei[0] == PROP_A).sum() == 1 and set(ei[1][ei[0] == PROP_B].tolist()) == {6} and not (ei == PROP_C).any()
    if inject == "nan_unused":
        assert informative(out, expect_nonfinite=False) and informative(gx, expect_nonfinite=False)
    elif inject == "nan_grad_row":
        assert informative(gx) and informative(out, expect_nonfinite=False)
    else:
        assert informative(out), int((~torch.isfinite(out)).sum())
        bad_rows = torch.nonzero(~torch.isfinite(out).all(1)).flatten().tolist()
        assert bad_rows == {"nan_ordinary": [4], "nan_hub_only": [6], "inf_weight": [3]}[inject]


@pytest.mark.gpu
@pytest.mark.parametrize("table,inject", PROP_CASES)
def test_spmm_forward_and_transposed_pass_nonfinite_values_like_torch(table, inject):
    from pangnn_amd import functional as PF
    from pangnn_amd.graph import EdgeStructure
    ei, w, x, g, zeroed, out64, gx64 = prop_case(table, inject)
    st = EdgeStructure(ei.to(_dev()), PROP_N)
    assert st.by_dst.long_rows() is not None and st.by_src.long_rows() is None
    wd = w.to(_dev())
    val_dst, val_src = wd[st.by_dst.perm.long()].contiguous(), wd[st.by_src.perm.long()].contiguous()

    def run(rows):
        o = PF.spmm_csr(st.by_dst, val_dst, rows.to(_dev()), PROP_N)
        t = PF.spmm_csr(st.by_src, val_src, g.to(_dev()), PROP_N)
        torch.cuda.synchronize()
        return o, t
    out, gx = run(x)
    # test_hip_parity's stated bound for intermediate tensors ("the same bound relative to magnitude": atol = rtol = 1e-4 of the
    # tensor's size — here raw weights up to 81 and rows up to 8 193 long, where that test's normalised weights keep sums O(1))
    scale = lambda r: allclose_bound(1e-4 * max(1.0, float(r[torch.isfinite(r)].abs().max())), 1e-4)        # noqa: E731
    assert_same_nonfinite(out, out64, finite_bound=scale(out64), what=f"A x {table} {inject}")
    assert_same_nonfinite(gx, gx64, finite_bound=scale(gx64), what=f"A^T g {table} {inject}")
    if inject == "nan_unused":
        out0, gx0 = run(zeroed)
        assert torch.equal(out, out0) and torch.equal(gx, gx0)


@functools.lru_cache(maxsize=None)
def band_case(table):
    """the positional-neighbour band (k = 1) on 300 nodes: inputs as stored and the float64 propagate + bias with its gradients"""
    from oracle import gcn_oracle as go
    from pangnn_amd import construct
    n, f = 300, PROP_F
    ei = construct.neighbour_edges(n, 1, device="cpu")
    gen = torch.Generator().manual_seed(2)
    x0 = torch.randn(n, f, generator=gen).to(TABLES[table])
    b0, g0 = torch.randn(f, generator=gen), torch.randn(n, f, generator=gen)
    x0[100], g0[200] = NAN, NAN
    xr, br = x0.double().requires_grad_(True), b0.double().requires_grad_(True)
    ref = go.propagate_add(xr, ei, go.gcn_norm(ei, None, n, dtype=torch.float64)) + br
    ref.backward(g0.double())
    return n, ei, x0, b0, g0, ref.detach(), xr.grad, br.grad


@pytest.mark.parametrize("table", list(TABLES))
def test_band_references_are_informative(table):
    n, ei, x0, b0, g0, ref, gx, gb = band_case(table)
    assert informative(ref) and informative(gx) and not torch.isfinite(gb).any()
    assert torch.nonzero(~torch.isfinite(ref).all(1)).flatten().tolist() == [99, 100, 101]
    assert torch.nonzero(~torch.isfinite(gx).all(1)).flatten().tolist() == [199, 200, 201]


@pytest.mark.gpu
@pytest.mark.parametrize("table", list(TABLES))
def test_propagate_and_band_propagate_pass_a_nan_row_like_the_oracle(table):
    """the autograd forms on the band: a NaN row of x reaches its two neighbours and itself, a NaN row of the upstream gradient
    likewise in the transposed pass; band kernel and generic kernel are both held to the float64 propagate position by position
    (test_spmm_forward_backward_match_oracle's atol = rtol = 1e-4; dL/dx comes back in x's type: one rounding of it on top)"""
    from pangnn_amd import functional as PF
    from pangnn_amd.graph import EdgeStructure
    n, ei, x0, b0, g0, ref, gx64, gb64 = band_case(table)
    st = EdgeStructure(ei.to(_dev()), n)
    assert st.band_width() == 1
    norm = st.gcn_norm(None)
    store = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}[table]
    for fn in (PF.band_propagate, PF.propagate):
        x, b = x0.to(_dev()).requires_grad_(True), b0.to(_dev()).requires_grad_(True)
        y = fn(x, b, st, norm)
        y.backward(g0.to(_dev()))
        assert_same_nonfinite(y, ref, finite_bound=allclose_bound(1e-4, 1e-4), what=f"{fn.__name__} {table}")
        assert_same_nonfinite(x.grad, gx64, finite_bound=allclose_bound(1e-4, 1e-4 + store), what=f"{fn.__name__} {table} dL/dx")
        assert_same_nonfinite(b.grad, gb64, finite_bound=allclose_bound(1e-4, 1e-4), what=f"{fn.__name__} {table} dL/db")


# ================================================================================================ end to end: the skipped step
E2E_FACTOR = 3e5          # on conv_out's weight: max |z| of the fp32 oracle is ~5, so z passes float16's 65 504 by a wide margin


def _e2e_graph():
    from conftest import whole_graph_from_golden
    g = whole_graph_from_golden("sim_200x4")
    return g, float((g.y == 0).sum() / g.y.sum())


@pytest.mark.parametrize("decoder", ["mlp", "cosine"])
def test_the_oracles_own_fp16_loop_skips_the_overflowed_step(decoder):
    """torch's side of the end-to-end test, on the CPU: under float16 autocast with a GradScaler(65536) the oracle takes one
    normal step, and after conv_out's weight is scaled by E2E_FACTOR its next step is skipped and the scale halved"""
    from oracle import gcn_oracle as go
    g, cb = _e2e_graph()
    torch.manual_seed(0)
    oracle = go.AlternateGCNOracle(dims=(64, 128), flags=go.default_flags(decoder=decoder))
    opt = torch.optim.Adam(oracle.parameters(), lr=1e-3)
    scaler = torch.amp.GradScaler("cpu", init_scale=65536.0)

    def step():
        opt.zero_grad()
        with torch.autocast("cpu", dtype=torch.float16):
            out = oracle(g)
        loss = F.binary_cross_entropy_with_logits(out.float(), g.y, pos_weight=torch.tensor(cb))
        scaler.scale(loss).backward()
        before = {k: v.clone() for k, v in oracle.state_dict().items()}
        scaler.step(opt)
        scaler.update()
        return loss.detach(), all(torch.equal(v, before[k]) for k, v in oracle.state_dict().items())
    loss, unchanged = step()
    assert torch.isfinite(loss) and not unchanged and scaler.get_scale() == 65536.0
    with torch.no_grad():
        assert float(oracle.encode(g).abs().max()) * E2E_FACTOR > 1e5
        oracle.conv_out.lin.weight.mul_(E2E_FACTOR)
    loss, unchanged = step()
    assert not torch.isfinite(loss) and unchanged and scaler.get_scale() == 32768.0


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["deferred", "plain", "cosine"])
def test_overflowed_fp16_step_is_skipped_as_torch_skips_it(route, monkeypatch):
    """test_reference_loop_under_accelerate_fp16_tracks_the_fp32_oracle_at_f16_resolution's loop on sim_200x4: one normal step,
    then conv_out's weight x E2E_FACTOR makes the float16 rows of z overflow — the step must be skipped (some gradient non-
    finite), every parameter bit-equal to before it, the scale halved.  Through the deferred-logits route, with
    PANGNN_DEFERRED_LOGITS=0, and with the cosine decoder."""
    import pangnn_amd
    from accelerate import Accelerator
    from accelerate.state import AcceleratorState
    from conftest import copy_graph
    from oracle import gcn_oracle as go
    g, cb = _e2e_graph()
    decoder = "cosine" if route == "cosine" else "mlp"
    torch.manual_seed(0)
    init = {k: v.clone() for k, v in go.AlternateGCNOracle(dims=(64, 128), flags=go.default_flags(decoder=decoder)).state_dict().items()}
    if route == "plain":
        monkeypatch.setenv("PANGNN_DEFERRED_LOGITS", "0")
    AcceleratorState._reset_state(True)
    try:
        accelerator = Accelerator(mixed_precision="fp16")
        assert accelerator.scaler is not None
        model = pangnn_amd.AlternateGCN(device=accelerator.device, dataset=None, categorical_nodes=False, dims=[64, 128],
                                        decoder=decoder)
        model.load_state_dict(init)
        optimizer = torch.optim.Adam(model.parameters(), lr=0.001)
        criterion = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor(cb))
        model, optimizer = accelerator.prepare(model, optimizer)
        batch = copy_graph(g, accelerator.device)

        def step():
            model.train()
            optimizer.zero_grad()
            output = model(batch)
            loss = criterion(output, batch.y)
            accelerator.backward(loss)
            optimizer.step()
            return output, loss.detach()
        output, loss = step()
        if route == "deferred":
            assert type(output) is pangnn_amd.DeferredLogits and output.route == "fused"
        elif route == "plain":
            assert type(output) is torch.Tensor
        scale0 = accelerator.scaler.get_scale()
        assert torch.isfinite(loss) and not optimizer.step_was_skipped and scale0 == 65536.0
        plain = accelerator.unwrap_model(model)
        with torch.no_grad():
            plain.conv_out.lin.weight.mul_(E2E_FACTOR)
        before = {k: v.clone() for k, v in plain.state_dict().items()}
        output, loss = step()
        assert not torch.isfinite(loss)
        assert optimizer.step_was_skipped, "an overflowed step was applied: some kernel swallowed the inf / NaN"
        for k, v in plain.state_dict().items():
            assert torch.equal(v, before[k]), k
        assert accelerator.scaler.get_scale() == scale0 / 2
    finally:
        AcceleratorState._reset_state(True)


# ================================================================================================ first layer by linearity
# conv_in(embedding(x)) = r a^T + s c^T + b_in with r = A_hat x, s = A_hat 1 (functional._EmbedConvIn): embed_conv_in
# (pangnn_embed_conv_in_rows / _grads, through the registered op: pangnn_rank2_rows / pangnn_weighted_colsum3), the same rows
# generated inside the next dense layer (embed_conv_in_linear), and the two kernels on their own with their bf16 variants.
FIRST_N, FIRST_D = 300, 64
FIRST_INJECT = ("nan_weight", "nan_grad_row", "nan_unused")


@functools.lru_cache(maxsize=None)
def first_graph():
    """300 nodes, 1200 edges; nodes 290 .. 299 are the source of no edge (their feature is read by nothing)"""
    gen = torch.Generator().manual_seed(31)
    src = torch.randint(0, 290, (1200,), generator=gen)
    dst = torch.randint(0, FIRST_N, (1200,), generator=gen)
    w = torch.rand(1200, generator=gen) * 80 + 1
    return torch.stack([src, dst]), w


@functools.lru_cache(maxsize=None)
def first_case(h, m, inject):
    """inputs and float64 results of hh = conv_in(embedding(x)) (with dL/d{w, b, W_in, b_in} for the upstream gradient g_h) and
    of y = linear(ELU(hh), W_out, b_out) (with all six gradients for g_y); A_hat from the oracle's gcn_norm in float64"""
    from oracle import gcn_oracle as go
    ei, w = first_graph()
    w = w.clone()
    n, d = FIRST_N, FIRST_D
    gen = torch.Generator().manual_seed(7 * h + m)
    x = torch.randn(n, 1, generator=gen)
    params = [torch.randn(*sh, generator=gen) * 0.3 for sh in ((d, 1), (d,), (h, d), (h,), (m, h), (m,))]
    g_h, g_y = torch.randn(n, h, generator=gen), torch.randn(n, m, generator=gen)
    zeroed = None
    if inject == "nan_weight":
        w[17] = NAN                                  # one entry of the in-degree, hence some entries of r and s
    elif inject == "nan_grad_row":
        g_h[33], g_y[33] = NAN, NAN
    else:
        zeroed = x.clone()
        zeroed[295] = 0.0
        x[295] = NAN
    nrm = go.gcn_norm(ei, w.double(), n, dtype=torch.float64)
    r = go.propagate_add(x.double(), ei, nrm)[:, 0]
    s_ = go.propagate_add(torch.ones(n, 1, dtype=torch.float64), ei, nrm)[:, 0]
    out = {}
    for form, g in (("rows", g_h), ("linear", g_y)):
        pd = [t.double().requires_grad_(True) for t in params]
        hh = r[:, None] * (pd[2] @ pd[0]).T + s_[:, None] * (pd[2] @ pd[1])[None, :] + pd[3]
        y = hh if form == "rows" else F.elu(hh) @ pd[4].T + pd[5]
        y.backward(g.double())
        out[form] = (y.detach(), [t.grad for t in pd])
    return dict(ei=ei, w=w, x=x, zeroed=zeroed, params=params, g_h=g_h, g_y=g_y, r=r, s=s_, out=out)


FIRST_CASES = [(h, m, inj) for (h, m) in ((64, 128), (128, 64)) for inj in FIRST_INJECT]


@pytest.mark.parametrize("h,m,inject", FIRST_CASES)
def test_first_layer_references_are_informative(h, m, inject):
    c = first_case(h, m, inject)
    ei = c["ei"]
    assert not (ei[0] >= 290).any()
    (hh, gh), (y, gy) = c["out"]["rows"], c["out"]["linear"]
    if inject == "nan_weight":
        assert informative(c["r"]) and informative(c["s"]) and informative(hh) and informative(y)
        # [r s 1]^T g: the sums weighted by r and s are non-finite, the plain column sum (dL/db_in of the rows form) is not
        assert all(not torch.isfinite(t).all() for t in gh[:3]) and torch.isfinite(gh[3]).all()
        assert all(not torch.isfinite(t).all() for t in gy[:5]) and torch.isfinite(gy[5]).all()        # (dL/db_out = 1^T g)
    elif inject == "nan_grad_row":
        assert informative(hh, expect_nonfinite=False) and informative(y, expect_nonfinite=False)
        assert all(not torch.isfinite(t).all() for t in gh[:4]) and all(not torch.isfinite(t).all() for t in gy)
    else:
        assert informative(hh, expect_nonfinite=False) and informative(y, expect_nonfinite=False)
        assert all(torch.isfinite(t).all() for t in gh[:4]) and all(torch.isfinite(t).all() for t in gy)


def _first_run(c, form, x, out_dtype=None):
    from pangnn_amd import functional as PF
    from pangnn_amd.graph import EdgeStructure
    st = EdgeStructure(c["ei"].to(_dev()), FIRST_N)
    norm = st.gcn_norm(c["w"].to(_dev()))
    ps = [t.clone().to(_dev()).requires_grad_(True) for t in c["params"]]
    xd = x.clone().to(_dev())
    if form == "rows":
        y = PF.embed_conv_in(xd, ps[0], ps[1], ps[2], ps[3], st, norm, out_dtype=out_dtype)
        y.backward(c["g_h"].to(_dev()).to(y.dtype))
    else:
        y = PF.embed_conv_in_linear(xd, ps[0], ps[1], ps[2], ps[3], ps[4], ps[5], st, norm)
        y.backward(c["g_y"].to(_dev()))
    torch.cuda.synchronize()
    return y.detach(), [t.grad for t in ps]


@pytest.mark.gpu
@pytest.mark.parametrize("form,table", [("rows", "f32"), ("rows", "bf16"), ("rows", "f16"), ("linear", "f32")])
@pytest.mark.parametrize("h,m,inject", FIRST_CASES)
def test_first_layer_by_linearity_passes_nonfinite_values_like_torch(h, m, inject, form, table):
    """bounds: test_first_layer_generated_inside_the_next_dense_layer's (forward atol 2e-5 / rtol 1e-5, gradients 2e-5 of the
    tensor's size / rtol 1e-4); rows stored as bf16 / f16: one rounding of that type on top, and the upstream gradient rows are
    then read in that type too (the reference takes the rounded rows)"""
    c = first_case(h, m, inject)
    y64, g64 = c["out"][form]
    if form == "rows" and table != "f32":                         # the reference of the 2-byte run: gradient rows as stored
        gq = c["g_h"].to(TABLES[table]).double()
        pd = [t.double().requires_grad_(True) for t in c["params"]]
        hh = c["r"][:, None] * (pd[2] @ pd[0]).T + c["s"][:, None] * (pd[2] @ pd[1])[None, :] + pd[3]
        hh.backward(gq)
        g64 = [t.grad for t in pd]
    y, grads = _first_run(c, form, c["x"], TABLES[table] if table != "f32" else None)
    tag = f"{form} H={h} M={m} {inject} {table}"
    store = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}[table]
    assert_same_nonfinite(y, as_stored(y64, table), finite_bound=allclose_bound(2e-5, 1e-5 + store), what=tag + " rows")
    for k in range(4 if form == "rows" else 6):
        def bound(got, ref):
            return bool(((got - ref).abs() <= 2e-5 * (float(ref.abs().max()) + 1e-30) + 1e-4 * ref.abs()).all())
        assert_same_nonfinite_tensorwise(grads[k], g64[k], finite_bound=bound, what=f"{tag} gradient {k}")
    if inject == "nan_unused":                                    # rule 3: the feature of a node that is the source of no edge
        y0, grads0 = _first_run(c, form, c["zeroed"], TABLES[table] if table != "f32" else None)
        assert torch.equal(y, y0) and all(torch.equal(a, b) for a, b in zip(grads[: 4 if form == "rows" else 6],
                                                                             grads0[: 4 if form == "rows" else 6]))


RANK2_CASES = [(f, bf16, inj) for f in (64, 128) for bf16 in (False, True) for inj in ("nan_r", "nan_grad_row")]


@functools.lru_cache(maxsize=None)
def rank2_case(f, bf16, inject):
    n = 1000
    gen = torch.Generator().manual_seed(f + n)
    r, s_ = torch.randn(n, generator=gen), torch.rand(n, generator=gen) + 0.5
    a, cc, b = torch.randn(f, generator=gen), torch.randn(f, generator=gen), torch.randn(f, generator=gen)
    g = torch.randn(n, f, generator=gen)
    g = g.to(torch.bfloat16) if bf16 else g
    if inject == "nan_r":
        r[123] = NAN
    else:
        g[777] = NAN
    ref = r.double()[:, None] * a.double() + s_.double()[:, None] * cc.double() + b.double()
    g64 = g.double()
    ref3 = torch.stack([(r.double()[:, None] * g64).sum(0), (s_.double()[:, None] * g64).sum(0), g64.sum(0)])
    return r, s_, a, cc, b, g, ref, ref3


@pytest.mark.parametrize("f,bf16,inject", RANK2_CASES)
def test_rank2_references_are_informative(f, bf16, inject):
    r, s_, a, cc, b, g, ref, ref3 = rank2_case(f, bf16, inject)
    if inject == "nan_r":
        assert informative(ref) and not torch.isfinite(ref3[0]).any() and torch.isfinite(ref3[1:]).all()
    else:
        assert informative(ref, expect_nonfinite=False) and not torch.isfinite(ref3).any()


@pytest.mark.gpu
@pytest.mark.parametrize("f,bf16,inject", RANK2_CASES)
def test_rank2_rows_and_weighted_colsum3_pass_nonfinite_values(f, bf16, inject):
    """the two kernels through the C ABI as test_rank2_rows_and_weighted_colsum3_kernels calls them, with its bounds: a NaN entry
    of r marks its row of the output and the r-weighted column sums only; a NaN gradient row marks all three sums"""
    from pangnn_amd import _lib
    lib = _lib.load()
    r, s_, a, cc, b, g, ref, ref3 = rank2_case(f, bf16, inject)
    n = r.shape[0]
    rd, sd, ad, cd, bd, gd = (t.to(_dev()) for t in (r, s_, a, cc, b, g))
    out = torch.zeros(n, f, dtype=torch.bfloat16 if bf16 else torch.float32, device=_dev())
    sums = torch.zeros(3, f, device=_dev())
    with torch.cuda.device(_dev()):
        _lib.check(lib.pangnn_rank2_rows(rd.data_ptr(), sd.data_ptr(), ad.data_ptr(), cd.data_ptr(), bd.data_ptr(),
                                         out.data_ptr(), int(bf16), f, n, f, _lib.stream_ptr()), "rank2_rows")
        nb = lib.pangnn_weighted_colsum3_workspace_bytes(f)
        ws = torch.empty(nb, dtype=torch.uint8, device=_dev())
        _lib.check(lib.pangnn_weighted_colsum3(gd.data_ptr(), int(bf16), gd.stride(0), rd.data_ptr(), sd.data_ptr(), n, f,
                                               sums.data_ptr(), ws.data_ptr(), nb, _lib.stream_ptr()), "colsum3")
    torch.cuda.synchronize()
    assert_same_nonfinite(out, ref, finite_bound=allclose_bound(4e-2 if bf16 else 1e-5, 8e-3 if bf16 else 1e-6),
                          what=f"rank2_rows F={f} bf16={bf16} {inject}")
    fin = ref3[torch.isfinite(ref3)]
    scale = (float(fin.abs().max()) if fin.numel() else 0.0) + 1e-12
    assert_same_nonfinite(sums, ref3, finite_bound=allclose_bound(1e-5 * scale + 1e-7, 1e-4),
                          what=f"weighted_colsum3 F={f} bf16={bf16} {inject}")
