"""pangnn_amd.weights — the Q-score edge weights as a differentiable function of the bit scores and the softmax temperature
(csrc/qscore.hip: pangnn_qscore_fwd / pangnn_qscore_bwd).  The CPU leg (plain torch under autograd, the formula of
construct.normalize_sim_scores' CPU leg over the segment plan) is the definition: it is checked against the construction's
fixtures and by gradcheck, and the device kernels are checked against it.

Bounds.  Forward, float64: the bound test_construct.py derives for the device kernel — exp / log of the GPU math library are
a few ulp from libm, amplified by p / (1 - p) <= 1e8 (the clip at epsilon): 5e-7.  Backward: the same factor sits in
1 / c_i, so per segment |d(dL/dscore_i)| <= 5e-7 max_j |dL/dscore_j|, and |d(dL/dt)| <= 5e-7 sum_i |gx_i score_i| / t^2.
Every test prints the figure it measured before it asserts."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from pangnn_amd import construct, simulate
from pangnn_amd.weights import QScoreWeights, qscore_weights, score_segments

FIXTURES = ["sim_200x4", "cfg1_2genomes", "cfg2_sim_1000x5", "cfg3_5genomes"]
DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
REL = 5e-7


def T(f, k, device="cpu"):
    return torch.from_numpy(f[k]).to(device)


def N(t):
    return t.detach().cpu().numpy()


def assert_weights(got, want, device):
    """test_construct.assert_weights: fp32 edge weights identical on the CPU; within 1 ulp on <= 0.1 % of the entries on the
    device"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    if device == "cpu":
        assert np.array_equal(got, want)
        return
    bad = got != want
    if bad.any():
        ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1 and bad.mean() <= 1e-3, (int(ulp.max()), float(bad.mean()))


def fixture_graph(name, device):
    f = load_golden(name)
    g = construct.build_from_raw(int(f["num_nodes"]), T(f, "raw_src", device), T(f, "raw_dst", device),
                                 T(f, "raw_score", device), T(f, "genome_of", device).long(),
                                 pair_src=T(f, "grp_src", device), pair_dst=T(f, "grp_dst", device), keep_raw=True)
    return f, g


# ---------------------------------------------------------------- 1. forward equals the construction
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("name", FIXTURES)
def test_forward_equals_the_construction(name, device):
    f, g = fixture_graph(name, device)
    assert g.raw_score.shape == g.edge_attr.shape and g.raw_score.dtype == T(f, "raw_score").dtype
    module = QScoreWeights(t=0.8).to(device)
    w = module(g)
    assert w.dtype == torch.float32 and w.device.type == device and w.requires_grad
    o = np.lexsort((f["whole_edge_index"][1], f["whole_edge_index"][0]))
    assert np.array_equal(N(g.edge_index), f["whole_edge_index"][:, o])
    assert_weights(N(w), f["whole_edge_attr"][o], device)
    assert score_segments(g.edge_index, g.genome_of, holder=g) is score_segments(g.edge_index, g.genome_of, holder=g)
    if device == "cpu":
        return
    # float64 weights against the construction's own device kernel on the same device tensors, matched by (src, dst): the
    # math and the summation order are the same, so any difference is a bug in the plan or the gather
    s, d, wn = construct.normalize_sim_scores(T(f, "flt_src", device), T(f, "flt_dst", device), T(f, "flt_score", device),
                                              T(f, "genome_of", device).long())
    o = torch.argsort(s * int(f["num_nodes"]) + d, stable=True)
    assert torch.equal(torch.stack([s[o], d[o]]), g.edge_index)
    w64 = qscore_weights(g.raw_score, score_segments(g.edge_index, g.genome_of, holder=g), 0.8, out_dtype=torch.float64)
    assert w64.dtype == torch.float64 and torch.equal(w64, wn[o])


# ---------------------------------------------------------------- the hand-built relation of checks 2-5
SEG_LENGTHS = (1, 2, 3, 63, 64, 65, 130, 200)


def hand_relation(score_dtype=torch.float64):
    """source gene k (genome 0) with SEG_LENGTHS[k] candidates in genome 1, integer scores in [10, 900], the edge order
    shuffled so that the plan's `item` is not the identity: (edge_index, genome_of, score), CPU tensors"""
    gen = torch.Generator().manual_seed(11)
    n_src, n_cand = len(SEG_LENGTHS), max(SEG_LENGTHS)
    src = torch.cat([torch.full((n,), k, dtype=torch.int64) for k, n in enumerate(SEG_LENGTHS)])
    dst = torch.cat([n_src + torch.randperm(n_cand, generator=gen)[:n] for n in SEG_LENGTHS])
    perm = torch.randperm(src.numel(), generator=gen)
    edge_index = torch.stack([src[perm], dst[perm]])
    genome_of = torch.cat([torch.zeros(n_src, dtype=torch.int64), torch.ones(n_cand, dtype=torch.int64)])
    score = torch.randint(10, 901, (src.numel(),), generator=gen).to(score_dtype)
    return edge_index, genome_of, score


def run(device, edge_index, genome_of, score, t, upstream, out_dtype=torch.float64):
    """(weights, dL/dscore, dL/dt, plan) of one forward + backward on `device`, t a float64 leaf"""
    ei, go = edge_index.to(device), genome_of.to(device)
    seg = score_segments(ei, go)
    sc = score.to(device).clone().requires_grad_()
    tt = torch.tensor(float(t), dtype=torch.float64, device=device, requires_grad=True)
    w = qscore_weights(sc, seg, tt, out_dtype=out_dtype)
    w.backward(upstream.to(device))
    return w.detach(), sc.grad, tt.grad, seg


def assert_backward(seg_cpu, score, t, gs_ref, gt_ref, gs, gt, what):
    """check 3's bounds, `gs_ref` / `gt_ref` from the CPU float64 leg"""
    gs, gt = gs.detach().cpu().to(torch.float64), float(gt)
    gs_ref = gs_ref.to(torch.float64)
    inv = seg_cpu.segment_of_edge
    seg_max = torch.zeros(seg_cpu.num_segments, dtype=torch.float64).scatter_reduce(0, inv, gs_ref.abs(), reduce="amax")
    err = (gs - gs_ref).abs()
    finite = torch.isfinite(gs_ref)
    ratio = (err[finite] / seg_max[inv][finite].clamp_min(1e-300)).max().item() if bool(finite.any()) else 0.0
    bound_t = REL * float((gs_ref[finite] * score.to(torch.float64)[finite]).abs().sum()) / t     # gx_i = t dL/dscore_i
    print(f"{what}: max |d dL/dscore| / segment max = {ratio:.3e} (bound {REL:.0e}); |d dL/dt| = "
          f"{abs(gt - float(gt_ref)):.3e} (bound {bound_t:.3e}, dL/dt = {float(gt_ref):.6e})")
    assert bool((err[finite] <= REL * seg_max[inv][finite]).all()), ratio
    zero = gs_ref == 0
    assert bool((gs[zero] == 0).all())                       # clipped-everywhere and single-candidate segments: exact zeros
    if math.isfinite(float(gt_ref)):
        assert abs(gt - float(gt_ref)) <= bound_t


# ---------------------------------------------------------------- 2. + 3. segment lengths, backward against CPU float64
@pytest.mark.gpu
@pytest.mark.parametrize("score_dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("t", [0.8, 50.0])
def test_segment_lengths_forward_and_backward(t, score_dtype):
    edge_index, genome_of, score = hand_relation(score_dtype)
    up = torch.randn(score.numel(), dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    w_ref, gs_ref, gt_ref, seg_cpu = run("cpu", edge_index, genome_of, score, t, up)
    assert not torch.equal(seg_cpu.item.long(), torch.arange(score.numel()))
    assert sorted(seg_cpu.counts.tolist()) == sorted(SEG_LENGTHS)
    unclipped = float(((w_ref - 1.0 > 1e-7) & (w_ref - 1.0 < 79.999)).double().mean())      # (q in (4.3e-8, 80) unclipped)
    print(f"t = {t}: unclipped share {unclipped:.3f}")
    w, gs, gt, seg = run("cuda", edge_index, genome_of, score, t, up)
    assert gs.dtype == score_dtype and gt.dtype == torch.float64 and w.dtype == torch.float64
    assert torch.equal(seg.item.cpu(), seg_cpu.item) and torch.equal(seg.rowptr.cpu(), seg_cpu.rowptr)
    print(f"forward: max |dw| = {(w.cpu() - w_ref).abs().max().item():.3e}")
    assert np.allclose(N(w), N(w_ref), rtol=REL, atol=REL)
    assert_backward(seg_cpu, score, t, gs_ref, gt_ref, gs, gt, f"hand-built t={t} {score_dtype}")
    # float32 weights and float32 upstream gradients: the other storage types of the two entry points
    w32, gs32, gt32, _ = run("cuda", edge_index, genome_of, score, t, up.float(), out_dtype=torch.float32)
    assert_weights(N(w32), N(w_ref.float()), "cuda")
    _, gs_ref32, gt_ref32, _ = run("cpu", edge_index, genome_of, score, t, up.float(), out_dtype=torch.float32)
    assert_backward(seg_cpu, score, t, gs_ref32, gt_ref32, gs32, gt32, f"hand-built t={t} {score_dtype} f32 upstream")


@pytest.mark.gpu
@pytest.mark.parametrize("t", [0.8, 50.0])
def test_backward_on_a_fixture(t):
    """The fixture is the case that needs the rounding residual of lse (csrc/qscore.hip, DESIGN.md 4b''): at t = 0.8 it has
    unclipped items with c = 2.5e-8 at lse = 701, where gx_i = p_i (a_i - S) without the residual is 8.2e-7 of the segment
    maximum from autograd (5.1e-7 in a second segment) — on the device and, digit for digit, in float64 on the CPU."""
    _, g = fixture_graph("sim_200x4", "cpu")
    up = torch.randn(g.raw_score.numel(), dtype=torch.float64, generator=torch.Generator().manual_seed(6))
    _, gs_ref, gt_ref, seg_cpu = run("cpu", g.edge_index, g.genome_of, g.raw_score, t, up)
    _, gs, gt, _ = run("cuda", g.edge_index, g.genome_of, g.raw_score, t, up)
    assert_backward(seg_cpu, g.raw_score, t, gs_ref, gt_ref, gs, gt, f"sim_200x4 t={t}")


# ---------------------------------------------------------------- 4. non-finite
@pytest.mark.gpu
def test_a_nan_score_stays_in_its_segment():
    edge_index, genome_of, score = hand_relation()
    up = torch.randn(score.numel(), dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    w0, gs0, gt0, seg = run("cuda", edge_index, genome_of, score, 50.0, up)
    k = int((seg.counts == 65).nonzero()[0])
    inv = seg.segment_of_edge.cpu()
    bad = score.clone()
    bad[int((inv == k).nonzero()[3])] = float("nan")
    w_ref, gs_ref, gt_ref, _ = run("cpu", edge_index, genome_of, bad, 50.0, up)
    w, gs, gt, _ = run("cuda", edge_index, genome_of, bad, 50.0, up)
    assert torch.equal(torch.isnan(w).cpu(), torch.isnan(w_ref))
    assert torch.equal(torch.isnan(gs).cpu(), torch.isnan(gs_ref)) and bool(torch.isnan(gs_ref[inv == k]).all())
    assert bool(torch.isnan(gt)) == bool(torch.isnan(gt_ref)) and bool(torch.isnan(gt))
    other = (inv != k).to(w.device)
    assert torch.equal(w[other], w0[other]) and torch.equal(gs[other], gs0[other])
    assert not bool(torch.isnan(gs[other]).any()) and bool(torch.isfinite(gt0))


# ---------------------------------------------------------------- 5. reproducibility, no host reads
@pytest.mark.gpu
def test_backward_is_reproducible_and_a_warm_call_reads_nothing_back():
    edge_index, genome_of, score = hand_relation(torch.float32)
    up = torch.randn(score.numel(), dtype=torch.float64, generator=torch.Generator().manual_seed(8))
    a, b = (run("cuda", edge_index, genome_of, score, 50.0, up) for _ in range(2))
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[0], b[0])
    g = simulate.simulate_graph(200, 4, 0.3, 10, 2, seed=0, device="cuda", keep_raw=True)
    module = QScoreWeights(t=0.8).to("cuda")
    upw = torch.randn(g.raw_score.numel(), device="cuda")
    module(g).backward(upw)                                            # cold: builds the plan
    first = module.log_t.grad.clone()
    module.log_t.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        module(g).backward(upw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(module.log_t.grad, first)


# ---------------------------------------------------------------- 6. gradcheck of the definition
def test_gradcheck_of_the_cpu_leg():
    gen = torch.Generator().manual_seed(3)
    src = torch.tensor([0] * 5 + [1] * 4 + [2] * 1 + [3] * 6 + [4] * 4)
    dst = torch.cat([5 + torch.randperm(8, generator=gen)[:n] for n in (5, 4, 1, 6, 4)])
    perm = torch.randperm(20, generator=gen)
    seg = score_segments(torch.stack([src[perm], dst[perm]]),
                         torch.cat([torch.zeros(5, dtype=torch.int64), torch.ones(4, dtype=torch.int64),
                                    torch.full((4,), 2, dtype=torch.int64)]))
    assert seg.num_edges == 20 and seg.num_segments > 5
    score = (10 + 90 * torch.rand(20, dtype=torch.float64, generator=gen)).requires_grad_()
    t = torch.tensor(20.0, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda s, tt: qscore_weights(s, seg, tt, out_dtype=torch.float64), (score, t))
    w = qscore_weights(score, seg, t, out_dtype=torch.float64).detach()
    single = seg.counts[seg.segment_of_edge] == 1
    assert bool(((w - 1.0 < 79.0) & (w - 1.0 > 1e-6) | single).all())            # nothing but a single candidate clips


# ---------------------------------------------------------------- 7. end to end
@pytest.mark.gpu
@pytest.mark.parametrize("skip", [False, True], ids=["default", "skip_connections"])
def test_temperature_gradient_through_the_model(skip):
    import pangnn_amd
    dev = torch.device("cuda")
    g = simulate.simulate_graph(200, 4, 0.3, 10, 2, seed=0, device=dev, keep_raw=True)
    torch.manual_seed(0)
    model = pangnn_amd.AlternateGCN(dev, None, False, skip_connections=skip)
    model.train()
    module = QScoreWeights().to(dev)
    w = module(g)
    w.retain_grad()
    loss, _ = model.loss_and_logits(module.apply_to(g, w), g.y, g.class_balance)
    loss.backward()
    gl = module.log_t.grad
    assert gl is not None and bool(torch.isfinite(gl)) and float(gl) != 0.0
    # the CPU float64 leg on the same upstream gradient
    ei, go, sc = g.edge_index.cpu(), g.genome_of.cpu(), g.raw_score.cpu().to(torch.float64)
    _, gs_ref, gt_ref, _ = run("cpu", ei, go, sc, 0.8, w.grad.cpu(), out_dtype=torch.float32)
    bound = REL * float((gs_ref * sc).abs().sum())             # t times check 3's bound on dL/dt (gx_i = t dL/dscore_i)
    print(f"log_t.grad = {float(gl):.9e}, t dL/dt (CPU) = {0.8 * float(gt_ref):.9e}, bound {bound:.3e}")
    assert abs(float(gl) - 0.8 * float(gt_ref)) <= bound
    # the producer changes nothing downstream: a leaf with the same values gives the same bits everywhere
    got = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    leaf = w.detach().requires_grad_()
    loss2, _ = model.loss_and_logits(module.apply_to(g, leaf), g.y, g.class_balance)
    loss2.backward()
    assert torch.equal(loss.detach(), loss2.detach()) and torch.equal(leaf.grad, w.grad)
    again = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    assert got.keys() == again.keys() and len(got) > 4
    for k in got:
        assert torch.equal(got[k], again[k]), k
