"""The halo sums of the partitioned path (pangnn_amd/dist.py) against float64 references, on real process groups.

test_dist_gpu.py compares the partitioned model with the single-GPU one at bounds that must absorb two different storage
layouts (8e-2 of a gradient's scale under float16).  Here each halo route is pinned by itself:

  * the overlapped training decoder (dist._OverlappedDecoderLoss): loss, logits, the weight gradients and every dL/d(P | Q)
    row against the re-associated decoder in float64 over the whole graph, on the same rounded P | Q rows — at the real
    edge count and at config 4's (E = 74 694 783), with an upstream gradient of 1 and of a GradScaler's 65 536.  The row
    gradient is split into the part from sources read in place and the part that returned through the halo exchange, and
    the rows that own a halo copy are checked apart from the others;
  * a float16 GradScaler step, overlapped decoder against the HaloGather route;
  * the positional-neighbour band with its boundary rows (dist._BandTinyHalo) for k = 1, 2, 3, 8 against A_hat x + b in
    float64, for reproducibility, and against the generic propagate.

Back ends as in test_dist_gpu.py: one rank over RCCL that exchanges the outer quarters of its node range with itself
(PANGNN_FORCE_EXCHANGE=1), and gloo ranks sharing the one GPU (host-staged collectives).  Each back end is ONE spawn that
runs all of its cases; a worker collects every failed check into a report, so that one run names all of them."""
import json
import os
import sys
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT

pytestmark = pytest.mark.gpu

E_CFG4 = 74_694_783               # config 4's similarity edge count: the loss denominator of a full-size run
SCALE0 = 65536.0                  # torch.amp.GradScaler's initial scale


# ----------------------------------------------------------------------------------------------------------- set-up
def _init(rank, world, init_file, backend):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if backend == "nccl":
        assert world == 1
        os.environ["PANGNN_FORCE_EXCHANGE"] = "1"
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("nccl", init_method=f"file://{init_file}", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    return dev


def _cfg2_graph(dev):
    """cfg2_sim_1000x5 in canonical (src, dst) order (source-sorted: the overlapped decoder's precondition)"""
    from conftest import copy_graph, whole_graph_from_golden
    g = whole_graph_from_golden("cfg2_sim_1000x5")
    o = torch.argsort(g.edge_index[0] * g.x.shape[0] + g.edge_index[1])
    g.edge_index, g.edge_attr, g.y = g.edge_index[:, o].contiguous(), g.edge_attr[o].contiguous(), g.y[o].contiguous()
    return g, copy_graph(g, dev)


class _Report:
    """every check of a worker: failures are collected (not raised) so that one run lists all of them"""

    def __init__(self, rank):
        self.rank, self.fail, self.info = rank, [], []

    def check(self, case, what, err, bound):
        """err, bound: tensors of the same shape (per element) or floats"""
        err, bound = torch.as_tensor(err, dtype=torch.float64), torch.as_tensor(bound, dtype=torch.float64)
        if err.numel() == 0:
            return
        ratio = float((err / bound).max())
        line = f"rank {self.rank} {case} {what}: max err {float(err.max()):.3e}, max err / bound {ratio:.3g}"
        self.info.append(line)
        if not ratio <= 1.0:                         # NaN fails too
            self.fail.append(line)

    def write(self, out_dir):
        with open(os.path.join(out_dir, f"report{self.rank}.json"), "w") as f:
            json.dump({"fail": self.fail, "info": self.info}, f)


def _spawn(worker, world, *args):
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(worker, args=(world, os.path.join(d, "rdzv"), d) + args, nprocs=world, join=True)
        fail = []
        for r in range(world):
            with open(os.path.join(d, f"report{r}.json")) as f:
                rep = json.load(f)
            print("\n".join(rep["info"]))
            fail += rep["fail"]
        assert not fail, "\n".join(fail)


# ------------------------------------------------------------- A1: overlapped decoder gradients against float64
def _via_halo(ei, n_local, forced):
    """per edge of the whole graph: is its source read from a halo COPY by the rank that owns its target (HaloPlan: the
    rows outside [lo, hi) of the owner, and under the forced self-exchange the outer quarters of the one range)"""
    lo_t = torch.div(ei[1], n_local, rounding_mode="floor") * n_local
    q = n_local // 4 if forced else 0
    return (ei[0] < lo_t + q) | (ei[0] >= lo_t + n_local - q)


def _clear_of_the_relu_kinks(pq, ei, extra, w):
    """b2, moved by at most 2e-4 per unit where needed, such that no second-layer pre-activation h2[e, j] of the graph lies
    within 2^-18 of its magnitude sum_k |W2[j, k]| relu(h1[e, k]) + |b2[j]| of zero — the worst-case error of a 64-term fp32
    dot product.  Closer to the kink, the kernel's relu mask may rightly differ from the float64 one, and one flipped
    (edge, unit) moves dL/db2[j], a row of dL/dW2 and the edge's dL/dP, dL/dQ rows by g_e w3[j]: far outside the bounds of
    this test, for a reason that says nothing about the halo sums (about one such pair is expected in 2.9 M values).
    The first layer needs no such care: the kernel's h1 is fl(P + Q), whose sign is that of P + Q, or fma(extra, cvec,
    fl(P + Q)), whose sign only the inner rounding (<= 2^-24 |P + Q|) can move — asserted not to happen for these rows."""
    d = pq.shape[1] // 2
    src, dst = ei
    h1 = pq[src, :d].double() + pq[dst, d:].double()
    if extra is not None:
        pq_sum = h1
        h1 = h1 + extra.double().unsqueeze(1) * w["cvec"].detach().double()
        assert not bool(((h1.abs() <= 2.0 ** -23 * pq_sum.abs()) & (h1 != 0)).any()), "an h1 lies on the relu kink"
    a1 = torch.relu(h1)
    w2 = w["w2"].detach().double()
    z, mag2 = a1 @ w2.t(), a1 @ w2.abs().t()
    b2 = w["b2"].detach().float()
    out = torch.full_like(b2, float("nan"))
    for t in [0.0] + [v for i in range(1, 21) for v in (i * 1e-5, -i * 1e-5)]:
        cand = (b2.double() + t).float()                      # an fp32 value: what the kernel reads
        cd = cand.double()
        ok = ((z + cd).abs() > 2.0 ** -18 * (mag2 + cd.abs())).all(dim=0) & torch.isnan(out)
        out = torch.where(ok, cand, out)
    assert not bool(torch.isnan(out).any()), "no b2 clear of the relu kinks"
    return out


def _decoder_ref64(pq, ei, via, extra, w, y, pw, denom, s, owned):
    """the re-associated decoder in float64: relu(relu(P[src] + Q[dst] (+ extra cvec)) W2^T + b2) w3 + b3, BCE(pos_weight)
    summed / denom, times the upstream gradient s.  P is read through two leaves of the same values, one for the edges whose
    source is read in place and one for the edges that read a halo copy, so that the row gradient comes out in those two
    parts.  Returns (own edges' logits, own edges' loss, {weight: grad of the own edges' loss}, dL/dP own part, dL/dP halo
    part, dL/dQ), the row gradients of the whole graph's loss."""
    d = pq.shape[1] // 2
    p_own = pq[:, :d].double().requires_grad_(True)
    p_halo = pq[:, :d].double().requires_grad_(True)
    q = pq[:, d:].double().requires_grad_(True)
    wd = {k: v.detach().double().requires_grad_(True) for k, v in w.items() if v is not None}
    src, dst = ei
    h1 = torch.where(via.unsqueeze(1), p_halo[src], p_own[src]) + q[dst]
    if extra is not None:
        h1 = h1 + extra.double().unsqueeze(1) * wd["cvec"]
    logit = torch.relu(torch.relu(h1) @ wd["w2"].t() + wd["b2"]) @ wd["w3"] + wd["b3"]
    per_edge = torch.nn.functional.binary_cross_entropy_with_logits(logit, y.double(), pos_weight=pw.double(),
                                                                    reduction="none")
    loss_own = per_edge[owned].sum() / denom
    names = list(wd)
    g_w = torch.autograd.grad(loss_own * s, [wd[k] for k in names], retain_graph=True)
    (per_edge.sum() / denom * s).backward()
    return logit[owned].detach(), loss_own.detach(), dict(zip(names, g_w)), p_own.grad, p_halo.grad, q.grad


def _a1(rank, world, dev, forced, rep):
    from pangnn_amd import dist as pdist
    g, gd = _cfg2_graph(dev)
    shard = pdist.partition_graph(gd, rank, world)
    lo, hi, nl = shard.lo, shard.hi, shard.n_local
    n = g.x.shape[0]
    ei = gd.edge_index
    via = _via_halo(ei, nl, forced)
    halo_owner = torch.zeros(n, dtype=torch.bool, device=dev)
    halo_owner[ei[0][via]] = True                                 # rows that some rank reads through a halo copy
    halo_owner = halo_owner[lo:hi]
    owned = shard.owned_mask
    pw = torch.tensor(float((g.y == 0).sum() / g.y.sum()), device=dev)
    e_real = int(g.edge_index.shape[1])
    for skip in (False, True):
        torch.manual_seed(0)                                      # the same parameters on every rank
        model = pdist.DistAlternateGCN(dev, dims=[64, 128], exchange="halo", part=shard, skip_connections=skip)
        assert model._overlap_ok(shard)
        plan = model._plan(shard, "sim")
        assert plan.any_exchange and plan.n_halo > 0
        st_loc, st_halo = model._st_split(shard)
        w = {"w2": model.mlp[2].weight, "b2": model.mlp[2].bias, "w3": model.mlp[4].weight.view(-1),
             "b3": model.mlp[4].bias, "cvec": model.mlp[0].weight[:, 128] if skip else None}
        extra = shard.edge_attr if skip else None
        for dtype in (torch.float32, torch.bfloat16, torch.float16):
            # rows of the magnitude the model's P | Q have (|z| <= ~1 after ELU, Linear(129, 64) init), the same on
            # every rank: each rank takes its block, the reference reads all of them
            gen = torch.Generator().manual_seed(7)
            pq = (torch.randn(n, 128, generator=gen) * 0.5).to(dtype).to(dev)
            wc = dict(w, b2=_clear_of_the_relu_kinks(pq, ei, gd.edge_attr if skip else None, w))
            for denom_name, denom in (("E", e_real), ("E_cfg4", E_CFG4)):
                for s in (1.0, SCALE0):
                    case = f"A1 skip={int(skip)} {str(dtype)[6:]} denom={denom_name} s={s:g}"
                    leaf = torch.zeros(nl, 128, dtype=dtype, device=dev)
                    leaf[: hi - lo] = pq[lo:hi]
                    leaf.requires_grad_(True)
                    wl = {k: (v.detach().clone().requires_grad_(True) if v is not None else None) for k, v in wc.items()}
                    loss, logits = pdist._OverlappedDecoderLoss.apply(
                        leaf, None, model.ops, plan, st_loc, st_halo, extra, wl["cvec"], wl["w2"], wl["b2"], wl["w3"],
                        wl["b3"], shard.y, pw, denom)
                    loss.backward(torch.full((), s, device=dev))
                    r_logit, r_loss, r_gw, r_po, r_ph, r_q = _decoder_ref64(pq, ei, via, gd.edge_attr if skip else None,
                                                                            wc, gd.y, pw, denom, s, owned)
                    rep.check(case, "logits", (logits.double() - r_logit).abs(), 1.6e-5)
                    rep.check(case, "loss (relative)", abs(float(loss) - float(r_loss)) / abs(float(r_loss)), 1e-6)
                    for k, ref in r_gw.items():
                        rep.check(case, f"d/d{k}", (wl[k].grad.double() - ref).abs(), 1e-6 * float(ref.abs().max()))
                    ref = torch.cat([(r_po + r_ph)[lo:hi], r_q[lo:hi]], dim=1)
                    halo_part = torch.cat([r_ph[lo:hi], torch.zeros_like(r_q[lo:hi])], dim=1)
                    bound = torch.full_like(ref, 1e-6 * float(ref.abs().max()))     # fp32: the decoder's own error
                    if dtype == torch.float16:
                        # one float16 rounding of the result, half the subnormal spacing where the result is subnormal
                        bound += 2.0 ** -11 * ref.abs() + 2.0 ** -25
                    elif dtype == torch.bfloat16:
                        # the result's bf16 rounding and the halo part's on the 16-bit wire
                        bound += 2.0 ** -8 * ref.abs() + 2.0 ** -8 * halo_part.abs()
                    err = (leaf.grad[: hi - lo].double() - ref).abs()
                    rep.check(case, "dL/dP of the halo-owner rows", err[halo_owner, :64], bound[halo_owner, :64])
                    rep.check(case, "dL/dP of the other rows", err[~halo_owner, :64], bound[~halo_owner, :64])
                    rep.check(case, "dL/dQ", err[:, 64:], bound[:, 64:])


# ---------------------------------------------------- A2: a float16 GradScaler step, overlapped against HaloGather
def _a2(rank, world, dev, rep):
    from pangnn_amd import dist as pdist
    g, gd = _cfg2_graph(dev)
    shard = pdist.partition_graph(gd, rank, world)
    shard.e_sim_total = E_CFG4                   # the loss denominator both decoder routes read
    pw = torch.tensor(float((g.y == 0).sum() / g.y.sum()), device=dev)
    torch.manual_seed(0)
    model = pdist.DistAlternateGCN(dev, dims=[64, 128], exchange="halo", part=shard)
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    grads = {}
    for overlap in (True, False):
        model.load_state_dict(init)
        model.overlap = overlap
        assert model._overlap_ok(shard) == overlap
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        scaler = torch.amp.GradScaler("cuda", init_scale=SCALE0)
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            loss, _ = model.loss_and_logits(shard, shard.y, pw)
        scaler.scale(loss).backward()
        model.sync_gradients()
        scaler.unscale_(opt)
        grads[overlap] = {k: p.grad.detach().double().clone() for k, p in model.named_parameters() if p.grad is not None}
        for k, t in grads[overlap].items():
            rep.check(f"A2 overlap={int(overlap)}", f"d/d{k} finite", 0.0 if bool(torch.isfinite(t).all()) else 1.0, 0.5)
        scaler.step(opt)
        scaler.update()
        rep.check(f"A2 overlap={int(overlap)}", "scale kept", 0.0 if scaler.get_scale() >= SCALE0 else 1.0, 0.5)
    assert grads[True].keys() == grads[False].keys()
    for k, ref in grads[False].items():
        # Both routes store the same float16 P | Q rows; their scaled dL/d(P | Q) rows are rounded to float16 once (overlapped:
        # the fp32 sum of the own and the returned part, cast for the P | Q Linear) or twice (HaloGather: the table's rows,
        # then the own rows after the halo sum), i.e. they differ by up to 2^-10 of each row element — what every parameter
        # gradient inherits through the first decoder layer and the encoder behind it: 1e-3 of the gradient's scale
        scale = float(ref.abs().max()) + 1e-30
        rep.check("A2", f"d/d{k} overlapped vs HaloGather", (grads[True][k] - ref).abs(), 1e-3 * scale)


# ------------------------------------------------------------- A3: the band propagate with its boundary rows
def _band_ref64(nb_ei, n, x, gup, b, lo, hi):
    """A_hat x + b over the whole positional-neighbour graph in float64 (unit weights, GCN norm, no added self loops), the
    transposed product of the upstream gradient, and the sums of magnitudes that bound an fp32 evaluation of each"""
    src, dst = nb_ei
    deg = torch.bincount(dst, minlength=n).double()
    dis = deg.pow(-0.5)
    dis[deg == 0] = 0.0
    a = (dis[src] * dis[dst]).unsqueeze(1)
    x, gup = x.double(), gup.double()
    out = torch.zeros(n, x.shape[1], dtype=torch.float64).index_add_(0, dst, a * x[src])
    s_out = torch.zeros_like(out).index_add_(0, dst, a.abs() * x[src].abs())
    gx = torch.zeros_like(out).index_add_(0, src, a * gup[dst])
    s_gx = torch.zeros_like(out).index_add_(0, src, a.abs() * gup[dst].abs())
    if b is not None:
        out = out + b.double()
    gb = gup[lo:hi].sum(0)
    s_gb = gup[lo:hi].abs().sum(0)
    return out[lo:hi], s_out[lo:hi], gx[lo:hi], s_gx[lo:hi], gb, s_gb


def _a3(rank, world, dev, rep):
    from conftest import copy_graph
    from pangnn_amd import dist as pdist
    from pangnn_amd import simulate
    eps = 2.0 ** -23
    for k in (1, 2, 3, 8):
        g = simulate.simulate_graph(30, 4, 0.5, neighbours=k, seed=k)        # 120 nodes: 60 / 40 per rank
        n = int(g.x.shape[0])
        assert n % world == 0
        gd = copy_graph(g, dev)
        for f in (64, 128):
            for with_bias in (False, True):
                case = f"A3 world={world} k={k} F={f} bias={int(with_bias)}"
                gen = torch.Generator().manual_seed(100 * k + f)
                x_full, g_full, b = torch.randn(n, f, generator=gen), torch.randn(n, f, generator=gen), torch.randn(f, generator=gen)
                runs = {}
                for band in (True, False):
                    os.environ["PANGNN_DIST_BAND"] = "1" if band else "0"
                    shard = pdist.partition_graph(gd, rank, world)
                    lo, hi = shard.lo, shard.hi
                    assert shard.n_local > 16 and hi - lo == shard.n_local
                    model = pdist.DistAlternateGCN(dev, dims=[64, 128], exchange="halo", part=shard)
                    res = []
                    for _ in range(3 if band else 1):
                        x = x_full[lo:hi].to(dev).requires_grad_(True)
                        bias = b.to(dev).requires_grad_(True) if with_bias else None
                        out = model._propagate_rows(x, bias, shard, "nb", None, "1", "nb")
                        out.backward(g_full[lo:hi].to(dev))
                        res.append((out.detach(), x.grad, bias.grad if with_bias else None))
                    taken = shard._dist_band["nb"] is not None
                    assert taken == band, (case, band, taken)
                    runs[band] = res
                os.environ.pop("PANGNN_DIST_BAND")
                r_out, s_out, r_gx, s_gx, r_gb, s_gb = _band_ref64(g.neighbour_edge_index, n, x_full, g_full,
                                                                   b if with_bias else None, lo, hi)
                # a sum of at most 2k + 1 products in fp32: (2k + 1) 2^-24 of the sum of magnitudes, doubled for the fp32
                # norms deg^-1/2[i] deg^-1/2[j]; the bias add is one more rounding
                b_out = (2 * k + 1) * eps * s_out + (eps * b.double().abs() if with_bias else 0.0) + 1e-30
                b_gx = (2 * k + 1) * eps * s_gx + 1e-30
                # the bias gradient is a column sum of the n_local own rows, in an order of the kernel's choosing
                b_gb = shard.n_local * eps / 2 * s_gb + 1e-30
                out, gx, gb = runs[True][0]
                rep.check(case, "A x + b", (out.cpu().double() - r_out).abs(), b_out)
                rep.check(case, "dL/dx", (gx.cpu().double() - r_gx).abs(), b_gx)
                if with_bias:
                    rep.check(case, "dL/db", (gb.cpu().double() - r_gb).abs(), b_gb)
                same = all(torch.equal(a, c) for rep_i in runs[True][1:] for a, c in zip(rep_i, runs[True][0])
                           if a is not None)
                rep.check(case, "3 calls bitwise equal", 0.0 if same else 1.0, 0.5)
                out2, gx2, gb2 = runs[False][0]
                rep.check(case, "band vs generic: A x + b", (out - out2).abs().cpu().double(), b_out)
                rep.check(case, "band vs generic: dL/dx", (gx - gx2).abs().cpu().double(), b_gx)
                if with_bias:
                    rep.check(case, "band vs generic: dL/db", (gb - gb2).abs().cpu().double(), b_gb)


# ----------------------------------------------------------------------------------------------- workers / tests
def _worker_rccl(rank, world, init_file, out_dir):
    dev = _init(rank, world, init_file, "nccl")
    rep = _Report(rank)
    _a1(rank, world, dev, True, rep)
    _a2(rank, world, dev, rep)
    rep.write(out_dir)
    dist.barrier()
    dist.destroy_process_group()


def _worker_gloo(rank, world, init_file, out_dir, parts):
    dev = _init(rank, world, init_file, "gloo")
    rep = _Report(rank)
    if "a1" in parts:
        _a1(rank, world, dev, False, rep)
    if "a2" in parts:
        _a2(rank, world, dev, rep)
    if "a3" in parts:
        _a3(rank, world, dev, rep)
    rep.write(out_dir)
    dist.barrier()
    dist.destroy_process_group()


def test_halo_sums_over_rccl_with_forced_self_exchange():
    """A1 and A2 on one rank over RCCL: the outer quarters of the node range are halo rows that the rank sends itself"""
    _spawn(_worker_rccl, 1)


@pytest.mark.parametrize("world,parts", [(2, ("a1", "a2", "a3")), (3, ("a3",))], ids=["gloo-2", "gloo-3"])
def test_halo_sums_over_gloo_ranks_on_one_gpu(world, parts):
    """A1 and A2 over two gloo ranks, A3 over two and three (host-staged collectives, HIP kernels on every rank)"""
    _spawn(_worker_gloo, world, parts)
