"""Training step of the default topology with the weightless decoders (`--decoder cosine` / `dotproduct`): the fused route
(csrc/edge_score.hip, `fused_decoder=True`) against today's literal gather-concat route (`fused_decoder=False`) at config 4's
workload, fp32, each configuration in a fresh child process; plus the fused cosine step under bf16 autocast at `cfg5slice`.
The literal route is NOT run at cfg5slice: its [E, 2D] fp32 gather alone is E * 128 * 4 bytes (printed, by arithmetic).

    python tools/time_score_decoder.py --out profiles/score_decoder.jsonl
    python tools/time_score_decoder.py --child cosine 1 cfg4 fp32          # one configuration (what the parent starts)

Per step: CUDA-event time of loss_and_logits + backward + Adam (median of --steps after --warmup), peak memory above the
pre-step level, and for the fused route the edge pass / node pass alone (events around the two entry points)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORK = {"cfg4": dict(args=(50000, 20, 0.2, 100, 20), kw={}),
        "cfg5slice": dict(args=(200000, 6, 0.1, 500, 50), kw=dict(mean_neg=220, adjacent_only=True))}


def child(decoder, fused, workload, prec, steps, warmup):
    import torch
    sys.path.insert(0, ROOT)
    import pangnn_amd
    from pangnn_amd import functional as PF
    from pangnn_amd import simulate
    from pangnn_amd.graph import structure_of
    from pangnn_amd.train import make_optimizer
    dev = torch.device("cuda")
    w = WORK[workload]
    g = simulate.simulate_graph(*w["args"], seed=0, device=dev, **w["kw"])
    n, e = g.num_nodes, g.edge_index.shape[1]
    torch.manual_seed(0)
    model = pangnn_amd.AlternateGCN(dev, None, False, dims=[64, 128], num_nodes=n, decoder=decoder, fused_decoder=fused)
    opt = make_optimizer(model)
    pw = g.class_balance
    ac = torch.autocast("cuda", dtype=torch.bfloat16, enabled=prec == "bf16")

    def step():
        opt.zero_grad(set_to_none=True)
        with ac:
            loss, _ = model.loss_and_logits(g, g.y, pw)
        loss.backward()
        opt.step()
        return loss

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        loss = step()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    peak = torch.cuda.max_memory_allocated() - base
    ts.sort()
    res = dict(decoder=decoder, fused=bool(fused), workload=workload, precision=prec, E=e, N=n, step_ms=ts[len(ts) // 2],
               step_ms_min=ts[0], peak_bytes_above_base=peak, loss=float(loss))
    if fused:
        # the two passes alone, on the encoder output of this model
        with torch.no_grad(), ac:
            z = model.encode(g)
        st = structure_of(g.edge_index, n, g, "sim")
        z = z.detach().requires_grad_(True)
        fw, bw = [], []
        for i in range(warmup + steps):
            a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            a.record()
            l, _ = PF.edge_score_loss(z, st, decoder, g.y, pw, e)
            b.record()
            l.backward()
            c.record()
            torch.cuda.synchronize()
            z.grad = None
            if i >= warmup:
                fw.append(a.elapsed_time(b))
                bw.append(b.elapsed_time(c))
        fw.sort()
        bw.sort()
        es = z.element_size()
        res.update(edge_pass_ms=fw[len(fw) // 2], node_pass_ms=bw[len(bw) // 2],
                   # gathered row bytes (two rows per edge forward, one row per CSR entry backward, both orders)
                   edge_pass_row_bytes=2 * e * 64 * es, node_pass_row_bytes=2 * e * 64 * es,
                   edge_pass_GBps=2 * e * 64 * es / fw[len(fw) // 2] / 1e6, node_pass_GBps=2 * e * 64 * es / bw[len(bw) // 2] / 1e6)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=4, metavar=("DECODER", "FUSED", "WORKLOAD", "PREC"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per child process")
    ap.add_argument("--out", default=None, help="append the JSON lines here")
    a = ap.parse_args()
    if a.child:
        d, f, wl, p = a.child
        child(d, int(f), wl, p, a.steps, a.warmup)
        return
    configs = [(d, f, "cfg4", "fp32") for d in ("cosine", "dot") for f in (1, 0)] + [("cosine", 1, "cfg5slice", "bf16")]
    lines = []
    for d, f, wl, p in configs:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", d, str(f), wl, p, "--steps", str(a.steps),
               "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
            sys.exit(f"child {d} fused={f} {wl} {p} failed with {r.returncode}: nothing more is started")
        lines.append(r.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    # the literal route at cfg5slice, by arithmetic: E from the fused child, one [E, 2D] fp32 gather + its gradient
    e5 = json.loads(lines[-1])["E"]
    lines.append(json.dumps(dict(decoder="cosine", fused=False, workload="cfg5slice", precision="bf16", E=e5, measured=False,
                                 gather_bytes=e5 * 128 * 4, gather_plus_grad_bytes=2 * e5 * 128 * 4)))
    print(lines[-1])
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
