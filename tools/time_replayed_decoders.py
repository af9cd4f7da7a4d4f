"""Training steps of the mini-batch regime on the decoders outside decoder16.hip, three ways (train.ReplayedFreshStep):

    python tools/time_replayed_decoders.py --out profiles/replayed_decoders.md

Data: config 2's sub-graph set, simulate_subgraph_dataset(1000, 5, 0.3, 10, 2); a pass is --steps consecutive 32-graph batches.
Variants: `--decoder cosine`, `--decoder dot`, the mlp decoder at node_dim 32 and 128, and at 64 in the strict-fp32 mode
(PANGNN_DECODER_PRECISION=0).  Routes, each on a model and optimizer of its own, alternated inside one loop of one process:
  (a) train.train_step(model, opt, ds.batch(i, i + 32), ...): unpadded collation, structure builds and every launch issued from
      the host — the route these variants had before the fused-loss kernels read the real-edge count from device memory;
  (b) train.ReplayedFreshStep(capture=False): the padded step, launches issued from the host;
  (c) train.ReplayedFreshStep(capture=True): one id write and one graph launch per step.
Host clock around a whole pass that ends in torch.cuda.synchronize(); --warmup passes, then the median of --passes passes and
their spread (min .. max), divided by the steps of a pass."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VARIANTS = {
    "cosine": dict(dims=[64, 128], decoder="cosine"),
    "dot": dict(dims=[64, 128], decoder="dot"),
    "mlp d32": dict(dims=[32, 64]),
    "mlp d128": dict(dims=[128, 128]),
    "mlp d64 strict fp32": dict(dims=[64, 128]),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20, help="32-graph batches per pass")
    ap.add_argument("--groups", type=int, default=1000)
    ap.add_argument("--out", default=None, help="write the markdown report here")
    a = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    import pangnn_amd
    from pangnn_amd import functional as PF
    from pangnn_amd import simulate
    from pangnn_amd.train import ReplayedFreshStep, make_optimizer, train_step
    if not torch.cuda.is_available():
        sys.exit("time_replayed_decoders.py measures on the GPU: none here")
    dev = torch.device("cuda")
    ds = simulate.simulate_subgraph_dataset(a.groups, 5, 0.3, 10, 2, seed=0, device=dev)
    pw = ds.class_balance()
    steps = min(a.steps, ds.num_graphs // 32)
    batches = [list(range(32 * k, 32 * k + 32)) for k in range(steps)]
    names = {"a": "(a) train_step on ds.batch(...)", "b": "(b) ReplayedFreshStep(capture=False)",
             "c": "(c) ReplayedFreshStep(capture=True)"}
    rows, notes = [], []
    for vname, kw in VARIANTS.items():
        old = PF.DECODER_PRECISION
        if "strict" in vname:
            PF.DECODER_PRECISION = 0
        try:
            def make():
                torch.manual_seed(0)
                model = pangnn_amd.AlternateGCN(dev, None, False, **kw)
                return model, make_optimizer(model, capturable=True)
            ma, oa = make()
            mb, ob = make()
            mc, oc = make()
            eager = ReplayedFreshStep(mb, ob, ds, pw, 32, capture=False)
            graphed = ReplayedFreshStep(mc, oc, ds, pw, 32, capture=True)

            def pass_a():
                for ids in batches:
                    g = ds.batch(ids[0], ids[-1] + 1)
                    loss, _ = train_step(ma, oa, g, g.y, pw)
                return loss

            def pass_of(step):
                def run():
                    for ids in batches:
                        loss, _ = step(ids)
                    return loss
                return run

            routes = {"a": pass_a, "b": pass_of(eager), "c": pass_of(graphed)}
            times = {k: [] for k in routes}
            last = {}
            for i in range(a.warmup + a.passes):
                for k, f in routes.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    last[k] = f()
                    torch.cuda.synchronize()
                    if i >= a.warmup:
                        times[k].append((time.perf_counter() - t0) * 1e3 / steps)
        finally:
            PF.DECODER_PRECISION = old
        med = {k: statistics.median(v) for k, v in times.items()}
        for k in routes:
            rows.append(f"| {vname} | {names[k]} | {med[k]:.3f} | {min(times[k]):.3f} .. {max(times[k]):.3f} | "
                        f"{med['a'] / med[k]:.2f} | {float(last[k]):.6f} |")
        spread = max(max(times[k]) - min(times[k]) for k in ("a", "c"))
        verdict = "faster captured" if med["a"] - med["c"] > spread else "NOT faster captured by more than the spread"
        notes.append(f"- {vname}: (a) / (c) = {med['a'] / med['c']:.2f}, (a) - (c) = {med['a'] - med['c']:.3f} ms per step against "
                     f"a pass-to-pass spread of {spread:.3f} ms: {verdict}.")
    out = ["# Training steps of the mini-batch regime on cosine, dot, node_dim 32 / 128 and strict fp32", "",
           f"`python tools/time_replayed_decoders.py --passes {a.passes} --warmup {a.warmup} --steps {steps}` on "
           f"{torch.cuda.get_device_name(0)}: simulate_subgraph_dataset({a.groups}, 5, 0.3, 10, 2), {ds.num_graphs} sub-graphs; a pass "
           f"is {steps} consecutive batches of 32 sub-graphs; host clock around a whole pass that ends in a synchronisation, routes "
           f"alternated, median of {a.passes} passes after {a.warmup}; each route trains a model of its own from the same seed "
           "(the last column is its loss on the pass's last batch after all passes: three models trained apart for "
           f"{(a.warmup + a.passes) * steps} steps, whose fp32 re-association differences grow with the steps).", "",
           "| variant | route | ms per step (median) | spread (min .. max) | (a) / route | last loss |", "|---|---|---|---|---|---|"]
    out += rows + [""] + notes
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
