"""--union_edge_weights mini-batches: the captured fresh training step and the captured validation batch against the eager
route a union model had before the padded batch carried a union list:

    python tools/time_union_batches.py --out profiles/union_batches.md

Data: config 2's sub-graph set, simulate_subgraph_dataset(1000, 5, 0.3, 10, 2); a pass is --steps shuffled 32-graph batches, the
same ids on every route.  Models: union at dims (64, 128), and with neighbours=4.  Routes, each on a model (and optimizer) of
its own, alternated inside one loop of one process:
  train (a) train.train_step over pangnn_amd.Batch.from_data_list of the reference-layout union sub-graphs ([neighbour |
            similarity] edges, [1 | w] weights, device-resident) of the batch's ids: collation, two structure builds and every
            launch issued from the host;
  train (c) train.ReplayedFreshStep(capture=True): one id write and one graph launch per step;
  val   (a) model.eval()(Batch.from_data_list(...)) under no_grad;
  val   (c) train.ReplayedFreshEval(capture=True, ranking=False).
Device events around a whole pass (recorded on the current stream, read after a synchronisation); --warmup passes, then the
median of --passes passes and their spread (min .. max), divided by the steps of a pass."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VARIANTS = {
    "union (64, 128)": dict(dims=[64, 128], union_edge_weights=True),
    "union neighbours=4 (64, 128)": dict(dims=[64, 128], union_edge_weights=True, neighbours=4),
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
    from pangnn_amd import simulate
    from pangnn_amd.train import ReplayedFreshEval, ReplayedFreshStep, make_optimizer, train_step
    if not torch.cuda.is_available():
        sys.exit("time_union_batches.py measures on the GPU: none here")
    dev = torch.device("cuda")
    ds = simulate.simulate_subgraph_dataset(a.groups, 5, 0.3, 10, 2, seed=0, device=dev)
    pw = ds.class_balance()
    h = ds._host()
    steps = min(a.steps, ds.num_graphs // 32)
    perm = torch.randperm(ds.num_graphs, generator=torch.Generator().manual_seed(0)).tolist()
    batches = [perm[32 * k:32 * k + 32] for k in range(steps)]
    # the reference's own union sub-graphs (dataset.py:287-302), one Data per group, resident on the device
    subs = []
    for i in range(ds.num_graphs):
        n0, e0, e1, b0, b1 = h.node[i], h.edge[i], h.edge[i + 1], h.nb[i], h.nb[i + 1]
        ei, nb = ds.edge_index[:, e0:e1] - n0, ds.neighbour_edge_index[:, b0:b1] - n0
        subs.append(pangnn_amd.Data(torch.ones(h.node[i + 1] - n0, 1, device=dev), ei.contiguous(),
                                    torch.cat([torch.ones(b1 - b0, device=dev), ds.edge_attr[e0:e1]]), ds.y[e0:e1].contiguous(),
                                    union_edge_index=torch.cat([nb, ei], dim=1).contiguous()))
    names = {"ta": "train (a) train_step on Batch.from_data_list", "tc": "train (c) ReplayedFreshStep(capture=True)",
             "va": "val (a) model.eval() on Batch.from_data_list", "vc": "val (c) ReplayedFreshEval(capture=True)"}
    rows, notes = [], []
    for vname, kw in VARIANTS.items():
        def make():
            torch.manual_seed(0)
            model = pangnn_amd.AlternateGCN(dev, None, False, **kw)
            return model, make_optimizer(model, capturable=True)
        ma, oa = make()
        mc, oc = make()
        mv, _ = make()
        mv.eval()
        graphed = ReplayedFreshStep(mc, oc, ds, pw, 32, capture=True)
        evaluator = ReplayedFreshEval(mv, ds, pw, 32, capture=True, ranking=False)

        def train_a():
            for ids in batches:
                g = pangnn_amd.Batch.from_data_list([subs[i] for i in ids])
                train_step(ma, oa, g, g.y, pw)

        def train_c():
            for ids in batches:
                graphed(ids)

        @torch.no_grad()
        def val_a():
            for ids in batches:
                mv(pangnn_amd.Batch.from_data_list([subs[i] for i in ids]))

        def val_c():
            for ids in batches:
                evaluator(ids)

        routes = {"ta": train_a, "tc": train_c, "va": val_a, "vc": val_c}
        times = {k: [] for k in routes}
        for i in range(a.warmup + a.passes):
            for k, f in routes.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0.record()
                f()
                t1.record()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    times[k].append(t0.elapsed_time(t1) / steps)
            evaluator.reset()
        med = {k: statistics.median(v) for k, v in times.items()}
        for k in routes:
            base = med[k[0] + "a"]
            rows.append(f"| {vname} | {names[k]} | {med[k]:.3f} | {min(times[k]):.3f} .. {max(times[k]):.3f} | {base / med[k]:.2f} |")
        for kind, x, y in (("training step", "ta", "tc"), ("validation batch", "va", "vc")):
            spread = max(max(times[k]) - min(times[k]) for k in (x, y))
            verdict = "faster captured" if med[x] - med[y] > spread else "NOT faster captured by more than the spread"
            notes.append(f"- {vname}, {kind}: (a) / (c) = {med[x] / med[y]:.2f}, (a) - (c) = {med[x] - med[y]:.3f} ms against a "
                         f"pass-to-pass spread of {spread:.3f} ms: {verdict}.")
    spec, worst = graphed.spec, graphed.spec_worst
    out = ["# --union_edge_weights mini-batches: captured step and validation batch against the eager route", "",
           f"`python tools/time_union_batches.py --passes {a.passes} --warmup {a.warmup} --steps {steps}` on "
           f"{torch.cuda.get_device_name(0)} ({getattr(torch.cuda.get_device_properties(0), 'gcnArchName', 'arch unknown')}): "
           f"simulate_subgraph_dataset({a.groups}, 5, 0.3, 10, 2), {ds.num_graphs} sub-graphs; a pass "
           f"is {steps} shuffled batches of 32 sub-graphs, the same ids on every route; device events around a whole pass, routes "
           f"alternated, median of {a.passes} passes after {a.warmup}; each route runs a model of its own from the same seed.  "
           f"Everyday buffers {tuple(spec)} (union list of {spec.edges + spec.nb_edges} columns), worst case {tuple(worst)} "
           f"({worst.edges + worst.nb_edges}); slots built during the run: {len(graphed._slots)}.", "",
           "| model | route | ms per batch (median) | spread (min .. max) | (a) / route |", "|---|---|---|---|---|"]
    out += rows + [""] + notes
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
