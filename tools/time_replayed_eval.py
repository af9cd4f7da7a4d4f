"""One validation pass of the mini-batch regime three ways, and the epoch around it (train.ReplayedFreshEval, train.run_epoch):

    python tools/time_replayed_eval.py --out profiles/replayed_eval.md

Data: config 2's sub-graph set, simulate_subgraph_dataset(1000, 5, 0.3, 10, 2); default model; the pass covers 15 % of the
graphs in 32-graph batches.  Routes, alternated inside one loop of the same process:
  (a) train.evaluate(model, [ds.batch(i, i + 32), ...], pw): unpadded collation, structure builds and every launch issued from
      the host, one score / label tensor per batch for the ranking metrics;
  (b) train.ReplayedFreshEval(capture=False): the padded step, launches issued from the host;
  (c) train.ReplayedFreshEval(capture=True): one id write and one graph launch per batch.
Host clock around a whole pass that ends in its read-out (`compute()` / evaluate's return: both synchronise); --warmup passes,
then the median of --passes passes and their spread (min .. max).  Also: an epoch over 70 % training graphs + that pass,
run_epoch against ReplayedFreshStep + route (a).

`--kernel-only` runs route (c)'s pass a few times and nothing else, for
    rocprofv3 --kernel-trace --stats -- python tools/time_replayed_eval.py --kernel-only
whose statistics give the time of the stats kernel itself (batch_stats_small_kernel)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--groups", type=int, default=1000)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None, help="write the markdown report here")
    a = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    import pangnn_amd
    from pangnn_amd import simulate
    from pangnn_amd.metrics import EpochStats
    from pangnn_amd.train import ReplayedFreshEval, ReplayedFreshStep, evaluate, make_optimizer, run_epoch
    if not torch.cuda.is_available():
        sys.exit("time_replayed_eval.py measures on the GPU: none here")
    dev = torch.device("cuda")
    ds = simulate.simulate_subgraph_dataset(a.groups, 5, 0.3, 10, 2, seed=0, device=dev)
    pw = ds.class_balance()
    n_train, n_val = int(0.7 * ds.num_graphs), int(0.15 * ds.num_graphs)
    train_ids, val_ids = list(range(n_train)), list(range(n_train, n_train + n_val))
    val_batches = [val_ids[k:k + 32] for k in range(0, n_val, 32)]
    torch.manual_seed(0)
    model = pangnn_amd.AlternateGCN(dev, None, False, dims=[64, 128])

    eager = ReplayedFreshEval(model, ds, pw, 32, graphs=val_ids, capture=False)
    graphed = ReplayedFreshEval(model, ds, pw, 32, graphs=val_ids, capture=True)

    def pass_a():
        return evaluate(model, [ds.batch(ids[0], ids[-1] + 1) for ids in val_batches], pw)

    def pass_of(ev):
        def run():
            ev.reset()
            for ids in val_batches:
                ev(ids)
            return ev.compute()
        return run

    if a.kernel_only:
        for _ in range(a.warmup + 3):
            pass_of(graphed)()
        torch.cuda.synchronize()
        return

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
                times[k].append((time.perf_counter() - t0) * 1e3)

    # the epoch: 70 % training graphs replayed + the validation pass
    opt = make_optimizer(model, capturable=True)
    step = ReplayedFreshStep(model, opt, ds, pw, 32, graphs=train_ids, stats=EpochStats(0, device=dev))
    plain = ReplayedFreshStep(model, opt, ds, pw, 32, graphs=train_ids)
    gen = torch.Generator().manual_seed(1)

    def epoch_new():
        return run_epoch(step, graphed, train_ids, val_ids, 32, generator=gen)

    def epoch_old():
        order = torch.randperm(n_train, generator=gen).tolist()
        for k in range(0, n_train, 32):
            plain([train_ids[j] for j in order[k:k + 32]])
        return pass_a()

    epochs = {"run_epoch": epoch_new, "ReplayedFreshStep + (a)": epoch_old}
    etimes = {k: [] for k in epochs}
    for i in range(2 + max(a.passes // 2, 5)):
        for k, f in epochs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            if i >= 2:
                etimes[k].append((time.perf_counter() - t0) * 1e3)

    def row(name, ts, per):
        med = statistics.median(ts)
        return f"| {name} | {med:.3f} | {min(ts):.3f} .. {max(ts):.3f} | {med / per:.3f} |"

    nb, steps = len(val_batches), -(-n_train // 32)
    edges = sum(ds._host().edge[i + 1] - ds._host().edge[i] for i in val_ids)
    names = {"a": "(a) train.evaluate over ds.batch(...)", "b": "(b) ReplayedFreshEval(capture=False)",
             "c": "(c) ReplayedFreshEval(capture=True)"}
    out = ["# Validation pass of the mini-batch regime: train.ReplayedFreshEval", "",
           f"`python tools/time_replayed_eval.py --passes {a.passes} --warmup {a.warmup}` on {torch.cuda.get_device_name(0)}: "
           f"simulate_subgraph_dataset({a.groups}, 5, 0.3, 10, 2), {ds.num_graphs} sub-graphs; the pass is {n_val} graphs "
           f"({edges} edges) in {nb} batches of 32; host clock around a whole pass including its read-out, routes alternated, "
           f"median of {a.passes} passes after {a.warmup}.", "",
           "| route | ms per pass (median) | spread (min .. max) | ms per batch |", "|---|---|---|---|"]
    out += [row(names[k], times[k], nb) for k in routes]
    ma, mc = statistics.median(times["a"]), statistics.median(times["c"])
    spread = max(max(times[k]) - min(times[k]) for k in ("a", "c"))
    out += ["", f"(a) / (c) = {ma / mc:.2f}; (a) - (c) = {ma - mc:.3f} ms against a pass-to-pass spread of {spread:.3f} ms: "
            + ("(c) beats (a) by more than the spread." if ma - mc > spread else "(c) does NOT beat (a) by more than the spread."),
            "", "The three routes' results on the last pass (same weights):", ""]
    out += [f"- {names[k]}: " + ", ".join(f"{m}={last[k][m]:.6f}" for m in ("loss", "accuracy", "f1", "roc_auc", "pr_auc"))
            for k in routes]
    out += ["", f"## The epoch: {n_train} training graphs ({steps} replayed steps) + that pass", "",
            "| route | ms per epoch (median) | spread (min .. max) | ms per batch |", "|---|---|---|---|"]
    out += [row(k, etimes[k], steps + nb) for k in epochs]
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
