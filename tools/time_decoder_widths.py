"""AlternateGCN(dims=[D, 128]) at node_dim D = 32 and 128: `loss_and_logits` + backward (the training step without the
optimizer) and the eval-mode forward, with the fused per-edge MLP decoder (the width template of csrc/decoder.hip) against the layer-by-layer
route (`fused_decoder=False`: gather-concat, torch Linear / relu_ / Linear), on two simulated similarity graphs:

  * small: config 2's size, `simulate_graph(1000, 5, 0.3, 10, 2)` (N = 5 000, E ~ 4.5e4);
  * large: `simulate_graph(--large-genes, 20, 0.2, 100, 20)` — config 4's law at a size whose layer-by-layer route still
    fits in memory; default 10 000 genes per genome (N = 2e5, E ~ 1.5e7).

Yardsticks: D = 64 with the fused decoder in both precision modes (PANGNN_DECODER_PRECISION = 1, the default, and 0).

Every (graph, width, route) runs in a fresh child process, by device events, median after warm-up, with the peak allocated
bytes of one training step above the level before it.  The routes of one width alternate, `--repeats` times each, so that
the spread between repeats of the same route is measured in the same run as the difference between the routes.

    python tools/time_decoder_widths.py --out profiles/decoder_widths.jsonl

On a shared machine run it under a time limit, e.g. `timeout -k 10 900 python tools/time_decoder_widths.py`.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GRAPHS = {"small": (1000, 5, 0.3, 10, 2)}
# (width, route, PANGNN_DECODER_PRECISION)
ROUTES = [(32, "fused", "1"), (32, "literal", "1"), (128, "fused", "1"), (128, "literal", "1"),
          (64, "fused", "1"), (64, "fused", "0")]


def _median_ms(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def child(a):
    import torch
    import pangnn_amd
    from pangnn_amd import functional as PF, simulate
    dev = torch.device("cuda")
    genes, genomes, frac, frags, shuf = GRAPHS.get(a.graph) or (a.large_genes, 20, 0.2, 100, 20)
    g = simulate.simulate_graph(genes, genomes, frac, frags, shuf, seed=0, device=dev)
    n, e = g.num_nodes, g.edge_index.shape[1]
    torch.manual_seed(0)
    model = pangnn_amd.AlternateGCN(dev, None, False, dims=[a.width, 128], num_nodes=n, fused_decoder=a.route == "fused")
    labels, pw = g.y, g.class_balance

    def train():
        model.train()
        loss, _ = model.loss_and_logits(g, labels, pw)
        loss.backward()
        model.zero_grad(set_to_none=True)

    def infer():
        model.eval()
        with torch.no_grad():
            return model(g)

    t_ms, t_min = _median_ms(train, a.steps, a.warmup)
    f_ms, f_min = _median_ms(infer, a.steps, a.warmup)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    train()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(json.dumps(dict(graph=a.graph, N=n, E=e, node_dim=a.width, route=a.route, decoder_precision=PF.DECODER_PRECISION,
                          repeat=a.repeat, train_ms=t_ms, train_ms_min=t_min, eval_fwd_ms=f_ms, eval_fwd_ms_min=f_min,
                          peak_bytes_train=peak)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--large-genes", type=int, default=10000)
    ap.add_argument("--graphs", default="small,large")
    ap.add_argument("--widths", default="32,128,64")
    ap.add_argument("--out", default=None, help="append the JSON lines here")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--graph", default="small", help=argparse.SUPPRESS)
    ap.add_argument("--width", type=int, default=32, help=argparse.SUPPRESS)
    ap.add_argument("--route", default="fused", help=argparse.SUPPRESS)
    ap.add_argument("--repeat", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    lines = []
    for graph in a.graphs.split(","):
        for width in (int(w) for w in a.widths.split(",")):
            for repeat in range(a.repeats):
                for w, route, precision in ROUTES:          # the routes of one width alternate inside every repeat
                    if w != width:
                        continue
                    env = dict(os.environ, PANGNN_DECODER_PRECISION=precision)
                    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--graph", graph, "--width", str(width),
                           "--route", route, "--repeat", str(repeat), "--steps", str(a.steps), "--warmup", str(a.warmup),
                           "--large-genes", str(a.large_genes)]
                    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
                    if r.returncode != 0:           # stop at the first failure: nothing more is started on the device
                        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                        raise SystemExit(f"child failed with status {r.returncode}: {' '.join(cmd)}")
                    line = r.stdout.strip().splitlines()[-1]
                    print(line, flush=True)
                    lines.append(line)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
