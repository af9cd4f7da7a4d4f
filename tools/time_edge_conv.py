"""EdgeConv(64, 64) and EdgeConv(64, 128), forward and forward + backward, fused (csrc/edge_conv.hip) against the literal
gather / MLP / segment-max route (PANGNN_FUSE_EDGE_CONV=0), on two simulated similarity graphs:

  * small: config 2's size, `simulate_graph(1000, 5, 0.3, 10, 2)` (N = 5 000, E ~ 4.5e4);
  * large: `simulate_graph(--large-genes, 20, 0.2, 100, 20)` — config 4's law at a size whose literal route (about 4 KB of
    [E, .] tensors per edge over forward + backward) still fits in memory; default 10 000 genes per genome
    (N = 2e5, E ~ 1.5e7).

Every (graph, width, route) runs in a fresh child process (the switch is read at import; no allocator state is shared), by
events, median after warm-up, with the peak allocated bytes of one forward + backward above the level before it.  The fused
lines carry the algorithmic bytes E * (out * 4 + 8) + 3 * N * out * 4 of the forward's edge pass and the fraction of 8 TB/s
the whole fused forward achieves against them.

    python tools/time_edge_conv.py --out profiles/edge_conv.jsonl

On a shared machine run it under a time limit, e.g. `timeout -k 10 900 python tools/time_edge_conv.py`.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BPS = 8e12
GRAPHS = {"small": (1000, 5, 0.3, 10, 2)}


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
    ei = g.edge_index.contiguous()
    n, e = g.num_nodes, ei.shape[1]
    del g
    torch.manual_seed(0)
    m = pangnn_amd.EdgeConv(64, a.out).to(dev)
    x = torch.randn(n, 64, device=dev)
    go = torch.randn(n, a.out, device=dev)

    def fwd():
        with torch.no_grad():
            return m(x, ei)

    def fwd_bwd():
        xg = x.detach().requires_grad_(True)
        m(xg, ei).backward(go)
        m.zero_grad(set_to_none=True)

    f_ms, f_min = _median_ms(fwd, a.steps, a.warmup)
    fb_ms, fb_min = _median_ms(fwd_bwd, a.steps, a.warmup)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fwd_bwd()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    line = dict(graph=a.graph, N=n, E=e, out=a.out, route="fused" if PF.FUSE_EDGE_CONV else "literal", fwd_ms=f_ms,
                fwd_ms_min=f_min, fwd_bwd_ms=fb_ms, fwd_bwd_ms_min=fb_min, peak_bytes_fwd_bwd=peak)
    if PF.FUSE_EDGE_CONV:
        nbytes = e * (a.out * 4 + 8) + 3 * n * a.out * 4
        line.update(fwd_algorithmic_bytes=nbytes, fwd_fraction_of_8TBps=nbytes / (f_ms * 1e-3) / HBM_BPS,
                    fwd_mfma_tflops=2.0 * e * a.out * a.out / (f_ms * 1e-3) / 1e12)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--large-genes", type=int, default=10000)
    ap.add_argument("--graphs", default="small,large")
    ap.add_argument("--out", default=None, help="append the JSON lines here")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--graph", default="small", help=argparse.SUPPRESS)
    ap.add_argument("--width", dest="out_width", type=int, default=64, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        a.out = a.out_width
        return child(a)
    lines = []
    for graph in a.graphs.split(","):
        for width in (64, 128):
            for fuse in ("1", "0"):
                env = dict(os.environ, PANGNN_FUSE_EDGE_CONV=fuse)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--graph", graph, "--width", str(width),
                       "--steps", str(a.steps), "--warmup", str(a.warmup), "--large-genes", str(a.large_genes)]
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
