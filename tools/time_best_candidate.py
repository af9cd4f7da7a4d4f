"""Max-candidate labelling at config 4 (`simulate_graph(50000, 20, 0.2, 100, 20)`, N = 1e6, E = 7.47e7), fp32 logits:

  * the segment build (candidates.build_segments): the sorted fast path on the canonical graph, and the general path on
    the same graph with its node ids permuted;
  * the kernel (pangnn_best_candidate_f32) by events, median after warm-up: fast / general path, with and without the
    fused confusion counts;
  * the whole predict_homolog_genes pass (forward in eval mode + every statistic + the one host read-out), first call
    (segment structure and model structures built) and warm calls.

Each kernel figure is set against its algorithmic bytes (value 4 B + label 1 B per edge, + seg_edge 4 B on the general
path, + y 4 B with counts, + 8 B per segment boundary) and the arithmetic bound at 8 TB/s.

    python tools/time_best_candidate.py --out profiles/best_candidate.jsonl
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/time_best_candidate.py --kernel-only     # a run of its own
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BPS = 8e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true", help="graph + segments, then the kernel calls only (for rocprofv3)")
    ap.add_argument("--out", default=None, help="append the JSON lines here")
    a = ap.parse_args()

    import torch
    import pangnn_amd
    from pangnn_amd import _lib, candidates, simulate
    dev = torch.device("cuda")
    lib = _lib.load()
    g = simulate.simulate_graph(50000, 20, 0.2, 100, 20, seed=0, device=dev)
    n, e = g.num_nodes, g.edge_index.shape[1]
    perm = torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    ei2 = perm[g.edge_index]
    go2 = torch.empty_like(g.genome_of)
    go2[perm] = g.genome_of
    torch.manual_seed(0)
    logits = torch.randn(e, device=dev)
    y = g.y.contiguous()
    lines = []

    seg_fast = candidates.build_segments(g.edge_index, g.genome_of)
    seg_gen = candidates.build_segments(ei2, go2)
    assert seg_fast.seg_edge is None and seg_gen.seg_edge is not None and seg_fast.num_segments == seg_gen.num_segments
    s = seg_fast.num_segments
    if not a.kernel_only:
        for name, (ei, go) in (("fast", (g.edge_index, g.genome_of)), ("general", (ei2, go2))):
            med, mn = _median_ms(lambda: candidates.build_segments(ei, go), max(a.steps // 4, 3), 2)
            lines.append(dict(what="segment_build", path=name, E=e, S=s, ms=med, ms_min=mn))
            print(json.dumps(lines[-1]), flush=True)

    label = torch.empty(e, dtype=torch.uint8, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    ref = None
    for name, seg in (("fast", seg_fast), ("general", seg_gen)):
        for fused in (False, True):
            def call():
                _lib.check(lib.pangnn_best_candidate_f32(seg.seg_rowptr.data_ptr(), _lib.ptr(seg.seg_edge), s, e,
                                                         logits.data_ptr(), y.data_ptr() if fused else None,
                                                         counts.data_ptr() if fused else None, label.data_ptr(),
                                                         _lib.stream_ptr()), "pangnn_best_candidate_f32")
            med, mn = _median_ms(call, a.steps, a.warmup)
            if name == "fast" and not fused:
                ref = label.clone()
            nbytes = e * (4 + 1) + 8 * (s + 1) + (4 * e if seg.seg_edge is not None else 0) + (4 * e if fused else 0)
            lines.append(dict(what="kernel", path=name, fused_counts=fused, E=e, S=s, ms=med, ms_min=mn,
                              algorithmic_bytes=nbytes, achieved_TBps=nbytes / med / 1e9,
                              bound_ms_at_8TBps=nbytes / HBM_BPS * 1e3))
            print(json.dumps(lines[-1]), flush=True)
    torch.cuda.synchronize()
    if a.kernel_only:
        return
    # the permuted graph labels the same edges: same bits in edge order
    lab_gen = candidates.best_candidate(logits, ei2, go2).view(torch.uint8)
    assert torch.equal(lab_gen, ref), "fast and general path disagree"

    model = pangnn_amd.AlternateGCN(dev, None, False, dims=[64, 128], num_nodes=n)
    candidates.SEGMENTS.clear()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, _, stats = pangnn_amd.predict_homolog_genes(model, None, g, binary_th=0.5)
    torch.cuda.synchronize()
    cold = (time.perf_counter() - t0) * 1e3
    walls = []
    for _ in range(max(a.steps // 4, 3)):
        t0 = time.perf_counter()
        pangnn_amd.predict_homolog_genes(model, None, g, binary_th=0.5)   # ends with a host read-out: wall time is the pass
        walls.append((time.perf_counter() - t0) * 1e3)
    walls.sort()
    lines.append(dict(what="predict_homolog_genes", E=e, first_call_ms=cold, warm_ms=walls[len(walls) // 2],
                      warm_ms_min=walls[0], stats={k: v for k, v in stats.items() if not isinstance(v, dict)},
                      max_logit_candidate=stats.get("max_logit_candidate")))
    print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
