#!/usr/bin/env python3
"""Backward of the decoder's P | Q layer on the cfg-4 graph (N = 1e6, E = 74.7e6): the four launches of the unfused route
(two pangnn_spmm_csr_f32 part sums into one [N, 128] matrix, pangnn_linear_dgrad_mixed, pangnn_linear_act_wgrad_mixed)
against the one launch of pangnn_linear_act_backward_parts_f32, on the graph's own run-sum plans with random part rows.
Event-timed; prints both times and torch.equal of the three outputs (gx, gw, gb).

    python tools/time_pq_backward.py [--genes 50000] [--iters 20] [--limit 300]

`--limit`: seconds after which the process ends itself (SIGALRM), whatever it is doing."""
import argparse
import json
import os
import signal
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=50000, help="genes per genome (cfg4: 50000 x 20 genomes)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--in-act", type=int, default=1)
    ap.add_argument("--limit", type=int, default=300)
    args = ap.parse_args()
    signal.alarm(args.limit)

    from pangnn_amd import _lib, simulate
    from pangnn_amd import functional as PF
    from pangnn_amd.graph import structure_of
    dev = torch.device("cuda:0")
    lib = _lib.load()
    g = simulate.simulate_graph(args.genes, 20, 0.2, 100, 20, seed=0, device=dev)
    n, e = g.num_nodes, g.edge_index.shape[1]
    st = structure_of(g.edge_index, n)
    ct = PF.d16_chunk(e)
    plan_s, plan_t = st.runsum_plan(ct), st.csr_plan("dst", ct)
    if plan_s is None:
        sys.exit("the edge list is not sorted by source: no run-sum plan")
    torch.manual_seed(0)
    parts_s = torch.randn(plan_s.n_parts, 64, device=dev)
    parts_t = torch.randn(plan_t.n_parts, 64, device=dev)
    z = torch.randn(n, 64, device=dev)
    w = torch.randn(128, 64, device=dev) * 0.1
    ws_bytes = lib.pangnn_linear_wgrad_workspace_bytes(64, 128)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    act = int(args.in_act)

    def unfused():
        gpq = torch.empty(n, 128, device=dev)
        PF._sum_parts(plan_s, parts_s, n, gpq[:, :64])
        PF._sum_parts(plan_t, parts_t, n, gpq[:, 64:])
        gx, gw, gb = torch.empty(n, 64, device=dev), torch.empty(128, 64, device=dev), torch.empty(128, device=dev)
        _lib.check(lib.pangnn_linear_dgrad_mixed(gpq.data_ptr(), 0, 128, w.data_ptr(), gx.data_ptr(), 0, 64, n, 64, 128,
                                                 z.data_ptr() if act else None, 0, 64 if act else 0, _lib.stream_ptr()),
                   "pangnn_linear_dgrad_mixed")
        _lib.check(lib.pangnn_linear_act_wgrad_mixed(gpq.data_ptr(), 0, 128, z.data_ptr(), 0, 64, n, 64, 128, act, gw.data_ptr(),
                                                     gb.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr()),
                   "pangnn_linear_act_wgrad_mixed")
        return gx, gw, gb

    def fused():
        gx, gw, gb = torch.empty(n, 64, device=dev), torch.empty(128, 64, device=dev), torch.empty(128, device=dev)
        _lib.check(lib.pangnn_linear_act_backward_parts_f32(
            parts_s.data_ptr(), plan_s.part_rowptr.data_ptr(), parts_s.shape[0], parts_t.data_ptr(),
            plan_t.part_rowptr.data_ptr(), parts_t.shape[0], z.data_ptr(), 64, w.data_ptr(), n, 64, 128, act, gx.data_ptr(), 64,
            gw.data_ptr(), gb.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr()), "pangnn_linear_act_backward_parts_f32")
        return gx, gw, gb

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        ms.sort()
        return out, ms[len(ms) // 2], ms[0], ms[-1]

    with _lib.device_guard(dev):
        ref, t_ref, lo_ref, hi_ref = timed(unfused)
        got, t_new, lo_new, hi_new = timed(fused)
    parts_per_row = [float(p.n_parts_exact()) / n for p in (plan_s, plan_t)]
    print(json.dumps({"nodes": n, "edges": e, "in_act": act, "parts_per_row": parts_per_row,
                      "unfused_ms": {"median": t_ref, "min": lo_ref, "max": hi_ref},
                      "fused_ms": {"median": t_new, "min": lo_new, "max": hi_new},
                      "equal": {k: bool(torch.equal(a, b)) for k, a, b in zip(("gx", "gw", "gb"), got, ref)}}))


if __name__ == "__main__":
    main()
