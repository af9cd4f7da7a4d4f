"""The launches of the edge-weight gradient (csrc/edge_weight_grad.hip) at conv_in's shape of config 4
(`--simulate_dataset 50000 20 0.2 100 20`, the similarity graph): the edge dot (pangnn_edge_dot_mixed) and the norm backward
(pangnn_gcn_norm_bwd_f32), beside the transposed propagate of the same structure and width in the same process, at F = 64
(conv_in is propagate-first) and F = 128.  The edge dot gathers the same rows as that propagate: its time is held against that
measured launch.  Also timed: the edge dot without its store through `perm`, and the forward propagate (the edge dot's own
gather order: by target).

    python tools/time_edge_weight_grad.py --out profiles/edge_weight_grad.jsonl

Per launch: CUDA events around the call, the three launches alternating inside one loop, median and minimum of --steps after
--warmup; gathered row bytes by arithmetic (one F-wide row per entry).  `--genes` shrinks the graph (debug)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--genes", type=int, default=50000)
    ap.add_argument("--rows", default="f32", choices=["f32", "bf16", "f16"])
    ap.add_argument("--out", default=None, help="append the JSON lines here")
    a = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    from pangnn_amd import functional as PF
    from pangnn_amd import simulate
    from pangnn_amd.graph import structure_of
    if not torch.cuda.is_available():
        sys.exit("time_edge_weight_grad.py measures on the GPU: none here")
    dev = torch.device("cuda")
    g = simulate.simulate_graph(a.genes, 20, 0.2, 100, 20, seed=0, device=dev)
    n, e = g.num_nodes, g.edge_index.shape[1]
    st = structure_of(g.edge_index, n, g, "sim")
    norm = st.gcn_norm(g.edge_attr)
    norm.by_src                                        # (the transposed propagate's weights: built outside the timed loop)
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[a.rows]
    lens = (st.by_dst.rowptr[1:] - st.by_dst.rowptr[:-1]).float()
    lines = []
    for f in (64, 128):
        torch.manual_seed(f)
        x = torch.randn(n, f, device=dev).to(dt)
        up = torch.randn(n, f, device=dev).to(dt)
        gw = PF.edge_dot(st.by_dst, up, x)[1]
        ts = {"propagate_T": [], "edge_dot": [], "norm_bwd": [], "edge_dot_sorted_only": [], "propagate_fwd": []}
        for i in range(a.warmup + a.steps):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
            ev[0].record()
            PF.spmm_csr(st.by_src, norm.by_src, up, st.num_src)
            ev[1].record()
            PF.edge_dot(st.by_dst, up, x)
            ev[2].record()
            PF.gcn_norm_backward(st, norm, gw)
            ev[3].record()
            PF.edge_dot(st.by_dst, up, x, want_orig=False)          # without the store through perm: what that store costs
            ev[4].record()
            PF.spmm_csr(st.by_dst, norm.by_dst, x, n)               # the forward propagate: the edge dot's own gather order
            ev[5].record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                for k, name in enumerate(ts):
                    ts[name].append(ev[k].elapsed_time(ev[k + 1]))
        row_bytes = e * f * x.element_size()
        res = dict(shape="cfg4 conv_in (sim graph)", genes=a.genes, N=n, E=e, F=f, rows=a.rows, steps=a.steps,
                   mean_in_degree=float(lens.mean()), max_in_degree=int(lens.max()), gathered_row_bytes=row_bytes)
        for name, v in ts.items():
            v.sort()
            res[name + "_ms"] = v[len(v) // 2]
            res[name + "_ms_min"] = v[0]
        res["edge_dot_over_propagate_T"] = res["edge_dot_ms"] / res["propagate_T_ms"]
        res["edge_dot_gather_GBps"] = row_bytes / res["edge_dot_ms"] / 1e6
        res["propagate_T_gather_GBps"] = row_bytes / res["propagate_T_ms"] / 1e6
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
