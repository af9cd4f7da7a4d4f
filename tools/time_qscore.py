"""The differentiable Q-score weights (csrc/qscore.hip: pangnn_qscore_fwd / pangnn_qscore_bwd through
pangnn_amd.weights.qscore_weights) at config 4's edge count (`--simulate_dataset 50000 20 0.2 100 20`, the similarity graph)
and on one mini-batch-sized graph, beside the plain-torch formulation of the same function on the same device tensors under
autograd (weights._qscore_torch: float64 scatter / gather passes) — the only other way to this gradient.

    python tools/time_qscore.py --out profiles/qscore_weights.jsonl

Per call: CUDA events around forward and around backward (dL/dscore and dL/dt both asked for), the two routes alternating
inside one loop, median and minimum of --steps after --warmup.  Bytes by arithmetic, every array once: score, item, weights
(+ rowptr, lse) forward; score, item, g, dL/dscore (+ rowptr, lse, the dL/dt shares) backward.  Also printed: the largest
difference between the two routes' results, and the construction's own kernel (pangnn_softmax_qscore_f64) on the same scores
laid out in segment order — the forward without its gather, temperature as a host constant.  `--genes` shrinks the large graph (debug)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--genes", type=int, default=50000)
    ap.add_argument("--t", type=float, default=0.8)
    ap.add_argument("--out", default=None, help="append the JSON lines here")
    a = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    from pangnn_amd import _lib, simulate, weights
    if not torch.cuda.is_available():
        sys.exit("time_qscore.py measures on the GPU: none here")
    dev = torch.device("cuda")
    shapes = [("cfg4 (sim graph)", (a.genes, 20, 0.2, 100, 20), True), ("mini-batch sized", (200, 4, 0.3, 10, 2), False)]
    lines = []
    for shape, sim, adjacent in shapes:
        g = simulate.simulate_graph(*sim, seed=0, device=dev, keep_raw=True, adjacent_only=adjacent)
        seg = weights.score_segments(g.edge_index, g.genome_of, holder=g)
        seg.segment_of_edge                                 # (the torch route's scatter index: built outside the timed loop)
        e, nseg = seg.num_edges, seg.num_segments
        lens = seg.counts
        for sdt in (torch.float64, torch.float32):
            score = g.raw_score.detach().to(sdt).clone().requires_grad_()
            t = torch.tensor(a.t, dtype=torch.float64, device=dev, requires_grad=True)
            up = torch.randn(e, device=dev)
            ts = {"hip_fwd": [], "hip_bwd": [], "torch_fwd": [], "torch_bwd": [], "construct_kernel": []}
            sorted64 = g.raw_score.detach().double()[seg.item.long()].contiguous()
            q = torch.empty_like(sorted64)
            res_of = {}
            for i in range(a.warmup + a.steps):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
                for k, route in enumerate(("hip", "torch")):
                    score.grad = t.grad = None
                    ev[2 * k].record()
                    if route == "hip":
                        w = weights.qscore_weights(score, seg, t)
                    else:
                        w = weights._qscore_torch(score, t, seg, 1e-8, 1.0, torch.float32)
                    ev[2 * k + 1].record()
                    w.backward(up)
                    if k == 1:
                        ev[4].record()
                    res_of[route] = (w.detach(), score.grad, t.grad)
                _lib.check(_lib.load().pangnn_softmax_qscore_f64(seg.rowptr.data_ptr(), sorted64.data_ptr(), nseg, e, a.t, 1e-8,
                                                                 1.0, q.data_ptr(), _lib.stream_ptr()))
                ev[5].record()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    for k, name in enumerate(ts):
                        ts[name].append(ev[k].elapsed_time(ev[k + 1]))
                del w
            sb = score.element_size()
            fwd_bytes = e * (sb + 4 + 4) + nseg * 24                 # + rowptr, lse and its residual
            bwd_bytes = e * (sb + 4 + 4 + sb) + nseg * 32            # + rowptr, lse and its residual, the dL/dt share
            res = dict(shape=shape, sim=list(sim), E=e, segments=nseg, mean_segment=float(lens.float().mean()),
                       max_segment=int(lens.max()), score=str(sdt).replace("torch.", ""), t=a.t, steps=a.steps,
                       fwd_bytes=fwd_bytes, bwd_bytes=bwd_bytes)
            for name, v in ts.items():
                v.sort()
                res[name + "_ms"] = v[len(v) // 2]
                res[name + "_ms_min"] = v[0]
            res["fwd_torch_over_hip"] = res["torch_fwd_ms"] / res["hip_fwd_ms"]
            res["bwd_torch_over_hip"] = res["torch_bwd_ms"] / res["hip_bwd_ms"]
            res["hip_fwd_GBps"] = fwd_bytes / res["hip_fwd_ms"] / 1e6
            res["hip_bwd_GBps"] = bwd_bytes / res["hip_bwd_ms"] / 1e6
            (wh, gh, th), (wt, gt, tt) = res_of["hip"], res_of["torch"]
            res["max_abs_dw"] = float((wh - wt).abs().max())
            res["max_abs_dgscore_over_max"] = float((gh - gt).abs().max() / gt.abs().max().clamp_min(1e-300))
            res["dLdt_hip"], res["dLdt_torch"] = float(th), float(tt)
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
            del res_of, score, up, sorted64, q
        del g, seg
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
