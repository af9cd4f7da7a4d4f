"""Per-step edge sub-sampling at config 4 (`simulate_graph(50000, 20, 0.2, 100, 20)`, N = 1e6, E = 7.47e7), fraction 0.8.
One process, device events on the stream, the two routes alternated call by call, warm-up discarded:

  (a) the child's edge list (+ edge_attr, y, kept_id) and BOTH CSR orders derived from the parent's tables by
      pangnn_structure_filter (EdgeStructure.filtered, num_kept known: no read-back);
  (b) what the same tables cost before: build_csr (stable radix sort) for both orders on the compacted edge_index, without
      the validity read-back — the compaction of the edge list itself (torch boolean indexing) is timed apart as (b');
  (c) drawing the exact-count mask (sampling.draw_keep_mask) with the selection kernel and with torch.topk;
  (e) what a fresh structure costs its first step, part by part: the GCN normalisation, the first layer's node vectors and
      the decoder's run-sum plan of each order, the plans with graph.PLAN_KERNEL on and off;
  (d) a full train_step on a fresh sub-sample per step (draw + derive + step + release) against the unsampled step on the
      parent graph — the sampled route on a graph object that is only ever sub-sampled — and the sampled step in parts: the sub-sample call, the step on the fresh structure, the same step again.

Once, before timing, the tables of (a) are compared with those of (b) entry for entry.  Each (a) figure is set against its
algorithmic bytes and the arithmetic bound at 8 TB/s.

    python tools/time_edge_filter.py --out profiles/edge_filter.jsonl

On a shared machine run it under its own time limit, e.g. `timeout -k 10 900 python tools/time_edge_filter.py`.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BPS = 8e12


def _event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def _stats(ts):
    ts = sorted(ts)
    return dict(ms=ts[len(ts) // 2], ms_min=ts[0], ms_max=ts[-1], calls=len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--genes", type=int, default=50000, help="genes per genome (config 4: 50000)")
    ap.add_argument("--fraction", type=float, default=0.8)
    ap.add_argument("--no-step", action="store_true", help="skip (d), the train steps")
    ap.add_argument("--out", default=None, help="append the JSON lines here")
    a = ap.parse_args()

    import torch
    import pangnn_amd
    from pangnn_amd import sampling, simulate
    from pangnn_amd.graph import EdgeStructure, build_csr, structure_of
    from pangnn_amd.train import make_optimizer, train_step
    if not torch.cuda.is_available():
        raise SystemExit("time_edge_filter.py measures on the GPU: none found")
    dev = torch.device("cuda")
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    g = simulate.simulate_graph(a.genes, 20, 0.2, 100, 20, seed=0, device=dev)
    n, e = int(g.x.shape[0]), int(g.edge_index.shape[1])
    parent = structure_of(g.edge_index, n, holder=g, name="sim")
    t0 = time.perf_counter()
    parent.by_dst, parent.by_src          # (a) derives the orders its parent holds: both, as filter_edges asks for
    torch.cuda.synchronize()
    emit(dict(what="graph", N=n, E=e, positives=float(g.y.mean()), parent_both_orders_first_build_wall_ms=(time.perf_counter() - t0) * 1e3))
    gen = torch.Generator(device=dev).manual_seed(0)
    keep, kept = sampling.draw_keep_mask(g, a.fraction, generator=gen)

    def route_a():
        return EdgeStructure.filtered(parent, keep, kept, [g.edge_attr, g.y])

    def route_b(ei):
        return build_csr(ei, n, 1, validate=False), build_csr(ei, n, 0, validate=False)

    def compaction():
        return g.edge_index[:, keep], g.edge_attr[keep], g.y[keep]

    # the same tables?  (before any timing; results must not change)
    child, kept_id, outs = route_a()
    d, s = route_b(child.edge_index)
    same = all(torch.equal(x, y) for x, y in ((child._by_dst.rowptr, d.rowptr), (child._by_dst.other, d.other),
                                              (child._by_dst.perm, d.perm), (child._by_src.rowptr, s.rowptr),
                                              (child._by_src.other, s.other), (child._by_src.perm, s.perm)))
    ref = compaction()
    same_list = torch.equal(child.edge_index, ref[0]) and torch.equal(outs[0], ref[1]) and torch.equal(outs[1], ref[2])
    emit(dict(what="agreement", kept=kept, tables_equal=bool(same), edge_list_equal=bool(same_list),
              filter_state=child.filter_state.tolist()))
    if not (same and same_list):
        raise SystemExit("the derived tables differ from build_csr's: nothing below would mean anything")
    child_ei = child.edge_index
    del child, kept_id, outs, d, s, ref

    def draw(kernel):
        sampling.MASK_KERNEL = kernel
        try:
            return sampling.draw_keep_mask(g, a.fraction, generator=gen)
        finally:
            sampling.MASK_KERNEL = mask_default

    mask_default = sampling.MASK_KERNEL
    ta, tb, tbc, tc, tct = [], [], [], [], []
    for it in range(a.warmup + a.steps):
        ms_a, out = _event_ms(route_a)
        del out
        ms_b, out = _event_ms(lambda: route_b(child_ei))
        del out
        ms_bc, out = _event_ms(compaction)
        del out
        ms_c, out = _event_ms(lambda: draw(True))
        del out
        ms_ct, out = _event_ms(lambda: draw(False))
        del out
        if it >= a.warmup:
            ta.append(ms_a), tb.append(ms_b), tbc.append(ms_bc), tc.append(ms_c), tct.append(ms_ct)
    # (a): per order  perm 4 + keep gather 1 + pos write 4 | pos 8 + perm 4 + other 4 + (new_id gather 4 + 8 written) per kept;
    # edge list  keep 1 + new_id write 4 | new_id 8 + (16 + 8 read, 16 + 8 + 4 written) per kept;  rowptr 16 per node
    bytes_a = 2 * (e * (4 + 1 + 4 + 8 + 4 + 4) + kept * 12 + n * 16) + e * (1 + 4 + 8) + kept * 52
    sa, sb = _stats(ta), _stats(tb)
    emit(dict(what="a_filter_both_orders_and_edge_list", **sa, algorithmic_bytes=bytes_a,
              achieved_TBps=bytes_a / sa["ms"] / 1e9, bound_ms_at_8TBps=bytes_a / HBM_BPS * 1e3))
    emit(dict(what="b_build_csr_both_orders", **sb))
    emit(dict(what="b_prime_torch_compaction_of_edge_list", **_stats(tbc)))
    sc, sct = _stats(tc), _stats(tct)
    emit(dict(what="c_draw_mask", route="selection kernel (pangnn_mask_k_smallest_i64)", **sc, default=bool(mask_default)))
    emit(dict(what="c_draw_mask_torch_topk", route="torch.topk + indexed store", **sct, default=not mask_default,
              topk_over_kernel=sct["ms"] / sc["ms"]))
    emit(dict(what="ratio", b_over_a=sb["ms"] / sa["ms"], a_over_b=sa["ms"] / sb["ms"]))
    del child_ei

    # (e) what a fresh structure costs its first step, part by part, on one derived child: the GCN normalisation of the new
    # weights, the first layer's node vectors r / s, and the decoder's run-sum plan of each order — the plans by the kernel
    # (graph.PLAN_KERNEL, pangnn_csr_plan) and by the index-op route, alternated call by call; every cache the part fills is
    # emptied before the call
    def first_step_parts():
        from pangnn_amd import _lib, functional, graph as G
        child, kept_id, outs = route_a()
        ct = int(_lib.load().pangnn_decoder_chunk_tiles_for(child.num_edges))
        w = outs[0]

        def norm_fresh():
            child._norm.clear()
            return child.gcn_norm(w)

        def plan_fresh(which, kernel):
            G.PLAN_KERNEL = kernel
            child._plans.clear()
            try:
                return child.runsum_plan(ct) if which == "runsum" else child.csr_plan(which, ct)
            finally:
                G.PLAN_KERNEL = plan_default

        plan_default = G.PLAN_KERNEL
        whichs = ("dst", "src") + (("runsum",) if child.sorted_by_src() else ())
        t_norm, t_act = [], []
        t_plan = {(wh, k): [] for wh in whichs for k in (True, False)}
        same_plans = True
        for wh in whichs:                    # the same tables?  (before any timing)
            pa, pb = plan_fresh(wh, True), plan_fresh(wh, False)
            same_plans &= all(torch.equal(getattr(pa, f), getattr(pb, f)) and getattr(pa, f).dtype == getattr(pb, f).dtype
                              for f in ("keys", "part_off", "part_rowptr", "last")) and pa.n_parts == pb.n_parts
        emit(dict(what="agreement_plans", chunk_tiles=ct, orders=list(whichs), plans_equal=bool(same_plans)))
        if not same_plans:
            raise SystemExit("the kernel's plans differ from the index-op route's")
        del pa, pb
        for it in range(a.warmup + a.steps):
            ms_n, norm = _event_ms(norm_fresh)
            ms_r, out = _event_ms(lambda: functional._node_actions(g.x, child, norm))
            del out, norm
            ms_p = {}
            for key in t_plan:
                ms_p[key], out = _event_ms(lambda: plan_fresh(*key))
                del out
            if it >= a.warmup:
                t_norm.append(ms_n), t_act.append(ms_r)
                for key in t_plan:
                    t_plan[key].append(ms_p[key])
        emit(dict(what="e_first_step_gcn_norm", **_stats(t_norm)))
        emit(dict(what="e_first_step_node_actions", **_stats(t_act)))
        for wh in whichs:
            sk, st_ = _stats(t_plan[(wh, True)]), _stats(t_plan[(wh, False)])
            emit(dict(what=f"e_first_step_plan_{wh}", route="pangnn_csr_plan", **sk, default=bool(plan_default)))
            emit(dict(what=f"e_first_step_plan_{wh}_index_ops", route="_plan_of_sorted_keys", **st_, default=not plan_default,
                      index_ops_over_kernel=st_["ms"] / sk["ms"]))
        child._norm.clear()
        del child, kept_id, outs, w

    if not a.no_step:
        torch.manual_seed(0)
        model = pangnn_amd.AlternateGCN(dev, None, False, dims=[64, 128], num_nodes=n)
        opt = make_optimizer(model)
        pw = g.class_balance

        def whole():
            return train_step(model, opt, g, g.y, pw)

        # the sampled route runs on a graph object of its own (the same tensors): like dataset.train in the reference's
        # loop it is only ever sub-sampled, never stepped on, so nothing the whole-graph step builds is there to borrow
        from types import SimpleNamespace
        g2 = SimpleNamespace(**{k: v for k, v in g.__dict__.items() if not k.startswith("_")})

        def sampled():
            batch = sampling.sub_sample_graph_edges(g2, dev, a.fraction, generator=gen)
            res = train_step(model, opt, batch, batch.y, pw)
            sampling.release(batch)
            return res

        tw, ts = [], []
        for it in range(a.warmup + a.steps):
            ms_w, out = _event_ms(whole)
            del out
            ms_s, out = _event_ms(sampled)
            del out
            if it >= a.warmup:
                tw.append(ms_w), ts.append(ms_s)
        # where the sampled step's time goes: the sub-sample itself (draw + derive + the Data), the step on the fresh
        # structure (which builds per structure what the whole graph builds once: gcn_norm, the first layer's node vectors,
        # the decoder's run-sum plans of both CSR orders), and the same step repeated on that batch (everything cached)
        t_sub, t_first, t_again = [], [], []
        for it in range(a.warmup + a.steps):
            ms_0, batch = _event_ms(lambda: sampling.sub_sample_graph_edges(g2, dev, a.fraction, generator=gen))
            ms_1, out = _event_ms(lambda: train_step(model, opt, batch, batch.y, pw))
            ms_2, out = _event_ms(lambda: train_step(model, opt, batch, batch.y, pw))
            sampling.release(batch)
            del batch, out
            if it >= a.warmup:
                t_sub.append(ms_0), t_first.append(ms_1), t_again.append(ms_2)
        emit(dict(what="d_parts_sub_sample_call", **_stats(t_sub)))
        emit(dict(what="d_parts_step_on_fresh_structure", **_stats(t_first)))
        emit(dict(what="d_parts_step_repeated_on_that_batch", **_stats(t_again)))
        emit(dict(what="d_train_step_whole_graph", **_stats(tw)))
        emit(dict(what="d_train_step_fresh_sub_sample", **_stats(ts), edges=kept,
                  max_memory_allocated_GB=torch.cuda.max_memory_allocated() / 1e9))
    torch.cuda.empty_cache()          # (d)'s cached blocks: (e) starts from a clean allocator, as (a)-(c) did
    first_step_parts()
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
