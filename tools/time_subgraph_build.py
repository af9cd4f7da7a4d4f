"""Building the per-ortholog-group sub-graph data set on the device at config 4's edge law, 1/50 scale
(`simulate_raw(1000, 20, 0.2, 100, 20, seed=0)`: N = 20 000, 1 000 groups), one process:

  (a) the first 128 groups, all at once: the index-op route of step 3 (`subgraphs.INDUCED_KERNEL = False`, what
      PANGNN_INDUCED_KERNEL=0 selects: the previous `build_subgraphs`) and the kernel route (pangnn_induced_edges_count / _fill),
      alternated call by call after a warm-up of each; per route the synchronised wall time of every call and
      `torch.cuda.max_memory_allocated` over the call's baseline; `torch.equal` of every field of the two data sets;
  (b) all 1 000 groups on the kernel route with `groups_per_pass=128`: time and peak memory;
  (c) with --large-genes n: `simulate_raw(n, 20, 0.2, 100, 20)` whole, kernel route, `groups_per_pass=128`, if the data set
      extrapolated from its first pass's offset tables fits the free device memory three times over.

The index-op route is only run where its estimate fits: expanded entries (`outdeg[node_global].sum()`, host arithmetic on
the kernel route's data set) times 32 bytes and up.  Writes a markdown record (default profiles/subgraph_build.md).

    timeout -k 10 900 python tools/time_subgraph_build.py
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIELDS = ("node_off", "edge_off", "nb_off", "node_global", "edge_index", "neighbour_edge_index", "edge_attr", "y",
          "group_of_graph")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5, help="timed calls per route in (a)")
    ap.add_argument("--subset", type=int, default=128, help="groups of (a)")
    ap.add_argument("--groups-per-pass", type=int, default=128)
    ap.add_argument("--large-genes", type=int, default=0, help="(c): genes per genome of the larger graph; 0 skips it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subgraph_build.md"))
    a = ap.parse_args()

    import torch
    from pangnn_amd import construct, simulate, subgraphs
    if not torch.cuda.is_available():
        raise SystemExit("time_subgraph_build.py measures on the GPU: none found")
    dev = torch.device("cuda")

    def relation(genes):
        raw = simulate.simulate_raw(genes, 20, 0.2, 100, 20, seed=0, device=dev)
        s, d, sc = construct.remove_trivial_cases(raw.src, raw.dst, raw.score, raw.genome_of)
        s, d, w = construct.normalize_sim_scores(s, d, sc, raw.genome_of)
        return raw, s, d, w

    def build(raw, s, d, w, groups=None, **kw):
        nodes = torch.arange(raw.num_nodes, device=dev)
        gid = raw.group_of
        if groups is not None:
            m = gid < groups
            gid, nodes = gid[m], nodes[m]
        return subgraphs.build_subgraphs(raw.num_nodes, s, d, w, gid, nodes, labels_group_of=raw.group_of, **kw)

    def measured(fn):
        """(data set, synchronised wall seconds, peak bytes allocated over the baseline at entry)"""
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        ds = fn()
        torch.cuda.synchronize()
        return ds, time.perf_counter() - t0, torch.cuda.max_memory_allocated() - base

    def expanded_entries(ds, s, n):
        outdeg = torch.bincount(s, minlength=n)
        return int(outdeg[ds.node_global].sum())

    def dataset_bytes(ds):
        return sum(getattr(ds, f).numel() * getattr(ds, f).element_size() for f in FIELDS)

    def med(xs):
        xs = sorted(xs)
        return xs[len(xs) // 2]

    out = ["# Building the sub-graph data set on the device (`tools/time_subgraph_build.py`)", ""]
    raw, s, d, w = relation(1000)
    n, e = raw.num_nodes, int(s.numel())
    outdeg = torch.bincount(s, minlength=n)
    out += [f"`simulate_raw(1000, 20, 0.2, 100, 20, seed=0)` through `remove_trivial_cases` and `normalize_sim_scores`: "
            f"N = {n}, E = {e}, out-degree median {int(outdeg.median())}, max {int(outdeg.max())}; "
            f"device {torch.cuda.get_device_name(0)}.  Wall times end in a device synchronise; peak memory is "
            f"`torch.cuda.max_memory_allocated` over the allocation at the call's entry (the relation itself excluded).", ""]

    # ---- (a)
    kernel_ds, _, _ = measured(lambda: build(raw, s, d, w, groups=a.subset))                 # warm-up of the kernel route
    expanded = expanded_entries(kernel_ds, s, n)
    kept = int(kernel_ds.edge_index.shape[1])
    free = torch.cuda.mem_get_info()[0]
    fits = 64 * expanded < free               # four int64 columns, the search result and masks, and their compacted copies
    out += [f"## (a) the first {a.subset} groups, all at once", "",
            f"{kernel_ds.num_graphs} sub-graphs, {int(kernel_ds.node_global.numel())} rows, {expanded} expanded entries "
            f"(`outdeg[node_global].sum()`), {kept} kept ({kept / max(expanded, 1):.3f}); data set {dataset_bytes(kernel_ds) / 1e6:.1f} MB; "
            f"index-op estimate at 32 B per expanded entry and up: {32 * expanded / 1e6:.0f} MB.", ""]
    if not fits:
        out += [f"The index-op route is not run: its estimate does not fit the {free / 1e9:.1f} GB free.  **not measured**", ""]
    else:
        rec = {"index ops": [], "kernel": []}
        equal = None
        try:
            for i in range(a.calls + 1):                                 # call 0 of each route is its warm-up
                for route, flag in (("index ops", False), ("kernel", True)):
                    subgraphs.INDUCED_KERNEL = flag
                    ds, sec, peak = measured(lambda: build(raw, s, d, w, groups=a.subset))
                    if i:
                        rec[route].append((sec, peak))
                    if not flag and equal is None:
                        equal = {f: bool(torch.equal(getattr(ds, f), getattr(kernel_ds, f))) for f in FIELDS}
                    del ds
        finally:
            subgraphs.INDUCED_KERNEL = True
        out += ["| route of step 3 | wall ms, median (min - max) | peak memory over baseline, MB | calls |", "|---|---|---|---|"]
        for route, label in (("index ops", "index ops (`PANGNN_INDUCED_KERNEL=0`, the previous `build_subgraphs`)"),
                             ("kernel", "`pangnn_induced_edges_count` / `_fill`")):
            ts, ps = [r[0] * 1e3 for r in rec[route]], [r[1] for r in rec[route]]
            out.append(f"| {label} | {med(ts):.1f} ({min(ts):.1f} - {max(ts):.1f}) | {max(ps) / 1e6:.1f} | {len(ts)} |")
        bad = [f for f, ok in equal.items() if not ok]
        out += ["", "`torch.equal` of the two data sets, field by field: " +
                ("**all equal** (" + ", ".join(FIELDS) + ")" if not bad else "**DIFFERENT in " + ", ".join(bad) + "**"), "",
                "Whole `build_subgraphs` calls: the BFS, the node tables, the neighbour edges, the labels and the join are the "
                "same index ops on both routes; only step 3 differs.", ""]
        # step 3 alone on the same node tables
        m = raw.group_of < a.subset
        _, dst_c, _, rowptr = subgraphs._canonical_relation(n, s, d, w)
        t = subgraphs._pass_tables(n, rowptr, dst_c, raw.group_of[m], torch.arange(n, device=dev)[m], a.subset, 1)
        step = {"index ops": [], "kernel": []}
        for i in range(a.calls + 1):
            for route, fn in (("index ops", subgraphs._induced_edges_index_ops), ("kernel", subgraphs._induced_edges_kernel)):
                _, sec, peak = measured(lambda: fn(n, rowptr, dst_c, t))
                if i:
                    step[route].append((sec, peak))
        out += ["Step 3 alone on the same node tables (`_induced_edges_index_ops` / `_induced_edges_kernel`, alternated):", "",
                "| route | wall ms, median (min - max) | peak memory over baseline, MB |", "|---|---|---|"]
        for route in ("index ops", "kernel"):
            ts, ps = [r[0] * 1e3 for r in step[route]], [r[1] for r in step[route]]
            out.append(f"| {route} | {med(ts):.2f} ({min(ts):.2f} - {max(ts):.2f}) | {max(ps) / 1e6:.1f} |")
        out.append("")
        del t, dst_c, rowptr
    del kernel_ds

    # ---- (b)
    measured(lambda: build(raw, s, d, w, groups_per_pass=a.groups_per_pass))                 # warm-up
    ds, sec, peak = measured(lambda: build(raw, s, d, w, groups_per_pass=a.groups_per_pass))
    expanded_all = expanded_entries(ds, s, n)
    out += [f"## (b) all 1 000 groups, kernel route, `groups_per_pass={a.groups_per_pass}`", "",
            f"{ds.num_graphs} sub-graphs, {int(ds.node_global.numel())} rows, {int(ds.edge_index.shape[1])} similarity edges, "
            f"{expanded_all} expanded entries (index-op estimate at 32 B each: {32 * expanded_all / 1e9:.1f} GB); data set "
            f"{dataset_bytes(ds) / 1e6:.1f} MB.", "",
            f"Wall {sec * 1e3:.1f} ms (second call), peak memory over baseline {peak / 1e6:.1f} MB.", ""]
    del ds, raw, s, d, w

    # ---- (c)
    out += ["## (c) a larger graph", ""]
    if not a.large_genes:
        out += ["**not measured** (run with `--large-genes n`)", ""]
    else:
        raw, s, d, w = relation(a.large_genes)
        n = raw.num_nodes
        first, _, _ = measured(lambda: build(raw, s, d, w, groups=a.groups_per_pass))
        per_group = dataset_bytes(first) / max(first.num_graphs, 1)
        estimate = per_group * a.large_genes
        free = torch.cuda.mem_get_info()[0]
        head = (f"`simulate_raw({a.large_genes}, 20, 0.2, 100, 20, seed=0)`: N = {n}, E = {int(s.numel())}; data set extrapolated "
                f"from the offset tables of the first {a.groups_per_pass} groups: {estimate / 1e9:.2f} GB, free {free / 1e9:.1f} GB.")
        del first
        if 3 * estimate > free:
            out += [head, "", "Does not fit three times over: **not measured**", ""]
        else:
            ds, sec, peak = measured(lambda: build(raw, s, d, w, groups_per_pass=a.groups_per_pass))
            expanded_all = expanded_entries(ds, s, n)
            out += [head, "",
                    f"{ds.num_graphs} sub-graphs, {int(ds.node_global.numel())} rows, {int(ds.edge_index.shape[1])} similarity "
                    f"edges, {expanded_all} expanded entries (index-op estimate at 32 B each: {32 * expanded_all / 1e9:.1f} GB); "
                    f"data set {dataset_bytes(ds) / 1e9:.2f} GB.", "",
                    f"Wall {sec:.2f} s (one call, kernel route, `groups_per_pass={a.groups_per_pass}`), peak memory over baseline "
                    f"{peak / 1e9:.2f} GB.", ""]

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out))
    print("\n".join(out))


if __name__ == "__main__":
    main()
