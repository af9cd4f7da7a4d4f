"""Per-ortholog-group sub-graphs — the reference's actual training regime — built for all groups at
once as sort / unique / searchsorted tensor programs (runs on the device the relation lives on).

Restates /root/reference/src/dataset.py:222-322 with src/helper.py:327-433 and
src/preprocessing.py:73-156,264-325:

  for every ortholog group (>= 2 genes):
    1. BFS over the normalised similarity relation, `neighbours` hops from the group's genes
       (get_connected_nodes)                                                       -> "core" nodes
    2. positional neighbours v +- k (k <= neighbours, inside [0, N), ignoring genome ends) of every
       core node are added as extra nodes; neighbour edges (core v, v +- k) in both directions,
       de-duplicated (get_neighbour_graph + remove_duplicate_edges_tuple)
    3. similarity edges = every normalised edge whose two endpoints are in the sub-graph
       (build_edge_index over the sub dict); weights and labels as for the whole graph
    4. the group is dropped if it has no similarity rows, or (real data on a genome subset) fewer
       similarity edges than group members (dataset.py:248,252)

The reference numbers a sub-graph's nodes in CPython string-set iteration order (helper.py:344), which
no other implementation can reproduce; here local ids are: core nodes by ascending gene position, then
the extra neighbour nodes by ascending position.  Parity with the reference-built fixtures is therefore
checked on GLOBAL ids: same node set, same similarity edge set with the same weights and labels, same
neighbour edge set (tests/test_construct.py).

Step 3 on a GPU-resident relation is a count / scan / fill pass of HIP that walks the out-edges in place
(csrc/induced_edges.hip; `induced_edges`), and `groups_per_pass` runs the whole program a slice of the group ids at a
time, so that no temporary grows with all groups at once; either way the data set is the same bit for bit.

The result is one flat "dataset" whose index tensors already carry dataset-wide node numbering, so a
mini-batch of consecutive sub-graphs (PyG `Batch.from_data_list`, pangnn.py:152-153) is a pair of
slices and one subtraction — no per-step collation on the host.
"""
from __future__ import annotations

import ctypes
import os
from types import SimpleNamespace
from typing import NamedTuple, Optional

import torch

from . import _lib
from .graph import (CSR, EdgeStructure, RunPlan, carve, chunk_tiles_for, forget, n_chunks, part_bound, register,
                    structure_key)


class PaddedSpec(NamedTuple):
    """the fixed shapes of a padded batch (SubGraphDataset.padded_spec)"""
    graphs: int
    nodes: int        # one more than the real nodes: the padding's endpoint
    edges: int
    nb_edges: int


# pangnn_batch_order / pangnn_batch_orders of include/pangnn_hip.h, field for field: `rank` is read, the rest written by
# pangnn_collate_subgraphs_padded (part_off / part_rowptr / last_part NULL: no plan for that order)
class BatchOrder(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("rank", "rowptr", "other", "perm", "keys", "part_off", "part_rowptr",
                                               "last_part")]


class BatchOrders(ctypes.Structure):
    _fields_ = [("chunk_edges", ctypes.c_int32), ("sim_dst", BatchOrder), ("sim_src", BatchOrder), ("nb_dst", BatchOrder),
                ("nb_src", BatchOrder)]


# pangnn_union_batch_orders (pangnn_collate_subgraphs_padded_union): the union list's two orders in place of the neighbour list's
class UnionBatchOrders(ctypes.Structure):
    _fields_ = [("chunk_edges", ctypes.c_int32), ("sim_dst", BatchOrder), ("sim_src", BatchOrder), ("union_dst", BatchOrder),
                ("union_src", BatchOrder)]


def _unique_sorted(keys: torch.Tensor) -> torch.Tensor:
    return torch.unique(keys)          # sorted ascending, duplicates dropped


def _isin_sorted(sorted_keys: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    if sorted_keys.numel() == 0:
        return torch.zeros_like(q, dtype=torch.bool)
    pos = torch.searchsorted(sorted_keys, q).clamp_(max=sorted_keys.numel() - 1)
    return sorted_keys[pos] == q


def _expand_by_src(rowptr: torch.Tensor, dst_sorted: torch.Tensor, gid: torch.Tensor, node: torch.Tensor):
    """all (gid, t, edge position) for edges node -> t of the src-grouped relation"""
    beg, end = rowptr[node], rowptr[node + 1]
    cnt = end - beg
    total = int(cnt.sum())
    rep = torch.repeat_interleave(torch.arange(node.numel(), device=node.device), cnt)
    off = torch.arange(total, device=node.device) - torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt)
    epos = beg[rep] + off
    return gid[rep], dst_sorted[epos], epos, rep


def _lookup(lk_sorted: torch.Tensor, lk_local: torch.Tensor, n: int, g: torch.Tensor, v: torch.Tensor):
    """(found, local id) of node v in group g, from the ascending (group * n + node) keys of every group's nodes"""
    q = g * n + v
    if lk_sorted.numel() == 0:
        return torch.zeros_like(q, dtype=torch.bool), torch.zeros_like(q)
    pos = torch.searchsorted(lk_sorted, q).clamp_(max=lk_sorted.numel() - 1)
    return lk_sorted[pos] == q, lk_local[pos]


# step 3 of build_subgraphs on a GPU-resident relation is a count / scan / fill pass of HIP (pangnn_induced_edges_count /
# _fill: nothing of the size of the expanded out-edges is stored); False, or PANGNN_INDUCED_KERNEL=0 in the environment: the
# index ops a CPU-resident relation always takes (_induced_edges_index_ops, what tests/test_induced_edges.py compares the
# kernel with)
INDUCED_KERNEL = os.environ.get("PANGNN_INDUCED_KERNEL", "1") != "0"


def _induced_edges_index_ops(n: int, rowptr: torch.Tensor, dst: torch.Tensor, t):
    """The definition of step 3: every out-edge of every (group, node) row of the tables `t` (_pass_tables) whose target is a
    node of the same group -> (group, edge position, source local id, target local id), rows in row order, positions
    ascending inside a row.  Expands ALL out-edges of all rows (four int64 columns, a search result and masks) before it
    drops those that leave the group."""
    eg, et, epos, rep = _expand_by_src(rowptr, dst, t.all_g, t.all_n)
    inside, t_local = _lookup(t.lk_sorted, t.lk_local, n, eg, et)
    return eg[inside], epos[inside], t.local[rep][inside], t_local[inside]


def _induced_edges_kernel(n: int, rowptr: torch.Tensor, dst: torch.Tensor, t):
    """the same four columns from pangnn_induced_edges_count / _fill (csrc/induced_edges.hip): temporaries of a few words per
    ROW, one host read-back (the total, which sizes the outputs)"""
    dev = dst.device
    rows, groups, e = int(t.all_n.numel()), int(t.node_off_g.numel()) - 1, int(dst.numel())
    if rows == 0:
        return tuple(torch.empty(0, dtype=torch.int64, device=dev) for _ in range(4))
    lib = _lib.load()
    # each group's node ids in ascending order: lk_sorted is ordered by (group, node) and all_g by group, with the same counts
    sorted_node = t.lk_sorted - t.all_g * n
    tables = (rowptr, dst, t.all_n, t.node_off_g, sorted_node, t.lk_local)
    if any(x.dtype != torch.int64 or not x.is_contiguous() or x.device != dev for x in tables):
        raise ValueError("the induced-edge pass takes contiguous int64 tables on the relation's device")
    with _lib.device_guard(dev):
        need = lib.pangnn_induced_edges_scratch_bytes(rows)
        if need <= 0:
            raise _lib.PangnnHipError("pangnn_induced_edges_scratch_bytes failed")
        row_off = torch.empty(rows + 1, dtype=torch.int64, device=dev)
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        head = (rowptr.data_ptr(), dst.data_ptr() if e else None, n, e, t.all_n.data_ptr(), rows, t.node_off_g.data_ptr(),
                groups, sorted_node.data_ptr(), t.lk_local.data_ptr())
        _lib.check(lib.pangnn_induced_edges_count(*head, row_off.data_ptr(), scratch.data_ptr(), need, _lib.stream_ptr()),
                   "pangnn_induced_edges_count")
        total = int(row_off[-1])
        del scratch
        out = torch.empty(3, total, dtype=torch.int64, device=dev)
        _lib.check(lib.pangnn_induced_edges_fill(*head, row_off.data_ptr(), total, _lib.ptr(out[0]) if total else None,
                                                 _lib.ptr(out[1]) if total else None, _lib.ptr(out[2]) if total else None,
                                                 _lib.stream_ptr()), "pangnn_induced_edges_fill")
    per_group = row_off[t.node_off_g[1:]] - row_off[t.node_off_g[:-1]]
    eg = torch.repeat_interleave(torch.arange(groups, device=dev), per_group, output_size=total)
    return eg, out[2], out[0], out[1]


def induced_edges(n: int, rowptr: torch.Tensor, dst: torch.Tensor, t):
    """step 3 of build_subgraphs over the node tables `t` of a pass: (group, edge position, source local id, target local id)
    of every similarity edge with both endpoints inside a sub-graph"""
    if dst.is_cuda and INDUCED_KERNEL:
        return _induced_edges_kernel(n, rowptr, dst, t)
    return _induced_edges_index_ops(n, rowptr, dst, t)


def _canonical_relation(n: int, src, dst, weight):
    """the relation without self hits and out-of-range ids, in (src, dst) order, and its by-source row pointer"""
    ok = (src != dst) & (src >= 0) & (dst >= 0) & (src < n) & (dst < n)
    src, dst, weight = src[ok], dst[ok], weight[ok]
    order = torch.argsort(src * n + dst, stable=True)                 # canonical (src, dst) order
    src, dst, weight = src[order], dst[order], weight[order]
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=src.device)
    rowptr[1:] = torch.cumsum(torch.bincount(src, minlength=n), 0)
    return src, dst, weight, rowptr


def _pass_tables(n: int, rowptr: torch.Tensor, dst: torch.Tensor, gid: torch.Tensor, mem: torch.Tensor, ngroups: int,
                 neighbours: int):
    """steps 1 and 2 for the groups 0..ngroups-1 given by their (gid, mem) member rows: every sub-graph's node list in
    (group, local id) order, the (group, node) -> local id lookup table, and the positional neighbour pairs"""
    dev = dst.device
    # 1. BFS (get_connected_nodes): keys = gid * n + node
    core = _unique_sorted(gid * n + mem)
    frontier = core
    for _ in range(int(neighbours)):
        fg, fn = torch.div(frontier, n, rounding_mode="floor"), frontier % n
        eg, et, _, _ = _expand_by_src(rowptr, dst, fg, fn)
        cand = _unique_sorted(eg * n + et)
        new = cand[~_isin_sorted(core, cand)]
        if new.numel() == 0:
            break
        core = _unique_sorted(torch.cat([core, new]))
        frontier = new
    cg, cn = torch.div(core, n, rounding_mode="floor"), core % n

    # 2. positional neighbours of core nodes (get_neighbour_graph)
    ks = torch.tensor([k for k in range(-neighbours, neighbours + 1) if k != 0], dtype=torch.int64, device=dev)
    nb_g = cg.repeat_interleave(ks.numel())
    nb_a = cn.repeat_interleave(ks.numel())
    nb_b = nb_a + ks.repeat(cn.numel())
    inr = (nb_b >= 0) & (nb_b < n)
    nb_g, nb_a, nb_b = nb_g[inr], nb_a[inr], nb_b[inr]
    extra = _unique_sorted(nb_g * n + nb_b)
    extra = extra[~_isin_sorted(core, extra)]
    xg, xn = torch.div(extra, n, rounding_mode="floor"), extra % n

    # node list per group: core (ascending) then extra (ascending)
    all_g = torch.cat([cg, xg])
    all_n = torch.cat([cn, xn])
    flag = torch.cat([torch.zeros_like(cg), torch.ones_like(xg)])
    o = torch.argsort((all_g * 2 + flag) * n + all_n)
    all_g, all_n = all_g[o], all_n[o]
    nodes_per_group = torch.bincount(all_g, minlength=ngroups)
    node_off_g = torch.zeros(ngroups + 1, dtype=torch.int64, device=dev)
    node_off_g[1:] = torch.cumsum(nodes_per_group, 0)
    local = torch.arange(all_g.numel(), device=dev) - node_off_g[all_g]
    # lookup (gid, node) -> local id
    lk = all_g * n + all_n
    lo = torch.argsort(lk)
    lk_sorted, lk_local = lk[lo], local[lo]
    return SimpleNamespace(all_g=all_g, all_n=all_n, local=local, node_off_g=node_off_g, nodes_per_group=nodes_per_group,
                           lk_sorted=lk_sorted, lk_local=lk_local, nb_g=nb_g, nb_a=nb_a, nb_b=nb_b)


def _build_pass(n: int, rel, gid: torch.Tensor, mem: torch.Tensor, gsize: torch.Tensor, neighbours: int, label_of,
                require_edges_ge_members: bool):
    """steps 1 to 4 for the groups 0..G-1 of one pass (G = gsize.numel(); `rel`: _canonical_relation): groups do not interact,
    so a pass is the whole program on a slice of the group ids.  Returns the kept groups (`kept`, pass-local ids) renumbered
    0..k-1 in the `*_g` columns, with LOCAL node ids in the edge columns."""
    src, dst, weight, rowptr = rel
    dev = dst.device
    ngroups = int(gsize.numel())
    t = _pass_tables(n, rowptr, dst, gid, mem, ngroups, neighbours)
    all_g, all_n, nodes_per_group = t.all_g, t.all_n, t.nodes_per_group

    # 3. similarity edges with both endpoints inside the sub-graph (build_edge_index on the sub dict)
    eg, epos, s_local, t_local = induced_edges(n, rowptr, dst, t)
    e_w = weight[epos].to(torch.float32)
    y = label_of(src[epos], dst[epos])
    edges_per_group = torch.bincount(eg, minlength=ngroups)

    # neighbour edges (core v, v +- k), both directions, de-duplicated
    nb_g = t.nb_g
    _, a_local = _lookup(t.lk_sorted, t.lk_local, n, nb_g, t.nb_a)
    _, b_local = _lookup(t.lk_sorted, t.lk_local, n, nb_g, t.nb_b)
    big = int(nodes_per_group.max().item()) + 1 if ngroups else 1
    und = _unique_sorted(torch.cat([(nb_g * big + a_local) * big + b_local, (nb_g * big + b_local) * big + a_local]))
    ng = torch.div(und, big * big, rounding_mode="floor")
    na = torch.div(und, big, rounding_mode="floor") % big
    nbb = und % big
    nb_per_group = torch.bincount(ng, minlength=ngroups)

    # 4. drop groups (dataset.py:230,235,248,252)
    has_rows = (rowptr[all_n + 1] - rowptr[all_n]) > 0
    sim_rows = torch.zeros(ngroups, dtype=torch.int64, device=dev).index_add_(0, all_g, has_rows.long())
    keep_g = (gsize > 1) & (nodes_per_group > 0) & (sim_rows > 0)
    if require_edges_ge_members:
        keep_g &= edges_per_group >= gsize
    new_gid = torch.cumsum(keep_g.long(), 0) - 1

    def compact(g, *cols):
        m = keep_g[g]
        return (new_gid[g[m]],) + tuple(c[m] for c in cols)

    all_g2, all_n2 = compact(all_g, all_n)
    eg2, s2, t2, w2, y2 = compact(eg, s_local, t_local, e_w, y)
    ng2, na2, nb2 = compact(ng, na, nbb)
    return SimpleNamespace(kept=torch.nonzero(keep_g).view(-1), node_g=all_g2, node_global=all_n2, edge_g=eg2, s=s2, t=t2,
                           w=w2, y=y2, nb_g=ng2, nb_a=na2, nb_b=nb2)


def build_subgraphs(num_nodes: int, src, dst, weight, group_id: torch.Tensor, group_member: torch.Tensor,
                    neighbours: int = 1, labels_group_of: Optional[torch.Tensor] = None, pair_src=None,
                    pair_dst=None, require_edges_ge_members: bool = False, groups_per_pass: Optional[int] = None):
    """(src, dst, weight): normalised similarity relation (self hits already removed).
    (group_id, group_member): the ortholog groups as parallel arrays (group ids 0..G-1, gene node ids).
    Labels as in construct.whole_graph: `labels_group_of[node]` or explicit (pair_src, pair_dst).
    `groups_per_pass`: None builds every group at once; an integer k builds k consecutive group ids at a time and joins the
    passes — the same data set bit for bit (groups do not interact), with the per-group temporaries (BFS expansion, node and
    neighbour tables, lookup keys) bounded by what k groups need instead of what all of them need."""
    dev = src.device
    n = int(num_nodes)
    if groups_per_pass is not None and int(groups_per_pass) < 1:
        raise ValueError(f"groups_per_pass must be a positive number of groups or None, not {groups_per_pass!r}")
    rel = _canonical_relation(n, src, dst, weight)

    ngroups = int(group_id.max().item()) + 1 if group_id.numel() else 0
    gsize = torch.bincount(group_id, minlength=ngroups)
    keep_m = gsize[group_id] > 1                                       # dataset.py:230
    gid, mem = group_id[keep_m], group_member[keep_m]

    if labels_group_of is not None:
        def label_of(s_glob, t_glob):
            a, b = labels_group_of[s_glob], labels_group_of[t_glob]
            return ((a == b) & (a >= 0)).to(torch.float32)
    else:
        pair_keys = torch.cat([pair_src * n + pair_dst, pair_dst * n + pair_src]).unique()

        def label_of(s_glob, t_glob):
            return _isin_sorted(pair_keys, s_glob * n + t_glob).to(torch.float32)

    if groups_per_pass is None or ngroups == 0:
        parts = [_build_pass(n, rel, gid, mem, gsize, int(neighbours), label_of, require_edges_ge_members)]
    else:
        parts, k, n_kept = [], int(groups_per_pass), 0
        for g0 in range(0, ngroups, k):
            g1 = min(g0 + k, ngroups)
            m = (gid >= g0) & (gid < g1)
            p = _build_pass(n, rel, gid[m] - g0, mem[m], gsize[g0:g1], int(neighbours), label_of, require_edges_ge_members)
            # join: group ids back to the caller's, sub-graph numbers running on across the passes
            p.kept, p.node_g, p.edge_g, p.nb_g = p.kept + g0, p.node_g + n_kept, p.edge_g + n_kept, p.nb_g + n_kept
            n_kept += int(p.kept.numel())
            parts.append(p)

    def joined(name):
        return getattr(parts[0], name) if len(parts) == 1 else torch.cat([getattr(p, name) for p in parts])

    kept = joined("kept")
    n_sub = int(kept.numel())
    all_g2, all_n2 = joined("node_g"), joined("node_global")
    eg2, s2, t2, w2, y2 = (joined(c) for c in ("edge_g", "s", "t", "w", "y"))
    ng2, na2, nb2 = joined("nb_g"), joined("nb_a"), joined("nb_b")
    del parts
    node_off = torch.zeros(n_sub + 1, dtype=torch.int64, device=dev)
    node_off[1:] = torch.cumsum(torch.bincount(all_g2, minlength=n_sub), 0)
    edge_off = torch.zeros(n_sub + 1, dtype=torch.int64, device=dev)
    edge_off[1:] = torch.cumsum(torch.bincount(eg2, minlength=n_sub), 0)
    nb_off = torch.zeros(n_sub + 1, dtype=torch.int64, device=dev)
    nb_off[1:] = torch.cumsum(torch.bincount(ng2, minlength=n_sub), 0)
    # dataset-wide node numbering: local id + first node of the sub-graph
    return SubGraphDataset(
        num_graphs=n_sub, node_off=node_off, edge_off=edge_off, nb_off=nb_off, node_global=all_n2,
        edge_index=torch.stack([s2 + node_off[eg2], t2 + node_off[eg2]]), edge_attr=w2, y=y2,
        neighbour_edge_index=torch.stack([na2 + node_off[ng2], nb2 + node_off[ng2]]),
        group_of_graph=kept)


# batches of a GPU-resident data set are collated by one HIP launch (pangnn_collate_subgraphs); False: the index ops
# a CPU-resident data set always uses (what tests/test_construct.py compares the kernel with)
COLLATE_KERNEL = True


class SubGraphDataset:
    """Flat storage of all sub-graphs; `batch(i0, i1)` is the disjoint union of sub-graphs [i0, i1)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __len__(self):
        return self.num_graphs

    @staticmethod
    def _default_layout(i, gr):
        """sub-graph `i` of a list in the layout the flat data set stores.  A --union_edge_weights sub-graph (src/dataset.py:
        287-302: `union_edge_index` = [neighbour | similarity] edges, `edge_attr` = [1 per neighbour edge | similarity
        weights], no `neighbour_edge_index`) is split back into its two lists; anything else is returned as it is."""
        if not hasattr(gr, "union_edge_index") or hasattr(gr, "neighbour_edge_index"):
            return gr
        un, ei, w = gr.union_edge_index, gr.edge_index, gr.edge_attr
        if un.dim() != 2 or un.shape[0] != 2 or ei.dim() != 2 or ei.shape[0] != 2:
            raise ValueError(f"sub-graph {i}: union_edge_index / edge_index must be [2, E]")
        u, e = int(un.shape[1]), int(ei.shape[1])
        if u < e or w.shape[0] != u:
            raise ValueError(f"sub-graph {i}: a union sub-graph needs one weight per union edge and its similarity edges "
                             f"inside the union ({u} union edges, {e} similarity edges, {w.shape[0]} weights)")
        if not torch.equal(un[:, u - e:], ei):
            raise ValueError(f"sub-graph {i}: the last {e} union edges are not edge_index")
        if not bool((w[:u - e] == 1).all()):
            raise ValueError(f"sub-graph {i}: the weights of the {u - e} neighbour edges in front are not all 1")
        return SimpleNamespace(x=gr.x, edge_index=ei, neighbour_edge_index=un[:, :u - e], edge_attr=w[u - e:], y=gr.y)

    @classmethod
    def from_data_list(cls, graphs, device=None) -> "SubGraphDataset":
        """The flat data set of a LIST of per-group sub-graphs as the reference builds them (`UnionGraphDataset`'s
        `generate_sub_graphs`, src/dataset.py:280-310: PyG `Data` objects with `x [n, 1]`, `edge_index [2, e]` and
        `neighbour_edge_index [2, b]` in LOCAL ids, `edge_attr [e]`, `y [e]`; any object with those attributes) — so that
        the reference's own sub-graphs train through `batch()`, `train.GraphedTrainStep` and `train.ReplayedFreshStep`
        (one captured HIP graph for every shuffled mini-batch) without going through this package's graph construction.
        Edge order inside a sub-graph is kept (PyG's `Batch.from_data_list` keeps it too: logits come back in that order);
        one host -> device copy per tensor kind, once per data set.
        --union_edge_weights sub-graphs (`union_edge_index`, no `neighbour_edge_index`) are accepted too and stored in the
        same default layout (`_default_layout`): union batches are derived at collation, `batch(..., union=True)`."""
        graphs = list(graphs)
        if not graphs:
            raise ValueError("from_data_list needs at least one sub-graph")
        if device is None:
            device = graphs[0].edge_index.device
        graphs = [cls._default_layout(i, gr) for i, gr in enumerate(graphs)]
        for i, gr in enumerate(graphs):
            n = int(gr.x.shape[0])
            ei, nb = gr.edge_index, gr.neighbour_edge_index
            if ei.dim() != 2 or ei.shape[0] != 2 or nb.dim() != 2 or nb.shape[0] != 2:
                raise ValueError(f"sub-graph {i}: edge_index / neighbour_edge_index must be [2, E]")
            if gr.edge_attr.shape[0] != ei.shape[1] or gr.y.shape[0] != ei.shape[1]:
                # (a longer edge_attr is the union layout, whose similarity weights are the LAST e entries: never slice it)
                raise ValueError(f"sub-graph {i}: edge_attr has {gr.edge_attr.shape[0]} and y {gr.y.shape[0]} entries for "
                                 f"{ei.shape[1]} similarity edges")
            for name, t in (("edge_index", ei), ("neighbour_edge_index", nb)):
                if t.numel() and (int(t.min()) < 0 or int(t.max()) >= n):
                    raise ValueError(f"sub-graph {i}: {name} holds ids outside [0, {n})")

        def offsets(counts):
            off = torch.zeros(len(counts) + 1, dtype=torch.int64)
            off[1:] = torch.cumsum(torch.tensor(counts, dtype=torch.int64), 0)
            return off

        node_off = offsets([int(gr.x.shape[0]) for gr in graphs])
        edge_off = offsets([int(gr.edge_index.shape[1]) for gr in graphs])
        nb_off = offsets([int(gr.neighbour_edge_index.shape[1]) for gr in graphs])
        ei = torch.cat([gr.edge_index.to("cpu", torch.int64) + int(node_off[i]) for i, gr in enumerate(graphs)], dim=1)
        nb = torch.cat([gr.neighbour_edge_index.to("cpu", torch.int64) + int(node_off[i]) for i, gr in enumerate(graphs)], dim=1)
        w = torch.cat([gr.edge_attr.to("cpu", torch.float32) for gr in graphs])
        y = torch.cat([gr.y.to("cpu", torch.float32) for gr in graphs])
        dev = torch.device(device)
        return cls(num_graphs=len(graphs), node_off=node_off.to(dev), edge_off=edge_off.to(dev), nb_off=nb_off.to(dev),
                   node_global=None, edge_index=ei.contiguous().to(dev), edge_attr=w.to(dev), y=y.to(dev),
                   neighbour_edge_index=nb.contiguous().to(dev), group_of_graph=None)

    def _host(self):
        """host copies of the three offset tables and the order property of the flat edge list, read back ONCE: collating a
        batch then needs no device -> host synchronisation"""
        h = self.__dict__.get("_host_cache")
        if h is None:
            src = self.edge_index[0]
            h = self._host_cache = SimpleNamespace(
                node=self.node_off.tolist(), edge=self.edge_off.tolist(), nb=self.nb_off.tolist(),
                sorted_by_src=bool((src[1:] >= src[:-1]).all()) if src.numel() > 1 else True)
        return h

    def batch(self, i0: int, i1: int, union: bool = False):
        """`union`: the --union_edge_weights layout (dataset.py:373-381) — `union_edge_index` = [the batch's similarity edges |
        its neighbour edges], `edge_attr` = [similarity weights | ones] (so `edge_attr[:E]` are the weights of `edge_index`),
        no `neighbour_edge_index`; `edge_index`, `y` and everything else as in the default layout."""
        i1 = min(i1, self.num_graphs)
        h = self._host()
        n0, n1 = h.node[i0], h.node[i1]
        e0, e1 = h.edge[i0], h.edge[i1]
        b0, b1 = h.nb[i0], h.nb[i1]
        dev = self.edge_index.device
        ptr = self.node_off[i0:i1 + 1] - n0
        if union:
            return self._union_batch(i0, i1, n0, n1, e0, e1, b0, b1, ptr)
        # what this producer knows about the batch (graph.EdgeStructure hints): ids are local and in range by
        # construction; a slice of a source-sorted flat list shifted by a constant is source-sorted
        hints = {"sim": {"valid_ids": True, "sorted_by_src": h.sorted_by_src}, "nb": {"valid_ids": True}}
        if dev.type == "cuda" and COLLATE_KERNEL:
            # one launch (pangnn_collate_subgraphs) instead of seven index ops: the step around it is launch-bound
            lib = _lib.load()
            n, e, b, g = n1 - n0, e1 - e0, b1 - b0, i1 - i0
            buf = torch.empty(2 * e + 2 * b + (g + 1) + n, dtype=torch.int64, device=dev)
            x = torch.empty(n, 1, dtype=torch.float32, device=dev)
            ei, nb = buf[:2 * e].view(2, e), buf[2 * e:2 * e + 2 * b].view(2, b)
            ptr, bid = buf[2 * e + 2 * b:2 * e + 2 * b + g + 1], buf[2 * e + 2 * b + g + 1:]
            src_ei, src_nb = self.edge_index, self.neighbour_edge_index
            if not (src_ei.is_contiguous() and src_nb.is_contiguous() and self.node_off.is_contiguous()):
                raise ValueError("SubGraphDataset tensors must be contiguous")
            with _lib.device_guard(dev):
                _lib.check(lib.pangnn_collate_subgraphs(
                    src_ei.data_ptr(), src_ei.shape[1], e0, e, src_nb.data_ptr(), src_nb.shape[1], b0, b,
                    self.node_off.data_ptr() + 8 * i0, g, n0, n, _lib.ptr(ei), _lib.ptr(nb), ptr.data_ptr(),
                    _lib.ptr(bid), _lib.ptr(x), _lib.stream_ptr()), "pangnn_collate_subgraphs")
            return SimpleNamespace(_pangnn_hints=hints, x=x, edge_index=ei, edge_attr=self.edge_attr[e0:e1],
                                   y=self.y[e0:e1], neighbour_edge_index=nb, ptr=ptr, num_graphs=g, batch=bid)
        return SimpleNamespace(
            _pangnn_hints=hints,
            x=torch.ones(n1 - n0, 1, dtype=torch.float32, device=dev),
            edge_index=(self.edge_index[:, e0:e1] - n0).contiguous(),
            edge_attr=self.edge_attr[e0:e1].contiguous(), y=self.y[e0:e1].contiguous(),
            neighbour_edge_index=(self.neighbour_edge_index[:, b0:b1] - n0).contiguous(),
            ptr=ptr, num_graphs=i1 - i0,
            # graph id of every node: position of the node among the graphs' end offsets (no data-dependent output size)
            batch=torch.searchsorted(ptr[1:].contiguous(), torch.arange(n1 - n0, device=dev), right=True))

    def _union_batch(self, i0, i1, n0, n1, e0, e1, b0, b1, ptr):
        """`batch(i0, i1, union=True)`: one launch on a device-resident set (pangnn_collate_subgraphs_union), index ops on a
        CPU-resident one"""
        dev = self.edge_index.device
        n, e, b, g = n1 - n0, e1 - e0, b1 - b0, i1 - i0
        hints = {"sim": {"valid_ids": True, "sorted_by_src": self._host().sorted_by_src},
                 "union": {"valid_ids": True, "band_width": 0}}
        if dev.type == "cuda" and COLLATE_KERNEL:
            lib = _lib.load()
            buf = torch.empty(2 * e + 2 * (e + b) + (g + 1) + n, dtype=torch.int64, device=dev)
            x = torch.empty(n, 1, dtype=torch.float32, device=dev)
            w = torch.empty(e + b, dtype=torch.float32, device=dev)
            ei, un = buf[:2 * e].view(2, e), buf[2 * e:4 * e + 2 * b].view(2, e + b)
            ptr, bid = buf[4 * e + 2 * b:4 * e + 2 * b + g + 1], buf[4 * e + 2 * b + g + 1:]
            src_ei, src_nb = self.edge_index, self.neighbour_edge_index
            if not (src_ei.is_contiguous() and src_nb.is_contiguous() and self.node_off.is_contiguous()
                    and self.edge_attr.is_contiguous()):
                raise ValueError("SubGraphDataset tensors must be contiguous")
            if self.edge_attr.dtype != torch.float32:
                raise ValueError("edge_attr must be float32")
            with _lib.device_guard(dev):
                _lib.check(lib.pangnn_collate_subgraphs_union(
                    src_ei.data_ptr(), src_ei.shape[1], e0, e, src_nb.data_ptr(), src_nb.shape[1], b0, b,
                    self.edge_attr.data_ptr(), self.node_off.data_ptr() + 8 * i0, g, n0, n, _lib.ptr(ei), _lib.ptr(un),
                    _lib.ptr(w), ptr.data_ptr(), _lib.ptr(bid), _lib.ptr(x), _lib.stream_ptr()),
                    "pangnn_collate_subgraphs_union")
            return SimpleNamespace(_pangnn_hints=hints, x=x, edge_index=ei, edge_attr=w, y=self.y[e0:e1],
                                   union_edge_index=un, ptr=ptr, num_graphs=g, batch=bid)
        ei = (self.edge_index[:, e0:e1] - n0).contiguous()
        return SimpleNamespace(
            _pangnn_hints=hints, x=torch.ones(n, 1, dtype=torch.float32, device=dev), edge_index=ei,
            edge_attr=torch.cat([self.edge_attr[e0:e1], torch.ones(b, dtype=self.edge_attr.dtype, device=dev)]),
            y=self.y[e0:e1].contiguous(),
            union_edge_index=torch.cat([ei, self.neighbour_edge_index[:, b0:b1] - n0], dim=1),
            ptr=ptr, num_graphs=g,
            batch=torch.searchsorted(ptr[1:].contiguous(), torch.arange(n, device=dev), right=True))

    def graph(self, i: int):
        return self.batch(i, i + 1)

    # ---- fixed-shape batches (train.ReplayedFreshStep): one set of buffers, one captured HIP graph, every mini-batch
    def padded_spec(self, batch_size: int = 32, graphs=None, slack: Optional[float] = None):
        """PaddedSpec (max_graphs, max_nodes, max_edges, max_nb): shapes that hold the disjoint union of ANY `batch_size` sub-graphs out
        of `graphs` (default: all) — the sums of the `batch_size` largest counts, plus the one node that is never real
        (the padding's endpoint).  `slack`: instead `slack` times the MEAN batch (capped by the worst case) — what a
        shuffled batch needs in practice (the sum of 32 draws concentrates around its mean); a batch that does not fit is
        refused by `set_graph_ids`, and the caller keeps a worst-case set of buffers for it (train.ReplayedFreshStep).
        Host arithmetic on the offset tables, which are read back once per data set."""
        h = self._host()
        idx = list(range(self.num_graphs)) if graphs is None else [int(i) for i in graphs]
        bs = int(batch_size)

        def cap(off):
            sizes = sorted((off[i + 1] - off[i] for i in idx), reverse=True)
            worst = sum(sizes[:bs])
            if slack is None or not sizes:
                return worst
            return min(worst, int(float(slack) * bs * sum(sizes) / len(sizes)) + 1)
        return PaddedSpec(bs, cap(h.node) + 1, max(cap(h.edge), 1), max(cap(h.nb), 1))

    def _counts(self, ids):
        """(nodes, edges, neighbour edges) of the disjoint union of the sub-graphs `ids` (host arithmetic)"""
        h = self._host()
        return tuple(sum(off[i + 1] - off[i] for i in ids) for off in (h.node, h.edge, h.nb))

    def fits(self, spec, ids) -> bool:
        """whether the disjoint union of the sub-graphs `ids` fits the padded shapes `spec` (host arithmetic)"""
        spec, ids = PaddedSpec(*spec), [int(i) for i in ids]
        n, e, b = self._counts(ids)
        return len(ids) <= spec.graphs and n < spec.nodes and e <= spec.edges and b <= spec.nb_edges

    def structure_index(self, union: bool = False):
        """per flat edge of both lists: its position inside its own sub-graph in the by-target and in the by-source order
        (int32; stable — equal keys keep list order).  A property of the data set, computed once with two stable sorts per
        list; with it a batch's CSR orders are written without any sort (pangnn_collate_subgraphs_padded, `orders`).
        `union`: also `union_dst` / `union_src` [E + B] — entry t for flat similarity edge t, entry E + t for flat neighbour
        edge t: the edge's position in either order of its sub-graph's union list (pangnn_collate_subgraphs_padded_union)."""
        idx = self.__dict__.get("_structure_index")
        if idx is None:
            dev = self.edge_index.device
            n_total = int(self._host().node[-1])

            def ranks(ei, off):
                cnt = off[1:] - off[:-1]
                gid = torch.repeat_interleave(torch.arange(self.num_graphs, device=dev), cnt)
                first = off[:-1][gid]
                pos = torch.arange(ei.shape[1], device=dev)
                out = []
                for row in (1, 0):            # by target, by source: node ids are data-set wide, so the id alone orders
                    order = torch.argsort(ei[row], stable=True)      # sub-graph after sub-graph, row after row
                    r = torch.empty_like(pos)
                    r[order] = pos
                    out.append((r - first).to(torch.int32).contiguous())
                return out
            assert n_total < 2 ** 31
            sd, ss = ranks(self.edge_index, self.edge_off)
            nd, ns = ranks(self.neighbour_edge_index, self.nb_off)
            idx = self._structure_index = SimpleNamespace(sim_dst=sd, sim_src=ss, nb_dst=nd, nb_src=ns)
        if union and not hasattr(idx, "union_dst"):
            # the same for the --union_edge_weights list of a sub-graph, [its similarity edges | its neighbour edges]: one
            # stable sort per order over [flat similarity | flat neighbour] keyed by the node id — at equal keys similarity
            # edges come first, each kind in list order: the tie order of a stable sort of a batch's union list
            dev = self.edge_index.device
            both = torch.cat([self.edge_index, self.neighbour_edge_index], dim=1)
            cnt_e, cnt_b = self.edge_off[1:] - self.edge_off[:-1], self.nb_off[1:] - self.nb_off[:-1]
            gids = torch.arange(self.num_graphs, device=dev)
            gid = torch.cat([torch.repeat_interleave(gids, cnt_e), torch.repeat_interleave(gids, cnt_b)])
            first = (self.edge_off[:-1] + self.nb_off[:-1])[gid]
            pos = torch.arange(both.shape[1], device=dev)
            for name, row in (("union_dst", 1), ("union_src", 0)):
                order = torch.argsort(both[row], stable=True)
                r = torch.empty_like(pos)
                r[order] = pos
                setattr(idx, name, (r - first).to(torch.int32).contiguous())
        return idx

    def padded_buffers(self, spec, orders: bool = True, union: bool = False):
        """the fixed buffers of a padded batch + the device list of sub-graph ids it is collated from.  `orders`: also the
        buffers of both CSR orders (and the decoder's run-sum plans) of both edge lists, written by the collation itself —
        no per-batch sort (`structure_index`); False, or shapes beyond the small-structure limits: built per batch by
        graph.EdgeStructure as for any other batch.
        Layout facts a consumer of the PyG-like fields needs: `ptr` has spec.graphs + 1 entries (entries past the real graphs
        repeat the real node count); `batch` gives a PADDED node the id of a dedicated padding segment — the number of real
        graphs of the current batch, which for a full batch equals spec.graphs — so per-graph pooling over `batch` must be sized
        `num_graphs` = spec.graphs + 1 (what this buffer reports), and its last used row is the padding's.
        `union`: the --union_edge_weights layout — no `neighbour_edge_index` but `union_edge_index` [2, U], U = spec.edges +
        spec.nb_edges: [real similarity edges | real neighbour edges | padding of the same kind], and `edge_attr` [U] = [real
        weights | ones], whose first spec.edges entries are the default layout's.  Its orders are those of the similarity list
        (with plans) and of the union list (none: the decoder runs on the similarity list); they are collation-written up to
        U = 32768 (pangnn_collate_union_orders_supported)."""
        spec = PaddedSpec(*spec)
        g, n, e, b = spec
        dev = self.edge_index.device
        u = e + b if union else b                         # columns of the second list: the union list / the neighbour list
        ei, nb, ptr, bid, live, ids = carve(torch.int64, dev, [2 * e, 2 * u, g + 1, n, 8, g])
        ids.fill_(-1)
        live.zero_()
        w, y, x = carve(torch.float32, dev, [u if union else e, e, n])
        hints = {"sim": {"valid_ids": True, "sorted_by_src": self._host().sorted_by_src, "band_width": 0},
                 "union" if union else "nb": {"valid_ids": True, "band_width": 0}}
        buf = SimpleNamespace(_pangnn_hints=hints, x=x.view(n, 1), edge_index=ei.view(2, e), edge_attr=w, y=y,
                              ptr=ptr, batch=bid, live=live, live_edges=live[:1],
                              graph_ids=ids, spec=spec, num_graphs=g + 1, orders=None, union=bool(union))
        setattr(buf, "union_edge_index" if union else "neighbour_edge_index", nb.view(2, u))
        lib = _lib.load()
        if not orders or dev.type != "cuda":
            return buf
        if union:
            if lib.pangnn_collate_union_orders_supported(e, b, n):
                buf.orders = self._order_buffers(n, e, b, dev, union=True)
        elif lib.pangnn_structure_small_supported(e, n) and lib.pangnn_structure_small_supported(b, n):
            buf.orders = self._order_buffers(n, e, b, dev)
        return buf

    def _order_buffers(self, n, e, b, dev, union: bool = False):
        """device tables of the four CSR orders of a padded batch + the ctypes descriptor the collation takes (`union`: the
        second list is the union list of e + b columns)"""
        ct = chunk_tiles_for(e)
        nc = n_chunks(e, ct)
        rk = self.structure_index(union=union)
        second, b = ("union", e + b) if union else ("nb", b)
        # order after order: other, perm, keys (+ part_off: the similarity list's plans) | rowptr (+ part_rowptr); behind
        # them each plan's last_part, in a 16-byte slot of its own
        i32 = iter(carve(torch.int32, dev, [e, e, e, nc] * 2 + [b] * 6))
        i64 = iter(carve(torch.int64, dev, [n + 1] * 6 + [1, 1]))
        seg = {}
        for name in ("sim_dst", "sim_src", second + "_dst", second + "_src"):
            t = seg[name] = {"other": next(i32), "perm": next(i32), "keys": next(i32), "rowptr": next(i64)}
            if name.startswith("sim"):
                t["part_off"], t["part_rowptr"] = next(i32), next(i64)
        seg["sim_dst"]["last_part"], seg["sim_src"]["last_part"] = i64
        desc = (UnionBatchOrders if union else BatchOrders)(chunk_edges=32 * ct)
        for name, t in seg.items():
            o = getattr(desc, name)
            o.rank = getattr(rk, name).data_ptr()
            for f, table in t.items():
                setattr(o, f, table.data_ptr())
        return SimpleNamespace(desc=desc, tables=seg, chunk_tiles=ct, n_chunks=nc, _keep=rk)

    def _structures_of(self, buf):
        """graph.EdgeStructure objects of the batch's two edge lists over the order tables the collation wrote"""
        spec, ct = buf.spec, buf.orders.chunk_tiles
        n_bound = part_bound(spec.nodes, spec.edges, ct)
        out = {}
        second = ("union", buf.union_edge_index) if buf.union else ("nb", buf.neighbour_edge_index)
        for name, ei in (("sim", buf.edge_index), second):
            td, ts = buf.orders.tables[name + "_dst"], buf.orders.tables[name + "_src"]
            plans = None if name != "sim" else {
                (by, ct): RunPlan(n_bound, t["part_off"], t["part_rowptr"], t["keys"], ct, t["last_part"])
                for by, t in (("dst", td), ("src", ts))}
            # (a collated batch of small sub-graphs: short rows)
            out[name] = EdgeStructure(ei, spec.nodes, hints=buf._pangnn_hints[name]).adopt_tables(
                CSR(td["rowptr"], td["other"], td["perm"]), CSR(ts["rowptr"], ts["other"], ts["perm"]), plans)
        return out

    def collate_padded(self, buf):
        """(re)fill the padded batch `buf` from the sub-graph ids in buf.graph_ids (device): ONE launch, no host read-back;
        capturable — a replay collates whatever ids the list holds at that moment"""
        lib = _lib.load()
        g, n, e, b = buf.spec
        src_ei, src_nb = self.edge_index, self.neighbour_edge_index
        if not (src_ei.is_contiguous() and src_nb.is_contiguous() and self.node_off.is_contiguous()
                and self.edge_off.is_contiguous() and self.nb_off.is_contiguous() and self.edge_attr.is_contiguous()
                and self.y.is_contiguous()):
            raise ValueError("SubGraphDataset tensors must be contiguous")
        if self.edge_attr.dtype != torch.float32 or self.y.dtype != torch.float32:
            raise ValueError("edge_attr / y must be float32")
        # (a union batch: the same arguments, the union list where the neighbour list goes and edge_attr of its length)
        union = getattr(buf, "union", False)
        entry = "pangnn_collate_subgraphs_padded_union" if union else "pangnn_collate_subgraphs_padded"
        second = buf.union_edge_index if union else buf.neighbour_edge_index
        with _lib.device_guard(src_ei.device):
            _lib.check(getattr(lib, entry)(
                src_ei.data_ptr(), src_ei.shape[1], src_nb.data_ptr(), src_nb.shape[1], self.edge_attr.data_ptr(),
                self.y.data_ptr(), self.node_off.data_ptr(), self.edge_off.data_ptr(), self.nb_off.data_ptr(),
                self.num_graphs, buf.graph_ids.data_ptr(), g, e, b, n, buf.edge_index.data_ptr(),
                second.data_ptr(), buf.edge_attr.data_ptr(), buf.y.data_ptr(), buf.ptr.data_ptr(),
                buf.batch.data_ptr(), buf.x.data_ptr(), buf.live.data_ptr(),
                None if buf.orders is None else ctypes.byref(buf.orders.desc), _lib.stream_ptr()), entry)
        # what is cached on the batch object belongs to the previous content of the buffers (same addresses): replace it
        # by the structures over the tables this collation wrote, or drop it (built on first use as for any batch)
        for ei in (buf.edge_index, second):        # only THIS batch's entries of the identity-keyed cache
            forget(structure_key(ei, n), ei)
        if buf.orders is None:
            buf.__dict__.pop("_pangnn_structs", None)
        else:
            sts = self._structures_of(buf)
            buf._pangnn_structs = {name: (structure_key(st.edge_index, st.num_nodes), st) for name, st in sts.items()}
            for st in sts.values():
                register(st)
        return buf

    def set_graph_ids(self, buf, ids):
        """hand the next batch's sub-graph ids (host ints, at most buf.spec.graphs and 64) to the device list: one tiny launch
        whose arguments carry the values (no staging buffer that a later call could overwrite before it is read); returns the
        batch's real (nodes, edges, neighbour edges) — host arithmetic"""
        spec, g = buf.spec, buf.spec.graphs
        ids = [int(i) for i in ids]
        if not 0 < len(ids) <= min(g, 64) or g > 64:
            raise ValueError(f"a padded batch takes 1..{min(g, 64)} sub-graph ids")
        if min(ids) < 0 or max(ids) >= self.num_graphs:
            raise ValueError("sub-graph id out of range")
        n, e, b = self._counts(ids)
        if n >= spec.nodes or e > spec.edges or b > spec.nb_edges:
            raise ValueError(f"batch ({n} nodes, {e} edges, {b} neighbour edges) does not fit the padded shapes {tuple(spec)}")
        vals = (ctypes.c_int64 * g)(*(ids + [-1] * (g - len(ids))))
        with _lib.device_guard(buf.graph_ids.device):
            _lib.check(_lib.load().pangnn_set_i64(buf.graph_ids.data_ptr(), ctypes.cast(vals, ctypes.c_void_p), g,
                                                  _lib.stream_ptr()), "pangnn_set_i64")
        return n, e, b

    def class_balance(self):
        pos = self.y.sum().clamp_min(1)
        return ((self.y == 0).sum() / pos).to(torch.float32)
