"""Gene groups from binary edge predictions: write_groups_file of the reference (src/postprocessing.py:5-36), whose call
is commented out on the last line of pangnn.py (pangnn.py:375) because it cannot run — its `for node_set in sets` loop
starts on an empty list and never initialises it, the `append` behind the loop runs for every positive edge, two existing
sets are never merged, the output lines carry no newline, and the whole thing is a Python scan of every set for every edge.
So the semantics are BUILD-DEFINED here, after the reference's evident intent (connected components of the
predicted edges, only endpoints of predicted edges ever entering a set):

  * the predicted graph is undirected: an edge kept in either direction joins its two endpoints; edge e is kept when
    keep[e] != 0 (`keep=None`: every edge);
  * labels[v] = the smallest node id of v's connected component of the kept edges; a node no kept edge touches has
    labels[v] == v;
  * a node is TOUCHED when a kept edge has it as an endpoint; a kept self loop touches its node and joins nothing;
  * the groups are the components restricted to touched nodes, numbered 0 .. G-1 by ascending smallest member, members
    ascending inside a group; include_singletons=True adds every untouched node as a group of one, in the same ordering.

The result is canonical: the order of edges, duplicates, the grid and the thread schedule change nothing, two runs agree
bit for bit.  Device tensors run the three launches of pangnn_components_i32 (csrc/components.hip: a lock-free union-find
over the label array, `keep` read at its stored width — the int32 predictions of predict_homolog_genes and a bool mask
both go in without a conversion pass); CPU tensors run the same definition in plain torch.
"""
from __future__ import annotations

import os
from typing import NamedTuple, Optional, Union

import torch

from . import _lib

_BAD_IDS = "edge_index contains node ids outside [0, N)"


class Groups(NamedTuple):
    """labels int32 [N] (smallest id of each node's component); group_of int64 [N] (group number, -1 for a node in no
    group); group_ptr int64 [G + 1] and members int64 [M]: group g = members[group_ptr[g]:group_ptr[g + 1]], ascending;
    num_groups = G (a Python int).  All tensors on the input's device."""
    labels: torch.Tensor
    group_of: torch.Tensor
    group_ptr: torch.Tensor
    members: torch.Tensor
    num_groups: int


def _keep_flat(keep, num_edges: int):
    if keep is None:
        return None
    k = keep.detach().reshape(-1)
    if k.numel() != num_edges:
        raise ValueError(f"{k.numel()} keep entries for {num_edges} edges")
    return k


def _num_nodes(edge_index: torch.Tensor, num_nodes) -> int:
    if num_nodes is not None:
        return int(num_nodes)
    return int(edge_index.max().item()) + 1 if edge_index.numel() else 0       # a host read: whole graphs pass num_nodes


def _components_cpu(edge_index, keep, n: int):
    src, dst = edge_index[0].to(torch.int64), edge_index[1].to(torch.int64)
    if keep is not None:
        on = keep != 0
        src, dst = src[on], dst[on]
    if src.numel() and (int(torch.min(src.min(), dst.min())) < 0 or int(torch.max(src.max(), dst.max())) >= n):
        raise ValueError(_BAD_IDS)
    touched = torch.zeros(n, dtype=torch.bool)
    touched[src] = True
    touched[dst] = True
    a, b = torch.cat([src, dst]), torch.cat([dst, src])
    labels = torch.arange(n, dtype=torch.int64)
    while True:
        # labels is flat here (every node names its root), so labels[a] is the root of a's tree: hook it onto the
        # smallest root among its tree's neighbours, then jump pointers to a fixed point.  labels[x] <= x throughout.
        # Every tree that has a neighbouring tree with a smaller root hooks onto one, so the trees of a component at least
        # halve per round: at most ceil(log2(N)) + 1 rounds (17 + 1 for a 100 000-node path, whatever its ids), each with at
        # most ceil(log2(N)) pointer jumps.
        new = labels.scatter_reduce(0, labels[a], labels[b], reduce="amin", include_self=True)
        while True:
            jumped = new[new]
            if torch.equal(jumped, new):
                break
            new = jumped
        if torch.equal(new, labels):
            return labels.to(torch.int32), touched
        labels = new


def _enqueue_components(edge_index, keep, n: int):
    """(labels int32 [n], touched uint8 [n], status int32 [1]) of pangnn_components_i32, enqueued on the current stream;
    nothing is read back.  `keep` flat or None."""
    lib = _lib.load()
    _lib.require_device(edge_index, keep)
    if n >= 1 << 31:
        raise ValueError(f"int32 labels cannot name {n} nodes")
    ei = edge_index if edge_index.dtype == torch.int64 else edge_index.to(torch.int64)
    if ei.stride(1) != 1:
        ei = ei.contiguous()
    e = ei.shape[1]
    if e == 0:
        keep = None                                        # nothing to select (an empty tensor has no address)
    if keep is not None:
        if keep.dtype not in (torch.bool, torch.uint8, torch.int8, torch.int32):
            keep = keep != 0                               # other widths: one pass to a mask
        keep = keep.contiguous()
    dev = ei.device
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    touched = torch.empty(n, dtype=torch.uint8, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    with _lib.device_guard(dev):
        _lib.check(lib.pangnn_components_i32(ei[0].data_ptr(), ei[1].data_ptr(), _lib.ptr(keep),
                                             0 if keep is None else keep.element_size(), e, n, labels.data_ptr(),
                                             touched.data_ptr(), status.data_ptr(), _lib.stream_ptr()),
                   "pangnn_components_i32")
    return labels, touched, status


def connected_components(edge_index: torch.Tensor, keep: Optional[torch.Tensor] = None, num_nodes: Optional[int] = None):
    """(labels int32 [N], touched bool [N]) of the kept edges (module docstring).

    edge_index [2, E] with node ids in [0, N); keep [E] of any dtype, an edge is kept when its entry is non-zero.
    Without `num_nodes`, N = edge_index.max() + 1, which costs a host read and leaves out trailing isolated nodes: a whole
    graph should pass its node count.  A kept edge that names a node outside [0, N) raises ValueError; on the device the
    kernel skips such an edge and raises a flag, and reading that flag is the one synchronisation of this function."""
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError(f"edge_index must be [2, E], got {tuple(edge_index.shape)}")
    keep = _keep_flat(keep, edge_index.shape[1])
    n = _num_nodes(edge_index, num_nodes)
    if n < 0:
        raise ValueError(f"num_nodes = {n}")
    if not edge_index.is_cuda:
        if keep is not None and keep.is_cuda:
            raise ValueError("edge_index on the host with keep on the device")
        return _components_cpu(edge_index, keep, n)
    labels, touched, status = _enqueue_components(edge_index, keep, n)
    if int(status.item()):
        raise ValueError(_BAD_IDS)
    return labels, touched.view(torch.bool)


def _groups_of(labels: torch.Tensor, member: torch.Tensor) -> Groups:
    n, dev = labels.numel(), labels.device
    lab = labels.to(torch.int64)
    idx = torch.arange(n, dtype=torch.int64, device=dev)
    roots = torch.nonzero(member & (lab == idx)).view(-1)       # ascending: groups by smallest member (sizes: a host read)
    g = int(roots.numel())
    number = torch.full((n,), -1, dtype=torch.int64, device=dev)
    number[roots] = torch.arange(g, dtype=torch.int64, device=dev)
    group_of = torch.where(member, number[lab], torch.full_like(number, -1))
    nodes = torch.nonzero(member).view(-1)
    of_nodes = group_of[nodes]
    order = torch.sort(of_nodes, stable=True).indices           # stable: ascending ids stay ascending inside a group
    group_ptr = torch.zeros(g + 1, dtype=torch.int64, device=dev)
    if g:
        group_ptr[1:] = torch.cumsum(torch.bincount(of_nodes, minlength=g), 0)
    return Groups(labels, group_of, group_ptr, nodes[order], g)


def homolog_groups(edge_index: torch.Tensor, binary_prediction: torch.Tensor, num_nodes: Optional[int] = None,
                   include_singletons: bool = False) -> Groups:
    """The gene groups of a binary edge prediction: connected components of the edges with binary_prediction != 0,
    restricted to the nodes such an edge touches (module docstring), as a `Groups` on the input's device.

    `binary_prediction` is what predict_homolog_genes returns first (int32 0 / 1), or the labels `y` for the true
    groups; any dtype.  The components come from connected_components (one host read of its status flag); the
    compaction to (group_of, group_ptr, members) is torch plumbing whose output sizes — the number of groups and of
    members — take one more host read (torch.nonzero)."""
    labels, touched = connected_components(edge_index, binary_prediction, num_nodes)
    return _groups_of(labels, torch.ones_like(touched) if include_singletons else touched)


def _labels_and_membership(g: Union[Groups, torch.Tensor]):
    if isinstance(g, Groups):
        return g.labels.to(torch.int64), g.group_of >= 0
    lab = g.reshape(-1).to(torch.int64)
    return lab, torch.ones_like(lab, dtype=torch.bool)


def group_agreement(pred: Union[Groups, torch.Tensor], true: Union[Groups, torch.Tensor]) -> dict:
    """{'groups_pred', 'groups_true', 'groups_exact'}: the number of predicted groups, of true groups, and of predicted
    groups whose member set equals a true group's ("how many RIBAP groups were recovered exactly").

    Each argument is a `Groups` (its members are the nodes with group_of >= 0) or a label vector [N] as
    connected_components returns it (every node is a member, an isolated node a group of one); `true` is typically
    homolog_groups(edge_index, graph.y, N).  A predicted group is exact iff its members share one true label, that true
    group's members all carry this predicted label, and the two sizes are equal.  Computed on the labels' device from the
    two label vectors; one read-out at the end."""
    pl, pm = _labels_and_membership(pred)
    tl, tm = _labels_and_membership(true)
    n = pl.numel()
    if tl.numel() != n:
        raise ValueError(f"{n} predicted labels against {tl.numel()} true labels")
    tl, tm = tl.to(pl.device), tm.to(pl.device)
    dev = pl.device
    idx = torch.arange(n, dtype=torch.int64, device=dev)
    pk, tk = torch.where(pm, pl, -1), torch.where(tm, tl, -1)          # label of a member, -1 outside every group
    ps, ts = torch.where(pm, pl, n), torch.where(tm, tl, n)            # slot n collects the non-members

    def spread(slot, value):
        lo = torch.full((n + 1,), n, dtype=torch.int64, device=dev).scatter_reduce(0, slot, value, reduce="amin")
        hi = torch.full((n + 1,), -2, dtype=torch.int64, device=dev).scatter_reduce(0, slot, value, reduce="amax")
        return lo[:n], hi[:n], torch.bincount(slot, minlength=n + 1)[:n]

    t_lo, t_hi, p_size = spread(ps, tk)          # per predicted label: range of its members' true labels, its size
    p_lo, p_hi, t_size = spread(ts, pk)          # per true label: range of its members' predicted labels, its size
    t_of = t_lo.clamp(0, max(n - 1, 0))
    exact = (p_size > 0) & (t_lo == t_hi) & (t_lo >= 0) & (t_lo < n)
    if n:
        exact &= (p_lo[t_of] == idx) & (p_hi[t_of] == idx) & (t_size[t_of] == p_size)
    out = torch.stack([(p_size > 0).sum(), (t_size > 0).sum(), exact.sum()]).tolist()      # the one read-out
    return dict(groups_pred=int(out[0]), groups_true=int(out[1]), groups_exact=int(out[2]))


def write_groups_file(dataset, binary_prediction, path=os.path.join('data', 'holiest_of_all_tables.csv')) -> Groups:
    """The reference's write_groups_file(dataset, binary_prediction) with its default path, `path` added: one line per
    group, `group_{idx}, id, id, ...\\n` — with the newline the reference forgot.  Reads dataset.edge_index, the node count
    from dataset.x.shape[0] or dataset.num_nodes, and the gene names from dataset.gene_ids_lst when the dataset has one
    (the integer node id otherwise).  One device-to-host copy of group_ptr / members; returns the `Groups`."""
    x = getattr(dataset, "x", None)
    n = x.shape[0] if x is not None else getattr(dataset, "num_nodes", None)
    groups = homolog_groups(dataset.edge_index, binary_prediction, n)
    names = getattr(dataset, "gene_ids_lst", None)
    host = torch.cat([groups.group_ptr, groups.members]).tolist()
    ptr, members = host[:groups.num_groups + 1], host[groups.num_groups + 1:]
    folder = os.path.dirname(path)
    if folder:
        os.makedirs(folder, exist_ok=True)
    with open(path, "w") as fh:
        for g in range(groups.num_groups):
            ids = members[ptr[g]:ptr[g + 1]]
            fh.write(f"group_{g}, {', '.join(str(v) if names is None else str(names[v]) for v in ids)}\n")
    return groups
