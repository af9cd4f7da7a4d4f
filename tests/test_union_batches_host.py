"""Host side of --union_edge_weights mini-batches (pangnn_amd/subgraphs.py): union-layout sub-graph lists through
`SubGraphDataset.from_data_list`, `batch(i0, i1, union=True)` on a CPU-resident set against the oracle's collation of the
reference-layout union sub-graphs, the union ranks of `structure_index(union=True)`, the index arithmetic of
pangnn_collate_subgraphs_padded_union (csrc/graph_build.hip) restated with tensor ops over those ranks — every computed
position inside its table, the tables those of a stable sort of the collated union list —, the new symbols and the ABI
number.  No GPU.  `expected_padded_union` is what tests/test_union_batches.py holds the kernel's output against."""
import functools
from types import SimpleNamespace

import pytest
import torch

from conftest import sub_graphs_from_golden
from oracle import gcn_oracle as go

NEW_SYMBOLS = ("pangnn_collate_subgraphs_union", "pangnn_collate_subgraphs_padded_union",
               "pangnn_collate_union_orders_supported")


def union_layout(subs):
    """the reference's --union_edge_weights sub-graphs (dataset.py:287-302) of default-layout ones: union_edge_index =
    [neighbour | similarity] edges, edge_attr = [1 per neighbour edge | similarity weights], no neighbour_edge_index"""
    out = []
    for g in subs:
        b = g.neighbour_edge_index.shape[1]
        out.append(SimpleNamespace(x=g.x, edge_index=g.edge_index, y=g.y,
                                   edge_attr=torch.cat([torch.ones(b, dtype=g.edge_attr.dtype), g.edge_attr]),
                                   union_edge_index=torch.cat([g.neighbour_edge_index, g.edge_index], dim=1)))
    return out


def hand_made():
    """three sub-graphs: edges present in both lists (0 -> 1, 1 -> 0, 1 -> 2 of the first, 0 -> 1 of the third), one
    sub-graph without neighbour edges, a similarity list that is not source-sorted"""
    def sub(n, ei, w, y, nb):
        return SimpleNamespace(x=torch.ones(n, 1), edge_index=torch.tensor(ei, dtype=torch.int64).view(2, -1),
                               edge_attr=torch.tensor(w, dtype=torch.float32), y=torch.tensor(y, dtype=torch.float32),
                               neighbour_edge_index=torch.tensor(nb, dtype=torch.int64).view(2, -1))
    return [sub(4, [[0, 1, 2, 1], [1, 0, 3, 2]], [0.5, 0.25, 2.0, 3.0], [1, 0, 1, 0], [[0, 1, 1, 2], [1, 0, 2, 1]]),
            sub(2, [[0, 1], [1, 0]], [1.5, 7.0], [1, 1], [[], []]),
            sub(3, [[2, 0, 0], [0, 2, 1]], [4.0, 5.0, 6.0], [0, 0, 1], [[0, 1, 1, 2], [1, 0, 2, 1]])]


@functools.lru_cache(maxsize=None)
def cpu_dataset(name):
    from pangnn_amd import simulate
    from pangnn_amd.subgraphs import SubGraphDataset
    if name == "cfg1":
        return SubGraphDataset.from_data_list(sub_graphs_from_golden("cfg1_2genomes"))
    if name == "hand":
        return SubGraphDataset.from_data_list(hand_made())
    assert name == "sim200"
    return simulate.simulate_subgraph_dataset(200, 4, 0.3, 10, 2, seed=0, device="cpu")


DATASETS = ("cfg1", "sim200", "hand")


def shuffled_ids(ds, count, seed=1):
    return torch.randperm(ds.num_graphs, generator=torch.Generator().manual_seed(seed)).tolist()[:count]


def pad_ids(real, total, n_r, max_n):
    """the padding of a padded list: `total - real` self loops spread evenly over the padded nodes, ids non-decreasing"""
    p = total - real
    return n_r + (torch.arange(p, dtype=torch.int64) * (max_n - n_r)) // max(p, 1)


def expected_padded_union(ds, ids, spec):
    """every field of a padded union batch as DESIGN.md §6e states it, with index ops on the host (ds: any device)"""
    g_max, max_n, max_e, max_b = spec
    max_u = max_e + max_b
    h = ds._host()
    ids = [int(i) for i in ids]
    n, e, b = ds._counts(ids)
    fits = len(ids) <= g_max and n < max_n and e <= max_e and b <= max_b
    ei, nb, w, y, ptr, bid, at = [], [], [], [], [0], [], 0
    for k, i in enumerate(ids):
        n0, e0, e1, b0, b1 = h.node[i], h.edge[i], h.edge[i + 1], h.nb[i], h.nb[i + 1]
        ei.append(ds.edge_index[:, e0:e1].cpu() - n0 + at)
        nb.append(ds.neighbour_edge_index[:, b0:b1].cpu() - n0 + at)
        w.append(ds.edge_attr[e0:e1].cpu()); y.append(ds.y[e0:e1].cpu())
        bid.append(torch.full((h.node[i + 1] - n0,), k, dtype=torch.int64))
        at += h.node[i + 1] - n0
        ptr.append(at)
    ei, nb, w, y, bid = torch.cat(ei, 1), torch.cat(nb, 1), torch.cat(w), torch.cat(y), torch.cat(bid)
    if not fits:
        ei, nb, w, y, bid, n, e, b = ei[:, :0], nb[:, :0], w[:0], y[:0], bid[:0], 0, 0, 0
    pad_e, pad_u = pad_ids(e, max_e, n, max_n), pad_ids(e + b, max_u, n, max_n)
    out = SimpleNamespace(
        edge_index=torch.cat([ei, torch.stack([pad_e, pad_e])], 1),
        union_edge_index=torch.cat([ei, nb, torch.stack([pad_u, pad_u])], 1),
        edge_attr=torch.cat([w, torch.ones(max_u - e)]), y=torch.cat([y, torch.zeros(max_e - e)]),
        ptr=torch.tensor([ptr[k] if k <= len(ids) else n for k in range(g_max + 1)], dtype=torch.int64),
        batch=torch.cat([bid, torch.full((max_n - n,), len(ids), dtype=torch.int64)]), x=torch.ones(max_n, 1),
        live=torch.tensor([e, b, n, len(ids), 0 if fits else 1], dtype=torch.int64))
    if not fits:                     # (ptr of the real graphs is still their cumulative node count: the kernel writes cn[k])
        out.ptr = torch.tensor([ptr[k] if k <= len(ids) else 0 for k in range(g_max + 1)], dtype=torch.int64)
    return out


def emulated_union_orders(ds, ids, spec):
    """the order tables of the union list as collate_padded_kernel<true> computes them: column -> slot by the cumulative
    counts, flat edge, sorted position = ce[j] + cb[j] + rank; returns {order: (perm, other, keys)} and asserts every
    store is inside its table and no position is written twice"""
    g_max, max_n, max_e, max_b = spec
    max_u = max_e + max_b
    rk = ds.structure_index(union=True)
    h = ds._host()
    ids = [int(i) for i in ids]
    E = ds.edge_index.shape[1]
    cn, ce, cb = [0], [0], [0]
    for i in ids:
        cn.append(cn[-1] + h.node[i + 1] - h.node[i]); ce.append(ce[-1] + h.edge[i + 1] - h.edge[i])
        cb.append(cb[-1] + h.nb[i + 1] - h.nb[i])
    e_r, b_r, n_r = ce[-1], cb[-1], cn[-1]
    assert n_r < max_n and e_r <= max_e and b_r <= max_b
    cn, ce, cb, gid = (torch.tensor(v, dtype=torch.int64) for v in (cn, ce, cb, ids))
    col = torch.arange(e_r + b_r)
    sim = col < e_r
    cc = torch.where(sim, col, col - e_r)
    # slot: the largest j < g with c[j] <= cc (the kernel's binary search over c[0 .. g - 1])
    j = torch.where(sim, torch.searchsorted(ce[:-1], cc, right=True) - 1, torch.searchsorted(cb[:-1], cc, right=True) - 1)
    first_own = torch.where(sim, ce[j], cb[j])
    off_own = torch.where(sim, ds.edge_off.cpu()[gid[j]], ds.nb_off.cpu()[gid[j]])
    t = off_own + (cc - first_own)
    assert bool(((t >= off_own) & (t < torch.where(sim, ds.edge_off.cpu()[gid[j] + 1], ds.nb_off.cpu()[gid[j] + 1]))).all())
    shift = cn[j] - ds.node_off.cpu()[gid[j]]
    both = torch.cat([ds.edge_index.cpu(), ds.neighbour_edge_index.cpu()], dim=1)
    r = torch.where(sim, t, E + t)
    sv, dv = both[0][r] + shift, both[1][r] + shift
    pad = pad_ids(e_r + b_r, max_u, n_r, max_n)
    out = {}
    for name, key, other in (("union_dst", dv, sv), ("union_src", sv, dv)):
        pos = ce[j] + cb[j] + getattr(rk, name).cpu().long()[r]
        assert bool(((pos >= 0) & (pos < e_r + b_r)).all()), name          # a wrong rank table is an out-of-bounds store
        assert torch.unique(pos).numel() == pos.numel(), name
        perm, oth, keys = (torch.full((max_u,), -1, dtype=torch.int64) for _ in range(3))
        perm[pos], oth[pos], keys[pos] = col, other, key
        tail = torch.arange(e_r + b_r, max_u)
        perm[tail], oth[tail], keys[tail] = tail, pad, pad
        out[name] = (perm, oth, keys)
    return out


# ------------------------------------------------------------------------------------------------------------------
# 1. from_data_list
# ------------------------------------------------------------------------------------------------------------------
def test_from_data_list_takes_union_layout_sub_graphs():
    from pangnn_amd.subgraphs import SubGraphDataset
    subs = sub_graphs_from_golden("cfg1_2genomes")
    a, b = SubGraphDataset.from_data_list(subs), SubGraphDataset.from_data_list(union_layout(subs))
    assert a.num_graphs == b.num_graphs == len(subs)
    for k in ("node_off", "edge_off", "nb_off", "edge_index", "neighbour_edge_index", "edge_attr", "y"):
        assert torch.equal(getattr(a, k), getattr(b, k)) and getattr(a, k).dtype == getattr(b, k).dtype, k
    assert b.neighbour_edge_index.is_contiguous() and b.edge_attr.is_contiguous()
    # a mixed list is taken too: each sub-graph in its own layout
    c = SubGraphDataset.from_data_list(union_layout(subs[:3]) + subs[3:6])
    assert torch.equal(c.edge_attr, a.edge_attr[:int(a.edge_off[6])])
    assert torch.equal(c.neighbour_edge_index, a.neighbour_edge_index[:, :int(a.nb_off[6])])


def test_from_data_list_refuses_malformed_union_sub_graphs():
    from pangnn_amd.subgraphs import SubGraphDataset
    subs = [g for g in sub_graphs_from_golden("cfg1_2genomes", 8) if g.neighbour_edge_index.shape[1] and g.edge_index.shape[1]]
    assert len(subs) >= 2
    bad = union_layout(subs)
    bad[1].union_edge_index = bad[1].union_edge_index.clone()
    bad[1].union_edge_index[0, -1] += 1                                   # the last e columns are not edge_index
    with pytest.raises(ValueError, match="sub-graph 1"):
        SubGraphDataset.from_data_list(bad)
    bad = union_layout(subs)
    bad[0].edge_attr = bad[0].edge_attr.clone()
    bad[0].edge_attr[0] = 2.0                                             # a neighbour weight that is not 1
    with pytest.raises(ValueError, match="sub-graph 0"):
        SubGraphDataset.from_data_list(bad)


# ------------------------------------------------------------------------------------------------------------------
# 2. batch(union=True) with index ops
# ------------------------------------------------------------------------------------------------------------------
def _triples(ei, w):
    t = torch.stack([ei[0].double(), ei[1].double(), w.double()], 1)
    for c in (2, 1, 0):
        t = t[torch.argsort(t[:, c], stable=True)]
    return t


@pytest.mark.parametrize("rng", [(0, 32), (5, 6), (40, 10 ** 6)], ids=["first32", "one", "tail"])
def test_union_batch_on_the_host(rng):
    subs = sub_graphs_from_golden("cfg1_2genomes")
    ds = cpu_dataset("cfg1")
    i0, i1 = rng[0], min(rng[1], len(subs))
    got, plain = ds.batch(i0, i1, union=True), ds.batch(i0, i1)
    ref = go.collate(union_layout(subs[i0:i1]))
    e, b = plain.edge_index.shape[1], plain.neighbour_edge_index.shape[1]
    assert not hasattr(got, "neighbour_edge_index") and got.num_graphs == i1 - i0
    assert torch.equal(got.union_edge_index, torch.cat([plain.edge_index, plain.neighbour_edge_index], 1))
    assert torch.equal(got.edge_attr, torch.cat([plain.edge_attr, torch.ones(b)])) and got.edge_attr.dtype == torch.float32
    assert torch.equal(got.edge_attr[:e], plain.edge_attr)                # aligned with edge_index: what skip_connections reads
    for k in ("x", "y", "edge_index", "ptr", "batch"):
        assert torch.equal(getattr(got, k), getattr(plain, k)), k
        assert torch.equal(getattr(got, k), getattr(ref, k)), k
    assert got.union_edge_index.is_contiguous() and got.union_edge_index.shape == ref.union_edge_index.shape == (2, e + b)
    assert torch.equal(_triples(got.union_edge_index, got.edge_attr), _triples(ref.union_edge_index, ref.edge_attr))
    assert set(got._pangnn_hints) == {"sim", "union"}


def test_cfg1_union_lists_do_hold_edges_twice():
    """388 similarity edges of cfg1's sub-graphs also are neighbour edges: the union is a multiset and its orders must break ties"""
    ds = cpu_dataset("cfg1")
    n = int(ds.node_off[-1])
    sim, nb = ds.edge_index[0] * n + ds.edge_index[1], ds.neighbour_edge_index[0] * n + ds.neighbour_edge_index[1]
    assert int(torch.isin(sim, nb).sum()) == 388


# ------------------------------------------------------------------------------------------------------------------
# 3. union ranks, and the kernel's index arithmetic over them
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DATASETS)
def test_union_ranks_are_the_stable_orders_of_every_sub_graph(name):
    ds = cpu_dataset(name)
    rk = ds.structure_index(union=True)
    assert rk is ds.structure_index() and rk.sim_dst.dtype == rk.union_dst.dtype == torch.int32
    h = ds._host()
    E, B = ds.edge_index.shape[1], ds.neighbour_edge_index.shape[1]
    assert rk.union_dst.shape == rk.union_src.shape == (E + B,)
    for g in range(ds.num_graphs):
        e0, e1, b0, b1 = h.edge[g], h.edge[g + 1], h.nb[g], h.nb[g + 1]
        m = (e1 - e0) + (b1 - b0)
        lst = torch.cat([ds.edge_index[:, e0:e1], ds.neighbour_edge_index[:, b0:b1]], 1)
        for order, row in (("union_dst", 1), ("union_src", 0)):
            r = torch.cat([getattr(rk, order)[e0:e1], getattr(rk, order)[E + b0:E + b1]]).long()
            assert torch.equal(torch.sort(r).values, torch.arange(m)), (g, order)
            placed = torch.empty(m, dtype=torch.int64)
            placed[r] = torch.arange(m)
            assert torch.equal(placed, torch.argsort(lst[row], stable=True)), (g, order)


@pytest.mark.parametrize("name", DATASETS)
def test_the_collation_index_arithmetic_gives_the_stable_orders_of_the_batch(name):
    from pangnn_amd.subgraphs import PaddedSpec
    ds = cpu_dataset(name)
    for ids in (shuffled_ids(ds, 32), shuffled_ids(ds, 1, seed=2), list(range(min(3, ds.num_graphs)))[::-1]):
        for spec in (ds.padded_spec(32), PaddedSpec(32, ds._counts(ids)[0] + 1, max(ds._counts(ids)[1], 1),
                                                     max(ds._counts(ids)[2], 1))):
            exp = expected_padded_union(ds, ids, spec)
            un = exp.union_edge_index
            assert un.shape == (2, spec.edges + spec.nb_edges) and int(un.max()) < spec.nodes
            for order, row in (("union_dst", 1), ("union_src", 0)):
                perm, other, keys = emulated_union_orders(ds, ids, spec)[order]
                want = torch.argsort(un[row], stable=True)
                assert torch.equal(perm, want), (name, order)
                assert torch.equal(keys, un[row][want]) and torch.equal(other, un[1 - row][want]), (name, order)


# ------------------------------------------------------------------------------------------------------------------
# 4. ABI
# ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_resolve_and_the_abi_number_stays():
    from pangnn_amd import _lib
    L = _lib.load()
    assert L.pangnn_abi_version() == 3 == _lib.ABI_VERSION
    for name in NEW_SYMBOLS:
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) > 0, name
    # the union forms: the default forms' arguments (+ the weights the unpadded one also writes: one in, one out)
    assert len(L.pangnn_collate_subgraphs_padded_union.argtypes) == len(L.pangnn_collate_subgraphs_padded.argtypes)
    assert len(L.pangnn_collate_subgraphs_union.argtypes) == len(L.pangnn_collate_subgraphs.argtypes) + 2


def test_host_argument_checks_and_the_order_limits():
    """null pointers only: nothing here could reach a device"""
    import ctypes
    from pangnn_amd import _lib
    from pangnn_amd.subgraphs import BatchOrders, UnionBatchOrders
    L = _lib.load()
    assert ctypes.sizeof(UnionBatchOrders) == ctypes.sizeof(BatchOrders)
    sup = L.pangnn_collate_union_orders_supported
    assert sup(16384, 16384, 65536) and sup(1, 32767, 2) and sup(7000, 7303, 4000) and sup(13000, 14090, 30000)
    assert not sup(16385, 1, 100) and not sup(16384, 16385, 100) and not sup(100, 100, 65537) and not sup(0, 5, 10)
    assert not sup(5, 0, 10)

    def padded(max_graphs=32, max_e=10, max_b=10, max_n=10):
        return L.pangnn_collate_subgraphs_padded_union(None, 0, None, 0, None, None, None, None, None, 0, None, max_graphs, max_e,
                                                       max_b, max_n, None, None, None, None, None, None, None, None, None, None)
    for kw in (dict(max_graphs=0), dict(max_graphs=257), dict(max_e=0), dict(max_b=0), dict(max_n=1), dict()):
        assert padded(**kw) == -1, kw                                       # PANGNN_E_BADARG (the last: null pointers)
        assert b"pangnn_collate_subgraphs_padded_union" in L.pangnn_last_error()
    un = L.pangnn_collate_subgraphs_union
    assert un(None, 5, 3, 4, None, 0, 0, 0, None, None, 1, 0, 2, None, None, None, None, None, None, None) == -1   # e0 + e > ld_e
    assert un(None, 5, 0, 4, None, 0, 0, 0, None, None, 1, 0, 2, None, None, None, None, None, None, None) == -1   # null pointers
    assert b"pangnn_collate_subgraphs_union" in L.pangnn_last_error()
