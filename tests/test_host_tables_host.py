"""The packed host tables where there is no GPU: graph.carve (views, alignment, disjoint byte ranges, storage size), the
plan sizes graph.n_chunks / graph.part_bound against the expressions every site wrote out before and against exact part
counts, subgraphs.PaddedSpec as the plain 4-tuple it replaces, and the two ctypes mirrors of include/pangnn_hip.h."""
import ctypes
from itertools import product

import pytest
import torch

from conftest import sub_graphs_from_golden
from pangnn_amd import graph as G, subgraphs as SG
from pangnn_amd.graph import EdgeStructure

COUNTS = [[], [0], [1], [0, 0], [1, 1, 1], [3, 0, 5, 0, 0, 7], [17, 16, 15, 1, 33], [0, 1000, 1, 0], [4, 8, 16, 32], [2, 2, 9, 1, 1]]


def _round_up(k, m):
    return -(-k // m) * m


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.float32, torch.uint8], ids=str)
@pytest.mark.parametrize("counts", COUNTS, ids=str)
def test_carve_gives_aligned_disjoint_views_of_one_allocation(dtype, counts):
    views = G.carve(dtype, "cpu", counts)
    assert type(views) is list and len(views) == len(counts)
    size = dtype.itemsize
    end = None
    for v, k in zip(views, counts):
        assert v.dtype == dtype and v.dim() == 1 and v.numel() == k and v.is_contiguous() and v.device.type == "cpu"
        assert v.data_ptr() % 16 == 0
        base = v.untyped_storage()
        assert base.data_ptr() == views[0].untyped_storage().data_ptr()                 # one allocation
        assert base.nbytes() <= sum(_round_up(c * size, 16) for c in counts)
        lo = base.data_ptr() + v.storage_offset() * size                                # (an empty view has no address of its own)
        assert lo % 16 == 0 and base.data_ptr() <= lo and lo + k * size <= base.data_ptr() + base.nbytes()
        assert end is None or lo >= end                                                 # in order, pairwise disjoint
        end = lo + k * size
    for i, v in enumerate(views):                                                       # a write to one reaches no other
        v.fill_(i + 1)
    assert all(bool((v == i + 1).all()) for i, v in enumerate(views))


def test_carve_takes_another_alignment():
    a, b, c = G.carve(torch.int32, "cpu", [1, 3, 2], align=64)
    assert [v.storage_offset() for v in (a, b, c)] == [0, 16, 32] and c.untyped_storage().nbytes() == 3 * 64


SIZES = [(rows, e, ct) for ct in (1, 16) for rows, e in
         [(0, 0), (5, 0), (0, 7), (9, 3), (3, 9), (1, 1), (40, 32 * ct), (40, 32 * ct + 1), (2000, 32 * ct - 1),
          (7, 3 * 32 * ct), (7, 3 * 32 * ct + 1), (100000, 70001)]]


@pytest.mark.parametrize("rows,e,ct", SIZES)
def test_plan_sizes_are_the_expressions_they_replace(rows, e, ct):
    span = 32 * ct
    assert G.n_chunks(e, ct) == (e + span - 1) // span
    assert G.part_bound(rows, e, ct) == (e + span - 1) // span + min(rows, e)
    assert type(G.n_chunks(e, ct)) is int and type(G.part_bound(rows, e, ct)) is int


def test_the_sizes_table_has_the_edge_cases():
    for ct in (1, 16):
        span = 32 * ct
        mine = [(r, e) for r, e, c in SIZES if c == ct]
        assert any(e == 0 and r > 0 for r, e in mine) and any(r == 0 and e > 0 for r, e in mine)
        assert any(0 < e < r for r, e in mine) and any(e and e % span == 0 for r, e in mine)
        assert any(e > span and e % span == 1 for r, e in mine)


@pytest.mark.parametrize("ct", [1, 16])
def test_the_part_bound_holds_for_random_sorted_keys(ct):
    gen = torch.Generator().manual_seed(7)
    span = 32 * ct
    for rows, e in product((1, 2, 50, 3000), (1, span - 1, span, span + 1, 5 * span + 3)):
        keys = torch.sort(torch.randint(0, rows, (e,), generator=gen)).values
        plan = EdgeStructure._plan_of_sorted_keys(keys, rows, ct)
        assert plan.n_parts == G.part_bound(rows, e, ct) >= plan.n_parts_exact() >= G.n_chunks(e, ct)
        assert plan.part_off.shape == (G.n_chunks(e, ct),)
    distinct = torch.arange(span + 1)                   # every key changes: the bound is met exactly
    plan = EdgeStructure._plan_of_sorted_keys(distinct, span + 1, ct)
    assert plan.n_parts_exact() == span + 1 and plan.n_parts == span + 3


def test_chunk_tiles_for_is_the_librarys_answer():
    from pangnn_amd import _lib, functional as PF
    lib = _lib.load()
    for e in (0, 1, 33, 3000, 20000, 140000, 10 ** 6, 10 ** 8):
        assert G.chunk_tiles_for(e) == PF.d16_chunk(e) == lib.pangnn_decoder_chunk_tiles_for(e)
        assert type(G.chunk_tiles_for(e)) is int
    assert PF.d16_chunk() == lib.pangnn_decoder_chunk_tiles()


def test_structure_key_is_the_identity_every_cache_uses():
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    key = G.structure_key(ei, 3)
    assert key == (ei.data_ptr(), ei._version, (2, 3), 3, ei.device.index)
    G._CACHE.clear()
    st = EdgeStructure(ei, 3)
    G.register(st)
    assert G._CACHE.pop(key) is st and not G._CACHE


def _golden_dataset():
    return SG.SubGraphDataset.from_data_list(sub_graphs_from_golden("cfg1_2genomes"))


def test_padded_spec_is_the_plain_tuple_with_names():
    ds = _golden_dataset()
    h = ds._host()

    def cap(off, idx, bs, slack):                       # the arithmetic padded_spec is documented to do
        sizes = sorted((off[i + 1] - off[i] for i in idx), reverse=True)
        worst = sum(sizes[:bs])
        return worst if slack is None else min(worst, int(float(slack) * bs * sum(sizes) / len(sizes)) + 1)

    for bs, graphs, slack in ((32, None, None), (4, None, 1.3), (3, range(min(5, ds.num_graphs)), None)):
        idx = list(range(ds.num_graphs)) if graphs is None else list(graphs)
        want = (bs, cap(h.node, idx, bs, slack) + 1, max(cap(h.edge, idx, bs, slack), 1), max(cap(h.nb, idx, bs, slack), 1))
        spec = ds.padded_spec(bs, graphs, slack)
        assert type(spec) is SG.PaddedSpec and isinstance(spec, tuple) and SG.PaddedSpec._fields == ("graphs", "nodes", "edges", "nb_edges")
        assert spec == want and want == spec and tuple(spec) == want and hash(spec) == hash(want)
        assert {want: 1}[spec] == 1 and (spec[0], spec[1], spec[2], spec[3]) == want
        assert (spec.graphs, spec.nodes, spec.edges, spec.nb_edges) == want
        g, n, e, b = spec
        assert (g, n, e, b) == want
        ids = idx[:bs]
        assert ds.fits(spec, ids) == ds.fits(want, ids)
        if slack is None:
            assert ds.fits(want, ids)
    assert not ds.fits((1, 10 ** 6, 10 ** 6, 10 ** 6), [0, 1]) and not ds.fits((2, 1, 10 ** 6, 10 ** 6), [0, 1])


def test_padded_buffers_on_the_host_are_carved_and_keep_the_spec():
    ds = _golden_dataset()
    want = tuple(ds.padded_spec(4))
    buf = ds.padded_buffers(want)                        # a plain tuple is taken too
    g, n, e, b = want
    assert buf.spec == want and type(buf.spec) is SG.PaddedSpec and buf.orders is None and buf.num_graphs == g + 1
    shapes = {"edge_index": (2, e), "neighbour_edge_index": (2, b), "ptr": (g + 1,), "batch": (n,), "live": (8,),
              "graph_ids": (g,), "edge_attr": (e,), "y": (e,), "x": (n, 1)}
    for dtype, names in ((torch.int64, ("edge_index", "neighbour_edge_index", "ptr", "batch", "live", "graph_ids")),
                         (torch.float32, ("edge_attr", "y", "x"))):
        end = None
        for name in names:                               # one allocation per element type, in this order
            t = getattr(buf, name)
            assert t.dtype == dtype and tuple(t.shape) == shapes[name] and t.is_contiguous() and t.data_ptr() % 16 == 0
            assert t.untyped_storage().data_ptr() == getattr(buf, names[0]).untyped_storage().data_ptr()
            assert end is None or t.data_ptr() >= end
            end = t.data_ptr() + t.numel() * t.element_size()
    assert buf.graph_ids.tolist() == [-1] * g and buf.live.tolist() == [0] * 8
    assert buf.live_edges.data_ptr() == buf.live.data_ptr() and buf.live_edges.shape == (1,)


def test_the_ctypes_classes_mirror_the_header():
    """pangnn_batch_order: eight pointers; pangnn_batch_orders: int32 chunk_edges, then four of them (pointer-aligned)"""
    pointers = ["rank", "rowptr", "other", "perm", "keys", "part_off", "part_rowptr", "last_part"]
    assert [(k, t) for k, t in SG.BatchOrder._fields_] == [(k, ctypes.c_void_p) for k in pointers]
    assert ctypes.sizeof(SG.BatchOrder) == 8 * ctypes.sizeof(ctypes.c_void_p)
    assert [k for k, _ in SG.BatchOrders._fields_] == ["chunk_edges", "sim_dst", "sim_src", "nb_dst", "nb_src"]
    assert [t for _, t in SG.BatchOrders._fields_] == [ctypes.c_int32] + [SG.BatchOrder] * 4
    assert ctypes.sizeof(SG.BatchOrders) == (1 + 4 * 8) * ctypes.sizeof(ctypes.c_void_p)
    assert SG.BatchOrders.sim_dst.offset == ctypes.sizeof(ctypes.c_void_p)
    fresh = SG.BatchOrders(chunk_edges=64)
    assert fresh.chunk_edges == 64 and fresh.nb_src.part_off is None and fresh.sim_dst.rank is None
