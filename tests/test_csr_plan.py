"""pangnn_csr_plan (csrc/csr_plan.hip): the decoder's run-sum plan from a row pointer, against the written definition
EdgeStructure._plan_of_sorted_keys on the expanded keys, and through EdgeStructure.csr_plan / runsum_plan against the
torch route (graph.PLAN_KERNEL off).  Every comparison is exact: same dtypes, torch.equal."""
import functools

import pytest
import torch

import pangnn_amd
from conftest import load_golden, random_graph
from pangnn_amd import _lib, graph as G, sub_sample_graph_edges
from pangnn_amd.data import Data
from pangnn_amd.graph import EdgeStructure
from pangnn_amd.sampling import release
from pangnn_amd.train import make_optimizer, train_step
from test_plan_mask_host import edge_counts, keys_of, layouts

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
LAYOUTS = ["hub_alone", "hub_among_empty_rows", "one_entry_per_row", "rows_on_chunk_boundaries", "empty_front_back_middle",
           "heavy_tailed"]


def plans_equal(got, want, what=""):
    for f in ("keys", "part_off", "part_rowptr", "last"):
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (what, f)
    assert got.n_parts == want.n_parts and got.chunk_tiles == want.chunk_tiles, what
    assert got.n_parts_exact() == want.n_parts_exact() <= got.n_parts, what


def tiles_for(e, which):
    return {"one": 1, "sixteen": 16, "for_e": int(_lib.load().pangnn_decoder_chunk_tiles_for(e))}[which]


def sizes(which):
    """(E, chunk_tiles): E in {1, span - 1, span, span + 1, 2 span, 3 span + 7, 70001} of the span that goes with it"""
    if which != "for_e":
        return [(e, tiles_for(e, which)) for e in edge_counts(32 * tiles_for(0, which))]
    # the chunk size is a function of E here: every E that stands in one of those relations to its OWN span
    every = sorted({e for span in range(32, 1024 + 1, 32) for e in edge_counts(span)})
    return [(e, tiles_for(e, which)) for e in every if e in edge_counts(32 * tiles_for(e, which))]


@pytest.mark.parametrize("name", LAYOUTS)
@pytest.mark.parametrize("which", ["one", "for_e", "sixteen"])
def test_the_plan_of_a_rowptr_is_the_plan_of_its_keys(which, name):
    cases = sizes(which)
    assert {1, 70001} <= {e for e, _ in cases} and len(cases) >= 7
    for e, ct in cases:
        rowptr = layouts(e, 32 * ct)[name].to(DEV)
        n_rows = rowptr.numel() - 1
        want = EdgeStructure._plan_of_sorted_keys(keys_of(rowptr), n_rows, ct)
        got = EdgeStructure._plan_of_rowptr(rowptr, e, ct)
        plans_equal(got, want, (name, e, ct))
        again = EdgeStructure._plan_of_rowptr(rowptr, e, ct)                  # two calls: bit-identical tables
        plans_equal(again, got, (name, e, ct, "again"))


# ---- the corners of the kernels' entry -> row search (csrc/common.h row_of_entry: the plan kernel here, the edge-dot kernels
# in tests/test_edge_weight_grad.py) at small sizes
SEARCH_ROWS = (1, 2, 3, 65, 130)


def _filled(m, e):
    """m non-empty rows that share e >= m entries: the first ends on entry 32 and the second on entry 64 where e allows (row
    boundaries on the 32-entry plan chunks and the 64-entry edge-dot chunks), one entry in each other row and the rest in
    the last one (boundaries off them)"""
    lens, spare = [1] * m, e - m
    for i in (0, 1):
        if i < m - 1 and spare >= 31:
            lens[i] += 31
            spare -= 31
    lens[-1] += spare
    return lens


@functools.lru_cache(maxsize=None)
def search_corners():
    """((name, rowptr int64 [n_rows + 1] on the CPU), ...): 1, 2, 3, 65 and 130 rows; every entry in the first row / in the
    last row, leading empty rows, trailing empty rows, empty and non-empty rows alternating (either first), one row of 200
    entries among single-entry rows; 1 to 329 entries"""
    out = []
    for n in SEARCH_ROWS:
        lens = {}
        for e in (1, 32, 33, 64, 65, 300):
            lens[f"all_in_first_row-{e}"] = [e] + [0] * (n - 1)
            if n > 1:
                lens[f"all_in_last_row-{e}"] = [0] * (n - 1) + [e]
        hub = [1] * n
        hub[n // 2] = 200
        lens["a_row_of_200_among_rows_of_one"] = hub
        if n > 1:
            m, k = n - n // 2, n // 2
            for e in sorted({m, 96, 130, 300}):
                if e >= m:
                    lens[f"leading_empty_rows-{e}"] = [0] * k + _filled(m, e)
                    lens[f"trailing_empty_rows-{e}"] = _filled(m, e) + [0] * k
            for e in sorted({k, 96, 130, 300}):
                if e >= k:
                    full = _filled(k, e)
                    lens[f"alternating_empty_first-{e}"] = [v for f in full for v in (0, f)] + [0] * (n - 2 * k)
                    lens[f"alternating_full_first-{e}"] = [v for f in full for v in (f, 0)] + [0] * (n - 2 * k)
        for name, ln in lens.items():
            assert len(ln) == n and 1 <= sum(ln) <= 329, (n, name)
            out.append((f"{n}_rows-{name}", torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.tensor(ln), 0)])))
    return tuple(out)


def row_of_entries(rowptr):
    """the row of every entry of a CPU row pointer: the last row r with rowptr[r] <= k, among equal row pointers the non-empty row"""
    return torch.searchsorted(rowptr, torch.arange(int(rowptr[-1])), right=True) - 1


@pytest.mark.parametrize("ct", [1, 2])
def test_the_plan_at_the_corners_of_the_row_search(ct):
    assert len(search_corners()) > 100
    for name, rowptr in search_corners():
        e, n_rows = int(rowptr[-1]), rowptr.numel() - 1
        rows = row_of_entries(rowptr)
        assert torch.equal(rows, keys_of(rowptr)), name
        got = EdgeStructure._plan_of_rowptr(rowptr.to(DEV), e, ct)
        assert torch.equal(got.keys.cpu().long(), rows), (name, ct)
        plans_equal(got, EdgeStructure._plan_of_sorted_keys(rows.to(DEV), n_rows, ct), (name, ct))


def _golden(name="cfg2_sim_1000x5"):
    f = load_golden(name)
    return Data(x=torch.from_numpy(f["whole_x"]).to(DEV), edge_index=torch.from_numpy(f["whole_edge_index"]).to(DEV),
                edge_attr=torch.from_numpy(f["whole_edge_attr"]).to(DEV), y=torch.from_numpy(f["whole_y"]).to(DEV),
                neighbour_edge_index=torch.from_numpy(f["whole_neighbour_edge_index"]).to(DEV))


def _edge_lists():
    ei, _ = random_graph(900, 9000, seed=3)
    by_src = ei[:, torch.sort(ei[0], stable=True).indices].contiguous()
    g = _golden()
    return {"random": (ei, 900), "random_sorted_by_source": (by_src, 900), "golden": (g.edge_index.cpu(), g.x.shape[0])}


@pytest.mark.parametrize("small", [False, True])
@pytest.mark.parametrize("case", ["random", "random_sorted_by_source", "golden"])
def test_structures_get_the_plans_of_the_torch_route(case, small, monkeypatch):
    ei, n = _edge_lists()[case]
    monkeypatch.setattr(G, "SMALL_STRUCTURE", small)
    e = ei.shape[1]
    for ct in sorted({1, 16, tiles_for(e, "for_e")}):
        for hold_src in (False, True):
            sts = []
            for kernel in (True, False):
                monkeypatch.setattr(G, "PLAN_KERNEL", kernel)
                st = EdgeStructure(ei.to(DEV), n)
                if hold_src:
                    st.by_src
                sts.append((st, st.runsum_plan(ct), st.csr_plan("dst", ct), st.csr_plan("src", ct)))
            (a, ra, da, sa), (b, rb, db, sb) = sts
            srt = bool((ei[0, 1:] >= ei[0, :-1]).all())
            assert srt == (case == "random_sorted_by_source") or case == "golden"
            assert (ra is None) == (rb is None) == (not srt)
            if ra is not None:
                plans_equal(ra, rb, (case, ct, "runsum"))
                plans_equal(ra, sa, (case, ct, "a source-sorted list is its own by-source order"))
            plans_equal(da, db, (case, ct, "dst"))
            plans_equal(sa, sb, (case, ct, "src"))


def test_runsum_plan_of_a_sorted_list_sorts_nothing(monkeypatch):
    ei, n = _edge_lists()["random_sorted_by_source"]
    monkeypatch.setattr(G, "SMALL_STRUCTURE", False)

    def no_sort(*a, **k):
        raise AssertionError("runsum_plan built a CSR order")

    monkeypatch.setattr(G, "build_csr", no_sort)
    st = EdgeStructure(ei.to(DEV), n)
    plan = st.runsum_plan(16)
    assert st._by_src is None and st._by_dst is None
    plans_equal(plan, EdgeStructure._plan_of_sorted_keys(st.edge_index[0], n, 16))
    empty = EdgeStructure(torch.zeros(2, 0, dtype=torch.int64, device=DEV), 5)
    assert empty.runsum_plan(16) is None


def test_an_empty_structure_has_no_plan():
    empty = EdgeStructure(torch.zeros(2, 0, dtype=torch.int64, device=DEV), 5)
    assert empty.csr_plan("dst", 16) is None and empty.csr_plan("src", 1) is None


def test_a_rectangular_structure(monkeypatch):
    """a destination-partitioned shard: local target ids, global source ids (num_src > num_nodes)"""
    gen = torch.Generator().manual_seed(5)
    n_dst, n_src, e = 300, 1100, 5000
    src = torch.sort(torch.randint(0, n_src - 40, (e,), generator=gen)).values        # (the last sources have no edge)
    dst = torch.randint(0, n_dst, (e,), generator=gen)
    ei = torch.stack([src, dst]).to(DEV)
    for ct in (1, 16):
        sts = []
        for kernel in (True, False):
            monkeypatch.setattr(G, "PLAN_KERNEL", kernel)
            st = EdgeStructure(ei, n_dst, num_src=n_src)
            sts.append((st.csr_plan("dst", ct), st.csr_plan("src", ct), st.runsum_plan(ct)))
        for got, want, by in zip(sts[0], sts[1], ("dst", "src", "runsum")):
            plans_equal(got, want, (by, ct))
        assert sts[0][0].part_rowptr.shape[0] == n_dst + 1 and sts[0][1].part_rowptr.shape[0] == n_src + 1


# ------------------------------------------------------------------------------------------------------------------
# the packed sites (graph.carve): every table aligned, disjoint from its neighbours, and the general route's table
# ------------------------------------------------------------------------------------------------------------------
def _general_tables(ei, n, ct):
    """{"dst" | "src": (CSR, plan)} of a device list by the general route: build_csr and _plan_of_sorted_keys"""
    out = {}
    for by, row in (("dst", 1), ("src", 0)):
        csr = G.build_csr(ei, n, row)
        out[by] = csr, EdgeStructure._plan_of_sorted_keys(ei[row][csr.perm.long()], n, ct)
    return out


def _csr_equal(got, want, what):
    for f in ("rowptr", "other", "perm"):
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (what, f)


def _aligned_and_disjoint(tables, what):
    """the tensors of one packed site: each starts on 16 bytes, no two share a byte"""
    spans = sorted((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in tables if t.numel())
    assert len(spans) == len(tables) and all(lo % 16 == 0 for lo, _ in spans), what
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), what


def _plan_tables(plan):
    return [plan.part_off, plan.part_rowptr, plan.keys, plan.last]


def _two_sub_graphs(ei, n):
    """sub-graphs of n and n + 1 nodes (so the batch's row pointers have an odd length) over the list and its front part"""
    from types import SimpleNamespace
    from pangnn_amd.subgraphs import SubGraphDataset
    e = ei.shape[1]
    subs = []
    for nodes, edges, nb in ((n, ei, ei.flip(0)[:, :(e + 1) // 2]), (n + 1, ei[:, :max(e - 1, 1)], ei.flip(0))):
        k = edges.shape[1]
        subs.append(SimpleNamespace(x=torch.ones(nodes, 1), edge_index=edges, neighbour_edge_index=nb,
                                    edge_attr=torch.arange(1, k + 1, dtype=torch.float32), y=torch.zeros(k)))
    return SubGraphDataset.from_data_list(subs, device=DEV)


@pytest.mark.parametrize("n,e", [(1, 1), (2, 3), (7, 5), (6, 33), (97, 1000)])
def test_every_packed_site_hands_out_aligned_disjoint_tables_of_the_general_route(n, e, monkeypatch):
    """segment lengths that are no multiple of their alignment unit (N + 1 odd, E below and just past one tile), through the
    small build, `filtered` with both orders held, gcn_norm with and without weights and a padded batch's order tables"""
    host_ei, host_w = random_graph(n, e, seed=n + e)
    ei, w = host_ei.to(DEV), host_w.to(DEV)
    ct = G.chunk_tiles_for(e)
    monkeypatch.setattr(G, "SMALL_STRUCTURE", False)
    monkeypatch.setattr(G, "PLAN_KERNEL", False)
    want = _general_tables(ei, n, ct)
    general = EdgeStructure(ei.clone(), n)
    assert general.by_dst is not None and not general._small_built

    monkeypatch.setattr(G, "SMALL_STRUCTURE", True)              # the small build
    st = EdgeStructure(ei, n)
    got = {"dst": (st.by_dst, st.csr_plan("dst", ct)), "src": (st.by_src, st.csr_plan("src", ct))}
    assert st._small_built
    for by in ("dst", "src"):
        _csr_equal(got[by][0], want[by][0], ("small", by))
        plans_equal(got[by][1], want[by][1], ("small", by))
    _aligned_and_disjoint([t for c, p in got.values() for t in [c.rowptr, c.other, c.perm] + _plan_tables(p)], "small")

    keep = (torch.arange(e) % 3 != 1).to(DEV)                    # filtered, both orders held by the parent
    child, kept_id, _ = EdgeStructure.filtered(st, keep)
    k = child.num_edges
    assert k == int(keep.sum()) > 0 and child._by_src is not None and child.filter_state.tolist() == [k, 0]
    assert torch.equal(child.edge_index, ei[:, keep]) and torch.equal(kept_id.long(), torch.nonzero(keep).view(-1))
    of_child = _general_tables(child.edge_index, n, 1)
    _csr_equal(child._by_dst, of_child["dst"][0], "filtered dst")
    _csr_equal(child._by_src, of_child["src"][0], "filtered src")
    _aligned_and_disjoint([t for c in (child._by_dst, child._by_src) for t in (c.rowptr, c.other, c.perm)]
                          + [child.filter_state], "filtered")

    for weight in (None, w):                                      # gcn_norm
        a, b = st.gcn_norm(weight), general.gcn_norm(weight)
        tables = [(x.deg_inv_sqrt, x.by_dst, x.orig, x.by_src) for x in (a, b)]
        assert a._by_src_buf is not None and a.by_src is a._by_src_buf
        for f, ta, tb in zip(("deg_inv_sqrt", "by_dst", "orig", "by_src"), *tables):
            assert ta.dtype == tb.dtype == torch.float32 and ta.shape == tb.shape and torch.equal(ta, tb), ("norm", f)
        assert bool(torch.isfinite(torch.cat(tables[0])).all())
        _aligned_and_disjoint(tables[0], "norm")

    ds = _two_sub_graphs(host_ei, n)                             # a padded batch's order tables
    spec = ds.padded_spec(2)
    assert spec.nodes == 2 * n + 2 and spec.edges == e + max(e - 1, 1)
    buf = ds.padded_buffers(spec)
    assert buf.orders is not None
    ds.set_graph_ids(buf, [1, 0])
    ds.collate_padded(buf)
    pct = buf.orders.chunk_tiles
    assert pct == G.chunk_tiles_for(spec.edges) and buf.orders.n_chunks == G.n_chunks(spec.edges, pct)
    packed = [buf.edge_index, buf.neighbour_edge_index, buf.ptr, buf.batch, buf.live, buf.graph_ids, buf.edge_attr, buf.y, buf.x]
    for name, lst in (("sim", buf.edge_index), ("nb", buf.neighbour_edge_index)):
        of_batch = _general_tables(lst.clone(), spec.nodes, pct)
        made = buf._pangnn_structs[name][1]
        for by in ("dst", "src"):
            t = buf.orders.tables[f"{name}_{by}"]
            csr = made.by_dst if by == "dst" else made.by_src
            assert csr.rowptr is t["rowptr"] and csr.other is t["other"] and csr.perm is t["perm"]
            _csr_equal(csr, of_batch[by][0], (name, by))
            assert t["keys"].dtype == torch.int32 and torch.equal(t["keys"], of_batch[by][1].keys), (name, by)
            assert ("part_off" in t) == ("part_rowptr" in t) == ("last_part" in t) == (name == "sim")
            if name == "sim":
                plans_equal(made.csr_plan(by, pct), of_batch[by][1], (name, by))
                assert made.csr_plan(by, pct).last is t["last_part"]
            packed += list(t.values())
    _aligned_and_disjoint(packed, "padded batch")


def _sub_sampled_step(skip, kernel, monkeypatch):
    G.clear_cache()
    monkeypatch.setattr(G, "PLAN_KERNEL", kernel)
    g = _golden()
    torch.manual_seed(0)
    model = pangnn_amd.AlternateGCN(DEV, None, False, dims=[64, 128], skip_connections=skip, decoder="mlp")
    opt = make_optimizer(model)
    pw = ((g.y == 0).sum() / g.y.sum()).float()
    batch = sub_sample_graph_edges(g, DEV, fraction=0.8, generator=torch.Generator(device=DEV).manual_seed(17))
    loss, logits = train_step(model, opt, batch, batch.y, pw)
    out = loss.clone(), logits.clone(), [p.detach().clone() for p in model.parameters()]
    release(batch)
    return out


@pytest.mark.parametrize("skip", [False, True])
def test_a_sub_sampled_step_needs_no_index_op_plan(skip, monkeypatch):
    monkeypatch.setattr(G, "SMALL_STRUCTURE", False)              # the general route: the plans are built on first use
    want = _sub_sampled_step(skip, False, monkeypatch)

    def refuse(*a, **k):
        raise AssertionError("the step took the index-op plan route")

    monkeypatch.setattr(EdgeStructure, "_plan_of_sorted_keys", staticmethod(refuse))
    got = _sub_sampled_step(skip, True, monkeypatch)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert len(got[2]) == len(want[2]) > 0
    for a, b in zip(got[2], want[2]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------
# which plans carry a stream (EdgeStructure._streams), producer by producer
# ------------------------------------------------------------------------------------------------------------------
N_NODES = 512


def _sorted_list(e, seed=0):
    gen = torch.Generator().manual_seed(seed)
    src = torch.sort(torch.randint(0, N_NODES, (e,), generator=gen)).values
    return torch.stack([src, torch.randint(0, N_NODES, (e,), generator=gen)]).to(DEV)


def _whole(e):
    return EdgeStructure(_sorted_list(e), N_NODES)


def _filtered_child(e):
    parent = _whole(e)
    parent.by_src
    keep = torch.rand(e, generator=torch.Generator().manual_seed(1)) < 0.8
    child = EdgeStructure.filtered(parent, keep.to(DEV))[0]
    assert child.filter_state is not None and child._by_src is not None and 0 < child.num_edges < e
    return child


def _adopted_without_plans(e):
    """tables handed over without plans, as a collated batch's neighbour list has them: the plan kernel makes its plans"""
    made = _whole(e)
    return EdgeStructure(made.edge_index, N_NODES).adopt_tables(made.by_dst, made.by_src)


def test_which_plans_carry_a_stream(monkeypatch):
    """every producer EdgeStructure._streams names: (run-sum, by-target, by-source) plan with a stream or without; then one
    decoder_loss step through the native registry, whose gradients are those of the same step on plans without streams"""
    from pangnn_amd import functional as PF, torch_ops
    big, more, small = 20000, 140000, 3000          # above the small build's 16384 edges; two-tile chunks; the small build
    assert (PF.d16_chunk(big), PF.d16_chunk(more), PF.d16_chunk(small)) == (1, 2, 1)
    d16 = None                                      # the S / T kernels' chunk size of the structure's own edge count
    table = [("whole graph", lambda: _whole(big), d16, (True, True, False)),
             ("whole graph, not the kernels' chunk size", lambda: _whole(big), 16, (False, False, False)),
             ("whole graph, two-tile chunks", lambda: _whole(more), d16, (True, True, False)),
             ("whole graph, one-tile chunks of a longer list", lambda: _whole(more), 1, (False, False, False)),
             ("small build", lambda: _whole(small), d16, (False, False, False)),
             ("adopted tables", lambda: _adopted_without_plans(big), d16, (False, False, False)),
             ("rectangular", lambda: EdgeStructure(_sorted_list(big), N_NODES, num_src=2 * N_NODES), d16, (False, False, False)),
             ("filtered child", lambda: _filtered_child(big), d16, (False, True, False)),
             ("index-op route", lambda: _whole(big), d16, (False, False, False))]
    for what, make, ct, want in table:
        monkeypatch.setattr(G, "PLAN_KERNEL", what != "index-op route")
        st = make()
        e = st.num_edges
        ct = PF.d16_chunk(e) if ct is None else ct
        plans = st.runsum_plan(ct), st.csr_plan("dst", ct), st.csr_plan("src", ct)
        assert st._small_built == (what in ("small build", "adopted tables")), what
        assert tuple(p.stream is not None for p in plans) == want, what
        assert [st._streams(kind, ct) for kind in ("run", "dst", "src")] == list(want), what
        for p, shape in zip(plans, (((e + 31) // 32 * 32, 2), (e,), None)):
            assert p.chunk_tiles == ct and (p.stream is None or (p.stream.dtype == torch.int32 and p.stream.shape == shape)), what
    monkeypatch.setattr(G, "PLAN_KERNEL", True)

    st = _whole(big)
    ct = PF.d16_chunk(big)
    gen = torch.Generator().manual_seed(2)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(DEV)          # noqa: E731
    leaves = [rnd(N_NODES, 128) / 4, rnd(64, 64) / 8, rnd(64) / 8, rnd(64) / 8, rnd(1) / 8]
    y, pw = (torch.rand(big, generator=gen) < 0.3).float().to(DEV), torch.tensor(2.5, device=DEV)
    need = G.NEED_BY_DST | G.NEED_RUNSUM | G.NEED_PLAN_DST
    res = []
    for stream in (True, False):
        plans = st.runsum_plan(ct), st.csr_plan("dst", ct)
        if not stream:
            for p in plans:
                p.stream = None
        assert all((p.stream is not None) == stream for p in plans)
        st.push_native(need, force=True)
        pq, w2, b2, w3, b3 = ws = [t.clone().requires_grad_(True) for t in leaves]
        loss, logits = torch_ops.decoder_loss_pq(pq, st, None, None, w2, b2, w3, b3, y, pw, big)
        loss.backward()
        res.append([loss.detach(), logits.detach()] + [t.grad for t in ws])
    assert bool(torch.isfinite(res[0][0]).all()) and all(bool(g.abs().sum() > 0) for g in res[0][2:])
    for a, b in zip(*res):
        assert torch.equal(a, b)
