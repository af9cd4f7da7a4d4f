"""A structure derived by filtering (EdgeStructure.filtered / pangnn_structure_filter, csrc/edge_filter.hip) and the
sub-sampled training step built on it (pangnn_amd/sampling.py).  There is no tolerance anywhere: the referee for the tables
is build_csr on the child's edge list, the referee for the step is the same model on a fresh `Data` of cloned tensors, and
every comparison is torch.equal."""
import gc

import pytest
import torch

from conftest import load_golden, random_graph
import pangnn_amd
from pangnn_amd import _lib
from pangnn_amd import functional as PF
from pangnn_amd.data import Data
from pangnn_amd.graph import CSR, EdgeStructure, build_csr, structure_of
from pangnn_amd.sampling import filter_edges, release, sub_sample_graph_edges
from pangnn_amd.train import make_optimizer, train_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def parent_of(ei, n, both=True):
    """a parent whose tables come from the general radix-sort build (never the one-launch small build)"""
    st = EdgeStructure(ei, n)
    st._by_dst = build_csr(ei, n, 1)
    if both:
        st._by_src = build_csr(ei, n, 0, validate=False)
    return st


def same_csr(a: CSR, b: CSR):
    assert a.rowptr.dtype == b.rowptr.dtype == torch.int64 and a.other.dtype == b.other.dtype == torch.int32
    assert torch.equal(a.rowptr, b.rowptr), "rowptr"
    assert torch.equal(a.other, b.other), "other"
    assert torch.equal(a.perm, b.perm), "perm"


def check_filtered(ei, n, keep, both=True, give_count=False, arrays=True):
    """derive the child of (ei, keep) and hold everything it carries against what exists today; returns (child, scratch)"""
    ei = ei.to(DEV)
    e = ei.shape[1]
    on = (keep != 0).to(DEV)
    keep = keep.to(DEV)
    gen = torch.Generator().manual_seed(e + n)
    w, y = torch.rand(e, generator=gen).to(DEV), (torch.rand(e, generator=gen) < 0.3).float().to(DEV)
    parent = parent_of(ei, n, both)
    before = [t.clone() for t in (ei, parent._by_dst.rowptr, parent._by_dst.other, parent._by_dst.perm)]
    child, kept_id, outs = EdgeStructure.filtered(parent, keep, int(on.sum()) if give_count else None,
                                                  [w, y] if arrays else [])
    ids = torch.nonzero(on).view(-1)
    assert child.num_edges == ids.numel() and child.num_nodes == n
    assert child.edge_index.dtype == torch.int64 and torch.equal(child.edge_index, ei[:, on])
    assert kept_id.dtype == torch.int32 and torch.equal(kept_id.long(), ids)
    if arrays:
        assert torch.equal(outs[0], w[on]) and torch.equal(outs[1], y[on])
    assert child.filter_state.tolist() == [ids.numel(), 0]
    child.check_filter()
    assert child._by_dst is not None and (child._by_src is not None) == both        # derived: nothing left to build
    scratch = parent_of(child.edge_index.clone(), n, True)
    same_csr(child._by_dst, scratch._by_dst)
    same_csr(child.by_src, scratch._by_src)                      # derived, or built lazily when the parent had none
    assert child.hints["valid_ids"] is True and child.hints["band_width"] == 0
    for t, b in zip((ei, parent._by_dst.rowptr, parent._by_dst.other, parent._by_dst.perm), before):
        assert torch.equal(t, b)                                 # the parent is read only
    return child, scratch


def random_keep(e, rate, seed):
    return torch.rand(e, generator=torch.Generator().manual_seed(seed)) < rate


def test_empty_graph_and_degenerate_selections():
    n = 50
    check_filtered(torch.zeros(2, 0, dtype=torch.int64), n, torch.zeros(0, dtype=torch.bool))
    check_filtered(torch.zeros(2, 0, dtype=torch.int64), 0, torch.zeros(0, dtype=torch.bool), both=False)
    check_filtered(torch.tensor([[2], [1]]), 3, torch.ones(1, dtype=torch.bool))     # one edge, kept
    ei, _ = random_graph(n, 700, seed=1)
    check_filtered(ei, n, torch.zeros(700, dtype=torch.bool))                        # keep nothing
    check_filtered(ei, n, torch.zeros(700, dtype=torch.bool), give_count=True, arrays=False)
    child, _ = check_filtered(ei, n, torch.ones(700, dtype=torch.bool))              # keep everything: the parent's tables
    parent = parent_of(ei.to(DEV), n)
    same_csr(child._by_dst, parent._by_dst)
    same_csr(child._by_src, parent._by_src)
    for one in (0, 350, 699):                                                        # exactly one kept edge
        keep = torch.zeros(700, dtype=torch.bool)
        keep[one] = True
        check_filtered(ei, n, keep, give_count=(one == 350))


@pytest.mark.parametrize("rate", [0.05, 0.5, 0.95])
@pytest.mark.parametrize("e", [1, 255, 256, 257, 4097, 70001])
def test_random_selection_at_scan_block_boundaries(e, rate):
    n = max(3, e // 7)
    ei, _ = random_graph(n, e, seed=e)
    check_filtered(ei, n, random_keep(e, rate, seed=e + int(100 * rate)), both=(e % 2 == 1), give_count=(e % 3 == 0))


@pytest.mark.parametrize("side", [1, 0])
def test_rows_emptied_whole(side):
    """every in-edge (side 1) / out-edge (side 0) of row 0, of the last row that has any, and of a run of adjacent rows
    dropped; the graph keeps its isolated nodes, duplicates and self loops"""
    n, e = 400, 6000
    ei, _ = random_graph(n, e, seed=7)
    ends = ei[side]
    last = int(ends.max())
    for rows in ([0], [last], [n - 1], list(range(100, 131)), [0, last] + list(range(200, 212))):
        keep = ~torch.isin(ends, torch.tensor(rows))
        child, _ = check_filtered(ei, n, keep)
        csr = child._by_dst if side == 1 else child._by_src
        lens = (csr.rowptr[1:] - csr.rowptr[:-1]).cpu()
        assert bool((lens[torch.tensor(rows)] == 0).all())


def test_hub_row_keeps_its_segments_and_propagates_bit_equal():
    n, e = 2000, 20000
    ei, w = random_graph(n, e, seed=3, hub=9000)
    keep = random_keep(e, 0.8, seed=5)
    keep[:9000] = True
    keep[8700:9000] = False                                      # 8700 > LONG_ROW of the hub's entries stay
    child, scratch = check_filtered(ei, n, keep)
    assert child.hints["short_rows"] is False
    got, want = child._by_dst.long_rows(), scratch._by_dst.long_rows()
    assert got is not None and want is not None
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    wk = w.to(DEV)[keep.to(DEV)]
    x = torch.rand(n, 64, generator=torch.Generator().manual_seed(0)).to(DEV)
    res = []
    for st in (child, scratch):
        xs = x.clone().requires_grad_(True)
        out = PF.propagate(xs, None, st, st.gcn_norm(wk.clone()))
        out.backward(torch.ones_like(out) * x)                   # the transposed propagate
        res.append((out.detach(), xs.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8, torch.int32, torch.float32])
def test_keep_is_read_at_its_stored_width(dtype):
    n, e = 300, 4097
    ei, _ = random_graph(n, e, seed=11)
    keep = random_keep(e, 0.6, seed=2)
    values = keep if dtype is torch.bool else keep.to(dtype) * 3                     # any non-zero value keeps
    assert values.dtype is dtype
    if dtype is torch.int32:
        values = values * 256                                                        # low byte zero: a whole word is read
    check_filtered(ei, n, values)


def plans_equal(a, b):
    assert (a is None) == (b is None)
    if a is not None:
        assert a.n_parts == b.n_parts and a.chunk_tiles == b.chunk_tiles
        assert torch.equal(a.part_off, b.part_off) and torch.equal(a.part_rowptr, b.part_rowptr)
        assert torch.equal(a.keys, b.keys)


@pytest.mark.parametrize("order", ["random", "source_sorted", "golden"])
def test_edge_order_and_the_decoder_plans(order):
    if order == "golden":
        f = load_golden("cfg2_sim_1000x5")
        ei, n = torch.from_numpy(f["whole_edge_index"]), int(f["num_nodes"])
    else:
        n = 900
        ei, _ = random_graph(n, 9000, seed=13)
        if order == "source_sorted":
            ei = ei[:, torch.sort(ei[0], stable=True).indices]
    e = ei.shape[1]
    child, scratch = check_filtered(ei, n, random_keep(e, 0.8, seed=4), give_count=True)
    srt = bool((ei[0][1:] >= ei[0][:-1]).all())
    assert child.hints["sorted_by_src"] is srt and child.sorted_by_src() is srt
    ct = int(_lib.load().pangnn_decoder_chunk_tiles_for(child.num_edges))
    for tiles in (1, ct):
        plans_equal(child.runsum_plan(tiles), scratch.runsum_plan(tiles))
        assert (child.runsum_plan(tiles) is not None) == srt
        plans_equal(child.csr_plan("dst", tiles), scratch.csr_plan("dst", tiles))
        plans_equal(child.csr_plan("src", tiles), scratch.csr_plan("src", tiles))
    child.push_native(pangnn_amd.graph.NEED_BY_DST | pangnn_amd.graph.NEED_BY_SRC | pangnn_amd.graph.NEED_RUNSUM |
                      pangnn_amd.graph.NEED_PLAN_DST | pangnn_amd.graph.NEED_PLAN_SRC | pangnn_amd.graph.NEED_NORM)
    pangnn_amd.graph.forget(pangnn_amd.graph.structure_key(child.edge_index, n), child.edge_index)


def test_rectangular_structure_and_bad_arguments_raise():
    ei, _ = random_graph(100, 500, seed=1)
    ei = ei.to(DEV)
    with pytest.raises(ValueError, match="square"):
        EdgeStructure.filtered(EdgeStructure(ei, 100, num_src=200), torch.ones(500, dtype=torch.bool, device=DEV))
    st = parent_of(ei, 100)
    with pytest.raises(ValueError):
        EdgeStructure.filtered(st, torch.ones(499, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError):
        EdgeStructure.filtered(st, torch.ones(500, dtype=torch.bool, device=DEV), num_kept=501)


@pytest.mark.parametrize("delta", [-37, 41])
def test_wrong_num_kept_sets_the_status_and_writes_nothing_outside(delta):
    """an argument check, not a fault test: every output is allocated at the CLAIMED size plus a poisoned guard region,
    the call returns, the status word says so and the guard is untouched"""
    lib = _lib.load()
    n, e, guard = 300, 1000, 512
    ei, _ = random_graph(n, e, seed=21)
    ei = ei.to(DEV)
    keep = random_keep(e, 0.5, seed=3).to(DEV)
    true = int(keep.sum())
    claim = true + delta
    w = torch.rand(e, device=DEV)
    p = parent_of(ei, n)

    def poisoned(count, dtype, poison):
        return torch.full((count + guard,), poison, dtype=dtype, device=DEV)

    c_ei = poisoned(2 * claim, torch.int64, -7)
    kept_id, c_w = poisoned(claim, torch.int32, -7), poisoned(claim, torch.float32, -7.0)
    rp = [poisoned(n + 1, torch.int64, -7) for _ in range(2)]
    ot = [poisoned(claim, torch.int32, -7) for _ in range(2)]
    pm = [poisoned(claim, torch.int32, -7) for _ in range(2)]
    state = poisoned(2, torch.int32, -7)
    ws_bytes = lib.pangnn_structure_filter_workspace_bytes(e)
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    rc = lib.pangnn_structure_filter(
        ei.data_ptr(), e, e, n, keep.data_ptr(), 1, claim,
        p._by_dst.rowptr.data_ptr(), p._by_dst.other.data_ptr(), p._by_dst.perm.data_ptr(),
        p._by_src.rowptr.data_ptr(), p._by_src.other.data_ptr(), p._by_src.perm.data_ptr(), w.data_ptr(), None,
        c_ei.data_ptr(), claim, kept_id.data_ptr(), c_w.data_ptr(), None,
        rp[0].data_ptr(), ot[0].data_ptr(), pm[0].data_ptr(), rp[1].data_ptr(), ot[1].data_ptr(), pm[1].data_ptr(),
        state.data_ptr(), state[1:].data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    count, status = state[:2].tolist()
    assert count == true and status == 1
    for buf, used in [(c_ei, 2 * claim), (kept_id, claim), (c_w, claim), (state, 2)] + [(t, n + 1) for t in rp] + \
            [(t, claim) for t in ot + pm]:
        assert bool((buf[used:] == -7).all()), "guard region written"
    m = min(claim, true)
    ids = torch.nonzero(keep).view(-1)
    assert torch.equal(c_ei[:2 * claim].view(2, claim)[:, :m], ei[:, ids[:m]])
    assert torch.equal(kept_id[:m].long(), ids[:m]) and torch.equal(c_w[:m], w[ids[:m]])
    if claim > true:                                             # the missing tail is defined and belongs to no row
        assert bool((c_ei[:2 * claim].view(2, claim)[:, true:] == 0).all()) and bool((kept_id[true:claim] == 0).all())
    for k in range(2):
        assert int(rp[k][0]) == 0 and int(rp[k][n]) == m and bool((rp[k][1:n + 1] >= rp[k][:n]).all())
        assert bool(((pm[k][:claim] >= 0) & (pm[k][:claim] < claim)).all())
        assert bool(((ot[k][:claim] >= 0) & (ot[k][:claim] < n)).all())
    # the Python constructor reports it on request
    child, _, _ = EdgeStructure.filtered(p, keep, num_kept=claim)
    with pytest.raises(ValueError, match="num_kept"):
        child.check_filter()


# ------------------------------------------------------------------------------------------------------------------
# end to end: the reference's loop with pangnn.py:190 uncommented
# ------------------------------------------------------------------------------------------------------------------
def golden_graph(name):
    f = load_golden(name)
    return Data(x=torch.from_numpy(f["whole_x"]).to(DEV), edge_index=torch.from_numpy(f["whole_edge_index"]).to(DEV),
                edge_attr=torch.from_numpy(f["whole_edge_attr"]).to(DEV), y=torch.from_numpy(f["whole_y"]).to(DEV),
                neighbour_edge_index=torch.from_numpy(f["whole_neighbour_edge_index"]).to(DEV))


_GRAPHS = {}


def shared_graph(name):
    if name not in _GRAPHS:
        _GRAPHS[name] = golden_graph(name)
    return _GRAPHS[name]


def step(model, graph, pos_weight):
    model.zero_grad(set_to_none=True)
    loss, logits = model.loss_and_logits(graph, graph.y, pos_weight)
    loss.backward()
    return loss.detach().clone(), logits.detach().clone(), [p.grad.clone() for p in model.parameters() if p.grad is not None]


@pytest.mark.parametrize("decoder", ["mlp", "cosine"])
@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("name", ["cfg2_sim_1000x5", "sim_200x4"])
def test_sub_sampled_step_equals_the_step_on_a_fresh_graph(name, skip, decoder, monkeypatch):
    g = golden_graph(name)                                       # a parent that is never stepped on, only sub-sampled
    e = g.edge_index.shape[1]
    gen = torch.Generator(device=DEV).manual_seed(17)
    batch = sub_sample_graph_edges(g, DEV, fraction=0.8, generator=gen)
    assert batch.edge_index.shape[1] == e - int(e * (1 - 0.8)) and batch.x is g.x
    assert batch.neighbour_edge_index is g.neighbour_edge_index
    assert torch.equal(batch.edge_index, g.edge_index[:, batch.kept_edge_id])
    assert torch.equal(batch.edge_attr, g.edge_attr[batch.kept_edge_id]) and torch.equal(batch.y, g.y[batch.kept_edge_id])
    assert float(batch.y.sum()) == float(g.y.sum())                                  # every positive stays
    st = structure_of(batch.edge_index, g.num_nodes, holder=batch, name="sim")
    assert st.filter_state is not None                                               # the derived one, found by the model
    assert st._by_dst is not None and st._by_src is not None                         # BOTH orders derived, none left to sort
    assert st.hints["short_rows"] is True and st._by_src._long is False              # nor a longest-row read-back
    assert structure_of(batch.neighbour_edge_index, g.num_nodes, holder=batch, name="nb") is \
        structure_of(g.neighbour_edge_index, g.num_nodes, holder=g, name="nb")
    fresh = Data(x=g.x.clone(), edge_index=batch.edge_index.clone(), edge_attr=batch.edge_attr.clone(), y=batch.y.clone(),
                 neighbour_edge_index=g.neighbour_edge_index.clone())
    torch.manual_seed(0)
    model = pangnn_amd.AlternateGCN(DEV, None, False, dims=[64, 128], skip_connections=skip, decoder=decoder)
    pw = ((g.y == 0).sum() / g.y.sum()).float()
    real_build = pangnn_amd.graph.build_csr

    def no_sort(edge_index, *args, **kwargs):
        assert edge_index.data_ptr() != batch.edge_index.data_ptr(), "the step sorted the sub-sample's edge list"
        return real_build(edge_index, *args, **kwargs)           # (the neighbour graph's own one-time build)

    with monkeypatch.context() as m:
        m.setattr(pangnn_amd.graph, "build_csr", no_sort)
        got = step(model, batch, pw)
    want = step(model, fresh, pw)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert len(got[2]) == len(want[2]) > 0
    for a, b in zip(got[2], want[2]):
        assert torch.equal(a, b)
    st.check_filter()
    release(batch)


def test_the_reference_loop_with_line_190_uncommented_runs():
    g = shared_graph("sim_200x4")
    torch.manual_seed(0)
    model = pangnn_amd.AlternateGCN(DEV, None, False, dims=[64, 128])
    model.train()
    optimizer = make_optimizer(model)
    criterion = pangnn_amd.BCEWithLogitsLoss(pos_weight=((g.y == 0).sum() / g.y.sum()).float())
    gen = torch.Generator(device=DEV).manual_seed(1)
    seen = []
    for _ in range(2):
        batch = pangnn_amd.sub_sample_graph_edges(g, DEV, fraction=0.8, generator=gen)
        optimizer.zero_grad()
        output = model(batch)
        assert isinstance(output, pangnn_amd.DeferredLogits)
        loss = criterion(output, batch.y)
        loss.backward()
        optimizer.step()
        assert bool(torch.isfinite(loss)) and all(p.grad is not None for p in model.mlp.parameters())
        seen.append(batch.kept_edge_id.clone())
    assert seen[0].shape == seen[1].shape and not torch.equal(seen[0], seen[1])      # a fresh subset per step


def test_same_seed_same_subset_and_filter_edges_by_mask():
    g = shared_graph("cfg2_sim_1000x5")
    a = sub_sample_graph_edges(g, generator=torch.Generator(device=DEV).manual_seed(5))
    b = sub_sample_graph_edges(g, generator=torch.Generator(device=DEV).manual_seed(5))
    c = sub_sample_graph_edges(g, generator=torch.Generator(device=DEV).manual_seed(6), sample_pos_edges=True)
    assert torch.equal(a.kept_edge_id, b.kept_edge_id) and a.kept_edge_id.shape == c.kept_edge_id.shape
    assert not torch.equal(a.kept_edge_id, c.kept_edge_id) and float(c.y.sum()) < float(g.y.sum())
    keep = torch.zeros(g.edge_index.shape[1], dtype=torch.int32, device=DEV)
    keep[a.kept_edge_id] = 1
    d = filter_edges(g, keep)                                    # the count is read back
    assert torch.equal(d.edge_index, a.edge_index) and torch.equal(d.kept_edge_id, a.kept_edge_id)
    with pytest.raises(ValueError, match="union"):
        sub_sample_graph_edges(Data(x=g.x, edge_index=g.edge_index, y=g.y, union_edge_index=g.edge_index))
    for t in (a, b, c, d):
        release(t)


def test_repeated_sub_sampling_does_not_accumulate_memory():
    n, e = 7000, 70000
    ei, w = random_graph(n, e, seed=9)
    y = (torch.rand(e, generator=torch.Generator().manual_seed(1)) < 0.05).float()
    g = Data(x=torch.ones(n, 1, device=DEV), edge_index=ei.to(DEV), edge_attr=w.to(DEV), y=y.to(DEV),
             neighbour_edge_index=torch.stack([torch.arange(n), torch.arange(n)]).to(DEV))
    torch.manual_seed(0)
    model = pangnn_amd.AlternateGCN(DEV, None, False, dims=[64, 128])
    optimizer = make_optimizer(model)
    pw = torch.tensor(19.0, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(2)
    used = []
    for _ in range(6):
        batch = sub_sample_graph_edges(g, DEV, fraction=0.8, generator=gen)
        loss, out = train_step(model, optimizer, batch, batch.y, pw)
        del batch, loss, out                                     # dropping the graph releases its tables (sampling.release)
        gc.collect()
        torch.cuda.synchronize()
        used.append(torch.cuda.memory_allocated())
    assert used[5] == used[2], used
