"""The T pass of the training decoder on its position-word stream (pangnn_decoder_dgrad_stream_f32, csrc/decoder16.hip) against
its keys route (pangnn_decoder_dgrad_f32) of the same library, and both against float64 — bit for bit.

The stream is tpos[k] = perm[k] | closes_k << 31 (pangnn_csr_plan_tpos): the by-target plan's edge id at position k and "a part
row ends behind k", built once per graph.  Both routes must write the same part rows into the same slots, touch no guard row,
and give the same dL/db2.  Inputs are on the exact grid of test_decoder_run_sums (every product and every partial sum in any
order is a float32), so a float64 evaluation is matched without a tolerance too — that is what holds T's mask value in place:
T multiplies a 2^-7 mask with images of 128 W2' and sums dL/db2 with the same half-word read as an IEEE-half 1.0."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_decoder_run_sums import (D, GUARD, SENTINEL, _dev_tables, _f32, call_S, chunk_tiles_expected, decoder_reference, dev,
                                   g_grid, grid_edges, grid_tables, part_layout)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------
# the graphs
# ------------------------------------------------------------------------------------------------------------------
DEGREES_3000 = [15, 1, 15, 1, 0, 600, 17, 1, 1, 1, 0, 600, 17, 1, 600, 0, 17, 1, 600, 0, 1, 17, 1, 1, 0, 17, 1, 1, 17, 0, 1, 1,
                17, 1, 0, 1, 17, 1, 1]
DEGREES_3000 = DEGREES_3000 + [3000 - sum(DEGREES_3000)]


def _shuffled(src, dst, seed):
    order = torch.randperm(src.numel(), generator=torch.Generator().manual_seed(seed))
    return src[order].contiguous(), dst[order].contiguous()


@functools.lru_cache(None)
def graph(name):
    """(src, dst, n): the caller's order is a seeded shuffle, so the by-target permutation is not the identity"""
    gen = torch.Generator().manual_seed(len(name) * 131 + 7)
    if name == "E33":                   # the last tile holds one live edge
        n, e = 9, 33
        dst = torch.randint(0, n, (e,), generator=gen)
    elif name == "E64-one-target":      # one run across both tiles; ends with the chunk
        n, e = 5, 64
        dst = torch.full((e,), 3, dtype=torch.int64)
    elif name == "E3000":               # 40 targets, designed in-degrees
        n, e = 40, 3000
        dst = torch.repeat_interleave(torch.arange(n), torch.tensor(DEGREES_3000))
    else:                               # long lists: runs of a few hundred positions over 257 targets, some targets empty
        n, e = 300, {"E70000": 70_000, "E140000": 140_000}[name]
        dst = torch.randint(0, 257, (e,), generator=gen)
    src = torch.randint(0, n, (e,), generator=gen)
    src, dst = _shuffled(src, dst, e)
    return src, dst, n


GRAPHS = ["E33", "E64-one-target", "E3000", "E70000", "E140000"]


def test_designed_graphs_have_the_designed_runs():
    deg = np.array(DEGREES_3000)
    assert len(deg) == 40 and deg.sum() == 3000 and deg.min() == 0 and {0, 1, 17, 600} <= set(deg.tolist())
    starts = (np.cumsum(deg) - deg)[deg > 0]
    assert {15, 16, 31} <= set((starts % 32).tolist())                       # a run starts at position 15, 16 and 31 of a tile
    ends = np.cumsum(deg)[deg > 0] - 1                                       # last position of every run
    assert np.bincount(ends // 16).max() >= 3                                # three or more runs end inside one half tile
    # the chunk sizes the lists select: one tile per chunk up to 131 040 edges, two from there (decoder16.hip, chunk_log_for)
    assert [chunk_tiles_expected(graph(g)[0].numel()) for g in GRAPHS] == [1, 1, 1, 1, 2]
    for name in ("E70000", "E140000"):
        src, dst, n = graph(name)
        span = 32 * chunk_tiles_expected(src.numel())
        keys = np.sort(dst.numpy())
        k = np.arange(span, len(keys), span)
        assert (keys[k] == keys[k - 1]).any() and (keys[k] != keys[k - 1]).any()   # runs cross chunk ends, and end at them
        assert np.bincount(keys, minlength=n).min() == 0


# ------------------------------------------------------------------------------------------------------------------
# one case: records from one S launch, the library's by-target plan with its stream, the float64 rows
# ------------------------------------------------------------------------------------------------------------------
def tpos_expected(perm, keys, span):
    """the stream's definition in plain torch, as non-negative int64 words"""
    e = keys.numel()
    k = torch.arange(e, device=keys.device)
    nxt = torch.clamp(k + 1, max=e - 1)
    closes = (k + 1 == e) | ((k + 1) % span == 0) | (keys[nxt] != keys)
    return perm.long() | (closes.long() << 31)


@functools.lru_cache(None)
def case(name):
    from pangnn_amd.graph import EdgeStructure
    src, dst, n = graph(name)
    e = src.numel()
    seed = 1000 + GRAPHS.index(name)
    t = grid_tables(n, seed)
    g, _, q = grid_edges(e, seed)
    # every partial sum of a run of dL/dh1 rows (|entry| <= 64 * 2 * 2 units of 1 / q each) and of dL/db2 is a float32
    assert int(torch.bincount(dst).max()) * 256 * q < 1 << 24 and e * 2 * q < 1 << 24 and q == g_grid(e)[0]
    td = _dev_tables(t)
    ei = torch.stack([src, dst]).to(dev()).contiguous()
    gd = g.to(dev())
    st = EdgeStructure(ei, n)
    csr = st.by_dst
    ct = chunk_tiles_expected(e)
    plan = EdgeStructure._plan_of_rowptr(csr.rowptr, e, ct, perm=csr.perm)
    s = call_S(td, td["P"], td["Q"], 0, n, ei, gd, None, None, None, None, 0)
    ref = decoder_reference({k: v.double() for k, v in td.items()}, ei[0], ei[1], gd.double(), rows=True)
    assert torch.equal(s.logits, _f32(ref["logits"]))
    keys = ei[1][csr.perm.long()]
    lay = part_layout(keys.cpu().numpy(), ct, n)
    assert torch.equal(plan.keys.long(), keys) and plan.part_off.cpu().tolist() == lay.part_off.tolist()
    return SimpleNamespace(name=name, e=e, n=n, td=td, ei=ei, g=gd, rec=s.rec, ref=ref, st=st, perm=csr.perm, plan=plan, lay=lay,
                           ct=ct, keys=keys)


def run_T(c, route, w2=None, want_b2=True):
    """one T launch through the C ABI on the case's records and plan; (parts with guard rows, dL/db2)"""
    from pangnn_amd import _lib as L
    lib = L.load()
    w2 = c.td["W2"] if w2 is None else w2
    parts = torch.full((c.lay.n_parts + GUARD, D), SENTINEL, dtype=torch.float32, device=dev())
    gb2 = torch.full((D,), SENTINEL, dtype=torch.float32, device=dev()) if want_b2 else None
    ws = torch.empty(lib.pangnn_decoder_dgrad_workspace_bytes(), dtype=torch.uint8, device=dev()) if want_b2 else None
    wsb = 0 if ws is None else ws.numel()
    if route == "stream":
        L.check(lib.pangnn_decoder_dgrad_stream_f32(c.rec.data_ptr(), c.plan.stream.data_ptr(), w2.data_ptr(), c.td["w3"].data_ptr(),
                                                    c.e, parts.data_ptr(), c.plan.part_off.data_ptr(), L.ptr(gb2), L.ptr(ws), wsb,
                                                    L.stream_ptr()), "pangnn_decoder_dgrad_stream_f32")
    else:
        L.check(lib.pangnn_decoder_dgrad_f32(c.rec.data_ptr(), c.perm.data_ptr(), c.plan.keys.data_ptr(), w2.data_ptr(),
                                             c.td["w3"].data_ptr(), c.e, parts.data_ptr(), c.plan.part_off.data_ptr(), L.ptr(gb2),
                                             None, L.ptr(ws), wsb, L.stream_ptr()), "pangnn_decoder_dgrad_f32")
    return parts, gb2


@functools.lru_cache(None)
def both_routes(name):
    c = case(name)
    return run_T(c, "keys"), run_T(c, "stream")


# ------------------------------------------------------------------------------------------------------------------
# tests
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAPHS)
def test_tpos_is_perm_with_the_close_bit(name):
    c = case(name)
    assert c.plan.stream.dtype == torch.int32 and c.plan.stream.shape == (c.e,)
    got = c.plan.stream.long() & 0xffffffff
    assert torch.equal(got, tpos_expected(c.perm, c.keys, 32 * c.ct))
    assert int((got >> 31).sum()) == c.lay.n_parts                            # one close bit per part row


@pytest.mark.parametrize("name", GRAPHS)
def test_stream_route_equals_keys_route(name):
    """part rows slot for slot (guard rows included: neither route writes past the plan's parts) and dL/db2"""
    c = case(name)
    (pk, bk), (ps, bs) = both_routes(name)
    print(f"{name}: E={c.e} parts={c.lay.n_parts} chunk tiles={c.ct}")
    assert torch.equal(ps, pk) and torch.equal(bs, bk)
    assert bool((ps[c.lay.n_parts:] == SENTINEL).all()) and bool((ps[:c.lay.n_parts] != SENTINEL).all())
    # the run sums alone (no dL/db2 asked for) take the same instances
    assert torch.equal(run_T(c, "stream", want_b2=False)[0], pk)


@pytest.mark.parametrize("name", GRAPHS)
def test_both_routes_equal_float64(name):
    """exact inputs: T's part rows, per-target sums and dL/db2 ARE the float64 values (the 2^-7 mask beside 128 W2' and the
    mixed-precision dL/db2 sums change no bit)"""
    from test_decoder_run_sums import sum_parts
    c = case(name)
    rows = c.ref["gh1"][c.perm.long()]
    want = torch.zeros(c.lay.n_parts, D, dtype=torch.float64, device=dev()).index_add_(
        0, torch.from_numpy(c.lay.part_id).to(dev()), rows)
    want_q = torch.zeros(c.n, D, dtype=torch.float64, device=dev()).index_add_(0, c.ei[1], c.ref["gh1"])
    for route, (parts, gb2) in zip(("keys", "stream"), both_routes(name)):
        assert torch.equal(parts[:c.lay.n_parts], _f32(want)), route
        assert torch.equal(sum_parts(parts[:c.lay.n_parts], c.lay.part_rowptr, c.n), _f32(want_q)), route
        assert torch.equal(gb2, _f32(c.ref["a"].sum(0))), route


@pytest.mark.parametrize("name", GRAPHS)
def test_T_equals_S_on_the_transposed_list(name):
    """the list with sources and targets swapped, in by-target order, is source-sorted: S's own by-source run parts of it (its
    second product, 1.0 masks beside W2') are T's by-target parts of the original, row for row"""
    c = case(name)
    p = c.perm.long()
    ei_t = torch.stack([c.ei[1][p], c.ei[0][p]]).contiguous()
    s = call_S(c.td, c.td["Q"], c.td["P"], 0, c.n, ei_t, c.g[p].contiguous(), None, None, None, c.plan.part_off, c.lay.n_parts)
    for parts, _ in both_routes(name):
        assert torch.equal(parts, s.parts)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("name", ["E3000", "E140000"])
def test_nonfinite_W2_reaches_the_same_outputs(name, bad):
    """a NaN / an inf in W2: the stream route's part rows and dL/db2 are non-finite exactly where the keys route's are (recorded
    in this run), and equal to it elsewhere"""
    c = case(name)
    w2 = c.td["W2"].clone()
    w2[5, 9] = bad
    (pk, bk), (ps, bs) = run_T(c, "keys", w2), run_T(c, "stream", w2)
    n = c.lay.n_parts
    assert not bool(torch.isfinite(pk[:n]).all()) and bool(torch.isfinite(pk[:n]).any())        # the poison arrives, not everywhere
    assert torch.equal(torch.isfinite(ps), torch.isfinite(pk)) and torch.equal(torch.isfinite(bs), torch.isfinite(bk))
    assert torch.equal(torch.isnan(ps), torch.isnan(pk)) and torch.equal(torch.isnan(bs), torch.isnan(bk))
    fin = torch.isfinite(pk)
    assert torch.equal(ps[fin], pk[fin]) and torch.equal(torch.nan_to_num(bs), torch.nan_to_num(bk))
    # dL/db2 does not read W2 at all: it is the clean value on both routes
    assert torch.equal(bk, both_routes(name)[0][1])


def test_structures_route_by_what_their_plan_carries():
    """a square structure's by-target plan from the plan kernel carries the stream and _dgrad_sum walks it; a plan without one
    (the small build of a mini-batch, a by-source plan, a padded batch with `live`) takes the keys route — same sums"""
    from pangnn_amd import functional as PF
    from pangnn_amd.graph import EdgeStructure
    c = case("E70000")
    st = EdgeStructure(c.ei, c.n)
    plan = st.csr_plan("dst", PF.d16_chunk(c.e))
    assert plan.stream is not None and torch.equal(plan.stream, c.plan.stream)
    assert st.csr_plan("src", PF.d16_chunk(c.e)).stream is None
    small = case("E3000")
    assert EdgeStructure(small.ei, small.n).csr_plan("dst", PF.d16_chunk(small.e)).stream is None
    w2, w3 = c.td["W2"], c.td["w3"]
    b_stream, b_keys, b_live = (torch.empty(D, device=dev()) for _ in range(3))
    got = PF._dgrad_sum(c.rec, st, "dst", w2, w3, c.n, g_b2=b_stream)
    live = torch.tensor([c.e], dtype=torch.int64, device=dev())
    got_live = PF._dgrad_sum(c.rec, st, "dst", w2, w3, c.n, g_b2=b_live, live=live)        # `live` given: keys route
    plan.stream = None
    got_keys = PF._dgrad_sum(c.rec, st, "dst", w2, w3, c.n, g_b2=b_keys)
    assert torch.equal(got, got_keys) and torch.equal(got, got_live)
    assert torch.equal(b_stream, b_keys) and torch.equal(b_stream, b_live)
    want_q = torch.zeros(c.n, D, dtype=torch.float64, device=dev()).index_add_(0, c.ei[1], c.ref["gh1"])
    assert torch.equal(got, _f32(want_q))


def test_dispatcher_route_uses_the_registered_stream():
    """torch.ops.pangnn.decoder_mlp's backward (csrc/graph_ops.cpp) finds the stream in the native structure registry: the
    by-target gradient and dL/db2 are the float64 values, as on the ctypes route above"""
    from pangnn_amd import torch_ops
    from pangnn_amd.graph import EdgeStructure
    c = case("E70000")
    st = EdgeStructure(c.ei, c.n)
    pq = torch.cat([c.td["P"], c.td["Q"]], 1).requires_grad_(True)
    b2 = c.td["b2"].clone().requires_grad_(True)
    out = torch_ops.decoder_mlp_pq(pq, st, None, None, c.td["W2"], b2, c.td["w3"], c.td["b3"])
    out.backward(c.g)
    assert st.csr_plan("dst", c.ct).stream is not None                          # what the backward registered and walked
    want_q = torch.zeros(c.n, D, dtype=torch.float64, device=dev()).index_add_(0, c.ei[1], c.ref["gh1"])
    assert torch.equal(out.detach(), _f32(c.ref["logits"]))
    assert torch.equal(pq.grad[:, D:], _f32(want_q)) and torch.equal(b2.grad, _f32(c.ref["a"].sum(0)))
