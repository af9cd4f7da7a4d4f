"""The S pass of the training decoder on its position stream (pangnn_decoder_train_stream_*, csrc/decoder16.hip) against its ids
route (pangnn_decoder_train_*) of the same library — bit for bit.

The stream is spos[k] = { src_k | closes_k << 31, dst_k } (pangnn_csr_plan_spos): the source-sorted list itself with "a part
row ends behind k", built once per graph.  Both routes run the same arithmetic on the same ids, so every output must be equal:
logits, loss, records, part rows slot for slot (and no guard row touched), the per-workgroup slabs and every gradient summed
from them.  The lists are those of tests/test_train_stream_host.py: every last-tile padding, run ends on and around every
half-tile, tile and chunk boundary, a run across three chunks, empty sources, half tiles of three and more runs, at 1, 2 and
16 tiles per chunk."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_decoder_run_sums import D, GUARD, SENTINEL, chunk_tiles_expected, part_layout
from test_train_stream_host import LISTS, sorted_list, spos_expected

pytestmark = pytest.mark.gpu

DTYPES = {"f32": (torch.float32, 0), "bf16": (torch.bfloat16, 1), "f16": (torch.float16, 2)}      # PANGNN_DTYPE_*


def dev():
    return torch.device("cuda")


@functools.lru_cache(None)
def case(name):
    """the list on the device with the library's plan and stream, seeded tables and per-edge inputs"""
    from pangnn_amd.graph import EdgeStructure
    src, dst, n = sorted_list(name)
    e = src.shape[0]
    ct = chunk_tiles_expected(e)
    gen = torch.Generator(device="cuda").manual_seed(e)
    rnd = lambda *s: torch.randn(*s, generator=gen, device=dev())       # noqa: E731
    ei = torch.from_numpy(np.stack([src, dst])).to(dev()).contiguous()
    rowptr = torch.searchsorted(ei[0].contiguous(), torch.arange(n + 1, device=dev()))
    plan = EdgeStructure._plan_of_rowptr(rowptr, e, ct)
    lay = part_layout(src, ct, n)
    assert plan.part_off.cpu().tolist() == lay.part_off.tolist()
    spos = EdgeStructure._spos_of_sorted_list(ei, ct)
    tabs = {k: (rnd(n, D).to(dt), rnd(n, D).to(dt)) for k, (dt, _) in DTYPES.items()}
    w = SimpleNamespace(W2=rnd(D, D) / 8, b2=rnd(D), w3=rnd(D), b3=rnd(1), cvec=rnd(D))
    return SimpleNamespace(name=name, e=e, n=n, ct=ct, ei=ei, plan=plan, lay=lay, spos=spos, tabs=tabs, w=w, g=rnd(e) / e,
                           y=(torch.rand(e, generator=gen, device=dev()) < 0.3).float(), extra=torch.rand(e, generator=gen, device=dev()),
                           pw=torch.tensor([2.5], device=dev()))


def run_S(c, route, store="f32", fused=False, skip=False):
    """one S launch through the C ABI; every output, the workspace (the slabs) included"""
    from pangnn_amd import _lib as L
    lib = L.load()
    p, q = c.tabs[store]
    full = lambda *s: torch.full(s, SENTINEL, dtype=torch.float32, device=dev())     # noqa: E731
    o = SimpleNamespace(logits=full(c.e), loss=full(1), rec=torch.zeros(c.e, 8, dtype=torch.int32, device=dev()),
                        parts=full(c.lay.n_parts + GUARD, D), gW2=full(D, D), gw3=full(D), gb3=full(1),
                        gcvec=full(D) if skip else None,
                        ws=torch.zeros(lib.pangnn_decoder_train_workspace_bytes(), dtype=torch.uint8, device=dev()))
    w = c.w
    head = (p.data_ptr(), p.stride(0), q.data_ptr(), q.stride(0), DTYPES[store][1], c.n)
    tail = (L.ptr(c.extra if skip else None), L.ptr(w.cvec if skip else None), w.W2.data_ptr(), w.b2.data_ptr(), w.w3.data_ptr(),
            w.b3.data_ptr(), D, L.ptr(c.y if fused else None), L.ptr(c.pw if fused else None), c.e if fused else 0,
            L.ptr(None if fused else c.g), o.logits.data_ptr(), L.ptr(o.loss if fused else None), o.rec.data_ptr(),
            o.parts.data_ptr(), c.plan.part_off.data_ptr(), o.gW2.data_ptr(), o.gw3.data_ptr(), o.gb3.data_ptr(), L.ptr(o.gcvec))
    if route == "stream":
        L.check(lib.pangnn_decoder_train_stream_mixed(*head, c.spos.data_ptr(), c.e, *tail, o.ws.data_ptr(), o.ws.numel(),
                                                      L.stream_ptr()), "pangnn_decoder_train_stream_mixed")
    else:
        L.check(lib.pangnn_decoder_train_mixed(*head, c.ei.data_ptr(), c.e, c.e, *tail, None, o.ws.data_ptr(), o.ws.numel(),
                                               L.stream_ptr()), "pangnn_decoder_train_mixed")
    return o


def assert_same(a, b, n_parts):
    for k in ("logits", "loss", "rec", "parts", "ws", "gW2", "gw3", "gb3", "gcvec"):
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None), k
        if x is not None:
            assert torch.equal(x, y) or torch.equal(x.view(torch.int32), y.view(torch.int32)), k
    assert bool((a.parts[n_parts:] == SENTINEL).all()) and bool((a.parts[:n_parts] != SENTINEL).all())
    assert bool(torch.isfinite(a.logits).all()) and bool(torch.isfinite(a.gW2).all())


@pytest.mark.parametrize("skip", [False, True], ids=["plain", "skip"])
@pytest.mark.parametrize("fused", [False, True], ids=["given-g", "fused-loss"])
@pytest.mark.parametrize("name", LISTS)
def test_stream_route_equals_ids_route(name, fused, skip):
    c = case(name)
    ids, stream = run_S(c, "ids", "f32", fused, skip), run_S(c, "stream", "f32", fused, skip)
    print(f"{name}: E={c.e} parts={c.lay.n_parts} chunk tiles={c.ct}")
    assert_same(stream, ids, c.lay.n_parts)
    if fused:
        assert bool(torch.isfinite(stream.loss).all())


@pytest.mark.parametrize("skip", [False, True], ids=["plain", "skip"])
@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("name", ["E17", "E33", "E65", "ct1", "ct2", "ct16"])
def test_stream_route_on_two_byte_tables(name, store, skip):
    c = case(name)
    for fused in (False, True):
        assert_same(run_S(c, "stream", store, fused, skip), run_S(c, "ids", store, fused, skip), c.lay.n_parts)


def test_stream_is_the_definition_for_every_case():
    for name in LISTS:
        c = case(name)
        src, dst, _ = sorted_list(name)
        assert torch.equal(c.spos.long() & 0xffffffff, torch.from_numpy(spos_expected(src, dst, 32 * c.ct)).to(dev()))


def test_structures_route_by_what_their_plan_carries():
    """a square structure's run-sum plan from the plan kernel carries the stream and _decoder_train16 walks it; a plan without
    one (the small build of a mini-batch, a padded batch with `live`, rows of a stride that is no power of two) takes the ids
    route — same outputs"""
    from pangnn_amd import functional as PF
    from pangnn_amd.graph import EdgeStructure
    c = case("ct2")
    st = EdgeStructure(c.ei, c.n)
    plan = st.runsum_plan(PF.d16_chunk(c.e))
    assert plan.stream is not None and torch.equal(plan.stream, c.spos)
    assert st.runsum_plan(1).stream is None                      # the strict-fp32 kernels' one-tile chunks
    small = case("ct1")
    assert EdgeStructure(small.ei, small.n).runsum_plan(PF.d16_chunk(small.e)).stream is None
    names = []
    orig = PF._launch

    def spy(dev_, name, *a, **k):
        names.append(name)
        return orig(dev_, name, *a, **k)
    p, q = c.tabs["f32"]
    w = c.w
    live = torch.tensor([c.e], dtype=torch.int64, device=dev())
    wide = torch.zeros(c.n, 96, device=dev())
    wide[:, :D] = p
    outs = []
    PF._launch = spy
    try:
        for kw, pp in ((dict(), p), (dict(live=live), p), (dict(), wide[:, :D])):
            outs.append(PF._decoder_train16(pp, q, st, None, None, w.W2, w.b2, w.w3, w.b3, y=c.y, pw=c.pw, denom=c.e, **kw))
        plan.stream = None
        outs.append(PF._decoder_train16(p, q, st, None, None, w.W2, w.b2, w.w3, w.b3, y=c.y, pw=c.pw, denom=c.e))
    finally:
        PF._launch = orig
    s_calls = [n for n in names if n.startswith("pangnn_decoder_train")]
    assert s_calls == ["pangnn_decoder_train_stream_mixed"] + ["pangnn_decoder_train_mixed"] * 3
    for o in outs[1:]:
        for x, y in zip(outs[0], o):
            assert (x is None and y is None) or torch.equal(x, y)


# ------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------
def _sorted_golden(name):
    """a golden graph with its similarity edges in source order (the order the decoder's run sums need), fresh tensors"""
    from conftest import whole_graph_from_golden
    g = whole_graph_from_golden(name, dev())
    order = torch.sort(g.edge_index[0], stable=True).indices
    g.edge_index = g.edge_index[:, order].contiguous()
    g.edge_attr, g.y = g.edge_attr[order].contiguous(), g.y[order].contiguous()
    del g.union_edge_index, g.union_edge_attr
    return g


@pytest.mark.parametrize("route", ["ops", "ctypes"])
def test_train_step_is_bit_identical_without_the_stream(route, monkeypatch):
    """train.train_step on the cfg2 golden graph: loss, logits and every parameter gradient with the stream equal those of a
    step whose plans carry none"""
    import pangnn_amd
    from pangnn_amd import functional as PF
    from pangnn_amd.graph import EdgeStructure
    from pangnn_amd.train import train_step
    pw = torch.tensor([3.0], device=dev())
    res = []
    for stream in (True, False):
        if not stream:
            monkeypatch.setattr(EdgeStructure, "_spos_of_sorted_list", staticmethod(lambda ei, ct: None))
        g = _sorted_golden("cfg2_sim_1000x5")
        torch.manual_seed(0)
        model = pangnn_amd.AlternateGCN(dev(), None, False, dims=[64, 128])
        opt = torch.optim.SGD(model.parameters(), lr=0.0)
        if route == "ctypes":
            monkeypatch.setattr(PF, "KERNEL_TIMER", {"dec.bwd": [], "dec.dgrad": [], "dec.fwd": []})
        loss, logits = train_step(model, opt, g, g.y, pw)
        sts = [st for _, st in g._pangnn_structs.values() if st.num_edges == g.edge_index.shape[1] and st._sorted and any(k[0] == "run" for k in st._plans)]
        assert sts, "the decoder's structure is held on the graph"
        plans = [p for st in sts for k, p in st._plans.items() if k[0] == "run"]
        assert plans and all((p.stream is not None) == stream for p in plans)
        res.append((loss.clone(), logits.clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}))
    a, b = res
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and bool(torch.isfinite(a[0]).all())
    assert a[2].keys() == b[2].keys() and len(a[2]) >= 8
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
