"""The width template of the strict-fp32 MLP link decoder (csrc/decoder.hip), the part that needs no GPU: which widths the
pangnn_decoder_nd_* entry points (node_dim 32 and 128) take, their argument checks (fake pointers, nothing launched), which
models pick the kernels, and the proof that every input set the bit-for-bit GPU cases of tests/test_decoder_widths.py use, the
node_dim 64 instance's included, is exact in float32 in any order of summation.

The input sets are defined here (`exact_inputs`) and imported by the GPU file."""
import functools
import zlib
from types import SimpleNamespace

import pytest
import torch

from pangnn_amd import _lib
from test_decoder_run_sums import _assert_exact_in_any_order, decoder_reference, g_grid, grid_edges, grid_tables

WIDTHS = (32, 128)                          # the widths of the pangnn_decoder_nd_* entry points and of the model gating
EXACT_WIDTHS = (32, 64, 128)                # the template's instances; 64 is what pangnn_decoder_mlp_* run at precision 0
N = 97
EXACT_E = (1, 31, 32, 33, 1000, 70001)     # around one tile; 70 001: a last tile of 17 edges, more tiles than 256 workgroups x
#                                            waves hold at every width, so waves walk several tiles and every workgroup has a slab
EXACT_SETS = [(d, skip, "list", e) for d in EXACT_WIDTHS for skip in (False, True) for e in EXACT_E] + \
             [(d, skip, kind, 1000) for d in EXACT_WIDTHS for skip in (False, True) for kind in ("one-source", "own-source")]


def set_id(s):
    return f"d{s[0]}-{'skip' if s[1] else 'plain'}-{s[2]}-E{s[3]}"


@functools.lru_cache(maxsize=4)
def exact_inputs(d, skip, kind, e):
    """tables, edges in a seeded random order (`src`, `dst`), dL/dlogit `g` and the skip feature `extra` on the exact grid of
    tests/test_decoder_run_sums.py at width d, and `by_src`: the stable permutation that sorts the list by source.
    kind "list": both ends random over 97 nodes; "one-source": every edge leaves node 5; "own-source": 1500 nodes, every edge
    has a source of its own."""
    seed = zlib.crc32(f"{d}-{skip}-{kind}-{e}".encode()) % 100003
    gen = torch.Generator().manual_seed(seed)
    n = 1500 if kind == "own-source" else N
    if kind == "list":
        src = torch.randint(0, n, (e,), generator=gen)
    elif kind == "one-source":
        src = torch.full((e,), 5, dtype=torch.int64)
    else:
        src = torch.randperm(n, generator=gen)[:e]
    dst = torch.randint(0, n, (e,), generator=gen)
    g, extra, q = grid_edges(e, seed, skip)
    assert q == g_grid(e, skip)[0]
    return SimpleNamespace(t=grid_tables(n, seed, d=d), src=src, dst=dst, g=g, extra=extra if skip else None, n=n, e=e, q=q,
                           d=d, by_src=torch.sort(src, stable=True).indices)


# ------------------------------------------------------------------------------------------------------------------
# supported widths and argument checks
# ------------------------------------------------------------------------------------------------------------------
def test_supported_widths():
    lib = _lib.load()
    assert [lib.pangnn_decoder_nd_supported(d) for d in WIDTHS] == [1, 1]
    assert [lib.pangnn_decoder_nd_supported(d) for d in (-1, 0, 16, 48, 64, 96, 256)] == [0] * 7


@pytest.mark.parametrize("d", WIDTHS)
def test_workspace_bytes_grow_with_the_list(d):
    lib = _lib.load()
    sizes = [lib.pangnn_decoder_nd_bwd_workspace_bytes(d, e) for e in (0, 1, 32, 33, 1000, 70001, 10 ** 6, 10 ** 8)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    assert sizes[0] >= 4 * (d * d + 3 * d + 2)                  # one slab at the least: the empty list is reduced too
    assert lib.pangnn_decoder_nd_bwd_workspace_bytes(64, 1000) == 0


F = 0x7f0000100000             # a fake device pointer, 16-byte aligned
E_BADARG, E_TOOLARGE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -4
BIG = 1 << 40                  # a workspace size no check can find too small


def _args(d, **kw):
    """the arguments the three entry points share, all valid: (p, ldp, q, ldq, num_nodes, edge_index, ld, num_edges, extra, cvec,
    w2, b2, w3, b3, D)"""
    a = dict(p=F, ldp=d, q=F, ldq=d, n=N, ei=F, ld=1000, e=1000, extra=None, cvec=None, w2=F, b2=F, w3=F, b3=F, D=d)
    a.update(kw)
    return tuple(a[k] for k in ("p", "ldp", "q", "ldq", "n", "ei", "ld", "e", "extra", "cvec", "w2", "b2", "w3", "b3", "D"))


def _calls(lib):
    """name -> f(head, **overrides of the entry point's own arguments) -> return code"""
    def fwd(head, logits=F):
        return lib.pangnn_decoder_nd_fwd_f32(*head, logits, None)

    def bwd(head, g_logits=F, g_h1=F, g_w2=F, g_b2=F, g_w3=F, g_b3=F, g_cvec=None, part_buf=None, part_off=None, ws=F,
            ws_bytes=BIG):
        return lib.pangnn_decoder_nd_bwd_f32(*head, g_logits, g_h1, g_w2, g_b2, g_w3, g_b3, g_cvec, part_buf, part_off, ws,
                                             ws_bytes, None)

    def loss(head, y=F, denom=1000, logits=F, loss_=F, g_h1=F, g_w2=F, g_b2=F, g_w3=F, g_b3=F, g_cvec=None, part_buf=None,
             part_off=None, ws=F, ws_bytes=BIG):
        return lib.pangnn_decoder_nd_loss_f32(*head, y, None, denom, logits, loss_, g_h1, g_w2, g_b2, g_w3, g_b3, g_cvec,
                                              part_buf, part_off, ws, ws_bytes, None)
    return dict(fwd=fwd, bwd=bwd, loss=loss)


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: only where a missing check cannot reach a GPU")
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("name", ["fwd", "bwd", "loss"])
def test_entry_points_refuse_bad_arguments(name, d):
    """every call fails a check, so nothing is launched; the codes and their order are those of pangnn_decoder_mlp_*"""
    lib = _lib.load()
    f = _calls(lib)[name]
    for other in (-1, 0, 16, 48, 64, 96, 256):
        assert f(_args(d, D=other, ldp=max(other, 4), ldq=max(other, 4))) == E_BADARG        # a width the kernels are not built for
    assert f"pangnn_decoder_nd_{name}_f32" in lib.pangnn_last_error().decode()
    assert f(_args(d, e=-1)) == E_BADARG and f(_args(d, ld=999)) == E_BADARG and f(_args(d, n=-1)) == E_BADARG
    for ld_bad in (d - 4, d + 2):                                                     # below D; not a multiple of 4
        assert f(_args(d, ldp=ld_bad)) == E_BADARG and f(_args(d, ldq=ld_bad)) == E_BADARG
    rows_4gib = (1 << 32) // (4 * d)
    assert f(_args(d, n=rows_4gib)) == E_TOOLARGE                                      # exactly 4 GiB
    assert f(_args(d, n=rows_4gib // 2, ldq=2 * d)) == E_TOOLARGE                      # the wider of the two strides counts
    assert f(_args(d, n=rows_4gib, ldp=d - 4)) == E_BADARG                             # the stride check comes first
    for k in ("p", "q", "ei", "w2", "b2", "w3", "b3"):
        assert f(_args(d, **{k: None})) == E_BADARG, k
    assert f(_args(d, extra=F, cvec=None)) == E_BADARG                                 # a skip feature without its vector
    for k in ("p", "q", "w2"):
        assert f(_args(d, **{k: F + 4})) == E_ALIGN, k
    assert f(_args(d, p=F + 4, b2=None)) == E_BADARG                                   # null pointers before alignment
    if name == "fwd":
        assert f(_args(d), logits=None) == E_BADARG
        assert f(_args(d, e=0, ld=0, p=None, q=None, ei=None), logits=None) == 0       # the empty list: nothing to do
        return
    if name == "bwd":
        assert f(_args(d), g_logits=None) == E_BADARG
    else:
        assert f(_args(d), denom=0) == E_BADARG and f(_args(d), loss_=None) == E_BADARG
        assert f(_args(d), y=None) == E_BADARG and f(_args(d), logits=None) == E_BADARG
    for k in ("g_w2", "g_b2", "g_w3", "g_b3"):
        assert f(_args(d), **{k: None}) == E_BADARG, k
    need = lib.pangnn_decoder_nd_bwd_workspace_bytes(d, 1000)
    assert f(_args(d), ws_bytes=need - 1) == E_WORKSPACE and f(_args(d), ws=None) == E_WORKSPACE
    assert f(_args(d), ws_bytes=0) == E_WORKSPACE and f(_args(d), ws_bytes=-1) == E_WORKSPACE
    assert b"workspace" in lib.pangnn_last_error().lower()
    assert f(_args(d), g_w2=None, ws_bytes=0) == E_BADARG                              # gradient outputs before the workspace
    assert f(_args(d), g_h1=None) == E_BADARG
    assert f(_args(d), g_h1=None, ws_bytes=0) == E_WORKSPACE                           # the workspace before g_h1
    assert f(_args(d), part_buf=F) == E_BADARG and f(_args(d), part_off=F) == E_BADARG   # together or not at all
    assert f(_args(d, e=0, ld=0), ws_bytes=0) == E_WORKSPACE                           # the empty list still reduces one slab


def test_d64_entry_points_keep_rejecting_other_widths():
    lib = _lib.load()
    for d in WIDTHS:
        assert lib.pangnn_decoder_mlp_fwd_f32(*_args(d), F, None) == E_BADARG
        assert "node_dim 64" in lib.pangnn_last_error().decode()


# ------------------------------------------------------------------------------------------------------------------
# which models take the kernels
# ------------------------------------------------------------------------------------------------------------------
def _model(dims, **kw):
    import pangnn_amd
    return pangnn_amd.AlternateGCN(torch.device("cpu"), None, False, dims=list(dims), num_nodes=10, **kw)


def test_model_gating():
    from pangnn_amd import functional as PF
    assert PF.DECODER_ND_WIDTHS == (32, 128)
    for dims in ((32, 64), (128, 128)):
        m = _model(dims)
        assert m._fused_width() and not m._decoder16() and m.training and not m._defers()
    m = _model((64, 128))
    assert m._fused_width() and m._decoder16() == (PF.DECODER_PRECISION == 1)
    assert m._defers() == (PF.DECODER_PRECISION == 1 and m.deferred_logits and not PF.observed())
    assert not _model((48, 64))._fused_width() and not _model((48, 64))._defers()


# ------------------------------------------------------------------------------------------------------------------
# the exact grid at widths 32, 64 and 128
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", EXACT_SETS, ids=set_id)
def test_grid_is_exact_in_float32_at_both_widths(s):
    """every quantity the bit-for-bit GPU cases compare: the sums of its positive and of its negative terms stay <= 2^24 units
    (1/q, or 1/(4 q) with skip connections), so no partial sum in any order or grouping can round — the sorted list is the same
    multiset of terms — and a float32 evaluation equals the float64 one"""
    inp = exact_inputs(*s)
    ref = decoder_reference(inp.t, inp.src, inp.dst, inp.g, inp.extra, magnitudes=True)
    _assert_exact_in_any_order(ref, 1.0 / (inp.q * (4 if inp.extra is not None else 1)))
    if inp.e <= 1000:
        r32 = decoder_reference(inp.t, inp.src, inp.dst, inp.g, inp.extra, dtype=torch.float32, order=inp.by_src, chunk=300)
        for k, v in r32.items():
            assert torch.equal(v.double(), ref[k]), k
    if s[2] == "list" and inp.e >= 1000:                       # relu masks of both kinds occur, and pre-activations exactly 0
        h1pre = inp.t["P"][inp.src[:4096]] + inp.t["Q"][inp.dst[:4096]]
        if inp.extra is not None:
            h1pre = h1pre + inp.extra[:4096, None] * inp.t["cvec"]
        h2pre = torch.relu(h1pre) @ inp.t["W2"].t() + inp.t["b2"]
        for pre in (h1pre, h2pre):
            assert 0.2 < float((pre > 0).float().mean()) < 0.8 and bool((pre == 0).any())
    if s[2] == "own-source":
        assert len(torch.unique(inp.src)) == inp.e
    # the fused-loss cases divide w3 by 64: the logits stay float32 values (the gradients are then held to a bound)
    t64 = dict(inp.t, w3=inp.t["w3"] / 64)
    lg = decoder_reference(t64, inp.src, inp.dst, torch.zeros(inp.e), inp.extra)["logits"]
    assert torch.equal(lg.float().double(), lg)
