"""The chunk walk of the STREAM instances of the training decoder's S and T kernels (csrc/decoder16.hip) against the ids / keys
instances of the same library on the same inputs — bit for bit.

The STREAM instances walk a wave's chunks in two loops: whole chunks of full tiles run a body without any tail or padding
logic (no live / store limits, no clamps, T without close_mask), the wave's final chunk (S) or final two chunks (T) run the
general body, which also handles the list's last tile and every prefetch that would point past the list.  The ids / keys
instances run one flat tile loop with the general body for every tile, their own per-tile bookkeeping and their own run-end
test — in T by calling the same body function as the walk, in S through a second textual copy of the half tile's statements —
and tests/test_decoder_run_sums.py pins them against a host reference, so they are the reference for the walk: logits and the
fused loss, the record table, the S and T part rows slot for slot (guard rows untouched), the per-workgroup slabs and every
parameter gradient reduced from them, and dL/db2 must be equal.

Lists: test_decoder_training_kernels_vs_fp64's generator on 97 nodes — every run is E / 97 edges long, so runs cross half
tiles, tiles and chunks.  A launch has one wave per chunk up to 2048 (S: 8 per workgroup) or 4096 (T: 16 per workgroup) waves
on a 256-CU chip, and the chunk size keeps a list at 2048 .. 4095 chunks until a chunk holds 16 tiles.  Lengths:
* one or two tiles with tails of 1, 31 and none;
* one tile per chunk at 2048 / 2048 / 2050 chunks with and without a tail, and 131 105 just behind the step to two tiles per
  chunk: S waves own 1 or 2 chunks (one wave walks one full chunk), T waves one chunk at the most;
* last chunks shorter than the chunk at 4 and 16 tiles per chunk (two tiles, the second a tail of one or two edges), and a
  last chunk of ONE tile, itself a tail, at 2 and at 16 tiles per chunk;
* 16 tiles per chunk and more than 2 x 4096 / 3 x 4096 chunks (4.2e6 and 6.3e6 edges), with and without a tail: only from
  there on does a T wave own a chunk it may walk with the full-tile body (its prefetch reaches two chunks ahead), and does a
  wave of either kernel walk a full chunk behind a full chunk (the part-offset hand-over and, in T, next32 across chunks).
  test_lengths_are_the_designed_ones replays the kernels' loop conditions and holds exactly that."""
import functools
from types import SimpleNamespace

import pytest
import torch

from conftest import random_graph
from test_decoder_run_sums import D, chunk_tiles_expected, part_layout
from test_dgrad_stream import run_T
from test_train_stream import DTYPES, assert_same, run_S

pytestmark = pytest.mark.gpu

N = 97
TAILS = [1, 31, 32, 33, 63, 64, 65]
ONE_TILE_CHUNKS = [32 * 2047 + 5, 32 * 2048, 32 * 2049 + 17, 32 * 4097 + 1]
SHORT_LAST_CHUNK = [262177, 1048609, 1048610]
SINGLE_TILE_LAST_CHUNK = [32 * 4096 + 1, 32 * 32768 + 5]
FULL_CHUNKS_IN_A_ROW = [32 * 16 * 8194 + 5, 32 * 16 * 8194, 32 * 16 * (3 * 4096 + 2) + 9]
LENGTHS = TAILS + ONE_TILE_CHUNKS + SHORT_LAST_CHUNK + SINGLE_TILE_LAST_CHUNK + FULL_CHUNKS_IN_A_ROW
CHUNK_TILES = {131105: 2, 262177: 4, 1048609: 16, 1048610: 16, 131073: 2, 1048581: 16,
               **{e: 16 for e in FULL_CHUNKS_IN_A_ROW}}                   # every other length: one tile per chunk

S_IDS, S_STREAM = "pangnn_decoder_train_mixed", "pangnn_decoder_train_stream_mixed"
T_KEYS, T_STREAM = "pangnn_decoder_dgrad_f32", "pangnn_decoder_dgrad_stream_f32"


def dev():
    return torch.device("cuda")


def walks(e, waves_per_group, reach):
    """the chunk walk's loop conditions (decoder16.hip) replayed: per wave of the launch the string of its chunks, F = walked
    by the full-tile loop (first + reach * cstep < nt - 1; reach 1 in S, 2 in T), G = by the general loop"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ct = chunk_tiles_expected(e)
    nt = (e + 31) // 32
    n_chunks = -(-nt // ct)
    grid = max(1, min(-(-n_chunks // waves_per_group), cus))
    cstep = grid * waves_per_group * ct
    out = []
    for wave in range(grid * waves_per_group):
        first, w, general = wave * ct, "", False
        while first < nt:
            general = general or not first + reach * cstep < nt - 1
            w += "G" if general else "F"
            first += cstep
        out.append(w)
    assert sum(len(w) for w in out) == n_chunks
    return out


def test_lengths_are_the_designed_ones():
    s_walks = {e: walks(e, 8, 1) for e in LENGTHS}
    t_walks = {e: walks(e, 16, 2) for e in LENGTHS}
    # below 4.2e6 edges: T's full-tile loop is never entered, S's for one chunk of a wave at the most
    for e in TAILS + ONE_TILE_CHUNKS + SHORT_LAST_CHUNK + SINGLE_TILE_LAST_CHUNK:
        assert not any("F" in w for w in t_walks[e]) and not any("FF" in w for w in s_walks[e])
    assert [e for e in LENGTHS if any("F" in w for w in s_walks[e])] == [65585, 131105, 262177, 1048609, 1048610] + FULL_CHUNKS_IN_A_ROW
    # from there on: full chunks in a row in S, a full chunk in T (two waves) and, at 6.3e6, two in a row; every wave ends in G
    for e in FULL_CHUNKS_IN_A_ROW:
        assert any("FF" in w for w in s_walks[e]) and sum("F" in w for w in t_walks[e]) >= 2
        assert all(w.endswith("G") and "GF" not in w for w in s_walks[e] + t_walks[e])
    assert any("FFG" in w for w in t_walks[FULL_CHUNKS_IN_A_ROW[2]]) and [e % 32 for e in FULL_CHUNKS_IN_A_ROW] == [5, 0, 9]
    assert {len(w) for w in s_walks[65585]} == {1, 2} and {len(w) for w in s_walks[65509]} == {1}
    assert ONE_TILE_CHUNKS == [65509, 65536, 65585, 131105]
    tiles = lambda e: (e + 31) // 32                                      # noqa: E731
    chunks = lambda e: -(-tiles(e) // chunk_tiles_expected(e))            # noqa: E731
    assert [tiles(e) for e in TAILS] == [1, 1, 1, 2, 2, 2, 3] and [e % 32 for e in TAILS] == [1, 31, 0, 1, 31, 0, 1]
    # waves of one launch: 2048 in S, so 2048 / 2048 / 2050 chunks give its waves 1 chunk each, 1 each, 1 or 2
    assert [chunks(e) for e in ONE_TILE_CHUNKS] == [2048, 2048, 2050, 2049]
    assert [chunk_tiles_expected(e) for e in ONE_TILE_CHUNKS] == [1, 1, 1, 2]
    assert [tiles(e) % chunk_tiles_expected(e) for e in SHORT_LAST_CHUNK] == [2, 2, 2]
    assert [tiles(e) % chunk_tiles_expected(e) for e in SINGLE_TILE_LAST_CHUNK] == [1, 1]
    assert [chunk_tiles_expected(e) for e in LENGTHS] == [CHUNK_TILES.get(e, 1) for e in LENGTHS]


@functools.lru_cache(None)
def case(e):
    """the source-sorted list on the device with the library's plans and streams, seeded tables and per-edge inputs, and the
    records of one S launch (ids route, f32 tables, no skip feature) for T"""
    from pangnn_amd import functional as PF
    from pangnn_amd.graph import EdgeStructure
    ct = CHUNK_TILES.get(e, 1)
    assert PF.d16_chunk(e) == ct == chunk_tiles_expected(e)
    ei, w = random_graph(N, e, seed=e, isolated=0.0)
    ei = ei[:, torch.argsort(ei[0] * N + ei[1])].contiguous()
    gen = torch.Generator(device="cuda").manual_seed(e)
    rnd = lambda *s: torch.randn(*s, generator=gen, device=dev())       # noqa: E731
    eid = ei.to(dev())
    rowptr = torch.searchsorted(eid[0].contiguous(), torch.arange(N + 1, device=dev()))
    lay = part_layout(ei[0].numpy(), ct, N)
    plan = EdgeStructure._plan_of_rowptr(rowptr, e, ct)
    assert plan.part_off.cpu().tolist() == lay.part_off.tolist()
    tabs = {k: (rnd(N, D).to(dt), rnd(N, D).to(dt)) for k, (dt, _) in DTYPES.items() if k != "f16"}
    wt = SimpleNamespace(W2=rnd(D, D) / 8, b2=rnd(D), w3=rnd(D), b3=rnd(1), cvec=rnd(D))
    c = SimpleNamespace(e=e, n=N, ct=ct, ei=eid, plan=plan, lay=lay, spos=EdgeStructure._spos_of_sorted_list(eid, ct), tabs=tabs,
                        w=wt, g=rnd(e) / e, y=(torch.rand(e, generator=gen, device=dev()) < 0.3).float(),
                        extra=(w / 40).to(dev()), pw=torch.tensor([2.5], device=dev()))
    # ---- the by-target side: the CSR order's plan with its stream, records of the ids route
    csr = EdgeStructure(eid, N).by_dst
    tplan = EdgeStructure._plan_of_rowptr(csr.rowptr, e, ct, perm=csr.perm)
    keys = eid[1][csr.perm.long()]
    tlay = part_layout(keys.cpu().numpy(), ct, N)
    assert tplan.stream is not None and tplan.part_off.cpu().tolist() == tlay.part_off.tolist()
    c.t = SimpleNamespace(e=e, n=N, ct=ct, rec=run_S(c, "ids", "f32", True, False).rec, plan=tplan, lay=tlay, perm=csr.perm,
                          td={"W2": wt.W2, "w3": wt.w3})
    return c


@pytest.fixture
def entry_calls(monkeypatch):
    """the names of the decoder entry points called, in order: a comparison of a route with itself is seen"""
    from pangnn_amd import _lib as L
    lib, calls = L.load(), []
    for name in (S_IDS, S_STREAM, T_KEYS, T_STREAM):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _fn=fn, _name=name: (calls.append(_name), _fn(*a))[1])
    return calls


@pytest.mark.parametrize("store", ["f32", "bf16"])
@pytest.mark.parametrize("skip", [False, True], ids=["plain", "skip"])
@pytest.mark.parametrize("e", LENGTHS)
def test_S_chunk_walk_equals_ids_route(e, skip, store, entry_calls):
    """fused loss: logits, loss, records, part rows (guard rows included), slabs, dL/dW2, dL/dw3, dL/db3, dL/dcvec"""
    c = case(e)
    del entry_calls[:]
    ids, stream = run_S(c, "ids", store, True, skip), run_S(c, "stream", store, True, skip)
    assert entry_calls == [S_IDS, S_STREAM]
    print(f"E={e} tiles={(e + 31) // 32} chunk tiles={c.ct} parts={c.lay.n_parts}")
    assert_same(stream, ids, c.lay.n_parts)
    assert bool(torch.isfinite(stream.loss).all())


@pytest.mark.parametrize("e", LENGTHS)
def test_S_chunk_walk_with_a_given_gradient(e, entry_calls):
    """the instances without the fused loss (dL/dlogit given): same outputs"""
    c = case(e)
    del entry_calls[:]
    ids, stream = run_S(c, "ids", "f32", False, True), run_S(c, "stream", "f32", False, True)
    assert entry_calls == [S_IDS, S_STREAM]
    assert_same(stream, ids, c.lay.n_parts)


@pytest.mark.parametrize("e", LENGTHS)
def test_T_chunk_walk_equals_keys_route(e, entry_calls):
    """part rows slot for slot (guard rows included) and dL/db2; the run sums alone take the same instance"""
    t = case(e).t
    del entry_calls[:]
    (pk, bk), (ps, bs) = run_T(t, "keys"), run_T(t, "stream")
    only_parts = run_T(t, "stream", want_b2=False)[0]
    assert entry_calls == [T_KEYS, T_STREAM, T_STREAM]
    print(f"E={e} tiles={(e + 31) // 32} chunk tiles={t.ct} parts={t.lay.n_parts}")
    assert torch.equal(ps, pk) and torch.equal(bs, bk) and torch.equal(only_parts, pk)
    from test_decoder_run_sums import SENTINEL
    assert bool((ps[t.lay.n_parts:] == SENTINEL).all()) and bool((ps[:t.lay.n_parts] != SENTINEL).all())
    assert bool(torch.isfinite(ps[:t.lay.n_parts]).all()) and bool(torch.isfinite(bs).all()) and bool((bs != 0).any())


def test_records_of_both_S_routes_feed_T_alike():
    """T on the records the stream route of S wrote: the same rows as on the ids route's (the records are equal, above)"""
    c = case(262177)
    rec = run_S(c, "stream", "f32", True, False).rec
    assert torch.equal(rec, c.t.rec)
    (pk, bk), (ps, bs) = run_T(c.t, "keys"), run_T(SimpleNamespace(**{**vars(c.t), "rec": rec}), "stream")
    assert torch.equal(ps, pk) and torch.equal(bs, bk)
