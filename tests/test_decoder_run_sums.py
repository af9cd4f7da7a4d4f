"""The training decoder's run sums, bit for bit, on inputs whose every intermediate is exactly representable in float32.

The S / T kernels of csrc/decoder16.hip (and the strict-fp32 pair of csrc/decoder.hip) compute nothing but products and sums
of their inputs and relu masks of those.  On the grid below every product, every partial sum in ANY order, every bf16
three-way split and every slab reduction is exact, the relu masks are the same in float32 and float64, and pre-activations
that are exactly 0 occur (they pin `[h > 0]` at zero).  A plain float64 torch evaluation must therefore be matched BIT FOR
BIT: there is no tolerance anywhere in this file, and one dropped, duplicated or misassigned edge fails a case.

  P, Q integers in [-4, 4], W2 in [-2, 2], b2 in [-8, 8], w3 in [-2, 2], b3 = 3, extra in multiples of 1/4 within [0, 2],
  cvec integers in [-2, 2]; dL/dlogit in multiples of 1/q within [-1, 1], q chosen per list length (`g_grid`).

Why a sum is exact in any order: every term of a sum is a multiple of one unit u (1/q, or 1/(4 q) with skip connections),
and a partial sum over any subset of the terms lies between minus the sum of the negative terms and the sum of the positive
ones.  If both of those are <= 2^24 u, every partial sum in every order is a multiple of u below 2^24 u: a float32.  The CPU
tests assert exactly that for every input set a GPU case uses (`_assert_exact_in_any_order`), and evaluate the reference in
float32 in two summation orders as a second witness.

Run boundaries are designed, not drawn: a 16-bit pattern describes one 16-position half tile (bit e set = position e is the
last of its run); all 65 536 patterns in a seeded shuffled order make the master sequence of 2^20 positions, whose prefixes
select every chunk size of the kernels (the chunk size is a function of the list length alone).  In a shuffle of ALL patterns
nearly every half tile has two or more inner boundaries (only 32 of the 65 536 patterns have none or one), so a second
sequence of the same length, the "mixed" one, gives every fourth half tile to those 32: each of its prefixes meets every
branch of run_sums(), every boundary position 0 .. 14, closing and open at position 15, after a half tile that left its run
open and after one that closed it (test_mixed_sequence_meets_every_branch_in_both_carry_states)."""
import functools
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

D = 64
GUARD = 4                      # guard rows behind the exact number of parts
SENTINEL = -7.5e33             # what unwritten rows / entries hold
gpu = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------------
# reference: the decoder of include/pangnn_hip.h in plain torch
# ------------------------------------------------------------------------------------------------------------------
SUMS = ("gP", "gQ", "gW2", "gb2", "gw3", "gb3", "gcvec")


def decoder_reference(t, src, dst, g, extra=None, live=None, dtype=torch.float64, order=None, chunk=1 << 16, rows=False,
                      magnitudes=False):
    """h1pre = P[src] + Q[dst] (+ extra cvec); h2pre = relu(h1pre) W2^T + b2; logit = relu(h2pre) . w3 + b3 and, for the given
    dL/dlogit g (edges >= live count as g = 0):  dL/dh2pre = [h2pre > 0] w3 g,  dL/dh1pre = [h1pre > 0] (dL/dh2pre W2),
    dL/dW2 = dL/dh2pre^T h1, dL/db2, dL/dw3 = sum g h2, dL/db3 = sum g, dL/dcvec = sum extra dL/dh1pre, dL/dP / dL/dQ = the
    rows of dL/dh1pre summed by source / target.  Edges are taken `chunk` at a time in `order` (default: list order).
    rows: also the per-edge dL/dh1pre ("gh1") and dL/dh2pre for g taken as given, without `live` ("a").
    magnitudes: also, under "mag", the sum of the ABSOLUTE values of the terms of every summed quantity."""
    P, Q, W2, b2, w3, b3 = (t[k].to(dtype) for k in ("P", "Q", "W2", "b2", "w3", "b3"))
    cv = t["cvec"].to(dtype) if extra is not None else None
    e, d, device = src.numel(), P.shape[1], src.device
    z = lambda *s: torch.zeros(*s, dtype=dtype, device=device)            # noqa: E731
    gl = g.to(dtype).clone()
    if live is not None:
        gl[min(max(int(live), 0), e):] = 0
    out = dict(logits=z(e), gP=z(P.shape[0], d), gQ=z(Q.shape[0], d), gW2=z(d, d), gb2=z(d), gw3=z(d), gb3=z(1), gcvec=z(d))
    if rows:
        out["gh1"], out["a"] = z(e, d), z(e, d)
    mag = {k: torch.zeros_like(out[k]) for k in SUMS} if magnitudes else None
    for c0 in range(0, e, chunk):
        ids = torch.arange(c0, min(c0 + chunk, e), device=device) if order is None else order[c0:c0 + chunk]
        s, tg, ge = src[ids], dst[ids], gl[ids]
        h1pre = P[s] + Q[tg]
        if extra is not None:
            x = extra[ids].to(dtype)
            h1pre = h1pre + x[:, None] * cv
        h1 = torch.relu(h1pre)
        h2pre = h1 @ W2.t() + b2
        h2 = torch.relu(h2pre)
        out["logits"][ids] = h2 @ w3 + b3
        m2w = (h2pre > 0).to(dtype) * w3
        a = m2w * ge[:, None]
        m1 = (h1pre > 0).to(dtype)
        gh1 = m1 * (a @ W2)
        if rows:
            out["a"][ids] = m2w * g[ids].to(dtype)[:, None]
            out["gh1"][ids] = m1 * ((m2w * g[ids].to(dtype)[:, None]) @ W2)
        terms = [(out, a, ge, gh1)]
        if magnitudes:                                    # |a| (x) h1 with h1 >= 0; |g| h2 with h2 >= 0; |rows|
            terms.append((mag, a.abs(), ge.abs(), gh1.abs()))
        for acc, a_, g_, r_ in terms:
            acc["gW2"] += a_.t() @ h1
            acc["gb2"] += a_.sum(0)
            acc["gw3"] += (g_[:, None] * h2).sum(0)
            acc["gb3"] += g_.sum()
            if extra is not None:
                acc["gcvec"] += (x[:, None] * r_).sum(0)
            acc["gP"].index_add_(0, s, r_)
            acc["gQ"].index_add_(0, tg, r_)
    if magnitudes:
        out["mag"] = mag
    return out


# ------------------------------------------------------------------------------------------------------------------
# inputs on the exact grid
# ------------------------------------------------------------------------------------------------------------------
def g_grid(e, skip=False):
    """(q, density): dL/dlogit is a multiple of 1/q in [-1, 1], non-zero on `density` of the edges.  The rule is the condition
    of `_assert_exact_in_any_order`, asserted per input set by the CPU tests; the numbers are the finest grid that meets it.
    The binding sum is dL/dw3 = sum g h2 (h2 is ~28 on average, in quarters with skip connections): on this grid its positive
    terms reach 0.6 * 2^24 units at (65 536 edges, q = 16) without and at (65 536, q = 4) with skip connections."""
    table = ([(4224, 64, 1.0), ((1 << 16) + 32, 16, 1.0), ((1 << 17) + 32, 8, 1.0), ((1 << 18) + 32, 4, 1.0)] if not skip else
             [(4224, 16, 1.0), ((1 << 16) + 32, 4, 1.0), ((1 << 17) + 32, 2, 1.0)])
    for limit, q, density in table:
        if e <= limit:
            return q, density
    return (1, 1.0) if not skip else (1, 0.125)


def grid_tables(n, seed, d=D):
    gen = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).float()      # noqa: E731
    return dict(P=ri(-4, 4, n, d), Q=ri(-4, 4, n, d), W2=ri(-2, 2, d, d), b2=ri(-8, 8, d), w3=ri(-2, 2, d),
                b3=torch.tensor([3.0]), cvec=ri(-2, 2, d))


def grid_edges(e, seed, skip=False):
    """(g, extra, q): dL/dlogit on the grid of g_grid(e, skip); the skip feature in multiples of 1/4 within [0, 2]"""
    gen = torch.Generator().manual_seed(seed + 977)
    q, density = g_grid(e, skip)
    g = torch.randint(-q, q + 1, (e,), generator=gen).float() / q
    extra = torch.randint(0, 9, (e,), generator=gen).float() / 4
    if density < 1:
        g = g * (torch.rand(e, generator=gen) < density).float()
    return g, extra, q


def _assert_exact_in_any_order(ref, unit):
    """every summed quantity of `ref` (decoder_reference(..., magnitudes=True)) has its positive terms and its negative terms
    each summing to <= 2^24 unit: then every partial sum, in every order and grouping, is a float32"""
    for k in SUMS:
        val, mag = ref[k], ref["mag"][k]
        worst = float(((mag + val.abs()) / 2).max())          # max(sum of positive terms, |sum of negative terms|)
        assert worst <= 2.0 ** 24 * unit, (k, worst / unit, 2.0 ** 24)
        assert torch.equal(val.float().double(), val), k
    assert torch.equal(ref["logits"].float().double(), ref["logits"])


# ------------------------------------------------------------------------------------------------------------------
# designed key sequences
# ------------------------------------------------------------------------------------------------------------------
def keys_from_patterns(patterns):
    """pattern m describes one 16-position half tile: bit e set = position e is the last of its run; the keys follow by
    incrementing after every set bit"""
    p = np.asarray(patterns, dtype=np.int64)
    last = ((p[:, None] >> np.arange(16)) & 1).reshape(-1)
    return np.concatenate([[0], np.cumsum(last)[:-1]]).astype(np.int64)


@functools.lru_cache(None)
def master_patterns():
    """all 65 536 patterns in a seeded shuffled order: 2^20 positions in which both carry-in states (bit 15 of the previous
    pattern clear or set) meet every kind of pattern"""
    p = torch.randperm(1 << 16, generator=torch.Generator().manual_seed(65536)).numpy().astype(np.int64)
    assert np.array_equal(np.sort(p), np.arange(1 << 16))
    return p


@functools.lru_cache(None)
def mixed_patterns():
    """65 536 half tiles: three of every four slots walk the shuffled patterns with two or more inner boundaries, the fourth
    walks the 32 patterns with none or exactly one (bit 15 clear and set), reshuffled on every round"""
    gen = torch.Generator().manual_seed(32)
    inner = np.arange(1 << 16) & 0x7fff
    rare = np.flatnonzero((inner & (inner - 1)) == 0)
    assert len(rare) == 32
    many = np.setdiff1d(np.arange(1 << 16), rare)
    many = many[torch.randperm(len(many), generator=gen).numpy()]
    out = np.empty(1 << 16, dtype=np.int64)
    slots = np.arange(1 << 16) % 4 == 3
    out[~slots] = many[: int((~slots).sum())]
    rounds = [rare[torch.randperm(32, generator=gen).numpy()] for _ in range((int(slots.sum()) + 31) // 32)]
    out[slots] = np.concatenate(rounds)[: int(slots.sum())]
    return out


def mixed_keys(e):
    """the first e positions of the mixed sequence (continued with its own start beyond 2^20)"""
    return keys_from_patterns(np.resize(mixed_patterns(), (e + 15) // 16))[:e].copy()


def master_keys(e):
    """the first e positions of the master sequence (continued with its own start beyond 2^20)"""
    return keys_from_patterns(np.resize(master_patterns(), (e + 15) // 16))[:e].copy()


def keys_from_starts(start):
    start = np.asarray(start, dtype=bool).copy()
    start[0] = True
    return (np.cumsum(start) - 1).astype(np.int64)


def chunk_tiles_expected(e):
    """tiles per run-sum chunk as the header documents it: 16 for lists of >= 2048 * 16 tiles, halved until the list has at
    least 2048 chunks"""
    tiles, ct = (e + 31) // 32, 16
    while ct > 1 and tiles // ct < 2048:
        ct //= 2
    return ct


E_OF_CT = {1: 6007, 2: 1 << 17, 16: 1 << 20}          # list lengths that select 1, 2 and 16 tiles per chunk
TAIL_BASE = 32 * 131                                  # tails: E = 32 k + r, nine T workgroups
LIVE_E = TAIL_BASE + 17
PERM_E = 32 * 127 + 15                                # <= the number of records: perm may be NULL


def _change_on_chunk_starts(e, ct):
    """the master sequence's boundaries, with a key change forced on every odd chunk start and removed from every even one"""
    k = mixed_keys(e)
    start = np.concatenate([[True], k[1:] != k[:-1]])
    span = 32 * ct
    start[span::2 * span] = True
    start[2 * span::2 * span] = False
    return keys_from_starts(start)


def _tail(e, last_run_of_one):
    k = mixed_keys(e)
    if last_run_of_one:
        k[-1] = k[-2] + 1
    else:
        k[e - 40:] = k[e - 41]                        # the last run starts in the tile before the last one
    return k


def _key_cases():
    c = {}
    for lg in range(16, 21):
        c[f"master-2^{lg}"] = functools.partial(master_keys, 1 << lg)
        c[f"mixed-2^{lg}"] = functools.partial(mixed_keys, 1 << lg)
    for ct, e in E_OF_CT.items():
        for run in sorted({16, 32, 32 * ct - 1, 32 * ct, 32 * ct + 1}):
            c[f"runs-of-{run}-ct{ct}"] = functools.partial(lambda e, run: np.arange(e, dtype=np.int64) // run, e, run)
    c["one-key"] = lambda: np.zeros(2049, dtype=np.int64)
    c["own-key-ct1"] = lambda: np.arange(4129, dtype=np.int64)
    c["own-key-ct2"] = lambda: np.arange((1 << 17) + 1, dtype=np.int64)
    c["change-on-chunk-start-ct1"] = functools.partial(_change_on_chunk_starts, 4129, 1)
    c["change-on-chunk-start-ct2"] = functools.partial(_change_on_chunk_starts, (1 << 17) + 1, 2)
    c["gaps-empty-rows"] = lambda: mixed_keys(5000) * 3 + 5
    for r in (1, 15, 16, 17, 31):
        c[f"tail-r{r}-last-run-of-1"] = functools.partial(_tail, TAIL_BASE + r, True)
        c[f"tail-r{r}-run-from-previous-tile"] = functools.partial(_tail, TAIL_BASE + r, False)
    for r in (1, 17):
        c[f"tail-ct2-r{r}-run-from-previous-tile"] = functools.partial(_tail, (1 << 17) + r, False)
    c["live-list"] = functools.partial(mixed_keys, LIVE_E)
    c["perm-list"] = functools.partial(mixed_keys, PERM_E)
    return c


KEY_CASES = _key_cases()
T_CASES = [k for k in KEY_CASES if k not in ("live-list", "perm-list")]


@functools.lru_cache(None)
def case_keys(name):
    """(keys int64 numpy, number of rows): 4 more rows than keys for the case with gaps, so that the last rows are empty too"""
    k = KEY_CASES[name]()
    assert (np.diff(k) >= 0).all() and k[0] >= 0
    return k, int(k[-1]) + 1 + (4 if name.startswith("gaps") else 0)


def case_perm(name, e, n_rec):
    """positions -> record ids, seeded by the case's name: a list longer than the record table repeats edge ids"""
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    return torch.randint(0, n_rec, (e,), generator=gen).to(torch.int32)


# ------------------------------------------------------------------------------------------------------------------
# part layout: the test's own definition (never EdgeStructure._plan_of_sorted_keys)
# ------------------------------------------------------------------------------------------------------------------
def part_layout(keys, chunk_tiles, n_rows):
    """A new part starts at every position k with k % (32 chunk_tiles) == 0 and at every k with keys[k] != keys[k - 1].
    part_id[k]: the part of position k; part_off[c]: the part of chunk c's first position; part_rowptr[r]: the first part
    of row r, an empty row repeating the next row's value, part_rowptr[n_rows] = the number of parts."""
    keys = np.asarray(keys, dtype=np.int64)
    e, span = keys.shape[0], 32 * int(chunk_tiles)
    start = np.zeros(e, dtype=bool)
    start[::span] = True
    start[1:] |= keys[1:] != keys[:-1]
    part_id = np.cumsum(start) - 1
    n_parts = int(start.sum())
    rowptr = np.full(n_rows + 1, n_parts, dtype=np.int64)
    first = np.concatenate([[True], keys[1:] != keys[:-1]])               # first position of every row that has any
    rowptr[keys[first]] = part_id[first]
    rowptr = np.minimum.accumulate(rowptr[::-1])[::-1].copy()             # empty rows: the next row's value
    return SimpleNamespace(part_id=part_id, n_parts=n_parts, part_off=part_id[::span].astype(np.int32),
                           part_rowptr=rowptr, chunk_tiles=int(chunk_tiles))


# ------------------------------------------------------------------------------------------------------------------
# the input sets of the GPU cases
# ------------------------------------------------------------------------------------------------------------------
REC_N, REC_E = 257, 4096


@functools.lru_cache(None)
def rec_inputs():
    """the list whose records feed every T case: 4096 edges over 257 nodes in random order, no skip connections"""
    gen = torch.Generator().manual_seed(11)
    src, dst = torch.randint(0, REC_N, (REC_E,), generator=gen), torch.randint(0, REC_N, (REC_E,), generator=gen)
    g, _, q = grid_edges(REC_E, 11)
    return SimpleNamespace(t=grid_tables(REC_N, 11), src=src, dst=dst, g=g, extra=None, n=REC_N, e=REC_E, q=q)


S_SIZES = {"2^16": 1 << 16, "2^17+1": (1 << 17) + 1, "2^18+17": (1 << 18) + 17, "2^19+1": (1 << 19) + 1, "2^20": 1 << 20,
           "2^20+17": (1 << 20) + 17}
S_CHUNK_TILES = {"2^16": 1, "2^17+1": 2, "2^18+17": 4, "2^19+1": 8, "2^20": 16, "2^20+17": 16}
S_SETS = [(k, False) for k in S_SIZES] + [("2^16", True), ("2^17+1", True), ("2^19+1", True)]
SMALL_E = {f"tail-r{r}": TAIL_BASE + r for r in (1, 15, 16, 17, 31)}        # the strict-fp32 kernels' tails
STRICT_SETS = [("2^16", False), ("2^16", True)] + [(k, k == "tail-r17") for k in SMALL_E]
ALL_SIZES = dict(S_SIZES, **SMALL_E)


def set_id(s):
    return s[0] + ("-skip" if s[1] else "")


@functools.lru_cache(4)
def s_inputs(size, skip):
    """a source-sorted list whose sources are the designed keys (prefix of the mixed sequence) and whose targets are seeded
    random over at most 4099 nodes (the other rows of dL/dQ stay empty)"""
    e = ALL_SIZES[size]
    keys = mixed_keys(e)
    n = int(keys[-1]) + 1
    seed = zlib.crc32(size.encode()) % 100003
    gen = torch.Generator().manual_seed(seed)
    dst = torch.randint(0, min(n, 4099), (e,), generator=gen)
    g, extra, q = grid_edges(e, seed, skip)
    return SimpleNamespace(t=grid_tables(n, seed), src=torch.from_numpy(keys), dst=dst, g=g, extra=extra if skip else None,
                           n=n, e=e, q=q, keys=keys)


def unit_of(inp):
    return 1.0 / (inp.q * (4 if inp.extra is not None else 1))


# ------------------------------------------------------------------------------------------------------------------
# CPU tests
# ------------------------------------------------------------------------------------------------------------------
def _check_exactness(inp):
    ref = decoder_reference(inp.t, inp.src, inp.dst, inp.g, inp.extra, magnitudes=True, rows=inp.e <= REC_E)
    _assert_exact_in_any_order(ref, unit_of(inp))
    # relu masks of both kinds, and pre-activations that are exactly 0, occur
    s, tg = inp.src[:4096], inp.dst[:4096]
    h1pre = inp.t["P"][s] + inp.t["Q"][tg] + (0 if inp.extra is None else inp.extra[:4096, None] * inp.t["cvec"])
    h2pre = torch.relu(h1pre) @ inp.t["W2"].t() + inp.t["b2"]
    for pre in (h1pre, h2pre):
        assert 0.2 < float((pre > 0).float().mean()) < 0.8 and bool((pre == 0).any())
    # the same reference in float32, in list order and in a random order with another chunking: both ARE the float64 values
    order = torch.randperm(inp.e, generator=torch.Generator().manual_seed(5))
    for kw in (dict(), dict(order=order, chunk=40000)):
        r32 = decoder_reference(inp.t, inp.src, inp.dst, inp.g, inp.extra, dtype=torch.float32, rows=inp.e <= REC_E, **kw)
        for k in r32:
            assert r32[k].dtype == torch.float32 and torch.equal(r32[k].double(), ref[k]), (k, kw.keys())
    return ref


@pytest.mark.parametrize("s", S_SETS + [s for s in STRICT_SETS if s not in S_SETS], ids=set_id)
def test_grid_is_exact_in_float32_for_the_sorted_lists(s):
    """every quantity the S and strict-fp32 cases compare: its terms cannot round in any order (sum of the positive / negative
    terms <= 2^24 units), and a float32 evaluation in two summation orders equals the float64 one bit for bit.  A `live` case
    zeroes dL/dlogit on a tail of the list, i.e. drops terms: the bound holds a fortiori."""
    inp = s_inputs(*s)
    assert inp.q == g_grid(inp.e, s[1])[0] and len(inp.keys) == inp.e and bool((inp.g * inp.q == (inp.g * inp.q).round()).all())
    _check_exactness(inp)


def test_grid_is_exact_in_float32_for_the_record_list():
    inp = rec_inputs()
    ref = _check_exactness(inp)
    assert float(ref["gh1"].abs().max()) <= MAX_ROW


MAX_ROW = 64.0         # bound on |dL/dh1pre| of the record list (asserted above; the worst case of the grid is 64 * 4 = 256)


@pytest.mark.parametrize("name", list(KEY_CASES))
def test_T_case_sums_are_exact_in_float32(name):
    """parts, per-row sums and dL/db2 of a T case: a row of the case is at most `longest run` positions, each holding a record
    row of at most MAX_ROW in multiples of 1/64, so the sums of its positive and of its negative terms stay below 2^24 / 64;
    and the float32 sums in forward and in reverse position order equal the float64 ones"""
    keys, n_rows = case_keys(name)
    e = len(keys)
    change = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1], [True]]))
    longest = int(np.diff(change).max())
    assert longest * MAX_ROW * 64 <= 2 ** 24, longest
    assert not _wants_b2(e) or e * 64 <= 2 ** 24           # dL/db2: e terms of at most 1 in multiples of 1/64 (times w3)
    inp = rec_inputs()
    ref = decoder_reference(inp.t, inp.src, inp.dst, inp.g, rows=True)
    perm = case_perm(name, e, REC_E).long()
    lay = part_layout(keys, chunk_tiles_expected(e), n_rows)
    pid, kt = torch.from_numpy(lay.part_id), torch.from_numpy(keys)
    cols = slice(None) if e <= (1 << 17) + 32 else slice(None, None, 16)   # the long lists: every 16th column (the bound above
    rows64 = ref["gh1"][:, cols][perm]                                     # covers all of them)
    w = rows64.shape[1]
    want_p = torch.zeros(lay.n_parts, w, dtype=torch.float64).index_add_(0, pid, rows64)
    want_r = torch.zeros(n_rows, w, dtype=torch.float64).index_add_(0, kt, rows64)
    rows32 = rows64.float()
    for idx in (torch.arange(e), torch.arange(e - 1, -1, -1)):
        got_p = torch.zeros(lay.n_parts, w).index_add_(0, pid[idx], rows32[idx])
        got_r = torch.zeros(n_rows, w).index_add_(0, kt[idx], rows32[idx])
        assert torch.equal(got_p.double(), want_p) and torch.equal(got_r.double(), want_r)
        if _wants_b2(e):
            a32 = ref["a"][perm].float()[idx]
            assert torch.equal(a32.sum(0).double(), ref["a"][perm].sum(0))


def _wants_b2(e):
    return e <= 1 << 18


@pytest.mark.parametrize("e,ct", [(1, 1), (4096, 1), (65536, 1), (131040, 1), (131041, 2), (1 << 17, 2), ((1 << 17) + 1, 2),
                                  (1 << 18, 4), ((1 << 18) + 17, 4), (1 << 19, 8), ((1 << 19) + 1, 8), ((1 << 20) - 32, 8),
                                  ((1 << 20) - 31, 16), (1 << 20, 16), ((1 << 20) + 17, 16), (6007, 1)])
def test_chunk_tiles_is_a_function_of_the_list_length(e, ct):
    from pangnn_amd import functional as PF
    assert PF._lib.load().pangnn_decoder_chunk_tiles_for(e) == ct == chunk_tiles_expected(e)


def test_every_designed_list_selects_its_chunk_size():
    for lg, ct in zip(range(16, 21), (1, 2, 4, 8, 16)):
        assert chunk_tiles_expected(1 << lg) == ct and len(case_keys(f"master-2^{lg}")[0]) == len(case_keys(f"mixed-2^{lg}")[0]) == 1 << lg
    for ct, e in E_OF_CT.items():
        assert chunk_tiles_expected(e) == ct
    for k, e in S_SIZES.items():
        assert chunk_tiles_expected(e) == S_CHUNK_TILES[k]
    for name in KEY_CASES:
        if "-ct" in name:
            assert chunk_tiles_expected(len(case_keys(name)[0])) == int(name.split("-ct")[1].split("-")[0]), name
        elif not name.startswith(("master", "mixed")):
            assert chunk_tiles_expected(len(case_keys(name)[0])) == 1, name


def test_mixed_sequence_meets_every_branch_in_both_carry_states():
    """per prefix: every half-tile pattern kind — no inner boundary, one inner boundary at each of 0 .. 14, two or more — with
    bit 15 clear and set, after a half tile that left a run open and after one that closed it"""
    assert len(np.unique(master_patterns())) == 1 << 16
    for lg in range(16, 21):
        p = mixed_patterns()[: (1 << lg) // 16]
        inner = p & 0x7fff
        pop = np.array([bin(int(x)).count("1") for x in np.unique(inner)])
        popc = dict(zip(np.unique(inner).tolist(), pop.tolist()))
        kind = np.array([-1 if x == 0 else (int(x).bit_length() - 1 if popc[int(x)] == 1 else 15) for x in inner])
        open_in = np.concatenate([[0], (p[:-1] >> 15) ^ 1])                 # 1: the previous half tile left its run open
        seen = set(zip(kind.tolist(), (p >> 15).tolist(), open_in.tolist()))
        assert len(seen) == 17 * 2 * 2, (lg, len(seen))


@pytest.mark.parametrize("name", list(KEY_CASES))
def test_own_part_layout_is_the_plan_of_sorted_keys(name):
    """entry for entry the part_off, part_rowptr, keys and n_parts_exact() of EdgeStructure._plan_of_sorted_keys, at every chunk
    size, for every designed key sequence"""
    from pangnn_amd.graph import EdgeStructure
    keys, n_rows = case_keys(name)
    kt = torch.from_numpy(keys)
    for ct in (1, 2, 4, 8, 16):
        lay = part_layout(keys, ct, n_rows)
        plan = EdgeStructure._plan_of_sorted_keys(kt, n_rows, ct)
        assert plan.part_off.dtype == torch.int32 and plan.keys.dtype == torch.int32
        assert np.array_equal(plan.part_off.numpy(), lay.part_off)
        assert np.array_equal(plan.part_rowptr.numpy(), lay.part_rowptr)
        assert np.array_equal(plan.keys.numpy(), keys.astype(np.int32))
        assert plan.n_parts_exact() == lay.n_parts <= plan.n_parts
        assert lay.part_rowptr[-1] == lay.n_parts and len(lay.part_off) == (len(keys) + 32 * ct - 1) // (32 * ct)


def test_part_layout_small_cases_by_hand():
    # a key change ON a chunk start opens one part, not two
    lay = part_layout([0] * 32 + [1] * 32, 1, 2)
    assert lay.n_parts == 2 and lay.part_off.tolist() == [0, 1] and lay.part_rowptr.tolist() == [0, 1, 2]
    # the same keys in one two-tile chunk: still two parts
    lay = part_layout([0] * 32 + [1] * 32, 2, 2)
    assert lay.n_parts == 2 and lay.part_off.tolist() == [0] and lay.part_rowptr.tolist() == [0, 1, 2]
    # one key over two chunks is two parts of the same row; rows 0, 2, 3 and 5 are empty
    lay = part_layout([1] * 40 + [4] * 2, 1, 6)
    assert lay.n_parts == 3 and lay.part_off.tolist() == [0, 1] and lay.part_id.tolist() == [0] * 32 + [1] * 8 + [2] * 2
    assert lay.part_rowptr.tolist() == [0, 0, 2, 2, 2, 3, 3]
    from pangnn_amd.graph import EdgeStructure
    plan = EdgeStructure._plan_of_sorted_keys(torch.tensor([1] * 40 + [4] * 2), 6, 1)
    assert plan.part_rowptr.tolist() == lay.part_rowptr.tolist() and plan.n_parts_exact() == 3
    assert keys_from_patterns([0x8001, 0x0000, 0x0004]).tolist() == [0] + [1] * 15 + [2] * 16 + [2] * 3 + [3] * 13


def test_reference_on_a_hand_worked_example():
    """two sources, two targets, four edges, width 2.  h1pre of edge 0 is [1, 0] (a pre-activation exactly 0: masked) and its
    h2pre is [1, 0] (the same in the second layer); edge 1 has both layers dead, edge 2 both alive, edge 3 an h1 alive behind
    a dead h2."""
    t = dict(P=torch.tensor([[1., -1.], [2., 0.]]), Q=torch.tensor([[0., 1.], [-3., 1.]]), W2=torch.tensor([[1., -1.], [2., 1.]]),
             b2=torch.tensor([0., -2.]), w3=torch.tensor([2., -1.]), b3=torch.tensor([3.]), cvec=torch.zeros(2))
    src, dst = torch.tensor([0, 0, 1, 1]), torch.tensor([0, 1, 0, 1])
    g = torch.tensor([1., -0.5, 0.25, 2.])
    r = decoder_reference(t, src, dst, g, rows=True)
    # h1 = [1 0] [0 0] [2 1] [0 1];  h2pre = [1 0] [0 -2] [1 3] [-1 -1]
    assert r["logits"].tolist() == [5., 3., 2., 3.]
    # dL/dh2pre = [2 0] [0 0] [.5 -.25] [0 0];  times W2 = [2 -2] . [0 -.75] .;  masked by [h1pre > 0] = [1 0] . [1 1] .
    assert r["a"].tolist() == [[2., 0.], [0., 0.], [0.5, -0.25], [0., 0.]]
    assert r["gh1"].tolist() == [[2., 0.], [0., 0.], [0., -0.75], [0., 0.]]
    assert r["gP"].tolist() == [[2., 0.], [0., -0.75]] and r["gQ"].tolist() == [[2., -0.75], [0., 0.]]
    assert r["gW2"].tolist() == [[3., 0.5], [-0.5, -0.25]]
    assert r["gb2"].tolist() == [2.5, -0.25] and r["gw3"].tolist() == [1.25, 0.75] and r["gb3"].tolist() == [2.75]
    # the first three edges live: edge 3 contributes nothing anyway; the first two: edge 2 drops out
    r2 = decoder_reference(t, src, dst, g, live=2)
    assert r2["gP"].tolist() == [[2., 0.], [0., 0.]] and r2["gb3"].tolist() == [0.5] and r2["logits"].tolist() == [5., 3., 2., 3.]
    # parts of the source-sorted list: one per source
    lay = part_layout(src.numpy(), 1, 2)
    parts = torch.zeros(lay.n_parts, 2, dtype=torch.float64).index_add_(0, torch.from_numpy(lay.part_id), r["gh1"])
    assert parts.tolist() == [[2., 0.], [0., -0.75]]
    # a skip feature: h1pre of edge 1 becomes [-2 0] + 2 [1 1] = [0 2]
    t["cvec"] = torch.tensor([1., 1.])
    r3 = decoder_reference(t, src, dst, g, extra=torch.tensor([0., 2., 0., 0.]))
    # h1 = [0 2], h2pre = [-2, 0]: no unit of the second layer alive, logit 3, no gradient
    assert r3["logits"].tolist() == [5., 3., 2., 3.] and r3["gcvec"].tolist() == [0., 0.]


# ------------------------------------------------------------------------------------------------------------------
# GPU helpers
# ------------------------------------------------------------------------------------------------------------------
def _dev_tables(t):
    return {k: v.to(dev()).contiguous() for k, v in t.items()}


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev())


def _live_tensor(live):
    return None if live is None else torch.tensor([live], dtype=torch.int64, device=dev())


def _f32(x):
    """the float64 reference as the float32 it must be matched against (exact: asserted by the CPU tests)"""
    y = x.float()
    assert torch.equal(y.double(), x)
    return y


def call_S(td, p, q, pq_dtype, n, ei, g, extra, cvec, live, part_off, n_parts):
    """one S launch in given-gradient mode through the C ABI (pangnn_decoder_train_mixed; y NULL)"""
    from pangnn_amd import functional as PF
    lib, L = PF._lib.load(), PF._lib
    e = ei.shape[1]
    assert ei.dtype == torch.int64 and ei.is_contiguous() and int(ei.min()) >= 0 and int(ei.max()) < n
    assert g.numel() == e and (extra is None or extra.numel() == e) and p.shape[0] >= n and q.shape[0] >= n
    assert part_off is None or part_off.numel() == (e + 32 * chunk_tiles_expected(e) - 1) // (32 * chunk_tiles_expected(e))
    full = lambda *s: torch.full(s, SENTINEL, dtype=torch.float32, device=dev())     # noqa: E731
    out = SimpleNamespace(logits=full(e), rec=torch.zeros(e, 8, dtype=torch.int32, device=dev()),
                          parts=None if part_off is None else full(n_parts + GUARD, D), gW2=full(D, D), gw3=full(D),
                          gb3=full(1), gcvec=None if extra is None else full(D))
    ws = torch.empty(lib.pangnn_decoder_train_workspace_bytes(), dtype=torch.uint8, device=dev())
    L.check(lib.pangnn_decoder_train_mixed(
        p.data_ptr(), p.stride(0), q.data_ptr(), q.stride(0), pq_dtype, n, ei.data_ptr(), e, e, L.ptr(extra),
        L.ptr(cvec if extra is not None else None), td["W2"].data_ptr(), td["b2"].data_ptr(), td["w3"].data_ptr(),
        td["b3"].data_ptr(), D, None, None, 0, g.data_ptr(), out.logits.data_ptr(), None, out.rec.data_ptr(),
        L.ptr(out.parts), L.ptr(part_off), out.gW2.data_ptr(), out.gw3.data_ptr(), out.gb3.data_ptr(), L.ptr(out.gcvec),
        L.ptr(live), ws.data_ptr(), ws.numel(), L.stream_ptr()), "pangnn_decoder_train_mixed")
    return out


def call_T(rs, e, keys, part_off, n_parts, perm, live, want_b2):
    """one T launch through the C ABI (pangnn_decoder_dgrad_f32); keys = None: the parameter sum alone"""
    from pangnn_amd import functional as PF
    lib, L = PF._lib.load(), PF._lib
    n_rec = rs.rec.shape[0]
    assert (perm is None and e <= n_rec) or (perm.numel() == e and int(perm.min()) >= 0 and int(perm.max()) < n_rec)
    parts = None
    if keys is not None:
        ct = chunk_tiles_expected(e)
        assert lib.pangnn_decoder_chunk_tiles_for(e) == ct
        assert keys.numel() == e and keys.dtype == torch.int32 and part_off.numel() == (e + 32 * ct - 1) // (32 * ct)
        parts = torch.full((n_parts + GUARD, D), SENTINEL, dtype=torch.float32, device=dev())
    gb2 = torch.full((D,), SENTINEL, dtype=torch.float32, device=dev()) if want_b2 else None
    ws = torch.empty(lib.pangnn_decoder_dgrad_workspace_bytes(), dtype=torch.uint8, device=dev()) if want_b2 else None
    L.check(lib.pangnn_decoder_dgrad_f32(rs.rec.data_ptr(), L.ptr(perm), L.ptr(keys), rs.td["W2"].data_ptr(),
                                         rs.td["w3"].data_ptr(), e, L.ptr(parts), L.ptr(part_off), L.ptr(gb2),
                                         L.ptr(_live_tensor(live)), L.ptr(ws), 0 if ws is None else ws.numel(),
                                         L.stream_ptr()), "pangnn_decoder_dgrad_f32")
    return parts, gb2


def sum_parts(parts, part_rowptr, n_rows):
    from pangnn_amd import functional as PF
    plan = SimpleNamespace(part_rowptr=torch.from_numpy(part_rowptr).to(dev()))
    return PF._sum_parts(plan, parts, n_rows, torch.full((n_rows, D), SENTINEL, dtype=torch.float32, device=dev()))


@pytest.fixture(scope="module")
def recset():
    """records of the 4096-edge list from ONE S launch in given-gradient mode, and the float64 reference rows they stand for"""
    inp = rec_inputs()
    td = _dev_tables(inp.t)
    ei = torch.stack([inp.src, inp.dst]).to(dev()).contiguous()
    g = inp.g.to(dev())
    s = call_S(td, td["P"], td["Q"], 0, inp.n, ei, g, None, None, None, None, 0)
    ref = decoder_reference({k: v.double() for k, v in td.items()}, ei[0], ei[1], g.double(), rows=True)
    assert torch.equal(s.logits, _f32(ref["logits"]))
    assert torch.equal(s.rec[:, 4:], g.view(torch.int32)[:, None].expand(-1, 4))
    return SimpleNamespace(rec=s.rec, td=td, gh1=ref["gh1"], a=ref["a"], e=inp.e)


def check_T(rs, name, keys, n_rows, perm, live, want_b2, want_parts=True):
    """launch T on `keys` with the test's own part layout and compare parts, guard rows, per-row sums and dL/db2 bit for bit"""
    e = len(keys)
    ct = chunk_tiles_expected(e)
    lay = part_layout(keys, ct, n_rows)
    idx = torch.arange(e, device=dev()) if perm is None or not want_parts else perm.long()
    alive = (torch.arange(e, device=dev()) < (e if live is None else min(live, e))).double()[:, None]
    parts, gb2 = call_T(rs, e, _i32(keys) if want_parts else None, _i32(lay.part_off) if want_parts else None, lay.n_parts,
                        perm if want_parts else None, live, want_b2)
    if want_parts:
        rows = rs.gh1[idx] * alive
        want = torch.zeros(lay.n_parts, D, dtype=torch.float64, device=dev()).index_add_(0, torch.from_numpy(lay.part_id).to(dev()), rows)
        bad = (parts[:lay.n_parts] != _f32(want)).any(1)
        assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {lay.n_parts} parts differ, first {int(bad.nonzero()[0])}"
        assert bool((parts[lay.n_parts:] == SENTINEL).all()), f"{name}: a guard row was written"
        want_rows = torch.zeros(n_rows, D, dtype=torch.float64, device=dev()).index_add_(0, torch.from_numpy(keys).to(dev()), rows)
        got_rows = sum_parts(parts[:lay.n_parts], lay.part_rowptr, n_rows)
        assert torch.equal(got_rows, _f32(want_rows)), f"{name}: per-row sums"
    if want_b2:
        assert torch.equal(gb2, _f32((rs.a[idx] * alive).sum(0))), f"{name}: dL/db2"
    return parts, gb2


# ------------------------------------------------------------------------------------------------------------------
# GPU: the T kernel on keys of the test's choosing
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", T_CASES)
def test_T_kernel_run_sums_on_designed_keys(recset, name):
    """pangnn_decoder_dgrad_f32 with keys and part_off from the test's own definition.  The records come from a list of 4096
    edges; `perm` maps the designed positions onto those records and repeats edge ids where the list is longer — the kernel
    only gathers through `perm`.  Every real part, every guard row and every per-row sum bit for bit; dL/db2 along with the
    run sums for lists up to 2^18 positions."""
    keys, n_rows = case_keys(name)
    e = len(keys)
    check_T(recset, name, keys, n_rows, case_perm(name, e, recset.e).to(dev()), None, _wants_b2(e))


def _live_id(e):
    return lambda v: "live-" + {e - 33: "E-33", e - 1: "E-1", e: "E", e + 5: "E+5", None: "NULL"}.get(v, str(v))


@gpu
@pytest.mark.parametrize("live", [0, 1, 15, 16, 17, 31, 32, 33, LIVE_E - 33, LIVE_E - 1, LIVE_E, LIVE_E + 5, None],
                         ids=_live_id(LIVE_E))
def test_T_kernel_live_edges(recset, live):
    """positions >= min(live_edges, E) of the order contribute 0 to every part and to dL/db2; NULL: every position is real"""
    keys, n_rows = case_keys("live-list")
    check_T(recset, _live_id(LIVE_E)(live), keys, n_rows, case_perm("live-list", LIVE_E, recset.e).to(dev()), live, True)


@gpu
@pytest.mark.parametrize("kind", ["null", "identity", "random-permutation"])
def test_T_kernel_perm(recset, kind):
    keys, n_rows = case_keys("perm-list")
    perm = {"null": None, "identity": torch.arange(PERM_E, dtype=torch.int32),
            "random-permutation": torch.randperm(PERM_E, generator=torch.Generator().manual_seed(3)).to(torch.int32)}[kind]
    check_T(recset, kind, keys, n_rows, None if perm is None else perm.to(dev()), None, True)


@gpu
@pytest.mark.parametrize("how", ["with-run-sums", "alone"])
@pytest.mark.parametrize("live", [None, 1000], ids=["all-live", "live-1000"])
def test_T_kernel_db2(recset, how, live):
    """dL/db2 requested together with the run sums, and alone (keys, part_buf and part_off NULL: the positions are the
    records in list order); a second identical call gives the same bits"""
    keys, n_rows = case_keys("perm-list")
    perm = None if how == "alone" else torch.randperm(PERM_E, generator=torch.Generator().manual_seed(4)).to(torch.int32).to(dev())
    first = check_T(recset, how, keys, n_rows, perm, live, True, want_parts=how != "alone")
    again = check_T(recset, how, keys, n_rows, perm, live, True, want_parts=how != "alone")
    assert torch.equal(first[1], again[1]) and (how == "alone" or torch.equal(first[0], again[0]))


# ------------------------------------------------------------------------------------------------------------------
# GPU: the S kernel on source-sorted lists with designed run lengths
# ------------------------------------------------------------------------------------------------------------------
def _store(tab, how):
    """(p, q) device tensors for the tables stored as `how`"""
    P, Q = tab["P"], tab["Q"]
    if how == "windows-of-128":
        pq = torch.cat([P, Q], 1).contiguous()
        return pq[:, :D], pq[:, D:]
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[how]
    p, q = P.to(dt), Q.to(dt)
    assert torch.equal(p.float(), P) and torch.equal(q.float(), Q)          # the grid is exact in both 16-bit formats
    return p, q


def _s_reference(inp, td, ei, g, extra, live):
    t64 = {k: v.double() for k, v in td.items()}
    return decoder_reference(t64, ei[0], ei[1], g.double(), extra, live=live, rows=True)


def _check_train16(inp, td, ref, ei, g, extra, how, live, sorted_by_src):
    """functional._decoder_train16 in given-gradient mode (the library's own plans): every gradient bit for bit"""
    from pangnn_amd import functional as PF
    from pangnn_amd.graph import EdgeStructure
    p, q = _store(td, how)
    st = EdgeStructure(ei, inp.n)
    assert (st.runsum_plan(PF.d16_chunk(inp.e)) is not None) == sorted_by_src
    _, _, gp, gq, g_cv, g_w2, g_b2, g_w3, g_b3 = PF._decoder_train16(
        p, q, st, extra, td["cvec"] if extra is not None else None, td["W2"], td["b2"], td["w3"], td["b3"], g_logits=g,
        live=_live_tensor(live))
    got = dict(gP=gp, gQ=gq, gW2=g_w2, gb2=g_b2, gw3=g_w3, gb3=g_b3, gcvec=g_cv)
    for k in SUMS:
        if k == "gcvec" and extra is None:
            assert g_cv is None
            continue
        bad = got[k] != _f32(ref[k])
        assert not bool(bad.any()), f"{k}: {int(bad.sum())} entries differ"


@gpu
@pytest.mark.parametrize("s", S_SETS, ids=set_id)
def test_S_kernel_on_source_sorted_designed_runs(s):
    """pangnn_decoder_train_mixed in given-gradient mode, sources = the designed key sequence: logits, the run parts (own
    layout, guard rows), dL/dP out of the parts, the parameter gradients and dwords 4 .. 7 of every record through the C ABI;
    then every gradient again through functional._decoder_train16 and the library's own plans."""
    from pangnn_amd import functional as PF
    inp = s_inputs(*s)
    assert PF.d16_chunk(inp.e) == S_CHUNK_TILES[s[0]]
    td = _dev_tables(inp.t)
    ei = torch.stack([inp.src, inp.dst]).to(dev()).contiguous()
    g = inp.g.to(dev())
    extra = None if inp.extra is None else inp.extra.to(dev())
    ref = _s_reference(inp, td, ei, g, extra, None)
    lay = part_layout(inp.keys, S_CHUNK_TILES[s[0]], inp.n)
    out = call_S(td, td["P"], td["Q"], 0, inp.n, ei, g, extra, td["cvec"], None, _i32(lay.part_off), lay.n_parts)
    assert torch.equal(out.logits, _f32(ref["logits"]))
    assert torch.equal(out.rec[:, 4:], g.view(torch.int32)[:, None].expand(-1, 4))
    want = torch.zeros(lay.n_parts, D, dtype=torch.float64, device=dev()).index_add_(0, torch.from_numpy(lay.part_id).to(dev()), ref["gh1"])
    bad = (out.parts[:lay.n_parts] != _f32(want)).any(1)
    assert not bool(bad.any()), f"{int(bad.sum())} of {lay.n_parts} parts differ, first {int(bad.nonzero()[0])}"
    assert bool((out.parts[lay.n_parts:] == SENTINEL).all())
    assert torch.equal(sum_parts(out.parts[:lay.n_parts], lay.part_rowptr, inp.n), _f32(ref["gP"]))
    assert torch.equal(out.gW2, _f32(ref["gW2"])) and torch.equal(out.gw3, _f32(ref["gw3"]))
    assert torch.equal(out.gb3, _f32(ref["gb3"]))
    if extra is not None:
        assert torch.equal(out.gcvec, _f32(ref["gcvec"]))
    del out, want
    _check_train16(inp, td, ref, ei, g, extra, "f32", None, True)


@gpu
@pytest.mark.parametrize("how", ["windows-of-128", "bf16", "f16"])
@pytest.mark.parametrize("s", [("2^16", False), ("2^16", True), ("2^17+1", False)], ids=set_id)
def test_S_kernel_table_storage(s, how):
    """P and Q as column windows of one [N, 128] table, and stored as bfloat16 / float16 (the grid is exact in both): the same
    float64 reference bit for bit, hence the float32-table results bit for bit as well; logits through the C ABI too"""
    inp = s_inputs(*s)
    td = _dev_tables(inp.t)
    ei = torch.stack([inp.src, inp.dst]).to(dev()).contiguous()
    g = inp.g.to(dev())
    extra = None if inp.extra is None else inp.extra.to(dev())
    ref = _s_reference(inp, td, ei, g, extra, None)
    p, q = _store(td, how)
    out = call_S(td, p, q, {"windows-of-128": 0, "bf16": 1, "f16": 2}[how], inp.n, ei, g, extra, td["cvec"], None, None, 0)
    assert p.stride(0) == (128 if how == "windows-of-128" else 64)
    assert torch.equal(out.logits, _f32(ref["logits"])) and torch.equal(out.gW2, _f32(ref["gW2"]))
    _check_train16(inp, td, ref, ei, g, extra, how, None, True)


@gpu
@pytest.mark.parametrize("s", [("2^16", False), ("2^16", True), ("2^17+1", False)], ids=set_id)
def test_S_kernel_lists_in_random_order(s):
    """the same lists in a seeded random order: S makes no run sums and both dL/dP and dL/dQ come from T over the two CSR
    orders, bit for bit the same sums"""
    inp = s_inputs(*s)
    td = _dev_tables(inp.t)
    order = torch.randperm(inp.e, generator=torch.Generator().manual_seed(8))
    ei = torch.stack([inp.src[order], inp.dst[order]]).to(dev()).contiguous()
    g = inp.g[order].to(dev())
    extra = None if inp.extra is None else inp.extra[order].to(dev())
    ref = _s_reference(inp, td, ei, g, extra, None)
    _check_train16(inp, td, ref, ei, g, extra, "f32", None, False)


@gpu
@pytest.mark.parametrize("live", [0, 1, 17, (1 << 16) - 33, 1 << 16, (1 << 16) + 5], ids=_live_id(1 << 16))
@pytest.mark.parametrize("skip", [False, True], ids=["plain", "skip"])
def test_S_kernel_live_edges(skip, live):
    """a padded list: the edges >= live keep their logit and record slots but enter no sum.  As in a collated batch, the padded
    edges' targets are the largest node id (no real edge's is), so that they sort last in the by-target order as well.  A record
    holds dL/dlogit AS GIVEN also for a padded edge: T masks by position."""
    inp = s_inputs("2^16", skip)
    td = _dev_tables(inp.t)
    dst = inp.dst.clone()
    assert int(dst.max()) < inp.n - 1
    dst[min(live, inp.e):] = inp.n - 1
    src = inp.src                                                         # the designed runs, one of them across `live`
    ei = torch.stack([src, dst]).to(dev()).contiguous()
    g = inp.g.to(dev())
    extra = None if inp.extra is None else inp.extra.to(dev())
    ref = _s_reference(inp, td, ei, g, extra, live)
    lay = part_layout(src.numpy(), 1, inp.n)
    out = call_S(td, td["P"], td["Q"], 0, inp.n, ei, g, extra, td["cvec"], _live_tensor(live), _i32(lay.part_off), lay.n_parts)
    assert torch.equal(out.logits, _f32(ref["logits"]))
    assert torch.equal(out.rec[:, 4:], g.view(torch.int32)[:, None].expand(-1, 4))
    alive = (torch.arange(inp.e, device=dev()) < live).double()[:, None]
    want = torch.zeros(lay.n_parts, D, dtype=torch.float64, device=dev()).index_add_(0, torch.from_numpy(lay.part_id).to(dev()), ref["gh1"] * alive)
    assert torch.equal(out.parts[:lay.n_parts], _f32(want)) and bool((out.parts[lay.n_parts:] == SENTINEL).all())
    assert torch.equal(out.gW2, _f32(ref["gW2"])) and torch.equal(out.gb3, _f32(ref["gb3"]))
    _check_train16(inp, td, ref, ei, g, extra, "f32", live, True)


# ------------------------------------------------------------------------------------------------------------------
# GPU: the strict-fp32 kernels
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("s", STRICT_SETS, ids=set_id)
def test_strict_fp32_kernels(s):
    """pangnn_decoder_mlp_bwd_f32, precision 0: dL/dh1pre per edge, the one-tile-chunk parts (own layout, guard rows) and every
    parameter gradient through the C ABI; dL/dP and dL/dQ through functional._decoder_f32"""
    from pangnn_amd import functional as PF
    from pangnn_amd.graph import EdgeStructure
    lib, L = PF._lib.load(), PF._lib
    inp = s_inputs(*s)
    e, n = inp.e, inp.n
    td = _dev_tables(inp.t)
    ei = torch.stack([inp.src, inp.dst]).to(dev()).contiguous()
    g = inp.g.to(dev())
    extra = None if inp.extra is None else inp.extra.to(dev())
    cv = td["cvec"] if extra is not None else None
    ref = _s_reference(inp, td, ei, g, extra, None)
    lay = part_layout(inp.keys, 1, n)
    full = lambda *sh: torch.full(sh, SENTINEL, dtype=torch.float32, device=dev())     # noqa: E731
    gh1, parts = full(e, D), full(lay.n_parts + GUARD, D)
    gW2, gb2, gw3, gb3, gcv = full(D, D), full(D), full(D), full(1), (full(D) if cv is not None else None)
    part_off = _i32(lay.part_off)
    assert part_off.numel() == (e + 31) // 32
    ws = torch.empty(lib.pangnn_decoder_mlp_bwd_workspace_bytes(e), dtype=torch.uint8, device=dev())
    L.check(lib.pangnn_decoder_mlp_bwd_f32(
        td["P"].data_ptr(), D, td["Q"].data_ptr(), D, n, ei.data_ptr(), e, e, L.ptr(extra), L.ptr(cv), td["W2"].data_ptr(),
        td["b2"].data_ptr(), td["w3"].data_ptr(), td["b3"].data_ptr(), D, g.data_ptr(), gh1.data_ptr(), gW2.data_ptr(),
        gb2.data_ptr(), gw3.data_ptr(), gb3.data_ptr(), L.ptr(gcv), parts.data_ptr(), part_off.data_ptr(), 0, ws.data_ptr(),
        ws.numel(), L.stream_ptr()), "pangnn_decoder_mlp_bwd_f32")
    assert torch.equal(gh1, _f32(ref["gh1"]))
    want = torch.zeros(lay.n_parts, D, dtype=torch.float64, device=dev()).index_add_(0, torch.from_numpy(lay.part_id).to(dev()), ref["gh1"])
    assert torch.equal(parts[:lay.n_parts], _f32(want)) and bool((parts[lay.n_parts:] == SENTINEL).all())
    assert torch.equal(sum_parts(parts[:lay.n_parts], lay.part_rowptr, n), _f32(ref["gP"]))
    for k, got in (("gW2", gW2), ("gb2", gb2), ("gw3", gw3), ("gb3", gb3), ("gcvec", gcv)):
        assert got is None or torch.equal(got, _f32(ref[k])), k
    old, PF.DECODER_PRECISION = PF.DECODER_PRECISION, 0
    try:
        r = PF._decoder_f32(td["P"], td["Q"], EdgeStructure(ei, n), extra, cv, td["W2"], td["b2"], td["w3"], td["b3"], g_logits=g)
    finally:
        PF.DECODER_PRECISION = old
    for k, got in zip(("gP", "gQ", "gcvec", "gW2", "gb2", "gw3", "gb3"), r[2:]):
        assert got is None or torch.equal(got, _f32(ref[k])), k


# ------------------------------------------------------------------------------------------------------------------
# GPU: the public routes
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", [1, 0], ids=["bf16x3", "f32mfma"])
@pytest.mark.parametrize("route", ["ctypes", "dispatcher"])
def test_public_decoder_routes(route, mode):
    """functional.decoder_mlp (ctypes) and torch.ops.pangnn.decoder_mlp (dispatcher) in both DECODER_PRECISION modes, a
    gradient vector from the grid back-propagated: logits and all leaf gradients equal the reference bit for bit — and so
    each other, across routes and modes"""
    from pangnn_amd import functional as PF
    from pangnn_amd import torch_ops
    from pangnn_amd.graph import EdgeStructure
    inp = s_inputs("2^16", True)
    td = _dev_tables(inp.t)
    ei = torch.stack([inp.src, inp.dst]).to(dev()).contiguous()
    g, extra = inp.g.to(dev()), inp.extra.to(dev())
    ref = _s_reference(inp, td, ei, g, extra, None)
    st = EdgeStructure(ei, inp.n)
    leaf = {k: td[k].clone().requires_grad_(True) for k in ("cvec", "W2", "b2", "w3", "b3")}
    old, PF.DECODER_PRECISION = PF.DECODER_PRECISION, mode
    try:
        if route == "ctypes":
            p, q = td["P"].clone().requires_grad_(True), td["Q"].clone().requires_grad_(True)
            out = PF.decoder_mlp(p, q, st, extra, leaf["cvec"], leaf["W2"], leaf["b2"], leaf["w3"], leaf["b3"])
            out.backward(g)
            gp, gq = p.grad, q.grad
        else:
            pq = torch.cat([td["P"], td["Q"]], 1).requires_grad_(True)
            out = torch_ops.decoder_mlp_pq(pq, st, extra, leaf["cvec"], leaf["W2"], leaf["b2"], leaf["w3"], leaf["b3"])
            out.backward(g)
            gp, gq = pq.grad[:, :D], pq.grad[:, D:]
    finally:
        PF.DECODER_PRECISION = old
    assert torch.equal(out.detach(), _f32(ref["logits"]))
    got = dict(gP=gp, gQ=gq, gW2=leaf["W2"].grad, gb2=leaf["b2"].grad, gw3=leaf["w3"].grad, gb3=leaf["b3"].grad,
               gcvec=leaf["cvec"].grad)
    for k in SUMS:
        assert torch.equal(got[k], _f32(ref[k])), k
