"""The node-level dense kernels of csrc/linear.hip, bit for bit, on operand grids whose every intermediate is a float32.

Every product of that file runs one scheme: both operands are truncated into three bf16 terms (hi + mid + lo, 8 + 8 + 8
significand bits), six of the nine partial products go through v_mfma_f32_32x32x16_bf16 smallest first, and the three of
order 2^-24 (mid.lo, lo.mid, lo.lo) are dropped.  The method is that of tests/test_decoder_run_sums.py: on a suitable grid
a plain float64 evaluation, rounded ONCE to float32 (and once more, to nearest even, where the result is stored in 16
bits), must be matched bit for bit whatever the matrix pipe's internal adder does.  Two conditions make a grid exact
(`_assert_exact_in_any_order`, asserted for every input set before any kernel sees it):

  1. each product is representable: the significant-bit spans of the two factors add up to <= 24.  The dropped terms then
     vanish by themselves (a non-zero lo needs a span >= 17, a non-zero mid one >= 9, and 17 + 9 - 1 > 24);
  2. each sum is exact in any order: all its terms are multiples of one unit u and their absolute values sum to < 2^24 u.
     The truncation split keeps signs, so the partial products of the split obey the bound of the products themselves.

Four operand classes isolate the six terms (a = the row operand, b = the operand it is contracted with):

  H    a, b integers below 16 in magnitude                               hi.hi, and pure addressing
  MM   a, b odd integers in 257 .. 511 (b: 64 non-zeros per row of 128)   mid.mid, mid.hi, hi.mid
  XL   a odd integers in (2^16, 2^17), b in {0, +-1}                      lo.hi, mid.hi
  WL   a in {0, +-1}, b odd integers in (2^16, 2^17)                      hi.lo, hi.mid

`test_dropping_a_term_is_caught_by_its_class` shows with a numpy emulation of the split and the six-term chain that the
emulation equals float64 on every grid and that leaving out any one term changes most outputs of the class meant to catch
it.  ELU is pinned on pre-activations from {positive grid values, 0, -128}: elu = v, 0, -1 and elu' = 1, 1, 0 exactly
(__expf(-128) underflows to +0; in float64 expm1(-128) == -1 and exp(-128) times any output here rounds to 0 in float32).
A whole operand may carry a factor 2^-10 (so that float16 results stay finite); every value stays in the normal range.

There is no tolerance in this file: `torch.equal` is its only comparison of a kernel's output.

What the cases cover, per entry point (terms / window edges / tiles per wave):
  pangnn_linear_act_fwd_mixed    all six terms at (K, M) in {64, 128}^2, plain / in_act / gated, bias and none, every
                                 storage triple launch_fwd compiles; columns beyond M and rows >= n of a wider y, NaN around
                                 x and gate; 1, 2 and 3 tiles per wave, the partial tile after 0, 1 and 2 full ones
  pangnn_linear_dgrad_mixed      the same through stage_w's transpose strides, with and without gate
  pangnn_linear_act_wgrad_mixed  all six terms, in_act 0 / 1, gb and none, every storage pair launch_wgrad compiles; guards
                                 around gw and gb, NaN around g and x; 1, 2 and 3 tiles per wave with g non-zero in chosen tiles
  pangnn_embed_linear_fwd / _bwd hi.hi and the lo / mid terms of the GENERATED rows (all three ELU branches), y inside a wider
                                 buffer, three full tiles and a partial one; the backward also at three tiles per wave
  pangnn_linear_act_backward_parts_f32   classes H and MM, rows of 0 .. 3 parts in both tables, positions >= n_parts, gx inside
                                 a wider buffer; class H at three tiles per wave (row pointers fetched two tiles ahead)
  functional.linear              classes H and MM under autograd on the dispatcher op (the function's only route)
A 16-bit operand carries 8 (bfloat16) or 11 (float16) significant bits: a class runs in a storage format only where its
values fit (`_fits`), i.e. bfloat16 operands take the narrow side of H / XL / WL, float16 ones also MM (a non-zero mid).
Left out, and why: MM / XL (WL) with a bfloat16 row (weight-gradient: either) operand and XL / WL with a float16 one — the
format cannot hold the values; classes MM and WL at the two long row counts (the issue of tiles per wave is addressing: H and
one wide class); the weight's mid / lo terms in the generated-first-layer kernels (the same stage_w and mfma6_fwd, pinned by the
forward cases) and the generated forward beyond one tile per wave (rows of h are distinct only while (r, s) pairs are, the
narrow grid has 256 of them, and that kernel's second tile starts beyond 131 072 rows); exact float16 ties at an inner
dimension of 64 (class H results rarely pass 2048 there)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
F64 = torch.float64
CODE = {F32: 0, BF16: 1, F16: 2}               # PANGNN_DTYPE_*
BITS = {F32: 24, BF16: 8, F16: 11}             # significant bits of a stored value
SENTINEL = {F32: -7.5e33, BF16: -7.5e33, F16: -1234.0}     # what unwritten output elements hold
LD, OFF, GUARD = 192, 64, 8                    # window tests: leading dimension, column offset, guard rows behind row n
NOMINAL_CUS = 256                              # the CPU tests size their grids for an MI355X
SHAPES = [(64, 64), (64, 128), (128, 64), (128, 128)]
CLASSES = {"H": ("small", "small"), "MM": ("mid", "mid"), "XL": ("wide", "unit"), "WL": ("unit", "wide")}
KIND_BITS = {"small": 4, "unit": 1, "mid": 9, "wide": 17}
TERMS = [("lo", "hi"), ("hi", "lo"), ("mid", "mid"), ("mid", "hi"), ("hi", "mid"), ("hi", "hi")]     # mfma6_*'s order
PINS = {"H": [("hi", "hi")], "MM": [("mid", "mid"), ("mid", "hi"), ("hi", "mid")], "XL": [("lo", "hi"), ("mid", "hi")],
        "WL": [("hi", "lo"), ("hi", "mid")]}
SCALE16 = 2.0 ** -10                           # on the weight of a wide class whose result is stored in 16 bits
STORAGE = [(F32, F32), (BF16, F32), (F32, BF16), (BF16, BF16), (F16, F32), (F32, F16), (F16, F16)]


def _name(dt):
    return {F32: "f32", BF16: "bf16", F16: "f16"}[dt]


def _ids(pairs):
    return [f"{_name(a)}-{_name(b)}" for a, b in pairs]


# ------------------------------------------------------------------------------------------------------------------
# grids
# ------------------------------------------------------------------------------------------------------------------
def _draw(kind, shape, gen, signed=True):
    """float64 values of one operand kind, random signs (or none)"""
    ri = lambda lo, hi: torch.randint(lo, hi, shape, generator=gen).to(F64)                # noqa: E731
    if kind == "small":
        mag = ri(0, 16)
    elif kind == "unit":
        mag = (torch.rand(shape, generator=gen) < 2 / 3).to(F64)
    elif kind == "mid":
        mag = 257 + 2 * ri(0, 128)                                   # odd, 257 .. 511: hi and mid both non-zero
    else:                                                            # odd, (2^16, 2^17), bit 8 set: the 9 bits below hi are
        mag = 2 ** 16 + 2 ** 9 * ri(0, 128) + 2 ** 8 + 2 * ri(0, 128) + 1    # a full mid and a lo of 1 — all three terms non-zero
    return mag * (2 * ri(0, 2) - 1) if signed else mag


def _sparse_rows_of_128(b, gen):
    """class MM at an inner dimension of 128: 64 non-zeros per row, a different 64 per row"""
    keep = torch.rand(b.shape, generator=gen).argsort(1).argsort(1) < 64
    return b * keep


def _elu_pre(mag, gen):
    """(pre-activation, ELU of it) from unsigned grid values: 1/8 of the entries become 0, 1/8 become -128 (ELU = -1)"""
    u = torch.rand(mag.shape, generator=gen)
    pre = torch.where(u < 0.125, torch.zeros_like(mag), torch.where(u < 0.25, torch.full_like(mag, -128.0), mag))
    return pre, elu_ref(pre)


def _gate(shape, gen):
    """gate values from {1 .. 15, 0, -128}: ELU' = 1, 1, 0"""
    u = torch.rand(shape, generator=gen)
    pos = torch.randint(1, 16, shape, generator=gen).to(F64)
    return torch.where(u < 0.25, torch.zeros_like(pos), torch.where(u < 0.5, torch.full_like(pos, -128.0), pos))


def elu_ref(v):
    return torch.where(v > 0, v, torch.expm1(v))


def elu_grad_ref(v):
    return torch.where(v > 0, torch.ones_like(v), torch.exp(v))


def _span_unit(t):
    """(largest number of significant bits, value of the lowest set bit) over the non-zero entries of a float64 tensor
    whose values are float32s"""
    t = t[t != 0].to(F64).reshape(-1)
    assert t.numel() > 0
    assert torch.equal(t.float().double(), t), "not float32 values"
    m, e = torch.frexp(t)
    i = (m.abs() * 2 ** 24).to(torch.int64)
    low = i & -i
    tz = torch.log2(low.double()).to(torch.int64)
    return int((24 - tz).max()), 2.0 ** int((e.to(torch.int64) - 24 + tz).min())


def _assert_exact_in_any_order(a, b, extra=None):
    """out[i][j] = sum_l a[i][l] b[j][l] (+ extra[j]): (1) every product is a float32 — the spans of the factors add up to
    <= 24 bits; (2) all terms of a sum are multiples of one unit and their magnitudes sum to < 2^24 units, so every partial
    sum in every order and grouping (the split's partial products included: truncation keeps signs) is a float32.  Values
    and units stay far inside the normal range of bf16 / float32.  Returns the unit."""
    (sa, ua), (sb, ub) = _span_unit(a), _span_unit(b)
    assert sa + sb <= 24, (sa, sb)
    u = ua * ub
    mag = a.abs().to(F64) @ b.abs().to(F64).t()
    if extra is not None:
        assert torch.equal(torch.round(extra / u) * u, extra), "bias off the unit grid"
        mag = mag + extra.abs()
    assert float(mag.max()) < 2 ** 24 * u, (float(mag.max()) / (2 ** 24 * u))
    assert min(ua, ub, u) >= 2.0 ** -60 and max(float(a.abs().max()), float(b.abs().max()), float(mag.max())) < 2.0 ** 60
    return u


def _assert_informative(ref):
    """no all-zero row or column and no two equal rows: a misplaced, dropped or duplicated row cannot pass.  (Columns are
    looked at from 16 rows on: below that a gate of slope 0 zeroes whole columns of a one- or few-row result by design.)"""
    assert bool((ref != 0).any(1).all()), "a reference row is all zero"
    assert ref.shape[0] < 16 or bool((ref != 0).any(0).all()), "a reference column is all zero"
    assert torch.unique(ref, dim=0).shape[0] == ref.shape[0], "two reference rows are equal"


def _fits(kind, dtype):
    return KIND_BITS[kind] <= BITS[dtype]


def _ties(ref, dtype):
    """number of reference values that are exact ties of the 16-bit format (its first dropped bit set, nothing below)"""
    bits = ref.to(F32).contiguous().view(torch.int32)
    cut = 16 if dtype == BF16 else 13
    normal = ref.abs() >= (2.0 ** -14 if dtype == F16 else 2.0 ** -126)
    return int((((bits & ((1 << cut) - 1)) == (1 << (cut - 1))) & normal & torch.isfinite(ref.to(F32).to(dtype).float())).sum())


# ------------------------------------------------------------------------------------------------------------------
# cases: CPU tensors in float64 (inputs, the two operands of the contraction, the reference), built once and left unchanged
# ------------------------------------------------------------------------------------------------------------------
def _memo_small(build):
    """cases up to 4096 rows are built once and shared (and left unchanged); the few long ones are rebuilt where they are used
    instead of being kept alive for the whole session"""
    cached = functools.lru_cache(maxsize=None)(build)

    @functools.wraps(build)
    def get(K, M, cls, n, *args, **kw):
        return cached(K, M, cls, n, *args, **kw) if n <= 4096 else build(K, M, cls, n, *args, **kw)
    return get


@_memo_small
def fwd_case(K, M, cls, n, act=False, gated=False, bias=False, scaled=False, seed=0):
    """y [n, M] = elu?(x) w^T (+ bias) (* elu'(gate)); scaled: w (and bias) of a wide class carry 2^-10"""
    gen = torch.Generator().manual_seed(1000 * K + 10 * M + n + 7 * seed + sum(map(ord, cls)))
    ka, kb = CLASSES[cls]
    a = _draw(ka, (n, K), gen, signed=not act)
    x, a = _elu_pre(a, gen) if act else (a, a)
    w = _draw(kb, (M, K), gen)
    if cls == "MM" and K > 64:
        w = _sparse_rows_of_128(w, gen)
    s = SCALE16 if scaled and cls != "H" else 1.0
    w = w * s
    b = torch.randint(-15, 16, (M,), generator=gen).to(F64) * s if bias else None
    g = _gate((n, M), gen) if gated else None
    _assert_exact_in_any_order(a, w, b)
    ref = a @ w.t()
    if b is not None:
        ref = ref + b
    if gated:
        ref = ref * elu_grad_ref(g)
    return SimpleNamespace(x=x, w=w, bias=b, gate=g, a=a, b=w, ref=ref, cls=cls)


def dgrad_case(K, M, cls, n, gated=False, scaled=False, seed=0):
    """gx [n, K] = g [n, M] w (* elu'(gate)) for the layer's own weight w [M, K]: the forward product with the roles of K and
    M exchanged and the operand [K][M] staged through the strides of the transpose"""
    c = fwd_case(M, K, cls, n, False, gated, False, scaled, seed + 3)
    return SimpleNamespace(g=c.x, w=c.w.t().contiguous(), gate=c.gate, a=c.a, b=c.b, ref=c.ref, cls=cls)


def wgrad_rows(n, cus=NOMINAL_CUS):
    """the rows on which g is non-zero: all of them up to n = 64 (the table of the module docstring carries over unchanged);
    for a longer matrix three rows of each tile chosen by design — a wave's first, second and third tile (two waves each), the
    last full tile and the partial tile — so that condition 2 holds and every one of those tiles is visible in the sums"""
    if n <= 64:
        return torch.arange(n)
    n_tiles, n_full = (n + 31) // 32, n // 32
    stride = 4 * min((n_tiles + 3) // 4, cus)
    tiles = {0, 1, stride, stride + 1, 2 * stride, 2 * stride + 2, n_full - 1, n_tiles - 1}
    rows = sorted({32 * t + o for t in tiles if 0 <= t < n_tiles for o in (0, 17, 31) if 32 * t + o < n} | {n - 1})
    return torch.tensor(rows)


@_memo_small
def wgrad_case(K, M, cls, n, act=False, cus=NOMINAL_CUS, seed=0):
    """gw [M, K] = g^T elu?(x), gb [M] = column sums of g: the row operand is g^T, the sum runs over the n rows"""
    gen = torch.Generator().manual_seed(2000 * K + 20 * M + n + 7 * seed + sum(map(ord, cls)))
    ka, kb = CLASSES[cls]
    rows = wgrad_rows(n, cus)
    g = torch.zeros(n, M, dtype=F64)
    g[rows] = _draw(ka, (rows.numel(), M), gen)
    xe = _draw(kb, (n, K), gen, signed=not act)
    x, xe = _elu_pre(xe, gen) if act else (xe, xe)
    _assert_exact_in_any_order(g.t(), xe.t())
    _assert_exact_in_any_order(g.t(), torch.ones(1, n, dtype=F64))
    return SimpleNamespace(g=g, x=x, a=g.t().contiguous(), b=xe.t().contiguous(), gw=g.t() @ xe, gb=g.sum(0), cls=cls, rows=rows)


def fwd_classes(tx):
    """the classes whose row operand fits the storage type tx (the weight is always float32)"""
    return [c for c, (ka, _) in CLASSES.items() if _fits(ka, tx)]


def wgrad_classes(tg, tx):
    return [c for c, (ka, kb) in CLASSES.items() if _fits(ka, tg) and _fits(kb, tx)]


FWD_VARIANTS = [dict(act=a, gated=g, bias=b) for a, g in ((False, False), (True, False), (False, True)) for b in (False, True)]


def tile_sizes(waves, cus):
    """tail only, one full tile, full tile plus tail; one workgroup exactly full, a row short, a row over; every wave of a full
    grid takes a second tile and the tail goes to a wave that skipped none; a third tile (the `tile + 2 stride` prefetch is
    live) and the tail goes to a wave after two iterations"""
    return [1, 31, 32, 33, 32 * waves - 1, 32 * waves, 32 * waves + 1, 32 * cus * waves + 33, 64 * cus * waves + 69]


def fwd_waves(K, M):
    return 3 if K == 128 and M == 128 else 4         # FwdGeo<K, M>::WAVES


def most_tiles_per_wave(n, waves, cus):
    n_tiles = (n + 31) // 32
    grid = min((n_tiles + waves - 1) // waves, cus)
    return (n_tiles + grid * waves - 1) // (grid * waves)


def tile_cases(cus, wgrad):
    """(K, M, class, n) of the tiles-per-wave cases, for the forward kernel (and dL/dx, the same kernel) with its FwdGeo waves
    per workgroup or for the weight gradient with its four: every shape for the sizes of one workgroup, the two square shapes
    for the two sizes that walk a full grid twice and three times; class H and one wide class"""
    out = []
    for K, M in SHAPES:
        sizes = tile_sizes(4 if wgrad else fwd_waves(K, M), cus)
        for n in sizes[:7] + (sizes[7:] if K == M else []):
            out += [(K, M, c, n) for c in ("H", "XL")]
    return out


# ------------------------------------------------------------------------------------------------------------------
# numpy emulation of split8 / stage_w and of the six-term chain
# ------------------------------------------------------------------------------------------------------------------
def split3(v):
    v = np.ascontiguousarray(v, dtype=np.float32)
    trunc = lambda a: (a.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)         # noqa: E731
    hi = trunc(v)
    r1 = v - hi
    mid = trunc(r1)
    r2 = r1 - mid
    lo = trunc(r2)
    assert np.array_equal(hi.astype(np.float64) + mid + lo, v.astype(np.float64)), "x = hi + mid + lo exactly"
    for t in (hi, mid, lo):                                         # no subnormal term
        assert not np.any((t != 0) & (np.abs(t) < 2.0 ** -126))
    return dict(hi=hi, mid=mid, lo=lo)


def term_products(a, b):
    """the six partial products of the split operands, each one exact in float64"""
    sa, sb = split3(a.numpy()), split3(b.numpy())
    return {(ta, tb): sa[ta].astype(np.float64) @ sb[tb].astype(np.float64).T for ta, tb in TERMS}


def chain(products, drop=None):
    """the sum of the six terms in mfma6's order, every accumulation rounded to float32"""
    acc = None
    for t in TERMS:
        if t != drop:
            acc = products[t].astype(np.float32) if acc is None else (acc.astype(np.float64) + products[t]).astype(np.float32)
    return acc


def _witness(a, b, cls, what):
    products = term_products(a, b)
    full = chain(products)
    ref = (a @ b.t()).float().numpy()
    assert np.array_equal(full, ref), (what, "the six-term chain is not the float64 product")
    for t in PINS[cls]:
        changed = float((chain(products, drop=t) != full).mean())
        assert changed > 0.5, (what, "dropping", t, "changes only", changed)


# ------------------------------------------------------------------------------------------------------------------
# CPU part
# ------------------------------------------------------------------------------------------------------------------
# every (description, row operand, contracted operand, class, reference matrix) a GPU case of sections 1 - 3 uses; the derived
# kernels' cases have their own tests next to them
def _term_grids(cus=NOMINAL_CUS):
    for K, M in SHAPES:
        for cls in CLASSES:
            for scaled in (False, True):
                for v in FWD_VARIANTS:
                    c = fwd_case(K, M, cls, 33, scaled=scaled, **v)
                    yield ("fwd", K, M, cls, scaled, tuple(v.items())), c.a, c.b, cls, c.ref
                for gated in (False, True):
                    c = dgrad_case(K, M, cls, 33, gated, scaled)
                    yield ("dgrad", K, M, cls, scaled, gated), c.a, c.b, cls, c.ref
            for act in (False, True):
                c = wgrad_case(K, M, cls, 33, act)
                yield ("wgrad", K, M, cls, act), c.a, c.b, cls, c.gw


def _tile_grids(cus=NOMINAL_CUS):
    for K, M, cls, n in tile_cases(cus, False):
        c = fwd_case(K, M, cls, n, bias=True)
        yield ("fwd tiles", K, M, cls, n), c.a, c.b, cls, c.ref
        c = dgrad_case(K, M, cls, n, True)
        yield ("dgrad tiles", K, M, cls, n), c.a, c.b, cls, c.ref
    for K, M, cls, n in tile_cases(cus, True):
        c = wgrad_case(K, M, cls, n, False, cus)
        # one row: gw is the outer product of two vectors, its rows are multiples of each other by construction
        yield ("wgrad tiles", K, M, cls, n), c.a, c.b, cls, (c.gw if n > 1 else None)


def _window_grids(cus=NOMINAL_CUS):
    for K, M in SHAPES:
        for cls in ("H", "MM"):
            n = 32 * fwd_waves(K, M) + 1
            for v in FWD_VARIANTS[1::2]:
                c = fwd_case(K, M, cls, n, **v)
                yield ("fwd window", K, M, cls, tuple(v.items())), c.a, c.b, cls, c.ref
            c = dgrad_case(K, M, cls, n, True)
            yield ("dgrad window", K, M, cls), c.a, c.b, cls, c.ref
            c = wgrad_case(K, M, cls, 33, True)
            yield ("wgrad window", K, M, cls), c.a, c.b, cls, c.gw


def test_grids_have_the_spans_their_class_needs():
    """class H stays inside hi; MM has hi and mid but no lo; the wide operand of XL / WL has all three; {0, +-1} only hi"""
    gen = torch.Generator().manual_seed(0)
    for kind, want in (("small", (True, False, False)), ("unit", (True, False, False)), ("mid", (True, True, False)),
                       ("wide", (True, True, True))):
        v = _draw(kind, (64, 64), gen)
        s = split3(v.numpy())
        nz = v.numpy() != 0
        got = tuple(bool(np.all(s[t][nz] != 0)) for t in ("hi", "mid", "lo"))
        none = tuple(bool(np.all(s[t] == 0)) for t in ("hi", "mid", "lo"))
        assert got == want and none == tuple(not w for w in want), (kind, got, none)
        assert _span_unit(v)[0] <= KIND_BITS[kind]
        for dt in (BF16, F16):                      # what `_fits` says is what the format holds
            assert torch.equal(v.to(dt).double(), v) == _fits(kind, dt), (kind, dt)
    pre, act = _elu_pre(_draw("wide", (64, 64), gen, signed=False), gen)
    assert set(torch.unique(act[pre <= 0]).tolist()) == {0.0, -1.0}
    assert torch.equal(act.float().double(), act) and torch.equal(elu_ref(pre.float()).double(), act)
    g = _gate((64, 64), gen)
    assert torch.equal(elu_grad_ref(g).float(), (g >= 0).float())            # 1, 1, 0 after the one rounding to float32
    assert float(torch.exp(torch.tensor(-128.0, dtype=F64)) * 2 ** 24) < 2.0 ** -150


@pytest.mark.parametrize("grids,at_least,pins", [(_term_grids, 288, set(TERMS)),
                                                 (_tile_grids, 192, set(PINS["H"] + PINS["XL"])),
                                                 (_window_grids, 40, set(PINS["H"] + PINS["MM"]))],
                         ids=["terms", "tiles", "windows"])
def test_dropping_a_term_is_caught_by_its_class(grids, at_least, pins):
    """for every grid a GPU case uses: both exactness conditions hold (asserted when the case is built), the emulated six-term
    chain equals the float64 product, dropping any one of the six terms changes most outputs of the class that pins it, and
    the reference has no zero row or column and no two equal rows"""
    seen, pinned = 0, set()
    for what, a, b, cls, ref in grids():
        _witness(a, b, cls, what)                       # (both exactness conditions: asserted where the case is built)
        if ref is not None:
            _assert_informative(ref)
        pinned |= set(PINS[cls])
        seen += 1
    assert pinned == pins and seen >= at_least, (pinned, seen)


def test_sixteen_bit_references_contain_exact_ties():
    """a 16-bit result is the float32 reference rounded to nearest even: class H results (10 .. 14 significant bits) hold exact
    ties of bfloat16 in every case and of float16 (values beyond 2048) wherever the inner dimension is 128"""
    for K, M in SHAPES:
        for v in FWD_VARIANTS:
            ref = fwd_case(K, M, "H", 33, **v).ref
            assert _ties(ref, BF16) > 0, (K, M, v)
            assert K < 128 or _ties(ref, F16) > 0, (K, M, v)
        for gated in (False, True):
            ref = dgrad_case(K, M, "H", 33, gated).ref
            assert _ties(ref, BF16) > 0 and (M < 128 or _ties(ref, F16) > 0), (K, M, gated)
    for cls in ("MM", "XL", "WL"):                  # scaled: finite in float16
        ref = fwd_case(128, 128, cls, 33, scaled=True).ref
        assert bool(torch.isfinite(ref.float().to(F16).float()).all()) and float(ref.abs().max()) > 2048


def test_sizes_reach_three_tiles_per_wave():
    for K, M in SHAPES:
        for waves in (fwd_waves(K, M), 4):
            sizes = tile_sizes(waves, NOMINAL_CUS)
            assert [most_tiles_per_wave(n, waves, NOMINAL_CUS) for n in sizes] == [1] * 7 + [2, 3]
    rows = wgrad_rows(tile_sizes(4, NOMINAL_CUS)[-1])
    stride = 4 * NOMINAL_CUS
    tiles = set((rows // 32).tolist())
    assert {0, stride, 2 * stride, 2 * stride + 2} <= tiles and rows.numel() <= 64
    assert int(rows[-1]) == tile_sizes(4, NOMINAL_CUS)[-1] - 1


# ------------------------------------------------------------------------------------------------------------------
# GPU part
# ------------------------------------------------------------------------------------------------------------------
def dev():
    return torch.device("cuda:0")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _put(t, dtype=F32):
    """the float64 grid tensor in its storage type on the device; the conversion is exact or the case is wrong"""
    if t is None:
        return None
    out = t.to(dtype)
    assert torch.equal(out.double(), t), "grid value does not fit its storage type"
    return out.to(dev())


def _expect(ref, dtype):
    """evaluate in float64, round once to float32, once more (nearest even) where the result is stored in 16 bits"""
    return ref.to(F32).to(dtype).to(dev())


def _window(t, dtype, fill, width):
    """(buffer [rows + GUARD, LD] full of `fill`, its window [rows, width] at column OFF holding t)"""
    rows = t.shape[0] if t is not None else width[0]
    w = t.shape[1] if t is not None else width[1]
    buf = torch.full((rows + GUARD, LD), fill, dtype=dtype, device=dev())
    view = buf[:rows, OFF:OFF + w]
    if t is not None:
        view.copy_(_put(t, dtype))
    return buf, view


def _fwd(x, w, bias, y, K, M, in_act=0, gate=None):
    from pangnn_amd import _lib
    lib = _lib.load()
    with torch.cuda.device(dev()):
        _lib.check(lib.pangnn_linear_act_fwd_mixed(
            x.data_ptr(), CODE[x.dtype], x.stride(0), w.data_ptr(), _lib.ptr(bias), y.data_ptr(), CODE[y.dtype], y.stride(0),
            x.shape[0], K, M, in_act, _lib.ptr(gate), CODE[gate.dtype] if gate is not None else 0,
            gate.stride(0) if gate is not None else 0, _lib.stream_ptr()), "pangnn_linear_act_fwd_mixed")


def _dgrad(g, w, gx, K, M, gate=None):
    from pangnn_amd import _lib
    lib = _lib.load()
    with torch.cuda.device(dev()):
        _lib.check(lib.pangnn_linear_dgrad_mixed(
            g.data_ptr(), CODE[g.dtype], g.stride(0), w.data_ptr(), gx.data_ptr(), CODE[gx.dtype], gx.stride(0), g.shape[0], K, M,
            _lib.ptr(gate), CODE[gate.dtype] if gate is not None else 0, gate.stride(0) if gate is not None else 0,
            _lib.stream_ptr()), "pangnn_linear_dgrad_mixed")


def _wgrad(g, x, K, M, in_act, gw, gb):
    from pangnn_amd import _lib
    lib = _lib.load()
    ws_bytes = lib.pangnn_linear_wgrad_workspace_bytes(K, M)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev())
    with torch.cuda.device(dev()):
        _lib.check(lib.pangnn_linear_act_wgrad_mixed(
            g.data_ptr(), CODE[g.dtype], g.stride(0), x.data_ptr(), CODE[x.dtype], x.stride(0), g.shape[0], K, M, in_act,
            gw.data_ptr(), _lib.ptr(gb), ws.data_ptr(), ws_bytes, _lib.stream_ptr()), "pangnn_linear_act_wgrad_mixed")


def _out(n, width, dtype):
    return torch.full((n, width), SENTINEL[dtype], dtype=dtype, device=dev())


# ---- 1. terms ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("K,M", SHAPES)
@pytest.mark.parametrize("tx,ty", STORAGE, ids=_ids(STORAGE))
def test_forward_terms(K, M, tx, ty):
    """pangnn_linear_act_fwd_mixed at n = 33: plain, in_act = 1 and gated (gate stored like y), with and without bias, for
    every class whose row operand fits x's storage: bfloat16 x (8 bits) runs H and WL — it has neither mid nor lo, the wide
    operand sits on the float32 weight —, float16 x (11 bits: a non-zero mid) also MM, float32 x all four"""
    n, ran = 33, 0
    for cls in fwd_classes(tx):
        for v in FWD_VARIANTS:
            c = fwd_case(K, M, cls, n, scaled=ty != F32, **v)
            x, w, b, gate = _put(c.x, tx), _put(c.w), _put(c.bias), _put(c.gate, ty)
            y = _out(n, M, ty)
            _fwd(x, w, b, y, K, M, int(v["act"]), gate)
            assert torch.equal(y, _expect(c.ref, ty)), (cls, v)
            ran += 1
    assert ran >= 12


@gpu
@pytest.mark.parametrize("K,M", SHAPES)
@pytest.mark.parametrize("tg,tx", STORAGE, ids=_ids(STORAGE))
def test_dgrad_terms(K, M, tg, tx):
    """pangnn_linear_dgrad_mixed: gx = g w from the layer's own [M, K] weight (stage_w through the transpose strides), with
    and without gate (stored like gx); the classes follow g's storage as in the forward test"""
    n, ran = 33, 0
    for cls in fwd_classes(tg):
        for gated in (False, True):
            c = dgrad_case(K, M, cls, n, gated, tx != F32)
            g, w, gate = _put(c.g, tg), _put(c.w), _put(c.gate, tx)
            gx = _out(n, K, tx)
            _dgrad(g, w, gx, K, M, gate)
            assert torch.equal(gx, _expect(c.ref, tx)), (cls, gated)
            ran += 1
    assert ran >= 4


@gpu
@pytest.mark.parametrize("K,M", SHAPES)
@pytest.mark.parametrize("tg,tx", STORAGE, ids=_ids(STORAGE))
def test_wgrad_terms(K, M, tg, tx):
    """pangnn_linear_act_wgrad_mixed at n = 33, in_act 0 and 1, gb present and null: both operands are data, so a class runs
    where BOTH fit their storage — bfloat16 on a side leaves H and the class whose wide operand is on the other, float32 side;
    float16 on both sides still runs MM"""
    n, ran = 33, 0
    for cls in wgrad_classes(tg, tx):
        for act in (False, True):
            c = wgrad_case(K, M, cls, n, act)
            g, x = _put(c.g, tg), _put(c.x, tx)
            for with_gb in (True, False):
                gw = torch.full((M, K), SENTINEL[F32], device=dev())
                gb = torch.full((M,), SENTINEL[F32], device=dev())
                _wgrad(g, x, K, M, int(act), gw, gb if with_gb else None)
                assert torch.equal(gw, _expect(c.gw, F32)), (cls, act, with_gb)
                assert torch.equal(gb, _expect(c.gb, F32) if with_gb else torch.full_like(gb, SENTINEL[F32])), (cls, act)
                ran += 1
    assert ran >= 4


# ---- 2. windows ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("K,M", SHAPES)
@pytest.mark.parametrize("dt", [F32, F16], ids=["f32", "f16"])
def test_forward_and_dgrad_stay_inside_their_windows(K, M, dt):
    """x, gate and y are windows (column 64 of a leading dimension of 192, 8 guard rows behind row n) of buffers that hold NaN
    around the inputs and a sentinel around the output: every element outside y's window keeps its bits, and no NaN reaches
    a result.  n = one workgroup's tiles plus one row: full tiles and the partial tile's predicated path"""
    n = 32 * fwd_waves(K, M) + 1
    nan = float("nan")
    for cls in ("H", "MM"):
        for v in FWD_VARIANTS[1::2]:                                     # with bias
            c = fwd_case(K, M, cls, n, **v)
            _, x = _window(c.x, dt, nan, None)
            _, gate = _window(c.gate, dt, nan, None) if c.gate is not None else (None, None)
            ybuf, y = _window(None, dt, SENTINEL[dt], (n, M))
            want = ybuf.clone()
            want[:n, OFF:OFF + M] = _expect(c.ref, dt)
            _fwd(x, _put(c.w), _put(c.bias), y, K, M, int(v["act"]), gate)
            assert torch.equal(ybuf, want), ("fwd", cls, v)
        c = dgrad_case(K, M, cls, n, True)
        _, g = _window(c.g, dt, nan, None)
        _, gate = _window(c.gate, dt, nan, None)
        xbuf, gx = _window(None, dt, SENTINEL[dt], (n, K))
        want = xbuf.clone()
        want[:n, OFF:OFF + K] = _expect(c.ref, dt)
        _dgrad(g, _put(c.w), gx, K, M, gate)
        assert torch.equal(xbuf, want), ("dgrad", cls)


@gpu
@pytest.mark.parametrize("K,M", SHAPES)
@pytest.mark.parametrize("dt", [F32, F16], ids=["f32", "f16"])
def test_wgrad_reads_and_writes_inside_its_windows(K, M, dt):
    """g and x are windows of NaN-filled buffers (rows >= n of the partial tile and the columns around them); gw and gb sit
    between sentinel guards of one allocation"""
    n, pad = 33, 64
    for cls in ("H", "MM"):
        c = wgrad_case(K, M, cls, n, True)
        _, g = _window(c.g, dt, float("nan"), None)
        _, x = _window(c.x, dt, float("nan"), None)
        out = torch.full((pad + M * K + pad + M + pad,), SENTINEL[F32], device=dev())
        want = out.clone()
        gw, gb = out[pad:pad + M * K].view(M, K), out[pad + M * K + pad:pad + M * K + pad + M]
        want[pad:pad + M * K] = _expect(c.gw, F32).reshape(-1)
        want[pad + M * K + pad:pad + M * K + pad + M] = _expect(c.gb, F32)
        _wgrad(g, x, K, M, 1, gw, gb)
        assert torch.equal(out, want), cls


# ---- 3. tiles per wave -----------------------------------------------------------------------------------------------
def _tile_params(wgrad):
    return tile_cases(_cus() if torch.cuda.is_available() else NOMINAL_CUS, wgrad)


@gpu
@pytest.mark.parametrize("K,M,cls,n", _tile_params(False))
def test_tiles_per_wave_forward_and_dgrad(K, M, cls, n):
    """forward (bias) and gated dL/dx at the sizes of `tile_sizes` for the device at hand: tail only, exactly full workgroups,
    and full grids walked twice and three times — the last size gives some wave three tiles, so the `tile + 2 stride`
    prefetch is live, and hands the partial tile to a wave that has been through the loop twice"""
    cus, waves = _cus(), fwd_waves(K, M)
    if n == tile_sizes(waves, cus)[-1]:
        assert most_tiles_per_wave(n, waves, cus) >= 3
    c = fwd_case(K, M, cls, n, bias=True)
    y = torch.full((n + GUARD, M), SENTINEL[F32], device=dev())
    want = y.clone()
    want[:n] = _expect(c.ref, F32)
    _fwd(_put(c.x), _put(c.w), _put(c.bias), y[:n], K, M)
    assert torch.equal(y, want), "fwd"
    c = dgrad_case(K, M, cls, n, True)
    gx = torch.full((n + GUARD, K), SENTINEL[F32], device=dev())
    want = gx.clone()
    want[:n] = _expect(c.ref, F32)
    _dgrad(_put(c.g), _put(c.w), gx[:n], K, M, _put(c.gate))
    assert torch.equal(gx, want), "dgrad"


@gpu
@pytest.mark.parametrize("K,M,cls,n", _tile_params(True))
def test_tiles_per_wave_wgrad(K, M, cls, n):
    """the weight gradient at the same kinds of sizes for its four waves per workgroup; beyond 64 rows g is non-zero on the rows
    of `wgrad_rows` only (a wave's first, second and third tile, the last full tile, the partial tile), x is dense"""
    cus = _cus()
    if n == tile_sizes(4, cus)[-1]:
        assert most_tiles_per_wave(n, 4, cus) >= 3
    c = wgrad_case(K, M, cls, n, False, cus)
    gw, gb = torch.full((M, K), SENTINEL[F32], device=dev()), torch.full((M,), SENTINEL[F32], device=dev())
    _wgrad(_put(c.g), _put(c.x), K, M, 0, gw, gb)
    assert torch.equal(gw, _expect(c.gw, F32)), "gw"
    assert torch.equal(gb, _expect(c.gb, F32)), "gb"


# ---- 4. derived kernels ----------------------------------------------------------------------------------------------
def _embed_build(H, M, wide, n, cus=NOMINAL_CUS):
    """the first layer by linearity, h = fma(r, a, fma(s, c, b)) with a = W_in w_emb, c = W_in b_emb (D = 2, w_emb = (1, 0),
    b_emb = (0, 1): a and c are the two columns of W_in), then y = elu(h) W_out^T + bias and its backward.
    narrow: r, s in 0 .. 15 (distinct pairs), a, c in 0 .. 7, b in 0 .. 15: h < 256 has no mid, W_out and g are class H.
    wide: r, s, a, c in 128 .. 255, so h in (2^15, 2^17) carries mid and, mostly, lo; W_out and g are in {0, +-1}.  Row 0 has
    r = s = 0 in both: its h is b_in.
    One column in eight has a = c = 0 and b = -128 (ELU = -1, ELU' = 0); h = 0 occurs (ELU' = 1).
    More than 255 rows (the backward's long case; y is not used then): the pairs repeat, and g is non-zero on `wgrad_rows`."""
    gen = torch.Generator().manual_seed(31 * H + M + wide + n)
    base, top, atop = (128, 128, 128) if wide else (0, 16, 8)
    if n < top * top:
        pairs = torch.randperm(top * top - 1, generator=gen)[:n] + 1     # distinct (r, s): distinct rows of h
    else:
        pairs = torch.randint(0, top * top, (n,), generator=gen)
    r, s = (base + pairs // top).to(F64), (base + pairs % top).to(F64)
    r[0] = s[0] = 0
    w_in = (base + torch.randint(0, atop, (H, 2), generator=gen)).to(F64)
    b_in = torch.randint(0, 16, (H,), generator=gen).to(F64)
    dead = torch.rand(H, generator=gen) < 0.125
    dead[5], dead[6] = True, False
    w_in[dead], b_in[dead] = 0.0, -128.0
    b_in[6] = 0.0                                                  # row 0 (r = s = 0) meets h = 0 here
    w_emb, b_emb = torch.tensor([1.0, 0.0], dtype=F64), torch.tensor([0.0, 1.0], dtype=F64)
    a, cc = w_in @ w_emb, w_in @ b_emb
    h = r[:, None] * a + (s[:, None] * cc + b_in)
    assert float(h[0, 6]) == 0 and float(h[0, 5]) == -128 and bool(((h > 0) | (h == 0) | (h == -128)).all())
    assert float(h.abs().max()) < (2 ** 17 if wide else 256)
    xe = elu_ref(h)
    kind = "unit" if wide else "small"
    w_out = _draw(kind, (M, H), gen)
    bias = torch.randint(-15, 16, (M,), generator=gen).to(F64)
    rows = wgrad_rows(n, cus) if n >= top * top else torch.arange(n)
    g = torch.zeros(n, M, dtype=F64)
    g[rows] = _draw(kind, (rows.numel(), M), gen)
    _assert_exact_in_any_order(xe, w_out, bias)                    # forward
    _assert_exact_in_any_order(g.t(), xe.t())                      # dL/dW_out
    _assert_exact_in_any_order(g.t(), torch.ones(1, n, dtype=F64))
    _assert_exact_in_any_order(g, w_out.t())                       # g W_out
    v = (g @ w_out) * elu_grad_ref(h)
    v = v.float().double()
    rs1 = torch.stack([r, s, torch.ones(n, dtype=F64)])
    _assert_exact_in_any_order(rs1, v.t())                         # the three weighted column sums
    return SimpleNamespace(r=r, s=s, w_emb=w_emb, b_emb=b_emb, w_in=w_in, b_in=b_in, w_out=w_out, bias=bias, g=g, xe=xe,
                           y=xe @ w_out.t() + bias, gw=g.t() @ xe, gb=g.sum(0), sums=rs1 @ v)


@functools.lru_cache(maxsize=None)
def embed_case(H, M, wide):
    return _embed_build(H, M, wide, 97)


def test_generated_first_layer_grids_are_exact_and_informative():
    for H, M in SHAPES[:3]:
        c = _embed_build(H, M, False, tile_sizes(4, NOMINAL_CUS)[-1])
        _assert_informative(c.gw)
        _witness(c.g.t().contiguous(), c.xe.t().contiguous(), "H", ("embed wgrad, long", H, M))
        for wide in (False, True):
            c = embed_case(H, M, wide)
            _assert_informative(c.y)
            _assert_informative(c.gw)
            _witness(c.xe, c.w_out, "XL" if wide else "H", ("embed fwd", H, M, wide))
            _witness(c.g.t().contiguous(), c.xe.t().contiguous(), "WL" if wide else "H", ("embed wgrad", H, M, wide))


@gpu
@pytest.mark.parametrize("H,M", SHAPES[:3])
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_generated_first_layer(H, M, wide):
    """pangnn_embed_linear_fwd / _bwd against float64; y sits in a wider buffer with guard rows"""
    _run_embed(embed_case(H, M, wide), H, M)


@gpu
@pytest.mark.parametrize("H,M", SHAPES[:3])
def test_generated_first_layer_backward_three_tiles_per_wave(H, M):
    """gen_linear_wgrad_kernel and gen_linear_dgrad_sums_kernel (four waves per workgroup for these shapes) walk a full grid
    three times; g is non-zero on the rows of `wgrad_rows`, so each of a wave's three tiles and the partial tile shows in
    dL/dW_out, dL/db_out and the three weighted column sums.  (The forward runs too; its long result is not compared: equal
    (r, s) pairs give equal rows.)"""
    cus = _cus()
    n = tile_sizes(4, cus)[-1]
    assert most_tiles_per_wave(n, 4, cus) >= 3
    _run_embed(_embed_build(H, M, False, n, cus), H, M, check_y=False)


def _run_embed(c, H, M, check_y=True):
    from pangnn_amd import _lib
    lib = _lib.load()
    n = c.r.numel()
    r, s, w_emb, b_emb, w_in, b_in, w_out, bias, g = (_put(t) for t in (c.r, c.s, c.w_emb, c.b_emb, c.w_in, c.b_in, c.w_out,
                                                                         c.bias, c.g))
    ybuf, y = _window(None, F32, SENTINEL[F32], (n, M))
    want = ybuf.clone()
    want[:n, OFF:OFF + M] = _expect(c.y, F32)
    gw, gb = torch.full((M, H), SENTINEL[F32], device=dev()), torch.full((M,), SENTINEL[F32], device=dev())
    sums = torch.full((3, H), SENTINEL[F32], device=dev())
    ws_bytes = lib.pangnn_embed_linear_bwd_workspace_bytes(H, M)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev())
    with torch.cuda.device(dev()):
        _lib.check(lib.pangnn_embed_linear_fwd(r.data_ptr(), s.data_ptr(), n, w_emb.data_ptr(), b_emb.data_ptr(), w_in.data_ptr(),
                                               b_in.data_ptr(), 2, H, w_out.data_ptr(), bias.data_ptr(), M, y.data_ptr(),
                                               y.stride(0), _lib.stream_ptr()), "pangnn_embed_linear_fwd")
        _lib.check(lib.pangnn_embed_linear_bwd(g.data_ptr(), g.stride(0), r.data_ptr(), s.data_ptr(), n, w_emb.data_ptr(),
                                               b_emb.data_ptr(), w_in.data_ptr(), b_in.data_ptr(), 2, H, w_out.data_ptr(), M,
                                               gw.data_ptr(), gb.data_ptr(), sums.data_ptr(), ws.data_ptr(), ws_bytes,
                                               _lib.stream_ptr()), "pangnn_embed_linear_bwd")
    if check_y:
        assert torch.equal(ybuf, want), "y"
    assert torch.equal(gw, _expect(c.gw, F32)), "g_w_out"
    assert torch.equal(gb, _expect(c.gb, F32)), "g_b_out"
    assert torch.equal(sums, _expect(c.sums, F32)), "sums"


@functools.lru_cache(maxsize=None)
def parts_case(cls, in_act, n=50):
    """the P | Q layer's backward from run parts (K = 64, M = 128): G [n, 128] on the class's grid, cut into 0 .. 3 integer
    parts per row and table (all sixteen combinations of the two counts occur; a row without parts has G = 0); the last row's
    parts of both tables lie at positions >= n_parts — they count as absent — and hold NaN.  x is a pre-activation from
    {positive, 0, -128} with in_act, a signed grid value without."""
    gen = torch.Generator().manual_seed(sum(map(ord, cls)) + in_act)
    ka, kb = CLASSES[cls]
    K, M = 64, 128
    cnt = torch.randint(0, 4, (2, n), generator=gen)
    cnt[0, :16], cnt[1, :16] = torch.arange(16) // 4, torch.arange(16) % 4
    cnt[:, n - 1] = 2
    G = _draw(ka, (n, M), gen)
    tables = []
    for h in range(2):
        rowptr = torch.zeros(n + 1, dtype=torch.int64)
        rowptr[1:] = torch.cumsum(cnt[h], 0)
        parts = torch.zeros(int(rowptr[-1]), 64, dtype=F64)
        for i in range(n):
            k, tgt = int(cnt[h, i]), G[i, 64 * h:64 * h + 64]
            if k == 0:
                tgt.zero_()
                continue
            p = torch.randint(-64, 65, (k, 64), generator=gen).to(F64)
            p[k - 1] = tgt - p[:k - 1].sum(0)
            parts[rowptr[i]:rowptr[i + 1]] = p
            for j in range(1, k + 1):                              # the kernel's own partial sums: small integers
                assert float(p[:j].sum(0).abs().max()) < 2 ** 12
        n_parts = int(rowptr[n - 1])                               # the last row's two parts are out of range
        parts[n_parts:] = float("nan")
        G[n - 1, 64 * h:64 * h + 64] = 0
        tables.append((parts, rowptr, n_parts))
    w = _draw(kb, (M, K), gen)
    if cls == "MM":                                                # operand of G w: [K][M], rows of 128
        w = _sparse_rows_of_128(w.t().contiguous(), gen).t().contiguous()
    if in_act:
        x, xe = _elu_pre(_draw(kb, (n, K), gen, signed=False), gen)
    else:
        x = xe = _draw(kb, (n, K), gen)
    _assert_exact_in_any_order(G, w.t())
    _assert_exact_in_any_order(G.t(), xe.t())
    _assert_exact_in_any_order(G.t(), torch.ones(1, n, dtype=F64))
    gx = G @ w
    if in_act:
        gx = gx * elu_grad_ref(x)
    return SimpleNamespace(tables=tables, x=x, xe=xe, w=w, G=G, cnt=cnt, gx=gx, gx_plain=G @ w, gw=G.t() @ xe, gb=G.sum(0))


def test_part_table_grids_are_exact_and_informative():
    for cls in ("H", "MM"):
        for in_act in (0, 1):
            c = parts_case(cls, in_act)
            assert {(int(a), int(b)) for a, b in c.cnt.t()} >= {(a, b) for a in range(4) for b in range(4)}
            _witness(c.G, c.w.t().contiguous(), cls, ("parts dgrad", cls))
            _witness(c.G.t().contiguous(), c.xe.t().contiguous(), cls, ("parts wgrad", cls))
            _assert_informative(c.gx_plain[(c.G != 0).any(1)])     # (a row without parts in either table: G = 0, gx = 0)
            _assert_informative(c.gw)


@gpu
@pytest.mark.parametrize("cls", ["H", "MM"])
@pytest.mark.parametrize("in_act", [0, 1])
def test_pq_backward_from_parts(cls, in_act):
    """pangnn_linear_act_backward_parts_f32 against float64, not only against the unfused sequence; gx is a window of a wider
    buffer with guard rows"""
    _run_parts(parts_case(cls, in_act), in_act)


def _run_parts(c, in_act):
    from pangnn_amd import _lib
    lib, n = _lib.load(), c.x.shape[0]
    (ps, rs, ns), (pt, rt, nt) = c.tables
    ps_d, pt_d = ps.float().to(dev()), pt.float().to(dev())          # (NaN rows behind n_parts: not through _put)
    rs_d, rt_d = rs.to(dev()), rt.to(dev())
    x, w = _put(c.x), _put(c.w)
    gxbuf, gx = _window(None, F32, SENTINEL[F32], (n, 64))
    want = gxbuf.clone()
    want[:n, OFF:OFF + 64] = _expect(c.gx, F32)
    gw, gb = torch.full((128, 64), SENTINEL[F32], device=dev()), torch.full((128,), SENTINEL[F32], device=dev())
    ws_bytes = lib.pangnn_linear_wgrad_workspace_bytes(64, 128)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev())
    with torch.cuda.device(dev()):
        _lib.check(lib.pangnn_linear_act_backward_parts_f32(
            ps_d.data_ptr(), rs_d.data_ptr(), ns, pt_d.data_ptr(), rt_d.data_ptr(), nt, x.data_ptr(), 64, w.data_ptr(), n, 64, 128,
            in_act, gx.data_ptr(), gx.stride(0), gw.data_ptr(), gb.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr()),
            "pangnn_linear_act_backward_parts_f32")
    assert torch.equal(gxbuf, want), "gx"
    assert torch.equal(gw, _expect(c.gw, F32)), "gw"
    assert torch.equal(gb, _expect(c.gb, F32)), "gb"


def parts_case_long(n, seed=0):
    """class H over many rows, built from the parts: 0 .. 3 parts per row and table with entries in -5 .. 5, so |G| <= 15;
    the last row's parts are out of range as in `parts_case`; x is a pre-activation from {1 .. 15, 0, -128}"""
    gen = torch.Generator().manual_seed(n + seed)
    K, M = 64, 128
    G = torch.zeros(n, M, dtype=F64)
    tables = []
    for h in range(2):
        cnt = torch.randint(0, 4, (n,), generator=gen)
        cnt[n - 1] = 2
        rowptr = torch.zeros(n + 1, dtype=torch.int64)
        rowptr[1:] = torch.cumsum(cnt, 0)
        parts = torch.randint(-5, 6, (int(rowptr[-1]), 64), generator=gen).to(F64)
        n_parts = int(rowptr[n - 1])
        row_of = torch.repeat_interleave(torch.arange(n), cnt)[:n_parts]
        G[:, 64 * h:64 * h + 64].index_add_(0, row_of, parts[:n_parts])
        parts[n_parts:] = float("nan")
        tables.append((parts, rowptr, n_parts))
    w = _draw("small", (M, K), gen)
    x, xe = _elu_pre(_draw("small", (n, K), gen, signed=False), gen)
    _assert_exact_in_any_order(G, w.t())
    _assert_exact_in_any_order(G.t(), xe.t())
    _assert_exact_in_any_order(G.t(), torch.ones(1, n, dtype=F64))
    return SimpleNamespace(tables=tables, x=x, xe=xe, w=w, G=G, gx=(G @ w) * elu_grad_ref(x), gx_plain=G @ w, gw=G.t() @ xe,
                           gb=G.sum(0))


def test_long_part_table_grid_is_exact_and_informative():
    n = tile_sizes(4, NOMINAL_CUS)[-1]
    c = parts_case_long(n)
    _witness(c.G, c.w.t().contiguous(), "H", "long parts dgrad")
    _witness(c.G.t().contiguous(), c.xe.t().contiguous(), "H", "long parts wgrad")
    _assert_informative(c.gx_plain[(c.G != 0).any(1)])
    _assert_informative(c.gw)


@gpu
def test_pq_backward_from_parts_three_tiles_per_wave():
    """the fused kernel walks a full grid three times: its row pointers are fetched two tiles ahead (`tile + 2 stride`), the
    first parts one tile ahead, and the partial tile goes to a wave that has carried its accumulators through two tiles"""
    n = tile_sizes(4, _cus())[-1]
    assert most_tiles_per_wave(n, 4, _cus()) >= 3
    _run_parts(parts_case_long(n), 1)


@functools.lru_cache(maxsize=None)
def autograd_case(cls, in_act):
    """a forward case at (K, M) = (64, 128) with bias and an upstream gradient g on the class's grid (class MM: 64 non-zeros per
    row of 128, as for every contraction of that length): y, dL/dx, dL/dw and dL/db in float64"""
    K, M, n = 64, 128, 33
    f = fwd_case(K, M, cls, n, act=bool(in_act), bias=True)
    gen = torch.Generator().manual_seed(5 + in_act)
    g = _draw(CLASSES[cls][0], (n, M), gen)
    if cls == "MM":
        g = _sparse_rows_of_128(g, gen)
    _assert_exact_in_any_order(g, f.w.t())                         # dL/dx = g w
    _assert_exact_in_any_order(g.t(), f.a.t())                     # dL/dw = g^T elu?(x)
    _assert_exact_in_any_order(g.t(), torch.ones(1, n, dtype=F64))
    gx = g @ f.w
    if in_act:
        gx = gx * elu_grad_ref(f.x)
    return SimpleNamespace(f=f, g=g, gx=gx, gx_plain=g @ f.w, gw=g.t() @ f.a, gb=g.sum(0))


def test_autograd_grids_are_exact_and_informative():
    for cls in ("H", "MM"):
        for in_act in (0, 1):
            c = autograd_case(cls, in_act)
            _witness(c.g, c.f.w.t().contiguous(), cls, ("autograd dgrad", cls))
            _witness(c.g.t().contiguous(), c.f.a.t().contiguous(), cls, ("autograd wgrad", cls))
            _assert_informative(c.gx_plain)
            _assert_informative(c.gw)


@gpu
@pytest.mark.parametrize("cls", ["H", "MM"])
@pytest.mark.parametrize("in_act", [0, 1])
def test_functional_linear_under_autograd(cls, in_act):
    """one pass through functional.linear and its backward on the dispatcher op — the only route that function has (its
    docstring: the ctypes twin is gone): output and the three gradients against float64"""
    from pangnn_amd import functional as PF
    c = autograd_case(cls, in_act)
    x = _put(c.f.x).requires_grad_(True)
    w, b = _put(c.f.w).requires_grad_(True), _put(c.f.bias).requires_grad_(True)
    out = PF.linear(x, w, b, in_act)
    out.backward(_put(c.g))
    assert torch.equal(out.detach(), _expect(c.f.ref, F32)), "y"
    assert torch.equal(x.grad, _expect(c.gx, F32)), "dL/dx"
    assert torch.equal(w.grad, _expect(c.gw, F32)), "dL/dw"
    assert torch.equal(b.grad, _expect(c.gb, F32)), "dL/db"
