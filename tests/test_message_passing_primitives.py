"""The generic message-passing kernels ("literal route"), branch by branch, through the C ABI.

Plain references (numpy / torch-CPU, float64 where something is summed) are defined first and checked on the CPU against
independent torch formulations; the GPU tests then compare every kernel with them.

Tolerances.  A sum of L fp32 terms, in ANY order, with at most a handful of extra roundings per element (the fma products
are exact, bias and prior content are one addition each), differs from the exact sum by at most

    (L + 8) * 2^-24 * S          S = sum of the absolute values of the terms (|bias| and |prior out| included)

(the standard bound gamma_k S with k <= L + 2 and room for the second-order terms up to L = 10^4).  That is the only
tolerance on sums here; `max`, the gathers and the permutation are bit-exact, and the fused multiply-add of edge_pair_add
is compared with a float64 emulation within 1 ulp (see ref_pair_add).  One more bound exists, in
test_propagate_lifts_two_node_tensors with aggr = 'max' only: there the messages themselves are computed by torch in fp32
(three roundings each) and compared with a float64 module, so the maximum of a row is held to (1 + u)^3 - 1 < 4 * 2^-24
times the largest |message| of that row — the rounding of the inputs of the kernel, not of the kernel, which copies.

Which case selects which instantiation of pangnn_spmm_csr_f32's dispatch (test_spmm_csr ids; `main` has E >= 8 n):

    row<F>-...          F in {16, 32, 64, 128, 256}, aligned, ld % 4 == 0, nnz >= 8 n   spmm_row_kernel<F, 4>
    row<F>-wide         the same through ldx = F + 4, ldo = F + 8 views                 spmm_row_kernel<F, 4>
    thin<F>-...         F in {64, 128}, nnz = 8 n - 1                                   spmm_thin_kernel<F>
    row<F>-nnz=-1       the thin graph with nnz = -1 (no hint)                          spmm_row_kernel<F, 4>
    row<F>-nnz=8n       E = 8 n exactly                                                 spmm_row_kernel<F, 4>
    generic-F<F>-...    F in {1, 3, 20, 63, 65, 130, 257}                               spmm_row_generic_kernel
    generic-F<F>-ldx=F+1 / -out+1float      a vector F with an odd ldx / a misaligned out   spmm_row_generic_kernel
    ...-idxNULL / -valNULL / -acc1 / -bias1     the in-kernel branches of whichever kernel the rest of the id names
test_segment_sum_rows ids: `w=2F` message matrices with col_off in {0, 4, F} stay on the vector kernel (row<F>, or thin<F>
on the thin graph), `w=2F+1` (odd ldm) goes to the generic kernel.
pangnn_edge_gather_concat_f32 (test_gather_concat ids): `vec` = gather_concat_kernel<true> (no extra, D % 4 == 0, ldz % 4 ==
0, ldo % 4 == 0), `scalar` = gather_concat_kernel<false>.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import random_graph

U = 2.0 ** -24
SENT = -12345.0
F_MAX = 130                                   # segment_max references are computed once at this width and sliced


# ===================================================================================================================
# 1. references
# ===================================================================================================================
def ref_segment_sum(rowptr, perm, m, col_off, f, out0=None):
    """out[r] = (out0[r] +) sum_{k in row r} m[perm[k], col_off : col_off + f] in float64, and the sum of |terms|"""
    m64 = np.asarray(m, dtype=np.float64)
    n = len(rowptr) - 1
    out, s = np.zeros((n, f)), np.zeros((n, f))
    if out0 is not None:
        out += np.asarray(out0, dtype=np.float64)
        s += np.abs(np.asarray(out0, dtype=np.float64))
    for r in range(n):
        rows = perm[rowptr[r]:rowptr[r + 1]]
        if len(rows):
            t = m64[rows, col_off:col_off + f]
            out[r] += t.sum(0)
            s[r] += np.abs(t).sum(0)
    return out, s


def ref_spmm(rowptr, idx, val, x, bias, out0):
    """out[r] = (out0[r] +) bias + sum_{k in row r} val[k] x[idx[k]] in float64 (idx None: identity, val None: ones), and
    the sum of |terms|"""
    x64 = np.asarray(x, dtype=np.float64)
    n, f = len(rowptr) - 1, x64.shape[1]
    out, s = np.zeros((n, f)), np.zeros((n, f))
    if bias is not None:
        out += np.asarray(bias, dtype=np.float64)
        s += np.abs(np.asarray(bias, dtype=np.float64))
    if out0 is not None:
        out += np.asarray(out0, dtype=np.float64)
        s += np.abs(np.asarray(out0, dtype=np.float64))
    for r in range(n):
        b, e = int(rowptr[r]), int(rowptr[r + 1])
        if e > b:
            t = x64[np.arange(b, e) if idx is None else idx[b:e]]
            if val is not None:
                t = t * np.asarray(val[b:e], dtype=np.float64)[:, None]
            out[r] += t.sum(0)
            s[r] += np.abs(t).sum(0)
    return out, s


def ref_segment_max(rowptr, perm, m):
    """(out, arg): a literal walk over each row's entries in stored order on the float32 values themselves (max is exact).
    The first entry is taken; a later one replaces it when it is strictly greater, or when it is NaN and the best so far is
    not.  Rows without entries: out = 0, arg = -1."""
    m = np.asarray(m, dtype=np.float32)
    n, f = len(rowptr) - 1, m.shape[1]
    out = np.zeros((n, f), dtype=np.float32)
    arg = np.full((n, f), -1, dtype=np.int32)
    with np.errstate(invalid="ignore"):
        for r in range(n):
            b, e = int(rowptr[r]), int(rowptr[r + 1])
            if e == b:
                continue
            best = m[perm[b]].copy()
            bi = np.full(f, perm[b], dtype=np.int32)
            for k in range(b + 1, e):
                o = perm[k]
                v = m[o]
                take = (v > best) | ((v != v) & (best == best))
                best[take] = v[take]
                bi[take] = o
            out[r], arg[r] = best, bi
    return out, arg


def ref_segment_max_bwd(g, arg, num_edges):
    g = np.asarray(g, dtype=np.float32)
    gm = np.zeros((num_edges, g.shape[1]), dtype=np.float32)
    r, f = np.nonzero(arg >= 0)
    gm[arg[r, f], f] = g[r, f]
    return gm


def ref_gather_concat(z, ei, e_begin, n_edges, extra=None):
    s, d = ei[0, e_begin:e_begin + n_edges], ei[1, e_begin:e_begin + n_edges]
    parts = [z[s], z[d]]
    if extra is not None:
        parts.append(extra[e_begin:e_begin + n_edges, None])
    return np.concatenate(parts, axis=1)


def ref_pair_add(p, q, ei, e_begin, n_edges, extra=None, cvec=None):
    """fp32 p[src] + q[dst]; with extra / cvec the kernel's fmaf(w, c, a + b), emulated as float64(float32(a + b)) +
    float64(w) * float64(c) rounded to fp32: the float64 product is exact, but the float64 sum is rounded once before the
    rounding to fp32 (double rounding), so the emulation may be 1 ulp from the single-rounded fma — callers allow 1 ulp."""
    s, d = ei[0, e_begin:e_begin + n_edges], ei[1, e_begin:e_begin + n_edges]
    a = (p[s] + q[d]).astype(np.float32)
    if extra is None:
        return a
    w = extra[e_begin:e_begin + n_edges].astype(np.float64)[:, None]
    return (a.astype(np.float64) + w * cvec.astype(np.float64)[None, :]).astype(np.float32)


def ref_permute(x, perm):
    return x[perm]


def csr_np(key, n_rows):
    """rows = key, entries in ascending original id (a stable sort): what EdgeStructure builds"""
    key = np.asarray(key)
    perm = np.argsort(key, kind="stable")
    rowptr = np.searchsorted(key[perm], np.arange(n_rows + 1), side="left")
    return rowptr.astype(np.int64), perm.astype(np.int32)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def within_sum_bound(got, ref, s, lengths, what=""):
    """asserts |got - ref| <= (L + 8) 2^-24 S element by element; the message names the worst element"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    bound = (np.asarray(lengths, dtype=np.float64).reshape(-1, *([1] * (ref.ndim - 1))) + 8.0) * U * s
    bad = err > bound
    if bad.any():
        i = np.unravel_index(np.argmax(err - bound), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside the bound; worst at {i}: err {err[i]:.3e} "
                             f"bound {bound[i]:.3e} ref {ref[i]:.6e}")
    return True


# ===================================================================================================================
# 2. graphs
# ===================================================================================================================
DEGREES = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193]
DEGREE_ROWS = [10 + 7 * i for i in range(len(DEGREES))]
EMPTY_ROWS = [0, 50, 51, 170, 299]
HUB_ROW, HUB = 200, 9000


@functools.lru_cache(maxsize=None)
def graph(name):
    """edge lists (CPU) with chosen row lengths; n = target rows, n_src = source rows"""
    if name == "main":
        n = 300
        rng = np.random.default_rng(20261018)
        indeg = rng.integers(0, 13, n)
        indeg[EMPTY_ROWS] = 0
        indeg[DEGREE_ROWS] = DEGREES
        indeg[HUB_ROW] = HUB
        dst = np.repeat(np.arange(n), indeg)
        e = dst.shape[0]
        src = rng.integers(0, n, e)
        loops = rng.choice(e, 60, replace=False)
        src[loops] = dst[loops]                                    # self loops
        same = np.nonzero(dst[1:] == dst[:-1])[0]
        dup = rng.choice(same, 60, replace=False)
        src[dup + 1] = src[dup]                                    # duplicate edges
        order = rng.permutation(e)                                 # shuffled original order: perm not monotone across rows
        ei = np.stack([src[order], dst[order]])
        assert np.array_equal(np.bincount(ei[1], minlength=n), indeg)
        return SimpleNamespace(n=n, n_src=n, ei=torch.from_numpy(ei))
    if name == "thin":                                             # nnz = 8 n - 1: the thin kernel for F = 64 / 128
        return SimpleNamespace(n=300, n_src=300, ei=random_graph(300, 8 * 300 - 1, seed=5)[0])
    if name == "dense":                                            # nnz = 8 n: the first size the wave-per-row kernel takes
        return SimpleNamespace(n=300, n_src=300, ei=random_graph(300, 8 * 300, seed=6, hub=70)[0])
    if name == "n1e0":
        return SimpleNamespace(n=1, n_src=1, ei=torch.zeros(2, 0, dtype=torch.int64))
    if name == "n1e5":
        return SimpleNamespace(n=1, n_src=1, ei=torch.zeros(2, 5, dtype=torch.int64))
    if name == "n64e0":
        return SimpleNamespace(n=64, n_src=64, ei=torch.zeros(2, 0, dtype=torch.int64))
    if name == "rect":                                             # a partitioned shard: local targets, global sources
        rng = np.random.default_rng(7)
        ei = np.stack([rng.integers(0, 200, 1500), rng.integers(0, 120, 1500)])
        return SimpleNamespace(n=120, n_src=200, ei=torch.from_numpy(ei))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def host_csr(name, by):
    g = graph(name)
    ei = g.ei.numpy()
    rp, pm = csr_np(ei[1 if by == "dst" else 0], g.n if by == "dst" else g.n_src)
    other = ei[0 if by == "dst" else 1][pm].astype(np.int32)
    return SimpleNamespace(rp=rp, pm=pm, ot=other, n_rows=len(rp) - 1, n_other=g.n_src if by == "dst" else g.n)


def test_main_graph_has_the_row_lengths_it_is_for():
    c, s = host_csr("main", "dst"), host_csr("main", "src")
    lens = np.diff(c.rp)
    assert [int(lens[r]) for r in DEGREE_ROWS] == DEGREES and int(lens[HUB_ROW]) == HUB
    assert all(lens[r] == 0 for r in EMPTY_ROWS) and EMPTY_ROWS[0] == 0 and EMPTY_ROWS[-1] == len(lens) - 1
    assert (np.diff(c.pm) < 0).any() and len(c.pm) >= 8 * 300 and len(c.pm) <= 16384
    ei = graph("main").ei.numpy()
    assert (ei[0] == ei[1]).sum() >= 60 and len(np.unique(ei.T, axis=0)) < ei.shape[1]
    assert len(host_csr("thin", "dst").pm) < 8 * 300 <= len(host_csr("dense", "dst").pm)
    assert np.diff(s.rp).max() > 64                              # the by-source order has its own long rows


# ===================================================================================================================
# 1b. the references against independent torch formulations (CPU)
# ===================================================================================================================
def _small_case(seed=3, n=60, e=500):
    ei, w = random_graph(n, e, seed=seed, hub=100)
    ei = ei.numpy()
    return n, e, ei, w.numpy().astype(np.float32), csr_np(ei[1], n), csr_np(ei[0], n)


def test_reference_sums_match_index_add():
    n, e, ei, w, (rp, pm), _ = _small_case()
    rng = np.random.default_rng(0)
    m = rng.standard_normal((e, 11)).astype(np.float32)
    out0 = rng.standard_normal((n, 4)).astype(np.float32)
    dst = torch.from_numpy(ei[1])
    lens = np.diff(rp)
    for col_off, prior in ((0, None), (7, out0), (3, None)):
        got, s = ref_segment_sum(rp, pm, m, col_off, 4, prior)
        t = torch.from_numpy(m[:, col_off:col_off + 4]).double()
        ref = torch.zeros(n, 4, dtype=torch.float64).index_add_(0, dst, t)
        rs = torch.zeros(n, 4, dtype=torch.float64).index_add_(0, dst, t.abs())
        if prior is not None:
            ref, rs = ref + torch.from_numpy(prior).double(), rs + torch.from_numpy(prior).double().abs()
        tol = (lens[:, None] + 8) * 2.0 ** -52 * rs.numpy()                  # two float64 summation orders
        assert (np.abs(got - ref.numpy()) <= tol).all() and (np.abs(s - rs.numpy()) <= tol).all()
    x = rng.standard_normal((n, 5)).astype(np.float32)
    xe = rng.standard_normal((e, 5)).astype(np.float32)
    bias = rng.standard_normal(5).astype(np.float32)
    prior = rng.standard_normal((n, 5)).astype(np.float32)
    other = ei[0][pm]
    row_of = torch.from_numpy(np.repeat(np.arange(n), lens))
    for idx, val, b, p0 in ((other, w[pm], bias, prior), (other, None, None, None), (None, w[pm], bias, None),
                            (None, None, None, prior)):
        got, s = ref_spmm(rp, idx, val, x if idx is not None else xe, b, p0)
        rows = torch.from_numpy(x[idx] if idx is not None else xe).double()
        if val is not None:
            rows = rows * torch.from_numpy(val).double()[:, None]
        ref = torch.zeros(n, 5, dtype=torch.float64).index_add_(0, row_of, rows)
        rs = torch.zeros(n, 5, dtype=torch.float64).index_add_(0, row_of, rows.abs())
        for extra in (b, p0):
            if extra is not None:
                ref, rs = ref + torch.from_numpy(extra).double(), rs + torch.from_numpy(extra).double().abs()
        tol = (lens[:, None] + 8) * 2.0 ** -52 * rs.numpy()
        assert (np.abs(got - ref.numpy()) <= tol).all() and (np.abs(s - rs.numpy()) <= tol).all()


def test_reference_max_matches_scatter_reduce_and_a_first_index_search():
    n, e, ei, _, (rp, pm), _ = _small_case(seed=4)
    rng = np.random.default_rng(1)
    dst = torch.from_numpy(ei[1])
    for m in (rng.standard_normal((e, 6)).astype(np.float32),
              rng.integers(-2, 3, (e, 6)).astype(np.float32)):                # the second: ties in most rows
        out, arg = ref_segment_max(rp, pm, m)
        mt = torch.from_numpy(m)
        index = dst[:, None].expand(e, 6)
        amax = torch.zeros(n, 6).scatter_reduce(0, index, mt, "amax", include_self=False)
        cand = torch.where(mt == amax[dst], torch.arange(e)[:, None].expand(e, 6), torch.full((e, 6), e))
        first = torch.full((n, 6), e).scatter_reduce(0, index, cand, "amin", include_self=False)
        empty = torch.from_numpy(np.diff(rp) == 0)
        first[empty] = -1
        assert torch.equal(torch.from_numpy(out), amax) and np.array_equal(arg, first.numpy().astype(np.int32))
        assert (out[empty.numpy()] == 0).all()


def test_reference_max_special_values_by_hand():
    """rows (stored order, original ids): [2, 0, 1] | [] | [4, 3] | [5, 6, 7]"""
    nan_a, nan_b = np.array([0x7FC00001, 0x7FC00002], dtype=np.uint32).view(np.float32)
    inf = np.float32(np.inf)
    rp, pm = np.array([0, 3, 3, 5, 8]), np.array([2, 0, 1, 4, 3, 5, 6, 7], dtype=np.int32)
    #             id:   0      1      2      3      4      5      6      7
    m = np.array([[1.0, -inf, 0.0, nan_a, 2.0],          # 0
                  [3.0, -inf, -0.0, 1.0, 2.0],           # 1
                  [3.0, -inf, -0.0, 5.0, 2.0],           # 2
                  [-1.0, 7.0, 0.0, 0.0, nan_b],          # 3
                  [-1.0, inf, -0.0, 0.0, nan_a],         # 4
                  [-inf, 1.0, 0.0, nan_b, 0.0],          # 5
                  [-inf, inf, 0.0, nan_a, 0.0],          # 6
                  [-inf, inf, 0.0, 9.0, nan_a]], dtype=np.float32)
    out, arg = ref_segment_max(rp, pm, m)
    want_arg = np.array([[2, 2, 2, 0, 2], [-1] * 5, [4, 4, 4, 4, 4], [5, 6, 5, 5, 7]], dtype=np.int32)
    want = np.array([[3.0, -inf, -0.0, nan_a, 2.0], [0.0] * 5, [-1.0, inf, -0.0, 0.0, nan_a],
                     [-inf, inf, 0.0, nan_b, nan_a]], dtype=np.float32)
    assert np.array_equal(arg, want_arg) and np.array_equal(bits(out), bits(want))
    assert bits(out)[0, 3] == 0x7FC00001 and bits(out)[3, 3] == 0x7FC00002        # the first NaN's payload, untouched


def test_reference_backward_rules_match_float64_autograd():
    n, e, ei, w, (rp_d, pm_d), (rp_s, pm_s) = _small_case(seed=5)
    rng = np.random.default_rng(2)
    src, dst = torch.from_numpy(ei[0]), torch.from_numpy(ei[1])
    d = 3
    # segment_max: the gradient goes to the arg-max entry (tie-free input)
    m = rng.standard_normal((e, 4)).astype(np.float32)
    g = rng.standard_normal((n, 4)).astype(np.float32)
    _, arg = ref_segment_max(rp_d, pm_d, m)
    mt = torch.from_numpy(m).double().requires_grad_(True)
    out = torch.zeros(n, 4, dtype=torch.float64).scatter_reduce(0, dst[:, None].expand(e, 4), mt, "amax", include_self=False)
    out.backward(torch.from_numpy(g).double())
    assert torch.equal(mt.grad, torch.from_numpy(ref_segment_max_bwd(g, arg, e)).double())
    # edge_gather_concat: dL/dz = by-source sum of g[:, :D], then the by-target sum of g[:, D:2D] accumulated onto it
    z = torch.from_numpy(rng.standard_normal((n, d))).requires_grad_(True)
    extra = torch.from_numpy(w).double()
    gc = rng.standard_normal((e, 2 * d + 1))
    torch.cat([z[src], z[dst], extra[:, None]], 1).backward(torch.from_numpy(gc))
    first, _ = ref_segment_sum(rp_s, pm_s, gc, 0, d)
    both, _ = ref_segment_sum(rp_d, pm_d, gc, d, d, out0=first)
    assert np.allclose(both, z.grad.numpy(), rtol=0, atol=e * 2.0 ** -52 * np.abs(gc).sum())      # two float64 orders
    # edge_pair_add: dL/dp by source, dL/dq by target, dL/dcvec = extra^T g
    p = torch.from_numpy(rng.standard_normal((n, d))).requires_grad_(True)
    q = torch.from_numpy(rng.standard_normal((n, d))).requires_grad_(True)
    cv = torch.from_numpy(rng.standard_normal(d)).requires_grad_(True)
    gh = rng.standard_normal((e, d))
    (p[src] + q[dst] + extra[:, None] * cv).backward(torch.from_numpy(gh))
    tol = e * 2.0 ** -52 * np.abs(gh).sum() * float(extra.abs().max())
    assert np.allclose(ref_segment_sum(rp_s, pm_s, gh, 0, d)[0], p.grad.numpy(), rtol=0, atol=tol)
    assert np.allclose(ref_segment_sum(rp_d, pm_d, gh, 0, d)[0], q.grad.numpy(), rtol=0, atol=tol)
    assert np.allclose(extra.numpy() @ gh, cv.grad.numpy(), rtol=0, atol=tol)
    # segment_sum: its backward is the gather g[dst]
    ms = torch.from_numpy(rng.standard_normal((e, d))).requires_grad_(True)
    gn = rng.standard_normal((n, d))
    torch.zeros(n, d, dtype=torch.float64).index_add_(0, dst, ms).backward(torch.from_numpy(gn))
    assert np.array_equal(ref_gather_concat(gn, ei, 0, e)[:, d:], ms.grad.numpy())
    # the indexing references against torch indexing
    zf = rng.standard_normal((n, d)).astype(np.float32)
    assert np.array_equal(ref_gather_concat(zf, ei, 7, 100, w),
                          torch.cat([torch.from_numpy(zf)[src[7:107]], torch.from_numpy(zf)[dst[7:107]],
                                     torch.from_numpy(w)[7:107, None]], 1).numpy())
    pf, qf = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)
    assert np.array_equal(ref_pair_add(pf, qf, ei, 5, 50), (torch.from_numpy(pf)[src[5:55]] + torch.from_numpy(qf)[dst[5:55]]).numpy())
    cf = rng.standard_normal(d).astype(np.float32)
    ab = pf[ei[0, :50]].astype(np.float64) + qf[ei[1, :50]]
    exact = ab + w[:50, None].astype(np.float64) * cf
    # two roundings: the fp32 sum a + b, then the fused multiply-add
    assert (np.abs(ref_pair_add(pf, qf, ei, 0, 50, w, cf) - exact) <= 2 * U * (np.abs(ab) + np.abs(exact))).all()
    assert np.array_equal(ref_permute(w, pm_s), torch.from_numpy(w)[torch.from_numpy(pm_s).long()].numpy())


def test_propagate_error_paths():
    import pangnn_amd
    with pytest.raises(ValueError):
        pangnn_amd.MessagePassing(aggr="mean")
    with pytest.raises(ValueError):
        pangnn_amd.MessagePassing(flow="target_to_source")
    with pytest.raises(ValueError):
        pangnn_amd.MessagePassing(aggr="sum").propagate(torch.zeros(2, 3, dtype=torch.int64), pos=torch.zeros(4, 2))
    assert pangnn_amd.MessagePassing(aggr="sum").aggr == "add"


# ===================================================================================================================
# GPU side: helpers
# ===================================================================================================================
def dev():
    return torch.device("cuda:0")


def _abi():
    from pangnn_amd import _lib
    return _lib, _lib.load()


def up(a):
    return torch.from_numpy(np.array(a, order="C")).to(dev())


class View:
    """a [rows, width] window with leading dimension ld, `off` floats into a sentinel-filled buffer"""

    def __init__(self, rows, width, ld=None, off=0, dtype=torch.float32, fill=SENT):
        self.rows, self.width, self.ld, self.off = rows, width, ld or width, off
        self.buf = torch.full((rows * self.ld + off,), fill, dtype=dtype, device=dev())
        self.v = self.of(self.buf)

    def of(self, buf):
        return buf[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)[:, :self.width]

    def put(self, a):
        self.v.copy_(torch.from_numpy(np.array(a, order="C")))
        self.before = self.buf.clone()
        return self

    def get(self):
        return self.v.cpu().contiguous().numpy()

    def only_window_written(self):
        """every element of the buffer outside the window has the bits it had after put()"""
        want = self.before.clone()
        self.of(want).copy_(self.v)
        i = torch.int32
        return torch.equal(want.view(i), self.buf.view(i))

    @property
    def ptr(self):
        return self.v.data_ptr() if self.rows else self.buf.data_ptr()


_STRUCT = {}


def structure(name):
    """(EdgeStructure on the device, {"dst" / "src": its CSR tables, device and host}); the tables are what a stable sort gives"""
    if name not in _STRUCT:
        from pangnn_amd.graph import EdgeStructure
        g = graph(name)
        st = EdgeStructure(g.ei.to(dev()), g.n, None if g.n_src == g.n else g.n_src)
        csr = {}
        for by, c in (("dst", st.by_dst), ("src", st.by_src)):
            h = host_csr(name, by)
            assert np.array_equal(c.rowptr.cpu().numpy(), h.rp) and np.array_equal(c.perm.cpu().numpy(), h.pm)
            assert np.array_equal(c.other.cpu().numpy(), h.ot)
            csr[by] = SimpleNamespace(rowptr=c.rowptr, perm=c.perm, other=c.other, rp=h.rp, pm=h.pm, ot=h.ot,
                                      n_rows=h.n_rows, n_other=h.n_other)
        _STRUCT[name] = (st, csr)
    return _STRUCT[name]


def p_or_null(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


# ===================================================================================================================
# 3. pangnn_spmm_csr_f32 / pangnn_segment_sum_rows_f32
# ===================================================================================================================
def run_spmm(c, f, x, val, bias, out0, ldx=None, ldo=None, out_off=0, acc=0, use_idx=True, nnz=None):
    """one call on fresh buffers -> (result [n_rows, f], the out View)"""
    _lib, lib = _abi()
    xv = View(x.shape[0], f, ldx).put(x)
    ov = View(c.n_rows, f, ldo, out_off).put(out0)
    vt, bt = (None if val is None else up(val)), (None if bias is None else up(bias))
    rc = lib.pangnn_spmm_csr_f32(c.rowptr.data_ptr(), p_or_null(c.other) if use_idx else None, p_or_null(vt), xv.ptr,
                                 xv.ld, x.shape[0], p_or_null(bt), ov.ptr, ov.ld, c.n_rows,
                                 len(c.pm) if nnz is None else nnz, f, int(acc), _lib.stream_ptr())
    _lib.check(rc, "pangnn_spmm_csr_f32")
    torch.cuda.synchronize()
    return ov.get(), ov


def spmm_inputs(c, f, use_idx, use_val, bias, seed):
    rng = np.random.default_rng([seed, f, len(c.pm)])
    e = len(c.pm)
    x = rng.standard_normal((c.n_other if use_idx else max(e, 1), f)).astype(np.float32)
    val = rng.uniform(-2, 2, e).astype(np.float32) if use_val else None
    b = rng.standard_normal(f).astype(np.float32) if bias else None
    out0 = rng.standard_normal((c.n_rows, f)).astype(np.float32)
    return x, val, b, out0


def check_empty_rows(got, lens, bias, out0, acc):
    want = np.zeros_like(got)
    if bias is not None:
        want = want + bias[None, :]
    if acc:
        want = (want + out0).astype(np.float32)              # one fp32 addition: exact expectation
    empty = lens == 0
    return np.array_equal(bits(got[empty]), bits(want.astype(np.float32)[empty]))


def spmm_case(gname, f, by="dst", ldx=None, ldo=None, out_off=0, acc=0, bias=0, idx=1, val=1, nnz=None, same_as_tight=False):
    _, csr = structure(gname)
    c = csr[by]
    x, v, b, out0 = spmm_inputs(c, f, idx, val, bias, seed=11)
    kw = dict(ldx=ldx, ldo=ldo, out_off=out_off, acc=acc, use_idx=bool(idx), nnz=nnz)
    got, ov = run_spmm(c, f, x, v, b, out0, **kw)
    ref, s = ref_spmm(c.rp, c.ot if idx else None, v, x, b, out0 if acc else None)
    lens = np.diff(c.rp)
    assert within_sum_bound(got, ref, s, lens, f"spmm {gname} F={f}")
    assert check_empty_rows(got, lens, b, out0, acc)
    assert ov.only_window_written()
    again, _ = run_spmm(c, f, x, v, b, out0, **kw)
    assert np.array_equal(bits(got), bits(again))                                      # reproducible
    if same_as_tight:                                                                  # same kernel, same order
        tight, _ = run_spmm(c, f, x, v, b, out0, acc=acc, use_idx=bool(idx), nnz=nnz)
        assert np.array_equal(bits(got), bits(tight))


VEC_F = [16, 32, 64, 128, 256]
GEN_F = [1, 3, 20, 63, 65, 130, 257]
SPMM_CASES = []


def _case(name, **kw):
    SPMM_CASES.append(pytest.param(kw, id=name))


for _f in VEC_F:
    for _acc, _bias in ((0, 0), (1, 1), (0, 1), (1, 0)):
        _case(f"row<{_f}>-main-acc{_acc}-bias{_bias}", gname="main", f=_f, acc=_acc, bias=_bias)
    _case(f"row<{_f}>-main-bysrc-acc1", gname="main", f=_f, by="src", acc=1)
    _case(f"row<{_f}>-wide-ldx=F+4-ldo=F+8-acc1-bias1", gname="main", f=_f, ldx=_f + 4, ldo=_f + 8, acc=1, bias=1,
          same_as_tight=True)
    _case(f"generic-F{_f}-ldx=F+1-acc1-bias1", gname="main", f=_f, ldx=_f + 1, acc=1, bias=1)
    _case(f"generic-F{_f}-out+1float-acc1-bias1", gname="main", f=_f, out_off=1, acc=1, bias=1)
    _case(f"row<{_f}>-idxNULL-acc1", gname="main", f=_f, idx=0, acc=1)
    _case(f"row<{_f}>-valNULL-bias1", gname="main", f=_f, val=0, bias=1)
    _case(f"row<{_f}>-idxNULL-valNULL", gname="main", f=_f, idx=0, val=0)
for _f in GEN_F:
    _case(f"generic-F{_f}-main-acc0-bias0", gname="main", f=_f)
    _case(f"generic-F{_f}-main-acc1-bias1", gname="main", f=_f, acc=1, bias=1)
    _case(f"generic-F{_f}-wide-ldx=F+4-ldo=F+8-acc1", gname="main", f=_f, ldx=_f + 4, ldo=_f + 8, acc=1, same_as_tight=True)
for _f in (3, 65):
    _case(f"generic-F{_f}-idxNULL-acc1", gname="main", f=_f, idx=0, acc=1)
    _case(f"generic-F{_f}-valNULL-bias1", gname="main", f=_f, val=0, bias=1)
    _case(f"generic-F{_f}-idxNULL-valNULL", gname="main", f=_f, idx=0, val=0)
for _f in (64, 128):
    for _acc, _bias in ((0, 0), (1, 1), (0, 1), (1, 0)):
        _case(f"thin<{_f}>-thin-acc{_acc}-bias{_bias}", gname="thin", f=_f, acc=_acc, bias=_bias)
    _case(f"thin<{_f}>-wide-ldx=F+4-ldo=F+8-acc1-bias1", gname="thin", f=_f, ldx=_f + 4, ldo=_f + 8, acc=1, bias=1,
          same_as_tight=True)
    _case(f"thin<{_f}>-idxNULL-acc1", gname="thin", f=_f, idx=0, acc=1)
    _case(f"thin<{_f}>-valNULL-bias1", gname="thin", f=_f, val=0, bias=1)
    _case(f"thin<{_f}>-idxNULL-valNULL", gname="thin", f=_f, idx=0, val=0)
    _case(f"row<{_f}>-thin-nnz=-1-acc1-bias1", gname="thin", f=_f, nnz=-1, acc=1, bias=1)
    _case(f"row<{_f}>-dense-nnz=8n-acc1-bias1", gname="dense", f=_f, acc=1, bias=1)
for _g in ("n1e0", "n1e5", "n64e0"):
    for _f, _k in ((16, "row<16>"), (64, "thin<64>"), (3, "generic-F3")):
        _case(f"{_k}-{_g}-acc1-bias1", gname=_g, f=_f, acc=1, bias=1)
        _case(f"{_k}-{_g}-acc0-bias0", gname=_g, f=_f)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", SPMM_CASES)
def test_spmm_csr(kw):
    spmm_case(**kw)


def emulate_serial(rp, idx, x):
    """spmm_thin_kernel / spmm_row_generic_kernel with unit weights: fmaf(1, x, acc) = acc + x, entries in stored order"""
    out = np.zeros((len(rp) - 1, x.shape[1]), dtype=np.float32)
    for r in range(len(rp) - 1):
        acc = np.zeros(x.shape[1], dtype=np.float32)
        for k in range(rp[r], rp[r + 1]):
            acc = acc + x[idx[k]]
        out[r] = acc
    return out


def emulate_wave_per_row(rp, idx, x, unroll=4):
    """spmm_row_kernel<F, 4> with unit weights: 64-entry blocks, entry k of a step of EPS * U goes to partial row k % EPS
    (EPS = 256 / F), the EPS partial rows are combined by the xor tree 32 .. G"""
    f = x.shape[1]
    eps = 64 // (f // 4)
    out = np.zeros((len(rp) - 1, f), dtype=np.float32)
    for r in range(len(rp) - 1):
        part = np.zeros((eps, f), dtype=np.float32)
        for b0 in range(rp[r], rp[r + 1], 64):
            cnt = min(64, rp[r + 1] - b0)
            for s in range(0, cnt, eps * unroll):
                for u in range(unroll):
                    for sub in range(eps):
                        k = s + u * eps + sub
                        if k < cnt:
                            part[sub] = part[sub] + x[idx[b0 + k]]
        d = eps // 2
        while d >= 1:
            part = part + part[np.arange(eps) ^ d]
            d //= 2
        out[r] = part[0]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("f", [64, 128])
def test_spmm_nnz_hint_selects_the_kernel(f):
    """The nnz hint is the only thing that tells the thin kernel from the wave-per-row kernel, and the only way to see
    which one ran is its order of additions.  With unit weights every fmaf is a plain fp32 addition, so both orders can be
    replayed exactly on the host: nnz = 8 n - 1 must give the serial order (thin), nnz = -1 on the same input and
    nnz = 8 n on the dense graph must give the wave-per-row order."""
    _, csr = structure("thin")
    c = csr["dst"]
    x, _, _, out0 = spmm_inputs(c, f, 1, 0, 0, seed=12)
    serial, tree = emulate_serial(c.rp, c.ot, x), emulate_wave_per_row(c.rp, c.ot, x)
    assert not np.array_equal(bits(serial), bits(tree))                     # the input tells the two apart
    hinted, _ = run_spmm(c, f, x, None, None, out0)
    unhinted, _ = run_spmm(c, f, x, None, None, out0, nnz=-1)
    assert np.array_equal(bits(hinted), bits(serial))
    assert np.array_equal(bits(unhinted), bits(tree))
    _, csr = structure("dense")
    c = csr["dst"]
    x, _, _, out0 = spmm_inputs(c, f, 1, 0, 0, seed=13)
    got, _ = run_spmm(c, f, x, None, None, out0)
    assert np.array_equal(bits(got), bits(emulate_wave_per_row(c.rp, c.ot, x)))


def run_segment_sum(c, m, ldm, col_off, f, out0, acc, ldo=None):
    _lib, lib = _abi()
    mv = View(m.shape[0], m.shape[1], ldm).put(m)
    ov = View(c.n_rows, f, ldo).put(out0)
    rc = lib.pangnn_segment_sum_rows_f32(c.rowptr.data_ptr(), p_or_null(c.perm), mv.ptr, mv.ld, m.shape[0], col_off, ov.ptr,
                                         ov.ld, c.n_rows, f, int(acc), _lib.stream_ptr())
    _lib.check(rc, "pangnn_segment_sum_rows_f32")
    torch.cuda.synchronize()
    return ov.get(), ov


SEGSUM_CASES = []
for _g, _f, _k in (("main", 16, "row<16>"), ("main", 32, "row<32>"), ("main", 64, "row<64>"), ("thin", 64, "thin<64>"), ("thin", 128, "thin<128>"),
                   ("dense", 128, "row<128>"), ("main", 256, "row<256>")):
    for _w, _kk in ((2 * _f, _k), (2 * _f + 1, f"generic-F{_f}")):
        for _off in (0, 4, _f):
            SEGSUM_CASES.append(pytest.param(_g, _f, _w, _off, id=f"{_kk}-{_g}-w={'2F' if _w == 2 * _f else '2F+1'}-col_off={_off}"))
for _f in (3, 5):
    for _w in (2 * _f, 2 * _f + 1):
        for _off in (0, _f):
            SEGSUM_CASES.append(pytest.param("main", _f, _w, _off, id=f"generic-F{_f}-main-w={_w}-col_off={_off}"))
for _g in ("n1e0", "n1e5", "n64e0"):
    SEGSUM_CASES.append(pytest.param(_g, 64, 128, 64, id=f"thin<64>-{_g}-w=2F-col_off=64"))
    SEGSUM_CASES.append(pytest.param(_g, 3, 7, 3, id=f"generic-F3-{_g}-w=7-col_off=3"))


@pytest.mark.gpu
@pytest.mark.parametrize("gname,f,width,col_off", SEGSUM_CASES)
def test_segment_sum_rows(gname, f, width, col_off):
    """the two message shapes edge_gather_concat's backward produces, [E, 2F] and [E, 2F + 1]; col_off = F accumulates
    (accumulate = 1) as that backward's second call does, on both CSR orders"""
    _, csr = structure(gname)
    for by in ("dst", "src"):
        c = csr[by]
        rng = np.random.default_rng([21, f, width, col_off])
        m = rng.standard_normal((len(c.pm), width)).astype(np.float32)
        out0 = rng.standard_normal((c.n_rows, f)).astype(np.float32)
        acc = int(col_off == f)
        got, ov = run_segment_sum(c, m, width, col_off, f, out0, acc)
        ref, s = ref_segment_sum(c.rp, c.pm, m, col_off, f, out0 if acc else None)
        lens = np.diff(c.rp)
        assert within_sum_bound(got, ref, s, lens, f"segment_sum {gname}/{by}")
        assert check_empty_rows(got, lens, None, out0, acc)
        again, _ = run_segment_sum(c, m, width, col_off, f, out0, acc)
        assert np.array_equal(bits(got), bits(again))
        wide, wv = run_segment_sum(c, m, width, col_off, f, out0, acc, ldo=f + 8)
        assert wv.only_window_written()
        assert np.array_equal(bits(got), bits(wide))          # ldo does not change the kernel here: same order


@pytest.mark.gpu
def test_segment_sum_rows_rejects_a_window_outside_the_matrix():
    _lib, lib = _abi()
    _, csr = structure("main")
    c = csr["dst"]
    m, out = View(len(c.pm), 6).put(np.zeros((len(c.pm), 6), np.float32)), View(c.n_rows, 3).put(np.zeros((c.n_rows, 3), np.float32))
    rc = lib.pangnn_segment_sum_rows_f32(c.rowptr.data_ptr(), c.perm.data_ptr(), m.ptr, 6, len(c.pm), 4, out.ptr, 3,
                                         c.n_rows, 3, 0, _lib.stream_ptr())
    assert rc == -1 and b"column window" in lib.pangnn_last_error()
    assert out.only_window_written() and (out.get() == 0).all()


# ===================================================================================================================
# 4. segment_max
# ===================================================================================================================
NAN_PAYLOADS = np.array([0x7FC00001, 0x7FC00002, 0x7FC00003, 0x7FC00004, 0x7FC00005], dtype=np.uint32).view(np.float32)
MAX_KINDS = ["random", "ties", "zeros", "neginf", "posinf", "nan"]


@functools.lru_cache(maxsize=None)
def max_input(gname, by, kind):
    """(m [E, F_MAX] float32, reference out, reference arg) for one graph, CSR order and kind of values"""
    h = host_csr(gname, by)
    e = len(h.pm)
    rng = np.random.default_rng([31, MAX_KINDS.index(kind), e])
    m = rng.standard_normal((e, F_MAX)).astype(np.float32)
    if kind == "ties":                                         # a handful of values: most rows have several maxima
        m = rng.choice(np.array([-1.0, 0.0, 0.5, 2.0], dtype=np.float32), (e, F_MAX))
    elif kind == "zeros":                                      # +0.0 / -0.0 ties above a negative floor
        m = rng.choice(np.array([-1.0, -0.0, 0.0, -0.0, 0.0], dtype=np.float32), (e, F_MAX))
    elif kind == "neginf":                                     # even columns: every row is all -inf; odd: some -inf
        m[:, 0::2] = -np.inf
        m[rng.random((e, F_MAX)) < 0.3] = -np.inf
    elif kind == "posinf":
        m[rng.random((e, F_MAX)) < 0.05] = np.inf
        m[rng.random((e, F_MAX)) < 0.05] = -np.inf
    elif kind == "nan":                                        # odd columns: NaNs anywhere; every column: the four rows below
        odd = rng.random((e, F_MAX)) < 0.004
        odd[:, 0::2] = False
        m[odd] = np.nan
        rows = [r for r in range(h.n_rows) if h.rp[r + 1] - h.rp[r] >= 5][:4]
        for j, r in enumerate(rows):
            b, end = int(h.rp[r]), int(h.rp[r + 1])
            if j == 0:
                m[h.pm[b]] = NAN_PAYLOADS[0]                   # first entry of the row
            elif j == 1:
                m[h.pm[b + (end - b) // 2]] = NAN_PAYLOADS[1]  # a middle entry
            elif j == 2:
                m[h.pm[end - 1]] = NAN_PAYLOADS[2]             # the last entry
            else:
                m[h.pm[b + 1]] = NAN_PAYLOADS[3]               # two in one row: the first one's payload and id win
                m[h.pm[end - 2]] = NAN_PAYLOADS[4]
    m = np.ascontiguousarray(m, dtype=np.float32)
    out, arg = ref_segment_max(h.rp, h.pm, m)
    for a in (m, out, arg):
        a.setflags(write=False)
    return m, out, arg


def run_segment_max(c, m, ldm=None, ldo=None, with_arg=True):
    _lib, lib = _abi()
    f = m.shape[1]
    mv = View(m.shape[0], f, ldm).put(m)
    ov = View(c.n_rows, f, ldo).put(np.full((c.n_rows, f), SENT, np.float32))
    av = View(c.n_rows, f, ldo, dtype=torch.int32, fill=-7).put(np.full((c.n_rows, f), -7, np.int32))
    rc = lib.pangnn_segment_max_rows_f32(c.rowptr.data_ptr(), p_or_null(c.perm), mv.ptr, mv.ld, ov.ptr,
                                         av.ptr if with_arg else None, ov.ld, c.n_rows, f, _lib.stream_ptr())
    _lib.check(rc, "pangnn_segment_max_rows_f32")
    torch.cuda.synchronize()
    return ov, av


@pytest.mark.gpu
@pytest.mark.parametrize("by", ["dst", "src"])
@pytest.mark.parametrize("kind", MAX_KINDS)
@pytest.mark.parametrize("f", [1, 8, 63, 64, 65, 130])
def test_segment_max_forward(f, kind, by):
    """first maximum in stored order (= ascending original edge id, both CSR orders of the shuffled list), NaN propagates
    with the first NaN's id, an all -inf row is -inf with its first edge, empty rows are 0 / -1: out and arg bit for bit"""
    _, csr = structure("main")
    m, out, arg = max_input("main", by, kind)
    ov, av = run_segment_max(csr[by], m[:, :f])
    assert np.array_equal(bits(ov.get()), bits(out[:, :f]))
    assert np.array_equal(av.get(), arg[:, :f])
    if kind == "ties":                                         # "first" means the smallest original edge id among the maxima
        c = csr[by]
        r = int(np.argmax(np.diff(c.rp)))
        ids = c.pm[c.rp[r]:c.rp[r + 1]]
        for col in range(min(f, 4)):
            assert av.get()[r, col] == ids[m[ids, col] == m[ids, col].max()].min()
    if kind == "neginf":
        assert np.isneginf(ov.get()[np.diff(csr[by].rp) > 0][:, 0]).all() and (av.get()[np.diff(csr[by].rp) > 0][:, 0] >= 0).all()
    if kind == "nan":
        assert np.isnan(ov.get()[:, 0]).sum() >= 4


@pytest.mark.gpu
@pytest.mark.parametrize("gname", ["thin", "dense", "n1e0", "n1e5", "n64e0"])
@pytest.mark.parametrize("f", [1, 65])
def test_segment_max_forward_other_graphs(gname, f):
    _, csr = structure(gname)
    for kind in ("random", "ties", "nan"):
        m, out, arg = max_input(gname, "dst", kind)
        ov, av = run_segment_max(csr["dst"], m[:, :f])
        assert np.array_equal(bits(ov.get()), bits(out[:, :f])) and np.array_equal(av.get(), arg[:, :f])


@pytest.mark.gpu
@pytest.mark.parametrize("f", [8, 65])
def test_segment_max_leading_dimensions_and_null_arg(f):
    _, csr = structure("main")
    c = csr["dst"]
    m, out, arg = max_input("main", "dst", "ties")
    ov, av = run_segment_max(c, m[:, :f], ldm=f + 3, ldo=f + 5)
    assert np.array_equal(bits(ov.get()), bits(out[:, :f])) and np.array_equal(av.get(), arg[:, :f])
    assert ov.only_window_written() and av.only_window_written()
    ov, av = run_segment_max(c, m[:, :f], with_arg=False)
    assert np.array_equal(bits(ov.get()), bits(out[:, :f]))
    assert (av.get() == -7).all() and av.only_window_written()


def run_segment_max_bwd(c, g, arg, num_edges, ldm=None, ldo=None):
    _lib, lib = _abi()
    f = g.shape[1]
    gv = View(c.n_rows, f, ldo).put(g)
    av = View(c.n_rows, f, ldo, dtype=torch.int32, fill=-7).put(arg)
    mv = View(num_edges, f, ldm).put(np.zeros((num_edges, f), np.float32))
    rc = lib.pangnn_segment_max_bwd_f32(gv.ptr, av.ptr, c.rowptr.data_ptr(), mv.ptr, mv.ld, gv.ld, c.n_rows, f,
                                        _lib.stream_ptr())
    _lib.check(rc, "pangnn_segment_max_bwd_f32")
    torch.cuda.synchronize()
    return mv


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "ties", "nan"])
@pytest.mark.parametrize("f,ldm,ldo", [(1, None, None), (8, None, None), (65, None, None), (130, None, None), (8, 11, 13),
                                        (65, 68, 70)])
def test_segment_max_backward(f, ldm, ldo, kind):
    """gm[arg[r, f], f] = g[r, f]; every edge that won nothing keeps the 0 it was given"""
    _, csr = structure("main")
    c = csr["dst"]
    _, _, arg = max_input("main", "dst", kind)
    g = np.random.default_rng([41, f]).standard_normal((c.n_rows, f)).astype(np.float32)
    mv = run_segment_max_bwd(c, g, arg[:, :f], len(c.pm), ldm, ldo)
    want = ref_segment_max_bwd(g, arg[:, :f], len(c.pm))
    assert np.array_equal(bits(mv.get()), bits(want)) and mv.only_window_written()
    losers = np.ones(len(c.pm), bool)
    losers[arg[:, 0][arg[:, 0] >= 0]] = False
    assert losers.any() and (mv.get()[losers, 0] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("f", [8, 65])
def test_functional_segment_max_autograd(f):
    """functional.segment_max on tie-free input: forward as the reference, backward as float64 autograd of amax"""
    from pangnn_amd import functional as PF
    st, csr = structure("main")
    g = graph("main")
    m, out, arg = max_input("main", "dst", "random")
    e = m.shape[0]
    msg = up(m[:, :f]).requires_grad_(True)
    got = PF.segment_max(msg, st)
    assert np.array_equal(bits(got.detach().cpu().numpy()), bits(out[:, :f]))
    gsel = np.random.default_rng([42, f]).standard_normal((g.n, f)).astype(np.float32)
    got.backward(up(gsel))
    mt = torch.from_numpy(m[:, :f].copy()).double().requires_grad_(True)
    ref = torch.zeros(g.n, f, dtype=torch.float64).scatter_reduce(0, g.ei[1][:, None].expand(e, f), mt, "amax",
                                                                 include_self=False)
    ref.backward(torch.from_numpy(gsel).double())
    assert torch.equal(msg.grad.cpu().double(), mt.grad)
    assert np.array_equal(bits(msg.grad.cpu().numpy()), bits(ref_segment_max_bwd(gsel, arg[:, :f], e)))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ties", "nan"])
@pytest.mark.parametrize("f", [8, 65])
def test_dispatcher_segment_max_ops_return_the_ctypes_bits(f, kind):
    import pangnn_amd  # noqa: F401
    _, csr = structure("main")
    c = csr["dst"]
    m, out, arg = max_input("main", "dst", kind)
    ov, av = run_segment_max(c, m[:, :f])
    o, a = torch.ops.pangnn.segment_max_rows(c.rowptr, c.perm, up(m[:, :f]), c.n_rows)
    assert a.dtype == torch.int32
    assert np.array_equal(bits(o.cpu().numpy()), bits(ov.get())) and np.array_equal(a.cpu().numpy(), av.get())
    assert np.array_equal(bits(o.cpu().numpy()), bits(out[:, :f])) and np.array_equal(a.cpu().numpy(), arg[:, :f])
    g = np.random.default_rng([43, f]).standard_normal((c.n_rows, f)).astype(np.float32)
    gm = torch.ops.pangnn.segment_max_bwd(up(g), a, c.rowptr, len(c.pm))
    mv = run_segment_max_bwd(c, g, av.get(), len(c.pm))
    assert np.array_equal(bits(gm.cpu().numpy()), bits(mv.get()))
    assert np.array_equal(bits(gm.cpu().numpy()), bits(ref_segment_max_bwd(g, arg[:, :f], len(c.pm))))


# ===================================================================================================================
# 5. gathers, pair-add, permute
# ===================================================================================================================
def run_gather_concat(ei_dev, ld, z, ldz, e_begin, n_edges, extra, ldo):
    _lib, lib = _abi()
    d = z.shape[1]
    width = 2 * d + (extra is not None)
    zv = View(z.shape[0], d, ldz).put(z)
    ov = View(n_edges, width, ldo).put(np.full((n_edges, width), SENT, np.float32))
    ex = None if extra is None else up(extra)
    rc = lib.pangnn_edge_gather_concat_f32(zv.ptr, zv.ld, z.shape[0], ei_dev.data_ptr(), ld, e_begin, n_edges, p_or_null(ex),
                                           ov.ptr, ov.ld, d, _lib.stream_ptr())
    _lib.check(rc, "pangnn_edge_gather_concat_f32")
    torch.cuda.synchronize()
    return ov


GATHER_CASES = []
for _d in (1, 3, 4, 16, 64, 100, 128):
    _v = "vec" if _d % 4 == 0 else "scalar"
    GATHER_CASES += [
        pytest.param(_d, False, None, None, 0, None, id=f"{_v}-D{_d}-tight"),
        pytest.param(_d, True, None, None, 0, None, id=f"scalar-D{_d}-extra"),
        pytest.param(_d, False, _d + 1, None, 0, None, id=f"scalar-D{_d}-ldz=D+1"),
        pytest.param(_d, False, None, 2 * _d + 4, 777, 2048, id=f"{_v}-D{_d}-ldo=2D+4-e_begin=777-n=2048"),
        pytest.param(_d, True, _d + 4, 2 * _d + 7, 1, 1001, id=f"scalar-D{_d}-extra-ldz=D+4-ldo=2D+7-e_begin=1-n=1001"),
        pytest.param(_d, False, None, 2 * _d + 3, 5000, 300, id=f"scalar-D{_d}-ldo=2D+3-e_begin=5000-n=300"),
    ]


@pytest.mark.gpu
@pytest.mark.parametrize("d,with_extra,ldz,ldo,e_begin,n_edges", GATHER_CASES)
def test_gather_concat(d, with_extra, ldz, ldo, e_begin, n_edges):
    st, _ = structure("main")
    ei = graph("main").ei.numpy()
    e = ei.shape[1]
    n_edges = e if n_edges is None else n_edges
    rng = np.random.default_rng([51, d])
    z = rng.standard_normal((graph("main").n, d)).astype(np.float32)
    extra = rng.standard_normal(e).astype(np.float32) if with_extra else None
    ov = run_gather_concat(st.edge_index, e, z, ldz, e_begin, n_edges, extra, ldo)
    assert np.array_equal(bits(ov.get()), bits(ref_gather_concat(z, ei, e_begin, n_edges, extra)))
    assert ov.only_window_written()


def run_pair_add(ei_dev, ld, p, q, ldpq, e_begin, n_edges, extra, cvec, ldo=None, p_off=0):
    _lib, lib = _abi()
    d = p.shape[1]
    pv, qv = View(p.shape[0], d, ldpq, p_off).put(p), View(q.shape[0], d, ldpq).put(q)
    ov = View(n_edges, d, ldo).put(np.full((n_edges, d), SENT, np.float32))
    ex, cv = (None if extra is None else up(extra)), (None if cvec is None else up(cvec))
    rc = lib.pangnn_edge_pair_add_f32(pv.ptr, qv.ptr, pv.ld, max(p.shape[0], q.shape[0]), ei_dev.data_ptr(), ld, e_begin, n_edges,
                                      p_or_null(ex), p_or_null(cv), ov.ptr, ov.ld, d, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, ov


def within_one_ulp(got, want):
    return ((got >= np.nextafter(want, np.float32(-np.inf))) & (got <= np.nextafter(want, np.float32(np.inf)))).all()


@pytest.mark.gpu
@pytest.mark.parametrize("d", [4, 16, 64, 128])
@pytest.mark.parametrize("ldpq_pad,e_begin,n_edges,ldo_pad", [(0, 0, None, 0), (4, 333, 4097, 8)])
def test_pair_add(d, ldpq_pad, e_begin, n_edges, ldo_pad):
    _lib, _ = _abi()
    st, _ = structure("main")
    g = graph("main")
    ei = g.ei.numpy()
    e = ei.shape[1]
    n_edges = e if n_edges is None else n_edges
    rng = np.random.default_rng([52, d])
    p, q = rng.standard_normal((g.n, d)).astype(np.float32), rng.standard_normal((g.n, d)).astype(np.float32)
    extra, cvec = rng.standard_normal(e).astype(np.float32), rng.standard_normal(d).astype(np.float32)
    rc, ov = run_pair_add(st.edge_index, e, p, q, d + ldpq_pad, e_begin, n_edges, None, None, d + ldo_pad)
    _lib.check(rc)
    assert np.array_equal(bits(ov.get()), bits(ref_pair_add(p, q, ei, e_begin, n_edges))) and ov.only_window_written()
    rc, ov = run_pair_add(st.edge_index, e, p, q, d + ldpq_pad, e_begin, n_edges, extra, cvec, d + ldo_pad)
    _lib.check(rc)
    # 1 ulp: the float64 emulation of the fma rounds twice (ref_pair_add)
    assert within_one_ulp(ov.get(), ref_pair_add(p, q, ei, e_begin, n_edges, extra, cvec)) and ov.only_window_written()


@pytest.mark.gpu
def test_pair_add_error_codes():
    _, lib = _abi()
    st, _ = structure("main")
    g = graph("main")
    e = g.ei.shape[1]
    z6, z8 = np.zeros((g.n, 6), np.float32), np.zeros((g.n, 8), np.float32)
    rc, ov = run_pair_add(st.edge_index, e, z6, z6, 8, 0, e, None, None, 8)              # D % 4 != 0
    assert rc == -1 and b"multiples of 4" in lib.pangnn_last_error() and ov.only_window_written() and (ov.get() == SENT).all()
    rc, ov = run_pair_add(st.edge_index, e, z8, z8, 8, 0, e, None, None, 8, p_off=1)     # p one float off 16 bytes
    assert rc == -4 and b"16-byte aligned" in lib.pangnn_last_error() and (ov.get() == SENT).all()


def sum_bound_torch(got, ref, s, lengths, what=""):
    return within_sum_bound(got.detach().cpu().numpy(), ref.detach().numpy(), s.detach().numpy(), lengths, what)


@pytest.mark.gpu
def test_pair_add_rectangular_structure_forward_and_backward():
    """num_src != num_nodes (a partitioned shard): p has source rows, q target rows"""
    from pangnn_amd import functional as PF
    st, csr = structure("rect")
    g = graph("rect")
    src, dst = g.ei[0], g.ei[1]
    e, d = g.ei.shape[1], 16
    rng = np.random.default_rng(53)
    p, q = rng.standard_normal((g.n_src, d)).astype(np.float32), rng.standard_normal((g.n, d)).astype(np.float32)
    extra, cvec = rng.standard_normal(e).astype(np.float32), rng.standard_normal(d).astype(np.float32)
    gh = rng.standard_normal((e, d)).astype(np.float32)
    pt, qt, ct = (up(a).requires_grad_(True) for a in (p, q, cvec))
    out = PF.edge_pair_add(pt, qt, st, up(extra), ct)
    assert within_one_ulp(out.detach().cpu().numpy(), ref_pair_add(p, q, g.ei.numpy(), 0, e, extra, cvec))
    assert np.array_equal(bits(PF.edge_pair_add(pt, qt, st).detach().cpu().numpy()), bits(ref_pair_add(p, q, g.ei.numpy(), 0, e)))
    out.backward(up(gh))
    g64 = torch.from_numpy(gh).double()
    for got, key, n_rows, by in ((pt.grad, src, g.n_src, "src"), (qt.grad, dst, g.n, "dst")):
        ref = torch.zeros(n_rows, d, dtype=torch.float64).index_add_(0, key, g64)
        s = torch.zeros(n_rows, d, dtype=torch.float64).index_add_(0, key, g64.abs())
        assert got.shape == ref.shape and sum_bound_torch(got, ref, s, np.diff(csr[by].rp), f"rect d{by}")
    terms = torch.from_numpy(extra).double()[:, None] * g64
    assert sum_bound_torch(ct.grad[None], terms.sum(0)[None], terms.abs().sum(0)[None], [e], "rect dcvec")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 257, 100003])
def test_permute(n):
    _lib, lib = _abi()
    rng = np.random.default_rng([54, n])
    x, perm = rng.standard_normal(n).astype(np.float32), rng.integers(0, max(n, 1), n).astype(np.int32)
    xv, ov = View(1, n).put(x[None]), View(1, n + 3).put(np.full((1, n + 3), SENT, np.float32))
    pt = up(perm)
    _lib.check(lib.pangnn_permute_f32(p_or_null(xv.buf), p_or_null(pt), ov.ptr, n, _lib.stream_ptr()), "pangnn_permute_f32")
    torch.cuda.synchronize()
    assert np.array_equal(bits(ov.get()[0, :n]), bits(ref_permute(x, perm))) and (ov.get()[0, n:] == SENT).all()


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 64])
@pytest.mark.parametrize("with_extra", [False, True])
def test_edge_gather_concat_autograd(d, with_extra):
    """backward = segment_sum_rows over the by-source order, then over the by-target order with col_off = D and
    accumulate = 1: row<64> twice for D = 64, the generic kernel for D = 3 and for the odd [E, 2D + 1] gradient"""
    from pangnn_amd import functional as PF
    st, csr = structure("main")
    g = graph("main")
    src, dst = g.ei[0], g.ei[1]
    e = g.ei.shape[1]
    rng = np.random.default_rng([55, d])
    z = rng.standard_normal((g.n, d)).astype(np.float32)
    extra = rng.standard_normal(e).astype(np.float32) if with_extra else None
    gc = rng.standard_normal((e, 2 * d + with_extra)).astype(np.float32)
    zt = up(z).requires_grad_(True)
    out = PF.edge_gather_concat(zt, st, None if extra is None else up(extra))
    assert np.array_equal(bits(out.detach().cpu().numpy()), bits(ref_gather_concat(z, g.ei.numpy(), 0, e, extra)))
    out.backward(up(gc))
    z64 = torch.from_numpy(z).double().requires_grad_(True)
    parts = [z64[src], z64[dst]] + ([torch.from_numpy(extra).double()[:, None]] if with_extra else [])
    torch.cat(parts, 1).backward(torch.from_numpy(gc).double())
    a = torch.from_numpy(gc).double().abs()
    s = torch.zeros(g.n, d, dtype=torch.float64).index_add_(0, src, a[:, :d]).index_add_(0, dst, a[:, d:2 * d])
    lens = np.diff(csr["src"].rp) + np.diff(csr["dst"].rp)
    assert sum_bound_torch(zt.grad, z64.grad, s, lens, "dL/dz")


@pytest.mark.gpu
@pytest.mark.parametrize("d", [16, 64])
def test_edge_pair_add_autograd(d):
    from pangnn_amd import functional as PF
    st, csr = structure("main")
    g = graph("main")
    src, dst = g.ei[0], g.ei[1]
    e = g.ei.shape[1]
    rng = np.random.default_rng([56, d])
    p, q = rng.standard_normal((g.n, d)).astype(np.float32), rng.standard_normal((g.n, d)).astype(np.float32)
    extra, cvec = rng.standard_normal(e).astype(np.float32), rng.standard_normal(d).astype(np.float32)
    gh = rng.standard_normal((e, d)).astype(np.float32)
    pt, qt, ct = (up(a).requires_grad_(True) for a in (p, q, cvec))
    PF.edge_pair_add(pt, qt, st, up(extra), ct).backward(up(gh))
    p64, q64, c64 = (torch.from_numpy(a).double().requires_grad_(True) for a in (p, q, cvec))
    g64, x64 = torch.from_numpy(gh).double(), torch.from_numpy(extra).double()
    (p64[src] + q64[dst] + x64[:, None] * c64).backward(g64)
    for got, ref, key, by in ((pt.grad, p64.grad, src, "src"), (qt.grad, q64.grad, dst, "dst")):
        s = torch.zeros(g.n, d, dtype=torch.float64).index_add_(0, key, g64.abs())
        assert sum_bound_torch(got, ref, s, np.diff(csr[by].rp), f"dL/d{by}")
    assert sum_bound_torch(ct.grad[None], c64.grad[None], (x64[:, None] * g64).abs().sum(0)[None], [e], "dL/dcvec")


@pytest.mark.gpu
@pytest.mark.parametrize("f", [5, 64])
def test_segment_sum_autograd(f):
    from pangnn_amd import functional as PF
    st, csr = structure("main")
    g = graph("main")
    dst = g.ei[1]
    e = g.ei.shape[1]
    rng = np.random.default_rng([57, f])
    m, gn = rng.standard_normal((e, f)).astype(np.float32), rng.standard_normal((g.n, f)).astype(np.float32)
    mt = up(m).requires_grad_(True)
    out = PF.segment_sum(mt, st)
    ref, s = ref_segment_sum(csr["dst"].rp, csr["dst"].pm, m, 0, f)
    assert within_sum_bound(out.detach().cpu().numpy(), ref, s, np.diff(csr["dst"].rp), "segment_sum")
    out.backward(up(gn))
    assert np.array_equal(bits(mt.grad.cpu().numpy()), bits(gn[dst.numpy()]))          # a gather: exact


# ===================================================================================================================
# 6. MessagePassing.propagate
# ===================================================================================================================
CX, CP = 5, 4


def _lift_module(aggr):
    import pangnn_amd

    class Lift(pangnn_amd.MessagePassing):
        """lifts x AND a second node tensor of another width (the `base is not x` branch), plus a per-edge argument"""

        def __init__(self):
            super().__init__(aggr=aggr)
            gen = torch.Generator().manual_seed(61)
            self.tx = torch.nn.Parameter(torch.randn(CX, generator=gen))
            self.tp = torch.nn.Parameter(torch.randn(CP, generator=gen))

        def forward(self, x, pos, edge_index, w, size=None):
            return self.propagate(edge_index, size=size, x=x, pos=pos, w=w)

        def message(self, x_i, x_j, pos_i, pos_j, w):
            return w.view(-1, 1) * torch.cat([self.tx * (x_j - x_i), self.tp * (pos_j - pos_i)], dim=1)

    return Lift()


@pytest.mark.gpu
@pytest.mark.parametrize("aggr", ["sum", "add", "max"])
def test_propagate_lifts_two_node_tensors(aggr):
    """Forward and the gradients to x, pos and the module's parameters against the same module in float64 torch.
    A message element takes three fp32 roundings (difference, times parameter, times edge argument), its gradient terms
    two or three, so a sum of L of them stays within (L + 8) 2^-24 S like every other sum here; a maximum is within
    4 * 2^-24 of the largest |message| of its row ((1 + u)^3 - 1 < 4u).  For 'max' the test first checks on the float64
    messages that the two largest of every row are further apart than 8u times their size — then the fp32 kernel
    provably selects the same edge — except where both are exactly 0: self loops, whose messages carry no gradient to
    any leaf."""
    g = graph("main")
    n, e = g.n, g.ei.shape[1]
    src, dst = g.ei[0], g.ei[1]
    rng = np.random.default_rng(62)
    x, pos = rng.standard_normal((n, CX)).astype(np.float32), rng.standard_normal((n, CP)).astype(np.float32)
    w = rng.uniform(0.5, 2.0, e).astype(np.float32)
    gsel = rng.standard_normal((n, CX + CP)).astype(np.float32)
    mod = _lift_module(aggr).to(dev())
    assert mod.aggr == ("max" if aggr == "max" else "add")
    ei_dev = g.ei.to(dev())
    xt, pt = up(x).requires_grad_(True), up(pos).requires_grad_(True)
    out = mod(xt, pt, ei_dev, up(w))
    for size in (n, (n, n)):
        assert torch.equal(out, mod(xt, pt, ei_dev, up(w), size=size))
    out.backward(up(gsel))

    x64, p64 = (torch.from_numpy(a).double().requires_grad_(True) for a in (x, pos))
    tx, tp = (t.detach().cpu().double().requires_grad_(True) for t in (mod.tx, mod.tp))
    w64 = torch.from_numpy(w).double()
    diff = torch.cat([x64[src] - x64[dst], p64[src] - p64[dst]], 1)
    msg = w64[:, None] * (torch.cat([tx, tp]) * diff)
    msg.retain_grad()
    index = dst[:, None].expand(e, CX + CP)
    lens = np.diff(host_csr("main", "dst").rp)
    if aggr == "max":
        ref = torch.zeros(n, CX + CP, dtype=torch.float64).scatter_reduce(0, index, msg, "amax", include_self=False)
        biggest = torch.zeros(n, CX + CP, dtype=torch.float64).scatter_reduce(0, index, msg.detach().abs(), "amax",
                                                                            include_self=False)
        h = host_csr("main", "dst")
        md = msg.detach().numpy()
        for r in np.nonzero(lens >= 2)[0]:
            top = np.sort(md[h.pm[h.rp[r]:h.rp[r + 1]]], axis=0)[-2:]
            ok = (top[1] - top[0] > 8 * U * np.abs(top).max(0)) | ((top[0] == 0) & (top[1] == 0))
            assert ok.all(), f"row {r}: the input has a near tie, the arg-max is not determined in fp32"
        err = (out.detach().cpu().double() - ref.detach()).abs()
        assert bool((err <= 4 * U * biggest).all()), float((err - 4 * U * biggest).max())
        assert bool((out.detach().cpu()[lens == 0] == 0).all())
    else:
        ref = torch.zeros(n, CX + CP, dtype=torch.float64).index_add_(0, dst, msg)
        s = torch.zeros(n, CX + CP, dtype=torch.float64).index_add_(0, dst, msg.detach().abs())
        assert sum_bound_torch(out, ref, s, lens, "forward")
        assert bool((out.detach().cpu()[lens == 0] == 0).all())
    ref.backward(torch.from_numpy(gsel).double())
    term = (msg.grad * w64[:, None] * torch.cat([tx, tp]).detach()).abs()          # |d loss / d (difference)| per edge
    both = np.diff(host_csr("main", "src").rp) + lens
    for got, want, cols in ((xt.grad, x64.grad, slice(0, CX)), (pt.grad, p64.grad, slice(CX, CX + CP))):
        width = cols.stop - cols.start
        s = torch.zeros(n, width, dtype=torch.float64).index_add_(0, src, term[:, cols]).index_add_(0, dst, term[:, cols])
        assert sum_bound_torch(got, want, s, both, "node gradient")
    pterm = (msg.grad * w64[:, None] * diff.detach()).abs().sum(0)
    assert sum_bound_torch(mod.tx.grad[None], tx.grad[None], pterm[None, :CX], [e], "dL/dtx")
    assert sum_bound_torch(mod.tp.grad[None], tp.grad[None], pterm[None, CX:], [e], "dL/dtp")


@pytest.mark.gpu
def test_propagate_size_none_and_missing_arguments_on_device():
    g = graph("thin")
    mod = _lift_module("add").to(dev())
    ei = g.ei.to(dev())
    x, pos, w = torch.randn(g.n, CX, device=dev()), torch.randn(g.n, CP, device=dev()), torch.rand(g.ei.shape[1], device=dev())
    with pytest.raises(ValueError):
        mod.propagate(ei, pos=pos, w=w)
    assert torch.equal(mod.propagate(ei, x=x, pos=pos, w=w), mod.propagate(ei, size=(g.n, g.n), x=x, pos=pos, w=w))
