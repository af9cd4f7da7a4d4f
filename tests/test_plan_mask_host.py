"""The two entry points that take the torch plumbing out of a sub-sampled step, where there is no GPU: the argument checks
of pangnn_csr_plan and pangnn_mask_k_smallest_i64 (fake pointers, nothing launched), and the row-pointer formulas of the
plan kernel restated in plain torch against EdgeStructure._plan_of_sorted_keys — the definition itself, pinned on the row
layouts the GPU test (tests/test_csr_plan.py) runs the kernel on.  Every comparison is exact."""
import pytest
import torch

from pangnn_amd import _lib
from pangnn_amd.graph import EdgeStructure

SPANS = (32, 64, 512)


def edge_counts(span):
    return (1, span - 1, span, span + 1, 2 * span, 3 * span + 7, 70001)


def _fit(lens, e):
    """row lengths cut (or the last row stretched) to e entries in all"""
    lens = lens.clone()
    over = int(lens.sum()) - e
    i = lens.numel() - 1
    while over > 0:
        cut = min(over, int(lens[i]))
        lens[i] -= cut
        over -= cut
        i -= 1
    if over < 0:
        lens[-1] -= over
    return lens


def layouts(e, span, seed=0):
    """name -> rowptr int64 [n_rows + 1] with rowptr[-1] == e"""
    gen = torch.Generator().manual_seed(seed * 7919 + e + span)
    z = lambda k: torch.zeros(k, dtype=torch.int64)
    out = {"hub_alone": torch.tensor([e]), "hub_among_empty_rows": torch.cat([z(500), torch.tensor([e]), z(500)]),
           "one_entry_per_row": torch.ones(e, dtype=torch.int64),
           "rows_on_chunk_boundaries": _fit(torch.full(((e + span - 1) // span,), span, dtype=torch.int64), e)}
    some = _fit(torch.randint(0, 9, (max(1, e // 3),), generator=gen), e)
    half = some.numel() // 2
    out["empty_front_back_middle"] = torch.cat([z(37), some[:half], z(span + 5), some[half:], z(41)])
    # geometric lengths (mean 4, many empty rows) and, where they fit, a few rows above 8192 entries
    tail = torch.empty(max(1, e // 4), dtype=torch.float32).geometric_(0.2, generator=gen).long() - 1
    if e > 30000:
        tail[torch.tensor([3, tail.numel() // 2, tail.numel() - 2])] = torch.tensor([8193, 12000, 9001])
        tail = tail[torch.randperm(tail.numel(), generator=gen)]
    out["heavy_tailed"] = _fit(tail, e)
    res = {}
    for name, lens in out.items():
        assert int(lens.sum()) == e and int(lens.min()) >= 0, name
        res[name] = torch.cat([z(1), torch.cumsum(lens, 0)])
    return res


def keys_of(rowptr):
    n = rowptr.numel() - 1
    return torch.repeat_interleave(torch.arange(n, device=rowptr.device), rowptr[1:] - rowptr[:-1])


def plan_by_the_formulas(rowptr, span):
    """pangnn_csr_plan's contract (include/pangnn_hip.h) in index ops"""
    e = int(rowptr[-1])
    p = rowptr[:-1]
    c = ((rowptr[1:] > p) & (p % span != 0)).long()
    cin = torch.cumsum(c, 0)
    cex = torch.cat([cin - c, cin[-1:]])
    last = (e - 1) // span + int(cin[-1])
    row = lambda q: torch.searchsorted(rowptr, q, right=True) - 1      # the last row with rowptr[row] <= q
    keys = row(torch.arange(e)).to(torch.int32)
    q = torch.arange(0, e, span)
    part_off = (q // span + cin[row(q)]).to(torch.int32)
    part_rowptr = torch.where(rowptr < e, rowptr // span + cex + (rowptr % span != 0).long(), torch.tensor(last + 1))
    return keys, part_off, part_rowptr, torch.tensor([last])


@pytest.mark.parametrize("span", SPANS)
def test_the_rowptr_formulas_are_the_plan_of_the_sorted_keys(span):
    for e in edge_counts(span):
        for name, rowptr in layouts(e, span).items():
            n_rows = rowptr.numel() - 1
            want = EdgeStructure._plan_of_sorted_keys(keys_of(rowptr), n_rows, span // 32)
            keys, part_off, part_rowptr, last = plan_by_the_formulas(rowptr, span)
            what = (name, e, span)
            assert keys.dtype == want.keys.dtype and torch.equal(keys, want.keys), what
            assert part_off.dtype == want.part_off.dtype and torch.equal(part_off, want.part_off), what
            assert part_rowptr.dtype == want.part_rowptr.dtype and torch.equal(part_rowptr, want.part_rowptr), what
            assert last.dtype == want.last.dtype and torch.equal(last, want.last), what
            assert want.n_parts == (e + span - 1) // span + min(n_rows, e) >= int(last) + 1, what


def test_the_layouts_hold_what_they_are_named_for():
    lay = layouts(70001, 512)
    lens = {k: v[1:] - v[:-1] for k, v in lay.items()}
    assert int((lens["heavy_tailed"] > 8192).sum()) >= 3 and int((lens["heavy_tailed"] == 0).sum()) > 100
    assert lens["hub_among_empty_rows"].numel() == 1001 and int(lens["hub_among_empty_rows"][500]) == 70001
    assert bool((lay["rows_on_chunk_boundaries"][:-1] % 512 == 0).all())
    front = lens["empty_front_back_middle"]
    assert int(front[:37].sum()) == 0 and int(front[-41:].sum()) == 0 and int((front == 0).sum()) > 37 + 41 + 512


F = 0x7f0000100000
E_BADARG, E_TOOLARGE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -4
no_gpu = pytest.mark.skipif(torch.cuda.is_available(),
                            reason="fake device pointers: only where a missing check cannot reach a GPU")


def _plan_args(**over):
    a = dict(rowptr=F, n_rows=1000, num_edges=5000, span=512, keys=F, part_off=F, part_rowptr=F, last=F, workspace=F,
             workspace_bytes=1 << 30, stream=None)
    assert not set(over) - set(a)
    a.update(over)
    return list(a.values())


@no_gpu
def test_plan_entry_point_refuses_bad_arguments():
    lib = _lib.load()
    fn = lib.pangnn_csr_plan
    for name in ("rowptr", "keys", "part_off", "part_rowptr", "last", "workspace"):
        assert fn(*_plan_args(**{name: None})) == E_BADARG, name
    assert b"pangnn_csr_plan" in lib.pangnn_last_error()
    for over in (dict(num_edges=0), dict(num_edges=-1), dict(n_rows=0), dict(n_rows=-3)):
        assert fn(*_plan_args(**over)) == E_BADARG, over
    for span in (0, -32, 1, 31, 33, 48, 500):
        assert fn(*_plan_args(span=span)) == E_BADARG, span                   # not a positive multiple of 32
    assert b"multiple of 32" in lib.pangnn_last_error()
    big = 1 << 31
    assert fn(*_plan_args(num_edges=big)) == E_TOOLARGE and fn(*_plan_args(n_rows=big)) == E_TOOLARGE
    assert fn(*_plan_args(num_edges=big + 7, n_rows=big + 1)) == E_TOOLARGE
    assert lib.pangnn_csr_plan_workspace_bytes(0) == 0 and lib.pangnn_csr_plan_workspace_bytes(big) == 0
    assert fn(*_plan_args(workspace=F + 8)) == E_ALIGN and fn(*_plan_args(rowptr=F + 4)) == E_ALIGN
    assert fn(*_plan_args(keys=F + 2)) == E_ALIGN and fn(*_plan_args(last=F + 4)) == E_ALIGN
    # every argument plausible: the scan's temporary size comes from rocPRIM, whose query needs a device — without one the
    # call refuses to run; with one, a workspace one byte short is PANGNN_E_WORKSPACE
    need = lib.pangnn_csr_plan_workspace_bytes(1000)
    if need == 0:
        assert fn(*_plan_args()) == E_BADARG and b"size query" in lib.pangnn_last_error()
    else:
        assert fn(*_plan_args(workspace_bytes=need - 1)) == E_WORKSPACE and fn(*_plan_args(workspace_bytes=-1)) == E_WORKSPACE


def _mask_args(**over):
    a = dict(keys=F, n=5000, k=1000, keep=F, workspace=F, workspace_bytes=1 << 20, stream=None)
    assert not set(over) - set(a)
    a.update(over)
    return list(a.values())


@no_gpu
def test_mask_entry_point_refuses_bad_arguments():
    lib = _lib.load()
    fn = lib.pangnn_mask_k_smallest_i64
    for name in ("keys", "keep", "workspace"):
        assert fn(*_mask_args(**{name: None})) == E_BADARG, name
    assert b"pangnn_mask_k_smallest_i64" in lib.pangnn_last_error()
    for over in (dict(k=5001), dict(k=-1), dict(n=-1, k=0), dict(n=0, k=1)):
        assert fn(*_mask_args(**over)) == E_BADARG, over                      # k outside [0, n]
    big = 1 << 31
    assert fn(*_mask_args(n=big)) == E_TOOLARGE and fn(*_mask_args(n=big + 3, k=big + 1)) == E_TOOLARGE
    assert lib.pangnn_mask_k_smallest_workspace_bytes(big) == 0 and lib.pangnn_mask_k_smallest_workspace_bytes(-1) == 0
    assert fn(*_mask_args(keys=F + 8)) == E_ALIGN and fn(*_mask_args(keep=F + 1)) == E_ALIGN
    assert fn(*_mask_args(workspace=F + 4)) == E_ALIGN
    need = lib.pangnn_mask_k_smallest_workspace_bytes(5000)
    assert 0 < need < 1 << 16 and need == lib.pangnn_mask_k_smallest_workspace_bytes(1 << 30)     # independent of n
    assert fn(*_mask_args(workspace_bytes=need - 1)) == E_WORKSPACE and fn(*_mask_args(workspace_bytes=-1)) == E_WORKSPACE
    assert fn(*_mask_args(n=0, k=0, keys=None, keep=None)) == 0               # nothing to do, nothing launched
