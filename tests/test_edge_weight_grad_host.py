"""The two entry points of the edge-weight gradient (csrc/edge_weight_grad.hip), the part that needs no GPU: their argument
checks (fake pointers, nothing launched), the workspace size, and the routing predicates of the Python layer."""
import pytest
import torch

from pangnn_amd import _lib
from pangnn_amd import functional as PF

F = 0x7f0000100000             # a fake device pointer, 16-byte aligned
E_BADARG, E_TOOLARGE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -4
BIG = 1 << 40
WIDTHS = (16, 32, 64, 128, 256)

no_gpu = pytest.mark.skipif(torch.cuda.is_available(),
                            reason="fake device pointers: only where a missing check cannot reach a GPU")


def test_abi_version_is_still_3():
    lib = _lib.load()
    assert lib.pangnn_abi_version() == 3 == _lib.ABI_VERSION
    for name in ("pangnn_edge_dot_mixed", "pangnn_gcn_norm_bwd_f32", "pangnn_gcn_norm_bwd_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)


def _dot(lib, **kw):
    a = dict(rowptr=F, idx=F, perm=F, g=F, g_dtype=0, ldg=64, g_rows=100, x=F, x_dtype=0, ldx=64, x_rows=100, n_rows=100,
             nnz=1000, f=64, out_sorted=F, out_orig=F)
    a.update(kw)
    return lib.pangnn_edge_dot_mixed(*(a[k] for k in ("rowptr", "idx", "perm", "g", "g_dtype", "ldg", "g_rows", "x", "x_dtype",
                                                      "ldx", "x_rows", "n_rows", "nnz", "f", "out_sorted", "out_orig")), None)


@no_gpu
def test_edge_dot_refuses_bad_arguments():
    """every call fails a check (or has nothing to do), so nothing is launched"""
    lib = _lib.load()
    for f in (-1, 0, 8, 48, 96, 512):
        assert _dot(lib, f=f, ldg=max(f, 4), ldx=max(f, 4)) == E_BADARG
    assert "pangnn_edge_dot_mixed" in lib.pangnn_last_error().decode()
    for dt in (-1, 3):
        assert _dot(lib, g_dtype=dt) == E_BADARG and _dot(lib, x_dtype=dt) == E_BADARG
    assert _dot(lib, g_dtype=1, x_dtype=2) == E_BADARG and _dot(lib, g_dtype=2, x_dtype=1) == E_BADARG      # one 2-byte type
    for dt in (1, 2):                      # width 16 is gathered as float32 only, like the propagate
        assert _dot(lib, f=16, ldg=16, ldx=16, g_dtype=dt) == E_BADARG
        assert _dot(lib, f=16, ldg=16, ldx=16, x_dtype=dt) == E_BADARG
    assert _dot(lib, n_rows=-1) == E_BADARG and _dot(lib, nnz=-1) == E_BADARG and _dot(lib, x_rows=-1) == E_BADARG
    assert _dot(lib, g_rows=99) == E_BADARG                                    # a g row per CSR row
    assert _dot(lib, ldg=60) == E_BADARG and _dot(lib, ldx=60) == E_BADARG     # below F
    assert _dot(lib, n_rows=0, g_rows=0) == E_BADARG and _dot(lib, x_rows=0) == E_BADARG      # entries without rows
    assert _dot(lib, nnz=1 << 31) == E_TOOLARGE and _dot(lib, x_rows=1 << 31) == E_TOOLARGE
    assert _dot(lib, n_rows=1 << 31, g_rows=1 << 31) == E_TOOLARGE
    for k in ("rowptr", "idx", "g", "x", "out_sorted"):
        assert _dot(lib, **{k: None}) == E_BADARG, k
    assert b"null" in lib.pangnn_last_error().lower()
    assert _dot(lib, perm=None) == E_BADARG                                     # out_orig needs perm
    for k in ("g", "x"):
        assert _dot(lib, **{k: F + 8}) == E_ALIGN, k                            # float32 rows start on 16 bytes
        assert _dot(lib, **{k: F + 4, k + "_dtype": 1}) == E_ALIGN, k           # 2-byte rows on 8
    assert _dot(lib, ldg=66) == E_ALIGN and _dot(lib, ldx=66) == E_ALIGN        # strides are multiples of 4
    assert _dot(lib, g=F + 8, idx=None) == E_BADARG                             # null pointers before alignment
    # the empty list: nothing to do, whatever the pointers
    assert _dot(lib, nnz=0, rowptr=None, idx=None, perm=None, g=None, x=None, out_sorted=None, out_orig=None) == 0
    assert _dot(lib, nnz=0, n_rows=0, g_rows=0, x_rows=0) == 0


def _norm(lib, **kw):
    a = dict(ei=F, ld=1000, e=1000, n=100, rp_d=F, ot_d=F, pm_d=F, seg_d=None, prp_d=None, ns_d=0, rp_s=F, ot_s=F, pm_s=F,
             seg_s=None, prp_s=None, ns_s=0, w=F, gw=F, dis=F, out=F, ws=F, ws_bytes=BIG)
    a.update(kw)
    return lib.pangnn_gcn_norm_bwd_f32(*(a[k] for k in ("ei", "ld", "e", "n", "rp_d", "ot_d", "pm_d", "seg_d", "prp_d", "ns_d",
                                                        "rp_s", "ot_s", "pm_s", "seg_s", "prp_s", "ns_s", "w", "gw", "dis",
                                                        "out", "ws", "ws_bytes")), None)


@no_gpu
def test_gcn_norm_bwd_refuses_bad_arguments():
    lib = _lib.load()
    assert _norm(lib, e=-1) == E_BADARG and _norm(lib, n=-1) == E_BADARG and _norm(lib, ld=999) == E_BADARG
    assert "pangnn_gcn_norm_bwd_f32" in lib.pangnn_last_error().decode()
    assert _norm(lib, n=0) == E_BADARG                                          # edges without nodes
    assert _norm(lib, e=1 << 31, ld=1 << 31) == E_TOOLARGE and _norm(lib, n=1 << 31) == E_TOOLARGE
    for k in ("ei", "rp_d", "ot_d", "pm_d", "rp_s", "ot_s", "pm_s", "w", "gw", "dis", "out"):
        assert _norm(lib, **{k: None}) == E_BADARG, k
    for o in ("d", "s"):                                                        # a segment table comes whole
        assert _norm(lib, **{"seg_" + o: F}) == E_BADARG and _norm(lib, **{"prp_" + o: F}) == E_BADARG
        assert _norm(lib, **{"seg_" + o: F, "prp_" + o: F, "ns_" + o: 99}) == E_BADARG      # a segment per row at the least
        assert _norm(lib, **{"seg_" + o: F, "prp_" + o: F, "ns_" + o: -1}) == E_BADARG
    need = lib.pangnn_gcn_norm_bwd_workspace_bytes(100, 0, 0)
    assert need >= 4 * 100
    assert _norm(lib, ws_bytes=need - 1) == E_WORKSPACE and _norm(lib, ws=None) == E_WORKSPACE
    assert _norm(lib, ws_bytes=0) == E_WORKSPACE and _norm(lib, ws_bytes=-1) == E_WORKSPACE
    assert b"workspace" in lib.pangnn_last_error().lower()
    need_seg = lib.pangnn_gcn_norm_bwd_workspace_bytes(100, 130, 0)
    assert need_seg >= need + 4 * 130
    assert _norm(lib, seg_d=F, prp_d=F, ns_d=130, ws_bytes=need) == E_WORKSPACE  # the segment partials count
    assert _norm(lib, ws=F + 4) == E_ALIGN
    assert _norm(lib, ws=F + 4, w=None) == E_BADARG                             # null pointers before the workspace
    assert _norm(lib, e=0, ld=0, ei=None, w=None, gw=None, out=None, ws=None, ws_bytes=0) == 0     # the empty list


def test_workspace_bytes():
    lib = _lib.load()
    sizes = [lib.pangnn_gcn_norm_bwd_workspace_bytes(n, 0, 0) for n in (0, 1, 5, 1000, 10 ** 6)]
    assert sizes == sorted(sizes) and all(s % 16 == 0 for s in sizes)
    assert lib.pangnn_gcn_norm_bwd_workspace_bytes(-1, 0, 0) == 0
    assert lib.pangnn_gcn_norm_bwd_workspace_bytes(10, -1, 0) == 0 == lib.pangnn_gcn_norm_bwd_workspace_bytes(10, 0, -1)


def test_route_predicate():
    """propagate_w is the route exactly when the weights require grad and grad is on; a watching mode raises"""
    w = torch.rand(5)
    assert not PF.wants_weight_grad(None) and not PF.wants_weight_grad(w)
    w.requires_grad_()
    assert PF.wants_weight_grad(w) and PF.wants_weight_grad(2 * torch.sigmoid(w))
    with torch.no_grad():
        assert not PF.wants_weight_grad(w)

    class Watch(torch.utils._python_dispatch.TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            return func(*args, **(kwargs or {}))

    with Watch():
        assert not PF.wants_weight_grad(w.detach())
        with pytest.raises(NotImplementedError, match="edge_weight"):
            PF.wants_weight_grad(w)
