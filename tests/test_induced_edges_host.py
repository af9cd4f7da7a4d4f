"""The entry points of the induced-edge pass (csrc/induced_edges.hip), the part that needs no GPU: the binding and every
argument check of the host halves (fake pointers, nothing launched)."""
import pytest
import torch

from pangnn_amd import _lib, subgraphs

F = 0x7f0000100000             # a fake device pointer
E_BADARG, E_TOOLARGE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -4
TABLES = ("rowptr", "row_node", "group_off", "sorted_node", "sorted_local")
HEAD = ("rowptr", "dst", "n", "e", "row_node", "rows", "group_off", "groups", "sorted_node", "sorted_local")

no_gpu = pytest.mark.skipif(torch.cuda.is_available(),
                            reason="fake device pointers: only where a missing check cannot reach a GPU")


def test_abi_version_is_still_3_and_the_binding_has_the_entries():
    lib = _lib.load()
    assert lib.pangnn_abi_version() == 3 == _lib.ABI_VERSION
    for name in ("pangnn_induced_edges_scratch_bytes", "pangnn_induced_edges_count", "pangnn_induced_edges_fill"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert subgraphs.INDUCED_KERNEL is True


def _head(**kw):
    a = dict(rowptr=F, dst=F, n=1000, e=5000, row_node=F, rows=300, group_off=F, groups=7, sorted_node=F, sorted_local=F)
    a.update(kw)
    return a


def _count(lib, **kw):
    a = _head(row_off=F, scratch=F, scratch_bytes=1 << 30)
    a.update(kw)
    return lib.pangnn_induced_edges_count(*(a[k] for k in HEAD + ("row_off", "scratch", "scratch_bytes")), None)


def _fill(lib, **kw):
    a = _head(row_off=F, total=100, out_src=F, out_dst=F, out_pos=F)
    a.update(kw)
    return lib.pangnn_induced_edges_fill(*(a[k] for k in HEAD + ("row_off", "total", "out_src", "out_dst", "out_pos")), None)


@no_gpu
@pytest.mark.parametrize("call,name", [(_count, "pangnn_induced_edges_count"), (_fill, "pangnn_induced_edges_fill")],
                         ids=["count", "fill"])
def test_entry_points_refuse_bad_tables(call, name):
    """every call fails a check, so nothing is launched"""
    lib = _lib.load()

    def refused(code, **kw):
        assert call(lib, **kw) == code, kw
        assert name in lib.pangnn_last_error().decode(), kw

    for size in ("n", "e", "rows", "groups"):
        refused(E_BADARG, **{size: -1})
    refused(E_TOOLARGE, n=1 << 31)                                  # node ids are held as 32-bit words
    refused(E_TOOLARGE, n=1 << 40)
    refused(E_TOOLARGE, rows=1 << 40)
    refused(E_TOOLARGE, groups=1 << 40)
    refused(E_TOOLARGE, n=1 << 31, rowptr=None)                     # sizes before pointers
    refused(E_BADARG, groups=0)                                     # rows in no group
    refused(E_BADARG, n=0)                                          # rows of a graph without nodes
    for k in TABLES:
        refused(E_BADARG, **{k: None})
        assert b"null" in lib.pangnn_last_error().lower()
    refused(E_BADARG, dst=None)                                     # edges without their targets
    for k in TABLES + ("dst",):
        refused(E_ALIGN, **{k: F + 4})


@no_gpu
def test_count_checks_its_output_and_scratch():
    lib = _lib.load()
    name = b"pangnn_induced_edges_count"
    assert _count(lib, row_off=None) == E_BADARG and name in lib.pangnn_last_error()
    assert _count(lib, row_off=F + 4) == E_ALIGN
    assert _count(lib, scratch=None) == E_WORKSPACE and name in lib.pangnn_last_error()
    assert _count(lib, scratch=F + 8) == E_ALIGN and b"16-byte" in lib.pangnn_last_error()
    # the scratch holds 301 row counts in front of the scan's temporary: anything below that is too small whatever the scan needs
    for nbytes in (-1, 0, 301 * 8 - 1, 2559):
        assert _count(lib, scratch_bytes=nbytes) == E_WORKSPACE, nbytes
        assert b"too small" in lib.pangnn_last_error()
    assert _count(lib, rows=0, groups=0, scratch_bytes=255) == E_WORKSPACE       # even the empty row list scans one entry
    assert lib.pangnn_induced_edges_scratch_bytes(-1) == 0 and lib.pangnn_induced_edges_scratch_bytes(1 << 40) == 0
    # every argument plausible: the scan's temporary size comes from rocPRIM, whose query needs a device — without one the
    # call refuses to run; with one, a scratch one byte short is PANGNN_E_WORKSPACE
    need = lib.pangnn_induced_edges_scratch_bytes(300)
    if need == 0:
        assert _count(lib) == E_BADARG and b"size query" in lib.pangnn_last_error()
    else:
        assert need >= 2560 + 256 and _count(lib, scratch_bytes=need - 1) == E_WORKSPACE


@no_gpu
def test_fill_checks_its_outputs_and_has_nothing_to_do_for_no_triples():
    lib = _lib.load()
    name = b"pangnn_induced_edges_fill"
    assert _fill(lib, total=-1) == E_BADARG and name in lib.pangnn_last_error()
    for k in ("row_off", "out_src", "out_dst", "out_pos"):
        assert _fill(lib, **{k: None}) == E_BADARG and b"null" in lib.pangnn_last_error().lower(), k
        assert _fill(lib, **{k: F + 4}) == E_ALIGN, k
    assert _fill(lib, rows=0, groups=0) == E_BADARG                 # triples out of no rows
    assert _fill(lib, e=0, dst=None) == E_BADARG                    # ... or out of no edges
    # no triples: nothing to write, whatever the outputs; an empty row list or relation needs no tables either
    assert _fill(lib, total=0, row_off=None, out_src=None, out_dst=None, out_pos=None) == 0
    assert _fill(lib, total=0, rows=0, groups=0, **{k: None for k in TABLES + ("dst",)}) == 0
    assert _fill(lib, total=0, e=0, dst=None) == 0
    assert _fill(lib, total=0, n=1 << 31) == E_TOOLARGE             # the argument rules come first
