"""Host halves of the two entry points of the T pass's stream route, on a box without a GPU (fake pointers, as in
test_c_abi_host.py): pangnn_decoder_dgrad_stream_f32 refuses a missing stream, a list beyond the 31-bit edge ids and a
workspace one byte short before anything is launched; pangnn_csr_plan_tpos checks sizes, span, pointers and alignment."""
import pytest
import torch

from pangnn_amd import _lib

pytestmark = pytest.mark.skipif(torch.cuda.is_available(),
                                reason="fake device pointers: only where a missing check cannot reach a GPU")

F = 0x7f0000100000          # an aligned address that is never dereferenced
E_BADARG, E_TOOLARGE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -4
E = 60_000_000              # a list whose launch is the whole chip: the entry needs the full workspace query


def test_binding_and_header_declare_both():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "pangnn_hip.h")).read()
    for name in ("pangnn_decoder_dgrad_stream_f32", "pangnn_csr_plan_tpos"):
        assert name in _lib.SIGNATURES and re.search(r"\b" + name + r"\(", hdr)
    assert _lib.load().pangnn_abi_version() == _lib.ABI_VERSION        # additive: the number stays, every symbol is resolved


def test_stream_entry_argument_checks():
    L = _lib.load()
    need = L.pangnn_decoder_dgrad_workspace_bytes()
    assert need > 0
    call = lambda tpos, parts, off, gb2, ws, b, e=E: L.pangnn_decoder_dgrad_stream_f32(F, tpos, F, F, e, parts, off, gb2, ws, b, None)   # noqa: E731
    assert call(F, F, F, F, F, need - 1) == E_WORKSPACE and b"workspace" in L.pangnn_last_error().lower()
    assert call(F, F, F, F, F, 0) == E_WORKSPACE and call(F, F, F, F, None, need) == E_WORKSPACE
    assert call(F, F, F, F, F, -1) == E_BADARG
    assert call(None, F, F, F, F, need) == E_BADARG                    # the stream is required ...
    assert call(F, None, F, F, F, need) == E_BADARG and call(F, F, None, F, F, need) == E_BADARG      # ... with both part tables
    assert call(F + 2, F, F, F, F, need) == E_BADARG                   # words are 4-byte aligned
    assert call(F, F, F, F, F, need, e=2 ** 31 + 5) == E_TOOLARGE and call(F, F, F, F, F, need, e=2 ** 31 - 1) == E_TOOLARGE
    assert call(F, F, F, F, F, need, e=-1) == E_BADARG
    assert L.pangnn_decoder_dgrad_stream_f32(None, F, F, F, E, F, F, None, None, 0, None) == E_BADARG   # rec
    # the keys entry is what it was: no stream, same refusals
    assert L.pangnn_decoder_dgrad_f32(F, F, None, F, F, E, F, F, None, None, None, 0, None) == E_BADARG  # run sums need keys


def test_plan_tpos_argument_checks():
    L = _lib.load()
    ok = lambda perm=F, keys=F, e=E, span=512, tpos=F: L.pangnn_csr_plan_tpos(perm, keys, e, span, tpos, None)   # noqa: E731
    assert ok(e=0) == E_BADARG and ok(e=-3) == E_BADARG
    assert ok(e=2 ** 31 - 1) == E_TOOLARGE and ok(e=2 ** 31 + 5) == E_TOOLARGE
    assert ok(span=0) == E_BADARG and ok(span=48) == E_BADARG and ok(span=-32) == E_BADARG
    assert ok(perm=None) == E_BADARG and ok(keys=None) == E_BADARG and ok(tpos=None) == E_BADARG
    assert ok(perm=F + 2) == E_ALIGN and ok(keys=F + 1) == E_ALIGN and ok(tpos=F + 2) == E_ALIGN
