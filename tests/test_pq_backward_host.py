"""Host half of pangnn_linear_act_backward_parts_f32 on a box without a GPU (fake device pointers, as tests/test_c_abi_host.py
does for the other entry points that carve a caller-provided workspace): shape, size and alignment errors first, then a
workspace one byte short of pangnn_linear_wgrad_workspace_bytes(64, 128) is refused before anything is launched."""
import pytest
import torch

from pangnn_amd import _lib

pytestmark = pytest.mark.skipif(torch.cuda.is_available(),
                                reason="fake device pointers: only where a missing check cannot reach a GPU")

F = 0x7f0000100000          # a 16-byte aligned address that is never dereferenced
E_BADARG, E_TOOLARGE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -4
N = 4_000_000               # the grid is the whole chip: the entry needs the full workspace


def _call(ws_bytes, n=N, K=64, M=128, in_act=1, parts_s=F, n_parts_s=N, x=F, gb=F):
    L = _lib.load()
    return L.pangnn_linear_act_backward_parts_f32(parts_s, F, n_parts_s, F, F, N, x, 64, F, n, K, M, in_act, F, 64, F, gb, F,
                                                  ws_bytes, None)


def test_workspace_one_byte_short_is_refused_before_anything_runs():
    L = _lib.load()
    need = L.pangnn_linear_wgrad_workspace_bytes(64, 128)
    assert need > 0
    for short in (need - 1, 0, -1):
        assert _call(short) == E_WORKSPACE, (short, L.pangnn_last_error())
        assert b"workspace" in L.pangnn_last_error().lower()


def test_argument_errors_come_before_the_workspace_check():
    L = _lib.load()
    need = L.pangnn_linear_wgrad_workspace_bytes(64, 128)
    assert _call(need, K=128) == E_BADARG                      # only the 64 -> 128 layer
    assert _call(need, M=64) == E_BADARG
    assert _call(need, in_act=2) == E_BADARG
    assert _call(need, n=-1) == E_BADARG
    assert _call(need, gb=None) == E_BADARG                    # null pointer
    assert _call(need, x=F + 4) == E_ALIGN
    assert _call(need, parts_s=F + 8) == E_ALIGN
    assert _call(need, n_parts_s=1 << 31) == E_TOOLARGE        # part positions are 32-bit in the kernel
