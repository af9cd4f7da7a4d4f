"""Host side of the live-aware fused-loss passes (a padded fixed-shape batch whose real-edge count the kernels read from
device memory): pangnn_edge_score_loss_live_mixed (csrc/edge_score.hip), pangnn_decoder_nd_loss_live_f32 and
pangnn_decoder_mlp_loss_live_f32 (csrc/decoder.hip) — the symbols and the ABI number, their argument checks on pointers that
are never dereferenced, and the dispatcher op pangnn::edge_score_loss_live (schema, fake kernel).  No GPU."""
import pytest
import torch

NEW_SYMBOLS = ("pangnn_edge_score_loss_live_mixed", "pangnn_decoder_nd_loss_live_f32", "pangnn_decoder_mlp_loss_live_f32")
_F = 0x7f0000100000          # a 16-byte aligned address that is never dereferenced
BAD, ALIGN = -1, -4          # PANGNN_E_BADARG, PANGNN_E_ALIGN


def test_new_symbols_resolve_and_the_abi_number_stays():
    from pangnn_amd import _lib
    L = _lib.load()
    assert L.pangnn_abi_version() == 3
    for name in NEW_SYMBOLS:
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) > 0, name
    # the live forms take the arguments of their plain forms plus the count's pointer
    for live, plain in (("pangnn_edge_score_loss_live_mixed", "pangnn_edge_score_loss_mixed"),
                        ("pangnn_decoder_nd_loss_live_f32", "pangnn_decoder_nd_loss_f32"),
                        ("pangnn_decoder_mlp_loss_live_f32", "pangnn_decoder_mlp_loss_f32")):
        assert len(getattr(L, live).argtypes) == len(getattr(L, plain).argtypes) + 1


def _score_args(z=_F, d=64, y=_F, live=_F, mode=1, n=1000, e=5000):
    # z, z_dtype, ldz, num_nodes, edge_index, ld, num_edges, d, mode, y, pos_weight, denom, norms, logits, loss, g_logits, parts,
    # live_edges, stream
    return (z, 0, 64 if d <= 64 else d, n, _F, e, e, d, mode, y, None, 0, _F, _F, _F, _F, _F, live, None)


def _decoder_args(nd, d, p=_F, y=_F, live=_F, n=1000, e=5000):
    head = (p, d, _F, d, n, _F, e, e, None, None, _F, _F, _F, _F, d)
    mid = (y, None, 0, _F, _F, _F, _F, _F, _F, _F, None, None, None)       # y, pos_weight, denom, logits .. part_off
    tail = (live, _F, 1 << 30, None)                                       # live_edges, workspace, bytes, stream
    return head + mid + (() if nd else (0,)) + tail                        # the mlp family: `precision` in front of live_edges


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: only where a missing check cannot reach a GPU")
def test_argument_checks_refuse_before_any_launch():
    from pangnn_amd import _lib
    L = _lib.load()
    score = L.pangnn_edge_score_loss_live_mixed
    assert score(*_score_args(live=None)) == BAD                           # null live_edges: required here
    assert b"pangnn_edge_score_loss_live_mixed" in L.pangnn_last_error()
    assert score(*_score_args(y=None)) == BAD                              # null y
    for d in (0, 8, 48, 63, 512):
        assert score(*_score_args(d=d)) == BAD                             # D
    assert score(*_score_args(z=_F + 4, mode=0)) == ALIGN                  # misaligned f32 rows
    assert score(*_score_args(mode=2)) == BAD
    for name, nd, good, bad in (("pangnn_decoder_nd_loss_live_f32", True, (32, 128), (64, 16, 48, 256)),
                                ("pangnn_decoder_mlp_loss_live_f32", False, (64,), (32, 128, 0))):
        fn = getattr(L, name)
        for d in good:
            assert fn(*_decoder_args(nd, d, live=None)) == BAD             # null live_edges
            assert name.encode() in L.pangnn_last_error() and b"live_edges" in L.pangnn_last_error()
            assert fn(*_decoder_args(nd, d, y=None)) == BAD                # null y
            assert fn(*_decoder_args(nd, d, p=_F + 4)) == ALIGN            # misaligned rows
        for d in bad:
            assert fn(*_decoder_args(nd, d)) == BAD                        # D
    args = list(_decoder_args(False, 64))                                  # strict fp32 only: the mlp family's `precision`
    assert args[28] == 0
    args[28] = 1
    assert L.pangnn_decoder_mlp_loss_live_f32(*args) == BAD


def test_the_op_is_registered_with_its_schema_and_the_pinned_ones_stay():
    from pangnn_amd import torch_ops  # noqa: F401
    ops = torch.ops.pangnn
    assert str(ops.edge_score_loss_live.default._schema) == (
        "pangnn::edge_score_loss_live(Tensor z, Tensor edge_index, int mode, Tensor y, Tensor? pos_weight, Tensor live) -> "
        "(Tensor, Tensor, Tensor, Tensor)")
    assert str(ops.edge_score_loss.default._schema) == (
        "pangnn::edge_score_loss(Tensor z, Tensor edge_index, int mode, Tensor y, Tensor? pos_weight, int denom) -> "
        "(Tensor, Tensor, Tensor, Tensor)")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fake_kernel_traces_with_shapes_and_dtypes(dtype):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from pangnn_amd import torch_ops  # noqa: F401
    ops = torch.ops.pangnn
    with FakeTensorMode():
        z = torch.empty(7, 32, dtype=dtype)
        ei = torch.empty(2, 11, dtype=torch.int64)
        y = torch.empty(11)
        live = torch.empty(1, dtype=torch.int64)
        for mode in (0, 1):
            loss, lg, g_l, nm = ops.edge_score_loss_live(z, ei, mode, y, None, live)
            assert loss.shape == () and lg.shape == g_l.shape == (11,)
            assert nm.shape == ((7, 2) if mode else (0, 2))
            assert loss.dtype == lg.dtype == g_l.dtype == nm.dtype == torch.float32
