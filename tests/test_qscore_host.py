"""The two entry points of the differentiable Q-score weights (csrc/qscore.hip), the part that needs no GPU: their argument
checks (fake pointers, nothing launched), the binding, and the host-side rules of pangnn_amd.weights."""
import pytest
import torch

from pangnn_amd import _lib, construct, simulate, weights

F = 0x7f0000100000             # a fake device pointer
E_BADARG, E_TOOLARGE = -1, -2
F32, F64 = 0, 3

no_gpu = pytest.mark.skipif(torch.cuda.is_available(),
                            reason="fake device pointers: only where a missing check cannot reach a GPU")


def test_abi_version_is_still_3_and_the_binding_has_both():
    lib = _lib.load()
    assert lib.pangnn_abi_version() == 3 == _lib.ABI_VERSION
    for name in ("pangnn_qscore_fwd", "pangnn_qscore_bwd"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert weights.SUM_PARTS == 1024 and weights.DTYPE_F64 == F64


def _fwd(lib, **kw):
    a = dict(rowptr=F, item=F, score=F, score_dtype=F64, nseg=100, e=1000, t=F, eps=1e-8, pseudo=1.0, weight=F,
             weight_dtype=F32, lse=F)
    a.update(kw)
    return lib.pangnn_qscore_fwd(*(a[k] for k in ("rowptr", "item", "score", "score_dtype", "nseg", "e", "t", "eps", "pseudo",
                                                  "weight", "weight_dtype", "lse")), None)


def _bwd(lib, **kw):
    a = dict(rowptr=F, item=F, score=F, score_dtype=F64, g=F, g_dtype=F32, lse=F, nseg=100, e=1000, t=F, eps=1e-8, gscore=F,
             gt=F, parts=F)
    a.update(kw)
    return lib.pangnn_qscore_bwd(*(a[k] for k in ("rowptr", "item", "score", "score_dtype", "g", "g_dtype", "lse", "nseg", "e",
                                                  "t", "eps", "gscore", "gt", "parts")), None)


@no_gpu
@pytest.mark.parametrize("call,name,other_dtype,pointers", [
    (_fwd, "pangnn_qscore_fwd", "weight_dtype", ("rowptr", "item", "score", "t", "weight", "lse")),
    (_bwd, "pangnn_qscore_bwd", "g_dtype", ("rowptr", "item", "score", "g", "lse", "t")),
], ids=["fwd", "bwd"])
def test_entry_points_refuse_bad_arguments(call, name, other_dtype, pointers):
    """every call fails a check (or has nothing to do), so nothing is launched"""
    lib = _lib.load()

    def refused(code, **kw):
        assert call(lib, **kw) == code, kw
        assert name in lib.pangnn_last_error().decode(), kw

    refused(E_BADARG, nseg=-1)
    refused(E_BADARG, e=-1)
    for dt in (-1, 1, 2, 4):                                   # float32 (0) and float64 (3) only
        refused(E_BADARG, score_dtype=dt)
        refused(E_BADARG, **{other_dtype: dt})
    for eps in (0.0, -1e-8, 0.5, 1.0, float("nan")):
        refused(E_BADARG, eps=eps)
    refused(E_TOOLARGE, e=1 << 31)
    refused(E_TOOLARGE, e=1 << 40, nseg=1 << 31)
    refused(E_BADARG, nseg=0)                                  # edges in no segment
    refused(E_BADARG, nseg=1001)                               # an empty segment
    for k in pointers:
        refused(E_BADARG, **{k: None})
        assert b"null" in lib.pangnn_last_error().lower()
    assert call(lib, e=1 << 31, rowptr=None) == E_TOOLARGE     # sizes before pointers
    # the empty relation: nothing to do, whatever the pointers
    assert call(lib, e=0, nseg=0, **{k: None for k in pointers}) == 0
    for dt in (F32, F64):
        assert call(lib, e=0, nseg=0, score_dtype=dt, **{other_dtype: dt}) == 0


@no_gpu
def test_bwd_outputs_are_optional():
    lib = _lib.load()
    assert _bwd(lib, gscore=None, gt=None, parts=None) == 0                    # nothing asked for: nothing launched
    assert _bwd(lib, gscore=None, gt=None, parts=None, rowptr=None) == 0
    assert _bwd(lib, parts=None) == E_BADARG                                   # dL/dt needs its scratch
    assert "pangnn_qscore_bwd" in lib.pangnn_last_error().decode()
    assert _bwd(lib, gscore=None, parts=None) == E_BADARG
    assert _bwd(lib, gscore=None, gt=None, parts=None, eps=0.7) == E_BADARG    # argument rules first


def test_route_predicate():
    """a gradient in score or t under a tracer / dispatch mode raises instead of being dropped (PF.wants_weight_grad)"""
    s, t = torch.rand(5), torch.tensor(0.8)
    assert not weights.wants_qscore_grad(s, 0.8) and not weights.wants_qscore_grad(s, t)
    assert weights.wants_qscore_grad(s.clone().requires_grad_(), 0.8)
    assert weights.wants_qscore_grad(s, t.clone().requires_grad_())
    with torch.no_grad():
        assert not weights.wants_qscore_grad(s.clone().requires_grad_(), 0.8)

    class Watch(torch.utils._python_dispatch.TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            return func(*args, **(kwargs or {}))

    with Watch():
        assert not weights.wants_qscore_grad(s, t)
        for a, b in ((s.clone().requires_grad_(), t), (s, t.clone().requires_grad_())):
            with pytest.raises(NotImplementedError, match="no dispatcher op yet"):
                weights.wants_qscore_grad(a, b)


def test_keep_raw_is_opt_in():
    plain = simulate.simulate_graph(60, 3, 0.3, 10, 2, seed=1)
    kept = simulate.simulate_graph(60, 3, 0.3, 10, 2, seed=1, keep_raw=True)
    assert not hasattr(plain, "raw_score") and sorted(set(vars(kept)) - set(vars(plain))) == ["raw_score"]
    for k, v in vars(plain).items():
        assert torch.equal(v, getattr(kept, k)) if torch.is_tensor(v) else v == getattr(kept, k), k
    assert kept.raw_score.shape == kept.edge_attr.shape and torch.equal(kept.genome_of, plain.genome_of)
    raw = simulate.simulate_raw(60, 3, 0.3, 10, 2, seed=1)
    s, d, sc = construct.remove_trivial_cases(raw.src, raw.dst, raw.score, raw.genome_of)
    look = {(int(a), int(b)): float(c) for a, b, c in zip(s, d, sc)}
    assert [look[(int(a), int(b))] for a, b in kept.edge_index.t()] == kept.raw_score.tolist()
    g = construct.build_from_raw(raw.num_nodes, raw.src, raw.dst, raw.score, raw.genome_of, group_of=raw.group_of)
    assert not hasattr(g, "raw_score") and not hasattr(g, "genome_of")
    n = construct.normalize_sim_scores(s, d, sc, raw.genome_of)
    w = construct.whole_graph(raw.num_nodes, *n, raw.group_of)
    assert not hasattr(w, "raw_score")
    with pytest.raises(ValueError, match="keep_raw"):
        construct.whole_graph(raw.num_nodes, *n, raw.group_of, keep_raw=True)
    w = construct.whole_graph(raw.num_nodes, *n, raw.group_of, keep_raw=True, raw=(s, d, sc), genome_of=raw.genome_of)
    assert torch.equal(w.raw_score, kept.raw_score)


def test_module_and_argument_rules():
    g = simulate.simulate_graph(60, 3, 0.3, 10, 2, seed=1, keep_raw=True)
    m = weights.QScoreWeights(t=0.8)
    assert float(m.temperature()) == 0.8 and m.log_t.requires_grad and abs(float(m.log_t) - (-0.2231435513142097)) < 1e-15
    assert not weights.QScoreWeights(learn_t=False).log_t.requires_grad
    w = m(g)
    assert torch.equal(w.detach(), g.edge_attr) and w.dtype == torch.float32            # the construction's weights
    g2 = m.apply_to(g)
    assert g2 is not g and g2.edge_index is g.edge_index and g2.edge_attr.requires_grad and not g.edge_attr.requires_grad
    g2.edge_attr.sum().backward()
    assert bool(torch.isfinite(m.log_t.grad)) and float(m.log_t.grad) != 0.0
    m2 = weights.QScoreWeights(t=2.0, epsilon=1e-6, pseudo_count=0.0)
    assert float(m2(g).max()) <= 60.0 + 1e-4 and float(m2(g).min()) >= 0.0
    seg = weights.score_segments(g.edge_index, g.genome_of)
    assert seg.item.dtype == torch.int32 and seg.rowptr.dtype == torch.int64 and int(seg.rowptr[-1]) == seg.num_edges
    with pytest.raises(ValueError):
        weights.qscore_weights(g.raw_score[:-1], seg)
    with pytest.raises(ValueError):
        weights.qscore_weights(g.raw_score, seg, epsilon=0.5)
    with pytest.raises(ValueError):
        weights.qscore_weights(g.raw_score, seg, out_dtype=torch.float16)
    with pytest.raises(ValueError):
        weights.qscore_weights(g.raw_score, seg, torch.tensor([0.8, 0.9]))
    with pytest.raises(ValueError):
        weights.QScoreWeights(t=0.0)
