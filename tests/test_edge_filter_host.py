"""Per-step edge sub-sampling on the CPU (pangnn_amd/sampling.py): the semantics of sub_sample_graph_edges on plain torch
tensors — the definition the device path shares — and the argument checks of pangnn_structure_filter (fake pointers,
nothing launched).  Every comparison is exact."""
import pytest
import torch

from conftest import load_golden, random_graph
from pangnn_amd import _lib, filter_edges, sub_sample_graph_edges
from pangnn_amd.data import Data
from pangnn_amd.graph import EdgeStructure
from pangnn_amd.sampling import draw_keep_mask

GOLDEN = ["cfg2_sim_1000x5", "sim_200x4"]


def golden_graph(name):
    f = load_golden(name)
    return Data(x=torch.from_numpy(f["whole_x"]), edge_index=torch.from_numpy(f["whole_edge_index"]),
                edge_attr=torch.from_numpy(f["whole_edge_attr"]), y=torch.from_numpy(f["whole_y"]),
                neighbour_edge_index=torch.from_numpy(f["whole_neighbour_edge_index"]))


def seeded(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("name", GOLDEN)
def test_the_goldens_admit_fraction_0_8(name):
    g = golden_graph(name)
    e = g.edge_index.shape[1]
    assert float(g.y.sum()) / e < 0.8 and int((g.y == 0).sum()) >= int(0.2 * e)
    assert bool(((g.y == 0) | (g.y == 1)).all())


@pytest.mark.parametrize("fraction", [0.8, 0.5, 1.0])
@pytest.mark.parametrize("name", GOLDEN)
def test_negative_down_sampling_keeps_every_positive_and_the_exact_count(name, fraction):
    g = golden_graph(name)
    before = {k: v.clone() for k, v in g.__dict__.items() if torch.is_tensor(v)}
    e = g.edge_index.shape[1]
    c = sub_sample_graph_edges(g, None, fraction, generator=seeded(3))
    kept = c.kept_edge_id
    assert c.edge_index.shape[1] == kept.numel() == e - int(e * (1 - fraction))
    assert kept.dtype == torch.int64 and bool((kept[1:] > kept[:-1]).all())          # a subsequence of the parent's list
    assert torch.equal(c.edge_index, g.edge_index[:, kept]) and torch.equal(c.edge_attr, g.edge_attr[kept])
    assert torch.equal(c.y, g.y[kept]) and float(c.y.sum()) == float(g.y.sum())      # every positive stays
    dropped = torch.ones(e, dtype=torch.bool)
    dropped[kept] = False
    assert bool((g.y[dropped] == 0).all())
    assert c.x is g.x and c.neighbour_edge_index is g.neighbour_edge_index           # shared, not copied
    assert not hasattr(c, "_pangnn_structs")                                         # the CPU path yields no structure
    for k, v in before.items():
        assert torch.equal(getattr(g, k), v)                                         # the parent is left untouched
    assert set(g.keys()) == {"x", "edge_index", "edge_attr", "y", "neighbour_edge_index"}


def test_sampling_the_positives_too():
    g = golden_graph("cfg2_sim_1000x5")
    e = g.edge_index.shape[1]
    c = sub_sample_graph_edges(g, None, 0.8, True, generator=seeded(1))
    assert c.edge_index.shape[1] == e - int(e * (1 - 0.8))
    assert 0 < float(c.y.sum()) < float(g.y.sum())
    assert torch.equal(c.edge_index, g.edge_index[:, c.kept_edge_id])
    # uniform over all edges: the positive share of the sample is the parent's within a few standard errors
    share, p = float(c.y.mean()), float(g.y.mean())
    assert abs(share - p) < 6 * (p * (1 - p) / c.y.numel()) ** 0.5


def test_same_seed_same_subset_and_two_seeds_differ():
    g = golden_graph("sim_200x4")
    a = sub_sample_graph_edges(g, generator=seeded(7))
    b = sub_sample_graph_edges(g, generator=seeded(7))
    c = sub_sample_graph_edges(g, generator=seeded(8))
    assert torch.equal(a.kept_edge_id, b.kept_edge_id) and torch.equal(a.edge_index, b.edge_index)
    assert a.kept_edge_id.shape == c.kept_edge_id.shape and not torch.equal(a.kept_edge_id, c.kept_edge_id)
    gen = seeded(7)                                                                  # one generator: a fresh subset per call
    d, f = sub_sample_graph_edges(g, generator=gen), sub_sample_graph_edges(g, generator=gen)
    assert torch.equal(d.kept_edge_id, a.kept_edge_id) and not torch.equal(f.kept_edge_id, d.kept_edge_id)


def test_the_draw_is_uniform_over_the_negatives():
    """each negative is dropped with probability k / n_neg: over 400 draws its count is Binomial(400, p); the largest
    deviation over ~300 negatives stays inside 5 standard deviations (a fixed seed: this is a regression check)"""
    ei, _ = random_graph(60, 400, seed=1)
    y = torch.zeros(400)
    y[::4] = 1
    g = Data(x=torch.ones(60, 1), edge_index=ei, edge_attr=torch.ones(400), y=y)
    gen, drops = seeded(0), torch.zeros(400)
    k = int(400 * (1 - 0.8))                                                         # 79: 1 - 0.8 is just below 0.2
    for _ in range(400):
        keep, kept = draw_keep_mask(g, 0.8, generator=gen)
        assert kept == 400 - k and int(keep.sum()) == 400 - k and bool(keep[y > 0].all())
        drops += (~keep).float()
    p = k / 300
    assert bool((drops[y > 0] == 0).all())
    assert float((drops[y == 0] - 400 * p).abs().max()) < 5 * (400 * p * (1 - p)) ** 0.5


def test_refusals():
    g = golden_graph("sim_200x4")
    share = float(g.y.mean())
    with pytest.raises(ValueError, match="positive"):
        sub_sample_graph_edges(g, None, share * 0.9)                                 # the positive share exceeds `fraction`
    few = Data(x=torch.ones(4, 1), edge_index=torch.tensor([[0, 1, 2, 3, 0], [1, 2, 3, 0, 2]]), edge_attr=torch.ones(5),
               y=torch.tensor([1.0, 1.0, 1.0, 0.0, 0.0]))
    with pytest.raises(ValueError):
        sub_sample_graph_edges(few, None, 0.5)                                       # 2 to remove, 60 % positive > 0.5
    sub_sample_graph_edges(few, None, 0.6)                                           # 2 to remove, 2 negatives: possible
    union = golden_graph("sim_200x4")
    union.union_edge_index = torch.cat([union.edge_index, union.neighbour_edge_index], dim=1)
    with pytest.raises(ValueError, match="union"):
        sub_sample_graph_edges(union)
    with pytest.raises(ValueError, match="union"):
        filter_edges(union, torch.ones(union.edge_index.shape[1]))
    with pytest.raises(ValueError):
        filter_edges(g, torch.ones(5))                                               # keep of another length
    with pytest.raises(ValueError):
        sub_sample_graph_edges(g, None, 1.5)
    with pytest.raises(ValueError):
        sub_sample_graph_edges(Data(x=g.x, edge_index=g.edge_index, edge_attr=g.edge_attr))      # no labels to spare
    with pytest.raises(_lib.PangnnHipError):
        EdgeStructure.filtered(EdgeStructure(g.edge_index, g.num_nodes), torch.ones(g.edge_index.shape[1]))   # device only


def test_filter_edges_on_cpu_tensors_and_other_dtypes():
    ei, w = random_graph(50, 300, seed=2)
    g = Data(x=torch.ones(50, 1), edge_index=ei, edge_attr=w.double(), y=(w > 40).long(), gene_lst=["a", "b"])
    keep = (torch.arange(300) % 3 != 0).int() * 5
    c = filter_edges(g, keep)
    idx = torch.nonzero(keep).view(-1)
    assert torch.equal(c.kept_edge_id, idx) and torch.equal(c.edge_index, ei[:, idx])
    assert c.edge_attr.dtype == torch.float64 and torch.equal(c.edge_attr, g.edge_attr[idx])
    assert c.y.dtype == torch.int64 and torch.equal(c.y, g.y[idx]) and c.gene_lst is g.gene_lst
    none = filter_edges(g, torch.zeros(300))
    assert none.edge_index.shape == (2, 0) and none.y.numel() == 0
    empty = Data(x=torch.ones(3, 1), edge_index=torch.zeros(2, 0, dtype=torch.int64), edge_attr=torch.zeros(0), y=torch.zeros(0))
    assert sub_sample_graph_edges(empty).edge_index.shape == (2, 0)


F = 0x7f0000100000
E_BADARG, E_TOOLARGE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -4


def _args(**over):
    """a complete, plausible argument list of pangnn_structure_filter (fake pointers), with overrides by name"""
    a = dict(edge_index=F, ld=5000, num_edges=5000, num_nodes=1000, keep=F, keep_itemsize=1, num_kept=4000,
             rowptr_dst=F, other_dst=F, perm_dst=F, rowptr_src=F, other_src=F, perm_src=F, attr0=F, attr1=F,
             child_edge_index=F, child_ld=4000, kept_id=F, child_attr0=F, child_attr1=F,
             child_rowptr_dst=F, child_other_dst=F, child_perm_dst=F, child_rowptr_src=F, child_other_src=F,
             child_perm_src=F, count=F, status=F, workspace=F, workspace_bytes=1 << 30, stream=None)
    unknown = set(over) - set(a)
    assert not unknown, unknown
    a.update(over)
    return list(a.values())


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: only where a missing check cannot reach a GPU")
def test_filter_entry_point_refuses_bad_arguments():
    fn = _lib.load().pangnn_structure_filter
    for name in ("edge_index", "keep", "rowptr_dst", "other_dst", "perm_dst", "child_edge_index", "kept_id",
                 "child_rowptr_dst", "child_other_dst", "child_perm_dst", "child_rowptr_src", "child_other_src",
                 "child_perm_src", "count", "status", "workspace"):
        assert fn(*_args(**{name: None})) == E_BADARG, name                          # NULL inputs and outputs
    assert b"pangnn_structure_filter" in _lib.load().pangnn_last_error()
    assert fn(*_args(attr0=None)) == E_BADARG and fn(*_args(child_attr1=None)) == E_BADARG      # an array without its twin
    for over in (dict(num_edges=-1), dict(num_nodes=-1), dict(num_kept=-1), dict(ld=4999), dict(child_ld=3999),
                 dict(num_kept=5001, child_ld=5001)):
        assert fn(*_args(**over)) == E_BADARG, over                                  # negative / inconsistent sizes
    for itemsize in (-1, 0, 2, 3, 8):
        assert fn(*_args(keep_itemsize=itemsize)) == E_BADARG                        # keep_itemsize outside {1, 4}
    for part in (dict(rowptr_src=None), dict(other_src=None), dict(perm_src=None), dict(rowptr_src=None, other_src=None),
                 dict(other_src=None, perm_src=None)):
        assert fn(*_args(**part)) == E_BADARG, part                                  # the by-source trio only partly given
    assert b"by-source" in _lib.load().pangnn_last_error()
    big = 1 << 31
    assert fn(*_args(num_edges=big, ld=big)) == E_TOOLARGE
    assert fn(*_args(num_edges=big + 5, ld=big + 5, num_kept=big, child_ld=big)) == E_TOOLARGE
    assert fn(*_args(num_nodes=big)) == E_TOOLARGE
    assert b"pangnn_structure_filter" in _lib.load().pangnn_last_error()
    assert _lib.load().pangnn_structure_filter_workspace_bytes(-1) == 0
    assert _lib.load().pangnn_structure_filter_workspace_bytes(big) == 0
    assert fn(*_args(workspace=F + 4)) == E_ALIGN                                    # misaligned pointers
    assert fn(*_args(edge_index=F + 4)) == E_ALIGN and fn(*_args(child_perm_dst=F + 2)) == E_ALIGN
    assert fn(*_args(keep=F + 1, keep_itemsize=4)) == E_ALIGN
    # every argument plausible: the scans' temporary size comes from rocPRIM, whose query needs a device — without one the
    # call refuses to run (as pangnn_csr_build does); with one, a workspace one byte short is PANGNN_E_WORKSPACE
    need = _lib.load().pangnn_structure_filter_workspace_bytes(5000)
    if need == 0:
        assert fn(*_args()) == E_BADARG and b"size query" in _lib.load().pangnn_last_error()
    else:
        assert fn(*_args(workspace_bytes=need - 1)) == E_WORKSPACE and fn(*_args(workspace_bytes=-1)) == E_WORKSPACE
