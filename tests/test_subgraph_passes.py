"""`build_subgraphs(..., groups_per_pass=k)` builds k consecutive group ids at a time and joins the passes: the data set is the
all-at-once one bit for bit, whatever k (groups do not interact; the running sub-graph number and the dropped groups are what
the join can get wrong).  CPU tensors: the index-op route of every step."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from pangnn_amd import construct, simulate, subgraphs

FIELDS = ("node_off", "edge_off", "nb_off", "node_global", "edge_index", "neighbour_edge_index", "edge_attr", "y",
          "group_of_graph")
SIM_CASES = [(60, 4, 0.3, 1), (200, 4, 0.3, 2), (300, 6, 0.2, 1)]


def assert_same_dataset(a, b):
    assert a.num_graphs == b.num_graphs
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), f


def simulated_inputs(n, genomes, frac, device="cpu"):
    raw = simulate.simulate_raw(n, genomes, frac, 10, 2, seed=3, device=device)
    s, d, sc = construct.remove_trivial_cases(raw.src, raw.dst, raw.score, raw.genome_of)
    s, d, w = construct.normalize_sim_scores(s, d, sc, raw.genome_of)
    return raw, s, d, w


def passes_of(ngroups):
    return [1, 7, 64, ngroups, ngroups + 5]


@pytest.mark.parametrize("n,genomes,frac,neighbours", SIM_CASES)
def test_passes_equal_the_all_at_once_build(n, genomes, frac, neighbours):
    raw, s, d, w = simulated_inputs(n, genomes, frac)
    nodes = torch.arange(raw.num_nodes)
    kw = dict(neighbours=neighbours, labels_group_of=raw.group_of)
    whole = subgraphs.build_subgraphs(raw.num_nodes, s, d, w, raw.group_of, nodes, **kw)
    assert whole.num_graphs > 1
    ngroups = int(raw.group_of.max()) + 1
    assert ngroups > 7                                  # 7 groups per pass: several passes, the last one shorter
    for k in passes_of(ngroups):
        ds = subgraphs.build_subgraphs(raw.num_nodes, s, d, w, raw.group_of, nodes, groups_per_pass=k, **kw)
        assert_same_dataset(ds, whole)
    assert_same_dataset(subgraphs.build_subgraphs(raw.num_nodes, s, d, w, raw.group_of, nodes, groups_per_pass=None, **kw), whole)


def _groups_from_pairs(f):
    """ortholog groups as (group id, member) arrays: a key gene and its members form one group (as tests/test_construct.py)"""
    ks, ms = f["grp_src"], f["grp_dst"]
    n = int(f["num_nodes"])
    gmin = np.arange(n)
    np.minimum.at(gmin, ks, ms)
    np.minimum.at(gmin, ks, ks)
    genes = np.unique(ks)
    rep = gmin[genes]
    rep = np.minimum(rep, gmin[rep])
    _, gid = np.unique(rep, return_inverse=True)
    return torch.from_numpy(gid.astype(np.int64)), torch.from_numpy(genes.astype(np.int64))


@pytest.mark.parametrize("name,subset", [("sim_200x4", False), ("cfg1_2genomes", True), ("cfg3_5genomes", True),
                                         ("cfg2_sim_1000x5", False)])
def test_passes_equal_the_all_at_once_build_on_the_golden_relations(name, subset):
    """explicit pair labels and, on the genome subsets, groups dropped for having fewer edges than members: sub-graph numbers
    run on across passes that drop groups"""
    f = load_golden(name)
    n = int(f["num_nodes"])
    gid, mem = _groups_from_pairs(f)
    T = lambda k: torch.from_numpy(f[k])
    args = (n, T("nrm_src"), T("nrm_dst"), T("nrm_weight"), gid, mem)
    kw = dict(neighbours=1, pair_src=T("grp_src"), pair_dst=T("grp_dst"), require_edges_ge_members=True)
    whole = subgraphs.build_subgraphs(*args, **kw)
    ngroups = int(gid.max()) + 1
    assert 1 < whole.num_graphs
    if subset:
        assert whole.num_graphs < ngroups                   # some group is dropped
    for k in passes_of(ngroups):
        assert_same_dataset(subgraphs.build_subgraphs(*args, groups_per_pass=k, **kw), whole)


def test_keyword_rules_and_pass_through():
    raw, s, d, w = simulated_inputs(60, 4, 0.3)
    nodes = torch.arange(raw.num_nodes)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="groups_per_pass"):
            subgraphs.build_subgraphs(raw.num_nodes, s, d, w, raw.group_of, nodes, labels_group_of=raw.group_of,
                                      groups_per_pass=bad)
    a = simulate.simulate_subgraph_dataset(60, 4, 0.3, 10, 2, seed=3)
    b = simulate.simulate_subgraph_dataset(60, 4, 0.3, 10, 2, seed=3, groups_per_pass=5)
    assert_same_dataset(a, b)
    # no group at all: an empty data set either way
    none = torch.zeros(0, dtype=torch.int64)
    for k in (None, 4):
        e = subgraphs.build_subgraphs(raw.num_nodes, s, d, w, none, none, labels_group_of=raw.group_of, groups_per_pass=k)
        assert e.num_graphs == 0 and e.edge_index.shape == (2, 0) and e.node_off.tolist() == [0]


def test_index_op_step_is_the_route_of_cpu_tensors():
    """the factored-out definition: CPU tensors never reach the kernel, whatever the switch says"""
    raw, s, d, w = simulated_inputs(200, 4, 0.3)
    src, dst, weight, rowptr = subgraphs._canonical_relation(raw.num_nodes, s, d, w)
    gid = raw.group_of
    t = subgraphs._pass_tables(raw.num_nodes, rowptr, dst, gid, torch.arange(raw.num_nodes), int(gid.max()) + 1, 1)
    assert subgraphs.INDUCED_KERNEL is True
    got = subgraphs.induced_edges(raw.num_nodes, rowptr, dst, t)
    want = subgraphs._induced_edges_index_ops(raw.num_nodes, rowptr, dst, t)
    assert len(got) == 4 and all(torch.equal(a, b) for a, b in zip(got, want))
    eg, epos, s_local, t_local = want
    assert eg.numel() > 0 and bool((eg[1:] >= eg[:-1]).all())
    # every triple is an edge of the relation between two nodes of the group
    node_of = lambda g, l: t.all_n[t.node_off_g[g] + l]
    assert torch.equal(node_of(eg, s_local), src[epos]) and torch.equal(node_of(eg, t_local), dst[epos])
