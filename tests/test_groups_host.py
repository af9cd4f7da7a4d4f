"""Gene groups from edge predictions on the CPU (pangnn_amd/postprocessing.py): the plain-torch path against
scipy.sparse.csgraph.connected_components + a per-component min (which pins the label vector exactly), the `Groups`
invariants, group_agreement, write_groups_file, the reference's defect that makes the semantics build-defined, and the
argument checks of pangnn_components_i32 (fake pointers, nothing launched).  Every comparison is exact."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch
from scipy.sparse.csgraph import connected_components as scipy_components
from types import SimpleNamespace

from conftest import load_golden, random_graph
from pangnn_amd import _lib
from pangnn_amd import functional as PF
from pangnn_amd.postprocessing import (Groups, connected_components, group_agreement, homolog_groups,
                                       write_groups_file)

GOLDEN = ["cfg1_2genomes", "cfg3_5genomes", "cfg2_sim_1000x5"]


def scipy_labels(edge_index, keep, n):
    """(labels int32 [n] = smallest id of the component, touched bool [n]) by the referee"""
    ei = edge_index.cpu().numpy()
    on = np.ones(ei.shape[1], dtype=bool) if keep is None else (keep.cpu().numpy() != 0)
    s, d = ei[0][on], ei[1][on]
    a = sp.coo_matrix((np.ones(s.size, dtype=np.int8), (s, d)), shape=(n, n))
    _, comp = scipy_components(a, directed=False)
    smallest = np.full(comp.max() + 1 if n else 0, n, dtype=np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    touched = np.zeros(n, dtype=bool)
    touched[s] = True
    touched[d] = True
    return torch.from_numpy(smallest[comp].astype(np.int32)), torch.from_numpy(touched)


def keep_mask(e, density, seed):
    if density <= 0:
        return torch.zeros(e, dtype=torch.bool)
    if density >= 1:
        return torch.ones(e, dtype=torch.bool)
    return torch.rand(e, generator=torch.Generator().manual_seed(seed)) < density


@pytest.mark.parametrize("density", [0.0, 0.03, 0.3, 1.0])
@pytest.mark.parametrize("n,e", [(1, 0), (7, 5), (65, 40), (1000, 700), (5000, 20000)])
def test_cpu_path_equals_scipy(n, e, density):
    ei, _ = random_graph(n, e, seed=n + e)
    keep = keep_mask(e, density, seed=e)
    want, want_touched = scipy_labels(ei, keep, n)
    labels, touched = connected_components(ei, keep, n)
    assert labels.dtype == torch.int32 and touched.dtype == torch.bool
    assert torch.equal(labels, want) and torch.equal(touched, want_touched)
    assert bool((labels.long() <= torch.arange(n)).all())
    assert bool((labels[~touched].long() == torch.arange(n)[~touched]).all())          # untouched: its own label


def test_cpu_keep_none_and_keep_dtypes():
    n, e = 3000, 4000
    ei, _ = random_graph(n, e, seed=3)
    want, want_touched = scipy_labels(ei, None, n)
    labels, touched = connected_components(ei, None, n)
    assert torch.equal(labels, want) and torch.equal(touched, want_touched)
    assert torch.equal(PF.connected_components(ei, num_nodes=n)[0], want)               # the functional re-export
    keep = keep_mask(e, 0.4, seed=1)
    want, want_touched = scipy_labels(ei, keep, n)
    neg_zero = torch.where(keep, torch.ones(e), -torch.zeros(e))                        # -0.0 is zero: not kept
    for k in (keep, keep.int(), keep.float(), keep.double(), keep.long(), keep.to(torch.uint8), neg_zero, 7 * keep.int()):
        labels, touched = connected_components(ei, k, n)
        assert torch.equal(labels, want) and torch.equal(touched, want_touched), k.dtype


def test_cpu_result_is_canonical_and_num_nodes_defaults_to_max_id():
    n, e = 2000, 3000
    ei, _ = random_graph(n, e, seed=5)
    keep = keep_mask(e, 0.5, seed=2)
    labels, touched = connected_components(ei, keep, n)
    p = torch.randperm(e, generator=torch.Generator().manual_seed(0))
    both = torch.cat([ei[:, p], ei[:, p].flip(0), ei[:, :50]], dim=1)                   # shuffled, both directions, duplicates
    l2, t2 = connected_components(both, torch.cat([keep[p], keep[p], keep[:50]]), n)
    assert torch.equal(l2, labels) and torch.equal(t2, touched)
    l3, t3 = connected_components(ei, keep)                                             # N = max id + 1
    m = int(ei.max()) + 1
    assert l3.numel() == m and torch.equal(l3, labels[:m]) and torch.equal(t3, touched[:m])
    empty = connected_components(torch.zeros(2, 0, dtype=torch.int64))
    assert empty[0].numel() == 0 and empty[1].numel() == 0


def test_cpu_self_loop_touches_and_joins_nothing():
    ei = torch.tensor([[4, 1, 2, 6], [4, 2, 1, 5]])
    labels, touched = connected_components(ei, None, 8)
    assert labels.tolist() == [0, 1, 1, 3, 4, 5, 5, 7]
    assert touched.tolist() == [False, True, True, False, True, True, True, False]
    g = homolog_groups(ei, torch.ones(4), 8)
    assert g.num_groups == 3 and g.group_ptr.tolist() == [0, 2, 3, 5] and g.members.tolist() == [1, 2, 4, 5, 6]
    assert g.group_of.tolist() == [-1, 0, 0, -1, 1, 2, 2, -1]
    s = PF.homolog_groups(ei, torch.ones(4), 8, include_singletons=True)
    assert s.num_groups == 6 and s.members.tolist() == [0, 1, 2, 3, 4, 5, 6, 7]
    assert s.group_ptr.tolist() == [0, 1, 3, 4, 5, 7, 8] and s.group_of.tolist() == [0, 1, 1, 2, 3, 4, 4, 5]


@pytest.mark.parametrize("bad", [-1, 9])
def test_cpu_id_outside_the_node_range_raises(bad):
    ei = torch.tensor([[0, 1, bad], [1, 2, 3]])
    with pytest.raises(ValueError, match="outside"):
        connected_components(ei, None, 9)
    with pytest.raises(ValueError, match="outside"):
        connected_components(ei.flip(0), torch.tensor([0, 0, 1]), 9)
    labels, _ = connected_components(ei, torch.tensor([1, 1, 0]), 9)                    # not kept: never looked at
    assert labels.tolist() == [0, 0, 0, 3, 4, 5, 6, 7, 8]
    with pytest.raises(ValueError):
        connected_components(ei, torch.ones(2), 9)                                      # keep of another length
    with pytest.raises(ValueError):
        connected_components(torch.zeros(3, 4, dtype=torch.int64))


def check_groups_invariants(g: Groups, labels, touched, singletons):
    n = labels.numel()
    member = torch.ones(n, dtype=torch.bool) if singletons else touched
    ptr, mem = g.group_ptr, g.members
    assert ptr.dtype == mem.dtype == g.group_of.dtype == torch.int64 and g.labels.dtype == torch.int32
    assert ptr.numel() == g.num_groups + 1 and ptr[0] == 0 and ptr[-1] == mem.numel() == int(member.sum())
    assert bool((ptr[1:] > ptr[:-1]).all())                                             # non-decreasing, and no empty group
    inner = torch.ones(mem.numel(), dtype=torch.bool)
    inner[ptr[:-1]] = False                                                             # positions that continue a group
    assert bool((mem[1:] > mem[:-1])[inner[1:]].all())                                  # ascending inside a group
    first = mem[ptr[:-1]]
    assert bool((first[1:] > first[:-1]).all())                                         # groups by smallest member
    assert torch.equal(first, labels.long()[first])                                     # which is the component's label
    assert torch.equal(g.group_of[mem], torch.repeat_interleave(torch.arange(g.num_groups), ptr[1:] - ptr[:-1]))
    assert bool((g.group_of[~member] == -1).all()) and bool((g.group_of[member] >= 0).all())
    assert torch.equal(labels.long()[mem], first[g.group_of[mem]])                      # a group is one component
    if singletons:
        assert torch.equal(torch.sort(mem).values, torch.arange(n))                     # every node exactly once


@pytest.mark.parametrize("singletons", [False, True])
@pytest.mark.parametrize("density", [0.0, 0.2, 1.0])
def test_groups_invariants(density, singletons):
    n, e = 4000, 5000
    ei, _ = random_graph(n, e, seed=11)
    keep = keep_mask(e, density, seed=4).int()
    labels, touched = scipy_labels(ei, keep, n)
    g = homolog_groups(ei, keep, n, include_singletons=singletons)
    assert torch.equal(g.labels, labels)
    check_groups_invariants(g, labels, touched, singletons)
    if density == 0.0:
        assert g.num_groups == (n if singletons else 0)


@pytest.mark.parametrize("name", GOLDEN)
def test_golden_whole_graph_labels_equal_scipy(name):
    f = load_golden(name)
    ei, y, n = torch.from_numpy(f["whole_edge_index"]), torch.from_numpy(f["whole_y"]), int(f["num_nodes"])
    want, want_touched = scipy_labels(ei, y, n)
    g = homolog_groups(ei, y, n)
    assert torch.equal(g.labels, want)
    check_groups_invariants(g, want, want_touched, False)
    assert g.num_groups > 0
    assert group_agreement(g, g) == dict(groups_pred=g.num_groups, groups_true=g.num_groups, groups_exact=g.num_groups)


def test_simulated_groups_are_ortholog_position_groups():
    """cfg2_sim_1000x5: the groups of the true edges are exactly the ortholog position groups of the generator (the
    components of the fixture's ortholog pairs grp_src / grp_dst): 1000 groups of one gene per genome"""
    f = load_golden("cfg2_sim_1000x5")
    ei, y, n = torch.from_numpy(f["whole_edge_index"]), torch.from_numpy(f["whole_y"]), int(f["num_nodes"])
    position, _ = connected_components(torch.from_numpy(np.stack([f["grp_src"], f["grp_dst"]])), None, n)
    g = homolog_groups(ei, y, n)
    assert torch.equal(g.labels, position) and bool((g.group_of >= 0).all())
    assert g.num_groups == 1000 and bool((g.group_ptr[1:] - g.group_ptr[:-1] == 5).all())
    genome = torch.from_numpy(f["genome_of"]).long()
    assert torch.equal(genome[g.members].view(1000, 5), torch.arange(5).expand(1000, 5))     # one gene of every genome
    assert group_agreement(g, g) == dict(groups_pred=1000, groups_true=1000, groups_exact=1000)
    assert group_agreement(g.labels, g.labels)["groups_exact"] == 1000
    assert group_agreement(g, position) == dict(groups_pred=1000, groups_true=1000, groups_exact=1000)


def test_switching_one_kept_edge_off_in_a_two_genome_group_costs_one_exact_group():
    """cfg1_2genomes, where every group has one gene of each of the two genomes (the simulated fixture has five genomes and
    no group of two).  A group held by a single kept edge is lost with that edge; one held by both directions survives
    the loss of one direction (the predicted graph is undirected) and is lost with the second."""
    f = load_golden("cfg1_2genomes")
    ei, y, n = torch.from_numpy(f["whole_edge_index"]), torch.from_numpy(f["whole_y"]), int(f["num_nodes"])
    g = homolog_groups(ei, y, n)
    G = g.num_groups
    assert bool((g.group_ptr[1:] - g.group_ptr[:-1] == 2).all())
    a, b = g.members[0::2], g.members[1::2]
    key = ei[0] * n + ei[1]
    kept = key[y > 0]
    fwd, bwd = torch.isin(a * n + b, kept), torch.isin(b * n + a, kept)
    single, double = torch.nonzero(fwd ^ bwd).view(-1), torch.nonzero(fwd & bwd).view(-1)
    assert single.numel() > 0 and double.numel() > 0

    def without(edges):
        flipped = y.clone()
        for s, d in edges:
            hit = torch.nonzero((ei[0] == s) & (ei[1] == d) & (y > 0)).view(-1)
            assert hit.numel() == 1
            flipped[hit] = 0
        return homolog_groups(ei, flipped, n)

    k = int(single[0])
    s, d = (int(a[k]), int(b[k])) if bool(fwd[k]) else (int(b[k]), int(a[k]))
    h = without([(s, d)])
    assert h.num_groups == G - 1 and int(h.group_of[s]) == int(h.group_of[d]) == -1
    assert group_agreement(h, g) == dict(groups_pred=G - 1, groups_true=G, groups_exact=G - 1)
    k = int(double[0])
    s, d = int(a[k]), int(b[k])
    assert group_agreement(without([(s, d)]), g) == dict(groups_pred=G, groups_true=G, groups_exact=G)
    assert group_agreement(without([(s, d), (d, s)]), g) == dict(groups_pred=G - 1, groups_true=G, groups_exact=G - 1)


def test_group_agreement_on_hand_made_groups():
    true = homolog_groups(torch.tensor([[0, 1, 3, 5, 6], [1, 2, 4, 6, 7]]), torch.ones(5), 10)   # {0,1,2} {3,4} {5,6,7}
    pred = homolog_groups(torch.tensor([[0, 1, 3, 5, 8], [1, 2, 4, 6, 9]]), torch.ones(5), 10)   # {0,1,2} {3,4} {5,6} {8,9}
    assert group_agreement(pred, true) == dict(groups_pred=4, groups_true=3, groups_exact=2)
    assert group_agreement(true, pred) == dict(groups_pred=3, groups_true=4, groups_exact=2)
    merged = homolog_groups(torch.tensor([[0, 1, 2, 5, 6], [1, 2, 3, 6, 7]]), torch.ones(5), 10)  # {0,1,2,3} {5,6,7}
    assert group_agreement(merged, true) == dict(groups_pred=2, groups_true=3, groups_exact=1)
    # label vectors: every node is a member, so the isolated nodes 8 and 9 of `true` are groups of one
    assert group_agreement(true.labels, true) == dict(groups_pred=5, groups_true=3, groups_exact=3)
    assert group_agreement(pred.labels, true.labels) == dict(groups_pred=5, groups_true=5, groups_exact=2)  # {7} is new
    with pytest.raises(ValueError):
        group_agreement(true.labels, true.labels[:5])


def test_write_groups_file(tmp_path):
    f = load_golden("cfg1_2genomes")
    n = int(f["num_nodes"])
    names = [f"gene_{i:05d}" for i in range(n)]
    ds = SimpleNamespace(edge_index=torch.from_numpy(f["whole_edge_index"]), x=torch.from_numpy(f["whole_x"]),
                         gene_ids_lst=names)
    y = torch.from_numpy(f["whole_y"])
    path = tmp_path / "out" / "groups.csv"
    g = write_groups_file(ds, y, path=str(path))
    text = path.read_text()
    lines = text.split("\n")
    assert lines[-1] == "" and len(lines) - 1 == g.num_groups == text.count("\n")       # every line ends in a newline
    for k, line in enumerate(lines[:-1]):
        cells = line.split(", ")
        assert cells[0] == f"group_{k}"
        assert cells[1:] == [names[v] for v in g.members[g.group_ptr[k]:g.group_ptr[k + 1]].tolist()]
    # without gene names the integer ids are written; the node count may come from num_nodes
    plain = SimpleNamespace(edge_index=ds.edge_index, num_nodes=n)
    g2 = write_groups_file(plain, y.int(), path=str(tmp_path / "plain.csv"))
    assert torch.equal(g2.members, g.members) and torch.equal(g2.group_ptr, g.group_ptr)
    back = [[int(c) for c in line.split(", ")[1:]] for line in (tmp_path / "plain.csv").read_text().splitlines()]
    assert back == [g.members[g.group_ptr[k]:g.group_ptr[k + 1]].tolist() for k in range(g.num_groups)]
    import inspect
    assert inspect.signature(write_groups_file).parameters["path"].default.endswith("holiest_of_all_tables.csv")


def test_the_reference_loop_cannot_group_which_is_why_semantics_are_defined_here():
    """The control flow of the reference's write_groups_file (src/postprocessing.py:11-28), restated: the scan over the
    existing sets adds the edge to the FIRST set it meets and stops, two sets are never merged, and the append behind
    the scan runs for every positive edge.  On the path 0-1, 2-3, 1-2 — one component — it leaves several sets."""
    def reference_sets(edges, labels):
        sets = []
        for label, (a, b) in zip(labels, edges):
            if not label:
                continue
            for node_set in sets:
                if not sets:                    # never true inside a loop over `sets`
                    sets.append({a, b})
                if node_set & {a, b}:
                    node_set.update({a, b})
                    break
            sets.append({a, b})                 # no `else`: also when a set matched
        return sets

    edges = [(0, 1), (2, 3), (1, 2)]
    sets = reference_sets(edges, [1, 1, 1])
    assert len(sets) > 1                                                            # one component, several sets
    assert {0, 1, 2, 3} not in sets                                                 # and none of them is the component
    g = homolog_groups(torch.tensor(edges).t(), torch.ones(3), 4)
    assert g.num_groups == 1 and g.members.tolist() == [0, 1, 2, 3] and g.labels.tolist() == [0, 0, 0, 0]


F = 0x7f0000100000
E_BADARG, E_TOOLARGE = -1, -2


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: only where a missing check cannot reach a GPU")
def test_components_entry_point_refuses_bad_arguments():
    fn = _lib.load().pangnn_components_i32
    N, E = 1000, 5000
    assert fn(None, F, F, 4, E, N, F, F, F, None) == E_BADARG               # null src
    assert fn(F, None, F, 4, E, N, F, F, F, None) == E_BADARG               # null dst
    assert fn(F, F, F, 4, E, N, None, F, F, None) == E_BADARG               # null labels
    assert fn(F, F, F, 4, E, N, F, F, None, None) == E_BADARG               # null status
    assert fn(F, F, F, 4, 0, 0, None, None, None, None) == E_BADARG         # status is written even for an empty graph
    assert fn(F, F, F, 4, -1, N, F, F, F, None) == E_BADARG                 # negative sizes
    assert fn(F, F, F, 4, E, -1, F, F, F, None) == E_BADARG
    for itemsize in (-1, 2, 3, 8):
        assert fn(F, F, F, itemsize, E, N, F, F, F, None) == E_BADARG       # keep_itemsize outside {0, 1, 4}
    assert fn(F, F, None, 1, E, N, F, F, F, None) == E_BADARG               # an item size without keep
    assert fn(F, F, None, 4, E, N, F, F, F, None) == E_BADARG
    assert b"pangnn_components_i32" in _lib.load().pangnn_last_error()
    assert fn(F, F, F, 4, E, 1 << 31, F, F, F, None) == E_TOOLARGE          # int32 labels
    assert fn(F, F, None, 0, E, (1 << 31) + 5, F, None, F, None) == E_TOOLARGE
    assert b"pangnn_components_i32" in _lib.load().pangnn_last_error()
