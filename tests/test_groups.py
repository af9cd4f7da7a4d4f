"""Components of the kept edges on the MI355X (csrc/components.hip, pangnn_amd/postprocessing.py): the HIP labels are held
bit for bit to the CPU path (itself held to scipy in test_groups_host.py), a subset also to scipy directly.  The shapes
are those at which the lock-free union-find can go wrong: the deepest trees the hook pass can build (a long path in three
edge orders), one root that every compare-and-swap lands on (a star, onto the smallest and onto the largest id), two
big trees joined by the last edge, a random graph at each width of `keep`, ids outside the node range.  There is no
tolerance: every comparison is torch.equal."""
import pytest
import torch

from conftest import load_golden, random_graph
from test_groups_host import check_groups_invariants, keep_mask, scipy_labels
from pangnn_amd.postprocessing import (_enqueue_components, connected_components, group_agreement, homolog_groups)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def on_device(edge_index, keep, n):
    labels, touched = connected_components(edge_index.to(DEV), None if keep is None else keep.to(DEV), n)
    assert labels.is_cuda and labels.dtype == torch.int32 and touched.dtype == torch.bool
    return labels.cpu(), touched.cpu()


def same_as_cpu(edge_index, keep, n, referee=False):
    want = connected_components(edge_index, keep, n)
    got = on_device(edge_index, keep, n)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    if referee:
        ref = scipy_labels(edge_index, keep, n)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    return want


def test_degenerate_sizes():
    none = torch.zeros(2, 0, dtype=torch.int64)
    for n in (1, 65):
        labels, touched = on_device(none, None, n)
        assert labels.tolist() == list(range(n)) and not bool(touched.any())
        labels, touched = on_device(none, torch.zeros(0, dtype=torch.int32), n)
        assert labels.tolist() == list(range(n)) and not bool(touched.any())
    labels, touched = on_device(none, None, 0)
    assert labels.numel() == 0 and touched.numel() == 0
    ei, _ = random_graph(300, 1000, seed=1)
    for keep in (torch.zeros(1000, dtype=torch.bool), torch.zeros(1000, dtype=torch.int32), torch.zeros(1000)):
        labels, touched = on_device(ei, keep, 300)                       # edges, none of them kept
        assert labels.tolist() == list(range(300)) and not bool(touched.any())
    g = homolog_groups(ei.to(DEV), torch.zeros(1000, dtype=torch.int32, device=DEV), 300)
    assert g.num_groups == 0 and g.members.numel() == 0 and g.group_ptr.tolist() == [0] and bool((g.group_of == -1).all())


PATH = 100_000


def path_edges():
    return torch.stack([torch.arange(PATH - 1), torch.arange(1, PATH)])


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_long_path_in_every_edge_order(order):
    ei = path_edges()
    if order == "descending":
        ei = ei.flip(1)
    elif order == "shuffled":
        ei = ei[:, torch.randperm(PATH - 1, generator=torch.Generator().manual_seed(0))]
    labels, touched = on_device(ei, None, PATH)
    assert not bool(labels.any()) and bool(touched.all())               # one component, smallest id 0
    # the same path with the last node left out of the graph's edges and two isolated nodes behind it
    labels, touched = on_device(ei, (ei.max(0).values < PATH - 1), PATH + 2)
    assert not bool(labels[:PATH - 1].any()) and labels[PATH - 1:].tolist() == [PATH - 1, PATH, PATH + 1]
    assert touched.tolist() == [True] * (PATH - 1) + [False] * 3


def test_long_path_over_shuffled_node_ids():
    perm = torch.randperm(PATH, generator=torch.Generator().manual_seed(1))
    same_as_cpu(perm[path_edges()], None, PATH, referee=True)


def test_path_with_every_edge_in_both_directions_and_twice():
    ei = path_edges()
    ei = torch.cat([ei, ei.flip(0), ei.flip(1), ei.flip(0).flip(1)], dim=1)
    keep = torch.ones(ei.shape[1], dtype=torch.int32)
    labels, touched = on_device(ei, keep, PATH)
    assert not bool(labels.any()) and bool(touched.all())


@pytest.mark.parametrize("hub", ["smallest", "largest"])
def test_star_every_join_lands_on_one_root(hub):
    n = 200_001
    leaves = torch.arange(1, n) if hub == "smallest" else torch.arange(0, n - 1)
    centre = torch.full_like(leaves, 0 if hub == "smallest" else n - 1)
    for ei in (torch.stack([leaves, centre]), torch.stack([centre, leaves])):
        labels, touched = on_device(ei, None, n)
        assert not bool(labels.any()) and bool(touched.all())


def test_two_big_components_joined_by_the_last_edge():
    half = 50_000
    a = torch.stack([torch.arange(half - 1), torch.arange(1, half)])
    p = torch.randperm(2 * (half - 1), generator=torch.Generator().manual_seed(2))
    ei = torch.cat([a, a + half], dim=1)[:, p]
    labels, _ = on_device(ei, None, 2 * half)
    assert torch.equal(labels, torch.cat([torch.zeros(half), torch.full((half,), half)]).to(torch.int32))
    joined = torch.cat([ei, torch.tensor([[2 * half - 1], [half - 1]])], dim=1)
    labels, touched = on_device(joined, None, 2 * half)
    assert not bool(labels.any()) and bool(touched.all())


@pytest.fixture(scope="module")
def big_random():
    n, e = 200_000, 2_000_000
    ei, _ = random_graph(n, e, seed=7)
    keep = keep_mask(e, 0.03, seed=8)
    return n, ei, keep, connected_components(ei, keep, n), scipy_labels(ei, keep, n)


@pytest.mark.parametrize("dtype", [torch.bool, torch.int32, torch.uint8, torch.float32])
def test_random_graph_three_percent_kept_at_every_keep_width(big_random, dtype):
    n, ei, keep, want, ref = big_random
    assert torch.equal(want[0], ref[0]) and torch.equal(want[1], ref[1])
    d_ei, d_keep = ei.to(DEV), keep.to(DEV).to(dtype)
    first = connected_components(d_ei, d_keep, n)
    second = connected_components(d_ei, d_keep, n)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])            # run twice: identical
    assert torch.equal(first[0].cpu(), want[0]) and torch.equal(first[1].cpu(), want[1])
    # keep starting off a 16-byte boundary and an edge count that is no multiple of 16: the one-by-one reads
    odd = slice(3, ei.shape[1] - 6)
    w = connected_components(ei[:, odd], keep[odd], n)
    got = connected_components(d_ei[:, odd], d_keep[odd], n)
    assert torch.equal(got[0].cpu(), w[0]) and torch.equal(got[1].cpu(), w[1])


def test_random_graph_every_edge_kept(big_random):
    n, ei, _, _, _ = big_random
    want = same_as_cpu(ei, None, n, referee=True)
    got = on_device(ei[:, torch.randperm(ei.shape[1], generator=torch.Generator().manual_seed(3))], None, n)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])                    # the order of edges changes nothing


def test_golden_simulated_graph_groups_and_agreement():
    f = load_golden("cfg2_sim_1000x5")
    ei, y, n = torch.from_numpy(f["whole_edge_index"]), torch.from_numpy(f["whole_y"]), int(f["num_nodes"])
    want, ref = homolog_groups(ei, y, n), scipy_labels(ei, y, n)
    for singletons in (False, True):
        cpu = homolog_groups(ei, y, n, include_singletons=singletons)
        got = homolog_groups(ei.to(DEV), y.to(DEV), n, include_singletons=singletons)
        assert got.members.is_cuda and got.num_groups == cpu.num_groups
        for a, b in zip(got[:4], cpu[:4]):
            assert torch.equal(a.cpu(), b)
        check_groups_invariants(Groups_cpu(got), ref[0], ref[1], singletons)
    got = homolog_groups(ei.to(DEV), y.to(DEV), n)
    # a prediction that loses some true edges and adds some false ones, against the true groups, on both devices
    pred = (y > 0) ^ (keep_mask(y.numel(), 0.02, seed=5))
    p_cpu, p_dev = homolog_groups(ei, pred, n), homolog_groups(ei.to(DEV), pred.to(DEV), n)
    assert torch.equal(p_dev.labels.cpu(), p_cpu.labels)
    agree = group_agreement(p_cpu, want)
    assert group_agreement(p_dev, got) == agree and 0 < agree["groups_exact"] < want.num_groups
    assert group_agreement(got, got) == dict(groups_pred=1000, groups_true=1000, groups_exact=1000)
    assert group_agreement(p_dev.labels, got.labels) == group_agreement(p_cpu.labels, want.labels)


def Groups_cpu(g):
    return type(g)(*[t.cpu() for t in g[:4]], g.num_groups)


@pytest.mark.parametrize("bad", ["N", "-1"])
@pytest.mark.parametrize("dtype", [None, torch.bool, torch.int32])
def test_id_outside_the_node_range_is_skipped_and_reported(bad, dtype):
    """a validation path, not a fault: the kernel never turns the id into an address"""
    n, e = 5000, 20000
    ei, _ = random_graph(n, e, seed=9)
    keep = None if dtype is None else torch.ones(e, dtype=dtype)
    want = connected_components(ei, keep, n)
    broken = ei.clone()
    at = 12345
    broken = torch.cat([ei[:, :at], torch.tensor([[n if bad == "N" else -1], [17]]), ei[:, at:]], dim=1)
    if bad == "-1":
        broken[:, at] = broken[:, at].flip(0)                               # the bad id as the target
    bkeep = None if keep is None else torch.ones(e + 1, dtype=dtype)
    with pytest.raises(ValueError, match="outside"):
        connected_components(broken.to(DEV), None if bkeep is None else bkeep.to(DEV), n)
    labels, touched, status = _enqueue_components(broken.to(DEV), None if bkeep is None else bkeep.to(DEV), n)
    assert int(status.item()) != 0
    assert torch.equal(labels.cpu(), want[0]) and torch.equal(touched.cpu().bool(), want[1])   # as without that edge
    if bkeep is not None:                                                   # not kept: never read, nothing to report
        bkeep[at] = 0
        labels, touched = connected_components(broken.to(DEV), bkeep.to(DEV), n)
        assert torch.equal(labels.cpu(), want[0]) and torch.equal(touched.cpu(), want[1])


def test_predictions_to_groups_end_to_end():
    import pangnn_amd
    from pangnn_amd import functional as PF
    from pangnn_amd.simulate import simulate_graph
    g = simulate_graph(500, 6, 0.2, 10, 2, seed=0, device=DEV)
    n = g.x.shape[0]
    torch.manual_seed(0)
    model = pangnn_amd.AlternateGCN(torch.device(DEV), None, False, dims=[64, 128])
    model.eval()
    with torch.no_grad():
        th = float(torch.sigmoid(model(g).float()).quantile(0.9))           # a tenth of the edges predicted
    pred, _, stats = pangnn_amd.predict_homolog_genes(model, None, g, binary_th=th)
    assert pred.dtype == torch.int32 and 0 < int(pred.sum()) < pred.numel()
    got = PF.homolog_groups(g.edge_index, pred, n)
    want = homolog_groups(g.edge_index.cpu(), pred.cpu(), n)
    assert got.num_groups == want.num_groups > 0
    for a, b in zip(got[:4], want[:4]):
        assert a.is_cuda and torch.equal(a.cpu(), b)
    true = homolog_groups(g.edge_index, g.y, n)
    assert group_agreement(got, true) == group_agreement(want, Groups_cpu(true))
