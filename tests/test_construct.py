"""The product's graph construction (pangnn_amd/construct.py, subgraphs.py, simulate.py) against fixtures built by
the reference's own code (tests/golden/*.npz), on BOTH devices: the `cpu` legs run in the CPU suite, the `cuda`
legs carry the gpu mark and run the same programs where bench.py and the product run them (device sort / unique /
searchsorted and the segmented softmax -> Q-score HIP kernel).  Ids and labels: bit-exact on both.  fp32 weights:
bit-exact on the CPU; on the device the float64 exp / log / log10 of the GPU math library may differ from the host
libm in the last place, which can move a value across an fp32 rounding boundary: at most 1 fp32 ulp, on at most
0.1 % of the edges (asserted below; in practice 0)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from pangnn_amd import construct, simulate, subgraphs

FIXTURES = ["sim_200x4", "cfg1_2genomes", "cfg2_sim_1000x5", "cfg3_5genomes"]
DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]


def T(f, k, device="cpu"):
    return torch.from_numpy(f[k]).to(device)


def N(t):
    return t.detach().cpu().numpy()


def assert_weights(got, want, device):
    """fp32 edge weights: identical on the CPU; within 1 ulp on <= 0.1 % of the entries on the device"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    if device == "cpu":
        assert np.array_equal(got, want)
        return
    bad = got != want
    if bad.any():
        ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1 and bad.mean() <= 1e-3, (int(ulp.max()), float(bad.mean()))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("name", FIXTURES)
def test_whole_graph_construction_is_bit_exact(name, device):
    f = load_golden(name)
    g = construct.build_from_raw(int(f["num_nodes"]), T(f, "raw_src", device), T(f, "raw_dst", device),
                                 T(f, "raw_score", device), T(f, "genome_of", device).long(),
                                 pair_src=T(f, "grp_src", device), pair_dst=T(f, "grp_dst", device))
    assert g.edge_index.device.type == device
    o = np.lexsort((f["whole_edge_index"][1], f["whole_edge_index"][0]))
    assert np.array_equal(N(g.edge_index), f["whole_edge_index"][:, o])               # bit-exact edge_index
    assert np.array_equal(N(g.neighbour_edge_index), f["whole_neighbour_edge_index"])
    assert np.array_equal(N(g.y), f["whole_y"][o])
    assert_weights(N(g.edge_attr), f["whole_edge_attr"][o], device)
    assert np.array_equal(N(g.x), f["whole_x"])


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("name", FIXTURES)
def test_normalized_relation_matches_reference_float64(name, device):
    """normalize_sim_scores alone, in float64 (the fixture holds the reference's float64 weights): the CPU torch
    program and the device kernel (pangnn_softmax_qscore_f64: one wavefront per (source, genome) segment)"""
    f = load_golden(name)
    s, d, w = construct.normalize_sim_scores(T(f, "flt_src", device), T(f, "flt_dst", device), T(f, "flt_score", device),
                                             T(f, "genome_of", device).long())
    n = int(f["num_nodes"])
    o1 = np.argsort(N(s) * n + N(d), kind="stable")
    o2 = np.argsort(f["nrm_src"] * n + f["nrm_dst"], kind="stable")
    assert np.array_equal(N(s)[o1], f["nrm_src"][o2]) and np.array_equal(N(d)[o1], f["nrm_dst"][o2])
    got, want = N(w)[o1], f["nrm_weight"][o2]
    assert got.dtype == np.float64
    # float64.  q = -10 log10(1 - p) amplifies a relative error d of p by p / (1 - p) <= 1e8 (the clip at epsilon = 1e-8):
    # |dq| <= 10 / ln 10 * p / (1 - p) * d.  CPU: the host's exp / log / log10 are picked at run time by its processor and
    # can be an ulp from those of the host that built the fixture (5.5e-9 at q = 71.6, 1 - p = 9e-8, between two x86-64
    # hosts), so each weight is held to its own bound with d = 4 eps, 1 - p taken from the fixture's q: ~1e-13 away from
    # the clip, 4e-8 at q = 71.6.  Device: exp / log of the GPU math library are a few ulp from libm: |dq| <= 4.35 * 1e8 * d
    # ~ 1e-7 for d ~ 2 ulp.  The fp32 weights the graph carries have an ulp of 7.6e-6 at 81, so they still come out
    # identical (test above).
    if device == "cpu":
        one_minus_p = 10.0 ** (-(want - 1.0) / 10.0)
        tol = 1e-13 + 10.0 / np.log(10.0) * (1.0 - one_minus_p) / one_minus_p * 4 * np.finfo(np.float64).eps
        assert np.allclose(got, want, rtol=1e-13, atol=tol)
    else:
        assert np.allclose(got, want, rtol=5e-7, atol=5e-7)


def _groups_from_pairs(f):
    """ortholog groups as (group id, member) arrays: a key gene and its members form one group"""
    ks, ms = f["grp_src"], f["grp_dst"]
    n = int(f["num_nodes"])
    gmin = np.arange(n)
    np.minimum.at(gmin, ks, ms)
    np.minimum.at(gmin, ks, ks)
    genes = np.unique(ks)
    rep = gmin[genes]
    # a group's representative is its smallest member; every member maps to it after one more hop
    rep = np.minimum(rep, gmin[rep])
    _, gid = np.unique(rep, return_inverse=True)
    return torch.from_numpy(gid.astype(np.int64)), torch.from_numpy(genes.astype(np.int64))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("name,subset", [("sim_200x4", False), ("cfg1_2genomes", True), ("cfg3_5genomes", True),
                                         ("cfg2_sim_1000x5", False)])
def test_subgraphs_equal_the_reference_sets(name, subset, device):
    """node set, similarity edges (+ weight, label) and neighbour edges of every reference sub-graph, in
    GLOBAL ids (the reference's local numbering is CPython set order)"""
    f = load_golden(name)
    n = int(f["num_nodes"])
    gid, mem = _groups_from_pairs(f)
    ds = subgraphs.build_subgraphs(n, T(f, "nrm_src", device), T(f, "nrm_dst", device), T(f, "nrm_weight", device),
                                   gid.to(device), mem.to(device), neighbours=1,
                                   pair_src=T(f, "grp_src", device), pair_dst=T(f, "grp_dst", device),
                                   require_edges_ge_members=subset)
    assert ds.node_global.device.type == device
    mine = {}          # node set -> candidate sub-graphs (two groups can span the same node set)
    for i in range(len(ds)):
        nodes = N(ds.node_global[int(ds.node_off[i]):int(ds.node_off[i + 1])])
        mine.setdefault(tuple(sorted(nodes.tolist())), []).append(i)
    no, eo, bo = f["sub_node_off"], f["sub_edge_off"], f["sub_nb_off"]
    total = int(f["n_train"]) + int(f["n_val"])
    assert len(ds) >= len(no) - 1
    if len(no) - 1 == total:                       # fixture holds every train+val graph (70 % + 15 %)
        assert abs(len(ds) * 0.85 - total) <= 2
    for k in range(len(no) - 1):
        glob = f["sub_global_node"][no[k]:no[k + 1]]
        key = tuple(sorted(glob.tolist()))
        assert key in mine, f"reference sub-graph {k} (|V|={len(key)}) has no counterpart"
        ref_nb = glob[f["sub_neighbour_edge_index"][:, bo[k]:bo[k + 1]]]
        ref_nb_set = set(map(tuple, ref_nb.T.tolist()))
        assert len(ref_nb_set) == ref_nb.shape[1]                       # reference de-duplicates
        match = None
        for i in mine[key]:            # same node set: the neighbour edges tell the groups apart
            b = ds.graph(i)
            mg = N(ds.node_global[int(ds.node_off[i]):int(ds.node_off[i + 1])])
            my_nb = mg[N(b.neighbour_edge_index)]
            if my_nb.shape == ref_nb.shape and set(map(tuple, my_nb.T.tolist())) == ref_nb_set:
                match = i
                break
        assert match is not None, f"no sub-graph with the neighbour edges of reference sub-graph {k}"
        mine[key].remove(match)        # one-to-one
        ref_e = glob[f["sub_edge_index"][:, eo[k]:eo[k + 1]]]
        my_e = mg[N(b.edge_index)]
        ro, mo = np.lexsort((ref_e[1], ref_e[0])), np.lexsort((my_e[1], my_e[0]))
        assert np.array_equal(ref_e[:, ro], my_e[:, mo])
        assert np.array_equal(f["sub_edge_attr"][eo[k]:eo[k + 1]][ro], N(b.edge_attr)[mo])
        assert np.array_equal(f["sub_y"][eo[k]:eo[k + 1]][ro], N(b.y)[mo])


@pytest.mark.parametrize("device", DEVICES)
def test_subgraph_batches_are_disjoint_unions(device):
    f = load_golden("cfg1_2genomes")
    gid, mem = _groups_from_pairs(f)
    ds = subgraphs.build_subgraphs(int(f["num_nodes"]), T(f, "nrm_src", device), T(f, "nrm_dst", device),
                                   T(f, "nrm_weight", device), gid.to(device), mem.to(device),
                                   pair_src=T(f, "grp_src", device), pair_dst=T(f, "grp_dst", device),
                                   require_edges_ge_members=True)
    b = ds.batch(3, 35)
    assert b.num_graphs == 32 and b.x.shape[0] == int(b.ptr[-1])
    assert int(b.edge_index.min()) >= 0 and int(b.edge_index.max()) < b.x.shape[0]
    # every edge stays inside its own sub-graph
    gb = b.batch
    assert torch.equal(gb[b.edge_index[0]], gb[b.edge_index[1]])
    assert torch.equal(gb[b.neighbour_edge_index[0]], gb[b.neighbour_edge_index[1]])
    one = ds.graph(5)
    e0 = int(ds.edge_off[5] - ds.edge_off[3])
    off = int(ds.node_off[5] - ds.node_off[3])
    assert torch.equal(b.edge_index[:, e0:e0 + one.edge_index.shape[1]], one.edge_index + off)


@pytest.mark.gpu
def test_collation_kernel_equals_the_index_op_collation():
    """pangnn_collate_subgraphs (one launch) against the torch index ops the CPU path uses: every field of the batch,
    first / middle / last / single-graph / short final batches"""
    ds = simulate.simulate_subgraph_dataset(300, 4, 0.3, 10, 2, seed=3, device="cuda")
    n = len(ds)
    for i0, i1 in [(0, 32), (5, 37), (n - 7, n + 20), (11, 12), (0, n)]:
        a = ds.batch(i0, i1)
        old, subgraphs.COLLATE_KERNEL = subgraphs.COLLATE_KERNEL, False
        try:
            b = ds.batch(i0, i1)
        finally:
            subgraphs.COLLATE_KERNEL = old
        assert a.num_graphs == b.num_graphs and a._pangnn_hints == b._pangnn_hints
        for f in ("x", "edge_index", "edge_attr", "y", "neighbour_edge_index", "ptr", "batch"):
            x, y = getattr(a, f), getattr(b, f)
            assert x.dtype == y.dtype and x.shape == y.shape and x.is_contiguous() and torch.equal(x, y), f


# ---------------------------------------------------------------- simulator: distributional parity
@pytest.mark.parametrize("device", DEVICES)
def test_simulator_matches_reference_statistics(device):
    """the reference never seeds its RNG, so compare laws, not samples (cfg 2: 1000 x 5, frac 0.3)"""
    f = load_golden("cfg2_sim_1000x5")
    g = simulate.simulate_graph(1000, 5, 0.3, 10, 2, seed=1, device=device)
    assert g.edge_index.device.type == device
    assert g.num_nodes == 5000 and g.neighbour_edge_index.shape[1] == 14998
    e_ref = f["whole_edge_index"].shape[1]
    # the edge count is a sum of clipped negative binomials: 2.6 % seed-to-seed spread (and the reference fixture is
    # one draw of the same law) -> one seed within 3 sigma, the mean over six seeds within 3 %
    assert abs(g.edge_index.shape[1] - e_ref) / e_ref < 0.08
    mean_e = np.mean([simulate.simulate_graph(1000, 5, 0.3, 10, 2, seed=s_, device=device).edge_index.shape[1]
                      for s_ in range(6)])
    assert abs(mean_e - e_ref) / e_ref < 0.03
    assert abs(float(g.y.mean()) - float(f["whole_y"].mean())) < 0.01
    assert abs(float(g.edge_attr.mean()) - float(f["whole_edge_attr"].mean())) / float(f["whole_edge_attr"].mean()) < 0.05
    assert float(g.edge_attr.min()) >= 1.0 and float(g.edge_attr.max()) <= 81.0001
    deg = torch.bincount(g.edge_index[1], minlength=5000).float().cpu()
    dref = np.bincount(f["whole_edge_index"][1], minlength=5000)
    assert abs(float(deg.median()) - np.median(dref)) <= 1
    assert 0.6 < float(deg.quantile(0.99)) / np.quantile(dref, 0.99) < 1.6
    # structure: no self loops; after remove_trivial_cases only adjacent genomes stay linked; the RAW
    # relation is symmetric with one score per pair (simulate.py:166-167,188-189)
    s, d = g.edge_index
    assert not bool((s == d).any())
    assert int(((s // 1000) - (d // 1000)).abs().max()) == 1
    raw = simulate.simulate_raw(1000, 5, 0.3, 10, 2, seed=1, device=device)
    fwd = torch.stack([raw.src * 5000 + raw.dst, raw.score.long()], 1)
    bwd = torch.stack([raw.dst * 5000 + raw.src, raw.score.long()], 1)
    assert torch.equal(fwd[torch.argsort(fwd[:, 0])], bwd[torch.argsort(bwd[:, 0])])
    assert torch.unique(fwd[:, 0]).numel() == fwd.shape[0]             # a dict: one score per ordered pair


@pytest.mark.parametrize("device", DEVICES)
def test_simulator_is_seeded(device):
    a = simulate.simulate_graph(300, 4, 0.3, 10, 2, seed=7, device=device)
    b = simulate.simulate_graph(300, 4, 0.3, 10, 2, seed=7, device=device)
    c = simulate.simulate_graph(300, 4, 0.3, 10, 2, seed=8, device=device)
    assert torch.equal(a.edge_index, b.edge_index) and torch.equal(a.edge_attr, b.edge_attr)
    assert a.edge_index.shape != c.edge_index.shape or not torch.equal(a.edge_index, c.edge_index)


# ---------------------------------------------------------------- rank-local generation (config 5: no rank holds the graph)
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("balanced", [False, True], ids=["equal-nodes", "equal-edges"])
@pytest.mark.parametrize("n,G,frac,world", [(300, 5, 0.3, 2), (1000, 5, 0.3, 3), (400, 7, 0.2, 4), (250, 20, 0.2, 8)])
def test_rank_local_generation_equals_partition_of_the_whole_graph(n, G, frac, world, device, balanced):
    """simulate_shard draws only the genome pairs around the rank's node range; its shard must be the one
    dist.partition_graph cuts out of the whole graph of the same seed — edge ids, labels and neighbour edges
    bit-exact, fp32 weights bit-exact on the CPU and within the construction test's device bound on the GPU."""
    from pangnn_amd.dist import balanced_bounds, partition_graph
    g = simulate.simulate_graph(n, G, frac, 10, 2, seed=5, device=device)
    bounds = balanced_bounds(n, G, world) if balanced else None
    tot = pos = 0
    for r in range(world):
        ref = partition_graph(g, r, world, bounds)
        sh = simulate.simulate_shard(n, G, frac, 10, 2, seed=5, device=device, rank=r, world=world, bounds=bounds)
        assert sh.edge_index.device.type == device
        assert torch.equal(ref.edge_index, sh.edge_index) and torch.equal(ref.y, sh.y)
        assert torch.equal(ref.neighbour_edge_index, sh.neighbour_edge_index) and torch.equal(ref.x, sh.x)
        assert_weights(N(sh.edge_attr), N(ref.edge_attr), device)
        assert (sh.n_local, sh.lo, sh.hi, sh.n_global) == (ref.n_local, ref.lo, ref.hi, ref.n_global)
        tot += sh.e_sim_local
        pos += sh.n_pos_local
    assert tot == g.edge_index.shape[1] and pos == int(g.y.sum())


@pytest.mark.parametrize("n,G,world", [(2000, 20, 8), (1500, 7, 4), (1000, 50, 8), (3000, 5, 2), (3000, 3, 3)])
def test_balanced_bounds_give_every_rank_the_same_share_of_edges(n, G, world):
    """dist.balanced_bounds: node ranges from the genome adjacency alone (no edge exists yet when a rank needs its
    range).  Ranges are contiguous, cover every node once, and the in-edges they own differ by a few per cent, where
    equal node ranges leave the two end ranks short (they hold an end genome, which has one neighbour genome)."""
    from pangnn_amd.dist import balanced_bounds
    b = balanced_bounds(n, G, world)
    assert len(b) == world + 1 and b[0] == 0 and b[-1] == n * G and all(b[i] <= b[i + 1] for i in range(world))
    # exact in expectation: every node weighs the number of genomes adjacent to its own (1 at the ends, else 2)
    wnode = torch.tensor([1 if (k == 0 or k == G - 1) else 2 for k in range(G)], dtype=torch.int64).repeat_interleave(n)
    load = torch.tensor([int(wnode[b[r]:b[r + 1]].sum()) for r in range(world)])
    assert int(load.max() - load.min()) <= 2 * world        # whole-node granularity
    # and on a drawn graph (per-pair edge counts are heavy-tailed negative-binomial sums: +-5 % at these sizes, 1 % at
    # cfg 4; equal node ranges are short by 1 / (2 - 2 / G) on the end ranks whatever the size)
    g = simulate.simulate_graph(n, G, 0.2, 10, 2, seed=3, device="cpu")
    dst = g.edge_index[1]
    bal = torch.tensor([int(((dst >= b[r]) & (dst < b[r + 1])).sum()) for r in range(world)], dtype=torch.float64)
    nl = (n * G + world - 1) // world
    eq = torch.tensor([int(((dst >= r * nl) & (dst < (r + 1) * nl)).sum()) for r in range(world)], dtype=torch.float64)
    assert float(bal.max() / bal.mean()) < 1.15
    if (G, world) == (3, 3):              # one genome per rank: the middle one has twice the in-edges
        assert float(eq.max() / eq.mean()) > 1.4
    assert balanced_bounds(n, G, 1) == [0, n * G]


def test_padded_batch_shapes_are_host_arithmetic_on_the_offset_tables():
    """SubGraphDataset.padded_spec / fits (train.ReplayedFreshStep's fixed shapes): the worst case holds ANY 32 sub-graphs,
    the slack form holds slack x the mean batch, and `fits` agrees with the sums (no GPU involved)"""
    from pangnn_amd import simulate
    ds = simulate.simulate_subgraph_dataset(200, 4, 0.3, 10, 2, seed=0, device="cpu")
    h = ds._host()
    sizes = lambda off: [off[i + 1] - off[i] for i in range(ds.num_graphs)]     # noqa: E731
    g, n, e, b = ds.padded_spec(32)
    assert g == 32 and n == sum(sorted(sizes(h.node))[-32:]) + 1 and e == sum(sorted(sizes(h.edge))[-32:])
    assert b == sum(sorted(sizes(h.nb))[-32:])
    gen = torch.Generator().manual_seed(0)
    for _ in range(20):
        ids = torch.randperm(ds.num_graphs, generator=gen)[:32].tolist()
        assert ds.fits((g, n, e, b), ids)
    tight = ds.padded_spec(32, slack=1.3)
    assert tight[1] <= n and tight[2] <= e and tight[3] <= b and tight[2] >= 32 * sum(sizes(h.edge)) / ds.num_graphs
    big = sorted(range(ds.num_graphs), key=lambda i: -(h.edge[i + 1] - h.edge[i]))[:32]
    assert ds.fits((g, n, e, b), big) and not ds.fits(tight, big) and not ds.fits((g, n, e, b), list(range(33)))
    sub = ds.padded_spec(8, graphs=range(20))
    assert sub[0] == 8 and sub[2] == sum(sorted(sizes(h.edge)[:20])[-8:])


@pytest.mark.parametrize("name", ["cfg1_2genomes", "cfg3_5genomes", "cfg2_sim_1000x5"])
def test_flat_dataset_from_reference_built_subgraphs_collates_like_pyg(name):
    """SubGraphDataset.from_data_list over the sub-graphs AS THE REFERENCE BUILT THEM (golden fixtures: its own local node
    numbering and edge order): every mini-batch of the flat data set is PyG's Batch.from_data_list of the same sub-graphs
    (oracle.collate: cumulative node offsets on the index tensors, concatenation of everything else), entry for entry."""
    from conftest import sub_graphs_from_golden
    from oracle import gcn_oracle as go
    from pangnn_amd.subgraphs import SubGraphDataset
    subs = sub_graphs_from_golden(name, count=70)
    ds = SubGraphDataset.from_data_list(subs, device="cpu")
    assert ds.num_graphs == len(subs)
    for i0, i1 in ((0, 32), (32, 64), (64, len(subs)), (5, 6)):
        if i0 >= len(subs):
            continue
        b = ds.batch(i0, i1)
        ref = go.collate(subs[i0:i1])
        assert torch.equal(b.edge_index, ref.edge_index) and torch.equal(b.neighbour_edge_index, ref.neighbour_edge_index)
        assert torch.equal(b.edge_attr, ref.edge_attr) and torch.equal(b.y, ref.y) and torch.equal(b.x, ref.x)
        assert torch.equal(b.batch, ref.batch) and b.num_graphs == min(i1, len(subs)) - i0
    with pytest.raises(ValueError):
        bad = sub_graphs_from_golden(name, count=2)
        bad[1].edge_index = bad[1].edge_index + 10_000
        SubGraphDataset.from_data_list(bad, device="cpu")

