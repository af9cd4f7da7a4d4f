"""The induced-edge pass on the device (csrc/induced_edges.hip: pangnn_induced_edges_count / _fill) against its definition,
`subgraphs._induced_edges_index_ops`, on the same device tensors: the same (group, position, source local id, target local
id) columns in the same order, bit for bit; then `build_subgraphs` through it at the head-line configuration's edge law, the
memory the step takes, and batches of a data set built in passes."""
from types import SimpleNamespace

import pytest
import torch

from pangnn_amd import _lib, construct, simulate, subgraphs
from test_subgraph_passes import SIM_CASES, assert_same_dataset, simulated_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
STAGE = 6144                    # node ids of a group the kernel holds on chip (csrc/induced_edges.hip, kStage)


def tables_of(n, groups, device=DEV):
    """the node tables of hand-made groups (lists of node ids in row order, any order) as subgraphs._pass_tables lays them out"""
    all_g = torch.tensor([g for g, nodes in enumerate(groups) for _ in nodes], dtype=torch.int64)
    all_n = torch.tensor([v for nodes in groups for v in nodes], dtype=torch.int64)
    off = torch.zeros(len(groups) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.tensor([len(nodes) for nodes in groups], dtype=torch.int64), 0)
    local = torch.arange(all_g.numel()) - off[all_g]
    lk = all_g * n + all_n
    lo = torch.argsort(lk)
    t = SimpleNamespace(all_g=all_g, all_n=all_n, local=local, node_off_g=off, lk_sorted=lk[lo], lk_local=local[lo])
    return SimpleNamespace(**{k: v.to(device) for k, v in vars(t).items()})


def csr_of(n, rows, device=DEV):
    """(rowptr, dst) of {node: list of targets}; targets stay as listed (duplicates included)"""
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    for v, ts in rows.items():
        rowptr[v + 1] = len(ts)
    rowptr = torch.cumsum(rowptr, 0)
    dst = torch.tensor([x for v in sorted(rows) for x in rows[v]], dtype=torch.int64)
    return rowptr.to(device), dst.to(device)


def check_against_definition(n, rowptr, dst, t):
    """kernel == index ops, column by column; a second call gives the same bytes; returns the number of triples"""
    want = subgraphs._induced_edges_index_ops(n, rowptr, dst, t)
    got = subgraphs._induced_edges_kernel(n, rowptr, dst, t)
    again = subgraphs._induced_edges_kernel(n, rowptr, dst, t)
    torch.cuda.synchronize()
    for name, w, g, a in zip(("group", "position", "source", "target"), want, got, again):
        assert g.dtype == torch.int64 and g.shape == w.shape and torch.equal(g, w), name
        assert torch.equal(a, g), name
    return int(want[0].numel())


@pytest.mark.parametrize("n,genomes,frac,neighbours", SIM_CASES)
def test_kernel_equals_the_index_ops_on_simulated_relations(n, genomes, frac, neighbours):
    raw, s, d, w = simulated_inputs(n, genomes, frac)
    _, dst, _, rowptr = subgraphs._canonical_relation(raw.num_nodes, s.to(DEV), d.to(DEV), w.to(DEV))
    gid = raw.group_of.to(DEV)
    t = subgraphs._pass_tables(raw.num_nodes, rowptr, dst, gid, torch.arange(raw.num_nodes, device=DEV), int(gid.max()) + 1,
                               neighbours)
    assert check_against_definition(raw.num_nodes, rowptr, dst, t) > 0


def hand_built():
    """rows of out-degree 0, 1, 63, 64, 65, 129 and a hub of 5 000 (wave-sized steps and their edges), duplicate entries, a row
    with every target inside its group and one with every target outside, a group of one row and a group without rows"""
    n = 6000
    gen = torch.Generator().manual_seed(11)
    draw = lambda k: sorted(torch.randint(0, n, (k,), generator=gen).tolist())          # with repetitions
    rows = {1: [3], 2: draw(63), 3: draw(64), 4: draw(65), 5: draw(127) + [5998, 5998],
            6: sorted(list(range(100, 5000)) + [200, 200, 201, 4000] + draw(96)),        # the hub: 5 000 entries
            7: [0, 1, 2, 3, 3, 4, 5, 6, 8],                                              # all inside groups 0 and 3
            8: list(range(101, 5100, 2))}                                                # odd ids: all outside group 0
    for v in range(100, 5100, 7):
        rows[v] = draw(v % 4)
    assert [len(rows[v]) for v in (1, 2, 3, 4, 5, 6)] == [1, 63, 64, 65, 129, 5000] and 0 not in rows
    evens = list(range(100, 5100, 2))
    perm = torch.randperm(len(evens), generator=gen).tolist()
    groups = [list(range(9)) + [evens[i] for i in perm] + [5998],       # 2 510 rows in no particular order: held on chip
              [6],                                                      # one row, the hub: nothing inside
              [],                                                       # no rows
              [8, 7, 6, 5, 4, 3, 2, 1, 0],
              [5998, 3, 5]]
    return n, rows, groups


def test_kernel_equals_the_index_ops_on_the_hand_built_relation():
    n, rows, groups = hand_built()
    rowptr, dst = csr_of(n, rows)
    t = tables_of(n, groups)
    total = check_against_definition(n, rowptr, dst, t)
    eg, epos, s_local, t_local = subgraphs._induced_edges_kernel(n, rowptr, dst, t)
    per_group = torch.bincount(eg, minlength=len(groups)).tolist()
    assert sum(per_group) == total and per_group[1] == rows[6].count(6) and per_group[2] == 0
    # node 7 inside group 3: all nine entries, the duplicate too, in position order
    in3 = (eg == 3) & (s_local == 1)
    assert t_local[in3].tolist() == [8, 7, 6, 5, 5, 4, 3, 2, 0]
    # node 8 inside group 0: nothing; the hub inside group 0: its even targets, duplicates each
    assert int(((eg == 0) & (s_local == 8)).sum()) == 0
    hub = [x for x in rows[6] if (100 <= x < 5100 and x % 2 == 0) or x < 9 or x == 5998]
    assert int(((eg == 0) & (s_local == 6)).sum()) == len(hub) > 2450 and hub.count(200) >= 3


def test_empty_inputs():
    n, rows, groups = hand_built()
    rowptr, dst = csr_of(n, rows)
    # an empty row list: nothing to walk
    none = tables_of(n, [[], []])
    assert check_against_definition(n, rowptr, dst, none) == 0
    # E = 0: every row is empty
    rowptr0, dst0 = csr_of(n, {})
    assert dst0.numel() == 0 and check_against_definition(n, rowptr0, dst0, tables_of(n, groups)) == 0
    # the count entry itself on an empty row list: one scanned entry, the total
    lib = _lib.load()
    need = lib.pangnn_induced_edges_scratch_bytes(0)
    assert need > 0
    row_off = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    _lib.check(lib.pangnn_induced_edges_count(None, None, n, 0, None, 0, None, 0, None, None, row_off.data_ptr(),
                                              scratch.data_ptr(), need, _lib.stream_ptr()), "pangnn_induced_edges_count")
    assert row_off.tolist() == [0]


def test_groups_beyond_the_on_chip_stage_are_searched_in_place():
    """a group of all 20 000 nodes and one of 7 000 (global-memory search) around one of 3 000 (on chip), in one row list"""
    n = 20000
    gen = torch.Generator().manual_seed(5)
    src = torch.randint(0, n, (60000,), generator=gen)
    dst = torch.randint(0, n, (60000,), generator=gen)
    src = torch.cat([src, torch.full((3000,), 17, dtype=torch.int64)])                   # and a hub
    dst = torch.cat([dst, torch.randint(0, n, (3000,), generator=gen)])
    w = torch.ones(src.numel())
    _, dst, _, rowptr = subgraphs._canonical_relation(n, src.to(DEV), dst.to(DEV), w.to(DEV))
    groups = [torch.randperm(n, generator=gen).tolist(), torch.randperm(n, generator=gen)[:3000].tolist(),
              torch.randperm(n, generator=gen)[:7000].tolist(), torch.randperm(n, generator=gen)[:STAGE].tolist(),
              torch.randperm(n, generator=gen)[:STAGE + 1].tolist()]
    assert len(groups[0]) > STAGE < len(groups[2]) and len(groups[1]) < STAGE
    t = tables_of(n, groups)
    total = check_against_definition(n, rowptr, dst, t)
    assert total >= int(dst.numel())                     # group 0 holds every node: every edge is induced there


# ---- the head-line configuration's own edge law (1/50 scale), first 16 groups: rows of ~1 000 entries, ~4e5 expanded entries
# per group of which one in four stays
@pytest.fixture(scope="module")
def cfg4_law():
    raw = simulate.simulate_raw(1000, 20, 0.2, 100, 20, seed=0, device=DEV)
    s, d, sc = construct.remove_trivial_cases(raw.src, raw.dst, raw.score, raw.genome_of)
    s, d, w = construct.normalize_sim_scores(s, d, sc, raw.genome_of)
    nodes = torch.arange(raw.num_nodes, device=DEV)
    m = raw.group_of < 16
    return SimpleNamespace(n=raw.num_nodes, s=s, d=d, w=w, gid=raw.group_of[m], mem=nodes[m], group_of=raw.group_of)


@pytest.fixture(scope="module")
def cfg4_datasets(cfg4_law):
    c = cfg4_law
    build = lambda **kw: subgraphs.build_subgraphs(c.n, c.s, c.d, c.w, c.gid, c.mem, labels_group_of=c.group_of, **kw)
    calls = []
    kernel = subgraphs._induced_edges_kernel
    subgraphs._induced_edges_kernel = lambda *a: calls.append(1) or kernel(*a)
    try:
        by_kernel = build()
        assert len(calls) == 1
        in_passes = build(groups_per_pass=5)
        assert len(calls) == 1 + 4                       # 16 groups, 5 at a time
        subgraphs.INDUCED_KERNEL = False
        by_index_ops = build()
        assert len(calls) == 5
    finally:
        subgraphs.INDUCED_KERNEL = True
        subgraphs._induced_edges_kernel = kernel
    return SimpleNamespace(by_kernel=by_kernel, in_passes=in_passes, by_index_ops=by_index_ops)


def test_three_routes_build_one_dataset_at_the_headline_edge_law(cfg4_law, cfg4_datasets):
    ds = cfg4_datasets
    assert ds.by_kernel.num_graphs > 1 and ds.by_kernel.edge_index.is_cuda
    rowlen = torch.bincount(cfg4_law.s, minlength=cfg4_law.n)
    assert int(rowlen[ds.by_kernel.node_global].max()) > 128            # rows of several wave steps are among them
    assert_same_dataset(ds.by_index_ops, ds.by_kernel)
    assert_same_dataset(ds.in_passes, ds.by_kernel)


def test_the_step_allocates_nothing_of_the_expanded_size(cfg4_law):
    """peak memory across the induced-edge step alone, over its baseline: at most twice the bytes of the four columns it
    returns plus 64 bytes per row (row offsets, row counts, the groups' sorted node ids and their transients: a few int64
    words per ROW).  The index-op route holds four int64 columns per EXPANDED entry at once, 32 bytes each, before it
    drops three in four of them."""
    c = cfg4_law
    _, dst, _, rowptr = subgraphs._canonical_relation(c.n, c.s, c.d, c.w)
    t = subgraphs._pass_tables(c.n, rowptr, dst, c.gid, c.mem, 16, 1)
    rows = int(t.all_n.numel())
    expanded = int((rowptr[t.all_n + 1] - rowptr[t.all_n]).sum())

    def peak_of(step):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = step(c.n, rowptr, dst, t)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, out

    peak, out = peak_of(subgraphs._induced_edges_kernel)
    returned = sum(x.numel() * x.element_size() for x in out)
    kept = int(out[0].numel())
    bound = 2 * returned + 64 * rows
    print(f"rows {rows}  expanded {expanded}  kept {kept}  returned {returned} B  peak {peak} B  bound {bound} B  "
          f"index ops need >= {32 * expanded} B")
    assert returned == 32 * kept and 0 < kept < expanded
    assert peak <= bound
    assert bound < 32 * expanded                                        # what the index-op route cannot stay under
    peak_ops, out_ops = peak_of(subgraphs._induced_edges_index_ops)
    print(f"index ops: peak {peak_ops} B")
    assert peak_ops >= 32 * expanded
    assert all(torch.equal(a, b) for a, b in zip(out, out_ops))


def test_batches_of_a_dataset_built_in_passes(cfg4_datasets):
    a, b = cfg4_datasets.in_passes.batch(0, 4), cfg4_datasets.by_kernel.batch(0, 4)
    assert subgraphs.COLLATE_KERNEL and a.num_graphs == b.num_graphs == 4
    for f in ("x", "edge_index", "edge_attr", "y", "neighbour_edge_index", "ptr", "batch"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
