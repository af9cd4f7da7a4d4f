"""pangnn_mask_k_smallest_i64 (csrc/mask_select.hip): keep = 0 for exactly the k entries that come first in (key, index)
order.  The referee is a stable sort on the CPU; draw_keep_mask on the device must return the mask torch.topk gave it
before, from the same generator.  Every comparison is exact."""
import pytest
import torch

from conftest import load_golden
from pangnn_amd import sampling
from pangnn_amd.data import Data
from pangnn_amd.sampling import draw_keep_mask, mask_k_smallest

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SIZES = [1, 255, 256, 257, 4097, 70001]


def ks(n):
    return sorted({0, 1, n // 5, n - 1, n})


def referee(keys, k):
    keep = torch.ones(keys.numel(), dtype=torch.bool)
    keep[torch.sort(keys.cpu(), stable=True).indices[:k]] = False
    return keep


def check(keys, k, what):
    before = keys.clone()
    got = mask_k_smallest(keys, k)
    assert got.dtype == torch.bool and got.shape == keys.shape and got.device == keys.device, what
    assert int((~got).sum()) == k, what
    assert torch.equal(got.cpu(), referee(keys, k)), what
    assert torch.equal(keys, before), what                                    # the keys are only read
    return got


def random_keys(n, seed):
    return torch.empty(n, dtype=torch.int64).random_(0, 1 << 62, generator=torch.Generator().manual_seed(seed)).to(DEV)


@pytest.mark.parametrize("n", SIZES)
def test_random_62_bit_keys(n):
    keys = random_keys(n, n)
    for k in ks(n):
        got = check(keys, k, (n, k))
        assert torch.equal(mask_k_smallest(keys, k), got)                     # deterministic
        if 0 < k < n:
            assert torch.equal(~got, torch.zeros(n, dtype=torch.bool, device=DEV).index_fill_(
                0, torch.topk(keys, k, largest=False).indices, True))         # distinct keys: what topk marks


@pytest.mark.parametrize("n", SIZES)
def test_ties_the_lower_index_loses(n):
    gen = torch.Generator().manual_seed(n + 1)
    few = torch.randint(0, 4, (n,), generator=gen).to(DEV)
    same = torch.full((n,), 12345678901234, dtype=torch.int64, device=DEV)
    top = torch.full((n,), (1 << 63) - 1, dtype=torch.int64, device=DEV)      # the largest key there is
    wide = few << 61                                                          # ties in the leading digit only
    for k in ks(n):
        check(few, k, ("four values", n, k))
        got = check(same, k, ("all equal", n, k))
        assert not bool(got[:k].any()) and bool(got[k:].all())
        check(top, k, ("all the largest key", n, k))
        check(wide, k, ("four values in the top bits", n, k))


@pytest.mark.parametrize("n", SIZES)
def test_the_shape_of_the_draw(n):
    """30 % of the keys are 1 << 62 and k is the number of the others: none of the masked ones may lose"""
    gen = torch.Generator().manual_seed(n + 2)
    keys = random_keys(n, n + 3)
    masked = (torch.rand(n, generator=gen) < 0.3).to(DEV)
    keys[masked] = 1 << 62
    k = n - int(masked.sum())
    got = check(keys, k, n)
    assert torch.equal(got, masked)
    if k > 1:
        got = check(keys, k // 2, n)
        assert bool(got[masked].all())


def test_arguments():
    keys = random_keys(100, 0)
    for k in (-1, 101):
        with pytest.raises(ValueError):
            mask_k_smallest(keys, k)
    with pytest.raises(ValueError):
        mask_k_smallest(keys.int(), 3)
    assert mask_k_smallest(keys[:0], 0).shape == (0,)
    odd = random_keys(101, 1)[1:]                                             # 8-byte aligned only: copied, same mask
    assert torch.equal(mask_k_smallest(odd, 20).cpu(), referee(odd, 20))


def golden_graph(name):
    f = load_golden(name)
    return Data(x=torch.from_numpy(f["whole_x"]).to(DEV), edge_index=torch.from_numpy(f["whole_edge_index"]).to(DEV),
                edge_attr=torch.from_numpy(f["whole_edge_attr"]).to(DEV), y=torch.from_numpy(f["whole_y"]).to(DEV),
                neighbour_edge_index=torch.from_numpy(f["whole_neighbour_edge_index"]).to(DEV))


@pytest.mark.parametrize("sample_pos", [False, True])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_device_draw_is_the_mask_topk_gave(seed, sample_pos, monkeypatch):
    g = golden_graph("cfg2_sim_1000x5")
    e = g.edge_index.shape[1]
    k = int(e * (1 - 0.8))
    # the mask rebuilt here from the same generator, with topk
    keys = torch.empty(e, dtype=torch.int64, device=DEV).random_(0, 1 << 62, generator=torch.Generator(device=DEV).manual_seed(seed))
    if not sample_pos:
        keys.masked_fill_(g.y != 0, 1 << 62)
    want = torch.ones(e, dtype=torch.bool, device=DEV)
    want[torch.topk(keys, k, largest=False, sorted=False).indices] = False
    real_topk = torch.topk

    def no_topk(*a, **kw):
        raise AssertionError("the device draw called torch.topk")

    monkeypatch.setattr(torch, "topk", no_topk)
    keep, kept = draw_keep_mask(g, 0.8, sample_pos, generator=torch.Generator(device=DEV).manual_seed(seed))
    again, _ = draw_keep_mask(g, 0.8, sample_pos, generator=torch.Generator(device=DEV).manual_seed(seed))
    monkeypatch.setattr(torch, "topk", real_topk)
    assert keep.dtype == torch.bool and keep.shape == (e,) and kept == e - k
    assert int((~keep).sum()) == k == int(e * (1 - 0.8))
    assert torch.equal(keep, want) and torch.equal(again, keep)
    if not sample_pos:
        assert bool(keep[g.y != 0].all())                                     # every positive kept
    monkeypatch.setattr(sampling, "MASK_KERNEL", False)                       # the torch route stays reachable: same mask
    torch_route, _ = draw_keep_mask(g, 0.8, sample_pos, generator=torch.Generator(device=DEV).manual_seed(seed))
    assert torch.equal(torch_route, keep)
