"""The host layer of the decoder's run-sum plans where there is no GPU: graph.RunPlan as EdgeStructure._plan_of_sorted_keys
builds it on CPU tensors (fields, dtypes, shapes, the part count against a plain-Python count), the route table of
functional._s_stream / _t_stream (which calls walk a plan's stream), and CSR.mark_short / long_rows."""
import dataclasses
from itertools import product
from types import SimpleNamespace

import pytest
import torch

from pangnn_amd import functional as PF, graph as G
from pangnn_amd.graph import CSR, EdgeStructure, RunPlan

KEYS = {"runs_and_gaps": ([0, 0, 1, 1, 1, 3], 5), "one_run_over_two_tiles": ([2] * 70, 3), "all_distinct": (list(range(33)), 33)}


def test_run_plan_declares_its_fields():
    assert [f.name for f in dataclasses.fields(RunPlan)] == ["n_parts", "part_off", "part_rowptr", "keys", "chunk_tiles", "last",
                                                             "stream"]


@pytest.mark.parametrize("ct", [1, 2])
@pytest.mark.parametrize("name", list(KEYS))
def test_the_plan_of_sorted_keys_is_a_run_plan(name, ct):
    keys, n_rows = KEYS[name]
    e, span = len(keys), 32 * ct
    plan = EdgeStructure._plan_of_sorted_keys(torch.tensor(keys, dtype=torch.int64), n_rows, ct)
    assert type(plan) is RunPlan and set(vars(plan)) == {f.name for f in dataclasses.fields(RunPlan)}
    n_chunks = (e + span - 1) // span
    assert type(plan.n_parts) is int and plan.n_parts == n_chunks + min(n_rows, e)
    assert type(plan.chunk_tiles) is int and plan.chunk_tiles == ct
    assert plan.part_off.dtype == torch.int32 and plan.part_off.shape == (n_chunks,)
    assert plan.part_rowptr.dtype == torch.int64 and plan.part_rowptr.shape == (n_rows + 1,)
    assert plan.keys.dtype == torch.int32 and plan.keys.tolist() == keys
    assert plan.last.dtype == torch.int64 and plan.last.shape == (1,)
    assert plan.stream is None
    starts = [k for k in range(e) if k % span == 0 or keys[k] != keys[k - 1]]           # a part per (chunk, key) run
    assert plan.n_parts_exact() == len(starts) <= plan.n_parts
    assert plan.part_off.tolist() == [starts.index(c * span) for c in range(n_chunks)]
    first = [sum(1 for k in starts if keys[k] < r) for r in range(n_rows + 1)]
    assert plan.part_rowptr.tolist() == first


def test_a_plan_answers_to_the_names_its_fields_had():
    """`spos` / `tpos` / `_last`, the attribute names of the untyped plans: the same objects as `stream` / `last`, and a write
    to either stream name is a write to `stream`"""
    words = torch.zeros(32, 2, dtype=torch.int32)
    plan = EdgeStructure._plan_of_sorted_keys(torch.tensor([0, 0, 1]), 2, 1)
    assert plan._last is plan.last and plan.spos is None and plan.tpos is None
    plan.stream = words
    assert plan.spos is words and plan.tpos is words
    plan.spos = None
    assert plan.stream is None and plan.tpos is None
    plan.tpos = words
    assert plan.stream is words and set(vars(plan)) == {f.name for f in dataclasses.fields(RunPlan)}


def _rows(stride, dtype):
    return torch.zeros(4, stride, dtype=dtype)[:, :64]


def test_route_table_of_the_stream_predicates():
    """words come back only for: the plan carries a stream, no `live` list and, for S, both byte strides powers of two"""
    words = torch.zeros(64, 2, dtype=torch.int32)
    plans = {"none": None, "standin_without": SimpleNamespace(stream=None), "standin_with": SimpleNamespace(stream=words),
             "run_plan_without": RunPlan(1, None, None, None, 1, None), "run_plan_with": RunPlan(1, None, None, None, 1, None, words)}
    lives = (None, torch.tensor([5], dtype=torch.int64))
    seen = set()
    for (name, plan), live in product(plans.items(), lives):
        walks = name.endswith("_with") and live is None
        assert (PF._t_stream(plan, live) is words) == walks and (walks or PF._t_stream(plan, live) is None), (name, live)
        for dtype, sp, sq in product((torch.float32, torch.bfloat16), (128, 192), (128, 192)):
            p, q = _rows(sp, dtype), _rows(sq, dtype)
            esz = p.element_size()
            assert esz == (4 if dtype == torch.float32 else 2) and (p.stride(0), q.stride(0)) == (sp, sq)
            pow2 = sp == 128 and sq == 128                                  # 512 / 256 bytes against 768 / 384
            assert pow2 == all((s * esz) & (s * esz - 1) == 0 for s in (sp, sq))
            got = PF._s_stream(plan, live, p, q)
            assert (got is words) == (walks and pow2) and (got is words or got is None), (name, live, dtype, sp, sq)
            seen.add((name, live is None, esz, sp, sq, got is words))
    assert len(seen) == 5 * 2 * 2 * 2 * 2 and sum(s[-1] for s in seen) == 2 * 2          # 2 plans x 2 element sizes


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"rowptr.{name} was read")


def test_mark_short_answers_without_reading_the_rows():
    c = CSR(_Untouchable(), _Untouchable(), _Untouchable())
    assert c.mark_short() is c and c._long is False
    assert c.long_rows() is None and c.long_rows(known_short=False) is None


def test_a_csr_decides_from_its_rows():
    lens = torch.tensor([1, G.LONG_ROW + 1, 0, 2])
    rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)])
    e = int(rowptr[-1])
    c = CSR(rowptr, torch.zeros(e, dtype=torch.int32), torch.arange(e, dtype=torch.int32))
    assert c._long is None and "_long" not in repr(c)
    seg_ptr, parts_rowptr = c.long_rows()
    assert c._long is not None and c.long_rows()[0] is seg_ptr                   # decided once
    seg = G.long_segment(G.LONG_ROW + 1)
    n_seg = [1, -(-(G.LONG_ROW + 1) // seg), 1, 1]                               # every row has at least one segment
    assert parts_rowptr.tolist() == [0] + torch.cumsum(torch.tensor(n_seg), 0).tolist()
    assert seg_ptr.shape == (sum(n_seg) + 1,) and seg_ptr[0] == 0 and seg_ptr[-1] == e
    assert int((seg_ptr[1:] - seg_ptr[:-1]).max()) <= seg
    short = CSR(rowptr[:2], torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    assert short._long is None and short.long_rows() is None and short._long is False
    same = CSR(rowptr, c.other, c.perm)
    assert same.long_rows(known_short=True) is None                              # the producer's word is taken
