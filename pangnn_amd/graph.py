"""Device-resident graph structure for the message-passing kernels.

The reference hands a COO `edge_index [2,E] int64` to `GCNConv` on every call
(/root/reference/src/gnn.py:158,165) and PyG walks it with index_select / scatter_add.  The HIP
kernels instead want the edges grouped by destination (forward) and by source (backward), with
int32 neighbour ids.  `EdgeStructure` builds both groupings once per `edge_index` tensor on the
GPU (stable radix sort => deterministic per-row order) and memoises the GCN normalisation per
`edge_weight` tensor.  The caller's edge order is never changed: per-edge outputs (logits) stay in
`edge_index` order, `perm` maps sorted positions back.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from operator import attrgetter
from typing import Dict, Optional, Tuple

import torch

from . import _lib


# mini-batch sized square structures are built by one launch (EdgeStructure._small_build); False: always the general
# radix-sort build + index-op plans (what the parity tests compare the small build with)
SMALL_STRUCTURE = os.environ.get("PANGNN_SMALL_STRUCTURE", "1") != "0"
# the decoder's run-sum plans of a structure that takes the general build come from its row pointers in one scan + one launch
# (pangnn_csr_plan, EdgeStructure._plan_of_rowptr); False: the index-op route (_plan_of_sorted_keys: the definition the
# kernel is tested against), for A/B
PLAN_KERNEL = os.environ.get("PANGNN_PLAN_KERNEL", "1") != "0"


# components of a structure as the native registry (csrc/graph_ops.cpp) names them: bits of `push_native(need)` and of
# pangnn::_prepare_structure(..., need)
(NEED_BY_DST, NEED_BY_SRC, NEED_BAND, NEED_RUNSUM, NEED_PLAN_DST, NEED_PLAN_SRC, NEED_NORM, NEED_NORM_SRC, NEED_ACTIONS,
 NEED_ENTRY) = (1 << i for i in range(10))
_STRUCT_BITS = NEED_BY_DST | NEED_BY_SRC | NEED_BAND | NEED_RUNSUM | NEED_ENTRY
_NORM_BITS = NEED_NORM | NEED_NORM_SRC | NEED_ACTIONS


# Long rows of the propagate kernels (one wave walks one row: spmm_row_kernel): a row of more than LONG_ROW entries — a hub of
# the similarity graph — would keep ONE wave busy for its whole length while the rest of the chip has finished (1e5 entries of
# 256-byte rows: 25 MB through one wave, ~0.5 ms).  A CSR whose longest row exceeds LONG_ROW is therefore run as SEGMENTS of at
# most ~sqrt(longest row) entries (long_segment): the same kernel over the segment table (a row pointer over virtual rows) writes one partial row per
# segment, and the contiguous part sum that the decoder's run sums already use adds a row's partials in order — fixed order,
# no atomics, independent of the grid.  SURVEY.md §7 step 3 ("long rows split across wavefronts with a second-pass reduce").
LONG_ROW = int(os.environ.get("PANGNN_LONG_ROW", "8192"))
LONG_SEG = int(os.environ.get("PANGNN_LONG_SEG", "0"))       # 0: about the square root of the longest row (below)


def long_segment(max_len: int) -> int:
    """entries per segment for a CSR whose longest row has `max_len` entries: the wave that walks a segment and the wave that
    adds the hub's partial rows both work serially (~25 ns per entry / per part row), so the critical path seg + max_len / seg
    is shortest at seg = sqrt(max_len); a power of two in [256, 4096]"""
    if LONG_SEG > 0:
        return LONG_SEG
    seg = 256
    while seg < 4096 and seg * seg < max_len:
        seg *= 2
    return seg


@dataclass
class CSR:
    rowptr: torch.Tensor   # int64 [N+1]
    other: torch.Tensor    # int32 [E]  opposite endpoint of each sorted edge
    perm: torch.Tensor     # int32 [E]  original edge id of each sorted edge
    _long: object = field(default=None, repr=False, compare=False)      # long_rows' answer: None undecided, False short rows

    def mark_short(self) -> "CSR":
        """the producer vouches that no row exceeds LONG_ROW: long_rows() answers None without reading the rows"""
        self._long = False
        return self

    def long_rows(self, known_short: bool = False):
        """None, or (seg_ptr int64 [V + 1], parts_rowptr int64 [N + 1]) when the longest row exceeds LONG_ROW: segment v covers
        entries [seg_ptr[v], seg_ptr[v + 1]), the segments of row r are [parts_rowptr[r], parts_rowptr[r + 1]) (every row has
        at least one).  Decided once per CSR (one host read-back of the longest row, none for structures whose producer
        vouches for short rows: `known_short`)."""
        hit = self._long
        if hit is None:
            hit = False
            n = self.rowptr.shape[0] - 1
            if not known_short and n > 0 and self.other.shape[0] > LONG_ROW:
                lens = self.rowptr[1:] - self.rowptr[:-1]
                longest = int(lens.max())
                if longest > LONG_ROW:
                    seg = long_segment(longest)
                    nseg = torch.div(lens + (seg - 1), seg, rounding_mode="floor").clamp_(min=1)
                    parts_rowptr = torch.zeros(n + 1, dtype=torch.int64, device=lens.device)
                    torch.cumsum(nseg, 0, out=parts_rowptr[1:])
                    row_of = torch.repeat_interleave(torch.arange(n, device=lens.device), nseg)
                    j = torch.arange(row_of.shape[0], device=lens.device) - parts_rowptr[row_of]
                    seg_ptr = torch.cat([self.rowptr[row_of] + j * seg, self.rowptr[-1:]]).contiguous()
                    hit = (seg_ptr, parts_rowptr)
            self._long = hit
        return hit or None


def carve(dtype: torch.dtype, device, counts, align: int = 16):
    """One allocation holding a table of counts[i] elements for every i: the 1-D views, in order, each starting on an
    `align`-byte boundary of the allocation (a count of 0: an empty view).  Every packed table the kernels write through raw
    pointers is laid out here."""
    unit = align // dtype.itemsize
    starts, end = [], 0
    for k in counts:
        starts.append(end)
        end += -(-k // unit) * unit
    buf = torch.empty(end, dtype=dtype, device=device)
    return [buf[s:s + k] for s, k in zip(starts, counts)]


def chunk_tiles_for(num_edges: int) -> int:
    """tiles per run-sum chunk of the S / T kernels for a list of `num_edges` edges: the one place that asks the library"""
    return int(_lib.load().pangnn_decoder_chunk_tiles_for(int(num_edges)))


def n_chunks(num_edges: int, chunk_tiles: int) -> int:
    """chunks of `chunk_tiles` 32-edge tiles that an edge list has (the entries of a plan's part_off)"""
    return (num_edges + 32 * chunk_tiles - 1) // (32 * chunk_tiles)


def part_bound(rows: int, num_edges: int, chunk_tiles: int) -> int:
    """upper bound of a plan's part count — one part per chunk start plus one per key change — that every S / T part buffer
    is sized by (RunPlan.n_parts)"""
    return n_chunks(num_edges, chunk_tiles) + min(rows, num_edges)


@dataclass
class RunPlan:
    """Layout of the per-(chunk, key) part rows of an edge order with non-decreasing keys; a chunk is `chunk_tiles` consecutive
    32-edge tiles.  part_off[c] (int32): index of chunk c's first part; the parts of row r are [part_rowptr[r],
    part_rowptr[r + 1]) (int64; consecutive: sorted); keys: the int32 [E] copy handed to the kernels; n_parts: an upper bound
    (what the part buffer is sized by, no read-back); last: device int64[1], the index of the last part.
    `stream` (where EdgeStructure._streams says so): the order as int32 words, read as uint32, that a decoder pass walks
    instead of the ids; bit 31 of a position's first word = "a part ends behind this position".  A CSR-order plan: [E] words
    perm[p] | closes << 31 (pangnn_csr_plan_tpos -> pangnn_decoder_dgrad_stream_f32).  The run-sum plan: [32 ceil(E / 32), 2]
    pairs { src | closes << 31, dst }, a position past the list repeating the last edge (pangnn_csr_plan_spos ->
    pangnn_decoder_train_stream_*)."""
    n_parts: int
    part_off: torch.Tensor
    part_rowptr: torch.Tensor
    keys: torch.Tensor
    chunk_tiles: int
    last: torch.Tensor
    stream: Optional[torch.Tensor] = None

    def n_parts_exact(self) -> int:           # the one device -> host read-back of a plan (bench accounting)
        return int(self.last) + 1

    # The names these fields had on the untyped plans (`spos` on a run-sum plan, `tpos` on a by-target plan, `_last`), kept
    # for callers outside the package (the streams writable too); nothing inside it uses them.
    def _set_stream(self, words: Optional[torch.Tensor]):
        self.stream = words

    spos = tpos = property(attrgetter("stream"), _set_stream)
    _last = property(attrgetter("last"))


def build_csr(edge_index: torch.Tensor, num_nodes: int, group_by: int, validate: bool = True,
              num_rows: Optional[int] = None) -> CSR:
    """pangnn_csr_build: group_by=1 rows are targets (edge_index[1]), 0 rows are sources.
    `num_nodes` bounds both endpoints; `num_rows` (<= num_nodes) trims rowptr for a rectangular
    (partitioned) graph whose grouped endpoint only takes ids < num_rows."""
    _lib.require_device(edge_index)
    if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError(f"edge_index must be int64 [2,E], got {edge_index.dtype} {tuple(edge_index.shape)}")
    lib = _lib.load()
    ei = edge_index if edge_index.is_contiguous() else edge_index.contiguous()
    e = ei.shape[1]
    dev = ei.device
    rowptr = torch.empty(num_nodes + 1, dtype=torch.int64, device=dev)
    other = torch.empty(e, dtype=torch.int32, device=dev)
    perm = torch.empty(e, dtype=torch.int32, device=dev)
    with _lib.device_guard(dev):
        ws_bytes = lib.pangnn_csr_build_workspace_bytes(e, num_nodes)
        if ws_bytes == 0:
            raise _lib.PangnnHipError("pangnn_csr_build_workspace_bytes failed")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.pangnn_csr_build(ei.data_ptr(), e, e, num_nodes, group_by, rowptr.data_ptr(),
                                        _lib.ptr(other), _lib.ptr(perm), ws.data_ptr(), ws_bytes,
                                        _lib.stream_ptr()), "pangnn_csr_build")
        if validate and e > 0:
            # the flag lives in the workspace; view it as a tensor slice (device -> host 4 bytes)
            off = lib.pangnn_csr_build_flag_ptr(ws.data_ptr(), e) - ws.data_ptr()
            if int(ws[off:off + 4].view(torch.int32).item()) != 0:
                raise ValueError(f"edge_index contains node ids outside [0, {num_nodes})")
    if num_rows is not None and num_rows < num_nodes:
        rowptr = rowptr[: num_rows + 1]
    return CSR(rowptr, other, perm)


class EdgeStructure:
    """Both groupings of one edge_index plus memoised GCN normalisations."""

    def __init__(self, edge_index: torch.Tensor, num_nodes: int, num_src: Optional[int] = None, hints: Optional[dict] = None):
        """`num_nodes` = number of TARGET rows (= all nodes for a whole graph).  `num_src` (default
        the same) = number of SOURCE rows: a destination-partitioned shard keeps local target ids
        and global source ids (pangnn_amd/dist.py).
        `hints` (optional; set by producers that KNOW them, e.g. SubGraphDataset.batch): {"valid_ids": True} — every id
        is inside [0, num_nodes), skip the range check and its host read-back; {"sorted_by_src": bool} — whether the
        list is source-sorted, skip that test's host read-back; {"band_width": k} — whether the list is the whole-graph
        positional-neighbour pattern (0: it is not), skip that comparison's host read-back; {"short_rows": bool} — whether
        no row exceeds LONG_ROW (default: what "valid_ids" says), skip the longest row's host read-back.  With all of them a structure
        is built without any device -> host synchronisation (a fresh mini-batch per step, pangnn.py:152-216)."""
        self.hints = dict(hints or {})
        self._key_tensor = edge_index        # the caches are keyed on THIS tensor's address: keep it alive
        self.edge_index = edge_index if edge_index.is_contiguous() else edge_index.contiguous()
        self.num_nodes = int(num_nodes)
        self.num_src = int(num_nodes if num_src is None else num_src)
        self.num_edges = int(edge_index.shape[1])
        self._by_dst: Optional[CSR] = None
        self._by_src: Optional[CSR] = None
        self._norm: Dict[Tuple, Tuple["GcnNorm", Optional[torch.Tensor]]] = {}
        self._sorted: Optional[bool] = None  # sorted_by_src's answer
        # by ("run" | "dst" | "src", chunk_tiles): the run-sum plan of a source-sorted list, the plans of the CSR orders
        self._plans: Dict[Tuple[str, int], Optional[RunPlan]] = {}
        self._band: Optional[int] = None
        self._small_built = False
        self.filter_state, self._filter_claim = None, None   # set on the children `filtered` makes
        self._native = 0                     # NEED_* bits already pushed to the native registry (push_native)

    @classmethod
    def filtered(cls, parent: "EdgeStructure", keep: torch.Tensor, num_kept: Optional[int] = None, arrays=()):
        """The structure of the kept edges of `parent` (keep[e] != 0), DERIVED from the parent's tables by an
        order-preserving compaction instead of two sorts (pangnn_structure_filter, csrc/edge_filter.hip): a fresh
        sub-sample of a whole graph per step (sampling.sub_sample_graph_edges, pangnn.py:190).
        Returns (child, kept_id int32 [E'], [compacted array for each of `arrays`]): child.edge_index holds the kept edges
        in the caller's order, kept_id the parent edge id of every child edge, `arrays` are up to two per-edge fp32
        tensors ([E], e.g. edge_attr and y) compacted alongside.  The child gets the by-target CSR always and the
        by-source CSR if the parent holds it (a missing order is built lazily, as ever) — the tables build_csr would make
        of child.edge_index, entry for entry — and the hints the parent vouches for: valid ids, the parent's
        sorted-by-source answer (a subsequence of a sorted list is sorted), no band, short rows where the parent's are
        (a CSR order of the parent with hub rows leaves the child's to decide for itself: one read-back on first use).
        `keep`: [E] bool / uint8 / int8 / int32 are read as stored, any other dtype through one `!= 0` pass.
        `num_kept`: the number of kept edges where the caller knows it: nothing is then read back, and
        child.filter_state (int32 [2]: the device's count, a status word that is non-zero when the count differs) says
        whether it was right — `child.check_filter()` reads it.  Without it the count costs one device -> host read.
        Square structures only: a partitioned shard's rectangular structure raises ValueError."""
        if parent.num_src != parent.num_nodes:
            raise ValueError("EdgeStructure.filtered needs a square structure (a whole graph or a collated batch), not a "
                             "partitioned shard's")
        lib = _lib.load()
        ei, e, n = parent.edge_index, parent.num_edges, parent.num_nodes
        _lib.require_device(ei, keep, *arrays)
        keep = keep.detach().reshape(-1)
        if keep.numel() != e:
            raise ValueError(f"{keep.numel()} keep entries for {e} edges")
        if keep.dtype not in (torch.bool, torch.uint8, torch.int8, torch.int32):
            keep = keep != 0
        keep = keep.contiguous()
        if len(arrays) > 2:
            raise ValueError("at most two per-edge arrays are compacted alongside")
        for a in arrays:
            if a.dtype != torch.float32 or a.dim() != 1 or a.shape[0] != e or not a.is_contiguous():
                raise ValueError(f"a per-edge array must be contiguous float32 [{e}], got {a.dtype} {tuple(a.shape)}")
        known = num_kept is not None
        kept = int(num_kept) if known else int(torch.count_nonzero(keep))           # the one read-back
        if not 0 <= kept <= e:
            raise ValueError(f"num_kept = {kept} of {e} edges")
        dev = ei.device
        d = parent.by_dst
        s = parent._by_src
        c_ei = torch.empty((2, kept), dtype=torch.int64, device=dev)
        kept_id = torch.empty(kept, dtype=torch.int32, device=dev)
        outs = [torch.empty(kept, dtype=torch.float32, device=dev) for _ in arrays]
        orders = 2 if s is not None else 1
        *seg32, state = carve(torch.int32, dev, [kept] * (2 * orders) + [2])       # (other, perm) per order, then the state
        rowptrs = carve(torch.int64, dev, [n + 1] * orders)
        tabs = [CSR(rowptrs[o], seg32[2 * o], seg32[2 * o + 1]) for o in range(orders)]
        a_in, a_out = list(arrays) + [None, None], outs + [None, None]
        with _lib.device_guard(dev):
            ws_bytes = lib.pangnn_structure_filter_workspace_bytes(e)
            if ws_bytes == 0:
                raise _lib.PangnnHipError("pangnn_structure_filter_workspace_bytes failed")
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            c_d, c_s = tabs[0], (tabs[1] if orders == 2 else None)
            _lib.check(lib.pangnn_structure_filter(
                _lib.ptr(ei) if e else None, e, e, n, _lib.ptr(keep) if e else None, keep.element_size(), kept,
                d.rowptr.data_ptr(), _lib.ptr(d.other) if e else None, _lib.ptr(d.perm) if e else None,
                None if s is None else s.rowptr.data_ptr(), None if s is None else s.other.data_ptr(),
                None if s is None else s.perm.data_ptr(), _lib.ptr(a_in[0]), _lib.ptr(a_in[1]),
                c_ei.data_ptr() if kept else None, kept, kept_id.data_ptr() if kept else None,
                _lib.ptr(a_out[0]), _lib.ptr(a_out[1]),
                c_d.rowptr.data_ptr(), c_d.other.data_ptr() if kept else None, c_d.perm.data_ptr() if kept else None,
                None if c_s is None else c_s.rowptr.data_ptr(),
                c_s.other.data_ptr() if (c_s is not None and kept) else None,
                c_s.perm.data_ptr() if (c_s is not None and kept) else None,
                state.data_ptr(), state[1:].data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr()),
                "pangnn_structure_filter")
        # what the parent knows holds for every subsequence of its list: sortedness, and rows no longer than LONG_ROW (both
        # decided once per PARENT — a read-back each the first time — so that a child per step costs none)
        short = [c.long_rows(parent._small_built or parent._vouched_short()) is None for c in (d, s) if c is not None]
        hints = {"valid_ids": True, "band_width": 0, "short_rows": len(short) == 2 and all(short)}
        if e:
            hints["sorted_by_src"] = parent.sorted_by_src()
        child = cls(c_ei, n, hints=hints)
        child._by_dst, child._by_src = tabs[0], (tabs[1] if orders == 2 else None)
        for c, is_short in zip(tabs, short):
            if is_short:
                c.mark_short()
        child.filter_state, child._filter_claim = state, (kept if known else None)
        return child, kept_id, outs

    def check_filter(self):
        """for a structure made by `filtered(..., num_kept=k)`: raise ValueError unless the mask had exactly k entries set
        (one device -> host read; the tables of a structure that fails this are not to be used)"""
        if self._filter_claim is not None:
            count, status = self.filter_state.tolist()
            if status & 1:
                raise ValueError(f"keep has {count} entries set, num_kept said {self._filter_claim}")
            if status:
                raise ValueError("the parent structure's tables are inconsistent")
        return self

    def _small_build(self) -> bool:
        """A small square structure (a mini-batch of sub-graphs): both CSR orders and the S / T kernels' chunk plans of both
        orders from ONE launch (pangnn_structure_small) instead of ~10 launches per CSR order and ~18 per plan — the same
        tables, entry for entry, as build_csr / _plan_of_sorted_keys (tests/test_hip_parity.py).  False: not applicable."""
        if not SMALL_STRUCTURE or self._by_dst is not None or self._by_src is not None or self.num_src != self.num_nodes:
            return False
        lib = _lib.load()
        e, n = self.num_edges, self.num_nodes
        if not lib.pangnn_structure_small_supported(e, n):
            return False
        ct = chunk_tiles_for(e)
        nc = n_chunks(e, ct)
        dev = self.edge_index.device
        other_d, perm_d, keys_d, other_s, perm_s, keys_s, poff_d, poff_s, bad = carve(
            torch.int32, dev, [e] * 6 + [nc] * 2 + [1])
        rp_d, prp_d, rp_s, prp_s, last_d, last_s = carve(torch.int64, dev, [n + 1] * 4 + [1] * 2)    # (a 16-byte slot per `last`)
        with _lib.device_guard(dev):
            _lib.check(lib.pangnn_structure_small(
                self.edge_index.data_ptr(), e, e, n, 32 * ct, rp_d.data_ptr(), other_d.data_ptr(), perm_d.data_ptr(),
                keys_d.data_ptr(), poff_d.data_ptr(), prp_d.data_ptr(), last_d.data_ptr(), rp_s.data_ptr(),
                other_s.data_ptr(), perm_s.data_ptr(), keys_s.data_ptr(), poff_s.data_ptr(), prp_s.data_ptr(),
                last_s.data_ptr(), bad.data_ptr(), _lib.stream_ptr()), "pangnn_structure_small")
            if not self.hints.get("valid_ids", False) and int(bad.item()) != 0:
                raise ValueError(f"edge_index contains node ids outside [0, {n})")
        n_bound = part_bound(n, e, ct)
        self.adopt_tables(CSR(rp_d, other_d, perm_d), CSR(rp_s, other_s, perm_s),
                          {("dst", ct): RunPlan(n_bound, poff_d, prp_d, keys_d, ct, last_d),
                           ("src", ct): RunPlan(n_bound, poff_s, prp_s, keys_s, ct, last_s)})
        return True

    def adopt_tables(self, by_dst: CSR, by_src: CSR, plans=None, short_rows: bool = True):
        """Take over tables written in the small build's format (by it, or for a collated batch: SubGraphDataset.
        _structures_of): both CSR orders and their stream-less plans {("dst" | "src", chunk_tiles): RunPlan}.  `short_rows`: no
        row exceeds LONG_ROW (<= 16384 edges in all, a batch of small sub-graphs): no split, no read-back."""
        self._by_dst, self._by_src, self._small_built = by_dst, by_src, True
        if short_rows:
            by_dst.mark_short(), by_src.mark_short()
        if plans:
            self._plans.update(plans)
        return self

    @property
    def by_dst(self) -> CSR:
        if self._by_dst is None and self._small_build():
            return self._by_dst
        if self._by_dst is None:
            nmax = max(self.num_nodes, self.num_src)
            self._by_dst = build_csr(self.edge_index, nmax, 1, validate=not self.hints.get("valid_ids", False),
                                     num_rows=self.num_nodes)
            if self.num_nodes < nmax and self.num_edges and int(self.edge_index[1].max()) >= self.num_nodes:
                raise ValueError("target id outside the local row range")
            if self._vouched_short():                    # a producer-vouched list (a collated batch): built without any
                self._by_dst.mark_short()                # read-back, so no read-back of the longest row either
        return self._by_dst

    @property
    def by_src(self) -> CSR:
        if self._by_src is None and self._small_build():
            return self._by_src
        if self._by_src is None:
            nmax = max(self.num_nodes, self.num_src)
            self._by_src = build_csr(self.edge_index, nmax, 0, validate=False, num_rows=self.num_src)
            if self._vouched_short():
                self._by_src.mark_short()
        return self._by_src

    def _vouched_short(self) -> bool:
        """the producer vouches that no row exceeds LONG_ROW: {"short_rows": bool} where it says so (a filtered structure
        inherits what its parent knows), else whatever vouches for the ids (a collated batch of small sub-graphs)"""
        return bool(self.hints.get("short_rows", self.hints.get("valid_ids", False)))

    def sorted_by_src(self) -> bool:
        """the caller's edge order is sorted by source (decided once: the producer's hint, or one host read-back)"""
        if self._sorted is None:
            src, e = self.edge_index[0], self.num_edges
            if e == 0:
                self._sorted = False
            elif "sorted_by_src" in self.hints:
                self._sorted = bool(self.hints["sorted_by_src"])
            else:
                self._sorted = bool((src[1:] >= src[:-1]).all())
        return self._sorted

    def band_width(self) -> int:
        """k > 0 if this edge list IS the positional-neighbour graph of a whole genome set as the reference builds it
        (dataset.py:356-361: edges (i, j), j in [i - k, i + k] within [0, N), self loops included, in nested-loop order) —
        a band matrix, propagated without index arrays (pangnn_band_propagate); 0 for any other list.  Decided once per
        structure by comparing with the generated pattern (one host sync)."""
        if self._band is None and "band_width" in self.hints:      # the producer knows (a collated batch: 0), no host sync
            self._band = int(self.hints["band_width"])
        if self._band is None:
            self._band = 0
            n, e = self.num_nodes, self.num_edges
            if self.num_src == n and n > 0 and e > 0:
                for k in range(1, 9):
                    if k < n and e == n * (2 * k + 1) - k * (k + 1):
                        dev = self.edge_index.device
                        i = torch.arange(n, dtype=torch.int64, device=dev).repeat_interleave(2 * k + 1)
                        j = i + torch.arange(-k, k + 1, dtype=torch.int64, device=dev).repeat(n)
                        keep = (j >= 0) & (j < n)
                        if torch.equal(self.edge_index, torch.stack([i[keep], j[keep]])):
                            self._band = k
                        break
        return self._band

    @staticmethod
    def _plan_of_sorted_keys(keys: torch.Tensor, n_rows: int, chunk_tiles: int = 1) -> RunPlan:
        """The stream-less RunPlan of an edge order whose `keys` are non-decreasing, by index ops (the definition the plan
        kernels are tested against); chunk_tiles 1: the strict-fp32 kernels of decoder.hip; pangnn_decoder_chunk_tiles()
        = 16: the S / T kernels of decoder16.hip, whose waves carry an open run from tile to tile inside a chunk."""
        e = keys.shape[0]
        span = 32 * int(chunk_tiles)
        flags = (torch.arange(e, device=keys.device) % span) == 0
        flags[1:] |= keys[1:] != keys[:-1]
        part_id = torch.cumsum(flags, 0) - 1
        # Everything stays on the device (no host read-back): the part buffer is sized by an upper bound — one part per
        # chunk start plus one per key change — and a row's first part is the part of its first entry (a key change
        # always starts a part).  `n_parts_exact()` reads the true count when somebody needs it (bench accounting).
        n_bound = part_bound(int(n_rows), e, int(chunk_tiles))
        first = torch.searchsorted(keys, torch.arange(n_rows + 1, device=keys.device, dtype=keys.dtype))
        pid_ext = torch.cat([part_id, part_id[-1:] + 1])
        return RunPlan(n_bound, part_id[::span].to(torch.int32).contiguous(), pid_ext[first].contiguous(),
                       keys.to(torch.int32).contiguous(), int(chunk_tiles), part_id[-1:])

    @staticmethod
    def _plan_of_rowptr(rowptr: torch.Tensor, num_edges: int, chunk_tiles: int = 1, perm: Optional[torch.Tensor] = None):
        """The plan `_plan_of_sorted_keys` makes of a CSR order's keys, from that order's row pointer alone (device tensors;
        pangnn_csr_plan, csrc/csr_plan.hip): the keys are non-decreasing, so the key changes sit at rowptr[r] of the
        non-empty rows — one scan over the rows and one write of `keys`, no pass over a key array.  Same fields, dtypes and
        shapes, entry for entry (tests/test_csr_plan.py).
        `perm` (that order's int32 edge ids): the plan also carries the CSR-order `stream` (4 more bytes per edge kept)."""
        lib = _lib.load()
        e, n_rows, ct = int(num_edges), rowptr.shape[0] - 1, int(chunk_tiles)
        span = 32 * ct
        dev = rowptr.device
        rowptr = rowptr if rowptr.is_contiguous() else rowptr.contiguous()
        keys = torch.empty(e, dtype=torch.int32, device=dev)
        part_off = torch.empty(n_chunks(e, ct), dtype=torch.int32, device=dev)
        part_rowptr, last = carve(torch.int64, dev, [n_rows + 1, 1])
        with _lib.device_guard(dev):
            ws_bytes = lib.pangnn_csr_plan_workspace_bytes(n_rows)
            if ws_bytes == 0:
                raise _lib.PangnnHipError("pangnn_csr_plan_workspace_bytes failed")
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.pangnn_csr_plan(rowptr.data_ptr(), n_rows, e, span, keys.data_ptr(), part_off.data_ptr(),
                                           part_rowptr.data_ptr(), last.data_ptr(), ws.data_ptr(), ws_bytes,
                                           _lib.stream_ptr()), "pangnn_csr_plan")
            stream = None
            if perm is not None:
                perm = perm if perm.is_contiguous() else perm.contiguous()
                stream = torch.empty(e, dtype=torch.int32, device=dev)
                _lib.check(lib.pangnn_csr_plan_tpos(perm.data_ptr(), keys.data_ptr(), e, span, stream.data_ptr(),
                                                    _lib.stream_ptr()), "pangnn_csr_plan_tpos")
        return RunPlan(part_bound(n_rows, e, ct), part_off, part_rowptr, keys, ct, last, stream)

    @staticmethod
    def _spos_of_sorted_list(edge_index: torch.Tensor, chunk_tiles: int) -> torch.Tensor:
        """The run-sum plan's `stream` (RunPlan) of a source-sorted device list: pangnn_csr_plan_spos."""
        lib = _lib.load()
        e = edge_index.shape[1]
        ei = edge_index if edge_index.stride(1) == 1 else edge_index.contiguous()
        spos = torch.empty((e + 31) // 32 * 32, 2, dtype=torch.int32, device=ei.device)
        with _lib.device_guard(ei.device):
            _lib.check(lib.pangnn_csr_plan_spos(ei.data_ptr(), ei.stride(0), e, 32 * int(chunk_tiles), spos.data_ptr(),
                                                _lib.stream_ptr()), "pangnn_csr_plan_spos")
        return spos

    def _streams(self, kind: str, ct: int) -> bool:
        """Whether the plan (kind, ct), kind in {"run", "dst", "src"}, carries a `stream` (RunPlan).  All of: a square structure
        (not a partitioned shard's rectangular one); ct is the S / T kernels' chunk size for this edge count (not the
        strict-fp32 kernels' one-tile chunks of a long list); the plan kernel makes the plan (PLAN_KERNEL on device tensors: not
        the index-op route, not the small build or a collated batch's tables); and the order is by target with int32 edge ids
        (4 more bytes per edge kept) or the run-sum plan's of a list that is no filtered child (8 more bytes; a child's list
        lives for one step: building its stream would cost more than S saves on it).  A pass over a plan without one reads
        the ids: S the int64 list, T the order's perm and keys."""
        if self.num_src != self.num_nodes or ct != chunk_tiles_for(self.num_edges) \
                or not (PLAN_KERNEL and self.edge_index.is_cuda) or self._small_built:
            return False
        if kind == "dst":
            return self._by_dst is not None and self._by_dst.perm.dtype == torch.int32    # (csr_plan has built the order)
        return kind == "run" and self.filter_state is None

    def csr_plan(self, by: str, chunk_tiles: int = 1) -> Optional[RunPlan]:
        """run-sum plan of the CSR order `by` in {"dst", "src"} (pangnn_decoder_dgrad_f32: perm = that CSR's perm)"""
        key = (by, int(chunk_tiles))
        if key not in self._plans:
            csr = self.by_dst if by == "dst" else self.by_src
            if key in self._plans:                       # (the small build, just triggered, made the plans too)
                return self._plans[key]
            n_rows = self.num_nodes if by == "dst" else self.num_src
            if not self.num_edges:
                self._plans[key] = None
            elif PLAN_KERNEL and csr.rowptr.is_cuda:
                self._plans[key] = self._plan_of_rowptr(csr.rowptr, self.num_edges, chunk_tiles,
                                                        csr.perm if self._streams(by, key[1]) else None)
            else:
                keys = self.edge_index[1 if by == "dst" else 0][csr.perm.long()]
                self._plans[key] = self._plan_of_sorted_keys(keys, n_rows, chunk_tiles)
        return self._plans[key]

    def runsum_plan(self, chunk_tiles: int = 1) -> Optional[RunPlan]:
        """If the caller's edge order is sorted by source: the plan of the per-(chunk, source) partial rows the decoder
        training kernels can emit (include/pangnn_hip.h, `part_buf` / `part_off`), else None."""
        if not self.sorted_by_src():
            return None
        ct = int(chunk_tiles)
        key = ("run", ct)
        if key not in self._plans:
            # a source-sorted list IS its by-source order (stable sort of a sorted list): the small build's ("src", ct) plan
            # is this plan
            self._small_build()              # no-op unless applicable and nothing is built yet
            small = self._plans.get(("src", ct)) if self._small_built else None
            if small is not None:
                self._plans[key] = small
            elif PLAN_KERNEL and self.edge_index.is_cuda:
                # the list is its own by-source order: that order's row pointer where it is held (a filtered child always
                # holds it), else the first entry of every source by one N-sized search of the sorted sources — no sort
                if self._by_src is not None:
                    rowptr = self._by_src.rowptr
                else:
                    src = self.edge_index[0]
                    rowptr = torch.searchsorted(src, torch.arange(self.num_src + 1, device=src.device, dtype=src.dtype))
                plan = self._plans[key] = self._plan_of_rowptr(rowptr, self.num_edges, ct)
                if self._streams("run", ct):
                    plan.stream = self._spos_of_sorted_list(self.edge_index, ct)
            else:
                self._plans[key] = self._plan_of_sorted_keys(self.edge_index[0], self.num_src, ct)
        return self._plans[key]

    def native_has(self, need: int, norm=None, x=None) -> bool:
        """everything `need` names is in the native registry already (as far as this object knows: the registry may have
        evicted it, in which case the op that misses it calls pangnn::_prepare_structure, i.e. push_native(force=True))"""
        if (self._native & need & (_STRUCT_BITS | NEED_PLAN_DST | NEED_PLAN_SRC)) != (need & (_STRUCT_BITS | NEED_PLAN_DST | NEED_PLAN_SRC)) \
                or not (self._native & NEED_ENTRY):
            return False
        nb = need & _NORM_BITS
        if not nb:
            return True
        if norm is None or (norm._native & nb & ~NEED_ACTIONS) != (nb & ~NEED_ACTIONS):
            return False
        return not (nb & NEED_ACTIONS) or (x is not None and norm._native_actions == (x.data_ptr(), x._version))

    def push_native(self, need: int, edge_weight: Optional[torch.Tensor] = None, x: Optional[torch.Tensor] = None,
                    force: bool = False):
        """Build (lazily, with the C entry points this class already uses) and push to the native structure registry
        (csrc/graph_ops.cpp) the components `need` names — NEED_* bits — so that the per-step ops `torch.ops.pangnn.
        {gcn_propagate, embed_conv_in[_linear], decoder_loss, decoder_mlp}` and their backward ops find them by the identity of
        `edge_index` (/ `edge_weight` / `x`) without entering Python.  Square structures only (a partitioned shard's
        rectangular structures take the ctypes route).  `force`: push again what this object believes is there (the
        registry evicts least-recently-used entries)."""
        if self.num_src != self.num_nodes:
            raise ValueError("the native registry holds square structures (whole graphs, collated batches)")
        from .torch_ops import ops
        ei, n, e = self._key_tensor, self.num_nodes, self.num_edges
        have = 0 if force else self._native
        ct = chunk_tiles_for(e)
        todo = need & _STRUCT_BITS & ~have
        if todo or not (have & NEED_ENTRY):
            by_dst, by_src, band, srt, plan = [], [], -1, -1, None
            short = self._small_built or self._vouched_short()
            if todo & NEED_BY_DST:
                c = self.by_dst
                by_dst = [c.rowptr, c.other, c.perm] + list(c.long_rows(short) or ())
            if todo & NEED_BY_SRC:
                c = self.by_src
                by_src = [c.rowptr, c.other, c.perm] + list(c.long_rows(short) or ())
            if todo & NEED_BAND:
                band = self.band_width()
            if todo & NEED_RUNSUM:
                plan = self.runsum_plan(ct)
                srt = 0 if plan is None else 1
            ops._register_structure(ei, n, self.num_src, self.edge_index, by_dst, by_src, band, srt)
            if plan is not None:
                ops._register_plan(ei, n, 0, ct, plan.part_off, plan.part_rowptr, plan.keys, int(plan.n_parts), plan.stream)
            have |= todo | NEED_ENTRY
        for bit, by, kind in ((NEED_PLAN_DST, "dst", 1), (NEED_PLAN_SRC, "src", 2)):
            if need & bit & ~have:
                if e:
                    plan = self.csr_plan(by, ct)
                    ops._register_plan(ei, n, kind, ct, plan.part_off, plan.part_rowptr, plan.keys, int(plan.n_parts), plan.stream)
                have |= bit
        self._native = have
        nb = need & _NORM_BITS
        if nb:
            norm = self.gcn_norm(edge_weight)
            nh = 0 if force else norm._native
            want_src = bool(nb & NEED_NORM_SRC)
            if (NEED_NORM & ~nh) or (want_src and (NEED_NORM_SRC & ~nh)):
                by_src = norm.by_src if want_src else norm._by_src
                ops._register_norm(ei, n, norm.weight_ref, norm.deg_inv_sqrt, norm.by_dst, norm.orig, by_src)
                nh |= NEED_NORM | (NEED_NORM_SRC if by_src is not None else 0)
            if nb & NEED_ACTIONS:
                if x is None:
                    raise ValueError("NEED_ACTIONS needs the feature tensor")
                key = (x.data_ptr(), x._version)
                if force or norm._native_actions != key:
                    from .functional import _node_actions
                    r, s_ = _node_actions(x, self, norm)
                    ops._register_actions(ei, n, norm.weight_ref, x, r, s_)
                    norm._native_actions = key
            norm._native = nh

    def gcn_norm(self, edge_weight: Optional[torch.Tensor], gather_dis=None) -> "GcnNorm":
        """norm for this edge_weight tensor (None = unit weights); cached on tensor identity.
        `gather_dis(dis_local [n_dst]) -> dis_src [n_src]` supplies the source nodes' deg^-1/2 for a
        partitioned shard (an all-gather); omitted for a whole graph."""
        key = None if edge_weight is None else (edge_weight.data_ptr(), edge_weight._version,
                                                tuple(edge_weight.shape))
        hit = self._norm.get(key)
        if hit is None:
            # the entry keeps `edge_weight` alive: a freed tensor's address can be handed to a new same-shape
            # tensor (fresh tensors all have _version 0), which would then match this key
            hit = (GcnNorm(self, edge_weight, gather_dis), edge_weight)
            hit[0].weight_ref = edge_weight              # the caller's tensor (cache key): the dispatcher ops pass it on
            if len(self._norm) >= 4:
                self._norm.pop(next(iter(self._norm)))
            self._norm[key] = hit
        return hit[0]


class GcnNorm:
    """k1-k3 of SURVEY.md §2.2: deg^-1/2[src] * w * deg^-1/2[dst], in both CSR orders."""

    def __init__(self, st: EdgeStructure, edge_weight: Optional[torch.Tensor], gather_dis=None):
        lib = _lib.load()
        dev = st.edge_index.device
        e, n = st.num_edges, st.num_nodes
        if edge_weight is not None:
            _lib.require_device(edge_weight)
            if edge_weight.dim() != 1 or edge_weight.shape[0] < e:
                raise ValueError(f"edge_weight must be [E>={e}], got {tuple(edge_weight.shape)}")
            edge_weight = edge_weight.detach().to(torch.float32).contiguous()
        self.weight = edge_weight               # the fp32 contiguous weights that were normalised (functional.propagate_w's backward)
        d = st.by_dst
        small = e <= (1 << 20)                  # small graphs: the by-source table too (a launch-bound step counts allocations)
        # one allocation: deg^-1/2, the norm in CSR(dst) order, in the caller's edge order, in CSR(src) order (filled on first use)
        self.deg_inv_sqrt, self.by_dst, self.orig, *rest = carve(torch.float32, dev, [n] + [e] * (3 if small else 2))
        self._by_src_buf = rest[0] if small else None
        with _lib.device_guard(dev):
            if gather_dis is None:
                if st.num_src != st.num_nodes:
                    raise ValueError("a rectangular structure needs gather_dis= for gcn_norm")
                _lib.check(lib.pangnn_gcn_norm_f32(d.rowptr.data_ptr(), _lib.ptr(d.other), _lib.ptr(d.perm),
                                                   _lib.ptr(edge_weight), n, e, self.deg_inv_sqrt.data_ptr(),
                                                   _lib.ptr(self.by_dst), _lib.ptr(self.orig),
                                                   _lib.stream_ptr()), "pangnn_gcn_norm_f32")
            else:
                _lib.check(lib.pangnn_gcn_degree_f32(d.rowptr.data_ptr(), _lib.ptr(d.perm), _lib.ptr(edge_weight),
                                                     n, self.deg_inv_sqrt.data_ptr(), _lib.stream_ptr()),
                           "pangnn_gcn_degree_f32")
                dis_src = gather_dis(self.deg_inv_sqrt).contiguous()
                assert dis_src.shape[0] >= st.num_src and dis_src.dtype == torch.float32
                _lib.check(lib.pangnn_gcn_edge_norm_f32(d.rowptr.data_ptr(), _lib.ptr(d.other), _lib.ptr(d.perm),
                                                        _lib.ptr(edge_weight), dis_src.data_ptr(),
                                                        self.deg_inv_sqrt.data_ptr(), n, e, _lib.ptr(self.by_dst),
                                                        _lib.ptr(self.orig), _lib.stream_ptr()),
                           "pangnn_gcn_edge_norm_f32")
        self._st = st
        self._by_src: Optional[torch.Tensor] = None
        self._native, self._native_actions = 0, None          # what the native registry holds of this normalisation
        self.weight_ref = None                                # the caller's tensor (set by EdgeStructure.gcn_norm)

    @property
    def by_src(self) -> torch.Tensor:
        """norm re-ordered into CSR(src) order (needed by the transposed propagate only)."""
        if self._by_src is None:
            st, lib = self._st, _lib.load()
            s = st.by_src
            out = self._by_src_buf if self._by_src_buf is not None else torch.empty_like(self.orig)
            with _lib.device_guard(out.device):
                _lib.check(lib.pangnn_permute_f32(_lib.ptr(self.orig), _lib.ptr(s.perm), _lib.ptr(out),
                                                  st.num_edges, _lib.stream_ptr()), "pangnn_permute_f32")
            self._by_src = out
        return self._by_src


# --------------------------------------------------------------------------------------
# structure cache: the reference passes raw tensors on every call, so memoise on identity
# --------------------------------------------------------------------------------------
_CACHE: Dict[Tuple, EdgeStructure] = {}
_CACHE_MAX = 16


def structure_key(edge_index: torch.Tensor, num_nodes: int):
    """identity of (edge_index tensor, node count): what the structure caches are keyed on"""
    return (edge_index.data_ptr(), edge_index._version, tuple(edge_index.shape), int(num_nodes), edge_index.device.index)


def structure_of(edge_index: torch.Tensor, num_nodes: int, holder=None, name: str = "") -> EdgeStructure:
    """EdgeStructure for `edge_index`.  If `holder` (a Data/Batch object) is given the structure is
    kept on it (`holder._pangnn_structs[name]`), otherwise in a small identity-keyed cache."""
    if torch.compiler.is_compiling():
        return TracedStructure(edge_index, num_nodes)
    key = structure_key(edge_index, num_nodes)
    if holder is not None:
        d = getattr(holder, "_pangnn_structs", None)
        if d is None:
            d = {}
            try:
                setattr(holder, "_pangnn_structs", d)
            except Exception:
                d = None
        if d is not None:
            hit = d.get(name)
            if hit is not None and hit[0] == key:
                return hit[1]
            hints = getattr(holder, "_pangnn_hints", None)
            st = EdgeStructure(edge_index, num_nodes, hints=None if hints is None else hints.get(name))
            d[name] = (key, st)
            register(st, key)
            return st
    hit = _CACHE.get(key)
    if hit is not None:
        return hit
    st = EdgeStructure(edge_index, num_nodes)
    if len(_CACHE) >= _CACHE_MAX:
        _CACHE.pop(next(iter(_CACHE)))
    _CACHE[key] = st
    return st


class TracedStructure:
    """What torch.compile sees of a graph while it traces the model: the tensors and the sizes, nothing built.  The
    dispatcher ops (torch_ops.py) take `edge_index` / `edge_weight` as tensors and look the real EdgeStructure / GcnNorm up
    by identity when the compiled graph RUNS (structure_of without a holder: the small global cache)."""
    traced = True

    def __init__(self, edge_index: torch.Tensor, num_nodes: int):
        self._key_tensor = self.edge_index = edge_index
        self.num_nodes = self.num_src = int(num_nodes)
        self.num_edges = edge_index.shape[1]

    def gcn_norm(self, edge_weight, gather_dis=None):
        return TracedNorm(edge_weight)


class TracedNorm:
    def __init__(self, edge_weight):
        self.weight_ref = edge_weight


def register(st, key=None):
    """make `st` the answer of structure_of(st.edge_index, st.num_nodes) without a holder (the dispatcher ops receive the
    raw tensors and look the structure up by identity)"""
    if getattr(st, "traced", False):
        return
    if key is None:
        key = structure_key(st._key_tensor, st.num_nodes)
    if _CACHE.get(key) is not st:
        if len(_CACHE) >= _CACHE_MAX:
            _CACHE.pop(next(iter(_CACHE)))
        _CACHE[key] = st


def clear_cache():
    for st in _CACHE.values():
        st._native = 0
    _CACHE.clear()
    from .torch_ops import ops
    ops._registry_clear(torch.empty(0))


def forget(key, edge_index: Optional[torch.Tensor] = None):
    """drop one entry of the identity-keyed cache (a buffer whose content was rewritten in place) — and, given the buffer,
    its entry of the native registry (same address, same version counter, new content)"""
    st = _CACHE.pop(key, None)
    if st is not None:
        st._native = 0
    if edge_index is not None and edge_index.is_cuda:
        from .torch_ops import ops
        ops._registry_forget(edge_index, int(key[3]))
