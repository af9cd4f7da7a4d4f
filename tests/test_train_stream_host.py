"""The position stream of the S pass's stream route (pangnn_csr_plan_spos, csrc/csr_plan.hip) and the host halves of its two
entry points.

The stream of a source-sorted list holds two words per position of whole 32-edge tiles, { src | closes << 31, dst }: `closes`
says that a part row ends behind the position.  `spos_expected` is the definition in numpy; the designed lists below (shared
with tests/test_train_stream.py) put run ends on, one before and one behind every half-tile, tile and chunk boundary, carry one
source across three chunks, leave sources without edges and fill half tiles with three and more runs — the CPU tests assert
that they do.  On a box without a GPU the entry points are called with fake pointers, as in test_c_abi_host.py."""
import functools

import numpy as np
import pytest
import torch

from pangnn_amd import _lib
from test_decoder_run_sums import chunk_tiles_expected, keys_from_starts, mixed_keys

no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: only where a missing check cannot reach a GPU")

F = 0x7f0000100000          # an aligned address that is never dereferenced
E_BADARG, E_TOOLARGE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -4
E = 60_000_000              # a list whose launch is the whole chip: the entry needs the full workspace query


# ------------------------------------------------------------------------------------------------------------------
# the definition, and the lists
# ------------------------------------------------------------------------------------------------------------------
def spos_expected(src, dst, span):
    """[P, 2] int64 words of non-negative value, P = 32 ceil(E / 32): a position past the list repeats the last edge; a part
    ends behind p where the source changes, at every span-th position and at the end of the last tile"""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    e = src.shape[0]
    padded = (e + 31) // 32 * 32
    p = np.arange(padded)
    k = np.minimum(p, e - 1)
    changes = np.zeros(padded, dtype=bool)
    changes[:e - 1] = src[1:] != src[:-1]
    closes = changes | ((p + 1) % span == 0) | (p + 1 == padded)
    return np.stack([src[k] | (closes.astype(np.int64) << 31), dst[k]], 1)


TINY = (1, 15, 16, 17, 31, 32, 33, 63, 65)                 # last-tile padding in both halves; 32 / 33: one chunk, and one more edge
DESIGNED = {"ct1": 6007, "ct2": (1 << 17) + 1, "ct16": (1 << 20) + 17}
LISTS = [f"E{e}" for e in TINY] + list(DESIGNED)


def boundary_marks(span):
    """positions at which a run is made to START: on, one before and one behind a half-tile, a tile and a chunk boundary, each
    in a chunk of its own (so the run before it ENDS at, one before and one behind the boundary's last position)"""
    marks = []
    for i, b in enumerate((16, 32, span)):
        for j, d in enumerate((-1, 0, 1)):
            marks.append((12 + 3 * i + j) * span + b + d)
    return marks


def long_run(span):
    """[first, last] positions of the run of one source that spans three chunks: it starts inside chunk 4, covers chunks 5 and
    6 whole and ends inside chunk 7"""
    return 4 * span + 7, 7 * span + 20


@functools.lru_cache(None)
def sorted_list(name):
    """(src, dst, n) int64 numpy / int: a source-sorted list"""
    if name in DESIGNED:
        e = DESIGNED[name]
        span = 32 * chunk_tiles_expected(e)
        k = mixed_keys(e)                                  # half tiles of every boundary pattern, three and more runs included
        start = np.concatenate([[True], k[1:] != k[:-1]])
        lo, hi = long_run(span)
        start[lo + 1:hi + 1] = False
        start[lo] = start[hi + 1] = True
        for m in boundary_marks(span):
            start[m - 2:m + 3] = False                     # the run around the mark is cut nowhere else nearby
            start[m] = True
        src = keys_from_starts(start)
        src = src + src // 7                               # every eighth source id has no edges
    else:
        e = int(name[1:])
        src = np.arange(e, dtype=np.int64) // 3 * 2        # runs of three, the odd ids empty
    n = int(src[-1]) + 3
    gen = torch.Generator().manual_seed(e)
    dst = torch.randint(0, n, (e,), generator=gen).numpy()
    return src, dst, n


def test_lists_select_their_chunk_sizes():
    L = _lib.load()
    assert [chunk_tiles_expected(DESIGNED[k]) for k in ("ct1", "ct2", "ct16")] == [1, 2, 16]
    for name in LISTS:
        e = sorted_list(name)[0].shape[0]
        assert L.pangnn_decoder_chunk_tiles_for(e) == chunk_tiles_expected(e)
    assert L.pangnn_decoder_chunk_tiles_for(32) == 1 and L.pangnn_decoder_chunk_tiles_for(33) == 1      # one chunk; one chunk + 1


@pytest.mark.parametrize("name", list(DESIGNED))
def test_designed_lists_have_the_designed_runs(name):
    src, dst, n = sorted_list(name)
    e = src.shape[0]
    span = 32 * chunk_tiles_expected(e)
    assert (np.diff(src) >= 0).all() and src[0] >= 0 and dst.min() >= 0 and dst.max() < n
    last = np.flatnonzero(np.concatenate([src[1:] != src[:-1], [True]]))           # last position of every run
    ends = set(last.tolist())
    for m in boundary_marks(span):
        assert m - 1 in ends and not ({m - 3, m - 2, m, m + 1} & ends)
    assert {(m - 1) % 16 for m in boundary_marks(span)} == {14, 15, 0} and span - 1 in {(m - 1) % span for m in boundary_marks(span)}
    lo, hi = long_run(span)
    assert src[lo] == src[hi] and src[lo - 1] != src[lo] and src[hi + 1] != src[hi] and hi // span - lo // span == 3
    assert np.bincount(last // 16).max() >= 3                                      # run_sums' LDS path
    assert np.bincount(last // 16, minlength=(e + 15) // 16).min() == 0            # ... and half tiles no run ends in
    assert np.bincount(src, minlength=n).min() == 0                                # sources without edges
    words = spos_expected(src, dst, span)
    assert words.shape == ((e + 31) // 32 * 32, 2) and (words[e:, 1] == dst[-1]).all()
    assert ((words[e:, 0] & 0x7fffffff) == src[-1]).all()
    # one close bit per part row of the list's own layout (a new part at every chunk start and every change of the source)
    starts = np.zeros(e, dtype=bool)
    starts[::span] = True
    starts[1:] |= src[1:] != src[:-1]
    assert int((words[:, 0] >> 31).sum()) == int(starts.sum())
    if e % 32:
        assert not (words[e - 1:-1, 0] >> 31).any() and words[-1, 0] >> 31           # the last run closes with the last tile


def test_definition_by_hand():
    w = spos_expected([0, 0, 2, 2, 2], [4, 3, 2, 1, 0], 32)
    assert w.shape == (32, 2)
    assert (w[:, 0] >> 31).tolist() == [0, 1, 0, 0] + [0] * 27 + [1]
    assert (w[:, 0] & 0x7fffffff).tolist() == [0, 0] + [2] * 30 and w[:, 1].tolist() == [4, 3, 2, 1] + [0] * 28
    w = spos_expected(np.zeros(96, dtype=np.int64), np.arange(96), 64)
    assert np.flatnonzero(w[:, 0] >> 31).tolist() == [63, 95]


# ------------------------------------------------------------------------------------------------------------------
# the kernel against the definition
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", LISTS)
def test_plan_spos_is_the_definition(name):
    from pangnn_amd.graph import EdgeStructure
    src, dst, n = sorted_list(name)
    e = src.shape[0]
    ct = chunk_tiles_expected(e)
    ei = torch.from_numpy(np.stack([src, dst])).cuda().contiguous()
    got = EdgeStructure._spos_of_sorted_list(ei, ct)
    assert got.dtype == torch.int32 and got.shape == ((e + 31) // 32 * 32, 2) and got.is_contiguous()
    want = torch.from_numpy(spos_expected(src, dst, 32 * ct)).cuda()
    assert torch.equal(got.long() & 0xffffffff, want)
    # a list held as two rows of a wider buffer (ld > E)
    wide = torch.full((2, e + 5), -1, dtype=torch.int64, device="cuda")
    wide[:, :e] = ei
    assert torch.equal(EdgeStructure._spos_of_sorted_list(wide[:, :e], ct), got)


# ------------------------------------------------------------------------------------------------------------------
# host halves
# ------------------------------------------------------------------------------------------------------------------
def test_binding_and_header_declare_them():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "pangnn_hip.h")).read()
    for name in ("pangnn_decoder_train_stream_f32", "pangnn_decoder_train_stream_mixed", "pangnn_csr_plan_spos"):
        assert name in _lib.SIGNATURES and re.search(r"\b" + name + r"\(", hdr)
    assert _lib.load().pangnn_abi_version() == _lib.ABI_VERSION        # additive: the number stays, every symbol is resolved


@no_gpu
def test_plan_spos_argument_checks():
    L = _lib.load()
    ok = lambda ei=F, ld=E, e=E, span=512, spos=F: L.pangnn_csr_plan_spos(ei, ld, e, span, spos, None)   # noqa: E731
    assert ok(e=0) == E_BADARG and ok(e=-3) == E_BADARG and ok(ld=E - 1) == E_BADARG
    assert ok(e=2 ** 31 - 1, ld=2 ** 31) == E_TOOLARGE and ok(e=2 ** 31 + 5, ld=2 ** 32) == E_TOOLARGE
    assert ok(span=0) == E_BADARG and ok(span=48) == E_BADARG and ok(span=-32) == E_BADARG
    assert ok(ei=None) == E_BADARG and ok(spos=None) == E_BADARG
    assert ok(ei=F + 4) == E_ALIGN and ok(spos=F + 4) == E_ALIGN


@no_gpu
def test_stream_entry_argument_checks():
    L = _lib.load()
    need = L.pangnn_decoder_train_workspace_bytes()
    assert need > 0

    def call(spos=F, parts=F, off=F, ws=F, b=need, e=E, ldp=64, ldq=64, dt=0, y=None, g=F, rec=F):
        return L.pangnn_decoder_train_stream_mixed(F, ldp, F, ldq, dt, 1000, spos, e, None, None, F, F, F, F, 64, y, None, 0, g,
                                                   None, None, rec, parts, off, F, F, F, None, ws, b, None)
    assert call(b=need - 1) == E_WORKSPACE and b"workspace" in L.pangnn_last_error().lower()
    assert call(b=0) == E_WORKSPACE and call(ws=None) == E_WORKSPACE
    assert call(b=-1) == E_BADARG
    assert call(spos=None) == E_BADARG                                 # the stream is required ...
    assert call(parts=None) == E_BADARG and call(off=None) == E_BADARG  # ... with both part tables
    assert call(spos=F + 4) == E_BADARG                                # word pairs are 8-byte aligned
    assert call(ldp=96) == E_BADARG and b"powers of two" in L.pangnn_last_error()         # 384-byte rows: the ids route's
    assert call(ldq=192) == E_BADARG and call(ldp=96, ldq=96, dt=1) == E_BADARG
    assert call(e=2 ** 31 + 5) == E_TOOLARGE and call(e=-1) == E_BADARG
    assert call(g=None) == E_BADARG and call(y=F) == E_BADARG          # exactly one of y / g_logits; the loss needs its outputs
    assert call(rec=None) == E_ALIGN
    assert L.pangnn_decoder_train_stream_f32(F, 64, F, 64, 1000, None, E, None, None, F, F, F, F, 64, None, None, 0, F, None, None,
                                             F, F, F, F, F, F, None, F, need, None) == E_BADARG
    # the ids entry is what it was: it needs the ids
    assert L.pangnn_decoder_train_mixed(F, 64, F, 64, 0, 1000, None, E, E, None, None, F, F, F, F, 64, None, None, 0, F, None, None,
                                        F, F, F, F, F, F, None, None, F, need, None) == E_BADARG
