// A structure derived by FILTERING: the edge list, the per-edge arrays and both CSR orders of a sub-sampled graph from the
// parent's tables, without a sort (sub_sample_graph_edges of the reference, src/helper.py:16-68, called per step at
// pangnn.py:190; semantics in pangnn_amd/sampling.py and DESIGN.md §2).
//
// Sub-sampling keeps the caller's edge order and pangnn_csr_build's radix sort is stable, so the child's sorted order is the
// parent's sorted order with the dropped entries squeezed out.  With
//     new_id = exclusive_scan(keep)             in the caller's order   (new_id[E] = number of kept edges)
//     pos    = exclusive_scan(keep[perm[i]])    in a CSR order          (pos[E]    = the same number)
// the child tables are   other'[pos[i]] = other[i],  perm'[pos[i]] = new_id[perm[i]]  for kept i,  rowptr'[r] = pos[rowptr[r]]:
// entry for entry what pangnn_csr_build makes of the child edge list.
//
// Per call: one rocPRIM scan + one launch for the edge list, one rocPRIM scan + one launch per CSR order.  The scans read
// their flags through transform iterators (`keep` at its stored width; the gather keep[perm[i]] happens inside the scan's
// load), both scans have E + 1 items so that the total is the last entry, and the passes behind them read "kept" off two
// neighbouring scan entries instead of gathering `keep` again.  Integer sums and plain stores to distinct addresses only:
// the result does not depend on the grid or the schedule.
//
// `num_kept` is the host's idea of the count and sizes every output; the device's count is written to `count`.  A write
// index is always checked against num_kept, the unwritten tail of a too-large num_kept is zero-filled (entries outside
// every row), and status bit 0 reports the mismatch — bit 1 a parent perm entry outside [0, E) or a parent rowptr entry
// outside [0, E] (the former is treated as dropped, the latter clamped).
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include "common.h"

namespace pangnn {
namespace {

constexpr int kFilterMaxBlocks = 2048;          // memory-bound streams: 8 workgroups per CU, grid-stride the rest

template <int ITEM>
__host__ __device__ __forceinline__ int32_t keep_at(const void* keep, int64_t i) {
  if constexpr (ITEM == 4) return static_cast<const uint32_t*>(keep)[i] != 0u ? 1 : 0;
  else return static_cast<const uint8_t*>(keep)[i] != 0 ? 1 : 0;
}

// item i of the caller-order scan: keep[i], 0 for the closing item i == E
template <int ITEM>
struct KeepFlag {
  const void* keep;
  int64_t e;
  __host__ __device__ int32_t operator()(int64_t i) const { return i < e ? keep_at<ITEM>(keep, i) : 0; }
};

// item i of a sorted-order scan: keep[perm[i]]; a perm entry outside [0, E) is never an address (status: scatter pass)
template <int ITEM>
struct KeepFlagOfSorted {
  const void* keep;
  const int32_t* perm;
  int64_t e;
  __host__ __device__ int32_t operator()(int64_t i) const {
    if (i >= e) return 0;
    const int64_t p = perm[i];
    return (uint64_t)p < (uint64_t)e ? keep_at<ITEM>(keep, p) : 0;
  }
};

template <class Flag>
hipError_t scan_flags(void* temp, size_t& temp_bytes, Flag flag, int32_t* out, int64_t items, hipStream_t s) {
  auto in = rocprim::make_transform_iterator(rocprim::make_counting_iterator<int64_t>(0), flag);
  return rocprim::exclusive_scan(temp, temp_bytes, in, out, (int32_t)0, (size_t)items, rocprim::plus<int32_t>(), s);
}

// rocPRIM's temporary storage for a scan of `items` flags read through `Flag` (size query only: nothing is launched)
template <class Flag>
size_t scan_temp_bytes(int64_t items) {
  size_t b = 0;
  if (scan_flags(nullptr, b, Flag{}, (int32_t*)nullptr, items, 0) != hipSuccess) return (size_t)-1;
  return b;
}

// Edge list, per-edge arrays and kept_id in the caller's order.  new_id [E + 1]; edge i is kept iff new_id[i + 1] != new_id[i].
__global__ __launch_bounds__(kBlock) void filter_edges_kernel(
    const int64_t* __restrict__ src, const int64_t* __restrict__ dst, const float* __restrict__ a0,
    const float* __restrict__ a1, const int32_t* __restrict__ new_id, int64_t e, int64_t num_kept,
    int64_t* __restrict__ c_src, int64_t* __restrict__ c_dst, float* __restrict__ c_a0, float* __restrict__ c_a1,
    int32_t* __restrict__ kept_id, int32_t* __restrict__ count, int32_t* __restrict__ status) {
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x, nthreads = (int64_t)gridDim.x * kBlock;
  const int64_t total = new_id[e];
  if (tid == 0) {
    *count = (int32_t)total;
    *status = total != num_kept ? 1 : 0;          // the first launch of the call: the order passes only OR bits in
  }
  for (int64_t i = tid; i < e; i += nthreads) {
    const int64_t j = new_id[i];
    if (new_id[i + 1] == j || j >= num_kept) continue;
    c_src[j] = src[i];
    c_dst[j] = dst[i];
    kept_id[j] = (int32_t)i;
    if (a0) c_a0[j] = a0[i];
    if (a1) c_a1[j] = a1[i];
  }
  for (int64_t j = total + tid; j < num_kept; j += nthreads) {      // fewer kept than claimed: a defined tail
    c_src[j] = 0;
    c_dst[j] = 0;
    kept_id[j] = 0;
    if (a0) c_a0[j] = 0.f;
    if (a1) c_a1[j] = 0.f;
  }
}

// One CSR order.  pos [E + 1]; sorted entry i is kept iff pos[i + 1] != pos[i].
__global__ __launch_bounds__(kBlock) void filter_order_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ other, const int32_t* __restrict__ perm,
    const int32_t* __restrict__ new_id, const int32_t* __restrict__ pos, int64_t e, int64_t n, int64_t num_kept,
    int64_t* __restrict__ c_rowptr, int32_t* __restrict__ c_other, int32_t* __restrict__ c_perm,
    int32_t* __restrict__ status) {
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x, nthreads = (int64_t)gridDim.x * kBlock;
  bool bad = false;
  for (int64_t i = tid; i < e; i += nthreads) {
    const int64_t p = pos[i], q = perm[i];
    if ((uint64_t)q >= (uint64_t)e) bad = true;
    if (pos[i + 1] == p || p >= num_kept) continue;      // (an entry with a bad perm has flag 0: never here)
    c_other[p] = other[i];
    const int64_t id = new_id[q];
    c_perm[p] = (int32_t)(id < num_kept ? id : num_kept - 1);      // (more kept than claimed: still a child edge id)
  }
  const int64_t total = pos[e];
  for (int64_t p = total + tid; p < num_kept; p += nthreads) {
    c_other[p] = 0;
    c_perm[p] = 0;
  }
  for (int64_t r = tid; r <= n; r += nthreads) {
    int64_t k = rowptr[r];
    if ((uint64_t)k > (uint64_t)e) {
      bad = true;
      k = k < 0 ? 0 : e;
    }
    const int64_t v = pos[k];
    c_rowptr[r] = v < num_kept ? v : num_kept;
  }
  if (bad) atomicOr(status, 2);
}

template <int ITEM>
int run_filter(const char* name, const int64_t* edge_index, int64_t ld, int64_t e, int64_t n, const void* keep,
               int64_t num_kept, const int64_t* const rowptr[2], const int32_t* const other[2],
               const int32_t* const perm[2], const float* a0, const float* a1, int64_t* c_edge_index, int64_t c_ld,
               int32_t* kept_id, float* c_a0, float* c_a1, int64_t* const c_rowptr[2], int32_t* const c_other[2],
               int32_t* const c_perm[2], int32_t* count, int32_t* status, int32_t* new_id, int32_t* pos, void* temp,
               size_t temp_bytes, hipStream_t s) {
  size_t tb = temp_bytes;
  hipError_t err = scan_flags(temp, tb, KeepFlag<ITEM>{keep, e}, new_id, e + 1, s);
  PG_CHECK_ARG(err == hipSuccess, (int)err, "%s: scan failed: %s", name, hipGetErrorString(err));
  const int64_t* dst = edge_index ? edge_index + ld : nullptr;            // (both may be null for an empty list)
  int64_t* c_dst = c_edge_index ? c_edge_index + c_ld : nullptr;
  hipLaunchKernelGGL(filter_edges_kernel, dim3(capped_grid(e > num_kept ? e : num_kept, kFilterMaxBlocks)), dim3(kBlock), 0, s,
                     edge_index, dst, a0, a1, new_id, e, num_kept, c_edge_index, c_dst, c_a0, c_a1, kept_id, count, status);
  PG_CHECK_LAUNCH(name);
  for (int o = 0; o < 2; ++o) {
    if (!rowptr[o]) continue;
    tb = temp_bytes;
    err = scan_flags(temp, tb, KeepFlagOfSorted<ITEM>{keep, perm[o], e}, pos, e + 1, s);
    PG_CHECK_ARG(err == hipSuccess, (int)err, "%s: scan failed: %s", name, hipGetErrorString(err));
    const int64_t work = e > n + 1 ? e : n + 1;
    hipLaunchKernelGGL(filter_order_kernel, dim3(capped_grid(work, kFilterMaxBlocks)), dim3(kBlock), 0, s, rowptr[o], other[o],
                       perm[o], new_id, pos, e, n, num_kept, c_rowptr[o], c_other[o], c_perm[o], status);
    PG_CHECK_LAUNCH(name);
  }
  return 0;
}

}  // namespace
}  // namespace pangnn

using namespace pangnn;

// workspace layout: [new_id (E + 1) * 4][pos (E + 1) * 4][rocPRIM temp], each on 256 bytes
extern "C" int64_t pangnn_structure_filter_workspace_bytes(int64_t num_edges) {
  if (num_edges < 0 || num_edges >= ((int64_t)1 << 31)) return 0;
  // (the size depends on the number and the type of the items, int32 for every scan of this file, not on the functor)
  const size_t t = scan_temp_bytes<KeepFlagOfSorted<4>>(num_edges + 1);
  if (t == (size_t)-1) return 0;
  return (int64_t)(2 * align_up((size_t)(num_edges + 1) * 4, 256) + align_up(t, 256));
}

extern "C" int pangnn_structure_filter(
    const int64_t* edge_index, int64_t ld, int64_t num_edges, int64_t num_nodes, const void* keep, int keep_itemsize,
    int64_t num_kept, const int64_t* rowptr_dst, const int32_t* other_dst, const int32_t* perm_dst,
    const int64_t* rowptr_src, const int32_t* other_src, const int32_t* perm_src, const float* attr0, const float* attr1,
    int64_t* child_edge_index, int64_t child_ld, int32_t* kept_id, float* child_attr0, float* child_attr1,
    int64_t* child_rowptr_dst, int32_t* child_other_dst, int32_t* child_perm_dst, int64_t* child_rowptr_src,
    int32_t* child_other_src, int32_t* child_perm_src, int32_t* count, int32_t* status, void* workspace,
    int64_t workspace_bytes, pangnn_stream_t stream) {
  const char* name = "pangnn_structure_filter";
  const int64_t e = num_edges, n = num_nodes;
  PG_CHECK_ARG(e >= 0 && n >= 0 && num_kept >= 0 && ld >= e && child_ld >= num_kept, PANGNN_E_BADARG,
               "%s: bad size (E=%lld N=%lld kept=%lld ld=%lld child ld=%lld)", name, (long long)e, (long long)n,
               (long long)num_kept, (long long)ld, (long long)child_ld);
  PG_CHECK_ARG(e < ((int64_t)1 << 31) && n < ((int64_t)1 << 31), PANGNN_E_TOOLARGE,
               "%s: E and N must be below 2^31 (int32 edge ids and positions)", name);
  PG_CHECK_ARG(num_kept <= e, PANGNN_E_BADARG, "%s: num_kept %lld of %lld edges", name, (long long)num_kept, (long long)e);
  PG_CHECK_ARG(keep_itemsize == 1 || keep_itemsize == 4, PANGNN_E_BADARG, "%s: keep_itemsize %d (1 or 4 bytes per edge)",
               name, keep_itemsize);
  PG_CHECK_ARG((keep && edge_index) || e == 0, PANGNN_E_BADARG, "%s: null keep / edge_index", name);
  PG_CHECK_ARG(count && status, PANGNN_E_BADARG, "%s: null count / status", name);
  PG_CHECK_ARG(rowptr_dst && child_rowptr_dst, PANGNN_E_BADARG, "%s: null by-target rowptr", name);
  PG_CHECK_ARG((other_dst && perm_dst) || e == 0, PANGNN_E_BADARG, "%s: null by-target other / perm", name);
  // (an empty graph's other / perm have no address: its rowptr alone says that the order is given)
  const int n_src = rowptr_src != nullptr ? 3 : 0;
  PG_CHECK_ARG(n_src ? (e == 0 || (other_src && perm_src)) : (!other_src && !perm_src), PANGNN_E_BADARG,
               "%s: the by-source rowptr / other / perm are given all three or not at all", name);
  PG_CHECK_ARG(n_src == 0 || child_rowptr_src, PANGNN_E_BADARG, "%s: null child by-source rowptr", name);
  // (an output of num_kept == 0 entries has no address)
  PG_CHECK_ARG((attr0 ? (child_attr0 || num_kept == 0) : !child_attr0) && (attr1 ? (child_attr1 || num_kept == 0) : !child_attr1),
               PANGNN_E_BADARG, "%s: a per-edge array and its compacted output go together", name);
  PG_CHECK_ARG(num_kept == 0 || (child_edge_index && kept_id && child_other_dst && child_perm_dst &&
                                 (n_src == 0 || (child_other_src && child_perm_src))),
               PANGNN_E_BADARG, "%s: null output", name);
  PG_CHECK_ARG(workspace, PANGNN_E_BADARG, "%s: null workspace", name);
  PG_CHECK_ARG(aligned16(workspace), PANGNN_E_ALIGN, "%s: workspace must be 16-byte aligned", name);
  const uintptr_t p8 = (uintptr_t)edge_index | (uintptr_t)child_edge_index | (uintptr_t)rowptr_dst |
                       (uintptr_t)rowptr_src | (uintptr_t)child_rowptr_dst | (uintptr_t)child_rowptr_src;
  const uintptr_t p4 = (uintptr_t)other_dst | (uintptr_t)perm_dst | (uintptr_t)other_src | (uintptr_t)perm_src |
                       (uintptr_t)attr0 | (uintptr_t)attr1 | (uintptr_t)kept_id | (uintptr_t)child_attr0 |
                       (uintptr_t)child_attr1 | (uintptr_t)child_other_dst | (uintptr_t)child_perm_dst |
                       (uintptr_t)child_other_src | (uintptr_t)child_perm_src | (uintptr_t)count | (uintptr_t)status |
                       (keep_itemsize == 4 ? (uintptr_t)keep : 0);
  PG_CHECK_ARG((p8 & 7u) == 0 && (p4 & 3u) == 0, PANGNN_E_ALIGN, "%s: a pointer is not aligned to its element size", name);
  const size_t seg = align_up((size_t)(e + 1) * 4, 256);
  const size_t temp = keep_itemsize == 1 ? scan_temp_bytes<KeepFlagOfSorted<1>>(e + 1)
                                         : scan_temp_bytes<KeepFlagOfSorted<4>>(e + 1);
  PG_CHECK_ARG(temp != (size_t)-1, PANGNN_E_BADARG, "%s: rocPRIM size query failed", name);
  PG_CHECK_ARG(workspace_bytes >= 0 && (size_t)workspace_bytes >= 2 * seg + align_up(temp, 256), PANGNN_E_WORKSPACE,
               "%s: workspace too small (%lld < %zu)", name, (long long)workspace_bytes, 2 * seg + align_up(temp, 256));
  char* ws = static_cast<char*>(workspace);
  int32_t* new_id = reinterpret_cast<int32_t*>(ws);
  int32_t* pos = reinterpret_cast<int32_t*>(ws + seg);
  void* tmp = ws + 2 * seg;
  const int64_t* const rowptr[2] = {rowptr_dst, rowptr_src};
  const int32_t* const other[2] = {other_dst, other_src};
  const int32_t* const perm[2] = {perm_dst, perm_src};
  int64_t* const c_rowptr[2] = {child_rowptr_dst, child_rowptr_src};
  int32_t* const c_other[2] = {child_other_dst, child_other_src};
  int32_t* const c_perm[2] = {child_perm_dst, child_perm_src};
  hipStream_t s = (hipStream_t)stream;
  if (keep_itemsize == 1)
    return run_filter<1>(name, edge_index, ld, e, n, keep, num_kept, rowptr, other, perm, attr0, attr1, child_edge_index,
                         child_ld, kept_id, child_attr0, child_attr1, c_rowptr, c_other, c_perm, count, status, new_id, pos,
                         tmp, align_up(temp, 256), s);
  return run_filter<4>(name, edge_index, ld, e, n, keep, num_kept, rowptr, other, perm, attr0, attr1, child_edge_index,
                       child_ld, kept_id, child_attr0, child_attr1, c_rowptr, c_other, c_perm, count, status, new_id, pos,
                       tmp, align_up(temp, 256), s);
}
