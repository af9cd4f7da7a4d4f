// Connected components of the kept (predicted) edges: the on-device half of write_groups_file (src/postprocessing.py:5-36,
// which the reference calls commented out at pangnn.py:375 because its set-merging loop cannot work; the semantics are
// defined in pangnn_amd/postprocessing.py and DESIGN.md §2).  labels[v] = the smallest node id of v's component of the
// undirected graph of kept edges, touched[v] = some kept edge has v as an endpoint.
//
// A lock-free union-find over the label array itself, in three launches: init (labels[v] = v), hook (one pass over the
// edges), compress (every node stores its root).  The invariant, held by every write of every launch:
//
//     labels[x] <= x at all times, a word only ever decreases, and labels[x] is a node of x's own tree.
//
// A root is a node with labels[r] == r.  The hook pass changes a word in two ways only: an atomicCAS that replaces a ROOT's
// own id by a smaller id of the tree it joins, and the path halving of find, an atomicMin of a non-root's word with its
// grandparent.  Neither can raise a word or make a non-root a root, so pointers strictly descend towards the root (no
// cycle, every find ends), a failed CAS returns a strictly smaller id to go on from (the loop ends), and the one root left
// in a component once all its edges are joined has nothing smaller to point to: it is the component's smallest id, whatever
// the order of edges, the grid or the schedule.  One edge pass therefore suffices and the result is canonical.
// A read of labels that returns an older value is harmless for the same reason: an old value is still a node of the same
// tree with a smaller id, and what decides a join is the CAS on the word itself.  Reads go through relaxed agent-scope
// atomic loads, so that the compiler keeps them inside the loops and one CU's L1 never serves another CU's old line.
//
// Integer atomics only, no float, no inline assembly.
#include "common.h"

namespace pangnn {
namespace {

// 2048 blocks x 4 waves = 8 waves per SIMD on 256 CUs: the joins are chains of dependent L2 reads, hidden by occupancy
constexpr int kCompMaxBlocks = 2048;

__device__ __forceinline__ int32_t label_load(const int32_t* labels, int32_t x) {
  return __hip_atomic_load(&labels[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x's tree; every visited node's word is lowered to its grandparent on the way (path halving)
__device__ __forceinline__ int32_t find_root(int32_t* labels, int32_t x) {
  int32_t p = label_load(labels, x);
  while (p != x) {
    const int32_t gp = label_load(labels, p);
    if (gp == p) return p;
    atomicMin(&labels[x], gp);          // gp < p < x: lowers the word, never makes x a root
    x = p;
    p = gp;
  }
  return x;
}

__device__ __forceinline__ void join(int32_t* labels, int32_t u, int32_t v) {
  for (;;) {
    u = find_root(labels, u);
    v = find_root(labels, v);
    if (u == v) return;
    if (u < v) {
      const int32_t t = u;
      u = v;
      v = t;
    }
    const int32_t old = atomicCAS(&labels[u], u, v);      // the larger root onto the smaller id
    if (old == u) return;
    u = old;                                              // u had been hooked meanwhile: go on from its parent (< u)
  }
}

__device__ __forceinline__ void join_edge(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int64_t e,
                                          int32_t n, int32_t* labels, uint8_t* touched, int32_t* status) {
  const int64_t u = src[e], v = dst[e];
  if ((uint64_t)u >= (uint64_t)n || (uint64_t)v >= (uint64_t)n) {      // never an address
    __hip_atomic_store(status, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  if (touched) {
    touched[u] = 1;
    touched[v] = 1;
  }
  if (u != v) join(labels, (int32_t)u, (int32_t)v);
}

__global__ __launch_bounds__(kBlock) void components_init_kernel(int32_t n, int32_t* __restrict__ labels,
                                                                 uint8_t* __restrict__ touched,
                                                                 int32_t* __restrict__ status) {
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x, nthreads = (int64_t)gridDim.x * kBlock;
  if (tid == 0) *status = 0;
  for (int64_t v = tid; v < n; v += nthreads) {
    labels[v] = (int32_t)v;
    if (touched) touched[v] = 0;
  }
}

// ITEM = bytes of one keep entry (0: no selection).  `vec`: keep is 16-byte aligned, and a thread reads 16 bytes of it at
// a time (16 / ITEM edges); the edges behind the last whole 16 bytes, or all of them without `vec`, are read one by one.
template <int ITEM>
__global__ __launch_bounds__(kBlock) void components_hook_kernel(const int64_t* __restrict__ src,
                                                                 const int64_t* __restrict__ dst,
                                                                 const void* __restrict__ keep, int vec, int64_t num_edges,
                                                                 int32_t n, int32_t* labels, uint8_t* touched,
                                                                 int32_t* status) {
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x, nthreads = (int64_t)gridDim.x * kBlock;
  if constexpr (ITEM == 0) {
    for (int64_t e = tid; e < num_edges; e += nthreads) join_edge(src, dst, e, n, labels, touched, status);
  } else {
    constexpr int kPer = 16 / ITEM;
    const int64_t nchunk = vec ? num_edges / kPer : 0;
    const uint4* __restrict__ kv = static_cast<const uint4*>(keep);
    for (int64_t c = tid; c < nchunk; c += nthreads) {
      const uint4 q = kv[c];
      if ((q.x | q.y | q.z | q.w) == 0u) continue;
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (w[k] == 0u) continue;
        if constexpr (ITEM == 4) {
          join_edge(src, dst, c * 4 + k, n, labels, touched, status);
        } else {
#pragma unroll
          for (int b = 0; b < 4; ++b)
            if ((w[k] >> (8 * b)) & 0xffu) join_edge(src, dst, c * 16 + 4 * k + b, n, labels, touched, status);
        }
      }
    }
    for (int64_t e = nchunk * kPer + tid; e < num_edges; e += nthreads) {
      bool on;
      if constexpr (ITEM == 4) on = static_cast<const uint32_t*>(keep)[e] != 0u;
      else on = static_cast<const uint8_t*>(keep)[e] != 0;
      if (on) join_edge(src, dst, e, n, labels, touched, status);
    }
  }
}

// Every node walks to its root (halving on the way, so that a deep chain is shortened by all its walkers together: a path
// hooked link by link is N deep) and stores it.  No root changes here, so a concurrent walker reads either a node's old
// ancestor or its root.
__global__ __launch_bounds__(kBlock) void components_compress_kernel(int32_t n, int32_t* labels) {
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x, nthreads = (int64_t)gridDim.x * kBlock;
  for (int64_t v = tid; v < n; v += nthreads) {
    const int32_t r = find_root(labels, (int32_t)v);
    if (r != (int32_t)v) atomicMin(&labels[v], r);
  }
}

}  // namespace
}  // namespace pangnn

extern "C" int pangnn_components_i32(const int64_t* src, const int64_t* dst, const void* keep, int keep_itemsize,
                                     int64_t num_edges, int64_t num_nodes, int32_t* labels, uint8_t* touched,
                                     int32_t* status, pangnn_stream_t stream) {
  using namespace pangnn;
  const char* name = "pangnn_components_i32";
  PG_CHECK_ARG(num_edges >= 0 && num_nodes >= 0, PANGNN_E_BADARG, "%s: negative size", name);
  PG_CHECK_ARG(keep_itemsize == 0 || keep_itemsize == 1 || keep_itemsize == 4, PANGNN_E_BADARG,
               "%s: keep_itemsize %d (0: no selection, 1 or 4 bytes per edge)", name, keep_itemsize);
  PG_CHECK_ARG(keep_itemsize == 0 || keep != nullptr, PANGNN_E_BADARG, "%s: keep_itemsize %d with a null keep", name,
               keep_itemsize);
  PG_CHECK_ARG(num_nodes < ((int64_t)1 << 31), PANGNN_E_TOOLARGE, "%s: int32 labels cannot name %lld nodes", name,
               (long long)num_nodes);
  PG_CHECK_ARG(status != nullptr, PANGNN_E_BADARG, "%s: null status", name);
  PG_CHECK_ARG(labels != nullptr || num_nodes == 0, PANGNN_E_BADARG, "%s: null labels", name);
  PG_CHECK_ARG((src != nullptr && dst != nullptr) || num_edges == 0, PANGNN_E_BADARG, "%s: null edge list", name);
  hipStream_t s = (hipStream_t)stream;
  const int32_t n = (int32_t)num_nodes;
  hipLaunchKernelGGL(components_init_kernel, dim3(capped_grid(num_nodes, kCompMaxBlocks)), dim3(kBlock), 0, s, n, labels,
                     touched, status);
  PG_CHECK_LAUNCH(name);
  if (num_edges == 0) return 0;
  const int vec = keep_itemsize != 0 && aligned16(keep);
  const int64_t work = keep_itemsize && vec ? (num_edges + 16 / keep_itemsize - 1) / (16 / keep_itemsize) : num_edges;
  const dim3 grid(capped_grid(work, kCompMaxBlocks));
  if (keep_itemsize == 0)
    hipLaunchKernelGGL(components_hook_kernel<0>, grid, dim3(kBlock), 0, s, src, dst, nullptr, 0, num_edges, n, labels,
                       touched, status);
  else if (keep_itemsize == 1)
    hipLaunchKernelGGL(components_hook_kernel<1>, grid, dim3(kBlock), 0, s, src, dst, keep, vec, num_edges, n, labels,
                       touched, status);
  else
    hipLaunchKernelGGL(components_hook_kernel<4>, grid, dim3(kBlock), 0, s, src, dst, keep, vec, num_edges, n, labels,
                       touched, status);
  PG_CHECK_LAUNCH(name);
  if (num_nodes == 0) return 0;
  hipLaunchKernelGGL(components_compress_kernel, dim3(capped_grid(num_nodes, kCompMaxBlocks)), dim3(kBlock), 0, s, n, labels);
  PG_CHECK_LAUNCH(name);
  return 0;
}
