// The exact-count mask of a random draw without a sort: keep[i] = 0 for exactly the k entries that come first in
// (key, index) order, 1 elsewhere (sampling.draw_keep_mask: one random 62-bit key per edge, the k smallest lose; the route
// this replaces is torch.topk of the k smallest keys plus an indexed store).
//
// A non-destructive radix select, most significant digit first: six passes of 11 bits cover the 63 key bits.  A pass streams
// the keys, counts the digit of those that still match the digits chosen so far in an LDS histogram (integer LDS atomics)
// and adds the workgroup's non-zero bins to a global histogram (integer global atomics: the sums do not depend on the
// order); a one-workgroup kernel then picks the bin that holds the k-th smallest key and the rank left inside it.  After
// the last pass the k-th smallest key T is known exactly, with r = the number of entries equal to T that lose (r >= 1).
// The mask pass writes  keep = key > T || (key == T && its rank among the equal keys, by index, >= r).  Only when the
// threshold key is tied with entries that stay (r < the number of equal keys — a 2^-62 event for the draw) are ranks needed:
// a counting pass over fixed contiguous ranges and a workgroup scan inside the mask pass, both skipped otherwise by a
// uniform branch on a device flag.  Nothing is read back and no result depends on an arrival order.
// The keys are only read.  Workspace: a few KB, independent of n.
#include "common.h"

namespace pangnn {
namespace {

constexpr int kSelBits = 11, kSelBins = 1 << kSelBits, kSelPasses = 6;       // 66 >= 63 bits
constexpr int kSelMaxBlocks = 1024;                                          // four workgroups per CU
constexpr int kSelStep = 4 * kBlock;                                         // entries per workgroup step of the mask pass

struct SelectState {
  uint64_t prefix;          // the digits chosen so far, in place; after the last pass the k-th smallest key
  int64_t k_rem;            // rank (from 1) of the k-th smallest key among the keys that match the prefix
  uint32_t in_bin;          // how many keys the chosen bin holds; after the last pass the number of keys equal to T
  uint32_t need_rank;       // after the last pass: in_bin != k_rem
};

constexpr size_t kSelStateBytes = 256, kSelHistBytes = kSelBins * 4, kSelCountBytes = kSelMaxBlocks * 4;
constexpr size_t kSelWorkspaceBytes = kSelStateBytes + kSelHistBytes + kSelCountBytes;

__global__ __launch_bounds__(kBlock) void select_hist_kernel(const int64_t* __restrict__ keys, int64_t n, int shift,
                                                             int first, const SelectState* __restrict__ st,
                                                             uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[kSelBins];
  for (int b = threadIdx.x; b < kSelBins; b += kBlock) h[b] = 0u;
  __syncthreads();
  const int above = first ? 0 : shift + kSelBits;                // (first pass: every key matches, nothing is shifted by 66)
  const uint64_t want = first ? 0u : st->prefix >> above;
  const int64_t pairs = n >> 1;
  const longlong2* __restrict__ k2 = reinterpret_cast<const longlong2*>(keys);
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < pairs; i += (int64_t)gridDim.x * kBlock) {
    const longlong2 v = k2[i];
    const uint64_t a = (uint64_t)v.x, b = (uint64_t)v.y;
    if (first || (a >> above) == want) atomicAdd(&h[(a >> shift) & (kSelBins - 1)], 1u);
    if (first || (b >> above) == want) atomicAdd(&h[(b >> shift) & (kSelBins - 1)], 1u);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const uint64_t a = (uint64_t)keys[n - 1];
    if (first || (a >> above) == want) atomicAdd(&h[(a >> shift) & (kSelBins - 1)], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < kSelBins; b += kBlock)
    if (h[b]) atomicAdd(&hist[b], h[b]);
}

// one workgroup: the bin of the k_rem-th smallest matching key; the histogram is cleared for the next pass
__global__ __launch_bounds__(kBlock) void select_bin_kernel(SelectState* __restrict__ st, uint32_t* __restrict__ hist,
                                                            int shift, int first, int is_last, int64_t k) {
  __shared__ uint32_t h[kSelBins];
  __shared__ uint32_t group[kBlock];
  constexpr int per = kSelBins / kBlock;
  const int tid = threadIdx.x;
  uint32_t sum = 0;
  for (int j = 0; j < per; ++j) {
    const uint32_t c = hist[tid * per + j];
    h[tid * per + j] = c;
    hist[tid * per + j] = 0u;
    sum += c;
  }
  group[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    const int64_t k_rem = first ? k : st->k_rem;
    const uint64_t prefix = first ? 0u : st->prefix;
    int64_t before = 0;
    int g = 0;
    while (g < kBlock - 1 && before + group[g] < k_rem) before += group[g++];
    int b = g * per;
    while (b < g * per + per - 1 && before + h[b] < k_rem) before += h[b++];
    st->prefix = prefix | ((uint64_t)b << shift);
    st->k_rem = k_rem - before;
    st->in_bin = h[b];
    st->need_rank = (is_last && (int64_t)h[b] != k_rem - before) ? 1u : 0u;
  }
}

// fixed contiguous ranges: workgroup b owns entries [b * chunk, (b + 1) * chunk), chunk a multiple of kSelStep
__global__ __launch_bounds__(kBlock) void select_count_equal_kernel(const int64_t* __restrict__ keys, int64_t n,
                                                                    int64_t chunk, const SelectState* __restrict__ st,
                                                                    uint32_t* __restrict__ block_count) {
  if (!st->need_rank) return;
  __shared__ uint32_t total;
  if (threadIdx.x == 0) total = 0u;
  __syncthreads();
  const int64_t t = (int64_t)st->prefix;
  const int64_t lo = blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
  uint32_t c = 0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kBlock) c += keys[i] == t ? 1u : 0u;
  if (c) atomicAdd(&total, c);
  __syncthreads();
  if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void select_mask_kernel(const int64_t* __restrict__ keys, int64_t n, int64_t chunk,
                                                             const SelectState* __restrict__ st,
                                                             const uint32_t* __restrict__ block_count,
                                                             uint8_t* __restrict__ keep) {
  __shared__ int64_t wave_sum[kWavesPerBlock];
  __shared__ int64_t base_sh;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int64_t t = (int64_t)st->prefix, r = st->k_rem;
  const bool ranks = st->need_rank != 0u;                        // uniform over the grid
  const int64_t lo = blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
  int64_t base = 0;                                              // equal keys before this step, by index
  if (ranks) {
    int64_t s = 0;
    for (int b = tid; b < (int)blockIdx.x; b += kBlock) s += block_count[b];
    for (int d = kWave / 2; d > 0; d >>= 1) s += __shfl_down(s, d, kWave);
    if (lane == 0) wave_sum[wave] = s;
    __syncthreads();
    if (tid == 0) {
      int64_t a = 0;
      for (int w = 0; w < kWavesPerBlock; ++w) a += wave_sum[w];
      base_sh = a;
    }
    __syncthreads();
    base = base_sh;
    __syncthreads();
  }
  for (int64_t i0 = lo; i0 < hi; i0 += kSelStep) {
    const int64_t i = i0 + 4 * tid;                              // four consecutive entries per thread
    int64_t v[4];
    if (i + 3 < hi) {
      const longlong2 a = *reinterpret_cast<const longlong2*>(keys + i), b = *reinterpret_cast<const longlong2*>(keys + i + 2);
      v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
    } else {
      for (int j = 0; j < 4; ++j) v[j] = i + j < hi ? keys[i + j] : INT64_MAX;
    }
    int64_t mine = 0;                                            // equal keys before this thread's entries, inside the step
    if (ranks) {
      int c = 0;
      for (int j = 0; j < 4; ++j) c += v[j] == t ? 1 : 0;
      int incl = c;
#pragma unroll
      for (int d = 1; d < kWave; d <<= 1) {
        const int up = __shfl_up(incl, d, kWave);
        if (lane >= d) incl += up;
      }
      if (lane == kWave - 1) wave_sum[wave] = incl;
      __syncthreads();
      mine = base + incl - c;
      int64_t step_total = 0;
      for (int w = 0; w < kWavesPerBlock; ++w) {
        if (w < wave) mine += wave_sum[w];
        step_total += wave_sum[w];
      }
      base += step_total;
      __syncthreads();
    }
    uint8_t o[4];
    for (int j = 0; j < 4; ++j) {
      bool loses = v[j] < t;
      if (v[j] == t) {
        loses = !ranks || mine < r;
        ++mine;
      }
      o[j] = loses ? 0 : 1;
    }
    if (i + 3 < hi) {
      *reinterpret_cast<uchar4*>(keep + i) = make_uchar4(o[0], o[1], o[2], o[3]);
    } else {
      for (int j = 0; j < 4; ++j)
        if (i + j < hi) keep[i + j] = o[j];
    }
  }
}

}  // namespace
}  // namespace pangnn

using namespace pangnn;

extern "C" int64_t pangnn_mask_k_smallest_workspace_bytes(int64_t n) {
  if (n < 0 || n >= ((int64_t)1 << 31)) return 0;
  return (int64_t)kSelWorkspaceBytes;
}

extern "C" int pangnn_mask_k_smallest_i64(const int64_t* keys, int64_t n, int64_t k, uint8_t* keep, void* workspace,
                                          int64_t workspace_bytes, pangnn_stream_t stream) {
  const char* name = "pangnn_mask_k_smallest_i64";
  PG_CHECK_ARG(n >= 0 && k >= 0 && k <= n, PANGNN_E_BADARG, "%s: bad size (n=%lld k=%lld: 0 <= k <= n)", name, (long long)n,
               (long long)k);
  PG_CHECK_ARG(n < ((int64_t)1 << 31), PANGNN_E_TOOLARGE, "%s: n must be below 2^31 (32-bit histogram counts)", name);
  PG_CHECK_ARG((keys && keep) || n == 0, PANGNN_E_BADARG, "%s: null keys / keep", name);
  PG_CHECK_ARG(workspace, PANGNN_E_BADARG, "%s: null workspace", name);
  PG_CHECK_ARG(aligned16(workspace) && aligned16(keys) && ((uintptr_t)keep & 3u) == 0, PANGNN_E_ALIGN,
               "%s: keys and workspace must be 16-byte aligned, keep 4-byte aligned", name);
  PG_CHECK_ARG(workspace_bytes >= (int64_t)kSelWorkspaceBytes, PANGNN_E_WORKSPACE, "%s: workspace too small (%lld < %zu)",
               name, (long long)workspace_bytes, kSelWorkspaceBytes);
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return 0;
  if (k == 0 || k == n) {                                       // nobody loses / everybody does: no key is read
    const hipError_t err = hipMemsetAsync(keep, k == 0 ? 1 : 0, (size_t)n, s);
    PG_CHECK_ARG(err == hipSuccess, (int)err, "%s: memset failed: %s", name, hipGetErrorString(err));
    return 0;
  }
  char* ws = static_cast<char*>(workspace);
  SelectState* st = reinterpret_cast<SelectState*>(ws);
  uint32_t* hist = reinterpret_cast<uint32_t*>(ws + kSelStateBytes);
  uint32_t* block_count = reinterpret_cast<uint32_t*>(ws + kSelStateBytes + kSelHistBytes);
  const hipError_t err = hipMemsetAsync(ws, 0, kSelWorkspaceBytes, s);
  PG_CHECK_ARG(err == hipSuccess, (int)err, "%s: memset failed: %s", name, hipGetErrorString(err));
  int64_t hist_blocks = ((n >> 1) + kBlock - 1) / kBlock;
  hist_blocks = hist_blocks < 1 ? 1 : (hist_blocks > kSelMaxBlocks ? kSelMaxBlocks : hist_blocks);
  for (int pass = 0; pass < kSelPasses; ++pass) {
    const int shift = (kSelPasses - 1 - pass) * kSelBits, first = pass == 0, is_last = pass == kSelPasses - 1;
    hipLaunchKernelGGL(select_hist_kernel, dim3((unsigned)hist_blocks), dim3(kBlock), 0, s, keys, n, shift, first, st, hist);
    PG_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(select_bin_kernel, dim3(1), dim3(kBlock), 0, s, st, hist, shift, first, is_last, k);
    PG_CHECK_LAUNCH(name);
  }
  int64_t chunk = (n + kSelMaxBlocks - 1) / kSelMaxBlocks;
  chunk = (chunk + kSelStep - 1) / kSelStep * kSelStep;
  const int64_t blocks = (n + chunk - 1) / chunk;
  hipLaunchKernelGGL(select_count_equal_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, keys, n, chunk, st, block_count);
  PG_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(select_mask_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, keys, n, chunk, st, block_count, keep);
  PG_CHECK_LAUNCH(name);
  return 0;
}
