// Everything an epoch keeps of one batch's logits, folded into device state by one capturable call (pangnn_batch_stats_f32):
// confusion counts at a device-resident threshold, the batch's mean BCEWithLogits(pos_weight) loss (or a loss handed in), and
// the raw logits / labels appended to the buffers the ranking metrics are computed from at the end of the pass
// (pangnn.py:218-222, 241-289).  The batch may be a padded fixed-shape one: only the first live[0] entries are read.
//
// No float atomics and nothing handed from workgroup to workgroup inside a launch:
//   n_max <= kSmallMaxEdges   ONE workgroup of kSumThreads threads does all of it (what a collated mini-batch is);
//   above                     up to kStatsBlocks workgroups write per-workgroup partials (and copy their slice of the logits
//                             behind the OLD cursor, which nobody moves in that launch); a one-workgroup finish kernel adds the
//                             partials in index order and updates the state.
// A thread adds its terms (fp32, the shared bce_term) in float64 in ascending index order; a workgroup adds its threads by the
// xor butterfly per wave and the waves in order: a fixed order, the same bits in every run.
#include "common.h"

namespace pangnn {

constexpr int kStatsBlocks = 1024;

struct StatsPart {
  double loss;
  unsigned long long c[4];
};

// state words (include/pangnn_hip.h): counts[4], batches, cursor, overflow, loss_sum (double), last_loss (float, low half)
constexpr int kStBatches = 4, kStCursor = 5, kStOverflow = 6, kStLossSum = 7, kStLastLoss = 8;

// number of real entries: live[0], or n_max where there is no count or the count is not one
__device__ __forceinline__ int64_t live_count(const int64_t* __restrict__ live, int64_t n_max) {
  if (!live) return n_max;
  const int64_t m = live[0];
  return (m < 0 || m > n_max) ? n_max : m;
}

// whether m more entries fit behind the cursor (a cursor that is no position of the buffer fits nothing)
__device__ __forceinline__ bool append_fits(int64_t cursor, int64_t m, int64_t cap) {
  return cursor >= 0 && cursor <= cap && m <= cap - cursor;
}

// a thread's share of entries [0, m): first, first + stride, ...  Counts, loss terms (unless a loss is handed in) and the copy.
__device__ __forceinline__ void stats_slice(const float* __restrict__ x, const float* __restrict__ y, int64_t m, int64_t first,
                                            int64_t stride, float pw, float threshold, bool want_loss,
                                            float* __restrict__ scores, uint8_t* __restrict__ slabels, StatsPart& part) {
  unsigned int c[4] = {0u, 0u, 0u, 0u};        // (one thread sees fewer than 2^32 entries: n_max < 2^40, checked on the host)
  double loss = 0.0;
  for (int64_t i = first; i < m; i += stride) {
    const float xv = x[i], yv = y[i];
    const int lab = label_positive(yv) ? 1 : 0;
    c[2 * lab + (predicted_positive(xv, threshold, true) ? 1 : 0)] += 1u;
    if (want_loss) loss += (double)bce_term(xv, yv, pw);
    if (scores) {
      scores[i] = xv;
      slabels[i] = (uint8_t)lab;
    }
  }
  part.loss = loss;
#pragma unroll
  for (int k = 0; k < 4; ++k) part.c[k] = c[k];
}

// sum of the workgroup's parts, valid in thread 0: butterfly inside a wave, waves in order
template <int THREADS>
__device__ __forceinline__ StatsPart block_total(StatsPart p) {
  __shared__ StatsPart red[THREADS / kWave];
  p.loss = wave_sum(p.loss);
#pragma unroll
  for (int k = 0; k < 4; ++k) p.c[k] = wave_sum(p.c[k]);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x >> 6] = p;
  __syncthreads();
  StatsPart t = {0.0, {0ull, 0ull, 0ull, 0ull}};
  if (threadIdx.x == 0) {
    for (int w = 0; w < THREADS / kWave; ++w) {
      t.loss += red[w].loss;
#pragma unroll
      for (int k = 0; k < 4; ++k) t.c[k] += red[w].c[k];
    }
  }
  return t;
}

// one thread folds a batch's totals into the state; `cursor` is the value every workgroup read
__device__ __forceinline__ void stats_apply(int64_t* __restrict__ state, const StatsPart& t, int64_t m, int64_t cursor,
                                            const float* __restrict__ loss_in, bool ranking, int64_t cap) {
  if (m <= 0) return;                                       // an empty batch adds nothing and is not counted
#pragma unroll
  for (int k = 0; k < 4; ++k) state[k] += (int64_t)t.c[k];
  const double l = loss_in ? (double)loss_in[0] : t.loss / (double)m;
  double* loss_sum = reinterpret_cast<double*>(state + kStLossSum);
  *loss_sum += l;
  *reinterpret_cast<float*>(state + kStLastLoss) = loss_in ? loss_in[0] : (float)l;
  state[kStBatches] += 1;
  if (ranking) {
    if (append_fits(cursor, m, cap)) state[kStCursor] = cursor + m;
    else state[kStOverflow] = 1;
  }
}

__global__ __launch_bounds__(kSumThreads) void batch_stats_small_kernel(
    const float* __restrict__ x, const float* __restrict__ y, int64_t n_max, const int64_t* __restrict__ live,
    const float* __restrict__ pos_weight, const float* __restrict__ threshold, const float* __restrict__ loss_in,
    int64_t* __restrict__ state, float* __restrict__ scores, uint8_t* __restrict__ slabels, int64_t cap) {
  const int64_t m = live_count(live, n_max);
  const int64_t cursor = state[kStCursor];                  // read by every thread before the barrier thread 0 writes behind
  const bool append = scores && append_fits(cursor, m, cap);
  StatsPart p;
  stats_slice(x, y, m, threadIdx.x, kSumThreads, pos_weight ? pos_weight[0] : 1.f, threshold[0], !loss_in,
              append ? scores + cursor : nullptr, append ? slabels + cursor : nullptr, p);
  const StatsPart t = block_total<kSumThreads>(p);
  if (threadIdx.x == 0) stats_apply(state, t, m, cursor, loss_in, scores != nullptr, cap);
}

// the state is only read here: the finish kernel is the one that moves the cursor
__global__ __launch_bounds__(kBlock) void batch_stats_parts_kernel(
    const float* __restrict__ x, const float* __restrict__ y, int64_t n_max, const int64_t* __restrict__ live,
    const float* __restrict__ pos_weight, const float* __restrict__ threshold, int want_loss,
    const int64_t* __restrict__ state, float* __restrict__ scores, uint8_t* __restrict__ slabels, int64_t cap,
    StatsPart* __restrict__ parts) {
  const int64_t m = live_count(live, n_max);
  const int64_t cursor = state[kStCursor];
  const bool append = scores && append_fits(cursor, m, cap);
  StatsPart p;
  stats_slice(x, y, m, (int64_t)blockIdx.x * kBlock + threadIdx.x, (int64_t)gridDim.x * kBlock,
              pos_weight ? pos_weight[0] : 1.f, threshold[0], want_loss != 0, append ? scores + cursor : nullptr,
              append ? slabels + cursor : nullptr, p);
  const StatsPart t = block_total<kBlock>(p);
  if (threadIdx.x == 0) parts[blockIdx.x] = t;
}

__global__ __launch_bounds__(kSumThreads) void batch_stats_finish_kernel(
    const StatsPart* __restrict__ parts, int n_parts, int64_t n_max, const int64_t* __restrict__ live,
    const float* __restrict__ loss_in, int64_t* __restrict__ state, int ranking, int64_t cap) {
  StatsPart p = {0.0, {0ull, 0ull, 0ull, 0ull}};
  if ((int)threadIdx.x < n_parts) p = parts[threadIdx.x];   // n_parts <= kStatsBlocks == kSumThreads
  const StatsPart t = block_total<kSumThreads>(p);
  if (threadIdx.x == 0) stats_apply(state, t, live_count(live, n_max), state[kStCursor], loss_in, ranking != 0, cap);
}

static_assert(kStatsBlocks <= kSumThreads, "the finish kernel reads one part per thread");

}  // namespace pangnn

using namespace pangnn;

extern "C" int64_t pangnn_batch_stats_workspace_bytes(int64_t n_max) {
  return n_max > kSmallMaxEdges ? (int64_t)(kStatsBlocks * sizeof(StatsPart)) : 0;
}

extern "C" int pangnn_batch_stats_f32(const float* logits, const float* labels, int64_t n_max, const int64_t* live,
                                      const float* pos_weight, const float* threshold, const float* loss_in,
                                      int64_t* state, float* scores, uint8_t* score_labels, int64_t cap, void* workspace,
                                      int64_t workspace_bytes, pangnn_stream_t stream) {
  PG_CHECK_ARG(logits && labels && state && threshold, PANGNN_E_BADARG, "pangnn_batch_stats_f32: null pointer");
  PG_CHECK_ARG(n_max >= 0, PANGNN_E_BADARG, "pangnn_batch_stats_f32: negative size");
  PG_CHECK_ARG(cap >= 0 && (cap == 0 || (scores && score_labels)), PANGNN_E_BADARG,
               "pangnn_batch_stats_f32: negative capacity, or a capacity without its buffers");
  PG_CHECK_ARG(n_max < ((int64_t)1 << 40), PANGNN_E_TOOLARGE, "pangnn_batch_stats_f32: n_max too large");
  PG_CHECK_ARG((reinterpret_cast<uintptr_t>(state) & 7u) == 0, PANGNN_E_ALIGN, "pangnn_batch_stats_f32: state must be 8-byte aligned");
  const int64_t need = pangnn_batch_stats_workspace_bytes(n_max);
  PG_CHECK_ARG(need == 0 || (workspace && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0),
               PANGNN_E_WORKSPACE, "pangnn_batch_stats_f32: workspace too small (%lld < %lld)", (long long)workspace_bytes,
               (long long)need);
  if (n_max == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (cap == 0) scores = nullptr, score_labels = nullptr;   // no ranking data: nothing is appended and nothing can overflow
  if (n_max <= kSmallMaxEdges) {
    hipLaunchKernelGGL(batch_stats_small_kernel, dim3(1), dim3(kSumThreads), 0, s, logits, labels, n_max, live, pos_weight,
                       threshold, loss_in, state, scores, score_labels, cap);
    PG_CHECK_LAUNCH("pangnn_batch_stats_f32");
    return 0;
  }
  const int blocks = (int)capped_grid(n_max, kStatsBlocks);
  StatsPart* parts = static_cast<StatsPart*>(workspace);
  hipLaunchKernelGGL(batch_stats_parts_kernel, dim3(blocks), dim3(kBlock), 0, s, logits, labels, n_max, live, pos_weight,
                     threshold, loss_in ? 0 : 1, static_cast<const int64_t*>(state), scores, score_labels, cap, parts);
  PG_CHECK_LAUNCH("pangnn_batch_stats_f32(parts)");
  hipLaunchKernelGGL(batch_stats_finish_kernel, dim3(1), dim3(kSumThreads), 0, s, static_cast<const StatsPart*>(parts), blocks,
                     n_max, live, loss_in, state, scores ? 1 : 0, cap);
  PG_CHECK_LAUNCH("pangnn_batch_stats_f32(finish)");
  return 0;
}
