// Max-candidate labelling ("best hit per genome"): the baselines of src/helper.py:437-485 (calculate_baseline_labels) and
// src/helper.py:494-576 (calculate_logit_baseline_labels / find_max_logit), which the reference runs as Python dict loops
// over every edge.  An edge is labelled 1 when no other candidate of its source in its target's genome has a larger value
// (the reference's strict `<`): label = isnan(v) | (v >= max of the segment's non-NaN values).
//
// Segments are the (source, candidate genome) groups that construct.normalize_sim_scores also builds for the Q-score
// softmax.  One wave per segment, lanes stride the segment; the grid is bounded and waves walk segments grid-stride so
// that the fused confusion counts cost one integer atomic per block per count.  No float atomics: labels are exact and
// the counts are integer sums, so the whole result is independent of scheduling.
#include "common.h"

namespace pangnn {
namespace {

// 8192 blocks x 4 waves = 32 768 waves: 32 per SIMD on 256 CUs x 4 SIMDs, i.e. four rounds at the 8-wave occupancy limit.
// Bounding the grid bounds the count atomics (one per block per count) at 32 768 in all.
constexpr int kCandMaxBlocks = 8192;

template <typename T>
__device__ __forceinline__ T neg_inf();
template <>
__device__ __forceinline__ float neg_inf<float>() { return -INFINITY; }
template <>
__device__ __forceinline__ double neg_inf<double>() { return -(double)INFINITY; }

// c[k] (valid in every lane) += number of lanes whose (label, prediction) pair is k, for the lanes with `on` set
__device__ __forceinline__ void count_lanes(bool on, bool lab, bool pred, unsigned int c[4]) {
  const unsigned long long l1 = __ballot(on && lab), p1 = __ballot(on && pred), all = __ballot(on);
  const unsigned long long tp = l1 & p1, fn = l1 & ~p1, fp = ~l1 & p1 & all, tn = all & ~l1 & ~p1;
  c[0] += (unsigned int)__popcll(tn);
  c[1] += (unsigned int)__popcll(fp);
  c[2] += (unsigned int)__popcll(fn);
  c[3] += (unsigned int)__popcll(tp);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void best_candidate_kernel(const int64_t* __restrict__ rowptr,
                                                                const int32_t* __restrict__ seg_edge, int64_t nseg,
                                                                const T* __restrict__ value, const float* __restrict__ y,
                                                                unsigned long long* __restrict__ counts,
                                                                uint8_t* __restrict__ label) {
  __shared__ unsigned int red[kWavesPerBlock][4];
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  unsigned int c[4] = {0u, 0u, 0u, 0u};        // wave-uniform counts of this wave's segments
  for (int64_t seg = (int64_t)blockIdx.x * kWavesPerBlock + w; seg < nseg; seg += nwaves) {
    const int64_t beg = rowptr[seg], end = rowptr[seg + 1];
    // first (usually only) chunk stays in registers for the labelling pass
    const int64_t i0 = beg + lane;
    const bool in0 = i0 < end;
    const int64_t e0 = in0 ? (seg_edge ? (int64_t)seg_edge[i0] : i0) : 0;
    const T v0 = in0 ? value[e0] : neg_inf<T>();
    T mx = v0 == v0 ? v0 : neg_inf<T>();       // NaN beats nobody
    for (int64_t i = i0 + kWave; i < end; i += kWave) {
      const T v = value[seg_edge ? (int64_t)seg_edge[i] : i];
      mx = fmax(mx, v);                        // fmax ignores a NaN operand
    }
    mx = wave_max(mx);
    {
      const bool lab = in0 && (v0 != v0 || v0 >= mx);
      if (in0) label[e0] = (uint8_t)lab;
      if (y) count_lanes(in0, in0 && y[e0] > 0.5f, lab, c);
    }
    for (int64_t i = i0 + kWave; i < end; i += kWave) {      // segments longer than a wave
      const int64_t e = seg_edge ? (int64_t)seg_edge[i] : i;
      const T v = value[e];
      const bool lab = v != v || v >= mx;
      label[e] = (uint8_t)lab;
      if (y) count_lanes(true, y[e] > 0.5f, lab, c);
    }
  }
  if (!y) return;                              // block-uniform
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) red[w][k] = c[k];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    unsigned long long t = 0;
    for (int k = 0; k < kWavesPerBlock; ++k) t += red[k][threadIdx.x];
    if (t) atomicAdd(&counts[threadIdx.x], t);
  }
}

template <typename T>
int best_candidate(const char* name, const int64_t* seg_rowptr, const int32_t* seg_edge, int64_t num_segments,
                   int64_t num_edges, const T* value, const float* y, int64_t* counts, uint8_t* label,
                   pangnn_stream_t stream) {
  PG_CHECK_ARG(num_segments >= 0 && num_edges >= 0, PANGNN_E_BADARG, "%s: negative size", name);
  PG_CHECK_ARG((y == nullptr) == (counts == nullptr), PANGNN_E_BADARG, "%s: y and counts go together", name);
  PG_CHECK_ARG(num_segments > 0 || num_edges == 0, PANGNN_E_BADARG, "%s: %lld edges in no segment", name,
               (long long)num_edges);
  if (num_edges == 0) return 0;
  PG_CHECK_ARG(seg_rowptr && value && label, PANGNN_E_BADARG, "%s: null pointer", name);
  PG_CHECK_ARG(num_segments <= num_edges, PANGNN_E_BADARG, "%s: %lld segments for %lld edges (no empty segments)", name,
               (long long)num_segments, (long long)num_edges);
  PG_CHECK_ARG(!seg_edge || num_edges <= (int64_t)INT32_MAX, PANGNN_E_TOOLARGE, "%s: int32 seg_edge cannot address %lld edges",
               name, (long long)num_edges);
  // one wave counts at most 2^32 - 1 edges of its grid-stride share (32 k waves)
  PG_CHECK_ARG(num_edges < ((int64_t)1 << 44), PANGNN_E_TOOLARGE, "%s: too many edges", name);
  int64_t blocks = (num_segments + kWavesPerBlock - 1) / kWavesPerBlock;
  if (blocks > kCandMaxBlocks) blocks = kCandMaxBlocks;
  hipLaunchKernelGGL(best_candidate_kernel<T>, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, seg_rowptr,
                     seg_edge, num_segments, value, y, reinterpret_cast<unsigned long long*>(counts), label);
  PG_CHECK_LAUNCH(name);
  return 0;
}

}  // namespace
}  // namespace pangnn

extern "C" int pangnn_best_candidate_f32(const int64_t* seg_rowptr, const int32_t* seg_edge, int64_t num_segments,
                                         int64_t num_edges, const float* value, const float* y, int64_t* counts,
                                         uint8_t* label, pangnn_stream_t stream) {
  return pangnn::best_candidate<float>("pangnn_best_candidate_f32", seg_rowptr, seg_edge, num_segments, num_edges, value, y,
                                       counts, label, stream);
}

extern "C" int pangnn_best_candidate_f64(const int64_t* seg_rowptr, const int32_t* seg_edge, int64_t num_segments,
                                         int64_t num_edges, const double* value, const float* y, int64_t* counts,
                                         uint8_t* label, pangnn_stream_t stream) {
  return pangnn::best_candidate<double>("pangnn_best_candidate_f64", seg_rowptr, seg_edge, num_segments, num_edges, value, y,
                                        counts, label, stream);
}
