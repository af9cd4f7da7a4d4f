// The Q-score edge weights as a differentiable function of the bit scores and of the softmax temperature
// (construct.normalize_sim_scores, src/preprocessing.py:454-548), over a segment plan of the graph's OWN edge list:
//   segment k = positions [rowptr[k], rowptr[k + 1]) of the (source gene, candidate genome) order, edge id item[pos];
//   x_i = score_i / t,  lse = log sum_j exp(x_j - max) + max,  p_i = exp(x_i - lse)   (one candidate: p = 1)
//   w_i = -10 log10(clip(1 - p_i, eps, 1 - eps)) + pseudo                              (NaN p: the nan_to_num branch)
// Scores are read and weights / gradients written at item[pos], so everything outside these kernels stays in the caller's
// edge order.  The forward is softmax_qscore_kernel (edge_ops.hip) statement for statement — the same float64 operations in
// the same lane-stride + xor-shuffle order, hence the same bits — with the temperature read from DEVICE memory (it is a
// parameter's value) and the per-segment lse kept for the backward, together with r, what its last addition rounded away
// (log(sum) + max = lse + r exactly, by TwoSum):
//   c_i = 1 - p_i,  a_i = g_i (10 / ln 10) / c_i where eps <= c_i <= 1 - eps, else 0   (torch.clamp's inclusive mask)
//   S = sum_j p_j a_j,  gx_i = p_i ((a_i - S) + S r),  dL/dscore_i = gx_i / t,  dL/dt += -(sum_i gx_i score_i) / t^2
// S (1 - r) is S with the softmax probability taken from the unrounded lse, exp(x_i - max) / sum — what autograd's walk through
// lse = log(sum) + max multiplies S by.  Mathematically r = 0; numerically a_i p_i and S p_i cancel down to c_i of their size,
// so at lse = 700 and c_i = 2.5e-8 leaving r out moves the result by 8e-7 of itself (DESIGN.md 4b'').
// One wave per segment, lanes stride the segment; the first 64 items of a segment (usually all of it) stay in registers
// between the passes.  The per-segment shares of dL/dt go to a buffer and are added in a fixed order by two further launches:
// no float atomics, every output is a function of the inputs alone.  Non-finite scores are not special-cased.
#include "common.h"

namespace pangnn {
namespace {

// the edge at position k of the segment order; an id outside [0, E) (a broken plan) is reported as -1 and touches nothing
__device__ __forceinline__ int64_t edge_at(const int32_t* __restrict__ item, int64_t k, int64_t E) {
  const int64_t e = item[k];
  return (uint64_t)e < (uint64_t)E ? e : -1;
}

struct Segment { int64_t beg, end; };
__device__ __forceinline__ Segment segment_of(const int64_t* __restrict__ rowptr, int64_t seg, int64_t E) {
  int64_t b = rowptr[seg], e = rowptr[seg + 1];
  b = b < 0 ? 0 : b;
  e = e > E ? E : e;                             // (a consistent plan is left as it is)
  return {b, e};
}

template <typename S, typename W>
__global__ __launch_bounds__(kBlock) void qscore_fwd_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ item,
                                                            const S* __restrict__ score, int64_t nseg, int64_t E,
                                                            const double* __restrict__ t_ptr, double eps, double pseudo,
                                                            W* __restrict__ w, double* __restrict__ lse_out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t seg = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (seg >= nseg) return;                       // wave-uniform: whole waves leave
  const double t = t_ptr[0];
  const Segment s = segment_of(rowptr, seg, E);
  const int64_t i0 = s.beg + lane;
  const bool in0 = i0 < s.end;
  const int64_t e0 = in0 ? edge_at(item, i0, E) : -1;
  const double x0 = e0 >= 0 ? (double)score[e0] / t : 0.0;   // divide like the reference (t = 0.8 is not a binary fraction)
  const double q_one = -10.0 * log10(eps) + pseudo;          // p = 1: clip(0, eps, 1 - eps) = eps
  if (s.end - s.beg == 1) {
    if (lane == 0) {
      if (e0 >= 0) w[e0] = (W)q_one;
      lse_out[seg] = x0;
      lse_out[nseg + seg] = 0.0;
    }
    return;
  }
  // (fmax drops a NaN score, the sum below does not: one NaN sends its whole segment through the nan_to_num branch)
  double mx = -INFINITY;
  if (e0 >= 0) mx = fmax(mx, x0);
  for (int64_t i = i0 + kWave; i < s.end; i += kWave) {
    const int64_t e = edge_at(item, i, E);
    if (e >= 0) mx = fmax(mx, (double)score[e] / t);
  }
  mx = wave_max(mx);
  double sm = 0.0;
  if (e0 >= 0) sm += exp(x0 - mx);
  for (int64_t i = i0 + kWave; i < s.end; i += kWave) {
    const int64_t e = edge_at(item, i, E);
    if (e >= 0) sm += exp((double)score[e] / t - mx);
  }
  sm = wave_sum(sm);
  const double ls = log(sm);
  const double lse = ls + mx;                                // scipy.special.logsumexp
  if (lane == 0) {
    const double bb = lse - ls;                              // TwoSum: ls + mx = lse + r exactly
    lse_out[seg] = lse;
    lse_out[nseg + seg] = (ls - (lse - bb)) + (mx - bb);
  }
  // (the clip stays in front of the log10, as in softmax_qscore_kernel: selecting the two clipped values instead — nearly every
  // item clips at t = 0.8 — measured no faster, 2.06 against 2.00 ms at E = 7.5e7, and did not keep that kernel's bits)
  for (int64_t i = i0; i < s.end; i += kWave) {
    const int64_t e = i == i0 ? e0 : edge_at(item, i, E);
    if (e < 0) continue;
    const double p = exp((i == i0 ? x0 : (double)score[e] / t) - lse);
    double c = 1.0 - p;
    c = c < eps ? eps : (c > 1.0 - eps ? 1.0 - eps : c);
    const double v = -10.0 * log10(c);
    w[e] = (W)((p != p ? -10.0 * log10(1.0 - eps) : v) + pseudo);       // NaN p: the reference's nan_to_num branch
  }
}

// p_i and a_i of one item from the saved lse
__device__ __forceinline__ void item_terms(double x, double g, double lse, double eps, double& p, double& a) {
  p = exp(x - lse);
  const double c = 1.0 - p;
  const double k = 10.0 / log(10.0);
  a = (c >= eps && c <= 1.0 - eps) ? g * k / c : 0.0;        // a NaN c fails both comparisons, as torch.clamp's mask does
}

template <typename S, typename G>
__global__ __launch_bounds__(kBlock) void qscore_bwd_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ item,
                                                            const S* __restrict__ score, const G* __restrict__ g,
                                                            const double* __restrict__ lse_in, int64_t nseg, int64_t E,
                                                            const double* __restrict__ t_ptr, double eps,
                                                            S* __restrict__ gscore, double* __restrict__ t_parts) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t seg = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (seg >= nseg) return;
  const double t = t_ptr[0];
  const Segment s = segment_of(rowptr, seg, E);
  const int64_t i0 = s.beg + lane;
  const bool in0 = i0 < s.end;
  const int64_t e0 = in0 ? edge_at(item, i0, E) : -1;
  if (s.end - s.beg <= 1) {                      // p = 1 whatever the score: no gradient
    if (lane == 0) {
      if (gscore && e0 >= 0) gscore[e0] = (S)0.0;
      if (t_parts) t_parts[seg] = 0.0;
    }
    return;
  }
  const double lse = lse_in[seg], r = lse_in[nseg + seg];
  const double sc0 = e0 >= 0 ? (double)score[e0] : 0.0;
  double p0 = 0.0, a0 = 0.0;
  if (e0 >= 0) item_terms(sc0 / t, (double)g[e0], lse, eps, p0, a0);
  double sum = p0 * a0;                          // (a lane without an item adds 0 * 0)
  for (int64_t i = i0 + kWave; i < s.end; i += kWave) {
    const int64_t e = edge_at(item, i, E);
    if (e < 0) continue;
    double p, a;
    item_terms((double)score[e] / t, (double)g[e], lse, eps, p, a);
    sum += p * a;
  }
  sum = wave_sum(sum);
  const double sum_r = sum * r;                  // a_i - S (1 - r) = (a_i - S) + S r: r is not rounded against 1
  double acc = 0.0;
  if (e0 >= 0) {
    const double gx = p0 * ((a0 - sum) + sum_r);
    if (gscore) gscore[e0] = (S)(gx / t);
    acc = gx * sc0;
  }
  for (int64_t i = i0 + kWave; i < s.end; i += kWave) {      // segments longer than a wave: recomputed, not kept
    const int64_t e = edge_at(item, i, E);
    if (e < 0) continue;
    const double sc = (double)score[e];
    double p, a;
    item_terms(sc / t, (double)g[e], lse, eps, p, a);
    const double gx = p * ((a - sum) + sum_r);
    if (gscore) gscore[e] = (S)(gx / t);
    acc += gx * sc;
  }
  if (t_parts) {                                 // wave-uniform
    acc = wave_sum(acc);
    if (lane == 0) t_parts[seg] = -acc / (t * t);
  }
}

// out[b] = in[b * chunk .. min((b + 1) * chunk, n)) added in a fixed order: thread i adds the entries i, i + 256, ... of the
// range in ascending position, the 64 lane sums of a wave meet in a butterfly, the 4 wave sums are added in wave order
__global__ __launch_bounds__(kBlock) void sum_f64_kernel(const double* __restrict__ in, int64_t n, int64_t chunk,
                                                         double* __restrict__ out) {
  __shared__ double red[kWavesPerBlock];
  const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
  double v = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kBlock) v += in[i];
  v = wave_sum(v);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = 0.0;
    for (int k = 0; k < kWavesPerBlock; ++k) r += red[k];
    out[blockIdx.x] = r;
  }
}

bool score_dtype(int32_t d) { return d == PANGNN_DTYPE_F32 || d == PANGNN_DTYPE_F64; }

int check_plan(const char* fn, int64_t nseg, int64_t E, int32_t s_dtype, int32_t o_dtype, const char* o_name, double eps) {
  PG_CHECK_ARG(nseg >= 0 && E >= 0, PANGNN_E_BADARG, "%s: negative size (num_segments=%lld num_edges=%lld)", fn,
               (long long)nseg, (long long)E);
  PG_CHECK_ARG(score_dtype(s_dtype) && score_dtype(o_dtype), PANGNN_E_BADARG,
               "%s: score_dtype and %s must be PANGNN_DTYPE_F32 or PANGNN_DTYPE_F64 (got %d, %d)", fn, o_name, (int)s_dtype,
               (int)o_dtype);
  PG_CHECK_ARG(eps > 0.0 && eps < 0.5, PANGNN_E_BADARG, "%s: epsilon must lie in (0, 0.5), got %g", fn, eps);
  PG_CHECK_ARG(E < ((int64_t)1 << 31) && nseg < ((int64_t)1 << 31), PANGNN_E_TOOLARGE,
               "%s: sizes exceed the int32 index range", fn);
  PG_CHECK_ARG(nseg > 0 || E == 0, PANGNN_E_BADARG, "%s: %lld edges in no segment", fn, (long long)E);
  PG_CHECK_ARG(nseg <= E, PANGNN_E_BADARG, "%s: %lld segments for %lld edges (no empty segments)", fn, (long long)nseg,
               (long long)E);
  return 0;
}

inline unsigned seg_blocks(int64_t nseg) { return (unsigned)((nseg + kWavesPerBlock - 1) / kWavesPerBlock); }

}  // namespace
}  // namespace pangnn

using namespace pangnn;

extern "C" int pangnn_qscore_fwd(const int64_t* rowptr, const int32_t* item, const void* score, int32_t score_dtype,
                                 int64_t num_segments, int64_t num_edges, const double* t, double epsilon,
                                 double pseudo_count, void* weight, int32_t weight_dtype, double* lse,
                                 pangnn_stream_t stream) {
  const char* fn = "pangnn_qscore_fwd";
  if (int rc = check_plan(fn, num_segments, num_edges, score_dtype, weight_dtype, "weight_dtype", epsilon)) return rc;
  if (num_edges == 0) return 0;
  PG_CHECK_ARG(rowptr && item && score && t && weight && lse, PANGNN_E_BADARG, "%s: null pointer", fn);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(seg_blocks(num_segments)), block(kBlock);
#define PG_QS_FWD(S, W)                                                                                                   \
  hipLaunchKernelGGL((qscore_fwd_kernel<S, W>), grid, block, 0, s, rowptr, item, static_cast<const S*>(score), num_segments, \
                     num_edges, t, epsilon, pseudo_count, static_cast<W*>(weight), lse)
  if (score_dtype == PANGNN_DTYPE_F64) {
    if (weight_dtype == PANGNN_DTYPE_F64) PG_QS_FWD(double, double); else PG_QS_FWD(double, float);
  } else {
    if (weight_dtype == PANGNN_DTYPE_F64) PG_QS_FWD(float, double); else PG_QS_FWD(float, float);
  }
#undef PG_QS_FWD
  PG_CHECK_LAUNCH(fn);
  return 0;
}

extern "C" int pangnn_qscore_bwd(const int64_t* rowptr, const int32_t* item, const void* score, int32_t score_dtype,
                                 const void* g, int32_t g_dtype, const double* lse, int64_t num_segments, int64_t num_edges,
                                 const double* t, double epsilon, void* gscore, double* gt, double* t_parts,
                                 pangnn_stream_t stream) {
  const char* fn = "pangnn_qscore_bwd";
  if (int rc = check_plan(fn, num_segments, num_edges, score_dtype, g_dtype, "g_dtype", epsilon)) return rc;
  if (num_edges == 0 || (!gscore && !gt)) return 0;          // (dL/dt of an empty relation is the caller's zero)
  PG_CHECK_ARG(rowptr && item && score && g && lse && t, PANGNN_E_BADARG, "%s: null pointer", fn);
  PG_CHECK_ARG(!gt || t_parts, PANGNN_E_BADARG, "%s: gt needs the t_parts buffer (null pointer)", fn);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(seg_blocks(num_segments)), block(kBlock);
  double* parts = gt ? t_parts : nullptr;
#define PG_QS_BWD(S, G)                                                                                                    \
  hipLaunchKernelGGL((qscore_bwd_kernel<S, G>), grid, block, 0, s, rowptr, item, static_cast<const S*>(score),            \
                     static_cast<const G*>(g), lse, num_segments, num_edges, t, epsilon, static_cast<S*>(gscore), parts)
  if (score_dtype == PANGNN_DTYPE_F64) {
    if (g_dtype == PANGNN_DTYPE_F64) PG_QS_BWD(double, double); else PG_QS_BWD(double, float);
  } else {
    if (g_dtype == PANGNN_DTYPE_F64) PG_QS_BWD(float, double); else PG_QS_BWD(float, float);
  }
#undef PG_QS_BWD
  PG_CHECK_LAUNCH(fn);
  if (!gt) return 0;
  // the shares of dL/dt, added in an order that num_segments alone fixes: up to PANGNN_QSCORE_SUM_PARTS block sums behind the
  // shares, then one block over those
  int64_t nb = (num_segments + kBlock - 1) / kBlock;
  nb = nb > PANGNN_QSCORE_SUM_PARTS ? PANGNN_QSCORE_SUM_PARTS : nb;
  const int64_t chunk = (num_segments + nb - 1) / nb;
  hipLaunchKernelGGL(sum_f64_kernel, dim3((unsigned)nb), block, 0, s, t_parts, num_segments, chunk, t_parts + num_segments);
  PG_CHECK_LAUNCH("pangnn_qscore_bwd(part sums)");
  hipLaunchKernelGGL(sum_f64_kernel, dim3(1), block, 0, s, t_parts + num_segments, nb, nb, gt);
  PG_CHECK_LAUNCH("pangnn_qscore_bwd(total)");
  return 0;
}
