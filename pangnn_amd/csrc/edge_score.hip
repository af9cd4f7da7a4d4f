// The weightless link decoders (src/gnn.py:171-180,202-207: --decoder cosine / dotproduct) as per-edge reductions over two
// gathered rows (an SDDMM), with no [E, 2D] edge tensor in either direction:
//   node pass   (cosine) norms[n] = (1 / max(|z_n|, eps), 1 / (max(|z_n|, eps) |z_n|))   (second entry 0 when |z_n| = 0)
//   edge pass   logit_e = z_s . z_d  (dot)   or   (z_s . z_d) inv_s inv_d  (cosine: torch's F.cosine_similarity, eps 1e-8)
//               + optionally BCEWithLogits(pos_weight): loss and dL/dlogit in the same pass (bce_kernel's parameterisation)
//   backward    dL/dz[n] = sum_{out-edges e=(n,m)} c_e z_m + sum_{in-edges e=(m,n)} c_e z_m  - z_n k_n sum_{e at n} g_e cos_e
//               c_e = g_e (dot) or g_e inv_n inv_m (cosine), k_n = the node's second norm entry (cosine only)
//               one wave walks both CSR rows of a node and writes its gradient row once; hub rows (graph.CSR.long_rows) are
//               walked as segments whose partial rows the node's wave then adds in a fixed order.  No atomics anywhere.
// Rows are gathered as stored (f32 / bf16 / f16, 16- or 8-byte pieces per lane) and every product and sum is fp32.
#include "common.h"

namespace pangnn {
namespace {

constexpr float kScoreEps = 1e-8f;   // F.cosine_similarity's default

// one group of G = D / 4 lanes per node
template <int D, int XF>
__global__ __launch_bounds__(kBlock) void score_norm_kernel(const char* __restrict__ z, int64_t ldz, int64_t n,
                                                            float* __restrict__ norms) {
  constexpr int G = D / 4, ES = XF ? 2 : 4;
  const int lane = threadIdx.x & (kWave - 1), fl = lane % G;
  const int64_t node = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
  if (node >= n) return;                                   // a whole group leaves together
  const float4 v = row_piece<true>(z + ((uint64_t)node * ldz + fl * 4) * ES, XF);
  const float s = group_sum<G>(dot4(v, v));
  if (fl == 0) {
    const float nrm = sqrtf(s);
    const float inv = 1.f / fmaxf(nrm, kScoreEps);
    norms[2 * node] = inv;
    norms[2 * node + 1] = nrm > 0.f ? inv / nrm : 0.f;       // (a NaN norm: the row's dot products and z_n itself carry the NaN on)
  }
}

// one group of G lanes per edge, U edges per group in flight; LOSS: BCEWithLogits(pos_weight) as bce_kernel computes it, one
// partial per block (fixed slice of edges, fixed order), finished by score_loss_finish_kernel.
// LIVE (with LOSS): the list is a fixed-shape padded batch whose first m = min(max(live[0], 0), e) edges are real
// (include/pangnn_hip.h, live_edges): every edge keeps its logit, an edge k >= m gets dL/dlogit = +0 and adds nothing to the
// loss, and the mean is over max(m, 1) edges (inv_denom is not read).  live[0] is one uniform load per block, outside the edge
// loop; the instances without LIVE never look at `live` and are the code they were before it existed.
template <int D, int XF, int MODE, bool LOSS, bool LIVE = false>
__global__ __launch_bounds__(kBlock) void edge_score_kernel(const char* __restrict__ z, int64_t ldz,
                                                            const int64_t* __restrict__ ei, int64_t ld, int64_t e,
                                                            const float* __restrict__ norms, float* __restrict__ logits,
                                                            const float* __restrict__ y, const float* __restrict__ pos_weight,
                                                            float inv_denom, float* __restrict__ g_logits,
                                                            float* __restrict__ partial, const int64_t* __restrict__ live) {
  static_assert(LOSS || !LIVE, "live_edges belongs to the fused loss");
  constexpr int G = D / 4, ES = XF ? 2 : 4, U = 2;
  const int lane = threadIdx.x & (kWave - 1), fl = lane % G;
  const int64_t groups = (int64_t)gridDim.x * (kBlock / G);
  const int64_t gid = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
  const char* zb = z + fl * 4 * ES;
  const uint64_t ldb = (uint64_t)ldz * ES;
  const float pw = (LOSS && pos_weight) ? pos_weight[0] : 1.f;
  int64_t m = e;                                             // LIVE: the number of real edges
  if (LIVE) {
    const int64_t lv = live[0];
    m = lv < 0 ? 0 : lv > e ? e : lv;
    inv_denom = 1.0f / (float)(m > 1 ? m : 1);               // the host's 1.0f / (float)denom of the list cut to m edges
  }
  float acc = 0.f;
  for (int64_t k = gid; k < e; k += U * groups) {
    int64_t s[U], d[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t kk = k + u * groups;
      s[u] = kk < e ? ei[kk] : 0;                            // node 0 exists whenever there is an edge
      d[u] = kk < e ? ei[ld + kk] : 0;
    }
    float4 a[U], b[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      a[u] = row_piece<true>(zb + (uint64_t)s[u] * ldb, XF);
      b[u] = row_piece<true>(zb + (uint64_t)d[u] * ldb, XF);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t kk = k + u * groups;
      float x = group_sum<G>(dot4(a[u], b[u]));
      if (kk < e && fl == 0) {
        if (MODE == PANGNN_SCORE_COSINE) x = x * norms[2 * s[u]] * norms[2 * d[u]];
        logits[kk] = x;
        if (LOSS) {
          const float yv = y[kk];
          const float lw = 1.f + (pw - 1.f) * yv;
          const float ax = fabsf(x);
          const float t = expf(-ax);
          const float sp = log1pf(t) + fmaxf(-x, 0.f);                      // softplus(-x)
          const bool real = !LIVE || kk < m;                                // padding: no term, dL/dlogit = 0 whatever x is
          if (real) acc += (1.f - yv) * x + lw * sp;
          const float sm = t / (1.f + t);                                   // sigmoid(-|x|): bce_kernel's form of dl/dx
          g_logits[kk] = real ? (x >= 0.f ? (1.f - yv) - lw * sm : lw * sm - pw * yv) * inv_denom : 0.f;
        }
      }
    }
  }
  if (LOSS) {
    __shared__ float red[kWavesPerBlock];
    // wave_sum written out: through the shared helper the compiler schedules this tail differently (same sums, other bytes)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      float t = 0.f;
      for (int w = 0; w < kWavesPerBlock; ++w) t += red[w];
      partial[blockIdx.x] = t * inv_denom;
    }
  }
}

// loss[0] = sum of the block partials: lane l adds partials l, l + 64, ... in order, then a fixed butterfly
__global__ void score_loss_finish_kernel(const float* __restrict__ partial, int n, float* __restrict__ loss) {
  const int lane = threadIdx.x;
  float s = 0.f;
  for (int i = lane; i < n; i += kWave) s += partial[i];
  s = wave_sum(s);
  if (lane == 0) loss[0] = s;
}

// entries [lo, hi) of one CSR row: sub-group `sub` of the wave takes entries lo + sub, lo + sub + EPS, ...; acc += c_e z_m,
// ds += g_e cos_e (cosine)
template <int D, int XF, int MODE>
__device__ __forceinline__ void score_walk(const char* zb, uint64_t ldb, const int32_t* __restrict__ other,
                                           const int32_t* __restrict__ perm, int64_t lo, int64_t hi, int sub,
                                           const float* __restrict__ g, const float* __restrict__ logits,
                                           const float* __restrict__ norms, float4& acc, float& ds) {
  constexpr int G = D / 4, EPS = kWave / G;
  for (int64_t k = lo + sub; k < hi; k += 2 * EPS) {
    const int64_t k1 = k + EPS;
    const bool ok1 = k1 < hi;
    const int32_t e0 = perm[k], m0 = other[k];
    const int32_t e1 = ok1 ? perm[k1] : e0, m1 = ok1 ? other[k1] : m0;
    const float4 r0 = row_piece<true>(zb + (uint64_t)m0 * ldb, XF);
    const float4 r1 = row_piece<true>(zb + (uint64_t)m1 * ldb, XF);
    float c0 = g[e0], c1 = ok1 ? g[e1] : 0.f;
    if (MODE == PANGNN_SCORE_COSINE) {
      ds = fmaf(c0, logits[e0], ds);
      if (ok1) ds = fmaf(c1, logits[e1], ds);
      c0 *= norms[2 * m0];
      c1 *= norms[2 * m1];
    }
    acc.x = fmaf(c0, r0.x, acc.x); acc.y = fmaf(c0, r0.y, acc.y); acc.z = fmaf(c0, r0.z, acc.z); acc.w = fmaf(c0, r0.w, acc.w);
    if (ok1) {
      acc.x = fmaf(c1, r1.x, acc.x); acc.y = fmaf(c1, r1.y, acc.y); acc.z = fmaf(c1, r1.z, acc.z); acc.w = fmaf(c1, r1.w, acc.w);
    }
  }
}

// the EPS sub-group partials of a wave, combined by a fixed butterfly (every lane ends with the same bits)
template <int G>
__device__ __forceinline__ void score_combine(float4& acc, float& ds) {
#pragma unroll
  for (int off = G; off < kWave; off <<= 1) {
    acc.x += __shfl_xor(acc.x, off);
    acc.y += __shfl_xor(acc.y, off);
    acc.z += __shfl_xor(acc.z, off);
    acc.w += __shfl_xor(acc.w, off);
    ds += __shfl_xor(ds, off);
  }
}

// one wave per segment of a hub-carrying CSR order: parts[v][0:D] = partial acc, parts[nseg * D + v] = partial ds
template <int D, int XF, int MODE>
__global__ __launch_bounds__(kBlock) void score_seg_kernel(const char* __restrict__ z, int64_t ldz,
                                                           const int64_t* __restrict__ seg_ptr, const int32_t* __restrict__ other,
                                                           const int32_t* __restrict__ perm, int64_t nseg,
                                                           const float* __restrict__ g, const float* __restrict__ logits,
                                                           const float* __restrict__ norms, float* __restrict__ parts) {
  constexpr int G = D / 4, ES = XF ? 2 : 4;
  const int lane = threadIdx.x & (kWave - 1), fl = lane % G, sub = lane / G;
  const int64_t v = (int64_t)blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (v >= nseg) return;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float ds = 0.f;
  score_walk<D, XF, MODE>(z + fl * 4 * ES, (uint64_t)ldz * ES, other, perm, seg_ptr[v], seg_ptr[v + 1], sub, g, logits, norms,
                          acc, ds);
  score_combine<G>(acc, ds);
  if (sub == 0) {
    *reinterpret_cast<float4*>(parts + v * D + fl * 4) = acc;
    if (fl == 0) parts[nseg * D + v] = ds;
  }
}

struct ScoreOrder {
  const int64_t* rowptr; const int32_t* other; const int32_t* perm;
  const int64_t* parts_rowptr; const float* parts; int64_t nseg;     // parts_rowptr == NULL: walk the row itself
};

template <int D, int XF, int MODE>
__device__ __forceinline__ void score_order(const ScoreOrder& o, int64_t node, const char* zb, uint64_t ldb, int sub, int fl,
                                            const float* g, const float* logits, const float* norms, float4& acc, float& ds) {
  constexpr int G = D / 4, EPS = kWave / G;
  if (o.parts_rowptr) {
    for (int64_t p = o.parts_rowptr[node] + sub; p < o.parts_rowptr[node + 1]; p += EPS) {
      const float4 t = *reinterpret_cast<const float4*>(o.parts + p * D + fl * 4);
      acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
      if (MODE == PANGNN_SCORE_COSINE) ds += o.parts[o.nseg * D + p];
    }
  } else {
    score_walk<D, XF, MODE>(zb, ldb, o.other, o.perm, o.rowptr[node], o.rowptr[node + 1], sub, g, logits, norms, acc, ds);
  }
}

// one wave per node: out-edges (by source), then in-edges (by target), the diagonal term, the upstream scale; one store.
// A padded batch (pangnn_edge_score_loss_live_mixed) needs nothing here: a padded edge arrives with g_e = +0, so its c_e z_m
// term adds an exact zero to the row of either endpoint (z finite) and, being later in list order than every real edge, it sits
// behind them in the stable CSR rows: the real entries keep their sub-group and their order, the row sum its bits.  A padded node
// has only such edges: acc = 0 and, for cosine, ds = sum g_e cos_e = 0, so the diagonal term k_n ds z_n is 0 too — a zero row.
template <int D, int XF, int MODE>
__global__ __launch_bounds__(kBlock) void score_grad_kernel(const char* __restrict__ z, int64_t ldz, int64_t n,
                                                            ScoreOrder src, ScoreOrder dst, const float* __restrict__ g,
                                                            const float* __restrict__ logits, const float* __restrict__ norms,
                                                            const float* __restrict__ g_scale, float* __restrict__ gz,
                                                            int64_t ldg) {
  constexpr int G = D / 4, ES = XF ? 2 : 4;
  const int lane = threadIdx.x & (kWave - 1), fl = lane % G, sub = lane / G;
  const int64_t node = (int64_t)blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (node >= n) return;
  const char* zb = z + fl * 4 * ES;
  const uint64_t ldb = (uint64_t)ldz * ES;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float ds = 0.f;
  score_order<D, XF, MODE>(src, node, zb, ldb, sub, fl, g, logits, norms, acc, ds);
  score_order<D, XF, MODE>(dst, node, zb, ldb, sub, fl, g, logits, norms, acc, ds);
  score_combine<G>(acc, ds);
  if (sub != 0) return;
  float4 out = acc;
  // a node without edges gets a zero row whatever its own row holds (0 * NaN would raise a false alarm in a GradScaler)
  if (MODE == PANGNN_SCORE_COSINE &&
      (src.rowptr[node + 1] > src.rowptr[node] || dst.rowptr[node + 1] > dst.rowptr[node])) {
    const float inv = norms[2 * node], k = norms[2 * node + 1] * ds;
    const float4 zn = row_piece<true>(zb + (uint64_t)node * ldb, XF);
    out = make_float4(inv * acc.x - k * zn.x, inv * acc.y - k * zn.y, inv * acc.z - k * zn.z, inv * acc.w - k * zn.w);
  }
  if (g_scale) {
    const float s = g_scale[0];
    out = make_float4(out.x * s, out.y * s, out.z * s, out.w * s);
  }
  *reinterpret_cast<float4*>(gz + node * ldg + fl * 4) = out;
}

// ---- launchers
constexpr int kScoreMaxBlocks = 4096;

template <int D, int XF>
int launch_norms(const void* z, int64_t ldz, int64_t n, float* norms, hipStream_t s) {
  if (n == 0) return 0;
  hipLaunchKernelGGL((score_norm_kernel<D, XF>), dim3(blocks_for(n, kBlock / (D / 4))), dim3(kBlock), 0, s,
                     static_cast<const char*>(z), ldz, n, norms);
  PG_CHECK_LAUNCH("pangnn_edge_score(node norms)");
  return 0;
}

template <int D, int XF, int MODE>
int launch_edges(const void* z, int64_t ldz, const int64_t* ei, int64_t ld, int64_t e, const float* norms, float* logits,
                 const float* y, const float* pw, int64_t denom, float* loss, float* g_logits, float* parts,
                 const int64_t* live, hipStream_t s) {
  const bool fused = loss != nullptr;
  int64_t blocks = blocks_for(e, kBlock / (D / 4));
  blocks = blocks < 1 ? 1 : blocks > kScoreMaxBlocks ? kScoreMaxBlocks : blocks;
  if (!fused) {
    if (e == 0) return 0;
    hipLaunchKernelGGL((edge_score_kernel<D, XF, MODE, false>), dim3(blocks), dim3(kBlock), 0, s, static_cast<const char*>(z),
                       ldz, ei, ld, e, norms, logits, nullptr, nullptr, 0.f, nullptr, nullptr, nullptr);
    PG_CHECK_LAUNCH("pangnn_edge_score_mixed");
    return 0;
  }
  if (live)
    hipLaunchKernelGGL((edge_score_kernel<D, XF, MODE, true, true>), dim3(blocks), dim3(kBlock), 0, s,
                       static_cast<const char*>(z), ldz, ei, ld, e, norms, logits, y, pw, 0.f, g_logits, parts, live);
  else
    hipLaunchKernelGGL((edge_score_kernel<D, XF, MODE, true>), dim3(blocks), dim3(kBlock), 0, s, static_cast<const char*>(z),
                       ldz, ei, ld, e, norms, logits, y, pw, 1.0f / (float)denom, g_logits, parts, nullptr);
  PG_CHECK_LAUNCH("pangnn_edge_score_loss_mixed");
  hipLaunchKernelGGL(score_loss_finish_kernel, dim3(1), dim3(kWave), 0, s, parts, (int)blocks, loss);
  PG_CHECK_LAUNCH("pangnn_edge_score_loss_mixed(finish)");
  return 0;
}

template <int D, int XF, int MODE>
int launch_grad(const void* z, int64_t ldz, int64_t n, ScoreOrder src, const int64_t* seg_src, float* parts_src,
                ScoreOrder dst, const int64_t* seg_dst, float* parts_dst, const float* g, const float* logits,
                const float* norms, const float* g_scale, float* gz, int64_t ldg, hipStream_t s) {
  const char* zc = static_cast<const char*>(z);
  for (int i = 0; i < 2; ++i) {
    ScoreOrder& o = i ? dst : src;
    const int64_t* seg = i ? seg_dst : seg_src;
    float* parts = i ? parts_dst : parts_src;
    if (!o.parts_rowptr) continue;
    if (o.nseg == 0) { o.parts_rowptr = nullptr; continue; }
    hipLaunchKernelGGL((score_seg_kernel<D, XF, MODE>), dim3(blocks_for(o.nseg, kWavesPerBlock)), dim3(kBlock), 0, s, zc, ldz,
                       seg, o.other, o.perm, o.nseg, g, logits, norms, parts);
    PG_CHECK_LAUNCH("pangnn_edge_score_bwd_mixed(segments)");
    o.parts = parts;
  }
  if (n == 0) return 0;
  hipLaunchKernelGGL((score_grad_kernel<D, XF, MODE>), dim3(blocks_for(n, kWavesPerBlock)), dim3(kBlock), 0, s, zc, ldz, n, src,
                     dst, g, logits, norms, g_scale, gz, ldg);
  PG_CHECK_LAUNCH("pangnn_edge_score_bwd_mixed");
  return 0;
}

// D x storage format x mode -> one instantiation
template <template <int, int, int> class Fn, typename... A>
int dispatch3(int d, int xf, int mode, A... a) {
#define PG_SCORE_CASE(DD)                                                                              \
  case DD:                                                                                             \
    if (xf == 0) return mode ? Fn<DD, 0, 1>::run(a...) : Fn<DD, 0, 0>::run(a...);                      \
    if (xf == 1) return mode ? Fn<DD, 1, 1>::run(a...) : Fn<DD, 1, 0>::run(a...);                      \
    return mode ? Fn<DD, 2, 1>::run(a...) : Fn<DD, 2, 0>::run(a...);
  switch (d) {
    PG_SCORE_CASE(16)
    PG_SCORE_CASE(32)
    PG_SCORE_CASE(64)
    PG_SCORE_CASE(128)
    PG_SCORE_CASE(256)
  }
#undef PG_SCORE_CASE
  return PANGNN_E_BADARG;
}

template <int D, int XF, int MODE>
struct FwdFn {
  static int run(const void* z, int64_t ldz, int64_t n, const int64_t* ei, int64_t ld, int64_t e, float* norms, float* logits,
                 const float* y, const float* pw, int64_t denom, float* loss, float* g_logits, float* parts, const int64_t* live,
                 hipStream_t s) {
    if (MODE == PANGNN_SCORE_COSINE) {
      const int rc = launch_norms<D, XF>(z, ldz, n, norms, s);
      if (rc) return rc;
    }
    return launch_edges<D, XF, MODE>(z, ldz, ei, ld, e, norms, logits, y, pw, denom, loss, g_logits, parts, live, s);
  }
};

template <int D, int XF, int MODE>
struct BwdFn {
  static int run(const void* z, int64_t ldz, int64_t n, ScoreOrder src, const int64_t* seg_src, float* parts_src,
                 ScoreOrder dst, const int64_t* seg_dst, float* parts_dst, const float* g, const float* logits,
                 const float* norms, const float* g_scale, float* gz, int64_t ldg, hipStream_t s) {
    return launch_grad<D, XF, MODE>(z, ldz, n, src, seg_src, parts_src, dst, seg_dst, parts_dst, g, logits, norms, g_scale, gz,
                                    ldg, s);
  }
};

// shared argument checks of the three entry points (z, its layout, sizes, mode)
int check_rows(const char* fn, const void* z, int32_t z_dtype, int64_t ldz, int64_t n, int64_t e, int32_t d, int32_t mode) {
  PG_CHECK_ARG(mode == PANGNN_SCORE_DOT || mode == PANGNN_SCORE_COSINE, PANGNN_E_BADARG, "%s: mode must be 0 (dot) or 1 (cosine)",
               fn);
  PG_CHECK_ARG(row_width_ok(d), PANGNN_E_BADARG, "%s: d must be 16, 32, 64, 128 or 256 (got %d)", fn, (int)d);
  PG_CHECK_ARG(row_dtype_ok(z_dtype), PANGNN_E_BADARG, "%s: z_dtype must be 0, 1 or 2", fn);
  PG_CHECK_ARG(n >= 0 && e >= 0 && ldz >= d, PANGNN_E_BADARG, "%s: bad size", fn);
  PG_CHECK_ARG(n > 0 || e == 0, PANGNN_E_BADARG, "%s: edges without nodes", fn);
  PG_CHECK_ARG(e < ((int64_t)1 << 31) && n < ((int64_t)1 << 31), PANGNN_E_TOOLARGE, "%s: sizes exceed the int32 index range", fn);
  PG_CHECK_ARG(n == 0 || z, PANGNN_E_BADARG, "%s: null pointer", fn);
  PG_CHECK_ARG(rows_aligned(z, z_dtype, ldz), PANGNN_E_ALIGN,
               "%s: z rows must start on 16 bytes (f32) / 8 bytes (2-byte rows): ldz a multiple of 4", fn);
  return 0;
}

}  // namespace
}  // namespace pangnn

using namespace pangnn;

extern "C" int pangnn_edge_score_supported(int32_t d) { return row_width_ok(d) ? 1 : 0; }

extern "C" int pangnn_edge_score_mixed(const void* z, int32_t z_dtype, int64_t ldz, int64_t num_nodes, const int64_t* edge_index,
                                       int64_t ld, int64_t num_edges, int32_t d, int32_t mode, float* norms, float* logits,
                                       pangnn_stream_t stream) {
  const char* fn = "pangnn_edge_score_mixed";
  if (int rc = check_rows(fn, z, z_dtype, ldz, num_nodes, num_edges, d, mode)) return rc;
  PG_CHECK_ARG(ld >= num_edges, PANGNN_E_BADARG, "%s: ld < num_edges", fn);
  PG_CHECK_ARG(num_edges == 0 || (edge_index && logits), PANGNN_E_BADARG, "%s: null pointer", fn);
  PG_CHECK_ARG(mode == PANGNN_SCORE_DOT || num_nodes == 0 || norms, PANGNN_E_BADARG, "%s: cosine needs norms", fn);
  return dispatch3<FwdFn>(d, z_dtype, mode, z, ldz, num_nodes, edge_index, ld, num_edges, norms, logits,
                          (const float*)nullptr, (const float*)nullptr, (int64_t)1, (float*)nullptr, (float*)nullptr,
                          (float*)nullptr, (const int64_t*)nullptr, (hipStream_t)stream);
}

extern "C" int pangnn_edge_score_loss_mixed(const void* z, int32_t z_dtype, int64_t ldz, int64_t num_nodes,
                                            const int64_t* edge_index, int64_t ld, int64_t num_edges, int32_t d, int32_t mode,
                                            const float* y, const float* pos_weight, int64_t denom, float* norms,
                                            float* logits, float* loss, float* g_logits, float* loss_parts,
                                            pangnn_stream_t stream) {
  const char* fn = "pangnn_edge_score_loss_mixed";
  if (int rc = check_rows(fn, z, z_dtype, ldz, num_nodes, num_edges, d, mode)) return rc;
  PG_CHECK_ARG(ld >= num_edges && denom > 0, PANGNN_E_BADARG, "%s: ld < num_edges or denom <= 0", fn);
  PG_CHECK_ARG(loss && loss_parts && (num_edges == 0 || (edge_index && logits && y && g_logits)), PANGNN_E_BADARG,
               "%s: null pointer", fn);
  PG_CHECK_ARG(mode == PANGNN_SCORE_DOT || num_nodes == 0 || norms, PANGNN_E_BADARG, "%s: cosine needs norms", fn);
  return dispatch3<FwdFn>(d, z_dtype, mode, z, ldz, num_nodes, edge_index, ld, num_edges, norms, logits, y, pos_weight, denom,
                          loss, g_logits, loss_parts, (const int64_t*)nullptr, (hipStream_t)stream);
}

extern "C" int pangnn_edge_score_loss_live_mixed(const void* z, int32_t z_dtype, int64_t ldz, int64_t num_nodes,
                                                 const int64_t* edge_index, int64_t ld, int64_t num_edges, int32_t d,
                                                 int32_t mode, const float* y, const float* pos_weight, int64_t denom,
                                                 float* norms, float* logits, float* loss, float* g_logits, float* loss_parts,
                                                 const int64_t* live_edges, pangnn_stream_t stream) {
  const char* fn = "pangnn_edge_score_loss_live_mixed";
  if (int rc = check_rows(fn, z, z_dtype, ldz, num_nodes, num_edges, d, mode)) return rc;
  PG_CHECK_ARG(ld >= num_edges, PANGNN_E_BADARG, "%s: ld < num_edges", fn);     // denom is ignored: the kernel divides by the live count
  PG_CHECK_ARG(live_edges && loss && loss_parts && (num_edges == 0 || (edge_index && logits && y && g_logits)), PANGNN_E_BADARG,
               "%s: null pointer", fn);
  PG_CHECK_ARG(mode == PANGNN_SCORE_DOT || num_nodes == 0 || norms, PANGNN_E_BADARG, "%s: cosine needs norms", fn);
  return dispatch3<FwdFn>(d, z_dtype, mode, z, ldz, num_nodes, edge_index, ld, num_edges, norms, logits, y, pos_weight,
                          (int64_t)1, loss, g_logits, loss_parts, live_edges, (hipStream_t)stream);
}

extern "C" int pangnn_edge_score_bwd_mixed(const void* z, int32_t z_dtype, int64_t ldz, int64_t num_nodes, int64_t num_edges,
                                           int32_t d, int32_t mode,
                                           const int64_t* rowptr_src, const int32_t* other_src, const int32_t* perm_src,
                                           const int64_t* seg_ptr_src, const int64_t* parts_rowptr_src, int64_t num_seg_src,
                                           float* parts_src,
                                           const int64_t* rowptr_dst, const int32_t* other_dst, const int32_t* perm_dst,
                                           const int64_t* seg_ptr_dst, const int64_t* parts_rowptr_dst, int64_t num_seg_dst,
                                           float* parts_dst,
                                           const float* g, const float* logits, const float* norms, const float* g_scale,
                                           float* gz, int64_t ldg, pangnn_stream_t stream) {
  const char* fn = "pangnn_edge_score_bwd_mixed";
  if (int rc = check_rows(fn, z, z_dtype, ldz, num_nodes, num_edges, d, mode)) return rc;
  PG_CHECK_ARG(ldg >= d && ldg % 4 == 0, PANGNN_E_BADARG, "%s: ldg must be >= d and a multiple of 4", fn);
  PG_CHECK_ARG(num_nodes == 0 || (gz && rowptr_src && rowptr_dst), PANGNN_E_BADARG, "%s: null pointer", fn);
  PG_CHECK_ARG(num_edges == 0 || (other_src && perm_src && other_dst && perm_dst && g), PANGNN_E_BADARG, "%s: null pointer", fn);
  PG_CHECK_ARG(mode == PANGNN_SCORE_DOT || num_nodes == 0 || (norms && (num_edges == 0 || logits)), PANGNN_E_BADARG,
               "%s: cosine needs norms and logits", fn);
  PG_CHECK_ARG((seg_ptr_src == nullptr) == (parts_rowptr_src == nullptr) && (seg_ptr_dst == nullptr) == (parts_rowptr_dst == nullptr),
               PANGNN_E_BADARG, "%s: seg_ptr and parts_rowptr go together", fn);
  PG_CHECK_ARG(num_seg_src >= 0 && num_seg_dst >= 0 && (!seg_ptr_src || num_seg_src == 0 || parts_src) &&
                   (!seg_ptr_dst || num_seg_dst == 0 || parts_dst), PANGNN_E_BADARG, "%s: segments need a parts buffer", fn);
  PG_CHECK_ARG(num_nodes == 0 || pangnn::aligned16(gz), PANGNN_E_ALIGN, "%s: gz must be 16-byte aligned", fn);
  PG_CHECK_ARG((!parts_src || pangnn::aligned16(parts_src)) && (!parts_dst || pangnn::aligned16(parts_dst)), PANGNN_E_ALIGN,
               "%s: parts buffers must be 16-byte aligned", fn);
  const ScoreOrder src{rowptr_src, other_src, perm_src, parts_rowptr_src, nullptr, seg_ptr_src ? num_seg_src : 0};
  const ScoreOrder dst{rowptr_dst, other_dst, perm_dst, parts_rowptr_dst, nullptr, seg_ptr_dst ? num_seg_dst : 0};
  return dispatch3<BwdFn>(d, z_dtype, mode, z, ldz, num_nodes, src, seg_ptr_src, parts_src, dst, seg_ptr_dst, parts_dst, g,
                          logits, norms, g_scale, gz, ldg, (hipStream_t)stream);
}
