// dL/d(edge_weight) of GCNConv (out = A_hat x + b, A_hat[d, s] = dis[s] w_e dis[d], dis = deg^-1/2, deg[v] = sum of the weights
// of v's in-edges), from the upstream gradient g = dL/dout and the rows x the propagate gathered:
//   edge dot      gw_e = <g[dst_e, :], x[src_e, :]>                                      (an SDDMM: pangnn_edge_dot_mixed)
//   norm backward t_e = gw_e w_e
//                 gdis[v] = sum_{e: dst_e = v} t_e dis[src_e] + sum_{e: src_e = v} t_e dis[dst_e]
//                 gdeg[v] = -1/2 dis[v]^3 gdis[v]          (0 where dis[v] == 0: torch's masked_fill)
//                 dL/dw_e = dis[src_e] dis[dst_e] gw_e + gdeg[dst_e]                     (pangnn_gcn_norm_bwd_f32)
// Rows are gathered as stored (f32 / bf16 / f16, 16- or 8-byte pieces per lane, the idiom of edge_score.hip); every product and
// sum is fp32 in a fixed order; no atomics anywhere, so every result is a function of its inputs alone.
#include "common.h"

namespace pangnn {
namespace {

// One wave owns `chunk` consecutive entries of the CSR (a multiple of 64), whatever rows they belong to: the work is balanced
// by entries, a hub row is shared by as many waves as it has chunks, and since every output is one entry's own dot product no
// part sums exist.  A group of G = F / 4 lanes takes one entry at a time (EPS = 64 / G entries per wave step, U steps in
// flight); sub-group `sub` sees the entries base + sub, base + sub + EPS, ... in ascending order, so it follows its row by
// stepping the row pointer and reloads its g piece only when the row changes: along a row the piece stays in registers.
// The entry lists are read 64 at a time, one coalesced non-temporal load per array (they are streamed once and must not
// displace the gathered rows), and handed to the groups by cross-lane reads, as spmm_row_kernel does.
template <int F, int XG, int XX>
__global__ __launch_bounds__(kBlock) void edge_dot_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ idx,
                                                          const int32_t* __restrict__ perm, const char* __restrict__ g,
                                                          int64_t ldg, const char* __restrict__ x, int64_t ldx, int64_t n_rows,
                                                          int64_t nnz, int64_t chunk, float* __restrict__ out_sorted,
                                                          float* __restrict__ out_orig) {
  constexpr int G = F / 4, EPS = kWave / G, U = 2;        // (4 or 8 steps in flight measured the same: profiles/edge_weight_grad.md)
  constexpr int GS = XG ? 2 : 4, XS = XX ? 2 : 4;          // bytes per stored element
  const int lane = threadIdx.x & (kWave - 1), fl = lane % G, sub = lane / G;
  const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t beg = wave * chunk;
  if (beg >= nnz) return;                                  // the whole wave leaves together
  const int64_t end = beg + chunk < nnz ? beg + chunk : nnz;
  const char* gb = g + fl * 4 * GS;
  const char* xb = x + fl * 4 * XS;
  const uint64_t ldgb = (uint64_t)ldg * GS, ldxb = (uint64_t)ldx * XS;

  // this sub-group's row: the row of its first entry
  int64_t row = 0, row_end = 0;
  float4 gv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (beg + sub < end) {
    row = row_of_entry(rowptr, n_rows, beg + sub);
    row_end = rowptr[row + 1];
    gv = row_piece<true>(gb + (uint64_t)row * ldgb, XG);
  }

  int c_nxt = 0, p_nxt = 0;
  if (beg + lane < end) {
    c_nxt = __builtin_nontemporal_load(idx + beg + lane);
    if (out_orig) p_nxt = __builtin_nontemporal_load(perm + beg + lane);
  }
  for (int64_t e0 = beg; e0 < end; e0 += kWave) {
    const int c_cur = c_nxt, p_cur = p_nxt;
    const int64_t rem = end - e0;
    const int cnt = rem < kWave ? (int)rem : kWave;
    {
      const int64_t en = e0 + kWave + lane;
      c_nxt = p_nxt = 0;
      if (en < end) {
        c_nxt = __builtin_nontemporal_load(idx + en);
        if (out_orig) p_nxt = __builtin_nontemporal_load(perm + en);
      }
    }
    for (int s = 0; s < cnt; s += EPS * U) {
      float4 xv[U], gu[U];
      int pu[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kl = s + u * EPS + sub;                    // < 64: EPS * U divides 64
        const bool ok = kl < cnt;
        const int c = __shfl(c_cur, kl);
        pu[u] = __shfl(p_cur, kl);
        if (ok) {
          const int64_t k = e0 + kl;
          if (k >= row_end) {
            while (k >= row_end && row + 1 < n_rows) {       // (a consistent CSR ends the walk by itself)
              ++row;
              row_end = rowptr[row + 1];
            }
            gv = row_piece<true>(gb + (uint64_t)row * ldgb, XG);
          }
          xv[u] = row_piece<true>(xb + (uint64_t)(uint32_t)c * ldxb, XX);
        } else {
          xv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        gu[u] = gv;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float d = group_sum<G>(dot4(gu[u], xv[u]));
        if (fl == 0 && s + u * EPS + sub < cnt) {
          out_sorted[e0 + s + u * EPS + sub] = d;
          if (out_orig) out_orig[pu[u]] = d;
        }
      }
    }
  }
}

constexpr int kDotMaxChunk = 2048, kDotTargetWaves = 256 * 16;

template <int F, int XG, int XX>
int launch_edge_dot(const int64_t* rowptr, const int32_t* idx, const int32_t* perm, const void* g, int64_t ldg, const void* x,
                    int64_t ldx, int64_t n_rows, int64_t nnz, float* out_sorted, float* out_orig, hipStream_t s) {
  // entries per wave: enough waves to fill the chip on a short list, at most kDotMaxChunk on a long one (the row search and
  // the first g piece are paid once per chunk); no output bit depends on it
  int64_t chunk = (nnz + kDotTargetWaves - 1) / kDotTargetWaves;
  chunk = (chunk + kWave - 1) / kWave * kWave;
  chunk = chunk < kWave ? kWave : chunk > kDotMaxChunk ? kDotMaxChunk : chunk;
  const int64_t waves = (nnz + chunk - 1) / chunk;
  const int64_t blocks = (waves + kWavesPerBlock - 1) / kWavesPerBlock;
  hipLaunchKernelGGL((edge_dot_kernel<F, XG, XX>), dim3((unsigned)blocks), dim3(kBlock), 0, s, rowptr, idx, perm,
                     static_cast<const char*>(g), ldg, static_cast<const char*>(x), ldx, n_rows, nnz, chunk, out_sorted,
                     out_orig);
  PG_CHECK_LAUNCH("pangnn_edge_dot_mixed");
  return 0;
}

template <int F, typename... A>
int dispatch_dot(int xg, int xx, A... a) {
  if (xg == 0 && xx == 0) return launch_edge_dot<F, 0, 0>(a...);
  if constexpr (F >= 32) {                                   // 2-byte rows: the widths the propagate gathers in that type
    if (xg == 0) return xx == 1 ? launch_edge_dot<F, 0, 1>(a...) : launch_edge_dot<F, 0, 2>(a...);
    if (xx == 0) return xg == 1 ? launch_edge_dot<F, 1, 0>(a...) : launch_edge_dot<F, 2, 0>(a...);
    return xg == 1 ? launch_edge_dot<F, 1, 1>(a...) : launch_edge_dot<F, 2, 2>(a...);
  }
  return PANGNN_E_BADARG;
}

// ---- the backward of gcn_norm -----------------------------------------------------------------------------------------
constexpr int kNG = 16;                       // lanes per node / per segment

// sum over entries [lo, hi) of one CSR order of (gw w)[perm[k]] dis[other[k]]: lane j of the group adds the entries lo + j,
// lo + j + 16, ... in ascending position, then the 16 lane sums meet in a fixed butterfly (every lane ends with the same bits)
__device__ __forceinline__ float norm_walk(const int32_t* __restrict__ other, const int32_t* __restrict__ perm, int64_t lo,
                                           int64_t hi, int j, const float* __restrict__ w, const float* __restrict__ gw,
                                           const float* __restrict__ dis) {
  float s = 0.f;
  for (int64_t k = lo + j; k < hi; k += kNG) {
    const int32_t e = perm[k];
    s = fmaf(gw[e] * w[e], dis[other[k]], s);
  }
  return group_sum<kNG>(s);
}

// the partials [lo, hi) of a hub-carrying order, added in index order by the same scheme
__device__ __forceinline__ float parts_walk(const float* __restrict__ parts, int64_t lo, int64_t hi, int j) {
  float s = 0.f;
  for (int64_t p = lo + j; p < hi; p += kNG) s += parts[p];
  return group_sum<kNG>(s);
}

struct NormOrder {
  const int64_t* rowptr; const int32_t* other; const int32_t* perm;
  const int64_t* seg_ptr; const int64_t* parts_rowptr; int64_t nseg; float* parts;     // seg_ptr == NULL: walk the rows
};

// one 16-lane group per segment of a hub-carrying CSR order
__global__ __launch_bounds__(kBlock) void norm_seg_kernel(NormOrder o, const float* __restrict__ w,
                                                          const float* __restrict__ gw, const float* __restrict__ dis) {
  const int j = threadIdx.x % kNG;
  const int64_t v = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kNG;
  if (v >= o.nseg) return;                                  // a whole group leaves together
  const float s = norm_walk(o.other, o.perm, o.seg_ptr[v], o.seg_ptr[v + 1], j, w, gw, dis);
  if (j == 0) o.parts[v] = s;
}

__device__ __forceinline__ float norm_order_sum(const NormOrder& o, int64_t v, int j, const float* w, const float* gw,
                                                const float* dis) {
  if (o.seg_ptr) return parts_walk(o.parts, o.parts_rowptr[v], o.parts_rowptr[v + 1], j);
  return norm_walk(o.other, o.perm, o.rowptr[v], o.rowptr[v + 1], j, w, gw, dis);
}

// one 16-lane group per node: in-edges, then out-edges; gdeg[v] = -1/2 dis[v]^3 gdis[v]
__global__ __launch_bounds__(kBlock) void norm_node_kernel(NormOrder dst, NormOrder src, int64_t n, const float* __restrict__ w,
                                                           const float* __restrict__ gw, const float* __restrict__ dis,
                                                           float* __restrict__ gdeg) {
  const int j = threadIdx.x % kNG;
  const int64_t v = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kNG;
  if (v >= n) return;
  const float a = norm_order_sum(dst, v, j, w, gw, dis);
  const float b = norm_order_sum(src, v, j, w, gw, dis);
  if (j == 0) {
    const float d = dis[v];
    // a node without weight on its in-edges: torch's masked_fill stops the gradient there (and 0 * inf is defined as 0)
    gdeg[v] = d == 0.f ? 0.f : -0.5f * (d * d * d) * (a + b);
  }
}

// the edge pass, in the caller's order
__global__ __launch_bounds__(kBlock) void norm_edge_kernel(const int64_t* __restrict__ ei, int64_t ld, int64_t e,
                                                           const float* __restrict__ gw, const float* __restrict__ dis,
                                                           const float* __restrict__ gdeg, float* __restrict__ gweight) {
  for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < e; k += (int64_t)gridDim.x * kBlock) {
    const int64_t s = ei[k], d = ei[ld + k];
    gweight[k] = fmaf(dis[s] * dis[d], gw[k], gdeg[d]);
  }
}

}  // namespace
}  // namespace pangnn

using namespace pangnn;

extern "C" int pangnn_edge_dot_mixed(const int64_t* rowptr, const int32_t* idx, const int32_t* perm, const void* g,
                                     int32_t g_dtype, int64_t ldg, int64_t g_rows, const void* x, int32_t x_dtype, int64_t ldx,
                                     int64_t x_rows, int64_t n_rows, int64_t nnz, int32_t F, float* out_sorted, float* out_orig,
                                     pangnn_stream_t stream) {
  const char* fn = "pangnn_edge_dot_mixed";
  PG_CHECK_ARG(row_width_ok(F), PANGNN_E_BADARG, "%s: F must be 16, 32, 64, 128 or 256 (got %d)", fn, (int)F);
  PG_CHECK_ARG(row_dtype_ok(g_dtype) && row_dtype_ok(x_dtype), PANGNN_E_BADARG, "%s: g_dtype and x_dtype must be 0, 1 or 2", fn);
  PG_CHECK_ARG(g_dtype == PANGNN_DTYPE_F32 || x_dtype == PANGNN_DTYPE_F32 || g_dtype == x_dtype, PANGNN_E_BADARG,
               "%s: the 2-byte rows of one call are all bfloat16 or all float16", fn);
  PG_CHECK_ARG(F >= 32 || (g_dtype == PANGNN_DTYPE_F32 && x_dtype == PANGNN_DTYPE_F32), PANGNN_E_BADARG,
               "%s: 2-byte rows need F in {32, 64, 128, 256} (got %d)", fn, (int)F);
  PG_CHECK_ARG(n_rows >= 0 && nnz >= 0 && g_rows >= n_rows && x_rows >= 0 && ldg >= F && ldx >= F, PANGNN_E_BADARG,
               "%s: bad size (n_rows=%lld nnz=%lld g_rows=%lld x_rows=%lld ldg=%lld ldx=%lld)", fn, (long long)n_rows,
               (long long)nnz, (long long)g_rows, (long long)x_rows, (long long)ldg, (long long)ldx);
  PG_CHECK_ARG((n_rows > 0 && x_rows > 0) || nnz == 0, PANGNN_E_BADARG, "%s: entries without rows", fn);
  PG_CHECK_ARG(nnz < ((int64_t)1 << 31) && n_rows < ((int64_t)1 << 31) && x_rows < ((int64_t)1 << 31), PANGNN_E_TOOLARGE,
               "%s: sizes exceed the int32 index range", fn);
  if (nnz == 0) return 0;
  PG_CHECK_ARG(rowptr && idx && g && x && out_sorted && (perm || !out_orig), PANGNN_E_BADARG, "%s: null pointer", fn);
  PG_CHECK_ARG(rows_aligned(g, g_dtype, ldg) && rows_aligned(x, x_dtype, ldx), PANGNN_E_ALIGN,
               "%s: rows must start on 16 bytes (f32) / 8 bytes (2-byte rows): ld a multiple of 4", fn);
  hipStream_t s = (hipStream_t)stream;
#define PG_DOT_CASE(FF) \
  case FF: return dispatch_dot<FF>(g_dtype, x_dtype, rowptr, idx, perm, g, ldg, x, ldx, n_rows, nnz, out_sorted, out_orig, s);
  switch (F) {
    PG_DOT_CASE(16)
    PG_DOT_CASE(32)
    PG_DOT_CASE(64)
    PG_DOT_CASE(128)
    PG_DOT_CASE(256)
  }
#undef PG_DOT_CASE
  return PANGNN_E_BADARG;
}

// workspace: gdeg | parts_dst | parts_src, each a whole number of 16 bytes (float counts rounded up to 4)
extern "C" int64_t pangnn_gcn_norm_bwd_workspace_bytes(int64_t num_nodes, int64_t num_seg_dst, int64_t num_seg_src) {
  if (num_nodes < 0 || num_seg_dst < 0 || num_seg_src < 0) return 0;
  return (int64_t)((align_up(num_nodes, 4) + align_up(num_seg_dst, 4) + align_up(num_seg_src, 4) + 4) * sizeof(float));
}

extern "C" int pangnn_gcn_norm_bwd_f32(const int64_t* edge_index, int64_t ld, int64_t num_edges, int64_t num_nodes,
                                       const int64_t* rowptr_dst, const int32_t* other_dst, const int32_t* perm_dst,
                                       const int64_t* seg_ptr_dst, const int64_t* parts_rowptr_dst, int64_t num_seg_dst,
                                       const int64_t* rowptr_src, const int32_t* other_src, const int32_t* perm_src,
                                       const int64_t* seg_ptr_src, const int64_t* parts_rowptr_src, int64_t num_seg_src,
                                       const float* w, const float* gw, const float* dis, float* gweight, void* workspace,
                                       int64_t workspace_bytes, pangnn_stream_t stream) {
  const char* fn = "pangnn_gcn_norm_bwd_f32";
  PG_CHECK_ARG(num_edges >= 0 && num_nodes >= 0 && ld >= num_edges, PANGNN_E_BADARG, "%s: bad size", fn);
  PG_CHECK_ARG(num_nodes > 0 || num_edges == 0, PANGNN_E_BADARG, "%s: edges without nodes", fn);
  PG_CHECK_ARG(num_edges < ((int64_t)1 << 31) && num_nodes < ((int64_t)1 << 31), PANGNN_E_TOOLARGE,
               "%s: sizes exceed the int32 index range", fn);
  if (num_edges == 0) return 0;
  PG_CHECK_ARG(edge_index && rowptr_dst && other_dst && perm_dst && rowptr_src && other_src && perm_src && w && gw && dis &&
                   gweight, PANGNN_E_BADARG, "%s: null pointer", fn);
  PG_CHECK_ARG((seg_ptr_dst == nullptr) == (parts_rowptr_dst == nullptr) && (seg_ptr_src == nullptr) == (parts_rowptr_src == nullptr),
               PANGNN_E_BADARG, "%s: seg_ptr and parts_rowptr go together", fn);
  PG_CHECK_ARG(num_seg_dst >= 0 && num_seg_src >= 0 && (!seg_ptr_dst || num_seg_dst >= num_nodes) &&
                   (!seg_ptr_src || num_seg_src >= num_nodes), PANGNN_E_BADARG,
               "%s: a segmented order has at least one segment per row", fn);
  const int64_t nsd = seg_ptr_dst ? num_seg_dst : 0, nss = seg_ptr_src ? num_seg_src : 0;
  PG_CHECK_ARG(workspace && workspace_bytes >= pangnn_gcn_norm_bwd_workspace_bytes(num_nodes, nsd, nss), PANGNN_E_WORKSPACE,
               "%s: workspace smaller than pangnn_gcn_norm_bwd_workspace_bytes()", fn);
  PG_CHECK_ARG(aligned16(workspace), PANGNN_E_ALIGN, "%s: workspace must be 16-byte aligned", fn);
  hipStream_t s = (hipStream_t)stream;
  float* gdeg = static_cast<float*>(workspace);
  float* parts_dst = gdeg + align_up(num_nodes, 4);
  float* parts_src = parts_dst + align_up(nsd, 4);
  const NormOrder dst{rowptr_dst, other_dst, perm_dst, seg_ptr_dst, parts_rowptr_dst, nsd, parts_dst};
  const NormOrder src{rowptr_src, other_src, perm_src, seg_ptr_src, parts_rowptr_src, nss, parts_src};
  for (const NormOrder* o : {&dst, &src}) {
    if (!o->seg_ptr) continue;
    hipLaunchKernelGGL(norm_seg_kernel, dim3((unsigned)blocks_for(o->nseg, kBlock / kNG)), dim3(kBlock), 0, s, *o, w, gw, dis);
    PG_CHECK_LAUNCH("pangnn_gcn_norm_bwd_f32(segments)");
  }
  hipLaunchKernelGGL(norm_node_kernel, dim3((unsigned)blocks_for(num_nodes, kBlock / kNG)), dim3(kBlock), 0, s, dst, src,
                     num_nodes, w, gw, dis, gdeg);
  PG_CHECK_LAUNCH("pangnn_gcn_norm_bwd_f32(nodes)");
  int64_t blocks = blocks_for(num_edges, kBlock);
  blocks = blocks > 8192 ? 8192 : blocks;
  hipLaunchKernelGGL(norm_edge_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, edge_index, ld, num_edges, gw, dis, gdeg,
                     gweight);
  PG_CHECK_LAUNCH("pangnn_gcn_norm_bwd_f32(edges)");
  return 0;
}
