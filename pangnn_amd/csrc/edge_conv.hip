// Fused EdgeConv (convolution.py:5-23), fp32, gfx950: max-aggregated mlp(cat[x_i, x_j - x_i]) without any edge-sized tensor.
//
//   first layer by linearity (node level, done by the caller):  u = x (Wa - Wb)^T + b1,  v = x Wb^T      [N, OUT] each
//   per edge e = (j -> i):   h_e = relu(u_i + v_j),   m_e = W2 h_e
//   out[i] = b2 + max_e m_e  (rows without in-edges: 0),   arg[i] = original id of the winning edge (-1)
//
// Forward: one wavefront owns a CHUNK of consecutive 32-entry tiles of the by-target CSR, whatever rows they belong to.  Per
// tile the 32 h rows are gathered into a padded LDS image and multiplied with W2 (LDS resident for the life of the block) on
// the f32 MFMA (v_mfma_f32_32x32x2_f32: exact fp32 FMA chains), oriented M[e][c] = sum_k h[e][k] W2[c][k] so that a lane
// holds one channel; the tile goes back to LDS and every lane walks its channel down the 32 entries with a running
// (max, arg) that is flushed whenever the target row changes (row ids are wave-uniform).  The open row is carried from tile
// to tile in registers.  A row that lies inside one chunk is written directly; a row that crosses chunk borders — a hub —
// leaves one partial per chunk (the chunk's "tail" while it goes on, its "head" where it closes) and a second small kernel
// combines them.  (max, arg) are combined under a total order — NaN first, then the larger value, then the smaller edge id —
// which is what a serial walk in ascending edge id with "first maximum wins, NaN propagates" computes (segment_max_kernel),
// so the result does not depend on the chunking: no atomics, bitwise reproducible.
//
// Backward: s_e[c] = g[i][c] * [arg[i][c] == e],  gh_e = (W2^T s_e) * [h_e > 0],  gu[i] = sum_{e into i} gh_e,
// gv[j] = sum_{e out of j} gh_e,  gW2 = sum_e s_e h_e^T.  The same chunked walk, once over the by-target CSR (gu, gW2) and once
// over the by-source CSR (gv): h_e is recomputed, the products run on the f32 MFMA, a tile none of whose edges won a channel
// (one byte per edge says so) skips them, the per-row sums are taken in CSR order with the same head / tail partials summed
// in a fixed order, and gW2 leaves each block as one slab that a last kernel adds in index order.  No float atomics.
#include "common.h"

namespace pangnn {

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int kTile = 32;            // CSR entries per tile
constexpr int kFwdChunks = 4096;     // most chunks (= waves with work) of a forward launch: bounds the partial buffers
constexpr int kBwdChunks = 2048;     // ... of a backward pass (each block also leaves an OUT x OUT slab)

template <int OUT> struct Cfg {
  static constexpr int RS = OUT + 4;          // padded LDS row stride (floats): 16-byte aligned, conflict-free b128 column reads
  static constexpr int LPR = OUT / 4;         // lanes that load one row (a float4 each)
  static constexpr int RPI = 64 / LPR;        // rows per wave-wide load
  static constexpr int CPL = OUT / 64;        // channels per lane in the row walk
  static constexpr int NB = OUT / 32;         // 32-wide column blocks
  static constexpr int FWD_WAVES = 4;
  static constexpr int BWD_WAVES = OUT == 64 ? 4 : 2;      // W2 + two tiles per wave within 160 KiB of LDS
};

// relu as torch computes it: a NaN stays a NaN (fmed3f / fmaxf would return 0), so that the max-aggregation sees it
__device__ __forceinline__ float relu1(float x) { return x < 0.f ? 0.f : x; }

// does candidate (b, ib) replace (a, ia)?  Total order: NaN beats numbers, larger beats smaller, the smaller edge id wins ties.
__device__ __forceinline__ bool better(float b, int ib, float a, int ia) {
  const bool nan_a = a != a, nan_b = b != b;
  return nan_a ? (nan_b && ib < ia) : (nan_b || b > a || (b == a && ib < ia));
}

template <int OUT>
__device__ __forceinline__ void stage_w2(const float* __restrict__ w2, float* Wl, int nthreads) {
  constexpr int RS = Cfg<OUT>::RS;
  for (int i = threadIdx.x; i < OUT * OUT / 4; i += nthreads) {
    const int j = i / (OUT / 4), k4 = i % (OUT / 4);
    *reinterpret_cast<float4*>(Wl + j * RS + 4 * k4) = reinterpret_cast<const float4*>(w2)[i];
  }
}

struct ChunkPlan { int64_t entries; int64_t n_chunks; };
ChunkPlan plan_chunks(int64_t num_edges, int max_chunks) {
  const int64_t n_tiles = (num_edges + kTile - 1) / kTile;
  const int64_t tiles = n_tiles == 0 ? 1 : (n_tiles + max_chunks - 1) / max_chunks;
  ChunkPlan p;
  p.entries = tiles * kTile;
  p.n_chunks = (num_edges + p.entries - 1) / p.entries;
  return p;
}

struct FwdParams {
  const float* u; const float* v; int64_t ldu, ldv;
  const float* w2; const float* b2;
  const int64_t* rowptr; const int32_t* col; const int32_t* perm; const int64_t* ei; int64_t ld; int64_t E;
  float* out; int32_t* arg; int64_t ldo;
  int64_t chunk_entries; int64_t n_chunks;
  int32_t* head_row; float* head_val; int32_t* head_arg; float* tail_val; int32_t* tail_arg;
};

template <int OUT>
__global__ __launch_bounds__(Cfg<OUT>::FWD_WAVES * 64) void edge_conv_fwd_kernel(FwdParams a) {
  using C = Cfg<OUT>;
  constexpr int RS = C::RS, WAVES = C::FWD_WAVES;
  __shared__ __attribute__((aligned(16))) float lds[OUT * RS + WAVES * kTile * RS];
  float* Wl = lds;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  float* Ht = lds + OUT * RS + wave * (kTile * RS);
  stage_w2<OUT>(a.w2, Wl, WAVES * 64);
  __syncthreads();
  const int64_t chunk = (int64_t)blockIdx.x * WAVES + wave;
  if (chunk >= a.n_chunks) return;                       // (no block-wide barrier below)
  const int64_t pos0 = chunk * a.chunk_entries;
  const int64_t pos1 = pos0 + a.chunk_entries < a.E ? pos0 + a.chunk_entries : a.E;
  const int r = lane & 31, hh = lane >> 5;
  int open = -1, head_row = -1;
  float best[C::CPL];
  int bi[C::CPL];
#pragma unroll
  for (int q = 0; q < C::CPL; ++q) { best[q] = 0.f; bi[q] = -1; }

  // the finished row `row`: written in place when it began inside this chunk, else it is the chunk's head partial
  auto flush = [&](int row) {
    const bool began_here = a.rowptr[row] >= pos0;
#pragma unroll
    for (int q = 0; q < C::CPL; ++q) {
      const int c = lane + 64 * q;
      if (began_here) {
        a.out[(int64_t)row * a.ldo + c] = best[q] + a.b2[c];
        a.arg[(int64_t)row * a.ldo + c] = bi[q];
      } else {
        a.head_val[chunk * OUT + c] = best[q];
        a.head_arg[chunk * OUT + c] = bi[q];
      }
    }
    if (!began_here) head_row = row;
  };

  for (int64_t base = pos0; base < pos1; base += kTile) {
    const int64_t p = base + r;
    const bool valid = p < pos1;
    const int o = valid ? a.perm[p] : -1;
    int id = -1;                                         // lanes 0-31: source of entry r, lanes 32-63: its target row
    if (valid) id = hh ? (int)a.ei[a.ld + o] : a.col[p];
    // ---- h tile: relu(u[target] + v[source]), LPR lanes per row
    const int c4 = lane % C::LPR, r4 = lane / C::LPR;
#pragma unroll
    for (int it = 0; it < kTile / C::RPI; ++it) {
      const int row = it * C::RPI + r4;
      const int js = __shfl(id, row), is = __shfl(id, 32 + row);
      float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
      if (js >= 0) {
        const float4 vv = *reinterpret_cast<const float4*>(a.v + (int64_t)js * a.ldv + 4 * c4);
        const float4 uu = *reinterpret_cast<const float4*>(a.u + (int64_t)is * a.ldu + 4 * c4);
        h.x = relu1(uu.x + vv.x); h.y = relu1(uu.y + vv.y); h.z = relu1(uu.z + vv.z); h.w = relu1(uu.w + vv.w);
      }
      *reinterpret_cast<float4*>(Ht + row * RS + 4 * c4) = h;
    }
    wave_lds_sync();
    // ---- M[e][c] = sum_k h[e][k] W2[c][k]: lane (r, hh) gets entries acc_row(reg, hh), channel 32 b + r
    f32x16 acc[C::NB];
#pragma unroll
    for (int b = 0; b < C::NB; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[b][i] = 0.f;
#pragma unroll 2
    for (int i = 0; i < OUT / 8; ++i) {
      const int k4 = (OUT / 8) * hh + i;
      const float4 hf = *reinterpret_cast<const float4*>(Ht + r * RS + 4 * k4);
#pragma unroll
      for (int b = 0; b < C::NB; ++b) {
        const float4 wf = *reinterpret_cast<const float4*>(Wl + (32 * b + r) * RS + 4 * k4);
        acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(hf.x, wf.x, acc[b], 0, 0, 0);
        acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(hf.y, wf.y, acc[b], 0, 0, 0);
        acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(hf.z, wf.z, acc[b], 0, 0, 0);
        acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(hf.w, wf.w, acc[b], 0, 0, 0);
      }
    }
    wave_lds_sync();                                     // every read of the h tile is done: the messages take its place
#pragma unroll
    for (int b = 0; b < C::NB; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) Ht[acc_row(i, hh) * RS + 32 * b + r] = acc[b][i];
    wave_lds_sync();
    // ---- running (max, arg) per channel down the tile, flushed at every change of the target row
    const int n_here = (int)(pos1 - base < kTile ? pos1 - base : kTile);
#pragma nounroll
    for (int t = 0; t < n_here; ++t) {
      const int row = __builtin_amdgcn_readlane(id, 32 + t);
      const int oe = __builtin_amdgcn_readlane(o, t);
      bool fresh = false;
      if (row != open) {
        if (open >= 0) flush(open);
        open = row;
        fresh = true;
      }
#pragma unroll
      for (int q = 0; q < C::CPL; ++q) {
        const float val = Ht[t * RS + lane + 64 * q];
        if (fresh || better(val, oe, best[q], bi[q])) { best[q] = val; bi[q] = oe; }
      }
    }
    wave_lds_sync();                                     // the next tile overwrites Ht
  }
  if (open >= 0) {
    if (a.rowptr[open + 1] <= pos1) {
      flush(open);
    } else {                                             // the row goes on in the next chunk
#pragma unroll
      for (int q = 0; q < C::CPL; ++q) {
        a.tail_val[chunk * OUT + lane + 64 * q] = best[q];
        a.tail_arg[chunk * OUT + lane + 64 * q] = bi[q];
      }
    }
  }
  if (lane == 0) a.head_row[chunk] = head_row;
}

// a row that crossed chunk borders: its head partial (chunk w, where it closed) with the tails of the chunks before, back to
// the chunk in which it began.  One block per chunk; 256 threads = 256 / OUT groups that stride the tails.
template <int OUT>
__global__ __launch_bounds__(256) void edge_conv_fwd_combine_kernel(FwdParams a) {
  constexpr int G = 256 / OUT;
  __shared__ float sv[G][OUT];
  __shared__ int sa[G][OUT];
  __shared__ int sh[G][OUT];
  const int64_t w = blockIdx.x;
  const int row = a.head_row[w];
  if (row < 0) return;
  const int64_t wa = a.rowptr[row] / a.chunk_entries;
  const int g = threadIdx.x / OUT, c = threadIdx.x % OUT;
  float best = 0.f;
  int bi = -1, has = 0;
  if (g == 0) { best = a.head_val[w * OUT + c]; bi = a.head_arg[w * OUT + c]; has = 1; }
  for (int64_t t = wa + g; t < w; t += G) {
    const float val = a.tail_val[t * OUT + c];
    const int o = a.tail_arg[t * OUT + c];
    if (!has || better(val, o, best, bi)) { best = val; bi = o; has = 1; }
  }
  sv[g][c] = best; sa[g][c] = bi; sh[g][c] = has;
  __syncthreads();
  if (g == 0) {
    for (int k = 1; k < G; ++k)
      if (sh[k][c] && better(sv[k][c], sa[k][c], best, bi)) { best = sv[k][c]; bi = sa[k][c]; }
    a.out[(int64_t)row * a.ldo + c] = best + a.b2[c];
    a.arg[(int64_t)row * a.ldo + c] = bi;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void edge_conv_mark_winners_kernel(const int32_t* __restrict__ arg, int64_t total,
                                                                        uint8_t* __restrict__ win) {
  for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kBlock) {
    const int32_t e = arg[t];
    if (e >= 0) win[e] = 1;                  // every writer stores the same byte
  }
}

struct BwdParams {
  const float* u; const float* v; const float* g; int64_t ldu, ldv, ldg;
  const int32_t* arg;                        // [N, OUT] contiguous
  const float* w2;
  const int64_t* rowptr; const int32_t* other; const int32_t* perm; const int64_t* ei; int64_t ld; int64_t E;
  const uint8_t* win;
  float* grad; int64_t ldo;                  // gu (by-target pass) / gv (by-source pass)
  int64_t chunk_entries; int64_t n_chunks;
  int32_t* head_row; float* head_val; float* tail_val;
  float* slabs;                              // [gridDim.x][OUT * OUT], by-target pass only
};

template <int OUT, bool BY_SRC>
__global__ __launch_bounds__(Cfg<OUT>::BWD_WAVES * 64) void edge_conv_bwd_kernel(BwdParams a) {
  using C = Cfg<OUT>;
  constexpr int RS = C::RS, WAVES = C::BWD_WAVES, NB = C::NB;
  constexpr bool WGRAD = !BY_SRC;
  constexpr int PER_WAVE = 2 * kTile * RS;               // h tile | s tile (later dL/dh)
  static_assert(PER_WAVE >= 32 * 33, "the slab reduction borrows a wave's tiles");
  __shared__ __attribute__((aligned(16))) float lds[OUT * RS + WAVES * PER_WAVE];
  float* Wl = lds;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  float* Ht = lds + OUT * RS + wave * PER_WAVE;
  float* St = Ht + kTile * RS;
  stage_w2<OUT>(a.w2, Wl, WAVES * 64);
  __syncthreads();
  const int64_t chunk = (int64_t)blockIdx.x * WAVES + wave;
  const bool working = chunk < a.n_chunks;
  const int64_t pos0 = chunk * a.chunk_entries;
  const int64_t pos1 = !working ? pos0 : (pos0 + a.chunk_entries < a.E ? pos0 + a.chunk_entries : a.E);
  const int r = lane & 31, hh = lane >> 5;
  int open = -1, head_row = -1;
  float sum[C::CPL];
#pragma unroll
  for (int q = 0; q < C::CPL; ++q) sum[q] = 0.f;
  f32x16 accw[WGRAD ? NB : 1][WGRAD ? NB : 1];           // gW2[32 bi + acc_row][32 bj + r] over this wave's tiles
#pragma unroll
  for (int x = 0; x < (WGRAD ? NB : 1); ++x)
#pragma unroll
    for (int y = 0; y < (WGRAD ? NB : 1); ++y)
#pragma unroll
      for (int i = 0; i < 16; ++i) accw[x][y][i] = 0.f;

  auto flush = [&](int row) {
    const bool began_here = a.rowptr[row] >= pos0;
#pragma unroll
    for (int q = 0; q < C::CPL; ++q) {
      const int c = lane + 64 * q;
      if (began_here) a.grad[(int64_t)row * a.ldo + c] = sum[q];
      else a.head_val[chunk * OUT + c] = sum[q];
    }
    if (!began_here) head_row = row;
  };

  for (int64_t base = pos0; base < pos1; base += kTile) {
    const int64_t p = base + r;
    const bool valid = p < pos1;
    const int o = valid ? a.perm[p] : -1;
    int rid = -1, it_ = 0, jt_ = 0;                      // row of the walked CSR; target i and source j of the entry
    bool won = false;
    if (valid) {
      const int oth = a.other[p];
      rid = (int)a.ei[(BY_SRC ? 0 : a.ld) + o];
      it_ = BY_SRC ? oth : rid;
      jt_ = BY_SRC ? rid : oth;
      won = a.win[o] != 0;
    }
    const bool any = __ballot(won) != 0ull;              // wave-uniform
    if (any) {
      const int c4 = lane % C::LPR, r4 = lane / C::LPR;
#pragma unroll
      for (int it = 0; it < kTile / C::RPI; ++it) {
        const int row = it * C::RPI + r4;
        const int oe = __shfl(o, row), is = __shfl(it_, row), js = __shfl(jt_, row);
        float4 h = make_float4(0.f, 0.f, 0.f, 0.f), s = make_float4(0.f, 0.f, 0.f, 0.f);
        if (oe >= 0) {
          const float4 vv = *reinterpret_cast<const float4*>(a.v + (int64_t)js * a.ldv + 4 * c4);
          const float4 uu = *reinterpret_cast<const float4*>(a.u + (int64_t)is * a.ldu + 4 * c4);
          const float4 gg = *reinterpret_cast<const float4*>(a.g + (int64_t)is * a.ldg + 4 * c4);
          const int4 aa = *reinterpret_cast<const int4*>(a.arg + (int64_t)is * OUT + 4 * c4);
          h.x = relu1(uu.x + vv.x); h.y = relu1(uu.y + vv.y); h.z = relu1(uu.z + vv.z); h.w = relu1(uu.w + vv.w);
          s.x = aa.x == oe ? gg.x : 0.f; s.y = aa.y == oe ? gg.y : 0.f;
          s.z = aa.z == oe ? gg.z : 0.f; s.w = aa.w == oe ? gg.w : 0.f;
        }
        *reinterpret_cast<float4*>(Ht + row * RS + 4 * c4) = h;
        *reinterpret_cast<float4*>(St + row * RS + 4 * c4) = s;
      }
      wave_lds_sync();
      // ---- P[e][k] = sum_c s[e][c] W2[c][k]: lane (r, hh) gets entries acc_row(reg, hh), column 32 b + r
      f32x16 acc[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[b][i] = 0.f;
#pragma unroll 2
      for (int i = 0; i < OUT / 8; ++i) {
        const int k4 = (OUT / 8) * hh + i;
        const float4 sf = *reinterpret_cast<const float4*>(St + r * RS + 4 * k4);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const float* wc = Wl + (4 * k4) * RS + 32 * b + r;
          acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(sf.x, wc[0], acc[b], 0, 0, 0);
          acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(sf.y, wc[RS], acc[b], 0, 0, 0);
          acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(sf.z, wc[2 * RS], acc[b], 0, 0, 0);
          acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(sf.w, wc[3 * RS], acc[b], 0, 0, 0);
        }
      }
      if (WGRAD) {
        // ---- gW2[c][k] += sum_e s[e][c] h[e][k]
#pragma unroll 2
        for (int st = 0; st < kTile / 2; ++st) {
          const int e = 2 * st + hh;
          float sa[NB], hb[NB];
#pragma unroll
          for (int b = 0; b < NB; ++b) { sa[b] = St[e * RS + 32 * b + r]; hb[b] = Ht[e * RS + 32 * b + r]; }
#pragma unroll
          for (int x = 0; x < NB; ++x)
#pragma unroll
            for (int y = 0; y < NB; ++y)
              accw[WGRAD ? x : 0][WGRAD ? y : 0] =
                  __builtin_amdgcn_mfma_f32_32x32x2f32(sa[x], hb[y], accw[WGRAD ? x : 0][WGRAD ? y : 0], 0, 0, 0);
        }
      }
      wave_lds_sync();                                   // every read of the s tile is done: dL/dh takes its place
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int e = acc_row(i, hh), k = 32 * b + r;
          St[e * RS + k] = Ht[e * RS + k] > 0.f ? acc[b][i] : 0.f;
        }
      wave_lds_sync();
    }
    // ---- per-row sums down the tile in CSR order
    const int n_here = (int)(pos1 - base < kTile ? pos1 - base : kTile);
#pragma nounroll
    for (int t = 0; t < n_here; ++t) {
      const int row = __builtin_amdgcn_readlane(rid, t);
      if (row != open) {
        if (open >= 0) flush(open);
        open = row;
#pragma unroll
        for (int q = 0; q < C::CPL; ++q) sum[q] = 0.f;
      }
      if (any) {
#pragma unroll
        for (int q = 0; q < C::CPL; ++q) sum[q] += St[t * RS + lane + 64 * q];
      }
    }
    wave_lds_sync();
  }
  if (working) {
    if (open >= 0) {
      if (a.rowptr[open + 1] <= pos1) {
        flush(open);
      } else {
#pragma unroll
        for (int q = 0; q < C::CPL; ++q) a.tail_val[chunk * OUT + lane + 64 * q] = sum[q];
      }
    }
    if (lane == 0) a.head_row[chunk] = head_row;
  }
  if (WGRAD) {
    // the block's slab: 32 x 32 blocks one at a time through LDS, the waves' parts added in wave order
    float* slab = a.slabs + (int64_t)blockIdx.x * (OUT * OUT);
#pragma unroll
    for (int x = 0; x < NB; ++x)
#pragma unroll
      for (int y = 0; y < NB; ++y) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i) Ht[acc_row(i, hh) * 33 + r] = accw[WGRAD ? x : 0][WGRAD ? y : 0][i];
        __syncthreads();
        for (int idx = threadIdx.x; idx < 32 * 32; idx += WAVES * 64) {
          const int rr = idx >> 5, cc = idx & 31;
          float s = 0.f;
          for (int w = 0; w < WAVES; ++w) s += lds[OUT * RS + w * PER_WAVE + rr * 33 + cc];
          slab[(32 * x + rr) * OUT + 32 * y + cc] = s;
        }
      }
  }
}

template <int OUT>
__global__ __launch_bounds__(256) void edge_conv_bwd_combine_kernel(BwdParams a) {
  constexpr int G = 256 / OUT;
  __shared__ float sv[G][OUT];
  const int64_t w = blockIdx.x;
  const int row = a.head_row[w];
  if (row < 0) return;
  const int64_t wa = a.rowptr[row] / a.chunk_entries;
  const int g = threadIdx.x / OUT, c = threadIdx.x % OUT;
  float s = 0.f;
  for (int64_t t = wa + g; t < w; t += G) s += a.tail_val[t * OUT + c];
  sv[g][c] = s;
  __syncthreads();
  if (g == 0) {
    for (int k = 1; k < G; ++k) s += sv[k][c];
    a.grad[(int64_t)row * a.ldo + c] = s + a.head_val[w * OUT + c];
  }
}

__global__ __launch_bounds__(kSumThreads) void edge_conv_slab_sum_kernel(const float* __restrict__ slabs, int n_slabs,
                                                                         int len, float* __restrict__ gw2) {
  const int i = blockIdx.x * kWave + (threadIdx.x & (kWave - 1));
  const float s = ordered_parts_sum(slabs, n_slabs, len, i, len);
  if (threadIdx.x < kWave && i < len) gw2[i] = s;
}

// scratch layout shared by the query and the launchers
struct Scratch { int64_t head_row, head_val, head_arg, tail_val, tail_arg, win, slabs, total; };
Scratch scratch_layout(int64_t num_edges, int out_dim, bool backward) {
  const ChunkPlan cp = plan_chunks(num_edges, backward ? kBwdChunks : kFwdChunks);
  const int64_t nc = cp.n_chunks > 0 ? cp.n_chunks : 1;
  Scratch s;
  int64_t off = 0;
  s.head_row = off; off += align_up(nc * 4, 16);
  s.head_val = off; off += align_up(nc * out_dim * 4, 16);
  s.head_arg = off; off += backward ? 0 : align_up(nc * out_dim * 4, 16);
  s.tail_val = off; off += align_up(nc * out_dim * 4, 16);
  s.tail_arg = off; off += backward ? 0 : align_up(nc * out_dim * 4, 16);
  s.win = off; off += backward ? align_up(num_edges > 0 ? num_edges : 1, 16) : 0;
  const int waves = out_dim == 64 ? Cfg<64>::BWD_WAVES : Cfg<128>::BWD_WAVES;
  s.slabs = off; off += backward ? align_up(((nc + waves - 1) / waves) * (int64_t)out_dim * out_dim * 4, 16) : 0;
  s.total = off;
  return s;
}

template <int OUT>
int launch_fwd(FwdParams a, hipStream_t stream) {
  const int64_t blocks = (a.n_chunks + Cfg<OUT>::FWD_WAVES - 1) / Cfg<OUT>::FWD_WAVES;
  hipLaunchKernelGGL(edge_conv_fwd_kernel<OUT>, dim3((unsigned)blocks), dim3(Cfg<OUT>::FWD_WAVES * 64), 0, stream, a);
  PG_CHECK_LAUNCH("edge_conv_fwd_kernel");
  hipLaunchKernelGGL(edge_conv_fwd_combine_kernel<OUT>, dim3((unsigned)a.n_chunks), dim3(256), 0, stream, a);
  PG_CHECK_LAUNCH("edge_conv_fwd_combine_kernel");
  return 0;
}

template <int OUT, bool BY_SRC>
int launch_bwd_pass(BwdParams a, float* gw2, hipStream_t stream) {
  const int64_t blocks = (a.n_chunks + Cfg<OUT>::BWD_WAVES - 1) / Cfg<OUT>::BWD_WAVES;
  hipLaunchKernelGGL((edge_conv_bwd_kernel<OUT, BY_SRC>), dim3((unsigned)blocks), dim3(Cfg<OUT>::BWD_WAVES * 64), 0, stream, a);
  PG_CHECK_LAUNCH("edge_conv_bwd_kernel");
  hipLaunchKernelGGL(edge_conv_bwd_combine_kernel<OUT>, dim3((unsigned)a.n_chunks), dim3(256), 0, stream, a);
  PG_CHECK_LAUNCH("edge_conv_bwd_combine_kernel");
  if (!BY_SRC) {
    hipLaunchKernelGGL(edge_conv_slab_sum_kernel, dim3((OUT * OUT + kWave - 1) / kWave), dim3(kSumThreads), 0, stream,
                       a.slabs, (int)blocks, OUT * OUT, gw2);
    PG_CHECK_LAUNCH("edge_conv_slab_sum_kernel");
  }
  return 0;
}

}  // namespace
}  // namespace pangnn

using namespace pangnn;

extern "C" int64_t pangnn_edge_conv_scratch_bytes(int64_t num_edges, int32_t out_dim, int backward) {
  if (num_edges < 0 || (out_dim != 64 && out_dim != 128)) return 0;
  return scratch_layout(num_edges, out_dim, backward != 0).total;
}

extern "C" int pangnn_edge_conv_fwd_f32(const float* u, int64_t ldu, const float* v, int64_t ldv, int64_t num_nodes,
                                        const float* w2, const float* b2, int32_t out_dim, const int64_t* rowptr,
                                        const int32_t* col, const int32_t* perm, const int64_t* edge_index, int64_t ld,
                                        int64_t num_edges, float* out, int32_t* arg, int64_t ldo, void* scratch,
                                        int64_t scratch_bytes, pangnn_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  PG_CHECK_ARG(out_dim == 64 || out_dim == 128, PANGNN_E_BADARG, "pangnn_edge_conv_fwd_f32: out must be 64 or 128, got %d",
               out_dim);
  PG_CHECK_ARG(num_nodes >= 0 && num_edges >= 0 && ld >= num_edges && ldu >= out_dim && ldv >= out_dim && ldo >= out_dim,
               PANGNN_E_BADARG, "pangnn_edge_conv_fwd_f32: bad size");
  PG_CHECK_ARG(num_nodes < (1ll << 31) && num_edges < (1ll << 31), PANGNN_E_TOOLARGE,
               "pangnn_edge_conv_fwd_f32: node / edge ids are int32");
  if (num_nodes == 0) return 0;
  PG_CHECK_ARG(rowptr && out && arg && u && v && w2 && b2, PANGNN_E_BADARG, "pangnn_edge_conv_fwd_f32: null pointer");
  PG_CHECK_ARG(num_edges == 0 || (col && perm && edge_index), PANGNN_E_BADARG, "pangnn_edge_conv_fwd_f32: null pointer");
  PG_CHECK_ARG(aligned16(u) && aligned16(v) && aligned16(w2) && ldu % 4 == 0 && ldv % 4 == 0, PANGNN_E_ALIGN,
               "pangnn_edge_conv_fwd_f32: u, v, w2 and the row strides must be 16-byte aligned");
  const Scratch s = scratch_layout(num_edges, out_dim, false);
  PG_CHECK_ARG(num_edges == 0 || (scratch && scratch_bytes >= s.total), PANGNN_E_WORKSPACE,
               "pangnn_edge_conv_fwd_f32: workspace of %lld bytes, %lld needed", (long long)scratch_bytes, (long long)s.total);
  // rows without in-edges: 0 / -1 (every other row is written by exactly one wave or combine block)
  if (ldo == out_dim) {
    (void)hipMemsetAsync(out, 0, (size_t)num_nodes * out_dim * 4, stream);
    (void)hipMemsetAsync(arg, 0xff, (size_t)num_nodes * out_dim * 4, stream);
  } else {
    (void)hipMemset2DAsync(out, (size_t)ldo * 4, 0, (size_t)out_dim * 4, (size_t)num_nodes, stream);
    (void)hipMemset2DAsync(arg, (size_t)ldo * 4, 0xff, (size_t)out_dim * 4, (size_t)num_nodes, stream);
  }
  PG_CHECK_LAUNCH("pangnn_edge_conv_fwd_f32(memset)");
  if (num_edges == 0) return 0;
  const ChunkPlan cp = plan_chunks(num_edges, kFwdChunks);
  char* ws = static_cast<char*>(scratch);
  FwdParams a;
  a.u = u; a.v = v; a.ldu = ldu; a.ldv = ldv; a.w2 = w2; a.b2 = b2;
  a.rowptr = rowptr; a.col = col; a.perm = perm; a.ei = edge_index; a.ld = ld; a.E = num_edges;
  a.out = out; a.arg = arg; a.ldo = ldo;
  a.chunk_entries = cp.entries; a.n_chunks = cp.n_chunks;
  a.head_row = reinterpret_cast<int32_t*>(ws + s.head_row);
  a.head_val = reinterpret_cast<float*>(ws + s.head_val);
  a.head_arg = reinterpret_cast<int32_t*>(ws + s.head_arg);
  a.tail_val = reinterpret_cast<float*>(ws + s.tail_val);
  a.tail_arg = reinterpret_cast<int32_t*>(ws + s.tail_arg);
  return out_dim == 64 ? launch_fwd<64>(a, stream) : launch_fwd<128>(a, stream);
}

extern "C" int pangnn_edge_conv_bwd_f32(const float* g, int64_t ldg, const int32_t* arg, const float* u, int64_t ldu,
                                        const float* v, int64_t ldv, int64_t num_nodes, const float* w2, int32_t out_dim,
                                        const int64_t* dst_rowptr, const int32_t* dst_col, const int32_t* dst_perm,
                                        const int64_t* src_rowptr, const int32_t* src_col, const int32_t* src_perm,
                                        const int64_t* edge_index, int64_t ld, int64_t num_edges, float* gu, float* gv,
                                        int64_t ldgrad, float* gw2, void* scratch, int64_t scratch_bytes,
                                        pangnn_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  PG_CHECK_ARG(out_dim == 64 || out_dim == 128, PANGNN_E_BADARG, "pangnn_edge_conv_bwd_f32: out must be 64 or 128, got %d",
               out_dim);
  PG_CHECK_ARG(num_nodes >= 0 && num_edges >= 0 && ld >= num_edges && ldu >= out_dim && ldv >= out_dim && ldg >= out_dim &&
                   ldgrad >= out_dim, PANGNN_E_BADARG, "pangnn_edge_conv_bwd_f32: bad size");
  PG_CHECK_ARG(num_nodes < (1ll << 31) && num_edges < (1ll << 31), PANGNN_E_TOOLARGE,
               "pangnn_edge_conv_bwd_f32: node / edge ids are int32");
  PG_CHECK_ARG(gw2, PANGNN_E_BADARG, "pangnn_edge_conv_bwd_f32: null pointer");
  PG_CHECK_ARG(num_nodes == 0 || (g && arg && u && v && w2 && gu && gv && dst_rowptr && src_rowptr), PANGNN_E_BADARG,
               "pangnn_edge_conv_bwd_f32: null pointer");
  PG_CHECK_ARG(num_edges == 0 || (dst_col && dst_perm && src_col && src_perm && edge_index), PANGNN_E_BADARG,
               "pangnn_edge_conv_bwd_f32: null pointer");
  PG_CHECK_ARG(aligned16(u) && aligned16(v) && aligned16(g) && aligned16(arg) && aligned16(w2) && ldu % 4 == 0 &&
                   ldv % 4 == 0 && ldg % 4 == 0, PANGNN_E_ALIGN,
               "pangnn_edge_conv_bwd_f32: g, arg, u, v, w2 and the row strides must be 16-byte aligned");
  const Scratch s = scratch_layout(num_edges, out_dim, true);
  PG_CHECK_ARG(num_edges == 0 || (scratch && scratch_bytes >= s.total), PANGNN_E_WORKSPACE,
               "pangnn_edge_conv_bwd_f32: workspace of %lld bytes, %lld needed", (long long)scratch_bytes, (long long)s.total);
  (void)hipMemsetAsync(gw2, 0, (size_t)out_dim * out_dim * 4, stream);
  if (num_nodes > 0) {
    // rows without entries get no sum
    (void)hipMemset2DAsync(gu, (size_t)ldgrad * 4, 0, (size_t)out_dim * 4, (size_t)num_nodes, stream);
    (void)hipMemset2DAsync(gv, (size_t)ldgrad * 4, 0, (size_t)out_dim * 4, (size_t)num_nodes, stream);
  }
  PG_CHECK_LAUNCH("pangnn_edge_conv_bwd_f32(memset)");
  if (num_edges == 0 || num_nodes == 0) return 0;
  const ChunkPlan cp = plan_chunks(num_edges, kBwdChunks);
  char* ws = static_cast<char*>(scratch);
  uint8_t* win = reinterpret_cast<uint8_t*>(ws + s.win);
  (void)hipMemsetAsync(win, 0, (size_t)num_edges, stream);
  const int64_t total = num_nodes * out_dim;
  const int64_t mark_blocks = (total + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(edge_conv_mark_winners_kernel, dim3((unsigned)(mark_blocks < 65536 ? mark_blocks : 65536)), dim3(kBlock),
                     0, stream, arg, total, win);
  PG_CHECK_LAUNCH("edge_conv_mark_winners_kernel");
  BwdParams a;
  a.u = u; a.v = v; a.g = g; a.ldu = ldu; a.ldv = ldv; a.ldg = ldg; a.arg = arg; a.w2 = w2;
  a.ei = edge_index; a.ld = ld; a.E = num_edges; a.win = win; a.ldo = ldgrad;
  a.chunk_entries = cp.entries; a.n_chunks = cp.n_chunks;
  a.head_row = reinterpret_cast<int32_t*>(ws + s.head_row);
  a.head_val = reinterpret_cast<float*>(ws + s.head_val);
  a.tail_val = reinterpret_cast<float*>(ws + s.tail_val);
  a.slabs = reinterpret_cast<float*>(ws + s.slabs);
  a.rowptr = dst_rowptr; a.other = dst_col; a.perm = dst_perm; a.grad = gu;
  int rc = out_dim == 64 ? launch_bwd_pass<64, false>(a, gw2, stream) : launch_bwd_pass<128, false>(a, gw2, stream);
  if (rc != 0) return rc;
  a.rowptr = src_rowptr; a.other = src_col; a.perm = src_perm; a.grad = gv;
  return out_dim == 64 ? launch_bwd_pass<64, true>(a, nullptr, stream) : launch_bwd_pass<128, true>(a, nullptr, stream);
}
