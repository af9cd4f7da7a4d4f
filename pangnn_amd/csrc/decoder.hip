// Fused link decoder for node_dim D in {32, 64, 128} (src/setup.py:38, src/gnn.py:110-116,171-177), fp32, gfx950.
//
//   h1[e]   = relu((P[src_e] + Q[dst_e]) (+ w_e * c))        P = z W1a^T, Q = z W1b^T + b1  (node level)
//   h2[e]   = relu(W2 h1[e] + b2)
//   logit_e = w3 . h2[e] + b3
//
// One wavefront owns a tile of 32 consecutive edges (caller's edge order, so logits are written coalesced and no
// permutation is needed).  The 32 x D h1 tile is gathered with row-contiguous 16-byte loads (D / 4 lanes per node row)
// into a padded LDS image and multiplied with W2 (LDS resident, loaded once per workgroup) on the f32 MFMA
// (v_mfma_f32_32x32x2_f32: exact, k-ordered fp32 FMA chains, so results match an fp32 reference to rounding).  The product
// is oriented C[j][e] = sum_k W2[j][k] h1[e][k] (A = W2, B = h1^T): the edge index stays on the lane, so bias + relu + the
// dot with w3 are in-lane and one xor-32 shuffle finishes a logit.
//
// Backward recomputes the forward per tile and chains two more MFMA products without leaving the CU: gW2 += G h1 with
// G = dL/dh2pre rebuilt from the h2 rows staged through LDS (the accumulator layout has the edge on the lane, this product
// wants the output j there), and gH1 = G^T W2 with G in the accumulator registers of the first product, used directly as
// the A operand (written out as dL/dh1pre [E, D]).  Parameter gradients are accumulated in registers across all tiles of
// a wave, reduced over the workgroup's waves in a fixed order and written as one partial slab per workgroup; a second
// tiny kernel sums the slabs in index order => bitwise reproducible, no float atomics.  One forward kernel, one backward
// kernel <D, FUSED_LOSS, RUNSUM, LIVE> (LIVE: the fused loss of a padded batch, real-edge count read on the device), one
// reduce kernel.
//
// What the width changes:
//   D = 32   8 waves per workgroup; everything is one 32 x 32 block.
//   D = 64   8 waves per workgroup, 2 x 2 blocks; the strict-fp32 mode (precision 0) of the default width, whose
//            default-mode kernels are decoder16.hip.
//   D = 128  the padded W2 image alone is 128 x 132 x 4 B = 66 KiB, so a workgroup has 4 waves (one per SIMD), each with a
//            32 x 132 h1 tile.  dL/dW2 is 16 blocks of 32 x 32: 256 accumulator registers per lane if one wave held it
//            all, every AGPR there is, so the backward's four waves own four blocks each and exchange the h2 slices (see
//            the kernel).
// The launch grid is a function of the edge count alone (never of the device), so a result does not depend on it.
#include "common.h"

#include <type_traits>

namespace pangnn {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TE = 32;          // edges per wave tile
constexpr int GS = 33;          // row stride of the staged h2 slice (floats): conflict-free column reads
constexpr int kMaxGrid = 256;   // workgroups at most (one per CU of an MI355X); fixed, so slabs and sums do not follow the device
constexpr int SLAB16 = 64 * 64 + 64 + 64 + 64 + 16;   // slab stride of decoder16.hip's training kernel (same layout, padded)

template <int D>
struct Shape {
  static_assert(D == 32 || D == 64 || D == 128, "decoder.hip is built for node_dim 32, 64 and 128");
  static constexpr int NB = D / 32;                 // 32-wide blocks per dimension
  // padded row stride of the W2 and h1 images (floats): 16-byte aligned rows, and RS mod 64 in {36, 4} = 4 * odd, so a
  // ds_read_b128 down a column of 16 rows touches 16 distinct groups of four banks; row-wise b32 / b128 accesses are
  // contiguous, and every address is `lane base + compile-time offset` (an XOR swizzle costs a VGPR per address)
  static constexpr int RS = D + 4;
  static constexpr int WAVES = D == 128 ? 4 : 8;
  static constexpr bool COOP = D == 128;            // the backward's waves share dL/dW2 out among them (see the kernel)
  static constexpr int WGRAD_UNROLL = D == 32 ? 16 : 4;   // D >= 64: a loop of four rounds, for the registers' sake
  static constexpr int LPR = D / 4;                 // lanes that cover one node row with 16-byte pieces
  static constexpr int RPI = 64 / LPR;              // rows per wave-wide load instruction
  static constexpr int NI = TE / RPI;               // load instructions per table and tile
  static constexpr int SLAB = D * D + 3 * D + 2;    // gW2 | gb2 | gw3 | gcvec | gb3 | loss
  static constexpr int FWD_LDS = D * RS + 3 * D + WAVES * TE * RS;
  static constexpr int PER_WAVE = TE * RS + 32 * GS + 64;   // h1 tile | h2 slice | w_e | g_e
  static constexpr int BWD_LDS = D * RS + 3 * D + WAVES * PER_WAVE;
  static_assert(BWD_LDS * 4 <= 160 * 1024 && FWD_LDS * 4 <= 160 * 1024, "LDS budget of one CU");
  static_assert(SLAB <= WAVES * PER_WAVE, "the slab is reduced in the tile area");
};

struct DecParams {
  const float* p; const float* q; uint32_t ldp4; uint32_t ldq4;   // row strides in float4 units
  const int64_t* ei; int64_t ld; int64_t E;
  const float* extra; const float* cvec;
  const float* w2; const float* b2; const float* w3; const float* b3;
};

// ---- stage W2 / b2 / w3 (/ cvec) into LDS, once per workgroup
template <int D>
__device__ __forceinline__ void stage_weights(const DecParams& a, float* Wl, float* b2l, float* w3l, float* cvl) {
  using S = Shape<D>;
  for (int i = threadIdx.x; i < D * (D / 4); i += S::WAVES * 64) {
    const int j = i / (D / 4), k4 = i % (D / 4);
    const float4 v = reinterpret_cast<const float4*>(a.w2)[i];
    *reinterpret_cast<float4*>(Wl + j * S::RS + 4 * k4) = v;
  }
  for (int i = threadIdx.x; i < D; i += S::WAVES * 64) {
    b2l[i] = a.b2[i];
    w3l[i] = a.w3[i];
    cvl[i] = a.cvec ? a.cvec[i] : 0.f;
  }
}

// relu as torch computes it: a NaN stays a NaN (fmaxf / fmed3f would return 0 and hide an overflow from a GradScaler).
// Compiler-visible (not inline asm: an asm statement that defines a VGPR is invisible to the MFMA hazard recognizer and may
// overwrite a source register of an in-flight MFMA — see decoder16.hip)
__device__ __forceinline__ float relu1(float x) { return x < 0.f ? 0.f : x; }

// 16-byte row piece at `table + byte_off`: uniform base pointer + 32-bit per-lane byte offset (node tables are < 4 GiB,
// checked by the host wrapper) — `global_load_dwordx4 v, v_off, s[base]`, no 64-bit vector address
__device__ __forceinline__ float4 ld_row16(const float* table, uint32_t byte_off) {
  return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(table) + byte_off);
}

// ---- gather the tile's 32 h1 rows into the wave's LDS image.  Returns w_e / the node id per lane (lanes 0-31: source of
// edge `lane`, 32-63: target of edge `lane - 32`).  FULL: all 32 edges exist, no bounds predicate on the id loads.
template <int D, bool FULL>
__device__ __forceinline__ void gather_tile(const DecParams& a, int64_t ebase, int lane, float* Ht, const float* cvl,
                                            float& w_e, int& id) {
  using S = Shape<D>;
  const int64_t e = ebase + (lane & 31);
  id = 0;
  w_e = 0.f;
  if (FULL || e < a.E) {
    id = (int)a.ei[(int64_t)(lane >> 5) * a.ld + e];
    if (a.extra && lane < 32) w_e = a.extra[e];
  }
  const int c4 = lane % S::LPR, r4 = lane / S::LPR;
  // byte offset of this lane's node row in its table (P for the source half, Q for the target half): one multiply per
  // lane and tile; the row gathers below shuffle the finished offset instead of the id
  const uint32_t row_off = (uint32_t)id * ((lane >> 5) ? a.ldq4 : a.ldp4) * 16u;
  const uint32_t col_off = 16u * c4;
  const bool has_extra = a.extra != nullptr;             // uniform: the w_e * c term only exists with skip connections
  float4 cv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (has_extra) cv = reinterpret_cast<const float4*>(cvl)[c4];
  // a real loop at D = 128 (four rounds of eight loads): unrolled, the scheduler issues all 32 loads first and the kernel
  // runs out of registers
#pragma unroll 1
  for (int g = 0; g < S::NI / 4; ++g) {
    float4 pv[4], qv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = S::RPI * (4 * g + i) + r4;
      pv[i] = ld_row16(a.p, (uint32_t)__shfl((int)row_off, row) + col_off);
      qv[i] = ld_row16(a.q, (uint32_t)__shfl((int)row_off, 32 + row) + col_off);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {                         // (p + q) + w c, in that association
      pv[i].x += qv[i].x; pv[i].y += qv[i].y; pv[i].z += qv[i].z; pv[i].w += qv[i].w;
    }
    if (has_extra) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float wv = __shfl(w_e, S::RPI * (4 * g + i) + r4);
        pv[i].x = fmaf(wv, cv.x, pv[i].x);
        pv[i].y = fmaf(wv, cv.y, pv[i].y);
        pv[i].z = fmaf(wv, cv.z, pv[i].z);
        pv[i].w = fmaf(wv, cv.w, pv[i].w);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = S::RPI * (4 * g + i) + r4;
      float4 h;
      h.x = relu1(pv[i].x);
      h.y = relu1(pv[i].y);
      h.z = relu1(pv[i].z);
      h.w = relu1(pv[i].w);
      // a row past the end of the list gathered node 0, which no edge may reference: its values (a NaN among them) must
      // not reach the weight-gradient products, whose zero dL/dlogit would turn them into 0 * NaN
      if (!FULL && ebase + row >= a.E) h = make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(Ht + row * S::RS + 4 * c4) = h;
    }
  }
}

// ---- C[j][e] = sum_k W2[j][k] h1[e][k]; lane (e = lane&31, hh = lane>>5) gets rows acc_row(i,hh) + 32b in acc[b][i].
// Half hh of the wave feeds k = (D/2) hh + 0 .. D/2 - 1, one k of each half per instruction.
template <int D>
__device__ __forceinline__ void gemm1(const float* Wl, const float* Ht, int lane, f32x16 (&acc)[Shape<D>::NB]) {
  using S = Shape<D>;
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int b = 0; b < S::NB; ++b)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[b][i] = 0.f;
#pragma unroll 4
  for (int i = 0; i < D / 8; ++i) {                        // D = 128: four rounds of four steps, for the registers' sake
    const int k4 = (D / 8) * h + i;
    const float4 bf = *reinterpret_cast<const float4*>(Ht + r * S::RS + 4 * k4);
    float4 af[S::NB];
#pragma unroll
    for (int b = 0; b < S::NB; ++b) af[b] = *reinterpret_cast<const float4*>(Wl + (r + 32 * b) * S::RS + 4 * k4);
#pragma unroll
    for (int b = 0; b < S::NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[b].x, bf.x, acc[b], 0, 0, 0);
#pragma unroll
    for (int b = 0; b < S::NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[b].y, bf.y, acc[b], 0, 0, 0);
#pragma unroll
    for (int b = 0; b < S::NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[b].z, bf.z, acc[b], 0, 0, 0);
#pragma unroll
    for (int b = 0; b < S::NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[b].w, bf.w, acc[b], 0, 0, 0);
  }
}

// ---- h2 = relu(C + b2) in place in the accumulators; returns this half's part of w3 . h2 (same order of additions in the
// forward and in the training kernel, so their logits are the same bits)
template <int D>
__device__ __forceinline__ float layer2_epilogue(const float* b2l, const float* w3l, int hh, f32x16 (&acc)[Shape<D>::NB]) {
  float part = 0.f;
#pragma unroll
  for (int b = 0; b < Shape<D>::NB; ++b)
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      const int j0 = 32 * b + 8 * qd + 4 * hh;
      const float4 bb = *reinterpret_cast<const float4*>(b2l + j0);
      const float4 ww = *reinterpret_cast<const float4*>(w3l + j0);
      const float bbv[4] = {bb.x, bb.y, bb.z, bb.w};
      const float wwv[4] = {ww.x, ww.y, ww.z, ww.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float h2 = relu1(acc[b][4 * qd + c] + bbv[c]);
        part = fmaf(h2, wwv[c], part);
        acc[b][4 * qd + c] = h2;
      }
    }
  return part;
}

// ---- software-pipelined gather of the forward kernel: edge ids two tiles ahead, node rows one tile ahead, so a wave never
// waits on HBM between two MFMA phases (the rows of tile t+1 land while tile t is in the matrix pipe)
struct TileIds { int id; float w_e; uint32_t row_off; };     // row_off: byte offset of the lane's node row in P / Q
template <int D> struct TileRows { float4 pv[Shape<D>::NI]; float4 qv[Shape<D>::NI]; float wv[Shape<D>::NI]; };

__device__ __forceinline__ TileIds load_ids(const DecParams& a, int64_t tile, int64_t n_tiles, int lane) {
  TileIds t;
  t.id = 0;
  t.w_e = 0.f;
  const int64_t e = tile * TE + (lane & 31);
  if (tile < n_tiles && e < a.E) {
    t.id = (int)a.ei[(int64_t)(lane >> 5) * a.ld + e];   // lanes 0-31: source, 32-63: target
    if (a.extra && lane < 32) t.w_e = a.extra[e];
  }
  t.row_off = (uint32_t)t.id * ((lane >> 5) ? a.ldq4 : a.ldp4) * 16u;
  return t;
}

template <int D>
__device__ __forceinline__ void issue_rows(const DecParams& a, const TileIds& t, int lane, TileRows<D>& rw) {
  using S = Shape<D>;
  const int r4 = lane / S::LPR;
  const uint32_t col_off = 16u * (lane % S::LPR);
  const bool has_extra = a.extra != nullptr;
#pragma unroll
  for (int i = 0; i < S::NI; ++i) {
    const int row = S::RPI * i + r4;
    rw.wv[i] = has_extra ? __shfl(t.w_e, row) : 0.f;
    rw.pv[i] = ld_row16(a.p, (uint32_t)__shfl((int)t.row_off, row) + col_off);
    rw.qv[i] = ld_row16(a.q, (uint32_t)__shfl((int)t.row_off, 32 + row) + col_off);
  }
}

template <int D>
__device__ __forceinline__ void commit_rows(const DecParams& a, const TileRows<D>& rw, int lane, const float* cvl,
                                            float* Ht) {
  using S = Shape<D>;
  const int c4 = lane % S::LPR, r4 = lane / S::LPR;
  const bool has_extra = a.extra != nullptr;
  float4 cv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (has_extra) cv = reinterpret_cast<const float4*>(cvl)[c4];
#pragma unroll
  for (int i = 0; i < S::NI; ++i) {
    const int row = S::RPI * i + r4;
    float4 h;
    h.x = rw.pv[i].x + rw.qv[i].x;
    h.y = rw.pv[i].y + rw.qv[i].y;
    h.z = rw.pv[i].z + rw.qv[i].z;
    h.w = rw.pv[i].w + rw.qv[i].w;
    if (has_extra) {
      h.x = fmaf(rw.wv[i], cv.x, h.x);
      h.y = fmaf(rw.wv[i], cv.y, h.y);
      h.z = fmaf(rw.wv[i], cv.z, h.z);
      h.w = fmaf(rw.wv[i], cv.w, h.w);
    }
    h.x = relu1(h.x); h.y = relu1(h.y); h.z = relu1(h.z); h.w = relu1(h.w);
    *reinterpret_cast<float4*>(Ht + row * S::RS + 4 * c4) = h;
  }
}

template <int D>
__global__ __launch_bounds__(Shape<D>::WAVES * 64) void decoder_fwd_kernel(DecParams a, float* __restrict__ logits,
                                                                          int64_t n_tiles) {
  using S = Shape<D>;
  __shared__ __attribute__((aligned(16))) float lds[S::FWD_LDS];
  float* Wl = lds;
  float* b2l = lds + D * S::RS;
  float* w3l = b2l + D;
  float* cvl = w3l + D;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;   // SGPR: tile index and its addresses stay scalar
  float* Ht = cvl + D + wave * (TE * S::RS);
  stage_weights<D>(a, Wl, b2l, w3l, cvl);
  __syncthreads();
  const float b3 = a.b3[0];
  const int hh = lane >> 5;
  const int64_t stride = (int64_t)gridDim.x * S::WAVES;
  int64_t tile = (int64_t)blockIdx.x * S::WAVES + wave;
  TileIds cur = load_ids(a, tile, n_tiles, lane);
  TileIds nxt = load_ids(a, tile + stride, n_tiles, lane);
  TileRows<D> rw;
  issue_rows<D>(a, cur, lane, rw);
  for (; tile < n_tiles; tile += stride) {
    const int64_t ebase = tile * TE;
    commit_rows<D>(a, rw, lane, cvl, Ht);                    // waits for this tile's rows only
    const TileIds nn = load_ids(a, tile + 2 * stride, n_tiles, lane);
    issue_rows<D>(a, nxt, lane, rw);                         // next tile's rows fly during the MFMAs
    nxt = nn;
    wave_lds_sync();
    f32x16 acc[S::NB];
    gemm1<D>(Wl, Ht, lane, acc);
    float part = layer2_epilogue<D>(b2l, w3l, hh, acc);
    part += __shfl_xor(part, 32);
    if (lane < 32 && ebase + lane < a.E) logits[ebase + lane] = part + b3;
    wave_lds_sync();   // the next commit overwrites Ht
  }
}

// FUSED_LOSS: the upstream gradient is not read but produced in place — the tile's logits come out of the first product
// anyway, so BCEWithLogits(pos_weight) and its derivative are evaluated right there (pangnn.py:200-207 in one pass): a
// training step then runs this kernel only, not forward + loss + backward.
struct LossParams {
  const float* y; const float* pos_weight; float inv_denom; float* logits;
};

// RUNSUM: when the caller's edge order is sorted by source (every edge list pangnn_amd/construct.py emits is), the rows of
// dL/dh1 that belong to one source are consecutive, so their sum — dL/dP[source] — is taken right here per (tile, source)
// run and written as one "part" row of D floats; a short contiguous segment sum over the parts replaces a pass over
// dL/dh1.  part_off[tile] = index of the tile's first part (EdgeStructure._plan_of_sorted_keys with chunk_tiles = 1); the
// number of parts a tile writes is fixed by the edge list, so the layout is deterministic.
struct RunSumParams {
  float* part; const int32_t* part_off;
};

// LIVE (with FUSED_LOSS): the list is a fixed-shape padded batch whose first m = min(max(live_edges[0], 0), E) edges are real
// (include/pangnn_hip.h, live_edges; one uniform load per workgroup, outside the tile loop).  An edge >= m still exists — its
// gather and its logit store are in bounds — but it gets dL/dlogit = +0 and no loss term, and the mean is over max(m, 1)
// edges (lp.inv_denom is not read).  Everything behind dL/dlogit is a product with it: the edge's dL/dh1 row is written as
// zeros (the segment sums and the run parts read every row), and the parameter slabs, gcvec and the run parts receive zeros
// from it (finite P | Q rows and weights).  The instances without LIVE never read the count and keep their FULL tile body
// free of selects.
// `given`: the one per-edge input that does not come with the fused loss — dL/dlogits [E] (float) without FUSED_LOSS,
// live_edges (int64) with LIVE, unused otherwise.  One slot for both (a call has one or the other) keeps the argument block
// of the instances without LIVE what it was before LIVE existed, and their code with it: the same instruction streams at
// D = 64 and 128; at D = 32 the same instructions to within one, in another register allocation.
template <int D, bool FUSED_LOSS, bool RUNSUM, bool LIVE = false>
__global__ __launch_bounds__(Shape<D>::WAVES * 64) void decoder_bwd_kernel(
    DecParams a, const void* __restrict__ given, LossParams lp, RunSumParams rs, float* __restrict__ g_h1,
    float* __restrict__ slabs, int64_t n_tiles) {
  static_assert(FUSED_LOSS || !LIVE, "live_edges belongs to the fused loss");
  const float* __restrict__ g_logits = static_cast<const float*>(given);
  using S = Shape<D>;
  constexpr int NB = S::NB, RS = S::RS, WAVES = S::WAVES;
  // D = 128: dL/dW2 is shared out over the workgroup's four waves, wave w owning the 32 rows j of block w (4 blocks of
  // 32 x 32 = 64 accumulator registers; all 16 blocks per wave would take every accumulator register there is and leave
  // none for the two other products).  The waves then walk their tiles in step, one round of WAVES tiles at a time.
  constexpr bool COOP = S::COOP;
  constexpr int NJ = COOP ? 1 : NB;      // blocks of 32 rows of dL/dW2 a wave accumulates
  constexpr int WGRAD_UNROLL = S::WGRAD_UNROLL;
  __shared__ __attribute__((aligned(16))) float lds[S::BWD_LDS];
  float* Wl = lds;
  float* b2l = lds + D * RS;
  float* w3l = b2l + D;
  float* cvl = w3l + D;
  float* tiles = cvl + D;         // WAVES x (h1 tile | h2 slice | w_e | g_e)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  float* Ht = tiles + wave * S::PER_WAVE;
  float* Gt = Ht + TE * RS;       // h2[j][e] of one block of 32 outputs j
  float* wl = Gt + 32 * GS;
  float* gl = wl + 32;
  stage_weights<D>(a, Wl, b2l, w3l, cvl);
  __syncthreads();
  const int hh = lane >> 5, r = lane & 31;

  f32x16 acc3[NJ][NB];   // gW2[j = acc_row(i,hh) + 32 (COOP ? wave : bj)][k = r + 32bk]
#pragma unroll
  for (int bj = 0; bj < NJ; ++bj)
#pragma unroll
    for (int bk = 0; bk < NB; ++bk)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc3[bj][bk][i] = 0.f;
  float w3j[NJ], gw3p[NJ], gb2p[NJ], gcv[NB];
#pragma unroll
  for (int b = 0; b < NJ; ++b) {
    w3j[b] = w3l[r + 32 * (COOP ? wave : b)];
    gw3p[b] = 0.f;   // lane (j = r + 32b, hh): partial of gw3[j] over the edges e = hh mod 2
    gb2p[b] = 0.f;   // same lanes: partial of gb2[j]
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) gcv[b] = 0.f;    // lane (k = r + 32b, hh): partial of gcvec[k]
  float gb3p = 0.f;
  float lossp = 0.f;            // FUSED_LOSS: partial of the (already 1/denom-scaled) loss
  const float b3v = a.b3[0];
  const float pw = (FUSED_LOSS && lp.pos_weight) ? lp.pos_weight[0] : 1.f;
  int64_t m_live = a.E;         // LIVE: the number of real edges
  float inv_denom = lp.inv_denom;
  if constexpr (LIVE) {
    const int64_t lv = static_cast<const int64_t*>(given)[0];
    m_live = lv < 0 ? 0 : lv > a.E ? a.E : lv;
    inv_denom = 1.0f / (float)(m_live > 1 ? m_live : 1);   // the host's 1.0f / (float)denom of the list cut to m edges
  }

  // what a tile carries from its front half (forward recomputation) to its back half (dL/dh1)
  f32x16 acc[NB];      // h2[j][e], lane (e = r, hh), rows acc_row(i,hh) + 32b
  float g_e = 0.f;
  int id = 0;

  // gW2[j][k] += sum_e G[j][e] h1[e][k] for the 32 rows j of one block, G rebuilt from the block's h2 rows in `Gs` and the
  // tile's dL/dlogit in `gls`; h1 from the tile image `Hs`
  auto wgrad_block = [&](const float* Hs, const float* Gs, const float* gls, int bj) __attribute__((always_inline)) {
#pragma unroll WGRAD_UNROLL
    for (int s = 0; s < 16; ++s) {
      const int e = 2 * s + hh;
      const float ge = gls[e];
      const float x = Gs[r * GS + e];                      // h2[j = r + 32 block][e]
      const float av = x <= 0.f ? 0.f : ge * w3j[bj];      // not `x > 0 ?`: a NaN h2 keeps its column on
      gw3p[bj] = fmaf(ge, x, gw3p[bj]);
      gb2p[bj] += av;
#pragma unroll
      for (int bk = 0; bk < NB; ++bk) {
        const float hv = Hs[e * RS + r + 32 * bk];
        acc3[bj][bk] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, hv, acc3[bj][bk], 0, 0, 0);
      }
    }
  };

  // Front half of a tile: gather, first product, logits / loss / dL/dlogit.  FULL (every tile but the last of the edge
  // list): all 32 edges exist, so the bounds predicates on loads / stores and the `live` selects fold away; the
  // instruction count of a tile is what the kernel's time follows (f32 MFMA and vector instructions share the SIMD's
  // lanes), so the common case carries none.
  auto front = [&](const int64_t tile, auto full_c) __attribute__((always_inline)) {
    constexpr bool FULL = decltype(full_c)::value;
    const int64_t ebase = tile * TE;
    float w_e;
    gather_tile<D, FULL>(a, ebase, lane, Ht, cvl, w_e, id);
    g_e = 0.f;
    float y_e = 0.f;
    const bool live = FULL || ebase + r < a.E;
    const bool real = LIVE ? ebase + r < m_live : live;     // (m_live <= E: a real edge is in bounds)
    if (FUSED_LOSS) {
      if (live) y_e = lp.y[ebase + r];
      if (lane < 32) wl[lane] = w_e;
    } else {
      if (live) g_e = g_logits[ebase + r];
      if (lane < 32) { wl[lane] = w_e; gl[lane] = g_e; gb3p += g_e; }
    }
    wave_lds_sync();

    gemm1<D>(Wl, Ht, lane, acc);
    float part = layer2_epilogue<D>(b2l, w3l, hh, acc);     // acc = h2[j][e]

    if (FUSED_LOSS) {
      part += __shfl_xor(part, 32);                 // both halves of the wave now hold edge r's logit
      const float xv = part + b3v;
      const float lw = 1.f + (pw - 1.f) * y_e;
      const float t = expf(-fabsf(xv));             // in (0, 1]
      const float u = 1.f + t;
      float ru = __builtin_amdgcn_rcpf(u);
      ru = ru * (2.f - u * ru);                     // 1 / (1 + t), one Newton step on the hardware reciprocal
      const float sig_neg = xv >= 0.f ? t * ru : ru;                              // sigmoid(-x)
      g_e = real ? ((1.f - y_e) - lw * sig_neg) * inv_denom : 0.f;
      // softplus(-x) = log1p(t) + max(-x, 0);  log1p(t) = log(u) * t / (u - 1) with u = fl(1 + t) (exact u - 1),
      // = t when u == 1
      const float um1 = u - 1.f;
      float rm = __builtin_amdgcn_rcpf(um1);
      rm = rm * (2.f - um1 * rm);
      const float l1p = um1 == 0.f ? t : logf(u) * (t * rm);
      gl[r] = g_e;                                   // the two halves write the same value
      gb3p += g_e;                                   // per-half partials; lane 0's half is the one read out
      lossp += real ? ((1.f - y_e) * xv + lw * (l1p + fmaxf(-xv, 0.f))) * inv_denom : 0.f;   // select, not a branch
      if (hh == 0 && live) lp.logits[ebase + r] = xv;
    }
  };

  // Back half: the accumulators become G[j][e] = g_e * w3[j] * [h2 > 0], the A operand of gH1[e][k] = sum_j G[j][e] W2[j][k]
  // (B = W2 rows); mask by h1 > 0, write dL/dh1pre, accumulate gcvec, run sums.
  auto back = [&](const int64_t tile, auto full_c) __attribute__((always_inline)) {
    constexpr bool FULL = decltype(full_c)::value;
    const int64_t ebase = tile * TE;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        const float4 ww = *reinterpret_cast<const float4*>(w3l + 32 * b + 8 * qd + 4 * hh);
        const float wwv[4] = {ww.x, ww.y, ww.z, ww.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[b][4 * qd + c] = acc[b][4 * qd + c] <= 0.f ? 0.f : g_e * wwv[c];
      }
    // run sums: a part closes at the last edge of every source run of the tile
    unsigned m = 0u;
    int64_t pidx = 0;
    if (RUNSUM) {
      const int id_nxt = __shfl(id, (lane + 1) & 63);
      const bool ok = lane < 32 && (FULL || ebase + lane < a.E);
      const bool ok_nxt = lane < 31 && (FULL || ebase + lane + 1 < a.E);
      const unsigned long long mask = __ballot(ok && (!ok_nxt || id != id_nxt));
      m = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(mask & 0xffffffffull));
      pidx = rs.part_off[tile];
    }
    const bool one_run = (m & (m - 1u)) == 0u, two_runs = __builtin_popcount(m) == 2;   // uniform
    const int bnd = __builtin_ctz(m | 0x80000000u);        // two runs: last edge of the first
    float* gout = g_h1 + (ebase + 4 * hh) * D + r;
    const bool full = FULL || ebase + TE <= a.E;
    const bool has_extra = a.extra != nullptr;             // uniform; only with skip connections
    // one block of 32 columns k at a time (16 accumulator registers, not 16 NB)
#pragma unroll
    for (int bp = 0; bp < NB; ++bp) {
      f32x16 acc2;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc2[i] = 0.f;
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int i = 0; i < 16; ++i)
          acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[b][i], Wl[(32 * b + acc_row(i, hh)) * RS + r + 32 * bp], acc2, 0, 0, 0);
      // mask by h1 > 0, write dL/dh1pre (full tiles store through one lane base pointer + compile-time offsets: no
      // per-element bounds test or address arithmetic), accumulate gcvec
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int e = acc_row(i, hh);
        const float hval = Ht[e * RS + r + 32 * bp];
        const float v = hval <= 0.f ? 0.f : acc2[i];
        if (full || ebase + e < a.E) __builtin_nontemporal_store(v, &gout[acc_row(i, 0) * D + 32 * bp]);   // written once
        acc2[i] = v;
      }
      if (has_extra) {
#pragma unroll
        for (int i = 0; i < 16; ++i) gcv[bp] = fmaf(wl[acc_row(i, hh)], acc2[i], gcv[bp]);
      }
      if (RUNSUM) {
        if (one_run) {
          // one run covers the tile (the common case at degree >> 32): column sums straight from registers
          float s0 = 0.f;
#pragma unroll
          for (int i = 0; i < 16; ++i) s0 += acc2[i];
          s0 += __shfl_xor(s0, 32);
          if (hh == 0) rs.part[pidx * D + 32 * bp + r] = s0;
        } else if (two_runs) {
          // both column sums from the registers, rows selected by their position relative to the boundary
          float s0 = 0.f, s1 = 0.f;
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const bool first = acc_row(i, hh) <= bnd;
            s0 += first ? acc2[i] : 0.f;
            s1 += first ? 0.f : acc2[i];
          }
          s0 += __shfl_xor(s0, 32);
          s1 += __shfl_xor(s1, 32);
          if (hh == 0) {
            rs.part[pidx * D + 32 * bp + r] = s0;
            rs.part[(pidx + 1) * D + 32 * bp + r] = s1;
          }
        } else {
          // three or more runs: the block's dL/dh1 values replace the h1 values they were masked with (same lane, same
          // address; the other blocks' columns stay)
#pragma unroll
          for (int i = 0; i < 16; ++i) Ht[acc_row(i, hh) * RS + r + 32 * bp] = acc2[i];
        }
      }
      if (D == 128) __builtin_amdgcn_sched_barrier(0);     // one block's loads in flight at a time: registers
    }
    if (RUNSUM && !one_run && !two_runs) {
      // a lane owns the columns lane, lane + 64 (D = 32: lanes 0-31 one column each) and walks the 32 rows
      constexpr int CPL = (D + 63) / 64;
      wave_lds_sync();
      if (D >= 64 || lane < D) {
        float sum[CPL];
#pragma unroll
        for (int x = 0; x < CPL; ++x) sum[x] = 0.f;
#pragma unroll
        for (int e = 0; e < TE; ++e) {
#pragma unroll
          for (int x = 0; x < CPL; ++x) sum[x] += Ht[e * RS + lane + 64 * x];
          if ((m >> e) & 1u) {
#pragma unroll
            for (int x = 0; x < CPL; ++x) {
              rs.part[pidx * D + lane + 64 * x] = sum[x];
              sum[x] = 0.f;
            }
            ++pidx;
          }
        }
      }
    }
    wave_lds_sync();   // next tile overwrites Ht / Gt / wl / gl
  };

  const int64_t n_full = a.E / TE, stride = (int64_t)gridDim.x * WAVES;
  if constexpr (!COOP) {
    // a wave finishes a tile on its own: one block of 32 outputs j at a time, the block's h2 rows go through LDS (the
    // accumulator layout has the edge on the lane, the weight-gradient product wants j there)
    auto body = [&](const int64_t tile, auto full_c) __attribute__((always_inline)) {
      front(tile, full_c);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
#pragma unroll
        for (int i = 0; i < 16; ++i) Gt[acc_row(i, hh) * GS + r] = acc[b][i];
        wave_lds_sync();
        wgrad_block(Ht, Gt, gl, b);
        wave_lds_sync();   // the next block overwrites Gt
      }
      back(tile, full_c);
    };
    int64_t tile = (int64_t)blockIdx.x * WAVES + wave;
    for (; tile < n_full; tile += stride) body(tile, std::true_type{});
    if (tile < n_tiles) body(tile, std::false_type{});     // tile == n_full: the partial tile, one wave's turn
  } else {
    // Rounds of WAVES consecutive tiles, wave w taking tile base + w.  In step t of a round wave w stages the h2 rows of
    // block (w + t) mod WAVES of its tile, and the owner of that block, wave (w + t) mod WAVES, multiplies them with w's h1
    // tile.  Every wave of the workgroup passes every barrier, with or without a tile of its own; the barriers stand
    // outside the FULL / partial instances of the two halves.
    static_assert(!COOP || (NB == WAVES && (WAVES & (WAVES - 1)) == 0), "one block of dL/dW2 rows per wave");
    for (int64_t base = (int64_t)blockIdx.x * WAVES; base < n_tiles; base += stride) {
      const int64_t tile = base + wave;
      const bool have = tile < n_tiles;                     // tiles base .. base + n_have - 1 exist
      const int n_have = (int)(n_tiles - base < WAVES ? n_tiles - base : WAVES);
      if (have) {
        if (tile < n_full) front(tile, std::true_type{});
        else front(tile, std::false_type{});
      }
#pragma unroll 1
      for (int t = 0; t < WAVES; ++t) {
        if (have) {
          const int pb = (wave + t) & (WAVES - 1);          // uniform; selects, not a register index
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            float v = acc[0][i];
#pragma unroll
            for (int b = 1; b < NB; ++b) v = pb == b ? acc[b][i] : v;
            Gt[acc_row(i, hh) * GS + r] = v;
          }
        }
        __syncthreads();
        const int src = (wave - t) & (WAVES - 1);           // the wave whose tile this wave's block is staged from
        if (src < n_have) {
          const float* Hs = tiles + src * S::PER_WAVE;
          wgrad_block(Hs, Hs + TE * RS, Hs + TE * RS + 32 * GS + 32, 0);
        }
        __syncthreads();   // the next step overwrites the slices; after the last step the tiles are their waves' again
      }
      if (have) {
        if (tile < n_full) back(tile, std::true_type{});
        else back(tile, std::false_type{});
      }
    }
  }

  // ---- fold the per-lane partials, then reduce the workgroup's waves in wave order
#pragma unroll
  for (int b = 0; b < NJ; ++b) {
    gw3p[b] += __shfl_xor(gw3p[b], 32);
    gb2p[b] += __shfl_xor(gb2p[b], 32);
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) gcv[b] += __shfl_xor(gcv[b], 32);
#pragma unroll
  for (int off = 16; off >= 1; off >>= 1) {
    gb3p += __shfl_xor(gb3p, off);
    lossp += __shfl_xor(lossp, off);
  }

  __syncthreads();
  float* red = tiles;   // reuse the tile area: SLAB floats
  if constexpr (COOP) {   // the rows of gW2 / gb2 / gw3 of block `wave` are this wave's alone
#pragma unroll
    for (int bk = 0; bk < NB; ++bk)
#pragma unroll
      for (int i = 0; i < 16; ++i) red[(32 * wave + acc_row(i, hh)) * D + r + 32 * bk] = acc3[0][bk][i];
    if (hh == 0) {
      red[D * D + 32 * wave + r] = gb2p[0];
      red[D * D + D + 32 * wave + r] = gw3p[0];
    }
  }
  for (int w = 0; w < WAVES; ++w) {
    if (wave == w) {
      const bool first = (w == 0);
      if constexpr (!COOP) {
#pragma unroll
        for (int bj = 0; bj < NB; ++bj)
#pragma unroll
          for (int bk = 0; bk < NB; ++bk)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              const int idx = (32 * bj + acc_row(i, hh)) * D + r + 32 * bk;
              red[idx] = (first ? 0.f : red[idx]) + acc3[bj][bk][i];
            }
      }
      if (hh == 0) {
#pragma unroll
        for (int x = 0; x < NB; ++x) {
          const int o = D * D + r + 32 * x;
          if constexpr (!COOP) {
            red[o] = (first ? 0.f : red[o]) + gb2p[x];
            red[o + D] = (first ? 0.f : red[o + D]) + gw3p[x];
          }
          red[o + 2 * D] = (first ? 0.f : red[o + 2 * D]) + gcv[x];
        }
      }
      if (lane == 0) {
        const int o = D * D + 3 * D;
        red[o] = (first ? 0.f : red[o]) + gb3p;
        red[o + 1] = (first ? 0.f : red[o + 1]) + lossp;
      }
    }
    __syncthreads();
  }
  float* slab = slabs + (int64_t)blockIdx.x * S::SLAB;
  for (int i = threadIdx.x; i < S::SLAB; i += WAVES * 64) slab[i] = red[i];
}

// out[i] = sum over the workgroup slabs (`stride` floats apart, layout of Shape<d>::SLAB) in index order (fixed =>
// reproducible)
__global__ __launch_bounds__(kSumThreads) void decoder_reduce_kernel(const float* __restrict__ slabs, int n_slabs,
                                                                     int stride, int d, float* __restrict__ g_w2,
                                                                     float* __restrict__ g_b2, float* __restrict__ g_w3,
                                                                     float* __restrict__ g_cvec, float* __restrict__ g_b3,
                                                                     float* __restrict__ loss) {
  const int dd = d * d, len = dd + 3 * d + 2;
  const int i = blockIdx.x * kWave + (threadIdx.x & (kWave - 1));
  const float s = ordered_parts_sum(slabs, n_slabs, stride, i, len);
  if (threadIdx.x >= kWave || i >= len) return;
  if (i < dd) g_w2[i] = s;
  else if (i < dd + d) { if (g_b2) g_b2[i - dd] = s; }
  else if (i < dd + 2 * d) g_w3[i - dd - d] = s;
  else if (i < dd + 3 * d) { if (g_cvec) g_cvec[i - dd - 2 * d] = s; }
  else if (i == dd + 3 * d) g_b3[0] = s;
  else if (loss) loss[0] = s;
}

static int launch_reduce(const char* who, const float* slabs, int n_slabs, int stride, int d, float* g_w2, float* g_b2,
                         float* g_w3, float* g_cvec, float* g_b3, float* loss, hipStream_t s) {
  const int len = d * d + 3 * d + 2;
  hipLaunchKernelGGL(decoder_reduce_kernel, dim3((len + kWave - 1) / kWave), dim3(kSumThreads), 0, s, slabs, n_slabs,
                     stride, d, g_w2, g_b2, g_w3, g_cvec, g_b3, loss);
  PG_CHECK_LAUNCH(who);
  return 0;
}

// for decoder16.hip: the same finishing reduction over its slabs (same layout at d = 64, its own stride)
int launch_decoder_reduce(const float* slabs, int n_slabs, float* g_w2, float* g_b2, float* g_w3, float* g_cvec,
                          float* g_b3, float* loss, hipStream_t s) {
  return launch_reduce("decoder_reduce", slabs, n_slabs, SLAB16, 64, g_w2, g_b2, g_w3, g_cvec, g_b3, loss, s);
}

// decoder16.hip: inference form of the bf16 matrix-pipe mode
int launch_decoder_infer16(const float* p, int64_t ldp, const float* q, int64_t ldq, const int64_t* edge_index, int64_t ld,
                           int64_t num_edges, const float* extra, const float* cvec, const float* w2, const float* b2,
                           const float* w3, const float* b3, float* logits, hipStream_t s);

// ---- host side.  Two families of entry points share it: pangnn_decoder_mlp_* (node_dim 64, with a `precision` argument)
// and pangnn_decoder_nd_* (node_dim 32 and 128); `nd` says which one is asking.
struct DecArgs {   // the argument head every entry point takes
  const float* p; int64_t ldp; const float* q; int64_t ldq; int64_t num_nodes; const int64_t* ei; int64_t ld; int64_t E;
  const float* extra; const float* cvec; const float* w2; const float* b2; const float* w3; const float* b3; int32_t D;
  DecParams params() const {
    return DecParams{p, q, (uint32_t)(ldp / 4), (uint32_t)(ldq / 4), ei, ld, E, extra, cvec, w2, b2, w3, b3};
  }
};

static bool nd_supported(int32_t D) { return D == 32 || D == 128; }

// f(std::integral_constant<int, D>) for the runtime width D (checked by check_common)
template <typename F>
static void with_width(int32_t D, F&& f) {
  if (D == 32) f(std::integral_constant<int, 32>{});
  else if (D == 64) f(std::integral_constant<int, 64>{});
  else f(std::integral_constant<int, 128>{});
}

// workgroups of a launch over `num_edges` edges: a function of the list's length alone
static int64_t grid_of(int32_t D, int64_t num_edges) {
  const int waves = D == 128 ? Shape<128>::WAVES : Shape<64>::WAVES;
  static_assert(Shape<32>::WAVES == Shape<64>::WAVES, "grid_of");
  const int64_t n_tiles = (num_edges + TE - 1) / TE;
  int64_t grid = (n_tiles + waves - 1) / waves;
  if (grid > kMaxGrid) grid = kMaxGrid;
  if (grid < 1) grid = 1;
  return grid;
}

static size_t workspace_of(int32_t D, int64_t num_edges) {
  return (size_t)grid_of(D, num_edges < 0 ? 0 : num_edges) * (size_t)(D * D + 3 * D + 2) * sizeof(float);
}

static int check_common(const char* who, bool nd, const DecArgs& c) {
  const int32_t D = c.D;
  if (nd) PG_CHECK_ARG(nd_supported(D), PANGNN_E_BADARG, "%s: built for node_dim 32 and 128, got %d", who, (int)D);
  else PG_CHECK_ARG(D == 64, PANGNN_E_BADARG, "%s: fused decoder is built for node_dim 64, got %d", who, (int)D);
  PG_CHECK_ARG(c.E >= 0 && c.ld >= c.E && c.num_nodes >= 0, PANGNN_E_BADARG, "%s: bad size", who);
  PG_CHECK_ARG(c.ldp >= D && c.ldq >= D && c.ldp % 4 == 0 && c.ldq % 4 == 0, PANGNN_E_BADARG,
               "%s: ldp / ldq must be multiples of 4 and >= %d", who, (int)D);
  PG_CHECK_ARG((double)c.num_nodes * (double)(c.ldp > c.ldq ? c.ldp : c.ldq) * 4.0 < 4294967296.0, PANGNN_E_TOOLARGE,
               "%s: node tables must stay under 4 GiB (32-bit gather offsets)", who);
  if (c.E == 0) return 0;
  PG_CHECK_ARG(c.p && c.q && c.ei && c.w2 && c.b2 && c.w3 && c.b3 && (!c.extra || c.cvec), PANGNN_E_BADARG,
               "%s: null pointer", who);
  PG_CHECK_ARG(aligned16(c.p) && aligned16(c.q) && aligned16(c.w2), PANGNN_E_ALIGN,
               "%s: p / q / w2 must be 16-byte aligned", who);
  return 0;
}

// precision: 0, or 1 from pangnn_decoder_mlp_infer_f32 = the bf16 matrix pipe with split operands of decoder16.hip (the
// first product of its training kernel)
static int decoder_fwd(const char* who, bool nd, const DecArgs& c, float* logits, int32_t precision, hipStream_t s) {
  int rc = check_common(who, nd, c);
  if (rc) return rc;
  PG_CHECK_ARG(precision == 0 || precision == 1, PANGNN_E_BADARG, "pangnn_decoder_mlp_infer_f32: precision must be 0 or 1");
  if (c.E == 0) return 0;
  PG_CHECK_ARG(logits, PANGNN_E_BADARG, "%s: null logits", who);
  if (precision)
    return launch_decoder_infer16(c.p, c.ldp, c.q, c.ldq, c.ei, c.ld, c.E, c.extra, c.cvec, c.w2, c.b2, c.w3, c.b3, logits, s);
  const int64_t n_tiles = (c.E + TE - 1) / TE;
  const dim3 g((unsigned)grid_of(c.D, c.E));
  const DecParams a = c.params();
  with_width(c.D, [&](auto d) {
    constexpr int D = decltype(d)::value;
    hipLaunchKernelGGL((decoder_fwd_kernel<D>), g, dim3(Shape<D>::WAVES * 64), 0, s, a, logits, n_tiles);
  });
  PG_CHECK_LAUNCH(who);
  return 0;
}

struct GradOut {   // the outputs and the workspace of the two training operations
  float* g_h1; float* g_w2; float* g_b2; float* g_w3; float* g_b3; float* g_cvec; float* part_buf; const int32_t* part_off;
  void* workspace; size_t workspace_bytes;
};

// the backward kernel (lp: with the fused loss; live: of a padded batch, with lp) and the reduction over its slabs
static int launch_bwd(const char* who, const DecArgs& c, const float* g_logits, const LossParams* lp, const int64_t* live,
                      float* loss, int32_t precision, const GradOut& o, hipStream_t s) {
  PG_CHECK_ARG(o.g_w2 && o.g_b2 && o.g_w3 && o.g_b3, PANGNN_E_BADARG, "%s: null gradient output", who);
  PG_CHECK_ARG(precision == 0, PANGNN_E_BADARG,
               "%s: only precision 0 (f32 MFMA) here; the bf16 matrix-pipe mode is pangnn_decoder_train_f32 + "
               "pangnn_decoder_dgrad_f32", who);
  const int64_t n_tiles = (c.E + TE - 1) / TE;
  const int64_t grid = grid_of(c.D, c.E);
  const size_t need = workspace_of(c.D, c.E);
  PG_CHECK_ARG(o.workspace && o.workspace_bytes >= need, PANGNN_E_WORKSPACE, "%s: workspace too small", who);
  PG_CHECK_ARG(c.E == 0 || o.g_h1, PANGNN_E_BADARG, "%s: null g_h1", who);
  float* ws = static_cast<float*>(o.workspace);
  if (c.E == 0) {
    hipError_t e = hipMemsetAsync(ws, 0, need, s);
    PG_CHECK_ARG(e == hipSuccess, (int)e, "%s: memset failed", who);
  } else {
    PG_CHECK_ARG((o.part_buf == nullptr) == (o.part_off == nullptr), PANGNN_E_BADARG,
                 "%s: part_buf and part_off go together", who);
    const DecParams a = c.params();
    const LossParams l = lp ? *lp : LossParams{nullptr, nullptr, 0.f, nullptr};
    const RunSumParams rs{o.part_buf, o.part_off};
    const dim3 g((unsigned)grid);
    with_width(c.D, [&](auto d) {
      constexpr int D = decltype(d)::value;
      const dim3 b(Shape<D>::WAVES * 64);
      const void* given = lp ? static_cast<const void*>(live) : static_cast<const void*>(g_logits);
      if (lp && live && rs.part) hipLaunchKernelGGL((decoder_bwd_kernel<D, true, true, true>), g, b, 0, s, a, given, l, rs, o.g_h1, ws, n_tiles);
      else if (lp && live) hipLaunchKernelGGL((decoder_bwd_kernel<D, true, false, true>), g, b, 0, s, a, given, l, rs, o.g_h1, ws, n_tiles);
      else if (lp && rs.part) hipLaunchKernelGGL((decoder_bwd_kernel<D, true, true>), g, b, 0, s, a, given, l, rs, o.g_h1, ws, n_tiles);
      else if (lp) hipLaunchKernelGGL((decoder_bwd_kernel<D, true, false>), g, b, 0, s, a, given, l, rs, o.g_h1, ws, n_tiles);
      else if (rs.part) hipLaunchKernelGGL((decoder_bwd_kernel<D, false, true>), g, b, 0, s, a, given, l, rs, o.g_h1, ws, n_tiles);
      else hipLaunchKernelGGL((decoder_bwd_kernel<D, false, false>), g, b, 0, s, a, given, l, rs, o.g_h1, ws, n_tiles);
    });
    PG_CHECK_LAUNCH(who);
  }
  return launch_reduce(who, ws, (int)grid, c.D * c.D + 3 * c.D + 2, c.D, o.g_w2, o.g_b2, o.g_w3, o.g_cvec, o.g_b3, loss, s);
}

static int decoder_bwd(const char* who, bool nd, const DecArgs& c, const float* g_logits, int32_t precision,
                       const GradOut& o, hipStream_t s) {
  int rc = check_common(who, nd, c);
  if (rc) return rc;
  PG_CHECK_ARG(c.E == 0 || g_logits, PANGNN_E_BADARG, "%s: null g_logits", who);
  return launch_bwd(who, c, g_logits, nullptr, nullptr, nullptr, precision, o, s);
}

// `want_live`: the *_loss_live_f32 entry points — live_edges is required and `denom` is not looked at (the kernel divides by
// the live count it reads)
static int decoder_loss(const char* who, bool nd, const DecArgs& c, const float* y, const float* pos_weight, int64_t denom,
                        float* logits, float* loss, int32_t precision, const GradOut& o, bool want_live, const int64_t* live,
                        hipStream_t s) {
  int rc = check_common(who, nd, c);
  if (rc) return rc;
  PG_CHECK_ARG((want_live || denom > 0) && loss && (c.E == 0 || (y && logits)), PANGNN_E_BADARG,
               "%s: bad denom / null pointer", who);
  PG_CHECK_ARG(!want_live || live, PANGNN_E_BADARG, "%s: null live_edges", who);
  const LossParams lp{y, pos_weight, want_live ? 0.f : 1.0f / (float)denom, logits};
  return launch_bwd(who, c, nullptr, &lp, want_live ? live : nullptr, loss, precision, o, s);
}

// the nd family passes its workspace size as an int64_t: a negative one is too small
static size_t ws_size(int64_t bytes) { return bytes > 0 ? (size_t)bytes : 0; }

}  // namespace pangnn

using namespace pangnn;

extern "C" int pangnn_decoder_mlp_infer_f32(const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t num_nodes,
                                            const int64_t* edge_index, int64_t ld, int64_t num_edges, const float* extra,
                                            const float* cvec, const float* w2, const float* b2, const float* w3,
                                            const float* b3, int32_t D, float* logits, int32_t precision,
                                            pangnn_stream_t stream) {
  const DecArgs c{p, ldp, q, ldq, num_nodes, edge_index, ld, num_edges, extra, cvec, w2, b2, w3, b3, D};
  return decoder_fwd("pangnn_decoder_mlp_fwd_f32", false, c, logits, precision, (hipStream_t)stream);
}

extern "C" int pangnn_decoder_mlp_fwd_f32(const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t num_nodes,
                                          const int64_t* edge_index, int64_t ld, int64_t num_edges, const float* extra,
                                          const float* cvec, const float* w2, const float* b2, const float* w3,
                                          const float* b3, int32_t D, float* logits, pangnn_stream_t stream) {
  const DecArgs c{p, ldp, q, ldq, num_nodes, edge_index, ld, num_edges, extra, cvec, w2, b2, w3, b3, D};
  return decoder_fwd("pangnn_decoder_mlp_fwd_f32", false, c, logits, 0, (hipStream_t)stream);
}

extern "C" size_t pangnn_decoder_mlp_bwd_workspace_bytes(int64_t num_edges) { return workspace_of(64, num_edges); }

extern "C" int pangnn_decoder_mlp_bwd_f32(const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t num_nodes,
                                          const int64_t* edge_index, int64_t ld, int64_t num_edges, const float* extra,
                                          const float* cvec, const float* w2, const float* b2, const float* w3,
                                          const float* b3, int32_t D, const float* g_logits, float* g_h1, float* g_w2,
                                          float* g_b2, float* g_w3, float* g_b3, float* g_cvec, float* part_buf,
                                          const int32_t* part_off, int32_t precision, void* workspace,
                                          size_t workspace_bytes, pangnn_stream_t stream) {
  const DecArgs c{p, ldp, q, ldq, num_nodes, edge_index, ld, num_edges, extra, cvec, w2, b2, w3, b3, D};
  const GradOut o{g_h1, g_w2, g_b2, g_w3, g_b3, g_cvec, part_buf, part_off, workspace, workspace_bytes};
  return decoder_bwd("pangnn_decoder_mlp_bwd_f32", false, c, g_logits, precision, o, (hipStream_t)stream);
}

extern "C" int pangnn_decoder_mlp_loss_f32(const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t num_nodes,
                                           const int64_t* edge_index, int64_t ld, int64_t num_edges, const float* extra,
                                           const float* cvec, const float* w2, const float* b2, const float* w3,
                                           const float* b3, int32_t D, const float* y, const float* pos_weight,
                                           int64_t denom, float* logits, float* loss, float* g_h1, float* g_w2,
                                           float* g_b2, float* g_w3, float* g_b3, float* g_cvec, float* part_buf,
                                           const int32_t* part_off, int32_t precision, void* workspace,
                                           size_t workspace_bytes, pangnn_stream_t stream) {
  const DecArgs c{p, ldp, q, ldq, num_nodes, edge_index, ld, num_edges, extra, cvec, w2, b2, w3, b3, D};
  const GradOut o{g_h1, g_w2, g_b2, g_w3, g_b3, g_cvec, part_buf, part_off, workspace, workspace_bytes};
  return decoder_loss("pangnn_decoder_mlp_loss_f32", false, c, y, pos_weight, denom, logits, loss, precision, o, false, nullptr,
                      (hipStream_t)stream);
}

extern "C" int pangnn_decoder_mlp_loss_live_f32(const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t num_nodes,
                                                const int64_t* edge_index, int64_t ld, int64_t num_edges, const float* extra,
                                                const float* cvec, const float* w2, const float* b2, const float* w3,
                                                const float* b3, int32_t D, const float* y, const float* pos_weight,
                                                int64_t denom, float* logits, float* loss, float* g_h1, float* g_w2,
                                                float* g_b2, float* g_w3, float* g_b3, float* g_cvec, float* part_buf,
                                                const int32_t* part_off, int32_t precision, const int64_t* live_edges,
                                                void* workspace, int64_t workspace_bytes, pangnn_stream_t stream) {
  const DecArgs c{p, ldp, q, ldq, num_nodes, edge_index, ld, num_edges, extra, cvec, w2, b2, w3, b3, D};
  const GradOut o{g_h1, g_w2, g_b2, g_w3, g_b3, g_cvec, part_buf, part_off, workspace, ws_size(workspace_bytes)};
  return decoder_loss("pangnn_decoder_mlp_loss_live_f32", false, c, y, pos_weight, denom, logits, loss, precision, o, true,
                      live_edges, (hipStream_t)stream);
}

extern "C" int pangnn_decoder_nd_supported(int32_t D) { return nd_supported(D) ? 1 : 0; }

extern "C" int pangnn_decoder_nd_fwd_f32(const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t num_nodes,
                                         const int64_t* edge_index, int64_t ld, int64_t num_edges, const float* extra,
                                         const float* cvec, const float* w2, const float* b2, const float* w3,
                                         const float* b3, int32_t D, float* logits, pangnn_stream_t stream) {
  const DecArgs c{p, ldp, q, ldq, num_nodes, edge_index, ld, num_edges, extra, cvec, w2, b2, w3, b3, D};
  return decoder_fwd("pangnn_decoder_nd_fwd_f32", true, c, logits, 0, (hipStream_t)stream);
}

extern "C" size_t pangnn_decoder_nd_bwd_workspace_bytes(int32_t D, int64_t num_edges) {
  return nd_supported(D) ? workspace_of(D, num_edges) : 0;
}

extern "C" int pangnn_decoder_nd_bwd_f32(const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t num_nodes,
                                         const int64_t* edge_index, int64_t ld, int64_t num_edges, const float* extra,
                                         const float* cvec, const float* w2, const float* b2, const float* w3,
                                         const float* b3, int32_t D, const float* g_logits, float* g_h1, float* g_w2,
                                         float* g_b2, float* g_w3, float* g_b3, float* g_cvec, float* part_buf,
                                         const int32_t* part_off, void* workspace, int64_t workspace_bytes,
                                         pangnn_stream_t stream) {
  const DecArgs c{p, ldp, q, ldq, num_nodes, edge_index, ld, num_edges, extra, cvec, w2, b2, w3, b3, D};
  const GradOut o{g_h1, g_w2, g_b2, g_w3, g_b3, g_cvec, part_buf, part_off, workspace, ws_size(workspace_bytes)};
  return decoder_bwd("pangnn_decoder_nd_bwd_f32", true, c, g_logits, 0, o, (hipStream_t)stream);
}

extern "C" int pangnn_decoder_nd_loss_f32(const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t num_nodes,
                                          const int64_t* edge_index, int64_t ld, int64_t num_edges, const float* extra,
                                          const float* cvec, const float* w2, const float* b2, const float* w3,
                                          const float* b3, int32_t D, const float* y, const float* pos_weight,
                                          int64_t denom, float* logits, float* loss, float* g_h1, float* g_w2,
                                          float* g_b2, float* g_w3, float* g_b3, float* g_cvec, float* part_buf,
                                          const int32_t* part_off, void* workspace, int64_t workspace_bytes,
                                          pangnn_stream_t stream) {
  const DecArgs c{p, ldp, q, ldq, num_nodes, edge_index, ld, num_edges, extra, cvec, w2, b2, w3, b3, D};
  const GradOut o{g_h1, g_w2, g_b2, g_w3, g_b3, g_cvec, part_buf, part_off, workspace, ws_size(workspace_bytes)};
  return decoder_loss("pangnn_decoder_nd_loss_f32", true, c, y, pos_weight, denom, logits, loss, 0, o, false, nullptr,
                      (hipStream_t)stream);
}

extern "C" int pangnn_decoder_nd_loss_live_f32(const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t num_nodes,
                                               const int64_t* edge_index, int64_t ld, int64_t num_edges, const float* extra,
                                               const float* cvec, const float* w2, const float* b2, const float* w3,
                                               const float* b3, int32_t D, const float* y, const float* pos_weight,
                                               int64_t denom, float* logits, float* loss, float* g_h1, float* g_w2,
                                               float* g_b2, float* g_w3, float* g_b3, float* g_cvec, float* part_buf,
                                               const int32_t* part_off, const int64_t* live_edges, void* workspace,
                                               int64_t workspace_bytes, pangnn_stream_t stream) {
  const DecArgs c{p, ldp, q, ldq, num_nodes, edge_index, ld, num_edges, extra, cvec, w2, b2, w3, b3, D};
  const GradOut o{g_h1, g_w2, g_b2, g_w3, g_b3, g_cvec, part_buf, part_off, workspace, ws_size(workspace_bytes)};
  return decoder_loss("pangnn_decoder_nd_loss_live_f32", true, c, y, pos_weight, denom, logits, loss, 0, o, true, live_edges,
                      (hipStream_t)stream);
}
