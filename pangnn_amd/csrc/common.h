// Shared helpers for libpangnn_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/pangnn_hip.h"

namespace pangnn {

void set_error(const char* fmt, ...);

#define PG_CHECK_ARG(cond, code, ...)            \
  do {                                           \
    if (!(cond)) {                               \
      ::pangnn::set_error(__VA_ARGS__);          \
      return (code);                             \
    }                                            \
  } while (0)

#define PG_CHECK_LAUNCH(name)                                                          \
  do {                                                                                 \
    hipError_t e__ = hipGetLastError();                                                \
    if (e__ != hipSuccess) {                                                           \
      ::pangnn::set_error("%s: launch failed: %s", (name), hipGetErrorString(e__));    \
      return (int)e__;                                                                 \
    }                                                                                  \
  } while (0)

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

constexpr int kWave = 64;          // CDNA4 wavefront
constexpr int kBlock = 256;        // 4 waves per workgroup
constexpr int kWavesPerBlock = kBlock / kWave;

// ---- host side: launch geometry, workspace carving and the argument checks that several entry points share
// compute units of the current device; 256 (an MI355X) where the query fails
inline int cu_count() {
  int dev = 0, v = 0;
  if (hipGetDevice(&dev) == hipSuccess &&
      hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
    return v;
  return 256;
}
inline int64_t blocks_for(int64_t items, int per_block) { return (items + per_block - 1) / per_block; }
// workgroups of kBlock threads for `work` items of a grid-stride kernel: at least one, at most `cap` (each file states its own)
inline unsigned capped_grid(int64_t work, int64_t cap) {
  const int64_t b = blocks_for(work, kBlock);
  return (unsigned)(b < 1 ? 1 : b > cap ? cap : b);
}
// v >= 0 rounded up to a multiple of a
template <typename T>
constexpr T align_up(T v, int a) { return (v + (a - 1)) / a * a; }
// the row widths of the gather kernels: G = F / 4 lanes per row, G a power of two that divides the wave
inline bool row_width_ok(int32_t f) { return f == 16 || f == 32 || f == 64 || f == 128 || f == 256; }
inline bool row_dtype_ok(int32_t t) { return t == PANGNN_DTYPE_F32 || t == PANGNN_DTYPE_BF16 || t == PANGNN_DTYPE_F16; }
// every row starts on a lane's load width: 16 bytes (f32) / 8 bytes (2-byte rows), ld a multiple of 4 elements
inline bool rows_aligned(const void* p, int32_t dtype, int64_t ld) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  return ld % 4 == 0 && (dtype == PANGNN_DTYPE_F32 ? (a & 15u) == 0 : (a & 7u) == 0);
}

// Second stage of the two-stage reductions (per-workgroup partial rows -> one row), reproducible and short:
// a 1024-thread block owns 64 consecutive elements; wave g adds parts g, g+16, g+32, ... in that order, then the
// 16 wave sums are added in wave order.  (One thread walking all parts serially took 60-240 us per call.)
// Launch with kSumThreads threads and (len + 63) / 64 blocks; the result is valid in wave 0 (threadIdx.x < 64).
constexpr int kSumGroups = 16;
constexpr int kSumThreads = kSumGroups * kWave;
// the longest edge list of the small-structure path (graph_build.hip): what one workgroup takes whole, a collated mini-batch
constexpr int kSmallMaxEdges = 16384;
#ifdef __HIPCC__
// ---- the two per-edge expressions of the loss and the confusion counts, stated once for every kernel that evaluates them
// (edge_ops.hip: bce_kernel, confusion_kernel; batch_stats.hip)
// prediction = (score >= threshold), score = sigmoid(x) or x itself (pangnn.py:219-221); label = (y > 0.5)
__device__ __forceinline__ bool predicted_positive(float x, float threshold, bool apply_sigmoid) {
  const float score = apply_sigmoid ? 1.0f / (1.0f + expf(-x)) : x;
  return score >= threshold;
}
__device__ __forceinline__ bool label_positive(float y) { return y > 0.5f; }
// BCEWithLogits(pos_weight) of one edge: (1-y) x + (1 + (pw-1) y) softplus(-x), softplus(-x) = log1p(exp(-|x|)) + max(-x, 0)
__device__ __forceinline__ float bce_term(float x, float y, float pw) {
  const float lw = 1.f + (pw - 1.f) * y;
  const float t = expf(-fabsf(x));
  const float sp = log1pf(t) + fmaxf(-x, 0.f);
  return (1.f - y) * x + lw * sp;
}

// ---- 2-byte row formats (storage only; every sum and product is fp32).  A kernel templated on its storage type uses
// `unsigned short` for bfloat16 bits (bf16 -> f32 is a shift) and `_Float16` for IEEE half (`--mixed_precision fp16`,
// src/setup.py:50; v_cvt_f32_f16 / v_cvt_f16_f32); RowFmt<T>::value is the PANGNN_DTYPE_* code of T.
template <typename T> struct RowFmt { static constexpr int value = 0; };
template <> struct RowFmt<unsigned short> { static constexpr int value = 1; };
template <> struct RowFmt<_Float16> { static constexpr int value = 2; };
// four consecutive stored elements (8 bytes) -> f32, exact
__device__ __forceinline__ float4 rows16_to_f32(uint2 t, int fmt) {
  if (fmt == 2) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 a = __builtin_bit_cast(h2, t.x), b = __builtin_bit_cast(h2, t.y);
    return make_float4((float)a[0], (float)a[1], (float)b[0], (float)b[1]);
  }
  return make_float4(__uint_as_float(t.x << 16), __uint_as_float(t.x & 0xffff0000u),
                     __uint_as_float(t.y << 16), __uint_as_float(t.y & 0xffff0000u));
}
__device__ __forceinline__ float row16_to_f32(unsigned short bits, int fmt) {
  return fmt == 2 ? (float)__builtin_bit_cast(_Float16, bits) : __uint_as_float((uint32_t)bits << 16);
}
// f32 -> four stored elements, each rounded to nearest even
__device__ __forceinline__ uint2 f32_to_rows16(float v0, float v1, float v2, float v3, int fmt) {
  if (fmt == 2) {
    // f32 values first, then one rounding each (no v_fma_mixlo_f16 folding of the producing multiply-add: see linear.hip)
    asm volatile("" : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3));
    const _Float16 o[4] = {(_Float16)v0, (_Float16)v1, (_Float16)v2, (_Float16)v3};
    return *reinterpret_cast<const uint2*>(o);
  }
  const __bf16 o[4] = {(__bf16)v0, (__bf16)v1, (__bf16)v2, (__bf16)v3};
  return *reinterpret_cast<const uint2*>(o);
}

// A lane's piece of a gathered row as stored: four consecutive elements (16 bytes of f32, 8 bytes of bf16 / f16; xf is the
// PANGNN_DTYPE_* code) -> f32, exact.  PIN, for the kernels that multiply two gathered pieces (edge_score.hip,
// edge_weight_grad.hip): half rows are f32 values first, so that no conversion is folded into a mixed / packed-dot instruction
// (v_dot2_f32_f16, v_fma_mix_f32) that rounds differently from the f32 call on the up-converted rows.  The propagate of
// spmm.hip deliberately has no pin: a piece meets nothing there but an fp32 weight in one fmaf.
template <bool PIN>
__device__ __forceinline__ float4 row_piece(const char* p, int xf) {
  if (!xf) return *reinterpret_cast<const float4*>(p);
  float4 r = rows16_to_f32(*reinterpret_cast<const uint2*>(p), xf);
  if (PIN && xf == 2) asm volatile("" : "+v"(r.x), "+v"(r.y), "+v"(r.z), "+v"(r.w));
  return r;
}

// the four products of two pieces in a fixed order
__device__ __forceinline__ float dot4(float4 a, float4 b) {
  return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)));
}

// sum / maximum over every aligned group of G lanes by an xor butterfly (offsets G / 2 ... 1): a fixed order, and every lane
// of a group ends with the same bits.  group_max is fmax's: a NaN operand is ignored.
template <int G, typename T>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
  for (int off = G / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
template <int G, typename T>
__device__ __forceinline__ T group_max(T v) {
#pragma unroll
  for (int off = G / 2; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  return v;
}
template <typename T> __device__ __forceinline__ T wave_sum(T v) { return group_sum<kWave>(v); }
template <typename T> __device__ __forceinline__ T wave_max(T v) { return group_max<kWave>(v); }

// The row of a CSR that holds entry k (0 <= k < rowptr[n_rows]): the last r in [0, n_rows) with rowptr[r] <= k, hence
// rowptr[r + 1] > k — among equal row pointers the non-empty row, empty rows are stepped over.  Always inside
// [0, n_rows - 1], whatever rowptr holds.
__device__ __forceinline__ int64_t row_of_entry(const int64_t* __restrict__ rowptr, int64_t n_rows, int64_t k) {
  int64_t lo = 0, hi = n_rows;                 // invariant: rowptr[lo] <= k < rowptr[hi]
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (rowptr[mid] <= k) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void wave_lds_sync() {
  // LDS operations of one wave execute in issue order; this only pins the compiler's ordering.
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// row of the 32x32 MFMA accumulator held in register r by a lane of half hh
__device__ __forceinline__ constexpr int acc_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

__device__ __forceinline__ float ordered_parts_sum(const float* __restrict__ part, int n_parts, int64_t stride, int i,
                                                   int len) {
  __shared__ float red[kSumGroups][kWave];
  const int e = threadIdx.x & (kWave - 1), g = threadIdx.x >> 6;
  float s = 0.f;
  if (i < len) {
    // same order of additions as the plain loop; eight loads in flight instead of one dependent load-add per L2 round trip
    // (the one-workgroup finish of 2048 x 64 band partials took 35 us)
    int p = g;
    for (; p + 7 * kSumGroups < n_parts; p += 8 * kSumGroups) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = part[(int64_t)(p + u * kSumGroups) * stride + i];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; p < n_parts; p += kSumGroups) s += part[(int64_t)p * stride + i];
  }
  red[g][e] = s;
  __syncthreads();
  float t = 0.f;
  if (g == 0)
    for (int k = 0; k < kSumGroups; ++k) t += red[k][e];
  return t;
}
#endif

}  // namespace pangnn
