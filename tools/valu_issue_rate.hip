// gfx950 micro-benchmark: vector-instruction issue rate of ONE SIMD as a function of the number of resident waves.
// Every wave runs a long stream of independent v_fma_f32 (16 accumulators, no memory traffic); the grid puts `w` waves
// on every SIMD of every CU.  Prints cycles per wave-instruction per SIMD (kernel time x clock / instructions per SIMD).
// Modes 6 / 7: v_fma_mix_f32 with an IEEE-half first operand taken from the low / high half of a dword (op_sel:[0,0,0] /
// [1,0,0], op_sel_hi:[1,0,0]) — the instruction the T kernel's dL/db2 sums use (csrc/decoder16.hip).  After the rates, a
// correctness pass: the first wave of every SIMD runs both forms on changing operands and compares every lane's result bit
// for bit with v_cvt_f32_f16 + v_fma_f32, while the other waves of the SIMD run v_mfma_f32_16x16x32_bf16 back to back
// (profiles/r03_pk_opsel_probe.txt saw packed-f32 op_sel forms go wrong in lanes 48-63 in that company).
//   hipcc --offload-arch=gfx950 -O3 -fno-slp-vectorize tools/valu_issue_rate.hip -o /tmp/valu_rate && /tmp/valu_rate
// (-fno-slp-vectorize as csrc/Makefile builds decoder16.hip: the SLP vectoriser turns pairs of the mixed FMAs into v_pk_fma_f32)
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <vector>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// (float)half `HI` of w, times g, plus acc: one v_fma_mix_f32
template <int HI>
__device__ __forceinline__ float fma_half(unsigned w, float g, float acc) {
  return __builtin_fmaf((float)__builtin_bit_cast(f16x2, w)[HI], g, acc);
}

struct MixReport { unsigned long long wrong, wrong_hi_lanes, checked; int lane[4]; unsigned word[4]; float got[4], want[4]; };

// waves 0-3 (one per SIMD) check; every further wave is the matrix-pipe neighbour
__global__ __launch_bounds__(1024) void mix_check(MixReport* rep, int iters, float seed) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (wave >= 4) {
    bf16x8 fa, fb;
    for (int q = 0; q < 8; ++q) { fa[q] = (__bf16)(float)(lane + q); fb[q] = (__bf16)(float)(lane - q); }
    f32x4 small = {0.f, 0.f, 0.f, 0.f};
    for (int it = 0; it < iters * 4; ++it) {
      small = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, small, 0, 0, 0);
      small = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, small, 0, 0, 0);
    }
    if (small[0] == 12345.678f) atomicAdd(&rep->wrong, 1ull << 40);
    return;
  }
  unsigned state = 2654435761u * (blockIdx.x * 256 + threadIdx.x + 1);
  float g = seed + 0.125f * lane, acc = -seed;
  unsigned long long nbad = 0;
  for (int it = 0; it < iters; ++it) {
    state = state * 1664525u + 1013904223u;
    // every finite half pattern; every fourth word the T kernel's own operand (halves 0x3c00 = 1.0 or 0)
    unsigned w = (it & 3) == 3 ? ((state >> 8) & 0x00010001u) * 0x3c00u : state & 0xfbfffbffu;
    asm volatile("" : "+v"(w));
    const float got0 = fma_half<0>(w, g, acc), got1 = fma_half<1>(w, g, acc);
    unsigned wc = w;
    asm volatile("" : "+v"(wc));                         // a copy the optimiser cannot trace back: its conversions are its own
    float f0 = (float)__builtin_bit_cast(f16x2, wc)[0], f1 = (float)__builtin_bit_cast(f16x2, wc)[1];
    asm volatile("" : "+v"(f0), "+v"(f1));               // a float in a register: v_cvt_f32_f16, then a plain v_fma_f32
    const float want0 = __builtin_fmaf(f0, g, acc), want1 = __builtin_fmaf(f1, g, acc);
    const int b0 = __builtin_bit_cast(unsigned, got0) != __builtin_bit_cast(unsigned, want0);
    const int b1 = __builtin_bit_cast(unsigned, got1) != __builtin_bit_cast(unsigned, want1);
    if (b0 | b1) {
      const unsigned long long slot = atomicAdd(&rep->wrong, (unsigned long long)(b0 + b1));
      if (slot < 4) { rep->lane[slot] = lane; rep->word[slot] = w; rep->got[slot] = b0 ? got0 : got1; rep->want[slot] = b0 ? want0 : want1; }
      if (lane >= 48) atomicAdd(&rep->wrong_hi_lanes, (unsigned long long)(b0 + b1));
      ++nbad;
    }
    g += 0.75f; acc = 0.5f * acc + 1.25f;
  }
  if (lane == 0) atomicAdd(&rep->checked, 2ull * 64 * iters);
  (void)nbad;
}

template <int MODE>
__global__ void k(float* out, int iters, float a, float b) {
  float x[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] = threadIdx.x + i;
  unsigned hw[4];                        // modes 6 / 7: four words of two halves each
#pragma unroll
  for (int i = 0; i < 4; ++i) hw[i] = __builtin_bit_cast(unsigned, b) + i;
  for (int it = 0; it < iters; ++it) {
    // opaque once per round, in ONE statement: the conversions stay in the loop and no instruction is added
    if (MODE == 6 || MODE == 7) asm volatile("" : "+v"(hw[0]), "+v"(hw[1]), "+v"(hw[2]), "+v"(hw[3]));
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (MODE == 0) x[i] = __builtin_fmaf(x[i], a, b);                      // v_fma_f32
      if (MODE == 1) x[i] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, x[i]) & 0xffff0fffu) - b;   // v_and + v_sub
      if (MODE == 2) x[i] = __builtin_bit_cast(float, __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, x[i]), __builtin_bit_cast(unsigned, x[(i + 1) & 15]), 0x07060302u));
      if (MODE == 3) x[0] = __builtin_fmaf(x[0], a, b);                      // one dependent chain of v_fma_f32
      if (MODE == 4) {                                                       // v_cvt_pk_bf16_f32
        typedef float f2 __attribute__((ext_vector_type(2)));
        typedef __bf16 b2 __attribute__((ext_vector_type(2)));
        asm volatile("" : "+v"(x[i]));
        x[i] = __builtin_bit_cast(float, __builtin_convertvector((f2){x[i], x[(i + 1) & 15]}, b2));
      }
      if (MODE == 6 || MODE == 7)                                            // v_fma_mix_f32, half operand low / high
        x[i] = MODE == 6 ? fma_half<0>(hw[i & 3], a, x[i]) : fma_half<1>(hw[i & 3], a, x[i]);
      if (MODE == 5 && (i & 1) == 0) {                                       // v_pk_add_f32 (two floats per lane)
        typedef float f2 __attribute__((ext_vector_type(2)));
        f2 v = {x[i], x[i + 1]};
        asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(v) : "v"((f2){a, b}));
        x[i] = v[0]; x[i + 1] = v[1];
      }
    }
  }
  float s = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) s += x[i];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

int main() {
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
  int clk_khz = 0;
  (void)hipDeviceGetAttribute(&clk_khz, hipDeviceAttributeClockRate, 0);
  float* out;
  (void)hipMalloc(&out, (size_t)cus * 2048 * sizeof(float));
  const int iters = 20000;
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  for (int mode = 0; mode < 8; ++mode)
    for (int waves_per_simd : {1, 2, 3, 4}) {
      const int threads = 64 * 4 * waves_per_simd;            // one block per CU
      auto launch = [&]() {
        if (mode == 0) hipLaunchKernelGGL(k<0>, dim3(cus), dim3(threads), 0, 0, out, iters, 1.0001f, 0.5f);
        if (mode == 1) hipLaunchKernelGGL(k<1>, dim3(cus), dim3(threads), 0, 0, out, iters, 1.0001f, 0.5f);
        if (mode == 2) hipLaunchKernelGGL(k<2>, dim3(cus), dim3(threads), 0, 0, out, iters, 1.0001f, 0.5f);
        if (mode == 3) hipLaunchKernelGGL(k<3>, dim3(cus), dim3(threads), 0, 0, out, iters, 1.0001f, 0.5f);
        if (mode == 4) hipLaunchKernelGGL(k<4>, dim3(cus), dim3(threads), 0, 0, out, iters, 1.0001f, 0.5f);
        if (mode == 5) hipLaunchKernelGGL(k<5>, dim3(cus), dim3(threads), 0, 0, out, iters, 1.0001f, 0.5f);
        if (mode == 6) hipLaunchKernelGGL(k<6>, dim3(cus), dim3(threads), 0, 0, out, iters, 1.0001f, 0.5f);
        if (mode == 7) hipLaunchKernelGGL(k<7>, dim3(cus), dim3(threads), 0, 0, out, iters, 1.0001f, 0.5f);
      };
      launch();
      (void)hipDeviceSynchronize();
      (void)hipEventRecord(e0);
      launch();
      (void)hipEventRecord(e1);
      (void)hipEventSynchronize(e1);
      float ms = 0;
      (void)hipEventElapsedTime(&ms, e0, e1);
      const double inst_per_simd = (double)iters * (mode == 1 ? 32 : mode == 5 ? 8 : 16) * waves_per_simd;
      static const char* names[] = {"v_fma_f32", "v_and+v_sub", "v_perm_b32", "v_fma_f32, one dependent chain", "v_cvt_pk_bf16_f32", "v_pk_add_f32",
                                     "v_fma_mix_f32 op_sel:[0,0,0] op_sel_hi:[1,0,0]", "v_fma_mix_f32 op_sel:[1,0,0] op_sel_hi:[1,0,0]"};
      printf("mode %d (%s) waves/SIMD %d: %.3f ms, %.2f cycles per wave-instruction per SIMD at %.2f GHz nominal\n", mode,
             names[mode], waves_per_simd, ms,
             ms * 1e-3 * clk_khz * 1e3 / inst_per_simd, clk_khz / 1e6);
    }
  MixReport* d;
  (void)hipMalloc(&d, sizeof(MixReport));
  for (int waves_per_simd : {1, 2, 4}) {
    (void)hipMemset(d, 0, sizeof(MixReport));
    const int citers = 200000;
    hipLaunchKernelGGL(mix_check, dim3(cus), dim3(256 * waves_per_simd), 0, 0, d, citers, 1.5f);
    (void)hipDeviceSynchronize();
    MixReport h;
    (void)hipMemcpy(&h, d, sizeof(MixReport), hipMemcpyDeviceToHost);
    printf("v_fma_mix_f32 (both halves) against v_cvt_f32_f16 + v_fma_f32, %d bf16-MFMA neighbour wave(s) per SIMD: %llu wrong of "
           "%llu results, %llu in lanes 48-63", waves_per_simd - 1, h.wrong, h.checked, h.wrong_hi_lanes);
    for (int i = 0; i < 4 && i < (int)h.wrong; ++i)
      printf("  [lane %d word %08x got %g want %g]", h.lane[i], h.word[i], h.got[i], h.want[i]);
    printf("\n");
  }
  return 0;
}
