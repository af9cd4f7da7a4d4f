// The decoder's run-sum plan of a CSR order from its row pointer alone (EdgeStructure._plan_of_sorted_keys is the written
// definition and the referee: pangnn_amd/graph.py; the S / T kernels of decoder.hip / decoder16.hip read the tables).
//
// The keys of a CSR order are non-decreasing, so a key change sits exactly at rowptr[r] of every non-empty row, and a part
// starts at every chunk boundary (a multiple of `span`) and at every key change.  With
//     c[r]  = rowptr[r + 1] > rowptr[r]  &&  rowptr[r] % span != 0        (a part start that is not a chunk start)
//     Cin   = inclusive scan of c,   Cex[r] = Cin[r] - c[r],   total = Cin[n_rows - 1]
// the part of entry p is  p / span + Cin[row(p)],  row(p) the row that holds p, hence
//     keys[p]        = row(p)
//     part_off[ch]   = ch + Cin[row(ch * span)]
//     part_rowptr[r] = p / span + Cex[r] + (p % span != 0)  with p = rowptr[r] < E,   last + 1  for p == E
//     last           = (E - 1) / span + total
// (an empty row takes the part of the next entry: the rows between are empty, their c is 0).
//
// Per call: one rocPRIM scan of n_rows flags read through a transform iterator, and one launch.  A workgroup expands the keys
// of 1024 consecutive entries at a time: two binary searches of rowptr find the rows of the tile's first and last entry, the
// rows between are read once, coalesced, and each non-empty one marks its first entry in LDS; a max-scan of the marks is the
// key of every entry.  A hub row costs its tiles two searches and no row reads, rows of one entry cost one rowptr read each:
// E * 4 bytes written, n_rows * 8 + tiles * 2 * log2(n_rows) * 8 read.  Integer sums, plain stores to distinct addresses.
//
// pangnn_csr_plan_tpos: the position words of the T kernel's stream route (decoder16.hip) from that order's perm and the
// keys above — tpos[p] = perm[p] | closes_p << 31, closes_p = [p + 1 == E  or  (p + 1) % span == 0  or  keys[p + 1] != keys[p]]:
// the edge id at position p and "a part ends behind p", which the kernel otherwise re-derives from three loads per position in
// every step.  One elementwise launch per graph, 4 bytes per edge kept.
//
// pangnn_csr_plan_spos: the same for the S kernel on a source-sorted list, which is its own by-source order — two words per
// position, spos[p] = { src_p | closes_p << 31, dst_p }, for the positions of whole 32-edge tiles: a position past the list
// repeats the last edge, and the last position of the last tile closes (so does every span-th position; the list's last
// edge itself only where one of the two says so — a wave carries its run to the end of the tile, the padding adds zeros).
// One elementwise launch per graph, 8 bytes per edge kept.
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include "common.h"

namespace pangnn {
namespace {

constexpr int kPlanTile = 4 * kBlock;           // entries per workgroup step: four consecutive ones per thread
constexpr int kPlanMaxBlocks = 2048;            // a memory-bound stream: 8 workgroups per CU, grid-stride the rest

// item r of the scan: row r starts a part inside a chunk
struct StartsInsideChunk {
  const int64_t* rowptr;
  int64_t span;
  __host__ __device__ int32_t operator()(int64_t r) const {
    const int64_t p = rowptr[r];
    return (rowptr[r + 1] > p && p % span != 0) ? 1 : 0;
  }
};

hipError_t scan_starts(void* temp, size_t& temp_bytes, StartsInsideChunk flag, int32_t* out, int64_t items, hipStream_t s) {
  auto in = rocprim::make_transform_iterator(rocprim::make_counting_iterator<int64_t>(0), flag);
  return rocprim::inclusive_scan(temp, temp_bytes, in, out, (size_t)items, rocprim::plus<int32_t>(), s);
}

size_t plan_scan_temp_bytes(int64_t items) {
  size_t b = 0;
  if (scan_starts(nullptr, b, StartsInsideChunk{nullptr, 32}, (int32_t*)nullptr, items, 0) != hipSuccess) return (size_t)-1;
  return b;
}

__global__ __launch_bounds__(kBlock) void csr_plan_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ cin, int64_t e, int64_t n, int64_t span,
    int32_t* __restrict__ keys, int32_t* __restrict__ part_off, int64_t* __restrict__ part_rowptr,
    int64_t* __restrict__ last_out) {
  __shared__ __attribute__((aligned(16))) int32_t mark[kPlanTile];
  __shared__ int32_t wave_top[kWavesPerBlock];
  __shared__ int32_t ends[2];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int64_t n_tiles = (e + kPlanTile - 1) / kPlanTile;
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int64_t q0 = t * kPlanTile;
    const int len = (int)(e - q0 < kPlanTile ? e - q0 : kPlanTile);
    if (tid < 2) ends[tid] = (int32_t)row_of_entry(rowptr, n, tid == 0 ? q0 : q0 + len - 1);   // n < 2^31
    reinterpret_cast<int4*>(mark)[tid] = make_int4(0, 0, 0, 0);
    __syncthreads();
    const int32_t lo = ends[0], hi = ends[1];
    // the non-empty rows that start inside the tile, behind its first entry: r in (lo, hi], all of them > 0
    for (int64_t r = (int64_t)lo + 1 + tid; r <= hi; r += kBlock) {
      const int64_t p = rowptr[r];
      const int64_t j = p - q0;
      if (rowptr[r + 1] > p && (uint64_t)j < (uint64_t)len) mark[j] = (int32_t)r;
    }
    __syncthreads();
    // running maximum of the marks, seeded with the row of the first entry
    int4 m = reinterpret_cast<int4*>(mark)[tid];
    m.y = max(m.x, m.y);
    m.z = max(m.y, m.z);
    m.w = max(m.z, m.w);
    int32_t run = m.w;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const int32_t up = __shfl_up(run, d, kWave);
      if (lane >= d) run = max(run, up);
    }
    if (lane == kWave - 1) wave_top[wave] = run;
    int32_t before = __shfl_up(run, 1, kWave);
    if (lane == 0) before = 0;
    __syncthreads();
    before = max(before, lo);
    for (int w = 0; w < wave; ++w) before = max(before, wave_top[w]);
    reinterpret_cast<int4*>(mark)[tid] = make_int4(max(m.x, before), max(m.y, before), max(m.z, before), max(m.w, before));
    __syncthreads();
    for (int j = tid; j < len; j += kBlock) keys[q0 + j] = mark[j];
    // the chunks that start inside the tile
    for (int64_t ch = (q0 + span - 1) / span + tid; ch * span < q0 + len; ch += kBlock)
      part_off[ch] = (int32_t)(ch + cin[mark[ch * span - q0]]);
    __syncthreads();
  }
  const int64_t total = cin[n - 1];
  const int64_t last = (e - 1) / span + total;
  const int64_t gtid = (int64_t)blockIdx.x * kBlock + tid, nthreads = (int64_t)gridDim.x * kBlock;
  if (gtid == 0) *last_out = last;
  for (int64_t r = gtid; r <= n; r += nthreads) {
    const int64_t p = rowptr[r];
    int64_t v = last + 1;
    if (p < e && r < n) {
      const int64_t rem = p % span;
      const int64_t cex = (int64_t)cin[r] - ((rowptr[r + 1] > p && rem != 0) ? 1 : 0);
      v = p / span + cex + (rem != 0 ? 1 : 0);
    }
    part_rowptr[r] = v;
  }
}

__global__ __launch_bounds__(kBlock) void csr_plan_tpos_kernel(const int32_t* __restrict__ perm, const int32_t* __restrict__ keys,
                                                              int64_t e, int64_t span, uint32_t* __restrict__ tpos) {
  const int64_t nthreads = (int64_t)gridDim.x * kBlock;
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < e; p += nthreads) {
    const int64_t q = p + 1;
    const bool closes = q == e || q % span == 0 || keys[q] != keys[p];
    tpos[p] = ((uint32_t)perm[p] & 0x7fffffffu) | (closes ? 0x80000000u : 0u);
  }
}

// p runs over the padded positions [0, 32 * ceil(e / 32)); a position past the list looks at the last edge
__global__ __launch_bounds__(kBlock) void csr_plan_spos_kernel(const int64_t* __restrict__ ei, int64_t ld, int64_t e, int64_t span,
                                                              uint2* __restrict__ spos) {
  const int64_t nthreads = (int64_t)gridDim.x * kBlock, padded = (e + 31) / 32 * 32;
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < padded; p += nthreads) {
    const int64_t q = p + 1, k = p < e ? p : e - 1;
    const int64_t src = ei[k];
    const bool closes = q == padded || q % span == 0 || (q < e && ei[q] != src);
    spos[p] = make_uint2(((uint32_t)src & 0x7fffffffu) | (closes ? 0x80000000u : 0u), (uint32_t)ei[ld + k]);
  }
}

}  // namespace
}  // namespace pangnn

using namespace pangnn;

extern "C" int pangnn_csr_plan_spos(const int64_t* edge_index, int64_t ld, int64_t num_edges, int32_t span, uint32_t* spos,
                                    pangnn_stream_t stream) {
  const char* name = "pangnn_csr_plan_spos";
  const int64_t e = num_edges;
  PG_CHECK_ARG(e >= 1 && ld >= e, PANGNN_E_BADARG, "%s: bad size (E=%lld, ld=%lld: at least one edge)", name, (long long)e,
               (long long)ld);
  PG_CHECK_ARG(e < ((int64_t)1 << 31) - 1, PANGNN_E_TOOLARGE, "%s: E must fit int32", name);
  PG_CHECK_ARG(span >= 32 && span % 32 == 0, PANGNN_E_BADARG, "%s: span %d is not a positive multiple of 32", name, (int)span);
  PG_CHECK_ARG(edge_index && spos, PANGNN_E_BADARG, "%s: null pointer", name);
  PG_CHECK_ARG((((uintptr_t)edge_index | (uintptr_t)spos) & 7u) == 0, PANGNN_E_ALIGN, "%s: a pointer is not 8-byte aligned", name);
  int64_t blocks = ((e + 31) / 32 * 32 + kBlock - 1) / kBlock;
  if (blocks > kPlanMaxBlocks) blocks = kPlanMaxBlocks;
  hipLaunchKernelGGL(csr_plan_spos_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, edge_index, ld, e,
                     (int64_t)span, reinterpret_cast<uint2*>(spos));
  PG_CHECK_LAUNCH(name);
  return 0;
}

extern "C" int pangnn_csr_plan_tpos(const int32_t* perm, const int32_t* keys, int64_t num_edges, int32_t span, uint32_t* tpos,
                                    pangnn_stream_t stream) {
  const char* name = "pangnn_csr_plan_tpos";
  const int64_t e = num_edges;
  PG_CHECK_ARG(e >= 1, PANGNN_E_BADARG, "%s: bad size (E=%lld: at least one edge)", name, (long long)e);
  PG_CHECK_ARG(e < ((int64_t)1 << 31) - 1, PANGNN_E_TOOLARGE, "%s: E must fit int32 (an edge id takes 31 bits of a word)", name);
  PG_CHECK_ARG(span >= 32 && span % 32 == 0, PANGNN_E_BADARG, "%s: span %d is not a positive multiple of 32", name, (int)span);
  PG_CHECK_ARG(perm && keys && tpos, PANGNN_E_BADARG, "%s: null pointer", name);
  PG_CHECK_ARG((((uintptr_t)perm | (uintptr_t)keys | (uintptr_t)tpos) & 3u) == 0, PANGNN_E_ALIGN,
               "%s: a pointer is not aligned to its element size", name);
  int64_t blocks = (e + kBlock - 1) / kBlock;
  if (blocks > kPlanMaxBlocks) blocks = kPlanMaxBlocks;
  hipLaunchKernelGGL(csr_plan_tpos_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, perm, keys, e,
                     (int64_t)span, tpos);
  PG_CHECK_LAUNCH(name);
  return 0;
}

// workspace layout: [Cin n_rows * 4][rocPRIM temp], each on 256 bytes
extern "C" int64_t pangnn_csr_plan_workspace_bytes(int64_t n_rows) {
  if (n_rows < 1 || n_rows >= ((int64_t)1 << 31)) return 0;
  const size_t t = plan_scan_temp_bytes(n_rows);
  if (t == (size_t)-1) return 0;
  return (int64_t)(align_up((size_t)n_rows * 4, 256) + align_up(t, 256));
}

extern "C" int pangnn_csr_plan(const int64_t* rowptr, int64_t n_rows, int64_t num_edges, int32_t span, int32_t* keys,
                               int32_t* part_off, int64_t* part_rowptr, int64_t* last, void* workspace,
                               int64_t workspace_bytes, pangnn_stream_t stream) {
  const char* name = "pangnn_csr_plan";
  const int64_t e = num_edges, n = n_rows;
  PG_CHECK_ARG(e >= 1 && n >= 1, PANGNN_E_BADARG, "%s: bad size (E=%lld rows=%lld: at least one of each)", name,
               (long long)e, (long long)n);
  PG_CHECK_ARG(e < ((int64_t)1 << 31) && n < ((int64_t)1 << 31), PANGNN_E_TOOLARGE,
               "%s: E and the number of rows must be below 2^31 (int32 keys and part ids)", name);
  PG_CHECK_ARG(span >= 32 && span % 32 == 0, PANGNN_E_BADARG, "%s: span %d is not a positive multiple of 32", name, (int)span);
  PG_CHECK_ARG(rowptr && keys && part_off && part_rowptr && last, PANGNN_E_BADARG, "%s: null pointer", name);
  PG_CHECK_ARG(workspace, PANGNN_E_BADARG, "%s: null workspace", name);
  PG_CHECK_ARG(aligned16(workspace), PANGNN_E_ALIGN, "%s: workspace must be 16-byte aligned", name);
  const uintptr_t p8 = (uintptr_t)rowptr | (uintptr_t)part_rowptr | (uintptr_t)last;
  const uintptr_t p4 = (uintptr_t)keys | (uintptr_t)part_off;
  PG_CHECK_ARG((p8 & 7u) == 0 && (p4 & 3u) == 0, PANGNN_E_ALIGN, "%s: a pointer is not aligned to its element size", name);
  const size_t temp = plan_scan_temp_bytes(n);
  PG_CHECK_ARG(temp != (size_t)-1, PANGNN_E_BADARG, "%s: rocPRIM size query failed", name);
  const size_t seg = align_up((size_t)n * 4, 256);
  PG_CHECK_ARG(workspace_bytes >= 0 && (size_t)workspace_bytes >= seg + align_up(temp, 256), PANGNN_E_WORKSPACE,
               "%s: workspace too small (%lld < %zu)", name, (long long)workspace_bytes, seg + align_up(temp, 256));
  char* ws = static_cast<char*>(workspace);
  int32_t* cin = reinterpret_cast<int32_t*>(ws);
  hipStream_t s = (hipStream_t)stream;
  size_t tb = align_up(temp, 256);
  const hipError_t err = scan_starts(ws + seg, tb, StartsInsideChunk{rowptr, span}, cin, n, s);
  PG_CHECK_ARG(err == hipSuccess, (int)err, "%s: scan failed: %s", name, hipGetErrorString(err));
  const int64_t n_tiles = (e + kPlanTile - 1) / kPlanTile, row_blocks = (n + kBlock) / kBlock;
  int64_t blocks = n_tiles > row_blocks ? n_tiles : row_blocks;
  if (blocks > kPlanMaxBlocks) blocks = kPlanMaxBlocks;
  hipLaunchKernelGGL(csr_plan_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, rowptr, cin, e, n, (int64_t)span, keys,
                     part_off, part_rowptr, last);
  PG_CHECK_LAUNCH(name);
  return 0;
}
