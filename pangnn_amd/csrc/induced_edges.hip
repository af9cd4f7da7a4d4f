// The induced similarity edges of per-group sub-graphs (pangnn_amd/subgraphs.py, step 3 of build_subgraphs;
// _induced_edges_index_ops there is the written definition and the referee).
//
// Rows are the (group, node) pairs of all sub-graphs in (group, local id) order: row r of group g (group_off[g] <= r <
// group_off[g + 1]) is global node v = row_node[r] with local id l = r - group_off[g].  For every row and every position p in
// [rowptr[v], rowptr[v + 1]), ascending, dst[p] is looked up in the group's node ids (sorted_node[group_off[g] ..), ascending,
// with their local ids beside them in sorted_local); found with local id m, the triple (l, m, p) is emitted.  Output order:
// rows in row order, positions ascending inside a row; duplicate (src, dst) entries of the relation are each emitted.
//
// The index-op route expands every out-edge of every row into four int64 columns and a searchsorted result before it drops
// the three in four whose target is outside the group.  Here nothing of that size exists: a count launch writes the hits of
// each row, one rocPRIM exclusive scan turns them into row offsets (row_off[rows] = total), and a fill launch repeats the
// walk and writes each hit behind its row's offset.  No atomics: inside a row a wave compacts its 64 positions by ballot and
// popcount prefix, so every store goes to an address that the inputs alone determine, and two calls give the same bytes.
//
// Work: a workgroup takes 512 consecutive rows at a time and walks the groups they belong to.  A group of at most kStage
// nodes is staged in LDS once per (task, group) as two int32 tables, 48 KiB, three workgroups per CU; a larger group is
// searched where it lies, in global memory, by the same code.  Each wave takes every fourth row of the segment and walks it
// 64 positions at a time: one coalesced 8-byte read of dst per lane, a branch-free lower bound, one ballot.  A hub row keeps
// its own wave busy for degree / 64 steps and no other wave waits for it before the segment ends — what a wave-per-row loop
// costs.  Positions and output addresses are 64-bit (the relation may hold more than 2^32 entries); node ids are staged as
// 32-bit words, hence num_nodes < 2^31.
#include <rocprim/device/device_scan.hpp>
#include "common.h"

namespace pangnn {
namespace {

constexpr int kStage = 6144;                    // node ids of a group held on chip: 2 x 4 bytes each
constexpr int kTaskRows = 512;                  // consecutive rows per workgroup step
constexpr int kInducedMaxBlocks = 2048;

struct InducedIn {
  const int64_t* rowptr;
  const int64_t* dst;
  int64_t n, e;
  const int64_t* row_node;
  int64_t rows;
  const int64_t* group_off;
  int64_t groups;
  const int64_t* sorted_node;
  const int64_t* sorted_local;
};

// index of `t` among the ascending keys[0, size), size >= 1, or -1: a lower bound whose step count depends on size alone
template <typename I, typename K>
__device__ __forceinline__ I find_sorted(const K* keys, I size, int64_t t) {
  I lo = 0, len = size;
  while (len > 1) {
    const I half = len >> 1;
    if ((int64_t)keys[lo + half - 1] < t) lo += half;
    len -= half;
  }
  if ((int64_t)keys[lo] < t) ++lo;
  return (lo < size && (int64_t)keys[lo] == t) ? lo : (I)-1;
}

// FILL false: cnt[r] = hits of row r.  FILL true: the hits of row r written at row_off[r] + (their rank inside the row).
template <bool FILL>
__global__ __launch_bounds__(kBlock) void induced_edges_kernel(InducedIn a, int64_t* __restrict__ cnt,
                                                              const int64_t* __restrict__ row_off, int64_t total,
                                                              int64_t* __restrict__ out_src, int64_t* __restrict__ out_dst,
                                                              int64_t* __restrict__ out_pos) {
  __shared__ int32_t s_node[kStage];
  __shared__ int32_t s_local[kStage];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const uint64_t below = ((uint64_t)1 << lane) - 1;
  const int64_t n_tasks = (a.rows + kTaskRows - 1) / kTaskRows;
  for (int64_t task = blockIdx.x; task < n_tasks; task += gridDim.x) {
    const int64_t r0 = task * kTaskRows;
    const int64_t r1 = r0 + kTaskRows < a.rows ? r0 + kTaskRows : a.rows;
    // every quantity that steers the two loops below is the same in all threads of the workgroup
    int64_t g = row_of_entry(a.group_off, a.groups, r0);
    for (int64_t r = r0; r < r1 && g < a.groups; ++g) {
      const int64_t gb = a.group_off[g], ge = a.group_off[g + 1];
      const int64_t s1 = ge < r1 ? ge : r1;
      if (s1 <= r) continue;                                   // a group without rows
      if (gb < 0 || gb > r || ge > a.rows) break;              // not an offset table: its rows keep a count of zero
      const int64_t size = ge - gb;
      const bool staged = size <= kStage;
      __syncthreads();                                         // the previous segment's lookups are done
      if (staged)
        for (int i = tid; i < (int)size; i += kBlock) {
          s_node[i] = (int32_t)a.sorted_node[gb + i];
          s_local[i] = (int32_t)a.sorted_local[gb + i];
        }
      __syncthreads();
      for (int64_t row = r + wave; row < s1; row += kWavesPerBlock) {
        const int64_t v = a.row_node[row];
        int64_t beg = 0, end = 0;
        if ((uint64_t)v < (uint64_t)a.n) {
          beg = a.rowptr[v];
          end = a.rowptr[v + 1];
        }
        if (beg < 0) beg = 0;
        if (end > a.e) end = a.e;
        int64_t base = FILL ? row_off[row] : 0;
        for (int64_t p0 = beg; p0 < end; p0 += kWave) {
          const int64_t p = p0 + lane;
          bool hit = false;
          int64_t m = 0;
          if (p < end) {
            const int64_t t = a.dst[p];
            if (staged) {
              const int i = find_sorted<int>(s_node, (int)size, t);
              hit = i >= 0;
              if (hit) m = s_local[i];
            } else {
              const int64_t i = find_sorted<int64_t>(a.sorted_node + gb, size, t);
              hit = i >= 0;
              if (hit) m = a.sorted_local[gb + i];
            }
          }
          const uint64_t hits = __ballot(hit);
          if (FILL && hit) {
            const int64_t at = base + __popcll(hits & below);
            if (at < total) {
              out_src[at] = row - gb;
              out_dst[at] = m;
              out_pos[at] = p;
            }
          }
          base += __popcll(hits);
        }
        if (!FILL && lane == 0) cnt[row] = base;
      }
      r = s1;
    }
  }
}

hipError_t scan_counts(void* temp, size_t& temp_bytes, const int64_t* cnt, int64_t* out, int64_t items, hipStream_t s) {
  return rocprim::exclusive_scan(temp, temp_bytes, cnt, out, (int64_t)0, (size_t)items, rocprim::plus<int64_t>(), s);
}

size_t induced_scan_temp_bytes(int64_t items) {
  size_t b = 0;
  if (scan_counts(nullptr, b, nullptr, nullptr, items, 0) != hipSuccess) return (size_t)-1;
  return b;
}

// the argument rules the two entry points share; sizes first, then pointers
int check_induced(const char* name, const InducedIn& a) {
  PG_CHECK_ARG(a.n >= 0 && a.e >= 0 && a.rows >= 0 && a.groups >= 0, PANGNN_E_BADARG,
               "%s: negative size (N=%lld E=%lld rows=%lld groups=%lld)", name, (long long)a.n, (long long)a.e,
               (long long)a.rows, (long long)a.groups);
  PG_CHECK_ARG(a.n < ((int64_t)1 << 31), PANGNN_E_TOOLARGE, "%s: num_nodes must be below 2^31 (node ids are staged as 32-bit words)",
               name);
  PG_CHECK_ARG(a.rows < ((int64_t)1 << 40) && a.groups < ((int64_t)1 << 40), PANGNN_E_TOOLARGE,
               "%s: more than 2^40 rows or groups", name);
  PG_CHECK_ARG(a.rows == 0 || a.groups > 0, PANGNN_E_BADARG, "%s: %lld rows in no group", name, (long long)a.rows);
  PG_CHECK_ARG(a.rows == 0 || a.n > 0, PANGNN_E_BADARG, "%s: %lld rows of a graph without nodes", name, (long long)a.rows);
  PG_CHECK_ARG(a.rows == 0 || (a.rowptr && a.row_node && a.group_off && a.sorted_node && a.sorted_local), PANGNN_E_BADARG,
               "%s: null table with rows > 0", name);
  PG_CHECK_ARG(a.e == 0 || a.rows == 0 || a.dst, PANGNN_E_BADARG, "%s: null dst with num_edges > 0", name);
  const uintptr_t p8 = (uintptr_t)a.rowptr | (uintptr_t)a.dst | (uintptr_t)a.row_node | (uintptr_t)a.group_off |
                       (uintptr_t)a.sorted_node | (uintptr_t)a.sorted_local;
  PG_CHECK_ARG((p8 & 7u) == 0, PANGNN_E_ALIGN, "%s: a table is not 8-byte aligned", name);
  return 0;
}

unsigned induced_grid(int64_t rows) {
  const int64_t tasks = blocks_for(rows, kTaskRows);
  return (unsigned)(tasks < 1 ? 1 : tasks > kInducedMaxBlocks ? kInducedMaxBlocks : tasks);
}

}  // namespace
}  // namespace pangnn

using namespace pangnn;

// scratch layout: [cnt (rows + 1) * 8][rocPRIM temp], each on 256 bytes
extern "C" int64_t pangnn_induced_edges_scratch_bytes(int64_t num_rows) {
  if (num_rows < 0 || num_rows >= ((int64_t)1 << 40)) return 0;
  const size_t t = induced_scan_temp_bytes(num_rows + 1);
  if (t == (size_t)-1) return 0;
  return (int64_t)(align_up((size_t)(num_rows + 1) * 8, 256) + align_up(t, 256));
}

extern "C" int pangnn_induced_edges_count(const int64_t* rowptr, const int64_t* dst, int64_t num_nodes, int64_t num_edges,
                                          const int64_t* row_node, int64_t num_rows, const int64_t* group_off,
                                          int64_t num_groups, const int64_t* sorted_node, const int64_t* sorted_local,
                                          int64_t* row_off, void* scratch, int64_t scratch_bytes, pangnn_stream_t stream) {
  const char* name = "pangnn_induced_edges_count";
  const InducedIn a{rowptr, dst, num_nodes, num_edges, row_node, num_rows, group_off, num_groups, sorted_node, sorted_local};
  if (const int rc = check_induced(name, a)) return rc;
  PG_CHECK_ARG(row_off, PANGNN_E_BADARG, "%s: null row_off", name);
  PG_CHECK_ARG(((uintptr_t)row_off & 7u) == 0, PANGNN_E_ALIGN, "%s: row_off is not 8-byte aligned", name);
  PG_CHECK_ARG(scratch, PANGNN_E_WORKSPACE, "%s: null scratch", name);
  PG_CHECK_ARG(aligned16(scratch), PANGNN_E_ALIGN, "%s: scratch must be 16-byte aligned", name);
  const size_t seg = align_up((size_t)(num_rows + 1) * 8, 256);
  PG_CHECK_ARG(scratch_bytes >= 0 && (size_t)scratch_bytes >= seg, PANGNN_E_WORKSPACE,
               "%s: scratch too small (%lld bytes do not hold %lld row counts)", name, (long long)scratch_bytes,
               (long long)num_rows + 1);
  const size_t temp = induced_scan_temp_bytes(num_rows + 1);
  PG_CHECK_ARG(temp != (size_t)-1, PANGNN_E_BADARG, "%s: rocPRIM size query failed", name);
  PG_CHECK_ARG((size_t)scratch_bytes >= seg + align_up(temp, 256), PANGNN_E_WORKSPACE, "%s: scratch too small (%lld < %zu)",
               name, (long long)scratch_bytes, seg + align_up(temp, 256));
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(scratch);
  int64_t* cnt = reinterpret_cast<int64_t*>(ws);
  // rows that no task reaches (an offset table that does not cover them) and the entry behind the last row count zero
  hipError_t err = hipMemsetAsync(cnt, 0, (size_t)(num_rows + 1) * 8, s);
  PG_CHECK_ARG(err == hipSuccess, (int)err, "%s: memset failed: %s", name, hipGetErrorString(err));
  if (num_rows > 0) {
    hipLaunchKernelGGL(induced_edges_kernel<false>, dim3(induced_grid(num_rows)), dim3(kBlock), 0, s, a, cnt,
                       (const int64_t*)nullptr, (int64_t)0, (int64_t*)nullptr, (int64_t*)nullptr, (int64_t*)nullptr);
    PG_CHECK_LAUNCH(name);
  }
  size_t tb = align_up(temp, 256);
  err = scan_counts(ws + seg, tb, cnt, row_off, num_rows + 1, s);
  PG_CHECK_ARG(err == hipSuccess, (int)err, "%s: scan failed: %s", name, hipGetErrorString(err));
  return 0;
}

extern "C" int pangnn_induced_edges_fill(const int64_t* rowptr, const int64_t* dst, int64_t num_nodes, int64_t num_edges,
                                         const int64_t* row_node, int64_t num_rows, const int64_t* group_off,
                                         int64_t num_groups, const int64_t* sorted_node, const int64_t* sorted_local,
                                         const int64_t* row_off, int64_t total, int64_t* out_src, int64_t* out_dst,
                                         int64_t* out_pos, pangnn_stream_t stream) {
  const char* name = "pangnn_induced_edges_fill";
  const InducedIn a{rowptr, dst, num_nodes, num_edges, row_node, num_rows, group_off, num_groups, sorted_node, sorted_local};
  if (const int rc = check_induced(name, a)) return rc;
  PG_CHECK_ARG(total >= 0, PANGNN_E_BADARG, "%s: negative total (%lld)", name, (long long)total);
  PG_CHECK_ARG(total == 0 || (num_rows > 0 && num_edges > 0), PANGNN_E_BADARG,
               "%s: %lld triples from %lld rows and %lld edges", name, (long long)total, (long long)num_rows, (long long)num_edges);
  if (total == 0) return 0;                                    // nothing to write
  PG_CHECK_ARG(row_off && out_src && out_dst && out_pos, PANGNN_E_BADARG, "%s: null row_off or output with total > 0", name);
  const uintptr_t p8 = (uintptr_t)row_off | (uintptr_t)out_src | (uintptr_t)out_dst | (uintptr_t)out_pos;
  PG_CHECK_ARG((p8 & 7u) == 0, PANGNN_E_ALIGN, "%s: row_off or an output is not 8-byte aligned", name);
  hipLaunchKernelGGL(induced_edges_kernel<true>, dim3(induced_grid(num_rows)), dim3(kBlock), 0, (hipStream_t)stream, a,
                     (int64_t*)nullptr, row_off, total, out_src, out_dst, out_pos);
  PG_CHECK_LAUNCH(name);
  return 0;
}
