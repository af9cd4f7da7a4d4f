/*
 * pangnn_hip.h — C ABI of libpangnn_hip.so, the MI355X (gfx950) implementation of panGNN's
 * edge-weighted message-passing hot path.
 *
 * Every entry point is plain C: device pointers + sizes + a hipStream_t passed as void*.
 * No torch types cross this boundary.  All pointers are DEVICE pointers unless stated otherwise.
 * Every call only ENQUEUES work on `stream` (no synchronisation, no allocation) and returns
 *   0                      on success,
 *   a positive hipError_t  if a HIP runtime call / launch failed,
 *   a negative PANGNN_E_*  on an argument error (nothing was launched).
 * `pangnn_last_error()` returns a thread-local human-readable message for the last non-zero return.
 *
 * The reference (fischer-hub/panGNN) is pure Python; the operator it calls for this path is the
 * third-party torch_geometric GCNConv.  Each function below cites the reference call site / PyG
 * stage it replaces (paths relative to /root/reference, stage names k1..k7 from SURVEY.md §2.2).
 */
#ifndef PANGNN_HIP_H
#define PANGNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 5): pangnn_decoder_train_f32 / _mixed / pangnn_decoder_dgrad_f32 took live_edges in round 4 and the 32-byte record
 * layout changed without a bump; pangnn_scale_unless_one_f32 added.  A library of another version is refused
 * by pangnn_amd/_lib.py and by libpangnn_torch.so when it resolves this ABI. */
/* 3 (round 5, later): PANGNN_DTYPE_F16 accepted by the node-level *_dtype arguments, pangnn_spmm_csr_f16 added; the 128 x 128
 * weight gradient is covered (pangnn_linear_supported(128, 128, 1) = 1). */
/* 3, extended: pangnn_linear_act_backward_parts_f32 added.  No entry point changed its signature or meaning, so the number
 * stays; the binding resolves every symbol at load, which refuses an older library of the same number.
 * Likewise pangnn_edge_dot_mixed, pangnn_gcn_norm_bwd_f32 and its _workspace_bytes (dL/d(edge_weight) of GCNConv), and
 * pangnn_qscore_fwd / pangnn_qscore_bwd with PANGNN_DTYPE_F64 (the differentiable Q-score edge weights), and
 * pangnn_csr_plan_tpos + pangnn_decoder_dgrad_stream_f32 (the T pass on one position word per edge), and
 * pangnn_csr_plan_spos + pangnn_decoder_train_stream_f32 / _mixed (the S pass on one word pair per position), and
 * pangnn_decoder_mlp_loss_live_f32 / pangnn_decoder_nd_loss_live_f32 / pangnn_edge_score_loss_live_mixed (the fused-loss
 * passes of the strict-fp32, node_dim 32 / 128 and cosine / dot decoders on a padded batch). */
#define PANGNN_ABI_VERSION 3

#define PANGNN_E_BADARG    (-1)  /* null pointer / negative size / unsupported feature width */
#define PANGNN_E_TOOLARGE  (-2)  /* size exceeds an int32 index range used by the kernels    */
#define PANGNN_E_WORKSPACE (-3)  /* workspace smaller than *_workspace_bytes() asked for     */
#define PANGNN_E_ALIGN     (-4)  /* pointer / leading dimension not 16-byte aligned          */

/* storage types of the *_mixed entry points: the arithmetic is fp32 either way, a matrix may be STORED as bfloat16 */
#define PANGNN_DTYPE_F32  0
#define PANGNN_DTYPE_BF16 1
#define PANGNN_DTYPE_F16  2   /* IEEE half rows (--mixed_precision fp16): accepted wherever a *_dtype argument accepts _BF16
                               * (dense layers, propagate gathers, generated rows, column sums, the decoder's P | Q tables); the
                               * 2-byte operands of one call are all bfloat16 or all float16. */
#define PANGNN_DTYPE_F64  3   /* float64 as stored: the *_dtype arguments of pangnn_qscore_fwd / pangnn_qscore_bwd only */

typedef void* pangnn_stream_t;   /* hipStream_t */

int         pangnn_abi_version(void);
const char* pangnn_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Graph structure (one-time per edge_index; replaces the implicit COO handling of
 * MessagePassing.propagate, src/gnn.py:158,165 -> PyG).
 *
 * Stable counting of a COO edge list edge_index[2][E] (row 0 = source j, row 1 = target i,
 * PyG flow 'source_to_target') into CSR grouped by `group_by`:
 *   group_by = 1: rows are TARGET nodes  (forward propagate,  out[i] += w * x[j])
 *   group_by = 0: rows are SOURCE nodes  (backward propagate, gx[j]  += w * g[i])
 * Outputs: rowptr[N+1] (int64), other[E] (int32: the opposite endpoint of every sorted edge),
 *          perm[E] (int32: original edge id of every sorted edge; stable => ascending in a row).
 * `ld` = element distance between row 0 and row 1 of edge_index (E when contiguous).
 * ---------------------------------------------------------------------------------------- */
size_t pangnn_csr_build_workspace_bytes(int64_t num_edges, int64_t num_nodes);
int    pangnn_csr_build(const int64_t* edge_index, int64_t ld, int64_t num_edges, int64_t num_nodes,
                        int group_by, int64_t* rowptr, int32_t* other, int32_t* perm,
                        void* workspace, size_t workspace_bytes, pangnn_stream_t stream);

/* Device address of the 4-byte validity flag of the last pangnn_csr_build that used `workspace`
 * (non-zero = some node id was outside [0, N) and was clamped).  Read it after synchronising. */
const void* pangnn_csr_build_flag_ptr(void* workspace, int64_t num_edges);

/* Small graphs — one mini-batch of sub-graphs (reference regime: DataLoader batches of 32 sub-graphs, pangnn.py:152-216,
 * collated by PyG's Batch): BOTH CSR orders of pangnn_csr_build (same stable order: identical rowptr / other / perm) and,
 * for each order, the int32 sorted keys and the run-sum plan over chunks of `chunk_edges` consecutive sorted positions
 * (the `part_off` / part row pointers the decoder's S / T kernels take, chunk_edges = 32 * pangnn_decoder_chunk_tiles_for(E)),
 * in ONE launch.  part_off_*[ceil(E / chunk_edges)], part_rowptr_*[N+1], last_part_*[1] = number of parts - 1.
 * bad_flag[0] (device) = 1 if a node id was outside [0, N) (clamped).  Limits: pangnn_structure_small_supported(E, N). */
int pangnn_structure_small_supported(int64_t num_edges, int64_t num_nodes);
int pangnn_structure_small(const int64_t* edge_index, int64_t ld, int64_t num_edges, int64_t num_nodes,
                           int32_t chunk_edges, int64_t* rowptr_dst, int32_t* other_dst, int32_t* perm_dst,
                           int32_t* keys_dst, int32_t* part_off_dst, int64_t* part_rowptr_dst, int64_t* last_part_dst,
                           int64_t* rowptr_src, int32_t* other_src, int32_t* perm_src, int32_t* keys_src,
                           int32_t* part_off_src, int64_t* part_rowptr_src, int64_t* last_part_src, int32_t* bad_flag,
                           pangnn_stream_t stream);

/* Collation of one mini-batch out of a flat sub-graph storage (the reference's DataLoader(batch_size=32) + PyG
 * Batch.from_data_list, pangnn.py:152-216; pangnn_amd/subgraphs.py): the batch is sub-graphs [i0, i0 + num_graphs), i.e.
 * nodes [n0, n0 + num_nodes), similarity edges [e0, e0 + num_edges) of edge_index[2][ld_e] and neighbour edges
 * [b0, b0 + num_nb) of nb_index[2][ld_b]; node_off points at entry i0 of the node offset table.  One launch writes the
 * batch-local lists out_edge_index[2][num_edges], out_nb_index[2][num_nb] (ids - n0), out_ptr[num_graphs + 1],
 * out_batch[num_nodes] (graph id of every node) and out_x[num_nodes] = 1 (the reference's node feature, dataset.py:369). */
int pangnn_collate_subgraphs(const int64_t* edge_index, int64_t ld_e, int64_t e0, int64_t num_edges,
                             const int64_t* nb_index, int64_t ld_b, int64_t b0, int64_t num_nb,
                             const int64_t* node_off, int32_t num_graphs, int64_t n0, int64_t num_nodes,
                             int64_t* out_edge_index, int64_t* out_nb_index, int64_t* out_ptr, int64_t* out_batch,
                             float* out_x, pangnn_stream_t stream);

/* Fixed-shape collation (train.ReplayedFreshStep: ONE captured HIP graph for every mini-batch of the reference's
 * DataLoader(batch_size=32, shuffle=True) loop, pangnn.py:152-216): the disjoint union of the sub-graphs whose ids are in the
 * DEVICE list graph_ids[max_graphs] (entries outside [0, num_graphs_total) are unused slots), in list order, written into
 * buffers of the fixed sizes max_edges / max_nb / max_nodes and padded with an inert tail: padded similarity and neighbour
 * edges are self loops of the padded nodes [n, max_nodes) — never real (max_nodes must exceed every batch's node count) —
 * spread evenly over them with non-decreasing ids (the lists stay source-sorted, the padding sorts last in both CSR orders
 * and no padded row is long), with weight 1 and label 0; out_ptr entries beyond the batch = n, out_batch of padded nodes =
 * g, out_x = 1.
 * node_off / edge_off / nb_off are the data set's [num_graphs_total + 1] offset tables (device); edge_attr / y its flat
 * per-edge arrays.  out_live[5] (device) = real similarity edges, neighbour edges, nodes, graphs, and 1 if the batch did
 * not fit (everything is then padding).  out_live is what the decoder entry points take as `live_edges`. */
/* One CSR order (by target / by source) of one edge list of a padded batch.  `rank` (in, per FLAT edge of the data set):
 * the edge's position among its own sub-graph's edges in this order (stable: equal keys keep list order) — a property of the
 * data set, computed once.  Outputs (device): rowptr [max_nodes + 1], other / perm / keys [max list length] as
 * pangnn_structure_small writes them; part_off / part_rowptr / last_part (nullable together): the run-sum plan of the order. */
typedef struct pangnn_batch_order {
  const int32_t* rank;
  int64_t* rowptr; int32_t* other; int32_t* perm; int32_t* keys;
  int32_t* part_off; int64_t* part_rowptr; int64_t* last_part;
} pangnn_batch_order;
/* `orders` of pangnn_collate_subgraphs_padded (nullable): also emit both CSR orders of both lists of the batch — without a
 * sort: sub-graph j's nodes all precede those of sub-graph j + 1, so the batch's order is the sub-graphs' own (static) orders
 * one after the other, sorted position = first edge of the sub-graph + rank; the padding is in order behind them.  The same
 * tables, entry for entry, as pangnn_structure_small on the collated lists (which costs a 70 us one-workgroup bitonic sort per
 * list).  chunk_edges: 32 * pangnn_decoder_chunk_tiles_for(max_edges).  Needs max_edges, max_nb, max_nodes within
 * pangnn_structure_small_supported. */
typedef struct pangnn_batch_orders {
  int32_t chunk_edges;
  pangnn_batch_order sim_dst, sim_src, nb_dst, nb_src;
} pangnn_batch_orders;
int pangnn_collate_subgraphs_padded(const int64_t* edge_index, int64_t ld_e, const int64_t* nb_index, int64_t ld_b,
                                    const float* edge_attr, const float* y, const int64_t* node_off,
                                    const int64_t* edge_off, const int64_t* nb_off, int64_t num_graphs_total,
                                    const int64_t* graph_ids, int32_t max_graphs, int64_t max_edges, int64_t max_nb,
                                    int64_t max_nodes, int64_t* out_edge_index, int64_t* out_nb_index,
                                    float* out_edge_attr, float* out_y, int64_t* out_ptr, int64_t* out_batch,
                                    float* out_x, int64_t* out_live, const pangnn_batch_orders* orders,
                                    pangnn_stream_t stream);
/* The same two collations in the --union_edge_weights layout (dataset.py:373-381): instead of a neighbour list of its own
 * the batch carries out_union_index[2][U] = [the batch's similarity edges | the batch's neighbour edges] and
 * out_edge_attr[U] = [similarity weights | ones], so out_edge_attr[0 .. E) stays aligned with out_edge_index.  Everything
 * else (out_edge_index, out_y, out_ptr, out_batch, out_x, out_live) is what the default-layout call writes.
 * pangnn_collate_subgraphs_union: U = num_edges + num_nb; edge_attr is the data set's flat weight array.
 * pangnn_collate_subgraphs_padded_union: U = max_edges + max_nb, union list = [real similarity edges | real neighbour edges
 * | padding of the same kind as above, spread over the padded nodes by U - real edges], weights = [real | ones]: the
 * first max_edges weights are the default layout's.  `orders` (nullable): both CSR orders of the similarity list with
 * their plans, as above, and both CSR orders of the union list (rowptr / other / perm / keys; the part_* fields are ignored:
 * only the decoder needs plans and it runs on the similarity list).  `rank` of a union order has ld_e + ld_b entries: for
 * flat similarity edge t entry t, for flat neighbour edge t entry ld_e + t — the edge's position in the stable by-key
 * order of ITS sub-graph's [similarity | neighbour] list.  Limits of `orders`: pangnn_collate_union_orders_supported
 * (max_edges within pangnn_structure_small_supported, max_edges + max_nb <= 32768: the walk reads keys from global
 * memory, so the one-workgroup sort's 16384 edges do not bound the union list). */
int pangnn_collate_subgraphs_union(const int64_t* edge_index, int64_t ld_e, int64_t e0, int64_t num_edges,
                                   const int64_t* nb_index, int64_t ld_b, int64_t b0, int64_t num_nb,
                                   const float* edge_attr, const int64_t* node_off, int32_t num_graphs, int64_t n0,
                                   int64_t num_nodes, int64_t* out_edge_index, int64_t* out_union_index,
                                   float* out_edge_attr, int64_t* out_ptr, int64_t* out_batch, float* out_x,
                                   pangnn_stream_t stream);
typedef struct pangnn_union_batch_orders {
  int32_t chunk_edges;
  pangnn_batch_order sim_dst, sim_src, union_dst, union_src;
} pangnn_union_batch_orders;
int pangnn_collate_union_orders_supported(int64_t max_edges, int64_t max_nb, int64_t max_nodes);
int pangnn_collate_subgraphs_padded_union(const int64_t* edge_index, int64_t ld_e, const int64_t* nb_index, int64_t ld_b,
                                          const float* edge_attr, const float* y, const int64_t* node_off,
                                          const int64_t* edge_off, const int64_t* nb_off, int64_t num_graphs_total,
                                          const int64_t* graph_ids, int32_t max_graphs, int64_t max_edges, int64_t max_nb,
                                          int64_t max_nodes, int64_t* out_edge_index, int64_t* out_union_index,
                                          float* out_edge_attr, float* out_y, int64_t* out_ptr, int64_t* out_batch,
                                          float* out_x, int64_t* out_live, const pangnn_union_batch_orders* orders,
                                          pangnn_stream_t stream);
/* dst[0 .. n) (device) = host_values[0 .. n), n <= 64, carried in the kernel arguments of one tiny launch: ordered with the
 * stream like any kernel and safe to call again before it ran (no pinned staging buffer to overwrite) — how the host hands
 * the next batch's sub-graph ids to a captured graph. */
int pangnn_set_i64(int64_t* dst, const int64_t* host_values, int32_t n, pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * gcn_norm (k1-k3; PyG gcn_norm as called by GCNConv.forward, src/gnn.py:158):
 *   deg[i]  = sum over in-edges of w        (w = 1 when edge_weight == NULL, src/gnn.py:165)
 *   dis[i]  = deg[i]^-1/2, 0 where deg == 0
 *   norm[e] = dis[src_e] * w_e * dis[dst_e]
 * Input structure is the target-grouped CSR from pangnn_csr_build(group_by=1).
 * Outputs: deg_inv_sqrt[N]; norm_sorted[E] in CSR order; norm_orig[E] in the caller's edge order
 * (nullable).  Deterministic: per-row sums run in ascending original edge id.
 * ---------------------------------------------------------------------------------------- */
int pangnn_gcn_norm_f32(const int64_t* rowptr_dst, const int32_t* src_sorted, const int32_t* perm_dst,
                        const float* edge_weight, int64_t num_nodes, int64_t num_edges,
                        float* deg_inv_sqrt, float* norm_sorted, float* norm_orig,
                        pangnn_stream_t stream);

/* The two stages of gcn_norm separately, for a destination-partitioned graph where the source
 * nodes' deg^-1/2 lives in another table (all-gathered from the other ranks): rows of the CSR are the
 * n_rows LOCAL targets, src_sorted holds GLOBAL source ids indexing dis_src. */
int pangnn_gcn_degree_f32(const int64_t* rowptr_dst, const int32_t* perm_dst, const float* edge_weight,
                          int64_t n_rows, float* deg_inv_sqrt, pangnn_stream_t stream);
int pangnn_gcn_edge_norm_f32(const int64_t* rowptr_dst, const int32_t* src_sorted, const int32_t* perm_dst,
                             const float* edge_weight, const float* dis_src, const float* dis_dst,
                             int64_t n_rows, int64_t num_edges, float* norm_sorted, float* norm_orig,
                             pangnn_stream_t stream);

/* out[i] = in[perm[i]]  (re-orders per-edge values into another CSR's order) */
int pangnn_permute_f32(const float* in, const int32_t* perm, float* out, int64_t n,
                       pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * propagate (k5+k6, and k5^T for backward; MessagePassing.propagate + GCNConv.message + 'add'
 * aggregation + bias, src/gnn.py:158,165):
 *   out[r, 0:F] (+)= bias[0:F] + sum_{e in [rowptr[r], rowptr[r+1])} val[e] * x[idx[e], 0:F]
 * val == NULL means 1.0; idx == NULL means the identity (row r sums x[rowptr[r] .. rowptr[r+1]));
 * bias == NULL means none; accumulate != 0 adds into `out`.
 * nnz = rowptr[n_rows] if known (a scheduling hint only: thin rows use a shallower unroll), else -1.
 * F in {16, 32, 64, 128, 256}; x/out/bias 16-byte aligned, ldx/ldo multiples of 4 floats.
 * No atomics: bitwise reproducible for a fixed structure.
 * ---------------------------------------------------------------------------------------- */
int pangnn_spmm_csr_f32(const int64_t* rowptr, const int32_t* idx, const float* val,
                        const float* x, int64_t ldx, int64_t n_src_rows,
                        const float* bias, float* out, int64_t ldo, int64_t n_rows,
                        int64_t nnz, int32_t F, int accumulate, pangnn_stream_t stream);
/* The same product with the gathered rows stored as bfloat16 (8 bytes per lane and row piece instead of 16): x is
 * [n_src_rows, ldx] bf16, 8-byte aligned; weights, accumulation, bias and the result are fp32.  This is what the
 * reference computes under `accelerate` bf16 mixed precision (PyG: bf16 x_j * fp32 edge weight -> fp32, scatter-add
 * into fp32), and the storage format SURVEY.md §8b lists for config 5.  F in {32, 64, 128, 256}. */
int pangnn_spmm_csr_bf16(const int64_t* rowptr, const int32_t* idx, const float* val, const void* x_bf16,
                         int64_t ldx, int64_t n_src_rows, const float* bias, float* out, int64_t ldo,
                         int64_t n_rows, int64_t nnz, int32_t F, int accumulate, pangnn_stream_t stream);
/* ... and as IEEE half (`--mixed_precision fp16`, /root/reference/src/setup.py:50: PyG's propagate under float16 autocast) */
int pangnn_spmm_csr_f16(const int64_t* rowptr, const int32_t* idx, const float* val, const void* x_f16,
                        int64_t ldx, int64_t n_src_rows, const float* bias, float* out, int64_t ldo,
                        int64_t n_rows, int64_t nnz, int32_t F, int accumulate, pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * edge decoder gather (k7; src/gnn.py:171-177):
 *   out[e, 0:D]   = z[src_e], out[e, D:2D] = z[dst_e], out[e, 2D] = extra[e] (if extra != NULL)
 * for e in [e_begin, e_begin + n_edges) of edge_index[2][ld]; out has leading dimension ldo.
 * ---------------------------------------------------------------------------------------- */
int pangnn_edge_gather_concat_f32(const float* z, int64_t ldz, int64_t num_nodes,
                                  const int64_t* edge_index, int64_t ld, int64_t e_begin,
                                  int64_t n_edges, const float* extra, float* out, int64_t ldo,
                                  int32_t D, pangnn_stream_t stream);

/* Re-associated first decoder layer: Linear(cat(z_s, z_d, w)) == P[s] + Q[d] + w*c with
 * P = z W_a^T, Q = z W_b^T + b (node-level GEMMs done by the caller).
 *   out[e, 0:D] = p[src_e] + q[dst_e] (+ extra[e] * cvec[0:D])
 * ---------------------------------------------------------------------------------------- */
int pangnn_edge_pair_add_f32(const float* p, const float* q, int64_t ldpq, int64_t num_nodes,
                             const int64_t* edge_index, int64_t ld, int64_t e_begin, int64_t n_edges,
                             const float* extra, const float* cvec, float* out, int64_t ldo,
                             int32_t D, pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Segment reductions over per-edge rows selected through a CSR permutation (backward of the edge
 * gathers above, and 'max' aggregation of src/convolution.py:7):
 *   sum : out[r, 0:F] (+)= sum_{k in row r} m[perm[k], col_off : col_off+F]   (m has n_m_rows rows)
 *   max : out[r, 0:F]   = max_{k in row r} m[perm[k], 0:F] (0 for empty rows), arg[r,f] = perm[k*]
 * ---------------------------------------------------------------------------------------- */
int pangnn_segment_sum_rows_f32(const int64_t* rowptr, const int32_t* perm, const float* m,
                                int64_t ldm, int64_t n_m_rows, int64_t col_off, float* out, int64_t ldo,
                                int64_t n_rows, int32_t F, int accumulate, pangnn_stream_t stream);
int pangnn_segment_max_rows_f32(const int64_t* rowptr, const int32_t* perm, const float* m,
                                int64_t ldm, float* out, int32_t* arg, int64_t ldo,
                                int64_t n_rows, int32_t F, pangnn_stream_t stream);
/* gm[arg[r,f], f] = g[r,f] for non-empty rows; gm must be zero-filled by the caller */
int pangnn_segment_max_bwd_f32(const float* g, const int32_t* arg, const int64_t* rowptr,
                               float* gm, int64_t ldm, int64_t ldo, int64_t n_rows, int32_t F,
                               pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused link decoder, node_dim D = 64 (k7 + the per-edge MLP, src/gnn.py:110-116,171-177):
 *   h1[e]   = relu(p[src_e] + q[dst_e] (+ extra[e] * cvec))     p = z W1[:, :D]^T, q = z W1[:, D:2D]^T + b1
 *   h2[e]   = relu(w2 h1[e] + b2)                               w2 [D,D] row-major [out][in]  (mlp.2)
 *   logits[e] = w3 . h2[e] + b3                                 w3 [D], b3 [1]                (mlp.4)
 * p and q are row-major with leading dimensions ldp / ldq (so both may be column windows of one
 * [N, 2D] product).  Edges are taken in the caller's order, e in [0, num_edges) of edge_index[2][ld].  No [E, D]
 * intermediate touches HBM in the forward pass.  fp32 MFMA (exact fp32 products and sums).
 *
 * Backward: given g_logits[E], recomputes the forward and returns
 *   g_h1[E, D] = dL/d(h1 pre-activation)  (the caller segment-sums it into g_p by source and g_q by
 *   target with pangnn_segment_sum_rows_f32), and the parameter gradients g_w2[D,D], g_b2[D],
 *   g_w3[D], g_b3[1], g_cvec[D] (nullable).  Reproducible: per-workgroup partial slabs in
 *   `workspace`, summed in a fixed order; no float atomics.
 *   part_buf / part_off (both NULL, or both set when the edge list is sorted by source): the kernel also
 *   sums the g_h1 rows of every (32-edge tile, source) run into part_buf[part, 0:D]; part_off[tile] is the
 *   index of the tile's first part, i.e. the number of k < 32*tile with k % 32 == 0 or src_k != src_{k-1}.
 *   g_p[s] is then the sum of the consecutive parts of source s (pangnn_spmm_csr_f32 with idx == NULL).
 *   precision: must be 0 here = every product on v_mfma_f32_32x32x2_f32 (exact fp32 FMA chains): the strict-fp32
 *              mode.  The bf16 matrix-pipe mode (fp32-level error, the default of the Python layer) is the
 *              pangnn_decoder_train_f32 + pangnn_decoder_dgrad_f32 pair below; it produces no [E, D] tensor.
 * ---------------------------------------------------------------------------------------- */
int pangnn_decoder_mlp_fwd_f32(const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t num_nodes,
                               const int64_t* edge_index, int64_t ld, int64_t num_edges,
                               const float* extra, const float* cvec, const float* w2, const float* b2,
                               const float* w3, const float* b3, int32_t D, float* logits,
                               pangnn_stream_t stream);
/* the same forward with the matrix-pipe mode of the training kernels (`precision`): 0 = f32 MFMA (bit-identical to
 * the logits of pangnn_decoder_mlp_loss_f32), 1 = bf16 matrix pipe with three-way split operands (fp32-level
 * error; bit-identical to the logits of pangnn_decoder_train_f32, about half the time of mode 0) */
int pangnn_decoder_mlp_infer_f32(const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t num_nodes,
                                 const int64_t* edge_index, int64_t ld, int64_t num_edges,
                                 const float* extra, const float* cvec, const float* w2, const float* b2,
                                 const float* w3, const float* b3, int32_t D, float* logits,
                                 int32_t precision, pangnn_stream_t stream);
/* one slab per workgroup of the launch over `num_edges` edges; the grid follows the edge count alone (at most 256), as for
 * the other widths of csrc/decoder.hip's template below */
size_t pangnn_decoder_mlp_bwd_workspace_bytes(int64_t num_edges);
int pangnn_decoder_mlp_bwd_f32(const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t num_nodes,
                               const int64_t* edge_index, int64_t ld, int64_t num_edges,
                               const float* extra, const float* cvec, const float* w2, const float* b2,
                               const float* w3, const float* b3, int32_t D, const float* g_logits,
                               float* g_h1, float* g_w2, float* g_b2, float* g_w3, float* g_b3,
                               float* g_cvec, float* part_buf, const int32_t* part_off, int32_t precision,
                               void* workspace, size_t workspace_bytes, pangnn_stream_t stream);

/* Training form of the decoder: logits, BCEWithLogits(pos_weight) mean loss (denominator `denom`) AND every
 * gradient in ONE pass over the edges — the logits of a tile come out of the backward's recomputed first
 * product, so forward + criterion + backward (pangnn.py:200-207) do not need three kernels and the
 * forward's product is not computed twice.  Outputs as pangnn_decoder_mlp_bwd_f32 plus logits[E], loss[1];
 * all gradients are those of `loss` (upstream gradient 1). */
int pangnn_decoder_mlp_loss_f32(const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t num_nodes,
                                const int64_t* edge_index, int64_t ld, int64_t num_edges, const float* extra,
                                const float* cvec, const float* w2, const float* b2, const float* w3,
                                const float* b3, int32_t D, const float* y, const float* pos_weight,
                                int64_t denom, float* logits, float* loss, float* g_h1, float* g_w2,
                                float* g_b2, float* g_w3, float* g_b3, float* g_cvec, float* part_buf,
                                const int32_t* part_off, int32_t precision, void* workspace,
                                size_t workspace_bytes, pangnn_stream_t stream);
/* ... of a fixed-shape padded batch: live_edges (DEVICE int64[1], required) as described under `live_edges` below — the first
 * m = min(max(*live_edges, 0), num_edges) edges are real, the loss is their mean (`denom` is ignored) and the padding enters
 * no sum.  Every other argument, the workspace and the return codes as pangnn_decoder_mlp_loss_f32; the workspace size is
 * passed as an int64_t, as in the nd family (a negative one: PANGNN_E_WORKSPACE). */
int pangnn_decoder_mlp_loss_live_f32(const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t num_nodes,
                                     const int64_t* edge_index, int64_t ld, int64_t num_edges, const float* extra,
                                     const float* cvec, const float* w2, const float* b2, const float* w3,
                                     const float* b3, int32_t D, const float* y, const float* pos_weight,
                                     int64_t denom, float* logits, float* loss, float* g_h1, float* g_w2,
                                     float* g_b2, float* g_w3, float* g_b3, float* g_cvec, float* part_buf,
                                     const int32_t* part_off, int32_t precision, const int64_t* live_edges,
                                     void* workspace, int64_t workspace_bytes, pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The same fused link decoder for node_dim D in {32, 128} (`--node_dim`, src/setup.py:38): two more instances of the width
 * template in csrc/decoder.hip that the entry points above run at D = 64 with precision 0, i.e. the strict-fp32 formulation
 * above (every product on v_mfma_f32_32x32x2_f32, per-workgroup slabs summed in index order, no float atomics) with the
 * width as a parameter.  Arguments, outputs, the part_buf / part_off layout (one 32-edge tile per chunk)
 * and the order of the return codes are those of pangnn_decoder_mlp_fwd_f32 / _bwd_f32 / _loss_f32 without `precision`;
 * p, q and g_h1 rows and the part rows are D floats wide, ldp / ldq >= D.  The launch grid follows the edge count alone, so
 * a result does not depend on the device's size.  pangnn_decoder_nd_supported(D): 1 for 32 and 128, 0 for every other
 * width, 64 included (that one stays with the entry points above, which keep rejecting D != 64); an unsupported D here:
 * PANGNN_E_BADARG.  Workspace: pangnn_decoder_nd_bwd_workspace_bytes(D, num_edges) (0 for an unsupported D); its size is
 * passed as an int64_t, like every other size of these entry points (a negative one: PANGNN_E_WORKSPACE).
 * ---------------------------------------------------------------------------------------- */
int pangnn_decoder_nd_supported(int32_t D);
int pangnn_decoder_nd_fwd_f32(const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t num_nodes,
                              const int64_t* edge_index, int64_t ld, int64_t num_edges,
                              const float* extra, const float* cvec, const float* w2, const float* b2,
                              const float* w3, const float* b3, int32_t D, float* logits,
                              pangnn_stream_t stream);
size_t pangnn_decoder_nd_bwd_workspace_bytes(int32_t D, int64_t num_edges);
int pangnn_decoder_nd_bwd_f32(const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t num_nodes,
                              const int64_t* edge_index, int64_t ld, int64_t num_edges,
                              const float* extra, const float* cvec, const float* w2, const float* b2,
                              const float* w3, const float* b3, int32_t D, const float* g_logits,
                              float* g_h1, float* g_w2, float* g_b2, float* g_w3, float* g_b3,
                              float* g_cvec, float* part_buf, const int32_t* part_off,
                              void* workspace, int64_t workspace_bytes, pangnn_stream_t stream);
int pangnn_decoder_nd_loss_f32(const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t num_nodes,
                               const int64_t* edge_index, int64_t ld, int64_t num_edges, const float* extra,
                               const float* cvec, const float* w2, const float* b2, const float* w3,
                               const float* b3, int32_t D, const float* y, const float* pos_weight,
                               int64_t denom, float* logits, float* loss, float* g_h1, float* g_w2,
                               float* g_b2, float* g_w3, float* g_b3, float* g_cvec, float* part_buf,
                               const int32_t* part_off, void* workspace, int64_t workspace_bytes,
                               pangnn_stream_t stream);
/* ... of a fixed-shape padded batch (live_edges required, `denom` ignored): see pangnn_decoder_mlp_loss_live_f32 */
int pangnn_decoder_nd_loss_live_f32(const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t num_nodes,
                                    const int64_t* edge_index, int64_t ld, int64_t num_edges, const float* extra,
                                    const float* cvec, const float* w2, const float* b2, const float* w3,
                                    const float* b3, int32_t D, const float* y, const float* pos_weight,
                                    int64_t denom, float* logits, float* loss, float* g_h1, float* g_w2,
                                    float* g_b2, float* g_w3, float* g_b3, float* g_cvec, float* part_buf,
                                    const int32_t* part_off, const int64_t* live_edges, void* workspace,
                                    int64_t workspace_bytes, pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Two-wave-per-SIMD training decoder (csrc/decoder16.hip) — what `precision = 1` training uses.
 * Replaces forward + criterion + backward of src/gnn.py:171-177 / pangnn.py:200-207 with TWO passes and
 * no [E, D] tensor:
 *
 * pangnn_decoder_train_f32  ("S"): one pass over the edges in the caller's order.  Exactly one of
 *   y        (fused loss: logits[E], loss[1] = mean BCEWithLogits(pos_weight) over `denom` edges are outputs and
 *             dL/dlogit is produced in place), or
 *   g_logits (given dL/dlogits[E]; logits nullable)
 *   is set.  Outputs: the parameter gradients g_w2[D,D], g_w3[D], g_b3[1], g_cvec[D] (nullable) — dL/db2 comes
 *   out of the dgrad pass (it needs only the records; keeping its per-lane partial sums out of this kernel is
 *   what lets two waves share a SIMD without spilling),
 *   rec[E][8] uint32 (required): per edge {4 dwords of relu masks — the h2 mask in the low byte of each half, the h1
 *             mask in the high byte —, dL/dlogit_e replicated into dwords 4 .. 7} for the dgrad pass, whose lane group g
 *             reads mask dword g and dL/dlogit through one address (offsets 0 and 16).  The value is the one given (or, with
 *             the fused loss, computed as for a real edge) also where the edge is padding (live_edges): S leaves such an edge
 *             out of its own sums, its record is not zeroed — T masks by position in its order,
 *   part_buf / part_off (both NULL or both set; edge list sorted by source): sums of dL/dh1 over every
 *   (chunk, source) run, where a chunk is pangnn_decoder_chunk_tiles_for(num_edges) (16 for E >= 1e6, down to 1 for short lists) consecutive 32-edge tiles walked by
 *   one wave with the open run carried from tile to tile: part_off[c] = index of chunk c's first part row, a new
 *   part starts at every chunk start and at every change of the key (pangnn_decoder_mlp_bwd_f32 uses the same layout
 *   with one-tile chunks).  Chunks are a property of the edge list, not of the launch: results do not depend on the
 *   grid.
 *   Arithmetic: every product on the bf16 matrix pipe with fp32 accumulation and fp32-exact operand handling —
 *   W2 h1 with both operands split into three bf16 terms (6 partial products); dL/dh1 = m1 g_e (m2^T W2') and
 *   dL/dW2 = diag(w3) m2 (g_e h1) with the relu mask m2 as the EXACT bf16 operand and the other operand split
 *   three ways.  The last tile is padded by clamping edge ids (one tile body, no divergent matrix operands).
 *   workspace: pangnn_decoder_train_workspace_bytes().
 * pangnn_decoder_train_stream_f32 / _mixed: the same pass and the same results, bit for bit, for a source-sorted list given
 *   as ONE 8-byte word pair per position, spos[k] = { src_k | closes_k << 31, dst_k } (pangnn_csr_plan_spos below: built once
 *   per graph) in place of edge_index: one id load per position instead of three, row offsets by shifts, no per-step key
 *   compares.  spos, part_buf and part_off are required (num_edges > 0); ldp and ldq times the element size must be powers
 *   of two (PANGNN_E_BADARG otherwise: such tables take pangnn_decoder_train_*); every edge is real (no live_edges).
 *
 * pangnn_decoder_dgrad_f32  ("T"): dL/dh1 summed over runs of equal keys in a permuted edge order, from `rec`:
 *   position k of the order is edge perm[k] (NULL = identity) with run key keys[k] (non-decreasing, e.g. the
 *   target id in by-target CSR order); part_buf / part_off as above for THIS order.  dL/dQ[t] is then the sum
 *   of the consecutive parts of target t (pangnn_spmm_csr_f32 with idx == NULL).  (dL/dcvec always comes out of
 *   pangnn_decoder_train_*; round 3's instances that recomputed it here were never launched and are gone.)
 *   g_b2[D] (nullable) = dL/db2 = w3[j] sum_e g_e [h2[j][e] > 0] — ask for it in exactly one dgrad call per step.
 *   part_buf / part_off / keys may all be NULL to get the parameter sum alone.  workspace (with g_b2):
 *   pangnn_decoder_dgrad_workspace_bytes().
 * pangnn_decoder_dgrad_stream_f32: the same pass and the same results, bit for bit, for an order given as ONE word per
 *   position, tpos[k] = perm[k] | closes_k << 31 (pangnn_csr_plan_tpos below: built once per graph) in place of perm and
 *   keys: one load per position instead of three, no per-step key compares.  tpos, part_buf and part_off are required
 *   (num_edges > 0); every edge is real (no live_edges: a padded batch takes pangnn_decoder_dgrad_f32).
 * live_edges (pangnn_decoder_train_* and pangnn_decoder_dgrad_f32; nullable, DEVICE int64[1]): the list is a fixed-shape batch whose first *live_edges edges
 *   are real and whose tail is padding (a mini-batch collated by pangnn_collate_subgraphs_padded so that one captured
 *   HIP graph serves every batch): in S the padded edges keep their own logit / record slots but enter every sum with
 *   dL/dlogit = 0 (the record itself keeps the unmasked value, see `rec`) and the fused loss is the mean over *live_edges
 *   edges (`denom` is ignored); in T the positions >= *live_edges of the order are the padding and contribute 0 whatever
 *   their records hold (the pads must sort last: their endpoints are the largest node id).  A value above num_edges counts
 *   as num_edges.  NULL: every edge is real.
 *   The one-pass fused-loss kernels of the other decoders take the same count through entry points of their own, where it is
 *   required: pangnn_decoder_mlp_loss_live_f32 / pangnn_decoder_nd_loss_live_f32 (strict fp32, node_dim 64 / 32 and 128) and
 *   pangnn_edge_score_loss_live_mixed (cosine / dot).  With m = min(max(*live_edges, 0), num_edges): logits are written for all
 *   num_edges positions; dL/dlogit of an edge k >= m is exactly 0, so its dL/dh1 row (strict fp32) is a zero row and it adds
 *   zeros to every parameter sum, run part and node row; loss and dL/dlogit[0:m] use 1.0f / (float)max(m, 1) (`denom` is
 *   ignored); m == 0 gives loss 0 and all-zero gradients.  The tables the padded edges gather must be finite.
 * Both are reproducible (fixed-order sums, no float atomics).
 * ---------------------------------------------------------------------------------------- */
int    pangnn_decoder_chunk_tiles(void);
/* ... as a function of the list: pangnn_decoder_chunk_tiles() (16) for lists of >= 2048 * 16 tiles, halved until the list
 * has at least 2048 chunks (1 for a mini-batch): the S / T kernels derive the same value from num_edges, and `part_off` /
 * `part_buf` must be laid out for it. */
int    pangnn_decoder_chunk_tiles_for(int64_t num_edges);
size_t pangnn_decoder_train_workspace_bytes(void);
int pangnn_decoder_train_f32(const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t num_nodes,
                             const int64_t* edge_index, int64_t ld, int64_t num_edges, const float* extra,
                             const float* cvec, const float* w2, const float* b2, const float* w3,
                             const float* b3, int32_t D, const float* y, const float* pos_weight,
                             int64_t denom, const float* g_logits, float* logits, float* loss, uint32_t* rec,
                             float* part_buf, const int32_t* part_off, float* g_w2, float* g_w3, float* g_b3,
                             float* g_cvec, const int64_t* live_edges, void* workspace, size_t workspace_bytes,
                             pangnn_stream_t stream);
/* bf16-storage mode of the gather (config 5, bf16 mixed precision: mlp[0] is an autocast Linear, src/gnn.py:173, so
 * its node-level halves P and Q are bf16 tensors): pq_dtype = PANGNN_DTYPE_BF16 reads p and q as bfloat16 rows
 * (ldp / ldq in elements, multiples of 8; half the gather bytes).  bf16 -> f32 is exact, so logits, loss and all
 * gradients equal, bit for bit, those of the f32 entry points on the up-converted tables.  Gradients stay fp32.
 * pangnn_decoder_train_f32 / the precision-1 pangnn_decoder_mlp_infer_f32 are these with PANGNN_DTYPE_F32. */
int pangnn_decoder_train_mixed(const void* p, int64_t ldp, const void* q, int64_t ldq, int32_t pq_dtype,
                               int64_t num_nodes, const int64_t* edge_index, int64_t ld, int64_t num_edges,
                               const float* extra, const float* cvec, const float* w2, const float* b2,
                               const float* w3, const float* b3, int32_t D, const float* y, const float* pos_weight,
                               int64_t denom, const float* g_logits, float* logits, float* loss, uint32_t* rec,
                               float* part_buf, const int32_t* part_off, float* g_w2, float* g_w3, float* g_b3,
                               float* g_cvec, const int64_t* live_edges, void* workspace, size_t workspace_bytes,
                               pangnn_stream_t stream);
int pangnn_decoder_train_stream_f32(const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t num_nodes,
                                    const uint32_t* spos, int64_t num_edges, const float* extra, const float* cvec,
                                    const float* w2, const float* b2, const float* w3, const float* b3, int32_t D,
                                    const float* y, const float* pos_weight, int64_t denom, const float* g_logits,
                                    float* logits, float* loss, uint32_t* rec, float* part_buf, const int32_t* part_off,
                                    float* g_w2, float* g_w3, float* g_b3, float* g_cvec, void* workspace,
                                    int64_t workspace_bytes, pangnn_stream_t stream);
int pangnn_decoder_train_stream_mixed(const void* p, int64_t ldp, const void* q, int64_t ldq, int32_t pq_dtype,
                                      int64_t num_nodes, const uint32_t* spos, int64_t num_edges, const float* extra,
                                      const float* cvec, const float* w2, const float* b2, const float* w3, const float* b3,
                                      int32_t D, const float* y, const float* pos_weight, int64_t denom,
                                      const float* g_logits, float* logits, float* loss, uint32_t* rec, float* part_buf,
                                      const int32_t* part_off, float* g_w2, float* g_w3, float* g_b3, float* g_cvec,
                                      void* workspace, int64_t workspace_bytes, pangnn_stream_t stream);
int pangnn_decoder_mlp_infer_mixed(const void* p, int64_t ldp, const void* q, int64_t ldq, int32_t pq_dtype,
                                   int64_t num_nodes, const int64_t* edge_index, int64_t ld, int64_t num_edges,
                                   const float* extra, const float* cvec, const float* w2, const float* b2,
                                   const float* w3, const float* b3, int32_t D, float* logits,
                                   pangnn_stream_t stream);
size_t pangnn_decoder_dgrad_workspace_bytes(void);
int pangnn_decoder_dgrad_f32(const uint32_t* rec, const int32_t* perm, const int32_t* keys, const float* w2,
                             const float* w3, int64_t num_edges, float* part_buf, const int32_t* part_off, float* g_b2,
                             const int64_t* live_edges, void* workspace, size_t workspace_bytes, pangnn_stream_t stream);
int pangnn_decoder_dgrad_stream_f32(const uint32_t* rec, const uint32_t* tpos, const float* w2, const float* w3,
                                    int64_t num_edges, float* part_buf, const int32_t* part_off, float* g_b2,
                                    void* workspace, int64_t workspace_bytes, pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Node-level dense layers with a short inner dimension, K (in) and M (out) in {64, 128}
 * (GCNConv.lin = k4 of SURVEY.md §2.2, the decoder's node-level P|Q product, and their backward):
 *   fwd  : y[n, 0:M]  = x[n, 0:K] . w[M,K]^T (+ bias[M])          (dL/dx = g . w is fwd with w^T)
 *   wgrad: gw[M,K]    = g[N,M]^T . x[N,K],  gb[M] = sum_n g[n,:]  (gb nullable)
 * fp32 storage and accumulation; the products run on the bf16 matrix pipe with both operands split into three exact
 * bf16 terms (six partial products: the error against an fp64 evaluation is that of an fp32 FMA chain; every
 * supported shape keeps its three split weight images in LDS, there is no other product to fall back on; the 128 x 128
 * weight gradient runs as two 64-column halves of g).  HBM-bound streaming kernels; wgrad is slab-reduced (reproducible).
 * pangnn_linear_supported(K, M, wgrad) tells the caller whether a shape is covered.
 * ---------------------------------------------------------------------------------------- */
int    pangnn_linear_supported(int32_t K, int32_t M, int wgrad);
int    pangnn_linear_fwd_f32(const float* x, int64_t ldx, const float* w, const float* bias, float* y,
                             int64_t ldy, int64_t n, int32_t K, int32_t M, pangnn_stream_t stream);
size_t pangnn_linear_wgrad_workspace_bytes(int32_t K, int32_t M);
int    pangnn_linear_wgrad_f32(const float* g, int64_t ldg, const float* x, int64_t ldx, int64_t n,
                               int32_t K, int32_t M, float* gw, float* gb, void* workspace,
                               size_t workspace_bytes, pangnn_stream_t stream);
/* The same layers with the encoder's activation folded in (src/gnn.py:108,129-166: h = ELU(conv(...)) is always
 * followed by exactly one dense layer — GCNConv.lin of the next conv, linear_out, or mlp[0] — so ELU(x) never has
 * to exist in HBM, and neither does its backward pass as a kernel of its own):
 *   act_fwd   in_act = 1 : y = ELU(x) . w^T (+ bias)          (x is the PRE-activation; alpha = 1)
 *             gate != NULL: y = (x . w^T) * ELU'(gate[n, 0:M]) — dL/d(pre-activation) straight from the dL/dx
 *                           product of the following layer (gate = that pre-activation); excludes in_act
 *   act_wgrad in_act = 1 : gw = g^T . ELU(x)
 * in_act = 0, gate = NULL are the plain entry points above. */
int    pangnn_linear_act_fwd_f32(const float* x, int64_t ldx, const float* w, const float* bias, float* y,
                                 int64_t ldy, int64_t n, int32_t K, int32_t M, int32_t in_act,
                                 const float* gate, int64_t ldgate, pangnn_stream_t stream);
int    pangnn_linear_act_wgrad_f32(const float* g, int64_t ldg, const float* x, int64_t ldx, int64_t n,
                                   int32_t K, int32_t M, int32_t in_act, float* gw, float* gb,
                                   void* workspace, size_t workspace_bytes, pangnn_stream_t stream);
/* bf16-storage modes (config 5: `accelerate` bf16 mixed precision, pangnn.py:25 — the reference's autocast Linear
 * layers, src/gnn.py:93,111,173, hand bf16 tensors to the next layer).  x / y / gate / g may each be stored as
 * bfloat16 (PANGNN_DTYPE_*; ld in ELEMENTS; rows start on 8 bytes); products and sums are the same exact-fp32 MFMA
 * chains as above, a bf16 result is rounded to nearest even once, on store.  w, bias, gw, gb stay fp32 (the
 * parameters are fp32 under autocast).  A gated product is the gradient of its gate tensor and is stored like it:
 * gate_dtype must equal y_dtype.  The *_f32 entry points are these with every dtype = PANGNN_DTYPE_F32. */
int    pangnn_linear_act_fwd_mixed(const void* x, int32_t x_dtype, int64_t ldx, const float* w, const float* bias,
                                   void* y, int32_t y_dtype, int64_t ldy, int64_t n, int32_t K, int32_t M,
                                   int32_t in_act, const void* gate, int32_t gate_dtype, int64_t ldgate,
                                   pangnn_stream_t stream);
int    pangnn_linear_act_wgrad_mixed(const void* g, int32_t g_dtype, int64_t ldg, const void* x, int32_t x_dtype,
                                     int64_t ldx, int64_t n, int32_t K, int32_t M, int32_t in_act, float* gw,
                                     float* gb, void* workspace, size_t workspace_bytes, pangnn_stream_t stream);
/* dL/dx of the dense layer y = act(x) . w^T straight from the layer's own weight w [M][K] row-major (the kernel stages w
 * through the strides of its transpose — no transposed copy of w per step, one launch less in a launch-bound mini-batch step):
 *   gx [n][K] = g [n][M] . w   (* ELU'(gate[n, 0:K]) when gate != NULL: dL/d(pre-activation), as act_fwd's gate)
 * Storage types / alignment as pangnn_linear_act_fwd_mixed with x = g, y = gx.  (autograd of nn.Linear / GCNConv.lin:
 * src/gnn.py:104,110-116; pangnn.py:207.) */
int    pangnn_linear_dgrad_mixed(const void* g, int32_t g_dtype, int64_t ldg, const float* w, void* gx, int32_t gx_dtype,
                                 int64_t ldgx, int64_t n, int32_t K, int32_t M, const void* gate, int32_t gate_dtype,
                                 int64_t ldgate, pangnn_stream_t stream);
/* Backward of the decoder's P | Q layer y = act(x) . w^T + b (K = 64, M = 128) straight from the run parts the S and T
 * kernels leave behind — the [n, 128] gradient dL/dP | dL/dQ is never written:
 *   G[r][0:64)   = sum of parts_s[rowptr_s[r] .. rowptr_s[r+1]),  G[r][64:128) = the same over parts_t
 *   gx [n][64] = (G . w) * ELU'(x) (in_act = 1; G . w for 0),  gw [128][64] = G^T . act(x),  gb [128] = column sums of G.
 * One launch (+ the slab reduction) in place of two pangnn_spmm_csr_f32 part sums, pangnn_linear_dgrad_mixed and
 * pangnn_linear_act_wgrad_mixed, and equal to that sequence bit for bit: same row sums in part order, same products, same
 * tile-to-wave assignment and slab order.  parts_* [n_parts_*, 64] contiguous f32, rowptr_* int64 [n + 1] absolute part
 * positions; x [n, 64] f32 is the layer's input (pre-activation when in_act = 1); workspace as
 * pangnn_linear_wgrad_workspace_bytes(64, 128), its size passed as int64_t like every other size of this call.  Part positions
 * outside [0, n_parts) are skipped, not read. */
int    pangnn_linear_act_backward_parts_f32(const float* parts_s, const int64_t* rowptr_s, int64_t n_parts_s,
                                            const float* parts_t, const int64_t* rowptr_t, int64_t n_parts_t,
                                            const float* x, int64_t ldx, const float* w, int64_t n, int32_t K, int32_t M,
                                            int32_t in_act, float* gx, int64_t ldgx, float* gw, float* gb,
                                            void* workspace, int64_t workspace_bytes, pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Confusion counts of thresholded link predictions, accumulated on the device:
 *   counts[2*label + prediction] += 1,  prediction = (score >= threshold),
 *   score = sigmoid(scores[i]) if apply_sigmoid else scores[i];  label = labels[i] > 0.5.
 * Replaces  probabilities = torch.sigmoid(output); (probabilities >= binary_th).int();
 *           BinaryConfusionMatrix.update(prediction, labels)      (pangnn.py:218-222, 257-262)
 * counts = {tn, fp, fn, tp} (torchmetrics layout [[tn, fp], [fn, tp]]), int64, caller-zeroed, never reset here.
 * ---------------------------------------------------------------------------------------- */
int    pangnn_confusion_update_f32(const float* scores, const float* labels, int64_t n, float threshold,
                                   int apply_sigmoid, int64_t* counts, pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Everything an epoch keeps of ONE batch's logits, folded into device state by one capturable call: no host read-back, no
 * allocation, no synchronisation, no float atomics — the same input gives the same bits in every run.
 * (pangnn.py:218-222: running training loss + training confusion matrix; pangnn.py:241-289: the validation loop.)
 *
 *   m = live[0], the number of real entries of a padded batch (device int64; NULL: n_max; a value outside [0, n_max]: n_max).
 *   Only logits[0:m] / labels[0:m] are read.  m == 0 adds nothing and the batch is not counted.
 *
 * state: PANGNN_BATCH_STATS_WORDS int64 words, 8-byte aligned, zeroed by the caller, only ever added to here:
 *   [0..3] counts[2*label + prediction], label = labels[i] > 0.5, prediction = sigmoid(logits[i]) >= threshold[0] — the
 *          predicate of pangnn_confusion_update_f32 (one device function serves both);
 *   [4]    batches   += 1
 *   [5]    cursor    += m  when the batch was appended (below)
 *   [6]    overflow   = 1  when it could not be
 *   [7]    loss_sum (double) += L,  L = loss_in[0] when loss_in is given, else the mean over the m real entries of the per-entry
 *          term of pangnn_bce_logits_f32 (fp32 terms, one device function serves both), summed in float64 in a fixed order;
 *   [8]    low 4 bytes: last_loss (float) = L
 *   the remaining words are the caller's (pangnn_amd keeps the threshold there).
 * threshold: device float, read by the kernel (it can change between replays of a captured graph).  pos_weight: device float or
 * NULL (1).  loss_in: device float or NULL.
 * Ranking data (cap > 0): scores float[cap] / score_labels uint8[cap] receive logits[0:m] as stored (no sigmoid: an exact
 * copy) and labels[0:m] > 0.5 at positions cursor .. cursor + m; if they do not fit, nothing is appended and overflow is set
 * (counts and loss are still taken).  cap == 0: no ranking data, the two buffers are not touched.
 * n_max up to the small-structure limit (16384): one workgroup; above: per-workgroup partials in `workspace`
 * (pangnn_batch_stats_workspace_bytes(n_max) bytes, 8-byte aligned, 0 below the limit) + a one-workgroup finish kernel.
 * Null logits / labels / state / threshold, n_max < 0, cap < 0 or cap > 0 without both buffers: PANGNN_E_BADARG; n_max >= 2^40:
 * PANGNN_E_TOOLARGE; a workspace that is NULL or too small where one is needed: PANGNN_E_WORKSPACE.
 * ---------------------------------------------------------------------------------------- */
#define PANGNN_BATCH_STATS_WORDS 16
int64_t pangnn_batch_stats_workspace_bytes(int64_t n_max);
int    pangnn_batch_stats_f32(const float* logits, const float* labels, int64_t n_max, const int64_t* live,
                              const float* pos_weight, const float* threshold, const float* loss_in, int64_t* state,
                              float* scores, uint8_t* score_labels, int64_t cap, void* workspace, int64_t workspace_bytes,
                              pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * out[0, c] = sum_n r[n] g[n, c], out[1, c] = sum_n s[n] g[n, c]  (out [2, F], F divides 256).
 * Backward of the scalar-feature embedding feeding the first GCN layer (src/gnn.py:97,125,158): the layer's
 * input is h0 = x w^T + 1 b^T, so dL/dw = (A_hat x)^T g and dL/db = (A_hat 1)^T g with g = dL/d(A_hat h0);
 * r = A_hat x and s = A_hat 1 are node vectors computed once per graph.  Reproducible two-stage sum.
 * ---------------------------------------------------------------------------------------- */
/* (r, s) = (A_hat x, A_hat 1) over one CSR order in ONE launch: r[i] = sum_{k in row i} val[k] x[other[k]],
 * s[i] = sum_{k in row i} val[k] (val = NULL: unit weights).  What the scalar-feature first layer needs of a graph
 * (src/gnn.py:97,125,158 by linearity: functional._EmbedConvIn); a fresh mini-batch pays it every step. */
int    pangnn_node_actions_f32(const int64_t* rowptr, const int32_t* other, const float* val, const float* x,
                               int64_t n_rows, float* r, float* s, pangnn_stream_t stream);
/* Operands of the decoder's re-associated first layer from mlp[0] = Linear(2D (+1), D) (src/gnn.py:110,173-175) in one
 * launch: w_pq [2D][D] = [W[:, :D] ; W[:, D:2D]], b_pq [2D] = [0 ; b], cvec [D] = W[:, 2D] (skip != 0).  w: [D] rows of
 * ldw >= 2D (+1) floats.  Plain data movement. */
int    pangnn_pq_operands_f32(const float* w, int64_t ldw, const float* b, int32_t d, int skip, float* w_pq,
                              float* b_pq, float* cvec, pangnn_stream_t stream);
/* out[c] = sum_n g[n, c] of a SHORT matrix (the node rows of a mini-batch; g f32 or bfloat16, ld in elements) in one
 * launch, fixed order of additions — the bias gradient of GCNConv (PyG: out + bias; src/gnn.py:165).  Long matrices: the
 * two-stage sums above. */
int    pangnn_colsum_small(const void* g, int32_t g_dtype, int64_t ldg, int64_t n, int32_t F, float* out,
                           pangnn_stream_t stream);
size_t pangnn_weighted_colsum_workspace_bytes(int32_t F);
int    pangnn_weighted_colsum_f32(const float* g, int64_t ldg, const float* r, const float* s, int64_t n,
                                  int32_t F, float* out, void* workspace, size_t workspace_bytes,
                                  pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Propagate over the positional-neighbour graph of a whole genome set (src/dataset.py:356-361: edges (i, j) for
 * j in [i - k, i + k] within [0, N), self loops included, unit weights — a band matrix; GCNConv at src/gnn.py:165):
 *   out[t, :] = bias + sum_{s = t-k .. t+k} dis[s] dis[t] x[s, :]       dis = deg^-1/2 (pangnn_gcn_norm_f32)
 * The same sums in the same order as pangnn_spmm_csr_f32 over that edge list (bit-identical), without index / weight
 * arrays.  The band is symmetric: the transposed propagate is the same call.  colsum (optional, [F]): column sums of
 * x — the bias gradient when x is the upstream gradient (backward of the layer in one pass).  x f32 or bf16 rows.
 * ---------------------------------------------------------------------------------------- */
size_t pangnn_band_propagate_workspace_bytes(int32_t F);
int    pangnn_band_propagate(const void* x, int32_t x_dtype, int64_t ldx, const float* dis, const float* bias, float* out,
                             int64_t ldo, int64_t n, int32_t F, int32_t k, float* colsum, void* workspace,
                             size_t workspace_bytes, pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The first GCN layer of the scalar-feature model as a rank-2 matrix (replaces, for `conv_in(embedding(x))`
 * of src/gnn.py:97,125,156-158 / :143-146 / :128-131, the embedding Linear(1, D), the propagate and GCNConv.lin):
 *   h0 = x w^T + 1 b^T (one scalar x per node)  =>  A_hat (h0) W^T + b_in = r a^T + s c^T + b_in,
 *   r = A_hat x, s = A_hat 1 (node vectors, once per graph: pangnn_spmm_csr_f32 on a 2-column table),
 *   a = W w, c = W b (H-vectors, per step; propagate and dense layer commute, so the same holds for D >= H).
 * pangnn_rank2_rows:       out[n, :] = r[n] a + s[n] c + bias   (out [N, F] stored as f32 or bf16, F % 4 == 0)
 * pangnn_weighted_colsum3: out[0] = sum_n r[n] g[n,:], out[1] = sum_n s[n] g[n,:], out[2] = sum_n g[n,:]  (out [3, F]):
 *   everything the layer's backward needs — dL/da, dL/dc, dL/db_in — from which dL/dW = dL/da w^T + dL/dc b^T,
 *   dL/dw = W^T dL/da, dL/db = W^T dL/dc.  g stored as f32 or bf16; reproducible two-stage sum.
 * ---------------------------------------------------------------------------------------- */
/* The same layer with the parameter algebra inside the kernels (one launch forward, three backward — what the
 * model uses): a = W w and c = W b are formed per workgroup in LDS; the backward runs pangnn_weighted_colsum3 and then
 * forms dL/dW_in [H, D], dL/dw [D], dL/db [D], dL/db_in [H] (nullable) in one small kernel.
 * workspace: pangnn_embed_conv_in_grads_workspace_bytes(H). */
int    pangnn_embed_conv_in_rows(const float* r, const float* s, const float* w_emb, const float* b_emb, const float* w_in,
                                 const float* b_in, int32_t D, void* out, int32_t out_dtype, int64_t ldo, int64_t n,
                                 int32_t H, pangnn_stream_t stream);
size_t pangnn_embed_conv_in_grads_workspace_bytes(int32_t H);
int    pangnn_embed_conv_in_grads(const void* g, int32_t g_dtype, int64_t ldg, const float* r, const float* s, int64_t n,
                                  const float* w_emb, const float* b_emb, const float* w_in, int32_t D, int32_t H,
                                  float* g_w_emb, float* g_b_emb, float* g_w_in, float* g_b_in, void* workspace,
                                  size_t workspace_bytes, pangnn_stream_t stream);

/* The same layer FUSED into the dense layer that follows it (GCNConv.lin of conv_out, gnn.py:164-166 / linear_out,
 * gnn.py:147): y = ELU(h) W_out^T (+ bias_out) with the [n, H] rows h = r a^T + s c^T + b_in generated inside the kernels
 * (8 bytes per row read instead of 4 H; the values are pangnn_embed_conv_in_rows', bit for bit).  Backward: dL/dW_out [M, H],
 * dL/dbias_out [M] (nullable) and sums [3, H] = [r s 1]^T dL/dh — dL/dh itself is never written — which
 * pangnn_embed_conv_in_grads_from_sums turns into the first layer's parameter gradients (as pangnn_embed_conv_in_grads
 * does after its own column sums).  (H, M) as pangnn_linear_supported(H, M, 1); fp32 storage. */
int    pangnn_embed_linear_supported(int32_t H, int32_t M);
int    pangnn_embed_linear_fwd(const float* r, const float* s, int64_t n, const float* w_emb, const float* b_emb,
                               const float* w_in, const float* b_in, int32_t D, int32_t H, const float* w_out,
                               const float* bias_out, int32_t M, float* y, int64_t ldy, pangnn_stream_t stream);
size_t pangnn_embed_linear_bwd_workspace_bytes(int32_t H, int32_t M);
int    pangnn_embed_linear_bwd(const float* g, int64_t ldg, const float* r, const float* s, int64_t n, const float* w_emb,
                               const float* b_emb, const float* w_in, const float* b_in, int32_t D, int32_t H,
                               const float* w_out, int32_t M, float* g_w_out, float* g_b_out, float* sums, void* workspace,
                               size_t workspace_bytes, pangnn_stream_t stream);
int    pangnn_embed_conv_in_grads_from_sums(const float* sums, const float* w_emb, const float* b_emb, const float* w_in,
                                            int32_t D, int32_t H, float* g_w_emb, float* g_b_emb, float* g_w_in,
                                            float* g_b_in, pangnn_stream_t stream);
int    pangnn_rank2_rows(const float* r, const float* s, const float* a, const float* c, const float* bias, void* out,
                         int32_t out_dtype, int64_t ldo, int64_t n, int32_t F, pangnn_stream_t stream);
size_t pangnn_weighted_colsum3_workspace_bytes(int32_t F);
int    pangnn_weighted_colsum3(const void* g, int32_t g_dtype, int64_t ldg, const float* r, const float* s, int64_t n,
                               int32_t F, float* out, void* workspace, size_t workspace_bytes, pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * BCEWithLogitsLoss(pos_weight), mean reduction (pangnn.py:98,203), loss and dL/dlogits in one pass:
 *   loss[0]     = 1/denom * sum_i (1-y_i) x_i + (1 + (pw-1) y_i) softplus(-x_i)
 *   g_logits[i] = 1/denom * ((1-y_i) - (1 + (pw-1) y_i) sigmoid(-x_i))
 * pos_weight is a DEVICE scalar (nullable = 1).  denom = number of edges of the whole job (differs from
 * n on a partitioned shard).  Reproducible two-stage sum.
 * ---------------------------------------------------------------------------------------- */
size_t pangnn_bce_logits_workspace_bytes(void);
int    pangnn_bce_logits_f32(const float* logits, const float* y, const float* pos_weight, int64_t n,
                             int64_t denom, float* loss, float* g_logits, void* workspace,
                             size_t workspace_bytes, pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * normalize_sim_scores (src/preprocessing.py:454-548) over a relation sorted by (source gene, candidate genome):
 * segment k = items [rowptr[k], rowptr[k+1]).  Per segment p = softmax(score / t) (one candidate: p = 1),
 * q = -10 log10(clip(1 - p, epsilon, 1 - epsilon)) + pseudo_count, float64 as in the reference.  One wavefront
 * per segment, fixed reduction order.  
 * ---------------------------------------------------------------------------------------- */
int    pangnn_softmax_qscore_f64(const int64_t* rowptr, const double* score, int64_t num_segments,
                                 int64_t num_items, double t, double epsilon, double pseudo_count, double* q,
                                 pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * `accelerator.backward(loss)` (pangnn.py:207) behind the one-pass training decoder: that pass has every gradient of the
 * step's loss in memory before autograd's backward starts, so backward only has to multiply them by the upstream
 * gradient of the loss — which `loss.backward()` / accelerate's `loss / gradient_accumulation_steps` make EXACTLY 1,
 * a fact the host cannot read without a synchronisation.  This entry scales up to PANGNN_SCALE_MAX_TENSORS fp32 buffers in
 * place by the DEVICE scalar scale[0] and does nothing at all (no loads beyond the scalar, no stores) when it is 1.0f.
 * ptrs / counts are HOST arrays of n_tensors device pointers / element counts (copied into the launch arguments).
 * ---------------------------------------------------------------------------------------- */
#define PANGNN_SCALE_MAX_TENSORS 8
int    pangnn_scale_unless_one_f32(float* const* ptrs, const int64_t* counts, int32_t n_tensors, const float* scale,
                                   pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The weightless link decoders, src/gnn.py:171-180,202-207 (`--decoder cosine` / `dotproduct`; pangnn_amd/gnn.py
 * AlternateGCN.cosine_sim / decode), as per-edge reductions over two gathered rows — no [E, 2D] edge tensor:
 *   mode PANGNN_SCORE_DOT:    logit_e = z[src_e] . z[dst_e]
 *   mode PANGNN_SCORE_COSINE: logit_e = torch.nn.functional.cosine_similarity(z[src_e], z[dst_e], dim=1, eps=1e-8)
 *                             = sum_k (a_k / max(|a|, eps)) (b_k / max(|b|, eps))
 * z [num_nodes, d] (row stride ldz elements, a multiple of 4) is read as stored: z_dtype = PANGNN_DTYPE_F32 (rows on 16
 * bytes), _BF16 or _F16 (rows on 8 bytes); every product and sum is fp32, so 2-byte rows give the bits of the f32 call on the
 * up-converted rows.  d in {16, 32, 64, 128, 256} (pangnn_edge_score_supported); any other d: PANGNN_E_BADARG.
 * edge_index[2][ld] int64, edges in the caller's order; node ids must lie in [0, num_nodes).
 * norms [num_nodes][2] (cosine; unused and nullable for dot) is WRITTEN by the forward entries — (1 / max(|z_n|, eps),
 * 1 / (max(|z_n|, eps) |z_n|), the latter 0 for a zero row) — and READ by the backward.
 * All results are reproducible bit for bit (fixed reduction orders, no atomics).
 * ---------------------------------------------------------------------------------------- */
#define PANGNN_SCORE_DOT    0
#define PANGNN_SCORE_COSINE 1
#define PANGNN_EDGE_SCORE_LOSS_PARTS 4096   /* floats of the loss_parts scratch of pangnn_edge_score_loss_mixed */
int    pangnn_edge_score_supported(int32_t d);
int    pangnn_edge_score_mixed(const void* z, int32_t z_dtype, int64_t ldz, int64_t num_nodes, const int64_t* edge_index,
                               int64_t ld, int64_t num_edges, int32_t d, int32_t mode, float* norms, float* logits,
                               pangnn_stream_t stream);
/* Forward with BCEWithLogitsLoss(pos_weight), mean over `denom`, in the same pass (parameterisation of pangnn_bce_logits_f32):
 * logits[E], loss[1], g_logits[E] = dL/dlogit (NOT multiplied by any upstream gradient).  pos_weight: device scalar, nullable
 * (= 1).  loss_parts: scratch of PANGNN_EDGE_SCORE_LOSS_PARTS floats (per-block partial sums, added in index order). */
int    pangnn_edge_score_loss_mixed(const void* z, int32_t z_dtype, int64_t ldz, int64_t num_nodes, const int64_t* edge_index,
                                    int64_t ld, int64_t num_edges, int32_t d, int32_t mode, const float* y,
                                    const float* pos_weight, int64_t denom, float* norms, float* logits, float* loss,
                                    float* g_logits, float* loss_parts, pangnn_stream_t stream);
/* ... of a fixed-shape padded batch (pangnn_collate_subgraphs_padded): live_edges (DEVICE int64[1], required) = the number of
 * real edges, read by the kernel, semantics as documented for `live_edges` of the decoder entry points above — with
 * m = min(max(*live_edges, 0), num_edges): logits[0:num_edges] are all written, g_logits[k] is exactly 0 for k >= m, loss and
 * g_logits[0:m] use 1.0f / (float)max(m, 1) (`denom` is ignored), m == 0 gives loss 0 and zero gradients.
 * pangnn_edge_score_bwd_mixed is the backward as it is: a padded edge's g = 0 adds exact zeros behind the real entries of a
 * row, and a padded node (only such edges) gets a zero row, the cosine diagonal term included (z finite). */
int    pangnn_edge_score_loss_live_mixed(const void* z, int32_t z_dtype, int64_t ldz, int64_t num_nodes,
                                         const int64_t* edge_index, int64_t ld, int64_t num_edges, int32_t d, int32_t mode,
                                         const float* y, const float* pos_weight, int64_t denom, float* norms, float* logits,
                                         float* loss, float* g_logits, float* loss_parts, const int64_t* live_edges,
                                         pangnn_stream_t stream);
/* Backward: gz[n] (fp32, row stride ldg, 16-byte aligned) = g_scale[0] * dL/dz[n], written once per node, with g[E] = dL/dlogit
 * in edge order and g_scale a DEVICE scalar (nullable = 1: `loss.backward()` needs no host read of the upstream gradient):
 *   dot:    sum_{out-edges e=(n,m)} g_e z_m + sum_{in-edges e=(m,n)} g_e z_m
 *   cosine: inv_n sum_{e at n} g_e inv_m z_m - z_n k_n sum_{e at n} g_e cos_e    (inv, k: the two norms entries, cos = logits)
 * The out-edges come from the by-source CSR (rowptr_src / other_src / perm_src of pangnn_csr_build(group_by = 0)), the in-edges
 * from the by-target CSR; per-edge scalars are read through perm.  A CSR order with hub rows may be passed as segments
 * (seg_ptr [num_seg + 1], parts_rowptr [num_nodes + 1], as pangnn_amd/graph.py CSR.long_rows builds them; both NULL: none):
 * one wave per segment writes a partial row into parts [num_seg * (d + 1)] floats (16-byte aligned), and the node's wave adds
 * its segments' partials in a fixed order.  logits / norms: what the forward wrote (cosine; nullable for dot). */
int    pangnn_edge_score_bwd_mixed(const void* z, int32_t z_dtype, int64_t ldz, int64_t num_nodes, int64_t num_edges, int32_t d,
                                   int32_t mode,
                                   const int64_t* rowptr_src, const int32_t* other_src, const int32_t* perm_src,
                                   const int64_t* seg_ptr_src, const int64_t* parts_rowptr_src, int64_t num_seg_src,
                                   float* parts_src,
                                   const int64_t* rowptr_dst, const int32_t* other_dst, const int32_t* perm_dst,
                                   const int64_t* seg_ptr_dst, const int64_t* parts_rowptr_dst, int64_t num_seg_dst,
                                   float* parts_dst,
                                   const float* g, const float* logits, const float* norms, const float* g_scale, float* gz,
                                   int64_t ldg, pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Max-candidate labelling, the "best hit per genome" baselines of predict_homolog_genes (src/predict.py:83-90):
 * calculate_baseline_labels (src/helper.py:437-485) over Q-scores and raw scores, calculate_logit_baseline_labels
 * (src/helper.py:494-576) over logits.  Segment k = the edges of one (source gene, candidate genome) group:
 * positions [seg_rowptr[k], seg_rowptr[k+1]) of the segment order, edge id seg_edge[pos] (int32), or pos itself when
 * seg_edge is NULL (a relation already in segment order).  seg_rowptr[num_segments + 1] starts at 0, ends at num_edges
 * and has no empty segment; every edge lies in exactly one segment.  Writes
 *   label[e] = isnan(v[e]) | (v[e] >= max of the non-NaN values of e's segment)      (uint8 0 / 1)
 * — the reference's strict `score < candidate_score` test: ties are all 1, a NaN value is 1, a NaN candidate beats nobody.
 * Optionally y[E] (float 0 / 1, > 0.5 = positive) with counts[4] (int64 [tn, fp, fn, tp], the layout of
 * pangnn_confusion_update_f32) += the confusion counts of label against y, in the same pass; both NULL or neither.
 * One wave per segment; integer atomics for the counts only; the result is bitwise reproducible.
 * ---------------------------------------------------------------------------------------- */
int    pangnn_best_candidate_f32(const int64_t* seg_rowptr, const int32_t* seg_edge, int64_t num_segments,
                                 int64_t num_edges, const float* value, const float* y, int64_t* counts, uint8_t* label,
                                 pangnn_stream_t stream);
int    pangnn_best_candidate_f64(const int64_t* seg_rowptr, const int32_t* seg_edge, int64_t num_segments,
                                 int64_t num_edges, const double* value, const float* y, int64_t* counts, uint8_t* label,
                                 pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Connected components of the kept edges: the groups that write_groups_file (src/postprocessing.py:5-36, called commented
 * out at pangnn.py:375) is meant to produce from the binary predictions.  The reference's loop cannot run (it never
 * initialises its list of sets and never merges two sets), so the semantics are defined here (pangnn_amd/postprocessing.py):
 * the graph of kept edges is undirected; edge e is kept when keep[e] != 0 (keep_itemsize 1: one byte per edge, e.g. a bool
 * mask; 4: one 32-bit word per edge, e.g. the int32 predictions of predict_homolog_genes, read as stored; 0: every edge is
 * kept and `keep` is not read).  Writes
 *   labels[v]  = the smallest node id of v's connected component (v itself for a node no kept edge joins to another),
 *   touched[v] = 1 when a kept edge (a self loop included) has v as an endpoint, else 0          (nullable),
 *   status[0]  = non-zero iff a kept edge names a node outside [0, num_nodes); such an edge is skipped, never dereferenced.
 * Three launches on `stream`: init, one lock-free union-find pass over the edges (integer atomicCAS / atomicMin on labels,
 * the larger root hooked onto the smaller id, so labels[x] <= x throughout), compress.  The result does not depend on the
 * order of edges, on duplicates or on scheduling.  src / dst are read for kept edges only.  num_nodes >= 2^31:
 * PANGNN_E_TOOLARGE.  num_edges == 0 or num_nodes == 0 still initialises labels, touched and status.
 * ---------------------------------------------------------------------------------------- */
int    pangnn_components_i32(const int64_t* src, const int64_t* dst, const void* keep, int keep_itemsize,
                             int64_t num_edges, int64_t num_nodes, int32_t* labels, uint8_t* touched, int32_t* status,
                             pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused EdgeConv (src/convolution.py:5-23): out[i] = b2 + max over the edges e = (j -> i) of W2 relu(u[i] + v[j]), 0 for a row
 * without in-edges, where u = x (Wa - Wb)^T + b1 and v = x Wb^T are the first Linear of mlp(cat[x_i, x_j - x_i]) taken at
 * node level by the caller ([num_nodes, out_dim] f32, row strides ldu / ldv in elements, 16-byte aligned).  out_dim in
 * {64, 128}; any other width: PANGNN_E_BADARG.  The graph is its by-target CSR (rowptr int64 [num_nodes + 1], col = source
 * and perm = original edge id per sorted entry, int32) plus the caller's edge_index [2, ld] (the target of entry k is
 * edge_index[ld + perm[k]]).  Nothing of size num_edges x out_dim exists: the product runs per 32-entry tile on
 * v_mfma_f32_32x32x2_f32 and the per-row maximum is taken on chip; rows that cross the chunks of entries a wave owns (hub
 * rows) leave one partial per chunk in `scratch`, combined by a second launch.
 *   arg[i][c] = original id of the edge whose message is out[i][c] - b2[c]; -1 on rows without in-edges.
 * Semantics of pangnn_segment_max_rows_f32: the first maximum in ascending edge id wins, NaN propagates, the maximum is
 * taken over the messages alone (an all-negative row returns that negative value).  Bitwise reproducible, no atomics.
 * `scratch`: pangnn_edge_conv_scratch_bytes(num_edges, out_dim, backward = 0 / 1) bytes (bounded in num_edges but for one
 * byte per edge in the backward); smaller: PANGNN_E_WORKSPACE.
 *
 * pangnn_edge_conv_bwd_f32: with s_e[c] = g[i][c] * [arg[i][c] == e], h_e = relu(u[i] + v[j]) recomputed,
 *   gh_e = (W2^T s_e) * [h_e > 0],  gu[i] = sum over in-edges,  gv[j] = sum over out-edges,  gw2 = sum_e s_e h_e^T.
 * One pass over the by-target CSR (gu, gw2) and one over the by-source CSR (src_*: rowptr, col = target, perm), each in CSR
 * order; tiles none of whose edges is an arg-max skip the products.  arg [num_nodes, out_dim] contiguous, as the forward
 * wrote it; g / gu / gv row strides ldg / ldgrad.  Fixed-order sums, no float atomics.
 * ---------------------------------------------------------------------------------------- */
int64_t pangnn_edge_conv_scratch_bytes(int64_t num_edges, int32_t out_dim, int backward);
int    pangnn_edge_conv_fwd_f32(const float* u, int64_t ldu, const float* v, int64_t ldv, int64_t num_nodes,
                                const float* w2, const float* b2, int32_t out_dim, const int64_t* rowptr,
                                const int32_t* col, const int32_t* perm, const int64_t* edge_index, int64_t ld,
                                int64_t num_edges, float* out, int32_t* arg, int64_t ldo, void* scratch,
                                int64_t scratch_bytes, pangnn_stream_t stream);
int    pangnn_edge_conv_bwd_f32(const float* g, int64_t ldg, const int32_t* arg, const float* u, int64_t ldu,
                                const float* v, int64_t ldv, int64_t num_nodes, const float* w2, int32_t out_dim,
                                const int64_t* dst_rowptr, const int32_t* dst_col, const int32_t* dst_perm,
                                const int64_t* src_rowptr, const int32_t* src_col, const int32_t* src_perm,
                                const int64_t* edge_index, int64_t ld, int64_t num_edges, float* gu, float* gv,
                                int64_t ldgrad, float* gw2, void* scratch, int64_t scratch_bytes, pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * A structure derived by filtering (csrc/edge_filter.hip): the sub-sampled graph of sub_sample_graph_edges (src/helper.py:
 * 16-68, pangnn.py:190) — edge list, per-edge arrays and CSR orders of the kept edges — from the PARENT's tables, by
 * order-preserving compaction instead of a sort.  Edge e is kept when keep[e] != 0; `keep` is read at its stored width,
 * keep_itemsize = 1 (one byte per edge) or 4 (one 32-bit word per edge).
 * Inputs: the parent's edge_index[2][ld] and its by-target CSR of pangnn_csr_build(group_by = 1) (rowptr [num_nodes + 1],
 * other, perm); optionally its by-source CSR (group_by = 0) — three pointers, all set or all NULL; up to two per-edge f32
 * arrays attr0 / attr1 (nullable, each with its output).  `num_kept` is the number of kept edges as the HOST knows it: every
 * output is sized by it.
 * Outputs: child_edge_index[2][child_ld] = the kept edges in the caller's order, child_attr0 / child_attr1 [num_kept],
 * kept_id [num_kept] int32 = the parent edge id of every child edge (ascending), and for each CSR order given the child's
 * rowptr [num_nodes + 1] / other / perm [num_kept], entry for entry what pangnn_csr_build makes of child_edge_index (the sort
 * and the compaction are both stable).  count[0] = the number of kept edges as counted on the device; status[0] = 0, or bit 0:
 * count != num_kept, bit 1: a parent perm entry outside [0, num_edges) (the entry counts as dropped) or a parent rowptr entry
 * outside [0, num_edges] (clamped).  With a wrong num_kept nothing is written outside the num_kept entries of an output:
 * surplus edges are dropped, a missing tail is zero-filled and belongs to no row.
 * num_edges == 0, num_kept == 0 (per-edge outputs may then be NULL) and num_kept == num_edges write every output.
 * Integer scans (rocPRIM) and plain stores: bitwise reproducible.  num_edges or num_nodes >= 2^31: PANGNN_E_TOOLARGE.
 * `workspace`: pangnn_structure_filter_workspace_bytes(num_edges) bytes, 16-byte aligned (0 from the query: failure — it
 * asks rocPRIM for the scans' temporary size, which needs a device); smaller: PANGNN_E_WORKSPACE.
 * ---------------------------------------------------------------------------------------- */
int64_t pangnn_structure_filter_workspace_bytes(int64_t num_edges);
int    pangnn_structure_filter(const int64_t* edge_index, int64_t ld, int64_t num_edges, int64_t num_nodes,
                               const void* keep, int keep_itemsize, int64_t num_kept,
                               const int64_t* rowptr_dst, const int32_t* other_dst, const int32_t* perm_dst,
                               const int64_t* rowptr_src, const int32_t* other_src, const int32_t* perm_src,
                               const float* attr0, const float* attr1,
                               int64_t* child_edge_index, int64_t child_ld, int32_t* kept_id,
                               float* child_attr0, float* child_attr1,
                               int64_t* child_rowptr_dst, int32_t* child_other_dst, int32_t* child_perm_dst,
                               int64_t* child_rowptr_src, int32_t* child_other_src, int32_t* child_perm_src,
                               int32_t* count, int32_t* status, void* workspace, int64_t workspace_bytes,
                               pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The decoder's run-sum plan of a CSR order from its row pointer (csrc/csr_plan.hip): the tables that
 * EdgeStructure._plan_of_sorted_keys (pangnn_amd/graph.py, the written definition) makes of the sorted keys, entry for entry,
 * without the keys: `part_buf` / `part_off` of the training decoder above, `part_rowptr` of its part sums.
 * Input: rowptr [n_rows + 1] int64, non-decreasing, rowptr[0] == 0, rowptr[n_rows] == num_edges (a rectangular structure's
 * trimmed row pointer is fine); num_edges >= 1, n_rows >= 1; span = 32 * chunk_tiles (anything else: PANGNN_E_BADARG).
 * With c[r] = (rowptr[r + 1] > rowptr[r] && rowptr[r] % span != 0), Cin / Cex its inclusive / exclusive prefix sums:
 *   keys [num_edges] int32          the row of every sorted entry
 *   part_off [ceil(E / span)] int32 part_off[ch] = ch + Cin[row of entry ch * span]
 *   part_rowptr [n_rows + 1] int64  rowptr[r] / span + Cex[r] + (rowptr[r] % span != 0) while rowptr[r] < E, else last + 1
 *   last [1] int64                  the last part id, (E - 1) / span + sum(c)
 * A rowptr that breaks the contract yields unspecified tables, but no access outside the arrays as sized above.
 * One integer scan over the rows (rocPRIM) and one launch with plain stores: bitwise reproducible, nothing read back.
 * num_edges or n_rows >= 2^31: PANGNN_E_TOOLARGE.  `workspace`: pangnn_csr_plan_workspace_bytes(n_rows) bytes, 16-byte
 * aligned (0 from the query: failure — it asks rocPRIM for the scan's temporary size, which needs a device); smaller:
 * PANGNN_E_WORKSPACE.
 * ---------------------------------------------------------------------------------------- */
int64_t pangnn_csr_plan_workspace_bytes(int64_t n_rows);
int    pangnn_csr_plan(const int64_t* rowptr, int64_t n_rows, int64_t num_edges, int32_t span, int32_t* keys,
                       int32_t* part_off, int64_t* part_rowptr, int64_t* last, void* workspace, int64_t workspace_bytes,
                       pangnn_stream_t stream);
/* The position words of that order for pangnn_decoder_dgrad_stream_f32: perm [E] int32 (the order's edge ids, each in
 * [0, 2^31)), keys [E] int32 as written by pangnn_csr_plan (non-decreasing), span as above ->
 *   tpos [E] uint32   perm[p] | closes_p << 31,  closes_p = (p + 1 == E  ||  (p + 1) % span == 0  ||  keys[p + 1] != keys[p])
 * i.e. bit 31 says that a part row ends behind position p.  One elementwise launch, plain stores; num_edges >= 1. */
int    pangnn_csr_plan_tpos(const int32_t* perm, const int32_t* keys, int64_t num_edges, int32_t span, uint32_t* tpos,
                            pangnn_stream_t stream);
/* The position stream of a source-sorted edge list for pangnn_decoder_train_stream_*: edge_index [2, ld] int64 (row 0
 * non-decreasing, every id in [0, 2^31)), span = 32 * pangnn_decoder_chunk_tiles_for(num_edges) ->
 *   spos [2 * P] uint32, P = 32 * ceil(num_edges / 32) positions of two words each (8-byte aligned):
 *   { src_k | closes_p << 31, dst_k } with k = min(p, num_edges - 1) — a position past the list repeats the last edge —
 *   closes_p = (p + 1 == P  ||  (p + 1) % span == 0  ||  (p + 1 < num_edges && src[p + 1] != src[p]))
 * i.e. bit 31 says that a part row ends behind position p: where the source changes, at the end of a chunk, and at the
 * end of the last tile (whose padding adds zeros to the last run).  One elementwise launch, plain stores; num_edges >= 1. */
int    pangnn_csr_plan_spos(const int64_t* edge_index, int64_t ld, int64_t num_edges, int32_t span, uint32_t* spos,
                            pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The mask of the k smallest keys (csrc/mask_select.hip): keep[i] = 0 for exactly the k entries that come first in
 * (key, index) order — among equal keys the lower index loses — and 1 for the others.  keys [n] int64 with
 * 0 <= key < 2^63, 16-byte aligned, only read (preserved); keep [n] one byte each, 4-byte aligned; 0 <= k <= n is the
 * host's number (k > n: PANGNN_E_BADARG).  k == 0 writes all ones, k == n all zeros, n == 0 nothing.
 * A radix select over histograms (integer atomics only) and one mask pass; ranks among keys tied with the k-th smallest
 * come from fixed index ranges, never from an arrival order: the mask is a function of (keys, k).  Nothing is read back.
 * n >= 2^31: PANGNN_E_TOOLARGE.  `workspace`: pangnn_mask_k_smallest_workspace_bytes(n) bytes (a few KB, 0: n out of
 * range), 16-byte aligned; smaller: PANGNN_E_WORKSPACE.
 * ---------------------------------------------------------------------------------------- */
int64_t pangnn_mask_k_smallest_workspace_bytes(int64_t n);
int    pangnn_mask_k_smallest_i64(const int64_t* keys, int64_t n, int64_t k, uint8_t* keep, void* workspace,
                                  int64_t workspace_bytes, pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * dL/d(edge_weight) of GCNConv (csrc/edge_weight_grad.hip).  With deg[v] = sum of w_e over the in-edges of v,
 * dis = deg^-1/2 (0 where deg == 0), w^_e = dis[src_e] w_e dis[dst_e], out = A^ x + b and g = dL/dout:
 *   gw_e    = <g[dst_e, :], x[src_e, :]>                  (pangnn_edge_dot_mixed over the by-target CSR)
 *   t_e     = gw_e w_e
 *   gdis[v] = sum_{e: dst_e = v} t_e dis[src_e] + sum_{e: src_e = v} t_e dis[dst_e]
 *   gdeg[v] = -1/2 dis[v]^3 gdis[v], 0 where dis[v] == 0   (torch's masked_fill; a target whose in-edges all weigh 0 is
 *                                                           0 * inf = NaN in torch and DEFINED as 0 here)
 *   dL/dw_e = dis[src_e] dis[dst_e] gw_e + gdeg[dst_e]    (pangnn_gcn_norm_bwd_f32, in the caller's edge order)
 *
 * pangnn_edge_dot_mixed: for every entry k of row r of a CSR (rowptr int64 [n_rows + 1], idx int32 [nnz], perm int32
 * [nnz]) out_sorted[k] = <g[r, 0:F], x[idx[k], 0:F]>, and the same value goes to out_orig[perm[k]] when out_orig is given
 * (perm may be NULL otherwise).  g [g_rows >= n_rows, F] and x [x_rows, F] are separate tables (a rectangular structure is
 * describable), each read as stored: *_dtype = PANGNN_DTYPE_F32 (rows on 16 bytes) or _BF16 / _F16 (rows on 8 bytes; two
 * 2-byte tables of one call have the same type), row strides ldg / ldx in elements, multiples of 4.  F in {16, 32, 64, 128,
 * 256} for float32 tables, {32, 64, 128, 256} as soon as one table has 2-byte rows (the widths the propagate gathers in that
 * type); anything else: PANGNN_E_BADARG.  Every product and sum is fp32 in a fixed order (four fused multiply-adds per lane,
 * a butterfly over the F / 4 lanes of an entry): 2-byte rows give the bits of the float32 call on the up-converted rows.
 * Work is dealt out by entries, not rows (a wave per chunk of consecutive entries): a hub row is shared by many waves and,
 * every output being one entry's own dot product, no part sums exist.  Along a row the g piece stays in registers.
 * nnz == 0 launches nothing; nnz, n_rows or x_rows >= 2^31: PANGNN_E_TOOLARGE.
 *
 * pangnn_gcn_norm_bwd_f32: the four lines below gw_e above, for a SQUARE structure given as edge_index (int64 [2, ld], the
 * caller's order) and both CSR orders (rowptr int64 [num_nodes + 1], other = opposite endpoint, perm = original edge id).
 * A CSR order with hub rows also brings its segment table in the form pangnn_edge_score_bwd_mixed takes (seg_ptr int64
 * [num_seg + 1], parts_rowptr int64 [num_nodes + 1], every row owning at least one segment; both NULL: the rows are walked
 * as they are).  w, gw [num_edges] in the caller's order, dis [num_nodes]; gweight [num_edges] is written in the caller's
 * order.  No float atomics: a 16-lane group per row (per segment) — lane j adds the entries j, j + 16, ... of the row in
 * ascending CSR position, the 16 lane sums meet in a fixed butterfly; a hub row's segment partials are added in index
 * order by the same scheme.  The result is a function of (structure, w, gw, dis): bit-reproducible.
 * `workspace`: pangnn_gcn_norm_bwd_workspace_bytes(num_nodes, num_seg_dst, num_seg_src) bytes (segment counts 0 for an
 * order without a table; passed as an int64_t), 16-byte aligned; smaller, negative or NULL: PANGNN_E_WORKSPACE.  num_edges == 0 launches nothing.
 * ---------------------------------------------------------------------------------------- */
int    pangnn_edge_dot_mixed(const int64_t* rowptr, const int32_t* idx, const int32_t* perm, const void* g, int32_t g_dtype,
                             int64_t ldg, int64_t g_rows, const void* x, int32_t x_dtype, int64_t ldx, int64_t x_rows,
                             int64_t n_rows, int64_t nnz, int32_t F, float* out_sorted, float* out_orig,
                             pangnn_stream_t stream);
int64_t pangnn_gcn_norm_bwd_workspace_bytes(int64_t num_nodes, int64_t num_seg_dst, int64_t num_seg_src);
int    pangnn_gcn_norm_bwd_f32(const int64_t* edge_index, int64_t ld, int64_t num_edges, int64_t num_nodes,
                               const int64_t* rowptr_dst, const int32_t* other_dst, const int32_t* perm_dst,
                               const int64_t* seg_ptr_dst, const int64_t* parts_rowptr_dst, int64_t num_seg_dst,
                               const int64_t* rowptr_src, const int32_t* other_src, const int32_t* perm_src,
                               const int64_t* seg_ptr_src, const int64_t* parts_rowptr_src, int64_t num_seg_src,
                               const float* w, const float* gw, const float* dis, float* gweight, void* workspace,
                               int64_t workspace_bytes, pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The Q-score edge weights of normalize_sim_scores (src/preprocessing.py:454-548) as a differentiable function of the bit
 * scores and of the softmax temperature (csrc/qscore.hip; pangnn_amd/weights.py).  A segment plan describes the (source
 * gene, candidate genome) groups over the graph's OWN edge list: rowptr int64 [num_segments + 1] (starts at 0, ends at
 * num_edges, no empty segment) and item int32 [num_edges], the edge id at every position of the segment order.  Scores are
 * read and weights / gradients written at item[pos]: every per-edge array is in the caller's edge order.  score is float32
 * or float64 as stored (score_dtype = PANGNN_DTYPE_F32 / _F64; any other code: PANGNN_E_BADARG); all arithmetic is float64.
 * t [1] is a DEVICE double (a parameter's value: never read on the host); 0 < epsilon < 0.5.
 *
 * pangnn_qscore_fwd: per segment x_i = score_i / t, lse = log sum_j exp(x_j - max_j x_j) + max_j x_j, p_i = exp(x_i - lse),
 *   weight_i = -10 log10(clip(1 - p_i, epsilon, 1 - epsilon)) + pseudo_count    (one candidate: p = 1; a NaN p: 1 - epsilon
 *   in place of the clip, the reference's nan_to_num), written as float32 or float64 (weight_dtype); lse [2 * num_segments]
 * is kept for the backward: lse of every segment, then r, what the last addition rounded away (log sum + max = lse + r
 * exactly).  The operations and their order (lanes stride the segment, xor-shuffle tree) are those of
 * pangnn_softmax_qscore_f64: float64 weights have its bits.
 *
 * pangnn_qscore_bwd: with g [num_edges] = dL/dweight (float32 or float64, g_dtype), c_i = 1 - p_i,
 *   a_i = g_i (10 / ln 10) / c_i where epsilon <= c_i <= 1 - epsilon, else 0          (torch.clamp's inclusive mask)
 *   S = sum_j p_j a_j,  gx_i = p_i ((a_i - S) + S r),  gscore_i = gx_i / t,  gt[0] = sum over segments of -(sum_i gx_i score_i) / t^2
 * (S (1 - r): S times the probability of the unrounded lse, as autograd's chain through lse = log sum + max has it; the two
 * terms cancel down to c_i of their size, so r matters where c_i is near epsilon).
 * gscore [num_edges] has the type of score; a one-candidate segment gives zeros.  Either output may be NULL and is then not
 * computed.  t_parts: float64 [num_segments + PANGNN_QSCORE_SUM_PARTS] scratch (needed with gt): the segments' shares of
 * dL/dt, then their block sums, added in an order that num_segments alone fixes.  No float atomics: two calls give the same
 * bits.  Non-finite scores are not special-cased: a NaN score makes its segment's gscore and gt NaN, as the formula does.
 * One wave per segment (segments are bounded by the genes of one genome; any length is correct).  num_edges == 0 launches
 * nothing; num_edges or num_segments >= 2^31: PANGNN_E_TOOLARGE.
 * ---------------------------------------------------------------------------------------- */
#define PANGNN_QSCORE_SUM_PARTS 1024
int    pangnn_qscore_fwd(const int64_t* rowptr, const int32_t* item, const void* score, int32_t score_dtype,
                         int64_t num_segments, int64_t num_edges, const double* t, double epsilon, double pseudo_count,
                         void* weight, int32_t weight_dtype, double* lse, pangnn_stream_t stream);
int    pangnn_qscore_bwd(const int64_t* rowptr, const int32_t* item, const void* score, int32_t score_dtype, const void* g,
                         int32_t g_dtype, const double* lse, int64_t num_segments, int64_t num_edges, const double* t,
                         double epsilon, void* gscore, double* gt, double* t_parts, pangnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The induced similarity edges of per-group sub-graphs (csrc/induced_edges.hip; pangnn_amd/subgraphs.py, step 3 of
 * build_subgraphs, whose index-op form _induced_edges_index_ops is the definition).  All tables are int64.
 *   rowptr [num_nodes + 1], dst [num_edges]: the relation grouped by source, targets in [0, num_nodes);
 *   row_node [num_rows]: the global node of every row, rows in (group, local id) order;
 *   group_off [num_groups + 1]: group g owns rows [group_off[g], group_off[g + 1]) (group_off[0] = 0, non-decreasing,
 *     group_off[num_groups] = num_rows; a group may be empty); the local id of row r of group g is r - group_off[g];
 *   sorted_node / sorted_local [num_rows]: over the same ranges, each group's node ids ascending and their local ids.
 * For every row r (group g, node v, local id l) and every position p in [rowptr[v], rowptr[v + 1]), ascending: if dst[p]
 * is a node of group g with local id m, the triple (l, m, p) is emitted.  Output order: rows in row order, positions
 * ascending inside a row — the inputs alone fix every output address (no atomics: two calls give the same bytes), and
 * duplicate (src, dst) entries of the relation are each emitted.  Nothing proportional to the number of positions walked
 * is stored.
 *
 * pangnn_induced_edges_count: row_off [num_rows + 1] = exclusive scan of the rows' hit counts, row_off[num_rows] = the
 *   total (read it back to size the outputs).  One memset, one launch and one rocPRIM scan on `stream`.
 * pangnn_induced_edges_fill: the same walk on the same inputs; out_src / out_dst / out_pos [total] = l / m / p of every hit,
 *   written at row_off[r] + its rank inside the row (a triple that would land at or past `total` is not written).
 *   total == 0 launches nothing.
 * Both only enqueue; neither allocates.  `scratch`: pangnn_induced_edges_scratch_bytes(num_rows) bytes, 16-byte aligned (0
 * from the query: num_rows out of range, or failure — it asks rocPRIM for the scan's temporary size, which needs a device);
 * NULL or smaller: PANGNN_E_WORKSPACE.  Negative sizes, rows without groups or nodes, a NULL table with num_rows > 0 (dst:
 * and num_edges > 0), a NULL output with total > 0: PANGNN_E_BADARG.  num_nodes >= 2^31 (node ids are held as 32-bit words on
 * chip), num_rows or num_groups >= 2^40: PANGNN_E_TOOLARGE; positions and output addresses are 64-bit, num_edges is not
 * bounded.  A group of any size and a row of any length are handled (a group's ids are staged on chip up to 6144 of them,
 * searched in place beyond).
 * ---------------------------------------------------------------------------------------- */
int64_t pangnn_induced_edges_scratch_bytes(int64_t num_rows);
int    pangnn_induced_edges_count(const int64_t* rowptr, const int64_t* dst, int64_t num_nodes, int64_t num_edges,
                                  const int64_t* row_node, int64_t num_rows, const int64_t* group_off, int64_t num_groups,
                                  const int64_t* sorted_node, const int64_t* sorted_local, int64_t* row_off, void* scratch,
                                  int64_t scratch_bytes, pangnn_stream_t stream);
int    pangnn_induced_edges_fill(const int64_t* rowptr, const int64_t* dst, int64_t num_nodes, int64_t num_edges,
                                 const int64_t* row_node, int64_t num_rows, const int64_t* group_off, int64_t num_groups,
                                 const int64_t* sorted_node, const int64_t* sorted_local, const int64_t* row_off,
                                 int64_t total, int64_t* out_src, int64_t* out_dst, int64_t* out_pos, pangnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PANGNN_HIP_H */
