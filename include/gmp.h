/*
 * gmp.h — C ABI of the MI355X (gfx950) geometric message-passing hot path.
 *
 * The reference (NW-JEFF/Geometric-Message-Passing) has no native code of its own: its hot path
 * runs through PyG `MessagePassing.propagate`, `torch_scatter.scatter` (C++/CUDA custom ops
 * `torch.ops.torch_scatter.scatter_sum/mean/max`) and e3nn modules.  Each
 * entry point below replaces one of those call sites; the replaced interface is cited per
 * function as reference file:line.
 *
 * Conventions (all functions):
 *   - plain device pointers, int64 sizes, fp32 features, int64 indices (the reference dtypes);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); no function allocates,
 *     frees or synchronises; all work is enqueued on `stream` (graph-capture safe);
 *   - return GMP_OK (0) or a negative error code (gmp_error_string); argument checks are done
 *     on the host before anything is enqueued; device-side index range errors are reported
 *     through an optional int32 device flag (`err_flag`, set to 1; caller checks when it wants);
 *   - outputs are fully written (zero rows included) unless documented as accumulating.
 */
#ifndef GMP_H_
#define GMP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3 (r04): K8 symmetric contraction takes the per-channel dim and A4 (gmp_sc_monomials added);
 * the TP descriptor holds 8 output blocks (128 bytes), <= 48 paths.
 * 2 (r04): EGNN forward / backward take save_planes; gmp_egnn_set_xhat_mode and
 * gmp_egnn_edge_bwd_ab_f32 removed.  (r03 changed gmp_triplet_fill_f32 under version 1.)
 * 4 (r05): gmp_egnn_node_fwd_f32 / gmp_egnn_node_params added.
 * Version 5 (r05): the opt-in TP kernels K7s / K7f (gmp_tp_node_fwd_fused_f32,
 * gmp_tp_z_fused_layout_*, gmp_tp_node_dw_*), the row GEMM (gmp_split_x3_f32, gmp_gemm_x3_f32),
 * gmp_tp_gemm_set_rings, gmp_wgrad_set_grid_cap and the CU-masked stream entries removed; K8 takes
 * the sparse term plan (any irreps), gmp_sc_monomials removed.
 * Version 6 (r06): gmp_gvp_ff_{fwd,bwd}_f32 (K17, the GVPConvLayer node feed-forward) and
 * gmp_egnn_node_bwd_f32 / gmp_egnn_node_bwd_partial_rows (K15b) added. */
#define GMP_ABI_VERSION 6

enum {
  GMP_OK = 0,
  GMP_ERR_ARG = -1,         /* bad pointer / size / unsupported combination */
  GMP_ERR_HIP = -2,         /* a HIP runtime call failed (see gmp_last_hip_error) */
  GMP_ERR_UNSUPPORTED = -3, /* shape not supported by this fused kernel */
  GMP_ERR_WORKSPACE = -4    /* workspace too small */
};

enum { GMP_REDUCE_SUM = 0, GMP_REDUCE_MEAN = 1, GMP_REDUCE_MAX = 2 };
enum { GMP_ACT_RELU = 0, GMP_ACT_SILU = 1 };

int gmp_abi_version(void);
const char* gmp_error_string(int code);
int gmp_last_hip_error(void);

/* ------------------------------------------------------------------------------------------
 * Index preprocessing: stable CSR of an index array (receiver-sorted edge lists).
 * Replaces the implicit ordering work of torch_scatter's atomics (egnn_layer.py:77,79;
 * tfn_layer.py:87; PyG aggregate): we sort once per graph and reduce deterministically.
 *   perm[k]      = position of the k-th item in stable order of index (k = 0..n_items-1)
 *   rowptr[s]    = first k with index[perm[k]] >= s   (s = 0..n_seg), rowptr[n_seg] = n_items
 *   payload_out  = payload[perm] (optional, may be NULL)
 * Workspace: gmp_csr_workspace_size(n_items, n_seg) bytes.
 * ------------------------------------------------------------------------------------------ */
size_t gmp_csr_workspace_size(int64_t n_items, int64_t n_seg);
int gmp_csr_build(const int64_t* index, int64_t n_items, int64_t n_seg, const int64_t* payload,
                  int64_t* perm, int64_t* rowptr, int64_t* index_sorted, int64_t* payload_out,
                  int32_t* err_flag, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * K2 gather: out[e, :] = src[index[e], :]   (PyG `_collect` index_select of x_i / x_j,
 * torch_geometric MessagePassing.propagate; tfn_layer.py:85 `node_attr[dst]`).
 * Out-of-range index -> row of zeros and *err_flag = 1 (err_flag may be NULL).
 * ------------------------------------------------------------------------------------------ */
int gmp_gather_rows_f32(const float* src, int64_t n_rows, int64_t F, const int64_t* index,
                        int64_t n_index, float* out, int32_t* err_flag, void* stream);

/* ------------------------------------------------------------------------------------------
 * K3 segmented reduce over a CSR (torch_scatter.scatter(src, index, dim=0, dim_size, reduce)
 * with reduce in {sum/add, mean, max}; egnn_layer.py:77,79, tfn_layer.py:87, PyG aggregate,
 * global_add_pool / global_mean_pool).
 *   out[s, f] = reduce_{k in [rowptr[s], rowptr[s+1])} src[perm ? perm[k] : k, f]
 *   empty segments -> 0; mean divides by max(count, 1); max also writes argmax[s, f]
 *   (item index, n_items for empty segments; argmax may be NULL for sum/mean).
 * Summation order is fixed by the CSR (deterministic).  Long segments (average length >= 2048,
 * e.g. global pools) are split over workgroups when a workspace of
 * gmp_segment_reduce_workspace_size(...) bytes is given (NULL / too small = single-wave path).
 * ------------------------------------------------------------------------------------------ */
size_t gmp_segment_reduce_workspace_size(int64_t n_items, int64_t n_seg, int64_t F, int reduce);
int gmp_segment_reduce_f32(const float* src, int64_t n_items, int64_t F, const int64_t* perm,
                           const int64_t* rowptr, int64_t n_seg, int reduce, float* out,
                           int64_t* argmax, void* workspace, size_t workspace_bytes,
                           void* stream);

/* Backward of gmp_segment_reduce_f32 w.r.t. src (torch_scatter autograd):
 *   sum : grad_src[e] = grad_out[index[e]]
 *   mean: grad_src[e] = grad_out[index[e]] / max(count[index[e]], 1)   (count from rowptr)
 *   max : grad_src[e, f] = (argmax[index[e], f] == e) ? grad_out[index[e], f] : 0            */
int gmp_segment_reduce_bwd_f32(const float* grad_out, int64_t n_seg, int64_t F,
                               const int64_t* index, int64_t n_items, const int64_t* rowptr,
                               int reduce, const int64_t* argmax, float* grad_src, void* stream);

/* ------------------------------------------------------------------------------------------
 * K4 EGNN fused edge message + aggregation (egnn_layer.py:62-80 message/aggregate; the node
 * update :82-86 stays a node-level op).  Edges must be receiver-sorted (CSR from
 * gmp_csr_build on edge_index[1]).  The first message Linear(2d+1 -> d) is split as
 *   W1 [h_i | h_j | dist] = (h W1a^T)[i] + (h W1b^T)[j] + w1d * dist
 * so the node projections AB = [h W1a^T | h W1b^T] (N x 2d) are computed once per node by the
 * caller.  Per edge e = (j -> i), in registers:
 *   rel = pos[i]-pos[j]; dist = |rel|; y1 = act(LN1(AB[i,:d] + AB[j,d:] + w1d*dist + b1))
 *   m = act(LN2(W2 y1 + b2)); y3 = act(LN3(W3 m + b3)); s = w4.y3 + b4; shift = rel * s
 * and per receiver i (segmented, deterministic, no atomics):
 *   m_aggr[i] = sum_e m  (or mean if msg_mean), pos_aggr[i] = mean_e shift.
 * d in {32, 64, 128}.  LayerNorm eps = ln_eps.
 * ------------------------------------------------------------------------------------------ */
typedef struct gmp_egnn_params {
  const float* w1d;  /* (d)  column 2d of mlp_msg.0.weight   */
  const float* b1;   /* (d)  mlp_msg.0.bias                   */
  const float* ln1_w;
  const float* ln1_b;
  const float* W2;   /* (d,d) mlp_msg.3.weight, row-major [out][in] */
  const float* b2;
  const float* ln2_w;
  const float* ln2_b;
  const float* W3;   /* (d,d) mlp_pos.0.weight */
  const float* b3;
  const float* ln3_w;
  const float* ln3_b;
  const float* w4;   /* (d)  mlp_pos.3.weight */
  const float* b4;   /* (1)  mlp_pos.3.bias   */
} gmp_egnn_params;

/* save_xhat / save_rstd: both NULL (inference) or, for training, (save_planes, E, d) and (E, 3)
 * buffers that receive the LayerNorm outputs and their 1/std per edge (receiver-sorted rows) for
 * gmp_egnn_edge_bwd_f32: save_planes = 2 (default form) stores x_hat1, x_hat2 — the backward
 * recomputes x_hat3 from x_hat2 and the saved 1/std, bitwise the forward's value; 3 also stores
 * x_hat3.  The backward takes the same save_planes (the caller keeps it with the buffer). */
/* The two d x d products per edge chunk run by default on the f16 MFMA over 2-plane (hi + lo)
 * splits of the operands with power-of-two scaling (22-bit operands, f32 accumulation; relative
 * error ~2^-21 per product); gmp_egnn_set_f32_mfma(1) selects
 * the exact f32-MFMA fmaf chains.  Returns the previous setting. */
int gmp_egnn_set_f32_mfma(int on);
int gmp_egnn_edge_fwd_f32(int64_t n_nodes, int64_t n_edges, int64_t d, const float* AB,
                          const float* pos, const int64_t* rowptr, const int64_t* recv,
                          const int64_t* send, const gmp_egnn_params* params, int act,
                          int msg_mean, float ln_eps, float* m_aggr, float* pos_aggr,
                          float* save_xhat, int save_planes, float* save_rstd, void* stream);
/* Flags of the _ex entry points (0: the forms above).
 * GMP_EGNN_NO_POS_BRANCH: nobody reads this layer's position output (egnn.py's last layer
 *   without equivariant_pred).  Forward: mlp_pos is not evaluated — no W3 product, LN3 or w4 dot;
 *   pos_aggr (may be NULL) and column 2 of save_rstd are not written; m_aggr, save_xhat's first
 *   two planes and save_rstd[:, 0:2] are bitwise those of flags = 0.  Backward: g_pos_aggr is
 *   taken as zero (g_pos_aggr, dpre3 may be NULL; x_hat3 and save_rstd[:, 2] are not read); the
 *   ln3_w / ln3_b / w4 / b4 slots of vec_partials are zeros, amax[1] is left alone, every other
 *   output is bitwise that of flags = 0 with a zero g_pos_aggr.
 * GMP_EGNN_NO_POS_GRAD (backward only): the caller wants no gradient w.r.t. pos; dpos_recv and
 *   gdiff (may be NULL) are not written, every other output unchanged. */
#define GMP_EGNN_NO_POS_BRANCH 1u
#define GMP_EGNN_NO_POS_GRAD 2u
int gmp_egnn_edge_fwd_ex_f32(int64_t n_nodes, int64_t n_edges, int64_t d, const float* AB,
                             const float* pos, const int64_t* rowptr, const int64_t* recv,
                             const int64_t* send, const gmp_egnn_params* params, int act,
                             int msg_mean, float ln_eps, float* m_aggr, float* pos_aggr,
                             float* save_xhat, int save_planes, float* save_rstd, uint32_t flags,
                             void* stream);

/* K15 (r05): the EGNN node update of one layer and the next layer's node projections in one
 * launch — replaces egnn_layer.py:82-86 (update: mlp_upd(cat([h, m_aggr]))), egnn.py:75-76 (the
 * residual h + h_update) and the AB = [h W1a^T | h W1b^T] projection of the next layer's
 * mlp_msg.0 (egnn_layer.py:28-29; the node half of gmp_egnn_edge_fwd_f32's split Linear):
 *   x1 = act(LN1(W0 [h | m_aggr] + b0)); x2 = act(LN2(W3 x1 + b3));
 *   h_out = (residual ? h + x2 : x2);  ab_out = [h_out W1n[:, :d]^T | h_out W1n[:, d:2d]^T]
 * W0 = mlp_upd.0.weight (d, 2d) row-major; W3 = mlp_upd.3.weight (d, d); W1n = the next layer's
 * mlp_msg.0.weight (d, 2d + 1) with row stride ld1 (>= 2d), or NULL (that layer has no ab_out).
 * The three matrices enter as a weight IMAGE (2-plane fp16 tiles with per-16-row power-of-two
 * scales, the layout the kernel copies into LDS): gmp_egnn_node_image_f32 builds the images of
 * n_layers layers (params: a host array of n_layers structs) into `images`
 * (n_layers x gmp_egnn_node_image_bytes(d) bytes, 16-byte aligned) in one launch; rebuild after
 * every weight change.  gmp_egnn_node_fwd_f32 reads this layer's image and, from params, the
 * vectors b0, ln1_w, ln1_b, b3, ln2_w, ln2_b; ab_out non-NULL only if the image holds W1n.
 * save_xhat ((2, N, d): the two LayerNorm outputs) and save_rstd ((2, N): their 1/std) both NULL
 * (inference) or both set (training; the LayerNorm backwards read them).  Products as
 * gmp_egnn_edge_fwd_f32's HF path (2-plane fp16 splits, f32 accumulation); GMP_ERR_UNSUPPORTED
 * under gmp_egnn_set_f32_mfma(1) and for d outside {32, 64, 128}. */
typedef struct gmp_egnn_node_params {
  const float* W0;   /* (d, 2d) mlp_upd.0.weight */
  const float* b0;   /* (d) */
  const float* ln1_w;
  const float* ln1_b;
  const float* W3;   /* (d, d) mlp_upd.3.weight */
  const float* b3;
  const float* ln2_w;
  const float* ln2_b;
  const float* W1n;  /* next layer's mlp_msg.0.weight (d, 2d + 1), row stride ld1; or NULL */
  int64_t ld1;
} gmp_egnn_node_params;
size_t gmp_egnn_node_image_bytes(int64_t d);
int gmp_egnn_node_image_f32(int64_t d, int64_t n_layers, const gmp_egnn_node_params* params,
                            void* images, void* stream);
int gmp_egnn_node_fwd_f32(int64_t n_nodes, int64_t d, const float* h, const float* m_aggr,
                          const gmp_egnn_node_params* params, const void* image, int act,
                          int residual, float ln_eps, float* h_out, float* ab_out,
                          float* save_xhat, float* save_rstd, void* stream);

/* K15b (r06): backward of gmp_egnn_node_fwd_f32 (egnn_layer.py:82-86 update, egnn.py:75-76
 * residual) in one launch, from grad_h (N, d) of h_out and the forward's save_xhat (2, N, d),
 * save_rstd (2, N):  dz2 = grad_h act'(x_hat2 ln2_w + ln2_b), dpre2 = LN2'(dz2 ln2_w);
 * dz1 = (W3^T dpre2) act'(x_hat1 ln1_w + ln1_b), dpre1 = LN1'(dz1 ln1_w);
 * dh = W0[:, :d]^T dpre1 (+ grad_h when residual), dm = W0[:, d:]^T dpre1 (the m_aggr gradient);
 * dpre1, dpre2 (N, d) out for the weight sums (dW0 = dpre1^T [h | m], dW3 = dpre2^T
 * act(x_hat1 ln1_w + ln1_b)); partials (gmp_egnn_node_bwd_partial_rows(N), 4 d) per-workgroup rows
 * of [d ln1_w | d ln1_b | d ln2_w | d ln2_b], the caller sums them in row order.  W0 (d, 2d),
 * W3 (d, d) f32 row-major (not the forward's image); exact f32 products; d in {32, 64, 128}
 * (GMP_ERR_UNSUPPORTED otherwise), act 0 relu / 1 swish. */
int64_t gmp_egnn_node_bwd_partial_rows(int64_t n_nodes);
int gmp_egnn_node_bwd_f32(int64_t n_nodes, int64_t d, int act, int residual, const float* grad_h,
                          const float* save_xhat, const float* save_rstd, const float* W0,
                          const float* W3, const float* ln1_w, const float* ln1_b,
                          const float* ln2_w, const float* ln2_b, float* dh, float* dm,
                          float* dpre1, float* dpre2, float* partials, void* stream);
/* Backward of gmp_egnn_edge_fwd_f32 from its saved x_hat / rstd (no forward recompute).
 * Inputs g_m_aggr (N,d), g_pos_aggr (N,3), the forward's save_xhat (save_planes, E, d) and
 * save_rstd (E, 3).  Outputs:
 *   dA        (N,d)  receiver part of d(AB)[:, :d]   (segment-summed in-kernel)
 *   dpos_recv (N,3)  receiver part of d(pos)          (segment-summed in-kernel)
 *   per edge, in receiver-sorted order (row e):
 *     dpre1 (E,d)  grad of the first pre-activation   -> caller reduces by sender for
 *                  d(AB)[:, d:], and takes db1 = sum_e dpre1
 *     gdiff (E,3)  grad of rel                         -> caller: dpos[send] -= gdiff
 *     dpre2, dpre3 (E,d)                               -> caller: dW2 = dpre2^T y1,
 *                  dW3 = dpre3^T m, db2 = sum dpre2, db3 = sum dpre3, with y1 / m rebuilt
 *                  from x_hat1 / x_hat2 inside gmp_edge_outer_sum_act_f32
 *   vec_partials (n_blocks, 8*d+1): per-workgroup partial sums of
 *     [dln1_w, dln1_b, dln2_w, dln2_b, dln3_w, dln3_b, dw4, dw1d, db4]   (caller sums rows;
 *     n_blocks from gmp_egnn_edge_bwd_partials_rows). Deterministic. */
int64_t gmp_egnn_edge_bwd_partials_rows(int64_t n_edges, int64_t d);
int gmp_egnn_edge_bwd_f32(int64_t n_nodes, int64_t n_edges, int64_t d, const float* pos,
                          const int64_t* rowptr, const int64_t* recv, const int64_t* send,
                          const gmp_egnn_params* params, int act, int msg_mean,
                          const float* save_xhat, int save_planes, const float* save_rstd,
                          const float* g_m_aggr, const float* g_pos_aggr, float* dA,
                          float* dpos_recv, float* dpre1, float* gdiff, float* dpre2, float* dpre3,
                          float* vec_partials, void* stream);
/* As gmp_egnn_edge_bwd_f32, also folding max |dpre2| and max |dpre3| into amax[0], amax[1]
 * (float bit patterns, atomic max; caller zeroes): the A scales of the HF weight-gradient outer
 * sums (gmp_edge_outer_sum_act_hf_f32). */
int gmp_egnn_edge_bwd_amax_f32(int64_t n_nodes, int64_t n_edges, int64_t d, const float* pos,
                               const int64_t* rowptr, const int64_t* recv, const int64_t* send,
                               const gmp_egnn_params* params, int act, int msg_mean,
                               const float* save_xhat, int save_planes, const float* save_rstd,
                               const float* g_m_aggr, const float* g_pos_aggr, float* dA,
                               float* dpos_recv, float* dpre1, float* gdiff, float* dpre2,
                               float* dpre3, float* vec_partials, uint32_t* amax, void* stream);
/* As gmp_egnn_edge_bwd_amax_f32 (amax may be NULL) with the GMP_EGNN_* flags above. */
int gmp_egnn_edge_bwd_ex_f32(int64_t n_nodes, int64_t n_edges, int64_t d, const float* pos,
                             const int64_t* rowptr, const int64_t* recv, const int64_t* send,
                             const gmp_egnn_params* params, int act, int msg_mean,
                             const float* save_xhat, int save_planes, const float* save_rstd,
                             const float* g_m_aggr, const float* g_pos_aggr, float* dA,
                             float* dpos_recv, float* dpre1, float* gdiff, float* dpre2,
                             float* dpre3, float* vec_partials, uint32_t* amax, uint32_t flags,
                             void* stream);

/* ------------------------------------------------------------------------------------------
 * Edge-reduction GEMM for per-edge Linear weight gradients (egnn_layer.py:28-39 mlp_msg /
 * mlp_pos backward; replaces torch's dW = dpre^T x over E rows):
 *   C (d x d) = A^T B with A (K, d), B (K, d) row-major fp32, K = edges;
 *   colsum_A (d) = sum_k A[k, :] (the bias gradient; may be NULL).
 * Split-K over workgroups, partial slabs in `workspace` and an ordered second pass: bitwise
 * deterministic.  d in {32, 64, 128}.  Arithmetic (all outer-sum entry points below): f32
 * operands split exactly into three bf16 planes on the bf16 MFMA with f32 accumulation, the
 * six partial products of order <= 2^-16 summed (error vs fp64 <= 2^-26 of sum |a b|, within
 * 2x of the f32-MFMA kernels', below rocBLAS f32 GEMM's); gmp_wgrad_set_f32_mfma(1) selects the f32-MFMA
 * kernels instead, returns the previous setting.
 * ------------------------------------------------------------------------------------------ */
int gmp_wgrad_set_f32_mfma(int on);
size_t gmp_edge_outer_sum_workspace_size(int64_t K, int64_t d);
int gmp_edge_outer_sum_f32(int64_t K, int64_t d, const float* A, const float* B, float* C,
                           float* colsum_A, void* workspace, size_t workspace_bytes,
                           void* stream);
/* Same with the activation rebuilt from a saved LayerNorm output at load time:
 * C = A^T act(X * w + b) (+ colsum_A = colsum(A)), w, b per column (d), act 0 = relu, 1 = silu
 * (the EGNN y1 / m of egnn_layer.py:28-34 from x_hat1 / x_hat2).  Workspace as above. */
int gmp_edge_outer_sum_act_f32(int64_t K, int64_t d, const float* A, const float* X,
                               const float* w, const float* b, int act, float* C,
                               float* colsum_A, void* workspace, size_t workspace_bytes,
                               void* stream);
/* HF form of gmp_edge_outer_sum_act_f32 for LayerNorm rows X (|X| <= sqrt(d), the EGNN x_hat):
 * two scaled fp16 planes per operand, three MFMA products per stage (22-bit operands, f32
 * accumulation; ~2^-21 relative per product).  amax_A: device word holding max |A| as a float
 * bit pattern (gmp_egnn_edge_bwd_amax_f32 produces it for dpre2 / dpre3); B's scale comes from
 * sqrt(d) max|w| + max|b|.  Falls back to the split-plane x3 / f32-MFMA paths where those apply
 * (node-level K, gmp_wgrad_set_f32_mfma(1)). */
int gmp_edge_outer_sum_act_hf_f32(int64_t K, int64_t d, const float* A, const float* X,
                                  const float* w, const float* b, int act, const uint32_t* amax_A,
                                  float* C, float* colsum_A, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* Rectangular variant (GVP message GVPs, gvp_layer.py:101-170 applied per edge at :319-324):
 * C (m x n) = A^T B, A (K, m), B (K, n) row-major, m, n multiples of 16, m <= 256,
 * (m/16)(n/16) <= 72; colsum_A (m) optional.  Same deterministic split-K reduction. */
size_t gmp_edge_outer_sum_rect_workspace_size(int64_t K, int64_t m, int64_t n);
/* gmp_edge_xyz_dot_f32 (r05): out[c] = sum_e sum_x A[e, 3c + x] v[e, x] for A (K, 3C) contiguous
 * 16-byte aligned, v (K, 3), C in {16, 48} (GMP_ERR_UNSUPPORTED otherwise): the xyz
 * contractions of the GVP first message's weight sums (sum dvpre . ev, sum dvh . ev,
 * gvp_layer.py:101-170 through the e_v column of W_h) in one pass over A; per-workgroup partial
 * rows in the workspace, added in a fixed order (deterministic). */
size_t gmp_edge_xyz_dot_workspace_size(int64_t K);
int gmp_edge_xyz_dot_f32(int64_t K, int64_t C, const float* A, const float* v, float* out,
                         void* workspace, size_t workspace_bytes, void* stream);
int gmp_edge_outer_sum_rect_f32(int64_t K, int64_t m, int64_t n, const float* A, const float* B,
                                float* C, float* colsum_A, void* workspace,
                                size_t workspace_bytes, void* stream);
/* General form (strided operands and output): C (m x n, row stride ldc) = A^T act(B),
 * A (K, m) with row stride lda, B (K, n) with row stride ldb (lda, ldb multiples of 4, A and B
 * 16-byte aligned), colsum_A (m) optional; act -1 = none, 0 = relu(B*w + b), 1 = silu(B*w + b)
 * (the activation prologue needs m == n in {32, 64, 128}).  Lets a Linear's weight gradient
 * be written straight into a column block of a wider parameter (egnn_layer.py:28 W1 =
 * [W1a | W1b | w1d]; :37 mlp_upd[0] over [h | m_aggr]) without concatenated copies.
 * Square 32/64/128 shapes use the square kernel, others the rectangular one. */
/* Two B operands as one: C (m x (n1 + n2)) = A^T [B1 | B2] for outer sums that share A (GVP:
 * dspre against [s | vn]), one pass over A; workspace gmp_edge_outer_sum_rect_workspace_size(K,
 * m, n1 + n2).  Split-plane path only: returns GMP_ERR_UNSUPPORTED where it does not apply
 * (narrow products, node-level K, f32-MFMA mode) — the caller then makes two calls. */
int gmp_edge_outer_sum_ex2_f32(int64_t K, int64_t m, int64_t n1, int64_t n2, const float* A,
                               int64_t lda, const float* B1, int64_t ldb1, const float* B2,
                               int64_t ldb2, float* C, int64_t ldc, float* colsum_A,
                               void* workspace, size_t workspace_bytes, void* stream);
size_t gmp_edge_outer_sum_ex_workspace_size(int64_t K, int64_t m, int64_t n);
/* Which kernel gmp_edge_outer_sum_ex_f32 runs for these sizes and strides in the current
 * gmp_wgrad_set_f32_mfma mode: host arithmetic only, no HIP call, and the very decision the
 * launch takes.  GMP_ERR_ARG for invalid arguments (valid: K >= 0, m and n positive multiples
 * of 16, lda >= m, ldb >= n, both strides multiples of 4, act in -1..1), else one of the values
 * below.  GMP_WGRAD_ROUTE_LIBRARY: no kernel applies and gmp_edge_outer_sum_ex_f32 returns
 * GMP_ERR_UNSUPPORTED (the caller runs the library GEMM); every valid shape outside the
 * kernels' buckets gets it, at K = 0 too. */
enum {
  GMP_WGRAD_ROUTE_ZERO = 1,       /* K = 0: C and colsum_A zero-filled */
  GMP_WGRAD_ROUTE_X3 = 2,         /* three bf16 planes, K >= 262144 */
  GMP_WGRAD_ROUTE_QUAD = 3,       /* node-level 64 x 64 quadrants, 0 < K < 262144 */
  GMP_WGRAD_ROUTE_SQUARE_F32 = 4, /* f32-MFMA square kernel, d in {32, 64, 128} */
  GMP_WGRAD_ROUTE_RECT_F32 = 5,   /* f32-MFMA rectangular buckets, m <= 256 */
  GMP_WGRAD_ROUTE_LIBRARY = 6     /* none: the caller's library GEMM */
};
int gmp_edge_outer_sum_ex_route(int64_t K, int64_t m, int64_t n, int64_t lda, int64_t ldb,
                                int act);
int gmp_edge_outer_sum_ex_f32(int64_t K, int64_t m, int64_t n, const float* A, int64_t lda,
                              const float* B, int64_t ldb, int act, const float* w, const float* b,
                              float* C, int64_t ldc, float* colsum_A, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * K1 per-edge featurisation (models/mace.py:170-174, models/tfn.py:171-175,
 * models/mace_modules/radial.py:44-46,71-78, blocks.py:91-96; e3nn SphericalHarmonics(l<=2,
 * normalize=True, 'component')):
 *   vec = pos[ei0] - pos[ei1] (E,3); len = |vec| (E); sh (E,9); radial = bessel * cutoff (E,nb)
 * edge_index is (2, E) int64 (row 0 then row 1).  `bessel_weights` is a HOST array of nb floats
 * (the module buffer, copied into the kernel arguments).  Any output pointer may be NULL.
 * Backward: g_vec (E,3) from g_sh / g_radial (either may be NULL); the caller scatters g_vec to
 * pos[ei0] (+) and pos[ei1] (-).
 * Cutoff: an edge with len >= r_max (len == r_max included) gets a radial row of zeros (signed:
 * -0.0 where the Bessel factor is negative, as the reference's product gives) and contributes
 * exactly +0.0 to g_vec through g_radial; sh and its gradient do not depend on r_max.
 * Zero-length edges (vec == 0: coincident nodes, or a self-loop (a, a)).  Forward, as the
 * reference gives: sh = (1, 0, ..., 0), the radial row is NaN (sin(0) / 0), the GVP unit row is
 * 0.  Backward: g_vec is exactly 0 from each of g_sh, g_radial and g_unit for finite cotangents
 * (the reference's autograd returns NaN there).  The forward normalises with 1 / max(len, 1e-12)
 * (F.normalize's eps) while the backward of sh is gated on len > 1e-12 and those of radial / unit
 * on len > 0; vectors so short that len^2 underflows in fp32 (|vec| below about 1e-19) or that
 * fall between the two gates are outside what the tests pin.
 * ------------------------------------------------------------------------------------------ */
int gmp_edge_featurize_f32(const float* pos, const int64_t* edge_index, int64_t n_edges,
                           int num_bessel, const float* bessel_weights, float prefactor,
                           float r_max, float p_cutoff, float* vec_out, float* len_out,
                           float* sh_out, float* radial_out, void* stream);
int gmp_edge_featurize_bwd_f32(const float* pos, const int64_t* edge_index, int64_t n_edges,
                               int num_bessel, const float* bessel_weights, float prefactor,
                               float r_max, float p_cutoff, const float* g_sh,
                               const float* g_radial, float* g_vec, void* stream);
/* The same for SphericalHarmonics(lmax) with 0 <= lmax <= 5 (max_ell of models/tfn.py:51 /
 * mace.py:25; anything else is GMP_ERR_ARG, as is num_bessel outside 0..32): sh rows of
 * (lmax + 1)^2 floats, the l = 3 block being e3nn's component-normalised sh_3_m and the l = 4, 5
 * blocks e3nn's CG recursion from it (the lmax = 2 entries above are these with lmax = 2).
 * lmax = 0: sh == 1 and g_sh contributes exactly 0 to g_vec.  num_bessel = 0: no radial output
 * is written and g_vec comes from g_sh alone. */
int gmp_edge_featurize_lmax_f32(const float* pos, const int64_t* edge_index, int64_t n_edges,
                                int lmax, int num_bessel, const float* bessel_weights,
                                float prefactor, float r_max, float p_cutoff, float* vec_out,
                                float* len_out, float* sh_out, float* radial_out, void* stream);
int gmp_edge_featurize_lmax_bwd_f32(const float* pos, const int64_t* edge_index,
                                    int64_t n_edges, int lmax, int num_bessel,
                                    const float* bessel_weights, float prefactor, float r_max,
                                    float p_cutoff, const float* g_sh, const float* g_radial,
                                    float* g_vec, void* stream);
/* The same with a per-edge Cartesian shift (E,3) added to vec (periodic images, K9p:
 * vec = (pos[ei0] - pos[ei1]) + shift).  shift == NULL is the entry point above, bit for bit
 * (and takes no workspace).  With a shift, a first pass writes the shifted vectors and a
 * redirected edge list into `workspace` (DEVICE, 16-byte aligned,
 * gmp_featurize_shift_workspace_size(n_edges) bytes) and the same kernel runs on them, so
 * shift = zeros gives bitwise the NULL result.  The backward formulas are unchanged and the
 * cotangent of shift is g_vec itself.  The SchNet entry points below follow the same rule. */
size_t gmp_featurize_shift_workspace_size(int64_t n_edges);
int gmp_edge_featurize_lmax_ex_f32(const float* pos, const int64_t* edge_index, int64_t n_edges,
                                   int lmax, int num_bessel, const float* bessel_weights,
                                   float prefactor, float r_max, float p_cutoff,
                                   const float* shift, void* workspace, size_t workspace_bytes,
                                   float* vec_out, float* len_out, float* sh_out,
                                   float* radial_out, void* stream);
int gmp_edge_featurize_lmax_bwd_ex_f32(const float* pos, const int64_t* edge_index,
                                       int64_t n_edges, int lmax, int num_bessel,
                                       const float* bessel_weights, float prefactor, float r_max,
                                       float p_cutoff, const float* shift, void* workspace,
                                       size_t workspace_bytes, const float* g_sh,
                                       const float* g_radial, float* g_vec, void* stream);
/* GVP-GNN edge features (models/gvpgnn.py:106-112): len (E), radial (E,nb) as above and the unit
 * vectors nan_to_num(vec / len) (E,3; zero rows for zero-length edges).  Backward from g_radial /
 * g_unit (either may be NULL) to g_vec. */
int gmp_edge_featurize_gvp_f32(const float* pos, const int64_t* edge_index, int64_t n_edges,
                               int num_bessel, const float* bessel_weights, float prefactor,
                               float r_max, float p_cutoff, float* len_out, float* radial_out,
                               float* unit_out, void* stream);
int gmp_edge_featurize_gvp_bwd_f32(const float* pos, const int64_t* edge_index, int64_t n_edges,
                                   int num_bessel, const float* bessel_weights, float prefactor,
                                   float r_max, float p_cutoff, const float* g_radial,
                                   const float* g_unit, float* g_vec, void* stream);
/* SchNet edge features (models/schnet.py:66-68; PyG 2.3.1 SchNet.forward, GaussianSmearing,
 * CFConv.forward): dist = |pos[row] - pos[col]| (E), rbf[e, k] = exp(coeff (dist - offsets[k])^2)
 * (E,G), cut = 0.5 (cos(dist pi / cutoff) + 1) (E).  `offsets` is the module's DEVICE buffer
 * (G <= 256).  Any output may be NULL.  Backward: g_vec (E,3) from g_dist / g_rbf / g_cut (any
 * may be NULL); the caller scatters g_vec to pos[row] (+) and pos[col] (-). */
int gmp_schnet_featurize_f32(const float* pos, const int64_t* edge_index, int64_t n_edges,
                             int num_gaussians, const float* offsets, float coeff, float cutoff,
                             float* dist_out, float* rbf_out, float* cut_out, void* stream);
int gmp_schnet_featurize_bwd_f32(const float* pos, const int64_t* edge_index, int64_t n_edges,
                                 int num_gaussians, const float* offsets, float coeff,
                                 float cutoff, const float* g_dist, const float* g_rbf,
                                 const float* g_cut, float* g_vec, void* stream);
/* Second order (energy-and-force training): the backward above, g_vec = s(dist) u with u = vec /
 * dist and s = g_dist + sum_k g_rbf[k] rbf'_k + g_cut cut', differentiated once more.  a_vec (E,3)
 * is the cotangent of g_vec and p = a_vec . u:
 *   gg_dist (E) = p, gg_rbf (E,G) = rbf'_k p, gg_cut (E) = cut' p  (cotangents of g_dist / g_rbf /
 *   g_cut), h_vec (E,3) = s' p u + (s / dist)(a_vec - p u)  (cotangent of vec; the caller
 *   scatters it to pos as g_vec above).
 * g_dist / g_rbf / g_cut and every output may be NULL.  Zero-length edges, and edges with an
 * endpoint outside [0, n_nodes) (never read), give zeros in every output. */
int gmp_schnet_featurize_bwd2_f32(const float* pos, int64_t n_nodes, const int64_t* edge_index,
                                  int64_t n_edges, int num_gaussians, const float* offsets,
                                  float coeff, float cutoff, const float* g_dist,
                                  const float* g_rbf, const float* g_cut, const float* a_vec,
                                  float* gg_dist, float* gg_rbf, float* gg_cut, float* h_vec,
                                  void* stream);
/* The three SchNet entry points with a per-edge Cartesian shift (E,3) added to the edge vector
 * (periodic images, K9p: dist = |(pos[row] - pos[col]) + shift|).  shift == NULL is the entry
 * point above, bit for bit; workspace as for gmp_edge_featurize_lmax_ex_f32.  The cotangent of
 * shift is g_vec (h_vec in the second backward). */
int gmp_schnet_featurize_ex_f32(const float* pos, const int64_t* edge_index, int64_t n_edges,
                                int num_gaussians, const float* offsets, float coeff,
                                float cutoff, const float* shift, void* workspace,
                                size_t workspace_bytes, float* dist_out, float* rbf_out,
                                float* cut_out, void* stream);
int gmp_schnet_featurize_bwd_ex_f32(const float* pos, const int64_t* edge_index, int64_t n_edges,
                                    int num_gaussians, const float* offsets, float coeff,
                                    float cutoff, const float* shift, void* workspace,
                                    size_t workspace_bytes, const float* g_dist,
                                    const float* g_rbf, const float* g_cut, float* g_vec,
                                    void* stream);
int gmp_schnet_featurize_bwd2_ex_f32(const float* pos, int64_t n_nodes, const int64_t* edge_index,
                                     int64_t n_edges, int num_gaussians, const float* offsets,
                                     float coeff, float cutoff, const float* shift,
                                     void* workspace, size_t workspace_bytes, const float* g_dist,
                                     const float* g_rbf, const float* g_cut, const float* a_vec,
                                     float* gg_dist, float* gg_rbf, float* gg_cut, float* h_vec,
                                     void* stream);

/* ------------------------------------------------------------------------------------------
 * K16 irreps epilogues of the TP convolution (models/layers/tfn_layer.py:89-92), row-major
 * (B, C) fp32 node features, all tables int32 on the DEVICE (built once per module):
 * Gate (e3nn nn.Gate, tfn_layer.py:45-63): y = [c_act silu(scalars), gated * c_gate
 *   sigmoid(gates)]; out_map (c_out, 2) = {source col, gate col or -1}; in_map (c_in, 4) =
 *   {kind 0 scalar / 1 gate / 2 gated, a, b, d} (gmp_irreps.hip header).
 * BatchNorm (e3nn nn.BatchNorm, component normalisation, affine): col_chan (C) channel of each
 *   column, chan_col (nf) first column of each channel, chan_info (nf, 2) = {2l+1, scalar index
 *   or -1}.  Training: batch statistics (fixed-order partial sums) and running-stat update in
 *   place (momentum); eval: running statistics.  save_shift / save_invstd (nf) feed the
 *   backward, which writes grad_x and grad_weight (nf) / grad_bias (number of scalar channels).
 * ------------------------------------------------------------------------------------------ */
int gmp_gate_fwd_f32(int64_t B, int c_in, int c_out, const int32_t* out_map, float c_act,
                     float c_gate, const float* x, float* y, void* stream);
int gmp_gate_bwd_f32(int64_t B, int c_in, int c_out, const int32_t* in_map, float c_act,
                     float c_gate, const float* x, const float* grad_y, float* grad_x,
                     void* stream);
size_t gmp_irreps_bn_workspace_size(int64_t B, int C, int nf);
int gmp_irreps_bn_fwd_f32(int64_t B, int C, int nf, const int32_t* col_chan,
                          const int32_t* chan_col, const int32_t* chan_info, const float* x,
                          const float* weight, const float* bias, float* running_mean,
                          float* running_var, int training, float momentum, float eps, float* y,
                          float* save_shift, float* save_invstd, void* workspace,
                          size_t workspace_bytes, void* stream);
int gmp_irreps_bn_bwd_f32(int64_t B, int C, int nf, const int32_t* col_chan,
                          const int32_t* chan_col, const int32_t* chan_info, const float* x,
                          const float* grad_y, const float* weight, const float* save_shift,
                          const float* save_invstd, int training, float* grad_x,
                          float* grad_weight, float* grad_bias, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * K7 tensor-product convolution messages (models/layers/tfn_layer.py:82-86): e3nn
 * FullyConnectedTensorProduct(in1, 1x0e+1x1o+1x2e, out, shared_weights=False) applied per edge
 * with per-edge weights W (chunk rows x weight_numel, produced by the radial MLP
 * tfn_layer.py:73-77).  The receiver sum of tfn_layer.py:87 (scatter(tp, ei[0], 'sum')) is the
 * segmented reduce above over the same receiver-sorted order.
 * Edges are addressed by their position k in the stable CSR of edge_index[0]:
 *   src_sorted[k] = ei1 of sorted edge k, perm[k] = original edge id, recv_sorted[k] = ei0.
 * x (N, in_dim) mul_ir; sh (E, 9) in ORIGINAL edge order; W row r = sorted edge c0 + r.
 * Forward writes msg rows c0..c1-1 (E x out_dim, sorted positions).
 * desc_host: host pointer to the descriptor {int n_paths, in_dim, out_dim, sh_dim;
 *   int64 weight_numel; int z_size, n_blocks; int blk_off[8], blk_mul[8], blk_l[8];}
 *   (128 bytes since ABI 3; <= 48 paths, <= 8 output blocks).  The per-edge-weight kernels below take l <= 2 (sh_dim 9, the
 *   two layouts); the node-form z / dz kernels (gmp_tp_edge_z*) take l <= 3 (sh_dim (lmax+1)^2
 *   <= 16, any block structure: max_ell = 3 models).
 * paths_dev: device array of 64-byte path records {int l1, l2, lo, mul1, mul_out, x_off, y_off,
 *   io, out_off, z_off, cg_off, pad; int64 w_off; float alpha, pad}; cg_dev: concatenated
 *   real CG tensors (cg_len floats).  layout: 0 = out blocks (0e,1o,2e), 1 = (0e,0e,1o,2e).
 *   Multiplicities <= 128 and multiples of 4.
 * Backward (per chunk): dW (chunk rows x weight_numel), dx_edge (E, in_dim) and dY_edge (E, 9)
 * at SORTED positions, given gout = dL/dout (N, out_dim) of the receiver sums.
 * ------------------------------------------------------------------------------------------ */
int gmp_tp_conv_fwd_f32(int layout, const void* desc_host, const void* paths_dev,
                        const float* cg_dev, int cg_len, const float* x, const float* sh,
                        const float* W, const int64_t* src_sorted, const int64_t* perm,
                        int64_t c0, int64_t c1, float* msg, void* stream);
int gmp_tp_conv_bwd_f32(int layout, const void* desc_host, const void* paths_dev,
                        const float* cg_dev, int cg_len, const float* x, const float* sh,
                        const float* W, const int64_t* recv_sorted, const int64_t* src_sorted,
                        const int64_t* perm, int64_t c0, int64_t c1, const float* gout,
                        float* dW, float* dx_edge, float* dY_edge, void* stream);

/* K7 receiver-factorised form helpers: per-edge z rows (alpha_p sum_ij C x Y) for the edges
 * [e0, e1) of a receiver chunk, in path-major layout: path p region starts at
 * z_off_p * (n_e + 1) floats (n_e = e1 - e0) and holds (n_e + 1) rows of (2lo+1) * mul1 floats,
 * k-major then u; row n_e is a padding row the kernels never write.  The backward maps dz (same
 * layout) to dx_edge (n_e, in_dim) and dY_edge (n_e, 9) for those edges (sorted positions).  */
int gmp_tp_edge_z_f32(const void* desc_host, const void* paths_dev, const float* cg_dev,
                      int cg_len, const float* x, const float* sh, const int64_t* src_sorted,
                      const int64_t* perm, int64_t e0, int64_t e1, float* zbuf, void* stream);
int gmp_tp_edge_z_bwd_f32(const void* desc_host, const void* paths_dev, const float* cg_dev,
                          int cg_len, const float* x, const float* sh, const int64_t* src_sorted,
                          const int64_t* perm, int64_t e0, int64_t e1, const float* dzbuf,
                          float* dx_edge, float* dY_edge, void* stream);
/* Same with l_max = the largest l of any path (input, SH or output irreps; 0..3): with
 * l_max <= 2 the kernels are the l <= 2 instantiation (fewer registers, more waves per SIMD).
 * The plain entries above are l_max = 3 (any path).  l_max 4 or 5, or sh_dim 25 or 36, select
 * the runtime-l kernels.  A path whose l exceeds l_max is not computed: its z rows stay unwritten.
 * SH layout contract: the kernels read SH component l2 * l2 + j of a path and ignore its y_off,
 * so sh rows hold exactly one irrep per l = 0..L in ascending order (sh_dim = (L + 1)^2, any
 * parities); gmp_amd.equivariant.TPPlan refuses any other irreps_sh.  dY_edge is (n_e, sh_dim). */
int gmp_tp_edge_z_lmax_f32(const void* desc_host, int l_max, const void* paths_dev,
                           const float* cg_dev, int cg_len, const float* x, const float* sh,
                           const int64_t* src_sorted, const int64_t* perm, int64_t e0, int64_t e1,
                           float* zbuf, void* stream);
int gmp_tp_edge_z_bwd_lmax_f32(const void* desc_host, int l_max, const void* paths_dev,
                               const float* cg_dev, int cg_len, const float* x, const float* sh,
                               const int64_t* src_sorted, const int64_t* perm, int64_t e0,
                               int64_t e1, const float* dzbuf, float* dx_edge, float* dY_edge,
                               void* stream);

/* K7 receiver-factorised per-receiver kernels (tfn_layer.py:73-87 regrouped): for the
 * receivers n of a chunk with chunk-local edge offsets eoff[n]..eoff[n+1] (receiver-sorted),
 * Z (n_e, w) z rows of one path, A (n_e, H) radial hidden features (H % 16 == 0, <= 256):
 *   outer: S[n, r, j] = sum_e Z[e, r] A[e, j] (n_recv, w, H), Sb[n, r] = sum_e Z[e, r]
 *   apply: dZ[e, r] = sum_j T[n, r, j] A[e, j] + Tb[n, r];  dA[e, j] += sum_r Z[e, r] T[n, r, j]
 * (T = G [W2_p]^T, Tb = G b2_p^T from the path GEMMs; dA is accumulated, dZ overwritten). */
int gmp_tp_node_outer_f32(int64_t n_recv, int64_t w, int64_t H, const int64_t* eoff,
                          const float* Z, const float* A, float* S, float* Sb, void* stream);
int gmp_tp_node_apply_f32(int64_t n_recv, int64_t w, int64_t H, const int64_t* eoff,
                          const float* Z, const float* A, const float* T, const float* Tb,
                          float* dZ, float* dA, void* stream);
/* apply runs on the bf16 MFMA over exact three-plane splits where its shapes allow (2, the
 * default: the v3 kernel for H = 256 and w % 32 == 0, then the v2 kernel for w >= 512,
 * w % 32 == 0, H % 64 == 0, 16-byte aligned operands), else on the f32 MFMA; set_x3(1) skips the
 * v3 kernel, set_x3(0) forces the f32 one (tests cover every form).  Returns the previous
 * setting. */
int gmp_tp_apply_set_x3(int on);

/* K7g path GEMMs of the receiver-factorised TP convolution on the bf16 MFMA through exact
 * three-plane f32 splits (replaces the library f32 GEMMs out = S W2p + Sb b2p and
 * T = G W2p^T of tfn_layer.py:73-87 regrouped; f32-class accuracy, see gmp_tpgemm.hip).
 * split_w2: from one path's block of the second radial Linear, W2p (mul1 * mul_out rows (u, w)
 *   of H floats) and b2p (mul1 * mul_out), writes (each if not null) the forward B planes Bf
 *   (bf16 values B[p][w][u H + j] = W2[(u, w), j], B[p][w][mul1 H + u] = b2[u, w], stored in
 *   MFMA fragment order, below; mul_out % 16 == 0) and the backward B planes Bt (values
 *   B[p][u H + j][w] = W2[(u, w), j], an N = mul1 H by K = mul_out operand in the same fragment
 *   order; mul_out % 32 == 0).
 * gemm_x3: C (+)= [A1 | A2] B^T for A1 (M x K1, row stride lda1), A2 (M x K2, lda2; K2 may be 0),
 *   B = 3 bf16 planes of an N x (K1 + K2) operand in fragment order: value (p, n, k) at
 *   ((((k / 32) (N / 16) + n / 16) 3 + p) 64 + n % 16 + 16 ((k % 32) / 8)) 8 + k % 8 (each
 *   64-lane block is one v_mfma_f32_16x16x32 B operand; the kernel loads it straight into
 *   registers); ldb = K1 + K2 and bplane = N ldb are checked (the dense sizes); N % 16 == 0.
 *   Element (r, col) of C at (r / cgrp) cldg + (r % cgrp) cldr + col cldn (accumulate != 0:
 *   C += result).  K1, K2 multiples of 32; lda* multiples of 4; A, B 16-byte aligned.
 *   Deterministic (no atomics, fixed k order). */
int gmp_tp_split_w2_f32(int64_t mul1, int64_t mul_out, int64_t H, const float* W2p,
                        const float* b2p, void* Bf, void* Bt, void* stream);
int gmp_tp_gemm_x3_f32(int64_t M, int64_t N, int64_t K1, const float* A1, int64_t lda1,
                       int64_t K2, const float* A2, int64_t lda2, const void* Bp, int64_t ldb,
                       int64_t bplane, float* C, int64_t cgrp, int64_t cldg, int64_t cldr,
                       int64_t cldn, int accumulate, void* stream);
/* Short-K, wide-N form of gemm_x3 (the backward T = G W2p^T: K = mul_out <= 128, N = mul1 H):
 *   C (M x N, row stride ldc) = A B^T, A (M x K, lda) f32, B = 3 bf16 planes of the N x K
 *   operand in gemm_x3's fragment order (ldb = K, bplane = N K checked; N % 16 == 0);
 * K a multiple of 32, <= 128.  Each workgroup keeps its split A rows in LDS and sweeps a range
 * of column tiles with B loaded straight into registers; C is written with non-temporal
 * stores. */
int gmp_tp_gemm_x3_widen_f32(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                             const void* Bp, int64_t ldb, int64_t bplane, float* C, int64_t ldc,
                             void* stream);
/* Wide edge/row reduction C (m_total x n, row stride ldc) = A^T B over K rows, A (K x m_total,
 * row stride lda), B (K x n, ldb), m_total a multiple of 128, n a multiple of 16 (<= 128): the
 * TP path GEMM dW2p = S^T G.  Split-plane bf16 MFMA (the K5 kernel with column blocks of 128),
 * deterministic split-K reduction through the workspace. */
size_t gmp_outer_sum_cols_workspace_size(int64_t K, int64_t m_total, int64_t n);
int gmp_outer_sum_cols_f32(int64_t K, int64_t m_total, int64_t n, const float* A, int64_t lda,
                           const float* B, int64_t ldb, float* C, int64_t ldc, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * K5g GVP-GNN message function (models/layers/gvp_layer.py:101-170 per edge via GVPConv.message
 * :319-324; configuration of models/gvpgnn.py: activations (relu, None), vector_gate, s = 128,
 * v = 16, edge (32, 1)).  Vector tensors in the reference's (channel, xyz) row layout.
 *   gmp_gvp_layer_*: one GVP (128, 16) -> (128, 16) on E rows; Ws (128 x 144) = ws.weight on
 *     [s | |vh|], Wsv (16 x 128), Wh, Wv (16 x 16); relu = scalar activation on/off.  Backward
 *     writes ds_in, dv_in and the per-edge weight-gradient factors dspre, spre (E,128),
 *     dgate, vn (E,16), vh, dvpre, dvh (E,48).
 *   gmp_gvp_msg0_*: the first message GVP on [s_j, e_s, s_i] / [v_j, e_v, v_i] (j = send,
 *     i = recv) from node projections P (N, 256) = [s W_a^T | s W_b^T] and Q (N, 288) =
 *     [v W_ha^T | v W_hb^T] (33 channels zero-padded to 48, (channel, xyz)), es (E, 32),
 *     ev (E, 3); We (128 x 32), Wn (128 x 48), Wv (16 x 48), wev (48) zero-padded.  Backward
 *     writes dspre, spre (E,128), dgate (E,16), vn (E,48), vh, dvh (E,144), dvpre (E,48),
 *     des (E,32), dev (E,3).
 * ------------------------------------------------------------------------------------------ */
int gmp_gvp_layer_fwd_f32(int64_t n_edges, int relu, const float* s_in, const float* v_in,
                          const float* Ws, const float* bs, const float* Wsv, const float* bsv,
                          const float* Wh, const float* Wv, float* s_out, float* v_out,
                          void* stream);
/* gmp_gvp_layer_bwd_f32: spre (the pre-activation scalar rows, only the dWsv weight sum reads
 * them) may be NULL -- the caller then forms dWsv = (sum_e dgate_e (x) [s_e | vn_e]) Ws^T +
 * (sum_e dgate_e) (x) bs without them (r04: 1 KB per edge of HBM traffic less); vh (read only
 * by dWv) may be NULL too -- dWv = (sum_(e,x) dvpre (x) v_in) Wh^T (r05: 0.4 KB per edge). */
int gmp_gvp_layer_bwd_f32(int64_t n_edges, int relu, const float* s_in, const float* v_in,
                          const float* Ws, const float* bs, const float* Wsv, const float* bsv,
                          const float* Wh, const float* Wv, const float* ds_out,
                          const float* dv_out, float* ds_in, float* dv_in, float* dspre,
                          float* spre, float* dgate, float* vn, float* vh, float* dvpre,
                          float* dvh, void* stream);
/* gmp_gvp_msg0_bwd_agg_f32: gmp_gvp_msg0_bwd_f32 walking the receiver-sorted edges (perm: original
 * edge of sorted position k, NULL if the edges are receiver-sorted; rowptr: the receiver CSR)
 * and also reducing over each receiver, in registers, the rows the receiver-side sums need:
 * dPb (n_nodes, 128) = S_i dspre, dQb (n_nodes, 144) = S_i dvh, sgate_recv (n_nodes, 16) =
 * S_i dgate, svpre_recv (n_nodes, 48) = S_i dvpre (receivers without edges: zero rows; tree
 * order inside a 16-edge chunk).  The per-edge outputs are bitwise gmp_gvp_msg0_bwd_f32's. */
int gmp_gvp_msg0_bwd_agg_f32(int64_t n_edges, int64_t n_nodes, const int64_t* send,
                             const int64_t* recv, const int64_t* perm, const int64_t* rowptr,
                             const float* P, const float* Q, const float* es, const float* ev,
                             const float* We, const float* Wn, const float* b, const float* Wv,
                             const float* Wsv, const float* bsv, const float* wev,
                             const float* ds_out, const float* dv_out, float* dspre, float* spre,
                             float* dgate, float* vn, float* vh, float* dvpre, float* dvh,
                             float* des, float* dev, float* dPb, float* dQb, float* sgate_recv,
                             float* svpre_recv, void* stream);
/* gmp_gvp_layer_fwd_agg_f32: the last message GVP of GVPConv fused with the receivers' sum /
 * mean (gvp_layer.py:319-324, aggr "add" / "mean" = reduce GMP_REDUCE_SUM / GMP_REDUCE_MEAN):
 * s_agg (n_nodes, 128), v_agg (n_nodes, 16, 3) directly, no per-edge output rows.  The receiver
 * CSR: rowptr (n_nodes + 1), skey (E) the receiver of sorted position k, perm (E) its original
 * edge (NULL: the edges are already receiver-sorted); s_in / v_in in original edge order.  Each
 * receiver's rows are summed in sorted order by an in-wave segmented scan (deterministic;
 * within fp32 rounding of K3's sequential sum); receivers without in-edges get zeros. */
int gmp_gvp_layer_fwd_agg_f32(int64_t n_edges, int64_t n_nodes, int reduce, const int64_t* perm,
                              const int64_t* skey, const int64_t* rowptr, const float* s_in,
                              const float* v_in, const float* Ws, const float* bs,
                              const float* Wsv, const float* bsv, const float* Wh,
                              const float* Wv, float* s_agg, float* v_agg, void* stream);
/* gmp_gvp_layer_bwd_agg_f32: the same backward for the last message GVP of GVPConv, whose
 * per-edge outputs feed the receivers' aggregation (gvp_layer.py:319-324, aggr "add" / "mean"
 * = reduce GMP_REDUCE_SUM / GMP_REDUCE_MEAN): ds_node (n_nodes, 128), dv_node (n_nodes, 16, 3)
 * are the aggregation's node gradients, gathered per edge at index[e] (the receiver; x 1 /
 * max(count, 1) for the mean with count = rowptr[n + 1] - rowptr[n] of the receiver CSR,
 * exactly K3's mean backward; an index outside [0, n_nodes) contributes zeros) -- the (E, 176)
 * per-edge gradient of gmp_segment_reduce_bwd_f32 is never materialised. */
int gmp_gvp_layer_bwd_agg_f32(int64_t n_edges, int64_t n_nodes, int reduce, const int64_t* index,
                              const int64_t* rowptr, int relu, const float* s_in,
                              const float* v_in, const float* Ws, const float* bs,
                              const float* Wsv, const float* bsv, const float* Wh,
                              const float* Wv, const float* ds_node, const float* dv_node,
                              float* ds_in, float* dv_in, float* dspre, float* spre,
                              float* dgate, float* vn, float* vh, float* dvpre, float* dvh,
                              void* stream);
/* gmp_gvp_edge_embed_{fwd,bwd}_f32 (K1e): the GVP-GNN edge embedding W_e (models/gvpgnn.py:73-77,
 * :116) = LayerNorm((R, 1)) then GVP((R, 1), (so, 1), activations (None, None), vector_gate,
 * h_dim 1) (gvp_layer.py:101-170, :221-243) over E edge rows: radial (E, R) row-major 16-byte
 * aligned, unit (E, 3); parameters ln_w, ln_b (R) [the LayerNorm's weight / bias, eps], wh (1)
 * [wh.weight], Ws (so, R + 1) [ws.weight], bs (so), wv (1) [wv.weight], wsv (so) [wsv.weight],
 * bsv (1).  Forward: es (E, so), ev (E, 3) [= (E, 1, 3)].  Backward: the parameters' gradients
 * from grad_es (E, so), grad_ev (E, 3) (radial / unit get none: positions without
 * requires_grad), packed in grad_params as [ln_w R | ln_b R | wh 1 | Ws so (R + 1) | bs so |
 * wv 1 | wsv so | bsv 1] (2R + 3 + so (R + 3) floats); per-workgroup partial rows in the
 * workspace, added in a fixed order (deterministic).  R = 8 and 1 <= so <= 32 are compiled
 * (GMP_ERR_UNSUPPORTED otherwise: the caller runs the module chain). */
int gmp_gvp_edge_embed_fwd_f32(int64_t n_edges, int64_t radial_dim, int64_t so,
                               const float* radial, const float* unit, const float* ln_w,
                               const float* ln_b, const float* wh, const float* Ws,
                               const float* bs, const float* wv, const float* wsv,
                               const float* bsv, float eps, float* es, float* ev, void* stream);
size_t gmp_gvp_edge_embed_bwd_workspace_size(int64_t n_edges);
int gmp_gvp_edge_embed_bwd_f32(int64_t n_edges, int64_t radial_dim, int64_t so,
                               const float* radial, const float* unit, const float* ln_w,
                               const float* ln_b, const float* wh, const float* Ws,
                               const float* bs, const float* wv, const float* wsv,
                               const float* bsv, float eps, const float* grad_es,
                               const float* grad_ev, float* grad_params, void* workspace,
                               size_t workspace_bytes, void* stream);
/* gmp_gvp_ff_{fwd,bwd}_f32 (K17, r06): the node feed-forward of GVPConvLayer
 * (models/layers/gvp_layer.py:361-366, :433-434 -- ff_func = GVP((128, 16), (512, 32)) with
 * activations (relu, None) then GVP((512, 32), (128, 16)) with (None, None), vector_gate, h_dim 32;
 * GVP.forward gvp_layer.py:140-170) over N node rows in one kernel per direction.  s (N, 128),
 * v (N, 16, 3) row-major, all row tensors 16-byte aligned; weights in the reference's nn.Linear
 * layout: Wh1 (32, 16), Ws1 (512, 160) [columns s | |vh1|], b1 (512), Wv1 (32, 32), Wsv1
 * (32, 512), bsv1 (32), Wh2 (32, 32), Ws2 (128, 544) [columns s1 | |vh2|], b2 (128), Wv2 (16, 32),
 * Wsv2 (16, 128), bsv2 (16); Ws1, Wsv1, Ws2 16-byte aligned.
 * Forward: s2 (N, 128), v2 (N, 16, 3), gate1 (N, 32) [the first GVP's gate pre-activation] and
 * the right operands of the weight sums, zero-padded: B1 = [s | vn1 | 0] (N, 192),
 * B2 = [s1 | vn2 | 0] (N, 576) [s1 = relu(p1), vn = |vh| clamped], B3 = [v | 0] (N, 64),
 * B4 = [v1 | 0] (N, 128) [v1 the first GVP's vector output, (channel, xyz)].
 * Backward (from gate1, B2, s2 = the second GVP's pre-activation, grad_s2, grad_v2): ds (N, 128),
 * dv (N, 16, 3) and the left operands A1 = [dp1 | dgate1 | 0] (N, 576), A2 = [dp2 | dgate2 | 0]
 * (N, 192), A3 = [dvh1 | du1] (N, 192), A4 = [dvh2 | du2 | 0] (N, 192) [dp the gradient at a
 * scalar Linear's output, du = grad_v * sigmoid(gate) at W_v vh, dvh at vh; (channel, xyz)].
 * With C_k = A_k^T B_k (sums over the N rows) and x~ the xyz diagonal of a (3a, 3b) block:
 *   dWs1 = C1[:512, :160], db1 = colsum(dp1), dWsv1 = C1[512:544, :160] Ws1^T + dbsv1 b1^T;
 *   dWs2 = C2[:128, :544], db2 = colsum(dp2), dWsv2 = C2[128:144, :544] Ws2^T + dbsv2 b2^T;
 *   dWh1 = C3[:96, :48]~, dWv1 = C3[96:, :48]~ Wh1^T; dWh2 = C4[:96, :96]~,
 *   dWv2 = C4[96:144, :96]~ Wh2^T.  Exact f32 products. */
int gmp_gvp_ff_fwd_f32(int64_t n_nodes, const float* s_in, const float* v_in, const float* Wh1,
                       const float* Ws1, const float* b1, const float* Wv1, const float* Wsv1,
                       const float* bsv1, const float* Wh2, const float* Ws2, const float* b2,
                       const float* Wv2, const float* Wsv2, const float* bsv2, float* s_out,
                       float* v_out, float* gate1_out, float* B1, float* B2, float* B3, float* B4,
                       void* stream);
int gmp_gvp_ff_bwd_f32(int64_t n_nodes, const float* v_in, const float* gate1, const float* B2,
                       const float* s2, const float* ds_out, const float* dv_out,
                       const float* Wh1, const float* Ws1, const float* b1, const float* Wv1,
                       const float* Wsv1, const float* bsv1, const float* Wh2, const float* Ws2,
                       const float* b2, const float* Wv2, const float* Wsv2, const float* bsv2,
                       float* ds_in, float* dv_in, float* A1, float* A2, float* A3, float* A4,
                       void* stream);
int gmp_gvp_msg0_fwd_f32(int64_t n_edges, const int64_t* send, const int64_t* recv,
                         const float* P, const float* Q, const float* es, const float* ev,
                         const float* We, const float* Wn, const float* b, const float* Wv,
                         const float* Wsv, const float* bsv, const float* wev, float* s_out,
                         float* v_out, void* stream);
/* gmp_gvp_msg0_bwd_f32: spre (E, 128) and vh (E, 144), read only by the dWsv / dWv weight sums,
 * may be NULL (r05): the caller then forms those sums from the node projections,
 *   dWsv = (dgate^T [es | vn]) [We | Wn]^T + (S_j dgate)^T Pa + (S_i dgate)^T Pb + (1^T dgate) b,
 *   dWv[o, h] = sum_(n,x) (S_j dvpre)[n, o, x] Qa[n, h, x] + (S_i dvpre) .. Qb + wev[h] u[o]
 * (S_j, S_i the sender / receiver segment sums, u[o] = sum_(e,x) dvpre[e, o, x] ev[e, x]):
 * 2.2 KB per edge of HBM traffic less per layer. */
int gmp_gvp_msg0_bwd_f32(int64_t n_edges, const int64_t* send, const int64_t* recv,
                         const float* P, const float* Q, const float* es, const float* ev,
                         const float* We, const float* Wn, const float* b, const float* Wv,
                         const float* Wsv, const float* bsv, const float* wev,
                         const float* ds_out, const float* dv_out, float* dspre, float* spre,
                         float* dgate, float* vn, float* vh, float* dvpre, float* dvh,
                         float* des, float* dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * K9 radius graph.  Replaces torch_cluster.radius_graph(pos, r, batch,
 * loop=False, max_num_neighbors) as PyG SchNet's RadiusInteractionGraph builds it
 * (models/schnet.py:47; GPU-kernel selection rule): edge j -> i for j != i of the same graph with
 * ((dx*dx + dy*dy) + dz*dz) < r*r in fp32 (dx = p_i - p_j, no contraction); per target the first
 * max_num_neighbors + 1 candidates in ascending j (self included) are kept, then self is dropped
 * (max_num_neighbors <= 0: no cap).  batch may be NULL (one graph).  Cells have edge
 * 1/inv_cell >= r over the box [lo, lo + dims/inv_cell), keyed (graph, cell):
 *   cells: cell id per node -> the caller buckets nodes with gmp_csr_build over
 *          num_graphs*dims[0]*dims[1]*dims[2] segments (cell_rowptr, cell_perm);
 *   count: number of sources per target;  fill: the sources of target i at
 *          offsets[i]..offsets[i+1], ascending -> edge_index sorted by (target, source).
 * ------------------------------------------------------------------------------------------ */
int gmp_radius_cells_f32(const float* pos, const int64_t* batch, int64_t n_nodes,
                         const float* lo3, float inv_cell, const int* dims3, int64_t* cell_out,
                         void* stream);
int gmp_radius_count_f32(const float* pos, const int64_t* batch, int64_t n_nodes, float r,
                         int64_t max_num_neighbors, const float* lo3, float inv_cell,
                         const int* dims3, const int64_t* cell, const int64_t* cell_rowptr,
                         const int64_t* cell_perm, int64_t* counts, void* stream);
int gmp_radius_fill_f32(const float* pos, const int64_t* batch, int64_t n_nodes, float r,
                        int64_t max_num_neighbors, const float* lo3, float inv_cell,
                        const int* dims3, const int64_t* cell, const int64_t* cell_rowptr,
                        const int64_t* cell_perm, const int64_t* offsets, int64_t* src_out,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * K9p radius graph under periodic boundary conditions.  THE CONTRACT (stated here only):
 *   pos (N,3) f32; cell (B,3,3) f32, rows = lattice vectors, one cell per graph; pbc: three
 *   booleans shared by all graphs; batch (N) or NULL (one graph); r > 0.
 * An edge (j -> i, S) exists for every S in Z^3 with S_k = 0 on each non-periodic axis, i and j
 * in the same graph b, (j, S) != (i, 0) and d2 < r2, where, in fp32 with every operation
 * rounded to nearest and nothing contracted (K9's rule),
 *   t  = ((S0*c[b,0,:] + S1*c[b,1,:]) + S2*c[b,2,:])
 *   dx = (p_i - p_j) - t                       (per component)
 *   d2 = (dx*dx + dy*dy) + dz*dz,   r2 = r*r.
 * Self-image edges (i == j, S != 0) and edges between coincident distinct atoms are edges.  The
 * result is defined on pos as given: atoms need not lie inside the cell.  There is no neighbour
 * cap.  Output: edge_index (2,E) int64 [sources; targets] and edge_shift_idx (E,3) int32, both
 * sorted by (i, j, S0, S1, S2); |S_k| <= 127.  The featurised vector of an edge is
 * (pos[src] - pos[dst]) + t, the exact negative of dx.
 *
 * Per-graph plan (DEVICE arrays, computed by the caller in fp64 from one copy of cell; the
 * margin argument is in gmp_radius_pbc.hip):
 *   graph_i (B,8) int32: nb[3] bins per axis, m[3] reach in bins, periodic-axis bit mask, 0;
 *   graph_f (B,24) f32: inv[9] (frac_k = sum_d p_d inv[3d+k]), org[3] and scale[3] (bin
 *     coordinate of a non-periodic axis = (frac - org) * scale; periodic: (frac - floor(frac))
 *     * scale with scale = nb), cell[9];
 *   graph_base (B) int64: first bin of each graph in the bin table.
 * bins:  bin id and packed wraps floor(frac) per node -> the caller buckets nodes with
 *        gmp_csr_build over the bin table (bin_rowptr, bin_perm);
 * count: edges per target;  fill: sources and shift indices of target i at offsets[i] ..
 *        offsets[i+1], sorted (targets with more than gmp_radius_pbc_sort_capacity() edges are
 *        sorted in global memory instead of LDS).
 * *err_flag (DEVICE, zeroed by the caller) is set to 1 for a batch entry outside [0, B), a
 * wrap or shift beyond 127, or counts that do not match the fill.
 * gmp_edge_shift_vectors_f32: t (E,3) of the contract from edge_shift_idx, cell and each edge's
 * graph (NULL: graph 0); an edge whose graph is outside [0, B) gets zeros.
 * ------------------------------------------------------------------------------------------ */
int gmp_radius_pbc_sort_capacity(void);
int gmp_radius_pbc_bins_f32(const float* pos, const int64_t* batch, int64_t n_nodes,
                            int64_t n_graphs, const int* graph_i, const float* graph_f,
                            const int64_t* graph_base, int64_t* bin_out, int* wrap_out,
                            int32_t* err_flag, void* stream);
int gmp_radius_pbc_count_f32(const float* pos, const int64_t* batch, int64_t n_nodes,
                             int64_t n_graphs, float r, const int* graph_i, const float* graph_f,
                             const int64_t* graph_base, const int64_t* bin, const int* wrap,
                             const int64_t* bin_rowptr, const int64_t* bin_perm, int64_t* counts,
                             int32_t* err_flag, void* stream);
int gmp_radius_pbc_fill_f32(const float* pos, const int64_t* batch, int64_t n_nodes,
                            int64_t n_graphs, float r, const int* graph_i, const float* graph_f,
                            const int64_t* graph_base, const int64_t* bin, const int* wrap,
                            const int64_t* bin_rowptr, const int64_t* bin_perm,
                            const int64_t* offsets, int64_t* src_out, int* shift_idx_out,
                            int32_t* err_flag, void* stream);
int gmp_edge_shift_vectors_f32(const int* edge_shift_idx, const float* cell,
                               const int64_t* edge_graph, int64_t n_edges, int64_t n_graphs,
                               float* shift_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * K10 batch collation (PyG Batch.from_data_list as the reference's loaders
 * build it, experiments/utils/train_utils.py:28,132).  edge_index_local: (2, E) graph-local
 * indices of B graphs packed back to back; node_ptr / edge_ptr: (B+1) prefix sums of the
 * per-graph node / edge counts.  Writes edge_index_out = local + node_ptr[graph of edge] and
 * batch_out[a] = graph of node a.  A local index outside [0, n_g) sets *err to 1 (err may be
 * NULL).  Empty graphs are allowed.
 * ------------------------------------------------------------------------------------------ */
int gmp_batch_collate(const int64_t* edge_index_local, int64_t n_edges, const int64_t* node_ptr,
                      const int64_t* edge_ptr, int64_t n_graphs, int64_t n_nodes,
                      int64_t* edge_index_out, int64_t* batch_out, int* err, void* stream);

/* ------------------------------------------------------------------------------------------
 * K11 triplets + angles / torsions.  Replaces `xyz_to_dat`
 * (models/layers/spherenet_layer.py:496-564) and the triplet/angle block of the DimeNet forward
 * (models/dimenet.py:79-90, PyG DimeNet.triplets).  edge_index (2, E): e = (j -> i).
 * Adjacency by target, entries sorted by (target, source): adj_rowptr (N+1), adj_src (source
 * of each entry), adj_eid (edge id of each entry).
 *   count: counts[e] = in-degree(j) - #{in-edges of j with source i}; dist[e] = |p_i - p_j|
 *          (dist may be NULL);
 *   fill:  for t in [offsets[e], offsets[e+1]): idx_kj[t] = edge (k -> j) for the k != i in
 *          ascending order, idx_ji[t] = e; angle[t] (mode 0: SphereNet, vertex j; mode 1:
 *          DimeNet, vertex i; may be NULL); torsion[t] (mode 0 only, may be NULL).
 * Arithmetic reproduces the reference's torch CPU evaluation op by op (see gmp_triplet.hip).
 * ------------------------------------------------------------------------------------------ */
int gmp_triplet_count(const float* pos, const int64_t* edge_index, int64_t n_edges,
                      int64_t n_nodes, const int64_t* adj_rowptr, const int64_t* adj_src,
                      int64_t* counts, float* dist, void* stream);
int gmp_triplet_fill_f32(const float* pos, const int64_t* edge_index, int64_t n_edges,
                         int64_t n_nodes, const int64_t* adj_rowptr, const int64_t* adj_src,
                         const int64_t* adj_eid, const int64_t* offsets, int64_t n_triplets,
                         int mode, int64_t* idx_kj, int64_t* idx_ji, float* angle,
                         float* torsion, int64_t* torsion_kn, void* stream);
/* Backward of dist (E) and angle (T) w.r.t. pos (DimeNet / SphereNet under autograd): writes
 * 3T + 2E rows of 3 floats (`rows`) and their node ids (`node`): vertex, u-end and v-end rows
 * of every triplet, then +/- rows of every edge's distance; d pos = the segmented sum of rows
 * by node (the caller's CSR; deterministic).  grad_dist / grad_angle may be NULL (zero). */
int gmp_triplet_geom_bwd_f32(const float* pos, const int64_t* edge_index, int64_t n_edges,
                             const int64_t* idx_kj, const int64_t* idx_ji, int64_t n_triplets,
                             int mode, const float* grad_dist, const float* grad_angle,
                             float* rows, int64_t* node, void* stream);
/* Second backward of dist and angle (models/dimenet.py:82-89 differentiated twice: a loss on the
 * forces -dE/dpos), modes 0 and 1, no torsion.  a_pos (N, 3) is the cotangent of the first
 * backward's d pos.  Writes gg_dist (E) = (a_i - a_j).(p_i - p_j) / d and gg_angle (T) =
 * a_u.dtheta/du + a_v.dtheta/dv (the gradients w.r.t. grad_dist / grad_angle; either may be
 * NULL), and 3T + 2E rows with node ids in the layout of gmp_triplet_geom_bwd_f32: the
 * directional derivative along a of the rows that entry writes; their segmented sum by node is
 * the gradient w.r.t. pos.  grad_dist / grad_angle may be NULL (zero rows).  A collinear
 * triplet, a zero-length edge and a zero cotangent follow the first backward. */
int gmp_triplet_geom_bwd2_f32(const float* pos, const int64_t* edge_index, int64_t n_edges,
                              const int64_t* idx_kj, const int64_t* idx_ji, int64_t n_triplets,
                              int mode, const float* grad_dist, const float* grad_angle,
                              const float* a_pos, float* gg_dist, float* gg_angle, float* rows,
                              int64_t* node, void* stream);
/* Backward of the SphereNet torsion (spherenet_layer.py:535-559 under autograd) w.r.t. pos:
 * torsion_kn (T, from gmp_triplet_fill_f32; -1 = no candidate) is the scatter-min's winning
 * k_n, which alone receives the gradient (torch_scatter's arg routing).  Writes 4T rows of 3
 * floats and their node ids (i, j, k, k_n blocks of T); d pos = their segmented sum by node.
 * Zero rows without a candidate, for a zero cotangent, for an edge of zero length and where
 * a^2 + b^2 == 0 (triplet or winner exactly collinear with the edge), where autograd gives NaN. */
int gmp_triplet_torsion_bwd_f32(const float* pos, const int64_t* edge_index, int64_t n_edges,
                                const int64_t* idx_kj, const int64_t* idx_ji,
                                const int64_t* torsion_kn, int64_t n_triplets,
                                const float* grad_torsion, float* rows, int64_t* node,
                                void* stream);

/* ------------------------------------------------------------------------------------------
 * K11p: DimeNet's triplets and angles on a periodic graph (gmp_triplet_pbc.hip).  The contract:
 * an edge is e = (j -> i, S_e): source edge_index[0][e], target edge_index[1][e], image
 * shift_idx[e] (an int32 triple).  Its vector is the K9p contract's featurised vector
 *   vec_e = (pos[j] - pos[i]) + t_e,  t_e from gmp_edge_shift_vectors_f32
 * (a subtraction, then an addition, each rounded in fp32); the caller forms vec (E, 3).
 *   triplets of e: all entries kj = (k -> j, S_kj) of j's in-adjacency except those with k == i
 *          AND S_kj == -S_e: the reverse image of e, an exact integer compare.  A self-image
 *          edge (i == j, S != 0) follows the same rule; k == i with S_kj != -S_e is another
 *          image of i and is kept; every entry that matches (a duplicated (j, i, S)) is excluded.
 *   order: edges in edge order (idx_ji non-decreasing); within an edge the order of the
 *          adjacency (ascending k, then ascending edge id; for a K9p graph ascending S).
 *   dist[e] = dist_len3(vec_e) = sqrt(fma(y, y, x x) + z z): K11's dist, bit-equal to it with
 *          all shifts zero.
 *   angle[t] = atan2f(norm3(cross3(u, v)), dot3_sum(u, v)), u = vec_ji, v = u + vec_kj (one
 *          rounded add per component; v is the image of k relative to i).  The helpers are those
 *          of K11 (gmp_triplet_geom.h), each rounding explicit: dot3_sum rounds every product,
 *          then ((+0 + xx) + yy) + zz; cross3 and norm3 are fma chains.
 *          With zero shifts the triplet lists equal K11's (mode 1) and the angle differs from
 *          its p_k - p_i form only by rounding.
 * Mode 1 (DimeNet, vertex i) only; no torsion.  adj_* as for K11.
 *   count: counts[e] = in-degree(j) - #excluded entries; dist (may be NULL; needs vec).
 *   fill:  idx_kj / idx_ji (T) and angle (T; may be NULL; needs vec) for the offsets (E + 1)
 *          that are the exclusive prefix sums of counts.
 * SphereNet (mode 0: angle at vertex j, and the torsion) on the same lists: idx_kj, idx_ji, dist
 * and the offsets are those of count / fill (angle = NULL), unchanged; gmp_triplet_dat_pbc_f32
 * adds, for triplet t of edge e, by the same device functions as K11's mode 0:
 *   vectors: u = sub3(0, vec_e) (a subtraction from +0, not a sign flip: an equal coordinate
 *          gives +0, as K11's p_i - p_j does), v = vec[idx_kj[t]].
 *   angle[t] = atan2f(norm3(cross3(u, v)), dot3_sum(u, v)), at vertex j, in [0, pi].
 *   candidates of t: all triplets t' of the same edge, [offsets[e], offsets[e+1]), in index
 *          order, t' = t included (the same kept adjacency entries; in the open case the
 *          reference's "k_n != i", which keeps k_n = k); w = vec[idx_kj[t']].
 *   t1(t, t') = torsion_candidate: plane1 = cross3(u, v), plane2 = cross3(u, w),
 *          a = dot3_sum(plane1, plane2), b = dot3_sum(cross3(plane1, plane2), u) / torsion_len3(u)
 *          (a rounded division; torsion_len3(u) = sqrt(fma(x, x, y y) + z z)),
 *          t1 = atan2f(b, a), and t1 + 2 pi (a rounded addition) if t1 <= 0.
 *   torsion[t] = the minimum of t1 over the candidates by K11's rule: identity FLT_MAX, NaN
 *          never wins, 0 if nothing won.  torsion_arg[t] = the TRIPLET index t' of the first
 *          candidate among equal minima, -1 if none: the winning edge is
 *          idx_kj[torsion_arg[t]], and a duplicated (j, i, S) resolves to the lower index.
 * With all shifts zero this is K11's mode 0 bit for bit: both kernels call the same helpers,
 * whose roundings are stated under fp contract(off) and do not depend on the compiler.
 * ------------------------------------------------------------------------------------------ */
int gmp_triplet_count_pbc(const float* vec, const int64_t* edge_index, int64_t n_edges,
                          int64_t n_nodes, const int64_t* adj_rowptr, const int64_t* adj_src,
                          const int64_t* adj_eid, const int32_t* shift_idx, int64_t* counts,
                          float* dist, void* stream);
int gmp_triplet_fill_pbc_f32(const float* vec, const int64_t* edge_index, int64_t n_edges,
                             int64_t n_nodes, const int64_t* adj_rowptr, const int64_t* adj_src,
                             const int64_t* adj_eid, const int32_t* shift_idx,
                             const int64_t* offsets, int64_t n_triplets, int64_t* idx_kj,
                             int64_t* idx_ji, float* angle, void* stream);
/* Backward of dist (E) and angle (T) of K11p w.r.t. vec (E, 3), in edge-vector form (no node
 * ids, no sort).  Writes rows (2T + E, 3): [0, T) g_u + g_v, the share of edge idx_ji[t];
 * [T, 2T) g_v, the share of edge idx_kj[t]; [2T, 2T + E) grad_dist vec / d.  d vec = rows[2T:]
 * + the sum of rows[:T] over the triplet offsets + the sum of rows[T:2T] over a CSR of idx_kj
 * (deterministic, no atomics).  grad_dist / grad_angle may be NULL (zero). */
int gmp_triplet_vec_bwd_f32(const float* vec, int64_t n_edges, const int64_t* idx_kj,
                            const int64_t* idx_ji, int64_t n_triplets, const float* grad_dist,
                            const float* grad_angle, float* rows, void* stream);
/* Second backward of the same: a_vec (E, 3) is the cotangent of d vec, a_u = a_vec[ji] and
 * a_v = a_vec[ji] + a_vec[kj].  Writes gg_dist (E) = a_vec . vec / d and gg_angle (T) =
 * a_u.dtheta/du + a_v.dtheta/dv (either may be NULL) and rows (2T + E, 3) in the layout above:
 * the directional derivative along a_vec of the rows gmp_triplet_vec_bwd_f32 writes.  u, v,
 * a_u, a_v are formed in fp32, the rest in double, rounded once.  A collinear triplet (b = 0
 * drops the c^ terms), a zero-length edge and a zero cotangent follow the first backward. */
int gmp_triplet_vec_bwd2_f32(const float* vec, int64_t n_edges, const int64_t* idx_kj,
                             const int64_t* idx_ji, int64_t n_triplets, const float* grad_dist,
                             const float* grad_angle, const float* a_vec, float* gg_dist,
                             float* gg_angle, float* rows, void* stream);
/* SphereNet's angle (T) and torsion (T) with its winner torsion_arg (T) on the K11p lists (the
 * contract above).  torsion and torsion_arg may be NULL together: angle only (offsets may then
 * be NULL).  GMP_OK without a launch for n_triplets == 0. */
int gmp_triplet_dat_pbc_f32(const float* vec, int64_t n_edges, const int64_t* idx_kj,
                            const int64_t* idx_ji, const int64_t* offsets, int64_t n_triplets,
                            float* angle, float* torsion, int64_t* torsion_arg, void* stream);
/* First backward of dist (E), the mode-0 angle (T) and the torsion (T) w.r.t. vec (E, 3), in
 * edge-vector form.  Writes rows (2T + E, 3) in the layout of gmp_triplet_vec_bwd_f32, summed the
 * same way: [0, T) -g_u of angle and torsion, the share of edge idx_ji[t]; [T, 2T) the share of
 * edge idx_kj[t]: g_v of the triplet's angle and torsion plus g_w of every triplet of the same
 * edge whose winner torsion_arg is t (gathered in index order inside the kernel: no sort, no
 * atomics, a fixed order); [2T, 2T + E) grad_dist vec / d (written for n_triplets == 0 too).
 * The winner is held fixed (torch_scatter's arg routing); the 2 pi shift has unit derivative.
 * Zero rows for a zero cotangent and, for the torsion, where a^2 + b^2 == 0 or |u| == 0 (an
 * exactly collinear triplet, a candidate exactly parallel to u), where autograd gives NaN (one
 * torsion_bwd serves this kernel and K11's gmp_triplet_torsion_bwd_f32, same dead cases); the
 * angle's dead cases are those of gmp_triplet_vec_bwd_f32.  Any of the three cotangents may be
 * NULL (zero); offsets and torsion_arg are needed with grad_torsion only. */
int gmp_triplet_dat_vec_bwd_f32(const float* vec, int64_t n_edges, const int64_t* idx_kj,
                                const int64_t* idx_ji, const int64_t* offsets,
                                const int64_t* torsion_arg, int64_t n_triplets,
                                const float* grad_dist, const float* grad_angle,
                                const float* grad_torsion, float* rows, void* stream);

/* ------------------------------------------------------------------------------------------
 * K12 fused LayerNorm + activation over rows (node-level MLPs: EGNN mlp_upd,
 * egnn_layer.py:37-39 / :82-86; GVP scalar LayerNorm, gvp_layer.py:221-243 with act = 2).
 * x (rows, d), d <= 512; act 0 relu, 1 silu, 2 identity.  Forward writes y = act(LN(x)) and
 * saves xhat (rows, d) and rstd (rows) for the backward.  Backward: grad_x (rows, d) and
 * grad_gamma_beta (2d) = [dgamma | dbeta] (deterministic; workspace from
 * gmp_ln_act_bwd_workspace_size).  grad_gamma_beta may be NULL: the workspace then holds
 * gmp_ln_act_bwd_partial_rows(rows) partial rows of width 2d, to be reduced by the caller
 * (gmp_sum_rows_f32, e.g. later / on another stream: gamma and beta are leaves of the graph).
 * gmp_sum_rows_f32: out[c] = sum_r partials[r, c] in a fixed order (deterministic).
 * ------------------------------------------------------------------------------------------ */
int gmp_ln_act_fwd_f32(int64_t rows, int64_t d, const float* x, const float* gamma,
                       const float* beta, float eps, int act, float* y, float* xhat_save,
                       float* rstd_save, void* stream);
size_t gmp_ln_act_bwd_workspace_size(int64_t rows, int64_t d);
int gmp_ln_act_bwd_f32(int64_t rows, int64_t d, const float* grad_y, const float* xhat,
                       const float* rstd, const float* gamma, const float* beta, int act,
                       float* grad_x, float* grad_gamma_beta, void* workspace,
                       size_t workspace_bytes, void* stream);
int64_t gmp_ln_act_bwd_partial_rows(int64_t rows);
int gmp_sum_rows_f32(const float* partials, int64_t nrows, int64_t width, float* out,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * GVP vector LayerNorm (gvp_layer.py:232-243: v / sqrt(mean_c clamp(|v_c|^2, 1e-8)), the norm
 * of _norm_no_nan, :66-73).  v (rows, channels, 3) contiguous, 1 <= channels <= 64.  Forward
 * writes out = v / vn; backward recomputes vn from v and writes grad_v from grad_out (the clamp
 * passes the gradient where |v_c|^2 >= 1e-8, as torch's clamp_min).  No workspace.
 * ------------------------------------------------------------------------------------------ */
int gmp_vec_norm_fwd_f32(int64_t rows, int64_t channels, const float* v, float* out,
                         void* stream);
int gmp_vec_norm_bwd_f32(int64_t rows, int64_t channels, const float* v, const float* grad_out,
                         float* grad_v, void* stream);
/* _norm_no_nan over the xyz axis of vh (rows, 3, h) contiguous (GVP.forward's |vh|,
 * gvp_layer.py:66-73, :101-170): out (rows, h) = sqrt(max(sum_x vh^2, 1e-8)); backward
 * grad_vh (rows, 3, h) from grad_out (rows, h). */
int gmp_xyz_norm_fwd_f32(int64_t rows, int64_t h, const float* vh, float* out, void* stream);
int gmp_xyz_norm_bwd_f32(int64_t rows, int64_t h, const float* vh, const float* grad_out,
                         float* grad_vh, void* stream);

/* ------------------------------------------------------------------------------------------
 * K8 MACE symmetric contraction (models/mace_modules/symmetric_contraction.py:20-188 with
 * element_dependent=False; SymmetricContraction.forward :81-85 concatenates the per-output-irrep
 * Contraction.forward :150-185), all output irreps of C channels at once, any irreps: x (N, C, D)
 * = reshape_irreps of C x (irreps) (irreps_tools.py:63-79; D <= 63 components per channel, any
 * parities, repeated l), correlation 1..4 folded into one polynomial over symmetric monomials
 * and evaluated over the sparse TERM LIST of the module's coupling pattern:
 *   out[b, out_base[m] + out_stride[m] c] = sum_{t in row m} coef[t, c] prod_{r < 4} xx[f_r(t)]
 * with xx = [x[b, c, 0..D-1], 1.0] (factor index D = the constant 1: degree < 4 monomials).
 * plan (int32): [row_ptr (rows + 1) | out_base (rows) | out_stride (rows) | terms (n_terms)],
 *   term word f0 | f1 << 6 | f2 << 12 | f3 << 18 | m << 24 (m < rows <= 255), terms of row m at
 *   row_ptr[m] .. row_ptr[m+1] - 1 (summed in that order);
 * coef (n_terms, C), term-major: coef[t, c] = A~_nu[c, m_t, q_t], the folded coefficient
 *   A~_nu[c, m, q] = sum over the distinct permutations p of monomial q of
 *   sum_k U_nu[m, p, k] W_nu[k, c] (the host builds the plan once and coef per call,
 *   differentiably).  out (N, rows C).
 * Backward: dx (N, C, D) (may be NULL) and dcoef partials (gmp_sc_groups(N), n_terms, C) (may
 * be NULL; the caller sums the groups in order; N = 0 writes one all-zero group).
 * Deterministic.  (ABI 5: the plan form replaces
 * the dense per-degree A_nu arguments and gmp_sc_monomials.)
 * ------------------------------------------------------------------------------------------ */
int gmp_sc_groups(int64_t n_nodes);
/* The launch decomposition the two entry points below use for these sizes (host arithmetic, and
 * the very values the launches take; node blocks depend on the current device's CU count).
 * out[0..5], forward and dx kernels: channels per tile CT = min(C, 16), nodes per pass 256 / CT,
 * channel tiles, node blocks (grid-stride over nodes), dynamic LDS bytes of the forward, of dx.
 * out[6..11], dcoef kernel: channels per tile CT_d = clamp(4096 / n_terms, 1, min(16, C)), terms
 * per workgroup 4096 / CT_d, term blocks (0 at n_terms = 0: no launch), nodes staged per round,
 * node groups (= gmp_sc_groups), nodes per group.  GMP_ERR_ARG for sizes the entry points
 * refuse. */
int gmp_sc_route(int64_t n_nodes, int channels, int dim, int rows, int n_terms,
                 int64_t out[12]);
int gmp_symmetric_contraction_fwd_f32(int64_t n_nodes, int channels, int dim, int rows,
                                      int n_terms, const int32_t* plan, const float* coef,
                                      const float* x, float* out, void* stream);
int gmp_symmetric_contraction_bwd_f32(int64_t n_nodes, int channels, int dim, int rows,
                                      int n_terms, const int32_t* plan, const float* coef,
                                      const float* x, const float* gout, float* dx,
                                      float* dcoef_partials, void* stream);

/* ------------------------------------------------------------------------------------------
 * K13 SchNet CFConv fused message + aggregation (PyG 2.3.1 CFConv.message `x_j * W` and
 * aggr "add", called at schnet.py:72; replaces the x_j gather, the (E, F) product and the
 * scatter-sum of a15):
 *   out[s, :] = sum_{k in [rowptr[s], rowptr[s+1])} x[xidx[perm[k]], :] * w[perm[k], :]
 * Forward: CSR over dst, xidx = src.  x-gradient: CSR over src, x = grad_out, xidx = dst.
 * F % 4 == 0, x / w / out 16-byte aligned.  Out-of-range xidx -> zero term, *err = 1.
 * gmp_cfconv_wgrad_f32: dw[e, :] = g[gidx[e], :] * x[xidx[e], :] (W-gradient, gidx = dst,
 * xidx = src); out-of-range -> zero row, *err = 1.  Deterministic (no atomics).
 * ------------------------------------------------------------------------------------------ */
int gmp_cfconv_aggregate_f32(const float* x, int64_t n_x, const int64_t* xidx, const float* w,
                             int64_t n_items, int64_t F, const int64_t* perm,
                             const int64_t* rowptr, int64_t n_seg, float* out, int32_t* err,
                             void* stream);
int gmp_cfconv_wgrad_f32(const float* g, int64_t n_g, const int64_t* gidx, const float* x,
                         int64_t n_x, const int64_t* xidx, int64_t n_items, int64_t F, float* dw,
                         int32_t* err, void* stream);
/* Scaled forms (SchNet W = filter(edge_attr) * C with the per-edge cosine cutoff C, never
 * materialised): the aggregate uses W[e] * escale[e] (rounded per element as the reference's
 * product); the W-gradient is written as (g[gidx[e]] * x[xidx[e]]) * escale[e], the gradient
 * w.r.t. filter(edge_attr).  escale may be NULL (= the unscaled entry points). */
int gmp_cfconv_aggregate_scaled_f32(const float* x, int64_t n_x, const int64_t* xidx,
                                    const float* w, const float* escale, int64_t n_items,
                                    int64_t F, const int64_t* perm, const int64_t* rowptr,
                                    int64_t n_seg, float* out, int32_t* err, void* stream);
int gmp_cfconv_wgrad_scaled_f32(const float* g, int64_t n_g, const int64_t* gidx, const float* x,
                                int64_t n_x, const int64_t* xidx, const float* escale,
                                int64_t n_items, int64_t F, float* dw, int32_t* err,
                                void* stream);
/* The gradient w.r.t. the per-edge factor (and the fourth partial derivative of the multilinear
 * form sum_e C[e] sum_f g[dst_e, f] x[src_e, f] W[e, f], from which every second-order term of
 * CFConv follows by substitution):
 *   dc[e] = (sum_f g[gidx[e], f] * x[xidx[e], f] * w[e, f]) (* escale[e])
 * F % 4 == 0, g / x / w 16-byte aligned, escale may be NULL.  A fixed lane group per edge
 * reduces in a fixed order (deterministic, no atomics); out-of-range -> dc[e] = 0, *err = 1. */
int gmp_cfconv_cgrad_f32(const float* g, int64_t n_g, const int64_t* gidx, const float* x,
                         int64_t n_x, const int64_t* xidx, const float* w, const float* escale,
                         int64_t n_items, int64_t F, float* dc, int32_t* err, void* stream);

/* ------------------------------------------------------------------------------------------
 * K14 shifted softplus (PyG ShiftedSoftplus, the SchNet filter-network / interaction
 * activation, schnet.py:72): torch softplus semantics (beta 1, threshold 20) minus `shift`.
 *   fwd: y = (x > 20 ? x : log1p(exp(x))) - shift
 *   bwd: grad_x = x > 20 ? grad_y : grad_y * z / (z + 1), z = exp(x)
 * n % 4 == 0, 16-byte aligned pointers.
 * ------------------------------------------------------------------------------------------ */
int gmp_ssp_fwd_f32(const float* x, int64_t n, float shift, float* y, void* stream);
int gmp_ssp_bwd_f32(const float* x, const float* grad_y, int64_t n, float* grad_x,
                    void* stream);
/* Second order: with a the cotangent of grad_x = grad_y sigmoid(x),
 *   gg = a sigmoid(x) (cotangent of grad_y), gx = a grad_y sigmoid(x) (1 - sigmoid(x))
 * (cotangent of x), in one pass; finite for every finite x (the product underflows to 0). */
int gmp_ssp_bwd2_f32(const float* x, const float* grad_y, const float* a, int64_t n, float* gg,
                     float* gx, void* stream);

/* ------------------------------------------------------------------------------------------
 * K18 SphereNet spherical basis (models/layers/spherenet_layer.py dist_emb / angle_emb /
 * torsion_emb).  Additions only: the ABI version is unchanged.  n = num_spherical (<= 16),
 * k = num_radial (<= 64).  Host tables: zeros (n k) the fp32 zeros z_lq of j_l, norm (n k)
 * the normalisers N_lq, pref (n^2) the harmonic prefactors by flat index l^2 + p, p = 0 (m = 0),
 * 1..l (cos, m = p), l+1..2l (sin, m = 2l + 1 - p), sqrt(2) of m != 0 included.
 *
 * Edge basis, x = dist / cutoff (dist > 0):
 *   rbf (E, k)  = envelope(x) sin(freq_q x), envelope(x) = 1/x + a x^(p-1) + b x^p + c x^(p+1),
 *                 p = envelope_exponent + 1, a = -(p+1)(p+2)/2, b = p(p+2), c = -p(p+1)/2;
 *   jb (E, n k) = N_lq j_l(z_lq x), accurate for every x in (0, z_max]: a power series below
 *                 x = l + 1, the upward recurrence above (never the closed form over x^l).
 *   bwd: grad_dist (E) from grad_rbf / grad_jb (either may be NULL) and grad_freq (k), the
 *        latter through freq_partials (gmp_sph_edge_basis_bwd_partial_rows(E), k) in a fixed
 *        order (no atomics).
 *
 * Triplet projection for L layers at once: the angle features jb[idx_kj[t]][l, q] Y_l0(angle_t)
 * (n k of them, index l k + q) and the torsion features jb[idx_kj[t]][b, q] Yflat[a n + b]
 * (angle_t, torsion_t) (n^2 k, index (a n + b) k + q) never leave the chip:
 *   S (L, T, ba) = W_sbf1[l] angle_emb_t,   P (L, T, bt) = W_t1[l] torsion_emb_t.
 * The weights come feature-major: w_sbf1_t (n k, lda), w_t1_t (n^2 k, ldt), column o =
 * layer * b + j, lda / ldt = L ba / L bt rounded up to a multiple of 8, padding zero.
 *   bwd: grad_w (n k lda + n^2 k ldt) = [grad w_sbf1_t | grad w_t1_t] recomputing the features,
 *        through partials (gmp_sph_triplet_proj_bwd_partial_rows(T) rows of that width), summed
 *        in a fixed order.  If grad_jb_rows (T, n k), grad_angle (T), grad_torsion (T) are
 *        given (all or none) the geometry gradients are written too; the caller sums
 *        grad_jb_rows per edge over the CSR of idx_kj.
 *   emb: the materialised angle_emb (T, n k) and torsion_emb (T, n^2 k) (tests, small T).
 * An idx_kj outside [0, E) contributes a zero jb row.
 * ------------------------------------------------------------------------------------------ */
int gmp_sph_edge_basis_fwd_f32(const float* dist, int64_t n_edges, float cutoff,
                               int envelope_exponent, const float* freq, int num_radial,
                               const float* zeros, const float* norm, int num_spherical,
                               float* rbf, float* jb, void* stream);
int64_t gmp_sph_edge_basis_bwd_partial_rows(int64_t n_edges);
int gmp_sph_edge_basis_bwd_f32(const float* dist, int64_t n_edges, float cutoff,
                               int envelope_exponent, const float* freq, int num_radial,
                               const float* zeros, const float* norm, int num_spherical,
                               const float* grad_rbf, const float* grad_jb, float* grad_dist,
                               float* grad_freq, float* freq_partials, void* stream);
int gmp_sph_triplet_proj_fwd_f32(int64_t n_triplets, int64_t n_edges, int num_spherical,
                                 int num_radial, const float* jb, const float* angle,
                                 const float* torsion, const int64_t* idx_kj, const float* pref,
                                 const float* w_sbf1_t, int n_layers, int ba, const float* w_t1_t,
                                 int bt, float* S, float* P, void* stream);
int gmp_sph_triplet_emb_f32(int64_t n_triplets, int64_t n_edges, int num_spherical,
                            int num_radial, const float* jb, const float* angle,
                            const float* torsion, const int64_t* idx_kj, const float* pref,
                            float* angle_emb, float* torsion_emb, void* stream);
int64_t gmp_sph_triplet_proj_bwd_partial_rows(int64_t n_triplets);
int gmp_sph_triplet_proj_bwd_f32(int64_t n_triplets, int64_t n_edges, int num_spherical,
                                 int num_radial, const float* jb, const float* angle,
                                 const float* torsion, const int64_t* idx_kj, const float* pref,
                                 const float* w_sbf1_t, int n_layers, int ba, const float* w_t1_t,
                                 int bt, const float* grad_S, const float* grad_P,
                                 float* grad_w, float* partials, float* grad_jb_rows,
                                 float* grad_angle, float* grad_torsion, void* stream);

/* ------------------------------------------------------------------------------------------
 * K19 SphereNet triplet interaction of one layer (spherenet_layer.py update_e.forward):
 *   out[s, c] = sum_{p in [rowptr[s], rowptr[s+1])} src[gather_idx[t], c]
 *               (W_sbf2 S_t)[c] (W_t2 P_t)[c],   t = perm ? perm[p] : p
 * src (n_src, I), S (T, ba), P (T, bt), w_sbf2 (I, ba), w_t2 (I, bt), out (n_seg, I).  With
 * rowptr = K11's triplet offsets, perm = NULL and gather_idx = idx_kj this is the message m;
 * with the CSR of idx_kj and gather_idx = idx_ji, src = grad_m, it is grad_xd.  One wave per
 * segment adds the triplets in order: no atomics, bit-identical between runs.  Empty segments
 * give zero rows; an index out of range contributes nothing.
 *   bwd (ba, bt <= 16): grad_S (T, ba), grad_P (T, bt) and grad_w (I ba + I bt) = [grad w_sbf2 |
 *   grad w_t2] through partials (gmp_triplet_interact_bwd_partial_rows(E) rows of that width),
 *   summed in a fixed order.
 * ------------------------------------------------------------------------------------------ */
int gmp_triplet_interact_fwd_f32(int64_t n_seg, int64_t n_src, int64_t n_triplets, int64_t I,
                                 int ba, int bt, const float* src, const float* S, const float* P,
                                 const float* w_sbf2, const float* w_t2, const int64_t* gather_idx,
                                 const int64_t* perm, const int64_t* rowptr, float* out,
                                 void* stream);
int64_t gmp_triplet_interact_bwd_partial_rows(int64_t n_edges);
int gmp_triplet_interact_bwd_f32(int64_t n_edges, int64_t n_triplets, int64_t I, int ba, int bt,
                                 const float* grad_m, const float* xd, const float* S,
                                 const float* P, const float* w_sbf2, const float* w_t2,
                                 const int64_t* idx_kj, const int64_t* offsets, float* grad_S,
                                 float* grad_P, float* grad_w, float* partials, void* stream);

/* ------------------------------------------------------------------------------------------
 * K18d DimeNet++ basis (PyG DimeNetPlusPlus: BesselBasisLayer, SphericalBasisLayer), the
 * angle-only form of K18.  Additions only: the ABI version is unchanged.  Tables as K18.
 *
 * Edge basis, x = dist / cutoff, env(x) = envelope(x) [x < 1] (K18's envelope, cut to zero at
 * and beyond the cutoff):
 *   rbf (E, k)   = env(x) sin(freq_q x)
 *   sbe (E, n k) = env(x) N_lq j_l(z_lq x)     (j_l by series / recurrence, in double)
 *   An edge with x >= 1 gives exact zero rows and, in bwd, an exact zero grad_dist.
 *   bwd: as gmp_sph_edge_basis_bwd_f32 (grad_freq through ordered partials, no atomics).
 *
 * Triplet projection for L layers at once, sbf_t[l k + q] = sbe[idx_kj[t]][l k + q]
 * Y_l0(angle_t) (only the n Legendre values of a triplet are formed; never written):
 *   S (L, T, b) = W_sbf1[l] sbf_t,   w_sbf1_t (n k, ld) feature-major, column layer * b + j,
 *   ld = L b rounded up to a multiple of 8, padding zero.
 *   bwd: grad_w (n k ld) through partials (gmp_dime_triplet_proj_bwd_partial_rows(T) rows of
 *        that width), summed in a fixed order.  If grad_sbe_rows (T, n k) and grad_angle (T)
 *        are given (both or neither) the geometry gradients are written too; the caller sums
 *        grad_sbe_rows per edge over the CSR of idx_kj.
 *   emb: the materialised sbf (T, n k) (tests, baselines).
 * An idx_kj outside [0, E) contributes a zero row.
 * ------------------------------------------------------------------------------------------ */
int gmp_dime_edge_basis_fwd_f32(const float* dist, int64_t n_edges, float cutoff,
                                int envelope_exponent, const float* freq, int num_radial,
                                const float* zeros, const float* norm, int num_spherical,
                                float* rbf, float* sbe, void* stream);
int64_t gmp_dime_edge_basis_bwd_partial_rows(int64_t n_edges);
int gmp_dime_edge_basis_bwd_f32(const float* dist, int64_t n_edges, float cutoff,
                                int envelope_exponent, const float* freq, int num_radial,
                                const float* zeros, const float* norm, int num_spherical,
                                const float* grad_rbf, const float* grad_sbe, float* grad_dist,
                                float* grad_freq, float* freq_partials, void* stream);
int gmp_dime_triplet_proj_fwd_f32(int64_t n_triplets, int64_t n_edges, int num_spherical,
                                  int num_radial, const float* sbe, const float* angle,
                                  const int64_t* idx_kj, const float* pref, const float* w_sbf1_t,
                                  int n_layers, int b, float* S, void* stream);
int gmp_dime_triplet_emb_f32(int64_t n_triplets, int64_t n_edges, int num_spherical,
                             int num_radial, const float* sbe, const float* angle,
                             const int64_t* idx_kj, const float* pref, float* sbf, void* stream);
int64_t gmp_dime_triplet_proj_bwd_partial_rows(int64_t n_triplets);
int gmp_dime_triplet_proj_bwd_f32(int64_t n_triplets, int64_t n_edges, int num_spherical,
                                  int num_radial, const float* sbe, const float* angle,
                                  const int64_t* idx_kj, const float* pref, const float* w_sbf1_t,
                                  int n_layers, int b, const float* grad_S, float* grad_w,
                                  float* partials, float* grad_sbe_rows, float* grad_angle,
                                  void* stream);

/* Second backwards of K18d (a loss on the forces differentiates PyG's BesselBasisLayer /
 * SphericalBasisLayer, models/dimenet.py:86-90, twice).  Additions only.
 *
 * Edge basis: the first backward maps (grad_rbf, grad_sbe) to (grad_dist, grad_freq); a_dist (E)
 * and a_freq (k) are the cotangents of those (each may be NULL, as may grad_rbf / grad_sbe).
 * Writes gg_rbf (E, k), gg_sbe (E, n k) (the gradients w.r.t. grad_rbf / grad_sbe), h_dist (E)
 * and h_freq (k) (w.r.t. dist / freq; h_freq through gmp_dime_edge_basis_bwd2_partial_rows(E)
 * ordered partial rows of k).  Double arithmetic rounded once; an edge with x >= 1 gives exact
 * zeros in all four.
 *
 * Triplet projection: the first backward maps grad_S (L, T, b) to (grad_w, grad_sbe, grad_angle);
 * a_w_t (n k, ld, feature-major as w_sbf1_t), a_sbe (E, n k), a_angle (T) are their cotangents
 * (each may be NULL).  Writes gg_S (L, T, b), h_w (n k, ld) through partials
 * (gmp_dime_triplet_proj_bwd2_partial_rows(T) rows of n k ld) and, if given (both or neither),
 * h_sbe_rows (T, n k) (summed per edge by the caller over the CSR of idx_kj) and h_angle (T).
 * Up to three kernels; no atomics.  T = 0: GMP_OK and a zero h_w. */
int64_t gmp_dime_edge_basis_bwd2_partial_rows(int64_t n_edges);
int gmp_dime_edge_basis_bwd2_f32(const float* dist, int64_t n_edges, float cutoff,
                                 int envelope_exponent, const float* freq, int num_radial,
                                 const float* zeros, const float* norm, int num_spherical,
                                 const float* grad_rbf, const float* grad_sbe,
                                 const float* a_dist, const float* a_freq, float* gg_rbf,
                                 float* gg_sbe, float* h_dist, float* h_freq,
                                 float* freq_partials, void* stream);
int64_t gmp_dime_triplet_proj_bwd2_partial_rows(int64_t n_triplets);
int gmp_dime_triplet_proj_bwd2_f32(int64_t n_triplets, int64_t n_edges, int num_spherical,
                                   int num_radial, const float* sbe, const float* angle,
                                   const int64_t* idx_kj, const float* pref,
                                   const float* w_sbf1_t, int n_layers, int b,
                                   const float* grad_S, const float* a_sbe, const float* a_angle,
                                   const float* a_w_t, float* gg_S, float* h_w, float* partials,
                                   float* h_sbe_rows, float* h_angle, void* stream);

/* ------------------------------------------------------------------------------------------
 * K19d DimeNet++ triplet interaction of one layer (InteractionPPBlock), K19 with one factor:
 *   out[s, c] = sum_{p in [rowptr[s], rowptr[s+1])} src[gather_idx[t], c] (W_sbf2 S_t)[c],
 *   t = perm ? perm[p] : p
 * src (n_src, I), S (T, b), w_sbf2 (I, b), out (n_seg, I); rowptr / perm / gather_idx as K19
 * (the message m, or grad_xd over the CSR of idx_kj).  One wave per segment, fixed order.
 *   bwd (b <= 16, any I >= 1): grad_S (T, b) and grad_w (I, b) through partials
 *   (gmp_triplet_interact1_bwd_partial_rows(E) rows of I b), summed in wave order.  The weight
 *   gradient accumulators live in registers (lane = channel, 64 channels per pass).
 *   GMP_ERR_UNSUPPORTED when I b floats exceed the forward's LDS cap; GMP_OK and a zero grad_w
 *   at E = 0 or T = 0.
 * ------------------------------------------------------------------------------------------ */
int gmp_triplet_interact1_fwd_f32(int64_t n_seg, int64_t n_src, int64_t n_triplets, int64_t I,
                                  int b, const float* src, const float* S, const float* w_sbf2,
                                  const int64_t* gather_idx, const int64_t* perm,
                                  const int64_t* rowptr, float* out, void* stream);
int64_t gmp_triplet_interact1_bwd_partial_rows(int64_t n_edges);
int gmp_triplet_interact1_bwd_f32(int64_t n_edges, int64_t n_triplets, int64_t I, int b,
                                  const float* grad_m, const float* xd, const float* S,
                                  const float* w_sbf2, const int64_t* idx_kj,
                                  const int64_t* offsets, float* grad_S, float* grad_w,
                                  float* partials, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GMP_H_ */
