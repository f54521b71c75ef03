/*
 * gts_hip.h — C ABI of libgts_hip.so, the MI355X (gfx950) kernels behind the GNN
 * node-classification path of rsinghlab/GNN-Tumor-Seg.
 *
 * The reference has no FFI of its own: its arithmetic is reached through DGL's Python
 * API.  Each entry point below names the reference call site (file:line under
 * /root/reference) and the DGL operator it stands in for.
 *
 * Conventions (all entry points)
 *   - every pointer is a DEVICE pointer owned by the caller; the library allocates
 *     nothing, frees nothing and keeps no state between calls (re-entrant);
 *   - `stream` is a hipStream_t (NULL = default stream); work is only enqueued, never
 *     synchronised; the device is whatever the caller made current;
 *   - return value: 0 on success, GTS_ERR_* (<0) for a rejected argument, otherwise a
 *     positive hipError_t from the launch.  Nothing throws or aborts;
 *   - feature matrices are dense row-major fp32; graphs are int32 CSR
 *     (E < 2^31, N < 2^31).  "in-CSR" = rows are destinations, entries are the
 *     sources of their in-edges in COO order; "out-CSR" = rows are sources.
 */
#ifndef GTS_HIP_H
#define GTS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GTS_OK 0
#define GTS_ERR_NULL (-1)    /* a required pointer is NULL            */
#define GTS_ERR_SHAPE (-2)   /* negative / overflowing / unsupported shape */
#define GTS_ERR_ARGKIND (-3) /* unsupported arg_bytes / mode value    */

/* ABI version, bumped when a signature changes. */
int32_t gts_abi_version(void);
/* Static string for a GTS_ERR_* / hipError_t code returned by this library. */
const char* gts_error_string(int32_t code);

/* ---- K1: copy_u + max reducer (forward) -------------------------------------------
 * Replaces DGL update_all(copy_u('h','m'), max('m','neigh')) inside SAGEConv('pool'),
 * reached from model/networks.py:25,28,30.
 *   out[v,f] = max_{k} x[indices[indptr[v]+k], f]; first maximum wins (strict '<');
 *   +-inf results and empty rows give 0 and select nothing.
 *   arg (optional, arg_bytes = 0 -> not written): the SLOT k of the winner inside
 *   row v, as uint8 (arg_bytes=1, slot 0xFF = none; needs max in-degree <= 254)
 *   or int32 (arg_bytes=4, -1 = none); layout [n_dst, n_feat].
 *   relu_input != 0: x is a ReLU output (SAGEConv-pool: x = relu(fc_pool(h))); a maximum that
 *   is not positive is recorded as "none", because relu'(0) = 0 stops its gradient anyway — the
 *   backward (K2) then gives the gradient w.r.t. the PRE-activation without reading x. */
int32_t gts_spmm_max_fwd_f32(const int32_t* indptr, const int32_t* indices, const float* x,
                             float* out, void* arg, int32_t arg_bytes, int32_t relu_input,
                             int64_t n_dst, int64_t n_feat, void* stream);

/* ---- K2: max reducer (backward), gather form over the out-CSR -----------------------
 * Replaces the autograd of K1 (DGL scatters gout by argmax).
 *   gx[u,f] = sum_{e in out(u)} [arg[t_indices[e], f] == t_slot[e]] * gout[t_indices[e], f]
 *   t_slot[e] = position of edge e inside its destination's in-CSR row.
 *   relu_src (optional): if given, gx[u,f] is zeroed where relu_src[u,f] <= 0
 *   (the ReLU that precedes the pooling, SAGEConv: relu(fc_pool(h))). */
int32_t gts_spmm_max_bwd_f32(const int32_t* t_indptr, const int32_t* t_indices,
                             const int32_t* t_slot, const float* gout, const void* arg,
                             int32_t arg_bytes, const float* relu_src, float* gx,
                             int64_t n_src, int64_t n_feat, void* stream);
/* K2 over a gradient of rank 4 that is never stored (the 4-class top layer of a SAGEConv('pool') stack,
 * model/networks.py:28-30 under autograd: gout = g @ fc_neigh.weight):
 *   gx = gts_spmm_max_bwd_f32(gout = gts_linear_bwd_input_t_f32(g, w^T), arg)     bit for bit, for
 *   g [n_src, rank], w [rank, n_feat] as torch stores fc_neigh.weight, rank = 4, n_feat = 256 (else GTS_ERR_SHAPE).
 * A lane forms gout[t_indices[e], f] in registers from the destination's 16-byte g row and its columns of w. */
int32_t gts_spmm_max_bwd_lowrank_f32(const int32_t* t_indptr, const int32_t* t_indices,
                                     const int32_t* t_slot, const float* g, const float* w, const void* arg,
                                     int32_t arg_bytes, float* gx, int64_t n_src, int64_t n_feat,
                                     int64_t rank, void* stream);

/* ---- K1 / K2 over a cluster row schedule (F = 256): LDS-staged neighbour tiles ---------------
 * Same operators as gts_spmm_max_fwd_f32 / gts_spmm_max_bwd_f32 (DGL copy_u + max inside SAGEConv('pool'),
 * model/networks.py:25,28,30, and its autograd), bit-identical results, different work distribution: the rows
 * of the CSR are dealt to workgroups as clusters that share their neighbour rows; persistent workgroups stage
 * each distinct neighbour row of a cluster in LDS once (LDS-DMA, several clusters ahead) instead of fetching
 * one row per edge behind a chain of dependent index loads.
 *
 * gts_cluster_schedule (HOST function: host pointers, no GPU call) builds the schedule of one CSR once per
 * graph: (indptr, indices) is the CSR to schedule, (t_indptr, t_indices) its transpose, edge_tag an optional
 * per-edge payload in 0..255 (K2: t_slot).  A cluster holds <= max_rows rows, <= max_srcs (<= 256) distinct
 * neighbours and <= max_edges (<= 65535) PADDED edges (every row's edge list is padded to whole chunks of 8);
 * rows keep their edges in CSR slot order.  One fixed-size RECORD per cluster is written to rec[c * W ...],
 * W = gts_cluster_record_words(max_rows, max_srcs, LW, with_tag) int32 words with LW = ((max_edges + 3) / 4
 * rounded up to a multiple of 4):
 *   words 0..3: n_rows, n_srcs, padded edges, 0 | row ids [max_rows] | neighbour ids [max_srcs] (entries
 *   past n_srcs repeat the last one) | per row [max_rows]: index of its first 8-edge chunk (low 16 bits),
 *   degree (high 16 bits) | uint8 per padded edge: position of its neighbour in the cluster's list [4 LW]
 *   (pads repeat the row's last edge) | uint8 per padded edge: its tag [4 LW] (only with edge_tag); every
 *   section starts on a multiple of 4 words.
 * rec may be NULL (count only); at most rec_capacity records are written.  Outputs: the number of clusters,
 * the neighbour rows staged over all clusters, the largest padded edge count of a cluster (a caller may re-pack the
 * records with a smaller LW).  Returns GTS_ERR_SHAPE when a row's degree exceeds max_srcs / max_edges or a tag
 * does not fit a byte, GTS_ERR_ARGKIND for limits outside the ranges above or records above 512 words.
 * gts_cluster_lds_bytes: LDS bytes of one ring slot for (max_rows, max_srcs, LW), kind 0 = forward, 1 =
 * backward; the kernels need at least two slots in the CU's 160 KiB.
 * The device entry points take a DEVICE copy of the records (stride W for the LW passed); n_feat must be 256,
 * arg_bytes 0 / 1 (forward) or 1 (backward), n_rows * 1024 < 2^32. */
int64_t gts_cluster_record_words(int32_t max_rows, int32_t max_srcs, int32_t loc_words, int32_t with_tag);
int32_t gts_cluster_schedule(const int32_t* indptr, const int32_t* indices, const int32_t* t_indptr,
                             const int32_t* t_indices, const int32_t* edge_tag, int64_t n_rows,
                             int32_t max_rows, int32_t max_srcs, int32_t max_edges, int32_t* rec,
                             int64_t rec_capacity, int64_t* n_clusters, int64_t* n_staged,
                             int32_t* max_cluster_edges);
int64_t gts_cluster_lds_bytes(int32_t max_rows, int32_t max_srcs, int32_t loc_words, int32_t kind);
int32_t gts_spmm_max_fwd_cluster_f32(const int32_t* rec, int64_t n_clusters, int32_t max_rows, int32_t max_srcs,
                                     int32_t loc_words, const float* x, float* out, void* arg,
                                     int32_t arg_bytes, int32_t relu_input, int64_t n_rows, int64_t n_feat,
                                     uint32_t* counters, void* stream);
int32_t gts_spmm_max_bwd_cluster_f32(const int32_t* rec, int64_t n_clusters, int32_t max_rows, int32_t max_srcs,
                                     int32_t loc_words, const float* gout, const void* arg, int32_t arg_bytes,
                                     float* gx, int64_t n_rows, int64_t n_feat, uint32_t* counters, void* stream);
/* `counters`: GTS_CLUSTER_COUNTER_WORDS words of caller scratch, ZERO on entry; a launch that uses them leaves them zero (the last workgroup
 * of each XCD to finish resets them), so one zeroed buffer per stream serves every launch on it.  On launches of 16 and more units per
 * workgroup (GTS_OPT_CLUSTER_DEALING) the persistent workgroups of an XCD take their units off one counter, which keeps the units in flight
 * neighbours in the walk whatever each workgroup's pace — their halo rows then meet in the XCD's L2 (profiles/r04/gat_l2_replay.log,
 * k12_dealing_ab.log).  NULL: static round-robin dealing (same values, more re-fetched rows at streaming sizes).
 * GTS_ERR_SHAPE, before anything is launched: an LDS plan above 160 KiB, records above 512 words, max_srcs above 64 x the waves of a
 * workgroup, or records of more 256-word pieces than a workgroup has waves (GTS_OPT_CLUSTER_CONSUMERS = 1 with records above 256 words). */
#define GTS_CLUSTER_COUNTER_WORDS 256
/* 1 when a launch over these records would deal its units off `counters` (so that a caller who carves them out of a scratch block knows whether
 * they need zeroing at all), 0 when it deals statically */
int32_t gts_cluster_uses_counters(int64_t n_clusters, int32_t max_rows, int32_t max_srcs, int32_t loc_words, int32_t backward);

/* ---- K3/K4: copy_u + sum / mean / gcn reducers (forward and backward) ---------------
 * Replaces DGL update_all(copy_u, sum|mean) of SAGEConv('mean'|'gcn')
 * (model/networks.py:73,75 via :25-30) and, on the out-CSR, their autograd.
 *   s[v,f]   = sum_k  x[idx_k, f] / (div_in ? div_in[idx_k] : 1)   (slot order)
 *   if add_self: s[v,f] += x[v,f] / (div_in ? div_in[v] : 1)        (needs square graph)
 *   out[v,f] = s[v,f] / (div_out ? div_out[v] : 1)   (+ accum[v,f] when accum is given: the gradient
 *              that reached row v by another path, e.g. through fc_self beside the neighbour term)
 * mean fwd: div_out = max(deg,1); mean bwd: out-CSR, div_in = max(deg,1);
 * gcn  fwd: add_self, div_out = deg+1;  gcn bwd: out-CSR, add_self, div_in = deg+1. */
int32_t gts_spmm_sum_f32(const int32_t* indptr, const int32_t* indices, const float* x,
                         float* out, const float* div_in, const float* div_out, const float* accum,
                         int32_t add_self, int64_t n_out, int64_t n_feat, void* stream);

/* ---- K5-K7: GATConv attention + aggregation (forward) -------------------------------
 * Replaces apply_edges(u_add_v) + leaky_relu + edge_softmax + update_all(u_mul_e, sum)
 * inside GATConv, reached from model/networks.py:46,52,56, plus the layer's tail
 * (+ res_fc(h) + bias, activation) on the way out.
 *   e_k = leaky_relu(el[src_k,h] + er[v,h]);  a_k = softmax_k(e_k) over row v (max-subtracted)
 *   out[v,h,:] = act( sum_k a_k * ft[src_k,h,:] + residual[v,h,:] + bias[h,:] )
 *   ft [n,H,D], el/er [n,H], out [n,H,D], attn [E,H] in in-CSR slot order (saved for K8);
 *   bias [H*D] and residual [n,H,D] optional; activation 0 = none, 1 = ELU (alpha 1). */
int32_t gts_gat_fwd_f32(const int32_t* indptr, const int32_t* indices, const float* ft,
                        const float* el, const float* er, float negative_slope, const float* bias,
                        const float* residual, int32_t activation, float* out, float* attn,
                        int64_t n, int64_t heads, int64_t dim, void* stream);
/* el[n,h] = <ft[n,h,:], attn_l[h,:]>, er[n,h] = <ft[n,h,:], attn_r[h,:]>  (GATConv: (feat * attn).sum(-1)) */
int32_t gts_gat_scores_f32(const float* ft, const float* attn_l, const float* attn_r, float* el,
                           float* er, int64_t n, int64_t heads, int64_t dim, void* stream);

/* ---- K8: GATConv backward ------------------------------------------------------------
 * Atomics-free passes:
 *  (0) gts_gat_act_bwd_f32: g_pre = gout * act'(out) (ELU / ReLU through its output; activation 0 leaves
 *      gout as is and g_pre may be NULL) and g_bias[c] = sum_n g_pre[n,c] (optional), cols = H*D.
 *  (1) per destination row (in-CSR):  ga_k = <g_pre[v,h,:], ft[src_k,h,:]>,
 *      ge_k = a_k*(ga_k - sum_j a_j ga_j) * leaky'(el[src_k]+er[v]);  ger[v,h] = sum_k ge_k;
 *      ge [E,H] written in in-CSR slot order.
 *  (2) per source row (out-CSR): gft[u,h,:] = sum_{e in out(u)} a[pos(e)] * g_pre[dst_e,h,:]
 *      (+ gel[u,h]*attn_l[h,:] + ger[u,h]*attn_r[h,:] when attn_l/attn_r/ger are given: the
 *      gradient of the score dot products), gel[u,h] = sum_e ge[pos(e)].
 *      t_pos[e] = absolute in-CSR position of out-edge e.
 *  (3) gts_gat_param_grad_f32: g_attn_l[h,:] = sum_n gel[n,h] ft[n,h,:], g_attn_r with ger.
 * (0) and (3) reduce over the node axis through `workspace` in a fixed order (bitwise reproducible): per-chunk column
 * sums of ceil(n / 512) rows each, then added 16 chunks abreast.  gts_gat_reduce_workspace(n, H*D) is the size of TWO
 * such arrays of chunk sums (0 for n <= 0 or a width that is not a multiple of 4): (3) needs all of it, (0) needs half
 * of it and only when g_bias is asked for.  A smaller workspace is refused before anything is launched.
 * In (0) g_pre may be gout itself (each element is read, then written, by one thread). */
int32_t gts_gat_bwd_edge_f32(const int32_t* indptr, const int32_t* indices, const float* ft,
                             const float* el, const float* er, const float* attn,
                             const float* gout, float negative_slope, float* ge, float* ger,
                             int64_t n, int64_t heads, int64_t dim, void* stream);
int32_t gts_gat_bwd_src_f32(const int32_t* t_indptr, const int32_t* t_indices,
                            const int32_t* t_pos, const float* attn, const float* ge,
                            const float* gout, const float* attn_l, const float* attn_r,
                            const float* ger, float* gft, float* gel, int64_t n, int64_t heads,
                            int64_t dim, void* stream);
int64_t gts_gat_reduce_workspace(int64_t n, int64_t cols);
int32_t gts_gat_act_bwd_f32(const float* gout, const float* out, int32_t activation, float* g_pre,
                            float* g_bias, float* workspace, int64_t workspace_bytes, int64_t n,
                            int64_t cols, void* stream);
int32_t gts_gat_param_grad_f32(const float* ft, const float* gel, const float* ger, float* g_attn_l,
                               float* g_attn_r, float* workspace, int64_t workspace_bytes, int64_t n,
                               int64_t heads, int64_t dim, void* stream);

/* ---- K5-K8 at D = 256 over a cluster row schedule (LDS-staged neighbour tiles; csrc/gts_gat_cluster.hip) -----------------
 * The same GATConv aggregation (model/networks.py:46,52,56 -> dgl GATConv: edge_softmax, u_mul_e + sum) and the source pass
 * of its backward, computed per cluster of a schedule made by gts_cluster_schedule (records `rec`, limits max_rows / max_srcs,
 * loc_words, tagged = the records carry the tag section): a unit of work is one 512-byte column half of one head of one
 * cluster, its distinct neighbour slices staged once in LDS.  Same values as gts_gat_fwd_f32 / gts_gat_bwd_src_f32 bit for
 * bit (edges in CSR slot order inside every row, the softmax in the plain kernel's association); no residual term here.
 *   gts_gat_attn_f32: attn [E, H] alone (max_degree: the largest in-degree, <= 64).
 *   forward: in-CSR (indptr, indices) + a schedule of the in-CSR;  bias [H*256] optional.
 *   backward: out-CSR (t_indptr, t_pos) + a schedule of the out-CSR;  attn_lr = attn_l | attn_r stacked [2, H*256] (with ger)
 *             or both null; gel [n, H] is written as by gts_gat_bwd_src_f32.  max_degree: the largest out-degree (or -1:
 *             unknown); with rows of at most one 8-edge chunk (<= 8) the weight pass takes a faster form, same values.
 * workspace >= gts_gat_cluster_workspace(n_clusters, max_rows, loc_words, heads, backward) bytes. */
int64_t gts_gat_cluster_workspace(int64_t n_clusters, int32_t max_rows, int32_t loc_words, int64_t heads, int32_t backward);
int32_t gts_gat_attn_f32(const int32_t* indptr, const int32_t* indices, const float* el, const float* er,
                         float negative_slope, float* attn, int64_t n, int64_t heads, int64_t max_degree, void* stream);
int32_t gts_gat_fwd_cluster_f32(const int32_t* indptr, const int32_t* indices, const int32_t* rec, int64_t n_clusters,
                                int32_t max_rows, int32_t max_srcs, int32_t loc_words, int32_t tagged, const float* ft,
                                const float* el, const float* er, float negative_slope, const float* bias,
                                int32_t activation, float* out, float* attn, float* workspace, int64_t workspace_bytes,
                                int64_t n, int64_t heads, int64_t dim, int64_t max_degree, void* stream);
/* edge pass (step 1 of gts_gat_bwd_edge_f32's job, same ge [E, H] / ger [n, H] bit for bit): in-CSR + a schedule of the in-CSR whose
 * images also hold the rows' own gradient slices; rows of one 8-edge chunk only (max_degree <= 8, else GTS_ERR_SHAPE).
 * workspace >= 2 * gts_gat_cluster_workspace(n_clusters, max_rows, loc_words, heads, 0) bytes (the two half dot products). */
int32_t gts_gat_bwd_edge_cluster_f32(const int32_t* indptr, const int32_t* indices, const int32_t* rec, int64_t n_clusters,
                                     int32_t max_rows, int32_t max_srcs, int32_t loc_words, int32_t tagged, const float* ft,
                                     const float* el, const float* er, const float* attn, const float* gout,
                                     float negative_slope, float* ge, float* ger, float* workspace, int64_t workspace_bytes,
                                     int64_t n, int64_t heads, int64_t dim, int64_t max_degree, void* stream);
int32_t gts_gat_bwd_src_cluster_f32(const int32_t* t_indptr, const int32_t* t_pos, const int32_t* rec, int64_t n_clusters,
                                    int32_t max_rows, int32_t max_srcs, int32_t loc_words, int32_t tagged,
                                    const float* attn, const float* ge, const float* gout, const float* attn_lr,
                                    const float* ger, float* gft, float* gel, float* workspace, int64_t workspace_bytes,
                                    int64_t n, int64_t heads, int64_t dim, int64_t max_degree, void* stream);

/* ---- K12: node -> voxel projection ----------------------------------------------------
 * Replaces data_processing/graph_io.py:21-24 (project_nodes_to_img) and
 * scripts/generate_gnn_predictions.py:55-61 (save_voxel_logits):
 *   out[i, :] = (svs[i] < 0 ? bg_row : table[svs[i], :]) for i in [0, n_vox).
 * svs holds supervoxel ids in [-1, n_rows) (int16, mri2graph/graphgen.py:77); any
 * negative id selects the background row, exactly numpy's table_plus_bg[-1].
 * Rows are `row_bytes` opaque bytes (4, 8 or 16): int64 labels, fp32 x4 logits, ... */
int32_t gts_project_rows_i16(const int16_t* svs, const void* table, const void* bg_row,
                             void* out, int64_t n_vox, int64_t n_rows, int32_t row_bytes,
                             void* stream);
/* Fused argmax + projection: out[i] = argmax_c logits[svs[i], c] (first maximum, as
 * torch.max(logits,1), generate_gnn_predictions.py:66), 0 for background; int16 out
 * with an optional 4-entry relabel table (swap_labels_to_brats, preprocess_dataset.py:159). */
int32_t gts_project_argmax_i16(const int16_t* svs, const float* logits, const int16_t* relabel,
                               int16_t* out, int64_t n_vox, int64_t n_rows, int64_t n_classes,
                               void* stream);

/* gts_project_argmax_i16 over a [dim_x, dim_y, dim_z] partitioning that also reports which
 * planes hold tumour: occupancy is a caller-zeroed uint8[dim_x + dim_y + dim_z]; byte x,
 * dim_x + y, dim_x + dim_y + z is set to 1 when some voxel of that plane gets a non-zero
 * label.  These are `mask.any(axis=...)` of determine_tumor_crop (data_processing/
 * image_processing.py:8-17, reached from scripts/generate_joint_predictions.py:66) before its
 * one-voxel dilation, which the host applies to the three vectors. */
int32_t gts_project_argmax_occupancy_i16(const int16_t* svs, const float* logits, int16_t* out,
                                         uint8_t* occupancy, int64_t dim_x, int64_t dim_y,
                                         int64_t dim_z, int64_t n_rows, int64_t n_classes,
                                         void* stream);

/* ---- K16/K17: glue between the GNN and the refinement CNN -----------------------------------
 * Replace the tensor indexing of predict_one_sample (scripts/generate_joint_predictions.py:
 * 59-73) and combine_logits_and_image (model/cnn_model.py:85-88).  A crop is the outer product
 * of three ascending index vectors xs [cx], ys [cy], zs [cz] (np.ix_ of boolean plane masks),
 * int32 on the device, into a volume whose two inner extents are dim_y, dim_z.
 *
 * crop_concat: out[c, i, j, k] (fp32, [img_channels + row_channels, cx, cy, cz] contiguous)
 *   = img[xs[i], ys[j], zs[k], c]                         for c <  img_channels
 *   = table_plus_bg[svs[xs[i], ys[j], zs[k]]][c - img_channels]   otherwise,
 *   table [n_rows, row_channels] node logits, bg_row the background logits (id -1), img
 *   [X, Y, Z, img_channels] channels-last.  Exact copies. */
int32_t gts_crop_concat_f32(const float* img, const int16_t* svs, const float* table,
                            const float* bg_row, const int32_t* xs, const int32_t* ys,
                            const int32_t* zs, float* out, int64_t cx, int64_t cy, int64_t cz,
                            int64_t dim_y, int64_t dim_z, int64_t n_rows, int64_t img_channels,
                            int64_t row_channels, void* stream);
/* argmax_scatter: out[xs[i], ys[j], zs[k]] = argmax_c scores[c, i, j, k] (first maximum, as
 * torch.argmax; optional relabel table), scores [n_classes, cx, cy, cz]; the other voxels of the
 * caller-zeroed int16 volume `out` are left alone. */
int32_t gts_argmax_scatter_i16(const float* scores, const int16_t* relabel, const int32_t* xs,
                               const int32_t* ys, const int32_t* zs, int16_t* out, int64_t cx,
                               int64_t cy, int64_t cz, int64_t dim_y, int64_t dim_z,
                               int64_t n_classes, void* stream);
/* J1 crop_concat_rows: crop_concat in channels-last, the layout gts_conv3d_* read (joint GNN + CNN
 * training, no counterpart in the reference: scripts/train_refinement_cnn.py:21-22 declines to build it):
 *   out[t, :] (fp32, [cx * cy * cz, img_channels + row_channels]) = [img[v, :], table_plus_bg[svs[v]]]
 *   for crop voxel t = (i * cy + j) * cz + k with source voxel v = (xs[i], ys[j], zs[k]).  Same id rules
 *   and limits as crop_concat; exact copies (bit-equal to crop_concat's output moved to channels-last). */
int32_t gts_crop_concat_rows_f32(const float* img, const int16_t* svs, const float* table,
                                 const float* bg_row, const int32_t* xs, const int32_t* ys,
                                 const int32_t* zs, float* out, int64_t cx, int64_t cy, int64_t cz,
                                 int64_t dim_y, int64_t dim_z, int64_t n_rows, int64_t img_channels,
                                 int64_t row_channels, void* stream);
/* J2 crop_concat_rows_bwd: the adjoint of J1 with respect to `table`:
 *   d_table[n, c] = sum over the crop voxels t whose source voxel took table row n of
 *                   dx[t, img_channels + c],   dx [cx * cy * cz, img_channels + row_channels].
 * Voxels that took the background row contribute to nothing; rows without a voxel in the box get 0.0.
 * list_ptr [n_rows + 1], list_vox: per table row the linear indices (x * dim_y + y) * dim_z + z of the
 * voxels that resolve to it (numpy's wrap of negative ids included), ascending; inv_x [dim_x], inv_y
 * [dim_y], inv_z [dim_z]: plane index -> index inside the crop, or -1 for a plane outside it (all int32,
 * on the device).  The list does not depend on the box.  Entries outside the volume or the box are
 * skipped.  Every sum is formed in a fixed order (no float atomics): two calls give identical bits. */
int32_t gts_crop_concat_rows_bwd_f32(const float* dx, const int32_t* list_ptr, const int32_t* list_vox,
                                     const int32_t* inv_x, const int32_t* inv_y, const int32_t* inv_z,
                                     float* d_table, int64_t cx, int64_t cy, int64_t cz, int64_t dim_x,
                                     int64_t dim_y, int64_t dim_z, int64_t n_rows, int64_t img_channels,
                                     int64_t row_channels, void* stream);

/* ---- K14: AdamW step over one flat fp32 buffer ---------------------------------------------
 * torch.optim.AdamW(net.parameters(), lr, weight_decay).step() (model/gnn_model.py:28,46), same
 * update rule (decoupled decay, bias-corrected moments, no amsgrad), for parameters, gradients
 * and both moment buffers laid out as ONE contiguous fp32 range each.  `step` is the 1-based
 * count of this update (for the bias corrections).  In-place on param / exp_avg / exp_avg_sq. */
int32_t gts_adamw_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                      double lr, double beta1, double beta2, double eps, double weight_decay,
                      int64_t step, void* stream);

/* ---- K15: label coincidence counts for the Dice metrics -------------------------------------
 * Replaces the numpy mask arithmetic of model/evaluation.py:24-46 (count_node_labels,
 * calculate_node_dices), :64-79 (voxel Dice in calculate_brats_metrics) and :98-106
 * (calculate_dice_from_logical_array) reached from GNN.evaluate, model/gnn_model.py:76-87.
 * counts[5*cp + ct] += #{ i : class(pred[i]) == cp and class(truth[i]) == ct }, where
 * class(v) = v for 0..3 and 4 for any other value.  counts is a caller-owned int64[25] on the
 * device that the call ADDS to (zero it first); workspace is caller-owned device scratch of at
 * least gts_label_confusion_workspace(n) bytes.  Integer sums: exact, independent of scheduling. */
int64_t gts_label_confusion_workspace(int64_t n);
int32_t gts_label_confusion_i16(const int16_t* pred, const int16_t* truth, int64_t* counts,
                                void* workspace, int64_t workspace_bytes, int64_t n, void* stream);

/* ---- K11: dense fp32 layer GEMMs on the matrix cores -------------------------------------
 * Replace the nn.Linear calls inside DGL's SAGEConv / GATConv (fc_pool, fc_self + fc_neigh,
 * fc; reached from model/networks.py:25,28,30,46,52,56) and their autograd.  Exact fp32
 * (v_mfma_f32_32x32x2_f32).  All dims that index a contiguous axis must be multiples of 4.
 *
 * forward:  out[m, n] = act( sum_k a0[m,k] w0[n,k] + (a1 ? sum_k a1[m,k] w1[n,k] : 0) + bias[n] )
 *   a0 [M,K0], w0 [N,K0], a1 [M,K1], w1 [N,K1] row-major (torch Linear layout); bias optional;
 *   relu != 0 applies max(., 0).  The pair form is fc_self(h) + fc_neigh(m) in one pass.
 *   relu_bits (optional, n % 64 == 0, gts_relu_bits_bytes(m, n) bytes): out > 0 as one bit per element, written
 *   while out is stored — the ReLU mask the input-gradient calls below can read instead of the floats of `out`
 *   (1/32 of the bytes, and scalar loads that do not queue behind the epilogue's stores).  Layout: 64-bit word
 *   ((col / 64) * ceil(m / 4) + row / 4) * 4 + e, bit 16 * (row % 4) + (col % 64) / 4, holds
 *   out[row][64 * (col / 64) + 4 * ((col % 64) / 4) + e] > 0  (e = 0..3): one word = one wave-wide comparison of the
 *   epilogue that stores four rows x 64 columns as 16-byte pieces, and the words of a wave's 80 rows are consecutive.
 *   Bits of rows >= m are unspecified. */
int64_t gts_relu_bits_bytes(int64_t m, int64_t n);
/* 1 when the launches for an [m, n] output would write / read these bits inside their epilogues (the panel kernels of
 * the tall shapes); 0 when asking for them would only add a pass (callers then pass no relu_bits at all). */
int32_t gts_relu_bits_pay(int64_t m, int64_t n);
int32_t gts_linear_fwd_f32(const float* a0, const float* w0, const float* a1, const float* w1,
                           const float* bias, float* out, int64_t m, int64_t n, int64_t k0,
                           int64_t k1, int32_t relu, uint64_t* relu_bits, const float* const* packed,
                           void* stream);
/* Weights in FRAGMENT ORDER — the optional `packed` argument of gts_linear_fwd_f32, gts_linear_fwd_chain_f32,
 * gts_linear_bwd_input_t_f32 and gts_linear_bwd_input_chain_t_f32: a HOST array with one device pointer per weight
 * operand of the call, in argument order (w0, w1[, w2] resp. w0t, w1t[, w2t]; NULL entries and a NULL array are
 * allowed), each a copy of that operand made by gts_pack_weights_f32.  The nn.Linear weights inside SAGEConv
 * (model/networks.py:25-30) are read by every workgroup of a layer GEMM; as torch stores them ([out, in] row-major) a
 * wave's 16-row MFMA fragment is 64 pieces of 16 bytes 1 KiB apart — 64 accesses of the vector L1, whose access rate
 * bounds the tall panel kernels (profiles/r04/panel144_l1_bound.log) — in fragment order it is 1 KiB of consecutive
 * bytes (16 accesses).  Same values, same reduction order: results are bit-identical with and without the copies;
 * kernels other than the panel kernels ignore them and read the plain operand.
 *   B [n, k] = the operand as the GEMM reads it (rows = output columns, columns = reduction); G = ceil(k / 16):
 *   packed[((T * G + g) * 64 + lane) * 4 + e] = B[16 T + (lane & 15)][16 g + 4 (lane >> 4) + e], 0 past the edges;
 *   gts_packed_weight_floats(n, k) = ceil(n / 16) * G * 256 floats.
 * gts_pack_weights_f32: n_mats matrices src[q] [rows, cols] of one shape (HOST arrays of device pointers), one launch
 * per 32.  transposed = 0: B = src[q];  transposed = 1: B = src[q]^T (the input gradient's operand), and plain_t
 * (optional, only then) also receives src[q]^T row-major [cols, rows] — what gts_transpose_batch_f32 writes. */
int64_t gts_packed_weight_floats(int64_t n, int64_t k);
int32_t gts_pack_weights_f32(const float* const* src, float* const* dst, float* const* plain_t, int32_t n_mats,
                             int64_t rows, int64_t cols, int32_t transposed, void* stream);
/* input gradient:  gin[m, k] = sum_n g0[m,n] w0[n,k] + (g1 ? sum_n g1[m,n] w1[n,k] : 0)
 *   g0 [M,N0], w0 [N0,K], g1 [M,N1], w1 [N1,K].  relu_mask (optional, [M,K]): gin is zeroed
 *   where relu_mask <= 0, i.e. the ReLU backward of the layer that produced this input. */
int32_t gts_linear_bwd_input_f32(const float* g0, const float* w0, const float* g1, const float* w1,
                                 const float* relu_mask, float* gin, int64_t m, int64_t k,
                                 int64_t n0, int64_t n1, void* stream);
/* the same input gradient from TRANSPOSED weights (w0t [K,N0], w1t [K,N1], e.g. made once per
 * backward pass by gts_transpose_batch_f32): both GEMM operands are then reduction-contiguous, the
 * forward kernel's form — bitwise the same sums in the same order as gts_linear_bwd_input_f32.
 * relu_bits (optional, k % 64 == 0; relu_mask must be given too): relu_mask > 0 in the bit layout above, as written by
 * the forward call that produced relu_mask; the kernels that can use the bits never touch relu_mask, the others read
 * its floats as before — the result is the same either way. */
int32_t gts_linear_bwd_input_t_f32(const float* g0, const float* w0t, const float* g1, const float* w1t,
                                   const float* relu_mask, const uint64_t* relu_bits, float* gin, int64_t m,
                                   int64_t k, int64_t n0, int64_t n1, const float* const* packed, void* stream);
/* the same input gradient carried through the activation of the layer BELOW (a GATConv stack: the next layer's input IS the
 * ELU output of this one, model/networks.py:46-58,61-63), with that layer's bias gradient:
 *   gin[m, k] = (g0 w0 (+ g1 w1)) * act'(act_out),  act' through the activation's OUTPUT act_out [m, k]: activation 1 = ELU
 *   (1 where act_out > 0, act_out + 1 elsewhere), 2 = ReLU;  g_bias[k] = sum_m gin[m, k] (optional).
 * Tall operands with k % 256 == 0 and ELU: both ride in the GEMM's epilogue (no pass over gin, column sums per 80-row block
 * in `workspace` and added in fixed order); otherwise gts_linear_bwd_input_t_f32 followed by gts_gat_act_bwd_f32 in place.
 * gin is bitwise the same either way; g_bias is summed in a different (each time fixed) order.
 * workspace >= gts_linear_bwd_input_t_act_workspace(m, k) bytes when g_bias is asked for. */
int64_t gts_linear_bwd_input_t_act_workspace(int64_t m, int64_t k);
int32_t gts_linear_bwd_input_t_act_f32(const float* g0, const float* w0t, const float* g1, const float* w1t,
                                       const float* act_out, int32_t activation, float* gin, float* g_bias,
                                       float* workspace, int64_t workspace_bytes, int64_t m, int64_t k,
                                       int64_t n0, int64_t n1, const float* const* packed,
                                       void* stream);
/* GATConv's projection with its attention scores (model/networks.py:46,52,56 -> dgl GATConv: feat_src = fc(h).view(N, H, D);
 * el = (feat_src * attn_l).sum(-1); er likewise):  ft [m, heads*dim] = h [m, k] w_fc^T,  el/er [m, heads] = <ft[n,h,:], attn_l/r[h,:]>.
 * Tall operands with dim % 64 == 0: the dot products ride in the GEMM epilogue (partials per 64 columns in `workspace`,
 * >= gts_gat_fc_scores_workspace bytes, summed in fixed order); otherwise the GEMM is followed by gts_gat_scores_f32. */
int64_t gts_gat_fc_scores_workspace(int64_t m, int64_t heads, int64_t dim);
int32_t gts_gat_fc_scores_f32(const float* h, const float* w_fc, const float* attn_l, const float* attn_r,
                              float* ft, float* el, float* er, float* workspace, int64_t workspace_bytes,
                              int64_t m, int64_t heads, int64_t dim, int64_t k, const float* w_fc_packed, void* stream);
/* two GEMMs of a layer chain in one call (one launch when the operands are tall and <= 256 wide, otherwise two):
 *   out  [m, n]  = act (a0 w0^T (+ a1 w1^T) + bias)          exactly gts_linear_fwd_f32
 *   out2 [m, n2] = act2(out w2^T + bias2)                      exactly gts_linear_fwd_f32 on `out`
 * (SAGEConv-pool stack: fc_self + fc_neigh of layer L, then fc_pool of layer L+1 on the rows just produced).
 * The input-gradient form chains  gin = (g0 w0 (+ g1 w1)) (. mask)  and  gin2 = gin w2  on transposed weights
 * (w0t [k, n0], w1t [k, n1], w2t [k2, k]).  n (resp. k) must be a multiple of 4.  relu_bits: the mask bits of
 * `out` (written) resp. of relu_mask (read), as in gts_linear_fwd_f32 / gts_linear_bwd_input_t_f32. */
int32_t gts_linear_fwd_chain_f32(const float* a0, const float* w0, const float* a1, const float* w1,
                                 const float* bias, float* out, const float* w2, const float* bias2,
                                 float* out2, int64_t m, int64_t n, int64_t k0, int64_t k1, int32_t relu,
                                 int64_t n2, int32_t relu2, uint64_t* relu_bits, const float* const* packed,
                                 void* stream);
int32_t gts_linear_bwd_input_chain_t_f32(const float* g0, const float* w0t, const float* g1,
                                         const float* w1t, const float* relu_mask, const uint64_t* relu_bits,
                                         float* gin, const float* w2t, float* gin2, int64_t m, int64_t k,
                                         int64_t n0, int64_t n1, int64_t k2, const float* const* packed,
                                         void* stream);
/* dst[q][c, r] = src[q][r, c] for n_mats matrices of one shape [rows, cols] in one launch per 32
 * (src, dst: HOST arrays of device pointers).  Serves the transposed-weight form above: the
 * weights of a layer stack (torch Linear layout [out, in]) are turned once per backward pass. */
int32_t gts_transpose_batch_f32(const float* const* src, float* const* dst, int32_t n_mats,
                                int64_t rows, int64_t cols, void* stream);
/* weight gradients of n_problems (1..32) same-shape problems in ONE launch (the three weight
 * gradients of a SAGE layer, or those of a whole stack of equal layers):  gw[q][n, k] = sum_m g[q][m,n] a[q][m,k];
 * gb[q][n] = sum_m g[q][m,n] where gb && gb[q].  g, a, gw, gb are HOST arrays of device pointers.
 *   The reduction over the M nodes is split over workgroups into slabs in `workspace`
 *   (>= gts_linear_bwd_weight_workspace(m,n,k,n_problems) bytes, caller-owned scratch) that a
 *   second kernel adds in a fixed order: bitwise reproducible, no float atomics. */
int64_t gts_linear_bwd_weight_workspace(int64_t m, int64_t n, int64_t k, int32_t n_problems);
int32_t gts_linear_bwd_weight_f32(const float* const* g, const float* const* a, float* const* gw,
                                  float* const* gb, int32_t n_problems, float* workspace,
                                  int64_t workspace_bytes, int64_t m, int64_t n, int64_t k,
                                  void* stream);
/* Backward of a 4-wide FIRST SAGEConv('pool') layer (model/networks.py:25-30: SAGEConv(in_feats, 256, 'pool') under
 * autograd) in ONE pass over g [m, w], the gradient w.r.t. the layer's pre-activation output:
 *   gm [m, s1]       = g @ w_neigh            exactly gts_linear_bwd_input_f32(g, w_neigh)          (w_neigh [w, s1] as stored)
 *   gw_self [w, s0]  = g^T x, g_bias [w]      exactly gts_linear_bwd_weight_f32 of (g, x) with its bias
 *   gw_neigh [w, s1] = g^T m0                 exactly gts_linear_bwd_weight_f32 of (g, m0)
 * bit for bit: the three kernels behind those calls give a lane the same columns of a row, and this one keeps each one's
 * arithmetic.  Takes w = 256 and s0 = s1 = 4 (x [m, 4] the layer's input, m0 [m, 4] its max-pooled neighbours); every other
 * shape is GTS_ERR_SHAPE and keeps the calls above.  workspace >= gts_sage_first_layer_bwd_workspace(...) bytes (0 = shape
 * not taken), caller-owned scratch for the chunk partials of the two weight gradients. */
int64_t gts_sage_first_layer_bwd_workspace(int64_t m, int64_t w, int64_t s0, int64_t s1);
int32_t gts_sage_first_layer_bwd_f32(const float* g, const float* x, const float* m0, const float* w_neigh, float* gm,
                                     float* gw_self, float* g_bias, float* gw_neigh, float* workspace,
                                     int64_t workspace_bytes, int64_t m, int64_t w, int64_t s0, int64_t s1, void* stream);
/* The 256 -> 4 TOP SAGEConv('pool') layer of a training step in ONE pass over its input h [m, k] and its max-pooled
 * neighbours mx [m, k] (model/gnn_model.py:41-45: logits, CrossEntropyLoss(weight), backward), plus three small launches:
 *   logits [m, 4]      = h w_self^T + mx w_neigh^T + bias        exactly gts_linear_fwd_f32 (weights [4, k] as stored)
 *   out3               = { num, den, num / den }                 exactly gts_weighted_ce_f32 on those logits
 *   g [m, 4]           = gu / den (normalise = 1: one IEEE division per element) or gu (normalise = 0: the gradient of
 *                        the numerator, for a step that divides after its all-reduce), gu as gts_weighted_ce_f32 gives it
 *   gw_self, gw_neigh [4, k], g_bias [4]                         exactly gts_linear_bwd_weight_f32 of (g, h) with its bias
 *                                                                and of (g, mx)
 * bit for bit.  labels int64 [m] with gts_weighted_ce_f32's rules (-100 contributes nothing, any other label outside
 * [0, 4) makes the loss NaN), class_w [4] optional.  Takes k = 256 and n_classes = 4 with 0 < m < 2^31; every other shape
 * is GTS_ERR_SHAPE and keeps the calls above.  workspace >= gts_sage_top_layer_train_workspace(...) bytes (0 = shape not
 * taken), caller-owned scratch. */
int64_t gts_sage_top_layer_train_workspace(int64_t m, int64_t k, int64_t n_classes);
int32_t gts_sage_top_layer_train_f32(const float* h, const float* mx, const float* w_self, const float* w_neigh,
                                     const float* bias, const int64_t* labels, const float* class_w, int32_t normalise,
                                     float* logits, float* g, float* gw_self, float* gw_neigh, float* g_bias, float* out3,
                                     float* workspace, int64_t workspace_bytes, int64_t m, int64_t k, int64_t n_classes,
                                     void* stream);

/* ---- a whole stack of SAGEConv('pool') layers in one call each way -------------------------------
 * Replaces the layer loop of GraphSage.forward (model/networks.py:32-36: `for layer in self.layers: h = layer(graph, h)`)
 * over SAGEConv('pool') layers (model/networks.py:25,28,30: ReLU on all but the last, bias on) and its autograd.  HOST
 * orchestration: the calls enqueue this library's own kernels (K1 / K2, K11 with their chained, transposed and batched
 * forms) in a fixed order on `stream`; nothing is allocated.
 *   widths[0] = in_feats, widths[i + 1] = output width of layer i (all multiples of 4); n_layers <= 64.
 *   params[5 i .. 5 i + 4] = fc_pool.weight [w_i, w_i], fc_pool.bias [w_i], fc_self.weight [w_{i+1}, w_i],
 *                            fc_neigh.weight [w_{i+1}, w_i], bias [w_{i+1}]                       (device pointers)
 *   sched_*: optional cluster row schedule (gts_cluster_schedule) of the in-CSR (forward) / of the out-CSR tagged with
 *            t_slot (backward); NULL = plain K1 / K2.  Used by the 256-wide layers when arg_bytes allows.
 *   relu_bits: 1 = the forward GEMMs record the ReLU masks as bits (where gts_relu_bits_pay says so) and the backward reads
 *          them; 0 = the backward reads the masks from the saved activations.  The same value in all four calls of a step.
 *   Which launches are chained (consecutive GEMMs in one) and which weights the backward reads transposed is decided by
 *   shape alone: widths <= 256 chain, weights with >= 128 columns are transposed once per backward call; the backward of a
 *   4 -> 256 first layer goes through gts_sage_first_layer_bwd_f32, that of a 256 -> 4 top layer with one-byte winners
 *   through gts_spmm_max_bwd_lowrank_f32 (same bits as the calls they stand for).
 * Forward: everything it produces lives in `arena` (>= gts_sage_pool_stack_fwd_arena(...) bytes, which also reports the
 * byte offsets: offsets[4 i .. 4 i + 3] = max-pooled features m_i [n, w_i], winners arg_i [n, w_i] (arg_bytes each; -1
 * when not training), output out_i [n, w_{i+1}] (the next layer's input; the last one holds the logits), ReLU bits of out_i
 * (-1 when absent); offsets[4 L], [4 L + 1] = two scratch buffers).  training = 0: no winners, no bits.
 * Backward: `fwd_arena` is the arena of a training forward with the same arguments; grads[5 i .. 5 i + 4] receive the
 * gradients of params[5 i .. 5 i + 4] (any caller-chosen destinations, e.g. slices of one flat buffer); gx [n, w_0]
 * optional; scratch >= gts_sage_pool_stack_bwd_scratch(...) bytes. */
int64_t gts_sage_pool_stack_fwd_arena(int64_t n_rows, const int64_t* widths, int32_t n_layers, int32_t training,
                                      int32_t arg_bytes, int32_t relu_bits, int64_t* offsets);
int32_t gts_sage_pool_stack_fwd_f32(const int32_t* indptr, const int32_t* indices, const int32_t* sched_rec,
                                    int64_t sched_clusters, int32_t sched_rows, int32_t sched_srcs,
                                    int32_t sched_loc_words, const float* x, const float* const* params,
                                    int64_t n_rows, const int64_t* widths, int32_t n_layers, int32_t training,
                                    int32_t arg_bytes, int32_t relu_bits, void* arena, int64_t arena_bytes, void* stream);
int64_t gts_sage_pool_stack_bwd_scratch(int64_t n_rows, const int64_t* widths, int32_t n_layers, int32_t relu_bits);
int32_t gts_sage_pool_stack_bwd_f32(const int32_t* t_indptr, const int32_t* t_indices, const int32_t* t_slot,
                                    const int32_t* sched_rec, int64_t sched_clusters, int32_t sched_rows,
                                    int32_t sched_srcs, int32_t sched_loc_words, const float* gout, const float* x,
                                    const float* const* params, int64_t n_rows, const int64_t* widths,
                                    int32_t n_layers, int32_t arg_bytes, int32_t relu_bits, const void* fwd_arena,
                                    float* const* grads, float* gx, void* scratch, int64_t scratch_bytes,
                                    void* stream);
/* The training step's forward with the turn to the backward folded in, for a stack whose top layer is 256 -> 4 (any other
 * is GTS_ERR_SHAPE): gts_sage_pool_stack_fwd_f32 with training = 1, except that the last layer's classifier launch is
 * gts_sage_top_layer_train_f32, which also leaves out3, g_top [n, 4] (the gradient w.r.t. the logits, see `normalise` there)
 * and the gradients of the top layer's fc_self.weight, fc_neigh.weight and bias in grads[5 (L - 1) + 2 .. + 4] (the other
 * entries of `grads` are not touched).  top_workspace >= gts_sage_top_layer_train_workspace(n_rows, 256, 4) bytes.
 * gts_sage_pool_stack_bwd_top_f32 is gts_sage_pool_stack_bwd_f32 with gout = g_top; with top_done = 1 it leaves those three
 * gradients as they are (top_done = 0: the same call as gts_sage_pool_stack_bwd_f32).  Same bits as the calls they stand for. */
int32_t gts_sage_pool_stack_train_fwd_f32(const int32_t* indptr, const int32_t* indices, const int32_t* sched_rec,
                                          int64_t sched_clusters, int32_t sched_rows, int32_t sched_srcs,
                                          int32_t sched_loc_words, const float* x, const float* const* params,
                                          int64_t n_rows, const int64_t* widths, int32_t n_layers, int32_t arg_bytes,
                                          int32_t relu_bits, void* arena, int64_t arena_bytes, const int64_t* labels,
                                          const float* class_w, int32_t normalise, float* g_top, float* const* grads,
                                          float* out3, float* top_workspace, int64_t top_workspace_bytes, void* stream);
int32_t gts_sage_pool_stack_bwd_top_f32(const int32_t* t_indptr, const int32_t* t_indices, const int32_t* t_slot,
                                        const int32_t* sched_rec, int64_t sched_clusters, int32_t sched_rows,
                                        int32_t sched_srcs, int32_t sched_loc_words, const float* gout, const float* x,
                                        const float* const* params, int64_t n_rows, const int64_t* widths,
                                        int32_t n_layers, int32_t arg_bytes, int32_t relu_bits, const void* fwd_arena,
                                        float* const* grads, float* gx, void* scratch, int64_t scratch_bytes,
                                        int32_t top_done, void* stream);

/* ---- class-weighted cross-entropy ----------------------------------------------------------
 * Replaces torch.nn.CrossEntropyLoss(weight=class_weights)(logits, labels) of the reference
 * harness (model/gnn_model.py:30,42) and, through grad_unscaled, its backward.
 *   out3 = { num = sum_i w[y_i] nll_i,  den = sum_i w[y_i],  num / den }
 *   grad_unscaled[i,c] = w[y_i] (softmax(x_i)_c - [c == y_i])   (optional; d loss/dx = that / den)
 * logits [n, n_classes] fp32, labels int64 in [0, n_classes) (no ignore_index), class_w optional.
 * Deterministic two-level reduction through `workspace`
 * (>= gts_weighted_ce_workspace(n) bytes).  n_classes <= 32. */
int64_t gts_weighted_ce_workspace(int64_t n);
int32_t gts_weighted_ce_f32(const float* logits, const int64_t* labels, const float* class_w,
                            float* grad_unscaled, float* workspace, int64_t workspace_bytes,
                            float* out3, int64_t n, int64_t n_classes, void* stream);

/* ---- soft Dice over class regions + class-weighted cross-entropy ---------------
 * The voxel loss of the refinement CNN and of joint training; no counterpart in the reference, whose
 * loops train on torch.nn.CrossEntropyLoss alone (model/cnn_model.py).  Two passes:
 *   fwd (D1): one read of logits [n, n_classes] fp32 and labels int64 [n] -> `stats`;
 *   bwd (D2): a second read, with `stats` -> grad [n, n_classes] = grad_scale * dL/dlogits, written once.
 * A row is valid when 0 <= label < n_classes; a label of -100 contributes to no sum and gets a zero
 * gradient; any other label makes the loss NaN.  Over the valid rows, p = softmax(logits):
 *   q_ir = sum_{c in region r} p_ic    t_ir = [label_i in region r]
 *   I_r = sum_i q_ir t_ir   S_r = sum_i q_ir   T_r = sum_i t_ir
 *   dice_r = (2 I_r + smooth) / (S_r + T_r + smooth)     L_dice = 1 - mean_r dice_r
 *   CE = sum_i w[y_i] nll_i / sum_i w[y_i]               loss = ce_weight CE + dice_weight L_dice
 * A term whose weight is 0 is skipped (its part reads 0), so ce_weight = 0 gives a finite loss when no
 * row is valid.  group_masks: HOST pointer to n_groups bitmasks over the classes (bit c = class c),
 * read during the call.  class_w [n_classes] optional (NULL = ones).  grad_scale: optional DEVICE
 * scalar (the upstream gradient; NULL = 1).  The same regions, weights and smooth go to both calls.
 * logits and grad need only float alignment: at n_classes = 4 a 16-byte aligned base takes the form that
 * moves a row as one 16-byte access, any other base the float-by-float form (same definition).
 * Deterministic: fixed-association sums through `workspace` (>= gts_dice_ce_workspace bytes), the last
 * level in float64; no atomics.
 * Errors, before any launch: NULL pointer -> GTS_ERR_NULL; n <= 0, n_classes outside [1, 32],
 * n_groups outside [1, 8], short workspace -> GTS_ERR_SHAPE; an empty mask, a mask bit >= n_classes,
 * a negative or non-finite weight, smooth <= 0 or non-finite -> GTS_ERR_ARGKIND.
 * stats: GTS_DICE_CE_STATS_FLOATS floats, entries not named below are 0:
 *   [0] loss  [1] CE  [2] L_dice  [3] CE numerator  [4] CE denominator
 *   [8 + r] dice_r   [16 + r] I_r   [24 + r] S_r   [32 + r] T_r      (r < n_groups) */
#define GTS_DICE_CE_MAX_GROUPS 8
#define GTS_DICE_CE_STATS_FLOATS 40
#define GTS_DICE_CE_STATS_LOSS 0
#define GTS_DICE_CE_STATS_CE 1
#define GTS_DICE_CE_STATS_LDICE 2
#define GTS_DICE_CE_STATS_CE_NUM 3
#define GTS_DICE_CE_STATS_CE_DEN 4
#define GTS_DICE_CE_STATS_DICE 8
#define GTS_DICE_CE_STATS_I 16
#define GTS_DICE_CE_STATS_S 24
#define GTS_DICE_CE_STATS_T 32
int64_t gts_dice_ce_workspace(int64_t n, int32_t n_groups);
int32_t gts_dice_ce_fwd_f32(const float* logits, const int64_t* labels, const float* class_w,
                            const uint32_t* group_masks, int32_t n_groups, double ce_weight,
                            double dice_weight, double smooth, float* stats, void* workspace,
                            int64_t workspace_bytes, int64_t n, int64_t n_classes, void* stream);
int32_t gts_dice_ce_bwd_f32(const float* logits, const int64_t* labels, const float* class_w,
                            const uint32_t* group_masks, int32_t n_groups, double ce_weight,
                            double dice_weight, double smooth, const float* stats,
                            const float* grad_scale, float* grad, int64_t n, int64_t n_classes,
                            void* stream);

/* ---- training-time augmentation -------------------------------------------------
 * No counterpart in the reference, whose loops show every sample the same way in every epoch.  Both
 * kernels write fresh outputs (never in place) with plain 16-byte stores; no atomics, no workspace.
 *
 * gts_augment_crop_f32 (A1): x [cx, cy, cz, channels] fp32 channels-last and labels int64 [cx*cy*cz],
 * either of which may be NULL (with its output).  flip_mask bit 0 / 1 / 2 mirrors axis x / y / z:
 *   x_out[i, j, k, c] = x[i', j', k', c] * a_c + b_c + s_c * n(v, c)   for c < image_channels
 *                     = x[i', j', k', c]                               for c >= image_channels
 *   labels_out[v]     = labels[v']
 * with i' = cx - 1 - i on a mirrored axis and v the C-order index of the OUTPUT voxel.  params: DEVICE
 * [image_channels][3] = (a_c, b_c, s_c), may be NULL when image_channels == 0 (the plain mirror, which is
 * its own inverse and its own adjoint).  The affine is a float32 multiply, then a float32 add (no fma).  A
 * channel with a == 1 and b == 0 is copied, a channel with s == 0 draws nothing: the identity returns its
 * input bit for bit.  channels % 4 == 0 with 16-byte aligned bases moves 16 bytes per access, anything
 * else float by float (same values).
 *
 * gts_augment_features_f32 (A2): feats [n_rows, n_feats] fp32 node features of a batch of n_graphs graphs;
 * row_ptr (DEVICE) and row_ptr_host (HOST, read during the call) both hold the n_graphs + 1 row offsets,
 * ascending from 0 to n_rows (graphs without rows are legal); params: DEVICE [n_graphs][modalities][2] =
 * (a, b), n_feats % modalities == 0, feature f belongs to modality f / (n_feats / modalities) (the
 * quantile columns of mri2graph/graphgen.py:23-25, 45-52):
 *   out[r, f] = feats[r, f] * a_{g(r), m(f)} + b_{g(r), m(f)} + sigma * n(r, f)
 * Same copy / no-draw rule as A1.  n_rows == 0 returns GTS_OK without touching the device.
 *
 * n(idx, c): Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter
 * (idx & 0xffffffff, idx >> 32 | (c / 4) << 24 | stream << 31, step & 0xffffffff, step >> 32), stream 0
 * with idx = v for A1 and stream 1 with idx = r for A2.  From the four output words, channel c takes normal
 * c % 4: normals 0, 1 from words (0, 1), normals 2, 3 from words (2, 3), by Box-Muller in float32 with the
 * accurate logf / sinf / cosf: u = ((w_even >> 8) + 1) 2^-24, t = 2 pi (w_odd >> 8) 2^-24,
 * r = sqrt(-2 ln u), normals r cos t and r sin t.  Independent of the launch geometry.
 * Errors, before any launch: a missing pointer -> GTS_ERR_NULL; a negative extent, channels or n_feats
 * outside [1, 512], image_channels > channels, n_feats % modalities != 0, 2^56 or more voxels / rows,
 * row_ptr_host not ascending from 0 to n_rows -> GTS_ERR_SHAPE; flip_mask outside 0..7, a negative or
 * non-finite sigma -> GTS_ERR_ARGKIND. */
int32_t gts_augment_crop_f32(const float* x, const int64_t* labels, const float* params, float* x_out,
                             int64_t* labels_out, int64_t cx, int64_t cy, int64_t cz, int64_t channels,
                             int64_t image_channels, int32_t flip_mask, uint64_t seed, uint64_t step,
                             void* stream);
int32_t gts_augment_features_f32(const float* feats, const int64_t* row_ptr, const int64_t* row_ptr_host,
                                 const float* params, float* out, int64_t n_rows, int64_t n_feats,
                                 int64_t modalities, int64_t n_graphs, double sigma, uint64_t seed,
                                 uint64_t step, void* stream);

/* ---- rotated and zoomed crops ----------------------------------------------------
 * No counterpart in the reference either.  gts_augment_spatial_f32 (A3) is A1 with a rotation and an
 * isotropic zoom between the mirror and the affine; gts_augment_spatial_bwd_f32 (A4) is the adjoint of its
 * resample and mirror.  Fresh outputs, no atomics, no workspace.  matrix: HOST, 9 doubles M[3][3] row-major,
 * read during the call.
 *
 * Definition.  Crop extents n = (cx, cy, cz), centre c_a = (n_a - 1) / 2.  Output voxel o has mirrored index
 * o', with o'_a = n_a - 1 - o_a on the axes of flip_mask; d = o' - c is exact.  All coordinate work is float64
 * with no fma:
 *   p_a = c_a + ((M[a][0] d_0 + M[a][1] d_1) + M[a][2] d_2)
 *   f_a = floor(p_a), t_a = p_a - f_a, with p_a clamped into [-2, n_a + 1] before any integer conversion.
 * Float channels: the eight corners are (f_a | f_a + 1); a corner with any index outside [0, n_a - 1] reads
 * 0.0 (a zero border, no clamping to the edge); lerp along x, then y, then z, each a + (b - a) t in float64;
 * round once to float32; then A1's per-modality affine (float32 multiply then add, copied when a == 1 and
 * b == 0) and A1's noise s_c n(v, c), v the C-order index of the OUTPUT voxel, Philox stream 0, unchanged.
 * Channels >= image_channels are resampled only.
 * Labels: m_a = floor(p_a + 0.5); a label outside the crop on any axis becomes 0, else it is labels[m].
 * Adjoint (A4): the resample and the mirror only, no affine and no noise: dy, dx [cx, cy, cz, channels],
 *   dx[q, k] = float32( sum_o w(o, q) dy[o, k] ),  w = prod_a w_a,
 *   w_a = 1 - t_a if f_a == q_a, t_a if f_a + 1 == q_a, else 0,
 * w computed in float64 from the same p(o), the sum in float64 over the contributing o in ascending C-order
 * of o'.  Two runs are bit-equal.  The candidates of q are the integer o' of the box
 * c + M^-1 (q - c) +- h, h_a = sum_b |M^-1[a][b]|, widened by one on each side and clipped to the crop (M^-1
 * is formed here in float64); every candidate recomputes p(o') with the expression above.
 * Either of x / labels may be NULL (with its output), as for A1; params as for A1.
 * Errors, before any launch: a missing pointer -> GTS_ERR_NULL; extents and channels as A1 ->
 * GTS_ERR_SHAPE; flip_mask outside 0..7, a non-finite matrix entry, a singular matrix (zero or non-finite
 * determinant or inverse) or any h_a > 8 -> GTS_ERR_ARGKIND.  A crop without voxels returns GTS_OK untouched. */
int32_t gts_augment_spatial_f32(const float* x, const int64_t* labels, const float* params,
                                const double* matrix, float* x_out, int64_t* labels_out, int64_t cx,
                                int64_t cy, int64_t cz, int64_t channels, int64_t image_channels,
                                int32_t flip_mask, uint64_t seed, uint64_t step, void* stream);
int32_t gts_augment_spatial_bwd_f32(const float* dy, const double* matrix, float* dx, int64_t cx, int64_t cy,
                                    int64_t cz, int64_t channels, int32_t flip_mask, void* stream);

/* ---- tuning knobs-----------------------------------------------------------------------
 * Process-wide tile selection of the K11 kernels (defaults are the tuned values; used by
 * tools/tune_gemm.py).  Returns GTS_ERR_ARGKIND for an unknown option. */
#define GTS_OPT_GEMM_TILE 1  /* forward tile: -1 automatic, -2 automatic among the 32x32x2 tiles only (a row's result then does
                                not depend on how many rows the call has: batched == per-sample, bit for bit), 1 = 128x256, 3 = 64x256, 5 = 256x128, 8 = 256x256 double-buffered, 10 = 240 / 192 / 144-row panels (16x16x4 MFMA) with direct-to-fragment buffer loads (12 waves).  Other values: GTS_ERR_ARGKIND (the forms measured and rejected — panels staged through LDS, four waves of 240x64 — are built from tools/diag/, not shipped) */
#define GTS_OPT_WGRAD_TILE 2 /* weight-gradient tile: -1 automatic, 1 = 128x128, 2 = 128x256, 4 = 256x256 double-buffered through registers and LDS,
                                6 = the same tile moved by LDS-DMA with a main loop of MFMAs and LDS reads only (immediate-offset fragment
                                    reads, scalar-built DMA descriptors, bias sums in one wave per SIMD): the automatic choice where 4 was
                                    (same bits as 4).  Other values: GTS_ERR_ARGKIND (rejected tiles: tools/diag/gemm_rejected_forms.inc) */
#define GTS_OPT_IGRAD_TILE 3 /* input-gradient tile: same numbering as the forward one (default 1) */
#define GTS_OPT_PROJECT_STREAMING 6  /* K12: non-temporal stores of the projected rows (default 1) */
#define GTS_OPT_SPMM_ROWS_PER_WAVE 4 /* K1-K4: rows one wave walks (0 = automatic) */
#define GTS_OPT_SPMM_STREAMING 5     /* K1/K2: bit 0 = non-temporal stores of write-once rows, bit 1 = non-temporal
                                        loads of read-once rows (K2's relu_src); -1 = per-kernel default */
#define GTS_OPT_GEMM_SCHED 7  /* K11 scheduling bits (default 1): 1 = s_setprio by progress inside a reduction tile (LDS kernels),
                                2 = non-temporal stores of the output panel (direct-to-fragment kernels; no gain measured),
                                4 = the direct-to-fragment kernels keep every epilogue switch a run-time argument (the generic
                                    instantiation) instead of the compile-time epilogues of the layer-stack launches (A/B runs),
                                8 = the chained 240-row launches of the layer stack issue the nine fragment loads of a reduction
                                    group in one burst (rounds 1 - 2) instead of one load per eight MFMAs (A/B runs; same bits) */
#define GTS_OPT_CLUSTER_STREAMING 8 /* clustered K1 / K2: bit 0 = non-temporal stores of out / gx; -1 = per-kernel default */
#define GTS_OPT_GAT_WALK 14          /* K5-K8: 1 = walk the (node, head) rows head-major (default), 0 = node-major */
#define GTS_OPT_GAT_CLUSTER_WAVES 15 /* clustered GAT aggregation: waves per persistent workgroup (0 = default 12; up to 16) */
#define GTS_OPT_GAT_CLUSTER_GROUP 16 /* clustered GAT aggregation UNDER STATIC DEALING (option 17 = 1): clusters of an XCD's span walked together through
                                        all their (head, half) slices (0 = 16; 100000 = the whole span).  Dealt units walk the whole span slice by slice */
#define GTS_OPT_GAT_CLUSTER_DEALING 17 /* clustered GAT aggregation: 0 = the workgroups of an XCD take their units off one counter (default: the units in
                                         flight stay neighbours in the walk whatever each workgroup's pace), 1 = static round-robin (A/B runs) */
#define GTS_OPT_CLUSTER_DEALING 18  /* clustered K1 / K2, where the caller gives counters: 0 = automatic (units dealt off the XCD's counter from 16 units per
                                       workgroup on, static round-robin below), 1 = always dealt, 2 = always static */
#define GTS_OPT_PANEL_ROWS 13        /* K11 direct-to-fragment panels: rows per panel, 0 = automatic among 240 / 192 / 144 */
#define GTS_OPT_CLUSTER_RING 10      /* clustered K1 / K2: units the gathers run ahead of the reduction (0 = automatic: 1; 2 where the LDS holds it) */
#define GTS_OPT_CLUSTER_PER_CU 11    /* clustered K1 / K2: persistent workgroups per CU (0 = automatic: 2, or 3 for short backward launches) */
#define GTS_OPT_CLUSTER_CONSUMERS 12 /* clustered K1 / K2: waves per workgroup (0 = automatic: 16 forward, 12 backward) */
int32_t gts_set_option(int32_t option, int32_t value);
/* Current value of a knob (INT32_MIN for an unknown option): callers that change one temporarily put it back. */
int32_t gts_get_option(int32_t option);

/* ---- K9h: batch collate on the host, straight into the upload layout ---------------------------------
 * HOST functions (host pointers, no GPU call, no allocation, no state; safe to call from any thread — a
 * ctypes caller holds no interpreter lock while they run).
 * Replace, for the training loader's hot path, what the reference does per step in
 * data_processing/data_loader.py:165-169 (`minibatch_graphs`: dgl.batch + np.concatenate of the
 * members' features and labels + FloatTensor / LongTensor conversions) and model/gnn_model.py:37-40
 * (`.to(device)` of graph, features, labels): the members' cached host arrays are written ONCE, already
 * shifted / converted, into one caller-owned (page-locked) block laid out exactly as the device will
 * read it, so that a batch reaches the GPU in ONE asynchronous copy:
 *
 *   features fp32 [N, feat_width] | labels int64 [N] |
 *   indptr [N+1] | indices [E] | t_indptr [N+1] | t_indices [E] | t_slot [E] | t_pos [E] |
 *   max(in-degree, 1) fp32 [N] | in-degree + 1 fp32 [N] |
 *   cluster-schedule records of kind 0 | kind 1 | ...        (every segment 256-byte aligned)
 *
 * Block-diagonal union as dgl.batch defines it: node ids of member j shifted by sum_{i<j} N_i, edges
 * (and CSR positions) by sum_{i<j} E_i, members in order; fp64 features are rounded to fp32 as
 * torch.FloatTensor(np.concatenate(features)) rounds them; labels widen to int64.  Schedule records
 * (gts_cluster_schedule) are concatenated member by member with their row / neighbour ids shifted and
 * their per-edge sections re-packed to the widest member's loc_words.  The bytes equal what the Python
 * path (gts.batch + ClusterSchedule.concat, the tested reference) produces: tests/test_collate_host.py.
 *
 * gts_collate_plan fills `plan` (sizes and byte offsets) for `members`; gts_collate_batch writes the block
 * (`dst_bytes` >= plan.total_bytes) using up to `n_threads` threads of its own (<= 1: the calling thread only).
 * A schedule kind that some member lacks (sched_rec NULL) is dropped for the whole batch (plan.sched_clusters
 * = -1).  Returns GTS_OK, GTS_ERR_NULL, GTS_ERR_SHAPE (sizes beyond int32, dst too small, members whose
 * records do not match the kind's limits) or GTS_ERR_ARGKIND (feature / label element kinds). */
#define GTS_COLLATE_MAX_SCHEDULES 6
typedef struct {
  int64_t n_nodes, n_edges;
  const int32_t *indptr, *indices, *t_indptr, *t_indices, *t_slot, *t_pos;
  const void* features;     /* [n_nodes, feat_width] row-major */
  const void* labels;       /* [n_nodes], or NULL when the batch carries none */
  int32_t feat_bytes;       /* 4 = fp32, 8 = fp64 */
  int32_t label_bytes;      /* 8 = int64, 4 = int32 (0 with labels == NULL) */
  const int32_t* sched_rec[GTS_COLLATE_MAX_SCHEDULES];   /* [clusters, record words] per kind, or NULL */
  int64_t sched_clusters[GTS_COLLATE_MAX_SCHEDULES];
  int32_t sched_loc_words[GTS_COLLATE_MAX_SCHEDULES];
} gts_collate_member_t;
typedef struct {
  int32_t max_rows, max_srcs, tagged, reserved;          /* the limits the kind's records were built with */
} gts_collate_kind_t;
typedef struct {
  int64_t total_bytes, n_nodes, n_edges;
  int64_t features, labels;                              /* byte offsets; labels = -1 when absent */
  int64_t csr[8];                                        /* indptr, indices, t_indptr, t_indices, t_slot, t_pos, deg_clamped, deg_plus1 */
  int64_t sched[GTS_COLLATE_MAX_SCHEDULES];              /* byte offset of each kind's records (-1: dropped) */
  int64_t sched_clusters[GTS_COLLATE_MAX_SCHEDULES];     /* clusters of the union (-1: dropped) */
  int32_t sched_loc_words[GTS_COLLATE_MAX_SCHEDULES];    /* loc_words of the union's records */
  int32_t sched_record_words[GTS_COLLATE_MAX_SCHEDULES];
} gts_collate_plan_t;
int32_t gts_collate_plan(const gts_collate_member_t* members, int32_t n_members, int64_t feat_width,
                         const gts_collate_kind_t* kinds, int32_t n_kinds, gts_collate_plan_t* plan);
int32_t gts_collate_batch(const gts_collate_member_t* members, int32_t n_members, int64_t feat_width,
                          const gts_collate_kind_t* kinds, int32_t n_kinds, void* dst, int64_t dst_bytes,
                          int32_t n_threads, gts_collate_plan_t* plan);

/* ---- G1-G8: supervoxel graph construction (reference mri2graph/graphgen.py) -----------------
 * The SLIC of skimage <= 0.18 (mri2graph/graphgen.py:243) and the statistics / discard / edge
 * builders around it, restated in DESIGN.md "Graph generation".  Volumes are [D, H, W, C]
 * row-major (C fastest), int32 voxel indexing (D*H*W*C < 2^31).  Supervoxel counts are at
 * most GTS_GG_MAX_SV (the partition is int16, as in the reference), k at most GTS_GG_MAX_K. */
#define GTS_GG_MAX_SV 32767
#define GTS_GG_MAX_K 32
#define GTS_GG_MAX_RADIUS 16
/* G1: scipy.ndimage.gaussian_filter(image, sigma=[s, s, s, 0]) (skimage slic's smoothing before
 * mri2graph/graphgen.py:243), mode 'reflect', then out *= scale (slic's 1 / compactness).
 * weights[0..radius]: the normalised taps, weights[j] = w(+-j).  tmp: scratch of the image's size.
 * Bit-exact against scipy: centre tap first, then (v[i-j] + v[i+j]) * w[j] for j = radius .. 1. */
int32_t gts_gg_gaussian_f64(const double* in, double* out, double* tmp, const double* weights, int32_t radius,
                            double scale, int64_t d, int64_t h, int64_t w, int64_t c, void* stream);
/* G2: one SLIC assignment round (mri2graph/graphgen.py:243, skimage _slic_cython's assignment loop).
 * centres [n_centres, 3 + c] = (z, y, x, colour...); a NaN centre (emptied segment) is skipped.
 * Every voxel takes the centre of least distance among the windows that contain it (lowest index
 * on ties); a voxel in no window keeps labels[v].  c <= 8.  best (uint64 [D*H*W]) and winner
 * (uint32 [D*H*W]) are scratch. */
int32_t gts_gg_slic_assign_f64(const double* img, const double* centres, int32_t n_centres, int64_t d, int64_t h,
                               int64_t w, int64_t c, int32_t step_z, int32_t step_y, int32_t step_x,
                               double spatial_weight, int32_t* labels, uint64_t* best, uint32_t* winner,
                               void* stream);
/* G3: SLIC centre update (same call site): centre = raster-order sums of (z, y, x, colour...) over
 * the segment's voxels / count (0 voxels -> NaN).  bbox: int32 scratch [n_centres * 6]. */
int32_t gts_gg_slic_update_f64(const double* img, const int32_t* labels, double* centres, int32_t n_centres,
                               int64_t d, int64_t h, int64_t w, int64_t c, int32_t* bbox, void* stream);
/* G4 (HOST function: host pointers, no GPU call): skimage's _enforce_label_connectivity_cython
 * (mri2graph/graphgen.py:243, enforce_connectivity=True): raster-order BFS over 6-neighbours
 * (+x, -x, +y, -y, +z, -z), truncated at max_size voxels; components below min_size take the
 * last adjacent relabelled neighbour (0 when none).  queue: int64 scratch [max_size].
 * n_labels = max label + 1. */
int32_t gts_gg_enforce_connectivity(const int32_t* labels, int32_t* out, int64_t d, int64_t h, int64_t w,
                                    int64_t min_size, int64_t max_size, int64_t* queue, int32_t* n_labels);
/* G5: extract_supervoxel_statistics (mri2graph/graphgen.py:47-61): per supervoxel and channel the
 * quantiles 0.1, 0.25, 0.5, 0.75, 0.9 of the float32 intensities (numpy 'linear'), fp64,
 * feats [n_sv, 5 * c] channel-major; the mode of vox_labels (NULL -> zeros; smallest value among
 * ties) and the centroid (mean of integer coordinates).  partition: int32 ids in [0, n_sv).
 * scratch: gts_gg_sv_stats_workspace(d * h * w, n_sv) bytes.  5 * c <= 256. */
int64_t gts_gg_sv_stats_workspace(int64_t n_vox, int32_t n_sv);
int32_t gts_gg_sv_stats(const int32_t* partition, const float* intensities, const int16_t* vox_labels, int64_t d,
                        int64_t h, int64_t w, int64_t c, int32_t n_sv, double* feats, double* centroids,
                        int32_t* sv_labels, void* scratch, void* stream);
/* G6: discard_empty_svs (mri2graph/graphgen.py:71-96): supervoxels whose feats[:, 4] is below
 * min(feats[:, 4]) + 0.01 are dropped, the kept ones numbered in order (remap, -1 = dropped) and
 * gathered into node_feats / node_centroids / node_labels; new_partition (int16) = remap[partition].
 * keep: int32 scratch [n_sv]; n_nodes: one device int32. */
int32_t gts_gg_discard_f64(const double* feats, const double* centroids, const int32_t* sv_labels, int32_t n_sv,
                           int32_t n_feat, const int32_t* partition, int64_t n_vox, int32_t* remap, int32_t* keep,
                           double* node_feats, double* node_centroids, int32_t* node_labels, int16_t* new_partition,
                           int32_t* n_nodes, void* stream);
/* G7: build_adjacency_matrix(..., weighted=False, enforce_regularity=True) (mri2graph/graphgen.py:120-153)
 * without the N x N matrices.  gts_gg_knn_candidates_f64: cand[i, 0..k) = the k nearest j > i by
 * (scipy cdist euclidean distance, j), -1 past the last one.  gts_gg_knn_greedy (HOST function):
 * the reference's sequential pass — row i takes the first k - (rows i' < i that took i) of its
 * candidates: picks[i, t] = j or -1; n_edges = undirected edges; got: int32 host scratch [n]. */
int32_t gts_gg_knn_candidates_f64(const double* positions, int32_t n, int32_t k, int32_t* cand, void* stream);
int32_t gts_gg_knn_greedy(const int32_t* cand, int32_t n, int32_t k, int32_t* picks, int32_t* got, int64_t* n_edges);
/* G8: find_adjacent_nodes (mri2graph/graphgen.py:161-196): pairs of distinct ids >= 0 that touch across
 * a face, both orientations, plus every (i, i).  gts_gg_touching_count_i16 marks them in scratch
 * (gts_gg_touching_workspace(n) bytes) and writes indptr [n + 1]; gts_gg_touching_emit then writes
 * the columns of each row in ascending order (the row-major order of np.where on the matrix). */
int64_t gts_gg_touching_workspace(int32_t n);
int32_t gts_gg_touching_count_i16(const int16_t* partition, int64_t d, int64_t h, int64_t w, int32_t n, void* scratch,
                                  int32_t* indptr, void* stream);
int32_t gts_gg_touching_emit(const void* scratch, int32_t n, const int32_t* indptr, int32_t* cols, void* stream);

/* ---- C1-C5: 5x5x5 Conv3d, stride 1, replicate padding 2 (refinement CNN training) ----------------
 * The two layers of CnnRefinementNet (model/networks.py:83-93) and their backward, as reached from
 * RefinementModel.run_epoch (model/cnn_model.py:36-56) and .evaluate (:58-78).  Activations are
 * channels-last [cx, cy, cz, C] (= [V, C]); w is torch's Conv3d weight [cout, cin, 5, 5, 5]; channel
 * counts 1..32; every dimension >= 1 and (cx + 4)(cy + 4)(cz + 4) * 32 < 2^31.  Each call first packs
 * w into its workspace.  Deterministic: no float atomics, fixed reduction orders.
 * gts_conv3d_fwd_f32 (C1 / C2): y = act(conv(x, w) + bias); bias may be NULL; relu 0 or 1. */
int64_t gts_conv3d_fwd_workspace(int32_t cin, int32_t cout);
int32_t gts_conv3d_fwd_f32(const float* x, const float* w, const float* bias, float* y, int64_t cx, int64_t cy,
                           int64_t cz, int32_t cin, int32_t cout, int32_t relu, void* workspace,
                           int64_t workspace_bytes, void* stream);
/* C3: dx = d conv(x, w) / d x applied to dy [V, cout] -> [V, cin], the exact adjoint of the replicate
 * clamp (every tap that clamps onto a boundary voxel contributes to it).  h (optional, [V, cin]): the
 * ReLU output that fed the layer; dx is zeroed where h <= 0. */
int64_t gts_conv3d_bwd_data_workspace(int64_t cx, int64_t cy, int64_t cz, int32_t cin, int32_t cout);
int32_t gts_conv3d_bwd_data_f32(const float* dy, const float* w, const float* h, float* dx, int64_t cx, int64_t cy,
                                int64_t cz, int32_t cin, int32_t cout, void* workspace, int64_t workspace_bytes,
                                void* stream);
/* C4 / C5: dw [cout, cin, 5, 5, 5] = sum over voxels of dy (x) the clamped input taps; db [cout] (optional)
 * = sum over voxels of dy.  Split-K over voxel bricks into the workspace, summed in a fixed order. */
int64_t gts_conv3d_bwd_weight_workspace(int64_t cx, int64_t cy, int64_t cz, int32_t cin, int32_t cout);
int32_t gts_conv3d_bwd_weight_f32(const float* x, const float* dy, float* dw, float* db, int64_t cx, int64_t cy,
                                  int64_t cz, int32_t cin, int32_t cout, void* workspace, int64_t workspace_bytes,
                                  void* stream);

/* ---- H1-H5: BraTS HD95 order statistics ------------------------------------------------------------
 * Replace the scipy / numpy arithmetic of model/evaluation.py:83-96 (calculate_hd95_from_logical_array) and
 * :112-189 (medpy's hd95 and __surface_distances: binary_erosion, distance_transform_edt, np.percentile), reached
 * from GNN.evaluate (model/gnn_model.py:76-87) and RefinementModel.evaluate.
 * pred, truth: int16 label volumes [X, Y, Z], Z contiguous.  Regions WT (v != 0), CT (v in {2, 3}), ET (v == 3).
 * Border B(r, side): region voxels with a 6-neighbour inside the volume outside the region, or on a face of an
 * axis longer than 1; all_border = 1 (scipy's erosion of an array with a unit axis) makes every region voxel
 * border, and so does a 1x1x1 volume.  out (device int64 [3][4], one row per region): n = |B(r, pred)| +
 * |B(r, truth)|; the squared distances at ranks lo and hi of the sorted multiset { d2(p, B(r, truth)) : p in
 * B(r, pred) } + { d2(q, B(r, pred)) : q in B(r, truth) }, where v = (n - 1) * 0.95, lo = floor(v), hi = lo + 1,
 * or lo = hi = n - 1 when v >= n - 1 (np.percentile's linear method); presence bits (1: the region is in
 * pred, 2: in truth).  Ranks are only selected when both bits are set; otherwise both entries are 0.
 * Limits: every extent >= 1, X * Y * Z < 2^31 and (X-1)^2 + (Y-1)^2 + (Z-1)^2 <= 2^24 (the histogram of
 * squared distances has one bin per value), else GTS_ERR_SHAPE; all_border outside {0, 1}: GTS_ERR_ARGKIND.
 * workspace: gts_hd95_workspace(X, Y, Z) bytes (0 for a rejected shape).  Integer arithmetic throughout:
 * identical results on every run. */
int64_t gts_hd95_workspace(int64_t X, int64_t Y, int64_t Z);
int32_t gts_hd95_order_stats_i16(const int16_t* pred, const int16_t* truth, int64_t X, int64_t Y, int64_t Z,
                                 int32_t all_border, int64_t* out, void* workspace, int64_t workspace_bytes,
                                 void* stream);

/* ---- H3w-H5w: surface distances under a voxel spacing (HD95 in millimetres, surface Dice) -------------
 * What medpy's hd95(voxelspacing=...) and the surface-Dice scripts of the BraTS tasks compute on the host with
 * distance_transform_edt(sampling=...), for the borders H1 defines (model/evaluation.py:112-189 with a spacing).
 * units (HOST int64 [3], read at launch): the voxel spacing along X, Y, Z as positive integers u_a <= 10^6 with
 * no common factor needed (gts.metrics.spacing_units: 1e-4 mm steps divided by a common divisor).  The device quantity
 * is D2(p) = min over border voxels q of the other side of sum_a u_a^2 (p_a - q_a)^2, an exact int64; a distance
 * is sqrt(double(D2)) times the caller's scale.  thresholds (HOST int64 [n_thresholds], 0 <= n_thresholds <= 4;
 * may be NULL when n_thresholds is 0): squared tolerances T_k >= 0 in the same integer units.
 * out (device int64 [3][12], one row per region): n, D2 at ranks lo and hi, presence bits, all four as in
 * gts_hd95_order_stats_i16 (with units {1, 1, 1} the same integers), then within[side][k] for side pred, truth
 * and k < 4: the number of border voxels of that side with D2 <= T_k (0 for k >= n_thresholds, and for a region
 * absent from either side).
 * Arithmetic is int64; with B = sum_a u_a^2 (N_a - 1)^2 a volume is accepted when every extent is in [1, 4097],
 * X * Y * Z < 2^31 and B * max(N_a) < 2^62 (the envelope's cross-multiplied comparison then cannot overflow),
 * else GTS_ERR_SHAPE; 240 x 240 x 155 passes at any spacing up to 10 mm.  A unit outside [1, 10^6], a negative
 * threshold, n_thresholds outside 0..4 or all_border outside {0, 1}: GTS_ERR_ARGKIND.  Every argument is checked
 * before anything is launched.  workspace: gts_surface_workspace(X, Y, Z, units) bytes (0 for a rejected shape
 * or unit).  Integer arithmetic and integer atomics throughout: identical results on every run. */
int64_t gts_surface_workspace(int64_t X, int64_t Y, int64_t Z, const int64_t* units);
int32_t gts_surface_stats_i16(const int16_t* pred, const int16_t* truth, int64_t X, int64_t Y, int64_t Z,
                              int32_t all_border, const int64_t* units, const int64_t* thresholds,
                              int32_t n_thresholds, int64_t* out, void* workspace, int64_t workspace_bytes,
                              void* stream);

/* ---- C1-C5: 3-D connected components and the small-island clean-up of a prediction ------------------
 * The post-processing step a user otherwise runs on the host with scipy.ndimage.label + np.bincount.
 * labels: int16 volume [X, Y, Z], Z contiguous; foreground is labels != 0, whatever the values.  connectivity
 * 6 or 26 (scipy's generate_binary_structure(3, 1) / (3, 3)); an axis of extent 1 has no neighbours along it.
 * Limits: every extent >= 0 and X * Y * Z < 2^31; a negative extent, a larger volume, another connectivity or
 * a workspace below gts_components_workspace(X, Y, Z) bytes: GTS_ERR_SHAPE.  A volume of zero voxels returns
 * GTS_OK without touching memory (its workspace size is 0, as for a rejected volume).
 * gts_components_roots_i16: roots_out (int32 [X, Y, Z]) = 1 + the smallest linear index of the voxel's
 *   component, 0 for background.
 * gts_components_filter_i16: labels_out (may be labels_in) = labels_in with, in this order,
 *   (a) every foreground voxel of a component of fewer than min_voxels voxels set to 0 (min_voxels <= 1: none);
 *   (b) with n_et the number of voxels equal to et_label that survive (a): when 0 < n_et < et_min_voxels each
 *       of them set to et_replacement (et_min_voxels <= 0: rule off).
 *   stats (device int64 [4]) = {components found, components removed, voxels removed, ET voxels relabelled}.
 * Lock-free union-find with integer atomics (no workgroup waits for another); the root of a component is its
 * smallest index and every count is an integer sum: identical results on every run. */
int64_t gts_components_workspace(int64_t X, int64_t Y, int64_t Z);
int32_t gts_components_roots_i16(const int16_t* labels, int64_t X, int64_t Y, int64_t Z, int32_t connectivity,
                                 int32_t* roots_out, void* workspace, int64_t workspace_bytes, void* stream);
int32_t gts_components_filter_i16(const int16_t* labels_in, int64_t X, int64_t Y, int64_t Z, int32_t connectivity,
                                  int64_t min_voxels, int32_t et_label, int64_t et_min_voxels, int32_t et_replacement,
                                  int16_t* labels_out, int64_t* stats, void* workspace, int64_t workspace_bytes,
                                  void* stream);

/* ---- L1-L3: lesion-wise scoring of a prediction (BraTS 2023 lesion-wise Dice / HD95) ----------------------
 * The device half of gts/lesionwise.py: what a user otherwise does on the host with scipy's binary_dilation,
 * two ndimage.label calls and one np.isin per lesion.  Label volumes are int16 [X, Y, Z], Z contiguous, in the
 * internal coding; region 0 = WT (v != 0), 1 = CT (v in {2, 3}), 2 = ET (v == 3), as in H1; another region:
 * GTS_ERR_ARGKIND.  Limits: every extent >= 1 and X * Y * Z < 2^31, else GTS_ERR_SHAPE; a workspace below
 * gts_lesionwise_workspace(X, Y, Z) bytes (0 for a rejected shape): GTS_ERR_SHAPE.  Nothing is launched for a
 * rejected argument.  Roots are those of gts_components_roots_i16 at connectivity 26: 1 + the smallest linear
 * index of the voxel's component, 0 for background.
 * gts_lesionwise_dilate_i16 (L1): mask_out (int16 0 / 1) = scipy's binary_dilation(region mask,
 *   generate_binary_structure(3, 2), iterations = dilation, border_value = 0), in one pass by the footprint
 *   { o : max |o_i| <= n, sum |o_i| <= 2 n }, clipped at every face; dilation 0 is the region mask itself.
 *   dilation outside 0..3: GTS_ERR_ARGKIND.
 * gts_lesionwise_tables_i16 (L2): pred_roots = the roots of the prediction's region mask P, dilated_roots = the
 *   roots of L1's mask D of the truth.  tables_out (device int32, tables_ints >= gts_lesionwise_table_ints(X, Y, Z),
 *   else GTS_ERR_SHAPE) = { n_lesions, n_components, n_pairs, 0 }, then n_lesions rows of 9 (one per component of
 *   D: root, |G_k| with G_k the truth region voxels in it, |P n G_k|, box of G_k), n_components rows of 9 (one
 *   per component of P: root, size, 0, box), then n_pairs pairs (component root, lesion root) that cover every
 *   pair with a common voxel at least once.  A box is { x_end, X - x_begin, y_end, Y - y_begin, z_end,
 *   Z - z_begin } (ends exclusive; all 0 when empty).  Rows and pairs come in arrival order, which may differ
 *   between runs; as sets they are the same on every run.  No list can outgrow its buffer: each holds at most
 *   one entry per 2 x 2 x 2 cell of the volume.
 * gts_lesionwise_masks_i16 (L3): over the box { x_begin, x_end, y_begin, y_end, z_begin, z_end } (HOST int64
 *   [6], read at launch; inside the volume and not empty, else GTS_ERR_SHAPE), mask_m and mask_g (int16, C-order
 *   over the box) = 3 where pred_roots is one of matched_roots (device int32 [n_matched], ascending), resp.
 *   where the voxel is in the truth region and its dilated root is lesion_root; 0 elsewhere.  The pair H1 takes.
 * Integer arithmetic and integer atomics throughout: identical results on every run. */
int64_t gts_lesionwise_workspace(int64_t X, int64_t Y, int64_t Z);
int64_t gts_lesionwise_table_ints(int64_t X, int64_t Y, int64_t Z);
int32_t gts_lesionwise_dilate_i16(const int16_t* labels, int64_t X, int64_t Y, int64_t Z, int32_t region,
                                  int32_t dilation, int16_t* mask_out, void* workspace, int64_t workspace_bytes,
                                  void* stream);
int32_t gts_lesionwise_tables_i16(const int16_t* truth, const int32_t* pred_roots, const int32_t* dilated_roots,
                                  int64_t X, int64_t Y, int64_t Z, int32_t region, int32_t* tables_out,
                                  int64_t tables_ints, void* workspace, int64_t workspace_bytes, void* stream);
int32_t gts_lesionwise_masks_i16(const int16_t* truth, const int32_t* pred_roots, const int32_t* dilated_roots,
                                 int64_t X, int64_t Y, int64_t Z, int32_t region, int32_t lesion_root,
                                 const int32_t* matched_roots, int64_t n_matched, const int64_t* box, int16_t* mask_m,
                                 int16_t* mask_g, void* stream);

/* ---- I1-I3: intake of a raw four-modality scan --------------------------------------------------------
 * The host step of DataPreprocessor.load (scripts/preprocess_dataset.py) on the device:
 *   crop = determine_brain_crop(image); image = standardize_img(normalize_img(image[crop]), mean, std).
 * src: the four modality volumes as NIfTI stores them, [4][Z][Y][X] (x fastest), dtype given by its NIfTI
 * code: 4 (int16) or 16 (float32), else GTS_ERR_ARGKIND; values are taken as float32.  Every extent in
 * [1, 4096] and X * Y * Z < 2^31, else GTS_ERR_SHAPE.
 * gts_intake_occupancy (I1): flag_x[X], flag_y[Y], flag_z[Z] (int32) = 1 where the plane holds a voxel whose
 * np.amax over the channels is > 0.01 (a NaN in any channel: not counted), else 0; nonfinite (one uint64) = the
 * number of voxels with a non-finite value in some channel.  Buffers are cleared by the call.
 * Crops: xs[cx], ys[cy], zs[cz] are plane indices inside the volume (the nonzeros of I1's flags); the cropped
 * region is their outer product (np.ix_), x fastest, n = cx * cy * cz, 1 <= cx <= X, 1 <= cy <= Y, 1 <= cz <= Z.
 * gts_intake_order_stats (I2): out (device float32 [4][2]) = the values at ranks rank_lo and rank_hi
 * (0 <= rank_lo <= rank_hi < n) of each channel's cropped values in ascending order; -0.0 counts as +0.0
 * (and is returned as +0.0).  Radix select on the order-preserving key, exact; workspace:
 * gts_intake_select_workspace() bytes.
 * gts_intake_standardize (I3): out (device float32, C-order [cx][cy][cz][4]) = ((v / top_c) - mean_c) /
 * std_c in IEEE float32, params = HOST float32 [3][4] (top, mean, std), copied at launch. */
int32_t gts_intake_occupancy(const void* src, int32_t dtype, int64_t X, int64_t Y, int64_t Z, int32_t* flag_x,
                             int32_t* flag_y, int32_t* flag_z, uint64_t* nonfinite, void* stream);
int64_t gts_intake_select_workspace(void);
int32_t gts_intake_order_stats(const void* src, int32_t dtype, int64_t X, int64_t Y, int64_t Z, const int32_t* xs,
                               int64_t cx, const int32_t* ys, int64_t cy, const int32_t* zs, int64_t cz,
                               int64_t rank_lo, int64_t rank_hi, float* out, void* workspace, int64_t workspace_bytes,
                               void* stream);
int32_t gts_intake_standardize(const void* src, int32_t dtype, int64_t X, int64_t Y, int64_t Z, const int32_t* xs,
                               int64_t cx, const int32_t* ys, int64_t cy, const int32_t* zs, int64_t cz,
                               const float* params, float* out, void* stream);

/* ---- D1-D3: per-scan standardization statistics ---------------------------------------------------------
 * One scan's share of DataPreprocessor.compute_dataset_stats (scripts/preprocess_dataset.py:93-115), with the
 * normalization of normalize_img(..., is_flat=True) (data_processing/image_processing.py:45-51), on the device:
 *   healthy = (img[..., 0] > 0.001) & (lab == 0); y = img[healthy] / q995; mean(y, 0), std(y, 0).
 * src, dtype and the extent limits: as for I1-I3, the WHOLE volume (nothing is cropped).  labels: int16
 * [Z][Y][X] in raw BraTS coding.  member(v) = float32(src[0][v]) > float32(0.001) && labels[v] == 0.
 * workspace: gts_dataset_stats_workspace(X, Y, Z) bytes (GTS_ERR_SHAPE for a rejected shape); the three calls
 * of one scan share it: D1 leaves the member bit mask there for D2 and D3.  A workspace that is too small:
 * GTS_ERR_SHAPE.  Nothing is launched for a rejected argument.
 * gts_dataset_stats_mask (D1): counts (device uint64 [2], cleared by the call) = the number of members n and
 * the number of members with a non-finite value in some channel.
 * gts_dataset_stats_order_stats (D2): out (device float32 [4][2]) = the values at ranks rank_lo and rank_hi
 * (0 <= rank_lo <= rank_hi < n, n = D1's count) of each channel's member values in ascending order; I2's radix
 * select and its rule for -0.0.
 * gts_dataset_stats_moments (D3): top = HOST float32 [4], copied at launch.  out (device float64 [4][4]): the
 * sum of y_c = float32(v) / top_c (IEEE float32 division) over the members, the sum of y_c^2, the mean and
 * the standard deviation sqrt(sum y^2 / n - mean^2), accumulated in float64 in a fixed order: the same bits
 * on every run, whatever grid the launcher picks. */
int64_t gts_dataset_stats_workspace(int64_t X, int64_t Y, int64_t Z);
int32_t gts_dataset_stats_mask(const void* src, int32_t dtype, const int16_t* labels, int64_t X, int64_t Y, int64_t Z,
                               uint64_t* counts, void* workspace, int64_t workspace_bytes, void* stream);
int32_t gts_dataset_stats_order_stats(const void* src, int32_t dtype, int64_t X, int64_t Y, int64_t Z, int64_t n,
                                      int64_t rank_lo, int64_t rank_hi, float* out, void* workspace,
                                      int64_t workspace_bytes, void* stream);
int32_t gts_dataset_stats_moments(const void* src, int32_t dtype, int64_t X, int64_t Y, int64_t Z, int64_t n,
                                  const float* top, double* out, void* workspace, int64_t workspace_bytes,
                                  void* stream);

/* ---- F1: conform a scan to the pipeline's frame, and labels back onto the scan's grid ----------------------
 * The reference reads and writes volumes as they are stored (data_processing/nifti_io.py:42-57, nibabel) and
 * so only serves LPS 1 mm scans; this gather is the reorientation / resampling step in front of the intake.
 * src: [C][Z][Y][X] (x fastest), dtype by its NIfTI code 4 (int16) or 16 (float32), else GTS_ERR_ARGKIND.
 * dst: [C][OZ][OY][OX] (x fastest).  Output axis k (0 = x) reads input axis axis_k; (axis0, axis1, axis2) must
 * be a permutation of 0..2, else GTS_ERR_ARGKIND.  idx0, idx1 (device int32) and t (device float64) hold
 * OX + OY + OZ entries each: the tables of output axis x, then y, then z.  For output coordinate i of an axis,
 * idx0[i] and idx1[i] are the two indices along the input axis it reads and t[i] the weight of the second;
 * entries are clamped to the input extent before use.
 * mode 0 (exact): dst = src[idx0 ...] in src's dtype, bit for bit; idx1 and t may be NULL.
 * mode 1 (trilinear): dst float32 = the eight neighbours lerped along input x, then y, then z, each lerp
 *   a + (b - a) * t in float64 without contraction (t == 0 gives a itself, whatever b is), rounded to float32
 *   once at the end.
 * mode 2 (nearest): int16 only (else GTS_ERR_ARGKIND); per axis t < 0.5 ? idx0 : idx1, a tie takes idx1.
 * Another mode: GTS_ERR_ARGKIND.  Every extent in [1, 65535] and C * X * Y * Z, C * OX * OY * OZ < 2^31, C >= 0,
 * else GTS_ERR_SHAPE; C == 0 returns GTS_OK without touching the device.  Nothing is launched for a rejected
 * argument.  Reads and writes both run along their own fastest axes (a padded LDS tile when the fastest axis
 * moves). */
int32_t gts_conform_gather(const void* src, int32_t dtype, int64_t C, int64_t X, int64_t Y, int64_t Z, int32_t axis0,
                           int32_t axis1, int32_t axis2, int64_t OX, int64_t OY, int64_t OZ, const int32_t* idx0,
                           const int32_t* idx1, const double* t, int32_t mode, void* dst, void* stream);

/* ---- E1/E2: ensemble prediction over several weight sets and mirrored views (no counterpart in the reference,
 * whose scripts/generate_joint_predictions.py:27-110 takes one GNN and one CNN weight file) --------------------
 * E1 softmax_accumulate: acc[r, :] (+)= sum over s = 0 .. n_sets - 1 of softmax(sets[s][r, :]), every tensor
 *   [rows, classes] fp32 row-major on the device.  `sets` itself is a HOST array of n_sets device pointers; they
 *   reach the kernel by value, at most 8 per launch, longer lists are chunked here.  softmax is the stable form
 *   (row maximum subtracted, denominator summed in class order); the sets are added in ascending s, each one
 *   plain fp32 add onto the running value, so the result does not depend on how a list of sets is split over
 *   calls.  overwrite != 0 starts from zero instead of reading acc.  acc must not alias a set.
 *   classes 1..8, n_sets >= 1, rows >= 0 (0: GTS_OK, nothing launched), else GTS_ERR_SHAPE. */
int32_t gts_softmax_accumulate_f32(const float* const* sets, int64_t n_sets, float* acc, int64_t rows,
                                   int64_t classes, int32_t overwrite, void* stream);
/* E2 argmax_scatter_rows: gts_argmax_scatter_i16 for channels-last scores [cx * cy * cz, n_classes]:
 *   out[xs[i], ys[j], zs[k]] = relabel[argmax_c scores[(i * cy + j) * cz + k, c]] (first maximum; relabel
 *   optional); the other voxels of the caller-zeroed int16 volume `out` are left alone.  Box operands and
 *   limits as gts_argmax_scatter_i16. */
int32_t gts_argmax_scatter_rows_i16(const float* scores, const int16_t* relabel, const int32_t* xs,
                                    const int32_t* ys, const int32_t* zs, int16_t* out, int64_t cx, int64_t cy,
                                    int64_t cz, int64_t dim_y, int64_t dim_z, int64_t n_classes, void* stream);

/* ---- U1/U1n/U2: voxel-wise uncertainty maps of an ensemble and their QU-BraTS style counts (no
 * counterpart in the reference) -------------------------------------------------------------------------------
 * The uncertainty of a row of fp32 class sums s[0..3] (E1's output, the SUM over `terms` softmaxes; classes
 * 0 healthy, 1 edema, 2 NET, 3 ET) for region r (0 WT = {1, 2, 3}, 1 CT = {2, 3}, 2 ET = {3}):
 *   S = the region's sums added as float64 in ascending class order;  p = S / (double)terms clamped to [0, 1];
 *   u = (uint8) rint(200 * min(p, 1 - p)), round-half-to-even, 0..100; a NaN p gives 100.
 * Float64 add, divide, min, multiply and rint only, none contracted: the bits of the same numpy expression.
 * n_classes must be 4 and 1 <= terms <= 2^31, else GTS_ERR_SHAPE.
 * U1 region_uncertainty_rows: out[r, xs[i], ys[j], zs[k]] = u_r(sums[(i * cy + j) * cz + k, :]) for the three
 *   regions; `out` is a caller-zeroed uint8 [3, dim_x, dim_y, dim_z] whose other voxels are left alone.  Box
 *   operands as gts_argmax_scatter_rows_i16, extents at most 32768, c* <= dim_* and cx * cy * cz < 2^31.  A
 *   `sums` pointer that is not 16-byte aligned is read with scalar loads: same bits. */
int32_t gts_region_uncertainty_rows_u8(const float* sums, const int32_t* xs, const int32_t* ys, const int32_t* zs,
                                       uint8_t* out, int64_t cx, int64_t cy, int64_t cz, int64_t dim_x,
                                       int64_t dim_y, int64_t dim_z, int64_t n_classes, int64_t terms, void* stream);
/* U1n region_uncertainty_nodes: out[r, v] = u_r(sums[row(svs[v]), :]) over the n_vox voxels of a partitioning,
 *   row() as gts_project_argmax_i16 resolves an id against n_rows table rows (<= 32768); a background voxel gets
 *   0 in all three maps.  out is uint8 [3, n_vox], written everywhere. */
int32_t gts_region_uncertainty_nodes_u8(const int16_t* svs, const float* sums, uint8_t* out, int64_t n_vox,
                                        int64_t n_rows, int64_t n_classes, int64_t terms, void* stream);
/* U2 uncertainty_histogram: one pass over pred / truth (int16 internal labels, n each) and unc (uint8 [3, n], the
 *   three region maps).  hist is int64 [4][4][GTS_UNCERTAINTY_BINS], ADDED to (the caller zeroes it): blocks 0..2
 *   are the regions, each [outcome: 0 TP, 1 FP, 2 FN, 3 TN of the region masks][map value], bin 101 collecting
 *   every value above 100; hist[3][0][0] counts the voxels with a label outside 0..3 on either side, which are
 *   counted nowhere else.  Integer sums: independent of launch geometry.  0 <= n <= 2^40, else GTS_ERR_SHAPE. */
#define GTS_UNCERTAINTY_BINS 102
#define GTS_UNCERTAINTY_HIST_WORDS 1632
int32_t gts_uncertainty_histogram(const int16_t* pred, const int16_t* truth, const uint8_t* unc, int64_t* hist,
                                  int64_t n, void* stream);

/* ---- R1/R2: co-register modalities that lie on different grids (no counterpart in the reference) --
 * A MOVING volume [Z][Y][X] (x fastest), dtype by its NIfTI code 4 (int16) or 16 (float32), else GTS_ERR_ARGKIND,
 * is sampled where a row-major 3 x 4 float64 matrix T (HOST memory, read at the call) sends the voxel index
 * (x, y, z) of another grid:
 *   u = ((T00 x + T01 y) + T02 z) + T03, v and w likewise from rows 1 and 2, in float64 without contraction;
 *   the sample is inside when 0 <= u <= X-1, 0 <= v <= Y-1 and 0 <= w <= Z-1 (a NaN coordinate is outside);
 *   inside: i0 = min(floor(u), X-1), i1 = min(i0 + 1, X-1), t = u - i0 per axis, the eight neighbours as float64,
 *   lerped along x, then y, then z, each lerp a + (b - a) * t and t == 0 giving a itself (gts_conform_gather's).
 * Every extent in [1, 65535] and every volume below 2^31 voxels, else GTS_ERR_SHAPE; a matrix entry that is not
 * finite: GTS_ERR_ARGKIND.  Nothing is launched for a rejected argument.
 * gts_affine_resample (R1): dst float32 [OZ][OY][OX] = that value rounded once, 0.0f outside.  path 0 picks the
 *   map of lanes to voxels (plain when |T00| is the largest of |T00|, |T10|, |T20|, else a 64 x 64 LDS tile whose
 *   reads run along the input's x), 1 forces the plain map, 2 the tiled one; all give the same bits for every T.
 * gts_joint_histogram (R2): `fixed` is float32 [FZ][FY][FX]; matrices HOST float64 [K][12], 1 <= K <=
 *   GTS_REGISTER_MAX_MATRICES; for every fixed voxel whose x, y and z are multiples of stride (>= 1) and every
 *   matrix k, with f the fixed value and m the moving value (float64, not rounded):
 *     outside: counts[k][B*B] += 1;   inside: counts[k][bin(f, lo_f, scale_f) * B + bin(m, lo_m, scale_m)] += 1,
 *     bin(v, lo, scale) = 0 when v is not finite (tested as v - v == 0.0), else with q = floor((v - lo) * scale):
 *     q >= 1 ? (q < B-1 ? (int)q : B-1) : 0, so a NaN q gives 0 as well.
 *   counts is int64 [K][B*B + 1], zeroed by the call; B = bins in {16, 32, 64}, else GTS_ERR_ARGKIND, as are range
 *   values that are not finite.  Integer LDS tables and integer global atomics only: the counts do not depend on
 *   grid_blocks (0: chosen by the library; tests pass small and large ones) or on any order of arrival. */
#define GTS_REGISTER_MAX_MATRICES 16
int32_t gts_affine_resample(const void* src, int32_t dtype, int64_t X, int64_t Y, int64_t Z, const double* matrix,
                            int64_t OX, int64_t OY, int64_t OZ, float* dst, int32_t path, void* stream);
int32_t gts_joint_histogram(const float* fixed, int64_t FX, int64_t FY, int64_t FZ, const void* moving, int32_t dtype,
                            int64_t X, int64_t Y, int64_t Z, const double* matrices, int64_t K, int64_t stride,
                            int64_t bins, double lo_f, double scale_f, double lo_m, double scale_m, int64_t* counts,
                            int64_t grid_blocks, void* stream);

/* ---- Z1-Z5: bias-field correction of one MRI volume, N4's scheme (no counterpart in the reference) --
 * A volume v[Z][Y][X] (x fastest), dtype by its NIfTI code 4 (int16) or 16 (float32), else GTS_ERR_ARGKIND.  Every
 * extent in [1, 65535] and fewer than 2^31 voxels, else GTS_ERR_SHAPE.  Nothing is launched for a rejected argument.
 * The log field is a sum of `levels` uniform cubic B-spline lattices; level l has spans0 << l cells and n_l = (spans0
 * << l) + 3 control points per axis, spans0 >= 1, 1 <= levels <= 6, spans0 << (levels - 1) <= GTS_BIAS_MAX_SPANS,
 * else GTS_ERR_SHAPE.  Device operands that describe it, shared by Z2-Z5:
 *   lattice  float64, the levels one after another, level l as [n_l][n_l][n_l] with z slowest;
 *   weights  float64 x: [levels][4][X], then y: [levels][4][Y], then z: [levels][4][Z]: the four B-spline weights of
 *            every index of an axis at every level;   cells  int32 x: [levels][X], y: [levels][Y], z: [levels][Z]: the
 *            first control point they sit on (clamped to 0 .. spans - 1 by the kernels).  gts/bias.py tabulates both.
 *   field(x, y, z) = sum_l sum_a Bx_a * (sum_b By_b * (sum_c Bz_c * L_l[cz + c][cy + b][cx + a])): float64 products
 *            and sums, nothing contracted, every sum ascending from its first term, the levels last.
 * u is float32 [Z][Y][X]; its NaNs are outside the mask; d = float64(u) - field.  grid_blocks: workgroups of the
 * pass over the rows (0: the library's choice, else 1 .. 2^31 - 1); no result below depends on it.
 * workspace: gts_bias_workspace(X, Y, Z, spans of the last level) bytes, else GTS_ERR_SHAPE.
 * gts_bias_log (Z1): u = float32(log(float64(v))) where v is finite and v > threshold, NaN elsewhere; *count (device)
 *   = the number of mask voxels.  threshold finite and >= 0, else GTS_ERR_ARGKIND.
 * gts_bias_range (Z2): range (device float64 [2]) = min and max of d over the mask, (+Inf, -Inf) for an empty one.
 * gts_bias_histogram (Z3): counts (device int64 [GTS_BIAS_BINS], zeroed by the call): one count per mask voxel at
 *   clamp(floor((d - lo) / w + 0.5), 0, BINS - 1), w = (hi - lo) / (BINS - 1).  lo, hi finite with hi > lo, else
 *   GTS_ERR_ARGKIND.  LDS integer tables and integer global atomics.
 * gts_bias_fit (Z4): with pos = (d - lo) / w, i0 = clamp(floor(pos), 0, BINS - 2) and the HOST float64 table
 *   [GTS_BIAS_BINS] (finite, else GTS_ERR_ARGKIND): r = d - (table[i0] + (table[i0 + 1] - table[i0]) * (pos - i0)).
 *   fit_weights (device float64 x: [8][X], y: [8][Y], z: [8][Z]) holds, for the fitted `level`, p_a = B_a^3 / sum_a
 *   B_a^2 (rows 0..3) and q_a = B_a^2 (rows 4..7).  out (device float64 [3][n][n][n], n of that level) = num, den,
 *   delta: num[c][b][a] = sum over the mask of pz py px r, den = sum of qz qy qx over the control points each voxel
 *   sits on, delta = num / den and 0 where den == 0.  Float64, no atomics, the same bits on every run and grid.
 * gts_bias_mean (Z5): out (device float64 [3]) = the sum of the field over the mask, the mask's size, their ratio (0
 *   for an empty mask); fixed order, no atomics.
 * gts_bias_apply (Z5): out = float32(float64(v) / exp(field - mean)) at every voxel; field_out, when not NULL,
 *   float32(field - mean).  mean finite, else GTS_ERR_ARGKIND. */
#define GTS_BIAS_BINS 200
#define GTS_BIAS_MAX_SPANS 32
int64_t gts_bias_workspace(int64_t X, int64_t Y, int64_t Z, int64_t spans);
int32_t gts_bias_log(const void* src, int32_t dtype, int64_t X, int64_t Y, int64_t Z, double threshold, float* u,
                     uint64_t* count, void* stream);
int32_t gts_bias_range(const float* u, int64_t X, int64_t Y, int64_t Z, const double* weights, const int32_t* cells,
                       const double* lattice, int64_t spans0, int64_t levels, double* range, void* workspace,
                       int64_t workspace_bytes, int64_t grid_blocks, void* stream);
int32_t gts_bias_histogram(const float* u, int64_t X, int64_t Y, int64_t Z, const double* weights, const int32_t* cells,
                           const double* lattice, int64_t spans0, int64_t levels, double lo, double hi, int64_t* counts,
                           int64_t grid_blocks, void* stream);
int32_t gts_bias_fit(const float* u, int64_t X, int64_t Y, int64_t Z, const double* weights, const int32_t* cells,
                     const double* lattice, int64_t spans0, int64_t levels, int64_t level, const double* fit_weights,
                     double lo, double hi, const double* table, double* out, void* workspace, int64_t workspace_bytes,
                     int64_t grid_blocks, void* stream);
int32_t gts_bias_mean(const float* u, int64_t X, int64_t Y, int64_t Z, const double* weights, const int32_t* cells,
                      const double* lattice, int64_t spans0, int64_t levels, double* out, void* workspace,
                      int64_t workspace_bytes, int64_t grid_blocks, void* stream);
int32_t gts_bias_apply(const void* src, int32_t dtype, int64_t X, int64_t Y, int64_t Z, const double* weights,
                       const int32_t* cells, const double* lattice, int64_t spans0, int64_t levels, double mean,
                       float* out, float* field_out, int64_t grid_blocks, void* stream);

/* ---- S1-S6: morphological brain extraction of one MRI volume (no counterpart in the reference) -----
 * A volume of three axes [X][Y][Z], Z contiguous; the scheme is symmetric in the axes, so a tensor's shape is handed
 * over as it is.  Intensities by their NIfTI code 4 (int16) or 16 (float32), else GTS_ERR_ARGKIND; masks are int16,
 * read as != 0 and written as 0 / 1.  Every extent >= 1 and X * Y * Z < 2^31, else GTS_ERR_SHAPE.  grid_blocks:
 * workgroups of the passes over the voxels (0: the library's choice, else 1 .. 2^31 - 1, else GTS_ERR_SHAPE); every
 * result is an integer or a copied value and depends neither on it nor on scheduling.  workspace:
 * gts_brainmask_workspace(X, Y, Z) bytes (0 for a rejected shape), one size for S3-S5; a smaller one: GTS_ERR_SHAPE.
 * Nothing is launched for a rejected argument.  P = the voxels that are finite and > 0.
 * gts_brain_range (S1): out (device uint64 [2]) = { |P|, the bits of float32(max over P) (0 for an empty P) }.
 * gts_brain_histogram (S2): counts (device int64 [GTS_BRAIN_BINS], zeroed by the call): one count per voxel of P at
 *   min(BINS - 1, floor(float64(v) / hi * BINS)).  hi finite and > 0, else GTS_ERR_ARGKIND.  LDS integer tables,
 *   one integer global atomic per non-empty bin and workgroup.
 * gts_brain_threshold (S2): mask = (v in P and float64(v) >= t), *count (device) = its voxels.  t finite and >= 0,
 *   else GTS_ERR_ARGKIND.
 * gts_ball_morph_i16 (S3): mask_out (may be mask_in) = ((the squared distance, in voxels, from the voxel to the
 *   nearest position whose mask value (!= 0) equals `target` is <= R2) != invert); positions outside the volume count
 *   as `target` iff `outside`.  Dilation by the ball |o|^2 <= R2: (target 1, outside 0, invert 0); erosion with the
 *   outside as background: (0, 1, 1), as foreground: (0, 0, 1).  0 <= R2 <= GTS_BRAIN_MAX_R2 and target, outside,
 *   invert in {0, 1}, else GTS_ERR_ARGKIND.  Three exact passes with a window of floor(sqrt(R2)) voxels.
 * gts_largest_component_i16 (S4): keep_out (may be mask) = the component of mask != 0 with the most voxels, a tie
 *   going to the smaller root of gts_components_roots_i16; connectivity 6 or 26, else GTS_ERR_SHAPE.
 *   stats (device int64 [5]) = { components, voxels of the largest, of the second largest (0 if none), the winner's
 *   root (0 for an empty mask, keep_out then all 0), voxels of the mask }.
 * gts_fill_holes_i16 (S5): mask_out (another buffer) = mask or every voxel of a connectivity-6 component of mask == 0
 *   that has no voxel on a face of the volume.  stats (device int64 [2]) = { voxels of mask_out, voxels filled }.
 * gts_apply_mask (S6): src and dst [C][X][Y][Z] of one dtype (two buffers), 1 <= C <= 64 else GTS_ERR_SHAPE:
 *   dst = src where mask != 0, 0 (also for NaN / Inf) elsewhere; *count (device) = the voxels of the mask. */
#define GTS_BRAIN_BINS 4096
#define GTS_BRAIN_MAX_R2 255
int64_t gts_brainmask_workspace(int64_t X, int64_t Y, int64_t Z);
int32_t gts_brain_range(const void* src, int32_t dtype, int64_t X, int64_t Y, int64_t Z, uint64_t* out,
                        int64_t grid_blocks, void* stream);
int32_t gts_brain_histogram(const void* src, int32_t dtype, int64_t X, int64_t Y, int64_t Z, double hi, int64_t* counts,
                            int64_t grid_blocks, void* stream);
int32_t gts_brain_threshold(const void* src, int32_t dtype, int64_t X, int64_t Y, int64_t Z, double t, int16_t* mask,
                            uint64_t* count, int64_t grid_blocks, void* stream);
int32_t gts_ball_morph_i16(const int16_t* mask_in, int64_t X, int64_t Y, int64_t Z, int32_t R2, int32_t target,
                           int32_t outside, int16_t* mask_out, void* workspace, int64_t workspace_bytes, int32_t invert,
                           int64_t grid_blocks, void* stream);
int32_t gts_largest_component_i16(const int16_t* mask, int64_t X, int64_t Y, int64_t Z, int32_t connectivity,
                                  int16_t* keep_out, int64_t* stats, void* workspace, int64_t workspace_bytes,
                                  int64_t grid_blocks, void* stream);
int32_t gts_fill_holes_i16(const int16_t* mask, int64_t X, int64_t Y, int64_t Z, int16_t* mask_out, int64_t* stats,
                           void* workspace, int64_t workspace_bytes, int64_t grid_blocks, void* stream);
int32_t gts_apply_mask(const void* src, int32_t dtype, int64_t C, int64_t X, int64_t Y, int64_t Z, const int16_t* mask,
                       void* dst, uint64_t* count, int64_t grid_blocks, void* stream);

/* ---- M1-M4: per-lesion measurements of one label volume (no counterpart in the reference) ----------
 * labels int16 [X][Y][Z] (Z contiguous, internal labels 0..3); region 0 WT, 1 CT, 2 ET; roots int32 [X][Y][Z] from
 * gts_components_roots_i16 on the region's 0 / 1 mask (gts_lesionwise_dilate_i16 with dilation 0 writes it) at
 * `connectivity` 6 or 26.  A lesion is a component of that mask.  units (HOST int64 [3], read at the call): the voxel
 * spacing as integers in [1, 10^6] (gts.metrics.spacing_units).  Every result is an exact int64 that depends neither
 * on grid_blocks (0: the library's choice, else 1 .. 2^31 - 1) nor on any order of arrival.
 * Refusals, nothing being launched: a NULL pointer GTS_ERR_NULL; then an extent outside [1, 4097], X * Y * Z >= 2^31,
 * a bad grid_blocks, a workspace below gts_measure_workspace(X, Y, Z) bytes or a table below
 * gts_measure_table_i64s(X, Y, Z, connectivity) entries (both 0 for a refused shape) GTS_ERR_SHAPE; then a region,
 * connectivity or unit out of range GTS_ERR_ARGKIND; then, with B = sum_a u_a^2 (N_a - 1)^2, 2 B >= 2^62
 * GTS_ERR_SHAPE (it needs the units to be valid).  gts_measure_check makes these checks on a shape and units alone.
 * table (device int64): a header of GTS_MEASURE_HEAD_I64 entries { lesions, slice rows, 3-D candidates, in-plane
 * candidates, 0 .. } and one row of GTS_MEASURE_ROW_I64 entries per lesion in arrival order (sort by root):
 *    0 root (1 + the smallest linear index)   1 n   2..4 voxels of label 1, 2, 3
 *    5..10 the box as max(x + 1), max(X - x), max(y + 1), max(Y - y), max(z + 1), max(Z - z)
 *   11..13 sum of x, y, z   14..16 faces F_x, F_y, F_z: (voxel, direction +-a) pairs whose neighbour is outside the mask
 *       or the volume   17 3-D candidates   18 end of its 3-D candidate list (start before M2)   19 its first slice row
 *   20 D3 = max over voxel pairs of sum_a u_a^2 d_a^2   21..23 plane z*, D2, W (see csrc/gts_measure.hip)
 * gts_measure_tables_i16 (M1): clears the header and the rows it uses and fills fields 0..19.  One row per 2 x 2 x 2 cell suffices at
 *   connectivity 26, one per two voxels at 6.
 * gts_measure_candidates (M2): the lists of hull-vertex candidates in the workspace, per lesion (3-D: a voxel that
 *   lacks one of its two neighbours along each of x, y, z) and per lesion and slice of constant z (along x and y).
 * gts_measure_diameters (M3): field 20.  work (device int32 [n_work][3]): (row, tile i, tile j >= i) over a row's
 *   3-D candidates in tiles of GTS_MEASURE_PAIR_TILE; a unit outside the table or the list is skipped.  n_work 0:
 *   nothing is launched.
 * gts_measure_planes (M4): fields 21..23.  work (device int32 [n_work][2]): (row, z - the box's first z); slices
 *   (device int64 [n_slices][2], n_slices = header entry 1, cleared by the call) receives (D2_z, W_z) per slice row,
 *   pairs taken in tiles of GTS_MEASURE_PLANE_TILE; z* is the smallest z with the largest W_z.  n_work 0: nothing is
 *   launched. */
#define GTS_MEASURE_HEAD_I64 8
#define GTS_MEASURE_ROW_I64 24
#define GTS_MEASURE_PAIR_TILE 256
#define GTS_MEASURE_PLANE_TILE 256
int64_t gts_measure_workspace(int64_t X, int64_t Y, int64_t Z);
int64_t gts_measure_table_i64s(int64_t X, int64_t Y, int64_t Z, int32_t connectivity);
int32_t gts_measure_check(int64_t X, int64_t Y, int64_t Z, const int64_t* units);
int32_t gts_measure_tables_i16(const int16_t* labels, const int32_t* roots, int64_t X, int64_t Y, int64_t Z,
                               int32_t region, int32_t connectivity, int64_t* table, int64_t table_i64s,
                               void* workspace, int64_t workspace_bytes, int64_t grid_blocks, void* stream);
int32_t gts_measure_candidates(const int32_t* roots, int64_t X, int64_t Y, int64_t Z, int64_t* table,
                               int64_t table_i64s, void* workspace, int64_t workspace_bytes, int64_t grid_blocks,
                               void* stream);
int32_t gts_measure_diameters(int64_t X, int64_t Y, int64_t Z, const int64_t* units, const int32_t* work,
                              int64_t n_work, int64_t* table, int64_t table_i64s, const void* workspace,
                              int64_t workspace_bytes, int64_t grid_blocks, void* stream);
int32_t gts_measure_planes(int64_t X, int64_t Y, int64_t Z, const int64_t* units, const int32_t* work, int64_t n_work,
                           int64_t* slices, int64_t n_slices, int64_t* table, int64_t table_i64s,
                           const void* workspace, int64_t workspace_bytes, int64_t grid_blocks, void* stream);

/* ---- T1-T5: triangle surfaces of one region's lesions (no counterpart in the reference) -------------
 * Marching tetrahedra on the six Kuhn tetrahedra of every cell of the mask padded by one layer of zeros; definitions,
 * orders and the 16-case rule: csrc/gts_mesh.hip.  roots int32 [X][Y][Z] from gts_components_roots_i16 on the region's
 * 0 / 1 mask at `connectivity` 6 or 26.  Coordinates are half-index units (2 x the voxel-centre index).  Every integer
 * result depends neither on grid_blocks (0: the library's choice, else 1 .. 2^31 - 1) nor on any order of arrival;
 * every float64 result is a gather in a fixed order, bit for bit the same on every run.
 * Refusals, nothing being launched: a NULL pointer that is needed GTS_ERR_NULL; then an extent outside [1, 4097],
 * (X + 1)(Y + 1)(Z + 1) >= 2^31, a bad grid_blocks, more than 2^31 - 1 vertices or (2^31 - 1) / 3 triangles, a
 * workspace below gts_mesh_workspace(X, Y, Z) (gts_mesh_adjacency_workspace(n_vertices)) bytes or a table below
 * gts_mesh_table_i64s(X, Y, Z, connectivity) entries (0 for a refused shape) GTS_ERR_SHAPE; then a connectivity, unit
 * (outside [1, 10^6]), scale (outside (0, 10^6]) or factor (not finite) out of range GTS_ERR_ARGKIND.
 * table (device int64): a header of GTS_MESH_HEAD_I64 entries { lesions, vertices, triangles, 0 .. } and one row of
 * GTS_MESH_ROW_I64 entries per lesion in arrival order (sort by root):
 *    0 root   1 triangles   2..9 triangles per normal class: entry 1 + k for |normal| = (k >> 2 & 1, k >> 1 & 1, k & 1),
 *    k = 1..7, and entry 9 for any other normal (always 0)   10 V6 = sum of p0 . (p1 x p2), 48 x the volume in voxels
 *    (modulo 2^64: exact for a closed surface, which every lesion's is at connectivity 26)
 * gts_mesh_classify (T1, T2): the table, and in the workspace every cell's corner mask and the bases of the emit pass.
 * gts_mesh_emit (T3), after the header came to the host: vertices int32 [n_vertices][3] by ascending (owner cell,
 *   direction), faces int32 [n_faces][3] by ascending (cell, tetrahedron, index), normals out of the lesion, and
 *   face_slot int32 [n_faces], the table row of the face's lesion.  n_vertices and n_faces are the header's; 0: nothing
 *   is launched.
 * gts_mesh_relabel: face_slot[f] = rank[face_slot[f]] (-1 outside [0, n_rank)): arrival order to the caller's order.
 * gts_mesh_adjacency (T4): the CSR of { b : (a, b) is a directed edge of a face }, row_start int32 [n_vertices + 1],
 *   neighbours int32 [3 n_faces], every row ascending.
 * gts_mesh_positions: positions[v][a] = (double)(vertices[v][a] * units[a]) * scale_mm / 2.0 (units: HOST int64 [3]).
 * gts_mesh_smooth (T5): `iterations` times P += lambda (mean - P), then P += mu (mean - P), each a Jacobi step between
 *   positions and scratch (float64 [n_vertices][3]); mean = (the neighbours' sum, left to right in row order) / degree.
 *   The result is in positions.
 * gts_mesh_terms (T5): per face area = 0.5 * sqrt((cx cx + cy cy) + cz cz), c = (p1 - p0) x (p2 - p0), and volume =
 *   ((p0x dx + p0y dy) + p0z dz) / 6.0, d = p1 x p2; no contraction. */
#define GTS_MESH_HEAD_I64 8
#define GTS_MESH_ROW_I64 12
int64_t gts_mesh_workspace(int64_t X, int64_t Y, int64_t Z);
int64_t gts_mesh_table_i64s(int64_t X, int64_t Y, int64_t Z, int32_t connectivity);
int64_t gts_mesh_adjacency_workspace(int64_t n_vertices);
int32_t gts_mesh_classify(const int32_t* roots, int64_t X, int64_t Y, int64_t Z, int32_t connectivity, int64_t* table,
                          int64_t table_i64s, void* workspace, int64_t workspace_bytes, int64_t grid_blocks,
                          void* stream);
int32_t gts_mesh_emit(const int32_t* roots, int64_t X, int64_t Y, int64_t Z, void* workspace, int64_t workspace_bytes,
                      int32_t* vertices, int64_t n_vertices, int32_t* faces, int32_t* face_slot, int64_t n_faces,
                      int64_t grid_blocks, void* stream);
int32_t gts_mesh_relabel(int32_t* face_slot, int64_t n_faces, const int32_t* rank, int64_t n_rank, int64_t grid_blocks,
                         void* stream);
int32_t gts_mesh_adjacency(const int32_t* faces, int64_t n_faces, int64_t n_vertices, int32_t* row_start,
                           int32_t* neighbours, void* workspace, int64_t workspace_bytes, int64_t grid_blocks,
                           void* stream);
int32_t gts_mesh_positions(const int32_t* vertices, int64_t n_vertices, const int64_t* units, double scale_mm,
                           double* positions, int64_t grid_blocks, void* stream);
int32_t gts_mesh_smooth(const int32_t* row_start, const int32_t* neighbours, int64_t n_vertices, int64_t n_faces,
                        double* positions, double* scratch, double lambda, double mu, int64_t iterations,
                        int64_t grid_blocks, void* stream);
int32_t gts_mesh_terms(const double* positions, const int32_t* faces, int64_t n_vertices, int64_t n_faces,
                       double* area, double* volume, int64_t grid_blocks, void* stream);

/* ---- X1-X3: per-lesion intensity range, grey levels, histogram and GLCM (no counterpart in the
 * reference) --------------------------------------------------------------------------------------------------------
 * roots int32 [X][Y][Z] (Z contiguous) from gts_components_roots_i16 at `connectivity` 6 or 26; image [X][Y][Z] of
 * dtype 4 (int16) or 16 (float32).  A lesion is the set of voxels of one root.  Definitions, the direction order and
 * the level expressions: csrc/gts_texture.hip.  Every result is an integer (or a value of the image) that depends
 * neither on grid_blocks (0: the library's choice, else 1 .. 2^31 - 1) nor on any order of arrival.
 * Refusals, nothing being launched, in this order: a NULL pointer GTS_ERR_NULL; an extent outside [1, 4097],
 * X * Y * Z >= 2^31 or a count (rows, lesions, listed voxels, work units) outside its range GTS_ERR_SHAPE; a
 * connectivity or dtype code GTS_ERR_ARGKIND; bins / bin_width GTS_ERR_ARGKIND (bin_width must be 0, for a fixed bin
 * number with bins in [1, GTS_TEXTURE_MAX_LEVELS], or positive and finite, bins then being ignored); a bad grid_blocks
 * GTS_ERR_SHAPE; a workspace below gts_texture_workspace(X, Y, Z) bytes or a table below its size GTS_ERR_SHAPE.
 * gts_texture_workspace and gts_texture_count_i64s return 0 for a refused shape; gts_texture_table_words(lesions,
 * max_levels) returns 0 for max_levels outside [1, GTS_TEXTURE_MAX_LEVELS] or when 4 x the words exceed
 * GTS_TEXTURE_MAX_TABLE_BYTES: the table is lesions x (max_levels + 13 max_levels (max_levels + 1) / 2) int32.
 * gts_texture_counts (X1): counts (device int64): a header of GTS_TEXTURE_HEAD_I64 entries { roots, 0 .. } and one row
 *   of GTS_TEXTURE_COUNT_ROW_I64 entries { root, voxels } per root in arrival order; the workspace keeps every root's
 *   row.  The host selects lesions from it and numbers them 0 .. lesions - 1.
 * gts_texture_ranges (X1): select (device int32 [n_rows]): row -> selected lesion or -1; segments (device int32
 *   [lesions + 1]): the exclusive sums of the selected lesions' voxels, segments[lesions] = n_listed.  ranges (device
 *   int64): a header { non-finite voxels of the selected lesions, 0 .. } and one row of GTS_TEXTURE_RANGE_ROW_I64
 *   entries { lo, hi (encoded: int16 v + 32768; float32 the bits of v + 0.0f, flipped entirely when negative, else
 *   with the sign set), end of the lesion's segment, non-finite voxels } per lesion.  list (device int32 [n_listed])
 *   receives every selected lesion's voxel indices in its segment, in arrival order.
 * gts_texture_levels (X2): plan (device int64 [lesions][GTS_TEXTURE_PLAN_I64]): { lo, hi as float64 bits, levels in
 *   [1, max_levels], root }.  levels (device uint8 [n_listed]) receives the grey level of every listed voxel, the
 *   workspace's level volume the same by voxel; table is cleared and its first lesions x max_levels words receive the
 *   histograms.
 * gts_texture_glcm (X3): work (device int32 [n_work][3]): (lesion, direction 0 .. 12, chunk of GTS_TEXTURE_CHUNK listed
 *   voxels); a unit outside the plan is skipped.  The folded matrices are added to table after the histograms:
 *   [lesion][direction][j (j + 1) / 2 + i], i <= j, with a stride of max_levels (max_levels + 1) / 2, every unordered
 *   neighbouring pair once.  n_work 0: nothing is launched. */
#define GTS_TEXTURE_MAX_LEVELS 128
#define GTS_TEXTURE_DIRECTIONS 13
#define GTS_TEXTURE_CHUNK 2048
#define GTS_TEXTURE_HEAD_I64 8
#define GTS_TEXTURE_COUNT_ROW_I64 2
#define GTS_TEXTURE_RANGE_ROW_I64 4
#define GTS_TEXTURE_PLAN_I64 4
#define GTS_TEXTURE_MAX_TABLE_BYTES 1073741824
int64_t gts_texture_workspace(int64_t X, int64_t Y, int64_t Z);
int64_t gts_texture_count_i64s(int64_t X, int64_t Y, int64_t Z, int32_t connectivity);
int64_t gts_texture_table_words(int64_t lesions, int64_t max_levels);
int32_t gts_texture_counts(const int32_t* roots, int64_t X, int64_t Y, int64_t Z, int32_t connectivity,
                           int64_t* counts, int64_t counts_i64s, void* workspace, int64_t workspace_bytes,
                           int64_t grid_blocks, void* stream);
int32_t gts_texture_ranges(const int32_t* roots, const void* image, int32_t dtype, int64_t X, int64_t Y, int64_t Z,
                           const int32_t* select, int64_t n_rows, const int32_t* segments, int64_t lesions,
                           int64_t* ranges, int64_t ranges_i64s, int32_t* list, int64_t n_listed,
                           const void* workspace, int64_t workspace_bytes, int64_t grid_blocks, void* stream);
int32_t gts_texture_levels(const void* image, int32_t dtype, int64_t X, int64_t Y, int64_t Z, int32_t bins,
                           double bin_width, const int32_t* segments, const int64_t* plan, int64_t lesions,
                           const int32_t* list, int64_t n_listed, uint8_t* levels, int32_t* table, int64_t table_words,
                           int64_t max_levels, void* workspace, int64_t workspace_bytes, int64_t grid_blocks,
                           void* stream);
int32_t gts_texture_glcm(const int32_t* roots, int64_t X, int64_t Y, int64_t Z, const int32_t* work, int64_t n_work,
                         const int32_t* segments, const int64_t* plan, int64_t lesions, const int32_t* list,
                         const uint8_t* levels, int64_t n_listed, int32_t* table, int64_t table_words,
                         int64_t max_levels, const void* workspace, int64_t workspace_bytes, int64_t grid_blocks,
                         void* stream);

/* ---- X4-X6: per-lesion run-length, size-zone, dependence and neighbourhood-difference tables (GLRLM, GLSZM, GLDM,
 * NGTDM; no counterpart in the reference) ------------------------------------------------------------
 * They run after gts_texture_levels on the same roots, segments, plan, list, levels and workspace (whose level volume
 * they read).  Definitions: csrc/gts_texture_matrices.hip.  Every result is an integer that depends neither on
 * grid_blocks nor on any order of arrival, the order of the zone records excepted (the host sorts them).
 * Refusals, nothing being launched, in this order: a NULL pointer GTS_ERR_NULL; a shape outside X1-X3's limits, a
 * count (lesions, listed voxels, work units: at least 1), max_levels outside [1, GTS_TEXTURE_MAX_LEVELS] or longest
 * outside [1, GTS_TEXTURE_MAX_RUN] GTS_ERR_SHAPE; a negative alpha GTS_ERR_ARGKIND; a bad grid_blocks GTS_ERR_SHAPE; a
 * workspace, scratch, record buffer or table below its size GTS_ERR_SHAPE.
 * gts_texture_run_words(lesions, max_levels, longest): the int32 words of the run table, lesions x 13 x max_levels x
 *   longest; 0 outside the limits or when 4 x the words exceed GTS_TEXTURE_MAX_TABLE_BYTES.
 * gts_texture_neighbourhood_i64s(lesions, max_levels): the int64 entries of X6's table, 3 x lesions x max_levels x
 *   GTS_TEXTURE_DEPENDENCES; 0 outside the limits or above the same byte cap.
 * gts_texture_run_lengths (X4, first pass): work is X3's (lesion, direction, chunk).  run_length (device uint16
 *   [13][n_listed]) receives per direction and listed voxel the length of the run that starts there, 0 where none
 *   does; head (device int64 [GTS_TEXTURE_HEAD_I64]) is cleared and head[0] receives the longest run.
 * gts_texture_runs (X4, second pass): table (device int32) is cleared and receives [lesion][direction][level]
 *   [length - 1] with strides max_levels and longest, longest being at least head[0] of the first pass.
 * gts_texture_zones (X5): scratch (device int32, 2 X Y Z words: parents and sizes by voxel).  records (device int32
 *   [n_listed][GTS_TEXTURE_ZONE_RECORD_I32]) receives { lesion, level, voxels } per zone in arrival order; head is
 *   cleared, head[0] receives the number of zones and head[1] the number of root searches that passed n_listed steps
 *   (a forest that is not well formed): the records are then not to be used.
 * gts_texture_neighbourhood (X6): work (device int32 [n_work][2]): (lesion, chunk).  table (device int64) is cleared
 *   and receives gldm, ngtdm_n and ngtdm_s one after another, each [lesion][level][GTS_TEXTURE_DEPENDENCES] with a
 *   stride of max_levels: column k - 1 of gldm is dependence k at `alpha`, column m of the others is a neighbourhood
 *   of m voxels. */
#define GTS_TEXTURE_NEIGHBOURS 26
#define GTS_TEXTURE_DEPENDENCES 27
#define GTS_TEXTURE_MAX_RUN 4097
#define GTS_TEXTURE_ZONE_RECORD_I32 3
int64_t gts_texture_run_words(int64_t lesions, int64_t max_levels, int64_t longest);
int64_t gts_texture_neighbourhood_i64s(int64_t lesions, int64_t max_levels);
int32_t gts_texture_run_lengths(const int32_t* roots, int64_t X, int64_t Y, int64_t Z, const int32_t* work,
                                int64_t n_work, const int32_t* segments, const int64_t* plan, int64_t lesions,
                                const int32_t* list, const uint8_t* levels, int64_t n_listed, uint16_t* run_length,
                                int64_t run_length_words, int64_t* head, const void* workspace,
                                int64_t workspace_bytes, int64_t grid_blocks, void* stream);
int32_t gts_texture_runs(const int32_t* work, int64_t n_work, const int32_t* segments, const int64_t* plan,
                         int64_t lesions, const uint8_t* levels, const uint16_t* run_length, int64_t n_listed,
                         int32_t* table, int64_t table_words, int64_t max_levels, int64_t longest, int64_t grid_blocks,
                         void* stream);
int32_t gts_texture_zones(const int32_t* roots, int64_t X, int64_t Y, int64_t Z, const int32_t* segments,
                          const int64_t* plan, int64_t lesions, const int32_t* list, const uint8_t* levels,
                          int64_t n_listed, int32_t* scratch, int64_t scratch_words, int32_t* records,
                          int64_t records_words, int64_t* head, const void* workspace, int64_t workspace_bytes,
                          int64_t grid_blocks, void* stream);
int32_t gts_texture_neighbourhood(const int32_t* roots, int64_t X, int64_t Y, int64_t Z, const int32_t* work,
                                  int64_t n_work, const int32_t* segments, const int64_t* plan, int64_t lesions,
                                  const int32_t* list, const uint8_t* levels, int64_t n_listed, int32_t alpha,
                                  int64_t* table, int64_t table_i64s, int64_t max_levels, const void* workspace,
                                  int64_t workspace_bytes, int64_t grid_blocks, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GTS_HIP_H */
