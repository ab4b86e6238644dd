/*
 * dcnr.h -- C ABI of libdcnr.so, the MI355X (gfx950) DCN-R ranking hot path.
 *
 * Drop-in boundary for the reference's DCN-R path.  The reference
 * (Krist-Marrakesh/Hybrid-Hotel-Recommendation-System-Based-on-Friends-
 * Recommendations) has no FFI of its own: its boundary is the PyTorch module
 * DCN_RecSys and its callers.  Each entry point below replaces one reference
 * interface (file:line in the reference repository):
 *
 *   dcnr_forward          DCN_RecSys.forward            train.py:155-170 (dup main.py:114-127)
 *                         incl. ResBlock.forward          train.py:112-122
 *                         and CrossLayer.forward          train.py:96-99
 *   dcnr_gather_cross     the front of DCN_RecSys.forward: embedding gathers,
 *                         x0 concat and the cross network   train.py:156-159,166-168
 *                         (BASELINE configs[1])
 *   dcnr_backward         loss.backward() through the model   train.py:225
 *   dcnr_bce_with_logits  nn.BCEWithLogitsLoss()(preds, y)    train.py:206,224,233,376
 *   dcnr_forward_bce      the train forward and that loss as one call: a step's
 *                         preds = model(...); criterion(preds, y)  train.py:223-224
 *   dcnr_adam_step        torch.optim.AdamW/Adam(...).step()  train.py:201-204,226
 *   dcnr_cosine_topk      NearestNeighbors(metric='cosine', algorithm='brute')
 *                         .kneighbors(vec, n_neighbors=k)      main.py:196-203,268-270,300
 *   dcnr_cosine_neighbor_table
 *                         that index's answer for every row of its own fitted
 *                         data (the only queries main.py:200, 300 make), once
 *   dcnr_row_inv_norms    the row normalisation inside sklearn's cosine metric
 *   dcnr_gather_rows      the batch assembly of TensorDataset + DataLoader
 *                         (train.py:195-196) on a device-resident dataset
 *   dcnr_candidate_union  _generate_candidates' union of positives and their
 *                         neighbours[1:]                      main.py:196-203
 *                         (dcnr_candidate_union_table, dcnr_requests_candidates_table:
 *                         the neighbours read from the item neighbour table)
 *   dcnr_ranking_batch    preprocess_for_ranking              main.py:215-230
 *   dcnr_rank_by_score    sorted(zip(scores, ids), reverse=True) main.py:325
 *   dcnr_mmr_rerank       rerank_with_mmr                     main.py:133-169
 *   dcnr_requests_*       the same four steps for a batch of requests, one
 *                         workgroup per request               main.py:309-332
 *   dcnr_requests_sources, dcnr_requests_recommended_by
 *                         the friends, positives / negatives and recommended_by
 *                         lists of those requests    main.py:172-194, 336-351
 *   dcnr_csr_insert       new main_df / friendships_df rows into those CSRs on the
 *                         device (the reference reloads both at start-up only)
 *   dcnr_csr_remove       the mirror: main_df.drop(rows) and dropped friendships_df
 *                         rows taken out of those CSRs on the device
 *   dcnr_eval_metrics     roc_auc_score / BCEWithLogitsLoss / sqrt(mean_squared_error)
 *                         over the validation logits          train.py:255-265, 366-387
 *   dcnr_eval_group_metrics  GAUC, NDCG@k, hit rate@k, recall@k and MRR of every
 *                         user's (or item's) list in the order main.py:325 serves it
 *   dcnr_eval_list_metrics   what the served lists look like under lambda_param
 *                         (rerank_with_mmr, main.py:133-169): intra-list diversity,
 *                         coverage, Gini of the exposure, mean weight, held-out hits
 *
 * Conventions
 *  - All tensor pointers are DEVICE pointers owned by the caller; the
 *    library allocates nothing on the hot path (workspace is caller-owned,
 *    size from dcnr_workspace_size / dcnr_cosine_topk_workspace_size).
 *    dcnr_forward (train mode: the embedding backward's id sort) and
 *    dcnr_backward (the cross backward) fork part of their work onto one
 *    library-owned stream per device (created on first use) and join it back
 *    into `stream` before they return their last kernels; callers see
 *    ordinary stream semantics.
 *  - Parameter tables are HOST arrays of device pointers:
 *      params: in the reference's state_dict() order (train.py:136-153):
 *        user_embedding.weight, item_embedding.weight,
 *        cat_embeddings.{k}.weight (k < n_cat),
 *        initial_deep_layer.weight [H,D], initial_deep_layer.bias [H],
 *        for j < n_res: res_blocks.{j}.{layer1.weight, layer1.bias,
 *            bn1.weight, bn1.bias, bn1.running_mean, bn1.running_var,
 *            bn1.num_batches_tracked (int64 scalar), layer2.weight,
 *            layer2.bias, bn2.weight, bn2.bias, bn2.running_mean,
 *            bn2.running_var, bn2.num_batches_tracked},
 *        for l < n_cross: cross_network.{l}.b [D], cross_network.{l}.w.weight [1,D],
 *        final_linear.weight [1,H+D], final_linear.bias [1]
 *      grads: in named_parameters() order (the same list without the BN
 *        running_mean / running_var / num_batches_tracked buffers).
 *    Every floating tensor is fp32, contiguous, row-major.
 *  - Index tensors are int64 (torch.long) like the reference; indices are
 *    clamped in-kernel (never an out-of-bounds access) and, with
 *    DCNR_FLAG_CHECK_INDICES, an out-of-range index is reported as
 *    DCNR_INDEX_OOB by dcnr_check_errors (torch raises IndexError there).
 *  - Everything is stream-ordered and asynchronous on `stream` (a
 *    hipStream_t); functions return after enqueueing.  No entry point
 *    synchronises except dcnr_check_errors.
 *  - Status codes are returned, never thrown or aborted across the ABI;
 *    dcnr_last_error() gives a thread-local message for the last failure.
 *  - Eval-mode forward is re-entrant (no shared scratch); train-mode forward
 *    mutates BN running statistics and must be serialised by the caller.
 */
#ifndef DCNR_H
#define DCNR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCNR_ABI_VERSION 4

typedef void* dcnr_stream_t; /* hipStream_t */

typedef enum {
  DCNR_OK = 0,
  DCNR_BAD_ARG = 1,
  DCNR_INDEX_OOB = 2,
  DCNR_HIP_ERROR = 3,
  DCNR_UNSUPPORTED_SHAPE = 4,
  DCNR_WORKSPACE_TOO_SMALL = 5
} dcnr_status;

typedef enum { DCNR_PREC_FP32 = 0, DCNR_PREC_BF16 = 1 } dcnr_precision;
typedef enum { DCNR_EVAL = 0, DCNR_TRAIN = 1 } dcnr_mode;

#define DCNR_FLAG_CHECK_INDICES 1u
/* Train workspace keeps every residual block's backward intermediates (du,
 * dt2, da, dt1) in buffers of their own instead of reusing one set: the
 * stage-by-stage parity tests read them (dcnr_workspace_offset).  Same
 * kernels, same results; more workspace.  In eval mode it keeps the
 * unfused tail (BN affine finalize launch, the last block's output h_R in
 * the workspace, separate head dot); without it the bf16 eval forward ends
 * in the last GEMM's head epilogue and never stores h_R; likewise the bf16
 * train forward does not store h_R (the backward rebuilds it from t2 and
 * h_{R-1}), so DCNR_WS_H at index R is only meaningful with this flag. */
#define DCNR_FLAG_KEEP_INTERMEDIATES 2u
/* bf16 eval forward: take the fused deep tower (one persistent launch, the
 * activations on chip) at any batch size it supports.  Without the flag it
 * is taken from 16384 samples on, where it overtakes the layer-by-layer path;
 * below that the layer path is faster (the tower walks a tile's layers in
 * sequence on one CU).  Same results either way up to bf16 rounding order. */
#define DCNR_FLAG_FUSED_TOWER 4u
/* Train mode (ABI 4): the backward leaves the embedding tables' gradient rows
 * that the batch did not reference as they were (no 142 MB zero fill at the
 * bench shape) and instead marks, in a byte map at the end of the workspace
 * (DCNR_WS_ROW_MAP: one byte per table row, the tables in order, 1 = this
 * call wrote the row), every row it wrote.  dcnr_adam_step_rows reads the map
 * and treats unmarked rows' gradients as exactly 0, which is bit-identical to
 * the dense-gradient step.  Only with accumulate = 0 (the flag and accumulate
 * together are DCNR_BAD_ARG).  Same workspace offsets for every other tensor. */
#define DCNR_FLAG_ROW_MAP 8u
/* Train step with BCE-with-logits, set on both calls of the pair
 * dcnr_forward_bce -> dcnr_backward: the forward's head pass goes on from each
 * row's logit to dlogits and to the last residual block's BatchNorm-backward
 * column partials, which it leaves in the workspace; dcnr_backward then runs
 * no statistics pass over that block (it reads those partials, and `dlogits`
 * must be the buffer that forward wrote, unchanged).  Taken where the bf16
 * fused head applies (hidden padded to 512) without
 * DCNR_FLAG_KEEP_INTERMEDIATES and without a bn_allreduce hook; everywhere
 * else the flag changes nothing.  Same results bit for bit, same workspace
 * layout.  dcnr_forward ignores it. */
#define DCNR_FLAG_HEAD_STATS 16u

/* Optional collective hook for SyncBN across data-parallel ranks: called
 * (stream-ordered, from the calling thread) with a device buffer of `count`
 * fp64 values that must be summed over all ranks in place before the call
 * returns or is stream-ordered before later work on `stream`.  NULL = local
 * BN (each rank normalises with its own batch statistics). */
typedef int (*dcnr_allreduce_fn)(void* ctx, double* device_buf, int64_t count, dcnr_stream_t stream);

/* Optional data-parallel hook of dcnr_backward: called (from the calling
 * thread, while the call enqueues its work) as soon as every kernel that
 * writes a group of gradients has been enqueued on `stream`:
 *   DCNR_GRADS_DENSE      initial_deep_layer .. final_linear (every
 *                         parameter after the embedding tables)
 *   DCNR_GRADS_EMBEDDING  user, item and categorical tables (last)
 * A caller starts that group's exchange from here (ordered after the
 * stream's work so far), so the dense group's exchange runs under the
 * embedding backward.  Nonzero return = failure (dcnr_backward fails). */
#define DCNR_GRADS_DENSE 0
#define DCNR_GRADS_EMBEDDING 1
typedef int (*dcnr_grad_ready_fn)(void* ctx, int32_t group, dcnr_stream_t stream);

/* Accepted model shapes.  Every entry point that takes a dcnr_model_desc checks
 * them first, before anything is launched, and dcnr_last_error names the
 * offending value:
 *   n_cat      0..64, every cat_rows[k] >= 1; n_users, n_items >= 1  (DCNR_BAD_ARG)
 *   emb_dim, hidden >= 1, n_num >= 0; precision FP32 or BF16          (DCNR_BAD_ARG)
 *   n_res      1..8                                        (DCNR_UNSUPPORTED_SHAPE)
 *   n_cross    0..7                                        (DCNR_UNSUPPORTED_SHAPE)
 *   input dim  D <= 1024 (dcnr_input_dim)                  (DCNR_UNSUPPORTED_SHAPE)
 *   hidden     rounded up to 8: <= 2048 with DCNR_PREC_BF16 (hidden <= 2048),
 *              <= 1024 with DCNR_PREC_FP32 (hidden <= 1024) (DCNR_UNSUPPORTED_SHAPE) */
typedef struct {
  int64_t n_users;          /* user_embedding rows      (train.py:136) */
  int64_t n_items;          /* item_embedding rows      (train.py:137) */
  int32_t n_cat;            /* number of categorical tables (len(cat_dims)) */
  const int64_t* cat_rows;  /* HOST array [n_cat]: cat_dims.values() (train.py:138-139) */
  int32_t emb_dim;          /* params['emb_dim'] */
  int32_t n_num;            /* n_num_features */
  int32_t hidden;           /* params['hidden_dim'] */
  int32_t n_cross;          /* params['n_cross_layers'] */
  int32_t n_res;            /* params.get('n_res_blocks', 2) */
  float dropout;            /* params['dropout'] (applied in train mode only) */
  int32_t precision;        /* dcnr_precision of the deep-tower GEMMs/activations */
  uint32_t flags;           /* DCNR_FLAG_* */
  dcnr_allreduce_fn bn_allreduce; /* SyncBN hook or NULL */
  void* bn_allreduce_ctx;
  dcnr_grad_ready_fn grad_ready;  /* gradient-group hook or NULL (ABI 2) */
  void* grad_ready_ctx;
  /* ABI 3.  With DCNR_FLAG_CHECK_INDICES: where dcnr_forward's last kernel
   * stores the call's index-error word (0 = every id in range), e.g. a slot
   * of pinned host memory the caller polls once an event recorded after the
   * call has completed -- no copy of its own on the stream.  NULL: the word
   * stays in the workspace (dcnr_check_errors / a caller's copy). */
  int32_t* error_mirror;
} dcnr_model_desc;

int dcnr_abi_version(void);
const char* dcnr_last_error(void);

/* Input dim D = 2*emb_dim + sum(int(sqrt(n_cat_k))+1) + n_num (train.py:139-141). */
int64_t dcnr_input_dim(const dcnr_model_desc* desc);

/* Workspace bytes for a batch of B in `mode`.  A train-mode workspace holds
 * the saved activations that dcnr_backward consumes. */
dcnr_status dcnr_workspace_size(const dcnr_model_desc* desc, int64_t B, int mode, size_t* bytes);

/* Where a stored tensor lives in the workspace of (desc, B, mode), for tests
 * that check each stage against a recomputation from the kernels' own stored
 * inputs.  Row-major with leading dimension Hp = hidden rounded up to 8
 * (Dp for x0, Dq = Dp rounded up to 32 for dx0); element type bf16 in bf16
 * mode, else fp32 (masks: 1 bit per element, Hp/8 bytes per row; BN vectors,
 * zc, dx0, xcoef, sc: fp32).  dx0 is the deep tower's part of d loss/d x0;
 * the cross network's part is sum_k xcoef[b][k] V_k with V = (w_0 .. w_{L-1},
 * w_f[H:]), xcoef [B][L+1]; sc [B][2L+1] holds the forward's per-sample cross
 * scalars (x_l . w_l for l < L, x_0 . w_m for m < L, x_0 . w_f[H:]).  `index` is
 * the block j (h: 0..n_res; bn_*: 2j for bn1, 2j+1 for bn2).  *offset = -1
 * when that tensor is not materialised in this configuration. */
typedef enum {
  DCNR_WS_X0 = 0, DCNR_WS_H = 1, DCNR_WS_T1 = 2, DCNR_WS_T2 = 3, DCNR_WS_A1 = 4,
  DCNR_WS_MASK_A1 = 5, DCNR_WS_MASK_H = 6, DCNR_WS_BN_MEAN = 7, DCNR_WS_BN_INVSTD = 8,
  DCNR_WS_BN_SCALE = 9, DCNR_WS_BN_SHIFT = 10, DCNR_WS_DU = 11, DCNR_WS_DT2 = 12,
  DCNR_WS_DA = 13, DCNR_WS_DT1 = 14, DCNR_WS_G = 15, DCNR_WS_DX0 = 16, DCNR_WS_ZC = 17,
  DCNR_WS_XCOEF = 18, DCNR_WS_SC = 19, DCNR_WS_ROW_MAP = 20, DCNR_WS_KINDS = 21
} dcnr_ws_tensor;
dcnr_status dcnr_workspace_offset(const dcnr_model_desc* desc, int64_t B, int mode, int kind,
                                  int index, int64_t* offset);

/* DCN_RecSys.forward: logits[B] (fp32, device).  mode = DCNR_TRAIN uses
 * batch statistics (B >= 2), updates BN running stats and
 * num_batches_tracked in `params`, applies dropout with `dropout_seed`, and
 * keeps the activations backward needs in `ws`. */
dcnr_status dcnr_forward(const dcnr_model_desc* desc, void* const* params,
                         const int64_t* user_ids, const int64_t* item_ids,
                         const int64_t* cat_features /* [B,n_cat] */,
                         const float* num_features /* [B,n_num] */, int64_t B, int mode,
                         uint64_t dropout_seed, float* logits, void* ws, size_t ws_bytes,
                         dcnr_stream_t stream);

/* The embedding gathers, x0 concat and cross network of DCN_RecSys.forward
 * on their own (train.py:156-159 and 166-168), fp32:
 *   x0[b]        = [U[u_b] | I[i_b] | C_0[c_b0] .. C_{K-1}[c_b,K-1] | num_b]   (bit-exact copy)
 *   cross_out[b] = x_L,  x_{l+1} = x_l + x_l * (x_l . w_l) + b_l     (CrossLayer, train.py:96-99)
 * x0 [B][ld_x0] and cross_out [B][ld_cross] are fp32 device buffers (either
 * may be NULL; ld >= D).  params as for dcnr_forward (only the embedding
 * tables and cross_network.* are read).  oob_flag: optional device int32 that
 * is set nonzero when an id is out of range (ids are clamped in-kernel).
 * Stateless and re-entrant. */
dcnr_status dcnr_gather_cross(const dcnr_model_desc* desc, void* const* params,
                              const int64_t* user_ids, const int64_t* item_ids,
                              const int64_t* cat_features, const float* num_features, int64_t B,
                              float* x0, int64_t ld_x0, float* cross_out, int64_t ld_cross,
                              int32_t* oob_flag, dcnr_stream_t stream);

/* Backward of the last train-mode dcnr_forward on `ws`: given dL/dlogits
 * [B], writes dL/dparam for every parameter into `grads`.  accumulate = 0
 * overwrites (embedding grads are zeroed, then every referenced row gets the
 * sum of its samples' dx0 rows, i.e. embedding_dense_backward semantics);
 * accumulate = 1 adds into grads.  Deterministic: the embedding sums run in
 * a fixed order after a stable sort of the ids, and every other reduction is
 * fixed-order too, so two calls on the same inputs give bit-identical
 * gradients. */
dcnr_status dcnr_backward(const dcnr_model_desc* desc, void* const* params, void* const* grads,
                          const int64_t* user_ids, const int64_t* item_ids,
                          const int64_t* cat_features, const float* num_features, int64_t B,
                          const float* dlogits, uint64_t dropout_seed, int accumulate, void* ws, size_t ws_bytes,
                          dcnr_stream_t stream);

/* The embedding rows the batch of the last train-mode dcnr_forward on `ws`
 * touched, read from that forward's stable id sort (the sorted (id, sample)
 * pairs the backward's fixed-order sums walk; still in `ws` after
 * dcnr_backward): the data-parallel sparse gradient exchange
 * (SURVEY.md 8(e) option B; the gradient rows come from train.py:156-158
 * under train.py:225) buckets them by owner without a torch.unique.
 * For each of n_tables tables (indices into the model's tables: 0 = user,
 * 1 = item, 2.. = categorical) writes the flat element offsets
 * elem_off[i] + row * width of its distinct rows, ascending, to
 * out_offsets[i*B ..] and their number to table_counts[i]; owner_counts[r]
 * (r < world <= DCNR_TOUCHED_MAX_WORLD) counts the offsets in
 * [r*shard_elems, (r+1)*shard_elems); an offset at or beyond
 * world*shard_elems is listed in out_offsets and table_counts but is in no
 * owner's count.  out_offsets[i*B + table_counts[i] ..] is not written.
 * B = 0: both counts zeroed.  world outside 1..DCNR_TOUCHED_MAX_WORLD,
 * shard_elems < 1 or a negative elem_off: DCNR_BAD_ARG, nothing launched.
 * Stream-ordered; outputs are device memory. */
#define DCNR_TOUCHED_MAX_WORLD 64

/* The sparse exchange's send buffers, built on the device from
 * dcnr_emb_touched_rows' output (SURVEY.md 8(e) option B; the rows of the
 * dense gradient of train.py:156-158 under train.py:225): for each of
 * n_tables tables, the table_counts[t] (device) offsets offsets[t*ld ..] and
 * the `width`-float gradient rows of `grad` they address are appended, tables
 * in order, to out_offsets / out_rows [sum(table_counts)][width].  Offsets
 * ascend within a table and the tables are in flat order, so the list is
 * grouped by shard owner.  Stream-ordered; no host synchronisation. */
dcnr_status dcnr_sparse_pack(const float* grad, const int64_t* offsets, int64_t ld,
                             const int64_t* table_counts, int32_t n_tables, int32_t width,
                             int64_t* out_offsets, float* out_rows, dcnr_stream_t stream);

/* The owner's half of the sparse exchange: zeroes shard [shard_elems] (flat
 * elements [shard_lo, shard_lo + shard_elems) of the gradient) and adds the
 * rows the n_sources ranks sent, back to back in `offsets` / `rows`
 * (source_counts[r] rows from rank r: a HOST array), sources in rank order --
 * every shard row is summed 0 + g_0 + g_1 + ..., the same bits run to run.
 * Within one source the rows are distinct and do not overlap.  A row is added
 * only if all of it lies in the shard (shard_lo <= offset and offset + width
 * <= shard_lo + shard_elems); a row below, beyond or straddling either end
 * of the shard is skipped whole. */
dcnr_status dcnr_sparse_accumulate(float* shard, int64_t shard_lo, int64_t shard_elems, int32_t width,
                                   const int64_t* offsets, const float* rows,
                                   const int64_t* source_counts, int32_t n_sources,
                                   dcnr_stream_t stream);
dcnr_status dcnr_emb_touched_rows(const dcnr_model_desc* desc, const void* ws, size_t ws_bytes,
                                  int64_t B, int32_t n_tables, const int32_t* tables,
                                  const int64_t* elem_off, int64_t shard_elems, int32_t world,
                                  int64_t* out_offsets, int64_t* table_counts,
                                  int64_t* owner_counts, dcnr_stream_t stream);

size_t dcnr_bce_workspace_size(void);

/* BCEWithLogitsLoss (mean): loss[0] = mean(max(z,0) - z*y + log1p(exp(-|z|)));
 * if dlogits != NULL also writes dlogits = grad_scale * (sigmoid(z) - y) / B.
 * Deterministic (fixed-order fp64 reduction through `ws`). */
dcnr_status dcnr_bce_with_logits(const float* logits, const float* labels, int64_t B,
                                 float* loss, float* dlogits, float grad_scale, void* ws,
                                 size_t ws_bytes, dcnr_stream_t stream);

/* dcnr_forward in train mode followed by dcnr_bce_with_logits(logits, labels,
 * B, loss, dlogits, grad_scale, bce_ws, ...) as one call (B >= 2; loss and
 * dlogits are required): the same logits, loss, dlogits, running statistics
 * and saved activations, bit for bit.  With DCNR_FLAG_HEAD_STATS in
 * desc->flags the last residual block's pass also produces dlogits and that
 * block's BatchNorm-backward partials for the dcnr_backward that follows on
 * `ws` with the same flags and this `dlogits` (see the flag). */
dcnr_status dcnr_forward_bce(const dcnr_model_desc* desc, void* const* params,
                             const int64_t* user_ids, const int64_t* item_ids,
                             const int64_t* cat_features, const float* num_features, int64_t B,
                             uint64_t dropout_seed, const float* labels, float grad_scale,
                             float* logits, float* loss, float* dlogits, void* bce_ws,
                             size_t bce_ws_bytes, void* ws, size_t ws_bytes,
                             dcnr_stream_t stream);

/* The reference's validation metrics (train.py:255-265, 366-387) over n
 * logits and labels, all n in one set as the reference's single validation
 * batch: BCEWithLogitsLoss, sklearn's roc_auc_score(y, z) and
 * sqrt(mean_squared_error(y, sigmoid(z))).  The struct is written to DEVICE
 * memory, stream-ordered; a caller copies its 72 bytes when it wants them. */
typedef struct {
  double logloss;       /* mean(max(z,0) - z*y + log1p(exp(-|z|))), terms and sum in fp64 */
  double auc;           /* (double)auc_u2 / (2.0 * n_pos * n_neg); NaN if n_pos * n_neg == 0 */
  double rmse;          /* sqrt(mean((y - p)^2)), p = (float)(1/(1+exp(-(double)z))), sum fp64 */
  int64_t n, n_pos, n_neg; /* n_pos: labels == 1.0f; n_neg = n - n_pos */
  int64_t auc_u2;       /* 2U, exact: sum over positives i of
                           2 * #{neg j: z_j < z_i} + #{neg j: z_j == z_i} */
  int64_t n_bad_label;  /* labels that are neither 0.0f nor 1.0f */
  int64_t n_nan;        /* NaN logits */
} dcnr_metrics;

/* Workspace bytes of dcnr_eval_metrics for n logits (0 for n <= 0): two
 * 8-byte keys per logit for the sort plus its counters,
 *   16 n + 4 * 2048 * (3 + U) + 40 * P + 40 * A   (+ < 2 KiB of alignment),
 * U = min(1024, ceil(n / 4096)), P = min(1024, ceil(n / 8192)),
 * A = ceil(n / max(2048, ceil(n / 1024) rounded up to 256)). */
size_t dcnr_eval_metrics_workspace_size(int64_t n);

/* AUC is exact: the midrank Mann-Whitney statistic (algebraically the
 * trapezoid area sklearn integrates) from a full stable sort of the scores;
 * equality is IEEE equality (-0.0 == +0.0; +-inf are ordinary values), and
 * auc_u2 is an integer, the same whatever the kernels' order.  logloss and
 * rmse are fixed-order fp64 reductions: the same input gives the same bits.
 * NaN logits and labels other than 0 / 1 are counted (n_nan, n_bad_label);
 * the metrics of such an input are unspecified (sklearn raises there; the
 * Python layer does too).  0 <= n < 2^31; n = 0 writes a zeroed struct with
 * NaN metrics and reads neither input nor workspace. */
dcnr_status dcnr_eval_metrics(const float* logits, const float* labels, int64_t n,
                              dcnr_metrics* out, void* ws, size_t ws_bytes, dcnr_stream_t stream);

/* Per-group ranking metrics over n (logit, label, group) rows: what
 * /recommendations does is order one user's hotels by a stable descending
 * sort of the logits (main.py:325), and these judge that order per group
 * (user, item, ...): AUC per group (GAUC), NDCG@k, hit rate@k, recall@k and
 * MRR, for up to DCNR_GROUP_MAX_K cutoffs.  Both structs are written to
 * DEVICE memory, stream-ordered.
 *
 * Inside a group the rows are ranked 1, 2, ... by descending logit under IEEE
 * equality (-0.0 == +0.0), ties in ascending input position: the served
 * order, not an average over ties. */
#define DCNR_GROUP_MAX_K 4

typedef struct {          /* one group u; 96 bytes; all zero for a group with no row */
  int64_t n, n_pos;       /* rows, labels == 1.0f */
  int64_t auc_u2;         /* 2U of dcnr_metrics.auc_u2 restricted to the group */
  int64_t first_pos_rank; /* 1-based rank of the first positive, 0 if n_pos == 0 */
  int64_t hits[DCNR_GROUP_MAX_K]; /* positives at rank <= ks[j] */
  double dcg[DCNR_GROUP_MAX_K];   /* sum of discount[r - 1] over positives at rank r <= ks[j] */
} dcnr_group_record;

typedef struct {          /* 216 bytes */
  int64_t n;
  int64_t n_groups_present; /* groups with n_u > 0 */
  int64_t n_groups_auc;     /* groups with P_u N_u > 0 (the AUC groups) */
  int64_t n_groups_ranked;  /* groups with P_u >= 1 (the ranked groups) */
  int64_t n_rows_auc;       /* sum of n_u over the AUC groups */
  int64_t n_bad_label;      /* labels that are neither 0.0f nor 1.0f */
  int64_t n_nan;            /* NaN logits */
  int64_t n_bad_group;      /* group ids outside [0, n_groups) */
  int64_t hit_groups[DCNR_GROUP_MAX_K]; /* ranked groups with hits[j] > 0 */
  double gauc;              /* sum of n_u AUC_u over the AUC groups / n_rows_auc,
                               AUC_u = (double)auc_u2 / (2.0 * P_u * N_u) */
  double auc_macro;         /* mean of AUC_u over the AUC groups */
  double mrr;               /* mean of 1.0 / first_pos_rank over the ranked groups */
  double hit_rate[DCNR_GROUP_MAX_K]; /* hit_groups[j] / n_groups_ranked */
  double recall[DCNR_GROUP_MAX_K];   /* mean of hits[j] / P_u over the ranked groups */
  double ndcg[DCNR_GROUP_MAX_K];     /* mean of dcg[j] / ideal[min(ks[j], P_u) - 1], likewise */
} dcnr_group_summary;     /* a mean over zero groups, and entries j >= n_k, are NaN (counts 0) */

/* Workspace bytes of dcnr_eval_group_metrics (0 for n <= 0): it depends on n
 * and on the number of sort passes p = ceil((32 + bits(n_groups - 1)) / 11)
 * (3 for one group, 6 at n_groups = 2^31 - 1; bits(v) = the length of v in
 * binary), not on the value of n_groups:
 *   16 n + 4 * 2048 * (p + U) + 32 + 552 * A   (+ < 2 KiB of alignment),
 * U and A as for dcnr_eval_metrics_workspace_size. */
size_t dcnr_eval_group_metrics_workspace_size(int64_t n, int64_t n_groups);

/* groups[i] in [0, n_groups) is row i's group.  ks: n_k (0..DCNR_GROUP_MAX_K)
 * cutoffs on the HOST, each in [1, 2^20], strictly ascending.  discount and
 * ideal: device arrays of ks[n_k - 1] doubles, discount[i] = 1 / log2(i + 2)
 * and ideal[i] = discount[0] + ... + discount[i] (not read when n_k = 0):
 * the caller's doubles, so the device takes no logarithm.  per_group: NULL,
 * or n_groups records, every one written.  0 <= n < 2^31,
 * 1 <= n_groups <= 2^31 - 1; anything else is DCNR_BAD_ARG before any launch.
 * n = 0 writes a zeroed summary with NaN means (and zeroed records) and
 * reads neither input nor workspace.
 *
 * One radix sort of the keys (group, descending logit) with the label riding
 * along puts every group's list in served order; a segmented walk over it
 * gives the records.  Every integer is exact.  Every fp64 sum (a group's DCG,
 * the means) is taken in an order that depends only on where the groups fall
 * in the sorted rows, with no floating-point atomics: the same input gives
 * the same bits.  NaN logits, labels other than 0 / 1 and group ids out of
 * range are counted; the metrics of such an input are unspecified (the
 * Python layer raises), but no such row indexes per_group or anything else
 * out of bounds: a row with a bad id belongs to no group. */
dcnr_status dcnr_eval_group_metrics(const float* logits, const float* labels, const int64_t* groups,
                                    int64_t n, int64_t n_groups, const int32_t* ks, int32_t n_k,
                                    const double* discount, const double* ideal,
                                    dcnr_group_summary* out, dcnr_group_record* per_group, void* ws,
                                    size_t ws_bytes, dcnr_stream_t stream);

/* List metrics: what R served lists look like, read where the batched serving
 * calls left them (the out_rows / offsets / out_count of
 * dcnr_requests_rank_mmr), with no read-back.  List r is
 * rows[offsets[r] .. offsets[r] + counts[r]); its first m_r = min(counts[r],
 * at) positions are measured.  Both structs are written to DEVICE memory,
 * stream-ordered. */
typedef struct {          /* one list; 112 bytes; all zero for a list that is skipped */
  int64_t m;              /* measured positions */
  int64_t n_rel;          /* size of the list's held-out set */
  int64_t first_hit_rank; /* 1-based position of the first held-out row, 0 for none */
  int64_t hits[DCNR_GROUP_MAX_K]; /* held-out rows at positions <= ks[j] */
  double pair_cos_sum;    /* sum over i < j < m of cos(e_i, e_j): each cosine in fp32 from
                             table and inv_norms as given, the sum in fp64, fixed order */
  double score_sum;       /* sum of scores over the m positions (0 without scores) */
  double info_sum;        /* sum of info[row] over the m positions (0 without info) */
  double dcg[DCNR_GROUP_MAX_K];   /* sum of discount[p] over held-out rows at position p < ks[j] */
} dcnr_list_record;

typedef struct {          /* 248 bytes */
  int64_t n_lists;        /* R */
  int64_t n_lists_scored; /* measured lists with m >= 1 */
  int64_t n_lists_pairs;  /* measured lists with m >= 2 */
  int64_t n_marked;       /* lists whose segment begins with row -1 (the "whole answer
                             marked" of dcnr_requests_rank_mmr, which also sets the count
                             to 0): skipped */
  int64_t n_bad_list;     /* an offset or count outside [0, n], beyond its segment or not
                             monotone, held-out offsets outside their CSR, or one of the m rows
                             >= n_items or < 0 (a -1 behind the first position too): skipped */
  int64_t n_entries;      /* sum of m over the measured lists */
  int64_t n_distinct_items; /* items in at least one measured position */
  int64_t gini_num;       /* sum over i = 1 .. n_items of (2 i - n_items - 1) c_(i), c_(i) the
                             items' exposure counts ascending, the zeros included */
  int64_t n_rel_lists;    /* measured lists with n_rel > 0 */
  int64_t hit_lists[DCNR_GROUP_MAX_K]; /* of those, lists with hits[j] > 0 */
  double ild;             /* mean over the lists with m >= 2 of 1 - pair_cos_sum / (m (m - 1) / 2) */
  double mean_score;      /* sum of score_sum / n_entries (NaN without scores) */
  double mean_info;       /* sum of info_sum / n_entries (NaN without info) */
  double mrr;             /* mean over the n_rel_lists of 1 / first_hit_rank (0 for no hit) */
  double coverage;        /* n_distinct_items / n_items */
  double gini;            /* gini_num / (n_items * n_entries) */
  double hit_rate[DCNR_GROUP_MAX_K]; /* hit_lists[j] / n_rel_lists */
  double recall[DCNR_GROUP_MAX_K];   /* mean of hits[j] / n_rel over the n_rel_lists */
  double ndcg[DCNR_GROUP_MAX_K];     /* mean of dcg[j] / ideal[min(ks[j], n_rel) - 1], likewise */
} dcnr_list_summary;      /* a mean over nothing, and entries j >= n_k, are NaN (counts 0) */

/* Workspace bytes of dcnr_eval_list_metrics: the exposure counts (4 n_items),
 * the count-of-counts histogram (4 (R + 1)), a few words and the workgroups'
 * partial sums (< 400 KiB); the call clears what it needs on the stream.  0
 * for R <= 0, n_items < 1 and shapes the call rejects. */
size_t dcnr_eval_list_metrics_workspace_size(int64_t R, int64_t n_items);

/* rows int64 [n], offsets int64 [R + 1], counts int32 [R] or NULL (whole
 * segments), all on the device; at in 1..128.  table fp32 [n_items][d] with
 * inv_norms [n_items] is the pair dcnr_requests_rank_mmr takes, d in 1..256;
 * a cosine is the fp32 dot of the two rows, each times its inverse norm as
 * given (a zero-norm row's cosines are whatever its inv_norms entry makes
 * them).  scores fp32 [n] (the logits beside the rows) or NULL; info fp64
 * [n_items] (a per-item weight) or NULL.  The held-out sets or NULLs:
 * rel_rows int64 [n_rel_rows] with rel_offsets [R + 1], each set ascending
 * and distinct.  ks: n_k (0..DCNR_GROUP_MAX_K) cutoffs on the HOST, strictly
 * ascending, each in [1, at]; discount and ideal as for
 * dcnr_eval_group_metrics (ks[n_k - 1] doubles; read only with held-out
 * sets).  per_list: NULL or R records, every one written.
 *
 * DCNR_BAD_ARG (R, n or n_rel_rows < 0, n_items < 1, at or d out of range, bad
 * ks, a null pointer that is needed), DCNR_UNSUPPORTED_SHAPE (n > 2^30,
 * n_items >= 2^31, R > 2^22: inside these every partial sum of gini_num is
 * below n_entries * 2^32 < 2^63) and DCNR_WORKSPACE_TOO_SMALL come before any
 * launch.  R = 0 writes a summary of zeros with NaN means (coverage 0) and
 * reads nothing else.  No state outside ws and stream.  The exposure counts
 * and every other integer are exact and independent of the order of
 * execution; every fp64 sum is taken in an order fixed by (R, at): the same
 * input gives the same bytes in the summary and in every record.  Every index
 * is checked against a length passed by value: a bad list is counted and
 * skipped, the other lists are unaffected. */
dcnr_status dcnr_eval_list_metrics(const int64_t* rows, int64_t n, const int64_t* offsets,
                                   const int32_t* counts, int64_t R, int32_t at,
                                   const float* table, const float* inv_norms, int32_t d,
                                   int64_t n_items, const float* scores, const double* info,
                                   const int64_t* rel_rows, int64_t n_rel_rows,
                                   const int64_t* rel_offsets, const int32_t* ks, int32_t n_k,
                                   const double* discount, const double* ideal,
                                   dcnr_list_summary* out, dcnr_list_record* per_list, void* ws,
                                   size_t ws_bytes, dcnr_stream_t stream);

/* One torch.optim.AdamW (decoupled = 1) or Adam (decoupled = 0) step over
 * n_tensors tensors (host arrays of device pointers + element counts).
 * `step` is the 1-based step number after increment (torch's state['step']). */
dcnr_status dcnr_adam_step(int32_t n_tensors, float* const* params, const float* const* grads,
                           float* const* exp_avg, float* const* exp_avg_sq, const int64_t* numel,
                           float lr, float beta1, float beta2, float eps, float weight_decay,
                           int64_t step, int decoupled, dcnr_stream_t stream);

/* dcnr_adam_step over gradients some of whose rows are not stored (ABI 4,
 * the same step, train.py:201-204, 226): tensor i with row_map[i] != NULL is
 * [numel[i] / row_width[i]][row_width[i]] and element e's gradient is
 * grads[i][e] where row_map[i][e / row_width[i]] != 0, else exactly 0 (the
 * row is not read) -- bit-identical to dcnr_adam_step on the dense gradient
 * with those rows zeroed.  row_map[i] == NULL: dense.  row_map / row_width are
 * HOST arrays (row_map entries device pointers, e.g. into the DCNR_WS_ROW_MAP
 * of the train workspace, offset to the table's first row). */
dcnr_status dcnr_adam_step_rows(int32_t n_tensors, float* const* params, const float* const* grads,
                                float* const* exp_avg, float* const* exp_avg_sq, const int64_t* numel,
                                const uint8_t* const* row_map, const int32_t* row_width,
                                float lr, float beta1, float beta2, float eps, float weight_decay,
                                int64_t step, int decoupled, dcnr_stream_t stream);

/* 1/||row|| for each row of table [N,d] (0-norm rows -> 1, as sklearn's normalize). */
dcnr_status dcnr_row_inv_norms(const float* table, int64_t N, int32_t d, float* inv_norms,
                               dcnr_stream_t stream);

size_t dcnr_cosine_topk_workspace_size(int64_t N, int64_t Q, int32_t k);

/* k nearest rows of `table` [N,d] to each query [Q,d] by cosine distance
 * dist = clip(1 - <q/|q|, x/|x|>, 0, 2) (fp32), ascending; ties by lower
 * row index.  idx int64 [Q,k], dist fp32 [Q,k].  1 <= k <= min(64, N).
 * Q = 0 returns DCNR_OK without touching the query / output / workspace
 * pointers (which may then be NULL). */
dcnr_status dcnr_cosine_topk(const float* table, const float* inv_norms, int64_t N, int32_t d,
                             const float* queries, int64_t Q, int32_t k, int64_t* idx,
                             float* dist, void* ws, size_t ws_bytes, dcnr_stream_t stream);

/* Fit-time bf16 copy of the normalised table for the batched scan:
 * packed[r][c] = bf16(table[r][c] * inv_norms[r]) (fp32 product, round to
 * nearest even), uint16 [N,d], d % 8 == 0.  Optional: 2 bytes per element
 * resident beside the fp32 table halve the batched (Q >= 16, d = 32 or 64)
 * scan's HBM stream; results are identical with or without it.  Part of
 * NearestNeighbors.fit (main.py:268-270) -- sklearn keeps its own copy of
 * the fitted data there too. */
dcnr_status dcnr_cosine_pack_rows(const float* table, const float* inv_norms, int64_t N, int32_t d,
                                  uint16_t* packed, dcnr_stream_t stream);

/* dcnr_cosine_topk reading `packed` (from dcnr_cosine_pack_rows over the same
 * table, or NULL) for its coarse bf16 scan; same results, same workspace. */
dcnr_status dcnr_cosine_topk_packed(const float* table, const float* inv_norms, const uint16_t* packed,
                                    int64_t N, int32_t d, const float* queries, int64_t Q, int32_t k,
                                    int64_t* idx, float* dist, void* ws, size_t ws_bytes,
                                    dcnr_stream_t stream);

/* The k nearest rows within a row set: dcnr_cosine_topk scoped to a listed
 * subset of the table ("the hotels in this city most like that one"), which
 * the reference approximates by intersecting global neighbours with the city
 * afterwards (main.py:196-203, 209-210).  A call carries G segments of
 * queries: queries [seg_offsets[g], seg_offsets[g+1]) search set seg_set[g]
 * of the CSR (set_rows int64 [n_set_rows], set_offsets int64 [S+1]; rows
 * distinct within a set); seg_set[g] < 0 skips the segment.  All of these
 * live on the device; max_set_rows is a host bound on the longest set a
 * segment names (it sizes the grid and the workspace).
 *
 * Query q of segment g gets the k rows of its set, other than exclude[q]
 * (int64 [Q] or NULL; -1 or any row outside the set = none), with the
 * smallest cosine distance, ascending by (dist, table row) for an ascending
 * set: idx int64 / dist fp32 [Q][ld], columns [0, k) written, ld >= k.  The
 * queries are raw (normalised inside) and the distance arithmetic is that of
 * every exact scan of dcnr_cosine_topk, so for an ascending set the answer
 * equals dcnr_cosine_topk over the compacted table table[set] with positions
 * mapped back through the set -- the same rows, distances bit for bit (but
 * for that call's fp32-MFMA leg, Q >= 16 with d % 16 == 0 and d not 32 / 64,
 * whose sums run in another order).  In a set that is not ascending, a row
 * tied with the k-th distance that is listed after it may lose to it.
 * Fewer than k eligible rows: the tail is (-1, FLT_MAX), which
 * dcnr_candidate_union and dcnr_requests_candidates skip.  A skipped
 * segment's output rows, a query no segment holds and, with ld > k, the
 * columns outside [0, k) are left untouched: the call overlays answers onto a
 * buffer that holds others.
 *
 * Device data are checked against the lengths passed by value before they are
 * used to address anything: a set index >= S; set offsets outside
 * [0, n_set_rows], decreasing, or longer than max_set_rows; a segment's
 * offsets decreasing or outside [0, Q]; a set row outside [0, N) (found when
 * the row is read: a segment without queries reads none).  Such a segment's
 * queries (those of its range inside [0, Q)) get (-1, FLT_MAX) in all k columns
 * and seg_status[g] (int32 [G] or NULL) = DCNR_REQ_BAD_DATA, else 0; other
 * segments are answered as usual.  Segments that overlap -- possible only
 * beside one with decreasing offsets -- each answer the shared queries, and
 * one of the answers stays.
 *
 * Host-side rejections before any launch: DCNR_BAD_ARG (a null pointer with
 * Q > 0 -- set_rows may be NULL with n_set_rows = 0 --, Q, G, S, n_set_rows or
 * max_set_rows < 0, N < 1, k < 1, ld < k), DCNR_UNSUPPORTED_SHAPE (k > 64,
 * d % 4 != 0, d outside [4, 256], N, n_set_rows, Q or G >= 2^31), then, with
 * Q > 0 and G > 0, DCNR_WORKSPACE_TOO_SMALL below
 * dcnr_cosine_topk_within_workspace_size(Q, k, d, max_set_rows) -- which is 0
 * for a shape the call rejects.  Q = 0 or G = 0 returns DCNR_OK without a
 * launch.  Stream-ordered: three launches, no host synchronisation, no
 * allocation. */
size_t dcnr_cosine_topk_within_workspace_size(int64_t Q, int32_t k, int32_t d, int64_t max_set_rows);
dcnr_status dcnr_cosine_topk_within(const float* table, const float* inv_norms, int64_t N, int32_t d,
                                    const float* queries, int64_t Q, const int64_t* exclude,
                                    const int64_t* seg_offsets, int64_t G, const int32_t* seg_set,
                                    const int64_t* set_rows, int64_t n_set_rows, const int64_t* set_offsets,
                                    int32_t S, int64_t max_set_rows, int32_t k, int64_t ld, int64_t* idx,
                                    float* dist, int32_t* seg_status, void* ws, size_t ws_bytes,
                                    dcnr_stream_t stream);

/* The item neighbour table: the k nearest rows of every row of the fitted
 * table, built once so that /recommendations' candidate step and
 * /similar_items become row lookups (the reference queries its index with rows
 * of the fitted data only: main.py:200 with n_neighbors = 11, main.py:300).
 * For rows [row_lo, row_hi) writes out_idx int32 [row_hi - row_lo][k] and,
 * unless NULL, out_dist fp32 of the same shape.  Row r holds exactly what
 * dcnr_cosine_topk_packed returns for the single query table[r]: the k best
 * ascending by (dist, row), the same bits whatever range or piece of a range
 * the row was built in.  The row itself is not treated specially (among
 * duplicate rows it need not be at position 0); callers keep dropping
 * position 0 as main.py:201 does.  1 <= k <= min(64, N), N < 2^31 (else
 * DCNR_BAD_ARG / DCNR_UNSUPPORTED_SHAPE); a range outside 0 <= row_lo <=
 * row_hi <= N is DCNR_BAD_ARG; an empty range returns DCNR_OK without a
 * launch.  The rows are searched in fixed-size chunks of queries read in place
 * from the table; stream-ordered, no host synchronisation; `ws` holds one
 * chunk's scratch (dcnr_cosine_neighbor_table_workspace_size bytes). */
size_t dcnr_cosine_neighbor_table_workspace_size(int64_t N, int32_t k);
dcnr_status dcnr_cosine_neighbor_table(const float* table, const float* inv_norms, const uint16_t* packed,
                                       int64_t N, int32_t d, int32_t k, int64_t row_lo, int64_t row_hi,
                                       int32_t* out_idx, float* out_dist, void* ws, size_t ws_bytes,
                                       dcnr_stream_t stream);

/* The item neighbour table brought up to date, in place, after m rows of
 * the fitted table got new vectors -- `table`, `inv_norms` and `packed` (or
 * NULL) already hold them (dcnr_row_inv_norms / dcnr_cosine_pack_rows over the
 * changed rows give the refit's bits).  Precondition: nbr int32 [N][k] was
 * exact for the table before the change.  Afterwards every row of nbr is what
 * dcnr_cosine_neighbor_table builds from the new table, bit for bit, with work
 * that grows with m: two calls, stream-ordered, no host synchronisation
 * inside either, and one wait of the caller's between them.
 *
 * _update (phases A + B): `changed` is a HOST array int32 [m], ascending,
 * distinct, inside [0, N), m <= 16384 per call (DCNR_UNSUPPORTED_SHAPE above;
 * a larger set is applied as consecutive changes).  One pass over the table
 * finds the rows a change can reach (a changed row in their list, or a
 * changed row at or under their k-th distance: a superset); each of those
 * merges its unchanged entries with the changed rows and either rewrites its
 * own list or joins the re-search list.  counts (device int32 [4]): changed,
 * affected, merged, to re-search; host_counts (or NULL): the same four words
 * stored to pinned host memory when the call's work is done.  research_rows
 * (device int32 [N]): the first counts[3] entries are the rows to search
 * again, the changed rows among them.
 *
 * _rows (phase C): the lists of rows[n] (device int32; a row outside [0, N)
 * is skipped) searched as the build searches them and written to those rows
 * of nbr.  n is the host's copy of counts[3].
 *
 * Both take `ws` of dcnr_cosine_neighbor_table_update_workspace_size(N, d, k,
 * m) bytes (exact; DCNR_WORKSPACE_TOO_SMALL below it; _rows needs the m = 0
 * size at most).  Shapes as dcnr_cosine_neighbor_table, and d % 4 == 0,
 * 4 <= d <= 256.  m == 0 / n == 0 return DCNR_OK without a launch.  A null
 * pointer, m < 0, k outside [1, N], or `changed` not ascending, distinct and
 * in range: DCNR_BAD_ARG, judged on the host before anything is launched. */
size_t dcnr_cosine_neighbor_table_update_workspace_size(int64_t N, int32_t d, int32_t k, int64_t m);
dcnr_status dcnr_cosine_neighbor_table_update(const float* table, const float* inv_norms, const uint16_t* packed,
                                              int64_t N, int32_t d, int32_t k, const int32_t* changed, int64_t m,
                                              int32_t* nbr, int32_t* counts, int32_t* host_counts,
                                              int32_t* research_rows, void* ws, size_t ws_bytes,
                                              dcnr_stream_t stream);
dcnr_status dcnr_cosine_neighbor_table_rows(const float* table, const float* inv_norms, const uint16_t* packed,
                                            int64_t N, int32_t d, int32_t k, const int32_t* rows, int64_t n,
                                            int32_t* nbr, void* ws, size_t ws_bytes, dcnr_stream_t stream);

/* _update without its merge (dcnr.NearestNeighbors.append_rows): phase A alone
 * -- the same kernels -- finds the rows a change can reach, and every one of
 * them joins the re-search list behind the changed rows; nbr is only read.
 * counts: {changed, affected, 0, changed + affected}.  _rows on that list then
 * gives every list that can differ the build's own answer, so the result does
 * not depend on the merge scoring a kept entry to the same last bit as the
 * search did: among 2^20 rows some pair of neighbours lies within one float32
 * step, and there the two need not order alike.  The filter's bound carries a
 * margin (1e-5) far above such a step, so no row a changed row could enter is
 * missed.  Everything else -- arguments, shapes, workspace, errors -- as
 * _update. */
dcnr_status dcnr_cosine_neighbor_table_affected(const float* table, const float* inv_norms, const uint16_t* packed,
                                                int64_t N, int32_t d, int32_t k, const int32_t* changed, int64_t m,
                                                const int32_t* nbr, int32_t* counts, int32_t* host_counts,
                                                int32_t* research_rows, void* ws, size_t ws_bytes,
                                                dcnr_stream_t stream);

/* Merge of row-sharded top-k lists (the cfg5 index split over ranks, SURVEY
 * 8(e)): dist fp32 / idx int64 [lists][Q][k] (global rows; padding entries
 * (FLT_MAX, -1) sort last) -> the k best per query, ascending by (dist, row),
 * the order dcnr_cosine_topk gives over the whole table.  lists * k <= 2048.
 * Replaces nothing in the reference (one sklearn index per process,
 * main.py:268-270); the single-index result is reproduced exactly. */
dcnr_status dcnr_topk_merge(const float* dist, const int64_t* idx, int32_t lists, int64_t Q,
                            int32_t k, int64_t* out_idx, float* out_dist, dcnr_stream_t stream);

/* Batch assembly of a device-resident dataset (TensorDataset + DataLoader,
 * train.py:195-196): for each of n_arrays (<= 8) arrays of n_src rows of
 * row_bytes[a] bytes (a multiple of 4), dst[a] row i = src[a] row idx[i]
 * (idx clamped to [0, n_src)).  Host arrays of device pointers. */
dcnr_status dcnr_gather_rows(const int64_t* idx, int64_t n, int64_t n_src, int32_t n_arrays,
                             const void* const* src, void* const* dst, const int64_t* row_bytes,
                             dcnr_stream_t stream);

/* ---- serving: the steps either side of scoring in /recommendations ----
 * All operate on at most 4096 items per call (DCNR_UNSUPPORTED_SHAPE above). */

/* Candidate set of _generate_candidates (main.py:196-203): the union of
 * positives[Q] (embedding rows of the positive hotels) and, for each, the
 * neighbour rows knn_idx[q][1..k-1] (the dcnr_cosine_topk output for
 * n_neighbors = k, position 0 dropped as main.py:201 does); negative rows are
 * skipped.  out_rows: the distinct rows ascending; out_count[0] (device
 * int32) = their number.  Q*k <= 4096. */
dcnr_status dcnr_candidate_union(const int64_t* positives, int64_t Q, const int64_t* knn_idx,
                                 int32_t k, int64_t* out_rows, int32_t* out_count,
                                 dcnr_stream_t stream);

/* dcnr_candidate_union reading the neighbours from the item neighbour table
 * (dcnr_cosine_neighbor_table): nbr int32 [n_items][kt], kt >= k; the
 * neighbours of positive p are nbr[p][1 .. k).  The same rows as
 * dcnr_candidate_union over knn_idx[q] = nbr[positives[q]][0 .. k).  Negative
 * positives are skipped, their neighbours with them; a positive >= n_items or a table entry outside
 * [0, n_items) is never followed and sets out_count[0] = -1. */
dcnr_status dcnr_candidate_union_table(const int64_t* positives, int64_t Q, const int32_t* nbr,
                                       int32_t kt, int64_t n_items, int32_t k, int64_t* out_rows,
                                       int32_t* out_count, dcnr_stream_t stream);

/* Ranking batch of preprocess_for_ranking (main.py:215-230) for one user:
 * user_ids[i] = user_row, item_ids[i] = item_rows[i], and the item's
 * categorical codes / scaled numeric features gathered from per-item tables
 * item_cat [n_items][n_cat] (int64) and item_num [n_items][n_num] (fp32). */
dcnr_status dcnr_ranking_batch(const int64_t* item_rows, int64_t n, int64_t user_row,
                               const int64_t* item_cat, int32_t n_cat, const float* item_num,
                               int32_t n_num, int64_t n_items, int64_t* user_ids,
                               int64_t* item_ids, int64_t* cat_features, float* num_features,
                               dcnr_stream_t stream);

/* order[i] = index of the i-th highest score; equal scores keep input order
 * (Python's stable sorted(..., reverse=True), main.py:325).  n <= 4096. */
dcnr_status dcnr_rank_by_score(const float* scores, int64_t n, int64_t* order,
                               dcnr_stream_t stream);

/* rerank_with_mmr (main.py:133-169) over n candidates given in ranked order:
 * rows[i] = embedding row of candidate i in `table` [., d] (-1: no embedding),
 * scores[i] its score.  Writes out_pos[0 .. top_k) = positions (into the ranked
 * list) of the re-ranked items, -1 padded; out_count[0] (device int32) = their
 * number.  Cosine similarity via inv_norms (dcnr_row_inv_norms). */
dcnr_status dcnr_mmr_rerank(const float* table, const float* inv_norms, int32_t d,
                            const int64_t* rows, const float* scores, int64_t n,
                            float lambda_param, int32_t top_k, int64_t* out_pos,
                            int32_t* out_count, dcnr_stream_t stream);

/* ---- serving, a batch of R requests in one pass (main.py:309-332 for each) ----
 * The same steps over CSR-style segments, one workgroup per request, so that
 * R requests cost one top-k call, one launch per step, one forward over all
 * their candidates and ONE host wait (for the forward's batch size).  Per
 * request the results are exactly those of the single-request calls above.
 *
 *   cosine_topk over all requests' positives  (Q_total queries, k neighbours)
 *   dcnr_requests_candidates     -> cand_rows [R][cap], count, status, offsets
 *   (host: wait, n = offsets[R] from the pinned mirror)
 *   dcnr_requests_ranking_batch  -> the forward's inputs for the n rows
 *   dcnr_forward (eval)          -> logits [n]
 *   dcnr_requests_rank_mmr       -> ranked rows / logits per segment
 *
 * Row sets (a city's hotels, its most reviewed hotels, a user's negative
 * reviews ...) are one CSR of S sets, set_rows [n_set_rows] with set_offsets
 * [S + 1], each set ascending and distinct; a request names its allowed,
 * excluded and fallback set by index (int32 [R], -1 = none; a NULL array =
 * none for every request).  An allowed set that is empty allows nothing.
 *
 * status [R] (device int32) bits: */
#define DCNR_REQ_OVERFLOW 1  /* the request's staged list (Q_r * k entries), its union (before
                                or after the fallback) or its result exceeds 4096 rows, or the
                                result exceeds cap: count 0; serve it with the single calls */
#define DCNR_REQ_BAD_DATA 2  /* offsets not monotone or outside [0, Q_total] / [0, n]; a set
                                index >= S or set offsets outside the CSR; a positive,
                                neighbour or set row >= n_items (a set row < 0); top_k < 1;
                                a logit of -inf or NaN (it has no rank): count 0.  No access is made outside the buffers: every index
                                is checked against a length passed by value */
/* Other requests of the batch are unaffected by one that overflows or has bad
 * data.  Argument errors are rejected before any launch: DCNR_BAD_ARG (R < 0,
 * k < 1, cap outside 1..4096, d outside 1..256, a null pointer with R > 0),
 * DCNR_UNSUPPORTED_SHAPE (R > 2^22, k > 64, n_set_rows >= 2^31),
 * DCNR_WORKSPACE_TOO_SMALL.  R = 0 returns DCNR_OK without a launch. */

/* Workspace bytes of dcnr_requests_rank_mmr: each request's ranked rows and
 * logits, 12 * R * cap (+ alignment); 0 for R <= 0 or arguments the calls
 * reject.  Q_total and k are validated only: the union is staged in LDS. */
size_t dcnr_requests_workspace_size(int64_t R, int64_t Q_total, int32_t k, int32_t cap);

/* Candidates of every request: request r owns positives[pos_offsets[r] ..
 * pos_offsets[r + 1]) and the matching rows of knn_idx [Q_total][k].  In order:
 * the union of dcnr_candidate_union; if it has fewer than min_candidates rows
 * and the request names a fallback set, that set joined in (distinct rows
 * ascending, as torch.unique(cat) gives); rows outside its allowed set and
 * rows in its excluded set dropped.  out_rows [R][cap]: the surviving rows
 * ascending in row r's slot; out_count [R]; status [R] (written, see above).
 * Then offsets [R + 1] = the exclusive sum of out_count in request order, also
 * stored to host_offsets, and status to host_status [R] (pinned, device-visible
 * host memory, or NULL), with system-scope stores: valid on the host once the
 * stream has reached here. */
dcnr_status dcnr_requests_candidates(const int64_t* positives, const int64_t* pos_offsets,
                                     int64_t R, int64_t Q_total, const int64_t* knn_idx, int32_t k,
                                     const int64_t* set_rows, int64_t n_set_rows,
                                     const int64_t* set_offsets, int32_t S, const int32_t* allowed,
                                     const int32_t* excluded, const int32_t* fallback,
                                     int32_t min_candidates, int64_t n_items, int32_t cap,
                                     int64_t* out_rows, int32_t* out_count, int32_t* status,
                                     int64_t* offsets, int64_t* host_offsets,
                                     int32_t* host_status, dcnr_stream_t stream);

/* dcnr_requests_candidates reading the neighbours from the item neighbour
 * table nbr int32 [n_items][kt], kt >= k (DCNR_BAD_ARG otherwise): the
 * neighbours of a positive p are nbr[p][1 .. k), and no top-k call precedes
 * this one.  Everything else as above.  A positive >= n_items or a table entry
 * outside [0, n_items) (a negative one too) is DCNR_REQ_BAD_DATA for that
 * request; a negative positive is skipped, its neighbours with it. */
dcnr_status dcnr_requests_candidates_table(const int64_t* positives, const int64_t* pos_offsets,
                                           int64_t R, int64_t Q_total, const int32_t* nbr, int32_t kt,
                                           int32_t k, const int64_t* set_rows, int64_t n_set_rows,
                                           const int64_t* set_offsets, int32_t S,
                                           const int32_t* allowed, const int32_t* excluded,
                                           const int32_t* fallback, int32_t min_candidates,
                                           int64_t n_items, int32_t cap, int64_t* out_rows,
                                           int32_t* out_count, int32_t* status, int64_t* offsets,
                                           int64_t* host_offsets, int32_t* host_status,
                                           dcnr_stream_t stream);

/* dcnr_ranking_batch over the compacted batch of n = offsets[R] rows: row i
 * belongs to the request r whose segment [offsets[r], offsets[r + 1]) holds
 * it, its item is cand_rows[r][i - offsets[r]], its user user_rows[r]. */
dcnr_status dcnr_requests_ranking_batch(const int64_t* cand_rows, int32_t cap,
                                        const int64_t* offsets, int64_t R, int64_t n,
                                        const int64_t* user_rows, const int64_t* item_cat,
                                        int32_t n_cat, const float* item_num, int32_t n_num,
                                        int64_t n_items, int64_t* user_ids, int64_t* item_ids,
                                        int64_t* cat_features, float* num_features,
                                        dcnr_stream_t stream);

/* dcnr_rank_by_score, then (lambda_param[r] < 1) dcnr_mmr_rerank with
 * top_k[r], of every request's segment of logits [n]; rows of `table`
 * [n_items][d] are the candidates themselves (cand_rows; a row < 0 has no
 * embedding).  The ranked rows and their logits are written from the start
 * of the request's segment of out_rows / out_logits [n]: out_count[r] of
 * them, the whole segment when lambda_param[r] >= 1, at most min(top_k[r],
 * segment length) otherwise.  status [R] must hold what
 * dcnr_requests_candidates wrote (or zeros): DCNR_REQ_BAD_DATA is OR-ed in.
 * A request whose logits hold -inf or NaN, or whose MMR meets a row >= n_items,
 * also gets its whole segment of out_rows set to -1 and of out_logits to NaN,
 * so a caller that derives the counts itself and reads nothing back (the
 * Python layer) cannot take unwritten memory for an answer. */
dcnr_status dcnr_requests_rank_mmr(const float* logits, int64_t n, const int64_t* cand_rows,
                                   int32_t cap, const int64_t* offsets, int64_t R,
                                   const float* table, const float* inv_norms, int32_t d,
                                   int64_t n_items, const float* lambda_param,
                                   const int32_t* top_k, int64_t* out_rows, float* out_logits,
                                   int32_t* out_count, int32_t* status, void* ws, size_t ws_bytes,
                                   dcnr_stream_t stream);

/* ---- serving, the large lane: the requests of a batch above the 4096-row capacity ----
 * A request whose bound need = (its positives) * k + (its fallback set's rows)
 * is at most 4096 can never be DCNR_REQ_OVERFLOW in the calls above; the L
 * requests above that go through these calls in the same pass, before the
 * same ONE wait.  All L are processed together, every step a grid over their
 * entries (a stable radix sort of (lane, row) keys, flags, a tiled scan: no
 * atomic decides a position), so there is no capacity but the workspace and
 * DCNR_REQ_OVERFLOW is never set.  Lane l serves request large_req[l] (int32
 * [L], each in [0, R)) of the batch: its positives, set indices and user are
 * read at that index of the batch's own arrays.  The calls take lanes of any
 * size, the small ones included, and give the bits the calls above give.
 *
 *   dcnr_requests_large_candidates     -> cand_rows [offsets[L]] compact, offsets,
 *                                         count, status
 *   (host: the batch's one wait; n = offsets[L] from the pinned mirror)
 *   dcnr_requests_large_ranking_batch  -> the forward's inputs for the n rows
 *   dcnr_forward (eval)                -> logits [n]
 *   dcnr_requests_large_rank_mmr       -> ranked rows / logits per segment
 *
 * Argument errors come before any launch: DCNR_BAD_ARG (a negative length,
 * k < 1, kt < k, d outside 1..256, a null pointer with L > 0),
 * DCNR_UNSUPPORTED_SHAPE (L > 2^22, more than 2^30 entries, k > 64,
 * n_set_rows >= 2^31, n_items > 2^38), DCNR_WORKSPACE_TOO_SMALL.  L = 0 returns
 * DCNR_OK without a launch. */

/* Workspace bytes of dcnr_requests_large_candidates and
 * dcnr_requests_large_rank_mmr for L lanes of n_staged entries in all (the
 * larger of the two: 24 bytes per entry and the sort's counts for the
 * candidates, 49 per entry for rank + MMR, + alignment); 0 for L <= 0 or
 * arguments the calls reject. */
size_t dcnr_requests_large_workspace_size(int64_t L, int64_t n_staged);

/* Candidates of the L large requests.  stage_offsets [L + 1] (device) splits
 * [0, n_staged) into the lanes' bounds: lane l stages stage_offsets[l + 1] -
 * stage_offsets[l] = need entries -- each positive of its request, the
 * positive's neighbours knn_idx[q][1 .. k) (nbr == NULL; knn_idx [Q_total][k]
 * as dcnr_requests_candidates takes it) or nbr[p][1 .. k) (the item neighbour
 * table int32 [n_items][kt], kt >= k), and every row of its fallback set.
 * Negative positives and neighbours are skipped.  Then, per request, what
 * dcnr_requests_candidates does: the distinct rows; those the fallback alone
 * brought kept iff the union has fewer than min_candidates rows; the allowed /
 * excluded filters.  out_rows [n_staged]: the surviving rows, ascending per
 * request, the requests' segments one behind the other; offsets [L + 1],
 * out_count [L], status [L] (written: 0 or DCNR_REQ_BAD_DATA -- a request index
 * outside [0, R), offsets outside [0, Q_total], a set index or set offsets
 * outside the CSR, a bound that is not the request's need, a positive,
 * neighbour or set row >= n_items, for that lane alone; stage_offsets that do
 * not rise from 0 to n_staged, for every lane).  offsets and status are also
 * stored to host_offsets [L + 1] / host_status [L] (pinned, or NULL) with
 * system-scope stores. */
dcnr_status dcnr_requests_large_candidates(
    const int64_t* positives, const int64_t* pos_offsets, int64_t R, int64_t Q_total,
    const int64_t* knn_idx, const int32_t* nbr, int32_t kt, int32_t k, const int64_t* set_rows,
    int64_t n_set_rows, const int64_t* set_offsets, int32_t S, const int32_t* allowed,
    const int32_t* excluded, const int32_t* fallback, int32_t min_candidates, int64_t n_items,
    const int32_t* large_req, const int64_t* stage_offsets, int64_t L, int64_t n_staged,
    int64_t* out_rows, int32_t* out_count, int32_t* status, int64_t* offsets, int64_t* host_offsets,
    int32_t* host_status, void* ws, size_t ws_bytes, dcnr_stream_t stream);

/* dcnr_requests_ranking_batch over the large lane's compact rows: row i of
 * cand_rows [n] belongs to the lane l whose segment [offsets[l], offsets[l + 1])
 * holds it; its user is user_rows[large_req[l]] (user_rows [R]; an index
 * outside [0, R) is clamped into it, as the item row is into the tables). */
dcnr_status dcnr_requests_large_ranking_batch(const int64_t* cand_rows, const int64_t* offsets,
                                              int64_t L, int64_t n, const int32_t* large_req,
                                              int64_t R, const int64_t* user_rows,
                                              const int64_t* item_cat, int32_t n_cat,
                                              const float* item_num, int32_t n_num, int64_t n_items,
                                              int64_t* user_ids, int64_t* item_ids,
                                              int64_t* cat_features, float* num_features,
                                              dcnr_stream_t stream);

/* dcnr_requests_rank_mmr over the large lane's segments of logits [n] and
 * cand_rows [n]: lambda_param and top_k are [L], one per lane.  The rank is a
 * stable radix sort of (lane, -logit), so equal logits keep their order; the
 * MMR runs one workgroup per lane, its per-candidate state in LDS up to 4096
 * candidates and in the workspace above -- the arithmetic and its order are
 * those of dcnr_mmr_rerank, hence the same picks.  Results, counts, status and
 * the marking of a request whose logits hold -inf or NaN as
 * dcnr_requests_rank_mmr; offsets that do not rise from 0 within [0, n] are
 * DCNR_REQ_BAD_DATA for every lane.  ws: dcnr_requests_large_workspace_size(L, n)
 * bytes. */
dcnr_status dcnr_requests_large_rank_mmr(const float* logits, int64_t n, const int64_t* cand_rows,
                                         const int64_t* offsets, int64_t L, const float* table,
                                         const float* inv_norms, int32_t d, int64_t n_items,
                                         const float* lambda_param, const int32_t* top_k,
                                         int64_t* out_rows, float* out_logits, int32_t* out_count,
                                         int32_t* status, void* ws, size_t ws_bytes,
                                         dcnr_stream_t stream);

/* dcnr_mmr_rerank for any n up to 2^30: the per-candidate state lives in ws
 * (dcnr_mmr_rerank_large_workspace_size(n) bytes, 5 per candidate + alignment;
 * 0 for n <= 0 or above the limit), everything else as dcnr_mmr_rerank: the
 * same arithmetic in the same order, one workgroup.  DCNR_BAD_ARG,
 * DCNR_UNSUPPORTED_SHAPE (n, d outside 1..256) and DCNR_WORKSPACE_TOO_SMALL
 * come before any launch. */
size_t dcnr_mmr_rerank_large_workspace_size(int64_t n);
dcnr_status dcnr_mmr_rerank_large(const float* table, const float* inv_norms, int32_t d,
                                  const int64_t* rows, const float* scores, int64_t n,
                                  float lambda_param, int32_t top_k, int64_t* out_pos,
                                  int32_t* out_count, void* ws, size_t ws_bytes,
                                  dcnr_stream_t stream);

/* ---- serving, requests by user: the reviews and the friend graph on the device ----
 * What /recommendations reads of main_df and friendships_df (get_friends_for_user,
 * main.py:172-178; the positives and negatives of _generate_candidates, main.py:
 * 187-194; the recommended_by lists, main.py:336-351), as two CSRs over the
 * n_reviewers reviewers, in device memory (dcnr.InteractionStore builds them):
 * the friends of a reviewer, distinct and symmetric (the reviewer itself only
 * where a (u, u) pair exists), and the reviews of a reviewer in main_df order. */
typedef struct {
  int64_t n_reviewers;
  const int64_t* friend_offsets; /* [n_reviewers + 1] */
  const int32_t* friend_rows;    /* [n_friend_rows] reviewer indices */
  int64_t n_friend_rows;
  const int64_t* review_offsets; /* [n_reviewers + 1] */
  const int32_t* review_items;   /* [n_reviews] hotel row * 4 + class bits:
                                    1 = rating_overall >= 8, 2 = rating_overall <= 4 */
  const int32_t* review_rows;    /* [n_reviews] the review's row in main_df: >= 0, ascending
                                    inside a reviewer; n_reviews or more once rows were removed */
  int64_t n_reviews;
} dcnr_interactions;

#define DCNR_MODE_FRIENDS 0  /* sources: the reviews of the reviewer's friends */
#define DCNR_MODE_PERSONAL 1 /* sources: the reviewer's own reviews */

/* The positives and negatives of R requests, one workgroup each, in front of
 * dcnr_requests_candidates: request r is reviewer reviewers[r] (-1: an unknown
 * user, no sources) in mode modes[r].  Its distinct positive hotel rows (a
 * source review with rating >= 8) are written ascending to positives
 * [pos_offsets[r] .. pos_offsets[r + 1]), the last repeated up to the segment's
 * end; its distinct negative rows (rating <= 4) likewise to neg_rows
 * [neg_offsets[r] .. neg_offsets[r + 1]), a segment inside [neg_lo, neg_hi):
 * an ascending set, so that neg_rows may be the set_rows of
 * dcnr_requests_candidates and the segment the request's excluded set.  The
 * segment lengths are the caller's bounds of the two counts (the sum over the
 * sources of their distinct positives / negatives): at least the count, zero
 * if and only if the count is.  counts [2 R]: the distinct numbers; status [R]:
 * DCNR_REQ_OVERFLOW when the friends or the sources' review rows exceed 4096
 * (answer it on the host), DCNR_REQ_BAD_DATA when a reviewer, mode, offset,
 * friend or hotel row lies outside the lengths passed by value or a segment
 * length breaks the rule above; either leaves counts 0 and the request's
 * segments filled with -1.  Both are also stored to host_counts / host_status
 * (pinned, device-visible host memory, or NULL) with system-scope stores.
 * DCNR_BAD_ARG / DCNR_UNSUPPORTED_SHAPE (n_items > 2^29, R > 2^22) before any
 * launch; R = 0 returns DCNR_OK. */
dcnr_status dcnr_requests_sources(const dcnr_interactions* store, const int32_t* reviewers,
                                  const int32_t* modes, int64_t R, int64_t n_items,
                                  const int64_t* pos_offsets, int64_t Q_total, int64_t* positives,
                                  const int64_t* neg_offsets, int64_t neg_lo, int64_t neg_hi,
                                  int64_t* neg_rows, int32_t* counts, int32_t* status,
                                  int32_t* host_counts, int32_t* host_status,
                                  dcnr_stream_t stream);

/* The recommended_by lists behind dcnr_requests_rank_mmr: for each of the first
 * out_count[r] positions of request r's segment of out_rows [n], the distinct
 * friends of reviewers[r] (in either mode) who reviewed that hotel with rating
 * >= 8, in the order of their first such review's main_df row.  Result: a CSR
 * over the n positions, by_offsets [n + 1] and by_reviewers [n_list_rows] (the
 * words behind by_offsets[n] are -1); by_count [n] = the list lengths.  lists
 * [n_list_rows] is workspace AND result: request r's reviewers, position by
 * position, from list_offsets[r] on (the rest of its segment -1), a place the
 * host knows without reading by_offsets.  A segment's length is the caller's
 * bound: the sum over the friends of their distinct positives.  status [R]
 * (words of this call): DCNR_REQ_OVERFLOW (friends or their review rows above
 * 4096), DCNR_REQ_BAD_DATA (as above; more reviewers than the segment holds):
 * every list of that request is empty. */
dcnr_status dcnr_requests_recommended_by(const dcnr_interactions* store, const int32_t* reviewers,
                                         int64_t R, int64_t n_items, const int64_t* out_rows,
                                         int64_t n, const int64_t* offsets,
                                         const int32_t* out_count, const int64_t* list_offsets,
                                         int64_t n_list_rows, int32_t* lists, int32_t* by_count,
                                         int64_t* by_offsets, int32_t* by_reviewers,
                                         int32_t* status, dcnr_stream_t stream);

/* A new generation of one of those CSRs with m entries inserted: what
 * dcnr.InteractionStore.append runs per device when reviews or friendships
 * arrive, once for the reviews (n_payloads = 2: review_items, review_rows) and
 * once for the friends (n_payloads = 1).  The old generation, old_offsets
 * [n_old_owners + 1] and old_payloads[w] [n_old_entries], is read only and
 * never an output: kernels on other streams may still read it.  The batch, in
 * device memory, prepared by the host from the batch alone: the t touched
 * owners, ascending and distinct, in [0, n_new_owners); insert_prefix [t + 1],
 * the exclusive sums of their insert counts (each >= 1; insert_prefix[t] = m);
 * and for each inserted entry, grouped by owner in that order, insert_pos: its
 * position inside the owner's NEW segment, ascending within the owner, and
 * insert_payloads[w]: its values.  Written: new_offsets [n_new_owners + 1] and
 * new_payloads[w] [n_old_entries + m]; owners at or beyond n_old_owners start
 * from n_old_entries.  Every output element is written exactly once by one
 * lane, without atomics: the same bits on every run.  All positions are 64-bit.
 * Workgroups take DCNR_CSR_INSERT_CHUNK output elements at a time.
 * With m = 0 only new_offsets is written (the payloads of the new generation
 * are the old ones; the payload arguments may be NULL); with m = 0 and
 * n_new_owners = n_old_owners nothing is launched.  DCNR_BAD_ARG before any
 * launch: a null or negative argument, n_payloads outside 1..2, n_new_owners <
 * n_old_owners, t > m, or t = 0 with m > 0. */
#define DCNR_CSR_INSERT_CHUNK 4096
dcnr_status dcnr_csr_insert(const int64_t* old_offsets, int64_t n_old_owners, int64_t n_new_owners,
                            int64_t n_old_entries, int32_t n_payloads,
                            const int32_t* const* old_payloads, const int64_t* touched,
                            const int64_t* insert_prefix, int64_t t, const int64_t* insert_pos,
                            const int32_t* const* insert_payloads, int64_t m, int64_t* new_offsets,
                            int32_t* const* new_payloads, dcnr_stream_t stream);

/* The mirror of dcnr_csr_insert: a new generation of one of those CSRs with m
 * entries taken out, what dcnr.InteractionStore.remove runs per device when
 * reviews are withdrawn (n_payloads = 2) or reviewers unfriend (n_payloads =
 * 1).  The old generation, old_offsets [n_owners + 1] and old_payloads[w]
 * [n_old_entries], is read only and never an output.  removed [m], in device
 * memory, prepared by the host from the batch alone: the global positions in
 * the old payloads that go, strictly ascending, in [0, n_old_entries).
 * Written: new_payloads[w] [n_old_entries - m], new[p] = old[p + c] with c the
 * smallest value in [0, m] with c == m or removed[c] - c > p (the removed
 * positions in front of the source element), and new_offsets [n_owners + 1],
 * new_offsets[o] = old_offsets[o] - #{i : removed[i] < old_offsets[o]}: the
 * owners stay.  Every output element is written exactly once by one lane,
 * without atomics: the same bits on every run.  All positions are 64-bit, and
 * every index taken from device data is clamped into its array: a malformed
 * removed list gives unspecified values, never an access outside the buffers.
 * Workgroups take DCNR_CSR_INSERT_CHUNK output elements at a time; a chunk no
 * removed position falls into is a shifted copy.  With m = 0 nothing is
 * launched or written; with m = n_old_entries only new_offsets is written (the
 * payload arguments may be NULL).  DCNR_BAD_ARG before any launch: a needed
 * null pointer, a negative count, n_payloads outside 1..2, or m >
 * n_old_entries.  Stream-ordered; no allocation, no host synchronisation. */
dcnr_status dcnr_csr_remove(const int64_t* old_offsets, int64_t n_owners, int64_t n_old_entries,
                            int32_t n_payloads, const int32_t* const* old_payloads,
                            const int64_t* removed, int64_t m, int64_t* new_offsets,
                            int32_t* const* new_payloads, dcnr_stream_t stream);

/* The row sets a /recommendations request filters by, for every city at once,
 * from the review rows (main.py:204-210): what dcnr.CitySets runs per device
 * when it is uploaded and after every append and remove.  One entry per
 * main_df row, in device memory: review_item [M] the hotel row, in [0,
 * n_items); review_city [M] the dense city code, in [0, n_cities); review_key
 * [M] the row's user_reviews_count (NaN, +-inf, +-0.0 allowed); review_row [M]
 * the row's main_df number, strictly ascending and >= 0 (NULL: the position).
 * With C = n_cities, for every city c:
 *   city c       the distinct hotel rows of the rows with review_city == c
 *   top rows c   the first `top` of those rows by key descending, NaN last,
 *                equal keys (-0.0 equals +0.0) by ascending main_df row: what
 *                sort_values(ascending=False, kind='stable').head(top) gives
 *   popular c    the distinct hotel rows of top rows c
 * Written: one CSR of 2C + 1 sets, each ascending and distinct, in the form
 * dcnr_requests_candidates reads: set c is city c, set C + c is popular c, set
 * 2C is empty (the unknown city); set_offsets [2C + 2], always complete, and
 * set_rows [cap].  top_rows [C][top]: the main_df numbers of top rows c in
 * served order, -1 behind a city's last.  status [1] (written): DCNR_REQ_OVERFLOW
 * if set_offsets[2C + 1] > cap -- nothing is written at or behind set_rows +
 * cap, and the offsets say what cap must be; DCNR_REQ_BAD_DATA for an item or
 * city outside its range or rows that do not ascend -- every index taken from
 * device data is clamped into its array, so the values are then unspecified
 * but no access leaves the buffers.  set_offsets and status are also stored to
 * host_offsets [2C + 2] and host_status [1] (pinned, device-visible host
 * memory, or NULL) with system-scope stores.
 * The rows are sorted twice with the stable radix sort of the metrics, by
 * (city, key) as 16-byte records and by (city, hotel) as 64-bit keys; the rest
 * is one lane per row or one workgroup per city over at most `top` rows, so a
 * city that holds every row costs what any table of M rows costs.  Every count
 * is an integer and every output word is written by one lane: the same bits
 * on every run.  Workspace: dcnr_city_sets_workspace_size bytes, about 32 M +
 * 4 C (top + 5) (+ 8 MB of sort counts at most); 0 for arguments the call
 * rejects.  DCNR_BAD_ARG before any launch: a needed null pointer or a
 * negative argument; DCNR_UNSUPPORTED_SHAPE: top outside 1..256, n_cities
 * outside 1..65536, n_items > 2^29 or M >= 2^31 - 1; DCNR_WORKSPACE_TOO_SMALL.
 * With M = 0 the offsets are zeros and top_rows is -1.  Stream-ordered; no
 * allocation, no host synchronisation. */
size_t dcnr_city_sets_workspace_size(int64_t M, int64_t n_items, int32_t n_cities, int32_t top);
dcnr_status dcnr_city_sets_build(const int32_t* review_item, const int32_t* review_city,
                                 const double* review_key, const int32_t* review_row, int64_t M,
                                 int64_t n_items, int32_t n_cities, int32_t top, int64_t* set_offsets,
                                 int64_t* set_rows, int64_t cap, int32_t* top_rows, int32_t* status,
                                 int64_t* host_offsets, int32_t* host_status, void* ws, size_t ws_bytes,
                                 dcnr_stream_t stream);

/* Every hotel's ranking features from its first main_df row (main.py:315's
 * isin + drop_duplicates(subset=['item_id']), then preprocess_for_ranking,
 * main.py:215-230): what dcnr.ItemFeatures runs per device when it is uploaded
 * and after every append, remove, set_values and set_scaler.  One entry per
 * main_df row, in device memory and in ascending main_df row order:
 * review_item [M] the hotel row, in [0, n_items); review_row [M] the row's
 * main_df number, strictly ascending and >= 0 (NULL: the position);
 * review_cat [M][n_cat] the caller's encoded codes; review_num [M][n_num] the
 * raw column values (anything a double holds).  scaler_scale, scaler_min
 * [n_num]: MinMaxScaler's scale_ and min_, in device memory.
 * Written, for every hotel h (all of every table, whatever the input):
 *   first_row [n_items]        the main_df number of h's first row, -1: none
 *   item_cat [n_items][n_cat]  that row's codes as int64; zeros without a row
 *   item_num [n_items][n_num]  float32(x * scale_ + min_) of that row's values:
 *                              the product and the sum each rounded to float64
 *                              (never an fma), then to float32 to nearest even,
 *                              as MinMaxScaler.transform followed by
 *                              torch.tensor(dtype=float32) gives, bit for bit;
 *                              NaN, +-inf and -0.0 as numpy passes them; zeros
 *                              without a row
 *   counts [2]                 {the hotels with a row, a status word}: the
 *                              status is 0 or DCNR_REQ_BAD_DATA for a
 *                              review_item outside [0, n_items) or a review_row
 *                              that is negative or does not ascend.  Such a row
 *                              names no hotel and nothing is read or written
 *                              outside the buffers; the tables are then those
 *                              of the other rows.  Also stored to host_counts
 *                              [2] (pinned, device-visible host memory, or
 *                              NULL) with system-scope stores.
 * The first row is the smallest position per hotel: an integer atomicMin into
 * an int32 [n_items] scratch, skipped where a plain load shows the slot already
 * lower; then one hotel per lane group gathers its row, and the hotels with a
 * row are counted per workgroup and summed by one.  Every word is an integer
 * or written by one lane: the same bytes on every run.  Workspace:
 * dcnr_item_features_workspace_size bytes, 4 n_items + 8 KiB (+ 512 at most); 0
 * for arguments the call rejects.  DCNR_BAD_ARG before any launch: a needed null pointer (a
 * column or table of width 0 may be NULL, and with M = 0 every column and the
 * workspace) or a negative argument; DCNR_UNSUPPORTED_SHAPE: n_cat or n_num
 * above 64, n_items > 2^29 or M >= 2^31 - 1; DCNR_WORKSPACE_TOO_SMALL.  With
 * M = 0 every first_row is -1 and the tables are zeros.  Stream-ordered; no
 * allocation, no host synchronisation. */
size_t dcnr_item_features_workspace_size(int64_t M, int64_t n_items, int32_t n_cat, int32_t n_num);
dcnr_status dcnr_item_features_build(const int32_t* review_item, const int32_t* review_row,
                                     const int32_t* review_cat, const double* review_num,
                                     const double* scaler_scale, const double* scaler_min, int64_t M,
                                     int64_t n_items, int32_t n_cat, int32_t n_num, int32_t* first_row,
                                     int64_t* item_cat, float* item_num, int32_t* counts,
                                     int32_t* host_counts, void* ws, size_t ws_bytes,
                                     dcnr_stream_t stream);

/* prepare_data on the device: the driver's noise filter and derived columns
 * (train.py:280-287) and prepare_data (train.py:36-65) up to the split, from
 * the raw review columns to the reference's training tensors and preprocessing
 * artifacts, bit for bit (DESIGN.md section 9 has the contract in full; the
 * split itself is a host permutation and two dcnr_gather_rows, dcnr/prepare.py).
 * Inputs, device memory, M rows in main_df order:
 *   user, item [M]        raw ids, any int64
 *   target [M]            uint8, 0 or not 0 (y is 0.0f or 1.0f)
 *   cat_key [M][n_cat]    int64 keys whose numeric order is the categories'
 *                         sorted order; any negative key: the value is missing
 *   raw [M][n_raw]        float64, anything a double holds
 *   filter_col, filter_lo, filter_hi   a row passes when raw[filter_col] >=
 *                         filter_hi or <= filter_lo (NaN fails); -1: no filter
 *   derived [n_derived][3]  HOST memory: {op, i, j} over raw columns, appended
 *                         behind the raw ones in this order.  DCNR_DERIVED_RATIO:
 *                         raw[i] / raw[j], +-inf and NaN become 0;
 *                         DCNR_DERIVED_DIFF: raw[i] - raw[j], NaN stays
 * n_num = n_raw + n_derived.  Over the rows that pass the filter: a numeric
 * NaN becomes its column's median over the non-NaN values of those rows (even
 * count: (v[k/2-1] + v[k/2]) / 2, one add, one halving; all NaN: NaN); rows
 * with a missing category are then dropped.  Over the n surviving rows: user
 * and item codes by first appearance, category codes by rank among the sorted
 * present keys, MinMaxScaler().fit (scale_ = 1 / range, 1 where range < 10
 * DBL_EPSILON; min_ = 0 - data_min_ * scale_) and float32(x * scale_ + min_),
 * the product and the sum each rounded to float64 (never an fma).
 * Outputs, device memory, every row-shaped one with room for M rows:
 *   row [n]               int32: the surviving rows' input positions, ascending
 *   collab [n][2], cat [n][n_cat] (int64), num [n][n_num], y [n] (float32)
 *   user_ids, item_ids [M]  the raw id of every code (n_users, n_items used)
 *   cat_keys [n_cat][M]   per column the sorted present keys
 *   stats [5][n_num]      float64: median, data_min_, data_max_, scale_, min_;
 *                         also stored to host_stats (pinned, or NULL)
 *   counts [DCNR_TRAIN_TABLE_COUNTS + n_cat]  int32: {n, n_users, n_items,
 *                         rows that passed the filter, status}, then each
 *                         category column's cardinality; also stored to
 *                         host_counts (pinned, or NULL) with system-scope
 *                         stores.  The status is 0, or DCNR_REQ_BAD_DATA when a
 *                         surviving, filled value is +-inf (where scikit-learn
 *                         raises); the other outputs are then unspecified, and
 *                         nothing is read or written outside the buffers.
 * The sign of a zero median, data_min_ or data_max_ is unspecified.  Every
 * atomic is an integer one and no atomic decides a position: the same bytes on
 * every run.  Workspace: dcnr_train_table_workspace_size bytes, about
 * M (8 n_num + 41) (0 for arguments the call rejects).  DCNR_BAD_ARG before
 * any launch: a null args, a needed null pointer (a column of width 0 may be
 * NULL, and with M = 0 everything but counts), a negative size, a derived op
 * that is neither, a derived or filter column outside [0, n_raw);
 * DCNR_UNSUPPORTED_SHAPE: M >= 2^31 - 1, n_cat > 64, n_raw + n_derived > 64;
 * DCNR_WORKSPACE_TOO_SMALL.  With M = 0 no kernel is launched: counts is
 * zeroed by a stream-ordered memset and host_counts by the calling thread.
 * Stream-ordered; no allocation, no host synchronisation. */
#define DCNR_DERIVED_RATIO 0
#define DCNR_DERIVED_DIFF 1
#define DCNR_TRAIN_TABLE_COUNTS 5
typedef struct {
  const int64_t* user; const int64_t* item; const uint8_t* target;
  const int64_t* cat_key; const double* raw;
  int64_t M; int32_t n_cat, n_raw;
  int32_t filter_col; double filter_lo, filter_hi;
  int32_t n_derived; const int32_t* derived;
  int32_t* row; int64_t* collab; int64_t* cat; float* num; float* y;
  int64_t* user_ids; int64_t* item_ids; int64_t* cat_keys;
  double* stats; double* host_stats;
  int32_t* counts; int32_t* host_counts;
} dcnr_train_table_args;
size_t dcnr_train_table_workspace_size(int64_t M, int32_t n_cat, int32_t n_raw, int32_t n_derived);
dcnr_status dcnr_train_table_build(const dcnr_train_table_args* args, void* ws, size_t ws_bytes,
                                   dcnr_stream_t stream);

/* A raw-id dictionary on the device (dcnr.IdMap): an open-addressing hash
 * table of `capacity` 16-byte slots {int64 key, int64 index}, capacity a power
 * of two above n, `table` 16-byte aligned device memory of capacity * 16 bytes.
 * The build clears the table, then one lane per id claims a slot (linear
 * probing from a 64-bit mixing hash, a compare-and-swap on the key word, then
 * the index is stored): the index of ids[i] is i.  INT64_MIN marks an empty
 * slot and is no legal id.  status (device int32, also stored to host_status:
 * pinned, or NULL): 0, DCNR_REQ_BAD_DATA for a duplicate or the reserved id,
 * DCNR_REQ_OVERFLOW when a lane found no free slot; the table is then
 * unusable.  The lookup writes out[q] = the index of raw[q], or default_index
 * for an id the table does not hold (the reserved one included); it only
 * reads the table.  Every probe loop ends after `capacity` slots and no lane
 * waits for another.  DCNR_BAD_ARG before any launch: a needed null pointer
 * (ids with n = 0 and raw / out with M = 0 may be NULL), a negative size, a
 * capacity that is no power of two or not above n, a misaligned table;
 * DCNR_UNSUPPORTED_SHAPE: capacity > 2^40.  Stream-ordered; no allocation, no
 * host synchronisation. */
dcnr_status dcnr_id_map_build(const int64_t* ids, int64_t n, void* table, int64_t capacity, int32_t* status,
                              int32_t* host_status, dcnr_stream_t stream);
dcnr_status dcnr_id_map_lookup(const void* table, int64_t capacity, const int64_t* raw, int64_t M,
                               int64_t default_index, int64_t* out, dcnr_stream_t stream);

/* Admit new ids into a built table that holds n (dcnr.IdMap.insert).  raw [M]
 * is any batch: known ids, new ids, duplicates.  out[q] = the index of raw[q]:
 * a known id's own; the distinct new ids are numbered n, n + 1, ... in the order
 * of their first appearance in raw (what enumerate(df[col].unique()) would have
 * given them, train.py:42-43), and new_ids[j] ([M] room) is the id numbered
 * n + j.  Every out[q] is final when the call's work is done, and the table
 * then answers dcnr_id_map_lookup for old and new ids alike.  counts (device
 * int32 [2], also stored to host_counts: pinned, or NULL) = {n_new, status}:
 *   0                  success
 *   DCNR_REQ_BAD_DATA  raw holds the reserved id INT64_MIN: decided by a
 *                      read-only pass before the first compare-and-swap, so
 *                      the table is unchanged, n_new is 0 and out holds the
 *                      plain lookup (-1 for an id the table does not hold)
 *   DCNR_REQ_OVERFLOW  a lane found no free slot: the table is unusable, as
 *                      after a failed build
 * out, new_ids and n_new are the same on every run: the numbering comes from a
 * sum scan over first-appearance marks, never from an atomic.  Which slot a new
 * id lands in depends on which lane wins its probe chain, as in the build; only
 * the table's bytes can differ between runs, never an answer.  Every atomic is
 * an integer one (compare-and-swap, min, or), every probe loop ends after
 * `capacity` slots and no lane waits for another.  The caller keeps
 * n + n_new < capacity (dcnr.IdMap rebuilds a larger table first).  Workspace:
 * dcnr_id_map_insert_workspace_size(M) bytes, about 12 M (0 for an M the call
 * rejects).  DCNR_BAD_ARG before any launch: a needed null pointer (with M = 0,
 * a no-op that zeroes counts, only table and counts are needed), a negative
 * size, a capacity that is no power of two or not above n, a misaligned table;
 * DCNR_UNSUPPORTED_SHAPE: M >= 2^31 - 1 or capacity > 2^40;
 * DCNR_WORKSPACE_TOO_SMALL.  Stream-ordered; no allocation, no host
 * synchronisation. */
size_t dcnr_id_map_insert_workspace_size(int64_t M);
dcnr_status dcnr_id_map_insert(void* table, int64_t capacity, int64_t n, const int64_t* raw, int64_t M,
                               int64_t* out, int64_t* new_ids, int32_t* counts, int32_t* host_counts,
                               void* ws, size_t ws_bytes, dcnr_stream_t stream);

/* A fitted preprocessing applied to rows it was not fitted on (dcnr.Preprocessor
 * .transform; preprocess_for_ranking, main.py:215-230, in train.py's order of
 * steps; DESIGN.md section 9 has the contract in full).  The inputs are those
 * of dcnr_train_table_args, but target may be NULL, and y with it; the fit,
 * device memory unless stated:
 *   user_table, item_table   id maps built over the fit's user_ids / item_ids
 *                            (their capacities; n_users, n_items ids)
 *   cat_keys, cat_offsets    the columns' ascending present keys, one list
 *                            behind the other; cat_offsets [n_cat + 1] HOST
 *   fit [3][n_num]           float64: median_, scale_, min_
 *   fill_nan                 not 0: a NaN numeric (after the derived columns)
 *                            becomes its column's median_; 0: it stays NaN
 *   drop_unknown             0: an unknown user becomes n_users / 2, an
 *                            unknown hotel 0, an unknown or missing (negative)
 *                            category key 0, and the row's bit in unknown_bits
 *                            says so (bit 0 the user, bit 1 the hotel, bit
 *                            2 + c category c); not 0: such rows are left out
 * Rows that fail the filter are left out first; the kept rows keep their input
 * order.  num = float32(x * scale_ + min_), the product and the sum each
 * rounded to float64 (never an fma); y = target != 0.
 * Outputs, device memory, each with room for M rows: row [n] int32 (the input
 * positions kept), collab [n][2], cat [n][n_cat], unknown_bits [n] (int64),
 * num [n][n_num], y [n] (float32).
 *   counts [DCNR_ROWS_TRANSFORM_COUNTS + n_cat]  int32: {n, rows the filter
 *                            removed, rows with an unknown user, with an
 *                            unknown hotel, status}, then per category column
 *                            the rows with an unknown or missing key (all
 *                            counted over the rows that passed the filter);
 *                            also stored to host_counts (pinned, or NULL) with
 *                            system-scope stores.  The status is 0, or
 *                            DCNR_REQ_BAD_DATA when a kept value is +-inf.
 * Every atomic is an integer one and no atomic decides a position: the same
 * bytes on every run.  Workspace: dcnr_rows_transform_workspace_size bytes,
 * about 4 M (0 for arguments the call rejects).  DCNR_BAD_ARG before any
 * launch: a null args, a needed null pointer (a column of width 0 may be NULL,
 * and with M = 0 everything but counts), target without y or y without target,
 * a negative size, a capacity that is no power of two or not above its id
 * count, a misaligned table, offsets that do not start at 0 or descend, a
 * derived op that is neither, a derived or filter column outside [0, n_raw);
 * DCNR_UNSUPPORTED_SHAPE: M >= 2^31 - 1, n_cat > 62, n_raw + n_derived > 64;
 * DCNR_WORKSPACE_TOO_SMALL.  With M = 0 no kernel is launched.  Stream-ordered;
 * no allocation, no host synchronisation. */
#define DCNR_ROWS_TRANSFORM_COUNTS 5
typedef struct {
  const int64_t* user; const int64_t* item; const uint8_t* target;
  const int64_t* cat_key; const double* raw;
  int64_t M; int32_t n_cat, n_raw;
  int32_t filter_col; double filter_lo, filter_hi;
  int32_t n_derived; const int32_t* derived;
  int32_t fill_nan, drop_unknown;
  const void* user_table; int64_t user_capacity, n_users;
  const void* item_table; int64_t item_capacity, n_items;
  const int64_t* cat_keys; const int64_t* cat_offsets;
  const double* fit;
  int32_t* row; int64_t* collab; int64_t* cat; float* num; float* y; int64_t* unknown_bits;
  int32_t* counts; int32_t* host_counts;
} dcnr_rows_transform_args;
size_t dcnr_rows_transform_workspace_size(int64_t M, int32_t n_cat, int32_t n_raw, int32_t n_derived);
dcnr_status dcnr_rows_transform(const dcnr_rows_transform_args* args, void* ws, size_t ws_bytes,
                                dcnr_stream_t stream);

/* The deep tower's Linear layer as a standalone bf16 call (nn.Linear forward,
 * train.py:143,105,109): C[M,N] = X[M,K] . W[N,K]^T + bias, X/W bf16
 * row-major (K, ldx, ldw multiples of 8), C bf16 (out_f32 = 0) or fp32.
 * ldc must be a multiple of 8 where the weight-stationary kernels take the
 * call (K <= 512 and N a multiple of 8: DCNR_UNSUPPORTED_SHAPE otherwise,
 * nothing written); the generic kernel (any other K, N) takes any ldc >= N.
 * Used by the deep tower internally; exported for unit tests and kernel
 * benchmarks. */
dcnr_status dcnr_linear_bf16(const void* X, int64_t ldx, int64_t M, int32_t K, const void* W,
                             int64_t ldw, int32_t N, const float* bias, void* C, int64_t ldc,
                             int out_f32, dcnr_stream_t stream);

/* The deep tower's weight gradient as a standalone bf16 call (backward of
 * nn.Linear, train.py:225): dW[N][K] (fp32) (+)= sum_b dY[b][n] * X[b][k],
 * dY [B][ldy] and X [B][ldx] bf16 row-major (N, K, ldy, ldx multiples of 8).
 * Workspace: dcnr_linear_wgrad_workspace_size bytes.  Used by the deep tower
 * internally; exported for unit tests and kernel benchmarks. */
size_t dcnr_linear_wgrad_workspace_size(int32_t N, int32_t K, int64_t B);
dcnr_status dcnr_linear_wgrad_bf16(const void* dY, int64_t ldy, const void* X, int64_t ldx,
                                   int64_t B, int32_t N, int32_t K, float* dW, int accumulate,
                                   void* ws, size_t ws_bytes, dcnr_stream_t stream);

/* Kernel-timing instrumentation (measurement only, off by default): when
 * enabled, every launch the library makes is bracketed by HIP events on its
 * stream and attributed to one of these classes. */
typedef enum {
  DCNR_K_GATHER_CROSS = 0, /* gather + x0 + cross forward                 */
  DCNR_K_GEMM_FWD = 1,     /* deep-tower Linear forward (MFMA)             */
  DCNR_K_GEMM_DX = 2,      /* deep-tower dX GEMMs (MFMA)                   */
  DCNR_K_GEMM_DW = 3,      /* deep-tower dW split-K GEMMs (MFMA)           */
  DCNR_K_ROWWISE = 4,      /* BN stats/apply, ReLU, dropout, residual      */
  DCNR_K_REDUCE = 5,       /* partial-sum / split-K reductions, BN finalize */
  DCNR_K_CROSS_BWD = 6,    /* cross backward + embedding-grad scatter      */
  DCNR_K_HEAD = 7,         /* head dot, logits, BCE                         */
  DCNR_K_ADAM = 8,         /* fused Adam/AdamW                              */
  DCNR_K_KNN = 9,          /* cosine top-k                                  */
  DCNR_K_PACK = 10,        /* weight packing / zero fills                  */
  DCNR_K_SERVE = 11,       /* candidate union, ranking batch, sort, MMR     */
  DCNR_K_EMB_SORT = 12,    /* embedding-backward stable id sort             */
  DCNR_K_EMB_SUM = 13,     /* embedding-backward per-row segmented sums     */
  DCNR_K_TOWER = 14,       /* fused eval deep tower (one persistent launch) */
  DCNR_K_COUNT = 15
} dcnr_kernel_class;

/* on = 0: off; 1: every launch timed per class with HIP events on its
 * stream (the backward's weight-gradient GEMMs then run on the caller's
 * stream, each launch priced alone); 2: only DCNR_K_GEMM_DW timed, on the
 * side stream where it overlaps the dX chain (its concurrent wall time). */
void dcnr_profile_enable(int on);
/* Synchronises the recorded events and returns, per class, the summed kernel
 * milliseconds and launch counts since the last collect (arrays of n). */
dcnr_status dcnr_profile_collect(double* ms, int64_t* launches, int32_t n);
/* ... plus, per class, the summed ALGORITHMIC bytes of those launches (the
 * operands each function must move: inputs read once, outputs written once;
 * split-K slabs count only in their reduction) -- the numerator of each
 * class's HBM roofline fraction. */
dcnr_status dcnr_profile_collect_bytes(double* ms, int64_t* launches, double* bytes, int32_t n);

/* Synchronises `stream` and reports kernel-side errors recorded in ws
 * (DCNR_INDEX_OOB when DCNR_FLAG_CHECK_INDICES saw an out-of-range id). */
dcnr_status dcnr_check_errors(void* ws, size_t ws_bytes, dcnr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DCNR_H */
