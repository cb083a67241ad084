/* mmt_layer.h -- C ABI of the fused residual-block kernels around the attention core
 * (SURVEY.md 8(f) rank 1).
 *
 * They replace the element-wise chain of etcmodel's `ResidualBlock` / `DenseLayers` as
 * instantiated by `RelativeTransformerLayers` (reference ctor src/modeling/models/mmt_encoder.py:124-135;
 * math SURVEY.md App. A.3, pre-activation order `y = x + Dropout(inner(LayerNorm(x)))`,
 * LayerNorm eps 1e-12, tanh-GELU mmt_encoder.py:53-54), i.e. what TF executes as separate
 * BiasAdd / Dropout / Add / LayerNormalization / Gelu kernels and their gradients.
 *
 * Conventions as in mmt_attn.h: device pointers, caller-owned buffers + workspace, caller's
 * hipStream_t, 0 / negative MMT_E_* return codes, message via mmt_last_error().
 * Activations are [rows, H] row-major in `dtype` (MMT_F32 | MMT_BF16); parameters (bias, gamma,
 * beta) and their gradients are fp32 (master weights); mean / rstd are fp32 [rows].
 * Dropout keeps element (row, col) iff hash(seed, row*H + col) >= p * 2^16 on 16 bits; the
 * backward regenerates the mask from the same seed (nothing is stored).
 */
#ifndef MMT_LAYER_H_
#define MMT_LAYER_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mmt_rows_desc {
  int64_t rows;        /* B * S                                         */
  int32_t H;           /* row length; multiple of 8, <= 8192            */
  int32_t dtype;       /* MMT_F32 | MMT_BF16                            */
  float eps;           /* LayerNorm epsilon (1e-12 in the reference)    */
  float dropout_p;     /* hidden_dropout_prob; 0 disables               */
  uint64_t dropout_seed;
  int32_t accumulate;  /* backward: != 0 adds dbias / dgamma / dbeta INTO the given buffers (fp32
                          master gradients) instead of overwriting them                       */
  int32_t defer_reduce; /* backward: != 0 leaves the column-sum partials in the workspace and does NOT launch
                           the fixed-order reduce; the caller finishes with mmt_colsum_reduce (same desc,
                           same workspace) on a stream of its choice -- the parameter gradients are off the
                           critical path of backward                                                      */
  const uint64_t* dropout_epoch; /* ABI 4: DEVICE uint64 added to dropout_seed by the kernel, or NULL (mmt_attn.h) */
} mmt_rows_desc;

/* Bytes of scratch the *_bwd entry points need (column-sum partials). */
size_t mmt_layer_workspace_bytes(const mmt_rows_desc* desc);

/* y = LayerNorm(x) * gamma + beta; mean, rstd saved for the backward. */
int mmt_ln_fwd(const mmt_rows_desc* desc, const void* x, const float* gamma, const float* beta,
               void* y, float* mean, float* rstd, void* stream);

/* dx, dgamma[H], dbeta[H] of mmt_ln_fwd (dgamma / dbeta are overwritten). */
/* mmt_ln_bwd with a second incoming gradient: dx = dx_in + LayerNormBackward(dy) (dx_in may be NULL) -- the input of
 * the first pre-activation block feeds both its LayerNorm and its residual sum (mmt_encoder.py:124-135); one kernel
 * instead of autograd's extra add over [B*S, H]. */
int mmt_ln_bwd_add(const mmt_rows_desc* desc, const void* dy, const void* x, const float* gamma,
                   const float* mean, const float* rstd, const void* dx_in, void* dx, float* dgamma, float* dbeta,
                   void* workspace, size_t workspace_bytes, void* stream);
int mmt_ln_bwd(const mmt_rows_desc* desc, const void* dy, const void* x, const float* gamma,
               const float* mean, const float* rstd, void* dx, float* dgamma, float* dbeta,
               void* workspace, size_t workspace_bytes, void* stream);

/* Residual block tail + next block's LayerNorm:
 *   x_new = x + Dropout(o + bias);   h = LayerNorm(x_new) * gamma + beta
 * gamma == NULL: no LayerNorm (h, mean, rstd unused) -- the last block of a pre-activation stack. */
int mmt_residual_block_fwd(const mmt_rows_desc* desc, const void* o, const float* bias,
                           const void* x, const float* gamma, const float* beta, void* x_new,
                           void* h, float* mean, float* rstd, void* stream);

/* Backward: dX = dx_new_in + LayerNormBwd(dh);  dx = dX;  do = DropoutBwd(dX);
 * dbias[H] = colsum(do), dgamma, dbeta overwritten.  dx_new_in may be NULL (treated as 0);
 * dh / gamma NULL together when the forward had no LayerNorm. */
int mmt_residual_block_bwd(const mmt_rows_desc* desc, const void* dx_new_in, const void* dh,
                           const void* x_new, const float* gamma, const float* mean,
                           const float* rstd, void* d_o, void* dx, float* dbias, float* dgamma,
                           float* dbeta, void* workspace, size_t workspace_bytes, void* stream);

/* Second half of a *_bwd call made with desc->defer_reduce: sums the partial column sums the first
 * half left in `workspace` into (o0, o1, o2) in fixed order (overwrite, or add with desc->accumulate).
 * kind: 0 = mmt_ln_bwd (dgamma, dbeta), 1 = mmt_residual_block_bwd with LayerNorm (dbias, dgamma, dbeta),
 * 2 = mmt_residual_block_bwd without LayerNorm (dbias), 3 = mmt_bias_gelu_bwd (dbias). */
int mmt_colsum_reduce(const mmt_rows_desc* desc, int32_t kind, const void* workspace, float* o0, float* o1,
                      float* o2, void* stream);

/* The same for up to 48 deferred reduces in ONE launch (a host that needs no parameter gradient before the backward
 * pass ends queues them: ~32 five-microsecond launches per step otherwise).  rows / H / kind / accumulate as in the
 * desc and call they stand for.  The outputs of the items (H floats each) must not overlap one another: every output is
 * read, added to and stored by a workgroup of its own item, so of two sums into the same memory one could be lost.  Such a
 * batch is refused before any launch with MMT_E_INVALID and a message that names both items (a parameter used twice in
 * one backward pass: launch its reduces one after the other). */
typedef struct mmt_colsum_item {
  const void* workspace;
  float* o0; float* o1; float* o2;
  int64_t rows;
  int32_t H, kind, accumulate, reserved;
} mmt_colsum_item;
int mmt_colsum_reduce_batch(int32_t n, const mmt_colsum_item* items, void* stream);

/* y = gelu_tanh(u + bias)   (DenseLayers hidden activation; rows x H with H = intermediate_size) */
int mmt_bias_gelu_fwd(const mmt_rows_desc* desc, const void* u, const float* bias, void* y,
                      void* stream);

/* du = dy * gelu_tanh'(u + bias);  dbias[H] = colsum(du) (overwritten). */
int mmt_bias_gelu_bwd(const mmt_rows_desc* desc, const void* dy, const void* u, const float* bias,
                      void* du, float* dbias, void* workspace, size_t workspace_bytes, void* stream);

/* acc[i] += g[i] for i < n: fp32 master-gradient accumulation of a low-precision gradient
 * (the `AccumulateGrad` step behind `optimizer.apply_gradients`, src/tasks/pretraining.py:262-273).
 * g_dtype: MMT_F32 | MMT_BF16; acc must be 16-byte aligned, g 8-byte aligned. */
/* out[c] (+)= sum_rows x[row, c] for a [rows, C] matrix (fp32 | bf16) with row stride ld >= C in elements and no
 * alignment requirement beyond the element's: the bias gradient dy.sum(0) of a Dense layer (`tape.gradient`,
 * src/tasks/pretraining.py:292-296) -- e.g. the output bias of the 30522-way MLM logits, whose rows start on odd
 * 4-byte boundaries.  Fixed-order sums (16 row groups, then the groups in order). */
size_t mmt_colsum_workspace_bytes(int64_t rows, int32_t C);
int mmt_colsum(int64_t rows, int32_t C, int32_t dtype, const void* x, int64_t ld, float* out, int32_t accumulate,
               void* workspace, size_t workspace_bytes, void* stream);
int mmt_accumulate_grad(float* acc, const void* g, int32_t g_dtype, int64_t n, void* stream);

/* Global-norm clip factor of the gradient slabs (`optimizer_config.gradient_clip_norm`, the reference's trainer
 * config src/configs/pretraining_experiments.py:24-47, applied after the all-reduce of pretraining.py:273):
 *   norm = pending_scale * sqrt(sum over all slabs of g^2),   *scale_out = min(1, max_norm / (norm + 1e-6)) * pending_scale
 * in one streaming pass + a fixed-order sum of 2048 per-block partials (bitwise reproducible).  `pending_scale` is a
 * factor (e.g. 1/replicas) the slabs have not been multiplied with yet; `scale_out` (device float) is what
 * mmt_adamw_step takes as grad_scale; `norm_out` (device float) may be NULL.  Up to 16 slabs, each 16-byte aligned
 * with a multiple of 4 elements; workspace: 2048 floats. */
int mmt_grad_clip_scale(int32_t n_slabs, const float* const* slabs, const int64_t* sizes, float max_norm,
                        float pending_scale, float* scale_out, float* norm_out, void* workspace,
                        size_t workspace_bytes, void* stream);

/* One AdamW step over a flat parameter slab (the optimizer of the reference's trainer config,
 * src/configs/pretraining_experiments.py:24-47: adamw, weight_decay_rate 0.01 with the
 * LayerNorm/bias exclusion list, applied after the gradient all-reduce of
 * src/tasks/pretraining.py:273).  Per element i of chunk c = i / 1024:
 *   g = grad[i] * (*grad_scale)                      (global-norm clip factor, device scalar, may be NULL)
 *   p = param[i] * (1 - lr * chunk_wd[c]);  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2
 *   p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)            (torch.optim.AdamW semantics)
 * writes param, exp_avg, exp_avg_sq (fp32), the bf16 shadow copy (nullable) and, with
 * zero_grad != 0, clears grad.  n must be a multiple of 1024; all buffers 16-byte aligned. */
typedef struct mmt_adamw_desc {
  int64_t n;
  float lr, beta1, beta2, eps;
  float bias_correction1, bias_correction2;   /* 1 - beta^t */
  int32_t zero_grad;
  int32_t reserved;
  const float* hyper;    /* ABI 4: DEVICE {lr, bias_correction1, bias_correction2} read by the kernel INSTEAD of the three
                            fields above, or NULL (mmt_attn.h: mmt_write_step_scalars)                                 */
} mmt_adamw_desc;

int mmt_adamw_step(const mmt_adamw_desc* desc, float* param, float* grad, float* exp_avg,
                   float* exp_avg_sq, void* param_bf16, const float* chunk_wd,
                   const float* grad_scale, void* stream);

/* One LAMB step over a flat parameter slab (TFM `optimizer.type: lamb` = tfa.optimizers.LAMB, restated from memory: no
 * TensorFlow was at hand to pin it).  The slab is cut into n_segments parameters, each of whole 1024-element chunks:
 * segment s owns chunks [segment_start[s], segment_start[s + 1]).  Per element i of chunk c in segment s, all in fp32:
 *   g  = grad[i] * (*grad_scale)                     (clip factor / deferred 1/replicas, device scalar, may be NULL)
 *   m  = b1 m + (1-b1) g;   v = b2 v + (1-b2) g^2;   mh = m / bc1;   vh = v / bc2
 *   u  = mh / (sqrt(vh) + eps) + chunk_wd[c] * w     (chunk_wd is 0 for parameters excluded from weight decay)
 *   r  = 1                                           when segment_adapt[s] == 0 (excluded from layer adaptation)
 *   r  = ||w||2 / ||u||2 over the whole segment      otherwise, if both norms are > 0; else 1
 *   w -= lr * r * u
 * writes param, exp_avg, exp_avg_sq (fp32), the bf16 shadow copy (nullable) and, with zero_grad != 0, clears grad;
 * with zero_grad == 0 grad holds u on return (the step uses the gradient slab for it).  Padding elements of a
 * parameter's last chunk must be zero in all four slabs on entry and are zero on exit.  Three launches and no atomics:
 * the sums have one fixed order that depends on the segment alone, so a step is bitwise reproducible and a
 * parameter's ratio does not depend on what shares the slab with it.  chunk_wd (n / 1024 floats), segment_start
 * (n_segments + 1 int32) and segment_adapt (n_segments int32) are DEVICE arrays; every chunk index read from
 * segment_start is clamped into [0, n / 1024], so a wrong table gives wrong ratios and never a stray access.
 * n must be a multiple of 1024; the fp32 slabs and the workspace 16-byte aligned; workspace: 12 bytes per chunk
 * (mmt_lamb_workspace_bytes; 0 for a bad n), caller-owned, nothing is allocated and the host does not wait.
 * `hyper` as in mmt_adamw_desc.  mmt_lamb_step_host runs the same per-element and per-chunk functions (csrc/lamb.h) as
 * plain loops on HOST arrays. */
typedef struct mmt_lamb_desc {
  int64_t n;
  float lr, beta1, beta2, eps;
  float bias_correction1, bias_correction2;   /* 1 - beta^t */
  int32_t zero_grad;
  int32_t n_segments;
  const float* hyper;    /* DEVICE {lr, bias_correction1, bias_correction2} read by the kernels INSTEAD of the three
                            fields above, or NULL (mmt_attn.h: mmt_write_step_scalars)                                 */
} mmt_lamb_desc;

size_t mmt_lamb_workspace_bytes(int64_t n);
int mmt_lamb_step(const mmt_lamb_desc* desc, float* param, float* grad, float* exp_avg, float* exp_avg_sq,
                  void* param_bf16, const float* chunk_wd, const int32_t* segment_start, const int32_t* segment_adapt,
                  const float* grad_scale, void* workspace, size_t workspace_bytes, void* stream);
int mmt_lamb_step_host(const mmt_lamb_desc* desc, float* param, float* grad, float* exp_avg, float* exp_avg_sq,
                       void* param_bf16, const float* chunk_wd, const int32_t* segment_start, const int32_t* segment_adapt,
                       const float* grad_scale, void* workspace, size_t workspace_bytes);

/* Exponential moving average of the weights over a flat parameter slab (TFM `optimizer_config.ema`, restated from memory
 * of official/modeling/optimization/ema_optimizer.py: no TensorFlow was at hand to pin it).  Per element, in fp32, with
 * omd = 1 - decay of the step:
 *   avg = fmaf(omd, param - avg, avg)                (the subtraction rounded first, then ONE fused multiply-add)
 * and exactly param for omd == 1, exactly avg for omd == 0.  `one_minus_decay_dev` is a DEVICE float read by the kernel
 * INSTEAD of the field, or NULL: the convention of mmt_adamw_desc.hyper, for a step replayed from a HIP graph.  One
 * launch, 12 bytes per element; nothing is allocated and the host does not wait.
 * mmt_ema_swap exchanges param and avg in place and writes param_bf16[i] = bf16(new param[i]) (round to nearest even,
 * what torch's copy_ gives; param_bf16 may be NULL): two calls restore all three buffers bit for bit.
 * n must be a positive multiple of 1024, the fp32 slabs 16-byte and the bf16 shadow 8-byte aligned, avg != param, and
 * one_minus_decay in [0, 1] when no device word is given: MMT_E_INVALID otherwise.  Padding elements are zero in param,
 * hence in avg, and stay zero.  The _host functions run the same per-element functions (csrc/ema.h) as plain loops on
 * HOST arrays (there the decay word, if given, is a host float). */
typedef struct mmt_ema_desc {
  int64_t n;
  float one_minus_decay;
  int32_t reserved;
  const float* one_minus_decay_dev;
} mmt_ema_desc;

int mmt_ema_step(const mmt_ema_desc* desc, const float* param, float* avg, void* stream);
int mmt_ema_step_host(const mmt_ema_desc* desc, const float* param, float* avg);
int mmt_ema_swap(int64_t n, float* param, float* avg, void* param_bf16, void* stream);
int mmt_ema_swap_host(int64_t n, float* param, float* avg, void* param_bf16);

/* Weight gradient of a Dense layer, accumulated into the fp32 master gradient:
 *   dw[M,N] += dy[K,M]^T . x[K,N]        (bf16 operands, fp32 accumulation, float atomics)
 * = the per-layer `tape.gradient` product + `AccumulateGrad` of src/tasks/pretraining.py:262-296.
 * Requires M % 128 == 0, N % 256 == 0 (any K), 16-byte aligned operands, ld* in elements
 * (ldy, ldx multiples of 8); returns MMT_E_UNSUPPORTED otherwise (callers fall back to a
 * library GEMM).  With a workspace of mmt_wgrad_workspace_bytes() the split-K partials are
 * written as plain fp32 slabs and summed in fixed order (bitwise reproducible); without one they
 * are added with float atomics (order not fixed). */
size_t mmt_wgrad_workspace_bytes(int32_t M, int32_t N, int64_t K);
/* Compute units one weight-gradient GEMM may fill (default 256 = the whole MI355X, clamped to [32, 256]).
 * Process-wide; a data-parallel host lowers it so that the split-K grid and the collective kernels
 * overlapping backward fit the chip together.  Affects mmt_wgrad_workspace_bytes: query after setting. */
void mmt_wgrad_set_cu_budget(int32_t cus);
int mmt_wgrad_accumulate(float* dw, int64_t ldw, const void* dy, int64_t ldy, const void* x,
                         int64_t ldx, int32_t M, int32_t N, int64_t K, void* workspace,
                         size_t workspace_bytes, void* stream);
/* Same, and additionally dbias[M] += column sums of dy (the Dense layer's bias gradient, fp32): the
 * workgroups of the first column tile add up the dy chunks they stage for the product anyway.
 * dbias == NULL: exactly mmt_wgrad_accumulate. */
int mmt_wgrad_bias_accumulate(float* dw, int64_t ldw, float* dbias, const void* dy, int64_t ldy,
                              const void* x, int64_t ldx, int32_t M, int32_t N, int64_t K,
                              void* workspace, size_t workspace_bytes, void* stream);

/* Up to 28 such products in ONE launch -- the weight gradients of the four Dense layers of one to seven encoder blocks
 * (`tape.gradient`, src/tasks/pretraining.py:292-296), which contract the same K = B*S rows.  Alone, the small
 * products need a deep split of K to fill the chip and write one fp32 slab per slice; together two slices
 * suffice for one block (108 tiles at BERT-base dims: 4x less slab traffic) and for two blocks K is not split
 * at all: every tile belongs to one workgroup, which adds it into dw with plain stores (no slabs, no reduce).
 * With more tiles than compute units (three blocks and up) the tiles go in whole rounds of one workgroup per tile over
 * the whole K, and only the tail that does not fill a round is split -- into compact per-tile slabs, reduced by a small
 * second launch (seven blocks: 756 tiles = 2 rounds + 244 unsplit; five: 2 rounds + 28 tiles x 8 slices).
 * Every problem needs M % 256 == 0, N % 256 == 0; K % 64 == 0; the workspace (mmt_wgrad_group_workspace_bytes, may be
 * 0 bytes) is required.  dbias may be NULL per problem.  Results are bitwise those of a fixed-order sum over the slices.
 * The outputs of a group must not overlap one another, judged by address range: dw from its first element to the last
 * one of row M - 1 (row stride ldw), dbias M floats.  Tiles of different problems are added into dw by different
 * workgroups with plain loads and stores, so of two products into the same memory one could be lost.  Such a group is
 * refused before any launch: mmt_wgrad_grouped returns MMT_E_INVALID and mmt_wgrad_group_workspace_bytes 0, each with a
 * message (mmt_last_error) that names the two problems.  Launch them one after the other. */
typedef struct mmt_wgrad_problem {
  float* dw;        /* [M, N] fp32, row stride ldw, accumulated into */
  int64_t ldw;
  float* dbias;     /* [M] fp32 += column sums of dy, or NULL */
  const void* dy;   /* [K, M] bf16, row stride ldy */
  int64_t ldy;
  const void* x;    /* [K, N] bf16, row stride ldx */
  int64_t ldx;
  int32_t M, N;
} mmt_wgrad_problem;
size_t mmt_wgrad_group_workspace_bytes(int32_t n, const mmt_wgrad_problem* problems, int64_t K);
int mmt_wgrad_grouped(int32_t n, const mmt_wgrad_problem* problems, int64_t K, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Embedding assembly of MmtEncoder.call (src/modeling/models/mmt_encoder.py:189-218):
 *   we  = Dropout(LayerNorm_eps(WordEmb[word_ids]))          LN + dropout on the WORD embeddings only
 *   out = we + SegEmb[segment_ids] (+ PosEmb[s]) (+ patch_proj[b, s - patch_start] + patch_bias
 *                                                 for patch_start <= s < patch_start + n_patch)
 * in one pass per row (one wave per row; tables fp32, `out` in `dtype`).  What TF runs as gather /
 * one-hot matmul, LayerNormalization, Dropout, three Adds, a Pad and a Cast.
 * Ids outside [0, vocab) contribute a zero row (one-hot lookup semantics, mmt_encoder.py:110).
 * patch_proj is the [B, n_patch, H] output of the patch projection GEMM WITHOUT its bias, in `dtype`. */
typedef struct mmt_embed_desc {
  int64_t rows;          /* B * S                                                        */
  int32_t S;             /* sequence length: row = b * S + s                             */
  int32_t H;             /* hidden size = embedding size; multiple of 8, <= 2048         */
  int32_t dtype;         /* MMT_F32 | MMT_BF16: out / patch_proj / dout / dpatch         */
  int32_t vocab;         /* rows of word_table                                           */
  int32_t seg_vocab;     /* rows of seg_table                                            */
  int32_t patch_start;   /* 2 in the reference ([CLS], [PATCH] first; mmt_encoder.py:213-218) */
  int32_t n_patch;       /* 0: no patch term                                             */
  float eps;             /* 1e-12                                                        */
  float dropout_p;       /* hidden_dropout_prob; 0 disables                              */
  int32_t accumulate;    /* backward: != 0 adds dgamma / dbeta INTO the given buffers     */
  uint64_t dropout_seed;
  const uint64_t* dropout_epoch; /* ABI 4: DEVICE uint64 added to dropout_seed by the kernel, or NULL (mmt_attn.h) */
} mmt_embed_desc;

int mmt_embed_fwd(const mmt_embed_desc* desc, const int32_t* word_ids, const int32_t* seg_ids,
                  const float* word_table, const float* seg_table, const float* pos_table /* nullable */,
                  const float* gamma, const float* beta, const void* patch_proj /* nullable */,
                  const float* patch_bias /* nullable */, void* out, float* mean, float* rstd,
                  void* stream);

/* Bytes of scratch mmt_embed_bwd needs. */
size_t mmt_embed_workspace_bytes(const mmt_embed_desc* desc);

/* Backward of mmt_embed_fwd for the word path and the patch slice:
 *   dword_table[id] += LayerNormBwd(DropoutBwd(dout[row]))   summed over the rows holding id,
 *   dgamma / dbeta (overwritten, or added to with desc->accumulate),
 *   dpatch[b, j] = dout[b, patch_start + j]                   (compact copy for the projection's wgrad GEMM; nullable).
 * `order` = the permutation that sorts word_ids ascending (stable: ties in row order) and
 * `sorted_ids[i] = word_ids[order[i]]` -- rows with the same id are then adjacent and are summed in that fixed order by ONE wave per id (runs longer
 * than 32 go through per-32 partial sums), so the scatter needs no atomics and is bitwise reproducible.
 * dword_table is fp32 [vocab, H] and is ACCUMULATED into (the master gradient).  The segment /
 * position table gradients are plain column sums of dout and are left to the caller. */
int mmt_embed_bwd(const mmt_embed_desc* desc, const void* dout, const int32_t* sorted_ids,
                  const int32_t* order, const float* word_table, const float* gamma, const float* mean,
                  const float* rstd, float* dword_table, float* dgamma, float* dbeta, void* dpatch,
                  void* workspace, size_t workspace_bytes, void* stream);

/* Packed multimodal rows (mmt_attn.h, MMT_FLAG_EXAMPLE_STARTS): the same two calls with two per-position inputs,
 *   example_starts int32 [B,S]  first position of the example the position belongs to (must not be NULL),
 *   patch_slots    int32 [B,S]  entry of the position's example in patch_proj / dpatch, now [n_examples, n_patch, H]
 *                               (one entry per imaged example of the batch); -1 = no image (NULL only with n_patch = 0).
 * With ls = s - start (clamped into [0, S)): the position row is pos_table[min(ls, pos_rows - 1)], and the patch row of
 * position s is patch_proj[slot][ls - patch_start] when 0 <= ls - patch_start < n_patch and 0 <= slot < n_examples.
 * The backward's compact copy scatters by the same rule, dpatch[slot][ls - patch_start] = dout[b, s]; rows of dpatch no
 * position maps to are not written (zero-fill it).  desc->patch_start + n_patch <= S is still asked.  Everything else,
 * and mmt_embed_fwd / mmt_embed_bwd themselves, as above. */
int mmt_embed_fwd_packed(const mmt_embed_desc* desc, const int32_t* word_ids, const int32_t* seg_ids,
                         const float* word_table, const float* seg_table, const float* pos_table /* nullable */,
                         int32_t pos_rows, const float* gamma, const float* beta, const void* patch_proj /* nullable */,
                         const float* patch_bias /* nullable */, const int32_t* example_starts,
                         const int32_t* patch_slots, int32_t n_examples, void* out, float* mean, float* rstd,
                         void* stream);
int mmt_embed_bwd_packed(const mmt_embed_desc* desc, const void* dout, const int32_t* sorted_ids,
                         const int32_t* order, const float* word_table, const float* gamma, const float* mean,
                         const float* rstd, float* dword_table, float* dgamma, float* dbeta, void* dpatch,
                         const int32_t* example_starts, const int32_t* patch_slots, int32_t n_examples,
                         void* workspace, size_t workspace_bytes, void* stream);

/* All pairs from separate sets (retrieval; the reference's loader enumerates image x text combinations,
 * src/data/retrieval_dataloader.py:139-195): mmt_embed_fwd on the batch whose row b is image image_entry[b] followed by
 * text text_entry[b], without that batch ever being materialised.  Forward only (the loader is for prediction only).
 *   image_entry, text_entry  int32 [B]  row of the image / text table for pair b; an entry is valid when (unsigned)entry < n
 *   prefix_ids   int32 [n_img], n_img = patch_start + n_patch   the shared image-side word ids ([CLS] [PATCH] patch ids)
 *   text_ids     int32 [n_texts, Lt], Lt = S - n_img             zero-padded text ids (data_utils.py:272-276)
 *   text_len     int32 [n_texts]                                 text length in wordpieces
 *   patch_proj   [n_images, n_patch, H] in `dtype`               projected patches of the image table
 * With i = image_entry[b], t = text_entry[b], for position s of row b:
 *   word   = s < n_img ? prefix_ids[s] : (t valid ? text_ids[t][s - n_img] : 0)
 *   n_text = t valid ? clamp(text_len[t], 0, Lt) : 0
 *   seg    = s < n_img ? 1 : (s > n_img && s < n_img + n_text ? 2 : 0)        (data_utils.py:350-361)
 *   out    = LN(word_table[word]) + seg_table[seg] (+ pos_table[s])
 *            (+ patch_proj[i][s - patch_start] + patch_bias when i valid and 0 <= s - patch_start < n_patch)
 *   valid_len_out[b] = n_img + n_text                                          (int32 [B])
 * Same arithmetic in the same order as mmt_embed_fwd: the result equals mmt_embed_fwd on the materialised batch bit
 * for bit.  Garbage entries, lengths and ids give the numbers of the rule, never a stray access.  desc->rows = B * S;
 * desc->dropout_p != 0 is MMT_E_UNSUPPORTED; n_img >= S is MMT_E_INVALID; mean / rstd are not produced. */
int mmt_embed_fwd_pairs(const mmt_embed_desc* desc, const int32_t* image_entry, const int32_t* text_entry,
                        const int32_t* prefix_ids, const int32_t* text_ids, const int32_t* text_len, int32_t n_images,
                        int32_t n_texts, const float* word_table, const float* seg_table,
                        const float* pos_table /* nullable */, const float* gamma, const float* beta,
                        const void* patch_proj /* nullable */, const float* patch_bias /* nullable */, void* out,
                        int32_t* valid_len_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-row softmax cross-entropy of wide logits (the tied 30522-way MLM head):
 *   loss[row] = logsumexp(logits[row, :]) - logits[row, labels[row]]       (natural log; lse saved)
 * = the `unweighted` term of src/modeling/losses/weighted_sparse_categorical_crossentropy_loss.py:17-43;
 * the weighting and divide_no_nan reduction over a few hundred rows stay with the caller.
 * logits are read once in their storage dtype (MMT_F32 | MMT_BF16), row stride `ld` elements.
 * A label outside [0, C) means "no target": loss 0, zero gradient.
 * A logit of -inf (a masked class) contributes exp(-inf) = 0 to its row's sum (softmax 0 there); a label on such a
 * column gives loss +inf and a finite gradient.  A row that is -inf everywhere is unspecified (NaN, as in torch).  A NaN logit makes the
 * loss of its own row NaN and of no other row.
 * Backward: dlogits[row, i] = (softmax(logits[row])[i] - [i == label]) * coef[row], written in `dtype`. */
int mmt_xent_fwd(int64_t rows, int32_t C, int32_t dtype, const void* logits, int64_t ld,
                 const int32_t* labels, float* loss, float* lse, void* stream);
/* The same pass also reporting argmax[row] = the FIRST index of the row's largest logit -- what tf.argmax, hence
 * tf.keras.metrics.SparseCategoricalAccuracy (src/tasks/pretraining.py:183-222), compares with the label -- so that the
 * accuracy metrics cost no second sweep over the 30522-way logits.  `argmax` may be NULL. */
int mmt_xent_fwd_argmax(int64_t rows, int32_t C, int32_t dtype, const void* logits, int64_t ld,
                        const int32_t* labels, float* loss, float* lse, int32_t* argmax, void* stream);
int mmt_xent_bwd(int64_t rows, int32_t C, int32_t dtype, const void* logits, int64_t ld,
                 const int32_t* labels, const float* lse, const float* coef, void* dlogits, int64_t ldd,
                 void* stream);
/* The same with one more factor read on the device: dlogits *= gscale[0] (gscale may be NULL) -- the upstream
 * gradient of a scalar loss, so that the host never reads it. */
int mmt_xent_bwd_scaled(int64_t rows, int32_t C, int32_t dtype, const void* logits, int64_t ld,
                        const int32_t* labels, const float* lse, const float* coef, const float* gscale,
                        void* dlogits, int64_t ldd, void* stream);
/* The reduction of `weighted_sparse_categorical_crossentropy_loss`
 * (src/modeling/losses/weighted_sparse_categorical_crossentropy_loss.py:36-43) and of the loss bookkeeping around it
 * (src/tasks/pretraining.py:95-140: MLM / MPP weights masked by the example's ITM label) in one launch:
 *   w_i = weight[i] * (mask ? mask[i / mask_div] : 1),   l_i = loss[i] * (lmul ? lmul[i] : 1)
 *   num = sum_i w_i l_i,  den = sum_i w_i,  out3 = { divide_no_nan(num, den), num, den }
 *   coef[i] = d out3[0] / d loss[i] = den != 0 ? w_i lmul_i / den : 0        (coef may be NULL)
 * All arrays fp32 on the device; one workgroup, sums in a fixed order (bitwise reproducible). */
int mmt_weighted_loss(int64_t rows, const float* loss, const float* weight, const float* lmul, const float* mask,
                      int64_t mask_div, float* out3, float* coef, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Feed-forward GEMMs with the GELU in the epilogue (bf16 operands, fp32 accumulate; K11, csrc/ffn_gemm.hip).
 * They replace, for the intermediate Dense of the encoder block (reference: the `inner_activation` Dense pair
 * of every TransformerEncoderBlock the encoder stacks, mmt_encoder.py:53-54 + 221-238), the sequence
 * "library GEMM -> mmt_bias_gelu_fwd" and, in the tape's backward, "library GEMM -> mmt_bias_gelu_bwd":
 *   mmt_ffn_gelu_gemm :  u[M,N] = x[M,K] . w[N,K]^T + bias[N]   (u optional, rounded to bf16)
 *                        g[M,N] = gelu_tanh(u)                    (of the ROUNDED u, so that the backward, which
 *                                                                  only has the stored u, sees the same function)
 *   mmt_ffn_dgelu_gemm:  du[M,N] = (dy[M,K] . w[K,N]) * gelu_tanh'(u[M,N] + bias[N])      (bias may be NULL)
 * All matrices row-major with row strides ld* in elements (multiples of 8), 16-byte aligned; bias fp32.
 * Needs M % 256 == 0, N % 256 == 0, K % 64 == 0, otherwise MMT_E_UNSUPPORTED (nothing launched).
 * The kernels are persistent, one workgroup per compute unit: mmt_ffn_set_cu_budget (default 256, clamped to
 * [32, 256], process-wide) sizes the grid, e.g. to leave units to collective kernels that overlap backward. */
void mmt_ffn_set_cu_budget(int32_t cus);
int mmt_ffn_gelu_gemm(const void* x, int64_t ldx, const void* w, int64_t ldw, const float* bias, void* u,
                      int64_t ldu, void* g, int64_t ldg, int64_t M, int64_t N, int64_t K, void* stream);
int mmt_ffn_dgelu_gemm(const void* dy, int64_t lddy, const void* w, int64_t ldw, const void* u, int64_t ldu,
                       const float* bias, void* du, int64_t lddu, int64_t M, int64_t N, int64_t K, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Image front end of the data layer: decoded uint8 RGB images of mixed sizes -> patch features, in one launch
 * (csrc/image_patches.hip).  The tensor half of the reference's `decode_fn` (src/data/data_utils.py:195-222):
 *   x = u8 / 255;   r = bilinear resize of x to image_size x image_size with tf.image.resize's TF2 defaults
 *   (half-pixel centres, no antialiasing, 2x2 taps:  src = (dst + 0.5) * in / out - 0.5,  lo = max(floor(src), 0),
 *   hi = min(ceil(src), in - 1),  t = src - floor(src);  horizontal lerp, then vertical);
 *   unnormalised = r;   normalised = (r - mean) / mean   (the reference's line 204 divides by the MEAN);
 *   flip[b] != 0: both outputs take column image_size - 1 - x (after the resize, :209-211);
 *   patches: P = image_size / patch_size, the remainder rows / columns dropped (VALID), raster order over patches,
 *   (row, column, channel) inside one: outputs are [B, P*P, patch_size^2 * 3];
 *   label ids [B, P*P] (masked-patch prediction, :448-481): the channel means of the unnormalised patch, times 255,
 *   in 2^channel_bits equal bins, combined as digits of base 2^channel_bits with channel 0 the least significant.
 * Example b is heights[b] x widths[b] x 3 bytes, row-major, starting at pixels + offsets[b].  pixels, offsets (int64
 * [B]), heights, widths (int32 [B]) and flip (uint8 [B], or NULL: no flip) are DEVICE memory, so the call can be
 * recorded into a graph.  normalised_out is `out_dtype`; unnormalised_out (fp32) and label_ids_out may each be NULL
 * and are then not computed; ids also need channel_bits > 0.  Ids are summed in a fixed order (no atomics): bitwise
 * reproducible.  The kernel never reads outside [pixels, pixels + pixels_bytes): taps are clamped to the image,
 * heights / widths below 1 count as 1, offsets and every byte address are clamped into the buffer -- wrong metadata
 * gives wrong pixels, not a fault.  B * P * P and patch_size^2 * 3 must each stay below 2^31. */
typedef struct mmt_image_desc {
  int32_t B;             /* examples                                                     */
  int32_t image_size;    /* output height = width                                        */
  int32_t patch_size;    /* <= image_size                                                */
  int32_t out_dtype;     /* MMT_F32 | MMT_BF16: normalised_out                           */
  int32_t channel_bits;  /* 1..8: bits per channel of the label ids; 0: no ids           */
  float mean[3];         /* per channel, non-zero; (0.485, 0.456, 0.406) in the reference */
} mmt_image_desc;

int mmt_image_patches(const mmt_image_desc* desc, const uint8_t* pixels, int64_t pixels_bytes, const int64_t* offsets,
                      const int32_t* heights, const int32_t* widths, const uint8_t* flip, void* normalised_out,
                      float* unnormalised_out, int32_t* label_ids_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * RandAugment on the device (csrc/rand_augment.hip): the augmentation `decode_fn` applies to the decoded uint8 image
 * before everything above (src/data/data_utils.py:125-145, 199-202; `RandAugment(num_layers=1)` with the reference's
 * list of 14 operations).  One operation per image, uint8 in and uint8 out at the source resolution, on the packed
 * layout of the front end: out_pixels has the size and the offsets of pixels, so the front end consumes it unchanged.
 *   op  int32 [B]      0 AutoContrast, 1 Equalize, 2 Rotate, 3 Posterize, 4 Solarize, 5 Color, 6 Contrast, 7 Brightness,
 *                      8 Sharpness, 9 ShearX, 10 ShearY, 11 TranslateX, 12 TranslateY, 13 SolarizeAdd; -1 and every
 *                      other value: the image is copied
 *   arg float [B, 8]   [0]: bits (3), threshold (4), addend (13), all truncated to int; blend factor (5, 6, 7, 8);
 *                      [0..5]: a0 a1 a2 b0 b1 b2 of the affine ops (2, 9..12): output (x, y) takes the source pixel
 *                      nearest to ((a0 x + a1 y) + a2, (b0 x + b1 y) + b2), or 128 when that lies outside the image
 * The definitions are in DESIGN.md section 4: integer arithmetic, and fp32 with every product and sum rounded on its
 * own where a blend or a coordinate needs it, so results are exact and bitwise reproducible (the histograms of ops 0,
 * 1 and 6 are summed with integer atomics).  pixels, offsets, heights, widths, op, arg, out_pixels and the workspace
 * are DEVICE memory and are read by the kernels, nothing is allocated and the host does not wait: a recorded graph
 * follows new values.  The workspace (mmt_rand_augment_workspace_bytes(B) bytes, 4-byte aligned) needs no
 * initialisation; the call clears what it uses.  Bytes of out_pixels outside every image are not written.
 * out_pixels must not overlap pixels (MMT_E_INVALID).  The front end's safety rule holds for reads and writes: sizes
 * below 1 count as 1, offsets and byte addresses are clamped into [0, pixels_bytes) -- wrong metadata gives wrong
 * pixels, not a fault.  h * w * 3 < 2^31 per image. */
size_t mmt_rand_augment_workspace_bytes(int32_t B);            /* host only; 0 for B < 1 */
int mmt_rand_augment(int32_t B, const uint8_t* pixels, int64_t pixels_bytes, const int64_t* offsets,
                     const int32_t* heights, const int32_t* widths, const int32_t* op, const float* arg /* [B,8] */,
                     uint8_t* out_pixels, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Text front end of the data layer (csrc/text_tokens.hip): the text half of `decode_fn` (src/data/data_utils.py:241-278).
 * Each of the F UTF-8 fields of an example is tokenised as original BERT does with do_lower_case (DESIGN.md section 4
 * states the definition per code point), the fields share `budget` wordpieces round-robin, and the row
 *   tok_0 pieces_0 tok_1 pieces_1 ... [SEP]   padded with 0 to T
 * is written with its length (F + sum a_f + 1) and the word starts: 1 on each field token, on [SEP] and on the first
 * piece of every word, 0 elsewhere and in the padding.  Field (b, f) is lengths[b*F + f] bytes from bytes +
 * offsets[b*F + f]; offsets are clamped into [0, bytes_len] and lengths into what is left, so wrong metadata gives wrong
 * ids, not a fault.  A field's work ends once it has produced `budget` pieces, however long it is.
 *
 * Vocabulary image (built on the host by mmt_wordpiece_vocab_build, uploaded by the caller; 32-bit words):
 *   words 0..7   magic "MWPV" (0x5650574d), tokens, slots (a power of two >= 2 * tokens), first word of the token bytes
 *                (8 + 4 * slots), token bytes stored, three reserved words
 *   slots        4 words each, open addressing with linear probing from mix(key) & (slots - 1):
 *                  [0] id + 1 (0: empty)   [1] key   [2] first byte, from the start of the token bytes
 *                  [3] bytes of the piece | bit 31: a `##` piece
 *                key = (sum_t c_t * 0x01000193^t mod 2^32) over the piece's code points c_t, xor 0x9e3779b9 for a `##`
 *                piece; mix(x): x ^= x >> 16, x *= 0x7feb352d, x ^= x >> 15, x *= 0x846ca68b, x ^= x >> 16
 *   token bytes  the pieces' UTF-8 bytes back to back, without the `##` prefix, padded to a whole word
 * A token that starts with `##` and is longer is a continuation piece; ids are the positions in the token list.  Empty,
 * duplicated and ill-formed (not UTF-8) tokens are refused.  A hash hit is confirmed byte by byte on the device.
 *
 * Code-point table (uint32, made by the caller: mmt_amd.text_frontend builds it from unicodedata): entries
 * [0, 0x110000) by source code point, then the side table.  Entry: bits 0..20 value, bit 21 "a word of its own",
 * bits 22..23 mapped characters n (0..3), bit 24 "separates words" (space).  n = 0 without bit 24: dropped.  n = 1: the
 * value is the mapped character.  n = 2, 3: the value indexes the side table, whose n consecutive entries hold a
 * character in bits 0..20 and bit 21 each.  codepoint_entries counts both parts; side indices are clamped into it.
 *
 * bytes, offsets (int64 [B*F]), lengths (int32 [B*F]), both tables, the outputs and the workspace are DEVICE memory;
 * field_token_ids (F ids, F <= 16) is HOST memory and is read during the call.  Nothing is allocated and the host does
 * not wait, so the call can be recorded into a graph.  Every element of token_ids_out [B,T], num_wordpieces_out [B] and
 * word_start_out [B,T] is written, nothing else.  The workspace (mmt_text_tokens_workspace_bytes, 4-byte aligned)
 * needs no initialisation.  No atomics: the same bytes give the same ids.  Refused: NULL arguments, B / F / T below 1,
 * budget < 0, F + budget + 1 > T, a table too small to be one, misalignment (MMT_E_INVALID), F > 16 (MMT_E_UNSUPPORTED),
 * a workspace that is too small (MMT_E_WORKSPACE). */
size_t mmt_wordpiece_vocab_bytes(int64_t n_tokens, int64_t token_bytes);   /* host only; 0 when out of range */
int mmt_wordpiece_vocab_build(int64_t n_tokens, const uint8_t* token_bytes, const int64_t* token_offsets /* [n_tokens + 1], from 0 */,
                              void* image /* host, 4-byte aligned */, size_t image_bytes);
size_t mmt_text_tokens_workspace_bytes(int32_t B, int32_t F, int32_t budget);   /* host only; 0 for B, F < 1 or budget < 0 */
int mmt_text_tokens(int32_t B, int32_t F, const uint8_t* bytes, int64_t bytes_len, const int64_t* offsets,
                    const int32_t* lengths, const void* vocab_image, size_t vocab_image_bytes,
                    const uint32_t* codepoint_table, int64_t codepoint_entries, const int32_t* field_token_ids /* host [F] */,
                    int32_t sep_id, int32_t unk_id, int32_t T, int32_t budget, int32_t* token_ids_out /* [B,T] */,
                    int32_t* num_wordpieces_out /* [B] */, uint8_t* word_start_out /* [B,T] */, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * JPEG decode in front of the image front end (csrc/jpeg_decode.hip): `tf.io.decode_image(example['image_data'])` of
 * `decode_fn` (src/data/data_utils.py:195) for JPEG bytes, as libjpeg decodes by default (JDCT_ISLOW, fancy
 * upsampling; the rules are DESIGN.md section 4, "JPEG decode").  The serial part -- markers and Huffman decoding --
 * runs on the host and yields quantised coefficients; dequantisation, the 8x8 inverse DCT, chroma upsampling, YCbCr to
 * RGB and range limiting run on the device and write the packed layout that the two entry points above read: image b
 * is height x width x 3 bytes, row-major RGB, from pixels_out + pixel_offset.
 *
 * Accepted: SOF0 / SOF1 (baseline, extended sequential), Huffman coded, 8-bit samples, 1 component (grey: R = G = B)
 * or 3 (YCbCr) with chroma 1x1 and luma 1x1, 2x1 or 2x2; any number of scans; DRI / RSTn; 8-bit DQT.  Refused with
 * MMT_E_UNSUPPORTED: progressive, arithmetic, lossless and hierarchical files, 12-bit samples, 16-bit quantisation
 * tables, 4 components, other sampling patterns, RGB stored directly (Adobe transform 0), and whatever is not a JPEG.
 * A truncated or corrupt stream is MMT_E_INVALID.
 *
 * One struct describes an image to every call.  The info call fills it with the offsets of a stand-alone image
 * (coef_offset from 0, pixel_offset 0); a caller that batches adds each image's base to coef_offset[] and sets
 * pixel_offset.  blocks_w / blocks_h are the component's grid of 8x8 blocks, padded to whole MCUs; component c owns
 * blocks_w[c] * blocks_h[c] * 64 int16 coefficients from coef + coef_offset[c]: quantised, DC prediction resolved,
 * natural (de-zigzagged) order, [block_y][block_x][64]; blocks no scan covers are zero.  coef_offset[] must be
 * multiples of 8.  qtables holds one table of 64 uint16 per component in natural order: [3][64] per image, image b of
 * a batch at qtables + b * 192. */
typedef struct mmt_jpeg_image {
  int32_t width, height;     /* pixels                                                        */
  int32_t components;        /* 1 | 3                                                         */
  int32_t h_samp[3];         /* sampling factors per component (1 | 2)                        */
  int32_t v_samp[3];
  int32_t blocks_w[3];       /* block grid per component, whole MCUs                          */
  int32_t blocks_h[3];
  int64_t coef_offset[3];    /* first coefficient of the component's plane, in int16 elements */
  int64_t coef_elems;        /* int16 elements of the whole image                             */
  int64_t pixel_offset;      /* first byte of the image in pixels_out                         */
} mmt_jpeg_image;

/* Host only, no device call, re-entrant, nothing allocated that outlives the call; never reads past len.
 * The info call parses the headers up to the first SOS.  The coefficients call entropy-decodes every scan into the
 * caller's HOST memory (pinned, if it is to be uploaded): `image` must describe this stream (as the info call
 * reported it, offsets rebased at will) and every plane must lie inside [0, coef_elems).  qtables_out: [3][64]. */
int mmt_jpeg_info(const uint8_t* bytes, int64_t len, mmt_jpeg_image* out);
int mmt_jpeg_coefficients(const uint8_t* bytes, int64_t len, const mmt_jpeg_image* image, int16_t* coef,
                          int64_t coef_elems, uint16_t* qtables_out /* [3][64] */);

/* Stage 2.  The device call takes DEVICE memory throughout (images [B], coef, qtables [B][3][64], pixels_out and the
 * workspace), allocates nothing and does not wait, so it can be recorded into a graph; two launches whatever B is
 * (dequantisation + IDCT into uint8 component planes in the workspace, then upsampling + colour), no atomics, bitwise
 * reproducible.  The workspace (mmt_jpeg_workspace_bytes(coef_elems) bytes) needs no initialisation.  coef and qtables
 * must be 16-byte aligned, coef_elems in [64, 2^60), pixels_bytes in [1, 2^60).  Bytes of pixels_out outside every
 * image are not written.  The front end's safety rule holds for every read and write: sizes, grids and offsets from
 * `images` are clamped into the buffers -- wrong metadata gives wrong pixels, not a fault.  The host variant is the
 * same arithmetic as a plain loop over HOST memory (CPU tensors, host tests, the sanitizer program). */
size_t mmt_jpeg_workspace_bytes(int64_t coef_elems);           /* host only; 0 for coef_elems < 64 */
int mmt_jpeg_pixels(int32_t B, const mmt_jpeg_image* images, const int16_t* coef, int64_t coef_elems,
                    const uint16_t* qtables, uint8_t* pixels_out, int64_t pixels_bytes, void* workspace,
                    size_t workspace_bytes, void* stream);
int mmt_jpeg_pixels_host(int32_t B, const mmt_jpeg_image* images, const int16_t* coef, int64_t coef_elems,
                         const uint16_t* qtables, uint8_t* pixels_out, int64_t pixels_bytes, void* workspace,
                         size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * JPEG entropy decode on the device (csrc/jpeg_entropy.hip; DESIGN.md section 4, "JPEG entropy decode on the device"):
 * the Huffman decode of the scan as kernels, so that the encoded bytes are uploaded in place of the coefficients.  Its
 * output is the coefficient layout described above, the one mmt_jpeg_coefficients writes and mmt_jpeg_pixels reads.
 * Served: files with ONE scan that carries every component (interleaved 4:4:4 / 4:2:2 / 4:2:0, or one grey component),
 * which is what libjpeg, Pillow and tf.io.encode_jpeg write.  The plan call refuses a file with more than one scan with
 * MMT_E_UNSUPPORTED; such a file goes through mmt_jpeg_coefficients.
 *
 * The scan is cut into restart segments (the bytes between RSTn markers; one segment without DRI) and every segment
 * into subsequences of subseq_bytes raw bytes (a power of two in [8, 1024]); a subsequence never straddles a segment.
 * One thread owns a subsequence.  Its state at a boundary is (bit position in the scan, block inside the MCU, zigzag
 * index); where all components share their tables the block inside the MCU is left out (uniform_tables).  Round 0 decodes every subsequence from an assumed state, round r from the exit state its left neighbour
 * reached in round r - 1; after r rounds the first r + 1 subsequences of every segment are exact, so max_rounds >=
 * max_segment_subseq is exact by construction and Huffman streams synchronise themselves long before.  A final pass
 * checks the chain of states, decodes once more and writes.
 *
 * Plan, per image (host memory, filled by mmt_jpeg_scan_plan; a caller that batches concatenates them and rebases
 * byte_offset, segment_offset and subseq_offset, as it rebases coef_offset):
 *   scan      mmt_jpeg_scan below
 *   huff      uint32 [6][MMT_JPEG_HUFF_WORDS]: the DC then the AC table of scan component 0, 1, 2 (unused: zero).
 *             Table: words 0..255 hold 512 uint16 entries indexed by the next 9 bits, (length << 8) | symbol, 0 when
 *             the code is longer; words 256..262 the largest code of lengths 10..16 (int32, -1: none); words 264..270
 *             (index of the first symbol of that length) - (its code); words 272..335 the 256 symbols as bytes
 *   qtables   uint16 [3][64], exactly what mmt_jpeg_coefficients writes
 *   segments  int32 [n_segments][4]: first byte and end byte (from the scan's first byte), first MCU, first
 *             subsequence (from the image's first)
 *   subseqs   int32 [n_subseq]: the segment of each subsequence (from the image's first)
 * With segments_out and subseqs_out both NULL the call only reports: it fills scan_out (n_segments and n_subseq are the
 * capacities to allocate) and, where given, huff_out and qtables_out.  Host only, re-entrant, never reads past len,
 * allocates nothing that outlives the call.  Malformed data is MMT_E_INVALID as in mmt_jpeg_coefficients. */
#define MMT_JPEG_HUFF_WORDS 336
#define MMT_JPEG_ST_OK 0            /* status[b] of the entropy calls                                        */
#define MMT_JPEG_ST_BAD_CODE 1      /* corrupt: a code that is not in the table                              */
#define MMT_JPEG_ST_RUN 2           /* corrupt: a zero run past coefficient 63                               */
#define MMT_JPEG_ST_OVERRUN 3       /* corrupt: a segment ends inside a block                                */
#define MMT_JPEG_ST_BLOCKS 4        /* corrupt: a segment holds the wrong number of blocks                   */
#define MMT_JPEG_ST_NOT_CONVERGED 16 /* no error: max_rounds did not suffice, decode the file on the host    */
typedef struct mmt_jpeg_scan {
  int64_t byte_offset;        /* first entropy-coded byte of the scan in `bytes`                             */
  int64_t byte_count;         /* bytes of the scan, restart markers included, below 2^28                     */
  int64_t segment_offset;     /* the image's first entry in `segments`                                       */
  int64_t subseq_offset;      /* the image's first entry in `subseqs`                                        */
  int32_t n_segments;
  int32_t n_subseq;
  int32_t max_segment_subseq; /* subsequences of the longest segment                                         */
  int32_t components;         /* of the MCU: 1 | 3                                                           */
  int32_t dc_table[3];        /* the scan header's table selectors (huff is laid out per component)          */
  int32_t ac_table[3];
  int32_t restart_interval;   /* MCUs per segment, 0: one segment                                            */
  int32_t mcus;               /* MCUs of the scan                                                            */
  int32_t subseq_bytes;
  int32_t uniform_tables;     /* 1: every component names the same DC and the same AC table, so the block inside the
                                 MCU decides nothing and is no part of a decoder's state (it stays 0)               */
} mmt_jpeg_scan;

int mmt_jpeg_scan_plan(const uint8_t* bytes, int64_t len, const mmt_jpeg_image* image, int32_t subseq_bytes,
                       mmt_jpeg_scan* scan_out, uint32_t* huff_out /* [6][336] | NULL */,
                       uint16_t* qtables_out /* [3][64] | NULL */, int32_t* segments_out, int64_t segment_capacity,
                       int32_t* subseqs_out, int64_t subseq_capacity);

/* The device call takes DEVICE memory throughout: bytes (the files back to back, 16-byte aligned, bytes_len of them),
 * images [B], scans [B], huff [B][6][336], segments [n_segments][4], subseqs [n_subseq], coef (16-byte aligned), status
 * (int32 [B]) and the workspace (mmt_jpeg_entropy_workspace_bytes, 16-byte aligned).  max_subseq is the largest
 * n_subseq of an image (an image that has more gets an error status), max_rounds >= 1 the number of rounds.  Nothing
 * is allocated and the host does not wait; the launches -- clear, max_rounds rounds, two for the offsets, write, DC
 * prediction: max_rounds + 5, their grids sized by B, max_subseq and subseq_bytes -- depend on the arguments alone, so
 * the call can be recorded into a graph.  Neither the workspace nor coef need be initialised: every plane of every
 * image is written whole, nothing of coef outside the planes is touched, and the result is bitwise reproducible.
 * status[b]: MMT_JPEG_ST_OK; MMT_JPEG_ST_NOT_CONVERGED (no error; the planes of that image are unspecified, inside their
 * bounds); or the largest error code met (corrupt stream).  One image's failure does not disturb another image.  After
 * the call the first max_rounds * B int32 of the workspace hold, [round][image], whether the round changed a state.
 * The front end's safety rule holds: every offset, count and index read from device memory is clamped into its buffer
 * and every loop is bounded by a buffer size, 64 slots per block or max_rounds -- wrong plans give wrong coefficients or
 * a status, not a fault.  No workgroup waits for another inside a launch.  The host variant runs the same functions as
 * plain loops over HOST memory, round for round and group for group: the same coefficients and the same status. */
size_t mmt_jpeg_entropy_workspace_bytes(int32_t B, int64_t n_subseq, int32_t max_subseq, int32_t subseq_bytes,
                                        int32_t max_rounds);     /* host only; 0 when an argument is out of range */
int mmt_jpeg_entropy(int32_t B, const uint8_t* bytes, int64_t bytes_len, const mmt_jpeg_image* images,
                     const mmt_jpeg_scan* scans, const uint32_t* huff, const int32_t* segments, int64_t n_segments,
                     const int32_t* subseqs, int64_t n_subseq, int32_t max_subseq, int32_t subseq_bytes,
                     int32_t max_rounds, int16_t* coef, int64_t coef_elems, int32_t* status, void* workspace,
                     size_t workspace_bytes, void* stream);
int mmt_jpeg_entropy_host(int32_t B, const uint8_t* bytes, int64_t bytes_len, const mmt_jpeg_image* images,
                          const mmt_jpeg_scan* scans, const uint32_t* huff, const int32_t* segments, int64_t n_segments,
                          const int32_t* subseqs, int64_t n_subseq, int32_t max_subseq, int32_t subseq_bytes,
                          int32_t max_rounds, int16_t* coef, int64_t coef_elems, int32_t* status, void* workspace,
                          size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------------------------
 * Record container of the data layer (csrc/records.hip; DESIGN.md section 4, "Records"): the TFRecord frames and the
 * tf.train.Example fields that src/data/pretrain_dataloader.py:62-72 reads.
 *
 * A frame is  uint64 length (little endian) | uint32 masked_crc32c(the 8 length bytes) | length payload bytes |
 * uint32 masked_crc32c(payload), with CRC-32C (Castagnoli, reflected 0x82F63B78, init and final xor 0xFFFFFFFF) and
 * mask(c) = ((c >> 15 | c << 17) + 0xa282ead8) mod 2^32.
 *
 * The two host calls are plain C++: re-entrant, they allocate nothing that outlives the call and never read past len;
 * errors go through mmt_last_error with the byte offset.
 *
 * mmt_records_scan walks frames from offset 0 and writes one mmt_record per whole frame.  The length checksum is
 * verified (wrong: MMT_E_INVALID -- there is no resynchronisation); the payload checksum is only copied out, it is
 * verified by mmt_records_crc.  A frame that does not fit in the remaining bytes, or a full records_out, ends the walk:
 * *consumed_out is that frame's first byte (len when every byte was consumed), so a chunked reader continues there.
 * The fit test cannot wrap for a declared length near 2^64.
 *
 * mmt_example_fields looks n_names features (NUL-terminated names) up in one serialized tf.train.Example
 * (Example.features = 1; Features.feature = 1, a map entry key = 1 / value = 2; Feature.bytes_list = 1, float_list = 2,
 * int64_list = 3; value = 1 in each list; int64 and float lists packed or unpacked; varints of up to 10 bytes; unknown
 * fields of wire types 0, 1, 2 and 5 skipped).  Groups, a length that leaves its enclosing message, a truncated or
 * 11-byte varint and a packed float list whose length is no multiple of 4 are MMT_E_INVALID.  Repeated `features`
 * merge, a repeated key keeps its last value, a Feature with no kind set counts as missing. */
#define MMT_FIELD_MISSING 0
#define MMT_FIELD_BYTES 1
#define MMT_FIELD_INT64 2
#define MMT_FIELD_FLOAT 3
typedef struct mmt_record {
  int64_t offset;          /* of the payload, from the start of the scanned bytes */
  int64_t length;          /* of the payload */
  uint32_t crc;            /* the stored (masked) payload checksum */
  uint32_t reserved;
} mmt_record;
typedef struct mmt_example_field {
  int32_t kind;            /* MMT_FIELD_* */
  float float_value;       /* the first value of a float list */
  int64_t count;           /* number of values */
  int64_t offset, length;  /* the first value of a bytes list, inside payload */
  int64_t int_value;       /* the first value of an int64 list */
} mmt_example_field;
int mmt_records_scan(const uint8_t* bytes, int64_t len, mmt_record* records_out, int64_t capacity, int64_t* n_out,
                     int64_t* consumed_out);
int mmt_example_fields(const uint8_t* payload, int64_t len, int32_t n_names, const char* const* names,
                       mmt_example_field* fields_out /* [n_names] */);

/* Payload checksums on the device: crc_out[i] = CRC-32C (unmasked) of records[i]'s payload inside bytes, bad_out[i] =
 * (mask(crc_out[i]) != records[i].crc).  DEVICE memory throughout (records 8-byte, crc_out and bad_out 4-byte, the
 * workspace of mmt_records_crc_workspace_bytes(n) 16-byte aligned; bytes at any alignment); nothing is allocated, the
 * host does not wait, and the three launches (piece counts and their prefix sum, the pieces, the comparison) and their
 * grids depend on bytes_len and n alone, so the call can be recorded into a graph.  Work is cut by bytes: every payload
 * into pieces of MMT_RECORDS_PIECE bytes counted from its END (so only a record's first piece is short), a lane takes a
 * piece, a workgroup MMT_RECORDS_PART bytes of pieces, which may belong to many records; pieces are joined with
 * raw(a||b) = shift(raw(a), |b|) ^ raw(b).  The same bytes give the same words.  Offsets and lengths are clamped into
 * [0, bytes_len] and nothing at or beyond bytes_len is read, also not by a wide load, whatever the records say; records
 * may overlap.  n = 0 is allowed.  The host variant runs the same functions (csrc/records.h) over HOST memory. */
#define MMT_RECORDS_PIECE 128
#define MMT_RECORDS_PART (256 * MMT_RECORDS_PIECE)
size_t mmt_records_crc_workspace_bytes(int64_t n);    /* host only; 0 for n outside [0, 2^31) */
int mmt_records_crc(const uint8_t* bytes, int64_t bytes_len, int64_t n, const mmt_record* records, uint32_t* crc_out,
                    int32_t* bad_out, void* workspace, size_t workspace_bytes, void* stream);
int mmt_records_crc_host(const uint8_t* bytes, int64_t bytes_len, int64_t n, const mmt_record* records,
                         uint32_t* crc_out, int32_t* bad_out, void* workspace, size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * PNG decode in front of the image front end (csrc/png_decode.hip): `tf.io.decode_image(example['image_data'])` of
 * `decode_fn` (src/data/data_utils.py:195) for PNG bytes, as libpng decodes with palette and low-bit grey expansion and
 * nothing else (no gamma; ancillary chunks ignored; the rules are DESIGN.md section 4, "PNG decode").  The serial part
 * -- the chunk walk and DEFLATE, by the library's own inflate -- runs on the host and yields the filtered scanlines;
 * unfiltering, de-interlacing, bit-depth expansion and the palette lookup run on the device and write the packed
 * layout of the JPEG calls: image b is height x width x 3 bytes, row-major RGB, from pixels_out + pixel_offset.
 *
 * Accepted: colour type 2 at depth 8; colour type 0 (grey: R = G = B, samples scaled by 255 / 85 / 17 / 1) and colour
 * type 3 (palette; an index beyond the palette's entries gives (0, 0, 0)) at depths 1, 2, 4 and 8; interlace methods 0
 * and 1 (Adam7); the five filter types; any number of IDAT chunks split anywhere; stored, fixed and dynamic DEFLATE
 * blocks.  Refused with MMT_E_UNSUPPORTED: depth 16, colour types 4 and 6, a tRNS chunk, an unknown critical chunk, a
 * compression or filter method other than 0, a width or height above 2^30 (a limit of this decode), and whatever does
 * not start with the first byte of a PNG.  MMT_E_INVALID: a wrong signature
 * behind a correct first byte, a CRC-32 mismatch on IHDR / PLTE / IDAT / IEND, truncation, a bad zlib header (preset
 * dictionary, window above 32 KiB), an invalid DEFLATE stream, an Adler-32 mismatch, inflated data shorter or longer
 * than IHDR requires, a filter-type byte above 4, a palette file without PLTE, a PLTE of more than 1 << depth entries
 * or of a length not divisible by 3, a width or height of 0 or above 2^31 - 1.  CRC errors of ancillary chunks and
 * bytes behind IEND are ignored.
 *
 * One struct describes an image to every call.  The info call fills it for a stand-alone image (raw_offset 0,
 * pixel_offset 0); a caller that batches rebases the two offsets.  raw_bytes is the exact inflated size: per non-empty
 * pass, rows x (1 + row bytes); the passes follow each other in Adam7 order (one pass without interlace). */
typedef struct mmt_png_image {
  int32_t width, height;     /* pixels                                                        */
  int32_t bit_depth;         /* 1 | 2 | 4 | 8                                                 */
  int32_t color_type;        /* 0 grey | 2 RGB | 3 palette                                    */
  int32_t interlace;         /* 0 | 1 (Adam7)                                                 */
  int32_t palette_entries;   /* entries of PLTE, 0 without one                                */
  int64_t raw_offset;        /* first byte of the image's filtered scanlines in raw           */
  int64_t raw_bytes;         /* their exact size                                              */
  int64_t pixel_offset;      /* first byte of the image in pixels_out                         */
} mmt_png_image;

/* Host only, no device call, re-entrant, nothing allocated that outlives the call; never reads past len.
 * The info call walks the chunks up to the first IDAT.  The inflate call concatenates the IDAT payloads logically (no
 * copy of the file) and inflates them straight into the caller's HOST memory (pinned, if it is to be uploaded) at
 * raw_out + image->raw_offset; it never writes outside [raw_offset, raw_offset + raw_bytes), which must lie inside
 * [0, raw_capacity).  `image` must describe this stream (as the info call reported it, offsets rebased at will).  It
 * checks the Adler-32, the length and every filter-type byte, and walks on to IEND.  palette_out: uint8 [256][3], the
 * PLTE entries, zero-padded (all zero without a PLTE). */
int mmt_png_info(const uint8_t* bytes, int64_t len, mmt_png_image* out);
int mmt_png_inflate(const uint8_t* bytes, int64_t len, const mmt_png_image* image, uint8_t* raw_out,
                    int64_t raw_capacity, uint8_t* palette_out /* [256][3] */);

/* Stage 2.  The device call takes DEVICE memory throughout (images [B], raw, palettes [B][256][3], pixels_out and the
 * workspace), allocates nothing and does not wait, so it can be recorded into a graph; one launch whatever B is, no
 * atomics, no floating point, bitwise reproducible.  raw is only read: a replay without a new upload gives the same
 * pixels.  The workspace (mmt_png_workspace_bytes(raw_bytes) bytes: the reconstructed last row of a band of 64 rows,
 * per image and pass) needs no initialisation.  raw_bytes and pixels_bytes in [1, 2^60).  Bytes of pixels_out outside
 * every image are not written.  The front end's safety rule holds for every read and write: sizes, offsets, the pass
 * geometry and palette indices that come from `images` or from `raw` are clamped into the buffers, and a filter byte
 * above 4 counts as None -- wrong metadata gives wrong pixels, not a fault -- and the work of a call is bounded by its
 * buffer sizes.  The host variant is the same arithmetic as a plain loop over HOST memory (CPU tensors, host tests, the
 * sanitizer program). */
size_t mmt_png_workspace_bytes(int64_t raw_bytes);             /* host only; 0 for raw_bytes < 1 */
int mmt_png_pixels(int32_t B, const mmt_png_image* images, const uint8_t* raw, int64_t raw_bytes,
                   const uint8_t* palettes, uint8_t* pixels_out, int64_t pixels_bytes, void* workspace,
                   size_t workspace_bytes, void* stream);
int mmt_png_pixels_host(int32_t B, const mmt_png_image* images, const uint8_t* raw, int64_t raw_bytes,
                        const uint8_t* palettes, uint8_t* pixels_out, int64_t pixels_bytes, void* workspace,
                        size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------------
 * PNG inflate on the device (csrc/png_inflate.hip, csrc/png_inflate.h; DESIGN.md section 4, "PNG inflate on the
 * device"): the opt-in replacement of mmt_png_inflate's DEFLATE stage.  The host keeps the chunk walk
 * (mmt_png_gather); one workgroup of 256 threads per image inflates the zlib stream by self-synchronising speculative
 * Huffman decoding with parallel resolution of the LZ77 copies, and makes every check the host inflate makes.  The
 * contract is an equivalence: status_out[b] == 0 exactly when mmt_png_inflate returns MMT_OK on the same file, and
 * then the scanlines are the same bytes.
 *
 * One struct per image describes its compressed bytes. */
typedef struct mmt_png_stream {
  int64_t comp_offset;   /* first byte of the image's zlib stream in comp (the IDAT payloads, concatenated) */
  int64_t comp_bytes;    /* its size, zlib header and everything behind the last block included               */
} mmt_png_stream;

/* status_out[b] of mmt_png_scanlines: 0, or why the stream was refused. */
enum {
  MMT_PNG_ST_OK = 0,
  MMT_PNG_ST_TRUNCATED = 1,      /* the stream ends inside a block, a token or the check value             */
  MMT_PNG_ST_BLOCK_TYPE = 2,     /* reserved block type 3                                                  */
  MMT_PNG_ST_STORED_LEN = 3,     /* the length of a stored block does not match its complement             */
  MMT_PNG_ST_CODE_LENGTHS = 4,   /* a bad code-length set (counts, repeats, over-subscribed, incomplete)    */
  MMT_PNG_ST_BAD_CODE = 5,       /* an unused literal/length or distance code, or a reserved symbol        */
  MMT_PNG_ST_DISTANCE = 6,       /* a distance before the start of the output                              */
  MMT_PNG_ST_TOO_LONG = 7,       /* more output than raw_bytes                                             */
  MMT_PNG_ST_TOO_SHORT = 8,      /* the final block ended before raw_bytes                                 */
  MMT_PNG_ST_ADLER = 9,          /* Adler-32 mismatch                                                      */
  MMT_PNG_ST_FILTER = 10,        /* a filter-type byte above 4                                             */
  MMT_PNG_ST_NO_PROGRESS = 11    /* a round that took no bit (a guard; no stream is known to reach it)     */
};

/* Host only, re-entrant, no device call, never reads past len.  The host work that remains: walks the chunks from the
 * first IDAT to IEND by the rules of mmt_png_inflate and with its messages (CRC-32 of IDAT and IEND, the stream ends at
 * the first gap between IDAT chunks, truncation, tRNS and unknown critical chunks behind the data), copies the IDAT
 * payloads back to back to comp_out + stream->comp_offset (HOST memory, pinned if it is to be uploaded; the payloads
 * are fewer bytes than the file, so len bytes always suffice), validates the two zlib header bytes, sets
 * stream->comp_bytes and fills the palette as mmt_png_inflate does.  It decodes no DEFLATE block.  `image` must
 * describe this file (mmt_png_info).  A refusal here is one mmt_png_inflate makes too. */
int mmt_png_gather(const uint8_t* bytes, int64_t len, const mmt_png_image* image, uint8_t* comp_out,
                   int64_t comp_capacity, mmt_png_stream* stream /* in: comp_offset; out: comp_bytes */,
                   uint8_t* palette_out /* [256][3] */);

/* The device call takes DEVICE memory throughout (images [B], streams [B], comp, raw_out, status_out [B] and the
 * workspace), allocates nothing and does not wait, so it can be recorded into a graph; one launch whatever the
 * arguments are (grid B, 256 threads), no floating point, no atomics, no workgroup waits for another, no scratch; lanes
 * own disjoint output ranges, so the bytes are the same on every run, also for a stream that is refused.  Image b's
 * filtered scanlines go to raw_out + images[b].raw_offset -- the layout mmt_png_pixels reads.  subseq_bytes: the bytes of
 * the stream a lane owns in a round, a power of two in [8, 128].  The return value is about the arguments only: a bad
 * stream is a status.  The front end's safety rule holds: every offset and size of `images`, `streams` and the stream
 * itself is clamped into its buffer, no byte is written outside [raw_offset, raw_offset + raw_bytes) cut to
 * [0, raw_bytes of the call), none is read outside comp, every loop is bounded by the buffer sizes -- wrong metadata or
 * a hostile stream gives a status or wrong bytes, not a fault.  comp_bytes and raw_bytes in [1, 2^60).  The workspace
 * (mmt_png_scanlines_workspace_bytes(B) bytes, no initialisation) holds the group's state for the host variant, which
 * runs the same functions with the 256 lanes as a loop over HOST memory (CPU tensors, host tests, the sanitizer
 * program); the device call keeps that state in LDS and leaves the workspace alone. */
size_t mmt_png_scanlines_workspace_bytes(int32_t B);           /* host only; 0 for B < 1 */
int mmt_png_scanlines(int32_t B, const mmt_png_image* images, const mmt_png_stream* streams, const uint8_t* comp,
                      int64_t comp_bytes, uint8_t* raw_out, int64_t raw_bytes, int32_t* status_out /* [B] */,
                      int32_t subseq_bytes, void* workspace, size_t workspace_bytes, void* stream);
int mmt_png_scanlines_host(int32_t B, const mmt_png_image* images, const mmt_png_stream* streams, const uint8_t* comp,
                           int64_t comp_bytes, uint8_t* raw_out, int64_t raw_bytes, int32_t* status_out /* [B] */,
                           int32_t subseq_bytes, void* workspace, size_t workspace_bytes);

/* Packing short examples into long rows for the train step ("Packed batches").  In: E unpacked
 * examples, word_ids and segment_ids int32 [E, S], lengths int32 [E] (the loaders' valid_len), and up to two position
 * tables int32 [E, n_mlm] / [E, n_mpp] (positions inside the example; either may be NULL).  Out: R rows of S_row positions.
 *
 * Rule (next-fit, arrival order): example i joins the current row if used + len_i <= S_row, otherwise it opens the next
 * row; packing stops before the first example that would open row R, and after E_max examples.  `consumed` examples
 * are taken, always a prefix of the input; packed example e is input example e.
 *
 * Outputs, every element written by every call (nothing needs initialising):
 *   out_word_ids, out_segment_ids  [R, S_row]  the examples' first len positions back to back; tails 0
 *   example_ids, example_starts, patch_slots  [R, S_row]  the layout the packed kernels read (mmt_attn.h,
 *                   MMT_FLAG_EXAMPLE_IDS | MMT_FLAG_EXAMPLE_STARTS; mmt_embed_fwd_packed): ids fall from the row's example
 *                   count to 1 and are 0 in the tail, starts name the first position of the run (the tail is a run),
 *                   the slot is the example's index in the input (every example carries an image), -1 in the tail
 *   first_positions int64 [E_max, 2]   (row, first position); (0, 0) for an absent slot e >= consumed
 *   example_weight  float [E_max]      1 for a consumed example, 0 for an absent slot
 *   out_mlm_positions, out_mpp_positions  [E_max, n_k]  flat indices row * S_row + first + position; 0 for an absent slot
 *   consumed        int32 [1]
 *
 * DEVICE memory throughout, nothing allocated, no host wait, two launches whatever the arguments and the data are (the
 * call records into a graph), no atomics, no floating-point sum: bitwise reproducible.  The plan (prefix sums of the
 * lengths, row ends) runs in ONE workgroup with the lengths in LDS, hence E and E_max <= MMT_PACK_MAX_EXAMPLES; the fill
 * is one thread per output position.  `lengths` and the position tables are data: a length is clamped into [1, S], a
 * position into [0, S), a flat index into [0, R * S_row) -- wrong values give wrong rows, never a stray access.
 * MMT_E_INVALID before any launch: a NULL pointer other than the position tables (a table that is given needs n_k >= 1
 * and its output); E, R or E_max below 1; S < 1 or S_row < S; E or E_max above the limit; E * S or R * S_row at or above
 * 2^31.  MMT_E_WORKSPACE: less than mmt_pack_rows_workspace_bytes (4 * (R + 1 + 2 E) bytes rounded up to 16; 0 for a bad
 * descriptor), caller-owned, no initialisation.  mmt_pack_rows_host runs the same functions (csrc/pack_rows.h) as loops
 * over HOST memory (CPU tensors, the host tests, the sanitizer program). */
#define MMT_PACK_MAX_EXAMPLES 4096
typedef struct mmt_pack_desc {
  int32_t E, S;          /* unpacked examples in, positions of each                */
  int32_t R, S_row;      /* rows out, positions of each                            */
  int32_t E_max;         /* example slots of the per-example outputs               */
  int32_t n_mlm, n_mpp;  /* columns of the two position tables (ignored when NULL) */
  int32_t reserved;
} mmt_pack_desc;

size_t mmt_pack_rows_workspace_bytes(const mmt_pack_desc* desc);
int mmt_pack_rows(const mmt_pack_desc* desc, const int32_t* word_ids, const int32_t* segment_ids, const int32_t* lengths,
                  const int32_t* mlm_positions, const int32_t* mpp_positions, int32_t* out_word_ids,
                  int32_t* out_segment_ids, int32_t* example_ids, int32_t* example_starts, int32_t* patch_slots,
                  int64_t* first_positions, float* example_weight, int32_t* out_mlm_positions, int32_t* out_mpp_positions,
                  int32_t* consumed, void* workspace, size_t workspace_bytes, void* stream);
int mmt_pack_rows_host(const mmt_pack_desc* desc, const int32_t* word_ids, const int32_t* segment_ids, const int32_t* lengths,
                       const int32_t* mlm_positions, const int32_t* mpp_positions, int32_t* out_word_ids,
                       int32_t* out_segment_ids, int32_t* example_ids, int32_t* example_starts, int32_t* patch_slots,
                       int64_t* first_positions, float* example_weight, int32_t* out_mlm_positions, int32_t* out_mpp_positions,
                       int32_t* consumed, void* workspace, size_t workspace_bytes);

/* Random item masking in one launch (csrc/item_masking.hip, csrc/item_masking.h; DESIGN.md section 4, "Masking in one
 * launch"): feature_pipeline.random_item_masking -- tf_text.mask_language_model with a RandomItemSelector and a
 * MaskValuesChooser, the random draws as inputs -- for a padded batch, bit for bit what its torch ops give.
 *
 * In: token_ids int32 [B, T]; n_tokens [B], int64 when desc->n_tokens_i64 is set and int32 otherwise (positions at or
 * beyond it are padding and never count, whatever the other inputs hold there); word_start uint8 [B, T], nonzero at the
 * first token of an item, or NULL (every token is an item); item_keys and value_u float [B, T], entry i for item i of the
 * row; random_ids int32 [B, T], entry t for token t.
 *
 * Definition.  Item of a valid token t: (word starts among the valid tokens [0, t]) - 1, at least 0.  An item is
 * selectable if it has a valid token and none of its valid tokens is one of the n_unselectable ids.  With n of them,
 * n_sel = min(ceil(float(n) * selection_rate), float(max_selections)), the product one fp32 multiplication rounded once.
 * The T keys -- an index that is no selectable item counts as +inf -- are ranked in ascending float order, NaN above
 * everything, -0 equal to +0, the lower index first among equals; a selectable item is chosen when its rank is below
 * n_sel.  A valid token of a chosen item becomes mask_token_id when value_u[item] < mask_threshold, random_ids[t] when
 * value_u[item] < random_threshold, and stays otherwise.  The caller rounds the thresholds to float the way its
 * reference does.
 *
 * Out, every element written by every call: masked int32 [B, T]; positions int32 [B, T], the chosen tokens ascending in
 * the first n_masked[b] entries and 0 behind them; labels int32 [B, T], token_ids at those positions, 0 behind them;
 * n_masked int64 [B].
 *
 * The device call takes DEVICE memory throughout, allocates nothing, takes no workspace and does not wait, so it records
 * into a graph: one launch whatever the arguments and the data are (grid B, 1024 threads, a row's three int32 arrays in
 * LDS: 12 * T + 1104 bytes), no atomics on global memory, no floating-point sum -- bitwise reproducible.  n_tokens is
 * clamped into [0, T]; item indices and compacted positions are counts below T and are clamped again where they become
 * addresses; token_ids and random_ids are values only -- wrong inputs give wrong rows, never a stray access.
 * MMT_E_INVALID before any launch: a NULL pointer other than word_start, B or T below 1, a negative n_unselectable,
 * B * T at or above 2^31.  MMT_E_UNSUPPORTED: T above MMT_MASK_MAX_TOKENS, more than MMT_MASK_MAX_UNSELECTABLE ids.  The
 * host variant runs the same functions (csrc/item_masking.h) as loops over HOST memory (CPU tensors, the host tests, the
 * sanitizer program). */
#define MMT_MASK_MAX_TOKENS 8192
#define MMT_MASK_MAX_UNSELECTABLE 8
typedef struct mmt_item_masking_desc {
  int32_t B, T;
  int32_t max_selections;
  int32_t mask_token_id;
  int32_t n_unselectable;
  int32_t unselectable[MMT_MASK_MAX_UNSELECTABLE];
  int32_t n_tokens_i64;     /* n_tokens is int64 [B] (nonzero) or int32 [B] (0) */
  float selection_rate;
  float mask_threshold;     /* value_u below it: mask_token_id                   */
  float random_threshold;   /* otherwise, value_u below it: the random id        */
  int32_t reserved;
} mmt_item_masking_desc;

int mmt_item_masking(const mmt_item_masking_desc* desc, const int32_t* token_ids, const void* n_tokens,
                     const uint8_t* word_start, const float* item_keys, const float* value_u, const int32_t* random_ids,
                     int32_t* masked, int32_t* positions, int64_t* n_masked, int32_t* labels, void* stream);
int mmt_item_masking_host(const mmt_item_masking_desc* desc, const int32_t* token_ids, const void* n_tokens,
                          const uint8_t* word_start, const float* item_keys, const float* value_u,
                          const int32_t* random_ids, int32_t* masked, int32_t* positions, int64_t* n_masked,
                          int32_t* labels);

#ifdef __cplusplus
}
#endif
#endif /* MMT_LAYER_H_ */
