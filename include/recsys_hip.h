/*
 * recsys_hip.h -- C ABI of librecsys_hip.so, the MI355X (gfx950) hot path for
 * SASRec / BERT4Rec training.
 *
 * The reference (Furyton/Recommender-Baseline-Model, NerualNetwork/bert4rec&sas4rec,
 * "BS/" below) has no native code and no FFI: every op on its hot path is a
 * stock PyTorch module call.  Each entry point here replaces the reference
 * call(s) cited on it; the Python host side (rbm_amd.ops, bound with ctypes)
 * keeps the reference's model/trainer API on top.
 *
 * Conventions (every function):
 *   - raw device pointers + sizes, plus a hipStream_t passed as void*; the
 *     caller passes torch.cuda.current_stream().cuda_stream;
 *   - nothing is allocated or freed; every buffer, including workspace, is
 *     owned by the caller (graph-capturable: no sync, no malloc);
 *   - returns 0 on success, a hipError_t value, or RS_ERR_* (1001 bad argument,
 *     1002 unsupported shape/dtype);
 *   - dtype: 0 = fp32 (parity mode: exact f32-input MFMA), 1 = bf16 (storage
 *     and MFMA operands; fp32 accumulate).  Gradients, LN/softmax statistics,
 *     biases, LN affine params and the loss are always fp32.
 *   - ids are int64 (the reference feeds torch.LongTensor / int64 numpy).
 */
#ifndef RECSYS_HIP_H
#define RECSYS_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define RS_ERR_ARG 1001
#define RS_ERR_UNSUPPORTED 1002

/* Fused GEMM epilogue, applied per output element in this order:
 *   v = alpha*acc (+ bias[n])
 *   act: 1 relu / 2 gelu_tanh (pre-activation stored to aux_out if set),
 *        3 relu_bwd (v *= aux>0), 4 gelu_bwd (v *= gelu'(aux))
 *   dropout: v *= keep(drop_seed, m*drop_ld+n) / (1-drop_p)
 *   v += resid[m*ldres+n];  v *= (rowmask_ids[m] != 0);
 *   post dropout: v *= keep(post_drop_seed, m*drop_ld+n) / (1-post_drop_p);  v += C (accumulate)
 * rows_dev (nullable, device int): only rows m < min(M, *rows_dev) are computed/stored -- the
 * row count of a device-side compaction (BERT labelled rows) without a host sync.           */
typedef struct rs_epilogue {
  const float* bias;
  float alpha;
  int act;
  const void* aux;
  void* aux_out;
  int64_t ldaux;
  float drop_p;
  uint64_t drop_seed;          /* site salt */
  const uint64_t* seed_base;   /* device step seed (nullable) */
  int64_t drop_ld;
  const void* resid;
  int64_t ldres;
  const int64_t* rowmask_ids;
  int accumulate;
  float post_drop_p;
  uint64_t post_drop_seed;
  const int* rows_dev;
} rs_epilogue;

/* C[M,N] = epi(A . B^T).  a_kmajor: A(m,k) at A[k*lda+m] (else A[m*lda+k]);
 * b_kmajor: B(n,k) at B[k*ldb+n] (else B[n*ldb+k]).  c_f32 selects an fp32 C.
 * split_k > 1 writes raw fp32 partials to slab[split_k][M][N] (epi ignored);
 * finish with rs_reduce_slabs.
 * Replaces: nn.Linear / nn.Conv1d(k=1) forward and autograd backward
 *   (BS/models/sas_model/sas.py:10-17, torch F.multi_head_attention_forward
 *   in_proj/out_proj via sas.py:45-47,75; BS/models/bert_modules/attention/
 *   multi_head.py:18-19,29,40; utils/feed_forward.py:10-16; BS/models/bert.py:10,16). */
int rs_gemm(int dtype, int a_kmajor, int b_kmajor, int64_t M, int64_t N, int64_t K,
            const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int c_f32,
            const rs_epilogue* epi, int split_k, float* slab, void* stream);

/* C = epi(LN(X) W^T) with the BERT LayerNorm (variant 1 of rs_layernorm_fwd: gamma (x - mean) / (std_unbiased + eps)
 * + beta) formed in the GEMM's prologue (bf16 X / W / C, K = d = 256, N % 128 == 0; epilogues: bias, bias + GELU
 * (+ dropout, aux_out = the pre-activation)).  h (bf16 [M][ldh]), mean, rinv (fp32 [M]) receive the LayerNorm output
 * and row statistics exactly as rs_layernorm_fwd writes them (each nullable); C is bit-identical to rs_layernorm_fwd
 * + rs_gemm.  RS_ERR_UNSUPPORTED for other shapes / epilogues (the caller runs the two launches).
 * Replaces: utils/sublayer.py:16-18's norm(x) feeding attention/multi_head.py:18-19 (the q/k/v Linears) and
 * utils/feed_forward.py:15-16 (w_1 + GELU + dropout). */
int rs_gemm_ln(int64_t M, int64_t N, int64_t K, const void* X, int64_t ldx, const float* gamma, const float* beta,
               float eps, const void* W, int64_t ldw, void* C, int64_t ldc, const rs_epilogue* epi, void* h,
               int64_t ldh, float* mean, float* rinv, void* stream);

/* out[i] (+)= sum_z slab[z*n+i], fixed order (deterministic split-K finish). */
int rs_reduce_slabs(const float* slab, int splits, int64_t n, float* out, int accumulate, void* stream);
/* Same over slabs of n0+n1 floats: the first n0 columns go to out0, the rest to out1. */
int rs_reduce_slabs2(const float* slab, int splits, int64_t n0, float* out0, int64_t n1, float* out1, int accumulate,
                     void* stream);

/* Weight + bias gradient of a Linear / Conv1d(k=1) layer over M token rows:
 *   dW[N,K] (+)= sum_m dY[m,:]^T X[m,:];   db[N] (+)= sum_m dY[m,:]   (db nullable)
 * split-K over the rows into `splits` fp32 slabs (slab >= splits*(N*K + N) floats), the bias
 * column sums fused into the GEMM, then one deterministic reduce.  accumulate: += into dW/db.
 * rows_dev (nullable, device int): only the first min(M, *rows_dev) rows contribute.
 * Replaces the autograd weight/bias gradients of nn.Linear / nn.Conv1d / in_proj / out_proj
 * (BS/models/sas_model/sas.py:10-17,45-47; BS/models/bert_modules/attention/multi_head.py:18-19;
 * utils/feed_forward.py:10-11; BS/models/bert.py:10). */
int rs_linear_wgrad(int dtype, int64_t M, int64_t N, int64_t K, const void* dY, int64_t lddy, const void* X,
                    int64_t ldx, float* dW, float* db, int accumulate, int splits, float* slab, const int* rows_dev,
                    void* stream);

/* out[n] (+)= sum_m X[m*ldx+n] over M rows (bias gradients).  ws: >= 64*N floats. */
int rs_colsum(int dtype, const void* X, int64_t M, int64_t N, int64_t ldx, float* ws, float* out,
              int accumulate, void* stream);

/* Embedding stage.  mode 0 = SAS (BS/models/sas_model/sas.py:60-67):
 *   x = table[ids]*scale + pos[t]; dropout; x *= (ids != 0)
 * mode 1 = BERT (BS/models/bert_modules/embedding/bert.py:29-31):
 *   x = table[ids] + pos[t]; dropout.        t = row % T, rows = B*T. */
int rs_embed_fwd(int dtype, int mode, const int64_t* ids, int64_t rows, int64_t T, const void* table,
                 const void* pos, int64_t d, float scale, float drop_p, uint64_t seed, const uint64_t* seed_base,
                 void* out, void* stream);
/* dtable[ids[r]] += dX*mask*scale (rows with id 0 skipped: padding_idx=0, fp32 atomics);
 * dpos[t] (+)= sum_b dX[b,t] * mask (deterministic; accumulate flag). */
int rs_embed_bwd(int dtype, int mode, const int64_t* ids, int64_t rows, int64_t T, const void* dx,
                 int64_t d, float scale, float drop_p, uint64_t seed, const uint64_t* seed_base,
                 float* dtable, float* dpos, int accumulate_pos, void* stream);

/* LayerNorm over rows of d.  variant 0 = torch.nn.LayerNorm (biased var,
 * eps in sqrt; BS/models/sas_model/sas.py:39,42,50); variant 1 = BERT custom
 * a2*(x-mean)/(std_unbiased+eps)+b2 (BS/models/bert_modules/utils/layer_norm.py:14-17).
 * Saves mean[M] and rinv[M] (1/sqrt(var+eps), or 1/(std+eps)). */
int rs_layernorm_fwd(int dtype, int variant, const void* X, int64_t ldx, int64_t M, int64_t d,
                     const float* gamma, const float* beta, float eps, void* Y, int64_t ldy,
                     float* mean, float* rinv, void* stream);
/* dX (+)= LN backward; dgamma/dbeta += column sums (deterministic, ws >= 2*d*512 floats). */
int rs_layernorm_bwd(int dtype, int variant, const void* X, int64_t ldx, const void* dY, int64_t lddy,
                     int64_t M, int64_t d, const float* gamma, const float* mean, const float* rinv, float eps,
                     void* dX, int64_t lddx, int accumulate_dx, float* dgamma, float* dbeta, float* ws,
                     void* stream);
/* The affine-gradient partial count of rs_layernorm_bwd's vectorised path (d a multiple of 8 bf16 / 4 fp32 with
 * 16-byte aligned rows and leading dimensions): with dgamma = dbeta = NULL it leaves ws[nparts][2][d] (gamma
 * terms, then beta terms) unreduced, for a later grouped reduction (rs_reduce_segments / rs_wgrad_grouped's extra
 * segments).  0 = the shape takes the other path (pass dgamma/dbeta). */
int64_t rs_layernorm_bwd_nparts(int dtype, int64_t M, int64_t d);
/* rs_layernorm_bwd followed by the dropout site(s) that consume dX, in one launch (vectorised path; other shapes
 * run the two launches): out2 == NULL -- out1 = drop(dX; salt1) as rs_dropout_rowmask without a row mask;
 * else out1 = drop(dX; salt1), out2 = drop(out1; salt2) as rs_dropout2.  dX as stored (accumulated) is the
 * input; hash index row * d + column; out1/out2 dense [M][d].  (BERT: bert_modules/utils/sublayer.py:18 and
 * transformer.py:32 backward.) */
int rs_layernorm_bwd_drop(int dtype, int variant, const void* X, int64_t ldx, const void* dY, int64_t lddy,
                          int64_t M, int64_t d, const float* gamma, const float* mean, const float* rinv, float eps,
                          void* dX, int64_t lddx, int accumulate_dx, float* dgamma, float* dbeta, float* ws,
                          float drop_p, uint64_t salt1, uint64_t salt2, const uint64_t* seed_base, void* out1,
                          void* out2, void* stream);

/* Fused scaled-dot-product attention per (sequence, head), T keys, head dim Dh.
 * q/k/v/o rows are tokens (b*T + t); head h occupies columns [h*Dh, (h+1)*Dh).
 * mask_kind 0 = causal, -inf above the diagonal (SAS, sas.py:70 + torch MHA baddbmm);
 * mask_kind 1 = key padding, scores of keys with ids==0 replaced by -1e9 (BERT,
 * bert_modules/bert.py:38 + attention/single.py:28).  S = scale * q.k^T;
 * P = softmax(S); P = dropout(P); O = P.v.  lse[(b*H+h)*T + t] = row logsumexp.
 * Dropout keep(seed, idx) of P[b,h,q,k] uses idx = ((b*H + h)*T + q)*Tp + k, Tp = T + (T & 1) (even row
 * pitch), i.e. rs_dropout_rowmask over a (B*H*T, Tp) tensor draws the same mask (tests materialise it). */
int rs_attn_fwd(int dtype, int64_t B, int64_t T, int64_t H, int64_t Dh, const void* q, int64_t ldq,
                const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo, float* lse,
                float scale, int mask_kind, const int64_t* ids, float drop_p, uint64_t seed,
                const uint64_t* seed_base, void* stream);
/* Backward: dq, dk, dv (overwritten).  ws: >= B*H*T floats (row deltas).  mask_kind | RS_ATTN_DELTA_IN: ws
 * already holds delta[(b*H+h)*T + t] = rowsum(dO * O) over the head's columns (rs_sas_block_out_bwd_delta with o
 * and delta given forms it); the bf16 LDS path then reads neither O nor recomputes it (other paths recompute it into ws). */
#define RS_ATTN_DELTA_IN 0x100
/* delta[(b*H+h)*T + t] = rowsum over head h's Dh columns of dout * o (values as stored; dtype as rs_attn_bwd) --
 * the RS_ATTN_DELTA_IN input when no fused kernel forms it (BERT: after the output projection's input gradient,
 * bert_modules/attention/multi_head.py + single.py reversed). */
int rs_attn_row_delta(int dtype, int64_t B, int64_t T, int64_t H, int64_t Dh, const void* dout, int64_t lddo,
                      const void* o, int64_t ldo, float* delta, void* stream);
int rs_attn_bwd(int dtype, int64_t B, int64_t T, int64_t H, int64_t Dh, const void* q, int64_t ldq,
                const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o, int64_t ldo,
                const void* dout, int64_t lddo, const float* lse, void* dq, int64_t lddq, void* dk,
                int64_t lddk, void* dv, int64_t lddv, float scale, int mask_kind, const int64_t* ids,
                float drop_p, uint64_t seed, const uint64_t* seed_base, float* ws, void* stream);

/* SAS sampled tied logits (sas.py:93-100): pl[m] = <f[m], E[pos[m]]>, nl likewise (fp32 out). */
int rs_sampled_logits_fwd(int dtype, const void* f, int64_t M, int64_t d, const void* E,
                          const int64_t* pos, const int64_t* neg, float* pl, float* nl, void* stream);
/* df[m] (+)= dpl*E[pos]+dnl*E[neg];  dE[pos] += dpl*f, dE[neg] += dnl*f (id 0 skipped). */
int rs_sampled_logits_bwd(int dtype, const void* f, int64_t M, int64_t d, const void* E,
                          const int64_t* pos, const int64_t* neg, const float* dpl, const float* dnl,
                          void* df, int accumulate_df, float* dE, void* stream);
/* SAS loss (BS/trainers/sas.py:40-49): mean BCEWithLogits(pl,1) + mean BCEWithLogits(nl,0)
 * over valid = (pos != 0).  Writes out[0] = sum of terms, out[1] = count, out[2] = loss
 * (= pos_sum/count + neg_sum/count, count taken from count_override if non-null -- the DP
 * global count), out[3] = neg_sum.  out needs 4 floats; ws >= 3*256 floats. */
int rs_bce_fwd(const float* pl, const float* nl, const int64_t* pos, int64_t M, const float* count_override,
               float* ws, float* out, void* stream);
/* dpl, dnl = dloss * (sigmoid(x) - y) / count on valid positions, 0 elsewhere. */
int rs_bce_bwd(const float* pl, const float* nl, const int64_t* pos, int64_t M, const float* count,
               const float* dloss, float* dpl, float* dnl, void* stream);

/* BERT loss (BS/trainers/bert.py:36-40): CrossEntropyLoss(ignore_index=0) over
 * R rows of V1 fp32 logits (leading dim ldl).  out[0] = sum of -log p(label),
 * out[1] = count, out[2] = loss (count_override as in rs_bce_fwd).
 * ws >= 3*R floats (row lse + partials).  rows_dev (nullable): rows >= *rows_dev are skipped (the
 * tail of a labelled-row compaction, see rs_compact_rows). */
int rs_ce_fwd(const float* logits, int64_t R, int64_t V1, int64_t ldl, const int64_t* labels,
              const float* count_override, float* ws, float* out, const int* rows_dev, void* stream);
/* dlogits (may alias logits) = dloss * (softmax - onehot)/count on labelled rows, 0 else; dtype of
 * dlogits selected by dtype (fp32 or bf16 copy for the following GEMMs). */
int rs_ce_bwd(int dtype, const float* logits, int64_t R, int64_t V1, int64_t ldl, const int64_t* labels,
              const float* count, const float* dloss, const float* ws, void* dlogits, int64_t lddl,
              const int* rows_dev, void* stream);

/* Labelled-row compaction for the BERT loss head (BS/trainers/bert.py:36-40 drops label-0 rows).
 * idx[i] = i-th row with labels != 0 (ascending, i < cap), rank[r] = position of row r in idx or -1,
 * *count = min(#labelled, cap) -- all on the device (the count bounds later GEMMs via rows_dev). */
int rs_compact_rows(const int64_t* labels, int64_t n, int64_t cap, int32_t* idx, int32_t* rank, int32_t* count,
                    void* stream);
/* dst[i,:] = src[idx[i],:] for i < *count, zero rows up to cap; lab_out[i] = labels[idx[i]] (0 beyond). */
int rs_gather_rows(int dtype, const void* src, int64_t lds, int64_t d, const int32_t* idx, const int32_t* count,
                   int64_t cap, void* dst, int64_t ldd, const int64_t* labels, int64_t* lab_out, void* stream);
/* dst[r,:] = rank[r] >= 0 ? src[rank[r],:] : 0 for r < n (the hidden-state gradient scattered back). */
int rs_scatter_rows(int dtype, const void* src, int64_t lds, int64_t d, const int32_t* rank, int64_t n, void* dst,
                    int64_t ldd, void* stream);

/* dst[r] = rank[r] >= 0 ? sum_z slab[z][rank[r]][:] : 0 (cast to dtype) for r < n: the split-K partials
 * (slab[splits][cap][d] fp32, rs_gemm split_k of a compacted-row GEMM) reduced, cast and scattered back
 * to the token rows in one pass (replaces rs_reduce_slabs + rs_cast_bf16 + rs_scatter_rows). */
int rs_splitk_scatter_rows(int dtype, const float* slab, int splits, int64_t cap, int64_t d, const int32_t* rank,
                           int64_t n, void* dst, int64_t ldd, void* stream);

/* Large-tile bf16 GEMM with a 256-wide output (gemm_n256.hip; the vocabulary head's weight-sized products at
 * d = 256, BS/models/bert.py:10,16 + BS/trainers/bert.py:36-40): C[m][0..256) = sum_k A(m, k) B(k, n), fp32 out.
 * A(m, k) = A[k*lda + m] (a_kmajor: dE = dlogits^T h) or A[m*lda + k] (dh = dlogits E); B(k, n) = B[k*ldb + n].
 * colsum (a_kmajor only, nullable): colsum[m] = sum_k A(m, k) (the bias gradient).  rows_dev (nullable, device int):
 * bounds K (a_kmajor) or M (else) -- the labelled-row count of a compacted batch.  split != 0 splits K into
 * rs_gemm_n256_splits(M, K) slices written to C + z * c_split_stride (fp32 partial slabs).  16-B aligned operands,
 * lda / ldb multiples of 8. */
int rs_gemm_n256_splits(int64_t M, int64_t K);
int rs_gemm_n256(int a_kmajor, int64_t M, int64_t K, const void* A, int64_t lda, const void* B, int64_t ldb, float* C,
                 int64_t ldc, int split, int64_t c_split_stride, float* colsum, const int* rows_dev, void* stream);

/* Eval scores at candidate ids (replaces SAS.predict's item_emb(candidates).matmul(final_feat), BS/models/sas_model/
 * sas.py:107-118, and BERTTrainer.calculate_metrics' logits[:, -1, :].gather(1, candidates), BS/trainers/bert.py:
 * 43-49): out[b][c] = <h[b*ldh .. + d], E[cand[b][c]]> (+ bias[cand[b][c]] when bias != NULL), fp32.  h, E in dtype
 * (RS_DTYPE_*); cand int64 [B][C] in [0, V) (others score NaN). */
int rs_candidate_scores(int dtype, const void* h, int64_t ldh, int64_t B, int64_t d, const void* E, const float* bias,
                        const int64_t* cand, int64_t C, int64_t V, float* out, void* stream);

/* torch.optim.Adam step (BS/trainers/base.py:225-228; amsgrad=False) over a
 * flat fp32 buffer.  hyper (device double[5]) = {lr, beta1, beta2, eps, weight_decay} (doubles, as torch's Python
 * floats: the scalars are formed in double and cast to float where they meet the tensors, like torch's).
 * state (device double[8]; double[144] for rs_adam_prepare_step; zero-initialised): rs_adam_prepare does state[0] += 1 (the step count t)
 * and forms state[1] = float(lr/(1-beta1^t)), state[2] = float(sqrt(1-beta2^t)) (double math), state[3] = 1/(*grad_divisor) (1 when null: the
 * data-parallel step all-reduces UNnormalised gradients plus the valid-position count and
 * divides here, so the summed gradient equals the single-device mean's).  rs_adam_step then
 * updates (grad scaled by state[3])
 * p, m, v (and writes the bf16 copy of p to p_bf16 when non-null); zero_grad != 0 also clears g
 * (the next step's accumulation starts from zero without a separate fill).  rs_adam_prepare
 * also advances *seed_base when non-null (the next step's dropout masks, as rs_seed_advance).
 * rs_adam_prepare_step = rs_adam_prepare + rs_adam_step in ONE launch (every workgroup derives step
 * t's scalars; the last to finish publishes them; state[7] and state[16 + 16 k], k < 8, are its arrival
 * counters and must be 0 between launches); further ranges of the same step then use rs_adam_step.  ntd > 0 (with p_bf16): the bf16
 * result is also written TRANSPOSED for ntd matrices of the buffer, tdesc (device int64 [ntd][6]) = rows,
 * cols, src_off (element offset of the matrix in the flat buffer whose element tbase is p[0]), lds
 * (% 4 == 0), dst_off, ldd: wT[dst_off + c*ldd + r] = bf16(p[src_off + r*lds + c]) (rs_transpose_bf16's
 * output, so the SAS backward's transposed weights need no separate launch).  Same results bit for bit. */
int rs_adam_prepare(double* state, const double* hyper, const float* grad_divisor, uint64_t* seed_base,
                    void* stream);
int rs_adam_step(int64_t n, float* p, float* g, float* m, float* v, void* p_bf16,
                 const double* state, const double* hyper, int zero_grad, void* stream);
/* rs_adam_step on at most max_wg workgroups (grid-stride; same results bit for bit): a range updated on a side
 * stream beside other kernels (BERT's out.weight during the encoder backward) takes a bounded share of the CUs.
 * Replaces the same torch.optim.Adam step (BS/trainers/base.py:225-228) over that range. */
int rs_adam_step_wg(int64_t n, float* p, float* g, float* m, float* v, void* p_bf16, const double* state,
                    const double* hyper, int zero_grad, int max_wg, void* stream);
int rs_adam_prepare_step(int64_t n, float* p, float* g, float* m, float* v, void* p_bf16, double* state,
                         const double* hyper, int zero_grad, const float* grad_divisor, uint64_t* seed_base,
                         const int64_t* tdesc, int ntd, int64_t tbase, void* wT, void* stream);
/* rs_adam_prepare_step that also writes *loss_out = *loss_sum / *grad_divisor (data parallel: the step's mean
 * loss from the all-reduced gradient tail) in the same launch. */
int rs_adam_prepare_step_loss(int64_t n, float* p, float* g, float* m, float* v, void* p_bf16, double* state,
                              const double* hyper, int zero_grad, const float* grad_divisor, uint64_t* seed_base,
                              const int64_t* tdesc, int ntd, int64_t tbase, void* wT, const float* loss_sum,
                              float* loss_out, void* stream);
/* rs_adam_step_wg / rs_adam_prepare_step_loss over a range holding (part of) a table whose gradient only
 * rs_item_grad_marked writes: table row r is launch element moff + r * 2^dshift (moff may be negative), mrows rows,
 * 5 <= dshift <= 16 (rows of at least 32 elements: a wave tests its rows' marks from one 16-byte window; smaller
 * dshift returns RS_ERR_ARG);
 * a row with row_marks[r] != *epoch has a zero gradient this step, so its gradient is not read (nor cleared: it
 * is zero already).  Same results bit for bit as the unmarked launches.  row_marks == NULL: the unmarked launch.
 * row_marks: 16-byte aligned, (mrows + 15) / 16 * 16 + 16 + 1024 bytes, the bytes past the stamps zero (the
 * sweep's scalar mark loads run up to 16 bytes past a row; unstamped rows' gradient loads read the zero tail).
 * Only valid while nothing but the marked item gradient writes that table's gradient rows (single device, no
 * l2 regulariser, no exchange). */
int rs_adam_step_marked(int64_t n, float* p, float* g, float* m, float* v, void* p_bf16, const double* state,
                        const double* hyper, int zero_grad, int max_wg, const uint8_t* row_marks, const uint8_t* epoch,
                        int64_t moff, int64_t mrows, int dshift, void* stream);
int rs_adam_prepare_step_marked(int64_t n, float* p, float* g, float* m, float* v, void* p_bf16, double* state,
                                const double* hyper, int zero_grad, const float* grad_divisor, uint64_t* seed_base,
                                const int64_t* tdesc, int ntd, int64_t tbase, void* wT, const float* loss_sum,
                                float* loss_out, const uint8_t* row_marks, const uint8_t* epoch, int64_t moff,
                                int64_t mrows, int dshift, void* stream);

/* SASRec's parameter-norm regulariser, BS/trainers/sas.py:51-52 (loss += l2_emb * torch.norm(p) for every
 * parameter p): *loss += l2 * sum_seg ||p_seg||_2 and g += scale * l2 * p / ||p_seg|| (0 where the norm is 0,
 * as torch's norm backward).  desc: device int64 [nchunk][4] = {lo, hi, first chunk of the segment, chunks of
 * the segment} over the flat parameter buffer (chunks of one segment consecutive); ws: fp32 [2 * nchunk]; scale:
 * device float or null (= 1; the data-parallel step passes the global count its optimizer divides by);
 * g and loss nullable.  Deterministic. */
int rs_l2_penalty(const float* p, float* g, const int64_t* desc, int64_t nchunk, float l2, const float* scale,
                  float* ws, float* loss, void* stream);

/* dst_bf16[i] = bf16(src[i]) */
int rs_cast_bf16(int64_t n, const float* src, void* dst, void* stream);

/* out = x * keep(seed, m*drop_ld+n)/(1-p) * (rowmask_ids[m] != 0); also (optional)
 * out_masked = x * (rowmask != 0).  Elementwise backward helper for dropout sites
 * that feed GEMMs (SAS FFN dropout2 + timeline mask, sas.py:17,84). */
int rs_dropout_rowmask(int dtype, const void* x, int64_t M, int64_t N, int64_t ld, float drop_p,
                       uint64_t seed, const uint64_t* seed_base, int64_t drop_ld, const int64_t* rowmask_ids,
                       void* out, void* out_masked, void* stream);

/* Two stacked dropout sites' backward in one pass (bert.py encode_backward: block-output then
 * residual dropout of BERT4Rec's SublayerConnection/TransformerBlock, BS/models/bert_modules/
 * transformer.py:32, utils/sublayer.py:18): out1 = x * keep(salt1)/(1-p),
 * out2 = out1 * keep(salt2)/(1-p), each rounded to the dtype.  N, ld multiples of 8. */
int rs_dropout2(int dtype, const void* x, int64_t M, int64_t N, int64_t ld, float drop_p, uint64_t salt1,
                uint64_t salt2, const uint64_t* seed_base, int64_t drop_ld, void* out1, void* out2, void* stream);

/* ---- BERT vocabulary head + CrossEntropyLoss(ignore_index=0), logits never materialised (bf16;
 * vocab_ce.hip).  Replaces, for the labelled rows of the fused step, rs_gemm (logits = h E^T + b,
 * BS/models/bert.py:16) + rs_ce_fwd + rs_ce_bwd (BS/trainers/bert.py:11,36-40).
 * h [R][d] bf16 (ldh), E [V1][d] bf16 (lde), bias [V1] fp32, labels [R] (0 = ignored), rows_dev:
 * device row count (rows >= it are skipped; nullable).  ws: rs_vocab_ce_ws_numel floats, written by
 * fwd and read by bwd.  fwd: out = {loss sum, labelled count, sum / (count_override or count)};
 * bwd: dlogits [R][V1] bf16 (lddl, 16-B aligned rows) = (softmax - onehot) * (dloss or 1) / count. */
int64_t rs_vocab_ce_ws_numel(int64_t R, int64_t V1);
int rs_vocab_ce_fwd(int64_t R, int64_t V1, int64_t d, const void* h, int64_t ldh, const void* E, int64_t lde,
                    const float* bias, const int64_t* labels, const int* rows_dev, const float* count_override,
                    float* ws, float* out, void* stream);
int rs_vocab_ce_bwd(int64_t R, int64_t V1, int64_t d, const void* h, int64_t ldh, const void* E, int64_t lde,
                    const float* bias, const int64_t* labels, const int* rows_dev, const float* count,
                    const float* dloss, const float* ws, void* dlogits, int64_t lddl, void* stream);

/* ---- vocabulary head, vocabulary-tile-stationary (vocab_head.hip; bf16, d in {64, 128, 256}) -----
 * Same math and workspace layout (rs_vocab_ce_ws_numel) as rs_vocab_ce_fwd/bwd, for the same reference
 * lines (BS/models/bert.py:10,16, BS/trainers/bert.py:11,36-40); one persistent workgroup per CU keeps a
 * 256- (fwd) / 128-entry (bwd) tile of E in LDS and walks every 128-row tile of h against it, so E streams
 * from HBM once and the short d-deep products run back to back instead of one cold tile at a time.
 * rs_vocab_head_fwd: out = {loss sum, labelled count, sum / (count_override or count)}, ws keeps lse.
 * rs_vocab_head_bwd: dlogits [R][V1] bf16 (rows < live count) = (softmax - onehot) * (dloss or 1) / count;
 *   its 16-byte stores may zero a written row's pad columns from V1 to the next multiple of 8 (rs_vocab_ce_bwd
 *   leaves them alone). */
int rs_vocab_head_supported(int64_t d);
int rs_vocab_head_fwd(int64_t R, int64_t V1, int64_t d, const void* h, int64_t ldh, const void* E, int64_t lde,
                      const float* bias, const int64_t* labels, const int* rows_dev, const float* count_override,
                      float* ws, float* out, void* stream);
int rs_vocab_head_bwd(int64_t R, int64_t V1, int64_t d, const void* h, int64_t ldh, const void* E, int64_t lde,
                      const float* bias, const int64_t* labels, const int* rows_dev, const float* count,
                      const float* dloss, const float* ws, void* dlogits, int64_t lddl, int64_t voff, void* stream);
/* Host-only (no launch, no allocation): the form rs_vocab_head_fwd (bwd = 0) / rs_vocab_head_bwd (bwd = 1) take for
 * R rows, V1 classes and width d on a device of `cus` compute units (cus <= 0: the current device's), from the
 * host functions the launchers themselves call; RS_VHEAD_PP is honoured.  out[0] = 1: the ping-pong kernels, 0: the
 * lock-step kernels (RS_VHEAD_PP=0, or a backward whose per-row metadata, 8 bytes per row of a workgroup's row
 * range, does not fit LDS); out[1], out[2] = gridDim.x, gridDim.y; out[3] = row tiles (32 rows ping-pong, 128 rows
 * lock-step) per y-group; out[4] = dynamic LDS bytes. */
int rs_vocab_head_form(int bwd, int64_t R, int64_t V1, int64_t d, int cus, int* out);

/* Vocabulary-sharded head (data-parallel rank r owns rows [v0, v1) of E = out.weight and b;
 * every rank holds the labelled rows h of ALL ranks, all-gathered).  Labels stay absolute vocabulary ids
 * (0 = not labelled); rs_vocab_head_bwd's voff = v0 places E's rows.
 * rs_vocab_shard_lse: per row, log-sum-exp of h E_shard^T + b_shard (0 for unlabelled rows); ws as
 *   rs_vocab_ce_ws_numel(R, v1 - v0).
 * rs_vocab_shard_label_logits: tgt[r] = <h[r], E[label - v0]> + b[label - v0] where this shard holds the label,
 *   else 0 (summed over ranks: every row's label logit).
 * rs_vocab_shard_combine: lse_parts [N][R] (every shard's lse, all-gathered) -> lse [R] over the whole
 *   vocabulary; out = {loss sum, labelled count, mean} of CE over the labelled rows. */
int rs_vocab_shard_lse(int64_t R, int64_t V1s, int64_t d, const void* h, int64_t ldh, const void* E, int64_t lde,
                       const float* bias, const int64_t* labels, float* ws, float* lse, void* stream);
int rs_vocab_shard_label_logits(int64_t R, int64_t d, const void* h, int64_t ldh, const void* E, int64_t lde,
                                const float* bias, const int64_t* labels, int64_t v0, int64_t v1, float* tgt,
                                void* stream);
int rs_vocab_shard_combine(int N, int64_t R, const float* lse_parts, const float* tgt, const int64_t* labels,
                           float* lse, float* out, void* stream);

/* Host-only: the causal attention backward's work plan for (B, T, H) -- per (split < 4, wave < 8, item < 6) a
 * uint32 (valid << 31 | slot << 26 | role << 24 | chunk end << 16 | chunk begin << 8 | tile; attention_lds.hip
 * make_plan) of the dK/dV (dkv = 1) or dQ pass; *nsplit = workgroups per sequence.  Returns RS_ERR_UNSUPPORTED
 * where the kernels fall back to one tile per wave (T < 128 or no plan fits). */
int rs_attn_bwd_plan(int64_t B, int64_t T, int64_t H, int dkv, uint32_t* plan, int* nsplit);
/* Host-only (no GPU call, no allocation): the code path rs_attn_fwd / rs_attn_bwd take for these arguments, from
 * the host functions the launchers themselves call.  out[0] = 1: the LDS-resident kernels (attention_lds.hip;
 * given 16-byte aligned rows), 0: the generic kernels, and then out[1..4] = 0.  out[1] = the forward's workgroups
 * per sequence-head, out[2] = the backward's, out[3] / out[4] = 1 where the dQ / dK/dV pass runs the work plan
 * (rs_attn_bwd_plan), 0 where it deals one tile per wave round robin.  mask_kind without RS_ATTN_DELTA_IN. */
int rs_attn_lds_regime(int dtype, int64_t B, int64_t T, int64_t H, int64_t Dh, int mask_kind, int* out);

/* Kernel stamps (bench.py's in-step timing of the dominant launch; not on the reference's path).
 * While enabled (buf != NULL), rs_attn_bwd (bf16 LDS path), rs_wgrad_grouped and rs_vocab_ce_fwd (its
 * logits GEMM) launches of the kinds in kind_mask (bit RS_STAMP_*) are stamped -- marks numbered in launch order from 0, fixed into the kernel
 * arguments, so a captured graph keeps stamping on every replay.  buf (device u64) = {base step, steps
 * held, marks per step, W, then per (slot = (int64)*step - base, mark) a record {begin, end lanes
 * 0 .. W-1}} in s_memrealtime ticks (begin: the first dispatched workgroup's start; each wave raises
 * end lane (wave index mod W) to its exit time; the launch ends at the max over the lanes).  step: the optimizer's device step count (double, rs_adam_prepare's
 * state[0]).  rs_kernel_stamps(NULL, NULL, 0) disables.  rs_kernel_stamp_count / rs_kernel_stamp_kinds:
 * the marks handed out since the last enable and their kinds.  rs_wall_clock_khz: tick rate. */
#define RS_STAMP_ATTN_BWD 1
#define RS_STAMP_WGRAD_GROUPED 2
#define RS_STAMP_VOCAB_CE_FWD 3   /* the logits GEMM of rs_vocab_ce_fwd / the rs_vocab_head_fwd kernel */
int rs_kernel_stamps(uint64_t* buf, const double* step, int kind_mask);
int rs_kernel_stamp_count(void);
int rs_kernel_stamp_kinds(int* kinds, int n);
int rs_wall_clock_khz(int* khz);

/* *seed_base += 1 on the stream (advances every dropout mask; capturable). */
int rs_seed_advance(uint64_t* seed_base, void* stream);
/* Upload an instantiated step graph (hipGraphExec_t) to the device ahead of its first launch (hipGraphUpload):
 * graph preparation, no step runs.  Infrastructure of the captured training step (BS/trainers/base.py:114-123's
 * loop body replayed as one graph), not a reference op. */
int rs_graph_upload(void* graph_exec, void* stream);

/* ---- fused SAS sublayers (bf16, d in {64, 128}; rowchain.hip) ----------------------------
 * One workgroup per CU stages the block's weights in LDS once, each wave carries 16 tokens
 * through the whole chain in registers.
 * Same outputs, saved tensors and dropout masks as the unfused kernel sequence, so rs_* backward
 * kernels consume them unchanged.
 *
 * Each entry takes the width d, one or two of the argument structs below and the stream.  The structs ARE the
 * kernels' arguments (field order = kernel-argument layout; rs_abi_sizeof reports their sizes).  An entry checks its
 * arguments first (RS_ERR_ARG for a bad value, RS_ERR_UNSUPPORTED for d not in {64, 128}: callers fall back to the
 * unfused sequence) and launches nothing in that case; otherwise it copies the structs BY VALUE into the launch and
 * keeps no pointer to them once it returns (a captured graph replays the copy; the caller may free or reuse the
 * struct at once).  Fields an entry fills itself are marked "set by ..." and are ignored in the caller's struct.
 * [M][d] tensors are bf16, dense (row stride d) and 16-byte aligned unless a stride is named; LayerNorm
 * parameters, biases and row statistics are fp32. */
#ifdef __HIPCC__
typedef __bf16 rs_bf16;
#else
typedef uint16_t rs_bf16;
#endif

/* The embedding stage folded into the first block's input side: x0 = (item_emb[ids]*scale + pos_emb[t]) ->
 * dropout(drop_p, salt) -> *(ids != 0), exactly as rs_embed_fwd mode 0. */
typedef struct rs_sas_embed_args {
  const int64_t* ids;          /* [M] item ids, M % T == 0 */
  const rs_bf16* item_emb;     /* item table [rows][d], 16-byte aligned */
  const rs_bf16* pos_emb;      /* positional table [T][d], 16-byte aligned */
  int64_t T;                   /* sequence length (t = row % T) */
  float scale;
  float drop_p;
  uint64_t salt;               /* dropout site salt */
  const uint64_t* seed_base;   /* device step seed (nullable) */
  rs_bf16* x0;                 /* [M][d] out: the embedding output (the backward's LN1 input), 16-byte aligned */
  const int64_t* count_ids;    /* optional, with count_parts (both or neither): [M] ids to count != 0 */
  int* count_parts;            /* [rs_sas_block_grid(M)] out: per-workgroup counts of count_ids != 0 (the BCE
                                  divisor of rs_sas_head_args) */
} rs_sas_embed_args;

/* Block i's attention input side (BS/models/sas_model/sas.py:73-76):
 *   Q = LN1(x) [mean/rstd saved];  q = Q Wq^T + bq;  kv = x Wkv^T + bkv */
typedef struct rs_sas_in_args {
  int64_t M;                   /* token rows */
  const rs_bf16* x;            /* [M] rows at stride ldx; set by the entry to e.x0 (embed form) / the first struct's
                                  xn (rs_sas_block_out_in) */
  int64_t ldx;                 /* % 8 == 0; set by the entry to d where it sets x */
  const float* ln_w;           /* LN1 affine [d] */
  const float* ln_b;
  float eps;
  rs_bf16* Q;                  /* [M][d] out */
  float* mean;                 /* [M] out */
  float* rstd;                 /* [M] out */
  const rs_bf16* Wq;           /* in_proj_weight[:d] (torch [out][in] layout) */
  const float* bq;
  rs_bf16* q;                  /* [M][d] out */
  const rs_bf16* Wkv;          /* in_proj_weight[d:] */
  const float* bkv;            /* [2d] */
  rs_bf16* kv;                 /* [M][2d] out */
  rs_sas_embed_args e;         /* e.item_emb == NULL: x is read; else the first block's embed form */
} rs_sas_in_args;

/* The SAS head riding in the LAST block's output side (token-local once the BCE divisor c = *divisor or the sum of
 * count_parts is known): f = LN_last(xn) [saved], pl/nl = <f, E[pos]>/<f, E[neg]>, dpl = (sigmoid(pl)-1)/c,
 * dnl = sigmoid(nl)/c on pos != 0 [saved], dx = LN_last'(xn, dpl E[pos] + dnl E[neg]). */
typedef struct rs_sas_head_args {
  const rs_bf16* E;            /* tied item table [rows][d] */
  const int64_t* pos;          /* [M] */
  const int64_t* neg;          /* [M] */
  const float* ln_w;           /* last LayerNorm affine [d] */
  const float* ln_b;
  float eps;                   /* set by the entry to the block's eps */
  const int* count_parts;      /* [ncount] valid-position counts (rs_sas_embed_args.count_parts), required */
  int ncount;                  /* > 0 */
  const float* divisor;        /* optional device scalar: replaces the summed count */
  rs_bf16* f;                  /* [M][d] out */
  float* pl;                   /* [M] out */
  float* nl;
  float* dpl;
  float* dnl;
  rs_bf16* dx;                 /* [M][d] out: dx_L for the blocks' backward.  rs_sas_block_out_head_bwd: the two-launch
                                  path's scratch, not written (set to NULL) by the one-launch kernel and may be NULL
                                  where rs_sas_block_boundary_fused */
  float* lnpart;               /* [G][2][d] out: LN affine partials per workgroup, G = rs_sas_block_grid(M) */
  float* part;                 /* [G][3] out: BCE partials (sum softplus(-pl), sum softplus(nl), count) for
                                  rs_wgrad_grouped_pos_stats */
} rs_sas_head_args;

/* Block i's output side (sas.py:75-84, PointWiseFeedForward sas.py:8-24):
 *   x1 = Q + o Wo^T + bo;  z = LN2(x1);  h1 = relu(drop(z W1^T + b1, salt1));
 *   xn = (drop(h1 W2^T + b2, salt2) + z) * (ids != 0)
 * Dropout element index m*d + n, seeds eff_seed(salt, *seed_base) as rs_gemm's epilogue. */
typedef struct rs_sas_out_args {
  int64_t M;
  const rs_bf16* o;            /* [M][d] attention output */
  const rs_bf16* Q;            /* [M][d] rs_sas_in_args.Q (the residual) */
  const rs_bf16* Wo;           /* out_proj.weight [d][d] */
  const float* bo;
  rs_bf16* x1;                 /* [M][d] out */
  const float* ln_w;           /* LN2 affine [d] */
  const float* ln_b;
  float eps;
  rs_bf16* z;                  /* [M][d] out */
  float* mean;                 /* [M] out (LN2 statistics) */
  float* rstd;
  const rs_bf16* W1;           /* conv1.weight [d][d] */
  const float* b1;
  rs_bf16* h1;                 /* [M][d] out */
  const rs_bf16* W2;           /* conv2.weight [d][d] */
  const float* b2;
  rs_bf16* xn;                 /* [M][d] out: the block's output */
  const int64_t* ids;          /* [M] row mask */
  float drop_p;
  uint64_t salt1;
  uint64_t salt2;
  const uint64_t* seed_base;   /* device step seed (nullable) */
  rs_sas_head_args h;          /* h.E == NULL: no head */
} rs_sas_out_args;

/* Backward of the output side (sas.py:75-84 reversed):
 *   dzres = dxn*(ids!=0); dy2 = drop2(dzres) [out]; da1 = relu'(h1)*drop1(dy2 W2) [out];
 *   dz = da1 W1 + dzres; dx1 = LN2'(x1, dz) [out]; dout = dx1 Wo [out]
 * Replaces rs_dropout_rowmask + 3 rs_gemm dgrads + rs_layernorm_bwd of the unfused sequence.
 * "set from out": rs_sas_block_out_head_bwd copies the field from its rs_sas_out_args. */
typedef struct rs_sas_out_bwd_args {
  int64_t M;
  const rs_bf16* dxn;          /* [M][d] gradient at xn; set by the two-struct entries (the first chain's dx, NULL in
                                  the one-launch kernels) */
  const int64_t* ids;          /* set from out */
  const rs_bf16* h1;           /* set from out */
  const rs_bf16* x1;           /* set from out */
  const float* mean2;          /* LN2 statistics; set from out (mean, rstd) */
  const float* rstd2;
  const float* ln_w;           /* LN2 weight; set from out */
  const rs_bf16* W2T;          /* TRANSPOSED weights ([in][out], rs_transpose_bf16); current when the launch runs */
  const rs_bf16* W1T;
  const rs_bf16* WoT;
  rs_bf16* dy2;                /* [M][d] out */
  rs_bf16* da1;
  rs_bf16* dx1;
  rs_bf16* dout;
  float* part;                 /* [G][2][d] out: LN2 dgamma / dbeta partial set per workgroup, G =
                                  rs_sas_block_grid(M); sum them with rs_reduce_segments / rs_wgrad_grouped (stride
                                  2d, splits G) */
  float drop_p;                /* set from out, with salt1, salt2, seed_base */
  uint64_t salt1;
  uint64_t salt2;
  const uint64_t* seed_base;
  const rs_bf16* o;            /* optional, with delta (both or neither): the attention output [M][d], one head; set
                                  from out (where delta is given) */
  float* delta;                /* [M] out: rowsum(dout * o), the attention backward's row term, so rs_attn_bwd
                                  (mask_kind | RS_ATTN_DELTA_IN, ws = delta) neither reads o nor recomputes it */
} rs_sas_out_bwd_args;

/* Backward of the input side (sas.py:73-76 reversed):
 *   dQ = dq Wq + dx1;  dx = dk Wk + dv Wv + LN1'(x, dQ) [out] */
typedef struct rs_sas_in_bwd_args {
  int64_t M;
  const rs_bf16* dq;           /* [M][d] */
  const rs_bf16* dkv;          /* [M][2d] */
  const rs_bf16* dx1;          /* [M][d] rs_sas_out_bwd_args.dx1 (the residual's gradient) */
  const rs_bf16* x;            /* [M][d] the block's input */
  const float* mean1;          /* LN1 statistics */
  const float* rstd1;
  const float* ln_w;           /* LN1 weight */
  const rs_bf16* WinT;         /* in_proj_weight^T [d][ldwt] */
  int64_t ldwt;                /* must be 3d (RS_ERR_ARG otherwise) */
  rs_bf16* dx;                 /* [M][d] out.  rs_sas_block_in_out_bwd: the two-launch path's scratch, not written (set
                                  to NULL) by the one-launch kernel and may be NULL where rs_sas_block_boundary_fused */
  float* part;                 /* [G][2][d] out: LN1 affine partials, as rs_sas_out_bwd_args.part */
} rs_sas_in_bwd_args;

/* Workgroups the row-chain kernels launch for M token rows = per-workgroup partial sets they write (0 for M <= 0). */
int64_t rs_sas_block_grid(int64_t M);
/* 1 where the two-struct entries below run their one-launch kernels: d in {64, 128} and every wave of the grid owns
 * at most one 16-row tile (M <= 128 * CUs); they launch the two single-chain kernels on the stream otherwise. */
int rs_sas_block_boundary_fused(int64_t M, int64_t d);

/* The input side; with in->e.item_emb the first block's embed form (one launch instead of two; there d not in
 * {64, 128} is RS_ERR_ARG). */
int rs_sas_block_in(int64_t d, const rs_sas_in_args* in, void* stream);
/* The output side; with out->h.E the LAST block's form with the head in the same kernel. */
int rs_sas_block_out(int64_t d, const rs_sas_out_args* out, void* stream);
/* The output side's backward; with out_bwd->o and out_bwd->delta also the attention backward's row term. */
int rs_sas_block_out_bwd_delta(int64_t d, const rs_sas_out_bwd_args* out_bwd, void* stream);
/* The same without o / delta, in the positional form its callers (and the kernel-level tests) use: the arguments are
 * rs_sas_out_bwd_args' fields of the same names. */
int rs_sas_block_out_bwd(int64_t M, int64_t d, const void* dxn, const int64_t* ids, const void* h1, const void* x1,
                         const float* mean2, const float* rstd2, const float* ln_w, const void* W2T, const void* W1T,
                         const void* WoT, void* dy2, void* da1, void* dx1, void* dout, float* part, float drop_p,
                         uint64_t salt1, uint64_t salt2, const uint64_t* seed_base, void* stream);
int rs_sas_block_in_bwd(int64_t d, const rs_sas_in_bwd_args* in_bwd, void* stream);
/* Block-boundary launches: two adjacent row chains of the step in ONE launch, the tensor handed from the first to the
 * second kept in registers.  Results are bitwise those of the two entries called back to back, for every M (both
 * structs' M must agree).
 *   rs_sas_block_out_in: rs_sas_block_out of block i (no head; every saved tensor still stored, xn included: it is
 *     block i+1's saved input), then rs_sas_block_in(x = out->xn) of block i+1 (no embed form).
 *   rs_sas_block_in_out_bwd: rs_sas_block_in_bwd of block i, then rs_sas_block_out_bwd_delta(dxn = in_bwd->dx) of block
 *     i-1.  In the one-launch kernel dx is NOT written (RS_ERR_ARG if it is NULL and needed). */
int rs_sas_block_out_in(int64_t d, const rs_sas_out_args* out, const rs_sas_in_args* in, void* stream);
int rs_sas_block_in_out_bwd(int64_t d, const rs_sas_in_bwd_args* in_bwd, const rs_sas_out_bwd_args* out_bwd,
                            void* stream);
/* The forward/backward turnaround of the fused training step: rs_sas_block_out of the LAST block with its head
 * (required) and, on the same rows, that block's rs_sas_block_out_bwd_delta(dxn = out->h.dx) in ONE launch: dx_L, h1, x1, o
 * and the row statistics pass from the forward chain to the backward chain in registers.  Bitwise the two entries
 * called back to back, for every M; every output of either is written except out->h.dx in the one-launch kernel
 * (RS_ERR_ARG if it is NULL and needed).  Of out_bwd the caller gives M, W2T, W1T, WoT, dy2, da1, dx1, dout, part and
 * delta (optional); the other fields are set from out. */
int rs_sas_block_out_head_bwd(int64_t d, const rs_sas_out_args* out, const rs_sas_out_bwd_args* out_bwd,
                              void* stream);

/* The first block's embed-form input side and its attention forward (one head, causal) in ONE launch
 * (block_in_attn.hip): rs_sas_block_in(in, embed form) followed by rs_attn_fwd(q = in.q, k / v = the halves of in.kv,
 * mask_kind 0, seed = salt, seed_base = in.e.seed_base) on B sequences of in.e.T rows, bit for bit, for every tensor
 * either writes.  The grid is the attention forward's; each workgroup forms its sequence's K/V image in LDS with the
 * row chain's stages, so nothing is reloaded across a launch boundary. */
typedef struct rs_sas_in_attn_args {
  rs_sas_in_args in;           /* the embed form (in.e.item_emb required); M = B * in.e.T; x / ldx set by the entry */
  int64_t B;                   /* sequences */
  rs_bf16* o;                  /* [M][d] out: the attention output, 16-byte aligned */
  float* lse;                  /* [M] out: row logsumexp */
  float scale;                 /* score scale (1 / sqrt(d)) */
  float drop_p;                /* attention dropout */
  uint64_t salt;               /* its site salt (rs_attn_fwd's seed) */
  int64_t ncount;              /* slots of in.e.count_parts, >= nsplit * B: EVERY slot is written (workgroup counts,
                                  then zeros), so rs_sas_head_args.count_parts may be summed over all of them */
} rs_sas_in_attn_args;
/* Host-only: the workgroups per sequence of rs_sas_block_in_attn for (d, B, T), or 0 where it does not cover the
 * shape and returns RS_ERR_UNSUPPORTED (d not in {64, 128}; T or the dropout index outside the LDS attention's range;
 * more than 8 query tiles per workgroup; the images and one weight slot beyond the 160 KB of LDS). */
int rs_sas_block_in_attn_nsplit(int64_t d, int64_t B, int64_t T);
/* RS_ERR_ARG (nothing launched) for a NULL or misaligned tensor, M != B * in.e.T, count_ids without count_parts (or
 * the reverse) or ncount < nsplit * B. */
int rs_sas_block_in_attn(int64_t d, const rs_sas_in_attn_args* args, void* stream);

/* Union-of-touched-rows exchange of an embedding-table gradient (sparse_rows.hip; data parallel,
 * replaces the dense all-reduce of the token / item table gradient -- the reference has no
 * multi-GPU path, BS/trainers/base.py:32-34).  rs_touched_rows: flags[v] = (v occurs in ids[0..n)),
 * index[v] = rank of v among flagged rows (ascending) or -1, *count = flagged rows; flags/index int32[rows],
 * ws int32[rs_touched_rows_ws_numel(rows)].  rs_rows_pack: compact[index[v]][:] = src[v][:] for flagged v,
 * compact rows [*count, cap) zeroed (cap >= *count).  rs_rows_unpack: dst[v][:] = compact[index[v]][:].
 * fp32 rows of d (d % 4 == 0, 16-B aligned). */
int64_t rs_touched_rows_ws_numel(int64_t rows);
int rs_touched_rows(const int64_t* ids, int64_t n, int64_t rows, int32_t* flags, int32_t* index, int32_t* count,
                    int32_t* ws, void* stream);
int rs_rows_pack(const float* src, int64_t rows, int64_t d, const int32_t* index, const int32_t* count,
                 float* compact, int64_t cap, void* stream);
int rs_rows_unpack(float* dst, int64_t rows, int64_t d, const int32_t* index, const float* compact, void* stream);

/* Sparse (touched-rows-only) Adam of an embedding / output table (adam_rows.hip): the lazy rule of torch's
 * SparseAdam / TensorFlow's LazyAdam in the dense sweep's arithmetic -- the reference's optimizer is the dense
 * torch.optim.Adam (BS/trainers/base.py:225-228), which rs_adam_step replaces; this one is an opt-in for sampled
 * losses whose step touches few rows of a large table.
 * rs_unique_rows: rows[0 .. *count) = the distinct keys in [1, table_rows) of up to three int64 key arrays (keysK
 * may be NULL when nK == 0), ascending; keys of 0 or >= table_rows (or negative) are dropped; entries past *count
 * are unspecified.  cap (the capacity of rows[]) >= n0 + n1 + n2.  ws: rs_unique_rows_ws_bytes(table_rows) =
 * 4 * (table_rows + 2 * ceil(table_rows / 2048)) bytes, 4-byte aligned -- ints per table row, nothing per row
 * element; needs no initialisation.  No host synchronisation (graph-capturable), no atomics: the same key set gives
 * the same list.  table_rows < 2^31.
 * rs_adam_rows: for i < min(*count, cap), row r = rows[i] of the table whose row 0 p / g / m / v / p_bf16 point at
 * (d fp32 per row; p_bf16 NULL in fp32 mode) gets rs_adam_step's per-element update with the step's scalars in
 * state[1..3] -- so it runs after the step's rs_adam_prepare / rs_adam_prepare_step launch on the same stream -- and
 * its gradient is cleared when zero_grad; bit for bit what rs_adam_step gives on those rows.  Every other row is
 * neither read nor written.  A row id outside [0, table_rows) is skipped; the listed ids must be distinct.  16-byte
 * accesses when d % 4 == 0 and the bases are 16-byte (p_bf16: 8-byte) aligned, else element by element (d = 50,
 * d = 1).  At most max_wg workgroups, grid-stride over the list; cap * d < 2^31. */
int64_t rs_unique_rows_ws_bytes(int64_t table_rows);
int rs_unique_rows(const int64_t* keys0, int64_t n0, const int64_t* keys1, int64_t n1, const int64_t* keys2,
                   int64_t n2, int64_t table_rows, int32_t* rows, int32_t* count, int64_t cap, void* ws,
                   int64_t ws_bytes, void* stream);
int rs_adam_rows(int64_t d, int64_t table_rows, const int32_t* rows, const int32_t* count, int64_t cap, float* p,
                 float* g, float* m, float* v, void* p_bf16, const double* state, const double* hyper, int zero_grad,
                 int max_wg, void* stream);

/* torch.optim.SGD step (sgd.hip): the reference trainer's other optimizer, BS/trainers/base.py:229-233
 * (args.optimizer == "SGD": optim.SGD(params, lr, weight_decay=args.weight_decay, momentum=args.momentum); dampening
 * 0, nesterov False), over n elements of a flat fp32 buffer, one launch.  hyper (device double[3]) = {lr, momentum,
 * weight_decay}: doubles as torch's Python floats, cast to float where they meet the tensors.  Per element, every
 * rounding as torch's float32 kernels place it (sgd_math.h):
 *     gj = (gs == 1) ? g : g * gs                  gs = 1 / *grad_divisor (data parallel), 1 when it is NULL
 *     if (wd != 0) gj = fma(wd, p, gj)             grad.add(param, alpha=weight_decay)
 *     if (buf)     b  = (b * momentum) + gj        buf.mul_(momentum).add_(grad): two roundings, no fma
 *                  p  = fma(-lr, buf ? b : gj, p)  param.add_(buf, alpha=-lr)
 * A zero-initialised buf gives torch's first-step rule (buf = grad.clone()) from the same line.  With gs == 1 the
 * result equals torch's CPU float32 SGD bit for bit.
 * buf == NULL: the momentum-free form -- no buffer is read or written and hyper[1] is ignored.  p_bf16 (NULL in fp32
 * mode) receives bf16(p); zero_grad != 0 clears g (stores only where it is not zero already).  ntd > 0: the bf16
 * result is also written transposed, tdesc / tbase / wT as rs_adam_prepare_step's (lds % 4 == 0, every matrix inside
 * [tbase, tbase + n / 4 * 4), rows * lds < 2^31: the caller's promise).  At most max_wg workgroups, grid-stride
 * (0 = one float4 per thread, unbounded); every grid gives the same bits.
 * prepare != 0 marks the first range of a step: that launch also does state[0] += 1 (state: device double[>= 1], the
 * step count kernel stamps and checkpoints read), *seed_base += 1 when given (the next step's dropout masks), and
 * *loss_out = *loss_sum / *grad_divisor when given.  Nothing in the kernel reads those three, so further ranges of
 * the step (prepare == 0) may follow in any order on the same stream.  Every launch reads grad_divisor itself.
 * RS_ERR_ARG before any launch: n <= 0; NULL p, g, state or hyper; p, g or buf not 16-byte (p_bf16: 8-byte) aligned;
 * ntd < 0, or ntd > 0 without p_bf16, tdesc and wT; loss_out without loss_sum and grad_divisor; max_wg < 0.
 * No allocation, no synchronisation, no atomics: graph-capturable and deterministic. */
int rs_sgd_step(int64_t n, float* p, float* g, float* buf, void* p_bf16, double* state, const double* hyper,
                int zero_grad, int prepare, const float* grad_divisor, uint64_t* seed_base, const int64_t* tdesc,
                int ntd, int64_t tbase, void* wT, const float* loss_sum, float* loss_out, int max_wg, void* stream);

/* Global gradient norm and clip coefficient (gradnorm.hip): torch.nn.utils.clip_grad_norm_(parameters, max_norm,
 * error_if_nonfinite=False) for a step whose backward and optimizer are one captured launch sequence.  The partial
 * launches write double partial sums of squares into consecutive slots of one workspace, rs_gradnorm_finish reduces
 * them; everything accumulates in double (the square of an fp32 is exact there).  The arithmetic of a range / list is
 * fixed by its length alone: max_wg (>= 1) only bounds the launch's workgroups and changes no bit, and the same
 * inputs give the same bits run to run, eager or replayed.  No allocation, no synchronisation, no atomics.
 * rs_gradnorm_dense: ranges (HOST int64 [nranges][2], 1 <= nranges <= 8) = {lo, hi} element ranges of g (16-byte
 * aligned, lo % 4 == 0, hi > lo; inside the buffer: the caller's promise); 16-byte loads and a scalar tail of
 * (hi - lo) % 4 elements.  Range r writes rs_gradnorm_dense_parts(hi - lo) slots (at most 2048), the ranges' slots
 * back to back from partials[0].
 * rs_gradnorm_rows: the rows rows[0 .. min(*count, cap)) (rs_unique_rows' list and device count) of the table [R][d]
 * whose row 0 g points at, d >= 1 (a bias vector is a d = 1 table); no other row is read; an id outside
 * [0, table_rows) is skipped.  16-byte loads when d % 4 == 0 and g is 16-byte aligned, else element by element.
 * Writes ALL rs_gradnorm_rows_parts(d, cap) slots (at most 1024) every launch, zeros where the list is short.
 * cap * d < 2^31.
 * rs_gradnorm_finish: s = the sum of partials[0 .. nparts) (nparts <= 2^24), norm = sqrt(s) / *div (div NULL: 1),
 * coef = float(*max_norm / (norm + 1e-6)) clamped at 1 (torch's formula; *max_norm a device double, so it may change
 * between graph replays; +inf never clips), record (device float[3]) = {norm, coef, effective divisor}: the divisor
 * is *div itself (bit for bit) when coef == 1, else *div * (norm + 1e-6) / *max_norm -- the optimizer entries take
 * &record[2] as their grad_divisor.  A non-finite sum gives coef 0 or NaN, which is applied; the record reports the
 * norm.
 * RS_ERR_ARG before any launch: NULL or misaligned g / partials / max_norm / record, nranges outside [1, 8], a range
 * with hi <= lo or lo % 4, d < 1, table_rows < 1, cap < 1, cap * d >= 2^31, max_wg < 1, nparts < 1.  The *_parts
 * helpers return -1 for such arguments. */
int64_t rs_gradnorm_dense_parts(int64_t n);
int64_t rs_gradnorm_rows_parts(int64_t d, int64_t cap);
int rs_gradnorm_dense(const float* g, const int64_t* ranges, int nranges, int max_wg, double* partials,
                      void* stream);
int rs_gradnorm_rows(const float* g, int64_t d, int64_t table_rows, const int32_t* rows, const int32_t* count,
                     int64_t cap, int max_wg, double* partials, void* stream);
int rs_gradnorm_finish(const double* partials, int64_t nparts, const float* div, const double* max_norm,
                       float* record, void* stream);

/* Batched bf16 transpose: for m < nmat, desc[6m..6m+5] = {rows, cols, src_off, lds, dst_off, ldd}
 * (elements): dst[dst_off + c*ldd + r] = src[src_off + r*lds + c].  Grid x = max_tiles >= the
 * largest ceil(rows/64)*ceil(cols/64). */
int rs_transpose_bf16(int64_t nmat, const int64_t* desc, int64_t max_tiles, const void* src, void* dst,
                      void* stream);

/* ---- grouped weight gradients (wgrad.hip) ---------------------------------------------------
 * Every Linear / Conv1d(k=1) weight gradient of a backward pass, dW[N][K] += dY^T X and
 * db[N] += colsum(dY) over the M token rows (the autograd accumulation of nn.Linear's backward,
 * BS/models/sas_model/sas.py:8-24,67-84; bert_modules/...), in ONE GEMM launch (problems x output
 * tiles x row splits) followed by ONE deterministic grouped reduction of the split partials.
 * bf16 dY/X (16-byte aligned, ld % 8 == 0), fp32 dW/db accumulated; N, K multiples of 64. */
typedef struct {
  const void* dY; int64_t lddy;   /* [M][N] bf16 */
  const void* X;  int64_t ldx;    /* [M][K] bf16 */
  int64_t N, K;
  float* dW;                      /* [N][K] fp32, += */
  float* db;                      /* [N] fp32, += (or NULL) */
} rs_wgrad_problem;
/* A partial-sum set: out[i] (+)= sum_{z < splits} src[z*stride + i], i < n (n, stride multiples
 * of 4; src/out 16-byte aligned). */
typedef struct {
  const float* src; int64_t stride; int64_t splits; int64_t n; float* out;
} rs_reduce_segment;
/* slab floats needed by rs_wgrad_grouped for these problems (splits = ceil(M / rows_per_split)). */
int64_t rs_wgrad_grouped_slab_numel(int nprob, const rs_wgrad_problem* probs, int64_t M, int64_t rows_per_split);
/* output tile edge rs_wgrad_grouped uses for these problems (reads N and K only): 256 when every N and K is a
 * multiple of 256 (the BERT d = 256 layer's weights), else 128 or 64; -1 on bad arguments.  Callers size the row
 * splits by it (about one 256-tile workgroup per CU in total). */
int rs_wgrad_grouped_tile(int nprob, const rs_wgrad_problem* probs);
/* the same with the tile edge capped at max_tile (>= 64) */
int rs_wgrad_grouped_tile_max(int nprob, const rs_wgrad_problem* probs, int max_tile);
/* nprob <= 16 problems; rows_per_split % 64 == 0; the extra segments (<= 64, e.g. LayerNorm
 * affine partials from rs_sas_block_*_bwd) are summed into their outputs (+=) by the same
 * reduction launch.  Returns RS_ERR_UNSUPPORTED for shapes outside the contract. */
int rs_wgrad_grouped(int nprob, const rs_wgrad_problem* probs, int64_t M, int64_t rows_per_split, float* slab,
                     int64_t slab_numel, int nextra, const rs_reduce_segment* extra, void* stream);
/* rs_wgrad_grouped with the output tile edge capped at max_tile (>= 64; rs_wgrad_grouped = 256): a launch that runs
 * beside a streaming kernel (the BERT token table's optimizer update) takes 128-wide tiles -- the 256-wide form's
 * one-workgroup-per-CU LDS-DMA pipeline measured 10x slower sharing the chip with it (cfg5). */
int rs_wgrad_grouped_max(int nprob, const rs_wgrad_problem* probs, int64_t M, int64_t rows_per_split, float* slab,
                         int64_t slab_numel, int nextra, const rs_reduce_segment* extra, int max_tile, void* stream);

/* rs_wgrad_grouped followed by rs_embed_bwd's positional part (bf16, SAS mode 0, scale 1, dpos +=): the
 * positional table's gradient rides in the grouped reduction's launch as T extra workgroups (grad_tail.hip).
 * dW, db and the extra segments' outputs are bit-equal to rs_wgrad_grouped's.  dpos is bit-equal to rs_embed_bwd's
 * for M / T <= 16 sequences; for more the fused launch adds the batch rows in 16 groups where rs_embed_bwd uses 32,
 * so the two agree within the float32 summation-order bound, not bit for bit (each is deterministic by itself).
 * Shapes outside the fused form (d > 128 or d % 8, more than 64 segments in all) run the functions one after the
 * other and give their bits. */
int rs_wgrad_grouped_pos(int nprob, const rs_wgrad_problem* probs, int64_t M, int64_t rows_per_split, float* slab,
                         int64_t slab_numel, int nextra, const rs_reduce_segment* extra, const int64_t* ids,
                         int64_t T, const void* dx, int64_t d, float drop_p, uint64_t salt,
                         const uint64_t* seed_base, float* dpos, void* stream);
/* rs_wgrad_grouped_pos whose reduction launch also carries rs_sas_head_finish (one more workgroup): the SAS
 * head's loss statistics loss_out[0..3] from the head's partials (head_part[head_blocks][3]); aux_out (optional,
 * data parallel): (loss sum, count) written there too -- the all-reduced tail of the gradient buffer.  loss_out
 * is bit-equal to rs_sas_head_finish's. */
int rs_wgrad_grouped_pos_stats(int nprob, const rs_wgrad_problem* probs, int64_t M, int64_t rows_per_split,
                               float* slab, int64_t slab_numel, int nextra, const rs_reduce_segment* extra,
                               const int64_t* ids, int64_t T, const void* dx, int64_t d, float drop_p, uint64_t salt,
                               const uint64_t* seed_base, float* dpos, const float* head_part, int64_t head_blocks,
                               const float* head_divisor, float* loss_out, float* aux_out, void* stream);
/* The reduction alone: out (+)= sum over splits, for nseg segments (any number, 64 per launch). */
int rs_reduce_segments(int nseg, const rs_reduce_segment* segs, int accumulate, void* stream);

/* ---- item-table gradient by inverted index (itemgrad.hip) ------------------------------------
 * dtable[v] += sum over the rows keyed v of: source 0  scale * dropout(m*d + c) * dx[m]  (the
 * embedding lookup, sas.py:59-66), source 1  w1[m] * f[m], source 2  w2[m] * f[m]  (the tied
 * sampled logits, sas.py:91-98); key 0 (padding_idx) skipped.  Deterministic: a stable radix
 * sort of the keys, per-key sums in fixed order, one writer per table row, no float atomics.
 * Build the index once per batch (the keys are step inputs), then rs_item_grad after the
 * backward pass.  ws: rs_item_index_ws_bytes() bytes (device). */
int64_t rs_item_index_ws_bytes(int nsrc, int64_t rows, int64_t table_rows, int64_t d);
int rs_item_index_build(int nsrc, const int64_t* keys0, const int64_t* keys1, const int64_t* keys2, int64_t rows,
                        int64_t table_rows, int64_t d, void* ws, int64_t ws_bytes, void* stream);
/* Where the built index lives in ws (for tests and tools): out[0..3] = byte offsets of the sorted keys (u32 [n]),
 * the sorted entries (u32 [n], entry = source * rows + row), start (int [table_rows + 1]), and the sort path
 * (0 counting sort, 1 / 2 one-workgroup LDS radix sort with u32 / u64 words, 3 multi-workgroup radix sort). */
int rs_item_index_layout(int nsrc, int64_t rows, int64_t table_rows, int64_t d, int64_t* out);
/* dx, f: bf16 [rows][d] (d in {64, 128, 256}); w1, w2: fp32 [rows]; dtable fp32 [table_rows][d]. */
int rs_item_grad(const void* ws, int nsrc, int64_t rows, int64_t table_rows, int64_t d, const void* dx, float scale,
                 float drop_p, uint64_t salt, const uint64_t* seed_base, const void* f, const float* w1,
                 const float* w2, float* dtable, void* stream);
/* rs_item_grad that also marks the table rows it writes: row_marks[v] = epoch for every key v of the batch and
 * *epoch_out = epoch, epoch = the low byte of *seed_base (0 without one): the step's stamp for rs_adam_*_marked.
 * row_marks: the rs_adam_*_marked layout over table_rows (stamps: any initial contents). */
int rs_item_grad_marked(const void* ws, int nsrc, int64_t rows, int64_t table_rows, int64_t d, const void* dx,
                        float scale, float drop_p, uint64_t salt, const uint64_t* seed_base, const void* f,
                        const float* w1, const float* w2, float* dtable, uint8_t* row_marks, uint8_t* epoch_out,
                        void* stream);
/* The same for fp32 dx, f (the fp32 parity path, any d): each key run summed in sorted-entry order inside 32-entry
 * chunks, a run crossing chunks as its chunk partials in chunk order (the index workspace's partial region). */
int rs_item_grad_f32(const void* ws, int nsrc, int64_t rows, int64_t table_rows, int64_t d, const float* dx, float scale,
                     float drop_p, uint64_t salt, const uint64_t* seed_base, const float* f, const float* w1,
                     const float* w2, float* dtable, void* stream);
/* The weighted form, one weight per entry: over an index built by rs_item_index_build(1, keys, NULL, NULL, rows * per,
 * table_rows, d, ...) on keys int64 [rows * per],
 *   dtable[key_e] += sum over the entries e keyed key_e of  w[e] * f[e / per]
 * f: dtype (RS_DTYPE_F32 / RS_DTYPE_BF16) [rows][d] of row stride ldf (elements), any d; w: fp32 [rows * per];
 * dtable fp32 [table_rows][d].  Key 0 is skipped (its w and f are not read).  One writer per table row; a key run is
 * summed in sorted-entry order inside 32-entry chunks, a run crossing chunks as its chunk partials in chunk order
 * (rs_item_grad_f32's rule and span pass): bitwise reproducible, no float atomics.  No [rows * per][d] buffer exists
 * anywhere: memory grows with rows * per, never with rows * per * d.  rows * per < 2^31. */
int rs_item_grad_weighted(const void* ws, int dtype, int64_t rows, int64_t per, int64_t table_rows, int64_t d,
                          const void* f, int64_t ldf, const float* w, float* dtable, void* stream);

/* ---- fused SASRec output head (head.hip), bf16, d in {64, 128, 256} ----------------------------
 * Forward (sas.py:87-100 + BCE of trainers/sas.py:40-49): f = LN_last(x) [f, mean, rstd saved];
 * pl = <f, E[pos]>, nl = <f, E[neg]> (E = item_emb); part[b][3] = per-64-row-block sums of
 * softplus(-pl), softplus(nl) and the valid count (pos != 0).  part >= 3*ceil(M/64) floats. */
int rs_sas_head_fwd(int64_t M, int64_t d, const void* x, const float* ln_w, const float* ln_b, float eps, void* f,
                    float* mean, float* rstd, const void* E, const int64_t* pos, const int64_t* neg, float* pl,
                    float* nl, float* part, void* stream);
/* Backward: with dpl_in == NULL the BCE gradient is formed here: dpl = (sigmoid(pl)-1)/c,
 * dnl = sigmoid(nl)/c on valid rows, c = *divisor or the forward's valid count, written to
 * dpl/dnl, and out[0..3] = {loss sum, count, mean loss (as rs_bce_fwd), neg-term sum}; with
 * dpl_in/dnl_in given (autograd) those are used and part, out, dpl, dnl are left alone.  A batch
 * without a valid row (count 0): dpl, dnl, dx and lnpart are exactly zero, out[0] = out[1] =
 * out[3] = 0 and out[2] = 0/c -- NaN without a divisor (the reference's mean over an empty
 * selection, as rs_bce_fwd), 0 with one.  Then df = dpl E[pos] + dnl E[neg] and
 * dx = LN'(x, df) (bf16); lnpart[b][2][d] = LN affine partials (reduce with rs_reduce_segments).
 * The item-table gradient of the logits is left to rs_item_grad. */
int rs_sas_head_bwd(int64_t M, int64_t d, const float* part, const float* divisor, float* out, const float* pl,
                    const float* nl, const float* dpl_in, const float* dnl_in, float* dpl, float* dnl,
                    const int64_t* pos, const int64_t* neg, const void* E, const void* x, const float* ln_w,
                    const float* mean, const float* rstd, void* dx, float* lnpart, void* stream);
/* out[0..3] from a head's BCE partials part[nblk][3] exactly as rs_sas_head_bwd forms them (one workgroup; the
 * unfused form of rs_wgrad_grouped_pos_stats' statistics). */
int rs_sas_head_finish(int64_t nblk, const float* part, const float* divisor, float* out, void* stream);

/* ---- on-device SAS sampler and ranking metrics (sampler.hip) ----------------------------------
 * rs_sas_sample: one training batch as WarpSampler's workers build it (BS/dataloaders/sas.py:65-91):
 * per row a uniform user, its last max_len items, seq/pos = the window shifted by one, left padded
 * with 0, neg = uniform draws over {0..item_num} minus the window's items.  Histories are a CSR pair
 * (user_offsets[n_users+1], user_items).  *seed_base is advanced first (device counter; graph-
 * capturable); salt separates samplers.  seq/pos/neg: int64 [batch][max_len]; max_len <= 512. */
int rs_sas_sample(const int64_t* user_offsets, const int64_t* user_items, int64_t n_users, int64_t item_num,
                  int64_t batch, int64_t max_len, uint64_t* seed_base, uint64_t salt, int64_t* seq, int64_t* pos,
                  int64_t* neg, void* stream);
/* rs_sas_sample_negs: rs_sas_sample with n_negs negatives per position, neg int64 [batch][max_len][n_negs],
 * 1 <= n_negs <= 1024.  Negative j of position (b, t) draws from the counters base + (j << 8) + a, a = 0..255, where
 * base = seed + ((b * max_len + t) << 20) is rs_sas_sample's own; the rejection set (the window) and the never-reached
 * linear fallback are rs_sas_sample's.  So seq, pos and neg[.][.][0] are rs_sas_sample's from the same seed and salt,
 * bit for bit.  Draws are with replacement; padded positions are all 0; *seed_base is advanced once, first. */
int rs_sas_sample_negs(const int64_t* user_offsets, const int64_t* user_items, int64_t n_users, int64_t item_num,
                       int64_t batch, int64_t max_len, uint64_t* seed_base, uint64_t salt, int64_t n_negs, int64_t* seq,
                       int64_t* pos, int64_t* neg, void* stream);
/* rs_bert_mask: one BERT4Rec training batch as BertTrainDataset builds it (BS/dataloaders/bert.py:77-110):
 * row b's user = perm[(cursor*batch + b) mod n_users] (perm nullable = identity), its last max_len items
 * cloze-masked (prob mask_prob, a double: the reference's Python float; then 80 % [MASK] = num_items+1, 10 % a uniform item, 10 % kept;
 * label = the item, 0 elsewhere), left padded.  state[2] = {step seed, cursor} on the device, both
 * advanced by 1 before sampling (graph-capturable; reset state[1] to 0 at an epoch start). */
int rs_bert_mask(const int64_t* user_offsets, const int64_t* user_items, int64_t n_users, int64_t num_items,
                 int64_t batch, int64_t max_len, double mask_prob, const int64_t* perm, uint64_t* state, uint64_t salt,
                 int64_t* tokens, int64_t* labels, void* stream);
/* The same two samplers, also recording the draws each row consumed (tests replay the reference's construction
 * on them, oracle/sampling.py).  SAS: draws int64 [batch][1 + max_len*256] = {user, then per position the 256
 * candidate negatives the rejection loop may try, in draw order (-1 where the position draws none)}.  BERT: draws int64 [batch][1 + 2*max_len]
 * = {user, then per position (k, item): the masking uniform is k / 2^24, the replacement item is item; -1 on
 * padding}. */
int rs_sas_sample_draws(const int64_t* user_offsets, const int64_t* user_items, int64_t n_users, int64_t item_num,
                        int64_t batch, int64_t max_len, uint64_t* seed_base, uint64_t salt, int64_t* seq, int64_t* pos,
                        int64_t* neg, int64_t* draws, void* stream);
int rs_bert_mask_draws(const int64_t* user_offsets, const int64_t* user_items, int64_t n_users, int64_t num_items,
                       int64_t batch, int64_t max_len, double mask_prob, const int64_t* perm, uint64_t* state,
                       uint64_t salt, int64_t* tokens, int64_t* labels, int64_t* draws, void* stream);

/* rs_rank_metrics: recalls_ndcgs_and_mrr_for_ks (BS/trainers/utils.py:28-57) over scores/labels
 * fp32 [rows][cands] (labels 0/1 weights), ks: device int[nk] (nk <= 8).  out[3*q + {0,1,2}] =
 * mean Recall@k, NDCG@k, MRR@k for ks[q]; ws >= 3*nk*rows floats.  Ranks follow a stable
 * descending sort (ties by candidate index). */
int rs_rank_metrics(const float* scores, const float* labels, int64_t rows, int64_t cands, int nk, const int* ks,
                    float* ws, float* out, void* stream);

/* ---- full-catalogue ranking and top-K (fullrank.hip) --------------------------------------------
 * Replaces: scoring a hand-picked candidate list and ranking it (BS/trainers/sas.py:56-62, BS/trainers/bert.py:43-52,
 * BS/trainers/utils.py:28-57) when the candidates are EVERY item -- one vocabulary-stationary sweep, no (B, V) scores.
 *   score      s(b, v) = fp32(sum_k h[b*ldh + k] * E[v*lde + k]) (+ bias[v] when bias != NULL); h, E in dtype
 *              (RS_DTYPE_*), d <= 256 (any value; more: RS_ERR_UNSUPPORTED), finite scores (the caller's promise)
 *   admissible A(b) = {v : v_lo <= v < v_hi, v not in excl[b*ldx .. + nx)}; excl int64 (nullable; nx = 0: none), each
 *              row SORTED ascending; duplicates allowed, entries outside [v_lo, v_hi) ignored (a history's 0 padding,
 *              BERT's [MASK] id); v_hi <= 2^31 - 256
 *   order      v before w  <=>  s_v > s_w, or s_v == s_w and v < w
 * rs_full_rank: rank[b] (int32) = number of v in A(b), v != target[b], before target[b]; the target itself is never
 * excluded (the reference's negatives avoid seen items, the answer stays); a target outside [v_lo, v_hi) gives -1.
 * target_score (nullable, fp32 [B]) = s(b, target[b]), formed by the sweep's own tile routine, so an item whose E
 * row and bias equal the target's ties with it exactly.
 * rs_full_topk: ids int64 [B][K], scores fp32 [B][K] = the first K of A(b) in the order; past |A(b)|: id -1, score
 * -inf.  1 <= K <= RS_TOPK_MAX (more: RS_ERR_UNSUPPORTED).
 * ws: rs_full_ws_bytes(dtype, B, d, v_hi - v_lo, K) bytes (host-only sizing; K = 0: rs_full_rank alone), 256-B
 * aligned.  No allocation, no sync, graph-capturable.
 * rs_rank_to_metrics: out[3*q + {0,1,2}] = mean over rows of [rank < k], [rank < k] / log2(rank + 2),
 * [rank < k] / (rank + 1) for k = ks[q] (device int[nk], nk <= 8) -- Recall / NDCG / MRR@k of
 * recalls_ndcgs_and_mrr_for_ks with one positive per row; rank -1 is a miss; ws >= 3*nk*rows floats; means in double,
 * fixed order (as rs_rank_metrics). */
#define RS_TOPK_MAX 128
int64_t rs_full_ws_bytes(int dtype, int64_t B, int64_t d, int64_t nrange, int64_t K);
int rs_full_rank(int dtype, const void* h, int64_t ldh, int64_t B, int64_t d, const void* E, int64_t lde,
                 const float* bias, int64_t v_lo, int64_t v_hi, const int64_t* target, const int64_t* excl, int64_t nx,
                 int64_t ldx, void* ws, int* rank, float* target_score, void* stream);
int rs_full_topk(int dtype, const void* h, int64_t ldh, int64_t B, int64_t d, const void* E, int64_t lde,
                 const float* bias, int64_t v_lo, int64_t v_hi, const int64_t* excl, int64_t nx, int64_t ldx, int64_t K,
                 void* ws, int64_t* ids, float* scores, void* stream);
int rs_rank_to_metrics(const int* rank, int64_t rows, int nk, const int* ks, float* ws, float* out, void* stream);

/* ---- SASRec tied full-catalogue cross-entropy head: the row kernels (sas_ce.hip; bf16, d in {64, 128}) ----
 * The objective: f = LN_last(x_L), logits = f item_emb^T over all V+1 rows (class 0 = the zero padding row),
 * CrossEntropyLoss(ignore_index=0) against pos.  The vocabulary part runs through rs_vocab_head_fwd / _bwd
 * (bias NULL, E = item_emb) on the compacted valid rows; these are the row-local launches around it.  Both return
 * RS_ERR_UNSUPPORTED, launching nothing, for any other dtype or width.
 * rs_sas_ce_rows_fwd: rs_compact_rows(labels, M, cap) + rs_layernorm_fwd (variant 0) + rs_gather_rows in one launch:
 *   idx [cap], rank [M], *count exactly as rs_compact_rows writes them; for i < *count, with r = idx[i]:
 *   hl[i] = LN(x[r]) (bf16, row stride ldh), lab[i] = labels[r], mean[i], rstd[i] (fp32, per COMPACT row).  Rows
 *   >= *count of hl / lab / mean / rstd are left untouched.  x: bf16 [M][d], row stride ldx (multiple of 8).
 *   divisor (nullable): *divisor = max(*count, 1) as a float -- the count_override / count of the vocabulary
 *   kernels, so that a batch with no valid row has loss 0 (0 / 1) instead of 0 / 0.
 * rs_sas_ce_rows_nparts (host only): affine-partial sets rs_sas_ce_rows_bwd writes for M rows.
 * rs_sas_ce_rows_bwd: rs_splitk_scatter_rows + rs_layernorm_bwd in one launch: for r < M with k = rank[r] >= 0,
 *   dh = bf16(sum over z < splits, in order, of slab[z][k][:]) (slab fp32 [splits][cap][d]) and
 *   dx[r] = LN'(x[r], dh; mean[k], rstd[k]); dx[r] = 0 where rank[r] < 0.  part[b][2][d] (b < nparts): the sums of
 *   dh * xhat (dgamma) and dh (dbeta) over the rows of set b -- row r belongs to set (r / (2048 / d)) mod nparts --
 *   to be reduced in set order (rs_reduce_segments; ops.ln_partial_segments).  No atomics. */
int rs_sas_ce_rows_fwd(int dtype, int64_t M, int64_t d, const void* x, int64_t ldx, const int64_t* labels,
                       int64_t cap, const float* gamma, const float* beta, float eps, int32_t* idx, int32_t* rank,
                       int32_t* count, float* divisor, void* hl, int64_t ldh, int64_t* lab, float* mean, float* rstd,
                       void* stream);
int64_t rs_sas_ce_rows_nparts(int64_t M);
int rs_sas_ce_rows_bwd(int dtype, int64_t M, int64_t d, const float* slab, int splits, int64_t cap,
                       const int32_t* rank, const void* x, int64_t ldx, const float* gamma, const float* mean,
                       const float* rstd, void* dx, int64_t lddx, float* part, void* stream);

/* ---- SASRec sampled-softmax head over batch-shared candidates (sas_sce.hip) ----
 * The objective, on the compact valid rows rs_sas_ce_rows_fwd leaves (or on all rows with count NULL: lab 0 = no row):
 *   f_r   = last_layernorm(log2feats(seq))[r]          for every position r with pos_r != 0 ("valid")
 *   z_r0  = <f_r, E[pos_r]>                            E = item_emb.weight (tied), fp32 accumulate
 *   z_rj  = <f_r, E[cand_j]>,  j = 1..K                cand: int64 [K], ids in [0, V]
 *   live(r, j) = cand_j != 0 and cand_j != pos_r       id 0 = an ignored slot; accidental hits masked
 *   loss  = (1 / max(n, 1)) * sum_valid r [ log( exp(z_r0) + sum_{live j} exp(z_rj) ) - z_r0 ],   n = #valid
 * Duplicate ids in cand are separate classes (each counts); no logQ correction in these entries (rs_sce_head_logq_*
 * below subtract one); a row with no live candidate has loss
 * 0 and gradient 0; an id outside [0, V] counts as 0.  With p_rj = softmax over {0} + live and s = *dloss / *divisor:
 *   dh[r]   = s ((p_r0 - 1) E[pos_r] + sum_live p_rj E[cand_j])     fp32 slabs [splits][cap][d], splits =
 *                                                                   rs_sas_sce_dh_splits(cap, K, d) (host only): one
 *                                                                   per split of the candidates, to be summed in
 *                                                                   split order (rs_sas_ce_rows_bwd(splits))
 *   coef[r] = s (p_r0 - 1),   pg[r] = coef[r] hl[r]                 fp32 [cap], [cap][d]: the table's gradient at pos_r
 *   dEc[j]  = s sum_r p_rj hl[r]                                    fp32 [K][d]: the table's gradient at cand_j, the
 *                                                                   rows summed in a fixed order (row splits in fp32
 *                                                                   slabs reduced in split order; no atomics)
 *   keys    (nullable) int64 [cap + K]: lab of the rows < *count (0 past it), then cand -- the inverted index's keys
 *           over the rows of {pg, dEc} (rs_item_index_build, rs_item_grad_f32: key 0 gets nothing)
 * hl: [cap][d] rows of stride ldh, lab [cap], count: device int32 (NULL: cap), E: [V1][d] in hl's dtype, divisor:
 * device float (max(n, 1)), dloss: device float or NULL (1).  rs_sas_sce_fwd writes lse and z_r0 per row into ws and
 * out = {loss sum, n, sum / *divisor}; rs_sas_sce_bwd reads them there.  Rows at or past *count are left untouched in
 * every per-row output.  ws: rs_sas_sce_ws_bytes(cap, K, d) bytes (host only; no argument for V: nothing here is
 * sized by the catalogue), 16-byte aligned.  dtype fp32 (any d <= 1024) or bf16 (d % 8 == 0, d <= 1024; d <= 128 runs
 * the MFMA sweep, wider rows a plain kernel with the same outputs), 1 <= K <=
 * rs_sas_sce_max_k() (65536); anything else: RS_ERR_UNSUPPORTED, nothing launched.  No allocation, no sync,
 * graph-capturable; the logits are never stored.
 * rs_uniform_items: out[j] = 1 + floor(u_j * item_num), u_j uniform from splitmix64 of (salt ^ f(*seed_base), j):
 * K draws with replacement over [1, item_num].  It advances nothing (the sampler's own kernel advances seed_base). */
int64_t rs_sas_sce_max_k(void);
int64_t rs_sas_sce_ws_bytes(int64_t cap, int64_t K, int64_t d);
int64_t rs_sas_sce_dh_splits(int64_t cap, int64_t K, int64_t d);
int rs_sas_sce_fwd(int dtype, int64_t cap, int64_t d, const void* hl, int64_t ldh, const int64_t* lab,
                   const int32_t* count, const void* E, int64_t V1, const int64_t* cand, int64_t K,
                   const float* divisor, void* ws, float* out, void* stream);
int rs_sas_sce_bwd(int dtype, int64_t cap, int64_t d, const void* hl, int64_t ldh, const int64_t* lab,
                   const int32_t* count, const void* E, int64_t V1, const int64_t* cand, int64_t K,
                   const float* divisor, const float* dloss, void* ws, float* dh, float* coef, float* pg, float* dEc,
                   int64_t* keys, void* stream);
int rs_uniform_items(const uint64_t* seed_base, uint64_t salt, int64_t item_num, int64_t K, int64_t* out,
                     void* stream);

/* ---- SASRec head with N negatives per position: multi-negative BCE / gBCE (sas_gbce.hip) ----
 * The objective, on the compact valid rows rs_sas_ce_rows_fwd leaves, with f = last_layernorm(log2feats(seq)),
 * E = item_emb.weight (tied) and neg int64 (B, T, N):
 *   valid r      : pos_r != 0,  n = #valid
 *   z_r0         = <f_r, E[pos_r]>
 *   z_rj         = <f_r, E[neg_rj]>,  j = 1..N
 *   loss         = (1 / max(n, 1)) * sum_valid r [ beta * softplus(-z_r0) + sum_j softplus(z_rj) ]
 *   g_r0         = s * beta * (sigmoid(z_r0) - 1),   g_rj = s * sigmoid(z_rj),   s = dloss / max(n, 1)
 *   df_r         = g_r0 E[pos_r] + sum_j g_rj E[neg_rj]
 *   dE[v]       += sum over (r, j = 0..N) with id_rj = v, v != 0 of  g_rj f_r
 * The negatives are summed, not averaged: N = 1, beta = 1 is the reference's BCE term for term.  A negative id 0 is
 * the zero row: logit exactly 0, softplus(0) in the loss, no table gradient.  Nothing is masked; equal ids in a row are
 * separate terms; an id outside [0, V] counts as 0; a batch with no valid row gives loss 0 and all-zero gradients;
 * table row 0 never receives a gradient.
 * hl: [cap][d] rows of stride ldh, lab [cap], count: device int32 (NULL: cap), idx: int32 [cap], the source row of
 * compact row r as rs_compact_rows defines it -- the negatives are read in place as neg[idx[r] * N + j]; idx == NULL
 * is the identity (the dense fp32 form: count NULL, a row with lab 0 is no row -- its z, w, dh and keys are written
 * as zeros).  E: [V1][d] in hl's dtype, divisor: device float (max(n, 1)), dloss: device float or NULL (1).
 * rs_sas_gbce_fwd writes the logits z fp32 [cap][1 + N] into ws and out = {loss sum, n, sum / *divisor, negative-term
 * sum}; the sums run in a fixed order (per-workgroup partials in double, one finishing pass, no atomics).
 * rs_sas_gbce_bwd reads z from ws and writes dh fp32 [cap][d] (a single slab, for rs_sas_ce_rows_bwd(splits = 1)), the
 * weights w fp32 [cap][1 + N] (the g above) and keys int64 [cap * (1 + N)] = {lab_r, neg_r1..neg_rN} per row, 0 past
 * the count and for ids out of range: the inverted index's keys for rs_item_grad_weighted(rows = cap, per = 1 + N,
 * f = hl).  Rows at or past *count are left untouched in every other per-row output.
 * ws: rs_sas_gbce_ws_bytes(cap, N, d) bytes (host only; grows with cap * N, no argument for V), 16-byte aligned.
 * dtype fp32 (any d <= 1024) or bf16 (d % 8 == 0, d <= 1024), 1 <= N <= rs_sas_gbce_max_n() (1024),
 * cap * (1 + N) < 2^31; anything else: RS_ERR_UNSUPPORTED, nothing launched.  No allocation, no sync,
 * graph-capturable.  A gather kernel (every row has its own 1 + N table rows): the traffic is cap * (1 + N) * d *
 * sizeof per pass. */
int64_t rs_sas_gbce_max_n(void);
int64_t rs_sas_gbce_ws_bytes(int64_t cap, int64_t N, int64_t d);
int rs_sas_gbce_fwd(int dtype, int64_t cap, int64_t d, const void* hl, int64_t ldh, const int64_t* lab,
                    const int32_t* idx, const int32_t* count, const void* E, int64_t V1, const int64_t* neg, int64_t N,
                    float beta, const float* divisor, void* ws, float* out, void* stream);
int rs_sas_gbce_bwd(int dtype, int64_t cap, int64_t d, const void* hl, int64_t ldh, const int64_t* lab,
                    const int32_t* idx, const int32_t* count, const void* E, int64_t V1, const int64_t* neg, int64_t N,
                    float beta, const float* divisor, const float* dloss, void* ws, float* dh, float* w, int64_t* keys,
                    void* stream);

/* ---- the same sampled-softmax head for an untied output layer with a bias (sas_sce.hip; BERT4Rec's out) ----
 * E: any [V1][d] table in hl's dtype, bias: fp32 [V1] or NULL.  The definition above with
 *   z_r0 = <h_r, E[lab_r]> + b[lab_r],   z_rj = <h_r, E[cand_j]> + b[cand_j]
 * live, the loss, dh, coef, pg, dEc and keys exactly as above on these logits, and in addition
 *   dbc[j] = s sum_r p_rj        fp32 [K]: the bias gradient at cand_j, the rows summed in a fixed order (the dEc
 *                                launch's row splits in slabs reduced in split order; no atomics)
 * The bias gradient at the positive is coef[r]: db[v] += the entries of {coef, dbc} keyed v, over the same keys (one
 * writer per element: rs_item_grad_f32 at d = 1 on the index built for {pg, dEc}, radix path).
 * dbc is required with a bias and must be NULL without one (RS_ERR_ARG).  bias == NULL gives the rs_sas_sce_* entries'
 * bits on every output and in ws wherever both run the same kernel (fp32, and bf16 up to d = 128).
 * rs_sce_head_path (host only): 1 = the MFMA sweep (fp32 d <= 128; bf16 d <= 256, padded to 64 / 128 / 256 in the
 * fragments), 0 = the plain kernel (wider rows up to 1024), < 0 = unsupported dtype / width.
 * ws: rs_sce_head_ws_bytes(dtype, cap, K, d, has_bias) bytes (host only; rs_sas_sce_ws_bytes plus the dbc slabs with a
 * bias; nothing is sized by V1), 16-byte aligned; dh: rs_sce_head_dh_splits(dtype, cap, K, d) slabs.  Argument
 * checks, limits and return codes as rs_sas_sce_fwd / _bwd. */
int64_t rs_sce_head_ws_bytes(int dtype, int64_t cap, int64_t K, int64_t d, int has_bias);
int64_t rs_sce_head_dh_splits(int dtype, int64_t cap, int64_t K, int64_t d);
int rs_sce_head_path(int dtype, int64_t d);
int rs_sce_head_fwd(int dtype, int64_t cap, int64_t d, const void* hl, int64_t ldh, const int64_t* lab,
                    const int32_t* count, const void* E, const float* bias, int64_t V1, const int64_t* cand, int64_t K,
                    const float* divisor, void* ws, float* out, void* stream);
int rs_sce_head_bwd(int dtype, int64_t cap, int64_t d, const void* hl, int64_t ldh, const int64_t* lab,
                    const int32_t* count, const void* E, const float* bias, int64_t V1, const int64_t* cand, int64_t K,
                    const float* divisor, const float* dloss, void* ws, float* dh, float* coef, float* pg, float* dEc,
                    float* dbc, int64_t* keys, void* stream);

/* ---- the logQ correction of the sampled softmax, and the sampler it describes (sas_sce.hip) ----
 * rs_sce_head_logq_fwd / _bwd: rs_sce_head_fwd / _bwd with logq, fp32 [V1] or NULL, after bias.  The definition of
 * rs_sce_head_* with
 *   z_r0 = <h_r, E[lab_r]>  + b[lab_r]  - logq[lab_r],   z_rj = <h_r, E[cand_j]> + b[cand_j] - logq[cand_j]
 * (fp32: the dot product plus the one per-id term b[id] - logq[id]; b = 0 without a bias).  live, the loss, lse, dh,
 * coef, pg, dEc, dbc and keys are computed on these logits exactly as above.  logq is the log of the proposal the
 * candidates were drawn from; it is not a parameter and gets no gradient.  dbc stays tied to bias alone: required with
 * a bias, NULL without one, whatever logq is.  logq[0] is never read (id 0 stays the ignored slot; an id outside
 * [0, V1) counts as 0).  logq == NULL gives rs_sce_head_*'s bits on every output and in ws.  The workspace and slab
 * counts are rs_sce_head_ws_bytes / rs_sce_head_dh_splits: the correction adds nothing sized by K, cap or V1.
 *
 * rs_alias_items: K draws with replacement over [1, item_num] from an alias table (Walker / Vose) of item_num 8-byte
 * entries, entry s = thr[s] | (uint64_t)alias[s] << 32 with thr[s] a uint32 and alias[s] an item id in [1, item_num].
 * Draw j, bit for bit (seed = eff_seed(salt, *seed_base) and the constant C = 0x632BE59BD9B4E019 of rs_uniform_items):
 *   r    = splitmix64(seed + C * (j + 1))                      (64-bit wrap-around arithmetic)
 *   s    = umulhi(r, item_num)                                 the high 64 bits of r * item_num: the slot, < item_num
 *   frac = (uint32)((r * item_num mod 2^64) >> 32)             the next 32 bits of the same product
 *   out[j] = frac < thr[s] ? s + 1 : alias[s]
 * A slot that keeps its whole mass has alias[s] = s + 1, so thr never has to hold 2^32; with every slot full the draws
 * are rs_uniform_items' for the same salt and seed.  The distribution the rule realises is fixed by the integers:
 *   N(v) = thr[v - 1] + sum over {s: alias[s] = v} of (2^32 - thr[s]),    Qhat(v) = N(v) / (item_num * 2^32),
 * and logq is to be log Qhat (not the log of the weights the table was built from).  How far a uniform 64-bit r lets
 * the true frequencies sit from Qhat: (s, frac) is floor(r * item_num / 2^32), and the r that land in a run of n
 * consecutive values of it fill an interval of length n * 2^32 / item_num, which holds within one of that many
 * integers; item v owns one run in its own slot and one in every slot aliased to it, so
 *   |P(out[j] = v) - Qhat(v)| < (1 + #{s: alias[s] = v}) * 2^-64,
 * which is below item_num * 2^-32 per run relative to Qhat(v) even for an item that holds a single cell
 * (Qhat(v) >= 2^-32 / item_num when N(v) >= 1).
 * It advances nothing, allocates nothing and is graph-capturable.  K < 1, item_num < 1 or item_num >= 2^32, or a NULL
 * table / out: RS_ERR_ARG, nothing launched.  The table's aliases are not checked on the device. */
int rs_sce_head_logq_fwd(int dtype, int64_t cap, int64_t d, const void* hl, int64_t ldh, const int64_t* lab,
                         const int32_t* count, const void* E, const float* bias, const float* logq, int64_t V1,
                         const int64_t* cand, int64_t K, const float* divisor, void* ws, float* out, void* stream);
int rs_sce_head_logq_bwd(int dtype, int64_t cap, int64_t d, const void* hl, int64_t ldh, const int64_t* lab,
                         const int32_t* count, const void* E, const float* bias, const float* logq, int64_t V1,
                         const int64_t* cand, int64_t K, const float* divisor, const float* dloss, void* ws, float* dh,
                         float* coef, float* pg, float* dEc, float* dbc, int64_t* keys, void* stream);
int rs_alias_items(const uint64_t* seed_base, uint64_t salt, const uint64_t* table, int64_t item_num, int64_t K,
                   int64_t* out, void* stream);

/* ---- on-device evaluation loader: seeded per-user negatives and evaluation batches (eval_loader.hip) ----
 * Replaces the reference's test negatives (BS/dataloaders/negative_samplers/random.py:18-35, popular.py:25-42) and its
 * evaluation datasets (SASEvalDataset, BS/dataloaders/sas.py:125-153; BertEvalDataset, BS/dataloaders/bert.py:116-142).
 *
 * rs_eval_negatives: for the users u in [user0, user0 + count) it writes negs[u * n_neg + 0 .. n_neg) (int32; negs,
 * n_drawn and draws are indexed by the ABSOLUTE user u, as seen_offsets is).  User u owns a raw draw stream
 *   k(u)    = splitmix64(seed ^ (A * (u + 1)))                    A = 0xA0761D6478BD642F, 64-bit wrap-around
 *   r(u, c) = splitmix64(k(u) + C * (c + 1)),  c = 0, 1, ...       C = 0x632BE59BD9B4E019 (rs_uniform_items' constant)
 *   s       = umulhi(r, item_num)                                  the high 64 bits of r * item_num, < item_num
 *   x(u, c) = s + 1                                                table == NULL: uniform over [1, item_num]
 *   x(u, c) = frac < thr[s] ? s + 1 : alias[s],  frac = (uint32)((r * item_num mod 2^64) >> 32)
 *                                                                  table: a packed alias table, exactly rs_alias_items' rule
 * with splitmix64(z): z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) *
 * 0x94D049BB133111EB; return z ^ z >> 31.  negs[u] is that stream with every item of seen(u) dropped and every repeat
 * of an earlier kept item dropped, the first n_neg survivors in stream order (RandomNegativeSampler's `while item in
 * seen or item in samples` loop on the stream).  seen(u) = seen_sorted[seen_offsets[u] .. seen_offsets[u + 1]) (int32,
 * ascending, unique): the user's WHOLE history, train + val + test.  x depends on (seed, u, c) only: one call over all
 * users equals any split into several calls.
 * Bounds: 1 <= n_neg <= rs_eval_negs_max() (1024), n_neg <= item_num < 2^31.  At most rs_eval_negatives_max_draws()
 * (4096; host only) raw draws are read per user; the slots still open then take the smallest ids of [1, item_num] that
 * are neither seen nor kept, ascending.  The caller guarantees item_num - |seen(u)| >= n_neg (slots that cannot be
 * filled get 0).  n_drawn (nullable, int32 [users]): the raw draws consumed, c + 1 of the draw that filled the last
 * slot, or -1 - (slots filled by the fallback).
 * rs_eval_negatives_draws: the same negs, and draws[u * max_draws + c] = x(u, c) (int64) for every c < max_draws,
 * before any filtering (tests replay the reference's loop on them).
 *
 * rs_eval_batch: for the users u = user0 + b, b in [0, B), one row each of
 *   seq    int64 [B][max_len]: the last max_len of  history(u) (+ extra[u] when extra != NULL: the validation item of
 *          test mode) (+ mask_token when mask_token > 0: BERT appends [MASK] BEFORE truncating), left padded with 0;
 *          history(u) = hist_items[hist_offsets[u] .. hist_offsets[u + 1]) (int64, may be empty)
 *   cand   int64 [B][1 + n_neg] = {answer[u], negs[u * n_neg + 0 .. n_neg)}
 *   labels int64 [B][1 + n_neg] = {1, 0, ..., 0}
 * extra / answer: int64 [users]; negs as rs_eval_negatives writes it.  1 <= max_len <= 512, n_neg as above.
 *
 * Every refusal is made on the host before any launch: RS_ERR_ARG for a NULL pointer (table, n_drawn, extra are
 * optional), user0 < 0, a non-positive size, or n_neg / item_num / max_len out of range.  No allocation, no sync. */
int64_t rs_eval_negs_max(void);
int64_t rs_eval_negatives_max_draws(void);
int rs_eval_negatives(const int64_t* seen_offsets, const int32_t* seen_sorted, int64_t user0, int64_t count,
                      int64_t item_num, int64_t n_neg, uint64_t seed, const uint64_t* table, int32_t* negs,
                      int32_t* n_drawn, void* stream);
int rs_eval_negatives_draws(const int64_t* seen_offsets, const int32_t* seen_sorted, int64_t user0, int64_t count,
                            int64_t item_num, int64_t n_neg, uint64_t seed, const uint64_t* table, int32_t* negs,
                            int32_t* n_drawn, int64_t* draws, void* stream);
int rs_eval_batch(const int64_t* hist_offsets, const int64_t* hist_items, const int64_t* extra, const int64_t* answer,
                  const int32_t* negs, int64_t user0, int64_t B, int64_t max_len, int64_t n_neg, int64_t mask_token,
                  int64_t* seq, int64_t* cand, int64_t* labels, void* stream);

/* ABI version of this header/library pair. */
int rs_abi_version(void);
/* sizeof of the structs of this header that bindings mirror (host only); -1 for an unknown index. */
enum {
  RS_SIZEOF_EPILOGUE = 0,
  RS_SIZEOF_WGRAD_PROBLEM = 1,
  RS_SIZEOF_REDUCE_SEGMENT = 2,
  RS_SIZEOF_SAS_EMBED_ARGS = 3,
  RS_SIZEOF_SAS_IN_ARGS = 4,
  RS_SIZEOF_SAS_HEAD_ARGS = 5,
  RS_SIZEOF_SAS_OUT_ARGS = 6,
  RS_SIZEOF_SAS_OUT_BWD_ARGS = 7,
  RS_SIZEOF_SAS_IN_BWD_ARGS = 8,
  RS_SIZEOF_SAS_IN_ATTN_ARGS = 9
};
int64_t rs_abi_sizeof(int which);

#ifdef __cplusplus
}
#endif
#endif
