/*
 * dstagnn.h — C-ABI of the MI355X-native DSTAGNN block (libdstagnn.so).
 *
 * Drop-in boundary for the hot path named by BASELINE.json.north_star:
 * DSTAGNN_block forward/backward of Ghoul-tn/DSTAGNN_Drought
 * (model/DSTAGNN_my.py:199-253).  The reference is pure Python/PyTorch with no
 * FFI; its "operator API" is the nn.Module surface.  The Python package
 * dstagnn_drought_amd mirrors that surface (make_model / DSTAGNN_block with the
 * same signatures and state_dict keys) and reaches the entry points below through
 * the PyTorch-ROCm operator library _C.so (TORCH_LIBRARY(dstagnn, ...),
 * csrc/torch_ops.cpp), which links this library.  No torch
 * types cross this boundary: plain device pointers, sizes and a hipStream_t.
 *
 * Conventions
 *   - All tensors are fp32, contiguous, row-major, device resident (HBM).
 *   - Every entry point is asynchronous on `stream` and returns 0 on success or a
 *     positive hipError_t / DSTAGNN_E_* code.  dstagnn_last_error() returns text.
 *   - Inputs are borrowed read-only; outputs are written (overwritten) in place.
 *   - No allocation happens inside any entry point: the caller passes a `save`
 *     buffer (kept from forward to backward) and a `scratch` buffer whose sizes
 *     come from dstagnn_block_sizes().
 */
#ifndef DSTAGNN_H
#define DSTAGNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dstagnn_stream_t; /* a hipStream_t (0 = default stream) */

#define DSTAGNN_MAX_K 8
#define DSTAGNN_HEAD_MAX_BLOCKS 16

enum {
  DSTAGNN_OK = 0,
  DSTAGNN_E_SHAPE = 10001,   /* shape / dims mismatch (reference raises RuntimeError)     */
  DSTAGNN_E_ARG = 10002,     /* null pointer or unsupported argument                      */
  DSTAGNN_E_SPACE = 10003    /* save / scratch buffer smaller than dstagnn_block_sizes()  */
};

/* res_att modes (ScaledDotProductAttention.forward, model/DSTAGNN_my.py:37):
 * 0 = the int 0 passed to the first block (DSTAGNN_submodule.forward:273)
 * 1 = tensor (B,1,h,T,T) broadcast over F (block 2 receives block 1's re_At)
 * 2 = tensor (B,F,h,T,T)                                                      */
enum { DSTAGNN_RES_NONE = 0, DSTAGNN_RES_BCAST = 1, DSTAGNN_RES_FULL = 2 };

/* dstagnn_block_dims::train is a word of flags (the struct keeps its layout): bit 0 turns the
 * dropout sites on; DSTAGNN_TRAIN_FIRST_MULTI marks a MULTI-FEATURE FIRST BLOCK — x (B,N,F,T)
 * with 1 <= F <= DSTAGNN_MAX_FIRST_F takes the first block's branches whatever F is:
 *   E = LN_N(x.permute(0,2,3,1) + P_T[t,:]) (B,F,T,N), one position row per t shared by the F
 *   features; tco = ReLU(tc); xres[b,c,n,t] = sum_f W_res[c,f] x[b,n,f,t] + b_res[c];
 *   out = LN_C(ReLU(xres + tco)).  Every parameter is used and gets a gradient; d_x is (B,N,F,T).
 * With the flag and F == 1 the call is the default first block, bit for bit.  Without it F must
 * be 1 or C (the reference's behaviour and error); with it, F outside 1..DSTAGNN_MAX_FIRST_F is
 * DSTAGNN_E_SHAPE.  Dropout is on when any bit other than DSTAGNN_TRAIN_FIRST_MULTI is set (so
 * every earlier caller's non-zero `train` keeps its meaning).                                */
enum { DSTAGNN_TRAIN_DROPOUT = 1, DSTAGNN_TRAIN_FIRST_MULTI = 256 };
#define DSTAGNN_MAX_FIRST_F 8

/* Shape of one DSTAGNN_block (DSTAGNN_block.__init__, model/DSTAGNN_my.py:200-201).
 * F = num_of_features of x (1 for the first block, else == C).               */
typedef struct dstagnn_block_dims {
  int B, N, F, T;          /* x is (B, N, F, T)                                   */
  int n_heads, d_k, d_v;   /* temporal attention (TAt)                            */
  int d_model;             /* D                                                   */
  int K;                   /* Chebyshev order == SAt heads (quirk 6)              */
  int C;                   /* nb_chev_filter == nb_time_filter                    */
  int res_mode;            /* DSTAGNN_RES_*                                       */
  int train;               /* DSTAGNN_TRAIN_* flags; bit 0: Dropout(0.05) at :234 and :221 active */
  float drop_p;            /* 0.05 in the reference                               */
  uint64_t seed;           /* dropout RNG seed (counter-based hash, per call)     */
  int cheb_sparse;         /* 1: aggregate over the CSC/CSR support in dstagnn_graph
                              (T_k elementwise recurrence => ~3 nnz/column, quirk 4);
                              0: dense (N,N) T_k.  Rows of any length C*T <= 2^20
                              (walked in 1024-element chunks).                      */
  int cheb_flash;          /* 1 (requires cheb_sparse, d_k == 32 and the flash fields of
                              dstagnn_graph): fused Chebyshev attention — the (B,K,N,N)
                              scores / softmax / score gradient are never materialised;
                              S tiles are recomputed from Q', K' on the matrix cores    */
  int cheb_nnz;            /* flash path: entries of the union support (== graph nnz)   */
  int cheb_apa_nnz;        /* flash path, N <= 512: entries of the adj_pa support (== graph apa_nnz) */
  int64_t sample_base;     /* global index of sample 0 of this call (>= 0): the dropout keep-mask
                              of an element is keyed by (seed, site, global sample index,
                              position), so data-parallel shards (rank r holds samples
                              [r*B, (r+1)*B) of the global batch) draw exactly the masks of a
                              1-GPU step on the concatenated batch                          */
} dstagnn_block_dims;

/* Parameter pointers in state_dict order.  For the first block
 * (F==1, or DSTAGNN_TRAIN_FIRST_MULTI) residual_conv / EmbedT are used; for inner blocks they are ignored
 * (their grads stay untouched, matching the reference's None grads, quirk 11). */
typedef struct dstagnn_block_params {
  const float* pre_conv_w;   /* (D, T, 1, F)          :207 */
  const float* pre_conv_b;   /* (D)                        */
  const float* embT_pos;     /* (T, N)   EmbedT.pos_embed  */
  const float* embT_g;       /* (N)      EmbedT.norm       */
  const float* embT_b;       /* (N)                        */
  const float* embS_pos;     /* (N, D)   EmbedS.pos_embed  */
  const float* embS_g;       /* (D)                        */
  const float* embS_b;       /* (D)                        */
  const float* tat_wq;       /* (h*dk, N) TAt.W_Q          */
  const float* tat_wk;       /* (h*dk, N)                  */
  const float* tat_wv;       /* (h*dv, N)                  */
  const float* tat_fc;       /* (N, h*dv)                  */
  const float* tat_ln_g;     /* (N)                        */
  const float* tat_ln_b;     /* (N)                        */
  const float* sat_wq;       /* (K*dk, D) SAt.W_Q          */
  const float* sat_wk;       /* (K*dk, D)                  */
  const float* theta[DSTAGNN_MAX_K]; /* (F, C) cheb_conv_SAt.Theta.k */
  const float* mask[DSTAGNN_MAX_K];  /* (N, N) cheb_conv_SAt.mask.k  */
  const float* gtu_w[3];     /* (2C, C, 1, k), k = 3,5,7   */
  const float* gtu_b[3];     /* (2C)                       */
  const float* res_w;        /* (C, F, 1, 1) residual_conv */
  const float* res_b;        /* (C)                        */
  const float* fcmy_w;       /* (T, 3T-12)                 */
  const float* fcmy_b;       /* (T)                        */
  const float* ln_g;         /* (C)                        */
  const float* ln_b;         /* (C)                        */
} dstagnn_block_params;

/* Same layout, writable: gradients (overwritten, not accumulated). */
typedef struct dstagnn_block_grads {
  float* pre_conv_w; float* pre_conv_b;
  float* embT_pos; float* embT_g; float* embT_b;
  float* embS_pos; float* embS_g; float* embS_b;
  float* tat_wq; float* tat_wk; float* tat_wv; float* tat_fc; float* tat_ln_g; float* tat_ln_b;
  float* sat_wq; float* sat_wk;
  float* theta[DSTAGNN_MAX_K]; float* mask[DSTAGNN_MAX_K];
  float* gtu_w[3]; float* gtu_b[3];
  float* res_w; float* res_b;
  float* fcmy_w; float* fcmy_b;
  float* ln_g; float* ln_b;
} dstagnn_block_grads;

/* Graph constants of cheb_conv_withSAt (init-time, lib/utils.py:149-203):
 * cheb = K stacked (N,N) Chebyshev polynomials T_k; adj_pa = (N,N) binary.
 * For the sparse path: the union support of T_0..T_{K-1} as CSC (per destination
 * column j the source rows i) and CSR (per row i the columns j), int32.          */
typedef struct dstagnn_graph {
  const float* cheb;     /* (K, N, N) */
  const float* adj_pa;   /* (N, N)    */
  int nnz;               /* entries of the union support (0 = none given)       */
  const int* csc_ptr;    /* (N+1) */
  const int* csc_row;    /* (nnz) */
  const int* csr_ptr;    /* (N+1) */
  const int* csr_col;    /* (nnz) */
  /* fused (flash) path only (cheb_flash = 1), else NULL / 0: */
  const int* csr2csc;          /* (nnz)  CSC position of every CSR entry                      */
  const int32_t* apa_bits;     /* (N, ceil(N/32)) bit j%32 of word [i][j/32] = adj_pa[i,j] != 0 */
  const int32_t* apa_bits_t;   /* (N, ceil(N/32)) bit i%32 of word [j][i/32] = adj_pa[i,j] != 0 */
  int apa_nnz;                 /* entries of the adj_pa support                                */
  const int* apa_ptr;          /* (N+1)  CSC of the adj_pa support: per column j ...            */
  const int* apa_row;          /* (apa_nnz) ... the rows i                                     */
  const float* tsupp;          /* (K, nnz) T_k on the union support, CSC order                  */
  /* flash path on small graphs (N <= 512), else NULL: */
  const int* csc2csr;          /* (nnz)  CSR position of every CSC entry (inverse of csr2csc)   */
  const int* apa_idx;          /* (N, N) index of (i, j) in the adj_pa CSC, -1 off the support  */
  const int* apa2t;            /* (apa_nnz) union-support CSC position of adj_pa entry q, or -1 */
} dstagnn_graph;

/* Bytes needed for the forward->backward `save` buffer and the per-call scratch. */
int dstagnn_block_sizes(const dstagnn_block_dims* d, size_t* save_bytes, size_t* scratch_bytes);

/* DSTAGNN_block.forward(x, res_att) -> (x_out, re_At)   (model/DSTAGNN_my.py:225-253)
 *   x       (B,N,F,T)      res_att  per res_mode (NULL for mode 0)
 *   out     (B,N,C,T)      re_at    (B,F,h,T,T)  pre-softmax TAt scores (quirk 7)  */
int dstagnn_block_forward(const dstagnn_block_dims* d, const dstagnn_block_params* p, const dstagnn_graph* g,
                          const float* x, const float* res_att, float* out, float* re_at,
                          void* save, size_t save_bytes, void* scratch, size_t scratch_bytes,
                          dstagnn_stream_t stream);

/* Forward-only form of the block (validation, test, prediction): the same `out` and `re_at`
 * bits as dstagnn_block_forward for the same arguments, but no tensor that only the backward
 * reads is written or allocated.  One workspace holds what a later forward kernel reads plus
 * the GEMM workspaces; its size comes from dstagnn_block_forward_only_size().  Conventions as
 * above: asynchronous on `stream`, no allocation, DSTAGNN_E_SPACE when `work` is too small, the
 * dims / graph errors (and texts) of dstagnn_block_forward.  d->train = 1 is legal: the dropout
 * masks are those of the training forward for the same seed and sample_base.  The forward bits
 * of dstagnn_block_paths() describe this call as well.  `work` holds nothing of use afterwards
 * and no backward can follow.                                                             */
int dstagnn_block_forward_only_size(const dstagnn_block_dims* d, size_t* work_bytes);
int dstagnn_block_forward_only(const dstagnn_block_dims* d, const dstagnn_block_params* p, const dstagnn_graph* g,
                               const float* x, const float* res_att, float* out, float* re_at,
                               void* work, size_t work_bytes, dstagnn_stream_t stream);

/* Introspection for parity tests: byte offset (from the 256-aligned start of `save`) and
 * element count of a tensor the forward keeps in `save`; the sign pattern of each is one of
 * the block's ReLU decisions, which an fp64 oracle can adopt where the pre-activation is
 * within rounding of 0.  which = 0: the Chebyshev output X = ReLU(cheb_conv_withSAt
 * pre-activation), layout (B,N,T,C) (:133); 1: tco = ReLU(X + tc) (first block ReLU(tc)),
 * layout (B,N,C,T) (:245/:247); 2: ReLU(residual + tco), layout (B,N,C,T) (:252). */
int dstagnn_block_save_offset(const dstagnn_block_dims* d, int which, size_t* offset_bytes, size_t* count);

/* Introspection for parity tests: the kernel path the block takes for these dims (and this
 * process's DSTAGNN_* environment knobs) as a bit set — so a test can assert that the kernels it
 * holds to the oracle are the ones that ran.  Pure function of its inputs; launches nothing. */
enum {
  DSTAGNN_PATH_SPARSE = 1,          /* cheb_conv_withSAt over the CSC/CSR union support          */
  DSTAGNN_PATH_FLASH = 2,           /* fused Chebyshev attention (cheb_flash.hip)                */
  DSTAGNN_PATH_FLASH_SMALL = 4,     /* ... its LDS-staged small-graph kernels (N <= 512)         */
  DSTAGNN_PATH_CHEB_AGG = 8,        /* aggregate-first Chebyshev aggregation (cheb_agg.hip)      */
  DSTAGNN_PATH_TAT_FUSED_FWD = 16,  /* temporal attention stage as one kernel (tat_fused.hip)    */
  DSTAGNN_PATH_TAT_FUSED_BWD = 32,  /* ... and its backward                                      */
  DSTAGNN_PATH_GTU_FUSED_FWD = 64,  /* GTU stage as one kernel (gtu_fused.hip)                   */
  DSTAGNN_PATH_GTU_FUSED_BWD = 128, /* ... and its backward                                      */
  DSTAGNN_PATH_SAT_LN_FUSED = 256,  /* retired (that kernel is gone): never reported             */
  DSTAGNN_PATH_FIRST_MULTI = 512    /* multi-feature first block (DSTAGNN_TRAIN_FIRST_MULTI, F > 1): the
                                       GTU stage runs the runtime-generic node kernels of gtu_tail.hip
                                       with the F -> C residual (never gtu_fused.hip or the C = 32
                                       compile-time tail)                                         */
};
int dstagnn_block_paths(const dstagnn_block_dims* d, uint32_t* bits);

/* Autograd backward of the block (replaces torch autograd over :225-253).
 *   d_out (B,N,C,T); d_re_at (B,F,h,T,T) or NULL (no gradient flows into re_At)
 *   d_x (B,N,F,T) written; d_res_att written per res_mode (NULL for mode 0)
 *   grads: every pointer used by this block kind is written.                     */
int dstagnn_block_backward(const dstagnn_block_dims* d, const dstagnn_block_params* p, const dstagnn_graph* g,
                           const float* x, const float* res_att, const float* d_out, const float* d_re_at,
                           float* d_x, float* d_res_att, const dstagnn_block_grads* grads,
                           void* save, size_t save_bytes, void* scratch, size_t scratch_bytes,
                           dstagnn_stream_t stream);

/* ---- individual hot-path operators (unit-testable pieces of the block) ---- */

/* cheb_conv_withSAt.forward (model/DSTAGNN_my.py:117-133).
 *   x (B,N,F,T); sat (B,K,N,N) spatial-attention scores (pre-softmax);
 *   theta_cat (F, K*C) = [Theta_0 | ... | Theta_{K-1}]; mask_cat (K,N,N);
 *   out (B,N,C,T) = ReLU(sum_k (T_k o softmax_i(sat_k + A_pa o M_k))^T x Theta_k)
 *   sparse = 1 aggregates over g's CSC/CSR support (W unused, may be NULL);
 *   save: P (B*K*N*N), W = T o P (dense path) and xTheta (B*N*K*C*T).           */
int dstagnn_cheb_sat_forward(int B, int N, int F, int T, int K, int C, int sparse,
                             const float* x, const float* sat, const float* theta_cat, const float* mask_cat,
                             const dstagnn_graph* g, float* out,
                             float* P, float* W, float* xth, void* scratch, size_t scratch_bytes,
                             dstagnn_stream_t stream);
/* Backward: d_out (B,N,C,T) -> d_x (B,N,F,T), d_sat (B,K,N,N), d_theta_cat (F,K*C),
 * d_mask_cat (K,N,N).  `out` is the forward output (ReLU mask).                  */
int dstagnn_cheb_sat_backward(int B, int N, int F, int T, int K, int C, int sparse,
                              const float* x, const float* theta_cat, const dstagnn_graph* g,
                              const float* out, const float* P, const float* W, const float* xth,
                              const float* d_out, float* d_x, float* d_sat, float* d_theta_cat, float* d_mask_cat,
                              void* scratch, size_t scratch_bytes, dstagnn_stream_t stream);

/* Generic strided fp32 GEMM on the f32 MFMA path (v_mfma_f32_32x32x2_f32):
 *   C(m,n) = alpha * sum_k A(m,k) B(k,n) + beta * C(m,n) + bias[n]   (opt. ReLU)
 * Every index may be a two-level affine map  off(i) = (i % div)*s0 + (i / div)*s1
 * (div = 0: off(i) = i*s0), so permuted / im2col views need no copies.          */
typedef struct dstagnn_idx { int64_t div, s0, s1; } dstagnn_idx;
typedef struct dstagnn_gemm_desc {
  int M, N, K, batch;
  const float* A; dstagnn_idx a_m, a_k, a_z; int64_t a_off;
  const float* B; dstagnn_idx b_k, b_n, b_z; int64_t b_off;
  float* C;       dstagnn_idx c_m, c_n, c_z; int64_t c_off;
  float alpha, beta;
  const float* bias; int64_t bias_stride;  /* bias[n*bias_stride], may be NULL */
  int relu;
} dstagnn_gemm_desc;
int dstagnn_gemm_f32(const dstagnn_gemm_desc* g, void* scratch, size_t scratch_bytes, dstagnn_stream_t stream);

/* Column sums used by every bias / LayerNorm-gamma/beta gradient of the block
 * (model/DSTAGNN_my.py:207,220,252 -- the autograd reductions of nn.Linear / nn.Conv2d
 * biases and nn.LayerNorm affine parameters):
 *   out[o*ostride] = beta*out[o*ostride] + sum_{a<A, i<I} in[(a*O + o)*I + i]
 * O*I <= 16384; A == 0 leaves out untouched.  Fixed summation order (bit-identical across launches); one launch with
 * an in-kernel ticketed two-level fold when I <= 256.  scratch >= 8 MB + 256.        */
int dstagnn_colsum(const float* in, int64_t A, int O, int I, float* out, int64_t ostride, float beta,
                   void* scratch, size_t scratch_bytes, dstagnn_stream_t stream);

/* The three GTU convolution weight and bias gradients of a block with C = 32, T = 12 as the
 * block's backward computes them where the fused GTU backward runs (gtu_dw_kernel + its fold):
 *   dw[q][o][c][j] = sum_{bn, t'} dconv[q][(bn Tg + t')][o] X[bn][t' + j][c],  db[q][o] = sum dconv[q][.][o]
 * for kernel widths kw = 3, 5, 7 (q = 0, 1, 2; Tg = 12 - kw + 1); dconv[q]: (BN Tg, 64), X: (BN, 12, 32),
 * all 16-B aligned.  chunks = 0: the planner's node partition; chunks > 0: that many chunks per
 * GTU (empty chunks allowed).  Fixed summation order: bit-identical from run to run.
 * scratch >= 32 MB + 256.  dstagnn_gtu_dw_plan: the planner's chunk counts per GTU for BN nodes on
 * the current device and the nodes per LDS stage. */
int dstagnn_gtu_dw(const float* const dconv[3], const float* X, int64_t BN, float* const dw[3], float* const db[3],
                   int chunks, void* scratch, size_t scratch_bytes, dstagnn_stream_t stream);
int dstagnn_gtu_dw_plan(int64_t BN, int chunks[3], int* stage_nodes);

/* Time `iters` back-to-back launches of one block stage with HIP events on
 * `stream`; writes the mean per-launch milliseconds.  stage: 0 = whole forward,
 * 2 = cheb_sat forward stage, 3 = pre_conv stage, 10 = the single kernel the
 * benchmark reports as dominant (gemm_f32_hot_kernel: the pre_conv fwd GEMM).
 * Buffers must be those of a preceding dstagnn_block_forward.                  */
int dstagnn_block_time_stage(const dstagnn_block_dims* d, const dstagnn_block_params* p, const dstagnn_graph* g,
                             const float* x, const float* res_att, float* out, float* re_at,
                             void* save, size_t save_bytes, void* scratch, size_t scratch_bytes,
                             int stage, int iters, float* ms_per_launch, dstagnn_stream_t stream);

/* Dropout keep-mask the block draws (value 1/(1-p) or 0) for tests:
 * which = 0 (EmbedS output, (B,N,D)), 1 (fcmy output, (B,N,C,T) order of out); samples
 * d->sample_base .. d->sample_base + B - 1 of the global batch. */
int dstagnn_dropout_mask(const dstagnn_block_dims* d, int which, float* mask, dstagnn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Model head of DSTAGNN_submodule (model/DSTAGNN_my.py:265-280, head.hip): replaces
 *   final_x = torch.cat(block outputs, -1); final_conv(final_x.permute(0,3,1,2))[..., -1]
 *   .permute(0,2,1); final_fc(.)
 * outs: nb device pointers (B,N,C,T) (host array); w1 final_conv.weight (O, nb*T, 1, C),
 * b1 (O); w2 final_fc.weight (P, O), b2 (P).  h (B,N,O) is the final_conv output (saved for
 * backward), y (B,N,P).  The cat is never materialised.  scratch >= dstagnn_head_scratch_bytes().
 * ------------------------------------------------------------------------------------- */
int64_t dstagnn_head_scratch_bytes(void);
int dstagnn_head_forward(int B, int N, int C, int T, int nb, int O, int P, const float* const* outs,
                         const float* w1, const float* b1, const float* w2, const float* b2, float* h, float* y,
                         void* scratch, size_t scratch_bytes, dstagnn_stream_t stream);
/* dy (B,N,P) -> dh (B,N,O) (scratch output), douts[j] (B,N,C,T) (NULL entries skipped),
 * dw1, db1, dw2, db2 (each may be NULL). */
int dstagnn_head_backward(int B, int N, int C, int T, int nb, int O, int P, const float* const* outs,
                          const float* w1, const float* w2, const float* h, const float* dy, float* dh,
                          float* const* douts, float* dw1, float* db1, float* dw2, float* db2, void* scratch,
                          size_t scratch_bytes, dstagnn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Optimiser step of the training driver (optim.hip): torch.optim.Adam as the reference builds
 * it (train_DSTAGNN_my.py:126: `optim.Adam(net.parameters(), lr=learning_rate)` — betas
 * (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad) over many fp32 tensors in ONE launch.
 * segs: device array of {param, grad, exp_avg, exp_avg_sq, n}; chunks: device array of nchunk
 * (segment index, element offset) pairs, one per dstagnn_adam_chunk_elems() elements of a
 * segment.  step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t) for step t.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
} dstagnn_adam_seg;
int dstagnn_adam_chunk_elems(void);
int dstagnn_adam_step(const dstagnn_adam_seg* segs, const int64_t* chunks, int nchunk, float beta1, float beta2,
                      float eps, float step_size, float bc2_sqrt, dstagnn_stream_t stream);

/* Opt-in extras of the optimiser step, over the same segment / chunk tables (optim.hip).
 *
 * dstagnn_grad_sumsq: stat[0] = sum of g^2 over every segment (double), stat[1] = sqrt(stat[0]),
 * the global L2 norm torch.nn.utils.clip_grad_norm_(norm_type=2) takes (there in fp32).  Only
 * the segments' g and n are read.  partials: nchunk floats of device scratch; stat: two doubles
 * on the device.  One launch, fixed summation order: the same bits on every call.  nchunk == 0
 * stores zeros.
 *
 * dstagnn_adam_step_ex: dstagnn_adam_step with, per element and in this order,
 *   max_norm > 0:    g = coef g, coef = min(1, max_norm / (sqrt(stat[0]) + 1e-6))
 *                    (torch.nn.utils.clip_grad_norm_; the gradient itself is not written);
 *   weight_decay > 0, decoupled == 0:  g += weight_decay p   (torch.optim.Adam(weight_decay=));
 *   weight_decay > 0, decoupled != 0:  p *= 1 - lr weight_decay before the update
 *                    (torch.optim.AdamW; lr is read for this only);
 *   skip_nonfinite != 0 and stat[0] not finite: nothing is stored (p, m, v keep their values)
 *                    and *skipped (device int, may be NULL) is incremented once.  The caller's
 *                    step count t still advances: step_size / bc2_sqrt of the next call are
 *                    those of t + 1, as if the skipped step had seen a zero update.
 * stat may be NULL when max_norm == 0 and skip_nonfinite == 0.
 *
 * dstagnn_grad_scale: g *= min(1, max_norm / (sqrt(stat[0]) + 1e-6)) in place over every
 * segment's g (written through the const pointer); with dstagnn_grad_sumsq in front, a
 * stand-alone clip_grad_norm_ in two launches.  A coefficient of 1 leaves every bit. */
typedef struct {
  float beta1, beta2, eps;
  float step_size, bc2_sqrt; /* as dstagnn_adam_step */
  float lr;                  /* decoupled weight decay only */
  float weight_decay;        /* 0: none */
  int decoupled;             /* 0: L2 (Adam), else decoupled (AdamW) */
  float max_norm;            /* 0: no clipping */
  int skip_nonfinite;
} dstagnn_adam_hyper;
int dstagnn_grad_sumsq(const dstagnn_adam_seg* segs, const int64_t* chunks, int nchunk, float* partials,
                       double* stat, dstagnn_stream_t stream);
int dstagnn_adam_step_ex(const dstagnn_adam_seg* segs, const int64_t* chunks, int nchunk,
                         const dstagnn_adam_hyper* hyper, const double* stat, int* skipped,
                         dstagnn_stream_t stream);
int dstagnn_grad_scale(const dstagnn_adam_seg* segs, const int64_t* chunks, int nchunk, const double* stat,
                       float max_norm, dstagnn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Training criterion and test-set scores (loss.hip).
 *
 * The criterion of train_DSTAGNN_my.py:132 (`nn.SmoothL1Loss()`) and its use at :156-157
 * (loss, loss.backward()), mean reduction, one launch per direction, plus the masked variants
 * the model family uses for series with gaps.  Per element, d = y - target in fp32:
 *   DSTAGNN_LOSS_SMOOTH_L1  |d| < param: 0.5 d^2 / param, else |d| - 0.5 param   (param = beta;
 *                           beta = 0 is DSTAGNN_LOSS_MAE)
 *   DSTAGNN_LOSS_HUBER      |d| <= param: 0.5 d^2, else param (|d| - 0.5 param)   (param = delta)
 *   DSTAGNN_LOSS_MAE        |d|          (derivative sign(d), sign(0) = 0)
 *   DSTAGNN_LOSS_MSE        d^2
 * An entry is valid under DSTAGNN_MASK_NONE always, under DSTAGNN_MASK_NEQ when
 * target != null_val, under DSTAGNN_MASK_NAN when target is not NaN (DSTAGNN_MASK_NEQ with a
 * NaN null_val means DSTAGNN_MASK_NAN).  loss = sum over valid entries / their count; no valid
 * entry: loss 0, gradient 0.  Invalid entries are selected out, never multiplied by zero: a NaN
 * target under the NaN mask leaves the loss finite and its gradient entry exactly 0.  A NaN
 * prediction at a valid entry makes the loss NaN.
 *
 * dstagnn_loss_forward: y, target (n floats) -> loss (one float), stat (two doubles: the fp64
 * sum of the terms and the valid count).  Terms in fp32, every add in fp64, fixed order: the
 * same bits on every call.  scratch: dstagnn_loss_scratch_bytes(n) bytes of device memory
 * (dstagnn_loss_tile_elems() elements per workgroup, the grid capped).
 * dstagnn_loss_backward: dy[i] = gout * l'(d_i) / count on valid entries, 0 elsewhere; count is
 * read from the forward's stat and gout (one float on the device, the upstream gradient; NULL
 * means 1) on the device: no host synchronisation.  Recomputes d from y and target.
 * Arguments are checked before anything touches the device: a null pointer, n outside
 * [1, 2^31), an unknown kind or mask mode, a negative or NaN param -> DSTAGNN_E_ARG.
 *
 * dstagnn_metrics_accumulate: pred, target (rows, P) -> table (P, 4) doubles on the device, a
 * RUNNING table the call adds to (zero it to start): per horizon p (the last axis) sum |e|,
 * sum e^2, sum over target != null_val of |e / target|, count of target != null_val, with
 * e = pred - target and e / target in fp32 (as lib/utils1.py:418-431 and lib/metrics.py:6-17
 * compute them on the host), the sums in fp64 in a fixed order (no atomics on floats: the same
 * bits on every call).  A NaN null_val counts the non-NaN targets.  MAE_p = table[p][0] / rows,
 * RMSE_p = sqrt(table[p][1] / rows), MAPE_p = 100 table[p][2] / table[p][3] (0 where the count
 * is 0).  1 <= P <= 256 and rows * P < 2^31, else DSTAGNN_E_SHAPE.  scratch:
 * dstagnn_metrics_scratch_bytes(rows, P) bytes.
 *
 * dstagnn_metrics_accumulate_masked: pred, target (B, N, P) -> htable (P, 8) and, unless NULL,
 * ntable (N, 8) doubles on the device, RUNNING tables the call adds to (zero them to start): per
 * horizon p, and per node n over all samples and horizons, eight sums over the VALID entries (the
 * criterion's rule above under mask_mode / null_val; selected out, never multiplied by zero):
 *   0 count   1 sum e   2 sum |e|   3 sum e^2   4 sum |e / t| over t != mape_null   5 its count
 *   6 sum t   7 sum t^2
 * with e = pred - t, e * e and e / t in fp32 as dstagnn_metrics_accumulate forms them, t and t * t
 * as doubles (exact), every add in fp64 in a fixed order (no atomics on floats: the same bits on
 * every call).  A NaN target under DSTAGNN_MASK_NAN leaves every sum finite; a NaN prediction at a
 * valid entry makes the sums NaN.  MAE = [2] / [0], RMSE = sqrt([3] / [0]), bias = [1] / [0],
 * MAPE = 100 [4] / [5], NSE = 1 - [3] / ([7] - [6]^2 / [0]).  One launch of ceil(N / (256 / P))
 * workgroups.  1 <= P <= 256, B, N >= 1 and B * N * P < 2^31, else DSTAGNN_E_SHAPE; a null pred /
 * target / htable / scratch or an unknown mask mode -> DSTAGNN_E_ARG; scratch smaller than
 * dstagnn_metrics_masked_scratch_bytes(B, N, P) bytes (0 for a shape it rejects) ->
 * DSTAGNN_E_SPACE.  All of it is checked before anything touches the device.
 * ------------------------------------------------------------------------------------- */
enum { DSTAGNN_LOSS_SMOOTH_L1 = 0, DSTAGNN_LOSS_HUBER = 1, DSTAGNN_LOSS_MAE = 2, DSTAGNN_LOSS_MSE = 3 };
enum { DSTAGNN_MASK_NONE = 0, DSTAGNN_MASK_NEQ = 1, DSTAGNN_MASK_NAN = 2 };
typedef struct {
  int kind;       /* DSTAGNN_LOSS_* */
  float param;    /* beta (smooth_l1) / delta (huber); ignored by mae / mse, still >= 0 */
  int mask_mode;  /* DSTAGNN_MASK_* */
  float null_val; /* DSTAGNN_MASK_NEQ only */
} dstagnn_loss_cfg;
int dstagnn_loss_tile_elems(void);
int64_t dstagnn_loss_scratch_bytes(int64_t n);
int dstagnn_loss_forward(const dstagnn_loss_cfg* cfg, int64_t n, const float* y, const float* target, float* loss,
                         double* stat, void* scratch, size_t scratch_bytes, dstagnn_stream_t stream);
int dstagnn_loss_backward(const dstagnn_loss_cfg* cfg, int64_t n, const float* y, const float* target,
                          const double* stat, const float* gout, float* dy, dstagnn_stream_t stream);
int64_t dstagnn_metrics_scratch_bytes(int64_t rows, int P);
int dstagnn_metrics_accumulate(int64_t rows, int P, const float* pred, const float* target, float null_val,
                               double* table, void* scratch, size_t scratch_bytes, dstagnn_stream_t stream);
int64_t dstagnn_metrics_masked_scratch_bytes(int64_t B, int64_t N, int P);
int dstagnn_metrics_accumulate_masked(int64_t B, int64_t N, int P, const float* pred, const float* target,
                                      int mask_mode, float null_val, float mape_null, double* htable,
                                      double* ntable /* may be NULL */, void* scratch, size_t scratch_bytes,
                                      dstagnn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Quantile forecasts (loss.hip): the pinball criterion and the calibration sums.
 *
 * Levels: tau_0 < tau_1 < ... < tau_{Q-1}, each strictly inside (0, 1), strictly increasing,
 * 1 <= Q <= DSTAGNN_MAX_QUANTILES; anything else is DSTAGNN_E_ARG.  They are fp32; the kernels
 * use tau and 1 - tau, the latter formed once on the host in fp32.
 * Layout: a quantile prediction is (M, Q) floats, q fastest (a (B, N, P, Q) head output with
 * M = B N P); the target stays (M).
 * Pinball term of d = y_q - t (the library's sign convention, d in fp32):
 *   d > 0: (1 - tau_q) d, slope 1 - tau_q      d < 0: tau_q (-d), slope -tau_q
 *   d = 0: 0, slope 0 (DSTAGNN_LOSS_MAE's sign(0) = 0)      a NaN d stays NaN
 * (Q = 1, tau = 0.5: half of DSTAGNN_LOSS_MAE.)  An entry is valid by its TARGET under the rule
 * above (DSTAGNN_MASK_*; selected out, never multiplied by zero).
 *   loss = sum over valid entries and levels of the term / (count_valid Q)
 * no valid entry: loss 0, gradient 0; a NaN prediction at a valid entry: a NaN loss.  Terms in
 * fp32, every add in fp64 in a fixed order: the same bits on every call.
 *
 * dstagnn_pinball_forward: y (m, Q), target (m) -> loss (one float), stat (two doubles: the
 * fp64 sum of the terms and count_valid).  scratch: dstagnn_pinball_scratch_bytes(m, Q) bytes.
 * dstagnn_pinball_backward: dy[i, q] = slope gout / (count_valid Q) on valid entries, exactly 0
 * at masked entries and where d = 0; count_valid from the forward's stat and gout (one float on
 * the device, NULL means 1) are read on the device: no host synchronisation.
 * A null pointer, a level or mask mode outside the rules -> DSTAGNN_E_ARG; m < 1 or
 * m Q >= 2^31 -> DSTAGNN_E_SHAPE; a short scratch -> DSTAGNN_E_SPACE.
 *
 * dstagnn_metrics_accumulate_quantile: pred (B, N, P, Q), target (B, N, P) -> htable
 * (P, 2 + 3 Q) and, unless NULL, ntable (N, 2 + 3 Q) doubles on the device, RUNNING tables the
 * call adds to (zero them to start), over the valid entries:
 *   0        count of valid entries
 *   1        count of crossing entries (some y_{q+1} < y_q: the Q predictions are not non-decreasing)
 *   2 + 3 q  sum of the pinball term of level q (fp32 term, fp64 add)
 *   3 + 3 q  count of t <= y_q (fp32 compare, exact)
 *   4 + 3 q  sum of y_q, each cast to double (exact terms)
 * One launch of ceil(N / (256 / P)) workgroups, fixed order, no atomics on floats.
 * 1 <= P <= 256, 1 <= Q <= 16, B, N >= 1 and B N P Q < 2^31, else DSTAGNN_E_SHAPE; a null cfg /
 * pred / target / htable / scratch, an unknown mask mode or a level outside the rule ->
 * DSTAGNN_E_ARG; scratch smaller than dstagnn_metrics_quantile_scratch_bytes(B, N, P, Q) (0 for
 * a shape it rejects) -> DSTAGNN_E_SPACE.  All of it is checked before anything touches the device.
 * ------------------------------------------------------------------------------------- */
#define DSTAGNN_MAX_QUANTILES 16
typedef struct {
  int mask_mode;     /* DSTAGNN_MASK_* */
  float null_val;    /* DSTAGNN_MASK_NEQ only */
  int num_quantiles; /* Q */
  float tau[DSTAGNN_MAX_QUANTILES]; /* the first Q are read */
} dstagnn_pinball_cfg;
int64_t dstagnn_pinball_scratch_bytes(int64_t m, int num_quantiles);
int dstagnn_pinball_forward(const dstagnn_pinball_cfg* cfg, int64_t m, const float* y, const float* target,
                            float* loss, double* stat, void* scratch, size_t scratch_bytes,
                            dstagnn_stream_t stream);
int dstagnn_pinball_backward(const dstagnn_pinball_cfg* cfg, int64_t m, const float* y, const float* target,
                             const double* stat, const float* gout, float* dy, dstagnn_stream_t stream);
int64_t dstagnn_metrics_quantile_scratch_bytes(int64_t B, int64_t N, int P, int num_quantiles);
int dstagnn_metrics_accumulate_quantile(int64_t B, int64_t N, int P, const dstagnn_pinball_cfg* cfg,
                                        const float* pred, const float* target, double* htable,
                                        double* ntable /* may be NULL */, void* scratch, size_t scratch_bytes,
                                        dstagnn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Training windows cut from the raw series on the device (windows.hip): what prepareData.py
 * (:63-161) materialises once per label position, per batch instead.
 *
 * dstagnn_window_gather: ONE launch, no host sync.  series (L, N, F), fp64 when series_f64 else
 * fp32 (call that type S); rel (Tin) int32 time offsets relative to a label position, in the
 * order read_and_generate_dataset concatenates its windows (week, day, hour kinds; each kind its
 * windows oldest first; an offset may be >= 0); labels (S) int64 label positions of a split;
 * idx (B) int64 positions in that table (a slice of an epoch permutation as it is); mean, std
 * (F) of type S.  Writes, with label_b = labels[idx[b]],
 *   x (B, N, F, Tin) fp32:  x[b,n,f,t] = float((S(series[label_b + rel[t], n, f]) - mean[f]) / std[f])
 *   y (B, N, P)      fp32:  y[b,n,p]   = float(series[label_b + p, n, F - 1])
 * the subtraction and the (correctly rounded) division in S, rounded to fp32 once at the end: the
 * operations of numpy's `(x - mean) / std` (prepareData.py:149-161) followed by
 * `.type(torch.FloatTensor)` (lib/utils1.py:302-312), bit for bit.  The caller validates the
 * tables (every label + rel[t] and label + p inside [0, L)); the kernel still never reads outside
 * the series: an idx[b] outside [0, S) makes x[b] and y[b] NaN, a time step outside [0, L) makes
 * that row NaN.  A workgroup handles dstagnn_window_tile_nodes(F, Tin) consecutive nodes of one
 * sample (chosen so that its LDS image stays at 32 KiB; dstagnn_window_gather_lds_bytes(F, Tin, P)
 * is the launch's dynamic LDS, which must not exceed 64 KiB: DSTAGNN_E_SHAPE).  All of L (< 2^31),
 * N, F, Tin, P, S, B >= 1, else DSTAGNN_E_SHAPE.
 *
 * dstagnn_window_stats: the z-score statistics of a training split from the raw series, in fp64.
 * w (L) int32: the number of (training label, window offset) pairs that land on time step s;
 * wtotal = N * sum(w).  stats (2 F) fp64 = {mean[F], std[F]} with mean[f] = sum w x / wtotal and
 * std[f] = sqrt(sum w (x - mean[f])^2 / wtotal) (ddof = 0): numpy's train.mean / train.std over
 * axes (0, 1, 3) of the materialised windows.  Two launches (the second centres on the first
 * one's mean), sums in a fixed order: the same bits on every call.  1 <= F <= 256, else
 * DSTAGNN_E_SHAPE; wtotal > 0, else DSTAGNN_E_ARG.  scratch:
 * dstagnn_window_stats_scratch_bytes(L, F) bytes.
 *
 * Series with gaps.  An element v of the series (type S) is MISSING when null_val is NaN
 * (std::isnan, as dstagnn_metrics_accumulate reads its null_val) and v != v, otherwise when
 * v == S(null_val) (IEEE ==: -0.0 == 0.0, and a NaN element is then valid).
 *
 * dstagnn_window_stats_masked: dstagnn_window_stats over the valid elements only:
 * wvalid[f] = sum_s w[s] * #valid(s, ., f) (int64, exact), mean[f] = sum_valid w x / wvalid[f],
 * std[f] = sqrt(sum_valid w (x - mean[f])^2 / wvalid[f]).  Same launches, threads and fp64 fold
 * order: on a series with no missing element stats equals dstagnn_window_stats' bits.  A feature
 * with wvalid[f] == 0 gives NaN.  scratch: dstagnn_window_stats_masked_scratch_bytes(L, F).
 *
 * dstagnn_window_fill_forward: the one-time forward fill along time.  filled (L, N, F) of type S:
 * a valid element is copied; a missing one takes the value of the latest valid step p < s of its
 * (n, f) over the whole series, if one exists and s - p <= max_gap (max_gap = 0: unlimited;
 * < 0: DSTAGNN_E_ARG); otherwise it keeps its marker, bits unchanged.  Never reads a later step.
 * counts (2, F) int64 = {missing elements per feature, how many of them were filled}.  Two
 * launches over chunks of dstagnn_window_fill_chunk() time steps and workgroups of
 * dstagnn_window_fill_cols() columns e = n F + f: the first writes every (chunk, column)'s last
 * valid step into scratch (int32; dstagnn_window_fill_scratch_bytes(L, N, F) bytes), the second
 * finds its carry there and walks its chunk.  L < 2^31, 1 <= F <= 256, filled != series.
 *
 * dstagnn_window_gather_masked: dstagnn_window_gather with the inputs read from xsrc and the
 * targets from ysrc (both (L, N, F) of type S; they may be the same array):
 *   x[b,n,f,t] = valid(v) ? float((v - mean[f]) / std[f]) : +0.0f,  v = xsrc[label_b + rel[t], n, f]
 *   y[b,n,p]   = float(ysrc[label_b + p, n, F-1])   (raw: the marker stays for the masked loss)
 * Same tile, LDS and checks as dstagnn_window_gather.
 * ------------------------------------------------------------------------------------- */
int dstagnn_window_tile_nodes(int F, int Tin);
int64_t dstagnn_window_gather_lds_bytes(int F, int Tin, int P);
int dstagnn_window_gather(int series_f64, const void* series, int64_t L, int N, int F, const int32_t* rel, int Tin,
                          int P, const int64_t* labels, int64_t S, const int64_t* idx, int B, const void* mean,
                          const void* std, float* x, float* y, dstagnn_stream_t stream);
int64_t dstagnn_window_stats_scratch_bytes(int64_t L, int F);
int dstagnn_window_stats(int series_f64, const void* series, int64_t L, int N, int F, const int32_t* w, double wtotal,
                         double* stats, void* scratch, size_t scratch_bytes, dstagnn_stream_t stream);
int64_t dstagnn_window_stats_masked_scratch_bytes(int64_t L, int F);
int dstagnn_window_stats_masked(int series_f64, const void* series, int64_t L, int N, int F, const int32_t* w,
                                double null_val, double* stats, int64_t* wvalid, void* scratch, size_t scratch_bytes,
                                dstagnn_stream_t stream);
int dstagnn_window_fill_chunk(void);
int dstagnn_window_fill_cols(void);
int64_t dstagnn_window_fill_scratch_bytes(int64_t L, int N, int F);
int dstagnn_window_fill_forward(int series_f64, const void* series, int64_t L, int N, int F, double null_val,
                                int64_t max_gap, void* filled, int64_t* counts, void* scratch, size_t scratch_bytes,
                                dstagnn_stream_t stream);
int dstagnn_window_gather_masked(int series_f64, const void* xsrc, const void* ysrc, int64_t L, int N, int F,
                                 const int32_t* rel, int Tin, int P, const int64_t* labels, int64_t S,
                                 const int64_t* idx, int B, const void* mean, const void* std, double null_val, float* x,
                                 float* y, dstagnn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Skill against persistence and the seasonal climatology (windows.hip: the climatology table;
 * loss.hip: the sums).  Both baseline forecasts are read straight out of the raw (L, N, F) series
 * (type S: fp64 when series_f64, else fp32; the target feature is F - 1) inside the scoring launch:
 * nothing is materialised.  A series element is missing by the windows section's rule (`masked` /
 * `src_masked` = 0: nothing is; 1: null_val NaN -> v != v, a number -> v == S(null_val)); an fp32
 * target is valid by the criterion's rule (mask_mode / null_val, DSTAGNN_MASK_*).
 *
 * dstagnn_climatology: clim (period, N) fp64 and cnt (period, N) int32 on the device:
 * cnt[phi, n] = the observed s[t, n, F-1] over the steps t in [0, t_end) with t mod period == phi
 * (the phase of the absolute series index), clim[phi, n] = their sum / cnt, each value converted to
 * double and added in increasing t, one division; cnt == 0 gives clim = NaN (the climatology is
 * undefined there).  Nothing at or beyond t_end is read.  One launch, one thread per (phi, n), n
 * fastest.  L, N, F >= 1, L N F < 2^31, period N < 2^31, 1 <= period <= L and 1 <= t_end <= L,
 * else DSTAGNN_E_SHAPE; a null series / clim / cnt, or a NaN null_val with masked = 0 ->
 * DSTAGNN_E_ARG.
 *
 * dstagnn_skill_accumulate: pred, target (B, N, P) fp32 and pos (B) int64 on the device, pos[b] =
 * the label position l_b of sample b (its targets are the steps l_b .. l_b + P - 1) -> htable
 * (P, 13) and, unless NULL, ntable (N, 13) doubles on the device, RUNNING tables the call adds to
 * (zero them to start).  pers_src (L, N, F) of type S is the series, or its unlimited forward fill
 * (dstagnn_window_fill_forward, max_gap = 0) when it has gaps: the persistence value of (b, n) is
 * pers_src[l_b - 1, n, F-1], undefined when l_b - 1 < 0 or when that element is (still) missing.
 * clim / cnt: dstagnn_climatology's tables; the climatology of (b, n, p) is
 * clim[(l_b + p) mod period, n], undefined where cnt is 0.  Per entry, with y the prediction, t the
 * target, q = float(persistence), c = float(climatology), all differences in fp32:
 * e_m = y - t, e_p = q - t, e_c = c - t, a_f = y - c, a_o = t - c.
 * Over the entries where t is valid AND persistence is defined:
 *   0 count   1 sum e_m e_m   2 sum e_p e_p   3 sum |e_m|   4 sum |e_p|
 * over the entries where t is valid AND the climatology is defined:
 *   5 count   6 sum e_m e_m   7 sum e_c e_c   8 sum |e_m|   9 sum |e_c|
 *   10 sum a_f a_o   11 sum a_f^2   12 sum a_o^2
 * the squares of columns 1, 2, 6, 7 in fp32 (as dstagnn_metrics_accumulate_masked forms e * e),
 * the products of 10 - 12 as doubles (exact), every add in fp64 in a fixed order, no atomics on
 * floats: the same bits on every call.  The model and a baseline are summed over the SAME entries.
 * Entries are selected out, never multiplied by zero: a NaN target under DSTAGNN_MASK_NAN reaches
 * no sum; a NaN prediction at a counted entry makes the sums NaN.  A sample with l_b < 0 or
 * l_b + P > L contributes nothing and nothing outside the series is read.
 * MSE skill over persistence = 1 - [1] / [2], over climatology = 1 - [6] / [7]; MAE skill =
 * 1 - [3] / [4], 1 - [8] / [9]; anomaly correlation = [10] / sqrt([11] [12]).
 * One launch of ceil(N / (256 / P)) workgroups, no host synchronisation.  1 <= P <= 256, B, N, L,
 * F >= 1, B N P, L N F and period N < 2^31, 1 <= period <= L, else DSTAGNN_E_SHAPE; a null pred /
 * target / pers_src / pos / clim / cnt / htable / scratch, an unknown mask mode, or a NaN src_null
 * with src_masked = 0 -> DSTAGNN_E_ARG; scratch smaller than dstagnn_skill_scratch_bytes(B, N, P)
 * (0 for a shape it rejects) -> DSTAGNN_E_SPACE.  All of it is checked before anything touches
 * the device.
 * ------------------------------------------------------------------------------------- */
#define DSTAGNN_SKILL_COLS 13
int dstagnn_climatology(int series_f64, const void* series, int64_t L, int64_t N, int64_t F, int64_t period,
                        int64_t t_end, int masked, double null_val, double* clim, int32_t* cnt,
                        dstagnn_stream_t stream);
int64_t dstagnn_skill_scratch_bytes(int64_t B, int64_t N, int P);
int dstagnn_skill_accumulate(int64_t B, int64_t N, int P, const float* pred, const float* target, int mask_mode,
                             float null_val, int series_f64, const void* pers_src, int64_t L, int64_t F,
                             int src_masked, double src_null, const int64_t* pos, const double* clim,
                             const int32_t* cnt, int64_t period, double* htable, double* ntable /* may be NULL */,
                             void* scratch, size_t scratch_bytes, dstagnn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Drought event scores (loss.hip): the class contingency counts of a forecast against K thresholds
 * on the index, per horizon and per node.
 *
 * dstagnn_events_accumulate: pred, target (B, N, P) fp32 and thr fp32 on the device -> htable
 * (P, cols) and, unless NULL, ntable (N, cols) doubles on the device, cols = 2 + (K + 1)^2, RUNNING
 * tables the call adds to (zero them to start).  Every value in them is an integer, exact in fp64.
 * thr is (K) when thr_per_node = 0 (one set for every node) or (K, N) row-major when 1, in the units
 * of target, mildest first.  Event k of a value v is v <= thr_k (above = 0) or v >= thr_k
 * (above = 1), every compare in fp32 (a value equal to the threshold is an event); the class of v
 * is c(v) = the number of events that hold, 0 .. K.  A target is valid by the criterion's rule
 * (mask_mode / null_val, DSTAGNN_MASK_*); an invalid one reaches no count.  A node one of whose
 * thresholds is NaN is excluded: none of its entries reaches any count (callers make such a column
 * all NaN; the library does not read the thresholds on the host).
 *   column 0                   entries with a valid target on a node that is not excluded
 *   column 1                   those among them whose prediction is NaN (they reach no cell)
 *   column 2 + co (K + 1) + cf the entries of observed class co = c(target), forecast class cf = c(pred)
 * so column 0 = column 1 + the sum of the cells.  +-inf predictions and targets are ordinary
 * values; a NaN target that the mask lets through has class 0.
 * One launch of ceil(N / (256 / P)) workgroups, no host synchronisation; the cells are uint32
 * histograms in (P + 256 / P) cols 4 bytes of LDS under integer atomic adds (no floating-point
 * atomics): the same bits on every call.  1 <= P <= 256, 1 <= K <= DSTAGNN_MAX_EVENT_LEVELS, B,
 * N >= 1, B N P and K N < 2^31, the LDS bytes <= 64 KiB (refuses only K = 7 with P = 1 or P >= 248: 257 rows), else
 * DSTAGNN_E_SHAPE; a null pred / target / thr / htable / scratch, an unknown mask mode, above or
 * thr_per_node outside {0, 1} -> DSTAGNN_E_ARG; scratch smaller than
 * dstagnn_events_scratch_bytes(B, N, P, K) (0 for a shape it rejects) -> DSTAGNN_E_SPACE.  All of
 * it is checked before anything touches the device.
 * ------------------------------------------------------------------------------------- */
#define DSTAGNN_MAX_EVENT_LEVELS 7
int64_t dstagnn_events_scratch_bytes(int64_t B, int64_t N, int P, int K);
int dstagnn_events_accumulate(int64_t B, int64_t N, int P, int K, int above, const float* pred, const float* target,
                              int mask_mode, float null_val, const float* thr, int thr_per_node, double* htable,
                              double* ntable /* may be NULL */, void* scratch, size_t scratch_bytes,
                              dstagnn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Graph builders (stag.hip).  fp64 throughout, like the reference's numpy/scipy code.
 * ------------------------------------------------------------------------------------- */

/* STAG_gen per-node preprocessing (data/STAG_gen.py:47-54 applied once per node instead of
 * once per pair): data (T,N,F) -> xhat (N,T,F) unit rows (zero rows stay 0), p (N,T)
 * marginals |x_t| / (sum_t |x_t| + 1e-12) with the 1e-12 zero-norm guard, psum (N) = sum p. */
int dstagnn_stag_prep(const double* data, int T, int N, int F, double* xhat, double* p, double* psum,
                      dstagnn_stream_t stream);

/* STAG_gen exact EMD of node pairs (replaces process_node_pair + wasserstein_distance,
 * data/STAG_gen.py:17-59, which solve the dense LP with scipy linprog/HiGHS).
 * pairs (P,2) int32 node ids; out (P) the optimal transport cost under
 * D = clip(1 - xhat_i xhat_j^T, 0, 1), or 1.0 where the reference's LP is infeasible
 * (marginal totals differ by > 1e-7, e.g. an all-zero node; status 1).  status (P): 0 ok,
 * 1 infeasible (1.0 returned, as the reference), 2 solver pivot cap (a bug: raise).
 * pivots (P) optional (may be NULL).  Needs 2T+1 <= 32767 and
 * dstagnn_stag_emd_lds_bytes(T,F) <= 160 KiB (T <= ~1100 at F = 4). */
int64_t dstagnn_stag_emd_lds_bytes(int T, int F);
int dstagnn_stag_emd_pairs(const double* xhat, const double* p, const double* psum, int T, int N, int F,
                           const int32_t* pairs, int64_t P, double* out, int32_t* status, int64_t* pivots,
                           dstagnn_stream_t stream);

/* STAG_gen on a series with gaps.  An element v of data (T,N,F) is MISSING by the rule of the
 * window calls above: when null_val is NaN, v != v; otherwise v == null_val (IEEE ==; a NaN
 * element is then valid and poisons its node as in dstagnn_stag_prep).  Step t of node n is
 * OBSERVED when none of its F features is missing; cnt[n] counts the observed steps.
 *
 * dstagnn_stag_prep_masked: dstagnn_stag_prep over the observed steps only, compacted in their
 * order to the front of the node's slices: row r < cnt[n] of xhat (N,T,F) / p (N,T) is the
 * node's r-th observed step, tidx (N,T) int32 its original step; beyond cnt[n] xhat and p are 0
 * and tidx is -1.  p_r = |x_r| / (sum over observed |x| + 1e-12), the 1e-12 zero-norm guard
 * kept on observed all-zero rows; psum (N) = sum p (0 for a node with no observed step).  On a
 * series with no missing element xhat, p and psum have dstagnn_stag_prep's bits.
 *
 * dstagnn_stag_emd_pairs_masked: the EMD of pair (i, j) is the optimal transport cost between
 * the two nodes' norm distributions, each on its OWN observed steps: rows = the cnt[i] observed
 * steps of i with their p, columns = the cnt[j] observed steps of j, cost
 * clip(1 - xhat_r . xhat_c, 0, 1) — the reference's LP restricted to those rows and columns,
 * equivalently the full T x T LP with zero marginals at the missing steps.  With cnt == T
 * everywhere, out, status and pivots are dstagnn_stag_emd_pairs'.  A node is EXCLUDED when
 * cnt[n] < min_observed (min_observed >= 1, else DSTAGNN_E_ARG); a pair with an excluded node,
 * or whose totals differ by > 1e-7 (e.g. a node whose observed rows are all zero), gets 1.0 with
 * status 1.  status 2: solver pivot cap; 3: a cnt above Tmax (both bugs: raise).  Tmax >= every
 * cnt[n] of a node in `pairs`, 1 <= Tmax <= T: the LDS workspace is
 * dstagnn_stag_emd_lds_bytes_rect(Tmax, Tmax), sized by the longest observed support and not by
 * T.  Needs 2 Tmax + 1 <= 32767 and that size <= 160 KiB.
 * dstagnn_stag_emd_lds_bytes_rect(Tr, Tc): the workspace of one Tr x Tc problem. */
int dstagnn_stag_prep_masked(const double* data, int T, int N, int F, double null_val, double* xhat, double* p,
                             double* psum, int32_t* cnt, int32_t* tidx, dstagnn_stream_t stream);
int64_t dstagnn_stag_emd_lds_bytes_rect(int Tr, int Tc);
int dstagnn_stag_emd_pairs_masked(const double* xhat, const double* p, const double* psum, const int32_t* cnt, int T,
                                  int Tmax, int min_observed, int N, int F, const int32_t* pairs, int64_t P,
                                  double* out, int32_t* status, int64_t* pivots, dstagnn_stream_t stream);

/* Batched wasserstein_distance(p, q, D) (data/STAG_gen.py:17-38): p, q (B,T), D (B,T,T) dense
 * costs (nan -> 0, +-inf -> +-1e12 as the reference).  1.0 / status 1 when infeasible
 * (negative mass or totals differing by > 1e-7). */
int dstagnn_emd_dense(const double* p, const double* q, const double* D, int T, int64_t B, double* out,
                      int32_t* status, dstagnn_stream_t stream);

/* fast_STAG_gen.calculate_distances, symmetrised with a zero diagonal
 * (data/fast_STAG_gen.py:16-35, 57-59): coords (N,Dc), feats (N,Fp) -> sta (N,N). */
int dstagnn_fast_stag_distances(const double* coords, int N, int Dc, const double* feats, int Fp, double max_distance,
                                double* sta, dstagnn_stream_t stream);

/* Per-row top-k adjacency.  mode 0 = fast_STAG_gen (:66-74): the k smallest sta[i,:],
 * A = 1, R = 1 - sta.  mode 1 = STAG_gen (:105-116): adj = 1 - sta + I, the k smallest
 * adj[i,:], A = 1, R = adj.  Ties go to the lower column index (np.argsort kind='stable';
 * the reference's default quicksort leaves tie order unspecified).  A, R (N,N) are fully
 * written; nbr (N,k) optional, ascending by (key, index).  N <= 8192. */
int dstagnn_graph_topk(const double* sta, int N, int k, int mode, double* A, double* R, int32_t* nbr,
                       dstagnn_stream_t stream);

/* dstagnn_graph_topk with excluded nodes.  excluded (N) uint8, non-zero = excluded; NULL means
 * dstagnn_graph_topk exactly.  An excluded node is never a neighbour: its key sorts after every
 * real key (a NaN's included).  An excluded node's own row of A and R is all zero and its nbr
 * row all -1.  Any other row takes min(k, #eligible columns) neighbours, the eligible columns
 * being the non-excluded ones (the row's own included, as in dstagnn_graph_topk); the rest of
 * its nbr row is -1.  Same checks (k <= N, N <= 8192). */
int dstagnn_graph_topk_masked(const double* sta, int N, int k, int mode, const uint8_t* excluded, double* A,
                              double* R, int32_t* nbr, dstagnn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * GEMM-family profiling (benchmark support).  dstagnn_prof_start(capacity) arms a timing
 * event pair around each of the next `capacity` GEMM calls (kernel + split-K fold, on the
 * stream they are issued on) and makes the block run on ONE stream (no side-stream overlap,
 * so each duration is that GEMM's own); dstagnn_prof_stop() synchronises and sums.
 * ------------------------------------------------------------------------------------- */
typedef struct dstagnn_prof_stats {
  double launches;  /* GEMM calls recorded                                      */
  double flops;     /* sum of 2*M*N*K*batch                                     */
  double bytes;     /* sum of minimum operand bytes 4*(MK + KN + MN (x2 if beta)) */
  double ms;        /* sum of event-measured durations                          */
  double max_ms;    /* longest single call                                      */
  double dropped;   /* calls beyond capacity (not recorded)                     */
} dstagnn_prof_stats;
int dstagnn_prof_start(int capacity);
int dstagnn_prof_stop(dstagnn_prof_stats* stats);
/* The recorded calls of the last start/stop window one by one (what the family sums are made of):
 * kind says which kernel computed the product, so the benchmark can report the dominant single
 * kernel (its own FLOP, bytes and duration) beside the family.  Returns the window's record
 * count; copies min(count, cap) records into out (may be NULL to query). */
enum {
  DSTAGNN_PROF_GEMM = 0,           /* gemm_f32 kernel(s) of one call + split-K fold             */
  DSTAGNN_PROF_SKINNY = 1,         /* skinny_dw_kernel (long skinny weight-gradient reduction)  */
  DSTAGNN_PROF_TAT_FUSED_FWD = 2,  /* tat_fused_fwd_kernel                                      */
  DSTAGNN_PROF_TAT_FUSED_BWD = 3,  /* tat_fused_bwd_kernel                                      */
  DSTAGNN_PROF_GTU_FUSED_FWD = 4,  /* gtu_fwd_fused_kernel                                      */
  DSTAGNN_PROF_GTU_FUSED_BWD = 5,  /* gtu_bwd_fused_kernel                                      */
  DSTAGNN_PROF_GTU_TCONV = 6,      /* gtu_tconv sliding-window convolution gradient             */
  DSTAGNN_PROF_SAT_FUSED = 7,      /* retired (that kernel is gone): never reported             */
  DSTAGNN_PROF_GTU_DW = 8          /* gtu_dw_kernel + its fold (GTU convolution weight gradients) */
};
typedef struct dstagnn_prof_record {
  double flops;  /* algorithmic FLOP of the call   */
  double bytes;  /* algorithmic (minimum) bytes    */
  double ms;     /* HIP-event duration             */
  int kind;      /* DSTAGNN_PROF_*                 */
} dstagnn_prof_record;
int dstagnn_prof_records(dstagnn_prof_record* out, int cap);

/* Split-K policy of the GEMMs: a GEMM with a grid below 128 workgroups splits its K range
 * over about `target` workgroups (default 448).  target = 1 never splits a tiled GEMM, so those
 * reductions run in one fixed order and a sample's data-path results (outputs, d_x, d_res_att)
 * are bit-identical at any batch size (parity tests).  Excluded: the skinny weight-gradient
 * kernel (batch-1 GEMMs with M <= 96, N <= 32, K >= 4096: the fcmy and dTheta gradients) always
 * splits K over up to 256 workgroups with a fixed-order fold — deterministic run to run, but
 * its summation order depends on K (so on B).  Returns the previous target; target <= 0 only
 * queries. */
int dstagnn_set_splitk_target(int target);

/* Operand precision of the GEMM family (every contraction of the block, its gradients and
 * the head): 0 = fp32 (default; the reference's arithmetic), 1 = bf16 operands (round to
 * nearest even) with fp32 accumulation on v_mfma_f32_32x32x16_bf16.  Softmax, LayerNorm,
 * the fused attention kernels and all reductions stay fp32.  An opt-in variant with its own
 * tolerance (tests/test_gpu_parity.py::test_bf16_gemm_variant); not a drop-in for the fp32
 * reference.  Returns the previous setting; on < 0 only queries. */
int dstagnn_set_gemm_bf16(int on);

const char* dstagnn_last_error(void);
int dstagnn_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DSTAGNN_H */
