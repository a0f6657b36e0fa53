// block.hip — DSTAGNN_block forward / backward orchestration and the C-ABI (include/dstagnn.h).
//
// Mirrors DSTAGNN_block.forward (model/DSTAGNN_my.py:225-253) stage by stage; every
// stage is one of our own HIP kernels (gemm.hip, ops.hip) launched asynchronously on
// the caller's stream.  Layouts in HBM (fp32, row-major):
//   x (B,N,F,T)           E (B,F,T,N)          qkv (B*F*T, 2h*dk+h*dv)
//   O (B,F,T,N)           Zd (B*N, D)          qk  (B*N, 2K*dk)  [Q' | K']
//   P, W (B,K,N,N)        xth (B,N,K,C,T) = x Theta_k (the Theta-first order of the
//                         Chebyshev product, so the aggregation writes (B,N,C,T) directly)
//   X (B,N,C,T)           conv_g (B*N, 2C, T-k+1)   G (B*N, C, 3T-12)   out (B,N,C,T)
#include <algorithm>
#include <atomic>
#include <vector>
#include <cstring>
#include <mutex>
#include <string>

#include "common.hpp"
#include <chrono>
#include <cstdio>
#include <initializer_list>
#include <map>
#include <utility>
#include "ops.hpp"
#include "streams.hpp"

static thread_local std::string g_last_error;
void set_last_error(const std::string& s) { g_last_error = s; }

namespace {

// ------------------------------------------------------------------------------
// buffer plan: carving of the save / scratch buffers (identical in sizes/fwd/bwd)
// ------------------------------------------------------------------------------
struct Arena {
  char* base;
  size_t off = 0;
  explicit Arena(void* b) : base((char*)b) {}
  float* take(size_t floats) {
    off = (off + 255) & ~size_t(255);
    float* p = base ? (float*)(base + off) : nullptr;
    off += floats * sizeof(float);
    return p;
  }
};

constexpr size_t kGemmWs = size_t(8) << 20;   // floats (32 MB) for split-K partial slabs
constexpr size_t kPart = size_t(2) << 20;      // floats (8 MB) for column-sum partials

struct Dims {
  int B, N, F, T, h, dk, dv, D, K, C;
  int64_t FT, BFT, BN, NN, HQ, HV, QW, KD, KC, CT, KCT, S;
  int Tg[3], ks[3];
  bool first, sparse, flash;
  bool mf;          // multi-feature first block (DSTAGNN_TRAIN_FIRST_MULTI, F > 1): F -> C residual, generic tail
  bool fsmall;      // flash on a small graph (flash_small): the LDS-staged kernels
  bool agg;         // sparse path in aggregate-first order (cheb_agg.hip): no x Theta GEMM
  bool dth;         // ... with dTheta from the transposed SpMM itself: agg_k is not stored
  bool tfused;      // the temporal-attention stage as one kernel per direction (tat_fused.hip)
  int NP;           // tfused: node count padded to 16 (the re-laid Q|K|V weights' row length)
  bool tfused_bwd;  // ... and its backward (tat_fused.hip)
  bool gfused;      // the GTU stage forward as one kernel (gtu_fused.hip)
  bool gbfused;     // ... and its backward (gtu_fused.hip): compact gate-gradient rows, no tconv
  int64_t tf_wg;    // tfused_bwd: its workgroups (one gamma / beta partial row each)
  int64_t nnz;      // flash: union-support entries
  int64_t apa_nnz;  // small-graph flash: A_pa support entries
};

// dstagnn_block_dims::train is a flag word: the first-block flag, and dropout on any other bit
bool first_flag(const dstagnn_block_dims& d) { return (d.train & DSTAGNN_TRAIN_FIRST_MULTI) != 0; }
bool drop_on(const dstagnn_block_dims& d) { return (d.train & ~DSTAGNN_TRAIN_FIRST_MULTI) != 0 && d.drop_p > 0.f; }

Dims mkdims(const dstagnn_block_dims& d) {
  Dims m;
  m.B = d.B; m.N = d.N; m.F = d.F; m.T = d.T; m.h = d.n_heads; m.dk = d.d_k; m.dv = d.d_v;
  m.D = d.d_model; m.K = d.K; m.C = d.C;
  m.FT = (int64_t)m.F * m.T; m.BFT = (int64_t)m.B * m.FT; m.BN = (int64_t)m.B * m.N; m.NN = (int64_t)m.N * m.N;
  m.HQ = (int64_t)m.h * m.dk; m.HV = (int64_t)m.h * m.dv; m.QW = 2 * m.HQ + m.HV; m.KD = (int64_t)m.K * m.dk;
  m.KC = (int64_t)m.K * m.C; m.CT = (int64_t)m.C * m.T; m.KCT = m.KC * m.T; m.S = 3 * (int64_t)m.T - 12;
  for (int g = 0; g < 3; ++g) { m.ks[g] = 3 + 2 * g; m.Tg[g] = m.T - m.ks[g] + 1; }
  m.first = first_flag(d) || m.F == 1;
  m.mf = m.first && m.F > 1;
  m.sparse = d.cheb_sparse != 0;
  m.flash = m.sparse && d.cheb_flash != 0;
  m.nnz = m.flash ? d.cheb_nnz : 0;
  m.fsmall = m.flash && flash_small(m.N);
  static const bool agg_env = env_flag("DSTAGNN_CHEB_AGG", true);
  m.agg = agg_env && m.sparse && cheb_agg_ok(m.F, m.C, m.K, m.T);
  m.dth = m.agg && cheb_agg_dtheta_fused(m.B, m.N, m.F, m.C, m.K, m.T, (int64_t)kGemmWs);
  m.apa_nnz = m.fsmall ? std::max(d.cheb_apa_nnz, 0) : 0;
  m.tfused = tat_fused_fwd_ok(m.N, m.T, m.h, m.dk, m.dv);
  m.NP = m.tfused ? tat_fused_np(m.N) : 0;
  m.tfused_bwd = m.tfused && tat_fused_bwd_ok(m.N, m.T, m.h, m.dk, m.dv, m.F, d.res_mode);
  m.tf_wg = m.tfused_bwd ? tat_fused_bwd_wgs(m.BFT) : 0;
  // (a multi-feature first block's F -> C residual lives in the runtime-generic tail kernels only)
  m.gfused = !m.mf && gtu_fused_fwd_ok(m.C, m.T);
  m.gbfused = !m.mf && gtu_fused_bwd_ok(m.C, m.T);
  return m;
}

struct SaveBufs {
  // parameters re-laid once per forward (Fwd::stage_params) and reused by the backward:
  // stacked projections [Wq; Wk; Wv] (QW, N) and [W_Q'; W_K'] (2KD, D), pre_conv as
  // (D, F*T), Theta_cat (F, K*C), GTU conv weights (o, j, c) fwd and (j', o, c) flipped bwd
  float *Wqkv, *Wqk, *Wp, *thcat, *Wgf[3], *Wgb[3];
  float* Wqkv_p;  // tfused: [Wq; Wk; Wv] with rows zero-padded to NP
  float *WfcT, *WqT;  // tfused_bwd: W_fc^T (h dv, NP) and [Wq; Wk; Wv]^T (NP, 3 h dk), zero-padded
  float* Wgt[3];      // gfused: GTU weights (o, j, c) for the fused GTU forward
  float *E, *qkv, *att, *ctx, *u_tat, *mu_tat, *rs_tat, *O, *u_s, *mu_s, *rs_s, *Zd, *qk, *P, *W, *xth, *X;
  float *lse, *psupp, *wsupp;  // flash path: column log-sum-exp (B,K,N), P and T o P on the support (B,K,nnz)
  float *am, *amt, *papa;      // small-graph flash: A_pa o M_k (K,N,N) and its transpose, P on the A_pa support
  float* conv[3];
  float *G, *tco, *r, *mu_c, *rs_c, *u_et, *mu_et, *rs_et;
};

// The one plan of the save arena, for the training pair (train: forward + backward over `save`) and
// for the forward-only workspace (dstagnn_block_forward_only).  One line per slot:
//   slot(member, floats, fwd, bwd)   fwd: a LATER FORWARD kernel reads it; bwd: the backward reads it
// The training plan takes a slot when either holds, the forward-only plan when fwd does; every other
// member is null: the stage functions pass the nulls on, the launchers pick the kernels'
// SAVE = false forms (neither the store nor the pointer), Fwd::stage_params skips the re-layout.
// Who writes and who reads each slot, path by path: DESIGN.md §14.4.
// Forward-only, one reuse: everything from E to xth is dead once X is written, and in an inner
// block with the unfused TAt stage X takes E's place (both (B N, C T) floats): E's last reader is
// the TAt LayerNorm on the caller's stream, X's writer the Chebyshev aggregation, later on that stream.
SaveBufs plan_bufs(const Dims& m, Arena& a, bool train) {
  SaveBufs s{};
  auto slot = [&](float*& p, int64_t floats, bool fwd, bool bwd) {
    if (fwd || (train && bwd)) p = a.take(floats);
  };
  const bool tf = m.tfused, tb = m.tfused_bwd, gf = m.gfused, gb = m.gbfused, e = m.first || !tf;
  const int64_t BK = (int64_t)m.B * m.K;
  slot(s.Wqkv, m.QW * m.N, !tf, !tb);
  slot(s.Wqkv_p, m.QW * m.NP, tf, false);
  slot(s.WfcT, m.HV * m.NP, false, tb);
  slot(s.WqT, m.QW * m.NP, false, tb);
  for (int g = 0; g < 3; ++g) slot(s.Wgt[g], 2 * (int64_t)m.C * m.C * m.ks[g], gf, false);
  slot(s.Wqk, 2 * m.KD * m.D, true, true);
  slot(s.Wp, (int64_t)m.D * m.FT, true, true);
  slot(s.thcat, (int64_t)m.F * m.KC, true, true);
  for (int g = 0; g < 3; ++g) slot(s.Wgf[g], 2 * (int64_t)m.C * m.C * m.ks[g], !gf, gb);  // (also the fused backward's)
  for (int g = 0; g < 3; ++g) slot(s.Wgb[g], 2 * (int64_t)m.C * m.C * m.ks[g], false, !gb);
  slot(s.E, m.BFT * m.N, e, e);  // (fused TAt, inner block: x is read in place, by tat_wqkv_grad too)
  slot(s.qkv, m.BFT * m.QW, !tf, true);
  slot(s.att, m.BFT * m.h * m.T, !tf, true);
  slot(s.ctx, m.BFT * m.HV, !tf, true);
  slot(s.u_tat, m.BFT * m.N, !tf, true);
  slot(s.mu_tat, m.BFT, false, true);
  slot(s.rs_tat, m.BFT, false, true);
  slot(s.O, m.BFT * m.N, true, true);
  slot(s.u_s, m.BN * m.D, true, true);
  slot(s.mu_s, m.BN, false, true);
  slot(s.rs_s, m.BN, false, true);
  slot(s.Zd, m.BN * m.D, true, true);
  slot(s.qk, m.BN * 2 * m.KD, true, true);
  slot(s.P, BK * m.NN, !m.flash, !m.flash);
  slot(s.W, BK * m.NN, !m.sparse, !m.sparse);
  slot(s.lse, BK * m.N, m.flash && !m.fsmall, m.flash);
  slot(s.psupp, BK * m.nnz, false, m.flash);
  slot(s.wsupp, BK * m.nnz, m.flash, m.flash);
  slot(s.am, (int64_t)m.K * m.NN, m.fsmall, m.fsmall);
  slot(s.amt, (int64_t)m.K * m.NN, false, m.fsmall);
  slot(s.papa, std::max<int64_t>(1, BK * m.apa_nnz), false, m.fsmall);
  slot(s.xth, m.BN * m.KCT, !m.agg, !m.dth);  // x Theta (Theta-first) | agg_k (m.dth: they stay in LDS)
  if (!train && !m.first && !tf) s.X = s.E;
  else slot(s.X, m.BN * m.CT, true, true);
  for (int g = 0; g < 3; ++g) slot(s.conv[g], m.BN * 2 * m.C * std::max(m.Tg[g], 0), !gf, true);
  // (the fused backward recomputes the gates; the unfused forward tail's SAVE form stores G with
  // tco, mu and rs whichever backward follows)
  slot(s.G, m.BN * m.C * m.S, false, !gf || !gb);
  slot(s.tco, m.BN * m.CT, false, true);
  slot(s.r, m.BN * m.CT, false, true);
  slot(s.mu_c, m.BN * m.T, false, true);
  slot(s.rs_c, m.BN * m.T, false, true);
  slot(s.u_et, m.BFT * m.N, false, m.first);
  slot(s.mu_et, m.BFT, false, m.first);
  slot(s.rs_et, m.BFT, false, m.first);
  return s;
}

struct Scratch {
  float *gemm_ws, *part;
  // bwd (the *_side workspaces belong to the side stream; gcon_* / bcon_* / dres_t are
  // per-stage so the side stream's reductions never race a later main-chain write)
  float *gemm_ws_side, *part_side, *dWqkv, *dWqk;
  float *dtc, *dX, *gpre, *gcon_t, *bcon_t, *dres_t, *gcon_s, *bcon_s, *gcon_a, *gcon_e, *dconv[3], *dW, *dxth,
      *dthcat, *dqk, *dZd, *dY, *dWp, *dO, *dU, *dE, *dctx, *dqkv, *dscore, *du_et, *dGt;
  float *dzs, *dzs_r, *cc;  // flash path: P o dP on the support (B,K,nnz; dzs_r in CSR order), c (B,K,N)
};

Scratch plan_scratch(const Dims& m, Arena& a) {
  Scratch s;
  s.gemm_ws = a.take(kGemmWs);
  s.part = a.take(kPart);
  s.dtc = a.take(m.BN * m.CT);
  s.dX = a.take(m.BN * m.CT);
  s.gpre = a.take(m.BN * m.CT);
  s.gemm_ws_side = a.take(kGemmWs);
  s.part_side = a.take(kPart);
  s.dWqkv = a.take(m.QW * m.N);
  s.dWqk = a.take(2 * m.KD * m.D);
  // (the fused GTU backward's ticket-tree rows live here too: at small B they outgrow BN CT)
  s.gcon_t = a.take(m.gbfused ? std::max<int64_t>(m.BN * m.CT, gtu_fused_bwd_part_floats(m.BN)) : m.BN * m.CT);
  // (first block: the residual_conv partials [bn][C F] | [bn][C]; they outgrow BN CT where F + 1 > T)
  s.bcon_t = a.take(std::max<int64_t>(m.BN * m.CT, m.first ? m.BN * m.C * (m.F + 1) : 0));
  s.dres_t = a.take(m.BN * m.CT);
  s.gcon_s = a.take(m.BN * m.D);
  s.bcon_s = a.take(m.BN * m.D);
  s.gcon_a = a.take(m.BFT * m.N);
  s.gcon_e = m.first ? a.take(m.BFT * m.N) : nullptr;
  for (int g = 0; g < 3; ++g) s.dconv[g] = a.take((m.BN * m.T + m.ks[g] - 1) * 2 * m.C);  // gtu_tail.hip layout
  s.dW = m.flash ? nullptr : a.take((int64_t)m.B * m.K * m.NN);
  s.dzs = m.flash ? a.take((int64_t)m.B * m.K * m.nnz) : nullptr;
  s.dzs_r = m.fsmall ? a.take((int64_t)m.B * m.K * m.nnz) : nullptr;
  s.cc = m.flash ? a.take((int64_t)m.B * m.K * m.N) : nullptr;
  s.dxth = m.agg ? nullptr : a.take(m.BN * m.KCT);
  s.dthcat = a.take((int64_t)m.F * m.KC);
  s.dqk = a.take(m.BN * 2 * m.KD);
  s.dZd = a.take(m.BN * m.D);
  s.dY = a.take(m.BN * m.D);
  s.dWp = a.take((int64_t)m.D * m.FT);
  s.dO = a.take(m.BFT * m.N);
  s.dU = a.take(m.BFT * m.N);
  s.dE = a.take(m.BFT * m.N);
  s.dctx = a.take(m.BFT * m.HV);
  s.dqkv = a.take(m.BFT * m.QW);
  s.dscore = a.take(m.BFT * m.h * m.T);
  s.du_et = m.first ? a.take(m.BFT * m.N) : nullptr;
  s.dGt = gtu_tail_bwd_split(m.C, m.T, m.first ? m.F : 0) ? a.take(m.BN * m.C * m.S) : nullptr;  // long series only
  return s;
}

// The forward-only workspace: plan_bufs' forward-only plan and the two GEMM workspaces (one per
// stream).  The split GTU tail (long series: gates | fcmy GEMM | tail) has two intermediates of its
// own: G goes through the main GEMM workspace a chunk of nodes at a time (Fwd::stage_tail; that
// workspace is idle from the convolutions on), the fcmy output through the out buffer itself.
struct WorkBufs {
  SaveBufs s;
  Scratch w;
};

WorkBufs plan_work(const Dims& m, Arena& a) {
  WorkBufs k{};
  k.s = plan_bufs(m, a, false);
  k.w.gemm_ws = a.take(kGemmWs);
  k.w.gemm_ws_side = a.take(kGemmWs);
  return k;
}

size_t plan_work_size(const Dims& m) {
  Arena a(nullptr);
  plan_work(m, a);
  return a.off + 256;
}

void plan_sizes(const Dims& m, size_t* save, size_t* scratch) {
  Arena a(nullptr);
  plan_bufs(m, a, true);
  *save = a.off + 256;
  Arena b(nullptr);
  plan_scratch(m, b);
  *scratch = b.off + 256;
}

int check_dims(const dstagnn_block_dims* d) {
  if (!d) { set_last_error("null dims"); return DSTAGNN_E_ARG; }
  if (d->B <= 0 || d->N <= 0 || d->F <= 0 || d->T <= 0 || d->n_heads <= 0 || d->d_k <= 0 || d->d_v <= 0 ||
      d->d_model <= 0 || d->K <= 0 || d->C <= 0) {
    set_last_error("non-positive dimension");
    return DSTAGNN_E_SHAPE;
  }
  if (d->K > DSTAGNN_MAX_K) { set_last_error("K > DSTAGNN_MAX_K"); return DSTAGNN_E_SHAPE; }
  if (d->T < 7) { set_last_error("T must be >= 7 (GTU kernel 7, fcmy 3T-12)"); return DSTAGNN_E_SHAPE; }
  if (d->cheb_sparse && !cheb_sparse_ok(d->C * d->T)) {
    set_last_error("cheb_sparse requires 0 < C*T <= 2^20");
    return DSTAGNN_E_SHAPE;
  }
  if (d->cheb_flash && (!d->cheb_sparse || d->d_k != 32 || d->cheb_nnz <= 0 || d->B > 128)) {
    set_last_error("cheb_flash requires cheb_sparse, d_k == 32, cheb_nnz > 0 and B <= 128");
    return DSTAGNN_E_SHAPE;
  }
  if (d->sample_base < 0) { set_last_error("sample_base < 0"); return DSTAGNN_E_ARG; }
  if (first_flag(*d)) {
    if (d->F > DSTAGNN_MAX_FIRST_F) {
      set_last_error("multi-feature first block: F = " + std::to_string(d->F) + " exceeds the limit of " +
                     std::to_string(DSTAGNN_MAX_FIRST_F) + " input features (1 <= F <= " +
                     std::to_string(DSTAGNN_MAX_FIRST_F) + ")");
      return DSTAGNN_E_SHAPE;
    }
  } else if (d->F != 1 && d->F != d->C) {
    // the reference fails at model/DSTAGNN_my.py:252 (x.permute + time_conv_output)
    set_last_error("The size of tensor a (" + std::to_string(d->F) + ") must match the size of tensor b (" +
                   std::to_string(d->C) + ") at non-singleton dimension 1");
    return DSTAGNN_E_SHAPE;
  }
  return 0;
}

// Dropout mask index offset of a dropout site (which 0: after EmbedS, (B,N,D) order; 1: after
// fcmy, (B,N,C,T) order): the keep-mask of an element is a hash of (seed, site, global index),
// and the global index counts from sample `sample_base` (a data-parallel shard's first sample in
// the global batch), so a sharded train step draws exactly the masks of the 1-GPU step on the
// concatenated batch.
uint64_t drop_off(const dstagnn_block_dims& d, int which) {
  const uint64_t per = which == 0 ? (uint64_t)d.N * d.d_model : (uint64_t)d.N * d.C * d.T;
  return (uint64_t)d.sample_base * per;
}

// ------------------------------------------------------------------------------
// Chebyshev graph convolution with spatial attention (cheb_conv_withSAt :117-133)
// ------------------------------------------------------------------------------
struct ChebIO {
  int B, N, F, T, K, C;
  const float* x;
  const float* S;          // scores (B,K,N,N) (may alias P)
  const float* const* mask;
  const dstagnn_graph* g;  // cheb (K,N,N), adj_pa, and the CSC/CSR support
  bool sparse;
  const float* thcat;      // (F, K*C)
  float *P, *W, *xth, *X;  // W unused (null) on the sparse path; xth (B,N,T,K,C), X (B,N,T,C)
  const ChebFl* fl = nullptr;  // fused (flash) attention: softmax statistics + support P, no dense P
  bool agg = false;            // aggregate-first order (cheb_agg.hip): xth holds the aggregates (B,N,K,F,T)
};

ChebSp make_sp(int B, int N, int K, int C, int T, const dstagnn_graph* g) {
  ChebSp a;
  a.B = B; a.N = N; a.K = K; a.CT = C * T; a.C = C;
  a.csc_ptr = g->csc_ptr; a.csc_row = g->csc_row; a.csr_ptr = g->csr_ptr; a.csr_col = g->csr_col;
  a.cheb = g->cheb;
  return a;
}

int cheb_softmax(const ChebIO& c, hipStream_t st) {
  if (c.fl) return op_flash_forward(*c.fl, st);
  ChebSm sm;
  sm.B = c.B; sm.K = c.K; sm.N = c.N; sm.S = c.S; sm.apa = c.g->adj_pa; sm.cheb = c.g->cheb; sm.P = c.P;
  sm.W = c.sparse ? nullptr : c.W;
  for (int k = 0; k < c.K; ++k) sm.mask[k] = c.mask[k];
  return op_cheb_softmax_fwd(sm, st);
}

// xth[(b,i,t),(k,c)] = sum_f x[b,i,f,t] Theta_k[f,c]   (plain row-major (B*N*T, K*C))
int cheb_xtheta(const ChebIO& c, float* ws, hipStream_t st) {
  const int64_t KC = (int64_t)c.K * c.C, T = c.T, FT = (int64_t)c.F * T;
  Gemm g;
  g.M = c.B * c.N * c.T; g.N = (int)KC; g.K = c.F;
  g.A = c.x; g.am = idx2(T, 1, FT); g.ak = idx1(T);
  g.B = c.thcat; g.bk = idx1(KC); g.bn = idx1(1);
  g.C = c.xth; g.cm = idx1(KC); g.cn = idx1(1);
  return run_gemm(g, ws, kGemmWs, st);
}

ChebAg make_ag(int B, int N, int K, int F, int C, int T, const dstagnn_graph* g) {
  ChebAg a;
  a.B = B; a.N = N; a.K = K; a.F = F; a.C = C; a.T = T; a.KC = K * C;
  a.csc_ptr = g->csc_ptr; a.csc_row = g->csc_row; a.csr_ptr = g->csr_ptr; a.csr_col = g->csr_col;
  a.csr2csc = g->csr2csc; a.cheb = g->cheb;
  return a;
}

// X[b,j,(t,c)] = relu( sum_{k,i} W[b,k,i,j] xth[b,i,t,k,c] )
// (aggregate-first: X = relu( sum_k (sum_i W[b,k,i,j] x_i)^T Theta_k ), xth holding the aggregates)
int cheb_aggregate(const ChebIO& c, float* ws, hipStream_t st) {
  const int64_t NN = (int64_t)c.N * c.N, KC = (int64_t)c.K * c.C, T = c.T, CT = (int64_t)c.C * T, KCT = KC * T;
  if (c.agg) {
    ChebAg a = make_ag(c.B, c.N, c.K, c.F, c.C, c.T, c.g);
    a.x = c.x; a.thcat = c.thcat; a.P = c.P; a.agg = c.xth; a.X = c.X;
    if (c.fl) { a.wsupp = c.fl->wsupp; a.nnz = c.fl->nnz; }
    return op_cheb_agg_fwd(a, st);
  }
  if (c.sparse) {
    ChebSp sp = make_sp(c.B, c.N, c.K, c.C, c.T, c.g);
    sp.P = c.P; sp.xth = c.xth; sp.out = c.X;
    if (c.fl) { sp.wsupp = c.fl->wsupp; sp.nnz = c.fl->nnz; }
    return op_cheb_spmm_fwd(sp, st);
  }
  Gemm g;
  g.M = c.N; g.N = (int)CT; g.K = c.K * c.N; g.batch = c.B;
  g.A = c.W; g.am = idx1(1); g.ak = idx2(c.N, c.N, NN); g.az = idx1(c.K * NN);
  g.B = c.xth; g.bk = idx2(c.N, KCT, c.C); g.bn = idx2(c.C, 1, KC); g.bz = idx1(c.N * KCT);
  g.C = c.X; g.cm = idx1(CT); g.cn = idx1(1); g.cz = idx1(c.N * CT);
  g.relu = 1;
  return run_gemm(g, ws, kGemmWs, st);
}

int cheb_forward(const ChebIO& c, float* ws, hipStream_t st) {
  DS_TRY(cheb_softmax(c, st));
  if (!c.agg) DS_TRY(cheb_xtheta(c, ws, st));
  return cheb_aggregate(c, ws, st);
}

struct ChebGradIO {
  int B, N, F, T, K, C;
  const float* x;
  const float* thcat;
  const dstagnn_graph* g;
  bool sparse;
  const float *P, *W, *xth;
  const float* gpre;       // d(pre-ReLU out) (B,N,T,C)
  float* dx;               // accumulated (beta = dx_beta)
  float dx_beta;
  float* dz;               // (B,K,N,N) d scores
  float* dthcat;           // (F, K*C)
  float* const* dmask;     // K pointers (N,N)
  float* dxth;             // scratch (B,N,T,K,C)
};

int cheb_backward(const ChebGradIO& c, float* ws, hipStream_t st) {
  const int64_t NN = (int64_t)c.N * c.N, KC = (int64_t)c.K * c.C, T = c.T, CT = (int64_t)c.C * T,
                KCT = KC * T, FT = (int64_t)c.F * T;
  if (c.sparse) {
    // dW only on the support (zero elsewhere); dxth by the transposed sparse product
    hipError_t e = hipMemsetAsync(c.dz, 0, sizeof(float) * (size_t)c.B * c.K * NN, st);
    if (e != hipSuccess) { set_last_error(std::string("memset: ") + hipGetErrorString(e)); return (int)e; }
    ChebSp sp = make_sp(c.B, c.N, c.K, c.C, c.T, c.g);
    sp.P = c.P; sp.xth = c.xth; sp.g = c.gpre; sp.dW = c.dz; sp.dxth = c.dxth;
    DS_TRY(op_cheb_sddmm_bwd(sp, st));
    DS_TRY(op_cheb_spmm_t_bwd(sp, st));
  }
  // dW[b,k,i,j] = sum_ct xth[b,i,k,ct] g[b,j,ct]
  if (!c.sparse) {
    Gemm g;
    g.M = c.N; g.N = c.N; g.K = (int)CT; g.batch = c.B * c.K;
    g.A = c.xth; g.am = idx1(KCT); g.ak = idx2(c.C, 1, KC); g.az = idx2(c.K, c.C, c.N * KCT);
    g.B = c.gpre; g.bk = idx1(1); g.bn = idx1(CT); g.bz = idx2(c.K, 0, c.N * CT);
    g.C = c.dz; g.cm = idx1(c.N); g.cn = idx1(1); g.cz = idx1(NN);
    DS_TRY(run_gemm(g, ws, kGemmWs, st));
  }
  // dxth[b,i,k,ct] = sum_j W[b,k,i,j] g[b,j,ct]
  if (!c.sparse) {
    Gemm g;
    g.M = c.N; g.N = (int)CT; g.K = c.N; g.batch = c.B * c.K;
    g.A = c.W; g.am = idx1(c.N); g.ak = idx1(1); g.az = idx1(NN);
    g.B = c.gpre; g.bk = idx1(CT); g.bn = idx1(1); g.bz = idx2(c.K, 0, c.N * CT);
    g.C = c.dxth; g.cm = idx1(KCT); g.cn = idx2(c.C, 1, KC); g.cz = idx2(c.K, c.C, c.N * KCT);
    DS_TRY(run_gemm(g, ws, kGemmWs, st));
  }
  // softmax backward in place: dz = P * (T o dW - colsum(P T o dW))
  ChebSm sm;
  sm.B = c.B; sm.K = c.K; sm.N = c.N; sm.apa = c.g->adj_pa; sm.cheb = c.g->cheb; sm.P = const_cast<float*>(c.P);
  sm.dW = c.dz; sm.dz = c.dz;
  for (int k = 0; k < c.K; ++k) sm.dmask[k] = c.dmask[k];
  DS_TRY(op_cheb_softmax_bwd(sm, st));
  DS_TRY(op_cheb_mask_grad(sm, st));
  // dTheta_cat[f,(k,c)] = sum_{b,i,t} x[b,i,f,t] dxth[b,i,t,k,c]
  {
    Gemm g;
    g.M = c.F; g.N = (int)KC; g.K = c.B * c.N * c.T;
    g.A = c.x; g.am = idx1(T); g.ak = idx2(T, 1, FT);
    g.B = c.dxth; g.bk = idx1(KC); g.bn = idx1(1);
    g.C = c.dthcat; g.cm = idx1(KC); g.cn = idx1(1);
    DS_TRY(run_gemm(g, ws, kGemmWs, st));
  }
  // dx[b,i,f,t] += sum_{k,c} Theta_k[f,c] dxth[b,i,t,k,c]
  {
    Gemm g;
    g.M = c.B * c.N * c.T; g.N = c.F; g.K = (int)KC;
    g.A = c.dxth; g.am = idx1(KC); g.ak = idx1(1);
    g.B = c.thcat; g.bk = idx1(1); g.bn = idx1(KC);
    g.C = c.dx; g.cm = idx2(T, 1, FT); g.cn = idx1(T);
    g.beta = c.dx_beta;
    DS_TRY(run_gemm(g, ws, kGemmWs, st));
  }
  return 0;
}

int unpack_theta(const float* thcat, int K, int F, int C, float* const* dtheta, hipStream_t st) {
  PackTheta a;
  a.K = K; a.F = F; a.C = C; a.unpack = 1; a.cat_in = thcat;
  for (int k = 0; k < K; ++k) a.dst[k] = dtheta[k];
  return op_pack_theta(a, st);
}

// the fused (flash) Chebyshev attention's arguments (cheb_flash.hip)
ChebFl make_fl(const Dims& m, const dstagnn_block_params& p, const dstagnn_graph& g, const SaveBufs& s) {
  ChebFl f;
  f.B = m.B; f.N = m.N; f.K = m.K; f.nnz = (int)m.nnz; f.nw = (m.N + 31) / 32;
  f.scale = 1.f / sqrtf((float)m.dk);
  f.qk = s.qk; f.ld = 2 * m.KD; f.kd = (int)m.KD;
  f.apa = g.adj_pa;
  for (int k = 0; k < m.K; ++k) f.mask[k] = p.mask[k];
  f.bits = g.apa_bits; f.bits_t = g.apa_bits_t;
  f.csc_ptr = g.csc_ptr; f.csc_row = g.csc_row; f.csr_ptr = g.csr_ptr; f.csr_col = g.csr_col; f.csr2csc = g.csr2csc;
  f.apa_ptr = g.apa_ptr; f.apa_row = g.apa_row; f.tsupp = g.tsupp;
  f.lse = s.lse; f.psupp = s.psupp; f.wsupp = s.wsupp;
  if (m.fsmall) {
    f.am = s.am; f.amt = s.amt; f.papa = s.papa; f.apa_nnz = (int)m.apa_nnz; f.apa_idx = g.apa_idx; f.apa2t = g.apa2t;
  }
  return f;
}

// host-side issue timing per stage (DSTAGNN_HOST_PROFILE=1): accumulates and prints
// the mean every 100 calls to stderr
struct HostTimer {
  bool on;
  const char* tag;
  std::chrono::steady_clock::time_point t;
  static std::map<std::string, std::pair<double, long>>& acc() {
    static std::map<std::string, std::pair<double, long>> a;
    return a;
  }
  HostTimer(bool on_, const char* tag_) : on(on_), tag(tag_) {
    if (on) t = std::chrono::steady_clock::now();
  }
  void lap(const char* what) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    auto& e = acc()[std::string(tag) + "." + what];
    e.first += std::chrono::duration<double, std::micro>(now - t).count();
    e.second += 1;
    t = now;
    if (e.second % 100 == 0) fprintf(stderr, "[host] %s.%s %.1f us\n", tag, what, e.first / e.second);
  }
};

// ------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------
struct Fwd {
  const Dims& m;
  const dstagnn_block_dims& d;
  const dstagnn_block_params& p;
  const dstagnn_graph& gr;
  const float* x;
  const float* res;
  float* out;
  float* re_at;
  SaveBufs& s;
  Scratch& w;
  hipStream_t st;
  Streams ks;
  bool e_side = false;           // E = x transposed is issued on the side stream (token e_ready)
  SyncTok e_ready;
  ChebFl fl;
  // forward-only mode (dstagnn_block_forward_only): s and w come from plan_work; the in-place
  // LayerNorm inputs are not rewritten, and the split GTU tail runs in chunks
  bool lean = false;
  // the TAt stage's first product (launch), and beside it the forward's side work: E (e_side)
  // and x Theta (xth non-null) need only x and the re-laid parameters, so the fork's flag rides
  // on that product
  template <class Launch>
  int fork_side(const ChebIO* xth, Launch&& launch) {
    if (!e_side && !xth) return launch(nullptr);
    DS_TRY(ks.fork_on(launch));
    if (e_side) {  // E = x transposed (read by the TAt LayerNorm and saved for the backward)
      DS_TRY(op_transpose(x, s.E, m.N, (int)m.FT, m.B, (int64_t)m.N * m.FT, m.FT * m.N, 0.f, ks.side()));
      DS_TRY(ks.signal(ks.sd, &e_ready));
    }
    if (xth) DS_TRY(cheb_xtheta(*xth, w.gemm_ws_side, ks.side()));
    return 0;
  }

  // the whole stage as one kernel (tat_fused.hip): E read in place from x (inner block) or from
  // the EmbedT LayerNorm's output (first block); no E transpose, no intermediate round trips
  int stage_tat_fused(const ChebIO* xth_side) {
    const int64_t N = m.N;
    TatFusedArgs t;
    if (m.first) {
      t.src = s.E; t.s0 = N; t.s1 = m.FT * N; t.sN = 1;
    } else {
      t.src = x; t.s0 = 1; t.s1 = N * m.FT; t.sN = m.FT;
    }
    t.wqkv = s.Wqkv_p; t.wfc = p.tat_fc;
    t.res = res; t.res_mode = d.res_mode;
    t.g = p.tat_ln_g; t.bta = p.tat_ln_b;
    t.qkv = s.qkv; t.re_at = re_at; t.att = s.att; t.ctx = s.ctx;
    t.u = s.u_tat; t.mu = s.mu_tat; t.rs = s.rs_tat; t.O = s.O;
    t.FT = m.FT; t.BFT = m.BFT; t.BN = m.BN;
    t.F = m.F; t.T = m.T; t.N = m.N; t.NP = m.NP; t.h = m.h;
    t.scale = 1.f / sqrtf((float)m.dk);
    return fork_side(xth_side, [&](ForkSig* sig) { return op_tat_fused_fwd(t, st, sig); });
  }

  int stage_tat(const ChebIO* xth_side) {
    const int64_t N = m.N;
    // E: TAt input (B,F,T,N)
    if (m.first) {
      LnFwd a;
      // rows (b, f, t): x[b, n, f, t] along n, the position row of t shared by the F features
      a.R = (int)m.BFT; a.L = m.N;
      a.src[0].p = x; a.src[0].row = idx2(m.FT, 1, (int64_t)m.N * m.FT); a.src[0].es = m.FT;
      a.src[1].p = p.embT_pos; a.src[1].row = idx2(m.T, m.N, 0); a.src[1].es = 1;
      a.nsrc = 2;
      a.g = p.embT_g; a.b = p.embT_b;
      a.y = s.E; a.yrow = idx1(N); a.yes = 1;
      a.u = s.u_et; a.mu = s.mu_et; a.rs = s.rs_et;
      DS_TRY(op_ln_fwd(a, st));
    } else if (!e_side && !m.tfused) {
      DS_TRY(op_transpose(x, s.E, m.N, (int)m.FT, m.B, N * m.FT, m.FT * N, 0.f, st));
    }
    // Q | K | V projections (MultiHeadAttention :92-94) as ONE GEMM over the stacked weights
    if (m.tfused) return stage_tat_fused(xth_side);
    {
      Gemm g;
      g.M = (int)m.BFT; g.N = (int)m.QW; g.K = m.N;
      if (m.first) {
        g.A = s.E; g.am = idx1(N); g.ak = idx1(1);
      } else {  // straight from x (B,N,F,T): rows (b,(f,t)) contiguous in (f,t) -> 16-B DMA
        g.A = x; g.am = idx2(m.FT, 1, N * m.FT); g.ak = idx1(m.FT);
      }
      g.B = s.Wqkv; g.bk = idx1(1); g.bn = idx1(N);
      g.C = s.qkv; g.cm = idx1(m.QW); g.cn = idx1(1);
      DS_TRY(fork_side(xth_side, [&](ForkSig* sig) { return run_gemm(g, w.gemm_ws, kGemmWs, st, sig); }));
    }
    DS_TRY(op_tat_fwd(m.B, m.F, m.T, m.h, m.dk, m.dv, s.qkv, res, d.res_mode, re_at, s.att, s.ctx, st));
    // fc (:99)
    {
      Gemm g;
      g.M = (int)m.BFT; g.N = m.N; g.K = (int)m.HV;
      g.A = s.ctx; g.am = idx1(m.HV); g.ak = idx1(1);
      g.B = p.tat_fc; g.bk = idx1(1); g.bn = idx1(m.HV);
      g.C = s.u_tat; g.cm = idx1(N); g.cn = idx1(1);
      DS_TRY(run_gemm(g, w.gemm_ws, kGemmWs, st));
    }
    // LN_N(fc + E) (:100)
    if (e_side) DS_TRY(ks.wait(st, e_ready));
    {
      LnFwd a;
      a.R = (int)m.BFT; a.L = m.N;
      a.src[0].p = s.u_tat; a.src[0].row = idx1(N);
      a.src[1].p = s.E; a.src[1].row = idx1(N);
      a.nsrc = 2;
      a.g = p.tat_ln_g; a.b = p.tat_ln_b;
      // O in [(f,t)][(b,n)] order: the pre_conv products read it with single-level unit-stride
      // maps (16-B DMA; no two-level k map in the weight gradient), row r = (b, ft) of the LN
      a.y = s.O; a.yrow = idx2(m.FT, m.BN, N);
      a.u = lean ? nullptr : s.u_tat; a.mu = s.mu_tat; a.rs = s.rs_tat;
      DS_TRY(op_ln_fwd(a, st));
    }
    return 0;
  }

  Gemm preconv_gemm() {
    Gemm g;  // u_s[(b,n), d] = bias[d] + sum_{(f,t)} O[b,f,t,n] Wp[d,(f,t)]
    g.M = (int)m.BN; g.N = m.D; g.K = (int)m.FT;
    g.A = s.O; g.am = idx1(1); g.ak = idx1(m.BN);
    g.B = s.Wp; g.bk = idx1(1); g.bn = idx1(m.FT);
    g.C = s.u_s; g.cm = idx1(m.D); g.cn = idx1(1);
    g.bias = p.pre_conv_b;
    g.hot = 1;
    return g;
  }

  int stage_preconv() { return run_gemm(preconv_gemm(), w.gemm_ws, kGemmWs, st); }

  // every parameter re-layout, as one launch on the caller's stream (a fork / join pair to the
  // side stream costs more host time, ~15 us, than these small copies cost GPU time)
  int stage_params() {
    ParamPrep pp;
    bool full = false;
    PrepSeg spare;  // (a segment past the capacity lands here; the call then fails below)
    auto add = [&](int kind, const float* src, float* dst, int64_t n, int p0 = 0, int p1 = 0, int p2 = 0,
                   int64_t off = 0) -> PrepSeg& {
      if (!dst) return spare;  // a re-layout nothing on this path reads (plan_bufs)
      full = full || pp.nseg >= kPrepSegsHost;
      PrepSeg& g = full ? spare : pp.seg[pp.nseg++];
      g.kind = kind; g.src = src; g.dst = dst; g.n = n; g.p0 = p0; g.p1 = p1; g.p2 = p2; g.dst_off = off;
      return g;
    };
    add(0, p.tat_wq, s.Wqkv, m.HQ * m.N, 0, 0, 0, 0);
    add(0, p.tat_wk, s.Wqkv, m.HQ * m.N, 0, 0, 0, m.HQ * m.N);
    add(0, p.tat_wv, s.Wqkv, m.HV * m.N, 0, 0, 0, 2 * m.HQ * m.N);
    if (m.tfused) {  // the fused TAt kernel's B operand: rows zero-padded to NP (16-B aligned quads)
      add(8, p.tat_wq, s.Wqkv_p, m.HQ * m.NP, m.N, m.NP, 0, 0);
      add(8, p.tat_wk, s.Wqkv_p, m.HQ * m.NP, m.N, m.NP, 0, m.HQ * m.NP);
      add(8, p.tat_wv, s.Wqkv_p, m.HV * m.NP, m.N, m.NP, 0, 2 * m.HQ * m.NP);
    }
    if (m.tfused_bwd) {  // the fused backward's B operands (zero-padded transposes, kind 9)
      add(9, p.tat_fc, s.WfcT, m.HV * m.NP, m.NP, (int)m.HV, m.NP, 0).p3 = m.N;
      add(9, p.tat_wq, s.WqT, m.NP * m.HQ, (int)m.HQ, m.N, (int)m.QW, 0).p3 = (int)m.HQ;
      add(9, p.tat_wk, s.WqT, m.NP * m.HQ, (int)m.HQ, m.N, (int)m.QW, m.HQ).p3 = (int)m.HQ;
      add(9, p.tat_wv, s.WqT, m.NP * m.HV, (int)m.HV, m.N, (int)m.QW, 2 * m.HQ).p3 = (int)m.HV;
    }
    add(0, p.sat_wq, s.Wqk, m.KD * m.D, 0, 0, 0, 0);
    add(0, p.sat_wk, s.Wqk, m.KD * m.D, 0, 0, 0, m.KD * m.D);
    add(1, p.pre_conv_w, s.Wp, (int64_t)m.D * m.FT, m.F, m.T);  // Wp[d][f][t] = W[d][t][0][f]
    for (int k = 0; k < m.K; ++k) add(2, p.theta[k], s.thcat, (int64_t)m.F * m.C, m.C, (int)m.KC, k);
    for (int g = 0; g < 3; ++g) {
      const int64_t n = 2 * (int64_t)m.C * m.C * m.ks[g];
      add(3, p.gtu_w[g], s.Wgt[g], n, m.C, m.ks[g]);  // (o, j, c): the fused forward
      add(7, p.gtu_w[g], s.Wgf[g], n, m.C, m.ks[g]);  // (j, c, o): the unfused forward, the fused backward
      add(4, p.gtu_w[g], s.Wgb[g], n, m.C, m.ks[g]);  // (j', o, c) flipped: the unfused backward
    }
    if (m.fsmall)  // the dense A_pa o M_k of the small-graph attention kernels (:122)
      for (int k = 0; k < m.K; ++k) {
        add(5, p.mask[k], s.am + (int64_t)k * m.NN, m.NN).src2 = gr.adj_pa;
        add(6, p.mask[k], s.amt ? s.amt + (int64_t)k * m.NN : nullptr, m.NN, m.N).src2 = gr.adj_pa;
      }
    if (full) {
      set_last_error("param_prep: more parameter re-layouts than kPrepSegsHost");
      return DSTAGNN_E_ARG;
    }
    DS_TRY(op_param_prep(pp, st));
    return 0;
  }

  int stage_sat() {
    {  // EmbedS LN_D(y + pos) + dropout (:233-234)
      LnFwd a;
      a.R = (int)m.BN; a.L = m.D;
      a.src[0].p = s.u_s; a.src[0].row = idx1(m.D);
      a.src[1].p = p.embS_pos; a.src[1].row = idx2(m.N, m.D, 0);
      a.nsrc = 2;
      a.g = p.embS_g; a.b = p.embS_b;
      a.y = s.Zd; a.yrow = idx1(m.D);
      a.u = lean ? nullptr : s.u_s; a.mu = s.mu_s; a.rs = s.rs_s;
      if (drop_on(d)) {
        a.drop_p = d.drop_p; a.seed = d.seed; a.which = 0; a.drop_off = drop_off(d, 0);
      }
      DS_TRY(op_ln_fwd(a, st));
    }
    {  // SMultiHeadAttention W_Q / W_K (:62-63) as ONE GEMM over the stacked weights
      Gemm g;
      g.M = (int)m.BN; g.N = (int)(2 * m.KD); g.K = m.D;
      g.A = s.Zd; g.am = idx1(m.D); g.ak = idx1(1);
      g.B = s.Wqk; g.bk = idx1(1); g.bn = idx1(m.D);
      g.C = s.qk; g.cm = idx1(2 * m.KD); g.cn = idx1(1);
      DS_TRY(run_gemm(g, w.gemm_ws, kGemmWs, st));
    }
    if (!m.flash) {  // S'[b,k] = Q'_k K'_k^T / sqrt(dk)  (:19) -> written into P (softmaxed in place)
      Gemm g;
      g.M = m.N; g.N = m.N; g.K = m.dk; g.batch = m.B * m.K;
      g.A = s.qk; g.am = idx1(2 * m.KD); g.ak = idx1(1); g.az = idx2(m.K, m.dk, m.N * 2 * m.KD);
      g.B = s.qk; g.b_off = m.KD; g.bk = idx1(1); g.bn = idx1(2 * m.KD); g.bz = idx2(m.K, m.dk, m.N * 2 * m.KD);
      g.C = s.P; g.cm = idx1(m.N); g.cn = idx1(1); g.cz = idx1(m.NN);
      g.alpha = 1.f / sqrtf((float)m.dk);
      DS_TRY(run_gemm(g, w.gemm_ws, kGemmWs, st));
    }
    return 0;
  }

  ChebIO cheb_io() {
    ChebIO c;
    c.B = m.B; c.N = m.N; c.F = m.F; c.T = m.T; c.K = m.K; c.C = m.C;
    c.x = x; c.S = s.P; c.mask = p.mask; c.g = &gr; c.sparse = m.sparse; c.thcat = s.thcat;
    c.P = s.P; c.W = s.W; c.xth = s.xth; c.X = s.X;  // (null with m.dth: agg_k stays in LDS, SAVE = false)
    c.agg = m.agg;
    if (m.flash) {
      fl = make_fl(m, p, gr, s);
      c.fl = &fl;
    }
    return c;
  }
  int stage_cheb() { return cheb_forward(cheb_io(), w.gemm_ws, st); }

  Gemm gtu_conv(int q) {
    // conv[(bn,t), o] = b[o] + sum_{(j,c)} X[bn, t+j, c] W[o,c,j]; with X rows (t,c) the
    // window (j, c) is one contiguous run of ks*C floats (GTU :190 as an implicit-im2col GEMM)
    const int ks = m.ks[q], Tg = m.Tg[q];
    Gemm g;
    g.M = (int)(m.BN * Tg); g.N = 2 * m.C; g.K = m.C * ks;
    g.A = s.X; g.am = idx2(Tg, m.C, m.CT); g.ak = idx1(1);
    g.B = s.Wgf[q]; g.bk = idx1(2 * m.C); g.bn = idx1(1);  // re-laid (j, c, o)
    g.C = s.conv[q]; g.cm = idx1(2 * m.C); g.cn = idx1(1);
    g.bias = p.gtu_b[q];
    return g;
  }

  int stage_tail() {
    if (m.gfused) {  // convolutions + gates + fcmy + residual + LN in one kernel (gtu_fused.hip)
      GtuFusedArgs g;
      g.BN = m.BN; g.C = m.C; g.T = m.T; g.first = m.first;
      g.X = s.X; g.x = x;
      for (int q = 0; q < 3; ++q) { g.wt[q] = s.Wgt[q]; g.bias[q] = p.gtu_b[q]; g.conv[q] = s.conv[q]; }
      g.fcmy_w = p.fcmy_w; g.fcmy_b = p.fcmy_b; g.res_w = p.res_w; g.res_b = p.res_b;
      g.ln_g = p.ln_g; g.ln_b = p.ln_b;
      if (drop_on(d)) { g.drop_p = d.drop_p; g.seed = d.seed; g.drop_off = drop_off(d, 1); }
      // G only for the unfused backward's fcmy weight gradient (the fused one recomputes the gates)
      g.G = s.G;
      g.tco = s.tco; g.r = s.r; g.mu = s.mu_c; g.rs = s.rs_c; g.out = out;
      return op_gtu_fused_fwd(g, st);
    }
    // the three independent convolutions (kernel widths 3, 5, 7) as ONE grouped launch
    const Gemm convs[3] = {gtu_conv(0), gtu_conv(1), gtu_conv(2)};
    DS_TRY(run_gemm_group(convs, 3, w.gemm_ws, kGemmWs, st));
    GtuTailArgs t;  // gates + fcmy + dropout + residual + LN, one workgroup per node
    t.BN = m.BN; t.C = m.C; t.T = m.T; t.first = m.first; t.F = m.first ? m.F : 1;
    for (int q = 0; q < 3; ++q) t.conv[q] = s.conv[q];
    t.fcmy_w = p.fcmy_w; t.fcmy_b = p.fcmy_b;
    t.X = s.X; t.x = x; t.res_w = p.res_w; t.res_b = p.res_b; t.ln_g = p.ln_g; t.ln_b = p.ln_b;
    if (drop_on(d)) { t.drop_p = d.drop_p; t.seed = d.seed; t.drop_off = drop_off(d, 1); }
    t.G = s.G; t.tco = s.tco; t.r = s.r; t.mu = s.mu_c; t.rs = s.rs_c; t.out = out;
    if (lean && gtu_tail_fwd_split(m.C, m.T, m.first ? m.F : 0)) {
      // forward-only, split tail: G in the main GEMM workspace (idle since the convolutions), as
      // many nodes at a time as fit it; the fcmy GEMM's output passes through the out buffer (a
      // workgroup of the tail kernel reads its node's values before it stores that node's
      // output).  A GEMM that does not split K keeps one summation order whatever its row count
      // (gemm.hip plan_gemm), so the chunks change no bit.
      const int64_t per = (int64_t)m.C * m.S, nb = (int64_t)kGemmWs / per;
      if (nb < 1) { set_last_error("gtu_tail: C*(3T-12) exceeds the GEMM workspace"); return DSTAGNN_E_SHAPE; }
      for (int64_t bn0 = 0; bn0 < m.BN; bn0 += nb) {
        GtuTailArgs c = t;
        c.BN = std::min(nb, m.BN - bn0);
        for (int q = 0; q < 3; ++q) c.conv[q] = t.conv[q] + bn0 * m.Tg[q] * 2 * m.C;
        c.X = t.X + bn0 * m.CT;
        c.x = t.x + bn0 * (m.first ? m.FT : m.CT);
        c.drop_off = t.drop_off + (uint64_t)(bn0 * m.CT);
        c.out = out + bn0 * m.CT;
        c.tco = c.out;
        c.G = w.gemm_ws;
        DS_TRY(op_gtu_tail_fwd(c, st));
      }
      return 0;
    }
    return op_gtu_tail_fwd(t, st);
  }

  int run() {
    static const bool prof = env_str("DSTAGNN_HOST_PROFILE") != nullptr;
    HostTimer ht(prof, "fwd");
    ks.init(st);
    const bool split = ks.split();
    DS_TRY(stage_params());
    ht.lap("params");
    ChebIO c = cheb_io();
    // aggregate-first Chebyshev (m.agg) has no x Theta GEMM: the side stream then carries only
    // E = x transposed, which the main chain awaits by its own token (e_ready)
    const bool side_xth = split && !m.agg;  // x Theta needs only x and Theta: it runs beside the whole attention chain
    e_side = split && !m.first && !m.tfused;  // (the fused TAt kernel reads x in place)
    DS_TRY(debug_delay(st, true));
    DS_TRY(stage_tat(side_xth ? &c : nullptr));
    DS_TRY(ks.order_err);
    ht.lap("tat");
    DS_TRY(debug_delay(st, true));
    DS_TRY(stage_preconv());
    ht.lap("preconv");
    DS_TRY(debug_delay(st, true));
    DS_TRY(stage_sat());
    ht.lap("sat");
    if (split) {
      DS_TRY(cheb_softmax(c, st));
      if (side_xth) DS_TRY(ks.join());
      DS_TRY(cheb_aggregate(c, w.gemm_ws, st));
    } else {
      DS_TRY(debug_delay(st, true));
      DS_TRY(stage_cheb());
    }
    ht.lap("cheb");
    DS_TRY(debug_delay(st, true));
    DS_TRY(stage_tail());
    ht.lap("tail");
    return 0;
  }
};

// ------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------
struct Bwd {
  const Dims& m;
  const dstagnn_block_dims& d;
  const dstagnn_block_params& p;
  const dstagnn_graph& gr;
  const dstagnn_block_grads& gd;
  const float* x;
  const float* dout;
  const float* dre;
  float* dx;
  float* dres;
  SaveBufs& s;
  Scratch& w;
  hipStream_t st;
  Streams ks;
  ChebFl fl;
  ChebFl flash_args() {
    ChebFl f = make_fl(m, p, gr, s);
    f.dzs = w.dzs; f.dzs_r = w.dzs_r; f.cc = w.cc; f.dqk = w.dqk;
    for (int k = 0; k < m.K; ++k) f.dmask[k] = gd.mask[k];
    return f;
  }
  int fork() { return ks.fork(); }
  int join() { return ks.join(); }
  // a point on the side stream that the main stream can wait for later (wait_side)
  SyncTok dx_ready;
  int mark_side(SyncTok* t) {
    *t = SyncTok{};
    if (!ks.split()) return 0;
    return ks.signal(ks.sd, t);
  }
  int wait_side(const SyncTok& t) {
    if (!ks.split()) return 0;
    return ks.wait(st, t);
  }

  // EmbedS LayerNorm backward: its dY partial sums (the pre_conv bias gradient) in the (BN, D)
  // gcon_s after the gamma slab, when both fit
  float* preconv_bias_part() const {
    const int64_t pb = ln_bwd_part_blocks(m.BN);
    if (!gd.pre_conv_b || !ln_bwd_partials_ok(m.D) || 2 * pb > m.BN) return nullptr;
    return w.gcon_s + pb * m.D;
  }
  // TAt LayerNorm backward: gamma / beta partial slabs (both fit in the (BFT, N) gcon_a)
  bool tat_part() const { return ln_bwd_partials_ok(m.N) && 2 * ln_bwd_part_blocks(m.BFT) <= m.BFT; }

  int colsum_on(hipStream_t q, const float* in, int64_t A, int O, int I, float* out) {
    if (!out) return 0;
    float* part = q == st ? w.part : w.part_side;
    return op_colsum(in, A, O, I, out, 1, 0.f, part, kPart, q);
  }
  // several same-shape column sums in one launch pair (side stream, or the main stream with
  // on_main: the caller's stream may be the null stream, so no stream-valued sentinel); null
  // outputs skipped
  int colsums(std::initializer_list<std::pair<const float*, float*>> io, int64_t A, int O, int I,
              bool on_main = false) {
    const hipStream_t q = on_main ? st : ks.side();
    const float* ins[4];
    float* outs[4];
    int n = 0;
    for (const auto& q : io)
      if (q.second && n < 4) { ins[n] = q.first; outs[n] = q.second; ++n; }
    if (!n) return 0;
    return op_colsum_multi(ins, outs, n, A, O, I, 1, 0.f, q == st ? w.part : w.part_side, kPart, q);
  }
  int gemm(const Gemm& g, ForkSig* sig = nullptr) { return run_gemm(g, w.gemm_ws, kGemmWs, st, sig); }
  // side-stream weight gradients: their own split-K target — fewer K slices mean a cheaper fold
  // and fewer CUs taken from the main chain.  192: with the GTU stage fused the side stream is
  // the step's last to finish, and 192 beat the global 448 by ~8 us/step (256: ~5) in same-box A/Bs (profiles/r05_knob_sweep.txt)
  static constexpr int kSideSplitK = 192;
  int sgemm(const Gemm& g0) {
    Gemm g = g0;
    if (ks.split() && !g.splitk_target) g.splitk_target = kSideSplitK;
    return run_gemm(g, ks.split() ? w.gemm_ws_side : w.gemm_ws, kGemmWs, ks.side());
  }

  // the GTU stage backward as one kernel (gtu_fused.hip): LN / residual / dropout backward, dG,
  // the gate derivatives (compact (BN Tg, 2C) rows) and the transposed convolutions -> gpre
  int stage_tail_fused() {
    GtuFusedBwdArgs g;
    g.BN = m.BN; g.C = m.C; g.T = m.T; g.first = m.first;
    g.dout = dout; g.r = s.r; g.tco = s.tco; g.mu = s.mu_c; g.rs = s.rs_c; g.x = x; g.X = s.X;
    for (int q = 0; q < 3; ++q) { g.conv[q] = s.conv[q]; g.wf[q] = s.Wgf[q]; g.dconv[q] = w.dconv[q]; }
    g.fcmy_w = p.fcmy_w; g.ln_g = p.ln_g; g.res_w = p.res_w;
    if (drop_on(d)) { g.drop_p = d.drop_p; g.seed = d.seed; g.drop_off = drop_off(d, 1); }
    g.dx = dx; g.gpre = w.gpre;
    // the LN / residual_conv / fcmy parameter gradients summed in-kernel (ticket tree over
    // per-workgroup rows in gcon_t): no column sums on the side stream
    g.gout = gd.ln_g; g.bout = gd.ln_b; g.fwout = gd.fcmy_w; g.fbout = gd.fcmy_b;
    if (m.first) { g.rwout = gd.res_w; g.rbout = gd.res_b; }
    g.part = w.gcon_t;  // (sized max(BN CT, gtu_fused_bwd_part_floats(BN)) by plan_scratch)
    // (a flag written by the kernel's last workgroup instead of this fork measured 20 us/step
    // SLOWER: the side's GTU weight-gradient GEMM then starts under the SDDMM and both stretch)
    // (no fork here, the weight gradients issued behind the SDDMM's kernel-carried flag in
    // stage_cheb instead: 0.544 ms/step with {GTU dW, SpMM^T}, 0.526 with {SpMM^T, GTU dW},
    // against 0.520 with this fork — same box, three interleaved rounds)
    DS_TRY(op_gtu_fused_bwd(g, st));
    DS_TRY(fork());
    return stage_tail_wgrads(true);
  }

  int stage_tail() {
    if (m.gbfused) return stage_tail_fused();
    GtuTailArgs t;  // LN / residual backward -> dtc -> dG = dtc W -> gates backward, per node
    t.BN = m.BN; t.C = m.C; t.T = m.T; t.first = m.first; t.F = m.first ? m.F : 1;
    for (int q = 0; q < 3; ++q) { t.conv[q] = s.conv[q]; t.dconv_pad[q] = w.dconv[q]; }
    t.fcmy_w = p.fcmy_w;
    t.X = s.X; t.x = x; t.res_w = p.res_w; t.res_b = p.res_b; t.ln_g = p.ln_g; t.ln_b = p.ln_b;
    if (drop_on(d)) { t.drop_p = d.drop_p; t.seed = d.seed; t.drop_off = drop_off(d, 1); }
    t.tco = s.tco; t.r = s.r; t.mu = s.mu_c; t.rs = s.rs_c;
    t.dout = dout; t.gcontrib = w.gcon_t; t.dtc = w.dtc; t.dX = w.dX; t.dx = dx;
    t.rcontrib = w.bcon_t; t.dres = w.dres_t; t.dG = w.dGt;
    // per-node [bn][C] partial sums of the LN gamma / beta (and first-block residual_conv)
    // contributions instead of the (B,N,C,T) tensors: the column sums below read BN*C floats
    t.gpart = w.gcon_t; t.bpart = w.gcon_t + m.BN * m.C;
    if (m.first) { t.rpart = w.bcon_t; t.dpart = w.bcon_t + m.BN * m.C * m.F; }
    // the LN gamma / beta (and residual_conv) sums folded in-kernel where the compile-time tail
    // runs (no colsum2d launch on the side stream); level-2 rows after the partials in gcon_t
    const bool tail_fold = gtu_tail_bwd_folds(t);
    if (tail_fold) {
      t.fold = 1;
      t.fold_out[0] = gd.ln_g; t.fold_out[1] = gd.ln_b;
      if (m.first) { t.fold_out[2] = gd.res_w; t.fold_out[3] = gd.res_b; }
      t.fold_ws = w.gcon_t + 2 * m.BN * m.C;
    }
    DS_TRY(op_gtu_tail_bwd(t, st));
    // --- side: LN / residual / fcmy / GTU parameter gradients (one fork; its flag rides on
    // the GTU input-gradient launch)
    DS_TRY(ks.fork_on([&](ForkSig* sig) -> int {
      // gpre = (X > 0) * (dX + sum_q sum_{(j',o)} dconv_pad_q[bn,t+j',o] W_q[o,c,ks-1-j']): the three
      // transposed convolutions as ONE K-concatenated product (K = 2C (3 + 5 + 7)), with the
      // tail's dX as the beta input and the ReLU backward of the Chebyshev output in the epilogue
      Gemm segs[3];
      for (int q = 0; q < 3; ++q) {
        const int ks = m.ks[q];
        const int64_t C2 = 2 * (int64_t)m.C;
        Gemm& g = segs[q];
        g.M = (int)(m.BN * m.T); g.N = m.C; g.K = (int)C2 * ks;
        // row (bn, t) of the padded layout sits at (bn T + t) C2 (node stride T C2): a
        // single-level row map (cheap prologue / epilogue row offsets)
        g.A = w.dconv[q]; g.am = idx1(C2); g.ak = idx1(1);
        g.B = s.Wgb[q]; g.bk = idx1(m.C); g.bn = idx1(1);  // flipped (j', o, c)
        g.C = w.dX; g.cm = idx1(m.C); g.cn = idx1(1);
      }
      segs[0].beta = 1.f;
      segs[0].Cout = w.gpre; segs[0].emask = s.X;  // fused ReLU backward of the cheb output
      if (tconv_on() && gtu_tconv_ok(m.C, m.ks, 3)) {
        // the same product as one sliding-window kernel: each tile stages the union of its
        // rows' windows once (gtu_tconv.hip)
        TconvArgs tc;
        for (int q = 0; q < 3; ++q) { tc.dconv[q] = w.dconv[q]; tc.wflip[q] = s.Wgb[q]; tc.ks[q] = m.ks[q]; }
        tc.dX = w.dX; tc.X = s.X; tc.gpre = w.gpre; tc.M = m.BN * m.T;
        return op_gtu_tconv(tc, st, sig);
      }
      return run_gemm_kcat(segs, 3, st, sig);
    }));
    if (!tail_fold && m.mf) {  // residual_conv.weight (C, F): its own shape, its own column sum
      DS_TRY(colsums({{w.gcon_t, gd.ln_g}, {w.gcon_t + m.BN * m.C, gd.ln_b}, {w.bcon_t + m.BN * m.C * m.F, gd.res_b}},
                     m.BN, m.C, 1));
      DS_TRY(colsums({{w.bcon_t, gd.res_w}}, m.BN, m.C * m.F, 1));
    } else if (!tail_fold)
      DS_TRY(colsums({{w.gcon_t, gd.ln_g}, {w.gcon_t + m.BN * m.C, gd.ln_b}, {w.bcon_t, m.first ? gd.res_w : nullptr},
                      {w.bcon_t + m.BN * m.C, m.first ? gd.res_b : nullptr}}, m.BN, m.C, 1));
    return stage_tail_wgrads(false);
  }
  // side: the fcmy and GTU weight / bias gradients; compact: the gate gradients in (BN Tg, 2C)
  // rows (the fused backward) instead of the zero-padded (BN T + ks - 1, 2C) layout
  int stage_tail_wgrads(bool compact) {
    // the bias gradients ride on their weight-gradient GEMMs as a column-sum column
    // (Gemm::ones_out: sum over the reduction of the gradient operand); a bias whose weight
    // gradient is not requested gets its own column sum
    if (compact) {
      // (the fused backward's partial rows: summed by the caller)
    } else if (gd.fcmy_w) {
      Gemm g;  // dW[t,s] = sum_r dtc[r,t] G[r,s]; db[t] = sum_r dtc[r,t]
      g.M = m.T; g.N = (int)m.S; g.K = (int)(m.BN * m.C);
      g.A = w.dtc; g.am = idx1(1); g.ak = idx1(m.T);
      g.B = s.G; g.bk = idx1(m.S); g.bn = idx1(1);
      g.C = gd.fcmy_w; g.cm = idx1(m.S); g.cn = idx1(1);
      g.ones_out = gd.fcmy_b;
      DS_TRY(sgemm(g));
    } else {
      DS_TRY(colsum_on(ks.side(), w.dtc, m.BN * m.C, m.T, 1, gd.fcmy_b));
    }
    // the fused backward's compact rows with all six gradients wanted: one sliding-window kernel
    // and its fold (gtu_dw.hip) — a gradient the caller does not ask for, the padded
    // rows, T != 12 or C != 32 keep the grouped GEMM below
    bool all6 = compact && m.gbfused && gtu_dw_ok(m.C, m.T);
    for (int q = 0; q < 3; ++q) all6 = all6 && gd.gtu_w[q] && gd.gtu_b[q];
    if (all6) {
      GtuDwArgs g;
      g.BN = m.BN; g.C = m.C; g.T = m.T; g.X = s.X;
      for (int q = 0; q < 3; ++q) { g.dconv[q] = w.dconv[q]; g.dw[q] = gd.gtu_w[q]; g.db[q] = gd.gtu_b[q]; }
      DS_TRY(op_gtu_dw(g, ks.split() ? w.gemm_ws_side : w.gemm_ws, kGemmWs, ks.side()));
    } else {
      Gemm dws[3];
      int nw = 0;
      for (int q = 0; q < 3; ++q) {
        const int kw = m.ks[q], Tg = m.Tg[q];
        const int64_t C2 = 2 * (int64_t)m.C;
        const int64_t cs = C2 * m.T;  // per-(b,n) stride of the padded dconv rows (t', o)
        if (gd.gtu_w[q]) {
          Gemm& g = dws[nw++];  // dW[o,c,j] = sum_{(bn,t')} dconv[bn,t',o] X[bn,t'+j,c]; db[o] = sum dconv[.,o]
          g.M = (int)C2; g.N = m.C * kw; g.K = (int)(m.BN * Tg);
          g.A = w.dconv[q]; g.am = idx1(1);
          if (compact) g.ak = idx1(C2);
          else { g.a_off = (kw - 1) * C2; g.ak = idx2(Tg, C2, cs); }
          g.B = s.X; g.bk = idx2(Tg, m.C, m.CT); g.bn = idx1(1);
          g.C = gd.gtu_w[q]; g.cm = idx1((int64_t)m.C * kw); g.cn = idx2(m.C, kw, 1);
          g.ones_out = gd.gtu_b[q];
        } else {
          DS_TRY(colsum_on(ks.side(), w.dconv[q], compact ? m.BN * Tg : m.BN * m.T + kw - 1, (int)C2, 1, gd.gtu_b[q]));
        }
      }
      if (ks.split())
        for (int q = 0; q < nw; ++q) dws[q].splitk_target = kSideSplitK;
      if (nw) DS_TRY(run_gemm_group(dws, nw, ks.split() ? w.gemm_ws_side : w.gemm_ws, kGemmWs, ks.side()));
    }
    return 0;
  }

  int stage_cheb() {
    // gpre = dX * (X > 0) was written by the last transposed-conv GEMM's epilogue
    const int64_t NN = m.NN, KC = m.KC, T = m.T, CT = m.CT, KCT = m.KCT, FT = m.FT;
    const int B = m.B, N = m.N, K = m.K, C = m.C, F = m.F;
    if (m.agg) {
      // aggregate-first (cheb_agg.hip).  Side stream: dx += the Chebyshev path's gradient
      // (transposed SpMM of g, Theta on the matrix cores) and dTheta_k = agg_k^T g, both from g
      // alone; main: the SDDMM dW = <x_i, Theta_k g_j^T> (flash: dzs and c) for the softmax backward.
      // (One fork after the SDDMM for the side's SpMM, dTheta and mask gradient together
      // measured 0.705 vs 0.703 ms/step, same box: the SpMM then starts later.)
      ChebAg a = make_ag(B, N, K, F, C, m.T, &gr);
      a.x = x; a.thcat = s.thcat; a.P = s.P; a.agg = s.xth; a.g = w.gpre; a.dW = w.dW; a.dx = dx; a.dx_beta = 1.f;
      bool adjacent = gd.theta[0] != nullptr;
      for (int k = 1; k < K && adjacent; ++k) adjacent = gd.theta[k] == gd.theta[0] + (int64_t)k * F * C;
      if (m.flash) {
        a.nnz = (int)m.nnz; a.wsupp = s.wsupp; a.psupp = s.psupp; a.tsupp = gr.tsupp; a.dzs = w.dzs; a.cc = w.cc;
        if (m.fsmall) { a.csc2csr = gr.csc2csr; a.dzs_r = w.dzs_r; }
      }
      DS_TRY(ks.fork_on([&](ForkSig* sig) { return op_cheb_agg_sddmm(a, st, sig); }));
      if (m.dth) {
        // dTheta_k = sum_{b,i} x[b,i] h_k[b,i] inside the transposed SpMM (no agg_k, no GEMM): its
        // fold rows in the side stream's GEMM workspace, idle between the side's GEMMs
        a.dth_ws = ks.split() ? w.gemm_ws_side : w.gemm_ws;
        if (adjacent) { a.dth = gd.theta[0]; a.dth_sk = (int64_t)F * C; a.dth_sf = C; }  // [k][f][c]
        else { a.dth = w.dthcat; a.dth_sk = C; a.dth_sf = KC; }                          // (F, K*C), unpacked below
      }
      DS_TRY(op_cheb_agg_spmm_t(a, ks.side()));
      DS_TRY(mark_side(&dx_ready));
      if (m.dth) {
        if (!adjacent) DS_TRY(unpack_theta(w.dthcat, K, F, C, gd.theta, ks.side()));
      } else {
        Gemm g;  // dTheta[(k,f), c] = sum_{b,j,t} agg[b,j,k,f,t] g[b,j,t,c]
        g.M = K * F; g.N = C; g.K = B * N * m.T;
        g.A = s.xth; g.am = idx1(T); g.ak = idx2(T, 1, (int64_t)K * FT);
        g.B = w.gpre; g.bk = idx1(C); g.bn = idx1(1);
        if (adjacent) {  // [k][f][c]: the parameters' own layout in the flat gradient buffer
          g.C = gd.theta[0]; g.cm = idx1(C); g.cn = idx1(1);
        } else {         // (F, K*C), unpacked below
          g.C = w.dthcat; g.cm = idx2(F, KC, C); g.cn = idx1(1);
        }
        DS_TRY(sgemm(g));
        if (!adjacent) DS_TRY(unpack_theta(w.dthcat, K, F, C, gd.theta, ks.side()));
      }
    } else if (m.sparse) {
      // dW is written on the support only; the softmax backward reads it only where
      // T_k != 0 (no memset)
      ChebSp sp = make_sp(B, N, K, C, m.T, &gr);
      sp.P = s.P; sp.xth = s.xth; sp.g = w.gpre; sp.dW = w.dW; sp.dxth = w.dxth;
      if (m.flash) {  // T o P compact on the support; the SDDMM writes dzs = P o T o dW and c
        sp.nnz = (int)m.nnz; sp.wsupp = s.wsupp; sp.csr2csc = gr.csr2csc;
        sp.psupp = s.psupp; sp.tsupp = gr.tsupp; sp.dzs = w.dzs; sp.cc = w.cc;
        if (m.fsmall) { sp.csc2csr = gr.csc2csr; sp.dzs_r = w.dzs_r; }
      }
      // dxth = W^T g on the side stream (only the Theta / x gradients, also on the side,
      // read it), dW = (x Theta) g^T on the support on the main chain: independent products
      DS_TRY(fork());
      DS_TRY(op_cheb_spmm_t_bwd(sp, ks.side()));
      DS_TRY(op_cheb_sddmm_bwd(sp, st));
    } else {
      {
        Gemm g;  // dW[b,k,i,j] = sum_e xth[b,i,t,k,c] g[b,j,e]
        g.M = N; g.N = N; g.K = (int)CT; g.batch = B * K;
        g.A = s.xth; g.am = idx1(KCT); g.ak = idx2(C, 1, KC); g.az = idx2(K, C, N * KCT);
        g.B = w.gpre; g.bk = idx1(1); g.bn = idx1(CT); g.bz = idx2(K, 0, N * CT);
        g.C = w.dW; g.cm = idx1(N); g.cn = idx1(1); g.cz = idx1(NN);
        DS_TRY(gemm(g));
      }
      {
        Gemm g;  // dxth[b,i,t,k,c] = sum_j W[b,k,i,j] g[b,j,e]
        g.M = N; g.N = (int)CT; g.K = N; g.batch = B * K;
        g.A = s.W; g.am = idx1(N); g.ak = idx1(1); g.az = idx1(NN);
        g.B = w.gpre; g.bk = idx1(CT); g.bn = idx1(1); g.bz = idx2(K, 0, N * CT);
        g.C = w.dxth; g.cm = idx1(KCT); g.cn = idx2(C, 1, KC); g.cz = idx2(K, C, N * KCT);
        DS_TRY(gemm(g));
      }
    }
    // softmax backward: dz = P * (T o dW - colsum(P T o dW)).  Unfused: in place, dense.
    // Fused (flash): only c_j and P dP on the support; dz is recomputed by the dQ'/dK' and
    // mask-gradient kernels
    ChebSm sm;
    sm.B = B; sm.K = K; sm.N = N; sm.apa = gr.adj_pa; sm.cheb = gr.cheb; sm.P = s.P;
    sm.dW = w.dW; sm.dz = w.dW;
    for (int k = 0; k < K; ++k) sm.dmask[k] = gd.mask[k];
    if (m.flash) {
      fl = flash_args();  // c and dzs came with the SDDMM
    } else {
      DS_TRY(op_cheb_softmax_bwd(sm, st));
    }
    // --- side: mask and Theta gradients
    if (m.flash && m.agg) return 0;  // (the mask gradient is forked on stage_sat's dQ'/dK' launch)
    DS_TRY(fork());
    if (m.flash) DS_TRY(op_flash_mask_grad(fl, ks.side()));
    else DS_TRY(op_cheb_mask_grad(sm, ks.side()));
    if (m.agg) return 0;  // Theta and x gradients came with the aggregate-first kernels above
    {
      Gemm g;  // dTheta_cat[f,(k,c)] = sum_{b,i,t} x[b,i,f,t] dxth[b,i,t,k,c]
      g.M = F; g.N = (int)KC; g.K = B * N * m.T;
      g.A = x; g.am = idx1(T); g.ak = idx2(T, 1, FT);
      g.B = w.dxth; g.bk = idx1(KC); g.bn = idx1(1);
      // the K Theta grads adjacent in memory (one flat gradient buffer): write them as
      // [k][f][c] directly, no unpack pass
      bool adjacent = gd.theta[0] != nullptr;
      for (int k = 1; k < K && adjacent; ++k) adjacent = gd.theta[k] == gd.theta[0] + (int64_t)k * F * C;
      if (adjacent) {
        g.C = gd.theta[0]; g.cm = idx1(C); g.cn = idx2(C, 1, (int64_t)F * C);
      } else {
        g.C = w.dthcat; g.cm = idx1(KC); g.cn = idx1(1);
      }
      DS_TRY(sgemm(g));
      if (!adjacent) DS_TRY(unpack_theta(w.dthcat, K, F, C, gd.theta, ks.side()));
    }
    {
      Gemm g;  // dx[b,i,f,t] += sum_{k,c} Theta_k[f,c] dxth[b,i,t,k,c]
      g.M = B * N * m.T; g.N = F; g.K = (int)KC;
      g.A = w.dxth; g.am = idx1(KC); g.ak = idx1(1);
      g.B = s.thcat; g.bk = idx1(1); g.bn = idx1(KC);
      g.C = dx; g.cm = idx2(T, 1, FT); g.cn = idx1(T);
      g.beta = 1.f;
      // on the side stream: dx is an output, only the TAt stage's final accumulation into it
      // (main) has to wait for this (event dx_ready), not the main chain in between
      DS_TRY(sgemm(g));
      DS_TRY(mark_side(&dx_ready));
    }
    return 0;
  }

  int stage_sat() {
    const float sc = 1.f / sqrtf((float)m.dk);
    const int64_t ld = 2 * m.KD;
    // dQ' | dK' with P tiles recomputed, no dense dz
    if (m.flash && m.agg) {  // side: the mask gradient; the fork's flag rides on the dQ'/dK' launch
      DS_TRY(ks.fork_on([&](ForkSig* sig) { return op_flash_dqk(fl, st, sig); }));
      DS_TRY(op_flash_mask_grad(fl, ks.side()));
    } else if (m.flash) {
      DS_TRY(op_flash_dqk(fl, st));
    }
    if (!m.flash) {  // dQ'[b,i,k,:] = sum_j dz[b,k,i,j] K'[b,j,k,:] / sqrt(dk)
      Gemm g;
      g.M = m.N; g.N = m.dk; g.K = m.N; g.batch = m.B * m.K;
      g.A = w.dW; g.am = idx1(m.N); g.ak = idx1(1); g.az = idx1(m.NN);
      g.B = s.qk; g.b_off = m.KD; g.bk = idx1(ld); g.bn = idx1(1); g.bz = idx2(m.K, m.dk, m.N * ld);
      g.C = w.dqk; g.cm = idx1(ld); g.cn = idx1(1); g.cz = idx2(m.K, m.dk, m.N * ld);
      g.alpha = sc;
      DS_TRY(gemm(g));
    }
    if (!m.flash) {  // dK'[b,j,k,:] = sum_i dz[b,k,i,j] Q'[b,i,k,:] / sqrt(dk)
      Gemm g;
      g.M = m.N; g.N = m.dk; g.K = m.N; g.batch = m.B * m.K;
      g.A = w.dW; g.am = idx1(1); g.ak = idx1(m.N); g.az = idx1(m.NN);
      g.B = s.qk; g.bk = idx1(ld); g.bn = idx1(1); g.bz = idx2(m.K, m.dk, m.N * ld);
      g.C = w.dqk; g.c_off = m.KD; g.cm = idx1(ld); g.cn = idx1(1); g.cz = idx2(m.K, m.dk, m.N * ld);
      g.alpha = sc;
      DS_TRY(gemm(g));
    }
    const int64_t ln_rows = ln_bwd_partials_ok(m.D) ? ln_bwd_part_blocks(m.BN) : m.BN;  // partial rows
    {
      Gemm g;  // dZd = dqk [W_Q'; W_K']
      g.M = (int)m.BN; g.N = m.D; g.K = (int)ld;
      g.A = w.dqk; g.am = idx1(ld); g.ak = idx1(1);
      g.B = s.Wqk; g.bk = idx1(m.D); g.bn = idx1(1);
      g.C = w.dZd; g.cm = idx1(m.D); g.cn = idx1(1);
      DS_TRY(gemm(g));
    }
    {  // EmbedS LN_D backward (dropout mask re-derived from the seed)
      LnBwd a;
      a.R = (int)m.BN; a.L = m.D;
      a.dy = w.dZd; a.dyrow = idx1(m.D);
      a.u = s.u_s; a.mu = s.mu_s; a.rs = s.rs_s; a.g = p.embS_g;
      if (drop_on(d)) {
        a.drop_p = d.drop_p; a.seed = d.seed; a.which = 0; a.drop_off = drop_off(d, 0);
      }
      a.dx = w.dY; a.dxrow = idx1(m.D);
      if (ln_bwd_partials_ok(m.D)) {
        a.gpart = w.gcon_s; a.bpart = w.bcon_s;
        a.xpart = preconv_bias_part();  // the pre_conv bias sums ride on this launch
      } else {
        a.gcontrib = w.gcon_s; a.bcontrib = w.bcon_s;
      }
      DS_TRY(op_ln_bwd(a, st));
    }
    // --- side: SAt projection, EmbedS gamma / beta / pos-embedding, pre_conv bias and weight
    // grads; the fork's flag rides on the pre_conv data-gradient GEMM
    DS_TRY(ks.fork_on([&](ForkSig* sig) -> int {
      DS_TRY(debug_delay(st, true));
      return stage_preconv(sig);
    }));
    if (gd.sat_wq || gd.sat_wk) {  // side: [dW_Q'; dW_K'] = dqk^T Zd, then split
      Gemm g;
      g.M = (int)ld; g.N = m.D; g.K = (int)m.BN;
      g.A = w.dqk; g.am = idx1(1); g.ak = idx1(ld);
      g.B = s.Zd; g.bk = idx1(m.D); g.bn = idx1(1);
      // adjacent grads (one flat gradient buffer): the stacked GEMM writes them in place
      const bool adjacent = gd.sat_wq && gd.sat_wk == gd.sat_wq + m.KD * m.D;
      g.C = adjacent ? gd.sat_wq : w.dWqk; g.cm = idx1(m.D); g.cn = idx1(1);
      DS_TRY(sgemm(g));
      if (!adjacent) {
        PackRows pk;
        pk.n = 2; pk.cols = m.D; pk.unpack = 1;
        pk.src[0] = w.dWqk; pk.rows[0] = (int)m.KD; pk.rows[1] = (int)m.KD;
        pk.dst[0] = gd.sat_wq; pk.dst[1] = gd.sat_wk;
        DS_TRY(op_pack_rows(pk, ks.side()));
      }
    }
    // gamma / beta: column sums of the LN backward's partial slabs (or contribution tensors)
    // pre_conv bias = column sum of dY: from the LN backward's per-workgroup dY sums in the same
    // launch as gamma / beta (as a column-sum column of the dW GEMM it would add a whole 64-wide
    // column tile to the 384-wide output: measured slower), else its own column sum
    float* xpart = preconv_bias_part();
    DS_TRY(colsums({{w.gcon_s, gd.embS_g}, {w.bcon_s, gd.embS_b}, {xpart, xpart ? gd.pre_conv_b : nullptr}},
                   ln_rows, m.D, 1));
    if (!xpart) DS_TRY(colsum_on(ks.side(), w.dY, m.BN, m.D, 1, gd.pre_conv_b));
    if (gd.embS_pos) DS_TRY(op_sum_middle(w.dY, 1, m.B, (int64_t)m.N * m.D, gd.embS_pos, 0.f, ks.side()));
    if (gd.pre_conv_w) DS_TRY(sgemm(dwp_gemm()));
    return 0;
  }

  Gemm dwp_gemm() {
    Gemm g;  // dWp[d,(f,t)] = sum_{(b,n)} dY[(b,n),d] O[b,f,t,n]
    g.M = m.D; g.N = (int)m.FT; g.K = (int)m.BN;
    g.A = w.dY; g.am = idx1(1); g.ak = idx1(m.D);
    g.B = s.O; g.bk = idx1(1); g.bn = idx1(m.BN);
    // written straight into pre_conv.weight's [d][t][0][f] layout: n = f*T + t
    g.C = gd.pre_conv_w; g.cm = idx1(m.FT); g.cn = idx2(m.T, m.F, 1);
    return g;
  }

  int stage_preconv(ForkSig* sig) {
    Gemm g;  // dO[b,(f,t),n] = sum_d Wp[d,(f,t)] dY[(b,n),d]
    g.M = (int)m.FT; g.N = (int)m.BN; g.K = m.D;
    g.A = s.Wp; g.am = idx1(1); g.ak = idx1(m.FT);
    g.B = w.dY; g.bk = idx1(1); g.bn = idx1(m.D);
    g.C = w.dO; g.cm = idx1(m.BN); g.cn = idx1(1);  // dO in O's [(f,t)][(b,n)] order
    return gemm(g, sig);
  }

  // the whole TAt backward as one kernel (tat_fused.hip): LN_N backward, dctx, attention
  // backward, dE accumulated into dx (inner block) or written for the EmbedT backward (first)
  int stage_tat_fused() {
    const int64_t N = m.N;
    if (!m.first) DS_TRY(wait_side(dx_ready));  // dx += the Chebyshev-path gradient (side stream) first
    TatFusedBwdArgs t;
    t.dO = w.dO; t.u = s.u_tat; t.mu = s.mu_tat; t.rs = s.rs_tat; t.g = p.tat_ln_g;
    // gamma / beta: the kernel's two-level ticket tree sums its partial rows (level-2 rows after
    // them in the same slabs)
    t.gpart = w.gcon_a; t.bpart = w.gcon_a + tat_bslab() * N;
#ifdef DSTAGNN_RACEBUG_NOFORK
    t.ln_fold = 0;  // (the racy build's side-stream column sums must be the only writer)
#else
    t.ln_fold = 1;
#endif
    t.gout = gd.tat_ln_g; t.bout = gd.tat_ln_b;
    t.dU = w.dU; t.wfcT = s.WfcT;
    t.qkv = s.qkv; t.att = s.att; t.dre = dre; t.dqkv = w.dqkv;
    t.res_mode = d.res_mode;
    t.dres = dres;  // FULL: dS itself; BCAST: its sum over f (folded in the kernel)
    t.dpart = w.dscore;
    t.wqT = s.WqT;
    if (m.first) {
      t.dE = w.dE;
    } else {
      t.dx = dx; t.dxb = N * m.FT;
    }
    t.FT = m.FT; t.BFT = m.BFT; t.BN = m.BN;
    t.F = m.F; t.T = m.T; t.N = m.N; t.NP = m.NP; t.h = m.h;
    t.scale = 1.f / sqrtf((float)m.dk);
    DS_TRY(op_tat_fused_bwd(t, st));
    return m.first ? embedT_backward() : 0;
  }

  // first block: the EmbedT LayerNorm backward of dE, its parameter sums, dx += (dE)^T
  int embedT_backward() {
    const int64_t N = m.N;
    LnBwd a;
    a.R = (int)m.BFT; a.L = m.N;  // rows (b, f, t)
    a.dy = w.dE; a.dyrow = idx1(N);
    a.u = s.u_et; a.mu = s.mu_et; a.rs = s.rs_et; a.g = p.embT_g;
    a.dx = w.du_et; a.dxrow = idx1(N);
    const int64_t pb = ln_bwd_part_blocks(m.BFT);
    const bool part = ln_bwd_partials_ok(m.N) && 2 * pb <= m.BFT;
    if (part) { a.gpart = w.gcon_e; a.bpart = w.gcon_e + pb * N; }
    else a.gcontrib = w.gcon_e;
    DS_TRY(op_ln_bwd(a, st));
    DS_TRY(fork());
    if (part) DS_TRY(colsums({{w.gcon_e, gd.embT_g}, {w.gcon_e + pb * N, gd.embT_b}}, pb, m.N, 1));
    else DS_TRY(colsums({{w.gcon_e, gd.embT_g}, {w.dE, gd.embT_b}}, m.BFT, m.N, 1));
    // the position gradient: summed over b and f (one row per t serves the F features)
    if (gd.embT_pos) DS_TRY(op_sum_middle(w.du_et, 1, m.B * m.F, (int64_t)m.T * m.N, gd.embT_pos, 0.f, ks.side()));
    DS_TRY(wait_side(dx_ready));  // dx += the Chebyshev-path gradient (side stream) first
    return op_transpose(w.du_et, dx, (int)m.FT, m.N, m.B, m.FT * m.N, (int64_t)m.N * m.FT, 1.f, st);
  }

  int stage_tat() {
    const int64_t N = m.N;
    if (m.tfused_bwd) return stage_tat_fused();
    {  // LN_N backward (:100); dU = d(fc + E)
      LnBwd a;
      a.R = (int)m.BFT; a.L = m.N;
      a.dy = w.dO; a.dyrow = idx2(m.FT, m.BN, N);
      a.u = s.u_tat; a.mu = s.mu_tat; a.rs = s.rs_tat; a.g = p.tat_ln_g;
      a.dx = w.dU; a.dxrow = idx1(N);
      if (tat_part()) {  // both slabs in gcon_a ((BFT, N) holds 2 slabs)
        a.gpart = w.gcon_a; a.bpart = w.gcon_a + ln_bwd_part_blocks(m.BFT) * N;
      } else {
        a.gcontrib = w.gcon_a;
      }
      DS_TRY(op_ln_bwd(a, st));
    }
    {  // dctx = dU Wfc
      Gemm g;
      g.M = (int)m.BFT; g.N = (int)m.HV; g.K = m.N;
      g.A = w.dU; g.am = idx1(N); g.ak = idx1(1);
      g.B = p.tat_fc; g.bk = idx1(m.HV); g.bn = idx1(1);
      g.C = w.dctx; g.cm = idx1(m.HV); g.cn = idx1(1);
      DS_TRY(gemm(g));
    }
    // d res_att: dS itself (full res_att), or its sum over f (broadcast res_att, folded in the
    // TAt backward's launch); w.dscore is the scratch either way
    float* dsc = (d.res_mode == DSTAGNN_RES_FULL && dres) ? dres : w.dscore;
    float* dsum = (d.res_mode == DSTAGNN_RES_BCAST && dres) ? dres : nullptr;
    DS_TRY(op_tat_bwd(m.B, m.F, m.T, m.h, m.dk, m.dv, s.qkv, s.att, w.dctx, dre, w.dqkv, dsc, dsum, st));
    {  // dE = dU + dqkv [Wq; Wk; Wv]
      Gemm g;
      g.M = (int)m.BFT; g.N = m.N; g.K = (int)m.QW;
      g.A = w.dqkv; g.am = idx1(m.QW); g.ak = idx1(1);
      g.B = s.Wqkv; g.bk = idx1(N); g.bn = idx1(1);
      // dU is only read (the fc weight grad at the step's end also reads it): beta input C = dU
      g.C = w.dU; g.cm = idx1(N); g.cn = idx1(1);
      g.beta = 1.f;
      g.Cout = w.dE;  // first block: -> the EmbedT LayerNorm backward; inner: transposed into dx
      DS_TRY(gemm(g));
    }
    // dE -> dx
    if (m.first) {
      DS_TRY(embedT_backward());
    } else {
      DS_TRY(wait_side(dx_ready));  // dx += the Chebyshev-path gradient (side stream) first
      DS_TRY(op_transpose(w.dE, dx, (int)m.FT, m.N, m.B, m.FT * N, N * m.FT, 1.f, st));
    }
    return 0;
  }

  // DSTAGNN_GTU_TCONV=0: the GTU input gradient as the K-concatenated GEMM (run_gemm_kcat)
  // instead of the sliding-window kernel (A/B)
  static bool tconv_on() {
    static const bool on = env_flag("DSTAGNN_GTU_TCONV", true);
    return on;
  }

  // [dWq; dWk; dWv] = dqkv^T E — the last product of the backward, issued on the main
  // stream after dx: the side stream is still busy with the earlier parameter gradients
  // (pre_conv, SAt), while the main chain has nothing left (measured: the side stream's tail
  // was the step's critical path); see tat_wqkv_grad.  The TAt fc weight gradient rides with it
  // as one grouped launch: with the main chain's fork flags kernel-written the side stream's
  // tail set the step (two-stream timeline: main ended ~48 us before the side).  The TAt
  // LayerNorm gamma / beta column sums are likewise on the main stream at the end, so the TAt
  // stage forks nothing (no side-stream wait at the step's end)

  // fused TAt backward: the beta slab's first row (gamma: level-1 rows, then the ticket tree's level-2 rows)
  int64_t tat_bslab() const { return tat_fused_bwd_part_rows(m.BFT); }  // the gamma slab's rows (tat_fused.hip)
  int tat_ln_colsums(bool on_main) {
    if (m.tfused_bwd)  // one gamma / beta partial row per fused-kernel workgroup
      return colsums({{w.gcon_a, gd.tat_ln_g}, {w.gcon_a + tat_bslab() * m.N, gd.tat_ln_b}}, m.tf_wg, m.N, 1, on_main);
    if (tat_part()) {
      const int64_t pb = ln_bwd_part_blocks(m.BFT);
      return colsums({{w.gcon_a, gd.tat_ln_g}, {w.gcon_a + pb * m.N, gd.tat_ln_b}}, pb, m.N, 1, on_main);
    }
    return colsums({{w.gcon_a, gd.tat_ln_g}, {w.dO, gd.tat_ln_b}}, m.BFT, m.N, 1, on_main);
  }
  Gemm fc_grad_gemm() {  // dWfc[n,c] = sum_r dU[r,n] ctx[r,c]
    Gemm g;
    g.M = m.N; g.N = (int)m.HV; g.K = (int)m.BFT;
    g.A = w.dU; g.am = idx1(1); g.ak = idx1(m.N);
    g.B = s.ctx; g.bk = idx1(m.HV); g.bn = idx1(1);
    g.C = gd.tat_fc; g.cm = idx1(m.HV); g.cn = idx1(1);
    return g;
  }
  int tat_wqkv_grad() {
    const bool fc_here = gd.tat_fc != nullptr;
    if (!(gd.tat_wq || gd.tat_wk || gd.tat_wv)) return fc_here ? gemm(fc_grad_gemm()) : 0;
    const int64_t N = m.N;
    Gemm g;
    g.M = (int)m.QW; g.N = m.N; g.K = (int)m.BFT;
    g.A = w.dqkv; g.am = idx1(1); g.ak = idx1(m.QW);
    if (m.tfused && !m.first) {  // E = x transposed was never written: E[(b,ft), n] = x[b, n, ft]
      g.B = x; g.bk = idx2(m.FT, 1, N * m.FT); g.bn = idx1(m.FT);
    } else {
      g.B = s.E; g.bk = idx1(N); g.bn = idx1(1);
    }
    const bool adjacent = gd.tat_wq && gd.tat_wk == gd.tat_wq + m.HQ * N && gd.tat_wv == gd.tat_wk + m.HQ * N;
    g.C = adjacent ? gd.tat_wq : w.dWqkv; g.cm = idx1(N); g.cn = idx1(1);
    if (fc_here) {
      const Gemm gs[2] = {g, fc_grad_gemm()};
      DS_TRY(run_gemm_group(gs, 2, w.gemm_ws, kGemmWs, st));
    } else {
      DS_TRY(gemm(g));
    }
    if (!adjacent) {
      PackRows pk;
      pk.n = 3; pk.cols = m.N; pk.unpack = 1;
      pk.src[0] = w.dWqkv; pk.rows[0] = (int)m.HQ; pk.rows[1] = (int)m.HQ; pk.rows[2] = (int)m.HV;
      pk.dst[0] = gd.tat_wq; pk.dst[1] = gd.tat_wk; pk.dst[2] = gd.tat_wv;
      DS_TRY(op_pack_rows(pk, st));
    }
    return 0;
  }

  int run() {
    static const bool prof = env_str("DSTAGNN_HOST_PROFILE") != nullptr;
    HostTimer ht(prof, "bwd");
    ks.init(st);
    ht.lap("init");
    DS_TRY(debug_delay(st, true));
    DS_TRY(stage_tail());
    DS_TRY(ks.order_err);
    ht.lap("tail");
    DS_TRY(debug_delay(st, true));
    DS_TRY(stage_cheb());
    DS_TRY(ks.order_err);
    ht.lap("cheb");
    DS_TRY(debug_delay(st, true));
    DS_TRY(stage_sat());  // + stage_preconv
    DS_TRY(ks.order_err);
    ht.lap("sat");
    DS_TRY(debug_delay(st, true));
    DS_TRY(stage_tat());
    DS_TRY(ks.order_err);
    ht.lap("tat");
    DS_TRY(tat_wqkv_grad());  // (+ the fc weight gradient)
#ifdef DSTAGNN_RACEBUG_NOFORK
    // deliberately racy build (make racebug -> abtest/racebug; tests/test_gpu_knobs.py::
    // test_race_probe_catches_a_missing_fork): the TAt LayerNorm column sums on the side stream
    // WITHOUT a fork after the LayerNorm backward that writes their partials
    DS_TRY(tat_ln_colsums(false));
#else
    if (!m.tfused_bwd) DS_TRY(tat_ln_colsums(true));  // (fused: summed in-kernel)
#endif
    DS_TRY(ks.order_err);
    DS_TRY(join());
    ht.lap("join");
    return 0;
  }
};

int check_space(const Dims& m, size_t save_bytes, size_t scratch_bytes) {
  size_t sv, sc;
  plan_sizes(m, &sv, &sc);
  if (save_bytes < sv || scratch_bytes < sc) {
    set_last_error("save/scratch smaller than dstagnn_block_sizes()");
    return DSTAGNN_E_SPACE;
  }
  return 0;
}

int check_graph(const Dims& m, const dstagnn_graph* g) {
  if (!g->cheb || !g->adj_pa) { set_last_error("graph: null cheb / adj_pa"); return DSTAGNN_E_ARG; }
  if (m.sparse && (g->nnz <= 0 || !g->csc_ptr || !g->csc_row || !g->csr_ptr || !g->csr_col)) {
    set_last_error("cheb_sparse set but the graph carries no CSC/CSR support");
    return DSTAGNN_E_ARG;
  }
  if (m.flash && (g->nnz != m.nnz || !g->csr2csc || !g->apa_bits || !g->apa_bits_t || !g->apa_ptr || !g->apa_row ||
                  !g->tsupp)) {
    set_last_error("cheb_flash set but the graph lacks the flash data (or its nnz differs from cheb_nnz)");
    return DSTAGNN_E_ARG;
  }
  if (m.fsmall && (!g->csc2csr || !g->apa_idx || !g->apa2t || g->apa_nnz != m.apa_nnz)) {
    set_last_error("cheb_flash on a small graph needs csc2csr / apa_idx / apa2t (and apa_nnz == cheb_apa_nnz)");
    return DSTAGNN_E_ARG;
  }
  return 0;
}

void* align256(void* p) { return (void*)(((uintptr_t)p + 255) & ~uintptr_t(255)); }

}  // namespace

// ==================================================================================
// C-ABI
// ==================================================================================
extern "C" {

const char* dstagnn_last_error(void) { return g_last_error.c_str(); }
int dstagnn_prof_start(int capacity) { return gemm_prof_start(capacity); }
int dstagnn_set_splitk_target(int target) { return gemm_set_splitk_target(target); }
int dstagnn_set_gemm_bf16(int on) { return gemm_set_bf16(on); }
int dstagnn_prof_stop(dstagnn_prof_stats* stats) { return gemm_prof_stop(stats); }
int dstagnn_prof_records(dstagnn_prof_record* out, int cap) { return gemm_prof_records(out, cap < 0 ? 0 : cap); }
int dstagnn_version(void) { return 1; }

int dstagnn_block_sizes(const dstagnn_block_dims* d, size_t* save_bytes, size_t* scratch_bytes) {
  DS_TRY(check_dims(d));
  if (!save_bytes || !scratch_bytes) return DSTAGNN_E_ARG;
  plan_sizes(mkdims(*d), save_bytes, scratch_bytes);
  return 0;
}

int dstagnn_block_save_offset(const dstagnn_block_dims* d, int which, size_t* offset_bytes, size_t* count) {
  DS_TRY(check_dims(d));
  if (!offset_bytes || !count || which < 0 || which > 2) return DSTAGNN_E_ARG;
  const Dims m = mkdims(*d);
  Arena a((void*)(uintptr_t)256);  // the forward carves the 256-aligned save buffer the same way
  SaveBufs s = plan_bufs(m, a, true);
  const float* t = which == 0 ? s.X : (which == 1 ? s.tco : s.r);
  *offset_bytes = (size_t)((const char*)t - (char*)(uintptr_t)256);
  *count = (size_t)(m.BN * m.CT);
  return 0;
}

int dstagnn_block_paths(const dstagnn_block_dims* d, uint32_t* bits) {
  DS_TRY(check_dims(d));
  if (!bits) return DSTAGNN_E_ARG;
  const Dims m = mkdims(*d);
  *bits = (m.sparse ? DSTAGNN_PATH_SPARSE : 0u) | (m.flash ? DSTAGNN_PATH_FLASH : 0u) |
          (m.fsmall ? DSTAGNN_PATH_FLASH_SMALL : 0u) | (m.agg ? DSTAGNN_PATH_CHEB_AGG : 0u) |
          (m.tfused ? DSTAGNN_PATH_TAT_FUSED_FWD : 0u) | (m.tfused_bwd ? DSTAGNN_PATH_TAT_FUSED_BWD : 0u) |
          (m.gfused ? DSTAGNN_PATH_GTU_FUSED_FWD : 0u) | (m.gbfused ? DSTAGNN_PATH_GTU_FUSED_BWD : 0u) |
          (m.mf ? DSTAGNN_PATH_FIRST_MULTI : 0u);
  return 0;
}

int dstagnn_block_forward(const dstagnn_block_dims* d, const dstagnn_block_params* p, const dstagnn_graph* g,
                          const float* x, const float* res_att, float* out, float* re_at, void* save,
                          size_t save_bytes, void* scratch, size_t scratch_bytes, dstagnn_stream_t stream) {
  DS_TRY(check_dims(d));
  if (!p || !g || !x || !out || !re_at || !save || !scratch) { set_last_error("null argument"); return DSTAGNN_E_ARG; }
  if (d->res_mode != DSTAGNN_RES_NONE && !res_att) { set_last_error("res_att missing"); return DSTAGNN_E_ARG; }
  Dims m = mkdims(*d);
  DS_TRY(check_space(m, save_bytes, scratch_bytes));
  DS_TRY(check_graph(m, g));
  Arena a(align256(save)), b(align256(scratch));
  SaveBufs s = plan_bufs(m, a, true);
  Scratch w = plan_scratch(m, b);
  Fwd f{m, *d, *p, *g, x, d->res_mode ? res_att : nullptr, out, re_at, s, w, (hipStream_t)stream};
  return f.run();
}

int dstagnn_block_forward_only_size(const dstagnn_block_dims* d, size_t* work_bytes) {
  DS_TRY(check_dims(d));
  if (!work_bytes) return DSTAGNN_E_ARG;
  *work_bytes = plan_work_size(mkdims(*d));
  return 0;
}

int dstagnn_block_forward_only(const dstagnn_block_dims* d, const dstagnn_block_params* p, const dstagnn_graph* g,
                               const float* x, const float* res_att, float* out, float* re_at, void* work,
                               size_t work_bytes, dstagnn_stream_t stream) {
  DS_TRY(check_dims(d));
  if (!p || !g || !x || !out || !re_at || !work) { set_last_error("null argument"); return DSTAGNN_E_ARG; }
  if (d->res_mode != DSTAGNN_RES_NONE && !res_att) { set_last_error("res_att missing"); return DSTAGNN_E_ARG; }
  Dims m = mkdims(*d);
  if (work_bytes < plan_work_size(m)) {
    set_last_error("work smaller than dstagnn_block_forward_only_size()");
    return DSTAGNN_E_SPACE;
  }
  DS_TRY(check_graph(m, g));
  Arena a(align256(work));
  WorkBufs k = plan_work(m, a);
  Fwd f{m, *d, *p, *g, x, d->res_mode ? res_att : nullptr, out, re_at, k.s, k.w, (hipStream_t)stream};
  f.lean = true;
  return f.run();
}

int dstagnn_block_backward(const dstagnn_block_dims* d, const dstagnn_block_params* p, const dstagnn_graph* g,
                           const float* x, const float* res_att, const float* d_out, const float* d_re_at, float* d_x,
                           float* d_res_att, const dstagnn_block_grads* grads, void* save, size_t save_bytes,
                           void* scratch, size_t scratch_bytes, dstagnn_stream_t stream) {
  (void)res_att;
  DS_TRY(check_dims(d));
  if (!p || !g || !x || !d_out || !d_x || !grads || !save || !scratch) {
    set_last_error("null argument");
    return DSTAGNN_E_ARG;
  }
  Dims m = mkdims(*d);
  DS_TRY(check_space(m, save_bytes, scratch_bytes));
  DS_TRY(check_graph(m, g));
  Arena a(align256(save)), b(align256(scratch));
  SaveBufs s = plan_bufs(m, a, true);
  Scratch w = plan_scratch(m, b);
  Bwd bw{m, *d, *p, *g, *grads, x, d_out, d_re_at, d_x, d->res_mode ? d_res_att : nullptr, s, w, (hipStream_t)stream};
  return bw.run();
}

int dstagnn_cheb_sat_forward(int B, int N, int F, int T, int K, int C, int sparse, const float* x, const float* sat,
                             const float* theta_cat, const float* mask_cat, const dstagnn_graph* g, float* out,
                             float* P, float* W, float* xth, void* scratch, size_t scratch_bytes,
                             dstagnn_stream_t stream) {
  if (K > DSTAGNN_MAX_K || K <= 0 || !g) return DSTAGNN_E_SHAPE;
  const int64_t nbig = (int64_t)B * N * C * T;
  if (scratch_bytes < (kGemmWs + nbig) * sizeof(float) + 2 * 256) {
    set_last_error("scratch too small");
    return DSTAGNN_E_SPACE;
  }
  if (sparse && (!cheb_sparse_ok(C * T) || g->nnz <= 0)) { set_last_error("sparse path unavailable"); return DSTAGNN_E_ARG; }
  Arena a(align256(scratch));
  float* ws = a.take(kGemmWs);
  float* Xtc = a.take(nbig);  // the block's internal (B,N,T,C) image
  const float* masks[DSTAGNN_MAX_K];
  for (int k = 0; k < K; ++k) masks[k] = mask_cat + (int64_t)k * N * N;
  ChebIO c;
  c.B = B; c.N = N; c.F = F; c.T = T; c.K = K; c.C = C;
  c.x = x; c.S = sat; c.mask = masks; c.g = g; c.sparse = sparse != 0; c.thcat = theta_cat;
  c.P = P; c.W = W; c.xth = xth; c.X = Xtc;
  hipStream_t st = (hipStream_t)stream;
  DS_TRY(cheb_forward(c, ws, st));
  return op_transpose(Xtc, out, T, C, B * N, (int64_t)C * T, (int64_t)C * T, 0.f, st);
}

int dstagnn_cheb_sat_backward(int B, int N, int F, int T, int K, int C, int sparse, const float* x,
                              const float* theta_cat, const dstagnn_graph* g, const float* out, const float* P,
                              const float* W, const float* xth, const float* d_out, float* d_x, float* d_sat,
                              float* d_theta_cat, float* d_mask_cat, void* scratch, size_t scratch_bytes,
                              dstagnn_stream_t stream) {
  if (K > DSTAGNN_MAX_K || K <= 0 || !g) return DSTAGNN_E_SHAPE;
  if (sparse && (!cheb_sparse_ok(C * T) || g->nnz <= 0)) { set_last_error("sparse path unavailable"); return DSTAGNN_E_ARG; }
  const int64_t nbig = (int64_t)B * N * C * T;
  const int64_t nxth = (int64_t)B * N * K * C * T;
  size_t need = (kGemmWs + 2 * nbig + nxth) * sizeof(float) + 4 * 256;
  if (scratch_bytes < need) { set_last_error("scratch too small"); return DSTAGNN_E_SPACE; }
  Arena a(align256(scratch));
  float* ws = a.take(kGemmWs);
  float* gct = a.take(nbig);
  float* gpre = a.take(nbig);
  float* dxth = a.take(nxth);
  hipStream_t st = (hipStream_t)stream;
  DS_TRY(op_relu_mask(d_out, out, gct, nbig, st));
  DS_TRY(op_transpose(gct, gpre, C, T, B * N, (int64_t)C * T, (int64_t)C * T, 0.f, st));  // -> (B,N,T,C)
  float* dmask[DSTAGNN_MAX_K];
  for (int k = 0; k < K; ++k) dmask[k] = d_mask_cat + (int64_t)k * N * N;
  ChebGradIO c;
  c.B = B; c.N = N; c.F = F; c.T = T; c.K = K; c.C = C;
  c.x = x; c.thcat = theta_cat; c.g = g; c.sparse = sparse != 0; c.P = P; c.W = W; c.xth = xth;
  c.gpre = gpre; c.dx = d_x; c.dx_beta = 0.f; c.dz = d_sat; c.dthcat = d_theta_cat; c.dmask = dmask; c.dxth = dxth;
  return cheb_backward(c, ws, st);
}

int dstagnn_gemm_f32(const dstagnn_gemm_desc* d, void* scratch, size_t scratch_bytes, dstagnn_stream_t stream) {
  if (!d) return DSTAGNN_E_ARG;
  Gemm g;
  g.M = d->M; g.N = d->N; g.K = d->K; g.batch = d->batch > 0 ? d->batch : 1;
  g.A = d->A; g.am = make_idx(d->a_m); g.ak = make_idx(d->a_k); g.az = make_idx(d->a_z); g.a_off = d->a_off;
  g.B = d->B; g.bk = make_idx(d->b_k); g.bn = make_idx(d->b_n); g.bz = make_idx(d->b_z); g.b_off = d->b_off;
  g.C = d->C; g.cm = make_idx(d->c_m); g.cn = make_idx(d->c_n); g.cz = make_idx(d->c_z); g.c_off = d->c_off;
  g.alpha = d->alpha; g.beta = d->beta; g.bias = d->bias; g.bias_stride = d->bias_stride; g.relu = d->relu;
  float* ws = scratch ? (float*)align256(scratch) : nullptr;
  size_t wsf = scratch ? (scratch_bytes > 256 ? (scratch_bytes - 256) / sizeof(float) : 0) : 0;
  return run_gemm(g, ws, wsf, (hipStream_t)stream);
}

int dstagnn_colsum(const float* in, int64_t A, int O, int I, float* out, int64_t ostride, float beta, void* scratch,
                   size_t scratch_bytes, dstagnn_stream_t stream) {
  if (A < 0 || O < 0 || I <= 0) return DSTAGNN_E_ARG;
  if (A == 0 || O == 0) return 0;  // empty: out untouched (include/dstagnn.h)
  if (!in || !out || !scratch) return DSTAGNN_E_ARG;
  size_t pf = scratch_bytes > 256 ? (scratch_bytes - 256) / sizeof(float) : 0;
  return op_colsum(in, A, O, I, out, ostride, beta, (float*)align256(scratch), pf, (hipStream_t)stream);
}

int dstagnn_dropout_mask(const dstagnn_block_dims* d, int which, float* mask, dstagnn_stream_t stream) {
  if (!d || !mask) return DSTAGNN_E_ARG;
  if (which != 0 && which != 1) return DSTAGNN_E_ARG;
  int64_t n = which == 0 ? (int64_t)d->B * d->N * d->d_model : (int64_t)d->B * d->N * d->C * d->T;
  return op_dropout_mask(mask, n, d->seed, (uint32_t)which, d->drop_p, drop_off(*d, which), (hipStream_t)stream);
}

int dstagnn_block_time_stage(const dstagnn_block_dims* d, const dstagnn_block_params* p, const dstagnn_graph* g,
                             const float* x, const float* res_att, float* out, float* re_at, void* save,
                             size_t save_bytes, void* scratch, size_t scratch_bytes, int stage, int iters,
                             float* ms_per_launch, dstagnn_stream_t stream) {
  DS_TRY(check_dims(d));
  if (!ms_per_launch || iters <= 0) return DSTAGNN_E_ARG;
  Dims m = mkdims(*d);
  DS_TRY(check_space(m, save_bytes, scratch_bytes));
  Arena a(align256(save)), b(align256(scratch));
  SaveBufs s = plan_bufs(m, a, true);
  Scratch w = plan_scratch(m, b);
  hipStream_t st = (hipStream_t)stream;
  Fwd f{m, *d, *p, *g, x, d->res_mode ? res_att : nullptr, out, re_at, s, w, st};
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  int rc = 0;
  (void)hipEventRecord(e0, st);
  for (int i = 0; i < iters && rc == 0; ++i) {
    switch (stage) {
      case 0: rc = f.run(); break;
      case 2: rc = f.stage_cheb(); break;
      case 3: rc = f.stage_preconv(); break;
      case 10: rc = run_gemm(f.preconv_gemm(), w.gemm_ws, kGemmWs, st); break;  // the hot GEMM alone
      default: rc = DSTAGNN_E_ARG;
    }
  }
  (void)hipEventRecord(e1, st);
  (void)hipEventSynchronize(e1);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  *ms_per_launch = ms / iters;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return rc;
}

}  // extern "C"
