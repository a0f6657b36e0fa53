// tat.hip — the unfused temporal-attention core per (b, f, head) problem (gfx950, wave64): T x T
// scores, softmax over the QUERY axis (model/DSTAGNN_my.py:37-41), context, and the backward.
// (The whole stage as one kernel per direction is tat_fused.hip.)  Three kernel families, chosen
// per direction by tat_fwd_path / tat_bwd_path:
//   tat_{fwd,bwd}_mfma_kernel<T>   T in {4, 8, 12, 16}, d_k = d_v = 32: the matrix-core core of
//                                  tat_core.hpp, operands from global memory, one wave per problem
//   tat_{fwd,bwd}_valu_kernel<G>   G threads per problem, 256 / G problems per workgroup: G = 64
//                                  for T <= 16, G = 256 while a problem's tiles fit 64 KB of LDS
//   tat_{fwd,bwd}_cols_kernel      longer series: a workgroup per 16-column chunk, then one GEMM
#include <initializer_list>

#include "common.hpp"
#include "handoff.hpp"
#include "ops.hpp"
#include "tat_core.hpp"

namespace {

struct TatArgs {
  int B, F, T, h, dk, dv;
  const float* qkv;      // (B*F*T, 2*h*dk + h*dv): [Q | K | V]
  const float* res;      // res_att or null
  int res_mode;
  float scale;
  float* re_at;          // (B,F,h,T,T) scores
  float* att;            // (B,F,h,T,T) softmax (saved)
  float* ctx;            // (B*F*T, h*dv)
  // bwd
  const float* dctx;     // (B*F*T, h*dv)
  const float* dre;      // (B,F,h,T,T) or null
  float* dqkv;           // (B*F*T, 3 cols blocks)
  float* dscore;         // (B,F,h,T,T) dS (== d res_att before f-reduction); scratch when !keep_ds
  // matrix-core backward only: dres_sum = sum_f dS ((B,1,h,T,T), the broadcast res_att's
  // gradient) folded in-kernel by tickets cnt[b*h + hd] over partials in dscore
  float* dres_sum;
  int* cnt;
  int keep_ds;           // write the full dS to dscore
};

constexpr int kTatW = 4;  // waves per workgroup (one problem each in the matrix-core and G = 64 kernels)

// the T x T residual tile of problem (b, f, hd) (sbase = its offset in a (B,F,h,T,T) tensor), or null
__device__ __forceinline__ const float* tat_res_tile(const TatArgs& a, int b, int hd, int T, int64_t sbase) {
  if (a.res_mode == DSTAGNN_RES_BCAST) return a.res + ((int64_t)b * a.h + hd) * T * T;
  if (a.res_mode == DSTAGNN_RES_FULL) return a.res + sbase;
  return nullptr;
}

__device__ __forceinline__ float xor_max_1632(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}

// -------------------------------------------------------------------------------------
// VALU kernels: G threads own one (b, f, head) problem, 256 / G problems per workgroup, Q / K / V
// (and dctx, A, dA) of a problem staged in LDS.  G = 256 is a workgroup per problem; G = 64 (short
// series, T <= 16) a wave per problem, so no lane idles through the T-wide softmax phases: the
// column softmax over the query axis runs on lanes (j = lane % 16, part = lane / 16) with the part
// sums combined by xor-shuffles over lane bits 4 and 5.  All global accesses are row-contiguous
// (coalesced).
// -------------------------------------------------------------------------------------
__host__ __device__ inline int tat_valu_fwd_floats(int T, int dk, int dv) {
  return 2 * T * (dk + 1) + T * (dv + 1) + T * T;
}
__host__ __device__ inline int tat_valu_bwd_floats(int T, int dk, int dv) {
  return 2 * T * (dk + 1) + 2 * T * (dv + 1) + 2 * T * T;
}

template <int G>
__global__ __launch_bounds__(256) void tat_fwd_valu_kernel(TatArgs a) {
  static_assert(G == 64 || G == 256, "a wave or the workgroup per problem");
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int T = a.T, dk = a.dk, dv = a.dv, dkp = dk + 1, dvp = dv + 1;
  const int w = G == 256 ? 0 : threadIdx.x / G, t = threadIdx.x - w * G;
  // the element loops' step; G = 256 keeps the runtime block size, unsigned: with a constant signed
  // step the compiler unrolls these loops to 58 VGPRs against 33
  const unsigned gs = G == 256 ? blockDim.x : G;
  const int id = blockIdx.x * (256 / G) + w;  // ((b*F + f)*h + hd)
  const bool live = G == 256 || id < a.B * a.F * a.h;  // (G = 64: the last workgroup's spare waves)
  float* Qs = sm + w * tat_valu_fwd_floats(T, dk, dv);
  float* Ks = Qs + T * dkp;
  float* Vs = Ks + T * dkp;
  float* Ss = Vs + T * dvp;
  const int hd = id % a.h, bf = id / a.h, b = bf / a.F;
  const int ld = 2 * a.h * dk + a.h * dv;
  const float* base = a.qkv + (int64_t)bf * T * ld;
  if (live) {
    for (int e = t; e < T * dk; e += gs) {
      const int i = e / dk, d = e - i * dk;
      Qs[i * dkp + d] = base[(int64_t)i * ld + hd * dk + d];
      Ks[i * dkp + d] = base[(int64_t)i * ld + a.h * dk + hd * dk + d];
    }
    for (int e = t; e < T * dv; e += gs) {
      const int i = e / dv, d = e - i * dv;
      Vs[i * dvp + d] = base[(int64_t)i * ld + 2 * a.h * dk + hd * dv + d];
    }
  }
  __syncthreads();
  const int64_t sbase = (int64_t)id * T * T;
  if (live) {
    const float* rp = tat_res_tile(a, b, hd, T, sbase);
    for (int e = t; e < T * T; e += gs) {
      const int i = e / T, j = e - i * T;
      float sc = 0.f;
      for (int d = 0; d < dk; ++d) sc = fmaf(Qs[i * dkp + d], Ks[j * dkp + d], sc);
      sc *= a.scale;
      if (rp) sc += rp[e];
      Ss[e] = sc;
      a.re_at[sbase + e] = sc;
    }
  }
  __syncthreads();
  if (live) {  // softmax over i (query axis) for each column j
    if constexpr (G == 64) {
      const int j = t & 15, part = t >> 4;
      float m = -INFINITY;
      if (j < T)
        for (int i = part; i < T; i += 4) m = fmaxf(m, Ss[i * T + j]);
      m = xor_max_1632(m);
      float l = 0.f;
      if (j < T)
        for (int i = part; i < T; i += 4) l += __expf(Ss[i * T + j] - m);
      l = xor_sum_1632(l);
      const float inv = 1.f / l;
      if (j < T)
        for (int i = part; i < T; i += 4) Ss[i * T + j] = __expf(Ss[i * T + j] - m) * inv;
    } else {
      for (int j = t; j < T; j += gs) {
        float m = -INFINITY;
        for (int i = 0; i < T; ++i) m = fmaxf(m, Ss[i * T + j]);
        float l = 0.f;
        for (int i = 0; i < T; ++i) l += expf(Ss[i * T + j] - m);
        float inv = 1.f / l;
        for (int i = 0; i < T; ++i) Ss[i * T + j] = expf(Ss[i * T + j] - m) * inv;
      }
    }
  }
  __syncthreads();
  if (live) {
    for (int e = t; e < T * T; e += gs) a.att[sbase + e] = Ss[e];
    const int ldc = a.h * dv;
    float* cbase = a.ctx + (int64_t)bf * T * ldc;
    for (int e = t; e < T * dv; e += gs) {
      const int i = e / dv, d = e - i * dv;
      float acc = 0.f;
      for (int j = 0; j < T; ++j) acc = fmaf(Ss[i * T + j], Vs[j * dvp + d], acc);
      cbase[(int64_t)i * ldc + hd * dv + d] = acc;
    }
  }
}

template <int G>
__global__ __launch_bounds__(256) void tat_bwd_valu_kernel(TatArgs a) {
  static_assert(G == 64 || G == 256, "a wave or the workgroup per problem");
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int T = a.T, dk = a.dk, dv = a.dv, dkp = dk + 1, dvp = dv + 1;
  const int w = G == 256 ? 0 : threadIdx.x / G, t = threadIdx.x - w * G;
  const unsigned gs = G == 256 ? blockDim.x : G;  // (as in the forward)
  const int id = blockIdx.x * (256 / G) + w;
  const bool live = G == 256 || id < a.B * a.F * a.h;
  float* Qs = sm + w * tat_valu_bwd_floats(T, dk, dv);
  float* Ks = Qs + T * dkp;
  float* Vs = Ks + T * dkp;
  float* dCs = Vs + T * dvp;    // T*dvp
  float* As = dCs + T * dvp;    // T*T
  float* dAs = As + T * T;      // T*T  (becomes dS)
  const int hd = id % a.h, bf = id / a.h;
  const int ld = 2 * a.h * dk + a.h * dv, ldc = a.h * dv;
  const float* base = a.qkv + (int64_t)bf * T * ld;
  const float* cb = a.dctx + (int64_t)bf * T * ldc;
  const int64_t sbase = (int64_t)id * T * T;
  if (live) {
    for (int e = t; e < T * dk; e += gs) {
      const int i = e / dk, d = e - i * dk;
      Qs[i * dkp + d] = base[(int64_t)i * ld + hd * dk + d];
      Ks[i * dkp + d] = base[(int64_t)i * ld + a.h * dk + hd * dk + d];
    }
    for (int e = t; e < T * dv; e += gs) {
      const int i = e / dv, d = e - i * dv;
      Vs[i * dvp + d] = base[(int64_t)i * ld + 2 * a.h * dk + hd * dv + d];
      dCs[i * dvp + d] = cb[(int64_t)i * ldc + hd * dv + d];
    }
    for (int e = t; e < T * T; e += gs) As[e] = a.att[sbase + e];
  }
  __syncthreads();
  float* dbase = a.dqkv + (int64_t)bf * T * ld;
  if (live) {
    for (int e = t; e < T * T; e += gs) {  // dA[i][j] = sum_d dctx[i][d] V[j][d]
      const int i = e / T, j = e - i * T;
      float acc = 0.f;
      for (int d = 0; d < dv; ++d) acc = fmaf(dCs[i * dvp + d], Vs[j * dvp + d], acc);
      dAs[e] = acc;
    }
    for (int e = t; e < T * dv; e += gs) {  // dV[j][d] = sum_i A[i][j] dctx[i][d]
      const int j = e / dv, d = e - j * dv;
      float acc = 0.f;
      for (int i = 0; i < T; ++i) acc = fmaf(As[i * T + j], dCs[i * dvp + d], acc);
      dbase[(int64_t)j * ld + 2 * a.h * dk + hd * dv + d] = acc;
    }
  }
  __syncthreads();
  if (live) {  // column softmax backward: dS = A (dA - sum_i A dA) + d re_At
    if constexpr (G == 64) {
      const int j = t & 15, part = t >> 4;
      float c = 0.f;
      if (j < T)
        for (int i = part; i < T; i += 4) c = fmaf(As[i * T + j], dAs[i * T + j], c);
      c = xor_sum_1632(c);
      if (j < T)
        for (int i = part; i < T; i += 4) {
          float v = As[i * T + j] * (dAs[i * T + j] - c);
          if (a.dre) v += a.dre[sbase + i * T + j];
          dAs[i * T + j] = v;
        }
    } else {
      for (int j = t; j < T; j += gs) {
        float c = 0.f;
        for (int i = 0; i < T; ++i) c = fmaf(As[i * T + j], dAs[i * T + j], c);
        for (int i = 0; i < T; ++i) {
          float v = As[i * T + j] * (dAs[i * T + j] - c);
          if (a.dre) v += a.dre[sbase + i * T + j];
          dAs[i * T + j] = v;
        }
      }
    }
  }
  __syncthreads();
  if (live) {
    for (int e = t; e < T * T; e += gs) a.dscore[sbase + e] = dAs[e];
    // dQ[i][d] = scale * sum_j dS[i][j] K[j][d];  dK[j][d] = scale * sum_i dS[i][j] Q[i][d]
    for (int e = t; e < T * dk; e += gs) {
      const int i = e / dk, d = e - i * dk;
      float sq = 0.f, sk = 0.f;
      for (int j = 0; j < T; ++j) {
        sq = fmaf(dAs[i * T + j], Ks[j * dkp + d], sq);
        sk = fmaf(dAs[j * T + i], Qs[j * dkp + d], sk);
      }
      dbase[(int64_t)i * ld + hd * dk + d] = sq * a.scale;
      dbase[(int64_t)i * ld + a.h * dk + hd * dk + d] = sk * a.scale;
    }
  }
}

// Long-series variants (GAMBIA T = 144: one workgroup per (b,f,head) problem would hold
// 140-160 KB of LDS and leave most of its threads idle in the column phases).  The query-axis
// softmax normalises each COLUMN j over the rows i, so a problem splits into column chunks of
// kTatCW columns, one workgroup each (B*F*h*ceil(T/kTatCW) workgroups):
//   fwd  S[:, chunk] -> re_At, softmax -> att; then ctx = att . V as one batched GEMM
//   bwd  dA[:, chunk] = dctx . V_chunk^T, dV_chunk = A_chunk^T dctx, dS[:, chunk] (-> d score),
//        dK_chunk = s dS_chunk^T Q; then dQ = s dS . K as one batched GEMM
constexpr int kTatCW = 16;

__host__ __device__ inline int tat_cols_fwd_floats(int T, int dk) {
  return T * (dk + 1) + kTatCW * (dk + 1) + T * kTatCW + 2 * 16 * 16;
}
__host__ __device__ inline int tat_cols_bwd_floats(int T, int dk, int dv) {
  return T * (dk + 1) + T * (dv + 1) + kTatCW * (dv + 1) + 2 * T * kTatCW + 16 * 16;
}

// column reduction helper: 256 threads = 16 columns x 16 row groups (tid = g * 16 + jj)
__device__ __forceinline__ float col_reduce16(float v, float* red, bool is_max) {
  const int jj = threadIdx.x & 15, g = threadIdx.x >> 4;
  red[g * 16 + jj] = v;
  __syncthreads();
  float r = red[jj];
#pragma unroll
  for (int q = 1; q < 16; ++q) r = is_max ? fmaxf(r, red[q * 16 + jj]) : r + red[q * 16 + jj];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void tat_fwd_cols_kernel(TatArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int T = a.T, dk = a.dk, dkp = dk + 1;
  const int nch = (T + kTatCW - 1) / kTatCW;
  const int id = blockIdx.x / nch, j0 = (blockIdx.x % nch) * kTatCW, cw = min(kTatCW, T - j0);
  float* Qs = sm;
  float* Ks = Qs + T * dkp;
  float* Ss = Ks + kTatCW * dkp;   // [i][jj]
  float* red = Ss + T * kTatCW;
  const int hd = id % a.h, bf = id / a.h, b = bf / a.F;
  const int ld = 2 * a.h * dk + a.h * a.dv;
  const float* base = a.qkv + (int64_t)bf * T * ld;
  for (int e = threadIdx.x; e < T * dk; e += 256) {
    const int i = e / dk, d = e - i * dk;
    Qs[i * dkp + d] = base[(int64_t)i * ld + hd * dk + d];
  }
  for (int e = threadIdx.x; e < cw * dk; e += 256) {
    const int jj = e / dk, d = e - jj * dk;
    Ks[jj * dkp + d] = base[(int64_t)(j0 + jj) * ld + a.h * dk + hd * dk + d];
  }
  __syncthreads();
  const int64_t sbase = (int64_t)id * T * T;
  const float* rp = tat_res_tile(a, b, hd, T, sbase);
  for (int e = threadIdx.x; e < T * kTatCW; e += 256) {
    const int i = e / kTatCW, jj = e - i * kTatCW;
    float sc = 0.f;
    if (jj < cw) {
      for (int d = 0; d < dk; ++d) sc = fmaf(Qs[i * dkp + d], Ks[jj * dkp + d], sc);
      sc *= a.scale;
      if (rp) sc += rp[(int64_t)i * T + j0 + jj];
      a.re_at[sbase + (int64_t)i * T + j0 + jj] = sc;
    }
    Ss[e] = sc;
  }
  __syncthreads();
  const int jj = threadIdx.x & 15, g = threadIdx.x >> 4;
  float m = -INFINITY;
  for (int i = g; i < T; i += 16) m = fmaxf(m, Ss[i * kTatCW + jj]);
  m = col_reduce16(m, red, true);
  float l = 0.f;
  for (int i = g; i < T; i += 16) l += __expf(Ss[i * kTatCW + jj] - m);
  l = col_reduce16(l, red, false);
  const float inv = 1.f / l;
  if (jj < cw)
    for (int i = g; i < T; i += 16) a.att[sbase + (int64_t)i * T + j0 + jj] = __expf(Ss[i * kTatCW + jj] - m) * inv;
}

__global__ __launch_bounds__(256) void tat_bwd_cols_kernel(TatArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int T = a.T, dk = a.dk, dv = a.dv, dkp = dk + 1, dvp = dv + 1;
  const int nch = (T + kTatCW - 1) / kTatCW;
  const int id = blockIdx.x / nch, j0 = (blockIdx.x % nch) * kTatCW, cw = min(kTatCW, T - j0);
  float* Qs = sm;                       // T x dkp
  float* dCs = Qs + T * dkp;            // T x dvp
  float* Vs = dCs + T * dvp;            // kTatCW x dvp
  float* As = Vs + kTatCW * dvp;        // [i][jj]
  float* dAs = As + T * kTatCW;         // [i][jj] -> dS
  float* red = dAs + T * kTatCW;
  const int hd = id % a.h, bf = id / a.h;
  const int ld = 2 * a.h * dk + a.h * dv, ldc = a.h * dv;
  const float* base = a.qkv + (int64_t)bf * T * ld;
  const float* cb = a.dctx + (int64_t)bf * T * ldc;
  const int64_t sbase = (int64_t)id * T * T;
  for (int e = threadIdx.x; e < T * dk; e += 256) {
    const int i = e / dk, d = e - i * dk;
    Qs[i * dkp + d] = base[(int64_t)i * ld + hd * dk + d];
  }
  for (int e = threadIdx.x; e < T * dv; e += 256) {
    const int i = e / dv, d = e - i * dv;
    dCs[i * dvp + d] = cb[(int64_t)i * ldc + hd * dv + d];
  }
  for (int e = threadIdx.x; e < cw * dv; e += 256) {
    const int jj = e / dv, d = e - jj * dv;
    Vs[jj * dvp + d] = base[(int64_t)(j0 + jj) * ld + 2 * a.h * dk + hd * dv + d];
  }
  for (int e = threadIdx.x; e < T * kTatCW; e += 256) {
    const int i = e / kTatCW, jj = e - i * kTatCW;
    As[e] = jj < cw ? a.att[sbase + (int64_t)i * T + j0 + jj] : 0.f;
  }
  __syncthreads();
  float* dbase = a.dqkv + (int64_t)bf * T * ld;
  for (int e = threadIdx.x; e < T * kTatCW; e += 256) {  // dA[i][j] = sum_d dctx[i][d] V[j][d]
    const int i = e / kTatCW, jj = e - i * kTatCW;
    float acc = 0.f;
    if (jj < cw)
      for (int d = 0; d < dv; ++d) acc = fmaf(dCs[i * dvp + d], Vs[jj * dvp + d], acc);
    dAs[e] = acc;
  }
  for (int e = threadIdx.x; e < cw * dv; e += 256) {  // dV[j][d] = sum_i A[i][j] dctx[i][d]
    const int jj = e / dv, d = e - jj * dv;
    float acc = 0.f;
    for (int i = 0; i < T; ++i) acc = fmaf(As[i * kTatCW + jj], dCs[i * dvp + d], acc);
    dbase[(int64_t)(j0 + jj) * ld + 2 * a.h * dk + hd * dv + d] = acc;
  }
  __syncthreads();
  // column softmax backward: dS = A (dA - sum_i A dA) + d re_At
  const int jj = threadIdx.x & 15, g = threadIdx.x >> 4;
  float c = 0.f;
  for (int i = g; i < T; i += 16) c = fmaf(As[i * kTatCW + jj], dAs[i * kTatCW + jj], c);
  c = col_reduce16(c, red, false);
  for (int i = g; i < T; i += 16) {
    float v = As[i * kTatCW + jj] * (dAs[i * kTatCW + jj] - c);
    if (jj < cw) {
      if (a.dre) v += a.dre[sbase + (int64_t)i * T + j0 + jj];
      a.dscore[sbase + (int64_t)i * T + j0 + jj] = v;
    }
    dAs[i * kTatCW + jj] = v;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < cw * dk; e += 256) {  // dK[j][d] = s sum_i dS[i][j] Q[i][d]
    const int jj2 = e / dk, d = e - jj2 * dk;
    float acc = 0.f;
    for (int i = 0; i < T; ++i) acc = fmaf(dAs[i * kTatCW + jj2], Qs[i * dkp + d], acc);
    dbase[(int64_t)(j0 + jj2) * ld + a.h * dk + hd * dk + d] = acc * a.scale;
  }
}

// =====================================================================================
// Matrix-core kernels (tat_core.hpp): one wave per (b, f, head) problem, four per workgroup,
// operands from global memory straight into registers.  (The G = 64 VALU kernels above spend
// ~2 400 VALU and ~700 LDS instructions per problem on index arithmetic and LDS operands.)
// =====================================================================================
template <int T>
__global__ __launch_bounds__(256) void tat_fwd_mfma_kernel(TatArgs a) {
  static_assert(T % 4 == 0 && T <= 16, "one 16 x 16 tile, float4 rows");
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c = l & 15, q = l >> 4;
  const int id = blockIdx.x * kTatW + w;
  if (id >= a.B * a.F * a.h) return;  // no barrier in this kernel
  const int h = a.h, hd = id % h, bf = id / h, b = bf / a.F;
  const int ld = 3 * h * kTatD;
  const float* Qp = a.qkv + (int64_t)bf * T * ld + hd * kTatD;
  const float* Kp = Qp + h * kTatD;
  const float* Vp = Qp + 2 * h * kTatD;
  const bool vi = c < T, vj = q < T / 4;
  TatFwdOps o;
  tat_fwd_load<T>(o, Qp, Kp, Vp, (int64_t)ld, c, q);
  const int64_t sbase = (int64_t)id * T * T;
  const float* rp = tat_res_tile(a, b, hd, T, sbase);
  float4 rr = {0.f, 0.f, 0.f, 0.f};
  if (rp && vi && vj) rr = *reinterpret_cast<const float4*>(rp + c * T + 4 * q);
  // lane (c, q) holds S[i = c][j = 4q + r]
  float sc[4], p[4];
  tat_fwd_scores(sc, o, rr, a.scale);
  if (vi && vj) *reinterpret_cast<float4*>(a.re_at + sbase + c * T + 4 * q) = make_float4(sc[0], sc[1], sc[2], sc[3]);
  tat_fwd_softmax<T>(p, sc, c, q);
  if (vi && vj) *reinterpret_cast<float4*>(a.att + sbase + c * T + 4 * q) = make_float4(p[0], p[1], p[2], p[3]);
  floatx4 c0, c1;
  tat_fwd_ctx(c0, c1, p, o);
  const int ldc = h * kTatD;
  float* cb = a.ctx + (int64_t)bf * T * ldc + hd * kTatD + c;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = 4 * q + r;
    if (i < T) {
      cb[(int64_t)i * ldc] = c0[r];
      cb[(int64_t)i * ldc + 16] = c1[r];
    }
  }
}

template <int T>
__global__ __launch_bounds__(256) void tat_bwd_mfma_kernel(TatArgs a) {
  static_assert(T % 4 == 0 && T <= 16, "one 16 x 16 tile");
  __shared__ float tr[kTatW][16 * 17];  // per-wave dS transpose (dQ's A operand)
  __shared__ float red[kTatW][T * T];   // F-sum: the workgroup's four dS tiles
  __shared__ int last;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c = l & 15, q = l >> 4;
  const int h = a.h, P = a.B * a.F * h;
  const int nch = a.F / kTatW;
  int id;
  if (a.dres_sum) {  // workgroup = (b, head, four consecutive f): wave w takes f = 4 ch + w
    const int bh = blockIdx.x / nch, ch = blockIdx.x - bh * nch;
    id = ((bh / h) * a.F + ch * kTatW + w) * h + bh % h;
  } else {
    id = blockIdx.x * kTatW + w;
  }
  const bool live = id < P;
  const int hd = id % h, bf = id / h;
  const int ld = 3 * h * kTatD, ldc = h * kTatD;
  const float* Qp = a.qkv + (int64_t)bf * T * ld + hd * kTatD;
  const float* Kp = Qp + h * kTatD;
  const float* Vp = Qp + 2 * h * kTatD;
  const float* Cp = a.dctx + (int64_t)bf * T * ldc + hd * kTatD;
  const int64_t sbase = (int64_t)id * T * T;
  const bool vj = c < T;  // lane column j = c; rows i = 4q + r
  // every load up front: the core's operands, then A[i = 4q + r][j = c] and d re_At
  TatBwdOps o;
  tat_bwd_load<T>(o, Qp, Kp, Vp, (int64_t)ld, Cp, (int64_t)ldc, c, q, live);
  float at[4], dr[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int i = 4 * q + s;
    const bool ok = live && i < T && vj;
    at[s] = ok ? a.att[sbase + i * T + c] : 0.f;
    dr[s] = ok && a.dre ? a.dre[sbase + i * T + c] : 0.f;
  }
  float ds[4];
  TatBwdGrads g;
  tat_bwd_part1(ds, g, tr[w], o, at, dr, c, q);
  if (a.keep_ds && live && vj) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (4 * q + r < T) a.dscore[sbase + (4 * q + r) * T + c] = ds[r];
  }
  if (a.dres_sum && vj) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (4 * q + r < T) red[w][(4 * q + r) * T + c] = ds[r];
  }
  __syncthreads();
  tat_bwd_part2(g, tr[w], o, c, q);
  if (live) {
    float* db = a.dqkv + (int64_t)bf * T * ld + hd * kTatD + c;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 4 * q + r;
      if (i >= T) continue;
      float* row = db + (int64_t)i * ld;
      row[0] = g.gq0[r] * a.scale;
      row[16] = g.gq1[r] * a.scale;
      row[h * kTatD] = g.gk0[r] * a.scale;
      row[h * kTatD + 16] = g.gk1[r] * a.scale;
      row[2 * h * kTatD] = g.gv0[r];
      row[2 * h * kTatD + 16] = g.gv1[r];
    }
  }
  if (!a.dres_sum) return;
  // res_att gradient sum_f dS (deterministic): the four tiles in wave order, one partial per
  // workgroup, a ticket per (b, head); the last of its nch workgroups adds the partials in chunk
  // order (handoff.hpp)
  const int t = threadIdx.x, bh = blockIdx.x / nch, ch = blockIdx.x - bh * nch;
  float* part = a.dscore + (int64_t)bh * nch * T * T;
  if (t < T * T) st_agent(part + (int64_t)ch * T * T + t, ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t]);
  if (!last_arrival(a.cnt + bh, nch, &last) || t >= T * T) return;
  float v = 0.f;
  for (int k = 0; k < nch; ++k) v += ld_agent(part + (int64_t)k * T * T + t);
  a.dres_sum[(int64_t)bh * T * T + t] = v;
}

// dynamic LDS above 64 KB must be opted into per kernel (gfx950 has 160 KB per workgroup)
int allow_lds(const void* kernel, size_t bytes) {
  hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) { set_last_error(std::string("LDS attribute: ") + hipGetErrorString(e)); return (int)e; }
  return 0;
}

// the matrix-core kernels: T in {4, 8, 12, 16}, d_k = d_v = 32, 16-B aligned operands
// (float4 rows); DSTAGNN_TAT_MFMA=0 keeps the G = 64 VALU kernels (A/B switch)
bool tat_mfma_ok(int T, int dk, int dv, std::initializer_list<const float*> ptrs) {
  static const bool off = !env_flag("DSTAGNN_TAT_MFMA", true);
  if (off || dk != kTatD || dv != kTatD || T % 4 != 0 || T < 4 || T > 16) return false;
  for (const float* p : ptrs)
    if (reinterpret_cast<uintptr_t>(p) % 16 != 0) return false;
  return true;
}

// The path per direction.  A G = 256 problem holds 4 (99 T + T^2) bytes of LDS in the forward and
// 4 (132 T + 2 T^2) in the backward at d_k = d_v = 32, so the forward leaves it for the column
// chunks at T >= 88 and the backward at T >= 64: for T in 64..87 the G = 256 forward feeds the
// column-chunk backward (both read and write the same att / re_At layout).
enum TatPath { kTatMfma, kTatValu64, kTatValu256, kTatCols };
TatPath tat_path(bool mfma, int T, size_t valu_floats) {
  if (mfma) return kTatMfma;
  if (T <= 16 && kTatW * valu_floats * sizeof(float) <= 64 * 1024) return kTatValu64;
  return valu_floats * sizeof(float) > 64 * 1024 ? kTatCols : kTatValu256;
}
TatPath tat_fwd_path(const TatArgs& a) {
  return tat_path(tat_mfma_ok(a.T, a.dk, a.dv, {a.qkv, a.res, a.re_at, a.att}), a.T,
                  (size_t)tat_valu_fwd_floats(a.T, a.dk, a.dv));
}
TatPath tat_bwd_path(const TatArgs& a) {
  return tat_path(tat_mfma_ok(a.T, a.dk, a.dv, {a.qkv, a.att, a.dctx, a.dre}), a.T,
                  (size_t)tat_valu_bwd_floats(a.T, a.dk, a.dv));
}

TatArgs tat_args(int B, int F, int T, int h, int dk, int dv, const float* qkv) {
  TatArgs a{};
  a.B = B; a.F = F; a.T = T; a.h = h; a.dk = dk; a.dv = dv;
  a.qkv = qkv; a.scale = 1.f / sqrtf((float)dk);
  return a;
}

// K<T> for the matrix-core kernels' four T
#define DS_TAT_MFMA(K, grid) \
  switch (a.T) { \
    case 4: hipLaunchKernelGGL(K<4>, grid, dim3(64 * kTatW), 0, st, a); break; \
    case 8: hipLaunchKernelGGL(K<8>, grid, dim3(64 * kTatW), 0, st, a); break; \
    case 12: hipLaunchKernelGGL(K<12>, grid, dim3(64 * kTatW), 0, st, a); break; \
    default: hipLaunchKernelGGL(K<16>, grid, dim3(64 * kTatW), 0, st, a); break; \
  }

// the column-chunk kernel K, then the batched GEMM g that completes it
template <class K>
int launch_tat_cols(K kernel, const char* what, const TatArgs& a, size_t lc, const Gemm& g, hipStream_t st) {
  if (lc > 160 * 1024) { set_last_error(std::string(what) + ": T too large for LDS"); return DSTAGNN_E_SHAPE; }
  if (lc > 64 * 1024) DS_TRY(allow_lds((const void*)kernel, lc));
  const int nch = (a.T + kTatCW - 1) / kTatCW;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(a.B * a.F * a.h * nch)), dim3(256), lc, st, a);
  DS_CHECK_LAUNCH();
  return run_gemm(g, nullptr, 0, st);
}

}  // namespace

int op_tat_fwd(int B, int F, int T, int h, int dk, int dv, const float* qkv, const float* res, int res_mode,
               float* re_at, float* att, float* ctx, hipStream_t st) {
  TatArgs a = tat_args(B, F, T, h, dk, dv, qkv);
  a.res = res; a.res_mode = res ? res_mode : 0;
  a.re_at = re_at; a.att = att; a.ctx = ctx;
  const int P = B * F * h;
  const size_t lds = sizeof(float) * (size_t)tat_valu_fwd_floats(T, dk, dv);
  switch (tat_fwd_path(a)) {
    case kTatMfma: DS_TAT_MFMA(tat_fwd_mfma_kernel, dim3((unsigned)cdiv64(P, kTatW))) break;
    case kTatValu64:
      hipLaunchKernelGGL(tat_fwd_valu_kernel<64>, dim3((unsigned)cdiv64(P, kTatW)), dim3(256), kTatW * lds, st, a);
      break;
    case kTatValu256: hipLaunchKernelGGL(tat_fwd_valu_kernel<256>, dim3((unsigned)P), dim3(256), lds, st, a); break;
    case kTatCols: {  // long series: column chunks, then ctx = att . V as one batched GEMM
      const int64_t ld = 2 * (int64_t)h * dk + (int64_t)h * dv, ldc = (int64_t)h * dv;
      Gemm g;  // ctx[bf,i,hd,:] = sum_j att[bf,hd,i,j] V[bf,j,hd,:]
      g.M = T; g.N = dv; g.K = T; g.batch = P;
      g.A = att; g.am = idx1(T); g.ak = idx1(1); g.az = idx1((int64_t)T * T);
      g.B = qkv; g.b_off = 2 * (int64_t)h * dk; g.bk = idx1(ld); g.bn = idx1(1); g.bz = idx2(h, dv, (int64_t)T * ld);
      g.C = ctx; g.cm = idx1(ldc); g.cn = idx1(1); g.cz = idx2(h, dv, (int64_t)T * ldc);
      return launch_tat_cols(tat_fwd_cols_kernel, "tat_fwd", a, sizeof(float) * (size_t)tat_cols_fwd_floats(T, dk), g, st);
    }
  }
  DS_CHECK_LAUNCH();
  return 0;
}

int op_tat_bwd(int B, int F, int T, int h, int dk, int dv, const float* qkv, const float* att, const float* dctx,
               const float* dre, float* dqkv, float* dscore, float* dres_sum, hipStream_t st) {
  TatArgs a = tat_args(B, F, T, h, dk, dv, qkv);
  a.att = const_cast<float*>(att); a.dctx = dctx; a.dre = dre; a.dqkv = dqkv; a.dscore = dscore;
  a.keep_ds = 1;
  const TatPath path = tat_bwd_path(a);
  if (dres_sum) {  // the full dS is scratch; the output is its sum over f
    a.cnt = path == kTatMfma && F % kTatW == 0 ? stream_counters(st, B * h) : nullptr;
    if (!a.cnt) {
      DS_TRY(op_tat_bwd(B, F, T, h, dk, dv, qkv, att, dctx, dre, dqkv, dscore, nullptr, st));
      return op_sum_middle(dscore, B, F, (int64_t)h * T * T, dres_sum, 0.f, st);
    }
    a.dres_sum = dres_sum; a.keep_ds = 0;
    DS_TAT_MFMA(tat_bwd_mfma_kernel, dim3((unsigned)(B * h * (F / kTatW))))
    DS_CHECK_LAUNCH();
    return 0;
  }
  const int P = B * F * h;
  const size_t lds = sizeof(float) * (size_t)tat_valu_bwd_floats(T, dk, dv);
  switch (path) {
    case kTatMfma: DS_TAT_MFMA(tat_bwd_mfma_kernel, dim3((unsigned)cdiv64(P, kTatW))) break;
    case kTatValu64:
      hipLaunchKernelGGL(tat_bwd_valu_kernel<64>, dim3((unsigned)cdiv64(P, kTatW)), dim3(256), kTatW * lds, st, a);
      break;
    case kTatValu256: hipLaunchKernelGGL(tat_bwd_valu_kernel<256>, dim3((unsigned)P), dim3(256), lds, st, a); break;
    case kTatCols: {  // long series: column chunks, then dQ = s dS . K as one batched GEMM
      const int64_t ld = 2 * (int64_t)h * dk + (int64_t)h * dv;
      Gemm g;  // dQ[bf,i,hd,:] = s sum_j dS[bf,hd,i,j] K[bf,j,hd,:]
      g.M = T; g.N = dk; g.K = T; g.batch = P;
      g.A = dscore; g.am = idx1(T); g.ak = idx1(1); g.az = idx1((int64_t)T * T);
      g.B = qkv; g.b_off = (int64_t)h * dk; g.bk = idx1(ld); g.bn = idx1(1); g.bz = idx2(h, dk, (int64_t)T * ld);
      g.C = dqkv; g.cm = idx1(ld); g.cn = idx1(1); g.cz = idx2(h, dk, (int64_t)T * ld);
      g.alpha = a.scale;
      return launch_tat_cols(tat_bwd_cols_kernel, "tat_bwd", a, sizeof(float) * (size_t)tat_cols_bwd_floats(T, dk, dv), g,
                             st);
    }
  }
  DS_CHECK_LAUNCH();
  return 0;
}
#undef DS_TAT_MFMA
