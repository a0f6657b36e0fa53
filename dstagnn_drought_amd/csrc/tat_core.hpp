// tat_core.hpp — the matrix-core temporal-attention core of one (b, f, head) problem on one wave:
// T <= 16 with T % 4 == 0, d_k = d_v = 32 (model/DSTAGNN_my.py:27-67 at T = 12).  The T x T tile
// is padded to 16 x 16 and every product is a v_mfma_f32_16x16x4_f32 chain (fragments:
// A[l&15][k = l>>4], B[k = l>>4][l&15], D[4(l>>4) + r][l&15]).  Each product's contraction index
// is assigned to (k slot q = l>>4, step s) as 4q + s, so an accumulator tile whose ROW index is
// that contraction index is, register s for register s, the next product's A operand: scores ->
// P -> ctx in the forward, dA -> dS -> dK / dV in the backward, with one 16 x 17 LDS transpose of
// dS for dQ.
//
// Two callers: tat.hip (operands from global memory, one problem per wave) and tat_fused.hip
// (operands from the workgroup's LDS tiles, several tasks per wave).  Operand loads take a
// pointer and a row stride of type LD (int64_t for global rows, int for LDS rows); which problem
// a wave takes, the residual / att / d re_At operands and every store of a result stay with the
// caller, and so does the barrier between the backward's two parts.  Lane (c = l & 15, q = l >> 4).
#pragma once
#include "common.hpp"

constexpr int kTatD = 32;  // d_k = d_v of the matrix-core kernels

__device__ __forceinline__ float xor_sum_1632(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// the eight-step contraction over d = 8q + s of two row fragments (a0 | a1)[8], (b0 | b1)[8]
__device__ __forceinline__ floatx4 tat_mfma_d8(const float4& a0, const float4& a1, const float4& b0, const float4& b1) {
  floatx4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = mfma16(a0.x, b0.x, acc);
  acc = mfma16(a0.y, b0.y, acc);
  acc = mfma16(a0.z, b0.z, acc);
  acc = mfma16(a0.w, b0.w, acc);
  acc = mfma16(a1.x, b1.x, acc);
  acc = mfma16(a1.y, b1.y, acc);
  acc = mfma16(a1.z, b1.z, acc);
  acc = mfma16(a1.w, b1.w, acc);
  return acc;
}

// row fragment p[row c][8q .. 8q + 7] (the operand of a contraction over d); zero when !ok
template <class LD>
__device__ __forceinline__ void tat_ld_row8(float4& lo, float4& hi, const float* p, LD ld, int c, int q, bool ok) {
  lo = hi = float4{0.f, 0.f, 0.f, 0.f};
  if (ok) {
    lo = *reinterpret_cast<const float4*>(p + (LD)c * ld + 8 * q);
    hi = *reinterpret_cast<const float4*>(p + (LD)c * ld + 8 * q + 4);
  }
}

// ---- forward ---------------------------------------------------------------------------------
struct TatFwdOps {
  float vv[2][4];         // ctx's B operand V[j = 4q + s][d = c + 16t]
  float4 k0, k1, q0, q1;  // S^T = K Q^T: A[m = j][k = d] = K[j = c][8q + s], B[k = d][n = i] = Q[i = c][8q + s]
};
// V first: it does not depend on the scores
template <int T, class LD>
__device__ __forceinline__ void tat_fwd_load(TatFwdOps& o, const float* Qp, const float* Kp, const float* Vp, LD ld,
                                             int c, int q) {
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int t = 0; t < 2; ++t) o.vv[t][s] = (4 * q + s < T) ? Vp[(LD)(4 * q + s) * ld + c + 16 * t] : 0.f;
  tat_ld_row8(o.k0, o.k1, Kp, ld, c, q, c < T);
  tat_ld_row8(o.q0, o.q1, Qp, ld, c, q, c < T);
}
// sc[r] = S[i = c][j = 4q + r] = scale Q K^T + the residual row fragment rr
__device__ __forceinline__ void tat_fwd_scores(float (&sc)[4], const TatFwdOps& o, const float4& rr, float scale) {
  const floatx4 acc = tat_mfma_d8(o.k0, o.k1, o.q0, o.q1);
  const float rv[4] = {rr.x, rr.y, rr.z, rr.w};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    sc[r] = acc[r] * scale;
    sc[r] += rv[r];
  }
}
// softmax over the query axis i = the 16 lanes c of this quarter (column j = 4q + r)
template <int T>
__device__ __forceinline__ void tat_fwd_softmax(float (&p)[4], const float (&sc)[4], int c, int q) {
  const bool vi = c < T, vj = q < T / 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float m = xor_max_16(vi ? sc[r] : -INFINITY);
    const float e = vi ? __expf(sc[r] - m) : 0.f;
    const float inv = 1.f / xor_sum_16(e);
    p[r] = vj ? e * inv : 0.f;
  }
}
// ctx = P V: A[m = i][k = j] = P[i = c][j = 4q + s] = p[s], B = vv; c0 / c1[r] = ctx[4q + r][c (+ 16)]
__device__ __forceinline__ void tat_fwd_ctx(floatx4& c0, floatx4& c1, const float (&p)[4], const TatFwdOps& o) {
  c0 = c1 = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    c0 = mfma16(p[s], o.vv[0][s], c0);
    c1 = mfma16(p[s], o.vv[1][s], c1);
  }
}

// ---- backward --------------------------------------------------------------------------------
struct TatBwdOps {
  float4 d0, d1, v0, v1;              // dA's operands dC[i = c][8q + s] / V[j = c][8q + s]
  float cb[2][4], qb[2][4], kb[2][4];  // the B operands [4q + s][c + 16t] of dV (dC), dK (Q) and dQ (K)
};
struct TatBwdGrads {
  floatx4 gq0, gq1, gk0, gk1, gv0, gv1;  // g*0 / g*1[r] = d{Q,K,V}[4q + r][c (+ 16)], unscaled
};
// every load up front (Cp: dctx rows of stride ldc; Qp / Kp / Vp: rows of stride ld)
template <int T, class LD>
__device__ __forceinline__ void tat_bwd_load(TatBwdOps& o, const float* Qp, const float* Kp, const float* Vp, LD ld,
                                             const float* Cp, LD ldc, int c, int q, bool live) {
  tat_ld_row8(o.d0, o.d1, Cp, ldc, c, q, live && c < T);
  tat_ld_row8(o.v0, o.v1, Vp, ld, c, q, live && c < T);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int i = 4 * q + s;
    const bool ok = live && i < T;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      o.cb[t][s] = ok ? Cp[(LD)i * ldc + c + 16 * t] : 0.f;
      o.qb[t][s] = ok ? Qp[(LD)i * ld + c + 16 * t] : 0.f;
      o.kb[t][s] = ok ? Kp[(LD)i * ld + c + 16 * t] : 0.f;
    }
  }
}
// part one: dA = dC V^T (D[m = i][n = j]); the column softmax backward over i (this lane's four
// rows, then the quarters), ds[r] = dS[4q + r][c] = A (dA - sum_i A dA) + d re_At; dV = A^T dC and
// dK = dS^T Q (A operand [m = j = c][k = i = 4q + s] = at[s] / ds[s]); dS into the wave's
// 16 x 17 transpose tile tr.  The caller's barrier over tr follows.
__device__ __forceinline__ void tat_bwd_part1(float (&ds)[4], TatBwdGrads& g, float* tr, const TatBwdOps& o,
                                              const float (&at)[4], const float (&dr)[4], int c, int q) {
  const floatx4 dA = tat_mfma_d8(o.d0, o.d1, o.v0, o.v1);
  float cs = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) cs = fmaf(at[r], dA[r], cs);
  cs = xor_sum_1632(cs);
#pragma unroll
  for (int r = 0; r < 4; ++r) ds[r] = at[r] * (dA[r] - cs) + dr[r];
  const floatx4 z = {0.f, 0.f, 0.f, 0.f};
  g.gv0 = g.gv1 = g.gk0 = g.gk1 = g.gq0 = g.gq1 = z;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    g.gv0 = mfma16(at[s], o.cb[0][s], g.gv0);
    g.gv1 = mfma16(at[s], o.cb[1][s], g.gv1);
    g.gk0 = mfma16(ds[s], o.qb[0][s], g.gk0);
    g.gk1 = mfma16(ds[s], o.qb[1][s], g.gk1);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) tr[(4 * q + r) * 17 + c] = ds[r];
}
// part two: dQ = dS K, A operand [m = i = c][k = j = 4q + s] = dS[c][4q + s] from tr
__device__ __forceinline__ void tat_bwd_part2(TatBwdGrads& g, const float* tr, const TatBwdOps& o, int c, int q) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const float x = tr[c * 17 + 4 * q + s];
    g.gq0 = mfma16(x, o.kb[0][s], g.gq0);
    g.gq1 = mfma16(x, o.kb[1][s], g.gq1);
  }
}
