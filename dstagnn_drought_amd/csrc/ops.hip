// ops.hip — the non-GEMM kernels of the DSTAGNN block (gfx950, wave64), apart from the temporal
// attention core (tat.hip, tat_fused.hip).
//
//   ln_fwd / ln_bwd       row LayerNorm over strided multi-source sums (TAt LN_N :100,
//                         EmbedT LN_N :176-181, EmbedS LN_D :180-181) + fused dropout
//   cheb_softmax_fwd/bwd  column softmax over source node i of S'+A_pa*M_k, times T_k
//                         (cheb_conv_withSAt :126-128), and its backward
//   gate_fwd / gate_bwd   GTU gates tanh(p)*sigmoid(q) + concat (:192-197, :242)
//   tail_fwd / tail_bwd   fcmy dropout + residual + ReLU + LN_C (:243-252)
//   reductions            deterministic two-stage column sums (bias / gamma / beta grads)
#include <map>
#include <mutex>

#include "common.hpp"
#include "handoff.hpp"
#include "ops.hpp"

namespace {

// =====================================================================================
// generic batched transpose  out[b][c][r] = in[b][r][c] (+ beta * out)
// =====================================================================================
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                        int R, int Cc, int64_t in_bs, int64_t out_bs, float beta) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z;
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  const float* ip = in + (int64_t)b * in_bs;
  float* op = out + (int64_t)b * out_bs;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  // the accumulated output's old values are loaded in the same round as the input tile (they do
  // not depend on it): one memory round trip per workgroup instead of two
  float old[4] = {0.f, 0.f, 0.f, 0.f};
  if (beta != 0.f) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = c0 + ty + 8 * u, r = r0 + tx;
      if (r < R && c < Cc) old[u] = op[(int64_t)c * R + r];
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int y = ty + 8 * u, r = r0 + y, c = c0 + tx;
    tile[y][tx] = (r < R && c < Cc) ? ip[(int64_t)r * Cc + c] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int y = ty + 8 * u, c = c0 + y, r = r0 + tx;
    if (r < R && c < Cc) {
      const int64_t o = (int64_t)c * R + r;
      float v = tile[tx][y];
      if (beta != 0.f) v += beta * old[u];
      op[o] = v;
    }
  }
}

// =====================================================================================
// LayerNorm over rows of length L; one wave per row, values kept in registers.
// Every global load of a row (all sources, gamma / beta) is issued in one round, branch-free
// (out-of-row lanes load the row's last element and are masked after): a per-element
// `if (e < L)` around a load, or a runtime loop over the sources, made the compiler wait
// vmcnt(0) after every load — 16 dependent round trips per row for the EmbedS LN (L = 512, two
// sources), ~1.3 TB/s.
// =====================================================================================
template <int VPT, int NSRC>
__global__ __launch_bounds__(256) void ln_fwd_kernel(LnFwd a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.R) return;
  const int L = a.L;
  const float* sp[NSRC];
  int64_t o[NSRC], es[NSRC];
#pragma unroll
  for (int s = 0; s < NSRC; ++s) {
    sp[s] = a.src[s].p;
    o[s] = ioff(a.src[s].row, row);
    es[s] = a.src[s].es;
  }
  // long rows (VPT > 16: GAMBIA's N = 2139) keep one value per element in registers and read
  // gamma / beta at the store (register budget); short ones preload everything
  constexpr bool PRE = VPT <= 16;
  float v[VPT], gv[PRE ? VPT : 1], bv[PRE ? VPT : 1];
  float sum = 0.f;
  if constexpr (PRE) {
    float xs[NSRC][VPT];
#pragma unroll
    for (int q = 0; q < VPT; ++q) {
      const int e = min(lane + 64 * q, L - 1);
#pragma unroll
      for (int s = 0; s < NSRC; ++s) xs[s][q] = sp[s][o[s] + (int64_t)e * es[s]];
      gv[q] = a.g[e];
      bv[q] = a.b[e];
    }
#pragma unroll
    for (int q = 0; q < VPT; ++q) {
      float u = 0.f;
#pragma unroll
      for (int s = 0; s < NSRC; ++s) u += xs[s][q];
      v[q] = lane + 64 * q < L ? u : 0.f;
    }
  } else {
#pragma unroll
    for (int q = 0; q < VPT; ++q) {
      const int e = min(lane + 64 * q, L - 1);
      float u = 0.f;
#pragma unroll
      for (int s = 0; s < NSRC; ++s) u += sp[s][o[s] + (int64_t)e * es[s]];
      v[q] = lane + 64 * q < L ? u : 0.f;
    }
  }
#pragma unroll
  for (int q = 0; q < VPT; ++q) sum += v[q];
  const float mean = wave_sum(sum) / L;
  float var = 0.f;
#pragma unroll
  for (int q = 0; q < VPT; ++q) {
    int e = lane + 64 * q;
    if (e < L) { float d = v[q] - mean; var += d * d; }
  }
  var = wave_sum(var) / L;
  const float rs = rsqrtf(var + a.eps);
  if (lane == 0 && a.mu) { a.mu[row] = mean; a.rs[row] = rs; }  // (null: forward-only, a scalar branch)
  const int64_t yo = ioff(a.yrow, row);
#pragma unroll
  for (int q = 0; q < VPT; ++q) {
    int e = lane + 64 * q;
    if (e < L) {
      if (a.u) a.u[(int64_t)row * L + e] = v[q];
      float y = (v[q] - mean) * rs * (PRE ? gv[PRE ? q : 0] : a.g[e]) + (PRE ? bv[PRE ? q : 0] : a.b[e]);
      if (a.drop_p > 0.f) y *= drop_scale(a.seed, a.which, (uint64_t)row * L + e + a.drop_off, a.drop_p);
      a.y[yo + (int64_t)e * a.yes] = y;
    }
  }
}

// Rows of L = 256 V4 contiguous floats (the EmbedS LayerNorm over D = 512): the same
// arithmetic with every load and store a float4 — lane l holds elements 4 (l + 64 q) .. + 3 —
// so a row is V4 16-B loads per source per lane instead of 4 V4 dword loads (the wave-per-row
// kernel above at L = 512 issued 32 loads and 16 stores per lane).  The row sums go over a
// different partition of the row (within the fp32 rounding of the other kernel).
__device__ __forceinline__ void l4set(float4& v, int c, float x) {
  if (c == 0) v.x = x; else if (c == 1) v.y = x; else if (c == 2) v.z = x; else v.w = x;
}
template <int V4, int NSRC>
__global__ __launch_bounds__(256) void ln_fwd_v4_kernel(LnFwd a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.R) return;
  constexpr int L = 256 * V4;
  float4 xs[NSRC][V4], gv[V4], bv[V4], v[V4];
#pragma unroll
  for (int q = 0; q < V4; ++q) {
    const int e4 = lane + 64 * q;
#pragma unroll
    for (int s = 0; s < NSRC; ++s)
      xs[s][q] = reinterpret_cast<const float4*>(a.src[s].p + ioff(a.src[s].row, row))[e4];
    gv[q] = reinterpret_cast<const float4*>(a.g)[e4];
    bv[q] = reinterpret_cast<const float4*>(a.b)[e4];
  }
  float sum = 0.f;
#pragma unroll
  for (int q = 0; q < V4; ++q) {
    v[q] = xs[0][q];
#pragma unroll
    for (int s = 1; s < NSRC; ++s) {
      v[q].x += xs[s][q].x; v[q].y += xs[s][q].y; v[q].z += xs[s][q].z; v[q].w += xs[s][q].w;
    }
    sum += (v[q].x + v[q].y) + (v[q].z + v[q].w);
  }
  const float mean = wave_sum(sum) / L;
  float var = 0.f;
#pragma unroll
  for (int q = 0; q < V4; ++q)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float d = f4at(v[q], c) - mean;
      var += d * d;
    }
  var = wave_sum(var) / L;
  const float rs = rsqrtf(var + a.eps);
  if (lane == 0 && a.mu) { a.mu[row] = mean; a.rs[row] = rs; }  // (null: forward-only, a scalar branch)
  const int64_t yo = ioff(a.yrow, row);
  const DropKey dk = drop_key(a.seed, a.which);
  const float dscale = 1.0f / (1.0f - a.drop_p);
#pragma unroll
  for (int q = 0; q < V4; ++q) {
    const int e4 = lane + 64 * q;
    if (a.u) reinterpret_cast<float4*>(a.u + (int64_t)row * L)[e4] = v[q];
    float4 y;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float t = (f4at(v[q], c) - mean) * rs * f4at(gv[q], c) + f4at(bv[q], c);
      if (a.drop_p > 0.f) t *= drop_u(dk, (uint64_t)row * L + 4 * e4 + c + a.drop_off) >= a.drop_p ? dscale : 0.0f;
      l4set(y, c, t);
    }
    reinterpret_cast<float4*>(a.y + yo)[e4] = y;
  }
}

// the backward of the same rows (ln_bwd_kernel's arithmetic; PART: per-workgroup partial slabs)
template <int V4, bool PART>
__global__ __launch_bounds__(256) void ln_bwd_v4_kernel(LnBwd a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  constexpr int L = 256 * V4;
  const int row = blockIdx.x * 4 + wv;
  float4 gp[V4], bp[V4], xp[V4];
#pragma unroll
  for (int q = 0; q < V4; ++q) gp[q] = bp[q] = xp[q] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (row < a.R) {
    const int64_t yo = ioff(a.dyrow, row), xo = ioff(a.dxrow, row);
    float4 dyl[V4], ul[V4], gl[V4], xin[V4];
#pragma unroll
    for (int q = 0; q < V4; ++q) {
      const int e4 = lane + 64 * q;
      dyl[q] = reinterpret_cast<const float4*>(a.dy + yo)[e4];
      ul[q] = reinterpret_cast<const float4*>(a.u + (int64_t)row * L)[e4];
      gl[q] = reinterpret_cast<const float4*>(a.g)[e4];
      if (a.beta != 0.f) xin[q] = reinterpret_cast<const float4*>(a.dx + xo)[e4];
    }
    const float mean = a.mu[row], rs = a.rs[row];
    const DropKey dk = drop_key(a.seed, a.which);
    const float dscale = 1.0f / (1.0f - a.drop_p);
    float4 dyv[V4], xh[V4];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int q = 0; q < V4; ++q) {
      const int e4 = lane + 64 * q;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float dy = f4at(dyl[q], c);
        if (a.drop_p > 0.f) dy *= drop_u(dk, (uint64_t)row * L + 4 * e4 + c + a.drop_off) >= a.drop_p ? dscale : 0.0f;
        const float x = (f4at(ul[q], c) - mean) * rs;
        l4set(dyv[q], c, dy);
        l4set(xh[q], c, x);
        const float dxh = dy * f4at(gl[q], c);
        s1 += dxh;
        s2 += dxh * x;
        if (PART) {
          l4set(gp[q], c, dy * x);
          l4set(bp[q], c, dy);
        } else {
          if (a.gcontrib) a.gcontrib[(int64_t)row * L + 4 * e4 + c] = dy * x;
          if (a.bcontrib) a.bcontrib[(int64_t)row * L + 4 * e4 + c] = dy;
        }
      }
    }
    s1 = wave_sum(s1) / L;
    s2 = wave_sum(s2) / L;
#pragma unroll
    for (int q = 0; q < V4; ++q) {
      float4 d;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float t = rs * (f4at(dyv[q], c) * f4at(gl[q], c) - s1 - f4at(xh[q], c) * s2);
        if (a.beta != 0.f) t += a.beta * f4at(xin[q], c);
        l4set(d, c, t);
      }
      reinterpret_cast<float4*>(a.dx + xo)[lane + 64 * q] = d;
      if (PART) xp[q] = d;
    }
  }
  if constexpr (PART) {
    __shared__ float4 red[2][4][64 * V4];
#pragma unroll
    for (int q = 0; q < V4; ++q) {
      red[0][wv][lane + 64 * q] = gp[q];
      red[1][wv][lane + 64 * q] = bp[q];
    }
    __syncthreads();
    for (int e4 = threadIdx.x; e4 < L / 4; e4 += 256) {
      float4 g = red[0][0][e4], b = red[1][0][e4];
#pragma unroll
      for (int k = 1; k < 4; ++k) {
        const float4 g2 = red[0][k][e4], b2 = red[1][k][e4];
        g.x += g2.x; g.y += g2.y; g.z += g2.z; g.w += g2.w;
        b.x += b2.x; b.y += b2.y; b.z += b2.z; b.w += b2.w;
      }
      if (a.gpart) reinterpret_cast<float4*>(a.gpart + (int64_t)blockIdx.x * L)[e4] = g;
      if (a.bpart) reinterpret_cast<float4*>(a.bpart + (int64_t)blockIdx.x * L)[e4] = b;
    }
    if (a.xpart) {  // the dx sums through the same LDS rows (workgroup-uniform branch)
      __syncthreads();
#pragma unroll
      for (int q = 0; q < V4; ++q) red[0][wv][lane + 64 * q] = xp[q];
      __syncthreads();
      for (int e4 = threadIdx.x; e4 < L / 4; e4 += 256) {
        float4 x = red[0][0][e4];
#pragma unroll
        for (int k = 1; k < 4; ++k) {
          const float4 x2 = red[0][k][e4];
          x.x += x2.x; x.y += x2.y; x.z += x2.z; x.w += x2.w;
        }
        reinterpret_cast<float4*>(a.xpart + (int64_t)blockIdx.x * L)[e4] = x;
      }
    }
  }
}

// the float4 kernels' preconditions: L = 256 or 512 or 1024, unit element strides, every row
// base and pointer 16-B aligned (row maps with strides that are multiples of 4 floats)
static bool al16p(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static bool map4(const Idx2& m) { return m.s0 % 4 == 0 && m.s1 % 4 == 0; }
static bool ln_v4_env() {
  static const bool on = env_flag("DSTAGNN_LN_V4", true);  // default on
  return on;
}
static bool ln_fwd_v4_ok(const LnFwd& a) {
  if (!ln_v4_env() || (a.L != 256 && a.L != 512 && a.L != 1024) || a.yes != 1 || !map4(a.yrow)) return false;
  for (int s = 0; s < a.nsrc; ++s)
    if (a.src[s].es != 1 || !map4(a.src[s].row) || !al16p(a.src[s].p)) return false;
  return al16p(a.g) && al16p(a.b) && al16p(a.y) && al16p(a.u);
}
static bool ln_bwd_v4_ok(const LnBwd& a) {
  return ln_v4_env() && (a.L == 256 || a.L == 512 || a.L == 1024) && a.dyes == 1 && a.dxes == 1 && map4(a.dyrow) &&
         map4(a.dxrow) && al16p(a.dy) && al16p(a.u) && al16p(a.g) && al16p(a.dx) && al16p(a.gpart) &&
         al16p(a.bpart) && al16p(a.xpart);
}

// Long rows (L > 1024: the TAt / EmbedT LayerNorm over N nodes at GAMBIA N = 2139 and SYN
// N = 4096): a 256-thread WORKGROUP per row, element e = tid + 256 q (VPT <= 16 values per
// thread, all loads in one round as above), the sums over the row by a wave reduction and the
// four waves' partials through LDS in a fixed order.  The wave-per-row kernel needed 64 values
// per lane there (~210-256 VGPRs + AGPR spills of the gradient: one wave per SIMD, ~25 % of
// HBM bandwidth).
__device__ __forceinline__ float wg_sum4(float v, float* red4) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red4[w] = v;
  __syncthreads();
  const float t = (red4[0] + red4[1]) + (red4[2] + red4[3]);
  __syncthreads();  // red4 reused by the next reduction
  return t;
}

template <int VPT, int NSRC>
__global__ __launch_bounds__(256) void ln_fwd_wg_kernel(LnFwd a) {
  __shared__ float red4[4];
  const int tid = threadIdx.x, row = blockIdx.x, L = a.L;
  float xs[NSRC][VPT], gv[VPT], bv[VPT], v[VPT];
#pragma unroll
  for (int q = 0; q < VPT; ++q) {
    const int e = min(tid + 256 * q, L - 1);
#pragma unroll
    for (int s = 0; s < NSRC; ++s) xs[s][q] = a.src[s].p[ioff(a.src[s].row, row) + (int64_t)e * a.src[s].es];
    gv[q] = a.g[e];
    bv[q] = a.b[e];
  }
  float sum = 0.f;
#pragma unroll
  for (int q = 0; q < VPT; ++q) {
    float u = 0.f;
#pragma unroll
    for (int s = 0; s < NSRC; ++s) u += xs[s][q];
    v[q] = tid + 256 * q < L ? u : 0.f;
    sum += v[q];
  }
  const float mean = wg_sum4(sum, red4) / L;
  float var = 0.f;
#pragma unroll
  for (int q = 0; q < VPT; ++q)
    if (tid + 256 * q < L) { const float d = v[q] - mean; var += d * d; }
  var = wg_sum4(var, red4) / L;
  const float rs = rsqrtf(var + a.eps);
  if (tid == 0 && a.mu) { a.mu[row] = mean; a.rs[row] = rs; }  // (null: forward-only, a scalar branch)
  const int64_t yo = ioff(a.yrow, row);
#pragma unroll
  for (int q = 0; q < VPT; ++q) {
    const int e = tid + 256 * q;
    if (e >= L) continue;
    if (a.u) a.u[(int64_t)row * L + e] = v[q];
    float y = (v[q] - mean) * rs * gv[q] + bv[q];
    if (a.drop_p > 0.f) y *= drop_scale(a.seed, a.which, (uint64_t)row * L + e + a.drop_off, a.drop_p);
    a.y[yo + (int64_t)e * a.yes] = y;
  }
}

// backward of the above (per-element gamma / beta contributions: the partial-slab form needs
// L <= 1024)
template <int VPT>
__global__ __launch_bounds__(256) void ln_bwd_wg_kernel(LnBwd a) {
  __shared__ float red4[4];
  const int tid = threadIdx.x, row = blockIdx.x, L = a.L;
  const int64_t yo = ioff(a.dyrow, row), xo = ioff(a.dxrow, row);
  float dyl[VPT], ul[VPT], gl[VPT], xin[VPT];
#pragma unroll
  for (int q = 0; q < VPT; ++q) {
    const int e = min(tid + 256 * q, L - 1);
    dyl[q] = a.dy[yo + (int64_t)e * a.dyes];
    ul[q] = a.u[(int64_t)row * L + e];
    gl[q] = a.g[e];
    xin[q] = a.beta != 0.f ? a.dx[xo + (int64_t)e * a.dxes] : 0.f;
  }
  const float mean = a.mu[row], rs = a.rs[row];
  float dyv[VPT], xh[VPT], s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int q = 0; q < VPT; ++q) {
    const int e = tid + 256 * q;
    dyv[q] = 0.f; xh[q] = 0.f;
    if (e < L) {
      float dy = dyl[q];
      if (a.drop_p > 0.f) dy *= drop_scale(a.seed, a.which, (uint64_t)row * L + e + a.drop_off, a.drop_p);
      const float x = (ul[q] - mean) * rs;
      dyv[q] = dy; xh[q] = x;
      const float dxh = dy * gl[q];
      s1 += dxh; s2 += dxh * x;
      if (a.gcontrib) a.gcontrib[(int64_t)row * L + e] = dy * x;
      if (a.bcontrib) a.bcontrib[(int64_t)row * L + e] = dy;
    }
  }
  s1 = wg_sum4(s1, red4) / L;
  s2 = wg_sum4(s2, red4) / L;
#pragma unroll
  for (int q = 0; q < VPT; ++q) {
    const int e = tid + 256 * q;
    if (e >= L) continue;
    float dx = rs * (dyv[q] * gl[q] - s1 - xh[q] * s2);
    if (a.beta != 0.f) dx += a.beta * xin[q];
    a.dx[xo + (int64_t)e * a.dxes] = dx;
  }
}

// PART: gamma / beta gradient partial sums per workgroup instead of per-element contribution
// tensors: a wave takes kLnRowsPerWave consecutive rows, keeps the sums over them in
// registers, and the 4 waves combine through LDS into one row of the (blocks, L) slabs
// gpart / bpart (reduced over blocks by a column sum afterwards).  Cuts the (R, L) contribution
// write and its re-read.  Loads: one branch-free round per row, as ln_fwd_kernel.
template <int VPT, bool PART>
__global__ __launch_bounds__(256) void ln_bwd_kernel(LnBwd a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  constexpr int RPW = PART ? kLnRowsPerWave : 1;
  const int L = a.L;
  float gp[VPT], bp[VPT], xp[VPT];
#pragma unroll
  for (int q = 0; q < VPT; ++q) { gp[q] = 0.f; bp[q] = 0.f; xp[q] = 0.f; }
  for (int i = 0; i < RPW; ++i) {
    const int row = (blockIdx.x * 4 + wv) * RPW + i;
    if (row >= a.R) break;  // wave-uniform
    const int64_t yo = ioff(a.dyrow, row);
    constexpr bool PRE = VPT <= 16;  // long rows: gamma read at its use (register budget)
    float dyl[VPT], ul[VPT], gl[PRE ? VPT : 1], xin[VPT];
#pragma unroll
    for (int q = 0; q < VPT; ++q) {
      const int e = min(lane + 64 * q, L - 1);
      dyl[q] = a.dy[yo + (int64_t)e * a.dyes];
      ul[q] = a.u[(int64_t)row * L + e];
      if constexpr (PRE) gl[q] = a.g[e];
    }
    const int64_t xo = ioff(a.dxrow, row);
    if (a.beta != 0.f) {
#pragma unroll
      for (int q = 0; q < VPT; ++q) xin[q] = a.dx[xo + (int64_t)min(lane + 64 * q, L - 1) * a.dxes];
    }
    const float mean = a.mu[row], rs = a.rs[row];
    float dyv[VPT], xh[VPT];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int q = 0; q < VPT; ++q) {
      int e = lane + 64 * q;
      dyv[q] = 0.f; xh[q] = 0.f;
      if (e < L) {
        float dy = dyl[q];
        if (a.drop_p > 0.f) dy *= drop_scale(a.seed, a.which, (uint64_t)row * L + e + a.drop_off, a.drop_p);
        float x = (ul[q] - mean) * rs;
        dyv[q] = dy; xh[q] = x;
        float dxh = dy * (PRE ? gl[PRE ? q : 0] : a.g[e]);
        s1 += dxh; s2 += dxh * x;
        if (PART) {
          gp[q] += dy * x;
          bp[q] += dy;
        } else {
          if (a.gcontrib) a.gcontrib[(int64_t)row * L + e] = dy * x;
          if (a.bcontrib) a.bcontrib[(int64_t)row * L + e] = dy;
        }
      }
    }
    s1 = wave_sum(s1) / L;
    s2 = wave_sum(s2) / L;
#pragma unroll
    for (int q = 0; q < VPT; ++q) {
      int e = lane + 64 * q;
      if (e < L) {
        float dx = rs * (dyv[q] * (PRE ? gl[PRE ? q : 0] : a.g[e]) - s1 - xh[q] * s2);
        int64_t oo = xo + (int64_t)e * a.dxes;
        if (a.beta != 0.f) dx += a.beta * xin[q];
        a.dx[oo] = dx;
        if (PART) xp[q] += dx;
      }
    }
  }
  if constexpr (PART) {
    __shared__ float red[2][4][64 * VPT];
#pragma unroll
    for (int q = 0; q < VPT; ++q) {
      red[0][wv][lane + 64 * q] = gp[q];
      red[1][wv][lane + 64 * q] = bp[q];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < L; e += 256) {
      const float g = red[0][0][e] + red[0][1][e] + red[0][2][e] + red[0][3][e];
      const float b = red[1][0][e] + red[1][1][e] + red[1][2][e] + red[1][3][e];
      if (a.gpart) a.gpart[(int64_t)blockIdx.x * L + e] = g;
      if (a.bpart) a.bpart[(int64_t)blockIdx.x * L + e] = b;
    }
    if (a.xpart) {  // the dx sums through the same LDS rows (workgroup-uniform branch)
      __syncthreads();
#pragma unroll
      for (int q = 0; q < VPT; ++q) red[0][wv][lane + 64 * q] = xp[q];
      __syncthreads();
      for (int e = threadIdx.x; e < L; e += 256)
        a.xpart[(int64_t)blockIdx.x * L + e] = red[0][0][e] + red[0][1][e] + red[0][2][e] + red[0][3][e];
    }
  }
}

// =====================================================================================
// per-(device, stream) zero-armed ticket counters for single-launch reductions: kernels
// that take tickets re-arm them (write 0) before they finish, so consecutive launches on
// one stream can share them; different streams never do.
// =====================================================================================
}  // namespace

int* stream_counters(hipStream_t st, int n) {
  constexpr int kCounters = 1 << 16;
  if (n > kCounters) return nullptr;
  static std::mutex mu;
  static std::map<std::pair<int, hipStream_t>, int*> table;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  auto key = std::make_pair(dev, st);
  auto it = table.find(key);
  if (it != table.end()) return it->second;
  if (table.size() >= 256) return nullptr;
  int* p = nullptr;
  if (hipMalloc(&p, sizeof(int) * kCounters) != hipSuccess) return nullptr;
  if (hipMemsetAsync(p, 0, sizeof(int) * kCounters, st) != hipSuccess) {
    (void)hipFree(p);
    return nullptr;
  }
  table[key] = p;
  return p;
}

namespace {

// =====================================================================================
// reductions
// =====================================================================================
// Column sums of up to 4 same-shape sources in one launch pair (deterministic: fixed
// reduction order, no atomics).
// stage 1: each source viewed as (A, E) rows, E = O*I contiguous per row a.
// part[p][s*O + o] = sum over the p-th chunk of rows, sum_i in_s[a][o*I+i].
// Column sums land in LDS (colv[E], dynamic), then each output folds its I columns, so
// stage 2 reads a compact (P, nsrc*O) slab.  E <= 256: the block is R' = 256/E row-lanes x
// E columns (consecutive threads read consecutive addresses); E > 256: threads stride e.
__global__ __launch_bounds__(256) void colsum_stage1(ColsumArgs a) {
  extern __shared__ float colv[];
  __shared__ float red[256];
  const int E = a.O * a.I, OT = a.nsrc * a.O;
  const int p = blockIdx.x;
  const int64_t a0 = (int64_t)p * a.achunk, a1 = min(a.A, a0 + a.achunk);
  const int t = threadIdx.x;
  for (int src = 0; src < a.nsrc; ++src) {
    const float* __restrict__ in = a.in[src];
    if (E <= 256) {
      const int R = 256 / E;
      const int r = t / E, e = t % E;
      float sum = 0.f;
      if (r < R) {
#pragma unroll 8
        for (int64_t aa = a0 + r; aa < a1; aa += R) sum += in[aa * E + e];
      }
      red[t] = sum;
      __syncthreads();
      if (t < E) {
        float tot = 0.f;
        for (int q = 0; q < R; ++q) tot += red[q * E + t];
        colv[t] = tot;
      }
    } else {
      for (int e = t; e < E; e += 256) {
        float sum = 0.f;
#pragma unroll 8
        for (int64_t aa = a0; aa < a1; ++aa) sum += in[aa * E + e];
        colv[e] = sum;
      }
    }
    __syncthreads();
    for (int o = t; o < a.O; o += 256) {
      float sum = 0.f;
      for (int i = 0; i < a.I; ++i) sum += colv[o * a.I + i];
      a.part[(int64_t)p * OT + src * a.O + o] = sum;
    }
    __syncthreads();
  }
}
// stage 2: out_s[o] = beta*out_s[o] + sum_p part[p][s*O + o].  1024 threads = OL output
// lanes x PG row groups (coalesced along o), LDS tree over the groups (fixed order).
__global__ __launch_bounds__(1024) void colsum_stage2(ColsumArgs a) {
  __shared__ float red[1024];
  const int OT = a.nsrc * a.O;
  const int t = threadIdx.x;
  const int PG = 1024 / a.OL, g = t / a.OL, l = t % a.OL;
  const int o = blockIdx.x * a.OL + l;
  float sum = 0.f;
  if (o < OT) {
#pragma unroll 8
    for (int pp = g; pp < a.P; pp += PG) sum += a.part[(int64_t)pp * OT + o];
  }
  red[t] = sum;
  __syncthreads();
  for (int w = PG >> 1; w > 0; w >>= 1) {
    if (g < w) red[t] += red[t + w * a.OL];
    __syncthreads();
  }
  if (g == 0 && o < OT) {
    const int src = o / a.O, oo = o - src * a.O;
    float* d = a.out[src] + (int64_t)oo * a.ostride;
    *d = (a.beta != 0.f ? a.beta * *d : 0.f) + red[l];
  }
}

// -------------------------------------------------------------------------------------
// Single-launch column sums (deterministic).  Each source is an (A, E) row-major matrix.
// Columns: E <= 256 -> one group, RP = 256/E rows per block pass (thread t: column t % E,
// row lane t / E, so a pass reads RP*E consecutive floats); E > 256 -> groups of
// W = I*floor(256/I) columns, one row per pass.  Rows: R chunks (grid.x), ~1K blocks in
// total, 8 independent loads in flight per thread.  The cross-block sum is a two-level
// ticket tree (handoff.hpp): the last block of each run of 32 row chunks adds their partials
// (fixed order) into a level-2 partial; the last of those adds the <= 32 level-2 partials,
// folds each output's I columns and stores.  One launch, no float atomics.
// -------------------------------------------------------------------------------------
constexpr int kCsW = 256;   // partial width (columns)
constexpr int kCsL1 = 32;   // row chunks per level-1 ticket

struct Colsum2dArgs {
  const float* in[4] = {};
  float* out[4] = {};
  int nsrc = 1;
  int64_t A = 0; int O = 0, I = 1, E = 0;
  int W = 256, G = 1, RP = 1, R = 1, R2 = 1;  // group width, groups/source, rows per pass, chunks, level-2 count
  int64_t achunk = 1;
  int64_t ostride = 1; float beta = 0.f;
  float* part = nullptr;   // level 1: [nsrc*G][R][256], then level 2: [nsrc*G][R2][256]
  int* cnt = nullptr;      // [nsrc*G][R2] level-1 tickets, then [nsrc*G] level-2 tickets
};

__global__ __launch_bounds__(256) void colsum2d_kernel(Colsum2dArgs a) {
  __shared__ float red[kCsW];
  __shared__ int last;
  const int t = threadIdx.x;
  const int r = blockIdx.x, gidx = blockIdx.y;  // gidx = src * G + group
  const int src = gidx / a.G, grp = gidx - src * a.G;
  const float* __restrict__ in = a.in[src];
  const int64_t a0 = (int64_t)r * a.achunk, a1 = min(a.A, a0 + a.achunk);
  // thread -> (column, row lane)
  int col, lane;
  bool act;
  if (a.G == 1 && a.E <= kCsW) { col = t % a.E; lane = t / a.E; act = lane < a.RP; }
  else { col = grp * a.W + t; lane = 0; act = t < a.W && col < a.E; }
  float s0 = 0.f, s1 = 0.f;
  if (act) {
    const int RP = a.RP;
    int64_t aa = a0 + lane;
    for (; aa + 15 * RP < a1; aa += 16 * RP) {
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = in[(aa + (int64_t)u * RP) * a.E + col];
#pragma unroll
      for (int u = 0; u < 16; u += 2) { s0 += v[u]; s1 += v[u + 1]; }
    }
    for (; aa < a1; aa += RP) s0 += in[aa * a.E + col];
  }
  // fold the row lanes in fixed order: thread t holds column t % E of lane t / E (E <= 256)
  red[t] = act ? s0 + s1 : 0.f;
  __syncthreads();
  float colv = red[t];
  if (a.G == 1 && a.E <= kCsW) {
    colv = 0.f;
    if (t < a.E)
      for (int l = 0; l < a.RP; ++l) colv += red[l * a.E + t];
  }
  // the two-level hand-off (handoff.hpp): n1, R2 <= kCsL1 rows per sum
  float* p1 = a.part + ((int64_t)gidx * a.R + r) * kCsW;
  if (t < a.W) st_agent(p1 + t, colv);
  const int c1 = r / kCsL1;
  const int n1 = min(kCsL1, a.R - c1 * kCsL1);
  if (!last_arrival(a.cnt + (int64_t)gidx * a.R2 + c1, n1, &last)) return;
  float* p2 = a.part + ((int64_t)a.nsrc * a.G * a.R + (int64_t)gidx * a.R2 + c1) * kCsW;
  if (t < a.W)
    st_agent(p2 + t, sum_rows_agent<kCsL1>(a.part + ((int64_t)gidx * a.R + (int64_t)c1 * kCsL1) * kCsW + t, kCsW, n1));
  if (!last_arrival(a.cnt + (int64_t)a.nsrc * a.G * a.R2 + gidx, a.R2, &last)) return;
  red[t] = t < a.W ? sum_rows_agent<kCsL1>(a.part + ((int64_t)a.nsrc * a.G * a.R + (int64_t)gidx * a.R2) * kCsW + t,
                                           kCsW, a.R2)
                   : 0.f;
  __syncthreads();
  const int opg = a.W / a.I;
  if (t < opg) {
    const int o = grp * opg + t;
    if (o < a.O) {
      float v = 0.f;
      for (int i = 0; i < a.I; ++i) v += red[t * a.I + i];
      float* d = a.out[src] + (int64_t)o * a.ostride;
      *d = (a.beta != 0.f ? a.beta * *d : 0.f) + v;
    }
  }
}

// out[a][i] = beta*out + sum_m in[a][m][i]; grid (i blocks, a)
// out[a][i] = beta*out[a][i] + sum_m in[a][m][i]: a workgroup owns 32 consecutive i of one a;
// its 8 wave-quarters sum interleaved m (8-way parallel chains per output instead of one
// Mm-long chain), combined through LDS in a fixed order.
__global__ __launch_bounds__(256) void sum_middle_kernel(const float* __restrict__ in, int64_t A, int Mm, int64_t I,
                                                         float* __restrict__ out, float beta) {
  __shared__ float red[8][33];
  const int64_t a = blockIdx.y;
  const int il = threadIdx.x & 31, mg = threadIdx.x >> 5;
  const int64_t i = (int64_t)blockIdx.x * 32 + il;
  const float* src = in + a * Mm * I;
  float s = 0.f;
  if (i < I) {
#pragma unroll 4
    for (int m = mg; m < Mm; m += 8) s += src[(int64_t)m * I + i];
  }
  red[mg][il] = s;
  __syncthreads();
  if (mg == 0 && i < I) {
    float t = red[0][il];
#pragma unroll
    for (int g = 1; g < 8; ++g) t += red[g][il];
    float* d = out + a * I + i;
    *d = (beta != 0.f ? beta * *d : 0.f) + t;
  }
}

// the same sums with float4 columns (I % 4 == 0, 16-B aligned rows): a workgroup takes 256
// consecutive columns (64 lanes x 4), its 4 waves split the Mm rows, 8 row loads in flight per
// lane (the scalar kernel's 128-B row pieces ran at ~2 TB/s: sum_middle 5-6 us at PEMS08)
__global__ __launch_bounds__(256) void sum_middle4_kernel(const float* __restrict__ in, int64_t A, int Mm, int64_t I,
                                                          float* __restrict__ out, float beta) {
  __shared__ floatx4 red[4][64];
  const int64_t a = blockIdx.y;
  const int il = threadIdx.x & 63, mg = threadIdx.x >> 6;
  const int64_t i4 = (int64_t)blockIdx.x * 64 + il;  // float4 column
  const floatx4* src = reinterpret_cast<const floatx4*>(in + a * Mm * I);
  const int64_t I4 = I / 4;
  floatx4 s = {0.f, 0.f, 0.f, 0.f};
  if (i4 < I4) {
    int m = mg;
    for (; m + 28 < Mm; m += 32) {
      floatx4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = src[(int64_t)(m + 4 * u) * I4 + i4];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; m < Mm; m += 4) s += src[(int64_t)m * I4 + i4];
  }
  red[mg][il] = s;
  __syncthreads();
  if (mg == 0 && i4 < I4) {
    floatx4 t = ((red[0][il] + red[1][il]) + red[2][il]) + red[3][il];
    floatx4* d = reinterpret_cast<floatx4*>(out + a * I) + i4;
    if (beta != 0.f) t += beta * *d;
    *d = t;
  }
}

__global__ __launch_bounds__(256) void relu_mask_kernel(const float* __restrict__ g, const float* __restrict__ y,
                                                        float* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = y[i] > 0.f ? g[i] : 0.f;
}

// =====================================================================================
// Chebyshev spatial-attention softmax (column softmax over source node i)
// grid ceil(N/64)*B*K (see sm_tile), block 512 = 64 columns x 8 row groups
// =====================================================================================
constexpr int kSmG = 8;  // row groups per workgroup (64 columns x 8 groups = 512 threads)
constexpr int kSmCondN = 1024;  // N from which the softmax kernels load under the support only

// workgroup -> (column group, b, k) with b fastest: the B workgroups that share one
// (k, column group) tile of A_pa, M_k and T_k are dispatched together (round-robin over the
// XCDs, B/8 per XCD), so those tiles come from L2 instead of HBM once per batch element
__device__ __forceinline__ void sm_tile(const ChebSm& a, int* b, int* k, int* cg) {
  const int ncg = (a.N + 63) / 64;
  int id = blockIdx.x;
  *b = id % a.B; id /= a.B;
  *cg = id % ncg;
  *k = id / ncg;
}

// CL ("conditional loads"): read M_k (fwd) and P / dW (bwd) only under the A_pa / T_k
// support.  Pays at large N (HBM-bound passes over N^2 tiles); at small N (PEMS08, 170) the
// passes are latency chains and the dependent load costs more than the bytes it saves.
template <bool CL>
__global__ __launch_bounds__(512) void cheb_softmax_fwd_kernel(ChebSm a) {
  __shared__ float sm_m[kSmG][64], sm_l[kSmG][64];
  const int N = a.N;
  int b, k, cg;
  sm_tile(a, &b, &k, &cg);
  const int bk = b * a.K + k;
  const int cj = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int j = cg * 64 + cj;
  const float* S = a.S + (int64_t)bk * N * N;
  const float* Mk = a.mask[k];
  const float* Tk = a.cheb + (int64_t)k * N * N;
  // one pass: online column max and sum of exp (4 independent chains, loads batched)
  float m = -INFINITY, l = 0.f;
  if (j < N) {
    float m4[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, l4[4] = {0.f, 0.f, 0.f, 0.f};
    int i = g;
    for (; i + 3 * kSmG < N; i += 4 * kSmG) {
      float z[4], w[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t o = (int64_t)(i + u * kSmG) * N + j;
        z[u] = S[o];
        w[u] = a.apa[o];
      }
      float mv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) mv[u] = CL ? 0.f : Mk[(int64_t)(i + u * kSmG) * N + j];
#pragma unroll
      for (int u = 0; u < 4; ++u) {  // CL: M_k read only under the A_pa support
        if (CL) {
          if (w[u] != 0.f) z[u] += w[u] * Mk[(int64_t)(i + u * kSmG) * N + j];
        } else {
          z[u] += w[u] * mv[u];
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float mn = fmaxf(m4[u], z[u]);
        l4[u] = l4[u] * __expf(m4[u] - mn) + __expf(z[u] - mn);
        m4[u] = mn;
      }
    }
    for (; i < N; i += kSmG) {
      const int64_t o = (int64_t)i * N + j;
      const float w = a.apa[o];
      const float z = S[o] + (CL ? (w != 0.f ? w * Mk[o] : 0.f) : w * Mk[o]);
      const float mn = fmaxf(m4[0], z);
      l4[0] = l4[0] * __expf(m4[0] - mn) + __expf(z - mn);
      m4[0] = mn;
    }
    m = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
#pragma unroll
    for (int u = 0; u < 4; ++u) l += m4[u] == -INFINITY ? 0.f : l4[u] * __expf(m4[u] - m);
  }
  sm_m[g][cj] = m; sm_l[g][cj] = l;
  __syncthreads();
  float M = sm_m[0][cj];
#pragma unroll
  for (int q = 1; q < kSmG; ++q) M = fmaxf(M, sm_m[q][cj]);
  float L = 0.f;
#pragma unroll
  for (int q = 0; q < kSmG; ++q) L += sm_m[q][cj] == -INFINITY ? 0.f : sm_l[q][cj] * __expf(sm_m[q][cj] - M);
  const float inv = 1.f / L;
  if (j < N) {
    float* P = a.P + (int64_t)bk * N * N;
    float* W = a.W ? a.W + (int64_t)bk * N * N : nullptr;
#pragma unroll 2
    for (int i = g; i < N; i += kSmG) {
      const int64_t o = (int64_t)i * N + j;
      const float w = a.apa[o];
      const float z = S[o] + (CL ? (w != 0.f ? w * Mk[o] : 0.f) : w * Mk[o]);
      const float p = __expf(z - M) * inv;
      P[o] = p;
      if (W) W[o] = Tk[o] * p;
    }
  }
}

// dz = P * (T*dW - sum_i P*T*dW)   written to dz (may alias dW)
template <bool CL>
__global__ __launch_bounds__(512) void cheb_softmax_bwd_kernel(ChebSm a) {
  __shared__ float sm_c[kSmG][64];
  const int N = a.N;
  int b, k, cg;
  sm_tile(a, &b, &k, &cg);
  const int bk = b * a.K + k;
  const int cj = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int j = cg * 64 + cj;
  const float* P = a.P + (int64_t)bk * N * N;
  const float* dW = a.dW + (int64_t)bk * N * N;
  const float* Tk = a.cheb + (int64_t)k * N * N;
  float c = 0.f;
  if (j < N) {
    // dW is only defined where T_k is non-zero (the sparse path writes the support only,
    // no memset) and only needed there: T_k (shared by the batch, from L2) is read first and
    // P / dW only under its support, so a sparse graph costs one dense pass over P, not
    // three over P, T_k and dW.  Off-support garbage in dW never propagates.
    float c4[4] = {0.f, 0.f, 0.f, 0.f};
    int i = g;
    for (; i + 3 * kSmG < N; i += 4 * kSmG) {
      float tv[4], pv[4], dv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t o = (int64_t)(i + u * kSmG) * N + j;
        tv[u] = Tk[o];
        if (!CL) { pv[u] = P[o]; dv[u] = dW[o]; }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t o = (int64_t)(i + u * kSmG) * N + j;
        if (CL) {
          if (tv[u] != 0.f) c4[u] += P[o] * (tv[u] * dW[o]);
        } else {
          c4[u] += pv[u] * (tv[u] != 0.f ? tv[u] * dv[u] : 0.f);
        }
      }
    }
    for (; i < N; i += kSmG) {
      const int64_t o = (int64_t)i * N + j;
      const float t = Tk[o];
      if (t != 0.f) c4[0] += P[o] * (t * dW[o]);
    }
    c = (c4[0] + c4[1]) + (c4[2] + c4[3]);
  }
  sm_c[g][cj] = c;
  __syncthreads();
  c = 0.f;
#pragma unroll
  for (int q = 0; q < kSmG; ++q) c += sm_c[q][cj];
  if (j < N) {
    float* dz = a.dz + (int64_t)bk * N * N;
    int i = g;
    for (; i + kSmG < N; i += 2 * kSmG) {
      const int64_t o0 = (int64_t)i * N + j, o1 = o0 + (int64_t)kSmG * N;
      const float t0 = Tk[o0], t1 = Tk[o1], p0 = P[o0], p1 = P[o1];
      float w0, w1;
      if (CL) {
        w0 = t0 != 0.f ? t0 * dW[o0] : 0.f;
        w1 = t1 != 0.f ? t1 * dW[o1] : 0.f;
      } else {
        const float d0 = dW[o0], d1 = dW[o1];
        w0 = t0 != 0.f ? t0 * d0 : 0.f;
        w1 = t1 != 0.f ? t1 * d1 : 0.f;
      }
      dz[o0] = p0 * (w0 - c);
      dz[o1] = p1 * (w1 - c);
    }
    for (; i < N; i += kSmG) {
      const int64_t o = (int64_t)i * N + j;
      const float t = Tk[o];
      dz[o] = P[o] * ((t != 0.f ? t * dW[o] : 0.f) - c);
    }
  }
}

// dM_k[i][j] = A_pa[i][j] * sum_b dz[b][k][i][j]
__global__ __launch_bounds__(256) void cheb_mask_grad_kernel(ChebSm a) {
  const int64_t NN = (int64_t)a.N * a.N;
  const int k = blockIdx.y;
  float* out = a.dmask[k];
  for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < NN; o += (int64_t)gridDim.x * blockDim.x) {
    const float w = a.apa[o];
    float s = 0.f;
    if (w != 0.f) {  // dz is read only under the A_pa support (dM_k is 0 elsewhere)
#pragma unroll 8
      for (int b = 0; b < a.B; ++b) s += a.dz[((int64_t)b * a.K + k) * NN + o];
    }
    out[o] = w * s;
  }
}


__global__ __launch_bounds__(256) void pack_rows_kernel(PackRows a) {
  int r0 = 0;
  for (int q = 0; q < a.n; ++q) {
    const int64_t n = (int64_t)a.rows[q] * a.cols;
    const float* src = a.unpack ? a.src[0] + (int64_t)r0 * a.cols : a.src[q];
    float* dst = a.unpack ? a.dst[q] : a.dst[0] + (int64_t)r0 * a.cols;
    if (dst)
      for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] = src[i];
    r0 += a.rows[q];
  }
}

// blockIdx.y = segment; grid-stride over the segment's source elements
__global__ __launch_bounds__(256) void param_prep_kernel(ParamPrepK a) {
  const PrepSeg& g = a.seg[blockIdx.y];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < g.n; i += (int64_t)gridDim.x * 256) {
    if (g.kind == 8) {  // DESTINATION-indexed: src (R, p0) -> dst (R, p1) rows zero-padded to p1 >= p0
      const int64_t r = i / g.p1, c = i - r * g.p1;
      g.dst[g.dst_off + i] = c < g.p0 ? g.src[r * g.p0 + c] : 0.f;
      continue;
    }
    if (g.kind == 9) {  // DESTINATION-indexed zero-padded transpose: src (p3, p1) row-major;
      // dst row a, column b < p0 (row stride p2): src[b][a] where b < p3 and a < p1, else 0
      const int64_t ra = i / g.p0, cb = i - ra * g.p0;
      g.dst[g.dst_off + ra * g.p2 + cb] = (cb < g.p3 && ra < g.p1) ? g.src[cb * g.p1 + ra] : 0.f;
      continue;
    }
    const float v = g.src[i];
    int64_t o;
    switch (g.kind) {
      case 0: o = g.dst_off + i; break;
      case 1: {  // src (d, t, f) -> dst (d, f, t)
        const int64_t f = i % g.p0, r = i / g.p0, t = r % g.p1, d = r / g.p1;
        o = (d * g.p0 + f) * g.p1 + t;
        break;
      }
      case 2: {  // src (f, c) -> dst (f, k*C + c)
        const int64_t c = i % g.p0, f = i / g.p0;
        o = f * g.p1 + (int64_t)g.p2 * g.p0 + c;
        break;
      }
      case 3: {  // src (o, c, j) -> dst (o, j, c)
        const int64_t j = i % g.p1, r = i / g.p1, c = r % g.p0, oc = r / g.p0;
        o = (oc * g.p1 + j) * g.p0 + c;
        break;
      }
      case 7: {  // src (o, c, j) -> dst (j, c, o): the forward convolution's B operand, o fastest
        const int64_t j = i % g.p1, r = i / g.p1, c = r % g.p0, oc = r / g.p0;
        o = (j * g.p0 + c) * 2 * g.p0 + oc;
        break;
      }
      case 4: {  // src (o, c, j) -> dst (ks-1-j, o, c)
        const int64_t j = i % g.p1, r = i / g.p1, c = r % g.p0, oc = r / g.p0;
        o = ((g.p1 - 1 - j) * 2 * g.p0 + oc) * g.p0 + c;
        break;
      }
      case 5:  // elementwise product (A_pa o M_k: the reference's adj_pa.mul(mask[k]), :122)
        g.dst[i] = v * g.src2[i];
        continue;
      default:  // its transpose: (i, j) -> (j, i), N = p0
        o = (i % g.p0) * g.p0 + i / g.p0;
        g.dst[o] = v * g.src2[i];
        continue;
    }
    g.dst[o] = v;
  }
}


// =====================================================================================
// block tail: fcmy dropout, residual, ReLUs and LN over C (one thread per (b,n,t) row)
// =====================================================================================
// one workgroup per node (b,n): its C*T elements are contiguous in (B,N,C,T), so every
// pass is a coalesced sweep; the LN over C (stride T) goes through LDS.



// thcat[f][k*C + c] = theta_k[f][c]   (and the inverse for the gradients)
__global__ __launch_bounds__(256) void pack_theta_kernel(PackTheta a) {
  const int total = a.K * a.F * a.C;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int c = i % a.C, r = i / a.C, f = r % a.F, k = r / a.F;
    const int64_t cat = (int64_t)f * a.K * a.C + (int64_t)k * a.C + c;
    if (a.unpack) {
      if (a.dst[k]) a.dst[k][(int64_t)f * a.C + c] = a.cat_in[cat];
    } else {
      a.cat_out[cat] = a.src[k][(int64_t)f * a.C + c];
    }
  }
}

__global__ void dropout_mask_kernel(float* out, int64_t n, uint64_t seed, uint32_t which, float p, uint64_t off) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = drop_scale(seed, which, (uint64_t)i + off, p);
}

inline unsigned grid1d(int64_t n, int64_t cap = 8192) {
  int64_t b = cdiv64(n, 256);
  return (unsigned)std::max<int64_t>(1, std::min(b, cap));
}

}  // namespace

// =====================================================================================
// launchers
// =====================================================================================
int op_transpose(const float* in, float* out, int R, int Cc, int batch, int64_t in_bs, int64_t out_bs, float beta,
                 hipStream_t st) {
  dim3 grid((unsigned)cdiv64(Cc, 32), (unsigned)cdiv64(R, 32), (unsigned)batch);
  hipLaunchKernelGGL(transpose_kernel, grid, dim3(256), 0, st, in, out, R, Cc, in_bs, out_bs, beta);
  DS_CHECK_LAUNCH();
  return 0;
}

template <int VPT>
static void launch_ln_fwd(const LnFwd& a, dim3 grid, hipStream_t st) {
  if (a.nsrc == 1) hipLaunchKernelGGL((ln_fwd_kernel<VPT, 1>), grid, dim3(256), 0, st, a);
  else if (a.nsrc == 2) hipLaunchKernelGGL((ln_fwd_kernel<VPT, 2>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((ln_fwd_kernel<VPT, 3>), grid, dim3(256), 0, st, a);
}

int op_ln_fwd(const LnFwd& a, hipStream_t st) {
  if (a.nsrc < 1 || a.nsrc > 3 || a.L < 1) { set_last_error("ln_fwd: 1..3 sources, L >= 1"); return DSTAGNN_E_ARG; }
  // the statistics are kept together or (the forward-only block) not at all
  if ((a.mu == nullptr) != (a.rs == nullptr)) { set_last_error("ln_fwd: mu and rs must both be set or both null"); return DSTAGNN_E_ARG; }
  dim3 grid((unsigned)cdiv64(a.R, 4));
  if (ln_fwd_v4_ok(a)) {  // float4 rows
#define DS_LN4(V) \
    if (a.nsrc == 1) hipLaunchKernelGGL((ln_fwd_v4_kernel<V, 1>), grid, dim3(256), 0, st, a); \
    else if (a.nsrc == 2) hipLaunchKernelGGL((ln_fwd_v4_kernel<V, 2>), grid, dim3(256), 0, st, a); \
    else hipLaunchKernelGGL((ln_fwd_v4_kernel<V, 3>), grid, dim3(256), 0, st, a);
    if (a.L == 256) { DS_LN4(1) } else if (a.L == 512) { DS_LN4(2) } else { DS_LN4(4) }
#undef DS_LN4
    DS_CHECK_LAUNCH();
    return 0;
  }
  int vpt = (int)cdiv64(a.L, 64);
  if (vpt <= 1) launch_ln_fwd<1>(a, grid, st);
  else if (vpt <= 2) launch_ln_fwd<2>(a, grid, st);
  else if (vpt <= 4) launch_ln_fwd<4>(a, grid, st);
  else if (vpt <= 8) launch_ln_fwd<8>(a, grid, st);
  else if (vpt <= 16) launch_ln_fwd<16>(a, grid, st);
  else if (a.L <= 4096) {  // a workgroup per row (ln_fwd_wg_kernel)
    const dim3 g((unsigned)a.R);
    const int v = (int)cdiv64(a.L, 256);
#define DS_LNW(V) \
  if (a.nsrc == 1) hipLaunchKernelGGL((ln_fwd_wg_kernel<V, 1>), g, dim3(256), 0, st, a); \
  else if (a.nsrc == 2) hipLaunchKernelGGL((ln_fwd_wg_kernel<V, 2>), g, dim3(256), 0, st, a); \
  else hipLaunchKernelGGL((ln_fwd_wg_kernel<V, 3>), g, dim3(256), 0, st, a);
    if (v <= 8) { DS_LNW(8) } else { DS_LNW(16) }
#undef DS_LNW
  }
  else { set_last_error("ln_fwd: row too long"); return DSTAGNN_E_SHAPE; }
  DS_CHECK_LAUNCH();
  return 0;
}

int op_ln_bwd(const LnBwd& a, hipStream_t st) {
  int vpt = (int)cdiv64(a.L, 64);
  if (a.gpart || a.bpart || a.xpart) {
    if (!ln_bwd_partials_ok(a.L)) { set_last_error("ln_bwd: partial slabs need L <= 1024"); return DSTAGNN_E_SHAPE; }
    dim3 grid((unsigned)ln_bwd_part_blocks(a.R));
    if (kLnRowsPerWave == 1 && ln_bwd_v4_ok(a)) {  // float4 rows (one row per wave, as below)
      if (a.L == 256) hipLaunchKernelGGL((ln_bwd_v4_kernel<1, true>), grid, dim3(256), 0, st, a);
      else if (a.L == 512) hipLaunchKernelGGL((ln_bwd_v4_kernel<2, true>), grid, dim3(256), 0, st, a);
      else hipLaunchKernelGGL((ln_bwd_v4_kernel<4, true>), grid, dim3(256), 0, st, a);
      DS_CHECK_LAUNCH();
      return 0;
    }
    if (vpt <= 1) hipLaunchKernelGGL((ln_bwd_kernel<1, true>), grid, dim3(256), 0, st, a);
    else if (vpt <= 2) hipLaunchKernelGGL((ln_bwd_kernel<2, true>), grid, dim3(256), 0, st, a);
    else if (vpt <= 4) hipLaunchKernelGGL((ln_bwd_kernel<4, true>), grid, dim3(256), 0, st, a);
    else if (vpt <= 8) hipLaunchKernelGGL((ln_bwd_kernel<8, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((ln_bwd_kernel<16, true>), grid, dim3(256), 0, st, a);
    DS_CHECK_LAUNCH();
    return 0;
  }
  dim3 grid((unsigned)cdiv64(a.R, 4));
  if (vpt <= 1) hipLaunchKernelGGL((ln_bwd_kernel<1, false>), grid, dim3(256), 0, st, a);
  else if (vpt <= 2) hipLaunchKernelGGL((ln_bwd_kernel<2, false>), grid, dim3(256), 0, st, a);
  else if (vpt <= 4) hipLaunchKernelGGL((ln_bwd_kernel<4, false>), grid, dim3(256), 0, st, a);
  else if (vpt <= 8) hipLaunchKernelGGL((ln_bwd_kernel<8, false>), grid, dim3(256), 0, st, a);
  else if (vpt <= 16) hipLaunchKernelGGL((ln_bwd_kernel<16, false>), grid, dim3(256), 0, st, a);
  else if (a.L <= 4096) {
    if (a.L <= 2048) hipLaunchKernelGGL((ln_bwd_wg_kernel<8>), dim3((unsigned)a.R), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((ln_bwd_wg_kernel<16>), dim3((unsigned)a.R), dim3(256), 0, st, a);
  }
  else { set_last_error("ln_bwd: row too long"); return DSTAGNN_E_SHAPE; }
  DS_CHECK_LAUNCH();
  return 0;
}

// out_s[o*ostride] = beta*out_s + sum_{a<A, i<I} in_s[a][o][i],  s < nsrc <= 4
int op_colsum_multi(const float* const* ins, float* const* outs, int nsrc, int64_t A, int O, int I,
                    int64_t ostride, float beta, float* part, size_t part_floats, hipStream_t st) {
  const int E = O * I;
  if (nsrc < 1 || nsrc > 4) { set_last_error("colsum: 1..4 sources"); return DSTAGNN_E_ARG; }
  if (E > 16384) { set_last_error("colsum: O*I > 16384"); return DSTAGNN_E_SHAPE; }
  if (A <= 0 || O <= 0) return 0;
  constexpr int kCsBlocks = 256;
  if (I <= kCsW) {
    Colsum2dArgs c;
    for (int q = 0; q < nsrc; ++q) { c.in[q] = ins[q]; c.out[q] = outs[q]; }
    c.nsrc = nsrc; c.A = A; c.O = O; c.I = I; c.E = E;
    if (E <= kCsW) { c.W = E; c.G = 1; c.RP = kCsW / E; }
    else { c.W = I * (kCsW / I); c.G = (int)cdiv64(E, c.W); c.RP = 1; }
    const int64_t groups = (int64_t)nsrc * c.G;
    // ~512 blocks in total, >= 16 row passes per block, <= 1024 chunks (two ticket levels of 32)
    int64_t R = std::max<int64_t>(1, std::min<int64_t>(1024, cdiv64(kCsBlocks, groups)));
    R = std::min<int64_t>(R, std::max<int64_t>(1, A / (16 * c.RP)));
    c.achunk = cdiv64(A, R);
    c.R = (int)cdiv64(A, c.achunk);
    c.R2 = (int)cdiv64(c.R, kCsL1);
    c.ostride = ostride; c.beta = beta; c.part = part;
    int* cnt = stream_counters(st, (int)(groups * (c.R2 + 1)));
    if (cnt && (size_t)groups * (c.R + c.R2) * kCsW <= part_floats) {
      c.cnt = cnt;
      hipLaunchKernelGGL(colsum2d_kernel, dim3((unsigned)c.R, (unsigned)groups), dim3(256), 0, st, c);
      DS_CHECK_LAUNCH();
      return 0;
    }
  }
  ColsumArgs a;
  for (int q = 0; q < nsrc; ++q) { a.in[q] = ins[q]; a.out[q] = outs[q]; }
  a.nsrc = nsrc; a.A = A; a.O = O; a.I = I; a.ostride = ostride; a.beta = beta; a.part = part;
  // ~4K elements per stage-1 workgroup, at most 256 partial rows (stage 2's loop over
  // the partials is latency-bound: keep it short)
  int64_t P = std::max<int64_t>(1, std::min<int64_t>(256, cdiv64(A * E, 4096)));
  P = std::min<int64_t>(P, A);
  while (P > 1 && (size_t)P * nsrc * O > part_floats) P /= 2;
  if ((size_t)P * nsrc * O > part_floats) { set_last_error("colsum: scratch too small"); return DSTAGNN_E_SPACE; }
  a.achunk = cdiv64(A, P);
  a.P = (int)cdiv64(A, a.achunk);
  hipLaunchKernelGGL(colsum_stage1, dim3((unsigned)a.P), dim3(256), (size_t)E * sizeof(float), st, a);
  DS_CHECK_LAUNCH();
  const int OT = nsrc * O;
  a.OL = 1;
  while (a.OL < OT && a.OL < 64) a.OL <<= 1;
  hipLaunchKernelGGL(colsum_stage2, dim3((unsigned)cdiv64(OT, a.OL)), dim3(1024), 0, st, a);
  DS_CHECK_LAUNCH();
  return 0;
}
int op_colsum(const float* in, int64_t A, int O, int I, float* out, int64_t ostride, float beta, float* part,
              size_t part_floats, hipStream_t st) {
  return op_colsum_multi(&in, &out, 1, A, O, I, ostride, beta, part, part_floats, st);
}

int op_sum_middle(const float* in, int64_t A, int Mm, int64_t I, float* out, float beta, hipStream_t st) {
  if (A <= 0 || I <= 0) return 0;
  if (A > 65535) { set_last_error("sum_middle: A > 65535"); return DSTAGNN_E_SHAPE; }
  if (cdiv64(I, 32) > 0x7fffffff) { set_last_error("sum_middle: I too large"); return DSTAGNN_E_SHAPE; }
  if (I % 4 == 0 && reinterpret_cast<uintptr_t>(in) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0)
    hipLaunchKernelGGL(sum_middle4_kernel, dim3((unsigned)cdiv64(I / 4, 64), (unsigned)A), dim3(256), 0, st, in, A, Mm,
                       I, out, beta);
  else
    hipLaunchKernelGGL(sum_middle_kernel, dim3((unsigned)cdiv64(I, 32), (unsigned)A), dim3(256), 0, st, in, A, Mm, I,
                       out, beta);
  DS_CHECK_LAUNCH();
  return 0;
}

int op_relu_mask(const float* g, const float* y, float* out, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(relu_mask_kernel, dim3(grid1d(n)), dim3(256), 0, st, g, y, out, n);
  DS_CHECK_LAUNCH();
  return 0;
}

int op_cheb_softmax_fwd(const ChebSm& a, hipStream_t st) {
  dim3 grid((unsigned)(cdiv64(a.N, 64) * a.B * a.K));
  if (a.N >= kSmCondN) hipLaunchKernelGGL(cheb_softmax_fwd_kernel<true>, grid, dim3(64 * kSmG), 0, st, a);
  else hipLaunchKernelGGL(cheb_softmax_fwd_kernel<false>, grid, dim3(64 * kSmG), 0, st, a);
  DS_CHECK_LAUNCH();
  return 0;
}
int op_cheb_softmax_bwd(const ChebSm& a, hipStream_t st) {
  dim3 grid((unsigned)(cdiv64(a.N, 64) * a.B * a.K));
  if (a.N >= kSmCondN) hipLaunchKernelGGL(cheb_softmax_bwd_kernel<true>, grid, dim3(64 * kSmG), 0, st, a);
  else hipLaunchKernelGGL(cheb_softmax_bwd_kernel<false>, grid, dim3(64 * kSmG), 0, st, a);
  DS_CHECK_LAUNCH();
  return 0;
}
int op_cheb_mask_grad(const ChebSm& a, hipStream_t st) {
  dim3 grid(grid1d((int64_t)a.N * a.N, 1024), (unsigned)a.K);
  hipLaunchKernelGGL(cheb_mask_grad_kernel, grid, dim3(256), 0, st, a);
  DS_CHECK_LAUNCH();
  return 0;
}

int op_param_prep(const ParamPrep& a, hipStream_t st) {
  if (a.nseg <= 0) return 0;
  if (a.nseg > kPrepSegsHost) { set_last_error("param_prep: too many segments"); return DSTAGNN_E_ARG; }
  // chunks of kPrepSegs segments per launch (K >= 4 on the small-graph attention path needs
  // more: 2 K mask re-layouts + K Theta blocks beside the fixed ones)
  for (int q0 = 0; q0 < a.nseg; q0 += kPrepSegs) {
    ParamPrepK k;
    k.nseg = std::min(kPrepSegs, a.nseg - q0);
    int64_t mx = 1;
    for (int q = 0; q < k.nseg; ++q) {
      k.seg[q] = a.seg[q0 + q];
      mx = std::max<int64_t>(mx, k.seg[q].n);
    }
    hipLaunchKernelGGL(param_prep_kernel, dim3((unsigned)std::min<int64_t>(cdiv64(mx, 256), 256), (unsigned)k.nseg),
                       dim3(256), 0, st, k);
    DS_CHECK_LAUNCH();
  }
  return 0;
}
int op_pack_rows(const PackRows& a, hipStream_t st) {
  if (a.n < 1 || a.n > 8) { set_last_error("pack_rows: 1..8 matrices"); return DSTAGNN_E_ARG; }
  int64_t mx = 1;
  for (int q = 0; q < a.n; ++q) mx = std::max<int64_t>(mx, (int64_t)a.rows[q] * a.cols);
  hipLaunchKernelGGL(pack_rows_kernel, dim3((unsigned)std::min<int64_t>(cdiv64(mx, 256), 1024)), dim3(256), 0, st, a);
  DS_CHECK_LAUNCH();
  return 0;
}


int op_dropout_mask(float* out, int64_t n, uint64_t seed, uint32_t which, float p, uint64_t off, hipStream_t st) {
  hipLaunchKernelGGL(dropout_mask_kernel, dim3(grid1d(n)), dim3(256), 0, st, out, n, seed, which, p, off);
  DS_CHECK_LAUNCH();
  return 0;
}

int op_pack_theta(const PackTheta& a, hipStream_t st) {
  hipLaunchKernelGGL(pack_theta_kernel, dim3(grid1d((int64_t)a.K * a.F * a.C, 256)), dim3(256), 0, st, a);
  DS_CHECK_LAUNCH();
  return 0;
}
