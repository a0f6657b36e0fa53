// loss.hip — the two ends of a training step on the GPU (gfx950): the criterion
// (train_DSTAGNN_my.py:132 `nn.SmoothL1Loss()`, :156-157 loss + backward) with the masked
// variants the model family uses for series with gaps, and the test-set scores
// (lib/utils1.py:418-431: per-horizon MAE / RMSE / MAPE; lib/metrics.py:6-17 masked MAPE).
//
// On a (B, N, P) head output of ~65 k floats all of this is launch latency, so each is ONE launch:
//   loss_fwd_kernel      d = y - t in fp32, the per-element term in fp32, every add from the first
//                        one in fp64 (sum and valid count per thread; the wave butterfly; the four
//                        wave sums ((w0 + w1) + (w2 + w3))).  A workgroup's {sum, count} goes out
//                        sc1 and the workgroup whose ticket came last (handoff.hpp) adds all
//                        partials in one fixed order: lane l of its first wave takes partials l,
//                        l + 64, ... in index order, then the butterfly.  stat = {sum, count},
//                        loss = sum / count (0 when nothing is valid).  Same bits on every launch.
//   loss_bwd_kernel      dy = l'(d) * (gout / count) on valid entries, 0 elsewhere; count from the
//                        forward's stat and gout from device memory: no host sync.  Recomputes d.
//   metrics_accum_kernel (rows, P) predictions / targets -> a running (P, 4) fp64 table of
//                        sum |e|, sum e^2, sum |e / t| over t != null, count of t != null.  Thread
//                        rl P + p of the first (256 / P) P reads element row0 P + rl P + p
//                        (coalesced; its p never changes), keeps four fp64 sums, LDS folds them
//                        over rl in order, workgroups hand off as above and the last one adds the
//                        folded sums into the table.  No floating-point atomics anywhere.
//   metrics_masked_kernel (B, N, P) predictions / targets -> a running (P, 8) horizon table and an
//                        optional running (N, 8) node table of fp64 sums over the VALID entries
//                        (the criterion's is_valid): count, sum e, sum |e|, sum e^2, sum |e / t|
//                        over t != mape_null, its count, sum t, sum t^2.  A workgroup owns a strip
//                        of 256 / P nodes: thread nl P + p walks the samples of element (n0 + nl,
//                        p), LDS folds the strip over nl (per horizon: a partial handed off as
//                        above) and over p (per node: added straight into the node table, whose
//                        rows have one owning workgroup each).
//   pinball_fwd_kernel / pinball_bwd_kernel   the quantile (pinball) criterion of an (M, Q)
//                        prediction, q fastest, against an (M) target: loss_fwd / loss_bwd's plan
//                        over the M Q stream (element i: target i / Q, level i mod Q).
//   metrics_quantile_kernel (B, N, P, Q) predictions -> running (P, 2 + 3 Q) and optional
//                        (N, 2 + 3 Q) tables of the calibration sums (valid and crossing counts;
//                        per level the pinball sum, the count of t <= y_q, the sum of y_q), on
//                        metrics_masked_kernel's plan.
//
// A masked entry is selected out (never multiplied by zero): a NaN target under the NaN mask
// leaves the loss finite and its gradient entry exactly 0.  A NaN prediction at a valid entry makes
// the loss NaN (HipAdam's non-finite skip then sees a NaN gradient norm).
//
// Vector (16-byte) loads where every pointer of the launch is 16-byte aligned and the tile is
// whole; scalar loads otherwise (a batch slice y[b:b+bs] of a contiguous tensor is often not
// aligned; the last tile is usually partial).
#include <cmath>

#include "handoff.hpp"
#include "ops.hpp"

namespace {

constexpr int kLossThreads = 256, kLossPer = 16, kLossTile = kLossThreads * kLossPer;
constexpr int kLossMaxWg = 1024;  // beyond it a workgroup walks tiles w, w + grid, ...
constexpr int kMetThreads = 256, kMetPasses = 8, kMetMaxWg = 256, kMetMaxP = 256;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ bool is_valid(int mask, float null_val, float t) {
  return mask == DSTAGNN_MASK_NONE ? true : mask == DSTAGNN_MASK_NAN ? !(t != t) : t != null_val;
}

// the per-element term of d = y - t (fp32; at most three roundings with d's own)
__device__ __forceinline__ float loss_term(int kind, float b, float d) {
  const float a = fabsf(d);
  switch (kind) {
    case DSTAGNN_LOSS_SMOOTH_L1: return a < b ? 0.5f * d * d / b : a - 0.5f * b;
    case DSTAGNN_LOSS_HUBER: return a <= b ? 0.5f * d * d : b * (a - 0.5f * b);
    case DSTAGNN_LOSS_MAE: return a;
    default: return d * d;
  }
}

// its derivative; sign(0) = 0 and a NaN d stays NaN
__device__ __forceinline__ float loss_slope(int kind, float b, float d) {
  const float a = fabsf(d);
  const float s = d > 0.f ? 1.f : d < 0.f ? -1.f : d;
  switch (kind) {
    case DSTAGNN_LOSS_SMOOTH_L1: return a < b ? d / b : s;
    case DSTAGNN_LOSS_HUBER: return a <= b ? d : b * s;
    case DSTAGNN_LOSS_MAE: return s;
    default: return 2.f * d;
  }
}

__global__ __launch_bounds__(kLossThreads) void loss_fwd_kernel(dstagnn_loss_cfg cfg, int64_t n,
                                                               const float* __restrict__ y,
                                                               const float* __restrict__ tg, int vec,
                                                               double* __restrict__ part, int* ticket,
                                                               double* __restrict__ stat, float* __restrict__ loss) {
  __shared__ double ws[kLossThreads / 64], wc[kLossThreads / 64];
  __shared__ int last;
  const int t = threadIdx.x;
  double sum = 0.0, cnt = 0.0;
  for (int64_t base = (int64_t)blockIdx.x * kLossTile; base < n; base += (int64_t)gridDim.x * kLossTile) {
    float yv[kLossPer], tv[kLossPer];
    if (vec && base + kLossTile <= n) {  // (uniform) a whole tile: four 16-byte loads per tensor
      const float4* __restrict__ y4 = reinterpret_cast<const float4*>(y + base);
      const float4* __restrict__ t4 = reinterpret_cast<const float4*>(tg + base);
#pragma unroll
      for (int u = 0; u < kLossPer / 4; ++u) {
        const float4 a = y4[u * kLossThreads + t], b = t4[u * kLossThreads + t];
        yv[4 * u] = a.x, yv[4 * u + 1] = a.y, yv[4 * u + 2] = a.z, yv[4 * u + 3] = a.w;
        tv[4 * u] = b.x, tv[4 * u + 1] = b.y, tv[4 * u + 2] = b.z, tv[4 * u + 3] = b.w;
      }
#pragma unroll
      for (int u = 0; u < kLossPer; ++u)
        if (is_valid(cfg.mask_mode, cfg.null_val, tv[u])) {
          sum += (double)loss_term(cfg.kind, cfg.param, yv[u] - tv[u]);
          cnt += 1.0;
        }
    } else {
#pragma unroll
      for (int u = 0; u < kLossPer; ++u) {
        const int64_t i = base + t + (int64_t)kLossThreads * u;
        const bool ok = i < n;
        yv[u] = ok ? y[i] : 0.f;
        tv[u] = ok ? tg[i] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kLossPer; ++u) {
        const int64_t i = base + t + (int64_t)kLossThreads * u;
        if (i < n && is_valid(cfg.mask_mode, cfg.null_val, tv[u])) {
          sum += (double)loss_term(cfg.kind, cfg.param, yv[u] - tv[u]);
          cnt += 1.0;
        }
      }
    }
  }
  sum = wave_sum_f64(sum);
  cnt = wave_sum_f64(cnt);
  if ((t & 63) == 0) ws[t >> 6] = sum, wc[t >> 6] = cnt;
  __syncthreads();
  // the hand-off of handoff.hpp: {sum, count} per workgroup, every partial an 8-byte sc1 store
  if (t == 0) {
    st_agent(part + 2 * (int64_t)blockIdx.x, (ws[0] + ws[1]) + (ws[2] + ws[3]));
    st_agent(part + 2 * (int64_t)blockIdx.x + 1, (wc[0] + wc[1]) + (wc[2] + wc[3]));
  }
  if (!last_arrival(ticket, (int)gridDim.x, &last)) return;
  if (t >= 64) return;
  double a = 0.0, c = 0.0;
  for (int64_t k = t; k < (int64_t)gridDim.x; k += 64) {
    a += ld_agent(part + 2 * k);
    c += ld_agent(part + 2 * k + 1);
  }
  a = wave_sum_f64(a);
  c = wave_sum_f64(c);
  if (t == 0) {
    stat[0] = a;
    stat[1] = c;
    loss[0] = c > 0.0 ? (float)(a / c) : 0.f;
  }
}

__global__ __launch_bounds__(kLossThreads) void loss_bwd_kernel(dstagnn_loss_cfg cfg, int64_t n,
                                                               const float* __restrict__ y,
                                                               const float* __restrict__ tg, int vec,
                                                               const double* __restrict__ stat,
                                                               const float* __restrict__ gout, float* __restrict__ dy) {
  const int t = threadIdx.x;
  const double cnt = stat[1];
  const float g = gout != nullptr ? gout[0] : 1.f;
  const float scale = cnt > 0.0 ? (float)((double)g / cnt) : 0.f;
  const int64_t base = (int64_t)blockIdx.x * kLossTile;
  if (vec && base + kLossTile <= n) {
    const float4* __restrict__ y4 = reinterpret_cast<const float4*>(y + base);
    const float4* __restrict__ t4 = reinterpret_cast<const float4*>(tg + base);
    float4* __restrict__ d4 = reinterpret_cast<float4*>(dy + base);
    float4 a[kLossPer / 4], b[kLossPer / 4];
#pragma unroll
    for (int u = 0; u < kLossPer / 4; ++u) a[u] = y4[u * kLossThreads + t], b[u] = t4[u * kLossThreads + t];
#pragma unroll
    for (int u = 0; u < kLossPer / 4; ++u) {
      float4 r;
      r.x = is_valid(cfg.mask_mode, cfg.null_val, b[u].x) ? loss_slope(cfg.kind, cfg.param, a[u].x - b[u].x) * scale : 0.f;
      r.y = is_valid(cfg.mask_mode, cfg.null_val, b[u].y) ? loss_slope(cfg.kind, cfg.param, a[u].y - b[u].y) * scale : 0.f;
      r.z = is_valid(cfg.mask_mode, cfg.null_val, b[u].z) ? loss_slope(cfg.kind, cfg.param, a[u].z - b[u].z) * scale : 0.f;
      r.w = is_valid(cfg.mask_mode, cfg.null_val, b[u].w) ? loss_slope(cfg.kind, cfg.param, a[u].w - b[u].w) * scale : 0.f;
      d4[u * kLossThreads + t] = r;
    }
    return;
  }
  float yv[kLossPer], tv[kLossPer];
#pragma unroll
  for (int u = 0; u < kLossPer; ++u) {
    const int64_t i = base + t + (int64_t)kLossThreads * u;
    const bool ok = i < n;
    yv[u] = ok ? y[i] : 0.f;
    tv[u] = ok ? tg[i] : 0.f;
  }
#pragma unroll
  for (int u = 0; u < kLossPer; ++u) {
    const int64_t i = base + t + (int64_t)kLossThreads * u;
    if (i < n)
      dy[i] = is_valid(cfg.mask_mode, cfg.null_val, tv[u]) ? loss_slope(cfg.kind, cfg.param, yv[u] - tv[u]) * scale : 0.f;
  }
}

__global__ __launch_bounds__(kMetThreads) void metrics_accum_kernel(int64_t n, int P, const float* __restrict__ pred,
                                                                   const float* __restrict__ tg, float null_val,
                                                                   int nan_mode, double* __restrict__ part,
                                                                   int* ticket, double* __restrict__ table) {
  __shared__ double red[4][kMetThreads];
  __shared__ int last;
  const int t = threadIdx.x;
  const int RL = kMetThreads / P, A = RL * P;  // rows per pass, threads that read
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if (t < A) {
    // a pass is RL whole rows = A contiguous floats; workgroup w takes passes w, w + grid, ...
    // (e0 is a multiple of P: this thread's horizon is t % P in every pass)
    for (int64_t e0 = (int64_t)blockIdx.x * A; e0 < n; e0 += (int64_t)gridDim.x * A) {
      const int64_t i = e0 + t;
      if (i < n) {
        const float pv = pred[i], tv = tg[i];
        const float e = pv - tv;
        s[0] += (double)fabsf(e);
        s[1] += (double)(e * e);
        if (nan_mode ? !(tv != tv) : tv != null_val) {
          s[2] += (double)fabsf(e / tv);
          s[3] += 1.0;
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) red[c][t] = s[c];
  __syncthreads();
  // fold over the rows of equal horizon in row order; item = c P + p
  const int items = 4 * P;
  for (int item = t; item < items; item += kMetThreads) {
    const int c = item / P, p = item - c * P;
    double a = 0.0;
    for (int rl = 0; rl < RL; ++rl) a += red[c][rl * P + p];
    st_agent(part + (int64_t)blockIdx.x * items + item, a);
  }
  if (!last_arrival(ticket, (int)gridDim.x, &last)) return;
  for (int item = t; item < items; item += kMetThreads) {
    const int c = item / P, p = item - c * P;
    double a = 0.0;
    for (int64_t k = 0; k < (int64_t)gridDim.x; ++k) a += ld_agent(part + k * items + item);
    table[p * 4 + c] += a;  // launches on one stream are ordered: the running table needs no atomics
  }
}

constexpr int kMmThreads = 256, kMmCols = 8, kMmUnroll = 4, kMmFold = 8;

// one entry into a thread's eight sums: e, e * e and e / t in fp32, every add in fp64; t and t * t
// as doubles (the product of two floats is exact there)
__device__ __forceinline__ void masked_entry(double (&s)[kMmCols], int mask, float null_val, float mape_null,
                                             float pv, float tv) {
  if (!is_valid(mask, null_val, tv)) return;  // selected out: a NaN target never reaches a sum
  const float e = pv - tv;
  s[0] += 1.0;
  s[1] += (double)e;
  s[2] += (double)fabsf(e);
  s[3] += (double)(e * e);
  if (tv != mape_null) {
    s[4] += (double)fabsf(e / tv);
    s[5] += 1.0;
  }
  s[6] += (double)tv;
  s[7] += (double)tv * (double)tv;
}

__global__ __launch_bounds__(kMmThreads) void metrics_masked_kernel(int B, int N, int P,
                                                                   const float* __restrict__ pred,
                                                                   const float* __restrict__ tg, int mask,
                                                                   float null_val, float mape_null,
                                                                   double* __restrict__ part, int* ticket,
                                                                   double* __restrict__ htable,
                                                                   double* __restrict__ ntable) {
  __shared__ double red[kMmCols][kMmThreads];
  __shared__ int last;
  const int t = threadIdx.x;
  const int TN = kMmThreads / P;                   // nodes of a whole strip
  const int n0 = (int)blockIdx.x * TN;             // (the grid is ceil(N / TN): n0 < N)
  const int tn = N - n0 < TN ? N - n0 : TN;        // nodes of this strip (the last one is partial)
  double s[kMmCols] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (t < tn * P) {
    // element (b, n0 + nl, p) with t = nl P + p sits at b N P + n0 P + t: for a fixed b the strip
    // reads tn P contiguous floats
    const int64_t step = (int64_t)N * P;
    const float* __restrict__ pp = pred + (int64_t)n0 * P + t;
    const float* __restrict__ tp = tg + (int64_t)n0 * P + t;
    int b = 0;
    for (; b + kMmUnroll <= B; b += kMmUnroll) {  // the loads of kMmUnroll samples in flight together
      float pv[kMmUnroll], tv[kMmUnroll];
#pragma unroll
      for (int u = 0; u < kMmUnroll; ++u) pv[u] = pp[(b + u) * step], tv[u] = tp[(b + u) * step];
#pragma unroll
      for (int u = 0; u < kMmUnroll; ++u) masked_entry(s, mask, null_val, mape_null, pv[u], tv[u]);
    }
    for (; b < B; ++b) masked_entry(s, mask, null_val, mape_null, pp[b * step], tp[b * step]);
  }
#pragma unroll
  for (int c = 0; c < kMmCols; ++c) red[c][t] = s[c];
  __syncthreads();
  // per node, over p in order: item = nl 8 + c lands on ntable[(n0 + nl) 8 + c].  This workgroup is
  // the only one that ever touches these rows and launches on a stream are ordered: plain adds.
  if (ntable != nullptr) {
    for (int item = t; item < kMmCols * tn; item += kMmThreads) {
      const int nl = item / kMmCols, c = item - nl * kMmCols;
      double a = 0.0;
      for (int p = 0; p < P; ++p) a += red[c][nl * P + p];
      ntable[(int64_t)n0 * kMmCols + item] += a;
    }
  }
  // per horizon, over nl in order (the idle rows of a partial strip hold zeros); item = c P + p
  const int items = kMmCols * P;
  for (int item = t; item < items; item += kMmThreads) {
    const int c = item / P, p = item - c * P;
    double a = 0.0;
    for (int nl = 0; nl < TN; ++nl) a += red[c][nl * P + p];
    st_agent(part + (int64_t)blockIdx.x * items + item, a);
  }
  if (!last_arrival(ticket, (int)gridDim.x, &last)) return;
  // the last arrival: the partials in workgroup order, kMmFold sc1 loads issued before their adds
  const int G = (int)gridDim.x;
  for (int item = t; item < items; item += kMmThreads) {
    const int c = item / P, p = item - c * P;
    double a = 0.0;
    for (int k0 = 0; k0 < G; k0 += kMmFold) {
      double u[kMmFold];
#pragma unroll
      for (int k = 0; k < kMmFold; ++k) u[k] = k0 + k < G ? ld_agent(part + (int64_t)(k0 + k) * items + item) : 0.0;
#pragma unroll
      for (int k = 0; k < kMmFold; ++k) a += u[k];
    }
    htable[p * kMmCols + c] += a;
  }
}

// ---- quantile forecasts: the pinball criterion and the calibration sums -----------------------
// Prediction (M, Q), q fastest; target (M).  Element i of the prediction stream belongs to target
// i / Q and level i mod Q: the stream itself is read as loss_fwd_kernel reads y (consecutive lanes,
// consecutive floats; 16-byte loads on whole aligned tiles), the target through the cache (Q
// neighbouring lanes share one).  The levels sit in LDS: tau and 1 - tau, both formed on the host.
constexpr int kMaxQ = DSTAGNN_MAX_QUANTILES;
struct PinballArgs {  // a checked dstagnn_pinball_cfg and the 1 - tau of its levels
  int mask_mode;
  float null_val;
  int num_quantiles;
  float tau[kMaxQ], one_minus_tau[kMaxQ];
};

// term and slope of d = y_q - t: d > 0: (1 - tau) d, slope 1 - tau; d < 0: tau (-d), slope -tau;
// d = 0: 0 and 0 (DSTAGNN_LOSS_MAE's sign(0) = 0); a NaN d stays NaN
__device__ __forceinline__ float pinball_term(float tau, float omt, float d) {
  return d > 0.f ? omt * d : d < 0.f ? tau * -d : d == 0.f ? 0.f : d;
}
__device__ __forceinline__ float pinball_slope(float tau, float omt, float d) {
  return d > 0.f ? omt : d < 0.f ? -tau : d == 0.f ? 0.f : d;
}

// (target index, level) of the four stream elements i0 .. i0 + 3
__device__ __forceinline__ void pinball_walk(unsigned i0, unsigned Q, unsigned (&m)[4], unsigned (&q)[4]) {
  m[0] = i0 / Q;
  q[0] = i0 - m[0] * Q;
#pragma unroll
  for (int j = 1; j < 4; ++j) {
    const bool wrap = q[j - 1] + 1 == Q;
    q[j] = wrap ? 0u : q[j - 1] + 1;
    m[j] = m[j - 1] + (wrap ? 1u : 0u);
  }
}

__global__ __launch_bounds__(kLossThreads) void pinball_fwd_kernel(PinballArgs cfg, int64_t n,
                                                                  const float* __restrict__ y,
                                                                  const float* __restrict__ tg, int vec,
                                                                  double* __restrict__ part, int* ticket,
                                                                  double* __restrict__ stat,
                                                                  float* __restrict__ loss) {
  __shared__ double ws[kLossThreads / 64], wc[kLossThreads / 64];
  __shared__ float tau[kMaxQ], omt[kMaxQ];
  __shared__ int last;
  const int t = threadIdx.x;
  const unsigned Q = (unsigned)cfg.num_quantiles;
  if (t < kMaxQ) tau[t] = cfg.tau[t], omt[t] = cfg.one_minus_tau[t];
  __syncthreads();
  double sum = 0.0, cnt = 0.0;  // cnt counts stream elements: Q per valid target entry
  for (int64_t base = (int64_t)blockIdx.x * kLossTile; base < n; base += (int64_t)gridDim.x * kLossTile) {
    if (vec && base + kLossTile <= n) {  // (uniform) a whole tile: four 16-byte loads of y
      const float4* __restrict__ y4 = reinterpret_cast<const float4*>(y + base);
      float4 a[kLossPer / 4];
#pragma unroll
      for (int u = 0; u < kLossPer / 4; ++u) a[u] = y4[u * kLossThreads + t];
#pragma unroll
      for (int u = 0; u < kLossPer / 4; ++u) {
        unsigned m[4], q[4];
        pinball_walk((unsigned)base + 4u * (unsigned)(u * kLossThreads + t), Q, m, q);
        const float yv[4] = {a[u].x, a[u].y, a[u].z, a[u].w};
        float tv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) tv[j] = tg[m[j]];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (is_valid(cfg.mask_mode, cfg.null_val, tv[j])) {
            sum += (double)pinball_term(tau[q[j]], omt[q[j]], yv[j] - tv[j]);
            cnt += 1.0;
          }
      }
    } else {
      float yv[kLossPer], tv[kLossPer];
      unsigned qv[kLossPer];
#pragma unroll
      for (int u = 0; u < kLossPer; ++u) {
        const int64_t i = base + t + (int64_t)kLossThreads * u;
        const bool ok = i < n;
        const unsigned m = ok ? (unsigned)i / Q : 0u;
        qv[u] = ok ? (unsigned)i - m * Q : 0u;
        yv[u] = ok ? y[i] : 0.f;
        tv[u] = ok ? tg[m] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kLossPer; ++u) {
        const int64_t i = base + t + (int64_t)kLossThreads * u;
        if (i < n && is_valid(cfg.mask_mode, cfg.null_val, tv[u])) {
          sum += (double)pinball_term(tau[qv[u]], omt[qv[u]], yv[u] - tv[u]);
          cnt += 1.0;
        }
      }
    }
  }
  sum = wave_sum_f64(sum);
  cnt = wave_sum_f64(cnt);
  if ((t & 63) == 0) ws[t >> 6] = sum, wc[t >> 6] = cnt;
  __syncthreads();
  if (t == 0) {  // the hand-off of handoff.hpp, as loss_fwd_kernel
    st_agent(part + 2 * (int64_t)blockIdx.x, (ws[0] + ws[1]) + (ws[2] + ws[3]));
    st_agent(part + 2 * (int64_t)blockIdx.x + 1, (wc[0] + wc[1]) + (wc[2] + wc[3]));
  }
  if (!last_arrival(ticket, (int)gridDim.x, &last)) return;
  if (t >= 64) return;
  double a = 0.0, c = 0.0;
  for (int64_t k = t; k < (int64_t)gridDim.x; k += 64) {
    a += ld_agent(part + 2 * k);
    c += ld_agent(part + 2 * k + 1);
  }
  a = wave_sum_f64(a);
  c = wave_sum_f64(c);
  if (t == 0) {
    stat[0] = a;
    stat[1] = c / (double)Q;  // the valid target entries (c is a multiple of Q: exact)
    loss[0] = c > 0.0 ? (float)(a / c) : 0.f;
  }
}

__global__ __launch_bounds__(kLossThreads) void pinball_bwd_kernel(PinballArgs cfg, int64_t n,
                                                                  const float* __restrict__ y,
                                                                  const float* __restrict__ tg, int vec,
                                                                  const double* __restrict__ stat,
                                                                  const float* __restrict__ gout,
                                                                  float* __restrict__ dy) {
  __shared__ float tau[kMaxQ], omt[kMaxQ];
  const int t = threadIdx.x;
  const unsigned Q = (unsigned)cfg.num_quantiles;
  if (t < kMaxQ) tau[t] = cfg.tau[t], omt[t] = cfg.one_minus_tau[t];
  __syncthreads();
  const double cnt = stat[1] * (double)Q;
  const float g = gout != nullptr ? gout[0] : 1.f;
  const float scale = cnt > 0.0 ? (float)((double)g / cnt) : 0.f;
  const int64_t base = (int64_t)blockIdx.x * kLossTile;
  if (vec && base + kLossTile <= n) {
    const float4* __restrict__ y4 = reinterpret_cast<const float4*>(y + base);
    float4* __restrict__ d4 = reinterpret_cast<float4*>(dy + base);
    float4 a[kLossPer / 4];
#pragma unroll
    for (int u = 0; u < kLossPer / 4; ++u) a[u] = y4[u * kLossThreads + t];
#pragma unroll
    for (int u = 0; u < kLossPer / 4; ++u) {
      unsigned m[4], q[4];
      pinball_walk((unsigned)base + 4u * (unsigned)(u * kLossThreads + t), Q, m, q);
      const float yv[4] = {a[u].x, a[u].y, a[u].z, a[u].w};
      float tv[4], r[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) tv[j] = tg[m[j]];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float s = pinball_slope(tau[q[j]], omt[q[j]], yv[j] - tv[j]);
        r[j] = is_valid(cfg.mask_mode, cfg.null_val, tv[j]) && s != 0.f ? s * scale : 0.f;
      }
      d4[u * kLossThreads + t] = make_float4(r[0], r[1], r[2], r[3]);
    }
    return;
  }
  float yv[kLossPer], tv[kLossPer];
  unsigned qv[kLossPer];
#pragma unroll
  for (int u = 0; u < kLossPer; ++u) {
    const int64_t i = base + t + (int64_t)kLossThreads * u;
    const bool ok = i < n;
    const unsigned m = ok ? (unsigned)i / Q : 0u;
    qv[u] = ok ? (unsigned)i - m * Q : 0u;
    yv[u] = ok ? y[i] : 0.f;
    tv[u] = ok ? tg[m] : 0.f;
  }
#pragma unroll
  for (int u = 0; u < kLossPer; ++u) {
    const int64_t i = base + t + (int64_t)kLossThreads * u;
    if (i < n) {
      const float s = pinball_slope(tau[qv[u]], omt[qv[u]], yv[u] - tv[u]);
      dy[i] = is_valid(cfg.mask_mode, cfg.null_val, tv[u]) && s != 0.f ? s * scale : 0.f;
    }
  }
}

// The calibration sums of (B, N, P, Q) predictions against (B, N, P) targets: metrics_masked_kernel's
// shape (a workgroup owns a strip of 256 / P nodes, thread nl P + p walks the samples of element
// (n0 + nl, p)) with 2 + 3 Q sums per thread: valid count, crossing count and, per level, the pinball
// sum (fp32 term), the count of t <= y_q (fp32 compare) and the sum of y_q (exact as doubles).
// A thread reads the Q floats of its entry (the wave: 64 Q contiguous floats, every byte used) and
// keeps its sums in registers; the loops over q are unrolled to kMaxQ under the uniform q < Q so
// every index is a constant.  The LDS folds go kQmChunk columns at a time.
constexpr int kQmThreads = 256, kQmCols = 2 + 3 * kMaxQ, kQmChunk = 8, kQmFold = 8;

__global__ __launch_bounds__(kQmThreads) void metrics_quantile_kernel(int B, int N, int P, PinballArgs cfg,
                                                                     const float* __restrict__ pred,
                                                                     const float* __restrict__ tg,
                                                                     double* __restrict__ part, int* ticket,
                                                                     double* __restrict__ htable,
                                                                     double* __restrict__ ntable) {
  __shared__ double red[kQmChunk][kQmThreads];
  __shared__ int last;
  const int t = threadIdx.x;
  const int Q = cfg.num_quantiles, cols = 2 + 3 * Q;
  const int TN = kQmThreads / P;
  const int n0 = (int)blockIdx.x * TN;       // (the grid is ceil(N / TN): n0 < N)
  const int tn = N - n0 < TN ? N - n0 : TN;  // nodes of this strip
  double s[kQmCols];
#pragma unroll
  for (int c = 0; c < kQmCols; ++c) s[c] = 0.0;
  if (t < tn * P) {
    const int64_t step = (int64_t)N * P;
    const float* __restrict__ tp = tg + (int64_t)n0 * P + t;
    const float* __restrict__ pp = pred + ((int64_t)n0 * P + t) * Q;
    for (int b = 0; b < B; ++b) {
      const float tv = tp[b * step];
      float yv[kMaxQ];
#pragma unroll
      for (int q = 0; q < kMaxQ; ++q) yv[q] = q < Q ? pp[b * step * Q + q] : 0.f;
      if (!is_valid(cfg.mask_mode, cfg.null_val, tv)) continue;  // selected out
      bool cross = false;
#pragma unroll
      for (int q = 0; q < kMaxQ; ++q)
        if (q < Q) {
          s[2 + 3 * q] += (double)pinball_term(cfg.tau[q], cfg.one_minus_tau[q], yv[q] - tv);
          s[3 + 3 * q] += tv <= yv[q] ? 1.0 : 0.0;
          s[4 + 3 * q] += (double)yv[q];
          if (q > 0) cross = cross || yv[q] < yv[q - 1];
        }
      s[0] += 1.0;
      s[1] += cross ? 1.0 : 0.0;
    }
  }
  const int items = cols * P;  // of a workgroup's horizon partial; item = c P + p
#pragma unroll
  for (int c0 = 0; c0 < kQmCols; c0 += kQmChunk) {
    if (c0 >= cols) break;  // (uniform)
    __syncthreads();        // the previous chunk's readers are done
#pragma unroll
    for (int j = 0; j < kQmChunk; ++j) {
      const int c = c0 + j;  // (a constant once unrolled)
      red[j][t] = c < kQmCols ? s[c < kQmCols ? c : 0] : 0.0;
    }
    __syncthreads();
    const int cw = cols - c0 < kQmChunk ? cols - c0 : kQmChunk;  // columns of this chunk
    // per node, over p in order; this workgroup is the only one that ever touches these rows
    if (ntable != nullptr) {
      for (int item = t; item < cw * tn; item += kQmThreads) {
        const int nl = item / cw, j = item - nl * cw;
        double a = 0.0;
        for (int p = 0; p < P; ++p) a += red[j][nl * P + p];
        ntable[(int64_t)(n0 + nl) * cols + c0 + j] += a;
      }
    }
    // per horizon, over nl in order (the idle rows of a partial strip hold zeros)
    for (int item = t; item < cw * P; item += kQmThreads) {
      const int j = item / P, p = item - j * P;
      double a = 0.0;
      for (int nl = 0; nl < TN; ++nl) a += red[j][nl * P + p];
      st_agent(part + (int64_t)blockIdx.x * items + (c0 + j) * P + p, a);
    }
  }
  if (!last_arrival(ticket, (int)gridDim.x, &last)) return;
  const int G = (int)gridDim.x;
  for (int item = t; item < items; item += kQmThreads) {
    const int c = item / P, p = item - c * P;
    double a = 0.0;
    for (int k0 = 0; k0 < G; k0 += kQmFold) {
      double u[kQmFold];
#pragma unroll
      for (int k = 0; k < kQmFold; ++k) u[k] = k0 + k < G ? ld_agent(part + (int64_t)(k0 + k) * items + item) : 0.0;
#pragma unroll
      for (int k = 0; k < kQmFold; ++k) a += u[k];
    }
    htable[p * cols + c] += a;
  }
}

int64_t loss_grid(int64_t n) {
  const int64_t tiles = (n + kLossTile - 1) / kLossTile;
  return tiles < 1 ? 1 : tiles > kLossMaxWg ? kLossMaxWg : tiles;
}

int64_t metrics_grid(int64_t rows, int P) {
  const int64_t per = (int64_t)(kMetThreads / P) * kMetPasses;  // rows per workgroup before the cap
  const int64_t g = (rows + per - 1) / per;
  return g < 1 ? 1 : g > kMetMaxWg ? kMetMaxWg : g;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the checks shared by forward and backward (nothing here touches the device); cfg normalised:
// smooth_l1 at beta = 0 is mae, and a NaN null value selects the NaN mask
int loss_args(const char* who, const dstagnn_loss_cfg* cfg, int64_t n, const void* y, const void* target,
              dstagnn_loss_cfg* out) {
  const std::string w(who);
  if (!cfg || !y || !target) {
    set_last_error(w + ": null cfg / y / target");
    return DSTAGNN_E_ARG;
  }
  if (n <= 0 || n >= (1ll << 31)) {
    set_last_error(w + ": n must be in [1, 2^31)");
    return DSTAGNN_E_ARG;
  }
  if (cfg->kind < DSTAGNN_LOSS_SMOOTH_L1 || cfg->kind > DSTAGNN_LOSS_MSE) {
    set_last_error(w + ": unknown loss kind " + std::to_string(cfg->kind));
    return DSTAGNN_E_ARG;
  }
  if (cfg->mask_mode < DSTAGNN_MASK_NONE || cfg->mask_mode > DSTAGNN_MASK_NAN) {
    set_last_error(w + ": unknown mask mode " + std::to_string(cfg->mask_mode));
    return DSTAGNN_E_ARG;
  }
  if (!(cfg->param >= 0.f)) {  // (a NaN fails too)
    set_last_error(w + ": negative or NaN param (beta / delta)");
    return DSTAGNN_E_ARG;
  }
  *out = *cfg;
  if (out->kind == DSTAGNN_LOSS_SMOOTH_L1 && out->param == 0.f) out->kind = DSTAGNN_LOSS_MAE;
  if (out->mask_mode == DSTAGNN_MASK_NEQ && std::isnan(out->null_val)) out->mask_mode = DSTAGNN_MASK_NAN;
  return 0;
}

// ceil(N / (256 / P)) workgroups, or 0 for a shape the masked metrics reject
int64_t masked_grid(int64_t B, int64_t N, int P) {
  if (P < 1 || P > kMetMaxP || B <= 0 || N <= 0) return 0;
  const int64_t lim = (1ll << 31) - 1;
  if (N > lim / P || B > lim / (N * P)) return 0;  // B N P >= 2^31
  const int64_t TN = kMmThreads / P;
  return (N + TN - 1) / TN;
}

}  // namespace

int dstagnn_loss_tile_elems(void) { return kLossTile; }

int64_t dstagnn_loss_scratch_bytes(int64_t n) {
  return n <= 0 ? 0 : loss_grid(n) * 2 * (int64_t)sizeof(double);
}

int dstagnn_loss_forward(const dstagnn_loss_cfg* cfg, int64_t n, const float* y, const float* target, float* loss,
                         double* stat, void* scratch, size_t scratch_bytes, dstagnn_stream_t stream) {
  dstagnn_loss_cfg c;
  if (int rc = loss_args("loss_forward", cfg, n, y, target, &c)) return rc;
  if (!loss || !stat || !scratch) {
    set_last_error("loss_forward: null loss / stat / scratch");
    return DSTAGNN_E_ARG;
  }
  if (scratch_bytes < (size_t)dstagnn_loss_scratch_bytes(n)) {
    set_last_error("loss_forward: scratch smaller than dstagnn_loss_scratch_bytes(n)");
    return DSTAGNN_E_SPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  int* ticket = stream_counters(st, 1);
  if (!ticket) {
    set_last_error("loss_forward: no ticket counter for this stream");
    return DSTAGNN_E_ARG;
  }
  const int vec = aligned16(y) && aligned16(target);
  hipLaunchKernelGGL(loss_fwd_kernel, dim3((unsigned)loss_grid(n)), dim3(kLossThreads), 0, st, c, n, y, target, vec,
                     static_cast<double*>(scratch), ticket, stat, loss);
  DS_CHECK_LAUNCH();
  return 0;
}

int dstagnn_loss_backward(const dstagnn_loss_cfg* cfg, int64_t n, const float* y, const float* target,
                          const double* stat, const float* gout, float* dy, dstagnn_stream_t stream) {
  dstagnn_loss_cfg c;
  if (int rc = loss_args("loss_backward", cfg, n, y, target, &c)) return rc;
  if (!stat || !dy) {
    set_last_error("loss_backward: null stat / dy");
    return DSTAGNN_E_ARG;
  }
  const int vec = aligned16(y) && aligned16(target) && aligned16(dy);
  const int64_t tiles = (n + kLossTile - 1) / kLossTile;
  hipLaunchKernelGGL(loss_bwd_kernel, dim3((unsigned)tiles), dim3(kLossThreads), 0, (hipStream_t)stream, c, n, y,
                     target, vec, stat, gout, dy);
  DS_CHECK_LAUNCH();
  return 0;
}

int64_t dstagnn_metrics_scratch_bytes(int64_t rows, int P) {
  if (rows <= 0 || P < 1 || P > kMetMaxP) return 0;
  return metrics_grid(rows, P) * 4 * (int64_t)P * (int64_t)sizeof(double);
}

int dstagnn_metrics_accumulate(int64_t rows, int P, const float* pred, const float* target, float null_val,
                               double* table, void* scratch, size_t scratch_bytes, dstagnn_stream_t stream) {
  if (P < 1 || P > kMetMaxP) {
    set_last_error("metrics_accumulate: P (the last axis) must be in [1, 256], got " + std::to_string(P));
    return DSTAGNN_E_SHAPE;
  }
  if (rows <= 0 || rows * (int64_t)P >= (1ll << 31)) {
    set_last_error("metrics_accumulate: rows * P must be in [1, 2^31)");
    return DSTAGNN_E_SHAPE;
  }
  if (!pred || !target || !table || !scratch) {
    set_last_error("metrics_accumulate: null pred / target / table / scratch");
    return DSTAGNN_E_ARG;
  }
  if (scratch_bytes < (size_t)dstagnn_metrics_scratch_bytes(rows, P)) {
    set_last_error("metrics_accumulate: scratch smaller than dstagnn_metrics_scratch_bytes(rows, P)");
    return DSTAGNN_E_SPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  int* ticket = stream_counters(st, 1);
  if (!ticket) {
    set_last_error("metrics_accumulate: no ticket counter for this stream");
    return DSTAGNN_E_ARG;
  }
  hipLaunchKernelGGL(metrics_accum_kernel, dim3((unsigned)metrics_grid(rows, P)), dim3(kMetThreads), 0, st,
                     rows * (int64_t)P, P, pred, target, null_val, std::isnan(null_val) ? 1 : 0,
                     static_cast<double*>(scratch), ticket, table);
  DS_CHECK_LAUNCH();
  return 0;
}

int64_t dstagnn_metrics_masked_scratch_bytes(int64_t B, int64_t N, int P) {
  return masked_grid(B, N, P) * kMmCols * (int64_t)P * (int64_t)sizeof(double);
}

int dstagnn_metrics_accumulate_masked(int64_t B, int64_t N, int P, const float* pred, const float* target,
                                      int mask_mode, float null_val, float mape_null, double* htable,
                                      double* ntable, void* scratch, size_t scratch_bytes, dstagnn_stream_t stream) {
  if (P < 1 || P > kMetMaxP) {
    set_last_error("metrics_accumulate_masked: P (the last axis) must be in [1, 256], got " + std::to_string(P));
    return DSTAGNN_E_SHAPE;
  }
  const int64_t grid = masked_grid(B, N, P);
  if (grid == 0) {
    set_last_error("metrics_accumulate_masked: B and N must be >= 1 and B * N * P in [1, 2^31)");
    return DSTAGNN_E_SHAPE;
  }
  if (!pred || !target || !htable || !scratch) {
    set_last_error("metrics_accumulate_masked: null pred / target / htable / scratch");
    return DSTAGNN_E_ARG;
  }
  if (mask_mode < DSTAGNN_MASK_NONE || mask_mode > DSTAGNN_MASK_NAN) {
    set_last_error("metrics_accumulate_masked: unknown mask mode " + std::to_string(mask_mode));
    return DSTAGNN_E_ARG;
  }
  if (scratch_bytes < (size_t)dstagnn_metrics_masked_scratch_bytes(B, N, P)) {
    set_last_error("metrics_accumulate_masked: scratch smaller than dstagnn_metrics_masked_scratch_bytes(B, N, P)");
    return DSTAGNN_E_SPACE;
  }
  if (mask_mode == DSTAGNN_MASK_NEQ && std::isnan(null_val)) mask_mode = DSTAGNN_MASK_NAN;  // as loss_args
  hipStream_t st = (hipStream_t)stream;
  int* ticket = stream_counters(st, 1);
  if (!ticket) {
    set_last_error("metrics_accumulate_masked: no ticket counter for this stream");
    return DSTAGNN_E_ARG;
  }
  hipLaunchKernelGGL(metrics_masked_kernel, dim3((unsigned)grid), dim3(kMmThreads), 0, st, (int)B, (int)N, P, pred,
                     target, mask_mode, null_val, mape_null, static_cast<double*>(scratch), ticket, htable, ntable);
  DS_CHECK_LAUNCH();
  return 0;
}

// ---- quantile forecasts -----------------------------------------------------------------------
namespace {

// the level rule (include/dstagnn.h): 1 <= Q <= 16 levels, each strictly inside (0, 1), strictly
// increasing; the mask mode as loss_args reads it.  Fills the kernels' argument block.
int pinball_args(const std::string& w, const dstagnn_pinball_cfg* cfg, PinballArgs* out) {
  if (!cfg) {
    set_last_error(w + ": null cfg");
    return DSTAGNN_E_ARG;
  }
  const int Q = cfg->num_quantiles;
  if (Q < 1 || Q > kMaxQ) {
    set_last_error(w + ": num_quantiles must be in [1, " + std::to_string(kMaxQ) + "], got " + std::to_string(Q));
    return DSTAGNN_E_ARG;
  }
  for (int q = 0; q < Q; ++q) {
    const float v = cfg->tau[q];
    if (!(v > 0.f && v < 1.f)) {  // (a NaN fails too)
      set_last_error(w + ": every quantile level must be strictly inside (0, 1), got " + std::to_string(v));
      return DSTAGNN_E_ARG;
    }
    if (q > 0 && !(cfg->tau[q - 1] < v)) {
      set_last_error(w + ": the quantile levels must be strictly increasing");
      return DSTAGNN_E_ARG;
    }
  }
  if (cfg->mask_mode < DSTAGNN_MASK_NONE || cfg->mask_mode > DSTAGNN_MASK_NAN) {
    set_last_error(w + ": unknown mask mode " + std::to_string(cfg->mask_mode));
    return DSTAGNN_E_ARG;
  }
  out->mask_mode = cfg->mask_mode;
  out->null_val = cfg->null_val;
  out->num_quantiles = Q;
  if (out->mask_mode == DSTAGNN_MASK_NEQ && std::isnan(out->null_val)) out->mask_mode = DSTAGNN_MASK_NAN;
  for (int q = 0; q < kMaxQ; ++q) {
    out->tau[q] = q < Q ? cfg->tau[q] : 0.5f;
    out->one_minus_tau[q] = 1.0f - out->tau[q];  // fp32, once
  }
  return 0;
}

// the checks shared by forward and backward; *n = m * Q, the length of the prediction stream
int pinball_pair(const std::string& w, const dstagnn_pinball_cfg* cfg, int64_t m, const void* y, const void* target,
                 PinballArgs* out, int64_t* n) {
  if (int rc = pinball_args(w, cfg, out)) return rc;
  if (m <= 0 || m > ((1ll << 31) - 1) / out->num_quantiles) {
    set_last_error(w + ": m must be >= 1 and m * num_quantiles < 2^31");
    return DSTAGNN_E_SHAPE;
  }
  if (!y || !target) {
    set_last_error(w + ": null y / target");
    return DSTAGNN_E_ARG;
  }
  *n = m * out->num_quantiles;
  return 0;
}

}  // namespace

int64_t dstagnn_pinball_scratch_bytes(int64_t m, int num_quantiles) {
  if (m <= 0 || num_quantiles < 1 || num_quantiles > kMaxQ || m > ((1ll << 31) - 1) / num_quantiles) return 0;
  return loss_grid(m * num_quantiles) * 2 * (int64_t)sizeof(double);
}

int dstagnn_pinball_forward(const dstagnn_pinball_cfg* cfg, int64_t m, const float* y, const float* target,
                            float* loss, double* stat, void* scratch, size_t scratch_bytes,
                            dstagnn_stream_t stream) {
  PinballArgs a;
  int64_t n = 0;
  if (int rc = pinball_pair("pinball_forward", cfg, m, y, target, &a, &n)) return rc;
  if (!loss || !stat || !scratch) {
    set_last_error("pinball_forward: null loss / stat / scratch");
    return DSTAGNN_E_ARG;
  }
  if (scratch_bytes < (size_t)dstagnn_pinball_scratch_bytes(m, a.num_quantiles)) {
    set_last_error("pinball_forward: scratch smaller than dstagnn_pinball_scratch_bytes(m, num_quantiles)");
    return DSTAGNN_E_SPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  int* ticket = stream_counters(st, 1);
  if (!ticket) {
    set_last_error("pinball_forward: no ticket counter for this stream");
    return DSTAGNN_E_ARG;
  }
  const int vec = aligned16(y);  // (the target is read through the cache, one float at a time)
  hipLaunchKernelGGL(pinball_fwd_kernel, dim3((unsigned)loss_grid(n)), dim3(kLossThreads), 0, st, a, n, y, target, vec,
                     static_cast<double*>(scratch), ticket, stat, loss);
  DS_CHECK_LAUNCH();
  return 0;
}

int dstagnn_pinball_backward(const dstagnn_pinball_cfg* cfg, int64_t m, const float* y, const float* target,
                             const double* stat, const float* gout, float* dy, dstagnn_stream_t stream) {
  PinballArgs a;
  int64_t n = 0;
  if (int rc = pinball_pair("pinball_backward", cfg, m, y, target, &a, &n)) return rc;
  if (!stat || !dy) {
    set_last_error("pinball_backward: null stat / dy");
    return DSTAGNN_E_ARG;
  }
  const int vec = aligned16(y) && aligned16(dy);
  const int64_t tiles = (n + kLossTile - 1) / kLossTile;
  hipLaunchKernelGGL(pinball_bwd_kernel, dim3((unsigned)tiles), dim3(kLossThreads), 0, (hipStream_t)stream, a, n, y,
                     target, vec, stat, gout, dy);
  DS_CHECK_LAUNCH();
  return 0;
}

int64_t dstagnn_metrics_quantile_scratch_bytes(int64_t B, int64_t N, int P, int num_quantiles) {
  if (num_quantiles < 1 || num_quantiles > kMaxQ) return 0;
  const int64_t grid = masked_grid(B, N, P);
  if (grid == 0 || B * N * P > ((1ll << 31) - 1) / num_quantiles) return 0;
  return grid * (2 + 3 * (int64_t)num_quantiles) * P * (int64_t)sizeof(double);
}

int dstagnn_metrics_accumulate_quantile(int64_t B, int64_t N, int P, const dstagnn_pinball_cfg* cfg,
                                        const float* pred, const float* target, double* htable, double* ntable,
                                        void* scratch, size_t scratch_bytes, dstagnn_stream_t stream) {
  const std::string w("metrics_accumulate_quantile");
  if (!cfg) {
    set_last_error(w + ": null cfg");
    return DSTAGNN_E_ARG;
  }
  if (P < 1 || P > kMetMaxP) {
    set_last_error(w + ": P (the horizon axis) must be in [1, 256], got " + std::to_string(P));
    return DSTAGNN_E_SHAPE;
  }
  const int Q = cfg->num_quantiles;
  if (Q < 1 || Q > kMaxQ) {
    set_last_error(w + ": Q (the last axis) must be in [1, " + std::to_string(kMaxQ) + "], got " + std::to_string(Q));
    return DSTAGNN_E_SHAPE;
  }
  const int64_t grid = masked_grid(B, N, P);
  if (grid == 0 || B * N * P > ((1ll << 31) - 1) / Q) {
    set_last_error(w + ": B and N must be >= 1 and B * N * P * Q in [1, 2^31)");
    return DSTAGNN_E_SHAPE;
  }
  if (!pred || !target || !htable || !scratch) {
    set_last_error(w + ": null pred / target / htable / scratch");
    return DSTAGNN_E_ARG;
  }
  PinballArgs a;
  if (int rc = pinball_args(w, cfg, &a)) return rc;
  if (scratch_bytes < (size_t)dstagnn_metrics_quantile_scratch_bytes(B, N, P, Q)) {
    set_last_error(w + ": scratch smaller than dstagnn_metrics_quantile_scratch_bytes(B, N, P, Q)");
    return DSTAGNN_E_SPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  int* ticket = stream_counters(st, 1);
  if (!ticket) {
    set_last_error(w + ": no ticket counter for this stream");
    return DSTAGNN_E_ARG;
  }
  hipLaunchKernelGGL(metrics_quantile_kernel, dim3((unsigned)grid), dim3(kQmThreads), 0, st, (int)B, (int)N, P, a,
                     pred, target, static_cast<double*>(scratch), ticket, htable, ntable);
  DS_CHECK_LAUNCH();
  return 0;
}
