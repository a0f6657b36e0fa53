// loss.hip — the two ends of a training step on the GPU (gfx950): the criterion
// (train_DSTAGNN_my.py:132 `nn.SmoothL1Loss()`, :156-157 loss + backward) with the masked
// variants the model family uses for series with gaps, its quantile (pinball) form, and the
// test-set scores (lib/utils1.py:418-431: per-horizon MAE / RMSE / MAPE; lib/metrics.py:6-17 masked
// MAPE).  On a (B, N, P) head output of ~65 k floats all of this is launch latency, so each is ONE
// launch.
//
// The numeric contract, the same in every kernel: a masked entry is selected out (never multiplied
// by zero: a NaN target under the NaN mask leaves the loss finite and its gradient entry exactly
// 0; a NaN prediction at a valid entry makes the loss NaN, which HipAdam's non-finite skip then
// sees), every term is fp32, every add from the first one is fp64 in a fixed order, no
// floating-point atomics: a launch gives the same bits every time.
//
// The shared pieces, each written once:
//   sum_count_handoff   a workgroup's {sum, count} out sc1, the hand-off of handoff.hpp, the last
//                       arrival's grid fold in lane order (the two criterion forwards).
//   fold_into_table     the last arrival of a score kernel: sum_rows_agent<8> over the workgroups,
//                       in order, added to the running table (metrics_accum_kernel,
//                       metrics_quantile_kernel).
//   lds_levels          tau and 1 - tau of the quantile levels into LDS (the pinball kernels).
//   mask_arg, horizon_arg, strip_arg, scratch_arg, ticket_arg   the entry points' common checks.
//
// The kernels:
//   loss_fwd_kernel      d = y - t, loss_term; tiles w, w + grid, ...; sum_count_handoff; stat =
//                        {sum, count}, loss = sum / count (0 when nothing is valid).
//   loss_bwd_kernel      dy = l'(d) * (gout / count) on valid entries, 0 elsewhere; count from the
//                        forward's stat and gout from device memory: no host sync.  Recomputes d.
//   pinball_fwd_kernel / pinball_bwd_kernel   the same two over the (M, Q) prediction stream, q
//                        fastest: element i belongs to target i / Q (read through the cache: Q
//                        neighbouring lanes share one) and level i mod Q (pinball_walk), the levels
//                        from LDS; stat = {sum, count / Q}; a slope of exactly 0 gives +0.
//   metrics_accum_kernel (rows, P) -> the running (P, 4) table of sum |e|, sum e^2, sum |e / t| over
//                        t != null, its count.  Thread rl P + p of the first (256 / P) P reads
//                        element row0 P + rl P + p (coalesced; its p never changes), LDS folds over
//                        rl in order; fold_into_table.
//   metrics_masked_kernel (B, N, P) -> the running (P, 8) and optional (N, 8) tables over the VALID
//                        entries (count, sum e, sum |e|, sum e^2, sum |e / t| over t != mape_null,
//                        its count, sum t, sum t^2).  A workgroup owns a strip of 256 / P nodes:
//                        thread nl P + p walks the samples of element (n0 + nl, p), LDS folds the
//                        strip over nl (per horizon: the sc1 partial) and over p (per node: straight
//                        into the node table, whose rows have one owning workgroup each).
//   metrics_quantile_kernel (B, N, P, Q) -> running (P, 2 + 3 Q) and optional (N, 2 + 3 Q) tables
//                        of the calibration sums (valid and crossing counts; per level the pinball
//                        sum, the count of t <= y_q, the sum of y_q): the masked kernel's strip
//                        plan, kQmChunk columns through LDS at a time; fold_into_table.
//   skill_kernel<S>      (B, N, P) and the series (type S) -> running (P, 13) and optional (N, 13)
//                        tables of the sums behind the skill over persistence, the skill over the
//                        seasonal climatology and the anomaly correlation: the masked kernel's strip
//                        plan, both baselines read out of the series by each sample's label position
//                        (a device array); fold_into_table.
//   events_kernel        (B, N, P) and K thresholds (one set, or one per node) -> running
//                        (P, 2 + (K + 1)^2) and optional (N, ...) tables of the class contingency counts
//                        behind the drought event scores: the masked kernel's strip plan, the cells as
//                        uint32 histograms in dynamic LDS under integer atomic adds; fold_into_table.
//
// In all four criterion kernels: 16-byte loads where every pointer of the launch is 16-byte aligned
// and the tile is whole; scalar loads otherwise (a batch slice y[b:b+bs] of a contiguous tensor is
// often not aligned; the last tile is usually partial).
//
// Copies kept on purpose: the tile walk of the four criterion kernels, the strip
// fold of the two (B, N, P) score kernels and metrics_masked_kernel's last-arrival fold.  Each shared
// form that was tried changed the code of kernels on the training or scoring path, and where it
// was measured it was slower or spilled SGPRs.
#include <cmath>

#include "handoff.hpp"
#include "ops.hpp"

namespace {

constexpr int kLossThreads = 256, kLossPer = 16, kLossTile = kLossThreads * kLossPer;
constexpr int kLossMaxWg = 1024;  // beyond it a workgroup walks tiles w, w + grid, ...
constexpr int kMetThreads = 256, kMetPasses = 8, kMetMaxWg = 256, kMetMaxP = 256;
constexpr int kFold = 8;  // sc1 loads in flight in a last arrival's fold (sum_rows_agent)
constexpr int kMaxQ = DSTAGNN_MAX_QUANTILES;

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

// term and slope of the pinball criterion at d = y_q - t: d > 0: (1 - tau) d, slope 1 - tau; d < 0:
// tau (-d), slope -tau; d = 0: 0 and 0 (DSTAGNN_LOSS_MAE's sign(0) = 0); a NaN d stays NaN
__device__ __forceinline__ float pinball_term(float tau, float omt, float d) {
  return d > 0.f ? omt * d : d < 0.f ? tau * -d : d == 0.f ? 0.f : d;
}
__device__ __forceinline__ float pinball_slope(float tau, float omt, float d) {
  return d > 0.f ? omt : d < 0.f ? -tau : d == 0.f ? 0.f : d;
}

// (target index, level) of the four stream elements i0 .. i0 + 3 of an (M, Q) prediction
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

// A checked dstagnn_pinball_cfg and the 1 - tau of its levels (both formed on the host).
struct PinballArgs {
  int mask_mode;
  float null_val;
  int num_quantiles;
  float tau[kMaxQ], one_minus_tau[kMaxQ];
};

// all threads of a pinball criterion kernel, first thing: the levels tau and 1 - tau into LDS
struct Levels {
  const float *tau, *omt;
};
__device__ __forceinline__ Levels lds_levels(const PinballArgs& cfg) {
  __shared__ float tau[kMaxQ], omt[kMaxQ];
  const int t = threadIdx.x;
  if (t < kMaxQ) tau[t] = cfg.tau[t], omt[t] = cfg.one_minus_tau[t];
  __syncthreads();
  return {tau, omt};
}

// ---- the {sum, count} hand-off ----------------------------------------------------------------
// Every thread of every workgroup of a kLossThreads launch calls it with its own fp64 sum and
// count.  The wave butterfly, the four wave sums as ((w0 + w1) + (w2 + w3)), the workgroup's pair
// out as two 8-byte sc1 stores, the hand-off of handoff.hpp; in the last arrival lane l of the first
// wave takes partials l, l + 64, ... in index order, then the butterfly.  True on thread 0 of the
// last arrival alone, where sum and cnt are then the launch's totals: the same bits every time.
__device__ __forceinline__ bool sum_count_handoff(double& sum, double& cnt, double* __restrict__ part, int* ticket) {
  __shared__ double ws[kLossThreads / 64], wc[kLossThreads / 64];
  __shared__ int last;
  const int t = threadIdx.x;
  sum = wave_sum(sum);
  cnt = wave_sum(cnt);
  if ((t & 63) == 0) ws[t >> 6] = sum, wc[t >> 6] = cnt;
  __syncthreads();
  if (t == 0) {
    st_agent(part + 2 * (int64_t)blockIdx.x, (ws[0] + ws[1]) + (ws[2] + ws[3]));
    st_agent(part + 2 * (int64_t)blockIdx.x + 1, (wc[0] + wc[1]) + (wc[2] + wc[3]));
  }
  if (!last_arrival(ticket, (int)gridDim.x, &last)) return false;
  if (t >= 64) return false;
  double a = 0.0, c = 0.0;
  for (int64_t k = t; k < (int64_t)gridDim.x; k += 64) {
    a += ld_agent(part + 2 * k);
    c += ld_agent(part + 2 * k + 1);
  }
  sum = wave_sum(a);
  cnt = wave_sum(c);
  return t == 0;
}

__global__ __launch_bounds__(kLossThreads) void loss_fwd_kernel(dstagnn_loss_cfg cfg, int64_t n,
                                                               const float* __restrict__ y,
                                                               const float* __restrict__ tg, int vec,
                                                               double* __restrict__ part, int* ticket,
                                                               double* __restrict__ stat, float* __restrict__ loss) {
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
  if (!sum_count_handoff(sum, cnt, part, ticket)) return;
  stat[0] = sum;
  stat[1] = cnt;
  loss[0] = cnt > 0.0 ? (float)(sum / cnt) : 0.f;
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

__global__ __launch_bounds__(kLossThreads) void pinball_fwd_kernel(PinballArgs cfg, int64_t n,
                                                                  const float* __restrict__ y,
                                                                  const float* __restrict__ tg, int vec,
                                                                  double* __restrict__ part, int* ticket,
                                                                  double* __restrict__ stat,
                                                                  float* __restrict__ loss) {
  const int t = threadIdx.x;
  const unsigned Q = (unsigned)cfg.num_quantiles;
  const Levels lv = lds_levels(cfg);
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
            sum += (double)pinball_term(lv.tau[q[j]], lv.omt[q[j]], yv[j] - tv[j]);
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
          sum += (double)pinball_term(lv.tau[qv[u]], lv.omt[qv[u]], yv[u] - tv[u]);
          cnt += 1.0;
        }
      }
    }
  }
  if (!sum_count_handoff(sum, cnt, part, ticket)) return;
  stat[0] = sum;
  stat[1] = cnt / (double)Q;  // the valid target entries (cnt is a multiple of Q: exact)
  loss[0] = cnt > 0.0 ? (float)(sum / cnt) : 0.f;
}

__global__ __launch_bounds__(kLossThreads) void pinball_bwd_kernel(PinballArgs cfg, int64_t n,
                                                                  const float* __restrict__ y,
                                                                  const float* __restrict__ tg, int vec,
                                                                  const double* __restrict__ stat,
                                                                  const float* __restrict__ gout,
                                                                  float* __restrict__ dy) {
  const int t = threadIdx.x;
  const unsigned Q = (unsigned)cfg.num_quantiles;
  const Levels lv = lds_levels(cfg);
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
        const float s = pinball_slope(lv.tau[q[j]], lv.omt[q[j]], yv[j] - tv[j]);
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
      const float s = pinball_slope(lv.tau[qv[u]], lv.omt[qv[u]], yv[u] - tv[u]);
      dy[i] = is_valid(cfg.mask_mode, cfg.null_val, tv[u]) && s != 0.f ? s * scale : 0.f;
    }
  }
}

// ---- the score tables --------------------------------------------------------------------------
// The last arrival of a score kernel: workgroup k's partial is part[k cols P + c P + p]; they are
// added in workgroup order (kFold sc1 loads issued before their adds) and the total joins the
// running table[p cols + c].  Launches on one stream are ordered: the table needs no atomics.
__device__ __forceinline__ void fold_into_table(const double* __restrict__ part, int P, int cols,
                                                double* __restrict__ table) {
  const int items = cols * P;
  for (int item = (int)threadIdx.x; item < items; item += kMetThreads) {  // (every score kernel: 256 threads)
    const int c = item / P, p = item - c * P;
    table[p * cols + c] += sum_rows_agent<kFold>(part + item, items, (int)gridDim.x);
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
  fold_into_table(part, P, 4, table);
}

constexpr int kMmCols = 8, kMmUnroll = 4;

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

__global__ __launch_bounds__(kMetThreads) void metrics_masked_kernel(int B, int N, int P,
                                                                   const float* __restrict__ pred,
                                                                   const float* __restrict__ tg, int mask,
                                                                   float null_val, float mape_null,
                                                                   double* __restrict__ part, int* ticket,
                                                                   double* __restrict__ htable,
                                                                   double* __restrict__ ntable) {
  __shared__ double red[kMmCols][kMetThreads];
  __shared__ int last;
  const int t = threadIdx.x;
  const int TN = kMetThreads / P;            // nodes of a whole strip
  const int n0 = (int)blockIdx.x * TN;       // (the grid is ceil(N / TN): n0 < N)
  const int tn = N - n0 < TN ? N - n0 : TN;  // nodes of this strip (the last one is partial)
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
    for (int item = t; item < kMmCols * tn; item += kMetThreads) {
      const int nl = item / kMmCols, c = item - nl * kMmCols;
      double a = 0.0;
      for (int p = 0; p < P; ++p) a += red[c][nl * P + p];
      ntable[(int64_t)n0 * kMmCols + item] += a;
    }
  }
  // per horizon, over nl in order (the idle rows of a partial strip hold zeros); item = c P + p
  const int items = kMmCols * P;
  for (int item = t; item < items; item += kMetThreads) {
    const int c = item / P, p = item - c * P;
    double a = 0.0;
    for (int nl = 0; nl < TN; ++nl) a += red[c][nl * P + p];
    st_agent(part + (int64_t)blockIdx.x * items + item, a);
  }
  if (!last_arrival(ticket, (int)gridDim.x, &last)) return;
  // the last arrival: the partials in workgroup order, kFold sc1 loads issued before their adds
  const int G = (int)gridDim.x;
  for (int item = t; item < items; item += kMetThreads) {
    const int c = item / P, p = item - c * P;
    double a = 0.0;
    for (int k0 = 0; k0 < G; k0 += kFold) {
      double u[kFold];
#pragma unroll
      for (int k = 0; k < kFold; ++k) u[k] = k0 + k < G ? ld_agent(part + (int64_t)(k0 + k) * items + item) : 0.0;
#pragma unroll
      for (int k = 0; k < kFold; ++k) a += u[k];
    }
    htable[p * kMmCols + c] += a;
  }
}

// The calibration sums of (B, N, P, Q) predictions against (B, N, P) targets: 2 + 3 Q sums per
// thread: valid count, crossing count and, per level, the pinball sum (fp32 term), the count of
// t <= y_q (fp32 compare) and the sum of y_q (exact as doubles).  A thread reads the Q floats of its
// entry (the wave: 64 Q contiguous floats, every byte used) and keeps its sums in registers; the
// loops over q are unrolled to kMaxQ under the uniform q < Q so every index is a constant.
constexpr int kQmCols = 2 + 3 * kMaxQ, kQmChunk = 8;

__global__ __launch_bounds__(kMetThreads) void metrics_quantile_kernel(int B, int N, int P, PinballArgs cfg,
                                                                     const float* __restrict__ pred,
                                                                     const float* __restrict__ tg,
                                                                     double* __restrict__ part, int* ticket,
                                                                     double* __restrict__ htable,
                                                                     double* __restrict__ ntable) {
  __shared__ double red[kQmChunk][kMetThreads];
  __shared__ int last;
  const int t = threadIdx.x;
  const int Q = cfg.num_quantiles, cols = 2 + 3 * Q;
  const int TN = kMetThreads / P;
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
      for (int item = t; item < cw * tn; item += kMetThreads) {
        const int nl = item / cw, j = item - nl * cw;
        double a = 0.0;
        for (int p = 0; p < P; ++p) a += red[j][nl * P + p];
        ntable[(int64_t)(n0 + nl) * cols + c0 + j] += a;
      }
    }
    // per horizon, over nl in order (the idle rows of a partial strip hold zeros)
    for (int item = t; item < cw * P; item += kMetThreads) {
      const int j = item / P, p = item - j * P;
      double a = 0.0;
      for (int nl = 0; nl < TN; ++nl) a += red[j][nl * P + p];
      st_agent(part + (int64_t)blockIdx.x * items + (c0 + j) * P + p, a);
    }
  }
  if (!last_arrival(ticket, (int)gridDim.x, &last)) return;
  fold_into_table(part, P, cols, htable);
}

// ---- skill against persistence and the seasonal climatology --------------------------------------
// The 13 sums of include/dstagnn.h's skill section.  Both baselines are read out of the series
// inside this launch: the persistence value of (b, n) is src[pos[b] - 1, n, F - 1] (src: the series,
// or its unlimited forward fill), the climatology of (b, n, p) is clim[(pos[b] + p) mod period, n].
constexpr int kSkCols = DSTAGNN_SKILL_COLS, kSkUnroll = 4;

struct SkillArgs {
  int B, N, P, F, period;
  int mask, src_masked, src_nan;
  float null_val;
  double src_null;
  int64_t L;
  const float *pred, *tg;
  const void* src;
  const int64_t* pos;
  const double* clim;
  const int32_t* cnt;
};

// the windows section's rule for a series element (windows.hip win_missing)
template <typename S>
__device__ __forceinline__ bool series_missing(S v, S null, int nan_mode) {
  return nan_mode ? v != v : v == null;
}

// one entry into a thread's 13 sums: the differences and the squares of columns 1, 2, 6, 7 in fp32,
// the anomaly products as doubles (exact), every add in fp64; pers / clim: that baseline is defined
__device__ __forceinline__ void skill_entry(double (&s)[kSkCols], int mask, float null_val, float pv, float tv,
                                            bool pers, float q, bool clim, float c) {
  if (!is_valid(mask, null_val, tv)) return;  // selected out: a NaN target never reaches a sum
  const float em = pv - tv;
  const float em2 = em * em, ema = fabsf(em);
  if (pers) {
    const float ep = q - tv;
    s[0] += 1.0;
    s[1] += (double)em2;
    s[2] += (double)(ep * ep);
    s[3] += (double)ema;
    s[4] += (double)fabsf(ep);
  }
  if (clim) {
    const float ec = c - tv, af = pv - c, ao = tv - c;
    s[5] += 1.0;
    s[6] += (double)em2;
    s[7] += (double)(ec * ec);
    s[8] += (double)ema;
    s[9] += (double)fabsf(ec);
    s[10] += (double)af * (double)ao;
    s[11] += (double)af * (double)af;
    s[12] += (double)ao * (double)ao;
  }
}

// metrics_masked_kernel's strip plan: a workgroup owns 256 / P nodes, thread nl P + p walks the
// samples of element (n0 + nl, p) with the loads of kSkUnroll samples in flight (each sample's label
// position first: it is uniform, and the two baseline addresses hang on it).  A sample whose targets
// would leave the series is skipped unread.  LDS folds over nl (per horizon: the sc1 partial) and
// over p (per node: straight into the node table, whose rows have one owning workgroup each).
template <typename S>
__global__ __launch_bounds__(kMetThreads) void skill_kernel(SkillArgs a, double* __restrict__ part, int* ticket,
                                                          double* __restrict__ htable, double* __restrict__ ntable) {
  __shared__ double red[kSkCols][kMetThreads];
  __shared__ int last;
  const int t = threadIdx.x;
  const int P = a.P, N = a.N;
  const int TN = kMetThreads / P;            // nodes of a whole strip
  const int n0 = (int)blockIdx.x * TN;       // (the grid is ceil(N / TN): n0 < N)
  const int tn = N - n0 < TN ? N - n0 : TN;  // nodes of this strip (the last one is partial)
  double s[kSkCols];
#pragma unroll
  for (int c = 0; c < kSkCols; ++c) s[c] = 0.0;
  if (t < tn * P) {
    const int nl = t / P, p = t - nl * P, n = n0 + nl;
    const int pm = p % a.period;  // this thread's phase is (pos mod period + pm) mod period
    const int64_t step = (int64_t)N * P, NF = (int64_t)N * a.F;
    const float* __restrict__ pp = a.pred + (int64_t)n0 * P + t;
    const float* __restrict__ tp = a.tg + (int64_t)n0 * P + t;
    const S* __restrict__ sp = static_cast<const S*>(a.src) + (int64_t)n * a.F + (a.F - 1);
    const double* __restrict__ cl = a.clim + n;
    const int32_t* __restrict__ cn = a.cnt + n;
    const S snull = (S)a.src_null;
    for (int b0 = 0; b0 < a.B; b0 += kSkUnroll) {
      float pv[kSkUnroll], tv[kSkUnroll];
      double cv[kSkUnroll];
      S qv[kSkUnroll];
      int cc[kSkUnroll];
      bool in[kSkUnroll], prev[kSkUnroll];
#pragma unroll
      for (int u = 0; u < kSkUnroll; ++u) {
        const int b = b0 + u;
        const int64_t l = b < a.B ? a.pos[b] : -1;
        in[u] = l >= 0 && l + P <= a.L;  // (uniform; b >= B fails it)
        prev[u] = in[u] && l >= 1;
        int64_t ph = in[u] ? l % a.period + pm : 0;  // (both terms below period)
        if (ph >= a.period) ph -= a.period;
        pv[u] = in[u] ? pp[b * step] : 0.f;
        tv[u] = in[u] ? tp[b * step] : 0.f;
        qv[u] = prev[u] ? sp[(l - 1) * NF] : snull;
        cv[u] = in[u] ? cl[ph * N] : 0.0;
        cc[u] = in[u] ? cn[ph * N] : 0;
      }
#pragma unroll
      for (int u = 0; u < kSkUnroll; ++u) {
        if (!in[u]) continue;
        const bool pers = prev[u] && !(a.src_masked && series_missing(qv[u], snull, a.src_nan));
        skill_entry(s, a.mask, a.null_val, pv[u], tv[u], pers, (float)qv[u], cc[u] > 0, (float)cv[u]);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < kSkCols; ++c) red[c][t] = s[c];
  __syncthreads();
  // per node, over p in order: item = nl 13 + c lands on ntable[(n0 + nl) 13 + c].  This workgroup is
  // the only one that ever touches these rows and launches on a stream are ordered: plain adds.
  if (ntable != nullptr) {
    for (int item = t; item < kSkCols * tn; item += kMetThreads) {
      const int nl = item / kSkCols, c = item - nl * kSkCols;
      double acc = 0.0;
      for (int p = 0; p < P; ++p) acc += red[c][nl * P + p];
      ntable[(int64_t)n0 * kSkCols + item] += acc;
    }
  }
  // per horizon, over nl in order (the idle rows of a partial strip hold zeros); item = c P + p
  const int items = kSkCols * P;
  for (int item = t; item < items; item += kMetThreads) {
    const int c = item / P, p = item - c * P;
    double acc = 0.0;
    for (int nl = 0; nl < TN; ++nl) acc += red[c][nl * P + p];
    st_agent(part + (int64_t)blockIdx.x * items + item, acc);
  }
  if (!last_arrival(ticket, (int)gridDim.x, &last)) return;
  fold_into_table(part, P, kSkCols, htable);
}

// ---- drought event scores: the class contingency table --------------------------------------------
// The counts of include/dstagnn.h's events section.  Unlike the sums above, an entry increments ONE
// cell of the (K + 1) x (K + 1) table and which one is known only at run time: a register array
// indexed that way would go to scratch, so the cells are uint32 histograms in (dynamic) LDS taking
// integer atomic adds.  Integer adds commute: the same bits on every launch, and no floating-point
// atomics here either.  A cell holds at most B N P < 2^31.
constexpr int kEvMax = DSTAGNN_MAX_EVENT_LEVELS, kEvUnroll = 4, kEvMaxLds = 64 * 1024;

// c(v) = the number of events v is: K fp32 compares (a NaN v is none of them)
__device__ __forceinline__ int event_class(const float (&th)[kEvMax], int K, int above, float v) {
  int c = 0;
#pragma unroll
  for (int k = 0; k < kEvMax; ++k)
    if (k < K) c += (above ? v >= th[k] : v <= th[k]) ? 1 : 0;
  return c;
}

// one entry: the valid count in a register (n), a NaN prediction into column 1, any other into its
// cell 2 + co (K + 1) + cf, one LDS atomic add per histogram (hp: this thread's horizon row, hq: its
// node row)
__device__ __forceinline__ void event_entry(const float (&th)[kEvMax], int K, int above, int mask, float null_val,
                                            float pv, float tv, unsigned& n, unsigned* hp, unsigned* hq) {
  if (!is_valid(mask, null_val, tv)) return;  // selected out: an invalid target reaches no count
  n += 1u;
  const int cell = pv != pv ? 1 : 2 + event_class(th, K, above, tv) * (K + 1) + event_class(th, K, above, pv);
  atomicAdd(hp + cell, 1u);
  atomicAdd(hq + cell, 1u);
}

// metrics_masked_kernel's strip plan: a workgroup owns 256 / P nodes, thread nl P + p walks the
// samples of element (n0 + nl, p) with the loads of kEvUnroll samples in flight; its node's K
// thresholds sit in registers (the loops over k unrolled to kEvMax under the uniform k < K, so every
// index is a constant).  The threads of a node whose thresholds are NaN skip the walk.  LDS:
// hh[P][cols] then hn[TN][cols], zeroed first; after the walk hn goes straight into this workgroup's
// own node rows and hh, as doubles, is the sc1 partial fold_into_table takes.
__global__ __launch_bounds__(kMetThreads) void events_kernel(int B, int N, int P, int K, int above,
                                                            const float* __restrict__ pred,
                                                            const float* __restrict__ tg, int mask, float null_val,
                                                            const float* __restrict__ thr, int per_node,
                                                            double* __restrict__ part, int* ticket,
                                                            double* __restrict__ htable, double* __restrict__ ntable) {
  extern __shared__ unsigned ev_hist[];
  __shared__ int last;
  const int t = threadIdx.x;
  const int cols = 2 + (K + 1) * (K + 1);
  const int TN = kMetThreads / P;            // nodes of a whole strip
  const int n0 = (int)blockIdx.x * TN;       // (the grid is ceil(N / TN): n0 < N)
  const int tn = N - n0 < TN ? N - n0 : TN;  // nodes of this strip (the last one is partial)
  unsigned* hh = ev_hist;
  unsigned* hn = ev_hist + P * cols;
  for (int i = t; i < (P + TN) * cols; i += kMetThreads) ev_hist[i] = 0u;
  __syncthreads();
  if (t < tn * P) {
    const int nl = t / P, p = t - nl * P;
    float th[kEvMax];
    bool excluded = false;
#pragma unroll
    for (int k = 0; k < kEvMax; ++k) {
      th[k] = k < K ? thr[per_node ? (int64_t)k * N + n0 + nl : k] : 0.f;
      excluded = excluded || th[k] != th[k];
    }
    if (!excluded) {
      // element (b, n0 + nl, p) sits at b N P + n0 P + t: for a fixed b the strip reads tn P
      // contiguous floats
      const int64_t step = (int64_t)N * P;
      const float* __restrict__ pp = pred + (int64_t)n0 * P + t;
      const float* __restrict__ tp = tg + (int64_t)n0 * P + t;
      unsigned* hp = hh + p * cols;
      unsigned* hq = hn + nl * cols;
      unsigned n = 0u;
      int b = 0;
      for (; b + kEvUnroll <= B; b += kEvUnroll) {  // the loads of kEvUnroll samples in flight together
        float pv[kEvUnroll], tv[kEvUnroll];
#pragma unroll
        for (int u = 0; u < kEvUnroll; ++u) pv[u] = pp[(b + u) * step], tv[u] = tp[(b + u) * step];
#pragma unroll
        for (int u = 0; u < kEvUnroll; ++u) event_entry(th, K, above, mask, null_val, pv[u], tv[u], n, hp, hq);
      }
      for (; b < B; ++b) event_entry(th, K, above, mask, null_val, pp[b * step], tp[b * step], n, hp, hq);
      atomicAdd(hp, n);  // column 0: once per thread
      atomicAdd(hq, n);
    }
  }
  __syncthreads();
  // per node: item = nl cols + c lands on ntable[(n0 + nl) cols + c].  This workgroup is the only one
  // that ever touches these rows and launches on a stream are ordered: plain adds.
  if (ntable != nullptr)
    for (int item = t; item < tn * cols; item += kMetThreads) ntable[(int64_t)n0 * cols + item] += (double)hn[item];
  // per horizon: item = c P + p, the layout fold_into_table reads
  const int items = cols * P;
  for (int item = t; item < items; item += kMetThreads) {
    const int c = item / P, p = item - c * P;
    st_agent(part + (int64_t)blockIdx.x * items + item, (double)hh[p * cols + c]);
  }
  if (!last_arrival(ticket, (int)gridDim.x, &last)) return;
  fold_into_table(part, P, cols, htable);
}

// the dynamic LDS of events_kernel at (P, K), in bytes
int64_t events_lds_bytes(int P, int K) {
  return ((int64_t)P + kMetThreads / P) * (2 + (K + 1) * (K + 1)) * (int64_t)sizeof(unsigned);
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

// ceil(N / (256 / P)) workgroups, or 0 for a shape the strip kernels reject
int64_t masked_grid(int64_t B, int64_t N, int P) {
  if (P < 1 || P > kMetMaxP || B <= 0 || N <= 0) return 0;
  const int64_t lim = (1ll << 31) - 1;
  if (N > lim / P || B > lim / (N * P)) return 0;  // B N P >= 2^31
  const int64_t TN = kMetThreads / P;
  return (N + TN - 1) / TN;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---- the checks every entry point shares (nothing here touches the device); w: the entry's name ----
int fail(const std::string& text, int rc) {
  set_last_error(text);
  return rc;
}

// the mask-mode range, and the rule that a NaN null value under the != mode selects the NaN mask
int mask_arg(const std::string& w, int* mask_mode, float null_val) {
  if (*mask_mode < DSTAGNN_MASK_NONE || *mask_mode > DSTAGNN_MASK_NAN)
    return fail(w + ": unknown mask mode " + std::to_string(*mask_mode), DSTAGNN_E_ARG);
  if (*mask_mode == DSTAGNN_MASK_NEQ && std::isnan(null_val)) *mask_mode = DSTAGNN_MASK_NAN;
  return 0;
}

// P of a score table; axis: what the entry calls it
int horizon_arg(const std::string& w, int P, const char* axis) {
  if (P < 1 || P > kMetMaxP)
    return fail(w + ": P (the " + axis + " axis) must be in [1, 256], got " + std::to_string(P), DSTAGNN_E_SHAPE);
  return 0;
}

// the (B, N, P) extent of a strip kernel, times Q values per entry; extent: its text; -> the grid
int strip_arg(const std::string& w, int64_t B, int64_t N, int P, int Q, const char* extent, int64_t* grid) {
  *grid = masked_grid(B, N, P);
  if (*grid == 0 || B * N * P > ((1ll << 31) - 1) / Q)
    return fail(w + ": B and N must be >= 1 and " + extent + " in [1, 2^31)", DSTAGNN_E_SHAPE);
  return 0;
}

// need: the entry's scratch-size function applied to its shape; call: that function as the header writes it
int scratch_arg(const std::string& w, size_t scratch_bytes, int64_t need, const char* call) {
  if (scratch_bytes < (size_t)need) return fail(w + ": scratch smaller than " + call, DSTAGNN_E_SPACE);
  return 0;
}

// the stream's ticket counter for one hand-off (zero between launches), or null with the error set
int* ticket_arg(const std::string& w, hipStream_t st) {
  int* ticket = stream_counters(st, 1);
  if (!ticket) set_last_error(w + ": no ticket counter for this stream");
  return ticket;
}

// the checks shared by the criterion's forward and backward; cfg normalised: smooth_l1 at beta = 0
// is mae, the mask as mask_arg leaves it
int loss_args(const std::string& w, const dstagnn_loss_cfg* cfg, int64_t n, const void* y, const void* target,
              dstagnn_loss_cfg* out) {
  if (!cfg || !y || !target) return fail(w + ": null cfg / y / target", DSTAGNN_E_ARG);
  if (n <= 0 || n >= (1ll << 31)) return fail(w + ": n must be in [1, 2^31)", DSTAGNN_E_ARG);
  if (cfg->kind < DSTAGNN_LOSS_SMOOTH_L1 || cfg->kind > DSTAGNN_LOSS_MSE)
    return fail(w + ": unknown loss kind " + std::to_string(cfg->kind), DSTAGNN_E_ARG);
  *out = *cfg;
  if (int rc = mask_arg(w, &out->mask_mode, out->null_val)) return rc;
  if (!(cfg->param >= 0.f))  // (a NaN fails too)
    return fail(w + ": negative or NaN param (beta / delta)", DSTAGNN_E_ARG);
  if (out->kind == DSTAGNN_LOSS_SMOOTH_L1 && out->param == 0.f) out->kind = DSTAGNN_LOSS_MAE;
  return 0;
}

// the level rule (include/dstagnn.h): 1 <= Q <= 16 levels, each strictly inside (0, 1), strictly
// increasing; the mask as mask_arg leaves it.  Fills the kernels' argument block.
int pinball_args(const std::string& w, const dstagnn_pinball_cfg* cfg, PinballArgs* out) {
  if (!cfg) return fail(w + ": null cfg", DSTAGNN_E_ARG);
  const int Q = cfg->num_quantiles;
  if (Q < 1 || Q > kMaxQ)
    return fail(w + ": num_quantiles must be in [1, " + std::to_string(kMaxQ) + "], got " + std::to_string(Q),
                DSTAGNN_E_ARG);
  for (int q = 0; q < Q; ++q) {
    const float v = cfg->tau[q];
    if (!(v > 0.f && v < 1.f))  // (a NaN fails too)
      return fail(w + ": every quantile level must be strictly inside (0, 1), got " + std::to_string(v),
                  DSTAGNN_E_ARG);
    if (q > 0 && !(cfg->tau[q - 1] < v))
      return fail(w + ": the quantile levels must be strictly increasing", DSTAGNN_E_ARG);
  }
  out->mask_mode = cfg->mask_mode;
  out->null_val = cfg->null_val;
  out->num_quantiles = Q;
  if (int rc = mask_arg(w, &out->mask_mode, out->null_val)) return rc;
  for (int q = 0; q < kMaxQ; ++q) {
    out->tau[q] = q < Q ? cfg->tau[q] : 0.5f;
    out->one_minus_tau[q] = 1.0f - out->tau[q];  // fp32, once
  }
  return 0;
}

// the checks shared by the pinball criterion's forward and backward; *n = m * Q, the length of the
// prediction stream
int pinball_pair(const std::string& w, const dstagnn_pinball_cfg* cfg, int64_t m, const void* y, const void* target,
                 PinballArgs* out, int64_t* n) {
  if (int rc = pinball_args(w, cfg, out)) return rc;
  if (m <= 0 || m > ((1ll << 31) - 1) / out->num_quantiles)
    return fail(w + ": m must be >= 1 and m * num_quantiles < 2^31", DSTAGNN_E_SHAPE);
  if (!y || !target) return fail(w + ": null y / target", DSTAGNN_E_ARG);
  *n = m * out->num_quantiles;
  return 0;
}

}  // namespace

int dstagnn_loss_tile_elems(void) { return kLossTile; }

int64_t dstagnn_loss_scratch_bytes(int64_t n) {
  return n <= 0 ? 0 : loss_grid(n) * 2 * (int64_t)sizeof(double);
}

int dstagnn_loss_forward(const dstagnn_loss_cfg* cfg, int64_t n, const float* y, const float* target, float* loss,
                         double* stat, void* scratch, size_t scratch_bytes, dstagnn_stream_t stream) {
  const std::string w("loss_forward");
  dstagnn_loss_cfg c;
  if (int rc = loss_args(w, cfg, n, y, target, &c)) return rc;
  if (!loss || !stat || !scratch) return fail(w + ": null loss / stat / scratch", DSTAGNN_E_ARG);
  if (int rc = scratch_arg(w, scratch_bytes, dstagnn_loss_scratch_bytes(n), "dstagnn_loss_scratch_bytes(n)")) return rc;
  hipStream_t st = (hipStream_t)stream;
  int* ticket = ticket_arg(w, st);
  if (!ticket) return DSTAGNN_E_ARG;
  const int vec = aligned16(y) && aligned16(target);
  hipLaunchKernelGGL(loss_fwd_kernel, dim3((unsigned)loss_grid(n)), dim3(kLossThreads), 0, st, c, n, y, target, vec,
                     static_cast<double*>(scratch), ticket, stat, loss);
  DS_CHECK_LAUNCH();
  return 0;
}

int dstagnn_loss_backward(const dstagnn_loss_cfg* cfg, int64_t n, const float* y, const float* target,
                          const double* stat, const float* gout, float* dy, dstagnn_stream_t stream) {
  const std::string w("loss_backward");
  dstagnn_loss_cfg c;
  if (int rc = loss_args(w, cfg, n, y, target, &c)) return rc;
  if (!stat || !dy) return fail(w + ": null stat / dy", DSTAGNN_E_ARG);
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
  const std::string w("metrics_accumulate");
  if (int rc = horizon_arg(w, P, "last")) return rc;
  if (rows <= 0 || rows * (int64_t)P >= (1ll << 31))
    return fail(w + ": rows * P must be in [1, 2^31)", DSTAGNN_E_SHAPE);
  if (!pred || !target || !table || !scratch) return fail(w + ": null pred / target / table / scratch", DSTAGNN_E_ARG);
  if (int rc = scratch_arg(w, scratch_bytes, dstagnn_metrics_scratch_bytes(rows, P),
                           "dstagnn_metrics_scratch_bytes(rows, P)"))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  int* ticket = ticket_arg(w, st);
  if (!ticket) return DSTAGNN_E_ARG;
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
  const std::string w("metrics_accumulate_masked");
  int64_t grid = 0;
  if (int rc = horizon_arg(w, P, "last")) return rc;
  if (int rc = strip_arg(w, B, N, P, 1, "B * N * P", &grid)) return rc;
  if (!pred || !target || !htable || !scratch) return fail(w + ": null pred / target / htable / scratch", DSTAGNN_E_ARG);
  if (int rc = mask_arg(w, &mask_mode, null_val)) return rc;
  if (int rc = scratch_arg(w, scratch_bytes, dstagnn_metrics_masked_scratch_bytes(B, N, P),
                           "dstagnn_metrics_masked_scratch_bytes(B, N, P)"))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  int* ticket = ticket_arg(w, st);
  if (!ticket) return DSTAGNN_E_ARG;
  hipLaunchKernelGGL(metrics_masked_kernel, dim3((unsigned)grid), dim3(kMetThreads), 0, st, (int)B, (int)N, P, pred,
                     target, mask_mode, null_val, mape_null, static_cast<double*>(scratch), ticket, htable, ntable);
  DS_CHECK_LAUNCH();
  return 0;
}

int64_t dstagnn_pinball_scratch_bytes(int64_t m, int num_quantiles) {
  if (m <= 0 || num_quantiles < 1 || num_quantiles > kMaxQ || m > ((1ll << 31) - 1) / num_quantiles) return 0;
  return loss_grid(m * num_quantiles) * 2 * (int64_t)sizeof(double);
}

int dstagnn_pinball_forward(const dstagnn_pinball_cfg* cfg, int64_t m, const float* y, const float* target,
                            float* loss, double* stat, void* scratch, size_t scratch_bytes,
                            dstagnn_stream_t stream) {
  const std::string w("pinball_forward");
  PinballArgs a;
  int64_t n = 0;
  if (int rc = pinball_pair(w, cfg, m, y, target, &a, &n)) return rc;
  if (!loss || !stat || !scratch) return fail(w + ": null loss / stat / scratch", DSTAGNN_E_ARG);
  if (int rc = scratch_arg(w, scratch_bytes, dstagnn_pinball_scratch_bytes(m, a.num_quantiles),
                           "dstagnn_pinball_scratch_bytes(m, num_quantiles)"))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  int* ticket = ticket_arg(w, st);
  if (!ticket) return DSTAGNN_E_ARG;
  const int vec = aligned16(y);  // (the target is read through the cache, one float at a time)
  hipLaunchKernelGGL(pinball_fwd_kernel, dim3((unsigned)loss_grid(n)), dim3(kLossThreads), 0, st, a, n, y, target, vec,
                     static_cast<double*>(scratch), ticket, stat, loss);
  DS_CHECK_LAUNCH();
  return 0;
}

int dstagnn_pinball_backward(const dstagnn_pinball_cfg* cfg, int64_t m, const float* y, const float* target,
                             const double* stat, const float* gout, float* dy, dstagnn_stream_t stream) {
  const std::string w("pinball_backward");
  PinballArgs a;
  int64_t n = 0;
  if (int rc = pinball_pair(w, cfg, m, y, target, &a, &n)) return rc;
  if (!stat || !dy) return fail(w + ": null stat / dy", DSTAGNN_E_ARG);
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
  if (!cfg) return fail(w + ": null cfg", DSTAGNN_E_ARG);
  if (int rc = horizon_arg(w, P, "horizon")) return rc;
  const int Q = cfg->num_quantiles;
  if (Q < 1 || Q > kMaxQ)
    return fail(w + ": Q (the last axis) must be in [1, " + std::to_string(kMaxQ) + "], got " + std::to_string(Q),
                DSTAGNN_E_SHAPE);
  int64_t grid = 0;
  if (int rc = strip_arg(w, B, N, P, Q, "B * N * P * Q", &grid)) return rc;
  if (!pred || !target || !htable || !scratch) return fail(w + ": null pred / target / htable / scratch", DSTAGNN_E_ARG);
  PinballArgs a;
  if (int rc = pinball_args(w, cfg, &a)) return rc;
  if (int rc = scratch_arg(w, scratch_bytes, dstagnn_metrics_quantile_scratch_bytes(B, N, P, Q),
                           "dstagnn_metrics_quantile_scratch_bytes(B, N, P, Q)"))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  int* ticket = ticket_arg(w, st);
  if (!ticket) return DSTAGNN_E_ARG;
  hipLaunchKernelGGL(metrics_quantile_kernel, dim3((unsigned)grid), dim3(kMetThreads), 0, st, (int)B, (int)N, P, a,
                     pred, target, static_cast<double*>(scratch), ticket, htable, ntable);
  DS_CHECK_LAUNCH();
  return 0;
}

int64_t dstagnn_skill_scratch_bytes(int64_t B, int64_t N, int P) {
  return masked_grid(B, N, P) * kSkCols * (int64_t)P * (int64_t)sizeof(double);
}

int dstagnn_skill_accumulate(int64_t B, int64_t N, int P, const float* pred, const float* target, int mask_mode,
                             float null_val, int series_f64, const void* pers_src, int64_t L, int64_t F,
                             int src_masked, double src_null, const int64_t* pos, const double* clim,
                             const int32_t* cnt, int64_t period, double* htable, double* ntable, void* scratch,
                             size_t scratch_bytes, dstagnn_stream_t stream) {
  const std::string w("skill_accumulate");
  int64_t grid = 0;
  if (int rc = horizon_arg(w, P, "last")) return rc;
  if (int rc = strip_arg(w, B, N, P, 1, "B * N * P", &grid)) return rc;
  const int64_t lim = (1ll << 31) - 1;
  if (L < 1 || F < 1 || N > lim / L || F > lim / (L * N))
    return fail(w + ": L and F must be >= 1 and L * N * F below 2^31", DSTAGNN_E_SHAPE);
  if (period < 1 || period > L || period > lim / N)
    return fail(w + ": period must be in [1, L] and period * N below 2^31, got " + std::to_string(period),
                DSTAGNN_E_SHAPE);
  if (!pred || !target || !pers_src || !pos || !clim || !cnt || !htable || !scratch)
    return fail(w + ": null pred / target / pers_src / pos / clim / cnt / htable / scratch", DSTAGNN_E_ARG);
  if (int rc = mask_arg(w, &mask_mode, null_val)) return rc;
  if (!src_masked && std::isnan(src_null)) return fail(w + ": a NaN src_null needs src_masked = 1", DSTAGNN_E_ARG);
  if (int rc = scratch_arg(w, scratch_bytes, dstagnn_skill_scratch_bytes(B, N, P), "dstagnn_skill_scratch_bytes(B, N, P)"))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  int* ticket = ticket_arg(w, st);
  if (!ticket) return DSTAGNN_E_ARG;
  SkillArgs a{};
  a.B = (int)B, a.N = (int)N, a.P = P, a.F = (int)F, a.period = (int)period;
  a.mask = mask_mode, a.null_val = null_val;
  a.src_masked = src_masked ? 1 : 0, a.src_nan = std::isnan(src_null) ? 1 : 0, a.src_null = src_masked ? src_null : 0.0;
  a.L = L, a.pred = pred, a.tg = target, a.src = pers_src, a.pos = pos, a.clim = clim, a.cnt = cnt;
  if (series_f64)
    hipLaunchKernelGGL(skill_kernel<double>, dim3((unsigned)grid), dim3(kMetThreads), 0, st, a,
                       static_cast<double*>(scratch), ticket, htable, ntable);
  else
    hipLaunchKernelGGL(skill_kernel<float>, dim3((unsigned)grid), dim3(kMetThreads), 0, st, a,
                       static_cast<double*>(scratch), ticket, htable, ntable);
  DS_CHECK_LAUNCH();
  return 0;
}

// 0 for a shape dstagnn_events_accumulate rejects
int64_t dstagnn_events_scratch_bytes(int64_t B, int64_t N, int P, int K) {
  if (K < 1 || K > kEvMax) return 0;
  const int64_t grid = masked_grid(B, N, P);
  if (grid == 0 || N > ((1ll << 31) - 1) / K || events_lds_bytes(P, K) > kEvMaxLds) return 0;
  return grid * (2 + (int64_t)(K + 1) * (K + 1)) * P * (int64_t)sizeof(double);
}

int dstagnn_events_accumulate(int64_t B, int64_t N, int P, int K, int above, const float* pred, const float* target,
                              int mask_mode, float null_val, const float* thr, int thr_per_node, double* htable,
                              double* ntable, void* scratch, size_t scratch_bytes, dstagnn_stream_t stream) {
  const std::string w("events_accumulate");
  int64_t grid = 0;
  if (int rc = horizon_arg(w, P, "last")) return rc;
  if (K < 1 || K > kEvMax)
    return fail(w + ": K (the number of thresholds) must be in [1, " + std::to_string(kEvMax) + "], got " +
                    std::to_string(K),
                DSTAGNN_E_SHAPE);
  if (int rc = strip_arg(w, B, N, P, 1, "B * N * P", &grid)) return rc;
  if (N > ((1ll << 31) - 1) / K) return fail(w + ": K * N must be below 2^31", DSTAGNN_E_SHAPE);
  const int64_t lds = events_lds_bytes(P, K);
  if (lds > kEvMaxLds)
    return fail(w + ": the histograms of P = " + std::to_string(P) + ", K = " + std::to_string(K) + " need " +
                    std::to_string(lds) + " bytes of LDS, more than " + std::to_string(kEvMaxLds),
                DSTAGNN_E_SHAPE);
  if (!pred || !target || !thr || !htable || !scratch)
    return fail(w + ": null pred / target / thr / htable / scratch", DSTAGNN_E_ARG);
  if (int rc = mask_arg(w, &mask_mode, null_val)) return rc;
  if (above < 0 || above > 1 || thr_per_node < 0 || thr_per_node > 1)
    return fail(w + ": above and thr_per_node must be 0 or 1, got " + std::to_string(above) + " and " +
                    std::to_string(thr_per_node),
                DSTAGNN_E_ARG);
  if (int rc = scratch_arg(w, scratch_bytes, dstagnn_events_scratch_bytes(B, N, P, K),
                           "dstagnn_events_scratch_bytes(B, N, P, K)"))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  int* ticket = ticket_arg(w, st);
  if (!ticket) return DSTAGNN_E_ARG;
  hipLaunchKernelGGL(events_kernel, dim3((unsigned)grid), dim3(kMetThreads), (size_t)lds, st, (int)B, (int)N, P, K,
                     above, pred, target, mask_mode, null_val, thr, thr_per_node, static_cast<double*>(scratch), ticket,
                     htable, ntable);
  DS_CHECK_LAUNCH();
  return 0;
}
