// optim.hip — the training driver's optimiser step on the GPU (gfx950): torch.optim.Adam
// (train_DSTAGNN_my.py:126, `optim.Adam(net.parameters(), lr=learning_rate)`, default betas /
// eps, no weight decay) over every parameter tensor of the model in ONE launch.
//
// torch's fused multi-tensor Adam splits a model's ~150 tensors over four launches of ~43 us
// each at PEMS08 (nb_block = 4: 2.6 M parameters, ~70 MB moved — ~10 us of HBM time), and
// its Python-side grouping leaves the GPU idle for ~0.2 ms before them
// (profiles/r04_model_step_*.txt).  Here the host hands over a table of (param, grad,
// exp_avg, exp_avg_sq, n) segments plus a chunk table ((segment, offset) per 4096 elements);
// a workgroup updates one chunk: every load of its 16 elements per thread first, then the
// update, then the stores.  Per element the arithmetic of torch's fused Adam
// (ATen/native/cuda/fused_adam_utils.cuh, ADAM_MODE::ORIGINAL) in fp32:
//   m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;
//   p -= step_size * m / (sqrt(v) / sqrt(1 - b2^t) + eps),  step_size = lr / (1 - b1^t)
//
// Opt-in extras on the same tables (nothing here runs unless asked for):
//   grad_sumsq_kernel  sum of g^2 over every listed gradient -> stat[0] (double), stat[1] = its
//                      root (the global L2 norm).  One workgroup per chunk: all 16 loads per
//                      thread, 16 sequential fp32 adds of the squares, the wave butterfly
//                      (6 adds), the four wave sums ((w0 + w1) + (w2 + w3)); the chunk's partial
//                      goes out sc1, and the workgroup whose ticket came last (the hand-off
//                      of handoff.hpp) adds all partials in fp64 in one fixed order: thread t
//                      takes partials t, t + 256, ... in index order, then a fixed LDS tree.  No
//                      workgroup waits for another; the same bits on every launch.
//   adam_ex_kernel     adam_kernel's body with, per element and in this order: g = coef g
//                      (coef = min(1, max_norm / (sqrt(stat[0]) + 1e-6)),
//                      torch.nn.utils.clip_grad_norm_), g += wd p (torch.optim.Adam's
//                      weight_decay) or p *= 1 - lr wd (torch.optim.AdamW); with skip_nonfinite
//                      and a non-finite stat[0] every workgroup returns before its first store.
//   grad_scale_kernel  g *= coef in place (the second half of a stand-alone clip_grad_norm_).
#include "handoff.hpp"
#include "ops.hpp"

namespace {

constexpr int kAdamThreads = 256, kAdamPer = 16, kAdamChunk = kAdamThreads * kAdamPer;

__global__ __launch_bounds__(kAdamThreads) void adam_kernel(const dstagnn_adam_seg* __restrict__ segs,
                                                            const int64_t* __restrict__ chunks, float b1, float b2,
                                                            float eps, float step_size, float bc2_sqrt) {
  const int64_t si = chunks[2 * (int64_t)blockIdx.x], off = chunks[2 * (int64_t)blockIdx.x + 1];
  const dstagnn_adam_seg s = segs[si];
  const int64_t end = min(off + (int64_t)kAdamChunk, s.n);
  float* __restrict__ p = s.p;
  const float* __restrict__ g = s.g;
  float* __restrict__ m = s.m;
  float* __restrict__ v = s.v;
  float gv[kAdamPer], mv[kAdamPer], vv[kAdamPer], pv[kAdamPer];
#pragma unroll
  for (int u = 0; u < kAdamPer; ++u) {
    const int64_t i = off + threadIdx.x + (int64_t)kAdamThreads * u;
    const bool ok = i < end;
    gv[u] = ok ? g[i] : 0.f;
    mv[u] = ok ? m[i] : 0.f;
    vv[u] = ok ? v[i] : 0.f;
    pv[u] = ok ? p[i] : 0.f;
  }
#pragma unroll
  for (int u = 0; u < kAdamPer; ++u) {
    const int64_t i = off + threadIdx.x + (int64_t)kAdamThreads * u;
    if (i >= end) continue;
    const float mm = b1 * mv[u] + (1.f - b1) * gv[u];
    const float vw = b2 * vv[u] + (1.f - b2) * gv[u] * gv[u];
    const float denom = sqrtf(vw) / bc2_sqrt + eps;
    m[i] = mm;
    v[i] = vw;
    p[i] = pv[u] - step_size * mm / denom;
  }
}

// torch.nn.utils.clip_grad_norm_'s coefficient, clamp(max_norm / (norm + 1e-6), max = 1) (a NaN
// stays NaN, as torch's clamp leaves it), from the fp64 sum of squares
__device__ __forceinline__ float clip_coef(double sumsq, float max_norm) {
  const double c = (double)max_norm / (sqrt(sumsq) + 1e-6);
  return c >= 1.0 ? 1.f : (float)c;
}

__global__ __launch_bounds__(kAdamThreads) void grad_sumsq_kernel(const dstagnn_adam_seg* __restrict__ segs,
                                                                 const int64_t* __restrict__ chunks,
                                                                 float* __restrict__ partials, int* ticket,
                                                                 double* __restrict__ stat) {
  __shared__ float wsum[kAdamThreads / 64];
  __shared__ double dred[kAdamThreads];
  __shared__ int last;
  const int t = threadIdx.x;
  const int64_t si = chunks[2 * (int64_t)blockIdx.x], off = chunks[2 * (int64_t)blockIdx.x + 1];
  const dstagnn_adam_seg s = segs[si];
  const int64_t end = min(off + (int64_t)kAdamChunk, s.n);
  const float* __restrict__ g = s.g;
  float gv[kAdamPer];
#pragma unroll
  for (int u = 0; u < kAdamPer; ++u) {
    const int64_t i = off + t + (int64_t)kAdamThreads * u;
    gv[u] = i < end ? g[i] : 0.f;
  }
  float acc = 0.f;
#pragma unroll
  for (int u = 0; u < kAdamPer; ++u) acc += gv[u] * gv[u];
  acc = wave_sum(acc);
  if ((t & 63) == 0) wsum[t >> 6] = acc;
  __syncthreads();
  // the hand-off of handoff.hpp: the last workgroup reads every partial (themselves sc1 loads)
  if (t == 0) st_agent(partials + blockIdx.x, (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]));
  if (!last_arrival(ticket, (int)gridDim.x, &last)) return;
  double a = 0.0;
  for (int64_t k = t; k < (int64_t)gridDim.x; k += kAdamThreads) a += (double)ld_agent(partials + k);
  dred[t] = a;
  __syncthreads();
#pragma unroll
  for (int w = kAdamThreads / 2; w > 0; w >>= 1) {
    if (t < w) dred[t] += dred[t + w];
    __syncthreads();
  }
  if (t == 0) {
    stat[0] = dred[0];
    stat[1] = sqrt(dred[0]);
  }
}

__global__ __launch_bounds__(kAdamThreads) void adam_ex_kernel(const dstagnn_adam_seg* __restrict__ segs,
                                                               const int64_t* __restrict__ chunks,
                                                               dstagnn_adam_hyper h, float decay,
                                                               const double* __restrict__ stat,
                                                               int* __restrict__ skipped) {
  float coef = 1.f;
  if (stat != nullptr) {  // (the host passes it exactly when clipping or skipping is on)
    const double sumsq = stat[0];
    if (h.skip_nonfinite && !__builtin_isfinite(sumsq)) {
      if (skipped != nullptr && blockIdx.x == 0 && threadIdx.x == 0) skipped[0] = skipped[0] + 1;
      return;
    }
    if (h.max_norm > 0.f) coef = clip_coef(sumsq, h.max_norm);
  }
  const float b1 = h.beta1, b2 = h.beta2, wd = h.decoupled ? 0.f : h.weight_decay;
  const int64_t si = chunks[2 * (int64_t)blockIdx.x], off = chunks[2 * (int64_t)blockIdx.x + 1];
  const dstagnn_adam_seg s = segs[si];
  const int64_t end = min(off + (int64_t)kAdamChunk, s.n);
  float* __restrict__ p = s.p;
  const float* __restrict__ g = s.g;
  float* __restrict__ m = s.m;
  float* __restrict__ v = s.v;
  float gv[kAdamPer], mv[kAdamPer], vv[kAdamPer], pv[kAdamPer];
#pragma unroll
  for (int u = 0; u < kAdamPer; ++u) {
    const int64_t i = off + threadIdx.x + (int64_t)kAdamThreads * u;
    const bool ok = i < end;
    gv[u] = ok ? g[i] : 0.f;
    mv[u] = ok ? m[i] : 0.f;
    vv[u] = ok ? v[i] : 0.f;
    pv[u] = ok ? p[i] : 0.f;
  }
#pragma unroll
  for (int u = 0; u < kAdamPer; ++u) {
    const int64_t i = off + threadIdx.x + (int64_t)kAdamThreads * u;
    if (i >= end) continue;
    const float gg = coef * gv[u] + wd * pv[u];
    const float pp = pv[u] * decay;
    const float mm = b1 * mv[u] + (1.f - b1) * gg;
    const float vw = b2 * vv[u] + (1.f - b2) * gg * gg;
    const float denom = sqrtf(vw) / h.bc2_sqrt + h.eps;
    m[i] = mm;
    v[i] = vw;
    p[i] = pp - h.step_size * mm / denom;
  }
}

__global__ __launch_bounds__(kAdamThreads) void grad_scale_kernel(const dstagnn_adam_seg* __restrict__ segs,
                                                                 const int64_t* __restrict__ chunks,
                                                                 const double* __restrict__ stat, float max_norm) {
  const float coef = clip_coef(stat[0], max_norm);
  if (coef == 1.f) return;  // below max_norm: the gradients keep their bits
  const int64_t si = chunks[2 * (int64_t)blockIdx.x], off = chunks[2 * (int64_t)blockIdx.x + 1];
  const dstagnn_adam_seg s = segs[si];
  const int64_t end = min(off + (int64_t)kAdamChunk, s.n);
  float* __restrict__ g = const_cast<float*>(s.g);
  float gv[kAdamPer];
#pragma unroll
  for (int u = 0; u < kAdamPer; ++u) {
    const int64_t i = off + threadIdx.x + (int64_t)kAdamThreads * u;
    gv[u] = i < end ? g[i] : 0.f;
  }
#pragma unroll
  for (int u = 0; u < kAdamPer; ++u) {
    const int64_t i = off + threadIdx.x + (int64_t)kAdamThreads * u;
    if (i < end) g[i] = coef * gv[u];
  }
}

bool tables_ok(const char* who, const dstagnn_adam_seg* segs, const int64_t* chunks, int nchunk) {
  if (nchunk < 0 || (nchunk > 0 && (!segs || !chunks))) {
    set_last_error(std::string(who) + ": null segment / chunk table");
    return false;
  }
  return true;
}

}  // namespace

int dstagnn_adam_chunk_elems(void) { return kAdamChunk; }

int dstagnn_adam_step(const dstagnn_adam_seg* segs, const int64_t* chunks, int nchunk, float beta1,
                        float beta2, float eps, float step_size, float bc2_sqrt, dstagnn_stream_t stream) {
  if (nchunk < 0 || (nchunk > 0 && (!segs || !chunks))) {
    set_last_error("adam_step: null segment / chunk table");
    return DSTAGNN_E_ARG;
  }
  if (nchunk == 0) return 0;
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)nchunk), dim3(kAdamThreads), 0, (hipStream_t)stream, segs, chunks,
                     beta1, beta2, eps, step_size, bc2_sqrt);
  DS_CHECK_LAUNCH();
  return 0;
}

int dstagnn_grad_sumsq(const dstagnn_adam_seg* segs, const int64_t* chunks, int nchunk, float* partials,
                       double* stat, dstagnn_stream_t stream) {
  if (!tables_ok("grad_sumsq", segs, chunks, nchunk)) return DSTAGNN_E_ARG;
  if (!stat || (nchunk > 0 && !partials)) {
    set_last_error("grad_sumsq: null partials / stat");
    return DSTAGNN_E_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  if (nchunk == 0) {  // no gradient: a zero norm
    hipError_t e = hipMemsetAsync(stat, 0, 2 * sizeof(double), st);
    if (e != hipSuccess) {
      set_last_error(std::string("grad_sumsq: ") + hipGetErrorString(e));
      return (int)e;
    }
    return 0;
  }
  int* ticket = stream_counters(st, 1);
  if (!ticket) {
    set_last_error("grad_sumsq: no ticket counter for this stream");
    return DSTAGNN_E_ARG;
  }
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)nchunk), dim3(kAdamThreads), 0, st, segs, chunks, partials,
                     ticket, stat);
  DS_CHECK_LAUNCH();
  return 0;
}

int dstagnn_adam_step_ex(const dstagnn_adam_seg* segs, const int64_t* chunks, int nchunk,
                         const dstagnn_adam_hyper* hyper, const double* stat, int* skipped,
                         dstagnn_stream_t stream) {
  if (!tables_ok("adam_step_ex", segs, chunks, nchunk)) return DSTAGNN_E_ARG;
  if (!hyper) {
    set_last_error("adam_step_ex: null hyper-parameters");
    return DSTAGNN_E_ARG;
  }
  const dstagnn_adam_hyper h = *hyper;
  if (!(h.weight_decay >= 0.f) || !(h.max_norm >= 0.f)) {
    set_last_error("adam_step_ex: negative weight_decay / max_norm");
    return DSTAGNN_E_ARG;
  }
  const bool need_stat = h.max_norm > 0.f || h.skip_nonfinite;
  if (need_stat && !stat) {
    set_last_error("adam_step_ex: clipping / non-finite skip need stat (dstagnn_grad_sumsq)");
    return DSTAGNN_E_ARG;
  }
  if (nchunk == 0) return 0;
  // torch.optim.AdamW: param.mul_(1 - lr * weight_decay), the factor formed in double
  const float decay = h.decoupled ? (float)(1.0 - (double)h.lr * (double)h.weight_decay) : 1.f;
  hipLaunchKernelGGL(adam_ex_kernel, dim3((unsigned)nchunk), dim3(kAdamThreads), 0, (hipStream_t)stream, segs, chunks,
                     h, decay, need_stat ? stat : nullptr, skipped);
  DS_CHECK_LAUNCH();
  return 0;
}

int dstagnn_grad_scale(const dstagnn_adam_seg* segs, const int64_t* chunks, int nchunk, const double* stat,
                       float max_norm, dstagnn_stream_t stream) {
  if (!tables_ok("grad_scale", segs, chunks, nchunk)) return DSTAGNN_E_ARG;
  if (!stat || !(max_norm > 0.f)) {
    set_last_error("grad_scale: null stat / max_norm <= 0");
    return DSTAGNN_E_ARG;
  }
  if (nchunk == 0) return 0;
  hipLaunchKernelGGL(grad_scale_kernel, dim3((unsigned)nchunk), dim3(kAdamThreads), 0, (hipStream_t)stream, segs,
                     chunks, stat, max_norm);
  DS_CHECK_LAUNCH();
  return 0;
}
