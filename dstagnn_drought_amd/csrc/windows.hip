// windows.hip — the data side of a training step on the GPU (gfx950): a batch's input windows and
// targets cut straight from the raw (L, N, F) series, and the z-score statistics of a split.
// Replaces, per batch, what prepareData.py materialises once for every label position
// (prepareData.py:63-147 read_and_generate_dataset, :149-161 normalization) and what
// lib/utils1.py:294-343 load_graphdata_channel1 then copies to the device whole.
//
//   window_gather_kernel<S>  one launch per batch, S = the series' dtype (float / double).
//       x[b, n, f, t] = float((S(series[label_b + rel[t], n, f]) - mean[f]) / std[f])
//       y[b, n, p]    = float(series[label_b + p, n, F - 1]),  label_b = labels[idx[b]]
//     (subtraction and division in S, one rounding to fp32 at the end: numpy's
//     `(x - mean) / std` followed by `.type(torch.FloatTensor)`).  A workgroup owns a tile of TN
//     consecutive nodes of one sample.  For a fixed t the tile's source is ONE contiguous run of
//     tn F elements (read with consecutive lanes on consecutive elements); its destination in
//     x[b] is ONE contiguous run of tn F Tin floats.  The transpose happens in LDS: element
//     (e, t), e = nl F + f, is stored at the position o = e Tin + t it has in the output run,
//     at address o + o / 32 (one pad dword per 32: the stores of one row are Tin dwords apart,
//     a 4-way (Tin = 12) to 16-way (Tin = 144) conflict on the linear image, 2-way and at most
//     3-way on the padded one; the four dwords a lane then collects for its float4 sit at
//     4 l + j + l / 8: the 32 lanes of a group on 32 different banks, 2-way at worst behind a
//     scalar head; counted lane by lane in DESIGN.md §12).  The run goes out as
//     float4 from the first 16-byte boundary on, with a scalar head and tail around it
//     (N F Tin odd: x[b] itself is not 16-byte aligned for odd b).  The targets take the same
//     road through a second, small LDS image (their source is strided by F, their run by P).
//     An idx[b] outside [0, S) or a time step outside [0, L) is never dereferenced: that sample
//     (that row) is NaN.  All offsets are 64-bit.
//   window_stats_kernel<S>   the training split's mean and standard deviation (ddof = 0) per
//     feature over its windows, axes (0, 1, 3), as the weighted moments of the raw series:
//     w[s] = how many (training label, window offset) pairs land on time step s (host-made, L
//     int32).  Two launches: sum w x, then sum w (x - mean)^2 around that mean (never the
//     sum-of-squares form).  A workgroup takes whole time steps s = wg, wg + grid, ... (w[s] is
//     uniform; a step of weight 0 is skipped unread), thread t of the first (256 / F) F reads
//     elements t, t + A, ... of the step (its feature never changes), every add in fp64.  The
//     workgroup folds its threads of equal feature in thread order, hands {F sums} off
//     (handoff.hpp) and the last arrival adds the partials in workgroup order: the same bits on
//     every call.  stats = {mean[F], std[F]} in fp64.
//
// Series with gaps (an element is missing when it is NaN, or equals a sentinel: win_missing):
//   window_gather_kernel<S, true, NANMODE>  the same gather with the inputs read from a second
//     source (the raw series, or its forward fill) and a select: a missing input becomes +0.0f,
//     the training mean in z-score units; the targets stay raw, marker included, for the masked
//     loss.  Same tile, LDS image and write-out: the same bytes moved.
//   window_stats_kernel<S, true>   the same sums over the valid elements only, divided by the valid
//     weight wvalid[f] = sum_s w[s] #valid(s, ., f), which is counted in int64 through the same
//     fold (exact in any order).  Same threads and fp64 add order: with nothing missing, the bits of
//     the unmasked kernel.
//   window_fill_last_kernel / window_fill_kernel<S>  the one-time forward fill along time, a max-scan
//     over L for the N F independent columns e = n F + f.  Time is cut into chunks of kFillChunk
//     steps; a workgroup owns kFillCols consecutive columns of one chunk, one per thread, so every
//     row access is one contiguous run.  Launch 1 writes the last valid step of each (chunk,
//     column), or -1, into an int32 table.  Launch 2 finds its carry by walking the table backwards
//     from its chunk (one read per earlier chunk, stopped at the first hit and where max_gap can no
//     longer reach), loads that one value, then walks its chunk forward and stores.  Nothing later
//     than s is ever read for step s.  Missing / filled counts per feature: LDS integer atomics,
//     then one global atomic per feature and workgroup (integers: exact in any order).
//
// The seasonal baseline of the skill scores (loss.hip skill_kernel):
//   climatology_kernel<S, MASKED>  clim (period, N) fp64 and cnt (period, N) int32: the mean of the
//     observed target feature over the training steps of each phase t mod period, one thread per
//     (phase, node), sequential in t: the same bits on every call.
#include <cmath>

#include "handoff.hpp"
#include "ops.hpp"

namespace {

constexpr int kWinThreads = 256, kWinUnroll = 4;
constexpr int kWinImageFloats = 8192;  // the padded x image of a tile: <= 32 KiB
constexpr int kWinMaxTile = 64;        // nodes; F = 1 rows are then 64 elements, one per lane
constexpr int kWinMaxLds = 64 << 10;   // x image + targets + row table: two workgroups per CU at worst
constexpr int kStatThreads = 256, kStatMaxWg = 512, kStatMaxF = 256;
constexpr int kFillChunk = 64, kFillCols = 256, kFillUnroll = 4;

// nan_mode: v is NaN; otherwise v == null (IEEE ==, as loss.hip's is_valid: -0.0 == 0.0)
template <typename S>
__device__ __forceinline__ bool win_missing(S v, S null, int nan_mode) {
  return nan_mode ? v != v : v == null;
}

__host__ __device__ __forceinline__ int win_pad(int o) { return o + (o >> 5); }

// nodes per tile: the most whose padded image fits kWinImageFloats, at most kWinMaxTile
int win_tile_nodes(int F, int Tin) {
  const int64_t per = (int64_t)F * Tin;  // floats of one node
  const int64_t tn = (int64_t)kWinImageFloats * 32 / 33 / per;
  return (int)(tn < 1 ? 1 : tn > kWinMaxTile ? kWinMaxTile : tn);
}

struct WinArgs {
  const void* series;  // the targets' source; the inputs' too unless MASKED
  int64_t L;
  int N, F, Tin, P, TN, ntile;
  int ximage;  // floats of the padded x image (the target image starts there)
  const int32_t* rel;
  const int64_t* labels;
  int64_t S;
  const int64_t* idx;
  const void *mean, *std;
  float *x, *y;
  const void* xseries;  // MASKED: the inputs' source (the raw series or its forward fill)
  double null_val;      // MASKED, not NANMODE: the missing marker
};

// MASKED: the gap-aware variant; NANMODE (with MASKED): the marker is NaN, else a.null_val.  The
// marker's kind is a template argument so that the select costs one compare per element.
template <typename S, bool MASKED, bool NANMODE = false>
__global__ __launch_bounds__(kWinThreads) void window_gather_kernel(WinArgs a) {
  extern __shared__ float win_lds[];
  float* xim = win_lds;
  float* yim = win_lds + a.ximage;
  int* srow = reinterpret_cast<int*>(yim + a.TN * a.P);  // time step of row t, -1: not in the series
  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.ntile, tile = blockIdx.x - b * a.ntile;
  const int n0 = tile * a.TN, tn = min(a.TN, a.N - n0);
  const int cnt = tn * a.F, run = cnt * a.Tin, yrun = tn * a.P;
  const S* __restrict__ series = static_cast<const S*>(a.series);
  const S* __restrict__ mean = static_cast<const S*>(a.mean);
  const S* __restrict__ sd = static_cast<const S*>(a.std);
  const int64_t NF = (int64_t)a.N * a.F;
  const float nanv = __builtin_nanf("");

  const int64_t i = a.idx[b];
  const bool ok = i >= 0 && i < a.S;
  const int64_t label = ok ? a.labels[i] : 0;
  for (int t = tid; t < a.Tin; t += kWinThreads) {
    const int64_t s = label + a.rel[t];
    srow[t] = ok && s >= 0 && s < a.L ? (int)s : -1;
  }
  __syncthreads();

  // stage: row t of the tile is cnt consecutive elements; j = t cnt + e walks the rows in order
  // (t, e, f = e % F) of j are carried from j to j + 256 without a division: cnt is a multiple of F
  const S* __restrict__ src = series + (int64_t)n0 * a.F;
  const S* __restrict__ xsrc = MASKED ? static_cast<const S*>(a.xseries) + (int64_t)n0 * a.F : src;
  const S nullv = MASKED ? (S)a.null_val : S(0);
  const int tstep = kWinThreads / cnt, estep = kWinThreads - tstep * cnt, fstep = estep % a.F;  // (uniform)
  int t = tid / cnt, e = tid - t * cnt, f = e % a.F;
  for (int j0 = tid; j0 < run; j0 += kWinThreads * kWinUnroll) {
    S v[kWinUnroll], mu[kWinUnroll], sg[kWinUnroll];
    int tt[kWinUnroll], ee[kWinUnroll], ff[kWinUnroll], ss[kWinUnroll];
#pragma unroll
    for (int u = 0; u < kWinUnroll; ++u) {
      tt[u] = t, ee[u] = e, ff[u] = f;
      ss[u] = j0 + u * kWinThreads < run ? srow[t] : -1;
      v[u] = ss[u] >= 0 ? xsrc[(int64_t)ss[u] * NF + e] : S(0);
      if constexpr (MASKED) mu[u] = mean[f], sg[u] = sd[f];  // (f < F always) in flight with the row loads
      t += tstep, e += estep, f += fstep;
      if (e >= cnt) e -= cnt, ++t;
      if (f >= a.F) f -= a.F;
    }
#pragma unroll
    for (int u = 0; u < kWinUnroll; ++u) {
      if (j0 + u * kWinThreads < run) {
        float z;
        if constexpr (MASKED) {
          z = ss[u] >= 0 ? (float)((v[u] - mu[u]) / sg[u]) : nanv;
          if (ss[u] >= 0 && win_missing(v[u], nullv, NANMODE ? 1 : 0)) z = 0.0f;  // the training mean
        } else {
          z = ss[u] >= 0 ? (float)((v[u] - mean[ff[u]]) / sd[ff[u]]) : nanv;
        }
        xim[win_pad(ee[u] * a.Tin + tt[u])] = z;
      }
    }
  }
  // the targets: steps label .. label + P - 1 of the last feature, un-normalised
  const bool tgt = ok && label >= 0 && label + a.P <= a.L;
  for (int j = tid; j < yrun; j += kWinThreads) {
    const int p = j / tn, nl = j - p * tn;
    yim[nl * a.P + p] = tgt ? (float)src[(label + p) * NF + (int64_t)nl * a.F + (a.F - 1)] : nanv;
  }
  __syncthreads();

  // x[b, n0 .. n0 + tn): one run of `run` floats; float4 from its first 16-byte boundary
  float* __restrict__ xo = a.x + ((int64_t)b * a.N + n0) * a.F * a.Tin;
  const int head = min(run, (int)((4 - ((reinterpret_cast<uintptr_t>(xo) >> 2) & 3)) & 3));
  const int nvec = (run - head) >> 2;
  if (tid < head) xo[tid] = xim[win_pad(tid)];
  float4* __restrict__ x4 = reinterpret_cast<float4*>(xo + head);
  for (int q = tid; q < nvec; q += kWinThreads) {
    const int o = head + 4 * q;
    float4 r;
    r.x = xim[win_pad(o)], r.y = xim[win_pad(o + 1)], r.z = xim[win_pad(o + 2)], r.w = xim[win_pad(o + 3)];
    x4[q] = r;
  }
  {
    const int o = head + 4 * nvec + tid;
    if (o < run) xo[o] = xim[win_pad(o)];
  }
  float* __restrict__ yo = a.y + ((int64_t)b * a.N + n0) * a.P;
  for (int j = tid; j < yrun; j += kWinThreads) yo[j] = yim[j];
}

// pass 0: stats[f] = sum w x / wtotal; pass 1: stats[F + f] = sqrt(sum w (x - stats[f])^2 / wtotal)
// MASKED: the sums skip the missing elements; pass 0 also counts wvalid[f] = sum w over the valid
// ones (int64 partials behind the fp64 ones in `part`, the same hand-off) and both passes divide by
// it instead of wtotal
template <typename S, bool MASKED>
__global__ __launch_bounds__(kStatThreads) void window_stats_kernel(const S* __restrict__ series, int64_t L,
                                                                  int64_t NF, int F, const int32_t* __restrict__ w,
                                                                  int pass, double wtotal, double* __restrict__ part,
                                                                  int* ticket, double* stats, double null_val,
                                                                  int null_nan, long long* wvalid) {
  __shared__ double red[kStatThreads];
  __shared__ int last;
  const int t = threadIdx.x;
  const int RL = kStatThreads / F, A = RL * F;  // threads that read; e = t + k A keeps feature t % F
  const S nullv = MASKED ? (S)null_val : S(0);
  long long* cpart = MASKED ? reinterpret_cast<long long*>(part + (int64_t)gridDim.x * F) : nullptr;  // (pass 0)
  long long cnt = 0;
  double acc = 0.0;
  if (t < A) {
    const double m = pass ? stats[t % F] : 0.0;
    for (int64_t s = blockIdx.x; s < L; s += gridDim.x) {
      const int wi = w[s];
      if (wi == 0) continue;  // (uniform)
      const double wd = (double)wi;
      const S* __restrict__ row = series + s * NF;
      if (pass) {
        for (int64_t e = t; e < NF; e += A) {
          const S v = row[e];
          const double d = (double)v - m;
          if (!MASKED || !win_missing(v, nullv, null_nan)) acc += wd * (d * d);
        }
      } else {
        for (int64_t e = t; e < NF; e += A) {
          const S v = row[e];
          if (!MASKED || !win_missing(v, nullv, null_nan)) {
            acc += wd * (double)v;
            if (MASKED) cnt += wi;
          }
        }
      }
    }
  }
  red[t] = acc;
  __syncthreads();
  if (t < F) {
    double a = 0.0;
    for (int r = 0; r < RL; ++r) a += red[r * F + t];
    st_agent(part + (int64_t)blockIdx.x * F + t, a);
  }
  if constexpr (MASKED) {
    if (!pass) {  // (uniform)
      __shared__ long long redc[kStatThreads];
      redc[t] = cnt;
      __syncthreads();
      if (t < F) {
        long long c = 0;
        for (int r = 0; r < RL; ++r) c += redc[r * F + t];
        st_agent(cpart + (int64_t)blockIdx.x * F + t, c);
      }
    }
  }
  if (!last_arrival(ticket, (int)gridDim.x, &last)) return;
  if (t < F) {
    double a = 0.0;
    for (int64_t k = 0; k < (int64_t)gridDim.x; ++k) a += ld_agent(part + k * F + t);
    double div = wtotal;
    if constexpr (MASKED) {
      if (!pass) {
        long long c = 0;
        for (int64_t k = 0; k < (int64_t)gridDim.x; ++k) c += ld_agent(cpart + k * F + t);
        wvalid[t] = c;
        div = (double)c;
      } else {
        div = (double)wvalid[t];  // (the first launch's, stream order)
      }
    }
    if (pass) stats[F + t] = sqrt(a / div);
    else stats[t] = a / div;
  }
}

// launch 1 of the forward fill: last[c E + e] = the last valid step of column e in chunk c, or -1
template <typename S>
__global__ __launch_bounds__(kFillCols) void window_fill_last_kernel(const S* __restrict__ series, int64_t L,
                                                                   int64_t E, int ncolblk, double null_val,
                                                                   int null_nan, int32_t* __restrict__ last) {
  const int64_t c = blockIdx.x / ncolblk;
  const int64_t e = (int64_t)(blockIdx.x - c * ncolblk) * kFillCols + threadIdx.x;
  if (e >= E) return;
  const S nullv = (S)null_val;
  const int64_t s0 = c * kFillChunk, s1 = min(L, s0 + kFillChunk);
  int p = -1;
  for (int64_t s = s0; s < s1; s += kFillUnroll) {
    S v[kFillUnroll];
#pragma unroll
    for (int u = 0; u < kFillUnroll; ++u) v[u] = s + u < s1 ? series[(s + u) * E + e] : nullv;
#pragma unroll
    for (int u = 0; u < kFillUnroll; ++u)
      if (s + u < s1 && !win_missing(v[u], nullv, null_nan)) p = (int)(s + u);
  }
  last[c * E + e] = p;
}

// launch 2: the carry from the table, then the chunk forward.  gap: the furthest a value is carried
// (>= L: unlimited).  counts (2, F): missing, filled.
template <typename S>
__global__ __launch_bounds__(kFillCols) void window_fill_kernel(const S* __restrict__ series, int64_t L, int64_t E,
                                                              int F, int ncolblk, double null_val, int null_nan,
                                                              int64_t gap, const int32_t* __restrict__ last,
                                                              S* __restrict__ out, unsigned long long* counts) {
  __shared__ unsigned long long lc[2 * kStatMaxF];
  const int tid = threadIdx.x;
  for (int i = tid; i < 2 * F; i += kFillCols) lc[i] = 0;
  __syncthreads();
  const int64_t c = blockIdx.x / ncolblk;
  const int64_t e = (int64_t)(blockIdx.x - c * ncolblk) * kFillCols + tid;
  if (e < E) {
    const S nullv = (S)null_val;
    const int64_t s0 = c * kFillChunk, s1 = min(L, s0 + kFillChunk);
    int64_t p = -1;
    for (int64_t k = c - 1; k >= 0; --k) {
      if (s0 - ((k + 1) * kFillChunk - 1) > gap) break;  // chunk k's last step no longer reaches s0
      p = last[k * E + e];
      if (p >= 0) break;
    }
    S pv = p >= 0 ? series[p * E + e] : nullv;
    unsigned miss = 0, fill = 0;
    for (int64_t s = s0; s < s1; s += kFillUnroll) {
      S v[kFillUnroll];
#pragma unroll
      for (int u = 0; u < kFillUnroll; ++u) v[u] = s + u < s1 ? series[(s + u) * E + e] : nullv;
#pragma unroll
      for (int u = 0; u < kFillUnroll; ++u) {
        if (s + u >= s1) break;
        S o = v[u];
        if (win_missing(o, nullv, null_nan)) {
          ++miss;
          if (p >= 0 && s + u - p <= gap) o = pv, ++fill;
        } else {
          p = s + u, pv = o;
        }
        out[(s + u) * E + e] = o;
      }
    }
    const int f = (int)(e % F);
    if (miss) atomicAdd(&lc[f], (unsigned long long)miss);
    if (fill) atomicAdd(&lc[F + f], (unsigned long long)fill);
  }
  __syncthreads();
  for (int i = tid; i < 2 * F; i += kFillCols)
    if (lc[i]) atomicAdd(counts + i, lc[i]);
}

int64_t stats_grid(int64_t L) { return L < 1 ? 1 : L > kStatMaxWg ? kStatMaxWg : L; }

// The seasonal climatology of the target feature over the training steps [0, t_end): one thread per
// (phase, node), n fastest (for a fixed t the lanes of a wave read elements F apart in one row),
// walking t = phase, phase + period, ... in order with kClimUnroll loads in flight.  Each value is
// converted to double and added in increasing t; one division.  MASKED: the missing elements are
// skipped.  A (phase, node) with no observed value: clim = NaN, cnt = 0.
constexpr int kClimThreads = 256, kClimUnroll = 4;

template <typename S, bool MASKED>
__global__ __launch_bounds__(kClimThreads) void climatology_kernel(const S* __restrict__ series, int64_t NF, int N,
                                                                  int F, int period, int64_t t_end, double null_val,
                                                                  int null_nan, double* __restrict__ clim,
                                                                  int32_t* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * kClimThreads + threadIdx.x;
  if (i >= (int64_t)period * N) return;
  const int phase = (int)(i / N), n = (int)(i - (int64_t)phase * N);
  const S nullv = MASKED ? (S)null_val : S(0);
  const S* __restrict__ col = series + (int64_t)n * F + (F - 1);
  double sum = 0.0;
  int c = 0;
  for (int64_t t = phase; t < t_end; t += (int64_t)period * kClimUnroll) {
    S v[kClimUnroll];
#pragma unroll
    for (int u = 0; u < kClimUnroll; ++u) {
      const int64_t tu = t + (int64_t)u * period;
      v[u] = tu < t_end ? col[tu * NF] : nullv;
    }
#pragma unroll
    for (int u = 0; u < kClimUnroll; ++u) {
      const int64_t tu = t + (int64_t)u * period;
      if (tu < t_end && !(MASKED && win_missing(v[u], nullv, null_nan))) sum += (double)v[u], ++c;
    }
  }
  clim[i] = c > 0 ? sum / (double)c : __builtin_nan("");
  cnt[i] = c;
}

template <typename S>
void launch_climatology(const void* series, int64_t N, int64_t F, int64_t period, int64_t t_end, int masked,
                        double null_val, double* clim, int32_t* cnt, hipStream_t st) {
  const dim3 grid((unsigned)((period * N + kClimThreads - 1) / kClimThreads)), block(kClimThreads);
  const int null_nan = std::isnan(null_val) ? 1 : 0;
  if (masked)
    hipLaunchKernelGGL((climatology_kernel<S, true>), grid, block, 0, st, static_cast<const S*>(series), N * F, (int)N,
                       (int)F, (int)period, t_end, null_val, null_nan, clim, cnt);
  else
    hipLaunchKernelGGL((climatology_kernel<S, false>), grid, block, 0, st, static_cast<const S*>(series), N * F, (int)N,
                       (int)F, (int)period, t_end, 0.0, 0, clim, cnt);
}

}  // namespace

int dstagnn_climatology(int series_f64, const void* series, int64_t L, int64_t N, int64_t F, int64_t period,
                        int64_t t_end, int masked, double null_val, double* clim, int32_t* cnt,
                        dstagnn_stream_t stream) {
  const int64_t lim = (1ll << 31) - 1;
  if (L < 1 || N < 1 || F < 1 || N > lim / L || F > lim / (L * N)) {
    set_last_error("climatology: L, N and F must be >= 1 and L * N * F below 2^31");
    return DSTAGNN_E_SHAPE;
  }
  if (period < 1 || period > L || period > lim / N) {
    set_last_error("climatology: period must be in [1, L] and period * N below 2^31, got " + std::to_string(period));
    return DSTAGNN_E_SHAPE;
  }
  if (t_end < 1 || t_end > L) {
    set_last_error("climatology: t_end (the end of the training steps) must be in [1, L], got " +
                   std::to_string(t_end));
    return DSTAGNN_E_SHAPE;
  }
  if (!series || !clim || !cnt) {
    set_last_error("climatology: null series / clim / cnt");
    return DSTAGNN_E_ARG;
  }
  if (!masked && std::isnan(null_val)) {
    set_last_error("climatology: a NaN null_val needs masked = 1");
    return DSTAGNN_E_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  if (series_f64) launch_climatology<double>(series, N, F, period, t_end, masked, null_val, clim, cnt, st);
  else launch_climatology<float>(series, N, F, period, t_end, masked, null_val, clim, cnt, st);
  DS_CHECK_LAUNCH();
  return 0;
}

int dstagnn_window_tile_nodes(int F, int Tin) { return F < 1 || Tin < 1 ? 0 : win_tile_nodes(F, Tin); }

int64_t dstagnn_window_gather_lds_bytes(int F, int Tin, int P) {
  if (F < 1 || Tin < 1 || P < 1) return 0;
  const int64_t TN = win_tile_nodes(F, Tin);
  const int64_t run = TN * F * Tin;
  return 4 * (run + (run >> 5) + 1 + TN * P + Tin);
}

namespace {

// both gathers: xsrc null = the plain one (inputs and targets from `series`)
int launch_gather(const std::string& who, int series_f64, const void* xsrc, const void* series, int64_t L, int N, int F,
                  const int32_t* rel, int Tin, int P, const int64_t* labels, int64_t S, const int64_t* idx, int B,
                  const void* mean, const void* std, double null_val, float* x, float* y, dstagnn_stream_t stream) {
  if (!series || !rel || !labels || !idx || !mean || !std || !x || !y) {
    set_last_error(who + ": null series / rel / labels / idx / mean / std / x / y");
    return DSTAGNN_E_ARG;
  }
  if (L < 1 || L >= (1ll << 31) || N < 1 || F < 1 || Tin < 1 || P < 1 || S < 1 || B < 1) {
    set_last_error(who + ": L (< 2^31), N, F, Tin, P, S and B must all be >= 1");
    return DSTAGNN_E_SHAPE;
  }
  const int64_t lds = dstagnn_window_gather_lds_bytes(F, Tin, P);
  if ((int64_t)F * Tin >= (1 << 24) || lds > kWinMaxLds) {
    set_last_error(who + ": one node's window (F * Tin floats) and its targets need " + std::to_string(lds) +
                   " bytes of LDS, over " + std::to_string(kWinMaxLds));
    return DSTAGNN_E_SHAPE;
  }
  WinArgs a{};
  a.series = series, a.xseries = xsrc, a.null_val = null_val;
  a.L = L, a.N = N, a.F = F, a.Tin = Tin, a.P = P;
  a.TN = win_tile_nodes(F, Tin);
  a.ntile = (N + a.TN - 1) / a.TN;
  const int64_t run = (int64_t)a.TN * F * Tin;
  a.ximage = (int)(run + (run >> 5) + 1);
  a.rel = rel, a.labels = labels, a.S = S, a.idx = idx, a.mean = mean, a.std = std, a.x = x, a.y = y;
  const int64_t grid = (int64_t)B * a.ntile;
  if (grid >= (1ll << 31)) {
    set_last_error(who + ": B * tiles must be below 2^31");
    return DSTAGNN_E_SHAPE;
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 g((unsigned)grid), b(kWinThreads);
  if (xsrc && std::isnan(null_val)) {
    if (series_f64) hipLaunchKernelGGL((window_gather_kernel<double, true, true>), g, b, (size_t)lds, st, a);
    else hipLaunchKernelGGL((window_gather_kernel<float, true, true>), g, b, (size_t)lds, st, a);
  } else if (xsrc) {
    if (series_f64) hipLaunchKernelGGL((window_gather_kernel<double, true, false>), g, b, (size_t)lds, st, a);
    else hipLaunchKernelGGL((window_gather_kernel<float, true, false>), g, b, (size_t)lds, st, a);
  } else {
    if (series_f64) hipLaunchKernelGGL((window_gather_kernel<double, false>), g, b, (size_t)lds, st, a);
    else hipLaunchKernelGGL((window_gather_kernel<float, false>), g, b, (size_t)lds, st, a);
  }
  DS_CHECK_LAUNCH();
  return 0;
}

}  // namespace

int dstagnn_window_gather(int series_f64, const void* series, int64_t L, int N, int F, const int32_t* rel, int Tin,
                          int P, const int64_t* labels, int64_t S, const int64_t* idx, int B, const void* mean,
                          const void* std, float* x, float* y, dstagnn_stream_t stream) {
  return launch_gather("window_gather", series_f64, nullptr, series, L, N, F, rel, Tin, P, labels, S, idx, B, mean, std,
                       0.0, x, y, stream);
}

int dstagnn_window_gather_masked(int series_f64, const void* xsrc, const void* ysrc, int64_t L, int N, int F,
                                 const int32_t* rel, int Tin, int P, const int64_t* labels, int64_t S,
                                 const int64_t* idx, int B, const void* mean, const void* std, double null_val, float* x,
                                 float* y, dstagnn_stream_t stream) {
  if (!xsrc) {
    set_last_error("window_gather_masked: null xsrc");
    return DSTAGNN_E_ARG;
  }
  return launch_gather("window_gather_masked", series_f64, xsrc, ysrc, L, N, F, rel, Tin, P, labels, S, idx, B, mean,
                       std, null_val, x, y, stream);
}

int64_t dstagnn_window_stats_scratch_bytes(int64_t L, int F) {
  if (L < 1 || F < 1 || F > kStatMaxF) return 0;
  return stats_grid(L) * (int64_t)F * (int64_t)sizeof(double);
}

namespace {

// both statistics: wvalid null = the plain one (divides by wtotal)
template <typename S>
int launch_stats(const void* series, int64_t L, int N, int F, const int32_t* w, double wtotal, double null_val,
                 double* stats, int64_t* wvalid, void* scratch, hipStream_t st, int* ticket) {
  const dim3 grid((unsigned)stats_grid(L)), block(kStatThreads);
  const int64_t NF = (int64_t)N * F;
  const int null_nan = std::isnan(null_val) ? 1 : 0;
  for (int pass = 0; pass < 2; ++pass) {  // the second launch reads the first one's mean (stream order)
    if (wvalid)
      hipLaunchKernelGGL((window_stats_kernel<S, true>), grid, block, 0, st, static_cast<const S*>(series), L, NF, F, w,
                         pass, wtotal, static_cast<double*>(scratch), ticket, stats, null_val, null_nan,
                         reinterpret_cast<long long*>(wvalid));
    else
      hipLaunchKernelGGL((window_stats_kernel<S, false>), grid, block, 0, st, static_cast<const S*>(series), L, NF, F,
                         w, pass, wtotal, static_cast<double*>(scratch), ticket, stats, 0.0, 0,
                         static_cast<long long*>(nullptr));
    DS_CHECK_LAUNCH();
  }
  return 0;
}

}  // namespace

int dstagnn_window_stats(int series_f64, const void* series, int64_t L, int N, int F, const int32_t* w, double wtotal,
                         double* stats, void* scratch, size_t scratch_bytes, dstagnn_stream_t stream) {
  if (!series || !w || !stats || !scratch) {
    set_last_error("window_stats: null series / w / stats / scratch");
    return DSTAGNN_E_ARG;
  }
  if (F < 1 || F > kStatMaxF || L < 1 || N < 1) {
    set_last_error("window_stats: L, N >= 1 and F in [1, 256], got F = " + std::to_string(F));
    return DSTAGNN_E_SHAPE;
  }
  if (!(wtotal > 0.0)) {
    set_last_error("window_stats: the total weight must be positive (an empty training split?)");
    return DSTAGNN_E_ARG;
  }
  if (scratch_bytes < (size_t)dstagnn_window_stats_scratch_bytes(L, F)) {
    set_last_error("window_stats: scratch smaller than dstagnn_window_stats_scratch_bytes(L, F)");
    return DSTAGNN_E_SPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  int* ticket = stream_counters(st, 1);
  if (!ticket) {
    set_last_error("window_stats: no ticket counter for this stream");
    return DSTAGNN_E_ARG;
  }
  return series_f64 ? launch_stats<double>(series, L, N, F, w, wtotal, 0.0, stats, nullptr, scratch, st, ticket)
                    : launch_stats<float>(series, L, N, F, w, wtotal, 0.0, stats, nullptr, scratch, st, ticket);
}

int64_t dstagnn_window_stats_masked_scratch_bytes(int64_t L, int F) {  // fp64 sums, then int64 counts
  return 2 * dstagnn_window_stats_scratch_bytes(L, F);
}

int dstagnn_window_stats_masked(int series_f64, const void* series, int64_t L, int N, int F, const int32_t* w,
                                double null_val, double* stats, int64_t* wvalid, void* scratch, size_t scratch_bytes,
                                dstagnn_stream_t stream) {
  if (!series || !w || !stats || !wvalid || !scratch) {
    set_last_error("window_stats_masked: null series / w / stats / wvalid / scratch");
    return DSTAGNN_E_ARG;
  }
  if (F < 1 || F > kStatMaxF || L < 1 || N < 1) {
    set_last_error("window_stats_masked: L, N >= 1 and F in [1, 256], got F = " + std::to_string(F));
    return DSTAGNN_E_SHAPE;
  }
  if (scratch_bytes < (size_t)dstagnn_window_stats_masked_scratch_bytes(L, F)) {
    set_last_error("window_stats_masked: scratch smaller than dstagnn_window_stats_masked_scratch_bytes(L, F)");
    return DSTAGNN_E_SPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  int* ticket = stream_counters(st, 1);
  if (!ticket) {
    set_last_error("window_stats_masked: no ticket counter for this stream");
    return DSTAGNN_E_ARG;
  }
  return series_f64 ? launch_stats<double>(series, L, N, F, w, 1.0, null_val, stats, wvalid, scratch, st, ticket)
                    : launch_stats<float>(series, L, N, F, w, 1.0, null_val, stats, wvalid, scratch, st, ticket);
}

int dstagnn_window_fill_chunk(void) { return kFillChunk; }
int dstagnn_window_fill_cols(void) { return kFillCols; }

int64_t dstagnn_window_fill_scratch_bytes(int64_t L, int N, int F) {
  if (L < 1 || N < 1 || F < 1) return 0;
  return (L + kFillChunk - 1) / kFillChunk * (int64_t)N * F * (int64_t)sizeof(int32_t);
}

namespace {

template <typename S>
int launch_fill(const void* series, int64_t L, int64_t E, int F, int ncolblk, unsigned grid, double null_val,
                int64_t gap, void* filled, int64_t* counts, void* scratch, hipStream_t st) {
  const int null_nan = std::isnan(null_val) ? 1 : 0;
  hipLaunchKernelGGL(window_fill_last_kernel<S>, dim3(grid), dim3(kFillCols), 0, st, static_cast<const S*>(series), L,
                     E, ncolblk, null_val, null_nan, static_cast<int32_t*>(scratch));
  DS_CHECK_LAUNCH();
  hipLaunchKernelGGL(window_fill_kernel<S>, dim3(grid), dim3(kFillCols), 0, st, static_cast<const S*>(series), L, E, F,
                     ncolblk, null_val, null_nan, gap, static_cast<const int32_t*>(scratch), static_cast<S*>(filled),
                     reinterpret_cast<unsigned long long*>(counts));
  DS_CHECK_LAUNCH();
  return 0;
}

}  // namespace

int dstagnn_window_fill_forward(int series_f64, const void* series, int64_t L, int N, int F, double null_val,
                                int64_t max_gap, void* filled, int64_t* counts, void* scratch, size_t scratch_bytes,
                                dstagnn_stream_t stream) {
  if (!series || !filled || !counts || !scratch || filled == series) {
    set_last_error("window_fill_forward: null series / filled / counts / scratch, or filled == series");
    return DSTAGNN_E_ARG;
  }
  if (max_gap < 0) {
    set_last_error("window_fill_forward: max_gap must be >= 0 (0: unlimited), got " + std::to_string(max_gap));
    return DSTAGNN_E_ARG;
  }
  if (L < 1 || L >= (1ll << 31) || N < 1 || F < 1 || F > kStatMaxF) {
    set_last_error("window_fill_forward: L in [1, 2^31), N >= 1 and F in [1, 256], got F = " + std::to_string(F));
    return DSTAGNN_E_SHAPE;
  }
  const int64_t E = (int64_t)N * F, nchunk = (L + kFillChunk - 1) / kFillChunk;
  const int64_t ncolblk = (E + kFillCols - 1) / kFillCols, grid = nchunk * ncolblk;
  if (grid >= (1ll << 31)) {
    set_last_error("window_fill_forward: chunks * column blocks must be below 2^31");
    return DSTAGNN_E_SHAPE;
  }
  if (scratch_bytes < (size_t)dstagnn_window_fill_scratch_bytes(L, N, F)) {
    set_last_error("window_fill_forward: scratch smaller than dstagnn_window_fill_scratch_bytes(L, N, F)");
    return DSTAGNN_E_SPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, 2 * (size_t)F * sizeof(int64_t), st) != hipSuccess) {
    set_last_error("window_fill_forward: clearing counts failed");
    return DSTAGNN_E_ARG;
  }
  const int64_t gap = max_gap == 0 ? L : max_gap;  // no carry is longer than L - 1
  return series_f64 ? launch_fill<double>(series, L, E, F, (int)ncolblk, (unsigned)grid, null_val, gap, filled, counts,
                                          scratch, st)
                    : launch_fill<float>(series, L, E, F, (int)ncolblk, (unsigned)grid, null_val, gap, filled, counts,
                                         scratch, st);
}
