// gtu_dw.hip — the three GTU convolution weight (and bias) gradients as ONE sliding-window
// kernel plus a fold, in place of the grouped split-K GEMM and its fold:
//   dW_q[o][c][j] = sum_{(bn, t')} dconv_q[(bn, t')][o] X[bn][t' + j][c],  db_q[o] = sum dconv_q[.][o]
// for kernel widths kw = 3 / 5 / 7 (Tg = T - kw + 1 output positions), C = 32, T = 12 — the
// geometry of the fused GTU backward, whose compact (BN Tg, 2C) gate-gradient rows are the
// first operand as they stand.
//
// The generic GEMM sees M = 2C = 64 (one row of tiles), so all its parallelism is split-K: ~1240
// workgroups of ~8 k-tiles, each with a 64 x 64 slab to store and fold, and an implicit-im2col
// B operand that stages every X row kw times.  Here a workgroup of 8 waves owns one GTU and one
// contiguous chunk of nodes (in units of 4 nodes), about one workgroup per CU in all, the chunk
// counts per GTU proportional to its MACs (kw Tg = 30 : 40 : 42):
//   * it walks its chunk in stages of kDS nodes: the nodes' X rows and dconv rows go to LDS once
//     (node strides padded to 16 mod 64 floats), double-buffered through registers — the next
//     stage's global loads are in flight during this stage's matrix-core work;
//   * the contraction index is reordered (t', node): MFMA k = lq is node 4 g + lq of a 4-node
//     group, so a lane's operands for every t' and tap j sit at compile-time offsets from one
//     base, and the window is a row offset: the lane reads its 12 X values and Tg dconv values of
//     a group once and issues kw Tg MFMAs on them;
//   * wave w owns output rows o = 16 (w & 3) .. + 15 and channel half h = w >> 2 for all kw taps:
//     the whole 64 x 32 kw dW_q stays in kw accumulator tiles per wave for the whole chunk;
//   * the bias sums are VALU adds of the same dconv fragments (the waves of h = 0);
//   * no store before the epilogue: one partial [o][j][c] + 2C bias sums per workgroup.
// gtu_dw_fold_kernel then sums the chunks in a fixed order (four slices of chunks per element,
// then the slices in order) and writes the parameters' own [o][c][j] layout: the same bits
// every run.
#include <algorithm>
#include <mutex>

#include "common.hpp"
#include "ops.hpp"

namespace {

constexpr int kDC = 32, kDT = 12, kDO = 2 * kDC;  // C, T, 2C
constexpr int kDW = 8, kDNT = kDW * 64;           // waves, threads per workgroup
#ifndef DSTAGNN_GTU_DW_STAGE
#define DSTAGNN_GTU_DW_STAGE 4
#endif
constexpr int kDS = DSTAGNN_GTU_DW_STAGE;         // nodes per stage
static_assert(kDS % 4 == 0 && kDS >= 4, "a stage is whole 4-node groups");
constexpr int kDXN = kDT * kDC + 16;              // LDS node stride of the X rows (16 mod 64)
constexpr int dw_dn(int Tg) { return Tg * kDO + 16; }  // ... of a node's dconv rows (16 mod 64)
constexpr int kDBuf = kDS * (kDXN + dw_dn(kDT - 2));   // one stage buffer (sized for kw = 3), floats
constexpr int kDFoldE = 64, kDFoldS = 4;          // fold: elements and chunk slices per workgroup
constexpr int kDMaxChunks = 4096;

constexpr int dw_ks(int q) { return 3 + 2 * q; }
constexpr int dw_row(int q) { return kDO * dw_ks(q) * kDC + kDO; }  // a partial: [o][j][c] + bias sums

struct GtuDwK {
  const float* dconv[3];
  const float* X;
  float* part[3];  // [chunks[q]][dw_row(q)]
  float* dw[3];
  float* db[3];
  int64_t BN;
  int chunks[3];
};

template <int KS>
__device__ __forceinline__ void dw_chunk(const GtuDwK& a, int q, int chunk, float* lds) {
  constexpr int Tg = kDT - KS + 1, DN = dw_dn(Tg), KK = KS * kDC;
  constexpr int XN4 = kDT * kDC / 4, DN4 = Tg * kDO / 4;  // float4s per node
  constexpr int XV = (kDS * XN4 + kDNT - 1) / kDNT, DV = (kDS * DN4 + kDNT - 1) / kDNT;
  const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), l = tid & 63, i = l & 15, lq = l >> 4;
  const int ot = w & 3, h = w >> 2;
  // the chunk's nodes: whole 4-node groups, the last group of all clipped to BN
  const int64_t NG = (a.BN + 3) / 4, nc = a.chunks[q];
  const int64_t n0 = 4 * (NG * chunk / nc), n1 = min(4 * (NG * (chunk + 1) / nc), a.BN);
  const int nstage = n1 > n0 ? (int)((n1 - n0 + kDS - 1) / kDS) : 0;

  float4 xv[XV], dv[DV];
  // stage s into registers (nodes past the chunk's end: zeros in both operands)
  auto load = [&](int s) {
    const int64_t nb = n0 + (int64_t)s * kDS;
    const int nv = (int)min<int64_t>(kDS, n1 - nb);
    const float4* gx = reinterpret_cast<const float4*>(a.X + nb * (kDT * kDC));
    const float4* gd = reinterpret_cast<const float4*>(a.dconv[q] + nb * (Tg * kDO));
#pragma unroll
    for (int u = 0; u < XV; ++u) {
      const int e4 = u * kDNT + tid;
      xv[u] = e4 < nv * XN4 ? gx[e4] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < DV; ++u) {
      const int e4 = u * kDNT + tid;
      dv[u] = e4 < nv * DN4 ? gd[e4] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto store = [&](float* buf) {
    float* Xs = buf;
    float* Ds = buf + kDS * kDXN;
#pragma unroll
    for (int u = 0; u < XV; ++u) {
      const int e4 = u * kDNT + tid, n = e4 / XN4;
      if (e4 < kDS * XN4) *reinterpret_cast<float4*>(Xs + n * kDXN + 4 * (e4 - n * XN4)) = xv[u];
    }
#pragma unroll
    for (int u = 0; u < DV; ++u) {
      const int e4 = u * kDNT + tid, n = e4 / DN4;
      if (e4 < kDS * DN4) *reinterpret_cast<float4*>(Ds + n * DN + 4 * (e4 - n * DN4)) = dv[u];
    }
  };

  floatx4 acc[KS];
#pragma unroll
  for (int j = 0; j < KS; ++j) acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};
  float bs = 0.f;

  if (nstage > 0) {
    load(0);
    store(lds);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
  for (int s = 0; s < nstage; ++s) {
    const float* buf = lds + (s & 1) * kDBuf;
    if (s + 1 < nstage) load(s + 1);
    const int ngrp = ((int)min<int64_t>(kDS, n1 - n0 - (int64_t)s * kDS) + 3) / 4;
#pragma unroll
    for (int g = 0; g < kDS / 4; ++g) {
      if (g >= ngrp) break;  // (workgroup-uniform)
      // A[m = o][k = node] = dconv[node][t'][16 ot + i], B[k = node][n = c] = X[node][t' + j][16 h + i]
      const float* xb = buf + (4 * g + lq) * kDXN + 16 * h + i;
      const float* db = buf + kDS * kDXN + (4 * g + lq) * DN + 16 * ot + i;
      float xr[kDT], ar[Tg];
#pragma unroll
      for (int t = 0; t < Tg; ++t) ar[t] = db[t * kDO];
#pragma unroll
      for (int u = 0; u < kDT; ++u) xr[u] = xb[u * kDC];
#pragma unroll
      for (int t = 0; t < Tg; ++t) {
        bs += ar[t];
#pragma unroll
        for (int j = 0; j < KS; ++j) acc[j] = mfma16(ar[t], xr[t + j], acc[j]);
      }
    }
    if (s + 1 < nstage) store(lds + ((s + 1) & 1) * kDBuf);
    // (the other buffer's readers passed the previous barrier; no vmcnt drain wanted here)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }

  // the partial, once: D[4 lq + r][i] of tap j is dW[o = 16 ot + 4 lq + r][j][c = 16 h + i]
  float* part = a.part[q] + (int64_t)chunk * dw_row(q);
#pragma unroll
  for (int j = 0; j < KS; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) part[(16 * ot + 4 * lq + r) * KK + j * kDC + 16 * h + i] = acc[j][r];
  bs += __shfl_xor(bs, 16, 64);
  bs += __shfl_xor(bs, 32, 64);
  if (h == 0 && lq == 0) part[kDO * KK + 16 * ot + i] = bs;
}

__global__ __launch_bounds__(kDNT, 1) void gtu_dw_kernel(GtuDwK a) {
  extern __shared__ float4 lds4[];
  float* lds = reinterpret_cast<float*>(lds4);
  const int b = blockIdx.x;
  if (b < a.chunks[0]) dw_chunk<3>(a, 0, b, lds);
  else if (b < a.chunks[0] + a.chunks[1]) dw_chunk<5>(a, 1, b - a.chunks[0], lds);
  else dw_chunk<7>(a, 2, b - a.chunks[0] - a.chunks[1], lds);
}

// a workgroup: kDFoldE consecutive entries of one GTU's partial row x kDFoldS slices of its chunks
__global__ __launch_bounds__(kDFoldE* kDFoldS) void gtu_dw_fold_kernel(GtuDwK a) {
  __shared__ float sh[kDFoldS][kDFoldE];
  constexpr int B0 = dw_row(0) / kDFoldE, B1 = dw_row(1) / kDFoldE;
  int b = blockIdx.x;
  const int q = b < B0 ? 0 : (b < B0 + B1 ? 1 : 2);
  b -= q == 0 ? 0 : (q == 1 ? B0 : B0 + B1);
  const int KS = 3 + 2 * q, KK = KS * kDC, row = kDO * KK + kDO;
  const int x = threadIdx.x & (kDFoldE - 1), sl = threadIdx.x / kDFoldE;
  const int e = b * kDFoldE + x, nc = a.chunks[q];
  const int c0 = nc * sl / kDFoldS, c1 = nc * (sl + 1) / kDFoldS;
  const float* p = a.part[q] + e;
  float s = 0.f;
#pragma unroll 4
  for (int c = c0; c < c1; ++c) s += p[(int64_t)c * row];
  sh[sl][x] = s;
  __syncthreads();
  if (sl != 0) return;
#pragma unroll
  for (int k = 1; k < kDFoldS; ++k) s += sh[k][x];
  if (e < kDO * KK) {
    const int o = e / KK, jc = e - o * KK, j = jc / kDC, c = jc - j * kDC;
    a.dw[q][(o * kDC + c) * KS + j] = s;
  } else {
    a.db[q][e - kDO * KK] = s;
  }
}
static_assert(dw_row(0) % kDFoldE == 0 && dw_row(1) % kDFoldE == 0 && dw_row(2) % kDFoldE == 0, "fold tiling");

bool dw_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int dw_cus() {
  static const int n = [] {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      cus = 256;
    return cus;
  }();
  return n;
}

}  // namespace

bool gtu_dw_ok(int C, int T) { return C == kDC && T == kDT; }
int gtu_dw_stage_nodes() { return kDS; }

// about one workgroup per CU in all, per GTU in proportion to its MACs (kw Tg = 30 : 40 : 42);
// never more chunks than 4-node groups
void gtu_dw_plan(int64_t BN, int chunks[3]) {
  const int64_t NG = std::max<int64_t>(1, (BN + 3) / 4);
  const int cus = dw_cus();
  for (int q = 0; q < 3; ++q) {
    const int ks = dw_ks(q), mac = ks * (kDT - ks + 1);
    chunks[q] = (int)std::min<int64_t>(NG, std::max(1, (cus * mac + 56) / 112));
  }
}

int op_gtu_dw(const GtuDwArgs& a, float* ws, size_t ws_floats, hipStream_t st) {
  if (!gtu_dw_ok(a.C, a.T) || a.BN <= 0 || !ws) {
    set_last_error("gtu_dw: C = 32, T = 12 and a workspace only");
    return DSTAGNN_E_SHAPE;
  }
  bool al = dw_al16(a.X) && dw_al16(ws);
  for (int q = 0; q < 3; ++q) al = al && a.dconv[q] && a.dw[q] && a.db[q] && dw_al16(a.dconv[q]);
  if (!al || !a.X) {
    set_last_error("gtu_dw: operands must be set and 16-B aligned");
    return DSTAGNN_E_ARG;
  }
  GtuDwK k;
  k.X = a.X; k.BN = a.BN;
  if (a.chunks > 0) k.chunks[0] = k.chunks[1] = k.chunks[2] = a.chunks;
  else gtu_dw_plan(a.BN, k.chunks);
  size_t need = 0;
  for (int q = 0; q < 3; ++q) {
    if (k.chunks[q] > kDMaxChunks) {
      set_last_error("gtu_dw: too many chunks");
      return DSTAGNN_E_ARG;
    }
    k.dconv[q] = a.dconv[q]; k.dw[q] = a.dw[q]; k.db[q] = a.db[q];
    k.part[q] = ws + need;
    need += (size_t)k.chunks[q] * dw_row(q);
  }
  if (need > ws_floats) {
    set_last_error("gtu_dw: workspace too small for the partials");
    return DSTAGNN_E_ARG;
  }
  const size_t lds = sizeof(float) * 2 * (size_t)kDBuf;
  {
    static std::mutex mu;
    static bool done = false;
    std::lock_guard<std::mutex> lock(mu);
    if (!done) {
      const hipError_t e =
          hipFuncSetAttribute((const void*)gtu_dw_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) { set_last_error(std::string("gtu_dw: ") + hipGetErrorString(e)); return (int)e; }
      done = true;
    }
  }
  // the three products' algorithmic FLOP (bias column included, as the GEMM counted it) and bytes
  double flops = 0.0, bytes = 4.0 * a.BN * kDT * kDC;
  for (int q = 0; q < 3; ++q) {
    const int ks = dw_ks(q), Tg = kDT - ks + 1;
    flops += 2.0 * kDO * (kDC * ks + 1) * (double)a.BN * Tg;
    bytes += 4.0 * ((double)a.BN * Tg * kDO + kDO * (kDC * ks + 1));
  }
  void* rec = gemm_prof_begin(flops, bytes, st, DSTAGNN_PROF_GTU_DW);
  hipLaunchKernelGGL(gtu_dw_kernel, dim3((unsigned)(k.chunks[0] + k.chunks[1] + k.chunks[2])), dim3(kDNT), lds, st, k);
  DS_CHECK_LAUNCH();
  hipLaunchKernelGGL(gtu_dw_fold_kernel, dim3((unsigned)((dw_row(0) + dw_row(1) + dw_row(2)) / kDFoldE)),
                     dim3(kDFoldE * kDFoldS), 0, st, k);
  DS_CHECK_LAUNCH();
  gemm_prof_end(rec, st);
  return 0;
}

int dstagnn_gtu_dw(const float* const dconv[3], const float* X, int64_t BN, float* const dw[3], float* const db[3],
                   int chunks, void* scratch, size_t scratch_bytes, dstagnn_stream_t stream) {
  if (!dconv || !dw || !db || !scratch || scratch_bytes <= 256 || chunks < 0) return DSTAGNN_E_ARG;
  GtuDwArgs a;
  for (int q = 0; q < 3; ++q) { a.dconv[q] = dconv[q]; a.dw[q] = dw[q]; a.db[q] = db[q]; }
  a.X = X; a.BN = BN; a.C = kDC; a.T = kDT; a.chunks = chunks;
  float* ws = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(scratch) + 255) & ~uintptr_t(255));
  return op_gtu_dw(a, ws, (scratch_bytes - 256) / sizeof(float), (hipStream_t)stream);
}

int dstagnn_gtu_dw_plan(int64_t BN, int chunks[3], int* stage_nodes) {
  if (BN <= 0 || !chunks || !stage_nodes) return DSTAGNN_E_ARG;
  gtu_dw_plan(BN, chunks);
  *stage_nodes = gtu_dw_stage_nodes();
  return 0;
}
