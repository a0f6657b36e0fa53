// Host build of the rectangular entry of the network-simplex EMD solver
// (dstagnn_drought_amd/csrc/emd_simplex.hpp: Tr rows, Tc columns) for the CPU test suite only:
// the masked STAG graph gives every node a distribution on its own observed steps, so a pair's
// transportation problem is Tr x Tc.  The product path runs the same code in the gfx950 kernel
// (stag.hip, stag_emd_masked_kernel); nothing in the package loads this library.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "../../dstagnn_drought_amd/csrc/emd_simplex.hpp"

// D null: cosine costs from xh (Tr, F) / yh (Tc, F); else dense (Tr, Tc) costs (xh / yh unused).
extern "C" double emd_rect_host(const double* xh, const double* yh, const double* p, const double* q,
                                const double* D, int Tr, int Tc, int F, int* status, long long* pivots) {
  double sp = 0, sq = 0;
  for (int t = 0; t < Tr; ++t) sp += p[t];
  for (int t = 0; t < Tc; ++t) sq += q[t];
  if (pivots) *pivots = 0;
  if (!emd::balanced(sp, sq)) { *status = 1; return 1.0; }
  const long long bytes = emd::work_bytes_rect(Tr, Tc, F);
  char* buf = (char*)aligned_alloc(64, (size_t)((bytes + 63) / 64 * 64));
  emd::Work w;
  emd::carve_rect(w, buf, Tr, Tc, F);
  if (!D) {
    memcpy((void*)w.xh, xh, sizeof(double) * Tr * F);
    memcpy((void*)w.yh, yh, sizeof(double) * Tc * F);
  }
  memcpy((void*)w.p, p, sizeof(double) * Tr);
  memcpy((void*)w.q, q, sizeof(double) * Tc);
  double cmax = 1.0;
  if (D) {
    w.Dm = D;
    cmax = 0.0;
    for (long long i = 0; i < (long long)Tr * Tc; ++i) cmax = fmax(cmax, fabs(emd::clean_cost(D[i])));
  }
  int64_t piv = 0;
  double r = emd::solve<1>(w, 0, [](emd::Cand c) { return c; }, [] {}, cmax, status, &piv);
  if (pivots) *pivots = piv;
  free(buf);
  return r;
}
