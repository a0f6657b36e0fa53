// Sanitizer driver (ASan + UBSan, host build) for the rectangular entry of the network-simplex
// EMD solver (dstagnn_drought_amd/csrc/emd_simplex.hpp via tests/native/emd_rect_host.cpp):
// random cosine-cost and dense-cost problems with Tr, Tc = 1..40 chosen independently, F = 1..4,
// strictly positive balanced marginals (what the masked prep hands the solver: every compacted
// row is an observed step); checks that every solve terminates with status 0 and a finite
// non-negative cost (the values are held to scipy linprog by tests/test_emd_rect_cpu.py).
// Test infrastructure only (tests/test_sanitize_rect_cpu.py builds and runs it); exit 0 = clean.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

extern "C" double emd_rect_host(const double* xh, const double* yh, const double* p, const double* q,
                                const double* D, int Tr, int Tc, int F, int* status, long long* pivots);

static double urand(unsigned long long* s) {
  *s = *s * 6364136223846793005ULL + 1442695040888963407ULL;
  return (double)(*s >> 11) / 9007199254740992.0;
}

static void unit_rows(double* x, int T, int F, unsigned long long* seed) {
  for (int t = 0; t < T; ++t) {
    double n = 0;
    for (int f = 0; f < F; ++f) { x[t * F + f] = urand(seed) - 0.5; n += x[t * F + f] * x[t * F + f]; }
    n = sqrt(n) > 0 ? sqrt(n) : 1.0;
    for (int f = 0; f < F; ++f) x[t * F + f] /= n;
  }
}

static void marginal(double* p, int T, unsigned long long* seed) {
  double s = 0;
  for (int t = 0; t < T; ++t) { p[t] = 1e-3 + urand(seed); s += p[t]; }
  for (int t = 0; t < T; ++t) p[t] /= s;
}

int main() {
  unsigned long long seed = 98765;
  int bad = 0, runs = 0;
  for (int rep = 0; rep < 160; ++rep) {
    int Tr = 1 + (int)(urand(&seed) * 40), Tc = 1 + (int)(urand(&seed) * 40);
    if (Tr > 40) Tr = 40;
    if (Tc > 40) Tc = 40;
    if (rep % 16 == 0) Tr = 1;
    if (rep % 16 == 1) Tc = 1;
    if (rep % 16 == 2) { Tr = 40; Tc = 1; }
    if (rep % 16 == 3) { Tr = 1; Tc = 40; }
    const int F = 1 + rep % 4;
    double* xh = (double*)malloc(sizeof(double) * Tr * F);
    double* yh = (double*)malloc(sizeof(double) * Tc * F);
    double* p = (double*)malloc(sizeof(double) * Tr);
    double* q = (double*)malloc(sizeof(double) * Tc);
    double* D = (double*)malloc(sizeof(double) * Tr * Tc);
    unit_rows(xh, Tr, F, &seed);
    unit_rows(yh, Tc, F, &seed);
    marginal(p, Tr, &seed);
    marginal(q, Tc, &seed);
    for (int i = 0; i < Tr; ++i)
      for (int j = 0; j < Tc; ++j) {
        double d = 0;
        for (int f = 0; f < F; ++f) d += xh[i * F + f] * yh[j * F + f];
        D[i * Tc + j] = 1.0 - d;
      }
    int st1 = -1, st2 = -1;
    long long pv1 = 0, pv2 = 0;
    const double r1 = emd_rect_host(xh, yh, p, q, NULL, Tr, Tc, F, &st1, &pv1);
    const double r2 = emd_rect_host(NULL, NULL, p, q, D, Tr, Tc, 0, &st2, &pv2);
    ++runs;
    if (st1 != 0 || st2 != 0 || !isfinite(r1) || !isfinite(r2) || r1 < -1e-12 || r2 < -1e-12) {
      fprintf(stderr, "Tr=%d Tc=%d F=%d rep=%d: status %d/%d cost %.17g / %.17g\n", Tr, Tc, F, rep, st1, st2, r1, r2);
      ++bad;
    }
    free(xh); free(yh); free(p); free(q); free(D);
  }
  printf("emd rect sanitize: %d problems, %d bad\n", runs, bad);
  return bad ? 1 : 0;
}
