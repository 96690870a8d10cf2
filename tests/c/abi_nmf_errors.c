/* abi_nmf_errors.c -- the argument-checking part of nagp_nmf_fp under AddressSanitizer (libnagp_asan.so: the host code of the C ABI
 * instrumented), on a machine without a GPU: every invalid call returns its status before any device call, and nothing is read
 * beyond the exactly-sized heap blocks the arguments live in.  Built and run by tests/test_nmf_host.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nagp.h"

#define EXPECT(call, code)                                                                         \
  do { int _s = (call); if (_s != (code)) { fprintf(stderr, "%s -> %d (%s), expected %d\n", #call, _s, nagp_last_error(), (code)); ++bad; } } while (0)

enum { P = 2, T = 7, D = 3, K = 2, ITS = 2 };

static double* filled(size_t n, double v) {
  double* p = (double*)malloc(n * sizeof *p); size_t i;
  for (i = 0; i < n; ++i) p[i] = v + 0.01 * (double)(i % 5);
  return p;
}

int main(void) {
  int bad = 0;
  double *A = filled(T * D, 1.0), *vary = filled(T * D, 1e-3), *W0 = filled(P * K * D, 0.2), *H0 = filled(P * T * K, 0.5);
  double *W = filled(P * K * D, 0.0), *H = filled(P * T * K, 0.0), *Obj = filled(P * 2 * ITS, 0.0);
#define CALL(np, t, d, k, a, v, w0, h0, its) nagp_nmf_fp(np, t, d, k, a, v, w0, h0, its, 1, W, H, Obj, 0)
  EXPECT(CALL(P, T, D, K, NULL, vary, W0, H0, ITS), NAGP_EINVAL);
  EXPECT(CALL(P, T, D, K, A, vary, NULL, H0, ITS), NAGP_EINVAL);
  EXPECT(CALL(P, T, D, K, A, vary, W0, NULL, ITS), NAGP_EINVAL);
  EXPECT(CALL(0, T, D, K, A, vary, W0, H0, ITS), NAGP_EINVAL);
  EXPECT(CALL(P, 0, D, K, A, vary, W0, H0, ITS), NAGP_EINVAL);
  EXPECT(CALL(P, T, 0, K, A, vary, W0, H0, ITS), NAGP_EINVAL);
  EXPECT(CALL(P, T, D, 0, A, vary, W0, H0, ITS), NAGP_EINVAL);
  EXPECT(CALL(P, T, D, K, A, vary, W0, H0, -1), NAGP_EINVAL);
  EXPECT(CALL(P, T, 65, K, A, vary, W0, H0, ITS), NAGP_EUNSUPPORTED);      /* refused on the sizes alone: nothing is read */
  EXPECT(CALL(P, T, D, 17, A, vary, W0, H0, ITS), NAGP_EUNSUPPORTED);
  A[T * D - 1] = -1e-9;   EXPECT(CALL(P, T, D, K, A, vary, W0, H0, ITS), NAGP_EINVAL); A[T * D - 1] = 1.0;          /* the last entry of each block */
  vary[T * D - 1] = -1.0; EXPECT(CALL(P, T, D, K, A, vary, W0, H0, ITS), NAGP_EINVAL); vary[T * D - 1] = 1e-3;
  H0[P * T * K - 1] = 0.0; EXPECT(CALL(P, T, D, K, A, NULL, W0, H0, ITS), NAGP_EINVAL); H0[P * T * K - 1] = 0.5;    /* H0 with a zero, in the last problem */
  W0[P * K * D - 1] = -0.1; EXPECT(CALL(P, T, D, K, A, vary, W0, H0, ITS), NAGP_EINVAL); W0[P * K * D - 1] = 0.2;
  { int d; double keep[D];                                                                                         /* a zero row of W0 of the last problem */
    for (d = 0; d < D; ++d) { keep[d] = W0[(P - 1) * K * D + 1 + d * K]; W0[(P - 1) * K * D + 1 + d * K] = 0.0; }
    EXPECT(CALL(P, T, D, K, A, vary, W0, H0, ITS), NAGP_EINVAL);
    for (d = 0; d < D; ++d) W0[(P - 1) * K * D + 1 + d * K] = keep[d]; }
  { int k; double keep[K];                                                                                         /* a zero column */
    for (k = 0; k < K; ++k) { keep[k] = W0[k + (D - 1) * K]; W0[k + (D - 1) * K] = 0.0; }
    EXPECT(CALL(P, T, D, K, A, vary, W0, H0, ITS), NAGP_EINVAL);
    for (k = 0; k < K; ++k) W0[k + (D - 1) * K] = keep[k]; }
  /* n_its = 0 copies the inputs through, on the host */
  EXPECT(CALL(P, T, D, K, A, vary, W0, H0, 0), NAGP_OK);
  if (memcmp(W, W0, P * K * D * sizeof *W) || memcmp(H, H0, P * T * K * sizeof *H)) { fprintf(stderr, "n_its = 0 did not copy the inputs\n"); ++bad; }
  EXPECT(nagp_nmf_fp(P, T, D, K, A, vary, W0, H0, 0, 1, NULL, NULL, NULL, 0), NAGP_OK);
  EXPECT(nagp_nmf_timings(NULL), NAGP_EINVAL);
  { double ms = -1.0;                                                                                              /* a refused call reports no time */
    EXPECT(CALL(P, T, 65, K, A, vary, W0, H0, ITS), NAGP_EUNSUPPORTED);
    EXPECT(nagp_nmf_timings(&ms), NAGP_OK);
    if (ms != 0.0) { fprintf(stderr, "nagp_nmf_timings after a refused call: %g, expected 0\n", ms); ++bad; } }
  free(A); free(vary); free(W0); free(H0); free(W); free(H); free(Obj);
  if (bad) { fprintf(stderr, "%d unexpected statuses\n", bad); return 1; }
  printf("all error paths returned their status\n");
  return 0;
}
