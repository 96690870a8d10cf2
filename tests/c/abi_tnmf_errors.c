/* abi_tnmf_errors.c -- the argument-checking part of nagp_sebf_conv, nagp_sebf_fit_* and nagp_tnmf_* under AddressSanitizer
 * (libnagp_asan.so: the host code of the C ABI instrumented), on a machine without a GPU: every refusal of include/nagp.h returns its
 * status before any device call, and nothing is read beyond the exactly-sized heap blocks the arguments live in.  The over-budget
 * refusal is reached through the developer switch NAGP_SEBF_BUDGET_MB (read behind NAGP_DEVELOPER, which this program sets before its
 * first call into the library).  Built and run by tests/test_tnmf_host.py. */
#define _POSIX_C_SOURCE 200112L
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "nagp.h"

#define EXPECT(call, code)                                                                         \
  do { int _s = (call); if (_s != (code)) { fprintf(stderr, "%s -> %d (%s), expected %d\n", #call, _s, nagp_last_error(), (code)); ++bad; } } while (0)

enum { P = 2, T = 5, D = 3, K = 2 };

static double* filled(size_t n, double v) {
  double* p = (double*)malloc(n * sizeof *p); size_t i;
  for (i = 0; i < n; ++i) p[i] = v;
  return p;
}

int main(void) {
  int bad = 0, k;
  double *xl = filled(P * (T * K + K * D), 0.1), *xi = filled(P * T * K, 0.1), *A = filled(T * D, 1.5), *vary = filled(T * D, 0.2);
  double *W = filled(P * K * D, 0.3), *len = filled(K, 2.0), *mu = filled(K, 0.25), *vx = filled(K, 0.5);
  double *Obj = filled(P, 0.0), *dObj = filled(P * (T * K + K * D), 0.0), *Z = filled(K * T, 0.1), *Y = filled(K * T, 0.0), *wide, *wideA, ms[3];
  nagp_tnmf* h = (nagp_tnmf*)ms;                             /* must come back NULL from a refused create */
  nagp_sebf_fit* hf = (nagp_sebf_fit*)ms;
  const double bads[3] = {NAN, INFINITY, -INFINITY};
  double tol = 9.0;
  setenv("NAGP_DEVELOPER", "1", 1);                          /* the library reads it once, at its first call */
#define CALL(n, t, d, kk, xx, aa, vy, ww, l, m, v, ob, dob) nagp_tnmf_obj(n, t, d, kk, xx, aa, vy, ww, l, m, v, tol, ob, dob, 0)
#define LEARN() CALL(P, T, D, K, xl, A, vary, NULL, len, mu, vx, Obj, dObj)
#define INF() CALL(P, T, D, K, xi, A, vary, W, len, mu, vx, Obj, dObj)
#define CONV() nagp_sebf_conv(K, T, Z, len, vx, tol, Y, 0)
#define FIT() nagp_sebf_fit_obj(K, T, Z, Y, len, vx, tol, Obj, dObj, 0)
  /* NULL arguments */
  EXPECT(CALL(P, T, D, K, NULL, A, vary, NULL, len, mu, vx, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, T, D, K, xl, NULL, vary, NULL, len, mu, vx, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, T, D, K, xl, A, vary, NULL, NULL, mu, vx, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, T, D, K, xl, A, vary, NULL, len, NULL, vx, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, T, D, K, xl, A, vary, NULL, len, mu, NULL, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, T, D, K, xl, A, vary, NULL, len, mu, vx, NULL, dObj), NAGP_EINVAL);
  EXPECT(nagp_sebf_conv(K, T, NULL, len, vx, tol, Y, 0), NAGP_EINVAL);
  EXPECT(nagp_sebf_conv(K, T, Z, NULL, vx, tol, Y, 0), NAGP_EINVAL);
  EXPECT(nagp_sebf_conv(K, T, Z, len, NULL, tol, Y, 0), NAGP_EINVAL);
  EXPECT(nagp_sebf_conv(K, T, Z, len, vx, tol, NULL, 0), NAGP_EINVAL);
  EXPECT(nagp_sebf_fit_obj(K, T, NULL, Y, len, vx, tol, Obj, dObj, 0), NAGP_EINVAL);
  EXPECT(nagp_sebf_fit_obj(K, T, Z, NULL, len, vx, tol, Obj, dObj, 0), NAGP_EINVAL);
  EXPECT(nagp_sebf_fit_obj(K, T, Z, Y, NULL, vx, tol, Obj, dObj, 0), NAGP_EINVAL);
  EXPECT(nagp_sebf_fit_obj(K, T, Z, Y, len, NULL, tol, Obj, dObj, 0), NAGP_EINVAL);
  EXPECT(nagp_sebf_fit_obj(K, T, Z, Y, len, vx, tol, NULL, dObj, 0), NAGP_EINVAL);
  /* sizes */
  EXPECT(CALL(0, T, D, K, xl, A, vary, NULL, len, mu, vx, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(-1, T, D, K, xl, A, vary, NULL, len, mu, vx, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, 0, D, K, xl, A, vary, NULL, len, mu, vx, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, T, 0, K, xl, A, vary, NULL, len, mu, vx, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, T, D, 0, xl, A, vary, NULL, len, mu, vx, Obj, dObj), NAGP_EINVAL);
  EXPECT(nagp_sebf_conv(0, T, Z, len, vx, tol, Y, 0), NAGP_EINVAL);
  EXPECT(nagp_sebf_conv(K, 0, Z, len, vx, tol, Y, 0), NAGP_EINVAL);
  EXPECT(nagp_sebf_fit_obj(0, T, Z, Y, len, vx, tol, Obj, dObj, 0), NAGP_EINVAL);
  EXPECT(nagp_sebf_fit_obj(K, -1, Z, Y, len, vx, tol, Obj, dObj, 0), NAGP_EINVAL);
  /* the limits of D and K (refused on the sizes alone: nothing is read) */
  EXPECT(CALL(P, T, 65, K, xl, A, vary, NULL, len, mu, vx, Obj, dObj), NAGP_EUNSUPPORTED);
  EXPECT(CALL(P, T, D, 17, xl, A, vary, NULL, len, mu, vx, Obj, dObj), NAGP_EUNSUPPORTED);
  /* values: the last entry of each block */
  for (k = 0; k < 3; ++k) {
    A[T * D - 1] = bads[k];      EXPECT(LEARN(), NAGP_EINVAL); A[T * D - 1] = 1.5;
    vary[T * D - 1] = bads[k];   EXPECT(INF(), NAGP_EINVAL); vary[T * D - 1] = 0.2;
    W[P * K * D - 1] = bads[k];  EXPECT(INF(), NAGP_EINVAL); W[P * K * D - 1] = 0.3;
    len[K - 1] = bads[k];        EXPECT(LEARN(), NAGP_EINVAL); EXPECT(CONV(), NAGP_EINVAL); EXPECT(FIT(), NAGP_EINVAL); len[K - 1] = 2.0;
    vx[K - 1] = bads[k];         EXPECT(INF(), NAGP_EINVAL); EXPECT(CONV(), NAGP_EINVAL); EXPECT(FIT(), NAGP_EINVAL); vx[K - 1] = 0.5;
    mu[K - 1] = bads[k];         EXPECT(LEARN(), NAGP_EINVAL); EXPECT(INF(), NAGP_EINVAL); mu[K - 1] = 0.25;
    tol = bads[k];               EXPECT(LEARN(), NAGP_EINVAL); EXPECT(CONV(), NAGP_EINVAL); EXPECT(FIT(), NAGP_EINVAL); tol = 9.0;
  }
  A[T * D - 1] = -1e-9;        EXPECT(LEARN(), NAGP_EINVAL); A[T * D - 1] = 1.5;
  vary[T * D - 1] = -1e-9;     EXPECT(LEARN(), NAGP_EINVAL); vary[T * D - 1] = 0.2;
  W[P * K * D - 1] = -1e-9;    EXPECT(INF(), NAGP_EINVAL); W[P * K * D - 1] = 0.3;
  for (k = 0; k < D; ++k) W[K * D + (K - 1) + k * K] = 0.0;                          /* the last row of the second problem's W all zero */
  EXPECT(INF(), NAGP_EINVAL);
  for (k = 0; k < D; ++k) W[K * D + (K - 1) + k * K] = 0.3;
  len[K - 1] = 0.0;            EXPECT(LEARN(), NAGP_EINVAL); EXPECT(CONV(), NAGP_EINVAL); len[K - 1] = -1.0; EXPECT(FIT(), NAGP_EINVAL); len[K - 1] = 2.0;
  vx[K - 1] = -1e-9;           EXPECT(INF(), NAGP_EINVAL); EXPECT(CONV(), NAGP_EINVAL); EXPECT(FIT(), NAGP_EINVAL); vx[K - 1] = 0.5;
  tol = -1e-9;                 EXPECT(LEARN(), NAGP_EINVAL); EXPECT(CONV(), NAGP_EINVAL); EXPECT(FIT(), NAGP_EINVAL); tol = 9.0;
  /* a tau beyond the int32 count of the taps: 2^30 at lenx = 2^30 sqrt(2), tol = 1 (and far beyond) */
  len[0] = 1073741824.0 * sqrt(2.0); tol = 1.0;
  EXPECT(LEARN(), NAGP_EUNSUPPORTED); EXPECT(CONV(), NAGP_EUNSUPPORTED); EXPECT(FIT(), NAGP_EUNSUPPORTED);
  len[0] = 1e300; tol = 1e300; EXPECT(INF(), NAGP_EUNSUPPORTED);
  len[0] = 2.0; tol = 9.0;
  /* the resident forms: the same checks, and handles that stay NULL */
  EXPECT(nagp_tnmf_create(NULL, P, T, D, K, A, vary, NULL, len, mu, vx, tol, 0), NAGP_EINVAL);
  EXPECT(nagp_tnmf_create(&h, P, T, D, K, A, vary, NULL, len, NULL, vx, tol, 0), NAGP_EINVAL);
  if (h != NULL) { fprintf(stderr, "a refused create left a handle\n"); ++bad; }
  EXPECT(nagp_tnmf_create(&h, P, T, 65, K, A, vary, NULL, len, mu, vx, tol, 0), NAGP_EUNSUPPORTED);
  EXPECT(nagp_tnmf_eval(NULL, xl, Obj, dObj), NAGP_EINVAL);
  nagp_tnmf_destroy(NULL);
  EXPECT(nagp_sebf_fit_create(NULL, K, T, Y, len, vx, tol, 0), NAGP_EINVAL);
  EXPECT(nagp_sebf_fit_create(&hf, K, T, NULL, len, vx, tol, 0), NAGP_EINVAL);
  if (hf != NULL) { fprintf(stderr, "a refused create left a handle\n"); ++bad; }
  EXPECT(nagp_sebf_fit_eval(NULL, Z, Obj, dObj), NAGP_EINVAL);
  nagp_sebf_fit_destroy(NULL);
  /* one problem beyond the budget of the per-evaluation buffers, lowered to 1 MiB: at T = 70000, D = K = 1 the learning form takes
   * 8 (4 * 70001 + 274 * 2 + 1) B, the fit 8 (3 * 70000 + 1) B and a column of the primitive 16 * 70000 B */
  wide = filled(70001, 0.0); wideA = filled(70000, 1.0);
  setenv("NAGP_SEBF_BUDGET_MB", "1", 1);
  EXPECT(CALL(1, 70000, 1, 1, wide, wideA, NULL, NULL, len, mu, vx, Obj, NULL), NAGP_EUNSUPPORTED);
  EXPECT(nagp_sebf_fit_obj(1, 70000, wide, wideA, len, vx, tol, Obj, NULL, 0), NAGP_EUNSUPPORTED);
  EXPECT(nagp_sebf_conv(1, 70000, wide, len, vx, tol, wideA, 0), NAGP_EUNSUPPORTED);
  unsetenv("NAGP_SEBF_BUDGET_MB");
  free(wide); free(wideA);
  EXPECT(nagp_tnmf_timings(NULL), NAGP_EINVAL);
  EXPECT(nagp_tnmf_timings(ms), NAGP_OK);
  free(xl); free(xi); free(A); free(vary); free(W); free(len); free(mu); free(vx); free(Obj); free(dObj); free(Z); free(Y);
  if (bad) { fprintf(stderr, "%d unexpected statuses\n", bad); return 1; }
  printf("all error paths returned their status\n");
  return 0;
}
