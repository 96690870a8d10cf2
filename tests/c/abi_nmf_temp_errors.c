/* abi_nmf_temp_errors.c -- the argument-checking part of nagp_nmf_temp_obj / nagp_nmf_temp_create / nagp_nmf_temp_eval under
 * AddressSanitizer (libnagp_asan.so: the host code of the C ABI instrumented), on a machine without a GPU: every refusal of
 * include/nagp.h returns its status before any device call, and nothing is read beyond the exactly-sized heap blocks the arguments live
 * in.  The over-budget refusal is reached through the developer switch NAGP_NMFT_BUDGET_MB (read behind NAGP_DEVELOPER, which this
 * program sets before its first call into the library).  Built and run by tests/test_nmf_temp_host.py. */
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
  double *W = filled(P * K * D, 0.3), *mu = filled(K, 0.25), *vi = filled(K, 0.0625), *la = filled(K, 0.1);
  double *Obj = filled(P, 0.0), *dObj = filled(P * (T * K + K * D), 0.0), *wide, *wideA, ms;
  nagp_nmf_temp* h = (nagp_nmf_temp*)&ms;                    /* must come back NULL from a refused create */
  const double bads[3] = {NAN, INFINITY, -INFINITY};
  setenv("NAGP_DEVELOPER", "1", 1);                          /* the library reads it once, at its first call */
#define CALL(n, t, d, kk, pr, xx, aa, vy, ww, m, v, l, ob, dob) nagp_nmf_temp_obj(n, t, d, kk, pr, xx, aa, vy, ww, m, v, l, ob, dob, 0)
#define LEARN(pr) CALL(P, T, D, K, pr, xl, A, vary, NULL, mu, vi, la, Obj, dObj)
#define INF(pr) CALL(P, T, D, K, pr, xi, A, vary, W, mu, vi, la, Obj, dObj)
  /* NULL arguments */
  EXPECT(CALL(P, T, D, K, NAGP_NMFT_IG, NULL, A, vary, NULL, mu, vi, la, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, T, D, K, NAGP_NMFT_IG, xl, NULL, vary, NULL, mu, vi, la, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, T, D, K, NAGP_NMFT_IG, xl, A, vary, NULL, mu, vi, la, NULL, dObj), NAGP_EINVAL);
  /* sizes */
  EXPECT(CALL(0, T, D, K, NAGP_NMFT_NONE, xl, A, vary, NULL, NULL, NULL, NULL, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(-1, T, D, K, NAGP_NMFT_NONE, xl, A, vary, NULL, NULL, NULL, NULL, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, T, 0, K, NAGP_NMFT_NONE, xl, A, vary, NULL, NULL, NULL, NULL, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, T, D, 0, NAGP_NMFT_NONE, xl, A, vary, NULL, NULL, NULL, NULL, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, 0, D, K, NAGP_NMFT_NONE, xl, A, vary, NULL, NULL, NULL, NULL, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, 1, D, K, NAGP_NMFT_TG, xl, A, vary, NULL, NULL, vi, la, Obj, dObj), NAGP_EINVAL);      /* T < 2 with a prior */
  EXPECT(CALL(P, 1, D, K, NAGP_NMFT_IG, xi, A, vary, W, mu, vi, la, Obj, dObj), NAGP_EINVAL);
  /* an unknown prior */
  EXPECT(LEARN(3), NAGP_EINVAL);
  EXPECT(INF(-1), NAGP_EINVAL);
  /* a prior parameter array NULL where it is read (and not missed where it is not) */
  EXPECT(CALL(P, T, D, K, NAGP_NMFT_TG, xl, A, vary, NULL, NULL, NULL, la, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, T, D, K, NAGP_NMFT_TG, xl, A, vary, NULL, NULL, vi, NULL, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, T, D, K, NAGP_NMFT_IG, xl, A, vary, NULL, NULL, vi, la, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, T, D, K, NAGP_NMFT_IG, xl, A, vary, NULL, mu, NULL, la, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, T, D, K, NAGP_NMFT_IG, xl, A, vary, NULL, mu, vi, NULL, Obj, dObj), NAGP_EINVAL);
  /* the limits of D and K (refused on the sizes alone: nothing is read) */
  EXPECT(CALL(P, T, 65, K, NAGP_NMFT_NONE, xl, A, vary, NULL, NULL, NULL, NULL, Obj, dObj), NAGP_EUNSUPPORTED);
  EXPECT(CALL(P, T, D, 17, NAGP_NMFT_NONE, xl, A, vary, NULL, NULL, NULL, NULL, Obj, dObj), NAGP_EUNSUPPORTED);
  /* values: the last entry of each block */
  for (k = 0; k < 3; ++k) {
    A[T * D - 1] = bads[k];      EXPECT(LEARN(NAGP_NMFT_NONE), NAGP_EINVAL); A[T * D - 1] = 1.5;
    vary[T * D - 1] = bads[k];   EXPECT(INF(NAGP_NMFT_NONE), NAGP_EINVAL); vary[T * D - 1] = 0.2;
    W[P * K * D - 1] = bads[k];  EXPECT(INF(NAGP_NMFT_TG), NAGP_EINVAL); W[P * K * D - 1] = 0.3;
    vi[K - 1] = bads[k];         EXPECT(LEARN(NAGP_NMFT_TG), NAGP_EINVAL); EXPECT(INF(NAGP_NMFT_IG), NAGP_EINVAL); vi[K - 1] = 0.0625;
    la[K - 1] = bads[k];         EXPECT(LEARN(NAGP_NMFT_TG), NAGP_EINVAL); EXPECT(INF(NAGP_NMFT_IG), NAGP_EINVAL); la[K - 1] = 0.1;
    mu[K - 1] = bads[k];         EXPECT(LEARN(NAGP_NMFT_IG), NAGP_EINVAL); mu[K - 1] = 0.25;
  }
  A[T * D - 1] = -1e-9;        EXPECT(LEARN(NAGP_NMFT_NONE), NAGP_EINVAL); A[T * D - 1] = 1.5;
  vary[T * D - 1] = -1e-9;     EXPECT(LEARN(NAGP_NMFT_NONE), NAGP_EINVAL); vary[T * D - 1] = 0.2;
  W[P * K * D - 1] = -1e-9;    EXPECT(INF(NAGP_NMFT_NONE), NAGP_EINVAL); W[P * K * D - 1] = 0.3;
  for (k = 0; k < D; ++k) W[K * D + (K - 1) + k * K] = 0.0;                          /* the last row of the second problem's W all zero */
  EXPECT(INF(NAGP_NMFT_NONE), NAGP_EINVAL);
  for (k = 0; k < D; ++k) W[K * D + (K - 1) + k * K] = 0.3;
  vi[K - 1] = 0.0;             EXPECT(LEARN(NAGP_NMFT_TG), NAGP_EINVAL); vi[K - 1] = -1.0; EXPECT(INF(NAGP_NMFT_IG), NAGP_EINVAL); vi[K - 1] = 0.0625;
  mu[K - 1] = 0.0;             EXPECT(LEARN(NAGP_NMFT_IG), NAGP_EINVAL); mu[K - 1] = -0.25; EXPECT(INF(NAGP_NMFT_IG), NAGP_EINVAL); mu[K - 1] = 0.25;
  la[K - 1] = -1e-9;           EXPECT(LEARN(NAGP_NMFT_IG), NAGP_EINVAL); la[K - 1] = 1.0 + 1e-9; EXPECT(INF(NAGP_NMFT_IG), NAGP_EINVAL); la[K - 1] = 0.1;
  /* the resident form: the same checks, and a handle that stays NULL */
  EXPECT(nagp_nmf_temp_create(NULL, P, T, D, K, NAGP_NMFT_NONE, A, vary, NULL, NULL, NULL, NULL, 0), NAGP_EINVAL);
  EXPECT(nagp_nmf_temp_create(&h, P, T, D, K, NAGP_NMFT_TG, A, vary, NULL, NULL, NULL, la, 0), NAGP_EINVAL);
  if (h != NULL) { fprintf(stderr, "a refused create left a handle\n"); ++bad; }
  EXPECT(nagp_nmf_temp_create(&h, P, T, 65, K, NAGP_NMFT_NONE, A, vary, NULL, NULL, NULL, NULL, 0), NAGP_EUNSUPPORTED);
  EXPECT(nagp_nmf_temp_eval(NULL, xl, Obj, dObj), NAGP_EINVAL);
  nagp_nmf_temp_destroy(NULL);
  /* one problem beyond the budget of the per-evaluation buffers, lowered to 1 MiB: 8 (2 * 70001 + 274 * 2 + 1) B at T = 70000, D = K = 1 */
  wide = filled(70001, 0.0); wideA = filled(70000, 1.0);
  setenv("NAGP_NMFT_BUDGET_MB", "1", 1);
  EXPECT(CALL(1, 70000, 1, 1, NAGP_NMFT_NONE, wide, wideA, NULL, NULL, NULL, NULL, NULL, Obj, NULL), NAGP_EUNSUPPORTED);
  unsetenv("NAGP_NMFT_BUDGET_MB");
  free(wide); free(wideA);
  EXPECT(nagp_nmf_temp_timings(NULL), NAGP_EINVAL);
  EXPECT(nagp_nmf_temp_timings(&ms), NAGP_OK);
  free(xl); free(xi); free(A); free(vary); free(W); free(mu); free(vi); free(la); free(Obj); free(dObj);
  if (bad) { fprintf(stderr, "%d unexpected statuses\n", bad); return 1; }
  printf("all error paths returned their status\n");
  return 0;
}
