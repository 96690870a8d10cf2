/* abi_pstft_errors.c -- the argument-checking part of nagp_pstft_obj under AddressSanitizer (libnagp_asan.so: the host code of the C
 * ABI instrumented), on a machine without a GPU: every refusal of include/nagp.h returns its status before any device call, and
 * nothing is read beyond the exactly-sized heap blocks the arguments live in.  Built and run by tests/test_pstft_host.py. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "nagp.h"

#define EXPECT(call, code)                                                                         \
  do { int _s = (call); if (_s != (code)) { fprintf(stderr, "%s -> %d (%s), expected %d\n", #call, _s, nagp_last_error(), (code)); ++bad; } } while (0)

enum { P = 2, D = 3, N = 7 };

static double* filled(size_t n, double v) {
  double* p = (double*)malloc(n * sizeof *p); size_t i;
  for (i = 0; i < n; ++i) p[i] = v;
  return p;
}

int main(void) {
  int bad = 0, d;
  double *theta = filled(P * 3 * D, -0.5), *spec = filled(P * N, 1.5), *vary = filled(P, 1e-4), *bet = filled(P, 3.0), *minVar = filled(D, 1e-3);
  double *limOm = filled(2 * D, 0.0), *limLam = filled(2 * D, 0.0), *Obj = filled(P, 0.0), *dObj = filled(P * 3 * D, 0.0), *big = filled(P * 3 * 65, -0.5);
  double ms;
  for (d = 0; d < D; ++d) { limOm[D + d] = 3.14159; limLam[D + d] = 0.4; }
#define CALL(np, k, f, dd, n, th, sp, st, vy, bt, mv, lo, ll, ob, dob) nagp_pstft_obj(np, k, f, dd, n, th, sp, st, vy, bt, mv, lo, ll, ob, dob, 0)
#define STD(k, f, dd, n, st) CALL(P, k, f, dd, n, theta, spec, st, vary, bet, minVar, limOm, limLam, Obj, dObj)
  EXPECT(CALL(P, 0, 0, D, N, NULL, spec, N, vary, bet, minVar, limOm, limLam, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, 0, 0, D, N, theta, NULL, N, vary, bet, minVar, limOm, limLam, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, 0, 0, D, N, theta, spec, N, NULL, bet, minVar, limOm, limLam, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, 0, 0, D, N, theta, spec, N, vary, NULL, minVar, limOm, limLam, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, 0, 0, D, N, theta, spec, N, vary, bet, NULL, limOm, limLam, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, 0, 0, D, N, theta, spec, N, vary, bet, minVar, NULL, limLam, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, 0, 0, D, N, theta, spec, N, vary, bet, minVar, limOm, NULL, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, 0, 0, D, N, theta, spec, N, vary, bet, minVar, limOm, limLam, NULL, dObj), NAGP_EINVAL);
  EXPECT(CALL(0, 0, 0, D, N, theta, spec, N, vary, bet, minVar, limOm, limLam, Obj, dObj), NAGP_EINVAL);
  EXPECT(STD(0, 0, 0, N, N), NAGP_EINVAL);
  EXPECT(STD(0, 2, D, N, N), NAGP_EINVAL);                               /* form */
  EXPECT(STD(0, 0, D, 3, 3), NAGP_EINVAL);                               /* N < 4 */
  EXPECT(STD(0, 0, D, N, 5), NAGP_EINVAL);                               /* spec_stride neither 0 nor N */
  /* refused on the sizes alone: nothing is read */
  EXPECT(CALL(P, 0, 0, 65, N, big, spec, N, vary, bet, minVar, limOm, limLam, Obj, dObj), NAGP_EUNSUPPORTED);
  EXPECT(STD(NAGP_PSTFT_MATERN72, 0, D, N, N), NAGP_EUNSUPPORTED);       /* matern72 has no closed-form file */
  EXPECT(STD(4, 1, D, N, N), NAGP_EUNSUPPORTED);                         /* se and anything else */
  EXPECT(STD(-1, 1, D, N, N), NAGP_EUNSUPPORTED);
  /* the last entry of each block */
  theta[P * 3 * D - 1] = NAN;     EXPECT(STD(0, 0, D, N, N), NAGP_EINVAL); theta[P * 3 * D - 1] = -0.5;
  spec[P * N - 1] = -1e-9;        EXPECT(STD(1, 0, D, N, N), NAGP_EINVAL); spec[P * N - 1] = INFINITY; EXPECT(STD(1, 1, D, N, N), NAGP_EINVAL); spec[P * N - 1] = 1.5;
  spec[N - 1] = -1.0;             EXPECT(STD(2, 0, D, N, 0), NAGP_EINVAL); spec[N - 1] = 1.5;          /* shared: N entries are read */
  vary[P - 1] = -1e-12;           EXPECT(STD(0, 0, D, N, N), NAGP_EINVAL); vary[P - 1] = NAN; EXPECT(STD(0, 0, D, N, N), NAGP_EINVAL); vary[P - 1] = 1e-4;
  bet[P - 1] = INFINITY;          EXPECT(STD(0, 0, D, N, N), NAGP_EINVAL); bet[P - 1] = 3.0;
  minVar[D - 1] = -1.0;           EXPECT(STD(0, 0, D, N, N), NAGP_EINVAL); minVar[D - 1] = 1e-3;
  limOm[2 * D - 1] = 0.0;         EXPECT(STD(0, 0, D, N, N), NAGP_EINVAL); limOm[2 * D - 1] = 3.14159;  /* upper = lower */
  limLam[2 * D - 1] = -0.1;       EXPECT(STD(3, 1, D, N, N), NAGP_EINVAL);                              /* upper < lower */
  limLam[2 * D - 1] = 1.5;        EXPECT(STD(3, 1, D, N, N), NAGP_EINVAL); limLam[2 * D - 1] = 0.4;     /* beyond 1 */
  limLam[D - 1] = NAN;            EXPECT(STD(0, 0, D, N, N), NAGP_EINVAL); limLam[D - 1] = 0.0;
  /* vary = 0 in the last problem with every lam of that problem saturated onto the lower limit 0: spec would be 0 */
  vary[P - 1] = 0.0;
  for (d = 0; d < D; ++d) theta[(P - 1) * 3 * D + 2 * D + d] = -800.0;
  EXPECT(STD(0, 0, D, N, N), NAGP_EINVAL);
  for (d = 0; d < D; ++d) theta[(P - 1) * 3 * D + 2 * D + d] = -0.5;
  vary[P - 1] = 1e-4;
  EXPECT(nagp_pstft_timings(NULL), NAGP_EINVAL);
  EXPECT(nagp_pstft_timings(&ms), NAGP_OK);
  ms = -1.0;                                                             /* a refused call reports no time */
  EXPECT(STD(4, 1, D, N, N), NAGP_EUNSUPPORTED);
  EXPECT(nagp_pstft_timings(&ms), NAGP_OK);
  if (ms != 0.0) { fprintf(stderr, "nagp_pstft_timings after a refused call: %g, expected 0\n", ms); ++bad; }
  free(theta); free(spec); free(vary); free(bet); free(minVar); free(limOm); free(limLam); free(Obj); free(dObj); free(big);
  if (bad) { fprintf(stderr, "%d unexpected statuses\n", bad); return 1; }
  printf("all error paths returned their status\n");
  return 0;
}
