/* abi_segp_errors.c -- the argument-checking part of nagp_segp_obj under AddressSanitizer (libnagp_asan.so: the host code of the C
 * ABI instrumented), on a machine without a GPU: every refusal of include/nagp.h returns its status before any device call, and
 * nothing is read beyond the exactly-sized heap blocks the arguments live in.  The over-budget refusal is reached through the developer
 * switch NAGP_SEGP_BUDGET_MB (read behind NAGP_DEVELOPER, which this program sets before its first call into the library).  Built and
 * run by tests/test_segp_host.py. */
#define _POSIX_C_SOURCE 200112L
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "nagp.h"

#define EXPECT(call, code)                                                                         \
  do { int _s = (call); if (_s != (code)) { fprintf(stderr, "%s -> %d (%s), expected %d\n", #call, _s, nagp_last_error(), (code)); ++bad; } } while (0)

enum { P = 2, T = 7 };

static double* filled(size_t n, double v) {
  double* p = (double*)malloc(n * sizeof *p); size_t i;
  for (i = 0; i < n; ++i) p[i] = v;
  return p;
}

int main(void) {
  int bad = 0, np;
  /* param blocks of exactly P x n_param entries, one per n_param */
  double *par[4] = {NULL, filled(P * 1, 0.5), filled(P * 2, 0.5), filled(P * 3, 0.5)};
  double *spec = filled(P * T, 1.5), *vary = filled(P, 0.1), *varx = filled(P, 1.0), *Obj = filled(P, 0.0), *dObj = filled(P * 3, 0.0);
  double ms;
  double *wide = NULL;
  setenv("NAGP_DEVELOPER", "1", 1);                          /* the library reads it once, at its first call */
#define CALL(n, k, t, pa, sp, st, vy, vx, ob, dob) nagp_segp_obj(n, k, t, pa, sp, st, vy, vx, ob, dob, 0)
#define STD(k, t, st) CALL(P, k, t, par[k], spec, st, vary, varx, Obj, dObj)
  EXPECT(CALL(P, 3, T, NULL, spec, T, vary, varx, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, 3, T, par[3], NULL, T, vary, varx, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, 3, T, par[3], spec, T, vary, varx, NULL, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, 2, T, par[2], spec, T, NULL, varx, Obj, dObj), NAGP_EINVAL);      /* vary is read with two parameters */
  EXPECT(CALL(P, 1, T, par[1], spec, T, NULL, varx, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, 1, T, par[1], spec, T, vary, NULL, Obj, dObj), NAGP_EINVAL);      /* varx is read with one */
  EXPECT(CALL(0, 3, T, par[3], spec, T, vary, varx, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(-1, 3, T, par[3], spec, T, vary, varx, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, 0, T, par[1], spec, T, vary, varx, Obj, dObj), NAGP_EINVAL);      /* refused on n_param alone: nothing is read */
  EXPECT(CALL(P, 4, T, par[3], spec, T, vary, varx, Obj, dObj), NAGP_EINVAL);
  EXPECT(STD(3, 1, 1), NAGP_EINVAL);                                               /* T < 2 */
  EXPECT(STD(3, T, 5), NAGP_EINVAL);                                               /* spec_stride neither 0 nor T */
  /* the last entry of each block */
  for (np = 1; np <= 3; ++np) {
    par[np][P * np - 1] = NAN;        EXPECT(STD(np, T, T), NAGP_EINVAL);
    par[np][P * np - 1] = -INFINITY;  EXPECT(STD(np, T, T), NAGP_EINVAL); par[np][P * np - 1] = 0.5;
  }
  spec[P * T - 1] = -1e-9;    EXPECT(STD(3, T, T), NAGP_EINVAL); spec[P * T - 1] = INFINITY; EXPECT(STD(2, T, T), NAGP_EINVAL);
  spec[P * T - 1] = NAN;      EXPECT(STD(1, T, T), NAGP_EINVAL); spec[P * T - 1] = 1.5;
  spec[T - 1] = -1.0;         EXPECT(STD(3, T, 0), NAGP_EINVAL); spec[T - 1] = 1.5;          /* shared: T entries are read */
  vary[P - 1] = 0.0;          EXPECT(STD(2, T, T), NAGP_EINVAL); vary[P - 1] = -0.1; EXPECT(STD(1, T, T), NAGP_EINVAL);
  vary[P - 1] = NAN;          EXPECT(STD(2, T, T), NAGP_EINVAL); vary[P - 1] = INFINITY; EXPECT(STD(1, T, 0), NAGP_EINVAL); vary[P - 1] = 0.1;
  varx[P - 1] = -1e-12;       EXPECT(STD(1, T, T), NAGP_EINVAL); varx[P - 1] = NAN; EXPECT(STD(1, T, T), NAGP_EINVAL); varx[P - 1] = 1.0;
  /* one problem beyond the device-memory budget, lowered to 1 MiB: 8 * 200 000 B of specy, shared or of the one problem */
  wide = filled(200000, 1.5);
  setenv("NAGP_SEGP_BUDGET_MB", "1", 1);
  EXPECT(CALL(1, 3, 200000, par[3], wide, 0, vary, varx, Obj, dObj), NAGP_EUNSUPPORTED);
  EXPECT(CALL(1, 1, 200000, par[1], wide, 200000, vary, varx, Obj, NULL), NAGP_EUNSUPPORTED);
  unsetenv("NAGP_SEGP_BUDGET_MB");
  free(wide);
  EXPECT(nagp_segp_timings(NULL), NAGP_EINVAL);
  EXPECT(nagp_segp_timings(&ms), NAGP_OK);
  free(par[1]); free(par[2]); free(par[3]); free(spec); free(vary); free(varx); free(Obj); free(dObj);
  if (bad) { fprintf(stderr, "%d unexpected statuses\n", bad); return 1; }
  printf("all error paths returned their status\n");
  return 0;
}
