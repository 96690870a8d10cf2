/* abi_gppad_cas_errors.c -- the argument-checking part of nagp_gppad_cas_obj / nagp_gppad_cas_create / nagp_gppad_cas_eval under
 * AddressSanitizer (libnagp_asan.so: the host code of the C ABI instrumented), on a machine without a GPU: every refusal of
 * include/nagp.h returns its status before any device call, and nothing is read beyond the exactly-sized heap blocks the arguments
 * live in.  The over-budget refusal is reached through the developer switch NAGP_GPPAD_BUDGET_MB (read behind NAGP_DEVELOPER, which this
 * program sets before its first call into the library).  Built and run by tests/test_gppad_cas_host.py. */
#define _POSIX_C_SOURCE 200112L
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "nagp.h"

#define EXPECT(call, code)                                                                         \
  do { int _s = (call); if (_s != (code)) { fprintf(stderr, "%s -> %d (%s), expected %d\n", #call, _s, nagp_last_error(), (code)); ++bad; } } while (0)

enum { P = 2, M = 3, T = 5, TX = 8 };

static double* filled(size_t n, double v) {
  double* p = (double*)malloc(n * sizeof *p); size_t i;
  for (i = 0; i < n; ++i) p[i] = v;
  return p;
}

int main(void) {
  int bad = 0, k;
  double *x = filled(P * M * TX, 0.2), *y = filled(P * T, 0.7), *len = filled(P * M, 3.0);
  double *cov1 = filled(M * TX, 0.5), *covP = filled(P * M * TX, 0.5), *varx = filled(P * M, 1.0), *mux = filled(P * M, -0.2), *varc = filled(P, 0.8);
  double *Obj = filled(P, 0.0), *dObj = filled(P * M * TX, 0.0), *wide, ms;
  double* three[3];
  size_t last[3];
  nagp_gppad_cas* h = (nagp_gppad_cas*)&ms;                  /* must come back NULL from a refused create */
  const double bads[3] = {NAN, INFINITY, -INFINITY};
  setenv("NAGP_DEVELOPER", "1", 1);                          /* the library reads it once, at its first call */
#define CALL(n, m, t, tx, xx, yy, ln, cv, cs, vx, mu, vc, ob, dob) nagp_gppad_cas_obj(n, m, t, tx, xx, yy, ln, cv, cs, vx, mu, vc, ob, dob, 0)
#define LEN(m, t, tx) CALL(P, m, t, tx, x, y, len, NULL, 0, varx, mux, varc, Obj, dObj)
#define COV(cs) CALL(P, M, T, TX, x, y, NULL, (cs) ? covP : cov1, cs, varx, mux, varc, Obj, dObj)
  /* NULL arguments */
  EXPECT(CALL(P, M, T, TX, NULL, y, len, NULL, 0, varx, mux, varc, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, M, T, TX, x, NULL, len, NULL, 0, varx, mux, varc, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, M, T, TX, x, y, len, NULL, 0, NULL, mux, varc, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, M, T, TX, x, y, len, NULL, 0, varx, NULL, varc, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, M, T, TX, x, y, len, NULL, 0, varx, mux, NULL, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, M, T, TX, x, y, len, NULL, 0, varx, mux, varc, NULL, dObj), NAGP_EINVAL);
  /* both or neither of len and fftCovs */
  EXPECT(CALL(P, M, T, TX, x, y, NULL, NULL, 0, varx, mux, varc, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, M, T, TX, x, y, len, cov1, 0, varx, mux, varc, Obj, dObj), NAGP_EINVAL);
  /* sizes and strides */
  EXPECT(CALL(0, M, T, TX, x, y, len, NULL, 0, varx, mux, varc, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(-1, M, T, TX, x, y, len, NULL, 0, varx, mux, varc, Obj, dObj), NAGP_EINVAL);
  EXPECT(LEN(0, T, TX), NAGP_EUNSUPPORTED);                                        /* M outside 1 .. 8 (refused on M alone: nothing is read) */
  EXPECT(LEN(9, T, TX), NAGP_EUNSUPPORTED);
  EXPECT(LEN(-2, T, TX), NAGP_EUNSUPPORTED);
  EXPECT(LEN(M, 0, TX), NAGP_EINVAL);                                              /* T < 1 */
  EXPECT(CALL(1, M, TX + 1, TX, x, y, len, NULL, 0, varx, mux, varc, Obj, dObj), NAGP_EINVAL);   /* T > Tx (one cascade: y holds 10 entries) */
  EXPECT(COV(TX), NAGP_EINVAL);                                                    /* cov_stride neither 0 nor M Tx */
  /* Tx: a power of two from 2 to 2^20 (refused on Tx alone: nothing is read) */
  EXPECT(LEN(M, 1, 1), NAGP_EUNSUPPORTED);
  EXPECT(LEN(M, T, 6), NAGP_EUNSUPPORTED);
  EXPECT(LEN(M, T, 12), NAGP_EUNSUPPORTED);
  EXPECT(LEN(M, T, (int64_t)1 << 21), NAGP_EUNSUPPORTED);
  EXPECT(LEN(M, T, 0), NAGP_EUNSUPPORTED);
  /* values: the last entry of each block */
  for (k = 0; k < 3; ++k) {
    y[P * T - 1] = bads[k];           EXPECT(LEN(M, T, TX), NAGP_EINVAL); y[P * T - 1] = 0.7;
    len[P * M - 1] = bads[k];         EXPECT(LEN(M, T, TX), NAGP_EINVAL); len[P * M - 1] = 3.0;
    cov1[M * TX - 1] = bads[k];       EXPECT(COV(0), NAGP_EINVAL); cov1[M * TX - 1] = 0.5;
    covP[P * M * TX - 1] = bads[k];   EXPECT(COV(M * TX), NAGP_EINVAL); covP[P * M * TX - 1] = 0.5;
    varx[P * M - 1] = bads[k];        EXPECT(LEN(M, T, TX), NAGP_EINVAL); varx[P * M - 1] = 1.0;
    mux[P * M - 1] = bads[k];         EXPECT(LEN(M, T, TX), NAGP_EINVAL); mux[P * M - 1] = -0.2;
    varc[P - 1] = bads[k];            EXPECT(LEN(M, T, TX), NAGP_EINVAL); varc[P - 1] = 0.8;
  }
  three[0] = varx; three[1] = varc; three[2] = len; last[0] = P * M - 1; last[1] = P - 1; last[2] = P * M - 1;
  for (k = 0; k < 3; ++k) {                                                        /* varx, varc, len: > 0 */
    three[k][last[k]] = 0.0;    EXPECT(LEN(M, T, TX), NAGP_EINVAL);
    three[k][last[k]] = -1.0;   EXPECT(LEN(M, T, TX), NAGP_EINVAL); three[k][last[k]] = 1.0;
  }
  cov1[M * TX - 1] = 0.0;         EXPECT(COV(0), NAGP_EINVAL); cov1[M * TX - 1] = -0.5; EXPECT(COV(0), NAGP_EINVAL); cov1[M * TX - 1] = 0.5;
  covP[P * M * TX - 1] = 0.0;     EXPECT(COV(M * TX), NAGP_EINVAL); covP[P * M * TX - 1] = 0.5;
  /* the resident form: the same checks, and a handle that stays NULL */
  EXPECT(nagp_gppad_cas_create(NULL, P, M, T, TX, y, len, NULL, 0, varx, mux, varc, 0), NAGP_EINVAL);
  EXPECT(nagp_gppad_cas_create(&h, P, M, T, TX, y, NULL, NULL, 0, varx, mux, varc, 0), NAGP_EINVAL);
  if (h != NULL) { fprintf(stderr, "a refused create left a handle\n"); ++bad; }
  EXPECT(nagp_gppad_cas_create(&h, P, M, T, 24, y, len, NULL, 0, varx, mux, varc, 0), NAGP_EUNSUPPORTED);
  EXPECT(nagp_gppad_cas_create(&h, P, 9, T, TX, y, len, NULL, 0, varx, mux, varc, 0), NAGP_EUNSUPPORTED);
  EXPECT(nagp_gppad_cas_eval(NULL, x, Obj, dObj), NAGP_EINVAL);
  nagp_gppad_cas_destroy(NULL);
  /* one cascade beyond the budget of the per-evaluation buffers, lowered to 1 MiB: 8 * 4 * 65536 B at M = 1, Tx = 65536 */
  wide = filled(65536, 0.5);
  setenv("NAGP_GPPAD_BUDGET_MB", "1", 1);
  EXPECT(CALL(1, 1, T, 65536, wide, y, len, NULL, 0, varx, mux, varc, Obj, NULL), NAGP_EUNSUPPORTED);
  unsetenv("NAGP_GPPAD_BUDGET_MB");
  free(wide);
  EXPECT(nagp_gppad_cas_timings(NULL), NAGP_EINVAL);
  EXPECT(nagp_gppad_cas_timings(&ms), NAGP_OK);
  free(x); free(y); free(len); free(cov1); free(covP); free(varx); free(mux); free(varc); free(Obj); free(dObj);
  if (bad) { fprintf(stderr, "%d unexpected statuses\n", bad); return 1; }
  printf("all error paths returned their status\n");
  return 0;
}
