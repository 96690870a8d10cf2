/* abi_gppad_errors.c -- the argument-checking part of nagp_gppad_obj / nagp_gppad_create / nagp_gppad_eval under AddressSanitizer
 * (libnagp_asan.so: the host code of the C ABI instrumented), on a machine without a GPU: every refusal of include/nagp.h returns its
 * status before any device call, and nothing is read beyond the exactly-sized heap blocks the arguments live in.  The over-budget
 * refusal is reached through the developer switch NAGP_GPPAD_BUDGET_MB (read behind NAGP_DEVELOPER, which this program sets before its
 * first call into the library).  Built and run by tests/test_gppad_host.py. */
#define _POSIX_C_SOURCE 200112L
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "nagp.h"

#define EXPECT(call, code)                                                                         \
  do { int _s = (call); if (_s != (code)) { fprintf(stderr, "%s -> %d (%s), expected %d\n", #call, _s, nagp_last_error(), (code)); ++bad; } } while (0)

enum { P = 2, T = 5, TX = 8 };

static double* filled(size_t n, double v) {
  double* p = (double*)malloc(n * sizeof *p); size_t i;
  for (i = 0; i < n; ++i) p[i] = v;
  return p;
}

int main(void) {
  int bad = 0, k;
  double *x = filled(P * TX, 0.2), *y = filled(P * T, 0.7), *vary1 = filled(P, 0.0), *varyT = filled(P * T, 0.0), *len = filled(P, 3.0);
  double *cov1 = filled(TX, 0.5), *covP = filled(P * TX, 0.5), *varx = filled(P, 1.0), *mux = filled(P, -0.2), *varc = filled(P, 0.8);
  double *Obj = filled(P, 0.0), *dObj = filled(P * TX, 0.0), *wide, ms;
  double* three[3];
  nagp_gppad* h = (nagp_gppad*)&ms;                          /* must come back NULL from a refused create */
  const double bads[3] = {NAN, INFINITY, -INFINITY};
  setenv("NAGP_DEVELOPER", "1", 1);                          /* the library reads it once, at its first call */
#define CALL(n, t, tx, xx, yy, vy, vs, ln, cv, cs, vx, mu, vc, ob, dob) nagp_gppad_obj(n, t, tx, xx, yy, vy, vs, ln, cv, cs, vx, mu, vc, ob, dob, 0)
#define LEN(t, tx, vs) CALL(P, t, tx, x, y, (vs) ? varyT : vary1, vs, len, NULL, 0, varx, mux, varc, Obj, dObj)
#define COV(cs) CALL(P, T, TX, x, y, vary1, 0, NULL, (cs) ? covP : cov1, cs, varx, mux, varc, Obj, dObj)
  /* NULL arguments */
  EXPECT(CALL(P, T, TX, NULL, y, vary1, 0, len, NULL, 0, varx, mux, varc, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, T, TX, x, NULL, vary1, 0, len, NULL, 0, varx, mux, varc, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, T, TX, x, y, NULL, 0, len, NULL, 0, varx, mux, varc, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, T, TX, x, y, vary1, 0, len, NULL, 0, NULL, mux, varc, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, T, TX, x, y, vary1, 0, len, NULL, 0, varx, NULL, varc, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, T, TX, x, y, vary1, 0, len, NULL, 0, varx, mux, NULL, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, T, TX, x, y, vary1, 0, len, NULL, 0, varx, mux, varc, NULL, dObj), NAGP_EINVAL);
  /* both or neither of len and fftCov */
  EXPECT(CALL(P, T, TX, x, y, vary1, 0, NULL, NULL, 0, varx, mux, varc, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(P, T, TX, x, y, vary1, 0, len, cov1, 0, varx, mux, varc, Obj, dObj), NAGP_EINVAL);
  /* sizes and strides */
  EXPECT(CALL(0, T, TX, x, y, vary1, 0, len, NULL, 0, varx, mux, varc, Obj, dObj), NAGP_EINVAL);
  EXPECT(CALL(-1, T, TX, x, y, vary1, 0, len, NULL, 0, varx, mux, varc, Obj, dObj), NAGP_EINVAL);
  EXPECT(LEN(0, TX, 0), NAGP_EINVAL);                                              /* T < 1 */
  EXPECT(CALL(1, TX + 1, TX, x, y, vary1, 0, len, NULL, 0, varx, mux, varc, Obj, dObj), NAGP_EINVAL);   /* T > Tx (one problem: y holds 10 entries) */
  EXPECT(LEN(T, TX, 3), NAGP_EINVAL);                                              /* vary_stride neither 0 nor T */
  EXPECT(COV(4), NAGP_EINVAL);                                                     /* cov_stride neither 0 nor Tx */
  /* Tx: a power of two from 2 to 2^20 (refused on Tx alone: nothing is read) */
  EXPECT(LEN(1, 1, 0), NAGP_EUNSUPPORTED);
  EXPECT(LEN(T, 6, 0), NAGP_EUNSUPPORTED);
  EXPECT(LEN(T, 12, 0), NAGP_EUNSUPPORTED);
  EXPECT(LEN(T, (int64_t)1 << 21, 0), NAGP_EUNSUPPORTED);
  EXPECT(LEN(T, 0, 0), NAGP_EUNSUPPORTED);
  /* values: the last entry of each block */
  for (k = 0; k < 3; ++k) {
    y[P * T - 1] = bads[k];       EXPECT(LEN(T, TX, 0), NAGP_EINVAL); y[P * T - 1] = 0.7;
    vary1[P - 1] = bads[k];       EXPECT(LEN(T, TX, 0), NAGP_EINVAL); vary1[P - 1] = 0.0;
    varyT[P * T - 1] = bads[k];   EXPECT(LEN(T, TX, T), NAGP_EINVAL); varyT[P * T - 1] = 0.0;
    len[P - 1] = bads[k];         EXPECT(LEN(T, TX, 0), NAGP_EINVAL); len[P - 1] = 3.0;
    cov1[TX - 1] = bads[k];       EXPECT(COV(0), NAGP_EINVAL); cov1[TX - 1] = 0.5;
    covP[P * TX - 1] = bads[k];   EXPECT(COV(TX), NAGP_EINVAL); covP[P * TX - 1] = 0.5;
    varx[P - 1] = bads[k];        EXPECT(LEN(T, TX, 0), NAGP_EINVAL); varx[P - 1] = 1.0;
    mux[P - 1] = bads[k];         EXPECT(LEN(T, TX, 0), NAGP_EINVAL); mux[P - 1] = -0.2;
    varc[P - 1] = bads[k];        EXPECT(LEN(T, TX, 0), NAGP_EINVAL); varc[P - 1] = 0.8;
  }
  vary1[P - 1] = -1e-9;       EXPECT(LEN(T, TX, 0), NAGP_EINVAL); vary1[P - 1] = 0.0;
  varyT[P * T - 1] = -1e-9;   EXPECT(LEN(T, TX, T), NAGP_EINVAL); varyT[P * T - 1] = 0.0;
  three[0] = varx; three[1] = varc; three[2] = len;
  for (k = 0; k < 3; ++k) {                                                        /* varx, varc, len: > 0 */
    three[k][P - 1] = 0.0;    EXPECT(LEN(T, TX, 0), NAGP_EINVAL);
    three[k][P - 1] = -1.0;   EXPECT(LEN(T, TX, 0), NAGP_EINVAL); three[k][P - 1] = 1.0;
  }
  cov1[TX - 1] = 0.0;         EXPECT(COV(0), NAGP_EINVAL); cov1[TX - 1] = -0.5; EXPECT(COV(0), NAGP_EINVAL); cov1[TX - 1] = 0.5;
  covP[P * TX - 1] = 0.0;     EXPECT(COV(TX), NAGP_EINVAL); covP[P * TX - 1] = 0.5;
  /* the resident form: the same checks, and a handle that stays NULL */
  EXPECT(nagp_gppad_create(NULL, P, T, TX, y, vary1, 0, len, NULL, 0, varx, mux, varc, 0), NAGP_EINVAL);
  EXPECT(nagp_gppad_create(&h, P, T, TX, y, vary1, 0, NULL, NULL, 0, varx, mux, varc, 0), NAGP_EINVAL);
  if (h != NULL) { fprintf(stderr, "a refused create left a handle\n"); ++bad; }
  EXPECT(nagp_gppad_create(&h, P, T, 24, y, vary1, 0, len, NULL, 0, varx, mux, varc, 0), NAGP_EUNSUPPORTED);
  EXPECT(nagp_gppad_eval(NULL, x, Obj, dObj), NAGP_EINVAL);
  nagp_gppad_destroy(NULL);
  /* one problem beyond the budget of the per-evaluation buffers, lowered to 1 MiB: 8 * 4 * 65536 B at Tx = 65536 */
  wide = filled(65536, 0.5);
  setenv("NAGP_GPPAD_BUDGET_MB", "1", 1);
  EXPECT(CALL(1, T, 65536, wide, y, vary1, 0, len, NULL, 0, varx, mux, varc, Obj, NULL), NAGP_EUNSUPPORTED);
  unsetenv("NAGP_GPPAD_BUDGET_MB");
  free(wide);
  EXPECT(nagp_gppad_timings(NULL), NAGP_EINVAL);
  EXPECT(nagp_gppad_timings(&ms), NAGP_OK);
  free(x); free(y); free(vary1); free(varyT); free(len); free(cov1); free(covP); free(varx); free(mux); free(varc); free(Obj); free(dObj);
  if (bad) { fprintf(stderr, "%d unexpected statuses\n", bad); return 1; }
  printf("all error paths returned their status\n");
  return 0;
}
