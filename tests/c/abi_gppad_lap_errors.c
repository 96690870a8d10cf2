/* abi_gppad_lap_errors.c -- the argument-checking part of nagp_gppad_lap_create and of the calls on its handle under AddressSanitizer
 * (libnagp_asan.so: the host code of the C ABI instrumented), on a machine without a GPU: every refusal of include/nagp.h that is
 * decided before a device call returns its status, and nothing is read beyond the exactly-sized heap blocks the arguments live in.  The
 * over-budget refusal is reached through the developer switch NAGP_GPPAD_BUDGET_MB (read behind NAGP_DEVELOPER, which this program sets
 * before its first call into the library).  Built and run by tests/test_gppad_lap_host.py. */
#define _POSIX_C_SOURCE 200112L
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "nagp.h"

#define EXPECT(call, code)                                                                         \
  do { int _s = (call); if (_s != (code)) { fprintf(stderr, "%s -> %d (%s), expected %d\n", #call, _s, nagp_last_error(), (code)); ++bad; } } while (0)

enum { P = 2, T = 5, TX = 8, JMAX = 4 };

static double* filled(size_t n, double v) {
  double* p = (double*)malloc(n * sizeof *p); size_t i;
  for (i = 0; i < n; ++i) p[i] = v;
  return p;
}

int main(void) {
  int bad = 0, k;
  double *y = filled(P * T, 0.7), *vary = filled(P, 0.1), *varyT = filled(P * T, 0.1), *len = filled(P, 3.0), *varx = filled(P, 1.0), *mux = filled(P, -0.2);
  double *varc = filled(P, 0.8), *x = filled(P * TX, 0.2), *out = filled(P * TX * JMAX, 0.0), ms;
  double* pos[3];
  int32_t nconv[P];
  nagp_gppad_lap* h = (nagp_gppad_lap*)&ms;                  /* must come back NULL from a refused create */
  const double bads[3] = {NAN, INFINITY, -INFINITY};
  setenv("NAGP_DEVELOPER", "1", 1);                          /* the library reads it once, at its first call */
#define CREATE(n, t, tx, yy, vy, vs, ln, vx, mu, vc, jm) nagp_gppad_lap_create(&h, n, t, tx, yy, vy, vs, ln, vx, mu, vc, jm, 0)
#define PLAIN(t, tx, jm) CREATE(P, t, tx, y, vary, 0, len, varx, mux, varc, jm)
  /* NULL arguments */
  EXPECT(nagp_gppad_lap_create(NULL, P, T, TX, y, vary, 0, len, varx, mux, varc, JMAX, 0), NAGP_EINVAL);
  EXPECT(CREATE(P, T, TX, NULL, vary, 0, len, varx, mux, varc, JMAX), NAGP_EINVAL);
  if (h != NULL) { fprintf(stderr, "a refused create left a handle\n"); ++bad; }
  EXPECT(CREATE(P, T, TX, y, NULL, 0, len, varx, mux, varc, JMAX), NAGP_EINVAL);
  EXPECT(CREATE(P, T, TX, y, vary, 0, NULL, varx, mux, varc, JMAX), NAGP_EINVAL);
  EXPECT(CREATE(P, T, TX, y, vary, 0, len, NULL, mux, varc, JMAX), NAGP_EINVAL);
  EXPECT(CREATE(P, T, TX, y, vary, 0, len, varx, NULL, varc, JMAX), NAGP_EINVAL);
  EXPECT(CREATE(P, T, TX, y, vary, 0, len, varx, mux, NULL, JMAX), NAGP_EINVAL);
  /* sizes and strides */
  EXPECT(CREATE(0, T, TX, y, vary, 0, len, varx, mux, varc, JMAX), NAGP_EINVAL);
  EXPECT(CREATE(-1, T, TX, y, vary, 0, len, varx, mux, varc, JMAX), NAGP_EINVAL);
  EXPECT(PLAIN(0, TX, JMAX), NAGP_EINVAL);                                         /* T < 1 */
  EXPECT(CREATE(1, TX + 1, TX, y, vary, 0, len, varx, mux, varc, JMAX), NAGP_EINVAL);   /* T > Tx (one problem: y holds 10 entries) */
  EXPECT(CREATE(P, T, TX, y, varyT, 3, len, varx, mux, varc, JMAX), NAGP_EINVAL);  /* vary_stride neither 0 nor T */
  EXPECT(PLAIN(T, TX, 0), NAGP_EINVAL);                                            /* jmax outside 1 .. min(Tx, 4096) */
  EXPECT(PLAIN(T, TX, TX + 1), NAGP_EINVAL);
  EXPECT(PLAIN(T, TX, -3), NAGP_EINVAL);
  /* Tx: a power of two from 2 to 2^20 (refused on Tx alone: nothing is read) */
  EXPECT(PLAIN(1, 1, 1), NAGP_EUNSUPPORTED);
  EXPECT(PLAIN(T, 6, JMAX), NAGP_EUNSUPPORTED);
  EXPECT(PLAIN(T, 12, JMAX), NAGP_EUNSUPPORTED);
  EXPECT(PLAIN(T, (int64_t)1 << 21, JMAX), NAGP_EUNSUPPORTED);
  EXPECT(PLAIN(T, 0, JMAX), NAGP_EUNSUPPORTED);
  /* values: the last entry of each block */
  for (k = 0; k < 3; ++k) {
    y[P * T - 1] = bads[k];      EXPECT(PLAIN(T, TX, JMAX), NAGP_EINVAL); y[P * T - 1] = 0.7;
    vary[P - 1] = bads[k];       EXPECT(PLAIN(T, TX, JMAX), NAGP_EINVAL); vary[P - 1] = 0.1;
    varyT[P * T - 1] = bads[k];  EXPECT(CREATE(P, T, TX, y, varyT, T, len, varx, mux, varc, JMAX), NAGP_EINVAL); varyT[P * T - 1] = 0.1;
    len[P - 1] = bads[k];        EXPECT(PLAIN(T, TX, JMAX), NAGP_EINVAL); len[P - 1] = 3.0;
    varx[P - 1] = bads[k];       EXPECT(PLAIN(T, TX, JMAX), NAGP_EINVAL); varx[P - 1] = 1.0;
    mux[P - 1] = bads[k];        EXPECT(PLAIN(T, TX, JMAX), NAGP_EINVAL); mux[P - 1] = -0.2;
    varc[P - 1] = bads[k];       EXPECT(PLAIN(T, TX, JMAX), NAGP_EINVAL); varc[P - 1] = 0.8;
  }
  vary[P - 1] = -0.1; EXPECT(PLAIN(T, TX, JMAX), NAGP_EINVAL); vary[P - 1] = 0.1;  /* vary >= 0 */
  pos[0] = varx; pos[1] = varc; pos[2] = len;
  for (k = 0; k < 3; ++k) {                                                        /* varx, varc, len: > 0 */
    pos[k][P - 1] = 0.0;    EXPECT(PLAIN(T, TX, JMAX), NAGP_EINVAL);
    pos[k][P - 1] = -1.0;   EXPECT(PLAIN(T, TX, JMAX), NAGP_EINVAL); pos[k][P - 1] = 1.0;
  }
  if (h != NULL) { fprintf(stderr, "a refused create left a handle\n"); ++bad; }
  /* the calls on a handle */
  EXPECT(nagp_gppad_lap_hess(NULL, x, NULL), NAGP_EINVAL);
  EXPECT(nagp_gppad_lap_apply(NULL, x, out), NAGP_EINVAL);
  EXPECT(nagp_gppad_lap_eig(NULL, 2, 1e-12, 1e-8, x, out, nconv, NULL, NULL, NULL), NAGP_EINVAL);
  EXPECT(nagp_gppad_lap_varx(NULL, 0, NULL, NULL, out, NULL), NAGP_EINVAL);
  EXPECT(nagp_gppad_lap_obj(NULL, out), NAGP_EINVAL);
  nagp_gppad_lap_destroy(NULL);
  /* one problem beyond the budget of the per-solve buffers, lowered to 1 MiB: 8 (2 x 4 + 2) x 16384 B of vectors alone at Tx = 16384, jmax = 4 */
  setenv("NAGP_GPPAD_BUDGET_MB", "1", 1);
  EXPECT(CREATE(1, T, 16384, y, vary, 0, len, varx, mux, varc, JMAX), NAGP_EUNSUPPORTED);
  unsetenv("NAGP_GPPAD_BUDGET_MB");
  EXPECT(nagp_gppad_lap_timings(NULL), NAGP_EINVAL);
  EXPECT(nagp_gppad_lap_timings(&ms), NAGP_OK);
  free(y); free(vary); free(varyT); free(len); free(varx); free(mux); free(varc); free(x); free(out);
  if (bad) { fprintf(stderr, "%d unexpected statuses\n", bad); return 1; }
  printf("all error paths returned their status\n");
  return 0;
}
