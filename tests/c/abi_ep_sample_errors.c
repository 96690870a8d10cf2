/* abi_ep_sample_errors.c -- the argument-checking part of nagp_ep_sample under AddressSanitizer (libnagp_asan.so: the host code of
 * the C ABI instrumented), on a machine without a GPU: every refusal of include/nagp.h returns its status before any device call, and
 * nothing is read beyond the exactly-sized heap blocks the arguments live in.  The over-budget refusal is reached through the developer
 * switch NAGP_EPS_BUDGET_MB (read behind NAGP_DEVELOPER, which this program sets before its first call into the library).  Built and
 * run by tests/test_epsample_host.py. */
#define _POSIX_C_SOURCE 200112L
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "nagp.h"

#define EXPECT(call, code)                                                                         \
  do { int _s = (call); if (_s != (code)) { fprintf(stderr, "%s -> %d (%s), expected %d\n", #call, _s, nagp_last_error(), (code)); ++bad; } } while (0)

enum { S = 5, M = 3, D = 2, N = 1, T = 4, ND = 2 };

static double* filled(size_t n, double v) {
  double* p = (double*)malloc(n * sizeof *p); size_t i;
  for (i = 0; i < n; ++i) p[i] = v;
  return p;
}

int main(void) {
  int bad = 0, k, i;
  int32_t* off = (int32_t*)malloc((M + 1) * sizeof *off);
  int32_t* off9 = (int32_t*)malloc(2 * sizeof *off9);
  double *A = filled(S * S, 0.0), *Q = filled(S * S, 0.0), *Pinf = filled(S * S, 0.0), *hv = filled(M, 1.0), *W = filled(D * N, 0.3);
  double *A9 = filled(81, 0.0), *h9 = filled(1, 1.0);
  double *ttau = filled(M * T, 2.0), *tnu = filled(M * T, 0.1), *y = filled(T, 0.5);
  double *X = filled(ND * S * T, 0.0), *F = filled(ND * M * T, 0.0), *Sd = filled(ND * T, 0.0), *MS = filled(S * T, 0.0), ms[3];
  int64_t cnt[2] = {-1, -1};
  const double bads[3] = {NAN, INFINITY, -INFINITY};
  nagp_model md, m2;
  nagp_epsample_sig sg, s2;
  setenv("NAGP_DEVELOPER", "1", 1);                          /* the library reads it once, at its first call */
  off[0] = 0; off[1] = 2; off[2] = 4; off[3] = 5;
  for (i = 0; i < S; ++i) { A[i + i * S] = 0.9; Q[i + i * S] = 0.19; Pinf[i + i * S] = 1.0; }
  md.S = S; md.M = M; md.D = D; md.N = N; md.block_offsets = off; md.A = A; md.Q = Q; md.Pinf = Pinf; md.h_val = hv; md.Wnmf = W; md.lik_param = -9.0;
  sg.Wnmf = W; sg.amp_kind = NAGP_AMP_LINEAR; sg.link_kind = NAGP_LINK_SOFTPLUS; sg.link_shift = 0.0;
#define CALL(mdl, tt, tn, yy, t, nd, sig, x, f, sd, m) nagp_ep_sample(mdl, tt, tn, yy, t, 0, nd, 7, NULL, sig, x, f, sd, m, cnt, 0)
#define PLAIN(mdl) CALL(mdl, ttau, tnu, y, T, ND, &sg, X, F, Sd, MS)
  /* NULL arguments */
  EXPECT(CALL(NULL, ttau, tnu, y, T, ND, &sg, X, F, Sd, MS), NAGP_EINVAL);
  EXPECT(CALL(&md, NULL, tnu, y, T, ND, &sg, X, F, Sd, MS), NAGP_EINVAL);
  EXPECT(CALL(&md, ttau, NULL, y, T, ND, &sg, X, F, Sd, MS), NAGP_EINVAL);
  EXPECT(CALL(&md, ttau, tnu, NULL, T, ND, &sg, X, F, Sd, MS), NAGP_EINVAL);
  m2 = md; m2.block_offsets = NULL; EXPECT(PLAIN(&m2), NAGP_EINVAL);
  m2 = md; m2.A = NULL; EXPECT(PLAIN(&m2), NAGP_EINVAL);
  m2 = md; m2.Q = NULL; EXPECT(PLAIN(&m2), NAGP_EINVAL);
  m2 = md; m2.Pinf = NULL; EXPECT(PLAIN(&m2), NAGP_EINVAL);
  m2 = md; m2.h_val = NULL; EXPECT(PLAIN(&m2), NAGP_EINVAL);
  /* sizes */
  EXPECT(CALL(&md, ttau, tnu, y, 0, ND, &sg, X, F, Sd, MS), NAGP_EINVAL);
  EXPECT(CALL(&md, ttau, tnu, y, -3, ND, &sg, X, F, Sd, MS), NAGP_EINVAL);
  EXPECT(CALL(&md, ttau, tnu, y, T, 0, &sg, X, F, Sd, MS), NAGP_EINVAL);
  EXPECT(CALL(&md, ttau, tnu, y, T, -1, &sg, X, F, Sd, MS), NAGP_EINVAL);
  m2 = md; m2.S = 0; EXPECT(PLAIN(&m2), NAGP_EINVAL);
  m2 = md; m2.M = 0; EXPECT(PLAIN(&m2), NAGP_EINVAL);
  off[1] = 0; EXPECT(PLAIN(&md), NAGP_EINVAL); off[1] = 2;                      /* not strictly ascending */
  off[3] = 4; EXPECT(PLAIN(&md), NAGP_EINVAL); off[3] = 5;                      /* does not end at S */
  off[0] = 1; EXPECT(PLAIN(&md), NAGP_EINVAL); off[0] = 0;
  /* outputs and sig */
  EXPECT(CALL(&md, ttau, tnu, y, T, ND, &sg, NULL, NULL, NULL, NULL), NAGP_EINVAL);      /* no output at all */
  EXPECT(CALL(&md, ttau, tnu, y, T, ND, NULL, X, F, Sd, MS), NAGP_EINVAL);               /* Sdraw without sig */
  s2 = sg; s2.Wnmf = NULL; EXPECT(CALL(&md, ttau, tnu, y, T, ND, &s2, X, F, Sd, MS), NAGP_EINVAL);
  s2 = sg; s2.amp_kind = 2; EXPECT(CALL(&md, ttau, tnu, y, T, ND, &s2, X, F, Sd, MS), NAGP_EINVAL);
  s2 = sg; s2.link_kind = -1; EXPECT(CALL(&md, ttau, tnu, y, T, ND, &s2, X, F, Sd, MS), NAGP_EINVAL);
  s2 = sg; s2.link_shift = NAN; EXPECT(CALL(&md, ttau, tnu, y, T, ND, &s2, X, F, Sd, MS), NAGP_EINVAL);
  m2 = md; m2.D = 1; EXPECT(PLAIN(&m2), NAGP_EINVAL);                            /* D + N != M */
  W[D * N - 1] = NAN; EXPECT(PLAIN(&md), NAGP_EINVAL); W[D * N - 1] = 0.3;
  /* the sites: the last entry of each block */
  for (k = 0; k < 3; ++k) {
    ttau[M * T - 1] = bads[k]; EXPECT(PLAIN(&md), NAGP_EINVAL); ttau[M * T - 1] = 2.0;
    tnu[M * T - 1] = bads[k];  EXPECT(PLAIN(&md), NAGP_EINVAL); tnu[M * T - 1] = 0.1;
  }
  ttau[M * T - 1] = -1e-300; EXPECT(PLAIN(&md), NAGP_EINVAL); ttau[M * T - 1] = 2.0;
  /* shapes the kernels do not serve: a block of nine states; S = 81 (refused on the sizes alone: the 5 x 5 arrays are not read beyond) */
  off9[0] = 0; off9[1] = 9;
  m2 = md; m2.S = 9; m2.M = 1; m2.block_offsets = off9; m2.A = A9; m2.Q = A9; m2.Pinf = A9; m2.h_val = h9;
  EXPECT(CALL(&m2, ttau, tnu, y, T, ND, NULL, X, F, NULL, MS), NAGP_EUNSUPPORTED);
  {
    int32_t* off81 = (int32_t*)malloc(82 * sizeof *off81);
    for (i = 0; i <= 81; ++i) off81[i] = i;
    m2 = md; m2.S = 81; m2.M = 81; m2.block_offsets = off81;
    EXPECT(CALL(&m2, ttau, tnu, y, T, ND, NULL, X, F, NULL, MS), NAGP_EUNSUPPORTED);
    free(off81);
  }
  /* the per-step storage beyond the budget: 48 GiB as shipped (T = 2^28 at S = 5 takes 8 T 2 S^2 = 100 GiB), 1 MiB behind the switch */
  EXPECT(CALL(&md, ttau, tnu, y, (int64_t)1 << 28, ND, &sg, X, F, Sd, MS), NAGP_ENOMEM);
  setenv("NAGP_EPS_BUDGET_MB", "1", 1);
  EXPECT(CALL(&md, ttau, tnu, y, 4000, ND, &sg, X, F, Sd, MS), NAGP_ENOMEM);
  unsetenv("NAGP_EPS_BUDGET_MB");
  if (cnt[0] != -1 || cnt[1] != -1) { fprintf(stderr, "a refused call wrote the counters\n"); ++bad; }
  EXPECT(nagp_ep_sample_timings(NULL), NAGP_EINVAL);
  EXPECT(nagp_ep_sample_timings(ms), NAGP_OK);
  if (ms[0] != 0.0 || ms[1] != 0.0 || ms[2] != 0.0) { fprintf(stderr, "a refused call reports device time\n"); ++bad; }
  free(off); free(off9); free(A); free(Q); free(Pinf); free(hv); free(W); free(A9); free(h9); free(ttau); free(tnu); free(y);
  free(X); free(F); free(Sd); free(MS);
  if (bad) { fprintf(stderr, "%d unexpected statuses\n", bad); return 1; }
  printf("all error paths returned their status\n");
  return 0;
}
