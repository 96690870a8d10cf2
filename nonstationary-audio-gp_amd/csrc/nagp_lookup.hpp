// nagp_lookup.hpp -- the table look-up of the infinite-horizon filter in its straight-line form (three-barrier schedule of
// ihgp_adf8_kernel): [~,ind] = min(abs(r-R)) (ihgp_ep_modulator_nmf.m:131, :283) on the reference's grid logspace(-2,4,200), the first
// minimiser, non-finite R -> 0.  Same index as nearest_idx3 (nagp_ihgp.hpp) for every R.  Written on a pointer template and without any
// device intrinsic, so that a host program can call it (tests/test_ihgp_lookup_host.py).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define NAGP_LK_HD __host__ __device__ __forceinline__
#else
#define NAGP_LK_HD inline
#endif

namespace nagp {

// log10 to ~0.003 absolute (exponent + quadratic in the mantissa), as coarse_log10: only seeds the three-point window
NAGP_LK_HD double lookup_log10(double R) {
  unsigned long long u;
  __builtin_memcpy(&u, &R, 8);
  const int e = (int)((u >> 52) & 0x7ff) - 1023;
  const unsigned long long mu = (u & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
  double t;
  __builtin_memcpy(&t, &mu, 8);
  t -= 1.0;
  return ((double)e + t + 0.3466 * t * (1.0 - t)) * 0.30102999566398120;
}

// the R that leave the straight line: finite and beyond the grid (rounding ties between r[NG-1] and its neighbours: the first minimiser)
NAGP_LK_HD bool lookup_beyond(double rmax, double R) { return R > rmax && R < INFINITY; }
template <class P>
NAGP_LK_HD int lookup_tail(P r, int NG, double R) {
  const double dmin = fabs(r[NG - 1] - R);
  if (fabs(r[0] - R) == dmin) return 0;
  int i = NG - 1;
  while (i > 0 && fabs(r[i - 1] - R) == dmin) --i;
  return i;
}

// centre of the three-point window, 1 .. ng2 = NG - 2, by selects only.  R <= 0, NaN, +-Inf: 1 (the window then holds index 0, which
// lookup_pick3 returns for them: every distance is NaN or Inf, or the first one is the smallest).
NAGP_LK_HD int lookup_mid(int ng2, double lr0, double inv_dlr, double R) {
  double f = (lookup_log10(R) - lr0) * inv_dlr;
  f = (R > 0.0 && R < INFINITY) ? f : 0.0;
  f = fmin(fmax(f, 0.0), (double)(ng2 + 1));      // (est of nearest_idx3, before its rounding)
  const int est = (int)(f + 0.5);
  return est < 1 ? 1 : (est > ng2 ? ng2 : est);
}
// The same centre from ttau = 1 / R, so that the window can be read beside the division that forms R: the coarse log10 of ttau with its
// sign flipped.  The two estimates differ by at most twice the error of lookup_log10 (0.006 against a grid spacing of 0.030), and the
// first minimiser lies within 0.51 spacings of log10 R, so it stays inside mid - 1 .. mid + 1.  ttau below DBL_MIN (zero, the denormals, -0):
// 1.  There R is Inf (ttau <= 2^-1024: the window must hold index 0, while -log10 of a tiny ttau alone points at the other end of the
// grid) or finite and beyond the grid (lookup_beyond: the caller leaves through lookup_tail and does not use the window).  ttau = +Inf
// (R = 0): the estimate is below the grid, 1 as in lookup_mid.  The caller's ttau is never negative or NaN (max0).
// The chain is part of every step of the serial waves, so it is written in as few operations as it takes: lookup_log10's polynomial
// e + t + 0.3466 t (1 - t) as two fma, and -log10(2) inv_dlr and 0.5 - lr0 inv_dlr folded into one more (lookup_seed_consts, once per
// launch); fma everywhere, so that host and device round alike.  No clamp ahead of the conversion: |est| < 4e4 for every normal ttau.
NAGP_LK_HD void lookup_seed_consts(double lr0, double inv_dlr, double& c1, double& c0) {
  c1 = -0.30102999566398120 * inv_dlr; c0 = 0.5 - lr0 * inv_dlr;
}
NAGP_LK_HD int lookup_mid_ttau_c(int ng2, double c1, double c0, double ttau) {
  unsigned long long u;
  __builtin_memcpy(&u, &ttau, 8);
  const int e = (int)((u >> 52) & 0x7ff) - 1023;
  const unsigned long long mu = (u & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
  double t;
  __builtin_memcpy(&t, &mu, 8);
  t -= 1.0;
  const double l2 = fma(t, fma(t, -0.3466, 1.3466), (double)e);      // log2 ttau to ~0.01
  double g = fma(l2, c1, c0);                                        // (-log10 ttau - lr0) inv_dlr + 0.5
  g = (ttau >= 2.2250738585072014e-308) ? g : 0.5;
  const int est = (int)g;
  return est < 1 ? 1 : (est > ng2 ? ng2 : est);
}
NAGP_LK_HD int lookup_mid_ttau(int ng2, double lr0, double inv_dlr, double ttau) {
  double c1, c0;
  lookup_seed_consts(lr0, inv_dlr, c1, c0);
  return lookup_mid_ttau_c(ng2, c1, c0, ttau);
}
// 0, 1 or 2: the first minimiser of |r[mid - 1 + s] - R|
NAGP_LK_HD int lookup_pick3(double r0, double r1, double r2, double R) {
  const double d0 = fabs(r0 - R), d1 = fabs(r1 - R), d2 = fabs(r2 - R);
  int s = 0; double bd = d0;
  if (d1 < bd) { bd = d1; s = 1; }
  if (d2 < bd) s = 2;
  return s;
}

template <class P>
NAGP_LK_HD int nearest_idx3_sl(P r, int NG, double lr0, double inv_dlr, double rmax, double R) {
  if (lookup_beyond(rmax, R)) return lookup_tail(r, NG, R);
  const int mid = lookup_mid(NG - 2, lr0, inv_dlr, R);
  return mid - 1 + lookup_pick3(r[mid - 1], r[mid], r[mid + 1], R);
}
// the seeded order of ihgp_adf8_kernel's site update: window from ttau, then R = 1 / ttau decides the branch and picks.  Same index as
// nearest_idx3_sl(..., 1.0 / ttau) for every ttau >= 0 (tests/test_ihgp_lookup_seeded_host.py).
template <class P>
NAGP_LK_HD int nearest_idx3_seeded(P r, int NG, double lr0, double inv_dlr, double rmax, double ttau) {
  const int mid = lookup_mid_ttau(NG - 2, lr0, inv_dlr, ttau);
  const double r0 = r[mid - 1], r1 = r[mid], r2 = r[mid + 1];
  const double R = 1.0 / ttau;
  if (lookup_beyond(rmax, R)) return lookup_tail(r, NG, R);
  return mid - 1 + lookup_pick3(r0, r1, r2, R);
}

}  // namespace nagp
