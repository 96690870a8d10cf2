// nagp_lookup.hpp -- the table look-up of the infinite-horizon filter in its straight-line form (three-barrier schedule of
// ihgp_adf8_kernel): [~,ind] = min(abs(r-R)) (ihgp_ep_modulator_nmf.m:131, :283) on the reference's grid logspace(-2,4,200), the first
// minimiser, non-finite R -> 0.  Same index as nearest_idx3 (nagp_ihgp.hpp) for every R.  Written on a pointer template and without any
// device intrinsic, so that a host program can call it (tests/test_ihgp_lookup_host.py).
#pragma once
#include <math.h>
#include <vector>

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
// (Since the look-up from ttau alone, below, the kernel's loop takes its centre from lookup_mid_bits; this seed remains the one of
// nearest_idx3_seeded, the oracle the threshold table is searched with.)
// The chain was part of every step of the serial waves, so it is written in as few operations as it takes: lookup_log10's polynomial
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

// ---- The same index from ttau alone (site update of ihgp_adf8_kernel): the exact division R = 1 / ttau leaves the chain to the look-up.
// Above t_beyond (the largest ttau whose fl(1 / ttau) satisfies lookup_beyond) the index is a non-increasing step function of ttau:
// fl(1 / t) is monotone in t, and inside the grid the differences r_i - R of neighbouring grid words are exact (Sterbenz), so the first
// minimiser is monotone in R.  Its NG - 1 steps tau_0 >= tau_1 >= .. (tau_i: the largest ttau whose index is at least i + 1) are found
// once per grid by bisection over the ordered doubles with nearest_idx3_seeded itself as the oracle (lookup_thresholds), and
//   index = #{ i : ttau <= tau_i } = mid - 1 + (ttau <= tau[mid - 1]) + (ttau <= tau[mid])          for a window mid - 1 .. mid + 1 that holds it.
// ttau <= t_inf (the largest ttau whose reciprocal rounds to Inf: zero and the smallest denormals): index 0.  t_inf < ttau <= t_beyond:
// finite R beyond the grid, where ties make the first minimiser non-monotone; the caller keeps lookup_tail on R there.
// The window's centre comes from the bit pattern of ttau by integer operations: the high word hi = exponent | 20 mantissa bits is
// piecewise linear in log2 ttau, hi / 2^20 - 1023 + c = log2 ttau +- 0.0431 with c centring the error of log2(1 + m) ~ m.  That is 0.43 steps of
// the reference's grid (0.1002 in log2); the first minimiser lies within 0.51 steps of the logarithmic position and the centre is rounded
// by 0.5 at most, so the window holds the index.  lookup_thresholds does not rely on that estimate: it checks the window at every step of
// either function, between which both are constant, and says so in its return value.
//   mid = med3((c0 - mulhi(hi, c1)) >> LOOKUP_SEED_SHIFT, 1, NG - 2)
#define NAGP_LOOKUP_SEED_SHIFT 8
NAGP_LK_HD int lookup_mid_bits(int ng2, unsigned int c1, int c0, double ttau) {
  unsigned long long u;
  __builtin_memcpy(&u, &ttau, 8);
  const unsigned int hi = (unsigned int)(u >> 32);
  const int est = (c0 - (int)(unsigned int)(((unsigned long long)hi * c1) >> 32)) >> NAGP_LOOKUP_SEED_SHIFT;
  return est < 1 ? 1 : (est > ng2 ? ng2 : est);
}
// 0, 1 or 2 from the two steps inside the window: ta = tau[mid - 1], tb = tau[mid]
NAGP_LK_HD int lookup_pick_thr(double ta, double tb, double ttau) { return (int)(ttau <= ta) + (int)(ttau <= tb); }

// what lookup_thresholds writes behind a grid of NG words: tau[NG - 1] | t_beyond | t_inf | c1 | c0 (the seed's two integers, as doubles)
NAGP_LK_HD int lookup_thr_doubles(int NG) { return NG + 3; }

// the order of ihgp_adf8_kernel's site update, ext = the table behind the grid: same index as nearest_idx3_seeded for every ttau >= 0
// (tests/test_ihgp_lookup_thresholds_host.py).  The straight path (ttau > t_beyond, or ttau <= t_inf) has no use for R.
template <class P>
NAGP_LK_HD int nearest_idx3_thr(P r, P ext, int NG, double ttau) {
  const double t_beyond = ext[NG - 1], t_inf = ext[NG];
  const int mid = lookup_mid_bits(NG - 2, (unsigned int)ext[NG + 1], (int)ext[NG + 2], ttau);
  int idx = mid - 1 + lookup_pick_thr(ext[mid - 1], ext[mid], ttau);
  idx = (ttau <= t_inf) ? 0 : idx;
  if (ttau <= t_beyond && ttau > t_inf) idx = lookup_tail(r, NG, 1.0 / ttau);
  return idx;
}

// ---- host only from here on (once per grid: the plan, nagp_api_plan.hpp)
inline double lookup_from_bits(unsigned long long u) { double x; __builtin_memcpy(&x, &u, 8); return x; }
inline unsigned long long lookup_to_bits(double x) { unsigned long long u; __builtin_memcpy(&u, &x, 8); return u; }
// the largest bit pattern in [lo, hi) at which pred holds; pred(lo) holds, pred(hi) does not, pred is monotone
template <class F>
inline unsigned long long lookup_bisect(unsigned long long lo, unsigned long long hi, F pred) {
  while (hi - lo > 1) {
    const unsigned long long m = lo + (hi - lo) / 2;
    if (pred(m)) lo = m; else hi = m;
  }
  return lo;
}
// the seed's integers for a grid: false when they do not fit their words (a grid finer than about 4000 words per octave)
inline bool lookup_seed_bits_consts(double lr0, double inv_dlr, unsigned int& c1, int& c0) {
  const double a = 0.30102999566398120 * inv_dlr;      // grid words per octave of ttau
  if (!(a > 0.0) || !(a < 2048.0) || !(fabs(lr0 * inv_dlr) < 1e6)) return false;
  const double one = (double)(1 << NAGP_LOOKUP_SEED_SHIFT);
  c1 = (unsigned int)floor(a * one * 4096.0 + 0.5);    // a 2^SHIFT 2^32 / 2^20
  const double z = ((1023.0 - 0.0430) * a - lr0 * inv_dlr + 0.5) * one;
  if (!(fabs(z) < 1.0e9)) return false;
  c0 = (int)floor(z + 0.5);
  return true;
}
// out[lookup_thr_doubles(NG)].  Returns true when the table is complete and the three-wide window of lookup_mid_bits holds the index for
// EVERY ttau above t_beyond; false (the caller must not run the threshold look-up) when the grid gives no such table: fewer than three
// words, not increasing, an index that does not span NG - 1 .. 0, or a window that misses.
template <class P>
inline bool lookup_thresholds(P r, int NG, double lr0, double inv_dlr, double* out) {
  for (int i = 0; i < lookup_thr_doubles(NG); ++i) out[i] = 0.0;
  if (NG < 3) return false;
  const double rmax = r[NG - 1];
  if (!(rmax > 0.0) || !(rmax < INFINITY)) return false;
  const unsigned long long b_one = lookup_to_bits(1.0), b_inf = lookup_to_bits(INFINITY);
  auto recip = [](unsigned long long u) { volatile double t = lookup_from_bits(u); return 1.0 / t; };      // the division the kernel performs
  auto index = [&](unsigned long long u) { volatile double t = lookup_from_bits(u); return nearest_idx3_seeded(r, NG, lr0, inv_dlr, rmax, t); };
  // t_inf, t_beyond: 1 / 0 = Inf > rmax; 1 / 1 is finite; 1 / Inf = 0 is not beyond
  const unsigned long long b_tinf = lookup_bisect(0ull, b_one, [&](unsigned long long u) { return !(recip(u) < INFINITY); });
  const unsigned long long b_tbey = lookup_bisect(b_tinf, b_inf, [&](unsigned long long u) { return recip(u) > rmax; });
  const unsigned long long b_lo = b_tbey + 1;          // the smallest ttau of the straight path
  if (b_lo >= b_inf || index(b_lo) != NG - 1 || index(b_inf) != 0) return false;
  unsigned long long hi = b_inf;
  std::vector<unsigned long long> tau((size_t)NG - 1);
  for (int i = 0; i < NG - 1; ++i) {                   // tau_i <= tau_(i-1): the search of step i ends where step i - 1 was found
    if (index(hi) >= i + 1) return false;
    tau[i] = lookup_bisect(b_lo, hi, [&](unsigned long long u) { return index(u) >= i + 1; });
    hi = tau[i] + 1;
    out[i] = lookup_from_bits(tau[i]);
  }
  out[NG - 1] = lookup_from_bits(b_tbey); out[NG] = lookup_from_bits(b_tinf);
  unsigned int c1; int c0;
  if (!lookup_seed_bits_consts(lr0, inv_dlr, c1, c0)) return false;
  out[NG + 1] = (double)c1; out[NG + 2] = (double)c0;
  // the window, at both sides of every step of the index and of the seed, and at the two ends of the straight path
  const int ng2 = NG - 2;
  auto seed = [&](unsigned long long u) { return lookup_mid_bits(ng2, c1, c0, lookup_from_bits(u)); };
  auto holds = [&](unsigned long long u) {
    if (u < b_lo || u > b_inf) return true;
    const double t = lookup_from_bits(u);
    int idx = 0;
    while (idx < NG - 1 && t <= out[idx]) ++idx;        // (tau is non-increasing: the count of steps at or above t)
    const int mid = seed(u);
    return idx >= mid - 1 && idx <= mid + 1 && idx == mid - 1 + lookup_pick_thr(out[mid - 1], out[mid], t);
  };
  if (!holds(b_lo) || !holds(b_inf)) return false;
  for (int i = 0; i < NG - 1; ++i)
    if (!holds(tau[i]) || !holds(tau[i] + 1)) return false;
  if (seed(b_lo) < seed(b_inf)) return false;
  for (int v = seed(b_inf) + 1; v <= seed(b_lo); ++v) {  // the largest ttau whose centre is at least v
    const unsigned long long s = lookup_bisect(b_lo, b_inf, [&](unsigned long long u) { return seed(u) >= v; });
    if (!holds(s) || !holds(s + 1)) return false;
  }
  return true;
}

}  // namespace nagp
