// nagp_explog.hpp -- exp and the softplus of the three-barrier schedule of ihgp_adf8_kernel, written out.
// The device math library's f64 exp and log are straight-line code: a reduction, a Horner chain and a few selects for the special values.
// Inlined into the serial chains of the ADF step they cost more instructions than they hold arithmetic: the compiler takes the two-address
// FMA for every Horner step and copies the step's coefficient into its destination first (one 64-bit register copy per coefficient), and
// the selects cover arguments the call sites exclude.  exp_le0, exp_any and log_ge1 perform the library's operations in the library's
// order -- the same reduction constants, coefficients and roundings, so the same bits on the stated domain -- with three-address FMAs in
// the Horner chains and only the selects the domain needs:
//   exp_le0(x)   x <= 0 or NaN          the Gaussian weights (argument -dy^2 / 2 sig2); the underflow to 0 stays
//   exp_any(x)   any x                  the link
//   log_ge1(x)   x in [1, +Inf] or NaN  x = 1 + exp(.): the softplus as link_eval writes it (no caller left in the product; kept as the
//                                       pinned restatement of the library's log, tests/test_explog_gpu.py)
// tests/test_explog_gpu.py counts differing bit patterns of these three against exp() and log() and requires none.
//   softplus_short(x)  any x            the softplus link of the serial chain (msr_link_serial): max(x, 0) + log1p_01(exp_le0(-|x|))
//   log1p_01(t)        t in [0, 1]      log(1 + t) without ever rounding 1 + t
// These two are NOT the bits of log(1 + exp(x)): they are closer to the true value (that form loses exp(x) against the 1 for x < 0 and
// overflows for x > 709.78).  tests/test_softplus_host.py measures both forms against an extended-precision reference, and
// tests/test_softplus_gpu.py requires the device's bits to be the host's: both compile the text below.
// The constants are plain C++; exp_le0, log1p_01 and softplus_short compile on the host as well (NAGP_XHD), the rest under hipcc only.
#pragma once

namespace nagp {
namespace explog {
// exp: x = n ln2 + t, n = rint(x / ln2), ln2 = LN2_HI + LN2_LO; e^t by a degree-12 polynomial, Horner from EXP_C[0] down to the two ones
constexpr double INV_LN2 = 0x1.71547652b82fep+0;
constexpr double LN2_HI = 0x1.62e42fefa39efp-1;
constexpr double LN2_LO = 0x1.abc9e3b39803fp-56;
constexpr int EXP_NC = 10;
constexpr double EXP_C[EXP_NC] = {0x1.ade156a5dcb37p-26, 0x1.28af3fca7ab0cp-22, 0x1.71dee623fde64p-19, 0x1.a01997c89e6b0p-16,
                                  0x1.a01a014761f6ep-13, 0x1.6c16c1852b7b0p-10, 0x1.1111111122322p-7,  0x1.55555555502a1p-5,
                                  0x1.5555555555511p-3,  0x1.000000000000bp-1};
constexpr double EXP_OVER = 1024.0;       // x > EXP_OVER: +Inf
constexpr double EXP_UNDER = -1075.0;     // x < EXP_UNDER: 0
// log: x = 2^e m, m in [2/3, 4/3); s = (m - 1) / (m + 1) in double-double; log m = 2 s + s^3 P(s^2), P by Horner from LOG_C[0]
constexpr double LOG_SPLIT = 0x1.5555555555555p-1;
constexpr int LOG_NC = 7;
constexpr double LOG_C[LOG_NC] = {0x1.3ab76bf559e2bp-3, 0x1.385386b47b09ap-3, 0x1.7474dd7f4df2ep-3, 0x1.c71c016291751p-3,
                                  0x1.249249b27acf1p-2, 0x1.99999998ef7b6p-2, 0x1.5555555555780p-1};
}  // namespace explog

// NAGP_XHD: a function of this file that the host compiles as well (under hipcc for both sides, under a plain C++ compiler for the host)
#if defined(__HIPCC__)
#define NAGP_XHD __host__ __device__ __forceinline__
#else
#define NAGP_XHD inline
#endif
// no contraction of a * b + c into an FMA the text does not write (first statement of a function body; the host tests compile with
// -ffp-contract=off as well)
#if defined(__clang__)
#define NAGP_FP_STRICT _Pragma("clang fp contract(off)")
#else
#define NAGP_FP_STRICT
#endif

// a * b + c, one rounding, as the three-address instruction: the destination is a register of its own, so no operand is copied to make
// room for the result
NAGP_XHD double fma3(double a, double b, double c) {
#if defined(__HIP_DEVICE_COMPILE__)
  double r;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
#else
  return __builtin_fma(a, b, c);
#endif
}
namespace explog {
// n of the reduction as an integer.  Where |x| is huge, infinite or NaN the conversion has no defined value in C++; exp's selects discard
// the result there, and the device's conversion instruction saturates.  The host takes 0 instead of stepping outside the language.
NAGP_XHD int exp_int(double dn) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (int)dn;
#else
  return (dn >= -4096.0 && dn <= 4096.0) ? (int)dn : 0;
#endif
}
// f / b, correctly rounded, for 1.75 <= b <= 2.5 and |f| <= 0.5: the division sequence of the compiler (hardware estimate, two Newton
// steps, quotient, one correction by its exact residual) without the scaling and the fix-up of the general case -- no operand here can
// make an intermediate overflow, and a residual that underflows belongs to b = 2, where every step is exact.  The host divides.
NAGP_XHD double div_b2(double f, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  double r = __builtin_amdgcn_rcp(b);
  r = __builtin_fma(__builtin_fma(-b, r, 1.0), r, r);
  r = __builtin_fma(__builtin_fma(-b, r, 1.0), r, r);
  const double q = f * r;
  return __builtin_fma(__builtin_fma(-b, q, f), r, q);
#else
  return f / b;
#endif
}
}  // namespace explog

// 2^n * (e^t), t and n = rint(x / ln2) of the reduction; no special values
NAGP_XHD double exp_core(double x) {
  NAGP_FP_STRICT
  using namespace explog;
  const double dn = __builtin_rint(x * INV_LN2);
  double t = __builtin_fma(-dn, LN2_HI, x);
  t = __builtin_fma(-dn, LN2_LO, t);
  double p = fma3(t, EXP_C[0], EXP_C[1]);
#if defined(__clang__)
#pragma unroll
#endif
  for (int i = 2; i < EXP_NC; ++i) p = fma3(t, p, EXP_C[i]);
  p = __builtin_fma(t, p, 1.0);
  p = __builtin_fma(t, p, 1.0);
  return __builtin_ldexp(p, exp_int(dn));
}
NAGP_XHD double exp_le0(double x) {
  const double z = exp_core(x);
  return (x < explog::EXP_UNDER) ? 0.0 : z;
}

// log(1 + t) for t in [0, 1] (NaN gives NaN).  1 + t = 2^e (1 + f) with e = 1, f = (t - 1) / 2 in [-1/4, 0] for t >= 1/2 and e = 0,
// f = t otherwise: f is exact either way -- 1 + t is never rounded, which is where log(1 + exp(x)) loses exp(x) for x < 0.
// log(1 + f) = 2 atanh(s), s = f / (2 + f) in [-1/7, 1/5]: the odd series 2 s + s^3 P(s^2) with the coefficients of the log above
// (fitted for |s| <= 1/5).  s = q + c: q the rounded quotient by b = fl(2 + f), c the first-order remainder from the quotient's exact
// residual and from bl = (2 + f) - b; 1 / (2 + f) ~ 1/2 - f/8 serves for c (c is below an ulp of q: three per cent of it are nothing).
// The result e ln2 + 2 q + (s^3 P + 2 c) is summed from its small end, 2 q against LN2_HI by an exact two-term sum (both zero for e = 0).
NAGP_XHD double log1p_01(double t) {
  NAGP_FP_STRICT
  using namespace explog;
  const bool hi = t >= 0.5;
  const double f = hi ? __builtin_fma(t, 0.5, -0.5) : t;
  const double kh = hi ? LN2_HI : 0.0, kl = hi ? LN2_LO : 0.0;
  const double b = 2.0 + f;
  const double bl = f - (b - 2.0);                   // b + bl = 2 + f exactly
  const double q = div_b2(f, b);
  double d = __builtin_fma(-q, b, f);
  d = __builtin_fma(-q, bl, d);                      // f - q (2 + f)
  const double c2 = d * __builtin_fma(f, -0.25, 1.0);      // 2 c
  const double s2 = q * q;
  double p = fma3(s2, LOG_C[0], LOG_C[1]);
#if defined(__clang__)
#pragma unroll
#endif
  for (int i = 2; i < LOG_NC; ++i) p = fma3(s2, p, LOG_C[i]);
  const double t1 = __builtin_fma(q * s2, p, c2);
  const double q2 = q + q;
  const double h = kh + q2;
  const double lo = (kh - h) + q2;                   // kh + q2 = h + lo exactly (|kh| >= |q2|, or kh = 0)
  return h + (lo + (t1 + kl));
}
// log(1 + e^x) = max(x, 0) + log(1 + e^-|x|), any x: +Inf gives +Inf, -Inf gives 0, NaN gives NaN (through the exp: max() drops it), and
// nothing overflows for large x.  Against an extended-precision reference its worst error is 1.5 ulp (tests/test_softplus_host.py prints
// the figure; most of it is the exp's own rounding, which counts double where t is just above a power of two and the result just below
// one), where log(1 + exp(x)) evaluated in double is off by 2^53 ulps once exp(x) < 2^-53.
NAGP_XHD double softplus_short(double x) {
  const double t = exp_le0(-__builtin_fabs(x));
  return __builtin_fmax(x, 0.0) + log1p_01(t);
}

#if defined(__HIPCC__)
__device__ __forceinline__ double exp_any(double x) {
  double z = exp_core(x);
  z = (x > explog::EXP_OVER) ? __builtin_inf() : z;
  return (x < explog::EXP_UNDER) ? 0.0 : z;
}

__device__ __forceinline__ double log_ge1(double x) {
#pragma clang fp contract(off)
  using namespace explog;
  double m = __builtin_amdgcn_frexp_mant(x);
  const bool lo = m < LOG_SPLIT;
  m = m * (lo ? 2.0 : 1.0);
  const int e = __builtin_amdgcn_frexp_exp(x) - (lo ? 1 : 0);
  // s = (m - 1) / (m + 1) as sh + sl
  const double a = m + -1.0, b = m + 1.0;
  const double bl = m - (b + -1.0);                  // b + bl = m + 1 exactly
  double r = __builtin_amdgcn_rcp(b);
  r = __builtin_fma(__builtin_fma(-b, r, 1.0), r, r);
  r = __builtin_fma(__builtin_fma(-b, r, 1.0), r, r);
  const double q = a * r;
  const double ph = b * q;
  double pl = __builtin_fma(q, b, -ph);
  pl = __builtin_fma(q, bl, pl);
  const double sh0 = ph + pl;
  const double sl0 = pl - (sh0 - ph);
  const double d = a - sh0;
  const double dl = ((a - d) - sh0) - sl0;
  const double c = r * (d + dl);
  const double sh = q + c;
  const double sl = c - (sh - q);
  // P(s^2)
  const double s2 = sh * sh;
  double p = fma3(s2, LOG_C[0], LOG_C[1]);
#pragma unroll
  for (int i = 2; i < LOG_NC; ++i) p = fma3(s2, p, LOG_C[i]);
  // log m = 2 s + s^3 P as (lh, ll)
  const double th = __builtin_ldexp(sh, 1), tl = __builtin_ldexp(sl, 1);
  const double u = (sh * s2) * p;
  const double v0 = th + u;
  const double v1 = tl + (u - (v0 - th));
  const double lh = v0 + v1;
  const double ll = v1 - (lh - v0);
  // e ln2 as (kh, kl)
  const double de = (double)e;
  const double k0 = de * LN2_HI;
  double k1 = __builtin_fma(de, LN2_HI, -k0);
  k1 = __builtin_fma(de, LN2_LO, k1);
  const double kh = k0 + k1;
  const double kl = k1 - (kh - k0);
  // (kh, kl) + (lh, ll)
  const double sa = kh + lh;
  const double sb = sa - kh;
  const double se = (lh - sb) + (kh - (sa - sb));
  const double ta = kl + ll;
  const double tb = ta - kl;
  const double te = (ll - tb) + (kl - (ta - tb));
  const double w0 = ta + se;
  const double w1 = sa + w0;
  const double w2 = te + (w0 - (w1 - sa));
  const double res = w1 + w2;
  return (x == __builtin_inf()) ? x : res;
}
#endif  // __HIPCC__
}  // namespace nagp
