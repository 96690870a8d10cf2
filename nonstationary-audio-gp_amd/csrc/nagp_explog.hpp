// nagp_explog.hpp -- exp and the softplus log of the three-barrier schedule of ihgp_adf8_kernel, written out.
// The device math library's f64 exp and log are straight-line code: a reduction, a Horner chain and a few selects for the special values.
// Inlined into the serial chains of the ADF step they cost more instructions than they hold arithmetic: the compiler takes the two-address
// FMA for every Horner step and copies the step's coefficient into its destination first (one 64-bit register copy per coefficient), and
// the selects cover arguments the call sites exclude.  The functions below perform the library's operations in the library's order -- the
// same reduction constants, coefficients and roundings, so the same bits on the stated domain -- with three-address FMAs in the Horner
// chains and only the selects the domain needs:
//   exp_le0(x)   x <= 0 or NaN          the Gaussian weights (argument -dy^2 / 2 sig2); the underflow to 0 stays
//   exp_any(x)   any x                  the link
//   log_ge1(x)   x in [1, +Inf] or NaN  the softplus link, x = 1 + exp(.)
// Nothing here is approximate: tests/test_explog_gpu.py counts differing bit patterns against exp() and log() and requires none.
// The constants are plain C++ (host-includable); the device functions exist under hipcc only.
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

#if defined(__HIPCC__)
// a * b + c, one rounding, as the three-address instruction: the destination is a register of its own, so no operand is copied to make
// room for the result
__device__ __forceinline__ double fma3(double a, double b, double c) {
  double r;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

// 2^n * (e^t), t and n = rint(x / ln2) of the reduction; no special values
__device__ __forceinline__ double exp_core(double x) {
#pragma clang fp contract(off)
  using namespace explog;
  const double dn = __builtin_rint(x * INV_LN2);
  double t = __builtin_fma(-dn, LN2_HI, x);
  t = __builtin_fma(-dn, LN2_LO, t);
  double p = fma3(t, EXP_C[0], EXP_C[1]);
#pragma unroll
  for (int i = 2; i < EXP_NC; ++i) p = fma3(t, p, EXP_C[i]);
  p = __builtin_fma(t, p, 1.0);
  p = __builtin_fma(t, p, 1.0);
  return __builtin_ldexp(p, (int)dn);
}
__device__ __forceinline__ double exp_le0(double x) {
  const double z = exp_core(x);
  return (x < explog::EXP_UNDER) ? 0.0 : z;
}
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
