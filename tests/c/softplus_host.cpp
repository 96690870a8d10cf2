// softplus_short of csrc/nagp_explog.hpp -- the text the device compiles -- on the host, against a reference of 64 mantissa bits
// (long double: max(z, 0) + log1pl(expl(-|z|))), beside today's form log(1 + exp(z)) evaluated in double against the same reference.
// Stand-alone (own main, no device, no library); built under -fsanitize=address,undefined by tests/test_softplus_host.py.
//   arguments z = x - shift, the subtraction in double as the kernel performs it, shifts 0 and 1:
//     x on a grid of 1 500 001 points over [-750, 750]; 1 000 001 points round 0, (i - 500 000) 2^-19; |z| = 2^k for every k in -1074 .. 1023,
//     both signs; the edges of the forms (the 1/2 split of log1p_01 at z = -ln 2, where exp(z) falls below 2^-53 and below the normal
//     range, the overflow of exp)
//   special values, asserted exactly: +Inf -> +Inf, -Inf -> 0, NaN -> NaN, the largest double -> itself, 0 -> ln 2
// An error is counted in ulps of the reference (a double's ulp at the reference's exponent, 2^-1074 at the least).  Prints
//   old form: <n> arguments, worst error <ulps> ulp at z = <z>; <m> arguments where it overflows and the softplus does not
//   new form: <n> arguments, worst error <ulps> ulp at z = <z>
// and returns 0 only if the new form's worst error is no larger than the old form's and below BOUND_ULP.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <vector>

#include "nagp_explog.hpp"

// 3 ulps, from the parts: t = exp_le0(.) is the device library's exp, 1 ulp by its documentation, so at most 2^-52 relative; an error of
// t reaches log(1 + t) scaled by t / ((1 + t) log(1 + t)) <= 1 relative to the result, and a relative 2^-52 is at most 2 ulps of the
// result (a result just above a power of two, t just below one).  log1p_01 adds the half ulp of its last addition and less than a tenth
// for the series, the remainder term and the two-term sums; for z > 0 the addition max(z, 0) + . adds its half ulp and shrinks the
// rest below one.  2 + 0.5 + 0.1 < 3.  (The library's exp is nearer half an ulp than one, so what the program prints is about half.)
static const double BOUND_ULP = 3.0;

static long double ref_softplus(double z) {
  const long double x = z;
  return fmaxl(x, 0.0L) + log1pl(expl(-fabsl(x)));
}
static double ulps(double got, long double ref) {
  if (std::isnan(got)) return HUGE_VAL;
  int e;
  frexpl(ref, &e);                                   // ref = m 2^e, m in [1/2, 1)
  int ue = e - 53;
  if (ue < -1074) ue = -1074;
  return (double)(fabsl((long double)got - ref) / ldexpl(1.0L, ue));
}

struct Worst { double err = 0.0, z = 0.0; long n = 0, overflow = 0; };
static void take(Worst& w, double got, long double ref, double z, bool count_overflow) {
  ++w.n;
  if (count_overflow && std::isinf(got) && !std::isinf((double)ref)) { ++w.overflow; return; }
  const double u = ulps(got, ref);
  if (u > w.err) { w.err = u; w.z = z; }
}

int main() {
  std::vector<double> args;
  const double shifts[2] = {0.0, 1.0};
  for (double shift : shifts) {
    for (long i = 0; i <= 1500000; ++i) args.push_back((-750.0 + 0.001 * (double)i) - shift);
    for (long i = 0; i <= 1000000; ++i) args.push_back(ldexp((double)(i - 500000), -19) - shift);
  }
  for (long i = 0; i <= 1000000; ++i) args.push_back(ldexp((double)(i - 500000), -19 - 20));      // 2^-39 apart round 0
  for (int k = -1074; k <= 1023; ++k) { args.push_back(ldexp(1.0, k)); args.push_back(-ldexp(1.0, k)); }
  const double edges[] = {-0.6931471805599453, -0.69314718055994529, -0.6931471805599454, 0.6931471805599453, -36.7368005696771, -36.8, -37.5,
                          -708.3964185322641, -708.4, -745.13321910194122, -745.2, -746.0, -1074.0, -1075.0, -1076.0, 709.782712893384, 709.7827128933841,
                          710.0, 745.2, 1024.0, 1e300, -1e300, DBL_MAX, -DBL_MAX, DBL_MIN, -DBL_MIN, 4.9e-324, -4.9e-324, 0.0, -0.0};
  for (double z : edges) for (int d = -2; d <= 2; ++d) {
    double v = z;
    for (int s = 0; s < (d < 0 ? -d : d); ++s) v = nextafter(v, d < 0 ? -HUGE_VAL : HUGE_VAL);
    if (std::isfinite(v)) args.push_back(v);
  }
  Worst wold, wnew;
  for (double z : args) {
    const long double ref = ref_softplus(z);
    take(wold, std::log(1.0 + std::exp(z)), ref, z, true);
    take(wnew, nagp::softplus_short(z), ref, z, false);
  }
  std::printf("old form: %ld arguments, worst error %.6g ulp at z = %.17g; %ld arguments where it overflows and the softplus does not\n", wold.n,
              wold.err, wold.z, wold.overflow);
  std::printf("new form: %ld arguments, worst error %.6g ulp at z = %.17g\n", wnew.n, wnew.err, wnew.z);
  int bad = 0;
  const double inf = HUGE_VAL, nan = std::nan("");
  if (nagp::softplus_short(inf) != inf) { std::printf("+Inf gives %g\n", nagp::softplus_short(inf)); ++bad; }
  if (nagp::softplus_short(-inf) != 0.0) { std::printf("-Inf gives %g\n", nagp::softplus_short(-inf)); ++bad; }
  if (!std::isnan(nagp::softplus_short(nan))) { std::printf("NaN gives %g\n", nagp::softplus_short(nan)); ++bad; }
  if (nagp::softplus_short(DBL_MAX) != DBL_MAX) { std::printf("the largest double gives %g\n", nagp::softplus_short(DBL_MAX)); ++bad; }
  if (nagp::softplus_short(0.0) != 0x1.62e42fefa39efp-1 || nagp::softplus_short(-0.0) != 0x1.62e42fefa39efp-1) { std::printf("0 gives %a\n", nagp::softplus_short(0.0)); ++bad; }
  if (!(wnew.err <= wold.err)) { std::printf("the new form's worst error exceeds the old form's\n"); ++bad; }
  if (!(wnew.err < BOUND_ULP)) { std::printf("the new form's worst error exceeds %g ulp\n", BOUND_ULP); ++bad; }
  if (bad) return 1;
  std::printf("softplus_short: special values exact, worst error within the old form's and %g ulp\n", BOUND_ULP);
  return 0;
}
